"""The active set as a call of its own, and the adjoint and the tangent at a RECORDED point (qpg_batch_get_active_device, qpg_batch_adjoint_at_device,
qpg_batch_tangent_at_device / QpalmBatch.active_device, adjoint_device(at=...), tangent_device(at=...) / QPLayer(replay=True)).

References: tests/adjoint_refs.py and tests/tangent_refs.py (one solve of K(J) in numpy.longdouble, rational below 14 unknowns).  The rule is the one
tests/test_adjoint.py and tests/test_tangent.py apply: per case err64 = max |z_numpy - z_ref| / max |z_ref| of float64 numpy.linalg.solve on the same
system is measured, and the kernel's error, measured the same way, must stay within 8 x err64; the per-entry gradients, which are products of [u; w]
with the point, get the rounding term of those products on top.  Nothing is fixed in advance.

Sizes: the smallest at which these kernels change form -- (n, m) = (1, 2), (5, 8), (31, 62), (33, 16); nine members on four and on two factor slots (the
128-thread instance on the GPU, the work queue); a batch of mixed sizes; the sparse factor on a `blocks` pattern; n = 257 for the 512-thread instance;
scaling 0 and 10."""
import ctypes as C

import numpy as np
import pytest
import torch

from qpalm_amd import capi
from qpalm_amd.capi import QpgError
from qpalm_amd.solver import QpalmBatch
from qpalm_amd.torch_layer import QPLayer
from tests import adjoint_refs as R
from tests import tangent_refs as TR
from tests.sens_helpers import (INVALID, REFUSED, REFUSED_WORD, ST, UNSUPPORTED, N, T, adjoint_errors, assert_complementary, batch_direction, host, judge_adjoint,
                                judge_tangent, other_data, padded, point, refused_mode, small_batch, snapshot)
from tests.sparse_gadgets import blocks_qp

LD = R.LD
ADJ_KEYS = ("dq", "dbmin", "dbmax", "dQx", "dAx", "active", "flag", "resid", "passes")
TAN_KEYS = ("dx", "dy", "active", "flag", "resid", "passes")


# ---- the shapes of checks 1 and 2 --------------------------------------------------------------------------------------------------------------------
SHAPES = ["n1-m2-s10", "n1-m2-J0-s0", "n5-m8-s10", "n31-m62-s0", "n33-m16-s10", "B9-slots4", "B9-slots2", "mixed", "blocks-sparse", "n257-512threads",
          "one-unsolved"]


def build(ctx, shape):
    """(solved batch, [(QP, side, x*, y*)]) on the instance of the kernels the shape is there for; the caller restores sparse_factor"""
    st, warm, threads = dict(scaling=10), None, 256
    if shape.startswith("n") and shape != "n257-512threads":
        n, m, nact, scaling, sides = dict([("n1-m2-s10", (1, 2, 1, 10, "lower")), ("n1-m2-J0-s0", (1, 2, 0, 0, "mixed")), ("n5-m8-s10", (5, 8, 3, 10, "mixed")),
                                           ("n31-m62-s0", (31, 62, 12, 0, "mixed")), ("n33-m16-s10", (33, 16, 1, 10, "mixed"))])[shape]
        planted = [R.planted_qp(n, m, nact, 9000 + 7 * n + nact, sides=sides)]
        st = dict(scaling=scaling, proximal=1 if shape != "n1-m2-s10" else 0)
    elif shape == "n257-512threads":
        planted = [R.planted_qp(257, 130, 40, 9000 + 7 * 257 + 40)]
        warm, threads, st = (planted[0][2][None, :], planted[0][3][None, :]), 512, dict(scaling=0)
    elif shape in ("B9-slots4", "B9-slots2"):
        ctx.set_option("max_slots", 2 if shape == "B9-slots2" else 4)
        planted = [R.planted_qp(12, 20, 2 + k % 6, 9500 + 11 * k) for k in range(9)]
        threads = 128
    elif shape == "mixed":
        planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate([(33, 50, 20), (20, 30, 7), (5, 8, 3)])]
    elif shape == "blocks-sparse":
        ctx.set_option("sparse_factor", 1)
        planted = [R.replant(blocks_qp(43, 2)[0], 10, 60 + b) for b in range(2)]
        threads = 512
    elif shape == "one-unsolved":   # max_iter = 1: members 0 and 2 start at their planted solutions and end SOLVED at once, member 1 starts cold
        planted = [R.planted_qp(12, 20, 5, 9960 + b) for b in range(3)]
        wx, wy = np.array([q[2] for q in planted]), np.array([q[3] for q in planted])
        wx[1], wy[1] = 0.0, 0.0
        warm, st = (wx, wy), dict(scaling=10, max_iter=1)
    bt = QpalmBatch(ctx, [q[0] for q in planted], ctx.default_settings(**dict(ST, **st)))
    if warm is not None:
        bt.warm_start(*warm)
    bt.solve()
    if shape == "blocks-sparse":
        assert bt.sparse_info(0)[0] > 0
    assert bt.launch_shape()[1] == (threads if ctx.kind == "hip" else 128), bt.launch_shape()
    if shape == "B9-slots2":
        assert bt.B > bt.launch_shape()[0]                        # more members than factor slots: the work queue
    want = [1, -2, 1] if shape == "one-unsolved" else [1] * bt.B
    assert bt.statuses().tolist() == want
    return bt, planted


def cotangents(bt, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((bt.B, bt.n)), rng.standard_normal((bt.B, bt.m))


# ---- 1. active_device is the adjoint's active_out --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_active_device_equals_active_out(ctx, shape):
    try:
        bt, planted = build(ctx, shape)
        gx, gy = cotangents(bt)
        own = N(bt.adjoint_device(T(ctx, gx), T(ctx, gy), want=("active", "flag"))["active"])
        before = bt.epoch
        got = N(bt.active_device())
        assert bt.epoch == before
        assert got.dtype == np.int64 and np.array_equal(got, own)
        for b, (p, side, _, _) in enumerate(planted):
            if shape == "one-unsolved" and b == 1:
                assert np.all(got[b] == 0)                           # not SOLVED / DUAL_TERMINATED: all zeros
                continue
            assert np.array_equal(got[b, :p.m], side) and np.all(got[b, p.m:] == 0)   # (strictly complementary: the planted set)
        # the subset form: the rows of members that are not selected keep what the caller's array held
        sel = np.arange(bt.B) % 2
        mine = T(ctx, np.full((bt.B, bt.m), 7), np.int64)
        back = bt.active_device(out=mine, select=T(ctx, sel, np.int64))
        assert back is mine
        assert np.array_equal(N(mine)[sel == 1], own[sel == 1]) and np.all(N(mine)[sel == 0] == 7)
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 2. the stored point handed in: the same bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_same_state_same_bits(ctx, shape):
    try:
        bt, planted = build(ctx, shape)
        gx, gy = cotangents(bt)
        plain = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy)))
        at = point(bt)
        if shape == "one-unsolved":   # a point does not consult the status: the plain call's flag 2 has no counterpart, the member is left out
            sel = T(ctx, [1, 0, 1], np.int64)
            zeros = {k: torch.zeros_like(v) for k, v in bt.adjoint_device(T(ctx, gx), T(ctx, gy)).items()}
            mine = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=at, out=zeros, select=sel))
            plain["flag"][1] = 0
        else:
            mine = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=at))
        for k in ADJ_KEYS:
            assert np.array_equal(plain[k], mine[k]), k
        rng = np.random.default_rng(7)
        d = batch_direction(bt, [TR.direction(q[0], rng) for q in planted])
        d = {k: T(ctx, np.nan_to_num(v)) for k, v in d.items()}
        plain = host(bt.tangent_device(**d))
        if shape == "one-unsolved":
            zeros = {k: torch.zeros_like(v) for k, v in bt.tangent_device(**d).items()}
            mine = host(bt.tangent_device(**d, at=at, out=zeros, select=sel))
            plain["flag"][1] = 0
        else:
            mine = host(bt.tangent_device(**d, at=at))
        for k in TAN_KEYS:
            assert np.array_equal(plain[k], mine[k]), k
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 3. an earlier solve ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor", [0.0, 1e6])
def test_an_earlier_solve(ctx, floor):
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate([(33, 50, 20), (20, 30, 7), (5, 8, 3)])]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    bt.sens_penalty = floor
    bt.solve()
    P1 = point(bt)
    x1, y1, a1 = (N(t) for t in P1)
    for b, (p, side, _, _) in enumerate(planted):
        assert_complementary(p, side, x1[b, :p.n], y1[b, :p.m])
        assert np.array_equal(a1[b, :p.m], side)
    for which in (0, 1):
        nxt = other_data(planted, which, 700 + 10 * which)
        bt.update_q_device(T(ctx, padded([q[0].q for q in nxt], bt.n)))
        assert bt.update_bounds_device(T(ctx, padded([q[0].bmin for q in nxt], bt.m)), T(ctx, padded([q[0].bmax for q in nxt], bt.m))) == 0
        rc, _ = bt.step_device(warm="last")
        assert rc == 0 and bt.statuses().tolist() == [1, 1, 1]
        xs, ys = bt.solution()
        for b, (p2, s2, _, _) in enumerate(nxt):
            # on the CPU: this solve's active set is not J1 in any member -- the stored solution would not do
            assert np.any(s2 != planted[b][1])
            assert_complementary(p2, s2, xs[b, :p2.n], ys[b, :p2.m])
    rng = np.random.default_rng(5)
    gx, gy = rng.standard_normal((bt.B, bt.n)), rng.standard_normal((bt.B, bt.m))
    epoch = bt.epoch
    out = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=P1))
    dirs = [TR.direction(p, rng) for p in probs]
    tan = host(bt.tangent_device(**{k: T(ctx, v) for k, v in batch_direction(bt, dirs).items()}, at=P1))
    assert bt.epoch == epoch
    now = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy)))         # the plain call at this moment: the gradients of the THIRD solve
    for b, (p, side, _, _) in enumerate(planted):
        xb, yb = x1[b, :p.n], y1[b, :p.m]
        judge_adjoint(ctx, "adjoint P1[%d] floor %g" % (b, floor), p, side, xb, yb, gx[b, :p.n], gy[b, :p.m], out, b, tag="SENS-AT")
        judge_tangent(ctx, "tangent P1[%d] floor %g" % (b, floor), p, side, xb, yb, dirs[b], tan, b, tag="SENS-AT")
        _, _, err64, errk = adjoint_errors(p, side, gx[b, :p.n], gy[b, :p.m], now, b)
        print("SENS-AT | %s | the plain adjoint two solves later against P1[%d] | err64 %.2e | kernel %.2e" % (ctx.kind, b, err64, errk))
        assert int(now["flag"][b]) == 0 and errk > 8.0 * err64     # ... which are not P1's: the check discriminates
        assert not np.array_equal(now["active"][b, :p.m], side)


# ---- 4. state: the call neither reads nor moves what the next solve starts from ----------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,slots,warm", [("dense", 3, 512, "last"), ("dense", 5, 1, None), ("sparse", 2, 512, None), ("sparse", 3, 2, "last")])
def test_next_step_is_bit_identical(ctx, mode, B, slots, warm):
    ctx.set_option("max_slots", slots)
    if mode == "sparse":
        ctx.set_option("sparse_factor", 1)
    try:
        if mode == "sparse":
            probs = [R.replant(blocks_qp(43, 2)[0], 10, 60 + b)[0] for b in range(B)]
        else:
            probs = [R.planted_qp(12, 20, 5, 9900 + b)[0] for b in range(B)]
        st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
        H, G = (QpalmBatch(ctx, probs, ctx.default_settings(**st)) for _ in range(2))
        rng = np.random.default_rng(4)
        q2 = T(ctx, np.array([p.q for p in probs]) + 0.05 * rng.standard_normal((B, G.n)))
        q3 = T(ctx, np.array([p.q for p in probs]) + 0.05 * rng.standard_normal((B, G.n)))
        H.solve(); G.solve()
        assert (B > G.launch_shape()[0]) == (slots != 512)        # more members than factor slots: the work queue
        P1 = point(G)                                             # a valid point of another solve than the one the batch will hold
        for bt in (H, G):
            rc, _ = bt.step_device(q=q2, warm=warm)
            assert rc == 0
        before = snapshot(G)
        out = host(G.adjoint_device(T(ctx, rng.standard_normal((B, G.n))), T(ctx, rng.standard_normal((B, G.m))), at=P1))
        tan = host(G.tangent_device(dq=T(ctx, rng.standard_normal((B, G.n))), at=P1))
        assert np.all(out["flag"] == 0) and np.all(tan["flag"] == 0)
        after = snapshot(G)
        assert all(np.array_equal(before[k], after[k]) for k in before)       # nothing the caller can read has moved
        for bt in (H, G):
            rc, _ = bt.step_device(q=q3, warm=warm)
            assert rc == 0
        a, b = snapshot(H), snapshot(G)
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not bad, bad
        assert np.all(a["status_val"] == 1)
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 5. refusals and flags ------------------------------------------------------------------------------------------------------------------------------
def at_calls(ctx, bt, at):
    """the three new calls, each as a thunk"""
    gx = T(ctx, np.ones((bt.B, bt.n)))
    return [("active_device", lambda: bt.active_device()), ("adjoint at", lambda: bt.adjoint_device(gx, at=at)),
            ("tangent at", lambda: bt.tangent_device(dq=gx, at=at))]


def fake_point(ctx, bt):
    return T(ctx, np.zeros((bt.B, bt.n))), T(ctx, np.zeros((bt.B, bt.m))), T(ctx, np.zeros((bt.B, bt.m)), np.int64)


@pytest.mark.parametrize("which", REFUSED)
def test_unsupported_modes_are_refused(ctx, which):
    with refused_mode(ctx, which) as bt:
        for name, call in at_calls(ctx, bt, fake_point(ctx, bt)):
            with pytest.raises(QpgError) as e:
                call()
            assert e.value.code == UNSUPPORTED, name
            assert REFUSED_WORD[which] in str(e.value)


def test_invalid_calls(ctx):
    bt, planted = small_batch(ctx, B=2)
    L, h = bt.L, bt.h
    gx = T(ctx, np.ones((2, 12)))
    bt.iterate(1)                                            # a solve in progress
    for name, call in at_calls(ctx, bt, fake_point(ctx, bt)):
        with pytest.raises(QpgError) as e:
            call()
        assert e.value.code == INVALID and "in progress" in str(e.value), name
    bt.solve()
    P = point(bt)
    ref = host(bt.adjoint_device(gx, at=P))
    # at the C ABI: no output array; no point; a point with a field missing
    assert L.qpg_batch_get_active_device(h, None) == INVALID
    assert L.qpg_batch_get_active_subset_device(h, None, C.c_void_p(P[2].data_ptr()), None) == INVALID
    io = capi.DeviceAdjoint(gx=gx.data_ptr(), dq=T(ctx, np.zeros((2, 12))).data_ptr())
    tio = capi.DeviceTangent(dq=gx.data_ptr(), dx=T(ctx, np.zeros((2, 12))).data_ptr())
    full = dict(x=P[0].data_ptr(), y=P[1].data_ptr(), active=P[2].data_ptr())
    for fn, arg in ((L.qpg_batch_adjoint_at_device, io), (L.qpg_batch_tangent_at_device, tio)):
        assert fn(h, C.byref(arg), None, None, None) == INVALID
        for k in full:
            pt = capi.DevicePoint(**{j: v for j, v in full.items() if j != k})
            assert fn(h, C.byref(arg), C.byref(pt), None, None) == INVALID, k
        assert fn(h, C.byref(arg), C.byref(capi.DevicePoint(**full)), None, None) == 0
    assert L.qpg_batch_adjoint_at_device(h, C.byref(capi.DeviceAdjoint()), C.byref(capi.DevicePoint(**full)), None, None) == INVALID    # gx = NULL
    assert L.qpg_batch_tangent_at_device(h, C.byref(capi.DeviceTangent()), C.byref(capi.DevicePoint(**full)), None, None) == INVALID   # no direction
    # one source for J
    for call in (lambda: bt.adjoint_device(gx, active=P[2], at=P), lambda: bt.tangent_device(dq=gx, active=P[2], at=P)):
        with pytest.raises(QpgError) as e:
            call()
        assert e.value.code == INVALID and "active_in" in str(e.value)
    # an entry of the point's set outside {-1, 0, 1}
    bad = N(P[2]).copy()
    bad[1, 19] = 2
    for call in (lambda: bt.adjoint_device(gx, at=(P[0], P[1], T(ctx, bad, np.int64))), lambda: bt.tangent_device(dq=gx, at=(P[0], P[1], T(ctx, bad, np.int64)))):
        with pytest.raises(QpgError) as e:
            call()
        assert e.value.code == INVALID
    # a bad select
    with pytest.raises(QpgError) as e:
        bt.adjoint_device(gx, at=P, select=T(ctx, [1, 2], np.int64))
    assert e.value.code == INVALID
    # wrong type, dtype or shape of the point, a field missing: ValueError before anything is launched
    for at in ((P[0], P[1]), (P[0], P[1], None), (P[0].to(torch.float32), P[1], P[2]), (P[0], P[1], P[2].to(torch.int32)), (P[0], P[0], P[2]), "point"):
        with pytest.raises(ValueError):
            bt.adjoint_device(gx, at=at)
        with pytest.raises(ValueError):
            bt.tangent_device(dq=gx, at=at)
    with pytest.raises(ValueError):
        bt.active_device(out=T(ctx, np.zeros((2, 20)), np.int32))
    with pytest.raises(ValueError):
        bt.active_device(select=1)
    # ... and the batch still works: the same bits as before the refusals
    again = host(bt.adjoint_device(gx, at=P))
    for k in ADJ_KEYS:
        assert np.array_equal(again[k], ref[k]), k
    assert np.array_equal(N(bt.active_device()), N(P[2]))
    rc, _ = bt.step_device(warm="last")
    assert rc == 0 and bt.statuses().tolist() == [1, 1]


def test_before_setup(ctx):
    """a batch that was created and never set up: QPG_ERR_INVALID from all four entry points"""
    L = ctx.L
    h = C.c_void_p()
    st = ctx.default_settings(**ST)
    assert L.qpg_batch_create(ctx.h, 1, 2, 2, 4, 3, C.byref(st), C.byref(h)) == 0
    try:
        buf = T(ctx, np.zeros(8))
        ibuf = T(ctx, np.zeros(8), np.int64)
        pt = capi.DevicePoint(x=buf.data_ptr(), y=buf.data_ptr(), active=ibuf.data_ptr())
        assert L.qpg_batch_get_active_device(h, C.c_void_p(ibuf.data_ptr())) == INVALID
        assert L.qpg_batch_get_active_subset_device(h, C.c_void_p(ibuf.data_ptr()), C.c_void_p(ibuf.data_ptr()), None) == INVALID
        assert L.qpg_batch_adjoint_at_device(h, C.byref(capi.DeviceAdjoint(gx=buf.data_ptr())), C.byref(pt), None, None) == INVALID
        assert L.qpg_batch_tangent_at_device(h, C.byref(capi.DeviceTangent(dq=buf.data_ptr())), C.byref(pt), None, None) == INVALID
    finally:
        L.qpg_batch_destroy(h)


def test_a_point_that_is_not_finite(ctx):
    """a NaN inside one member's x: flag 1 and zeros for that member, its neighbours meet the rule; NaNs beyond a sized member's own n / m are never read"""
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate([(33, 50, 20), (20, 30, 7), (5, 8, 3)])]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    bt.solve()
    x, y, act = point(bt)
    rng = np.random.default_rng(9)
    gx, gy = rng.standard_normal((3, bt.n)), rng.standard_normal((3, bt.m))
    dirs = [TR.direction(p, rng) for p in probs]
    d = {k: T(ctx, v) for k, v in batch_direction(bt, dirs).items()}
    clean = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=(x, y, act)))
    clean_t = host(bt.tangent_device(**d, at=(x, y, act)))
    # beyond the members' own sizes: nothing changes
    xn, yn = N(x).copy(), N(y).copy()
    for b, p in enumerate(probs):
        xn[b, p.n:], yn[b, p.m:] = np.nan, np.nan
    assert np.isnan(xn).any() and np.isnan(yn).any()
    got = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=(T(ctx, xn), T(ctx, yn), act)))
    got_t = host(bt.tangent_device(**d, at=(T(ctx, xn), T(ctx, yn), act)))
    for k in ADJ_KEYS:
        assert np.array_equal(got[k], clean[k]), k
    for k in TAN_KEYS:
        assert np.array_equal(got_t[k], clean_t[k]), k
    # inside member 1: its x once, its y once
    for where in ("x", "y"):
        xb, yb = xn.copy(), yn.copy()
        (xb if where == "x" else yb)[1, 3] = np.nan if where == "x" else np.inf
        got = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=(T(ctx, xb), T(ctx, yb), act)))
        got_t = host(bt.tangent_device(**d, at=(T(ctx, xb), T(ctx, yb), act)))
        assert got["flag"].tolist() == [0, 1, 0] and got_t["flag"].tolist() == [0, 1, 0]
        for k in ("dq", "dbmin", "dbmax", "dQx", "dAx"):
            assert np.all(got[k][1] == 0), k
        assert np.all(got_t["dx"][1] == 0) and np.all(got_t["dy"][1] == 0)
        assert np.array_equal(got["active"][1], N(act)[1]) and np.array_equal(got_t["active"][1], N(act)[1])   # the set given
        for b in (0, 2):
            p, side, _, _ = planted[b]
            judge_adjoint(ctx, "adjoint NaN-neighbour[%d]" % b, p, side, N(x)[b, :p.n], N(y)[b, :p.m], gx[b, :p.n], gy[b, :p.m], got, b, tag="SENS-AT")
            judge_tangent(ctx, "tangent NaN-neighbour[%d]" % b, p, side, N(x)[b, :p.n], N(y)[b, :p.m], dirs[b], got_t, b, tag="SENS-AT")
            for k in ADJ_KEYS:
                assert np.array_equal(got[k][b], clean[k][b]), k


# ---- 6. a subset at a point ---------------------------------------------------------------------------------------------------------------------------
def test_subset_at_a_point(ctx):
    ctx.set_option("max_slots", 2)
    planted = [R.planted_qp(12, 20, 2 + k % 6, 9500 + 11 * k) for k in range(5)]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    bt.solve()
    P1 = point(bt)
    rc, _ = bt.step_device(q=T(ctx, np.array([p.q for p in probs]) + 0.3), warm="last")
    assert rc == 0
    gx, gy = cotangents(bt, 11)
    full = host(bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=P1))
    full_t = host(bt.tangent_device(dq=T(ctx, gx), dbmin=T(ctx, gy), at=P1))
    sel = np.array([1, 0, 0, 1, 1])
    mark = lambda ref: {k: torch.full_like(T(ctx, v, v.dtype), 7) for k, v in ref.items()}
    sub = bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=P1, out=mark(full), select=T(ctx, sel, np.int64))
    sub_t = bt.tangent_device(dq=T(ctx, gx), dbmin=T(ctx, gy), at=P1, out=mark(full_t), select=T(ctx, sel, np.int64))
    assert sub["n_selected"] == 3 and sub_t["n_selected"] == 3
    for ref, got, keys in ((full, host(sub), ADJ_KEYS), (full_t, host(sub_t), TAN_KEYS)):
        for k in keys:
            assert np.array_equal(got[k][sel == 1], ref[k][sel == 1]), k
            assert np.all(got[k][sel == 0] == 7), k
    # nothing selected: nothing is written, QPG_OK
    none = bt.adjoint_device(T(ctx, gx), T(ctx, gy), at=P1, out=mark(full), select=T(ctx, np.zeros(5), np.int64))
    assert none["n_selected"] == 0 and all(np.all(N(none[k]) == 7) for k in ADJ_KEYS)


# ---- 7. the layer: one backward through a rollout on ONE batch -------------------------------------------------------------------------------------------
def split_solve(p, side, r1, r2):
    """the reference solve of K(J) [u; w_J] = [r1; r2_J] for a longdouble right-hand side (head + tail, as tests/tangent_refs.py does), and float64
    numpy's on the head"""
    h1, h2 = r1.astype(np.float64), r2.astype(np.float64)
    t1, t2 = (r1 - h1).astype(np.float64), (r2 - h2).astype(np.float64)
    zh, z64, _ = R.reference(p, side, h1, h2)
    zt, _, _ = R.reference(p, side, t1, t2)
    return zh + zt, z64


def rollout_gradients(probs, pts, W, c, dtype):
    """d loss / d q0 [B][n] and d loss / d W [n][n] of loss = sum_t |x_t|^2 + <c, y_t>, q_1 = q0, q_{t+1} = q0 + W x_t, by the chain rule through the
    recorded points pts[t] = (x [B][n], y [B][m], side [B][m]); dtype longdouble: the reference solve, float64: numpy.linalg.solve"""
    B, n = len(probs), probs[0].n
    gq0, gW = np.zeros((B, n), dtype=dtype), np.zeros((n, n), dtype=dtype)
    Wd = W.astype(dtype)
    for b, p in enumerate(probs):
        gq_next = np.zeros(n, dtype=dtype)                     # d loss / d q_{t+1}
        for t in range(len(pts) - 1, -1, -1):
            x, y, side = (a[b] for a in pts[t])
            if t + 1 < len(pts):
                gW += np.outer(gq_next, x.astype(dtype))       # q_{t+1} = q0 + W x_t
            gx = 2 * x.astype(dtype) + Wd.T @ gq_next
            gy = c[b].astype(dtype)
            if dtype is np.float64:
                J = np.flatnonzero(side)
                z = np.linalg.solve(R.kkt_dense(p, J), np.concatenate([gx, gy[J]]))
            else:
                z, _ = split_solve(p, side, gx, gy)
            gq_next = -z[:n]
            gq0[b] += gq_next
    return gq0, gW


def rollout(layer, q0, W, c, steps=3):
    q, loss = q0, 0.0
    for _ in range(steps):
        x, y, status = layer(q)
        assert N(status).tolist() == [1] * q0.shape[0]
        loss = loss + (x * x).sum() + (c * y).sum()
        q = q0 + x @ W.T
    return loss


def test_layer_rollout(ctx):
    n, m, B = 5, 8, 3
    planted = [R.planted_qp(n, m, 3, 9300 + b) for b in range(B)]
    probs = [q[0] for q in planted]
    rng = np.random.default_rng(31)
    Wn, cn = 2.0 * rng.standard_normal((n, n)), rng.standard_normal((B, m))     # (a feedback strong enough to move the active sets along the rollout)
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    leaf = lambda a: T(ctx, a).requires_grad_(True)
    q0, W, c = leaf([p.q for p in probs]), leaf(Wn), T(ctx, cn)
    layer = QPLayer(bt, replay=True)
    q, loss, rec = q0, 0.0, []
    for t in range(3):
        x, y, status = layer(q)
        assert N(status).tolist() == [1] * B
        side = np.array([R.default_rule(bt, p, b) for b, p in enumerate(probs)])
        assert np.array_equal(N(bt.active_device()), side)        # the recorded set, restated in numpy
        rec.append((N(x).copy(), N(y).copy(), side))
        loss = loss + (x * x).sum() + (c * y).sum()
        q = q0 + x @ W.T
    loss.backward()
    assert N(layer.last_adjoint["flag"]).tolist() == [0] * B
    ref_q, ref_W = rollout_gradients(probs, rec, Wn, cn, LD)
    num_q, num_W = rollout_gradients(probs, rec, Wn, cn, np.float64)
    zr = np.concatenate([ref_q.ravel(), ref_W.ravel()])
    z64 = np.concatenate([num_q.ravel(), num_W.ravel()])
    zk = np.concatenate([N(q0.grad).ravel(), N(W.grad).ravel()])
    scale = float(np.max(np.abs(zr)))
    err64, errk = float(np.max(np.abs(z64 - zr))) / scale, float(np.max(np.abs(zk - zr))) / scale
    moved = sum(int(not np.array_equal(rec[t][2], rec[0][2])) for t in (1, 2))
    print("SENS-AT | %s | rollout T=3 B=3 | err64 %.2e | kernel %.2e | steps whose active sets differ from the first: %d" % (ctx.kind, err64, errk, moved))
    assert moved > 0                                              # the points differ in J: the batch's latest solve alone would not give these gradients
    assert err64 <= 1e-10 and errk <= 8.0 * err64, (errk, err64)
    # without replay the same rollout is refused at its first late backward (the existing rule)
    q0b, Wb = leaf([p.q for p in probs]), leaf(Wn)
    loss = rollout(QPLayer(bt), q0b, Wb, c)
    with pytest.raises(RuntimeError):
        loss.backward()
    # a replay backward after the values of Q and A have moved: the recorded points are no longer valid
    q0c, Wc = leaf([p.q for p in probs]), leaf(Wn)
    loss = rollout(layer, q0c, Wc, c)
    epoch = bt.matrix_epoch
    Qx, Ax = T(ctx, padded([p.Qx for p in probs], bt.nnzQ)), T(ctx, padded([p.Ax for p in probs], bt.nnzA))
    bt.update_Q_A_device(Qx.data_ptr(), Ax.data_ptr())
    assert bt.matrix_epoch == epoch + 1
    with pytest.raises(RuntimeError):
        loss.backward()

"""The tangent of a solved batch (qpg_batch_tangent_device / QpalmBatch.tangent_device / forward-mode AD through qpalm_amd.torch_layer).

Reference: tests/tangent_refs.py -- the right-hand side r1 = -(dq + dQ x + dA' y), r2 = db_J - (dA x)_J in numpy.longdouble from the problem's own data and
the direction in the caller's entry order, then the solve of tests/adjoint_refs.py (exact in rationals below 14 unknowns).  The engine supplies x and y
and is handed the planted J.

Tolerance: nothing fixed in advance, the rule of tests/test_adjoint.py.  Per case err64 = max |z_numpy - z_ref| / max |z_ref| of float64
numpy.linalg.solve on the same K and right-hand side is measured, and the kernel's [dx; dy_J], measured the same way, must stay within 8 x err64.
Measured figures (both backends): profiles/tangent/accuracy.md.

The duality checks pair the tangent with the adjoint: <g, z_tan> = <adjoint gradients of g, direction> holds exactly in exact arithmetic (K is symmetric
and both use the stored y of every row); what float64 may lose is err64_T scale_T ||g||_1 + err64_A scale_A ||direction||_1, each err64 measured."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest
import torch

from qpalm_amd import capi
from qpalm_amd.capi import QpgError
from qpalm_amd.solver import QpalmBatch
from qpalm_amd.torch_layer import QPLayer, _QPFunction
from tests import adjoint_refs as R
from tests import tangent_refs as TR
from tests.sparse_gadgets import blocks_qp, gadget_qp
from tests.sens_helpers import (INVALID, REFUSED, REFUSED_WORD, ST, UNSUPPORTED, N, T, assert_complementary, assert_instance, batch_direction, padded,
                                refused_mode, run_tangent, small_batch, snapshot, solved)
from tests.sens_helpers import judge_tangent as judge
from tests.sens_helpers import tangent_measure as measure

LD = R.LD
OUT = ("dx", "dy", "active", "flag", "resid", "passes")


# ---- 0. the reference itself, without a backend: duality with the adjoint's reference ------------------------------------------------------------
@pytest.mark.parametrize("n,m,nact,equality", [(5, 8, 3, False), (12, 20, 5, False), (33, 50, 20, False), (20, 30, 9, True)])
def test_reference_is_dual_to_the_adjoint_reference(n, m, nact, equality):
    p, side, x, y = R.planted_qp(n, m, nact, 8100 + n, equality=equality)
    p = R.shuffled_entries(p, 5) if n == 12 else p               # once with upper entries of Q and unsorted columns
    rng = np.random.default_rng(n)
    y = y + np.where(side == 0, 0.1 * rng.standard_normal(m), 0.0)    # (any y: the identity needs the unmasked y on both sides)
    d = TR.direction(p, rng)
    gx, gy = rng.standard_normal(n), rng.standard_normal(m)
    zt, J, scale_t, err_t = measure(p, side, x, y, d)
    za, z64a, _ = R.reference(p, side, gx, gy)
    scale_a = float(np.max(np.abs(za)))
    err_a = float(np.max(np.abs(z64a - za))) / scale_a
    lhs = np.asarray(gx, dtype=LD) @ zt[:n] + np.asarray(gy[J], dtype=LD) @ zt[n:]
    rhs = TR.pairing(d, R.gradients(p, side, x.astype(LD), y.astype(LD), za))
    bound = err_t * scale_t * (np.sum(np.abs(gx)) + np.sum(np.abs(gy[J]))) + err_a * scale_a * TR.norm1(d)
    print("TANGENT-REF | n=%d m=%d |J|=%d | <g, z_tan> %.15e | <adjoint, d> %.15e | gap %.2e | float64 slack %.2e" %
          (n, m, len(J), float(lhs), float(rhs), float(abs(lhs - rhs)), bound))
    assert abs(lhs - rhs) <= bound
    assert bound <= 1e-9 * max(1.0, abs(float(lhs)))             # (a wrong formula misses by O(1))


# ---- 1. sizes where a form changes ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    m: int
    nact: int
    scaling: int
    proximal: int
    sides: str = "mixed"
    equality: bool = False

    @property
    def id(self):
        return "n%d-m%d-J%d%s-s%d-p%d" % (self.n, self.m, self.nact, "eq" if self.equality else "", self.scaling, self.proximal)


CASES = [Case(1, 2, 1, 10, 0, sides="lower"), Case(1, 2, 0, 0, 1), Case(5, 8, 3, 10, 1), Case(33, 16, 1, 10, 1), Case(64, 128, 63, 10, 0, equality=True),
         Case(65, 32, 20, 10, 0), Case(193, 386, 90, 10, 1), Case(257, 514, 256, 0, 1, equality=True)]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_tangent_matches_the_reference_solve(ctx, case):
    p, side, xs, ys = R.planted_qp(case.n, case.m, case.nact, 9000 + 7 * case.n + case.nact, sides=case.sides, equality=case.equality)
    warm = (xs[None, :], ys[None, :]) if case.n >= 192 else None
    bt = solved(ctx, [p], warm=warm, scaling=case.scaling, proximal=case.proximal)
    assert int(bt.info(0).status_val) == 1
    assert_instance(ctx, bt, 256 if case.n <= 256 else 512)
    x, y = bt.solution_of(0)
    assert_complementary(p, side, x, y)
    d = TR.direction(p, np.random.default_rng(case.n))
    out = run_tangent(ctx, bt, batch_direction(bt, [d]), side[None, :])
    judge(ctx, case.id, p, side, x, y, d, out)


# ---- 2. each input alone and all together; NULL = zero, bit for bit --------------------------------------------------------------------------------
ALONE = [("dq",), ("dbmin", "dbmax"), ("dAx",), ("dQx",), TR.KEYS]


@pytest.mark.parametrize("n,m,nact", [(5, 8, 3), (65, 32, 20)])
def test_each_input_alone(ctx, n, m, nact):
    p, side, _, _ = R.planted_qp(n, m, nact, 9000 + 7 * n + nact)
    bt = solved(ctx, [p], scaling=10)
    x, y = bt.solution_of(0)
    assert_complementary(p, side, x, y)
    full = TR.direction(p, np.random.default_rng(n + 1))
    for keys in ALONE:
        d = {k: full[k] for k in keys}
        out = run_tangent(ctx, bt, batch_direction(bt, [d]), side[None, :])
        judge(ctx, "n%d-%s" % (n, "+".join(keys)), p, side, x, y, d, out)
        zeros = {k: (full[k] if k in keys else np.zeros_like(full[k])) for k in TR.KEYS}
        explicit = run_tangent(ctx, bt, batch_direction(bt, [zeros]), side[None, :])
        for k in OUT:
            assert np.array_equal(out[k], explicit[k]), (keys, k)


# ---- 3. the caller's order of the entries ----------------------------------------------------------------------------------------------------------
def test_entries_in_the_callers_order(ctx):
    base, side, _, _ = R.planted_qp(12, 20, 5, 9600)
    same, side1, _, _ = R.planted_qp(12, 20, 4, 9601)
    p = R.shuffled_entries(base, 3)
    cq = np.repeat(np.arange(12), np.diff(p.Qp))
    upper = p.Qi < cq
    assert np.any(upper) and np.any(np.diff(p.Ai)[np.diff(np.repeat(np.arange(12), np.diff(p.Ap))) == 0] < 0)
    probs, sides = [p, same], np.array([side, side1])             # member 1 in the engine's own order: no map for it, the "same order" flag
    bt = solved(ctx, probs, scaling=10)
    assert bt.nnzQ == len(p.Qx) > len(base.Qx)
    rng = np.random.default_rng(6)
    dirs = [TR.direction(q, rng) for q in probs]
    out = run_tangent(ctx, bt, batch_direction(bt, dirs), sides)
    for b, q in enumerate(probs):
        x, y = bt.solution_of(b)
        assert_complementary(q, sides[b], x, y)
        judge(ctx, "order[%d]" % b, q, sides[b], x, y, dirs[b], out, b)   # the direction position by position in q's own arrays
    # what sits in the upper-triangle positions of dQx is not part of the direction
    moved = dict(dirs[0], dQx=np.where(upper, 1e3 * rng.standard_normal(len(p.Qx)), dirs[0]["dQx"]))
    again = run_tangent(ctx, bt, batch_direction(bt, [moved, dirs[1]]), sides)
    for k in OUT:
        assert np.array_equal(out[k], again[k]), k
    lower = dict(dirs[0], dQx=np.where(~upper & (p.Qi > cq), dirs[0]["dQx"] + 1.0, dirs[0]["dQx"]))
    assert not np.array_equal(run_tangent(ctx, bt, batch_direction(bt, [lower, dirs[1]]), sides)["dx"][0], out["dx"][0])


# ---- 4. a direction on inactive rows only ----------------------------------------------------------------------------------------------------------
def test_direction_on_inactive_rows_only(ctx):
    n, m = 33, 50
    p, side, xs, ys = R.planted_qp(n, m, 20, 9700)
    bt = solved(ctx, [p], warm=(xs[None, :], ys[None, :]), scaling=10)   # from the planted solution: y starts at 0 on the inactive rows and stays there
    x, y = bt.solution_of(0)
    assert_complementary(p, side, x, y)
    rng = np.random.default_rng(14)
    off = side == 0
    d = dict(dbmin=np.where(off, rng.standard_normal(m), 0.0), dbmax=np.where(off, rng.standard_normal(m), 0.0))
    exact = bool(np.all(y[off] == 0))                                # the unmasked y term dA' y vanishes only where the stored y is exactly 0
    if exact:
        d["dAx"] = np.where(off[p.Ai], rng.standard_normal(len(p.Ax)), 0.0)
    print("TANGENT-INACTIVE | %s | stored y exactly 0 on the inactive rows: %s (dA rows %s)" % (ctx.kind, exact, "included" if exact else "left out"))
    out = run_tangent(ctx, bt, batch_direction(bt, [d]), side[None, :])
    assert int(out["flag"][0]) == 0
    assert np.all(out["dx"] == 0) and np.all(out["dy"] == 0)
    # with the engine's own rule for J as well
    own = run_tangent(ctx, bt, batch_direction(bt, [d]), None)
    assert np.array_equal(own["active"][0], side) and np.all(own["dx"] == 0) and np.all(own["dy"] == 0)


# ---- 5. an equality row: only dbmin is read -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [True, False])
def test_equality_rows_read_dbmin_only(ctx, given):
    p, side, _, _ = R.planted_qp(12, 20, 5, 9710, equality=True)
    eq = p.bmin == p.bmax
    assert np.array_equal(eq, side != 0) and np.all(side[eq] == -1)
    bt = solved(ctx, [p], scaling=10)
    x, y = bt.solution_of(0)
    d = TR.direction(p, np.random.default_rng(15), keys=("dq", "dbmin", "dbmax"))
    sides = side[None, :] if given else None
    out = run_tangent(ctx, bt, batch_direction(bt, [d]), sides)
    judge(ctx, "equality-%s" % ("given" if given else "rule"), p, side, x, y, d, out)
    other = dict(d, dbmax=np.where(eq, d["dbmax"] + 7.0, d["dbmax"]))
    again = run_tangent(ctx, bt, batch_direction(bt, [other]), sides)
    for k in OUT:
        assert np.array_equal(out[k], again[k]), k
    lower = dict(d, dbmin=np.where(eq, d["dbmin"] + 7.0, d["dbmin"]))
    assert not np.array_equal(run_tangent(ctx, bt, batch_direction(bt, [lower]), sides)["dx"], out["dx"])


# ---- 6. batch shapes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["mixed", "B9-slots4", "B9-slots2"])
def test_batches(ctx, shape):
    if shape == "mixed":
        dims = [(33, 50, 20), (20, 30, 7), (5, 8, 3)]
    else:
        ctx.set_option("max_slots", 2 if shape == "B9-slots2" else 4)
        dims = [(12, 20, 2 + k % 6) for k in range(9)]
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate(dims)]
    probs = [q[0] for q in planted]
    bt = solved(ctx, probs, scaling=10)
    assert_instance(ctx, bt, 256 if shape == "mixed" else 128)
    rng = np.random.default_rng(5)
    dirs = [TR.direction(p, rng) for p in probs]
    sides = padded([q[1] for q in planted], bt.m, np.int64)
    out = run_tangent(ctx, bt, batch_direction(bt, dirs), sides)       # (NaN beyond every member's own sizes: ignored on input)
    if shape == "B9-slots2":
        assert bt.B > bt.launch_shape()[0]                    # more members than factor slots: the work queue
    for b, (p, side, _, _) in enumerate(planted):
        assert int(bt.info(b).status_val) == 1
        x, y = bt.solution_of(b)
        assert_complementary(p, side, x, y)
        judge(ctx, "%s[%d]" % (shape, b), p, side, x, y, dirs[b], out, b)
    again = run_tangent(ctx, bt, batch_direction(bt, dirs), sides)     # 9. two calls on the same state: the same bits in every output
    for k in OUT:
        assert np.array_equal(out[k], again[k]), k


def test_batch_without_constraints(ctx):
    n = 12
    base = [R.planted_qp(n, 20, 0, 9520 + b)[0] for b in range(2)]
    probs = [dataclasses.replace(p, m=0, Ap=np.zeros(n + 1, dtype=np.int64), Ai=np.zeros(0, dtype=np.int64), Ax=np.zeros(0), bmin=np.zeros(0),
                                 bmax=np.zeros(0)) for p in base]
    bt = solved(ctx, probs, scaling=10)
    assert bt.m == 0
    rng = np.random.default_rng(16)
    dirs = [TR.direction(p, rng, keys=("dq", "dQx")) for p in probs]
    out = run_tangent(ctx, bt, batch_direction(bt, dirs), None)
    for b, p in enumerate(probs):
        x, y = bt.solution_of(b)
        judge(ctx, "m0[%d]" % b, p, np.zeros(0, int), x, y, dirs[b], out, b)


# ---- 7. the sparse factor --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blocks", "banded"])
def test_sparse_factor_instance(ctx, kind):
    if kind == "blocks":
        base, _ = blocks_qp(43, 2)
    else:
        base, _ = gadget_qp((), 4105, 5, cliques=False, stars=False, arrow=False, single=False, band=12)
    p, side, _, _ = R.replant(base, min(base.n - 1, base.m) // 2, 77)
    ctx.set_option("sparse_factor", 1)
    try:
        bt = solved(ctx, [p], scaling=10)
        assert bt.sparse_info(0)[0] > 0
        x, y = bt.solution_of(0)
        assert int(bt.info(0).status_val) == 1
        assert_complementary(p, side, x, y)
        d = TR.direction(p, np.random.default_rng(3))
        out = run_tangent(ctx, bt, batch_direction(bt, [d]), side[None, :])
        judge(ctx, "sparse-" + kind, p, side, x, y, d, out)
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 8. duality with the shipped adjoint, on the device --------------------------------------------------------------------------------------------
def test_duality_with_the_adjoint(ctx):
    planted = [R.planted_qp(33, 50, 20, 9980), R.planted_qp(33, 50, 9, 9981), R.planted_qp(20, 30, 7, 9982)]
    probs = [q[0] for q in planted]
    bt = solved(ctx, probs, scaling=10)
    rng = np.random.default_rng(22)
    dirs = [TR.direction(p, rng) for p in probs]
    sides = padded([q[1] for q in planted], bt.m, np.int64)
    gx, gy = rng.standard_normal((bt.B, bt.n)), rng.standard_normal((bt.B, bt.m))
    tan = run_tangent(ctx, bt, batch_direction(bt, dirs), sides)
    adj = {k: N(v) for k, v in bt.adjoint_device(T(ctx, gx), T(ctx, gy), T(ctx, sides, np.int64)).items()}
    assert np.all(tan["flag"] == 0) and np.all(adj["flag"] == 0)
    for b, (p, side, _, _) in enumerate(planted):
        n, m = p.n, p.m
        x, y = bt.solution_of(b)
        assert_complementary(p, side, x, y)
        _, J, scale_t, err_t = measure(p, side, x, y, dirs[b])
        za, z64a, _ = R.reference(p, side, gx[b, :n], gy[b, :m])
        scale_a = float(np.max(np.abs(za)))
        err_a = float(np.max(np.abs(z64a - za))) / scale_a
        lhs = np.asarray(gx[b, :n], dtype=LD) @ tan["dx"][b, :n] + np.asarray(gy[b, :m], dtype=LD) @ tan["dy"][b, :m]
        got = {k: adj[k][b, :len(dirs[b][k])] for k in TR.KEYS}
        rhs = TR.pairing(dirs[b], got)
        bound = 8.0 * (err_t * scale_t * (np.sum(np.abs(gx[b, :n])) + np.sum(np.abs(gy[b, :m][J]))) + err_a * scale_a * TR.norm1(dirs[b]))
        print("TANGENT-DUAL | %s | member %d | <g, tangent> %.15e | <adjoint, direction> %.15e | gap %.2e | bound %.2e" %
              (ctx.kind, b, float(lhs), float(rhs), float(abs(lhs - rhs)), bound))
        assert abs(lhs - rhs) <= bound


# ---- 10. the forward path does not see the tangent -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,slots,then_adjoint", [("dense", 3, 512, False), ("dense", 5, 1, True), ("sparse", 3, 2, False)])
def test_next_step_is_bit_identical(ctx, mode, B, slots, then_adjoint):
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
        H.solve(); G.solve()
        assert (B > G.launch_shape()[0]) == (slots != 512)
        rng = np.random.default_rng(4)
        before, epoch = snapshot(G), G.epoch
        dirs = [TR.direction(p, rng) for p in probs]
        out = run_tangent(ctx, G, batch_direction(G, dirs), None)
        assert np.all(out["flag"] == 0) and G.epoch == epoch
        if then_adjoint:                                      # the two do not disturb each other: the adjoint after a tangent is the adjoint alone
            gx, gy = rng.standard_normal((B, G.n)), rng.standard_normal((B, G.m))
            a_g = G.adjoint_device(T(ctx, gx), T(ctx, gy))
            a_h = H.adjoint_device(T(ctx, gx), T(ctx, gy))
            for k in a_g:
                assert torch.equal(a_g[k], a_h[k]), k
            again = run_tangent(ctx, G, batch_direction(G, dirs), None)
            for k in OUT:
                assert np.array_equal(out[k], again[k]), k
        after = snapshot(G)
        assert all(np.array_equal(before[k], after[k]) for k in before)       # nothing the caller can read has moved
        q2 = T(ctx, np.array([p.q for p in probs]) + 0.05 * rng.standard_normal((B, G.n)))
        for bt in (H, G):
            rc, _ = bt.step_device(q=q2, warm="last")
            assert rc == 0
        a, b = snapshot(H), snapshot(G)
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not bad, bad
        assert np.all(a["status_val"] == 1)
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 11. flags and refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", REFUSED)
def test_unsupported_modes_are_refused(ctx, which):
    with refused_mode(ctx, which) as bt:
        with pytest.raises(QpgError) as e:
            bt.tangent_device(dq=T(ctx, np.ones((1, 12))))
        assert e.value.code == UNSUPPORTED and "qpg_batch_tangent_device" in str(e.value)
        assert REFUSED_WORD[which] in str(e.value)


def test_invalid_calls(ctx):
    bt, _ = small_batch(ctx, B=2)
    dq = T(ctx, np.ones((2, 12)))
    bt.iterate(1)                                            # a solve in progress
    with pytest.raises(QpgError) as e:
        bt.tangent_device(dq=dq)
    assert e.value.code == INVALID and "in progress" in str(e.value)
    bt.solve()
    with pytest.raises(ValueError):
        bt.tangent_device()                                  # no direction at all
    io = capi.DeviceTangent()                                # ... and at the C ABI: all five NULL
    assert bt.L.qpg_batch_tangent_device(bt.h, C.byref(io)) == INVALID
    assert bt.L.qpg_batch_tangent_device(bt.h, None) == INVALID
    bad = np.zeros((2, 20), np.int64)
    bad[1, 19] = 2
    with pytest.raises(QpgError) as e:
        bt.tangent_device(dq=dq, active=T(ctx, bad, np.int64))
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        bt.tangent_device(dq=dq.to(torch.float32))
    with pytest.raises(ValueError):
        bt.tangent_device(dq=T(ctx, np.ones((2, 13))))
    with pytest.raises(ValueError):
        bt.tangent_device(dq=dq, dAx=T(ctx, np.ones((2, bt.nnzA + 1))))
    with pytest.raises(ValueError):
        bt.tangent_device(dq=dq, out=dict(dx=T(ctx, np.zeros((2, 11)))))
    with pytest.raises(ValueError):
        bt.tangent_device(dq=dq, want=("dx", "dq"))
    out = bt.tangent_device(dq=dq)                           # ... and the batch still works
    assert np.all(N(out["flag"]) == 0)


def test_tangent_before_setup_is_refused(ctx):
    h = C.c_void_p()
    L = ctx.L
    st = ctx.default_settings(**ST)
    assert L.qpg_batch_create(ctx.h, 1, 4, 2, 8, 4, C.byref(st), C.byref(h)) == 0
    try:
        io = capi.DeviceTangent()
        io.dq = 8                                            # (not NULL: the call has to stop at "not set up" before it looks at any array)
        assert L.qpg_batch_tangent_device(h, C.byref(io)) == INVALID
    finally:
        L.qpg_batch_destroy(h)


def test_unsolved_member_gets_flag_2_and_its_neighbours_are_right(ctx):
    """max_iter = 1: members 0 and 2 start at their planted solutions and end SOLVED at once, member 1 starts cold and ends at MAX_ITER"""
    planted = [R.planted_qp(12, 20, 5, 9960 + b) for b in range(3)]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10, max_iter=1)))
    wx, wy = np.array([q[2] for q in planted]), np.array([q[3] for q in planted])
    wx[1], wy[1] = 0.0, 0.0
    bt.warm_start(wx, wy)
    bt.solve()
    assert bt.statuses().tolist() == [1, -2, 1]
    rng = np.random.default_rng(17)
    dirs = [TR.direction(p, rng) for p in probs]
    out = run_tangent(ctx, bt, batch_direction(bt, dirs), np.array([q[1] for q in planted]))
    assert out["flag"].tolist() == [0, 2, 0]
    for k in OUT:
        assert np.all(out[k][1] == 0) or k == "flag", k
    for b in (0, 2):
        p, side, _, _ = planted[b]
        x, y = bt.solution_of(b)
        assert_complementary(p, side, x, y)
        judge(ctx, "neighbour[%d]" % b, p, side, x, y, dirs[b], out, b)


def test_dependent_active_rows(ctx):
    """two identical rows, both handed in as active, with different db: K is singular and the system has no solution -- flag 1, zeros, nothing non-finite"""
    p, side, _, _ = R.planted_qp(12, 20, 5, 9970)
    A = p.A_mat().tolil()
    i0 = int(np.flatnonzero(side)[0])
    i1 = int(np.flatnonzero(side == 0)[0])
    A[i1, :] = A[i0, :]
    A = A.tocsc(); A.sort_indices()
    x = np.linalg.solve(p.Q_full().toarray(), -p.q)
    ax = A @ x
    p2 = dataclasses.replace(p, Ap=A.indptr.astype(np.int64), Ai=A.indices.astype(np.int64), Ax=A.data.copy(), bmin=ax - 1.0, bmax=ax + 1.0)
    bt = solved(ctx, [p2], scaling=10)
    assert int(bt.info(0).status_val) == 1
    sides = np.zeros((1, 20), np.int64)
    sides[0, i0], sides[0, i1] = -1, -1
    db = np.zeros((1, 20))
    db[0, i0], db[0, i1] = 1.0, -1.0
    out = run_tangent(ctx, bt, dict(dq=np.ones((1, 12)), dbmin=db), sides)
    assert int(out["flag"][0]) == 1 and int(out["passes"][0]) == 200
    assert np.all(out["dx"] == 0) and np.all(out["dy"] == 0)
    assert np.array_equal(out["active"], sides) and np.isfinite(out["resid"][0])


# ---- 12. forward-mode AD through the torch layer ---------------------------------------------------------------------------------------------------
def test_torch_forward_mode(ctx):
    import torch.autograd.forward_ad as fwad
    n, m = 33, 50
    planted = [R.planted_qp(n, m, 20, 9980), R.planted_qp(n, m, 9, 9981)]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    layer = QPLayer(bt)
    rng = np.random.default_rng(23)
    q, lo, hi = (T(ctx, [getattr(p, k) for p in probs]) for k in ("q", "bmin", "bmax"))
    Qx, Ax = T(ctx, padded([p.Qx for p in probs], bt.nnzQ)), T(ctx, padded([p.Ax for p in probs], bt.nnzA))
    tq, tA = T(ctx, rng.standard_normal((2, n))), T(ctx, rng.standard_normal((2, bt.nnzA)))
    with fwad.dual_level():
        x, y, status = layer(fwad.make_dual(q, tq), lo, hi, Qx=Qx, Ax=fwad.make_dual(Ax, tA))
        assert N(status).tolist() == [1, 1]
        dx, dy = fwad.unpack_dual(x).tangent, fwad.unpack_dual(y).tangent
        own = bt.tangent_device(dq=tq, dAx=tA)
        assert torch.equal(dx, own["dx"]) and torch.equal(dy, own["dy"])          # bit for bit the call's own outputs
        assert N(layer.last_tangent["flag"]).tolist() == [0, 0]
        assert fwad.unpack_dual(status).tangent is None
    out = {k: N(v) for k, v in own.items()}
    for b, (p, side, _, _) in enumerate(planted):
        xb, yb = bt.solution_of(b)
        assert_complementary(p, side, xb, yb)
        judge(ctx, "layer[%d]" % b, p, side, xb, yb, dict(dq=N(tq)[b], dAx=N(tA)[b, :len(p.Ax)]), out, b)
    # a tangent asked for after the batch has moved on would differentiate another solve: refused
    # (torch asks for the jvp inside the forward pass itself, so the late request is made by hand, with the record a forward pass leaves)
    late = types.SimpleNamespace(layer=layer, epoch=bt.epoch)
    assert torch.equal(_QPFunction.jvp(late, None, tq, None, None, None, tA)[0], own["dx"])
    bt.solve()
    with pytest.raises(RuntimeError):
        _QPFunction.jvp(late, None, tq, None, None, None, tA)
    # reverse mode still works after a forward-mode pass
    q2 = q.clone().requires_grad_(True)
    x2, _, _ = layer(q2)
    x2.sum().backward()
    ref = bt.adjoint_device(torch.ones_like(x2), want=("dq",))["dq"]
    assert torch.equal(q2.grad, ref)

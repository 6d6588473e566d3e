"""The polish of a solved batch (qpg_batch_polish_device / QpalmBatch.polish_device / QPLayer(polish=True)); DESIGN.md section 14.

Problems: the planted QPs of tests/adjoint_refs.py (|y_i| >= 0.5 on J, slack >= 0.5 elsewhere), solved at LOOSE tolerances (eps_abs = eps_rel = 1e-3, or
the defaults of 1e-4), so that the stored solution is visibly inexact while its active set is still the planted one -- asserted before every polish
(assert_inexact_but_right).

Reference: tests/polish_refs.py -- K [x; y_J] = [-q; b_J] in numpy.longdouble (rationals below 14 unknowns), the clip, and the residual measures of the
termination test in unscaled space.

Tolerances:
  accuracy   err64 = the error of float64 numpy.linalg.solve on the same system against that reference, relative to ||[x; y_J]||inf; the polished
             [x^; y^_J] must be within 8 err64 + 4 u of the reference on the same scale: the rule of tests/test_adjoint.py plus the rounding of x + dx
             (and of its own halves).  Measured figures (both backends): profiles/polish/accuracy.md.
  residuals  the componentwise bound gamma_k (|A| |x| + |b|), gamma_k (|Q| |x| + |q| + |A'| |y|), k counted in polish_refs.residual_bounds.
  rejections the reference's own verdict must fail by a factor of at least 10 before the device is asked (asserted on the reference alone).

Where pri_old is exactly 0 (no active row, every slack >= 0.5: the violation is max(.., 0) = 0) "pri_new < pri_old" cannot hold; pri_new == 0 is asserted
there instead."""
import ctypes as C

import numpy as np
import pytest
import torch

from qpalm_amd import capi
from qpalm_amd.capi import QpgError
from qpalm_amd.solver import QpalmBatch
from qpalm_amd.torch_layer import QPLayer
from tests import adjoint_refs as R
from tests import polish_refs as PR
from tests.sens_helpers import (CASES, INVALID, REFUSED, REFUSED_WORD, UNSUPPORTED, N, T, assert_complementary, assert_instance, judge_adjoint, padded,
                                refused_mode, run_adjoint, run_polish, small_batch, snapshot)
from tests.sens_helpers import judge_polish as judge
from tests.sparse_gadgets import blocks_qp, gadget_qp

LD = R.LD
U = 2.0 ** -53
LOOSE = dict(eps_abs=1e-3, eps_rel=1e-3, verbose=0)
DEFAULT = dict(verbose=0)                                    # eps_abs = eps_rel = 1e-4


def loose(ctx, probs, **st):
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(LOOSE, **st)))
    bt.solve()
    return bt


def assert_inexact_but_right(p, side, x, y, zr=None, least=0.0):
    """the stored solution of a loose solve: the planted active set is still unmistakable (the multipliers of J at least 0.25 with the planted sign, the
    other rows at least 0.25 inside their bounds with multipliers below 1e-2, the rows of J within 1e-2 of their bound) and, where a reference is given,
    the point is at least `least` away from it in the accuracy test's measure"""
    ax = p.A_mat() @ x
    act, eq = side != 0, p.bmin == p.bmax
    assert np.all(np.abs(y[act]) >= 0.25)
    assert np.all((np.sign(y) == side)[act & ~eq])           # y > 0 on an upper bound, < 0 on a lower one
    assert np.all(np.abs(y[~act]) <= 1e-2)
    assert np.all(np.minimum(ax - p.bmin, p.bmax - ax)[~act] >= 0.25)
    assert np.all(np.abs(np.where(side < 0, ax - p.bmin, ax - p.bmax))[act] <= 1e-2)
    if zr is not None:
        J = np.flatnonzero(side)
        err = float(np.max(np.abs(np.concatenate([x, y[J]]) - zr))) / (float(np.max(np.abs(zr))) or 1.0)
        assert err >= least, (err, least)


# ---- 1. accuracy at every size where a kernel changes form; 2. the reported residuals (the same calls) ----------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_polished_solution_matches_the_reference_solve(ctx, case):
    p, side, _, _ = R.planted_qp(case.n, case.m, case.nact, 9000 + 7 * case.n + case.nact, sides=case.sides, equality=case.equality)
    bt = loose(ctx, [p], scaling=case.scaling, proximal=case.proximal)
    assert int(bt.info(0).status_val) == 1
    assert_instance(ctx, bt, 256 if case.n <= 256 else 512)
    x, y = bt.solution_of(0)
    zr = PR.candidate(p, side)[0]
    assert_inexact_but_right(p, side, x, y, zr, least=1e-9)
    out = run_polish(ctx, bt, side[None, :])
    tol, err0 = judge(ctx, case.id, p, side, x, y, out)
    assert err0 >= 1e4 * tol                                  # what the polish had to do
    # ---- the four reported residuals against the same quantities in longdouble ----
    nscale = case.scaling
    for tag, (xx, yy), got in (("old", (x, y), out["res"][0, :2]), ("new", (out["x"][0], out["y"][0]), out["res"][0, 2:])):
        ref = PR.residuals(p, xx, yy)
        bpri, bdua, kp, kd = PR.residual_bounds(p, xx, yy, nscale)
        print("POLISH-RES | %s | %s | %s | pri %.3e (ref %.3e, bound %.1e, k %d) | dua %.3e (ref %.3e, bound %.1e, k %d)" %
              (ctx.kind, case.id, tag, got[0], float(ref["pri"]), float(bpri), kp, got[1], float(ref["dua"]), float(bdua), kd))
        assert abs(LD(got[0]) - ref["pri"]) <= bpri, (tag, "pri")
        assert abs(LD(got[1]) - ref["dua"]) <= bdua, (tag, "dua")
    # again: the same bits (no atomics, the state has not moved); active_in = NULL: the engine's own rule on the stored solution (its numpy restatement;
    # after a loose solve it need not find the planted set) -- where it does find it, the same bits once more
    again, by_rule, rule = run_polish(ctx, bt, side[None, :]), run_polish(ctx, bt, None), R.default_rule(bt, p, 0)
    assert np.array_equal(by_rule["active"][0], rule)
    for k in out:
        assert np.array_equal(out[k], again[k]), k
        assert np.array_equal(out[k], by_rule[k]) or not np.array_equal(rule, side), k


# ---- 3. rejections that convexity guarantees ---------------------------------------------------------------------------------------------------
def pick_wrong_set(p, side, x, y, which):
    """(the set to hand in, the row changed): (a) an inactive row marked active on the side nearer to A x, (b) an active row left out -- the first row
    for which the REFERENCE's verdict misses by a factor of at least 10"""
    ax = p.A_mat() @ x
    for i in range(p.m):
        s = side.copy()
        if which == "extra-row":
            if side[i] != 0:
                continue
            s[i] = -1 if ax[i] - p.bmin[i] <= p.bmax[i] - ax[i] else 1
        else:
            if side[i] == 0:
                continue
            s[i] = 0
        v = PR.verdict(p, s, x, y, LOOSE["eps_abs"], LOOSE["eps_rel"])
        if which == "extra-row" and v["new"]["dua"] >= 10 * max(v["old"]["dua"], v["eps_dua"]) and v["y"][i] == 0:
            return s, i, v
        if which == "missing-row" and v["new"]["pri"] >= 10 * max(v["old"]["pri"], v["eps_pri"]):
            return s, i, v
    raise AssertionError("no row of this problem gives a rejection with a margin of 10: choose another seed")


@pytest.mark.parametrize("which", ["extra-row", "missing-row"])
def test_wrong_active_sets_are_rejected(ctx, which):
    p, side, _, _ = R.planted_qp(12, 20, 5, 9910)
    bt = loose(ctx, [p], scaling=10)
    x, y = bt.solution_of(0)
    assert_inexact_but_right(p, side, x, y)
    s, i, v = pick_wrong_set(p, side, x, y, which)
    assert not v["accepted"]
    if which == "extra-row":
        assert abs(float(PR.candidate(p, s)[0][p.n + int(np.searchsorted(np.flatnonzero(s), i))])) > 0    # the multiplier there: wrong-signed, clipped
    print("POLISH-REJ | %s | %s | row %d | reference: pri %.2e -> %.2e (eps %.2e), dua %.2e -> %.2e (eps %.2e)" %
          (ctx.kind, which, i, float(v["old"]["pri"]), float(v["new"]["pri"]), float(v["eps_pri"]), float(v["old"]["dua"]), float(v["new"]["dua"]), float(v["eps_dua"])))
    before = snapshot(bt)
    for store in (False, True):
        epoch = bt.epoch
        out = run_polish(ctx, bt, s[None, :], store=store)
        assert int(out["flag"][0]) == 3 and bt.epoch == epoch
        assert np.array_equal(out["x"][0], x) and np.array_equal(out["y"][0], y)            # the stored solution, bit for bit
        assert np.array_equal(out["active"][0], s)
        got = out["res"][0]
        assert got[2] == pytest.approx(float(v["new"]["pri"]), rel=1e-6, abs=1e-12) and got[3] == pytest.approx(float(v["new"]["dua"]), rel=1e-6, abs=1e-12)
        after = snapshot(bt)
        assert all(np.array_equal(before[k], after[k]) for k in before)                    # nothing stored
    assert int(run_polish(ctx, bt, side[None, :])["flag"][0]) == 0                          # the right set: accepted


# ---- 4. batches: mixed sizes; nine members on four slots (the 128-thread instance on the GPU, once with n = 192); B > slots; one unsolved member ------
@pytest.mark.parametrize("shape", ["mixed", "B9-slots4", "B9-slots4-n192", "B9-slots2"])
def test_batches(ctx, shape):
    if shape == "mixed":
        dims = [(33, 50, 20), (20, 30, 7), (5, 8, 3)]
    else:
        ctx.set_option("max_slots", 2 if shape == "B9-slots2" else 4)
        dims = [(12, 20, 2 + k % 6) for k in range(9)]
        if shape == "B9-slots4-n192":
            dims[4] = (192, 96, 60)
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate(dims)]
    bt = loose(ctx, [q[0] for q in planted], scaling=10)
    assert_instance(ctx, bt, 256 if shape == "mixed" else 128)
    sides = padded([q[1] for q in planted], bt.m, np.int64)
    stored = [bt.solution_of(b) for b in range(bt.B)]
    out = run_polish(ctx, bt, sides)
    if shape == "B9-slots2":
        assert bt.B > bt.launch_shape()[0]                    # more members than factor slots: the work queue
    elif ctx.kind == "hip":
        assert bt.B <= bt.launch_shape()[0]                   # (the emulator's one instance keeps fewer slots)
    for b, (p, side, _, _) in enumerate(planted):
        assert int(bt.info(b).status_val) == 1
        assert_inexact_but_right(p, side, *stored[b])
        judge(ctx, "%s[%d]" % (shape, b), p, side, *stored[b], out, b)


def test_unsolved_member_gets_flag_2_and_its_neighbours_are_right(ctx):
    """max_iter = 1: members 0 and 2 start at their planted solutions and end SOLVED at once, member 1 starts cold and ends at MAX_ITER.  The neighbours'
    stored solutions are at rounding level already: they must be accepted all the same (not rejected for rounding), and stay as exact."""
    planted = [R.planted_qp(12, 20, 5, 9960 + b) for b in range(3)]
    bt = QpalmBatch(ctx, [q[0] for q in planted], ctx.default_settings(**dict(LOOSE, scaling=10, max_iter=1)))
    wx, wy = np.array([q[2] for q in planted]), np.array([q[3] for q in planted])
    wx[1], wy[1] = 0.0, 0.0
    bt.warm_start(wx, wy)
    bt.solve()
    assert bt.statuses().tolist() == [1, -2, 1]
    stored = [bt.solution_of(b) for b in range(3)]
    out = run_polish(ctx, bt, np.array([q[1] for q in planted]), store=True)
    assert out["flag"].tolist() == [0, 2, 0]
    assert np.array_equal(out["x"][1], stored[1][0]) and np.array_equal(out["y"][1], stored[1][1])
    for k in ("res", "active", "resid", "passes"):
        assert np.all(out[k][1] == 0), k
    now = [bt.solution_of(b) for b in range(3)]
    assert np.array_equal(now[1][0], stored[1][0]) and np.array_equal(now[1][1], stored[1][1])   # it keeps its stored solution
    for b in (0, 2):
        p, side, _, _ = planted[b]
        judge(ctx, "neighbour[%d]" % b, p, side, *stored[b], out, b, improves=False)
        assert np.array_equal(now[b][0], out["x"][b]) and np.array_equal(now[b][1], out["y"][b])


# ---- 5. the sparse factor instance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blocks", "banded"])
def test_sparse_factor_instance(ctx, kind):
    if kind == "blocks":
        base, _ = blocks_qp(43, 2)
    else:
        base, _ = gadget_qp((), 4105, 5, cliques=False, stars=False, arrow=False, single=False, band=12)
    p, side, _, _ = R.replant(base, min(base.n - 1, base.m) // 2, 77)
    ctx.set_option("sparse_factor", 1)
    try:
        bt = loose(ctx, [p], scaling=10)
        assert bt.sparse_info(0)[0] > 0 and int(bt.info(0).status_val) == 1
        x, y = bt.solution_of(0)
        assert_inexact_but_right(p, side, x, y, PR.candidate(p, side)[0], least=1e-9)
        out = run_polish(ctx, bt, side[None, :])
        judge(ctx, "sparse-" + kind, p, side, x, y, out)
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 6. state -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,slots,warm", [("dense", 3, 512, "last"), ("dense", 5, 1, None), ("sparse", 2, 512, None), ("sparse", 3, 2, "last")])
def test_next_step_is_bit_identical_without_store(ctx, mode, B, slots, warm):
    ctx.set_option("max_slots", slots)
    if mode == "sparse":
        ctx.set_option("sparse_factor", 1)
    try:
        if mode == "sparse":
            probs = [R.replant(blocks_qp(43, 2)[0], 10, 60 + b)[0] for b in range(B)]
        else:
            probs = [R.planted_qp(12, 20, 5, 9900 + b)[0] for b in range(B)]
        H, G = (QpalmBatch(ctx, probs, ctx.default_settings(**LOOSE)) for _ in range(2))
        H.solve(); G.solve()
        assert (B > G.launch_shape()[0]) == (slots != 512)        # more members than factor slots: the work queue
        before, epoch = snapshot(G), G.epoch
        out = run_polish(ctx, G, None, store=False)
        # (active_in = NULL: after a loose solve the engine's rule misses the planted set for some of the sparse members -- the stored y is yh, and
        # yh / sigma can be smaller than a slack of 1e-5 -- and those are rejected: both ends of the call are in this test)
        assert np.all((out["flag"] == 0) | (out["flag"] == 3)) and int(out["flag"][0]) == 0 and G.epoch == epoch
        assert (mode == "dense") <= bool(np.all(out["flag"] == 0))
        assert not np.array_equal(out["x"], before["x"])          # (the call did find something to do)
        after = snapshot(G)
        assert all(np.array_equal(before[k], after[k]) for k in before)       # nothing the caller can read has moved
        rng = np.random.default_rng(4)
        q2 = T(ctx, np.array([p.q for p in probs]) + 0.05 * rng.standard_normal((B, G.n)))
        for bt in (H, G):
            rc, _ = bt.step_device(q=q2, warm=warm)
            assert rc == 0
        a, b = snapshot(H), snapshot(G)
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not bad, bad
        assert np.all(a["status_val"] == 1)
    finally:
        ctx.set_option("sparse_factor", -1)


def test_store_replaces_the_stored_solution_and_nothing_else(ctx):
    """two members, the second with equality rows only on J (multipliers of both signs).  store = 1: get_solution_device returns the call's x, y; infos and
    counters stay; the adjoint called afterwards is that of (x^, y^) by the rule of tests/test_adjoint.py; warm_start_last starts from the polished point."""
    planted = [R.planted_qp(20, 30, 9, 9920), R.planted_qp(20, 30, 9, 9921, equality=True)]
    probs = [q[0] for q in planted]
    sides = np.array([q[1] for q in planted])
    bt = loose(ctx, probs, scaling=10)
    stored = [bt.solution_of(b) for b in range(2)]
    for b, (p, side, _, _) in enumerate(planted):
        assert_inexact_but_right(p, side, *stored[b])
    before, epoch = snapshot(bt), bt.epoch
    dry = run_polish(ctx, bt, sides)                          # twice without store: the same bits
    assert all(np.array_equal(dry[k], v) for k, v in run_polish(ctx, bt, sides).items()) and bt.epoch == epoch
    out = run_polish(ctx, bt, sides, store=True)
    assert all(np.array_equal(dry[k], out[k]) for k in dry) and out["flag"].tolist() == [0, 0] and bt.epoch == epoch + 1
    gx_, gy_ = bt.solution_device()
    assert np.array_equal(N(gx_), out["x"]) and np.array_equal(N(gy_), out["y"])
    after = snapshot(bt)
    assert all(np.array_equal(before[k], after[k]) for k in before if k not in ("x", "y"))
    assert np.array_equal(after["x"], out["x"]) and np.array_equal(after["y"], out["y"])
    yeq = out["y"][1][sides[1] != 0]
    assert np.any(yeq <= -0.25) and np.any(yeq >= 0.25)       # the equality rows keep either sign
    for b, (p, side, _, _) in enumerate(planted):
        judge(ctx, "store[%d]" % b, p, side, *stored[b], out, b)
    # the adjoint at the polished point: its own active-set rule finds J there, and the gradients are those of (x^, y^)
    rng = np.random.default_rng(31)
    gx, gy = rng.standard_normal((2, 20)), rng.standard_normal((2, 30))
    adj = run_adjoint(ctx, bt, gx, gy, None)
    for b, (p, side, _, _) in enumerate(planted):
        assert_complementary(p, side, out["x"][b], out["y"][b])
        judge_adjoint(ctx, "after-polish[%d]" % b, p, side, out["x"][b], out["y"][b], gx[b], gy[b], adj, b)
    # a third polish starts from the polished point: accepted again (a point at rounding level is not rejected for rounding) and as exact
    third = run_polish(ctx, bt, sides, store=True)
    assert third["flag"].tolist() == [0, 0]
    for b, (p, side, _, _) in enumerate(planted):
        judge(ctx, "again[%d]" % b, p, side, out["x"][b], out["y"][b], third, b, improves=False)
    bt.warm_start_last()
    bt.solve()
    assert bt.statuses().tolist() == [1, 1] and all(int(i.iter) <= 2 for i in bt.infos())      # it starts where it ends


# ---- 7. invalid calls and refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", REFUSED)
def test_unsupported_modes_are_refused(ctx, which):
    with refused_mode(ctx, which) as bt:
        with pytest.raises(QpgError) as e:
            bt.polish_device()
        assert e.value.code == UNSUPPORTED and "qpg_batch_polish_device" in str(e.value)
        assert REFUSED_WORD[which] in str(e.value)


def test_invalid_calls(ctx):
    bt, _ = small_batch(ctx, B=2)
    bt.iterate(1)                                            # a solve in progress
    with pytest.raises(QpgError) as e:
        bt.polish_device()
    assert e.value.code == INVALID and "in progress" in str(e.value)
    bt.solve()
    io = capi.DevicePolish()                                 # x, y, res all NULL and store = 0 at the C ABI
    assert bt.L.qpg_batch_polish_device(bt.h, C.byref(io)) == INVALID
    assert bt.L.qpg_batch_polish_device(bt.h, None) == INVALID
    with pytest.raises(QpgError) as e:
        bt.polish_device(want=("flag", "active"))            # ... and through the wrapper: outputs, but none of the three
    assert e.value.code == INVALID and "nothing to do" in str(e.value)
    epoch = bt.epoch
    assert bt.polish_device(want=(), store=True) == {}       # store alone is a call
    assert bt.epoch == epoch + 1
    bad = np.zeros((2, 20), np.int64)
    bad[1, 19] = 2
    with pytest.raises(QpgError) as e:
        bt.polish_device(T(ctx, bad, np.int64))
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        bt.polish_device(T(ctx, np.zeros((2, 20)), np.int32))
    with pytest.raises(ValueError):
        bt.polish_device(out=dict(x=T(ctx, np.zeros((2, 11)))))
    with pytest.raises(ValueError):
        bt.polish_device(want=("x", "dq"))
    assert np.all(N(bt.polish_device()["flag"]) == 0)        # ... and the batch still works


def test_polish_before_setup_is_refused(ctx):
    h = C.c_void_p()
    L = ctx.L
    st = ctx.default_settings(**LOOSE)
    assert L.qpg_batch_create(ctx.h, 1, 4, 2, 8, 4, C.byref(st), C.byref(h)) == 0
    try:
        io = capi.DevicePolish()
        io.x = 8                                             # (not NULL: the call has to stop at "not set up" before it looks at any array)
        assert L.qpg_batch_polish_device(h, C.byref(io)) == INVALID
    finally:
        L.qpg_batch_destroy(h)


# ---- 8. the torch layer -----------------------------------------------------------------------------------------------------------------------------
def test_layer_with_polish_differentiates_at_the_exact_solution(ctx):
    """a default-tolerance solve (1e-4): with polish=True the gradients are those of the exact solution at J by the rule of tests/test_adjoint.py (judge, fed
    the longdouble solution); with polish=False the per-entry gradients, products with the stored (x, y), miss that rule by the solve's own error"""
    n, m = 33, 50
    planted = [R.planted_qp(n, m, 20, 9980), R.planted_qp(n, m, 9, 9981)]
    probs = [q[0] for q in planted]
    rng = np.random.default_rng(21)
    cx, cy = rng.standard_normal((2, n)), rng.standard_normal((2, m))
    grads = {}
    for polish in (True, False):
        bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(DEFAULT, scaling=10)))
        leaf = lambda a: T(ctx, a).requires_grad_(True)
        q, lo, hi = leaf([p.q for p in probs]), leaf([p.bmin for p in probs]), leaf([p.bmax for p in probs])
        Qx, Ax = leaf(padded([p.Qx for p in probs], bt.nnzQ)), leaf(padded([p.Ax for p in probs], bt.nnzA))
        layer = QPLayer(bt, polish=polish)
        x, y, status = layer(q, lo, hi, Qx=Qx, Ax=Ax)
        assert N(status).tolist() == [1, 1]
        sx, sy = bt.solution_device()
        assert torch.equal(sx, x) and torch.equal(sy, y)      # what the layer returns is what the batch stores (and differentiates at)
        if polish:
            assert N(layer.last_polish["flag"]).tolist() == [0, 0]
        else:
            assert layer.last_polish is None
        ((T(ctx, cx) * x).sum() + (T(ctx, cy) * y).sum()).backward()
        assert N(layer.last_adjoint["flag"]).tolist() == [0, 0]
        act = bt.adjoint_device(T(ctx, cx), T(ctx, cy), want=("active",))["active"]       # the set backward() found (the state has not moved)
        grads[polish] = dict(dq=N(q.grad), dbmin=N(lo.grad), dbmax=N(hi.grad), dQx=N(Qx.grad), dAx=N(Ax.grad), flag=N(layer.last_adjoint["flag"]),
                             passes=N(layer.last_adjoint["passes"]), resid=N(layer.last_adjoint["resid"]), x=N(x), y=N(y), active=N(act))
    for b, (p, side, _, _) in enumerate(planted):
        zs, _, J = PR.candidate(p, side)                      # the exact solution at J
        xe, ye = zs[:n], np.zeros(m, dtype=LD)
        ye[J] = zs[n:]
        for polish in (True, False):
            g = grads[polish]
            if polish:
                judge_adjoint(ctx, "layer-polish[%d]" % b, p, side, xe, ye, cx[b], cy[b], g, b)
                continue
            assert_inexact_but_right(p, side, g["x"][b], g["y"][b])
            with pytest.raises(AssertionError):
                judge_adjoint(ctx, "layer-plain[%d]" % b, p, side, xe, ye, cx[b], cy[b], g, b)
            # by how much: the rule's own bound on dAx (sens_helpers.judge_adjoint), and the largest miss over the entries
            zr, z64, _ = R.reference(p, side, cx[b], cy[b])
            scale = float(np.max(np.abs(zr)))
            tol = 8.0 * float(np.max(np.abs(z64 - zr))) / scale
            ref = R.gradients(p, side, xe, ye, zr)["dAx"]
            ca = np.repeat(np.arange(n), np.diff(p.Ap))
            f = np.abs(ye[p.Ai]) + np.abs(xe[ca]) + 1.0
            miss = float(np.max(np.abs(g["dAx"][b][:len(ref)] - ref) / ((tol * scale + 4 * U * scale) * f)))
            print("POLISH-LAYER | %s | member %d | polish=False misses the bound on dAx by a factor of %.2e" % (ctx.kind, b, miss))
            assert miss >= 100.0

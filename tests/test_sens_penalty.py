"""The penalty floor of the sensitivity solves (qpg_batch_set_sens_penalty / QpalmBatch.sens_penalty / QPLayer(sens_penalty=...)).

With a floor s the preconditioner of the adjoint's, the tangent's and the polish's refinement uses sigma'_i = max(sigma_i, s) on the active rows.  The system
solved, the residual and the stopping rule are the same, so what the floor may change is the number of passes and the last bits of a converged member --
never the state of the batch, the active-set rule, or anything at all when it binds on no row.

  1  floor 0 and a floor below every penalty (1e-300: the new path runs and changes nothing): the bits of a batch that never set one
  2  a loose solve with small penalties: floor 0 runs into the pass cap, the recommended floor does not; the same set; the polish within its bound
  3  accuracy with the recommended floor at every size of tests/test_adjoint.py, by that file's judge; the tangent's duality with the adjoint
     3b a floor that binds costs few passes (PASS_BOUND) on every form of the assembly: the three dense instances, narrow rows, the sparse factor
  4  the state after a call with a binding floor, and the next solve
  5  dependent active rows
  6  subsets and the torch layer
  7  the interface

References and bounds are those of tests/test_adjoint.py, tests/test_tangent.py and tests/test_polish.py (8 x the error of float64 numpy against the
long-double solve; + 4 u for the polish); nothing is fixed here.  REC is the floor the documents recommend (profiles/sens_penalty/passes.md)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from qpalm_amd import capi
from qpalm_amd.capi import QpgError
from qpalm_amd.solver import QpalmBatch
from qpalm_amd.torch_layer import QPLayer
from tests import adjoint_refs as R
from tests import tangent_refs as TR
from tests.sens_helpers import (CASES, INVALID, ST, UNSUPPORTED, Case, N, T, assert_complementary, assert_instance, batch_direction, judge_adjoint, judge_polish,
                                padded, run_adjoint, run_polish, run_tangent, small_batch, snapshot, solved, tangent_measure)
from tests.sparse_gadgets import blocks_qp

LD = R.LD
REC = 1e6
MODES = ("adjoint", "tangent", "polish")


def call(ctx, bt, mode, sides, gx, gy, select=None, out=None, store=False):
    """one of the three calls on the same inputs (the tangent's direction: dq = gx, dbmin = dbmax = gy); host arrays"""
    act = None if sides is None else T(ctx, sides, np.int64)
    sel = None if select is None else T(ctx, select, np.int64)
    kw = dict(select=sel) if out is None else dict(select=sel, out=out)
    if mode == "adjoint":
        got = bt.adjoint_device(T(ctx, gx), None if gy is None else T(ctx, gy), act, **kw)
    elif mode == "tangent":
        got = bt.tangent_device(dq=T(ctx, gx), dbmin=None if gy is None else T(ctx, gy), dbmax=None if gy is None else T(ctx, gy), active=act, **kw)
    else:
        got = bt.polish_device(act, store=store, **kw)
    return {k: N(v) for k, v in got.items() if k != "n_selected"}


def set_floor(bt, s):
    """set the floor and read it back through the C call: a value that only stayed in a Python attribute would let every test below pass with the floor
    ignored"""
    bt.sens_penalty = s
    v = C.c_double(-1.0)
    assert bt.L.qpg_batch_get_sens_penalty(bt.h, C.byref(v)) == 0 and v.value == s


# With s = 1e6 on every row of J the preconditioner misses K~ only by -Sigma'^-1 <= 1e-6 in the (2, 2) block, so a pass contracts the error by
# 1 / (1 + s lambda) with lambda the eigenvalues of A~_J (Q~ + I / gamma)^-1 A~_J'.  The problems below are scaled (rows of A~ of norm about 1, Q~ of norm
# about 1), lambda >= 1e-3 by a wide margin, so a pass gains at least three digits and sixteen digits take at most five passes, plus the correction of the
# pass that meets the stopping rule: 6.  An assembly that boosts a row in one place and not in another is no such preconditioner and needs many more.
PASS_BOUND = 6


def histogram(passes):
    v, c = np.unique(np.asarray(passes), return_counts=True)
    return " ".join("%d:%d" % (int(a), int(b)) for a, b in zip(v, c))


# ---- 1. floor 0 and a floor that binds nowhere: today's bits ---------------------------------------------------------------------------------------
BITS = [("n65-128", Case(65, 32, 20, 10, 0), 128), ("n193-256", Case(193, 386, 90, 10, 1), 256), ("n257-512", Case(257, 514, 256, 0, 1, equality=True), 512),
        ("sparse", None, 512)]


@pytest.mark.parametrize("name,case,threads", BITS, ids=[b[0] for b in BITS])
def test_floor_zero_and_a_floor_that_binds_nowhere_are_todays_bits(ctx, name, case, threads):
    ctx.set_option("small_workgroups", 2 if threads == 128 else 1)       # (2: the 128-thread instance wherever its LDS fits)
    if case is None:
        ctx.set_option("sparse_factor", 1)
    try:
        if case is None:
            p, side, xs, ys = R.replant(blocks_qp(43, 2)[0], 10, 61)
            bt = solved(ctx, [p], scaling=10)
            assert bt.sparse_info(0)[0] > 0
        else:
            p, side, xs, ys = R.planted_qp(case.n, case.m, case.nact, 9000 + 7 * case.n + case.nact, sides=case.sides, equality=case.equality)
            bt = solved(ctx, [p], warm=(xs[None, :], ys[None, :]) if case.n >= 192 else None, scaling=case.scaling, proximal=case.proximal)
        assert int(bt.info(0).status_val) == 1
        assert_instance(ctx, bt, threads)
        assert float(np.min(bt.vec("sigma", 0)[:p.m])) > 1e-300
        rng = np.random.default_rng(17)
        gx, gy = rng.standard_normal((1, p.n)), rng.standard_normal((1, p.m))
        base = {mode: call(ctx, bt, mode, side[None, :], gx, gy) for mode in MODES}      # before any set call
        assert all(int(base[mode]["flag"][0]) == 0 for mode in MODES)
        for floor in (0.0, 1e-300):
            set_floor(bt, floor)
            for mode in MODES:
                got = call(ctx, bt, mode, side[None, :], gx, gy)
                for k in base[mode]:
                    assert np.array_equal(got[k], base[mode][k]), (floor, mode, k)
    finally:
        ctx.set_option("small_workgroups", 1)
        ctx.set_option("sparse_factor", -1)


# ---- 2. a loose solve: the cap is gone -------------------------------------------------------------------------------------------------------------
# nine members, max_slots 4 (the emulator's members then share four factor slots); every second one has no active row (F = Q~ + I / gamma is then the system itself: two passes with any floor), which keeps
# the emulator's 200-pass members to five.  sigma_init = sigma_max = 1e-3 holds every penalty at 1e-3 (in the engine's scaling: c * 1e-3): the
# refinement contracts by 1 / (1 + sigma lambda) ~ 1 - 1e-3 lambda per pass and the active members need thousands of passes.
LOOSE_DIMS = [(33 + 4 * k, 40 + 3 * k, (0, 5, 0, 9, 13, 0, 17, 0, 21)[k]) for k in range(9)]
LOOSE_ST = dict(eps_abs=1e-3, eps_rel=1e-3, verbose=0, scaling=10, sigma_init=1e-3, sigma_max=1e-3)
_LOOSE = {}


def loose_planted():
    if "planted" not in _LOOSE:
        _LOOSE["planted"] = [R.planted_qp(n, m, k, 9300 + 13 * b) for b, (n, m, k) in enumerate(LOOSE_DIMS)]
    return _LOOSE["planted"]


def loose_batch(ctx):
    """the batch of test 2 (and of the layer's test): solved from the planted solutions, penalties held at 1e-3"""
    planted = loose_planted()
    ctx.set_option("max_slots", 4)
    bt = QpalmBatch(ctx, [q[0] for q in planted], ctx.default_settings(**LOOSE_ST))
    bt.warm_start(padded([q[2] for q in planted], bt.n), padded([q[3] for q in planted], bt.m))
    bt.solve()
    assert bt.statuses().tolist() == [1] * 9
    return bt, planted


def test_a_loose_solve_no_longer_runs_into_the_pass_cap(ctx):
    try:
        bt, planted = loose_batch(ctx)
        sides = padded([q[1] for q in planted], bt.m, np.int64)
        stored = [bt.solution_of(b) for b in range(bt.B)]
        rng = np.random.default_rng(5)
        gx, gy = rng.standard_normal((bt.B, bt.n)), rng.standard_normal((bt.B, bt.m))
        for mode in MODES:
            assert bt.sens_penalty == 0.0
            slow = call(ctx, bt, mode, sides, gx, gy)
            set_floor(bt, REC)
            fast = call(ctx, bt, mode, sides, gx, gy)
            set_floor(bt, 0.0)
            print("SENS-PASSES | %s | %s | floor 0: %s | floor %g: %s" % (ctx.kind, mode, histogram(slow["passes"]), REC, histogram(fast["passes"])))
            capped = (slow["flag"] == 1) & (slow["passes"] == 200)
            assert capped.any(), mode                                       # (not vacuous: the cap is there without the floor)
            assert np.all(fast["flag"] == 0), (mode, fast["flag"])
            assert int(fast["passes"].sum()) < int(slow["passes"].sum())
            assert np.array_equal(fast["active"], slow["active"]) and np.array_equal(fast["active"], sides)
            if mode == "polish":
                for b, (p, side, _, _) in enumerate(planted):
                    judge_polish(ctx, "loose[%d]" % b, p, side, *stored[b], fast, b, improves=False)
        # ... and by the engine's own rule on the stored solution (sigma_inv of the solve): the same set with either floor
        by_rule = call(ctx, bt, "polish", None, gx, gy)["active"]
        set_floor(bt, REC)
        assert np.array_equal(call(ctx, bt, "polish", None, gx, gy)["active"], by_rule)
    finally:
        ctx.set_option("max_slots", 512)


# ---- 3. accuracy at every size ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_accuracy_with_the_recommended_floor(ctx, case):
    p, side, xs, ys = R.planted_qp(case.n, case.m, case.nact, 9000 + 7 * case.n + case.nact, sides=case.sides, equality=case.equality)
    bt = solved(ctx, [p], warm=(xs[None, :], ys[None, :]) if case.n >= 192 else None, scaling=case.scaling, proximal=case.proximal)
    set_floor(bt, REC)
    assert_instance(ctx, bt, 256 if case.n <= 256 else 512)
    x, y = bt.solution_of(0)
    assert_complementary(p, side, x, y)
    rng = np.random.default_rng(case.n)
    gx, gy = rng.standard_normal((1, case.n)), (rng.standard_normal((1, case.m)) if case.gy else None)
    adj = run_adjoint(ctx, bt, gx, gy, side[None, :])
    judge_adjoint(ctx, "floor-" + case.id, p, side, x, y, gx[0], None if gy is None else gy[0], adj)
    duality(ctx, bt, [(p, side)], gx, gy if gy is not None else np.zeros((1, case.m)), side[None, :], adj if gy is not None else None, "floor-" + case.id)


def duality(ctx, bt, members, gx, gy, sides, adj, what):
    """<gx, dx> + <gy, dy> = <adjoint outputs of (gx, gy), direction>, to the tolerance of tests/test_tangent.py's duality check"""
    rng = np.random.default_rng(22)
    dirs = [TR.direction(p, rng) for p, _ in members]
    tan = run_tangent(ctx, bt, batch_direction(bt, dirs), sides)
    if adj is None:
        adj = run_adjoint(ctx, bt, gx, gy, sides)
    assert np.all(tan["flag"] == 0) and np.all(adj["flag"] == 0)
    assert np.all(tan["passes"] <= PASS_BOUND) and np.all(adj["passes"] <= PASS_BOUND), (tan["passes"], adj["passes"])
    for b, (p, side) in enumerate(members):
        n, m = p.n, p.m
        x, y = bt.solution_of(b)
        _, J, scale_t, err_t = tangent_measure(p, side, x, y, dirs[b])
        za, z64a, _ = R.reference(p, side, gx[b, :n], gy[b, :m])
        scale_a = float(np.max(np.abs(za))) or 1.0
        err_a = float(np.max(np.abs(z64a - za))) / scale_a
        lhs = np.asarray(gx[b, :n], dtype=LD) @ tan["dx"][b, :n] + np.asarray(gy[b, :m], dtype=LD) @ tan["dy"][b, :m]
        rhs = TR.pairing(dirs[b], {k: adj[k][b, :len(dirs[b][k])] for k in TR.KEYS})
        bound = 8.0 * (err_t * scale_t * (np.sum(np.abs(gx[b, :n])) + np.sum(np.abs(gy[b, :m][J]))) + err_a * scale_a * TR.norm1(dirs[b]))
        print("SENS-DUAL | %s | %s[%d] | gap %.2e | bound %.2e" % (ctx.kind, what, b, float(abs(lhs - rhs)), bound))
        assert abs(lhs - rhs) <= bound


def test_accuracy_no_active_row_no_constraint_and_a_padded_member(ctx):
    """|J| = 0 and a sized member inside a larger batch (mixed sizes: every member but the first is padded); then a batch with m = 0"""
    dims = [(33, 50, 20), (20, 30, 0), (5, 8, 3)]
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate(dims)]
    bt = solved(ctx, [q[0] for q in planted], scaling=10)
    set_floor(bt, REC)
    rng = np.random.default_rng(5)
    gx, gy = rng.standard_normal((bt.B, bt.n)), rng.standard_normal((bt.B, bt.m))
    sides = padded([q[1] for q in planted], bt.m, np.int64)
    adj = run_adjoint(ctx, bt, gx, gy, sides)
    pol = run_polish(ctx, bt, sides)
    assert np.all(pol["passes"] <= PASS_BOUND), pol["passes"]
    for b, (p, side, _, _) in enumerate(planted):
        x, y = bt.solution_of(b)
        assert_complementary(p, side, x, y)
        judge_adjoint(ctx, "floor-mixed[%d]" % b, p, side, x, y, gx[b, :p.n], gy[b, :p.m], adj, b)
        judge_polish(ctx, "floor-mixed[%d]" % b, p, side, x, y, pol, b, improves=False)
    duality(ctx, bt, [(q[0], q[1]) for q in planted], gx, gy, sides, adj, "floor-mixed")
    # m = 0: nothing for the floor to act on
    p0 = R.planted_qp(12, 20, 0, 9990)[0]
    e = np.zeros(0)
    p0 = dataclasses.replace(p0, m=0, Ap=np.zeros(13, np.int64), Ai=np.zeros(0, np.int64), Ax=e, bmin=e, bmax=e)
    b0 = solved(ctx, [p0], scaling=10)
    g0 = rng.standard_normal((1, 12))
    want = b0.adjoint_device(T(ctx, g0), want=("dq", "flag", "passes"))
    set_floor(b0, REC)
    got = b0.adjoint_device(T(ctx, g0), want=("dq", "flag", "passes"))
    assert int(N(got["flag"])[0]) == 0 and all(np.array_equal(N(got[k]), N(want[k])) for k in got)
    u = np.linalg.solve(p0.Q_full().toarray(), g0[0])
    assert np.max(np.abs(-N(got["dq"])[0] - u)) <= 1e-12 * np.max(np.abs(u))


def test_accuracy_on_the_sparse_factor(ctx):
    p, side, _, _ = R.replant(blocks_qp(43, 2)[0], 10, 77)
    ctx.set_option("sparse_factor", 1)
    try:
        bt = solved(ctx, [p], scaling=10)
        assert bt.sparse_info(0)[0] > 0
        set_floor(bt, REC)
        x, y = bt.solution_of(0)
        assert_complementary(p, side, x, y)
        rng = np.random.default_rng(3)
        gx, gy = rng.standard_normal((1, p.n)), rng.standard_normal((1, p.m))
        adj = run_adjoint(ctx, bt, gx, gy, side[None, :])
        judge_adjoint(ctx, "floor-sparse", p, side, x, y, gx[0], gy[0], adj)
        duality(ctx, bt, [(p, side)], gx, gy, side[None, :], adj, "floor-sparse")
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 3b. a floor that binds costs few passes, on every form of the assembly --------------------------------------------------------------------
FORMS = [("n65-128", Case(65, 32, 20, 10, 0), 128), ("n193-256", Case(193, 386, 90, 10, 1), 256), ("n257-512", Case(257, 514, 256, 0, 1, equality=True), 512),
         ("narrow-rows", None, 256), ("sparse", None, 512)]


@pytest.mark.parametrize("name,case,threads", FORMS, ids=[f[0] for f in FORMS])
def test_a_binding_floor_costs_few_passes_on_every_form_of_the_assembly(ctx, name, case, threads):
    """the wide form_schur on the three dense instances, form_schur_narrow (an MPC problem: rows of A of a handful of entries) and sp_factor: the floor
    binds on a row of J, and every call converges within PASS_BOUND and in no more passes than with the solve's own penalties (the contraction
    1 / (1 + sigma lambda) only improves when sigma grows; the count may move by one where a residual sits at the threshold)"""
    ctx.set_option("small_workgroups", 2 if threads == 128 else 1)
    if name == "sparse":
        ctx.set_option("sparse_factor", 1)
    try:
        if name == "sparse":
            p, side, xs, ys = R.replant(blocks_qp(43, 2)[0], 10, 61)
            bt = solved(ctx, [p], scaling=10)
            assert bt.sparse_info(0)[0] > 0
        elif name == "narrow-rows":
            from qpalm_amd.problems import random_mpc_qp
            p = random_mpc_qp(T=4, nx=6, nu=3, seed=3)
            bt = solved(ctx, [p], scaling=10)
            # the host's condition for form_schur_narrow (qpg_batch_setup): rows of at most 16 entries on average, four column buffers per wavefront in LDS
            _, thr, lds = bt.launch_shape()
            assert len(p.Ax) <= 16 * p.m and 4 * (thr // 64) * p.n * 8 <= lds
            side = None
        else:
            p, side, xs, ys = R.planted_qp(case.n, case.m, case.nact, 9000 + 7 * case.n + case.nact, sides=case.sides, equality=case.equality)
            bt = solved(ctx, [p], warm=(xs[None, :], ys[None, :]) if case.n >= 192 else None, scaling=case.scaling, proximal=case.proximal)
        assert int(bt.info(0).status_val) == 1
        if name != "narrow-rows":
            assert_instance(ctx, bt, threads)
        rng = np.random.default_rng(19)
        gx, gy = rng.standard_normal((1, p.n)), rng.standard_normal((1, p.m))
        sides = None if side is None else side[None, :]
        own = {mode: call(ctx, bt, mode, sides, gx, gy) for mode in MODES}
        J = own["adjoint"]["active"][0, :p.m] != 0
        sigma = bt.vec("sigma", 0)[:p.m]
        assert J.any() and float(np.min(sigma[J])) < REC                 # the floor binds on a row of J
        set_floor(bt, REC)
        for mode in MODES:
            got = call(ctx, bt, mode, sides, gx, gy)
            print("SENS-FORMS | %s | %s | %s | sigma on J %.3g .. %.3g | passes %d -> %d | resid %.1e" %
                  (ctx.kind, name, mode, float(np.min(sigma[J])), float(np.max(sigma[J])), int(own[mode]["passes"][0]), int(got["passes"][0]), float(got["resid"][0])))
            assert int(own[mode]["flag"][0]) == 0 and int(got["flag"][0]) == 0, mode
            assert int(got["passes"][0]) <= PASS_BOUND, (mode, got["passes"])
            assert int(got["passes"][0]) <= int(own[mode]["passes"][0]) + 1, (mode, own[mode]["passes"], got["passes"])
            assert np.array_equal(got["active"], own[mode]["active"])
    finally:
        ctx.set_option("small_workgroups", 1)
        ctx.set_option("sparse_factor", -1)


# ---- 4. state --------------------------------------------------------------------------------------------------------------------------------------
def penalties(bt):
    out = []
    for b in range(bt.B):
        out += [bt.vec(k, b) for k in ("sigma", "sigma_inv", "sqrt_sigma")] + [bt.named_vec("At_sqrt_sigma", bt.nnzA, b), bt.ivec("active", b)]
    return out


@pytest.mark.parametrize("mode,B,slots", [("dense", 5, 1), ("sparse", 2, 512)])
def test_state_stays_and_the_next_solve_is_bit_identical(ctx, mode, B, slots):
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
        assert (B > G.launch_shape()[0]) == (mode == "dense")             # dense: B beyond the slots
        floor = 4.0 * max(float(np.max(G.vec("sigma", b))) for b in range(B))
        set_floor(G, floor)                                            # binds on every row
        rng = np.random.default_rng(4)
        gx, gy = rng.standard_normal((B, G.n)), rng.standard_normal((B, G.m))
        before, pen, epoch = snapshot(G), penalties(G), G.epoch
        for m_ in MODES:
            out = call(ctx, G, m_, None, gx, gy)
            assert np.all(out["flag"] == 0), m_
            after = penalties(G)
            assert all(np.array_equal(a, b) for a, b in zip(pen, after)), m_
        assert G.epoch == epoch
        assert all(np.array_equal(before[k], v) for k, v in snapshot(G).items())
        for bt in (H, G):
            bt.warm_start_last()
            bt.solve()
        a, b = snapshot(H), snapshot(G)
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not bad, bad
        assert np.all(a["status_val"] == 1)
    finally:
        ctx.set_option("max_slots", 512)
        ctx.set_option("sparse_factor", -1)


# ---- 5. dependent rows (the duplicated-row member of tests/test_adjoint.py::test_dependent_active_rows) -----------------------------------------------
def test_dependent_active_rows(ctx):
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
    set_floor(bt, REC)
    sides = np.zeros((1, 20), np.int64)
    sides[0, i0], sides[0, i1] = -1, -1
    gx = np.ones((1, 12))
    out = run_adjoint(ctx, bt, gx, None, sides)                      # consistent: the unique u, and the sum of the two rows' w
    assert int(out["flag"][0]) == 0
    assert all(np.all(np.isfinite(v)) for v in out.values())
    one = np.zeros(20, int)
    one[i0] = -1
    zr, z64, _ = R.reference(p2, one, gx[0], None)
    scale = float(np.max(np.abs(zr)))
    err64 = float(np.max(np.abs(z64 - zr))) / scale
    zk = np.concatenate([-out["dq"][0], [out["dbmin"][0, i0] + out["dbmin"][0, i1]]])
    errk = float(np.max(np.abs(zk - zr))) / scale
    print("SENS-DEP | %s | err64 %.2e | kernel %.2e | passes %d | resid %.1e" % (ctx.kind, err64, errk, int(out["passes"][0]), float(out["resid"][0])))
    assert errk <= 8 * err64
    gy = np.zeros((1, 20))                                              # inconsistent: no solution, with any preconditioner
    gy[0, i0], gy[0, i1] = 1.0, -1.0
    out = run_adjoint(ctx, bt, gx, gy, sides)
    assert int(out["flag"][0]) == 1
    for k in ("dq", "dbmin", "dbmax", "dQx", "dAx"):
        assert np.all(out[k] == 0), k
    assert all(np.all(np.isfinite(v)) for v in out.values())


# ---- 6. subsets and the layer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_subset_with_a_binding_floor(ctx, mode):
    """B9-slots4: selected members bit for bit the full call's, the rows of the others untouched"""
    ctx.set_option("max_slots", 4)
    try:
        probs = [R.planted_qp(12, 20, 2 + k % 6, 9500 + 11 * k)[0] for k in range(9)]
        bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=1e-3, eps_rel=1e-3, verbose=0, scaling=10))
        bt.solve()
        assert_instance(ctx, bt, 128)
        set_floor(bt, 4.0 * max(float(np.max(bt.vec("sigma", b))) for b in range(9)))
        rng = np.random.default_rng(11)
        gx, gy = rng.standard_normal((9, 12)), rng.standard_normal((9, 20))
        full = call(ctx, bt, mode, None, gx, gy)
        s = (np.arange(9) % 2).astype(np.int64)
        sel = s.astype(bool)
        pre = {k: T(ctx, np.full(v.shape, np.nan if v.dtype.kind == "f" else -7), v.dtype.type) for k, v in full.items()}
        part = call(ctx, bt, mode, None, gx, gy, select=s, out=pre)
        for k in full:
            assert np.array_equal(part[k][sel], full[k][sel]), k
            a = part[k][~sel]
            assert np.all(np.isnan(a)) if a.dtype.kind == "f" else np.all(a == -7), k
    finally:
        ctx.set_option("max_slots", 512)


def test_layer_with_polish_and_a_floor(ctx):
    """the batch of test 2 behind QPLayer(polish=True, sens_penalty=REC): every polish accepted, and the gradients of backward within judge's bound"""
    import torch
    try:
        bt, planted = loose_batch(ctx)
        layer = QPLayer(bt, warm="last", polish=True, sens_penalty=REC)
        v = C.c_double(-1.0)
        assert bt.L.qpg_batch_get_sens_penalty(bt.h, C.byref(v)) == 0 and v.value == REC
        assert QPLayer(bt).batch.sens_penalty == REC                       # None leaves the batch's value alone
        leaf = lambda a: T(ctx, a).requires_grad_(True)
        q = leaf(padded([p[0].q for p in planted], bt.n))
        x, y, status = layer(q)
        assert N(status).tolist() == [1] * 9
        assert N(layer.last_polish["flag"]).tolist() == [0] * 9
        rng = np.random.default_rng(21)
        cx, cy = T(ctx, rng.standard_normal((9, bt.n))), T(ctx, rng.standard_normal((9, bt.m)))
        ((cx * x).sum() + (cy * y).sum()).backward()
        assert N(layer.last_adjoint["flag"]).tolist() == [0] * 9
        own = {k: N(v) for k, v in bt.adjoint_device(cx, cy).items()}      # (the set by the engine's rule, as backward uses it)
        assert torch.equal(q.grad, T(ctx, own["dq"]))
        for b, (p, side, _, _) in enumerate(planted):
            xb, yb = bt.solution_of(b)
            assert np.array_equal(N(x)[b, :p.n], xb[:p.n])
            judge_adjoint(ctx, "floor-layer[%d]" % b, p, side, xb[:p.n], yb[:p.m], N(cx)[b, :p.n], N(cy)[b, :p.m], own, b)
    finally:
        ctx.set_option("max_slots", 512)


# ---- 7. the interface ------------------------------------------------------------------------------------------------------------------------------
def test_interface(ctx):
    bt, planted = small_batch(ctx, B=2)
    probs = [q[0] for q in planted]
    L = bt.L
    assert bt.sens_penalty == 0.0
    bt.sens_penalty = 1e6
    assert bt.sens_penalty == 1e6
    epoch = bt.epoch
    bt.sens_penalty = 2.5
    assert bt.sens_penalty == 2.5 and bt.epoch == epoch
    for bad in (-1.0, -0.0 - 1e-300, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(QpgError) as e:
            bt.sens_penalty = bad
        assert e.value.code == INVALID
        assert bt.sens_penalty == 2.5
    v = C.c_double(-1.0)
    assert L.qpg_batch_set_sens_penalty(None, 1.0) == INVALID and L.qpg_batch_get_sens_penalty(None, C.byref(v)) == INVALID
    # kept across solves, update_settings and update_Q_A_device
    bt.solve()
    bt.update_settings(ctx.default_settings(**dict(ST, eps_abs=1e-8)))
    Qx, Ax = T(ctx, padded([p.Qx for p in probs], bt.nnzQ)), T(ctx, padded([p.Ax for p in probs], bt.nnzA))
    a, b = bt._dev_args((Qx, (bt.B, bt.nnzQ), "Qx", "float64"), (Ax, (bt.B, bt.nnzA), "Ax", "float64"))
    bt.update_Q_A_device(a.value, b.value)
    bt.solve()
    assert bt.sens_penalty == 2.5
    assert np.all(N(bt.adjoint_device(T(ctx, np.ones((2, 12))))["flag"]) == 0)
    # before qpg_batch_setup: a batch that has only been created
    h = C.c_void_p()
    st = ctx.default_settings(**ST)
    assert L.qpg_batch_create(ctx.h, 1, 12, 20, 40, 40, C.byref(st), C.byref(h)) == 0
    try:
        assert L.qpg_batch_set_sens_penalty(h, 1e4) == 0
        assert L.qpg_batch_get_sens_penalty(h, C.byref(v)) == 0 and v.value == 1e4
        assert L.qpg_batch_set_sens_penalty(h, -1.0) == INVALID
        assert L.qpg_batch_get_sens_penalty(h, C.byref(v)) == 0 and v.value == 1e4
    finally:
        L.qpg_batch_destroy(h)
    for s in ("qpg_batch_set_sens_penalty", "qpg_batch_get_sens_penalty"):
        assert s in capi.SYMBOLS


def test_refused_batches_store_the_floor_and_still_refuse(ctx):
    bt, _ = small_batch(ctx, factorization_method=0)
    bt.solve()
    set_floor(bt, 1e6)
    with pytest.raises(QpgError) as e:
        bt.adjoint_device(T(ctx, np.ones((1, 12))))
    assert e.value.code == UNSUPPORTED and "dense KKT" in str(e.value)

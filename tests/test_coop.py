"""Coop mode (BASELINE.json configs 2 and 5 as written: ONE large QP on one MI355X): the QP's iteration stays on its workgroup but
suspends at its linear-algebra site, and the host chains multi-workgroup kernels for the Schur assembly, the blocked LDL' (panel
update on the matrix cores by row tiles / diagonal block / rows below: two launches per 32 columns), the rank updates (one launch
per 32 columns: every workgroup repeats the diagonal block's recurrence, then updates its rows) and the triangular solves (one
launch per 64-column block), qpalm_capi.inc: coop_solve.  Reference: src/solver_interface.c:319-519 (the same factorise / update / solve
calls), src/nonconvex.c:29-168 for config 5's front-end.

Parity: against the one-workgroup engine (same statuses, iteration counts and refactorise / rank-update split, x, y to 1e-9; the
factorisation, the updates -- where the one-workgroup sweep takes 16 ranks at a time like the grid's, not 8 -- and the forward
substitution are bit-identical per entry, the backward substitution sums in another order) and against the oracle.  The bit-identity statements themselves -- L and D of the grid kernels against the one-workgroup
kernels', the one-launch sweep against the chain of launches, operation by operation at the block edges -- are asserted in
tests/test_coop_ops_exact.py."""
import time

import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import binding as ob
from qpalm_amd.problems import random_qp
from qpalm_amd.solver import QpalmBatch
from tests.helpers import STATUS
from tests.test_parity import RTOL, rel, sizes


def _solve(ctx, probs, st, coop, policy=-1):
    ctx.set_option("coop", 1 if coop else 0)
    ctx.set_option("coop_rank_threshold", policy)   # -1: the reference's refactorise-or-update rule (the default, -2, goes by measured cost)
    try:
        bt = QpalmBatch(ctx, probs, ctx.default_settings(**st))
        t0 = time.perf_counter()
        bt.solve()
        dt = time.perf_counter() - t0
        x, y = bt.solution()
        return bt, x, y, dt
    finally:
        ctx.set_option("coop", 0)
        ctx.set_option("coop_rank_threshold", -2)


@pytest.mark.parametrize("extra", [dict(), dict(enable_dual_termination=1), dict(proximal=0, scaling=2)])
def test_coop_matches_single_workgroup_and_oracle(ctx, extra):
    n, m = sizes(ctx, (70, 100), (1000, 2000))    # emu: three block columns (two full, one ragged)
    nb = sizes(ctx, 1, 2)
    probs = [random_qp(n, m, seed=1000 + k, density_A=0.01 if n >= 400 else 4.0 / n, density_M=0.005 if n >= 400 else 2.0 / n) for k in range(nb)]
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, **extra)
    b1, x1, y1, _ = _solve(ctx, probs, st, coop=False)
    b2, x2, y2, _ = _solve(ctx, probs, st, coop=True)
    b3, x3, y3, _ = _solve(ctx, probs, st, coop=True, policy=-2)   # default policy: below 2048 rows every changed active set refactorises
    for k, p in enumerate(probs):
        assert int(b3.info(k).status_val) == int(b2.info(k).status_val) and int(b3.info(k).iter) == int(b2.info(k).iter)
        assert rel(x3[k], x2[k]) <= RTOL and rel(y3[k], y2[k]) <= RTOL and int(b3.stats(k).n_rank1) == 0
        o = ob.OracleQP(*p.args(), settings=ob.default_settings(**st))
        o.solve()
        i1, i2, s2 = b1.info(k), b2.info(k), b2.stats(k)
        assert int(i2.status_val) == int(i1.status_val) == o.status_val
        assert int(i2.iter) == int(i1.iter) == int(o.info.iter) and int(i2.iter_out) == int(o.info.iter_out)
        assert rel(x2[k], x1[k]) <= RTOL and rel(y2[k], y1[k]) <= RTOL
        assert rel(x2[k], o.x) <= RTOL and rel(y2[k], o.y) <= RTOL
        assert abs(i2.objective - o.info.objective) <= 1e-9 * max(1.0, abs(o.info.objective))
        if extra.get("enable_dual_termination"):
            assert abs(i2.dual_objective - o.info.dual_objective) <= 1e-9 * max(1.0, abs(o.info.dual_objective))
        s1 = b1.stats(k)
        assert int(s2.n_refactor) == int(s1.n_refactor) >= 1 and int(s2.n_rank1) == int(s1.n_rank1) > 0 and int(s2.n_factor_Q) == int(s1.n_factor_Q)
        assert int(s2.n_refactor) == o.counter("n_refactor") and int(s2.n_rank1) == o.counter("n_rank1")
        assert np.array_equal(b2.ivec("active", k), o.ivec("active"))


def test_coop_update_sweep_in_one_launch_equals_the_chain_of_launches(ctx):
    """coop_updates = 2 (default): a rank-update sweep is ONE launch, a workgroup owns 128 rows for the whole sweep and the owners of the
    diagonal blocks hand their tables down through a counter; = 1: one launch per 32-column block.  Same arithmetic per entry: the two
    must agree BIT FOR BIT (x, y and the counts), and with the one-workgroup path to rounding.  Sizes: three / eight row chunks, the last
    one ragged; more than 16 ranks in some iterations (two sweeps)."""
    n, m = sizes(ctx, (260, 300), (1000, 2000))
    p = random_qp(n, m, seed=4242, density_A=0.01 if n >= 400 else 4.0 / n, density_M=0.005 if n >= 400 else 2.0 / n)
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    res = {}
    try:
        for cu in (2, 1):
            ctx.set_option("coop_updates", cu)
            bt, x, y, _ = _solve(ctx, [p], st, coop=True)
            res[cu] = (int(bt.info(0).status_val), int(bt.info(0).iter), int(bt.stats(0).n_rank1), int(bt.stats(0).n_refactor), x[0].copy(), y[0].copy())
            bt.close()
    finally:
        ctx.set_option("coop_updates", 2)
    assert res[2][:4] == res[1][:4] and res[2][0] == 1 and res[2][2] > 0
    assert np.array_equal(res[2][4], res[1][4]) and np.array_equal(res[2][5], res[1][5])
    b1, x1, y1, _ = _solve(ctx, [p], st, coop=False)
    assert int(b1.info(0).iter) == res[2][1] and rel(res[2][4], x1[0]) <= RTOL and rel(res[2][5], y1[0]) <= RTOL
    b1.close()


def test_coop_update_sweep_survives_a_workgroup_that_gives_up(ctx):
    """a workgroup of the one-launch sweep that gives up waiting for a table (bounded spin) used to return with the factor half
    updated, every later workgroup waited out a timeout of its own, and the solver iterated on the corrupt factor until the host looked at
    the mark after the WHOLE solve.  Now the mark makes the workgroups behind it leave at once, and the iteration kernel that resumes after
    the sweep sees it, clears it and takes the Newton step again with a fresh factorisation.  The test hook `coop_test_kill = N` makes the
    second workgroup of the N-th sweep of the solve give up at once: the solve must still end SOLVED at the oracle's solution, with the
    rebuilt factor counted (n_guard_refactor), and the next solve of the same batch must not see a stale mark."""
    n, m = sizes(ctx, (260, 300), (700, 1400))
    p = random_qp(n, m, seed=4242, density_A=0.01 if n >= 400 else 4.0 / n, density_M=0.005 if n >= 400 else 2.0 / n)
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    o = ob.OracleQP(*p.args(), settings=ob.default_settings(**st))
    o.solve()
    ctx.set_option("coop", 1)
    ctx.set_option("coop_rank_threshold", -1)   # the reference's refactorise-or-update rule: rank updates at this size
    try:
        ctx.set_option("coop_test_kill", 2)
        bt = QpalmBatch(ctx, [p], ctx.default_settings(**st))
        bt.solve()
        x, y = bt.solution()
        assert int(bt.info(0).status_val) == 1 and int(bt.stats(0).n_guard_refactor) == 1, (bt.info(0).status_val, bt.stats(0).n_guard_refactor)
        assert rel(x[0], o.x) <= 1e-8 and rel(y[0], o.y) <= 1e-8
        assert int(bt.info(0).iter) == int(o.info.iter)            # the rebuilt factor is that of the same matrix: the path does not change
        ctx.set_option("coop_test_kill", 0)
        bt.warm_start(None, None)
        bt.solve()
        x2, y2 = bt.solution()
        assert int(bt.info(0).status_val) == 1 and int(bt.stats(0).n_guard_refactor) == 0
        assert rel(x2[0], o.x) <= RTOL and rel(y2[0], o.y) <= RTOL and int(bt.info(0).iter) == int(o.info.iter)
        bt.close()
    finally:
        ctx.set_option("coop_test_kill", 0)
        ctx.set_option("coop_rank_threshold", -2)
        ctx.set_option("coop", 0)


def test_coop_members_of_different_sizes_and_repeated_solves(ctx):
    """two QPs of different sizes in one coop batch, solved three times (on the GPU the launch chains of each member are recorded
    during the second solve and replayed as graphs in the third): every solve against the oracle"""
    (n1, m1), (n2, m2) = sizes(ctx, ((70, 100), (45, 80)), ((900, 1500), (700, 1000)))
    probs = [random_qp(n1, m1, seed=301, density_A=max(0.01, 4.0 / n1), density_M=max(0.005, 2.0 / n1)),
             random_qp(n2, m2, seed=302, density_A=max(0.01, 4.0 / n2), density_M=max(0.005, 2.0 / n2))]
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    ctx.set_option("coop", 1)
    try:
        bt = QpalmBatch(ctx, probs, ctx.default_settings(**st))
        for rep in range(3):
            if rep:
                bt.warm_start(None, None)
            bt.solve()
            x, y = bt.solution()
            for k, p in enumerate(probs):
                o = ob.OracleQP(*p.args(), settings=ob.default_settings(**st))
                o.solve()
                assert int(bt.info(k).status_val) == o.status_val == 1 and int(bt.info(k).iter) == int(o.info.iter), (rep, k)
                assert rel(x[k][:p.n], o.x) <= RTOL and rel(y[k][:p.m], o.y) <= RTOL, (rep, k)
    finally:
        ctx.set_option("coop", 0)


def test_coop_time_limit_counts_the_grid_kernels(ctx):
    """info.solve_time / run_time and the time_limit check see WALL time in coop mode (qpalm.c:680-723): the time of the host-chained
    factorisation / update / solve kernels between two launches of the iteration kernel is added on resume (qpg_scalars.pend_clock)"""
    n, m = sizes(ctx, (70, 100), (1000, 2000))
    p = random_qp(n, m, seed=1003, density_A=0.01 if n >= 400 else 4.0 / n, density_M=0.005 if n >= 400 else 2.0 / n)
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    bt, _, _, dt = _solve(ctx, [p], st, coop=True)
    info = bt.info(0)
    assert int(info.status_val) == STATUS["SOLVED"]
    if ctx.kind == "hip":   # (the emulator's clock is the host's: its kernels take no device time between launches)
        assert 0.5 * dt <= float(info.solve_time) <= 1.05 * dt, (float(info.solve_time), dt)
        assert int(bt.stats(0).n_sweeps) >= 0
    # a limit far below one solve: stops with TIME_LIMIT_REACHED after a few iterations, not after the whole solve
    iters_full = int(info.iter)
    limit = sizes(ctx, 1e-7, 0.25 * float(info.solve_time))
    b2, _, _, _ = _solve(ctx, [p], dict(st, time_limit=limit), coop=True)
    assert int(b2.info(0).status_val) == STATUS["TIME_LIMIT_REACHED"]
    assert int(b2.info(0).iter) < iters_full


def test_coop_is_selected_automatically_for_one_large_qp(ctx):
    """default policy (coop = -1): one QP with a factor of at least 640 rows (two to four from 1536 rows on: smaller ones are better off on a workgroup each, measured in round 5); small or many QPs keep the batch engine"""
    n, m = sizes(ctx, (40, 60), (1400, 1500))
    p = random_qp(n, m, seed=77, density_A=max(0.01, 4.0 / n), density_M=max(0.005, 2.0 / n))
    ctx.set_option("coop", -1)
    try:
        bt = QpalmBatch(ctx, [p], ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0))
        bt.solve()
        s = bt.stats(0)
        if ctx.kind == "emu":
            assert int(s.n_rank1) > 0 and int(s.n_fused_solve) > 0    # n = 40: not selected
        else:
            assert int(s.n_refactor) > 1 and int(s.n_rank1) == 0 and int(s.n_fused_solve) == 0   # selected: below 2048 rows the grid refactorises instead of updating
        assert int(bt.info(0).status_val) == STATUS["SOLVED"]
    finally:
        ctx.set_option("coop", 0)


def test_coop_nonconvex(ctx):
    """config 5's shape at test size: indefinite Q, LOBPCG front-end, proximal penalty 1/|lambda|; against the oracle"""
    n, m = sizes(ctx, (36, 40), (600, 900))
    p = random_qp(n, m, seed=5, density_A=max(0.01, 4.0 / n), density_M=max(0.005, 2.0 / n))
    Q = sp.csc_matrix((p.Qx, p.Qi, p.Qp), shape=(n, n)).tolil()
    for j in range(0, n, 3):
        Q[j, j] = Q[j, j] - 3.0 * abs(Q[j, j])     # negative curvature in a third of the directions
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    p2 = type(p)(n, m, Q.indptr.astype(np.int64), Q.indices.astype(np.int64), Q.data.copy(), p.Ap, p.Ai, p.Ax, p.q, p.bmin, p.bmax)
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, nonconvex=1, max_iter=sizes(ctx, 60, 2000))
    b1, x1, y1, _ = _solve(ctx, [p2], st, coop=False)
    b2, x2, y2, _ = _solve(ctx, [p2], st, coop=True)
    o = ob.OracleQP(*p2.args(), settings=ob.default_settings(**st))
    o.solve()
    assert int(b2.stats(0).nonconvex) == 1
    assert int(b2.info(0).status_val) == int(b1.info(0).status_val) == o.status_val
    assert int(b2.info(0).iter) == int(b1.info(0).iter) == int(o.info.iter)
    assert rel(x2[0], o.x) <= 1e-8 and rel(y2[0], o.y) <= 1e-8


@pytest.mark.gpu
def test_coop_large_factor_against_oracle():
    """n = 2500 (the large-factor sweep's size class, the same QP as test_large_factor_path) in coop mode against the oracle:
    reference rule (-1): status, iteration counts, refactorise / rank-update split, active set, x and y; default rule: x and y."""
    from qpalm_amd.solver import Context
    ctx = Context(0)
    p = random_qp(2500, 3200, seed=11, density_A=0.004, density_M=0.002)
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    o = ob.OracleQP(*p.args(), settings=ob.default_settings(**st))
    o.solve()
    for policy in (-1, -2):
        bt, x, y, _ = _solve(ctx, [p], st, coop=True, policy=policy)
        info, s = bt.info(0), bt.stats(0)
        assert int(info.status_val) == o.status_val == 1 and int(info.iter) == int(o.info.iter) and int(info.iter_out) == int(o.info.iter_out)
        assert rel(x[0], o.x) <= RTOL and rel(y[0], o.y) <= RTOL
        assert np.array_equal(bt.ivec("active", 0), o.ivec("active"))
        if policy == -1:
            assert int(s.n_refactor) == o.counter("n_refactor") and int(s.n_rank1) == o.counter("n_rank1") > 0
        assert int(s.n_fused_solve) == 0
        bt.close()


@pytest.mark.gpu
def test_config2_single_qp_latency():
    """BASELINE.json config 2 as written: ONE random convex QP, n = 1000, m = 2000, on one MI355X, default policy (automatic from
    640 rows; at this size every changed active set refactorises on the grid): measured 37.6 ms against 62.3 ms on one workgroup
    (n = 2500: 123 vs 1546 ms, n = 5000: 0.35 vs ~7 s).  The test pins parity with the oracle and an upper bound on the time."""
    from qpalm_amd.solver import Context
    ctx = Context(0)
    p = random_qp(1000, 2000, seed=1000, density_A=0.01, density_M=0.005)
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    ctx.set_option("coop", -1)
    bt = QpalmBatch(ctx, [p], ctx.default_settings(**st))
    bt.solve()                                    # warm-up (code objects, allocations)
    t = []
    for _ in range(3):
        bt.warm_start(None, None)
        t0 = time.perf_counter()
        bt.solve()
        t.append(time.perf_counter() - t0)
    o = ob.OracleQP(*p.args(), settings=ob.default_settings(**st))
    o.solve()
    x, y = bt.solution()
    assert int(bt.info(0).status_val) == o.status_val == 1 and int(bt.info(0).iter) == int(o.info.iter)
    assert rel(x[0], o.x) <= RTOL and rel(y[0], o.y) <= RTOL
    print("config 2, one QP, coop: %.1f ms per solve (best of 3), %d iterations" % (1e3 * min(t), int(bt.info(0).iter)))
    assert min(t) <= 0.080 and int(bt.stats(0).n_fused_solve) == 0, t   # (no fused solves: the grid ran it)


@pytest.mark.gpu
def test_config5_nonconvex_n5000():
    """BASELINE.json config 5 as written: nonconvex random QP, n = 5000, LOBPCG + indefinite LDL' on one MI355X (one workgroup:
    145 s in round 2).  The front-end against the oracle at full size (lobpcg + set_settings_nonconvex run in the oracle's setup, which
    takes seconds: lambda to 1e-11, iteration count exact) and against numpy (lambda is a lower bound of the smallest eigenvalue of
    the SCALED Hessian c D Q D -- D, c read back from the device -- within LOBPCG's own residual bound, nonconvex.c:150-160); the
    solve at eps 1e-6 like every other config: stationarity / feasibility of the returned point with numpy on the unscaled data
    (the oracle's solve at this size is minutes of CPU), and the solve time."""
    from qpalm_amd.solver import Context
    ctx = Context(0)
    from qpalm_amd.problems import config5_qp
    n, m = 5000, 5000
    p2 = config5_qp(n, m)
    Q = sp.csc_matrix((p2.Qx, p2.Qi, p2.Qp), shape=(n, n))
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, nonconvex=1, max_iter=40000)
    ctx.set_option("coop", 1)
    ctx.set_option("coop_rank_threshold", -1)   # the reference's refactorise-or-update rule: the split of the golden fixture
    bt = QpalmBatch(ctx, [p2], ctx.default_settings(**st))
    s0 = bt.stats(0)
    # ---- the front-end alone, at size: oracle (setup only) and numpy ----
    o = ob.OracleQP(*p2.args(), settings=ob.default_settings(**st))
    assert abs(s0.lobpcg_lambda - o.scalar("lobpcg_lambda")) <= 1e-11 * max(1.0, abs(o.scalar("lobpcg_lambda"))), (s0.lobpcg_lambda, o.scalar("lobpcg_lambda"))
    assert int(s0.lobpcg_iter) == o.counter("n_lobpcg_iter") and int(s0.nonconvex) == o.counter("nonconvex") == 1
    o.cleanup()
    Qfull = (sp.tril(Q) + sp.tril(Q, -1).T).toarray()
    D, c = bt.vec("D", 0), float(s0.sc_c)
    lam_min = np.linalg.eigvalsh(c * (D[:, None] * Qfull * D[None, :]))[0]
    # lobpcg stops at ||Q x - lambda x||_inf < 1e-5 and returns lambda - sqrt(2) ||residual||_2 - 1e-6: below lambda_min by at most that
    assert lam_min < 0 and s0.lobpcg_lambda <= lam_min + 1e-9, (s0.lobpcg_lambda, lam_min)
    assert lam_min - s0.lobpcg_lambda <= np.sqrt(2.0) * np.sqrt(n) * 1e-5 + 2e-6 + 1e-4 * abs(lam_min), (s0.lobpcg_lambda, lam_min)
    # ---- the solve ----
    t0 = time.perf_counter()
    bt.solve()
    dt = time.perf_counter() - t0
    info, s = bt.info(0), bt.stats(0)
    print("config 5, n = 5000 nonconvex, coop: %.2f s, %d iterations, status %d, lambda %.6f (lambda_min of the scaled Hessian %.6f)" % (
        dt, int(info.iter), int(info.status_val), s.lobpcg_lambda, lam_min))
    assert int(s.nonconvex) == 1 and int(info.status_val) == STATUS["SOLVED"]
    x, y = bt.solution()
    A = sp.csc_matrix((p2.Ax, p2.Ai, p2.Ap), shape=(m, n))
    ax = A @ x[0]
    prim = np.max(np.maximum(p2.bmin - ax, 0) + np.maximum(ax - p2.bmax, 0))
    grad = Qfull @ x[0] + p2.q + A.T @ y[0]
    assert prim <= 1e-5 * max(1.0, np.max(np.abs(ax)))
    assert np.max(np.abs(grad)) <= 1e-4 * max(1.0, np.max(np.abs(Qfull @ x[0])), np.max(np.abs(p2.q)))
    assert dt <= 120.0, dt   # 136.8 s before the rank updates moved to the grid, 34 s at eps 1e-5 at the end of round 3 (own rule; the reference's rule: 46.6 s)
    # ---- the solve against the ORACLE at size (round 5): tests/golden/config5_n5000.npz, written once in the build container by
    # tests/golden/make_config5_fixture.py (hours of one CPU core: the oracle factorises dense 5000 x 5000 panels) ----
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config5_n5000.npz")
    if not os.path.exists(gold):
        pytest.skip("tests/golden/config5_n5000.npz is missing (python tests/golden/make_config5_fixture.py, build container only): properties checked, oracle comparison skipped")
    g = np.load(gold)
    assert int(g["status_val"]) == int(info.status_val) == 1
    print("config 5 against the oracle: iterations %d / %d, outer %d / %d, refactorisations %d / %d, rank-1 updates %d / %d, dx %.2e dy %.2e" % (
        int(info.iter), int(g["iter"]), int(info.iter_out), int(g["iter_out"]), int(s.n_refactor), int(g["n_refactor"]), int(s.n_rank1), int(g["n_rank1"]),
        rel(x[0], g["x"]), rel(y[0], g["y"])))
    assert int(info.iter) == int(g["iter"]) and int(info.iter_out) == int(g["iter_out"])
    assert int(s.n_refactor) == int(g["n_refactor"]) and int(s.n_rank1) == int(g["n_rank1"])
    assert rel(x[0], g["x"]) <= 1e-8 and rel(y[0], g["y"]) <= 1e-8
    assert abs(s.lobpcg_lambda - float(g["lobpcg_lambda"])) <= 1e-11 * max(1.0, abs(float(g["lobpcg_lambda"])))
    ctx.set_option("coop_rank_threshold", -2)

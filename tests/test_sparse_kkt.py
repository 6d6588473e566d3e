"""The sparse L D L' of the KKT matrix (context option "sparse_kkt" = 1, qpalm_amd/csrc/qpalm_sparse_kkt.h): FACTORIZE_KKT batches keep
P K P' = L D L' on the pattern of K_full (every row of A present), ordered by nested dissection with the dense rows of A last, and enter / leave
constraints by sparse row additions / deletions (ladel_row_add / ladel_row_del, src/solver_interface.c:202-236) instead of a dense panel.

Yardstick: the oracle's KKT mode (dense, natural order) -- statuses, iteration counts, refactorisation and row-operation counts and active sets
exact, x and y to 1e-9 relative; the row operations on their own against K built in numpy; at sizes the oracle cannot take, the KKT
conditions of the returned point checked with scipy.  Every test sets "sparse_kkt" and "sparse_ordering" itself and restores them."""
import contextlib
import time

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import binding as ob
from qpalm_amd.capi import QpgError
from qpalm_amd.problems import fixture_qp, random_qp, sparse_qp
from qpalm_amd.solver import QpalmBatch
from tests.fuzz_cases import cases, judge_case, run_case
from tests.helpers import STATUS
from tests.test_kkt_path import _check, _pair
from tests.test_parity import RTOL, gsettings, rel, sizes

ST = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, factorization_method=0)
UNSUPPORTED = -5
HIP_ONLY = pytest.mark.parametrize("ctx", [pytest.param("hip", marks=pytest.mark.gpu, id="hip")], indirect=True)


@contextlib.contextmanager
def sparse_kkt(ctx, ordering=-1, on=1):
    ctx.set_option("sparse_kkt", on)
    ctx.set_option("sparse_ordering", ordering)
    try:
        yield
    finally:
        ctx.set_option("sparse_kkt", 0)
        ctx.set_option("sparse_ordering", -1)


def _problem(kind, n):
    if kind == "random":
        return random_qp(n, int(1.5 * n), seed=11, density_A=max(0.02, 3.0 / n), density_M=max(0.01, 2.0 / n))
    if kind == "blocks+budget3":
        return sparse_qp(n, "blocks+budget", seed=3, dense_rows=3)
    return sparse_qp(n, kind, seed=3)


def test_sparse_kkt_batches_exist(ctx):
    """the option, qpg_batch_sparse_info / _perm on a KKT batch (n + m entries), and a factor beyond the dense panel's 8192 rows"""
    p = sparse_qp(sizes(ctx, 120, 200), "banded+budget", seed=1)      # (n > 90: the budget row's degree makes it a hub of K's graph)
    big = sparse_qp(5000, "banded+budget", seed=2)
    assert big.n + big.m > 8192
    with pytest.raises(QpgError) as e:    # the default: KKT keeps the dense panel, which refuses this size
        QpalmBatch(ctx, [big], ctx.default_settings(**ST))
    assert e.value.code == UNSUPPORTED
    with sparse_kkt(ctx):
        bt = QpalmBatch(ctx, [p], ctx.default_settings(**ST))
        nnz, dev = bt.sparse_info(0)
        perm, lev = bt.sparse_perm(0)
        assert nnz > 0 and dev > 0 and 0 < lev < p.n + p.m
        assert len(perm) == p.n + p.m and np.array_equal(np.sort(perm), np.arange(p.n + p.m))
        assert perm[-1] == p.n + p.m - 1          # the budget row (the last constraint) is a high-degree vertex: ordered last
        with pytest.raises(QpgError):
            bt.factor(0)                          # a sparse factor is not read back as a dense panel
        bt.close()
        t0 = time.perf_counter()
        bt = QpalmBatch(ctx, [big], ctx.default_settings(**ST))
        nnz, dev = bt.sparse_info(0)
        nf = big.n + big.m
        print("banded+budget n = %d, n + m = %d: nnz(L) = %d (%.1f per row), levels %d, setup %.2f s"
              % (big.n, nf, nnz, nnz / nf, bt.sparse_perm(0)[1], time.perf_counter() - t0))
        assert nnz <= 12 * nf                    # measured: 10.1 per row
        if ctx.kind == "hip":
            bt.solve()
            assert int(bt.info(0).status_val) == STATUS["SOLVED"]
        bt.close()


@pytest.mark.parametrize("ordering", [0, -1])
@pytest.mark.parametrize("kind", ["random", "blocks", "banded", "arrow", "banded+budget", "blocks+budget3"])
def test_parity_with_the_oracle_kkt_mode(ctx, kind, ordering):
    """against the oracle's dense natural-order KKT mode: status, iter, iter_out, n_refactor, row operations, active set exact; x, y 1e-9"""
    p = _problem(kind, sizes(ctx, 48, 200))
    with sparse_kkt(ctx, ordering):
        o, bt = _pair(ctx, p, ST)
        o.solve(); bt.solve()
        assert o.status_val == STATUS["SOLVED"]
        _check(o, bt)
        assert bt.sparse_info(0)[0] > 0
        bt.close()
        o.cleanup()


@pytest.mark.parametrize("name", ["basic_qp", "medium_qp", "degen_hess", "ls_qp"])
def test_reference_solutions_with_the_sparse_kkt_factor(ctx, golden, name):
    e = golden["expect"][name]
    p = fixture_qp(golden["problems"][name])
    with sparse_kkt(ctx):
        o, bt = _pair(ctx, p, gsettings(ctx, golden, name))
        o.solve(); bt.solve()
        assert int(bt.info(0).status_val) == STATUS["SOLVED"]
        x = bt.solution()[0][0]
        if "rel_tol" in e:
            for a, b in zip(x, e["solution"]):
                assert abs(a - b) <= abs(e["rel_tol"] * b)
        else:
            assert np.max(np.abs(x - e["solution"])) <= e["abs_tol"]
        _check(o, bt)


def _K(bt, p, n, m):
    """K of the factor's current state in numpy ([x; y] numbering): state 1 = row present, else a unit row"""
    nzA, nzQ = int(p.Ap[-1]), int(p.Qp[-1])
    A = sp.csc_matrix((bt.named_vec("A_values", nzA), p.Ai, p.Ap), shape=(m, n)).toarray()
    Ql = sp.csc_matrix((bt.named_vec("Q_values", nzQ), p.Qi, p.Qp), shape=(n, n)).toarray()
    K = np.eye(n + m)
    K[:n, :n] = np.tril(Ql) + np.tril(Ql, -1).T + np.eye(n) / bt.stats(0).gamma
    sig_inv = bt.vec("sigma_inv")
    state = bt.ivec("kkt_state")
    for k in np.where(state == 1)[0]:
        K[n + k, :n] = A[k]
        K[:n, n + k] = A[k]
        K[n + k, n + k] = -sig_inv[k] if np.any(A[k]) else 1.0
    return K, state


def test_row_add_and_delete_through_the_boundary_operations(ctx):
    """qpg_kkt_form / _factorize, then a scripted sequence of row additions and deletions (a constraint ordered before all its variables, one
    ordered before some of them -- the k32 != 0 case --, the dense budget row, a deleted row added again): after every step qpg_kkt_solve
    solves K sol = [-dphi; 0] to 1e-11 and agrees with a fresh factorisation of the same K to 1e-11"""
    p = sparse_qp(sizes(ctx, 40, 160), "banded+budget", seed=5)
    n, m = p.n, p.m
    st = dict(ST, max_iter=4)
    with sparse_kkt(ctx, -1):
        bt = QpalmBatch(ctx, [p], ctx.default_settings(**st))
        fresh = QpalmBatch(ctx, [p], ctx.default_settings(**st))
        bt.iterate(4); fresh.iterate(4)
        perm = bt.sparse_perm(0)[0]
        ip = np.empty_like(perm); ip[perm] = np.arange(n + m)
        act = (np.arange(m) % 3 == 0).astype(np.int64)
        budget = m - 1
        act[budget] = 0
        A = sp.csc_matrix((p.Ax, p.Ai, p.Ap), shape=(m, n)).tocsr()
        k32_zero, k32_nonzero = [], []          # inactive constraints ordered after all their variables / before one of them at least
        for k in np.where(act == 0)[0]:
            if k != budget:
                (k32_nonzero if np.any(ip[A.indices[A.indptr[k]:A.indptr[k + 1]]] > ip[n + k]) else k32_zero).append(int(k))
        assert k32_zero and k32_nonzero
        c0, c1 = k32_zero[0], k32_nonzero[0]
        leave1 = int(np.where(act == 1)[0][1])
        script = [("enter", [c0, c1, budget]), ("leave", [budget, leave1]), ("enter", [budget]), ("leave", [c1])]
        rhs = np.random.default_rng(3).standard_normal(n)
        bt.set_ivec("active", act)
        bt.op("kkt_form")
        bt.op("kkt_factorize")
        for step, (what, lst) in enumerate(script):
            bt.set_ivec(what, lst)
            bt.set_scalar("nb_" + what, len(lst))
            bt.op("kkt_update_entering_constraints" if what == "enter" else "kkt_update_leaving_constraints")
            bt.set_vec("dphi", rhs)
            bt.op("kkt_solve")
            sol = bt.named_vec("sol_kkt", n + m)
            K, state = _K(bt, p, n, m)
            b = np.concatenate([-rhs, np.zeros(m)])
            res = np.max(np.abs(K @ sol - b)) / max(np.max(np.abs(K)) * np.max(np.abs(sol)), np.max(np.abs(b)))
            assert res <= 1e-11, (step, res)
            fresh.set_ivec("active", (state == 1).astype(np.int64))
            fresh.op("kkt_form")
            fresh.op("kkt_factorize")
            fresh.set_vec("dphi", rhs)
            fresh.op("kkt_solve")
            ref = fresh.named_vec("sol_kkt", n + m)
            assert np.max(np.abs(sol - ref)) <= 1e-11 * max(1.0, np.max(np.abs(ref))), (step, np.max(np.abs(sol - ref)))
        assert set(np.where(state == 1)[0]) == (set(np.where(act == 1)[0]) | {c0, budget}) - {leave1}
        assert set(np.where(state == 2)[0]) == {leave1, c1}
        bt.close(); fresh.close()


def _check_member(o, bt, k, counts=True):
    """test_kkt_path._check for member k of a batch of mixed sizes (the batch's vectors are padded to its largest member); counts = False after a
    warm-started step (the oracle's counters run on over its solves; test_mpc_scale compares the same fields).  y to 1e-8 as test_mpc_scale's KKT
    mode: the multipliers of the quasi-definite systems (-1/sigma on the diagonal, dense rows) lose a digit (measured 2.8e-9 on one member, x 2e-14)"""
    n, m = bt.dims[k]
    info, s = bt.info(k), bt.stats(k)
    assert o.counter("kkt_mode") == 1
    assert int(info.status_val) == o.status_val
    assert int(info.iter) == int(o.info.iter) and int(info.iter_out) == int(o.info.iter_out)
    if counts:
        assert int(s.n_refactor) == o.counter("n_refactor")
        assert int(s.n_rank1) == o.counter("n_row_add") + o.counter("n_row_del")
    x, y = bt.solution()
    assert rel(x[k][:n], o.x) <= RTOL and rel(y[k][:m], o.y) <= 1e-8, (k, rel(x[k][:n], o.x), rel(y[k][:m], o.y))
    assert np.array_equal(bt.ivec("active", k)[:m], o.ivec("active"))


def test_batches_of_mixed_members_and_warm_started_sequences(ctx):
    """members of different patterns and sizes, more members than resident slots, then two warm-started steps with moved bounds and a
    moved linear term: every member against its own oracle run"""
    nb = sizes(ctx, 48, 160)
    probs = [sparse_qp(nb, "banded+budget", seed=1), sparse_qp(nb - 8, "blocks", seed=2), random_qp(nb // 2, nb, seed=3, density_A=0.08, density_M=0.05),
             sparse_qp(nb - 16, "arrow", seed=4), sparse_qp(nb, "blocks+budget", seed=5, dense_rows=2)]
    ctx.set_option("max_slots", 2)
    try:
        with sparse_kkt(ctx):
            bt = QpalmBatch(ctx, probs, ctx.default_settings(**ST))
            assert bt.B > 2
            oracles = [ob.OracleQP(*p.args(), c=p.c, settings=ob.default_settings(**ST)) for p in probs]
            bt.solve()
            for o in oracles:
                o.solve()
            for k, o in enumerate(oracles):
                _check_member(o, bt, k)
            rng = np.random.default_rng(8)
            for step in range(2):
                xs, ys = bt.solution()
                bmin = np.zeros((bt.B, bt.m)); bmax = np.zeros((bt.B, bt.m)); q = np.zeros((bt.B, bt.n))
                for k, p in enumerate(probs):
                    shift = 0.05 * rng.standard_normal(p.m)
                    bmin[k, :p.m] = p.bmin + shift; bmax[k, :p.m] = p.bmax + shift
                    q[k, :p.n] = p.q + 0.1 * rng.standard_normal(p.n)
                assert bt.update_bounds(bmin, bmax) == 0
                bt.update_q(q)
                bt.warm_start(xs, ys)
                bt.solve()
                for k, (p, o) in enumerate(zip(probs, oracles)):
                    o.update_bounds(bmin[k, :p.m], bmax[k, :p.m])
                    o.update_q(q[k, :p.n])
                    o.warm_start(xs[k, :p.n], ys[k, :p.m])
                    o.solve()
                    assert o.status_val == STATUS["SOLVED"]
                    _check_member(o, bt, k, counts=False)
            bt.close()
            for o in oracles:
                o.cleanup()
    finally:
        ctx.set_option("max_slots", 512)


def test_sparse_kkt_refusals(ctx):
    """dual termination (no LD_Q on the pattern of K) and nonconvex are refused with the sparse KKT factor; without the option the dense
    KKT path is what it was"""
    p = sparse_qp(40, "banded+budget", seed=1)
    with sparse_kkt(ctx):
        for kw in (dict(enable_dual_termination=1), dict(nonconvex=1)):
            with pytest.raises(QpgError) as e:
                QpalmBatch(ctx, [p], ctx.default_settings(**dict(ST, **kw)))
            assert e.value.code == UNSUPPORTED
        bt = QpalmBatch(ctx, [p], ctx.default_settings(**ST))
        assert bt.update_settings(ctx.default_settings(**dict(ST, enable_dual_termination=1))) == UNSUPPORTED
        bt.close()
    with sparse_kkt(ctx, on=0):
        o, bt = _pair(ctx, p, ST)
        with pytest.raises(QpgError):
            bt.sparse_info(0)                     # the dense panel
        o.solve(); bt.solve()
        _check(o, bt)


def test_fuzz_with_the_sparse_kkt_factor(ctx):
    """the general fuzz stream with factorization_method = FACTORIZE_KKT forced (dual termination off: refused), judged as the other campaigns"""
    plan = [(61, 20, 2, 40, -1), (62, 20, 2, 40, 0)] if ctx.kind == "emu" else [(61, 150, 2, 70, -1), (62, 150, 2, 70, 0)]
    force = dict(factorization_method=0, enable_dual_termination=0)
    bad, buckets, total = [], {}, 0
    for seed, count, n_lo, n_hi, ordering in plan:
        with sparse_kkt(ctx, ordering):
            for it, p, st, warm, meta in cases(seed, count, n_lo, n_hi, force):
                r = run_case(ctx, p, st, warm)
                ok, why, cls = judge_case(r, p, st, warm, 1e-8, ctx)
                if not ok:
                    bad.append((seed, it, meta, why))
                key = "exact" if ok and not cls else (cls if isinstance(cls, str) else "rounding") if ok else "failed"
                buckets[key] = buckets.get(key, 0) + 1
                total += 1
    print("sparse KKT fuzz: %d cases, buckets %s" % (total, buckets))
    assert not bad, bad


def _kkt_conditions(p, x, y, tol):
    """max violations of primal feasibility, stationarity and complementarity of (x, y) on the unscaled problem (scipy)"""
    Qf = sp.csc_matrix((p.Qx, p.Qi, p.Qp), shape=(p.n, p.n))
    Qf = Qf + sp.tril(Qf, -1).T
    A = sp.csc_matrix((p.Ax, p.Ai, p.Ap), shape=(p.m, p.n))
    Ax = A @ x
    prim = np.max(np.maximum(0.0, np.maximum(p.bmin - Ax, Ax - p.bmax)))
    dual = np.max(np.abs(Qf @ x + p.q + A.T @ y))
    scale = 1.0 + max(np.max(np.abs(Qf @ x)), np.max(np.abs(p.q)), np.max(np.abs(A.T @ y)))
    comp = 0.0
    up, lo = y > tol, y < -tol
    if np.any(up):
        comp = max(comp, np.max(np.abs(Ax[up] - p.bmax[up])))
    if np.any(lo):
        comp = max(comp, np.max(np.abs(Ax[lo] - p.bmin[lo])))
    return prim, dual / scale, comp


@HIP_ONLY
@pytest.mark.parametrize("kind,n", [("banded+budget", 20000), ("blocks+budget", 100000), ("banded", 20000)])
def test_at_size(ctx, kind, n):
    """sizes the dense KKT panel refuses and, with a dense row, the sparse Schur factor too: solved, KKT conditions, nnz(L) per row"""
    p = sparse_qp(n, kind, seed=21)
    nf = p.n + p.m
    with sparse_kkt(ctx):
        t0 = time.perf_counter()
        bt = QpalmBatch(ctx, [p], ctx.default_settings(**ST))
        t1 = time.perf_counter()
        bt.solve()
        t2 = time.perf_counter()
        info, s = bt.info(0), bt.stats(0)
        nnz, dev = bt.sparse_info(0)
        lev = bt.sparse_perm(0)[1]
        print("%s n = %d, n + m = %d: setup %.2f s, solve %.2f s, iter %d, levels %d, nnz(L) = %d (%.2f per row), device block %.1f MB, "
              "refactorisations %d (%.2f ms per step), row operations %d (update steps: %.3f ms per row; both with the step's solve + refinement)"
              % (kind, p.n, nf, t1 - t0, t2 - t1, int(info.iter), lev, nnz, nnz / nf, dev / 2 ** 20, int(s.n_refactor),
                 s.ms_factor / max(1, int(s.n_refactor)), int(s.n_rank1), s.ms_update / max(1, int(s.n_rank1))))
        assert int(info.status_val) == STATUS["SOLVED"]
        x, y = bt.solution()
        prim, dual, comp = _kkt_conditions(p, x[0], y[0], 1e-6)
        assert prim <= 1e-4 and dual <= 1e-4 and comp <= 1e-4, (prim, dual, comp)
        assert nnz <= 12 * nf                     # measured: 10.0, 6.1 and 9.1 entries per row
        assert dev <= 64 * 8 * nf + (64 << 20)     # the device block grows with nnz(L) and n + m, not (n + m)^2
        bt.close()
    ctx.set_option("sparse_factor", 1)
    try:
        st = dict(ST, factorization_method=1)
        if kind == "banded":                       # the same problem through the sparse Schur factor
            bs = QpalmBatch(ctx, [p], ctx.default_settings(**st))
            bs.solve()
            assert int(bs.info(0).status_val) == STATUS["SOLVED"]
            xs = bs.solution()[0][0]
            assert np.max(np.abs(x[0] - xs)) <= 1e-5 * max(1.0, np.max(np.abs(xs)))
            bs.close()
        elif kind == "blocks+budget":              # the motivation: one dense row makes Q + A'A dense, beyond the sparse Schur factor's cap
            with pytest.raises(QpgError) as e:
                QpalmBatch(ctx, [p], ctx.default_settings(**st))
            assert e.value.code == UNSUPPORTED
    finally:
        ctx.set_option("sparse_factor", -1)

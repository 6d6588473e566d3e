"""qpalm_update_Q_A for a set-up batch (qpg_batch_update_Q_A / _device): new values of Q and A on the same sparsity patterns, without a new setup.

Yardstick: the same backend's own fresh setup.  Run A is  create(P0) -> setup -> solve -> update_Q_A(values of P1) -> warm start -> solve;  run B is
create(P1 with the current q and bounds) -> setup -> the same warm start -> solve.  The two must agree BIT FOR BIT (np.array_equal) in x, y, status,
iteration counts, the work counters of QPGStats, gamma, the scaling vectors D, E and the scaling constant c: the update leaves what a fresh setup
leaves, and the solve after it is the same kernel on the same bits.  P1 has P0's pattern with every value redrawn (Q kept diagonally dominant in the
convex cases).  That both runs are right, not merely equal, is checked against the CPU oracle on the dense Schur path (1e-9 relative, exact counts).

Sizes: n = 45 on the emulator (128-thread workgroups) and n = 150, m = 300 on the GPU: nnz(A) and nnz(Q, both triangles) exceed one workgroup's
threads, so the strided loops of the update kernel wrap."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import binding as ob
from qpalm_amd import capi
from qpalm_amd.capi import f64, fptr, i64, iptr
from qpalm_amd.problems import QP, random_qp, sparse_qp
from qpalm_amd.solver import Qpalm, QpalmBatch
from tests.helpers import STATUS
from tests.test_nonconvex import indefinite_qp
from tests.test_parity import RTOL, rel, sizes

ST = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
INVALID = -2
HIP_ONLY = pytest.mark.parametrize("ctx", [pytest.param("hip", marks=pytest.mark.gpu, id="hip")], indirect=True)


def redraw(p, seed, convex=True):
    """p's patterns with every value of Q and A drawn again (Q diagonally dominant with a positive diagonal when convex; else its values perturbed by
    up to 30 %, which moves the negative eigenvalue)"""
    rng = np.random.default_rng(seed)
    Ax = rng.standard_normal(len(p.Ax))
    Qx = np.array(p.Qx, float).copy()
    if not convex:
        return dataclasses.replace(p, Qx=Qx * (1.0 + 0.3 * rng.random(len(Qx))), Ax=Ax)
    col = np.repeat(np.arange(p.n), np.diff(p.Qp))
    offd = np.asarray(p.Qi) != col
    Qx[offd] = 0.3 * rng.standard_normal(int(offd.sum()))
    rowsum = np.zeros(p.n)
    np.add.at(rowsum, np.asarray(p.Qi)[offd], np.abs(Qx[offd]))
    np.add.at(rowsum, col[offd], np.abs(Qx[offd]))
    Qx[~offd] = rowsum[np.asarray(p.Qi)[~offd]] + 1.0 + rng.random(int((~offd).sum()))
    return dataclasses.replace(p, Qx=Qx, Ax=Ax)


def dense_probs(ctx, count=2, seed=300):
    n, m = sizes(ctx, (45, 90), (150, 300))
    dA, dM = sizes(ctx, (0.15, 0.1), (0.04, 0.03))
    P0 = [random_qp(n, m, seed=seed + k, density_A=dA, density_M=dM) for k in range(count)]
    threads = sizes(ctx, 128, 512)
    assert all(len(p.Ax) > threads and 2 * len(p.Qx) - p.n > threads for p in P0)
    return P0, [redraw(p, seed + 50 + k) for k, p in enumerate(P0)]


def snapshot(bt):
    """everything the two runs are compared in"""
    x, y = bt.solution()
    out = dict(x=x.copy(), y=y.copy())
    infos, stats = bt.infos(), bt.stats_all()
    for k in ("status_val", "iter", "iter_out"):
        out[k] = np.array([int(getattr(i, k)) for i in infos])
    out["dual_objective"] = np.array([float(i.dual_objective) for i in infos])
    for k in ("n_refactor", "n_rank1", "n_solve", "n_sweeps", "lobpcg_iter", "nonconvex"):
        out[k] = np.array([int(getattr(s, k)) for s in stats])
    for k in ("gamma", "sc_c", "lobpcg_lambda"):
        out[k] = np.array([float(getattr(s, k)) for s in stats])
    out["D"] = np.array([bt.vec("D", b) for b in range(bt.B)])
    out["E"] = np.array([bt.vec("E", b) for b in range(bt.B)])
    return out


def assert_same(a, b, what=""):
    bad = []
    for k in a:
        same = np.array_equal(a[k], b[k])
        if a[k].size <= 8:
            print(what, k, a[k], b[k], "same" if same else "DIFFERENT")
        else:
            print(what, k, "max |difference|", float(np.max(np.abs(a[k] - b[k]))) if a[k].size else 0.0, "same" if same else "DIFFERENT")
        if not same:
            bad.append(k)
    assert not bad, (what, bad)


def warm(bt, how, x0, y0):
    if how == "last":
        bt.warm_start_last()
    elif how == "given":
        bt.warm_start(x0, y0)


def runs(ctx, P0, P1, st, how="last", update=None, fresh=None):
    """(run A's batch after the update and its solve, run B's batch after its solve, the warm start's x and y)"""
    A = QpalmBatch(ctx, P0, ctx.default_settings(**st))
    A.solve()
    x0, y0 = (v.copy() for v in A.solution())
    if how == "given":   # some point other than the stored solution
        x0, y0 = 0.5 * x0 + 0.01, 0.9 * y0
    (update or (lambda bt: bt.update_Q_A([p.Qx for p in P1], [p.Ax for p in P1])))(A)
    assert all(int(i.status_val) == STATUS["UNSOLVED"] and int(i.iter) == 0 for i in A.infos())
    assert all(int(s.n_refactor) == 0 and int(s.n_solve) == 0 for s in A.stats_all())      # the counters restart as after setup
    warm(A, how, x0, y0)
    A.solve()
    B = QpalmBatch(ctx, fresh or P1, ctx.default_settings(**st))
    warm(B, "given" if how == "last" else how, x0, y0)       # (the stored solution of run A, handed over)
    B.solve()
    return A, B, x0, y0


# ---- 1. dense Schur ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["last", "given", "none"])
@pytest.mark.parametrize("proximal", [1, 0])
@pytest.mark.parametrize("scaling", [10, 0])
def test_dense_schur(ctx, scaling, proximal, how):
    P0, P1 = dense_probs(ctx)
    st = dict(ST, scaling=scaling, proximal=proximal)
    A, B, x0, y0 = runs(ctx, P0, P1, st, how)
    assert_same(snapshot(A), snapshot(B), "dense Schur")
    xb, yb = B.solution()
    for k, p in enumerate(P1):     # ... and both are right: the oracle on P1 with the same warm start
        o = ob.OracleQP(*p.args(), c=p.c, settings=ob.default_settings(**st))
        if how != "none":
            o.warm_start(x0[k], y0[k])
        o.solve()
        info, s = B.info(k), B.stats(k)
        assert int(info.status_val) == o.status_val == STATUS["SOLVED"]
        assert int(info.iter) == int(o.info.iter) and int(info.iter_out) == int(o.info.iter_out)
        assert int(s.n_refactor) == o.counter("n_refactor") and int(s.n_rank1) == o.counter("n_rank1")
        assert rel(xb[k], o.x) <= RTOL and rel(yb[k], o.y) <= RTOL


# ---- 2. value maps ----------------------------------------------------------------------------------------------------------------------------
def scrambled(p, dup_seed=5):
    """the same QP the way a careless caller hands it over: columns of A in descending row order with one entry split into two (a duplicate), Q with
    both triangles (the upper entries are ignored, like stype = -1), columns descending too"""
    rng = np.random.default_rng(dup_seed)
    Ap, Ai, Ax = [0], [], []
    split = int(p.Ap[p.n // 2])          # first entry of a middle column
    assert p.Ap[p.n // 2 + 1] > split
    for j in range(p.n):
        ks = list(range(p.Ap[j], p.Ap[j + 1]))[::-1]
        for k in ks:
            if k == split:
                Ai += [p.Ai[k], p.Ai[k]]; Ax += [0.25 * p.Ax[k], 0.75 * p.Ax[k]]
            else:
                Ai.append(p.Ai[k]); Ax.append(p.Ax[k])
        Ap.append(len(Ai))
    Qf = p.Q_full().tocsc()
    Qf.sort_indices()
    Qp, Qi, Qx = [0], [], []
    for j in range(p.n):
        for k in range(Qf.indptr[j], Qf.indptr[j + 1])[::-1]:
            i = int(Qf.indices[k])
            Qi.append(i); Qx.append(float(Qf.data[k]) if i >= j else float(rng.standard_normal()))    # (what stands above the diagonal does not matter)
        Qp.append(len(Qi))
    return QP(p.n, p.m, i64(Qp), i64(Qi), f64(Qx), i64(Ap), i64(Ai), f64(Ax), p.q, p.bmin, p.bmax, p.c)


def test_value_maps(ctx):
    """entry k of the update's arrays is the k-th entry the CALLER gave: a member with unsorted columns, both triangles of Q and a duplicate in A next
    to a member with sorted input (which copies straight)"""
    P0, P1 = dense_probs(ctx, seed=320)
    S0, S1 = [scrambled(P0[0]), P0[1]], [scrambled(P1[0]), P1[1]]
    assert not np.array_equal(S0[0].Ai, np.sort(S0[0].Ai)) and len(S0[0].Ax) == len(P0[0].Ax) + 1 and len(S0[0].Qx) == 2 * len(P0[0].Qx) - P0[0].n
    A, B, _, _ = runs(ctx, S0, S1, ST)
    assert_same(snapshot(A), snapshot(B), "value maps")


# ---- 3. the other factor modes ------------------------------------------------------------------------------------------------------------------
def test_dense_kkt_panel(ctx):
    P0, P1 = dense_probs(ctx, seed=340)
    A, B, _, _ = runs(ctx, P0, P1, dict(ST, factorization_method=0))
    assert_same(snapshot(A), snapshot(B), "dense KKT")
    assert all(int(s.n_rank1) > 0 for s in A.stats_all())     # row additions / deletions happened after the update too


def sparse_runs(ctx, kind, st):
    p0 = sparse_qp(sizes(ctx, 104, 400), kind, seed=3)
    P0, P1 = [p0], [redraw(p0, 17)]
    assert len(p0.Ax) > sizes(ctx, 128, 512)
    kept = {}

    def update(bt):
        kept["perm"], kept["info"] = bt.sparse_perm(0), bt.sparse_info(0)
        bt.update_Q_A([p.Qx for p in P1], [p.Ax for p in P1])
        perm, info = bt.sparse_perm(0), bt.sparse_info(0)
        assert np.array_equal(perm[0], kept["perm"][0]) and perm[1] == kept["perm"][1] and info == kept["info"]    # the analysis was kept
    A, B, _, _ = runs(ctx, P0, P1, st, update=update)
    assert B.sparse_info(0) == kept["info"] and np.array_equal(B.sparse_perm(0)[0], kept["perm"][0])
    assert_same(snapshot(A), snapshot(B), "sparse " + kind)
    assert int(A.info(0).status_val) == STATUS["SOLVED"]


@pytest.mark.parametrize("ordering,kind", [(0, "banded"), (1, "banded"), (0, "blocks"), (1, "blocks")])
def test_sparse_factor(ctx, ordering, kind):
    ctx.set_option("sparse_factor", 1)
    ctx.set_option("sparse_ordering", ordering)
    try:
        sparse_runs(ctx, kind, ST)
    finally:
        ctx.set_option("sparse_factor", -1)
        ctx.set_option("sparse_ordering", -1)


def test_sparse_kkt_factor(ctx):
    ctx.set_option("sparse_kkt", 1)
    try:
        sparse_runs(ctx, "banded+budget", dict(ST, factorization_method=0))
    finally:
        ctx.set_option("sparse_kkt", 0)


# ---- 4. dual termination and nonconvex ----------------------------------------------------------------------------------------------------------
def test_dual_termination(ctx):
    P0, P1 = dense_probs(ctx, seed=360)
    A, B, _, _ = runs(ctx, P0, P1, dict(ST, enable_dual_termination=1))
    sa, sb = snapshot(A), snapshot(B)
    assert_same(sa, sb, "dual termination")
    assert np.all(sa["dual_objective"] != 0.0) and np.all(np.isfinite(sa["dual_objective"]))      # LD_Q was rebuilt from the new Q


def test_nonconvex(ctx):
    n, m = sizes(ctx, (30, 50), (150, 300))
    p0 = indefinite_qp(n, m, 7)[0]
    P0, P1 = [p0], [redraw(p0, 8, convex=False)]
    A, B, _, _ = runs(ctx, P0, P1, dict(ST, nonconvex=1))
    sa, sb = snapshot(A), snapshot(B)
    assert_same(sa, sb, "nonconvex")
    first = QpalmBatch(ctx, P0, ctx.default_settings(**dict(ST, nonconvex=1))).stats(0)
    assert sa["nonconvex"][0] == 1 and sa["lobpcg_lambda"][0] < 0 and sa["lobpcg_lambda"][0] != float(first.lobpcg_lambda)    # another eigenvalue than P0's
    assert sa["gamma"][0] <= 1.0 / abs(sa["lobpcg_lambda"][0])


# ---- 5. after update_q and update_bounds ----------------------------------------------------------------------------------------------------------
def test_after_update_q_and_bounds(ctx):
    P0, P1 = dense_probs(ctx, seed=380)
    rng = np.random.default_rng(1)
    B_, n, m = len(P0), P0[0].n, P0[0].m
    q2 = rng.standard_normal((B_, n))
    lo1, hi1 = -1.0 - rng.random((B_, m)), 1.0 + rng.random((B_, m))
    lo2, hi2 = -0.5 - rng.random((B_, m)), 0.5 + rng.random((B_, m))
    lo2[1, 3], hi2[1, 3] = 2.0, 1.0      # member 1's second bounds are refused: it keeps the first ones

    def update(bt):
        bt.update_q(q2)
        assert bt.update_bounds(lo1, hi1) == 0
        assert bt.update_bounds(lo2, hi2) == INVALID
        assert [int(i.status_val) for i in bt.infos()] == [STATUS["SOLVED"], STATUS["ERROR"]]
        bt.update_Q_A([p.Qx for p in P1], [p.Ax for p in P1])
    fresh = [dataclasses.replace(P1[0], q=q2[0], bmin=lo2[0], bmax=hi2[0]), dataclasses.replace(P1[1], q=q2[1], bmin=lo1[1], bmax=hi1[1])]
    A, B, _, _ = runs(ctx, P0, P1, ST, update=update, fresh=fresh)
    assert_same(snapshot(A), snapshot(B), "after update_q / update_bounds")
    # a second setup of the same batch still returns to the problem as it was set
    assert A.L.qpg_batch_setup(A.h) == 0
    A.solve()
    F = QpalmBatch(ctx, P0, ctx.default_settings(**ST))
    F.solve()
    assert_same(snapshot(A), snapshot(F), "second setup")
    # ... and an update after it starts from the slab's q and bounds again
    A.update_Q_A([p.Qx for p in P1], [p.Ax for p in P1])
    A.solve()
    G = QpalmBatch(ctx, P1, ctx.default_settings(**ST))
    G.solve()
    assert_same(snapshot(A), snapshot(G), "update after the second setup")


# ---- 6. queue and mixed sizes ---------------------------------------------------------------------------------------------------------------------
def mixed_batch_steps(ctx, queue):
    """five members of two sizes, three updates in a row (P1, P2, P3) with a solve after each, every solve against its own fresh setup.  Where every
    member is resident the second update interrupts an unfinished solve (qpg_batch_iterate needs B <= the resident slots)."""
    (n1, m1), (n2, m2) = sizes(ctx, ((32, 48), (21, 30)), ((150, 300), (97, 201)))
    P0 = [random_qp(n1 if k % 2 == 0 else n2, m1 if k % 2 == 0 else m2, seed=400 + k, density_A=sizes(ctx, 0.15, 0.04), density_M=sizes(ctx, 0.1, 0.03)) for k in range(5)]
    A = QpalmBatch(ctx, P0, ctx.default_settings(**ST))
    print("launch shape (workgroups, threads, LDS bytes):", A.launch_shape())
    assert (A.launch_shape()[0] < 5) == queue
    A.solve()
    for step in (1, 2, 3):
        P = [redraw(p, 1000 * step + k) for k, p in enumerate(P0)]
        x0, y0 = (v.copy() for v in A.solution())
        if step == 2 and not queue:
            A.warm_start(0.3 * x0, 0.3 * y0)
            A.begin_solve()
            A.iterate(3)
            assert A.num_unfinished() > 0      # the update ends a solve that was under way
            x0, y0 = (v.copy() for v in A.solution())
        A.update_Q_A([p.Qx for p in P], [p.Ax for p in P])
        A.warm_start_last()
        A.solve()
        B = QpalmBatch(ctx, P, ctx.default_settings(**ST))
        B.warm_start(x0, y0)
        B.solve()
        assert_same(snapshot(A), snapshot(B), "step %d" % step)
        assert all(s == STATUS["SOLVED"] for s in A.statuses())
        B.close()
    return A


@pytest.mark.parametrize("max_slots", [2, 512])
def test_queue_and_mixed_sizes(ctx, max_slots):
    """max_slots = 2: the members go through the work queue.  (The GPU library would run five factors of at most 192 rows on its 128-thread instance,
    seven workgroups per pair of slots = no queue: small_workgroups = 3 keeps the 256-thread instance, two workgroups per slot = four for five
    members; the emulator has one instance, two workgroups.)  max_slots = 512: every member is resident."""
    ctx.set_option("max_slots", max_slots)
    if max_slots == 2:
        ctx.set_option("small_workgroups", 3)
    try:
        mixed_batch_steps(ctx, queue=(max_slots == 2))
    finally:
        ctx.set_option("max_slots", 512)
        ctx.set_option("small_workgroups", 1)


@HIP_ONLY
def test_mixed_sizes_on_the_128_thread_instance(ctx):
    """the same steps on the third instance of the kernels (128-thread workgroups, forced: it takes large batches of small factors by itself)"""
    ctx.set_option("small_workgroups", 2)
    try:
        A = mixed_batch_steps(ctx, queue=False)
        assert A.launch_shape()[1] == 128
    finally:
        ctx.set_option("small_workgroups", 1)


# ---- 7. device entry -------------------------------------------------------------------------------------------------------------------------------
def test_device_entry(ctx):
    """the values already in device memory (a torch tensor on the GPU; under emulation device memory is host memory): bit-identical to the host entry"""
    P0, P1 = dense_probs(ctx, seed=420)
    S0, S1 = [scrambled(P0[0]), P0[1]], [scrambled(P1[0]), P1[1]]       # one member through its value maps
    H, D = (QpalmBatch(ctx, S0, ctx.default_settings(**ST)) for _ in range(2))
    H.solve(); D.solve()
    Qx, Ax = D._padded([p.Qx for p in S1], D.nnzQ), D._padded([p.Ax for p in S1], D.nnzA)
    H.update_Q_A(Qx, Ax)
    if ctx.kind == "hip":
        import torch
        tq, ta = torch.from_numpy(Qx).to("cuda:0"), torch.from_numpy(Ax).to("cuda:0")
        torch.cuda.synchronize()
        D.update_Q_A_device(tq.data_ptr(), ta.data_ptr())
        assert np.array_equal(tq.cpu().numpy(), Qx) and np.array_equal(ta.cpu().numpy(), Ax)      # the caller's arrays are read, not written
    else:
        D.update_Q_A_device(Qx.ctypes.data, Ax.ctypes.data)
    for bt in (H, D):
        bt.warm_start_last()
        bt.solve()
    sh, sd = snapshot(H), snapshot(D)
    assert_same(sh, sd, "device entry")
    assert all(s == STATUS["SOLVED"] for s in sh["status_val"])
    first = QpalmBatch(ctx, S0, ctx.default_settings(**ST))
    first.solve()
    F = QpalmBatch(ctx, S1, ctx.default_settings(**ST))
    F.warm_start(*first.solution())
    F.solve()
    assert_same(sd, snapshot(F), "device entry against a fresh setup")


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    P0, P1 = dense_probs(ctx, count=1, seed=440)
    p, L = P0[0], ctx.L
    st = ctx.default_settings(**ST)
    h = C.c_void_p()
    assert L.qpg_batch_create(ctx.h, 1, p.n, p.m, len(p.Ax), len(p.Qx), C.byref(st), C.byref(h)) == 0
    arrs = (i64(p.Qp), i64(p.Qi), f64(p.Qx), i64(p.Ap), i64(p.Ai), f64(p.Ax), f64(p.q), f64(p.bmin), f64(p.bmax))
    assert L.qpg_batch_set_problem(h, 0, iptr(arrs[0]), iptr(arrs[1]), fptr(arrs[2]), iptr(arrs[3]), iptr(arrs[4]), fptr(arrs[5]), fptr(arrs[6]), 0.0,
                                   fptr(arrs[7]), fptr(arrs[8])) == 0
    Qx, Ax = f64(P1[0].Qx), f64(P1[0].Ax)
    assert L.qpg_batch_update_Q_A(h, fptr(Qx), fptr(Ax)) == INVALID                      # not set up
    assert L.qpg_batch_update_Q_A_device(h, Qx.ctypes.data, Ax.ctypes.data) == INVALID
    assert b"not set up" in L.qpg_last_error()
    assert L.qpg_batch_setup(h) == 0
    assert L.qpg_batch_update_Q_A(h, None, fptr(Ax)) == INVALID
    assert L.qpg_batch_update_Q_A(h, fptr(Qx), None) == INVALID
    assert L.qpg_batch_update_Q_A_device(h, None, Ax.ctypes.data) == INVALID
    assert L.qpg_batch_update_Q_A_device(h, Qx.ctypes.data, None) == INVALID
    assert L.qpg_batch_update_Q_A(None, fptr(Qx), fptr(Ax)) == INVALID
    assert L.qpg_batch_solve(h) == 0                                                     # ... and the batch still solves P0
    info = capi.Info()
    x, y = np.zeros(p.n), np.zeros(p.m)
    assert L.qpg_batch_get_info(h, 0, C.byref(info)) == 0 and L.qpg_batch_get_solution(h, fptr(x), fptr(y)) == 0
    o = ob.OracleQP(*p.args(), c=p.c, settings=ob.default_settings(**ST))
    o.solve()
    assert int(info.status_val) == o.status_val == STATUS["SOLVED"] and int(info.iter) == int(o.info.iter)
    assert rel(x, o.x) <= RTOL and rel(y, o.y) <= RTOL
    L.qpg_batch_destroy(h)


def test_shapes_are_checked(ctx):
    P0, P1 = dense_probs(ctx, count=2, seed=460)
    bt = QpalmBatch(ctx, P0, ctx.default_settings(**ST))
    with pytest.raises(ValueError):
        bt.update_Q_A([P1[0].Qx], [P1[0].Ax])                          # one member's values for a batch of two
    with pytest.raises(ValueError):
        bt.update_Q_A(np.zeros((2, bt.nnzQ + 1)), np.zeros((2, bt.nnzA)))
    with pytest.raises(ValueError):
        bt.update_Q_A([np.zeros(bt.nnzQ + 1)] * 2, [p.Ax for p in P1])


def test_single_qp_facade(ctx):
    """Qpalm.update_Q_A: the one-QP form"""
    P0, P1 = dense_probs(ctx, count=1, seed=480)
    q = Qpalm(ctx)
    q.settings = ctx.default_settings(**ST)
    q.set_problem(P0[0])
    q.setup().solve()
    q.update_Q_A(P1[0].Qx, P1[0].Ax)
    assert q.status_val == STATUS["UNSOLVED"]
    q.solve()
    F = QpalmBatch(ctx, P1, ctx.default_settings(**ST))
    F.solve()
    assert_same(snapshot(q.batch), snapshot(F), "single QP")


# ---- 9. coop mode ------------------------------------------------------------------------------------------------------------------------------------
@HIP_ONLY
def test_coop_mode(ctx):
    """one QP whose linear algebra runs on many workgroups: the recorded launch chains survive the update (they hold sizes and addresses, no values)"""
    n, m = 600, 900
    p0 = random_qp(n, m, seed=500, density_A=0.01, density_M=0.005)
    P0, P1 = [p0], [redraw(p0, 501)]
    ctx.set_option("coop", 1)
    ctx.set_option("coop_rank_threshold", -1)
    try:
        A, B, _, _ = runs(ctx, P0, P1, ST)
    finally:
        ctx.set_option("coop", 0)
        ctx.set_option("coop_rank_threshold", -2)
    assert_same(snapshot(A), snapshot(B), "coop")
    assert int(A.info(0).status_val) == STATUS["SOLVED"] and int(A.stats(0).n_rank1) > 0

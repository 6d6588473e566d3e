"""Sparse coop mode (context option "sparse_coop" = 1): the sparse L D L' of ONE QP factorised and solved on many workgroups -- what the reference hands
to CHOLMOD's factorize and solve (src/solver_interface.c:319-370, 505-519).  The levels of the elimination tree become a chain of launches
(qpalm_host_symbolic.h: sparse_coop_plan; kernels k_co_sp_factor / k_co_sp_solve): a level wider than one workgroup's round runs on a grid, a run of narrower
levels on one workgroup.  No column's arithmetic depends on the workgroup that computes it, so the yardstick is exact: the same build with
"sparse_coop" = 0 -- x, y, objective and dual objective BIT FOR BIT, status, iteration counts and the factorisation / update / solve counters equal --
and, beside it, the oracle in its sparse-storage mode as tests/test_sparse_factor.py sets it up (x, y to RTOL).

Shapes: the smallest at which these kernels can go wrong.  "sparse_gpw" = 1 makes a workgroup's round 8 columns (2 in the emulator's 128-thread
workgroups), so that even the small QPs have levels wider than one workgroup; "coop_workgroups" = 8.  Every test sets its options and restores them."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp

from qpalm_amd.capi import QpgError
from qpalm_amd.problems import random_qp, sparse_qp
from qpalm_amd.solver import QpalmBatch
from tests.test_parity import RTOL, rel, sizes
from tests.test_sparse_factor import ST, oracle_sparse

DEFAULTS = dict(sparse_factor=-1, sparse_ordering=-1, sparse_gpw=0, sparse_lds=1, sparse_coop=0, sparse_kkt=0, coop_max_batch=4)
G = 8
UNSUPPORTED = -5


@contextlib.contextmanager
def options(ctx, **kw):
    """sparse_factor = 1, 8 coop workgroups and the given options; everything back to its default afterwards"""
    try:
        ctx.set_option("sparse_factor", 1)
        ctx.set_option("coop_workgroups", G)
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


def snapshot(bt):
    """everything the two modes must agree on, per member"""
    x, y = bt.solution()
    out = []
    for k in range(bt.B):
        i, s = bt.info(k), bt.stats(k)
        out.append(dict(x=x[k].copy(), y=y[k].copy(), objective=float(i.objective), dual_objective=float(i.dual_objective),
                        ints=(int(i.status_val), int(i.iter), int(i.iter_out), int(s.n_refactor), int(s.n_rank1), int(s.n_solve), int(s.n_factor_Q))))
    return out


def assert_same(a, b, what=""):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert u["ints"] == v["ints"], (what, k, u["ints"], v["ints"])      # status, iter, iter_out, n_refactor, n_rank1, n_solve, n_factor_Q
        assert np.array_equal(u["x"], v["x"]) and np.array_equal(u["y"], v["y"]), (what, k, float(np.max(np.abs(u["x"] - v["x"]))))
        assert u["objective"] == v["objective"] and u["dual_objective"] == v["dual_objective"], (what, k)


def both_modes(ctx, probs, st=ST, steps=None):
    """the same batch, and the same sequence of steps on it, with "sparse_coop" = 0 and 1: ({mode: [snapshot after every solve]}, the plans of mode 1,
    the orderings)"""
    res, plans, perms = {}, None, None
    for mode in (0, 1):
        ctx.set_option("sparse_coop", mode)
        bt = QpalmBatch(ctx, probs, ctx.default_settings(**st))
        assert bt.sparse_info(0)[0] > 0                        # the batch really keeps the sparse factor
        plan = [bt.sparse_coop_info(k) for k in range(bt.B)]
        if mode == 0:
            assert all(p == (0, 0, 0) for p in plan)
        else:
            plans, perms = plan, [bt.sparse_perm(k) for k in range(bt.B)]
        bt.solve()
        res[mode] = [snapshot(bt)]
        for step in (steps or []):
            step(bt)
            bt.solve()
            res[mode].append(snapshot(bt))
        bt.close()
    for k, (a, b) in enumerate(zip(res[1], res[0])):
        assert_same(a, b, "solve %d" % k)
    return res, plans, perms


def level_widths(p, perm):
    """columns per level of the elimination tree of P (Q + A'A) P' (symbolic elimination on a dense pattern: the test shapes are small)"""
    n = p.n
    A = sp.csc_matrix((np.ones(len(p.Ax)), p.Ai, p.Ap), shape=(p.m, n))
    Q = sp.csc_matrix((np.ones(len(p.Qx)), p.Qi, p.Qp), shape=(n, n))
    M = ((Q + Q.T + A.T @ A).toarray() != 0)[np.ix_(perm, perm)]
    level = np.zeros(n, dtype=np.int64)
    for j in range(n):
        rows = j + 1 + np.flatnonzero(M[j + 1:, j])
        if len(rows):
            M[np.ix_(rows, rows)] = True
            level[rows[0]] = max(level[rows[0]], level[j] + 1)
    return np.bincount(level)


def rounds(ctx):
    """(columns of a factorisation round at sparse_gpw = 1, rows of a solve round) of this backend's 512-thread instance"""
    t = 128 if ctx.kind == "emu" else 512
    return t // 64, t


def check_plan(ctx, p, perm, plan, gpw=1):
    """the plan against the level widths: narrow runs share a launch, a wide level gets min(G, ceil(width / round)) workgroups"""
    w = level_widths(p, perm)
    rf, rs = rounds(ctx)
    rf *= gpw
    f, s, g = plan

    def launches(round_):
        out, grids, prev_narrow = 0, [1], False
        for x in w:
            if x > round_:
                out += 1; prev_narrow = False; grids.append(min(G, -(-int(x) // round_)))
            else:
                out += 0 if prev_narrow else 1; prev_narrow = True
        return out, max(grids)
    nf, gf = launches(rf)
    ns, gs = launches(rs)
    assert f == nf and s == 2 + 2 * ns + (1 if w[0] > rs else 0), (plan, list(w))
    assert g == max(gf, gs, min(G, -(-p.n // rs))), (plan, list(w))
    if w.max() > rf:
        assert g >= 2
    return w


# ---- 1. kinds x orderings -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", [0, 1])
@pytest.mark.parametrize("kind", ["blocks", "banded", "arrow", "random"])
def test_kinds_and_orderings(ctx, kind, ordering):
    n = sizes(ctx, 72, 400)
    p = random_qp(n, n, seed=9, density_A=1.5 / n, density_M=1.0 / n) if kind == "random" else sparse_qp(n, kind, seed=11)
    with options(ctx, sparse_ordering=ordering, sparse_gpw=1):
        res, plans, perms = both_modes(ctx, [p])
    perm, levels = perms[0]
    w = check_plan(ctx, p, perm, plans[0])
    assert len(w) == levels
    if kind == "banded" and ordering == 0:
        assert levels == p.n and plans[0][0] == 1          # n one-column levels: ONE launch, not n
    if kind == "blocks":
        assert w.max() > rounds(ctx)[0] and plans[0][2] >= 2
    o = oracle_sparse(p, perm, **ST)
    r = res[1][0][0]
    assert r["ints"][0] == o.status_val == 1 and r["ints"][1] == int(o.info.iter)
    assert rel(r["x"], o.x) <= RTOL and rel(r["y"], o.y) <= RTOL


# ---- 2. grid-strided and ragged levels ------------------------------------------------------------------------------------------------------------
def _ragged_cases():
    # emu (rounds of 2 columns / 128 rows): 19 columns per level > 8 workgroups x 2, odd; 151 rows per level > 128 (blocks of two)
    # hip (rounds of 8 or 64 columns / 512 rows): 77 columns per level > 8 x 8, no multiple of 8; n = 4000 at the default sparse_gpw;
    #      1025 columns per level: 17 rounds of 64 on 8 workgroups, three workgroups' worth of solve rows, both ragged
    emu = [(152, 8, 1), (302, 2, 1)]
    hip = [(616, 8, 1), (4000, 8, 0), (8200, 8, 0)]
    return [pytest.param("emu", c, id="emu-%d-%d" % c[:2]) for c in emu] + [pytest.param("hip", c, marks=pytest.mark.gpu, id="hip-%d-%d" % c[:2]) for c in hip]


@pytest.mark.parametrize("ctx,case", _ragged_cases(), indirect=["ctx"])
def test_grid_strided_and_ragged_levels(ctx, case):
    n, block, gpw = case
    p = sparse_qp(n, "blocks", seed=13, block=block, rows_per_block=4 if block == 8 else 1)
    with options(ctx, sparse_ordering=0, sparse_gpw=gpw):
        res, plans, perms = both_modes(ctx, [p])
    rf, rs = rounds(ctx)
    rf *= gpw if gpw else 8
    width = p.n // block
    f, s, g = plans[0]
    assert perms[0][1] == block and f == block                                   # every level is wider than a round: one launch each
    assert g == max(min(G, -(-width // rf)), min(G, -(-width // rs)), min(G, -(-p.n // rs)))
    assert width > rf and (width % rf) != 0
    if width > G * rf:
        assert g == G                                                             # wider than the grid: grid-strided
    if width > rs:
        assert s == 2 + 2 * block + 1 and (width % rs) != 0                       # the solve's levels on a grid too
    assert res[1][0][0]["ints"][0] == 1


# ---- 3. both column forms across workgroups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blocks", "arrow"])
def test_hbm_and_lds_columns_across_workgroups(ctx, kind):
    """"sparse_lds" = 0: every column through an HBM work vector of its workgroup; 2: columns of at most two entries in LDS, the others in HBM;
    default: LDS where it fits.  The work vectors must be zero on entry and are left zero: a column that met a stale entry would differ.
    blocks: short columns, solved twice; arrow under nested dissection: every column one entry longer, the last ones long."""
    p = sparse_qp(sizes(ctx, 48, 200), "blocks", seed=5) if kind == "blocks" else sparse_qp(sizes(ctx, 40, 200), "arrow", seed=5)
    steps = [lambda bt: bt.warm_start(None, None)] if kind == "blocks" else []
    got = {}
    for lds in (0, 2, 1):
        with options(ctx, sparse_ordering=0 if kind == "blocks" else 1, sparse_gpw=1, sparse_lds=lds):
            res, plans, _ = both_modes(ctx, [p], steps=steps)
        assert plans[0][2] >= 2
        got[lds] = res[1]
    for lds in (2, 1):
        for a, b in zip(got[lds], got[0]):
            assert_same(a, b, "sparse_lds %d" % lds)
    assert got[0][0][0]["ints"][3] + got[0][0][0]["ints"][6] >= 2       # several factorisations went through the same work vectors


# ---- 4. dual termination --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", [dict(enable_dual_termination=1, dual_objective_limit=1e20), dict(proximal=0, scaling=2)], ids=["dual", "noprox"])
def test_dual_termination_and_the_factor_of_Q(ctx, st):
    """enable_dual_termination: LD_Q through the which = 1 chain (into the second value array); proximal = 0: the factorisation of Q alone
    (la = 3: no A' Sigma A, no 1 / gamma), chosen inside the kernel from the QP's scalars"""
    p = sparse_qp(sizes(ctx, 96, 320), "blocks", seed=4)
    with options(ctx, sparse_ordering=0, sparse_gpw=1):
        res, plans, perms = both_modes(ctx, [p], st=dict(ST, **st))
    r = res[1][0][0]
    assert r["ints"][0] == 1 and plans[0][2] >= 2
    o = oracle_sparse(p, perms[0][0], **dict(ST, **st))
    assert o.status_val == 1 and r["ints"][1] == int(o.info.iter) and r["ints"][3] == o.counter("n_refactor") and r["ints"][6] == o.counter("n_factor_Q")
    assert rel(r["x"], o.x) <= RTOL and rel(r["y"], o.y) <= RTOL
    if "enable_dual_termination" in st:
        assert r["dual_objective"] != 0.0 and abs(r["dual_objective"] - r["objective"]) <= 1e-4 * max(1.0, abs(r["objective"]))
        assert abs(r["dual_objective"] - o.info.dual_objective) <= 1e-8 * max(1.0, abs(o.info.dual_objective))
    else:
        assert r["ints"][6] >= 1                                          # n_factor_Q


# ---- 5. a batch of two ----------------------------------------------------------------------------------------------------------------------------
def test_batch_of_two_members_of_different_sizes_and_kinds(ctx):
    probs = [sparse_qp(60, "banded", seed=1), sparse_qp(sizes(ctx, 96, 320), "blocks", seed=2)]
    with options(ctx, sparse_ordering=0, sparse_gpw=1):
        res, plans, perms = both_modes(ctx, probs)
    assert plans[0][0] == 1 and plans[0][1] == 4                         # the natural-order band: one launch per phase
    for k, p in enumerate(probs):
        check_plan(ctx, p, perms[k][0][:p.n], plans[k])
        o = oracle_sparse(p, perms[k][0][:p.n], **ST)
        r = res[1][0][k]
        assert r["ints"][0] == o.status_val == 1 and r["ints"][1] == int(o.info.iter)
        assert rel(r["x"][:p.n], o.x) <= RTOL and rel(r["y"][:p.m], o.y) <= RTOL
    assert plans[1][2] >= 2 and plans[1][0] == 8


# ---- 6. warm-started sequence ---------------------------------------------------------------------------------------------------------------------
def test_warm_started_sequence_and_update_Q_A(ctx):
    """the recorded chains hold no values: new bounds, a new q, a warm start and new values of Q and A go through the same chains"""
    p = sparse_qp(sizes(ctx, 96, 320), "blocks", seed=6)

    def step1(bt):
        bt.update_bounds((p.bmin - 0.05)[None, :], (p.bmax + 0.1)[None, :])
        bt.update_q((1.1 * p.q)[None, :])
        bt.warm_start_last()

    def step2(bt):
        bt.update_Q_A([1.05 * p.Qx], [0.9 * p.Ax])
    with options(ctx, sparse_ordering=0, sparse_gpw=1):
        res, plans, _ = both_modes(ctx, [p], steps=[step1, step2])
    assert plans[0][2] >= 2
    assert all(r[0]["ints"][0] == 1 for r in res[1])
    assert not np.array_equal(res[1][0][0]["x"], res[1][1][0]["x"]) and not np.array_equal(res[1][1][0]["x"], res[1][2][0]["x"])
    # the oracle through the same sequence (natural ordering); new values of Q and A: a fresh oracle on them with the latest q and bounds
    o = oracle_sparse(p, **ST)
    assert rel(res[1][0][0]["x"], o.x) <= RTOL and rel(res[1][0][0]["y"], o.y) <= RTOL
    x0, y0 = o.x.copy(), o.y.copy()
    o.update_bounds(p.bmin - 0.05, p.bmax + 0.1); o.update_q(1.1 * p.q); o.warm_start(x0, y0)
    o.solve()
    assert res[1][1][0]["ints"][1] == int(o.info.iter) and rel(res[1][1][0]["x"], o.x) <= RTOL and rel(res[1][1][0]["y"], o.y) <= RTOL
    p2 = type(p)(p.n, p.m, p.Qp, p.Qi, 1.05 * p.Qx, p.Ap, p.Ai, 0.9 * p.Ax, 1.1 * p.q, p.bmin - 0.05, p.bmax + 0.1)
    o2 = oracle_sparse(p2, **ST)
    assert res[1][2][0]["ints"][1] == int(o2.info.iter) and rel(res[1][2][0]["x"], o2.x) <= RTOL and rel(res[1][2][0]["y"], o2.y) <= RTOL


# ---- 7. fallbacks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sparse_kkt", "large_batch", "dense"])
def test_fallbacks_run_on_one_workgroup(ctx, case):
    p = sparse_qp(48, "blocks", seed=3)
    probs, st, opts = [p], dict(ST), dict(sparse_ordering=0, sparse_gpw=1)
    if case == "sparse_kkt":
        st["factorization_method"] = 0
        opts["sparse_kkt"] = 1
    elif case == "large_batch":
        probs = [p, sparse_qp(40, "banded", seed=4)]
        opts["coop_max_batch"] = 1
    res = {}
    with options(ctx, **opts):
        if case == "dense":
            ctx.set_option("sparse_factor", 0)
        for mode in (0, 1):
            ctx.set_option("sparse_coop", mode)
            bt = QpalmBatch(ctx, probs, ctx.default_settings(**st))
            if case == "dense":
                with pytest.raises(QpgError) as e:
                    bt.sparse_coop_info(0)
                assert e.value.code == UNSUPPORTED
            else:
                assert all(bt.sparse_coop_info(k) == (0, 0, 0) for k in range(bt.B))
            bt.solve()
            res[mode] = snapshot(bt)
            bt.close()
    assert_same(res[1], res[0], case)
    assert all(r["ints"][0] == 1 for r in res[1])


def test_option_values(ctx):
    with options(ctx):
        with pytest.raises(QpgError):
            ctx.set_option("sparse_coop", 2)
        with pytest.raises(QpgError):
            ctx.set_option("sparse_coop", -1)        # no automatic choice

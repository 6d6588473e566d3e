"""Coop mode's grid kernels (k_co_form, k_co_factor_diag / _rows / _trailing, k_co_solve, k_co_updown, k_co_sweep; qpalm_capi.inc: coop_linear_algebra)
one operation at a time, against the high-precision references and bounds of tests/test_ops_exact.py, at the sizes where these kernels change form.

On a batch in coop mode the single operations of the boundary (ldlchol, ldlcholQAtsigmaA, ldlupdate_entering_constraints,
ldldowndate_leaving_constraints, ldlupdate_sigma_changed, ldlsolveLD_neg_dphi) run through the launch chains a suspended iteration gets (run_op);
QpalmBatch.coop_op_chains() counts them, and every case here asserts that the count moved -- and that it does not move with coop = 0.

Judges (tests/test_ops_exact.py, no constant of this module's own):
  factor            |L D L' - H| <= gamma_{n+1} |L||D||L'| + gamma_{r+2} (|Q| + |A_a|' Sigma_a |A_a| + I / gamma)             (_check_factor)
  update, downdate  err_kernel <= C_SWEEP max(err_ref, n u max|H_0|), err_ref: exact_refs.sequential_updown in fp64, C_SWEEP = 0.5    (_judge)
  sigma change      19 active rows' sigma multiplied by the settings' delta, driven as dev_update_sigma_pre leaves the state (At_sqrt_sigma at the new
                    sigma, At_scale = sqrt(delta), the rows listed in enter[]): the update's judge against H at the new sigma
  solve             |L D L' d + dphi| <= 3 gamma_n |L||D||L'||d|, L and D as read back                                           (SolveJudge)
Bit identity, as the source states it (qpalm_dense.h, "Coop mode"; tests/test_coop.py): the factor of the coop chain equals the factor of the
one-workgroup k_op (coop = 0) after the factorisation and after every update, downdate and sigma change, and coop_updates = 2 (the sweep in one
launch, tables handed from workgroup to workgroup) equals coop_updates = 1 (one launch per block column): np.array_equal on L and D.  The solve
is not part of that claim (its backward substitution sums in another order): the bound alone judges it.  One part of the claim turned out
false and its comments were corrected: after an update the grid's factor is the one-workgroup kernel's only where that kernel takes 16 ranks per
sweep as the grid does (sweeps_alike); with three or four rows per thread it takes 8, the prefix tree of a column's pivots sums other groups and
L, D differ by rounding (measured: |dL| <= 4e-14, |dD| <= 5e-12).  There both factors are judged by the bound and the two coop forms must still agree.

Measured ratios err_kernel / max(err_ref, n u max|H_0|), largest over the shapes of the table (bit-identical factors: the same figures for
coop_updates = 2 and = 1, for both grid sizes, and for the one-workgroup kernel wherever sweeps_alike below holds; where it does not -- n = 1025
on the MI355X, n = 257 and 289 on the emulator -- both kernels' ratios are 0.05 and below):
  update   (17 rows enter):             MI355X 0.230 (n = 48)   emulator 0.174 (n = 32)
  downdate (33 rows leave):             MI355X 0.197 (n = 31)   emulator 0.197 (n = 31)
  sigma    (19 rows, sigma * delta):    MI355X 0.412 (n = 32)   emulator 0.412 (n = 32)

Shapes (m = n + 40, the QPs of test_ops_exact.edge_qp; the 17 entering, 33 leaving and 19 rescaled rows include every special row, whose first
entries are in columns 0, 31, 32 and n - 1: the sweeps start in different blocks, CO_UD_JMIN):
  MI355X (512 threads, QP_NW = 8; small_workgroups = 0, asserted):  n = 31 32 33 | 47 48 49 (16-row tiles) | 63 64 65 (CO_SNB) | 127 128 129
      (CO_UD_ROWS) | 160 161 (8, then 9 row tiles below the second block column: factor_panel_update<1,2> / <2,2>) | 288 289 (a second row pass
      of co_factor_trailing) | 512 513 545 (QP_T-row chunks of co_factor_rows) | 1025 (nine workgroups in k_co_sweep).  Grid: the fixture's
      coop_workgroups = 256, and the shapes from n = 257 on again with coop_workgroups = 8, the smallest grid the library uses: more items than
      workgroups in co_factor_trailing, co_factor_rows and k_co_updown's phase 2.  At n = 33 every grid is clamped to a single workgroup (grid_for).
  emulator (QP_T = 128, QP_NW = 2; a grid's workgroups run one after the other: indexing and edges, not hand-over races):  n = 31 32 33 | 63 64 65
      (CO_SNB; two, then three row tiles below the second block column) | 96 97 (a second row pass: QP_FNT QP_NW = 4 tiles) | 127 128 129
      (CO_UD_ROWS, QP_T) | 161 (one row past a QP_T chunk below the first block) | 257 289 (three workgroups in k_co_sweep; a ragged last
      block).  Grid: the fixture's coop_workgroups = 3 is raised to 8 by the library (coop_grid), so the pass at 8 is the only one there.
"""
import numpy as np
import pytest

from oracle import binding as ob
from tests import exact_refs as xr
from tests.test_ops_exact import (ST, Case, Opened, SolveJudge, _check_factor, _judge, _run_updown, _updown_errors, solve_rhs)
from tests.test_parity import RTOL, rel

HIP_N = (31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 160, 161, 288, 289, 512, 513, 545, 1025)
EMU_N = (31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 161, 257, 289)
SMALL_GRID = 8                      # coop_grid's lower limit (qpalm_capi.inc)
TABLE = ([(Case("hip", 0, n, 512), None) for n in HIP_N] + [(Case("hip", 0, n, 512), SMALL_GRID) for n in HIP_N if n >= 257] +
         [(Case("emu", 1, n, 128), None) for n in EMU_N])
LDLCHOL = [Case("hip", 0, n, 512) for n in (33, 289, 1025)] + [Case("emu", 1, n, 128) for n in (33, 161, 289)]
REPLAY = [Case("hip", 0, 289, 512), Case("emu", 1, 161, 128)]


def grid_cases(lst):
    return pytest.mark.parametrize("ctx,case,wg", [c.param(wg, suffix="" if wg is None else "-g%d" % wg) for c, wg in lst], indirect=["ctx"])


def cases(lst):
    return pytest.mark.parametrize("ctx,case", [c.param() for c in lst], indirect=["ctx"])


def _grid(wg):
    return {} if wg is None else dict(coop_workgroups=wg)


def counted(o, expect, fn, *args):
    """fn(*args), asserting that `expect` single operations of the batch went to the grid kernels meanwhile"""
    c0 = o.bt.coop_op_chains()
    out = fn(*args)
    moved = o.bt.coop_op_chains() - c0
    assert moved == expect, (o.case.id, fn.__name__, moved, expect)
    return out


# the three ways an update runs: (name, coop, coop_updates, single operations on the grid per factorise-and-update)
MODES = (("coop, one-launch sweep", 1, 2, 2), ("coop, one launch per block", 1, 1, 2), ("one workgroup", 0, 2, 0))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def sweeps_alike(case):
    """does the one-workgroup sweep take its ranks 16 at a time, as the grid's sweeps do?  dense_updown takes QP_KSEL(rows per thread) ranks per sweep:
    16 with one or two rows per thread, 8 with three or four; beyond four rows per thread dense_updown_big takes 16.  A column's pivots are summed
    by a prefix tree over the ranks of ONE sweep (qp_rank_pivots), so other groups of ranks round differently: with three or four rows per thread
    (n = 1025 on 512 threads, n = 257 and 289 on the emulator's 128) the two factors differ in the last bits and only the bound judges them."""
    rpt = -(-case.n // case.threads)
    return rpt <= 2 or rpt > 4


def _judge_and_compare(o, what, runs, errors):
    """runs: [(mode name, (L0, D0, L, D))] of the same operation on the same state, the coop chain first, the one-workgroup kernel last.  Every distinct
    result is judged by `errors` (L0, D0, L, D) -> (e_k, e_r, floor); then all of them must be the same bits -- the two coop forms always, the
    one-workgroup kernel where sweeps_alike"""
    judged = []
    for name, res in runs:
        twin = [n for n, r in judged if same(r, res)]
        if twin:
            print("%s %s: %s: the same bits as %s" % (what, o.case.id, name, twin[0]))
            continue
        if judged:
            print("%s %s: %s DIFFERS from %s: max |dL| = %.3g, max |dD| = %.3g" % (
                what, o.case.id, name, judged[0][0], np.max(np.abs(res[2] - judged[0][1][2])), np.max(np.abs(res[3] - judged[0][1][3]))))
        judged.append((name, res))
    for name, res in judged:
        _judge(o, "%s (%s)" % (what, name), *errors(*res))
    allowed = {runs[0][0]} if sweeps_alike(o.case) else {runs[0][0], runs[-1][0]}
    assert {n for n, _ in judged} <= allowed, (what, o.case.id, [n for n, _ in judged])


# ------------------------------------------------------------------------------------------------------------------ 1. factor
@grid_cases(TABLE)
def test_factor(ctx, case, wg):
    with Opened(ctx, case, coop=1, **_grid(wg)) as o:
        L, D = counted(o, 1, _check_factor, o)
        ctx.set_option("coop", 0)
        L1, D1 = counted(o, 0, o.factor_of, o.base_active() + o.special_rows())
        assert np.array_equal(L, L1) and np.array_equal(D, D1), (case.id, np.max(np.abs(L - L1)), np.max(np.abs(D - D1)))


@cases(LDLCHOL)
def test_ldlchol(ctx, case):
    """Q + I / gamma alone (pend_la = 3: k_co_form leaves A' Sigma A out)"""
    with Opened(ctx, case, coop=1) as o:
        L, D = counted(o, 1, _check_factor, o, [], "ldlchol")
        ctx.set_option("coop", 0)
        L1, D1 = counted(o, 0, o.factor_of, [], "ldlchol")
        assert np.array_equal(L, L1) and np.array_equal(D, D1), (case.id, np.max(np.abs(L - L1)), np.max(np.abs(D - D1)))


# ------------------------------------------------------------------------------------------------------------------ 2. update / downdate
def _updown_all_modes(ctx, o, what, start, change, sign):
    runs = []
    new_rows = None
    for name, coop, cu, chains in MODES:
        ctx.set_option("coop", coop)
        ctx.set_option("coop_updates", cu)
        L0, D0, L, D, new_rows = counted(o, chains, _run_updown, o, start, change, sign)
        runs.append((name, (L0, D0, L, D)))
    H0, Hn, W = o.H(start), o.H(new_rows), o.update_vectors(change)
    _judge_and_compare(o, what, runs, lambda L0, D0, L, D: _updown_errors(o, L0, D0, L, D, H0, Hn, W, sign))


@grid_cases(TABLE)
def test_update_17_rows_enter(ctx, case, wg):
    """two sweeps (16 ranks, then one); the entering rows include every special row of A"""
    with Opened(ctx, case, coop=1, **_grid(wg)) as o:
        enter = o.entering(17)
        assert set(o.special_rows()) <= set(enter)
        _updown_all_modes(ctx, o, "update", o.base_active(), enter, +1)


@grid_cases(TABLE)
def test_downdate_33_rows_leave(ctx, case, wg):
    """three sweeps (16, 16, one); the leaving rows include every special row of A"""
    with Opened(ctx, case, coop=1, **_grid(wg)) as o:
        start = o.base_active() + o.entering(17)
        leave = (o.special_rows() + o.base_active())[:33]
        assert len(leave) == 33 and set(leave) <= set(start)
        _updown_all_modes(ctx, o, "downdate", start, leave, -1)


# ------------------------------------------------------------------------------------------------------------------ 3. sigma change
@grid_cases(TABLE)
def test_sigma_of_19_rows_changed(ctx, case, wg):
    """ldlupdate_sigma_changed (solver_interface.c:443-503): two sweeps.  The state before the call is the one dev_update_sigma_pre leaves: the changed
    rows of At_sqrt_sigma at the NEW sigma (= delta sigma), At_scale = sqrt(delta) there and 1 elsewhere.  The operation scales those rows by
    sqrt(1 - 1 / At_scale^2) (its first step, on the QP's workgroup), applies them as rank-1 updates (the grid) and scales At_sqrt_sigma back
    (its last step, on the QP's workgroup again).
    The other active rows carry delta sigma already (raised by an earlier update, as happens in a solve, where the rows are raised in turns).  The
    update's judge takes its floor n u max|H_0| at the matrix BEFORE the change and C_SWEEP < 1 presumes that floor above both errors; a change
    that multiplies the largest entries of H by delta = 100 has the rounding of the new entries, u max|H_new|, far above it, in the kernel and in
    the fp64 reference alike.  Measured with every other row at the base sigma (emulator, max|H_new| = 80 max|H_0|): kernel 0.6e-11 .. 1.6e-11,
    reference 0.6e-11 .. 2.0e-11, floor 1.2e-12 .. 1.6e-11, ratios 0.38 .. 1.64 -- the two fp64 computations against each other, which C_SWEEP
    cannot judge.  With the other rows raised before, max|H_0| is max|H_new| to a factor 1.5 and the judge means what it means for an update."""
    with Opened(ctx, case, coop=1, **_grid(wg)) as o:
        bt, n, m = o.bt, case.n, case.m
        start = o.base_active() + o.special_rows()
        changed = (o.special_rows() + o.base_active())[:19]
        before = [i for i in start if i not in set(changed)]
        assert len(changed) == 19 and len(before) >= 8
        delta = float(bt.settings.delta)
        s = float(np.sqrt(delta))
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in o.Arows])]).astype(np.int64)
        nnz = int(o.p.Ap[-1])
        assert ptr[-1] == nnz
        Atss = bt.named_vec("At_sqrt_sigma", nnz)
        for i in changed:    # the layout this test relies on: the rows of A one after the other, columns ascending
            want = np.sqrt(o.sigma[i]) * np.array([v for _, v in o.Arows[i]])
            assert np.allclose(Atss[ptr[i]:ptr[i + 1]], want, rtol=1e-14, atol=0.0), i
        Atss0, sigma0 = Atss.copy(), o.sigma.copy()
        for i in before:
            Atss0[ptr[i]:ptr[i + 1]] *= s
            sigma0[i] = delta * sigma0[i]
        Atss1, scale, sigma1 = Atss0.copy(), np.ones(m), sigma0.copy()
        t = float(np.sqrt(1.0 - 1.0 / (s * s)))      # dev_ldlupdate_sigma_scale's arithmetic
        W = np.zeros((len(changed), n))              # the update vectors as the sweeps get them
        for k, i in enumerate(changed):
            Atss1[ptr[i]:ptr[i + 1]] *= s
            scale[i] = s
            sigma1[i] = delta * sigma1[i]
            for e, (j, _) in zip(range(int(ptr[i]), int(ptr[i + 1])), o.Arows[i]):
                W[k, j] = Atss1[e] * t

        def run():
            bt.set_vec("At_sqrt_sigma", Atss0)
            bt.set_vec("At_scale", np.ones(m))
            L0, D0 = o.factor_of(start)
            bt.set_vec("At_sqrt_sigma", Atss1)
            bt.set_vec("At_scale", scale)
            bt.set_ivec("enter", changed)
            bt.set_scalar("nb_sigma_changed", len(changed))
            bt.op("ldlupdate_sigma_changed")
            L, D = bt.factor(0)
            return (L0, D0, L, D), (bt.vec("At_scale")[:m], bt.named_vec("At_sqrt_sigma", nnz))

        runs, lefts = [], []
        for name, coop, cu, chains in MODES:
            ctx.set_option("coop", coop)
            ctx.set_option("coop_updates", cu)
            res, left = counted(o, chains, run)
            runs.append((name, res))
            lefts.append(left)
        # the two steps on the QP's own workgroup ran, in every mode alike: At_scale inverted, At_sqrt_sigma back at the new sigma
        for left in lefts:
            assert np.array_equal(left[0], lefts[-1][0]) and np.array_equal(left[1], lefts[-1][1])
        assert np.array_equal(lefts[0][0][changed], np.full(len(changed), 1.0 / t)) and rel(lefts[0][1], Atss1) <= 1e-15
        H0 = xr.schur_matrix(o.Qrows, o.Arows, sigma0, start, o.gamma)
        Hn = xr.schur_matrix(o.Qrows, o.Arows, sigma1, start, o.gamma)
        print("sigma change %s: max|H_0| = %.3g, max|H_new| = %.3g" % (case.id, float(np.max(np.abs(H0))), float(np.max(np.abs(Hn)))))
        _judge_and_compare(o, "sigma change", runs, lambda L0, D0, L, D: _updown_errors(o, L0, D0, L, D, H0, Hn, W, +1))


# ------------------------------------------------------------------------------------------------------------------ 4. solve
@grid_cases(TABLE)
def test_solve(ctx, case, wg):
    with Opened(ctx, case, coop=1, **_grid(wg)) as o:
        bt = o.bt
        L, D = counted(o, 1, o.factor_of, o.base_active() + o.special_rows())
        judge = SolveJudge(case, L, D)
        for name, rhs in solve_rhs(case.n):
            bt.set_vec("dphi", rhs)
            counted(o, 1, bt.op, "ldlsolveLD_neg_dphi")
            judge.check(bt.vec("d"), rhs, name)


# ------------------------------------------------------------------------------------------------------------------ 5. replayed chains
def _replay_updates(ctx, case, graphs, judged):
    """factorise, update, factorise, downdate with 17, 3 and 33 rows on ONE batch: the first, second and later uses of the same launch chains (plain,
    recorded, replayed as a graph where the backend has graphs) with different rank counts, which the kernels read from the QP's scalars"""
    out = []
    with Opened(ctx, case, coop=1, coop_graphs=graphs) as o:
        base = o.base_active()
        for count in (17, 3, 33):
            rows = o.entering(count)
            for what, start, sign in (("update", base, +1), ("downdate", base + rows, -1)):
                L0, D0, L, D, new_rows = counted(o, 2, _run_updown, o, start, rows, sign)
                if judged:
                    e = _updown_errors(o, L0, D0, L, D, o.H(start), o.H(new_rows), o.update_vectors(rows), sign)
                    _judge(o, "%s of %d rows, coop_graphs = %d" % (what, count, graphs), *e)
                out.append((L0, D0, L, D))
    return out


@cases(REPLAY)
def test_replayed_update_chains(ctx, case):
    with_graphs = _replay_updates(ctx, case, 1, True)
    plain = _replay_updates(ctx, case, 0, False)
    for k, (a, b) in enumerate(zip(with_graphs, plain)):
        assert same(a, b), (case.id, k)


def _replay_solves(ctx, case, graphs, judged):
    out = []
    with Opened(ctx, case, coop=1, coop_graphs=graphs) as o:
        bt, n = o.bt, case.n
        L, D = counted(o, 1, o.factor_of, o.base_active() + o.special_rows())
        judge = SolveJudge(case, L, D) if judged else None
        rng = np.random.default_rng(900 + n)
        for k in range(3):
            rhs = rng.standard_normal(n) * 10.0 ** k
            bt.set_vec("dphi", rhs)
            counted(o, 1, bt.op, "ldlsolveLD_neg_dphi")
            d = bt.vec("d")
            if judged:
                judge.check(d, rhs, "solve %d, coop_graphs = %d" % (k, graphs))
            out.append(d)
    return out


@cases(REPLAY)
def test_replayed_solve_chain(ctx, case):
    with_graphs = _replay_solves(ctx, case, 1, True)
    plain = _replay_solves(ctx, case, 0, False)
    for k, (a, b) in enumerate(zip(with_graphs, plain)):
        assert np.array_equal(a, b), (case.id, k)
    assert not np.array_equal(with_graphs[0], with_graphs[1])


# ------------------------------------------------------------------------------------------------------------------ 6. nothing left behind
@cases(REPLAY)
def test_solve_after_single_operations(ctx, case):
    """every single operation once on the grid, then a whole solve of the same batch in coop mode against the oracle: no pend_* field, table or
    counter word of the operations is left for the solve to trip over"""
    o_ref = ob.OracleQP(*edge_args(case), settings=ob.default_settings(**ST))
    o_ref.solve()
    with Opened(ctx, case, coop=1) as o:
        bt, m = o.bt, case.m
        base, enter = o.base_active(), o.entering(17)
        counted(o, 2, _run_updown, o, base, enter, +1)
        counted(o, 2, _run_updown, o, base + enter, enter, -1)
        counted(o, 1, o.factor_of, [], "ldlchol")
        o.factor_of(base + o.special_rows())
        scale = np.ones(m)
        scale[base[:3]] = 10.0
        bt.set_vec("At_scale", scale)
        bt.set_ivec("enter", base[:3])
        bt.set_scalar("nb_sigma_changed", 3)
        counted(o, 1, bt.op, "ldlupdate_sigma_changed")
        bt.set_vec("dphi", np.ones(case.n))
        counted(o, 1, bt.op, "ldlsolveLD_neg_dphi")
        bt.warm_start(None, None)       # a new qpalm_solve from the cold start, as the oracle's
        bt.solve()
        x, y = bt.solution()
        info = bt.info(0)
        assert int(info.status_val) == o_ref.status_val == 1 and int(info.iter) == int(o_ref.info.iter), (info.status_val, info.iter, o_ref.info.iter)
        assert rel(x[0], o_ref.x) <= RTOL and rel(y[0], o_ref.y) <= RTOL
        assert int(bt.stats(0).n_fused_solve) == 0      # (the grid ran the solve's linear algebra)


def edge_args(case):
    from tests.test_ops_exact import edge_qp
    return edge_qp(case.n, case.m, 7000 + case.n)[0].args()


# ------------------------------------------------------------------------------------------------------------------ 7. which path
@cases(REPLAY)
def test_coop_off_keeps_the_single_workgroup(ctx, case):
    """coop = 0: no operation goes to the grid.  coop = 1: the six factor operations do, nothing else does; coop_updates = 0 keeps the updates on
    the QP's workgroup, as a solve in coop mode does"""
    with Opened(ctx, case) as o:
        bt = o.bt
        base, enter = o.base_active(), o.entering(3)
        counted(o, 0, _run_updown, o, base, enter, +1)
        counted(o, 0, bt.op, "ldlsolveLD_neg_dphi")
        ctx.set_option("coop", 1)
        counted(o, 0, bt.op, "compute_residuals")
        counted(o, 0, bt.op, "set_active_constraints")
        counted(o, 0, bt.mat_vec, "A", np.ones(case.n))
        ctx.set_option("coop_updates", 0)
        counted(o, 1, _run_updown, o, base, enter, +1)          # the factorisation alone
        ctx.set_option("coop_updates", 2)
        counted(o, 2, _run_updown, o, base, enter, +1)


@pytest.mark.parametrize("ctx,n,routed", [pytest.param("hip", n, r, id="hip-n%d" % n, marks=pytest.mark.gpu) for n, r in ((545, 0), (1025, 1))], indirect=["ctx"])
def test_automatic_choice_is_coop_wanteds(ctx, n, routed):
    """coop = -1: the operations of one QP go to the grid from 640 factor rows on, like its solves (coop_wanted)"""
    with Opened(ctx, Case("hip", 0, n, 512), coop=-1) as o:
        counted(o, routed, o.factor_of, o.base_active())

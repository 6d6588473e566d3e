"""The diagonal-block recurrence of the rank-update sweep (qpalm_dense.h: dense_updown, the panel wave's column loop) at the edges of its forms:
one reciprocal per column and rank group, and the block's part of the fused forward substitution riding in the column loop.

The updated factor is judged as tests/test_ops_exact.py judges sweeps (same helpers, same constant, tests/exact_refs.py untouched):
  err_kernel = max|L D L' - H_new| (longdouble) <= C_SWEEP max(err of the sequential fp64 rank-1 recurrence, n u max|H_0|).

Shapes: n = 31, 32, 33, 64, 65 on the 512-thread instance, n = 255 on the 256-thread and n = 127 on the 128-thread one (the emulator has the
128-thread instance only: the same n).  Ranks per call 1, 8, 9, 15, 16, 17, 33: one lane, half a DPP row, a full row and one beyond (a second
sweep), two sweeps and one rank of a third (sweep_ranks = 32: both rank groups, then one rank).  The entering / leaving rows start with the
special rows of edge_qp (first nonzero in column 0, 31, 32, n - 1, last column only), so from eight ranks on a sweep holds ranks whose vector is
zero in its first columns (the `wv == 0.0` branch).

Paths: the single operations (unfused sweeps: entering, leaving, sigma changed) and a whole iteration built so that its Newton step rides on
sweeps of entering and leaving rows with the sign changing inside a rank group (fused; 16- and 32-rank form).  Pivot modes: the guarded tree (default), running pivots
(sequential_rank_sums = 1), and a downdate into a numerically singular matrix in which the guard re-sums columns."""
import numpy as np
import pytest
import scipy.sparse as sp

from qpalm_amd.problems import random_qp
from qpalm_amd.solver import QpalmBatch
from tests import exact_refs as xr
from tests.test_ops_exact import C_SWEEP, ST, Case, Opened, _judge, _updown, check_conditioning, product_error, worst_ratio
from tests.test_parity import _with_Q

RANKS = (1, 8, 9, 15, 16, 17, 33)
SHAPES = ([Case("hip", 0, n, 512) for n in (31, 32, 33, 64, 65)] + [Case("hip", 1, 255, 256), Case("hip", 2, 127, 128)] +
          [Case("emu", 1, n, 128) for n in (31, 32, 33, 64, 65, 127)])
SHAPES32 = [Case("hip", 0, 65, 512), Case("emu", 1, 65, 128)]


def shapes(lst):
    return pytest.mark.parametrize("ctx,case", [c.param() for c in lst], indirect=["ctx"])


def _first_nonzero(o, rows):
    return [min((j for j, _ in o.Arows[int(i)]), default=o.case.n) for i in rows]


def _enter_and_leave(o, ranks, what):
    """every rank count once as an update and once as a downdate; returns the factors by (sign, ranks)"""
    out = {}
    for k in ranks:
        enter = o.entering(k)
        if k >= 8:          # a rank whose vector is zero in the sweep's first columns rides along
            f = _first_nonzero(o, enter[:min(k, 16)])
            assert max(f) > min(f)
        e_k, e_r, floor, L, D = _updown(o, o.base_active(), enter, +1)
        _judge(o, "%s, %d rows enter" % (what, k), e_k, e_r, floor)
        out[+1, k] = (L, D)
        start = o.base_active() + o.entering(17)
        leave = (o.special_rows() + o.base_active())[:k]
        assert len(leave) == k and set(leave) <= set(start)
        e_k, e_r, floor, L, D = _updown(o, start, leave, -1)
        _judge(o, "%s, %d rows leave" % (what, k), e_k, e_r, floor)
        out[-1, k] = (L, D)
    return out


@shapes(SHAPES)
def test_rank_counts_updates_and_downdates(ctx, case):
    with Opened(ctx, case) as o:
        _enter_and_leave(o, RANKS, "guarded tree")
        assert int(o.bt.stats(0).n_seq_columns) == 0       # well conditioned: the guard never fired, the tree form is what was judged


@shapes(SHAPES)
def test_rank_counts_running_pivots(ctx, case):
    """sequential_rank_sums = 1: every column's pivots as running sums"""
    try:
        with Opened(ctx, case, sequential_rank_sums=1) as o:
            _enter_and_leave(o, RANKS, "running pivots")
    finally:
        ctx.set_option("sequential_rank_sums", -1)


@shapes(SHAPES32)
def test_both_rank_groups_bit_identical_to_two_sweeps(ctx, case):
    """sweep_ranks = 32: 17 ranks (group 1 holds one), 33 (both groups full, then a sweep of one); the same bits as the 16-rank form's sweeps"""
    out = {}
    for sr in (16, 32):
        with Opened(ctx, case, sweep_ranks=sr) as o:
            out[sr] = _enter_and_leave(o, (17, 33), "sweep_ranks = %d" % sr)
    for key in out[16]:
        assert np.array_equal(out[16][key][0], out[32][key][0]) and np.array_equal(out[16][key][1], out[32][key][1]), key


@shapes(SHAPES)
def test_sigma_changed_is_an_unfused_sweep(ctx, case):
    """ldlupdate_sigma_changed: the penalties of k active rows grow by At_scale^2 = 4: H gains sigma_i (1 - 1 / 4) a_i a_i' for each; k as above"""
    with Opened(ctx, case) as o:
        n, bt = case.n, o.bt
        start = o.base_active() + o.entering(33)
        for k in RANKS:
            changed = o.entering(k)
            L0, D0 = o.factor_of(start)
            scale = np.ones(case.m); scale[changed] = 2.0
            bt.set_vec("At_scale", scale)
            bt.set_ivec("enter", changed); bt.set_scalar("nb_sigma_changed", len(changed))
            bt.op("ldlupdate_sigma_changed")
            L, D = bt.factor(0)
            assert np.all(np.isfinite(L)) and np.all(np.isfinite(D))
            W = np.sqrt(0.75) * o.update_vectors(changed)
            H0 = o.H(start)
            Hn = H0.copy()
            for w in W:
                wl = np.asarray(w, dtype=xr.LD)
                Hn += np.outer(wl, wl)
            check_conditioning(Hn)
            Lr, Dr = xr.sequential_updown(L0, D0, W, +1)
            e_k = float(np.max(np.abs(product_error(L, D, Hn, None))))
            e_r = float(np.max(np.abs(product_error(Lr, Dr, Hn, None))))
            _judge(o, "sigma changed, %d rows" % k, e_k, e_r, n * xr.U * float(np.max(np.abs(H0))))


FUSED = ([c.param(16) for c in SHAPES] +
         [c.param(32, suffix="-sweep32") for c in SHAPES32])      # (32 ranks: the substitution is a loop of its own behind the recurrence there)
MIXED = ((5, 7), (9, 20), (17, 3))     # (rows made to enter, rows made to leave): the sign changes at rank 5, 9 and 17 = rank 1 of the second group


@pytest.mark.parametrize("ctx,case,sweep_ranks", FUSED, indirect=["ctx"])
def test_newton_step_rides_on_a_sweep_of_both_signs(ctx, case, sweep_ranks):
    """The fused path is reached through whole iterations only: a Newton step whose active set differs from `active_old` updates the factor (entering
    rows first, then leaving rows, in the same sweeps) and the last sweep does the forward substitution of the solve that follows.  The test builds
    such a step: it takes rows out of `active_old` that are active (they enter) and puts rows in that are not (they leave), factorises that set, and
    lets the solver take one iteration.  Counted are only steps that were fused updates (n_fused_solve + 1, no refactorisation, sigma and gamma as
    before) with entering AND leaving rows and the change of sign inside a group of 16 ranks (rows read back from the active sets, asserted).  Then
      * the updated factor is judged like every sweep of this file: against the sequential fp64 recurrence under C_SWEEP, with the longdouble H of the
        new active set;
      * d solves L D L' d = -dphi under the solve's componentwise bound (test_ops_exact: 3 gamma_n |L||D||L'||d|);
      * d agrees with the solve through a fresh factorisation (L_f, D_f) of the same set.  With H the exact matrix, |L D L' - H| <= B_1 entrywise (the
        sweep bound just asserted, so at most n B_1 in the Frobenius norm) and |L_f D_f L_f' - H| <= B_2 (test_factor's componentwise bound, asserted
        here), and both solves backward stable, to first order
          |d - d_f|_2 <= |H^-1|_2 ((|E_1|_F + n B_1) |d|_2 + (|E_2|_F + |B_2|_F) |d_f|_2),   |E_i| <= 3 gamma_n |L_i||D_i||L_i'|;
        twice that is allowed.  Nothing in the allowance is measured on the factor under test."""
    with Opened(ctx, case, sweep_ranks=sweep_ranks) as o:
        n, m, bt = case.n, case.m, o.bt
        # the reference's rule refactorises when more than max_rank_update_fraction (n + m) rows change: here every change is an update
        assert bt.update_settings(ctx.default_settings(**dict(ST, max_rank_update_fraction=1.0))) == 0
        bt.iterate(4)                                      # (the active set is empty after the first iterations)
        done = 0
        for ke, kl in MIXED:
            act = bt.ivec("active")
            on, off = np.where(act == 1)[0], np.where(act == 0)[0]
            if len(on) < ke or len(off) < kl:
                continue
            old = act.copy(); old[on[:ke]] = 0; old[off[:kl]] = 1
            sig0, s0 = bt.vec("sigma")[:m].copy(), bt.stats(0)
            o.sigma, o.gamma = sig0, float(s0.gamma)
            old_rows = [int(i) for i in np.where(old == 1)[0]]
            L0, D0 = o.factor_of(old_rows)
            bt.set_ivec("active_old", old); bt.set_scalar("reset_newton", 0)
            s0 = bt.stats(0)
            bt.iterate(1)
            s1, act2 = bt.stats(0), bt.ivec("active")
            enter = [int(i) for i in np.where((act2 == 1) & (old == 0))[0]]
            leave = [int(i) for i in np.where((act2 == 0) & (old == 1))[0]]
            print("%s: %d rows entered, %d left, fused solves +%d, refactorisations +%d, rank-1 changes +%d" % (
                case.id, len(enter), len(leave), int(s1.n_fused_solve) - int(s0.n_fused_solve), int(s1.n_refactor) - int(s0.n_refactor),
                int(s1.n_rank1) - int(s0.n_rank1)))
            if (int(s1.n_fused_solve) != int(s0.n_fused_solve) + 1 or int(s1.n_refactor) != int(s0.n_refactor) or float(s1.gamma) != o.gamma or
                    not np.array_equal(bt.vec("sigma")[:m], sig0) or int(s1.n_rank1) - int(s0.n_rank1) != len(enter) + len(leave)):
                continue                                  # (not a plain fused update step: an outer iteration came first)
            if not (enter and leave and len(enter) % 16 != 0):
                continue
            done += 1
            # 1. the factor the fused sweeps left
            L, D = bt.factor(0)
            d, dphi = bt.vec("d"), bt.vec("dphi")
            assert np.all(np.isfinite(d)) and np.all(np.isfinite(L)) and np.all(np.isfinite(D))
            new_rows = [int(i) for i in np.where(act2 == 1)[0]]
            H0, Hn = o.H(old_rows), o.H(new_rows)
            check_conditioning(H0); check_conditioning(Hn)
            Lr, Dr = xr.sequential_updown(L0, D0, o.update_vectors(enter), +1)
            Lr, Dr = xr.sequential_updown(Lr, Dr, o.update_vectors(leave), -1)
            e_k = float(np.max(np.abs(product_error(L, D, Hn, None))))
            e_r = float(np.max(np.abs(product_error(Lr, Dr, Hn, None))))
            floor = n * xr.U * float(np.max(np.abs(H0)))
            _judge(o, "fused, %d enter + %d leave, sweep_ranks = %d" % (len(enter), len(leave), sweep_ranks), e_k, e_r, floor)
            B1 = C_SWEEP * max(e_r, floor)
            # 2. the direction against the factor as read back
            Lu = xr.unit_lower(L)
            Ll, Dl = np.asarray(Lu, dtype=xr.LD), np.asarray(D, dtype=xr.LD)
            res = np.abs(Ll @ (Dl * (Ll.T @ np.asarray(d, dtype=xr.LD))) + np.asarray(dphi, dtype=xr.LD))
            A1 = xr.ldl_abs_product(Lu, D)
            ratio = worst_ratio(res, 3 * xr.gamma_k(n) * (A1 @ np.abs(d)))
            print("   fused solve: max residual / bound = %.3g" % ratio)
            assert ratio <= 1.0, (case.id, ratio)
            # 3. the same right-hand side through a fresh factorisation of the same set (the iteration goes on from that factor)
            bt.op("ldlcholQAtsigmaA")
            Lf, Df = bt.factor(0)
            bt.op("ldlsolveLD_neg_dphi")
            df = bt.vec("d")
            Lfu = xr.unit_lower(Lf)
            A2 = xr.ldl_abs_product(Lfu, Df)
            B2 = xr.gamma_k(n + 1) * A2 + xr.gamma_k(xr.longest_column(o.Arows, new_rows, n) + 2) * np.asarray(o.H(new_rows, absolute=True), dtype=np.float64)
            assert worst_ratio(np.abs(product_error(Lf, Df, Hn, None)), B2) <= 1.0
            inv = 1.0 / float(np.min(np.linalg.eigvalsh(np.asarray(Hn, dtype=np.float64))))
            E1, E2 = 3 * xr.gamma_k(n) * np.linalg.norm(A1), 3 * xr.gamma_k(n) * np.linalg.norm(A2)
            tol = 2 * inv * ((E1 + n * B1) * np.linalg.norm(d) + (E2 + np.linalg.norm(B2)) * np.linalg.norm(df))
            print("   against a fresh factorisation: |d - d_f| = %.3g, allowed %.3g" % (np.linalg.norm(d - df), tol))
            assert np.linalg.norm(d - df) <= tol, (case.id, np.linalg.norm(d - df), tol)
        assert done > 0, case.id


def test_guard_resums_columns_of_a_singular_downdate(ctx):
    """test_parity's downdate into a numerically singular matrix (86 of 90 active rows leave, lambda_min 150 -> 1e-7, Q = 1e-10 I) in the default
    pivot mode: the guard must fire (n_seq_columns > 0) and the factor stay backward stable; the sequential fp64 reference on the same inputs must
    itself be within the bound (checked on every backend: it is plain numpy)."""
    n, m = 40, 120
    st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, scaling=0, gamma_init=1e7, gamma_max=1e7, sigma_init=1e3)
    p = _with_Q(random_qp(n, m, seed=9100, density_A=0.08, density_M=0.05), "tiny")
    bt = QpalmBatch(ctx, [p], ctx.default_settings(**st))
    try:
        bt.begin_solve()
        bt.iterate(2)
        A = sp.csc_matrix((p.Ax, p.Ai, p.Ap), shape=(p.m, p.n)).toarray()
        Ql = sp.csc_matrix((p.Qx, p.Qi, p.Qp), shape=(p.n, p.n)).toarray()
        Qd = Ql + np.tril(Ql, -1).T
        act = np.zeros(m, dtype=np.int64); act[:90] = 1
        bt.set_ivec("active", act)
        bt.op("ldlcholQAtsigmaA")
        L0, D0 = bt.factor(0)
        leave = np.where(act == 1)[0][2:88]
        bt.set_ivec("leave", leave); bt.set_scalar("nb_leave", len(leave)); bt.set_scalar("nb_enter", 0)
        bt.op("ldldowndate_leaving_constraints")
        L, D = bt.factor(0)
        assert int(bt.stats(0).n_seq_columns) > 0
        sig, gam = bt.vec("sigma", 0)[:m], float(bt.stats(0).gamma)
        keep = act.copy(); keep[leave] = 0
        LD = xr.LD
        Al = np.asarray(A, dtype=LD)
        H = np.asarray(Qd, dtype=LD) + (Al[keep == 1].T * np.asarray(sig[keep == 1], dtype=LD)) @ Al[keep == 1] + np.eye(n, dtype=LD) / LD(gam)
        H0 = Qd + (A[act == 1].T * sig[act == 1]) @ A[act == 1] + np.eye(n) / gam
        W = np.sqrt(sig[leave])[:, None] * A[leave]
        Lr, Dr = xr.sequential_updown(L0, D0, W, -1)
        e_k = float(np.max(np.abs(product_error(L, D, H, None))))
        e_r = float(np.max(np.abs(product_error(Lr, Dr, H, None))))
        floor = n * xr.U * float(np.max(np.abs(H0)))
        print("singular downdate: kernel %.3g, sequential fp64 reference %.3g, n u max|H0| %.3g" % (e_k, e_r, floor))
        assert e_r <= 16 * floor                          # the reference alone is backward stable on these inputs
        assert e_k <= C_SWEEP * max(e_r, floor), (e_k, e_r, floor)
    finally:
        bt.close()

"""Single operations of the boundary (include/qpalm_gfx950.h: ldlcholQAtsigmaA, ldlupdate_entering_constraints, ldldowndate_leaving_constraints,
ldlsolveLD_neg_dphi, mat_vec / mat_tpose_vec, exact_linesearch) against high-precision references (tests/exact_refs.py: numpy longdouble and
Fraction; no oracle, no kernel), at the sizes where the kernels change form: the 32-column blocks of the factor, solve and sweep kernels, the
rows-per-thread instances k_op<1|2|4|0> (rpt = ceil(n / threads): 512/513, 1024/1025, 2048/2049 on 512 threads, 128/129 and 256 on 128 threads), the
choice of the workgroup size, the sub-wavefront row walk of the SpMV and the power-of-two padding of the line search's sort.

Every bound but one is a textbook componentwise bound (gamma_k = k u / (1 - k u), u = 2^-53), valid for any summation order and for FMA:
  factor   |L D L' - H|        <= gamma_{n+1} |L||D||L'| + gamma_{r+2} (|Q| + |A_a|' Sigma_a |A_a| + I / gamma),   r = longest column of A_a
  solve    |L D L' d + dphi|   <= 3 gamma_n |L||D||L'||d|                                  (L, D as read back: dense_solve alone is judged)
  SpMV     |y - A x|           <= gamma_r |A||x|,   r = length of the row;   an empty row gives exactly 0.0
  search   |psi'(tau)|         <= 2 m u (sum of the absolute values of the terms of psi' at tau)
The rank-update sweep has no such constant.  Its error max|L D L' - H_new| is compared with that of a plain sequential rank-1 recurrence in fp64
(exact_refs.rank1_updown, Gill-Golub-Murray-Saunders C1) applied to the same starting factor and the same rows:
  err_kernel <= C_SWEEP max(err_ref, n u max|H_0|).
Measured ratios err_kernel / max(err_ref, n u max|H_0|), largest over all shapes of the table:
  update   (17 rows enter):             MI355X 0.174 (n = 32)   emulator 0.174 (n = 32)
  downdate (33 rows leave):             MI355X 0.197 (n = 31)   emulator 0.197 (n = 31)
  32-rank form (33 rows enter):         MI355X 0.063 (n = 65)   emulator 0.063 (n = 65), the same as the 16-rank form's, bit for bit
  (at n >= 1024: 0.01 and below.  On these well-conditioned matrices the kernel's error and the reference's agree to within a factor 2.5 at every
  shape -- 1e-13 to 6e-13 both -- and both lie below the floor n u max|H_0|, so the floor is what the ratio is taken against.)
C_SWEEP = 0.5 is the next power of two above twice the largest ratio (the prefix-tree pivots and the blocked order change the rounding by a small
factor); it may not exceed 16: a larger ratio is a finding to explain, not a tolerance to set.

H is well conditioned by construction (Q diagonally dominant; asserted: cond(H) <= 1e6), m = n + 40, A has about four entries per row and, on purpose,
a row whose only entry is in the last column, rows whose first entry is in column 0, 31, 32 and n - 1, a row of 37 entries, an empty row and rows of
1, 15, 16, 17, 63, 64 and 65 entries (lengths and columns clipped to n where n is smaller).
"""
import numpy as np
import pytest

from qpalm_amd.problems import QP, _csc
from qpalm_amd.solver import QpalmBatch
from tests import exact_refs as xr

C_SWEEP = 0.5
INF = 1e20                     # the reference's QPALM_INFTY
SPECIAL_LENGTHS = (1, 15, 16, 17, 63, 64, 65)
ST = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, scaling=0)


def test_longdouble_has_a_64_bit_mantissa():
    """what every longdouble reference of this module rests on"""
    assert xr.has_extended_precision()


# ------------------------------------------------------------------------------------------------------------------ problems
def edge_qp(n, m, seed):
    """(QP, special): the QP of the module docstring; special = row numbers of A by name.  Deterministic in (n, m, seed)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    specs = [("last_only", [n - 1])]
    for c in (0, 31, 32, n - 1):
        c = min(c, n - 1)
        rest = rng.choice(np.arange(c + 1, n), size=min(2, n - 1 - c), replace=False) if c + 1 < n else []
        specs.append(("first_%d" % c, [c] + [int(v) for v in rest]))
    specs.append(("len_37", sorted(int(v) for v in rng.choice(n, size=min(37, n), replace=False))))
    specs.append(("empty", []))
    for ln in SPECIAL_LENGTHS:
        specs.append(("len_%d" % ln, sorted(int(v) for v in rng.choice(n, size=min(ln, n), replace=False))))
    specs = specs[:m]
    where = rng.permutation(m)[:len(specs)]
    special, rows = {}, [None] * m
    for (name, cols), i in zip(specs, where):
        special.setdefault(name, int(i))
        rows[int(i)] = list(cols)
    normal = [i for i in range(m) if rows[i] is None]
    for i in normal:
        k = int(min(n, max(1, rng.binomial(8, 0.5))))
        rows[i] = sorted(int(v) for v in rng.choice(n, size=k, replace=False))
    # two pairs of identical rows with identical, wide bounds: exactly equal breakpoints in the line search
    dups = []
    if len(normal) >= 8:
        for a, b in ((normal[1], normal[-2]), (normal[3], normal[-4])):
            rows[b] = list(rows[a])
            dups.append((a, b))
    ar, ac, av = [], [], []
    vals = {}
    for i in range(m):
        v = rng.standard_normal(len(rows[i]))
        v = np.where(np.abs(v) < 0.05, 0.05, v)
        vals[i] = v
    for a, b in dups:
        vals[b] = vals[a].copy()
    for i in range(m):
        ar += [i] * len(rows[i]); ac += rows[i]; av += list(vals[i])
    import scipy.sparse as sp
    A = sp.csc_matrix((av, (ar, ac)), shape=(m, n))
    # Q: sparse symmetric, an "arrow" in the last row (long rows for the SpMV), diagonally dominant
    M = sp.random(n, n, density=min(1.0, 2.0 / n), format="csc", random_state=rng, data_rvs=rng.standard_normal)
    S = sp.lil_matrix((M + M.T) * 0.5)
    for j in rng.choice(n, size=min(40, n), replace=False):
        if j != n - 1:
            S[n - 1, j] = S[j, n - 1] = 0.1 * rng.standard_normal()
    S = sp.csc_matrix(S)
    S.setdiag(0.0)
    S.eliminate_zeros()
    Qf = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsc()
    q = rng.standard_normal(n)
    bmin, bmax = -rng.random(m), rng.random(m)
    third = np.arange(m) % 3 == 0                     # about a third of the rows are bounded on one side only
    bmin[third & (np.arange(m) % 2 == 0)] = -INF
    bmax[third & (np.arange(m) % 2 == 1)] = INF
    for a, b in dups:
        bmin[a] = bmin[b] = -5.0
        bmax[a] = bmax[b] = 5.0
    Qp, Qi, Qx = _csc(sp.tril(Qf))
    Ap, Ai, Ax = _csc(A)
    special["dups"] = dups
    special["normal"] = [i for i in normal if all(i != b for _, b in dups)]
    return QP(n, m, Qp, Qi, Qx, Ap, Ai, Ax, q, bmin, bmax), special


class Case:
    """one row of the shape table: backend, small_workgroups, n, the workgroup size the batch must report"""

    def __init__(self, kind, sw, n, threads, m=None):
        self.kind, self.sw, self.n, self.threads, self.m = kind, sw, n, threads, (n + 40 if m is None else m)

    @property
    def id(self):
        return "%s-t%d-n%d" % (self.kind, self.threads, self.n) + ("" if self.m == self.n + 40 else "-m%d" % self.m)

    def param(self, *extra, suffix=""):
        return pytest.param(self.kind, self, *extra, id=self.id + suffix, marks=[pytest.mark.gpu] if self.kind == "hip" else [])


TABLE = ([Case("hip", 0, n, 512) for n in (31, 32, 33, 64, 65, 511, 512, 513, 1024, 1025, 2048, 2049)] +
         [Case("hip", 1, 255, 256), Case("hip", 1, 256, 256), Case("hip", 1, 257, 512)] +
         [Case("hip", 2, n, 128) for n in (127, 128, 129, 191, 192, 193, 256)] +       # (n = 256, m = 296 fits the 128-thread instance's LDS: it takes it)
         [Case("emu", 1, n, 128) for n in (31, 32, 33, 127, 128, 129, 256, 257, 512, 513)])
SWEEP32 = [Case("hip", 0, n, 512) for n in (65, 513, 1025)] + [Case("emu", 1, n, 128) for n in (65, 129, 257)]
NARROW = [Case("hip", 0, n, 512) for n in (33, 65)] + [Case("emu", 1, n, 128) for n in (33, 65)]


def _spmv_cases():
    out = list(TABLE)
    for kind, T in (("hip", 512), ("emu", 128)):
        for v in (1, 63, 64, 65, T - 1, T, T + 1, 4 * T + 1):
            out.append(Case(kind, 0 if kind == "hip" else 1, v, T, m=v))
    return out


LS_M = (63, 64, 65, 127, 128, 129, 1024, 1025)


def _ls_case(kind, m):
    return Case(kind, 0 if kind == "hip" else 1, m - 40 if m < 1000 else 200, 512 if kind == "hip" else 128, m=m)


def cases(lst):
    return pytest.mark.parametrize("ctx,case", [c.param() for c in lst], indirect=["ctx"])


class Opened:
    """the common set-up: one QP, scaling = 0, begin_solve, iterate(2); the batch is closed and every context option restored on exit.
    options: context options for the batch, e.g. sweep_ranks, linesearch_hbm, narrow_rows, and coop / coop_updates / coop_workgroups / coop_graphs
    (tests/test_coop_ops_exact.py: the same operations on the grid kernels)"""

    def __init__(self, ctx, case, seed=None, **options):
        self.ctx, self.case, self.options = ctx, case, options
        self.p, self.special = edge_qp(case.n, case.m, 7000 + case.n if seed is None else seed)
        self.bt = None

    def __enter__(self):
        ctx, case = self.ctx, self.case
        assert ctx.kind == case.kind
        ctx.set_option("small_workgroups", case.sw)
        for k, v in self.options.items():
            ctx.set_option(k, v)
        self.bt = bt = QpalmBatch(ctx, [self.p], ctx.default_settings(**ST))
        assert bt.launch_shape()[1] == case.threads, (bt.launch_shape(), case.id)     # a silently different instance fails here
        bt.begin_solve()
        bt.iterate(2)                                  # sigma and A' sqrt(Sigma) are set up by the first iterations
        self.sigma, self.gamma = bt.vec("sigma")[:case.m], float(bt.stats(0).gamma)
        assert np.all(np.isfinite(self.sigma)) and np.all(self.sigma > 0) and self.gamma > 0
        p = self.p
        self.Arows = xr.csc_to_rows(p.m, p.n, p.Ap, p.Ai, p.Ax)
        self.Qrows = xr.sym_rows_from_lower(p.n, p.Qp, p.Qi, p.Qx)
        return self

    def __exit__(self, *exc):
        try:
            if self.bt is not None:
                self.bt.close()
        finally:
            ctx = self.ctx
            ctx.set_option("small_workgroups", 1)
            ctx.set_option("sweep_ranks", 16)
            ctx.set_option("linesearch_hbm", 0)
            ctx.set_option("narrow_rows", 1)
            ctx.set_option("coop", 0)
            ctx.set_option("coop_updates", 2)
            ctx.set_option("coop_graphs", 1)
            ctx.set_option("coop_workgroups", 3 if ctx.kind == "emu" else 256)     # what the ctx fixture sets (tests/conftest.py)
        return False

    # -- the sets of rows the tests use ---------------------------------------------------------------------------------------
    def special_rows(self):
        return [v for k, v in self.special.items() if k not in ("dups", "normal")]

    def base_active(self):
        """every second ordinary row"""
        return self.special["normal"][::2]

    def entering(self, count):
        """the special rows first, then ordinary rows that are not in base_active"""
        rows = self.special_rows() + self.special["normal"][1::2]
        assert len(rows) >= count
        return rows[:count]

    def H(self, rows_in, absolute=False):
        return xr.schur_matrix(self.Qrows, self.Arows, self.sigma, rows_in, self.gamma, absolute=absolute)

    def set_active(self, rows_in):
        act = np.zeros(self.case.m, dtype=np.int64)
        act[np.asarray(rows_in, dtype=np.int64)] = 1
        self.bt.set_ivec("active", act)

    def factor_of(self, rows_in, op="ldlcholQAtsigmaA"):
        self.set_active(rows_in)
        self.bt.op(op)
        return self.bt.factor(0)

    def update_vectors(self, rows):
        """sqrt(sigma_i) a_i as dense fp64 vectors"""
        W = np.zeros((len(rows), self.case.n))
        for k, i in enumerate(rows):
            for j, v in self.Arows[int(i)]:
                W[k, j] = np.sqrt(self.sigma[int(i)]) * v
        return W


def check_conditioning(H):
    ev = np.linalg.eigvalsh(np.asarray(H, dtype=np.float64))
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e6, (ev[0], ev[-1])


def worst_ratio(err, bound):
    """max err / bound over the entries; an entry whose bound is 0 (a structural zero) must be exactly 0: inf otherwise"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if np.any((bound == 0) & (err != 0)) or not np.all(np.isfinite(err)):
        return float("inf")
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if np.any(nz) else 0.0


def sample_columns(n, seed):
    """None (= all columns) up to n = 1025; above, the columns around the first two, the last two and the last block edges plus 16 seeded ones"""
    if n <= 1025:
        return None
    fixed = [0, 31, 32, 33, 63, 64, n - 33, n - 32, n - 1]
    rnd = np.random.default_rng(seed).choice(n, size=16, replace=False)
    return np.unique(np.array(fixed + [int(v) for v in rnd], dtype=np.int64))


def product_error(L, D, H, cols):
    """L D L' - H on the sampled columns, longdouble"""
    Lu = xr.unit_lower(L)
    return xr.ldl_product(Lu, D, cols) - (H if cols is None else H[:, cols])


# ------------------------------------------------------------------------------------------------------------------ 1. factor
def _check_factor(o, rows_in=None, op="ldlcholQAtsigmaA"):
    """rows_in = None: every second ordinary row and every special row; op = "ldlchol" factorises Q + I / gamma alone (rows_in = [])"""
    n = o.case.n
    if rows_in is None:
        rows_in = o.base_active() + o.special_rows()
    L, D = o.factor_of(rows_in, op)
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(D))
    H = o.H(rows_in)
    check_conditioning(H)
    cols = sample_columns(n, 11)
    R = np.abs(product_error(L, D, H, cols))
    Habs = o.H(rows_in, absolute=True)
    r = xr.longest_column(o.Arows, rows_in, n)
    Lu = xr.unit_lower(L)
    bound = xr.gamma_k(n + 1) * xr.ldl_abs_product(Lu, D, cols) + xr.gamma_k(r + 2) * np.asarray(Habs if cols is None else Habs[:, cols], dtype=np.float64)
    ratio = worst_ratio(R, bound)
    print("factor %s: max |R| / bound = %.3g, r = %d" % (o.case.id, ratio, r))
    assert ratio <= 1.0, (o.case.id, ratio)
    return L, D


@cases(TABLE)
def test_factor(ctx, case):
    with Opened(ctx, case) as o:
        _check_factor(o)


@pytest.mark.parametrize("narrow", [0, 1])
@cases(NARROW)
def test_factor_narrow_rows(ctx, case, narrow):
    """form_schur_narrow (a quarter wavefront per column; rows of more than 16 entries take its chunk loop) and form_schur on the same matrices"""
    with Opened(ctx, case, narrow_rows=narrow) as o:
        _check_factor(o)


# ------------------------------------------------------------------------------------------------------------------ 2. update / downdate
def _run_updown(o, start_rows, change_rows, sign):
    """(L0, D0, L, D, new rows): the factor of `start_rows`, and after `change_rows` have entered (sign = +1) or left (-1) it"""
    bt = o.bt
    L0, D0 = o.factor_of(start_rows)
    if sign > 0:
        bt.set_ivec("enter", change_rows); bt.set_scalar("nb_enter", len(change_rows)); bt.set_scalar("nb_leave", 0)
        bt.op("ldlupdate_entering_constraints")
        new_rows = list(start_rows) + list(change_rows)
    else:
        bt.set_ivec("leave", change_rows); bt.set_scalar("nb_leave", len(change_rows)); bt.set_scalar("nb_enter", 0)
        bt.op("ldldowndate_leaving_constraints")
        new_rows = [i for i in start_rows if i not in set(change_rows)]
    L, D = bt.factor(0)
    return L0, D0, L, D, new_rows


def _updown_errors(o, L0, D0, L, D, H0, Hn, vectors, sign):
    """(kernel's error, reference's error, floor n u max|H_0|) of a factor (L, D) meant to be that of Hn = H0 + sign sum w w' over the rows w of
    `vectors`, reached from the factor (L0, D0) of H0: the reference applies the same vectors to (L0, D0) one rank at a time in fp64"""
    n = o.case.n
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(D))
    check_conditioning(H0)
    check_conditioning(Hn)
    Lr, Dr = xr.sequential_updown(L0, D0, vectors, sign)
    cols = sample_columns(n, 13)
    e_k = float(np.max(np.abs(product_error(L, D, Hn, cols))))
    e_r = float(np.max(np.abs(product_error(Lr, Dr, Hn, cols))))
    floor = n * xr.U * float(np.max(np.abs(H0)))
    return e_k, e_r, floor


def _updown(o, start_rows, change_rows, sign):
    """(kernel's error, reference's error, floor n u max|H_0|, L, D): `change_rows` enter (sign = +1) or leave (-1) the factor of `start_rows`"""
    L0, D0, L, D, new_rows = _run_updown(o, start_rows, change_rows, sign)
    e_k, e_r, floor = _updown_errors(o, L0, D0, L, D, o.H(start_rows), o.H(new_rows), o.update_vectors(change_rows), sign)
    return e_k, e_r, floor, L, D


def _judge(o, what, e_k, e_r, floor):
    ratio = e_k / max(e_r, floor)
    print("%s %s: kernel %.3g, sequential fp64 reference %.3g, n u max|H0| %.3g, ratio %.3g" % (what, o.case.id, e_k, e_r, floor, ratio))
    assert ratio <= C_SWEEP, (what, o.case.id, e_k, e_r, floor)


@cases(TABLE)
def test_update_17_rows_enter(ctx, case):
    """one sweep of 16 ranks and one of one; the entering rows include every special row of A"""
    with Opened(ctx, case) as o:
        enter = o.entering(17)
        assert set(o.special_rows()) <= set(enter)
        e_k, e_r, floor, _, _ = _updown(o, o.base_active(), enter, +1)
        _judge(o, "update", e_k, e_r, floor)


@cases(TABLE)
def test_downdate_33_rows_leave(ctx, case):
    """two sweeps of 16 ranks and one of one; the leaving rows include every special row of A"""
    with Opened(ctx, case) as o:
        start = o.base_active() + o.entering(17)
        leave = o.special_rows() + o.base_active()
        leave = leave[:33]
        assert len(leave) == 33 and set(leave) <= set(start)
        e_k, e_r, floor, _, _ = _updown(o, start, leave, -1)
        _judge(o, "downdate", e_k, e_r, floor)


@cases(SWEEP32)
def test_update_33_rows_enter_32_ranks(ctx, case):
    """the 32-rank form of the sweep (16-column blocks): same bound, and bit-identical to the 16-rank form (tests/test_sweep32.py states that for solves)"""
    out = {}
    for ranks in (16, 32):
        with Opened(ctx, case, sweep_ranks=ranks) as o:
            enter = o.entering(33)
            e_k, e_r, floor, L, D = _updown(o, o.base_active(), enter, +1)
            _judge(o, "update, sweep_ranks = %d" % ranks, e_k, e_r, floor)
            out[ranks] = (L, D)
    assert np.array_equal(out[16][0], out[32][0]) and np.array_equal(out[16][1], out[32][1])


# ------------------------------------------------------------------------------------------------------------------ 3. solve
class SolveJudge:
    """|L D L' d + dphi| <= 3 gamma_n |L||D||L'||d| for the factor (L, D) as read back"""

    def __init__(self, case, L, D):
        self.case = case
        Lu = xr.unit_lower(L)
        self.Ll, self.Dl = np.asarray(Lu, dtype=xr.LD), np.asarray(D, dtype=xr.LD)
        self.La, self.Da = np.abs(Lu), np.abs(D)

    def check(self, d, rhs, name):
        n, Ll, Dl, La, Da = self.case.n, self.Ll, self.Dl, self.La, self.Da
        assert np.all(np.isfinite(d))
        dl = np.asarray(d, dtype=xr.LD)
        res = np.abs(Ll @ (Dl * (Ll.T @ dl)) + np.asarray(rhs, dtype=xr.LD))
        bound = 3 * xr.gamma_k(n) * (La @ (Da * (La.T @ np.abs(d))))
        ratio = worst_ratio(res, bound)
        print("solve %s, rhs %s: max residual / bound = %.3g" % (self.case.id, name, ratio))
        assert ratio <= 1.0, (self.case.id, name, ratio)


def solve_rhs(n):
    ends = np.zeros(n); ends[0] += 1.0; ends[n - 1] += 1.0
    return (("random", np.random.default_rng(500 + n).standard_normal(n)), ("e_0 + e_{n-1}", ends))


@cases(TABLE)
def test_solve(ctx, case):
    with Opened(ctx, case) as o:
        n, bt = case.n, o.bt
        L, D = o.factor_of(o.base_active() + o.special_rows())
        judge = SolveJudge(case, L, D)
        for name, rhs in solve_rhs(n):
            bt.set_vec("dphi", rhs)
            bt.op("ldlsolveLD_neg_dphi")
            judge.check(bt.vec("d"), rhs, name)


# ------------------------------------------------------------------------------------------------------------------ 4. SpMV
def _spmv_x(k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, size=k)
    x[::7] = 0.0
    if k > 1:
        x[-1] = -3.5
    return x


@cases(_spmv_cases())
def test_spmv(ctx, case):
    """mat_vec / mat_tpose_vec of Q and A against exact rational arithmetic on the fp64 data"""
    ctx.set_option("small_workgroups", case.sw)
    bt = None
    try:
        p, special = edge_qp(case.n, case.m, 7100 + case.n)
        bt = QpalmBatch(ctx, [p], ctx.default_settings(**ST))
        assert bt.launch_shape()[1] == case.threads, (bt.launch_shape(), case.id)
        Arows = xr.csc_to_rows(p.m, p.n, p.Ap, p.Ai, p.Ax)
        Acols = [[(int(p.Ai[k]), float(p.Ax[k])) for k in range(int(p.Ap[j]), int(p.Ap[j + 1]))] for j in range(p.n)]
        Qrows = xr.sym_rows_from_lower(p.n, p.Qp, p.Qi, p.Qx)
        xn, xm = _spmv_x(p.n, 1), _spmv_x(p.m, 2)
        for name, rows, got in (("A x", Arows, bt.mat_vec("A", xn)), ("A' y", Acols, bt.mat_tpose_vec("A", xm)),
                                ("Q x", Qrows, bt.mat_vec("Q", xn)), ("Q' x", Qrows, bt.mat_tpose_vec("Q", xn))):
            y, bnd = xr.spmv_fraction(rows, xn if name != "A' y" else xm)
            assert len(got) == len(rows)
            worst = 0.0
            for i, (yi, bi, gi, r) in enumerate(zip(y, bnd, got, rows)):
                assert np.isfinite(gi)
                if not r:
                    assert gi == 0.0, (case.id, name, i)
                    continue
                err = abs(xr.Fraction(float(gi)) - yi)
                assert err <= bi, (case.id, name, i, len(r), float(err), float(bi))
                if bi > 0:
                    worst = max(worst, float(err / bi))
            print("spmv %s %s: max error / bound = %.3g" % (case.id, name, worst))
        if "empty" in special:
            assert bt.mat_vec("A", xn)[special["empty"]] == 0.0
    finally:
        if bt is not None:
            bt.close()
        ctx.set_option("small_workgroups", 1)


# ------------------------------------------------------------------------------------------------------------------ 5. line search
def _judge_tau(o, what):
    """run exact_linesearch on the state of the batch and judge tau by the exact derivative of the piecewise quadratic there"""
    bt, m = o.bt, o.case.m
    tau = bt.exact_linesearch()
    d, Qd, df, delta, alpha = bt.vec("d"), bt.vec("Qd"), bt.vec("df"), bt.vec("delta"), bt.vec("alpha")
    assert np.isfinite(tau) and tau > 0
    val, mag, nact = xr.linesearch_derivative(tau, d, Qd, df, delta, alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        keys = alpha / delta
    pos = np.sort(keys[keys > 0])
    crossed = int(np.sum(pos < tau))
    equal_pairs = int(np.sum(pos[1:] == pos[:-1]))
    ratio = float(abs(val) / (2 * m * xr.Fraction(xr.U) * mag))
    print("linesearch %s m = %d, %s: tau = %.17g, %d of %d positive breakpoints crossed, %d active terms, %d equal pairs, |psi'| / bound = %.3g"
          % (o.case.id, m, what, tau, crossed, len(pos), nact, equal_pairs, ratio))
    assert equal_pairs >= 2
    assert ratio <= 1.0, (o.case.id, what, tau, float(val), float(mag))
    return tau, pos, crossed


def _linesearch(o):
    """(tau, tau): exact_linesearch along the Newton direction of the EMPTY active set, then along the same direction with df replaced by a multiple of
    d chosen so that psi' changes sign near the median positive breakpoint: the crossing lies deep inside the sorted buffer, past its first tiles"""
    bt, m = o.bt, o.case.m
    assert int(np.sum((o.p.bmin <= -INF) | (o.p.bmax >= INF))) >= m // 4
    bt.op("compute_residuals")
    o.set_active([])
    bt.op("ldlcholQAtsigmaA")
    bt.op("ldlsolveLD_neg_dphi")
    tau1, pos, _ = _judge_tau(o, "Newton direction")
    d, Qd, delta, alpha = bt.vec("d"), bt.vec("Qd"), bt.vec("delta"), bt.vec("alpha")
    t = float(pos[len(pos) // 2])
    g = t * float(d @ Qd) + float(np.sum(delta * np.maximum(delta * t - alpha, 0.0)))
    assert g > 0
    bt.set_vec("df", -g / float(d @ d) * d)
    tau2, pos, crossed = _judge_tau(o, "crossing at the median breakpoint")
    assert crossed >= len(pos) // 4, (crossed, len(pos))
    return tau1, tau2


@pytest.mark.parametrize("ctx,case", [_ls_case(k, m).param() for k in ("emu", "hip") for m in LS_M], indirect=["ctx"])
def test_linesearch(ctx, case):
    with Opened(ctx, case, seed=7200 + case.m) as o:
        _linesearch(o)


@pytest.mark.parametrize("ctx,case", [_ls_case(k, m).param() for k in ("emu", "hip") for m in (65, 129)], indirect=["ctx"])
def test_linesearch_sort_in_hbm(ctx, case):
    """the sort buffer in HBM with LDS tiles (linesearch_hbm = 1) and with tiles of 32 entries (= 32): same network, tau bit-identical"""
    taus = {}
    for hbm in (0, 1, 32):
        with Opened(ctx, case, seed=7200 + case.m, linesearch_hbm=hbm) as o:
            taus[hbm] = _linesearch(o)
    assert taus[1] == taus[0] and taus[32] == taus[0], taus

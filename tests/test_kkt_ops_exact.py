"""Single operations of the DENSE KKT path (qpalm_amd/csrc/qpalm_kkt.h, reached through kkt_newton<RPT>: kkt_form, kkt_factorize, kkt_solve,
kkt_update_entering_constraints, kkt_update_leaving_constraints of include/qpalm_gfx950.h, and the solver's own compact refactorisation
kkt_form_compact + dense_factor + kkt_expand with the solve on the compact factor) against high-precision references (tests/exact_refs.py: numpy
longdouble, plain fp64 recurrences; no oracle, no kernel), in the style of tests/test_ops_exact.py, at the sizes where the kernels change form.
Sizes are rows of the factor, np = n + m, split n = ceil(0.4 np), m = np - n (m >= 67), or n = 5, m = 70 (p = n + k smaller than one unrolled round
of the row addition's mat-vec: 32 / 16 / 8 columns on 512 / 256 / 128 threads):
  512 threads   np = 75 (n = 5), 511, 512, 513, 1024, 1025, 2048, 2049      (rpt = ceil(np / threads): k_op<1|2|4>, 2049: dense_updown_big)
  256 threads   np = 255, 256; 257 reports 512
  128 threads   np = 75 (n = 5), 127, 128, 129, 191, 192, 193, 256           (every one of them lands on the 128-thread instance)
  emulator      np = 75 (n = 5), 127, 128, 129, 256, 257, 512, 513           (128 threads; 513: the large-factor form)
Every case asserts the workgroup size the batch reports.  scaling = 0, factorization_method = 0, one QP per batch.  Parts 1 to 3 write DISTINCT
sigma_inv values (seeded, two decades) after two solver iterations: the solver's own are all equal then and an index mix-up would not show.

Bounds (gamma_k = k u / (1 - k u), u = 2^-53; valid for any elimination order and for FMA, no conditioning assumption):
  form     the lower triangle of the slot equals K assembled in fp64 on the host BIT FOR BIT (the only rounding is Q_jj + 1 / gamma)
  factor   |L D L' - K|              <= gamma_{np+1} |L||D||L'| + 2 u |K|      (entry by entry; an inactive row: d = 1.0, row and column exactly 0)
  solve    |L D L' sol - [-dphi; 0]| <= 3 gamma_np |L||D||L'||sol|            (L, D as read back: dense_solve alone is judged; sol[:n] == d bit for bit)
Above np = 300 the products are taken on sampled columns (test_ops_exact.sample_columns' recipe, plus the columns next to n and to the row changed).
Largest measured ratios of the two bounds over the table (the compact path's cases among them):
  factor   MI355X 0.0521 (np = 129, 128 threads)    emulator 0.0521 (np = 129)
  solve    MI355X 0.00669 (np = 110, compact factor)   emulator 0.00897 (np = 129, compact factor)
A row addition / deletion has no such constant.  Its error e_k = max|L D L' - K_new| is compared with e_r, that of the sequential fp64 recurrence
(exact_refs.kkt_row_add / kkt_row_del) applied to the SAME starting factor, one row per call, each step starting from the factor the previous one left:
  e_k <= C_ROW_DENSE max(e_r, np u max|K_old|)
Rows are scripted by POSITION: k = 0 (p = n), m-1 (no trailing block, the sweep is skipped), m-2, m-64, m-65, m-66 (63, 64, 65 trailing rows: the 64-row
blocks of the mat-vec), the first k with (n + k) % 32 = 31, 0, 1 (p + 1 on and beside a 32-column block edge of the forward solve and the sweep) and
30 (p + 1 the last column of its block; row p + 1 is present by then, so that column has work to do), and by content: the empty row, len_65, last_only,
first_0.  All of them enter, every second one leaves, one of those enters again (state 2 -> 1).  The row after each scripted row is present from the
start.  Above np = 300 the script has six steps (k = 0, the rows at 31 and 30, m-1; the row at 30 leaves and enters again), at 2048 / 2049 three
(host time).  Largest measured ratios e_k / max(e_r, np u max|K_old|):
  single rows        MI355X 0.172 (np = 193, 128 threads, an addition)           emulator 0.157 (np = 128, an addition)
  multi-row calls    MI355X 0.278 (np = 193, 128 threads, three rows enter)      emulator 0.109 (np = 128, three rows enter)
(The kernel's error is between 0.7 and 1.9 times the reference's at every step -- 1e-15 to 4e-14 both: mostly the error the starting factor already
has -- and both lie below the floor np u max|K_old|, so the floor is what the ratio is taken against.)
C_ROW_DENSE = 1.0: the next power of two above twice the largest ratio (0.556), as C_SWEEP of tests/test_ops_exact.py and C_ROW of tests/test_sparse_ops_exact.py;
it may not exceed 16: a larger ratio is a finding to explain, not a tolerance to set.
After any step the columns j < p outside row p and d[:p] are bit-identical to before; after a deletion row and column p are exactly 0 and d_p = 1.0.

An EMPTY constraint row: kkt_form / kkt_factorize (and the compact form) give it a unit pivot, a row addition gives it -sigma_inv[k] exactly (the
reference's own behaviour, see tests/test_sparse_ops_exact.py); from its addition on K carries -sigma_inv[k] there.

The compact path runs only inside the solver's refactorisation, so it is driven through the bounds: with x = y = 0 a row is active iff bmin > 0 or
bmax < 0; rows of the chosen set get [0.5, 1.5], the others [-1, 1], and iterate(1) is called until n_refactor = 1 (asserted, with n_rank1 = 0 and
active == the chosen set).  kkt_solve then runs on the compact factor (gather / scatter through kkt_list); reading the factor spreads it out
(kkt_expand), and the same bounds judge both.  The two layouts' solutions need not be bit-equal.  On the 512-thread instance two shapes straddle
QP_NW (n + m) 8 + 4 m <= lds_bytes: the larger one takes the full (n + m) form.
"""
import numpy as np
import pytest

from qpalm_amd.solver import QpalmBatch
from tests import exact_refs as xr
from tests.test_ops_exact import Case, cases, edge_qp, product_error, sample_columns, worst_ratio

C_ROW_DENSE = 1.0
ST = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, scaling=0, factorization_method=0)
FULL_PRODUCTS = 300            # rows of the factor up to which L D L' is taken on every column and the whole script runs
WANTED = ("empty", "len_65", "last_only", "first_0")


def kcase(kind, sw, rows, threads, n=None):
    """the case of a factor of `rows` rows: n = ceil(0.4 rows) unless given"""
    n = (2 * rows + 4) // 5 if n is None else n
    return Case(kind, sw, n, threads, m=rows - n)


TABLE = ([kcase("hip", 0, 75, 512, n=5)] + [kcase("hip", 0, r, 512) for r in (511, 512, 513, 1024, 1025, 2048, 2049)] +
         [kcase("hip", 1, 255, 256), kcase("hip", 1, 256, 256), kcase("hip", 1, 257, 512)] +
         [kcase("hip", 2, 75, 128, n=5)] + [kcase("hip", 2, r, 128) for r in (127, 128, 129, 191, 192, 193, 256)] +
         [kcase("emu", 1, 75, 128, n=5)] + [kcase("emu", 1, r, 128) for r in (127, 128, 129, 256, 257, 512, 513)])
SMALL = [c for c in TABLE if c.n + c.m <= FULL_PRODUCTS]


def test_longdouble_has_a_64_bit_mantissa():
    assert xr.has_extended_precision()


# ------------------------------------------------------------------------------------------------------------------ K and the script's bookkeeping
class KBook:
    """K of a state, no kernel: the longdouble matrix with every row present is built once (exact_refs.kkt_matrix), a state then turns the rows that are
    not present (state 0: never there, 2: deleted) into unit rows.  `minus`: the empty rows that a row ADDITION gave -sigma_inv (form + factorise
    leave them unit rows)."""

    def __init__(self, Qrows, Arows, sigma_inv, gamma):
        self.Qrows, self.Arows, self.n, self.m = Qrows, Arows, len(Qrows), len(Arows)
        self.sigma_inv, self.gamma = np.array(sigma_inv, dtype=np.float64), float(gamma)
        self.K_all = xr.kkt_matrix(Qrows, Arows, self.sigma_inv, self.gamma, np.ones(self.m, dtype=np.int64))
        self.state, self.minus = np.zeros(self.m, dtype=np.int64), set()

    def start(self, rows_in):
        self.state[:] = 0
        self.state[np.asarray(rows_in, dtype=np.int64)] = 1
        self.minus = set()

    def apply(self, what, k):
        """the bookkeeping of one row operation"""
        assert self.state[k] != 1 if what == "enter" else self.state[k] == 1, (what, k, self.state[k])
        self.state[k] = 1 if what == "enter" else 2
        if not self.Arows[k]:
            (self.minus.add if what == "enter" else self.minus.discard)(k)

    def K(self):
        n = self.n
        K = self.K_all.copy()
        unit = n + np.nonzero(self.state != 1)[0]
        K[unit, :] = 0
        K[:, unit] = 0
        K[unit, unit] = 1
        for k in self.minus:
            K[n + k, n + k] = -xr.LD(self.sigma_inv[k])
        return K

    def K_fp64(self):
        """the matrix as kkt_form assembles it in fp64: Q_jj + 1 / gamma is a rounded quotient and a rounded sum, everything else is copied"""
        n, m = self.n, self.m
        K = np.zeros((n + m, n + m))
        K[:n, :n] = xr.dense_from_rows(self.Qrows, n, dtype=np.float64)
        K[np.arange(n), np.arange(n)] += 1.0 / self.gamma
        for k in range(m):
            p = n + k
            if self.state[k] == 1 and self.Arows[k]:
                for j, v in self.Arows[k]:
                    K[p, j] = K[j, p] = v
                K[p, p] = -self.sigma_inv[k]
            else:
                K[p, p] = 1.0
        return K

    def column(self, k):
        """(the off-diagonal part of column n + k of K when the row is present, its diagonal entry as a row addition writes it)"""
        kcol = np.zeros(self.n + self.m)
        for j, v in self.Arows[k]:
            kcol[j] = v
        return kcol, -float(self.sigma_inv[k])

    def reference(self, L0, D0, steps):
        """the fp64 factor after `steps` ((what, k), in order) by the sequential recurrences, from the factor (L0, D0)"""
        L, D = np.asfortranarray(xr.unit_lower(L0)), np.array(D0, dtype=np.float64)
        for what, k in steps:
            if what == "enter":
                xr.kkt_row_add(L, D, self.n + k, *self.column(k))
            else:
                xr.kkt_row_del(L, D, self.n + k)
        return L, D


def script_rows(n, m, special):
    """the scripted constraints (module docstring), by position and by content, without repeats"""
    edge = [next(k for k in range(m) if (n + k) % 32 == r) for r in (31, 0, 1, 30)]      # (30: p + 2 on the edge, entering when row p + 1 is present)
    rows = [0, m - 1, m - 2, m - 64, m - 65, m - 66] + edge + [special[w] for w in WANTED]
    assert all(0 <= k < m for k in rows)
    return list(dict.fromkeys(int(k) for k in rows))


def script(n, m, special):
    """[(what, k)]: every scripted row enters, every second one leaves, one of those enters again; above FULL_PRODUCTS rows six steps, from 2048 three"""
    rows = script_rows(n, m, special)
    if n + m >= 2048:
        return [("enter", 0), ("enter", m - 2), ("leave", 0)]
    if n + m > FULL_PRODUCTS:
        e31, e30 = (next(k for k in range(m) if (n + k) % 32 == r) for r in (31, 30))
        assert len({0, e31, e30, m - 1}) == 4
        return [("enter", 0), ("enter", e31), ("enter", e30), ("enter", m - 1), ("leave", e30), ("enter", e30)]
    left = rows[::2]
    return [("enter", k) for k in rows] + [("leave", k) for k in left] + [("enter", left[len(left) // 2])]


def columns(rows, seed, extra=()):
    """None (= every column) up to FULL_PRODUCTS rows; above, sample_columns' recipe (the columns around the first two, the last two and the last block
    edges, 16 seeded ones) plus `extra`"""
    if rows <= FULL_PRODUCTS:
        return None
    cols = sample_columns(rows, seed)
    if cols is None:
        fixed = [0, 31, 32, 33, 63, 64, rows - 33, rows - 32, rows - 1]
        cols = np.array(fixed + [int(v) for v in np.random.default_rng(seed).choice(rows, size=16, replace=False)], dtype=np.int64)
    cols = np.concatenate([cols, np.asarray([c for c in extra if 0 <= c < rows], dtype=np.int64)])
    return np.unique(cols)


def factor_ratio(L, D, K, cols):
    """max over the sampled entries of |L D L' - K| / (gamma_{np+1} |L||D||L'| + 2 u |K|)"""
    rows = L.shape[0]
    R = np.abs(product_error(L, D, K, cols))
    Kc = K if cols is None else K[:, cols]
    bound = xr.gamma_k(rows + 1) * xr.ldl_abs_product(xr.unit_lower(L), D, cols) + 2 * xr.U * np.abs(Kc).astype(np.float64)
    return worst_ratio(R, bound)


def solve_ratio(L, D, sol, dphi):
    """max |L D L' sol - [-dphi; 0]| / (3 gamma_np |L||D||L'||sol|) with the factor as read back"""
    rows = L.shape[0]
    Lu = xr.unit_lower(L)
    Ll, Dl, La, Da = np.asarray(Lu, dtype=xr.LD), np.asarray(D, dtype=xr.LD), np.abs(Lu), np.abs(D)
    b = np.zeros(rows, dtype=xr.LD)
    b[:len(dphi)] = -np.asarray(dphi, dtype=xr.LD)
    res = np.abs(Ll @ (Dl * (Ll.T @ np.asarray(sol, dtype=xr.LD))) - b)
    bound = 3 * xr.gamma_k(rows) * (La @ (Da * (La.T @ np.abs(sol))))
    return worst_ratio(res, bound)


def unit_rows_are_exact(L, D, n, state):
    """an absent constraint: d = 1.0, its row and its column of L exactly 0"""
    idx = n + np.nonzero(np.asarray(state) != 1)[0]
    Ls = np.tril(L, -1)
    return bool(np.all(D[idx] == 1.0) and not np.any(Ls[idx, :]) and not np.any(Ls[:, idx]))


def test_row_recurrences_and_bookkeeping_on_a_small_matrix():
    """no kernel: KBook's matrices and the script's bookkeeping against exact_refs.kkt_row_add / kkt_row_del on a dense L D L' computed here -- after every
    step of a script (an empty row among its rows) L D L' = K of the book's state within 16 np u max|K|"""
    rng = np.random.default_rng(3)
    n, m = 6, 9
    M = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.4)
    Q = np.tril(M + M.T, -1)
    Q = Q + Q.T + np.diag(np.abs(Q + Q.T).sum(axis=1) + 1.0)
    Qrows = [[(j, float(Q[i, j])) for j in range(n) if Q[i, j] != 0.0] for i in range(n)]
    Arows = [[(int(j), float(rng.standard_normal())) for j in sorted(rng.choice(n, size=int(rng.integers(1, 4)), replace=False))] for _ in range(m)]
    Arows[4] = []
    book = KBook(Qrows, Arows, 10.0 ** rng.uniform(-2, 0, m), 1e3)
    rows = n + m

    def ldl(K):
        L, D = np.eye(rows), np.zeros(rows)
        for j in range(rows):
            D[j] = K[j, j] - (L[j, :j] ** 2) @ D[:j]
            for i in range(j + 1, rows):
                L[i, j] = (K[i, j] - (L[i, :j] * L[j, :j]) @ D[:j]) / D[j]
        return L, D
    book.start([1, 3, 8])
    K64 = book.K_fp64()
    assert float(np.max(np.abs(K64 - book.K()))) <= 2 * xr.U * float(np.max(np.abs(K64))) and np.array_equal(K64, K64.T)
    book.start([1, 3, 4, 8])                                     # the empty row present from the start: a unit row
    assert book.K()[n + 4, n + 4] == 1.0 and book.K_fp64()[n + 4, n + 4] == 1.0
    book.start([1, 3, 8])
    L, D = ldl(K64)
    steps = [("enter", 0), ("enter", 4), ("enter", 7), ("leave", 3), ("leave", 4), ("enter", 3), ("enter", 4), ("leave", 0)]
    for what, k in steps:
        L, D = book.reference(L, D, [(what, k)])
        book.apply(what, k)
        K = book.K()
        tol = 16 * rows * xr.U * float(np.max(np.abs(K)))
        assert float(np.max(np.abs(xr.ldl_product(L, D) - K))) <= tol, (what, k)
        if what == "leave":
            assert D[n + k] == 1.0 and not np.any(L[n + k, :n + k]) and not np.any(L[n + k + 1:, n + k])
    assert list(book.state) == [2, 1, 0, 1, 1, 0, 0, 1, 1] and book.minus == {4} and book.K()[n + 4, n + 4] == -xr.LD(book.sigma_inv[4])
    # the script: every row once, positions in range, the three lengths
    for nn, mm in ((5, 70), (51, 76), (206, 307), (820, 1229)):
        special = dict(empty=3, len_65=9, last_only=11, first_0=mm - 1)
        rws, sc = script_rows(nn, mm, special), script(nn, mm, special)
        assert len(set(rws)) == len(rws) and {0, mm - 1, mm - 2, mm - 64, mm - 65, mm - 66, 3, 9, 11} <= set(rws)
        assert {31, 0, 1, 30} <= {(nn + k) % 32 for k in rws}
        assert len(sc) == (len(rws) + (len(rws) + 1) // 2 + 1 if nn + mm <= FULL_PRODUCTS else 6 if nn + mm < 2048 else 3)
        bk = KBook([[(0, 1.0)]], [[(0, 1.0)]] * mm, np.ones(mm), 1.0)
        for what, k in sc:
            bk.apply(what, k)                                  # (asserts that an entering row is absent and a leaving one present)


# ------------------------------------------------------------------------------------------------------------------ the batch
class Opened:
    """one QP (test_ops_exact.edge_qp) in KKT mode on the case's instance; `chosen`: the rows that the bounds make active at x = y = 0 (the compact
    path's driver); the batch is closed and every context option restored on exit"""

    def __init__(self, ctx, case, chosen=None, **options):
        self.ctx, self.case, self.options, self.bt = ctx, case, options, None
        self.n, self.m, self.rows = case.n, case.m, case.n + case.m
        self.p, self.special = edge_qp(case.n, case.m, 8000 + self.rows)
        if chosen is not None:
            on = np.zeros(case.m, dtype=bool)
            on[np.asarray(chosen, dtype=np.int64)] = True
            self.p.bmin, self.p.bmax = np.where(on, 0.5, -1.0), np.where(on, 1.5, 1.0)

    def __enter__(self):
        ctx, case, p = self.ctx, self.case, self.p
        assert ctx.kind == case.kind
        ctx.set_option("small_workgroups", case.sw)
        for k, v in self.options.items():
            ctx.set_option(k, v)
        st = ctx.default_settings(**ST)
        assert int(st.proximal) == 1
        self.bt = bt = QpalmBatch(ctx, [p], st)
        self.shape = bt.launch_shape()
        assert self.shape[1] == case.threads, (self.shape, case.id)          # a silently different instance fails here
        self.Arows = xr.csc_to_rows(p.m, p.n, p.Ap, p.Ai, p.Ax)
        self.Qrows = xr.sym_rows_from_lower(p.n, p.Qp, p.Qi, p.Qx)
        for w in WANTED:
            assert w in self.special
        assert not self.Arows[self.special["empty"]] and len(self.Arows[self.special["len_65"]]) == min(65, p.n)
        bt.begin_solve()
        return self

    def __exit__(self, *exc):
        try:
            if self.bt is not None:
                self.bt.close()
        finally:
            self.ctx.set_option("small_workgroups", 1)
            self.ctx.set_option("kkt_compact", 1)
        return False

    def distinct_penalties(self):
        """two solver iterations, then seeded sigma_inv values spread over two decades; the book of this state"""
        bt, m = self.bt, self.m
        bt.iterate(2)
        sigma_inv = 0.05 * 10.0 ** np.random.default_rng(90 + self.rows).uniform(-1.0, 1.0, m)
        assert len(np.unique(sigma_inv)) == m
        bt.set_vec("sigma_inv", sigma_inv)
        assert np.array_equal(bt.vec("sigma_inv")[:m], sigma_inv)
        self.book = KBook(self.Qrows, self.Arows, sigma_inv, float(bt.stats(0).gamma))
        assert self.book.gamma > 0
        return self.book

    def base_rows(self, without=()):
        """every second row and the special rows, without the rows listed but with the row after each of them (row p + 1 is then present when row p
        changes: the first column of the trailing sweep has work to do)"""
        rows = set(range(0, self.m, 2)) | {self.special[w] for w in WANTED} | {k + 1 for k in without if k + 1 < self.m}
        return [k for k in sorted(rows) if k not in set(without)]

    def form_and_factor(self, rows_in):
        act = np.zeros(self.m, dtype=np.int64)
        act[np.asarray(rows_in, dtype=np.int64)] = 1
        self.bt.set_ivec("active", act)
        self.book.start(rows_in)
        self.bt.op("kkt_form")
        self.bt.op("kkt_factorize")
        return self.factor()

    def factor(self):
        L, D = self.bt.factor_rows(self.rows)
        assert np.all(np.isfinite(L)) and np.all(np.isfinite(D))
        return L, D

    def state(self):
        return self.bt.ivec("kkt_state")[:self.m]

    def slot(self):
        """the factor slot as it stands, [i, j] = entry (i, j) of the column-major panel"""
        ld = self.bt.device_ptr("L")[1] // (8 * self.rows)
        assert ld >= self.rows
        return self.bt.named_vec("L", ld * self.rows).reshape(self.rows, ld).T[:self.rows]

    def solve(self, dphi):
        """kkt_solve with the factor the slot holds: (sol, d)"""
        self.bt.set_vec("dphi", dphi)
        self.bt.op("kkt_solve")
        sol, d = self.bt.named_vec("sol_kkt", self.rows), self.bt.vec("d")
        assert np.all(np.isfinite(sol)) and np.array_equal(sol[:self.n], d)
        return sol

    def right_hand_sides(self):
        n = self.n
        ends = np.zeros(n); ends[0] += 1.0; ends[n - 1] += 1.0
        return (("random", np.random.default_rng(500 + self.rows).standard_normal(n)), ("e_0 + e_{n-1}", ends))


# ------------------------------------------------------------------------------------------------------------------ 1. form and factorise
@cases(TABLE)
def test_form_and_factor(ctx, case):
    with Opened(ctx, case) as o:
        bt, n, m, rows = o.bt, o.n, o.m, o.rows
        book = o.distinct_penalties()
        rows_in = o.base_rows()
        act = np.zeros(m, dtype=np.int64); act[rows_in] = 1
        bt.set_ivec("active", act)
        book.start(rows_in)
        bt.op("kkt_form")
        assert np.array_equal(o.state(), act) and np.array_equal(bt.ivec("active")[:m], act)
        K64 = book.K_fp64()
        formed = np.tril(o.slot())
        assert np.array_equal(formed, np.tril(K64)), (case.id, float(np.max(np.abs(formed - np.tril(K64)))))
        pe = n + o.special["empty"]
        assert act[o.special["empty"]] == 1 and formed[pe, pe] == 1.0 and not np.any(formed[pe, :pe]) and not np.any(formed[pe + 1:, pe])
        bt.op("kkt_factorize")
        L, D = o.factor()
        K = book.K()
        cols = columns(rows, 11, extra=(n - 1, n, n + 1, pe))
        ratio = factor_ratio(L, D, K, cols)
        print("KKT factor %s: %d of %d rows present, max |R| / bound = %.3g" % (case.id, len(rows_in) - 1, m, ratio))
        assert ratio <= 1.0, (case.id, ratio)
        state = act.copy(); state[o.special["empty"]] = 0              # (the empty row is a unit row too)
        assert unit_rows_are_exact(L, D, n, state), case.id


# ------------------------------------------------------------------------------------------------------------------ 2. solve on the full factor
@cases(TABLE)
def test_solve(ctx, case):
    with Opened(ctx, case) as o:
        o.distinct_penalties()
        L, D = o.form_and_factor(o.base_rows())
        for name, rhs in o.right_hand_sides():
            sol = o.solve(rhs)
            ratio = solve_ratio(L, D, sol, rhs)
            print("KKT solve %s, rhs %s: max residual / bound = %.3g" % (case.id, name, ratio))
            assert ratio <= 1.0, (case.id, name, ratio)


# ------------------------------------------------------------------------------------------------------------------ 3. row additions and deletions
OPS = dict(enter="kkt_update_entering_constraints", leave="kkt_update_leaving_constraints")


def _set_lists(o, enter=(), leave=()):
    """the lists and BOTH counts of the two boundary operations (each operation reads its own)"""
    bt = o.bt
    bt.set_ivec("enter", list(enter)); bt.set_scalar("nb_enter", len(enter))
    bt.set_ivec("leave", list(leave)); bt.set_scalar("nb_leave", len(leave))


def _judge_steps(o, what, L0, D0, steps, seed, tag):
    """the kernel's factor after `steps` (already applied on the device; all of one kind) against the sequential recurrence from (L0, D0): criterion (a),
    the exact properties (c), the empty row (b); returns (L, D, ratio)"""
    n, rows, book = o.n, o.rows, o.book
    K0 = book.K()
    Lr, Dr = book.reference(L0, D0, steps)
    for w, k in steps:
        book.apply(w, k)
    L1, D1 = o.factor()
    assert np.array_equal(o.state(), book.state), (tag, steps)
    Kn = book.K()
    ps = [n + k for _, k in steps]
    cols = columns(rows, seed, extra=[c for p in ps for c in (p - 1, p, p + 1, p + 2, (p + 1) // 32 * 32 - 1, (p + 1) // 32 * 32, (p + 1) // 32 * 32 + 32)])
    e_k = float(np.max(np.abs(product_error(L1, D1, Kn, cols))))
    e_r = float(np.max(np.abs(product_error(Lr, Dr, Kn, cols))))
    floor = rows * xr.U * float(np.max(np.abs(K0)))
    ratio = e_k / max(e_r, floor)
    print("KKT row %s %s: %s rows %s (p = %s of %d), kernel %.3g, reference %.3g, floor %.3g, ratio %.3g"
          % (tag, o.case.id, what, [k for _, k in steps], ps, rows, e_k, e_r, floor, ratio))
    # (c) nothing in front of the first changed row moves: columns j < p outside the changed rows, and d[:p]
    p0 = min(ps)
    keep = np.ones(rows, dtype=bool); keep[ps] = False
    assert np.array_equal(L1[keep][:, :p0], L0[keep][:, :p0]) and np.array_equal(D1[:p0], D0[:p0]), (tag, steps, "an entry in front of row p was written")
    for w, k in steps:
        p = n + k
        if w == "leave":
            assert D1[p] == 1.0 and not np.any(L1[p, :p]) and not np.any(L1[p + 1:, p]), (tag, w, k, "row / column p after a deletion")
        elif not o.Arows[k]:
            assert D1[p] == -book.sigma_inv[k] and Dr[p] == -book.sigma_inv[k], (tag, w, k, "the empty row's pivot")        # (b)
    assert ratio <= C_ROW_DENSE, (tag, o.case.id, steps, e_k, e_r, floor)
    return L1, D1, ratio


@cases(TABLE)
def test_row_operations(ctx, case):
    with Opened(ctx, case) as o:
        bt, n, m = o.bt, o.n, o.m
        o.distinct_penalties()
        steps = script(n, m, o.special)
        first_enter = {k for w, k in steps if w == "enter"}
        L, D = o.form_and_factor(o.base_rows(without=first_enter))
        worst = 0.0
        for i, (what, k) in enumerate(steps):
            _set_lists(o, **{what: [k]})
            bt.op(OPS[what])
            L, D, ratio = _judge_steps(o, what, L, D, [(what, k)], 13 + i, "step %d" % i)
            worst = max(worst, ratio)
        assert o.special["empty"] in first_enter or n + m > FULL_PRODUCTS
        for name, rhs in o.right_hand_sides()[:1]:                              # (e) the solve on the factor as it stands
            ratio = solve_ratio(L, D, o.solve(rhs), rhs)
            print("KKT solve after the row operations %s: max residual / bound = %.3g; largest row-operation ratio %.3g" % (case.id, ratio, worst))
            assert ratio <= 1.0, (case.id, ratio)


@cases(SMALL)
def test_multi_row_calls(ctx, case):
    """three rows enter in one call (not in ascending order); then nb_enter = 2 and nb_leave = 2 are both set and each operation is called once"""
    with Opened(ctx, case) as o:
        bt, m = o.bt, o.m
        o.distinct_penalties()
        three, two_in, two_out = [m - 3, 1, m // 2], [2, m - 4], [m // 2, m - 3]
        L, D = o.form_and_factor(o.base_rows(without=three + two_in))
        _set_lists(o, enter=three)
        bt.op("kkt_update_entering_constraints")
        L, D, _ = _judge_steps(o, "enter", L, D, [("enter", k) for k in three], 31, "three in one call")
        _set_lists(o, enter=two_in, leave=two_out)
        bt.op("kkt_update_entering_constraints")
        L, D, _ = _judge_steps(o, "enter", L, D, [("enter", k) for k in two_in], 32, "two of two and two, entering")
        bt.op("kkt_update_leaving_constraints")
        L, D, _ = _judge_steps(o, "leave", L, D, [("leave", k) for k in two_out], 33, "two of two and two, leaving")
        rhs = o.right_hand_sides()[0][1]
        assert solve_ratio(L, D, o.solve(rhs), rhs) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ 4. the compact path
def spread(m, count):
    """`count` rows spread evenly over 0 .. m-1"""
    return [(i * m) // count for i in range(count)]


def chosen_set(what, n, m):
    return {"none": [], "first": [0], "last": [m - 1], "all": list(range(m)), "rows64": spread(m, 64 - n), "rows65": spread(m, 65 - n),
            "second": list(range(0, m, 2)), "second1": list(range(1, m, 2))}[what]


def _compact_cases():
    out = []
    for kind, sw, T in (("emu", 1, 128), ("hip", 0, 512)):
        small = Case(kind, sw, 40, T, m=70)
        out += [small.param(w, suffix="-" + w) for w in ("none", "first", "last", "all", "rows64", "rows65")]
        out.append(Case(kind, sw, 5, T, m=70).param("first", suffix="-first"))
    out += [kcase("hip", 0, 513, 512).param("second", suffix="-second"), kcase("hip", 1, 256, 256).param("second", suffix="-second"),
            kcase("hip", 2, 192, 128).param("second", suffix="-second"), kcase("emu", 1, 129, 128).param("second", suffix="-second")]
    return out


def drive_refactor(o, chosen=None):
    """iterate until the solver has refactorised once more (at most three iterations), without a rank-1 update on the way; returns (active, book)"""
    bt = o.bt
    s0 = bt.stats(0)
    for _ in range(3):
        bt.iterate(1)
        if int(bt.stats(0).n_refactor) > int(s0.n_refactor):
            break
    s = bt.stats(0)
    assert int(s.n_refactor) == int(s0.n_refactor) + 1 and int(s.n_rank1) == int(s0.n_rank1), (s.n_refactor, s.n_rank1)
    act = bt.ivec("active")[:o.m]
    if chosen is not None:
        want = np.zeros(o.m, dtype=np.int64); want[np.asarray(chosen, dtype=np.int64)] = 1
        assert np.array_equal(act, want), (np.nonzero(act)[0], chosen)
    assert np.array_equal(o.state(), act)
    o.book = KBook(o.Qrows, o.Arows, bt.vec("sigma_inv")[:o.m], float(s.gamma))
    o.book.start(np.nonzero(act)[0])
    return act, o.book


def check_compact(o, act, tag):
    """the solve on the compact factor, then the factor read back (spread out), then the solve on the full layout"""
    n, rows, book = o.n, o.rows, o.book
    rhs = np.random.default_rng(600 + rows).standard_normal(n)
    sol_c = o.solve(rhs)                                          # before the factor is read: the compact solve
    L, D = o.factor()
    K = book.K()
    pe = n + o.special["empty"]
    ratio = factor_ratio(L, D, K, columns(rows, 17, extra=(n - 1, n, n + 1, pe, rows - 2)))
    print("KKT compact factor %s: %d active rows, max |R| / bound = %.3g" % (tag, int(act.sum()), ratio))
    assert ratio <= 1.0, (tag, ratio)
    state = act.copy(); state[o.special["empty"]] = 0
    assert unit_rows_are_exact(L, D, n, state), tag
    r_c = solve_ratio(L, D, sol_c, rhs)
    assert np.all(sol_c[n:][act == 0] == 0.0), (tag, "an inactive row's solution is not 0")
    sol_f = o.solve(rhs)
    r_f = solve_ratio(L, D, sol_f, rhs)
    print("KKT compact solve %s: max residual / bound = %.3g on the compact factor, %.3g on the full layout; max difference %.3g"
          % (tag, r_c, r_f, float(np.max(np.abs(sol_c - sol_f)))))
    assert r_c <= 1.0 and r_f <= 1.0, (tag, r_c, r_f)
    return L, D


@pytest.mark.parametrize("ctx,case,what", _compact_cases(), indirect=["ctx"])
def test_compact_refactorisation(ctx, case, what):
    chosen = chosen_set(what, case.n, case.m)
    with Opened(ctx, case, chosen=chosen) as o:
        assert what not in ("rows64", "rows65") or case.n + len(chosen) == int(what[4:])
        assert what != "all" or o.special["empty"] in chosen
        assert 8 * (case.threads // 64) * o.rows + 4 * o.m <= o.shape[2]                # the staging fits: the compact form runs
        act, _ = drive_refactor(o, chosen)
        check_compact(o, act, case.id + "-" + what)


@pytest.mark.parametrize("ctx,case", [Case("emu", 1, 40, 128, m=70).param(), Case("hip", 0, 40, 512, m=70).param(), kcase("hip", 2, 192, 128).param()],
                         indirect=["ctx"])
def test_compact_refactorisation_with_distinct_penalties(ctx, case):
    """the solver's own penalties differ from row to row after a few iterations; a refactorisation forced then (reset_newton) forms the compact matrix
    with two or more distinct sigma_inv among its active rows"""
    with Opened(ctx, case) as o:
        bt, m = o.bt, o.m
        drive_refactor(o)
        for it in range(40):
            bt.iterate(1)
            act, sinv = bt.ivec("active")[:m], bt.vec("sigma_inv")[:m]
            present = [k for k in np.nonzero(act)[0] if o.Arows[k]]
            if len(np.unique(sinv[present])) >= 2 and bt.num_unfinished() == 1:
                break
        assert bt.num_unfinished() == 1, "the solve ended before the penalties differed"
        bt.set_scalar("reset_newton", 1)
        act, book = drive_refactor(o)
        present = [k for k in np.nonzero(act)[0] if o.Arows[k]]
        assert len(np.unique(book.sigma_inv[present])) >= 2, "sigma_inv has one value among the active rows: a wrong index would not show"
        assert 0 < len(present) < m
        print("distinct penalties %s: %d iterations, %d active rows, %d values of sigma_inv among them" % (case.id, it + 1, len(present), len(np.unique(book.sigma_inv[present]))))
        check_compact(o, act, case.id + "-distinct")


@pytest.mark.parametrize("ctx,case", [Case("emu", 1, 40, 128, m=70).param(), Case("hip", 0, 40, 512, m=70).param(), kcase("hip", 1, 256, 256).param(),
                                      kcase("hip", 2, 192, 128).param()], indirect=["ctx"])
def test_expansion_inside_a_row_operation(ctx, case):
    """a row addition on a compact factor spreads it out first: the same factor, bit for bit, as when a read spread it out before"""
    chosen = chosen_set("second", case.n, case.m)
    out = []
    for read_first in (True, False):
        with Opened(ctx, case, chosen=chosen) as o:
            drive_refactor(o, chosen)
            k = next(k for k in range(1, case.m, 2) if o.Arows[k])
            if read_first:
                o.factor()
            _set_lists(o, enter=[k])
            o.bt.op("kkt_update_entering_constraints")
            out.append(o.factor())
            assert o.state()[k] == 1 and out[-1][1][case.n + k] < 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("ctx", [pytest.param("hip", marks=pytest.mark.gpu, id="hip")], indirect=True)
def test_lds_fallback_to_the_full_form(ctx):
    """512 threads: the staging of kkt_expand needs 8 (n + m) 8 + 4 m bytes of LDS; the last shape that fits refactorises compactly, four rows more
    take the full (n + m) form.  Both give the factor of K."""
    m, nw = 200, 8
    with Opened(ctx, Case("hip", 0, 40, 512, m=70)) as o:
        lds = o.shape[2]                                         # the 512-thread instance's LDS
    sides = []
    for more in (0, 4):
        n = (lds - 4 * m) // (8 * nw) - m - 3 + more
        case = Case("hip", 0, n, 512, m=m)
        chosen = chosen_set("second", n, m)
        with Opened(ctx, case, chosen=chosen) as o:
            assert o.shape[2] == lds, o.shape
            fits = 8 * nw * o.rows + 4 * m <= o.shape[2]
            sides.append((fits, o.shape[2], n))
            act, book = drive_refactor(o, chosen)
            L, D = o.factor()
            ratio = factor_ratio(L, D, book.K(), columns(o.rows, 19, extra=(n - 1, n, n + 1, o.rows - 2)))
            print("KKT factor through the solver, n = %d, m = %d, LDS %d bytes, %s form: max |R| / bound = %.3g" % (n, m, o.shape[2], "compact" if fits else "full", ratio))
            assert ratio <= 1.0, (n, m, ratio)
            state = act.copy(); state[o.special["empty"]] = 0
            assert unit_rows_are_exact(L, D, n, state)
    assert [s[0] for s in sides] == [True, False], sides

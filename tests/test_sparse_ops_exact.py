"""Single operations on the SPARSE factors (qpalm_amd/csrc/qpalm_sparse.h: sp_factor, sp_solve, sp_updown / sp_path_walk; qpalm_sparse_kkt.h: spk_rows,
sp_factor<true>) against high-precision references (tests/exact_refs.py; no oracle, no kernel), through the factor itself, read back in compressed
columns (QpalmBatch.sparse_factor), on matrices whose gadgets sit on the edges of the kernels' forms (tests/sparse_gadgets.py; g = the lanes of a
column's group, spg = 64 / sparse_gpw = 8, 16, 32 or 64):
  column form (LDS iff the longest column of the wavefront has at most min(2 spg, LDS share) accumulators)   cliques of g-1 .. 2g+1 variables
  rows of A / contributing columns longer than a group (the a_over / l_over tail loops)                     the same cliques
  more rows of A or contributing columns through a column than a group has lanes (the pb / rb reloads),
    counts 1, 3, 4, 5 against the batches of four, a whole round of inactive rows                            stars of 1 .. 2g+1 leaves, hub last
  level width against the groups of a workgroup (the cw += gtot stride), runs of one-column levels           w pairs + a chain of six
  solves: rows / columns modulo four, level width against the workgroup, right-hand side in LDS iff 8 n <= 77824
  path walks: columns and rows of A of more than 64 entries, a root-only row, an empty row
  every index under a nested dissection (sparse_ordering = 1; a band is added in front, 90 columns on the GPU and 48 on the emulator: the gadgets alone
    are left in natural order, the band's separators go behind them and renumber every gadget's columns -- asserted)
Every case asserts the workgroup size (512 on the MI355X, 128 on the emulator), that sigma takes at least two values among the rows used, and,
under the natural ordering, the level widths it claims (exact_refs.etree_levels of the read-back pattern).  In the gadget matrices w is chosen so
that level 0 holds a multiple of the workgroup's groups plus ONE column (65 columns on the emulator, 705 on the GPU: 1 modulo 64, 32, 16 and 8);
the "levels" cases hold w pairs and the chain only, w + 1 = groups - 1, groups, groups + 1, 2 groups + 1 and workgroup size + 1.

Bounds (gamma_k = k u / (1 - k u), u = 2^-53; t = the longest row of L's pattern, r = the longest column of A_a; valid for any order and for FMA):
  factor   |L D L' - P H P'|         <= gamma_{t+2} |L||D||L'| + gamma_{r+2} (|Q| + |A_a|' Sigma |A_a| + I / gamma), entry by entry, over the WHOLE
                                        matrix (by connected component of the pattern); an entry of H outside the pattern fails
  solve    |L D L' (P d) + P b|      <= 3 gamma_{t+1} |L||D||L'||P d|          (L, D as read back: the solve alone is judged)
  K        |L D L' - P K P'|         <= gamma_{t+2} |L||D||L'| + 2 u |diag(K)|   (K from the batch's own A_values, Q_values, sigma_inv, gamma, kkt_state)
  kkt_solve  the same residual bound as the solve's on K sol = [-dphi; 0], WITHOUT refinement (qpg_kkt_solve is one solve with the factor)
Largest measured ratio of each bound over the cases of the table (the few-term bounds of the "levels" cases, t = r = 1, are the tight ones; on the
gadget matrices the factor's and the solve's ratios are 0.03 and below):
  factor     MI355X 0.885 (levels, w + 1 = 513)    emulator 0.548 (levels, w + 1 = 129)
  solve      MI355X 0.286 (levels, w + 1 = 63)     emulator 0.242 (levels, w + 1 = 129)
  K          MI355X 0.00753 (natural order)        emulator 0.0126 (natural order)
  kkt_solve  MI355X 0.00151                        emulator 0.00337
The path updates and the KKT row operations have no such constant.  Their error max|L D L' - (new matrix)| is compared with that of the plain sequential
fp64 recurrences of exact_refs (rank-1 changes one after the other by rank1_updown; kkt_row_add / kkt_row_del) on the dense expansion of the same
starting factor:
  err_kernel <= C max(err_ref, nf u max|H_0|)          (nf = rows of the factor, H_0 = the matrix before the change)
Largest measured ratios err_kernel / max(err_ref, nf u max|H_0|):
  rows enter             MI355X 0.00542 (gpw 8, natural)      emulator 0.0125 (gpw 8 and 1, natural)
  rows leave             MI355X 0.00229 (gpw 8, dissection)   emulator 0.0116 (dissection)
  sigma changed          MI355X 0.00396 (gpw 8, natural)      emulator 0.235 (dissection: kernel 3.3e-12, reference 1.3e-12, floor 1.4e-11)
  KKT row operations     MI355X 0.0157 (natural, the budget row)   emulator 0.0165 (natural, the budget row)
(The kernel's error is at most 3 times the reference's in the path updates and at most 7 times in the row operations -- the budget row's pivot
d22 = -1 / sigma - sum z_j^2 / d_j is one lane's running sum of 1107 terms, numpy's dot sums pairwise -- and both lie below the floor
nf u max|H_0| in every case, so the floor is what the ratio is taken against.)
C_PATH = 0.5 (from 0.235) and C_ROW = 0.0625 (from 0.0165): the next power of two above twice the largest ratio, as C_SWEEP of tests/test_ops_exact.py;
neither may exceed 16: a larger ratio is a finding to explain, not a tolerance to set.
The path updates also leave the pattern (Lp, Li) as it was and every column off the changed rows' elimination-tree paths bit-identical; a row operation
leaves everything outside row p, column p and the path from parent(p) bit-identical, and a deletion leaves row and column p exactly 0 and d_p = 1.

An EMPTY constraint row in KKT mode: qpg_kkt_form / qpg_kkt_factorize give it a unit pivot, a row addition gives it -1 / sigma.  That is the reference's
own behaviour (src/solver_interface.c: qpalm_form_kkt sets the diagonal of a constraint without entries to 1, kkt_update_entering_constraints hands
ladel_row_add -sigma_inv unconditionally), the column is decoupled from everything else and the x part of a solve does not depend on it: pinned here
as it is (test_kkt_row_operations, the last step; test_kkt_factor).
"""
import numpy as np
import pytest

from qpalm_amd.solver import QpalmBatch
from tests import exact_refs as xr
from tests.sparse_gadgets import block_sizes, blocks_qp, gadget_qp
from tests.test_ops_exact import worst_ratio

C_PATH = 0.5
C_ROW = 0.0625
ST = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0, scaling=0)
THREADS = dict(hip=512, emu=128)
LDS_BYTES = 77824
BAND = dict(hip=90, emu=48)     # columns of the band that ordering 1 gets: the gadgets alone come back in natural order (48: what the emulator's time allows)
MAX_ITER = 12


class Case:
    """one row of the table: backend, matrix ("gadget": g-list + w; "levels": w; "blocks": n), sparse_gpw, sparse_ordering, sparse_lds, KKT mode"""

    def __init__(self, kind, shape, gpw=8, ordering=0, lds=1, glist=(), w=0, n=0, kkt=False):
        self.kind, self.shape, self.gpw, self.ordering, self.lds, self.glist, self.w, self.n, self.kkt = kind, shape, gpw, ordering, lds, tuple(glist), w, n, kkt
        self.threads = THREADS[kind]
        self.ngrp = (self.threads // 64) * gpw

    @property
    def id(self):
        what = {"gadget": "g" + "_".join(str(g) for g in self.glist), "levels": "levels%d" % (self.w + 1), "blocks": "blocks%d" % self.n}[self.shape]
        return "%s-%s-gpw%d-ord%d%s" % (self.kind, what, self.gpw, self.ordering, "" if self.lds == 1 else "-lds%d" % self.lds)

    def param(self):
        return pytest.param(self.kind, self, id=self.id, marks=[pytest.mark.gpu] if self.kind == "hip" else [])


G_HIP, W_HIP, W_EMU = (8, 16, 32, 64), 24, 4
GADGET = ([Case("emu", "gadget", gpw, o, glist=(8,), w=W_EMU) for gpw in (8, 1) for o in (0, 1)] +
          [Case("hip", "gadget", gpw, o, glist=G_HIP, w=W_HIP) for gpw in (8, 4, 2, 1) for o in (0, 1)] +
          [Case("hip", "gadget", 8, 0, lds=0, glist=G_HIP, w=W_HIP)])
LEVELS = ([Case("emu", "levels", 8, w=16), Case("emu", "levels", 1, w=2), Case("emu", "levels", 8, w=128)] +
          [Case("hip", "levels", 8, w=wp1 - 1) for wp1 in (63, 64, 65, 129, 513)])
BLOCKS = [Case("hip", "blocks", 8, n=n) for n in (LDS_BYTES // 8, LDS_BYTES // 8 + 1)]
KKT = ([Case("emu", "gadget", 8, o, glist=(8,), w=W_EMU, kkt=True) for o in (0, -1)] +
       [Case("hip", "gadget", 8, o, glist=(8, 64), w=W_HIP, kkt=True) for o in (0, -1)])


def cases(lst):
    return pytest.mark.parametrize("ctx,case", [c.param() for c in lst], indirect=["ctx"])


class Factor:
    """the factor as read back, with what the checks derive from its pattern"""

    def __init__(self, bt, nf):
        self.nf = nf
        self.Lp, self.Li, self.Lx, self.D = bt.sparse_factor(0)
        assert len(self.D) == nf and self.Lp[nf] == len(self.Li) == len(self.Lx) == bt.sparse_info(0)[0]
        assert np.all(np.isfinite(self.Lx)) and np.all(np.isfinite(self.D))
        self.col = np.repeat(np.arange(nf), np.diff(self.Lp))          # column of every entry
        self.parent = xr.etree_parent(self.Lp, self.Li, nf)
        self.comps = xr.etree_components(self.Lp, self.Li, nf)
        self.comp_of = np.zeros(nf, dtype=np.int64)
        for c, cols in enumerate(self.comps):
            self.comp_of[cols] = c
        self.t = int(np.bincount(self.Li, minlength=nf).max()) if len(self.Li) else 0      # the longest row of the pattern

    def same_pattern(self, other):
        return np.array_equal(self.Lp, other.Lp) and np.array_equal(self.Li, other.Li)

    def with_values(self, Lx, D):
        out = object.__new__(Factor)
        out.__dict__.update(self.__dict__)
        out.Lx, out.D = Lx, D
        return out

    def dense(self, c):
        return np.asfortranarray(xr.sparse_to_unit_lower(self.Lp, self.Li, self.Lx, self.nf, cols=self.comps[c])), self.D[self.comps[c]].copy()

    def from_dense(self, blocks):
        """this factor with the components of `blocks` ({component: (L, D) dense}) in place of its own; a dense entry outside the pattern must be 0"""
        Lx, D = self.Lx.copy(), self.D.copy()
        for c, (L, Dc) in blocks.items():
            cols = self.comps[c] if c is not None else np.arange(self.nf)      # (None: the whole matrix)
            local = np.full(self.nf, -1, dtype=np.int64)
            local[cols] = np.arange(len(cols))
            sel = np.nonzero(self.comp_of[self.col] == c)[0] if c is not None else np.arange(len(self.Li))
            Lx[sel] = L[local[self.Li[sel]], local[self.col[sel]]]
            assert np.count_nonzero(np.tril(L, -1)) <= len(sel)
            assert np.count_nonzero(Lx[sel]) == np.count_nonzero(np.tril(L, -1))
            D[cols] = Dc
        return self.with_values(Lx, D)

    def off_columns_identical(self, other, touched):
        """every column outside `touched` has the same values and pivot, bit for bit"""
        keep = np.ones(self.nf, dtype=bool)
        keep[np.asarray(sorted(touched), dtype=np.int64)] = False
        return bool(np.array_equal(self.D[keep], other.D[keep]) and np.array_equal(self.Lx[keep[self.col]], other.Lx[keep[self.col]]))


class Opened:
    """the common set-up: one QP on a sparse factor with the case's options, scaling = 0, begin_solve, then iterations until sigma has more than one value
    among the base active rows (at most MAX_ITER; every test asserts it on the rows it uses); the batch is closed and every context option restored on exit"""

    def __init__(self, ctx, case):
        self.ctx, self.case, self.bt = ctx, case, None
        band = BAND[case.kind] if (case.ordering == 1 and case.shape == "gadget") else 0
        if case.shape == "gadget":
            self.p, self.rows = gadget_qp(case.glist, 4000 + len(case.glist), case.w, band=band, budget=case.kkt)
        elif case.shape == "levels":
            self.p, self.rows = gadget_qp((), 4100 + case.w, case.w, cliques=False, stars=False, arrow=False, single=False)
        else:
            self.p, self.rows = blocks_qp(case.n, 4200)

    def __enter__(self):
        ctx, case, p = self.ctx, self.case, self.p
        assert ctx.kind == case.kind
        ctx.set_option("sparse_kkt" if case.kkt else "sparse_factor", 1)
        ctx.set_option("sparse_ordering", case.ordering)
        ctx.set_option("sparse_gpw", case.gpw)
        ctx.set_option("sparse_lds", case.lds)
        ctx.set_option("small_workgroups", 0 if case.kind == "hip" else 1)
        st = dict(ST, factorization_method=0) if case.kkt else ST
        self.bt = bt = QpalmBatch(ctx, [p], ctx.default_settings(**st))
        shape = bt.launch_shape()
        assert shape[1] == case.threads, (shape, case.id)                  # a silently different instance fails here
        assert case.kkt or shape[2] == LDS_BYTES, (shape, case.id)         # (the limit of the "LDS fit" cases)
        assert bt.sparse_info(0)[0] > 0
        self.nf = nf = p.n + p.m if case.kkt else p.n
        self.perm, self.nlev = bt.sparse_perm(0)
        assert np.array_equal(np.sort(self.perm), np.arange(nf))
        if case.ordering == 0:
            assert np.array_equal(self.perm, np.arange(nf))
        elif case.shape == "gadget":
            assert not np.array_equal(self.perm, np.arange(nf)), "the ordering left the matrix in natural order: nothing permuted is tested"
        self.iperm = np.empty_like(self.perm)
        self.iperm[self.perm] = np.arange(nf)
        bt.begin_solve()
        for self.iterations in range(1, MAX_ITER + 1):      # (with iterate(2) sigma is 20.0 in every row: a wrong sigma index would not show)
            bt.iterate(1)
            self.sigma = bt.vec("sigma")[:p.m]
            if len(np.unique(self.sigma[self.rows["active"]])) >= 2:
                break
        self.gamma = float(bt.stats(0).gamma)
        assert np.all(np.isfinite(self.sigma)) and np.all(self.sigma > 0) and self.gamma > 0
        self.Arows = xr.csc_to_rows(p.m, p.n, p.Ap, p.Ai, p.Ax)
        self.Qrows = xr.sym_rows_from_lower(p.n, p.Qp, p.Qi, p.Qx)
        if not case.kkt:      # the same rows in the factor's numbering
            ip = self.iperm
            self.ArowsP = [sorted((int(ip[j]), v) for j, v in r) for r in self.Arows]
            self.QrowsP = [sorted((int(ip[j]), v) for j, v in self.Qrows[int(self.perm[k])]) for k in range(p.n)]
            self.first = [r[0][0] if r else -1 for r in self.ArowsP]
        return self

    def __exit__(self, *exc):
        try:
            if self.bt is not None:
                self.bt.close()
        finally:
            ctx = self.ctx
            ctx.set_option("sparse_factor", -1)
            ctx.set_option("sparse_kkt", 0)
            ctx.set_option("sparse_ordering", -1)
            ctx.set_option("sparse_gpw", 0)
            ctx.set_option("sparse_lds", 1)
            ctx.set_option("small_workgroups", 1)
        return False

    # -- rows -------------------------------------------------------------------------------------------------------------------
    def distinct_sigma(self, rows):
        assert len(np.unique(self.sigma[np.asarray(rows, dtype=np.int64)])) >= 2, "sigma has one value among the rows used: a wrong sigma index would not show"

    def changing_rows(self):
        """the rows that enter / leave in the path tests: every clique row, the empty row, the root-only row, up to three rows of every star and four of the
        band; under a dissection the columns of these rows must have been renumbered (else Ati and AtiP could be mixed up unnoticed)"""
        r = self.rows
        out = [row for _, _, row in r["clique"]] + [x for x in (r["empty"], r["root_only"]) if x is not None] + r["band"][1:8:2]
        if self.case.ordering == 1:
            moved = [row for row in out if any(self.iperm[j] != j for j, _ in self.Arows[row])]
            assert len(moved) >= len(r["clique"]), "the ordering renumbered no column of the changing rows"
        for _, _, mine in r["star"]:
            out += mine[1:6:2][:3] if len(mine) > 1 else mine
        return out

    def set_active(self, rows_in):
        act = np.zeros(self.p.m, dtype=np.int64)
        act[np.asarray(rows_in, dtype=np.int64)] = 1
        self.bt.set_ivec("active", act)

    def factor_of(self, rows_in):
        self.set_active(rows_in)
        self.bt.op("ldlcholQAtsigmaA")
        return Factor(self.bt, self.nf)

    # -- P H P' by connected component of the factor's pattern ---------------------------------------------------------------------
    def rows_by_component(self, F, rows_in):
        out = [[] for _ in F.comps]
        for i in rows_in:
            if self.first[int(i)] >= 0:
                out[F.comp_of[self.first[int(i)]]].append(int(i))
        return out

    def H(self, F, c, rows_c, sigma=None, absolute=False):
        """the block of P H P' on component c (AssertionError where H couples the component to a column outside: the pattern lacks an entry)"""
        return xr.schur_matrix(self.QrowsP, self.ArowsP, self.sigma if sigma is None else sigma, rows_c, self.gamma, absolute=absolute, cols=F.comps[c])

    def product_error(self, F, rows_in, sigma=None):
        """(max |L D L' - P H P'|, max |P H P'|) over the whole matrix"""
        by = self.rows_by_component(F, rows_in)
        err, big = 0.0, 0.0
        for c in range(len(F.comps)):
            H = self.H(F, c, by[c], sigma)
            P = xr.sparse_ldl_product(F.Lp, F.Li, F.Lx, F.D, F.nf, cols=F.comps[c])
            err, big = max(err, float(np.max(np.abs(P - H)))), max(big, float(np.max(np.abs(H))))
        return err, big

    def max_abs_H(self, F, rows_in):
        by = self.rows_by_component(F, rows_in)
        return max(float(np.max(np.abs(self.H(F, c, by[c])))) for c in range(len(F.comps)))

    def update_vector(self, F, c, i, scale=None):
        """sqrt(sigma_i) a_i on component c, dense fp64, in the factor's numbering"""
        cols = F.comps[c]
        local = {int(v): k for k, v in enumerate(cols)}
        w = np.zeros(len(cols))
        s = np.sqrt(self.sigma[int(i)]) if scale is None else scale
        for j, v in self.ArowsP[int(i)]:
            w[local[j]] = s * v
        return w


def test_longdouble_has_a_64_bit_mantissa():
    assert xr.has_extended_precision()


def test_references_on_a_small_dense_matrix():
    """the references of this module against each other, no kernel: the compressed forms against the dense ones, and kkt_row_add / kkt_row_del against a
    dense L D L' of the bordered matrix"""
    rng = np.random.default_rng(1)
    n = 9
    M = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.35)
    K = M + M.T + np.diag(np.r_[6.0 * np.ones(6), -6.0 * np.ones(3)])

    def ldl(K):
        L, D = np.eye(n), np.zeros(n)
        for j in range(n):
            D[j] = K[j, j] - (L[j, :j] ** 2) @ D[:j]
            for i in range(j + 1, n):
                L[i, j] = (K[i, j] - (L[i, :j] * L[j, :j]) @ D[:j]) / D[j]
        return L, D
    L, D = ldl(K)
    Lp, Li, Lx = [0], [], []
    for j in range(n):
        for i in range(j + 1, n):
            Li.append(i); Lx.append(L[i, j])
        Lp.append(len(Li))
    Lp, Li, Lx = np.array(Lp), np.array(Li), np.array(Lx)
    assert np.array_equal(xr.sparse_to_unit_lower(Lp, Li, Lx, n), L)
    assert float(np.max(np.abs(xr.sparse_ldl_product(Lp, Li, Lx, D, n) - xr.ldl_product(L, D)))) <= 1e-18 * 40
    x = rng.standard_normal(n)
    assert float(np.max(np.abs(xr.sparse_ldl_apply(Lp, Li, Lx, D, x) - xr.ldl_product(L, D) @ x.astype(xr.LD)))) <= 1e-17 * 40
    assert list(xr.etree_levels(Lp, Li, n)) == [1] * n and xr.etree_path(xr.etree_parent(Lp, Li, n), 6) == [6, 7, 8]
    assert len(xr.etree_components(Lp, Li, n)) == 1
    for p in (7, 3):
        K0 = K.copy()
        K0[p, :] = 0.0; K0[:, p] = 0.0; K0[p, p] = 1.0
        L0, D0 = ldl(K0)
        La, Da = np.asfortranarray(L0.copy()), D0.copy()
        kcol = K[:, p].copy(); kcol[p] = 0.0
        xr.kkt_row_add(La, Da, p, kcol, K[p, p])
        assert np.max(np.abs((La * Da) @ La.T - K)) <= 1e-13
        xr.kkt_row_del(La, Da, p)
        assert np.max(np.abs((La * Da) @ La.T - K0)) <= 1e-13 and Da[p] == 1.0 and not np.any(La[p, :p]) and not np.any(La[p + 1:, p])


def test_read_back_of_a_batch_member_and_refusals(ctx):
    """QpalmBatch.sparse_factor: member 1 of a batch of two patterns of different sizes reads back what the same QP gives alone, bit for bit (the strides
    of the symbolic arrays are the batch's, of the values the slot's); dense batches and batches with more members than slots are refused"""
    from qpalm_amd.capi import QpgError
    small, _ = gadget_qp((), 1, 5, cliques=False, stars=False, arrow=False, single=False)
    big, rows = blocks_qp(43, 2)
    got = []
    ctx.set_option("sparse_factor", 1)
    ctx.set_option("sparse_ordering", 0)
    try:
        for probs, b in (([big], 0), ([small, big], 1)):
            bt = QpalmBatch(ctx, probs, ctx.default_settings(**ST))
            bt.begin_solve()
            bt.iterate(3)
            act = np.zeros(bt.m, dtype=np.int64); act[rows["active"]] = 1
            bt.set_ivec("active", act, b)
            bt.op("ldlcholQAtsigmaA", b)
            got.append(bt.sparse_factor(b))
            assert len(got[-1][3]) == big.n and len(got[-1][1]) == bt.sparse_info(b)[0]
            bt.close()
        for x, y in zip(*got):
            assert np.array_equal(x, y)
        assert np.all(np.isfinite(got[0][2])) and np.all(got[0][3] > 0) and len(xr.etree_components(got[0][0], got[0][1], big.n)) == len(block_sizes(big.n))
        ctx.set_option("max_slots", 2)
        bt = QpalmBatch(ctx, [small, big, small], ctx.default_settings(**ST))
        with pytest.raises(QpgError) as e:
            bt.sparse_factor(0)
        assert e.value.code == -5                       # QPG_ERR_UNSUPPORTED: a slot holds whichever QP ran last
        bt.close()
    finally:
        ctx.set_option("max_slots", 512)
        ctx.set_option("sparse_factor", -1)
        ctx.set_option("sparse_ordering", -1)
    bt = QpalmBatch(ctx, [small], ctx.default_settings(**ST))
    with pytest.raises(QpgError) as e:
        bt.sparse_factor(0)
    assert e.value.code == -5                           # a dense batch: factor() reads that one
    bt.factor(0)
    bt.close()


def check_levels(o, F):
    case = o.case
    widths = xr.etree_levels(F.Lp, F.Li, F.nf)
    assert len(widths) == o.nlev
    if case.ordering != 0:
        return widths
    if case.shape == "levels":
        assert list(widths) == [case.w + 1, case.w + 1, 1, 1, 1, 1], widths
    elif case.shape == "gadget" and not case.kkt:
        assert widths[0] % case.ngrp == 1 and widths[0] > case.ngrp and widths[0] == widths.max(), (widths, case.ngrp)
        assert widths[-1] == widths[-2] == 1          # (a run of one-column levels at the top: no workgroup barrier between them)
    return widths


# ------------------------------------------------------------------------------------------------------------------ 1. factor
@cases(GADGET + LEVELS)
def test_factor(ctx, case):
    with Opened(ctx, case) as o:
        rows_in = o.rows["active"]
        o.distinct_sigma(rows_in)
        F = o.factor_of(rows_in)
        widths = check_levels(o, F)
        by = o.rows_by_component(F, rows_in)
        r = xr.longest_column(o.ArowsP, rows_in, o.p.n)
        worst = 0.0
        for c in range(len(F.comps)):
            H, Habs = o.H(F, c, by[c]), o.H(F, c, by[c], absolute=True)
            ev = np.linalg.eigvalsh(np.asarray(H, dtype=np.float64))
            assert ev[0] > 0 and ev[-1] / ev[0] <= 1e6, (ev[0], ev[-1])
            mask = xr.sparse_pattern(F.Lp, F.Li, F.nf, cols=F.comps[c])
            assert not np.any(np.tril(np.asarray(Habs, dtype=np.float64) > 0) & ~mask), "H has an entry the factor's pattern lacks"
            R = np.abs(xr.sparse_ldl_product(F.Lp, F.Li, F.Lx, F.D, F.nf, cols=F.comps[c]) - H)
            bound = (xr.gamma_k(F.t + 2) * xr.sparse_ldl_product(F.Lp, F.Li, F.Lx, F.D, F.nf, cols=F.comps[c], absolute=True)
                     + xr.gamma_k(r + 2) * np.asarray(Habs, dtype=np.float64))
            worst = max(worst, worst_ratio(R, bound))
        print("factor %s: n = %d, nnz(L) = %d, t = %d, r = %d, level widths %s, max |R| / bound = %.3g" % (case.id, o.p.n, len(F.Li), F.t, r, list(widths[:3]), worst))
        assert worst <= 1.0, (case.id, worst)


# ------------------------------------------------------------------------------------------------------------------ 2. solve
def solve_ratio(F, Pd, Pb):
    """max over the rows of |L D L' (P d) + P b| / (3 gamma_{t+1} |L||D||L'||P d|)"""
    res = np.abs(xr.sparse_ldl_apply(F.Lp, F.Li, F.Lx, F.D, Pd) + np.asarray(Pb, dtype=xr.LD))
    bound = 3 * xr.gamma_k(F.t + 1) * xr.sparse_ldl_apply(F.Lp, F.Li, F.Lx, F.D, Pd, dtype=np.float64, absolute=True)
    return worst_ratio(res, bound)


@cases(GADGET + LEVELS + BLOCKS)
def test_solve(ctx, case):
    with Opened(ctx, case) as o:
        n, bt = o.p.n, o.bt
        assert (8 * n <= LDS_BYTES) == (case.shape != "blocks" or n == LDS_BYTES // 8)      # the right-hand side is in LDS iff it fits
        o.distinct_sigma(o.rows["active"])
        F = o.factor_of(o.rows["active"])
        check_levels(o, F)
        ends = np.zeros(n); ends[0] += 1.0; ends[n - 1] += 1.0
        for name, rhs in (("random", np.random.default_rng(600 + n).standard_normal(n)), ("e_first + e_last", ends)):
            bt.set_vec("dphi", rhs)
            bt.op("ldlsolveLD_neg_dphi")
            d = bt.vec("d")
            assert np.all(np.isfinite(d))
            ratio = solve_ratio(F, d[o.perm], rhs[o.perm])
            print("solve %s, rhs %s: max residual / bound = %.3g" % (case.id, name, ratio))
            assert ratio <= 1.0, (case.id, name, ratio)


# ------------------------------------------------------------------------------------------------------------------ 3. path updates
def _path_updown(o, start, change, sign, what, new_rows, scales=None, sigma_new=None, run=None):
    """the rank-1 terms of the rows `change` are added to (sign = +1) or taken from (-1) the factor of the active set `start`, by the boundary operation or
    by run(); the result is judged against H of the active set `new_rows` (and the penalties sigma_new); scales: the factors of a_i in the rank-1
    vectors where they are not sqrt(sigma_i)"""
    bt, case = o.bt, o.case
    F0 = o.factor_of(start)
    if run is not None:
        run()
    elif sign > 0:
        bt.set_ivec("enter", change); bt.set_scalar("nb_enter", len(change)); bt.set_scalar("nb_leave", 0)
        bt.op("ldlupdate_entering_constraints")
    else:
        bt.set_ivec("leave", change); bt.set_scalar("nb_leave", len(change)); bt.set_scalar("nb_enter", 0)
        bt.op("ldldowndate_leaving_constraints")
    F1 = Factor(bt, o.nf)
    assert F1.same_pattern(F0)                                               # (b)
    touched = set()
    for i in change:
        touched |= set(xr.etree_path(F0.parent, o.first[int(i)]))
    assert F0.off_columns_identical(F1, touched), "a column off every changed row's path was written"       # (c)
    comps = sorted({int(F0.comp_of[o.first[int(i)]]) for i in change if o.first[int(i)] >= 0})
    blocks = {}
    for c in comps:
        L, D = F0.dense(c)
        for k, i in enumerate(change):
            if o.first[int(i)] >= 0 and F0.comp_of[o.first[int(i)]] == c:
                xr.rank1_updown(L, D, o.update_vector(F0, c, i, None if scales is None else scales[k]), sign)
        blocks[c] = (L, D)
    Fr = F0.from_dense(blocks)
    big0 = o.max_abs_H(F0, start)
    e_k, _ = o.product_error(F1, new_rows, sigma_new)
    e_r, _ = o.product_error(Fr, new_rows, sigma_new)
    floor = o.nf * xr.U * big0
    ratio = e_k / max(e_r, floor)
    print("%s %s: %d rows, %d path columns, kernel %.3g, sequential fp64 reference %.3g, n u max|H0| %.3g, ratio %.3g"
          % (what, case.id, len(change), len(touched), e_k, e_r, floor, ratio))
    assert ratio <= C_PATH, (what, case.id, e_k, e_r, floor)


def _check_changing_rows(o, change):
    lens = [len(o.Arows[i]) for i in change]
    assert 0 in lens or o.case.shape == "blocks"
    if o.case.shape == "gadget":
        assert max(lens) == 2 * max(o.case.glist) + 1 and o.rows["root_only"] in change and 2 in lens
        if o.case.kind == "hip":
            assert max(lens) > 64


@cases(GADGET + BLOCKS)
def test_rows_enter_along_their_paths(ctx, case):
    with Opened(ctx, case) as o:
        change = o.changing_rows()
        _check_changing_rows(o, change)
        start = [i for i in o.rows["active"] if i not in set(change)]
        o.distinct_sigma(change)
        _path_updown(o, start, change, +1, "update", start + change)


@cases(GADGET + BLOCKS)
def test_rows_leave_along_their_paths(ctx, case):
    with Opened(ctx, case) as o:
        change = o.changing_rows()
        _check_changing_rows(o, change)
        start = sorted(set(o.rows["active"]) | set(change))
        o.distinct_sigma(change)
        _path_updown(o, start, change, -1, "downdate", [i for i in start if i not in set(change)])


@cases(GADGET)
def test_sigma_changed_on_five_active_rows(ctx, case):
    """ldlupdate_sigma_changed as the reference calls it (update_sigma has set the new sigma and scaled At_sqrt_sigma by At_scale = sqrt(factor) before):
    the factor of the old penalties becomes that of the penalties the batch reports afterwards"""
    with Opened(ctx, case) as o:
        bt, p, r = o.bt, o.p, o.rows
        start = sorted(set(r["active"]) | {row for _, _, row in r["clique"]})
        gmax = max(case.glist)
        big = [row for g, L, row in r["clique"] if (g, L) == (gmax, 2 * gmax + 1)][0]
        small = [row for g, L, row in r["clique"] if (g, L) == (min(case.glist), min(case.glist) - 1)][0]
        stars = [mine[0] for _, k, mine in r["star"] if k in (3, 2 * gmax + 1)][:2]
        changed = [big, small] + stars + [r["root_only"]]
        assert len(changed) == 5 and set(changed) <= set(start)
        mult = 1.0 + 50.0 * np.random.default_rng(4).random(5)
        sigma_old = o.sigma.copy()
        sigma_new = sigma_old.copy(); sigma_new[changed] *= mult
        scale = np.ones(p.m); scale[changed] = np.sqrt(sigma_new[changed] / sigma_old[changed])
        nzA = int(p.Ap[-1])
        row_of = np.repeat(np.arange(p.m), [len(a) for a in o.Arows])            # At: rows of A one after the other
        Atx = bt.named_vec("Atx", nzA)
        assert np.array_equal(Atx, np.array([v for a in o.Arows for _, v in a]))

        def run():
            bt.set_vec("sigma", sigma_new)
            bt.set_vec("sqrt_sigma", np.sqrt(sigma_new))
            bt.set_vec("At_sqrt_sigma", Atx * np.sqrt(sigma_new)[row_of])
            bt.set_vec("At_scale", scale)
            bt.set_ivec("enter", changed); bt.set_scalar("nb_sigma_changed", 5)
            bt.op("ldlupdate_sigma_changed")
        # the rank-1 vectors: sqrt(1 - 1 / At_scale^2) sqrt(sigma_new) a_i, i.e. sigma_new - sigma_old times a_i a_i'
        vec_scales = [np.sqrt(1.0 - 1.0 / scale[i] ** 2) * np.sqrt(sigma_new[i]) for i in changed]
        _path_updown(o, start, changed, +1, "sigma changed", start, scales=vec_scales, sigma_new=sigma_new, run=run)
        reported = bt.vec("sigma")[:p.m]
        assert np.array_equal(reported, sigma_new) and len(np.unique(reported[changed])) >= 2
        back = Atx * np.sqrt(sigma_new)[row_of]          # At_sqrt_sigma goes back to sqrt(sigma) scaling: times s, times 1 / s, two roundings
        assert np.all(np.abs(bt.named_vec("At_sqrt_sigma", nzA) - back) <= 4 * xr.U * np.abs(back))


# ------------------------------------------------------------------------------------------------------------------ 4. the sparse factor of K
class KState:
    """P K P' of the batch's current state in longdouble (exact_refs.kkt_matrix on the batch's own A_values, Q_values, sigma_inv, gamma and kkt_state;
    the matrix with every row present is built once per batch, a state then turns the absent rows into unit rows)"""

    def __init__(self, o):
        bt, p = o.bt, o.p
        n, m = p.n, p.m
        if not hasattr(o, "K_all"):
            Ax, Qx = bt.named_vec("A_values", int(p.Ap[-1])), bt.named_vec("Q_values", int(p.Qp[-1]))
            Arows, Qrows = xr.csc_to_rows(m, n, p.Ap, p.Ai, Ax), xr.sym_rows_from_lower(n, p.Qp, p.Qi, Qx)
            assert Arows == o.Arows and Qrows == o.Qrows                       # scaling = 0
            o.sigma_inv = bt.vec("sigma_inv")[:m]
            assert np.all(np.abs(o.sigma_inv * o.sigma - 1.0) <= 4 * xr.U)
            K = xr.kkt_matrix(Qrows, Arows, o.sigma_inv, float(bt.stats(0).gamma), np.ones(m, dtype=np.int64))
            o.K_all = K[np.ix_(o.perm, o.perm)]
        self.sigma_inv = o.sigma_inv
        self.state = bt.ivec("kkt_state")[:m]
        unit = o.iperm[n + np.nonzero(self.state != 1)[0]]
        self.K = o.K_all.copy()
        self.K[unit, :] = 0
        self.K[:, unit] = 0
        self.K[unit, unit] = 1


def _k_error(F, KP):
    P = xr.sparse_ldl_product(F.Lp, F.Li, F.Lx, F.D, F.nf)
    return np.abs(P - KP)


def _product_from(P0, F0, F):
    """L D L' of F (longdouble) from that of F0, which has the same pattern: the terms of the columns in which the two differ are exchanged"""
    diff = np.zeros(F.nf, dtype=bool)
    diff[F0.D != F.D] = True
    diff[F0.col[F0.Lx != F.Lx]] = True
    only = np.nonzero(diff)[0]
    work = (np.diff(F.Lp) + 1.0) ** 2
    if 2 * work[only].sum() > work.sum():          # (most of the work sits in the changed columns: the plain product is cheaper than the exchange)
        return xr.sparse_ldl_product(F.Lp, F.Li, F.Lx, F.D, F.nf)
    P = P0.copy()
    xr.sparse_ldl_product(F0.Lp, F0.Li, F0.Lx, F0.D, F0.nf, into=P, sign=-1, only=only)
    xr.sparse_ldl_product(F.Lp, F.Li, F.Lx, F.D, F.nf, into=P, sign=1, only=only)
    return P


def _kkt_begin(o, extra=()):
    """kkt_form + kkt_factorize of the base active set without the rows the script adds (o.script_rows), plus `extra`"""
    bt, r = o.bt, o.rows
    absent = set(o.script_rows)
    act = [i for i in r["active"] if i not in absent] + list(extra)
    o.distinct_sigma(act)
    o.set_active(act)
    bt.op("kkt_form")
    bt.op("kkt_factorize")
    return act


def _script(o):
    """the rows of the scripted sequence: a constraint ordered after all its variables (k32 = 0), one ordered before one of them (k32 != 0), the budget
    row, the constraint ordered last, a clique row of 65 entries where the matrix has one (else the longest), the empty row"""
    p, r, ip, n = o.p, o.rows, o.iperm, o.p.n
    short = [k for k in range(p.m) if 1 <= len(o.Arows[k]) <= 2]             # star rows, boxes, the root-only row
    after = [k for k in short if all(ip[j] < ip[n + k] for j, _ in o.Arows[k])]
    before = [k for k in short if any(ip[j] > ip[n + k] for j, _ in o.Arows[k])]
    print("constraints ordered after all their variables: %d, before one of them: %d" % (len(after), len(before)))
    last = int(o.perm[-1]) - n
    assert last >= 0, "the last row of the factor is a variable"
    lens = {L: row for _, L, row in r["clique"]}
    long_row = lens.get(65, lens[max(lens)])
    o.k32_zero = after[0]
    o.k32_nonzero = before[0] if before else None            # (under the natural [x; y] order every constraint comes after its variables)
    o.ordered_last, o.long_row = last, long_row
    o.script_rows = [x for x in dict.fromkeys([o.k32_zero, o.k32_nonzero, r["budget"], last, long_row, r["empty"]]) if x is not None]


@cases(KKT)
def test_kkt_factor(ctx, case):
    with Opened(ctx, case) as o:
        o.script_rows = []
        act = _kkt_begin(o, extra=[o.rows["budget"]])            # every second row of each gadget, the empty row and the root-only row among them, and the dense row
        assert o.rows["empty"] in act
        F = Factor(o.bt, o.nf)
        ks = KState(o)
        assert set(np.where(ks.state == 1)[0]) == set(act)
        pe = int(o.iperm[o.p.n + o.rows["empty"]])
        assert F.D[pe] == 1.0 and not np.any(F.Lx[F.Lp[pe]:F.Lp[pe + 1]]) and not np.any(F.Lx[F.Li == pe])      # the empty row: a unit pivot from form + factorise
        mask = xr.sparse_pattern(F.Lp, F.Li, F.nf)
        assert not np.any(np.tril(np.asarray(ks.K, dtype=np.float64) != 0) & ~mask), "K has an entry the factor's pattern lacks"
        bound = xr.gamma_k(F.t + 2) * xr.sparse_ldl_product(F.Lp, F.Li, F.Lx, F.D, F.nf, absolute=True) + np.diag(2 * xr.U * np.abs(np.diag(ks.K)).astype(np.float64))
        ratio = worst_ratio(_k_error(F, ks.K), bound)
        print("K %s: nf = %d, nnz(L) = %d, t = %d, levels %d, max |R| / bound = %.3g" % (case.id, F.nf, len(F.Li), F.t, o.nlev, ratio))
        assert ratio <= 1.0, (case.id, ratio)
        # kkt_solve: K sol = [-dphi; 0] through the read-back factor, no refinement
        n, m = o.p.n, o.p.m
        rhs = np.random.default_rng(7).standard_normal(n)
        o.bt.set_vec("dphi", rhs)
        o.bt.op("kkt_solve")
        sol = o.bt.named_vec("sol_kkt", n + m)
        assert np.all(np.isfinite(sol)) and np.array_equal(sol[:n], o.bt.vec("d"))
        b = np.concatenate([rhs, np.zeros(m)])
        ratio = solve_ratio(F, sol[o.perm], b[o.perm])
        print("kkt_solve %s: max residual / bound = %.3g" % (case.id, ratio))
        assert ratio <= 1.0, (case.id, ratio)


@cases(KKT)
def test_kkt_row_operations(ctx, case):
    with Opened(ctx, case) as o:
        bt, p, r = o.bt, o.p, o.rows
        n, m, nf = p.n, p.m, o.nf
        _script(o)
        act = _kkt_begin(o)
        present = [i for i in act if o.Arows[i]]
        leave1 = present[1]
        steps = [("enter", o.k32_zero)]
        if o.k32_nonzero is not None:
            steps.append(("enter", o.k32_nonzero))
        else:
            assert case.ordering == 0
        steps += [("enter", r["budget"]), ("enter", o.ordered_last), ("enter", o.long_row), ("leave", r["budget"]), ("leave", leave1), ("enter", r["budget"]),
                  ("leave", o.long_row), ("enter", r["empty"])]
        steps = [s for k, s in enumerate(steps) if not (s[0] == "enter" and s in steps[:k] and ("leave", s[1]) not in steps[:k])]
        assert len(o.Arows[o.long_row]) >= (65 if case.kind == "hip" else 17) and len(o.Arows[r["budget"]]) == n
        want = np.zeros(m, dtype=np.int64); want[act] = 1
        F0 = Factor(bt, nf)
        P0 = xr.sparse_ldl_product(F0.Lp, F0.Li, F0.Lx, F0.D, nf)
        worst = 0.0
        for step, (what, k) in enumerate(steps):
            pk = int(o.iperm[n + k])
            K0 = KState(o)
            assert np.array_equal(K0.state, want)
            bt.set_ivec(what, [k])
            bt.set_scalar("nb_" + what, 1)
            bt.op("kkt_update_entering_constraints" if what == "enter" else "kkt_update_leaving_constraints")
            want[k] = 1 if what == "enter" else 2
            F1, K1 = Factor(bt, nf), KState(o)
            assert np.array_equal(K1.state, want), (step, what, k)
            assert F1.same_pattern(F0)
            # (b) exact properties
            in_row_p = F0.Li == pk
            path = xr.etree_path(F0.parent, F0.parent[pk])
            free = np.ones(nf, dtype=bool); free[[pk] + path] = False
            same = free[F0.col] & ~in_row_p
            assert np.array_equal(F1.Lx[same], F0.Lx[same]) and np.array_equal(F1.D[free], F0.D[free]), (step, "an entry outside row p, column p and the path was written")
            if what == "leave":
                assert not np.any(F1.Lx[in_row_p]) and not np.any(F1.Lx[F0.Lp[pk]:F0.Lp[pk + 1]]) and F1.D[pk] == 1.0, (step, "row / column p after a deletion")
            # (a) against the dense sequential recipe on the same starting factor
            L, D = np.asfortranarray(xr.sparse_to_unit_lower(F0.Lp, F0.Li, F0.Lx, nf)), F0.D.copy()
            if what == "enter":
                kcol = np.zeros(nf)
                for j, v in o.Arows[k]:
                    kcol[int(o.iperm[j])] = v
                d_pp = -float(K0.sigma_inv[k])
                xr.kkt_row_add(L, D, pk, kcol, d_pp)
                Kn = K1.K
                if not o.Arows[k]:      # the empty row: K's convention (a unit row) is form + factorise's; the row addition writes -1 / sigma
                    assert F1.D[pk] == d_pp and D[pk] == d_pp
                    Kn = Kn.copy(); Kn[pk, pk] = xr.LD(d_pp)
            else:
                xr.kkt_row_del(L, D, pk)
                Kn = K1.K
            Fr = F0.from_dense({None: (L, D)})
            P1 = _product_from(P0, F0, F1)
            e_k, e_r = float(np.max(np.abs(P1 - Kn))), float(np.max(np.abs(_product_from(P0, F0, Fr) - Kn)))
            floor = nf * xr.U * float(np.max(np.abs(K0.K)))
            ratio = e_k / max(e_r, floor)
            worst = max(worst, ratio)
            print("KKT row %s %s, step %d: %s row %d (%d entries, column %d of %d), kernel %.3g, reference %.3g, floor %.3g, ratio %.3g"
                  % (case.id, what, step, what, k, len(o.Arows[k]), pk, nf, e_k, e_r, floor, ratio))
            assert ratio <= C_ROW, (case.id, step, what, k, e_k, e_r, floor)
            F0, P0 = F1, P1
        assert float(np.max(np.abs(P0 - xr.sparse_ldl_product(F0.Lp, F0.Li, F0.Lx, F0.D, nf)))) <= 64 * 2.0 ** -64 * float(np.max(np.abs(P0)))      # (the exchanges have not drifted)
        # the solve after the whole sequence, judged through the factor as it stands
        rhs = np.random.default_rng(8).standard_normal(n)
        bt.set_vec("dphi", rhs)
        bt.op("kkt_solve")
        sol = bt.named_vec("sol_kkt", n + m)
        ratio = solve_ratio(F0, sol[o.perm], np.concatenate([rhs, np.zeros(m)])[o.perm])
        print("kkt_solve after the row operations %s: max residual / bound = %.3g; largest row-operation ratio %.3g" % (case.id, ratio, worst))
        assert ratio <= 1.0, (case.id, ratio)

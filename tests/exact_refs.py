"""Plain high-precision references for tests/test_ops_exact.py: numpy `longdouble` (64-bit mantissa on x86-64) and `fractions.Fraction`.

Nothing here calls the oracle or a kernel of the project: dense matrices, loops and textbook error bounds only.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of fp64


def gamma_k(k):
    """gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1)"""
    return k * U / (1.0 - k * U)


def has_extended_precision():
    return np.finfo(LD).nmant >= 63


# ---------------------------------------------------------------------------------------------------------------- matrices
def csc_to_rows(nrow, ncol, Ap, Ai, Ax):
    """rows of a CSC matrix as lists of (column, value), columns ascending"""
    rows = [[] for _ in range(nrow)]
    for j in range(ncol):
        for k in range(int(Ap[j]), int(Ap[j + 1])):
            rows[int(Ai[k])].append((j, float(Ax[k])))
    return rows


def sym_rows_from_lower(n, Qp, Qi, Qx):
    """rows of the symmetric matrix whose lower triangle is given in CSC"""
    rows = [[] for _ in range(n)]
    for j in range(n):
        for k in range(int(Qp[j]), int(Qp[j + 1])):
            i = int(Qi[k])
            if i < j:
                continue
            rows[i].append((j, float(Qx[k])))
            if i != j:
                rows[j].append((i, float(Qx[k])))
    return rows


def dense_from_rows(rows, ncol, dtype=LD):
    M = np.zeros((len(rows), ncol), dtype=dtype)
    for i, r in enumerate(rows):
        for j, v in r:
            M[i, j] += dtype(v)
    return M


def schur_matrix(Qrows, Arows, sigma, rows_in, gamma, absolute=False):
    """H = Q + sum_{i in rows_in} sigma_i a_i a_i' + I / gamma in longdouble; absolute = True: |Q| + sum sigma_i |a_i| |a_i|' + I / gamma"""
    n = len(Qrows)
    H = dense_from_rows(Qrows, n)
    if absolute:
        H = np.abs(H)
    for i in rows_in:
        r = Arows[int(i)]
        if not r:
            continue
        idx = np.array([j for j, _ in r])
        v = np.array([LD(x) for _, x in r], dtype=LD)
        if absolute:
            v = np.abs(v)
        H[np.ix_(idx, idx)] += LD(float(sigma[int(i)])) * np.outer(v, v)
    H[np.arange(n), np.arange(n)] += LD(1.0) / LD(float(gamma))
    return H


def longest_column(Arows, rows_in, n):
    cnt = np.zeros(n, dtype=np.int64)
    for i in rows_in:
        for j, _ in Arows[int(i)]:
            cnt[j] += 1
    return int(cnt.max()) if n else 0


# ---------------------------------------------------------------------------------------------------------------- L D L'
def unit_lower(L):
    n = L.shape[0]
    return np.tril(np.asarray(L, dtype=np.float64), -1) + np.eye(n)


def ldl_product(L, D, cols=None, block=128):
    """L diag(D) L' in longdouble (L unit lower triangular, fp64 input).  cols = None: the full symmetric product, by blocks of the lower triangle
    (block (I, J), J <= I, needs the columns up to the end of J only: a sixth of the work of the square product); else the listed columns,
    each as L (D (L' e_j))."""
    n = L.shape[0]
    Ll = np.asarray(L, dtype=LD)
    Dl = np.asarray(D, dtype=LD)
    if cols is not None:
        cols = np.asarray(cols, dtype=np.int64)
        return Ll @ (Dl[:, None] * Ll[cols, :].T)
    LDm = Ll * Dl[None, :]
    P = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        for j0 in range(0, i0 + 1, block):
            j1 = min(n, j0 + block)
            blk = LDm[i0:i1, :j1] @ Ll[j0:j1, :j1].T
            P[i0:i1, j0:j1] = blk
            if j0 != i0:
                P[j0:j1, i0:i1] = blk.T
    return P


def ldl_abs_product(L, D, cols=None):
    """|L| |D| |L|' in fp64 (every term is non-negative: the fp64 sum is within n u of the exact one, which the caller's margin covers)"""
    La, Da = np.abs(np.asarray(L, dtype=np.float64)), np.abs(np.asarray(D, dtype=np.float64))
    if cols is not None:
        return La @ (Da[:, None] * La[np.asarray(cols, dtype=np.int64), :].T)
    return (La * Da[None, :]) @ La.T


def rank1_updown(L, D, w, sign):
    """L D L' + sign w w' -> (L, D) in place: Gill, Golub, Murray, Saunders (1974), method C1, one rank at a time in fp64 -- the sequential recurrence the
    reference's sparse library applies along the elimination path.  L: unit lower triangular, Fortran order (columns contiguous)."""
    n = L.shape[0]
    w = np.array(w, dtype=np.float64)
    nz = np.nonzero(w)[0]
    if len(nz) == 0:
        return
    a = float(sign)
    for j in range(int(nz[0]), n):
        p = w[j]
        if p == 0.0:
            continue                 # (a column the vector does not touch stays as it is: t = 1, beta = 0)
        dj = D[j]
        dn = dj + a * p * p
        beta = p * a / dn
        a = dj * a / dn
        D[j] = dn
        if j + 1 < n:
            w[j + 1:] -= p * L[j + 1:, j]
            L[j + 1:, j] += beta * w[j + 1:]


def sequential_updown(L0, D0, vectors, sign):
    """the fp64 reference factor after the rank-1 changes `vectors` (rows of a 2-d array), in the order given"""
    L = np.asfortranarray(unit_lower(L0))
    D = np.array(D0, dtype=np.float64)
    for w in vectors:
        rank1_updown(L, D, w, sign)
    return L, D


# ---------------------------------------------------------------------------------------------------------------- SpMV
def spmv_fraction(rows, x):
    """(y, bound): y_i = sum_j a_ij x_j exactly (Fraction), bound_i = gamma_r sum |a_ij| |x_j| with r the length of row i -- the componentwise
    bound of a sum of r products in any order, with or without FMA (Higham, section 3.1)"""
    xs = [Fraction(float(v)) for v in x]
    y, bnd = [], []
    for r in rows:
        s, t = Fraction(0), Fraction(0)
        for j, v in r:
            pr = Fraction(v) * xs[j]
            s += pr
            t += abs(pr)
        y.append(s)
        bnd.append(Fraction(gamma_k(max(len(r), 1))) * t)
    return y, bnd


# ---------------------------------------------------------------------------------------------------------------- line search
def linesearch_derivative(tau, d, Qd, df, delta, alpha):
    """(psi'(tau), sum of the absolute values of its terms, number of active breakpoints), exactly, of the piecewise quadratic of exact_linesearch:
         psi'(t) = t d'Qd + d'df + sum_i delta_i max(delta_i t - alpha_i, 0)
    over the 2m breakpoints (delta_i, alpha_i) the kernel wrote; Qd holds Q d + d / gamma.  The terms are d_j Qd_j t, d_j df_j and, for every i with
    delta_i t - alpha_i > 0, delta_i^2 t and delta_i alpha_i."""
    t = Fraction(float(tau))
    val, mag, nact = Fraction(0), Fraction(0), 0
    for dj, qj, fj in zip(d, Qd, df):
        a, b = Fraction(float(dj)) * Fraction(float(qj)) * t, Fraction(float(dj)) * Fraction(float(fj))
        val += a + b
        mag += abs(a) + abs(b)
    for de, al in zip(delta, alpha):
        de, al = Fraction(float(de)), Fraction(float(al))
        if de * t - al > 0:
            val += de * (de * t - al)
            mag += de * de * abs(t) + abs(de * al)
            nact += 1
    return val, mag, nact

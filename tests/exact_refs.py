"""Plain high-precision references for tests/test_ops_exact.py and tests/test_sparse_ops_exact.py: numpy `longdouble` (64-bit mantissa on x86-64) and `fractions.Fraction`.

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


def schur_matrix(Qrows, Arows, sigma, rows_in, gamma, absolute=False, cols=None):
    """H = Q + sum_{i in rows_in} sigma_i a_i a_i' + I / gamma in longdouble; absolute = True: |Q| + sum sigma_i |a_i| |a_i|' + I / gamma.
    cols: the square block H[cols][:, cols] instead (rows / columns in the order given) of a set of columns that H does not couple to the rest --
    a row of Q among them, or a row of A of rows_in that touches them, with an entry outside raises AssertionError"""
    if cols is None:
        n = len(Qrows)
        H = dense_from_rows(Qrows, n)
        local = None
    else:
        n = len(cols)
        local = {int(c): k for k, c in enumerate(cols)}
        H = np.zeros((n, n), dtype=LD)
        for k, c in enumerate(cols):
            for j, v in Qrows[int(c)]:
                assert j in local, "Q couples column %d to column %d outside the block" % (int(c), j)
                H[k, local[j]] += LD(v)
    if absolute:
        H = np.abs(H)
    for i in rows_in:
        r = Arows[int(i)]
        if not r:
            continue
        if local is None:
            idx = np.array([j for j, _ in r])
        else:
            assert all(j in local for j, _ in r) or not any(j in local for j, _ in r), "row %d of A leaves the block" % int(i)
            if r[0][0] not in local:
                continue
            idx = np.array([local[j] for j, _ in r])
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


# ---------------------------------------------------------------------------------------------------------------- sparse L D L'
def sparse_to_unit_lower(Lp, Li, Lx, n, cols=None):
    """the dense unit lower triangular matrix of a factor read back in compressed columns (strict lower part); cols: the square block on these
    columns (ascending; a union of trees of the elimination forest, so no entry of theirs lies outside) instead of the whole matrix.  Asserts what a
    compressed lower triangle must satisfy: monotone pointers, rows strictly ascending within a column, every row index below the diagonal."""
    Lp, Li = np.asarray(Lp, dtype=np.int64), np.asarray(Li, dtype=np.int64)
    assert len(Lp) == n + 1 and Lp[0] == 0 and np.all(np.diff(Lp) >= 0) and Lp[n] <= len(Li)
    if cols is None:
        cols, local = np.arange(n), None
    else:
        cols = np.asarray(cols, dtype=np.int64)
        assert np.all(np.diff(cols) > 0)
        local = np.full(n, -1, dtype=np.int64)
        local[cols] = np.arange(len(cols))
    L = np.eye(len(cols))
    for k, j in enumerate(cols):
        r = Li[Lp[j]:Lp[j + 1]]
        assert np.all(r > j) and np.all(r < n) and np.all(np.diff(r) > 0), j
        if local is not None:
            r = local[r]
            assert np.all(r >= 0), j
        L[r, k] = Lx[Lp[j]:Lp[j + 1]]
    return L


def sparse_ldl_product(Lp, Li, Lx, D, n, cols=None, absolute=False, into=None, sign=1, only=None):
    """L diag(D) L' of the compressed factor over its pattern, in longdouble (absolute: |L| |D| |L|' in fp64, every term non-negative): column j adds
    d_j (1; l_j)(1; l_j)' on the rows of its pattern, so the work is the sum of the squared column lengths and no entry outside the pattern of
    L + L' is ever touched (the rows of a column's pattern form a clique of the filled graph).  The same block as sparse_to_unit_lower's.
    into / sign / only: the terms of the columns `only` are added to (sign = 1) or taken from (-1) the matrix `into` instead -- the product of a
    factor that differs from another one in a few columns, from that one's (two more longdouble roundings per entry and changed column)."""
    Lp, Li = np.asarray(Lp, dtype=np.int64), np.asarray(Li, dtype=np.int64)
    if cols is None:
        cols, local = np.arange(n), np.arange(n)
    else:
        cols = np.asarray(cols, dtype=np.int64)
        local = np.full(n, -1, dtype=np.int64)
        local[cols] = np.arange(len(cols))
    dt = np.float64 if absolute else LD
    P = np.zeros((len(cols), len(cols)), dtype=dt) if into is None else into
    assert P.dtype == dt and P.shape == (len(cols), len(cols))
    for c, j in (enumerate(cols) if only is None else ((int(local[j]), int(j)) for j in only)):
        e0, e1 = int(Lp[j]), int(Lp[j + 1])
        idx = np.concatenate([[c], local[Li[e0:e1]]])
        assert np.all(idx >= 0), j
        v = np.concatenate([[1.0], np.asarray(Lx[e0:e1], dtype=np.float64)]).astype(dt)
        d = dt(D[j])
        if absolute:
            v, d = np.abs(v), abs(d)
        P[np.ix_(idx, idx)] += (d if sign > 0 else -d) * np.outer(v, v)
    return P


def sparse_pattern(Lp, Li, n, cols=None):
    """boolean mask of the pattern (strict lower part and diagonal) of the same block as sparse_to_unit_lower's"""
    return sparse_to_unit_lower(Lp, Li, np.ones(len(Li)), n, cols) != 0


def etree_parent(Lp, Li, n):
    """parent of column j in the elimination tree = the first row index of its pattern, -1 at a root"""
    return np.array([int(Li[Lp[j]]) if Lp[j + 1] > Lp[j] else -1 for j in range(n)], dtype=np.int64)


def etree_levels(Lp, Li, n):
    """widths of the levels of the elimination tree: leaves at level 0, a column at 1 + the highest level among its children"""
    parent = etree_parent(Lp, Li, n)
    level = np.zeros(n, dtype=np.int64)
    for j in range(n):
        p = parent[j]
        if p >= 0:
            assert p > j
            level[p] = max(level[p], level[j] + 1)
    return np.bincount(level)


def etree_components(Lp, Li, n):
    """the trees of the elimination forest as ascending arrays of columns (the connected components of the pattern)"""
    parent = etree_parent(Lp, Li, n)
    root = np.arange(n)
    for j in range(n - 1, -1, -1):
        if parent[j] >= 0:
            root[j] = root[parent[j]]
    order = np.argsort(root, kind="stable")
    cuts = np.nonzero(np.diff(root[order]))[0] + 1
    return [np.sort(c) for c in np.split(order, cuts)]


def etree_path(parent, j):
    """columns from j to its root (empty for j < 0)"""
    out = []
    while j >= 0:
        out.append(int(j))
        j = parent[j]
    return out


def sparse_ldl_apply(Lp, Li, Lx, D, x, dtype=LD, absolute=False):
    """L diag(D) L' x for the compressed factor, in `dtype`; absolute: |L| |D| |L|' |x|"""
    n = len(D)
    col = np.repeat(np.arange(n), np.diff(np.asarray(Lp, dtype=np.int64)[:n + 1]))
    nz = int(Lp[n])
    Li = np.asarray(Li, dtype=np.int64)[:nz]
    lx, d, x = np.asarray(Lx[:nz], dtype=dtype), np.asarray(D, dtype=dtype), np.asarray(x, dtype=dtype)
    if absolute:
        lx, d, x = np.abs(lx), np.abs(d), np.abs(x)
    y = x.copy()
    np.add.at(y, col, lx * x[Li])          # L' x
    y = d * y
    z = y.copy()
    np.add.at(z, Li, lx * y[col])          # L (D L' x)
    return z


# ---------------------------------------------------------------------------------------------------------------- K and its row operations
def kkt_matrix(Qrows, Arows, sigma_inv, gamma, state):
    """K = [[Q + I / gamma, A_a'], [A_a, -Sigma_a^-1]] in longdouble, [x; y] numbering: a constraint with state 1 and at least one entry is present,
    every other constraint is a unit row (tests/test_sparse_kkt.py: _K)"""
    n, m = len(Qrows), len(Arows)
    K = np.zeros((n + m, n + m), dtype=LD)
    K[:n, :n] = dense_from_rows(Qrows, n)
    K[np.arange(n), np.arange(n)] += LD(1.0) / LD(float(gamma))
    for k in range(m):
        if int(state[k]) == 1 and Arows[k]:
            for j, v in Arows[k]:
                K[n + k, j] = K[j, n + k] = LD(v)
            K[n + k, n + k] = -LD(float(sigma_inv[k]))
        else:
            K[n + k, n + k] = LD(1.0)
    return K


def kkt_row_add(L, D, p, kcol, d_pp):
    """row / column p of the factored matrix goes from a unit row to (kcol off the diagonal, d_pp on it): the bordering step of the header of
    qpalm_sparse_kkt.h, dense and sequential in fp64, in place.  L11 z = k12; l21 = z / d1; d22 = d_pp - l21 z; l32 = (k32 - L31 z) / d22; then
    the rank-1 term -d22 l32 l32' on the trailing block (rank1_updown).  L: unit lower triangular, Fortran order."""
    n = L.shape[0]
    z = np.array(kcol[:p], dtype=np.float64)
    for j in range(p):
        if z[j] != 0.0 and j + 1 < p:
            z[j + 1:] -= L[j + 1:p, j] * z[j]
    l21 = z / D[:p]
    d22 = float(d_pp) - float(np.dot(l21, z))
    l32 = (np.array(kcol[p + 1:], dtype=np.float64) - L[p + 1:, :p] @ z) / d22
    L[p, :p] = l21
    L[p + 1:, p] = l32
    D[p] = d22
    w = np.zeros(n)
    w[p + 1:] = np.sqrt(abs(d22)) * l32
    rank1_updown(L, D, w, 1.0 if d22 < 0 else -1.0)


def kkt_row_del(L, D, p):
    """row / column p becomes a unit row: w = sqrt|d_p| L(:, p), row and column p zeroed, d_p = 1, then the rank-1 term + d_p l l' on the
    trailing block; in place"""
    n = L.shape[0]
    d = float(D[p])
    w = np.zeros(n)
    w[p + 1:] = np.sqrt(abs(d)) * L[p + 1:, p]
    L[p, :p] = 0.0
    L[p + 1:, p] = 0.0
    D[p] = 1.0
    rank1_updown(L, D, w, 1.0 if d > 0 else -1.0)


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

"""Problems and references of tests/test_adjoint.py.

Problems are planted: a solution x*, an active set J with sides and multipliers y* are chosen first and q and the bounds derived from them, so that the QP
is strictly complementary (|y_i| >= 0.5 on J, slack >= 0.5 and y_i = 0 elsewhere) and no rule can disagree about J.  Q = G G' + I with a sparse G;
the active rows of A carry a dominant entry each in a column of their own, which keeps them linearly independent.

References: at a fixed J the gradients are one linear solve K [u; w] = [gx; gy_J], K = [[Q, A_J'], [A_J, 0]] -- Gaussian elimination with partial pivoting
in numpy.longdouble plus one step of refinement there, or exactly in rational arithmetic where the system is small."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

from qpalm_amd.problems import QP, _csc

LD = np.longdouble


def plant(Qf, A, side, seed, equality=()):
    """(QP, x*, y*) with the given full symmetric Q and A (scipy sparse): side[i] in {-1, 0, 1} says where row i sits at the solution; rows listed in
    `equality` get bmin = bmax"""
    rng = np.random.Generator(np.random.PCG64(seed))
    m, n = A.shape
    side = np.asarray(side)
    x = rng.standard_normal(n)
    y = np.where(side != 0, side * (0.5 + rng.random(m)), 0.0)      # y > 0 on an upper bound, < 0 on a lower one
    eq = np.zeros(m, bool)
    eq[list(equality)] = True
    y = np.where(eq, y * np.where(rng.random(m) < 0.5, -1.0, 1.0), y)
    ax = A @ x
    lo = np.where(side < 0, ax, ax - 0.5 - rng.random(m))
    hi = np.where(side > 0, ax, ax + 0.5 + rng.random(m))
    lo, hi = np.where(eq, ax, lo), np.where(eq, ax, hi)
    q = -(Qf @ x) - A.T @ y
    Qp, Qi, Qx = _csc(sp.tril(sp.csc_matrix(Qf)))
    Ap, Ai, Ax = _csc(sp.csc_matrix(A))
    return QP(n, m, Qp, Qi, Qx, Ap, Ai, Ax, q, lo, hi), x, y


def planted_qp(n, m, nact, seed, sides="mixed", equality=False):
    """random planted QP: Q = G G' + I, `nact` <= min(n, m) active rows (sides: "mixed", "lower"; equality: all of them bmin = bmax).
    Returns (QP, side, x*, y*)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    per = min(n, 4)
    G = sp.random(n, n, density=min(1.0, 2.0 / n), format="csc", random_state=rng, data_rvs=rng.standard_normal)
    Qf = (G @ G.T + sp.identity(n)).tocsc()
    rows, cols, vals = [], [], []
    own = rng.permutation(n)                      # the column in which active row k is dominant
    act_rows = np.sort(rng.choice(m, size=nact, replace=False)) if nact else np.zeros(0, int)
    for i in range(m):
        c = set(int(v) for v in rng.choice(n, size=per, replace=False))
        for j in c:
            rows.append(i); cols.append(j); vals.append(0.3 * rng.standard_normal())
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n)).tolil()
    for k, i in enumerate(act_rows):
        A[i, int(own[k])] = 2.0 + rng.random()
    A = sp.csc_matrix(A)
    side = np.zeros(m, int)
    if nact:
        side[act_rows] = -1 if sides == "lower" else np.where(rng.random(nact) < 0.5, -1, 1)
    p, x, y = plant(Qf, A, side, seed + 1, equality=act_rows if equality else ())
    if equality:
        side[act_rows] = -1                       # an equality row counts as lower
    return p, side, x, y


def replant(p, nact, seed):
    """a given QP's Q and A (tests/sparse_gadgets.py) with q and bounds planted: up to `nact` active rows chosen greedily so that they stay independent"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A, Qf = p.A_mat(), p.Q_full()
    Ad = A.toarray()
    chosen = []
    for i in rng.permutation(p.m):
        if len(chosen) >= nact:
            break
        if np.count_nonzero(Ad[i]) and np.linalg.matrix_rank(Ad[chosen + [int(i)]]) == len(chosen) + 1:
            chosen.append(int(i))
    side = np.zeros(p.m, int)
    side[chosen] = np.where(rng.random(len(chosen)) < 0.5, -1, 1)
    pp, x, y = plant(Qf, A, side, seed + 1)
    return pp, side, x, y


def shuffled_entries(p, seed):
    """the same QP as a caller may hand it over: Q with BOTH triangles stored, the entries of every column of Q and of A in a random order.  The engine
    keeps the lower entries of Q, sorted, so its order of the values is not the caller's: update_Q_A's maps (and the adjoint's, the other way round)"""
    rng = np.random.Generator(np.random.PCG64(seed))

    def shuffle(M):
        M = sp.csc_matrix(M); M.sort_indices()
        Mp, Mi, Mx = M.indptr.astype(np.int64), M.indices.astype(np.int64).copy(), M.data.astype(np.float64).copy()
        for j in range(M.shape[1]):
            perm = Mp[j] + rng.permutation(Mp[j + 1] - Mp[j])
            Mi[Mp[j]:Mp[j + 1]], Mx[Mp[j]:Mp[j + 1]] = Mi[perm], Mx[perm]
        return Mp, Mi, Mx
    Qp, Qi, Qx = shuffle(p.Q_full())
    Ap, Ai, Ax = shuffle(p.A_mat())
    return QP(p.n, p.m, Qp, Qi, Qx, Ap, Ai, Ax, p.q, p.bmin, p.bmax)


def kkt_dense(p, J):
    """K = [[Q, A_J'], [A_J, 0]] of the problem's own (unscaled) data, float64"""
    Q, A = p.Q_full().toarray(), p.A_mat().toarray()
    AJ = A[J]
    k = len(J)
    return np.block([[Q, AJ.T], [AJ, np.zeros((k, k))]])


def _ge_solve(K, rhs, dtype):
    """Gaussian elimination with partial pivoting in `dtype` (numpy.linalg has no extended precision)"""
    M = np.array(K, dtype=dtype)
    b = np.array(rhs, dtype=dtype)
    N = len(b)
    for c in range(N):
        pv = c + int(np.argmax(np.abs(M[c:, c])))
        if pv != c:
            M[[c, pv]] = M[[pv, c]]; b[[c, pv]] = b[[pv, c]]
        f = M[c + 1:, c] / M[c, c]
        M[c + 1:, c:] -= np.outer(f, M[c, c:])
        b[c + 1:] -= f * b[c]
    z = np.zeros(N, dtype=dtype)
    for c in range(N - 1, -1, -1):
        z[c] = (b[c] - M[c, c + 1:] @ z[c + 1:]) / M[c, c]
    return z


def solve_longdouble(K, rhs):
    Kl, rl = np.array(K, dtype=LD), np.array(rhs, dtype=LD)
    z = _ge_solve(Kl, rl, LD)
    return z + _ge_solve(Kl, rl - Kl @ z, LD)     # one step of refinement in the same precision


def solve_rational(K, rhs):
    """exact: Gauss-Jordan on Fractions (every float64 is a rational); for systems of a dozen unknowns"""
    N = len(rhs)
    M = [[Fraction(float(v)) for v in row] + [Fraction(float(r))] for row, r in zip(K, rhs)]
    for c in range(N):
        pv = next(r for r in range(c, N) if M[r][c] != 0)
        M[c], M[pv] = M[pv], M[c]
        inv = 1 / M[c][c]
        M[c] = [v * inv for v in M[c]]
        for r in range(N):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return np.array([M[r][N] for r in range(N)], dtype=object)


def reference(p, side, gx, gy, exact_below=14):
    """(z_ref as longdouble [u; w_J], z of float64 numpy.linalg.solve, J): the reference solve and the yardstick's own answer"""
    J = np.flatnonzero(side)
    K = kkt_dense(p, J)
    rhs = np.concatenate([gx, gy[J] if gy is not None else np.zeros(len(J))])
    if len(rhs) <= exact_below:
        zr = np.array([LD(v.numerator) / LD(v.denominator) for v in solve_rational(K, rhs)], dtype=LD)
    else:
        zr = solve_longdouble(K, rhs)
    return zr, np.linalg.solve(K, rhs), J


def gradients(p, side, x, y, z):
    """the outputs of the adjoint from [u; w_J] (any dtype) and the solution (x, y): dq, dbmin, dbmax, dQx, dAx in the problem's own entry order"""
    n, m = p.n, p.m
    J = np.flatnonzero(side)
    u = z[:n]
    w = np.zeros(m, dtype=z.dtype)
    w[J] = z[n:]
    dq = -u
    dbmin, dbmax = np.where(side < 0, w, 0), np.where(side > 0, w, 0)
    ca = np.repeat(np.arange(n), np.diff(p.Ap))
    dAx = -(y[p.Ai] * u[ca] + w[p.Ai] * x[ca])
    cq = np.repeat(np.arange(n), np.diff(p.Qp))
    dQx = np.where(p.Qi == cq, -(u[cq] * x[cq]), -(u[p.Qi] * x[cq] + u[cq] * x[p.Qi]))
    dQx = np.where(p.Qi < cq, 0, dQx)             # an upper entry is not part of the problem
    return dict(dq=dq, dbmin=dbmin, dbmax=dbmax, dQx=dQx, dAx=dAx)


def default_rule(bt, p, b=0):
    """numpy restatement of the engine's set_active_constraints test on the stored solution, in scaled space, from what `vec` reads"""
    n, m = p.n, p.m
    x, y = bt.solution_of(b)
    scaled = int(bt.settings.scaling) > 0
    D, E = (bt.vec("D", b)[:n], bt.vec("E", b)[:m]) if scaled else (np.ones(n), np.ones(m))
    c = float(bt.stats(b).sc_c) if scaled else 1.0
    sigma = bt.vec("sigma", b)[:m]
    A = p.A_mat()
    Ab = sp.diags(E) @ A @ sp.diags(D)
    axys = Ab @ (x / D) + (c * y / E) / sigma
    lo, hi = E * p.bmin, E * p.bmax
    return np.where((p.bmin == p.bmax) | (axys <= lo), -1, np.where(axys >= hi, 1, 0))

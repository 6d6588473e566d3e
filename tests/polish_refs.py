"""References of tests/test_polish.py, all in numpy.longdouble on the problem's own (unscaled) data.

The candidate of a polish does not depend on the point it starts from: K [x + dx; y_J + dy_J] = [-q; b_J] with K = [[Q, A_J'], [A_J, 0]], b_i = bmin_i on a
lower-active row and bmax_i on an upper-active one, so the reference is the solve of tests/adjoint_refs.py on that right-hand side (exact in rationals below
14 unknowns), followed by the clip.  The residual measures are those of the solver's termination test in unscaled space."""
import numpy as np

from tests import adjoint_refs as R
from tests.exact_refs import gamma_k

LD = R.LD


def bound_rhs(p, side):
    """b: bmin on lower-active rows, bmax on upper-active ones (full length m; rows outside J are never read)"""
    return np.where(np.asarray(side) < 0, p.bmin, p.bmax)


def candidate(p, side):
    """(z_ref longdouble [x; y_J], z of float64 numpy.linalg.solve, J) of K z = [-q; b_J]"""
    return R.reference(p, side, -p.q, bound_rhs(p, side))


def clip(p, side, yJ, J):
    """y of full length from y_J: zero outside J; on a row of J with bmin < bmax a multiplier on the wrong side of its bound is set to zero"""
    y = np.zeros(p.m, dtype=LD)
    y[J] = yJ
    eq = p.bmin == p.bmax
    wrong = (side != 0) & ~eq & (((side < 0) & (y > 0)) | ((side > 0) & (y < 0)))
    return np.where(wrong, LD(0), y)


def dense(p):
    return p.Q_full().toarray().astype(LD), p.A_mat().toarray().astype(LD)


def residuals(p, x, y, mats=None):
    """pri = max_i max(bmin_i - (A x)_i, (A x)_i - bmax_i, 0), dua = ||Q x + q + A' y||inf, and the norms the thresholds take, in longdouble"""
    Q, A = mats if mats is not None else dense(p)
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    ax, qx, aty = A @ x, Q @ x, A.T @ y
    lo, hi = p.bmin.astype(LD), p.bmax.astype(LD)
    inf = lambda v: np.max(np.abs(v)) if len(v) else LD(0)
    pri = np.max(np.maximum(np.maximum(lo - ax, ax - hi), 0)) if p.m else LD(0)
    dua = inf(qx + p.q.astype(LD) + aty)
    norm_pri = max(inf(ax), inf(np.minimum(np.maximum(ax, lo), hi)))
    norm_dua = max(inf(qx), inf(p.q), inf(aty))
    return dict(pri=pri, dua=dua, norm_pri=norm_pri, norm_dua=norm_dua)


def verdict(p, side, x, y, eps_abs, eps_rel):
    """the whole call in longdouble from the stored (x, y) and the set used: candidate, clip, residuals before and after, thresholds, accepted or not"""
    mats = dense(p)
    zr, _, J = candidate(p, side)
    xh, yh = zr[:p.n], clip(p, np.asarray(side), zr[p.n:], J)
    old, new = residuals(p, x, y, mats), residuals(p, xh, yh, mats)
    eps_pri, eps_dua = eps_abs + eps_rel * new["norm_pri"], eps_abs + eps_rel * new["norm_dua"]
    ok = new["pri"] <= max(old["pri"], eps_pri) and new["dua"] <= max(old["dua"], eps_dua)
    return dict(x=xh, y=yh, old=old, new=new, eps_pri=eps_pri, eps_dua=eps_dua, accepted=bool(ok))


def residual_bounds(p, x, y, nscale):
    """Componentwise rounding bounds on the device's pri and dua of (x, y): gamma_k (|A| |x| + |b|) and gamma_k (|Q| |x| + |q| + |A'| |y|), maxima over the rows.

    The device evaluates them on the scaled problem and scales back (u = one rounding):
      entries   A~_ij: every scaling pass multiplies by the pass's E and D factor (2 u) and D, E themselves are running products (1 u each): 4 u per pass;
                Q~_ij = ((D_i D_j) Q_ij) c: 3 u;    q~_j = (D_j q_j) c: 2 u;    b~_i = E_i b_i: 1 u
      vectors   x~_j = x_j * (1 / D_j): 2 u;        y~_i = (y_i * (1 / E_i)) c: 3 u
      sums      a row of r entries: r u (Higham, Lemma 3.1, whatever the order)
      way back  A x: Einv_i (b~_i - s_i): the subtraction, Einv (a rounded reciprocal) and the product: 3 u
                dual: (Q~x~ + q~) + A~'y~: 2 u, then Dinv_j and 1 / c, rounded reciprocals, and the two products: 4 u
    so k_pri = r_A' + 4 passes + 2 + 3 (the b term has fewer) and k_dua = max(r_Q + 3 + 2, 2, r_A + 4 passes + 3) + 6, r the longest row of A / of the full
    Q / the longest column of A.  Without scaling the same bounds hold with room to spare."""
    Q, A = dense(p)
    rA = int(np.max(np.diff(p.A_mat().tocsr().indptr))) if p.m else 0
    cA = int(np.max(np.diff(p.Ap))) if p.n else 0
    rQ = int(np.max(np.diff(p.Q_full().tocsc().indptr)))
    k_pri = rA + 4 * nscale + 5
    k_dua = max(rQ + 5, cA + 4 * nscale + 3) + 6
    ax, ay = np.abs(np.asarray(x, dtype=LD)), np.abs(np.asarray(y, dtype=LD))
    b = np.maximum(np.where(np.abs(p.bmin) < 1e20, np.abs(p.bmin), 0), np.where(np.abs(p.bmax) < 1e20, np.abs(p.bmax), 0)).astype(LD)
    bpri = LD(gamma_k(k_pri)) * np.max(np.abs(A) @ ax + b) if p.m else LD(0)
    bdua = LD(gamma_k(k_dua)) * np.max(np.abs(Q) @ ax + np.abs(p.q).astype(LD) + np.abs(A).T @ ay)
    return bpri, bdua, k_pri, k_dua

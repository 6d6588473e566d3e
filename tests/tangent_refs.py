"""References of tests/test_tangent.py: the tangent of a solved QP along one direction of its data.

At a fixed active set J (sides as in tests/adjoint_refs.py) and a solution (x, y), for a direction d = (dq, dbmin, dbmax, dQx, dAx) -- the last two per
stored entry, in the problem's own order of the entries --
    r1 = -(dq + dQ x + dA' y)        (y of EVERY row),        r2_i = db_i - (dA x)_i on J  (db_i = dbmin_i on a lower row, dbmax_i on an upper one),
    K [dx; dy_J] = [r1; r2],  K = [[Q, A_J'], [A_J, 0]].
dQ is the symmetric matrix the stored LOWER entries give (an entry below the diagonal stands for both positions); upper entries are not part of the
problem.  r1 and r2 are formed in numpy.longdouble; the solve is adjoint_refs.reference (exact in rationals below 14 unknowns, longdouble elimination
above).  That function takes float64 right-hand sides, so the longdouble one goes in as the sum of two float64 vectors (head and tail) and the two
solutions are added: the solve is linear, and the yardstick float64 numpy.linalg.solve gets the head, the right-hand side rounded to float64."""
import numpy as np

from tests import adjoint_refs as R

LD = R.LD
KEYS = ("dq", "dbmin", "dbmax", "dQx", "dAx")


def direction(p, rng, keys=KEYS):
    """a random direction in the problem's own entry order (a dict; absent keys = zero)"""
    size = dict(dq=p.n, dbmin=p.m, dbmax=p.m, dQx=len(p.Qx), dAx=len(p.Ax))
    return {k: rng.standard_normal(size[k]) for k in keys}


def rhs(p, side, x, y, d):
    """(r1 [n], r2 [m] with zeros outside J) in longdouble"""
    n, m = p.n, p.m
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    get = lambda k, size: np.asarray(d[k], dtype=LD) if d.get(k) is not None else np.zeros(size, dtype=LD)
    dq, lo, hi, dQx, dAx = get("dq", n), get("dbmin", m), get("dbmax", m), get("dQx", len(p.Qx)), get("dAx", len(p.Ax))
    cq, ca = np.repeat(np.arange(n), np.diff(p.Qp)), np.repeat(np.arange(n), np.diff(p.Ap))
    Qi, Ai = np.asarray(p.Qi), np.asarray(p.Ai)
    dQx_v = np.zeros(n, dtype=LD)
    low, strict = Qi >= cq, Qi > cq
    np.add.at(dQx_v, Qi[low], dQx[low] * x[cq[low]])               # entry (i, j), i >= j: row i takes dQ_ij x_j ...
    np.add.at(dQx_v, cq[strict], dQx[strict] * x[Qi[strict]])      # ... and, below the diagonal, row j takes dQ_ij x_i
    dAty = np.zeros(n, dtype=LD)
    np.add.at(dAty, ca, dAx * y[Ai])
    dAx_v = np.zeros(m, dtype=LD)
    np.add.at(dAx_v, Ai, dAx * x[ca])
    side = np.asarray(side)
    r1 = -(dq + dQx_v + dAty)
    r2 = np.where(side != 0, np.where(side < 0, lo, hi) - dAx_v, LD(0))
    return r1, r2


def tangent(p, side, x, y, d):
    """(z_ref as longdouble [dx; dy_J], z of float64 numpy.linalg.solve on the right-hand side rounded to float64, J)"""
    r1, r2 = rhs(p, side, x, y, d)
    h1, h2 = r1.astype(np.float64), r2.astype(np.float64)
    t1, t2 = (r1 - h1).astype(np.float64), (r2 - h2).astype(np.float64)
    zh, z64, J = R.reference(p, side, h1, h2)
    zt, _, _ = R.reference(p, side, t1, t2)
    return zh + zt, z64, J


def pairing(d, g):
    """<g, d> over the five arrays, in longdouble (absent in d = zero)"""
    return sum((np.asarray(g[k], dtype=LD) @ np.asarray(d[k], dtype=LD) for k in KEYS if d.get(k) is not None), LD(0))


def norm1(d):
    return float(sum(np.sum(np.abs(d[k])) for k in KEYS if d.get(k) is not None))

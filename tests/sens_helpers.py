"""What the tests of the sensitivity calls share (test_adjoint, test_tangent, test_polish, test_subset, test_sens_penalty, test_sens_at, test_sens_multi,
test_sens_routes, and tools/evidence): tensors to and from the backend, the planted batches, the judges against tests/adjoint_refs.py,
tests/tangent_refs.py and tests/polish_refs.py, and the scaffold of the refused modes.

The rule of every judge: nothing fixed in advance.  err64 = max |z_numpy - z_ref| / max |z_ref| of float64 numpy.linalg.solve on the same system is
measured, and the kernel's error, measured the same way, must stay within 8 x err64.  Each prints its figures under the tag of the calling file
(ADJOINT-ACC, TANGENT-ACC, POLISH-ACC, SENS-AT): profiles/*/accuracy.md record them."""
import contextlib
import dataclasses

import numpy as np
import torch

from qpalm_amd.solver import QpalmBatch
from tests import adjoint_refs as R
from tests import polish_refs as PR
from tests import tangent_refs as TR

ST = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=0)
U = 2.0 ** -53
INVALID, UNSUPPORTED = -2, -5


def dev(ctx):
    return "cuda:0" if ctx.kind == "hip" else "cpu"


def T(ctx, a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev(ctx))


def N(t):
    return t.detach().cpu().numpy()


def host(out):
    return {k: (N(v) if hasattr(v, "detach") else v) for k, v in out.items()}


def padded(rows, width, dtype=np.float64, fill=0):
    out = np.full((len(rows), width), fill, dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    m: int
    nact: int
    scaling: int
    proximal: int
    sides: str = "mixed"
    equality: bool = False
    gy: bool = True

    @property
    def id(self):
        return "n%d-m%d-J%d%s-s%d-p%d" % (self.n, self.m, self.nact, "eq" if self.equality else "", self.scaling, self.proximal)


# n on the edges of the 32- and 64-column blocks and of the hand-over between the 128-, 256- and 512-thread instances (tests/test_adjoint.py)
CASES = [Case(1, 2, 1, 10, 0, sides="lower"), Case(1, 2, 0, 0, 1), Case(5, 8, 3, 10, 1), Case(31, 62, 12, 0, 1), Case(33, 16, 1, 10, 1, gy=False),
         Case(64, 128, 63, 10, 0, equality=True), Case(65, 32, 20, 10, 0), Case(192, 96, 60, 0, 0), Case(193, 386, 90, 10, 1),
         Case(256, 128, 0, 10, 1), Case(257, 514, 256, 0, 1, equality=True)]


def assert_complementary(p, side, x, y):
    """active rows: on their bound with |y| >= 1e-2; the others: slack >= 1e-2 and |y| <= 1e-8"""
    ax = p.A_mat() @ x
    act = side != 0
    assert np.all(np.abs(y[act]) >= 1e-2)
    assert np.all(np.abs(y[~act]) <= 1e-8)
    slack = np.minimum(ax - p.bmin, p.bmax - ax)
    assert np.all(slack[~act] >= 1e-2)
    assert np.all(np.abs(np.where(side < 0, ax - p.bmin, ax - p.bmax))[act] <= 1e-6)


def assert_instance(ctx, bt, threads):
    """the instance of the kernels the batch runs on: a silently different one fails here (the emulator has one, of 128 threads)"""
    assert bt.launch_shape()[1] == (threads if ctx.kind == "hip" else 128), bt.launch_shape()


def solved(ctx, probs, warm=None, **st):
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, **st)))
    if warm is not None:
        bt.warm_start(*warm)
    bt.solve()
    return bt


def small_batch(ctx, B=1, **st):
    """(a set-up batch of B planted QPs with n = 12, m = 20 and five active rows, not solved yet; their (QP, side, x*, y*))"""
    planted = [R.planted_qp(12, 20, 5, 9950 + b) for b in range(B)]
    return QpalmBatch(ctx, [q[0] for q in planted], ctx.default_settings(**dict(ST, **st))), planted


def snapshot(bt):
    """what a caller can read of the batch's state: the forward path must not see a sensitivity call"""
    x, y = bt.solution()
    infos, stats = bt.infos(), bt.stats_all()
    out = dict(x=x.copy(), y=y.copy())
    for k in ("status_val", "iter", "iter_out"):
        out[k] = np.array([int(getattr(i, k)) for i in infos])
    for k in ("n_refactor", "n_rank1", "n_factor_Q", "n_solve"):
        out[k] = np.array([int(getattr(s, k)) for s in stats])
    return out


def point(bt):
    """the point of the batch's latest solve: (x, y, active) in device memory"""
    x, y = bt.solution_device()
    return x, y, bt.active_device()


def other_data(planted, which, seed):
    """q and bounds planted on the same Q and A with another active set: J1 without its first (which = 0) or its last (which = 1) row"""
    out = []
    for b, (p, side, _, _) in enumerate(planted):
        J = np.flatnonzero(side)
        s2 = side.copy()
        s2[J[0] if which == 0 else J[-1]] = 0
        p2, x2, y2 = R.plant(p.Q_full(), p.A_mat(), s2, seed + b)
        assert np.array_equal(p2.Ax, p.Ax) and np.array_equal(p2.Qx, p.Qx)     # the same matrices: only q and the bounds move
        out.append((p2, s2, x2, y2))
    return out


# ---- the modes every sensitivity call refuses ---------------------------------------------------------------------------------------------------------
REFUSED = ["kkt", "sparse_kkt", "coop", "nonconvex"]
REFUSED_WORD = dict(kkt="dense KKT", sparse_kkt="sparse_kkt", coop="coop", nonconvex="nonconvex")    # what the refusal's message names


@contextlib.contextmanager
def refused_mode(ctx, which):
    """the solved small_batch in one of the REFUSED modes; the context's options are as before afterwards"""
    opts = dict(kkt=(), sparse_kkt=(("sparse_kkt", 1),), coop=(("coop", 1), ("small_workgroups", 0)), nonconvex=())[which]
    st = dict(kkt=dict(factorization_method=0), sparse_kkt=dict(factorization_method=0), coop={}, nonconvex=dict(nonconvex=1))[which]
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        bt, _ = small_batch(ctx, **st)
        bt.solve()
        yield bt
    finally:
        ctx.set_option("sparse_kkt", 0)
        ctx.set_option("small_workgroups", 1)


# ---- the adjoint ----------------------------------------------------------------------------------------------------------------------------------------
def run_adjoint(ctx, bt, gx, gy, sides, **kw):
    out = bt.adjoint_device(T(ctx, gx), None if gy is None else T(ctx, gy), None if sides is None else T(ctx, sides, np.int64), **kw)
    return {k: N(v) for k, v in out.items()}


def adjoint_errors(p, side, gx, gy, out, b):
    """(zr, scale, err64, errk): the reference [u; w_J] at `side`, float64 numpy's error on that system and that of member b of `out`"""
    n, m = p.n, p.m
    zr, z64, J = R.reference(p, side, gx, gy)
    scale = float(np.max(np.abs(zr))) or 1.0
    err64 = float(np.max(np.abs(z64 - zr))) / scale
    w = out["dbmin"][b, :m] + out["dbmax"][b, :m]
    zk = np.concatenate([-out["dq"][b, :n], w[J]])
    return zr, scale, err64, float(np.max(np.abs(zk - zr))) / scale


def judge_adjoint(ctx, what, p, side, x, y, gx, gy, out, b=0, tag="ADJOINT-ACC"):
    """member b of `out` (host arrays) against the reference at the point (x, y, side)"""
    n, m = p.n, p.m
    zr, scale, err64, errk = adjoint_errors(p, side, gx, gy, out, b)
    assert err64 <= 1e-10, "the generator's promise: float64 numpy itself solves K"
    tol = 8.0 * err64
    print("%s | %s | %s | n=%d m=%d |J|=%d | err64 %.2e | kernel %.2e | passes %d | resid %.1e" %
          (tag, ctx.kind, what, n, m, int(np.count_nonzero(side)), err64, errk, int(out["passes"][b]), float(out["resid"][b])))
    assert int(out["flag"][b]) == 0
    assert errk <= tol, (what, errk, err64)
    assert np.array_equal(out["active"][b, :m], side)
    assert np.all(out["dbmin"][b, :m][side >= 0] == 0) and np.all(out["dbmax"][b, :m][side <= 0] == 0)
    # the per-entry gradients are products of [u; w] with the point: the same relative error, times the factors they are multiplied with
    ref = R.gradients(p, side, x.astype(R.LD), y.astype(R.LD), zr)
    ca, cq = np.repeat(np.arange(n), np.diff(p.Ap)), np.repeat(np.arange(n), np.diff(p.Qp))
    fa = np.abs(y[p.Ai]) + np.abs(x[ca]) + 1.0
    fq = np.abs(x[cq]) + np.abs(x[p.Qi]) + 1.0
    for k, f in (("dAx", fa), ("dQx", fq)):
        got, want = out[k][b], ref[k]
        assert np.all(np.abs(got[:len(want)] - want) <= (tol * scale + 4 * U * scale) * f), (what, k)
        assert np.all(got[len(want):] == 0), (what, k)
    for k, width in (("dq", n), ("dbmin", m), ("dbmax", m), ("active", m)):
        assert np.all(out[k][b, width:] == 0), (what, k)


# ---- the tangent ----------------------------------------------------------------------------------------------------------------------------------------
def run_tangent(ctx, bt, d, sides, **kw):
    """d: dict of host arrays [B][...] (absent / None = not passed)"""
    args = {k: (None if d.get(k) is None else T(ctx, d[k])) for k in TR.KEYS}
    out = bt.tangent_device(active=None if sides is None else T(ctx, sides, np.int64), **args, **kw)
    return {k: N(v) for k, v in out.items()}


def batch_direction(bt, dirs):
    """per-member directions (tangent_refs.direction) as the [B][stride] arrays of the call (an input no member has is left out); what lies beyond a
    member's own sizes is NaN: never read"""
    width = dict(dq=bt.n, dbmin=bt.m, dbmax=bt.m, dQx=bt.nnzQ, dAx=bt.nnzA)
    out = {}
    for k in TR.KEYS:
        if all(d.get(k) is None for d in dirs):
            continue
        a = np.full((len(dirs), width[k]), np.nan)
        for b, d in enumerate(dirs):
            a[b, :len(d[k])] = d[k]
        out[k] = a
    return out


def tangent_measure(p, side, x, y, d):
    zr, z64, J = TR.tangent(p, side, x, y, d)
    scale = float(np.max(np.abs(zr))) or 1.0
    err64 = float(np.max(np.abs(z64 - zr))) / scale
    return zr, J, scale, err64


def judge_tangent(ctx, what, p, side, x, y, d, out, b=0, tag="TANGENT-ACC"):
    """member b of `out` (host arrays) against the reference at (x, y, side)"""
    n, m = p.n, p.m
    zr, J, scale, err64 = tangent_measure(p, side, x, y, d)
    assert err64 <= 1e-10, "the generator's promise: float64 numpy itself solves K"
    zk = np.concatenate([out["dx"][b, :n], out["dy"][b, :m][J]])
    errk = float(np.max(np.abs(zk - zr))) / scale
    print("%s | %s | %s | n=%d m=%d |J|=%d | err64 %.2e | kernel %.2e | passes %d | resid %.1e" %
          (tag, ctx.kind, what, n, m, len(J), err64, errk, int(out["passes"][b]), float(out["resid"][b])))
    assert int(out["flag"][b]) == 0
    assert errk <= 8.0 * err64, (what, errk, err64)
    assert np.array_equal(out["active"][b, :m], side)
    assert np.all(out["dy"][b, :m][side == 0] == 0)
    for k, width in (("dx", n), ("dy", m), ("active", m)):
        assert np.all(out[k][b, width:] == 0), (what, k)


# ---- the polish -----------------------------------------------------------------------------------------------------------------------------------------
def run_polish(ctx, bt, sides=None, store=False, **kw):
    out = bt.polish_device(None if sides is None else T(ctx, sides, np.int64), store=store, **kw)
    return {k: N(v) for k, v in out.items()}


def judge_polish(ctx, what, p, side, x, y, out, b=0, improves=True):
    """member b of `out` (host arrays) against the reference at the set `side`; (x, y): the stored solution before the call.  The bound is the judges'
    rule plus the rounding of x + dx (and of its own halves): 8 err64 + 4 u."""
    n, m = p.n, p.m
    zr, z64, J = PR.candidate(p, side)
    scale = float(np.max(np.abs(zr))) or 1.0
    err64 = float(np.max(np.abs(z64 - zr))) / scale
    assert err64 <= 1e-10, "the generator's promise: float64 numpy itself solves K"
    tol = 8.0 * err64 + 4.0 * U
    zk = np.concatenate([out["x"][b, :n], out["y"][b, :m][J]])
    err0 = float(np.max(np.abs(np.concatenate([x, y[J]]) - zr))) / scale
    errk = float(np.max(np.abs(zk - zr))) / scale
    pri_old, dua_old, pri_new, dua_new = (float(v) for v in out["res"][b])
    print("POLISH-ACC | %s | %s | n=%d m=%d |J|=%d | err64 %.2e | stored %.2e | polished %.2e | bound %.2e | passes %d | resid %.1e | pri %.2e -> %.2e | dua %.2e -> %.2e"
          % (ctx.kind, what, n, m, len(J), err64, err0, errk, tol, int(out["passes"][b]), float(out["resid"][b]), pri_old, pri_new, dua_old, dua_new))
    assert int(out["flag"][b]) == 0
    assert errk <= tol, (what, errk, err64)
    if improves:
        assert (pri_new < pri_old) if pri_old > 0 else (pri_new == 0), (pri_old, pri_new)
        assert (dua_new < dua_old) if dua_old > 0 else (dua_new == 0), (dua_old, dua_new)
    assert np.array_equal(out["active"][b, :m], side)
    assert np.all(out["y"][b, :m][side == 0] == 0)
    for k, width in (("x", n), ("y", m), ("active", m)):
        assert np.all(out[k][b, width:] == 0), (what, k)
    return tol, err0

"""The per-step calls on arrays in device memory (qpg_batch_update_bounds_device / _update_q_device / _warm_start_device / _get_solution_device /
_get_status_device) and the one-call step (qpg_batch_step_device).

Yardstick: the same backend's HOST forms, driven with the same values on a twin batch.  Nothing in the arithmetic may differ, so agreement is BIT FOR
BIT (np.array_equal) in x, y, status_val, iter, iter_out, n_refactor, n_rank1 and the active vectors; no tolerance anywhere in this file.

"Device memory" is torch tensors on cuda:0 under [hip] and host memory on the emulator (numpy arrays whose addresses are handed over).

Shapes: the smallest that reach every branch.  [emu] B = 3, n = 12, m = 20.  [hip] B = 700, n = 40, m = 70 with max_slots = 512: more members than the
512-thread instance keeps resident (its solve goes through the work queue), the one-thread-per-member status kernel spans several workgroups, and
m = 70 is no multiple of a workgroup width."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from qpalm_amd import capi
from qpalm_amd.problems import random_qp
from qpalm_amd.solver import QpalmBatch
from tests.helpers import STATUS
from tests.test_mpc_scale import NU, NX, T, _plants, _shift
from tests.test_parity import sizes
from tests.test_update_matrices import assert_same, redraw
from tests.test_update_matrices import snapshot as setup_snapshot

ST = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
INVALID = -2
SMALL = (3, 12, 20)
REFUSED = "Lower bound greater than upper bound"


def shape(ctx):
    return sizes(ctx, SMALL, (700, 40, 70))


_PROBS = {}


def problems(B, n, m, seed=0):
    """B members drawn from eight distinct random QPs (the updates below give every member its own q and bounds)"""
    key = (B, n, m, seed)
    if key not in _PROBS:
        distinct = [random_qp(n, m, seed=7000 + 10 * seed + k, density_A=min(0.5, 4.0 / n), density_M=min(0.3, 2.0 / n)) for k in range(min(B, 8))]
        _PROBS[key] = [distinct[k % len(distinct)] for k in range(B)]
    return _PROBS[key]


class Dev:
    """arrays in the backend's device memory"""

    def __init__(self, ctx):
        self.hip = ctx.kind == "hip"

    def put(self, a, dtype=np.float64):
        a = np.array(a, dtype=dtype, order="C")
        if self.hip:
            import torch
            return torch.from_numpy(a).to("cuda:0")
        return a

    def full(self, shape, value, dtype=np.float64):
        return self.put(np.full(shape, value, dtype=dtype), dtype)

    def arg(self, v):
        """what the QpalmBatch methods take: the tensor itself, or the address of the host array under emulation"""
        if v is None or self.hip:
            return v
        return v.ctypes.data

    def get(self, v):
        return v.cpu().numpy() if self.hip else np.array(v)


def snapshot(bt):
    x, y = bt.solution()
    out = dict(x=x.copy(), y=y.copy())
    infos, stats = bt.infos(), bt.stats_all()
    for k in ("status_val", "iter", "iter_out"):
        out[k] = np.array([int(getattr(i, k)) for i in infos])
    for k in ("n_refactor", "n_rank1"):
        out[k] = np.array([int(getattr(s, k)) for s in stats])
    out["active"] = np.array([bt.ivec("active", b) for b in range(bt.B)])
    return out


def same(H, G, what):
    """the twin driven through the host forms and the batch driven through the device forms"""
    a, b = snapshot(H), snapshot(G)
    bad = [k for k in a if not np.array_equal(a[k], b[k])]
    assert not bad, (what, bad)
    return a


def pair(ctx, probs, **st):
    s = dict(ST, **st)
    H, G = QpalmBatch(ctx, probs, ctx.default_settings(**s)), QpalmBatch(ctx, probs, ctx.default_settings(**s))
    H.solve(); G.solve()
    return H, G


def check_outputs(D, G, ref, out):
    """what the device read-outs wrote against the host forms' snapshot of the twin"""
    for k in ("x", "y", "status_val", "iter"):
        if out.get(k) is not None:
            assert np.array_equal(D.get(out[k]), ref[k]), k


# ---- 1. each single call against its host form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [10, 0])
def test_single_calls_equal_their_host_forms(ctx, scaling):
    D = Dev(ctx)
    B, n, m = shape(ctx)
    H, G = pair(ctx, problems(B, n, m), scaling=scaling)
    ref = same(H, G, "first solve")
    rng = np.random.default_rng(11)
    lo, hi = -rng.random((B, m)), rng.random((B, m))
    x0, y0 = 0.9 * ref["x"] + 0.01, 0.8 * ref["y"]
    cases = [("bounds", lo, hi), ("bounds", 0.5 * lo, None), ("bounds", None, 0.7 * hi), ("q", rng.standard_normal((B, n)), None),
             ("warm", x0, None), ("warm", None, y0), ("warm", x0, y0)]
    for kind, a, b in cases:
        da, db = (None if v is None else D.put(v) for v in (a, b))
        if kind == "bounds":
            assert H.update_bounds(a, b) == 0
            assert G.update_bounds_device(D.arg(da), D.arg(db)) == 0
        elif kind == "q":
            H.update_q(a)
            G.update_q_device(D.arg(da))
        else:
            H.warm_start(a, b)
            G.warm_start_device(D.arg(da), D.arg(db))
        for v, t in ((a, da), (b, db)):      # the caller's arrays are only read
            assert v is None or np.array_equal(D.get(t), v)
        H.solve(); G.solve()
        ref = same(H, G, (kind, a is not None, b is not None))
        assert np.all(ref["status_val"] == STATUS["SOLVED"])
        # the read-outs: into arrays of the caller (filled with something else before), one of the two, and freshly allocated ones
        ox, oy = D.full((B, n), np.nan), D.full((B, m), np.nan)
        G.solution_device(out=(D.arg(ox), D.arg(oy)))
        osv, oit = D.full((B,), -77, np.int64), D.full((B,), -77, np.int64)
        G.status_device(out=(D.arg(osv), D.arg(oit)))
        check_outputs(D, G, ref, dict(x=ox, y=oy, status_val=osv, iter=oit))
    only_y = D.full((B, m), np.nan)
    G.solution_device(out=(None, D.arg(only_y)))
    only_it = D.full((B,), -77, np.int64)
    G.status_device(out=(None, D.arg(only_it)))
    check_outputs(D, G, ref, dict(y=only_y, iter=only_it))
    tx, ty = G.solution_device()          # torch tensors of the wrapper's own (CPU tensors on the emulator)
    tsv, tit = G.status_device()
    got = dict(x=tx, y=ty, status_val=tsv, iter=tit)
    for k, v in got.items():
        assert np.array_equal(v.cpu().numpy(), ref[k]), k
        assert v.device.type == ("cuda" if D.hip else "cpu")


# ---- 2. step_device on every instance of the kernels --------------------------------------------------------------------------------------------
def host_step(H, bmin=None, bmax=None, q=None, warm="last"):
    """the sequence qpg_batch_step_device stands for, through the host forms; the code of the bounds update is ignored in between"""
    rc = 0
    if bmin is not None or bmax is not None:
        rc = H.update_bounds(bmin, bmax)
    if q is not None:
        H.update_q(q)
    if isinstance(warm, str):
        H.warm_start_last()
    elif warm is not None:
        H.warm_start(*warm)
    H.solve()
    return rc


def device_step(D, G, bmin=None, bmax=None, q=None, warm="last", alloc=True):
    """the same through step_device on device arrays; returns (rc, results on the host, the device arrays handed in)"""
    put = lambda v: None if v is None else D.put(v)
    ins = dict(bmin=put(bmin), bmax=put(bmax), q=put(q))
    w = warm if warm is None or isinstance(warm, str) else tuple(put(v) for v in warm)
    wargs = w if w is None or isinstance(w, str) else tuple(D.arg(v) for v in w)
    out = None
    if alloc:
        B, n, m = G.B, G.n, G.m
        keep = dict(x=D.full((B, n), np.nan), y=D.full((B, m), np.nan), status_val=D.full((B,), -77, np.int64), iter=D.full((B,), -77, np.int64),
                    rejected=D.full((B,), -77, np.int64))
        out = {k: D.arg(v) for k, v in keep.items()}
    rc, res = G.step_device(D.arg(ins["bmin"]), D.arg(ins["bmax"]), D.arg(ins["q"]), warm=wargs, out=out)
    if alloc:
        res = keep
    res = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.array(v)) for k, v in res.items()}
    for k, v in (("bmin", bmin), ("bmax", bmax), ("q", q)):
        assert v is None or np.array_equal(D.get(ins[k]), v, equal_nan=True), k
    return rc, res


def step_pair(D, H, G, what, expect_rc=0, rejected=(), **kw):
    rc_h = host_step(H, **kw)
    rc_g, res = device_step(D, G, **kw)
    assert rc_h == rc_g == expect_rc, (what, rc_h, rc_g)
    ref = same(H, G, what)
    for k in ("x", "y", "status_val", "iter"):
        assert np.array_equal(res[k], ref[k]), (what, k)
    want = np.zeros(G.B, dtype=np.int64)
    want[list(rejected)] = 1
    assert np.array_equal(res["rejected"], want), what
    return ref


@pytest.mark.parametrize("inst", ["512", "256", "128", "kkt", "sparse"])
def test_step_device_on_every_kernel_instance(ctx, inst):
    D = Dev(ctx)
    B, n, m = SMALL if inst in ("kkt", "sparse") else shape(ctx)
    st = dict(factorization_method=0) if inst == "kkt" else {}
    try:
        ctx.set_option("small_workgroups", {"512": 0, "128": 2}.get(inst, 1))
        if inst == "sparse":
            ctx.set_option("sparse_factor", 1)
        H, G = pair(ctx, problems(B, n, m, seed=1), **st)
        if ctx.kind == "hip":
            assert G.launch_shape()[1] == {"512": 512, "256": 256, "128": 128, "kkt": 256, "sparse": 512}[inst]
        if inst == "sparse":
            assert G.sparse_info(0)[0] > 0
        same(H, G, "first solve")
        rng = np.random.default_rng(21)
        lo, hi = -rng.random((B, m)), rng.random((B, m))
        ref = step_pair(D, H, G, "bounds + q, warm last", bmin=lo, bmax=hi, q=rng.standard_normal((B, n)), warm="last")
        assert np.all(ref["status_val"] == STATUS["SOLVED"])
        step_pair(D, H, G, "bmax, given warm start", bmax=0.8 * hi, warm=(0.9 * ref["x"], 1.1 * ref["y"]))
        step_pair(D, H, G, "q, warm x only", q=rng.standard_normal((B, n)), warm=(0.5 * ref["x"], None))
        # ... with results the wrapper allocates, and without a warm start (a second solve of finished QPs starts over)
        rc_h = host_step(H, bmin=1.2 * lo, warm=None)
        rc_g, res = device_step(D, G, bmin=1.2 * lo, warm=None, alloc=False)
        ref = same(H, G, "no warm start")
        assert rc_h == rc_g == 0 and not res["rejected"].any()
        for k in ("x", "y", "status_val", "iter"):
            assert np.array_equal(res[k], ref[k]), k
    finally:
        ctx.set_option("small_workgroups", 1)
        ctx.set_option("sparse_factor", -1)


# ---- 3. members smaller than the batch, and no constraints at all -------------------------------------------------------------------------------
def test_sized_members_ignore_and_zero_what_is_beyond_them(ctx):
    D = Dev(ctx)
    B, n, m = shape(ctx)
    dims = [(n, m), (n - 3, m - 5), (n - 1, m), (n, m - 1)]
    distinct = [random_qp(nk, mk, seed=7300 + k, density_A=min(0.5, 4.0 / nk), density_M=min(0.3, 2.0 / nk)) for k, (nk, mk) in enumerate(dims)]
    probs = [distinct[k % len(distinct)] for k in range(B)]
    H, G = pair(ctx, probs)
    assert (G.n, G.m) == (n, m)
    ref = same(H, G, "first solve")
    rng = np.random.default_rng(31)
    in_n = np.array([[j < p.n for j in range(n)] for p in probs])
    in_m = np.array([[i < p.m for i in range(m)] for p in probs])
    assert not ref["x"][~in_n].any() and not ref["y"][~in_m].any()

    def beyond(v, inside):     # (the host twin gets zeros there, the device arrays NaN)
        return np.where(inside, v, 0.0), np.where(inside, v, np.nan)
    lo_h, lo_d = beyond(-rng.random((B, m)), in_m)
    hi_h, hi_d = beyond(rng.random((B, m)), in_m)
    q_h, q_d = beyond(rng.standard_normal((B, n)), in_n)
    x_h, x_d = beyond(0.9 * ref["x"] + 0.01, in_n)
    y_h, y_d = beyond(0.8 * ref["y"], in_m)
    # the single calls
    t = [D.put(v) for v in (lo_d, hi_d, q_d, x_d, y_d)]
    assert H.update_bounds(lo_h, hi_h) == 0 and G.update_bounds_device(D.arg(t[0]), D.arg(t[1])) == 0
    H.update_q(q_h); G.update_q_device(D.arg(t[2]))
    H.warm_start(x_h, y_h); G.warm_start_device(D.arg(t[3]), D.arg(t[4]))
    for v, tv in zip((lo_d, hi_d, q_d, x_d, y_d), t):
        assert np.array_equal(D.get(tv), v, equal_nan=True)
    H.solve(); G.solve()
    ref = same(H, G, "single calls")
    assert np.all(ref["status_val"] == STATUS["SOLVED"])
    ox, oy = D.full((B, n), np.nan), D.full((B, m), np.nan)
    G.solution_device(out=(D.arg(ox), D.arg(oy)))
    gx, gy = D.get(ox), D.get(oy)
    assert np.array_equal(gx, ref["x"]) and np.array_equal(gy, ref["y"])
    assert not gx[~in_n].any() and not gy[~in_m].any() and gx[in_n].any()
    # the whole step (its outputs start as NaN: device_step)
    rc_h = host_step(H, bmin=0.5 * lo_h, bmax=0.5 * hi_h, q=0.5 * q_h, warm=(0.5 * x_h, 0.5 * y_h))
    rc_g, res = device_step(D, G, bmin=0.5 * lo_d, bmax=0.5 * hi_d, q=0.5 * q_d, warm=(0.5 * x_d, 0.5 * y_d))
    ref = same(H, G, "step")
    assert rc_h == rc_g == 0
    assert np.array_equal(res["x"], ref["x"]) and np.array_equal(res["y"], ref["y"]) and not res["x"][~in_n].any() and not res["y"][~in_m].any()
    assert np.array_equal(res["status_val"], ref["status_val"]) and np.array_equal(res["iter"], ref["iter"]) and not res["rejected"].any()


def test_batch_without_constraints(ctx):
    D = Dev(ctx)
    B, n = 3, SMALL[1]
    base = problems(B, n, SMALL[2], seed=2)
    p0 = [dataclasses.replace(p, m=0, Ap=np.zeros(n + 1, dtype=np.int64), Ai=np.zeros(0, dtype=np.int64), Ax=np.zeros(0), bmin=np.zeros(0),
                              bmax=np.zeros(0)) for p in base]
    H, G = pair(ctx, p0)
    ref = same(H, G, "first solve")
    rng = np.random.default_rng(41)
    empty = np.zeros((B, 0))
    step_pair(D, H, G, "m = 0: q and empty bounds", bmin=empty, bmax=empty, q=rng.standard_normal((B, n)), warm=(0.5 * ref["x"], empty))
    q = rng.standard_normal((B, n))
    H.update_q(q); G.update_q_device(D.arg(D.put(q)))
    assert G.update_bounds_device(D.arg(D.put(empty)), D.arg(D.put(empty))) == 0
    H.solve(); G.solve()
    ref = same(H, G, "m = 0: single calls")
    ox = D.full((B, n), np.nan)
    G.solution_device(out=(D.arg(ox), D.arg(D.put(empty))))
    assert np.array_equal(D.get(ox), ref["x"])


# ---- 4. refused bounds --------------------------------------------------------------------------------------------------------------------------
def test_refused_bounds(ctx):
    D = Dev(ctx)
    B, n, m = shape(ctx)
    H, G = pair(ctx, problems(B, n, m, seed=3))
    same(H, G, "first solve")
    rng = np.random.default_rng(51)
    lo, hi = -rng.random((B, m)), rng.random((B, m))
    k1, k2 = B // 2, B - 1
    lo[k1, 3] = hi[k1, 3] + 0.5              # one entry of one member
    dlo, dhi = D.put(lo), D.put(hi)
    assert H.update_bounds(lo, hi) == INVALID
    msg = H.L.qpg_last_error().decode()
    assert G.update_bounds_device(D.arg(dlo), D.arg(dhi)) == INVALID
    assert G.L.qpg_last_error().decode() == msg == REFUSED
    # the refused member reads QPG_ERROR until the next solve, on both; the others what they were
    sv_h = np.array([int(i.status_val) for i in H.infos()])
    assert sv_h[k1] == STATUS["ERROR"] and np.all(np.delete(sv_h, k1) == STATUS["SOLVED"])
    dsv, dit = D.full((B,), -77, np.int64), D.full((B,), -77, np.int64)
    G.status_device(out=(D.arg(dsv), D.arg(dit)))
    assert np.array_equal(D.get(dsv), sv_h) and np.array_equal(D.get(dit), [int(i.iter) for i in H.infos()])
    assert np.array_equal([int(i.status_val) for i in G.infos()], sv_h)
    H.warm_start_last(); G.warm_start_last()
    H.solve(); G.solve()
    ref = same(H, G, "after the refused update")       # (member k1 solved on the bounds it had)
    assert np.all(ref["status_val"] == STATUS["SOLVED"])
    # accepted bounds clear the mark without a solve
    lo[k1, 3] = -0.25
    lo2, hi2 = 0.9 * lo, 0.9 * hi
    lo2[k1, 5] = hi2[k1, 5] + 1.0
    assert H.update_bounds(lo2, hi2) == INVALID and G.update_bounds_device(D.arg(D.put(lo2)), D.arg(D.put(hi2))) == INVALID
    assert H.update_bounds(lo, hi) == 0 and G.update_bounds_device(D.arg(D.put(lo)), D.arg(D.put(hi))) == 0
    G.status_device(out=(D.arg(dsv), None))
    assert np.array_equal(D.get(dsv), [int(i.status_val) for i in H.infos()]) and np.all(D.get(dsv) == STATUS["SOLVED"])
    # the whole step: QPG_ERR_INVALID at the end, every member solved, `rejected` says who kept the old bounds
    lo3, hi3 = 0.8 * lo, 0.8 * hi
    lo3[k2, m - 1] = hi3[k2, m - 1] + 1e-3
    lo3[0, 0] = hi3[0, 0] + 2.0
    ref = step_pair(D, H, G, "step with refused members", expect_rc=INVALID, rejected=(0, k2), bmin=lo3, bmax=hi3, q=rng.standard_normal((B, n)), warm="last")
    assert G.L.qpg_last_error().decode() == REFUSED
    assert np.all(ref["status_val"] == STATUS["SOLVED"])
    step_pair(D, H, G, "a good step after it", bmin=0.7 * lo, bmax=0.7 * hi, warm="last")


# ---- 5. a receding-horizon sequence ---------------------------------------------------------------------------------------------------------------
def test_receding_horizon_sequence(ctx):
    """the mpc-160 plants of tests/test_mpc_scale.py: apply the first input, move the initial-state bounds, warm start, solve.  Under [hip] the new bounds
    are computed in torch on the device and never leave it; the host twin is handed a copy of the same values.  Even steps warm start with "last", odd
    ones with the shifted solution."""
    D = Dev(ctx)
    nb, nsteps = sizes(ctx, (3, 2), (512, 4))
    probs, dyn, rng = _plants(nb, per_plant=max(1, nb // 8))
    n, m = probs[0].n, probs[0].m
    assert (n, m) == (160, 270)
    H, G = pair(ctx, probs)
    ref = same(H, G, "first solve")
    Adyn, Bdyn = np.stack([d[0] for d in dyn]), np.stack([d[1] for d in dyn])
    bmin, bmax = D.put(np.stack([p.bmin for p in probs])), D.put(np.stack([p.bmax for p in probs]))
    x, y = D.put(ref["x"]), D.put(ref["y"])
    sv, it = D.full((nb,), -77, np.int64), D.full((nb,), -77, np.int64)
    if D.hip:
        import torch
        tA, tB = D.put(Adyn), D.put(Bdyn)
    for step in range(nsteps):
        noise = 1e-2 * rng.standard_normal((nb, NX))
        if D.hip:
            u0 = x[:, (T + 1) * NX:(T + 1) * NX + NU]
            x_init = torch.bmm(tA, x[:, :NX, None])[:, :, 0] + torch.bmm(tB, u0[:, :, None])[:, :, 0] + D.put(noise)
        else:
            x_init = np.einsum("bij,bj->bi", Adyn, x[:, :NX]) + np.einsum("bij,bj->bi", Bdyn, x[:, (T + 1) * NX:(T + 1) * NX + NU]) + noise
        bmin[:, :NX] = x_init
        bmax[:, :NX] = x_init
        if step % 2 == 0:
            warm_h, warm_g = "last", "last"
        else:
            xw = np.stack([_shift(xk, dyn[k][0]) for k, xk in enumerate(D.get(x))])
            yw = D.get(y)
            dxw, dyw = D.put(xw), D.put(yw)
            warm_h, warm_g = (xw, yw), (D.arg(dxw), D.arg(dyw))
        rc, _ = G.step_device(D.arg(bmin), D.arg(bmax), warm=warm_g, out=dict(x=D.arg(x), y=D.arg(y), status_val=D.arg(sv), iter=D.arg(it)))
        assert rc == 0
        assert host_step(H, bmin=D.get(bmin), bmax=D.get(bmax), warm=warm_h) == 0
        ref = same(H, G, "step %d" % step)
        assert np.all(ref["status_val"] == STATUS["SOLVED"])
        check_outputs(D, G, ref, dict(x=x, y=y, status_val=sv, iter=it))


# ---- 6. the record of the raw q / bounds that update_Q_A relies on ------------------------------------------------------------------------------------
def full_snapshot(bt):
    out = setup_snapshot(bt)
    out["active"] = np.array([bt.ivec("active", b) for b in range(bt.B)])
    return out


@pytest.mark.parametrize("sequence", ["device updates, update_Q_A", "device, host, device, update_Q_A_device"])
def test_raw_record_survives_device_updates(ctx, sequence):
    """G makes its updates through the device forms, its twin H the same ones through the host forms, and F is a fresh setup on the final values: the
    three are equal bit for bit after the same warm start and solve (what tests/test_update_matrices.py checks for the host forms alone).  One member's
    bounds are refused on the way: its record must keep the bounds it had."""
    D = Dev(ctx)
    B, n, m = shape(ctx)
    P0 = problems(B, n, m, seed=4)
    redrawn = {}
    P1 = [redrawn.setdefault(id(p), redraw(p, 900 + len(redrawn))) for p in P0]
    H, G = pair(ctx, P0)
    ref = same(H, G, "first solve")
    x0, y0 = 0.5 * ref["x"] + 0.01, 0.9 * ref["y"]
    rng = np.random.default_rng(61)
    q1, q2 = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    lo1, hi1, hi3 = -rng.random((B, m)), rng.random((B, m)), 1.0 + rng.random((B, m))
    kbad = 1
    lo1[kbad, 2] = hi1[kbad, 2] + 1.0
    Qx, Ax = G._padded([p.Qx for p in P1], G.nnzQ), G._padded([p.Ax for p in P1], G.nnzA)
    if sequence == "device updates, update_Q_A":
        H.update_q(q1); G.update_q_device(D.arg(D.put(q1)))
        assert H.update_bounds(lo1, hi1) == INVALID and G.update_bounds_device(D.arg(D.put(lo1)), D.arg(D.put(hi1))) == INVALID
        H.update_Q_A(Qx, Ax); G.update_Q_A(Qx, Ax)
        q_f, lo_f, hi_f = q1, lo1.copy(), hi1.copy()
    else:
        H.update_q(q1); G.update_q_device(D.arg(D.put(q1)))
        assert H.update_bounds(lo1, hi1) == INVALID and G.update_bounds_device(D.arg(D.put(lo1)), D.arg(D.put(hi1))) == INVALID
        H.update_q(q2); G.update_q(q2)                                      # the host form on both: G's record comes over from the device
        assert H.update_bounds(None, hi3) == 0 and G.update_bounds_device(None, D.arg(D.put(hi3))) == 0   # ... and goes back
        dQ, dA = D.put(Qx), D.put(Ax)
        H.update_Q_A(Qx, Ax)
        G.update_Q_A_device(*(v.data_ptr() if D.hip else v.ctypes.data for v in (dQ, dA)))
        q_f, lo_f, hi_f = q2, lo1.copy(), hi3.copy()
    lo_f[kbad] = P0[kbad].bmin              # the refused update left this member's bounds alone (the bmax-only one after it is not validated)
    if sequence == "device updates, update_Q_A":
        hi_f[kbad] = P0[kbad].bmax
    F = QpalmBatch(ctx, [dataclasses.replace(p, q=q_f[k], bmin=lo_f[k], bmax=hi_f[k]) for k, p in enumerate(P1)], ctx.default_settings(**ST))
    for bt in (H, G, F):
        assert all(int(i.status_val) == STATUS["UNSOLVED"] and int(i.iter) == 0 for i in bt.infos())
        bt.warm_start(x0, y0)
        bt.solve()
    sh, sg, sf = full_snapshot(H), full_snapshot(G), full_snapshot(F)
    assert_same(sh, sg, "host forms / device forms")
    assert_same(sf, sg, "fresh setup / device forms")
    assert np.all(sg["status_val"] == STATUS["SOLVED"])


# ---- 7. refusals and argument checks ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_argument_checks(ctx):
    import torch
    D = Dev(ctx)
    B, n, m = SMALL
    probs = problems(B, n, m, seed=5)
    L = ctx.L
    err = lambda: L.qpg_last_error().decode()
    buf = D.full((B, max(n, m)), 0.0)
    p = C.c_void_p(D.arg(buf) if not D.hip else buf.data_ptr())
    io = capi.DeviceStep()
    # before qpg_batch_setup
    h = C.c_void_p()
    st = ctx.default_settings(**ST)
    assert L.qpg_batch_create(ctx.h, B, n, m, 10, 10, C.byref(st), C.byref(h)) == 0
    for call in (lambda: L.qpg_batch_update_bounds_device(h, p, p), lambda: L.qpg_batch_update_q_device(h, p), lambda: L.qpg_batch_warm_start_device(h, p, p),
                 lambda: L.qpg_batch_get_solution_device(h, p, p), lambda: L.qpg_batch_get_status_device(h, p, p),
                 lambda: L.qpg_batch_step_device(h, C.byref(io))):
        assert call() == INVALID and "not set up" in err()
    L.qpg_batch_destroy(h)
    H, G = pair(ctx, probs)
    ref = same(H, G, "first solve")
    assert L.qpg_batch_update_q_device(G.h, None) == INVALID and "NULL" in err()
    assert L.qpg_batch_step_device(G.h, None) == INVALID and "NULL" in err()
    io.warm = 2
    assert L.qpg_batch_step_device(G.h, C.byref(io)) == INVALID and "warm" in err()
    io.warm = 3
    assert L.qpg_batch_step_device(G.h, C.byref(io)) == INVALID and "warm" in err()
    # the wrapper's checks: nothing is launched
    dev = "cuda:0" if D.hip else "cpu"
    good = torch.zeros((B, m), dtype=torch.float64, device=dev)
    wrong = [torch.zeros((B, m), dtype=torch.float32, device=dev),                       # dtype
             torch.zeros((B, m + 1), dtype=torch.float64, device=dev),                   # shape
             torch.zeros((B * m,), dtype=torch.float64, device=dev),
             torch.zeros((m, B), dtype=torch.float64, device=dev).t(),                   # contiguity
             torch.zeros((B, m), dtype=torch.float64, device="cpu" if D.hip else "meta"),  # device
             np.zeros((B, m))]                                                           # not a tensor, not an address
    for w in wrong:
        with pytest.raises(ValueError):
            G.update_bounds_device(good, w)
        with pytest.raises(ValueError):
            G.warm_start_device(None, w)
        with pytest.raises(ValueError):
            G.solution_device(out=(None, w))
        with pytest.raises(ValueError):
            G.step_device(bmax=w)
        with pytest.raises(ValueError):
            G.step_device(out=dict(y=w))
    with pytest.raises(ValueError):
        G.update_q_device(torch.zeros((B, n), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        G.update_q_device(None)
    with pytest.raises(ValueError):
        G.status_device(out=(torch.zeros((B,), dtype=torch.int32, device=dev), None))
    with pytest.raises(ValueError):
        G.status_device(out=(None, torch.zeros((B + 1,), dtype=torch.int64, device=dev)))
    with pytest.raises(ValueError):
        G.step_device(warm="first")
    with pytest.raises(ValueError):
        G.step_device(warm=(None, None))
    with pytest.raises(ValueError):
        G.step_device(out=dict(z=good))
    # nothing above touched the batch: it is still the twin of H, and still solves
    assert same(H, G, "after the refusals")["iter"].tolist() == ref["iter"].tolist()
    rng = np.random.default_rng(71)
    step_pair(D, H, G, "a step after the refusals", bmin=-rng.random((B, m)), bmax=rng.random((B, m)), warm="last")

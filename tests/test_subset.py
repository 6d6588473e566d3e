"""Subsets of a batch (qpg_batch_{step,adjoint,tangent,polish}_subset_device / the `select` argument of QpalmBatch and QPLayer); DESIGN.md section 15.

Yardstick: the same backend's own full call.  Members are independent, so a selected member of a subset call must come out BIT FOR BIT (np.array_equal)
as the same member of the full call on a twin batch, and a member that is not selected must not move at all: its state against a snapshot taken before
the call, its rows of the caller's output arrays against a NaN / -7 prefill.  Nothing here has a tolerance.

Shapes: the smallest at which a form changes -- nine (12, 20) members on four slots (the 128-thread instance on the GPU; the full step takes the static
path there and the subset the queue) and on two slots (both through the queue), mixed sizes, one (257, 514) member (the 512-thread instance), the sparse
factor on two slots, the dense KKT panel; the selection kernel at B below, at and above one wavefront, one tile of every instance, and several tiles."""
import ctypes as C

import numpy as np
import pytest
import torch

from qpalm_amd import capi
from qpalm_amd.capi import QpgError
from qpalm_amd.solver import QpalmBatch
from qpalm_amd.torch_layer import QPLayer
from tests import adjoint_refs as R
from tests.sens_helpers import INVALID, UNSUPPORTED, N, T, assert_instance, padded, snapshot
from tests.sparse_gadgets import blocks_qp

ST = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
VECS = ("x", "y", "q", "bmin", "bmax", "sigma")
PATTERNS = ("none", "all", "first", "last", "alternating")
SHAPES = ("B9-slots4", "B9-slots2", "mixed", "n257", "sparse", "kkt")


def pattern(name, B):
    s = np.zeros(B, np.int64)
    if name == "all":
        s[:] = 1
    elif name == "first":
        s[0] = 1
    elif name == "last":
        s[-1] = 1
    elif name == "alternating":
        s[::2] = 1
    return s


class Twin:
    """a shape of the list above: its problems, settings, context options and the warm start of the first solve; make() builds one solved batch"""

    def __init__(self, ctx, shape):
        self.ctx, self.shape, self.opts, self.st, self.warm, self.threads = ctx, shape, {}, dict(ST, scaling=10), None, 128
        if shape in ("B9-slots4", "B9-slots2"):
            self.opts = dict(max_slots=4 if shape == "B9-slots4" else 2)
            self.probs = [R.planted_qp(12, 20, 2 + k % 6, 9500 + 11 * k)[0] for k in range(9)]
        elif shape == "mixed":
            self.probs = [R.planted_qp(n, m, k, 9500 + 11 * b)[0] for b, (n, m, k) in enumerate([(33, 50, 20), (20, 30, 7), (5, 8, 3)])]
            self.threads = 256
        elif shape == "n257":     # the big member starts at its planted solution: the emulator spends its time on the step, not on the first solve
            planted = [R.planted_qp(257, 514, 256, 9000 + 7 * 257 + 256, equality=True), R.planted_qp(12, 20, 5, 9901)]
            self.probs = [q[0] for q in planted]
            self.warm = (padded([q[2] for q in planted], 257), padded([q[3] for q in planted], 514))
            self.st, self.threads = dict(ST, scaling=0, proximal=1), 512
        elif shape == "sparse":
            self.opts = dict(max_slots=2, sparse_factor=1)
            self.probs = [R.replant(blocks_qp(43, 2)[0], 10, 60 + b)[0] for b in range(3)]
            self.threads = 512
        elif shape == "kkt":
            self.probs = [R.planted_qp(12, 20, 5, 9900 + b)[0] for b in range(3)]
            self.st, self.threads = dict(ST, scaling=10, factorization_method=0), 256
        self.B = len(self.probs)

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)
        return self

    def __exit__(self, *exc):
        self.ctx.set_option("sparse_factor", -1)
        self.ctx.set_option("max_slots", 512)

    def make(self, **st):
        bt = QpalmBatch(self.ctx, self.probs, self.ctx.default_settings(**dict(self.st, **st)))
        if self.warm is not None:
            bt.warm_start(*self.warm)
        bt.solve()
        return bt

    def q2(self, bt, scale=0.05):
        rng = np.random.default_rng(4)
        return padded([p.q for p in self.probs], bt.n) + scale * padded([rng.standard_normal(p.n) for p in self.probs], bt.n)


def state(bt):
    """snapshot() of tests/sens_helpers.py plus the vectors of every member a caller can read"""
    out = snapshot(bt)
    for k in VECS:
        out["vec_" + k] = np.array([bt.vec(k, b) for b in range(bt.B)])
    return out


def prefilled(ctx, bt):
    return dict(x=T(ctx, np.full((bt.B, bt.n), np.nan)), y=T(ctx, np.full((bt.B, bt.m), np.nan)), status_val=T(ctx, np.full(bt.B, -7), np.int64),
                iter=T(ctx, np.full(bt.B, -7), np.int64), rejected=T(ctx, np.full(bt.B, -7), np.int64))


def assert_prefill(out, rows):
    """rows (a boolean mask) of every output array still hold the prefill: NaN in float arrays, -7 in integer ones"""
    for k, v in out.items():
        if not hasattr(v, "cpu"):
            continue
        a = N(v)[rows]
        assert np.all(np.isnan(a)) if a.dtype.kind == "f" else np.all(a == -7), k


def assert_rows(a, b, rows, what):
    bad = [k for k in a if not np.array_equal(a[k][rows], b[k][rows])]
    assert not bad, (what, bad)


_FULL = {}


def full_step(ctx, tw, w):
    """the twin's full step, once per (backend, shape, warm): its state afterwards and its outputs on the host"""
    key = (ctx.kind, tw.shape, w)
    if key not in _FULL:
        H = tw.make()
        assert_instance(ctx, H, tw.threads)
        rc, out = H.step_device(q=T(ctx, tw.q2(H)), warm=w)
        assert rc == 0
        _FULL[key] = (state(H), {k: N(v) for k, v in out.items()})
    return _FULL[key]


# ---- 1. selected rows equal a full step, the others do not move ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [None, "last"], ids=["cold", "last"])
@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_selected_rows_equal_a_full_step(ctx, shape, pat, w):
    with Twin(ctx, shape) as tw:
        h, hout = full_step(ctx, tw, w)
        G = tw.make()
        assert_instance(ctx, G, tw.threads)
        slots = G.launch_shape()[0]
        if shape in ("B9-slots2", "sparse"):
            assert G.B > slots                                 # the full step goes through the work queue as well
        elif ctx.kind == "hip":
            assert G.B <= slots                                # the full step took the static path, the subset takes the queue
        s = pattern(pat, G.B)
        sel = s.astype(bool)
        before, epoch = state(G), G.epoch
        out = prefilled(ctx, G)
        rc, got = G.step_device(q=T(ctx, tw.q2(G)), warm=w, out=out, select=T(ctx, s, np.int64))
        assert rc == 0 and got["n_selected"] == int(s.sum()) and G.epoch == epoch + 1
        after = state(G)
        assert_rows(after, h, sel, "selected members against the full step")
        assert_rows(after, before, ~sel, "members that were not selected against their own state before")
        assert_prefill(out, ~sel)
        for k in ("x", "y", "status_val", "iter"):
            assert np.array_equal(N(out[k])[sel], hout[k][sel]), k
        assert np.all(N(out["rejected"])[sel] == 0)
        if pat == "none":
            assert got["n_selected"] == 0 and all(np.array_equal(before[k], after[k]) for k in before)
        if pat == "all":
            assert all(np.array_equal(h[k], after[k]) for k in h)
        assert np.all(after["status_val"][sel] == 1)


# ---- 2. a subset and then its complement equal one full step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [None, "last"], ids=["cold", "last"])
@pytest.mark.parametrize("shape", ["B9-slots2", "mixed"])
def test_subset_then_complement_is_one_full_step(ctx, shape, w):
    with Twin(ctx, shape) as tw:
        h, hout = full_step(ctx, tw, w)
        G = tw.make()
        s = pattern("alternating", G.B)
        out = prefilled(ctx, G)
        for part in (s, 1 - s):
            rc, got = G.step_device(q=T(ctx, tw.q2(G)), warm=w, out=out, select=T(ctx, part, np.int64))
            assert rc == 0 and got["n_selected"] == int(part.sum())
        g = state(G)
        bad = [k for k in h if not np.array_equal(h[k], g[k])]
        assert not bad, bad
        for k in ("x", "y", "status_val", "iter"):
            assert np.array_equal(N(out[k]), hout[k]), k


# ---- 3. the selection kernel at its edges -------------------------------------------------------------------------------------------------------
def tiny_problems(B):
    return [R.planted_qp(2, 2, b % 3, 7000 + b) for b in range(B)]


def tiny_batch(ctx, planted, members, first):
    """the listed members of `planted` (n = m = 2) as a batch; first = "unequal": a first solve in which the odd members start at their planted solution
    and the even ones cold, so the solves differ in length and the queue's order is not the index order; "none": no solve yet (every cost is zero)"""
    bt = QpalmBatch(ctx, [planted[b][0] for b in members], ctx.default_settings(**dict(ST, scaling=2)))
    if first == "unequal":
        wx, wy = np.array([planted[b][2] for b in members]), np.array([planted[b][3] for b in members])
        cold = np.array(members) % 2 == 0
        wx[cold], wy[cold] = 0.0, 0.0
        bt.warm_start(wx, wy)
        bt.solve()
    return bt


@pytest.mark.parametrize("which", ["random", "last-only"])
@pytest.mark.parametrize("B,first", [(1, "none"), (63, "none"), (64, "none"), (65, "none"), (65, "unequal"), (127, "none"), (128, "none"), (129, "none"),
                                     (513, "none")])
def test_selection_kernel_edges(ctx, B, first, which):
    """The yardstick of a selected member is the same member in a twin batch made of the selected members alone, taken through the same calls in full
    (members are independent: the same bits in any batch).  The random select picks about eight members wherever they fall, so that a case costs a
    handful of solves whatever B; the members that are not selected have never been solved when first = "none": n_solve = 0 before, and after."""
    planted = tiny_problems(B)
    rng = np.random.default_rng(B)
    if which == "random":
        s = (rng.random(B) < min(0.5, 8.0 / B)).astype(np.int64)
        s[rng.integers(B)] = 1
    else:
        s = np.zeros(B, np.int64)
        s[-1] = 1
    sel = s.astype(bool)
    members = np.flatnonzero(s).tolist()
    q2 = np.array([p[0].q for p in planted]) + 0.05 * np.random.default_rng(5).standard_normal((B, 2))
    H, G = tiny_batch(ctx, planted, members, first), tiny_batch(ctx, planted, range(B), first)
    if first == "unequal":
        it = snapshot(G)["iter"]
        assert it[1::2].max() < it[::2].min()                   # the first solves did differ in length
    rc, _ = H.step_device(q=T(ctx, q2[sel]), warm="last")
    assert rc == 0
    h = snapshot(H)
    before = dict(snapshot(G), ms_total=np.array([float(v.ms_total) for v in G.stats_all()]))
    out = prefilled(ctx, G)
    rc, got = G.step_device(q=T(ctx, q2), warm="last", out=out, select=T(ctx, s, np.int64))
    assert rc == 0 and got["n_selected"] == int(s.sum()) == len(members)
    after = dict(snapshot(G), ms_total=np.array([float(v.ms_total) for v in G.stats_all()]))
    for k in h:                                                 # iter, x and everything else of the snapshot
        assert np.array_equal(after[k][sel], h[k]), k
    assert np.all(h["status_val"] == 1) and np.all(h["n_solve"] >= 1)
    assert np.array_equal(N(out["x"])[sel], h["x"]) and np.array_equal(N(out["iter"])[sel], h["iter"])
    assert_rows(after, before, ~sel, "members that were not selected")                       # n_solve and the kernel time among them: none was solved
    assert_prefill(out, ~sel)


# ---- 4. the record of the raw q and bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_first", [False, True], ids=["device-record", "host-record-current"])
def test_raw_record_keeps_both_kinds_of_rows(ctx, host_first):
    """a masked update of q and bounds through a subset step, then update_Q_A_device with the original values: bit for bit a fresh batch set up with the
    mixed q / bounds (the comparison of tests/test_update_matrices.py).  host_first: the host forms of update_q / update_bounds ran before, so the
    current record is the host's when the subset step comes (raw_cur == 0) and has to come over whole."""
    import dataclasses
    B, n, m = 3, 12, 20
    probs = [R.planted_qp(n, m, 5, 9900 + b)[0] for b in range(B)]
    rng = np.random.default_rng(8)
    G = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    G.solve()
    base = probs
    if host_first:
        base = [dataclasses.replace(p, q=p.q + 0.02 * rng.standard_normal(n), bmin=p.bmin - 0.125, bmax=p.bmax + 0.25) for p in probs]
        G.update_q(np.array([p.q for p in base]))
        assert G.update_bounds(np.array([p.bmin for p in base]), np.array([p.bmax for p in base])) == 0
    new = [dataclasses.replace(p, q=p.q + 0.05 * rng.standard_normal(n), bmin=p.bmin - 0.5, bmax=p.bmax + 0.5) for p in base]
    s = np.array([1, 0, 1], np.int64)
    arr = lambda k: T(ctx, np.array([getattr(p, k) for p in new]))
    rc, got = G.step_device(arr("bmin"), arr("bmax"), arr("q"), warm="last", select=T(ctx, s, np.int64))
    assert rc == 0 and got["n_selected"] == 2
    Qx, Ax = T(ctx, padded([p.Qx for p in probs], G.nnzQ)), T(ctx, padded([p.Ax for p in probs], G.nnzA))
    G.update_Q_A_device(Qx.data_ptr(), Ax.data_ptr())
    G.solve()
    mixed = [new[b] if s[b] else base[b] for b in range(B)]
    F = QpalmBatch(ctx, mixed, ctx.default_settings(**dict(ST, scaling=10)))
    F.solve()
    f, g = state(F), state(G)
    for bt, d in ((F, f), (G, g)):
        d["D"] = np.array([bt.vec("D", b) for b in range(B)])
        d["E"] = np.array([bt.vec("E", b) for b in range(B)])
        d["sc_c"] = np.array([float(v.sc_c) for v in bt.stats_all()])
        d["n_sweeps"] = np.array([int(v.n_sweeps) for v in bt.stats_all()])
    bad = [k for k in f if not np.array_equal(f[k], g[k])]
    assert not bad, bad
    assert np.all(f["status_val"] == 1)


# ---- 5. bounds ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_is_selected", [True, False])
def test_refused_bounds(ctx, bad_is_selected):
    with Twin(ctx, "B9-slots2") as tw:
        H, G = tw.make(), tw.make()
        lo, hi = padded([p.bmin - 0.5 for p in tw.probs], G.m), padded([p.bmax + 0.5 for p in tw.probs], G.m)
        rc, _ = H.step_device(T(ctx, lo), T(ctx, hi), T(ctx, tw.q2(H)), warm="last")           # the twin: valid bounds everywhere ...
        assert rc == 0
        K = tw.make()                                                                          # ... and, for the refused member, its old bounds
        rc, _ = K.step_device(q=T(ctx, tw.q2(K)), warm="last")
        assert rc == 0
        h, k = state(H), state(K)
        s = pattern("alternating", G.B)
        bad = 2 if bad_is_selected else 3
        lo[bad, 4], hi[bad, 4] = 1.0, -1.0
        before = state(G)
        out = prefilled(ctx, G)
        rc, got = G.step_device(T(ctx, lo), T(ctx, hi), T(ctx, tw.q2(G)), warm="last", out=out, select=T(ctx, s, np.int64))
        g, rej = state(G), N(out["rejected"])
        sel = s.astype(bool)
        assert_rows(g, before, ~sel, "members that were not selected")
        assert_prefill(out, ~sel)
        if bad_is_selected:
            assert rc == INVALID and b"Lower bound" in G.L.qpg_last_error()
            assert rej[bad] == 1 and np.all(np.delete(rej[sel], 1) == 0)
            assert_rows(g, k, np.arange(G.B) == bad, "the refused member: solved on its old bounds")
            assert np.array_equal(N(out["x"])[bad], k["x"][bad]) and int(N(out["status_val"])[bad]) == 1
            sel[bad] = False
        else:
            assert rc == 0 and rej[bad] == -7 and np.all(rej[sel] == 0)
        assert_rows(g, h, sel, "the other selected members: the new bounds")


# ---- 6. invalid and refused calls ---------------------------------------------------------------------------------------------------------------
def test_invalid_calls(ctx):
    with Twin(ctx, "B9-slots2") as tw:
        G = tw.make()
        gx = T(ctx, np.ones((G.B, G.n)))
        calls = dict(step=lambda s: G.step_device(q=T(ctx, tw.q2(G)), select=s), adjoint=lambda s: G.adjoint_device(gx, select=s),
                     tangent=lambda s: G.tangent_device(dq=gx, select=s), polish=lambda s: G.polish_device(store=True, select=s))
        before = state(G)
        for value in (2, -1):
            s = pattern("alternating", G.B)
            s[5] = value
            for name, call in calls.items():
                with pytest.raises(QpgError) as e:
                    call(T(ctx, s, np.int64))
                assert e.value.code == INVALID and "select" in str(e.value), name
        good = pattern("alternating", G.B)
        for name, call in calls.items():
            for wrong in (T(ctx, good, np.int32), T(ctx, good[:-1], np.int64), good, 5):
                with pytest.raises(ValueError):
                    call(wrong)
            if ctx.kind == "hip":
                with pytest.raises(ValueError):
                    call(T(ctx, good, np.int64).cpu())
        after = state(G)
        assert all(np.array_equal(before[k], after[k]) for k in before)
        io = capi.DeviceStep()                                   # the arguments of the full call are checked in the subset form too
        io.warm = 3
        cnt = capi.c_int(-1)
        sel = T(ctx, good, np.int64)
        assert G.L.qpg_batch_step_subset_device(G.h, C.byref(io), C.c_void_p(sel.data_ptr()), C.byref(cnt)) == INVALID
        io.warm = 0                                              # select = NULL: the full call; n_selected may be NULL
        assert G.L.qpg_batch_step_subset_device(G.h, C.byref(io), None, C.byref(cnt)) == 0 and cnt.value == G.B
        assert G.L.qpg_batch_step_subset_device(G.h, C.byref(io), C.c_void_p(sel.data_ptr()), None) == 0
        rc, got = G.step_device(q=T(ctx, tw.q2(G)), select=sel)  # ... and the batch still works
        assert rc == 0 and got["n_selected"] == 5


def test_a_solve_in_progress_is_refused(ctx):
    probs = [R.planted_qp(12, 20, 5, 9950 + b)[0] for b in range(2)]
    G = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, eps_abs=1e-9, eps_rel=1e-9)))
    G.iterate(1)
    s = T(ctx, np.array([1, 0]), np.int64)
    before = state(G)
    for call in (lambda: G.step_device(select=s), lambda: G.adjoint_device(T(ctx, np.ones((2, 12))), select=s), lambda: G.polish_device(select=s)):
        with pytest.raises(QpgError) as e:
            call()
        assert e.value.code == INVALID and "in progress" in str(e.value)
    after = state(G)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    G.solve()
    rc, got = G.step_device(select=s)
    assert rc == 0 and got["n_selected"] == 1


def test_coop_and_kkt_refusals(ctx):
    probs = [R.planted_qp(12, 20, 5, 9950)[0]]
    s = T(ctx, np.array([1]), np.int64)
    ctx.set_option("coop", 1)
    ctx.set_option("small_workgroups", 0)
    try:
        G = QpalmBatch(ctx, probs, ctx.default_settings(**ST))
        G.solve()
        with pytest.raises(QpgError) as e:
            G.step_device(select=s)
        assert e.value.code == UNSUPPORTED and "coop" in str(e.value)
    finally:
        ctx.set_option("coop", 0)
        ctx.set_option("small_workgroups", 1)
    G = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, factorization_method=0)))
    G.solve()
    gx = T(ctx, np.ones((1, 12)))
    for call in (lambda: G.adjoint_device(gx, select=s), lambda: G.tangent_device(dq=gx, select=s), lambda: G.polish_device(select=s)):
        with pytest.raises(QpgError) as e:
            call()
        assert e.value.code == UNSUPPORTED and "dense KKT" in str(e.value)


# ---- 7. sensitivities ---------------------------------------------------------------------------------------------------------------------------
SENS = {"adjoint": dict(dq=np.float64, dbmin=np.float64, dbmax=np.float64, dQx=np.float64, dAx=np.float64, active=np.int64, flag=np.int64,
                        resid=np.float64, passes=np.int64),
        "tangent": dict(dx=np.float64, dy=np.float64, active=np.int64, flag=np.int64, resid=np.float64, passes=np.int64),
        "polish": dict(x=np.float64, y=np.float64, res=np.float64, active=np.int64, flag=np.int64, resid=np.float64, passes=np.int64)}


def sens_call(ctx, bt, mode, store, select=None):
    """one sensitivity call into prefilled outputs (NaN / -7); returns them on the host"""
    rng = np.random.default_rng(11)
    nB, n, m = bt.B, bt.n, bt.m
    shp = dict(dq=(nB, n), dx=(nB, n), x=(nB, n), dbmin=(nB, m), dbmax=(nB, m), dy=(nB, m), y=(nB, m), active=(nB, m), dQx=(nB, bt.nnzQ),
               dAx=(nB, bt.nnzA), res=(nB, 4), flag=(nB,), resid=(nB,), passes=(nB,))
    out = {k: T(ctx, np.full(shp[k], np.nan if dt is np.float64 else -7), dt) for k, dt in SENS[mode].items()}
    sel = None if select is None else T(ctx, select, np.int64)
    gx, gy = T(ctx, rng.standard_normal((nB, n))), T(ctx, rng.standard_normal((nB, m)))
    if mode == "adjoint":
        got = bt.adjoint_device(gx, gy, out=out, select=sel)
    elif mode == "tangent":
        got = bt.tangent_device(dq=gx, dbmin=gy, dbmax=gy, out=out, select=sel)
    else:
        got = bt.polish_device(store=store, out=out, select=sel)
    assert (select is None) or got["n_selected"] == int(np.sum(select))
    return {k: N(v) for k, v in out.items() if k != "n_selected"}


@pytest.mark.parametrize("mode,store", [("adjoint", False), ("tangent", False), ("polish", False), ("polish", True)],
                         ids=["adjoint", "tangent", "polish", "polish-store"])
@pytest.mark.parametrize("shape", ["B9-slots4", "B9-slots2", "sparse"])
def test_sensitivities_of_a_subset(ctx, shape, mode, store):
    loose = dict(eps_abs=1e-3, eps_rel=1e-3)                    # a visibly inexact stored solution: the polish has something to store
    with Twin(ctx, shape) as tw:
        H, G, K = tw.make(**loose), tw.make(**loose), tw.make(**loose)      # H: the full call; G: the subset; K: no call at all
        s = pattern("alternating", G.B)
        sel = s.astype(bool)
        full = sens_call(ctx, H, mode, store)
        before, epoch = state(G), G.epoch
        part = sens_call(ctx, G, mode, store, s)
        for k in full:
            assert np.array_equal(part[k][sel], full[k][sel]), k
            a = part[k][~sel]
            assert np.all(np.isnan(a)) if a.dtype.kind == "f" else np.all(a == -7), k
        after = state(G)
        moved = sel & (full["flag"] == 0) if store else np.zeros(G.B, bool)
        assert_rows(after, before, ~moved, "members the call may not change")
        if store:
            assert moved.any() and G.epoch == epoch + 1
            assert np.array_equal(after["x"][moved], full["x"][moved]) and np.array_equal(after["y"][moved], full["y"][moved])
            assert not np.array_equal(after["x"][moved], before["x"][moved])
            assert all(np.array_equal(after[k], before[k]) for k in before if k not in ("x", "y"))
        else:
            assert G.epoch == epoch
        q2 = T(ctx, tw.q2(G))
        for bt in (H, G, K):                                    # a following full step: a selected member as after the full call, the others as if
            rc, _ = bt.step_device(q=q2, warm="last")           # nothing had been called
            assert rc == 0
        h, g, k = state(H), state(G), state(K)
        assert_rows(g, h, sel, "selected members after the next step")
        assert_rows(g, k, ~sel, "the other members after the next step")
        if not store:
            assert all(np.array_equal(h[key], k[key]) for key in h)


# ---- 8. the torch layer -------------------------------------------------------------------------------------------------------------------------
def test_layer_steps_and_differentiates_a_subset(ctx):
    n, m, B = 12, 20, 4
    probs = [R.planted_qp(n, m, 5, 9980 + b)[0] for b in range(B)]
    st = ctx.default_settings(**dict(ST, eps_abs=1e-9, eps_rel=1e-9, scaling=10))
    H, G = QpalmBatch(ctx, probs, st), QpalmBatch(ctx, probs, st)
    H.solve(); G.solve()
    x0, y0 = G.solution()
    rng = np.random.default_rng(3)
    qn = np.array([p.q for p in probs]) + 0.05 * rng.standard_normal((B, n))
    cx, cy = T(ctx, rng.standard_normal((B, n))), T(ctx, rng.standard_normal((B, m)))
    s = np.array([0, 1, 1, 0], np.int64)
    sel = s.astype(bool)
    qh, qg = T(ctx, qn).requires_grad_(True), T(ctx, qn).requires_grad_(True)
    lh, lg = QPLayer(H, warm="last"), QPLayer(G, warm="last")
    xh, yh, _ = lh(qh)
    ((cx * xh).sum() + (cy * yh).sum()).backward()
    xg, yg, status = lg(qg, select=T(ctx, s, np.int64))
    assert N(status).tolist() == [1] * B
    assert np.array_equal(N(xg)[~sel], x0[~sel]) and np.array_equal(N(yg)[~sel], y0[~sel])      # the stored solutions from before
    assert np.array_equal(N(xg)[sel], N(xh)[sel]) and np.array_equal(N(yg)[sel], N(yh)[sel])
    ((cx * xg).sum() + (cy * yg).sum()).backward()
    assert np.all(N(qg.grad)[~sel] == 0)
    assert np.array_equal(N(qg.grad)[sel], N(qh.grad)[sel]) and np.any(N(qg.grad)[sel] != 0)
    assert np.all(N(lg.last_adjoint["flag"])[sel] == 0)
    with pytest.raises(ValueError):
        lg(qg, Qx=T(ctx, padded([p.Qx for p in probs], G.nnzQ)), Ax=T(ctx, padded([p.Ax for p in probs], G.nnzA)), select=T(ctx, s, np.int64))

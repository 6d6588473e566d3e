"""The adjoint of a solved batch (qpg_batch_adjoint_device / QpalmBatch.adjoint_device / qpalm_amd.torch_layer).

Reference: at a fixed active set J the gradients are ONE linear solve K [u; w] = [gx; gy_J], K = [[Q, A_J'], [A_J, 0]] on the problem's own (unscaled) data,
done in numpy.longdouble (rational arithmetic where the system has at most 14 unknowns), tests/adjoint_refs.py.  The engine supplies x and y and is
handed the same J, so the arithmetic is judged apart from the active-set rule; the rule has cases of its own against a numpy restatement.

Tolerance: nothing fixed in advance.  Per case err64 = max |z_numpy - z_ref| / max |z_ref| of float64 numpy.linalg.solve on the same K is measured, and the
kernel's error, measured the same way, must stay within 8 x err64.
Measured figures (both backends): profiles/adjoint/accuracy.md.

Sizes: n on the edges of the 32- and 64-column blocks and of the hand-over between the 128-, 256- and 512-thread instances, m about n / 2 and 2 n,
|J| = 0, 1, mixed sides and all-equality n - 1, scaling 0 / 10, proximal 0 / 1.  Problems are planted strictly complementary (asserted on the returned
solution).  The members with n >= 192 are warm-started at the planted solution: the emulator then spends its time on the adjoint, not on the solve."""
import dataclasses

import numpy as np
import pytest
import torch

from qpalm_amd.capi import QpgError
from qpalm_amd.solver import QpalmBatch
from qpalm_amd.torch_layer import QPLayer
from tests import adjoint_refs as R
from tests.sens_helpers import (CASES, INVALID, REFUSED, REFUSED_WORD, ST, UNSUPPORTED, N, T, assert_complementary, assert_instance, padded, refused_mode,
                                run_adjoint, small_batch, snapshot, solved)
from tests.sens_helpers import judge_adjoint as judge
from tests.sparse_gadgets import blocks_qp, gadget_qp


# ---- 1. the arithmetic at a given active set, every size -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gradients_match_the_reference_solve(ctx, case):
    p, side, xs, ys = R.planted_qp(case.n, case.m, case.nact, 9000 + 7 * case.n + case.nact, sides=case.sides, equality=case.equality)
    warm = (xs[None, :], ys[None, :]) if case.n >= 192 else None
    bt = solved(ctx, [p], warm=warm, scaling=case.scaling, proximal=case.proximal)
    assert int(bt.info(0).status_val) == 1
    assert_instance(ctx, bt, 256 if case.n <= 256 else 512)
    x, y = bt.solution_of(0)
    assert_complementary(p, side, x, y)
    rng = np.random.default_rng(case.n)
    gx, gy = rng.standard_normal((1, case.n)), (rng.standard_normal((1, case.m)) if case.gy else None)
    out = run_adjoint(ctx, bt, gx, gy, side[None, :])
    judge(ctx, case.id, p, side, x, y, gx[0], None if gy is None else gy[0], out)


# ---- 2. batches: mixed sizes; nine members on four slots, B > 2 max_slots: the 128-thread instance on the GPU, once with a member at its edge n = 192;
#         more members than slots (the work queue) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["mixed", "B9-slots4", "B9-slots4-n192", "B9-slots2"])
def test_batches(ctx, shape):
    if shape == "mixed":
        dims = [(33, 50, 20), (20, 30, 7), (5, 8, 3)]
    else:
        ctx.set_option("max_slots", 2 if shape == "B9-slots2" else 4)
        dims = [(12, 20, 2 + k % 6) for k in range(9)]
        if shape == "B9-slots4-n192":
            dims[4] = (192, 96, 60)
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate(dims)]
    probs = [q[0] for q in planted]
    # (the batch with the large member starts at the planted solutions, like the large single cases)
    warm = (padded([q[2] for q in planted], 192), padded([q[3] for q in planted], 96)) if shape == "B9-slots4-n192" else None
    bt = solved(ctx, probs, warm=warm, scaling=10)
    assert_instance(ctx, bt, 256 if shape == "mixed" else 128)
    nmax, mmax = bt.n, bt.m
    rng = np.random.default_rng(5)
    gx, gy = rng.standard_normal((bt.B, nmax)), rng.standard_normal((bt.B, mmax))
    sides = padded([q[1] for q in planted], mmax, np.int64)
    out = run_adjoint(ctx, bt, gx, gy, sides)
    if shape == "B9-slots2":
        assert bt.B > bt.launch_shape()[0]                    # more members than factor slots: the work queue
    elif ctx.kind == "hip":
        assert bt.B <= bt.launch_shape()[0]                   # (the emulator's one instance keeps fewer slots)
    for b, (p, side, _, _) in enumerate(planted):
        assert int(bt.info(b).status_val) == 1
        x, y = bt.solution_of(b)
        assert_complementary(p, side, x, y)
        judge(ctx, "%s[%d]" % (shape, b), p, side, x, y, gx[b, :p.n], gy[b, :p.m], out, b)


# ---- 2b. the caller's order of the entries: Q with both triangles, unsorted columns of Q and A (update_Q_A's maps, inverted) -----------------------
def test_entries_in_the_callers_order(ctx):
    base, side, _, _ = R.planted_qp(12, 20, 5, 9600)
    same, _, _, _ = R.planted_qp(12, 20, 4, 9601)
    p = R.shuffled_entries(base, 3)
    assert np.any(p.Qi < np.repeat(np.arange(12), np.diff(p.Qp))) and np.any(np.diff(p.Ai)[np.diff(np.repeat(np.arange(12), np.diff(p.Ap))) == 0] < 0)
    probs = [p, same]                                          # member 1 in the engine's own order: no map for it, the "same order" flag
    sides = np.array([side, R.planted_qp(12, 20, 4, 9601)[1]])
    bt = solved(ctx, probs, scaling=10)
    assert bt.nnzQ == len(p.Qx) > len(base.Qx)
    rng = np.random.default_rng(6)
    gx, gy = rng.standard_normal((2, 12)), rng.standard_normal((2, 20))
    out = run_adjoint(ctx, bt, gx, gy, sides)
    for b, q in enumerate(probs):
        x, y = bt.solution_of(b)
        assert_complementary(q, sides[b], x, y)
        judge(ctx, "order[%d]" % b, q, sides[b], x, y, gx[b], gy[b], out, b)    # dQx / dAx position by position in q's own arrays
    upper = p.Qi < np.repeat(np.arange(12), np.diff(p.Qp))
    assert np.all(out["dQx"][0][:len(p.Qx)][upper] == 0) and np.any(out["dQx"][0][:len(p.Qx)][~upper] != 0)
    # ... and they are the gradients of the values update_Q_A takes: the round trip through it leaves the solution where it was
    bt.update_Q_A([q.Qx for q in probs], [q.Ax for q in probs])
    bt.solve()
    again = run_adjoint(ctx, bt, gx, gy, sides)
    for k in ("dQx", "dAx"):
        assert np.allclose(again[k], out[k], rtol=0, atol=1e-6), k


# ---- 3. the sparse Schur instance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blocks", "banded"])
def test_sparse_factor_instance(ctx, kind):
    if kind == "blocks":
        base, _ = blocks_qp(43, 2)
    else:
        base, _ = gadget_qp((), 4105, 5, cliques=False, stars=False, arrow=False, single=False, band=12)
    p, side, _, _ = R.replant(base, min(base.n - 1, base.m) // 2, 77)
    ctx.set_option("sparse_factor", 1)
    try:
        bt = solved(ctx, [p], scaling=10)
        assert bt.sparse_info(0)[0] > 0
        x, y = bt.solution_of(0)
        assert int(bt.info(0).status_val) == 1
        assert_complementary(p, side, x, y)
        rng = np.random.default_rng(3)
        gx, gy = rng.standard_normal((1, p.n)), rng.standard_normal((1, p.m))
        out = run_adjoint(ctx, bt, gx, gy, side[None, :])
        judge(ctx, "sparse-" + kind, p, side, x, y, gx[0], gy[0], out)
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 4. the default active-set rule against its numpy restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [0, 10])
def test_default_rule(ctx, scaling):
    planted = [R.planted_qp(33, 50, 20, 9700), R.planted_qp(33, 50, 12, 9701, equality=True)]
    probs = [q[0] for q in planted]
    bt = solved(ctx, probs, scaling=scaling)
    rng = np.random.default_rng(8)
    gx, gy = rng.standard_normal((2, 33)), rng.standard_normal((2, 50))
    out = run_adjoint(ctx, bt, gx, gy, None)
    given = run_adjoint(ctx, bt, gx, gy, np.array([q[1] for q in planted]))
    for b, (p, side, _, _) in enumerate(planted):
        x, y = bt.solution_of(b)
        assert_complementary(p, side, x, y)
        rule = R.default_rule(bt, p, b)
        assert np.array_equal(rule, side)                    # strictly complementary: every rule finds the planted set
        assert np.array_equal(out["active"][b], rule)
    for k in out:                                            # the same set, found or handed in: the same arithmetic
        assert np.array_equal(out[k], given[k]), k


# ---- 5. finite differences ------------------------------------------------------------------------------------------------------------------------
def test_directional_derivative_against_central_differences(ctx):
    n, m, h = 33, 50, 1e-3
    p, side, _, _ = R.planted_qp(n, m, 20, 9800)
    rng = np.random.default_rng(12)
    dq, dlo, dhi = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    gx = rng.standard_normal((1, n))
    st = dict(eps_abs=1e-10, eps_rel=1e-10, scaling=10)
    J = np.flatnonzero(side)
    K = R.kkt_dense(p, J)
    ell, delta = [], 0.0
    for s in (+1.0, -1.0):
        ps = dataclasses.replace(p, q=p.q + s * h * dq, bmin=p.bmin + s * h * dlo, bmax=p.bmax + s * h * dhi)
        bt = solved(ctx, [ps], **st)
        x, _ = bt.solution_of(0)
        assert np.array_equal(run_adjoint(ctx, bt, gx, None, None, want=("active",))["active"][0], side)   # J unchanged
        z = np.linalg.solve(K, np.concatenate([-ps.q, np.where(side < 0, ps.bmin, ps.bmax)[J]]))
        delta = max(delta, float(np.max(np.abs(x - z[:n]))))
        ell.append(float(gx[0] @ x))
    bt = solved(ctx, [p], **st)
    out = run_adjoint(ctx, bt, gx, None, None)
    assert np.array_equal(out["active"][0], side) and int(out["flag"][0]) == 0
    got = float(out["dq"][0] @ dq + out["dbmin"][0] @ dlo + out["dbmax"][0] @ dhi)
    fd = (ell[0] - ell[1]) / (2 * h)
    bound = 4 * delta * float(np.sum(np.abs(gx))) / h
    print("ADJOINT-FD | %s | adjoint %.12e | central difference %.12e | delta %.2e | bound %.2e" % (ctx.kind, got, fd, delta, bound))
    assert abs(got - fd) <= bound


# ---- 6. the forward path does not see the adjoint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,slots,warm", [("dense", 3, 512, "last"), ("dense", 5, 1, None), ("sparse", 2, 512, None), ("sparse", 3, 2, "last")])
def test_next_step_is_bit_identical(ctx, mode, B, slots, warm):
    ctx.set_option("max_slots", slots)
    if mode == "sparse":
        ctx.set_option("sparse_factor", 1)
    try:
        if mode == "sparse":
            probs = [R.replant(blocks_qp(43, 2)[0], 10, 60 + b)[0] for b in range(B)]
        else:
            probs = [R.planted_qp(12, 20, 5, 9900 + b)[0] for b in range(B)]
        st = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
        H, G = (QpalmBatch(ctx, probs, ctx.default_settings(**st)) for _ in range(2))
        H.solve(); G.solve()
        assert (B > G.launch_shape()[0]) == (slots != 512)        # more members than factor slots: the work queue
        rng = np.random.default_rng(4)
        before = snapshot(G)
        out = run_adjoint(ctx, G, rng.standard_normal((B, G.n)), rng.standard_normal((B, G.m)), None)
        assert np.all(out["flag"] == 0)
        after = snapshot(G)
        assert all(np.array_equal(before[k], after[k]) for k in before)       # nothing the caller can read has moved
        q2 = T(ctx, np.array([p.q for p in probs]) + 0.05 * rng.standard_normal((B, G.n)))
        for bt in (H, G):
            rc, _ = bt.step_device(q=q2, warm=warm)
            assert rc == 0
        a, b = snapshot(H), snapshot(G)
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not bad, bad
        assert np.all(a["status_val"] == 1)
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 7. refusals and flags ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", REFUSED)
def test_unsupported_modes_are_refused(ctx, which):
    with refused_mode(ctx, which) as bt:
        with pytest.raises(QpgError) as e:
            bt.adjoint_device(T(ctx, np.ones((1, 12))))
        assert e.value.code == UNSUPPORTED
        assert REFUSED_WORD[which] in str(e.value)


def test_invalid_calls(ctx):
    bt, _ = small_batch(ctx, B=2)
    gx = T(ctx, np.ones((2, 12)))
    bt.iterate(1)                                            # a solve in progress
    with pytest.raises(QpgError) as e:
        bt.adjoint_device(gx)
    assert e.value.code == INVALID and "in progress" in str(e.value)
    bt.solve()
    with pytest.raises(ValueError):
        bt.adjoint_device(None)
    from qpalm_amd import capi
    import ctypes as C
    io = capi.DeviceAdjoint()                                # gx = NULL at the C ABI
    assert bt.L.qpg_batch_adjoint_device(bt.h, C.byref(io)) == INVALID
    bad = np.zeros((2, 20), np.int64)
    bad[1, 19] = 2
    with pytest.raises(QpgError) as e:
        bt.adjoint_device(gx, active=T(ctx, bad, np.int64))
    assert e.value.code == INVALID
    # wrong device, dtype or shape: ValueError before anything is launched
    with pytest.raises(ValueError):
        bt.adjoint_device(gx.to(torch.float32))
    with pytest.raises(ValueError):
        bt.adjoint_device(T(ctx, np.ones((2, 13))))
    with pytest.raises(ValueError):
        bt.adjoint_device(gx, gy=T(ctx, np.ones((2, 20)), np.float32))
    with pytest.raises(ValueError):
        bt.adjoint_device(gx, active=T(ctx, np.zeros((2, 20)), np.int32))
    with pytest.raises(ValueError):
        bt.adjoint_device(gx, out=dict(dq=T(ctx, np.zeros((2, 11)))))
    with pytest.raises(ValueError):
        bt.adjoint_device(gx, want=("dq", "nonsense"))
    if ctx.kind == "hip":
        with pytest.raises(ValueError):
            bt.adjoint_device(gx.cpu())
    out = bt.adjoint_device(gx)                              # ... and the batch still works
    assert np.all(N(out["flag"]) == 0)


def test_unsolved_member_gets_flag_2_and_its_neighbours_are_right(ctx):
    """max_iter = 1: members 0 and 2 start at their planted solutions and end SOLVED at once, member 1 starts cold and ends at MAX_ITER"""
    planted = [R.planted_qp(12, 20, 5, 9960 + b) for b in range(3)]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10, max_iter=1)))
    wx, wy = np.array([q[2] for q in planted]), np.array([q[3] for q in planted])
    wx[1], wy[1] = 0.0, 0.0
    bt.warm_start(wx, wy)
    bt.solve()
    assert bt.statuses().tolist() == [1, -2, 1]
    gx, gy = np.ones((3, 12)), np.ones((3, 20))
    out = run_adjoint(ctx, bt, gx, gy, np.array([q[1] for q in planted]))
    assert out["flag"].tolist() == [0, 2, 0]
    for k in ("dq", "dbmin", "dbmax", "dQx", "dAx", "active", "resid", "passes"):
        assert np.all(out[k][1] == 0), k
    for b in (0, 2):
        p, side, _, _ = planted[b]
        x, y = bt.solution_of(b)
        assert_complementary(p, side, x, y)
        judge(ctx, "neighbour[%d]" % b, p, side, x, y, gx[b], gy[b], out, b)


def test_dependent_active_rows(ctx):
    """two identical rows, both handed in as active: K is singular.  With different gy on the two rows the system has no solution: the refinement cannot
    converge, flag 1, zero outputs.  With gy = None it is consistent and the refinement converges to the unique u (flag 0)."""
    p, side, _, _ = R.planted_qp(12, 20, 5, 9970)
    A = p.A_mat().tolil()
    i0 = int(np.flatnonzero(side)[0])
    i1 = int(np.flatnonzero(side == 0)[0])
    A[i1, :] = A[i0, :]
    A = A.tocsc(); A.sort_indices()
    x = np.linalg.solve(p.Q_full().toarray(), -p.q)
    ax = A @ x
    p2 = dataclasses.replace(p, Ap=A.indptr.astype(np.int64), Ai=A.indices.astype(np.int64), Ax=A.data.copy(), bmin=ax - 1.0, bmax=ax + 1.0)
    bt = solved(ctx, [p2], scaling=10)
    assert int(bt.info(0).status_val) == 1
    sides = np.zeros((1, 20), np.int64)
    sides[0, i0], sides[0, i1] = -1, -1
    gx, gy = np.ones((1, 12)), np.zeros((1, 20))
    gy[0, i0], gy[0, i1] = 1.0, -1.0
    out = run_adjoint(ctx, bt, gx, gy, sides)
    assert int(out["flag"][0]) == 1 and int(out["passes"][0]) == 200
    for k in ("dq", "dbmin", "dbmax", "dQx", "dAx"):
        assert np.all(out[k] == 0), k
    assert np.array_equal(out["active"], sides) and np.isfinite(out["resid"][0])
    # consistent (gy = None): the refinement converges.  u is unique -- that of the system with one of the two rows left out -- and w_i0 + w_i1 is that
    # system's w_i0; how the sum is split between the two rows is not determined (the penalties weigh it)
    out = run_adjoint(ctx, bt, gx, None, sides)
    assert int(out["flag"][0]) == 0
    assert all(np.all(np.isfinite(v)) for v in out.values())
    one = np.zeros(20, int)
    one[i0] = -1
    zr, z64, _ = R.reference(p2, one, gx[0], None)
    scale = float(np.max(np.abs(zr)))
    err64 = float(np.max(np.abs(z64 - zr))) / scale
    zk = np.concatenate([-out["dq"][0], [out["dbmin"][0, i0] + out["dbmin"][0, i1]]])
    errk = float(np.max(np.abs(zk - zr))) / scale
    print("ADJOINT-ACC | %s | dependent-rows | n=12 m=20 |J|=2 | err64 %.2e | kernel %.2e | passes %d | resid %.1e" %
          (ctx.kind, err64, errk, int(out["passes"][0]), float(out["resid"][0])))
    assert errk <= 8 * err64


# ---- 8. the torch layer ---------------------------------------------------------------------------------------------------------------------------
def test_torch_layer(ctx):
    n, m = 33, 50
    planted = [R.planted_qp(n, m, 20, 9980), R.planted_qp(n, m, 9, 9981)]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    leaf = lambda a: T(ctx, a).requires_grad_(True)
    q, lo, hi = leaf([p.q for p in probs]), leaf([p.bmin for p in probs]), leaf([p.bmax for p in probs])
    Qx, Ax = leaf(padded([p.Qx for p in probs], bt.nnzQ)), leaf(padded([p.Ax for p in probs], bt.nnzA))
    layer = QPLayer(bt)
    x, y, status = layer(q, lo, hi, Qx=Qx, Ax=Ax)
    assert N(status).tolist() == [1, 1] and not status.requires_grad
    rng = np.random.default_rng(21)
    cx, cy = T(ctx, rng.standard_normal((2, n))), T(ctx, rng.standard_normal((2, m)))
    ((cx * x).sum() + (cy * y).sum()).backward()
    own = bt.adjoint_device(cx, cy)
    for t, k in ((q, "dq"), (lo, "dbmin"), (hi, "dbmax"), (Qx, "dQx"), (Ax, "dAx")):
        assert torch.equal(t.grad, own[k]), k                                  # bit for bit the call's own outputs
    assert N(layer.last_adjoint["flag"]).tolist() == [0, 0]
    out = {k: N(v) for k, v in own.items()}
    for b, (p, side, _, _) in enumerate(planted):
        xb, yb = bt.solution_of(b)
        assert np.array_equal(N(x)[b], xb) and np.array_equal(N(y)[b], yb)
        assert_complementary(p, side, xb, yb)
        judge(ctx, "layer[%d]" % b, p, side, xb, yb, N(cx)[b], N(cy)[b], out, b)
    # only what needs a gradient is computed; inputs left out stay as they are
    q2 = leaf([p.q for p in probs])
    x2, _, _ = layer(q2)
    x2.sum().backward()
    assert q2.grad is not None and q2.grad.shape == q2.shape and torch.allclose(x2, x, rtol=0, atol=1e-7)
    # a backward pass after the batch has moved on would differentiate another solve: refused
    q3 = leaf([p.q for p in probs])
    x3, _, _ = layer(q3)
    bt.solve()
    with pytest.raises(RuntimeError):
        x3.sum().backward()

"""Sensitivities for K directions per call (qpg_batch_adjoint_multi_device, qpg_batch_tangent_multi_device / QpalmBatch.adjoints_device, tangents_device,
jacobian_device).

A member's K directions run one after another on the factor its set-up left, each with the arithmetic of the single call, so the checks of the two
multi calls are bit equality with calls the project already ships (adjoint_device / tangent_device, their subset forms and their forms at a recorded
point): no tolerance enters.  "Bit for bit" is taken literally: the arrays' bytes are compared (a -0.0 is not a 0.0).

The Jacobian has a reference of its own: column j of dx/dq is -(K^-1)[:n, j] and column i of dx/dbmin is (K^-1)[:n, n + pos(i)] for a lower-active
row i (zero for every other row), K = [[Q, A_J'], [A_J, 0]], solved by tests/adjoint_refs.py (exact in rationals below 14 unknowns, numpy.longdouble
elimination above).  Each column (tangent mode) or row (adjoint mode) is ONE solve and is judged by the rule of tests/test_adjoint.py: per solve
err64 = max |z_numpy - z_ref| / max |z_ref| of float64 numpy.linalg.solve on the same K and right-hand side is measured, and the kernel's error on
the entries of that solve the Jacobian holds, measured against the same scale, must stay within 8 x err64.  One addition, which random right-hand
sides never needed: a unit right-hand side on a variable that Q and A_J couple to nothing has a solution that is a float64 exactly, numpy returns
it and err64 = 0.  The engine solves the SCALED system -- c D g going in, D u~ coming out, a rounding each -- so no bound below one unit roundoff
U = 2^-53 can hold for it whatever the solve does: err64 counts as max(err64, U).  The two modes are compared entry by entry by the duality rule of
tests/test_tangent.py with g = e_i and the direction e_j, both of 1-norm 1: 8 x (err64_j scale_j + err64_i scale_i).

Sizes: those of tests/test_adjoint.py at which these kernels change form -- n = 5, 65 (more than one 64-column block), 193 (256-thread instance on
the GPU), 257 (512-thread instance), the sparse factor, nine members on two factor slots (a workgroup runs several members' K directions in turn), a
batch of mixed sizes.  Members with n >= 192 are warm-started at the planted solution."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from qpalm_amd import capi
from qpalm_amd.capi import QpgError
from qpalm_amd.solver import QpalmBatch
from tests import adjoint_refs as R
from tests.sens_helpers import (INVALID, REFUSED, REFUSED_WORD, ST, UNSUPPORTED, N, T, assert_complementary, assert_instance, host, other_data, padded, point,
                                refused_mode, small_batch, snapshot, solved)
from tests.sparse_gadgets import blocks_qp

ADJ_KEYS = ("dq", "dbmin", "dbmax", "dQx", "dAx", "active", "flag", "resid", "passes")
TAN_KEYS = ("dx", "dy", "active", "flag", "resid", "passes")
TAN_IN = ("dq", "dbmin", "dbmax", "dQx", "dAx")
SHARED = ("active",)          # written once per call: not per direction
FLOORS = (0.0, 1e6)
U = 2.0 ** -53


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def widths(bt):
    return dict(gx=bt.n, gy=bt.m, dq=bt.n, dbmin=bt.m, dbmax=bt.m, dQx=bt.nnzQ, dAx=bt.nnzA)


def own_sizes(p):
    return dict(gx=p.n, gy=p.m, dq=p.n, dbmin=p.m, dbmax=p.m, dQx=len(p.Qx), dAx=len(p.Ax))


def directions(bt, probs, keys, K, seed):
    """{key: [K][B][stride]}: direction 0 carries every input, direction 1 is all zeros, direction 2 the first key (gx / dq) only, any further one
    every input again.  What lies beyond a member's own sizes is NaN in the directions that are not all zeros: never read."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in keys:
        a = np.zeros((K, bt.B, widths(bt)[key]))
        for k in range(K):
            if k == 1 or (k == 2 and key != keys[0]):
                continue
            a[k] = np.nan
            for b, p in enumerate(probs):
                size = own_sizes(p)[key]
                a[k, b, :size] = rng.standard_normal(size)
        out[key] = a
    return out


def multi_and_singles(ctx, bt, which, d, K, sides=None, **kw):
    """(the multi call's outputs, [the single call's outputs for slice k]) on the same state, host arrays"""
    act = None if sides is None else T(ctx, sides, np.int64)
    dev_d = {k: T(ctx, v) for k, v in d.items()}
    if which == "adjoint":
        multi = host(bt.adjoints_device(dev_d["gx"], dev_d["gy"], active=act, **kw))
        singles = [host(bt.adjoint_device(T(ctx, d["gx"][k]), T(ctx, d["gy"][k]), active=act, **kw)) for k in range(K)]
    else:
        multi = host(bt.tangents_device(**dev_d, active=act, **kw))
        singles = [host(bt.tangent_device(**{key: T(ctx, v[k]) for key, v in d.items()}, active=act, **kw)) for k in range(K)]
    return multi, singles


def assert_slices(what, multi, singles, keys):
    for k, one in enumerate(singles):
        for key in keys:
            got = multi[key] if key in SHARED else multi[key][k]
            assert np.array_equal(got, one[key]) and same_bits(got, one[key]), (what, "direction %d" % k, key)


def check_both(ctx, what, bt, probs, K, sides=None, floors=FLOORS, **kw):
    """the two multi calls against the single calls, with the floor at 0 and at 1e6; returns the last outputs (adjoint, tangent)"""
    last = None
    for floor in floors:
        bt.sens_penalty = floor
        epoch = bt.epoch
        da = directions(bt, probs, ("gx", "gy"), K, 41)
        ma, sa = multi_and_singles(ctx, bt, "adjoint", da, K, sides, **kw)
        assert_slices("%s adjoint floor %g" % (what, floor), ma, sa, ADJ_KEYS)
        dt = directions(bt, probs, TAN_IN, K, 43)
        mt, st = multi_and_singles(ctx, bt, "tangent", dt, K, sides, **kw)
        assert_slices("%s tangent floor %g" % (what, floor), mt, st, TAN_KEYS)
        assert bt.epoch == epoch
        if K >= 3:   # a NULL array is a zero one: direction 2 has gx / dq only
            one = host(bt.adjoint_device(T(ctx, da["gx"][2]), None, active=None if sides is None else T(ctx, sides, np.int64), **kw))
            assert all(same_bits(ma[k] if k in SHARED else ma[k][2], one[k]) for k in ADJ_KEYS)
            one = host(bt.tangent_device(dq=T(ctx, dt["dq"][2]), active=None if sides is None else T(ctx, sides, np.int64), **kw))
            assert all(same_bits(mt[k] if k in SHARED else mt[k][2], one[k]) for k in TAN_KEYS)
            # ... and the directions differ: slice 0 is not slice 2, and the all-zero direction gives zeros
            assert not np.array_equal(ma["dq"][0], ma["dq"][2]) and not np.array_equal(mt["dx"][0], mt["dx"][2])
            assert np.all(ma["dq"][1] == 0) and np.all(mt["dx"][1] == 0) and np.all(mt["dy"][1] == 0)
        last = (ma, mt)
    bt.sens_penalty = 0.0
    return last


# ---- 1. slice k is the single call, bit for bit ----------------------------------------------------------------------------------------------------
SHAPES = ["n5-m8-J3", "n5-m8-J3-K1", "n65-m32-J20", "n193-m386-J90", "n257-m514", "sparse-blocks", "B9-slots2", "mixed"]


@pytest.mark.parametrize("shape", SHAPES)
def test_slice_k_is_the_single_call(ctx, shape):
    K = 1 if shape.endswith("K1") else 3
    try:
        if shape in ("B9-slots2", "mixed"):
            if shape == "B9-slots2":
                ctx.set_option("max_slots", 2)
                dims = [(12, 20, 2 + k % 6) for k in range(9)]
            else:
                dims = [(33, 50, 20), (20, 30, 7), (5, 8, 3)]
            planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate(dims)]
            bt = solved(ctx, [q[0] for q in planted], scaling=10)
            assert_instance(ctx, bt, 128 if shape == "B9-slots2" else 256)
            if shape == "B9-slots2":
                assert bt.B > bt.launch_shape()[0]                    # more members than factor slots: a workgroup takes several members in turn
        elif shape == "sparse-blocks":
            ctx.set_option("sparse_factor", 1)
            base = blocks_qp(43, 2)[0]
            planted = [R.replant(base, min(base.n - 1, base.m) // 2, 77)]
            bt = solved(ctx, [planted[0][0]], scaling=10)
            assert bt.sparse_info(0)[0] > 0
        else:
            n, m, nact, scaling, proximal, equality = {"n5-m8-J3": (5, 8, 3, 10, 1, False), "n5-m8-J3-K1": (5, 8, 3, 10, 1, False),
                                                       "n65-m32-J20": (65, 32, 20, 10, 0, False), "n193-m386-J90": (193, 386, 90, 10, 1, False),
                                                       "n257-m514": (257, 514, 256, 0, 1, True)}[shape]
            planted = [R.planted_qp(n, m, nact, 9000 + 7 * n + nact, equality=equality)]
            warm = (planted[0][2][None, :], planted[0][3][None, :]) if n >= 192 else None
            bt = solved(ctx, [planted[0][0]], warm=warm, scaling=scaling, proximal=proximal)
            assert_instance(ctx, bt, 256 if n <= 256 else 512)
        assert bt.statuses().tolist() == [1] * bt.B
        probs = [q[0] for q in planted]
        for b, (p, side, _, _) in enumerate(planted):
            x, y = bt.solution_of(b)
            assert_complementary(p, side, x, y)
        sides = padded([q[1] for q in planted], bt.m, np.int64)
        ma, mt = check_both(ctx, shape, bt, probs, K, sides)
        assert np.all(ma["flag"] == 0) and np.all(mt["flag"] == 0)
        assert ma["flag"].shape == (K, bt.B) and ma["active"].shape == (bt.B, bt.m) and mt["dx"].shape == (K, bt.B, bt.n)
        for b, p in enumerate(probs):   # entries beyond a member's own n / m are zero in every slice
            for out, key, width in ((ma, "dq", p.n), (ma, "dbmin", p.m), (ma, "dbmax", p.m), (mt, "dx", p.n), (mt, "dy", p.m), (ma, "dQx", len(p.Qx)),
                                    (ma, "dAx", len(p.Ax))):
                assert np.all(out[key][:, b, width:] == 0), (shape, key)
        if shape == "mixed":
            assert any(p.n < bt.n for p in probs) and any(p.m < bt.m for p in probs)
            check_both(ctx, shape + " rule", bt, probs, K, None, floors=(0.0,))          # ... and with the engine's own rule for J
    finally:
        ctx.set_option("sparse_factor", -1)


# ---- 2. a failing direction stays alone --------------------------------------------------------------------------------------------------------------
def test_a_failing_direction_stays_alone(ctx):
    """the member of test_adjoint.test_dependent_active_rows: two identical rows, both active, K singular.  gy differs on them in direction 1 (no
    solution: the pass cap) and is equal on them in directions 0 and 2 (consistent: the refinement converges)"""
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
    rng = np.random.default_rng(2)
    gx, gy = rng.standard_normal((3, 1, 12)), np.zeros((3, 1, 20))
    gy[0, 0, i0] = gy[0, 0, i1] = 0.75
    gy[1, 0, i0], gy[1, 0, i1] = 1.0, -1.0
    multi, singles = multi_and_singles(ctx, bt, "adjoint", dict(gx=gx, gy=gy), 3, sides)
    assert multi["flag"][:, 0].tolist() == [0, 1, 0] and int(multi["passes"][1, 0]) == 200
    for k in ("dq", "dbmin", "dbmax", "dQx", "dAx"):
        assert np.all(multi[k][1] == 0), k
        if k != "dbmax":   # (both active rows are lower ones)
            assert np.any(multi[k][0] != 0) and np.any(multi[k][2] != 0), k
    assert np.array_equal(multi["active"], sides) and np.isfinite(multi["resid"][1, 0])
    assert_slices("dependent rows", multi, singles, ADJ_KEYS)


# ---- 3. a member that is not solved --------------------------------------------------------------------------------------------------------------------
def test_an_unsolved_member_is_flagged_in_every_slice(ctx):
    """max_iter = 1: members 0 and 2 start at their planted solutions and end SOLVED at once, member 1 starts cold and ends at MAX_ITER"""
    planted = [R.planted_qp(12, 20, 5, 9960 + b) for b in range(3)]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10, max_iter=1)))
    wx, wy = np.array([q[2] for q in planted]), np.array([q[3] for q in planted])
    wx[1], wy[1] = 0.0, 0.0
    bt.warm_start(wx, wy)
    bt.solve()
    assert bt.statuses().tolist() == [1, -2, 1]
    ma, mt = check_both(ctx, "one-unsolved", bt, probs, 3, np.array([q[1] for q in planted]))
    for out, keys in ((ma, ADJ_KEYS), (mt, TAN_KEYS)):
        assert out["flag"].tolist() == [[0, 2, 0]] * 3
        for k in keys:
            if k != "flag":
                assert np.all((out[k][1] if k in SHARED else out[k][:, 1]) == 0), k
    assert np.any(ma["dq"][0, 0] != 0) and np.any(mt["dx"][0, 2] != 0)


# ---- 4. state: the forward path does not see the multi calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,slots,warm", [("dense", 5, 1, None), ("sparse", 3, 2, "last")])
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
        assert B > G.launch_shape()[0]                              # more members than factor slots: the work queue
        rng = np.random.default_rng(4)
        before = snapshot(G)
        epoch = G.epoch
        tan = host(G.tangents_device(dq=T(ctx, rng.standard_normal((3, B, G.n))), dAx=T(ctx, rng.standard_normal((3, B, G.nnzA)))))
        adj = host(G.adjoints_device(T(ctx, rng.standard_normal((3, B, G.n))), T(ctx, rng.standard_normal((3, B, G.m)))))
        assert np.all(tan["flag"] == 0) and np.all(adj["flag"] == 0) and G.epoch == epoch
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


# ---- 5. a subset, and a recorded point ------------------------------------------------------------------------------------------------------------------
def test_subset(ctx):
    ctx.set_option("max_slots", 2)
    planted = [R.planted_qp(12, 20, 2 + k % 6, 9500 + 11 * k) for k in range(9)]
    probs = [q[0] for q in planted]
    bt = solved(ctx, probs, scaling=10)
    K = 3
    sel = np.array([1, 0, 0, 1, 0, 1, 0, 0, 1])
    mark = lambda ref: {k: torch.full_like(T(ctx, v, v.dtype), 7) for k, v in ref.items()}
    da, dt = directions(bt, probs, ("gx", "gy"), K, 51), directions(bt, probs, TAN_IN, K, 53)
    full = host(bt.adjoints_device(T(ctx, da["gx"]), T(ctx, da["gy"])))
    full_t = host(bt.tangents_device(**{k: T(ctx, v) for k, v in dt.items()}))
    sub = bt.adjoints_device(T(ctx, da["gx"]), T(ctx, da["gy"]), out=mark(full), select=T(ctx, sel, np.int64))
    sub_t = bt.tangents_device(**{k: T(ctx, v) for k, v in dt.items()}, out=mark(full_t), select=T(ctx, sel, np.int64))
    assert sub["n_selected"] == 4 and sub_t["n_selected"] == 4
    for ref, got, keys in ((full, host(sub), ADJ_KEYS), (full_t, host(sub_t), TAN_KEYS)):
        for k in keys:
            rows = (lambda a, s: a[s]) if k in SHARED else (lambda a, s: a[:, s])
            assert same_bits(rows(got[k], sel == 1), rows(ref[k], sel == 1)), k
            assert np.all(rows(got[k], sel == 0) == 7), k                  # every slice of every output, flag included
    # ... and the selected rows are the single subset calls'
    one = host(bt.adjoint_device(T(ctx, da["gx"][0]), T(ctx, da["gy"][0]), select=T(ctx, sel, np.int64)))
    assert same_bits(one["dq"][sel == 1], full["dq"][0][sel == 1])
    none = bt.adjoints_device(T(ctx, da["gx"]), T(ctx, da["gy"]), out=mark(full), select=T(ctx, np.zeros(9), np.int64))
    assert none["n_selected"] == 0 and all(np.all(N(none[k]) == 7) for k in ADJ_KEYS)


def test_at_a_recorded_point(ctx):
    """the set-up of test_sens_at.test_an_earlier_solve: the point of the first of three solves, whose active set no later solve has"""
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate([(33, 50, 20), (20, 30, 7), (5, 8, 3)])]
    probs = [q[0] for q in planted]
    bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, scaling=10)))
    bt.solve()
    P1 = point(bt)
    for which in (0, 1):
        nxt = other_data(planted, which, 700 + 10 * which)
        bt.update_q_device(T(ctx, padded([q[0].q for q in nxt], bt.n)))
        assert bt.update_bounds_device(T(ctx, padded([q[0].bmin for q in nxt], bt.m)), T(ctx, padded([q[0].bmax for q in nxt], bt.m))) == 0
        rc, _ = bt.step_device(warm="last")
        assert rc == 0 and bt.statuses().tolist() == [1, 1, 1]
    assert not np.array_equal(N(bt.active_device()), N(P1[2]))
    ma, mt = check_both(ctx, "at P1", bt, probs, 3, None, at=P1)
    assert np.all(ma["flag"] == 0) and np.all(mt["flag"] == 0) and np.array_equal(ma["active"], N(P1[2]))
    now = host(bt.adjoints_device(T(ctx, directions(bt, probs, ("gx", "gy"), 3, 41)["gx"])))
    assert not np.array_equal(now["dq"][0], ma["dq"][0])              # the stored solutions would not do: the check discriminates
    # a point that is not finite inside member 1: flag 1 and zeros in all K slices, as the single call at that point gives them
    xb = N(P1[0]).copy()
    xb[1, 3] = np.nan
    ma, mt = check_both(ctx, "at a NaN", bt, probs, 3, None, floors=(0.0,), at=(T(ctx, xb), P1[1], P1[2]))
    assert ma["flag"].tolist() == [[0, 1, 0]] * 3 and mt["flag"].tolist() == [[0, 1, 0]] * 3
    assert np.all(ma["dq"][:, 1] == 0) and np.all(mt["dx"][:, 1] == 0)


# ---- 6. the Jacobian ------------------------------------------------------------------------------------------------------------------------------------
def unit_solves(p, side):
    """per unit right-hand side of K(J) z = e_r, r < n + |J|: (z_ref longdouble, scale, err64 of float64 numpy.linalg.solve, at least U)"""
    n, J = p.n, np.flatnonzero(side)
    out = []
    for r in range(n + len(J)):
        gx, gy = np.zeros(n), np.zeros(p.m)
        if r < n:
            gx[r] = 1.0
        else:
            gy[J[r - n]] = 1.0
        zr, z64, _ = R.reference(p, side, gx, gy)
        scale = float(np.max(np.abs(zr)))
        out.append((zr, scale, max(float(np.max(np.abs(z64 - zr))) / scale, U)))   # (U: see the module's docstring)
    return out


@pytest.mark.parametrize("n,m,nact", [(5, 8, 3), (33, 16, 1)])
def test_jacobian(ctx, n, m, nact):
    p, side, _, _ = R.planted_qp(n, m, nact, 9000 + 7 * n + nact)
    bt = solved(ctx, [p], scaling=10)
    x, y = bt.solution_of(0)
    assert_complementary(p, side, x, y)
    act = T(ctx, side[None, :], np.int64)
    J = np.flatnonzero(side)
    ref = unit_solves(p, side)
    assert all(e <= 1e-10 for _, _, e in ref), "the generator's promise: float64 numpy itself solves K"
    epoch = bt.epoch
    tq, aq = host(bt.jacobian_device("q", active=act)), host(bt.jacobian_device("q", mode="adjoint", active=act))
    tb, ab = host(bt.jacobian_device("bmin", active=act)), host(bt.jacobian_device("bmin", mode="adjoint", active=act))
    assert bt.epoch == epoch
    assert tq["dx"].shape == (1, n, n) and tq["dy"].shape == (1, m, n) and tb["dx"].shape == (1, n, m) and tb["dy"].shape == (1, m, m)
    assert "dy" not in aq and "dy" not in ab and aq["dx"].shape == (1, n, n) and ab["dx"].shape == (1, n, m)
    for out in (tq, aq, tb, ab):
        assert out["flag"].tolist() == [0]
    # dx/dq, dy/dq: column j of the tangent mode is the solve of -e_j (dx and dy_J); row j of the adjoint mode is the u of the solve of e_j
    for j in range(n):
        zr, scale, err64 = ref[j]
        col = np.concatenate([tq["dx"][0, :, j], tq["dy"][0, J, j]])
        errt = float(np.max(np.abs(col + zr))) / scale
        erra = float(np.max(np.abs(aq["dx"][0, j, :] + zr[:n]))) / scale
        print("SENS-MULTI | %s | n=%d dx/dq %d | err64 %.2e | tangent mode %.2e | adjoint mode %.2e" % (ctx.kind, n, j, err64, errt, erra))
        assert errt <= 8.0 * err64 and erra <= 8.0 * err64, (j, errt, erra, err64)
        assert np.all(np.delete(tq["dy"][0, :, j], J) == 0)
    # dx/dbmin, dy/dbmin: column i is the solve of e_(n + pos(i)) for a lower-active row i, zero for every other row; row j of the adjoint mode
    # is the w of the solve of e_j on the lower-active rows
    lower = np.flatnonzero(side < 0)
    for i in range(m):
        if side[i] >= 0:
            assert np.all(tb["dx"][0, :, i] == 0) and np.all(tb["dy"][0, :, i] == 0) and np.all(ab["dx"][0, :, i] == 0), i
            continue
        zr, scale, err64 = ref[n + int(np.flatnonzero(J == i)[0])]
        col = np.concatenate([tb["dx"][0, :, i], tb["dy"][0, J, i]])
        errt = float(np.max(np.abs(col - zr))) / scale
        print("SENS-MULTI | %s | n=%d dx/dbmin %d | err64 %.2e | tangent mode %.2e" % (ctx.kind, n, i, err64, errt))
        assert errt <= 8.0 * err64, (i, errt, err64)
    pos = np.array([int(np.flatnonzero(J == i)[0]) for i in lower], dtype=int)
    for j in range(n):
        zr, scale, err64 = ref[j]
        erra = float(np.max(np.abs(ab["dx"][0, j, lower] - zr[n + pos]))) / scale if len(lower) else 0.0
        print("SENS-MULTI | %s | n=%d dx/dbmin row %d | err64 %.2e | adjoint mode %.2e" % (ctx.kind, n, j, err64, erra))
        assert erra <= 8.0 * err64, (j, erra, err64)
    # the two modes, entry by entry, by the duality rule: g = e_i, the direction e_j
    for i in range(n):
        for j in range(n):
            bound = 8.0 * (ref[j][2] * ref[j][1] + ref[i][2] * ref[i][1])
            assert abs(tq["dx"][0, i, j] - aq["dx"][0, i, j]) <= bound, ("q", i, j)
        for c, r in zip(lower, pos):
            bound = 8.0 * (ref[n + r][2] * ref[n + r][1] + ref[i][2] * ref[i][1])
            assert abs(tb["dx"][0, i, c] - ab["dx"][0, i, c]) <= bound, ("bmin", i, c)
    if n == 5:   # three calls, the last one short: the bits of one call
        for mode in ("tangent", "adjoint"):
            a, b = host(bt.jacobian_device("q", mode=mode, chunk=2, active=act)), host(bt.jacobian_device("q", mode=mode, chunk=16, active=act))
            assert all(same_bits(a[k], b[k]) for k in a), mode
        # dbmax: the mirror image on the upper-active rows
        tx = host(bt.jacobian_device("bmax", active=act))
        assert np.all(tx["dx"][0][:, side <= 0] == 0) and all(np.any(tx["dx"][0][:, i] != 0) for i in np.flatnonzero(side > 0))
    with pytest.raises(ValueError):
        bt.jacobian_device("Q")
    with pytest.raises(ValueError):
        bt.jacobian_device("q", mode="both")
    with pytest.raises(ValueError):
        bt.jacobian_device("q", chunk=0)


def test_jacobian_of_a_mixed_batch(ctx):
    """a unit vector beyond a sized member's own n / m gives a zero column; the columns within are the single tangent calls'"""
    planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate([(20, 30, 7), (5, 8, 3)])]
    probs = [q[0] for q in planted]
    bt = solved(ctx, probs, scaling=10)
    jq = host(bt.jacobian_device("q", chunk=7))
    assert jq["flag"].tolist() == [0, 0] and jq["dx"].shape == (2, 20, 20)
    assert np.all(jq["dx"][1, 5:, :] == 0) and np.all(jq["dx"][1, :, 5:] == 0) and np.all(jq["dy"][1, :, 5:] == 0) and np.any(jq["dx"][1, :5, :5] != 0)
    for j in (0, 4, 13):
        e = np.zeros((2, 20))
        e[:, j] = 1.0
        one = host(bt.tangent_device(dq=T(ctx, e)))
        assert same_bits(jq["dx"][:, :, j], one["dx"]) and same_bits(jq["dy"][:, :, j], one["dy"]), j


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", REFUSED)
def test_unsupported_modes_are_refused(ctx, which):
    with refused_mode(ctx, which) as bt:
        g = T(ctx, np.ones((2, 1, 12)))
        for call, single in ((lambda: bt.adjoints_device(g), lambda: bt.adjoint_device(g[0])), (lambda: bt.tangents_device(dq=g), lambda: bt.tangent_device(dq=g[0]))):
            with pytest.raises(QpgError) as e:
                call()
            with pytest.raises(QpgError) as e1:
                single()
            assert e.value.code == e1.value.code == UNSUPPORTED
            assert REFUSED_WORD[which] in str(e.value)


def test_invalid_calls(ctx):
    bt, _ = small_batch(ctx, B=2)
    L, h = bt.L, bt.h
    g = T(ctx, np.ones((3, 2, 12)))
    bt.iterate(1)                                            # a solve in progress
    for call in (lambda: bt.adjoints_device(g), lambda: bt.tangents_device(dq=g)):
        with pytest.raises(QpgError) as e:
            call()
        assert e.value.code == INVALID and "in progress" in str(e.value)
    bt.solve()
    ref, ref_t = host(bt.adjoints_device(g)), host(bt.tangents_device(dq=g))
    # K = 0 and K = -1, at the C ABI and through the methods
    dq, dx = T(ctx, np.zeros((3, 2, 12))), T(ctx, np.zeros((3, 2, 12)))
    io = capi.DeviceAdjoint(gx=g.data_ptr(), dq=dq.data_ptr())
    tio = capi.DeviceTangent(dq=g.data_ptr(), dx=dx.data_ptr())
    for fn, arg in ((L.qpg_batch_adjoint_multi_device, io), (L.qpg_batch_tangent_multi_device, tio)):
        for K in (0, -1):
            assert fn(h, C.byref(arg), K, None, None, None) == INVALID, K
        assert fn(h, C.byref(arg), 3, None, None, None) == 0
    assert same_bits(N(dq), ref["dq"]) and same_bits(N(dx), ref_t["dx"])
    for K in (0, -1):
        with pytest.raises(QpgError) as e:
            bt.adjoints_device(g.data_ptr(), K=K, out=dict(dq=dq.data_ptr()))
        assert e.value.code == INVALID
        with pytest.raises(QpgError) as e:
            bt.tangents_device(dq=g.data_ptr(), K=K, out=dict(dx=dx.data_ptr()))
        assert e.value.code == INVALID
    with pytest.raises(QpgError) as e:
        bt.adjoints_device(T(ctx, np.ones((0, 2, 12))))
    assert e.value.code == INVALID
    # what the single calls refuse: no gx, no direction
    assert L.qpg_batch_adjoint_multi_device(h, C.byref(capi.DeviceAdjoint()), 2, None, None, None) == INVALID
    assert L.qpg_batch_adjoint_device(h, C.byref(capi.DeviceAdjoint())) == INVALID
    assert L.qpg_batch_tangent_multi_device(h, C.byref(capi.DeviceTangent()), 2, None, None, None) == INVALID
    assert L.qpg_batch_tangent_device(h, C.byref(capi.DeviceTangent())) == INVALID
    with pytest.raises(ValueError):
        bt.adjoints_device(None)
    with pytest.raises(ValueError):
        bt.tangents_device()
    # a point with a field missing
    P = point(bt)
    pt = capi.DevicePoint(x=P[0].data_ptr(), y=P[1].data_ptr())
    assert L.qpg_batch_adjoint_multi_device(h, C.byref(io), 3, C.byref(pt), None, None) == INVALID
    # leading dimensions that disagree; K against the tensors; raw addresses without K; wrong dtype or shape: ValueError before anything is launched
    with pytest.raises(ValueError):
        bt.adjoints_device(g, gy=T(ctx, np.ones((2, 2, 20))))
    with pytest.raises(ValueError):
        bt.tangents_device(dq=g, dbmin=T(ctx, np.ones((4, 2, 20))))
    with pytest.raises(ValueError):
        bt.adjoints_device(g, K=2)
    with pytest.raises(ValueError):
        bt.adjoints_device(g.data_ptr())
    with pytest.raises(ValueError):
        bt.adjoints_device(g, out=dict(flag=T(ctx, np.zeros(2), np.int64)))
    with pytest.raises(ValueError):
        bt.adjoints_device(g[0])
    with pytest.raises(ValueError):
        bt.tangents_device(dq=g.to(torch.float32))
    with pytest.raises(ValueError):
        bt.adjoints_device(g, want=("dq", "nonsense"))
    # an entry of 2 in active, and in select
    bad = np.zeros((2, 20), np.int64)
    bad[1, 19] = 2
    for call, single in ((lambda: bt.adjoints_device(g, active=T(ctx, bad, np.int64)), lambda: bt.adjoint_device(g[0], active=T(ctx, bad, np.int64))),
                         (lambda: bt.tangents_device(dq=g, active=T(ctx, bad, np.int64)), lambda: bt.tangent_device(dq=g[0], active=T(ctx, bad, np.int64))),
                         (lambda: bt.adjoints_device(g, select=T(ctx, [1, 2], np.int64)), lambda: bt.adjoint_device(g[0], select=T(ctx, [1, 2], np.int64)))):
        with pytest.raises(QpgError) as e:
            call()
        with pytest.raises(QpgError) as e1:
            single()
        assert e.value.code == e1.value.code == INVALID
    # ... and the batch still works: the same bits as before the refusals
    again, again_t = host(bt.adjoints_device(g)), host(bt.tangents_device(dq=g))
    assert all(same_bits(again[k], ref[k]) for k in ADJ_KEYS) and all(same_bits(again_t[k], ref_t[k]) for k in TAN_KEYS)
    rc, _ = bt.step_device(warm="last")
    assert rc == 0 and bt.statuses().tolist() == [1, 1]


def test_before_setup(ctx):
    """a batch that was created and never set up: QPG_ERR_INVALID, as from the single calls"""
    L = ctx.L
    h = C.c_void_p()
    st = ctx.default_settings(**ST)
    assert L.qpg_batch_create(ctx.h, 1, 2, 2, 4, 3, C.byref(st), C.byref(h)) == 0
    try:
        buf = T(ctx, np.zeros(8))
        assert L.qpg_batch_adjoint_multi_device(h, C.byref(capi.DeviceAdjoint(gx=buf.data_ptr())), 2, None, None, None) == INVALID
        assert L.qpg_batch_tangent_multi_device(h, C.byref(capi.DeviceTangent(dq=buf.data_ptr())), 2, None, None, None) == INVALID
        assert L.qpg_batch_adjoint_device(h, C.byref(capi.DeviceAdjoint(gx=buf.data_ptr()))) == INVALID
    finally:
        L.qpg_batch_destroy(h)

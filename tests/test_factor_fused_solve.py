"""The forward substitution of a Newton solve that rides on the factorisation before it (dense_factor with a right-hand side, context option
"factor_fused_solve"), against the separate pass and against tests/exact_refs.py.

Twin batches run the same QP with the option off and on.  Each is stepped with bt.iterate(1) -- "reset_newton" set ahead of every pass, so that the
next Newton pass refactorises (newton.c:98) -- until a pass has factorised and solved.  Of that pass:
  1. d of the two batches is equal bit for bit (the fused pass applies the same fma chain per entry: v = fma(-l_rc, y_c, v), c ascending, on the same
     thread); so are x, y and the iteration count of the complete solve (COMPLETE below; the other cases compare the iterates three passes later);
  2. n_fused_solve rises by one with the option on (where the vector fits the LDS) and not at all with it off;
  3. |L D L' d + dphi| <= 3 gamma_n |L||D||L'||d| componentwise, L and D as read back: test_ops_exact.test_solve's bound (any order of summation, FMA);
  4. where the n-vector does not fit the LDS behind the factorisation's blocks the pass stays unfused, is not counted, and agrees all the same.

Sizes: the 32-column block edges and a partial last block (31 .. 65); the 128-thread instance at its edge (129); the choice between the 256- and the
512-thread instance (255, 256, 257); 544 and 545 on 512 threads: the first block column's row loop takes a second trip for rows 512 + 32 and beyond;
1000, the benchmark's size.  The emulator has one instance (128 threads, 76 KB): the block edges, 129 (one row more than threads) and 161, where the first block
column's row loop takes a second trip for one row (an emulated solve of more rows takes minutes).
The vector does not fit: a factor of more than 4352 rows under the default 76 KB of the 512-thread instance (the smaller instances' factors always
fit theirs, and so does everything the emulator can run in seconds): n = 4353 on the GPU.
"""
import numpy as np
import pytest

from tests import exact_refs as xr
from tests.test_ops_exact import Case, Opened, worst_ratio

FIT = ([Case("hip", 0, n, 512) for n in (31, 32, 33, 64, 65)] + [Case("hip", 2, 129, 128)] +
       [Case("hip", 1, 255, 256), Case("hip", 1, 256, 256), Case("hip", 1, 257, 512)] +
       [Case("hip", 0, n, 512) for n in (544, 545, 1000)] +
       [Case("emu", 0, n, 128) for n in (31, 32, 33, 64, 65, 129, 161)])
NO_FIT = [Case("hip", 0, 4353, 512)]
MAX_PASSES = 12


def COMPLETE(case):
    """the solve is run to its end (an emulated one of more than 65 rows takes a minute; n = 4353 has 0.4 s factorisations)"""
    return case.n <= (65 if case.kind == "emu" else 1000)


def _counts(bt):
    s = bt.stats(0)
    return int(s.n_refactor) + int(s.n_factor_Q), int(s.n_solve), int(s.n_fused_solve)


def _run(ctx, case, fused, complete):
    """one batch: the first pass after Opened's two that factorises and solves -> d, dphi, (L, D), the counters' steps, the rest of the solve"""
    out = {}
    try:
        with Opened(ctx, case, factor_fused_solve=fused) as o:
            bt, n = o.bt, case.n
            for k in range(MAX_PASSES):
                before = _counts(bt)
                bt.set_scalar("reset_newton", 1)
                bt.iterate(1)
                after = _counts(bt)
                step = tuple(a - b for a, b in zip(after, before))
                if step[0] == 1 and step[1] == 1:
                    break
                assert step[0] == 0 and step[2] <= step[1], (case.id, step)      # (a pass that only updates the factor may fuse on the sweep)
            else:
                raise AssertionError("%s: no pass factorised and solved within %d passes" % (case.id, MAX_PASSES))
            out["passes"], out["step"] = k + 1, step
            out["d"], out["dphi"] = bt.vec("d")[:n].copy(), bt.vec("dphi")[:n].copy()
            out["factor"] = bt.factor(0) if n <= 1000 else None
            if complete:
                bt.solve()
                info = bt.info(0)
                out["iter"], out["status"] = int(info.iter), int(info.status_val)
                x, y = bt.solution()
                out["x"], out["y"] = x[0].copy(), y[0].copy()
            else:
                bt.iterate(3)
                out["iter"], out["status"] = int(bt.info(0).iter), 0
                out["x"], out["y"] = bt.vec("x")[:n].copy(), bt.vec("y")[:case.m].copy()
    finally:
        ctx.set_option("factor_fused_solve", 1)
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _twins(ctx, case, fits):
    off, on = _run(ctx, case, 0, COMPLETE(case)), _run(ctx, case, 1, COMPLETE(case))
    print("factor_fused_solve %s: pass %d, counter steps (factorisations, solves, fused) off %s on %s" % (case.id, on["passes"], off["step"], on["step"]))
    assert off["passes"] == on["passes"]
    assert off["step"] == (1, 1, 0), (case.id, off["step"])
    assert on["step"] == (1, 1, 1 if fits else 0), (case.id, on["step"])
    assert np.all(np.isfinite(on["d"])) and np.any(on["d"] != 0)
    assert _same_bits(off["dphi"], on["dphi"]) and _same_bits(off["d"], on["d"]), (case.id, float(np.max(np.abs(off["d"] - on["d"]))))
    assert off["iter"] == on["iter"] and off["status"] == on["status"], (case.id, off["iter"], on["iter"])
    assert _same_bits(off["x"], on["x"]) and _same_bits(off["y"], on["y"]), case.id
    return off, on


@pytest.mark.parametrize("ctx,case", [c.param() for c in FIT], indirect=["ctx"])
def test_factor_carries_the_forward_substitution(ctx, case):
    off, on = _twins(ctx, case, True)
    assert on["status"] == (1 if COMPLETE(case) else 0), (case.id, on["status"])
    n = case.n
    L, D = on["factor"]
    assert _same_bits(L, off["factor"][0]) and _same_bits(D, off["factor"][1])
    Lu = xr.unit_lower(L)
    Ll, Dl = np.asarray(Lu, dtype=xr.LD), np.asarray(D, dtype=xr.LD)
    La, Da = np.abs(Lu), np.abs(D)
    d = on["d"]
    res = np.abs(Ll @ (Dl * (Ll.T @ np.asarray(d, dtype=xr.LD))) + np.asarray(on["dphi"], dtype=xr.LD))
    bound = 3 * xr.gamma_k(n) * (La @ (Da * (La.T @ np.abs(d))))
    ratio = worst_ratio(res, bound)
    print("factor_fused_solve %s: max residual / bound = %.3g" % (case.id, ratio))
    assert ratio <= 1.0, (case.id, ratio)


@pytest.mark.parametrize("ctx,case", [c.param() for c in NO_FIT], indirect=["ctx"])
def test_vector_that_does_not_fit_stays_unfused(ctx, case):
    _twins(ctx, case, False)

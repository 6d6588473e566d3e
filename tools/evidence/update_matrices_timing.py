#!/usr/bin/env python3
"""What qpg_batch_update_Q_A saves: wall time of  update_Q_A + warm_start_last  against  close + QpalmBatch(...) (create, set_problems, setup) +
warm_start  with the same data, on one MI355X.  Two batches: random QPs at n = 1000, m = 2000 (dense Schur factors) and sparse_qp(2000, "banded")
with the sparse factor.  Median of --reps runs each; every timed window ends in a device synchronise (the entry points synchronise themselves).
The solve that follows either path is timed by the library's own events (last_solve_ms): same kernel, same bits, so the two must agree.

  python tools/evidence/update_matrices_timing.py --batch random --B 2048 [--lib OTHER_BUILD.so --paths recreate]

--lib times another build of the library (the parent commit's, which has no update entry: --paths recreate).  One JSON line per batch."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def redraw(p, seed):
    """p's patterns, every value of A drawn again and Q scaled entry by entry by a factor in [1, 1.2) on the diagonal and [0.8, 1) off it (stays dominant)"""
    rng = np.random.default_rng(seed)
    col = np.repeat(np.arange(p.n), np.diff(p.Qp))
    diag = np.asarray(p.Qi) == col
    Qx = np.asarray(p.Qx, float) * np.where(diag, 1.0 + 0.2 * rng.random(len(p.Qx)), 0.8 + 0.2 * rng.random(len(p.Qx)))
    return dataclasses.replace(p, Qx=Qx, Ax=np.asarray(p.Ax, float) * (0.5 + rng.random(len(p.Ax))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", choices=["random", "sparse"], required=True)
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64, help="distinct QPs generated; the batch repeats them")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--paths", default="update,recreate")
    ap.add_argument("--n", type=int, default=0)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU fallback"
    torch.cuda.init()
    from qpalm_amd.problems import random_qp, sparse_qp
    from qpalm_amd.solver import Context, QpalmBatch
    ctx = Context(0, lib_path=a.lib)
    assert ctx.backend == "gfx950-hip"
    if a.batch == "random":
        n = a.n or 1000
        base = [random_qp(n, 2 * n, seed=1000 + k) for k in range(a.distinct)]
    else:
        n = a.n or 2000
        ctx.set_option("sparse_factor", 1)
        base = [sparse_qp(n, "banded", seed=k) for k in range(a.distinct)]
    sets = [[(base if s == 0 else [redraw(p, 100 * s + k) for k, p in enumerate(base)])[b % a.distinct] for b in range(a.B)] for s in range(3)]
    st = ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    paths = a.paths.split(",")
    out = dict(batch=a.batch, B=a.B, n=n, m=base[0].m, lib=a.lib or "this build", reps=a.reps)
    bt = QpalmBatch(ctx, sets[0], st)
    bt.solve()          # warm-up of every kernel, and the stored solutions the warm starts use
    out["first_solve_ms"] = bt.last_solve_ms()
    if "update" in paths:
        padded = [(bt._padded([p.Qx for p in s], bt.nnzQ), bt._padded([p.Ax for p in s], bt.nnzA)) for s in sets]
        bt.update_Q_A(*padded[1]); bt.warm_start_last(); bt.solve()       # warm-up of the update kernel
        t, ms = [], []
        for r in range(a.reps):
            Qx, Ax = padded[(r + 2) % 3]
            t0 = time.perf_counter()
            bt.update_Q_A(Qx, Ax)
            bt.warm_start_last()
            t.append(time.perf_counter() - t0)
            bt.solve()
            ms.append(bt.last_solve_ms())
            assert all(int(v) == 1 for v in bt.statuses())
        out.update(update_s=t, update_median_s=statistics.median(t), solve_after_update_ms=ms)
    if "recreate" in paths:
        t, ms = [], []
        for r in range(a.reps + 1):      # (the first one is a warm-up)
            x, y = bt.solution()
            probs = sets[(r + 2) % 3]
            t0 = time.perf_counter()
            bt.close()
            bt = QpalmBatch(ctx, probs, st)
            bt.warm_start(x, y)
            dt = time.perf_counter() - t0
            bt.solve()
            assert all(int(v) == 1 for v in bt.statuses())
            if r > 0:
                t.append(dt); ms.append(bt.last_solve_ms())
        out.update(recreate_s=t, recreate_median_s=statistics.median(t), solve_after_recreate_ms=ms)
    if "update_median_s" in out and "recreate_median_s" in out:
        out["ratio"] = out["recreate_median_s"] / out["update_median_s"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

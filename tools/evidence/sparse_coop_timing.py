#!/usr/bin/env python3
"""Sparse coop mode against the one-workgroup sparse factor: ONE QP at eps = 1e-6, the at-size cases of profiles/r06/final/sparse_factor_at_size.txt
(blocks n = 100 000; banded n = 20 000 and n = 100 000 under nested dissection; arrow n = 20 000), wall time of qpg_batch_solve on one MI355X:
median of --reps solves after one warm-up (every solve restarts from the cold start), with the launch plan and the level count beside it.

  python tools/evidence/sparse_coop_timing.py --case blocks:100000 --coop 0,1            # this build, "sparse_coop" = 0 and 1
  python tools/evidence/sparse_coop_timing.py --case blocks:100000 --lib PARENT_BUILD.so # another build (the parent commit's: no such option)

One process per case and build (run each under its own `timeout`); one JSON line per setting.  The comparison that counts is against the parent
commit's build; the "sparse_coop" = 0 column only shows what the shared level code cost the one-workgroup path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, help="kind:n, e.g. blocks:100000")
    ap.add_argument("--ordering", type=int, default=-1)
    ap.add_argument("--coop", default="", help="comma-separated values of sparse_coop to time; empty: the option is not touched (older builds)")
    ap.add_argument("--workgroups", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU fallback"
    torch.cuda.init()
    from qpalm_amd.problems import sparse_qp
    from qpalm_amd.solver import Context, QpalmBatch
    kind, n = a.case.split(":")
    p = sparse_qp(int(n), kind, seed=21)
    ctx = Context(0, lib_path=a.lib)
    assert ctx.backend == "gfx950-hip"
    ctx.set_option("sparse_factor", 1)
    ctx.set_option("sparse_ordering", a.ordering)
    ctx.set_option("coop_workgroups", a.workgroups)
    for mode in ([int(v) for v in a.coop.split(",")] if a.coop else [None]):
        if mode is not None:
            ctx.set_option("sparse_coop", mode)
        bt = QpalmBatch(ctx, [p], ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0))
        plan = bt.sparse_coop_info(0) if hasattr(bt.L, "qpg_batch_sparse_coop_info") else (0, 0, 0)
        t = []
        for r in range(a.reps + 1):          # (the first one is the warm-up: first launches, recorded chains)
            bt.warm_start(None, None)
            t0 = time.perf_counter()
            bt.solve()
            if r > 0:
                t.append(time.perf_counter() - t0)
            assert int(bt.info(0).status_val) == 1
        s = bt.stats(0)
        print(json.dumps(dict(case=a.case, ordering=a.ordering, lib=a.lib or "this build", sparse_coop=mode, levels=bt.sparse_perm(0)[1], nnzL=bt.sparse_info(0)[0],
                              factor_launches=plan[0], solve_launches=plan[1], max_grid=plan[2], iter=int(bt.info(0).iter),
                              n_refactor=int(s.n_refactor), n_factor_Q=int(s.n_factor_Q), n_rank1=int(s.n_rank1), n_solve=int(s.n_solve),
                              solve_s=[round(v, 4) for v in t], median_s=round(statistics.median(t), 4))), flush=True)
        bt.close()


if __name__ == "__main__":
    main()

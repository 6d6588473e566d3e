#!/usr/bin/env python3
"""What the polish of a solved batch costs and buys: the mpc-160 batch of `bench.py --workload mpc-160` (8192 QPs, one plant per 64, every QP its own
initial state), brought to the state tools/evidence/adjoint_timing.py times (a cold step and --warmup warm steps on tensors that stay on the GPU).

GPU steps, each a process of its own under `timeout -k 10` (a step that faults, aborts or runs out of time ends the chain: nothing more is started on
the device); the first four in turn, --runs times:

  forward   this build: step_device (new initial states, warm start from the last solution);
  adjoint   this build: adjoint_device with gx = ones and every output wanted;
  parent    --lib (another build, the parent commit's): the same adjoint call -- the kernel the polish shares must not have slowed down;
  polish    this build: polish_device without store and every output wanted, at the benchmark's 1e-6; the distribution of `passes`, the count of each
            flag, the medians of pri / dua before and after;
  trade     this build, once: the same batch cold, "solve to 1e-3, then polish with store" against "solve to 1e-9": wall ms of each part and the
            residuals of the stored solutions at the end, over every member (as a further polish call reports them: pri_old / dua_old of whatever is
            stored -- the candidate where it was accepted, the solve's solution where not).  With --sens-penalty the first arm runs twice: with the
            solve's own penalties, and with the floor (QpalmBatch.sens_penalty).

--sens-penalty also applies to this build's `adjoint` and `polish` steps (never to `parent`: an older build has no such call).

Per figure: wall ms per call (host clock around a call that ends in a device synchronise), median and minimum of --calls calls after two untimed ones.
No ratio is judged here: read the figures side by side, and the spread between the runs.

  python tools/evidence/polish_timing.py [--lib PARENT_BUILD.so] [--B 8192] [--calls 10] [--runs 2] [--limit 300] [--sens-penalty FLOOR] [--steps forward,adjoint,...]

One JSON line per step."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NX = 10


def timed(fn, calls):
    ms = []
    for k in range(2 + calls):
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            ms.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_per_call_median=statistics.median(ms), ms_per_call_min=min(ms), ms_per_call_max=max(ms), calls=len(ms))


def once(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def res_summary(res, flag, formed=True):
    """medians and maxima of the four residuals over the members a candidate was formed for (formed = False: over every member that is solved --
    where the refinement was flagged, the `_new` values repeat the old ones)"""
    import torch
    r = res[((flag == 0) | (flag == 3)) if formed else (flag != 2)]
    if r.shape[0] == 0:
        return {}
    names = ("pri_old", "dua_old", "pri_new", "dua_new")
    out = {k + "_median": float(torch.median(r[:, i]).item()) for i, k in enumerate(names)}
    out.update({k + "_max": float(r[:, i].max().item()) for i, k in enumerate(names)})
    return out


def flags(flag):
    return {"flag%d" % f: int((flag == f).sum().item()) for f in range(4)}


def child(args):
    import torch
    from qpalm_amd.solver import Context, QpalmBatch
    from tools.evidence.device_step_timing import mpc_problems
    rng = np.random.Generator(np.random.PCG64(2024))
    probs = mpc_problems(args.B, rng)
    if args.rehearse:   # the kernels on the host emulator: the script's own logic, no figure means anything
        from qpalm_amd import build
        ctx, dev = Context(0, lib_path=build.build_emu()), "cpu"
    else:
        torch.cuda.init()
        ctx, dev = Context(0, lib_path=args.lib if args.child == "parent" else None), "cuda:0"
    eps = 1e-6
    bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=eps, eps_rel=eps, verbose=0))
    out = dict(x=bt._empty((bt.B, bt.n)), y=bt._empty((bt.B, bt.m)), status_val=bt._empty((bt.B,), "int64"))
    res = dict(step=args.child, B=bt.B, n=bt.n, m=bt.m)
    pol = {k: bt._empty(*s) for k, s in dict(x=((bt.B, bt.n),), y=((bt.B, bt.m),), res=((bt.B, 4),), active=((bt.B, bt.m), "int64"),
                                               flag=((bt.B,), "int64"), resid=((bt.B,),), passes=((bt.B,), "int64")).items()}
    if args.child == "trade":
        # both arms start cold on the same batch (warm=None: no warm start); the settings change between them
        arms = [("solve_1e-3_then_polish", 1e-3, 0.0)] + ([("solve_1e-3_then_polish_floor", 1e-3, args.sens_penalty)] if args.sens_penalty > 0 else [])
        for arm, e, floor in arms + [("solve_1e-9", 1e-9, 0.0)]:
            bt.sens_penalty = floor
            bt.update_settings(ctx.default_settings(eps_abs=e, eps_rel=e, verbose=0))
            bt.step_device(warm=None, out=out)                                     # untimed: the first launch of this shape
            ms_solve = [once(lambda: bt.step_device(warm=None, out=out)) for _ in range(args.calls)]
            solved = int((out["status_val"] == 1).sum().item())
            d = dict(ms_solve_median=statistics.median(ms_solve), ms_solve_min=min(ms_solve), solved=solved, sens_penalty=floor)
            if e == 1e-3:
                ms_pol = []
                for _ in range(args.calls):                                        # every timed polish starts from the 1e-3 solution again
                    bt.step_device(warm=None, out=out)
                    ms_pol.append(once(lambda: bt.polish_device(store=True, out=pol)))
                d.update(ms_polish_median=statistics.median(ms_pol), ms_polish_min=min(ms_pol), **flags(pol["flag"]))
                d["polish_" + "passes_max"] = int(pol["passes"].max().item())
                first = res_summary(pol["res"], pol["flag"])
                d.update({"polish_" + k: v for k, v in first.items()})
            bt.polish_device(out=pol)                                              # not timed: what is stored now, measured
            d.update({"final_" + k: v for k, v in res_summary(pol["res"], pol["flag"], formed=False).items() if k.startswith(("pri_old", "dua_old"))},
                     final_members=int((pol["flag"] != 2).sum().item()))
            res[arm] = d
        print(json.dumps(res), flush=True)
        return
    if args.child != "parent" and args.sens_penalty > 0:
        bt.sens_penalty = args.sens_penalty
        res["sens_penalty"] = args.sens_penalty
    bmin = torch.from_numpy(np.stack([p.bmin for p in probs])).to(dev)
    bmax = torch.from_numpy(np.stack([p.bmax for p in probs])).to(dev)
    noise = torch.from_numpy(0.1 * rng.standard_normal((args.warmup + 2 + args.calls, args.B, NX))).to(dev)
    bt.step_device(warm=None, out=out)
    step = [0]

    def forward():
        x0 = bmin[:, :NX] + noise[step[0]]
        step[0] += 1
        bmin[:, :NX] = x0
        bmax[:, :NX] = x0
        rc, _ = bt.step_device(bmin, bmax, warm="last", out=out)
        assert rc == 0

    for _ in range(args.warmup):
        forward()
    res["solved"] = int((out["status_val"] == 1).sum().item())
    if args.child == "forward":
        res.update(timed(forward, args.calls))
    elif args.child in ("adjoint", "parent"):
        gx = torch.ones((bt.B, bt.n), dtype=torch.float64, device=dev)
        outs = {k: bt._empty(*s) for k, s in dict(dq=((bt.B, bt.n),), dbmin=((bt.B, bt.m),), dbmax=((bt.B, bt.m),), dQx=((bt.B, bt.nnzQ),),
                                                   dAx=((bt.B, bt.nnzA),), active=((bt.B, bt.m), "int64"), flag=((bt.B,), "int64"),
                                                   resid=((bt.B,),), passes=((bt.B,), "int64")).items()}
        res.update(timed(lambda: bt.adjoint_device(gx, out=outs), args.calls))
        res.update(flag0=int((outs["flag"] == 0).sum().item()), max_passes=int(outs["passes"].max().item()), lib=args.lib if args.child == "parent" else "this build")
    else:
        res.update(timed(lambda: bt.polish_device(out=pol), args.calls))
        passes = pol["passes"][(pol["flag"] == 0) | (pol["flag"] == 3)]
        vals, counts = torch.unique(passes, return_counts=True)
        res.update(flags(pol["flag"]), passes={int(v): int(c) for v, c in zip(vals.tolist(), counts.tolist())}, eps=eps, **res_summary(pol["res"], pol["flag"]))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's) for the `parent` step; without it that step is left out")
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds each GPU step may take")
    ap.add_argument("--rehearse", action="store_true", help="run the steps on the host emulator (a check of this script; use a small --B)")
    ap.add_argument("--sens-penalty", type=float, default=0.0, help="penalty floor of the sensitivity solves' preconditioner (0: the solve's own penalties)")
    ap.add_argument("--steps", default="forward,adjoint,parent,polish,trade", help="the steps to run, of those above")
    ap.add_argument("--child", choices=("forward", "adjoint", "parent", "polish", "trade"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    steps = [s for s in ("forward", "adjoint", "parent", "polish") if s != "parent" or args.lib] * args.runs + ["trade"]
    steps = [s for s in steps if s in args.steps.split(",")]
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--B", str(args.B),
               "--calls", str(args.calls), "--warmup", str(args.warmup), "--sens-penalty", repr(args.sens_penalty)] + (["--lib", os.path.abspath(args.lib)] if args.lib else []) + (["--rehearse"] if args.rehearse else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps(dict(step=step, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

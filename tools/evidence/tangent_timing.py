#!/usr/bin/env python3
"""What the tangent of a solved batch costs, next to the adjoint call of another build (the parent commit's): the mpc-160 batch of
`bench.py --workload mpc-160` (8192 QPs, one plant per 64, every QP its own initial state), brought to the state tools/evidence/adjoint_timing.py times
(a cold step and --warmup warm steps on tensors that stay on the GPU).

GPU steps, each a process of its own under `timeout -k 10` (a step that faults, aborts or runs out of time ends the chain: nothing more is started on
the device), the two builds in turn, --runs times:

  adjoint   --lib (the other build): adjoint_device with gx = ones and every output wanted;
  tangent   this build: tangent_device with a q-and-bounds direction (dq, dbmin, dbmax), then with all five inputs, dx and dy and every flag wanted.

Per figure: wall ms per call (host clock around a call that ends in a device synchronise), median and minimum of --calls calls after two untimed ones.
No ratio is judged here: read the figures side by side, and the spread between the runs.

  python tools/evidence/tangent_timing.py --lib PARENT_BUILD.so [--B 8192] [--calls 10] [--runs 2] [--limit 300] [--sens-penalty FLOOR]

--sens-penalty: the penalty floor of the preconditioner (QpalmBatch.sens_penalty) for this build's tangent calls.

One JSON line per step and one at the end."""
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


def child(args):
    import torch
    torch.cuda.init()
    from qpalm_amd.solver import Context, QpalmBatch
    from tools.evidence.device_step_timing import mpc_problems
    rng = np.random.Generator(np.random.PCG64(2024))
    probs = mpc_problems(args.B, rng)
    ctx = Context(0, lib_path=args.lib if args.child == "adjoint" else None)
    bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0))
    dev = "cuda:0"
    bmin = torch.from_numpy(np.stack([p.bmin for p in probs])).to(dev)
    bmax = torch.from_numpy(np.stack([p.bmax for p in probs])).to(dev)
    noise = torch.from_numpy(0.1 * rng.standard_normal((args.warmup, args.B, NX))).to(dev)
    out = dict(x=bt._empty((bt.B, bt.n)), y=bt._empty((bt.B, bt.m)), status_val=bt._empty((bt.B,), "int64"))
    bt.step_device(warm=None, out=out)
    for k in range(args.warmup):
        x0 = bmin[:, :NX] + noise[k]
        bmin[:, :NX] = x0
        bmax[:, :NX] = x0
        rc, _ = bt.step_device(bmin, bmax, warm="last", out=out)
        assert rc == 0
    if args.child == "tangent":
        bt.sens_penalty = args.sens_penalty
    res = dict(step=args.child, lib=(args.lib if args.child == "adjoint" else "this build"), B=bt.B, n=bt.n, m=bt.m, sens_penalty=args.sens_penalty if args.child == "tangent" else 0.0,
               solved=int((out["status_val"] == 1).sum().item()))
    rnd = lambda *shape: torch.from_numpy(rng.standard_normal(shape)).to(dev)
    flags = lambda o: dict(flag0=int((o["flag"] == 0).sum().item()), flag1=int((o["flag"] == 1).sum().item()), flag2=int((o["flag"] == 2).sum().item()),
                           max_passes=int(o["passes"].max().item()), max_resid=float(o["resid"].max().item()))
    if args.child == "adjoint":
        gx = torch.ones((bt.B, bt.n), dtype=torch.float64, device=dev)
        outs = {k: bt._empty(*s) for k, s in dict(dq=((bt.B, bt.n),), dbmin=((bt.B, bt.m),), dbmax=((bt.B, bt.m),), dQx=((bt.B, bt.nnzQ),),
                                                   dAx=((bt.B, bt.nnzA),), active=((bt.B, bt.m), "int64"), flag=((bt.B,), "int64"),
                                                   resid=((bt.B,),), passes=((bt.B,), "int64")).items()}
        res["adjoint"] = dict(timed(lambda: bt.adjoint_device(gx, out=outs), args.calls), **flags(outs))
    else:
        outs = {k: bt._empty(*s) for k, s in dict(dx=((bt.B, bt.n),), dy=((bt.B, bt.m),), active=((bt.B, bt.m), "int64"), flag=((bt.B,), "int64"),
                                                   resid=((bt.B,),), passes=((bt.B,), "int64")).items()}
        dq, lo, hi, dQ, dA = rnd(bt.B, bt.n), rnd(bt.B, bt.m), rnd(bt.B, bt.m), rnd(bt.B, bt.nnzQ), rnd(bt.B, bt.nnzA)
        res["tangent_q_bounds"] = dict(timed(lambda: bt.tangent_device(dq, lo, hi, out=outs), args.calls), **flags(outs))
        res["tangent_all_five"] = dict(timed(lambda: bt.tangent_device(dq, lo, hi, dQ, dA, out=outs), args.calls), **flags(outs))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds each GPU step may take")
    ap.add_argument("--lib", default=None, help="the other build, whose adjoint call is timed")
    ap.add_argument("--sens-penalty", type=float, default=0.0)
    ap.add_argument("--child", choices=("adjoint", "tangent"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    got = {"adjoint": [], "tangent": []}
    for _ in range(args.runs):
        for step in (("adjoint", "tangent") if args.lib else ("tangent",)):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--B", str(args.B),
                   "--calls", str(args.calls), "--warmup", str(args.warmup), "--sens-penalty", repr(args.sens_penalty)] + (["--lib", args.lib] if args.lib else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:
                print(json.dumps(dict(step=step, failed=r.returncode)))
                return r.returncode
            got[step].append(json.loads(r.stdout.strip().splitlines()[-1]))
    med = lambda step, key: [g[key]["ms_per_call_median"] for g in got[step]]
    print(json.dumps(dict(workload="mpc-160", B=args.B, other_build_adjoint_ms_per_call=med("adjoint", "adjoint") if args.lib else None,
                          tangent_q_bounds_ms_per_call=med("tangent", "tangent_q_bounds"), tangent_all_five_ms_per_call=med("tangent", "tangent_all_five"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())

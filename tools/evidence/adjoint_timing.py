#!/usr/bin/env python3
"""What the adjoint of a solved batch costs next to a forward step of the same build: the mpc-160 batch of `bench.py --workload mpc-160` (8192 QPs, one
plant per 64, every QP its own initial state).

Two GPU steps, each a process of its own under `timeout -k 10` (a step that faults, aborts or runs out of time ends the chain: nothing more is started
on the device):

  forward   step_device on tensors that stay on the GPU (new initial states, warm start from the last solution), --steps timed steps after --warmup;
  adjoint   the same batch brought to the same state, then adjoint_device with gx = ones and every output wanted, --steps timed calls.

Per step: wall ms per call (host clock around a call that ends in a device synchronise; median and minimum over the calls).  The adjoint step also
reports the flags, the largest pass count and the largest residual ratio of its last call.  No ratio is printed: read the two figures side by side.

  python tools/evidence/adjoint_timing.py [--B 8192] [--steps 20] [--warmup 3] [--limit 300]

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


def child(args):
    import torch
    torch.cuda.init()
    from qpalm_amd.solver import Context, QpalmBatch
    from tools.evidence.device_step_timing import mpc_problems
    rng = np.random.Generator(np.random.PCG64(2024))
    probs = mpc_problems(args.B, rng)
    ctx = Context(0)
    bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0))
    dev = "cuda:0"
    bmin = torch.from_numpy(np.stack([p.bmin for p in probs])).to(dev)
    bmax = torch.from_numpy(np.stack([p.bmax for p in probs])).to(dev)
    noise = torch.from_numpy(0.1 * rng.standard_normal((args.warmup + args.steps, args.B, NX))).to(dev)
    out = dict(x=bt._empty((bt.B, bt.n)), y=bt._empty((bt.B, bt.m)), status_val=bt._empty((bt.B,), "int64"))
    bt.step_device(warm=None, out=out)

    def forward(k):
        x0 = bmin[:, :NX] + noise[k]
        bmin[:, :NX] = x0
        bmax[:, :NX] = x0
        rc, _ = bt.step_device(bmin, bmax, warm="last", out=out)
        assert rc == 0

    ms = []
    nfwd = args.warmup + (args.steps if args.child == "forward" else 0)
    for k in range(nfwd):
        t0 = time.perf_counter()
        forward(k)
        if k >= args.warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    res = dict(step=args.child, B=bt.B, n=bt.n, m=bt.m, solved=int((out["status_val"] == 1).sum().item()))
    if args.child == "adjoint":
        gx = torch.ones((bt.B, bt.n), dtype=torch.float64, device=dev)
        outs = {k: bt._empty(*s) for k, s in dict(dq=((bt.B, bt.n),), dbmin=((bt.B, bt.m),), dbmax=((bt.B, bt.m),), dQx=((bt.B, bt.nnzQ),),
                                                   dAx=((bt.B, bt.nnzA),), active=((bt.B, bt.m), "int64"), flag=((bt.B,), "int64"),
                                                   resid=((bt.B,),), passes=((bt.B,), "int64")).items()}
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            bt.adjoint_device(gx, out=outs)
            if k >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        res.update(flag0=int((outs["flag"] == 0).sum().item()), flag1=int((outs["flag"] == 1).sum().item()), flag2=int((outs["flag"] == 2).sum().item()),
                   max_passes=int(outs["passes"].max().item()), max_resid=float(outs["resid"].max().item()))
    res.update(ms_per_call_median=statistics.median(ms), ms_per_call_min=min(ms), calls=len(ms))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds each GPU step may take")
    ap.add_argument("--child", choices=("forward", "adjoint"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    got = {}
    for step in ("forward", "adjoint"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--B", str(args.B),
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(json.dumps(dict(step=step, failed=r.returncode)))
            return r.returncode
        got[step] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(dict(workload="mpc-160", B=args.B, forward_ms_per_step=got["forward"]["ms_per_call_median"],
                          adjoint_ms_per_call=got["adjoint"]["ms_per_call_median"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())

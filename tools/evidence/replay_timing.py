#!/usr/bin/env python3
"""What differentiating at a recorded point costs: the mpc-160 batch of `bench.py --workload mpc-160` (8192 QPs, one plant per 64,
every QP its own initial state), brought to the state tools/evidence/adjoint_timing.py times (a cold step and --warmup warm steps on tensors that stay
on the GPU).

GPU steps, each a process of its own under `timeout -k 10` (a step that faults, aborts or runs out of time ends the chain: nothing more is started on
the device); the first four in turn, --runs times:

  active    this build: active_device (the active set of the stored solutions on its own);
  adjoint   this build: adjoint_device with gx = ones and every output wanted;
  at        this build: the same call with at = (the stored x, the stored y, active_device()) -- the same kernel with two pointers swapped;
  parent    --lib (another build, the parent commit's): the plain adjoint call -- the shared kernel must not have slowed down;
  rollout   this build, once: a closed-loop rollout of --T steps on ONE batch through QPLayer(replay=True) -- the initial state of step t + 1 is the
            state the solution of step t predicts (plus the benchmark's noise), loss = sum_t |x_t|^2, one backward() through all of it; wall ms of
            the forward loop and of the backward, the adjoint flags per step.

Per figure: wall ms per call (host clock around a call that ends in a device synchronise), median, minimum and maximum of --calls calls after two untimed
ones.  No ratio is judged here: read the figures side by side, and the spread between the runs.

  python tools/evidence/replay_timing.py [--lib PARENT_BUILD.so] [--B 8192] [--calls 10] [--runs 2] [--T 10] [--limit 300] [--steps active,adjoint,...]

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
STEPS = ("active", "adjoint", "at", "parent")


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
    from qpalm_amd.solver import Context, QpalmBatch
    from qpalm_amd.torch_layer import QPLayer
    from tools.evidence.device_step_timing import mpc_problems
    rng = np.random.Generator(np.random.PCG64(2024))
    probs = mpc_problems(args.B, rng)
    if args.rehearse:   # the kernels on the host emulator: the script's own logic, no figure means anything
        from qpalm_amd import build
        ctx, dev = Context(0, lib_path=build.build_emu()), "cpu"
    else:
        torch.cuda.init()
        ctx, dev = Context(0, lib_path=args.lib if args.child == "parent" else None), "cuda:0"
    sync = (lambda: None) if args.rehearse else torch.cuda.synchronize
    eps = 1e-6
    bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=eps, eps_rel=eps, verbose=0))
    out = dict(x=bt._empty((bt.B, bt.n)), y=bt._empty((bt.B, bt.m)), status_val=bt._empty((bt.B,), "int64"))
    res = dict(step=args.child, B=bt.B, n=bt.n, m=bt.m)
    bmin = torch.from_numpy(np.stack([p.bmin for p in probs])).to(dev)
    bmax = torch.from_numpy(np.stack([p.bmax for p in probs])).to(dev)
    noise = torch.from_numpy(0.1 * rng.standard_normal((args.warmup + args.T, args.B, NX))).to(dev)
    bt.step_device(warm=None, out=out)
    for k in range(args.warmup):
        x0 = bmin[:, :NX] + noise[k]
        bmin[:, :NX] = x0
        bmax[:, :NX] = x0
        rc, _ = bt.step_device(bmin, bmax, warm="last", out=out)
        assert rc == 0
    res["solved"] = int((out["status_val"] == 1).sum().item())
    if args.child == "active":
        act = bt._empty((bt.B, bt.m), "int64")
        res.update(timed(lambda: bt.active_device(out=act), args.calls))
        res.update(active_rows=int((act != 0).sum().item()))
    elif args.child in ("adjoint", "at", "parent"):
        gx = torch.ones((bt.B, bt.n), dtype=torch.float64, device=dev)
        outs = {k: bt._empty(*s) for k, s in dict(dq=((bt.B, bt.n),), dbmin=((bt.B, bt.m),), dbmax=((bt.B, bt.m),), dQx=((bt.B, bt.nnzQ),),
                                                   dAx=((bt.B, bt.nnzA),), active=((bt.B, bt.m), "int64"), flag=((bt.B,), "int64"),
                                                   resid=((bt.B,),), passes=((bt.B,), "int64")).items()}
        if args.child == "at":
            x, y = bt.solution_device()
            at = (x, y, bt.active_device())
            res.update(timed(lambda: bt.adjoint_device(gx, out=outs, at=at), args.calls))
        else:
            res.update(timed(lambda: bt.adjoint_device(gx, out=outs), args.calls))
        res.update(flag0=int((outs["flag"] == 0).sum().item()), max_passes=int(outs["passes"].max().item()), lib=args.lib if args.child == "parent" else "this build")
    else:   # rollout
        layer = QPLayer(bt, warm="last", replay=True)
        x0 = (bmin[:, :NX] + noise[args.warmup]).clone().requires_grad_(True)
        lo_rest, hi_rest = bmin[:, NX:].clone(), bmax[:, NX:].clone()
        sync()
        t0 = time.perf_counter()
        cur, loss = x0, 0.0
        for t in range(args.T):
            x, _, status = layer(None, torch.cat([cur, lo_rest], 1), torch.cat([cur, hi_rest], 1))
            loss = loss + (x * x).sum()
            if t + 1 < args.T:
                cur = x[:, NX:2 * NX] + noise[args.warmup + t + 1]     # closed loop: the state the plan predicts, disturbed
        sync()
        t1 = time.perf_counter()
        epoch = bt.epoch
        loss.backward()
        sync()
        t2 = time.perf_counter()
        flags = layer.last_adjoint["flag"]
        res.update(T=args.T, ms_forward=1e3 * (t1 - t0), ms_backward=1e3 * (t2 - t1), ms_forward_per_step=1e3 * (t1 - t0) / args.T,
                   ms_backward_per_step=1e3 * (t2 - t1) / args.T, solved_last=int((status == 1).sum().item()),
                   flag0_first_step=int((flags == 0).sum().item()), grad_finite=bool(torch.isfinite(x0.grad).all().item()),
                   grad_absmax=float(x0.grad.abs().max().item()), epoch_moved_by_backward=bt.epoch - epoch)
        # what one backward step is made of: the call it makes (the bounds' gradients only, select = all) at the last point, timed on its own
        at = bt.solution_device() + (bt.active_device(),)
        sel = torch.ones((bt.B,), dtype=torch.int64, device=dev)
        outs = {k: bt._empty(*s) for k, s in dict(dbmin=((bt.B, bt.m),), dbmax=((bt.B, bt.m),), flag=((bt.B,), "int64"), resid=((bt.B,),),
                                                   passes=((bt.B,), "int64")).items()}
        gx = (2 * x).detach().contiguous()
        call = timed(lambda: bt.adjoint_device(gx, out=outs, select=sel, at=at), args.calls)
        res.update(ms_backward_call_alone_median=call["ms_per_call_median"], ms_backward_call_alone_min=call["ms_per_call_min"],
                   backward_call_max_passes=int(outs["passes"].max().item()), backward_call_flag0=int((outs["flag"] == 0).sum().item()))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's) for the `parent` step; without it that step is left out")
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--T", type=int, default=10, help="steps of the rollout")
    ap.add_argument("--limit", type=int, default=300, help="seconds each GPU step may take")
    ap.add_argument("--rehearse", action="store_true", help="run the steps on the host emulator (a check of this script; use a small --B)")
    ap.add_argument("--steps", default="active,adjoint,at,parent,rollout", help="the steps to run, of those above")
    ap.add_argument("--child", choices=STEPS + ("rollout",))
    args = ap.parse_args()
    if args.child:
        return child(args)
    steps = [s for s in STEPS if s != "parent" or args.lib] * args.runs + ["rollout"]
    steps = [s for s in steps if s in args.steps.split(",")]
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--B", str(args.B),
               "--calls", str(args.calls), "--warmup", str(args.warmup), "--T", str(args.T)] + (["--lib", os.path.abspath(args.lib)] if args.lib else []) + (["--rehearse"] if args.rehearse else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps(dict(step=step, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What a step on a subset of the members costs: the mpc-160 batch of `bench.py --workload mpc-160` (8192 QPs, one plant per 64, every QP its own
initial state) on tensors that stay on the GPU.

GPU steps, each a process of its own under `timeout -k 10` (a step that faults, aborts or runs out of time ends the chain: nothing more is started on
the device); the first two in turn, --runs times:

  scale     this build: the receding-horizon loop of tools/evidence/device_step_timing.py (new initial states, warm start from the last solution) as
            step_device without `select` ("full") and with select = every member, every 2nd, 8th and 64th ("1/1" .. "1/64"), each on a batch of its
            own, a block of --steps steps of each in turn, --blocks times; per configuration the medians over the blocks of wall ms per step (host clock
            around work that ends in a device synchronise), ms in the solve kernel (the library's events, last_solve_ms) and their difference.
            "select_none": ms per call of a subset step that selects nobody -- the selection launch and the read-back of the count, nothing else;
  parent    --lib (another build, the parent commit's): the "full" loop alone, the same protocol;
  pipeline  this build, once: the batch cold, "solve to 1e-3, polish with store, tighten the settings to 1e-9, subset step on the members the polish did
            not accept (flag != 0), warm-started from their stored solutions" against "solve cold to 1e-9": wall ms of every part, the number of members
            selected, and how many members end SOLVED.

No ratio is judged here: read the figures side by side, and the spread between the runs.

  python tools/evidence/subset_step_timing.py [--lib PARENT_BUILD.so] [--B 8192] [--steps 5] [--blocks 5] [--runs 2] [--limit 300]

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
FRACTIONS = (1, 2, 8, 64)


def once(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


class Loop:
    """one configuration: its own batch, bounds and noise stream; every = None: step_device without select"""

    def __init__(self, torch, ctx, probs, dev, every, seed):
        from qpalm_amd.solver import QpalmBatch
        self.torch, self.every = torch, every
        self.bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0))
        B = self.bt.B
        self.bmin = torch.from_numpy(np.stack([p.bmin for p in probs])).to(dev)
        self.bmax = torch.from_numpy(np.stack([p.bmax for p in probs])).to(dev)
        self.out = dict(x=self.bt._empty((B, self.bt.n)), y=self.bt._empty((B, self.bt.m)), status_val=self.bt._empty((B,), "int64"))
        self.select = None if every is None else (torch.arange(B, device=dev) % every == 0).to(torch.int64)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        rc, _ = self.bt.step_device(warm=None, out=self.out)
        assert rc == 0

    def step(self):
        x0 = self.bmin[:, :NX] + 0.1 * self.torch.randn((self.bt.B, NX), dtype=self.torch.float64, device=self.bmin.device, generator=self.gen)
        self.bmin[:, :NX] = x0
        self.bmax[:, :NX] = x0
        rc, _ = self.bt.step_device(self.bmin, self.bmax, warm="last", out=self.out, **({} if self.select is None else dict(select=self.select)))
        assert rc == 0

    def block(self, steps):
        self.torch.cuda.synchronize()
        kms = []
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
            kms.append(self.bt.last_solve_ms())
        self.torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, float(np.mean(kms))


def child(args):
    import torch
    from qpalm_amd.solver import Context, QpalmBatch
    from tools.evidence.device_step_timing import mpc_problems
    probs = mpc_problems(args.B, np.random.Generator(np.random.PCG64(2024)))
    if args.rehearse:   # the kernels on the host emulator: the script's own logic, no figure means anything
        from qpalm_amd import build
        ctx, dev = Context(0, lib_path=build.build_emu()), "cpu"
        torch.cuda.synchronize = lambda: None
    else:
        torch.cuda.init()
        ctx, dev = Context(0, lib_path=args.lib if args.child == "parent" else None), "cuda:0"
    res = dict(step=args.child, B=args.B, lib=args.lib if args.child == "parent" else "this build")
    if args.child in ("scale", "parent"):
        configs = {"full": None}
        if args.child == "scale":
            configs.update({"1/%d" % f: f for f in FRACTIONS})
        loops = {k: Loop(torch, ctx, probs, dev, every, 77) for k, every in configs.items()}
        rows = {k: [] for k in loops}
        for lp in loops.values():
            lp.block(args.warmup)
        for _ in range(args.blocks):
            for k, lp in loops.items():
                rows[k].append(lp.block(args.steps))
        for k, r in rows.items():
            wall, kern = [v[0] for v in r], [v[1] for v in r]
            res[k] = dict(selected=loops[k].bt.B if loops[k].select is None else int(loops[k].select.sum().item()),
                          wall_ms_per_step=statistics.median(wall), kernel_ms_per_step=statistics.median(kern),
                          outside_kernel_ms_per_step=statistics.median([w - q for w, q in zip(wall, kern)]), wall_blocks=wall,
                          solved=int((loops[k].out["status_val"] == 1).sum().item()))
        if args.child == "scale":
            lp = loops["1/64"]
            nobody = torch.zeros_like(lp.select)
            ms = [once(lambda: lp.bt.step_device(lp.bmin, lp.bmax, warm="last", out=lp.out, select=nobody)) for _ in range(2 + 20)][2:]
            res["select_none"] = dict(ms_per_call_median=statistics.median(ms), ms_per_call_min=min(ms), ms_per_call_max=max(ms))
        print(json.dumps(res), flush=True)
        return
    # ---- pipeline ----
    bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=1e-3, eps_rel=1e-3, verbose=0))
    B = bt.B
    out = dict(x=bt._empty((B, bt.n)), y=bt._empty((B, bt.m)), status_val=bt._empty((B,), "int64"))
    pol = dict(flag=bt._empty((B,), "int64"))
    setting = lambda e: bt.update_settings(ctx.default_settings(eps_abs=e, eps_rel=e, verbose=0))
    arms = {"cold_1e-9": [], "cold_1e-3": [], "polish_store": [], "subset_1e-9": []}
    selected = solved_a = solved_b = None
    for k in range(1 + args.calls):                             # the first round is not timed: the first launch of every shape
        setting(1e-9)
        t = [once(lambda: bt.step_device(warm=None, out=out))]
        solved_b = int((out["status_val"] == 1).sum().item())
        setting(1e-3)
        t.append(once(lambda: bt.step_device(warm=None, out=out)))
        t.append(once(lambda: bt.polish_device(store=True, out=pol)))
        sel = (pol["flag"] != 0).to(torch.int64)
        torch.cuda.synchronize()
        setting(1e-9)
        t.append(once(lambda: bt.step_device(warm="last", out=out, select=sel)))
        selected, solved_a = int(sel.sum().item()), int((out["status_val"] == 1).sum().item())
        if k:
            for name, v in zip(arms, t):
                arms[name].append(v)
    res.update({name: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for name, v in arms.items()})
    tot = [a + b + c for a, b, c in zip(arms["cold_1e-3"], arms["polish_store"], arms["subset_1e-9"])]
    res.update(pipeline_total_ms_median=statistics.median(tot), cold_1e9_total_ms_median=statistics.median(arms["cold_1e-9"]), selected=selected,
               solved_after_pipeline=solved_a, solved_after_cold_1e9=solved_b, calls=args.calls)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's) for the `parent` step; without it that step is left out")
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds each GPU step may take")
    ap.add_argument("--rehearse", action="store_true", help="run the steps on the host emulator (a check of this script; use a small --B)")
    ap.add_argument("--child", choices=("scale", "parent", "pipeline"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    steps = [s for s in ("scale", "parent") if s != "parent" or args.lib] * args.runs + ["pipeline"]
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--B", str(args.B), "--steps", str(args.steps),
               "--blocks", str(args.blocks), "--warmup", str(args.warmup), "--calls", str(args.calls)] \
            + (["--lib", os.path.abspath(args.lib)] if args.lib else []) + (["--rehearse"] if args.rehearse else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps(dict(step=step, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What K directions cost in one multi call, next to K single calls: the mpc-160 batch of `bench.py --workload mpc-160` (8192 QPs,
one plant per 64, every QP its own initial state), brought to the state tools/evidence/tangent_timing.py times (a cold step and --warmup warm steps on
tensors that stay on the GPU).

GPU steps, each a process of its own under `timeout -k 10` (a step that faults, aborts or runs out of time ends the chain: nothing more is started on
the device), the two builds in turn, --runs times; inside a step the penalty floor (QpalmBatch.sens_penalty) is 0 and then 1e6:

  other   --lib (the other build: the parent commit's): the single adjoint call (gx = ones, gy random, every output wanted) and the single tangent call
          (all five inputs, dx, dy and every flag wanted);
  this    this build: the same two single calls, and for K in --ks the multi call on K random directions next to K single calls on its K slices, for
          the tangent (all five inputs) and for the adjoint (every output).

Per figure: wall ms (host clock around calls that end in a device synchronise), median of --calls repetitions after two untimed ones.  No ratio is
judged here: the table is the result.

  python tools/evidence/multi_direction_timing.py --lib PARENT_BUILD.so [--B 8192] [--calls 10] [--runs 2] [--limit 420] [--out timing.md]

--rehearse runs the same script on the host emulator (with --lib an emulator build and a small --B): it tries the script out, its figures mean nothing.

One JSON line per step; at the end the table in markdown (to --out as well)."""
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
FLOORS = (0.0, 1e6)


def timed(fn, calls):
    ms = []
    for k in range(2 + calls):
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            ms.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def child(args):
    import torch
    if not args.rehearse:
        torch.cuda.init()
    from qpalm_amd import build
    from qpalm_amd.solver import Context, QpalmBatch
    from tools.evidence.device_step_timing import mpc_problems
    rng = np.random.Generator(np.random.PCG64(2024))
    probs = mpc_problems(args.B, rng)
    ctx = Context(0, lib_path=args.lib if args.child == "other" else (build.build_emu() if args.rehearse else None))
    bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0))
    dev = "cpu" if args.rehearse else "cuda:0"
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
    B, n, m = bt.B, bt.n, bt.m
    ks = [int(k) for k in args.ks.split(",")] if args.child == "this" else [1]
    kmax = max(ks)
    gen = torch.Generator(device="cpu").manual_seed(7)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, generator=gen).to(dev)
    tan_in = dict(dq=rnd(kmax, B, n), dbmin=rnd(kmax, B, m), dbmax=rnd(kmax, B, m), dQx=rnd(kmax, B, bt.nnzQ), dAx=rnd(kmax, B, bt.nnzA))
    gx, gy = rnd(kmax, B, n), rnd(kmax, B, m)
    gx[0] = 1.0
    adj_shapes = dict(dq=((B, n),), dbmin=((B, m),), dbmax=((B, m),), dQx=((B, bt.nnzQ),), dAx=((B, bt.nnzA),), active=((B, m), "int64"), flag=((B,), "int64"),
                      resid=((B,),), passes=((B,), "int64"))
    tan_shapes = dict(dx=((B, n),), dy=((B, m),), active=((B, m), "int64"), flag=((B,), "int64"), resid=((B,),), passes=((B,), "int64"))

    def outs(shapes, K=None):
        lead = lambda k, s: s if (K is None or k == "active") else (K,) + s
        return {k: bt._empty(lead(k, s[0]), *s[1:]) for k, s in shapes.items()}
    flags = lambda o: dict(flag0=int((o["flag"] == 0).sum().item()), flag1=int((o["flag"] == 1).sum().item()), flag2=int((o["flag"] == 2).sum().item()),
                           max_passes=int(o["passes"].max().item()))
    res = dict(step=args.child, lib=(args.lib if args.child == "other" else "this build"), B=B, n=n, m=m, solved=int((out["status_val"] == 1).sum().item()), floors={})
    a1, t1 = outs(adj_shapes), outs(tan_shapes)
    for floor in FLOORS:
        bt.sens_penalty = floor
        r = {}
        r["adjoint_single"] = dict(timed(lambda: bt.adjoint_device(gx[0], gy[0], out=a1), args.calls), **flags(a1))
        r["tangent_single"] = dict(timed(lambda: bt.tangent_device(**{k: v[0] for k, v in tan_in.items()}, out=t1), args.calls), **flags(t1))
        for K in (ks if args.child == "this" else []):
            aK, tK = outs(adj_shapes, K), outs(tan_shapes, K)
            gxK, gyK = gx[:K].contiguous(), gy[:K].contiguous()
            tinK = {k: v[:K].contiguous() for k, v in tan_in.items()}

            def adjoint_singles():
                for k in range(K):
                    bt.adjoint_device(gxK[k], gyK[k], out=a1)

            def tangent_singles():
                for k in range(K):
                    bt.tangent_device(**{key: v[k] for key, v in tinK.items()}, out=t1)
            r["adjoint_multi_K%d" % K] = dict(timed(lambda: bt.adjoints_device(gxK, gyK, out=aK), args.calls), **flags(aK))
            r["adjoint_singles_K%d" % K] = timed(adjoint_singles, args.calls)
            r["tangent_multi_K%d" % K] = dict(timed(lambda: bt.tangents_device(**tinK, out=tK), args.calls), **flags(tK))
            r["tangent_singles_K%d" % K] = timed(tangent_singles, args.calls)
            # the last single call worked on slice K - 1: the multi call's slice holds its bits
            assert torch.equal(aK["dq"][K - 1], a1["dq"]) and torch.equal(tK["dx"][K - 1], t1["dx"]), "slice K - 1 is not the single call"
            del aK, tK
        res["floors"][repr(floor)] = r
    print(json.dumps(res), flush=True)


def table(got, ks):
    """markdown: per floor and run, the single calls of the two builds, then per K the multi call next to K single calls"""
    L = []
    f = lambda v: "%.2f" % v
    for floor in FLOORS:
        L.append("### penalty floor %g" % floor)
        L.append("")
        L.append("Single calls, ms per call (median): the other build (the parent commit) next to this build.")
        L.append("")
        L.append("| run | adjoint, other build | adjoint, this build | tangent, other build | tangent, this build | passes (max) adjoint / tangent |")
        L.append("|---|---|---|---|---|---|")
        for r in range(len(got["this"])):
            t = got["this"][r]["floors"][repr(floor)]
            o = got["other"][r]["floors"][repr(floor)] if got["other"] else None
            L.append("| %d | %s | %s | %s | %s | %d / %d |" % (r + 1, f(o["adjoint_single"]["ms_median"]) if o else "-", f(t["adjoint_single"]["ms_median"]),
                                                             f(o["tangent_single"]["ms_median"]) if o else "-", f(t["tangent_single"]["ms_median"]),
                                                             t["adjoint_single"]["max_passes"], t["tangent_single"]["max_passes"]))
        L.append("")
        L.append("K directions, ms (median): one multi call next to K single calls of this build, per run.")
        L.append("")
        L.append("| K | run | tangent multi | tangent K singles | adjoint multi | adjoint K singles | flag 0 / 1 / 2 of the multi calls (tangent; adjoint) |")
        L.append("|---|---|---|---|---|---|---|")
        for K in ks:
            for r in range(len(got["this"])):
                t = got["this"][r]["floors"][repr(floor)]
                tm, am = t["tangent_multi_K%d" % K], t["adjoint_multi_K%d" % K]
                L.append("| %d | %d | %s | %s | %s | %s | %d / %d / %d; %d / %d / %d |" %
                         (K, r + 1, f(tm["ms_median"]), f(t["tangent_singles_K%d" % K]["ms_median"]), f(am["ms_median"]), f(t["adjoint_singles_K%d" % K]["ms_median"]),
                          tm["flag0"], tm["flag1"], tm["flag2"], am["flag0"], am["flag1"], am["flag2"]))
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--limit", type=int, default=420, help="seconds each GPU step may take")
    ap.add_argument("--lib", default=None, help="the other build (the parent commit's), whose single calls are timed")
    ap.add_argument("--out", default=None, help="where the markdown table goes (besides the standard output)")
    ap.add_argument("--rehearse", action="store_true", help="on the host emulator (--lib: an emulator build), to try the script out: use a small --B")
    ap.add_argument("--child", choices=("other", "this"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    got = {"other": [], "this": []}
    for _ in range(args.runs):
        for step in (("other", "this") if args.lib else ("this",)):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--B", str(args.B),
                   "--calls", str(args.calls), "--warmup", str(args.warmup), "--ks", args.ks] + (["--lib", args.lib] if args.lib else []) + (["--rehearse"] if args.rehearse else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:
                print(json.dumps(dict(step=step, failed=r.returncode)))
                return r.returncode
            got[step].append(json.loads(r.stdout.strip().splitlines()[-1]))
    t0 = got["this"][0]
    md = ("mpc-160, B = %d (n = %d, m = %d), %d solved; median of %d calls; %d runs on one box.\n\n" % (t0["B"], t0["n"], t0["m"], t0["solved"], args.calls, args.runs)
          + table(got, [int(k) for k in args.ks.split(",")]))
    print(md)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(md + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

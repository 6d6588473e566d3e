#!/usr/bin/env python3
"""How many refinement passes the sensitivity solves take with a penalty floor (QpalmBatch.sens_penalty): for every floor in
--floors, the histogram of `passes`, the count of each flag and the largest `resid` over a batch, for the adjoint (gx = ones), the tangent (a random
direction of the bounds) and the polish (no store); before them, per batch, the penalties over the rows of J of the first 64 members.  The batches:

  mpc-160 @ 1e-3, mpc-160 @ 1e-6   the generator of `bench.py --workload mpc-160` (one plant per 64 members, every member its own initial state),
                                   --B members, after a cold solve to that tolerance;
  planted                          the planted problems of tests/adjoint_refs.py at the sizes of tests/test_adjoint.py's CASES up to --nmax, one
                                   batch per case, solved to 1e-9 (and the active set handed in, as the tests do).

On the GPU every batch is a process of its own under `timeout -k 10` (a step that faults, aborts or runs out of time ends the chain); --emu runs the
same on the host emulator (a library built for it; use a small --B).

  python tools/evidence/sens_penalty_passes.py [--B 8192] [--floors 0,1e4,1e6,1e8] [--nmax 257] [--emu] [--limit 300]

One JSON line per batch and floor."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def summary(out, torch):
    vals, counts = torch.unique(out["passes"], return_counts=True)
    flag = out["flag"]
    return dict(passes={int(v): int(c) for v, c in zip(vals.tolist(), counts.tolist())}, passes_sum=int(out["passes"].sum().item()),
                flags={int(f): int((flag == f).sum().item()) for f in range(4) if int((flag == f).sum().item())}, resid_max=float(out["resid"].max().item()))


def child(a):
    import torch
    from qpalm_amd.solver import Context, QpalmBatch
    if a.emu:
        from qpalm_amd import build
        ctx, dev = Context(0, lib_path=build.build_emu()), "cpu"
    else:
        torch.cuda.init()
        ctx, dev = Context(0), "cuda:0"
    put = lambda v, dt=np.float64: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)
    floors = [float(f) for f in a.floors.split(",")]
    rng = np.random.default_rng(7)

    def report(name, bt, sides):
        act = None if sides is None else put(sides, np.int64)
        gx = torch.ones((bt.B, bt.n), dtype=torch.float64, device=dev)
        db = put(rng.standard_normal((bt.B, bt.m)))
        dq = put(rng.standard_normal((bt.B, bt.n)))
        want = ("flag", "resid", "passes")
        # the penalties the floor acts on: sigma over the rows of J (the set the calls use), first 64 members
        bt.sens_penalty = 0.0
        J = bt.adjoint_device(gx, active=act, want=("active",))["active"].cpu().numpy() != 0
        sig = np.concatenate([bt.vec("sigma", b)[J[b]] for b in range(min(bt.B, 64))])
        if sig.size:
            print(json.dumps(dict(batch=name, rows_of_J=int(sig.size), members=min(bt.B, 64), sigma_J_min=float(sig.min()), sigma_J_median=float(np.median(sig)),
                                  sigma_J_max=float(sig.max()), sigma_J_below_1e6=int((sig < 1e6).sum()))), flush=True)
        for floor in floors:
            bt.sens_penalty = floor
            calls = dict(adjoint=bt.adjoint_device(gx, active=act, want=want), tangent=bt.tangent_device(dq=dq, dbmin=db, dbmax=db, active=act, want=want),
                         polish=bt.polish_device(act, want=want + ("x",)))
            print(json.dumps(dict(batch=name, backend=ctx.backend, B=bt.B, n=bt.n, m=bt.m, floor=floor, **{k: summary(v, torch) for k, v in calls.items()})),
                  flush=True)

    if a.child.startswith("mpc"):
        from tools.evidence.device_step_timing import mpc_problems
        eps = float(a.child.split("@")[1])
        probs = mpc_problems(a.B, np.random.Generator(np.random.PCG64(2024)))
        bt = QpalmBatch(ctx, probs, ctx.default_settings(eps_abs=eps, eps_rel=eps, verbose=0))
        bt.solve()
        print(json.dumps(dict(batch=a.child, solved=int((bt.statuses() == 1).sum()))), flush=True)
        report(a.child, bt, None)
    else:
        from tests import adjoint_refs as R
        from tests.sens_helpers import CASES, ST
        for c in CASES:
            if c.n > a.nmax:
                continue
            p, side, xs, ys = R.planted_qp(c.n, c.m, c.nact, 9000 + 7 * c.n + c.nact, sides=c.sides, equality=c.equality)
            bt = QpalmBatch(ctx, [p], ctx.default_settings(**dict(ST, scaling=c.scaling, proximal=c.proximal)))
            if c.n >= 192:
                bt.warm_start(xs[None, :], ys[None, :])
            bt.solve()
            report("planted-" + c.id, bt, side[None, :])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--floors", default="0,1e4,1e6,1e8")
    ap.add_argument("--nmax", type=int, default=257)
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--limit", type=int, default=300, help="seconds each step may take")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for step in ("mpc@1e-3", "mpc@1e-6", "planted"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--B", str(a.B), "--floors", a.floors,
               "--nmax", str(a.nmax)] + (["--emu"] if a.emu else [])
        r = subprocess.run(cmd)
        if r.returncode != 0:
            print(json.dumps(dict(step=step, failed=r.returncode)), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Does a first-order predictor pay on the receding-horizon loop?  The mpc-160 loop of tools/evidence/device_step_timing.py (8192 QPs, new initial
states every step, everything on the GPU) driven on three batches set up from the same problems, with the same disturbances:

  last       step_device(bmin, bmax, warm="last"): every QP starts from its own last solution;
  last_xy    the same start handed over as arrays, step_device(bmin, bmax, warm=(x, y)): what the predicted loop does, without the prediction;
  predicted  tangent_device(dbmin = dbmax = new bounds - old bounds) on the solved batch, then step_device(bmin, bmax, warm=(x + dx, y + dy)).

Per loop: mean iteration count over the timed steps, wall ms per step (host clock around work that ends in a device synchronise; the
predicted loop's figure includes the tangent call and the two additions), solve-kernel ms per step, and for the predicted loop the tangent's flags.
The loops take turns in blocks of --steps steps; figures are medians over --blocks blocks.  A report, not a gate.

  python tools/evidence/tangent_predictor.py [--B 8192] [--steps 5] [--blocks 5] [--sens-penalty FLOOR]

--sens-penalty: the penalty floor of the tangent's preconditioner (QpalmBatch.sens_penalty) on the predicted loop's batch.

One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NX = 10


class Loop:
    def __init__(self, torch, ctx, probs, st, predict):
        from qpalm_amd.solver import QpalmBatch
        self.torch, self.bt, self.predict = torch, QpalmBatch(ctx, probs, st), predict
        bt, dev = self.bt, "cuda:%d" % ctx.device
        self.bmin = torch.from_numpy(np.stack([p.bmin for p in probs])).to(dev)
        self.bmax = torch.from_numpy(np.stack([p.bmax for p in probs])).to(dev)
        self.out = dict(x=bt._empty((bt.B, bt.n)), y=bt._empty((bt.B, bt.m)), iter=bt._empty((bt.B,), "int64"), status_val=bt._empty((bt.B,), "int64"))
        self.tan = dict(dx=bt._empty((bt.B, bt.n)), dy=bt._empty((bt.B, bt.m)), flag=bt._empty((bt.B,), "int64"))
        self.db = torch.zeros_like(self.bmin)
        self.iters, self.flagged = [], 0
        rc, _ = bt.step_device(warm=None, out=self.out)
        assert rc == 0

    def step(self, noise):
        x0 = self.bmin[:, :NX] + 0.1 * noise
        if self.predict is True:
            self.db[:, :NX] = x0 - self.bmin[:, :NX]
        self.bmin[:, :NX] = x0
        self.bmax[:, :NX] = x0
        if self.predict is True:
            self.bt.tangent_device(dbmin=self.db, dbmax=self.db, out=self.tan)
            warm = (self.out["x"] + self.tan["dx"], self.out["y"] + self.tan["dy"])
        elif self.predict == "xy":
            warm = (self.out["x"].clone(), self.out["y"].clone())
        else:
            warm = "last"
        rc, _ = self.bt.step_device(self.bmin, self.bmax, warm=warm, out=self.out)
        assert rc == 0

    def block(self, noises, record):
        torch = self.torch
        torch.cuda.synchronize()
        kms, t0 = [], time.perf_counter()
        for nz in noises:
            self.step(nz)
            kms.append(self.bt.last_solve_ms())
            if record:
                self.iters.append(self.out["iter"].double().mean().item())
                self.flagged += int((self.tan["flag"] != 0).sum().item()) if self.predict is True else 0
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(noises), float(np.mean(kms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--sens-penalty", type=float, default=0.0)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU fallback"
    torch.cuda.init()
    from qpalm_amd.solver import Context
    from tools.evidence.device_step_timing import mpc_problems
    ctx = Context(0)
    rng = np.random.default_rng(12345)
    probs = mpc_problems(a.B, rng)
    st = ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    loops = {"last": Loop(torch, ctx, probs, st, False), "last_xy": Loop(torch, ctx, probs, st, "xy"), "predicted": Loop(torch, ctx, probs, st, True)}
    loops["predicted"].bt.sens_penalty = a.sens_penalty
    rows = {k: [] for k in loops}
    for blk in range(a.blocks + 1):                          # block 0: warm-up, not recorded
        noises = [torch.from_numpy(rng.standard_normal((a.B, NX))).to("cuda:0") for _ in range(a.steps)]
        for k, lp in loops.items():                          # a block of each in turn, on the same disturbances
            r = lp.block(noises, blk > 0)
            if blk > 0:
                rows[k].append(r)
    out = dict(tool="tangent_predictor", workload="mpc-160", B=a.B, steps=a.steps, blocks=a.blocks, sens_penalty=a.sens_penalty)
    for k, lp in loops.items():
        out[k] = dict(mean_iterations=float(np.mean(lp.iters)), wall_ms_per_step=statistics.median(r[0] for r in rows[k]),
                      wall_blocks=[r[0] for r in rows[k]], solve_kernel_ms_per_step=statistics.median(r[1] for r in rows[k]),
                      all_solved=bool((lp.out["status_val"] == 1).all().item()))
    out["predicted"]["tangent_flagged_members"] = loops["predicted"].flagged
    out["final_x_max_difference"] = float((loops["last"].out["x"] - loops["predicted"].out["x"]).abs().max().item())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

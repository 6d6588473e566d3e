#!/usr/bin/env python3
"""What the device forms of the per-step calls save on the receding-horizon loop: the mpc-160 batch of `bench.py --workload mpc-160` (8192 QPs, one
plant per 64, every QP its own initial state) driven twice in one process, on two batches set up from the same problems:

  host    the loop as bench.py writes it: page-locked arrays, update_bounds, warm_start_last, solve, solution(out=...);
  device  step_device on torch tensors that never leave the GPU (the new initial states are computed in torch).

Both loops see the same seeds, hence the same bounds bit for bit, and the same number of warm-up and timed steps; the timed steps come in --blocks
blocks of --steps steps, a block of the host loop and a block of the device loop in turn, and every figure is the median over the blocks.  Per loop:
wall ms per step (host clock around work that ends in a device synchronise), kernel ms per step (the library's events around the solve launch,
last_solve_ms) and their difference -- everything a step spends outside the solve kernel.  `controller_ms` is the part of the wall time spent computing
the new bounds (host: drawing the disturbance and writing the page-locked arrays; device: enqueuing the torch operations; the disturbance of the device
loop is uploaded before its block starts).  At the end the two loops' x and y must be equal bit for bit.

  python tools/evidence/device_step_timing.py [--lib OTHER_BUILD.so]

--lib times another build of the library; one without qpg_batch_step_device (the parent commit's) runs the host loop alone.  One JSON line."""
import argparse
import copy
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NX, NU, T = 10, 5, 10


def mpc_problems(B, rng):
    """the construction of bench.py's mpc-160 workload (rank 0)"""
    from qpalm_amd.problems import random_mpc_qp
    plants, probs = {}, []
    for k in range(B):
        seed = k // 64
        if seed not in plants:
            plants[seed] = random_mpc_qp(T=T, nx=NX, nu=NU, seed=seed)
        base = plants[seed]
        x0 = 2.0 * (2 * rng.random(NX) - 1)
        bmin, bmax = base.bmin.copy(), base.bmax.copy()
        bmin[:NX] = x0
        bmax[:NX] = x0
        probs.append(type(base)(base.n, base.m, base.Qp, base.Qi, base.Qx, base.Ap, base.Ai, base.Ax, base.q, bmin, bmax))
    return probs


class HostLoop:
    def __init__(self, ctx, probs, rng, st):
        from qpalm_amd.solver import QpalmBatch
        self.bt, self.rng, self.B = QpalmBatch(ctx, probs, st), rng, len(probs)
        n, m = probs[0].n, probs[0].m
        self.bmin, self.bmax = ctx.pinned_array((self.B, m)), ctx.pinned_array((self.B, m))
        self.bmin[:] = np.stack([p.bmin for p in probs])
        self.bmax[:] = np.stack([p.bmax for p in probs])
        self.sol = (ctx.pinned_array((self.B, n)), ctx.pinned_array((self.B, m)))
        self.first, self.ctrl = True, 0.0

    def prepare(self, steps):
        pass

    def step(self):
        bt = self.bt
        if self.first:
            bt.warm_start(None, None)
            self.first = False
        else:
            t0 = time.perf_counter()
            x0 = self.bmin[:, :NX] + 0.1 * self.rng.standard_normal((self.B, NX))
            self.bmin[:, :NX] = x0
            self.bmax[:, :NX] = x0
            self.ctrl += time.perf_counter() - t0
            if bt.update_bounds(self.bmin, self.bmax) != 0:
                raise RuntimeError("update_bounds rejected the new bounds")
            bt.warm_start_last()
        bt.solve()
        bt.solution(out=self.sol)

    def result(self):
        return np.array(self.sol[0]), np.array(self.sol[1])


class DeviceLoop:
    def __init__(self, ctx, probs, rng, st):
        import torch
        from qpalm_amd.solver import QpalmBatch
        self.torch, self.bt, self.rng, self.B = torch, QpalmBatch(ctx, probs, st), rng, len(probs)
        n, m = probs[0].n, probs[0].m
        dev = "cuda:%d" % ctx.device
        self.bmin = torch.from_numpy(np.stack([p.bmin for p in probs])).to(dev)
        self.bmax = torch.from_numpy(np.stack([p.bmax for p in probs])).to(dev)
        self.out = dict(x=torch.zeros((self.B, n), dtype=torch.float64, device=dev), y=torch.zeros((self.B, m), dtype=torch.float64, device=dev))
        self.first, self.ctrl, self.noise, self.dev = True, 0.0, [], dev

    def prepare(self, steps):
        """the disturbances of the next `steps` steps, drawn as the host loop draws them, put on the device (outside the timed window)"""
        k = steps - (1 if self.first else 0)
        self.noise = [self.torch.from_numpy(self.rng.standard_normal((self.B, NX))).to(self.dev) for _ in range(k)]
        self.torch.cuda.synchronize()

    def step(self):
        if self.first:
            rc, _ = self.bt.step_device(warm=None, out=self.out)
            self.first = False
        else:
            t0 = time.perf_counter()
            x0 = self.bmin[:, :NX] + 0.1 * self.noise.pop(0)
            self.bmin[:, :NX] = x0
            self.bmax[:, :NX] = x0
            self.ctrl += time.perf_counter() - t0
            rc, _ = self.bt.step_device(self.bmin, self.bmax, warm="last", out=self.out)
        if rc != 0:
            raise RuntimeError("step_device: %d" % rc)

    def result(self):
        return self.out["x"].cpu().numpy(), self.out["y"].cpu().numpy()


def block(loop, steps, torch):
    """(wall ms per step, kernel ms per step, controller ms per step) of `steps` steps"""
    loop.prepare(steps)
    torch.cuda.synchronize()
    loop.ctrl = 0.0
    kms = []
    t0 = time.perf_counter()
    for _ in range(steps):
        loop.step()
        kms.append(loop.bt.last_solve_ms())
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    return wall, float(np.mean(kms)), loop.ctrl * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU fallback"
    torch.cuda.init()
    from qpalm_amd.solver import Context
    ctx = Context(0, lib_path=a.lib)
    assert ctx.backend == "gfx950-hip"
    rng = np.random.default_rng(12345)
    probs = mpc_problems(a.B, rng)
    st = ctx.default_settings(eps_abs=1e-6, eps_rel=1e-6, verbose=0)
    loops = {"host": HostLoop(ctx, probs, copy.deepcopy(rng), st)}
    if hasattr(ctx.L, "qpg_batch_step_device"):
        loops["device"] = DeviceLoop(ctx, probs, copy.deepcopy(rng), st)
    prop = torch.cuda.get_device_properties(0)
    out = dict(tool="device_step_timing", lib=a.lib or "this build", B=a.B, n=probs[0].n, m=probs[0].m, steps=a.steps, warmup=a.warmup, blocks=a.blocks,
               box="%s / %s / %s" % (socket.gethostname(), prop.name, getattr(prop, "uuid", "")))
    rows = {k: [] for k in loops}
    if a.warmup:
        for lp in loops.values():
            block(lp, a.warmup, torch)
    for _ in range(a.blocks):
        for k, lp in loops.items():      # a block of each in turn
            rows[k].append(block(lp, a.steps, torch))
    for k, r in rows.items():
        wall, kern = [v[0] for v in r], [v[1] for v in r]
        out[k] = dict(wall_ms_per_step=statistics.median(wall), kernel_ms_per_step=statistics.median(kern),
                      outside_kernel_ms_per_step=statistics.median([w - q for w, q in zip(wall, kern)]),
                      controller_ms_per_step=statistics.median([v[2] for v in r]), wall_blocks=wall, kernel_blocks=kern)
        if not all(int(v) == 1 for v in loops[k].bt.statuses()):
            raise RuntimeError("%s loop: not every QP solved" % k)
    if "device" in loops:
        (xh, yh), (xd, yd) = loops["host"].result(), loops["device"].result()
        out["final_iterates_bit_equal"] = bool(np.array_equal(xh, xd) and np.array_equal(yh, yd))
        out["wall_saved_ms_per_step"] = out["host"]["wall_ms_per_step"] - out["device"]["wall_ms_per_step"]
    print(json.dumps(out), flush=True)
    if out.get("final_iterates_bit_equal") is False:
        sys.exit("the two loops' final x, y differ")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Is the adjoint still, bit for bit, what another build of the library computes?  A fixed set of adjoint calls -- the problems, settings and inputs of
tests/test_adjoint.py's sizes (case 1), batches (case 2) and sparse-factor cases -- and one line per call with a SHA-256 of every output array.  Run it on
two builds and compare the lines:

  python tools/evidence/adjoint_hashes.py [--lib OTHER_BUILD.so] > hashes.txt

(a library built for the host emulator works too: the tensors then stay on the CPU).  The last line hashes all the lines before it."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KEYS = ("dq", "dbmin", "dbmax", "dQx", "dAx", "active", "flag", "resid", "passes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from qpalm_amd.solver import Context, QpalmBatch
    from tests import adjoint_refs as R
    from tests.sparse_gadgets import blocks_qp, gadget_qp
    from tests.sens_helpers import CASES, ST, padded
    ctx = Context(0, lib_path=a.lib)
    dev = "cpu" if ctx.backend == "host-emulation" else "cuda:0"
    put = lambda v, dt=np.float64: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)
    lines = []

    def run(name, probs, sides, seed, warm=None, **st):
        bt = QpalmBatch(ctx, probs, ctx.default_settings(**dict(ST, **st)))
        if warm is not None:
            bt.warm_start(*warm)
        bt.solve()
        rng = np.random.default_rng(seed)
        gx, gy = rng.standard_normal((bt.B, bt.n)), rng.standard_normal((bt.B, bt.m))
        for how, act in (("given", put(sides, np.int64)), ("rule", None)):
            out = bt.adjoint_device(put(gx), put(gy), act)
            h = " ".join("%s=%s" % (k, hashlib.sha256(out[k].cpu().numpy().tobytes()).hexdigest()[:16]) for k in KEYS)
            lines.append("%s %s flags=%s %s" % (name, how, "".join(str(int(f)) for f in out["flag"].cpu()), h))
            print(lines[-1], flush=True)

    for c in CASES:
        p, side, xs, ys = R.planted_qp(c.n, c.m, c.nact, 9000 + 7 * c.n + c.nact, sides=c.sides, equality=c.equality)
        warm = (xs[None, :], ys[None, :]) if c.n >= 192 else None
        run(c.id, [p], side[None, :], c.n, warm=warm, scaling=c.scaling, proximal=c.proximal)
    for shape in ("mixed", "B9-slots4", "B9-slots2"):
        ctx.set_option("max_slots", 2 if shape == "B9-slots2" else (4 if shape == "B9-slots4" else 512))
        dims = [(33, 50, 20), (20, 30, 7), (5, 8, 3)] if shape == "mixed" else [(12, 20, 2 + k % 6) for k in range(9)]
        planted = [R.planted_qp(n, m, k, 9500 + 11 * b) for b, (n, m, k) in enumerate(dims)]
        run(shape, [q[0] for q in planted], padded([q[1] for q in planted], max(d[1] for d in dims), np.int64), 5, scaling=10)
    ctx.set_option("max_slots", 512)
    base, side, _, _ = R.planted_qp(12, 20, 5, 9600)         # the caller's order of the entries (the value maps)
    run("order", [R.shuffled_entries(base, 3)], side[None, :], 6, scaling=10)
    ctx.set_option("sparse_factor", 1)
    for kind in ("blocks", "banded"):
        base = blocks_qp(43, 2)[0] if kind == "blocks" else gadget_qp((), 4105, 5, cliques=False, stars=False, arrow=False, single=False, band=12)[0]
        p, side, _, _ = R.replant(base, min(base.n - 1, base.m) // 2, 77)
        run("sparse-" + kind, [p], side[None, :], 3, scaling=10)
    print("all %s" % hashlib.sha256("\n".join(lines).encode()).hexdigest())


if __name__ == "__main__":
    main()

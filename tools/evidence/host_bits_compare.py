"""Same bits on the host side: two builds of the emulator library (say a parent commit's and this tree's) set up the same batches, each in a
process of its own, and everything the host-side conversion and symbolic analysis produce is compared with array_equal.

  python tools/evidence/host_bits_compare.py --a /path/to/parent/libqpalm_gfx950_emu.so --b tests/emu/libqpalm_gfx950_emu.so

Per batch member: sparse_perm and the tree's height, sparse_info's nnz(L), sparse_factor's Lp / Li, sparse_coop_info (Schur cases run with
sparse_coop = 1), the named arrays Ap .. Qfperm, A_values, Q_values after setup, and A_values / Q_values after one update_Q_A with new values."""
import argparse
import dataclasses
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

INT_ARRAYS = ("Ap", "Ai", "Atp", "Ati", "Atperm", "Ainv", "Qp", "Qi", "Qfp", "Qfi", "Qfperm")


def unsorted_full(p):
    """p with Q in full storage (both triangles) and the entries of every column of Q and A in descending row order"""
    import scipy.sparse as sp
    Q = sp.csc_matrix(p.Q_full())
    Q.sort_indices()
    A = sp.csc_matrix(p.A_mat())
    A.sort_indices()

    def rev(M):
        idx, val = M.indices.copy(), M.data.copy()
        for j in range(M.shape[1]):
            s = slice(M.indptr[j], M.indptr[j + 1])
            idx[s], val[s] = idx[s][::-1], val[s][::-1]
        return M.indptr.astype(np.int64), idx.astype(np.int64), val.astype(np.float64)
    Qp, Qi, Qx = rev(Q)
    Ap, Ai, Ax = rev(A)
    return dataclasses.replace(p, Qp=Qp, Qi=Qi, Qx=Qx, Ap=Ap, Ai=Ai, Ax=Ax)


def cases():
    """(name, problems, context options, settings)"""
    from qpalm_amd.problems import sparse_qp
    from tests.sparse_gadgets import gadget_qp
    out = []
    for kind in ("banded", "arrow", "blocks"):
        for n in (96, 300, 2000):
            for ordering in (-1, 0, 1):
                p = sparse_qp(n, kind, seed=n + ordering)
                out.append(("%s n=%d ordering=%d schur" % (kind, n, ordering), [p], dict(sparse_factor=1, sparse_ordering=ordering, sparse_coop=1), dict(factorization_method=1)))
                out.append(("%s n=%d ordering=%d kkt" % (kind, n, ordering), [p], dict(sparse_kkt=1, sparse_ordering=ordering), dict(factorization_method=0)))
    for ordering in (0, 1):
        g = gadget_qp([8, 16], 7, 3, band=48)[0]
        out.append(("gadgets ordering=%d schur" % ordering, [g], dict(sparse_factor=1, sparse_ordering=ordering, sparse_coop=1), dict(factorization_method=1)))
        gb = gadget_qp([8], 9, 3, band=48, budget=True)[0]
        out.append(("gadgets+budget ordering=%d kkt" % ordering, [gb], dict(sparse_kkt=1, sparse_ordering=ordering), dict(factorization_method=0)))
    mixed = [sparse_qp(96, "banded", seed=1), sparse_qp(300, "arrow", seed=2), sparse_qp(200, "blocks", seed=3), sparse_qp(520, "banded", seed=4)]
    out.append(("mixed sizes schur", mixed, dict(sparse_factor=1, sparse_ordering=-1, sparse_coop=1), dict(factorization_method=1)))
    out.append(("mixed sizes kkt", mixed, dict(sparse_kkt=1, sparse_ordering=-1), dict(factorization_method=0)))
    uns = [unsorted_full(sparse_qp(96, "arrow", seed=5)), sparse_qp(96, "banded", seed=6), unsorted_full(sparse_qp(300, "blocks", seed=7))]
    out.append(("unsorted columns, full Q, schur", uns, dict(sparse_factor=1, sparse_ordering=-1, sparse_coop=1), dict(factorization_method=1)))
    out.append(("unsorted columns, full Q, dense", uns[:2], dict(sparse_factor=0), dict(factorization_method=1)))
    return out


DEFAULTS = dict(sparse_factor=-1, sparse_ordering=-1, sparse_coop=0, sparse_kkt=0)


def dump(lib, path):
    from qpalm_amd.solver import Context, QpalmBatch
    ctx = Context(0, lib_path=lib)
    res = {}
    for ci, (name, probs, opts, st) in enumerate(cases()):
        for k, v in dict(DEFAULTS, **opts).items():
            ctx.set_option(k, v)
        bt = QpalmBatch(ctx, probs, ctx.default_settings(verbose=0, **st))
        nzA, nzQ = bt.nnzA, bt.nnzQ
        lens = dict(Ap=bt.n + 1, Ai=nzA, Atp=bt.m + 1, Ati=nzA, Atperm=nzA, Ainv=nzA, Qp=bt.n + 1, Qi=nzQ, Qfp=bt.n + 1, Qfi=2 * nzQ, Qfperm=2 * nzQ)

        def put(key, v):
            res["%03d|%s|%s" % (ci, name, key)] = np.asarray(v)
        sparse = "dense" not in name
        for b in range(bt.B):
            if sparse:
                perm, lev = bt.sparse_perm(b)
                Lp, Li, _, _ = bt.sparse_factor(b)
                put("%d perm" % b, perm); put("%d levels" % b, lev); put("%d nnzL" % b, bt.sparse_info(b)[0])
                put("%d Lp" % b, Lp); put("%d Li" % b, Li); put("%d coop" % b, bt.sparse_coop_info(b))
            for a in INT_ARRAYS:
                put("%d %s" % (b, a), bt.ivec(a, b, lens[a]))
            put("%d A_values" % b, bt.named_vec("A_values", nzA, b)); put("%d Q_values" % b, bt.named_vec("Q_values", nzQ, b))
        rng = np.random.default_rng(ci)
        bt.update_Q_A([1.0 + rng.random(len(p.Qx)) for p in probs], [rng.standard_normal(len(p.Ax)) for p in probs])
        for b in range(bt.B):
            put("%d A_values updated" % b, bt.named_vec("A_values", nzA, b)); put("%d Q_values updated" % b, bt.named_vec("Q_values", nzQ, b))
        bt.close()
    np.savez(path, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a"); ap.add_argument("--b"); ap.add_argument("--dump", nargs=2, metavar=("LIB", "OUT"))
    a = ap.parse_args()
    if a.dump:
        return dump(*a.dump)
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for tag, lib in (("a", a.a), ("b", a.b)):
            outs.append(os.path.join(d, tag + ".npz"))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--dump", os.path.abspath(lib), outs[-1]])
        A, B = np.load(outs[0]), np.load(outs[1])
        assert sorted(A.files) == sorted(B.files)
        ncase = len({k.split("|")[0] for k in A.files})
        diff = [k for k in A.files if not (A[k].shape == B[k].shape and np.array_equal(A[k], B[k]))]
        entries = sum(int(A[k].size) for k in A.files)
        print("%d batches, %d arrays, %d entries compared: %s" % (ncase, len(A.files), entries, "all equal" if not diff else "%d DIFFERENT" % len(diff)))
        for k in diff[:40]:
            print("  DIFFERENT", k)
        return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())

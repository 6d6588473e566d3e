"""The test matrices of tests/test_sparse_ops_exact.py: QPs put together from independent gadgets, each of which drives one shape-dependent branch of
the sparse kernels (qpalm_amd/csrc/qpalm_sparse.h, qpalm_sparse_kkt.h).  g stands for the lanes a column's group has (spg = 64 / sparse_gpw).

  cliques   for L in (g-1, g, g+1, 2g-1, 2g, 2g+1) one row of A over L fresh consecutive variables: columns of every length up to 2g+1 (the LDS form
            takes a column of at most 2 spg accumulators, decided per wavefront), rows of A and contributing columns of L longer than a group
  stars     k in {1, 3, 4, 5, g-1, g, g+1, 2g+1} two-entry rows (leaf_i, hub), the hub numbered last: the hub's column meets k rows of A and k
            contributing columns -- the batches of four, the reload past a group's lanes --, its row of L has k entries
  levels    w pairs of variables joined through Q and a tridiagonal chain of six: w + 1 columns in each of the first two levels, then a run of
            one-column levels
  arrow     a last variable coupled through Q to every other: one very long row of L, one root
  single    an empty row of A and a row whose only entry is the last column
  band      (optional) `band` variables with two sub-diagonals in Q and difference rows (x_i, x_i+1) in A, half of them numbered in front of the
            gadgets and half behind: something for the nested dissection to reorder -- it keeps a component's columns together, so the
            gadgets' columns are renumbered too
  budget    (optional) one dense row of A over all variables (the KKT tests)
Deterministic in the arguments.
"""
import numpy as np
import scipy.sparse as sp

from qpalm_amd.problems import QP, _csc

INF = 1e20


def clique_lengths(g):
    return (g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1)


def star_sizes(g):
    return sorted({1, 3, 4, 5, g - 1, g, g + 1, 2 * g + 1})


def block_sizes(n, block=8):
    """n variables in dense blocks of `block`, the last one taking the remainder"""
    sizes = [block] * (n // block)
    sizes[-1] += n - block * (n // block)
    return sizes


def gadget_qp(glist, seed, w, cliques=True, stars=True, arrow=True, single=True, band=0, budget=False):
    """(QP, rows): rows = dict of row numbers of A by gadget -- 'clique' [(g, L, row)], 'star' [(g, k, [rows])], 'box' [rows] (one-entry rows on the
    pairs and the chain), 'band' [rows], 'empty', 'root_only', 'budget' (None where absent) -- and 'active': the base active set (every second row inside each
    gadget; in the largest star of every g the rows g .. 2g-1, one whole round of a group's lanes, are inactive)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nvar, arows, qpairs = 0, [], []
    rows = dict(clique=[], star=[], box=[], band=[], empty=None, root_only=None, budget=None)
    active = []
    bandvars = list(range(band // 2))           # the first half of the band in front of the gadgets, the second half behind them
    nvar = len(bandvars)
    for g in (glist if cliques else ()):
        first = len(arows)
        for L in clique_lengths(g):
            rows["clique"].append((g, L, len(arows)))
            arows.append(list(range(nvar, nvar + L)))
            nvar += L
        active += list(range(first, len(arows), 2))
    for g in (glist if stars else ()):
        for k in star_sizes(g):
            hub = nvar + k
            mine = []
            for i in range(k):
                mine.append(len(arows))
                arows.append([nvar + i, hub])
            nvar += k + 1
            rows["star"].append((g, k, mine))
            if k == 2 * g + 1:
                active += mine[0:g:2] + [mine[2 * g]]
            else:
                active += mine[0::2]
    first = len(arows)
    for _ in range(w):
        qpairs.append((nvar, nvar + 1))
        rows["box"].append(len(arows)); arows.append([nvar])
        nvar += 2
    for i in range(6):
        if i:
            qpairs.append((nvar - 1, nvar))
        rows["box"].append(len(arows)); arows.append([nvar])
        nvar += 1
    active += list(range(first, len(arows), 2))
    bandvars += list(range(nvar, nvar + band - band // 2))
    nvar += band - band // 2
    for i in range(band):
        for d in (1, 2):
            if i >= d:
                qpairs.append(tuple(sorted((bandvars[i - d], bandvars[i]))))
        if i % 2:
            rows["band"].append(len(arows)); arows.append([bandvars[i - 1], bandvars[i]])
    active += rows["band"][0::2]
    if arrow:
        qpairs += [(j, nvar) for j in range(nvar)]
        nvar += 1
    n = nvar
    if single:
        rows["empty"] = len(arows); arows.append([])
        rows["root_only"] = len(arows); arows.append([n - 1])
        active += [rows["empty"], rows["root_only"]]
    if budget:
        rows["budget"] = len(arows); arows.append(list(range(n)))
    m = len(arows)
    ar, ac, av = [], [], []
    for i, cols in enumerate(arows):
        v = 0.3 * rng.standard_normal(len(cols))
        v = np.where(np.abs(v) < 0.05, np.where(v < 0, -0.05, 0.05), v)      # clipped away from zero
        ar += [i] * len(cols); ac += cols; av += list(v)
    A = sp.csc_matrix((av, (ar, ac)), shape=(m, n))
    A.sort_indices()
    qi = np.array([a for a, _ in qpairs] + [b for _, b in qpairs], dtype=np.int64)
    qj = np.array([b for _, b in qpairs] + [a for a, _ in qpairs], dtype=np.int64)
    qv = np.array([(0.1 if (arrow and b == n - 1) else 0.3) * rng.standard_normal() for _, b in qpairs])
    S = sp.csc_matrix((np.concatenate([qv, qv]), (qi, qj)), shape=(n, n))
    Qf = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsc()
    q = rng.standard_normal(n)
    bmin, bmax = -rng.random(m), rng.random(m)
    third = np.arange(m) % 3 == 0
    bmin[third & (np.arange(m) % 2 == 0)] = -INF
    bmax[third & (np.arange(m) % 2 == 1)] = INF
    box = np.asarray(rows["box"], dtype=np.int64)       # narrow boxes: most of them are violated on the way, so their penalties move early
    bmin[box] = np.where(bmin[box] > -INF, 0.05 * bmin[box], -INF)
    bmax[box] = np.where(bmax[box] < INF, 0.05 * bmax[box], INF)
    Ql = sp.tril(Qf).tocsc(); Ql.sort_indices()
    Qp, Qi, Qx = _csc(Ql)
    Ap, Ai, Ax = _csc(A)
    rows["active"] = sorted(active)
    return QP(n, m, Qp, Qi, Qx, Ap, Ai, Ax, q, bmin, bmax), rows


def blocks_qp(n, seed, block=8, rows_per_block=3):
    """(QP, rows): block-diagonal Q with dense blocks (block_sizes(n)), `rows_per_block` three-entry rows of A inside each block -- a forest of n / block
    small trees, any n; rows as gadget_qp's ('clique' holds the rows of the first, a middle and the last block, 'active' every second row)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = block_sizes(n, block)
    blocks, ar, ac, av, m, start = [], [], [], [], 0, 0
    rows = dict(clique=[], star=[], box=[], band=[], empty=None, root_only=None, budget=None)
    for b, sz in enumerate(sizes):
        M = 0.3 * rng.standard_normal((sz, sz))
        Sb = 0.5 * (M + M.T)
        np.fill_diagonal(Sb, 0.0)
        blocks.append(Sb + np.diag(np.abs(Sb).sum(axis=1) + 1.0))
        for _ in range(rows_per_block):
            idx = np.sort(rng.choice(sz, size=3, replace=False))
            v = 0.3 * rng.standard_normal(3)
            v = np.where(np.abs(v) < 0.05, np.where(v < 0, -0.05, 0.05), v)
            ar += [m] * 3; ac += [start + int(i) for i in idx]; av += list(v)
            if b in (0, len(sizes) // 2, len(sizes) - 1):
                rows["clique"].append((block, 3, m))
            m += 1
        start += sz
    Qf = sp.block_diag(blocks, format="csc")
    A = sp.csc_matrix((av, (ar, ac)), shape=(m, n)); A.sort_indices()
    q = rng.standard_normal(n)
    bmin, bmax = -rng.random(m), rng.random(m)
    third = np.arange(m) % 3 == 0
    bmin[third & (np.arange(m) % 2 == 0)] = -INF
    bmax[third & (np.arange(m) % 2 == 1)] = INF
    Ql = sp.tril(Qf).tocsc(); Ql.sort_indices()
    Qp, Qi, Qx = _csc(Ql)
    Ap, Ai, Ax = _csc(A)
    rows["active"] = list(range(0, m, 2))
    return QP(n, m, Qp, Qi, Qx, Ap, Ai, Ax, q, bmin, bmax), rows

/*
 * qpalm_host_symbolic.h -- symbolic analysis of the sparse factors: host algorithms on index arrays, standard library only (no device,
 * no batch: tests/c/test_host_symbolic.cpp runs them stand-alone).  qpalm_capi.inc's sparse_setup calls sparse_symbolic and
 * sparse_factor_index per member and sparse_coop_plan per member of a sparse coop batch.
 */
#pragma once

#include <algorithm>
#include <string>
#include <vector>

/* one member's patterns in the device layout (qpalm_host_convert.h): A by columns and by rows, Q with both triangles */
struct SparsePattern { int n, m; const int *Ap, *Ai, *Atp, *Ati, *Qfp, *Qfi; };

/* ---- sparse factor: symbolic analysis (host, once per member) ------------------------------------------------------------------
 * Pattern of H = Q + A'A (+ diagonal) with ALL rows of A, natural ordering (solver_interface.c:530-540); elimination tree and the
 * pattern of L by the classic column recurrence  struct(L_j) = struct(H_j) u U_{children c of j} struct(L_c) \ {c},
 * parent(j) = min struct(L_j)  (Liu 1990; what cholmod_analyze computes for a simplicial factor); the same entries by rows; the level
 * sets of the tree (level = height above the leaves: the columns a column depends on are its descendants).  Everything int32. */
struct SparseSym {
  std::vector<int> Lp, Li, Rp, Rk, Rpos, levptr, levcol;
  std::vector<int> perm, iperm; /* the factor is that of P H P': perm[new] = old, iperm[old] = new (identity: natural ordering) */
  int nlev;
  bool dissected;
};
/* Nested dissection (sparse_order, below) of the graph of H = Q + A'A or of K (sparse_adj_H / sparse_adj_K; George's automatic scheme on breadth-first level structures): a band-like pattern,
 * whose elimination tree under the natural ordering is a chain of n columns (one column per level: the factorisation and the solves
 * then run at the latency of n dependent steps), becomes a tree of height ~ leaf + separator x log2(n / leaf) whose levels hold
 * hundreds of independent columns.  Vertices of very high degree (dense rows / columns: an arrow's shaft) are set aside and ordered last;
 * the rest is split recursively: connected components one after the other; a component by the middle level of the level structure
 * rooted at a pseudo-peripheral vertex (first half, second half, separator last); small pieces keep their natural order.  The
 * reference configures CHOLMOD_NATURAL; this is an engine option that changes speed and rounding, not what is computed. */
/* the graph a factor's ordering works on: neighbours of every vertex (original numbering, no self loops) */
struct SparseAdj { std::vector<int> p, i; };
/* column jo of H = Q + A'A with ALL rows of A: visit(i) for its row indices i (original numbering, with repeats) */
template <class Visit>
static void sparse_cols_H(const SparsePattern &P, const int jo, Visit &&visit) {
  for (int k = P.Qfp[jo]; k < P.Qfp[jo + 1]; k++) visit(P.Qfi[k]);
  for (int p = P.Ap[jo]; p < P.Ap[jo + 1]; p++) { const int t = P.Ai[p]; for (int q = P.Atp[t]; q < P.Atp[t + 1]; q++) visit(P.Ati[q]); }
}
/* graph of H = Q + A'A (a long row of A -- a clique of H whatever the ordering -- enters as a chain of its columns: ordering quality only) */
static void sparse_adj_H(const SparsePattern &P, SparseAdj &G) {
  const int n = P.n;
  const int *Ap = P.Ap, *Ai = P.Ai, *Atp = P.Atp, *Ati = P.Ati, *Qfp = P.Qfp, *Qfi = P.Qfi;
  const int LONG_ROW = 64;
  std::vector<int> &adjp = G.p, &adji = G.i, mark((size_t)n, -1);
  adjp.assign((size_t)n + 1, 0); adji.clear();
  for (int j = 0; j < n; j++) {
    mark[j] = j;
    for (int k = Qfp[j]; k < Qfp[j + 1]; k++) { const int i = Qfi[k]; if (mark[i] != j) { mark[i] = j; adji.push_back(i); } }
    for (int p = Ap[j]; p < Ap[j + 1]; p++) {
      const int t = Ai[p], q0 = Atp[t], q1 = Atp[t + 1];
      if (q1 - q0 <= LONG_ROW) { for (int q = q0; q < q1; q++) { const int i = Ati[q]; if (mark[i] != j) { mark[i] = j; adji.push_back(i); } } }
      else for (int q = q0; q < q1; q++) if (Ati[q] == j) { /* neighbours in the row's chain */
        if (q > q0 && mark[Ati[q - 1]] != j) { mark[Ati[q - 1]] = j; adji.push_back(Ati[q - 1]); }
        if (q + 1 < q1 && mark[Ati[q + 1]] != j) { mark[Ati[q + 1]] = j; adji.push_back(Ati[q + 1]); }
      }
    }
    adjp[j + 1] = (int)adji.size();
  }
}
/* graph of K_full = [[Q + I, A'], [A, I]] with ALL rows of A (the reference's kkt_full): vertices 0 .. n-1 the variables, n + k constraint k.
 * A superset of every active set's K, so the factor's structure never changes when rows enter or leave */
static void sparse_adj_K(const SparsePattern &P, SparseAdj &G) {
  const int n = P.n, m = P.m;
  const int *Ap = P.Ap, *Ai = P.Ai, *Atp = P.Atp, *Ati = P.Ati, *Qfp = P.Qfp, *Qfi = P.Qfi;
  std::vector<int> &adjp = G.p, &adji = G.i, mark((size_t)n, -1);
  adjp.assign((size_t)n + m + 1, 0); adji.clear();
  for (int j = 0; j < n; j++) {
    mark[j] = j;
    for (int k = Qfp[j]; k < Qfp[j + 1]; k++) { const int i = Qfi[k]; if (mark[i] != j) { mark[i] = j; adji.push_back(i); } }
    for (int p = Ap[j]; p < Ap[j + 1]; p++) adji.push_back(n + Ai[p]);
    adjp[j + 1] = (int)adji.size();
  }
  for (int k = 0; k < m; k++) {
    for (int q = Atp[k]; q < Atp[k + 1]; q++) adji.push_back(Ati[q]);
    adjp[n + k + 1] = (int)adji.size();
  }
}
static void sparse_order(const SparseAdj &G, const int n, std::vector<int> &perm) {
  const std::vector<int> &adjp = G.p, &adji = G.i;
  const int LEAF = 24;
  const size_t hub_deg = std::max<size_t>(48, 10 * (adji.size() / std::max(n, 1) + 1));
  std::vector<int> part((size_t)n, 0), level((size_t)n, 0), queue((size_t)n);
  perm.assign((size_t)n, -1);
  std::vector<int> rest, hubs;
  for (int j = 0; j < n; j++) { if ((size_t)(adjp[j + 1] - adjp[j]) > hub_deg) { hubs.push_back(j); part[j] = -1; } else rest.push_back(j); }
  for (size_t k = 0; k < hubs.size(); k++) perm[rest.size() + k] = hubs[k];
  struct Item { std::vector<int> nodes; int lo; };
  std::vector<Item> stack;
  stack.push_back(Item{std::move(rest), 0});
  int label = 0;
  /* breadth-first search inside the piece labelled `lab` from `root`: fills queue[0 .. count), level[]; visited vertices get label -lab-2
   * ... and are restored by the caller */
  auto bfs = [&](int root, int lab, int vis) -> int {
    int head = 0, tail = 0;
    queue[tail++] = root; part[root] = vis; level[root] = 0;
    while (head < tail) {
      const int v = queue[head++];
      for (int e = adjp[v]; e < adjp[v + 1]; e++) { const int u = adji[e]; if (part[u] == lab) { part[u] = vis; level[u] = level[v] + 1; queue[tail++] = u; } }
    }
    return tail;
  };
  while (!stack.empty()) {
    Item it = std::move(stack.back());
    stack.pop_back();
    std::vector<int> &nodes = it.nodes;
    const int cnt = (int)nodes.size();
    if (cnt == 0) continue;
    if (cnt <= LEAF) { std::sort(nodes.begin(), nodes.end()); for (int k = 0; k < cnt; k++) perm[it.lo + k] = nodes[k]; continue; }
    const int lab = ++label * 2, vis = lab + 1;
    for (int v : nodes) part[v] = lab;
    /* connected components, by smallest vertex */
    std::sort(nodes.begin(), nodes.end());
    int got = bfs(nodes[0], lab, vis);
    if (got < cnt) {
      int lo = it.lo;
      std::vector<int> comp(queue.begin(), queue.begin() + got);
      stack.push_back(Item{std::move(comp), lo}); lo += got;
      for (int v : nodes) if (part[v] == lab) { got = bfs(v, lab, vis); stack.push_back(Item{std::vector<int>(queue.begin(), queue.begin() + got), lo}); lo += got; }
      continue;
    }
    /* one component: pseudo-peripheral root (two more sweeps from the far end), then its level structure */
    int root = queue[cnt - 1];
    for (int sweep = 0; sweep < 2; sweep++) {
      for (int v : nodes) part[v] = lab;
      bfs(root, lab, vis);
      const int far = level[queue[cnt - 1]];
      int best = queue[cnt - 1];
      for (int k = cnt - 1; k >= 0 && level[queue[k]] == far; k--) if (adjp[queue[k] + 1] - adjp[queue[k]] < adjp[best + 1] - adjp[best]) best = queue[k];
      if (sweep == 0) root = best;
    }
    const int nlev = level[queue[cnt - 1]] + 1;
    if (nlev < 3) { for (int k = 0; k < cnt; k++) perm[it.lo + k] = nodes[k]; continue; } /* (nodes is sorted) no separator to be had: natural order */
    std::vector<int> lsize((size_t)nlev, 0);
    for (int k = 0; k < cnt; k++) lsize[level[queue[k]]]++;
    /* separator: the smallest level among those that leave between 30 % and 70 % of the piece in front of them; else the median's level */
    int sep = -1, before = 0, med = 1;
    { int acc = 0; for (int l = 0; l < nlev; l++) { if (acc <= cnt / 2) med = l; acc += lsize[l]; } med = std::min(std::max(med, 1), nlev - 2); }
    for (int l = 0; l < nlev; l++) {
      if (l >= 1 && l <= nlev - 2 && 10 * before >= 3 * cnt && 10 * before <= 7 * cnt && (sep < 0 || lsize[l] < lsize[sep])) sep = l;
      before += lsize[l];
    }
    if (sep < 0) sep = med;
    std::vector<int> A, Bn, Sn;
    for (int k = 0; k < cnt; k++) {
      const int v = queue[k], l = level[v];
      if (l < sep) A.push_back(v);
      else if (l > sep) Bn.push_back(v);
      else { /* a separator vertex without a neighbour beyond the separator belongs to the first half */
        bool touches = false;
        for (int e = adjp[v]; e < adjp[v + 1] && !touches; e++) { const int u = adji[e]; touches = (part[u] == vis && level[u] == sep + 1); }
        if (touches) Sn.push_back(v); else A.push_back(v);
      }
    }
    std::sort(Sn.begin(), Sn.end());
    const int na = (int)A.size(), nb2 = (int)Bn.size();
    for (size_t k = 0; k < Sn.size(); k++) perm[it.lo + na + nb2 + (int)k] = Sn[k];
    stack.push_back(Item{std::move(A), it.lo});
    stack.push_back(Item{std::move(Bn), it.lo + na});
  }
}
/* cols(jo, visit) calls visit(i) for the row indices i (original numbering; repeats allowed) of column jo of the matrix to factorise */
template <class Cols>
static int sparse_analyze(const int n, const Cols &cols, SparseSym &S, size_t max_nnz, std::string &why) {
  if (S.perm.size() != (size_t)n) { S.perm.resize((size_t)n); for (int j = 0; j < n; j++) S.perm[j] = j; }
  S.iperm.assign((size_t)n, 0);
  for (int j = 0; j < n; j++) S.iperm[S.perm[j]] = j;
  const int *perm = S.perm.data(), *ip = S.iperm.data();
  S.Lp.assign((size_t)n + 1, 0);
  S.Li.clear();
  std::vector<int> parent((size_t)n, -1), mark((size_t)n, -1), child_head((size_t)n, -1), child_next((size_t)n, -1), col;
  for (int j = 0; j < n; j++) { /* column j of P H P' = column perm[j] of H, rows renumbered */
    col.clear();
    mark[j] = j;
    cols(perm[j], [&](const int io) { const int i = ip[io]; if (i > j && mark[i] != j) { mark[i] = j; col.push_back(i); } });
    for (int c = child_head[j]; c >= 0; c = child_next[c])
      for (int e = S.Lp[c]; e < S.Lp[c + 1]; e++) { const int i = S.Li[e]; if (i > j && mark[i] != j) { mark[i] = j; col.push_back(i); } }
    std::sort(col.begin(), col.end());
    if (S.Li.size() + col.size() > max_nnz) { why = "the sparse factor would hold more than " + std::to_string(max_nnz) + " entries"; return 1; }
    S.Li.insert(S.Li.end(), col.begin(), col.end());
    S.Lp[j + 1] = (int)S.Li.size();
    if (!col.empty()) { parent[j] = col[0]; child_next[j] = child_head[col[0]]; child_head[col[0]] = j; }
  }
  const size_t nz = S.Li.size();
  /* the same entries by rows: columns ascending inside a row because the columns are walked in ascending order */
  S.Rp.assign((size_t)n + 1, 0);
  for (size_t e = 0; e < nz; e++) S.Rp[S.Li[e] + 1]++;
  for (int i = 0; i < n; i++) S.Rp[i + 1] += S.Rp[i];
  S.Rk.resize(nz); S.Rpos.resize(nz);
  { std::vector<int> cur(S.Rp.begin(), S.Rp.end() - 1);
    for (int k = 0; k < n; k++)
      for (int e = S.Lp[k]; e < S.Lp[k + 1]; e++) { const int dst = cur[S.Li[e]]++; S.Rk[dst] = k; S.Rpos[dst] = e; } }
  /* levels: height above the leaves (children before parents: a child's index is smaller than its parent's) */
  std::vector<int> level((size_t)n, 0);
  int nlev = 0;
  for (int j = 0; j < n; j++) {
    if (parent[j] >= 0 && level[parent[j]] < level[j] + 1) level[parent[j]] = level[j] + 1;
    if (level[j] + 1 > nlev) nlev = level[j] + 1;
  }
  S.nlev = nlev;
  S.levptr.assign((size_t)nlev + 1, 0);
  for (int j = 0; j < n; j++) S.levptr[level[j] + 1]++;
  for (int l = 0; l < nlev; l++) S.levptr[l + 1] += S.levptr[l];
  S.levcol.resize((size_t)n);
  { std::vector<int> cur(S.levptr.begin(), S.levptr.end() - 1);
    for (int j = 0; j < n; j++) S.levcol[cur[level[j]]++] = j; }
  return 0;
}
/* The analysis of one member: of K_full (kkt) or of H, under `ordering` (context option "sparse_ordering": 0 natural, 1 nested dissection, -1 automatic).
 * Returns 0, or 1 with the reason in `why` (a factor of more than max_nnz entries). */
static int sparse_symbolic(const SparsePattern &P, const bool kkt, const int ordering, const size_t max_nnz, SparseSym &S, std::string &why) {
  S.dissected = false;
  if (kkt) {
    /* K_full: nested dissection unless the natural order [x; y] is asked for (under [x; y] a banded Q fills the whole constraint block:
     * about n m entries); the dense rows of A are high-degree vertices, set aside and ordered last */
    SparseAdj G;
    sparse_adj_K(P, G);
    const int nf = P.n + P.m;
    if (ordering != 0) { sparse_order(G, nf, S.perm); S.dissected = true; }
    auto cols = [&G](const int jo, auto &&visit) { for (int e = G.p[jo]; e < G.p[jo + 1]; e++) visit(G.i[e]); };
    return sparse_analyze(nf, cols, S, max_nnz, why);
  }
  auto cols = [&P](const int jo, auto &&visit) { sparse_cols_H(P, jo, visit); };
  int rc = 0;
  if (ordering != 1) rc = sparse_analyze(P.n, cols, S, max_nnz, why); /* natural ordering */
  const bool deep = ordering == 1 || (ordering < 0 && rc == 0 && S.nlev > 256 && (size_t)S.nlev * 8 > (size_t)P.n);
  if (!deep) return rc;
  SparseSym nd;
  { SparseAdj G; sparse_adj_H(P, G); sparse_order(G, P.n, nd.perm); }
  std::string why_nd;
  const int rc_nd = sparse_analyze(P.n, cols, nd, max_nnz, why_nd);
  nd.dissected = true;
  /* automatic: kept when the tree is at least four times shallower and the factor at most three times larger */
  if (ordering == 1) { rc = rc_nd; why = why_nd; S = std::move(nd); }
  else if (rc_nd == 0 && (size_t)nd.nlev * 4 <= (size_t)S.nlev && nd.Li.size() <= 3 * S.Li.size() + (size_t)P.n) S = std::move(nd);
  return rc;
}
/* the index arrays the factor reads, in the factor's numbering: rows of A (atip), columns of the full Q (qfip), and each row's first path column
 * (first; KKT mode: the constraint's own row / column of K).  The vectors keep their sizes (the batch's strides); entries beyond the member's are 0.
 * The full Q's entry count is read from the pattern itself, Qfp[n] (the conversion's nzQf). */
static void sparse_factor_index(const SparsePattern &P, const SparseSym &S, const bool kkt, std::vector<int> &atip, std::vector<int> &qfip, std::vector<int> &first) {
  const int *Atp = P.Atp, *Ati = P.Ati, *Qfi = P.Qfi;
  const int *ip = S.iperm.data();
  std::fill(atip.begin(), atip.end(), 0); std::fill(qfip.begin(), qfip.end(), 0); std::fill(first.begin(), first.end(), 0);
  for (int t = 0; t < P.m; t++) {
    int f = P.n;
    for (int q = Atp[t]; q < Atp[t + 1]; q++) { atip[(size_t)q] = ip[Ati[q]]; f = std::min(f, ip[Ati[q]]); }
    first[(size_t)t] = kkt ? ip[P.n + t] : f; /* KKT mode: the constraint's own row / column of K in the factor's numbering */
  }
  for (int k = 0; k < P.Qfp[P.n]; k++) qfip[(size_t)k] = ip[Qfi[k]];
}
/* Sparse coop mode: the launch plan of one member from the level sets of its elimination tree (patterns only: qpg_batch_update_Q_A leaves it valid).
 * Consecutive levels that one workgroup finishes in one round (at most `round_f` columns for the factorisation, `round_s` rows for the solves) become ONE
 * launch on one workgroup, which runs the one-workgroup loop with its barriers -- a band under the natural ordering (n one-column levels) is one launch;
 * a wider level is a launch of its own on min(G, ceil(width / round)) workgroups, grid-strided where it is wider than the grid.  G = 1 (no memory for
 * a second workgroup's work vectors): one launch per phase.
 * A launch covers the levels [lev0, lev1) of the elimination tree on `grid` workgroups: more than one level only with grid = 1 */
struct SpLaunch { int lev0, lev1, grid; };
struct SpPlan { std::vector<SpLaunch> factor, solve; int vec_grid, solve_launches, max_grid; }; /* vec_grid: workgroups of the solve's elementwise launches */
static void sparse_coop_plan(const std::vector<int> &levptr, int nlev, int n, int round_f, int round_s, int G, SpPlan &P) {
  auto cut = [&](int round, std::vector<SpLaunch> &out) {
    out.clear();
    if (G <= 1) round = 0x7fffffff; /* no grid to spread a level over: the whole phase is one launch of the one-workgroup loop, not a launch per wide level */
    for (int l = 0; l < nlev;) {
      const int w = levptr[(size_t)l + 1] - levptr[(size_t)l];
      if (w > round) { out.push_back({l, l + 1, std::min(G, (w + round - 1) / round)}); l++; continue; }
      int l1 = l + 1;
      while (l1 < nlev && levptr[(size_t)l1 + 1] - levptr[(size_t)l1] <= round) l1++;
      out.push_back({l, l1, 1});
      l = l1;
    }
  };
  cut(round_f, P.factor);
  cut(round_s, P.solve);
  P.vec_grid = std::max(1, std::min(G, (n + round_s - 1) / round_s));
  /* permute in, forward launches, D, backward launches; level 0 on a grid: the permutation back is a launch of its own */
  P.solve_launches = 2 + 2 * (int)P.solve.size() + ((!P.solve.empty() && P.solve[0].grid > 1) ? 1 : 0);
  P.max_grid = P.vec_grid;
  for (auto &l : P.factor) P.max_grid = std::max(P.max_grid, l.grid);
  for (auto &l : P.solve) P.max_grid = std::max(P.max_grid, l.grid);
}

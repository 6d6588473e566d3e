/*
 * qpalm_host_convert.h -- a caller's problem (CSC Q and A, q, bounds) into the device layout of one batch member: host code on plain arrays,
 * standard library and the ABI's types only (tests/c/test_host_convert.cpp runs it stand-alone).  This is where the caller's column pointers
 * and row indices are checked before they index the destination.  qpalm_capi.inc's set_problem_impl points it at the member's part of the host slab.
 */
#pragma once

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/qpalm_gfx950.h"

/* the arrays of one member in the device layout: int32 up to H_QFPERM, doubles from H_AX */
enum { H_AP, H_AI, H_ATP, H_ATI, H_ATPERM, H_AINV, H_QP, H_QI, H_QFP, H_QFI, H_QFPERM, H_AX, H_QX, H_Q, H_BMIN, H_BMAX, H_COUNT };
struct HostProblem { /* one member: its own dimensions (<= the batch's) and entry counts; the arrays live in the slab */
  int n, m, nzA, nzQ, nzQf;
  double c;
  bool set;
};
/* where a member's arrays go: p[a] holds stride[a] entries (the batch's stride of array a); convert_problem writes all of them and nothing beyond */
struct ConvertDst {
  void *p[H_COUNT];
  size_t stride[H_COUNT];
  int *i(int a) const { return (int *)p[a]; }
  double *d(int a) const { return (double *)p[a]; }
};

/* the member's entries, then padding up to the batch's stride: zeros, or (column pointers of a smaller member) the last value
 * repeated = empty columns */
template <class T> static void pad(T *d, size_t used, size_t stride) { if (used < stride) memset(d + used, 0, (stride - used) * sizeof(*d)); }
static void pad_ptr(int *d, size_t used, size_t stride) { for (size_t j = used; j < stride; j++) d[j] = d[used - 1]; }
/* One column of a CSC matrix (entries k0 .. k1-1 of the caller's arrays, optionally only rows >= rmin) into dst at position pos,
 * rows ascending: already-sorted columns (the usual case) are copied straight, others sorted by row (stable: equal rows keep
 * the caller's order, QPS-loaded matrices may be unsorted).  Returns the new position, -1 on a bad index.
 * reordered is set when the column was sorted or lost an entry: the device's order of the values is not the caller's (value_map below) */
static qpg_int take_column(std::vector<std::pair<int, double> > &tmp, bool &reordered, const qpg_int *I, const qpg_float *X, qpg_int k0, qpg_int k1,
                           qpg_int rmin, qpg_int rmax, int *di, double *dx, qpg_int pos) {
  bool sorted = true;
  qpg_int prev = -1;
  const qpg_int p0 = pos;
  for (qpg_int k = k0; k < k1; k++) {
    const qpg_int r = I[k];
    if (r < 0 || r >= rmax) return -1;
    if (r < rmin) { reordered = true; continue; }
    if (r < prev) sorted = false;
    prev = r;
    di[pos] = (int)r; dx[pos] = X[k]; pos++;
  }
  if (!sorted) {
    reordered = true;
    tmp.clear();
    for (qpg_int t = p0; t < pos; t++) tmp.push_back(std::make_pair(di[t], dx[t]));
    std::stable_sort(tmp.begin(), tmp.end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });
    for (qpg_int t = p0; t < pos; t++) { di[t] = tmp[t - p0].first; dx[t] = tmp[t - p0].second; }
  }
  return pos;
}
/* position in the caller's arrays of every entry take_column keeps, in its order (the same stable sort, on positions); only for input it reordered */
static void value_map(const int n, const qpg_int *Pc, const qpg_int *I, bool lower, std::vector<int> &map) {
  map.clear();
  for (int j = 0; j < n; j++) {
    const size_t p0 = map.size();
    for (qpg_int k = Pc[j]; k < Pc[j + 1]; k++) if (!lower || I[k] >= j) map.push_back((int)k);
    std::stable_sort(map.begin() + p0, map.end(), [I](int a, int b) { return I[a] < I[b]; });
  }
}
/* Validates one n x n / m x n problem and writes it to D.  Returns QPG_OK, or QPG_ERR_INVALID with the reason in msg; P.set says whether D holds a
 * whole problem (a refusal after the first write leaves it false).  map_A / map_Q: entry k of D's A / Q values = entry map[k] of Ax / Qx; empty = the
 * same order (sorted columns, no upper entry of Q: the usual input). */
static int convert_problem(const ConvertDst &D, const int n, const int m, const qpg_int *Qp, const qpg_int *Qi, const qpg_float *Qx,
                           const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax, const qpg_float *q, qpg_float c, const qpg_float *bmin,
                           const qpg_float *bmax, HostProblem &P, std::vector<int> &map_A, std::vector<int> &map_Q, std::string &msg) {
  if (!Qp || !Ap || !q || (m && (!bmin || !bmax))) { msg = "Missing data"; return QPG_ERR_INVALID; }
  for (int j = 0; j < m; j++)
    if (bmin[j] > bmax[j]) { /* validate_data, src/validate.c:31-39 */
      char buf[160]; snprintf(buf, sizeof buf, "Lower bound at index %d is greater than upper bound: %.4e > %.4e", j, bmin[j], bmax[j]);
      msg = buf; return QPG_ERR_INVALID;
    }
  const qpg_int nzA = Ap[n], nzQ = Qp[n];
  if (Ap[0] != 0 || Qp[0] != 0) { msg = "qpg_batch_set_problem: column pointers must start at 0"; return QPG_ERR_INVALID; } /* (entries before Ap[0] of the reused slab would be stale: ADVICE round 4) */
  if (nzA < 0 || nzQ < 0 || nzA > (qpg_int)D.stride[H_AI] || nzQ > (qpg_int)D.stride[H_QI]) { msg = "qpg_batch_set_problem: more nonzeros than nnzA_max / nnzQ_max"; return QPG_ERR_INVALID; }
  P.n = n; P.m = m; P.set = false;
  int *hAp = D.i(H_AP), *hAi = D.i(H_AI), *hAtp = D.i(H_ATP), *hAti = D.i(H_ATI), *hAtperm = D.i(H_ATPERM), *hAinv = D.i(H_AINV);
  int *hQp = D.i(H_QP), *hQi = D.i(H_QI), *hQfp = D.i(H_QFP), *hQfi = D.i(H_QFI), *hQfperm = D.i(H_QFPERM);
  double *hAx = D.d(H_AX), *hQx = D.d(H_QX);
  std::vector<std::pair<int, double> > tmp;
  bool reordered = false;
  /* A: CSC with sorted rows inside each column */
  for (int j = 0; j < n; j++) {
    if (Ap[j + 1] < Ap[j] || Ap[j] < 0 || Ap[j + 1] > nzA) { msg = "A: column pointers not monotone"; return QPG_ERR_INVALID; }
    hAp[j] = (int)Ap[j];
    if (take_column(tmp, reordered, Ai, Ax, Ap[j], Ap[j + 1], 0, m, hAi, hAx, Ap[j]) < 0) { msg = "A: row index out of range"; return QPG_ERR_INVALID; }
  }
  hAp[n] = (int)nzA;
  map_A.clear();
  if (reordered) value_map(n, Ap, Ai, false, map_A);
  reordered = false;
  pad_ptr(hAp, (size_t)n + 1, D.stride[H_AP]); pad(hAi, (size_t)nzA, D.stride[H_AI]); pad(hAx, (size_t)nzA, D.stride[H_AX]);
  P.nzA = (int)nzA;
  /* A' pattern (what cholmod_transpose(A,1) builds, iteration.c:81) + permutation into A */
  {
    std::vector<int> cnt(m + 1, 0);
    for (qpg_int k = 0; k < nzA; k++) cnt[hAi[k] + 1]++;
    for (int r = 0; r < m; r++) cnt[r + 1] += cnt[r];
    for (int r = 0; r <= m; r++) hAtp[r] = cnt[r];
    for (int j = 0; j < n; j++)
      for (int k = hAp[j]; k < hAp[j + 1]; k++) { const int dst = cnt[hAi[k]]++; hAti[dst] = j; hAtperm[dst] = k; hAinv[k] = dst; }
    pad_ptr(hAtp, (size_t)m + 1, D.stride[H_ATP]);
    pad(hAti, (size_t)nzA, D.stride[H_ATI]); pad(hAtperm, (size_t)nzA, D.stride[H_ATPERM]); pad(hAinv, (size_t)nzA, D.stride[H_AINV]);
  }
  /* Q: keep the lower triangle only (stype = -1: upper entries are ignored, B6), sorted */
  {
    qpg_int pos = 0;
    for (int j = 0; j < n; j++) {
      if (Qp[j + 1] < Qp[j] || Qp[j] < 0 || Qp[j + 1] > nzQ) { msg = "Q: column pointers not monotone"; return QPG_ERR_INVALID; }
      hQp[j] = (int)pos;
      pos = take_column(tmp, reordered, Qi, Qx, Qp[j], Qp[j + 1], j, n, hQi, hQx, pos);
      if (pos < 0) { msg = "Q: row index out of range"; return QPG_ERR_INVALID; }
    }
    hQp[n] = (int)pos;
    P.nzQ = (int)pos;
    map_Q.clear();
    if (reordered) value_map(n, Qp, Qi, true, map_Q);
    pad_ptr(hQp, (size_t)n + 1, D.stride[H_QP]); pad(hQi, (size_t)pos, D.stride[H_QI]); pad(hQx, (size_t)pos, D.stride[H_QX]);
    /* both triangles, compressed by column (== by row), rows ascending, with the map into Q */
    std::vector<int> cnt(n + 1, 0);
    for (int j = 0; j < n; j++)
      for (int k = hQp[j]; k < hQp[j + 1]; k++) { cnt[j + 1]++; if (hQi[k] != j) cnt[hQi[k] + 1]++; }
    for (int j = 0; j < n; j++) cnt[j + 1] += cnt[j];
    memcpy(hQfp, cnt.data(), ((size_t)n + 1) * sizeof(int));
    P.nzQf = cnt[n];
    std::vector<int> cur(cnt.begin(), cnt.end() - 1);
    for (int j = 0; j < n; j++) /* upper parts: entry (i>j, j) is element (j, i) of column i */
      for (int k = hQp[j]; k < hQp[j + 1]; k++) { const int i = hQi[k]; if (i != j) { const int dst = cur[i]++; hQfi[dst] = j; hQfperm[dst] = k; } }
    for (int j = 0; j < n; j++)
      for (int k = hQp[j]; k < hQp[j + 1]; k++) { const int dst = cur[j]++; hQfi[dst] = hQi[k]; hQfperm[dst] = k; }
    pad_ptr(hQfp, (size_t)n + 1, D.stride[H_QFP]); pad(hQfi, (size_t)cnt[n], D.stride[H_QFI]); pad(hQfperm, (size_t)cnt[n], D.stride[H_QFPERM]);
  }
  {
    double *hq = D.d(H_Q), *hlo = D.d(H_BMIN), *hhi = D.d(H_BMAX);
    memcpy(hq, q, (size_t)n * sizeof(double)); pad(hq, (size_t)n, D.stride[H_Q]);
    if (m) { memcpy(hlo, bmin, (size_t)m * sizeof(double)); memcpy(hhi, bmax, (size_t)m * sizeof(double)); }
    pad(hlo, (size_t)m, D.stride[H_BMIN]); pad(hhi, (size_t)m, D.stride[H_BMAX]);
  }
  P.c = c; P.set = true;
  return QPG_OK;
}

/* Stand-alone test of qpalm_amd/csrc/qpalm_host_convert.h (built and run by tests/test_host_units.py under ASan + UBSan): a caller's problem into the
 * device layout of one member, against references written out here; every refusal with its code and text; guard words behind every stride. */
#include "../../qpalm_amd/csrc/qpalm_host_convert.h"

#include <stdint.h>

static int g_fail = 0, g_checks = 0;
static const char *g_case = "";
#define CHECK(c) do { g_checks++; if (!(c)) { if (++g_fail <= 40) printf("FAIL [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #c); } } while (0)

/* the caller's side */
struct Input {
  int n, m;
  std::vector<qpg_int> Qp, Qi, Ap, Ai;
  std::vector<qpg_float> Qx, Ax, q, bmin, bmax;
};
/* one member's part of a slab with the batch's strides (qpg_batch_create's), GUARD bytes of 0xA5 around every array and 0x77 inside */
struct Slab {
  enum { GUARD = 64 };
  std::vector<unsigned char> buf[H_COUNT];
  ConvertDst D;
  Slab(int n, int m, qpg_int nnzA_max, qpg_int nnzQ_max) {
    const size_t nn = (size_t)n, mm = (size_t)m, zA = (size_t)std::max<qpg_int>(nnzA_max, 1), zQ = (size_t)std::max<qpg_int>(nnzQ_max, 1), zF = 2 * zQ;
    const size_t per[H_COUNT] = {nn + 1, zA, mm + 1, zA, zA, zA, nn + 1, zQ, nn + 1, zF, zF, zA, zQ, nn, mm, mm};
    for (int a = 0; a < H_COUNT; a++) {
      const size_t bytes = per[a] * (a >= H_AX ? sizeof(double) : sizeof(int));
      buf[a].assign(bytes + 2 * GUARD, 0xA5);
      memset(buf[a].data() + GUARD, 0x77, bytes);
      D.p[a] = buf[a].data() + GUARD; D.stride[a] = per[a];
    }
  }
  bool guards_intact() const {
    for (int a = 0; a < H_COUNT; a++)
      for (size_t k = 0; k < GUARD; k++) if (buf[a][k] != 0xA5 || buf[a][buf[a].size() - 1 - k] != 0xA5) return false;
    return true;
  }
};
static int convert(const Slab &S, const Input &in, HostProblem &P, std::vector<int> &map_A, std::vector<int> &map_Q, std::string &msg,
                   bool with_q = true, bool with_bounds = true) {
  return convert_problem(S.D, in.n, in.m, in.Qp.data(), in.Qi.data(), in.Qx.data(), in.Ap.data(), in.Ai.data(), in.Ax.data(), with_q ? in.q.data() : nullptr, 1.5,
                         with_bounds ? in.bmin.data() : nullptr, with_bounds ? in.bmax.data() : nullptr, P, map_A, map_Q, msg);
}

static unsigned g_seed = 2024u;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

enum { Q_LOWER, Q_BOTH, Q_UPPER };
/* a random problem; every value is its own position + 1 (distinct, exact in sums); unsorted: every column's entries reversed; dup: a row twice in a column of A */
static Input make_input(int n, int m, int qmode, bool unsorted, bool dup, int empty_col) {
  Input in;
  in.n = n; in.m = m;
  in.Ap.push_back(0); in.Qp.push_back(0);
  for (int j = 0; j < n; j++) {
    std::vector<qpg_int> ra, rq;
    if (j != empty_col) {
      for (int i = 0; i < m; i++) if (rnd() % 3 == 0) ra.push_back(i);
      if (dup && m > 0 && j == n / 2) { ra.push_back(m - 1); ra.push_back(0); ra.push_back(m - 1); std::sort(ra.begin(), ra.end()); }
      for (int i = 0; i < n; i++) {
        const bool on = i == j || rnd() % 3 == 0;
        if (on && (qmode == Q_BOTH || (qmode == Q_LOWER && i >= j) || (qmode == Q_UPPER && i <= j))) rq.push_back(i);
      }
    }
    if (unsorted) { std::reverse(ra.begin(), ra.end()); std::reverse(rq.begin(), rq.end()); }
    for (qpg_int i : ra) { in.Ai.push_back(i); in.Ax.push_back((double)in.Ai.size()); }
    for (qpg_int i : rq) { in.Qi.push_back(i); in.Qx.push_back(1000.0 + (double)in.Qi.size()); }
    in.Ap.push_back((qpg_int)in.Ai.size()); in.Qp.push_back((qpg_int)in.Qi.size());
  }
  for (int j = 0; j < n; j++) in.q.push_back(0.25 + j);
  for (int i = 0; i < m; i++) { in.bmin.push_back(-1.0 - i); in.bmax.push_back(2.0 + i); }
  /* (never empty arrays: data() of an empty vector may be null) */
  in.Ai.reserve(in.Ai.size() + 1); in.Ax.reserve(in.Ax.size() + 1); in.Qi.reserve(in.Qi.size() + 1); in.Qx.reserve(in.Qx.size() + 1);
  in.bmin.reserve((size_t)m + 1); in.bmax.reserve((size_t)m + 1);
  return in;
}

/* a column's kept entries in the device's order: the caller's positions, stably sorted by row */
static std::vector<qpg_int> kept_sorted(const std::vector<qpg_int> &Pc, const std::vector<qpg_int> &I, int j, qpg_int rmin) {
  std::vector<qpg_int> pos;
  for (qpg_int k = Pc[j]; k < Pc[j + 1]; k++) if (I[k] >= rmin) pos.push_back(k);
  /* insertion sort: stable by construction */
  for (size_t a = 1; a < pos.size(); a++) for (size_t b = a; b > 0 && I[pos[b]] < I[pos[b - 1]]; b--) std::swap(pos[b], pos[b - 1]);
  return pos;
}

static void check_ok(const char *name, const Input &in, int ns, int ms, qpg_int nnzA_max, qpg_int nnzQ_max) {
  g_case = name;
  const int n = in.n, m = in.m;
  Slab S(ns, ms, nnzA_max, nnzQ_max);
  HostProblem P;
  memset(&P, 0, sizeof P);
  std::vector<int> map_A(3, -1), map_Q(3, -1);
  std::string msg;
  const int rc = convert(S, in, P, map_A, map_Q, msg, true, m > 0);
  CHECK(rc == QPG_OK && msg.empty());
  CHECK(S.guards_intact());
  if (rc != QPG_OK) return;
  const ConvertDst &D = S.D;
  const int *Ap = D.i(H_AP), *Ai = D.i(H_AI), *Atp = D.i(H_ATP), *Ati = D.i(H_ATI), *Atperm = D.i(H_ATPERM), *Ainv = D.i(H_AINV);
  const int *Qp = D.i(H_QP), *Qi = D.i(H_QI), *Qfp = D.i(H_QFP), *Qfi = D.i(H_QFI), *Qfperm = D.i(H_QFPERM);
  const double *Ax = D.d(H_AX), *Qx = D.d(H_QX);
  /* expected A and lower Q, entry for entry, and the maps */
  std::vector<qpg_int> eA, eQ;
  bool orderA = true, orderQ = true;
  for (int j = 0; j < n; j++) {
    CHECK(Ap[j] == (int)eA.size() && Qp[j] == (int)eQ.size());
    const std::vector<qpg_int> a = kept_sorted(in.Ap, in.Ai, j, 0), q = kept_sorted(in.Qp, in.Qi, j, j);
    eA.insert(eA.end(), a.begin(), a.end()); eQ.insert(eQ.end(), q.begin(), q.end());
  }
  for (size_t k = 0; k < eA.size(); k++) if (eA[k] != (qpg_int)k) orderA = false;
  if (eQ.size() != in.Qi.size()) orderQ = false;
  for (size_t k = 0; k < eQ.size(); k++) if (eQ[k] != (qpg_int)k) orderQ = false;
  const int nzA = (int)eA.size(), nzQ = (int)eQ.size();
  CHECK(Ap[n] == nzA && Qp[n] == nzQ);
  CHECK(P.set && P.n == n && P.m == m && P.nzA == nzA && P.nzQ == nzQ && P.c == 1.5);
  for (int k = 0; k < nzA; k++) CHECK(Ai[k] == (int)in.Ai[eA[k]] && Ax[k] == in.Ax[eA[k]]);
  for (int k = 0; k < nzQ; k++) CHECK(Qi[k] == (int)in.Qi[eQ[k]] && Qx[k] == in.Qx[eQ[k]]);
  for (int j = 0; j < n; j++) {
    for (int k = Ap[j] + 1; k < Ap[j + 1]; k++) CHECK(Ai[k - 1] <= Ai[k]);
    for (int k = Qp[j]; k < Qp[j + 1]; k++) { CHECK(Qi[k] >= j); if (k > Qp[j]) CHECK(Qi[k - 1] <= Qi[k]); }
  }
  CHECK(map_A.empty() == orderA);
  CHECK(map_Q.empty() == orderQ);
  if (!map_A.empty()) { CHECK((int)map_A.size() == nzA); for (int k = 0; k < nzA && k < (int)map_A.size(); k++) CHECK(map_A[k] == (int)eA[k] && Ax[k] == in.Ax[map_A[k]]); }
  if (!map_Q.empty()) { CHECK((int)map_Q.size() == nzQ); for (int k = 0; k < nzQ && k < (int)map_Q.size(); k++) CHECK(map_Q[k] == (int)eQ[k] && Qx[k] == in.Qx[map_Q[k]]); }
  /* dense reconstruction: A and the lower Q from the converted arrays = from the caller's (duplicates add up) */
  std::vector<double> dA((size_t)m * n + 1, 0.0), cA((size_t)m * n + 1, 0.0), dQ((size_t)n * n, 0.0), cQ((size_t)n * n, 0.0), dF((size_t)n * n, 0.0);
  for (int j = 0; j < n; j++) {
    for (int k = Ap[j]; k < Ap[j + 1]; k++) dA[(size_t)Ai[k] * n + j] += Ax[k];
    for (qpg_int k = in.Ap[j]; k < in.Ap[j + 1]; k++) cA[(size_t)in.Ai[k] * n + j] += in.Ax[k];
    for (int k = Qp[j]; k < Qp[j + 1]; k++) dQ[(size_t)Qi[k] * n + j] += Qx[k];
    for (qpg_int k = in.Qp[j]; k < in.Qp[j + 1]; k++) if (in.Qi[k] >= j) cQ[(size_t)in.Qi[k] * n + j] += in.Qx[k];
  }
  CHECK(dA == cA);
  CHECK(dQ == cQ);
  /* A' with its two maps */
  CHECK(Atp[0] == 0 && Atp[m] == nzA);
  std::vector<int> colof((size_t)nzA + 1, -1), seen((size_t)nzA + 1, 0);
  for (int j = 0; j < n; j++) for (int k = Ap[j]; k < Ap[j + 1]; k++) colof[k] = j;
  for (int r = 0; r < m; r++) {
    CHECK(Atp[r] <= Atp[r + 1]);
    for (int k = Atp[r]; k < Atp[r + 1]; k++) {
      const int s = Atperm[k];
      const bool in_range = s >= 0 && s < nzA;
      CHECK(in_range);
      if (!in_range) continue;
      CHECK(Ai[s] == r && colof[s] == Ati[k] && Ainv[s] == k);
      seen[s]++;
      if (k > Atp[r]) CHECK(Ati[k - 1] < Ati[k] || (Ati[k - 1] == Ati[k] && Atperm[k - 1] < s));
    }
  }
  for (int k = 0; k < nzA; k++) CHECK(seen[k] == 1);
  /* both triangles of Q: rows ascending, Qx[Qfperm[k]] the value of entry k */
  int offdiag = 0;
  std::vector<int> qcol((size_t)nzQ + 1, -1), qseen((size_t)nzQ + 1, 0);
  for (int j = 0; j < n; j++) for (int k = Qp[j]; k < Qp[j + 1]; k++) { qcol[k] = j; if (Qi[k] != j) offdiag++; }
  CHECK(Qfp[0] == 0 && Qfp[n] == nzQ + offdiag && P.nzQf == nzQ + offdiag);
  for (int j = 0; j < n; j++) {
    CHECK(Qfp[j] <= Qfp[j + 1]);
    for (int k = Qfp[j]; k < Qfp[j + 1]; k++) {
      const int s = Qfperm[k], i = Qfi[k];
      const bool in_range = s >= 0 && s < nzQ && i >= 0 && i < n;
      CHECK(in_range);
      if (!in_range) continue;
      CHECK((Qi[s] == i && qcol[s] == j) || (Qi[s] == j && qcol[s] == i));
      qseen[s]++;
      dF[(size_t)i * n + j] += Qx[s];
      if (k > Qfp[j]) CHECK(Qfi[k - 1] <= i);
    }
  }
  for (int k = 0; k < nzQ; k++) CHECK(qseen[k] == (Qi[k] == qcol[k] ? 1 : 2));
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) CHECK(dF[(size_t)i * n + j] == (i >= j ? cQ[(size_t)i * n + j] : cQ[(size_t)j * n + i]));
  /* q, bounds */
  for (int j = 0; j < n; j++) CHECK(D.d(H_Q)[j] == in.q[j]);
  for (int i = 0; i < m; i++) CHECK(D.d(H_BMIN)[i] == in.bmin[i] && D.d(H_BMAX)[i] == in.bmax[i]);
  /* padding up to the strides: zeros, pointers repeat their last value */
  const size_t used[H_COUNT] = {(size_t)n + 1, (size_t)nzA, (size_t)m + 1, (size_t)nzA, (size_t)nzA, (size_t)nzA, (size_t)n + 1, (size_t)nzQ, (size_t)n + 1,
                                (size_t)P.nzQf, (size_t)P.nzQf, (size_t)nzA, (size_t)nzQ, (size_t)n, (size_t)m, (size_t)m};
  for (int a = 0; a < H_COUNT; a++) {
    CHECK(used[a] <= D.stride[a]);
    const bool ptr = a == H_AP || a == H_ATP || a == H_QP || a == H_QFP;
    for (size_t k = used[a]; k < D.stride[a]; k++) {
      if (a >= H_AX) CHECK(D.d(a)[k] == 0.0);
      else CHECK(D.i(a)[k] == (ptr ? D.i(a)[used[a] - 1] : 0));
    }
  }
}

/* a refusal: code, text, nothing outside the strides; nnz limits as for the input unless given */
static void check_refused(const char *name, const Input &in, const char *text, bool with_q = true, bool with_bounds = true, qpg_int nnzA_max = -1, qpg_int nnzQ_max = -1) {
  g_case = name;
  Slab S(in.n, in.m, nnzA_max >= 0 ? nnzA_max : (qpg_int)in.Ai.size(), nnzQ_max >= 0 ? nnzQ_max : (qpg_int)in.Qi.size());
  HostProblem P;
  memset(&P, 0, sizeof P);
  std::vector<int> map_A, map_Q;
  std::string msg;
  const int rc = convert(S, in, P, map_A, map_Q, msg, with_q, with_bounds);
  CHECK(rc == QPG_ERR_INVALID);
  if (msg != text) printf("  [%s] message: \"%s\"\n", name, msg.c_str());
  CHECK(msg == text);
  CHECK(!P.set);
  CHECK(S.guards_intact());
}

int main() {
  {
    const Input a = make_input(7, 5, Q_LOWER, false, false, -1);
    check_ok("sorted", a, 7, 5, (qpg_int)a.Ai.size() + 4, (qpg_int)a.Qi.size() + 4);
    check_ok("sorted, nnz exactly at the limits", a, 7, 5, (qpg_int)a.Ai.size(), (qpg_int)a.Qi.size());
    check_ok("sorted, smaller than the strides", a, 10, 7, (qpg_int)a.Ai.size() + 9, (qpg_int)a.Qi.size() + 5);
    const Input d = make_input(7, 5, Q_LOWER, false, true, -1);
    check_ok("sorted with duplicate rows", d, 7, 5, (qpg_int)d.Ai.size(), (qpg_int)d.Qi.size());
    const Input u = make_input(9, 6, Q_LOWER, true, true, -1);
    check_ok("unsorted columns, duplicates", u, 9, 6, (qpg_int)u.Ai.size() + 1, (qpg_int)u.Qi.size() + 1);
    check_ok("unsorted, smaller than the strides", u, 12, 9, (qpg_int)u.Ai.size() + 7, (qpg_int)u.Qi.size() + 3);
    const Input b = make_input(8, 4, Q_BOTH, false, false, -1);
    check_ok("Q with both triangles", b, 8, 4, (qpg_int)b.Ai.size(), (qpg_int)b.Qi.size());
    const Input bu = make_input(8, 4, Q_BOTH, true, false, -1);
    check_ok("Q with both triangles, unsorted", bu, 8, 4, (qpg_int)bu.Ai.size(), (qpg_int)bu.Qi.size());
    const Input up = make_input(8, 4, Q_UPPER, false, false, -1);
    check_ok("Q upper only", up, 8, 4, (qpg_int)up.Ai.size(), (qpg_int)up.Qi.size());
    { /* ... keeps the diagonal alone */
      g_case = "Q upper only: diagonal";
      Slab S(8, 4, (qpg_int)up.Ai.size(), (qpg_int)up.Qi.size());
      HostProblem P; memset(&P, 0, sizeof P);
      std::vector<int> mA, mQ; std::string msg;
      CHECK(convert(S, up, P, mA, mQ, msg) == QPG_OK);
      CHECK(P.nzQ == 8 && P.nzQf == 8);
      for (int j = 0; j < 8; j++) CHECK(S.D.i(H_QI)[j] == j && S.D.i(H_QFI)[j] == j);
    }
    const Input z = make_input(6, 0, Q_LOWER, false, false, -1);
    check_ok("m = 0", z, 6, 0, 0, (qpg_int)z.Qi.size());
    check_ok("m = 0 in a batch with rows", z, 6, 3, 5, (qpg_int)z.Qi.size());
    const Input e = make_input(7, 5, Q_LOWER, false, false, 3);
    check_ok("an empty column", e, 7, 5, (qpg_int)e.Ai.size(), (qpg_int)e.Qi.size());
    const Input e0 = make_input(7, 5, Q_BOTH, true, false, 0);
    check_ok("an empty first column, unsorted", e0, 7, 5, (qpg_int)e0.Ai.size(), (qpg_int)e0.Qi.size());
    const Input one = make_input(1, 1, Q_LOWER, false, false, -1);
    check_ok("n = 1", one, 1, 1, 1, 1);
    for (int it = 0; it < 60; it++) {
      const int n = 1 + (int)(rnd() % 12), m = (int)(rnd() % 9);
      const Input r = make_input(n, m, (int)(rnd() % 3), rnd() % 2 != 0, rnd() % 2 != 0, rnd() % 4 == 0 ? (int)(rnd() % (unsigned)n) : -1);
      check_ok("random", r, n + (int)(rnd() % 3), m + (int)(rnd() % 3), (qpg_int)r.Ai.size() + (qpg_int)(rnd() % 3), (qpg_int)r.Qi.size() + (qpg_int)(rnd() % 3));
    }
  }
  { /* refusals */
    Input base = make_input(7, 5, Q_LOWER, false, false, -1);
    while (base.Ap[1] < 1 || base.Ap[2] - base.Ap[1] < 1 || base.Qp[2] - base.Qp[1] < 1) base = make_input(7, 5, Q_LOWER, false, false, -1);
    const char *START = "qpg_batch_set_problem: column pointers must start at 0", *MANY = "qpg_batch_set_problem: more nonzeros than nnzA_max / nnzQ_max";
    Input x;
    x = base; x.Ap[0] = 1; check_refused("Ap[0] != 0", x, START);
    x = base; x.Qp[0] = 1; check_refused("Qp[0] != 0", x, START);
    check_refused("Ap[n] > nnzA_max", base, MANY, true, true, (qpg_int)base.Ai.size() - 1, -1);
    check_refused("Qp[n] > nnzQ_max", base, MANY, true, true, -1, (qpg_int)base.Qi.size() - 1);
    x = base; x.Ap[7] = -1; check_refused("negative Ap[n]", x, MANY);
    x = base; x.Qp[7] = -1; check_refused("negative Qp[n]", x, MANY);
    x = base; x.Ap[2] = x.Ap[1] - 1; check_refused("A: non-monotone pointers", x, "A: column pointers not monotone");
    x = base; x.Qp[2] = x.Qp[1] - 1; check_refused("Q: non-monotone pointers", x, "Q: column pointers not monotone");
    x = base; x.Ap[1] = x.Ap[7] + 1; check_refused("A: a pointer above Ap[n]", x, "A: column pointers not monotone");
    x = base; x.Qp[1] = x.Qp[7] + 1; check_refused("Q: a pointer above Qp[n]", x, "Q: column pointers not monotone");
    x = base; x.Ap[3] = (qpg_int)1 << 40; check_refused("A: a pointer beyond int32", x, "A: column pointers not monotone");
    x = base; x.Ai[x.Ai.size() - 1] = 5; check_refused("A: row index = m", x, "A: row index out of range");
    x = base; x.Ai[0] = -1; check_refused("A: negative row index", x, "A: row index out of range");
    x = base; x.Ai[1] = ((qpg_int)1 << 32) + 1; check_refused("A: row index beyond int32", x, "A: row index out of range");
    x = base; x.Qi[x.Qi.size() - 1] = 7; check_refused("Q: row index = n", x, "Q: row index out of range");
    x = base; x.Qi[0] = -1; check_refused("Q: negative row index", x, "Q: row index out of range");
    x = base; x.bmin[4] = 3.0; x.bmax[4] = 2.5; check_refused("bmin > bmax at the last row", x, "Lower bound at index 4 is greater than upper bound: 3.0000e+00 > 2.5000e+00");
    check_refused("NULL q", base, "Missing data", false, true);
    check_refused("NULL bounds with m > 0", base, "Missing data", true, false);
    /* several violations: the first check in the order of the source decides */
    x = base; x.Ap[0] = 1; check_refused("NULL q before Ap[0] != 0", x, "Missing data", false, true);
    x = base; x.Ap[0] = 1; x.bmin[0] = 9.0; x.bmax[0] = 1.0; check_refused("bounds before Ap[0] != 0", x, "Lower bound at index 0 is greater than upper bound: 9.0000e+00 > 1.0000e+00");
    x = base; x.Ap[0] = 1; x.Ap[7] = -1; check_refused("Ap[0] != 0 before the counts", x, START);
    x = base; x.Ai[0] = -1; x.Qi[0] = -1; x.Qp[2] = x.Qp[1] - 1; check_refused("A before Q", x, "A: row index out of range");
  }
  printf("%d checks\n%d failures\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}

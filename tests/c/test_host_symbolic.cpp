/* Stand-alone test of qpalm_amd/csrc/qpalm_host_symbolic.h (built and run by tests/test_host_units.py under ASan + UBSan): the ordering, the symbolic
 * factorisation, the factor-numbering index arrays and the launch plans of sparse coop mode against dense, obvious references. */
#include "../../qpalm_amd/csrc/qpalm_host_symbolic.h"

#include <stdio.h>

#include <set>
#include <utility>

static int g_fail = 0, g_checks = 0;
static const char *g_case = "";
#define CHECK(c) do { g_checks++; if (!(c)) { if (++g_fail <= 40) printf("FAIL [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #c); } } while (0)

typedef std::vector<std::vector<char> > Dense;
typedef std::vector<std::pair<int, int> > Edges;
typedef std::vector<std::vector<int> > Rows;

/* a member's patterns as the conversion leaves them: A by columns and by rows (rows ascending), Q with both triangles and its diagonal */
struct Prob {
  int n, m;
  std::vector<int> Ap, Ai, Atp, Ati, Qfp, Qfi;
  SparsePattern pat() const { return SparsePattern{n, m, Ap.data(), Ai.data(), Atp.data(), Ati.data(), Qfp.data(), Qfi.data()}; }
};
static Prob make_prob(int n, const Edges &q, const Rows &a) {
  Prob P;
  P.n = n; P.m = (int)a.size();
  std::vector<std::set<int> > qa((size_t)n), ac((size_t)n);
  for (int j = 0; j < n; j++) qa[j].insert(j);
  for (auto &e : q) { qa[e.first].insert(e.second); qa[e.second].insert(e.first); }
  P.Qfp.assign(1, 0);
  for (int j = 0; j < n; j++) { for (int i : qa[j]) P.Qfi.push_back(i); P.Qfp.push_back((int)P.Qfi.size()); }
  P.Atp.assign(1, 0);
  for (int t = 0; t < P.m; t++) {
    std::set<int> r(a[t].begin(), a[t].end());
    for (int j : r) { P.Ati.push_back(j); ac[j].insert(t); }
    P.Atp.push_back((int)P.Ati.size());
  }
  P.Ap.assign(1, 0);
  for (int j = 0; j < n; j++) { for (int t : ac[j]) P.Ai.push_back(t); P.Ap.push_back((int)P.Ai.size()); }
  P.Ai.push_back(0); P.Ati.push_back(0); /* (never empty arrays: data() of an empty vector may be null) */
  return P;
}
/* H = Q + A'A and K = [[Q, A'], [A, I]] as dense boolean matrices */
static Dense dense_H(int n, const Edges &q, const Rows &a) {
  Dense H((size_t)n, std::vector<char>((size_t)n, 0));
  for (int j = 0; j < n; j++) H[j][j] = 1;
  for (auto &e : q) H[e.first][e.second] = H[e.second][e.first] = 1;
  for (auto &r : a) for (int i : r) for (int j : r) H[i][j] = 1;
  return H;
}
static Dense dense_K(int n, const Edges &q, const Rows &a) {
  const int nf = n + (int)a.size();
  Dense K((size_t)nf, std::vector<char>((size_t)nf, 0));
  for (int j = 0; j < nf; j++) K[j][j] = 1;
  for (auto &e : q) K[e.first][e.second] = K[e.second][e.first] = 1;
  for (size_t t = 0; t < a.size(); t++) for (int j : a[t]) K[(size_t)n + t][j] = K[j][(size_t)n + t] = 1;
  return K;
}

static bool is_perm(const std::vector<int> &p, int n) {
  if (p.size() != (size_t)n) return false;
  std::vector<char> seen((size_t)n, 0);
  for (int v : p) { if (v < 0 || v >= n || seen[v]) return false; seen[v] = 1; }
  return true;
}
static bool is_identity(const std::vector<int> &p) { for (size_t j = 0; j < p.size(); j++) if (p[j] != (int)j) return false; return true; }

/* every invariant of a SparseSym against the boolean dense elimination of P M P' */
static void check_sym(const Dense &M, const SparseSym &S) {
  const int n = (int)M.size();
  CHECK(is_perm(S.perm, n));
  CHECK(S.iperm.size() == (size_t)n);
  if (!is_perm(S.perm, n) || S.iperm.size() != (size_t)n) return;
  for (int j = 0; j < n; j++) CHECK(S.iperm[S.perm[j]] == j);
  Dense F((size_t)n, std::vector<char>((size_t)n, 0));
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) F[i][j] = M[S.perm[i]][S.perm[j]];
  std::vector<int> below;
  for (int k = 0; k < n; k++) {
    below.clear();
    for (int i = k + 1; i < n; i++) if (F[i][k]) below.push_back(i);
    for (int i : below) for (int j : below) F[i][j] = 1;
  }
  /* Lp / Li: the strict lower part of F, column by column, rows ascending */
  CHECK(S.Lp.size() == (size_t)n + 1 && S.Lp[0] == 0);
  if (S.Lp.size() != (size_t)n + 1) return;
  bool same = true;
  for (int k = 0; k < n && same; k++) {
    int e = S.Lp[k];
    for (int i = k + 1; i < n; i++) if (F[i][k]) { if (e >= S.Lp[k + 1] || (size_t)e >= S.Li.size() || S.Li[e] != i) { same = false; break; } e++; }
    if (e != S.Lp[k + 1]) same = false;
  }
  CHECK(same);
  CHECK((size_t)S.Lp[n] == S.Li.size());
  if (!same || (size_t)S.Lp[n] != S.Li.size()) return;
  const size_t nz = S.Li.size();
  /* Rp / Rk / Rpos: the same entries by rows, columns ascending */
  CHECK(S.Rp.size() == (size_t)n + 1 && S.Rk.size() == nz && S.Rpos.size() == nz);
  if (S.Rp.size() != (size_t)n + 1 || S.Rk.size() != nz || S.Rpos.size() != nz) return;
  CHECK(S.Rp[0] == 0 && (size_t)S.Rp[n] == nz);
  std::vector<char> hit(nz, 0);
  for (int i = 0; i < n; i++) {
    int e = S.Rp[i];
    for (int k = 0; k < i; k++) if (F[i][k]) {
      const bool in = e < S.Rp[i + 1];
      CHECK(in);
      if (!in) return;
      CHECK(S.Rk[e] == k);
      const int pos = S.Rpos[e];
      CHECK(pos >= S.Lp[k] && pos < S.Lp[k + 1] && S.Li[pos] == i);
      if (pos >= 0 && (size_t)pos < nz) hit[pos] = 1;
      e++;
    }
    CHECK(e == S.Rp[i + 1]);
  }
  for (size_t e = 0; e < nz; e++) CHECK(hit[e]);
  /* levels: 0 for a column nothing flows into, else 1 + the highest level among the columns k with L[j,k] != 0 */
  std::vector<int> level((size_t)n, 0);
  int height = 0;
  for (int j = 0; j < n; j++) {
    for (int k = 0; k < j; k++) if (F[j][k]) level[j] = std::max(level[j], level[k] + 1);
    height = std::max(height, level[j] + 1);
  }
  CHECK(S.nlev == height);
  CHECK(S.levptr.size() == (size_t)height + 1 && S.levcol.size() == (size_t)n);
  if (S.levptr.size() != (size_t)height + 1 || S.levcol.size() != (size_t)n) return;
  CHECK(S.levptr[0] == 0 && S.levptr[height] == n);
  CHECK(is_perm(S.levcol, n));
  for (int l = 0; l < height; l++) {
    CHECK(S.levptr[l] <= S.levptr[l + 1]);
    for (int e = S.levptr[l]; e < S.levptr[l + 1] && e < n && e >= 0; e++) CHECK(S.levcol[e] >= 0 && S.levcol[e] < n && level[S.levcol[e]] == l);
  }
}

/* atip / qfip / first, with three entries of stride beyond the member's own */
static void check_index(const Prob &P, const SparseSym &S, bool kkt) {
  const size_t zA = (size_t)P.Atp[P.m] + 3, zF = (size_t)P.Qfp[P.n] + 3, zm = (size_t)P.m + 3;
  std::vector<int> atip(zA, -7), qfip(zF, -7), first(zm, -7);
  sparse_factor_index(P.pat(), S, kkt, atip, qfip, first);
  CHECK(atip.size() == zA && qfip.size() == zF && first.size() == zm);
  for (int t = 0; t < P.m; t++) {
    int f = P.n;
    for (int q = P.Atp[t]; q < P.Atp[t + 1]; q++) { CHECK(atip[q] == S.iperm[P.Ati[q]]); f = std::min(f, S.iperm[P.Ati[q]]); }
    CHECK(first[t] == (kkt ? S.iperm[P.n + t] : f));
  }
  for (int k = 0; k < P.Qfp[P.n]; k++) CHECK(qfip[k] == S.iperm[P.Qfi[k]]);
  for (size_t k = zA - 3; k < zA; k++) CHECK(atip[k] == 0);
  for (size_t k = zF - 3; k < zF; k++) CHECK(qfip[k] == 0);
  for (size_t k = zm - 3; k < zm; k++) CHECK(first[k] == 0);
}

/* one phase of a plan: tiles [0, nlev) in order; grid = 1 exactly for runs of levels of at most `round` columns (or G = 1), maximal runs; a wider
 * level alone on min(G, ceil(w / round)) workgroups */
static void check_phase(const std::vector<SpLaunch> &L, const std::vector<int> &levptr, int nlev, int round, int G) {
  int at = 0;
  bool prev_narrow = false;
  for (const SpLaunch &l : L) {
    CHECK(l.lev0 == at && l.lev1 > l.lev0 && l.lev1 <= nlev);
    if (l.lev0 != at || l.lev1 <= l.lev0 || l.lev1 > nlev) return;
    bool narrow = true;
    for (int v = l.lev0; v < l.lev1; v++) if (levptr[v + 1] - levptr[v] > round) narrow = false;
    CHECK((l.grid == 1) == (narrow || G == 1));
    if (!narrow && G > 1) {
      const int w = levptr[l.lev0 + 1] - levptr[l.lev0];
      CHECK(l.lev1 == l.lev0 + 1);
      CHECK(l.grid == std::min(G, (w + round - 1) / round));
    }
    if (G > 1) CHECK(!(narrow && prev_narrow)); /* consecutive narrow levels are ONE launch */
    prev_narrow = narrow;
    at = l.lev1;
  }
  CHECK(at == nlev);
  if (G == 1) CHECK(L.size() == (nlev > 0 ? 1u : 0u));
}
static void check_plans(const SparseSym &S, int n) {
  const int rounds[3] = {1, 8, 64}, Gs[3] = {1, 3, 256};
  for (int rf : rounds) for (int rs : rounds) for (int G : Gs) {
    SpPlan P;
    sparse_coop_plan(S.levptr, S.nlev, n, rf, rs, G, P);
    check_phase(P.factor, S.levptr, S.nlev, rf, G);
    check_phase(P.solve, S.levptr, S.nlev, rs, G);
    CHECK(P.vec_grid == std::max(1, std::min(G, (n + rs - 1) / rs)));
    CHECK(P.solve_launches == 2 + 2 * (int)P.solve.size() + ((!P.solve.empty() && P.solve[0].grid > 1) ? 1 : 0));
    int mg = P.vec_grid;
    for (auto &l : P.factor) mg = std::max(mg, l.grid);
    for (auto &l : P.solve) mg = std::max(mg, l.grid);
    CHECK(P.max_grid == mg);
  }
}

static const size_t NO_LIMIT = (size_t)1 << 30;
/* one pattern under the natural ordering and under sparse_order, as H and (kkt) as K: everything above.  Returns the dissected analysis of H */
static SparseSym run_pattern(const char *name, int n, const Edges &q, const Rows &a, bool kkt) {
  g_case = name;
  const Prob P = make_prob(n, q, a);
  const Dense H = dense_H(n, q, a), K = dense_K(n, q, a);
  SparseSym keep;
  for (int k = 0; k <= (kkt ? 1 : 0); k++)
    for (int ordering = 0; ordering <= 1; ordering++) {
      SparseSym S;
      std::string why;
      const int rc = sparse_symbolic(P.pat(), k != 0, ordering, NO_LIMIT, S, why);
      CHECK(rc == 0 && why.empty());
      CHECK(S.dissected == (ordering == 1));
      if (ordering == 0) CHECK(is_identity(S.perm));
      check_sym(k ? K : H, S);
      check_index(P, S, k != 0);
      check_plans(S, k ? n + P.m : n);
      if (!k && ordering == 1) keep = S;
    }
  return keep;
}

static Edges band(int n, int lo = 0) { Edges e; for (int j = 0; j + 1 < n; j++) e.push_back(std::make_pair(lo + j, lo + j + 1)); return e; }

/* the glibc-independent generator of the random patterns */
static unsigned g_seed = 12345u;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

int main() {
  { /* n = 1, n = 2 */
    run_pattern("n=1", 1, Edges(), Rows(), true);
    run_pattern("n=2", 2, Edges{{0, 1}}, Rows{{0}, {0, 1}}, true);
    run_pattern("n=2 diagonal", 2, Edges(), Rows(), true);
  }
  { /* LEAF = 24: 25 is the first piece that is split */
    const SparseSym a = run_pattern("band 24", 24, band(24), Rows(), false);
    CHECK(is_identity(a.perm));
    const SparseSym b = run_pattern("band 25", 25, band(25), Rows(), false);
    CHECK(!is_identity(b.perm));
    CHECK(b.nlev < 25);
  }
  { /* complete graph: fewer than 3 levels, natural order */
    Edges e;
    for (int i = 0; i < 30; i++) for (int j = 0; j < i; j++) e.push_back(std::make_pair(i, j));
    const SparseSym s = run_pattern("complete 30", 30, e, Rows(), false);
    CHECK(is_identity(s.perm));
  }
  { /* 12 x 12 grid: a separator inside the 30-70 % window; separator vertices without a neighbour beyond it join the first half */
    Edges e;
    for (int r = 0; r < 12; r++) for (int c = 0; c < 12; c++) { if (c + 1 < 12) e.push_back(std::make_pair(r * 12 + c, r * 12 + c + 1)); if (r + 1 < 12) e.push_back(std::make_pair(r * 12 + c, r * 12 + 12 + c)); }
    const SparseSym s = run_pattern("grid 12x12", 144, e, Rows(), false);
    CHECK(!is_identity(s.perm));
  }
  { /* a star of 26: three levels from a leaf, no level in the window: the median's level is the separator */
    Edges e;
    for (int j = 1; j < 26; j++) e.push_back(std::make_pair(0, j));
    const SparseSym s = run_pattern("star 26", 26, e, Rows(), false);
    CHECK(s.perm.size() == 26 && s.perm[25] == 0); /* the centre is the separator: last */
  }
  { /* 40 isolated vertices and three disjoint bands of 30: the component loop */
    Edges e;
    for (int b = 0; b < 3; b++) { const Edges x = band(30, 40 + 30 * b); e.insert(e.end(), x.begin(), x.end()); }
    run_pattern("components", 130, e, Rows(), false);
  }
  { /* arrow: the shaft (vertex 0, degree 119 > hub_deg = 48) is set aside and ordered last */
    Edges e = band(119, 1);
    for (int j = 1; j < 120; j++) e.push_back(std::make_pair(0, j));
    const SparseSym s = run_pattern("arrow 120", 120, e, Rows(), false);
    CHECK(s.perm.size() == 120 && s.perm[119] == 0);
    /* ... and the other 119 are ordered exactly as the band without the shaft */
    const Prob B = make_prob(119, band(119), Rows());
    SparseAdj G;
    std::vector<int> alone;
    sparse_adj_H(B.pat(), G);
    sparse_order(G, 119, alone);
    CHECK(alone.size() == 119 && !is_identity(alone));
    for (int k = 0; k < 119 && alone.size() == 119 && s.perm.size() == 120; k++) CHECK(s.perm[k] == alone[k] + 1);
  }
  { /* long rows of A: 64 entries = a clique of the ordering's graph, 65 = a chain */
    for (int len = 64; len <= 65; len++) {
      g_case = len == 64 ? "row of 64" : "row of 65";
      Rows a(1);
      for (int j = 0; j < len; j++) a[0].push_back(2 * j); /* columns 0, 2, 4, ... of n = 140 */
      const Prob P = make_prob(140, Edges(), a);
      SparseAdj G;
      sparse_adj_H(P.pat(), G);
      CHECK(G.p.size() == 141);
      for (int v = 0; v < 140; v++) {
        std::set<int> got(G.i.begin() + G.p[v], G.i.begin() + G.p[v + 1]), want;
        CHECK((int)got.size() == G.p[v + 1] - G.p[v]); /* no repeats */
        if (v % 2 == 0 && v / 2 < len) {
          if (len == 64) { for (int j = 0; j < len; j++) if (2 * j != v) want.insert(2 * j); }
          else { if (v >= 2) want.insert(v - 2); if (v / 2 + 1 < len) want.insert(v + 2); }
        }
        CHECK(got == want);
      }
      run_pattern(g_case, 140, Edges(), a, true);
    }
  }
  { /* K of a banded QP with 40 rows, the last one dense: natural = [x; y], dissected = the dense row's vertex last */
    Rows a;
    for (int t = 0; t < 39; t++) a.push_back(std::vector<int>{t, t + 1});
    a.push_back(std::vector<int>());
    for (int j = 0; j < 60; j++) a.back().push_back(j);
    run_pattern("kkt dense row", 60, band(60), a, true);
    const Prob P = make_prob(60, band(60), a);
    SparseSym S;
    std::string why;
    CHECK(sparse_symbolic(P.pat(), true, -1, NO_LIMIT, S, why) == 0); /* automatic = dissected in KKT mode */
    CHECK(S.dissected && S.perm.size() == 100 && S.perm[99] == 60 + 39);
    SparseAdj G;
    sparse_adj_K(P.pat(), G);
    const Dense K = dense_K(60, band(60), a);
    CHECK(G.p.size() == 101);
    for (int v = 0; v < 100 && G.p.size() == 101; v++) {
      std::set<int> got(G.i.begin() + G.p[v], G.i.begin() + G.p[v + 1]), want;
      for (int u = 0; u < 100; u++) if (u != v && K[v][u]) want.insert(u);
      CHECK(got == want && (int)got.size() == G.p[v + 1] - G.p[v]);
    }
  }
  { /* the automatic rule: 257 is the first n with nlev > 256 */
    for (int n = 256; n <= 257; n++) {
      g_case = n == 256 ? "auto band 256" : "auto band 257";
      const Prob P = make_prob(n, band(n), Rows());
      SparseSym S, nat, nd;
      std::string why;
      CHECK(sparse_symbolic(P.pat(), false, -1, NO_LIMIT, S, why) == 0);
      CHECK(sparse_symbolic(P.pat(), false, 0, NO_LIMIT, nat, why) == 0);
      CHECK(sparse_symbolic(P.pat(), false, 1, NO_LIMIT, nd, why) == 0);
      CHECK(nat.nlev == n && !nat.dissected && nd.dissected);
      /* the rule's conditions hold for the dissected band: at least four times shallower, nnz <= 3 nnz_natural + n */
      CHECK((size_t)nd.nlev * 4 <= (size_t)nat.nlev && nd.Li.size() <= 3 * nat.Li.size() + (size_t)n);
      if (n == 257) {
        CHECK(S.dissected); CHECK(S.perm == nd.perm && S.Lp == nd.Lp && S.Li == nd.Li && S.nlev == nd.nlev);
        /* a dissected factor beyond max_nnz is not kept, and is no error: the natural one stands */
        SparseSym T;
        CHECK(nd.Li.size() > nat.Li.size());
        CHECK(sparse_symbolic(P.pat(), false, -1, nat.Li.size(), T, why) == 0 && why.empty());
        CHECK(!T.dissected && is_identity(T.perm) && T.Li == nat.Li);
      }
      else { CHECK(!S.dissected); CHECK(is_identity(S.perm) && S.Li == nat.Li && S.nlev == nat.nlev); }
      check_sym(dense_H(n, band(n), Rows()), S);
      check_plans(S, n);
    }
  }
  { /* a visitor that reports indices several times, the diagonal and the upper part included */
    g_case = "repeating visitor";
    const int n = 40;
    Edges e = band(n);
    for (int j = 0; j + 7 < n; j += 3) e.push_back(std::make_pair(j, j + 7));
    const Dense H = dense_H(n, e, Rows());
    auto cols = [&H, n](const int jo, auto &&visit) { for (int rep = 0; rep < 3; rep++) for (int i = n - 1; i >= 0; i--) if (H[i][jo]) { visit(i); visit(i); } };
    SparseSym S;
    std::string why;
    CHECK(sparse_analyze(n, cols, S, NO_LIMIT, why) == 0);
    check_sym(H, S);
    /* max_nnz one below the pattern's size */
    SparseSym T;
    const size_t nz = S.Li.size();
    CHECK(nz > 1);
    CHECK(sparse_analyze(n, cols, T, nz - 1, why) == 1);
    CHECK(why == "the sparse factor would hold more than " + std::to_string(nz - 1) + " entries");
    SparseSym U;
    why.clear();
    CHECK(sparse_analyze(n, cols, U, nz, why) == 0 && why.empty() && U.Li == S.Li);
    /* the same through sparse_symbolic, natural and dissected */
    const Prob P = make_prob(n, e, Rows());
    for (int ordering = 0; ordering <= 1; ordering++) {
      SparseSym A, B;
      CHECK(sparse_symbolic(P.pat(), false, ordering, NO_LIMIT, A, why) == 0);
      why.clear();
      CHECK(sparse_symbolic(P.pat(), false, ordering, A.Li.size() - 1, B, why) == 1);
      CHECK(why == "the sparse factor would hold more than " + std::to_string(A.Li.size() - 1) + " entries");
    }
  }
  { /* 200 random symmetric patterns, each with a random permutation preset in S.perm */
    g_case = "random";
    for (int it = 0; it < 200; it++) {
      const int n = 1 + (int)(rnd() % 60);
      const unsigned density = 1 + rnd() % 12; /* of 64 */
      Dense H((size_t)n, std::vector<char>((size_t)n, 0));
      for (int i = 0; i < n; i++) { H[i][i] = 1; for (int j = 0; j < i; j++) if (rnd() % 64 < density) H[i][j] = H[j][i] = 1; }
      SparseSym S;
      S.perm.resize((size_t)n);
      for (int j = 0; j < n; j++) S.perm[j] = j;
      for (int j = n - 1; j > 0; j--) std::swap(S.perm[j], S.perm[rnd() % (unsigned)(j + 1)]);
      const std::vector<int> preset = S.perm;
      auto cols = [&H, n](const int jo, auto &&visit) { for (int i = 0; i < n; i++) if (H[i][jo]) visit(i); };
      std::string why;
      CHECK(sparse_analyze(n, cols, S, NO_LIMIT, why) == 0);
      CHECK(S.perm == preset);
      check_sym(H, S);
      check_plans(S, n);
    }
  }
  printf("%d checks\n%d failures\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}

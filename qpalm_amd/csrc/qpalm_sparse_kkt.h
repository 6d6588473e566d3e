/*
 * qpalm_sparse_kkt.h -- the KKT path of newton_set_direction (src/newton.c:22-95) on a SPARSE L D L' of K (context option "sparse_kkt").
 *   qpalm_form_kkt / qpalm_reform_kkt + ladel_factorize*_with_diag      src/solver_interface.c:119-200, newton.c:32-45
 *   kkt_update_entering_constraints (ladel_row_add)                     src/solver_interface.c:202-218
 *   kkt_update_leaving_constraints  (ladel_row_del)                     src/solver_interface.c:220-236
 *   kkt_solve + iterative refinement                                    src/solver_interface.c:238-247, newton.c:55-90
 *
 * K = [[Q + I/gamma, A_a'], [A_a, -Sigma_a^{-1}]] of n + m rows, inactive constraints = unit rows, as P K P' = L D L' on the pattern of
 * K_full (every row of A present: qpalm_host_symbolic.h, sparse_adj_K), the pattern the reference's kkt_full gives LADEL.  The ordering is a nested
 * dissection of K's graph with the dense rows of A last (or the natural [x; y], "sparse_ordering" = 0).  D has mixed signs (K is
 * quasi-definite); nothing here divides by anything but a pivot.
 *  - Form + factorise: sp_factor<true> (qpalm_sparse.h), K assembled column by column inside the left-looking level-parallel factorisation.
 *  - Row addition of constraint k, column p of P K P' (a unit column before): Davis & Hager's bordering step on the fixed pattern (the sparse
 *    form of qpalm_kkt.h's).  Column p of K goes into a zero work vector; the forward solve L11 z = k12 runs over row p's pattern, columns
 *    ascending, each scattering its column into the vector -- below row p that accumulates k32 - L31 z (k32: the variables ordered after the
 *    constraint; zero under the natural order); row p of L = z_j / d_j, d22 = -1/sigma_k - sum z_j^2 / d_j, column p = (k32 - L31 z) / d22;
 *    then one rank-1 term -d22 l32 l32' on the trailing block, walked along the elimination-tree path from parent(p) (sp_path_walk).
 *  - Row deletion: w = sqrt|d_p| L(:, p), column and row p zeroed, d_p = 1, the rank-1 term + d_p l l' along the same path.
 *  - Solve: permute in, sp_solve, permute out; the refinement of newton.c:57-90 on top (kkt_refine, qpalm_kkt.h).
 * Policy (newton.c:32-53, as the dense path): refactorise on reset_newton or more changes than the threshold, else row operations; every row
 * operation counts in n_rank1.  One workgroup per QP; the row operations are wavefront 0's.  Included by qpalm_iter.h after qpalm_sparse.h.
 */
#ifndef QPALM_SPARSE_KKT_H
#define QPALM_SPARSE_KKT_H

/* row additions for enter[0 .. ne), then row deletions for leave[0 .. nl), on the sparse factor of K (nf = n + m rows) */
QPNI void spk_rows(const qpg_view &V, int b, const int nf, const SpArrays &S_, const int *enter, int ne, const int *leave, int nl) {
#if QP_SP_LOCAL
  const SpArrays S = S_;
#else
  const SpArrays &S = S_;
#endif
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int *Atp = V.Atp + (size_t)b * (V.m + 1);
  const double *Atx = V.Atx + (size_t)b * V.nnzA, *sigma_inv = V.sigma_inv + (size_t)b * V.m;
  int *state = V.kkt_state + (size_t)b * V.m;
  const int *Lp = QP_UNIFORM_PTR(S.Lp), *Li = QP_UNIFORM_PTR(S.Li), *Rp = QP_UNIFORM_PTR(S.Rp), *Rk = QP_UNIFORM_PTR(S.Rk), *Rpos = QP_UNIFORM_PTR(S.Rpos);
  const int *AtiP = QP_UNIFORM_PTR(S.AtiP), *first = QP_UNIFORM_PTR(S.first);
  double *Lx = QP_UNIFORM_PTR(S.Lx), *Dg = QP_UNIFORM_PTR(S.Dg);
  /* the work vector in LDS where nf doubles fit (as sp_updown), else wavefront 0's in HBM; zero on entry and again after every row */
  const bool in_lds = QP_SP_LDS_SOLVE && S.lds_cap && (size_t)nf * sizeof(double) <= (size_t)S.lds_bytes;
  auto rows = [&](auto w) QP_ALWAYS_INLINE {
    for (int c = 0; c < ne + nl; c++) {
      const bool add = c < ne;
      const int k = add ? enter[c] : leave[c - ne], p = first[k];
      const int e0 = Lp[p], e1 = Lp[p + 1];
      bool update; /* sign of the trailing rank-1 term: L33 D33 L33' + (update ? + : -) w w' */
      if (add) { /* ladel_row_add(LD, sym, n+k, kkt, n+k, -sigma_inv[k]) */
        for (int q = Atp[k] + lane; q < Atp[k + 1]; q += 64) w[AtiP[q]] = Atx[q]; /* column p of K off the diagonal: k12 and k32 */
        QP_WAVE_SYNC();
        double zz = 0.0; /* lane 0: sum z_j^2 / d_j, columns ascending */
        for (int r = Rp[p]; r < Rp[p + 1]; r++) {
          const int j = Rk[r], pos = Rpos[r], f0 = Lp[j], f1 = Lp[j + 1];
          const double zj = w[j], dj = Dg[j]; /* final: every column before j that reaches row j has been scattered */
          for (int e = f0 + lane; e < f1; e += 64) { const int i = Li[e]; if (i != p) w[i] -= Lx[e] * zj; }
          QP_WAVE_SYNC();
          if (lane == 0) { const double l = zj / dj; Lx[pos] = l; zz += l * zj; w[j] = 0.0; } /* row p of L */
          QP_WAVE_SYNC();
        }
        const double d22 = -sigma_inv[k] - __shfl(zz, 0);
        const double sq = QP_SQRT(qabs(d22));
        for (int e = e0 + lane; e < e1; e += 64) { /* l32 = (k32 - L31 z) / d22; its scaled copy is the rank-1 vector */
          const int i = Li[e];
          const double l = w[i] / d22;
          Lx[e] = l;
          w[i] = sq * l;
        }
        if (lane == 0) { Dg[p] = d22; state[k] = 1; }
        update = d22 < 0; /* - l32 d22 l32' */
      } else { /* ladel_row_del(LD, sym, n+k) */
        const double d = Dg[p];
        const double sq = QP_SQRT(qabs(d));
        for (int e = e0 + lane; e < e1; e += 64) { w[Li[e]] = sq * Lx[e]; Lx[e] = 0.0; }
        for (int r = Rp[p] + lane; r < Rp[p + 1]; r += 64) Lx[Rpos[r]] = 0.0;
        QP_WAVE_SYNC(); /* every lane has read d_p */
        if (lane == 0) { Dg[p] = 1.0; state[k] = 2; }
        update = d > 0; /* + l32 d l32' */
      }
      QP_WAVE_SYNC();
      sp_path_walk(Lp, Li, Lx, Dg, w, (e1 > e0) ? Li[e0] : -1, update); /* from parent(p): the rows below p all lie on its path */
    }
  };
  __syncthreads();
  if (in_lds) {
    double QP_LDS_AS *w = QP_LDS_ARG(double, S.lds);
    for (int i = threadIdx.x; i < nf; i += QP_T) w[i] = 0.0;
    __syncthreads();
    if (wid == 0) rows(w);
  } else {
    if (wid == 0) rows(S.wv);
  }
  __syncthreads();
}

/* The KKT branch on the sparse factor; action and flags as kkt_newton's (qpalm_kkt.h): 1 form + factorise, 2 row additions then deletions,
 * 3 form only (the state of every constraint from the active set), 4 factorise the K the states describe, 0 keep; QP_KKT_SOLVE, QP_KKT_REFINE. */
QPNI void spk_newton(const qpg_view *Vp, int b_, int slot_, double *Dg, IterShared *Ip, char *lds, int action_, int ne_, int nl_, int flags_) {
  const qpg_view &V = *Vp;
  IterShared &I = *Ip;
  const int b = QP_UNIFORM(b_), slot = QP_UNIFORM(slot_), action = QP_UNIFORM(action_), ne = QP_UNIFORM(ne_), nl = QP_UNIFORM(nl_), flags = QP_UNIFORM(flags_);
  const QpArrays a = qp_arrays(V, b);
  const qpg_settings &st = *V.settings;
  const int n = a.n, m = a.m, nf = n + m, tid = threadIdx.x, prox = qp_prox(st, I.s);
  const double gamma = I.s.gamma;
  const size_t sk = (size_t)V.n + V.m; /* batch strides */
  double *sol = V.kkt_sol + (size_t)b * sk, *rhs = V.kkt_rhs + (size_t)b * sk, *z = V.kkt_tmp + (size_t)b * sk;
  int *state = V.kkt_state + (size_t)b * V.m;
  const SpArrays S = sp_arrays(V, b, slot, Dg, lds);
  if (action == 1 || action == 3) {
    __syncthreads();
    for (int k = tid; k < m; k += QP_T) state[k] = a.active()[k] ? 1 : 0;
    __syncthreads();
  }
  if (action == 1 || action == 4) sp_factor<true>(V, b, nf, S, false, prox != 0, gamma, n);
  if (action == 2) {
    spk_rows(V, b, nf, S, a.enter(), ne, a.leave(), nl);
    if (tid == 0) I.s.n_rank1 += ne + nl;
  }
  __syncthreads();
  if (!(flags & QP_KKT_SOLVE)) return;
  for (int j = tid; j < nf; j += QP_T) sol[j] = (j < n) ? a.dphi()[j] * -1 : 0.0;
  sp_solve(nf, S, sol);
  for (int j = tid; j < n; j += QP_T) a.d()[j] = sol[j];
  if (!(flags & QP_KKT_REFINE)) { __syncthreads(); return; }
  auto solve_in_place = [&](double *v) QP_ALWAYS_INLINE { sp_solve(nf, S, v); };
  kkt_refine(V, a, b, I, gamma, prox, sol, rhs, z, solve_in_place);
}

#endif

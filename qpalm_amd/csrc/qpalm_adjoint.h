/*
 * qpalm_adjoint.h -- the adjoint of a solved QP: gradients of a loss l(x*, y*) with respect to q, bmin, bmax and the stored entries of Q and A
 * (qpg_batch_adjoint_device, include/qpalm_gfx950.h).  No reference counterpart.
 *
 * At a fixed active set J (each active row on its lower or its upper bound) the solution satisfies K [x; y_J] = [-q; b_J] with
 * K = [[Q, A_J'], [A_J, 0]], so for g = (dl/dx, dl/dy_J) the gradients follow from ONE solve K [u; w] = g:
 *   dl/dq = -u,  dl/db_i = w_i on the bound row i sits on,  dl/dA_ij = -(y_i u_j + w_i x_j),  dl/dQ_ij = -(u_i x_j + u_j x_i)  (-u_i x_i on the diagonal).
 * The engine works on the scaled problem (x~ = D^-1 x, y~ = c E^-1 y, Q~ = c D Q D, A~ = E A D): K~ [u~; w~] = [c D gx; E gy] with u = D u~,
 * w = E w~ / c -- the transformations of x and y (dev_store_solution).
 *
 * K~ is solved by iterative refinement.  The preconditioner is the regularised system the iteration factorises all the time,
 *   K_reg = [[Q~ + I / gamma, A~_J'], [A~_J, -Sigma_J^-1]]:   du = F^-1 (r1 + A~_J' Sigma_J r2),  dw = Sigma_J (A~_J du - r2),
 * F = Q~ + I / gamma + A~_J' Sigma_J A~_J = one form_schur + dev_factor (sp_factor) on J with the member's own sigma and gamma; a pass is three
 * SpMVs for the residual, one more and a triangular solve for du, one more for dw.  It stops with the correction of the first residual that has
 * ||r||inf <= 4 eps (||K~||inf ||z||inf + ||rhs||inf) (a backward-stable solve), or at the pass cap (flag 1).
 *
 * The penalty floor (qpg_adjoint_args.sens_floor, qpg_batch_set_sens_penalty): a pass contracts by about 1 / (1 + sigma lambda), so the
 * penalties a loose solve stops with make the refinement slow, and nothing in the linear solve needs them.  With a floor s > 0 the preconditioner uses
 * sigma'_i = max(sigma_i, s) on J -- in F (form_schur / sp_factor with BOOST: a row below the floor takes the factor s / sigma_i once, where its entry of
 * the column is read; At_sqrt_sigma itself, the reference's running product, is only read) and in the two places of a pass that multiply by Sigma.  K~,
 * the residual, the stopping rule and the outputs do not see it; the rule for J keeps the solve's sigma_inv (it is a statement about the stored solution).
 * A row with sigma_i >= s contributes the same terms in the same order: s = 0, or any s below every penalty, gives the same bits as no floor.
 *
 * The tangent (qpg_batch_tangent_device) is the same solve, K being symmetric, on the right-hand side of a direction of the data:
 *   r1 = -(dq + dQ x + dA' y),  r2_i = db_i - (dA x)_i on J,  K [dx; dy_J] = [r1; r2]  -- a mode of the same kernel (qpg_adjoint_args.tangent).
 * sens_setup (step 1: active set, scaled solution, ||K~||inf, the fresh factor) and sens_refine (step 2: the refinement on a given right-hand side and
 * the way back to the caller's scaling) are shared as one copy of the code; adj_rhs / tan_rhs and the outputs are what differs.
 *
 * The polish (qpg_batch_polish_device) is the same solve once more, on the residuals of the stored solution itself:
 *   r1 = -(q + Q x + A_J' y_J),  r2_i = b_i - (A x)_i on J,  K [dx; dy_J] = [r1; r2],  x^ = x + dx,  y^ = y + dy on J and 0 elsewhere
 * (qpg_adjoint_args.polish; pol_rhs / pol_finish).  pol_finish clips multipliers on the wrong side of their bound, measures the candidate's residuals
 * the way check_termination does with scaled_termination = 0, and takes the candidate iff neither residual got worse than max(old, the solve's eps).
 * Which vector holds what in that mode (all of them scratch of the kind described below):
 *   after sens_setup            xs = x~ (the stored x, scaled)   t[0, m) = A~ x~       u = w = 0
 *   inside pol_rhs              r2 = y~ (every row)   rhs2 = y~ masked by J   rhs1 = Q~ x~   r1 = A~' y~, then A~_J' y~_J
 *                               -> dua_old (rhs1, q~, r1 with every row's y) and pri_old (t) are reduced to scalars here, before anything is reused
 *   leaving pol_rhs             rhs1 = -(q~ + Q~ x~ + A~_J' y~_J)   rhs2 = b~_J - A~_J x~   (sens_refine reads them, overwrites xs, r1, r2, t)
 *   after sens_refine           u = dx   w = dy   (unscaled; xs = 0)
 *   inside pol_finish           u = x^   w = y^ (clipped)   xs = x^ scaled   r2 = y^ scaled   rhs1 = Q~ x^~   r1 = A~' y^~   t[0, m) = A~ x^~
 *   leaving pol_finish          xs = 0, as sens_refine leaves it
 * sol_x / sol_y are read by sens_setup, pol_rhs and pol_finish and written, if at all, by the last loop of pol_finish.
 *
 * At a recorded point (qpg_batch_adjoint_at_device / qpg_batch_tangent_at_device): K holds Q, A and J and neither q nor the bounds, and
 * x, y enter only tan_rhs and the dAx / dQx outputs, so a solve from any number of steps ago is differentiated from its x, y and J as long as the values
 * of Q and A are still its own.  qpg_adjoint_args.at_x / at_y replace sol_x / sol_y wherever dev_adjoint hands a point on, J is active_in, and the
 * member's status -- that of a later solve -- is not consulted.  k_get_active gives the J of the stored solutions on its own, by sens_setup's rule.
 *
 * Several directions per call (qpg_batch_adjoint_multi_device / qpg_batch_tangent_multi_device): sens_setup does not depend on the
 * right-hand side, so dev_adjoint runs it once per member and then, for each of qpg_adjoint_args.ndir directions in turn, the right-hand side,
 * sens_refine and the outputs on slice k of the per-direction arrays.  The arithmetic of a direction is that of the single call: slice k holds its bits.
 *
 * Scratch: vectors a finished solve leaves behind and the next one rebuilds before it reads them (d, temp_n, delta_x, dphi, z, temp_m, delta_y,
 * the line-search scratch, enter / leave) and the workgroup's factor slot.  The active flags form_schur / sp_factor read are saved and put back
 * (update_sigma of a later solve may read them before its first Newton step).  x, y, the stored solution, sigma, gamma, Qx / Ax products and
 * every scalar of the member stay as they are: the scalars are read into LDS and never written back.
 */
#ifndef QPALM_ADJOINT_H
#define QPALM_ADJOINT_H

QPD int adj_bad(double v) { return (qabs(v) <= 1.7976931348623157e308) ? 0 : 1; } /* NaN or infinite */

/* The vectors of a member the sensitivity solve works on (see "Scratch" above) */
struct SensVecs {
  double *u, *w, *xs, *rhs1, *r1, *rhs2, *r2, *t;
  int *sgn, *keep, *act;
};
QPD SensVecs sens_vecs(const QpArrays &a) {
  SensVecs v;
  v.u = a.delta_x(); v.w = a.temp_m(); v.xs = a.d(); v.rhs1 = a.dphi(); v.r1 = a.temp_n(); v.rhs2 = a.z(); v.r2 = a.delta_y(); v.t = a.ls_delta();
  v.sgn = a.enter(); v.keep = a.leave(); v.act = a.active();
  return v;
}

/* The rule for J on a solution: set_active_constraints (newton.c:122-131) at row i, with t = A~ x~ and y the unscaled multipliers; an equality row counts
 * as lower.  -1 lower, +1 upper, 0 inactive.  One copy for sens_setup and k_get_active: the two give the same bits. */
QPD int sens_active_row(const QpArrays &a, const double *t, const double *y, int i, int scal, double c) {
  double yv = y[i];
  if (scal) { yv = yv * a.Einv()[i]; yv *= c; }
  const double axys = t[i] + 1 * (yv * a.sigma_inv()[i]);
  const double lo = a.bmin()[i], hi = a.bmax()[i];
  return (lo == hi || axys <= lo) ? -1 : ((axys >= hi) ? 1 : 0);
}

/* ---- step 1 of a sensitivity solve (adjoint and tangent): the scaled solution xs, the active set (sgn; the flags form_schur / sp_factor read are saved
 * in keep), z = [u; w] = 0, and F = Q~ (+ I / gamma) + A~_J' Sigma_J A~_J factorised afresh: the slot may hold another member's factor, or this member's
 * for another set.  px / py: the point (the stored solution, or the caller's of a call "at" a recorded point, for which J is always given).  Returns
 * ||K~||inf (largest absolute row sum). ---- */
template <int RPT>
QPN double sens_setup(const qpg_view &V, const QpArrays &a, const SensVecs &v, const double *px, const double *py, const int64_t *active_in, int b, int slot,
                      IterShared &I, char *lds, const double sfloor) {
  constexpr bool SPARSE = (RPT == QPG_RPT_SPARSE);
  const qpg_settings &st = *V.settings;
  const int n = a.n, m = a.m, tid = threadIdx.x;
  const size_t om = (size_t)b * V.m;
  double *L = V.L + (size_t)slot * V.ld * V.nfac, *Dg = V.Dg + (size_t)slot * V.nfac;
  const int scal = I.s.has_scaling, prox = qp_prox(st, I.s);
  const double c = I.s.sc_c, gam = I.s.gamma;
  for (int j = tid; j < n; j += QP_T) {
    v.xs[j] = scal ? px[j] * a.Dinv()[j] : px[j];
    v.u[j] = 0.0;
  }
  __syncthreads();
  spmv_rows<8>(m, a.Atp(), a.Ati(), a.Atx(), (const double *)v.xs, [&](int r, double s) { v.t[r] = s; });
  __syncthreads();
  for (int i = tid; i < m; i += QP_T) {
    int sg;
    if (active_in) { const int64_t av = active_in[om + i]; sg = (av < 0) ? -1 : ((av > 0) ? 1 : 0); }
    else sg = sens_active_row(a, v.t, py, i, scal, c);
    v.sgn[i] = sg; v.keep[i] = v.act[i]; v.act[i] = (sg != 0) ? 1 : 0;
    v.w[i] = 0.0;
  }
  __syncthreads();
  double vm[1] = {0.0}, vs[1] = {0.0};
  for (int j = tid; j < n; j += QP_T) {
    double s = 0.0;
    for (int k = a.Qfp()[j]; k < a.Qfp()[j + 1]; k++) s += qabs(a.Qfx()[k]);
    for (int k = a.Ap()[j]; k < a.Ap()[j + 1]; k++) if (v.sgn[a.Ai()[k]]) s += qabs(a.Ax()[k]);
    vm[0] = qmax(vm[0], s);
  }
  for (int i = tid; i < m; i += QP_T) {
    if (!v.sgn[i]) continue;
    double s = 0.0;
    for (int k = a.Atp()[i]; k < a.Atp()[i + 1]; k++) s += qabs(a.Atx()[k]);
    vm[0] = qmax(vm[0], s);
  }
  block_reduce<1, 0>(I.S, vm, vs);
  if constexpr (SPARSE) {
    const SpArrays SP = sp_arrays(V, b, slot, Dg, lds);
    if (QP_CALL_BLOCK()) sp_factor<false, true>(V, b, n, SP, true, prox != 0, gam, 0, 0, -1, 0, 0, sfloor);
  } else {
    form_schur<true>(V, b, n, L, false, true, prox != 0, gam, I.S, lds, 0, 1, sfloor);
    dev_factor<RPT>(V, n, L, Dg, lds, I.s.ticks_dbg);
  }
  return vm[0];
}

/* ---- step 2: refinement on K~ z = [rhs1; rhs2], z = [u; w] (zero on entry), on the factor sens_setup left; then z back in the caller's scaling
 * (u = D u~, w = E w~ / c; zeros when flagged) and the flags of the active set back where the next solve expects them ---- */
template <int RPT>
QPN void sens_refine(const qpg_view &V, const QpArrays &a, const SensVecs &v, int b, int slot, IterShared &I, char *lds, double normK, int max_pass,
                     const double sfloor, int &flag, int &passes, double &ratio) {
  constexpr bool SPARSE = (RPT == QPG_RPT_SPARSE);
  const int n = a.n, m = a.m, tid = threadIdx.x;
  const int scal = I.s.has_scaling;
  double *L = V.L + (size_t)slot * V.ld * V.nfac, *Dg = V.Dg + (size_t)slot * V.nfac;
  double *u = v.u, *w = v.w, *xs = v.xs, *rhs1 = v.rhs1, *r1 = v.r1, *rhs2 = v.rhs2, *r2 = v.r2, *t = v.t;
  const int *sgn = v.sgn;
  double vm[2] = {0.0, 0.0}, vs[1] = {0.0};
  for (int j = tid; j < n; j += QP_T) vm[0] = qmax(vm[0], qabs(rhs1[j]));
  for (int i = tid; i < m; i += QP_T) if (sgn[i]) vm[0] = qmax(vm[0], qabs(rhs2[i]));
  block_reduce<1, 0>(I.S, vm, vs);
  const double rhsn = vm[0];
  for (int pass = 0;; pass++) {
    __syncthreads();
    spmv_rows<8>(n, a.Qfp(), a.Qfi(), a.Qfx(), (const double *)u, [&](int r, double s) { r1[r] = rhs1[r] - s; });
    spmv_rows<8>(m, a.Atp(), a.Ati(), a.Atx(), (const double *)u, [&](int r, double s) { r2[r] = sgn[r] ? rhs2[r] - s : 0.0; });
    __syncthreads();
    spmv_rows<16>(n, a.Ap(), a.Ai(), a.Ax(), (const double *)w, [&](int r, double s) { r1[r] = r1[r] - s; });
    __syncthreads();
    vm[0] = 0.0; vm[1] = 0.0; vs[0] = 0.0;
    for (int j = tid; j < n; j += QP_T) {
      vm[0] = qmax(vm[0], qabs(r1[j])); vm[1] = qmax(vm[1], qabs(u[j]));
      vs[0] += (double)(adj_bad(r1[j]) | adj_bad(u[j]));
    }
    for (int i = tid; i < m; i += QP_T) {
      vm[0] = qmax(vm[0], qabs(r2[i])); vm[1] = qmax(vm[1], qabs(w[i]));
      vs[0] += (double)(adj_bad(r2[i]) | adj_bad(w[i]));
    }
    block_reduce<2, 1>(I.S, vm, vs);
    const double den = normK * vm[1] + rhsn;
    /* (the same values in every lane: scalar branches) */
    const int bad = QP_UNIFORM((int)(vs[0] != 0.0)), conv = QP_UNIFORM((int)(vm[0] <= 4.0 * 2.220446049250313e-16 * den));
    passes = pass;
    ratio = bad ? -1.0 : ((den > 0.0) ? vm[0] / den : 0.0);
    if (bad) { flag = 1; break; }
    if (!conv && pass >= max_pass) { flag = 1; break; }
    if (vm[0] == 0.0) break;
    /* the correction this residual gives is applied in either case: the iteration converges linearly, so the iterate whose residual first meets the
     * bound sits AT the bound, and its correction is what takes the error down to the rounding level of the solve (`passes` counts it) */
    passes = pass + 1;
    for (int i = tid; i < m; i += QP_T) t[i] = sgn[i] ? qmax(a.sigma()[i], sfloor) * r2[i] : 0.0;
    __syncthreads();
    spmv_rows<16>(n, a.Ap(), a.Ai(), a.Ax(), (const double *)t, [&](int r, double s) { xs[r] = r1[r] + s; });
    __syncthreads();
    if constexpr (SPARSE) { if (QP_CALL_BLOCK()) sp_solve(n, sp_arrays(V, b, slot, Dg, lds), xs); }
    else { if (QP_CALL_BLOCK()) dense_solve(L, Dg, n, V.ld, xs, lds, V.lds_bytes); }
    __syncthreads();
    spmv_rows<8>(m, a.Atp(), a.Ati(), a.Atx(), (const double *)xs, [&](int r, double s) { if (sgn[r]) w[r] = w[r] + qmax(a.sigma()[r], sfloor) * (s - r2[r]); });
    for (int j = tid; j < n; j += QP_T) u[j] = u[j] + xs[j];
    if (conv) break;
  }
  __syncthreads();
  for (int j = tid; j < n; j += QP_T) { u[j] = (flag == 0) ? (scal ? a.D()[j] * u[j] : u[j]) : 0.0; xs[j] = 0.0; }
  for (int i = tid; i < m; i += QP_T) {
    double wv = w[i];
    if (scal) { wv = wv * I.s.sc_cinv; wv = wv * a.E()[i]; }
    w[i] = (flag == 0) ? wv : 0.0;
    v.act[i] = v.keep[i];
  }
  __syncthreads();
}

/* sum_k vals[pos(k)] * x[idx[k]] over the entries k in [ptr[r], ptr[r + 1]) of every row r with keep(r): G lanes per row, lane `sub` takes the entries
 * sub, sub + G, ... in order, then the xor tree -- a gather in a fixed order (no atomics: the result does not depend on arrival order).  pos(k): where
 * the caller's array holds entry k.  post(r, sum) consumes the result (sum = 0 for a row that is not kept). */
template <int G, class Pos, class Keep, class Post>
QPD void tan_gather_rows(int nrows, const int *__restrict__ ptr, const int *__restrict__ idx, const double *__restrict__ vals, const double *x,
                         Pos pos, Keep keep, Post post) {
  const int sub = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  for (int r0 = 0; r0 < nrows; r0 += QP_T / G) {
    const int r = r0 + grp;
    double acc = 0.0;
    if (r < nrows && keep(r))
      for (int k = ptr[r] + sub; k < ptr[r + 1]; k += G) acc = QP_FMA(vals[pos(k)], x[idx[k]], acc);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (r < nrows && sub == 0) post(r, acc);
  }
}

/* ---- the adjoint's right-hand side: [c D gx; E gy_J], of direction k (MULTI = false: the only one) ---- */
template <bool MULTI>
QPN void adj_rhs(const qpg_view &V, const QpArrays &a, const SensVecs &v, const qpg_adjoint_args &io, int b, int k, const IterShared &I) {
  const int n = a.n, m = a.m, tid = threadIdx.x, scal = I.s.has_scaling;
  const size_t on = (MULTI ? (size_t)k * (size_t)io.dir_n : 0) + (size_t)b * V.n, om = (MULTI ? (size_t)k * (size_t)io.dir_m : 0) + (size_t)b * V.m;
  const double c = I.s.sc_c;
  for (int j = tid; j < n; j += QP_T) {
    const double g = io.gx[on + j];
    double r = g;
    if (scal) { r = a.D()[j] * g; r *= c; }
    v.rhs1[j] = r;
  }
  for (int i = tid; i < m; i += QP_T) {
    const double g = (io.gy && v.sgn[i]) ? io.gy[om + i] : 0.0;
    v.rhs2[i] = scal ? a.E()[i] * g : g;
  }
  __syncthreads();
}

/* ---- the tangent's right-hand side: r1 = -(dq + dQ x + dA' y), r2_i = db_i - (dA x)_i on J, formed in unscaled space from the
 * point (x, y: the stored solution, or the caller's recorded one) and the caller's directions, then [c D r1; E r2].  y is that of every row.  dQx / dAx
 * are read where the caller put them (k_update_Q_A's maps): dA' y by the columns of A, dQ x by the rows of the full symmetric pattern (Qfperm: a stored lower entry stands for both
 * positions; upper entries of the caller are in no map), dA x by the rows of A' (Atperm) -- gathers, eight lanes per column / row.  kd: the direction
 * (slice kd of the five direction arrays; MULTI = false: the only one). ---- */
template <bool MULTI>
QPN void tan_rhs(const qpg_view &V, const QpArrays &a, const SensVecs &v, const qpg_adjoint_args &io, const double *x, const double *y, int b, int kd,
                 const IterShared &I) {
  const int n = a.n, m = a.m, scal = I.s.has_scaling;
  const size_t on = (MULTI ? (size_t)kd * (size_t)io.dir_n : 0) + (size_t)b * V.n, om = (MULTI ? (size_t)kd * (size_t)io.dir_m : 0) + (size_t)b * V.m;
  const double c = I.s.sc_c;
  const int sameA = io.same ? QP_UNIFORM(io.same[2 * b]) : 1, sameQ = io.same ? QP_UNIFORM(io.same[2 * b + 1]) : 1;
  const int32_t *mA = io.mapA ? io.mapA + (size_t)b * V.nnzA : nullptr, *mQ = io.mapQ ? io.mapQ + (size_t)b * V.nnzQ : nullptr;
  const double *dA = io.t_dAx ? io.t_dAx + ((MULTI ? (size_t)kd * (size_t)io.dir_A : 0) + (size_t)b * io.strideA) : nullptr;
  const double *dQ = io.t_dQx ? io.t_dQx + ((MULTI ? (size_t)kd * (size_t)io.dir_Q : 0) + (size_t)b * io.strideQ) : nullptr;
  const int *Atperm = a.Atperm(), *Qfperm = a.Qfperm();
  double *r1 = v.r1;
  auto all = [](int) { return true; };
  for (int j = threadIdx.x; j < n; j += QP_T) r1[j] = io.t_dq ? io.t_dq[on + j] : 0.0;
  __syncthreads();
  if (dQ) {
    tan_gather_rows<8>(n, a.Qfp(), a.Qfi(), dQ, x, [&](int k) { const int e = Qfperm[k]; return sameQ ? e : mQ[e]; }, all, [&](int r, double s) { r1[r] = r1[r] + s; });
    __syncthreads();
  }
  if (dA) {
    tan_gather_rows<8>(n, a.Ap(), a.Ai(), dA, y, [&](int k) { return sameA ? k : mA[k]; }, all, [&](int r, double s) { r1[r] = r1[r] + s; });
    __syncthreads();
  }
  for (int j = threadIdx.x; j < n; j += QP_T) {
    const double g = -r1[j];
    double r = g;
    if (scal) { r = a.D()[j] * g; r *= c; }
    v.rhs1[j] = r;
  }
  for (int i = threadIdx.x; i < m; i += QP_T) {
    const int sg = v.sgn[i];
    const double *db = (sg < 0) ? io.t_dbmin : io.t_dbmax;
    v.r2[i] = (sg && db) ? db[om + i] : 0.0; /* (inactive rows: nothing is read) */
  }
  __syncthreads();
  if (dA) {
    tan_gather_rows<8>(m, a.Atp(), a.Ati(), dA, x, [&](int k) { const int e = Atperm[k]; return sameA ? e : mA[e]; }, [&](int r) { return v.sgn[r] != 0; },
                       [&](int r, double s) { v.r2[r] = v.r2[r] - s; });
    __syncthreads();
  }
  for (int i = threadIdx.x; i < m; i += QP_T) { const double g = v.r2[i]; v.rhs2[i] = scal ? a.E()[i] * g : g; }
  __syncthreads();
}

/* the largest violation of a row's bounds (>= 0) and the row's value clipped to them: pri_res and z of compute_residuals at y = 0 */
QPD double pol_viol(double ax, double lo, double hi) { return qmax(qmax(lo - ax, ax - hi), 0.0); }
QPD double pol_clip(double ax, double lo, double hi) { return qmax(lo, qmin(ax, hi)); }

/* ---- the polish's right-hand side, in the engine's scaled variables: [-(q~ + Q~ x~ + A~_J' y~_J); b~_J - A~_J x~], from xs = x~ and
 * t = A~ x~ as sens_setup left them.  On the way the residuals of the stored solution (every row's y), unscaled as check_termination reports them:
 * pri_old = max_i viol(A x; bmin, bmax)_i, dua_old = ||Q x + q + A' y||inf. ---- */
QPN void pol_rhs(const qpg_view &V, const QpArrays &a, const SensVecs &v, IterShared &I, double &pri_old, double &dua_old) {
  const int n = a.n, m = a.m, tid = threadIdx.x, scal = I.s.has_scaling;
  const double c = I.s.sc_c;
  for (int i = tid; i < m; i += QP_T) {
    double yv = a.sol_y()[i];
    if (scal) { yv = yv * a.Einv()[i]; yv *= c; }
    v.r2[i] = yv; v.rhs2[i] = v.sgn[i] ? yv : 0.0;
  }
  __syncthreads();
  spmv_rows<8>(n, a.Qfp(), a.Qfi(), a.Qfx(), (const double *)v.xs, [&](int r, double s) { v.rhs1[r] = s; });
  spmv_rows<16>(n, a.Ap(), a.Ai(), a.Ax(), (const double *)v.r2, [&](int r, double s) { v.r1[r] = s; });
  __syncthreads();
  double vm[2] = {0.0, 0.0}, vs[1] = {0.0};
  for (int j = tid; j < n; j += QP_T) {
    double g = v.rhs1[j] + a.q()[j]; g = g + v.r1[j];
    vm[0] = qmax(vm[0], qabs(scal ? a.Dinv()[j] * g : g));
  }
  for (int i = tid; i < m; i += QP_T) {
    const double pr = pol_viol(v.t[i], a.bmin()[i], a.bmax()[i]);
    vm[1] = qmax(vm[1], scal ? a.Einv()[i] * pr : pr);
  }
  block_reduce<2, 0>(I.S, vm, vs); /* (its barriers: every read of r1 above is done before the next SpMV writes it) */
  dua_old = scal ? vm[0] * I.s.sc_cinv : vm[0]; pri_old = vm[1];
  spmv_rows<16>(n, a.Ap(), a.Ai(), a.Ax(), (const double *)v.rhs2, [&](int r, double s) { v.r1[r] = s; });
  __syncthreads();
  for (int j = tid; j < n; j += QP_T) { double g = v.rhs1[j] + a.q()[j]; g = g + v.r1[j]; v.rhs1[j] = -g; }
  for (int i = tid; i < m; i += QP_T) {
    const int sg = v.sgn[i];
    v.rhs2[i] = sg ? ((sg < 0) ? a.bmin()[i] : a.bmax()[i]) - v.t[i] : 0.0;
  }
  __syncthreads();
}

/* ---- the polish's candidate, verdict, outputs and store: u = dx, w = dy on entry (sens_refine; zeros when flagged).  flag: 0 accepted, 1 (unchanged, or
 * the candidate is not finite), 2 (unchanged), 3 formed and rejected.  Only an accepted candidate is written anywhere but into scratch. ---- */
QPN void pol_finish(const qpg_view &V, const QpArrays &a, const SensVecs &v, const qpg_adjoint_args &io, int b, IterShared &I, int &flag,
                    double pri_old, double dua_old) {
  const qpg_settings &st = *V.settings;
  const int n = a.n, m = a.m, tid = threadIdx.x, scal = I.s.has_scaling;
  const size_t on = (size_t)b * V.n, om = (size_t)b * V.m;
  double *u = v.u, *w = v.w, *xs = v.xs;
  double pri_new = pri_old, dua_new = dua_old;
  if (flag == 0) {
    for (int j = tid; j < n; j += QP_T) {
      const double xv = a.sol_x()[j] + u[j];
      u[j] = xv; xs[j] = scal ? xv * a.Dinv()[j] : xv;
    }
    for (int i = tid; i < m; i += QP_T) {
      const int sg = v.sgn[i];
      double yv = sg ? a.sol_y()[i] + w[i] : 0.0;
      /* the clip: a multiplier on the wrong side of its bound (y > 0 pushes on bmax, y < 0 on bmin); an equality row keeps either sign */
      if (sg && a.bmin()[i] != a.bmax()[i] && ((sg < 0) ? (yv > 0.0) : (yv < 0.0))) yv = 0.0;
      w[i] = yv;
      if (scal) { yv = yv * a.Einv()[i]; yv *= I.s.sc_c; }
      v.r2[i] = yv;
    }
    __syncthreads();
    spmv_rows<8>(n, a.Qfp(), a.Qfi(), a.Qfx(), (const double *)xs, [&](int r, double s) { v.rhs1[r] = s; });
    spmv_rows<8>(m, a.Atp(), a.Ati(), a.Atx(), (const double *)xs, [&](int r, double s) { v.t[r] = s; });
    spmv_rows<16>(n, a.Ap(), a.Ai(), a.Ax(), (const double *)v.r2, [&](int r, double s) { v.r1[r] = s; });
    __syncthreads();
    /* compute_residuals + check_termination at the candidate, unscaled (termination.c:61-129 with scaled_termination = 0) */
    double vm[4] = {0.0, 0.0, 0.0, 0.0}, vs[1] = {0.0};
    for (int j = tid; j < n; j += QP_T) {
      const double Qx = v.rhs1[j], qj = a.q()[j], Aty = v.r1[j], Dinv = scal ? a.Dinv()[j] : 1.0;
      double g = Qx + qj; g = g + Aty;
      vm[0] = qmax(vm[0], qabs(Dinv * g));
      vm[1] = qmax(vm[1], qmax(qabs(Dinv * Qx), qmax(qabs(Dinv * qj), qabs(Dinv * Aty))));
      vs[0] += (double)(adj_bad(g) | adj_bad(u[j]));
    }
    for (int i = tid; i < m; i += QP_T) {
      const double ax = v.t[i], lo = a.bmin()[i], hi = a.bmax()[i], Einv = scal ? a.Einv()[i] : 1.0;
      vm[2] = qmax(vm[2], Einv * pol_viol(ax, lo, hi));
      vm[3] = qmax(vm[3], qmax(qabs(Einv * ax), qabs(Einv * pol_clip(ax, lo, hi))));
      vs[0] += (double)(adj_bad(ax) | adj_bad(w[i]));
    }
    block_reduce<4, 1>(I.S, vm, vs);
    const double cinv = scal ? I.s.sc_cinv : 1.0;
    const double eps_pri = st.eps_abs + st.eps_rel * vm[3], eps_dua = st.eps_abs + st.eps_rel * (vm[1] * cinv);
    /* (the same values in every lane: scalar branches) */
    const int bad = QP_UNIFORM((int)(vs[0] != 0.0));
    const int take = QP_UNIFORM((int)(vm[2] <= qmax(pri_old, eps_pri) && vm[0] * cinv <= qmax(dua_old, eps_dua)));
    if (!bad) { pri_new = vm[2]; dua_new = vm[0] * cinv; }
    flag = bad ? 1 : (take ? 0 : 3);
  }
  /* ---- outputs; whole strides: entries beyond the member's own n / m are zeros.  Not accepted: the stored solution as it is ---- */
  const bool ok = (flag == 0);
  if (io.p_x) for (int j = tid; j < V.n; j += QP_T) io.p_x[on + j] = (j < n) ? (ok ? u[j] : a.sol_x()[j]) : 0.0;
  if (io.p_y) for (int i = tid; i < V.m; i += QP_T) io.p_y[om + i] = (i < m) ? (ok ? w[i] : a.sol_y()[i]) : 0.0;
  if (io.p_res && tid == 0) {
    double *o = io.p_res + (size_t)4 * b;
    o[0] = pri_old; o[1] = dua_old; o[2] = pri_new; o[3] = dua_new;
  }
  if (io.store && ok) {
    for (int j = tid; j < n; j += QP_T) a.sol_x()[j] = u[j];
    for (int i = tid; i < m; i += QP_T) a.sol_y()[i] = w[i];
  }
  if (flag != 2) for (int j = tid; j < n; j += QP_T) xs[j] = 0.0; /* (as sens_refine leaves it) */
  __syncthreads();
}

/* One member of k_adjoint: the adjoint, the tangent (io.tangent) or the polish (io.polish).  They differ in the right-hand side and in what they write.
 * MULTI = false (k_adjoint, the single calls): one direction and no distance between directions, known to the compiler -- the loop below and its
 * offsets fold away.  MULTI = true (k_adjoint_multi): io.ndir directions, io.dir_* apart. */
template <int RPT, bool MULTI>
QPN void dev_adjoint(const qpg_view &V, const qpg_adjoint_args &io, int b, int slot, IterShared &I, char *lds) {
  const QpArrays a = qp_arrays(V, b);
  const int n = a.n, m = a.m, tid = threadIdx.x;
  const size_t on = (size_t)b * V.n, om = (size_t)b * V.m;
  const int tangent = QP_UNIFORM(io.tangent), polish = QP_UNIFORM(io.polish);
  const double sfloor = io.sens_floor; /* the preconditioner's penalties: max(sigma_i, sfloor) on J (0: the solve's own) */
  __syncthreads();
  if (tid == 0) I.s = V.sc[b]; /* a copy: the factorisation's timers land in it and go nowhere */
  __syncthreads();
  /* the point: the member's stored solution, or the caller's recorded one (qpg_batch_*_at_device: the status is that of another solve and is not
   * consulted; J = active_in, which the host requires) */
  const bool at = (io.at_x != nullptr);
  const double *px = at ? io.at_x + on : a.sol_x(), *py = at ? io.at_y + om : a.sol_y();
  const int status = QP_UNIFORM(I.s.status);
  /* the member's own flag: 2 = not solved, 1 = a recorded point that is not finite; every direction of such a member gets it, and zeros */
  int mflag = (at || status == QPG_SOLVED || status == QPG_DUAL_TERMINATED) ? 0 : 2;
  double normK = 0.0, pri_old = 0.0, dua_old = 0.0;
  const SensVecs v = sens_vecs(a);
  double *u = v.u, *w = v.w;
  int *sgn = v.sgn;
  if (at) { /* a point that is not finite within the member's own n / m: flag 1 and zeros, nothing is solved; active_out is still the set given */
    double vs[1] = {0.0};
    for (int j = tid; j < n; j += QP_T) vs[0] += (double)adj_bad(px[j]);
    for (int i = tid; i < m; i += QP_T) vs[0] += (double)adj_bad(py[i]);
    block_reduce<0, 1>(I.S, vs, vs);
    if (QP_UNIFORM((int)(vs[0] != 0.0))) {
      mflag = 1;
      for (int i = tid; i < m; i += QP_T) { const int64_t av = io.active_in[om + i]; sgn[i] = (av < 0) ? -1 : ((av > 0) ? 1 : 0); }
      __syncthreads();
    }
  }
  if (mflag == 0) normK = sens_setup<RPT>(V, a, v, px, py, io.active_in, b, slot, I, lds, sfloor);
  /* ---- the directions, one after another on the factor sens_setup left.  Each starts where the single call's only one starts:
   * z = 0 (sens_setup for the first, the loop for the others), and every other vector of SensVecs is written before it is read -- r1 / r2 by the
   * right-hand side, xs, r1, r2, t by a pass of sens_refine.  sens_refine puts the saved active flags back after every direction; nothing from there
   * to the next direction's refinement reads them (adj_rhs, tan_rhs, the refinement and the two solves go by sgn and the factor). ---- */
  const int ndir = MULTI ? QP_UNIFORM(io.ndir) : 1;
  for (int kd = 0; kd < ndir; kd++) {
    const size_t dn = (MULTI ? (size_t)kd * (size_t)io.dir_n : 0) + on, dm = (MULTI ? (size_t)kd * (size_t)io.dir_m : 0) + om;
    const size_t db = (MULTI ? (size_t)kd * (size_t)io.dir_b : 0) + (size_t)b;
    int flag = mflag, passes = 0;
    double ratio = 0.0;
    if (mflag == 0) {
      if (kd > 0) {
        for (int j = tid; j < n; j += QP_T) u[j] = 0.0;
        for (int i = tid; i < m; i += QP_T) w[i] = 0.0;
        __syncthreads();
      }
      if (polish) pol_rhs(V, a, v, I, pri_old, dua_old);
      else if (tangent) tan_rhs<MULTI>(V, a, v, io, px, py, b, kd, I);
      else adj_rhs<MULTI>(V, a, v, io, b, kd, I);
      sens_refine<RPT>(V, a, v, b, slot, I, lds, normK, io.max_pass, sfloor, flag, passes, ratio);
    }
    if (polish) pol_finish(V, a, v, io, b, I, flag, pri_old, dua_old); /* (x, y, res and the store; the outputs below that a polish has are written there) */
    /* ---- outputs of the direction; whole strides: entries beyond the member's own n / m are zeros ---- */
    const bool ok = (flag == 0);
    if (tangent) {
      if (io.dx) for (int j = tid; j < V.n; j += QP_T) io.dx[dn + j] = (ok && j < n) ? u[j] : 0.0;
      if (io.dy) for (int i = tid; i < V.m; i += QP_T) io.dy[dm + i] = (ok && i < m && sgn[i]) ? w[i] : 0.0;
    } else if (io.dq) for (int j = tid; j < V.n; j += QP_T) io.dq[dn + j] = (ok && j < n) ? -u[j] : 0.0;
    for (int i = tid; i < V.m; i += QP_T) {
      const int sg = (flag != 2 && i < m) ? sgn[i] : 0;
      const double wv = (ok && i < m) ? w[i] : 0.0;
      if (io.dbmin) io.dbmin[dm + i] = (sg < 0) ? wv : 0.0;
      if (io.dbmax) io.dbmax[dm + i] = (sg > 0) ? wv : 0.0;
      if (io.active_out && kd == 0) io.active_out[om + i] = sg; /* (the set is the member's, not the direction's) */
    }
    if (tid == 0) {
      if (io.flag) io.flag[db] = flag;
      if (io.resid) io.resid[db] = ratio;
      if (io.passes) io.passes[db] = passes;
    }
    /* ---- the per-entry gradients, in the order qpg_batch_update_Q_A takes its values (k_update_Q_A's maps, the other way round); eight lanes per column ---- */
    if (io.dAx) {
      double *o = io.dAx + ((MULTI ? (size_t)kd * (size_t)io.dir_A : 0) + (size_t)b * io.strideA);
      for (int64_t k = tid; k < io.strideA; k += QP_T) o[k] = 0.0;
      __syncthreads();
      if (ok) {
        const int sameA = io.same ? QP_UNIFORM(io.same[2 * b]) : 1;
        const int32_t *mA = io.mapA ? io.mapA + (size_t)b * V.nnzA : nullptr;
        for (int j = tid >> 3; j < n; j += QP_T >> 3) {
          const double uj = u[j], xj = px[j];
          for (int k = a.Ap()[j] + (tid & 7); k < a.Ap()[j + 1]; k += 8) {
            const int i = a.Ai()[k];
            o[sameA ? k : mA[k]] = -(py[i] * uj + w[i] * xj);
          }
        }
      }
    }
    if (io.dQx) {
      double *o = io.dQx + ((MULTI ? (size_t)kd * (size_t)io.dir_Q : 0) + (size_t)b * io.strideQ);
      for (int64_t k = tid; k < io.strideQ; k += QP_T) o[k] = 0.0;
      __syncthreads();
      if (ok) {
        const int sameQ = io.same ? QP_UNIFORM(io.same[2 * b + 1]) : 1;
        const int32_t *mQ = io.mapQ ? io.mapQ + (size_t)b * V.nnzQ : nullptr;
        for (int j = tid >> 3; j < n; j += QP_T >> 3) {
          const double uj = u[j], xj = px[j];
          for (int k = a.Qp()[j] + (tid & 7); k < a.Qp()[j + 1]; k += 8) {
            const int i = a.Qi()[k]; /* i >= j: the stored entry stands for both symmetric positions */
            o[sameQ ? k : mQ[k]] = (i == j) ? -(uj * xj) : -(u[i] * xj + uj * px[i]);
          }
        }
      }
    }
    __syncthreads(); /* (u and w have been read: the next direction may zero them) */
  }
}

/* One workgroup per factor slot; the members come off the work queue (V.queue[0], zeroed by the host) as in k_solve, so B > slots works.
 * io.list: the members of a subset call, through the same queue (everything dev_adjoint touches is the member's own or the workgroup's slot).
 * RPT = QPG_RPT_SPARSE: the sparse factor (sp_factor / sp_solve); any other value: the dense panel.
 * k_adjoint: the single calls (one direction per member, the code the compiler made of it before there were several); k_adjoint_multi: io.ndir > 1. */
template <int RPT, bool MULTI>
QPD void adjoint_queue(const qpg_view &V, const qpg_adjoint_args &io, IterShared &I, char *lds) {
  while (true) {
    __syncthreads();
    if (threadIdx.x == 0) I.S.ibc[0] = atomicAdd(V.queue, 1);
    __syncthreads();
    int b = QP_UNIFORM(I.S.ibc[0]);
    if (b < V.B && io.list != nullptr) b = QP_UNIFORM(io.list[b]); /* a subset: the listed members, then B (k_select) */
    if (b >= V.B) break;
    dev_adjoint<RPT, MULTI>(V, io, b, blockIdx.x, I, lds);
  }
}
template <int RPT>
__global__ __launch_bounds__(QP_T) QP_OCCUPANCY void k_adjoint(qpg_view V, qpg_adjoint_args io) {
  __shared__ IterShared I;
  adjoint_queue<RPT, false>(V, io, I, QP_DYN_LDS());
}
template <int RPT>
__global__ __launch_bounds__(QP_T) QP_OCCUPANCY void k_adjoint_multi(qpg_view V, qpg_adjoint_args io) {
  __shared__ IterShared I;
  adjoint_queue<RPT, true>(V, io, I, QP_DYN_LDS());
}

/* qpg_batch_get_active_device: the active set of the stored solutions by the rule of sens_setup (sens_active_row on t = A~ x~), into the caller's [B][m]
 * array: -1 lower, +1 upper, 0 inactive; rows beyond a member's own m and every row of a member that is not SOLVED / DUAL_TERMINATED are 0.  One
 * workgroup per listed member (qp_listed).  Scratch: d and ls_delta, as in sens_setup; the active flags are not touched. */
__global__ __launch_bounds__(QP_T) void k_get_active(qpg_view V, int64_t *out, const int32_t *list) {
  for (int h = blockIdx.x, b; h < V.B && (b = qp_listed(list, h)) < V.B; h += gridDim.x) {
    const QpArrays a = qp_arrays(V, b);
    const int n = a.n, m = a.m, tid = threadIdx.x;
    const int status = QP_UNIFORM(V.sc[b].status), scal = QP_UNIFORM(V.sc[b].has_scaling);
    const double c = V.sc[b].sc_c;
    int64_t *o = out + (size_t)b * V.m;
    if (status != QPG_SOLVED && status != QPG_DUAL_TERMINATED) {
      for (int i = tid; i < V.m; i += QP_T) o[i] = 0;
      continue;
    }
    double *xs = a.d(), *t = a.ls_delta();
    for (int j = tid; j < n; j += QP_T) xs[j] = scal ? a.sol_x()[j] * a.Dinv()[j] : a.sol_x()[j];
    __syncthreads();
    spmv_rows<8>(m, a.Atp(), a.Ati(), a.Atx(), (const double *)xs, [&](int r, double s) { t[r] = s; });
    __syncthreads();
    for (int i = tid; i < V.m; i += QP_T) o[i] = (i < m) ? sens_active_row(a, t, a.sol_y(), i, scal, c) : 0;
  }
}

/* active_in ([B][m] of the batch's strides) may only hold -1, 0, 1 within a member's own rows: *bad = 1 otherwise */
__global__ __launch_bounds__(QP_T) void k_adjoint_check(qpg_view V, const int64_t *active_in, int *bad) {
  const size_t total = (size_t)V.B * V.m;
  for (size_t e = (size_t)blockIdx.x * QP_T + threadIdx.x; e < total; e += (size_t)gridDim.x * QP_T) {
    const int b = (int)(e / V.m), i = (int)(e % V.m);
    const int64_t v = active_in[e];
    if (i < (V.mq ? V.mq[b] : V.m) && (v < -1 || v > 1)) *bad = 1;
  }
}

#endif

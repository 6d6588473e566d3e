/*
 * qpalm_gfx950.h -- C ABI of the MI355X (gfx950) backend for the QPALM semismooth-Newton path.
 *
 * This is the drop-in boundary: plain C, `extern "C"`, caller-owned host buffers, int status codes,
 * no torch / C++ types.  It replaces what the reference reaches through its compile-time solver
 * backend (include/types.h:17-32 typedef block + include/solver_interface.h) and the API of
 * include/qpalm.h for a BATCH of independent QPs whose state lives in HBM.
 *
 * Reference interface replaced by each entry point (paths relative to Benny44/QPALM):
 *
 *   qpg_batch_create / qpg_batch_set_problem / qpg_batch_setup
 *        qpalm_setup                      include/qpalm.h:59-60,   src/qpalm.c:73-319
 *        (validate_data/validate_settings src/validate.c:18-221,  scale_data src/scaling.c:34-113)
 *   qpg_batch_warm_start                  qpalm_warm_start  include/qpalm.h:71-73, src/qpalm.c:322-399
 *   qpg_batch_solve / qpg_batch_iterate   qpalm_solve       include/qpalm.h:82,    src/qpalm.c:401-736
 *   qpg_batch_update_settings/bounds/q    qpalm_update_*    include/qpalm.h:95-126, src/qpalm.c:739-871
 *   qpg_batch_*_device, qpg_batch_step_device   the same calls on arrays in device memory (no reference counterpart: it runs where its data is)
 *   qpg_batch_destroy                     qpalm_cleanup     include/qpalm.h:133,   src/qpalm.c:874-1096
 *   qpg_mat_vec / qpg_mat_tpose_vec       mat_vec / mat_tpose_vec          include/solver_interface.h:33,47
 *   qpg_ldlchol / qpg_ldlchol_matrix      ldlchol                           include/solver_interface.h:172
 *   qpg_sparse_matvec                     mat_vec / mat_tpose_vec on a caller-owned matrix
 *   qpg_ldlcholQAtsigmaA                  ldlcholQAtsigmaA                  include/solver_interface.h:185
 *   qpg_ldlupdate_entering_constraints    ldlupdate_entering_constraints    include/solver_interface.h:196
 *   qpg_ldldowndate_leaving_constraints   ldldowndate_leaving_constraints   include/solver_interface.h:207
 *   qpg_ldlupdate_sigma_changed           ldlupdate_sigma_changed           include/solver_interface.h:218
 *   qpg_ldlsolveLD_neg_dphi               ldlsolveLD_neg_dphi               include/solver_interface.h:228
 *   qpg_exact_linesearch                  exact_linesearch                  include/linesearch.h, src/linesearch.c:14-120
 *   qpg_compute_residuals                 compute_residuals                 include/iteration.h,  src/iteration.c:24-48
 *   qpg_set_active_constraints            set_active_constraints + set_entering_leaving_constraints src/newton.c:122-149
 *
 * All functions return QPG_OK (0) or a negative error code; qpg_last_error() gives the message.
 * There is NO CPU fallback: without a usable gfx950 device every entry point fails.
 */
#ifndef QPALM_GFX950_H
#define QPALM_GFX950_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int64_t qpg_int;   /* == c_int  (CMakeLists.txt:53 -DDLONG, include/global_opts.h:31-39) */
typedef double  qpg_float; /* == c_float (include/global_opts.h:61) */

#define QPG_OK 0
#define QPG_ERR_NO_DEVICE (-1)
#define QPG_ERR_INVALID (-2)
#define QPG_ERR_ALLOC (-3)
#define QPG_ERR_RUNTIME (-4)
#define QPG_ERR_UNSUPPORTED (-5)

/* == QPALMSettings, include/types.h:119-150 (same field order; ABI witnessed by
 *    interfaces/python/qpalm.py:49-80) */
typedef struct {
  qpg_int   max_iter;
  qpg_int   inner_max_iter;
  qpg_float eps_abs;
  qpg_float eps_rel;
  qpg_float eps_abs_in;
  qpg_float eps_rel_in;
  qpg_float rho;
  qpg_float eps_prim_inf;
  qpg_float eps_dual_inf;
  qpg_float theta;
  qpg_float delta;
  qpg_float sigma_max;
  qpg_float sigma_init;
  qpg_int   proximal;
  qpg_float gamma_init;
  qpg_float gamma_upd;
  qpg_float gamma_max;
  qpg_int   scaling;
  qpg_int   nonconvex;
  qpg_int   verbose;
  qpg_int   print_iter;
  qpg_int   warm_start;
  qpg_int   reset_newton_iter;
  qpg_int   enable_dual_termination;
  qpg_float dual_objective_limit;
  qpg_float time_limit;
  qpg_int   ordering;
  qpg_int   factorization_method;
  qpg_int   max_rank_update;
  qpg_float max_rank_update_fraction;
} QPGSettings;

/* == QPALMInfo with PROFILING, include/types.h:76-95 */
typedef struct {
  qpg_int   iter;
  qpg_int   iter_out;
  char      status[32];
  qpg_int   status_val;
  qpg_float pri_res_norm;
  qpg_float dua_res_norm;
  qpg_float dua2_res_norm;
  qpg_float objective;
  qpg_float dual_objective;
  qpg_float setup_time;
  qpg_float solve_time;
  qpg_float run_time;
} QPGInfo;

/* device-side work counters of one QP (for the roofline accounting) */
typedef struct {
  qpg_int n_refactor, n_factor_Q, n_sweeps, n_rank1, n_solve, n_sigma_updates, n_boost_gamma;
  qpg_int nb_active, nb_enter, nb_leave, last_kind, last_fact;
  qpg_float gamma, tau, eta, beta, eps_pri, eps_dua, eps_dua_in, sc_c;
  qpg_float ms_total, ms_factor, ms_update, ms_solve, ms_linesearch;
  qpg_float ms_dbg[16]; /* update: 0 staging, 1 panel wave busy, 2 last trailing wave busy, 7 sweep phases (wall);
                           factor: 3 form, 4 panel gemm, 5 block, 6 panel solve;
                           solve: 8 forward block, 9 forward rows below, 10 backward dots, 11 backward block; 12 SpMV+residuals;
                           line search: 13 SpMVs, 14 breakpoints + compaction, 15 sort (the scan is the rest) */
  qpg_int sweep_entries;         /* entries of L the rank-update sweeps touched (each read and written once): sum of nnz(L[:, J0:]) */
  qpg_int factor_reread_entries; /* entries of L re-read by the panel updates of the factorisations (beyond the compulsory write) */
  qpg_float lobpcg_lambda;       /* nonconvex QPs: the eigenvalue bound of lobpcg (nonconvex.c:29-168); gamma_init = gamma_max = 1/|lambda| */
  qpg_int placement;             /* where the QP's last solve ran: (XCC, SE, SH, CU) key << 16 | arrival index of the workgroup on
                                    that CU << 8 | panel wavefront << 4 | SIMD of wavefront 0 (qp_place_panel_wave) */
  qpg_int lobpcg_iter, nonconvex; /* LOBPCG iterations; settings->nonconvex of THIS QP after set_settings_nonconvex (:171-183) */
  qpg_int n_fused_solve;         /* of n_solve: solves whose forward substitution was done by the last update sweep or by the factorisation before it (L read once, not twice) */
  qpg_int n_seq_columns;         /* columns of the update sweeps whose pivots the per-column guard re-summed as the reference's running pivot (a pivot shrank by 2^8 or more) */
  qpg_int n_sweep_columns;       /* ... out of this many columns of diagonal-block recurrences */
  qpg_int n_guard_refactor;      /* Newton steps redone with a fresh factorisation because the direction from an updated factor was not finite */
} QPGStats;

typedef struct qpg_ctx qpg_ctx;
typedef struct qpg_batch qpg_batch;

const char *qpg_last_error(void);
const char *qpg_backend_name(void); /* "gfx950-hip" for the shipped library */

void qpg_set_default_settings(QPGSettings *s);          /* src/qpalm.c:38-70 */
int  qpg_validate_settings(const QPGSettings *s);       /* 1 = valid, src/validate.c:43-221 */

int  qpg_ctx_create(int device, qpg_ctx **out);
void qpg_ctx_destroy(qpg_ctx *ctx);
/* Engine options (no reference counterpart; they change speed or placement, never what is computed):
 *   "max_slots"             resident factor panels = workgroups in flight (default 512)
 *   "lds_bytes"             dynamic LDS per 512-thread workgroup
 *   "update_rank_threshold" -1 = the reference's refactorise-or-update rule (newton.c:98-101), k >= 0: refactorise beyond k changed rows
 *   "small_workgroups"      1 = factors of at most 256 rows run on the 256-thread instance of the kernels (four workgroups per CU), and
 *                           batches of more than 2 max_slots QPs with factors of at most 192 rows on the 128-thread instance (seven per CU);
 *                           2 = the 128-thread instance wherever its 21.5 KB of LDS fit, 3 = never the 128-thread one, 0 = neither
 *   "narrow_rows"           1 = quarter-wavefront Schur assembly for short rows of A
 *   "ld_align"              leading dimension of the factor panels in doubles (16 = every column on a 128-byte line)
 *   "sweep_ranks"           16 (default) or 32 ranks per update sweep (32: the multi-pass sweep, bit-identical factors, slower)
 *   "kkt_compact"           1 = FACTORIZE_KKT factorises the variables + ACTIVE constraints only and spreads the factor out on demand
 *   "factor_fused_solve"    1 (default) = on the Schur path a factorisation that a Newton solve follows (ldlcholQAtsigmaA / ldlchol, then
 *                           ldlsolveLD_neg_dphi) carries the forward substitution of that solve: -dphi sits in LDS behind the factorisation's own
 *                           blocks, every finished block column is applied to it at once, and the solve streams L once instead of twice.  d is bit
 *                           for bit what the separate pass gives (same fma chain per entry); counted in n_fused_solve.  Where the vector does not
 *                           fit the LDS, in KKT mode, in coop mode and with the sparse factor the solve stays whole.  0 = never (A/B runs, tests).
 *   "place_panel_wave"      0 / 1 / 2: SIMD placement of the sweeps' panel wavefronts (0 = the hardware's own)
 *   "sequential_rank_sums"  how an update sweep sums a column's pivots.  -1 (default) = a prefix tree, and any column in which a pivot
 *                           shrinks by 2^8 or more inside the sweep is summed again as the reference's running pivot (per-column guard); the running
 *                           pivot in every column for QPs whose factor can get near-singular (nonconvex; Q without a positive diagonal: LPs).
 *                           1 = the running pivot everywhere (-5 % on the benchmark); 0 = the unguarded tree (A/B runs only: loses eight digits on a
 *                           downdate into a numerically singular matrix)
 *   "queue_order"           1 (default) = a launch of more QPs than resident slots starts the members in descending order of the kernel time of
 *                           their previous solve (the launch's tail is then made of short solves); 0 = index order.  Never changes a result.
 *   "sparse_factor", "sparse_ordering"   the sparse L D L' and its ordering (qpg_batch_sparse_info / qpg_batch_sparse_perm below)
 *   "sparse_kkt"            0 (default) = a batch created with factorization_method = FACTORIZE_KKT keeps the dense (n+m) x (n+m) panel (more than 8192
 *                           rows are refused); 1 = it keeps a sparse L D L' of K on the pattern of K_full (every row of A), ordered by nested
 *                           dissection with the dense rows of A last ("sparse_ordering" -1 / 1; 0 = the natural [x; y]), whatever its size, with
 *                           sparse row additions / deletions (ladel_row_add / ladel_row_del) and the reference's refactorise-or-update rule.
 *                           Fixed when the batch is created.  enable_dual_termination and nonconvex are refused (QPG_ERR_UNSUPPORTED)
 *   "sparse_gpw"            columns of a level a wavefront of the sparse factorisation takes at a time: 1, 2, 4 or 8 groups of 64 / gpw lanes (default 8,
 *                           halved while the work vectors of all resident factors would exceed 4 GB).  Never changes a result.
 *   "sparse_lds"            1 (default) = the sparse factorisation accumulates a column, the sparse solves keep the right-hand side and the path
 *                           updates their work vector in LDS where they fit; 0 = the forms on vectors in HBM (same iterates bit for bit: A/B and
 *                           tests); >= 2 = LDS only for columns of at most that many entries (tests)
 *   "sparse_coop"           0 (default) = the factor operations of a sparse QP run on the QP's own workgroup; 1 = a batch that keeps the sparse
 *                           Schur factor, has at most "coop_max_batch" members and B <= "max_slots" runs its factorisations and Newton solves
 *                           (what the reference hands to CHOLMOD's factorize and solve, solver_interface.c:319-370, 505-519) on up to
 *                           "coop_workgroups" workgroups: the levels of the elimination tree become a chain of launches
 *                           (qpg_batch_sparse_coop_info below), replayed as graphs under "coop_graphs".  Every other batch -- "sparse_kkt",
 *                           larger batches, dense factors -- runs as with 0.  Path updates stay on the QP's workgroup.  Read by
 *                           qpg_batch_setup.  Same iterates bit for bit; "coop" does not switch this on, and nothing does by itself.
 *   "coop", "coop_workgroups", "coop_updates", "coop_rank_threshold"   one large QP on many workgroups
 * Environment: QPALM_HOST_THREADS = host threads of qpg_batch_set_problems (default: hardware threads, at most 24). */
int  qpg_ctx_set_option(qpg_ctx *ctx, const char *name, qpg_int value);

/* A batch = B QPs of dimensions up to (n, m) (equal for all members with qpg_batch_set_problem, smaller ones through
 * qpg_batch_set_problem_sized).  nnzA_max / nnzQ_max bound the entries of any member. */
int  qpg_batch_create(qpg_ctx *ctx, qpg_int B, qpg_int n, qpg_int m, qpg_int nnzA_max, qpg_int nnzQ_max,
                      const QPGSettings *settings, qpg_batch **out);
/* CSC, 64-bit indices as in cholmod_sparse; Q symmetric, only entries with row >= col are read
 * (stype = -1, B6).  Data is copied -- converted straight into the batch's host slab (huge pages, laid out as it is uploaded);
 * qpg_batch_create also starts the allocation of the batch's device memory on a thread of its own, qpg_batch_setup joins it. */
int  qpg_batch_set_problem(qpg_batch *bt, qpg_int idx, const qpg_int *Qp, const qpg_int *Qi, const qpg_float *Qx,
                           const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax, const qpg_float *q,
                           qpg_float c, const qpg_float *bmin, const qpg_float *bmax);
/* A member smaller than the batch (n <= batch n, m <= batch m): size-bucketed batches, e.g. the Maros-Meszaros QPS set
 * streamed through interfaces/qps (BASELINE.json config 4).  The member keeps its own dimensions on the device; results
 * come back in the batch's [B][n] / [B][m] arrays, entries beyond the member's n / m are zero. */
int  qpg_batch_set_problem_sized(qpg_batch *bt, qpg_int idx, qpg_int n, qpg_int m, const qpg_int *Qp, const qpg_int *Qi,
                                 const qpg_float *Qx, const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax,
                                 const qpg_float *q, qpg_float c, const qpg_float *bmin, const qpg_float *bmax);
/* qpg_batch_set_problem_sized for members first .. first + count - 1 in ONE call (entry k of every array = member first + k; n / m
 * NULL: every member has the batch's dimensions; c NULL: zero constants): the per-QP host work of qpalm_setup -- deep copies,
 * sorted CSC, the A' pattern (src/qpalm.c:128-144, iteration.c:81) -- runs on host threads (QPALM_HOST_THREADS; default: at most 24).  No reference counterpart (the reference sets up one QP per call). */
int  qpg_batch_set_problems(qpg_batch *bt, qpg_int first, qpg_int count, const qpg_int *n, const qpg_int *m,
                            const qpg_int *const *Qp, const qpg_int *const *Qi, const qpg_float *const *Qx,
                            const qpg_int *const *Ap, const qpg_int *const *Ai, const qpg_float *const *Ax,
                            const qpg_float *const *q, const qpg_float *c, const qpg_float *const *bmin, const qpg_float *const *bmax);
int  qpg_batch_setup(qpg_batch *bt);                               /* upload (one DMA per array from the host slab) + Ruiz scaling on device */
int  qpg_batch_warm_start(qpg_batch *bt, const qpg_float *x, const qpg_float *y); /* [B][n], [B][m] or NULL */
int  qpg_batch_warm_start_last(qpg_batch *bt);                     /* qpalm_warm_start(work, last x, last y) of every QP, from HBM (no host copy) */
int  qpg_batch_solve(qpg_batch *bt);                               /* run every QP to termination */
int  qpg_batch_iterate(qpg_batch *bt, qpg_int k);                  /* at most k more loop iterations each */
int  qpg_batch_begin_solve(qpg_batch *bt);                         /* start of a qpalm_solve driven by qpg_batch_iterate: finished QPs start over */
int  qpg_batch_last_solve_ms(qpg_batch *bt, float *ms);            /* HIP-event time of the last solve/iterate launch */
int  qpg_batch_num_unfinished(qpg_batch *bt, qpg_int *count);
/* how the batch runs: concurrent workgroups (= resident factor panels), threads per workgroup (512, or 256 for QPs whose
 * factor has at most 256 rows -- four workgroups per CU instead of two), dynamic LDS per workgroup.  No reference
 * counterpart (the reference runs one QP on one core); used by bench.py's per-phase bandwidth figures. */
int  qpg_batch_launch_shape(qpg_batch *bt, qpg_int *workgroups, qpg_int *threads, qpg_int *lds_bytes);
/* The sparse L D L' (round 5): replaces what solver_interface.c:319-370, 523-541 hands to cholmod_analyze / cholmod_factorize for
 * factors that are sparse or have more than 8192 rows (context option "sparse_factor": -1 automatic for > 8192 rows, 1 always,
 * 0 never; Schur path; dual termination keeps a second value array per slot for LD_Q, the factor of Q alone on the same pattern).  nnzL: entries of the member's strict lower triangle; device_bytes: the block that holds
 * the symbolic arrays of all members and the values of all resident factors.  QPG_ERR_UNSUPPORTED on a batch with dense factors.
 * Where its policy is not the reference's: rows that enter or leave the active set, and rows whose penalty changed
 * (ldlupdate_sigma_changed, solver_interface.c:443-503), are rank-1 updates along their elimination-tree paths only while
 * 2 x changed rows x tree height < n; beyond that the factor is rebuilt (on a chain-like tree -- a band under the natural ordering --
 * a path is the whole matrix).  QPGStats.n_refactor / n_rank1 then differ from the reference's split; the matrices factorised do not.
 * KKT mode under "sparse_kkt" = 1: the sparse L D L' of K (n + m rows); the refactorise-or-update rule is the reference's (newton.c:32-53) and
 * n_rank1 counts row additions + deletions as on the dense KKT panel. */
int  qpg_batch_sparse_info(qpg_batch *bt, qpg_int idx, qpg_int *nnzL, qpg_int *device_bytes);
/* The ordering of member idx's sparse factor, P H P' = L D L': perm[new] = old (n entries; KKT mode under "sparse_kkt": P K P', n + m entries
 * in the [x; y] numbering, nested dissection unless "sparse_ordering" = 0), and the height of its elimination tree.
 * The reference configures CHOLMOD_NATURAL (solver_interface.c:530-540: identity); context option "sparse_ordering" = 1 orders by
 * nested dissection instead, -1 (default) does so where the natural tree is deep (a band: one column per level) and dissection makes it
 * at least four times shallower -- the factorisation and the solves run at the latency of the tree's height.  Changes rounding, not
 * what is computed. */
int  qpg_batch_sparse_perm(qpg_batch *bt, qpg_int idx, qpg_int *perm, qpg_int *levels);
/* Member idx's sparse factor as it stands, in the factor's own numbering (qpg_batch_sparse_perm maps it to the caller's): Lp = column pointers
 * (nf + 1 entries; nf = n, or n + m in KKT mode under "sparse_kkt"), Li / Lx = row indices (ascending within a column) and values of the strict
 * lower part (nnzL of qpg_batch_sparse_info entries each; the pattern is that of ALL rows of A, so entries may be zero), D = the nf pivots.  Any
 * output may be NULL.  For tests and diagnostics (the sparse counterpart of qpg_batch_get_factor, which stays refused on a sparse batch): the
 * index arrays are copied back from the device.  QPG_ERR_UNSUPPORTED on a batch with dense factors and when B > max_slots (a slot then holds
 * whichever QP ran last). */
int  qpg_batch_get_sparse_factor(qpg_batch *bt, qpg_int idx, qpg_int *Lp, qpg_int *Li, qpg_float *Lx, qpg_float *D);
/* The launch plan of member idx under the context option "sparse_coop" = 1, made by qpg_batch_setup from the level sets of the member's
 * elimination tree (patterns only: qpg_batch_update_Q_A leaves it valid): launches per factorisation, launches per Newton solve (permutation in,
 * forward levels, D, backward levels, permutation out) and the largest grid among them.  Consecutive levels that one workgroup finishes in one
 * round (64 columns of the factorisation at the default "sparse_gpw", 512 rows of a solve) share ONE launch on one workgroup -- a band under the
 * natural ordering is one launch per phase --, a wider level is a launch of its own on min(G, ceil(width / round)) workgroups; G = "coop_workgroups"
 * (at most 1024 / B), fewer while the zeroed work vectors of those workgroups and of the resident slots together would exceed 4 GB (G = 1: one
 * launch per phase).  All three are 0 when the batch runs on one
 * workgroup per QP; QPG_ERR_UNSUPPORTED on a batch with dense factors. */
int  qpg_batch_sparse_coop_info(qpg_batch *bt, qpg_int idx, qpg_int *factor_launches, qpg_int *solve_launches, qpg_int *max_grid);
int  qpg_batch_update_settings(qpg_batch *bt, const QPGSettings *s);
int  qpg_batch_update_bounds(qpg_batch *bt, const qpg_float *bmin, const qpg_float *bmax); /* [B][m] or NULL */
int  qpg_batch_update_q(qpg_batch *bt, const qpg_float *q);                              /* [B][n] */
/* qpalm_update_Q_A for every member: new values of Q and A on the sparsity patterns the batch was set up with.  Entry k of member b is the new value of
 * the k-th entry its caller passed to qpg_batch_set_problem* (the caller's own order: duplicates and upper-triangle entries of Q included; positions
 * past the member's own count are ignored).  Afterwards the batch is, bit for bit, what qpg_batch_setup would leave for the same patterns with the new
 * values, the latest accepted raw q / bmin / bmax, the same c and the current settings -- without the host-side conversion, the symbolic analysis of the
 * sparse factors or a new arena.  The stored solutions survive (qpg_batch_warm_start_last works next); an unfinished solve ends; every status goes back to
 * unsolved and the counters of QPGStats restart.  QPG_ERR_INVALID before qpg_batch_setup or on a NULL array. */
int  qpg_batch_update_Q_A(qpg_batch *bt, const qpg_float *Qx, const qpg_float *Ax);          /* host arrays [B][nnzQ_max], [B][nnzA_max] */
int  qpg_batch_update_Q_A_device(qpg_batch *bt, const qpg_float *dQx, const qpg_float *dAx); /* the same layout, already in device memory (see qpg_batch_device_ptr) */
/* ---- the per-step calls on arrays in DEVICE memory (of the context's device): the receding-horizon loop without the host.
 * Each of the first five is its host form with the copy taken away: the same layout ([B][n] / [B][m] float64, contiguous; [B] qpg_int), the same
 * state, validation (bmin <= bmax per member; a refused member keeps its bounds and reads QPG_ERROR until the next solve) and error codes
 * (QPG_ERR_INVALID before qpg_batch_setup, on a NULL d_q, and with "Lower bound greater than upper bound").  Entries beyond a sized member's own
 * n / m are ignored on input and zero on output.  Input arrays are only read; kernels of the batch's own instance move the data.
 * Ordering: synchronous.  The caller guarantees that whatever produced the input arrays has finished; when a call returns the inputs have been
 * read and the outputs are complete and visible to every stream.
 * The latest accepted raw q / bounds, which qpg_batch_update_Q_A needs, are kept in a device-side record of B (n + 2 m) doubles (allocated by the
 * first of these updates); host and device forms may be mixed in any order. */
int  qpg_batch_update_bounds_device(qpg_batch *bt, const qpg_float *d_bmin, const qpg_float *d_bmax); /* either may be NULL */
int  qpg_batch_update_q_device(qpg_batch *bt, const qpg_float *d_q);
int  qpg_batch_warm_start_device(qpg_batch *bt, const qpg_float *d_x, const qpg_float *d_y);          /* either may be NULL */
int  qpg_batch_get_solution_device(qpg_batch *bt, qpg_float *d_x, qpg_float *d_y);                    /* either may be NULL */
int  qpg_batch_get_status_device(qpg_batch *bt, qpg_int *d_status_val, qpg_int *d_iter);              /* [B] each, either may be NULL */
/* One whole step: update_bounds -> update_q -> warm start -> qpg_batch_solve -> get_solution -> get_status on the arrays below, all in device
 * memory.  Returns QPG_ERR_INVALID at the end, after every member has been solved, if the bounds of any member were refused (that member
 * solves on its old bounds). */
typedef struct {
  const qpg_float *bmin, *bmax, *q;      /* NULL = unchanged */
  const qpg_float *warm_x, *warm_y;      /* used when warm == 2 (either may be NULL, not both) */
  qpg_int          warm;                 /* 0 none, 1 = qpg_batch_warm_start_last, 2 = warm_x / warm_y */
  qpg_float       *x, *y;                /* out, NULL = not wanted */
  qpg_int         *status_val, *iter;    /* out [B], NULL = not wanted */
  qpg_int         *rejected;             /* out [B], 1 = this member's bounds were refused (bmin > bmax), NULL = not wanted */
} QPGDeviceStep;
int  qpg_batch_step_device(qpg_batch *bt, const QPGDeviceStep *io);
/* The adjoint of the solved batch: gradients of a loss l(x*, y*) through the stored solutions, one launch, no second batch.
 * Per member, with J = its active rows (each on its lower or its upper bound) and K = [[Q, A_J'], [A_J, 0]]: K [u; w] = [gx; gy_J] is solved by
 * iterative refinement on a fresh factor of the member's regularised Schur complement, then
 *   dq = -u;  dbmin_i = w_i on lower-active rows, dbmax_i = w_i on upper-active rows, 0 elsewhere;
 *   dAx_k = -(y_i u_j + w_i x_j) for the k-th entry (i, j) the caller passed to qpg_batch_set_problem* (w_i = 0 outside J);
 *   dQx_k = -(u_i x_j + u_j x_i) for a strictly lower entry, -u_i x_i for a diagonal one (a lower entry stands for both symmetric positions; upper
 *   entries, which the engine ignores, and the padding up to nnzQ_max / nnzA_max get 0) -- the layout qpg_batch_update_Q_A takes.
 * active_in = NULL: J by the engine's own test on the stored solution in scaled space (A x + y / sigma <= bmin: lower, >= bmax: upper; a row with
 * bmin = bmax always, as lower); else -1 = lower, +1 = upper, 0 = inactive.  flag: 0 done; 1 the pass cap (200) was reached or the solve gave a
 * non-finite value (qpg_batch_set_sens_penalty: a penalty floor for the preconditioner, which takes the cap away after loose solves); 2 the member's
 * status is not SOLVED / DUAL_TERMINATED.  With flag 1 or 2 every output of the member is zero.  resid = the last
 * ||r||inf / (||K||inf ||z||inf + ||rhs||inf) in the engine's scaling (-1: non-finite), passes = corrections applied.  Entries beyond a sized member's
 * own n / m are zero.  Synchronous, like the calls above; all arrays in device memory; inputs are only read.  The call may overwrite the factor slots
 * and scratch vectors a finished solve leaves (the next solve rebuilds them); the iterates, stored solutions, penalties, statuses and counters stay.
 * QPG_ERR_INVALID before qpg_batch_setup, while a solve is in progress (qpg_batch_iterate left a member unfinished), with gx = NULL and for an
 * active_in entry outside {-1, 0, 1}; QPG_ERR_UNSUPPORTED for FACTORIZE_KKT batches, coop mode and nonconvex settings. */
typedef struct {
  const qpg_float *gx;        /* [B][n] dl/dx, required */
  const qpg_float *gy;        /* [B][m] dl/dy or NULL (rows outside J are ignored: y_i = 0 there) */
  const qpg_int   *active_in; /* [B][m] or NULL */
  qpg_float       *dq;        /* out [B][n] */
  qpg_float       *dbmin, *dbmax; /* out [B][m] */
  qpg_float       *dQx, *dAx; /* out [B][nnzQ_max], [B][nnzA_max] */
  qpg_int         *active_out; /* out [B][m]: the set used */
  qpg_int         *flag;      /* out [B] */
  qpg_float       *resid;     /* out [B] */
  qpg_int         *passes;    /* out [B] */
} QPGDeviceAdjoint;
int  qpg_batch_adjoint_device(qpg_batch *bt, const QPGDeviceAdjoint *io);
/* The tangent of the solved batch: how the stored solutions move when q, the bounds and the stored entries of Q and A move along ONE direction
 * (DESIGN.md section 13).  Per member, with (x, y) its stored solution and J, K as for the adjoint above (the same rule for J and its sides, the
 * same active_in; an equality row counts as lower, so only dbmin is read there):
 *   r1 = -(dq + dQ x + dA' y)     (y: the stored y of EVERY row),      r2_i = db_i - (dA x)_i for i in J, db_i = dbmin_i on a lower-active row,
 *   dbmax_i on an upper-active one;      K [dx; dy_J] = [r1; r2],  dy_i = 0 outside J.
 * dQx / dAx are read in the layout qpg_batch_update_Q_A takes and the adjoint writes: entry k belongs to the k-th entry the caller passed to
 * qpg_batch_set_problem*; a stored lower entry of Q stands for both symmetric positions, upper entries and the padding up to nnzQ_max / nnzA_max are
 * ignored.  On inactive rows dbmin, dbmax and (dA x)_i are not read.  A NULL direction array is a zero one (the same bits as an array of zeros).
 * K is symmetric, so this is the adjoint's solve on another right-hand side: the same fresh factor (and penalty floor), refinement, stopping rule, pass cap (200), flag /
 * resid / passes, and <gx, dx> + <gy, dy> = <adjoint outputs of (gx, gy), direction> up to the rounding of the two solves.  With flag 1 or 2 dx and
 * dy of the member are zero.  Entries beyond a sized member's own n / m are ignored on input and zero on output.  Synchronous; all arrays in device
 * memory; inputs are only read; one deterministic launch (no floating-point atomics: two calls on the same state return the same bits).  The call
 * may overwrite what the adjoint may overwrite and leaves everything else: solve -> tangent -> step is bit for bit solve -> step.
 * QPG_ERR_INVALID before qpg_batch_setup, while a solve is in progress, for an active_in entry outside {-1, 0, 1} and when all five direction
 * arrays are NULL; QPG_ERR_UNSUPPORTED for FACTORIZE_KKT batches, coop mode and nonconvex settings. */
typedef struct {
  const qpg_float *dq;            /* [B][n] or NULL = zero */
  const qpg_float *dbmin, *dbmax; /* [B][m] or NULL = zero */
  const qpg_float *dQx, *dAx;     /* [B][nnzQ_max], [B][nnzA_max] or NULL = zero */
  const qpg_int   *active_in;     /* [B][m] or NULL */
  qpg_float       *dx, *dy;       /* out [B][n], [B][m]; either may be NULL */
  qpg_int         *active_out;    /* out [B][m]: the set used */
  qpg_int         *flag;          /* out [B] */
  qpg_float       *resid;         /* out [B] */
  qpg_int         *passes;        /* out [B] */
} QPGDeviceTangent;
int  qpg_batch_tangent_device(qpg_batch *bt, const QPGDeviceTangent *io);
/* The polish of the solved batch: the exact solution at the final active set.  Per member, with (x, y) its stored solution and
 * J, K as for the adjoint above (the same rule for J and its sides, the same active_in; a row with bmin = bmax always counts as lower):
 *   K [dx; dy_J] = [-(q + Q x + A_J' y_J); b_J - A_J x],  b_i = bmin_i on a lower-active row, bmax_i on an upper-active one    (y masked by J),
 *   candidate x^ = x + dx,  y^_i = y_i + dy_i on J and 0 elsewhere; then, on a row of J with bmin < bmax, a multiplier on the wrong side of its bound
 *   (y^_i > 0 on a lower-active row, y^_i < 0 on an upper-active one) is set to zero.
 * The solve is the adjoint's: the same fresh factor (and penalty floor, qpg_batch_set_sens_penalty), refinement from zero, stopping rule, pass cap (200), resid and passes.  The verdict is taken in
 * unscaled space with the measures of the solver's own termination test: pri(x) = max_i max(bmin_i - (A x)_i, (A x)_i - bmax_i, 0),
 * dua(x, y) = ||Q x + q + A' y||inf, eps_pri = eps_abs + eps_rel max(||A x^||inf, ||clip(A x^, bmin, bmax)||inf), eps_dua = eps_abs + eps_rel
 * max(||Q x^||inf, ||q||inf, ||A' y^||inf) with the batch's current settings; the clipped candidate is accepted iff
 *   pri(x^) <= max(pri(x), eps_pri)  and  dua(x^, y^) <= max(dua(x, y), eps_dua)
 * -- each residual is no worse than before, or still passes the termination test (a wrong active set shows up as a residual and is rejected).
 * x, y: the candidate where accepted, the stored solution bit for bit otherwise (never zeros).  res: pri_old, dua_old, pri_new, dua_new of the member
 * (old: the stored solution with every row's y; new: the clipped candidate; new repeats old with flag 1, and all four are 0 with flag 2, for which
 * nothing is computed).  flag: 0 accepted; 1 the pass cap was reached or a value was not finite; 2 the member's status is not SOLVED /
 * DUAL_TERMINATED; 3 a candidate was formed and rejected.  active_out, resid, passes: as for the adjoint.
 * store != 0: the accepted candidates replace the members' stored solutions -- what qpg_batch_get_solution*, the adjoint, the tangent and
 * qpg_batch_warm_start_last read.  Nothing else of a member changes: iterates, penalties, statuses, counters and QPGInfo stay and still describe the
 * SOLVE (its residual norms and objective are those of the point the solve stopped at).  With store = 0 the call leaves exactly the state the adjoint
 * leaves: solve -> polish -> step is bit for bit solve -> step.  Synchronous; all arrays in device memory; one deterministic launch (no floating-point
 * atomics: two calls on the same state return the same bits).
 * QPG_ERR_INVALID before qpg_batch_setup, while a solve is in progress, for an active_in entry outside {-1, 0, 1} and when x, y and res are all NULL
 * and store is 0; QPG_ERR_UNSUPPORTED for FACTORIZE_KKT batches, coop mode and nonconvex settings. */
typedef struct {
  const qpg_int   *active_in;     /* [B][m] or NULL */
  qpg_int          store;         /* != 0: accepted candidates become the stored solutions */
  qpg_float       *x, *y;         /* out [B][n], [B][m]; either may be NULL */
  qpg_float       *res;           /* out [B][4]: pri_old, dua_old, pri_new, dua_new; or NULL */
  qpg_int         *active_out;    /* out [B][m]: the set used */
  qpg_int         *flag;          /* out [B] */
  qpg_float       *resid;         /* out [B] */
  qpg_int         *passes;        /* out [B] */
} QPGDevicePolish;
int  qpg_batch_polish_device(qpg_batch *bt, const QPGDevicePolish *io);
/* The penalty floor of the three calls above and of their subset forms.  Their refinement is preconditioned with the factor of
 * Q + I / gamma + A_J' Sigma_J A_J and contracts by about 1 / (1 + sigma lambda) per pass, so the penalties a loose solve stops with make it slow
 * (the pass cap, flag 1).  With a floor s > 0 the preconditioner -- the fresh factor and the two places of a pass that multiply by Sigma -- uses
 * sigma'_i = max(sigma_i, s) on the rows of J.  The system solved, its residual, the stopping rule, the pass cap, resid, passes and the flags are the
 * same, so a converged member is as accurate as before; the rule for J keeps the solve's own sigma; the member's penalties and everything else of its
 * state stay bit for bit (solve -> call -> step is solve -> step with any floor).  A row with sigma_i >= s enters as before: s = 0 (the default), or
 * any s below every penalty, gives the bits of a batch that never set one.  Per batch; allowed before and after qpg_batch_setup; kept across
 * qpg_batch_setup, the updates, the settings and the solves; applies to every later call.  Stored without effect on batches for which the three calls
 * are refused.  QPG_ERR_INVALID (value unchanged) for a NULL batch, a negative value, a NaN or an infinity. */
int  qpg_batch_set_sens_penalty(qpg_batch *bt, qpg_float sigma_floor);
int  qpg_batch_get_sens_penalty(qpg_batch *bt, qpg_float *out);
/* ---- the four calls above on a SUBSET of the members.  d_select: [B] qpg_int in device memory, 1 = the member takes part,
 * 0 = it does not; NULL = every member, and the call is its counterpart above.  n_selected (host, may be NULL): how many took part.
 * A member that is not selected is untouched: nothing is read from its rows of the input arrays (a bmin > bmax there is no error), nothing is written
 * to its rows of the output arrays (they keep what the caller's arrays held), and nothing of its state moves -- iterates, stored solution, q, bounds,
 * penalties, scaling, status, QPGInfo, QPGStats, the record of its raw q / bounds, its error mark.  For a selected member every array reads and
 * writes what the full call reads and writes, bit for bit: members are independent, and the selected ones run the same kernels, handed out through
 * the work queue (always, whatever B and the option "queue_order") in the order of the full call's queue among themselves.  Nothing selected: nothing
 * is launched but the selection, QPG_OK.  One read of three words per call brings back the count.
 * QPG_ERR_INVALID, before anything has changed: before qpg_batch_setup; an entry of d_select other than 0 or 1; any member (selected or not) in a
 * solve that qpg_batch_iterate left unfinished.  QPG_ERR_UNSUPPORTED: coop and sparse coop mode; B > 131072.  Everything else as for the
 * counterpart, its own refusals first. */
/* The step for the selected members, in every factor mode of the one-workgroup solve.  A selected member whose bounds are refused keeps them and solves
 * on them; QPG_ERR_INVALID at the end.  rejected: written for selected members only. */
int  qpg_batch_step_subset_device(qpg_batch *bt, const QPGDeviceStep *io, const qpg_int *d_select, qpg_int *n_selected);
/* Gradients of the selected members (the rows of the others, flag included, are not written). */
int  qpg_batch_adjoint_subset_device(qpg_batch *bt, const QPGDeviceAdjoint *io, const qpg_int *d_select, qpg_int *n_selected);
/* Tangents of the selected members. */
int  qpg_batch_tangent_subset_device(qpg_batch *bt, const QPGDeviceTangent *io, const qpg_int *d_select, qpg_int *n_selected);
/* The polish of the selected members; with store, accepted candidates of selected members replace their stored solutions. */
int  qpg_batch_polish_subset_device(qpg_batch *bt, const QPGDevicePolish *io, const qpg_int *d_select, qpg_int *n_selected);
/* ---- the active set on its own, and the adjoint and the tangent at a RECORDED point.
 * The active set of the stored solutions by the rule the adjoint applies with active_in = NULL: d_active [B][m] in device memory, -1 lower, +1 upper,
 * 0 inactive; rows beyond a sized member's own m are 0 and a member whose status is not SOLVED / DUAL_TERMINATED gets all zeros.  Bit for bit the
 * active_out of qpg_batch_adjoint_device on the same state.  It may overwrite two of the scratch vectors the adjoint may overwrite and nothing else.
 * The subset form writes the rows of selected members only (d_select, n_selected: as above).  QPG_ERR_INVALID before qpg_batch_setup, while a solve is
 * in progress and for d_active = NULL; QPG_ERR_UNSUPPORTED for FACTORIZE_KKT batches, coop mode and nonconvex settings. */
int  qpg_batch_get_active_device(qpg_batch *bt, qpg_int *d_active /* [B][m] */);
int  qpg_batch_get_active_subset_device(qpg_batch *bt, qpg_int *d_active, const qpg_int *d_select, qpg_int *n_selected);
/* A recorded point: the solution (x, y) of some earlier solve of this batch and its active set (qpg_batch_get_active_device right after that solve, or
 * the active_out of a sensitivity call made then).  The system K [u; w] = rhs the adjoint and the tangent solve holds Q, A and the active set; it
 * holds neither q nor the bounds, and x, y enter only the tangent's right-hand side and the adjoint's dAx / dQx.  So the two calls below are
 * qpg_batch_adjoint_subset_device / qpg_batch_tangent_subset_device with (x, y) := at->x, at->y and J := at->active wherever those read the stored
 * solution: the same system, refinement, stopping rule, pass cap, flag 0 / 1, resid, passes; active_out = at->active (signs).  d_select = NULL: every
 * member.  The members' current statuses are not consulted (flag 2 does not occur): exclude members through d_select.  The preconditioner uses the
 * members' current penalties and gamma and the penalty floor, as always.  Entries of at->x / at->y beyond a sized member's own n / m are not read; a
 * member with a non-finite entry within them gets flag 1 and zeros, its neighbours are unaffected.  State: as for the adjoint -- the call neither
 * reads nor moves the stored solutions, and solve -> call -> step is bit for bit solve -> step.  There is no polish at a point (it needs q and the bounds).
 * VALIDITY: the values of Q and A (and with them the scaling) must be those of the solve that produced the point -- no qpg_batch_update_Q_A* and no
 * new setup in between.  q, the bounds, the penalties, warm starts and any number of later solves may differ.  The engine cannot verify this; the
 * Python layer does (QpalmBatch.matrix_epoch).
 * QPG_ERR_INVALID: as for the counterpart, and for at = NULL, a NULL field of it, io->active_in != NULL (one source for J) and an entry of
 * at->active outside {-1, 0, 1}; QPG_ERR_UNSUPPORTED as for the counterpart. */
typedef struct {
  const qpg_float *x;       /* [B][n] */
  const qpg_float *y;       /* [B][m] */
  const qpg_int   *active;  /* [B][m]: -1 lower, +1 upper, 0 inactive */
} QPGDevicePoint;
int  qpg_batch_adjoint_at_device(qpg_batch *bt, const QPGDeviceAdjoint *io, const QPGDevicePoint *at, const qpg_int *d_select, qpg_int *n_selected);
int  qpg_batch_tangent_at_device(qpg_batch *bt, const QPGDeviceTangent *io, const QPGDevicePoint *at, const qpg_int *d_select, qpg_int *n_selected);
/* ---- K directions per call: the adjoint for K pairs (gx, gy) and the tangent for K directions of the data, in one call.  What
 * does not depend on the direction is done once per call or per member -- the check for a solve in progress, the check of active_in, the selection, the
 * launch, the active set, ||K||inf and the fresh factor -- and a member's K right-hand sides are then refined one after another on that factor.
 * Layout: every per-direction array is K consecutive blocks of the single call's array, direction-major, so slice k IS a single call's array:
 *   gx, dq (both calls), dx                  [K][B][n]
 *   gy, dbmin, dbmax (both calls), dy        [K][B][m]
 *   dQx / dAx (both calls)                   [K][B][nnzQ_max] / [K][B][nnzA_max]
 *   flag, resid, passes                      [K][B]
 *   active_in, active_out, at->x, at->y, at->active, d_select      as in the single calls, shared by all directions (active_out is written once)
 * A NULL direction array is zero in every direction.  at = NULL: the stored solutions (as qpg_batch_*_subset_device); otherwise the recorded point (as
 * qpg_batch_*_at_device).  d_select = NULL: every member.  n_selected as in the subset forms.
 * CONTRACT: slice k of every output is bit for bit what the corresponding single call (qpg_batch_*_device, *_subset_device or *_at_device) returns for
 * slice k of the inputs on the same state, with the same active_in / at / d_select and the same penalty floor.  flag, resid and passes are per
 * direction: a direction that reaches the pass cap or is not finite gets flag 1 and zeros in ITS slice only.  A member that is not SOLVED /
 * DUAL_TERMINATED (flag 2), or whose recorded point is not finite (flag 1), gets that flag and zeros in all K slices.  A member that is not selected
 * has none of its rows written in any slice.  State: as for the single calls -- solve -> multi call -> step is bit for bit solve -> step.  The polish has
 * no K form.
 * QPG_ERR_INVALID: K < 1, and whatever the single call refuses, checked once per call (for the tangent: all five direction arrays NULL; for the
 * adjoint: gx = NULL); QPG_ERR_UNSUPPORTED: exactly the single calls' refusals. */
int  qpg_batch_adjoint_multi_device(qpg_batch *bt, const QPGDeviceAdjoint *io, qpg_int K, const QPGDevicePoint *at, const qpg_int *d_select, qpg_int *n_selected);
int  qpg_batch_tangent_multi_device(qpg_batch *bt, const QPGDeviceTangent *io, qpg_int K, const QPGDevicePoint *at, const qpg_int *d_select, qpg_int *n_selected);
int  qpg_batch_get_info(qpg_batch *bt, qpg_int idx, QPGInfo *out);
int  qpg_batch_get_stats(qpg_batch *bt, qpg_int idx, QPGStats *out);
int  qpg_batch_get_info_all(qpg_batch *bt, QPGInfo *out /* [B] */);   /* QPALMInfo of every QP (what the multi-GPU gather sends) */
int  qpg_batch_get_stats_all(qpg_batch *bt, QPGStats *out /* [B] */);
int  qpg_batch_get_solution(qpg_batch *bt, qpg_float *x, qpg_float *y);                  /* [B][n], [B][m] */
int  qpg_batch_get_vector(qpg_batch *bt, const char *name, qpg_int idx, qpg_float *out, qpg_int len);
int  qpg_batch_set_vector(qpg_batch *bt, const char *name, qpg_int idx, const qpg_float *in, qpg_int len);
int  qpg_batch_get_ivector(qpg_batch *bt, const char *name, qpg_int idx, qpg_int *out, qpg_int len);
int  qpg_batch_set_ivector(qpg_batch *bt, const char *name, qpg_int idx, const qpg_int *in, qpg_int len);
int  qpg_batch_set_scalar(qpg_batch *bt, const char *name, qpg_int idx, qpg_float v);   /* "gamma", ... */
int  qpg_batch_get_factor(qpg_batch *bt, qpg_int idx, qpg_float *L_colmajor, qpg_float *D, qpg_int n);
void qpg_batch_destroy(qpg_batch *bt);
/* raw device pointers (for harnesses that keep data resident, e.g. torch tensors via from_dlpack) */
int  qpg_batch_device_ptr(qpg_batch *bt, const char *name, void **ptr, size_t *bytes);
int  qpg_batch_sync(qpg_batch *bt);

/* ---- solver_interface.h surface, acting on QP `idx` of the batch (device-resident state) ---- */
int qpg_mat_vec(qpg_batch *bt, qpg_int idx, int which /* 'A' or 'Q' */, const qpg_float *x, qpg_float *y);
int qpg_mat_tpose_vec(qpg_batch *bt, qpg_int idx, int which, const qpg_float *x, qpg_float *y);
int qpg_ldlchol(qpg_batch *bt, qpg_int idx);               /* factor Q (+ I/gamma if proximal) */
/* ldlchol(M, work, c) for an arbitrary symmetric M given as CSC (lower triangle read), solver_interface.h:172 */
int qpg_ldlchol_matrix(qpg_batch *bt, qpg_int idx, qpg_int n, const qpg_int *Mp, const qpg_int *Mi, const qpg_float *Mx);
/* mat_vec / mat_tpose_vec for a caller-owned CSC matrix (stype 0, or -1/+1 = symmetric, one triangle stored) */
int qpg_sparse_matvec(qpg_ctx *ctx, qpg_int nrow, qpg_int ncol, const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax,
                      int stype, int transpose, const qpg_float *x, qpg_float *y);
int qpg_ldlcholQAtsigmaA(qpg_batch *bt, qpg_int idx);
int qpg_ldlupdate_entering_constraints(qpg_batch *bt, qpg_int idx);
int qpg_ldldowndate_leaving_constraints(qpg_batch *bt, qpg_int idx);
int qpg_ldlupdate_sigma_changed(qpg_batch *bt, qpg_int idx);
int qpg_ldlsolveLD_neg_dphi(qpg_batch *bt, qpg_int idx);
int qpg_compute_residuals(qpg_batch *bt, qpg_int idx);
int qpg_set_active_constraints(qpg_batch *bt, qpg_int idx);
int qpg_exact_linesearch(qpg_batch *bt, qpg_int idx, qpg_float *tau);
/* On a batch in coop mode (context option "coop": one large QP on many workgroups; Schur mode, dense factor) the six factor operations above --
 * qpg_ldlchol, qpg_ldlcholQAtsigmaA, the three updates (unless "coop_updates" = 0) and qpg_ldlsolveLD_neg_dphi -- run on the grid kernels, through
 * the launch chains a solve in coop mode uses; every other operation, and every other batch, runs on the QP's own workgroup.  `count`: how many
 * single operations of this batch have run on the grid since it was created (0 on a batch that is not in coop mode). */
int qpg_batch_coop_op_chains(qpg_batch *bt, qpg_int *count);
/* ---- the KKT operations of solver_interface.h (batches created with factorization_method = FACTORIZE_KKT; QPG_ERR_UNSUPPORTED
 * otherwise).  State as in the reference: active_constraints, enter / leave lists with nb_enter / nb_leave, sigma_inv, gamma,
 * dphi; the (n+m) x (n+m) panel and sol_kkt / rhs_kkt live on the device ("L", "Dfac", "sol_kkt", "kkt_state").  With the context option
 * "sparse_kkt" = 1 the same five operations work on the sparse L D L' of K: qpg_kkt_form then records every constraint's state from the active
 * set (kkt_state 1 / 0) and qpg_kkt_factorize assembles K from those states inside the sparse factorisation. ---- */
/* qpalm_form_kkt / qpalm_reform_kkt (solver_interface.h:82,89; solver_interface.c:119-200): K = [[Q + I/gamma, A_a'], [A_a, -Sigma_a^-1]]
 * for the current active set into the slot (lower triangle; inactive constraints = unit diagonal), not factorised */
int qpg_kkt_form(qpg_batch *bt, qpg_int idx);
/* what newton.c:36,44 calls LADEL for after (re)forming: LDL' of the matrix in the slot, natural order (ladel_factorize_*_with_diag) */
int qpg_kkt_factorize(qpg_batch *bt, qpg_int idx);
/* kkt_update_entering_constraints (solver_interface.h:97; .c:202-218): ladel_row_add for enter[0 .. nb_enter) */
int qpg_kkt_update_entering_constraints(qpg_batch *bt, qpg_int idx);
/* kkt_update_leaving_constraints (solver_interface.h:106; .c:220-236): ladel_row_del for leave[0 .. nb_leave) */
int qpg_kkt_update_leaving_constraints(qpg_batch *bt, qpg_int idx);
/* kkt_solve (solver_interface.h:126; .c:238-247): sol_kkt = K^-1 [-dphi; 0], d = sol_kkt[0 .. n) (no iterative refinement: that is newton.c's) */
int qpg_kkt_solve(qpg_batch *bt, qpg_int idx);
/* batched LDL^T solve of the current factors with right-hand side dphi (the kernel the metric's
 * "HBM GB/s on LDL" refers to): every QP of the batch, `reps` times, for benchmarking. */
int qpg_batch_ldlsolve_all(qpg_batch *bt, qpg_int reps, float *ms_per_rep);
/* diagnostic (tools/sweep_probe.py): every resident workgroup factorises Q + I/gamma and applies `reps` times a rank-`nranks`
 * update + the matching downdate (rows 0 .. nranks-1 of A), i.e. the sweeps of solver_interface.c:407-441 alone under full-chip
 * contention; the sweep's phase timers are left in QPGStats.ms_dbg, *ms = duration of the launch */
int qpg_batch_sweep_probe(qpg_batch *bt, qpg_int reps, qpg_int nranks, float *ms);
/* attainable HBM bandwidth of this device, measured with a plain copy kernel (best of `reps` copies of `bytes` bytes;
 * read + write counted): the yardstick quoted next to the 8 TB/s spec figure */
int qpg_ctx_hbm_copy_gbs(qpg_ctx *ctx, size_t bytes, qpg_int reps, float *gbs);
int qpg_ctx_hbm_read_gbs(qpg_ctx *ctx, size_t bytes, qpg_int reps, float *gbs); /* read-only stream (the LDL' solve only reads L) */
/* page-locked (DMA-able) host memory for the arrays handed over every step (bounds in, solutions out); zero-filled.
 * The reference has no counterpart: it runs where its data is. */
int qpg_host_alloc(qpg_ctx *ctx, size_t bytes, void **out);
int qpg_host_free(qpg_ctx *ctx, void *p);

#ifdef __cplusplus
}
#endif
#endif

/*
 * qpalm_capi.inc -- host side of the C ABI (include/qpalm_gfx950.h).  Included by
 * qpalm_gfx950.hip (the shipped HIP build) and by tests/emu/qpalm_emu.cpp (kernel-source emulation,
 * test-only); both define the RT_* runtime macros first.
 *
 * Host work is what the reference's host does around the path: validation (src/validate.c) and data copies / format conversion
 * (qpalm_setup's deep copies, src/qpalm.c:128-144; the A' pattern that cholmod_transpose builds in iteration.c:81), both in
 * qpalm_host_convert.h; the symbolic analysis of the sparse factors (what cholmod_analyze does; with the nested dissection and the launch
 * plans of sparse coop mode in qpalm_host_symbolic.h); and, here, the batch's memory and launching kernels.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <string>
#include <vector>
#include <map>

#include "../../include/qpalm_gfx950.h"
#include "qpalm_host_convert.h"
#include "qpalm_host_symbolic.h"

/* The HIP build holds two instances of the kernels (namespaces qp512 / qp256, see qpalm_gfx950.hip); the emulation build
 * (tests) holds one, in the global namespace.  BT_LAUNCH picks the instance of a batch. */
#ifdef QP_TWO_INSTANCES
#define QP_INST(ns, kern) ns::kern
#else
#define QP_INST(ns, kern) kern
#define QP_T_SMALL QP_T
#define QP_LDS_SMALL 38912
#define QP_T_TINY QP_T
#define QP_LDS_TINY 22016
#define QP_TINY_PER_CU 7
#endif
#define BT_LAUNCH(bt, kern, grid, shmem, ...)                                                              \
  do {                                                                                                      \
    if ((bt)->small == 2) RT_LAUNCH(QP_INST(qp128, kern), grid, QP_T_TINY, shmem, __VA_ARGS__);             \
    else if ((bt)->small) RT_LAUNCH(QP_INST(qp256, kern), grid, QP_T_SMALL, shmem, __VA_ARGS__);            \
    else RT_LAUNCH(QP_INST(qp512, kern), grid, QP_T, shmem, __VA_ARGS__);                                   \
  } while (0)
#define BT_TIMED_LAUNCH(ms, bt, kern, grid, shmem, ...)                                                    \
  do {                                                                                                      \
    if ((bt)->small == 2) RT_TIMED_LAUNCH(ms, QP_INST(qp128, kern), grid, QP_T_TINY, shmem, __VA_ARGS__);   \
    else if ((bt)->small) RT_TIMED_LAUNCH(ms, QP_INST(qp256, kern), grid, QP_T_SMALL, shmem, __VA_ARGS__);  \
    else RT_TIMED_LAUNCH(ms, QP_INST(qp512, kern), grid, QP_T, shmem, __VA_ARGS__);                         \
  } while (0)
/* A kernel template over the dense factor's rows per thread (rpt): up to 4 the update sweep keeps its running vectors in registers (kern<1|2|4>), larger
 * factors use the large-factor sweep with the vectors in HBM (kern<0>).  BT_RPT(rpt, R, BT_LAUNCH(bt, kern<R>, grid, ...)) launches that instance. */
#define BT_RPT(rpt, R, ...)                                                                                 \
  do {                                                                                                      \
    if ((rpt) <= 1) { constexpr int R = 1; __VA_ARGS__; }                                                   \
    else if ((rpt) <= 2) { constexpr int R = 2; __VA_ARGS__; }                                              \
    else if ((rpt) <= 4) { constexpr int R = 4; __VA_ARGS__; }                                              \
    else { constexpr int R = 0; __VA_ARGS__; }                                                              \
  } while (0)

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
/* success exit of every entry point: a hipMemcpy / hipMemset that failed anywhere inside the call turns it into an error */
static int api_ok() {
  if (RT_STICKY()) { RT_STICKY_CLEAR(); return fail(QPG_ERR_RUNTIME, std::string("device copy failed: ") + RT_LAST_ERROR()); }
  return QPG_OK;
}
extern "C" const char *qpg_last_error(void) { return g_err.c_str(); }
extern "C" const char *qpg_backend_name(void) { return RT_BACKEND_NAME; }

static_assert(sizeof(QPGSettings) == sizeof(qpg_settings), "settings layout");

extern "C" void qpg_set_default_settings(QPGSettings *s) { /* src/qpalm.c:38-70, include/constants.h:65-110 */
  s->max_iter = 10000; s->inner_max_iter = 100; s->eps_abs = 1e-4; s->eps_rel = 1e-4;
  s->eps_abs_in = 1; s->eps_rel_in = 1; s->rho = 0.1; s->eps_prim_inf = 1e-5; s->eps_dual_inf = 1e-5;
  s->theta = 0.25; s->delta = 100; s->sigma_max = 1e9; s->sigma_init = 2e1; s->proximal = 1;
  s->gamma_init = 1e7; s->gamma_upd = 10; s->gamma_max = 1e7; s->scaling = 10; s->nonconvex = 0;
  s->verbose = 1; s->print_iter = 1; s->warm_start = 0; s->reset_newton_iter = 10000;
  s->enable_dual_termination = 0; s->dual_objective_limit = 1e20; s->time_limit = 1e20;
  s->ordering = 0; s->factorization_method = 2; s->max_rank_update = 160; s->max_rank_update_fraction = 0.1;
}

extern "C" int qpg_validate_settings(const QPGSettings *s) { /* src/validate.c:43-221 */
  if (!s) return 0;
  if (s->max_iter <= 0 || s->inner_max_iter <= 0) return 0;
  if (s->eps_abs < 0 || s->eps_rel < 0 || (s->eps_rel == 0 && s->eps_abs == 0)) return 0;
  if (s->eps_abs_in < 0 || s->eps_rel_in < 0 || (s->eps_rel_in == 0 && s->eps_abs_in == 0)) return 0;
  if (s->rho <= 0 || s->rho >= 1) return 0;
  if (s->eps_prim_inf < 0 || s->eps_dual_inf < 0) return 0;
  if (s->theta > 1 || s->delta <= 1 || s->sigma_max <= 0) return 0;
  if (s->proximal != 0 && s->proximal != 1) return 0;
  if (s->gamma_init <= 0 || s->gamma_upd < 1 || s->gamma_max < s->gamma_init) return 0;
  if (s->scaling < 0) return 0;
  if (s->warm_start != 0 && s->warm_start != 1) return 0;
  if (s->verbose != 0 && s->verbose != 1) return 0;
  if (s->print_iter <= 0 || s->reset_newton_iter <= 0) return 0;
  if (s->enable_dual_termination != 0 && s->enable_dual_termination != 1) return 0;
  return 1;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct qpg_ctx {
  int device;
  int lds_bytes;
  int max_slots;
  int update_rank_threshold;
  int narrow_rows;      /* 1: small QPs with short rows of A assemble the Schur matrix four columns per wavefront (form_schur_narrow) */
  int place_panel_wave; /* 0 (default since round 4): wavefront 0 of every workgroup runs the serial chains; 1: the workgroups of a CU run them on different SIMDs
                           (qp_place_panel_wave); 2: + the wavefronts that share those SIMDs own the rows that retire first.  Same box, round 4: 5340-5343 / 5278-5285 /
                           5320-5322 QP/s for 0 / 1 / 2 -- the hardware already spreads the wavefronts 0 of a CU's workgroups */
  int small_workgroups; /* 1: QPs whose factor has at most 256 rows run on 256-thread workgroups, four per CU, or (large batches of factors up to 192 rows) on
                           128-thread ones, seven per CU; 2 / 3 force one of the two; 0: the 512-thread instance for everything */
  int coop;             /* -1 automatic (a batch of at most 4 QPs with factors of at least 640 rows), 0 never, 1 whenever possible: the
                           factorisations and Newton solves of such QPs run on coop_workgroups workgroups (coop_solve) */
  int coop_workgroups;
  int coop_max_batch;      /* the automatic choice takes coop mode for batches of at most this many QPs (round 5: the launch chains of the members run
                              on streams of their own, min(coop_workgroups, 1024 / B) workgroups each) */
  int coop_rank_threshold; /* coop mode: k >= 0: active-set changes of more than k rows refactorise; -1: the reference's rule alone
                              (max_rank_update, max_rank_update_fraction: the reference's n_refactor / n_rank1 split); -2 (default): k = 16 (n / 2048),
                              from the measured costs -- a sweep of <= 16 ranks is a chain of n / 32 diagonal-block recurrences (about 40 us
                              each: 1.4 / 3.4 / 6.7 ms at n = 1000 / 2500 / 5000) against 1.0 / 4.2 / 14.3 ms for a refactorisation on the grid */
  int queue_order;         /* 1 (default): a launch through the work queue (B > slots) starts the members in descending order of the kernel time of their previous
                              solve (k_queue_order: the launch's tail is then made of short solves); 0: index order */
  int coop_test_kill;      /* TEST HOOK of the persistent sweep's give-up path: > 0 = the second workgroup of the N-th sweep launch of a solve gives up at once (as if
                              it had timed out): the iteration kernel must then rebuild the factor (tests/test_coop.py) */
  int coop_graphs;         /* coop mode: 1 = the fixed launch chains (factorisation, solve, update sweep) are recorded once and replayed as HIP graphs */
  int coop_updates;        /* coop mode: 2 (default) = a rank-update sweep is ONE launch, one workgroup per 128 rows, tables handed from owner to owner
                              inside it (co_updown_persist); 1 = one launch per block column (k_co_updown phase 2); 0 = they stay on
                              the QP's own workgroup (round 3's first version: 2.9 ms per rank at n = 2500, three quarters of config 5's time) */
  int sweep_ranks;         /* most ranks per sweep of the rank update: 16 (default) or 32 (the multi-pass form of dense_updown: half the panel traffic per
                              rank, bit-identical factors -- but measured SLOWER on MI355X in round 4, DESIGN section 7: 4.4-4.8 k against 5.2-5.3 k QP/s;
                              the sweep is bound by its serial chain, not by the bytes) */
  int factor_fused_solve;  /* 1 (default): on the Schur path a factorisation that a Newton solve follows carries the solve's forward substitution (dense_factor:
                              the right-hand side sits in LDS behind the factorisation's own blocks where it fits) -- L is streamed once less, d is bit for bit
                              the same; 0: the separate forward pass (A/B runs, tests) */
  int kkt_compact;         /* 1 (default): KKT mode's form + factorise skips the inactive constraints' unit rows (qpalm_kkt.h: kkt_form_compact / kkt_expand) */
  int sequential_rank_sums; /* the pivots of an update sweep as d_r = d_{r-1} + p_r, rank after rank (the reference's order; 15 dependent steps per column) instead of as a
                              prefix tree (4 steps): -1 (default) for QPs whose factor can get near-singular -- nonconvex ones and those whose Q has a column
                              without a positive diagonal entry (LPs) --, 1 for all, 0 for none.  DESIGN.md section 5 */
  int linesearch_hbm;      /* tests: 1 = the exact line search sorts in HBM with LDS tiles also where the breakpoints would fit the LDS (m > 3200 takes that path by itself) */
  int sparse_gpw;          /* sparse factor: columns a wavefront factorises at a time (1, 2, 4 or 8 groups of 64 / gpw lanes); 0 = the default */
  int sparse_lds;          /* sparse factor: 1 (default) = columns accumulate, and right-hand sides are solved, in LDS where they fit; 0 = the HBM forms, >= 2 = LDS for columns of at most that many entries (tests) */
  int sparse_ordering;     /* sparse factor: 0 = natural ordering (what the reference configures, solver_interface.c:530-540); 1 = nested dissection
                              (sparse_order: P H P' = L D L' -- a shallow, bushy elimination tree instead of a chain for band-like patterns);
                              -1 (default): dissection where the natural tree is deep and the dissected one at least four times shallower */
  int sparse_factor;       /* -1 (default): the sparse L D L' (qpalm_sparse.h) for factors of more than 8192 rows, the dense panel otherwise; 1: sparse
                              whenever the mode allows it (Schur path); 0: never (larger factors are refused) */
  int sparse_coop;         /* 0 (default): a sparse QP's factor operations run on its own workgroup; 1: a batch that keeps the sparse Schur factor, has at most
                              coop_max_batch members and B <= max_slots runs its factorisations and Newton solves on up to coop_workgroups workgroups
                              (sparse_coop_plan, coop_solve); read by qpg_batch_setup.  Path updates stay on the QP's workgroup.  The option "coop" does not switch this on */
  int sparse_kkt;          /* 0 (default): FACTORIZE_KKT keeps the dense (n+m) x (n+m) panel (more than 8192 rows are refused); 1: every KKT batch keeps a
                              sparse L D L' of K (qpalm_sparse_kkt.h), whatever its size */
  int ld_align;            /* leading dimension of the factor panels = rows rounded up to this many doubles.  16 (default): every column starts on a
                              128-byte line of the L2, so a wavefront's 1 KB column segment is 8 whole lines; with 8 (rounds 1-3) the odd columns of the
                              n = 1000 panel started mid-line and every segment touched 9 (measured: DESIGN section 4, round 4) */
  /* grow-only device scratch of qpg_sparse_matvec (the boundary's mat_vec on caller-owned matrices) */
  void *mv_buf[5];
  size_t mv_cap[5];
};

/* Host copy of the batch's problem data, already in the device layout AND in the upload layout: one slab of [array][QP][entries],
 * every array padded to the batch's strides, so that qpg_batch_setup copies each array with one DMA transfer (no packing pass).
 * The slab is anonymous memory with transparent huge pages requested: first-touching 5.8 GB of 4 KB pages (the benchmark batch)
 * costs 0.55 s whatever the number of threads -- the kernel serialises the faults -- against 0.03-0.06 s with 2 MB pages, and the
 * runtime copies from such memory at 44-56 GB/s, the rate of page-locked memory, whose allocation alone would cost 1.2 s
 * (tools/evidence/host_alloc_probe.hip, profiles/r04/setup/).  The arrays (H_*) and HostProblem: qpalm_host_convert.h. */

struct qpg_batch {
  qpg_ctx *ctx;
  int B, n, m, nnzA, nnzQ, nnzQf, ld, nslots, ls_stride;
  int small, threads, lds_bytes; /* instance of the kernels this batch runs on: 256-thread workgroups with 38 KB LDS, or 512 / ctx->lds_bytes */
  int kkt, nfac; /* FACTORIZE_KKT: factor slots of n + m rows (qpalm_set_factorization_method, solver_interface.c:20-75) */
  QPGSettings settings;
  std::vector<HostProblem> probs;
  char *hslab; size_t hslab_bytes, hoff[H_COUNT + 1], hper[H_COUNT], helem[H_COUNT]; /* slab, byte offset of each array, entries per QP, bytes per entry */
  template <class T> T *harr(int a, size_t b) const { return (T *)(hslab + hoff[a]) + b * hper[a]; } /* array a of member b */
  std::thread arena_thread; int arena_rc; bool arena_clean; /* the device arena is allocated next to the host-side conversion (see qpg_batch_create) */
  std::vector<int> host_status; /* QPG_ERROR marks from update_* validation */
  void *arena_d; size_t arena_d_bytes;
  void *dual_d; /* second resident factor per slot (LD_Q), present only while enable_dual_termination is set */
  size_t dual_d_bytes = 0;
  int sparse;            /* 1: the factor is a sparse L D L' (qpalm_sparse.h): symbolic analysis in qpg_batch_setup, values in sparse_d */
  void *co_tab_d; /* coop mode, persistent update sweep: the published tables of every member + its counter words (co_updown_persist) */
  void *sparse_d; size_t sparse_d_bytes; /* symbolic arrays of every member + values / work vectors of every slot */
  std::vector<long long> sp_nnz; /* nnz(L) of every member (qpg_batch_sparse_info) */
  std::vector<int> sp_levels, sp_perm; /* height of every member's elimination tree; [B][n] ordering of its factor (qpg_batch_sparse_perm) */
  std::vector<SpPlan> sp_plan; /* sparse coop mode: every member's launch plan (sparse_coop_plan; empty: the batch runs on one workgroup per QP) */
  qpg_view V;
  bool is_setup;
  float last_solve_ms;
  std::vector<std::pair<std::string, std::pair<void *, size_t> > > named; /* device arrays by name */
  /* coop mode: recorded launch chains (key = QP * 16 + chain: 0/1 factorisation into L / LD_Q, 2 solve, 3.. update sweep);
   * dropped when anything the chains depend on changes (co_sig) */
  struct CoGraph { int uses; bool ready; rt_graph_t exec; };
  std::map<int, CoGraph> co_graphs;
  std::string co_sig;
  long co_replays; /* graph launches of the last solve (QPALM_COOP_PROFILE prints it) */
  long co_sweeps;  /* persistent-sweep launches of the last solve (coop_test_kill counts them) */
  long co_op_chains = 0; /* single operations of the boundary that ran on the grid kernels (run_op_coop; qpg_batch_coop_op_chains) */
  /* qpg_batch_update_Q_A: entry k of the device's A / Q values of a member = entry map[k] of the arrays its caller passed to qpg_batch_set_problem*
   * (take_column sorts a column's rows, Q keeps rows >= column).  An empty map = the same order (sorted columns, no upper entry of Q: the usual input).
   * The maps go to the device at the first update that needs one (val_maps_d: [B][nnzA] + [B][nnzQ] positions + [B][2] "same order" flags). */
  int nnzA_in, nnzQ_in; /* nnzA_max / nnzQ_max as the caller gave them: the strides of the arrays qpg_batch_update_Q_A takes */
  std::vector<std::vector<int> > map_A, map_Q;
  void *val_maps_d = nullptr; bool val_maps_current = false;
  /* the latest accepted raw q / bmin / bmax ([B][n], [B][m], [B][m], one block in that order): created by the first qpg_batch_update_q / _bounds after
   * a setup as a copy of the slab's arrays + the update (the device holds them scaled in place; the slab keeps the problem as set, which a second
   * qpg_batch_setup returns to).  The host forms of the updates keep the record in raw_h; the device forms (qpg_batch_update_q_device /
   * _bounds_device) keep it in raw_d, a block of the same layout in device memory that their kernels fill (allocated by the first of them).
   * raw_cur says which is current -- 0: raw_h (empty: the slab), 1: raw_d, 2: both -- and whoever needs the other one copies it over at that
   * moment, in one transfer (raw_need_host / raw_need_device). */
  std::vector<double> raw_h;
  void *raw_d = nullptr; int raw_cur = 0;
  double sens_floor = 0.0; /* qpg_batch_set_sens_penalty: the penalty floor of the sensitivity solves' preconditioner (0: the solve's own penalties) */
  double *raw_q() { return raw_h.data(); }
  double *raw_bmin() { return raw_h.data() + (size_t)B * n; }
  double *raw_bmax() { return raw_h.data() + (size_t)B * n + (size_t)B * m; }
  double *raw_d_q() const { return (double *)raw_d; }
  double *raw_d_bmin() const { return (double *)raw_d + (size_t)B * n; }
  double *raw_d_bmax() const { return (double *)raw_d + (size_t)B * n + (size_t)B * m; }
};
static void co_graphs_clear(qpg_batch *bt) {
  for (auto &g : bt->co_graphs) if (g.second.ready) RT_GRAPH_FREE(g.second.exec);
  bt->co_graphs.clear();
}

extern "C" int qpg_ctx_create(int device, qpg_ctx **out) {
  if (!out) return fail(QPG_ERR_INVALID, "qpg_ctx_create: out is NULL");
  std::string why;
  if (RT_DEVICE_INIT(device, why) != 0) return fail(QPG_ERR_NO_DEVICE, "qpg_ctx_create: " + why);
  qpg_ctx *c = new qpg_ctx();
  c->device = device; c->lds_bytes = QPG_LDS_DEFAULT; c->max_slots = 512; c->update_rank_threshold = -1; c->small_workgroups = 1; c->place_panel_wave = 0; c->narrow_rows = 1; c->coop = -1; c->coop_workgroups = 256; c->coop_max_batch = 4; c->coop_rank_threshold = -2; c->coop_updates = 2; c->coop_test_kill = 0; c->queue_order = 1; c->coop_graphs = 1; c->ld_align = 16; c->sweep_ranks = 16; c->kkt_compact = 1; c->factor_fused_solve = 1; c->sparse_factor = -1; c->sparse_kkt = 0; c->sparse_coop = 0; c->sparse_ordering = -1; c->sparse_lds = 1; c->sparse_gpw = 0; c->linesearch_hbm = 0; c->sequential_rank_sums = -1;
  for (int k = 0; k < 5; k++) { c->mv_buf[k] = nullptr; c->mv_cap[k] = 0; }
  *out = c;
  return api_ok();
}
extern "C" void qpg_ctx_destroy(qpg_ctx *ctx) {
  if (!ctx) return;
  for (int k = 0; k < 5; k++) if (ctx->mv_buf[k]) RT_FREE(ctx->mv_buf[k]);
  RT_RELEASE_STREAMS();
  delete ctx;
}
static int ctx_scratch(qpg_ctx *ctx, int k, size_t bytes, void **p) {
  if (bytes > ctx->mv_cap[k]) {
    if (ctx->mv_buf[k]) RT_FREE(ctx->mv_buf[k]);
    ctx->mv_buf[k] = nullptr; ctx->mv_cap[k] = 0;
    const size_t cap = align_up(bytes + bytes / 2, 4096);
    if (RT_MALLOC(&ctx->mv_buf[k], cap) != 0) return 1;
    ctx->mv_cap[k] = cap;
  }
  *p = ctx->mv_buf[k];
  return 0;
}
extern "C" int qpg_ctx_set_option(qpg_ctx *ctx, const char *name, qpg_int value) {
  if (!ctx || !name) return fail(QPG_ERR_INVALID, "qpg_ctx_set_option: NULL");
  if (!strcmp(name, "lds_bytes")) { if (value < QPG_LDS_DEFAULT || value > 160 * 1024 - 8192) return fail(QPG_ERR_INVALID, "lds_bytes out of range"); ctx->lds_bytes = (int)value; }
  else if (!strcmp(name, "max_slots")) { if (value < 1) return fail(QPG_ERR_INVALID, "max_slots < 1"); ctx->max_slots = (int)value; }
  else if (!strcmp(name, "update_rank_threshold")) ctx->update_rank_threshold = (int)value;
  else if (!strcmp(name, "small_workgroups")) ctx->small_workgroups = (value >= 0 && value <= 3) ? (int)value : 1;
  else if (!strcmp(name, "place_panel_wave")) ctx->place_panel_wave = (value < 0 || value > 2) ? 2 : (int)value; /* 0 (default) the hardware's own placement, 1 panel waves on SIMDs 0 / 1, 2 + row ownership by SIMD */
  else if (!strcmp(name, "narrow_rows")) ctx->narrow_rows = value ? 1 : 0;
  else if (!strcmp(name, "coop")) ctx->coop = (value < 0) ? -1 : (value ? 1 : 0);
  else if (!strcmp(name, "coop_rank_threshold")) ctx->coop_rank_threshold = (value < -1) ? -2 : (int)value;
  else if (!strcmp(name, "coop_updates")) ctx->coop_updates = (value >= 0 && value <= 2) ? (int)value : 2;
  else if (!strcmp(name, "coop_graphs")) ctx->coop_graphs = value ? 1 : 0;
  else if (!strcmp(name, "coop_test_kill")) ctx->coop_test_kill = (int)value;
  else if (!strcmp(name, "queue_order")) ctx->queue_order = value ? 1 : 0;
  else if (!strcmp(name, "sweep_ranks")) { if (value != 16 && value != 32) return fail(QPG_ERR_INVALID, "sweep_ranks must be 16 or 32"); ctx->sweep_ranks = (int)value; }
  else if (!strcmp(name, "kkt_compact")) ctx->kkt_compact = value ? 1 : 0;
  else if (!strcmp(name, "factor_fused_solve")) ctx->factor_fused_solve = value ? 1 : 0;
  else if (!strcmp(name, "sparse_factor")) ctx->sparse_factor = (value < 0) ? -1 : (value ? 1 : 0);
  else if (!strcmp(name, "sparse_kkt")) ctx->sparse_kkt = value ? 1 : 0;
  else if (!strcmp(name, "sparse_coop")) { if (value != 0 && value != 1) return fail(QPG_ERR_INVALID, "sparse_coop must be 0 or 1"); ctx->sparse_coop = (int)value; }
  else if (!strcmp(name, "sequential_rank_sums")) ctx->sequential_rank_sums = (value < 0) ? -1 : (value ? 1 : 0);
  else if (!strcmp(name, "linesearch_hbm")) ctx->linesearch_hbm = (value < 0) ? 0 : (int)std::min<qpg_int>(value, 1 << 20); /* >= 2: also caps the tile (a power of two): small QPs then exercise several tiles and the HBM steps between them */
  else if (!strcmp(name, "sparse_gpw")) ctx->sparse_gpw = (int)value;
  else if (!strcmp(name, "sparse_lds")) ctx->sparse_lds = (value < 0) ? 0 : (int)value; /* >= 2: the LDS form takes columns of at most that many entries (tests) */
  else if (!strcmp(name, "sparse_ordering")) ctx->sparse_ordering = (value < 0) ? -1 : (value ? 1 : 0);
  else if (!strcmp(name, "ld_align")) { if (value != 8 && value != 16 && value != 32) return fail(QPG_ERR_INVALID, "ld_align must be 8, 16 or 32"); ctx->ld_align = (int)value; }
  else if (!strcmp(name, "coop_max_batch")) { if (value < 1) return fail(QPG_ERR_INVALID, "coop_max_batch < 1"); ctx->coop_max_batch = (int)value; }
  else if (!strcmp(name, "coop_workgroups")) { if (value < 1 || value > 4096) return fail(QPG_ERR_INVALID, "coop_workgroups out of range"); ctx->coop_workgroups = (int)value; }
  else return fail(QPG_ERR_INVALID, std::string("unknown option ") + name);
  return api_ok();
}

static int arena_alloc(qpg_batch *bt);
/* anonymous memory, transparent huge pages requested (madvise; plain pages where the kernel does not offer them) */
static void *host_slab_alloc(size_t bytes) {
  void *p = mmap(nullptr, std::max<size_t>(bytes, 4096), PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (p == MAP_FAILED) return nullptr;
#ifdef MADV_HUGEPAGE
  if (bytes >= ((size_t)64 << 20)) (void)madvise(p, bytes, MADV_HUGEPAGE);
#endif
  return p;
}
static void host_slab_free(void *p, size_t bytes) { if (p) munmap(p, std::max<size_t>(bytes, 4096)); }

extern "C" int qpg_batch_create(qpg_ctx *ctx, qpg_int B, qpg_int n, qpg_int m, qpg_int nnzA_max, qpg_int nnzQ_max,
                                const QPGSettings *settings, qpg_batch **out) {
  if (!ctx || !out) return fail(QPG_ERR_INVALID, "qpg_batch_create: NULL argument");
  if (B <= 0 || n <= 0 || m < 0 || nnzA_max < 0 || nnzQ_max < 0) return fail(QPG_ERR_INVALID, "qpg_batch_create: bad dimensions");
  if (!qpg_validate_settings(settings)) return fail(QPG_ERR_INVALID, "Settings validation returned failure");
  /* qpalm_set_factorization_method (solver_interface.c:20-75): FACTORIZE_KKT (0) and FACTORIZE_SCHUR (1) are honoured.
   * FACTORIZE_KKT_OR_SCHUR (2) compares nnz(KKT) with an estimate of nnz(Schur) for SPARSE factors; this engine keeps the
   * factor as one dense panel, for which the n x n Schur panel is never larger than the (n+m) x (n+m) KKT panel: SCHUR. */
  const int kkt = (settings->factorization_method == 0) ? 1 : 0;
  const qpg_int nfac = kkt ? n + m : n;
  /* Factors of more than 8192 rows (the dense panel's limit: its right-hand side must fit the LDS) are kept as a sparse L D L'
   * (qpalm_sparse.h; round 5) on the Schur path (round 6: with the second resident factor of dual termination); "sparse_factor" = 1
   * selects it for any size.  KKT mode keeps the dense panel unless "sparse_kkt" = 1 asks for the sparse factor of K (qpalm_sparse_kkt.h),
   * whatever the size.  (The reference decides per matrix inside CHOLMOD; here the mode is fixed when the batch is created,
   * before the patterns are known, because the device arena is sized then.) */
  const int sparse = kkt ? ctx->sparse_kkt : ((ctx->sparse_factor == 1 || (ctx->sparse_factor != 0 && nfac > 8192)) ? 1 : 0);
  /* the sparse factor of K (option "sparse_kkt") has no LD_Q on K's pattern and no lobpcg / Gershgorin bound of its own */
  if (kkt && sparse && settings->enable_dual_termination)
    return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_create: the sparse KKT factor does not support enable_dual_termination (no LD_Q on the pattern of K)");
  if (kkt && sparse && settings->nonconvex)
    return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_create: the sparse KKT factor does not support nonconvex");
  if (nfac > 8192 && !sparse)
    return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_create: the factor exceeds the dense-panel limit of 8192 rows (the sparse factor covers the Schur path)");
  /* up to 4 QP_T rows the update sweep keeps its running vectors in registers (k_solve<1|2|4>); larger factors (up to the
   * 8192 rows whose right-hand side fits the LDS) use the large-factor sweep with the vectors in HBM (k_solve<0>) */
  qpg_batch *bt = new qpg_batch();
  bt->ctx = ctx; bt->B = (int)B; bt->n = (int)n; bt->m = (int)m;
  bt->nnzA = (int)std::max<qpg_int>(nnzA_max, 1); bt->nnzQ = (int)std::max<qpg_int>(nnzQ_max, 1); bt->nnzQf = 2 * bt->nnzQ;
  bt->nnzA_in = (int)nnzA_max; bt->nnzQ_in = (int)nnzQ_max;
  bt->map_A.resize((size_t)B); bt->map_Q.resize((size_t)B);
  bt->kkt = kkt; bt->nfac = (int)nfac; bt->sparse = sparse;
  bt->ld = (int)align_up((size_t)nfac, (size_t)ctx->ld_align);
  {
    int p2s = 2; while (p2s < 2 * (int)m) p2s <<= 1;
#ifdef QP_TWO_INSTANCES
    bt->small = (!sparse && ctx->small_workgroups && nfac <= QP_T_SMALL && (size_t)p2s * 12 <= (size_t)QP_LDS_SMALL) ? 1 : 0;
    /* ... and on the 128-thread instance (seven workgroups per CU) when that is the faster one: more QPs than the 256-thread instance
     * keeps resident, factor of at most 192 rows (measured, 16384 QPs: n = 64 +25 %, 128 +12 %, mpc-160 +3..6 %, 250 -4 %: DESIGN.md section 7);
     * option value 2 forces it wherever its LDS fits, 3 keeps the 256-thread instance */
    const bool tiny_fits = (size_t)p2s * 12 <= (size_t)QP_LDS_TINY && (size_t)8 * n <= (size_t)QP_LDS_TINY;
    if (bt->small && tiny_fits && (ctx->small_workgroups == 2 || (ctx->small_workgroups == 1 && nfac <= 192 && B > (qpg_int)(2 * ctx->max_slots)))) bt->small = 2;
#else
    bt->small = 0;
#endif
    bt->threads = bt->small == 2 ? QP_T_TINY : bt->small ? QP_T_SMALL : QP_T;
    bt->lds_bytes = bt->small == 2 ? QP_LDS_TINY : bt->small ? QP_LDS_SMALL : ctx->lds_bytes;
    /* dense_solve keeps the whole right-hand side behind its two diagonal-block tiles in LDS (also for the dual objective and in
     * KKT mode, where the factor has n + m rows): large factors get the LDS they need -- one workgroup per CU then, which is
     * all a factor of that size leaves room for anyway -- instead of reading and writing beyond the block */
    const size_t need = sparse ? 0 : sizeof(QP_INST(qp512, SolveLds)) + (size_t)nfac * sizeof(double); /* (the sparse solves work in HBM) */
    if (need > (size_t)bt->lds_bytes) {
      if (need > (size_t)(160 * 1024 - 8192)) { delete bt; return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_create: the factor's right-hand side does not fit the LDS of a compute unit"); }
      bt->lds_bytes = (int)align_up(need, 256);
    }
  }
  bt->nslots = std::min(bt->B, bt->small == 2 ? QP_TINY_PER_CU * ctx->max_slots / 2 : bt->small ? 2 * ctx->max_slots : ctx->max_slots);
  { /* resident factor panels: at most 64 GB of the 288 GB (a 5000 x 5000 panel is 200 MB) */
    const size_t slot_bytes = sparse ? (size_t)64 * nfac * sizeof(double) : (size_t)bt->ld * (size_t)nfac * sizeof(double); /* (sparse: a guess, the patterns come later) */
    const size_t cap = std::max<size_t>(1, ((size_t)64 << 30) / std::max<size_t>(slot_bytes, 1));
    if ((size_t)bt->nslots > cap) bt->nslots = (int)cap;
  }
  int p2 = 2; while (p2 < 2 * bt->m) p2 <<= 1;
  bt->ls_stride = p2;
  bt->settings = *settings;
  bt->probs.resize(bt->B);
  for (auto &p : bt->probs) p.set = false;
  bt->host_status.assign(bt->B, QPG_UNSOLVED);
  bt->arena_d = nullptr; bt->dual_d = nullptr; bt->sparse_d = nullptr; bt->sparse_d_bytes = 0; bt->co_tab_d = nullptr; bt->is_setup = false; bt->last_solve_ms = 0.f;
  memset(&bt->V, 0, sizeof(bt->V));
  { /* host slab: [array][QP][entries] */
    const size_t nn = bt->n, mm = bt->m, zA = bt->nnzA, zQ = bt->nnzQ, zF = bt->nnzQf;
    const size_t per[H_COUNT] = {nn + 1, zA, mm + 1, zA, zA, zA, nn + 1, zQ, nn + 1, zF, zF, zA, zQ, nn, mm, mm};
    size_t off = 0, raw = 0;
    for (int a = 0; a < H_COUNT; a++) raw += (size_t)bt->B * per[a] * ((a >= H_AX) ? sizeof(double) : sizeof(int));
    /* arrays of a large batch start on 2 MB boundaries (whole huge pages); a small batch must not pin sixteen huge pages for a few KB */
    const size_t aln = (raw >= ((size_t)64 << 20)) ? ((size_t)2 << 20) : 256;
    for (int a = 0; a < H_COUNT; a++) {
      bt->hper[a] = per[a]; bt->helem[a] = (a >= H_AX) ? sizeof(double) : sizeof(int);
      bt->hoff[a] = off;
      off = align_up(off + (size_t)bt->B * per[a] * bt->helem[a], aln);
    }
    bt->hoff[H_COUNT] = off;
    bt->hslab_bytes = off;
    bt->hslab = (char *)host_slab_alloc(off);
    if (!bt->hslab) { delete bt; return fail(QPG_ERR_ALLOC, "qpg_batch_create: host allocation failed"); }
  }
  /* The device arena's size depends on the batch's dimensions only, and allocating it is driver work on the host (26 ms per GB,
   * 0.3-0.5 s for the benchmark batch): a thread of its own does it while the caller converts the problem data
   * (qpg_batch_set_problems); qpg_batch_setup joins it. */
  bt->arena_rc = 0; bt->arena_clean = false;
  {
    const int device = ctx->device;
    bt->arena_thread = std::thread([bt, device]() { RT_THREAD_DEVICE(device); bt->arena_rc = arena_alloc(bt); });
  }
  *out = bt;
  return api_ok();
}

static int set_problem_impl(qpg_batch *bt, qpg_int idx, qpg_int n_, qpg_int m_, const qpg_int *Qp, const qpg_int *Qi, const qpg_float *Qx,
                            const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax, const qpg_float *q,
                            qpg_float c, const qpg_float *bmin, const qpg_float *bmax);
extern "C" int qpg_batch_set_problem(qpg_batch *bt, qpg_int idx, const qpg_int *Qp, const qpg_int *Qi, const qpg_float *Qx,
                                     const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax, const qpg_float *q,
                                     qpg_float c, const qpg_float *bmin, const qpg_float *bmax) {
  if (!bt) return fail(QPG_ERR_INVALID, "qpg_batch_set_problem: NULL");
  return set_problem_impl(bt, idx, bt->n, bt->m, Qp, Qi, Qx, Ap, Ai, Ax, q, c, bmin, bmax);
}
/* a member smaller than the batch (size-bucketed batches, e.g. a directory of QPS files): n <= batch n, m <= batch m.
 * The member keeps its own dimensions on the device (loops and the factor run over n x n / m rows); only the array
 * strides are the batch's. */
extern "C" int qpg_batch_set_problem_sized(qpg_batch *bt, qpg_int idx, qpg_int n, qpg_int m, const qpg_int *Qp, const qpg_int *Qi,
                                           const qpg_float *Qx, const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax,
                                           const qpg_float *q, qpg_float c, const qpg_float *bmin, const qpg_float *bmax) {
  if (!bt) return fail(QPG_ERR_INVALID, "qpg_batch_set_problem_sized: NULL");
  if (n <= 0 || n > bt->n || m < 0 || m > bt->m) return fail(QPG_ERR_INVALID, "qpg_batch_set_problem_sized: dimensions exceed the batch's");
  return set_problem_impl(bt, idx, n, m, Qp, Qi, Qx, Ap, Ai, Ax, q, c, bmin, bmax);
}
static int set_problem_impl(qpg_batch *bt, qpg_int idx, qpg_int n_, qpg_int m_, const qpg_int *Qp, const qpg_int *Qi, const qpg_float *Qx,
                            const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax, const qpg_float *q,
                            qpg_float c, const qpg_float *bmin, const qpg_float *bmax) {
  if (idx < 0 || idx >= bt->B) return fail(QPG_ERR_INVALID, "qpg_batch_set_problem: bad index");
  const size_t ib = (size_t)idx;
  ConvertDst D;
  for (int a = 0; a < H_COUNT; a++) { D.p[a] = bt->hslab + bt->hoff[a] + ib * bt->hper[a] * bt->helem[a]; D.stride[a] = bt->hper[a]; }
  std::string msg;
  const int rc = convert_problem(D, (int)n_, (int)m_, Qp, Qi, Qx, Ap, Ai, Ax, q, c, bmin, bmax, bt->probs[ib], bt->map_A[ib], bt->map_Q[ib], msg);
  return rc ? fail(rc, msg) : api_ok();
}

/* qpalm_setup's host work for MANY QPs in one call (src/qpalm.c:128-144 deep copies + the A' pattern of iteration.c:81): members
 * first .. first + count - 1 from arrays of pointers (entry k = member first + k; n / m NULL = the batch's dimensions for every
 * member), the per-QP conversion to the device layout spread over host threads.  One C call instead of `count` calls from the
 * caller's loop: 8192 QPs of the benchmark took 3.1 s through qpg_batch_set_problem from Python, round 3. */
static int host_threads(size_t items) {
  unsigned hw = std::thread::hardware_concurrency();
  if (hw == 0) hw = 4;
  const char *e = getenv("QPALM_HOST_THREADS");
  if (e && atoi(e) > 0) hw = (unsigned)atoi(e);
  /* measured on the 2 x EPYC 9575F host of the MI355X box, 8192 QPs of the benchmark (tools/evidence/setup_timing.py, profiles/r04/setup/): 1 thread 1.00 s,
   * 8 threads 0.21 s, 16: 0.12 s, 32: 0.12 s, 64: 0.22 s.  (Before the huge-page slab the conversion allocated ~1 MB of 4 KB pages per QP
   * and the page faults queued up on the address space: 0.55 s at 8 threads, slower beyond.) */
  const unsigned cap = (e && atoi(e) > 0) ? 256u : 24u;
  return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(hw, cap), items));
}
template <class F> static void parallel_for(size_t count, F body) { /* body(k) for k in [0, count), dealt dynamically */
  const int nt = host_threads(count);
  if (nt <= 1) { for (size_t k = 0; k < count; k++) body(k); return; }
  std::atomic<size_t> next(0);
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++)
    th.emplace_back([&]() { for (size_t k = next.fetch_add(1); k < count; k = next.fetch_add(1)) body(k); });
  for (auto &t : th) t.join();
}
extern "C" int qpg_batch_set_problems(qpg_batch *bt, qpg_int first, qpg_int count, const qpg_int *n, const qpg_int *m,
                                      const qpg_int *const *Qp, const qpg_int *const *Qi, const qpg_float *const *Qx,
                                      const qpg_int *const *Ap, const qpg_int *const *Ai, const qpg_float *const *Ax,
                                      const qpg_float *const *q, const qpg_float *c, const qpg_float *const *bmin, const qpg_float *const *bmax) {
  if (!bt || !Qp || !Qi || !Qx || !Ap || !Ai || !Ax || !q || !bmin || !bmax) return fail(QPG_ERR_INVALID, "qpg_batch_set_problems: NULL");
  if (first < 0 || count < 0 || first + count > bt->B) return fail(QPG_ERR_INVALID, "qpg_batch_set_problems: bad range");
  for (qpg_int k = 0; k < count; k++) {
    const qpg_int nk = n ? n[k] : bt->n, mk = m ? m[k] : bt->m;
    if (nk <= 0 || nk > bt->n || mk < 0 || mk > bt->m) return fail(QPG_ERR_INVALID, "qpg_batch_set_problems: dimensions exceed the batch's");
  }
  std::vector<int> rc((size_t)count, QPG_OK);
  std::vector<std::string> msg((size_t)count);
  parallel_for((size_t)count, [&](size_t k) {
    rc[k] = set_problem_impl(bt, first + (qpg_int)k, n ? n[k] : bt->n, m ? m[k] : bt->m, Qp[k], Qi[k], Qx[k], Ap[k], Ai[k], Ax[k], q[k], c ? c[k] : 0.0, bmin[k], bmax[k]);
    if (rc[k] != QPG_OK) msg[k] = g_err; /* (the message is thread-local) */
  });
  for (qpg_int k = 0; k < count; k++)
    if (rc[k] != QPG_OK) return fail(rc[k], msg[k]);
  return api_ok();
}

/* ---- device arena ------------------------------------------------------------------------- */
struct Carver {
  char *base; size_t off; qpg_batch *bt;
  template <class T> void take(T *&p, size_t count, const char *name) {
    off = align_up(off, 256);
    if (base) { p = (T *)(base + off); if (name) bt->named.push_back(std::make_pair(std::string(name), std::make_pair((void *)p, count * sizeof(T)))); }
    off += count * sizeof(T);
  }
};

static void carve(qpg_batch *bt, Carver &c) {
  qpg_view &V = bt->V;
  const size_t B = bt->B, n = bt->n, m = bt->m, nzA = bt->nnzA, nzQ = bt->nnzQ, nzQf = bt->nnzQf, ns = bt->nslots;
  const size_t mx = std::max(n, m), ls = bt->ls_stride;
  c.take(V.Ap, B * (n + 1), "Ap"); c.take(V.Ai, B * nzA, "Ai"); c.take(V.Atp, B * (m + 1), "Atp"); c.take(V.Ati, B * nzA, "Ati");
  c.take(V.Atperm, B * nzA, "Atperm"); c.take(V.Ainv, B * nzA, "Ainv"); c.take(V.Qp, B * (n + 1), "Qp"); c.take(V.Qi, B * nzQ, "Qi");
  c.take(V.Qfp, B * (n + 1), "Qfp"); c.take(V.Qfi, B * nzQf, "Qfi"); c.take(V.Qfperm, B * nzQf, "Qfperm");
  c.take(V.Ax, B * nzA, "A_values"); c.take(V.Atx, B * nzA, "Atx"); c.take(V.Atss, B * nzA, "At_sqrt_sigma");
  c.take(V.Qx, B * nzQ, "Q_values"); c.take(V.Qfx, B * nzQf, "Qfx");
  c.take(V.q, B * n, "q"); c.take(V.bmin, B * m, "bmin"); c.take(V.bmax, B * m, "bmax"); c.take(V.c0, B, "c");
  c.take(V.x, B * n, "x"); c.take(V.y, B * m, "y"); c.take(V.Axv, B * m, "Ax"); c.take(V.Qxv, B * n, "Qx");
  c.take(V.Aty, B * n, "Aty"); c.take(V.x_prev, B * n, "x_prev"); c.take(V.x0, B * n, "x0");
  c.take(V.sigma, B * m, "sigma"); c.take(V.sigma_inv, B * m, "sigma_inv"); c.take(V.sqrt_sigma, B * m, "sqrt_sigma");
  c.take(V.At_scale, B * m, "At_scale");
  c.take(V.Axys, B * m, "Axys"); c.take(V.z, B * m, "z"); c.take(V.pri_res, B * m, "pri_res"); c.take(V.pri_res_in, B * m, "pri_res_in");
  c.take(V.yh, B * m, "yh"); c.take(V.Atyh, B * n, "Atyh"); c.take(V.df, B * n, "df"); c.take(V.dphi, B * n, "dphi");
  c.take(V.dphi_prev, B * n, "dphi_prev"); c.take(V.d, B * n, "d"); c.take(V.Qd, B * n, "Qd"); c.take(V.Ad, B * m, "Ad");
  c.take(V.delta_y, B * m, "delta_y"); c.take(V.delta_x, B * n, "delta_x"); c.take(V.temp_n, B * n, "temp_n"); c.take(V.temp_m, B * m, "temp_m");
  c.take(V.D, B * n, "D"); c.take(V.Dinv, B * n, "Dinv"); c.take(V.E, B * m, "E"); c.take(V.Einv, B * m, "Einv");
  c.take(V.ls_key, B * ls, "ls_key"); c.take(V.ls_idx, B * ls, "ls_idx");
  c.take(V.ls_delta, B * 2 * m, "delta"); c.take(V.ls_alpha, B * 2 * m, "alpha");
  c.take(V.active, B * m, "active"); c.take(V.active_old, B * m, "active_old"); c.take(V.enter, B * m, "enter"); c.take(V.leave, B * m, "leave");
  c.take(V.sol_x, B * n, "solution_x"); c.take(V.sol_y, B * m, "solution_y");
  const size_t nf = bt->nfac;
  if (bt->sparse) { c.take(V.L, 64, "L"); c.take(V.Dg, ns * nf, "Dfac"); c.take(V.Wst, 64, "Wst"); } /* no dense panel, no update staging */
  else { c.take(V.L, ns * (size_t)bt->ld * nf, "L"); c.take(V.Dg, ns * nf, "Dfac"); c.take(V.Wst, ns * QPG_WST_STRIDE(nf), "Wst"); }
  if (bt->kkt) {
    c.take(V.kkt_sol, B * (n + m), "sol_kkt"); c.take(V.kkt_rhs, B * (n + m), "rhs_kkt"); c.take(V.kkt_tmp, B * (n + m), "kkt_tmp"); c.take(V.kkt_rhs2, B * (n + m), "kkt_rhs2");
    c.take(V.kkt_state, B * m, "kkt_state"); c.take(V.kkt_list, B * m, "kkt_list");
  }
  c.take(V.dual_rhs, B * n, "dual_rhs"); c.take(V.nq, B, "nq"); c.take(V.mq, B, "mq");
  c.take(V.op_in, mx, "op_in"); c.take(V.op_out, mx, "op_out");
  c.take(V.sc, B, "scalars"); c.take(V.settings, 1, "settings"); c.take(V.queue, 64 + QPG_CU_KEYS, "queue");
  c.take(V.order, B, "queue_order");
}

static int find_named(qpg_batch *bt, const char *name, void **p, size_t *bytes) {
  for (auto &e : bt->named) if (e.first == name) { *p = e.second.first; *bytes = e.second.second; return 1; }
  return 0;
}

static int blocks_for(qpg_batch *bt) { return std::min(bt->B, 2048); }

/* LD_Q slots (qpalm.c:274,466-467): one more dense panel per resident workgroup, only for dual termination */
static int ensure_dual_slots(qpg_batch *bt) {
  qpg_view &V = bt->V;
  if (!bt->settings.enable_dual_termination) { V.LQ = nullptr; V.DgQ = nullptr; return 0; }
  /* same slot strides as L / Dfac: ld * n and n doubles; with the sparse factor the values of LD_Q on the main factor's pattern (sp_nnzL per slot:
   * known after sparse_setup, which calls this again) */
  if (bt->sparse && V.sp_nnzL <= 0) { V.LQ = nullptr; V.DgQ = nullptr; return 0; }
  const size_t lbytes = align_up(bt->sparse ? (size_t)bt->nslots * (size_t)V.sp_nnzL * sizeof(double) : (size_t)bt->nslots * bt->ld * bt->nfac * sizeof(double), 256),
               dbytes = (size_t)bt->nslots * bt->nfac * sizeof(double);
  if (bt->dual_d && bt->dual_d_bytes < lbytes + dbytes) { RT_FREE(bt->dual_d); bt->dual_d = nullptr; }
  if (!bt->dual_d) { if (RT_MALLOC(&bt->dual_d, lbytes + dbytes) != 0) { bt->dual_d = nullptr; return 1; } bt->dual_d_bytes = lbytes + dbytes; }
  V.LQ = (double *)bt->dual_d;
  V.DgQ = (double *)((char *)bt->dual_d + lbytes);
  return 0;
}

static int arena_alloc(qpg_batch *bt) { /* runs on the thread qpg_batch_create starts */
  Carver c0 = {nullptr, 0, bt};
  carve(bt, c0);
  bt->arena_d_bytes = align_up(c0.off, 256);
  if (RT_MALLOC(&bt->arena_d, bt->arena_d_bytes) != 0) { bt->arena_d = nullptr; return 1; }
  bt->named.clear();
  Carver c1 = {(char *)bt->arena_d, 0, bt};
  carve(bt, c1);
  RT_MEMSET(bt->arena_d, 0, bt->arena_d_bytes);
  if (RT_SYNC() != 0) return 1;
  bt->arena_clean = true;
  return 0;
}

/* ---- sparse factor: the symbolic analysis (host, once per member) is qpalm_host_symbolic.h; this is the pattern it reads */
static SparsePattern member_pattern(const qpg_batch *bt, size_t b) {
  const HostProblem &P = bt->probs[b];
  return SparsePattern{P.n, P.m, bt->harr<int>(H_AP, b), bt->harr<int>(H_AI, b), bt->harr<int>(H_ATP, b), bt->harr<int>(H_ATI, b),
                       bt->harr<int>(H_QFP, b), bt->harr<int>(H_QFI, b)};
}
/* analysis of every member (host threads), one device block for the symbolic arrays of all members and the values / work vectors of
 * all slots, upload */
static int sparse_setup(qpg_batch *bt) {
  qpg_view &V = bt->V;
  const size_t B = bt->B, n = bt->nfac, ns = bt->nslots; /* n: rows of the factor (n + m in KKT mode) */
  std::vector<SparseSym> sym(B);
  std::vector<int> rc(B, 0);
  std::vector<std::string> why(B);
  const size_t max_nnz = (size_t)1 << 30; /* int32 positions; 8 GB of values per slot */
  const int ordering = bt->ctx->sparse_ordering;
  const bool kkt = bt->kkt != 0;
  parallel_for(B, [&](size_t b) { rc[b] = sparse_symbolic(member_pattern(bt, b), kkt, ordering, max_nnz, sym[b], why[b]); });
  for (size_t b = 0; b < B; b++) if (rc[b]) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_setup: member " + std::to_string(b) + ": " + why[b]);
  size_t nzmax = 1;
  bt->sp_nnz.assign(B, 0); bt->sp_levels.assign(B, 0); bt->sp_perm.assign(B * n, 0);
  for (size_t b = 0; b < B; b++) {
    nzmax = std::max(nzmax, sym[b].Li.size()); bt->sp_nnz[b] = (long long)sym[b].Li.size(); bt->sp_levels[b] = sym[b].nlev;
    for (size_t j = 0; j < n; j++) bt->sp_perm[b * n + j] = j < sym[b].perm.size() ? sym[b].perm[j] : (int)j; /* (members smaller than the batch: identity beyond their n) */
  }
  const int nw = bt->threads / 64;
  const size_t m = bt->m, zA = bt->nnzA, zF = bt->nnzQf;
  /* layout of the block: ints first */
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
  const size_t oLp = take(B * (n + 1) * 4), oLi = take(B * nzmax * 4), oRp = take(B * (n + 1) * 4), oRk = take(B * nzmax * 4), oRpos = take(B * nzmax * 4);
  const size_t oLev = take(B * (n + 1) * 4), oCol = take(B * n * 4), oNlev = take(B * 4);
  const size_t oPerm = take(B * n * 4), oAtiP = take(B * zA * 4), oQfiP = take(B * zF * 4), oFirst = take(B * m * 4);
  /* columns per wavefront: eight groups of eight lanes (round 6; measured on the two sparse batch workloads, profiles/r06/sparse_lds/gpw.txt: 2 / 4 / 8
   * groups 11.0 / 13.4 / 14.8 k QP/s banded, 15.9 / 16.9 / 17.3 k blocks -- a wavefront's instructions serve twice the columns, and a sparse
   * factor's columns rarely have more than eight entries), halved while the work vectors of all slots would exceed 4 GB */
  int gpw = (bt->ctx->sparse_gpw == 1 || bt->ctx->sparse_gpw == 2 || bt->ctx->sparse_gpw == 4 || bt->ctx->sparse_gpw == 8) ? bt->ctx->sparse_gpw : 8;
  while (gpw > 1 && ns * (size_t)nw * gpw * n * 8 > ((size_t)4 << 30)) gpw >>= 1;
  V.sp_gpw = gpw; V.sp_lds = bt->ctx->sparse_lds;
  const size_t oLx = take(ns * nzmax * 8), oWv = take(ns * (size_t)nw * gpw * n * 8), oTmp = take(ns * n * 8);
  /* sparse coop mode: G workgroups per launch as in coop_linear_algebra (the members' chains run side by side), fewer while the work vectors of the HBM
   * form of a column -- one zeroed n-vector per group of lanes per workgroup per member -- would not fit what the slots' own work vectors (sp_wv above)
   * leave of the SAME 4 GB: the two together stay under it (columns in the LDS form need no vector) */
  int coG = 0;
  if (bt->ctx->sparse_coop == 1 && !kkt && bt->threads == QP_T && bt->B <= bt->ctx->coop_max_batch && bt->B <= bt->nslots) {
    coG = std::max(8, std::min(bt->ctx->coop_workgroups, 1024 / std::max(1, bt->B)));
    const size_t per = B * (size_t)nw * gpw * n * 8, own = ns * (size_t)nw * gpw * n * 8, left = (own < ((size_t)4 << 30)) ? ((size_t)4 << 30) - own : 0;
    coG = (int)std::max<size_t>(1, std::min<size_t>((size_t)coG, left / std::max<size_t>(per, 1)));
  }
  const size_t oCoWv = take(B * (size_t)coG * nw * gpw * n * 8);
  if (bt->sparse_d && bt->sparse_d_bytes < off) { RT_FREE(bt->sparse_d); bt->sparse_d = nullptr; }
  if (!bt->sparse_d) { if (RT_MALLOC(&bt->sparse_d, off) != 0) { bt->sparse_d = nullptr; return fail(QPG_ERR_ALLOC, "device allocation failed (sparse factor: " + std::to_string(off >> 20) + " MB)"); } bt->sparse_d_bytes = off; }
  char *base = (char *)bt->sparse_d;
  RT_MEMSET(base, 0, off); /* (the work vectors must start as zeros) */
  V.sparse = 1; V.sp_nnzL = (int)nzmax;
  V.sp_Lp = (int32_t *)(base + oLp); V.sp_Li = (int32_t *)(base + oLi); V.sp_Rp = (int32_t *)(base + oRp); V.sp_Rk = (int32_t *)(base + oRk);
  V.sp_Rpos = (int32_t *)(base + oRpos); V.sp_levptr = (int32_t *)(base + oLev); V.sp_levcol = (int32_t *)(base + oCol); V.sp_nlev = (int32_t *)(base + oNlev);
  V.sp_Lx = (double *)(base + oLx); V.sp_wv = (double *)(base + oWv); V.sp_tmp = (double *)(base + oTmp);
  V.sp_co_G = coG; V.sp_co_wv = coG ? (double *)(base + oCoWv) : nullptr;
  bt->sp_plan.clear();
  if (coG) {
    bt->sp_plan.resize(B);
    for (size_t b = 0; b < B; b++) sparse_coop_plan(sym[b].levptr, sym[b].nlev, bt->probs[b].n, nw * gpw, bt->threads, coG, bt->sp_plan[b]);
  }
  V.sp_perm = (int32_t *)(base + oPerm); V.sp_AtiP = (int32_t *)(base + oAtiP); V.sp_QfiP = (int32_t *)(base + oQfiP); V.sp_first = (int32_t *)(base + oFirst);
  std::vector<int> nlev(B);
  std::vector<int> atip(zA), qfip(zF), first(m);
  for (size_t b = 0; b < B; b++) {
    const SparseSym &S = sym[b];
    nlev[b] = S.nlev;
    sparse_factor_index(member_pattern(bt, b), S, kkt, atip, qfip, first);
    RT_MEMCPY_H2D(V.sp_perm + b * n, bt->sp_perm.data() + b * n, n * 4);
    RT_MEMCPY_H2D(V.sp_AtiP + b * zA, atip.data(), zA * 4);
    RT_MEMCPY_H2D(V.sp_QfiP + b * zF, qfip.data(), zF * 4);
    RT_MEMCPY_H2D(V.sp_first + b * m, first.data(), m * 4);
    RT_MEMCPY_H2D(V.sp_Lp + b * (n + 1), S.Lp.data(), S.Lp.size() * 4);
    if (!S.Li.empty()) {
      RT_MEMCPY_H2D(V.sp_Li + b * nzmax, S.Li.data(), S.Li.size() * 4);
      RT_MEMCPY_H2D(V.sp_Rk + b * nzmax, S.Rk.data(), S.Rk.size() * 4);
      RT_MEMCPY_H2D(V.sp_Rpos + b * nzmax, S.Rpos.data(), S.Rpos.size() * 4);
    }
    RT_MEMCPY_H2D(V.sp_Rp + b * (n + 1), S.Rp.data(), S.Rp.size() * 4);
    RT_MEMCPY_H2D(V.sp_levptr + b * (n + 1), S.levptr.data(), S.levptr.size() * 4);
    RT_MEMCPY_H2D(V.sp_levcol + b * n, S.levcol.data(), S.levcol.size() * 4);
  }
  RT_MEMCPY_H2D(V.sp_nlev, nlev.data(), B * 4);
  return QPG_OK;
}
/* nnz(L) of one member's sparse factor and the levels of its elimination tree (after qpg_batch_setup; QPG_ERR_UNSUPPORTED in the dense modes) */
extern "C" int qpg_batch_sparse_info(qpg_batch *bt, qpg_int idx, qpg_int *nnzL, qpg_int *device_bytes) {
  if (!bt || !bt->is_setup) return fail(QPG_ERR_INVALID, "qpg_batch_sparse_info: batch is not set up");
  if (!bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_sparse_info: the batch keeps dense factors");
  if (idx < 0 || idx >= bt->B) return fail(QPG_ERR_INVALID, "qpg_batch_sparse_info: bad index");
  if (nnzL) *nnzL = (qpg_int)bt->sp_nnz[(size_t)idx];
  if (device_bytes) *device_bytes = (qpg_int)bt->sparse_d_bytes;
  return api_ok();
}

/* the launch plan of one member in sparse coop mode: launches per factorisation, launches per Newton solve, the largest grid among them; all zero when
 * the batch runs on one workgroup per QP (QPG_ERR_UNSUPPORTED in the dense modes) */
extern "C" int qpg_batch_sparse_coop_info(qpg_batch *bt, qpg_int idx, qpg_int *factor_launches, qpg_int *solve_launches, qpg_int *max_grid) {
  if (!bt || !bt->is_setup) return fail(QPG_ERR_INVALID, "qpg_batch_sparse_coop_info: batch is not set up");
  if (!bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_sparse_coop_info: the batch keeps dense factors");
  if (idx < 0 || idx >= bt->B) return fail(QPG_ERR_INVALID, "qpg_batch_sparse_coop_info: bad index");
  const bool on = !bt->sp_plan.empty();
  if (factor_launches) *factor_launches = on ? (qpg_int)bt->sp_plan[(size_t)idx].factor.size() : 0;
  if (solve_launches) *solve_launches = on ? (qpg_int)bt->sp_plan[(size_t)idx].solve_launches : 0;
  if (max_grid) *max_grid = on ? (qpg_int)bt->sp_plan[(size_t)idx].max_grid : 0;
  return api_ok();
}

/* the ordering of one member's sparse factor: P H P' = L D L' with perm[new] = old (n entries; identity = the reference's natural
 * ordering), and the height of its elimination tree; in KKT mode P K P' = L D L' (n + m entries, [x; y] numbering) */
extern "C" int qpg_batch_sparse_perm(qpg_batch *bt, qpg_int idx, qpg_int *perm, qpg_int *levels) {
  if (!bt || !bt->is_setup) return fail(QPG_ERR_INVALID, "qpg_batch_sparse_perm: batch is not set up");
  if (!bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_sparse_perm: the batch keeps dense factors");
  if (idx < 0 || idx >= bt->B) return fail(QPG_ERR_INVALID, "qpg_batch_sparse_perm: bad index");
  const HostProblem &P = bt->probs[(size_t)idx];
  const int nf = bt->kkt ? P.n + P.m : P.n; /* rows of the member's factor: n + m in KKT mode */
  if (perm) for (int j = 0; j < nf; j++) perm[j] = bt->sp_perm[(size_t)idx * bt->nfac + j];
  if (levels) *levels = bt->sp_levels[(size_t)idx];
  return api_ok();
}

/* member idx's sparse factor as it stands in device memory, in the factor's own numbering (qpg_batch_sparse_perm maps it): column pointers (nf + 1
 * entries, nf = n, or n + m in KKT mode), row indices and values of the strict lower part (nnz(L) of qpg_batch_sparse_info each), pivots (nf).  Any
 * output may be NULL.  The symbolic arrays are copied back from the device (the analysis is not kept on the host); a slot holds QP idx's values only
 * while B <= max_slots (as qpg_batch_get_factor). */
extern "C" int qpg_batch_get_sparse_factor(qpg_batch *bt, qpg_int idx, qpg_int *Lp, qpg_int *Li, qpg_float *Lx, qpg_float *D) {
  if (!bt || !bt->is_setup) return fail(QPG_ERR_INVALID, "qpg_batch_get_sparse_factor: batch is not set up");
  if (!bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_get_sparse_factor: the batch keeps dense factors (qpg_batch_get_factor reads those)");
  if (idx < 0 || idx >= bt->B) return fail(QPG_ERR_INVALID, "qpg_batch_get_sparse_factor: bad index");
  if (bt->B > bt->nslots) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_get_sparse_factor: a slot belongs to a QP only while B <= max_slots");
  const qpg_view &V = bt->V;
  const HostProblem &P = bt->probs[(size_t)idx];
  const size_t nf = (size_t)(bt->kkt ? P.n + P.m : P.n), nz = (size_t)bt->sp_nnz[(size_t)idx], b = (size_t)idx;
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, RT_LAST_ERROR());
  std::vector<int> tmp(std::max(nf + 1, nz));
  if (Lp) {
    RT_MEMCPY_D2H(tmp.data(), V.sp_Lp + b * ((size_t)V.nfac + 1), (nf + 1) * sizeof(int));
    for (size_t j = 0; j <= nf; j++) Lp[j] = tmp[j];
  }
  if (Li && nz) {
    RT_MEMCPY_D2H(tmp.data(), V.sp_Li + b * (size_t)V.sp_nnzL, nz * sizeof(int));
    for (size_t e = 0; e < nz; e++) Li[e] = tmp[e];
  }
  if (Lx && nz) RT_MEMCPY_D2H(Lx, V.sp_Lx + b * (size_t)V.sp_nnzL, nz * sizeof(double));
  if (D) RT_MEMCPY_D2H(D, V.Dg + b * (size_t)V.nfac, nf * sizeof(double));
  return api_ok();
}

/* the per-QP scalars qpalm_setup leaves (seq_hint is the member's own) */
static qpg_scalars setup_scalars(const qpg_batch *bt) {
  qpg_scalars sc0;
  memset(&sc0, 0, sizeof(sc0));
  sc0.status = QPG_UNSOLVED; sc0.gamma = bt->settings.gamma_init; sc0.sqrt_delta = sqrt(bt->settings.delta);
  sc0.sc_c = 1.0; sc0.sc_cinv = 1.0; sc0.kkt_first = 1; /* qpalm.c:272 */
  sc0.kkt_na = -1;
  return sc0;
}
/* set_settings_nonconvex (qpalm.c:293-296), after scale_data like the reference */
static int run_lobpcg(qpg_batch *bt) {
  qpg_view &V = bt->V;
  const size_t B = bt->B, n = bt->n;
  /* start vector of lobpcg: rand()/RAND_MAX from the C library's default state (nonconvex.c:41-44, B9).  Every QP of the
   * batch gets the sequence a fresh process would produce (glibc TYPE_3 generator, seed 1), restated here so that the
   * result does not depend on the host's libc or on earlier rand() calls. */
  std::vector<double> x0(B * n, 0.0);
  {
    int32_t tab[344];
    tab[0] = 1;
    for (int i = 1; i < 31; i++) { long hi = tab[i - 1] / 127773, lo = tab[i - 1] % 127773; long v = 16807 * lo - 2836 * hi; if (v < 0) v += 2147483647; tab[i] = (int32_t)v; }
    for (int i = 31; i < 34; i++) tab[i] = tab[i - 31];
    for (int i = 34; i < 344; i++) tab[i] = (int32_t)((uint32_t)tab[i - 31] + (uint32_t)tab[i - 3]);
    std::vector<uint32_t> o(344 + n);
    for (int i = 0; i < 344; i++) o[i] = (uint32_t)tab[i];
    for (size_t k = 0; k < n; k++) o[344 + k] = o[344 + k - 31] + o[344 + k - 3];
    for (size_t b = 0; b < B; b++)
      for (int k = 0; k < bt->probs[b].n; k++) x0[b * n + k] = (double)(int)(o[344 + k] >> 1) / 2147483647;
  }
  RT_MEMCPY_H2D(V.d, x0.data(), x0.size() * sizeof(double));
  BT_LAUNCH(bt, k_lobpcg, blocks_for(bt), 0, V);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_lobpcg failed: " + std::string(RT_LAST_ERROR()));
  return QPG_OK;
}

extern "C" int qpg_batch_setup(qpg_batch *bt) {
  if (!bt) return fail(QPG_ERR_INVALID, "qpg_batch_setup: NULL");
  for (int b = 0; b < bt->B; b++) if (!bt->probs[b].set) return fail(QPG_ERR_INVALID, "qpg_batch_setup: problem not set for every batch member");
  co_graphs_clear(bt); /* recorded coop launch chains hold the members' sizes */
  qpg_view &V = bt->V;
  if (bt->arena_thread.joinable()) bt->arena_thread.join();
  if (bt->arena_rc != 0 || !bt->arena_d) return fail(QPG_ERR_ALLOC, "device allocation failed");
  if (!bt->arena_clean) { /* a second setup of the same batch starts from a cleared arena like the first */
    RT_MEMSET(bt->arena_d, 0, bt->arena_d_bytes);
    if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "arena clear failed: " + std::string(RT_LAST_ERROR()));
  }
  bt->arena_clean = false;
  bt->is_setup = false;
  bt->raw_h.clear(); bt->raw_cur = 0; /* the device gets the slab's q and bounds again (raw_d, if there is one, is stale until the next device-form update) */
  bt->val_maps_current = false;                                  /* (the members may have been set again) */
  V.B = bt->B; V.n = bt->n; V.m = bt->m; V.ld = bt->ld; V.nnzA = bt->nnzA; V.nnzQ = bt->nnzQ; V.nnzQf = bt->nnzQf;
  V.ls_hbm = bt->ctx->linesearch_hbm; V.seq_mode = bt->ctx->sequential_rank_sums;
  V.nslots = bt->nslots; V.lds_bytes = bt->lds_bytes; V.update_rank_threshold = bt->ctx->update_rank_threshold; V.place_panel_wave = bt->ctx->place_panel_wave;
  V.ls_stride = bt->ls_stride;
  { /* form_schur_narrow (a quarter wavefront per column): small QPs with short rows of A, Schur path */
    size_t nnz_rows = 0, rows = 0;
    for (auto &hp : bt->probs) { nnz_rows += (size_t)hp.nzA; rows += (size_t)hp.m; }
    const size_t colbufs = (size_t)4 * (bt->threads / 64) * bt->n * sizeof(double);
    V.narrow_rows = (bt->ctx->narrow_rows && !bt->kkt && colbufs <= (size_t)bt->lds_bytes && nnz_rows <= 16 * std::max<size_t>(rows, 1)) ? 1 : 0;
  }
  V.wst_stride = (int)QPG_WST_STRIDE(bt->nfac);
  V.sweep_ranks = bt->ctx->sweep_ranks;
  V.kkt_compact = bt->ctx->kkt_compact;
  V.factor_fused_solve = bt->ctx->factor_fused_solve;
  V.kkt = bt->kkt; V.nfac = bt->nfac;
  if (ensure_dual_slots(bt) != 0) return fail(QPG_ERR_ALLOC, "device allocation failed (LD_Q slots)");
  V.sparse = 0; V.sp_co_G = 0; V.sp_co_wv = nullptr;
  bt->sp_plan.clear();
  if (bt->sparse) {
    const int rcs = sparse_setup(bt);
    if (rcs != QPG_OK) return rcs;
    if (ensure_dual_slots(bt) != 0) return fail(QPG_ERR_ALLOC, "device allocation failed (LD_Q values of the sparse factor)");
  }
  /* upload the problem data: the host slab already holds every array in the device layout with the batch's strides
   * (qpg_batch_set_problems), one transfer per array.  (Round 3 packed 5.8 GB into pageable vectors and copied array by array: 1.8 s;
   * the first form of round 4 packed chunks into page-locked staging, 0.26 s of which 0.17 s were hipHostMalloc / hipHostFree.) */
  const size_t B = bt->B, n = bt->n, m = bt->m;
  {
    char *const dev[H_COUNT] = {(char *)V.Ap, (char *)V.Ai, (char *)V.Atp, (char *)V.Ati, (char *)V.Atperm, (char *)V.Ainv, (char *)V.Qp, (char *)V.Qi,
                                (char *)V.Qfp, (char *)V.Qfi, (char *)V.Qfperm, (char *)V.Ax, (char *)V.Qx, (char *)V.q, (char *)V.bmin, (char *)V.bmax};
    for (int a = 0; a < H_COUNT; a++)
      if (bt->hper[a] && RT_MEMCPY_H2D_ASYNC(dev[a], bt->hslab + bt->hoff[a], B * bt->hper[a] * bt->helem[a], 0) != 0)
        return fail(QPG_ERR_RUNTIME, "upload failed: " + std::string(RT_LAST_ERROR()));
    RT_COPY_MARK(0);
    /* ... while the copies run: the small per-QP records */
    std::vector<double> c0(B);
    std::vector<qpg_scalars> sc(B);
    const qpg_scalars sc0 = setup_scalars(bt);
    for (size_t b = 0; b < B; b++) {
      c0[b] = bt->probs[b].c; sc[b] = sc0; bt->host_status[b] = QPG_UNSOLVED;
      /* a column of Q without a positive diagonal entry: H = Q + A' Sigma A + I / gamma can have pivots of the size of 1 / gamma (seq_hint) */
      const int *Qp = bt->harr<int>(H_QP, b), *Qi = bt->harr<int>(H_QI, b);
      const double *Qx = bt->harr<double>(H_QX, b);
      int hint = 0;
      for (int j = 0; j < bt->probs[b].n && !hint; j++) {
        bool pos = false;
        for (int k = Qp[j]; k < Qp[j + 1]; k++) if (Qi[k] == j && Qx[k] > 0.0) { pos = true; break; }
        if (!pos) hint = 1;
      }
      sc[b].seq_hint = hint;
    }
    RT_MEMCPY_H2D(V.c0, c0.data(), B * sizeof(double));
    RT_MEMCPY_H2D(V.sc, sc.data(), B * sizeof(qpg_scalars));
    RT_COPY_WAIT(0);
  }
#define UP(dst, vec) RT_MEMCPY_H2D(dst, (vec).data(), (vec).size() * sizeof((vec)[0]))
  {
    std::vector<int> nq(B), mq(B);
    bool mixed = false;
    for (size_t b = 0; b < B; b++) { nq[b] = bt->probs[b].n; mq[b] = bt->probs[b].m; mixed = mixed || nq[b] != bt->n || mq[b] != bt->m; }
    void *pn = nullptr, *pm = nullptr; size_t nb_ = 0;
    find_named(bt, "nq", &pn, &nb_); find_named(bt, "mq", &pm, &nb_);
    int32_t *dn = (int32_t *)pn, *dm = (int32_t *)pm;
    UP(dn, nq); UP(dm, mq);
    V.nq = dn; V.mq = dm;
    if (!mixed) { V.nq = nullptr; V.mq = nullptr; } /* uniform batch: the kernels use the batch dimensions directly */
  }
#undef UP
  qpg_settings st;
  memcpy(&st, &bt->settings, sizeof(st));
  RT_MEMCPY_H2D(V.settings, &st, sizeof(st));
  BT_LAUNCH(bt, k_setup, blocks_for(bt), 0, V, (int)bt->settings.scaling, 0);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_setup failed: " + std::string(RT_LAST_ERROR()));
  if (bt->settings.nonconvex) {
    const int rcl = run_lobpcg(bt);
    if (rcl != QPG_OK) return rcl;
  }
  bt->is_setup = true;
  return api_ok();
}

#define NEED_SETUP(bt, fn) \
  if (!(bt) || !(bt)->is_setup) return fail(QPG_ERR_INVALID, std::string(fn) + ": batch is not set up")

/* The members a per-step call covers: every member (list = NULL), or the S members k_select listed in V.order (qpg_batch_*_subset_device).  The
 * kernels that take it visit one listed member per workgroup and stop at the entry behind the last one. */
struct Subset {
  const int32_t *list = nullptr;
  int S = 0;
  int count(const qpg_batch *bt) const { return list ? S : bt->B; }
  int blocks(const qpg_batch *bt) const { return std::min(count(bt), 2048); }
};

static int warm_start_launch(qpg_batch *bt, int has_x, int has_y, const qpg_float *d_x, const qpg_float *d_y, const Subset &sub) {
  BT_LAUNCH(bt, k_warm_start, sub.blocks(bt), 0, bt->V, has_x, has_y, (const double *)d_x, (const double *)d_y, sub.list);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_warm_start failed: " + std::string(RT_LAST_ERROR()));
  return api_ok();
}
extern "C" int qpg_batch_warm_start(qpg_batch *bt, const qpg_float *x, const qpg_float *y) {
  NEED_SETUP(bt, "qpg_batch_warm_start");
  if (x) RT_MEMCPY_H2D(bt->V.x, x, (size_t)bt->B * bt->n * sizeof(double));
  if (y) RT_MEMCPY_H2D(bt->V.y, y, (size_t)bt->B * bt->m * sizeof(double));
  return warm_start_launch(bt, x ? 1 : 0, y ? 1 : 0, nullptr, nullptr, Subset());
}
/* ... with x, y already in device memory: the kernel reads the caller's arrays */
extern "C" int qpg_batch_warm_start_device(qpg_batch *bt, const qpg_float *d_x, const qpg_float *d_y) {
  NEED_SETUP(bt, "qpg_batch_warm_start_device");
  return warm_start_launch(bt, d_x ? 1 : 0, d_y ? 1 : 0, d_x, d_y, Subset());
}

/* qpalm_warm_start with each QP's own last solution (what qpg_batch_get_solution returns), taken from HBM: the receding-
 * horizon loop of an MPC controller without the round trip of x, y through the host. */
extern "C" int qpg_batch_warm_start_last(qpg_batch *bt) {
  NEED_SETUP(bt, "qpg_batch_warm_start_last");
  return warm_start_launch(bt, 2, 2, nullptr, nullptr, Subset());
}

/* subset > 0: the launch covers the `subset` members k_select listed in V.order (always through the work queue, whatever B and "queue_order"): the
 * list is there already, and the workgroups stop at the entry behind it */
static int launch_solve_kernel(qpg_batch *bt, const qpg_view &V_, int budget, int dynamic, float *ms_out, int subset = 0) { /* dynamic: bit 0 work queue, bit 1 fresh solve */
  qpg_view V = V_;
  if (!subset && (!bt->ctx->queue_order || bt->B > (1 << 17))) V.order = nullptr; /* (k_queue_order is B^2 compares: beyond 131 072 members the queue hands out the index order) */
  const int grid = std::min(subset ? subset : bt->B, bt->nslots);
  if (ms_out || (dynamic & 2)) RT_MEMSET(bt->V.queue, 0, (64 + QPG_CU_KEYS) * sizeof(int)); /* work-queue head and the per-CU arrival counters
                                                                                               (coop mode: once per solve, it needs neither) */
  const int rpt = (bt->nfac + bt->threads - 1) / bt->threads;
  const size_t shm = (size_t)bt->lds_bytes;
  float ms = 0.f;
  if ((dynamic & 1) && (dynamic & 2) && V.order && !subset) /* a fresh solve through the work queue: longest previous solve first (k_queue_order) */
    BT_LAUNCH(bt, k_queue_order, (bt->B + bt->threads - 1) / bt->threads, 0, V);
  if (bt->sparse) {
    RT_TIMED_LAUNCH(ms, QP_INST(qp512, k_solve<QPG_RPT_SPARSE>), grid, QP_T, shm, V, budget, dynamic);
    if (ms_out) *ms_out = ms;
    if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_solve (sparse factor) failed: " + std::string(RT_LAST_ERROR()));
    return QPG_OK;
  }
  if (!ms_out) { /* coop mode: thousands of short launches per solve, no event pair around each */
    BT_RPT(rpt, R, BT_LAUNCH(bt, k_solve<R>, grid, shm, V, budget, dynamic));
    return QPG_OK;
  }
  BT_RPT(rpt, R, BT_TIMED_LAUNCH(ms, bt, k_solve<R>, grid, shm, V, budget, dynamic));
  if (ms_out) *ms_out = ms;
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_solve failed: " + std::string(RT_LAST_ERROR()));
  return QPG_OK;
}
static int launch_solve(qpg_batch *bt, int budget, int dynamic, int subset = 0) {
  float ms = 0.f;
  const int rc = launch_solve_kernel(bt, bt->V, budget, dynamic, &ms, subset);
  if (rc != QPG_OK) return rc;
  bt->last_solve_ms = ms;
  return api_ok();
}

/* ---- coop mode ------------------------------------------------------------------------------------------------------------
 * One large QP (BASELINE.json configs 2 and 5 as written: "single ... QP on 1 MI355X") cannot fill the chip from one workgroup:
 * its time goes into the factorisation, the rank updates and the triangular solves of ONE dense panel.  Here the QP's iteration
 * still runs on its workgroup (k_solve, unchanged code: residuals, termination, active sets, line search), but it suspends at
 * its linear-algebra site (qpg_view.offload, qpg_scalars.pend_*) and the host chains multi-workgroup kernels for it: Schur
 * assembly by columns, a right-looking LDL' with two launches per 32-column block (rows below the block; trailing update on the
 * matrix cores over every later (block column, row pass) item + the next diagonal block), and the triangular solves one block
 * per launch; the kernel boundary is the only
 * synchronisation.  Rank updates (coop_updates = 1): k_co_updown, one launch per 32-column block (every workgroup repeats the
 * recurrence on the diagonal block, then applies the table to its rows).  Refactorise-or-update: by default the cheaper of the two
 * by measured cost (coop_rank_threshold, see qpg_ctx), so n_refactor / n_rank1 are not the reference's split -- the matrices
 * factorised, and the iterates to rounding, are; coop_rank_threshold = -1 keeps the reference's rule and its split.
 * Schur mode, 512-thread instance, B <= resident slots. */
static bool coop_wanted(const qpg_batch *bt) {
  if (bt->kkt || bt->small || bt->sparse || bt->B > bt->nslots) return false;
  if (bt->ctx->coop == 0) return false;
  if (bt->ctx->coop == 1) return true;
  /* round 5, B = 4 at n = 1000 (ms per step of the whole batch): coop 92.6 (the members' chains on side streams; one after the other before: ~150), one workgroup
   * per QP 60.4 -- several QPs at that size are better off side by side on their own workgroups; from ~1500 rows on a workgroup alone is ten times slower */
  if (bt->B == 1) return bt->nfac >= 640;
  return bt->B <= bt->ctx->coop_max_batch && bt->nfac >= 1536; /* measured (ms per solve, coop / one workgroup): n = 384 14.0 / 11.7, 512 20.5 / 21.2, 768 28.6 / 39.0, 1000 40.6 / 64.0,
                                            2500 137 / 1712, 5000 399 / ~7000 */
}
/* sparse coop mode: decided at setup, where the launch plans are made (sparse_setup) */
static bool sparse_coop_wanted(const qpg_batch *bt) { return bt->sparse && !bt->kkt && !bt->sp_plan.empty(); }
/* runs one launch chain: plainly the first time (function attributes get set), recorded into a graph the second time, replayed after */
template <class F> static void co_chain(qpg_batch *bt, int key, F issue) {
  if (!RT_GRAPHS || !bt->ctx->coop_graphs || key < 0) { issue(); return; }
  qpg_batch::CoGraph &g = bt->co_graphs[key];
  if (g.ready) { bt->co_replays++; RT_GRAPH_LAUNCH(g.exec); return; }
  if (++g.uses < 2 || g.uses > 2) { issue(); return; } /* (a recording that failed is not tried again) */
  if (RT_GRAPH_BEGIN() != 0) { issue(); return; }
  issue();
  if (RT_GRAPH_END(&g.exec) != 0) { issue(); return; }
  g.ready = true;
  bt->co_replays++;
  RT_GRAPH_LAUNCH(g.exec);
}
/* workgroups per launch of a member's chain: the members' chains run side by side (coop_solve) */
static int coop_grid(const qpg_batch *bt) { return std::max(8, std::min(bt->ctx->coop_workgroups, 1024 / std::max(1, bt->B))); }
static int coop_linear_algebra(qpg_batch *bt, const qpg_view &V, int b, const qpg_scalars &sc) {
  if (bt->sparse) { /* sparse coop mode: the member's plan, launch by launch (chains 0 / 1: the factorisation into the factor / LD_Q, 2: the solve) */
    const SpPlan &P = bt->sp_plan[(size_t)b];
    const int slot = b;
    {
      char sig[200];
      snprintf(sig, sizeof(sig), "sp %d %d %p %p %p %p", V.sp_co_G, (int)bt->lds_bytes, (void *)bt->sparse_d, (void *)V.LQ, (void *)V.sc, (void *)V.sp_co_wv);
      if (bt->co_sig != sig) { co_graphs_clear(bt); bt->co_sig = sig; }
    }
    if (sc.pend_la == 1 || sc.pend_la == 3 || sc.pend_la == 7) { /* (with or without A' Sigma A, the proximal term, gamma: read from the QP's scalars by the kernel) */
      const int which = (sc.pend_la == 7) ? 1 : 0;
      co_chain(bt, b * 16 + which, [&]() {
        for (const auto &l : P.factor) RT_LAUNCH(QP_INST(qp512, k_co_sp_factor), l.grid, QP_T, (size_t)bt->lds_bytes, V, b, slot, which, l.lev0, l.lev1);
      });
    }
    if (sc.pend_kind == 0 && sc.pend_la != 7) { /* Newton step: d = -(L D L')^{-1} dphi */
      co_chain(bt, b * 16 + 2, [&]() {
        RT_LAUNCH(QP_INST(qp512, k_co_sp_solve), P.vec_grid, QP_T, (size_t)64, V, b, slot, 0, 0, 0);
        for (const auto &l : P.solve) RT_LAUNCH(QP_INST(qp512, k_co_sp_solve), l.grid, QP_T, (size_t)64, V, b, slot, 1, l.lev0, l.lev1);
        RT_LAUNCH(QP_INST(qp512, k_co_sp_solve), P.vec_grid, QP_T, (size_t)64, V, b, slot, 2, 0, 0);
        for (size_t k = P.solve.size(); k-- > 0;) RT_LAUNCH(QP_INST(qp512, k_co_sp_solve), P.solve[k].grid, QP_T, (size_t)64, V, b, slot, 3, P.solve[k].lev0, P.solve[k].lev1);
        if (!P.solve.empty() && P.solve[0].grid > 1) RT_LAUNCH(QP_INST(qp512, k_co_sp_solve), P.vec_grid, QP_T, (size_t)64, V, b, slot, 3, 0, 0);
      });
    }
    return 0;
  }
  const int n = bt->probs[b].n, NB = 32, slot = b;
  const int G = coop_grid(bt);
  /* FactorLds + FactorStage / SolveLds: below 48 KB, so that no launch needs a function-attribute call */
  const size_t lds_factor = ((sizeof(QP_INST(qp512, FactorLds)) + 15) & ~(size_t)15) + sizeof(QP_INST(qp512, FactorStage)) + 64, lds_solve = sizeof(QP_INST(qp512, CoSolveLds)) + 64;
  auto grid_for = [&](long units) { return (int)std::max<long>(1, std::min<long>(G, units)); };
  { /* the recorded chains hold the view and the grid sizes by value */
    char sig[200];
    snprintf(sig, sizeof(sig), "%d %d %d %p %p %p %p", G, bt->nfac, (int)bt->lds_bytes, (void *)V.L, (void *)V.LQ, (void *)V.sc, (void *)V.co_tab); /* (a chain is keyed by its QP: members of different sizes keep theirs) */
    if (bt->co_sig != sig) { co_graphs_clear(bt); bt->co_sig = sig; }
  }
  if (sc.pend_la == 1 || sc.pend_la == 3 || sc.pend_la == 7) {
    const int which = (sc.pend_la == 7) ? 1 : 0;
    co_chain(bt, b * 16 + which, [&]() {
      RT_LAUNCH(QP_INST(qp512, k_co_form), grid_for(n), QP_T, (size_t)bt->lds_bytes, V, b, slot);
      RT_LAUNCH(QP_INST(qp512, k_co_factor_diag), 1, QP_T, lds_factor, V, b, slot, which, 0);
      for (int J = 0; J + NB < n; J += NB) { /* right-looking: rows below block J, then the trailing update with its 32 columns (+ the next diagonal block) */
        RT_LAUNCH(QP_INST(qp512, k_co_factor_rows), grid_for((n - J - NB + QP_T - 1) / QP_T), QP_T, lds_factor, V, b, slot, which, J);
        long items = 0;
        for (int Jc = J + NB; Jc < n; Jc += NB) items += ((n - Jc + 15) / 16 + 15) / 16;
        RT_LAUNCH(QP_INST(qp512, k_co_factor_trailing), grid_for(items), QP_T, lds_factor, V, b, slot, which, J);
      }
    });
  }
  if (sc.pend_la == 2 || sc.pend_la == 4) { /* rank update / downdate of the resident factor, <= 16 ranks per sweep, one launch per block column */
    const int n_up = (sc.pend_la == 2) ? sc.nb_enter : sc.pend_nchange, n_dn = (sc.pend_la == 2) ? sc.nb_leave : 0, K = QPG_KMAX;
    const size_t lds_ud = sizeof(QP_INST(qp512, UpdownBigLds)<QPG_KMAX>) + 64;
    for (int r0 = 0; r0 < n_up + n_dn; r0 += K) {
      if (V.co_tab && bt->ctx->coop_test_kill > 0 && ++bt->co_sweeps == bt->ctx->coop_test_kill) { const int one = 1; RT_MEMCPY_H2D(V.co_flags + (size_t)b * 4 + 2, &one, sizeof(int)); }
      co_chain(bt, (r0 / K < 12) ? b * 16 + 3 + r0 / K : -1, [&]() { /* (the kernels read the rank counts from the QP's scalars: the chain of sweep r0 / 16 never changes) */
        RT_LAUNCH(QP_INST(qp512, k_co_updown), grid_for(((long)K * n + 4 * QP_T - 1) / (4 * QP_T)), QP_T, (size_t)64, V, b, slot, 0, 0, r0);
        RT_LAUNCH(QP_INST(qp512, k_co_updown), 1, QP_T, (size_t)64, V, b, slot, 1, 0, r0);
        if (V.co_tab) { /* the whole sweep in one launch: one workgroup per 128 rows, all resident (at most 64) */
          RT_LAUNCH(QP_INST(qp512, k_co_sweep), (n + CO_UD_ROWS - 1) / CO_UD_ROWS, QP_T, lds_ud + (size_t)NB * K * sizeof(double) + 16, V, b, slot, r0);
        } else
        for (int J = 0; J < n + NB; J += NB) /* the launch after the last block writes its stage back */
          RT_LAUNCH(QP_INST(qp512, k_co_updown), grid_for((std::max(0, n - J - NB) + CO_UD_ROWS - 1) / CO_UD_ROWS), QP_T, lds_ud, V, b, slot, 2, J, r0);
      });
    }
  }
  if (sc.pend_kind == 0 && sc.pend_la != 7) { /* Newton step: d = -(L D L')^{-1} dphi */
    co_chain(bt, b * 16 + 2, [&]() {
      const int SB = CO_SNB, Jlast = ((n - 1) / SB) * SB; /* 64-column blocks */
      for (int J = 0; J < n; J += SB) RT_LAUNCH(QP_INST(qp512, k_co_solve), grid_for((n - J - SB + QP_T - 1) / QP_T), QP_T, lds_solve, V, b, slot, 0, J);
      RT_LAUNCH(QP_INST(qp512, k_co_solve), grid_for((n + QP_T - 1) / QP_T), QP_T, lds_solve, V, b, slot, 1, 0);
      for (int J = Jlast; J >= 0; J -= SB) RT_LAUNCH(QP_INST(qp512, k_co_solve), grid_for((J + 31) / 32), QP_T, lds_solve, V, b, slot, 2, J);
      RT_LAUNCH(QP_INST(qp512, k_co_solve), grid_for((n + QP_T - 1) / QP_T), QP_T, lds_solve, V, b, slot, 3, 0);
    });
  }
  return 0;
}
static int launch_solve_kernel(qpg_batch *bt, const qpg_view &V, int budget, int dynamic, float *ms, int subset);
/* the view a coop batch's kernels run with -- the iteration kernel that suspends, the chains of coop_linear_algebra -- for a whole solve (coop_solve)
 * and for a single operation of the boundary (run_op_coop): where the iteration suspends, the refactorise-or-update rule, and the tables + counter
 * words of the persistent sweep (allocated and cleared at first use) */
static int coop_view(qpg_batch *bt, qpg_view &V) {
  V = bt->V;
  V.offload = bt->sparse ? 1 : (bt->ctx->coop_updates ? 2 : 1); /* sparse coop mode: path updates stay on the QP's workgroup, and so does the one-workgroup path's refactorise-or-update rule */
  /* refactorise-or-update: an update_rank_threshold the user set explicitly wins; else coop_rank_threshold (-2: by measured cost) */
  if (!bt->sparse)
  V.update_rank_threshold = (bt->ctx->update_rank_threshold >= 0) ? bt->ctx->update_rank_threshold
                            : ((bt->ctx->coop_rank_threshold == -2) ? 16 * (bt->nfac / 2048) : bt->ctx->coop_rank_threshold);
  V.co_tab = nullptr; V.co_flags = nullptr; V.co_tab_stride = 0;
  if (!bt->sparse && bt->ctx->coop_updates == 2) { /* tables + counter words of the persistent sweep, per member */
    const size_t stride = ((size_t)bt->nfac / 32 + 2) * CO_UD_TAB(QPG_KMAX), flag_bytes = align_up((size_t)bt->B * 4 * sizeof(int), 256);
    if (!bt->co_tab_d) {
      if (RT_MALLOC(&bt->co_tab_d, flag_bytes + (size_t)bt->B * stride * sizeof(double)) != 0) { bt->co_tab_d = nullptr; return fail(QPG_ERR_ALLOC, "device allocation failed (coop update tables)"); }
      RT_MEMSET(bt->co_tab_d, 0, flag_bytes);
    }
    V.co_flags = (int32_t *)bt->co_tab_d; V.co_tab = (double *)((char *)bt->co_tab_d + flag_bytes); V.co_tab_stride = (int64_t)stride;
  }
  return QPG_OK;
}
static int coop_solve(qpg_batch *bt) {
  qpg_view V;
  { const int rc = coop_view(bt, V); if (rc != QPG_OK) return rc; }
  std::vector<qpg_scalars> sc(bt->B);
  auto t0 = std::chrono::steady_clock::now();
  bt->co_replays = 0; bt->co_sweeps = 0;
  /* QPALM_COOP_PROFILE=1: where one solve's wall time goes (synchronises after every phase; stderr) */
  const bool prof = getenv("QPALM_COOP_PROFILE") != nullptr;
  double t_iter = 0, t_factor = 0, t_solve = 0, t_update = 0; long n_round = 0, n_factor = 0, n_solve = 0, n_update = 0, n_own_update = 0;
  auto now = []() { return std::chrono::steady_clock::now(); };
  auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  bool first = true, finished = false;
  /* the give-up marks of the persistent sweep (flags[1] per member) are consumed by the iteration kernel, which rebuilds the factor when it sees
   * one (dev_solve); every exit path of this function clears whatever is left so that a failed solve cannot poison the next one */
  auto clear_flags = [&]() { if (V.co_flags) RT_MEMSET(V.co_flags, 0, (size_t)bt->B * 4 * sizeof(int)); };
  for (long round = 0; round < 4000000; round++) {
    auto ta = now();
    const int rc = launch_solve_kernel(bt, V, 0x7fffffff, first ? 2 : 0, nullptr);
    first = false;
    if (rc != QPG_OK) { clear_flags(); return rc; }
    RT_MEMCPY_D2H(sc.data(), bt->V.sc, sc.size() * sizeof(qpg_scalars)); /* (the copy waits for the kernels before it) */
    if (RT_STICKY()) { clear_flags(); return api_ok(); }
    if (prof) { t_iter += secs(ta, now()); n_round++; }
    bool all_done = true, any = false;
    for (int b = 0; b < bt->B; b++) {
      if (!sc[b].done) all_done = false;
      if (!sc[b].done && sc[b].pend_stage == 1) {
        any = true;
        if (!prof) { if (bt->B > 1) RT_USE_STREAM(b); coop_linear_algebra(bt, V, b, sc[b]); continue; }
        qpg_scalars part = sc[b];
        const bool fac = part.pend_la == 1 || part.pend_la == 3 || part.pend_la == 7, upd = part.pend_la == 2 || part.pend_la == 4, sol = part.pend_kind == 0 && part.pend_la != 7;
        if (part.pend_la == 0 && part.pend_nchange > 0) n_own_update++;
        if (fac) { qpg_scalars f = part; f.pend_kind = 1; auto tb = now(); coop_linear_algebra(bt, V, b, f); RT_SYNC(); t_factor += secs(tb, now()); n_factor++; }
        if (upd) { qpg_scalars f = part; f.pend_kind = 1; auto tb = now(); coop_linear_algebra(bt, V, b, f); RT_SYNC(); t_update += secs(tb, now()); n_update++; }
        if (sol) { qpg_scalars g = part; g.pend_la = 0; auto tb = now(); coop_linear_algebra(bt, V, b, g); RT_SYNC(); t_solve += secs(tb, now()); n_solve++; }
      }
    }
    RT_USE_STREAM(-1); /* back to the null stream: the next iteration kernel waits for every member's chain */
    if (all_done) { finished = true; break; }
    if (!any) { (void)RT_SYNC(); clear_flags(); return fail(QPG_ERR_RUNTIME, "coop_solve: an unfinished QP did not suspend (internal error)"); }
  }
  if (!finished) { (void)RT_SYNC(); clear_flags(); return fail(QPG_ERR_RUNTIME, "coop_solve: round cap reached with unfinished QPs"); }
  if (RT_SYNC() != 0) { clear_flags(); return fail(QPG_ERR_RUNTIME, "coop kernels failed: " + std::string(RT_LAST_ERROR())); }
  if (V.co_flags) { /* every mark should have been consumed by the iteration kernel (which rebuilt the factor); one that is left belongs to a sweep nobody resumed after */
    std::vector<int> fl((size_t)bt->B * 4);
    RT_MEMCPY_D2H(fl.data(), V.co_flags, fl.size() * sizeof(int));
    for (int b = 0; b < bt->B; b++) if (fl[(size_t)b * 4 + 1] != 0) {
      clear_flags();
      return fail(QPG_ERR_RUNTIME, "coop update sweep: workgroup " + std::to_string(fl[(size_t)b * 4 + 1] - 1) + " of member " + std::to_string(b) + " timed out waiting for a table and no iteration resumed after it");
    }
  }
  bt->last_solve_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (prof)
    fprintf(stderr, "coop profile: %.3f s total; iteration kernel %.3f s in %ld rounds (%ld of them after a one-workgroup update); "
            "factorisations %.3f s / %ld; rank updates %.3f s / %ld; solves %.3f s / %ld; %ld chains replayed as graphs\n", bt->last_solve_ms * 1e-3, t_iter, n_round, n_own_update, t_factor, n_factor, t_update, n_update, t_solve, n_solve, bt->co_replays);
  return api_ok();
}

/* a QP whose previous solve finished starts a new solve (qpalm_solve can be called repeatedly) */
static void rearm(qpg_batch *bt) {
  std::vector<qpg_scalars> sc(bt->B);
  RT_MEMCPY_D2H(sc.data(), bt->V.sc, sc.size() * sizeof(qpg_scalars));
  bool any = false;
  for (auto &s : sc) if (s.done) { s.done = 0; s.in_solve = 0; any = true; }
  if (any) RT_MEMCPY_H2D(bt->V.sc, sc.data(), sc.size() * sizeof(qpg_scalars));
}

/* qpalm_solve can be called again on a finished workspace (src/qpalm.c:401-420 re-initialises its locals): QPs whose
 * previous solve has finished are re-armed.  qpg_batch_solve does this itself; a host that drives the loop with
 * qpg_batch_iterate calls it once per qpalm_solve. */
extern "C" int qpg_batch_begin_solve(qpg_batch *bt) {
  NEED_SETUP(bt, "qpg_batch_begin_solve");
  std::fill(bt->host_status.begin(), bt->host_status.end(), QPG_UNSOLVED); /* qpalm_solve overwrites info->status_val */
  rearm(bt);
  return api_ok();
}

extern "C" int qpg_batch_solve(qpg_batch *bt) {
  NEED_SETUP(bt, "qpg_batch_solve");
  std::fill(bt->host_status.begin(), bt->host_status.end(), QPG_UNSOLVED); /* an error mark of an earlier update_* call ends here, as in the reference */
  if (coop_wanted(bt) || sparse_coop_wanted(bt)) return coop_solve(bt);
  return launch_solve(bt, 0x7fffffff, (bt->B > bt->nslots ? 1 : 0) | 2); /* finished QPs are re-armed on the device */
}

extern "C" int qpg_batch_iterate(qpg_batch *bt, qpg_int k) {
  NEED_SETUP(bt, "qpg_batch_iterate");
  if (bt->B > bt->nslots) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_iterate needs B <= max_slots (one resident factor per QP)");
  if (k <= 0) return api_ok();
  return launch_solve(bt, (int)std::min<qpg_int>(k, 0x7fffffff), 0);
}

extern "C" int qpg_batch_last_solve_ms(qpg_batch *bt, float *ms) {
  NEED_SETUP(bt, "qpg_batch_last_solve_ms");
  if (ms) *ms = bt->last_solve_ms;
  return api_ok();
}

/* Page-locked host memory for the arrays a caller hands over every step (bounds in, solutions out): copies to and from
 * it are DMA transfers at PCIe rate instead of staged pageable copies.  No reference counterpart. */
extern "C" int qpg_host_alloc(qpg_ctx *ctx, size_t bytes, void **out) {
  if (!ctx || !out || bytes == 0) return fail(QPG_ERR_INVALID, "qpg_host_alloc: bad argument");
  *out = nullptr;
  if (RT_HOST_ALLOC(out, bytes) != 0 || !*out) return fail(QPG_ERR_ALLOC, "qpg_host_alloc: allocation failed");
  memset(*out, 0, bytes);
  return api_ok();
}
extern "C" int qpg_host_free(qpg_ctx *ctx, void *p) {
  if (!ctx) return fail(QPG_ERR_INVALID, "qpg_host_free: NULL context");
  if (p) RT_HOST_FREE(p);
  return api_ok();
}

extern "C" int qpg_batch_launch_shape(qpg_batch *bt, qpg_int *workgroups, qpg_int *threads, qpg_int *lds_bytes) {
  if (!bt) return fail(QPG_ERR_INVALID, "qpg_batch_launch_shape: NULL batch");
  if (workgroups) *workgroups = bt->nslots;
  if (threads) *threads = bt->threads;
  if (lds_bytes) *lds_bytes = bt->lds_bytes;
  return api_ok();
}

extern "C" int qpg_batch_num_unfinished(qpg_batch *bt, qpg_int *count) {
  NEED_SETUP(bt, "qpg_batch_num_unfinished");
  std::vector<qpg_scalars> sc(bt->B);
  RT_MEMCPY_D2H(sc.data(), bt->V.sc, sc.size() * sizeof(qpg_scalars));
  qpg_int c = 0;
  for (auto &s : sc) c += s.done ? 0 : 1;
  *count = c;
  return api_ok();
}

static const char *status_string(int v) { /* src/util.c:61-105 */
  switch (v) {
    case QPG_SOLVED: return "solved";
    case QPG_DUAL_TERMINATED: return "dual terminated";
    case QPG_PRIMAL_INFEASIBLE: return "primal infeasible";
    case QPG_DUAL_INFEASIBLE: return "dual infeasible";
    case QPG_TIME_LIMIT_REACHED: return "time limit exceeded";
    case QPG_MAX_ITER_REACHED: return "maximum iterations reached";
    case QPG_UNSOLVED: return "unsolved";
    case QPG_ERROR: return "error";
    default: return "unrecognised status value";
  }
}

static void fill_info(qpg_batch *bt, qpg_int idx, const qpg_scalars &s, QPGInfo *out) {
  memset(out, 0, sizeof(*out));
  out->iter = s.iter; out->iter_out = s.iter_out;
  int sv = s.status;
  if (bt->host_status[idx] == QPG_ERROR) sv = QPG_ERROR;
  out->status_val = sv;
  strncpy(out->status, status_string(sv), sizeof(out->status) - 1);
  out->pri_res_norm = s.pri_res_norm; out->dua_res_norm = s.dua_res_norm; out->dua2_res_norm = s.dua2_res_norm;
  out->objective = s.objective; out->dual_objective = s.dual_objective;
  out->setup_time = s.setup_time; out->solve_time = s.solve_time; out->run_time = s.setup_time + s.solve_time;
}
static void fill_stats(const qpg_scalars &s, QPGStats *out);

extern "C" int qpg_batch_get_info(qpg_batch *bt, qpg_int idx, QPGInfo *out) {
  NEED_SETUP(bt, "qpg_batch_get_info");
  if (idx < 0 || idx >= bt->B || !out) return fail(QPG_ERR_INVALID, "qpg_batch_get_info: bad argument");
  qpg_scalars s;
  RT_MEMCPY_D2H(&s, bt->V.sc + idx, sizeof(s));
  fill_info(bt, idx, s, out);
  return api_ok();
}

/* every QP's QPALMInfo / work counters in one device-to-host copy ([B] records) */
extern "C" int qpg_batch_get_info_all(qpg_batch *bt, QPGInfo *out) {
  NEED_SETUP(bt, "qpg_batch_get_info_all");
  if (!out) return fail(QPG_ERR_INVALID, "qpg_batch_get_info_all: NULL");
  std::vector<qpg_scalars> sc(bt->B);
  RT_MEMCPY_D2H(sc.data(), bt->V.sc, sc.size() * sizeof(qpg_scalars));
  for (int b = 0; b < bt->B; b++) fill_info(bt, b, sc[b], out + b);
  return api_ok();
}
extern "C" int qpg_batch_get_stats_all(qpg_batch *bt, QPGStats *out) {
  NEED_SETUP(bt, "qpg_batch_get_stats_all");
  if (!out) return fail(QPG_ERR_INVALID, "qpg_batch_get_stats_all: NULL");
  std::vector<qpg_scalars> sc(bt->B);
  RT_MEMCPY_D2H(sc.data(), bt->V.sc, sc.size() * sizeof(qpg_scalars));
  for (int b = 0; b < bt->B; b++) fill_stats(sc[b], out + b);
  return api_ok();
}

extern "C" int qpg_batch_get_stats(qpg_batch *bt, qpg_int idx, QPGStats *out) {
  NEED_SETUP(bt, "qpg_batch_get_stats");
  if (idx < 0 || idx >= bt->B || !out) return fail(QPG_ERR_INVALID, "qpg_batch_get_stats: bad argument");
  qpg_scalars s;
  RT_MEMCPY_D2H(&s, bt->V.sc + idx, sizeof(s));
  fill_stats(s, out);
  return api_ok();
}
static void fill_stats(const qpg_scalars &s, QPGStats *out) {
  out->n_refactor = s.n_refactor; out->n_factor_Q = s.n_factor_Q; out->n_sweeps = s.n_sweeps; out->n_rank1 = s.n_rank1;
  out->n_solve = s.n_solve; out->n_sigma_updates = s.n_sigma_updates; out->n_boost_gamma = s.n_boost_gamma;
  out->nb_active = s.nb_active; out->nb_enter = s.nb_enter; out->nb_leave = s.nb_leave; out->last_kind = s.last_kind; out->last_fact = s.last_fact;
  out->gamma = s.gamma; out->tau = s.tau; out->eta = s.eta; out->beta = s.beta; out->eps_pri = s.eps_pri; out->eps_dua = s.eps_dua;
  out->eps_dua_in = s.eps_dua_in; out->sc_c = s.sc_c;
  out->ms_total = s.ticks_total * 1e-5; out->ms_factor = s.ticks_factor * 1e-5; out->ms_update = s.ticks_update * 1e-5;
  out->ms_solve = s.ticks_solve * 1e-5; out->ms_linesearch = s.ticks_linesearch * 1e-5;
  for (int k = 0; k < 16; k++) out->ms_dbg[k] = s.ticks_dbg[k] * 1e-5;
  out->sweep_entries = s.ticks_dbg[QPG_CNT_SWEEP_ENTRIES]; out->factor_reread_entries = s.ticks_dbg[QPG_CNT_FACTOR_REREAD];
  out->placement = s.ticks_dbg[QPG_CNT_PLACEMENT]; out->lobpcg_lambda = s.lobpcg_lambda; out->lobpcg_iter = s.lobpcg_iter; out->nonconvex = s.nc_flag;
  out->n_fused_solve = s.n_fused_solve;
  out->n_seq_columns = s.ticks_dbg[QPG_CNT_SEQ_COLS]; out->n_sweep_columns = s.ticks_dbg[QPG_CNT_SWEEP_COLS]; out->n_guard_refactor = s.n_guard_refactor;
}

extern "C" int qpg_batch_get_solution(qpg_batch *bt, qpg_float *x, qpg_float *y) {
  NEED_SETUP(bt, "qpg_batch_get_solution");
  if (x) RT_MEMCPY_D2H(x, bt->V.sol_x, (size_t)bt->B * bt->n * sizeof(double));
  if (y) RT_MEMCPY_D2H(y, bt->V.sol_y, (size_t)bt->B * bt->m * sizeof(double));
  return api_ok();
}
/* ... into arrays in device memory: a kernel writes them */
static int solution_to_device(qpg_batch *bt, qpg_float *d_x, qpg_float *d_y, const Subset &sub) {
  if (!d_x && !d_y) return api_ok();
  BT_LAUNCH(bt, k_get_solution, sub.blocks(bt), 0, bt->V, (double *)d_x, (double *)d_y, sub.list);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_get_solution failed: " + std::string(RT_LAST_ERROR()));
  return api_ok();
}
extern "C" int qpg_batch_get_solution_device(qpg_batch *bt, qpg_float *d_x, qpg_float *d_y) {
  NEED_SETUP(bt, "qpg_batch_get_solution_device");
  return solution_to_device(bt, d_x, d_y, Subset());
}
/* info->status_val / info->iter of every QP into [B] arrays in device memory.  The QPG_ERROR marks of refused updates live on the host
 * (host_status): while there are any, they go to the device as one flag per member (the line-search scratch is idle between solves).
 * flags_in (device, [B] ints) / flags_out: see k_get_status */
static int status_to_device(qpg_batch *bt, qpg_int *d_status_val, qpg_int *d_iter, const int *flags_in, qpg_int *flags_out, const Subset &sub = Subset()) {
  if (!d_status_val && !d_iter && !flags_out) return api_ok();
  const int *err_d = nullptr;
  if (d_status_val && std::find(bt->host_status.begin(), bt->host_status.end(), (int)QPG_ERROR) != bt->host_status.end()) {
    std::vector<int> err((size_t)bt->B);
    for (int b = 0; b < bt->B; b++) err[b] = bt->host_status[b] == QPG_ERROR ? 1 : 0;
    int *scratch = (int *)bt->V.ls_idx + bt->B; /* (behind the flags of k_update_bounds: [B][ls_stride] ints, ls_stride >= 2) */
    RT_MEMCPY_H2D(scratch, err.data(), err.size() * sizeof(int));
    err_d = scratch;
  }
  BT_LAUNCH(bt, k_get_status, (sub.count(bt) + bt->threads - 1) / bt->threads, 0, bt->V, err_d, (int64_t *)d_status_val, (int64_t *)d_iter, flags_in, (int64_t *)flags_out, sub.list);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_get_status failed: " + std::string(RT_LAST_ERROR()));
  return api_ok();
}
extern "C" int qpg_batch_get_status_device(qpg_batch *bt, qpg_int *d_status_val, qpg_int *d_iter) {
  NEED_SETUP(bt, "qpg_batch_get_status_device");
  return status_to_device(bt, d_status_val, d_iter, nullptr, nullptr);
}

static int vec_lookup(qpg_batch *bt, const char *name, qpg_int idx, size_t elem, char **ptr, size_t *count) {
  void *p; size_t bytes;
  if (!find_named(bt, name, &p, &bytes)) return 0;
  const size_t per = bytes / elem / bt->B;
  *ptr = (char *)p + (size_t)idx * per * elem; *count = per;
  return 1;
}

extern "C" int qpg_batch_get_vector(qpg_batch *bt, const char *name, qpg_int idx, qpg_float *out, qpg_int len) {
  NEED_SETUP(bt, "qpg_batch_get_vector");
  char *p; size_t cnt;
  if (idx < 0 || idx >= bt->B || !vec_lookup(bt, name, idx, sizeof(double), &p, &cnt)) return fail(QPG_ERR_INVALID, std::string("unknown vector ") + name);
  if ((size_t)len > cnt) return fail(QPG_ERR_INVALID, "qpg_batch_get_vector: len too large");
  RT_MEMCPY_D2H(out, p, (size_t)len * sizeof(double));
  return api_ok();
}
extern "C" int qpg_batch_set_vector(qpg_batch *bt, const char *name, qpg_int idx, const qpg_float *in, qpg_int len) {
  NEED_SETUP(bt, "qpg_batch_set_vector");
  char *p; size_t cnt;
  if (idx < 0 || idx >= bt->B || !vec_lookup(bt, name, idx, sizeof(double), &p, &cnt)) return fail(QPG_ERR_INVALID, std::string("unknown vector ") + name);
  if ((size_t)len > cnt) return fail(QPG_ERR_INVALID, "qpg_batch_set_vector: len too large");
  RT_MEMCPY_H2D(p, in, (size_t)len * sizeof(double));
  return api_ok();
}
extern "C" int qpg_batch_get_ivector(qpg_batch *bt, const char *name, qpg_int idx, qpg_int *out, qpg_int len) {
  NEED_SETUP(bt, "qpg_batch_get_ivector");
  char *p; size_t cnt;
  if (idx < 0 || idx >= bt->B || !vec_lookup(bt, name, idx, sizeof(int), &p, &cnt)) return fail(QPG_ERR_INVALID, std::string("unknown vector ") + name);
  if ((size_t)len > cnt) return fail(QPG_ERR_INVALID, "qpg_batch_get_ivector: len too large");
  std::vector<int> tmp(len);
  RT_MEMCPY_D2H(tmp.data(), p, (size_t)len * sizeof(int));
  for (qpg_int k = 0; k < len; k++) out[k] = tmp[k];
  return api_ok();
}
extern "C" int qpg_batch_set_ivector(qpg_batch *bt, const char *name, qpg_int idx, const qpg_int *in, qpg_int len) {
  NEED_SETUP(bt, "qpg_batch_set_ivector");
  char *p; size_t cnt;
  if (idx < 0 || idx >= bt->B || !vec_lookup(bt, name, idx, sizeof(int), &p, &cnt)) return fail(QPG_ERR_INVALID, std::string("unknown vector ") + name);
  if ((size_t)len > cnt) return fail(QPG_ERR_INVALID, "qpg_batch_set_ivector: len too large");
  std::vector<int> tmp(len);
  for (qpg_int k = 0; k < len; k++) tmp[k] = (int)in[k];
  RT_MEMCPY_H2D(p, tmp.data(), (size_t)len * sizeof(int));
  return api_ok();
}

extern "C" int qpg_batch_set_scalar(qpg_batch *bt, const char *name, qpg_int idx, qpg_float v) {
  NEED_SETUP(bt, "qpg_batch_set_scalar");
  if (idx < 0 || idx >= bt->B) return fail(QPG_ERR_INVALID, "qpg_batch_set_scalar: bad index");
  qpg_scalars s;
  RT_MEMCPY_D2H(&s, bt->V.sc + idx, sizeof(s));
  if (!strcmp(name, "gamma")) s.gamma = v;
  else if (!strcmp(name, "tau")) s.tau = v;
  else if (!strcmp(name, "nb_enter")) s.nb_enter = (int)v;
  else if (!strcmp(name, "nb_leave")) s.nb_leave = (int)v;
  else if (!strcmp(name, "nb_active")) s.nb_active = (int)v;
  else if (!strcmp(name, "nb_sigma_changed")) s.nb_sigma_changed = (int)v;
  else if (!strcmp(name, "reset_newton")) s.reset_newton = (int)v;
  else if (!strcmp(name, "proximal")) { /* per-batch setting; the reference's tests flip it on the workspace */
    bt->settings.proximal = (qpg_int)v;
    qpg_settings st; memcpy(&st, &bt->settings, sizeof(st));
    RT_MEMCPY_H2D(bt->V.settings, &st, sizeof(st));
    return api_ok();
  } else return fail(QPG_ERR_INVALID, std::string("unknown scalar ") + name);
  RT_MEMCPY_H2D(bt->V.sc + idx, &s, sizeof(s));
  return api_ok();
}

static int run_op(qpg_batch *bt, qpg_int idx, int op, const char *fn);
extern "C" int qpg_batch_get_factor(qpg_batch *bt, qpg_int idx, qpg_float *Lout, qpg_float *Dout, qpg_int n) {
  NEED_SETUP(bt, "qpg_batch_get_factor");
  if (bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_get_factor: works on the dense factor (this batch keeps a sparse L D L')");
  if (idx < 0 || idx >= bt->nslots || n != bt->nfac) return fail(QPG_ERR_INVALID, "qpg_batch_get_factor: bad argument (n = rows of the factor: n, or n + m in KKT mode)");
  if (bt->kkt && bt->B > bt->nslots) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_get_factor: in KKT mode a slot belongs to a QP only while B <= max_slots"); /* (kkt_na / kkt_list of QP idx describe slot idx only then) */
  if (bt->kkt && idx < bt->B) { /* the solver keeps the KKT factor compact (active rows only) until somebody needs the full layout */
    const int rc = run_op(bt, idx, QP_OP_KKT_EXPAND, "qpg_batch_get_factor");
    if (rc != QPG_OK) return rc;
  }
  std::vector<double> tmp((size_t)bt->ld * bt->nfac);
  RT_MEMCPY_D2H(tmp.data(), bt->V.L + (size_t)idx * bt->ld * bt->nfac, tmp.size() * sizeof(double));
  for (int j = 0; j < bt->nfac; j++) for (int i = 0; i < bt->nfac; i++) Lout[(size_t)j * n + i] = (i > j) ? tmp[(size_t)j * bt->ld + i] : (i == j ? 1.0 : 0.0);
  RT_MEMCPY_D2H(Dout, bt->V.Dg + (size_t)idx * bt->nfac, (size_t)bt->nfac * sizeof(double));
  return api_ok();
}

extern "C" int qpg_batch_device_ptr(qpg_batch *bt, const char *name, void **ptr, size_t *bytes) {
  NEED_SETUP(bt, "qpg_batch_device_ptr");
  if (!find_named(bt, name, ptr, bytes)) return fail(QPG_ERR_INVALID, std::string("unknown array ") + name);
  return api_ok();
}
extern "C" int qpg_batch_sync(qpg_batch *bt) { (void)bt; return RT_SYNC() == 0 ? QPG_OK : fail(QPG_ERR_RUNTIME, RT_LAST_ERROR()); }

extern "C" int qpg_batch_update_settings(qpg_batch *bt, const QPGSettings *s) { /* src/qpalm.c:739-791 */
  NEED_SETUP(bt, "qpg_batch_update_settings");
  auto mark_error = [&]() { std::fill(bt->host_status.begin(), bt->host_status.end(), QPG_ERROR); };
  if (!qpg_validate_settings(s)) { mark_error(); return fail(QPG_ERR_INVALID, "Settings validation returned failure"); }
  if (bt->settings.scaling > s->scaling) { mark_error(); return fail(QPG_ERR_INVALID, "Decreasing the number of scaling iterations is not allowed"); }
  if ((s->nonconvex != 0) != (bt->settings.nonconvex != 0))
    return fail(QPG_ERR_UNSUPPORTED, "nonconvex is fixed at setup (set_settings_nonconvex runs in qpalm_setup, qpalm.c:293-296)");
  if (((s->factorization_method == 0) ? 1 : 0) != bt->kkt)
    return fail(QPG_ERR_UNSUPPORTED, "factorization_method is fixed at setup (qpalm_set_factorization_method runs in qpalm_setup, qpalm.c:196)");
  if (bt->kkt && bt->sparse && s->enable_dual_termination)
    return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_update_settings: the sparse KKT factor does not support enable_dual_termination (no LD_Q on the pattern of K)");
  const int extra = (int)(s->scaling - bt->settings.scaling);
  bt->settings = *s;
  if (ensure_dual_slots(bt) != 0) return fail(QPG_ERR_ALLOC, "device allocation failed (LD_Q slots)");
  qpg_settings st; memcpy(&st, &bt->settings, sizeof(st));
  RT_MEMCPY_H2D(bt->V.settings, &st, sizeof(st));
  if (extra > 0) {
    BT_LAUNCH(bt, k_setup, blocks_for(bt), 0, bt->V, extra, 1);
    if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_setup (rescale) failed: " + std::string(RT_LAST_ERROR()));
  }
  return api_ok();
}

/* The record of the raw q / bounds (see qpg_batch).  raw_need_host: raw_h is current afterwards -- created from the slab, or fetched from the
 * device mirror where a device-form update was the last to write; raw_need_device: the same for raw_d.  The caller then sets raw_cur to the side
 * it writes. */
static void raw_need_host(qpg_batch *bt) {
  const size_t B = bt->B, n = bt->n, m = bt->m;
  if (bt->raw_cur == 1) {
    bt->raw_h.resize(B * (n + 2 * m));
    RT_MEMCPY_D2H(bt->raw_h.data(), bt->raw_d, bt->raw_h.size() * sizeof(double));
    bt->raw_cur = 2;
  }
  if (!bt->raw_h.empty()) return;
  bt->raw_h.resize(B * (n + 2 * m));
  memcpy(bt->raw_q(), bt->harr<double>(H_Q, 0), B * n * sizeof(double));
  memcpy(bt->raw_bmin(), bt->harr<double>(H_BMIN, 0), B * m * sizeof(double));
  memcpy(bt->raw_bmax(), bt->harr<double>(H_BMAX, 0), B * m * sizeof(double));
}
static int raw_need_device(qpg_batch *bt) {
  const size_t B = bt->B, n = bt->n, m = bt->m;
  if (!bt->raw_d && RT_MALLOC(&bt->raw_d, B * (n + 2 * m) * sizeof(double)) != 0) { bt->raw_d = nullptr; return 1; }
  if (bt->raw_cur >= 1) return 0;
  if (!bt->raw_h.empty()) RT_MEMCPY_H2D(bt->raw_d, bt->raw_h.data(), bt->raw_h.size() * sizeof(double));
  else { /* nothing updated since the setup: the slab's arrays */
    RT_MEMCPY_H2D(bt->raw_d_q(), bt->harr<double>(H_Q, 0), B * n * sizeof(double));
    if (m > 0) {
      RT_MEMCPY_H2D(bt->raw_d_bmin(), bt->harr<double>(H_BMIN, 0), B * m * sizeof(double));
      RT_MEMCPY_H2D(bt->raw_d_bmax(), bt->harr<double>(H_BMAX, 0), B * m * sizeof(double));
    }
  }
  return 0;
}

/* after k_update_bounds: the flags come back (one int per member), refused members are marked QPG_ERROR until the next solve */
/* subset: the kernel wrote the flags of the listed members into zeroed scratch; a member that is not listed keeps its mark */
static int bounds_flags(qpg_batch *bt, const int *bad_d, std::vector<int> &bad, bool subset = false) {
  bad.assign((size_t)bt->B, 0);
  RT_MEMCPY_D2H(bad.data(), bad_d, bad.size() * sizeof(int));
  int nbad = 0;
  for (size_t b = 0; b < bad.size(); b++) {
    if (bad[b]) { bt->host_status[b] = QPG_ERROR; nbad++; }
    else if (!subset && bt->host_status[b] == QPG_ERROR) bt->host_status[b] = QPG_UNSOLVED; /* valid bounds now: qpalm_solve overwrites the status (qpalm.c:401-420) */
  }
  return nbad;
}

extern "C" int qpg_batch_update_bounds(qpg_batch *bt, const qpg_float *bmin, const qpg_float *bmax) { /* qpalm.c:793-827 */
  NEED_SETUP(bt, "qpg_batch_update_bounds");
  const size_t B = bt->B, m = bt->m, ls = (size_t)bt->ls_stride;
  /* the raw bounds go to the line-search scratch of each QP (one strided copy per array); validation, scaling and the
   * copy into place happen on the device (no pass over the B x m values on the host) */
  if (m > 0) {
    if (bmin) RT_MEMCPY2D_H2D(bt->V.ls_key, ls * sizeof(double), bmin, m * sizeof(double), m * sizeof(double), B);
    if (bmax) RT_MEMCPY2D_H2D(bt->V.ls_key + m, ls * sizeof(double), bmax, m * sizeof(double), m * sizeof(double), B);
  }
  int *bad_d = (int *)bt->V.ls_idx; /* scratch: one flag per QP */
  BT_LAUNCH(bt, k_update_bounds, blocks_for(bt), 0, bt->V, bmin ? 1 : 0, bmax ? 1 : 0, bad_d, (const double *)bt->V.ls_key, (const double *)(bt->V.ls_key + m),
            (long long)ls, (double *)nullptr, (double *)nullptr, (const int32_t *)nullptr);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_update_bounds failed: " + std::string(RT_LAST_ERROR()));
  std::vector<int> bad;
  const int nbad = bounds_flags(bt, bad_d, bad);
  raw_need_host(bt);
  bt->raw_cur = 0;
  for (size_t b = 0; b < B; b++)
    if (!bad[b] && m > 0) { /* accepted: the member's raw bounds from now on (qpg_batch_update_Q_A) */
      if (bmin) memcpy(bt->raw_bmin() + b * m, bmin + b * m, m * sizeof(double));
      if (bmax) memcpy(bt->raw_bmax() + b * m, bmax + b * m, m * sizeof(double));
    }
  if (nbad) return fail(QPG_ERR_INVALID, "Lower bound greater than upper bound");
  return api_ok();
}
/* ... with the bounds already in device memory: the kernel reads the caller's arrays and keeps the record of the accepted raw values in
 * the device mirror; only the flags (one int per member) come back.  rejected (device, [B], or NULL): the flags for the caller */
static int update_bounds_device(qpg_batch *bt, const qpg_float *d_bmin, const qpg_float *d_bmax, qpg_int *rejected, const Subset &sub = Subset()) {
  if (raw_need_device(bt) != 0) return fail(QPG_ERR_ALLOC, "device allocation failed (record of the raw q and bounds)"); /* (a current host-side record comes over whole) */
  int *bad_d = (int *)bt->V.ls_idx;
  if (sub.list) RT_MEMSET(bad_d, 0, (size_t)bt->B * sizeof(int));
  BT_LAUNCH(bt, k_update_bounds, sub.blocks(bt), 0, bt->V, d_bmin ? 1 : 0, d_bmax ? 1 : 0, bad_d, (const double *)d_bmin, (const double *)d_bmax,
            (long long)bt->m, bt->raw_d_bmin(), bt->raw_d_bmax(), sub.list);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_update_bounds failed: " + std::string(RT_LAST_ERROR()));
  bt->raw_cur = 1;
  std::vector<int> bad;
  const int nbad = bounds_flags(bt, bad_d, bad, sub.list != nullptr);
  if (rejected) {
    const int rc = status_to_device(bt, nullptr, nullptr, bad_d, rejected, sub);
    if (rc != QPG_OK) return rc;
  }
  if (nbad) return fail(QPG_ERR_INVALID, "Lower bound greater than upper bound");
  return api_ok();
}
extern "C" int qpg_batch_update_bounds_device(qpg_batch *bt, const qpg_float *d_bmin, const qpg_float *d_bmax) {
  NEED_SETUP(bt, "qpg_batch_update_bounds_device");
  return update_bounds_device(bt, d_bmin, d_bmax, nullptr);
}

extern "C" int qpg_batch_update_q(qpg_batch *bt, const qpg_float *q) { /* qpalm.c:829-871 */
  NEED_SETUP(bt, "qpg_batch_update_q");
  if (!q) return fail(QPG_ERR_INVALID, "qpg_batch_update_q: NULL");
  RT_MEMCPY_H2D(bt->V.q, q, (size_t)bt->B * bt->n * sizeof(double));
  BT_LAUNCH(bt, k_update_q, blocks_for(bt), 0, bt->V, (const double *)nullptr, (double *)nullptr, (const int32_t *)nullptr);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_update_q failed: " + std::string(RT_LAST_ERROR()));
  raw_need_host(bt);
  bt->raw_cur = 0;
  memcpy(bt->raw_q(), q, (size_t)bt->B * bt->n * sizeof(double));
  return api_ok();
}
static int update_q_device(qpg_batch *bt, const qpg_float *d_q, const Subset &sub) {
  if (raw_need_device(bt) != 0) return fail(QPG_ERR_ALLOC, "device allocation failed (record of the raw q and bounds)"); /* (a current host-side record comes over whole) */
  BT_LAUNCH(bt, k_update_q, sub.blocks(bt), 0, bt->V, (const double *)d_q, bt->raw_d_q(), sub.list);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_update_q failed: " + std::string(RT_LAST_ERROR()));
  bt->raw_cur = 1;
  return api_ok();
}
extern "C" int qpg_batch_update_q_device(qpg_batch *bt, const qpg_float *d_q) {
  NEED_SETUP(bt, "qpg_batch_update_q_device");
  if (!d_q) return fail(QPG_ERR_INVALID, "qpg_batch_update_q_device: NULL");
  return update_q_device(bt, d_q, Subset());
}

/* The maps between the device's order of the entries of A / Q and the caller's (qpg_batch::map_A / map_Q), in device memory: uploaded at the first call
 * that needs them.  All three stay NULL when every member was given in the device's order. */
static int value_maps_device(qpg_batch *bt, int32_t **mapA_d, int32_t **mapQ_d, int32_t **same_d) {
  const size_t B = bt->B, zA = bt->nnzA, zQ = bt->nnzQ;
  *mapA_d = *mapQ_d = *same_d = nullptr;
  bool any_map = false;
  for (size_t b = 0; b < B && !any_map; b++) any_map = !bt->map_A[b].empty() || !bt->map_Q[b].empty();
  if (!any_map) return QPG_OK;
  const size_t oQ = align_up(B * zA * 4, 256), oS = oQ + align_up(B * zQ * 4, 256), bytes = oS + B * 2 * 4;
  if (!bt->val_maps_d && RT_MALLOC(&bt->val_maps_d, bytes) != 0) { bt->val_maps_d = nullptr; return fail(QPG_ERR_ALLOC, "device allocation failed (value maps)"); }
  *mapA_d = (int32_t *)bt->val_maps_d; *mapQ_d = (int32_t *)((char *)bt->val_maps_d + oQ); *same_d = (int32_t *)((char *)bt->val_maps_d + oS);
  if (!bt->val_maps_current) {
    std::vector<int32_t> same(B * 2);
    for (size_t b = 0; b < B; b++) {
      same[2 * b] = bt->map_A[b].empty() ? 1 : 0; same[2 * b + 1] = bt->map_Q[b].empty() ? 1 : 0;
      if (!same[2 * b]) RT_MEMCPY_H2D(*mapA_d + b * zA, bt->map_A[b].data(), bt->map_A[b].size() * 4);
      if (!same[2 * b + 1]) RT_MEMCPY_H2D(*mapQ_d + b * zQ, bt->map_Q[b].data(), bt->map_Q[b].size() * 4);
    }
    RT_MEMCPY_H2D(*same_d, same.data(), same.size() * 4);
    bt->val_maps_current = true;
  }
  return QPG_OK;
}

/* qpalm_update_Q_A for every member: new values of Q and A on the patterns the batch was set up with.  Afterwards the batch is what qpg_batch_setup
 * would leave for these values, the latest accepted raw q / bounds and the current settings -- without the host-side conversion, the symbolic
 * analysis of the sparse factors, the pattern uploads or a new arena.  Kept: the arena, the factor and LD_Q slots, nq / mq, the settings block, the
 * sparse symbolic state (sparse_adj_* / sparse_analyze read patterns only: an entry whose new value is 0 stays an entry), the stored solutions and the
 * recorded coop launch chains (they hold pointers and sizes, no values).  dQx / dAx: device arrays [B][nnzQ_max] / [B][nnzA_max] in the caller's
 * order of qpg_batch_set_problem*; strideQ / strideA: doubles between two members in them. */
static int update_Q_A_device(qpg_batch *bt, const double *dQx, size_t strideQ, const double *dAx, size_t strideA) {
  qpg_view &V = bt->V;
  const size_t B = bt->B, n = bt->n, m = bt->m;
  int32_t *mapA_d = nullptr, *mapQ_d = nullptr, *same_d = nullptr;
  { const int rcm = value_maps_device(bt, &mapA_d, &mapQ_d, &same_d); if (rcm != QPG_OK) return rcm; }
  /* the raw q and bounds a fresh setup would upload */
  if (bt->raw_cur == 1) raw_need_host(bt); /* the device forms of the updates wrote last: their record comes over (one transfer) */
  const bool rec = !bt->raw_h.empty();
  RT_MEMCPY_H2D(V.q, rec ? bt->raw_q() : bt->harr<double>(H_Q, 0), B * n * sizeof(double));
  if (m > 0) {
    RT_MEMCPY_H2D(V.bmin, rec ? bt->raw_bmin() : bt->harr<double>(H_BMIN, 0), B * m * sizeof(double));
    RT_MEMCPY_H2D(V.bmax, rec ? bt->raw_bmax() : bt->harr<double>(H_BMAX, 0), B * m * sizeof(double));
  }
  BT_LAUNCH(bt, k_update_Q_A, blocks_for(bt), 0, V, dQx, (long long)strideQ, dAx, (long long)strideA, (const int32_t *)mapQ_d, (const int32_t *)mapA_d,
            (const int32_t *)same_d, setup_scalars(bt), (int)bt->settings.scaling);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_update_Q_A failed: " + std::string(RT_LAST_ERROR()));
  if (bt->settings.nonconvex) {
    const int rcl = run_lobpcg(bt);
    if (rcl != QPG_OK) return rcl;
  }
  std::fill(bt->host_status.begin(), bt->host_status.end(), QPG_UNSOLVED);
  return api_ok();
}
extern "C" int qpg_batch_update_Q_A_device(qpg_batch *bt, const qpg_float *dQx, const qpg_float *dAx) {
  NEED_SETUP(bt, "qpg_batch_update_Q_A_device");
  if (!dQx || !dAx) return fail(QPG_ERR_INVALID, "qpg_batch_update_Q_A_device: NULL");
  return update_Q_A_device(bt, dQx, (size_t)bt->nnzQ_in, dAx, (size_t)bt->nnzA_in);
}
extern "C" int qpg_batch_update_Q_A(qpg_batch *bt, const qpg_float *Qx, const qpg_float *Ax) {
  NEED_SETUP(bt, "qpg_batch_update_Q_A");
  if (!Qx || !Ax) return fail(QPG_ERR_INVALID, "qpg_batch_update_Q_A: NULL");
  /* staged in the arrays of derived values, which the kernel rebuilds after it has read them: A's values where the member's A' values go, Q's at the
   * start of the member's full-Q values (a stride of 2 nnzQ: no workgroup writes where another still reads) */
  const size_t B = bt->B;
  if (bt->nnzA_in > 0) RT_MEMCPY_H2D(bt->V.Atx, Ax, B * (size_t)bt->nnzA_in * sizeof(double));
  if (bt->nnzQ_in > 0) RT_MEMCPY2D_H2D(bt->V.Qfx, (size_t)bt->nnzQf * sizeof(double), Qx, (size_t)bt->nnzQ_in * sizeof(double), (size_t)bt->nnzQ_in * sizeof(double), B);
  return update_Q_A_device(bt, bt->V.Qfx, (size_t)bt->nnzQf, bt->V.Atx, (size_t)bt->nnzA);
}

/* One receding-horizon step on arrays in device memory: update_bounds -> update_q -> warm start -> solve -> get_solution -> get_status, each the
 * device form above (or qpg_batch_warm_start_last / qpg_batch_solve).  A refused member (bmin > bmax) keeps its bounds and solves on them; the call
 * then returns QPG_ERR_INVALID after the whole step has run.  Any other error ends the step where it occurs. */
static int step_args(const QPGDeviceStep *io, const std::string &fn) {
  if (!io) return fail(QPG_ERR_INVALID, fn + ": NULL");
  if (io->warm < 0 || io->warm > 2) return fail(QPG_ERR_INVALID, fn + ": warm must be 0, 1 or 2");
  if (io->warm == 2 && !io->warm_x && !io->warm_y) return fail(QPG_ERR_INVALID, fn + ": warm = 2 needs warm_x or warm_y");
  return QPG_OK;
}
/* qpg_batch_solve for the listed members: a fresh solve through the work queue on the list k_select left.  The error marks of the listed members end
 * here, as those of every member do in qpg_batch_solve (the list comes over only while there are marks) */
static int solve_subset(qpg_batch *bt, const Subset &sub) {
  if (std::find(bt->host_status.begin(), bt->host_status.end(), (int)QPG_ERROR) != bt->host_status.end()) {
    std::vector<int32_t> members((size_t)sub.S);
    RT_MEMCPY_D2H(members.data(), sub.list, members.size() * sizeof(int32_t));
    for (int32_t b : members) if (b >= 0 && b < bt->B) bt->host_status[b] = QPG_UNSOLVED;
  }
  return launch_solve(bt, 0x7fffffff, 1 | 2, sub.S);
}
static int step_run(qpg_batch *bt, const QPGDeviceStep *io, const Subset &sub) {
  int rc, refused = 0;
  if (io->bmin || io->bmax) {
    rc = update_bounds_device(bt, io->bmin, io->bmax, io->rejected, sub);
    if (rc == QPG_ERR_INVALID) refused = 1;
    else if (rc != QPG_OK) return rc;
  } else if (io->rejected) {
    if ((rc = status_to_device(bt, nullptr, nullptr, nullptr, io->rejected, sub)) != QPG_OK) return rc;
  }
  if (io->q && (rc = update_q_device(bt, io->q, sub)) != QPG_OK) return rc;
  if (io->warm == 1 && (rc = warm_start_launch(bt, 2, 2, nullptr, nullptr, sub)) != QPG_OK) return rc;
  if (io->warm == 2 && (rc = warm_start_launch(bt, io->warm_x ? 1 : 0, io->warm_y ? 1 : 0, io->warm_x, io->warm_y, sub)) != QPG_OK) return rc;
  if ((rc = sub.list ? solve_subset(bt, sub) : qpg_batch_solve(bt)) != QPG_OK) return rc;
  if ((rc = solution_to_device(bt, io->x, io->y, sub)) != QPG_OK) return rc;
  if ((rc = status_to_device(bt, io->status_val, io->iter, nullptr, nullptr, sub)) != QPG_OK) return rc;
  if (refused) return fail(QPG_ERR_INVALID, "Lower bound greater than upper bound");
  return api_ok();
}
extern "C" int qpg_batch_step_device(qpg_batch *bt, const QPGDeviceStep *io) {
  NEED_SETUP(bt, "qpg_batch_step_device");
  { const int rc = step_args(io, "qpg_batch_step_device"); if (rc != QPG_OK) return rc; }
  return step_run(bt, io, Subset());
}

/* ---- subsets (DESIGN.md section 15): `d_select` ([B] qpg_int in device memory, entries 0 / 1) -> the work list of one call, in V.order (k_select).
 * What comes back: S, and the two flags of the queue block -- one read of three words.  Refused before anything of the batch has changed: more
 * than 2^17 members (the counting is quadratic, as k_queue_order's), an entry other than 0 / 1, a solve in progress. */
static int select_members(qpg_batch *bt, const std::string &fn, const qpg_int *d_select, Subset &sub) {
  if (bt->B > (1 << 17)) return fail(QPG_ERR_UNSUPPORTED, fn + ": a subset needs B <= 131072");
  static_assert(QPG_Q_SELBAD == QPG_Q_NSEL + 1 && QPG_Q_SELBUSY == QPG_Q_NSEL + 2, "read as one block");
  int *words = (int *)bt->V.queue + QPG_Q_NSEL;
  RT_MEMSET(words, 0, 3 * sizeof(int));
  BT_LAUNCH(bt, k_select, (bt->B + bt->threads - 1) / bt->threads, 0, bt->V, (const int64_t *)d_select);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_select failed: " + std::string(RT_LAST_ERROR()));
  int got[3] = {0, 0, 0};
  RT_MEMCPY_D2H(got, words, sizeof(got));
  if (RT_STICKY()) return api_ok();
  if (got[1]) return fail(QPG_ERR_INVALID, fn + ": select holds a value other than 0 or 1");
  if (got[2]) return fail(QPG_ERR_INVALID, fn + ": a solve is in progress (qpg_batch_iterate left a member unfinished)");
  sub.list = bt->V.order; sub.S = got[0];
  return QPG_OK;
}
extern "C" int qpg_batch_step_subset_device(qpg_batch *bt, const QPGDeviceStep *io, const qpg_int *d_select, qpg_int *n_selected) {
  NEED_SETUP(bt, "qpg_batch_step_subset_device");
  if (!d_select) { if (n_selected) *n_selected = bt->B; return qpg_batch_step_device(bt, io); }
  { const int rc = step_args(io, "qpg_batch_step_subset_device"); if (rc != QPG_OK) return rc; }
  if (coop_wanted(bt) || sparse_coop_wanted(bt)) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_step_subset_device: not available in coop mode (one QP on many workgroups)");
  Subset sub;
  { const int rc = select_members(bt, "qpg_batch_step_subset_device", d_select, sub); if (rc != QPG_OK) return rc; }
  if (n_selected) *n_selected = sub.S;
  if (sub.S == 0) return api_ok();
  return step_run(bt, io, sub);
}

/* The adjoint of the solved batch (include/qpalm_gfx950.h; the kernel: qpalm_adjoint.h).  One launch of one workgroup per factor slot; the members come
 * off the work queue.  Pass cap of the refinement: 200 (a pass contracts the error by about 1 / (1 + sigma lambda), lambda the eigenvalues of
 * A_J Q^-1 A_J': sixteen digits in a handful of passes at the penalties a finished solve holds, and a member that needs more than 200 is flagged). */
#define QPG_ADJOINT_MAX_PASS 200
/* The penalty floor of the three sensitivity calls (include/qpalm_gfx950.h; DESIGN.md section 16): a number of the batch, kept by everything but
 * qpg_batch_destroy; sens_launch hands it to the kernel. */
extern "C" int qpg_batch_set_sens_penalty(qpg_batch *bt, qpg_float sigma_floor) {
  if (!bt) return fail(QPG_ERR_INVALID, "qpg_batch_set_sens_penalty: NULL");
  if (!(sigma_floor >= 0.0 && sigma_floor <= 1.7976931348623157e308)) return fail(QPG_ERR_INVALID, "qpg_batch_set_sens_penalty: the floor must be finite and >= 0");
  bt->sens_floor = sigma_floor;
  return QPG_OK;
}
extern "C" int qpg_batch_get_sens_penalty(qpg_batch *bt, qpg_float *out) {
  if (!bt || !out) return fail(QPG_ERR_INVALID, "qpg_batch_get_sens_penalty: NULL");
  *out = bt->sens_floor;
  return QPG_OK;
}
/* what the adjoint and the tangent refuse alike: modes without the Schur factor, a solve in progress (the scalars come over for it: one transfer of
 * B qpg_scalars per call, DESIGN.md section 13), a bad active_in */
static int sens_refusals(qpg_batch *bt, const std::string &fn, const qpg_int *active_in) {
  if (bt->kkt) return fail(QPG_ERR_UNSUPPORTED, fn + (bt->sparse ? ": not available for FACTORIZE_KKT batches (sparse_kkt)" : ": not available for FACTORIZE_KKT batches (dense KKT panel)"));
  if (bt->settings.nonconvex) return fail(QPG_ERR_UNSUPPORTED, fn + ": not available with nonconvex = 1");
  if (coop_wanted(bt) || sparse_coop_wanted(bt)) return fail(QPG_ERR_UNSUPPORTED, fn + ": not available in coop mode (one QP on many workgroups)");
  {
    std::vector<qpg_scalars> sc(bt->B);
    RT_MEMCPY_D2H(sc.data(), bt->V.sc, sc.size() * sizeof(qpg_scalars));
    for (auto &s : sc) if (s.in_solve) return fail(QPG_ERR_INVALID, fn + ": a solve is in progress (qpg_batch_iterate left a member unfinished)");
  }
  int *word = (int *)bt->V.queue; /* [0]: the work-queue head */
  if (active_in && bt->m > 0) {
    int *bad_d = word + 1; /* (a free word of the queue block: k_solve uses [0] and [64 ..)) */
    RT_MEMSET(bad_d, 0, sizeof(int));
    BT_LAUNCH(bt, k_adjoint_check, (int)std::min<size_t>(((size_t)bt->B * bt->m + bt->threads - 1) / bt->threads, 1024), 0, bt->V, (const int64_t *)active_in, bad_d);
    if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_adjoint_check failed: " + std::string(RT_LAST_ERROR()));
    int bad = 0;
    RT_MEMCPY_D2H(&bad, bad_d, sizeof(int));
    if (bad) return fail(QPG_ERR_INVALID, fn + ": active_in holds a value other than -1, 0, 1");
  }
  return QPG_OK;
}
/* the launch of k_adjoint (either mode); maps: the call reads or writes per-entry arrays in the caller's order.  K directions per member (DESIGN.md
 * section 18): the per-direction arrays are K blocks of the single call's layout; the single calls have K = 1 and no distance between directions */
static int sens_launch(qpg_batch *bt, qpg_adjoint_args &ar, bool maps, const Subset &sub, qpg_int K = 1) {
  ar.strideQ = bt->nnzQ_in; ar.strideA = bt->nnzA_in; ar.max_pass = QPG_ADJOINT_MAX_PASS; ar.sens_floor = bt->sens_floor;
  ar.ndir = (int32_t)K;
  if (K > 1) {
    const int64_t nB = bt->B;
    ar.dir_n = nB * bt->V.n; ar.dir_m = nB * bt->V.m; ar.dir_Q = nB * ar.strideQ; ar.dir_A = nB * ar.strideA; ar.dir_b = nB;
  }
  if (maps) {
    int32_t *mapA_d, *mapQ_d, *same_d;
    const int rcm = value_maps_device(bt, &mapA_d, &mapQ_d, &same_d);
    if (rcm != QPG_OK) return rcm;
    ar.mapA = mapA_d; ar.mapQ = mapQ_d; ar.same = same_d;
  }
  RT_MEMSET((int *)bt->V.queue, 0, sizeof(int));
  ar.list = sub.list;
  const int grid = std::min(sub.count(bt), bt->nslots);
  const size_t shm = (size_t)bt->lds_bytes;
  if (K > 1) { /* (K = 1: the single calls' kernel, whichever entry point the call came through) */
    if (bt->sparse) RT_LAUNCH(QP_INST(qp512, k_adjoint_multi<QPG_RPT_SPARSE>), grid, QP_T, shm, bt->V, ar);
    else BT_LAUNCH(bt, k_adjoint_multi<1>, grid, shm, bt->V, ar);
  } else if (bt->sparse) RT_LAUNCH(QP_INST(qp512, k_adjoint<QPG_RPT_SPARSE>), grid, QP_T, shm, bt->V, ar);
  else BT_LAUNCH(bt, k_adjoint<1>, grid, shm, bt->V, ar);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_adjoint failed: " + std::string(RT_LAST_ERROR()));
  return api_ok();
}
/* what the three subset forms do before their launch, after the refusals of the full form: the list.  1: nothing is selected, the call is over */
static int sens_select(qpg_batch *bt, const std::string &fn, const qpg_int *d_select, qpg_int *n_selected, Subset &sub, int &rc) {
  rc = QPG_OK;
  if (!d_select) { if (n_selected) *n_selected = bt->B; return 0; }
  if ((rc = select_members(bt, fn, d_select, sub)) != QPG_OK) return 1;
  if (n_selected) *n_selected = sub.S;
  if (sub.S == 0) { rc = api_ok(); return 1; }
  return 0;
}
/* the recorded point of the *_at_device calls (include/qpalm_gfx950.h; DESIGN.md section 17): all three arrays, and the point's set is the only source
 * for J.  use_at: the call is an "at" form (at == NULL is an error there). */
static int sens_point(const std::string &fn, bool use_at, const QPGDevicePoint *at, const qpg_int *io_active_in, const qpg_int **active_in) {
  *active_in = io_active_in;
  if (!use_at) return QPG_OK;
  if (!at || !at->x || !at->y || !at->active) return fail(QPG_ERR_INVALID, fn + ": the point needs x, y and active");
  if (io_active_in) return fail(QPG_ERR_INVALID, fn + ": active_in together with a point (the point's active set is the one used)");
  *active_in = at->active;
  return QPG_OK;
}
static int adjoint_run(qpg_batch *bt, const std::string &fn, const QPGDeviceAdjoint *io, bool use_at, const QPGDevicePoint *at, const qpg_int *d_select,
                       qpg_int *n_selected, qpg_int K = 1) {
  NEED_SETUP(bt, fn);
  if (K < 1 || K > 0x7fffffff) return fail(QPG_ERR_INVALID, fn + ": K must be at least 1");
  if (!io || !io->gx) return fail(QPG_ERR_INVALID, fn + ": gx is NULL");
  const qpg_int *active_in;
  { const int rc = sens_point(fn, use_at, at, io->active_in, &active_in); if (rc != QPG_OK) return rc; }
  { const int rc = sens_refusals(bt, fn, active_in); if (rc != QPG_OK) return rc; }
  Subset sub;
  { int rc; if (sens_select(bt, fn, d_select, n_selected, sub, rc)) return rc; }
  qpg_adjoint_args ar;
  memset(&ar, 0, sizeof(ar));
  ar.gx = io->gx; ar.gy = io->gy; ar.active_in = (const int64_t *)active_in;
  if (use_at) { ar.at_x = at->x; ar.at_y = at->y; }
  ar.dq = io->dq; ar.dbmin = io->dbmin; ar.dbmax = io->dbmax; ar.dQx = io->dQx; ar.dAx = io->dAx;
  ar.active_out = (int64_t *)io->active_out; ar.flag = (int64_t *)io->flag; ar.passes = (int64_t *)io->passes; ar.resid = io->resid;
  return sens_launch(bt, ar, io->dQx || io->dAx, sub, K);
}
extern "C" int qpg_batch_adjoint_device(qpg_batch *bt, const QPGDeviceAdjoint *io) { return qpg_batch_adjoint_subset_device(bt, io, nullptr, nullptr); }
extern "C" int qpg_batch_adjoint_subset_device(qpg_batch *bt, const QPGDeviceAdjoint *io, const qpg_int *d_select, qpg_int *n_selected) {
  return adjoint_run(bt, d_select ? "qpg_batch_adjoint_subset_device" : "qpg_batch_adjoint_device", io, false, nullptr, d_select, n_selected);
}
extern "C" int qpg_batch_adjoint_at_device(qpg_batch *bt, const QPGDeviceAdjoint *io, const QPGDevicePoint *at, const qpg_int *d_select, qpg_int *n_selected) {
  return adjoint_run(bt, "qpg_batch_adjoint_at_device", io, true, at, d_select, n_selected);
}
/* The tangent of the solved batch (include/qpalm_gfx950.h; DESIGN.md section 13): the adjoint's launch in its other mode -- the same kernel, set-up,
 * factor and refinement, on the right-hand side of a direction. */
static int tangent_run(qpg_batch *bt, const std::string &fn, const QPGDeviceTangent *io, bool use_at, const QPGDevicePoint *at, const qpg_int *d_select,
                       qpg_int *n_selected, qpg_int K = 1) {
  NEED_SETUP(bt, fn);
  if (K < 1 || K > 0x7fffffff) return fail(QPG_ERR_INVALID, fn + ": K must be at least 1");
  if (!io || (!io->dq && !io->dbmin && !io->dbmax && !io->dQx && !io->dAx)) return fail(QPG_ERR_INVALID, fn + ": no direction (dq, dbmin, dbmax, dQx and dAx are all NULL)");
  const qpg_int *active_in;
  { const int rc = sens_point(fn, use_at, at, io->active_in, &active_in); if (rc != QPG_OK) return rc; }
  { const int rc = sens_refusals(bt, fn, active_in); if (rc != QPG_OK) return rc; }
  Subset sub;
  { int rc; if (sens_select(bt, fn, d_select, n_selected, sub, rc)) return rc; }
  qpg_adjoint_args ar;
  memset(&ar, 0, sizeof(ar));
  ar.tangent = 1; ar.active_in = (const int64_t *)active_in;
  if (use_at) { ar.at_x = at->x; ar.at_y = at->y; }
  ar.t_dq = io->dq; ar.t_dbmin = io->dbmin; ar.t_dbmax = io->dbmax; ar.t_dQx = io->dQx; ar.t_dAx = io->dAx;
  ar.dx = io->dx; ar.dy = io->dy;
  ar.active_out = (int64_t *)io->active_out; ar.flag = (int64_t *)io->flag; ar.passes = (int64_t *)io->passes; ar.resid = io->resid;
  return sens_launch(bt, ar, io->dQx || io->dAx, sub, K);
}
extern "C" int qpg_batch_tangent_device(qpg_batch *bt, const QPGDeviceTangent *io) { return qpg_batch_tangent_subset_device(bt, io, nullptr, nullptr); }
extern "C" int qpg_batch_tangent_subset_device(qpg_batch *bt, const QPGDeviceTangent *io, const qpg_int *d_select, qpg_int *n_selected) {
  return tangent_run(bt, d_select ? "qpg_batch_tangent_subset_device" : "qpg_batch_tangent_device", io, false, nullptr, d_select, n_selected);
}
extern "C" int qpg_batch_tangent_at_device(qpg_batch *bt, const QPGDeviceTangent *io, const QPGDevicePoint *at, const qpg_int *d_select, qpg_int *n_selected) {
  return tangent_run(bt, "qpg_batch_tangent_at_device", io, true, at, d_select, n_selected);
}
/* K directions per call (include/qpalm_gfx950.h; DESIGN.md section 18): the same runners -- one round trip for in_solve, one k_adjoint_check, one selection
 * and one launch, in which a member's directions run one after another on the factor its set-up left.  at / d_select = NULL: the stored solutions / every
 * member, so one entry point covers the plain, the subset and the recorded-point forms. */
extern "C" int qpg_batch_adjoint_multi_device(qpg_batch *bt, const QPGDeviceAdjoint *io, qpg_int K, const QPGDevicePoint *at, const qpg_int *d_select,
                                              qpg_int *n_selected) {
  return adjoint_run(bt, "qpg_batch_adjoint_multi_device", io, at != nullptr, at, d_select, n_selected, K);
}
extern "C" int qpg_batch_tangent_multi_device(qpg_batch *bt, const QPGDeviceTangent *io, qpg_int K, const QPGDevicePoint *at, const qpg_int *d_select,
                                              qpg_int *n_selected) {
  return tangent_run(bt, "qpg_batch_tangent_multi_device", io, at != nullptr, at, d_select, n_selected, K);
}
/* The active set of the stored solutions on its own (include/qpalm_gfx950.h; k_get_active): what active_out of an adjoint call on this state holds */
extern "C" int qpg_batch_get_active_device(qpg_batch *bt, qpg_int *d_active) { return qpg_batch_get_active_subset_device(bt, d_active, nullptr, nullptr); }
extern "C" int qpg_batch_get_active_subset_device(qpg_batch *bt, qpg_int *d_active, const qpg_int *d_select, qpg_int *n_selected) {
  const std::string fn = d_select ? "qpg_batch_get_active_subset_device" : "qpg_batch_get_active_device";
  NEED_SETUP(bt, fn);
  if (!d_active) return fail(QPG_ERR_INVALID, fn + ": d_active is NULL");
  { const int rc = sens_refusals(bt, fn, nullptr); if (rc != QPG_OK) return rc; }
  Subset sub;
  { int rc; if (sens_select(bt, fn, d_select, n_selected, sub, rc)) return rc; }
  BT_LAUNCH(bt, k_get_active, sub.blocks(bt), 0, bt->V, (int64_t *)d_active, sub.list);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_get_active failed: " + std::string(RT_LAST_ERROR()));
  return api_ok();
}
/* The polish of the solved batch (include/qpalm_gfx950.h; DESIGN.md section 14): the same launch in its third mode -- the correction of the stored
 * solution to the exact solution at its active set, a verdict per member and, with store, the accepted candidates as the new stored solutions. */
extern "C" int qpg_batch_polish_device(qpg_batch *bt, const QPGDevicePolish *io) { return qpg_batch_polish_subset_device(bt, io, nullptr, nullptr); }
extern "C" int qpg_batch_polish_subset_device(qpg_batch *bt, const QPGDevicePolish *io, const qpg_int *d_select, qpg_int *n_selected) {
  const std::string fn = d_select ? "qpg_batch_polish_subset_device" : "qpg_batch_polish_device";
  NEED_SETUP(bt, fn);
  if (!io || (!io->x && !io->y && !io->res && !io->store)) return fail(QPG_ERR_INVALID, fn + ": nothing to do (x, y and res are all NULL and store is 0)");
  { const int rc = sens_refusals(bt, fn, io->active_in); if (rc != QPG_OK) return rc; }
  Subset sub;
  { int rc; if (sens_select(bt, fn, d_select, n_selected, sub, rc)) return rc; }
  qpg_adjoint_args ar;
  memset(&ar, 0, sizeof(ar));
  ar.polish = 1; ar.store = io->store ? 1 : 0; ar.active_in = (const int64_t *)io->active_in;
  ar.p_x = io->x; ar.p_y = io->y; ar.p_res = io->res;
  ar.active_out = (int64_t *)io->active_out; ar.flag = (int64_t *)io->flag; ar.passes = (int64_t *)io->passes; ar.resid = io->resid;
  return sens_launch(bt, ar, false, sub);
}

extern "C" void qpg_batch_destroy(qpg_batch *bt) {
  if (!bt) return;
  if (bt->arena_thread.joinable()) bt->arena_thread.join();
  if (bt->arena_d) RT_FREE(bt->arena_d);
  if (bt->dual_d) RT_FREE(bt->dual_d);
  if (bt->sparse_d) RT_FREE(bt->sparse_d);
  if (bt->co_tab_d) RT_FREE(bt->co_tab_d);
  if (bt->val_maps_d) RT_FREE(bt->val_maps_d);
  if (bt->raw_d) RT_FREE(bt->raw_d);
  co_graphs_clear(bt);
  host_slab_free(bt->hslab, bt->hslab_bytes);
  delete bt;
}

/* ---- solver_interface.h surface -------------------------------------------------------------- */
static int run_op(qpg_batch *bt, qpg_int idx, int op, const char *fn) {
  NEED_SETUP(bt, fn);
  if (idx < 0 || idx >= bt->B || idx >= bt->nslots) return fail(QPG_ERR_INVALID, std::string(fn) + ": bad index (needs idx < max_slots)");
  const int rpt = bt->sparse ? 1 : (bt->nfac + bt->threads - 1) / bt->threads;
  const size_t shm = (size_t)bt->lds_bytes;
  const bool sp_kkt_op = bt->kkt && (op == QP_OP_KKT_FORM || op == QP_OP_KKT_FACTOR || op == QP_OP_KKT_ENTER || op == QP_OP_KKT_LEAVE || op == QP_OP_KKT_SOLVE);
  if (bt->sparse && bt->kkt && (op == QP_OP_LDLCHOL || op == QP_OP_LDLCHOL_QATSA || op == QP_OP_UPDATE_ENTER || op == QP_OP_DOWNDATE_LEAVE || op == QP_OP_UPDATE_SIGMA || op == QP_OP_SOLVE))
    return fail(QPG_ERR_UNSUPPORTED, std::string(fn) + ": Schur-mode factor operation (this batch keeps a sparse L D L' of K)");
  if (bt->sparse && (sp_kkt_op || op == QP_OP_LDLCHOL || op == QP_OP_LDLCHOL_QATSA || op == QP_OP_UPDATE_ENTER || op == QP_OP_DOWNDATE_LEAVE || op == QP_OP_UPDATE_SIGMA || op == QP_OP_SOLVE)) {
    BT_LAUNCH(bt, k_op_sparse, 1, shm, bt->V, (int)idx, op); /* the factor operations of solver_interface.h on the sparse L D L' (round 6) */
    if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, std::string(fn) + " failed: " + RT_LAST_ERROR());
    return api_ok();
  }
  if (bt->sparse && op != QP_OP_MATVEC_A && op != QP_OP_MATVEC_Q && op != QP_OP_MATTVEC_A && op != QP_OP_RESIDUALS && op != QP_OP_ACTIVE && op != QP_OP_LINESEARCH)
    return fail(QPG_ERR_UNSUPPORTED, std::string(fn) + ": works on the dense panel (this batch keeps a sparse L D L')");
  auto own = [&](int o) { BT_RPT(rpt, R, BT_LAUNCH(bt, k_op<R>, 1, shm, bt->V, (int)idx, o)); }; /* the operation on the QP's own workgroup */
  const bool factor_op = op == QP_OP_LDLCHOL || op == QP_OP_LDLCHOL_QATSA || op == QP_OP_SOLVE;
  const bool update_op = op == QP_OP_UPDATE_ENTER || op == QP_OP_DOWNDATE_LEAVE || op == QP_OP_UPDATE_SIGMA;
  if ((factor_op || (update_op && bt->ctx->coop_updates != 0)) && coop_wanted(bt)) {
    /* A coop batch (Schur mode, dense factor, 512-thread instance: coop_wanted): the factor operations run on the grid kernels, through the chain
     * a suspended iteration gets (coop_linear_algebra).  The chain's kernels read what they do from the member's scalars: pend_la / pend_gam /
     * pend_nchange and the two rank counts are written for the call and put back after it; pend_stage stays 0, so that a later iterate or solve
     * finds no suspension.  coop_updates = 0 keeps the updates on the QP's workgroup, as a solve does. */
    qpg_view V;
    { const int rc = coop_view(bt, V); if (rc != QPG_OK) return rc; }
    if (op == QP_OP_UPDATE_SIGMA) own(QP_OP_SIGMA_SCALE); /* dev_solve's order around its la == 4 suspension: scale, sweeps, post */
    if (op == QP_OP_SOLVE) own(QP_OP_NEG_DPHI);
    qpg_scalars s0;
    RT_MEMCPY_D2H(&s0, bt->V.sc + idx, sizeof(s0)); /* (the copy waits for the kernel before it) */
    if (RT_STICKY()) return api_ok();
    qpg_scalars s = s0;
    s.pend_stage = 0; s.pend_action = 0; s.pend_kind = (op == QP_OP_SOLVE) ? 0 : 1; s.pend_nchange = 0; s.pend_gam = s0.gamma;
    switch (op) {
      case QP_OP_LDLCHOL: s.pend_la = 3; break;
      case QP_OP_LDLCHOL_QATSA: s.pend_la = 1; break;
      case QP_OP_UPDATE_ENTER: s.pend_la = 2; s.nb_leave = 0; break; /* (the one-workgroup operation passes 0 for the other count) */
      case QP_OP_DOWNDATE_LEAVE: s.pend_la = 2; s.nb_enter = 0; break;
      case QP_OP_UPDATE_SIGMA: s.pend_la = 4; s.pend_nchange = s0.nb_sigma_changed; break;
      default: s.pend_la = 0; break; /* QP_OP_SOLVE: the solve chain alone */
    }
    RT_MEMCPY_H2D(bt->V.sc + idx, &s, sizeof(s));
    coop_linear_algebra(bt, V, (int)idx, s);
    bt->co_op_chains++;
    const int rc_sync = RT_SYNC();
    qpg_scalars s1; /* the kernels' counters stay, the fields written for the call go back */
    RT_MEMCPY_D2H(&s1, bt->V.sc + idx, sizeof(s1));
    s1.pend_stage = s0.pend_stage; s1.pend_la = s0.pend_la; s1.pend_action = s0.pend_action; s1.pend_kind = s0.pend_kind;
    s1.pend_nchange = s0.pend_nchange; s1.pend_gam = s0.pend_gam; s1.nb_enter = s0.nb_enter; s1.nb_leave = s0.nb_leave;
    RT_MEMCPY_H2D(bt->V.sc + idx, &s1, sizeof(s1));
    if (rc_sync != 0) return fail(QPG_ERR_RUNTIME, std::string(fn) + " failed (coop kernels): " + RT_LAST_ERROR());
    if (update_op && V.co_flags) { /* a workgroup of the one-launch sweep that gave up waiting: nobody resumes after a single operation to rebuild the factor */
      int fl[4];
      RT_MEMCPY_D2H(fl, V.co_flags + (size_t)idx * 4, sizeof(fl));
      if (fl[1] != 0) {
        RT_MEMSET(V.co_flags + (size_t)idx * 4, 0, sizeof(fl));
        return fail(QPG_ERR_RUNTIME, std::string(fn) + ": coop update sweep: workgroup " + std::to_string(fl[1] - 1) + " timed out waiting for a table (the factor is half updated)");
      }
    }
    if (op != QP_OP_UPDATE_SIGMA) return api_ok();
    op = QP_OP_SIGMA_POST;
  }
  own(op);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, std::string(fn) + " failed: " + RT_LAST_ERROR());
  return api_ok();
}
/* single operations of the boundary that ran on the coop grid kernels since the batch was created (run_op; 0 on a batch that is not in coop mode) */
extern "C" int qpg_batch_coop_op_chains(qpg_batch *bt, qpg_int *count) {
  NEED_SETUP(bt, "qpg_batch_coop_op_chains");
  if (count) *count = (qpg_int)bt->co_op_chains;
  return api_ok();
}
static int matvec_common(qpg_batch *bt, qpg_int idx, int op, size_t nin, size_t nout, const qpg_float *x, qpg_float *y, const char *fn) {
  NEED_SETUP(bt, fn);
  if (!x || !y) return fail(QPG_ERR_INVALID, std::string(fn) + ": NULL");
  /* x may alias y (solver_interface.c:257-261 copies x first); the staging copy gives that for free */
  RT_MEMCPY_H2D(bt->V.op_in, x, nin * sizeof(double));
  const int rc = run_op(bt, idx, op, fn);
  if (rc != QPG_OK) return rc;
  RT_MEMCPY_D2H(y, bt->V.op_out, nout * sizeof(double));
  return api_ok();
}
extern "C" int qpg_mat_vec(qpg_batch *bt, qpg_int idx, int which, const qpg_float *x, qpg_float *y) {
  if (!bt) return fail(QPG_ERR_INVALID, "qpg_mat_vec: NULL");
  if (which == 'A') return matvec_common(bt, idx, QP_OP_MATVEC_A, bt->n, bt->m, x, y, "qpg_mat_vec");
  if (which == 'Q') return matvec_common(bt, idx, QP_OP_MATVEC_Q, bt->n, bt->n, x, y, "qpg_mat_vec");
  return fail(QPG_ERR_INVALID, "qpg_mat_vec: which must be 'A' or 'Q'");
}
extern "C" int qpg_mat_tpose_vec(qpg_batch *bt, qpg_int idx, int which, const qpg_float *x, qpg_float *y) {
  if (!bt) return fail(QPG_ERR_INVALID, "qpg_mat_tpose_vec: NULL");
  if (which == 'A') return matvec_common(bt, idx, QP_OP_MATTVEC_A, bt->m, bt->n, x, y, "qpg_mat_tpose_vec");
  if (which == 'Q') return matvec_common(bt, idx, QP_OP_MATVEC_Q, bt->n, bt->n, x, y, "qpg_mat_tpose_vec"); /* symmetric */
  return fail(QPG_ERR_INVALID, "qpg_mat_tpose_vec: which must be 'A' or 'Q'");
}
extern "C" int qpg_ldlchol(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_LDLCHOL, "qpg_ldlchol"); }
extern "C" int qpg_ldlchol_matrix(qpg_batch *bt, qpg_int idx, qpg_int n, const qpg_int *Mp, const qpg_int *Mi, const qpg_float *Mx) {
  NEED_SETUP(bt, "qpg_ldlchol_matrix");
  if (bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_ldlchol_matrix: works on the dense factor (this batch keeps a sparse L D L')");
  if (n != bt->n || idx < 0 || idx >= bt->nslots || !Mp) return fail(QPG_ERR_INVALID, "qpg_ldlchol_matrix: bad argument");
  if (bt->kkt) return fail(QPG_ERR_UNSUPPORTED, "qpg_ldlchol_matrix: Schur-mode boundary operation (the batch is in KKT mode)");
  std::vector<double> H((size_t)bt->ld * n, 0.0);
  for (qpg_int j = 0; j < n; j++)
    for (qpg_int k = Mp[j]; k < Mp[j + 1]; k++) if (Mi[k] >= j) H[(size_t)j * bt->ld + Mi[k]] += Mx[k];
  RT_MEMCPY_H2D(bt->V.L + (size_t)idx * bt->ld * bt->nfac, H.data(), H.size() * sizeof(double));
  return run_op(bt, idx, QP_OP_FACTOR_LOADED, "qpg_ldlchol_matrix");
}

extern "C" int qpg_sparse_matvec(qpg_ctx *ctx, qpg_int nrow, qpg_int ncol, const qpg_int *Ap, const qpg_int *Ai, const qpg_float *Ax,
                                 int stype, int transpose, const qpg_float *x, qpg_float *y) {
  if (!ctx || !Ap || !x || !y) return fail(QPG_ERR_INVALID, "qpg_sparse_matvec: NULL");
  /* compressed rows of the operator (A, A' or the symmetric completion), like cholmod_sdmult's cases */
  const bool sym = stype != 0;
  const qpg_int nout = sym ? ncol : (transpose ? ncol : nrow), nin = sym ? ncol : (transpose ? nrow : ncol);
  std::vector<std::vector<std::pair<int, double> > > rows(nout);
  for (qpg_int j = 0; j < ncol; j++)
    for (qpg_int k = Ap[j]; k < Ap[j + 1]; k++) {
      const qpg_int i = Ai[k];
      if (sym) {
        if (stype < 0 ? i < j : i > j) continue; /* ignored triangle */
        rows[i].push_back(std::make_pair((int)j, Ax[k]));
        if (i != j) rows[j].push_back(std::make_pair((int)i, Ax[k]));
      } else if (transpose) rows[j].push_back(std::make_pair((int)i, Ax[k]));
      else rows[i].push_back(std::make_pair((int)j, Ax[k]));
    }
  std::vector<int> ptr(nout + 1, 0), idx;
  std::vector<double> val;
  for (qpg_int r = 0; r < nout; r++) { ptr[r] = (int)idx.size(); for (auto &e : rows[r]) { idx.push_back(e.first); val.push_back(e.second); } }
  ptr[nout] = (int)idx.size();
  if (idx.empty()) { idx.push_back(0); val.push_back(0.0); }
  int *dptr = nullptr, *didx = nullptr; double *dval = nullptr, *dx = nullptr, *dy = nullptr;
  if (ctx_scratch(ctx, 0, ptr.size() * sizeof(int), (void **)&dptr) || ctx_scratch(ctx, 1, idx.size() * sizeof(int), (void **)&didx) ||
      ctx_scratch(ctx, 2, val.size() * sizeof(double), (void **)&dval) ||
      ctx_scratch(ctx, 3, (size_t)std::max<qpg_int>(nin, 1) * sizeof(double), (void **)&dx) ||
      ctx_scratch(ctx, 4, (size_t)std::max<qpg_int>(nout, 1) * sizeof(double), (void **)&dy))
    return fail(QPG_ERR_ALLOC, "qpg_sparse_matvec: device allocation failed");
  RT_MEMCPY_H2D(dptr, ptr.data(), ptr.size() * sizeof(int)); RT_MEMCPY_H2D(didx, idx.data(), idx.size() * sizeof(int));
  RT_MEMCPY_H2D(dval, val.data(), val.size() * sizeof(double)); RT_MEMCPY_H2D(dx, x, (size_t)nin * sizeof(double)); /* x may alias y */
  RT_LAUNCH(QP_INST(qp512, k_spmv_generic), 1, QP_T, 0, (int)nout, (const int *)dptr, (const int *)didx, (const double *)dval, (const double *)dx, dy);
  const int rc = RT_SYNC();
  RT_MEMCPY_D2H(y, dy, (size_t)nout * sizeof(double));
  return rc == 0 ? api_ok() : fail(QPG_ERR_RUNTIME, std::string("qpg_sparse_matvec failed: ") + RT_LAST_ERROR());
}

extern "C" int qpg_ldlcholQAtsigmaA(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_LDLCHOL_QATSA, "qpg_ldlcholQAtsigmaA"); }
extern "C" int qpg_ldlupdate_entering_constraints(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_UPDATE_ENTER, "qpg_ldlupdate_entering_constraints"); }
extern "C" int qpg_ldldowndate_leaving_constraints(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_DOWNDATE_LEAVE, "qpg_ldldowndate_leaving_constraints"); }
extern "C" int qpg_ldlupdate_sigma_changed(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_UPDATE_SIGMA, "qpg_ldlupdate_sigma_changed"); }
extern "C" int qpg_ldlsolveLD_neg_dphi(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_SOLVE, "qpg_ldlsolveLD_neg_dphi"); }
extern "C" int qpg_compute_residuals(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_RESIDUALS, "qpg_compute_residuals"); }
extern "C" int qpg_set_active_constraints(qpg_batch *bt, qpg_int idx) { return run_op(bt, idx, QP_OP_ACTIVE, "qpg_set_active_constraints"); }
/* KKT operations (solver_interface.h:82-126); the batch must have been created with factorization_method = FACTORIZE_KKT */
static int run_kkt_op(qpg_batch *bt, qpg_int idx, int op, const char *fn) {
  if (bt && !bt->kkt) return fail(QPG_ERR_UNSUPPORTED, std::string(fn) + ": the batch is in Schur mode (factorization_method != FACTORIZE_KKT)");
  return run_op(bt, idx, op, fn);
}
extern "C" int qpg_kkt_form(qpg_batch *bt, qpg_int idx) { return run_kkt_op(bt, idx, QP_OP_KKT_FORM, "qpg_kkt_form"); }
extern "C" int qpg_kkt_factorize(qpg_batch *bt, qpg_int idx) { return run_kkt_op(bt, idx, QP_OP_KKT_FACTOR, "qpg_kkt_factorize"); }
extern "C" int qpg_kkt_update_entering_constraints(qpg_batch *bt, qpg_int idx) { return run_kkt_op(bt, idx, QP_OP_KKT_ENTER, "qpg_kkt_update_entering_constraints"); }
extern "C" int qpg_kkt_update_leaving_constraints(qpg_batch *bt, qpg_int idx) { return run_kkt_op(bt, idx, QP_OP_KKT_LEAVE, "qpg_kkt_update_leaving_constraints"); }
extern "C" int qpg_kkt_solve(qpg_batch *bt, qpg_int idx) { return run_kkt_op(bt, idx, QP_OP_KKT_SOLVE, "qpg_kkt_solve"); }
extern "C" int qpg_exact_linesearch(qpg_batch *bt, qpg_int idx, qpg_float *tau) {
  const int rc = run_op(bt, idx, QP_OP_LINESEARCH, "qpg_exact_linesearch");
  if (rc != QPG_OK) return rc;
  qpg_scalars s;
  RT_MEMCPY_D2H(&s, bt->V.sc + idx, sizeof(s));
  if (tau) *tau = s.tau;
  return api_ok();
}

extern "C" int qpg_batch_ldlsolve_all(qpg_batch *bt, qpg_int reps, float *ms_per_rep) {
  NEED_SETUP(bt, "qpg_batch_ldlsolve_all");
  if (bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_ldlsolve_all: works on the dense factor (this batch keeps a sparse L D L')");
  const int grid = std::min(bt->B, bt->nslots);
  float ms = 0.f;
  BT_TIMED_LAUNCH(ms, bt, k_ldlsolve_all, grid, (size_t)bt->lds_bytes, bt->V, (int)reps);
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_ldlsolve_all failed: " + std::string(RT_LAST_ERROR()));
  if (ms_per_rep) *ms_per_rep = ms / (float)(reps > 0 ? reps : 1);
  return api_ok();
}

/* diagnostic: the update sweep alone on every resident workgroup (k_sweep_probe); ms = duration of the launch */
extern "C" int qpg_batch_sweep_probe(qpg_batch *bt, qpg_int reps, qpg_int nranks, float *ms_out) {
  NEED_SETUP(bt, "qpg_batch_sweep_probe");
  if (bt->sparse) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_sweep_probe: works on the dense factor (this batch keeps a sparse L D L')");
  if (bt->kkt) return fail(QPG_ERR_UNSUPPORTED, "qpg_batch_sweep_probe: Schur mode only");
  const int grid = std::min(bt->B, bt->nslots);
  RT_MEMSET(bt->V.queue, 0, (64 + QPG_CU_KEYS) * sizeof(int));
  const int rpt = (bt->nfac + bt->threads - 1) / bt->threads;
  const size_t shm = (size_t)bt->lds_bytes;
  float ms = 0.f;
  BT_RPT(rpt, R, BT_TIMED_LAUNCH(ms, bt, k_sweep_probe<R>, grid, shm, bt->V, (int)reps, (int)nranks));
  if (RT_SYNC() != 0) return fail(QPG_ERR_RUNTIME, "k_sweep_probe failed: " + std::string(RT_LAST_ERROR()));
  if (ms_out) *ms_out = ms;
  return api_ok();
}

/* measured bandwidth of this device: best of `reps` passes over `bytes` bytes.  mode 0: copy (read + write counted),
 * mode 1: read-only stream (GB/s, 1e9) */
static int hbm_yardstick(qpg_ctx *ctx, size_t bytes, qpg_int reps, int mode, float *gbs) {
  if (!ctx || !gbs || bytes < 4096 || reps < 1) return fail(QPG_ERR_INVALID, "qpg_ctx_hbm_*_gbs: bad argument");
  bytes &= ~(size_t)255;
  double *src = nullptr, *dst = nullptr;
  if (RT_MALLOC(&src, bytes) != 0) return fail(QPG_ERR_ALLOC, "qpg_ctx_hbm_*_gbs: device allocation failed");
  if (RT_MALLOC(&dst, mode ? 256 : bytes) != 0) { RT_FREE(src); return fail(QPG_ERR_ALLOC, "qpg_ctx_hbm_*_gbs: device allocation failed"); }
  RT_MEMSET(src, 0, bytes); RT_MEMSET(dst, 0, mode ? 256 : bytes);
  const size_t npairs = bytes / 16;
  const int grid = (int)std::min<size_t>((npairs + 255) / 256, mode ? 4096 : 8192);
  float ms = 0.f, best = 1e30f;
  for (qpg_int r = 0; r <= reps; r++) { /* pass 0 is the warm-up */
    if (mode) RT_TIMED_LAUNCH(ms, QP_INST(qp512, k_hbm_read), grid, 256, 0, (const double *)src, dst, npairs);
    else RT_TIMED_LAUNCH(ms, QP_INST(qp512, k_hbm_copy), grid, 256, 0, (const double *)src, dst, npairs);
    if (r > 0 && ms < best) best = ms;
  }
  const int rc = RT_SYNC();
  RT_FREE(src); RT_FREE(dst);
  if (rc != 0) return fail(QPG_ERR_RUNTIME, std::string("HBM yardstick kernel failed: ") + RT_LAST_ERROR());
  *gbs = (float)((mode ? 1.0 : 2.0) * (double)bytes / ((double)best * 1e-3) / 1e9);
  return api_ok();
}
extern "C" int qpg_ctx_hbm_copy_gbs(qpg_ctx *ctx, size_t bytes, qpg_int reps, float *gbs) { return hbm_yardstick(ctx, bytes, reps, 0, gbs); }
extern "C" int qpg_ctx_hbm_read_gbs(qpg_ctx *ctx, size_t bytes, qpg_int reps, float *gbs) { return hbm_yardstick(ctx, bytes, reps, 1, gbs); }

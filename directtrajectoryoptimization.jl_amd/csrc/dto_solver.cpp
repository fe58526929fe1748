// Host driver of the batched interior-point / KKT path (the part of the reference that lives inside
// Ipopt: src/solver.jl:45-47 `solve!` -> MOI.optimize!).  All numerics run in the plugin's kernels
// (dto_kkt_kernels.hpp); this file only owns device state and the launch sequence of one iteration:
//     EVAL -> CONV -> FACTOR_SOLVE -> LINESEARCH -> LS_REDUCE -> UPDATE
// No host round trip happens inside an iteration; the host polls completion every `check_every`
// iterations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dto.h"
#include "dto_kkt_kernels.hpp"
#include "dto_point_rules.hpp"
#include "dto_im_kernels.hpp"
#include "dto_wide_kernels.hpp"
#include "dto_border_kernels.hpp"
#include "dto_problem.hpp"
#include "dto_host_globalization.hpp"

#define HIP_TRY(expr)                                       \
  do {                                                      \
    hipError_t e_ = (expr);                                 \
    if (e_ != hipSuccess) return dto::hip_fail(e_, #expr);  \
  } while (0)

namespace dto {

// Ownership rule of this file: device memory lives in DevBuf members and locals (dto_problem.hpp) and nowhere else.  A state is
// rebuilt release-old-then-allocate-new, and a set-up that fails after the old state was dropped leaves an EMPTY state (B = 0),
// so that the retry hip_fail promises to callers builds it again instead of reusing half of one.

// The device buffers of a SolverState: a base of their own, so that release() drops them all with one assignment.
struct SolverBufs {
  DevBuf<double> wtile;                     // per-instance parameters (SoA tiles), allocated on first use
  DevBuf<int> d_inst_of_slot, d_src_slot;   // dto_solver_repack: d_inst_of_slot is empty while the map is the identity
  DevBuf<double> repack_tmp;
  DevBuf<double> sigx, sigc;                // linear-solver entry points: extra diagonals (SoA tiles), allocated on first use
  DevBuf<int> d_ioff;
  DevBuf<int64_t> d_recoff, d_facoff;
  DevBuf<dto_stage_run> d_runs;             // the horizon as runs of one stage kind with constant strides (sequential sweeps)
  DevBuf<double> d_lo, d_hi;
  DevBuf<double> z, lam, zl, zu, s, zs;     // SoA state
  DevBuf<int> tile_fwd_tag, tile_bwd_tag, fwd_started;   // sequential sweeps overlapped through a second stream (k_kkt_bwd_early)
  DevBuf<double> qn;                        // limited-memory BFGS: history, columns and small matrices per tile (QnRows)
  // iterative refinement (dto_options.kkt_refinement): cross-stage terms, the step being refined, copy of the records (lazy)
  DevBuf<double> refq, refvz, refvl, rec_bak;
  DevBuf<double> z_alt, lam_alt;            // second iterate / multiplier buffers of the fused UPDATE+EVAL pass (lazy)
  DevBuf<double> dz, dlam, ds;
  DevBuf<double> rec, fac, part, lspart, scal, filt;
  DevBuf<double> csum, sfac, xsep, cacc, cpart;
  DevBuf<int> csync;         // per tile: arrival counters of the in-launch joins of the time-partitioned form (dto_kkt_args.csync)
  DevBuf<int> d_cstart_all;  // chunk boundaries for P = 1 .. P_cap back to back (a batch that started sequential may
                             // switch to 2 / 4 chunks when repacking has left too few tiles to fill the GPU)
};

struct SolverState : SolverBufs {
  int64_t B = 0;
  int G = 0;
  int64_t Ni = 0, rec_total = 0, fac_total = 0, n_bnd = 0;
  bool use_wtile = false;
  // dto_solver_repack: running instances are moved to the leading tiles; slot <-> instance maps (identity until then)
  int G_active = 0;
  std::vector<int> inst_of_slot, slot_of_inst;
  bool use_sigx = false, use_sigc = false, assembled = false;
  std::vector<int> ioff;
  std::vector<int64_t> recoff, facoff;
  int n_runs = 0;
  int sweep_tag = 0;
  hipStream_t stream_lo = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  SolverState* cols = nullptr;   // limited-memory BFGS, small batches: a second state whose instances are the columns of U
  int fuse_state = 0;   // 0 not decided, 1 buffers allocated, -1 not available (memory, switch)
  int sb = 8;           // stages per wavefront of the stage-parallel kernels (dto_kkt_args.sb)
  int P = 1;            // chunks of the time-partitioned factorisation (current)
  int P0 = 1;           // ... as chosen when the batch was loaded; P_cap: what the chunk arrays are sized for
  int P_cap = 1;
  int forced_P = 0;     // 0 = choose from the batch size
  int n_simd = 1024;
  std::vector<int> cstart;
  int* d_cstart = nullptr;   // the block of the current P inside d_cstart_all
  dto_kkt_info info{};
  dto_solver_opts opt{};
  dto_options user{};
  bool begun = false;
  std::vector<double> h_scal;  // host copy of the scalar block

  void release() {
    static_cast<SolverBufs&>(*this) = SolverBufs();
    d_cstart = nullptr; n_runs = 0; fuse_state = 0; sweep_tag = 0;
    if (stream_lo) { (void)hipStreamDestroy(stream_lo); stream_lo = nullptr; }
    if (ev_fork) { (void)hipEventDestroy(ev_fork); ev_fork = nullptr; }
    if (ev_join) { (void)hipEventDestroy(ev_join); ev_join = nullptr; }
    use_wtile = false;
    use_sigx = use_sigc = assembled = false;
    G_active = 0;
    inst_of_slot.clear(); slot_of_inst.clear();
    B = 0; G = 0;
    delete cols; cols = nullptr;
  }
  ~SolverState() { release(); }
};
// releases a state when its set-up returns early (ensure_state, ensure_im_state); `s = nullptr` once the state is complete
template <class S>
struct ReleaseOnError {
  S* s;
  ~ReleaseOnError() { if (s) s->release(); }
};

// Device state of the instance-major engine (dto_im_kernels.hpp)
struct ImBufs {
  DevBuf<int> d_aoff, d_doff, d_coff, d_boff, d_ioff;
  DevBuf<double> d_lo, d_hi;
  DevBuf<double> A, R, D, C, Bd;
  DevBuf<double> part, lspart, scal, filt, wbuf;
  DevBuf<int> phase;
  DevBuf<int> lists;   // 3 x B
  DevBuf<int> ctr;     // [0..2] list lengths, [3..4] sweep tickets, [5..6] running / work left
};
struct ImState : ImBufs {
  int64_t B = 0;
  dto_im_info info{};
  std::vector<int> aoff, doff, coff, boff, ioff;
  int64_t a_total = 0, d_total = 0, c_total = 0, b_total = 0, Ni = 0, n_bnd = 0;
  bool use_w = false;
  int* h_ctr = nullptr;   // pinned host mirror of ctr
  int nwin_e = 1, nwin_l = 1;
  dto_solver_opts opt{};
  dto_options user{};
  bool begun = false;
  int iter_base = 0;      // iterations requested so far through dto_solver_iterate
  int64_t passes = 0;     // passes launched since dto_solver_begin (diagnostic)
  std::vector<double> h_scal;

  void release() {
    static_cast<ImBufs&>(*this) = ImBufs();
    if (h_ctr) (void)hipHostFree(h_ctr);
    h_ctr = nullptr;
    B = 0; begun = false; use_w = false;
  }
  ~ImState() { release(); }
};

static void default_opts(dto_solver_opts& o, const dto_options& u) {
  o.tol = u.tol; o.s_max = u.s_max; o.dual_inf_tol = u.dual_inf_tol; o.constr_viol_tol = u.constr_viol_tol;
  o.compl_inf_tol = u.compl_inf_tol; o.max_iter = u.max_iter;
  o.acceptable_tol = u.acceptable_tol; o.acceptable_iter = u.acceptable_iter; o.acceptable_dual_inf_tol = u.acceptable_dual_inf_tol;
  o.acceptable_constr_viol_tol = u.acceptable_constr_viol_tol; o.acceptable_compl_inf_tol = u.acceptable_compl_inf_tol;
  o.acceptable_obj_change_tol = u.acceptable_obj_change_tol;
  o.diverging_iterates_tol = u.diverging_iterates_tol; o.mu_target = u.mu_target;
  o.mu_init = u.mu_init; o.kappa_eps = 10.0; o.kappa_mu = 0.2; o.theta_mu = 1.5; o.tau_min = 0.99;
  o.bound_push = 1e-2; o.bound_frac = 1e-2;
  o.delta_c = u.delta_c; o.delta_w_init = u.delta_w_init; o.delta_w_min = 1e-20; o.delta_w_max = 1e20;
  // (measurement knob: DTO_DW_FLOOR=1e-4 restores the floor of rounds 2 - 5 for the decaying delta_w)
  if (const char* e = getenv("DTO_DW_FLOOR")) { const double v = atof(e); if (v > 0.0) o.delta_w_min = v; }
  o.kappa_w_minus = 1.0 / 3.0; o.kappa_w_plus = 8.0; o.kappa_w_plus_first = 100.0;
  // largest delta_w tried on the exact Hessian before the constraint curvature is dropped (Gauss-Newton fallback).  Round 1
  // used 1: measured on the C port over 128-256 seeds per config, 100 halves the iterations of
  // acrobot T=301 (median 73 -> 34) and car T=51 (58 -> 25), takes acrobot T=1000 from 50 % to 60 % converged within 1000
  // iterations and leaves the other configs where they were; 1000 is better still at T=1000 (70 %) but loses T=301 instances,
  // no cap at all is the delta_w death spiral of round 1
  o.delta_w_exact_cap = 100.0;
  if (const char* e = getenv("DTO_EXACT_CAP")) o.delta_w_exact_cap = atof(e);  // experiment knob
  o.eta_armijo = 1e-4; o.rho_penalty = 0.1; o.piv_tol = 1e-9;
  o.max_refactor = 9;
  // Ipopt's watchdog defaults are (10, 3) with a rollback; this one has no rollback but bounds the violation of its trial
  // steps (k_ls_reduce), which makes an earlier trigger safe and much faster: (2, 4) on the C port
  o.watchdog_trigger = 2; o.watchdog_trials = 4;
  if (const char* e = getenv("DTO_WATCHDOG")) sscanf(e, "%d,%d", &o.watchdog_trigger, &o.watchdog_trials);  // experiment knob
  o.newton_only = 0; o.fixed_delta_w = 0.0;
  o.warm = 0; o.mu_warm = 0.0;
  // two-phase line search (k_ls_reduce): l1-penalty while theta_inf > penalty_switch_theta, then Ipopt's filter
  o.ls_penalty = u.line_search == DTO_LS_PENALTY_FILTER ? 1 : 0; o.ls_switch = u.penalty_switch_theta;
  if (const char* e = getenv("DTO_LS_MERIT")) o.ls_penalty = atoi(e);   // experiment knobs (same names as the C port's)
  o.pen_gn = 1;
  o.qn_lbfgs = u.hessian_approximation == DTO_HESSIAN_LBFGS ? 1 : 0;
  o.cost_hess_scale = o.qn_lbfgs ? 0.0 : 1.0;
  if (const char* e = getenv("DTO_PEN_GN")) o.pen_gn = atoi(e);
}

struct BorderStats;

static int bordered_step(Problem* p, const dto_batch* b, const double* mu, int64_t ldmu, const double* dw, double delta_c,
                         double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* ok_out, BorderStats* stats, bool pin_fixed = false,
                         const double* gdiag = nullptr, const double* gshift = nullptr, const BorderBar* bar = nullptr,
                         const BorderSlack* slk = nullptr);
static int general_solve_batch(Problem* p, const dto_options* opt, const dto_batch* b, double* x_out, int64_t ldxo,
                               double* mu_out, int64_t ldmuo, int32_t* status, int32_t* iterations, bool lbfgs = false,
                               const dto_point* start = nullptr, const dto_point* end = nullptr);

// ---- wide-stage models, the linear solver alone: device copies of what dto_kkt_assemble was given.  The factor itself is in
//      p->wide_fac, which dto_kkt_step_batch and the solver write too: each of them clears `factored`
struct WideKkt {
  int64_t B = 0;
  bool assembled = false, factored = false, own_params = false, use_sigx = false, use_sigc = false;
  bool first_order = false;      // dto_kkt_assemble_first_order: W = 0, the multipliers are not read (mu holds zeros)
  double delta_w = 0.0, delta_c = 0.0;
  DevBuf<double> z, mu, params, sigx, sigc;
  DevBuf<int> flags;             // [2][B]: inertia flags, negative-pivot counts
  DevBuf<double> ws;             // [B][T][multi_ws_stage]: intermediates of one block of right-hand sides (dto_kkt_solve_multi), allocated
                                 // by the first multi-solve
  DevBuf<double> ref_r, ref_d;   // [B][Nz + Nc] each: residual and correction (or K sol) of dto_kkt_solve_refined, allocated by its
                                 // first call with passes > 0 or a residual norm to report
};
// ---- both paths: what dto_kkt_border_factor left for dto_kkt_border_solve (dto_border_kernels.hpp).  `valid` is cleared by
//      dto_kkt_assemble, dto_kkt_factor and everything that takes the factor or the assembled system
struct KktBorder {
  bool valid = false;
  int nb = 0;
  int64_t B = 0;
  DevBuf<double> g, y;     // [B * nb][Nz + Nc] each: the panel of border rows (the right-hand sides) and Y = K^-1 G'
  DevBuf<double> part;     // [B][chunks][256]: partial products of k_border_gram
  DevBuf<double> lu, yw;   // [B][256] LU of S, [B][16] border unknowns of the last solve
  DevBuf<double> v0;       // [B][Nz + Nc]: K^-1 r of the last solve
  DevBuf<int> iw;          // [B][16] pivots, then [2][B] flags (negdef, singular)
  // ---- for dto_kkt_border_multiply / dto_kkt_border_solve_refined (tile path)
  int64_t chunk = 0, n_c = 0;   // doubles of k per workgroup and the length of the constraint segment (0: no g_c) the factor call used
  int chunks = 0;
  DevBuf<double> csym;     // [B][256], stride 16: (C + C')/2
  DevBuf<double> tpart;    // [B][chunks][16]: partial G v of k_border_mul
  DevBuf<double> ref_r, ref_d;   // [B][Nz + Nc + 16] each: residual and correction (or M sol) of dto_kkt_border_solve_refined, allocated
                                 // by its first call with passes > 0 or a residual norm to report
  // ---- dto_kkt_lbfgs_border: M [B][nb * nb], the Schur complement before its LU [B][256], sigma [B] and the pair counts [B]
  DevBuf<double> qc, skeep, qsig;
  DevBuf<int> qnp;
};
// constraint rows of K as the border entry points see it: on the tile path the stage part (GeneralConstraint rows, the tail of
// every constraint-side array, are neither read nor written there)
static inline int64_t kkt_rows(const Problem* p) {
  return p->vt->launch_wide ? p->L.Nc - p->L.Ngen : p->L.Nc;
}
// tile path with GeneralConstraint rows: solved by the bordered path of dto_solve_batch only (general_solve_batch): the stepwise
// entry points and per-instance bounds belong to the tile solver, which has no border
static inline int wide_general_refused(const Problem* p, const char* who) {
  if (!p->vt->launch_wide || p->L.Ngen == 0) return DTO_OK;
  return set_error(DTO_ERR_UNSUPPORTED, std::string(who) + ": GeneralConstraint rows on the tile path are solved by the bordered path of "
                                        "dto_solve_batch, which has no stepwise, warm-started or shifted solves and no per-instance bounds");
}
static inline void kkt_border_taken(Problem* p) {
  if (p->kkt_border) p->kkt_border->valid = false;
}
// every other writer of p->wide_fac calls this before it launches
static inline void wide_fac_taken(Problem* p) {
  if (p->wide_kkt) p->wide_kkt->factored = false;
  kkt_border_taken(p);
}
static inline void wide_args_no_linear(dto_wide_args& a) {
  a.sigma_x = a.sigma_c = nullptr; a.ldsx = a.ldsc = 0; a.nneg = nullptr;
  a.rhs_x = a.rhs_c = nullptr; a.ldrx = a.ldrc = 0;
  a.nrhs = a.rhs0 = 0; a.ws = nullptr;
  a.kmul_s = 0;
  a.first_order = 0;
}

// ---- wide-stage models (dto_wide_kernels.hpp): one workgroup per instance, AoS buffers used as they are
static int wide_step(Problem* p, const dto_batch* b, const double* mu, int64_t ldmu, double delta_w, double delta_c,
                     double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* inertia_ok) {
  int rc = p->ensure_device();
  if (rc) return rc;
  dto_wide_info info;
  p->vt->wide_info(&info);
  const Layout& L = p->L;
  if (L.Nstage != 0 || L.Ngen != 0) return set_error(DTO_ERR_UNSUPPORTED, "wide-stage models: dynamics rows and bounds only");
  hipStream_t st = (hipStream_t)b->stream;
  wide_fac_taken(p);
  const size_t need = (size_t)b->B * (size_t)L.T * (size_t)info.fac_stage;
  HIP_TRY(p->wide_fac.grow(need));
  HIP_TRY(p->wide_flags.grow((size_t)b->B));
  dto_wide_args a;
  a.T = L.T; a.B = b->B;
  a.kind = p->d_kind; a.zoff = p->d_zoff; a.woff = p->d_woff; a.cdoff = p->d_cdoff;
  a.params = b->params ? b->params : p->d_params; a.ldw = b->params ? b->ldp : 0;
  a.z = b->x; a.ldz = b->ldx; a.mu = mu; a.ldmu = ldmu;
  a.delta_w = delta_w; a.delta_c = delta_c; a.piv_tol = 1e-9;
  a.dz = dx; a.lddz = lddx; a.dmu = dmu; a.lddmu = lddmu;
  a.fac = p->wide_fac; a.flags = p->wide_flags; a.Nc = L.Nc;
  a.fixed_lo = a.fixed_hi = nullptr; a.ldb = 0; a.dw_inst = nullptr; a.gam_inst = nullptr; a.active = nullptr; a.stats = nullptr; a.merit = nullptr;
  a.zl = a.zu = nullptr; a.mu_inst = nullptr; a.tau_min = 0.99;
  wide_args_no_linear(a);
  a.prof = nullptr;
  if (const char* e = getenv("DTO_WIDE_PROF")) a.prof = (long long*)(uintptr_t)strtoull(e, nullptr, 0);  // debug: device pointer
  const int lrc = p->vt->launch_wide(DTO_WIDE_STEP, &a, (void*)st);
  if (lrc != 0) return hip_fail((hipError_t)lrc, "wide kernel launch");
  if (inertia_ok) {
    std::vector<int> fl((size_t)b->B);
    HIP_TRY(hipMemcpyAsync(fl.data(), p->wide_flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *inertia_ok = 1;
    for (int v : fl) if (!v) *inertia_ok = 0;
  }
  return DTO_OK;
}


// ---- wide-stage models, the linear solver alone (dto_kkt_assemble / dto_kkt_factor / dto_kkt_solve): factor once into
//      p->wide_fac (k_wide_step in its linear-solver mode, terminal block included), then every solve is substitution only
//      (k_wide_fsub + k_wide_bwd).  Bounds are ignored, as on the lane path.
template <class T>
static int grow_buf(DevBuf<T>& buf, size_t need, const char* what) {   // DevBuf::grow with the caller's message for a failure
  const hipError_t e = buf.grow(need);
  return e == hipSuccess ? DTO_OK : hip_fail(e, what);
}
static void wide_kkt_args(Problem* p, dto_wide_args& a) {
  const Layout& L = p->L;
  const WideKkt& K = *p->wide_kkt;
  a.T = L.T; a.B = K.B;
  a.kind = p->d_kind; a.zoff = p->d_zoff; a.woff = p->d_woff; a.cdoff = p->d_cdoff;
  a.params = K.own_params ? K.params : p->d_params; a.ldw = K.own_params ? L.Nw : 0;
  a.z = K.z; a.ldz = L.Nz; a.mu = K.mu; a.ldmu = L.Nc;
  a.delta_w = K.delta_w; a.delta_c = K.delta_c; a.piv_tol = 1e-9;
  a.dz = nullptr; a.lddz = 0; a.dmu = nullptr; a.lddmu = 0;
  // (GeneralConstraint rows, the tail of every constraint-side array, are not part of K: the kernels reach multipliers through
  //  cdoff[t] only, and the inertia test expects one negative pivot per dynamics row)
  a.fac = p->wide_fac; a.flags = K.flags; a.Nc = L.Nc - L.Ngen; a.prof = nullptr;
  a.fixed_lo = a.fixed_hi = nullptr; a.ldb = 0; a.dw_inst = nullptr; a.gam_inst = nullptr; a.active = nullptr; a.stats = nullptr; a.merit = nullptr;
  a.zl = a.zu = nullptr; a.mu_inst = nullptr; a.tau_min = 0.99;
  wide_args_no_linear(a);
  a.first_order = K.first_order ? 1 : 0;
}
static int wide_kkt_assemble(Problem* p, const dto_batch* b, const dto_kkt_system* sys, bool first_order = false) {
  int rc = p->ensure_device();
  if (rc) return rc;
  const Layout& L = p->L;
  // GeneralConstraint rows: K is the stage part, of dimension Nz + Ns (as on the lane path); their entries of mu and sigma_c are
  // not read
  if (L.Nstage != 0) return set_error(DTO_ERR_UNSUPPORTED, "wide-stage models: dynamics rows, GeneralConstraint rows and bounds only");
  const size_t Ns = (size_t)(L.Nc - L.Ngen);
  if (b->B < 1) return set_error(DTO_ERR_INVALID, "empty batch");
  if (b->params && L.Nw > 0 && b->ldp < L.Nw) return set_error(DTO_ERR_INVALID, "ldp < num_parameters");
  if (!p->wide_kkt) p->wide_kkt = new WideKkt();
  WideKkt& K = *p->wide_kkt;
  K.assembled = K.factored = false;
  kkt_border_taken(p);
  dto_wide_info info;
  p->vt->wide_info(&info);
  const size_t B = (size_t)b->B, Nz = (size_t)L.Nz, Nc = (size_t)std::max<int64_t>(1, L.Nc), Nw = (size_t)L.Nw;
  // the factor records: T per instance, the last one for the terminal block
  const size_t need_fac = B * (size_t)L.T * (size_t)info.fac_stage;
  if (const hipError_t e = p->wide_fac.grow(need_fac); e != hipSuccess)
    return hip_fail(e, ("dto_kkt_assemble: hipMalloc of the factor records (" + std::to_string(need_fac * sizeof(double)) + " bytes: " +
                        std::to_string(b->B) + " instances x " + std::to_string(L.T) + " knots x " +
                        std::to_string(info.fac_stage * (int64_t)sizeof(double)) + " bytes)").c_str());
  if ((rc = grow_buf(K.z, B * Nz, "dto_kkt_assemble: hipMalloc of the point"))) return rc;
  if ((rc = grow_buf(K.mu, B * Nc, "dto_kkt_assemble: hipMalloc of the multipliers"))) return rc;
  K.own_params = b->params != nullptr && Nw > 0;
  if (K.own_params && (rc = grow_buf(K.params, B * Nw, "dto_kkt_assemble: hipMalloc of the parameters"))) return rc;
  K.use_sigx = sys->sigma_x != nullptr;
  K.use_sigc = sys->sigma_c != nullptr && Ns > 0;
  if (K.use_sigx && (rc = grow_buf(K.sigx, B * Nz, "dto_kkt_assemble: hipMalloc of sigma_x"))) return rc;
  if (K.use_sigc && (rc = grow_buf(K.sigc, B * Nc, "dto_kkt_assemble: hipMalloc of sigma_c"))) return rc;
  HIP_TRY(K.flags.grow(2 * B));
  hipStream_t st = (hipStream_t)b->stream;
  auto copy = [&](double* dst, size_t n, const double* src, int64_t ld) {
    return hipMemcpy2DAsync(dst, n * sizeof(double), src, (size_t)ld * sizeof(double), n * sizeof(double), B, hipMemcpyDeviceToDevice, st);
  };
  auto copy2 = [&](double* dst, size_t pitch, size_t n, const double* src, int64_t ld) {   // n entries of rows `pitch` apart
    return hipMemcpy2DAsync(dst, pitch * sizeof(double), src, (size_t)ld * sizeof(double), n * sizeof(double), B, hipMemcpyDeviceToDevice, st);
  };
  HIP_TRY(copy(K.z, Nz, b->x, b->ldx));
  if (first_order) HIP_TRY(hipMemsetAsync(K.mu, 0, B * Nc * sizeof(double), st));   // (never part of a result: W = 0)
  else if (Ns > 0) HIP_TRY(copy2(K.mu, Nc, Ns, sys->mu, sys->ldmu));
  if (K.own_params) HIP_TRY(copy(K.params, Nw, b->params, b->ldp));
  if (K.use_sigx) HIP_TRY(copy(K.sigx, Nz, sys->sigma_x, sys->ldsx));
  if (K.use_sigc) HIP_TRY(copy2(K.sigc, Nc, Ns, sys->sigma_c, sys->ldsc));
  // (dto_kkt_factor takes a stream of its own: the copies are complete when this returns)
  HIP_TRY(hipStreamSynchronize(st));
  K.B = b->B; K.delta_w = sys->delta_w; K.delta_c = sys->delta_c;
  K.first_order = first_order;
  K.assembled = true;
  return DTO_OK;
}
static int wide_kkt_factor(Problem* p, int32_t* inertia_ok, int32_t* num_negative, hipStream_t st) {
  if (!p->wide_kkt || !p->wide_kkt->assembled) return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  WideKkt& K = *p->wide_kkt;
  K.factored = false;
  kkt_border_taken(p);
  dto_wide_info info;
  p->vt->wide_info(&info);
  if (p->wide_fac.size() < (size_t)K.B * (size_t)p->L.T * (size_t)info.fac_stage) return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  dto_wide_args a;
  wide_kkt_args(p, a);
  a.sigma_x = K.use_sigx ? K.sigx : nullptr; a.ldsx = p->L.Nz;
  a.sigma_c = K.use_sigc ? K.sigc : nullptr; a.ldsc = std::max<int64_t>(1, p->L.Nc);
  a.nneg = K.flags + K.B;
  const int lrc = p->vt->launch_wide(DTO_WIDE_FACTOR, &a, (void*)st);
  if (lrc != 0) return hip_fail((hipError_t)lrc, "wide factor launch");
  K.factored = true;
  if (inertia_ok || num_negative) {
    std::vector<int> fl(2 * (size_t)K.B);
    HIP_TRY(hipMemcpyAsync(fl.data(), K.flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < K.B; ++i) {
      if (inertia_ok) inertia_ok[i] = fl[(size_t)i] ? 1 : 0;
      if (num_negative) num_negative[i] = fl[(size_t)(K.B + i)];
    }
  }
  return DTO_OK;
}
static int wide_kkt_solve(Problem* p, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc, double* sol_x, int64_t ldsx,
                          double* sol_c, int64_t ldsc, hipStream_t st) {
  if (!p->wide_kkt || !p->wide_kkt->assembled) return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  if (!p->wide_kkt->factored)
    return set_error(DTO_ERR_INVALID, "dto_kkt_factor has not been called (or dto_kkt_step_batch / the solver has used the factor storage since)");
  dto_wide_args a;
  wide_kkt_args(p, a);
  a.rhs_x = rhs_x; a.ldrx = ldrx; a.rhs_c = rhs_c; a.ldrc = ldrc;
  a.dz = sol_x; a.lddz = ldsx; a.dmu = sol_c; a.lddmu = ldsc;
  const int lrc = p->vt->launch_wide(DTO_WIDE_SOLVE, &a, (void*)st);
  if (lrc != 0) return hip_fail((hipError_t)lrc, "wide solve launch");
  return DTO_OK;
}
// nrhs right-hand sides per instance (row b * nrhs + r of every array) in blocks of multi_r columns on the stream: a block reads
// every record once on the way forward and once on the way back.  The records are only read, the intermediates of a block live
// in K.ws, so single and multi solves may follow one another on one factorisation.
static int wide_kkt_solve_multi(Problem* p, int64_t nrhs, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc,
                                double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc, hipStream_t st) {
  if (!p->wide_kkt || !p->wide_kkt->assembled) return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  WideKkt& K = *p->wide_kkt;
  if (!K.factored)
    return set_error(DTO_ERR_INVALID, "dto_kkt_factor has not been called (or dto_kkt_step_batch / the solver has used the factor storage since)");
  dto_wide_info info;
  p->vt->wide_info(&info);
  if (info.multi_r < 1) return set_error(DTO_ERR_UNSUPPORTED, "this plugin was built without the panel substitution kernels");
  const size_t need = (size_t)K.B * (size_t)p->L.T * (size_t)info.multi_ws_stage;
  if (const hipError_t e = K.ws.grow(need); e != hipSuccess)
    return hip_fail(e, ("dto_kkt_solve_multi: hipMalloc of the workspace (" + std::to_string(need * sizeof(double)) + " bytes: " +
                        std::to_string(K.B) + " instances x " + std::to_string(p->L.T) + " knots x " +
                        std::to_string(info.multi_ws_stage * (int64_t)sizeof(double)) + " bytes)").c_str());
  dto_wide_args a;
  wide_kkt_args(p, a);
  a.rhs_x = rhs_x; a.ldrx = ldrx; a.rhs_c = rhs_c; a.ldrc = ldrc;
  a.dz = sol_x; a.lddz = ldsx; a.dmu = sol_c; a.lddmu = ldsc;
  a.nrhs = nrhs; a.ws = K.ws;
  for (int64_t r0 = 0; r0 < nrhs; r0 += info.multi_r) {
    a.rhs0 = r0;
    const int lrc = p->vt->launch_wide(DTO_WIDE_SOLVE_MULTI, &a, (void*)st);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "wide multi-solve launch");
  }
  return DTO_OK;
}

// ---- wide-stage models: helpers of the host-driven solver below (wide_outer)
constexpr int AXPY_BLOCKS_PER_ROW = 64;
static __global__ void k_rows_axpy(double* y, const double* x, const double* alpha, int64_t n, int64_t ldy, int64_t ldx) {
  // grid.x = B * AXPY_BLOCKS_PER_ROW (the instance index lives in grid.x: grid.y is limited to 65535)
  const int64_t b = blockIdx.x / AXPY_BLOCKS_PER_ROW;
  const int64_t blk = blockIdx.x % AXPY_BLOCKS_PER_ROW;
  const double al = alpha[b];
  if (al == 0.0) return;
  for (int64_t i = blk * blockDim.x + threadIdx.x; i < n; i += (int64_t)AXPY_BLOCKS_PER_ROW * blockDim.x)
    y[b * ldy + i] += al * x[b * ldx + i];
}

// ---- wide-stage models: y = K v on the assembled system (k_wide_kmul) and the refined solve built on it.  The product reads what
//      dto_kkt_assemble copied (point, multipliers, parameters, sigmas) and never the factor records, so it needs no
//      factorisation and leaves one alone.
static __global__ void k_rows_residual(double* r, const double* rhs, const double* kx, int64_t n, int64_t ldr, int64_t ldrhs, int64_t ldk) {
  // r = rhs - K x, row by row (grid.x = B * AXPY_BLOCKS_PER_ROW, as k_rows_axpy)
  const int64_t b = blockIdx.x / AXPY_BLOCKS_PER_ROW, blk = blockIdx.x % AXPY_BLOCKS_PER_ROW;
  for (int64_t i = blk * blockDim.x + threadIdx.x; i < n; i += (int64_t)AXPY_BLOCKS_PER_ROW * blockDim.x)
    r[b * ldr + i] = rhs[b * ldrhs + i] - kx[b * ldk + i];
}
static __global__ void k_rows_add(double* y, const double* d, int64_t n, int64_t ldy, int64_t ldd) {
  const int64_t b = blockIdx.x / AXPY_BLOCKS_PER_ROW, blk = blockIdx.x % AXPY_BLOCKS_PER_ROW;
  for (int64_t i = blk * blockDim.x + threadIdx.x; i < n; i += (int64_t)AXPY_BLOCKS_PER_ROW * blockDim.x)
    y[b * ldy + i] += d[b * ldd + i];
}
// out[b] = max |r[b][0 .. n)|: one workgroup of 256 per instance; the maximum does not depend on the order it is taken in
static __global__ __launch_bounds__(256) void k_rows_maxabs(const double* r, int64_t n, int64_t ldr, double* out) {
  __shared__ double part[256];
  const int64_t b = blockIdx.x;
  double m = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) m = fmax(m, fabs(r[b * ldr + i]));
  part[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[b] = part[0];
}
static int wide_kkt_multiply(Problem* p, const double* v_x, int64_t ldvx, const double* v_c, int64_t ldvc, double* out_x, int64_t ldox,
                             double* out_c, int64_t ldoc, hipStream_t st) {
  if (!p->wide_kkt || !p->wide_kkt->assembled) return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  const WideKkt& K = *p->wide_kkt;
  dto_wide_args a;
  wide_kkt_args(p, a);
  a.sigma_x = K.use_sigx ? K.sigx : nullptr; a.ldsx = p->L.Nz;
  a.sigma_c = K.use_sigc ? K.sigc : nullptr; a.ldsc = std::max<int64_t>(1, p->L.Nc);
  a.rhs_x = v_x; a.ldrx = ldvx; a.rhs_c = v_c; a.ldrc = ldvc;
  a.dz = out_x; a.lddz = ldox; a.dmu = out_c; a.lddmu = ldoc;
  // stages per workgroup (0: the kernel's default DTO_WIDE_KMUL_S); the variable is for tools/wide_refine_bench.py, the result does
  // not depend on it
  static const int chunk = [] { const char* e = getenv("DTO_WIDE_KMUL_S"); return e ? std::max(0, atoi(e)) : 0; }();
  a.kmul_s = chunk;
  const int lrc = p->vt->launch_wide(DTO_WIDE_KMUL, &a, (void*)st);
  if (lrc != 0) return hip_fail((hipError_t)lrc, "wide K v launch");
  return DTO_OK;
}
// dto_kkt_solve, then `passes` rounds of r = rhs - K sol, d = K^-1 r against the same records, sol += d; with `resid` one more
// product for max |rhs - K sol| of what is returned.  Residuals are formed in working precision (fixed-precision refinement).
static int wide_kkt_solve_refined(Problem* p, int passes, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc, double* sol_x,
                                  int64_t ldsx, double* sol_c, int64_t ldsc, double* resid, hipStream_t st) {
  int rc = wide_kkt_solve(p, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc, st);
  if (rc || (passes == 0 && !resid)) return rc;
  WideKkt& K = *p->wide_kkt;
  const int64_t Nz = p->L.Nz, Nc = p->L.Nc - p->L.Ngen, ld = Nz + Nc;   // (the stage part: general rows are not touched)
  const size_t need = (size_t)K.B * (size_t)ld;
  const std::string what = "dto_kkt_solve_refined: hipMalloc of a workspace array (" + std::to_string(need * sizeof(double)) + " bytes: " +
                           std::to_string(K.B) + " instances x " + std::to_string(ld) + " doubles)";
  if ((rc = grow_buf(K.ref_r, need, what.c_str()))) return rc;
  if ((rc = grow_buf(K.ref_d, need, what.c_str()))) return rc;
  double *r_x = K.ref_r, *r_c = K.ref_r + Nz, *d_x = K.ref_d, *d_c = K.ref_d + Nz;
  const dim3 grid((unsigned)(K.B * AXPY_BLOCKS_PER_ROW)), block(256);
  auto residual = [&]() -> int {   // ref_r = rhs - K sol (K sol passes through ref_d)
    int e = wide_kkt_multiply(p, sol_x, ldsx, sol_c, ldsc, d_x, ld, d_c, ld, st);
    if (e) return e;
    hipLaunchKernelGGL(k_rows_residual, grid, block, 0, st, r_x, rhs_x, (const double*)d_x, Nz, ld, ldrx, ld);
    if (Nc > 0) hipLaunchKernelGGL(k_rows_residual, grid, block, 0, st, r_c, rhs_c, (const double*)d_c, Nc, ld, ldrc, ld);
    HIP_TRY(hipGetLastError());
    return DTO_OK;
  };
  for (int it = 0; it < passes; ++it) {
    if ((rc = residual())) return rc;
    if ((rc = wide_kkt_solve(p, r_x, ld, r_c, ld, d_x, ld, d_c, ld, st))) return rc;
    hipLaunchKernelGGL(k_rows_add, grid, block, 0, st, sol_x, (const double*)d_x, Nz, ldsx, ld);
    if (Nc > 0) hipLaunchKernelGGL(k_rows_add, grid, block, 0, st, sol_c, (const double*)d_c, Nc, ldsc, ld);
    HIP_TRY(hipGetLastError());
  }
  if (resid) {
    if ((rc = residual())) return rc;
    hipLaunchKernelGGL(k_rows_maxabs, dim3((unsigned)K.B), dim3(256), 0, st, (const double*)K.ref_r, ld, ld, resid);
    HIP_TRY(hipGetLastError());
  }
  return DTO_OK;
}

// ---- finite variable bounds on the wide path (round 4): the barrier bookkeeping around k_wide_step, instance-major ----------
// (lo / hi of instance b at lo[b * ldb]: ldb = 0 for the problem's shared bounds, Nz for those of dto_solver_set_bounds)
// push the guess into the bounds and put the bound multipliers on the central path of mu (Waechter & Biegler 2006, section 3.6;
// the same rule as k_init of the lane-per-instance path)
static __global__ void k_wide_init_bounds(double* z, double* zl, double* zu, const double* lo, const double* hi, int64_t ldb, double mu,
                                          double bound_push, double bound_frac, int64_t n) {
  const int64_t b = blockIdx.x / AXPY_BLOCKS_PER_ROW, blk = blockIdx.x % AXPY_BLOCKS_PER_ROW;
  for (int64_t i = blk * blockDim.x + threadIdx.x; i < n; i += (int64_t)AXPY_BLOCKS_PER_ROW * blockDim.x) {
    double v = z[b * n + i], l = 0.0, u = 0.0;
    const double a = lo[b * ldb + i], c = hi[b * ldb + i];
    if (a == c) v = a;
    else {
      const bool fl = a > -1e300, fh = c < 1e300;
      if (fl && fh) {
        const double pl = fmin(bound_push * fmax(1.0, fabs(a)), bound_frac * (c - a));
        const double pu = fmin(bound_push * fmax(1.0, fabs(c)), bound_frac * (c - a));
        v = fmin(fmax(v, a + pl), c - pu);
      } else if (fl) v = fmax(v, a + bound_push * fmax(1.0, fabs(a)));
      else if (fh) v = fmin(v, c - bound_push * fmax(1.0, fabs(c)));
      if (fl) l = mu / (v - a);
      if (fh) u = mu / (c - v);
    }
    z[b * n + i] = v; zl[b * n + i] = l; zu[b * n + i] = u;
  }
}
// bound multipliers after a step: z_L + alpha_d dz_L with dz_L = mu/(x-lo) - z_L - z_L/(x-lo) dx at the OLD point, kept within
// [mu / (kappa gap'), kappa mu / gap'] of the NEW gap (Ipopt's kappa_Sigma = 1e10 safeguard); runs before z is updated
static __global__ void k_wide_update_bounds(const double* z, const double* dz, double* zl, double* zu, const double* lo, const double* hi,
                                            int64_t ldb, const double* alpha_p, const double* alpha_d, const double* mu, int64_t n) {
  const int64_t b = blockIdx.x / AXPY_BLOCKS_PER_ROW, blk = blockIdx.x % AXPY_BLOCKS_PER_ROW;
  const double ap = alpha_p[b], ad = alpha_d[b], m = mu[b];
  if (ap == 0.0 && ad == 0.0) return;
  constexpr double KSIG = 1e10;
  for (int64_t i = blk * blockDim.x + threadIdx.x; i < n; i += (int64_t)AXPY_BLOCKS_PER_ROW * blockDim.x) {
    const double a = lo[b * ldb + i], c = hi[b * ldb + i];
    if (a == c) continue;
    const double x = z[b * n + i], dx = dz[b * n + i], xn = x + ap * dx;
    if (a > -1e300) {
      const double g = x - a, gn = xn - a, l = zl[b * n + i];
      zl[b * n + i] = fmin(fmax(l + ad * (m / g - l - (l / g) * dx), m / (KSIG * gn)), KSIG * m / gn);
    }
    if (c < 1e300) {
      const double g = c - x, gn = c - xn, u = zu[b * n + i];
      zu[b * n + i] = fmin(fmax(u + ad * (m / g - u + (u / g) * dx), m / (KSIG * gn)), KSIG * m / gn);
    }
  }
}

// warm start (dto_solver_begin_warm on the tile path): the rules of k_init's warm branch -- variables with lo == hi go to their
// bound (whether or not the problem has other finite bounds), the others are pushed into the interior as at a cold start, positive
// bound multipliers of the previous solve are kept and non-positive ones re-initialised to mu / gap with the instance's new mu.
// zl / zu / mu are NULL when the problem has no finite bounds (no barrier).  The dynamics multipliers are not touched.
static __global__ void k_wide_init_warm(double* z, double* zl, double* zu, const double* lo, const double* hi, int64_t ldb, const double* mu,
                                        double bound_push, double bound_frac, int64_t n) {
  const int64_t b = blockIdx.x / AXPY_BLOCKS_PER_ROW, blk = blockIdx.x % AXPY_BLOCKS_PER_ROW;
  const double m = mu ? mu[b] : 0.0;
  for (int64_t i = blk * blockDim.x + threadIdx.x; i < n; i += (int64_t)AXPY_BLOCKS_PER_ROW * blockDim.x) {
    // (the rule itself: warm_var of dto_point_rules.hpp, shared with the bordered loop's k_border_warm_vars)
    const WarmVar w = warm_var(z[b * n + i], lo[b * ldb + i], hi[b * ldb + i], zl != nullptr, zl ? zl[b * n + i] : 0.0, zl ? zu[b * n + i] : 0.0, m,
                               bound_push, bound_frac);
    z[b * n + i] = w.v;
    if (zl) { zl[b * n + i] = w.zl; zu[b * n + i] = w.zu; }
  }
}

// receding horizon on the tile path: out = in moved forward by k knots, instance-major [B][n] with a uniform stride per knot
// (n + m variables, or n dynamics rows).  Block t of out = block min(t + k, T_blocks - 1) of in; in the blocks that enter at the
// end the first last_len entries take the final state (the trailing short block: x_T without an action), the rest repeat the
// last action.  Entries behind the blocks, and rows with keep[j] != 0 (the stage rows an embedded problem carries as dynamics
// rows), keep their values.  One thread per entry, out of place: one read and one write of the array.
static __global__ void k_wide_shift_knots(const double* in, double* out, int64_t n, int64_t total, int stride, int T_blocks,
                                          int last_len, int k, const int* keep) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / n, j = idx % n;
  out[b * n + j] = in[b * n + shift_source(j, stride, T_blocks, last_len, k, keep && keep[j])];
}

// dto_solver_set_bounds: per-instance bounds lo / hi [B][n] against the problem's own slo / shi [n] -- the same pattern (fixed where
// the problem's are, finite lower / upper bounds where the problem's are, lo < hi elsewhere, no NaN).  out[0] counts the entries
// that break it, out[1] is the smallest flat index among them.  One thread per entry.
static __global__ void k_wide_check_bounds(const double* lo, const double* hi, const double* slo, const double* shi, int64_t n,
                                           int64_t total, unsigned long long* out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t j = idx % n;
  const double l = lo[idx], h = hi[idx], sl = slo[j], sh = shi[j];
  const bool fixed = sl == sh;
  const bool ok = l == l && h == h && (l == h) == fixed && isfinite(l) == isfinite(sl) && isfinite(h) == isfinite(sh) && (fixed || l < h);
  if (!ok) {
    atomicAdd(&out[0], 1ull);
    atomicMin(&out[1], (unsigned long long)idx);
  }
}

// ---- the tile-path solver state (dto_solver_begin / iterate / run / end / begin_warm / shift on a wide plugin) ----------------
// Host record of one instance: the shared globalisation record (filter ring, ladder memory, barrier parameter) plus what only this
// path has -- acceptable-level counter, Gauss-Newton fallback of the ladder, and the measures of the current iterate
struct WideInst : GlobInst {
  int full_streak = 0, attempt = 0, acc_count = 0;
  double f_last = 1e300;
  double dw = 0.0, alpha = 0.0, gam = 1.0, gamma_acc = 1.0;
  double f = 0.0, thinf = 0.0, dinf = 0.0;   // at the last convergence test (dto_solver_stats)
};

struct WideState {
  int64_t B = 0, len = 0, n_bnd = 0;  // len: doubles per instance of z / lam / zl / zu / tmp (max(Nz, Nc): the shift swaps them)
  int64_t ldb = 0;                    // lo / hi: [Nz] shared (ldb = 0) or [B][Nz] per instance (ldb = Nz)
  bool barrier = false, begun = false, any_running = false, timed_out = false;
  DevBuf<double> z, lam, dz, dlam, lo, hi, dw, stats, merit, alpha, gam, zl, zu, mu, alphad, params, tmp;
  DevBuf<int> flags, active;
  bool own_params = false;            // the batch's per-instance parameters, copied at the begin ([B][Nw])
  dto_options user{};
  dto_solver_opts opt{};
  std::vector<WideInst> I;
  std::vector<int> h_active, h_flags;
  std::vector<double> h_gam, h_dw, h_stats, h_merit, h_alpha, h_mu, h_alphad;
  std::chrono::steady_clock::time_point t_start;
  int dump_launch = 0, dump_merit = 0;
};

static void release_wide(Problem* p) {
  delete p->wide;
  p->wide = nullptr;
}

void Problem::free_solver() {
  release_wide(this);
  delete wide_kkt; wide_kkt = nullptr;
  delete kkt_border; kkt_border = nullptr;
  delete solver; solver = nullptr;
  delete im; im = nullptr;
}

// device buffers for a batch of B (kept when the batch size is the same)
static int wide_alloc(Problem* p, int64_t B, bool barrier) {
  const Layout& L = p->L;
  if (p->wide && p->wide->B == B && p->wide->z) return DTO_OK;
  release_wide(p);
  p->wide = new WideState();
  WideState& W = *p->wide;
  const int64_t len = std::max<int64_t>(L.Nz, std::max<int64_t>(1, L.Nc));
  const size_t n = (size_t)B * (size_t)len;
  int rc;
  if ((rc = grow_buf(W.z, n, "hipMalloc W.z")) || (rc = grow_buf(W.lam, n, "hipMalloc W.lam")) || (rc = grow_buf(W.tmp, n, "hipMalloc W.tmp")) ||
      (rc = grow_buf(W.dz, (size_t)B * L.Nz, "hipMalloc W.dz")) || (rc = grow_buf(W.dlam, (size_t)B * std::max<int64_t>(1, L.Nc), "hipMalloc W.dlam")) ||
      // (lo / hi are grown to [B][Nz] by wide_begin when per-instance bounds are set)
      (rc = grow_buf(W.lo, L.Nz, "hipMalloc W.lo")) || (rc = grow_buf(W.hi, L.Nz, "hipMalloc W.hi")) ||
      (rc = grow_buf(W.dw, B, "hipMalloc W.dw")) || (rc = grow_buf(W.stats, (size_t)B * DTO_WIDE_NSTAT, "hipMalloc W.stats")) ||
      (rc = grow_buf(W.merit, (size_t)B * 2 * DTO_WIDE_TRIALS, "hipMalloc W.merit")) ||
      (rc = grow_buf(W.alpha, B, "hipMalloc W.alpha")) || (rc = grow_buf(W.gam, B, "hipMalloc W.gam")) ||
      (rc = grow_buf(W.flags, B, "hipMalloc W.flags")) || (rc = grow_buf(W.active, B, "hipMalloc W.active")) ||
      (barrier && ((rc = grow_buf(W.zl, n, "hipMalloc W.zl")) || (rc = grow_buf(W.zu, n, "hipMalloc W.zu")) ||
                   (rc = grow_buf(W.mu, B, "hipMalloc W.mu")) || (rc = grow_buf(W.alphad, B, "hipMalloc W.alphad")))) ||
      (L.Nw > 0 && (rc = grow_buf(W.params, (size_t)B * L.Nw, "hipMalloc W.params")))) {
    release_wide(p);
    return rc;
  }
  W.B = B; W.len = len;
  return DTO_OK;
}

static void wide_fill_args(Problem* p, dto_wide_args& a) {
  const Layout& L = p->L;
  WideState& W = *p->wide;
  a.T = L.T; a.B = W.B;
  a.kind = p->d_kind; a.zoff = p->d_zoff; a.woff = p->d_woff; a.cdoff = p->d_cdoff;
  a.params = W.own_params ? W.params : p->d_params; a.ldw = W.own_params ? L.Nw : 0;
  a.z = W.z; a.ldz = L.Nz; a.mu = W.lam; a.ldmu = L.Nc;
  a.delta_w = 0.0; a.delta_c = W.opt.delta_c; a.piv_tol = W.opt.piv_tol;
  a.dz = W.dz; a.lddz = L.Nz; a.dmu = W.dlam; a.lddmu = L.Nc;
  a.fac = p->wide_fac; a.flags = W.flags; a.Nc = L.Nc; a.prof = nullptr;
  a.fixed_lo = W.lo; a.fixed_hi = W.hi; a.ldb = W.ldb; a.dw_inst = W.dw; a.gam_inst = W.gam; a.active = W.active; a.stats = W.stats; a.merit = W.merit;
  a.zl = W.zl; a.zu = W.zu; a.mu_inst = W.mu; a.tau_min = W.opt.tau_min;
  wide_args_no_linear(a);
}

// the batch's parameters: b->params (DEVICE [B][ldp]) copied into the state, NULL = the problem's shared ones
static int wide_set_params(Problem* p, const dto_batch* b, hipStream_t st) {
  WideState& W = *p->wide;
  const int64_t Nw = p->L.Nw;
  W.own_params = false;
  if (!b->params || Nw == 0) return DTO_OK;
  if (b->ldp < Nw) return set_error(DTO_ERR_INVALID, "ldp < num_parameters");
  HIP_TRY(hipMemcpy2DAsync(W.params, Nw * sizeof(double), b->params, b->ldp * sizeof(double), Nw * sizeof(double), W.B,
                           hipMemcpyDeviceToDevice, st));
  W.own_params = true;
  return DTO_OK;
}

// begin (cold: exactly what dto_solve_batch did before the state existed) or begin_warm
static int wide_begin(Problem* p, const dto_options* opt, const dto_batch* b, bool warm, double mu0) {
  int rc = p->ensure_device();
  if (rc) return rc;
  const Layout& L = p->L;
  if (L.Nstage != 0 || L.Ngen != 0) return set_error(DTO_ERR_UNSUPPORTED, "wide-stage models: dynamics rows and bounds only");
  if (p->wide) p->wide->begun = false;
  wide_fac_taken(p);
  if (warm) {
    if (!p->wide || !p->wide->z || p->wide->B != b->B)
      return set_error(DTO_ERR_INVALID, "dto_solver_begin_warm needs the device state of a previous solve of the same batch size");
  } else if (!b->x) {
    return set_error(DTO_ERR_INVALID, "null argument");
  }
  if (b->x && b->ldx < L.Nz) return set_error(DTO_ERR_INVALID, "ldx < num_variables");
  if (p->d_bnd && p->bnd_B != b->B)
    return set_error(DTO_ERR_INVALID, "dto_solver_set_bounds set bounds for " + std::to_string(p->bnd_B) + " instances, the batch has " +
                                          std::to_string(b->B));
  // finite bounds (lo < hi, one side finite): primal-dual barrier, round 4; n_bnd = number of bound multipliers.  Per-instance
  // bounds (dto_solver_set_bounds) have the problem's pattern, so everything decided here holds for them too
  int64_t n_bnd = 0;
  bool any_fixed = false;
  for (int64_t i = 0; i < L.Nz; ++i) {
    if (L.var_lo[i] != L.var_hi[i]) n_bnd += (std::isfinite(L.var_lo[i]) ? 1 : 0) + (std::isfinite(L.var_hi[i]) ? 1 : 0);
    else any_fixed = true;
  }
  const bool barrier = n_bnd > 0;
  dto_wide_info info;
  p->vt->wide_info(&info);
  const int64_t B = b->B, Nz = L.Nz, Nc = L.Nc;
  hipStream_t st = (hipStream_t)b->stream;
  const size_t need_fac = (size_t)B * (size_t)L.T * (size_t)info.fac_stage;
  HIP_TRY(p->wide_fac.grow(need_fac));
  if ((rc = wide_alloc(p, B, barrier))) return rc;
  WideState& W = *p->wide;
  W.n_bnd = n_bnd; W.barrier = barrier;
  if (opt) W.user = *opt; else dto_options_default(&W.user);
  default_opts(W.opt, W.user);
  if ((rc = wide_set_params(p, b, st))) return rc;
  const dto_solver_opts& o = W.opt;
  // the bounds this batch runs with: the handle's per-instance ones (copied, so that a later dto_solver_set_bounds leaves the
  // begun state alone) or the problem's shared ones
  W.ldb = p->d_bnd ? Nz : 0;
  const size_t lo_len = (size_t)(p->d_bnd ? B * Nz : Nz);
  if (W.lo.size() != lo_len || W.hi.size() != lo_len) {
    W.lo.reset(); W.hi.reset();
    HIP_TRY(W.lo.alloc(lo_len));
    HIP_TRY(W.hi.alloc(lo_len));
  }
  if (p->d_bnd) {
    HIP_TRY(hipMemcpyAsync(W.lo, p->d_bnd, (size_t)B * Nz * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.hi, p->d_bnd + (size_t)B * Nz, (size_t)B * Nz * sizeof(double), hipMemcpyDeviceToDevice, st));
  } else {
    HIP_TRY(hipMemcpyAsync(W.lo, L.var_lo.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.hi, L.var_hi.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (!warm) {
    HIP_TRY(hipMemcpy2DAsync(W.z, Nz * sizeof(double), b->x, b->ldx * sizeof(double), Nz * sizeof(double), B, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(W.lam, 0, (size_t)B * std::max<int64_t>(1, Nc) * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(W.dz, 0, (size_t)B * Nz * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(W.dlam, 0, (size_t)B * std::max<int64_t>(1, Nc) * sizeof(double), st));
    if (barrier) {
      hipLaunchKernelGGL(k_wide_init_bounds, dim3((unsigned)(B * AXPY_BLOCKS_PER_ROW)), dim3(256), 0, st, W.z, W.zl, W.zu, (const double*)W.lo,
                         (const double*)W.hi, W.ldb, o.mu_init, o.bound_push, o.bound_frac, Nz);
      HIP_TRY(hipGetLastError());
    } else if (any_fixed) {
      // no finite bounds besides the fixed variables: put those on their values (the guess may miss them -- a measured state
      // pinned by bounds).  k_wide_init_warm without multipliers does exactly that: the other variables are free on both sides
      hipLaunchKernelGGL(k_wide_init_warm, dim3((unsigned)(B * AXPY_BLOCKS_PER_ROW)), dim3(256), 0, st, W.z, (double*)nullptr,
                         (double*)nullptr, (const double*)W.lo, (const double*)W.hi, W.ldb, (const double*)nullptr, o.bound_push,
                         o.bound_frac, Nz);
      HIP_TRY(hipGetLastError());
    }
    W.I.assign((size_t)B, WideInst());
    W.h_active.assign((size_t)B, 0); W.h_flags.assign((size_t)B, 0);
    W.h_gam.assign((size_t)B, 1.0);
    W.h_dw.assign((size_t)B, 0.0); W.h_stats.assign((size_t)B * DTO_WIDE_NSTAT, 0.0);
    W.h_merit.assign((size_t)B * 2 * DTO_WIDE_TRIALS, 0.0); W.h_alpha.assign((size_t)B, 0.0);
    W.h_mu.assign((size_t)B, barrier ? o.mu_init : 0.0); W.h_alphad.assign((size_t)B, 0.0);
    for (auto& s : W.I) s.mu = barrier ? o.mu_init : 0.0;
  } else {
    // every host record starts afresh as k_init resets its scalars (status, iterations, filter, ladder memory, theta_max /
    // theta_min, acceptable-level counter); the barrier parameter stays unless mu0 > 0
    if (b->x) HIP_TRY(hipMemcpy2DAsync(W.z, Nz * sizeof(double), b->x, b->ldx * sizeof(double), Nz * sizeof(double), B, hipMemcpyDeviceToDevice, st));
    for (int64_t i = 0; i < B; ++i) {
      WideInst& s = W.I[(size_t)i];
      const double m = !barrier ? 0.0 : (mu0 > 0.0 ? mu0 : (s.mu > 0.0 ? s.mu : o.mu_init));
      s = WideInst();
      s.mu = m;
      W.h_mu[(size_t)i] = m;
      W.h_gam[(size_t)i] = 1.0;
    }
    if (barrier) HIP_TRY(hipMemcpyAsync(W.mu, W.h_mu.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_wide_init_warm, dim3((unsigned)(B * AXPY_BLOCKS_PER_ROW)), dim3(256), 0, st, W.z, W.zl, W.zu, (const double*)W.lo,
                       (const double*)W.hi, W.ldb, (const double*)W.mu, o.bound_push, o.bound_frac, Nz);
    HIP_TRY(hipGetLastError());
  }
  if (barrier && !warm) HIP_TRY(hipMemcpyAsync(W.mu, W.h_mu.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
  W.dump_launch = W.dump_merit = 0;
  W.t_start = std::chrono::steady_clock::now();   // Options.max_cpu_time counts from here
  W.timed_out = false;
  W.any_running = true;
  W.begun = true;
  p->hessian_mode_last = DTO_HESSIAN_EXACT;
  return DTO_OK;
}

// debug (tools/wide_debug.py), DTO_WIDE_DUMP=<prefix>, for the first DTO_WIDE_DUMP_MAX (default 1) of each: <prefix>_L<k>_<what>.bin --
// everything factorisation launch k produced (factor records, step, statistics, flags) plus its inputs -- or, merit = true,
// <prefix>_M<k>_merit.bin: the line-search table of iteration k
static void wide_debug_dump(Problem* p, bool merit) {
  const char* prefix = getenv("DTO_WIDE_DUMP");
  if (!prefix) return;
  WideState& W = *p->wide;
  int& count = merit ? W.dump_merit : W.dump_launch;
  if (count >= (getenv("DTO_WIDE_DUMP_MAX") ? atoi(getenv("DTO_WIDE_DUMP_MAX")) : 1)) return;
  char fn[1024];
  if (merit) {
    snprintf(fn, sizeof(fn), "%s_M%d_merit.bin", prefix, count);
    if (FILE* f = fopen(fn, "wb")) { fwrite(W.h_merit.data(), sizeof(double), W.h_merit.size(), f); fclose(f); }
  } else {
    auto wr = [&](const char* what, const void* dptr, size_t bytes) {
      std::vector<char> hb(bytes);
      if (hipMemcpy(hb.data(), dptr, bytes, hipMemcpyDeviceToHost) != hipSuccess) return;
      snprintf(fn, sizeof(fn), "%s_L%d_%s.bin", prefix, count, what);
      if (FILE* f = fopen(fn, "wb")) { fwrite(hb.data(), 1, bytes, f); fclose(f); }
    };
    const Layout& L = p->L;
    const size_t B = (size_t)W.B, nz = B * L.Nz * sizeof(double), nc = B * std::max<int64_t>(1, L.Nc) * sizeof(double);
    dto_wide_info info;
    p->vt->wide_info(&info);
    wr("fac", p->wide_fac, B * (size_t)L.T * (size_t)info.fac_stage * sizeof(double));
    wr("dz", W.dz, nz);
    wr("dlam", W.dlam, nc);
    wr("z", W.z, nz);
    wr("lam", W.lam, nc);
    wr("stats", W.stats, B * DTO_WIDE_NSTAT * sizeof(double));
    wr("flags", W.flags, B * sizeof(int));
    wr("dw", W.dw, B * sizeof(double));
    wr("active", W.active, B * sizeof(int));
  }
  ++count;
}

// ------------------------------------------------------------------------------------------------
// Solver for wide-stage models (configs[4]): the same filter line-search SQP iteration as the register path, driven from
// the host -- one iteration costs a dense block factorisation per instance (hundreds of milliseconds at T = 2000), so a
// few stream synchronisations per iteration are free.  wide_outer = one outer iteration of every running instance; its host
// arithmetic is the phases A - E below, the rules they share with the bordered path are in dto_host_globalization.hpp.
// ------------------------------------------------------------------------------------------------
// ---- A: delta_w of the first factorisation attempt of every running instance, on the exact Hessian of the Lagrangian
static void wide_first_delta_w(WideState& W) {
  const dto_solver_opts& o = W.opt;
  for (size_t i = 0; i < (size_t)W.B; ++i) {
    WideInst& s = W.I[i];
    W.h_active[i] = s.status == 0;
    if (s.status != 0) continue;
    s.attempt = 0;
    if (s.ls_fail) s.dw = ladder_after_ls_fail(o, s.dlast);
    else if (s.dlast > 1.1 * o.delta_w_min && s.full_streak < 2) s.dw = std::max(o.delta_w_min, o.kappa_w_minus * s.dlast);
    else s.dw = 0.0;
    s.gam = 1.0;
    W.h_dw[i] = s.dw;
    W.h_gam[i] = 1.0;
  }
}

// ---- B: convergence test at the current iterate (Ipopt's scaled error, reference Options tolerances) and monotone barrier update
//      (Waechter & Biegler (7)) with mu_target as the floor.  Terminated instances leave h_active; true when the barrier parameter
//      of some instance moved
static bool wide_convergence(WideState& W, int64_t Nc) {
  const dto_solver_opts& o = W.opt;
  bool mu_moved = false;
  for (size_t i = 0; i < (size_t)W.B; ++i) {
    if (!W.h_active[i]) continue;
    WideInst& s = W.I[i];
    const double* sv = &W.h_stats[i * DTO_WIDE_NSTAT];
    const double f = sv[DTO_WIDE_F], th1 = sv[DTO_WIDE_TH1], thinf = sv[DTO_WIDE_THINF], dinf = sv[DTO_WIDE_DINF];
    s.f = f; s.thinf = thinf; s.dinf = dinf;
    // Ipopt's scaling with the bound multipliers included; complementarity measured against mu_target (as k_conv does)
    const ErrScale es = ipopt_scaling(o, sv[DTO_WIDE_SUMLAM], Nc, W.barrier ? sv[DTO_WIDE_SUMZ] : 0.0, W.n_bnd);
    auto compl_at = [&](double m) {
      if (!W.barrier) return 0.0;
      const double szmin = sv[DTO_WIDE_ISZMAX] > 0.0 ? 1.0 / sv[DTO_WIDE_ISZMAX] : 1e300;
      return std::max(sv[DTO_WIDE_SZMAX] - m, m - szmin);
    };
    const double c0 = compl_at(o.mu_target);
    const IterMeasures m{f, th1, thinf, dinf, std::max(std::max(dinf / es.sd, thinf), c0 / es.sc), c0};
    s.acc_count = acceptable_point(o, m, s.f_last) ? s.acc_count + 1 : 0;
    s.f_last = f;
    s.status = terminal_status(o, s.iter, m, s.acc_count);
    if (s.status == 0 && W.barrier) {
      const double mu = monotone_mu(o, s.mu, std::max(dinf / es.sd, thinf), es.sc, compl_at);
      if (mu != s.mu) { s.mu = mu; W.h_mu[i] = mu; s.filter_n = 0; mu_moved = true; }
    }
    init_theta_limits(s, th1);
    if (s.status != 0) W.h_active[i] = 0;
  }
  return mu_moved;
}

// ---- C: inertia of the factorisations just made (Algorithm IC).  Accepted: the instance leaves h_active and its flag becomes 2
//      ("step available").  Rejected: the next rung -- the ladder of k_kkt_sep, exact Hessian up to delta_w_exact_cap, then the
//      constraint curvature is dropped (Gauss-Newton) instead of inflating delta_w further: large delta_w only inflates the
//      multipliers it fights.  True when some instance needs another attempt
static bool wide_inertia_verdict(WideState& W) {
  const dto_solver_opts& o = W.opt;
  bool again = false;
  for (size_t i = 0; i < (size_t)W.B; ++i) {
    if (!W.h_active[i]) continue;
    WideInst& s = W.I[i];
    if (W.h_flags[i] || s.attempt >= o.max_refactor) {
      if (s.dw > 0.0 && s.gam != 0.0) s.dlast = s.dw;
      if (s.dw == 0.0) s.dlast = 0.0;
      s.gamma_acc = s.gam;
      if (!W.h_flags[i]) s.ls_fail = 1;
      W.h_active[i] = 0;
      W.h_flags[i] = 2;
      continue;
    }
    if (s.gam != 0.0) {
      const bool skip_ladder = (s.gamma_acc == 0.0) && (s.iter % 4 != 0);
      if (!skip_ladder) s.dw = ladder_next(o, s.dw, s.dlast);
      if (skip_ladder || s.dw > o.delta_w_exact_cap) { s.gam = 0.0; s.dw = o.delta_w_init; }
    } else {
      s.dw = std::min(s.dw * o.kappa_w_plus, o.delta_w_max);
    }
    s.attempt++;
    W.h_dw[i] = s.dw;
    W.h_gam[i] = s.gam;
    again = true;
  }
  return again;
}

// ---- D: filter line search over the merit table of the trial steps alpha_pmax 2^-k: h_alpha, h_alphad.  With finite bounds
//      phi = f - mu sum log(gaps) (the merit kernel adds the same terms at the trial points), alpha_pmax is the fraction-to-the-
//      boundary step and the bound multipliers take the dual step alpha_dmax
static void wide_line_search(WideState& W) {
  for (size_t i = 0; i < (size_t)W.B; ++i) {
    W.h_alpha[i] = 0.0;
    if (!W.h_active[i]) continue;
    WideInst& s = W.I[i];
    const double* sv = &W.h_stats[i * DTO_WIDE_NSTAT];
    const double* mv = &W.h_merit[i * 2 * DTO_WIDE_TRIALS];
    const double amax = W.barrier ? sv[DTO_WIDE_APMAX] : 1.0;
    const double th0 = sv[DTO_WIDE_TH1], phi0 = sv[DTO_WIDE_F] - (W.barrier ? s.mu * sv[DTO_WIDE_LOGBAR] : 0.0), dphi = sv[DTO_WIDE_GPHID];
    double alpha = amax, accepted = -1.0;
    bool ftype = false;
    MostFeasible best;
    for (int k = 0; k < DTO_WIDE_TRIALS; ++k, alpha *= 0.5) {
      note_most_feasible(best, k, mv[2 * k + 1]);
      const TrialVerdict v = trial_acceptable(s, th0, phi0, dphi, alpha, mv[2 * k + 1], mv[2 * k]);
      if (v != TRIAL_REJECTED) { accepted = alpha; ftype = v == TRIAL_ACCEPTED_FTYPE; break; }
    }
    const double chosen = finish_line_search(s, accepted, ftype, best, th0, phi0, amax, DTO_WIDE_TRIALS, 0);
    s.alpha = chosen;
    s.full_streak = (chosen >= amax) ? s.full_streak + 1 : 0;
    W.h_alphad[i] = W.barrier ? sv[DTO_WIDE_ADMAX] : 0.0;
    if (i == 0 && getenv("DTO_WIDE_VERBOSE"))
      fprintf(stderr, "it %3d f %.6e th1 %.3e thinf %.3e dinf %.3e dphi %.3e dw %.2e att %d alpha %.4g lsfail %d | f(1) %.6e th(1) %.3e f(.5) %.6e th(.5) %.3e\n",
              s.iter, phi0, th0, sv[DTO_WIDE_THINF], sv[DTO_WIDE_DINF], dphi, s.dw, s.attempt, chosen, s.ls_fail, mv[0], mv[1], mv[2], mv[3]);
    s.iter++;
    W.h_alpha[i] = chosen;
  }
}

// ---- E: take the steps (bound multipliers first: their update reads the old point)
static int wide_take_steps(Problem* p, hipStream_t st) {
  WideState& W = *p->wide;
  const int64_t B = W.B, Nz = p->L.Nz, Nc = p->L.Nc;
  const dim3 grid((unsigned)(B * AXPY_BLOCKS_PER_ROW));
  HIP_TRY(hipMemcpyAsync(W.alpha, W.h_alpha.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
  if (W.barrier) {
    for (size_t i = 0; i < (size_t)B; ++i) if (W.h_alpha[i] == 0.0) W.h_alphad[i] = 0.0;
    HIP_TRY(hipMemcpyAsync(W.alphad, W.h_alphad.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_wide_update_bounds, grid, dim3(256), 0, st, (const double*)W.z, (const double*)W.dz, (double*)W.zl, (double*)W.zu,
                       (const double*)W.lo, (const double*)W.hi, W.ldb, (const double*)W.alpha, (const double*)W.alphad, (const double*)W.mu, Nz);
  }
  hipLaunchKernelGGL(k_rows_axpy, grid, dim3(256), 0, st, (double*)W.z, (const double*)W.dz, (const double*)W.alpha, Nz, Nz, Nz);
  if (Nc > 0) hipLaunchKernelGGL(k_rows_axpy, grid, dim3(256), 0, st, (double*)W.lam, (const double*)W.dlam, (const double*)W.alpha, Nc, Nc, Nc);
  return DTO_OK;
}

static int wide_outer(Problem* p, hipStream_t st) {
  WideState& W = *p->wide;
  const int64_t B = W.B;
  dto_wide_args a;
  wide_fill_args(p, a);
  auto launch = [&](int op) -> int {
    if (op == DTO_WIDE_STEP) wide_fac_taken(p);
    return p->vt->launch_wide(op, &a, (void*)st);
  };
  wide_first_delta_w(W);
  for (bool first_pass = true;; first_pass = false) {
    HIP_TRY(hipMemcpyAsync(W.active, W.h_active.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.dw, W.h_dw.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.gam, W.h_gam.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
    { const int lrc = launch(DTO_WIDE_STEP); if (lrc) return hip_fail((hipError_t)lrc, "wide step"); }
    HIP_TRY(hipMemcpyAsync(W.h_flags.data(), W.flags, B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(W.h_stats.data(), W.stats, W.h_stats.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    wide_debug_dump(p, false);
    if (first_pass && wide_convergence(W, p->L.Nc)) {
      // the step just computed belongs to the old mu: it (and the statistics) are evaluated again with the new one before the
      // inertia of that factorisation is judged; nothing of the ladder advances in this pass
      HIP_TRY(hipMemcpyAsync(W.mu, W.h_mu.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
      continue;
    }
    if (!wide_inertia_verdict(W)) break;
  }
  W.any_running = false;
  for (size_t i = 0; i < (size_t)B; ++i) {
    W.h_active[i] = W.I[i].status == 0;
    W.any_running = W.any_running || W.h_active[i];
  }
  if (!W.any_running) return DTO_OK;
  HIP_TRY(hipMemcpyAsync(W.active, W.h_active.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  { const int lrc = launch(DTO_WIDE_MERIT); if (lrc) return hip_fail((hipError_t)lrc, "wide merit"); }
  HIP_TRY(hipMemcpyAsync(W.h_merit.data(), W.merit, W.h_merit.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  wide_debug_dump(p, true);
  wide_line_search(W);
  const int rc = wide_take_steps(p, st);
  if (rc) return rc;
  if (W.user.max_cpu_time > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - W.t_start).count() > W.user.max_cpu_time)
    W.timed_out = true;
  return DTO_OK;
}

// n outer iterations of the running instances (fewer when every instance has terminated or max_cpu_time has expired)
static int wide_iterate(Problem* p, int64_t n, hipStream_t st) {
  WideState& W = *p->wide;
  for (int64_t k = 0; k < n && W.any_running && !W.timed_out; ++k) {
    const int rc = wide_outer(p, st);
    if (rc) { W.begun = false; return rc; }
  }
  return DTO_OK;
}

static int wide_end(Problem* p, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, hipStream_t st) {
  WideState& W = *p->wide;
  const Layout& L = p->L;
  if (x_out) {
    if (ldxo < L.Nz) return set_error(DTO_ERR_INVALID, "ldxo < num_variables");
    HIP_TRY(hipMemcpy2DAsync(x_out, ldxo * sizeof(double), W.z, L.Nz * sizeof(double), L.Nz * sizeof(double), W.B, hipMemcpyDeviceToDevice, st));
  }
  if (mu_out && L.Nc > 0) {
    if (ldmuo < L.Nc) return set_error(DTO_ERR_INVALID, "ldmuo < num_constraint");
    HIP_TRY(hipMemcpy2DAsync(mu_out, ldmuo * sizeof(double), W.lam, L.Nc * sizeof(double), L.Nc * sizeof(double), W.B, hipMemcpyDeviceToDevice, st));
  }
  return DTO_OK;
}

static int wide_run(Problem* p, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, int32_t* status, int32_t* iterations,
                    hipStream_t st) {
  WideState& W = *p->wide;
  int rc = wide_iterate(p, INT64_MAX, st);
  if (rc) return rc;
  if ((rc = wide_end(p, x_out, ldxo, mu_out, ldmuo, st))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  for (int64_t i = 0; i < W.B; ++i) {
    // Options.max_cpu_time expired: the running instances come back with DTO_STATUS_CPU_TIME
    if (status) status[i] = (W.I[(size_t)i].status == 0 && W.timed_out) ? DTO_STATUS_CPU_TIME : W.I[(size_t)i].status;
    if (iterations) iterations[i] = W.I[(size_t)i].iter;
  }
  return DTO_OK;
}

// per-instance scalar of the tile path; false for slots the host loop does not keep
static bool wide_scalar(const WideInst& s, int slot, double* v) {
  switch (slot) {
    case SC_STATUS: *v = s.status; return true;
    case SC_ITER: *v = s.iter; return true;
    case SC_MU: *v = s.mu; return true;
    case SC_DELTA_W: *v = s.dw; return true;
    case SC_ALPHA: *v = s.alpha; return true;
    case SC_F: *v = s.f; return true;
    case SC_THETA_INF: *v = s.thinf; return true;
    case SC_DINF: *v = s.dinf; return true;
    case SC_LS_FAIL: *v = s.ls_fail; return true;
    case SC_DELTA_LAST: *v = s.dlast; return true;
    case SC_THETA_MAX: *v = s.theta_max; return true;
    case SC_THETA_MIN: *v = s.theta_min; return true;
    case SC_FILTER_N: *v = s.filter_n; return true;
    case SC_FULL_STREAK: *v = s.full_streak; return true;
    case SC_ACC_COUNT: *v = s.acc_count; return true;
    case SC_F_LAST: *v = s.f_last; return true;
    default: return false;
  }
}

// receding horizon: z, the dynamics multipliers and z_L / z_U moved forward by `knots` knots (k_wide_shift_knots into the spare
// buffer, then the two are swapped); rows marked by dto_solver_shift_keep_rows keep their multipliers
static int wide_shift(Problem* p, int knots, hipStream_t st) {
  if (!p->wide || !p->wide->z || p->wide->I.empty())
    return set_error(DTO_ERR_INVALID, "dto_solver_shift needs the device state of a previous solve");
  if (knots == 0) return DTO_OK;
  WideState& W = *p->wide;
  const Layout& L = p->L;
  const int T = L.T;
  if (knots >= T - 1) return set_error(DTO_ERR_INVALID, "shift by fewer knots than the horizon has");
  for (int t = 1; t < T; ++t)
    if (L.nx[t] != L.nx[0] || (t < T - 1 && L.nu[t] != L.nu[0]))
      return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_shift needs the same state / action dimensions at every knot");
  const int nx = L.nx[0], nu = L.nu[0];
  if (L.Ndyn != (int64_t)(T - 1) * nx || L.Nc != L.Ndyn || L.Nz != (int64_t)(T - 1) * (nx + nu) + nx)
    return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_shift: unexpected variable / dynamics row count");
  auto shift = [&](DevBuf<double>& buf, int64_t n, int stride, int last_len, const int* keep) -> int {
    const int64_t total = W.B * n;
    if (total == 0) return DTO_OK;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffff) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_shift: batch too large");
    hipLaunchKernelGGL(k_wide_shift_knots, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)buf, W.tmp, n, total, stride,
                       T - 1, last_len, knots, keep);
    HIP_TRY(hipGetLastError());
    std::swap(buf, W.tmp);   // every buffer holds B x len doubles
    return DTO_OK;
  };
  int rc;
  if ((rc = shift(W.z, L.Nz, nx + nu, nx, nullptr))) return rc;
  if ((rc = shift(W.lam, L.Nc, nx, 0, p->d_shift_keep))) return rc;
  if (W.zl) {
    if ((rc = shift(W.zl, L.Nz, nx + nu, nx, nullptr))) return rc;
    if ((rc = shift(W.zu, L.Nz, nx + nu, nx, nullptr))) return rc;
  }
  return DTO_OK;
}

// switch the number of chunks among those the state was allocated for (dto_solver_repack; back to P0 when a batch is loaded)
// Inertia-correction rounds the sequential sweep does per launch (0 = all of them in one launch).  DTO_FWD_ROUNDS is a
// measurement knob (tools/), not part of the interface.
// Back substitutions next to the draining forward launch (csrc/dto_kkt_kernels.hpp: k_kkt_bwd_early): sequential form with
// more tiles than wavefront slots (1 024 at one wavefront per SIMD), all rounds in one forward launch, the caller's stream not being captured into a graph.
// DTO_OVERLAP_SWEEPS=0 switches it off (read at every call: tests flip it).
static bool overlap_sweeps(Problem* p, hipStream_t st) {
  SolverState& S = *p->solver;
  if (const char* e = getenv("DTO_OVERLAP_SWEEPS")) if (atoi(e) == 0) return false;
  const int tiles = S.G_active > 0 ? S.G_active : S.G;
  // pays as soon as the tiles do not all fit the 1 024 wavefront slots at once (measured with the gate: 66 560 instances 37.1
  // vs 41.7 ms per iteration, 90 112: 42.1 vs 44.9, 131 072: 53.7 vs 55.9, 524 288: 199.5 vs 206.7; 65 536: 29.9 vs 29.6)
  static const int min_tiles = [] { const char* e = getenv("DTO_OVERLAP_MIN_TILES"); return e ? atoi(e) : 1024; }();
  if (S.P != 1 || tiles <= min_tiles || S.opt.newton_only) return false;
  static const int per = [] { const char* e = getenv("DTO_FWD_ROUNDS"); return e ? atoi(e) : 0; }();
  if (per > 0) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return false;
  if (!S.stream_lo) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return false;
    if (hipStreamCreateWithPriority(&S.stream_lo, hipStreamNonBlocking, lo) != hipSuccess) { S.stream_lo = nullptr; return false; }
    if (hipEventCreateWithFlags(&S.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.ev_join, hipEventDisableTiming) != hipSuccess)
      return false;
  }
  return S.ev_fork && S.ev_join;
}
// chunks of the time-partitioned factorisation for `tiles` tiles when the caller leaves the choice to the library: as many as
// keep every chunk wavefront resident at once while that is at least eight; see below for larger batches
// Round 5 (chunk sweeps with the next stage's rows requested ahead; profiles/r05/partition_sweep_T1000.jsonl, ms per iteration):
//   12 288 instances: 5 chunks 9.3, 8 chunks 7.8;   16 384: 4 -> 9.9, 8 -> 9.6;   20 480: 3 -> 12.3, 6 -> 12.1, 8 -> 12.5;
//   24 576: sequential 18.9, 8 chunks 13.8;   32 768: sequential 20.3, 6 chunks 17.9;   49 152: sequential 24.2, 6 chunks 27.3
// -- beyond one residency the chunk wavefronts queue, and still win up to ~36 000 instances: eight chunks up to 7/16 of the SIMD
// count in tiles, six up to 9/16, the sequential sweeps after that.
static int auto_chunks(int64_t tiles, int n_simd) {
  const int64_t fit = tiles > 0 ? (int64_t)n_simd / tiles : 1;
  if (fit >= 8) return (int)std::min<int64_t>(fit, 64);
  if (tiles * 16 <= (int64_t)7 * n_simd) return 8;
  if (tiles * 16 <= (int64_t)9 * n_simd) return 6;
  return 1;
}
static int fwd_rounds_per_launch() {
  static const int v = [] { const char* e = getenv("DTO_FWD_ROUNDS"); return e ? atoi(e) : 0; }();
  return v;
}

static void set_partitions_now(SolverState& S, int P) {
  if (S.P_cap > S.P0) {            // blocks for q = 1 .. P_cap back to back: block q starts at sum_{r<q} (r + 1)
    int off = 0;
    for (int q = 1; q < P; ++q) off += q + 1;
    S.d_cstart = S.d_cstart_all + off;
  } else {
    S.d_cstart = S.d_cstart_all;
  }
  S.P = P;
}

static int ensure_state(Problem* p, int64_t B, bool allow_general = false) {
  int rc = p->ensure_device();
  if (rc) return rc;
  if (!p->vt->kkt_info || !p->vt->launch_kkt) return set_error(DTO_ERR_UNSUPPORTED, "plugin has no KKT kernels");
  if (!p->solver) p->solver = new SolverState();
  SolverState& S = *p->solver;
  const Layout& L = p->L;
  const int G_new = (int)((B + 63) / 64);
  // chunks: enough wavefronts to put one on every SIMD (4 per CU: 1024 on an MI355X), at least 8 stages per chunk
  int n_simd = 1024;
  {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
      n_simd = 4 * cus;
  }
  // Round 3 (tools/partition_sweep.py, acrobot T = 1000, ms per iteration): the time-partitioned form pays while ALL its chunk
  // wavefronts (512 registers: one per SIMD) are resident at once and there are at least three chunks --
  //   16 384 instances (256 tiles): 4 chunks 12.6, sequential 19.5;   18 432: 3 chunks 15.4, 4 chunks (1 152 waves) 20.1, seq. 20.2;
  //   20 480: 3 chunks 16.0, seq. 20.5;   22 528: 3 chunks (1 056 waves) 24.3, seq. 20.9;   24 576: 2 chunks 22.6, seq. 21.2;
  //   32 768: 2 chunks 25.5, seq. 22.5;   49 152: 2 chunks 41.9, seq. 25.9;   57 344: 43.6 / 28.1
  // -- otherwise the sequential sweeps (one launch for all inertia-correction rounds, next stage in flight) are faster
  int P_new = S.forced_P > 0 ? S.forced_P : auto_chunks(G_new, n_simd);
  // (chunks of at least `min_chunk` stages: every chunk but the first pays for its spike; DTO_MIN_CHUNK is a measurement knob)
  static const int min_chunk = [] { const char* e = getenv("DTO_MIN_CHUNK"); return e ? std::max(1, atoi(e)) : 4; }();
  P_new = std::max(1, std::min(P_new, std::min(64, S.forced_P > 0 ? L.T : std::max(1, L.T / min_chunk))));
  // per-stage state dimensions (dimensions(), src/dynamics.jl:206-211): the sequential sweep takes them as they come; the
  // time-partitioned form assumes one separator size, so such problems run with a single chunk
  bool uniform_nx = true;
  for (int t = 1; t < L.T; ++t) uniform_nx = uniform_nx && (L.nx[t] == L.nx[0]);
  if (!uniform_nx) {
    if (S.forced_P > 1) return set_error(DTO_ERR_UNSUPPORTED, "time partitions need a uniform state dimension (use 0 or 1)");
    P_new = 1;
  }
  // what the chunk arrays would be sized for: a sequential batch (P = 1) with uniform dimensions may later run with up to
  // 8 chunks (dto_solver_repack) -- unless it is so large (more than two residencies of the sequential sweep) that the
  // switch, which waits for <= 512 tiles, would hardly ever come: such a batch stays sequential and stores its carries
  // without the spike coupling (14 instead of 30 rows per acrobot stage: 128 KB per instance at T = 1000)
  const int P_cap_new = (P_new == 1 && uniform_nx && S.forced_P == 0 && (int64_t)G_new <= 2 * (int64_t)n_simd)
                            ? std::max(1, std::min(8, L.T / 8)) : P_new;   // (8 since round 5: auto_chunks)
  // the state is reused only if the chunk layout is the same too (a dto_solver_set_partitions between two batches of one
  // size changes P_cap and with it the carry records: ADVICE r2)
  if (S.B == B && S.z && S.P0 == P_new && S.P_cap == P_cap_new) {
    if (S.info.has_general && !allow_general)
      return set_error(DTO_ERR_UNSUPPORTED, "the in-kernel interior-point iteration has no border for GeneralConstraint rows");
    set_partitions_now(S, S.P0);
    return DTO_OK;
  }
  S.release();   // (keeps forced_P)
  ReleaseOnError<SolverState> guard{&S};
  S.P = S.P0 = P_new;
  S.n_simd = n_simd;
  S.P_cap = P_cap_new;
  const bool seq_only = S.P_cap == 1;
  p->vt->kkt_info(&S.info);
  if (!S.info.supported) return set_error(DTO_ERR_UNSUPPORTED, "the KKT/solver path supports at most 16 stage kinds");
  if (S.info.has_general && !allow_general)
    return set_error(DTO_ERR_UNSUPPORTED, "the in-kernel interior-point iteration has no border for GeneralConstraint rows that couple "
                                          "several knots: such problems are solved by the bordered path of dto_solve_batch");
  S.B = B;
  S.G = (int)((B + 63) / 64);
  S.ioff.assign(L.T + 1, 0); S.recoff.assign(L.T + 1, 0); S.facoff.assign(L.T + 1, 0);
  for (int t = 0; t < L.T; ++t) {
    const int k = L.kind[t];
    S.ioff[t + 1] = S.ioff[t] + S.info.n_ineq[k];
    S.recoff[t + 1] = S.recoff[t] + S.info.rec_size[k];
    S.facoff[t + 1] = S.facoff[t] + (seq_only ? S.info.fac_size_seq[k] : S.info.fac_size[k]);
  }
  S.Ni = S.ioff[L.T]; S.rec_total = S.recoff[L.T]; S.fac_total = S.facoff[L.T];
  // the sweeps address a tile's arrays through 32-bit buffer offsets (rows of 512 bytes): 2^22 rows per array and tile
  for (int64_t rows : {(int64_t)L.Nz, (int64_t)L.Nc, (int64_t)L.Nw, (int64_t)S.Ni, S.rec_total, S.fac_total})
    if (rows >= (int64_t)1 << 22)
      return set_error(DTO_ERR_UNSUPPORTED, "problem too large for the solver path: an array of one instance exceeds 4194303 rows");
  S.n_bnd = S.Ni;
  for (int64_t i = 0; i < L.Nz; ++i) {
    if (L.var_lo[i] == L.var_hi[i]) continue;
    if (std::isfinite(L.var_lo[i])) ++S.n_bnd;
    if (std::isfinite(L.var_hi[i])) ++S.n_bnd;
  }
  {
    // runs of consecutive stages of one kind whose offsets advance by constant strides
    std::vector<dto_stage_run> runs;
    auto bounded = [&](int t) {
      for (int i = L.zoff[t]; i < L.zoff[t] + L.nx[t] + L.nu[t]; ++i)
        if (L.var_lo[i] == L.var_hi[i] || std::isfinite(L.var_lo[i]) || std::isfinite(L.var_hi[i])) return 1;
      return 0;
    };
    auto zstep = [&](int t) { return t + 1 < L.T ? L.zoff[t + 1] - L.zoff[t] : L.nx[t] + L.nu[t]; };
    for (int t = 0; t < L.T;) {
      dto_stage_run r{};
      r.kind = L.kind[t]; r.t0 = t; r.bounded = bounded(t);
      r.z0 = L.zoff[t]; r.cd0 = L.cdoff[t]; r.cc0 = L.ccoff[t]; r.io0 = S.ioff[t]; r.w0 = L.woff[t];
      r.rec0 = S.recoff[t]; r.fac0 = S.facoff[t];
      r.zs = zstep(t);
      int e = t + 1;
      if (e < L.T && L.kind[e] == r.kind && bounded(e) == r.bounded && zstep(e) == r.zs && L.zoff[e] - L.zoff[t] == r.zs) {
        r.cds = L.cdoff[e] - L.cdoff[t]; r.ccs = L.ccoff[e] - L.ccoff[t]; r.ios = S.ioff[e] - S.ioff[t]; r.ws = L.woff[e] - L.woff[t];
        r.recs = S.recoff[e] - S.recoff[t]; r.facs = S.facoff[e] - S.facoff[t];
        for (;; ++e) {
          if (e >= L.T || L.kind[e] != r.kind || bounded(e) != r.bounded || zstep(e) != r.zs) break;
          const int64_t n = e - t;
          if (L.zoff[e] != r.z0 + n * r.zs || L.cdoff[e] != r.cd0 + n * r.cds || L.ccoff[e] != r.cc0 + n * r.ccs ||
              S.ioff[e] != r.io0 + n * r.ios || L.woff[e] != r.w0 + n * r.ws || S.recoff[e] != r.rec0 + n * r.recs ||
              S.facoff[e] != r.fac0 + n * r.facs)
            break;
        }
      }
      r.t1 = e;
      runs.push_back(r);
      t = e;
    }
    S.n_runs = (int)runs.size();
    HIP_TRY(S.d_runs.alloc(runs.size()));
    HIP_TRY(hipMemcpy(S.d_runs, runs.data(), runs.size() * sizeof(dto_stage_run), hipMemcpyHostToDevice));
  }
  const size_t lanes = (size_t)S.G * 64;
  HIP_TRY(S.d_ioff.alloc(L.T + 1));
  HIP_TRY(hipMemcpy(S.d_ioff, S.ioff.data(), (L.T + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(S.d_recoff.alloc(L.T + 1));
  HIP_TRY(hipMemcpy(S.d_recoff, S.recoff.data(), (L.T + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(S.d_facoff.alloc(L.T + 1));
  HIP_TRY(hipMemcpy(S.d_facoff, S.facoff.data(), (L.T + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(S.d_lo.alloc(L.Nz));
  HIP_TRY(S.d_hi.alloc(L.Nz));
  HIP_TRY(hipMemcpy(S.d_lo, L.var_lo.data(), L.Nz * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.d_hi, L.var_hi.data(), L.Nz * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(S.z.alloc_zeroed(lanes * L.Nz));
  HIP_TRY(S.lam.alloc_zeroed(lanes * L.Nc));
  // bound multipliers exist only where a variable has a finite bound that is not a fixing pair (the acrobot has none: 80 KB
  // per instance, 31 GB at the default bench batch); the kernels test the pointer
  if (S.n_bnd > S.Ni) {
    HIP_TRY(S.zl.alloc_zeroed(lanes * L.Nz));
    HIP_TRY(S.zu.alloc_zeroed(lanes * L.Nz));
  }
  HIP_TRY(S.s.alloc_zeroed(lanes * S.Ni));
  HIP_TRY(S.zs.alloc_zeroed(lanes * S.Ni));
  HIP_TRY(S.dz.alloc_zeroed(lanes * L.Nz));
  HIP_TRY(S.dlam.alloc_zeroed(lanes * L.Nc));
  HIP_TRY(S.ds.alloc_zeroed(lanes * S.Ni));
  HIP_TRY(S.rec.alloc_zeroed(lanes * S.rec_total));
  HIP_TRY(S.fac.alloc_zeroed(lanes * S.fac_total));
  // residual / merit partials: one row set per block of DTO_SB stages (k_stage_eval, k_linesearch), not per stage
  // (small batches: fewer stages per wavefront, down to one -- a batch of one then evaluates its T stages on T wavefronts
  //  instead of walking 8 at a time on T / 8: 37 -> ~8 us for the line search of one acrobot T=101 instance; DTO_STAGE_BLOCK sets it)
  {
    const int64_t want = ((int64_t)S.G * L.T) / 1024;
    S.sb = (int)std::max<int64_t>(1, std::min<int64_t>(DTO_SB, want));
    if (const char* e = getenv("DTO_STAGE_BLOCK")) S.sb = std::max(1, std::min((int)DTO_SB, atoi(e)));
  }
  const size_t nblk = ((size_t)L.T + S.sb - 1) / S.sb;
  HIP_TRY(S.part.alloc_zeroed(lanes * nblk * S.info.npart));
  HIP_TRY(S.lspart.alloc_zeroed(lanes * nblk * 2 * S.info.ls_trials));
  HIP_TRY(S.scal.alloc_zeroed(lanes * S.info.nscal));
  HIP_TRY(S.tile_fwd_tag.alloc_zeroed((size_t)S.G + 8));
  HIP_TRY(S.tile_bwd_tag.alloc_zeroed((size_t)S.G + 8));
  HIP_TRY(S.fwd_started.alloc_zeroed(16));
  HIP_TRY(S.filt.alloc_zeroed(lanes * 2 * S.info.filter_cap));
  {
    // chunk boundaries of every P in [1, P_cap] (or of the one fixed P), back to back: block q holds q + 1 entries
    const int q_lo = (S.P_cap > S.P) ? 1 : S.P, q_hi = S.P_cap;
    std::vector<int> all;
    int off_cur = 0;
    for (int q = q_lo; q <= q_hi; ++q) {
      if (q == S.P) off_cur = (int)all.size();
      for (int c = 0; c <= q; ++c) all.push_back((int)(((int64_t)c * L.T) / q));
    }
    S.cstart.assign(all.begin() + off_cur, all.begin() + off_cur + S.P + 1);
    HIP_TRY(S.d_cstart_all.alloc(all.size()));
    HIP_TRY(hipMemcpy(S.d_cstart_all, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
    S.d_cstart = S.d_cstart_all + off_cur;
  }
  HIP_TRY(S.csum.alloc_zeroed(lanes * (size_t)S.P_cap * S.info.chunk_sum_size));
  HIP_TRY(S.sfac.alloc_zeroed(lanes * (size_t)S.P_cap * S.info.sep_fac_size));
  HIP_TRY(S.xsep.alloc_zeroed(lanes * (size_t)S.P_cap * S.info.nx));
  HIP_TRY(S.cacc.alloc_zeroed(lanes * (size_t)S.P_cap * 4));
  HIP_TRY(S.cpart.alloc_zeroed(lanes * (size_t)S.P_cap * 16));
  HIP_TRY(S.csync.alloc_zeroed((size_t)S.G * 4));
  S.h_scal.assign(lanes * S.info.nscal, 0.0);
  // the zero fills and table copies above ran on the null stream; the kernels run on the caller's stream, which may be a
  // non-blocking one: order them once here (allocation time only)
  HIP_TRY(hipDeviceSynchronize());
  guard.s = nullptr;
  return DTO_OK;
}

static void fill_kkt_args(Problem* p, dto_kkt_args& a) {
  SolverState& S = *p->solver;
  const Layout& L = p->L;
  std::memset(&a, 0, sizeof(a));
  a.T = L.T; a.B = S.B; a.G = S.G;
  a.Nz = L.Nz; a.Nc = L.Nc - L.Ngen; a.Ni = S.Ni;   // GeneralConstraint rows (the tail of the multiplier vector) are the host's border
  a.n_mult = L.Nc; a.n_bnd = S.n_bnd;
  a.kind = p->d_kind; a.zoff = p->d_zoff; a.woff = p->d_woff; a.cdoff = p->d_cdoff; a.ccoff = p->d_ccoff;
  a.ioff = S.d_ioff; a.recoff = S.d_recoff; a.facoff = S.d_facoff;
  a.rec_total = S.rec_total; a.fac_total = S.fac_total;
  a.runs = S.d_runs; a.n_runs = S.n_runs;
  a.lo = S.d_lo; a.hi = S.d_hi; a.params = p->d_params;
  a.wtile = S.use_wtile ? S.wtile : nullptr; a.Nw = L.Nw;
  a.sigx = (S.opt.newton_only && S.use_sigx) ? S.sigx : nullptr;
  a.sigc = (S.opt.newton_only && S.use_sigc) ? S.sigc : nullptr;
  a.z_next = nullptr; a.lam_next = nullptr;
  a.tile_fwd_tag = a.tile_bwd_tag = nullptr; a.sweep_tag = 0; a.fwd_started = nullptr;
  a.z = S.z; a.lam = S.lam; a.zl = S.zl; a.zu = S.zu; a.s = S.s; a.zs = S.zs;
  a.dz = S.dz; a.dlam = S.dlam; a.ds = S.ds;
  a.rec = S.rec; a.fac = S.fac; a.part = S.part; a.lspart = S.lspart; a.scal = S.scal; a.filt = S.filt;
  a.inst_of_slot = S.d_inst_of_slot;
  a.fwd_rounds = fwd_rounds_per_launch();
  a.qn = S.qn; a.qn_mode = 0; a.qn_col = 0;
  a.refq = S.refq; a.refvz = S.refvz; a.refvl = S.refvl;
  a.prof = nullptr;
  if (const char* e = getenv("DTO_KKT_PROF")) a.prof = (long long*)(uintptr_t)strtoull(e, nullptr, 0);  // debug: device pointer
  a.P = S.P; a.cstart = S.d_cstart; a.csum = S.csum; a.sfac = S.sfac; a.xsep = S.xsep; a.cacc = S.cacc; a.cpart = S.cpart;
  a.sb = S.sb;
  {
    // the joins of the time-partitioned form inside the launches: batches of at most two tiles (measured, profiles/r05/
    // join_in_launch_sc1_ab.txt: a batch of one gains 7 - 50 % at every chunk count since the join data moves at agent scope;
    // 1 024 - 24 576 instances lose 0 - 5 %).  DTO_FUSE_JOIN=0: off (read at every call: tests flip it); DTO_FUSE_JOIN_TILES: the limit
    const char* e = getenv("DTO_FUSE_JOIN");
    const char* mt = getenv("DTO_FUSE_JOIN_TILES");
    const int max_tiles = mt ? atoi(mt) : 2;
    a.csync = ((!e || atoi(e) != 0) && (S.G_active > 0 ? S.G_active : S.G) <= max_tiles) ? S.csync : nullptr;
  }
  {
    // cyclic reduction over the separators for batches of at most DTO_SEP_CR_MAX_INST instances -- decided by the BATCH, not by
    // how many lanes of a tile happen to need a factorisation: the arithmetic of an instance must not depend on its neighbours
    // (tests/test_entry_points_gpu.py: repacking changes nothing).  DTO_SEP_CR=0: off (read at every call: tests flip it)
    // larger batches with at least 16 chunks: the same elimination on one wavefront per instance (k_kkt_sep_cr) -- the
    // lane-per-instance form walks the separators one after the other: 63 x 4 us at 64 chunks against ~20 us
    const char* e = getenv("DTO_SEP_CR");
    const bool cr_on = !e || atoi(e) != 0;
    a.sep_cr = !cr_on ? 0 : (S.B <= DTO_SEP_CR_MAX_INST ? 1 : (S.P >= 16 ? 2 : 0));
  }
  a.opt = S.opt;
}

// The fused UPDATE+EVAL pass needs a second copy of the iterate and the multipliers (0.07 MB per instance at T = 1000):
// allocated at the first use if the device has the memory to spare; DTO_FUSE_UPDATE=0 switches the pass off (A/B, tests).
static bool fused_update_available(Problem* p) {
  SolverState& S = *p->solver;
  if (const char* e = getenv("DTO_FUSE_UPDATE")) if (atoi(e) == 0) return false;   // read per call: tests flip it
  if (S.opt.qn_lbfgs) return false;   // the limited-memory mode saves its secant data between LS_REDUCE and UPDATE
  if (S.fuse_state != 0) return S.fuse_state > 0;
  S.fuse_state = -1;
  const size_t lanes = (size_t)S.G * 64;
  const size_t need = lanes * (size_t)(p->L.Nz + p->L.Nc) * sizeof(double);
  size_t free_b = 0, total_b = 0;
  // head room left to the caller after the second buffers: an eighth of the device (36 GB of an MI355X's 288; the bench's own
  // buffers at the default batch need 28 GB), DTO_FUSE_RESERVE_GB overrides; dto_solver_footprint reports whether the pass is on
  static const double reserve_gb = [] { const char* e = getenv("DTO_FUSE_RESERVE_GB"); return e ? atof(e) : -1.0; }();
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  const size_t reserve = reserve_gb >= 0.0 ? (size_t)(reserve_gb * 1073741824.0) : total_b / 8;
  if (free_b < need + reserve) return false;
  if (S.z_alt.alloc(lanes * p->L.Nz) != hipSuccess) return false;
  if (S.lam_alt.alloc(lanes * p->L.Nc) != hipSuccess) { S.z_alt.reset(); return false; }
  S.fuse_state = 1;
  return true;
}

// Adjacent tiles per wavefront of the sequential forward sweep (csrc/dto_kkt_kernels.hpp: kkt_fwd_seq_body): the retry rounds
// of a group run on its packed needing lanes.  Only where the tiles outnumber the wavefront slots (one wavefront per SIMD)
// several times over: k = tiles / (4 x compute units), at most DTO_FWD_GROUP_MAX -- below that every tile has a slot of its own
// and grouping would only remove parallelism (65 536 instances, the tail of a full solve).  DTO_FWD_GROUP=1 forces one tile
// per wavefront, n > 1 groups of n whatever the batch (read at every call: tests flip it).  One tile per wavefront whenever a
// launch does not run all its rounds (DTO_FWD_ROUNDS) and for the single factorisation of the linear-solver entry points.
#ifndef DTO_FWD_GROUP_MAX
#define DTO_FWD_GROUP_MAX 4
#endif
static int fwd_group_for(Problem* p, const dto_kkt_args& a) {
  const SolverState& S = *p->solver;
  if (a.P != 1 || a.fwd_rounds > 0 || a.opt.newton_only || a.G < 2) return 1;
  int k = (int)std::min<int64_t>(DTO_FWD_GROUP_MAX, (int64_t)a.G / std::max(1, S.n_simd));
  if (const char* e = getenv("DTO_FWD_GROUP")) { const int v = atoi(e); if (v >= 1) k = std::min(v, 64); }
  // a group's rows of every array stay below 2 GiB: the sweep addresses them with 32-bit offsets inside one buffer resource
  const int64_t rows = std::max<int64_t>({a.Nz, a.Nc, a.Ni, a.Nw, a.rec_total, a.fac_total, 1});
  k = (int)std::min<int64_t>(k, (((int64_t)1 << 31) - 1) / (rows * 512));
  return std::max(1, std::min(k, a.G));
}

static int kkt_launch(Problem* p, int op, const dto_kkt_args& a, hipStream_t st) {
  if ((op == DTO_KKT_FWD || op == DTO_KKT_FACTOR_SOLVE || op == DTO_KKT_BWD_GATE) && a.fwd_group == 0 && p->solver) {
    const int k = fwd_group_for(p, a);
    if (k > 1) {
      dto_kkt_args b = a;
      b.fwd_group = k;
      return kkt_launch(p, op, b, st);
    }
  }
  LaunchTrace* tr = (p->trace && p->trace->on && p->trace->recs.size() < LaunchTrace::MAX_RECS) ? p->trace : nullptr;
  int e0 = -1, e1 = -1;
  if (tr) {
    e0 = tr->take(); e1 = tr->take();
    if (e0 < 0 || e1 < 0) tr = nullptr;
    else HIP_TRY(hipEventRecord(tr->pool[(size_t)e0], st));
  }
  const int rc = p->vt->launch_kkt(op, &a, (void*)st);
  if (rc != 0) return hip_fail((hipError_t)rc, "KKT kernel launch");
  if (tr) {
    HIP_TRY(hipEventRecord(tr->pool[(size_t)e1], st));
    tr->recs.push_back({op, tr->iteration, e0, e1});
  }
  return DTO_OK;
}

// One pass of iterative refinement of the step in dz / dlam (csrc/dto_kkt_kernels.hpp: "iterative refinement"): the residual goes
// into the stage records (a copy of the real ones is kept), `solve` runs the factor + solve of the caller's path once more at the
// accepted (delta_w, gamma), the records come back, and the step becomes saved step + correction with its by-products recomputed.
static int ensure_refine_buffers(Problem* p, dto_kkt_args& a) {
  SolverState& S = *p->solver;
  const size_t lanes = (size_t)S.G * 64;
  if (!S.refq) HIP_TRY(S.refq.alloc_zeroed(lanes * (size_t)p->L.T * (size_t)S.info.nx));
  if (!S.refvz) HIP_TRY(S.refvz.alloc_zeroed(lanes * (size_t)p->L.Nz));
  if (!S.refvl) HIP_TRY(S.refvl.alloc_zeroed(lanes * (size_t)std::max<int64_t>(1, p->L.Nc)));
  if (!S.rec_bak) HIP_TRY(S.rec_bak.alloc_zeroed(lanes * (size_t)S.rec_total));
  a.refq = S.refq; a.refvz = S.refvz; a.refvl = S.refvl;
  return DTO_OK;
}
template <class F>
static int refine_pass(Problem* p, dto_kkt_args& a, hipStream_t st, F&& solve) {
  SolverState& S = *p->solver;
  int rc;
  const size_t rec_bytes = (size_t)a.G * 64 * (size_t)S.rec_total * sizeof(double);
  HIP_TRY(hipMemcpyAsync(S.rec_bak, S.rec, rec_bytes, hipMemcpyDeviceToDevice, st));
  if ((rc = kkt_launch(p, DTO_KKT_REFINE, a, st))) return rc;
  if ((rc = solve())) return rc;
  HIP_TRY(hipMemcpyAsync(S.rec, S.rec_bak, rec_bytes, hipMemcpyDeviceToDevice, st));
  return kkt_launch(p, DTO_KKT_REFINE_APPLY, a, st);
}

static int pack(Problem* p, dto_kkt_args a, int which, const double* src, int64_t ld, hipStream_t st) {
  a.aos_in = src; a.ld_aos = ld; a.aos_which = which;
  return kkt_launch(p, DTO_KKT_PACK, a, st);
}
static int unpack(Problem* p, dto_kkt_args a, int which, double* dst, int64_t ld, hipStream_t st) {
  a.aos_out = dst; a.ld_aos = ld; a.aos_which = which;
  return kkt_launch(p, DTO_KKT_UNPACK, a, st);
}

// per-instance parameters of a batch: packed into SoA tiles next to the iterates (NULL: the problem's shared parameters)
static int set_batch_params(Problem* p, const dto_batch* b, hipStream_t st) {
  SolverState& S = *p->solver;
  S.use_wtile = false;
  if (!b->params || p->L.Nw == 0) return DTO_OK;
  if (b->ldp < p->L.Nw) return set_error(DTO_ERR_INVALID, "ldp < num_parameters");
  if (!S.wtile) HIP_TRY(S.wtile.alloc_zeroed((size_t)S.G * 64 * (size_t)p->L.Nw));
  S.use_wtile = true;
  dto_kkt_args a;
  fill_kkt_args(p, a);
  return pack(p, a, 4, b->params, b->ldp, st);
}

static int fetch_scalars(Problem* p, hipStream_t st) {
  SolverState& S = *p->solver;
  HIP_TRY(hipMemcpyAsync(S.h_scal.data(), S.scal, S.h_scal.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DTO_OK;
}

static inline double hscal(const SolverState& S, int64_t inst, int slot) {
  const int64_t pos = S.slot_of_inst.empty() ? inst : S.slot_of_inst[(size_t)inst];
  return S.h_scal[((pos >> 6) * S.info.nscal + slot) * 64 + (pos & 63)];
}

// identity slot <-> instance map (every entry point that loads a fresh batch)
static void reset_slot_map(SolverState& S) {
  S.d_inst_of_slot.reset();
  S.inst_of_slot.clear(); S.slot_of_inst.clear();
  S.G_active = S.G;
}

static __global__ void k_gather_rows(double* dst, const double* src, int64_t n, const int* src_slot, unsigned nrb) {
  // grid G * nrb (nrb = ceil(n / 4) row blocks; the tile index lives in grid.x: grid.y is limited to 65535);
  // block 256 = 4 rows x 64 lanes: dst[tile][i][lane] = src[tile'][i][lane'], (tile', lane') = src_slot
  const int64_t tile = blockIdx.x / nrb;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)(blockIdx.x % nrb) * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int ss = src_slot[tile * 64 + lane];
  dst[((tile * n + i) << 6) + lane] = src[((((int64_t)(ss >> 6)) * n + i) << 6) + (ss & 63)];
}

// the same for rows [row0, row0 + n) of an array with `total` rows per tile (the limited-memory history block): dst is compact
static __global__ void k_gather_rows_of(double* dst, const double* src, int64_t n, int64_t total, int64_t row0, const int* src_slot,
                                        unsigned nrb) {
  const int64_t tile = blockIdx.x / nrb;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)(blockIdx.x % nrb) * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int ss = src_slot[tile * 64 + lane];
  dst[((tile * n + i) << 6) + lane] = src[((((int64_t)(ss >> 6)) * total + row0 + i) << 6) + (ss & 63)];
}

// Move the instances that are still running to the leading tiles (stable), the finished ones behind them, so that the
// per-iteration kernels only cover tiles with work: without it a batch keeps paying for all its tiles until the last lane
// of each has terminated.  Only the persistent per-instance state moves (iterates, multipliers, filter, scalars,
// per-instance parameters); records, carries and partials are rebuilt by every iteration.  h_scal must be current.
static int repack(Problem* p, hipStream_t st, int* n_running_out) {
  SolverState& S = *p->solver;
  const Layout& L = p->L;
  const int lanes = S.G * 64;
  // (the per-stage SR1 blocks of a plugin without second derivatives live in the records, which do not move: such batches are not
  //  repacked; finished lanes are skipped by every kernel all the same.  The limited-memory history block `qn` moves with its
  //  instance since round 6 -- rounds 5's batches in that mode paid for every tile until its last lane ended)
  if (S.info.quasi_newton) { if (n_running_out) *n_running_out = -1; return DTO_OK; }
  if (S.inst_of_slot.empty()) {
    S.inst_of_slot.resize(lanes); S.slot_of_inst.resize(lanes);
    for (int i = 0; i < lanes; ++i) S.inst_of_slot[i] = S.slot_of_inst[i] = i;
  }
  std::vector<int> src(lanes);
  int nrun = 0, k = 0;
  auto running = [&](int slot) {
    return S.inst_of_slot[slot] < S.B && S.h_scal[(((size_t)slot >> 6) * S.info.nscal + SC_STATUS) * 64 + (slot & 63)] == 0.0;
  };
  for (int sl = 0; sl < lanes; ++sl) if (running(sl)) src[k++] = sl;
  nrun = k;
  for (int sl = 0; sl < lanes; ++sl) if (!running(sl)) src[k++] = sl;
  if (n_running_out) *n_running_out = nrun;
  const int g_new = std::max(1, (nrun + 63) / 64);
  if (g_new >= S.G_active) return DTO_OK;            // nothing to gain
  if (!S.d_src_slot) HIP_TRY(S.d_src_slot.alloc(lanes));
  if (!S.d_inst_of_slot) HIP_TRY(S.d_inst_of_slot.alloc(lanes));
  HIP_TRY(hipMemcpyAsync(S.d_src_slot, src.data(), lanes * sizeof(int), hipMemcpyHostToDevice, st));
  // the staging buffer must hold the widest vector that moves: iterates, multipliers, slacks, filter (2 * filter_cap
  // rows), scalars, per-instance parameters (the filter rows were missing from the maximum)
  int64_t widest = std::max<int64_t>(std::max<int64_t>(L.Nz, L.Nc), std::max<int64_t>(S.info.nscal, L.Nw));
  widest = std::max<int64_t>(widest, std::max<int64_t>(S.Ni, 2 * (int64_t)S.info.filter_cap));
  const size_t need = (size_t)lanes * (size_t)widest;
  HIP_TRY(S.repack_tmp.grow(need));
  auto move = [&](double* buf, int64_t n) -> int {
    if (!buf || n <= 0) return DTO_OK;
    const unsigned nrb = (unsigned)((n + 3) / 4);
    if ((uint64_t)nrb * (uint64_t)S.G > 0x7fffffffull) return set_error(DTO_ERR_INVALID, "batch too large to repack");
    hipLaunchKernelGGL(k_gather_rows, dim3(nrb * (unsigned)S.G), dim3(256), 0, st, S.repack_tmp, (const double*)buf, n,
                       (const int*)S.d_src_slot, nrb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(buf, S.repack_tmp, (size_t)lanes * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    return DTO_OK;
  };
  int rc;
  if ((rc = move(S.z, L.Nz))) return rc;
  if ((rc = move(S.lam, L.Nc))) return rc;
  if (S.n_bnd > S.Ni) { if ((rc = move(S.zl, L.Nz))) return rc; if ((rc = move(S.zu, L.Nz))) return rc; }
  if ((rc = move(S.s, S.Ni))) return rc;
  if ((rc = move(S.zs, S.Ni))) return rc;
  if ((rc = move(S.filt, 2 * S.info.filter_cap))) return rc;
  if ((rc = move(S.scal, S.info.nscal))) return rc;
  if (S.use_wtile && (rc = move(S.wtile, L.Nw))) return rc;
  if (S.opt.qn_lbfgs && S.qn) {
    // history block [G][total][64]: in pieces of at most `widest` rows through the same staging buffer
    const int64_t total = dto::QnRows{L.Nz}.total();
    for (int64_t row0 = 0; row0 < total; row0 += widest) {
      const int64_t n = std::min<int64_t>(widest, total - row0);
      const unsigned nrb = (unsigned)((n + 3) / 4);
      if ((uint64_t)nrb * (uint64_t)S.G > 0x7fffffffull) return set_error(DTO_ERR_INVALID, "batch too large to repack");
      hipLaunchKernelGGL(k_gather_rows_of, dim3(nrb * (unsigned)S.G), dim3(256), 0, st, S.repack_tmp, (const double*)S.qn, n, total, row0,
                         (const int*)S.d_src_slot, nrb);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy2DAsync(S.qn + ((size_t)row0 << 6), (size_t)total * 64 * sizeof(double), S.repack_tmp, (size_t)n * 64 * sizeof(double),
                               (size_t)n * 64 * sizeof(double), (size_t)S.G, hipMemcpyDeviceToDevice, st));
    }
  }
  std::vector<int> inst_new(lanes);
  for (int sl = 0; sl < lanes; ++sl) inst_new[sl] = S.inst_of_slot[src[sl]];
  S.inst_of_slot.swap(inst_new);
  for (int sl = 0; sl < lanes; ++sl) S.slot_of_inst[S.inst_of_slot[sl]] = sl;
  HIP_TRY(hipMemcpyAsync(S.d_inst_of_slot, S.inst_of_slot.data(), lanes * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));   // src / inst_new are host temporaries of this call
  S.G_active = g_new;
  // too few tiles left to fill the wavefront slots of the sequential sweeps: cut the horizon into chunks again (each chunk wave carries a spike, one
  // wavefront per SIMD); the chunk arrays were sized for it when the batch was loaded
  if (S.P_cap > S.P0) {
    // only while the chunk waves (one per SIMD: 512-VGPR kernels) still fit the GPU at once; just above one residency the
    // in-kernel round loop of the sequential form is faster (262 144 instances, full solves: 1.285 M it/s with the switch
    // at 7/8 of the SIMDs, 1.295 M with this rule, 1.304 M without any switch -- the batch never gets that small).
    // The same rule as when a batch is loaded (auto_chunks returns 1 or >= 6; the cstart tables hold every P in [1, P_cap]):
    // two to five chunks were measured slower than the sequential sweeps or than eight (profiles/r05/)
    const int P_new = std::max(1, std::min(S.P_cap, auto_chunks(g_new, S.n_simd)));
    set_partitions_now(S, P_new);
  }
  return fetch_scalars(p, st);         // the host copy of the scalar block follows the move
}

// ------------------------------------------------------------------------------------------------
// instance-major engine: host side.  One PASS = [list EVAL -> residuals, convergence test] [list FACT -> one factorisation
// attempt each] [list STEP -> back substitution, line search, update]; nothing of it waits for the host.
// ------------------------------------------------------------------------------------------------
// engine choice: 0 automatic (instance-major where the SoA engine would run its plain sequential sweep, i.e. at least one
// tile per SIMD), 1 SoA tiles, 2 instance-major.  DTO_ENGINE=soa|im overrides the automatic choice (measurements, tests).
static bool im_supported(Problem* p) {
  if (!p->vt->launch_im || !p->vt->im_info) return false;
  dto_im_info info;
  p->vt->im_info(&info);
  return info.supported != 0;
}

static bool use_im(Problem* p, int64_t B) {
  if (!im_supported(p)) return false;
  int eng = p->engine_req;
  if (eng == 0) {
    if (const char* e = getenv("DTO_ENGINE")) eng = !strcmp(e, "im") ? 2 : (!strcmp(e, "soa") ? 1 : 0);
  }
  if (eng == 2) return true;
  if (eng == 1) return false;
  // automatic: the SoA engine.  Measured (MI355X, acrobot T = 1000, 131 072 instances, 25 iterations): SoA tiles 67 ms per
  // iteration, instance-major 112 ms -- its forward sweep does pay for attempts only (30-34 ms against 35 ms), but its
  // stage kernels (lane = knot) and its backward sweep are 2-2.5x slower than the lane = instance forms; DESIGN.md section 4.4
  (void)B;
  return false;
}

static int ensure_im_state(Problem* p, int64_t B) {
  int rc = p->ensure_device();
  if (rc) return rc;
  if (!p->im) p->im = new ImState();
  ImState& S = *p->im;
  const Layout& L = p->L;
  if (S.B == B && S.A) return DTO_OK;
  S.release();
  ReleaseOnError<ImState> guard{&S};
  p->vt->im_info(&S.info);
  if (!S.info.supported) return set_error(DTO_ERR_UNSUPPORTED, "the instance-major engine needs an exact-Hessian model without GeneralConstraint");
  S.B = B;
  const int T = L.T;
  S.aoff.assign(T + 1, 0); S.doff.assign(T + 1, 0); S.coff.assign(T + 1, 0); S.boff.assign(T + 1, 0); S.ioff.assign(T + 1, 0);
  for (int t = 0; t < T; ++t) {
    const int k = L.kind[t];
    S.aoff[t + 1] = S.aoff[t] + S.info.a_size[k];
    S.doff[t + 1] = S.doff[t] + S.info.d_size[k];
    S.coff[t + 1] = S.coff[t] + S.info.c_size[k];
    S.boff[t + 1] = S.boff[t] + S.info.b_size[k];
    S.ioff[t + 1] = S.ioff[t] + S.info.n_ineq[k];
  }
  S.a_total = S.aoff[T]; S.d_total = S.doff[T]; S.c_total = S.coff[T]; S.b_total = S.boff[T]; S.Ni = S.ioff[T];
  S.n_bnd = S.Ni;
  for (int64_t i = 0; i < L.Nz; ++i) {
    if (L.var_lo[i] == L.var_hi[i]) continue;
    if (std::isfinite(L.var_lo[i])) ++S.n_bnd;
    if (std::isfinite(L.var_hi[i])) ++S.n_bnd;
  }
  S.nwin_e = (T + S.info.own_eval - 1) / S.info.own_eval;
  S.nwin_l = (T + S.info.own_ls - 1) / S.info.own_ls;
  auto table = [&](DevBuf<int>& d, const std::vector<int>& h) -> int {
    HIP_TRY(d.alloc(h.size()));
    HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
    return DTO_OK;
  };
  if ((rc = table(S.d_aoff, S.aoff)) || (rc = table(S.d_doff, S.doff)) || (rc = table(S.d_coff, S.coff)) ||
      (rc = table(S.d_boff, S.boff)) || (rc = table(S.d_ioff, S.ioff)))
    return rc;
  HIP_TRY(S.d_lo.alloc(L.Nz));
  HIP_TRY(S.d_hi.alloc(L.Nz));
  HIP_TRY(hipMemcpy(S.d_lo, L.var_lo.data(), L.Nz * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.d_hi, L.var_hi.data(), L.Nz * sizeof(double), hipMemcpyHostToDevice));
  const size_t nb = (size_t)B;
  // + one record of slack at the end: the sweeps form (never read) the address of the record after the last stage
  HIP_TRY(S.A.alloc_zeroed(nb * (size_t)S.a_total + 16));
  HIP_TRY(S.R.alloc_zeroed(nb * (size_t)S.a_total + 16));
  HIP_TRY(S.D.alloc_zeroed(nb * (size_t)S.d_total + 16));
  HIP_TRY(S.C.alloc_zeroed(nb * (size_t)S.c_total + 16));
  if (S.n_bnd > 0) HIP_TRY(S.Bd.alloc_zeroed(nb * (size_t)S.b_total + 16));
  HIP_TRY(S.part.alloc_zeroed(nb * (size_t)S.nwin_e * S.info.npart));
  HIP_TRY(S.lspart.alloc_zeroed(nb * (size_t)S.nwin_l * 2 * S.info.ls_trials));
  HIP_TRY(S.scal.alloc_zeroed(nb * (size_t)S.info.nscal));
  HIP_TRY(S.filt.alloc_zeroed(nb * 2 * (size_t)S.info.filter_cap));
  HIP_TRY(S.phase.alloc_zeroed(nb));
  HIP_TRY(S.lists.alloc_zeroed(3 * nb));
  HIP_TRY(S.ctr.alloc_zeroed((size_t)8));
  HIP_TRY(hipHostMalloc((void**)&S.h_ctr, 8 * sizeof(int)));
  S.h_scal.assign(nb * S.info.nscal, 0.0);
  HIP_TRY(hipDeviceSynchronize());
  guard.s = nullptr;
  return DTO_OK;
}

static void fill_im_args(Problem* p, dto_im_args& a) {
  ImState& S = *p->im;
  const Layout& L = p->L;
  std::memset(&a, 0, sizeof(a));
  a.T = L.T; a.B = S.B;
  a.Nz = L.Nz; a.Nc = L.Nc; a.Ni = S.Ni; a.Nw = L.Nw;
  a.n_mult = L.Nc; a.n_bnd = S.n_bnd;
  a.kind = p->d_kind; a.zoff = p->d_zoff; a.woff = p->d_woff; a.cdoff = p->d_cdoff; a.ccoff = p->d_ccoff; a.ioff = S.d_ioff;
  a.aoff = S.d_aoff; a.doff = S.d_doff; a.coff = S.d_coff; a.boff = S.d_boff;
  a.a_total = S.a_total; a.d_total = S.d_total; a.c_total = S.c_total; a.b_total = S.b_total;
  a.lo = S.d_lo; a.hi = S.d_hi; a.params = p->d_params;
  a.wpi = S.use_w ? S.wbuf : nullptr; a.ldw = L.Nw;
  a.A = S.A; a.R = S.R; a.D = S.D; a.C = S.C; a.Bd = S.Bd;
  a.part = S.part; a.lspart = S.lspart; a.scal = S.scal; a.filt = S.filt; a.phase = S.phase;
  a.nwin_e = S.nwin_e; a.nwin_l = S.nwin_l;
  a.iter_target = -1;
  a.ticket = S.ctr + 3; a.running = S.ctr + 5;
  // measurement knob: register budget of the sweeps
  static const int occ = [] { const char* e = getenv("DTO_IM_OCC"); return e ? atoi(e) : 2; }();
  a.sweep_occ = occ;
  a.opt = S.opt;
}

static int im_launch(Problem* p, int op, const dto_im_args& a, hipStream_t st) {
  const int rc = p->vt->launch_im(op, &a, (void*)st);
  if (rc != 0) return hip_fail((hipError_t)rc, "instance-major kernel launch");
  return DTO_OK;
}

static int im_set_params(Problem* p, const dto_batch* b, hipStream_t st) {
  ImState& S = *p->im;
  S.use_w = false;
  if (!b->params || p->L.Nw == 0) return DTO_OK;
  if (b->ldp < p->L.Nw) return set_error(DTO_ERR_INVALID, "ldp < num_parameters");
  if (!S.wbuf) HIP_TRY(S.wbuf.alloc_zeroed((size_t)S.B * (size_t)p->L.Nw));
  HIP_TRY(hipMemcpy2DAsync(S.wbuf, p->L.Nw * sizeof(double), b->params, b->ldp * sizeof(double), p->L.Nw * sizeof(double),
                           (size_t)S.B, hipMemcpyDeviceToDevice, st));
  S.use_w = true;
  return DTO_OK;
}

static int im_begin(Problem* p, const dto_options* opt, const dto_batch* b, bool warm, double mu0) {
  ImState& S = *p->im;
  hipStream_t st = (hipStream_t)b->stream;
  int rc;
  if ((rc = im_set_params(p, b, st))) return rc;
  dto_options u;
  if (opt) u = *opt; else dto_options_default(&u);
  S.user = u;
  default_opts(S.opt, u);
  S.opt.warm = warm ? 1 : 0;
  S.opt.mu_warm = mu0;
  dto_im_args a;
  fill_im_args(p, a);
  a.aos_in = b->x; a.ld_aos = b->ldx;
  if ((rc = im_launch(p, DTO_IM_INIT, a, st))) return rc;
  S.opt.warm = 0;
  S.begun = true;
  S.iter_base = 0;
  S.passes = 0;
  return DTO_OK;
}

// one pass; iter_target < 0: no iteration limit besides max_iter
static int im_pass(Problem* p, hipStream_t st, int iter_target) {
  ImState& S = *p->im;
  dto_im_args a;
  fill_im_args(p, a);
  a.iter_target = iter_target;
  int rc;
  HIP_TRY(hipMemsetAsync(S.ctr, 0, 5 * sizeof(int), st));
  auto with_list = [&](int k) { a.list = S.lists + (size_t)k * S.B; a.count = S.ctr + k; };
  auto compact = [&](int k, int phase) -> int {
    a.list_out = S.lists + (size_t)k * S.B; a.count_out = S.ctr + k; a.phase_sel = phase;
    return im_launch(p, DTO_IM_COMPACT, a, st);
  };
  if ((rc = compact(0, DTO_IM_PH_EVAL))) return rc;
  with_list(0);
  if ((rc = im_launch(p, DTO_IM_EVAL, a, st))) return rc;
  if ((rc = im_launch(p, DTO_IM_CONV, a, st))) return rc;
  if ((rc = compact(1, DTO_IM_PH_FACT))) return rc;
  with_list(1);
  a.ticket = S.ctr + 3;
  if ((rc = im_launch(p, DTO_IM_FWD, a, st))) return rc;
  if ((rc = compact(2, DTO_IM_PH_STEP))) return rc;
  with_list(2);
  a.ticket = S.ctr + 4;
  if ((rc = im_launch(p, DTO_IM_BWD, a, st))) return rc;
  if ((rc = im_launch(p, DTO_IM_LINESEARCH, a, st))) return rc;
  if ((rc = im_launch(p, DTO_IM_LS_REDUCE, a, st))) return rc;
  if ((rc = im_launch(p, DTO_IM_UPDATE, a, st))) return rc;
  ++S.passes;
  return DTO_OK;
}

// [0] running instances, [1] those of them with work left below the iteration target (host values after the call)
static int im_count(Problem* p, hipStream_t st, int iter_target, int* running, int* work) {
  ImState& S = *p->im;
  dto_im_args a;
  fill_im_args(p, a);
  a.iter_target = iter_target;
  HIP_TRY(hipMemsetAsync(S.ctr + 5, 0, 2 * sizeof(int), st));
  int rc;
  if ((rc = im_launch(p, DTO_IM_COUNT, a, st))) return rc;
  HIP_TRY(hipMemcpyAsync(S.h_ctr, S.ctr, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (running) *running = S.h_ctr[5];
  if (work) *work = S.h_ctr[6];
  return DTO_OK;
}

static int im_fetch_scalars(Problem* p, hipStream_t st) {
  ImState& S = *p->im;
  HIP_TRY(hipMemcpyAsync(S.h_scal.data(), S.scal, S.h_scal.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DTO_OK;
}

static inline double im_hscal(const ImState& S, int64_t inst, int slot) { return S.h_scal[(size_t)inst * S.info.nscal + slot]; }

static int im_unpack(Problem* p, int which, double* out, int64_t ld, hipStream_t st) {
  dto_im_args a;
  fill_im_args(p, a);
  a.aos_out = out; a.ld_aos = ld; a.aos_which = which;
  return im_launch(p, DTO_IM_UNPACK, a, st);
}

// every running instance advances by n iterations (instances that terminate on the way stop earlier)
static int im_iterate(Problem* p, int n, hipStream_t st) {
  ImState& S = *p->im;
  S.iter_base += n;
  const int target = S.iter_base;
  const int group = std::max(1, std::min(S.user.check_every > 0 ? S.user.check_every : 10, n));
  int rc, work = 1;
  // an iteration takes one pass plus one per rejected factorisation: max_refactor + 1 passes at most
  const int64_t pass_cap = (int64_t)n * (S.opt.max_refactor + 2) + 2;
  for (int64_t done = 0; work > 0 && done < pass_cap;) {
    for (int k = 0; k < group; ++k, ++done)
      if ((rc = im_pass(p, st, target))) return rc;
    if ((rc = im_count(p, st, target, nullptr, &work))) return rc;
  }
  return DTO_OK;
}

static int im_run(Problem* p, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, int32_t* status, int32_t* iterations,
                  hipStream_t st) {
  ImState& S = *p->im;
  int rc, running = 1;
  const int group = std::max(1, S.user.check_every);
  const auto t_start = std::chrono::steady_clock::now();
  bool timed_out = false;
  const int64_t pass_cap = ((int64_t)S.user.max_iter + 1) * (S.opt.max_refactor + 2) + 2;
  for (int64_t done = 0; running > 0 && done < pass_cap;) {
    for (int k = 0; k < group; ++k, ++done)
      if ((rc = im_pass(p, st, -1))) return rc;
    if ((rc = im_count(p, st, -1, &running, nullptr))) return rc;
    if (S.user.max_cpu_time > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > S.user.max_cpu_time) {
      timed_out = true;
      break;
    }
  }
  if (x_out) {
    if (ldxo < p->L.Nz) return set_error(DTO_ERR_INVALID, "ldxo < num_variables");
    if ((rc = im_unpack(p, 0, x_out, ldxo, st))) return rc;
  }
  if (mu_out) {
    if (ldmuo < p->L.Nc) return set_error(DTO_ERR_INVALID, "ldmuo < num_constraint");
    if ((rc = im_unpack(p, 1, mu_out, ldmuo, st))) return rc;
  }
  if ((rc = im_fetch_scalars(p, st))) return rc;
  for (int64_t i = 0; i < S.B; ++i) {
    if (status) { status[i] = (int32_t)im_hscal(S, i, SC_STATUS); if (status[i] == 0 && timed_out) status[i] = DTO_STATUS_CPU_TIME; }
    if (iterations) iterations[i] = (int32_t)im_hscal(S, i, SC_ITER);
  }
  return DTO_OK;
}

// ------------------------------------------------------------------------------------------------
// Bordered system: GeneralConstraint rows that couple several knots (src/general_constraint.jl:18-59; rows appended behind
// the stage rows, src/data.jl:72-75).  With the stage-interleaved ordering these rows are a dense border of the
// block-tridiagonal matrix:
//     [ K_s   G' ] [ v  ]   [ r_s ]        K_s: stage part (variables, dynamics rows, stage rows) -- the device kernels
//     [ G   -dc I ] [ drho] = [ r_g ]      G:   Jacobian of the general rows (constant pattern, few rows)
// solved by the Schur complement on the border:  Y = K_s^-1 [G'; 0]  (one forward + backward sweep per general row, all
// instances at once, through dto_kkt_assemble / factor / solve),  S = -(G Y_x + dc I),  S drho = r_g - G v0_x,
// v = v0 - Y drho.  The border algebra (n_g x n_g per instance, n_g = a handful) and the products with G run on the host:
// everything of size O(T) stays on the GPU.  The general rows must be Hessian-free (the layout refuses others: the
// reference's own Hessian call for them is broken, src/general_constraint.jl:87).
// dw: per-instance primal regularisation (host [B]); ok_out (host [B]): inertia of the whole bordered matrix is (Nz, Nc).
// stats (optional, host): per instance f-gradient / residual vectors the solve loop needs.
// ------------------------------------------------------------------------------------------------
struct BorderStats {
  std::vector<double> grad, c, rx, dz, dmu;   // [B][Nz], [B][Nc], [B][Nz], [B][Nz], [B][Nc]
  // device border: where grad f, c and r_x of the point lie in the problem's workspace (valid until the next step); the caller
  // fetches them -- and the step from its own buffers -- once per iteration instead of once per inertia-correction attempt
  const double *d_grad = nullptr, *d_c = nullptr, *d_rx = nullptr;
  const double* d_J = nullptr;   // (tile path) the Jacobian values of the point, COO order, [B][nnzJ]
  bool reuse_point = false;   // in: the point did not move since the last call (another delta_w attempt): keep J, c, grad f, r_x, G
  struct QnHistory* qn = nullptr;   // in (tile path, at most four general rows): the limited-memory mode -- the step is the compact L-BFGS one
};

// ---- limited-memory mode of the bordered loop on the tile path: the secant pairs of every instance on the device, the rules of
//      Ipopt's limited-memory update (skip, reset, scalar1 initialisation) on the host -- qn_decide / qn_update of dto_kkt_kernels.hpp
//      and of the CPU port.  The kernels are in dto_border_kernels.hpp (k_border_qn_save, k_border_qn_y, k_border_qn_push).
struct QnHistory {
  static constexpr int M = 6;      // pairs kept (Ipopt's limited_memory_max_history)
  DevBuf<double> S, Y;             // [B][M][Nz], oldest first
  DevBuf<double> s, gl, y;         // [B][Nz]: the saved step, grad_x L(x_k, lam_{k+1}), the new y
  DevBuf<double> dots, rb, sb;     // [B][3]: s'y, s's, y'y; [B][16] each: the zero right-hand side and the unknowns of the border
  DevBuf<int> flag;                // [2][B]: pending, slot
  std::vector<int32_t> npairs;     // pairs in the history of each instance
  std::vector<int> skipped, pending;
  std::vector<double> sigma;
  int init(int64_t B, int64_t Nz, hipStream_t st) {
    const size_t hist = (size_t)B * M * (size_t)Nz;
    for (DevBuf<double>* q : {&S, &Y})
      if (const hipError_t e = q->alloc(hist); e != hipSuccess)
        return hip_fail(e, ("limited-memory mode: hipMalloc of the history (" + std::to_string(2 * hist * sizeof(double)) + " bytes: " + std::to_string(B) +
                            " instances x " + std::to_string(2 * M) + " vectors x " + std::to_string(Nz) + " doubles)").c_str());
    for (DevBuf<double>* q : {&s, &gl, &y}) HIP_TRY(q->alloc((size_t)B * Nz));
    HIP_TRY(dots.alloc((size_t)B * 3));
    HIP_TRY(rb.alloc((size_t)B * 16));
    HIP_TRY(sb.alloc((size_t)B * 16));
    HIP_TRY(flag.alloc(2 * (size_t)B));
    // (the panel kernel reads only the pairs an instance has, but the history starts defined)
    HIP_TRY(hipMemsetAsync(S, 0, hist * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(Y, 0, hist * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(rb, 0, (size_t)B * 16 * sizeof(double), st));
    npairs.assign((size_t)B, 0); skipped.assign((size_t)B, 0); pending.assign((size_t)B, 0); sigma.assign((size_t)B, 1.0);
    return DTO_OK;
  }
};

static int ensure_border_csc(Problem* p) {
  if (p->d_csc_ptr) return DTO_OK;
  const Layout& L = p->L;
  std::vector<int> ptr((size_t)L.Nz + 1, 0), ck((size_t)L.nnzJ), crow((size_t)L.nnzJ);
  for (int64_t k = 0; k < L.nnzJ; ++k) ptr[(size_t)L.jac_cols[(size_t)k]] += 1;   // 1-based column -> slot col + 1 - 1 + 1
  for (int64_t cidx = 0; cidx < L.Nz; ++cidx) ptr[(size_t)cidx + 1] += ptr[(size_t)cidx];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int64_t k = 0; k < L.nnzJ; ++k) {   // increasing k inside every column
    const int64_t col = L.jac_cols[(size_t)k] - 1;
    const int e = fill[(size_t)col]++;
    ck[(size_t)e] = (int)k;
    crow[(size_t)e] = (int)(L.jac_rows[(size_t)k] - 1);
  }
  HIP_TRY(p->d_csc_ptr.alloc(ptr.size()));
  HIP_TRY(p->d_csc_k.alloc(ck.size()));
  HIP_TRY(p->d_csc_row.alloc(crow.size()));
  HIP_TRY(hipMemcpy(p->d_csc_ptr, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_csc_k, ck.data(), ck.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_csc_row, crow.data(), crow.size() * sizeof(int), hipMemcpyHostToDevice));
  std::vector<int> fx((size_t)L.Nz);
  for (int64_t k = 0; k < L.Nz; ++k) fx[(size_t)k] = (L.var_lo[(size_t)k] == L.var_hi[(size_t)k]) ? 1 : 0;
  HIP_TRY(p->d_var_fixed.alloc(fx.size()));
  HIP_TRY(hipMemcpy(p->d_var_fixed, fx.data(), fx.size() * sizeof(int), hipMemcpyHostToDevice));
  return DTO_OK;
}

// ---- what the three bordered steps share ------------------------------------------------------------------------------------
// carving the problem's one workspace (border_ws), in the order of each layout's map comment
struct BorderCarve {
  double* w;
  double* take(size_t n) { double* q = w; w += n; return q; }
};
// J, c and grad f of the point into the workspace.  Not at a further delta_w attempt at the same point (reuse_point): everything
// that depends on the point alone is still there
static int border_eval_point(dto_problem* h, const dto_batch* b, double* dJ, int64_t nnzJ, double* dC, int64_t Nc, double* dG, int64_t Nz) {
  int rc;
  if ((rc = dto_eval_jac_g_batch(h, b, dJ, nnzJ))) return rc;
  if ((rc = dto_eval_g_batch(h, b, dC, Nc))) return rc;
  return dto_eval_grad_f_batch(h, b, dG, Nz);
}
// per-instance delta_w (dw: host [B]) through the sigma_x diagonal (k_border_sig; pin_fixed: a variable with lo == hi keeps its
// value; bar: the barrier terms of finite bounds ride the same diagonal), and the system both linear solvers assemble from
static int border_sigma_system(Problem* p, const dto_batch* b, const double* mu, int64_t ldmu, const double* dw, double delta_c, bool pin_fixed,
                               const BorderBar& bar, double* dDw, double* dSig, double* dSigC, dto_kkt_system& sys) {
  const int64_t B = b->B, Nz = p->L.Nz;
  hipStream_t st = (hipStream_t)b->stream;
  HIP_TRY(hipMemcpyAsync(dDw, dw, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_border_sig, dim3((unsigned)(((size_t)B * Nz + 255) / 256)), dim3(256), 0, st, B, Nz, (const double*)dDw,
                     (const int*)p->d_var_fixed, pin_fixed ? 1 : 0, dSig, bar);
  sys.mu = mu; sys.ldmu = ldmu; sys.sigma_x = dSig; sys.ldsx = Nz; sys.sigma_c = dSigC; sys.ldsc = dSigC ? p->L.Nc : 0;
  sys.delta_w = 0.0; sys.delta_c = delta_c;
  return DTO_OK;
}

// ---- the bordered step on the lane path, border algebra on the device (kernels: dto_border_kernels.hpp): one dto_kkt_solve for
//      the step and one per general row, k_border_solve / k_border_apply for the Schur complement
static int bordered_step_device(Problem* p, const dto_batch* b, const double* mu, int64_t ldmu, const double* dw, double delta_c,
                                double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* ok_out, BorderStats* stats, bool pin_fixed,
                                const double* gdiag, const double* gshift, const BorderBar* barp, const BorderSlack* slk) {
  const Layout& L = p->L;
  const int64_t B = b->B, Nz = L.Nz, Nc = L.Nc, ng = L.Ngen, Ns = Nc - ng, nnzJ = L.nnzJ;
  hipStream_t st = (hipStream_t)b->stream;
  dto_problem* h = reinterpret_cast<dto_problem*>(p);
  const BorderBar bar = barp ? *barp : BorderBar();   // (no bounds: all NULL, the kernels take their old branches)
  const BorderSlack sl = slk ? *slk : BorderSlack();  // (no inequality stage rows: the same)
  int rc = ensure_border_csc(p);
  if (rc) return rc;
  // workspace: J | c | g | sig | rx | rhsx | rhsc | zero_c | v0x | v0c | Grow[ng] | Yx[ng] | Yc[ng] | hdx | hdm | rho | flags | dw
  // (| sigma_c behind them, with inequality stage rows only)
  const size_t nBz = (size_t)B * Nz, nBc = (size_t)B * Nc;
  const size_t ws_need = (size_t)B * nnzJ + nBc + nBz * 6 + nBc * 4 + (size_t)ng * (2 * nBz + nBc) + (size_t)B * ng + 2 * (size_t)B + 8 +
                         (sl.s ? nBc : 0);
  HIP_TRY(p->border_ws.grow(ws_need));
  BorderCarve ws{p->border_ws};
  double *dJ = ws.take((size_t)B * nnzJ), *dC = ws.take(nBc), *dG = ws.take(nBz), *dSig = ws.take(nBz), *dRxv = ws.take(nBz),
         *dRhsx = ws.take(nBz), *dRhsc = ws.take(nBc), *dZeroC = ws.take(nBc), *dV0x = ws.take(nBz), *dV0c = ws.take(nBc),
         *dGrow = ws.take((size_t)ng * nBz), *dYx = ws.take((size_t)ng * nBz), *dYc = ws.take((size_t)ng * nBc), *dHdx = ws.take(nBz),
         *dHdm = ws.take(nBc), *dRho = ws.take((size_t)B * ng);
  int* dFlag = reinterpret_cast<int*>(ws.take((size_t)B / 2 + 4));
  double* dDw = ws.take((size_t)B);
  double* dSigC = sl.s ? ws.take(nBc) : nullptr;
#define DRC(expr) do { rc = (expr); if (rc) return rc; } while (0)
  if (!(stats && stats->reuse_point)) {
    DRC(border_eval_point(h, b, dJ, nnzJ, dC, Nc, dG, Nz));
    HIP_TRY(hipMemsetAsync(dGrow, 0, (size_t)ng * nBz * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(dZeroC, 0, nBc * sizeof(double), st));
    hipLaunchKernelGGL(k_border_rx, dim3((unsigned)((nBz + 255) / 256)), dim3(256), 0, st, B, Nz, Ns, nnzJ, (const double*)dJ, (const double*)dG,
                       mu, ldmu, (const int*)p->d_csc_ptr, (const int*)p->d_csc_k, (const int*)p->d_csc_row, dRxv, dRhsx, dGrow, bar);
    hipLaunchKernelGGL(k_border_rhsc, dim3((unsigned)((nBc + 255) / 256)), dim3(256), 0, st, B, Nc, Ns, (const double*)dC, dRhsc, sl, mu, ldmu,
                       dSigC);
  }
  dto_kkt_system sys;
  DRC(border_sigma_system(p, b, mu, ldmu, dw, delta_c, pin_fixed, bar, dDw, dSig, dSigC, sys));
  DRC(dto_kkt_assemble(h, b, &sys));
  std::vector<int32_t> iok((size_t)B, 1);
  DRC(dto_kkt_factor(h, iok.data(), nullptr, (void*)st));
  DRC(dto_kkt_solve(h, dRhsx, Nz, dRhsc, Nc, dV0x, Nz, dV0c, Nc, (void*)st));
  for (int64_t j = 0; j < ng; ++j)
    DRC(dto_kkt_solve(h, dGrow + (size_t)j * nBz, Nz, dZeroC, Nc, dYx + (size_t)j * nBz, Nz, dYc + (size_t)j * nBc, Nc, (void*)st));
  hipLaunchKernelGGL(k_border_solve, dim3((unsigned)B), dim3(64), 0, st, B, Nz, Nc, Ns, (int)ng, delta_c, (const double*)dGrow,
                     (const double*)dYx, (const double*)dV0x, (const double*)dC, gdiag, gshift, dRho, dFlag);
  hipLaunchKernelGGL(k_border_apply, dim3((unsigned)(((size_t)B * (Nz + Nc) + 255) / 256)), dim3(256), 0, st, B, Nz, Nc, Ns, (int)ng,
                     (const double*)dV0x, (const double*)dV0c, (const double*)dYx, (const double*)dYc, (const double*)dRho, dx, lddx, dmu,
                     lddmu, dHdx, dHdm);
  HIP_TRY(hipGetLastError());
  std::vector<int> flag((size_t)B);
  HIP_TRY(hipMemcpyAsync(flag.data(), dFlag, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (stats) { stats->d_grad = dG; stats->d_c = dC; stats->d_rx = dRxv; }
  HIP_TRY(hipStreamSynchronize(st));
  if (ok_out)
    for (int64_t i = 0; i < B; ++i) ok_out[i] = (iok[(size_t)i] != 0 && flag[(size_t)i] != 0) ? 1 : 0;
#undef DRC
  return DTO_OK;
}

// At a new point (J and grad f just evaluated there, lam the multipliers the step ended with): y and the three dot products of the
// instances with a saved step, then the rules of the update -- a pair without curvature (s'y <= sqrt(eps) |s| |y|) is skipped, two
// skips in a row drop the history, sigma = clamp(s'y / s's, 1e-8, 1e8) of the newest pair -- and the push.
static int qn_update(Problem* p, QnHistory& Q, int64_t B, const double* dJ, const double* dG, const double* lam, int64_t ldl, hipStream_t st) {
  bool any = false;
  for (int v : Q.pending) any = any || v != 0;
  if (!any) return DTO_OK;
  const int64_t Nz = p->L.Nz, nnzJ = p->L.nnzJ;
  int* dpend = Q.flag;
  int* dslot = Q.flag + B;
  HIP_TRY(hipMemcpyAsync(dpend, Q.pending.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_border_qn_y, dim3((unsigned)B), dim3(256), 0, st, Nz, nnzJ, dJ, dG, lam, ldl, (const int*)p->d_csc_ptr, (const int*)p->d_csc_k,
                     (const int*)p->d_csc_row, (const int*)p->d_var_fixed, (const int*)dpend, (double*)Q.s, (const double*)Q.gl, (double*)Q.y,
                     (double*)Q.dots);
  HIP_TRY(hipGetLastError());
  std::vector<double> hd((size_t)B * 3);
  HIP_TRY(hipMemcpyAsync(hd.data(), Q.dots, hd.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<int> slot((size_t)B, -1);
  bool push = false;
  for (int64_t i = 0; i < B; ++i) {
    if (!Q.pending[(size_t)i]) continue;
    Q.pending[(size_t)i] = 0;
    const double sy = hd[(size_t)i * 3], ss = hd[(size_t)i * 3 + 1], yy = hd[(size_t)i * 3 + 2];
    if (!(sy > 1.4901161193847656e-08 * std::sqrt(ss) * std::sqrt(yy))) {
      if (++Q.skipped[(size_t)i] >= 2) { Q.npairs[(size_t)i] = 0; Q.skipped[(size_t)i] = 0; }
      continue;
    }
    Q.skipped[(size_t)i] = 0;
    slot[(size_t)i] = Q.npairs[(size_t)i];   // (M: the oldest pair is dropped)
    Q.npairs[(size_t)i] = std::min<int32_t>(QnHistory::M, Q.npairs[(size_t)i] + 1);
    Q.sigma[(size_t)i] = std::min(1e8, std::max(1e-8, sy / ss));
    push = true;
  }
  if (!push) return DTO_OK;
  HIP_TRY(hipMemcpyAsync(dslot, slot.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_border_qn_push, dim3((unsigned)(((size_t)B * Nz + 255) / 256)), dim3(256), 0, st, B, (int)QnHistory::M, Nz, (const int*)dslot,
                     (const double*)Q.s, (const double*)Q.y, (double*)Q.S, (double*)Q.Y);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));   // (slot is a local of this call)
  return DTO_OK;
}

// ---- the bordered step on the tile path: the stage part is factorised ONCE into the stored records, the n_g border rows go
//      through one panel substitution (dto_kkt_border_factor) and the step is one single substitution and two passes over Y
//      (dto_kkt_border_solve) -- instead of the n_g + 1 sweeps of the lane path above.  Fixed variables (pin_fixed): sigma_x = 1e16,
//      as on the lane path (why not the identity rows of the tile solver, and why 1e16 is safe in
//      k_wide_step's linear-solver mode); k_border_point zeroes their entries of the right-hand side and of the panel, and
//      k_border_unpin the 1e-16-sized step that is left, so that a fixed variable keeps its value to the last bit.
static int bordered_step_tile(Problem* p, const dto_batch* b, const double* mu, int64_t ldmu, const double* dw, double delta_c,
                              double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* ok_out, BorderStats* stats, bool pin_fixed,
                              const double* gdiag, const double* gshift, const BorderBar* barp) {
  const Layout& L = p->L;
  const int64_t B = b->B, Nz = L.Nz, Nc = L.Nc, ng = L.Ngen, Ns = Nc - ng, nnzJ = L.nnzJ;
  if (ng > KB_MAX) return set_error(DTO_ERR_UNSUPPORTED, "dto_kkt_border_factor: more than 16 border rows (one panel of right-hand sides)");
  if (L.Nstage != 0) return set_error(DTO_ERR_UNSUPPORTED, "wide-stage models: dynamics rows, GeneralConstraint rows and bounds only");
  hipStream_t st = (hipStream_t)b->stream;
  dto_problem* h = reinterpret_cast<dto_problem*>(p);
  const BorderBar bar = barp ? *barp : BorderBar();   // (no bounds: all NULL, the kernels take their old branches)
  QnHistory* qn = stats ? stats->qn : nullptr;
  if (qn && 2 * QnHistory::M + ng > KB_MAX)
    return set_error(DTO_ERR_UNSUPPORTED, "limited-memory mode beside more than four GeneralConstraint rows on the tile border (12 + n_g rows, one panel)");
  int rc = p->ensure_device();
  if (rc) return rc;
  if ((rc = ensure_border_csc(p))) return rc;
  // workspace: J | c | grad | sigma | r_x | rhs_x | rhs_c | panel [B * ng][Nz] | C [B][ng * ng] | rhs_b [B][ng] | delta_w [B]
  const size_t nBz = (size_t)B * Nz, nBc = (size_t)B * Nc, nBg = (size_t)B * ng;
  HIP_TRY(p->border_ws.grow((size_t)B * nnzJ + 2 * nBc + 5 * nBz + nBg * Nz + nBg * ng + nBg + (size_t)B));
  BorderCarve ws{p->border_ws};
  double *dJ = ws.take((size_t)B * nnzJ), *dC = ws.take(nBc), *dG = ws.take(nBz), *dSig = ws.take(nBz), *dRxv = ws.take(nBz),
         *dRhsx = ws.take(nBz), *dRhsc = ws.take(nBc), *dPanel = ws.take(nBg * Nz), *dCb = ws.take(nBg * ng), *dRhsb = ws.take(nBg),
         *dDw = ws.take((size_t)B);
#define DRC(expr) do { rc = (expr); if (rc) return rc; } while (0)
  if (!(stats && stats->reuse_point)) {
    DRC(border_eval_point(h, b, dJ, nnzJ, dC, Nc, dG, Nz));
    if (qn) DRC(qn_update(p, *qn, B, dJ, dG, mu, ldmu, st));   // the pair of the step that led here joins the history
  }
  // (the right-hand sides, the panel and C are written again at every attempt: one launch, and nothing to clear first)
  {
    const size_t n = std::max(nBz, std::max((size_t)B * Ns, nBg * ng));
    hipLaunchKernelGGL(k_border_point, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, B, Nz, Nc, Ns, (int)ng, nnzJ, (const double*)dJ,
                       (const double*)dG, (const double*)dC, mu, ldmu, (const int*)p->d_csc_ptr, (const int*)p->d_csc_k, (const int*)p->d_csc_row,
                       (const int*)p->d_var_fixed, pin_fixed ? 1 : 0, delta_c, gdiag, gshift, dRxv, dRhsx, dPanel, dRhsc, dRhsb, dCb, bar);
    HIP_TRY(hipGetLastError());
  }
  // per-instance delta_w through the sigma_x diagonal (pin_fixed: a variable with lo == hi keeps its value)
  // (limited-memory mode: sigma of the compact matrix rides the same diagonal)
  std::vector<double> dws;
  if (qn) {
    dws.resize((size_t)B);
    for (int64_t i = 0; i < B; ++i) dws[(size_t)i] = dw[i] + qn->sigma[(size_t)i];
  }
  dto_kkt_system sys;
  DRC(border_sigma_system(p, b, mu, ldmu, qn ? dws.data() : dw, delta_c, pin_fixed, bar, dDw, dSig, nullptr, sys));
  DRC(wide_kkt_assemble(p, b, &sys, qn != nullptr));
  std::vector<int32_t> iok((size_t)B, 1), negdef((size_t)B, 1), sing((size_t)B, 0);
  DRC(wide_kkt_factor(p, iok.data(), nullptr, st));
  if (qn && ng > 0) {
    // both borders in one panel: [sigma S; Y; G] with blkdiag(M, C) -- the right-hand side of the compact part is zero, that of the
    // rows is theirs; the rows' part of the border unknowns is the step of their multipliers.  negdef carries inertia_ok
    constexpr int64_t QM2 = 2 * QnHistory::M;
    DRC(dto_kkt_lbfgs_border_rows(h, QnHistory::M, qn->S, Nz, qn->Y, Nz, qn->npairs.data(), qn->sigma.data(), ng, dPanel, Nz, nullptr, 0, dCb, ng * ng,
                                  negdef.data(), sing.data(), (void*)st));
    HIP_TRY(hipMemcpy2DAsync((double*)qn->rb + QM2, 16 * sizeof(double), dRhsb, (size_t)ng * sizeof(double), (size_t)ng * sizeof(double), (size_t)B,
                             hipMemcpyDeviceToDevice, st));
    DRC(dto_kkt_border_solve(h, dRhsx, Nz, dRhsc, Nc, qn->rb, 16, dx, lddx, dmu, lddmu, qn->sb, 16, (void*)st));
    HIP_TRY(hipMemcpy2DAsync(dmu + Ns, (size_t)lddmu * sizeof(double), (const double*)qn->sb + QM2, 16 * sizeof(double), (size_t)ng * sizeof(double),
                             (size_t)B, hipMemcpyDeviceToDevice, st));
  } else if (qn) {
    // K0 = first-order system + (sigma + delta_w) I, the compact matrix as a border of 2 M rows; negdef carries inertia_ok
    DRC(dto_kkt_lbfgs_border(h, QnHistory::M, qn->S, Nz, qn->Y, Nz, qn->npairs.data(), qn->sigma.data(), negdef.data(), sing.data(), (void*)st));
    DRC(dto_kkt_border_solve(h, dRhsx, Nz, dRhsc, Nc, qn->rb, 16, dx, lddx, dmu, lddmu, qn->sb, 16, (void*)st));
  } else {
    DRC(dto_kkt_border_factor(h, ng, dPanel, Nz, nullptr, 0, dCb, ng * ng, negdef.data(), sing.data(), (void*)st));
    DRC(dto_kkt_border_solve(h, dRhsx, Nz, dRhsc, Nc, dRhsb, ng, dx, lddx, dmu, lddmu, dmu + Ns, lddmu, (void*)st));
  }
#undef DRC
  if (pin_fixed) {
    hipLaunchKernelGGL(k_border_unpin, dim3((unsigned)((nBz + 255) / 256)), dim3(256), 0, st, B, Nz, (const int*)p->d_var_fixed, dx, lddx);
    HIP_TRY(hipGetLastError());
  }
  if (stats) { stats->d_grad = dG; stats->d_c = dC; stats->d_rx = dRxv; stats->d_J = dJ; }
  HIP_TRY(hipStreamSynchronize(st));
  if (ok_out)
    for (int64_t i = 0; i < B; ++i) ok_out[i] = (iok[(size_t)i] != 0 && negdef[(size_t)i] != 0 && sing[(size_t)i] == 0) ? 1 : 0;
  return DTO_OK;
}

// ---- the bordered step on the lane path, border algebra on the host (round 3; DTO_BORDER_HOST=1, or more than BORDER_MAX_NG
//      general rows): every right-hand side and solution of the n_g + 1 solves crosses PCIe, the Schur complement is formed and
//      solved here (border_schur_solve, the function lane 0 of k_border_solve calls).  Equality rows and free or fixed variables
//      only; stats gets whole vectors, which border_loop_host_stats reduces to the numbers the device border delivers
static int bordered_step_host(Problem* p, const dto_batch* b, const double* mu, int64_t ldmu, const double* dw, double delta_c,
                              double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* ok_out, BorderStats* stats, bool pin_fixed) {
  const Layout& L = p->L;
  const int64_t B = b->B, Nz = L.Nz, Nc = L.Nc, ng = L.Ngen, Ns = Nc - ng, nnzJ = L.nnzJ;
  hipStream_t st = (hipStream_t)b->stream;
  dto_problem* h = reinterpret_cast<dto_problem*>(p);
  int rc;
  // workspace: J | c | grad | sigma | rhs_x | rhs_c | sol_x | sol_c
  const size_t nBz = (size_t)B * Nz, nBc = (size_t)B * Nc;
  HIP_TRY(p->border_ws.grow((size_t)B * nnzJ + 4 * nBz + 3 * nBc));
  BorderCarve ws{p->border_ws};
  double *dJ = ws.take((size_t)B * nnzJ), *dC = ws.take(nBc), *dG = ws.take(nBz), *dSig = ws.take(nBz), *dRx = ws.take(nBz),
         *dRc = ws.take(nBc), *dSx = ws.take(nBz), *dSc = ws.take(nBc);
  // ---- derivatives at (x, mu): callbacks on the device, the small vectors come to the host
#define DRC(expr) do { rc = (expr); if (rc) return rc; } while (0)
  DRC(border_eval_point(h, b, dJ, nnzJ, dC, Nc, dG, Nz));
  std::vector<double> J((size_t)B * nnzJ), c(nBc), g(nBz), m(nBc);
  HIP_TRY(hipMemcpyAsync(J.data(), dJ, J.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(c.data(), dC, c.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(g.data(), dG, g.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpy2DAsync(m.data(), Nc * sizeof(double), mu, ldmu * sizeof(double), Nc * sizeof(double), (size_t)B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // r_x = grad f + J' mu (all rows, general ones included); the general rows of J as dense vectors
  std::vector<double> rx(nBz), Grow((size_t)ng * nBz, 0.0);
  for (int64_t i = 0; i < B; ++i) {
    double* r = &rx[(size_t)i * Nz];
    for (int64_t k = 0; k < Nz; ++k) r[k] = g[(size_t)i * Nz + k];
    for (int64_t k = 0; k < nnzJ; ++k) {
      const int64_t row = L.jac_rows[(size_t)k] - 1, col = L.jac_cols[(size_t)k] - 1;
      const double v = J[(size_t)i * nnzJ + k];
      r[col] += v * m[(size_t)i * Nc + row];
      if (row >= Ns) Grow[((size_t)(row - Ns) * B + i) * Nz + col] += v;
    }
  }
  // ---- stage part: assemble, factor (per-instance delta_w through the sigma_x diagonal), solve for the 1 + n_g right-hand sides
  std::vector<double> sig(nBz);
  for (int64_t i = 0; i < B; ++i)
    for (int64_t k = 0; k < Nz; ++k)   // pin_fixed: a variable with lo == hi keeps its value (a huge diagonal entry: its step is ~1e-16 r)
      sig[(size_t)i * Nz + k] = (pin_fixed && L.var_lo[(size_t)k] == L.var_hi[(size_t)k]) ? 1e16 : dw[i];
  HIP_TRY(hipMemcpyAsync(dSig, sig.data(), sig.size() * sizeof(double), hipMemcpyHostToDevice, st));
  dto_kkt_system sys;
  sys.mu = mu; sys.ldmu = ldmu; sys.sigma_x = dSig; sys.ldsx = Nz; sys.sigma_c = nullptr; sys.ldsc = 0;
  sys.delta_w = 0.0; sys.delta_c = delta_c;
  DRC(dto_kkt_assemble(h, b, &sys));
  std::vector<int32_t> iok((size_t)B, 1);
  DRC(dto_kkt_factor(h, iok.data(), nullptr, (void*)st));
  std::vector<double> rhsx(nBz), rhsc(nBc, 0.0), solx(nBz), solc(nBc), Yx((size_t)ng * nBz), Yc((size_t)ng * nBc);
  auto solve = [&](const double* hx, const double* hc, double* ox, double* oc) -> int {
    HIP_TRY(hipMemcpyAsync(dRx, hx, nBz * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dRc, hc, nBc * sizeof(double), hipMemcpyHostToDevice, st));
    DRC(dto_kkt_solve(h, dRx, Nz, dRc, Nc, dSx, Nz, dSc, Nc, (void*)st));
    HIP_TRY(hipMemcpyAsync(ox, dSx, nBz * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(oc, dSc, nBc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DTO_OK;
  };
  for (size_t k = 0; k < rhsx.size(); ++k) rhsx[k] = -rx[k];
  for (int64_t i = 0; i < B; ++i)
    for (int64_t k = 0; k < Ns; ++k) rhsc[(size_t)i * Nc + k] = -c[(size_t)i * Nc + k];
  DRC(solve(rhsx.data(), rhsc.data(), solx.data(), solc.data()));
  std::vector<double> zero_c(nBc, 0.0);
  for (int64_t j = 0; j < ng; ++j) DRC(solve(&Grow[(size_t)j * nBz], zero_c.data(), &Yx[(size_t)j * nBz], &Yc[(size_t)j * nBc]));
  // ---- border: S = -(G Y_x + dc I), S drho = r_g - G v0_x per instance; v = v0 - Y drho, the general rows' multipliers are drho
  std::vector<double> hdx(nBz), hdm(nBc), Sm((size_t)ng * ng), rg((size_t)ng), Lc((size_t)ng * ng);
  for (int64_t i = 0; i < B; ++i) {
    auto gdot = [&](int64_t row, const double* v) {
      const double* gr = &Grow[((size_t)row * B + i) * Nz];
      double acc = 0.0;
      for (int64_t k = 0; k < Nz; ++k) acc += gr[k] * v[k];
      return acc;
    };
    for (int64_t a = 0; a < ng; ++a) {
      for (int64_t q = 0; q < ng; ++q) Sm[(size_t)a * ng + q] = -gdot(a, &Yx[((size_t)q * B + i) * Nz]) - (a == q ? delta_c : 0.0);
      rg[(size_t)a] = -c[(size_t)i * Nc + Ns + a] - gdot(a, &solx[(size_t)i * Nz]);
    }
    const bool negdef = border_schur_solve((int)ng, Sm.data(), rg.data(), Lc.data());
    if (ok_out) ok_out[i] = (iok[(size_t)i] != 0 && negdef) ? 1 : 0;
    for (int64_t k = 0; k < Nz; ++k) {
      double v = solx[(size_t)i * Nz + k];
      for (int64_t q = 0; q < ng; ++q) v -= Yx[((size_t)q * B + i) * Nz + k] * rg[(size_t)q];
      hdx[(size_t)i * Nz + k] = v;
    }
    for (int64_t k = 0; k < Ns; ++k) {
      double v = solc[(size_t)i * Nc + k];
      for (int64_t q = 0; q < ng; ++q) v -= Yc[((size_t)q * B + i) * Nc + k] * rg[(size_t)q];
      hdm[(size_t)i * Nc + k] = v;
    }
    for (int64_t q = 0; q < ng; ++q) hdm[(size_t)i * Nc + Ns + q] = rg[(size_t)q];
  }
  HIP_TRY(hipMemcpy2DAsync(dx, lddx * sizeof(double), hdx.data(), Nz * sizeof(double), Nz * sizeof(double), (size_t)B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpy2DAsync(dmu, lddmu * sizeof(double), hdm.data(), Nc * sizeof(double), Nc * sizeof(double), (size_t)B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (stats) {
    stats->grad.swap(g); stats->c.swap(c); stats->rx.swap(rx); stats->dz.swap(hdx); stats->dmu.swap(hdm);
  }
#undef DRC
  return DTO_OK;
}

// ---- the linear solver of general_solve_batch and of dto_kkt_step_batch with general rows: tile path, lane path with the border
//      algebra on the device, or on the host
static int bordered_step(Problem* p, const dto_batch* b, const double* mu, int64_t ldmu, const double* dw, double delta_c,
                         double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* ok_out, BorderStats* stats, bool pin_fixed,
                         const double* gdiag, const double* gshift, const BorderBar* barp, const BorderSlack* slk) {
  if (p->vt->launch_wide)   // (no stage rows on the tile path: slk is NULL)
    return bordered_step_tile(p, b, mu, ldmu, dw, delta_c, dx, lddx, dmu, lddmu, ok_out, stats, pin_fixed, gdiag, gshift, barp);
  const char* e = getenv("DTO_BORDER_HOST");
  if (!(e && atoi(e) != 0) && p->L.Ngen <= BORDER_MAX_NG)
    return bordered_step_device(p, b, mu, ldmu, dw, delta_c, dx, lddx, dmu, lddmu, ok_out, stats, pin_fixed, gdiag, gshift, barp, slk);
  if (slk) return set_error(DTO_ERR_UNSUPPORTED, "inequality stage rows beside GeneralConstraint rows need the device border (DTO_BORDER_HOST unset, at most 16 general rows)");
  if (barp) return set_error(DTO_ERR_UNSUPPORTED, "variable bounds beside GeneralConstraint rows need the device border (DTO_BORDER_HOST unset, at most 16 general rows)");
  if (gdiag) return set_error(DTO_ERR_UNSUPPORTED, "inequality GeneralConstraint rows need the device border (DTO_BORDER_HOST unset, at most 16 general rows)");
  return bordered_step_host(p, b, mu, ldmu, dw, delta_c, dx, lddx, dmu, lddmu, ok_out, stats, pin_fixed);
}


// ------------------------------------------------------------------------------------------------
// Solve for models with multi-knot GeneralConstraint rows: the filter line-search SQP iteration of the other paths, driven
// from the host like the wide-stage solver, with bordered_step as its linear solver.  Scope: equality rows (dynamics, stage,
// general), inequality rows c <= 0 among the general rows (slacks, on the host over n_g <= 16 entries) and among the rows of stage
// Constraints (lane path, device border: slacks on the device, BorderSlack -- k_border_slack_init / _stats / _update, the shifted
// sums of k_border_stats and k_border_trial, s / nu through dto_kkt_system.sigma_c), shared or per-instance parameters, and
// variable bounds: free, fixed by equal bounds, or finite on either side.  One barrier parameter per instance serves all of them.
// Finite bounds are a primal-dual barrier with the bound multipliers eliminated, as in
// wide_outer: z_L / z_U live on the device as [B][Nz], the barrier terms of the KKT system are written by the step's own kernels
// (BorderBar), k_border_bar_stats reduces what the host rules need to eight numbers per instance that ride the copy of
// k_border_stats, k_border_trial adds sum log(gap) of a trial point to the launch that sums its violation, and
// k_wide_init_bounds / k_wide_update_bounds keep the multipliers.  Without a finite bound none of that is allocated or launched.
// dto_solve_batch returns x and the constraint multipliers; dto_solve_batch_warm hands in a whole primal-dual point and gets one
// back (bound multipliers, slacks, barrier parameters, the limited-memory history): border_loop_start_point / _end_point.
// ------------------------------------------------------------------------------------------------
// out[b] = sum_k |rows[b][k]| in a fixed order (lane-strided partial sums, then a tree): the l1 constraint violation of a trial point
static __global__ __launch_bounds__(64) void k_rows_abs_sum(const double* rows, int64_t ld, int64_t n, double* out, const double* shift = nullptr,
                                                            int64_t n0 = 0, int64_t nsh = 0) {
  // shift (optional, [B][nsh]): added to rows n0 .. n0 + nsh - 1 before the absolute value (the slacks of inequality rows)
  const int64_t b = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 64) acc += fabs(rows[b * ld + i] + ((shift && i >= n0) ? shift[b * nsh + (i - n0)] : 0.0));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) out[b] = acc;
}

// The state of one general_solve_batch call: device buffers (DevBufs: released on every return), their host mirrors, the
// per-instance globalisation records, the row classification with the flags that follow from it, and the optional parts (barrier
// terms of bounds, slacks of stage rows, secant pairs).  The phases below are the loop in order, as A - E are wide_outer's; the
// differences from that loop that are kept on purpose ("Host-driven loops") are marked (difference n) where they live.
struct BorderLoop {
  Problem* p = nullptr;
  dto_problem* h = nullptr;
  hipStream_t st = nullptr;
  dto_options user{};
  dto_solver_opts o{};
  dto_batch bz{};                      // the caller's batch with x = z (params / ldp stay the caller's: the point, the trials, the slack
                                       // initialisation and bordered_step)
  int64_t B = 0, Nz = 0, Nc = 0, ng = 0, Ns = 0;
  // rows and bounds: ineq [ng] marks the inequality general rows (ni of them), smask [Ns] the inequality stage rows (nsi; empty
  // without one), n_bound counts the finite bound sides of the variables that are not fixed
  std::vector<char> ineq;
  std::vector<int> smask;
  int64_t ni = 0, nsi = 0, n_bound = 0;
  bool bounds = false, bounds_or_slk = false, barrier = false;   // n_bound > 0; that or nsi > 0; that or ni > 0: one mu per instance
  bool lbfgs = false, timed_out = false;
  int nth = 1;                         // numbers per instance of a trial point (k_rows_abs_sum / k_border_trial)
  std::chrono::steady_clock::time_point t_start;
  DevBuf<double> z, lam, dz, dlam, zt, df, dc, dal, dth;
  DevBuf<double> dgd, dgs, dst;        // [B][ng]: s / nu, mu / nu, trial slacks of the general rows
  DevBuf<double> d5;                   // [B][5] statistics of the point and the step; with bounds [B][BORDER_BAR_NSTAT] behind them,
                                       // with inequality stage rows [B][BORDER_SLK_NSTAT] behind those
  DevBuf<double> zl, zu, dlo, dhi, dmub, dad;   // finite bounds only: multipliers [B][Nz], shared bounds [Nz]; mu and alpha_d [B]: those
                                                // and inequality stage rows
  DevBuf<double> ss, sds;                       // inequality stage rows only: slacks and their step [B][Ns]
  DevBuf<int> dsmask;                           //   and the 0/1 mask of those rows [Ns]
  BorderBar bar;
  BorderSlack slk;
  QnHistory qn;                        // (allocated in the limited-memory mode only)
  BorderStats bs;                      // what the step of this iteration left
  std::vector<GlobInst> I;             // (mu: finite bounds, inequality general rows and inequality stage rows share one per instance)
  std::vector<double> hz, hmu, had;    // (hz: the start point without bounds, staged here so that its upload needs no wait)
  std::vector<double> hout;            // (the barrier parameters on their way into a caller's end point)
  // slacks and multipliers of the general rows on the host (the multipliers are mirrored into lam after every update), the slack
  // steps, s / nu, mu / nu and the trial slacks
  std::vector<double> hs, hnu, hds, hgd, hgs, hst;
  std::vector<double> dwv, hf, hth, hal, hphi0, hst5, hdnu, th0, gphid, chosen_a, apmax, admax;
  std::vector<int> okv;
  std::vector<char> mu_moved, ftype_a;
  std::vector<MostFeasible> best_a;
  // hst5, the host copy of d5: the block of instance i behind the [B][5]
  const double* bound_stats(int64_t i) const { return bounds ? &hst5[(size_t)B * 5 + (size_t)i * BORDER_BAR_NSTAT] : nullptr; }
  const double* slack_stats(int64_t i) const {
    return nsi > 0 ? &hst5[(size_t)B * 5 + (bounds ? (size_t)B * BORDER_BAR_NSTAT : 0) + (size_t)i * BORDER_SLK_NSTAT] : nullptr;
  }
  bool running(int64_t i) const { return I[(size_t)i].status == 0; }
  int put_nu() {   // host multipliers of the general rows -> their columns of lam
    HIP_TRY(hipMemcpy2DAsync(lam + Ns, Nc * sizeof(double), hnu.data(), ng * sizeof(double), ng * sizeof(double), (size_t)B, hipMemcpyHostToDevice, st));
    return DTO_OK;
  }
};

// ---- the start of a warm solve (dto_solve_batch_warm, start != NULL; the rules are stated in include/dto.h): the barrier parameter
//      of every instance, the variables with their bound multipliers (k_border_warm_vars), the multipliers as given, the history.
//      The slacks follow in border_loop_begin, where the cold start has them.  Every host record is the fresh one of a cold start
static int border_loop_start_point(BorderLoop& G, const dto_point& s) {
  const int64_t B = G.B, Nz = G.Nz, Nc = G.Nc, ng = G.ng, Ns = G.Ns;
  hipStream_t st = G.st;
  const dto_solver_opts& o = G.o;
  if (G.barrier) {
    std::vector<double> hb((size_t)B, 0.0);
    if (s.barrier) {
      HIP_TRY(hipMemcpyAsync(hb.data(), s.barrier, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    for (int64_t i = 0; i < B; ++i) G.I[(size_t)i].mu = hb[(size_t)i] > 0.0 ? hb[(size_t)i] : o.mu_init;
  }
  if (G.bounds_or_slk) {
    for (int64_t i = 0; i < B; ++i) G.hmu[(size_t)i] = G.I[(size_t)i].mu;
    HIP_TRY(hipMemcpyAsync(G.dmub, G.hmu.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (!G.bounds) {   // (the shared bounds are on the device with finite bounds only: the fixed variables need them here)
    HIP_TRY(G.dlo.alloc((size_t)Nz));
    HIP_TRY(G.dhi.alloc((size_t)Nz));
    HIP_TRY(hipMemcpyAsync(G.dlo, G.p->L.var_lo.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(G.dhi, G.p->L.var_hi.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st));
  }
  const size_t blocks = ((size_t)B * Nz + 255) / 256;
  if (blocks > 0x7fffffff) return set_error(DTO_ERR_UNSUPPORTED, "dto_solve_batch_warm: batch too large");
  hipLaunchKernelGGL(k_border_warm_vars, dim3((unsigned)blocks), dim3(256), 0, st, B, Nz, (const double*)s.x, s.ldx, (const double*)s.zl, s.ldzl,
                     (const double*)s.zu, s.ldzu, (const double*)G.dlo, (const double*)G.dhi, (const double*)(G.bounds ? (double*)G.dmub : nullptr),
                     o.bound_push, o.bound_frac, (double*)G.z, (double*)(G.bounds ? (double*)G.zl : nullptr), (double*)(G.bounds ? (double*)G.zu : nullptr));
  HIP_TRY(hipGetLastError());
  if (s.mu) {
    HIP_TRY(hipMemcpy2DAsync(G.lam, Nc * sizeof(double), s.mu, s.ldmu * sizeof(double), Nc * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, st));
    if (G.ni > 0)   // the host keeps the multipliers of the general rows (read after the synchronisation of the slack start)
      HIP_TRY(hipMemcpy2DAsync(G.hnu.data(), ng * sizeof(double), s.mu + Ns, s.ldmu * sizeof(double), ng * sizeof(double), (size_t)B,
                               hipMemcpyDeviceToHost, st));
  }
  if (G.lbfgs && s.qn_s) {
    HIP_TRY(hipMemcpy2DAsync(G.qn.S, Nz * sizeof(double), s.qn_s, s.ldqs * sizeof(double), Nz * sizeof(double), (size_t)B * QnHistory::M,
                             hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpy2DAsync(G.qn.Y, Nz * sizeof(double), s.qn_y, s.ldqy * sizeof(double), Nz * sizeof(double), (size_t)B * QnHistory::M,
                             hipMemcpyDeviceToDevice, st));
    for (int64_t i = 0; i < B; ++i) { G.qn.npairs[(size_t)i] = s.qn_npairs[i]; G.qn.sigma[(size_t)i] = s.qn_sigma[i]; }
  }
  return DTO_OK;
}

// ---- the rest of the point a solve ends at (dto_solve_batch_warm: x and mu are border_loop_end's own copies): strided copies of
//      what the loop has -- bound multipliers, the slacks of the stage rows from the device and of the general rows from the
//      host (as put_nu mirrors their multipliers), the barrier parameter of every instance, the history.  What the problem does
//      not have comes back as zeros.  hout lives in G until border_loop_end has waited for the stream
static int border_loop_end_point(BorderLoop& G, const dto_point& e) {
  const int64_t B = G.B, Nz = G.Nz, ng = G.ng, Ns = G.Ns;
  const size_t D = sizeof(double);
  hipStream_t st = G.st;
  if (e.zl) {
    if (G.bounds) {
      HIP_TRY(hipMemcpy2DAsync(e.zl, e.ldzl * D, G.zl, Nz * D, Nz * D, (size_t)B, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpy2DAsync(e.zu, e.ldzu * D, G.zu, Nz * D, Nz * D, (size_t)B, hipMemcpyDeviceToDevice, st));
    } else {
      HIP_TRY(hipMemset2DAsync(e.zl, e.ldzl * D, 0, Nz * D, (size_t)B, st));
      HIP_TRY(hipMemset2DAsync(e.zu, e.ldzu * D, 0, Nz * D, (size_t)B, st));
    }
  }
  if (e.slack) {
    if (G.nsi > 0) HIP_TRY(hipMemcpy2DAsync(e.slack, e.ldslack * D, G.ss, Ns * D, Ns * D, (size_t)B, hipMemcpyDeviceToDevice, st));
    else if (Ns > 0) HIP_TRY(hipMemset2DAsync(e.slack, e.ldslack * D, 0, Ns * D, (size_t)B, st));
    if (ng > 0) HIP_TRY(hipMemcpy2DAsync(e.slack + Ns, e.ldslack * D, G.hs.data(), ng * D, ng * D, (size_t)B, hipMemcpyHostToDevice, st));
  }
  if (e.barrier) {
    G.hout.assign((size_t)B, 0.0);
    for (int64_t i = 0; i < B && G.barrier; ++i) G.hout[(size_t)i] = G.I[(size_t)i].mu;
    HIP_TRY(hipMemcpyAsync(e.barrier, G.hout.data(), (size_t)B * D, hipMemcpyHostToDevice, st));
  }
  if (e.qn_s) {
    const size_t rows = (size_t)B * QnHistory::M;
    if (G.lbfgs) {
      HIP_TRY(hipMemcpy2DAsync(e.qn_s, e.ldqs * D, G.qn.S, Nz * D, Nz * D, rows, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpy2DAsync(e.qn_y, e.ldqy * D, G.qn.Y, Nz * D, Nz * D, rows, hipMemcpyDeviceToDevice, st));
    } else {
      HIP_TRY(hipMemset2DAsync(e.qn_s, e.ldqs * D, 0, Nz * D, rows, st));
      HIP_TRY(hipMemset2DAsync(e.qn_y, e.ldqy * D, 0, Nz * D, rows, st));
    }
    for (int64_t i = 0; i < B; ++i) {
      e.qn_npairs[i] = G.lbfgs ? G.qn.npairs[(size_t)i] : 0;
      e.qn_sigma[i] = G.lbfgs ? G.qn.sigma[(size_t)i] : 1.0;
    }
  }
  return DTO_OK;
}

// ---- begin: argument checks, row classification, allocation, the start point (pushed inside finite bounds, fixed variables on
//      their values), slacks and multipliers of the inequality rows (s = max(-c, 1e-2), nu = 1, mu_init)
static int border_loop_begin(BorderLoop& G, Problem* p, const dto_options* opt, const dto_batch* b, int64_t ldxo, bool want_mu, int64_t ldmuo,
                             bool lbfgs, const dto_point* start) {
  int rc = p->ensure_device();
  if (rc) return rc;
  const Layout& L = p->L;
  const int64_t B = b->B, Nz = L.Nz, Nc = L.Nc;
  // lbfgs: the limited-memory mode of the tile path (12 border rows are the compact matrix, up to four general rows share its panel).
  // The loop is the same; the step (bordered_step_tile) and the secant pairs after it (border_loop_save_pair) are what differ
  if (lbfgs && (!p->vt->launch_wide || 2 * QnHistory::M + L.Ngen > KB_MAX))
    return set_error(DTO_ERR_UNSUPPORTED, "limited-memory bordered loop: tile path with at most four GeneralConstraint rows");
  if (lbfgs && b->B < 1) return set_error(DTO_ERR_INVALID, "empty batch");
  if (lbfgs && ((!start && b->ldx < Nz) || ldxo < Nz || (want_mu && ldmuo < Nc))) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if (lbfgs && L.Nstage != 0) return set_error(DTO_ERR_UNSUPPORTED, "wide-stage models: dynamics rows, GeneralConstraint rows and bounds only");
  // per-instance parameters (dto_batch.params, [B][ldp]): every callback of this loop and both linear solvers read the instance's own
  // (dto_kkt_assemble / wide_kkt_assemble take them from the batch at every call, a further delta_w attempt at the same point included)
  if (b->params && L.Nw > 0 && b->ldp < L.Nw) return set_error(DTO_ERR_INVALID, "ldp < num_parameters");
  // finite bound sides of the variables that are not fixed (the tests of k_wide_init_bounds: a side is finite inside +-1e300)
  for (int64_t i = 0; i < Nz; ++i)
    if (L.var_lo[i] != L.var_hi[i]) G.n_bound += (L.var_lo[i] > -1e300 ? 1 : 0) + (L.var_hi[i] < 1e300 ? 1 : 0);
  // inequality rows (c <= 0: src/general_constraint.jl:15-19 `indices_inequality`) among the GENERAL rows are carried with slacks
  // g_i + s_i = 0, s_i >= 0 (round 4): the border's diagonal gets s_i / nu_i, its right-hand side mu / nu_i.  Inequality rows of
  // stage Constraints get the same elimination with their slacks on the device (BorderSlack: about T of them per instance), s / nu
  // through dto_kkt_system.sigma_c; dynamics rows are equalities
  const int64_t ng = L.Ngen, Ns = Nc - ng;
  G.ineq.assign((size_t)std::max<int64_t>(1, ng), 0);
  for (int64_t i = 0; i < Nc; ++i) {
    if (L.con_lo[i] == L.con_hi[i]) continue;
    if (i < L.Ndyn || !(L.con_hi[i] == 0.0) || std::isfinite(L.con_lo[i]))
      return set_error(DTO_ERR_UNSUPPORTED, "GeneralConstraint solve path: equality rows and inequality rows c <= 0");
    if (i < Ns) {
      if (G.smask.empty()) G.smask.assign((size_t)Ns, 0);
      G.smask[(size_t)i] = 1; ++G.nsi;
    } else {
      G.ineq[(size_t)(i - Ns)] = 1; ++G.ni;
    }
  }
  const int64_t ni = G.ni, nsi = G.nsi;
  const bool bounds = G.bounds = G.n_bound > 0;
  G.bounds_or_slk = bounds || nsi > 0;
  G.barrier = bounds || ni > 0 || nsi > 0;
  G.nth = nsi > 0 ? 3 : (bounds ? 2 : 1);
  G.lbfgs = lbfgs;
  G.p = p; G.h = reinterpret_cast<dto_problem*>(p); G.st = (hipStream_t)b->stream;
  G.B = B; G.Nz = Nz; G.Nc = Nc; G.ng = ng; G.Ns = Ns;
  if (opt) G.user = *opt; else dto_options_default(&G.user);
  default_opts(G.o, G.user);
  const dto_solver_opts& o = G.o;
  hipStream_t st = G.st;
  HIP_TRY(G.z.alloc((size_t)B * Nz));
  HIP_TRY(G.lam.alloc((size_t)B * Nc));
  HIP_TRY(G.dz.alloc((size_t)B * Nz));
  HIP_TRY(G.dlam.alloc((size_t)B * Nc));
  HIP_TRY(G.zt.alloc((size_t)B * Nz));
  HIP_TRY(G.df.alloc((size_t)B));
  HIP_TRY(G.dc.alloc((size_t)B * Nc));
  HIP_TRY(G.dal.alloc((size_t)B));
  HIP_TRY(G.dth.alloc((size_t)B * G.nth));   // (with bounds: theta and sum log(gap) of a trial point; with stage slacks sum log(s) behind)
  if (ni > 0) {
    for (DevBuf<double>* q : {&G.dgd, &G.dgs, &G.dst}) HIP_TRY(q->alloc((size_t)B * ng));
  }
  if (G.bounds_or_slk) {
    HIP_TRY(G.dmub.alloc((size_t)B));
    HIP_TRY(G.dad.alloc((size_t)B));
  }
  if (bounds) {
    // the guess pushed inside the bounds, fixed variables on their values, z_L / z_U on the central path of mu_init: the cold
    // start of the tile solver, instance-major over [B][Nz] with the problem's shared bounds (ldb = 0)
    HIP_TRY(G.zl.alloc((size_t)B * Nz));
    HIP_TRY(G.zu.alloc((size_t)B * Nz));
    HIP_TRY(G.dlo.alloc((size_t)Nz));
    HIP_TRY(G.dhi.alloc((size_t)Nz));
    HIP_TRY(hipMemcpyAsync(G.dlo, L.var_lo.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(G.dhi, L.var_hi.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st));
    if (!start) {
      HIP_TRY(hipMemcpy2DAsync(G.z, Nz * sizeof(double), b->x, b->ldx * sizeof(double), Nz * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_wide_init_bounds, dim3((unsigned)(B * AXPY_BLOCKS_PER_ROW)), dim3(256), 0, st, (double*)G.z, (double*)G.zl, (double*)G.zu,
                         (const double*)G.dlo, (const double*)G.dhi, (int64_t)0, o.mu_init, o.bound_push, o.bound_frac, Nz);
      HIP_TRY(hipGetLastError());
    }
    G.bar.z = G.z; G.bar.zl = G.zl; G.bar.zu = G.zu; G.bar.lo = G.dlo; G.bar.hi = G.dhi; G.bar.mu = G.dmub;
  } else if (!start) {
    // the guess, with the fixed variables put on their values
    std::vector<double>& hz = G.hz;
    hz.resize((size_t)B * Nz);
    HIP_TRY(hipMemcpy2DAsync(hz.data(), Nz * sizeof(double), b->x, b->ldx * sizeof(double), Nz * sizeof(double), (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < B; ++i)
      for (int64_t k = 0; k < Nz; ++k)
        if (L.var_lo[k] == L.var_hi[k]) hz[(size_t)i * Nz + k] = L.var_lo[k];
    HIP_TRY(hipMemcpyAsync(G.z, hz.data(), hz.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (!start || !start->mu) HIP_TRY(hipMemsetAsync(G.lam, 0, (size_t)B * Nc * sizeof(double), st));
  if (lbfgs) {
    if ((rc = ensure_border_csc(p))) return rc;
    if ((rc = G.qn.init(B, Nz, st))) return rc;
  }
  G.I.assign((size_t)B, GlobInst());
  if (G.barrier)
    for (int64_t i = 0; i < B; ++i) G.I[(size_t)i].mu = o.mu_init;
  const size_t nBg = (size_t)B * std::max<int64_t>(1, ng);
  G.hmu.assign((size_t)(G.bounds_or_slk ? B : 0), 0.0); G.had = G.hmu;
  for (std::vector<double>* v : {&G.hs, &G.hnu, &G.hds, &G.hgd, &G.hgs, &G.hst}) v->assign(nBg, 0.0);
  for (std::vector<double>* v : {&G.dwv, &G.hf, &G.hal, &G.hphi0}) v->assign((size_t)B, 0.0);
  G.hth.assign((size_t)B * G.nth, 0.0);
  G.okv.assign((size_t)B, 0);
  G.mu_moved.assign((size_t)B, 0);
  G.bz = *b;
  G.bz.x = G.z; G.bz.ldx = Nz;
  if (start && (rc = border_loop_start_point(G, *start))) return rc;
  if (nsi > 0) {
    // the same start for the slacks of the inequality stage rows, on the device: s = max(-c, 1e-2), nu = 1 in their entries of lam
    HIP_TRY(G.ss.alloc((size_t)B * Ns));
    HIP_TRY(G.sds.alloc((size_t)B * Ns));
    HIP_TRY(G.dsmask.alloc((size_t)Ns));
    HIP_TRY(hipMemcpyAsync(G.dsmask, G.smask.data(), (size_t)Ns * sizeof(int), hipMemcpyHostToDevice, st));
    G.slk.s = G.ss; G.slk.ds = G.sds; G.slk.mask = G.dsmask; G.slk.mu = G.dmub; G.slk.Ns = Ns;
    if ((rc = dto_eval_g_batch(G.h, &G.bz, G.dc, Nc))) return rc;
    if (start)
      hipLaunchKernelGGL(k_border_slack_warm, dim3((unsigned)(((size_t)B * Ns + 255) / 256)), dim3(256), 0, st, B, Nc, G.slk, (const double*)G.dc,
                         (double*)G.lam, (const double*)start->slack, start->ldslack, o.bound_push);
    else
      hipLaunchKernelGGL(k_border_slack_init, dim3((unsigned)(((size_t)B * Ns + 255) / 256)), dim3(256), 0, st, B, Nc, G.slk, (const double*)G.dc,
                         (double*)G.lam);
    HIP_TRY(hipGetLastError());
  }
  if (ni > 0) {
    // slacks from the constraint values at the guess, pushed inside (s >= 1e-2), multipliers 1 (Ipopt's bound_mult_init_val), mu_init
    if ((rc = dto_eval_g_batch(G.h, &G.bz, G.dc, Nc))) return rc;
    std::vector<double> hg((size_t)B * ng);
    HIP_TRY(hipMemcpy2DAsync(hg.data(), ng * sizeof(double), G.dc + Ns, Nc * sizeof(double), ng * sizeof(double), (size_t)B, hipMemcpyDeviceToHost, st));
    if (start && start->slack)   // (hnu holds the caller's multipliers of the general rows: border_loop_start_point)
      HIP_TRY(hipMemcpy2DAsync(G.hs.data(), ng * sizeof(double), start->slack + Ns, start->ldslack * sizeof(double), ng * sizeof(double), (size_t)B,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < B; ++i)
      for (int64_t q = 0; q < ng; ++q) {
        const size_t e = (size_t)(i * ng + q);
        if (!G.ineq[(size_t)q]) { G.hs[e] = 0.0; continue; }
        if (start) {   // the warm rule of the stage rows' slacks (k_border_slack_warm), here on the host
          const WarmSlack w = warm_slack(hg[e], G.hs[e], G.hnu[e], G.I[(size_t)i].mu, o.bound_push);
          G.hs[e] = w.s; G.hnu[e] = w.nu;
        } else { G.hs[e] = std::max(-hg[e], 1e-2); G.hnu[e] = 1.0; }
      }
    if ((rc = G.put_nu())) return rc;
  }
  G.t_start = std::chrono::steady_clock::now();
  return DTO_OK;
}

// ---- the step at the current point: what it needs of the host state (s / nu and mu / nu of the inequality general rows, the
//      barrier parameter), then the delta_w ladder per instance (Algorithm IC) around bordered_step -- all instances share the
//      sweeps, a further attempt keeps the point's derivatives.  (difference 3) the first delta_w is 0 unless the last line search
//      failed: no decay of the last value, no Gauss-Newton fallback
static int border_loop_step(BorderLoop& G) {
  const int64_t B = G.B, ng = G.ng;
  const dto_solver_opts& o = G.o;
  hipStream_t st = G.st;
  if (G.ni > 0) {
    for (int64_t i = 0; i < B; ++i)
      for (int64_t q = 0; q < ng; ++q) {
        const size_t e = (size_t)(i * ng + q);
        G.hgd[e] = G.ineq[(size_t)q] ? G.hs[e] / G.hnu[e] : 0.0;
        G.hgs[e] = G.ineq[(size_t)q] ? G.I[(size_t)i].mu / G.hnu[e] : 0.0;
      }
    HIP_TRY(hipMemcpyAsync(G.dgd, G.hgd.data(), (size_t)B * ng * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(G.dgs, G.hgs.data(), (size_t)B * ng * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (G.bounds_or_slk) {   // the barrier parameter the step is computed with
    for (int64_t i = 0; i < B; ++i) G.hmu[(size_t)i] = G.I[(size_t)i].mu;
    HIP_TRY(hipMemcpyAsync(G.dmub, G.hmu.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  }
  for (int64_t i = 0; i < B; ++i) G.dwv[(size_t)i] = G.I[(size_t)i].ls_fail ? ladder_after_ls_fail(o, G.I[(size_t)i].dlast) : 0.0;
  G.bs = BorderStats();
  G.bs.qn = G.lbfgs ? &G.qn : nullptr;
  for (int attempt = 0;; ++attempt) {
    G.bs.reuse_point = attempt > 0;
    const int rc = bordered_step(G.p, &G.bz, G.lam, G.Nc, G.dwv.data(), o.delta_c, G.dz, G.Nz, G.dlam, G.Nc, G.okv.data(), &G.bs, true,
                                 G.ni > 0 ? G.dgd : nullptr, G.ni > 0 ? G.dgs : nullptr, G.bounds ? &G.bar : nullptr, G.nsi > 0 ? &G.slk : nullptr);
    if (rc) return rc;
    bool again = false;
    for (int64_t i = 0; i < B; ++i) {
      if (!G.running(i) || G.okv[(size_t)i] || attempt >= o.max_refactor) continue;
      G.dwv[(size_t)i] = ladder_next(o, G.dwv[(size_t)i], G.I[(size_t)i].dlast);
      again = true;
    }
    if (!again) return DTO_OK;
  }
}

// the host border's whole vectors (BorderStats grad, c, rx, dz, dmu; hm: the multipliers) reduced to what the device border delivers:
// theta_1, theta_inf, dual infeasibility over the free variables, sum |lam|, grad f' dz per instance in hst5, the steps of the
// general rows' multipliers in hdnu.  Sums run over k ascending, the slack of an inequality general row is added before the
// absolute value
static void border_loop_host_stats(BorderLoop& G, const std::vector<double>& hm) {
  const Layout& L = G.p->L;
  const int64_t Nz = G.Nz, Nc = G.Nc, ng = G.ng, Ns = G.Ns;
  const BorderStats& bs = G.bs;
  G.hst5.assign((size_t)G.B * 5, 0.0);
  G.hdnu.resize((size_t)G.B * ng);
  for (int64_t i = 0; i < G.B; ++i) {
    for (int64_t q = 0; q < ng; ++q) G.hdnu[(size_t)(i * ng + q)] = bs.dmu[(size_t)i * Nc + Ns + q];
    if (!G.running(i)) continue;
    double th1 = 0, thinf = 0, dinf = 0, slam = 0, gd = 0;
    for (int64_t k = 0; k < Nc; ++k) {
      const double sk = (k >= Ns && G.ineq[(size_t)(k - Ns)]) ? G.hs[(size_t)(i * ng + (k - Ns))] : 0.0;   // inequality rows: g + s
      const double v = std::fabs(bs.c[(size_t)i * Nc + k] + sk); th1 += v; thinf = std::max(thinf, v); slam += std::fabs(hm[(size_t)i * Nc + k]);
    }
    for (int64_t k = 0; k < Nz; ++k) {
      if (L.var_lo[k] != L.var_hi[k]) dinf = std::max(dinf, std::fabs(bs.rx[(size_t)i * Nz + k]));
      gd += bs.grad[(size_t)i * Nz + k] * bs.dz[(size_t)i * Nz + k];
    }
    double* q5 = &G.hst5[(size_t)i * 5];
    q5[0] = th1; q5[1] = thinf; q5[2] = dinf; q5[3] = slam; q5[4] = gd;
  }
}

// ---- what the host rules need of the point and the step, per instance: the objective (hf, and phi_0 of the line search), five
//      numbers in hst5 -- behind them BORDER_BAR_NSTAT with bounds and BORDER_SLK_NSTAT with inequality stage rows, in the same
//      buffer and the same copy (difference 6: the tile path has all of this from k_wide_step) -- and the steps of the general
//      rows' multipliers (hdnu).  The device borders left grad f, c and r_x in the workspace (bs.d_*): three reductions, one copy;
//      the host border left vectors: border_loop_host_stats
static int border_loop_point_stats(BorderLoop& G) {
  const int64_t B = G.B, Nz = G.Nz, Nc = G.Nc, ng = G.ng, Ns = G.Ns;
  hipStream_t st = G.st;
  const BorderStats& bs = G.bs;
  const bool dev_stats = bs.d_grad != nullptr;
  std::vector<double> hm;
  if (dev_stats) {
    const size_t n5 = (size_t)B * 5, nbar = n5 + (G.bounds ? (size_t)B * BORDER_BAR_NSTAT : 0),
                 nstat = nbar + (G.nsi > 0 ? (size_t)B * BORDER_SLK_NSTAT : 0);
    if (!G.d5) HIP_TRY(G.d5.alloc(nstat));
    if (G.ni > 0) HIP_TRY(hipMemcpyAsync(G.dst, G.hs.data(), (size_t)B * ng * sizeof(double), hipMemcpyHostToDevice, st));   // slack shift of theta
    hipLaunchKernelGGL(k_border_stats, dim3((unsigned)B), dim3(64), 0, st, Nz, Nc, bs.d_c, bs.d_rx, bs.d_grad, (const double*)G.dz, (const double*)G.lam,
                       (const int*)G.p->d_var_fixed, (const double*)(G.ni > 0 ? G.dst : nullptr), Ns, ng, G.d5, (const double*)G.slk.s, G.slk.Ns);
    if (G.bounds)
      hipLaunchKernelGGL(k_border_bar_stats, dim3((unsigned)B), dim3(64), 0, st, Nz, G.bar, (const double*)G.dz, bs.d_rx, (const int*)G.p->d_var_fixed,
                         G.o.tau_min, G.d5 + n5);
    if (G.nsi > 0)
      hipLaunchKernelGGL(k_border_slack_stats, dim3((unsigned)B), dim3(64), 0, st, Nc, G.slk, (const double*)G.lam, (const double*)G.dlam, G.o.tau_min,
                         G.d5 + nbar);
    G.hst5.resize(nstat);
    HIP_TRY(hipMemcpyAsync(G.hst5.data(), G.d5, G.hst5.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    G.hdnu.resize((size_t)B * ng);
    if (ng > 0)
      HIP_TRY(hipMemcpy2DAsync(G.hdnu.data(), ng * sizeof(double), G.dlam + Ns, Nc * sizeof(double), ng * sizeof(double), (size_t)B, hipMemcpyDeviceToHost, st));
  }
  const int rc = dto_eval_f_batch(G.h, &G.bz, G.df);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(G.hf.data(), G.df, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
  if (!dev_stats) {
    hm.resize((size_t)B * Nc);
    HIP_TRY(hipMemcpyAsync(hm.data(), G.lam, hm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (!dev_stats) border_loop_host_stats(G, hm);
  G.hphi0 = G.hf;   // objective at the current point: the line search's phi_0
  return DTO_OK;
}

// ---- convergence test at the point the step was computed at (Ipopt's scaled error, reference Options) and monotone barrier
//      update; host arithmetic only.  Fills th0 and gphid (theta_1 and the merit's directional derivative) for the line search and
//      the slack steps hds of the inequality general rows; false when no instance is left running.
//      (difference 1) no acceptable-level termination: terminal_status with acc_count = 0 never returns 4.
//      (difference 4) dlast is recorded here, after the test, not when the factorisation is accepted; a step from a matrix whose
//      inertia was never corrected sets ls_fail.
//      (difference 5) an instance whose barrier parameter moved keeps the step of the old one unused: mu_moved gives it alpha = 0
//      for this round (border_loop_step_limits) and the iteration is not counted (border_loop_trials)
static bool border_loop_convergence(BorderLoop& G) {
  const dto_solver_opts& o = G.o;
  const int64_t B = G.B, ng = G.ng;
  bool any = false;
  G.th0.assign((size_t)B, 0.0); G.gphid.assign((size_t)B, 0.0);
  for (int64_t i = 0; i < B; ++i) {
    GlobInst& s = G.I[(size_t)i];
    if (s.status != 0) continue;
    const double* q5 = &G.hst5[(size_t)i * 5];
    const double th1 = q5[0], thinf = q5[1], slam = q5[3], gd = q5[4];
    double dinf = q5[2];
    // complementarity of the slack / multiplier pairs against mu_target (termination; against mu: the barrier update below); the
    // step of the inequality rows: ds = (mu - s nu) / nu - (s / nu) dnu, barrier term of the merit's directional derivative
    double c0 = 0.0, snu = 0.0, bar_d = 0.0;
    for (int64_t q = 0; q < ng; ++q) {
      if (!G.ineq[(size_t)q]) continue;
      const size_t e = (size_t)(i * ng + q);
      const double sv = G.hs[e], nv = G.hnu[e], dnu = G.hdnu[e];
      c0 = std::max(c0, std::fabs(sv * nv - o.mu_target)); snu += std::fabs(nv);
      G.hds[e] = (s.mu - sv * nv) / nv - (sv / nv) * dnu;
      bar_d += G.hds[e] / sv;
    }
    // finite variable bounds: the bound multipliers join the scaling, the largest and the smallest gap z give the complementarity
    // error against any mu (as wide_convergence forms it), r_x already holds - z_L + z_U
    const double* qb = G.bound_stats(i);
    auto compl_bounds = [&](double mu_at) {
      if (!qb) return 0.0;
      const double szmin = qb[BORDER_BAR_ISZMAX] > 0.0 ? 1.0 / qb[BORDER_BAR_ISZMAX] : 1e300;
      return std::max(qb[BORDER_BAR_SZMAX] - mu_at, mu_at - szmin);
    };
    if (qb) { dinf = qb[BORDER_BAR_DINF]; c0 = std::max(c0, compl_bounds(o.mu_target)); }
    // inequality stage rows: the same two extremes of s nu from the device (nsi > 0 implies the device border), their ds / s in
    // the merit's directional derivative exactly as the general rows' slacks
    const double* qs = G.slack_stats(i);
    auto compl_slack = [&](double mu_at) {
      if (!qs) return 0.0;
      const double snumin = qs[BORDER_SLK_ISNUMAX] > 0.0 ? 1.0 / qs[BORDER_SLK_ISNUMAX] : 1e300;
      return std::max(qs[BORDER_SLK_SNUMAX] - mu_at, mu_at - snumin);
    };
    if (qs) { c0 = std::max(c0, compl_slack(o.mu_target)); snu += qs[BORDER_SLK_SUMNU]; bar_d += qs[BORDER_SLK_DSS]; }
    // (the slack's bound multiplier of a slack-eliminated row IS its nu: it counts among the bound multipliers, as the slack
    //  multipliers do in conv_body)
    const ErrScale es = ipopt_scaling(o, slam, G.Nc, snu + (qb ? qb[BORDER_BAR_SUMZ] : 0.0), G.ni + G.n_bound + G.nsi);
    const IterMeasures m{G.hf[(size_t)i], th1, thinf, dinf, std::max(std::max(dinf / es.sd, thinf), c0 / es.sc), c0};
    G.mu_moved[(size_t)i] = 0;
    s.status = terminal_status(o, s.iter, m, 0);
    if (s.status == 0 && G.barrier) {
      // Ipopt's monotone rule: once the barrier problem is solved to kappa_eps mu the parameter drops (and the filter is reset);
      // the step computed above belongs to the old mu: this instance waits one round (alpha = 0) for the step of the new one
      const double mu = monotone_mu(o, s.mu, std::max(dinf / es.sd, thinf), es.sc, [&](double mu_at) {
        double c = std::max(compl_bounds(mu_at), compl_slack(mu_at));
        for (int64_t q = 0; q < ng; ++q)
          if (G.ineq[(size_t)q]) c = std::max(c, std::fabs(G.hs[(size_t)(i * ng + q)] * G.hnu[(size_t)(i * ng + q)] - mu_at));
        return c;
      });
      if (mu != s.mu) { s.mu = mu; s.filter_n = 0; G.mu_moved[(size_t)i] = 1; }
    }
    init_theta_limits(s, th1);
    G.th0[(size_t)i] = th1; G.gphid[(size_t)i] = gd - s.mu * bar_d;
    if (qb) G.gphid[(size_t)i] += qb[BORDER_BAR_DPHI];
    if (s.status == 0) {
      any = true;
      if (G.dwv[(size_t)i] > 0.0) s.dlast = G.dwv[(size_t)i]; else s.dlast = 0.0;
      if (!G.okv[(size_t)i]) s.ls_fail = 1;
    }
  }
  return any;
}

// ---- where the trials start: alpha_p^max and alpha_d^max, the fraction-to-the-boundary steps combined by min over the bounds and
//      the slacks of inequality stage rows (from the device's statistics) and of inequality general rows (here), and phi_0, the
//      barrier function f - mu (sum log(gap) + sum log s) at the point.  Without a barrier alpha^max = 1 and phi_0 = f
static void border_loop_step_limits(BorderLoop& G) {
  const int64_t B = G.B, ng = G.ng;
  G.chosen_a.assign((size_t)B, -1.0);
  G.ftype_a.assign((size_t)B, 0);
  G.best_a.assign((size_t)B, MostFeasible());
  G.apmax.assign((size_t)B, 1.0); G.admax.assign((size_t)B, 1.0);
  for (int64_t i = 0; i < B && G.barrier; ++i) {
    const GlobInst& s = G.I[(size_t)i];
    if (s.status != 0) continue;
    if (G.mu_moved[(size_t)i]) { G.chosen_a[(size_t)i] = 0.0; continue; }   // waits for the step of its new barrier parameter
    double &ap = G.apmax[(size_t)i], &ad = G.admax[(size_t)i], &phi0 = G.hphi0[(size_t)i];
    if (const double* qb = G.bound_stats(i)) {
      ap = qb[BORDER_BAR_APMAX]; ad = qb[BORDER_BAR_ADMAX];
      phi0 -= s.mu * qb[BORDER_BAR_LOGBAR];
    }
    if (const double* qs = G.slack_stats(i)) {   // the slacks of the inequality stage rows: the same three numbers
      ap = std::min(ap, qs[BORDER_SLK_APMAX]); ad = std::min(ad, qs[BORDER_SLK_ADMAX]);
      phi0 -= s.mu * qs[BORDER_SLK_LOGS];
    }
    if (G.ni == 0) continue;
    const double tau = std::max(G.o.tau_min, 1.0 - s.mu);
    double lb = 0.0;
    for (int64_t q = 0; q < ng; ++q) {
      if (!G.ineq[(size_t)q]) continue;
      const size_t e = (size_t)(i * ng + q);
      const double dnu = G.hdnu[e];
      if (G.hds[e] < 0.0) ap = std::min(ap, -tau * G.hs[e] / G.hds[e]);
      if (dnu < 0.0) ad = std::min(ad, -tau * G.hnu[e] / dnu);
      lb += std::log(G.hs[e]);
    }
    phi0 -= s.mu * lb;
  }
}

// ---- filter line search over alpha = alpha_p^max 2^-k: objective and l1 violation of a trial point from the callbacks (the
//      violation summed on the device, with bounds or stage slacks the sums of logarithms in the same launch: difference 6, the
//      tile path reads a merit table of all trials).  Trial k is evaluated only while some running instance has not accepted a
//      shorter-numbered one (round 4: all eight trials of every iteration, each with its constraint vector over PCIe, were most of
//      the 8.7 ms an iteration of a 512-instance batch took; a Newton step near the solution is accepted at alpha = 1).  Then the
//      decision per instance: hal, the alpha it moves with.  (difference 2) ls_fail after an accepted trial is okv ? 0 : 1
static int border_loop_trials(BorderLoop& G) {
  constexpr int TRIALS = DTO_LS_TRIALS;
  const int64_t B = G.B, Nz = G.Nz, Nc = G.Nc, ng = G.ng, Ns = G.Ns;
  const int nth = G.nth;
  hipStream_t st = G.st;
  auto undecided = [&](int64_t i) { return G.running(i) && G.chosen_a[(size_t)i] < 0.0; };
  for (int k = 0; k < TRIALS; ++k) {
    bool some = false;
    for (int64_t i = 0; i < B; ++i) some = some || undecided(i);
    if (!some) break;
    const double alpha2 = std::ldexp(1.0, -k);
    for (int64_t i = 0; i < B; ++i) G.hal[(size_t)i] = undecided(i) ? G.apmax[(size_t)i] * alpha2 : 0.0;
    if (G.ni > 0) {
      for (int64_t i = 0; i < B; ++i)
        for (int64_t q = 0; q < ng; ++q) {
          const size_t e = (size_t)(i * ng + q);
          G.hst[e] = G.ineq[(size_t)q] ? G.hs[e] + G.hal[(size_t)i] * G.hds[e] : 0.0;
        }
      HIP_TRY(hipMemcpyAsync(G.dst, G.hst.data(), (size_t)B * ng * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(G.zt, G.z, (size_t)B * Nz * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(G.dal, G.hal.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rows_axpy, dim3((unsigned)(B * AXPY_BLOCKS_PER_ROW)), dim3(256), 0, st, (double*)G.zt, (const double*)G.dz, (const double*)G.dal,
                       Nz, Nz, Nz);
    dto_batch bt = G.bz;
    bt.x = G.zt;
    int rc;
    if ((rc = dto_eval_f_batch(G.h, &bt, G.df))) return rc;
    if ((rc = dto_eval_g_batch(G.h, &bt, G.dc, Nc))) return rc;
    const double* shift = G.ni > 0 ? (const double*)G.dst : nullptr;
    if (G.bounds_or_slk)   // the violation and sum log(gap) of the trial point in one launch, both in the copy of theta (with inequality
                           // stage rows: their slacks at alpha in the violation, and sum log of them as a third number)
      hipLaunchKernelGGL(k_border_trial, dim3((unsigned)B), dim3(64), 0, st, (const double*)G.dc, Nc, Nc, shift, Ns, ng,
                         (const double*)(G.bounds ? (double*)G.zt : nullptr), Nz, (const double*)G.dlo, (const double*)G.dhi, (double*)G.dth, G.slk,
                         (const double*)G.dal);
    else
      hipLaunchKernelGGL(k_rows_abs_sum, dim3((unsigned)B), dim3(64), 0, st, (const double*)G.dc, Nc, Nc, (double*)G.dth, shift, Ns, ng);
    HIP_TRY(hipMemcpyAsync(G.hf.data(), G.df, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(G.hth.data(), G.dth, G.hth.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < B; ++i) {
      if (!undecided(i)) continue;
      GlobInst& s = G.I[(size_t)i];
      double pk = G.hf[(size_t)i];
      const double tk = G.hth[(size_t)(nth * i)];
      if (G.bounds) pk -= s.mu * G.hth[(size_t)(nth * i + 1)];
      if (G.nsi > 0) pk -= s.mu * G.hth[(size_t)(nth * i + 2)];
      for (int64_t q = 0; q < ng && G.ni > 0; ++q)
        if (G.ineq[(size_t)q]) pk -= s.mu * std::log(G.hst[(size_t)(i * ng + q)]);
      note_most_feasible(G.best_a[(size_t)i], k, tk);
      const TrialVerdict v = trial_acceptable(s, G.th0[(size_t)i], G.hphi0[(size_t)i], G.gphid[(size_t)i], G.hal[(size_t)i], tk, pk);
      if (v != TRIAL_REJECTED) { G.chosen_a[(size_t)i] = G.hal[(size_t)i]; G.ftype_a[(size_t)i] = v == TRIAL_ACCEPTED_FTYPE; }
    }
  }
  for (int64_t i = 0; i < B; ++i) {
    G.hal[(size_t)i] = 0.0;
    GlobInst& s = G.I[(size_t)i];
    if (s.status != 0) continue;
    if (G.barrier && G.mu_moved[(size_t)i]) continue;   // no step, no iteration: its barrier parameter just moved
    // (an instance whose trials were all rejected had all TRIALS of them evaluated)
    G.hal[(size_t)i] = finish_line_search(s, G.chosen_a[(size_t)i], G.ftype_a[(size_t)i] != 0, G.best_a[(size_t)i], G.th0[(size_t)i], G.hphi0[(size_t)i],
                                          G.apmax[(size_t)i], TRIALS, G.okv[(size_t)i] ? 0 : 1);
    s.iter++;
  }
  return DTO_OK;
}

// ---- take the steps: bound multipliers first (their update reads the old point; alpha_d^max with the kappa_Sigma clamp against
//      the instance's mu), then z, then lam -- with inequality stage rows their multipliers move with alpha_d and are clamped, their
//      slacks with alpha -- and on the host the general rows: equality multipliers move with the primal step, slack / multiplier pairs
//      of the inequality rows with alpha and the common alpha_d (difference 6), then Ipopt's kappa_sigma safeguard; mirrored into
//      lam.  An instance that takes no step (terminated, or its mu just moved) keeps everything
static int border_loop_take_steps(BorderLoop& G) {
  const double kappa_sigma = 1e10;
  const int64_t B = G.B, Nz = G.Nz, Nc = G.Nc, ng = G.ng;
  hipStream_t st = G.st;
  const dim3 grid((unsigned)(B * AXPY_BLOCKS_PER_ROW));
  HIP_TRY(hipMemcpyAsync(G.dal, G.hal.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  if (G.bounds_or_slk) {
    for (int64_t i = 0; i < B; ++i) G.had[(size_t)i] = G.hal[(size_t)i] == 0.0 ? 0.0 : G.admax[(size_t)i];
    HIP_TRY(hipMemcpyAsync(G.dad, G.had.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (G.bounds)
    hipLaunchKernelGGL(k_wide_update_bounds, grid, dim3(256), 0, st, (const double*)G.z, (const double*)G.dz, (double*)G.zl, (double*)G.zu,
                       (const double*)G.dlo, (const double*)G.dhi, (int64_t)0, (const double*)G.dal, (const double*)G.dad, (const double*)G.dmub, Nz);
  hipLaunchKernelGGL(k_rows_axpy, grid, dim3(256), 0, st, (double*)G.z, (const double*)G.dz, (const double*)G.dal, Nz, Nz, Nz);
  if (G.nsi > 0)
    hipLaunchKernelGGL(k_border_slack_update, grid, dim3(256), 0, st, Nc, G.slk, (double*)G.lam, (const double*)G.dlam, (const double*)G.dal,
                       (const double*)G.dad, kappa_sigma, AXPY_BLOCKS_PER_ROW);
  else
    hipLaunchKernelGGL(k_rows_axpy, grid, dim3(256), 0, st, (double*)G.lam, (const double*)G.dlam, (const double*)G.dal, Nc, Nc, Nc);
  if (G.ni == 0) return DTO_OK;
  for (int64_t i = 0; i < B; ++i) {
    const double al = G.hal[(size_t)i];
    if (!G.running(i) && al == 0.0) continue;
    const double ad = al == 0.0 ? 0.0 : G.admax[(size_t)i];
    for (int64_t q = 0; q < ng; ++q) {
      const size_t e = (size_t)(i * ng + q);
      const double dnu = G.hdnu[e];
      if (!G.ineq[(size_t)q]) { G.hnu[e] += al * dnu; continue; }
      G.hs[e] += al * G.hds[e];
      G.hnu[e] += ad * dnu;
      const double mu_i = G.I[(size_t)i].mu;
      G.hnu[e] = std::max(std::min(G.hnu[e], kappa_sigma * mu_i / G.hs[e]), mu_i / (kappa_sigma * G.hs[e]));
    }
  }
  return G.put_nu();
}

// ---- limited-memory mode: save the step just taken, and grad_x L at the point it left with the multipliers it arrived at -- grad f
//      and J of that point are still in the step's workspace.  The pair joins the history when the next step has the derivatives of
//      the new point (qn_update).  An instance that took no step (alpha = 0) saves nothing and pushes nothing
static int border_loop_save_pair(BorderLoop& G) {
  Problem* p = G.p;
  hipLaunchKernelGGL(k_border_qn_save, dim3((unsigned)(((size_t)G.B * G.Nz + 255) / 256)), dim3(256), 0, G.st, G.B, G.Nz, p->L.nnzJ, G.bs.d_J, G.bs.d_grad,
                     (const double*)G.lam, G.Nc, (const int*)p->d_csc_ptr, (const int*)p->d_csc_k, (const int*)p->d_csc_row, (const double*)G.dz,
                     (const double*)G.dal, (double*)G.qn.s, (double*)G.qn.gl);
  HIP_TRY(hipGetLastError());
  for (int64_t i = 0; i < G.B; ++i) G.qn.pending[(size_t)i] = G.hal[(size_t)i] != 0.0 ? 1 : 0;
  return DTO_OK;
}

// ---- end: the iterate and the multipliers to the caller, status (a running instance that ran out of max_cpu_time:
//      DTO_STATUS_CPU_TIME) and iteration counts; with an end point (dto_solve_batch_warm) the rest of the primal-dual point
static int border_loop_end(BorderLoop& G, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, int32_t* status, int32_t* iterations,
                           const dto_point* end) {
  const int64_t B = G.B, Nz = G.Nz, Nc = G.Nc;
  HIP_TRY(hipMemcpy2DAsync(x_out, ldxo * sizeof(double), G.z, Nz * sizeof(double), Nz * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, G.st));
  if (mu_out) HIP_TRY(hipMemcpy2DAsync(mu_out, ldmuo * sizeof(double), G.lam, Nc * sizeof(double), Nc * sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, G.st));
  int rc;
  if (end && (rc = border_loop_end_point(G, *end))) return rc;
  HIP_TRY(hipStreamSynchronize(G.st));
  for (int64_t i = 0; i < B; ++i) {
    if (status) status[i] = (G.running(i) && G.timed_out) ? DTO_STATUS_CPU_TIME : G.I[(size_t)i].status;
    if (iterations) iterations[i] = G.I[(size_t)i].iter;
  }
  return DTO_OK;
}

static int general_solve_batch(Problem* p, const dto_options* opt, const dto_batch* b, double* x_out, int64_t ldxo,
                               double* mu_out, int64_t ldmuo, int32_t* status, int32_t* iterations, bool lbfgs, const dto_point* start,
                               const dto_point* end) {
  BorderLoop G;   // (its device buffers are released on every return)
  int rc = border_loop_begin(G, p, opt, b, ldxo, mu_out != nullptr, ldmuo, lbfgs, start);
  if (rc) return rc;
  for (;;) {
    if ((rc = border_loop_step(G))) return rc;
    if ((rc = border_loop_point_stats(G))) return rc;
    if (!border_loop_convergence(G)) break;
    border_loop_step_limits(G);
    if ((rc = border_loop_trials(G))) return rc;
    if ((rc = border_loop_take_steps(G))) return rc;
    if (G.lbfgs && (rc = border_loop_save_pair(G))) return rc;
    if (G.user.max_cpu_time > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - G.t_start).count() > G.user.max_cpu_time) {
      G.timed_out = true;
      break;
    }
  }
  return border_loop_end(G, x_out, ldxo, mu_out, ldmuo, status, iterations, end);
}


// ---- what dto_kkt_border_factor and dto_kkt_lbfgs_border share: the workspace of a border of nb rows (border_prepare), and, once
//      the panel stands in W.g, Y = K^-1 G', the Schur complement and its LU (border_finish)
struct BorderPlan {
  int64_t B = 0, chunk = 0, n_c = 0;
  int chunks = 0;
};
static int border_prepare(Problem* p, int64_t nb, bool has_gc, BorderPlan& P) {
  const bool wide = p->vt->launch_wide != nullptr;
  const int64_t Nz = p->L.Nz, Nc = kkt_rows(p), N = Nz + Nc;
  int rc;
  const int64_t B = wide ? p->wide_kkt->B : p->solver->B;
  if (!p->kkt_border) p->kkt_border = new KktBorder();
  KktBorder& W = *p->kkt_border;
  W.valid = false;
  // doubles of k per workgroup of k_border_gram, rounded up to the slab; read at every call so that a test can force several
  // chunks on a small system (the sums of a result depend on it, nothing else does)
  int64_t chunk = KB_CHUNK_DEFAULT;
  if (const char* e = getenv("DTO_BORDER_GRAM_CHUNK")) {
    const long long v = atoll(e);
    if (v > 0) chunk = std::min<long long>(v, (long long)1 << 40);
  }
  chunk = (chunk + KB_KT - 1) / KB_KT * KB_KT;
  const int64_t n_c = has_gc ? Nc : 0;   // without g_c the constraint part of every border row is zero: the product skips it
  const int chunks = (int)((Nz + n_c + chunk - 1) / chunk);
  const size_t rows = (size_t)B * (size_t)nb;
  auto grow = [&](DevBuf<double>& buf, size_t need, const char* name, const std::string& shape) {
    return grow_buf(buf, need, ("dto_kkt_border_factor: hipMalloc of " + std::string(name) + " (" + std::to_string(need * sizeof(double)) +
                                " bytes: " + shape + ")").c_str());
  };
  const std::string panel = std::to_string(B) + " instances x " + std::to_string(nb) + " rows x " + std::to_string(N) + " doubles";
  if ((rc = grow(W.g, rows * (size_t)N, "the border panel", panel))) return rc;
  if ((rc = grow(W.y, rows * (size_t)N, "K^-1 G'", panel))) return rc;
  if ((rc = grow(W.part, (size_t)B * (size_t)chunks * 256, "the partial products",
                 std::to_string(B) + " instances x " + std::to_string(chunks) + " chunks x 256 doubles"))) return rc;
  if ((rc = grow(W.lu, (size_t)B * 256, "the LU of the Schur complement", std::to_string(B) + " instances x 256 doubles"))) return rc;
  if ((rc = grow(W.yw, (size_t)B * 16, "the border unknowns", std::to_string(B) + " instances x 16 doubles"))) return rc;
  if ((rc = grow(W.v0, (size_t)B * (size_t)N, "K^-1 r", std::to_string(B) + " instances x " + std::to_string(N) + " doubles"))) return rc;
  if ((rc = grow(W.csym, (size_t)B * 256, "the symmetric part of C", std::to_string(B) + " instances x 256 doubles"))) return rc;
  if ((rc = grow(W.tpart, (size_t)B * (size_t)chunks * 16, "the partial products of G v",
                 std::to_string(B) + " instances x " + std::to_string(chunks) + " chunks x 16 doubles"))) return rc;
  if (const hipError_t e = W.iw.grow((size_t)B * 18); e != hipSuccess)
    return hip_fail(e, ("dto_kkt_border_factor: hipMalloc of pivots and flags (" + std::to_string((size_t)B * 18 * sizeof(int)) + " bytes)").c_str());
  P.B = B; P.chunk = chunk; P.chunks = chunks; P.n_c = n_c;
  return DTO_OK;
}
static int border_finish(dto_problem* h, Problem* p, const BorderPlan& P, int64_t nb, const double* c, int64_t ldc, int32_t* schur_negdef,
                         int32_t* schur_singular, double* skeep, hipStream_t st) {
  KktBorder& W = *p->kkt_border;
  const int64_t Nz = p->L.Nz, Nc = kkt_rows(p), N = Nz + Nc, B = P.B;
  int rc;
  if ((rc = dto_kkt_solve_multi(h, nb, W.g, N, W.g + Nz, N, W.y, N, W.y + Nz, N, (void*)st))) return rc;
  int* piv = W.iw;
  int* flags = W.iw + (size_t)B * 16;
  hipLaunchKernelGGL(k_border_gram, dim3((unsigned)(B * P.chunks)), dim3(KB_THREADS), 0, st, (int)nb, Nz, P.n_c, P.chunk, P.chunks,
                     (const double*)W.g, N, (const double*)(W.g + Nz), N, (const double*)W.y, N, (const double*)(W.y + Nz), N, W.part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_border_schur, dim3((unsigned)B), dim3(64), 0, st, B, (int)nb, P.chunks, (const double*)W.part, c, ldc, W.lu, piv, flags,
                     (double*)W.csym, skeep);
  HIP_TRY(hipGetLastError());
  // the panel and c have been consumed when this returns (and the flags are there)
  std::vector<int> fl(2 * (size_t)B);
  if (schur_negdef || schur_singular) HIP_TRY(hipMemcpyAsync(fl.data(), flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int64_t i = 0; i < B; ++i) {
    if (schur_negdef) schur_negdef[i] = fl[(size_t)i];
    if (schur_singular) schur_singular[i] = fl[(size_t)(B + i)];
  }
  W.nb = (int)nb; W.B = B;
  W.chunk = P.chunk; W.chunks = P.chunks; W.n_c = P.n_c;
  W.valid = true;
  return DTO_OK;
}
// eigenvalue signs of a small symmetric matrix A (n x n, n <= 16, row stride 16) by cyclic Jacobi: the number of negative
// eigenvalues; tiny = one of them is within 1e-13 of the largest entry of zero (the rule of the CPU port's limited-memory mode)
static int small_inertia(const double* A, int n, bool& tiny) {
  double M[16][16];
  double scale = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) { M[i][j] = A[i * 16 + j]; scale = std::max(scale, std::fabs(M[i][j])); }
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) off += M[i][j] * M[i][j];
    if (off <= 1e-30 * scale * scale) break;
    for (int a = 0; a < n; ++a)
      for (int q = a + 1; q < n; ++q) {
        if (std::fabs(M[a][q]) < 1e-300) continue;
        const double th = (M[q][q] - M[a][a]) / (2.0 * M[a][q]);
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0)), c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < n; ++k) { const double u = M[k][a], v = M[k][q]; M[k][a] = c * u - sn * v; M[k][q] = sn * u + c * v; }
        for (int k = 0; k < n; ++k) { const double u = M[a][k], v = M[q][k]; M[a][k] = c * u - sn * v; M[q][k] = sn * u + c * v; }
      }
  }
  int neg = 0;
  tiny = false;
  for (int i = 0; i < n; ++i) { if (M[i][i] < 0.0) ++neg; if (!(std::fabs(M[i][i]) > 1e-13 * scale)) tiny = true; }
  return neg;
}

}  // namespace dto

using dto::Problem;
using dto::set_error;
using dto::SolverState;
using dto::ImState;

extern "C" {

int dto_options_default(dto_options* o) {
  if (!o) return set_error(DTO_ERR_INVALID, "null argument");
  o->tol = 1e-6; o->s_max = 100.0; o->max_iter = 1000;
  o->dual_inf_tol = 1.0; o->constr_viol_tol = 1e-3; o->compl_inf_tol = 1e-3;
  o->mu_init = 0.1; o->delta_c = 1e-8; o->delta_w_init = 1e-4; o->check_every = 10;
  o->max_cpu_time = 300.0;
  o->acceptable_tol = 1e-6; o->acceptable_iter = 15; o->acceptable_dual_inf_tol = 1e10; o->acceptable_constr_viol_tol = 1e-2;
  o->acceptable_compl_inf_tol = 1e-2; o->acceptable_obj_change_tol = 1e-5;
  o->diverging_iterates_tol = 1e8; o->mu_target = 1e-4;
  o->line_search = DTO_LS_PENALTY_FILTER; o->penalty_switch_theta = 1.0;
  o->hessian_approximation = DTO_HESSIAN_EXACT;
  o->kkt_refinement = 0;
  return DTO_OK;
}

int dto_kkt_step_batch(dto_problem* h, const dto_batch* b, const double* mu, int64_t ldmu, double delta_w,
                       double delta_c, double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* inertia_ok) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !b || !b->x || !mu || !dx || !dmu) return set_error(DTO_ERR_INVALID, "null argument");
  if (b->ldx < p->L.Nz || ldmu < p->L.Nc || lddx < p->L.Nz || lddmu < p->L.Nc) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if (p->vt->launch_wide && p->L.Ngen == 0) {
    return dto::wide_step(p, b, mu, ldmu, delta_w, delta_c, dx, lddx, dmu, lddmu, inertia_ok);
  }
  // GeneralConstraint rows coupling several knots: bordered system, Schur complement on the border (on the tile path: the stored
  // factor, the panel substitution and one bordered solve)
  if (p->L.Ngen > 0) {
    std::vector<double> dwv((size_t)b->B, delta_w);
    std::vector<int> okv((size_t)b->B, 1);
    int rcg = dto::bordered_step(p, b, mu, ldmu, dwv.data(), delta_c, dx, lddx, dmu, lddmu, okv.data(), nullptr);
    if (rcg) return rcg;
    if (inertia_ok) { *inertia_ok = 1; for (int v : okv) if (!v) *inertia_ok = 0; }
    return DTO_OK;
  }
  int rc = dto::ensure_state(p, b->B);
  if (rc) return rc;
  p->im_active = false;   // the Newton-KKT entry points live on the SoA engine
  SolverState& S = *p->solver;
  if ((rc = dto::set_batch_params(p, b, (hipStream_t)b->stream))) return rc;
  dto_options u;
  dto_options_default(&u);
  u.delta_c = delta_c;
  dto::default_opts(S.opt, u);
  S.opt.newton_only = 1;
  S.opt.fixed_delta_w = delta_w;
  S.use_sigx = S.use_sigc = S.assembled = false;
  dto::reset_slot_map(S);
  hipStream_t st = (hipStream_t)b->stream;
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  if ((rc = dto::pack(p, a, 0, b->x, b->ldx, st))) return rc;
  if ((rc = dto::pack(p, a, 1, mu, ldmu, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_INIT, a, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_EVAL, a, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_CONV, a, st))) return rc;
  // CONV may flag "converged"/"failed" for this artificial point; the step is wanted regardless
  // (only the lanes that hold an instance: the tail of the last tile stays "no instance")
  for (int g = 0; g < S.G; ++g) {
    const size_t live = (size_t)std::min<int64_t>(64, S.B - (int64_t)g * 64);
    HIP_TRY(hipMemsetAsync(S.scal + ((size_t)g * S.info.nscal + SC_STATUS) * 64, 0, live * sizeof(double), st));
  }
  if ((rc = dto::kkt_launch(p, DTO_KKT_FACTOR_SOLVE, a, st))) return rc;
  if ((rc = dto::unpack(p, a, 2, dx, lddx, st))) return rc;
  if ((rc = dto::unpack(p, a, 3, dmu, lddmu, st))) return rc;
  if (inertia_ok) {
    if ((rc = dto::fetch_scalars(p, st))) return rc;
    *inertia_ok = 1;
    for (int64_t i = 0; i < S.B; ++i)
      if (dto::hscal(S, i, SC_LS_FAIL) != 0.0) *inertia_ok = 0;
  }
  S.begun = false;
  return DTO_OK;
}

// ---- limited-memory mode, small batches: the columns of U as instances of a second state ---------------------------------
// slot s' = s * QN_M2 + c of the column state is a copy of the main state's slot s (iterate, multipliers, bound multipliers,
// slacks, per-instance parameters, stage records, scalars); csrc/dto_kkt_kernels.hpp: k_qn_cols_rhs then subtracts column c.
// Every SoA array is [tile][row][64 lanes] (the records pair-interleaved: position (r >> 1) * 128 + 2 lane + (r & 1)).
namespace dto {
static __global__ __launch_bounds__(64) void k_qn_cols_copy(dto_kkt_args am, dto_kkt_args ac, int ncol, int nblk) {
  const int64_t gc = blockIdx.x / nblk;
  const int blk = blockIdx.x % nblk;
  const int lc = threadIdx.x;
  const int64_t sc_ = gc * 64 + lc, ms = sc_ / ncol;
  const int64_t gm = ms >> 6;
  const int lm = (int)(ms & 63);
  const bool in_range = gm < am.G;
  auto rows = [&](double* dst, const double* src, int64_t n) {
    if (!dst || !src || n == 0 || !in_range) return;
    const int64_t r0 = (n * blk) / nblk, r1 = (n * (blk + 1)) / nblk;
    for (int64_t r = r0; r < r1; ++r) dst[((gc * n + r) << 6) + lc] = src[((gm * n + r) << 6) + lm];
  };
  rows(ac.z, am.z, am.Nz);
  rows(ac.lam, am.lam, am.Nc);
  rows(ac.zl, am.zl, am.Nz);
  rows(ac.zu, am.zu, am.Nz);
  rows(ac.s, am.s, am.Ni);
  rows(ac.zs, am.zs, am.Ni);
  if (am.wtile && ac.wtile) rows(const_cast<double*>(ac.wtile), am.wtile, am.Nw);
  if (in_range) {
    const int64_t n = am.rec_total, r0 = (n * blk) / nblk, r1 = (n * (blk + 1)) / nblk;
    for (int64_t r = r0; r < r1; ++r)
      ac.rec[((gc * n) << 6) + ((r >> 1) << 7) + 2 * lc + (r & 1)] = am.rec[((gm * n) << 6) + ((r >> 1) << 7) + 2 * lm + (r & 1)];
  }
  if (blk == 0) {
    for (int k = 0; k < SC_COUNT; ++k)
      ac.scal[((gc * SC_COUNT + k) << 6) + lc] = in_range ? am.scal[((gm * SC_COUNT + k) << 6) + lm] : (k == SC_STATUS ? DTO_ST_NO_INSTANCE : 0.0);
  }
}
// Z_c := dz_c - v0 back into the main state's history block (what DTO_KKT_QN_COL does for one column at a time)
static __global__ __launch_bounds__(64) void k_qn_cols_gather(dto_kkt_args am, dto_kkt_args ac, int ncol, int nblk) {
  const int64_t gm = blockIdx.x / ((int64_t)ncol * nblk);
  const int rem = (int)(blockIdx.x % ((int64_t)ncol * nblk));
  const int c = rem / nblk, blk = rem % nblk;
  const int lm = threadIdx.x;
  if (am.scal[((gm * SC_COUNT + SC_STATUS) << 6) + lm] != 0.0) return;
  const int64_t sc_ = (gm * 64 + lm) * ncol + c, gc = sc_ >> 6;
  const int lc = (int)(sc_ & 63);
  const QnRows R{am.Nz};
  double* q = am.qn + ((gm * R.total()) << 6) + lm;
  const int64_t n = am.Nz, r0 = (n * blk) / nblk, r1 = (n * (blk + 1)) / nblk;
  for (int64_t r = r0; r < r1; ++r) q[(R.Z(c) + r) << 6] = ac.dz[((gc * n + r) << 6) + lc] - q[(R.v0() + r) << 6];
}
}  // namespace dto

int dto_solver_begin(dto_problem* h, const dto_options* opt, const dto_batch* b) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !b || !b->x) return set_error(DTO_ERR_INVALID, "null argument");
  if (b->ldx < p->L.Nz) return set_error(DTO_ERR_INVALID, "ldx < num_variables");
  if (int rg = dto::wide_general_refused(p, "dto_solver_begin")) return rg;
  if (p->vt->launch_wide) return dto::wide_begin(p, opt, b, false, 0.0);   // tile path: cold start, as dto_solve_batch
  int rc = p->ensure_device();
  if (rc) return rc;
  // no batch is begun until this call has succeeded: a failed set-up must not leave the previous batch (of either engine)
  // marked as running, or a caller that ignores the error would silently advance it
  if (p->solver) p->solver->begun = false;
  if (p->im) p->im->begun = false;
  p->im_active = false;
  if (dto::use_im(p, b->B)) {
    if ((rc = dto::ensure_im_state(p, b->B))) return rc;
    if ((rc = dto::im_begin(p, opt, b, false, 0.0))) return rc;
    p->im_active = true;
    p->hessian_mode_last = DTO_HESSIAN_EXACT;   // the instance-major engine exists for exact-Hessian plugins only
    return DTO_OK;
  }
  rc = dto::ensure_state(p, b->B);
  if (rc) return rc;
  SolverState& S = *p->solver;
  dto::reset_slot_map(S);
  S.use_sigx = S.use_sigc = S.assembled = false;
  if ((rc = dto::set_batch_params(p, b, (hipStream_t)b->stream))) return rc;
  dto_options u;
  if (opt) u = *opt; else dto_options_default(&u);
  S.user = u;
  dto::default_opts(S.opt, u);
  if (S.info.quasi_newton) S.opt.pen_gn = 0;   // per-stage SR1 blocks: dropping them for the penalty phase would also restart them
  hipStream_t st = (hipStream_t)b->stream;
  // A plugin generated without Hessians (evaluate_hessian = 0: `emit_model(...; evaluate_hessian = false)` on the Julia side) keeps
  // per-stage SR1 blocks in its records and has no code for the compact L-BFGS border: a limited-memory request runs those blocks
  // (what such a problem ran before ABI 3) instead of failing, and dto_solver_hessian_mode says so
  if (S.opt.qn_lbfgs && S.info.quasi_newton) S.opt.qn_lbfgs = 0;
  p->hessian_mode_last = S.info.quasi_newton ? DTO_HESSIAN_SR1_BLOCKS : (S.opt.qn_lbfgs ? DTO_HESSIAN_LBFGS : DTO_HESSIAN_EXACT);
  if (S.opt.qn_lbfgs) {
    if (p->L.Ngen != 0)
      return set_error(DTO_ERR_UNSUPPORTED, "hessian_approximation = limited-memory: lane-per-instance solver path without GeneralConstraint rows");
    const size_t need = (size_t)S.G * (size_t)dto::QnRows{p->L.Nz}.total() * 64;
    HIP_TRY(S.qn.grow(need));
    HIP_TRY(hipMemsetAsync(S.qn, 0, need * sizeof(double), st));
    // small batches: the QN_M2 column solves of an iteration side by side, as the instances of a second state (12 x the memory of
    // the batch; DTO_QN_COLS=0: one after the other as for large batches)
    const char* ce = getenv("DTO_QN_COLS");   // read at every begin: tests flip it
    const bool cols_on = !ce || atoi(ce) != 0;
    if (cols_on && (int64_t)S.G * 64 * dto::QN_M2 <= 65536) {
      if (!S.cols) S.cols = new dto::SolverState();
      dto::SolverState& C = *S.cols;
      C.forced_P = 0;
      p->solver = &C;
      rc = dto::ensure_state(p, (int64_t)S.G * 64 * dto::QN_M2);
      p->solver = &S;
      if (rc) return rc;
      C.opt = S.opt; C.user = S.user;
      dto::reset_slot_map(C);
      C.use_sigx = C.use_sigc = C.assembled = false;
      C.use_wtile = false;
      if (S.use_wtile) {
        if (!C.wtile) HIP_TRY(C.wtile.alloc_zeroed((size_t)C.G * 64 * (size_t)p->L.Nw));
        C.use_wtile = true;
      }
    } else if (S.cols) {
      delete S.cols; S.cols = nullptr;
    }
  }
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  const size_t lanes = (size_t)S.G * 64;
  // (the arrival counters of the in-launch joins reset themselves; a batch starts from zero whatever happened to the last one)
  if (S.csync) HIP_TRY(hipMemsetAsync(S.csync, 0, (size_t)S.G * 4 * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(S.lam, 0, std::max<size_t>(1, lanes * p->L.Nc) * sizeof(double), st));
  if ((rc = dto::pack(p, a, 0, b->x, b->ldx, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_INIT, a, st))) return rc;
  S.begun = true;
  (void)dto::fused_update_available(p);   // the second iterate buffers are allocated here, not inside the first iteration
  return DTO_OK;
}

int dto_solver_iterate(dto_problem* h, int n, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && p->im_active && p->im && p->im->begun) return dto::im_iterate(p, n, (hipStream_t)stream);
  if (p && p->vt->launch_wide) {
    if (int rg = dto::wide_general_refused(p, "dto_solver_iterate")) return rg;
    if (!p->wide || !p->wide->begun) return set_error(DTO_ERR_INVALID, "dto_solver_begin has not been called");
    return dto::wide_iterate(p, std::max(0, n), (hipStream_t)stream);
  }
  if (!p || !p->solver || !p->solver->begun) return set_error(DTO_ERR_INVALID, "dto_solver_begin has not been called");
  hipStream_t st = (hipStream_t)stream;
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  if (p->solver->G_active > 0) a.G = p->solver->G_active;   // tiles behind hold finished instances only (dto_solver_repack)
  int rc;
  // UPDATE of iteration k and EVAL of iteration k+1 run as one pass (k_update_eval: 36 instead of 49 rows per stage) into
  // the second iterate buffers; an EVEN number of them per call, so that the call ends on the buffers it started on (the
  // tiles behind G_active, finished instances, are not touched and stay valid there)
  SolverState& S = *p->solver;
  const int n_fused = dto::fused_update_available(p) ? ((n - 1) / 2) * 2 : 0;
  const bool qn = S.opt.qn_lbfgs != 0;
  const bool overlap = !qn && dto::overlap_sweeps(p, st);
  static const bool gate = [] { const char* e = getenv("DTO_OVERLAP_GATE"); return !e || atoi(e) != 0; }();
  // (limited-memory mode and per-stage quasi-Newton records rewrite the records themselves: no refinement there)
  const int n_refine = (!qn && !S.info.quasi_newton && S.user.kkt_refinement > 0) ? std::min(S.user.kkt_refinement, 4) : 0;
  if (n_refine > 0 && (rc = dto::ensure_refine_buffers(p, a))) return rc;
  for (int it = 0; it < n; ++it) {
    if (p->trace && p->trace->on && it > 0) ++p->trace->iteration;
    if (it > 0 && it <= n_fused) {
      a.z_next = S.z_alt; a.lam_next = S.lam_alt;
      if ((rc = dto::kkt_launch(p, DTO_KKT_UPDATE_EVAL, a, st))) return rc;
      std::swap(S.z, S.z_alt); std::swap(S.lam, S.lam_alt);
      a.z = S.z; a.lam = S.lam; a.z_next = nullptr; a.lam_next = nullptr;
    } else {
      if ((rc = dto::kkt_launch(p, DTO_KKT_EVAL, a, st))) return rc;
    }
    if (qn && (rc = dto::kkt_launch(p, DTO_KKT_QN_BEGIN, a, st))) return rc;   // secant pair of the last step, history, sigma
    if ((rc = dto::kkt_launch(p, DTO_KKT_CONV, a, st))) return rc;
    auto factor_solve = [&]() -> int {
    if (overlap) {
      // forward sweeps on the caller's stream, early back substitutions on the low-priority one, the rest and the post pass
      // after both have finished
      a.tile_fwd_tag = S.tile_fwd_tag; a.tile_bwd_tag = S.tile_bwd_tag; a.sweep_tag = ++S.sweep_tag;
      a.fwd_started = gate ? S.fwd_started : nullptr;
      if (gate) HIP_TRY(hipMemsetAsync(S.fwd_started, 0, sizeof(int), st));
      HIP_TRY(hipEventRecord(S.ev_fork, st));
      HIP_TRY(hipStreamWaitEvent(S.stream_lo, S.ev_fork, 0));
      if ((rc = dto::kkt_launch(p, DTO_KKT_FWD, a, st))) return rc;
      if (gate && (rc = dto::kkt_launch(p, DTO_KKT_BWD_GATE, a, S.stream_lo))) return rc;
      // (DTO_OVERLAP_PASSES: further passes for the tiles whose block came too early; measured: 1, 3 and 8 passes give the
      // same 202 ms per iteration at 524 288 instances against 205 without the second stream)
      {
        static const int passes = [] { const char* e = getenv("DTO_OVERLAP_PASSES"); return e ? atoi(e) : 1; }();
        for (int k = 0; k < passes; ++k)
          if ((rc = dto::kkt_launch(p, DTO_KKT_BWD_EARLY, a, S.stream_lo))) return rc;
      }
      HIP_TRY(hipEventRecord(S.ev_join, S.stream_lo));
      HIP_TRY(hipStreamWaitEvent(st, S.ev_join, 0));
      if ((rc = dto::kkt_launch(p, DTO_KKT_BWD_REST, a, st))) return rc;
      if ((rc = dto::kkt_launch(p, DTO_KKT_POST, a, st))) return rc;
      a.tile_fwd_tag = a.tile_bwd_tag = nullptr; a.fwd_started = nullptr;
    } else {
      if ((rc = dto::kkt_launch(p, DTO_KKT_FACTOR_SOLVE, a, st))) return rc;
    }
    return DTO_OK;
    };
    if ((rc = factor_solve())) return rc;
    // iterative refinement (dto_options.kkt_refinement passes; csrc/dto_kkt_kernels.hpp: "iterative refinement")
    for (int r = 0; r < n_refine; ++r)
      if ((rc = dto::refine_pass(p, a, st, factor_solve))) return rc;
    if (qn) {
      // limited-memory BFGS (csrc/dto_kkt_kernels.hpp): the step above is v0 = K0^-1 b; one solve per column of U = [sigma S, Y],
      // the 12 x 12 system per instance, and the corrected step as one more solve (its step-length limits come with it)
      a.qn_col = -1;
      if ((rc = dto::kkt_launch(p, DTO_KKT_QN_COL, a, st))) return rc;
      if (S.cols) {
        // all columns at once: copy every running slot QN_M2 times into the column state, subtract the columns, ONE factor + solve
        // of that state (its own chunk count: it is a batch of 12 x the slots), take the Z_c back
        dto::SolverState& C = *S.cols;
        dto_kkt_args ac;
        p->solver = &C;
        dto::fill_kkt_args(p, ac);
        p->solver = &S;
        ac.qn_main = S.qn;
        ac.opt = a.opt;            // (a warm re-begin may have changed the options of the batch: the columns follow)
        const int nblk = 16;
        hipLaunchKernelGGL(dto::k_qn_cols_copy, dim3((unsigned)((int64_t)C.G * nblk)), dim3(64), 0, st, a, ac, (int)dto::QN_M2, nblk);
        HIP_TRY(hipGetLastError());
        if ((rc = dto::kkt_launch(p, DTO_KKT_QN_COLS_RHS, ac, st))) return rc;
        if ((rc = dto::kkt_launch(p, DTO_KKT_FACTOR_SOLVE, ac, st))) return rc;
        hipLaunchKernelGGL(dto::k_qn_cols_gather, dim3((unsigned)((int64_t)a.G * dto::QN_M2 * nblk)), dim3(64), 0, st, a, ac, (int)dto::QN_M2, nblk);
        HIP_TRY(hipGetLastError());
      } else {
        for (int col = 0; col < dto::QN_M2; ++col) {
          a.qn_mode = 0; a.qn_col = col;
          if ((rc = dto::kkt_launch(p, DTO_KKT_QN_RHS, a, st))) return rc;
          if ((rc = dto::kkt_launch(p, DTO_KKT_FACTOR_SOLVE, a, st))) return rc;
          if ((rc = dto::kkt_launch(p, DTO_KKT_QN_COL, a, st))) return rc;
        }
      }
      if ((rc = dto::kkt_launch(p, DTO_KKT_QN_SMALL, a, st))) return rc;
      a.qn_mode = 1;
      if ((rc = dto::kkt_launch(p, DTO_KKT_QN_RHS, a, st))) return rc;
      if ((rc = dto::kkt_launch(p, DTO_KKT_FACTOR_SOLVE, a, st))) return rc;
      a.qn_mode = 2;
      if ((rc = dto::kkt_launch(p, DTO_KKT_QN_RHS, a, st))) return rc;
      a.qn_mode = 0; a.qn_col = 0;
    }
    if ((rc = dto::kkt_launch(p, DTO_KKT_LINESEARCH, a, st))) return rc;
    if ((rc = dto::kkt_launch(p, DTO_KKT_LS_REDUCE, a, st))) return rc;
    if (qn && (rc = dto::kkt_launch(p, DTO_KKT_QN_SAVE, a, st))) return rc;
    if (!(it + 1 < n && it + 1 <= n_fused))
      if ((rc = dto::kkt_launch(p, DTO_KKT_UPDATE, a, st))) return rc;
  }
  if (p->trace && p->trace->on) ++p->trace->iteration;   // the next call starts a new iteration
  return DTO_OK;
}

int dto_solver_hessian_mode(dto_problem* h, int* mode) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !mode) return set_error(DTO_ERR_INVALID, "null argument");
  *mode = p->hessian_mode_last;
  return DTO_OK;
}

int dto_solver_trace(dto_problem* h, int on) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  if (p->vt->launch_wide) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_trace: the tile path has no launch trace");
  if (!p->trace) p->trace = new dto::LaunchTrace();
  if (on) p->trace->clear();
  p->trace->on = on != 0;
  return DTO_OK;
}

int dto_solver_trace_read(dto_problem* h, int32_t* op, int32_t* iteration, double* start_ms, double* duration_ms, int64_t capacity,
                          int64_t* count) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !count) return set_error(DTO_ERR_INVALID, "null argument");
  *count = 0;
  if (!p->trace) return DTO_OK;
  dto::LaunchTrace& T = *p->trace;
  *count = (int64_t)T.recs.size();
  if (T.recs.empty() || capacity <= 0) return DTO_OK;
  HIP_TRY(hipDeviceSynchronize());
  const hipEvent_t origin = T.pool[(size_t)T.recs[0].e0];
  const int64_t n = std::min<int64_t>(capacity, (int64_t)T.recs.size());
  for (int64_t i = 0; i < n; ++i) {
    const dto::LaunchTrace::Rec& r = T.recs[(size_t)i];
    float t0 = 0.f, dt = 0.f;
    HIP_TRY(hipEventElapsedTime(&t0, origin, T.pool[(size_t)r.e0]));
    HIP_TRY(hipEventElapsedTime(&dt, T.pool[(size_t)r.e0], T.pool[(size_t)r.e1]));
    if (op) op[i] = r.op;
    if (iteration) iteration[i] = r.iteration;
    if (start_ms) start_ms[i] = (double)t0;
    if (duration_ms) duration_ms[i] = (double)dt;
  }
  return DTO_OK;
}

int dto_solver_stats(dto_problem* h, int32_t* status, int32_t* iterations, double* objective, double* constr_viol,
                     double* dual_inf, double* mu, double* delta_w, double* alpha) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && p->im_active && p->im && p->im->A) {
    ImState& I = *p->im;
    HIP_TRY(hipDeviceSynchronize());
    int rc = dto::im_fetch_scalars(p, p->stream);
    if (rc) return rc;
    for (int64_t i = 0; i < I.B; ++i) {
      if (status) status[i] = (int32_t)dto::im_hscal(I, i, SC_STATUS);
      if (iterations) iterations[i] = (int32_t)dto::im_hscal(I, i, SC_ITER);
      if (objective) objective[i] = dto::im_hscal(I, i, SC_F);
      if (constr_viol) constr_viol[i] = dto::im_hscal(I, i, SC_THETA_INF);
      if (dual_inf) dual_inf[i] = dto::im_hscal(I, i, SC_DINF);
      if (mu) mu[i] = dto::im_hscal(I, i, SC_MU);
      if (delta_w) delta_w[i] = dto::im_hscal(I, i, SC_DELTA_W);
      if (alpha) alpha[i] = dto::im_hscal(I, i, SC_ALPHA);
    }
    return DTO_OK;
  }
  if (p && p->vt->launch_wide) {
    if (!p->wide || p->wide->I.empty()) return set_error(DTO_ERR_INVALID, "no solver state");
    const dto::WideState& W = *p->wide;
    for (int64_t i = 0; i < W.B; ++i) {
      const dto::WideInst& s = W.I[(size_t)i];
      if (status) status[i] = s.status;
      if (iterations) iterations[i] = s.iter;
      if (objective) objective[i] = s.f;
      if (constr_viol) constr_viol[i] = s.thinf;
      if (dual_inf) dual_inf[i] = s.dinf;
      if (mu) mu[i] = s.mu;
      if (delta_w) delta_w[i] = s.dw;
      if (alpha) alpha[i] = s.alpha;
    }
    return DTO_OK;
  }
  if (!p || !p->solver || !p->solver->z) return set_error(DTO_ERR_INVALID, "no solver state");
  SolverState& S = *p->solver;
  HIP_TRY(hipDeviceSynchronize());
  int rc = dto::fetch_scalars(p, p->stream);
  if (rc) return rc;
  for (int64_t i = 0; i < S.B; ++i) {
    if (status) status[i] = (int32_t)dto::hscal(S, i, SC_STATUS);
    if (iterations) iterations[i] = (int32_t)dto::hscal(S, i, SC_ITER);
    if (objective) objective[i] = dto::hscal(S, i, SC_F);
    if (constr_viol) constr_viol[i] = dto::hscal(S, i, SC_THETA_INF);
    if (dual_inf) dual_inf[i] = dto::hscal(S, i, SC_DINF);
    if (mu) mu[i] = dto::hscal(S, i, SC_MU);
    if (delta_w) delta_w[i] = dto::hscal(S, i, SC_DELTA_W);
    if (alpha) alpha[i] = dto::hscal(S, i, SC_ALPHA);
  }
  return DTO_OK;
}

int dto_solver_launch_op(dto_problem* h, int op, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && p->im_active && p->im && p->im->begun) {
    // instance-major engine: op = 100 + enum dto_im_op, launched on the list its last pass built for it (diagnostic: timing)
    ImState& I = *p->im;
    const int iop = op - 100;
    if (iop < DTO_IM_EVAL || iop > DTO_IM_UPDATE) return set_error(DTO_ERR_INVALID, "op out of range (instance-major engine: 100 + dto_im_op)");
    dto_im_args a;
    dto::fill_im_args(p, a);
    const int k = (iop == DTO_IM_EVAL || iop == DTO_IM_CONV) ? 0 : (iop == DTO_IM_FWD ? 1 : 2);
    a.list = I.lists + (size_t)k * I.B; a.count = I.ctr + k;
    a.ticket = I.ctr + (iop == DTO_IM_BWD ? 4 : 3);
    HIP_TRY(hipMemsetAsync(I.ctr + 3, 0, 2 * sizeof(int), (hipStream_t)stream));
    return dto::im_launch(p, iop, a, (hipStream_t)stream);
  }
  if (p && p->vt->launch_wide) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_launch_op: the tile path has no per-kernel iteration ops");
  if (!p || !p->solver || !p->solver->begun) return set_error(DTO_ERR_INVALID, "dto_solver_begin has not been called");
  if (op < DTO_KKT_EVAL || op >= DTO_KKT_OP_COUNT) return set_error(DTO_ERR_INVALID, "op out of range");
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  if (p->solver->G_active > 0) a.G = p->solver->G_active;
  if (op == DTO_KKT_UPDATE_EVAL) {
    // the fused pass writes the updated iterate into the second buffers and the pairs are swapped: a caller that replays an
    // iteration kernel by kernel uses it an even number of times between two calls that touch finished tiles (repack, end)
    SolverState& S = *p->solver;
    if (!dto::fused_update_available(p)) return set_error(DTO_ERR_UNSUPPORTED, "the fused UPDATE+EVAL pass is not available (memory, DTO_FUSE_UPDATE=0)");
    a.z_next = S.z_alt; a.lam_next = S.lam_alt;
    const int rc = dto::kkt_launch(p, op, a, (hipStream_t)stream);
    if (rc) return rc;
    std::swap(S.z, S.z_alt); std::swap(S.lam, S.lam_alt);
    return DTO_OK;
  }
  if (op == DTO_KKT_REFINE) {
    // one whole pass, as dto_solver_iterate runs it after FACTOR_SOLVE (here with the plain, non-overlapped factor + solve)
    SolverState& S = *p->solver;
    if (S.info.quasi_newton || S.opt.qn_lbfgs) return set_error(DTO_ERR_UNSUPPORTED, "iterative refinement: exact-Hessian plugins, not in limited-memory mode");
    int rc = dto::ensure_refine_buffers(p, a);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dto::refine_pass(p, a, st, [&]() { return dto::kkt_launch(p, DTO_KKT_FACTOR_SOLVE, a, st); });
  }
  if (op == DTO_KKT_REFINE_APPLY) return set_error(DTO_ERR_INVALID, "DTO_KKT_REFINE_APPLY is part of DTO_KKT_REFINE");
  return dto::kkt_launch(p, op, a, (hipStream_t)stream);
}

int dto_solver_set_partitions(dto_problem* h, int partitions) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || partitions < 0 || partitions > 64) return set_error(DTO_ERR_INVALID, "partitions must be in [0, 64]");
  if (p->vt->launch_wide) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_set_partitions: the tile path factorises every instance in one workgroup");
  if (partitions > p->L.T) return set_error(DTO_ERR_INVALID, "more partitions than stages");
  if (!p->solver) p->solver = new SolverState();
  p->solver->forced_P = partitions;
  return DTO_OK;
}

// ---- receding horizon: shift the device-resident iterate by whole knots -------------------------------------------------
// instance-major work buffers: v[b][n], stage-major with a uniform stride per knot; out[b][..] = shifted copy
static __global__ void k_shift_knots(const double* in, double* out, int64_t ld, int T_blocks, int stride, int last_len, int k) {
  // block t of `out` = block min(t + k, last full block) of `in`; the trailing short block (x_T without an action: last_len
  // entries, 0 = none) takes the head of block min(T_blocks + k, ...) -- i.e. the final state is held
  const int64_t b = blockIdx.y;
  const int t = blockIdx.x;                      // 0 .. T_blocks (the last index addresses the short block)
  const int i = threadIdx.x;
  const double* src = in + b * ld;
  double* dst = out + b * ld;
  if (t < T_blocks) {
    const int ts = t + k < T_blocks ? t + k : T_blocks - 1;
    if (i < stride) {
      // states of a block beyond the horizon: the final state (head of the short block) is held, the action repeats
      double v = src[(int64_t)ts * stride + i];
      if (t + k >= T_blocks && i < last_len) v = src[(int64_t)T_blocks * stride + i];
      dst[(int64_t)t * stride + i] = v;
    }
  } else if (i < last_len) {
    dst[(int64_t)T_blocks * stride + i] = src[(int64_t)T_blocks * stride + i];
  }
}

int dto_solver_shift(dto_problem* h, int knots, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || knots < 0) return set_error(DTO_ERR_INVALID, "bad arguments");
  if (int rg = dto::wide_general_refused(p, "dto_solver_shift")) return rg;
  if (p->vt->launch_wide) return dto::wide_shift(p, knots, (hipStream_t)stream);
  if (p->im_active) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_shift: SoA engine only");
  if (!p->solver || !p->solver->z) return set_error(DTO_ERR_INVALID, "dto_solver_shift needs the device state of a previous solve");
  if (knots == 0) return DTO_OK;
  SolverState& S = *p->solver;
  const dto::Layout& L = p->L;
  const int T = L.T;
  if (knots >= T - 1) return set_error(DTO_ERR_INVALID, "shift by fewer knots than the horizon has");
  for (int t = 1; t < T; ++t)
    if (L.nx[t] != L.nx[0] || (t < T - 1 && L.nu[t] != L.nu[0]))
      return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_shift needs the same state / action dimensions at every knot");
  const int nx = L.nx[0], nu = L.nu[0];
  if (L.Ndyn != (int64_t)(T - 1) * nx) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_shift: unexpected dynamics row count");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = S.B, Nz = L.Nz, Nc = L.Nc;
  dto::DevBuf<double> a, b;
  const size_t n = (size_t)B * (size_t)std::max<int64_t>(Nz, Nc);
  HIP_TRY(a.alloc(n));
  if (b.alloc(n) != hipSuccess) return set_error(DTO_ERR_DEVICE, "hipMalloc");
  dto_kkt_args ka;
  dto::fill_kkt_args(p, ka);
  int rc = DTO_OK;
  auto shift = [&](int which, int64_t ld, int blocks, int stride, int last_len) -> int {
    int r;
    if ((r = dto::unpack(p, ka, which, a, ld, st))) return r;
    HIP_TRY(hipMemcpyAsync(b, a, (size_t)B * ld * sizeof(double), hipMemcpyDeviceToDevice, st));   // rows beyond the shifted part (stage rows of the multipliers) stay
    hipLaunchKernelGGL(k_shift_knots, dim3((unsigned)(blocks + 1), (unsigned)B), dim3(64), 0, st, (const double*)a, b, ld, blocks,
                       stride, last_len, knots);
    HIP_TRY(hipGetLastError());
    return dto::pack(p, ka, which, b, ld, st);
  };
  if (B > 65535 || nx + nu > 64) rc = set_error(DTO_ERR_UNSUPPORTED, "dto_solver_shift: at most 65535 instances and 64 variables per knot");
  // primal iterate: T - 1 blocks [x_t; u_t] and the final state
  if (!rc) rc = shift(0, Nz, T - 1, nx + nu, nx);
  // dynamics multipliers: T - 1 blocks of nx rows (the stage-constraint multipliers behind them belong to their knots: kept)
  if (!rc && Nc > 0) rc = shift(1, Nc, T - 1, nx, 0);
  // bound multipliers follow their variables
  if (!rc && S.zl) { rc = shift(5, Nz, T - 1, nx + nu, nx); if (!rc) rc = shift(6, Nz, T - 1, nx + nu, nx); }
  const hipError_t e = hipStreamSynchronize(st);   // a and b are dropped at the return: the launches above must have finished
  if (rc) return rc;
  if (e != hipSuccess) return dto::hip_fail(e, "dto_solver_shift");
  return DTO_OK;
}

int dto_solver_shift_keep_rows(dto_problem* h, const int32_t* keep, int64_t n) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  if (!keep) {
    p->d_shift_keep.reset();
    return DTO_OK;
  }
  if (n != p->L.Nc) return set_error(DTO_ERR_INVALID, "dto_solver_shift_keep_rows: one flag per constraint row");
  if (n == 0) return DTO_OK;
  int rc = p->ensure_device();
  if (rc) return rc;
  if (!p->d_shift_keep) HIP_TRY(p->d_shift_keep.alloc((size_t)n));
  HIP_TRY(hipMemcpy(p->d_shift_keep, keep, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  return DTO_OK;
}

int dto_solver_set_bounds(dto_problem* h, int64_t B, const double* lower, int64_t ldl, const double* upper, int64_t ldu,
                          void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  if (!p->vt->launch_wide)
    return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_set_bounds: per-instance variable bounds are a tile-path (17..64-state) feature; on "
                                          "the lane-per-instance path per-instance values enter through parameters in stage rows");
  if (int rg = dto::wide_general_refused(p, "dto_solver_set_bounds")) return rg;
  if (!lower && !upper) {
    p->d_bnd.reset(); p->bnd_B = 0;
    return DTO_OK;
  }
  const dto::Layout& L = p->L;
  const int64_t Nz = L.Nz;
  if (!lower || !upper) return set_error(DTO_ERR_INVALID, "dto_solver_set_bounds: lower and upper are both NULL or both set");
  if (B < 1 || Nz < 1) return set_error(DTO_ERR_INVALID, "dto_solver_set_bounds: B >= 1 instances of num_variables >= 1 entries");
  if (ldl < Nz || ldu < Nz) return set_error(DTO_ERR_INVALID, "dto_solver_set_bounds: ldl / ldu < num_variables");
  const int64_t total = B * Nz, blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_set_bounds: batch too large");
  int rc = p->ensure_device();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the new bounds go to a buffer of their own: a violation leaves the previous setting in force
  // (the temporaries are dropped at the return: every path that launched something has waited for the stream by then)
  dto::DevBuf<double> buf, shared;
  dto::DevBuf<unsigned long long> res;
  hipError_t e = buf.alloc((size_t)2 * total);
  if (e == hipSuccess) e = shared.alloc((size_t)2 * Nz);
  if (e == hipSuccess) e = res.alloc(2);
  const unsigned long long init[2] = {0ull, ~0ull};
  unsigned long long out[2] = {0ull, 0ull};
  if (e == hipSuccess) e = hipMemcpy2DAsync(buf, Nz * sizeof(double), lower, ldl * sizeof(double), Nz * sizeof(double), B, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpy2DAsync(buf + total, Nz * sizeof(double), upper, ldu * sizeof(double), Nz * sizeof(double), B, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(shared, L.var_lo.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(shared + Nz, L.var_hi.data(), Nz * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(res, init, sizeof(init), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(dto::k_wide_check_bounds, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)buf, (const double*)(buf + total),
                       (const double*)shared, (const double*)(shared + Nz), Nz, total, res);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, res, sizeof(out), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  double lh[2] = {0.0, 0.0};
  if (e == hipSuccess && out[0] > 0) {
    e = hipMemcpy(&lh[0], buf + out[1], sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&lh[1], buf + total + out[1], sizeof(double), hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return dto::hip_fail(e, "dto_solver_set_bounds");
  if (out[0] > 0) {
    const int64_t b = (int64_t)(out[1] / (unsigned long long)Nz), j = (int64_t)(out[1] % (unsigned long long)Nz);
    const double l = lh[0], u = lh[1], sl = L.var_lo[(size_t)j], su = L.var_hi[(size_t)j];
    const char* why = (l != l || u != u) ? "NaN"
                      : (sl == su && l != u) ? "not fixed (lower != upper) where the problem's variable is fixed"
                      : (sl != su && l == u) ? "fixed (lower == upper) where the problem's variable is not"
                      : (std::isfinite(l) != std::isfinite(sl)) ? (std::isfinite(l) ? "finite lower bound where the problem's is infinite"
                                                                                     : "infinite lower bound where the problem's is finite")
                      : (std::isfinite(u) != std::isfinite(su)) ? (std::isfinite(u) ? "finite upper bound where the problem's is infinite"
                                                                                     : "infinite upper bound where the problem's is finite")
                      : "lower >= upper";
    char msg[384];
    snprintf(msg, sizeof(msg), "dto_solver_set_bounds: instance %lld, variable %lld: %s (lower %.17g, upper %.17g; the problem's %.17g, %.17g); "
             "%llu entries break the problem's bound pattern", (long long)b, (long long)j, why, l, u, sl, su, out[0]);
    return set_error(DTO_ERR_INVALID, msg);
  }
  p->d_bnd = std::move(buf); p->bnd_B = B;
  return DTO_OK;
}

int dto_solver_release(dto_problem* h) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  const int forced = p->solver ? p->solver->forced_P : 0;
  p->free_solver();
  p->im_active = false;
  if (forced > 0) {   // the partition request outlives the state it was stored with
    p->solver = new SolverState();
    p->solver->forced_P = forced;
  }
  return DTO_OK;
}

int dto_solver_set_engine(dto_problem* h, int engine) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || engine < 0 || engine > 2) return set_error(DTO_ERR_INVALID, "engine must be 0 (automatic), 1 (SoA tiles) or 2 (instance-major)");
  if (p->vt->launch_wide) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_set_engine: the tile path has one engine");
  if (engine == 2 && !dto::im_supported(p))
    return set_error(DTO_ERR_UNSUPPORTED, "the instance-major engine needs an exact-Hessian register-path model without GeneralConstraint");
  p->engine_req = engine;
  return DTO_OK;
}

int dto_solver_engine(dto_problem* h, int* engine) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !engine) return set_error(DTO_ERR_INVALID, "null argument");
  *engine = p->im_active ? 2 : 1;
  return DTO_OK;
}

int dto_solver_partitions(dto_problem* h, int* partitions) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !p->solver || !partitions) return set_error(DTO_ERR_INVALID, "no solver state");
  *partitions = p->solver->P;
  return DTO_OK;
}

int dto_solver_fused_update(dto_problem* h, int* fused) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !fused) return set_error(DTO_ERR_INVALID, "null argument");
  *fused = (!p->im_active && p->solver && p->solver->begun && dto::fused_update_available(p)) ? 1 : 0;
  return DTO_OK;
}

int dto_solver_footprint(dto_problem* h, int64_t* rec, int64_t* fac, int64_t* ni, int* rounds) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && p->im_active && p->im && p->im->A) {
    if (rec) *rec = p->im->a_total;   // residual records
    if (fac) *fac = p->im->c_total;   // carries
    if (ni) *ni = p->im->Ni;
    if (rounds) *rounds = 1;
    return DTO_OK;
  }
  if (p && p->vt->launch_wide) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_footprint: the tile path keeps no stage records");
  if (!p || !p->solver || !p->solver->z) return set_error(DTO_ERR_INVALID, "no solver state");
  if (rec) *rec = p->solver->rec_total;
  if (fac) *fac = p->solver->fac_total;
  if (ni) *ni = p->solver->Ni;
  // launches of k_kkt_fwd per iteration: the sequential sweep runs several rounds (all, by default) inside one launch
  if (rounds) {
    const int all = p->solver->opt.newton_only ? 1 : p->solver->opt.max_refactor + 1;
    const int per = (p->solver->P == 1) ? (dto::fwd_rounds_per_launch() > 0 ? dto::fwd_rounds_per_launch() : all) : 1;
    *rounds = (all + per - 1) / per;
  }
  return DTO_OK;
}

int dto_solver_scalar(dto_problem* h, int slot, double* out) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && out && p->im_active && p->im && p->im->A) {
    ImState& I = *p->im;
    if (slot < 0 || slot >= I.info.nscal) return set_error(DTO_ERR_INVALID, "slot out of range");
    HIP_TRY(hipDeviceSynchronize());
    int rc = dto::im_fetch_scalars(p, p->stream);
    if (rc) return rc;
    for (int64_t i = 0; i < I.B; ++i) out[i] = dto::im_hscal(I, i, slot);
    return DTO_OK;
  }
  if (p && out && p->vt->launch_wide) {
    if (!p->wide || p->wide->I.empty()) return set_error(DTO_ERR_INVALID, "no solver state");
    if (slot < 0 || slot >= SC_COUNT) return set_error(DTO_ERR_INVALID, "slot out of range");
    const dto::WideState& W = *p->wide;
    for (int64_t i = 0; i < W.B; ++i)
      if (!dto::wide_scalar(W.I[(size_t)i], slot, &out[i]))
        return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_scalar: the tile path keeps status, iter, mu, delta_w, alpha, f, theta_inf, dinf, "
                                              "ls_fail, delta_last, theta_max, theta_min, filter_n, full_streak, acc_count and f_last");
    return DTO_OK;
  }
  if (!p || !p->solver || !p->solver->z || !out) return set_error(DTO_ERR_INVALID, "no solver state");
  SolverState& S = *p->solver;
  if (slot < 0 || slot >= S.info.nscal) return set_error(DTO_ERR_INVALID, "slot out of range");
  HIP_TRY(hipDeviceSynchronize());
  int rc = dto::fetch_scalars(p, p->stream);
  if (rc) return rc;
  for (int64_t i = 0; i < S.B; ++i) out[i] = dto::hscal(S, i, slot);
  return DTO_OK;
}

int dto_solver_peek(dto_problem* h, int which, double* out, int64_t ld, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && out && p->im_active && p->im && p->im->A) {
    if (which < 0 || which > 9 || which == 4) return set_error(DTO_ERR_INVALID, "unknown vector");
    ImState& I = *p->im;
    const int64_t n = (which == 0 || which == 2 || which == 5 || which == 6) ? p->L.Nz : (which == 1 || which == 3) ? p->L.Nc : I.Ni;
    if (ld < n) return set_error(DTO_ERR_INVALID, "leading dimension too small");
    if (n == 0) return DTO_OK;
    if ((which == 5 || which == 6) && !I.Bd) {
      if (hipMemset2DAsync(out, (size_t)ld * sizeof(double), 0, (size_t)n * sizeof(double), (size_t)I.B, (hipStream_t)stream) != hipSuccess)
        return set_error(DTO_ERR_DEVICE, "hipMemset2DAsync");
      return DTO_OK;
    }
    return dto::im_unpack(p, which, out, ld, (hipStream_t)stream);
  }
  if (p && out && p->vt->launch_wide) {
    if (!p->wide || p->wide->I.empty()) return set_error(DTO_ERR_INVALID, "no solver state");
    if (which < 0 || which > 9 || which == 4) return set_error(DTO_ERR_INVALID, "unknown vector");
    if (which > 6) return set_error(DTO_ERR_UNSUPPORTED, "dto_solver_peek: the tile path has no slacks (which = 0, 1, 2, 3, 5, 6)");
    const dto::WideState& W = *p->wide;
    const int64_t n = (which == 0 || which == 2 || which == 5 || which == 6) ? p->L.Nz : p->L.Nc;
    if (ld < n) return set_error(DTO_ERR_INVALID, "leading dimension too small");
    if (n == 0) return DTO_OK;
    const double* src = which == 0 ? W.z : which == 1 ? W.lam : which == 2 ? W.dz : which == 3 ? W.dlam : which == 5 ? W.zl : W.zu;
    if (!src) {   // no finite variable bounds: the bound multipliers are identically zero
      HIP_TRY(hipMemset2DAsync(out, (size_t)ld * sizeof(double), 0, (size_t)n * sizeof(double), (size_t)W.B, (hipStream_t)stream));
      return DTO_OK;
    }
    HIP_TRY(hipMemcpy2DAsync(out, ld * sizeof(double), src, n * sizeof(double), n * sizeof(double), W.B, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    return DTO_OK;
  }
  if (!p || !p->solver || !p->solver->z || !out) return set_error(DTO_ERR_INVALID, "no solver state");
  if (which < 0 || which > 9 || which == 4) return set_error(DTO_ERR_INVALID, "unknown vector");
  SolverState& S = *p->solver;
  const int64_t n = (which == 0 || which == 2 || which == 5 || which == 6) ? p->L.Nz : (which == 1 || which == 3) ? p->L.Nc : S.Ni;
  if (ld < n) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if ((which == 5 || which == 6) && !S.zl) {   // no finite variable bounds: the bound multipliers are identically zero
    if (hipMemset2DAsync(out, (size_t)ld * sizeof(double), 0, (size_t)n * sizeof(double), (size_t)S.B, (hipStream_t)stream) != hipSuccess)
      return set_error(DTO_ERR_DEVICE, "hipMemset2DAsync");
    return DTO_OK;
  }
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  return dto::unpack(p, a, which, out, ld, (hipStream_t)stream);
}

int dto_solver_end(dto_problem* h, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && p->im_active && p->im && p->im->A) {
    int rc;
    if (x_out) {
      if (ldxo < p->L.Nz) return set_error(DTO_ERR_INVALID, "ldxo < num_variables");
      if ((rc = dto::im_unpack(p, 0, x_out, ldxo, (hipStream_t)stream))) return rc;
    }
    if (mu_out && p->L.Nc > 0) {
      if (ldmuo < p->L.Nc) return set_error(DTO_ERR_INVALID, "ldmuo < num_constraint");
      if ((rc = dto::im_unpack(p, 1, mu_out, ldmuo, (hipStream_t)stream))) return rc;
    }
    return DTO_OK;
  }
  if (p && p->vt->launch_wide) {
    if (!p->wide || p->wide->I.empty()) return set_error(DTO_ERR_INVALID, "no solver state");
    return dto::wide_end(p, x_out, ldxo, mu_out, ldmuo, (hipStream_t)stream);
  }
  if (!p || !p->solver || !p->solver->z) return set_error(DTO_ERR_INVALID, "no solver state");
  hipStream_t st = (hipStream_t)stream;
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  int rc;
  if (x_out) {
    if (ldxo < p->L.Nz) return set_error(DTO_ERR_INVALID, "ldxo < num_variables");
    if ((rc = dto::unpack(p, a, 0, x_out, ldxo, st))) return rc;
  }
  if (mu_out) {
    if (ldmuo < p->L.Nc) return set_error(DTO_ERR_INVALID, "ldmuo < num_constraint");
    if ((rc = dto::unpack(p, a, 1, mu_out, ldmuo, st))) return rc;
  }
  return DTO_OK;
}

int dto_solver_run(dto_problem* h, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, int32_t* status,
                   int32_t* iterations, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && p->im_active && p->im && p->im->begun) return dto::im_run(p, x_out, ldxo, mu_out, ldmuo, status, iterations, (hipStream_t)stream);
  if (p && p->vt->launch_wide) {
    if (int rg = dto::wide_general_refused(p, "dto_solver_run")) return rg;
    if (!p->wide || !p->wide->begun) return set_error(DTO_ERR_INVALID, "dto_solver_begin[_warm] has not been called");
    return dto::wide_run(p, x_out, ldxo, mu_out, ldmuo, status, iterations, (hipStream_t)stream);
  }
  if (!p || !p->solver || !p->solver->begun) return set_error(DTO_ERR_INVALID, "dto_solver_begin[_warm] has not been called");
  SolverState& S = *p->solver;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  const int chunk = std::max(1, S.user.check_every);
  int done_iters = 0;
  const auto t_start = std::chrono::steady_clock::now();
  bool timed_out = false;
  // max_iter + 1 evaluations: the last one only classifies the final iterate
  while (done_iters <= S.user.max_iter) {
    const int n = std::min(chunk, S.user.max_iter + 1 - done_iters);
    if ((rc = dto_solver_iterate(h, n, (void*)st))) return rc;
    done_iters += n;
    if ((rc = dto::fetch_scalars(p, st))) return rc;
    int64_t n_run = 0;
    for (int64_t i = 0; i < S.B; ++i) n_run += dto::hscal(S, i, SC_STATUS) == 0.0;
    if (n_run == 0) break;
    // tiles are only worth running while they hold work: close the gaps once a quarter of the active lanes has finished
    if (S.G_active > 1 && n_run < (int64_t)48 * S.G_active && (rc = dto::repack(p, st, nullptr))) return rc;
    // Options.max_cpu_time (src/options.jl:10): the instances still running are handed back as they are (DTO_STATUS_CPU_TIME)
    if (S.user.max_cpu_time > 0.0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > S.user.max_cpu_time) {
      timed_out = true;
      break;
    }
  }
  if ((rc = dto_solver_end(h, x_out, ldxo, mu_out, ldmuo, (void*)st))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  for (int64_t i = 0; i < S.B; ++i) {
    if (status) { status[i] = (int32_t)dto::hscal(S, i, SC_STATUS); if (status[i] == 0 && timed_out) status[i] = DTO_STATUS_CPU_TIME; }
    if (iterations) iterations[i] = (int32_t)dto::hscal(S, i, SC_ITER);
  }
  return DTO_OK;
}

int dto_solver_repack(dto_problem* h, int* num_running, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  // instance-major engine: nothing to move (work lists are rebuilt every pass); only the count is reported
  if (p && p->im_active && p->im && p->im->begun) return dto::im_count(p, (hipStream_t)stream, -1, num_running, nullptr);
  if (p && p->vt->launch_wide) {
    // tile path: nothing to move (the host loop skips finished instances); only the count is reported
    if (!p->wide || !p->wide->begun) return set_error(DTO_ERR_INVALID, "dto_solver_begin[_warm] has not been called");
    int n = 0;
    for (const dto::WideInst& s : p->wide->I) n += s.status == 0 && !p->wide->timed_out;
    if (num_running) *num_running = n;
    return DTO_OK;
  }
  if (!p || !p->solver || !p->solver->begun) return set_error(DTO_ERR_INVALID, "dto_solver_begin[_warm] has not been called");
  int rc = dto::fetch_scalars(p, (hipStream_t)stream);
  if (rc) return rc;
  return dto::repack(p, (hipStream_t)stream, num_running);
}

int dto_solve_batch(dto_problem* h, const dto_options* opt, const dto_batch* b, double* x_out, int64_t ldxo,
                    double* mu_out, int64_t ldmuo, int32_t* status, int32_t* iterations) {
  Problem* p = reinterpret_cast<Problem*>(h);
  // (the stepwise tile solver, the lane path's border and a tile border of more than four general rows have no limited-memory mode:
  //  they run the exact second derivatives of the traced expressions whatever dto_options.hessian_approximation asks for, and dto_solver_hessian_mode
  //  reports it -- ADVICE r5)
  if (p && b && b->x && x_out && p->vt->launch_wide && 2 * dto::QnHistory::M + p->L.Ngen <= dto::KB_MAX && opt &&
      opt->hessian_approximation == DTO_HESSIAN_LBFGS) {
    // tile path, limited-memory mode: the host-driven bordered loop with the compact L-BFGS matrix as its border, beside at most four
    // general rows in the same panel (more of them: the exact substitute below).
    // The stepwise state of the handle (dto_solver_begin ...) is not touched; the factor storage is taken, as by every solve
    int rc = dto::general_solve_batch(p, opt, b, x_out, ldxo, mu_out, ldmuo, status, iterations, true);
    if (rc == DTO_OK) p->hessian_mode_last = DTO_HESSIAN_LBFGS;
    return rc;
  }
  if (p && b && b->x && x_out && p->vt->launch_wide && p->L.Ngen == 0) {
    // tile path: begin + run on the state of the handle, which stays allocated for dto_solver_begin_warm / dto_solver_shift
    int rc = dto::wide_begin(p, opt, b, false, 0.0);
    if (rc) return rc;
    return dto::wide_run(p, x_out, ldxo, mu_out, ldmuo, status, iterations, (hipStream_t)b->stream);
  }
  if (p && b && b->x && x_out && p->L.Ngen > 0) {
    p->hessian_mode_last = DTO_HESSIAN_EXACT;
    return dto::general_solve_batch(p, opt, b, x_out, ldxo, mu_out, ldmuo, status, iterations);
  }
  int rc = dto_solver_begin(h, opt, b);
  if (rc) return rc;
  return dto_solver_run(h, x_out, ldxo, mu_out, ldmuo, status, iterations, b->stream);
}

// the argument checks that dto_solve_batch_warm and dto_point_shift share: x, the leading dimensions, zl / zu together, the history
// whole (host_values: qn_npairs and qn_sigma are read, a start point's)
static int point_check(const dto::Problem* p, const dto_point* pt, int64_t B, const char* who, bool host_values) {
  const int64_t Nz = p->L.Nz, Nc = p->L.Nc;
  const std::string w(who);
  if (!pt->x) return set_error(DTO_ERR_INVALID, w + ": x is NULL");
  if ((pt->zl == nullptr) != (pt->zu == nullptr)) return set_error(DTO_ERR_INVALID, w + ": zl and zu are both NULL or both set");
  const int nq = (pt->qn_s ? 1 : 0) + (pt->qn_y ? 1 : 0) + (pt->qn_npairs ? 1 : 0) + (pt->qn_sigma ? 1 : 0);
  if (nq != 0 && nq != 4) return set_error(DTO_ERR_INVALID, w + ": qn_s, qn_y, qn_npairs and qn_sigma are all NULL or all set");
  if (pt->ldx < Nz || (pt->mu && pt->ldmu < Nc) || (pt->zl && (pt->ldzl < Nz || pt->ldzu < Nz)) || (pt->slack && pt->ldslack < Nc) ||
      (nq && (pt->ldqs < Nz || pt->ldqy < Nz)))
    return set_error(DTO_ERR_INVALID, w + ": leading dimension too small");
  for (int64_t i = 0; host_values && nq && i < B; ++i) {
    if (pt->qn_npairs[i] < 0 || pt->qn_npairs[i] > dto::QnHistory::M) return set_error(DTO_ERR_INVALID, w + ": qn_npairs outside 0..6");
    if (!(pt->qn_sigma[i] > 0.0) || !std::isfinite(pt->qn_sigma[i])) return set_error(DTO_ERR_INVALID, w + ": qn_sigma must be positive and finite");
  }
  return DTO_OK;
}

int dto_solve_batch_warm(dto_problem* h, const dto_options* opt, const dto_batch* b, const dto_point* start, dto_point* end,
                         int32_t* status, int32_t* iterations) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !b || !end) return set_error(DTO_ERR_INVALID, "null argument");
  // exactly the problems dto_solve_batch sends to general_solve_batch
  const bool lbfgs = p->vt->launch_wide && 2 * dto::QnHistory::M + p->L.Ngen <= dto::KB_MAX && opt && opt->hessian_approximation == DTO_HESSIAN_LBFGS;
  if (!lbfgs && p->L.Ngen == 0)
    return set_error(DTO_ERR_UNSUPPORTED, "dto_solve_batch_warm: the bordered loop's problems only (GeneralConstraint rows, or the tile path's limited-memory "
                                          "mode); this problem has warm starts through dto_solver_begin_warm");
  if (b->B < 1) return set_error(DTO_ERR_INVALID, "dto_solve_batch_warm: empty batch");
  int rc;
  if ((rc = point_check(p, end, b->B, "dto_solve_batch_warm, end", false))) return rc;
  if (start && (rc = point_check(p, start, b->B, "dto_solve_batch_warm, start", true))) return rc;
  if (!start && (!b->x || b->ldx < p->L.Nz)) return set_error(DTO_ERR_INVALID, "dto_solve_batch_warm: a cold start needs b->x with ldx >= num_variables");
  rc = dto::general_solve_batch(p, opt, b, end->x, end->ldx, end->mu, end->ldmu, status, iterations, lbfgs, start, end);
  if (rc == DTO_OK) p->hessian_mode_last = lbfgs ? DTO_HESSIAN_LBFGS : DTO_HESSIAN_EXACT;
  return rc;
}

int dto_point_shift(dto_problem* h, int64_t B, dto_point* pt, int knots, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !pt || knots < 0) return set_error(DTO_ERR_INVALID, "bad arguments");
  if (B < 1) return set_error(DTO_ERR_INVALID, "dto_point_shift: empty batch");
  int rc;
  if ((rc = point_check(p, pt, B, "dto_point_shift", false))) return rc;
  const dto::Layout& L = p->L;
  const int T = L.T;
  if (knots >= T - 1) return set_error(DTO_ERR_INVALID, "shift by fewer knots than the horizon has");
  for (int t = 1; t < T; ++t)
    if (L.nx[t] != L.nx[0] || (t < T - 1 && L.nu[t] != L.nu[0]))
      return set_error(DTO_ERR_UNSUPPORTED, "dto_point_shift needs the same state / action dimensions at every knot");
  const int nx = L.nx[0], nu = L.nu[0];
  const int64_t Nz = L.Nz, Nc = L.Nc;
  if (L.Ndyn != (int64_t)(T - 1) * nx || Nz != (int64_t)(T - 1) * (nx + nu) + nx)
    return set_error(DTO_ERR_UNSUPPORTED, "dto_point_shift: unexpected variable / dynamics row count");
  if (knots == 0) return DTO_OK;
  if ((rc = p->ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t M = dto::QnHistory::M;
  const int64_t longest = std::max<int64_t>(B * Nz * (pt->qn_s ? M : 1), pt->mu ? B * Nc : 0);
  if ((longest + 255) / 256 > 0x7fffffff) return set_error(DTO_ERR_UNSUPPORTED, "dto_point_shift: batch too large");
  dto::DevBuf<double> tmp;   // the one scratch buffer: every array goes through it and back, in stream order
  HIP_TRY(tmp.alloc((size_t)longest));
  auto shift = [&](double* a, int64_t ld, int64_t n, int64_t inner, int stride, int last_len, const int* keep) -> int {
    if (!a || n == 0) return DTO_OK;
    const int64_t total = B * inner * n;
    hipLaunchKernelGGL(dto::k_point_shift, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)a, ld, (double*)tmp, n, B, inner, stride,
                       T - 1, last_len, knots, keep);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(a, ld * sizeof(double), tmp, n * sizeof(double), n * sizeof(double), (size_t)(B * inner), hipMemcpyDeviceToDevice, st));
    return DTO_OK;
  };
  rc = shift(pt->x, pt->ldx, Nz, 1, nx + nu, nx, nullptr);
  // dynamics multipliers: T - 1 blocks of n_x rows; the stage and general rows behind them stay, and so do the marked rows
  if (!rc) rc = shift(pt->mu, pt->ldmu, Nc, 1, nx, 0, (const int*)p->d_shift_keep);
  if (!rc) rc = shift(pt->zl, pt->ldzl, Nz, 1, nx + nu, nx, nullptr);
  if (!rc) rc = shift(pt->zu, pt->ldzu, Nz, 1, nx + nu, nx, nullptr);
  if (!rc) rc = shift(pt->qn_s, pt->ldqs, Nz, M, nx + nu, nx, nullptr);
  if (!rc) rc = shift(pt->qn_y, pt->ldqy, Nz, M, nx + nu, nx, nullptr);
  const hipError_t e = hipStreamSynchronize(st);   // tmp is dropped at the return: the launches above must have finished
  if (rc) return rc;
  if (e != hipSuccess) return dto::hip_fail(e, "dto_point_shift");
  return DTO_OK;
}

int dto_solver_begin_warm(dto_problem* h, const dto_options* opt, const dto_batch* b, double mu0) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !b) return set_error(DTO_ERR_INVALID, "null argument");
  if (int rg = dto::wide_general_refused(p, "dto_solver_begin_warm")) return rg;
  if (p->vt->launch_wide) return dto::wide_begin(p, opt, b, true, mu0);
  if (p->im_active && p->im && p->im->A) {
    if (p->im->B != b->B) return set_error(DTO_ERR_INVALID, "dto_solver_begin_warm needs the device state of a previous solve of the same batch size");
    if (b->x && b->ldx < p->L.Nz) return set_error(DTO_ERR_INVALID, "ldx < num_variables");
    return dto::im_begin(p, opt, b, true, mu0);
  }
  if (!p->solver || !p->solver->z || p->solver->B != b->B)
    return set_error(DTO_ERR_INVALID, "dto_solver_begin_warm needs the device state of a previous solve of the same batch size");
  if (b->x && b->ldx < p->L.Nz) return set_error(DTO_ERR_INVALID, "ldx < num_variables");
  SolverState& S = *p->solver;
  int rc;
  if ((rc = dto::set_batch_params(p, b, (hipStream_t)b->stream))) return rc;
  dto_options u;
  if (opt) u = *opt; else dto_options_default(&u);
  S.user = u;
  dto::default_opts(S.opt, u);
  if (S.info.quasi_newton) S.opt.pen_gn = 0;
  if (S.opt.qn_lbfgs && S.info.quasi_newton) S.opt.qn_lbfgs = 0;   // as in dto_solver_begin: such a plugin runs its SR1 blocks
  if (S.opt.qn_lbfgs && !S.qn) return set_error(DTO_ERR_INVALID, "dto_solver_begin_warm: the previous solve did not run in limited-memory mode");
  p->hessian_mode_last = S.info.quasi_newton ? DTO_HESSIAN_SR1_BLOCKS : (S.opt.qn_lbfgs ? DTO_HESSIAN_LBFGS : DTO_HESSIAN_EXACT);
  S.opt.warm = 1;
  S.opt.mu_warm = mu0;
  S.G_active = S.G;   // every instance runs again (the slot map of an earlier dto_solver_repack stays valid)
  dto::set_partitions_now(S, S.P0);
  S.use_sigx = S.use_sigc = S.assembled = false;
  hipStream_t st = (hipStream_t)b->stream;
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  if (b->x && (rc = dto::pack(p, a, 0, b->x, b->ldx, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_INIT, a, st))) return rc;
  S.opt.warm = 0;   // the flag only concerns the initialisation kernel
  S.begun = true;
  (void)dto::fused_update_available(p);
  return DTO_OK;
}

// ---- the linear solver alone ---------------------------------------------------------------------------------------
int dto_kkt_assemble(dto_problem* h, const dto_batch* b, const dto_kkt_system* sys) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !b || !b->x || !sys || !sys->mu) return set_error(DTO_ERR_INVALID, "null argument");
  if (b->ldx < p->L.Nz || sys->ldmu < p->L.Nc) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if ((sys->sigma_x && sys->ldsx < p->L.Nz) || (sys->sigma_c && sys->ldsc < p->L.Nc)) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if (p->vt->launch_wide) return dto::wide_kkt_assemble(p, b, sys);   // tile path: the factor is stored, a solve is substitution only
  // models with GeneralConstraint rows: this is the STAGE part of K (dynamics + stage rows); the border is the caller's
  dto::kkt_border_taken(p);
  int rc = dto::ensure_state(p, b->B, true);
  if (rc) return rc;
  p->im_active = false;
  SolverState& S = *p->solver;
  dto::reset_slot_map(S);
  hipStream_t st = (hipStream_t)b->stream;
  if ((rc = dto::set_batch_params(p, b, st))) return rc;
  dto_options u;
  dto_options_default(&u);
  u.delta_c = sys->delta_c;
  dto::default_opts(S.opt, u);
  S.opt.newton_only = 1;
  S.opt.fixed_delta_w = sys->delta_w;
  const size_t lanes = (size_t)S.G * 64;
  if (sys->sigma_x && !S.sigx) HIP_TRY(S.sigx.alloc_zeroed(lanes * (size_t)p->L.Nz));
  if (sys->sigma_c && !S.sigc) HIP_TRY(S.sigc.alloc_zeroed(lanes * (size_t)std::max<int64_t>(1, p->L.Nc)));
  S.use_sigx = sys->sigma_x != nullptr;
  S.use_sigc = sys->sigma_c != nullptr;
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  if ((rc = dto::pack(p, a, 0, b->x, b->ldx, st))) return rc;
  if ((rc = dto::pack(p, a, 1, sys->mu, sys->ldmu, st))) return rc;
  if (sys->sigma_x && (rc = dto::pack(p, a, 10, sys->sigma_x, sys->ldsx, st))) return rc;
  if (sys->sigma_c && (rc = dto::pack(p, a, 11, sys->sigma_c, sys->ldsc, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_INIT, a, st))) return rc;
  // residuals of this point into the records (a right-hand side must be there for dto_kkt_factor; dto_kkt_solve replaces it)
  if ((rc = dto::kkt_launch(p, DTO_KKT_EVAL, a, st))) return rc;
  S.assembled = true;
  S.begun = false;
  return DTO_OK;
}

int dto_kkt_assemble_first_order(dto_problem* h, const dto_batch* b, const dto_kkt_system* sys) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !b || !b->x || !sys) return set_error(DTO_ERR_INVALID, "null argument");
  if (!p->vt->launch_wide)
    return set_error(DTO_ERR_UNSUPPORTED, "dto_kkt_assemble_first_order: tile path only (the lane-per-instance path keeps no assembled system: "
                                          "its solver runs the limited-memory mode inside its sweeps)");
  if (b->ldx < p->L.Nz) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if ((sys->sigma_x && sys->ldsx < p->L.Nz) || (sys->sigma_c && sys->ldsc < p->L.Nc)) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  return dto::wide_kkt_assemble(p, b, sys, true);
}

int dto_kkt_factor(dto_problem* h, int32_t* inertia_ok, int32_t* num_negative, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (p && p->vt->launch_wide) return dto::wide_kkt_factor(p, inertia_ok, num_negative, (hipStream_t)stream);
  if (!p || !p->solver || !p->solver->assembled) return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  dto::kkt_border_taken(p);
  SolverState& S = *p->solver;
  hipStream_t st = (hipStream_t)stream;
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  int rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_REARM, a, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_FWD, a, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_SEP, a, st))) return rc;
  if (inertia_ok || num_negative) {
    if ((rc = dto::fetch_scalars(p, st))) return rc;
    for (int64_t i = 0; i < S.B; ++i) {
      if (inertia_ok) inertia_ok[i] = dto::hscal(S, i, SC_LS_FAIL) == 0.0 ? 1 : 0;
      if (num_negative) num_negative[i] = (int32_t)dto::hscal(S, i, SC_NNEG);
    }
  }
  return DTO_OK;
}

// The checks of the entry points that take vectors against the assembled system, in the order the callers report them: has
// dto_kkt_assemble been called (on the path of this handle), `bad` (the entry point's own check of nrhs or passes: its message,
// or nullptr), null vectors, leading dimensions.  (in, out): the vectors of the variables and of the constraint rows.
static int check_kkt_vectors(const Problem* p, const char* bad, const double* in_x, int64_t ldix, const double* in_c, int64_t ldic,
                             const double* out_x, int64_t ldox, const double* out_c, int64_t ldoc) {
  if (!p || (p->vt->launch_wide ? !p->wide_kkt || !p->wide_kkt->assembled : !p->solver || !p->solver->assembled))
    return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  if (bad) return set_error(DTO_ERR_INVALID, bad);
  if (!in_x || !out_x || (p->L.Nc > 0 && (!in_c || !out_c))) return set_error(DTO_ERR_INVALID, "null argument");
  if (ldix < p->L.Nz || ldox < p->L.Nz || ldic < p->L.Nc || ldoc < p->L.Nc) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  return DTO_OK;
}

int dto_kkt_solve(dto_problem* h, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc, double* sol_x,
                  int64_t ldsx, double* sol_c, int64_t ldsc, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (int bad = check_kkt_vectors(p, nullptr, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc)) return bad;
  const bool wide = p->vt->launch_wide != nullptr;
  if (wide) return dto::wide_kkt_solve(p, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc, (hipStream_t)stream);
  hipStream_t st = (hipStream_t)stream;
  dto_kkt_args a;
  dto::fill_kkt_args(p, a);
  a.rhs_x = rhs_x; a.ld_rhs_x = ldrx; a.rhs_c = rhs_c; a.ld_rhs_c = ldrc;
  int rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_RHS, a, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_REARM, a, st))) return rc;
  // the factors are not kept between calls (the sweeps recompute a stage's LDL^T instead of storing it):
  // a solve is forward sweep + separator system + backward sweep with the new right-hand side
  if ((rc = dto::kkt_launch(p, DTO_KKT_FWD, a, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_SEP, a, st))) return rc;
  if ((rc = dto::kkt_launch(p, DTO_KKT_BWD, a, st))) return rc;
  if ((rc = dto::unpack(p, a, 2, sol_x, ldsx, st))) return rc;
  if (p->L.Nc > 0 && (rc = dto::unpack(p, a, 3, sol_c, ldsc, st))) return rc;
  return DTO_OK;
}

int dto_kkt_solve_multi(dto_problem* h, int64_t nrhs, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc,
                        double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();   // (allocates the tables of the handle once, launches nothing)
  if (rc) return rc;
  const bool wide = p->vt->launch_wide != nullptr;
  if ((rc = check_kkt_vectors(p, nrhs < 1 ? "nrhs < 1" : nullptr, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc))) return rc;
  if (wide) return dto::wide_kkt_solve_multi(p, nrhs, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc, (hipStream_t)stream);
  // lane-per-instance path: no stored factor, so nrhs passes of the single solve -- right-hand side r of every instance is a
  // batch of its own with the rows nrhs apart
  for (int64_t r = 0; r < nrhs; ++r) {
    rc = dto_kkt_solve(h, rhs_x + r * ldrx, nrhs * ldrx, rhs_c ? rhs_c + r * ldrc : nullptr, nrhs * ldrc, sol_x + r * ldsx, nrhs * ldsx,
                       sol_c ? sol_c + r * ldsc : nullptr, nrhs * ldsc, stream);
    if (rc) return rc;
  }
  return DTO_OK;
}

int dto_kkt_multiply(dto_problem* h, const double* v_x, int64_t ldvx, const double* v_c, int64_t ldvc, double* out_x, int64_t ldox,
                     double* out_c, int64_t ldoc, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();   // (allocates the tables of the handle once, launches nothing)
  if (rc) return rc;
  if (!p->vt->launch_wide)
    return set_error(DTO_ERR_UNSUPPORTED, "dto_kkt_multiply: tile path only (the lane-per-instance path keeps no assembled system: its sweeps "
                                          "rebuild the stage blocks in registers)");
  if ((rc = check_kkt_vectors(p, nullptr, v_x, ldvx, v_c, ldvc, out_x, ldox, out_c, ldoc))) return rc;
  return dto::wide_kkt_multiply(p, v_x, ldvx, v_c, ldvc, out_x, ldox, out_c, ldoc, (hipStream_t)stream);
}

int dto_kkt_solve_refined(dto_problem* h, int passes, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc, double* sol_x,
                          int64_t ldsx, double* sol_c, int64_t ldsc, double* resid, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();
  if (rc) return rc;
  if (!p->vt->launch_wide)
    return set_error(DTO_ERR_UNSUPPORTED, "dto_kkt_solve_refined: tile path only (the lane-per-instance path stores no factor; its solver "
                                          "refines through dto_options.kkt_refinement)");
  if ((rc = check_kkt_vectors(p, passes < 0 || passes > 4 ? "passes outside 0..4" : nullptr, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc)))
    return rc;
  return dto::wide_kkt_solve_refined(p, passes, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc, resid, (hipStream_t)stream);
}

// ---- bordered solves against the factor (dto_border_kernels.hpp): [K G'; G C] [v; y] = [r; s] by the Schur complement on the
//      border.  Y = K^-1 G' and v0 = K^-1 r come from the entry points above -- the panel substitution and the single
//      substitution of the tile path, nb + 1 sweeps of the lane path -- so both paths share everything below.
int dto_kkt_border_factor(dto_problem* h, int64_t nb, const double* g_x, int64_t ldgx, const double* g_c, int64_t ldgc, const double* c,
                          int64_t ldc, int32_t* schur_negdef, int32_t* schur_singular, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();
  if (rc) return rc;
  const bool wide = p->vt->launch_wide != nullptr;
  if (wide ? !p->wide_kkt || !p->wide_kkt->assembled : !p->solver || !p->solver->assembled)
    return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  if (nb < 1) return set_error(DTO_ERR_INVALID, "dto_kkt_border_factor: nb < 1");
  if (nb > dto::KB_MAX) return set_error(DTO_ERR_UNSUPPORTED, "dto_kkt_border_factor: more than 16 border rows (one panel of right-hand sides)");
  // tile path with GeneralConstraint rows: K is the stage part, a row of the panel and of Y has Nz + Ns entries and the tail of
  // g_c is not read
  const int64_t Nz = p->L.Nz, Nc = dto::kkt_rows(p), N = Nz + Nc;
  if (!g_x) return set_error(DTO_ERR_INVALID, "null argument");
  if (ldgx < Nz || (g_c && ldgc < p->L.Nc) || (c && ldc < nb * nb)) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if (wide && !p->wide_kkt->factored)
    return set_error(DTO_ERR_INVALID, "dto_kkt_factor has not been called (or dto_kkt_step_batch / the solver has used the factor storage since)");
  dto::BorderPlan P;
  if ((rc = dto::border_prepare(p, nb, g_c != nullptr, P))) return rc;
  dto::KktBorder& W = *p->kkt_border;
  hipStream_t st = (hipStream_t)stream;
  const size_t rows = (size_t)P.B * (size_t)nb;
  // the panel of right-hand sides: row b * nb + j = [g_x row; g_c row or zeros]
  const size_t pitch = (size_t)N * sizeof(double);
  HIP_TRY(hipMemcpy2DAsync(W.g, pitch, g_x, (size_t)ldgx * sizeof(double), (size_t)Nz * sizeof(double), rows, hipMemcpyDeviceToDevice, st));
  if (Nc > 0) {
    if (g_c) HIP_TRY(hipMemcpy2DAsync(W.g + Nz, pitch, g_c, (size_t)ldgc * sizeof(double), (size_t)Nc * sizeof(double), rows, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemset2DAsync(W.g + Nz, pitch, 0, (size_t)Nc * sizeof(double), rows, st));
  }
  return dto::border_finish(h, p, P, nb, c, ldc, schur_negdef, schur_singular, nullptr, st);
}

// The compact limited-memory BFGS matrix as the border of the factorised system (dto_border_kernels.hpp: k_lbfgs_panel, k_lbfgs_c):
// the panel [sigma S; Y] and M are formed on the device, then everything dto_kkt_border_factor runs.  The eigenvalue signs of M and
// of the Schur complement come from cyclic Jacobi on the host, over the copies k_border_schur keeps (16 x 16 per instance).
// nr > 0 (dto_kkt_lbfgs_border_rows): the caller's rows join the panel behind the history (k_lbfgs_rows) and their block C the
// diagonal block behind M (k_lbfgs_c_rows); nr == 0 launches exactly what dto_kkt_lbfgs_border launched before there were rows.
static int lbfgs_border(dto_problem* h, const char* who, int64_t m, const double* s, int64_t lds, const double* y, int64_t ldy,
                        const int32_t* npairs, const double* sigma, int64_t nr, const double* g_x, int64_t ldgx, const double* g_c, int64_t ldgc,
                        const double* c, int64_t ldc, int32_t* inertia_ok, int32_t* schur_singular, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  const std::string w = who;
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();
  if (rc) return rc;
  if (!p->vt->launch_wide)
    return set_error(DTO_ERR_UNSUPPORTED, (w + ": tile path only (the lane-per-instance solver carries its limited-memory "
                                               "matrix inside its sweeps)").c_str());
  if (!p->wide_kkt || !p->wide_kkt->assembled) return set_error(DTO_ERR_INVALID, "dto_kkt_assemble has not been called");
  if (m < 1) return set_error(DTO_ERR_INVALID, (w + ": m < 1").c_str());
  if (nr < 0) return set_error(DTO_ERR_INVALID, (w + ": nr < 0").c_str());
  if (2 * m > dto::KB_MAX) return set_error(DTO_ERR_UNSUPPORTED, (w + ": more than 8 pairs (16 border rows, one panel of right-hand sides)").c_str());
  if (2 * m + nr > dto::KB_MAX)
    return set_error(DTO_ERR_UNSUPPORTED, (w + ": 2 m + nr > 16 border rows (one panel of right-hand sides)").c_str());
  if (!s || !y || !sigma || (nr > 0 && (!g_x || !c))) return set_error(DTO_ERR_INVALID, "null argument");
  const int64_t Nz = p->L.Nz, Nc = dto::kkt_rows(p), N = Nz + Nc, nb = 2 * m + nr;
  if (lds < Nz || ldy < Nz || (nr > 0 && (ldgx < Nz || (g_c && ldgc < p->L.Nc) || ldc < nr * nr)))
    return set_error(DTO_ERR_INVALID, "leading dimension too small");
  if (!p->wide_kkt->factored)
    return set_error(DTO_ERR_INVALID, "dto_kkt_factor has not been called (or dto_kkt_step_batch / the solver has used the factor storage since)");
  const int64_t B = p->wide_kkt->B;
  std::vector<int> hnp((size_t)B);
  std::vector<double> hsig((size_t)B);
  for (int64_t i = 0; i < B; ++i) {
    const int64_t np = npairs ? npairs[i] : m;
    if (np < 0 || np > m) return set_error(DTO_ERR_INVALID, (w + ": npairs outside 0..m").c_str());
    if (!(sigma[i] > 0.0) || !std::isfinite(sigma[i])) return set_error(DTO_ERR_INVALID, (w + ": sigma must be positive and finite").c_str());
    hnp[(size_t)i] = (int)np; hsig[(size_t)i] = sigma[i];
  }
  const bool has_gc = nr > 0 && g_c != nullptr;
  dto::BorderPlan P;
  if ((rc = dto::border_prepare(p, nb, has_gc, P))) return rc;
  dto::KktBorder& W = *p->kkt_border;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = dto::grow_buf(W.qc, (size_t)B * 256, "dto_kkt_lbfgs_border: hipMalloc of the compact matrix"))) return rc;
  if ((rc = dto::grow_buf(W.skeep, (size_t)B * 256, "dto_kkt_lbfgs_border: hipMalloc of the kept Schur complement"))) return rc;
  if ((rc = dto::grow_buf(W.qsig, (size_t)B, "dto_kkt_lbfgs_border: hipMalloc of sigma"))) return rc;
  HIP_TRY(W.qnp.grow((size_t)B));
  HIP_TRY(hipMemcpyAsync(W.qnp, hnp.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(W.qsig, hsig.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  {
    const size_t n = (size_t)B * (size_t)m * (size_t)Nz;
    hipLaunchKernelGGL(dto::k_lbfgs_panel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, B, (int)m, (int)nb, Nz, s, lds, y, ldy,
                       (const int*)W.qnp, (const double*)W.qsig, (double*)W.g, N);
    HIP_TRY(hipGetLastError());
  }
  // (the constraint side of the history rows is zero; with rows this clears theirs too, and k_lbfgs_rows writes it again)
  if (Nc > 0) HIP_TRY(hipMemset2DAsync(W.g + Nz, (size_t)N * sizeof(double), 0, (size_t)Nc * sizeof(double), (size_t)B * (size_t)nb, st));
  if (nr > 0) {
    const size_t n = (size_t)B * (size_t)N;
    hipLaunchKernelGGL(dto::k_lbfgs_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, B, (int)nb, (int)nr, Nz, Nc, g_x, ldgx, g_c, ldgc,
                       (double*)W.g, N);
    HIP_TRY(hipGetLastError());
  }
  // M from ONE Gram pass over the history: the panel as both operands (the partials are consumed by k_lbfgs_c before the Schur
  // complement's own Gram pass writes them again, on the same stream).  The pass covers the variables' part only -- the history is
  // zero beyond it -- in the chunks of the plan: a chunk that lies beyond it adds zeros.  With rows it runs over all nb rows and
  // k_lbfgs_c_rows reads the history's corner
  hipLaunchKernelGGL(dto::k_border_gram, dim3((unsigned)(B * P.chunks)), dim3(dto::KB_THREADS), 0, st, (int)nb, Nz, (int64_t)0, P.chunk, P.chunks,
                     (const double*)W.g, N, (const double*)nullptr, (int64_t)0, (const double*)W.g, N, (const double*)nullptr, (int64_t)0, (double*)W.part);
  HIP_TRY(hipGetLastError());
  if (nr > 0)
    hipLaunchKernelGGL(dto::k_lbfgs_c_rows, dim3((unsigned)B), dim3(64), 0, st, (int)m, (int)nr, P.chunks, (const double*)W.part, (const int*)W.qnp,
                       (const double*)W.qsig, c, ldc, (double*)W.qc);
  else
    hipLaunchKernelGGL(dto::k_lbfgs_c, dim3((unsigned)B), dim3(64), 0, st, (int)m, P.chunks, (const double*)W.part, (const int*)W.qnp,
                       (const double*)W.qsig, (double*)W.qc);
  HIP_TRY(hipGetLastError());
  if ((rc = dto::border_finish(h, p, P, nb, W.qc, nb * nb, nullptr, schur_singular, W.skeep, st))) return rc;
  if (inertia_ok) {
    // In(K0) + In(Schur) = In(blkdiag(M, C)) + In of the bordered K: with K0 at (Nz, Ns) the bordered K = K0 - U M^-1 U' has
    // (Nz, Ns + nr) exactly when the Schur complement has neg(M) + nr negative eigenvalues.  M is the top-left 2 m x 2 m of the
    // kept sym(blkdiag(M, C)); C is not looked at on its own (it is 0 for an equality row with delta_c = 0)
    std::vector<double> hm((size_t)B * 256), hs((size_t)B * 256);
    HIP_TRY(hipMemcpyAsync(hm.data(), W.csym, hm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hs.data(), W.skeep, hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < B; ++i) {
      bool tiny_m = false, tiny_s = false;
      const int neg_m = dto::small_inertia(&hm[(size_t)i * 256], (int)(2 * m), tiny_m), neg_s = dto::small_inertia(&hs[(size_t)i * 256], (int)nb, tiny_s);
      inertia_ok[i] = (neg_m + (int)nr == neg_s && !tiny_m && !tiny_s) ? 1 : 0;
    }
  }
  return DTO_OK;
}

int dto_kkt_lbfgs_border(dto_problem* h, int64_t m, const double* s, int64_t lds, const double* y, int64_t ldy, const int32_t* npairs,
                         const double* sigma, int32_t* inertia_ok, int32_t* schur_singular, void* stream) {
  return lbfgs_border(h, "dto_kkt_lbfgs_border", m, s, lds, y, ldy, npairs, sigma, 0, nullptr, 0, nullptr, 0, nullptr, 0, inertia_ok, schur_singular,
                      stream);
}

int dto_kkt_lbfgs_border_rows(dto_problem* h, int64_t m, const double* s, int64_t lds, const double* y, int64_t ldy, const int32_t* npairs,
                              const double* sigma, int64_t nr, const double* g_x, int64_t ldgx, const double* g_c, int64_t ldgc, const double* c,
                              int64_t ldc, int32_t* inertia_ok, int32_t* schur_singular, void* stream) {
  return lbfgs_border(h, "dto_kkt_lbfgs_border_rows", m, s, lds, y, ldy, npairs, sigma, nr, g_x, ldgx, g_c, ldgc, c, ldc, inertia_ok, schur_singular,
                      stream);
}

int dto_kkt_border_solve(dto_problem* h, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc, const double* rhs_b,
                         int64_t ldrb, double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc, double* sol_b, int64_t ldsb, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();
  if (rc) return rc;
  if (!p->kkt_border || !p->kkt_border->valid)
    return set_error(DTO_ERR_INVALID, "dto_kkt_border_factor has not been called (or dto_kkt_assemble, dto_kkt_factor, dto_kkt_step_batch or the "
                                      "solver has run since)");
  if ((rc = check_kkt_vectors(p, nullptr, rhs_x, ldrx, rhs_c, ldrc, sol_x, ldsx, sol_c, ldsc))) return rc;
  dto::KktBorder& W = *p->kkt_border;
  if (!rhs_b || !sol_b) return set_error(DTO_ERR_INVALID, "null argument");
  if (ldrb < W.nb || ldsb < W.nb) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  const int64_t Nz = p->L.Nz, Nc = dto::kkt_rows(p), N = Nz + Nc, B = W.B;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = dto_kkt_solve(h, rhs_x, ldrx, rhs_c, ldrc, W.v0, N, W.v0 + Nz, N, stream))) return rc;
  const int* singular = W.iw + (size_t)B * 17;
  hipLaunchKernelGGL(dto::k_border_rhs, dim3((unsigned)B), dim3(dto::KB_RHS_THREADS), 0, st, W.nb, Nz, Nc, (const double*)W.y, N,
                     (const double*)(W.y + Nz), N, rhs_x, ldrx, rhs_c, ldrc, rhs_b, ldrb, (const double*)W.lu, (const int*)W.iw, singular, sol_b, ldsb,
                     W.yw);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dto::k_border_sub, dim3((unsigned)(B * dto::KB_ROW_BLOCKS)), dim3(dto::KB_THREADS), 0, st, W.nb, Nz, Nc, (const double*)W.v0,
                     (const double*)W.y, N, (const double*)(W.y + Nz), N, (const double*)W.yw, sol_x, ldsx, sol_c, ldsc);
  HIP_TRY(hipGetLastError());
  return DTO_OK;
}

// ---- the bordered matrix as an operator and refined bordered solves (tile path): K v from k_wide_kmul, the border part from one
//      pass over the kept panel (k_border_mul, with the chunks of the factor call) and sym(C) v_b from what k_border_schur kept.
// The checks both entry points share, in the order of dto_kkt_border_solve: path, border in place, `bad`, the vectors.
static int check_border_vectors(Problem* p, const char* who, const char* bad, const double* in_x, int64_t ldix, const double* in_c,
                                int64_t ldic, const double* in_b, int64_t ldib, const double* out_x, int64_t ldox, const double* out_c,
                                int64_t ldoc, const double* out_b, int64_t ldob) {
  if (!p->vt->launch_wide)
    return set_error(DTO_ERR_UNSUPPORTED, (std::string(who) + ": tile path only (the lane-per-instance path keeps no assembled system to "
                                           "multiply with: dto_kkt_multiply is unsupported there)").c_str());
  if (!p->kkt_border || !p->kkt_border->valid)
    return set_error(DTO_ERR_INVALID, "dto_kkt_border_factor has not been called (or dto_kkt_assemble, dto_kkt_factor, dto_kkt_step_batch or the "
                                      "solver has run since)");
  if (int rc = check_kkt_vectors(p, bad, in_x, ldix, in_c, ldic, out_x, ldox, out_c, ldoc)) return rc;
  if (!in_b || !out_b) return set_error(DTO_ERR_INVALID, "null argument");
  if (ldib < p->kkt_border->nb || ldob < p->kkt_border->nb) return set_error(DTO_ERR_INVALID, "leading dimension too small");
  return DTO_OK;
}
static int border_multiply(Problem* p, const double* v_x, int64_t ldvx, const double* v_c, int64_t ldvc, const double* v_b, int64_t ldvb,
                           double* out_x, int64_t ldox, double* out_c, int64_t ldoc, double* out_b, int64_t ldob, hipStream_t st) {
  dto::KktBorder& W = *p->kkt_border;
  const int64_t Nz = p->L.Nz, Nc = dto::kkt_rows(p), N = Nz + Nc, B = W.B;
  if (int rc = dto::wide_kkt_multiply(p, v_x, ldvx, v_c, ldvc, out_x, ldox, out_c, ldoc, st)) return rc;
  hipLaunchKernelGGL(dto::k_border_mul, dim3((unsigned)(B * W.chunks)), dim3(dto::KB_THREADS), 0, st, W.nb, Nz, W.n_c, W.chunk, W.chunks,
                     (const double*)W.g, N, (const double*)(W.g + Nz), N, v_x, ldvx, v_c, ldvc, v_b, ldvb, out_x, ldox, out_c, ldoc,
                     (double*)W.tpart);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dto::k_border_mul_fin, dim3((unsigned)B), dim3(64), 0, st, W.nb, W.chunks, (const double*)W.tpart, (const double*)W.csym,
                     v_b, ldvb, out_b, ldob);
  HIP_TRY(hipGetLastError());
  return DTO_OK;
}

int dto_kkt_border_multiply(dto_problem* h, const double* v_x, int64_t ldvx, const double* v_c, int64_t ldvc, const double* v_b, int64_t ldvb,
                            double* out_x, int64_t ldox, double* out_c, int64_t ldoc, double* out_b, int64_t ldob, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();
  if (rc) return rc;
  if ((rc = check_border_vectors(p, "dto_kkt_border_multiply", nullptr, v_x, ldvx, v_c, ldvc, v_b, ldvb, out_x, ldox, out_c, ldoc, out_b, ldob)))
    return rc;
  return border_multiply(p, v_x, ldvx, v_c, ldvc, v_b, ldvb, out_x, ldox, out_c, ldoc, out_b, ldob, (hipStream_t)stream);
}

// dto_kkt_border_solve, then `passes` rounds of (rho, sigma) = (r, s) - M (v, y), (dv, dy) = the bordered solve of it, (v, y) += (dv, dy);
// with `resid` one more product for max |(r, s) - M (v, y)| of what is returned.  A row of the workspace is [x | c | border]: the
// border segment is a third short row of the row kernels.  The correction solves write the workspace, never the caller's arrays
// (v0 and yw of the handle are scratch of every bordered solve).
int dto_kkt_border_solve_refined(dto_problem* h, int passes, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc,
                                 const double* rhs_b, int64_t ldrb, double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc, double* sol_b,
                                 int64_t ldsb, double* resid, void* stream) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();
  if (rc) return rc;
  if ((rc = check_border_vectors(p, "dto_kkt_border_solve_refined", passes < 0 || passes > 4 ? "passes outside 0..4" : nullptr, rhs_x, ldrx,
                                 rhs_c, ldrc, rhs_b, ldrb, sol_x, ldsx, sol_c, ldsc, sol_b, ldsb)))
    return rc;
  if ((rc = dto_kkt_border_solve(h, rhs_x, ldrx, rhs_c, ldrc, rhs_b, ldrb, sol_x, ldsx, sol_c, ldsc, sol_b, ldsb, stream))) return rc;
  if (passes == 0 && !resid) return DTO_OK;
  dto::KktBorder& W = *p->kkt_border;
  const int64_t Nz = p->L.Nz, Nc = dto::kkt_rows(p), N = Nz + Nc, ld = N + dto::KB_MAX, B = W.B;
  const int nb = W.nb;
  hipStream_t st = (hipStream_t)stream;
  const size_t need = (size_t)B * (size_t)ld;
  const std::string what = "dto_kkt_border_solve_refined: hipMalloc of a workspace array (" + std::to_string(need * sizeof(double)) +
                           " bytes: " + std::to_string(B) + " instances x " + std::to_string(ld) + " doubles)";
  if ((rc = dto::grow_buf(W.ref_r, need, what.c_str()))) return rc;
  if ((rc = dto::grow_buf(W.ref_d, need, what.c_str()))) return rc;
  double *r_x = W.ref_r, *r_c = r_x + Nz, *r_b = r_x + N, *d_x = W.ref_d, *d_c = d_x + Nz, *d_b = d_x + N;
  const dim3 grid((unsigned)(B * dto::AXPY_BLOCKS_PER_ROW)), block(256);
  auto residual = [&]() -> int {   // ref_r = rhs - M sol (M sol passes through ref_d)
    if (int e = border_multiply(p, sol_x, ldsx, sol_c, ldsc, sol_b, ldsb, d_x, ld, d_c, ld, d_b, ld, st)) return e;
    hipLaunchKernelGGL(dto::k_rows_residual, grid, block, 0, st, r_x, rhs_x, (const double*)d_x, Nz, ld, ldrx, ld);
    if (Nc > 0) hipLaunchKernelGGL(dto::k_rows_residual, grid, block, 0, st, r_c, rhs_c, (const double*)d_c, Nc, ld, ldrc, ld);
    hipLaunchKernelGGL(dto::k_rows_residual, grid, block, 0, st, r_b, rhs_b, (const double*)d_b, (int64_t)nb, ld, ldrb, ld);
    HIP_TRY(hipGetLastError());
    return DTO_OK;
  };
  for (int it = 0; it < passes; ++it) {
    if ((rc = residual())) return rc;
    if ((rc = dto_kkt_border_solve(h, r_x, ld, r_c, ld, r_b, ld, d_x, ld, d_c, ld, d_b, ld, stream))) return rc;
    hipLaunchKernelGGL(dto::k_rows_add, grid, block, 0, st, sol_x, (const double*)d_x, Nz, ldsx, ld);
    if (Nc > 0) hipLaunchKernelGGL(dto::k_rows_add, grid, block, 0, st, sol_c, (const double*)d_c, Nc, ldsc, ld);
    hipLaunchKernelGGL(dto::k_rows_add, grid, block, 0, st, sol_b, (const double*)d_b, (int64_t)nb, ldsb, ld);
    HIP_TRY(hipGetLastError());
  }
  if (resid) {
    if ((rc = residual())) return rc;
    // (the x, c and border segments of a workspace row are contiguous: one maximum over Nz + Nc + nb entries)
    hipLaunchKernelGGL(dto::k_rows_maxabs, dim3((unsigned)B), dim3(256), 0, st, (const double*)W.ref_r, N + nb, ld, resid);
    hipLaunchKernelGGL(dto::k_border_resid_singular, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B, (const int*)(W.iw + (size_t)B * 17),
                       resid);
    HIP_TRY(hipGetLastError());
  }
  return DTO_OK;
}

int dto_shard_range(int64_t total, int rank, int world, int64_t* first, int64_t* count) {
  if (total < 0 || world < 1 || rank < 0 || rank >= world || !first || !count) return set_error(DTO_ERR_INVALID, "bad shard arguments");
  const int64_t lo = (total * rank) / world, hi = (total * (rank + 1)) / world;
  *first = lo;
  *count = hi - lo;
  return DTO_OK;
}

int dto_solve(dto_problem* h, const dto_options* opt, const double* x0, double* x, double* mu, int32_t* status,
              int32_t* iterations) {
  Problem* p = reinterpret_cast<Problem*>(h);
  if (!p || !x0 || !x) return set_error(DTO_ERR_INVALID, "null argument");
  int rc = p->ensure_device();
  if (rc) return rc;
  const dto::Layout& L = p->L;
  dto::DevBuf<double> d_x, d_mu;   // released on every path
  HIP_TRY(d_x.alloc(L.Nz));
  HIP_TRY(d_mu.alloc(L.Nc));
  HIP_TRY(hipMemcpy(d_x, x0, L.Nz * sizeof(double), hipMemcpyHostToDevice));
  dto_batch b;
  b.B = 1; b.x = d_x; b.ldx = L.Nz; b.params = nullptr; b.ldp = 0; b.stream = (void*)p->stream;
  if ((rc = dto_solve_batch(h, opt, &b, d_x, L.Nz, d_mu, L.Nc, status, iterations))) return rc;
  HIP_TRY(hipMemcpy(x, d_x, L.Nz * sizeof(double), hipMemcpyDeviceToHost));
  if (mu) HIP_TRY(hipMemcpy(mu, d_mu, L.Nc * sizeof(double), hipMemcpyDeviceToHost));
  return DTO_OK;
}

}  // extern "C"

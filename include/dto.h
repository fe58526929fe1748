/*
 * dto.h -- C ABI of the MI355X-native sparse NLP callback + KKT engine.
 *
 * Drop-in boundary for DirectTrajectoryOptimization.jl's collocation hot path.  The reference
 * has no FFI of its own: its boundary is the MathOptInterface evaluator protocol implemented on
 * `NLPData` (reference src/data.jl:106, src/moi.jl:1-125) and consumed by Ipopt.jl.  Every entry
 * point below names the reference method it replaces; a Julia `ccall` shim that implements the
 * MOI methods on top of these calls is shown in INTEGRATION.md.
 *
 * Conventions (same as the reference unless stated):
 *   - all numerics are double, all structure indices are int64 and 1-BASED (Julia convention),
 *   - variables      z = [x_1; u_1; ...; x_{T-1}; u_{T-1}; x_T]          (src/dynamics.jl:188-195)
 *   - constraints    [dynamics t=1..T-1; stage t=1..T; general]           (src/data.jl:64-75)
 *   - Jacobian       COO list, dynamics ++ stage ++ general, local CSC order (src/data.jl:170-175)
 *   - Hessian        sort(unique(raw)) key, row-major, BOTH triangles       (src/data.jl:184)
 *   - output buffers are caller-owned and fully overwritten (src/moi.jl:16,33,53,73),
 *   - every function returns an int status (DTO_OK = 0); nothing throws across the ABI,
 *   - a handle is not thread-safe (the reference evaluator is not re-entrant either).
 *
 * Pointers are HOST pointers for the dto_eval_* family (the MOI-callback replacement: one
 * instance, copied over PCIe) and DEVICE pointers for the *_batch / kkt / solve families
 * (B instances resident in HBM, instance-major: instance b starts at ptr + b*ld).
 */
#ifndef DTO_H
#define DTO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTO_ABI_VERSION 4

enum dto_status {
  DTO_OK = 0,
  DTO_ERR_INVALID = 1,      /* bad argument / inconsistent spec */
  DTO_ERR_PLUGIN = 2,       /* model plugin missing or wrong ABI */
  DTO_ERR_DEVICE = 3,       /* HIP error (no GPU, OOM, launch failure) */
  DTO_ERR_UNSUPPORTED = 4,  /* feature outside the built path */
  DTO_ERR_NOT_CONVERGED = 5
};

/* feature bits, MOI.features_available (src/moi.jl:122) */
#define DTO_FEATURE_GRAD 1
#define DTO_FEATURE_JAC 2
#define DTO_FEATURE_HESS 4

typedef struct dto_problem dto_problem; /* opaque; plays the role of NLPData (src/data.jl:106-121) */

/*
 * Problem description: what `Solver(dynamics, objective, constraints, bounds; ...)` receives
 * (src/solver.jl:6-21) after the per-stage objects have been compiled into a model plugin.
 * `stage_kind[t]` selects, for stage t (0-based here), one entry of the plugin's kind table
 * = (dynamics class, previous dynamics class, cost class, constraint class).
 */
typedef struct dto_problem_spec {
  int abi_version;            /* DTO_ABI_VERSION */
  const char* model_library;  /* path of the generated plugin .so (gfx950 code object inside) */
  int horizon;                /* T */
  const int32_t* stage_kind;  /* [T] */
  const double* variable_lower; /* [num_variables] or NULL = -Inf  (src/data.jl:123-133) */
  const double* variable_upper; /* [num_variables] or NULL = +Inf */
  const double* parameters;     /* [num_parameters] flattened w_1..w_T (src/data.jl:218) or NULL */
  int64_t num_parameters;       /* length of `parameters`; must equal dto_sizes_t.num_parameters (sum over the stages of the
                                   largest num_parameter among the stage's dynamics, cost and constraint) when it is given */
  int evaluate_hessian;         /* Solver(...; evaluate_hessian) (src/solver.jl:7) */
} dto_problem_spec;

int dto_problem_create(const dto_problem_spec* spec, dto_problem** out);
int dto_problem_destroy(dto_problem* p);
const char* dto_last_error(void);

/* totals of NLPData (src/data.jl:155-167,187): nnz_hess_key = length(hessian_lagrangian_structure),
 * nnz_hess_raw = nlp.num_hessian_lagrangian (duplicate-counting). */
typedef struct dto_sizes_t {
  int64_t num_variables, num_parameters;
  int64_t num_constraint, num_constraint_dynamics, num_constraint_stage, num_constraint_general;
  int64_t num_jacobian, num_jacobian_dynamics, num_jacobian_stage, num_jacobian_general;
  int64_t nnz_hess_key, nnz_hess_raw;
  int64_t horizon, num_state_max, num_action_max;
} dto_sizes_t;
int dto_sizes(const dto_problem* p, dto_sizes_t* out);

/* MOI.features_available (src/moi.jl:122) */
int dto_features_available(const dto_problem* p, int* feature_bits);
/* MOI.jacobian_structure (src/moi.jl:124): rows/cols [num_jacobian], 1-based */
int dto_jacobian_structure(const dto_problem* p, int64_t* rows, int64_t* cols);
/* MOI.hessian_lagrangian_structure (src/moi.jl:125): rows/cols [nnz_hess_key], 1-based */
int dto_hessian_structure(const dto_problem* p, int64_t* rows, int64_t* cols);
/* The KKT matrix of the reference's scratch (examples/pendulum/pendulum.jl:138-198, built there with spzeros + index loops and
 * handed to QDLDL), in CSR form and in the reference ordering [z; dynamics rows; stage rows; general rows]:
 *     K = [ H + delta_w I   J' ;  J   -delta_c I ],   dimension num_variables + num_constraint,
 * full symmetric pattern (both triangles, like the Hessian key: src/data.jl:184), columns sorted inside every row, 1-based.
 * dto_kkt_csr_structure: row_ptr [dim + 1], col_ind [nnz]; either may be NULL to query *dim / *nnz only (HOST arrays).
 * dto_kkt_csr_values_batch: values [B][ldv] (DEVICE) from evaluated Hessian-of-the-Lagrangian values H [B][ldh] (order of
 * dto_hessian_structure: dto_eval_h_batch) and Jacobian values J [B][ldj] (dto_eval_jac_g_batch): one gather per CSR slot,
 * fully coalesced stores -- for a caller that wants K itself (an A/B against QDLDL / MUMPS, or its own factorisation). */
int dto_kkt_csr_structure(dto_problem* p, int64_t* row_ptr, int64_t* col_ind, int64_t* dim, int64_t* nnz);
int dto_kkt_csr_values_batch(dto_problem* p, int64_t B, const double* H, int64_t ldh, const double* J, int64_t ldj,
                             double delta_w, double delta_c, double* values, int64_t ldv, void* stream);
/* nlp.variable_bounds / nlp.constraint_bounds (src/data.jl:123-148) */
int dto_variable_bounds(const dto_problem* p, double* lower, double* upper);
int dto_constraint_bounds(const dto_problem* p, double* lower, double* upper);

/* TrajectoryOptimizationIndices (src/data.jl:44-104): 1-based index vector of stage t (1-based t).
 * Returns the length in *n; `out` may be NULL to query the length. */
enum dto_index_kind {
  DTO_IDX_STATE = 0,                 /* indices.states[t]               src/dynamics.jl:188-191 */
  DTO_IDX_ACTION = 1,                /* indices.actions[t]              src/dynamics.jl:193-195 */
  DTO_IDX_STATE_ACTION = 2,          /* indices.state_action[t]         src/dynamics.jl:197-200 */
  DTO_IDX_STATE_ACTION_NEXT = 3,     /* indices.state_action_next_state src/dynamics.jl:202-204 */
  DTO_IDX_DYNAMICS_CONSTRAINT = 4,   /* indices.dynamics_constraints[t] src/dynamics.jl:162-165 */
  DTO_IDX_DYNAMICS_JACOBIAN = 5,     /* indices.dynamics_jacobians[t]   src/dynamics.jl:167-170 */
  DTO_IDX_DYNAMICS_HESSIAN = 6,      /* indices.dynamics_hessians[t]    src/dynamics.jl:172-186 */
  DTO_IDX_STAGE_CONSTRAINT = 7,      /* indices.stage_constraints[t]    src/constraints.jl:141-153 */
  DTO_IDX_STAGE_JACOBIAN = 8,        /* indices.stage_jacobians[t]      src/constraints.jl:155-166 */
  DTO_IDX_STAGE_HESSIAN = 9,         /* indices.stage_hessians[t]       src/constraints.jl:168-183 */
  DTO_IDX_OBJECTIVE_HESSIAN = 10     /* indices.objective_hessians[t]   src/costs.jl:88-104 */
};
int dto_stage_indices(const dto_problem* p, int which, int t, int64_t* out, int64_t* n);

/* ---- the five MOI evaluator methods, one instance, HOST pointers --------------------------- */
/* MOI.eval_objective (src/moi.jl:1-13) */
int dto_eval_f(dto_problem* p, const double* x, double* f);
/* MOI.eval_objective_gradient (src/moi.jl:15-30): g[num_variables] */
int dto_eval_grad_f(dto_problem* p, const double* x, double* g);
/* MOI.eval_constraint (src/moi.jl:32-50): c[num_constraint] */
int dto_eval_g(dto_problem* p, const double* x, double* c);
/* MOI.eval_constraint_jacobian (src/moi.jl:52-70): J[num_jacobian], order of dto_jacobian_structure */
int dto_eval_jac_g(dto_problem* p, const double* x, double* J);
/* MOI.eval_hessian_lagrangian (src/moi.jl:72-120): H[nnz_hess_key], order of dto_hessian_structure */
int dto_eval_h(dto_problem* p, const double* x, double sigma, const double* mu, double* H);

/* ---- batched forms: B independent instances, DEVICE pointers, asynchronous on `stream` -------
 * x: [B][ldx] (ldx >= num_variables); outputs instance-major with the given leading dimension.
 * params: NULL = the spec's parameters shared by all instances, else [B][ldp] (also honoured by the solver entry points
 * dto_kkt_step_batch / dto_solve_batch / dto_solver_begin: one parameter set per instance, e.g. MPC rollouts).
 * These run the same kernels as above without the PCIe copies. `stream` is a hipStream_t. */
typedef struct dto_batch {
  int64_t B;
  const double* x;      int64_t ldx;
  const double* params; int64_t ldp;
  void* stream;
} dto_batch;
int dto_eval_f_batch(dto_problem* p, const dto_batch* b, double* f /* [B] */);
int dto_eval_grad_f_batch(dto_problem* p, const dto_batch* b, double* g, int64_t ldg);
int dto_eval_g_batch(dto_problem* p, const dto_batch* b, double* c, int64_t ldc);
int dto_eval_jac_g_batch(dto_problem* p, const dto_batch* b, double* J, int64_t ldj);
/* sigma: host scalar applied to every instance; mu: [B][ldmu] */
int dto_eval_h_batch(dto_problem* p, const dto_batch* b, double sigma, const double* mu, int64_t ldmu,
                     double* H, int64_t ldh);

/* ---- KKT step and solver: the work the reference delegates to Ipopt (src/solver.jl:45-47,
 *      src/data.jl:229-255) -------------------------------------------------------------------- */

/* Solver options: the subset of reference `Options` (src/options.jl:6-36) that defines convergence,
 * plus the interior-point constants Ipopt documents as defaults.  Print/file options of the
 * reference are out of scope. */
typedef struct dto_options {
  double tol;               /* 1e-6  src/options.jl:7  */
  double s_max;             /* 100   src/options.jl:8  */
  int max_iter;             /* 1000  src/options.jl:9  */
  double dual_inf_tol;      /* 1.0   src/options.jl:12 */
  double constr_viol_tol;   /* 1e-3  src/options.jl:13 */
  double compl_inf_tol;     /* 1e-3  src/options.jl:14 */
  double mu_init;           /* 0.1   (Ipopt default)   */
  double delta_c;           /* 1e-8  dual regularisation, examples/pendulum/pendulum.jl:195 uses 1e-5 */
  double delta_w_init;      /* 1e-4  first primal regularisation tried when the inertia is wrong */
  int check_every;          /* host polls the batch for completion every this many iterations */
  double max_cpu_time;      /* 300   src/options.jl:10: wall-clock limit of one dto_solve[_batch] call in seconds; instances
                               still running when it expires are returned as they are with DTO_STATUS_CPU_TIME (6) */
  /* Ipopt's "acceptable" termination (src/options.jl:15-20): an instance stops with status 4 after `acceptable_iter`
   * consecutive iterations whose scaled error is <= acceptable_tol, whose unscaled residuals are within the three
   * acceptable_*_tol values and whose objective changed by less than acceptable_obj_change_tol (relative). 0 = off. */
  double acceptable_tol;             /* 1e-6  src/options.jl:15 */
  int acceptable_iter;               /* 15    src/options.jl:16 */
  double acceptable_dual_inf_tol;    /* 1e10  src/options.jl:17 */
  double acceptable_constr_viol_tol; /* 1e-2  src/options.jl:18 */
  double acceptable_compl_inf_tol;   /* 1e-2  src/options.jl:19 */
  double acceptable_obj_change_tol;  /* 1e-5  src/options.jl:20 */
  double diverging_iterates_tol;     /* 1e8   src/options.jl:21: status 5 once max|z_i| exceeds it */
  double mu_target;                  /* 1e-4  src/options.jl:22: the barrier parameter is not driven below it and the
                                        complementarity in every termination test is measured against it (Ipopt's
                                        mu_target semantics); only matters for problems with bounds / inequality rows */
  /* ABI 3: globalisation.  DTO_LS_FILTER = Ipopt's filter line search from the first iteration (what the reference runs,
   * src/solver.jl:45-47).  DTO_LS_PENALTY_FILTER (default) = while the iterate is far from the constraint manifold
   * (max |c_i| > penalty_switch_theta) the step size is chosen on the l1 exact-penalty function, then the filter takes over:
   * same minimisers class, acrobot T = 1000 from the reference's straight-line guess in a median of ~60 instead of ~630
   * iterations.  Lane-per-instance solver path; the tile (64-state) and bordered paths run the filter. */
  int line_search;                   /* DTO_LS_PENALTY_FILTER */
  double penalty_switch_theta;       /* 1.0 */
  /* ABI 3: what stands in for the Hessian of the Lagrangian.  DTO_HESSIAN_EXACT: second derivatives of the traced expressions.
   * DTO_HESSIAN_LBFGS: Ipopt's hessian_approximation = limited-memory, i.e. what the reference runs when a problem is built
   * with evaluate_hessian = false (src/solver.jl:7, its default and its own acrobot / car examples): compact L-BFGS, history 6,
   * sigma = s'y / s's, updates skipped without curvature -- no second derivatives are evaluated.  Lane-per-instance solver
   * path, and dto_solve_batch / dto_solve on the tile path (17 .. 64 states): there the compact matrix is a border of 12 rows on a
   * first-order factorisation (dto_kkt_assemble_first_order, dto_kkt_lbfgs_border) inside the host-driven bordered loop, with at
   * most four coupling rows in limited-memory mode on the tile path (multi-knot GeneralConstraint rows share the panel of 16:
   * dto_kkt_lbfgs_border_rows; with more than four the exact second derivatives run and are reported).  Where the mode does not exist the library says what it runs instead (dto_solver_hessian_mode): a
   * model plugin built without Hessians (evaluate_hessian = 0 in its generator) keeps per-stage SR1 blocks; the STEPWISE entry
   * points of the tile path (dto_solver_begin / begin_warm / iterate / run / shift) keep their exact-Hessian state and report
   * DTO_HESSIAN_EXACT whatever is asked for -- only dto_solve_batch / dto_solve run the limited-memory mode there -- and the
   * bordered (multi-knot GeneralConstraint) path of the lane-per-instance solver uses the exact second derivatives of the traced
   * expressions. */
  int hessian_approximation;         /* DTO_HESSIAN_EXACT */
  /* ABI 4: passes of iterative refinement per KKT step (0 = none).  One pass: the residual r = b - K v of the step just computed,
   * evaluated stage by stage from the code the sweeps factorise, one more factor + solve for K e = r, v := v + e.  Measured on the
   * acrobot T = 1000 bench state against an extended-precision solve of the oracle's K (profiles/r06/step_truth_*.json): the
   * sequential sweeps (batches that fill the GPU) are within 1e-9 of it without any pass; the time-partitioned sweeps (small
   * batches: chunks joined through a separator system) within 2.5e-8, 5e-6 at delta_w = 0, and within 1e-10 after one pass, which
   * costs them one more factor + solve per iteration.  Lane-per-instance path, exact-Hessian plugins; ignored elsewhere. */
  int kkt_refinement;                /* 0 */
} dto_options;
enum { DTO_LS_FILTER = 0, DTO_LS_PENALTY_FILTER = 1 };
enum { DTO_HESSIAN_EXACT = 0, DTO_HESSIAN_LBFGS = 1, DTO_HESSIAN_SR1_BLOCKS = 2 /* reported only: dto_solver_hessian_mode */ };
/* per-instance status reported by dto_solve[_batch] / dto_solver_run / dto_solver_stats */
enum { DTO_STATUS_RUNNING = 0, DTO_STATUS_CONVERGED = 1, DTO_STATUS_MAX_ITER = 2, DTO_STATUS_NONFINITE = 3,
       DTO_STATUS_ACCEPTABLE = 4, DTO_STATUS_DIVERGING = 5, DTO_STATUS_CPU_TIME = 6 /* cut off by max_cpu_time */ };
int dto_options_default(dto_options* o);

/* One regularised Newton-KKT step at given (x, mu), all constraints treated as equalities and bounds
 * ignored -- exactly the system of examples/pendulum/pendulum.jl:138-198:
 *     [ H + delta_w I   J' ] [dx ]     [ grad f + J' mu ]
 *     [ J         -delta_c I ] [dmu] = - [ c              ]
 * assembled stage-interleaved and solved by the block-tridiagonal LDL^T.  DEVICE pointers,
 * instance-major; dx: [B][lddx], dmu: [B][lddmu].  *inertia_ok (host, may be NULL) is set to 0 if any
 * instance had a pivot of the wrong sign (the matrix is not quasi-definite for this delta_w). */
int dto_kkt_step_batch(dto_problem* p, const dto_batch* b, const double* mu, int64_t ldmu, double delta_w,
                       double delta_c, double* dx, int64_t lddx, double* dmu, int64_t lddmu, int* inertia_ok);

/* ---- the linear solver alone: for a caller that keeps its own outer iteration (Ipopt's augmented system,
 *      cf. the sketch at examples/pendulum/pendulum.jl:138-198 with delta_w / delta_c on the diagonals):
 *     [ W(x, mu) + diag(sigma_x) + delta_w I            J(x)'               ] [ sol_x ]   [ rhs_x ]
 *     [ J(x)                              -diag(sigma_c) - delta_c I  ] [ sol_c ] = [ rhs_c ]
 *  W = hess f + sum_i mu_i hess c_i (exact Hessians), every constraint row treated as an equality, bounds ignored -- barrier
 *  terms enter through sigma_x / sigma_c.  DEVICE pointers, instance-major.  dto_kkt_assemble packs the point and the
 *  diagonals; dto_kkt_factor runs the block-tridiagonal LDL^T once and reports the inertia (HOST arrays [B], may be NULL:
 *  inertia_ok[i] = the matrix has exactly num_constraint negative and no tiny pivots; num_negative[i] = negative pivots);
 *  dto_kkt_solve solves for one right-hand side, any number of times per factorisation.  What a solve costs depends on the path:
 *  - lane-per-instance path (states <= 16): the factors are NOT stored between calls -- the sweeps recompute each stage's
 *    LDL^T, which is cheaper than the HBM traffic on this hardware -- so every dto_kkt_solve costs a forward + backward sweep;
 *  - tile (MFMA) path (64-state models, and 17 .. 63-state problems in their 64-state embedding): dto_kkt_factor STORES the
 *    factor, about 170 KB per stage and instance (B x T x 145 024 bytes with one action; dto_kkt_assemble allocates it and
 *    reports the size if that fails), and dto_kkt_solve is substitution only: one forward and one backward pass over the
 *    stored records, no O(n^3) work.  The storage is shared with dto_kkt_step_batch and the solver entry points of the same
 *    handle: any of them invalidates the stored factor, and dto_kkt_solve then fails with DTO_ERR_INVALID until
 *    dto_kkt_factor is called again (the assembled system is kept).  dto_kkt_assemble copies the point, the multipliers, the
 *    diagonals and the batch's parameters, so the caller's arrays may change after it returns.
 *  Problems with GeneralConstraint rows (both paths): K is the STAGE part K_s, of dimension num_variables + Ns with Ns =
 *  num_constraint - (number of general rows); the general rows are the caller's border (dto_kkt_border_factor below).  Every
 *  constraint-side array keeps its length and leading dimension (>= num_constraint), but on the tile path its last entries, those of
 *  the general rows, are neither read nor written -- mu, sigma_c, rhs_c, sol_c here, v_c / out_c of dto_kkt_multiply, g_c of
 *  dto_kkt_border_factor -- and inertia_ok expects Ns negative pivots.  This holds for every entry point of this block and of the
 *  two blocks below (stage Constraint rows are not taken on the tile path: DTO_ERR_UNSUPPORTED).
 *  Order: assemble, factor, solve; dto_kkt_factor before dto_kkt_assemble and dto_kkt_solve before dto_kkt_factor fail with
 *  DTO_ERR_INVALID.  The single factorisation attempt is swept to the end whatever its inertia: dto_kkt_solve returns
 *  K^-1 rhs (unpivoted) also when inertia_ok is 0.
 *  dto_kkt_solve_multi solves for nrhs right-hand sides per instance against the same factorisation: right-hand side r of
 *  instance b is row b * nrhs + r of rhs_x ([B * nrhs][ldrx]) and of rhs_c, and its solution is the same row of sol_x / sol_c;
 *  nrhs = 1 is the layout of dto_kkt_solve.  The solutions must not overlap the right-hand sides.  Same state and same errors
 *  as dto_kkt_solve, DTO_ERR_INVALID also for nrhs < 1; an indefinite matrix gives the unpivoted K^-1 rhs.  Cost per path:
 *  - lane-per-instance path: nrhs passes of dto_kkt_solve (there is no stored factor to share), results bit-identical to them;
 *  - tile path: the right-hand sides travel as 64 x 16 panels, so the stored records are read once forward and once backward
 *    per block of 16 right-hand sides instead of once per right-hand side, and the triangular solves and matrix products of
 *    a stage run on the matrix cores.  The records are only read (the intermediates of a block go to a workspace of
 *    B x T x 16 x (128 + actions) doubles, allocated by the first call; the size is reported if that fails), so
 *    dto_kkt_solve and dto_kkt_solve_multi may be mixed in any order on one factorisation.  With a single right-hand side
 *    dto_kkt_solve is the cheaper call.
 *  dto_kkt_multiply writes [out_x; out_c] = K [v_x; v_c] for the system of dto_kkt_assemble,
 *      K = [ W(x,mu) + diag(sigma_x) + delta_w I    J(x)'                      ]
 *          [ J(x)                                   -diag(sigma_c) - delta_c I ],
 *  per instance, v and the product as [B][ld] DEVICE arrays in the layout of rhs_x / rhs_c and sol_x / sol_c.  It needs
 *  dto_kkt_assemble only, not a factorisation: the blocks are rebuilt from the point stage by stage, the stored factor is
 *  neither read nor invalidated, so the call may stand anywhere among dto_kkt_factor / dto_kkt_solve / dto_kkt_solve_multi.
 *  The product must not overlap v.  Results are bit-identical from run to run (no atomic sums).  Errors: DTO_ERR_INVALID before
 *  dto_kkt_assemble, for a null array or a leading dimension below the row length.
 *  dto_kkt_solve_refined is dto_kkt_solve followed by `passes` rounds of iterative refinement against the same stored factor:
 *  r = rhs - K sol (the product above, residual in working precision), d = K^-1 r (substitution only), sol += d.  passes = 0
 *  is dto_kkt_solve, bit for bit; 1 .. 4 are accepted, anything else is DTO_ERR_INVALID.  resid: DEVICE [B] or NULL -- when
 *  given, one further product writes max |rhs - K sol| over the rows of each instance for the solution returned.  The
 *  factorisation is not repeated, so a pass (one product, one substitution) costs far less than a new dto_kkt_factor; where the single
 *  attempt of dto_kkt_factor met an indefinite block (inertia_ok 0) the unpivoted solve loses digits that the passes win back
 *  as long as the factor is still a contraction.  Same state and same errors as dto_kkt_solve (assemble, factor, a factor not
 *  taken by dto_kkt_step_batch or the solver); the solution must not overlap the right-hand side.  Workspace: two arrays of
 *  B x (num_variables + num_constraint) doubles kept with the handle, allocated by the first call that needs them (the size
 *  is reported if that fails).  Per path:
 *  - tile path: as described;
 *  - lane-per-instance path: both return DTO_ERR_UNSUPPORTED -- no assembled system or factor is kept there (the sweeps
 *    rebuild the stage blocks in registers), and refinement lives in its solver (dto_options.kkt_refinement). */
typedef struct dto_kkt_system {
  const double* mu;      int64_t ldmu;   /* [B][ldmu] multipliers inside W */
  const double* sigma_x; int64_t ldsx;   /* [B][ldsx] >= 0, or NULL */
  const double* sigma_c; int64_t ldsc;   /* [B][ldsc] >= 0, or NULL */
  double delta_w, delta_c;
} dto_kkt_system;
int dto_kkt_assemble(dto_problem* p, const dto_batch* b, const dto_kkt_system* sys);
int dto_kkt_factor(dto_problem* p, int32_t* inertia_ok, int32_t* num_negative, void* stream);
int dto_kkt_solve(dto_problem* p, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc, double* sol_x,
                  int64_t ldsx, double* sol_c, int64_t ldsc, void* stream);
int dto_kkt_solve_multi(dto_problem* p, int64_t nrhs, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc,
                        double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc, void* stream);
int dto_kkt_multiply(dto_problem* p, const double* v_x, int64_t ldvx, const double* v_c, int64_t ldvc, double* out_x,
                     int64_t ldox, double* out_c, int64_t ldoc, void* stream);
int dto_kkt_solve_refined(dto_problem* p, int passes, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc,
                          double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc, double* resid, void* stream);
/* dto_kkt_assemble with W = 0 (tile path): the first-order system
 *     K0 = [ diag(sigma_x) + delta_w I    J(x)'                      ]
 *          [ J(x)                         -diag(sigma_c) - delta_c I ]
 * No second derivative of a cost or a dynamics function is evaluated; sys->mu is not read and may be NULL.  The handle is in the
 * state dto_kkt_assemble leaves it in, until the next assemble of either kind: dto_kkt_factor, _solve, _solve_multi, _multiply,
 * _solve_refined and the dto_kkt_border_* / dto_kkt_lbfgs_border calls then act on K0.  A caller with a quasi-Newton matrix of
 * its own puts the scalar part on the diagonal through sigma_x and the low-rank part on the border.  Every other rule is
 * dto_kkt_assemble's: stage Constraint rows are DTO_ERR_UNSUPPORTED, with GeneralConstraint rows K0 is the stage part, a leading
 * dimension below its row length is DTO_ERR_INVALID, a refused call writes nothing.  Lane-per-instance path: DTO_ERR_UNSUPPORTED
 * ("tile path only", as dto_kkt_multiply). */
int dto_kkt_assemble_first_order(dto_problem* p, const dto_batch* b, const dto_kkt_system* sys);
/* Bordered solves against the factor of dto_kkt_factor.  For every instance, with K the matrix of dto_kkt_assemble
 * (dimension N = num_variables + num_constraint):
 *     [ K   G' ] [ v ]   [ r ]        G: nb x N (border rows, 1 <= nb <= 16)
 *     [ G   C  ] [ y ] = [ s ]        C: nb x nb, dense; only its symmetric part is used; may be absent (zero)
 * by the Schur complement on the border: Y = K^-1 G' (one dto_kkt_solve_multi of nb right-hand sides), S = C - G Y,
 * v0 = K^-1 r, y = S^-1 (s - Y' r) (G K^-1 r = Y' r because K is symmetric), v = v0 - Y y.  dto_kkt_border_factor does
 * everything that does not depend on (r, s) and keeps Y and the pivoted LU of S with the handle; dto_kkt_border_solve is one
 * dto_kkt_solve plus two passes over Y, any number of times per border.
 * dto_kkt_border_factor -- row j of instance b is row b * nb + j of g_x ([B * nb][ldgx], num_variables entries) and of g_c
 * ([B * nb][ldgc], num_constraint entries; NULL = zero).  c: [B][ldc] with ldc >= nb * nb, row-major nb x nb, of which
 * (C + C')/2 is used; NULL = zero block.  All three are DEVICE arrays; they have been consumed when the call returns (it waits
 * for the stream) and may change afterwards.  schur_negdef (HOST [B], may be NULL): 1 when -S is positive definite (K
 * quasi-definite and S negative definite is the inertia an interior-point caller wants), else 0.  schur_singular (HOST [B],
 * may be NULL): 1 when the pivoted LU of S met a zero pivot; solves of that instance then return NaN in every entry of
 * sol_x, sol_c and sol_b, the other instances are not affected.
 * dto_kkt_border_solve -- one bordered right-hand side per instance: rhs_x / rhs_c / sol_x / sol_c as for dto_kkt_solve,
 * rhs_b / sol_b are [B][ld] with nb entries.  The solutions must not overlap the right-hand sides.
 * State: dto_kkt_assemble, dto_kkt_factor, dto_kkt_border_factor, then dto_kkt_border_solve any number of times.
 * dto_kkt_border_factor before dto_kkt_assemble or (tile path) before dto_kkt_factor fails with DTO_ERR_INVALID and the
 * messages of dto_kkt_solve_multi; dto_kkt_border_solve without a border in place fails with DTO_ERR_INVALID.  A new
 * dto_kkt_assemble or dto_kkt_factor invalidates the border, and so does everything that takes the factor storage
 * (dto_kkt_step_batch, the solver entry points): dto_kkt_border_factor has to be called again.  nb < 1, a null g_x, rhs_b or
 * sol_b and a leading dimension below its row length are DTO_ERR_INVALID; nb > 16 is DTO_ERR_UNSUPPORTED (one panel of
 * right-hand sides is the limit).  A refused call writes nothing.  dto_kkt_solve, dto_kkt_solve_multi, dto_kkt_multiply and
 * dto_kkt_solve_refined may be interleaved freely with border solves on one factorisation and return what they return
 * without a border, bit for bit.  Results are bit-identical from run to run (no atomic sums; G Y is summed in chunks of
 * 2048 entries of a row, DTO_BORDER_GRAM_CHUNK in the environment of a dto_kkt_border_factor call sets another length).
 * Workspace kept with the handle, allocated by dto_kkt_border_factor (sizes are reported if that fails): the panel of border
 * rows and Y, B x nb x N doubles each, v0 with B x N, the partial products of G Y (256 doubles per 2048 entries of a row and
 * instance) and a few hundred doubles per instance for the LU, the pivots and y.  Per path:
 * - tile path: Y comes from the panel substitution (the stored records are read once forward and once backward for all nb
 *   rows), v0 from the single substitution; nothing is factorised again;
 * - lane-per-instance path: no factor is stored there, so dto_kkt_border_factor costs nb sweeps (dto_kkt_solve_multi) and
 *   dto_kkt_border_solve one sweep (dto_kkt_solve) plus the two passes over Y -- against nb + 1 sweeps per right-hand side
 *   without it.  As dto_kkt_solve on that path, the calls need dto_kkt_assemble only. */
int dto_kkt_border_factor(dto_problem* p, int64_t nb, const double* g_x, int64_t ldgx, const double* g_c, int64_t ldgc,
                          const double* c, int64_t ldc, int32_t* schur_negdef, int32_t* schur_singular, void* stream);
int dto_kkt_border_solve(dto_problem* p, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc,
                         const double* rhs_b, int64_t ldrb, double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc,
                         double* sol_b, int64_t ldsb, void* stream);

/* The bordered matrix as an operator, and bordered solves refined against it (tile path).  M = [K G'; G sym(C)] with the border of
 * the last dto_kkt_border_factor: K as dto_kkt_multiply applies it, G the kept panel of border rows, sym(C) = (C + C')/2 (zero
 * without c).  All arrays are DEVICE arrays, [B][ld], laid out as for dto_kkt_border_solve; outputs must not overlap inputs.
 * dto_kkt_border_multiply -- [out_x; out_c; out_b] = M [v_x; v_c; v_b].  out_x / out_c first receive K v (dto_kkt_multiply's
 * kernel), then one pass over the panel -- nb x N doubles per instance, every entry read once -- adds G' v_b to them and forms
 * G v; out_b = G v + sym(C) v_b.  No factor record and no Schur complement is read: the product of an instance whose Schur
 * complement is singular is finite.
 * dto_kkt_border_solve_refined -- dto_kkt_border_solve, then `passes` (0 .. 4) rounds of (rho, sigma) = (r, s) - M (v, y),
 * (dv, dy) = dto_kkt_border_solve of it, (v, y) += (dv, dy): fixed-precision iterative refinement, residuals in working
 * precision.  It repairs what an inexact K^-1 (a factorisation of wrong inertia, delta_w = 0) leaves in Y, S and v0, as
 * dto_kkt_solve_refined does for plain solves; nothing is factorised again.  passes = 0 without resid is dto_kkt_border_solve,
 * bit for bit.  resid: DEVICE [B] or NULL; when given, one further product writes max |(r, s) - M (v, y)| over the N + nb rows of
 * the returned solution, formed element by element as rhs - product with the product exactly as dto_kkt_border_multiply computes
 * it.  An instance with a singular Schur complement returns NaN in every solution entry and NaN in resid; the others are not
 * affected.
 * State: both need a valid border (dto_kkt_assemble, dto_kkt_factor, dto_kkt_border_factor) -- the product too, that is where G
 * and C live -- and fail with DTO_ERR_INVALID and the message of dto_kkt_border_solve without one; whatever invalidates the
 * border (see above) invalidates them.  Errors, in this order: no border; passes outside 0..4; a null vector; a leading dimension
 * below its row length (nb for v_b / out_b / rhs_b / sol_b) -- all DTO_ERR_INVALID.  A refused call writes nothing.
 * Results are bit-identical from run to run (no atomic sums) and do not depend on the callers' leading dimensions; padding is
 * neither read nor written.  The panel is summed in the chunks dto_kkt_border_factor used (DTO_BORDER_GRAM_CHUNK at factor time
 * sets both).  The calls may be mixed freely with dto_kkt_solve, _solve_multi, _multiply, _solve_refined and _border_solve on one
 * factorisation; all of those return what they return without them, bit for bit.
 * Workspace kept with the handle: dto_kkt_border_factor keeps sym(C) (256 doubles per instance) and 16 doubles per chunk and
 * instance for the partial G v; dto_kkt_border_solve_refined allocates two arrays of B x (N + 16) doubles at its first call with
 * passes > 0 or resid (the size is reported if that fails); all freed with the handle.  Per path:
 * - tile path: as above;
 * - lane-per-instance path: DTO_ERR_UNSUPPORTED ("tile path only": no assembled system is kept there, dto_kkt_multiply is
 *   unsupported too); nothing is written and the border stays usable. */
int dto_kkt_border_multiply(dto_problem* p, const double* v_x, int64_t ldvx, const double* v_c, int64_t ldvc, const double* v_b,
                            int64_t ldvb, double* out_x, int64_t ldox, double* out_c, int64_t ldoc, double* out_b, int64_t ldob,
                            void* stream);
int dto_kkt_border_solve_refined(dto_problem* p, int passes, const double* rhs_x, int64_t ldrx, const double* rhs_c, int64_t ldrc,
                                 const double* rhs_b, int64_t ldrb, double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc,
                                 double* sol_b, int64_t ldsb, double* resid, void* stream);
/* The compact limited-memory BFGS matrix as a border (tile path).  With the pairs (s_j, y_j), oldest first,
 *     B  = sigma I - W M^-1 W',   W = [sigma S, Y],   M = [[sigma S'S, L], [L', -D]]   (L, D: strictly lower part / diagonal of S'Y)
 *     K  = K0 - U M^-1 U',  U = [W; 0]:       K v = b   <=>   [K0 U; U' M] [v; w] = [b; 0]
 * which is dto_kkt_border_factor's system with G = U' (rows sigma s_j, then y_j; zero on the constraint side), C = M.  The call
 * forms the panel and M on the device (M from one Gram pass over the history) and then runs what dto_kkt_border_factor runs;
 * afterwards dto_kkt_border_solve with rhs_b = 0 returns K^-1 r, and dto_kkt_border_multiply / _solve_refined work on the bordered
 * matrix as for any border (2 m border rows).
 * It needs a factorised system (dto_kkt_assemble_first_order, or dto_kkt_assemble, then dto_kkt_factor).  THE CALLER puts sigma on
 * the x-diagonal of that system through dto_kkt_system.sigma_x, beside whatever else it adds there: this call adds only the
 * low-rank part.
 * s, y: DEVICE [B * m][ld], num_variables entries per row, pair j of instance b in row b * m + j.  npairs: HOST [B] or NULL (m
 * everywhere): instance b uses its first npairs[b] pairs; the rows of the others are zero in the panel and their diagonal entries
 * of M are +1 (S block) and -1 (Y block), so the Schur complement stays regular and the expected inertia does not change.
 * sigma: HOST [B], positive.  inertia_ok (HOST [B], may be NULL): 1 when the Schur complement M - U' K0^-1 U has exactly as many
 * negative eigenvalues as M and neither has a numerically zero one (signs from cyclic Jacobi, zero = within 1e-13 of the largest
 * entry) -- with K0 of the right inertia, K then has it too.  schur_singular (HOST [B], may be NULL): as dto_kkt_border_factor.
 * Errors: m < 1, a null s, y or sigma, npairs outside 0..m, a sigma that is not positive and finite, a leading dimension below
 * num_variables: DTO_ERR_INVALID; 2 m > 16: DTO_ERR_UNSUPPORTED (one panel); no assembled or factorised system: the messages of
 * dto_kkt_border_factor; lane-per-instance path: DTO_ERR_UNSUPPORTED ("tile path only").  A refused call writes nothing.  Results are
 * bit-identical from run to run (no atomic sums; both Gram passes are summed in the chunks of dto_kkt_border_factor). */
int dto_kkt_lbfgs_border(dto_problem* p, int64_t m, const double* s, int64_t lds, const double* y, int64_t ldy, const int32_t* npairs,
                         const double* sigma, int32_t* inertia_ok, int32_t* schur_singular, void* stream);
/* The same with nr rows of the caller's beside the compact matrix, in ONE border of nb = 2 m + nr rows (tile path):
 *     [ K0   U    G' ] [ v ]   [ r ]      U' = [sigma S; Y] as above, G: the caller's rows (coupling constraints, say),
 *     [ U'   M    0  ] [ w ] = [ 0 ]      the diagonal block blkdiag(M, C), C the caller's nr x nr block
 *     [ G    0    C  ] [ y ]   [ t ]
 * i.e. [K G'; G C] [v; y] = [r; t] with K = K0 - U M^-1 U'.  g_x / g_c / c: layout and meaning of dto_kkt_border_factor with nb = nr
 * (row j of instance b is row b * nr + j; g_c may be NULL: zero on the constraint side; c is [B][ldc], nr x nr row-major, its
 * symmetric part is used), DEVICE arrays.  One launch appends the rows to the panel behind the history rows, the layout step of M
 * places C beside it; M has the bits dto_kkt_lbfgs_border gives it for the same history.  Afterwards dto_kkt_border_solve,
 * dto_kkt_border_multiply and dto_kkt_border_solve_refined act on the bordered matrix with rhs_b / sol_b of nb entries: the first
 * 2 m belong to the compact part (right-hand side 0), the last nr to the rows.
 * inertia_ok (HOST [B], may be NULL): 1 exactly when the Schur complement blkdiag(M, C) - [U G']' K0^-1 [U G'] has neg(M) + nr negative
 * eigenvalues and neither M nor the Schur complement a numerically zero one (the Jacobi and the 1e-13 rule of dto_kkt_lbfgs_border).
 * Why: the whole matrix has inertia In(K0) + In(Schur) = In(M) + In([K G'; G C]); for K bordered by nr constraint rows to have
 * (num_variables, Ns + nr) given K0 at (num_variables, Ns), the Schur complement needs pos(M) positive and neg(M) + nr negative
 * eigenvalues.  C is not inspected on its own (it is 0 for an equality row with delta_c = 0).
 * Errors: 2 m + nr > 16: DTO_ERR_UNSUPPORTED (one panel); nr < 0, a null g_x or c with nr > 0, ldgx < num_variables,
 * ldgc < num_constraint (with g_c) or ldc < nr * nr: DTO_ERR_INVALID; everything else as dto_kkt_lbfgs_border.  A refused call writes
 * nothing and launches nothing.  nr = 0 is dto_kkt_lbfgs_border, bit for bit.  No atomic sums: results are bit-identical from run to run. */
int dto_kkt_lbfgs_border_rows(dto_problem* p, int64_t m, const double* s, int64_t lds, const double* y, int64_t ldy,
                              const int32_t* npairs, const double* sigma,
                              int64_t nr, const double* g_x, int64_t ldgx, const double* g_c, int64_t ldgc,
                              const double* c, int64_t ldc,
                              int32_t* inertia_ok, int32_t* schur_singular, void* stream);

/* Batched interior-point solve, one independent NLP per instance, same structure, different guesses.
 * x0: DEVICE [B][ldx] initial guesses (what initialize_states!/initialize_controls! set,
 * src/solver.jl:23-39); x_out/mu_out: DEVICE [B][ld*] final accepted iterates (get_trajectory,
 * src/solver.jl:41-43, returns the last *evaluated* point in the reference -- here it is the accepted one);
 * status/iterations: HOST [B] (0 running, 6 cut off by max_cpu_time, 1 converged, 2 max_iter, 3 failed: non-finite iterate,
 * 4 converged to the acceptable level, 5 diverging iterates).
 * Paths by model: lane-per-instance tiles (states <= 16; bounds, inequality rows, per-instance parameters); the tile (MFMA)
 * kernels for 64-state models (variables free, fixed or bounded; no stage constraints, one to four actions, shared or per-instance parameters;
 * 17..63-state models through their 64-state embedding; stepwise, warm-started and shifted solves through the entry points below); a
 * GeneralConstraint whose rows couple several knots is solved through a border (general rows and the rows of stage Constraints
 * equalities or inequalities c <= 0, variables free, fixed or bounded on either side -- the problem's shared bounds, by a
 * primal-dual barrier; shared parameters or dto_batch.params, ldp < num_parameters being
 * DTO_ERR_INVALID before anything is written; warm starts, and the bound multipliers, slacks and barrier parameters as outputs,
 * through dto_solve_batch_warm below; a limited-memory mode on the tile path only, last item below), the
 * filter line-search loop around it
 * driven from the host (dto_kkt_step_batch on such a problem stays the plain Newton step of the bordered system: no barrier
 * terms of the bounds or of inequality rows in it).  All barrier kinds of an instance -- bounds, slacks of inequality general
 * rows, slacks of inequality stage rows -- share one barrier parameter; the multiplier of an inequality row comes back >= 0 in
 * mu_out, the slacks are not returned:
 * - lane-per-instance path: one factorisation and n_g + 1 sweeps per step, the border algebra on the device since round 4
 *   (DTO_BORDER_HOST=1: on the host -- equality rows and free or fixed variables only: bounds, inequality general rows and
 *   inequality stage rows need the device border, DTO_ERR_UNSUPPORTED otherwise, as with more than 16 general rows); the slacks of
 *   inequality stage rows stay on the device, s / nu enters through dto_kkt_system.sigma_c;
 * - tile path (a 64-state model with general rows, or a 17..63-state problem embedded with them): one stored factorisation, one
 *   panel substitution for all n_g rows and one bordered solve per step (dto_kkt_border_factor / dto_kkt_border_solve inside); at
 *   most 16 general rows (more: DTO_ERR_UNSUPPORTED), no stage rows.  dto_solve_batch, dto_solve and dto_kkt_step_batch take such a
 *   problem; dto_solver_begin / begin_warm / iterate / run / shift and dto_solver_set_bounds return DTO_ERR_UNSUPPORTED for it
 *   (the problem's shared bounds; warm starts and shifts: dto_solve_batch_warm / dto_point_shift).  dto_solver_hessian_mode reports DTO_HESSIAN_EXACT (with
 *   DTO_HESSIAN_EXACT asked for, or more than four general rows), kkt_refinement is ignored;
 * - tile path with dto_options.hessian_approximation = DTO_HESSIAN_LBFGS and at most four general rows (none included): the same
 *   host-driven loop, its step a first-order factorisation with the compact L-BFGS matrix (history 6) as a border of 12 rows; the
 *   general rows share that panel (12 + n_g <= 16: dto_kkt_lbfgs_border_rows), their multipliers enter the secant pairs.  The
 *   history lives on the device, 12 x num_variables doubles per instance (the size is reported if the allocation fails).  The
 *   problem's shared bounds, inequality general rows, shared or per-instance parameters, filter line search (no penalty phase); warm
 *   starts with or without the history through dto_solve_batch_warm.  dto_solver_hessian_mode reports DTO_HESSIAN_LBFGS after such a solve. */
int dto_solve_batch(dto_problem* p, const dto_options* opt, const dto_batch* b, double* x_out, int64_t ldxo,
                    double* mu_out, int64_t ldmuo, int32_t* status, int32_t* iterations);

/* The same solve split in three so a caller (bench.py) can time exactly K iterations.  On the tile path (64-state models and the
 * 17..63-state embedding) the state of these entry points is the host-driven loop's: begin = the cold start of dto_solve_batch
 * (which is itself begin + run there, bit for bit), iterate(n) = n outer iterations of the instances still running, resumable;
 * the state stays allocated after the solve until dto_solver_release or a begin with another batch size; max_cpu_time counts
 * from the begin.  There dto_solver_peek has which = 0, 1, 2, 3, 5, 6, dto_solver_scalar the slots the host loop keeps
 * (status, iter, mu, delta_w, alpha, f, theta_inf, dinf and the filter / ladder counters), dto_solver_repack only counts, and
 * dto_solver_launch_op, _trace, _set_partitions, _footprint and _set_engine return DTO_ERR_UNSUPPORTED. */
int dto_solver_begin(dto_problem* p, const dto_options* opt, const dto_batch* b);
/* Warm start for receding-horizon (MPC) re-solves -- what repeated initialize_states!/initialize_controls! + solve! calls
 * (src/solver.jl:23-47) amount to, without re-initialising the interior-point state: the multipliers, bound multipliers, slacks
 * and the barrier parameter of the previous solve of this handle stay on the device.  b->x (DEVICE, may be NULL = keep the
 * final iterate) replaces the primal iterate (e.g. the shifted trajectory), b->params the parameters (e.g. the newly
 * measured state); b->B must equal the previous batch size.  mu0 > 0 resets the barrier parameter, mu0 <= 0 keeps it.
 * Variables with lo == hi go to their bound, the others are pushed into the interior as at a cold start; positive bound
 * multipliers are kept, non-positive ones re-initialised to mu / gap; the filter, the inertia-ladder memory and the iteration
 * counters restart.  Both paths, the tile path included (there: the k_wide_init_warm kernel, per-instance host records reset). */
int dto_solver_begin_warm(dto_problem* p, const dto_options* opt, const dto_batch* b, double mu0);
/* Receding horizon: shift the device-resident iterate of the previous solve forward by `knots` knots -- x_t <- x_{t+k},
 * u_t <- u_{t+k}, dynamics multipliers and bound multipliers with them; the knots that enter at the end of the horizon hold the
 * final state and repeat the last action (the usual MPC warm start).  Stage-constraint multipliers stay with their knots.
 * Follow with dto_solver_begin_warm(x = NULL, params = the newly measured state) and dto_solver_run.  Needs the same state /
 * action dimensions at every knot and knots < horizon - 1.  Tile path: one launch per array (z, multipliers, z_L, z_U), no host
 * round trip; the rows marked by dto_solver_shift_keep_rows keep their multipliers.  Variable bounds do not move: with
 * per-instance bounds (dto_solver_set_bounds) the caller sets those of the new horizon (e.g. the measured first-knot state)
 * before dto_solver_begin_warm. */
int dto_solver_shift(dto_problem* p, int knots, void* stream);
/* Per-instance variable bounds for the batched solver entry points of a tile-path (17..64-state) plugin.
 * lower / upper: DEVICE [B][ldl] / [B][ldu], solver layout (num_variables entries per instance).  Copied on `stream` into
 * storage owned by the handle and checked before the call returns.  They apply to every later dto_solve_batch /
 * dto_solver_begin / dto_solver_begin_warm whose batch has B instances.  A begun state keeps the bounds it was begun with.
 * lower = upper = NULL: back to the problem's shared bounds.
 * Every instance's bounds have the pattern of the problem's own (dto_variable_bounds): a variable is fixed (lo == hi) exactly
 * where the problem's is (its value may differ), a lower / upper bound is finite exactly where the problem's is, lo < hi where
 * the variable is not fixed, no NaN.  So the barrier, the bound multipliers and the identity rows of fixed variables are the
 * problem's; only the values are per instance (e.g. a measured initial state pinned by lo == hi, per-scenario actuator
 * limits).  A violation returns DTO_ERR_INVALID naming the first offending instance and variable and leaves the previous
 * setting in force; a begin whose B differs from the B set here returns DTO_ERR_INVALID.  The lane-per-instance path returns
 * DTO_ERR_UNSUPPORTED (per-instance values enter there through parameters in stage rows). */
int dto_solver_set_bounds(dto_problem* p, int64_t B, const double* lower, int64_t ldl, const double* upper, int64_t ldu,
                          void* stream);
/* Tile path: keep[i] != 0 (HOST [n], n = num_constraint) marks constraint row i as one whose multiplier stays with its knot in
 * dto_solver_shift -- the stage rows that a 17..63-state problem carries as dynamics rows of its 64-state embedding (the Python
 * Solver sets them from its embedding before every shift).  keep = NULL clears the marks.  The lane-per-instance path keeps its
 * stage rows by itself and ignores the marks. */
int dto_solver_shift_keep_rows(dto_problem* p, const int32_t* keep, int64_t n);

/* ---- warm-started solves of the bordered path from a point the CALLER owns -----------------------------------------------
 * A primal-dual point of B instances.  DEVICE arrays of the caller's, instance-major, each with its own leading dimension:
 *   x       [B][ldx   >= num_variables]
 *   mu      [B][ldmu  >= num_constraint]  constraint multipliers in the solver's row order (what dto_solve_batch writes to mu_out)
 *   zl, zu  [B][ldzl / ldzu >= num_variables]  bound multipliers; 0 where a side is infinite or the variable is fixed.  Both NULL
 *           or both set
 *   slack   [B][ldslack >= num_constraint]  slacks of the inequality rows (c + s = 0), stage and general; entries of equality rows
 *           are not read and are written as 0.  May be NULL
 *   barrier [B]  the barrier parameter of each instance.  May be NULL
 *   qn_s, qn_y  [B * 6][ldqs / ldqy >= num_variables]  the secant pairs of the limited-memory mode, pair j of instance b in row 6 b + j,
 *           oldest first (the layout dto_kkt_lbfgs_border takes, m = 6); qn_npairs (int32) and qn_sigma: HOST [B], like status and
 *           iterations.  All four NULL or all four set. */
typedef struct dto_point {
  double* x;
  int64_t ldx;
  double* mu;
  int64_t ldmu;
  double* zl;
  int64_t ldzl;
  double* zu;
  int64_t ldzu;
  double* slack;
  int64_t ldslack;
  double* barrier;
  double* qn_s;
  int64_t ldqs;
  double* qn_y;
  int64_t ldqy;
  int32_t* qn_npairs;
  double* qn_sigma;
} dto_point;
/* dto_solve_batch for the problems its host-driven bordered loop solves -- GeneralConstraint rows that stay on the border (lane
 * path and tile path), and a tile-path problem with dto_options.hessian_approximation = DTO_HESSIAN_LBFGS and at most four general
 * rows -- started from `start` and returning the whole point in `end`.  Nothing of the solve stays in the handle: the caller keeps
 * the point between calls, may shift it (dto_point_shift) and may rotate several batches over one handle.  Any other problem:
 * DTO_ERR_UNSUPPORTED (the ordinary lane and tile loops have dto_solver_begin_warm); the refusals of dto_solve_batch otherwise.
 * b: B, params / ldp, stream as for dto_solve_batch; b->x is the guess of a cold start and is not read with start != NULL.
 * end: x is required, every other array is written where it is set (mu, zl / zu, slack, barrier, the history; without a barrier
 *   zl = zu = 0, barrier = 0; without the limited-memory mode the history comes back empty: npairs 0, sigma 1).  start and end
 *   may be the same point.
 * start == NULL: the cold start of dto_solve_batch, the same launches and the same bits in end->x / end->mu.
 * start != NULL: x is required (mu == NULL: zero multipliers); the rules of dto_solver_begin_warm --
 *   - a variable with lo == hi goes to its value; every other one is pushed inside its bounds by bound_push / bound_frac as at a
 *     cold start;
 *   - entries of zl / zu that are > 0 are kept; the others, and all of them with zl == NULL, become barrier / gap;
 *   - the barrier parameter of instance i is start->barrier[i] where that is > 0, else dto_options.mu_init; it is ignored when the
 *     problem has no finite bound and no inequality row;
 *   - mu of the equality rows is taken as given; an inequality row keeps (slack, mu) when both are > 0, otherwise
 *     s = max(-c(x), bound_push max(1, |c(x)|)) and mu = barrier / s;
 *   - the filter, the inertia-ladder memory, the iteration count and the status of every instance start afresh;
 *   - the history is used when given (rows of pairs beyond qn_npairs[i] are ignored; the skip and pending counters restart),
 *     else it starts empty;
 *   - the loop itself is dto_solve_batch's: it tests convergence before its first step, so a converged point handed back returns
 *     as it is with 0 iterations.
 * DTO_ERR_INVALID before anything is written: B < 1, a NULL end or end->x (or start->x), a leading dimension below its row length,
 * only one of zl / zu, a partial history, qn_npairs outside 0..6 or a qn_sigma that is not positive and finite. */
int dto_solve_batch_warm(dto_problem* p, const dto_options* opt, const dto_batch* b, const dto_point* start, dto_point* end,
                         int32_t* status, int32_t* iterations);
/* dto_solver_shift on a caller's point: block t of x, zl and zu (n_x + n_u variables a knot) and of the dynamics rows of mu (n_x a
 * knot) takes block min(t + knots, T - 2); the final state is held, the last action repeats.  Multipliers and slacks of stage rows,
 * rows marked by dto_solver_shift_keep_rows, the general rows behind them and `barrier` stay; each of the 12 history vectors of an
 * instance shifts like x.  Arrays that are NULL are skipped (x is required).  Any problem with the same state / action dimensions
 * at every knot, GeneralConstraint rows included; knots >= T - 1: DTO_ERR_INVALID, varying dimensions: DTO_ERR_UNSUPPORTED, the
 * argument checks of dto_solve_batch_warm.  Out of place through one scratch buffer that is released before the call returns (it
 * waits for `stream`); nothing is kept in the handle. */
int dto_point_shift(dto_problem* p, int64_t B, dto_point* pt, int knots, void* stream);
/* Move the instances that are still running to the leading tiles of the batch so that the following iterations only cover
 * tiles with work (a batch otherwise pays for every tile until its last lane has terminated); results keep coming back in
 * the caller's instance order.  dto_solver_run / dto_solve_batch do this by themselves; a caller that drives
 * dto_solver_iterate directly (bench.py) calls it between slices.  *num_running (may be NULL) = instances still iterating. */
int dto_solver_repack(dto_problem* p, int* num_running, void* stream);
/* iterate the begun batch to termination (the polling loop of dto_solve_batch) and hand the results over */
int dto_solver_run(dto_problem* p, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, int32_t* status,
                   int32_t* iterations, void* stream);
int dto_solver_iterate(dto_problem* p, int n_iterations, void* stream);
/* per-instance scalars, HOST [B] each, any may be NULL */
int dto_solver_stats(dto_problem* p, int32_t* status, int32_t* iterations, double* objective, double* constr_viol,
                     double* dual_inf, double* mu, double* delta_w, double* alpha);
/* diagnostic: launch ONE kernel of the iteration (enum dto_kkt_op in csrc/dto_kkt_kernels.hpp: 3 EVAL, 4 CONV,
 * 5 FACTOR_SOLVE, 6 LINESEARCH, 7 LS_REDUCE, 8 UPDATE, 9..12 the kernels behind FACTOR_SOLVE, 15 UPDATE_EVAL: UPDATE of one
 * iteration and EVAL of the next in one pass -- it writes into the second iterate buffers and swaps them: use it an even
 * number of times between calls that touch finished tiles) so a caller can time it with events on `stream`.
 * dto_solver_iterate itself runs UPDATE_EVAL wherever it can and, for batches of more than 1 024 tiles (65 536 instances), the
 * back substitutions of finished tiles on a second low-priority stream next to the forward launch (joined before it
 * returns to the caller's stream order); both bit-identical to the plain sequence (DTO_FUSE_UPDATE=0, DTO_OVERLAP_SWEEPS=0).
 * From 2 048 tiles on (256 compute units) the sequential forward sweep gives a wavefront a group of up to four adjacent tiles and runs their
 * inertia-correction rounds on the packed lanes that need one; bit-identical to one tile per wavefront (DTO_FWD_GROUP=1). */
int dto_solver_launch_op(dto_problem* p, int op, void* stream);
/* chunks of the time-partitioned block-tridiagonal factorisation: 0 = chosen from the batch size so that
 * tiles x chunks fills the GPU's SIMDs; 1 = plain sequential sweep.  Takes effect at the next begin/step. */
int dto_solver_set_partitions(dto_problem* p, int partitions);
int dto_solver_partitions(dto_problem* p, int* partitions);
/* 1 if dto_solver_iterate runs UPDATE of one iteration and EVAL of the next as one pass for the batch begun last (the second
 * iterate buffers could be allocated: an eighth of the device stays free after them, DTO_FUSE_RESERVE_GB overrides; and
 * DTO_FUSE_UPDATE is not 0), else 0: the two-kernel sequence, bit-identical */
int dto_solver_fused_update(dto_problem* p, int* fused);
/* Engine behind dto_solver_begin / dto_solve_batch: 0 = automatic, 1 = SoA tiles (64 instances share a wavefront for the whole
 * solve; time-partitioned sweeps for small batches), 2 = instance-major (csrc/dto_im_kernels.hpp: per-instance stage records,
 * work lists, one factorisation attempt per instance and pass; exact-Hessian models).  Automatic = SoA tiles (the faster one
 * on every measured workload) unless the environment says DTO_ENGINE=im.  Takes effect at the next
 * dto_solver_begin.  dto_solver_engine reports the engine of the batch begun last (1 or 2). */
int dto_solver_set_engine(dto_problem* p, int engine);
/* free the device state of the solver entry points (both engines); the next dto_solver_begin allocates again */
int dto_solver_release(dto_problem* p);
int dto_solver_engine(dto_problem* p, int* engine);
/* per-instance footprint of the solver state in doubles: stage records, factors (for roofline arithmetic) */
int dto_solver_footprint(dto_problem* p, int64_t* record_doubles, int64_t* factor_doubles, int64_t* num_slacks,
                         int* factor_rounds /* (k_kkt_fwd, k_kkt_sep) launch pairs per iteration */);
/* diagnostic: one per-instance scalar slot of the device state (enum dto_scal in csrc/dto_kkt_kernels.hpp), HOST [B] */
int dto_solver_scalar(dto_problem* p, int slot, double* out);
/* diagnostic: one vector of the device state, instance-major into DEVICE out[B][ld].  which: 0 z, 1 multipliers, 2 dz,
 * 3 d multipliers, 5 z_L, 6 z_U (bound multipliers, [num_variables]), 7 slacks, 8 slack multipliers, 9 d slacks (one per
 * inequality row, in stage order).  Used by the tests that re-derive the interior-point step in numpy. */
int dto_solver_peek(dto_problem* p, int which, double* out, int64_t ld, void* stream);
int dto_solver_end(dto_problem* p, double* x_out, int64_t ldxo, double* mu_out, int64_t ldmuo, void* stream);
/* What stood in for the Hessian of the Lagrangian in the solve / batch begun last on this handle: DTO_HESSIAN_EXACT,
 * DTO_HESSIAN_LBFGS or DTO_HESSIAN_SR1_BLOCKS -- a caller that asked for DTO_HESSIAN_LBFGS on a path without that mode reads
 * here what it got (-1: nothing solved yet). */
int dto_solver_hessian_mode(dto_problem* p, int* mode);
/* Diagnostic: time every kernel launch of the solver entry points (dto_solver_iterate, dto_solver_launch_op, dto_solver_run ...)
 * with a HIP event pair on the stream the kernel is launched on -- the caller's, or the library's low-priority stream for the
 * early back substitutions.  on = 1 clears the records and starts, on = 0 stops.  dto_solver_trace_read synchronises the device
 * and returns, launch by launch in issue order: the op (enum dto_kkt_op in csrc/dto_kkt_kernels.hpp; FACTOR_SOLVE = 5 covers the
 * kernels behind it when they are not launched one by one), the iteration index since the trace was switched on, the start
 * relative to the first traced launch and the duration in milliseconds.  HOST arrays of `capacity` entries (any may be NULL);
 * *count = launches recorded (may exceed capacity).  bench.py uses it to report per-kernel times of the iterations it timed. */
int dto_solver_trace(dto_problem* p, int on);
int dto_solver_trace_read(dto_problem* p, int32_t* op, int32_t* iteration, double* start_ms, double* duration_ms, int64_t capacity,
                          int64_t* count);

/* single instance, HOST pointers: solve!(solver) (src/solver.jl:45-47) */
int dto_solve(dto_problem* p, const dto_options* opt, const double* x0, double* x, double* mu, int32_t* status,
              int32_t* iterations);

/* device memory helpers so a host language without a HIP binding can stay on this ABI */
int dto_device_alloc(void** ptr, int64_t bytes);
int dto_device_free(void* ptr);
int dto_copy_to_device(void* dst, const void* src, int64_t bytes);
int dto_copy_to_host(void* dst, const void* src, int64_t bytes);
int dto_device_synchronize(void);
int dto_device_count(int* n);
/* instance sharding across ranks (one process per GPU): contiguous block [first, first + count) of `total` for `rank` */
int dto_shard_range(int64_t total, int rank, int world, int64_t* first, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* DTO_H */

// Problem handle behind the opaque `dto_problem*` of include/dto.h.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "dto_layout.hpp"
#include "dto_model_plugin.h"

namespace dto {

int set_error(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

// The one owner of device memory in the runtime library: a move-only pointer + element count that frees in its destructor.
// alloc / alloc_zeroed / grow release what is held BEFORE they allocate (the lane state is tens of gigabytes at the bench batch:
// old and new must never exist together) and never keep the contents; after a failure the buffer is empty and the error is
// returned.  Converts to T* so that argument structs and kernel launches read as with a raw pointer.
template <class T>
class DevBuf {
  T* p_ = nullptr;
  size_t n_ = 0;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {   // (every hipFree is a device synchronisation: none for an empty buffer)
    if (p_) (void)hipFree(p_);
    p_ = nullptr; n_ = 0;
  }
  hipError_t alloc(size_t n) {   // max(1, n) elements, not initialised
    reset();
    n = n ? n : 1;
    const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr; else n_ = n;
    return e;
  }
  hipError_t alloc_zeroed(size_t n) {   // ... zero-filled on the null stream
    hipError_t e = alloc(n);
    if (e == hipSuccess && (e = hipMemset(p_, 0, n_ * sizeof(T))) != hipSuccess) reset();
    return e;
  }
  hipError_t grow(size_t n) { return n_ >= n ? hipSuccess : alloc(n); }   // no-op while n elements fit
  size_t size() const { return n_; }   // elements allocated
  operator T*() const { return p_; }
};

struct SolverState;  // dto_solver.cpp
struct ImState;      // dto_solver.cpp: instance-major engine
struct WideState;    // dto_solver.cpp: solver state of the tile (MFMA) path
struct WideKkt;      // dto_solver.cpp: tile path, the linear solver alone (dto_kkt_assemble / factor / solve)
struct KktBorder;    // dto_solver.cpp: workspace of dto_kkt_border_factor / dto_kkt_border_solve

// dto_solver_trace: a HIP event pair around every kernel launch of the solver entry points, on the stream the kernel is launched
// on (the caller's, or the low-priority one of the early back substitutions) -- so that a caller can report what each kernel
// took INSIDE the region it timed instead of replaying the launches afterwards.  Events are pooled; nothing is synchronised
// until the trace is read.
struct LaunchTrace {
  struct Rec { int op, iteration, e0, e1; };
  bool on = false;
  int iteration = 0;                 // iterations of dto_solver_iterate since the trace was switched on
  std::vector<hipEvent_t> pool;      // events created so far (re-used by the next trace)
  size_t used = 0;
  std::vector<Rec> recs;
  static constexpr size_t MAX_RECS = 1u << 18;
  int take() {
    if (used == pool.size()) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return -1;
      pool.push_back(e);
    }
    return (int)used++;
  }
  void clear() { used = 0; recs.clear(); iteration = 0; }
  ~LaunchTrace() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
};

struct Problem {
  void* dl = nullptr;
  const dto_model_vtable* vt = nullptr;
  Layout L;
  // device tables
  bool dev_ready = false;
  DevBuf<int> d_kind, d_zoff, d_woff, d_cdoff, d_ccoff, d_jdoff, d_jcoff, d_hoff;
  DevBuf<int> d_hmap_cost, d_hmap_dyn_own, d_hmap_dyn_next, d_hmap_con;
  DevBuf<double> d_params;
  // single-instance staging for host-pointer callbacks
  DevBuf<double> d_x1, d_mu1, d_out1;
  DevBuf<double> d_scratch;
  hipStream_t stream = nullptr;
  // the solver states are incomplete types outside dto_solver.cpp: raw pointers, deleted by free_solver()
  SolverState* solver = nullptr;
  ImState* im = nullptr;
  WideState* wide = nullptr;   // tile path: iterate, multipliers and host records of the batch begun last
  WideKkt* wide_kkt = nullptr; // tile path: the system assembled last by dto_kkt_assemble; its factor lives in wide_fac
  KktBorder* kkt_border = nullptr;   // both paths: Y = K^-1 G' and the LU of the Schur complement of dto_kkt_border_factor
  DevBuf<int> d_shift_keep;    // dto_solver_shift_keep_rows: [Nc] 1 = the multiplier of this row stays with its knot (empty: none)
  DevBuf<double> d_bnd;        // dto_solver_set_bounds (tile path): per-instance bounds [2][bnd_B][Nz], lower then upper (empty: shared)
  int64_t bnd_B = 0;
  LaunchTrace* trace = nullptr;   // dto_solver_trace
  int hessian_mode_last = -1;     // dto_solver_hessian_mode: what the last solve / begun batch used
  int engine_req = 0;      // dto_solver_set_engine: 0 automatic, 1 SoA tiles, 2 instance-major
  bool im_active = false;  // which engine holds the batch that was begun last
  // factor storage and inertia flags of the wide-stage KKT kernels (wide_fac is shared by dto_kkt_step_batch, the solver and
  // dto_kkt_factor: whoever writes it last owns it, WideKkt::factored says whether that is dto_kkt_factor)
  DevBuf<double> wide_fac;
  DevBuf<int> wide_flags;
  // device workspace of the bordered (multi-knot GeneralConstraint) step, kept between steps (eight hipMalloc /
  // hipFree per Newton step -- every hipFree is a device synchronisation)
  DevBuf<double> border_ws;
  // Jacobian pattern by columns (entries of a column in COO order) for the device-side products of the bordered step
  DevBuf<int> d_csc_ptr, d_csc_k, d_csc_row;
  DevBuf<int> d_var_fixed;   // [Nz] 1 where lo == hi

  // CSR pattern of the KKT matrix in the reference ordering (dto_kkt_csr_structure / dto_kkt_csr_values_batch), built on first use
  std::vector<int64_t> csr_rowptr, csr_col;   // 1-based
  DevBuf<int> d_csr_h, d_csr_j;      // per CSR slot: 0-based index into the Hessian key / Jacobian values, -1 = none
  DevBuf<signed char> d_csr_diag;    // per CSR slot: 1 = primal diagonal (+delta_w), 2 = dual diagonal (-delta_c), 0 = off-diagonal
  int build_kkt_csr();

  int ensure_device();
  int ensure_scratch(int64_t B);
  void fill_args(dto_eval_args& a, int64_t B, const double* z, int64_t ldz, const double* w, int64_t ldw) const;
  int launch(int op, const dto_eval_args& a, hipStream_t s);
  void free_solver();
  ~Problem();
};

}  // namespace dto

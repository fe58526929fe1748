// The step-acceptance rules of Waechter & Biegler's Algorithm A (2006) that the two HOST-driven interior-point loops of
// dto_solver.cpp share -- tile path: wide_outer; bordered path: general_solve_batch.  Plain scalar arithmetic over one small record
// per instance: no HIP call, so tests/host/globalization_main.cpp checks every rule on the CPU.  Each loop keeps what is its own:
// how the trial points are evaluated (and alpha computed) and how the linear system is solved.  The in-kernel iteration has the same
// rules in conv_body / ls_reduce_body / retry_update_t (dto_kkt_kernels.hpp), with the watchdog, the penalty phase and the null
// step on top.  Where the two loops differ ON PURPOSE the difference is written next to the function it touches (list: DESIGN.md
// section 5).
//
// Include after dto_kkt_kernels.hpp (dto_solver_opts, DTO_FILTER_CAP, DTO_LS_TRIALS).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace dto {

// Ipopt's scaled optimality error (Waechter & Biegler 2006, (5)-(6)) and monotone barrier update (7) -- the in-kernel iteration has
// the same expressions in conv_body (the two host loops had drifted apart -- the bordered one left the slack multipliers
// out of s_d and reset theta_max with the filter).  On a decrease of mu the FILTER is reset, theta_max / theta_min stay (Ipopt, step A-3).
struct ErrScale { double sd, sc; };
static inline ErrScale ipopt_scaling(const dto_solver_opts& o, double sum_mult, int64_t n_mult, double sum_bound_mult, int64_t n_bound) {
  ErrScale e;
  e.sd = std::max(o.s_max, (sum_mult + sum_bound_mult) / (double)std::max<int64_t>(1, n_mult + n_bound)) / o.s_max;
  e.sc = n_bound > 0 ? std::max(o.s_max, sum_bound_mult / (double)n_bound) / o.s_max : 1.0;
  return e;
}
static inline double barrier_mu_floor(const dto_solver_opts& o) {
  return std::max(o.mu_target, std::min(o.tol, o.compl_inf_tol) / (o.kappa_eps + 1.0));
}
// mu -> the first value of the monotone sequence at which the barrier problem is NOT yet solved to kappa_eps mu (or the floor);
// err_rest: max(dual infeasibility / s_d, constraint violation); compl_at(mu): complementarity error against mu
// Kept difference: on a moved mu the tile path evaluates the step again in the same pass; the bordered path gives the instance
// alpha = 0 for one round and does not count the iteration.
template <class ComplAt>
static inline double monotone_mu(const dto_solver_opts& o, double mu, double err_rest, double sc, ComplAt&& compl_at) {
  const double mu_floor = barrier_mu_floor(o);
  for (;;) {
    const double emu = std::max(err_rest, compl_at(mu) / sc);
    if (!(emu <= o.kappa_eps * mu) || mu <= mu_floor) break;
    mu = std::max(mu_floor, std::min(o.kappa_mu * mu, std::pow(mu, o.theta_mu)));
  }
  return mu;
}

// filter margins gamma_theta / gamma_phi, exponents of the switching condition s_theta / s_phi, Armijo factor eta_phi
constexpr double G_TH = 1e-5, G_PHI = 1e-8, S_TH = 1.1, S_PHI = 2.3, ETA = 1e-8;

// What the globalisation keeps per instance.  WideInst (tile path) derives from it; the bordered path uses it as it is.
struct GlobInst {
  int status = 0, iter = 0, ls_fail = 0, filter_n = 0;   // filter_n counts augmentations: min(filter_n, DTO_FILTER_CAP) entries are live
  double dlast = 0.0, theta_max = -1.0, theta_min = -1.0;   // last accepted delta_w (ladder memory); filter limits, < 0 = not set yet
  double mu = 0.0;                                          // barrier parameter
  std::vector<double> filt;                                 // (theta, phi) pairs, ring of DTO_FILTER_CAP (sized by the first augmentation)
};

// theta_max / theta_min from the violation of the FIRST iterate; they survive every filter reset
static inline void init_theta_limits(GlobInst& s, double th1) {
  if (s.theta_max < 0.0) { s.theta_max = 1e4 * std::max(1.0, th1); s.theta_min = 1e-4 * std::max(1.0, th1); }
}

// The measures of an iterate the termination ladder reads: objective, l1 and max-norm violation, dual infeasibility, Ipopt's scaled
// error against mu_target and the unscaled complementarity error against mu_target
struct IterMeasures { double f, th1, thinf, dinf, e0, c0; };

// Ipopt's acceptable level at one point (the caller counts consecutive ones in acc_count).  Tile path only.
static inline bool acceptable_point(const dto_solver_opts& o, const IterMeasures& m, double f_last) {
  return o.acceptable_iter > 0 && m.e0 <= o.acceptable_tol && m.dinf <= o.acceptable_dual_inf_tol &&
         m.thinf <= o.acceptable_constr_viol_tol && m.c0 <= o.acceptable_compl_inf_tol &&
         std::fabs(m.f - f_last) / std::max(1.0, std::fabs(m.f)) <= o.acceptable_obj_change_tol;
}
// Termination ladder: non-finite -> 3, converged -> 1, acceptable level held for acceptable_iter points -> 4, max_iter -> 2, else 0.
// Kept difference: the tile path counts acceptable points (acc_count, f_last); the bordered path ignores the acceptable_* options
// and passes acc_count = 0, with which 4 is never returned.
static inline int terminal_status(const dto_solver_opts& o, int iter, const IterMeasures& m, int acc_count) {
  if (!(m.f == m.f) || !(m.th1 == m.th1) || !(m.dinf == m.dinf)) return 3;
  if (m.e0 <= o.tol && m.dinf <= o.dual_inf_tol && m.thinf <= o.constr_viol_tol && m.c0 <= o.compl_inf_tol) return 1;
  if (o.acceptable_iter > 0 && acc_count >= o.acceptable_iter) return 4;
  if (iter >= o.max_iter) return 2;
  return 0;
}

// Algorithm IC, next rung of the delta_w ladder after a factorisation with the wrong inertia.
// Kept differences: the FIRST delta_w of an iteration is each loop's own (tile path: kappa_w_minus * dlast while full_streak < 2,
// floored at delta_w_min; bordered path: 0 unless ls_fail), so is where dlast is recorded (tile path: when a factorisation is
// accepted; bordered path: after the convergence test), and the tile path's Gauss-Newton fallback sits around this call.
static inline double ladder_next(const dto_solver_opts& o, double dw, double dlast) {
  return (dw == 0.0) ? ((dlast == 0.0) ? o.delta_w_init : std::max(o.delta_w_min, o.kappa_w_minus * dlast))
                     : dw * ((dlast == 0.0) ? o.kappa_w_plus_first : o.kappa_w_plus);
}
// first delta_w of the iteration after a failed line search (or a step taken on a matrix of the wrong inertia)
static inline double ladder_after_ls_fail(const dto_solver_opts& o, double dlast) {
  return std::min(o.delta_w_exact_cap, std::max(10.0 * dlast, o.delta_w_init));
}

// A-5.4: is the trial (tk, pk) = (theta, phi) at step size alpha acceptable from the iterate (th0, phi0) with directional derivative
// dphi of the merit?  NaN / theta_max guard; where the switching condition holds and th0 <= theta_min the Armijo inequality,
// elsewhere sufficient decrease against the iterate; then against every live filter entry.  f-type: switching condition + Armijo.
enum TrialVerdict { TRIAL_REJECTED = 0, TRIAL_ACCEPTED = 1, TRIAL_ACCEPTED_FTYPE = 2 };
static inline TrialVerdict trial_acceptable(const GlobInst& s, double th0, double phi0, double dphi, double alpha, double tk, double pk) {
  if (!((tk == tk) && (pk == pk) && tk <= s.theta_max)) return TRIAL_REJECTED;
  const bool sw = dphi < 0.0 && alpha * std::pow(-dphi, S_PHI) > std::pow(th0, S_TH);
  const bool armijo = pk <= phi0 + ETA * alpha * dphi + 1e-13 * std::fabs(phi0);
  const bool ok = (sw && th0 <= s.theta_min) ? armijo : (tk <= (1.0 - G_TH) * th0) || (pk <= phi0 - G_PHI * th0);
  if (!ok) return TRIAL_REJECTED;
  const int nf = std::min(s.filter_n, DTO_FILTER_CAP);
  for (int q = 0; q < nf; ++q) {
    const double tf = s.filt[2 * q], pf = s.filt[2 * q + 1];
    if (!(tk <= (1.0 - G_TH) * tf || pk <= pf - G_PHI * tf)) return TRIAL_REJECTED;
  }
  return sw && armijo ? TRIAL_ACCEPTED_FTYPE : TRIAL_ACCEPTED;
}

// the most feasible trial seen so far (a NaN violation loses against anything); note every evaluated trial, in order of k
struct MostFeasible { int k = 0; double theta = std::numeric_limits<double>::quiet_NaN(); };
static inline void note_most_feasible(MostFeasible& b, int k, double tk) {
  if (tk < b.theta || !(b.theta == b.theta)) { b.k = k; b.theta = tk; }
}
// no trial alpha = amax 2^-k, k < trials, was acceptable: the most feasible one if it lowers the violation, else the shortest
static inline double fallback_alpha(const MostFeasible& b, double th0, double amax, int trials) {
  return amax * std::ldexp(1.0, -((b.theta < th0) ? b.k : trials - 1));
}

// A-7: (1 - gamma_theta) th0, phi0 - gamma_phi th0 into the ring
static inline void filter_augment(GlobInst& s, double th0, double phi0) {
  if ((int)s.filt.size() < 2 * DTO_FILTER_CAP) s.filt.resize(2 * DTO_FILTER_CAP, 0.0);
  const int slot = s.filter_n % DTO_FILTER_CAP;
  s.filt[2 * slot] = (1.0 - G_TH) * th0;
  s.filt[2 * slot + 1] = phi0 - G_PHI * th0;
  s.filter_n++;
}

// End of the line search of one instance: `accepted` is the alpha of the first acceptable trial (ftype: how it was accepted) or
// negative when all `trials` were rejected.  Returns the step to take; a fallback step raises ls_fail, and every step that is not
// f-type augments the filter with the iterate.
// Kept difference, ls_fail after an ACCEPTED trial (ls_fail_if_accepted): 0 on the tile path; on the bordered path 1 when the step
// came from a matrix whose inertia was never corrected (okv == 0).
static inline double finish_line_search(GlobInst& s, double accepted, bool ftype, const MostFeasible& b, double th0, double phi0,
                                        double amax, int trials, int ls_fail_if_accepted) {
  const bool fallback = accepted < 0.0;
  s.ls_fail = fallback ? 1 : ls_fail_if_accepted;
  if (fallback || !ftype) filter_augment(s, th0, phi0);
  return fallback ? fallback_alpha(b, th0, amax, trials) : accepted;
}

}  // namespace dto

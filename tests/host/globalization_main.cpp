// The step-acceptance rules of csrc/dto_host_globalization.hpp on the CPU (tests/test_host_globalization.py builds this without device
// code and runs it under the address and undefined-behaviour sanitizers).  No HIP function is called.  Every expected value below
// is worked out by hand from Waechter & Biegler's Algorithm A and the option values of default_opts (csrc/dto_solver.cpp), never
// taken from the functions under test.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "dto_kkt_kernels.hpp"
#include "dto_host_globalization.hpp"

using namespace dto;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #c);                \
      return 1;                                                    \
    }                                                              \
  } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-14 * std::fabs(b); }

// dto_options_default + default_opts, the fields the rules read
static dto_solver_opts options() {
  dto_solver_opts o;
  memset(&o, 0, sizeof(o));
  o.tol = 1e-6; o.s_max = 100.0; o.dual_inf_tol = 1.0; o.constr_viol_tol = 1e-3; o.compl_inf_tol = 1e-3; o.max_iter = 1000;
  o.acceptable_tol = 1e-6; o.acceptable_iter = 15; o.acceptable_dual_inf_tol = 1e10; o.acceptable_constr_viol_tol = 1e-2;
  o.acceptable_compl_inf_tol = 1e-2; o.acceptable_obj_change_tol = 1e-5;
  o.mu_target = 1e-4; o.mu_init = 0.1; o.kappa_eps = 10.0; o.kappa_mu = 0.2; o.theta_mu = 1.5;
  o.delta_w_init = 1e-4; o.delta_w_min = 1e-20; o.delta_w_max = 1e20;
  o.kappa_w_minus = 1.0 / 3.0; o.kappa_w_plus = 8.0; o.kappa_w_plus_first = 100.0; o.delta_w_exact_cap = 100.0;
  return o;
}

static GlobInst instance() {   // theta_max = 1e4, theta_min = 1e-4: first iterate with theta <= 1
  GlobInst s;
  init_theta_limits(s, 0.5);
  return s;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const dto_solver_opts o = options();

  {  // theta_max = 1e4 max(1, theta), theta_min = 1e-4 max(1, theta), set once
    GlobInst s;
    CHECK(s.theta_max < 0.0 && s.status == 0 && s.iter == 0 && s.filter_n == 0 && s.ls_fail == 0);
    init_theta_limits(s, 20.0);
    CHECK(near(s.theta_max, 2e5) && near(s.theta_min, 2e-3));
    init_theta_limits(s, 500.0);
    CHECK(near(s.theta_max, 2e5) && near(s.theta_min, 2e-3));
    s = instance();
    CHECK(near(s.theta_max, 1e4) && near(s.theta_min, 1e-4));
  }
  {  // 1: NaN theta / NaN phi; 2: theta above theta_max, however much phi improves
    const GlobInst s = instance();
    CHECK(trial_acceptable(s, 1.0, 10.0, -1.0, 1.0, nan, 0.0) == TRIAL_REJECTED);
    CHECK(trial_acceptable(s, 1.0, 10.0, -1.0, 1.0, 0.5, nan) == TRIAL_REJECTED);
    CHECK(trial_acceptable(s, 1.0, 10.0, -1.0, 1.0, 2e4, -100.0) == TRIAL_REJECTED);
    CHECK(trial_acceptable(s, 1.0, 10.0, -1.0, 1.0, 0.5, -100.0) != TRIAL_REJECTED);
  }
  {  // 3: dphi = -1, alpha = 1: alpha (-dphi)^2.3 = 1 > th0^1.1 for th0 = 1e-5 and 1e-3 -- the switching condition holds.
     //    Armijo: phi <= 10 - 1e-8 + 1e-12.  phi = 10 - 1e-6 passes it, phi = 10 - 1e-9 does not.
    const GlobInst s = instance();
    // th0 = 1e-5 <= theta_min: Armijo alone decides -- no decrease of theta needed, and a vanishing theta does not help
    CHECK(trial_acceptable(s, 1e-5, 10.0, -1.0, 1.0, 1e-5, 10.0 - 1e-6) == TRIAL_ACCEPTED_FTYPE);
    CHECK(trial_acceptable(s, 1e-5, 10.0, -1.0, 1.0, 0.0, 10.0 - 1e-9) == TRIAL_REJECTED);
    // th0 = 1e-3 > theta_min: sufficient decrease decides (theta -> 0 passes), f-type only with Armijo
    CHECK(trial_acceptable(s, 1e-3, 10.0, -1.0, 1.0, 0.0, 10.0 - 1e-9) == TRIAL_ACCEPTED);
    CHECK(trial_acceptable(s, 1e-3, 10.0, -1.0, 1.0, 0.0, 10.0 - 1e-6) == TRIAL_ACCEPTED_FTYPE);
    // ... and neither measure decreasing enough is rejected: theta stays, phi <= 10 - 1e-11 fails for phi = 10
    CHECK(trial_acceptable(s, 1e-3, 10.0, -1.0, 1.0, 1e-3, 10.0) == TRIAL_REJECTED);
    // a short step does not switch: alpha = 1e-5 < th0^1.1 = 4.0e-5 at th0 = 1e-4 = theta_min, so sufficient decrease decides and
    // nothing is f-type, Armijo or not
    CHECK(trial_acceptable(s, 1e-4, 10.0, -1.0, 1e-5, 0.0, 10.0 - 1e-6) == TRIAL_ACCEPTED);
  }
  {  // 4: dphi >= 0 never switches: th0 <= theta_min, Armijo true (10 - 1e-6 <= 10 + 1e-8 ...), yet judged by sufficient decrease
    const GlobInst s = instance();
    for (double dphi : {0.0, 1.0}) {
      CHECK(trial_acceptable(s, 1e-5, 10.0, dphi, 1.0, 0.0, 10.0 - 1e-6) == TRIAL_ACCEPTED);
      CHECK(trial_acceptable(s, 1e-5, 10.0, dphi, 1.0, 1e-5, 10.0 - 1e-15) == TRIAL_REJECTED);   // phi <= 10 - 1e-13 fails
    }
  }
  {  // 5: passes against the iterate (theta 0.6 <= 0.99999), dominated by the filter entry (0.5, 5): 0.6 > 0.499995 and 6 > 5 - 5e-9
    GlobInst s = instance();
    s.filt.assign(2 * DTO_FILTER_CAP, 0.0);
    s.filt[0] = 0.5; s.filt[1] = 5.0; s.filter_n = 1;
    CHECK(trial_acceptable(s, 1.0, 10.0, 1.0, 1.0, 0.6, 6.0) == TRIAL_REJECTED);
    CHECK(trial_acceptable(s, 1.0, 10.0, 1.0, 1.0, 0.6, 4.9) == TRIAL_ACCEPTED);    // phi below the entry's
    CHECK(trial_acceptable(s, 1.0, 10.0, 1.0, 1.0, 0.4, 6.0) == TRIAL_ACCEPTED);    // theta below the entry's
    s.filter_n = 0;
    CHECK(trial_acceptable(s, 1.0, 10.0, 1.0, 1.0, 0.6, 6.0) == TRIAL_ACCEPTED);
  }
  {  // 6: the entry is ((1 - 1e-5) th0, phi0 - 1e-8 th0) at slot filter_n % CAP
    GlobInst s = instance();
    filter_augment(s, 2.0, 3.0);
    CHECK(s.filter_n == 1 && (int)s.filt.size() == 2 * DTO_FILTER_CAP && near(s.filt[0], 1.99998) && near(s.filt[1], 2.99999998));
    filter_augment(s, 4.0, -1.0);
    CHECK(s.filter_n == 2 && near(s.filt[2], 3.99996) && near(s.filt[3], -1.00000004) && near(s.filt[0], 1.99998));
  }
  {  // 7: entries k = 0 .. 23: theta about k + 1, phi about 100 - k.  The iterate (1e3, 1e3) with dphi > 0 lets every trial below pass
     //    the test against the iterate itself.
    GlobInst s = instance();
    CHECK(DTO_FILTER_CAP == 24);
    for (int k = 0; k < DTO_FILTER_CAP; ++k) filter_augment(s, k + 1.0, 100.0 - k);
    CHECK(s.filter_n == DTO_FILTER_CAP && near(s.filt[2 * 23], 23.99976) && near(s.filt[2 * 23 + 1], 77.0 - 24e-8));
    // (1, 150) is dominated by slot 0 alone (theta 0.99999, phi 100): every other entry has theta >= 1.99998
    CHECK(trial_acceptable(s, 1e3, 1e3, 1.0, 1.0, 1.0, 150.0) == TRIAL_REJECTED);
    filter_augment(s, 1000.0, -1000.0);   // the 25th: slot 0
    CHECK(s.filter_n == DTO_FILTER_CAP + 1 && (int)s.filt.size() == 2 * DTO_FILTER_CAP);
    CHECK(near(s.filt[0], 999.99) && near(s.filt[1], -1000.00001) && near(s.filt[2], 1.99998));
    CHECK(trial_acceptable(s, 1e3, 1e3, 1.0, 1.0, 1.0, 150.0) == TRIAL_ACCEPTED);
    // (23.9999, 77.5) is dominated by the LAST slot alone (theta 23.99976, phi 77): the others have phi >= 78 or theta 999.99.
    // The scan covers the 24 slots -- and no 25th, which would be a read past the ring
    CHECK(trial_acceptable(s, 1e3, 1e3, 1.0, 1.0, 23.9999, 77.5) == TRIAL_REJECTED);
    s.filt[2 * 23 + 1] = 200.0;
    CHECK(trial_acceptable(s, 1e3, 1e3, 1.0, 1.0, 23.9999, 77.5) == TRIAL_ACCEPTED);
  }
  {  // 8: an f-type acceptance does not augment; any other accepted step does; ls_fail is what the caller asks for
    GlobInst s = instance();
    const MostFeasible none;
    s.ls_fail = 1;
    CHECK(finish_line_search(s, 0.5, true, none, 1.0, 10.0, 1.0, DTO_LS_TRIALS, 0) == 0.5 && s.filter_n == 0 && s.ls_fail == 0);
    CHECK(finish_line_search(s, 0.25, true, none, 1.0, 10.0, 1.0, DTO_LS_TRIALS, 1) == 0.25 && s.filter_n == 0 && s.ls_fail == 1);
    CHECK(finish_line_search(s, 0.5, false, none, 1.0, 10.0, 1.0, DTO_LS_TRIALS, 0) == 0.5 && s.filter_n == 1 && s.ls_fail == 0);
    CHECK(near(s.filt[0], 0.99999) && near(s.filt[1], 9.99999999));
  }
  {  // 9 - 11: every trial rejected, eight trials from amax = 0.8 at th0 = 1
    CHECK(DTO_LS_TRIALS == 8);
    const double thA[8] = {3.0, 2.0, 0.7, 0.9, 1.5, 1.5, 1.5, 1.5};       // A: the most feasible one, k* = 2, lowers theta: 0.8 / 4
    const double thB[8] = {3.0, 2.0, 1.2, 1.9, 1.5, 1.5, 1.5, 1.5};       // B: it does not: the shortest, 0.8 / 128
    const double thN[8] = {nan, nan, nan, nan, nan, nan, nan, nan};       // B: never a number
    const double thM[8] = {nan, 5.0, nan, 0.5, 0.6, nan, 0.5, 2.0};       // A: NaN loses, the FIRST of two equal ones stays: k* = 3
    const struct { const double* th; int k; double alpha; } cases[] = {{thA, 2, 0.2}, {thB, 2, 0.00625}, {thN, 7, 0.00625}, {thM, 3, 0.1}};
    for (const auto& c : cases) {
      MostFeasible best;
      for (int k = 0; k < 8; ++k) note_most_feasible(best, k, c.th[k]);
      CHECK(best.k == c.k);
      CHECK(near(fallback_alpha(best, 1.0, 0.8, 8), c.alpha));
      GlobInst s = instance();
      CHECK(near(finish_line_search(s, -1.0, false, best, 1.0, 10.0, 0.8, 8, 0), c.alpha));
      CHECK(s.ls_fail == 1 && s.filter_n == 1 && near(s.filt[0], 0.99999) && near(s.filt[1], 9.99999999));
      s.ls_fail = 0;   // ... also where the flag says f-type (it is stale when nothing was accepted)
      CHECK(near(finish_line_search(s, -1.0, true, best, 1.0, 10.0, 0.8, 8, 0), c.alpha) && s.ls_fail == 1 && s.filter_n == 2);
    }
  }
  {  // 12, 13: precedence of the ladder; converged: e0 <= 1e-6, dinf <= 1, thinf <= 1e-3, c0 <= 1e-3
    const IterMeasures conv{1.0, 1e-4, 1e-4, 0.5, 1e-7, 1e-4}, far{1.0, 1.0, 1.0, 0.5, 1.0, 0.0};
    IterMeasures bad = conv;
    CHECK(terminal_status(o, 3, far, 0) == 0 && terminal_status(o, 999, far, 0) == 0);
    CHECK(terminal_status(o, 1000, far, 0) == 2 && terminal_status(o, 1000, conv, 0) == 1 && terminal_status(o, 3, conv, 0) == 1);
    bad.f = nan;
    CHECK(terminal_status(o, 1000, bad, 0) == 3);
    bad = conv; bad.th1 = nan;
    CHECK(terminal_status(o, 1000, bad, 0) == 3);
    bad = far; bad.dinf = nan;
    CHECK(terminal_status(o, 0, bad, 0) == 3);
    bad = conv; bad.thinf = 2e-3;   // each tolerance of its own
    CHECK(terminal_status(o, 3, bad, 0) == 0);
    bad = conv; bad.dinf = 2.0;
    CHECK(terminal_status(o, 3, bad, 0) == 0);
    bad = conv; bad.c0 = 2e-3;
    CHECK(terminal_status(o, 3, bad, 0) == 0);
  }
  {  // 14: acceptable_tol = 1e-3 (by hand: the default equals tol).  The point: e0 = 5e-4 -- not converged, acceptable.  The first
     //     point is not acceptable (no previous objective: f_last = 1e300), points 2 .. 16 are: the 16th is the 15th in a row -> 4
    dto_solver_opts oa = o;
    oa.acceptable_tol = 1e-3;
    const IterMeasures m{1.0, 5e-4, 5e-4, 0.1, 5e-4, 0.0};
    int acc = 0, first4 = -1, never = 0;
    double f_last = 1e300;
    for (int point = 1; point <= 40; ++point) {
      acc = acceptable_point(oa, m, f_last) ? acc + 1 : 0;
      f_last = m.f;
      CHECK(acc == point - 1);
      if (first4 < 0 && terminal_status(oa, point, m, acc) == 4) first4 = point;
      never += terminal_status(oa, point, m, 0);   // the bordered path's call
    }
    CHECK(first4 == 16 && never == 0);
    CHECK(terminal_status(oa, 1000, m, 0) == 2 && terminal_status(oa, 1000, m, 15) == 4);   // 4 before 2
    IterMeasures moved = m;                  // an objective that still moves (relative change 1e-4 > 1e-5) breaks the run
    moved.f = 1.0001;
    CHECK(!acceptable_point(oa, moved, 1.0) && acceptable_point(oa, moved, 1.0001));
    moved = m; moved.thinf = 2e-2;           // ... so does a violation above acceptable_constr_viol_tol
    CHECK(!acceptable_point(oa, moved, 1.0));
    oa.acceptable_iter = 0;                  // switched off
    CHECK(!acceptable_point(oa, m, 1.0) && terminal_status(oa, 5, m, 100) == 0);
  }
  {  // 15 - 18: delta_w_init = 1e-4, kappa_w_minus = 1/3, kappa_w_plus_first = 100, kappa_w_plus = 8, delta_w_min = 1e-20
    CHECK(ladder_next(o, 0.0, 0.0) == 1e-4);
    CHECK(near(ladder_next(o, 0.0, 3e-3), 1e-3));
    CHECK(ladder_next(o, 0.0, 1e-21) == 1e-20);          // floored at delta_w_min
    CHECK(near(ladder_next(o, 1e-4, 0.0), 1e-2));
    CHECK(near(ladder_next(o, 1e-3, 1e-3), 8e-3));
    // 19: min(100, max(10 dlast, 1e-4))
    CHECK(ladder_after_ls_fail(o, 0.0) == 1e-4 && ladder_after_ls_fail(o, 1e-6) == 1e-4 && ladder_after_ls_fail(o, 1e9) == 100.0);
    CHECK(near(ladder_after_ls_fail(o, 0.5), 5.0));
  }
  {  // 20: floor = max(1e-4, min(1e-6, 1e-3) / 11) = 1e-4.  Barrier problem solved at every mu: 0.1 -> 0.02 -> 0.02^1.5 = 2.83e-3 ->
     //     1.50e-4 -> the floor.  err = 0.1: solved at 0.1 (0.1 <= 1) and 0.02 (0.1 <= 0.2), not at 2.83e-3.  err = 2: not at 0.1.
    const auto zero = [](double) { return 0.0; };
    CHECK(barrier_mu_floor(o) == 1e-4);
    CHECK(monotone_mu(o, 0.1, 0.0, 1.0, zero) == 1e-4);
    CHECK(monotone_mu(o, 1e-4, 0.0, 1.0, zero) == 1e-4);
    CHECK(near(monotone_mu(o, 0.1, 0.1, 1.0, zero), 0.002828427124746190));
    CHECK(monotone_mu(o, 0.1, 2.0, 1.0, zero) == 0.1);
    // complementarity |s nu - mu| with s nu = 0.05, scaled by s_c = 2: at mu = 0.1 the error is 0.025 <= 1; at 0.02 it is 0.015 <= 0.2;
    // at 2.83e-3 it is 0.0236 <= 0.0283; at 0.02^2.25 = 1.50e-4 it is 0.0249 > 1.5e-3: the barrier problem is not solved there
    CHECK(near(monotone_mu(o, 0.1, 0.0, 2.0, [](double mu) { return std::fabs(0.05 - mu); }), 1.5042412372345574e-4));
    dto_solver_opts ot = o;
    ot.mu_target = 1e-9;
    CHECK(near(barrier_mu_floor(ot), 1e-6 / 11.0));
    // Ipopt's scaling: s_d = max(100, (1000 + 200) / 5) / 100 = 2.4, s_c = max(100, 200 / 1) / 100 = 2; without bound multipliers
    // s_d = max(100, 1000 / 4) / 100 = 2.5, s_c = 1; small multipliers: both 1
    ErrScale e = ipopt_scaling(o, 1000.0, 4, 200.0, 1);
    CHECK(near(e.sd, 2.4) && near(e.sc, 2.0));
    e = ipopt_scaling(o, 1000.0, 4, 0.0, 0);
    CHECK(near(e.sd, 2.5) && e.sc == 1.0);
    e = ipopt_scaling(o, 10.0, 4, 3.0, 2);
    CHECK(e.sd == 1.0 && e.sc == 1.0);
  }
  printf("globalization ok\n");
  return 0;
}

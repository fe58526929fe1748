// The per-entry rules of a warm start from a primal-dual point and of a receding-horizon shift, each written once for the
// kernels that apply them (k_wide_init_warm of the tile solver; k_border_warm_vars, k_border_slack_warm and k_point_shift of the
// bordered loop), for the host side of that loop (the slacks of the general rows) and for tests/host/point_rules_main.cpp, which
// checks them on the CPU.  Plain scalar arithmetic: no HIP call, no other header of the library.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define DTO_HD __host__ __device__
#else
#define DTO_HD
#endif

namespace dto {

// One variable of a warm start (the rules of k_init's warm branch, dto_kkt_kernels.hpp): v the caller's value, [a, c] its bounds
// (a side is finite inside +-1e300), pl / pu the caller's bound multipliers (read with have_z only), m the barrier parameter of
// the instance.  a == c: the variable goes to its value, no multipliers.  Otherwise v is pushed inside by bound_push /
// bound_frac as at a cold start (Waechter & Biegler 2006, section 3.6); with have_z a positive multiplier of a finite side is
// kept, any other becomes m / gap at the pushed point, and a side that is infinite has multiplier 0.
struct WarmVar { double v, zl, zu; };
DTO_HD static inline WarmVar warm_var(double v, double a, double c, bool have_z, double pl_in, double pu_in, double m, double bound_push,
                                      double bound_frac) {
  double l = 0.0, u = 0.0;
  if (a == c) v = a;
  else {
    const bool fl = a > -1e300, fh = c < 1e300;
    if (fl && fh) {
      const double pl = fmin(bound_push * fmax(1.0, fabs(a)), bound_frac * (c - a));
      const double pu = fmin(bound_push * fmax(1.0, fabs(c)), bound_frac * (c - a));
      v = fmin(fmax(v, a + pl), c - pu);
    } else if (fl) v = fmax(v, a + bound_push * fmax(1.0, fabs(a)));
    else if (fh) v = fmin(v, c - bound_push * fmax(1.0, fabs(c)));
    if (have_z) {
      if (fl) l = pl_in > 0.0 ? pl_in : m / (v - a);
      if (fh) u = pu_in > 0.0 ? pu_in : m / (c - v);
    }
  }
  return WarmVar{v, l, u};
}

// One inequality row c(x) + s = 0, s >= 0 of a warm start: the caller's pair (s_in, nu_in) is kept when both are positive;
// otherwise the slack starts at max(-c, bound_push max(1, |c|)) and its multiplier on the central path of the instance's barrier
// parameter m
struct WarmSlack { double s, nu; };
DTO_HD static inline WarmSlack warm_slack(double c, double s_in, double nu_in, double m, double bound_push) {
  if (s_in > 0.0 && nu_in > 0.0) return WarmSlack{s_in, nu_in};
  const double s = fmax(-c, bound_push * fmax(1.0, fabs(c)));
  return WarmSlack{s, m / s};
}

// Receding horizon, the index map of one array of n entries per instance whose first T_blocks * stride entries are T_blocks
// blocks of one knot each (stride = n_x + n_u variables, or n_x dynamics rows): entry j of the shifted array takes entry
// shift_source(j) of the old one.  Block t takes block t + k while that exists; in the blocks that enter at the end the first
// last_len entries take the final state (the short block behind the T_blocks: x_T without an action; last_len = 0 for rows) and the
// rest repeat the last block.  Entries behind the blocks, and kept ones, stay (kept: the rows of dto_solver_shift_keep_rows).
DTO_HD static inline int64_t shift_source(int64_t j, int stride, int T_blocks, int last_len, int k, bool kept) {
  const int64_t t = j / stride, r = j % stride;
  if (t >= T_blocks || kept) return j;
  if (t + k < T_blocks) return (t + k) * stride + r;
  if (r < last_len) return (int64_t)T_blocks * stride + r;
  return (int64_t)(T_blocks - 1) * stride + r;
}

}  // namespace dto

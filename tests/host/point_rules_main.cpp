// The per-entry rules of csrc/dto_point_rules.hpp on the CPU (tests/test_point_rules_host.py builds this without device code and
// runs it under the address and undefined-behaviour sanitizers): the warm start of one variable, of one inequality row's slack, and
// the index map of a receding-horizon shift.  No HIP function is called.  Expected values are worked out by hand from the rules
// stated in include/dto.h (dto_solve_batch_warm, dto_point_shift), never taken from the functions under test; the shift is
// applied to whole arrays that are allocated at their exact length, so an index outside them is a sanitizer error.
#include <cmath>
#include <cstdio>
#include <vector>

#include "dto_point_rules.hpp"

using namespace dto;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #c);                \
      return 1;                                                    \
    }                                                              \
  } while (0)

static const double INF = INFINITY;

// shifted copy of one array through shift_source
static std::vector<double> shifted(const std::vector<double>& in, int stride, int T_blocks, int last_len, int k, const std::vector<int>* keep) {
  std::vector<double> out(in.size());
  for (size_t j = 0; j < in.size(); ++j) out[j] = in[(size_t)shift_source((int64_t)j, stride, T_blocks, last_len, k, keep && (*keep)[j])];
  return out;
}

int main() {
  const double push = 1e-2, frac = 1e-2;   // default_opts: bound_push, bound_frac
  {  // fixed variable: goes to its value, no multipliers, whatever was handed in
    const WarmVar w = warm_var(3.0, 1.5, 1.5, true, 7.0, 8.0, 0.1, push, frac);
    CHECK(w.v == 1.5 && w.zl == 0.0 && w.zu == 0.0);
  }
  {  // free on both sides: untouched, multipliers 0 even when some are handed in
    const WarmVar w = warm_var(-4.25, -INF, INF, true, 2.0, 3.0, 0.1, push, frac);
    CHECK(w.v == -4.25 && w.zl == 0.0 && w.zu == 0.0);
  }
  {  // two finite sides, interior point, positive multipliers: everything kept
    const WarmVar w = warm_var(0.5, 0.0, 1.0, true, 0.25, 0.125, 0.1, push, frac);
    CHECK(w.v == 0.5 && w.zl == 0.25 && w.zu == 0.125);
  }
  {  // on the lower bound: pushed by min(push max(1, |lo|), frac (hi - lo)) = min(1e-2, 1e-2 * 4) = 1e-2; the zero and the negative
     // multiplier become mu / gap
    const WarmVar w = warm_var(-2.0, -2.0, 2.0, true, 0.0, -1.0, 0.5, push, frac);
    CHECK(w.v == -2.0 + 0.02);
    CHECK(w.zl == 0.5 / (w.v + 2.0) && w.zu == 0.5 / (2.0 - w.v));
  }
  {  // a narrow box: the push is the fraction of the width, 1e-2 * 1e-3, on both sides
    const WarmVar lo = warm_var(-1.0, 0.0, 1e-3, true, 1.0, 1.0, 0.1, push, frac);
    const WarmVar hi = warm_var(1.0, 0.0, 1e-3, true, 1.0, 1.0, 0.1, push, frac);
    CHECK(lo.v == 0.0 + frac * 1e-3 && hi.v == 1e-3 - frac * 1e-3 && lo.zl == 1.0 && hi.zu == 1.0);
  }
  {  // one finite side each: push max(1, |bound|), the multiplier of the infinite side stays 0
    const WarmVar a = warm_var(5.0, 10.0, INF, true, 0.0, 9.0, 0.2, push, frac);
    CHECK(a.v == 10.0 + push * 10.0 && a.zl == 0.2 / (a.v - 10.0) && a.zu == 0.0);
    const WarmVar b = warm_var(5.0, -INF, 0.5, true, 9.0, 0.0, 0.2, push, frac);
    CHECK(b.v == 0.5 - push * 1.0 && b.zl == 0.0 && b.zu == 0.2 / (0.5 - b.v));
  }
  {  // without multipliers (a problem without finite bounds, or the tile solver's cold start of fixed variables): the point only
    const WarmVar w = warm_var(0.0, 1.0, 3.0, false, 5.0, 5.0, 0.1, push, frac);
    CHECK(w.v == 1.0 + std::fmin(push * 1.0, frac * 2.0) && w.zl == 0.0 && w.zu == 0.0);
  }
  {  // slacks: a positive pair is kept; anything else starts from the constraint value
    WarmSlack s = warm_slack(-0.3, 0.4, 2.0, 0.1, push);
    CHECK(s.s == 0.4 && s.nu == 2.0);
    s = warm_slack(-0.3, 0.4, 0.0, 0.1, push);           // multiplier not positive: s = max(0.3, 1e-2), nu = mu / s
    CHECK(s.s == 0.3 && s.nu == 0.1 / 0.3);
    s = warm_slack(-0.3, -1.0, 2.0, 0.1, push);          // slack not positive
    CHECK(s.s == 0.3 && s.nu == 0.1 / 0.3);
    s = warm_slack(5.0, 0.0, 0.0, 0.1, push);            // violated row: s = push max(1, 5)
    CHECK(s.s == push * 5.0 && s.nu == 0.1 / (push * 5.0));
    s = warm_slack(-1e-4, 0.0, 1.0, 1e-3, push);         // nearly active: s = push
    CHECK(s.s == push && s.nu == 1e-3 / push);
  }
  {  // shift of the variables: T = 5 knots, n_x = 2, n_u = 1: blocks [x x u] x 4, then x_T.  Entry value = 10 * knot + position
    const int nx = 2, nu = 1, T = 5, st = nx + nu;
    std::vector<double> z((size_t)((T - 1) * st + nx));
    for (int t = 0; t < T; ++t)
      for (int r = 0; r < (t < T - 1 ? st : nx); ++r) z[(size_t)(t * st + r)] = 10.0 * t + r;
    // k = 1: blocks 0..2 take 1..3; block 3 takes the final state (40, 41) and the last action (32); x_T stays
    const std::vector<double> w1 = {10, 11, 12, 20, 21, 22, 30, 31, 32, 40, 41, 32, 40, 41};
    CHECK(shifted(z, st, T - 1, nx, 1, nullptr) == w1);
    // k = 3 = T - 2: block 0 takes block 3, the others hold the end
    const std::vector<double> w3 = {30, 31, 32, 40, 41, 32, 40, 41, 32, 40, 41, 32, 40, 41};
    CHECK(shifted(z, st, T - 1, nx, 3, nullptr) == w3);
    CHECK(shifted(z, st, T - 1, nx, 0, nullptr) == z);
  }
  {  // shift of the multipliers: 4 blocks of 2 dynamics rows, 3 rows behind them (stage / general), row 2 kept
    const int nx = 2, T = 5;
    std::vector<double> mu = {0, 1, 10, 11, 20, 21, 30, 31, 100, 101, 102};
    std::vector<int> keep(mu.size(), 0);
    keep[2] = 1;
    // k = 2: block 0 <- 2, block 1 <- 3 (row 2 kept: 10), blocks 2, 3 repeat the last block; the tail stays
    const std::vector<double> want = {20, 21, 10, 31, 30, 31, 30, 31, 100, 101, 102};
    CHECK(shifted(mu, nx, T - 1, 0, 2, &keep) == want);
    const std::vector<double> nokeep = {20, 21, 30, 31, 30, 31, 30, 31, 100, 101, 102};
    CHECK(shifted(mu, nx, T - 1, 0, 2, nullptr) == nokeep);
  }
  {  // every source index of a 64-state, T = 16 layout is inside the array, for every k the entry points accept
    const int nx = 64, nu = 1, T = 16;
    const int64_t n = (int64_t)(T - 1) * (nx + nu) + nx;
    for (int k = 0; k <= T - 2; ++k)
      for (int64_t j = 0; j < n; ++j) {
        const int64_t s = shift_source(j, nx + nu, T - 1, nx, k, false);
        CHECK(s >= 0 && s < n && s % (nx + nu) == j % (nx + nu));
      }
  }
  printf("point rules ok\n");
  return 0;
}

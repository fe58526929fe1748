// The dense Schur-complement solve of the bordered step (csrc/dto_border_kernels.hpp: border_schur_solve -- lane 0 of k_border_solve
// and bordered_step_host call the same function) on the CPU.  tests/test_host_border_schur.py builds this without device code and
// runs it under the address and undefined-behaviour sanitizers.  No HIP function is called.  Expected values are worked out by
// hand (right-hand sides formed from a chosen solution in small integers) or, for n = 16, by an independent elimination (the
// Thomas algorithm on the tridiagonal matrix), never taken from the function under test.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "dto_kkt_kernels.hpp"
#include "dto_wide_kernels.hpp"
#include "dto_border_kernels.hpp"

using namespace dto;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #c);                \
      return 1;                                                    \
    }                                                              \
  } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-13 * std::fmax(1.0, std::fabs(b)); }

// storage of exactly n * n, n and n * n doubles on the heap (the address sanitizer sees one entry too far), the Cholesky scratch
// filled with NaN: whatever the function reads of it, it has written before
struct Case {
  int n;
  std::vector<double> S, r, L;
  Case(int n_, std::vector<double> S_, std::vector<double> r_)
      : n(n_), S(std::move(S_)), r(std::move(r_)), L((size_t)n_ * n_, std::numeric_limits<double>::quiet_NaN()) {}
  bool solve() { return border_schur_solve(n, S.data(), r.data(), L.data()); }
};

int main() {
  {  // n = 1: -2 y = 4
    Case c(1, {-2.0}, {4.0});
    CHECK(c.solve());
    CHECK(near(c.r[0], -2.0));
  }
  {  // n = 2, negative definite (-S = [2 -1; -1 3]), y = (1, -2)
    Case c(2, {-2.0, 1.0, 1.0, -3.0}, {-4.0, 7.0});
    CHECK(c.solve());
    CHECK(near(c.r[0], 1.0) && near(c.r[1], -2.0));
  }
  {  // n = 3, negative definite (diagonally dominant), y = (1, 2, 3)
    Case c(3, {-4.0, 1.0, 0.0, 1.0, -3.0, 1.0, 0.0, 1.0, -2.0}, {-2.0, -2.0, -4.0});
    CHECK(c.solve());
    CHECK(near(c.r[0], 1.0) && near(c.r[1], 2.0) && near(c.r[2], 3.0));
  }
  {  // n = 16: S = -tridiag(-1, 2, -1), the negative of the (positive definite) second-difference matrix; r_k = (-1)^k (k + 1).
     // Reference: the Thomas algorithm on S (no pivoting, its own recurrences)
    const int n = 16;
    std::vector<double> S((size_t)n * n, 0.0), r((size_t)n), ref((size_t)n), cp((size_t)n), dp((size_t)n);
    for (int k = 0; k < n; ++k) {
      S[(size_t)k * n + k] = -2.0;
      if (k > 0) S[(size_t)k * n + k - 1] = 1.0;
      if (k + 1 < n) S[(size_t)k * n + k + 1] = 1.0;
      r[(size_t)k] = (k % 2 ? -1.0 : 1.0) * (k + 1);
    }
    cp[0] = 1.0 / -2.0; dp[0] = r[0] / -2.0;
    for (int k = 1; k < n; ++k) {
      const double den = -2.0 - cp[(size_t)k - 1];
      cp[(size_t)k] = 1.0 / den;
      dp[(size_t)k] = (r[(size_t)k] - dp[(size_t)k - 1]) / den;
    }
    ref[(size_t)n - 1] = dp[(size_t)n - 1];
    for (int k = n - 2; k >= 0; --k) ref[(size_t)k] = dp[(size_t)k] - cp[(size_t)k] * ref[(size_t)k + 1];
    Case c(n, S, r);
    CHECK(c.solve());
    // condition number of the matrix is about 4 (n + 1)^2 / pi^2 = 117: 1e-13 relative leaves three decimal orders
    double big = 0.0;
    for (int k = 0; k < n; ++k) big = std::fmax(big, std::fabs(ref[(size_t)k]));
    for (int k = 0; k < n; ++k) CHECK(std::fabs(c.r[(size_t)k] - ref[(size_t)k]) <= 1e-13 * big);
  }
  {  // not negative definite (one positive eigenvalue): verdict false, the solution is still the elimination's, y = (2, -3)
    Case c(2, {1.0, 0.0, 0.0, -1.0}, {2.0, 3.0});
    CHECK(!c.solve());
    CHECK(near(c.r[0], 2.0) && near(c.r[1], -3.0));
  }
  {  // not symmetric: the verdict is about the symmetric part, -(S + S') / 2 = [2 -1; -1 2], positive definite.  The lower triangle
     // read alone would give [2 -3; -3 2], which is indefinite; y = (1, 2) (and a row swap: |3| > |-2|)
    Case c(2, {-2.0, -1.0, 3.0, -2.0}, {-4.0, -1.0});
    CHECK(c.solve());
    CHECK(near(c.r[0], 1.0) && near(c.r[1], 2.0));
  }
  {  // its transpose: the same symmetric part, now the upper triangle alone would be the indefinite one; y = (1, 2)
    Case c(2, {-2.0, 3.0, -1.0, -2.0}, {4.0, -5.0});
    CHECK(c.solve());
    CHECK(near(c.r[0], 1.0) && near(c.r[1], 2.0));
  }
  {  // the reverse: -(S + S') / 2 = [2 -3; -3 2] is indefinite though the lower triangle alone gives [2 -1; -1 2]: verdict false, the
     // solution is the elimination's of S as it stands (det = -1), y = (1, 1)
    Case c(2, {-2.0, 5.0, 1.0, -2.0}, {3.0, -1.0});
    CHECK(!c.solve());
    CHECK(near(c.r[0], 1.0) && near(c.r[1], 1.0));
  }
  {  // a row swap on a negative definite matrix: |S10| > |S00| (det = 4 - 2.25 > 0, trace < 0), y = (1, 1)
    Case c(2, {-1.0, 1.5, 1.5, -4.0}, {0.5, -2.5});
    CHECK(c.solve());
    CHECK(near(c.r[0], 1.0) && near(c.r[1], 1.0));
  }
  {  // a row swap that nothing but pivoting survives: zero diagonal, y = (5, 3); not negative definite
    Case c(2, {0.0, 1.0, 1.0, 0.0}, {3.0, 5.0});
    CHECK(!c.solve());
    CHECK(near(c.r[0], 5.0) && near(c.r[1], 3.0));
  }
  {  // exactly singular: the second pivot is -1 - (-1)(-1)/(-1) = 0.  Verdict false, zero written for that unknown, the first one
     // from the row that is left: -y0 - 0 = 2; nothing is divided by zero
    Case c(2, {-1.0, -1.0, -1.0, -1.0}, {2.0, 2.0});
    CHECK(!c.solve());
    CHECK(c.r[1] == 0.0 && near(c.r[0], -2.0));
    CHECK(std::isfinite(c.r[0]) && std::isfinite(c.r[1]));
  }
  {  // n = 0: no border.  Nothing is read or written (empty storage), the verdict is true: the stage part alone decides the inertia
    Case c(0, {}, {});
    CHECK(c.solve());
    CHECK(border_schur_solve(0, nullptr, nullptr, nullptr));
  }
  printf("border schur ok\n");
  return 0;
}

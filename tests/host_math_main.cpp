// Stand-alone checks of csrc/ccmm_host_math.hip (built by tests/test_host_math.py together with that unit; no GPU,
// no HIP call).  One command per input line, one "ok" per line answered, exit status 1 at the first failure:
//   self                         the built-in checks, on inputs whose arithmetic is exact in double
//   gl R X.. W..                 rule R of make_gl_nodes against the expected half rule (nodes, then weights)
//   tn MU SIG ELB U DRAW FLAG    ccmm_draw_trunc_normal against a recorded draw
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "ccmm_host.h"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                             \
    }                                                           \
  } while (0)

// A = L L' for L unit lower bidiagonal with ones on the subdiagonal: every pivot is exactly 1, the factor is L and
// the inverse is the integer matrix L^-T L^-1 = (-1)^(i + j) (n - max(i, j))
static void check_chol(int n) {
  std::vector<double> A((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    A[i + (size_t)i * n] = i ? 2.0 : 1.0;
    if (i + 1 < n) A[(i + 1) + (size_t)i * n] = A[i + (size_t)(i + 1) * n] = 1.0;
  }
  std::vector<double> L = A;
  host_chol(L, n);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) CHECK(L[i + (size_t)j * n] == ((i == j || i == j + 1) ? 1.0 : 0.0));
  const std::vector<double> inv = host_spd_inverse(A, n);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i)
      CHECK(inv[i + (size_t)j * n] == (((i + j) & 1) ? -1.0 : 1.0) * (n - std::max(i, j)));
}

static void check_not_spd() {
  std::vector<double> A = {1.0, 1.0, 1.0, 1.0};  // second pivot 1 - 1 = 0
  bool thrown = false;
  try {
    host_chol(A, 2);
  } catch (const ArgError& e) {
    thrown = std::strcmp(e.what(), "matrix not positive definite") == 0;
  }
  CHECK(thrown);
}

// P (K x Ny, K = Ny p + 1) with M in rows 1..Ny and a row 0 the inverse must not read
static std::vector<double> with_offset(const std::vector<double>& M, int Ny, int K) {
  std::vector<double> P((size_t)K * Ny, 7.0);
  for (int c = 0; c < Ny; ++c)
    for (int r = 0; r < Ny; ++r) P[(1 + r) + (size_t)c * K] = M[r + (size_t)c * Ny];
  return P;
}

// triangular branch: power-of-two diagonal, small integers below it; every quotient is a dyadic rational, so the
// substitution is exact and M A = I holds entry by entry
static void check_struct_lower() {
  const int Ny = 5, K = Ny * 2 + 1;
  const double dg[Ny] = {2.0, 0.5, 4.0, 1.0, 8.0};
  std::vector<double> M((size_t)Ny * Ny, 0.0);
  for (int c = 0; c < Ny; ++c)
    for (int r = c; r < Ny; ++r) M[r + (size_t)c * Ny] = r == c ? dg[c] : (double)((r * 3 + c * 5) % 7 - 3);
  const std::vector<double> P = with_offset(M, Ny, K);
  std::vector<double> A((size_t)Ny * Ny, 0.0);
  CHECK(host_struct_inverse(P.data(), K, Ny, true, A.data()));
  for (int c = 0; c < Ny; ++c)
    for (int r = 0; r < Ny; ++r) {
      if (r < c) CHECK(A[r + (size_t)c * Ny] == 0.0);
      double s = 0.0;
      for (int q = 0; q < Ny; ++q) s += M[r + (size_t)q * Ny] * A[q + (size_t)c * Ny];
      CHECK(s == (r == c ? 1.0 : 0.0));
    }
}

// Gauss-Jordan branch: M = (row permutation) x (power-of-two diagonal), M(perm(c), c) = d(c): column c's pivot sits
// in another row (Ny > 1), and the inverse A(c, perm(c)) = 1 / d(c) is exact
static void check_struct_full(int Ny) {
  const int K = Ny * 3 + 1;
  std::vector<double> M((size_t)Ny * Ny, 0.0), dg(Ny);
  for (int c = 0; c < Ny; ++c) {
    dg[c] = std::ldexp(1.0, c % 7 - 3);
    M[(c + 1) % Ny + (size_t)c * Ny] = dg[c];
  }
  const std::vector<double> P = with_offset(M, Ny, K);
  std::vector<double> A((size_t)Ny * Ny, -1.0);
  CHECK(host_struct_inverse(P.data(), K, Ny, false, A.data()));
  for (int c = 0; c < Ny; ++c)
    for (int r = 0; r < Ny; ++r) CHECK(A[r + (size_t)c * Ny] == (c == (r + 1) % Ny ? 1.0 / dg[r] : 0.0));
}

static void check_struct_singular() {
  const int Ny = 3, K = Ny + 1;
  std::vector<double> M = {0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 4.0, 0.0, 1.0};  // column 1 is zero
  const std::vector<double> P = with_offset(M, Ny, K);
  std::vector<double> A((size_t)Ny * Ny, 0.0);
  CHECK(!host_struct_inverse(P.data(), K, Ny, false, A.data()));
}

static void check_trunc_branches() {
  uint8_t fl = 9;
  CHECK(ccmm_draw_trunc_normal(0.7, 1e-12, 0.25, 0.3, &fl) == 0.7 && fl == 0);  // sig <= tol: the mean
  CHECK(ccmm_draw_trunc_normal(60.0, 1.0, 0.25, 0.3, &fl) == 0.25 && fl == 1);  // no mass below the bound: the bound
  const double v = ccmm_draw_trunc_normal(0.0, 1.0, 0.25, 0.3, &fl);
  CHECK(v < 0.25 && fl == 3);
  CHECK(ccmm_draw_trunc_normal(0.0, 1.0, 0.25, 0.3, nullptr) == v);
}

static bool within_ulps(double got, double want, int k) {
  const double ulp = std::nextafter(std::fabs(want), INFINITY) - std::fabs(want);
  return std::fabs(got - want) <= k * ulp;
}

int main() {
  const ccmm::GLNodes g = make_gl_nodes();
  CHECK(std::memcmp(&g, &gl_nodes(), sizeof g) == 0);
  char buf[1 << 14];
  while (std::fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    std::vector<double> v;
    while (in >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));  // (hex floats: exact)
    if (cmd == "self") {
      for (int n : {1, 2, 5, 128}) check_chol(n);
      check_not_spd();
      check_struct_lower();
      for (int Ny : {1, 3, 128}) check_struct_full(Ny);
      check_struct_singular();
      check_trunc_branches();
    } else if (cmd == "gl") {
      const int r = (int)v[0], half = ((int)v.size() - 1) / 2;
      CHECK(r >= 0 && r < 3 && half == (r == 0 ? 3 : r == 1 ? 6 : 10));
      for (int i = 0; i < half; ++i) {
        CHECK(g.w[r][i] > 0.0 && g.x[r][i] > -1.0 && g.x[r][i] < 0.0);
        CHECK(i == 0 || g.x[r][i] > g.x[r][i - 1]);
        CHECK(within_ulps(g.x[r][i], v[1 + i], 2));
        // (the recurrence's rounding in P_n', amplified by 1 / (1 - x^2) <= 73 and squared: below 2e-12 relative)
        CHECK(std::fabs(g.w[r][i] - v[1 + half + i]) <= 2e-12 * v[1 + half + i]);
      }
    } else if (cmd == "tn") {
      CHECK(v.size() == 6);
      uint8_t fl = 9;
      const double d = ccmm_draw_trunc_normal(v[0], v[1], v[2], v[3], &fl);
      CHECK(fl == (uint8_t)v[5]);
      CHECK(std::fabs(d - v[4]) <= 1e-12 * std::max(1.0, std::fabs(v[4])));
    } else {
      CHECK(!"unknown command");
    }
    std::printf("ok\n");
  }
  return 0;
}

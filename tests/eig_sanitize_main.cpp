// Stand-alone program for a sanitizer build of the eigenvalue core (csrc/ccmm_eig.hip, ccmm_eig.h): calls
// ccmm_max_var_root_host on a (3, 2) and a (20, 12) Minnesota-like batch and on a batch with a NaN and an Inf
// entry, and checks the documented answers (info, NaN, untouched neighbours).  Not a pytest; build the two
// files together with the host pass under -fsanitize=address,undefined and run the program once:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -I include -I ccmmshadowratevar-code_amd/csrc tests/eig_sanitize_main.cpp \
//       ccmmshadowratevar-code_amd/csrc/ccmm_eig.hip -o eig_sanitize && ./eig_sanitize
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ccmm.h"
#include "ccmm_err.h"

// the library's error string lives in ccmm_abi.hip; the stand-alone build carries its own
namespace ccmm {
static thread_local std::string g_err;
void set_last_error(const std::string& msg) { g_err = msg; }
const std::string& last_error() { return g_err; }
}  // namespace ccmm

static unsigned long long g_state = 88172645463325252ull;
static double urand() {  // xorshift64, uniform in (-1, 1)
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 4503599627370496.0 - 1.0;
}

// M Minnesota-like coefficient matrices: own first lag 0.5, own lag l 0.3 / l^2, small noise elsewhere
static std::vector<double> minnesota(int M, int N, int p) {
  const int K = N * p + 1;
  std::vector<double> P((size_t)M * K * N);
  for (int m = 0; m < M; ++m)
    for (int j = 0; j < N; ++j)
      for (int k = 0; k < K; ++k) {
        double v = 0.01 * urand();
        if (k >= 1 && (k - 1) % N == j) {
          const int l = (k - 1) / N + 1;
          v += l == 1 ? 0.5 : 0.3 / (l * l);
        }
        P[((size_t)m * N + j) * K + k] = v;
      }
  return P;
}

static int fails = 0;
static void check(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++fails;
  }
}

int main() {
  const int shapes[2][3] = {{3, 2, 7}, {20, 12, 3}};
  for (auto& s : shapes) {
    const int N = s[0], p = s[1], M = s[2], K = N * p + 1;
    std::vector<double> P = minnesota(M, N, p), root(M, -1.0);
    std::vector<int> info(M, -1);
    check(ccmm_max_var_root_host(M, N, p, K, P.data(), root.data(), info.data()) == CCMM_OK, "return code");
    for (int m = 0; m < M; ++m) {
      check(info[m] == 0, "info == 0");
      check(root[m] > 0.3 && root[m] < 1.2, "root in the family's range");
      std::printf("N=%d p=%d m=%d maxroot=%.17g\n", N, p, m, root[m]);
    }
    // non-finite entries in matrices 1 and 2: NaN, info = 1; the others bit for bit as before
    if (M >= 3) {
      std::vector<double> Q = P, r2(M, -1.0);
      std::vector<int> i2(M, -1);
      Q[(size_t)1 * K * N + 1] = std::nan("");
      Q[(size_t)2 * K * N + (size_t)(N - 1) * K + N * p] = INFINITY;
      check(ccmm_max_var_root_host(M, N, p, K, Q.data(), r2.data(), i2.data()) == CCMM_OK, "return code (NaN)");
      check(std::isnan(r2[1]) && i2[1] == 1, "NaN entry -> NaN, info 1");
      check(std::isnan(r2[2]) && i2[2] == 1, "Inf entry -> NaN, info 1");
      check(std::memcmp(&r2[0], &root[0], sizeof(double)) == 0 && i2[0] == 0, "neighbour unchanged");
      // info may be NULL; the intercept row is not part of the companion
      Q = P;
      Q[0] = std::nan("");
      check(ccmm_max_var_root_host(M, N, p, K, Q.data(), r2.data(), nullptr) == CCMM_OK, "info NULL");
      check(std::memcmp(r2.data(), root.data(), M * sizeof(double)) == 0, "NaN intercept ignored");
    }
  }
  check(ccmm_max_var_root_host(1, 2, 2, 4, nullptr, nullptr, nullptr) == CCMM_ERR_ARG, "K too small refused");
  std::printf(fails ? "eig_sanitize: %d FAILED\n" : "eig_sanitize OK\n", fails);
  return fails != 0;
}

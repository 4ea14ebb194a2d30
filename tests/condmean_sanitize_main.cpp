// Stand-alone program for a sanitizer build of the host twin of the conditional-mean core (csrc/ccmm_condmean.hip,
// ccmm_condmean.h): calls ccmm_cond_mean_host over the plan-edge shapes (N in {1, 16, 17, 32, 33}, N p in {255, 256,
// 257}) and the reference shape, with rows beyond 1 + N p in every matrix, exactly sized buffers, shared and per-draw
// y0, and checks the documented answers (H = 1 is the one fma chain, info and NaN of a non-finite draw, untouched
// neighbours, the refusals).  Not a pytest and no GPU call; build the two files together with the host pass under
// -fsanitize=address,undefined and run the program once:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -I include -I ccmmshadowratevar-code_amd/csrc tests/condmean_sanitize_main.cpp \
//       ccmmshadowratevar-code_amd/csrc/ccmm_condmean.hip -o condmean_sanitize && ./condmean_sanitize
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

static int fails = 0;
static void check(bool ok, const char* what, int N, int p) {
  if (!ok) {
    std::printf("FAIL N=%d p=%d %s\n", N, p, what);
    ++fails;
  }
}

int main() {
  const int shapes[][2] = {{1, 1},  {1, 255}, {1, 256}, {1, 257}, {16, 1}, {16, 16}, {17, 2}, {17, 15},
                           {5, 51}, {32, 8},  {33, 2},  {3, 86},  {20, 12}};
  const int M = 5, H = 7, extra = 2;
  for (auto& s : shapes) {
    const int N = s[0], p = s[1], Np = N * p, K = Np + 1 + extra;
    const size_t per = (size_t)K * N;
    std::vector<double> P(M * per), y0((size_t)M * Np), mean((size_t)M * N), mean1((size_t)M * N), one((size_t)M * N);
    for (auto& v : P) v = 0.9 * urand() / std::sqrt((double)Np);
    for (auto& v : y0) v = urand();
    for (int m = 0; m < M; ++m)  // the rows beyond 1 + N p: never read
      for (int i = 0; i < N; ++i)
        for (int e = 0; e < extra; ++e) P[m * per + (size_t)i * K + Np + 1 + e] = NAN;
    std::vector<int> info(M, -1);
    check(ccmm_cond_mean_host(M, N, p, K, H, P.data(), y0.data(), M, mean.data(), info.data()) == CCMM_OK,
          "return code (per-draw y0)", N, p);
    check(ccmm_cond_mean_host(M, N, p, K, H, P.data(), y0.data(), 1, mean1.data(), nullptr) == CCMM_OK,
          "return code (shared y0, info NULL)", N, p);
    check(ccmm_cond_mean_host(M, N, p, K, 1, P.data(), y0.data(), M, one.data(), nullptr) == CCMM_OK,
          "return code (H = 1)", N, p);
    bool ok = true, same0 = true, h1 = true;
    for (int m = 0; m < M; ++m) {
      ok = ok && info[m] == 0;
      for (int i = 0; i < N; ++i) {
        ok = ok && std::isfinite(mean[(size_t)m * N + i]);
        double acc = P[m * per + (size_t)i * K];  // H = 1: the one chain from the intercept over k ascending
        for (int k = 0; k < Np; ++k) acc = std::fma(P[m * per + (size_t)i * K + 1 + k], y0[(size_t)m * Np + k], acc);
        h1 = h1 && std::memcmp(&acc, &one[(size_t)m * N + i], sizeof acc) == 0;
      }
    }
    same0 = std::memcmp(mean.data(), mean1.data(), N * sizeof(double)) == 0;  // draw 0 has the shared state
    check(ok, "finite means, info 0", N, p);
    check(h1, "H = 1 is the fma chain from the intercept", N, p);
    check(same0, "draw 0 does not depend on how y0 is given", N, p);
    // a non-finite lag coefficient and a non-finite intercept: info 1, NaN, the neighbours keep their bits
    std::vector<double> Q = P, got((size_t)M * N);
    Q[1 * per + (size_t)(N - 1) * K + Np] = INFINITY;
    Q[3 * per] = NAN;
    check(ccmm_cond_mean_host(M, N, p, K, H, Q.data(), y0.data(), M, got.data(), info.data()) == CCMM_OK,
          "return code (non-finite)", N, p);
    bool flags = info[0] == 0 && info[1] == 1 && info[2] == 0 && info[3] == 1 && info[4] == 0, nan = true, keep = true;
    for (int i = 0; i < N; ++i) nan = nan && std::isnan(got[(size_t)N + i]) && std::isnan(got[(size_t)3 * N + i]);
    for (int m : {0, 2, 4})
      keep = keep && std::memcmp(&got[(size_t)m * N], &mean[(size_t)m * N], N * sizeof(double)) == 0;
    check(flags, "info of the non-finite draws", N, p);
    check(nan, "NaN means of the non-finite draws", N, p);
    check(keep, "the other draws keep their bits", N, p);
  }
  double y[4] = {0, 0, 0, NAN}, Pz[10] = {0}, mz[4];
  check(ccmm_cond_mean_host(2, 2, 2, 4, 3, Pz, y, 1, mz, nullptr) == CCMM_ERR_ARG, "K too small refused", 2, 2);
  check(ccmm_cond_mean_host(1, 2, 2, 5, 3, Pz, y, 1, mz, nullptr) == CCMM_ERR_ARG, "non-finite y0 refused", 2, 2);
  check(ccmm_cond_mean_host(1, 2, 2, 5, 0, Pz, y, 1, mz, nullptr) == CCMM_ERR_ARG, "H = 0 refused", 2, 2);
  check(ccmm_cond_mean_host(1, 2, 2, 5, 3, Pz, y, 2, mz, nullptr) == CCMM_ERR_ARG, "ny0 not 1 or M refused", 2, 2);
  std::printf(fails ? "condmean_sanitize: %d FAILED\n" : "condmean_sanitize OK\n", fails);
  return fails != 0;
}

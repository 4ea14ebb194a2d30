// Stand-alone program for a sanitizer build of the host twin of the impulse-response core (csrc/ccmm_vma.hip,
// ccmm_vma.h): calls ccmm_vma_host over the plan-edge shapes (N in {1, 16, 17, 32, 33}, N p in {255, 256, 257}) and
// the reference shape, with rows beyond 1 + N p in every matrix, and checks the documented answers (Psi_1 = Phi_1
// exactly, the first horizons independent of H, info and NaN of a non-finite draw, untouched neighbours).  Not a
// pytest and no GPU call; build the two files together with the host pass under -fsanitize=address,undefined and
// run the program once:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -I include -I ccmmshadowratevar-code_amd/csrc tests/vma_sanitize_main.cpp \
//       ccmmshadowratevar-code_amd/csrc/ccmm_vma.hip -o vma_sanitize && ./vma_sanitize
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
  const int M = 3, H = 6, extra = 2;
  for (auto& s : shapes) {
    const int N = s[0], p = s[1], Np = N * p, K = Np + 1 + extra;
    const size_t per = (size_t)K * N, NN = (size_t)N * N;
    std::vector<double> P(M * per);
    for (int m = 0; m < M; ++m)
      for (int j = 0; j < N; ++j)
        for (int k = 0; k < K; ++k) P[m * per + (size_t)j * K + k] = k > Np ? 1e300 : urand() / std::sqrt((double)Np);
    std::vector<double> V(M * H * NN, -1.0), V1(M * NN, -1.0);
    std::vector<int> info(M, -1);
    check(ccmm_vma_host(M, N, p, K, H, P.data(), V.data(), info.data()) == CCMM_OK, "return code", N, p);
    check(ccmm_vma_host(M, N, p, K, 1, P.data(), V1.data(), nullptr) == CCMM_OK, "return code (H = 1, info NULL)", N, p);
    double worst = 0.0;
    for (int m = 0; m < M; ++m) {
      check(info[m] == 0, "info == 0", N, p);
      for (int j = 0; j < N; ++j)
        for (int i = 0; i < N; ++i) {
          const double psi1 = V[(size_t)m * H * NN + (size_t)j * N + i];
          check(psi1 == P[m * per + (size_t)i * K + 1 + j], "Psi_1 == Phi_1", N, p);
          check(psi1 == V1[(size_t)m * NN + (size_t)j * N + i], "horizon 1 independent of H", N, p);
        }
      for (size_t e = 0; e < H * NN; ++e) {
        check(std::isfinite(V[(size_t)m * H * NN + e]), "finite", N, p);
        worst = std::fmax(worst, std::fabs(V[(size_t)m * H * NN + e]));
      }
    }
    // a NaN in matrix 1, an Inf in the last coefficient of matrix 2, a NaN in matrix 0's intercept
    std::vector<double> Q = P, W(M * H * NN, -1.0);
    Q[1 * per + 1] = std::nan("");
    Q[2 * per + (size_t)(N - 1) * K + Np] = INFINITY;
    Q[0] = std::nan("");
    check(ccmm_vma_host(M, N, p, K, H, Q.data(), W.data(), info.data()) == CCMM_OK, "return code (NaN)", N, p);
    check(info[0] == 0 && info[1] == 1 && info[2] == 1, "info of the non-finite draws", N, p);
    for (size_t e = 0; e < H * NN; ++e)
      check(std::isnan(W[H * NN + e]) && std::isnan(W[2 * H * NN + e]), "non-finite draw all NaN", N, p);
    check(std::memcmp(W.data(), V.data(), H * NN * sizeof(double)) == 0, "NaN intercept ignored, neighbour unchanged", N,
          p);
    std::printf("N=%d p=%d Np=%d max|Psi|=%.6g Psi_%d(0,0)=%.17g\n", N, p, Np, worst, H, V[(size_t)(H - 1) * NN]);
  }
  check(ccmm_vma_host(1, 2, 2, 4, 3, nullptr, nullptr, nullptr) == CCMM_ERR_ARG, "K too small refused", 2, 2);
  std::printf(fails ? "vma_sanitize: %d FAILED\n" : "vma_sanitize OK\n", fails);
  return fails != 0;
}

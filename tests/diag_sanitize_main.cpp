// Stand-alone program for a sanitizer build of the diagnostics host twin (csrc/ccmm_diag.cpp with the core of
// ccmm_diagk.h): calls ccmm_diagnostics_host at M = 100, 101, 250 and S = 1, 65 in both stride conventions, on
// buffers of exactly M * S doubles, and checks the documented answers (same bits in both conventions, a constant
// series, the refusal below 100 draws).  Not a pytest; build the two files together under
// -fsanitize=address,undefined and run the program once:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -I include \
//       -I ccmmshadowratevar-code_amd/csrc tests/diag_sanitize_main.cpp \
//       ccmmshadowratevar-code_amd/csrc/ccmm_diag.cpp -pthread -o diag_sanitize && ./diag_sanitize
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
static void check(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++fails;
  }
}

int main() {
  for (int M : {100, 101, 250})
    for (int S : {1, 65}) {
      // AR(1) series with mean s, series-major (MATLAB's ndraw x nvar) and its transpose (the store's order)
      std::vector<double> a((size_t)M * S), b((size_t)M * S);
      for (int s = 0; s < S; ++s) {
        double x = urand();
        for (int m = 0; m < M; ++m) {
          x = 0.8 * x + 0.6 * urand();
          a[(size_t)s * M + m] = b[(size_t)m * S + s] = x + s;
        }
      }
      if (S > 1)
        for (int m = 0; m < M; ++m) a[(size_t)(S - 1) * M + m] = b[(size_t)m * S + S - 1] = 1.5;  // constant
      std::vector<double> oa((size_t)CCMM_DIAG_NSTAT * S, -7.0), ob(oa);
      check(ccmm_diagnostics_host(M, S, 1, M, a.data(), oa.data()) == CCMM_OK, "return code (ld_draw = 1)");
      check(ccmm_diagnostics_host(M, S, S, 1, b.data(), ob.data()) == CCMM_OK, "return code (ld_series = 1)");
      for (size_t i = 0; i < oa.size(); ++i) {
        const bool same = std::memcmp(&oa[i], &ob[i], sizeof(double)) == 0 || (std::isnan(oa[i]) && std::isnan(ob[i]));
        check(same, "both stride conventions give the same bits");
      }
      const int s0 = 0;
      check(oa[1 * S + s0] > 0 && oa[2 * S + s0] > 0 && oa[5 * S + s0] > 0 && oa[10 * S + s0] > 0.5,
            "pstd, nse, rne1, psrf of an AR(1) series");
      if (S > 1) {
        const int c = S - 1;
        check(oa[0 * S + c] == 1.5 && oa[1 * S + c] == -1.0 && oa[2 * S + c] == -1.0, "constant: pmean, pstd, nse");
        check(std::isnan(oa[3 * S + c]) && std::isnan(oa[5 * S + c]) && std::isnan(oa[10 * S + c]),
              "constant: rne, rne1, psrf NaN");
      }
      std::printf("M=%d S=%d pmean=%.17g rne1=%.17g psrf=%.17g\n", M, S, oa[0], oa[5 * S], oa[10 * S]);
    }
  std::vector<double> x(99, 1.0), o(CCMM_DIAG_NSTAT);
  check(ccmm_diagnostics_host(99, 1, 1, 99, x.data(), o.data()) == CCMM_ERR_ARG, "M = 99 refused");
  check(ccmm::last_error() == "momentg: needs a larger number of ndraws", "momentg's message");
  std::printf(fails ? "diag_sanitize: %d FAILED\n" : "diag_sanitize OK\n", fails);
  return fails != 0;
}

// Prints the launch plan of the predictive-density kernel with and without the IRF1 simulations, as ccmm_fcst.h
// computes it, one line per query read from standard input (tests/test_irf1_plans.py).  Host code only: no HIP
// runtime call.
//
//   plan N p H bh Kx reg_opt -> the k_fcst<RN> instance; hc and LDS bytes of the plain form (fcst_chunk,
//                               fcst_paths_lds_doubles); hc and LDS bytes of the IRF form (fcst_irf_chunk,
//                               fcst_irf_lds_doubles); fcst_irf_rings
#include <cstdio>
#include <cstring>

#include "ccmm_fcst.h"

using namespace ccmm;

int main() {
  char cmd[16];
  int N, p, H, bh, Kx, ro;
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "plan") && std::scanf("%d %d %d %d %d %d", &N, &p, &H, &bh, &Kx, &ro) == 6) {
      const bool reg = fcst_reg_path(N, p, bh) && ro;
      const int hc = fcst_chunk(N, Kx, p, H, reg), hi = fcst_irf_chunk(N, Kx, p, H, reg, bh);
      std::printf("%d %d %zu %d %zu %zu\n", fcst_variant(N, p, bh, ro != 0), hc,
                  fcst_paths_lds_doubles(N, Kx, p, hc, reg) * sizeof(double), hi,
                  fcst_irf_lds_doubles(N, Kx, p, hi, reg, bh) * sizeof(double), fcst_irf_rings(bh));
    } else {
      std::fprintf(stderr, "bad query: %s\n", cmd);
      return 2;
    }
  }
  return 0;
}

// Prints the plan of the large-N predictive-density kernels that ccmm_fcst_big.h computes, one line per query
// read from standard input (tests/test_fcst_big_plans.py).  Host code only: no HIP runtime call.
//
//   plan N p H Nd bh   -> ok cols hc tiles waves lds lds_scores ring_stride columns pai_bytes
#include <cstdio>
#include <cstring>

#include "ccmm_fcst_big.h"

using namespace ccmm;

int main() {
  char cmd[16];
  int N, p, H, Nd, bh;
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "plan") && std::scanf("%d %d %d %d %d", &N, &p, &H, &Nd, &bh) == 5) {
      const FcstBigPlan pl = fcst_big_plan(N, p, H, Nd, bh);
      std::printf("%d %d %d %d %d %zu %zu %d %d %zu\n", (int)pl.ok, pl.cols, pl.hc, pl.tiles, pl.waves, pl.lds,
                  pl.lds_scores, fcst_big_ring_stride(N, p), fcst_big_columns(Nd, bh), fcst_big_pai_bytes(N, p, H, Nd, bh));
    } else {
      std::fprintf(stderr, "bad query: %s\n", cmd);
      return 2;
    }
  }
  return 0;
}

// Prints the launch arithmetic of the diagnostics kernel (ccmm_diagk.h diag_plan, diag_entry, diag_block_series)
// for tests/test_diag_plan.py: one line "S C M" in; out "threads waves grid_x grid_y lds per_cu block" and then,
// per chain, the entry of every thread of every workgroup on one line.  No HIP runtime call.
#include <cstdio>

#include "ccmm_diagk.h"

int main() {
  int S, C, M;
  while (std::scanf("%d %d %d", &S, &C, &M) == 3) {
    const ccmm::DiagPlan pl = ccmm::diag_plan(S, C);
    std::printf("%d %d %d %d %zu %d %d\n", pl.threads, pl.waves, pl.grid_x, pl.grid_y, pl.lds, pl.per_cu,
                ccmm::diag_block_series(M));
    for (int c = 0; c < pl.grid_y; ++c) {
      for (int bx = 0; bx < pl.grid_x; ++bx)
        for (int t = 0; t < pl.threads; ++t) std::printf("%lld ", ccmm::diag_entry(bx, t));
      std::printf("\n");
    }
  }
  return 0;
}

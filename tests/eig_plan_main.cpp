// Prints the launch arithmetic of the maximum-VAR-root kernel (ccmm_eig.h eig_plan) for tests/test_eig_plan.py:
// one line "n M" in, one line "device threads chunk launches grid lds scratch" out.  No HIP runtime call.
#include <cstdio>

#include "ccmm_eig.h"

int main() {
  int n, M;
  while (std::scanf("%d %d", &n, &M) == 2) {
    const ccmm::EigPlan pl = ccmm::eig_plan(n, M);
    std::printf("%d %d %d %d %d %zu %zu\n", pl.device, pl.threads, pl.chunk, pl.launches, pl.grid, pl.lds, pl.scratch);
  }
  return 0;
}

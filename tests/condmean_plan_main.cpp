// Prints the launch arithmetic of the conditional-mean kernel (ccmm_condmean.h cond_mean_plan) for
// tests/test_condmean_host.py: one line "N p M" in, one line "device stride per waves threads lds grid" out.
// No HIP runtime call.
#include <cstdio>

#include "ccmm_condmean.h"

int main() {
  int N, p;
  long long M;
  while (std::scanf("%d %d %lld", &N, &p, &M) == 3) {
    const ccmm::CondMeanPlan pl = ccmm::cond_mean_plan(N, p, M);
    std::printf("%d %d %zu %d %d %zu %lld\n", pl.device, pl.stride, pl.per, pl.waves, pl.threads, pl.lds, pl.grid);
  }
  return 0;
}

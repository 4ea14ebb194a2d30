// Prints the pass arithmetic of the stored-draw GIRFs (ccmm_girf_store.h girf_pass_plan) for
// tests/test_girf_store_host.py: one line "n N H nsim want cap p" in (cap 0: the header's kGirfPassCap), one line
// "per draws npass last bytes prep_lds rb_lds" out.  No HIP runtime call.
#include <cstdio>

#include "ccmm_girf_store.h"

int main() {
  long long n;
  int N, H, nsim, want, p;
  unsigned long long cap;
  while (std::scanf("%lld %d %d %d %d %llu %d", &n, &N, &H, &nsim, &want, &cap, &p) == 7) {
    const ccmm::GirfPassPlan pl =
        cap ? ccmm::girf_pass_plan(n, N, H, nsim, want, (size_t)cap) : ccmm::girf_pass_plan(n, N, H, nsim, want);
    std::printf("%zu %d %d %d %zu %zu %zu\n", pl.per, pl.draws, pl.npass, pl.last, pl.bytes, ccmm::girf_prep_lds(N),
                ccmm::girf_rb_lds(N, p));
  }
  return 0;
}

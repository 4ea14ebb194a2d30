// Prints the launch arithmetic of the impulse-response kernel (ccmm_vma.h vma_plan) for tests/test_vma_plan.py:
// one line "N p n H cap" in (cap 0: the header's kVmaBufCap), one line "device tiles threads lds hslab nslab last
// buf" out.  No HIP runtime call.
#include <cstdio>

#include "ccmm_vma.h"

int main() {
  int N, p, H;
  long long n;
  unsigned long long cap;
  while (std::scanf("%d %d %lld %d %llu", &N, &p, &n, &H, &cap) == 5) {
    const ccmm::VmaPlan pl = cap ? ccmm::vma_plan(N, p, n, H, (size_t)cap) : ccmm::vma_plan(N, p, n, H);
    std::printf("%d %d %d %zu %d %d %d %zu\n", pl.device, pl.tiles, pl.threads, pl.lds, pl.hslab, pl.nslab, pl.last,
                pl.buf);
  }
  return 0;
}

// Batched spectral radius of VAR companion matrices: the device kernel and the host twin of ccmm_eig.h.
//
// Mapping.  A 240 x 240 fp64 companion is 460 KB, more than one CU's LDS, and the bulge chase is a dependent
// chain of about n^2 small steps: one matrix is latency-bound, the parallelism is the batch.  One wave owns
// one matrix (kEigWaves independent waves per workgroup); the working matrix is an n^2 slab of global scratch
// that stays in L2 / MALL while it is hot, the current reflector sits in LDS.  Inside the wave the lanes split
// the columns (or rows) of each reflector's update; the hand-off between the lanes goes through memory with
// a workgroup-scope fence and a wave barrier.  No wave waits on another wave: no flags, no spinning, no
// workgroup barrier.  Every loop is bounded by n or by the iteration cap of eig_qr.
//
// Built with -ffp-contract=off: the host twin below instantiates the same core with one lane and returns
// the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/ccmm.h"
#include "ccmm_eig.h"
#include "ccmm_err.h"
#include "ccmm_internal.h"

namespace {

// accepted chains (acc[c] != 0) take PAI, E and the status word back from the snapshot
__global__ __launch_bounds__(256) void k_stat_select(int nPAI, int nE, const int* __restrict__ acc,
                                                     const double* __restrict__ sPAI, const double* __restrict__ sE,
                                                     const int* __restrict__ sStatus, double* __restrict__ PAI,
                                                     double* __restrict__ E, int* __restrict__ status) {
  const int c = blockIdx.y;
  if (!acc[c]) return;
  const size_t oP = (size_t)c * nPAI, oE = (size_t)c * nE;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nPAI; i += gridDim.x * blockDim.x) PAI[oP + i] = sPAI[oP + i];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nE; i += gridDim.x * blockDim.x) E[oE + i] = sE[oE + i];
  if (blockIdx.x == 0 && threadIdx.x == 0) status[c] = sStatus[c];
}

}  // namespace

namespace ccmm {

namespace {

struct EigWave {
  static constexpr int W = 64;
  __device__ inline int lane() const { return threadIdx.x & 63; }
  __device__ inline void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
};

__host__ __device__ inline const double* eig_src(const EigSrc& s, long long m) {
  return s.PAI + (m % s.na) * s.sa + (m / s.na) * s.sb;
}

// matrix m0 + (wave of the grid); scratch slab = wave of the grid
__global__ __launch_bounds__(64 * kEigWaves) void k_eig_maxroot(int m0, int m1, int N, int p, EigSrc src,
                                                                 double* __restrict__ maxroot,
                                                                 int* __restrict__ info, double* scratch) {
  __shared__ double ort[kEigWaves][kEigMaxN];
  const int wave = threadIdx.x >> 6;
  const long long w = (long long)blockIdx.x * kEigWaves + wave;
  const long long m = m0 + w;
  if (m >= m1) return;
  const int n = N * p;
  const EigMat H{scratch + (size_t)w * n * n, n};
  const EigWave g;
  double rho = 0.0;
  const int fl = eig_core(g, eig_src(src, m), src.ld, N, p, H, ort[wave], &rho);
  if (g.lane() == 0) {
    maxroot[m] = rho;
    info[m] = fl;
  }
}

}  // namespace

hipError_t eig_launch(hipStream_t st, int M, int N, int p, const EigSrc& src, double* maxroot, int* info,
                      double* scratch) {
  const EigPlan pl = eig_plan(N * p, M);
  if (!pl.device) return hipErrorInvalidValue;
  for (int m0 = 0; m0 < M; m0 += pl.chunk) {  // launches on one stream share the scratch in order
    const int m1 = std::min(M, m0 + pl.chunk);
    const int grid = (m1 - m0 + kEigWaves - 1) / kEigWaves;
    const hipError_t e = launch_k(k_eig_maxroot, dim3(grid), dim3(pl.threads), 0, false, st, m0, m1, N, p, src, maxroot,
                                  info, scratch);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t eig_launch_stat_select(hipStream_t st, int B, int nPAI, int nE, const int* acc, const double* sPAI,
                                  const double* sE, const int* sStatus, double* PAI, double* E, int* status) {
  return launch_k(k_stat_select, dim3(8, B), dim3(256), 0, false, st, nPAI, nE, acc, sPAI, sE, sStatus, PAI, E, status);
}

void eig_host(int M, int N, int p, const EigSrc& src, double* maxroot, int* info) {
  const int n = N * p;
  std::atomic<int> next{0};
  auto work = [&] {
    std::vector<double> H((size_t)n * n), ort(n);
    const EigSerial g;
    for (int m; (m = next++) < M;) {
      double rho = 0.0;
      const int fl = eig_core(g, eig_src(src, m), src.ld, N, p, EigMat{H.data(), n}, ort.data(), &rho);
      maxroot[m] = rho;
      if (info) info[m] = fl;
    }
  };
  const unsigned nth = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
  std::vector<std::thread> th;
  for (unsigned i = 1; i < std::min<unsigned>(nth, (unsigned)M); ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

}  // namespace ccmm

extern "C" int ccmm_max_var_root_host(int M, int N, int p, int K, const double* PAI, double* maxroot, int* info) {
  if (M < 0 || N < 1 || p < 1 || (long long)N * p + 1 > K || (M > 0 && (!PAI || !maxroot))) {
    ccmm::set_last_error("ccmm_max_var_root_host: need M >= 0, N, p >= 1, K >= 1 + N p, PAI and maxroot");
    return CCMM_ERR_ARG;
  }
  try {
    ccmm::eig_host(M, N, p, ccmm::EigSrc{PAI, K, M > 0 ? M : 1, (long long)K * N, 0}, maxroot, info);
  } catch (const std::exception& e) {  // allocation or thread start
    ccmm::set_last_error(e.what());
    return CCMM_ERR_HIP;
  }
  return CCMM_OK;
}

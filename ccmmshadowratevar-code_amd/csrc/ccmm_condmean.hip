// Conditional mean paths of VAR coefficient draws: the device kernel and the host twin of ccmm_condmean.h.
//
// Mapping.  One wave per draw, up to four draws per workgroup (cond_mean_plan).  The draw's (1 + N p) x N
// coefficients are staged once into LDS, in the global layout (equation i's column contiguous, so both the loads
// and the LDS writes are consecutive across the lanes) with the leading dimension made odd: at step k the lanes
// i < N read coef[i * stride + k], 8-byte reads on distinct banks.  The state is a ring of p + 1 blocks of N in
// LDS; every lane reads the same x[k] (a broadcast).  Lane i < N owns equation i.  A wave touches only its own
// part of the LDS, so the waves of a workgroup never wait for each other.  The kernel reads every stored
// coefficient once and computes 2 H N N p flops per draw: it is bound by that one pass over the store.
// Built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

#include "../../include/ccmm.h"
#include "ccmm_condmean.h"
#include "ccmm_err.h"
#include "ccmm_internal.h"

namespace ccmm {

namespace {

__host__ __device__ inline const double* cond_mean_src(const EigSrc& s, long long m) {
  return s.PAI + (m % s.na) * s.sa + (m / s.na) * s.sb;
}

// one wave as the lane group
struct CondMeanWave {
  static constexpr int W = 64;
  __device__ inline int lane() const { return threadIdx.x & 63; }
  // the wave's LDS writes are complete before any of its lanes reads them
  __device__ inline void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ inline int any(int bad) const { return __any(bad) ? 1 : 0; }
};

// the host twin's group: one lane
struct CondMeanSerial {
  static constexpr int W = 1;
  inline int lane() const { return 0; }
  inline void sync() const {}
  inline int any(int bad) const { return bad; }
};

__global__ __launch_bounds__(64 * kCondMeanMaxWaves) void k_cond_mean(int M, int N, int p, int H, EigSrc src,
                                                                      const double* __restrict__ y0, int ny0, int stride,
                                                                      int per, double* __restrict__ mean,
                                                                      int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double cond_mean_lds[];
  const int wave = threadIdx.x >> 6;
  const long long m = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (m >= M) return;  // whole waves only; no workgroup barrier follows
  double* coef = cond_mean_lds + (size_t)wave * per;
  double* ring = coef + (size_t)N * stride;
  const CondMeanWave g;
  const double* y = y0 + (ny0 == 1 ? 0 : (size_t)m * N * p);
  const int fl = cond_mean_core(g, cond_mean_src(src, m), src.ld, N, p, H, y, mean + (size_t)m * N, coef, stride, ring);
  if (g.lane() == 0) info[m] = fl;
}

}  // namespace

hipError_t cond_mean_launch(hipStream_t st, int M, int N, int p, int H, const EigSrc& src, const double* y0, int ny0,
                            double* mean, int* info) {
  const CondMeanPlan pl = cond_mean_plan(N, p, M);
  if (!pl.device || H < 1 || (ny0 != 1 && ny0 != M) || pl.grid > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_k(k_cond_mean, dim3((unsigned)pl.grid), dim3(pl.threads), pl.lds, pl.lds > kLdsDefault, st, M, N, p, H,
                  src, y0, ny0, pl.stride, (int)pl.per, mean, info);
}

void cond_mean_host(int M, int N, int p, int H, const EigSrc& src, const double* y0, int ny0, double* mean, int* info) {
  const size_t Np = (size_t)N * p;
  const int stride = (int)Np + 1;
  std::atomic<int> next{0};
  auto work = [&] {
    std::vector<double> coef((size_t)N * stride), ring(Np + N);
    const CondMeanSerial g;
    for (int m; (m = next++) < M;) {
      const int fl = cond_mean_core(g, cond_mean_src(src, m), src.ld, N, p, H, y0 + (ny0 == 1 ? 0 : (size_t)m * Np),
                                    mean + (size_t)m * N, coef.data(), stride, ring.data());
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

extern "C" int ccmm_cond_mean_host(int M, int N, int p, int K, int H, const double* PAI, const double* y0, int ny0,
                                   double* mean, int* info) {
  if (M < 0 || N < 1 || p < 1 || H < 1 || (long long)N * p + 1 > K || (ny0 != 1 && ny0 != M) ||
      (M > 0 && (!PAI || !y0 || !mean))) {
    ccmm::set_last_error("ccmm_cond_mean_host: need M >= 0, N, p, H >= 1, K >= 1 + N p, ny0 in {1, M}, PAI, y0 and mean");
    return CCMM_ERR_ARG;
  }
  const size_t ny = (size_t)(M > 0 ? ny0 : 0) * N * p;
  for (size_t e = 0; e < ny; ++e)
    if (!std::isfinite(y0[e])) {
      ccmm::set_last_error("ccmm_cond_mean_host: y0 must be finite");
      return CCMM_ERR_ARG;
    }
  try {
    ccmm::cond_mean_host(M, N, p, H, ccmm::EigSrc{PAI, K, M > 0 ? M : 1, (long long)K * N, 0}, y0, ny0, mean, info);
  } catch (const std::exception& e) {  // allocation or thread start
    ccmm::set_last_error(e.what());
    return CCMM_ERR_HIP;
  }
  return CCMM_OK;
}

// Compute_diagnostics on the device: IF, NSE and PSRF of stored draws (Diagnostics.m; core in ccmm_diagk.h).
//
// Mapping.  One lane owns one series; the 64 lanes of a wave sit on 64 consecutive entries of the draw store
// ([chain][capacity][entry]), so one draw of one wave is one 512-byte coalesced load.  Every draw is read once
// for momentg and for the sums of psrf's two sequences, and the first and last thirds once more for psrf's
// centred sums.  The loads do not depend on the arithmetic: kDiagAhead of them are issued before the first is
// used.  The 100 centred group means of the wave's series are [100][64] doubles of LDS, written and read by
// their own lane only: no barrier, no exchange between lanes, no wave waits on another.
//
// Built with -ffp-contract=off: ccmm_diagnostics_host (ccmm_diag.cpp) runs the same core and returns the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccmm_diagk.h"
#include "ccmm_internal.h"

namespace ccmm {

namespace {

struct DiagLds {
  double* p;
  __device__ inline double& operator()(int ig) const { return p[ig * kDiagWave]; }
};

__global__ __launch_bounds__(kDiagWave) void k_diag_series(const double* __restrict__ base, long long ld_draw,
                                                           long long ld_chain, int S, int C, int M,
                                                           const int* __restrict__ nvalid,
                                                           const uint8_t* __restrict__ mask,
                                                           double* __restrict__ out) {
  extern __shared__ double diag_cn[];  // [100][64]
  const int c = blockIdx.y;
  const long long e = diag_entry(blockIdx.x, threadIdx.x);
  if (e >= S || c >= C) return;
  const size_t ldo = (size_t)C * S;
  double* o = out + (size_t)c * S + e;
  const bool on = (!nvalid || e < nvalid[c]) && (!mask || mask[e]);
  if (!on) {
    for (int k = 0; k < kDiagNStat; ++k) o[k * ldo] = __builtin_nan("");
    return;
  }
  double st[kDiagNStat];
  diag_series(base + (size_t)c * ld_chain + e, ld_draw, M, DiagLds{diag_cn + threadIdx.x}, st);
  for (int k = 0; k < kDiagNStat; ++k) o[k * ldo] = st[k];
}

constexpr int kTrTile = 32;

// 32 x 32 tiles through LDS (one padding column): reads along m, writes along s
__global__ __launch_bounds__(kTrTile * 8) void k_diag_transpose(const double* __restrict__ in, int M, int S,
                                                                 double* __restrict__ out) {
  __shared__ double tile[kTrTile][kTrTile + 1];
  const int tx = threadIdx.x % kTrTile, ty = threadIdx.x / kTrTile;
  const int m0 = blockIdx.x * kTrTile, s0 = blockIdx.y * kTrTile;
  for (int r = ty; r < kTrTile; r += 8) {
    const int s = s0 + r, m = m0 + tx;
    if (s < S && m < M) tile[r][tx] = in[(size_t)s * M + m];
  }
  __syncthreads();
  for (int r = ty; r < kTrTile; r += 8) {
    const int m = m0 + r, s = s0 + tx;
    if (s < S && m < M) out[(size_t)m * S + s] = tile[tx][r];
  }
}

}  // namespace

hipError_t diag_launch(hipStream_t st, const double* base, long long ld_draw, long long ld_chain, int S, int C, int M,
                       const int* nvalid, const unsigned char* mask, double* out) {
  const DiagPlan pl = diag_plan(S, C);
  if (pl.grid_x == 0 || pl.grid_y == 0 || M < kDiagNG) return hipErrorInvalidValue;
  return launch_k(k_diag_series, dim3(pl.grid_x, pl.grid_y), dim3(pl.threads), pl.lds, false, st, base, ld_draw, ld_chain,
                  S, C, M, nvalid, mask, out);
}

hipError_t diag_transpose_launch(hipStream_t st, const double* in, int M, int S, double* out) {
  if (M < 1 || S < 1) return hipErrorInvalidValue;
  return launch_k(k_diag_transpose, dim3((M + kTrTile - 1) / kTrTile, (S + kTrTile - 1) / kTrTile), dim3(kTrTile * 8), 0,
                  false, st, in, M, S, out);
}

}  // namespace ccmm

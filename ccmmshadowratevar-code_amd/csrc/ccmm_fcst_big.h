// The predictive density of the large-N path (32 < N <= 128; its own translation unit, ccmm_fcst_big.hip): the plan
// of k_fcst_big and k_fcst_scores_big and their host launcher.  The plan functions make no HIP call
// (tests/test_fcst_big_plans.py checks them against a restatement).
//
// k_fcst_big batches the companion recursions of a chain as the columns of v_mfma_f64_16x16x4_f64: every forecast
// draw is a column pair (ring l, ring c) -- linear model: the unfloored and the floored recursion; block hybrid:
// the shadow lags and the same lags with the yields at max(shadow, ELB) -- and the linear model's zero-shock mean
// path one more column.  One workgroup takes `cols` columns of one chain (a whole number of draws), one wave per
// tile of 16 equations; the columns' lag rings (stride fcst_big_ring_stride) and the shock side of `hc` horizons
// of its cols / 2 draws live in LDS:
//   ring cols x stride | A (cols / 2) x hc x N | B (cols / 2) x hc x N | logSV (cols / 2) x N
#pragma once
#include "ccmm_bign.h"  // kBignMaxN, kNL
#include "ccmm_fcst.h"

namespace ccmm {

constexpr int kFcstBigMaxN = kBignMaxN;  // 128
constexpr int kFcstBigMaxK = 1536;       // K = N p + 1 of the large path
constexpr int kFcstBigHc = 16;           // horizons per shock chunk at most
constexpr int kFcstBigScoreThreads = 256;

// recursion columns of one chain: a pair per draw, and the linear model's mean path
__host__ __device__ inline int fcst_big_columns(int Nd, int bh) { return bh ? 2 * Nd : 2 * Nd + 1; }

// doubles between two columns' rings: p N rounded up to 2 mod 32, so that the 32 lanes of a half wave (16
// columns x 2 consecutive lags entries) read 32 different 8-byte banks
__host__ __device__ inline int fcst_big_ring_stride(int N, int p) { return (N * p - 2 + 31) / 32 * 32 + 2; }

__host__ __device__ inline size_t fcst_big_paths_lds_doubles(int N, int p, int cols, int hc) {
  return (size_t)cols * fcst_big_ring_stride(N, p) + 2 * (size_t)(cols / 2) * hc * N + (size_t)(cols / 2) * N;
}

// LDS of k_fcst_scores_big, the same at every N (wg_chol reads rows up to 127 of the matrix before it masks them):
//   M 128 x kNL | mu, y, sv1, dev 128 each | Ms kMvnMaxD x kFcstMaxN | res 8 | order, sel 128 ints each |
//   flags 8 ints | cens, yields 128 bytes each
__host__ __device__ inline size_t fcst_big_scores_lds_doubles() {
  return (size_t)kBignMaxN * kNL + 4 * 128 + kMvnMaxD * kFcstMaxN + 8 + 64 + 64 + 4 + 16 + 16;
}

struct FcstBigPlan {
  bool ok;         // false: even 8 columns at hc = 1 exceed one CU's LDS
  int cols;        // recursion columns per workgroup: 16, or 8 where 16 do not fit
  int hc;          // horizons per shock chunk: min(H, kFcstBigHc), halved until the workgroup fits
  int tiles;       // workgroups per chain (grid.x)
  int waves;       // row tiles of 16 equations = waves per workgroup
  size_t lds;      // bytes of k_fcst_big
  size_t lds_scores;
};

inline FcstBigPlan fcst_big_plan(int N, int p, int H, int Nd, int bh) {
  FcstBigPlan pl{};
  pl.waves = (N + 15) / 16;
  pl.lds_scores = fcst_big_scores_lds_doubles() * sizeof(double);
  for (int cols = 16; cols >= 8 && !pl.ok; cols /= 2) {
    int hc = std::min(H, kFcstBigHc);
    while (hc > 1 && fcst_big_paths_lds_doubles(N, p, cols, hc) * sizeof(double) > kLdsCu) hc = (hc + 1) / 2;
    pl.cols = cols;
    pl.hc = hc;
    pl.lds = fcst_big_paths_lds_doubles(N, p, cols, hc) * sizeof(double);
    pl.ok = pl.lds <= kLdsCu;
  }
  pl.tiles = (fcst_big_columns(Nd, bh) + pl.cols - 1) / pl.cols;
  return pl;
}

// bytes of PAI one kept draw of one chain reads: every workgroup streams the lag rows once per horizon
inline size_t fcst_big_pai_bytes(int N, int p, int H, int Nd, int bh) {
  return (size_t)fcst_big_plan(N, p, H, Nd, bh).tiles * H * N * p * N * sizeof(double);
}

// k_fcst_big then k_fcst_scores_big of one kept draw per chain (a.bh = 0 or 1, no IRF form); sets a.hc and a.sv1.
// Throws std::runtime_error when the plan does not fit one CU's LDS, before any launch
hipError_t launch_fcst_big(hipStream_t st, FcstArgs& a, double* sv1);

}  // namespace ccmm

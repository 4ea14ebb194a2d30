// Workgroup primitives of the large-N path on one N x N LDS matrix (row-major, row stride kNL, N <= 128), shared by
// the Gibbs blocks (ccmm_bign.hip) and the predictive-density scores (ccmm_fcst_big.hip): the blocked Cholesky and
// the one-vector lower-triangular solve.
#pragma once
#include "ccmm_bign.h"

namespace ccmm {

constexpr int kPB = 16;    // Cholesky panel width (16: no spills at 1024 threads)

// ---------------------------------------------------------------- Cholesky (LDS)
// In place on the lower triangle of S (n x n, ld kNL, n <= 128): blocked right-looking with
// 16-wide panels (kPB).  Wave 0 factors the diagonal block (lane = row, readlane broadcasts);
// the panel below and the trailing update use every thread.  Upper triangle zeroed.
// *bad set on a non-positive pivot (the pivot is then taken as 1).
template <int NT>
__device__ void wg_chol(double* S, int n, int* bad) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int p0 = 0; p0 < n; p0 += kPB) {
    const int pw = min(kPB, n - p0);
    if (wave == 0) {
      double row[kPB];
#pragma unroll
      for (int m = 0; m < kPB; ++m) row[m] = (lane < pw && m <= lane && m < pw) ? S[(p0 + lane) * kNL + p0 + m] : 0.0;
#pragma unroll
      for (int kk = 0; kk < kPB; ++kk) {
        if (kk < pw) {
          double dkk = readlane_d(row[kk], kk);
          if (!(dkk > 0.0)) {
            *bad = 1;
            dkk = 1.0;
          }
          const double piv = sqrt(dkk);
          if (lane == kk) row[kk] = piv;
          if (lane > kk) row[kk] /= piv;
          const double lik = row[kk];
#pragma unroll
          for (int m = kk + 1; m < kPB; ++m) {
            const double lmk = readlane_d(lik, m);
            if (lane >= m) row[m] = fma(-lik, lmk, row[m]);
          }
        }
      }
      if (lane < pw)
#pragma unroll
        for (int m = 0; m < kPB; ++m)
          if (m < pw) S[(p0 + lane) * kNL + p0 + m] = (m <= lane) ? row[m] : 0.0;
    }
    __syncthreads();
    // panel: L(i, p0:p0+pw) = S(i, p0:p0+pw) L_pp^{-T}, thread per row i >= p0 + pw
    for (int i = p0 + pw + tid; i < n; i += NT) {
      double x[kPB];
#pragma unroll
      for (int m = 0; m < kPB; ++m) x[m] = (m < pw) ? S[i * kNL + p0 + m] : 0.0;
#pragma unroll
      for (int m = 0; m < kPB; ++m) {
        if (m < pw) {
          double s = x[m];
#pragma unroll
          for (int q = 0; q < m; ++q) s = fma(-x[q], S[(p0 + m) * kNL + p0 + q], s);
          x[m] = s / S[(p0 + m) * kNL + p0 + m];
        }
      }
#pragma unroll
      for (int m = 0; m < kPB; ++m)
        if (m < pw) S[i * kNL + p0 + m] = x[m];
    }
    __syncthreads();
    // trailing update: S(i, j) -= L(i, panel) . L(j, panel), i >= j >= p0 + pw; 4 x 4 tiles
    const int r0 = p0 + pw, nr = n - r0;
    const int mt = (nr + 3) / 4, ntile = mt * (mt + 1) / 2;
    for (int tile = tid; tile < ntile; tile += NT) {
      int ti = 0, tj = tile;
      while (tj > ti) {
        tj -= ti + 1;
        ++ti;
      }
      const int a0 = r0 + 4 * ti, b0 = r0 + 4 * tj;
      double acc[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.0;
      for (int m = 0; m < pw; ++m) {
        double la[4], lb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          la[i] = S[min(a0 + i, 127) * kNL + p0 + m];
          lb[i] = S[min(b0 + i, 127) * kNL + p0 + m];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[i * 4 + jj] = fma(la[i], lb[jj], acc[i * 4 + jj]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          if (a0 + i < n && b0 + jj <= a0 + i) S[(a0 + i) * kNL + b0 + jj] -= acc[i * 4 + jj];
    }
    __syncthreads();
  }
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    if (j > i) S[i * kNL + j] = 0.0;
  }
  __syncthreads();
}

// ---------------------------------------------------------------- one-vector solves (wave 0)
// L (n x n lower, row stride ld, LDS or global), v (LDS, n): v <- L^{-1} v  or  L^{-T} v.
// Lanes own rows lane and lane + 64.  Called by wave 0 only.
__device__ inline void wave_trsv_lower(const double* L, int ld, double* v, int n) {
  const int lane = threadIdx.x & 63;
  double r0 = lane < n ? v[lane] : 0.0, r1 = lane + 64 < n ? v[lane + 64] : 0.0;
  for (int k = 0; k < n; ++k) {
    const double vk = (k < 64 ? readlane_d(r0, k) : readlane_d(r1, k - 64)) / L[(size_t)k * ld + k];
    if (k < 64 && lane == k) r0 = vk;
    if (k >= 64 && lane == k - 64) r1 = vk;
    if (lane > k && lane < n) r0 = fma(-L[(size_t)lane * ld + k], vk, r0);
    if (lane + 64 > k && lane + 64 < n) r1 = fma(-L[(size_t)(lane + 64) * ld + k], vk, r1);
  }
  if (lane < n) v[lane] = r0;
  if (lane + 64 < n) v[lane + 64] = r1;
}

}  // namespace ccmm

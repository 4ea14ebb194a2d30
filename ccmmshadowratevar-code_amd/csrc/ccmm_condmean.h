// Conditional mean path of VAR coefficient draws (ccmm_condmean.hip): for each of M matrices PAI (K x N
// column-major) and a jump-off state y0 (N p doubles, p blocks of N in the order of the companion state),
//
//   x_0 = y0,   x_{h+1} = c~ + comp x_h,   c~ = [PAI(0, :)'; 0],   mean = x_H(1:N)
//
// (doVARshadowrateBlockHybridMissingData.m:433-468 thatMean = ((I - comp) \ (I - comp^H)) c~ + comp^H y0, which is
// x_H whenever I - comp is nonsingular; the recursion needs no solve and no power).  The lower block of the
// companion is a shift, so a step is N equations
//
//   y_i = PAI(0, i) + sum_{k = 0 .. N p - 1} PAI(1 + k, i) x[k]
//
// and the new state [y; x[0 .. N p - N - 1]].
//
// One core, two builds.  Every y_i is one fp64 fused multiply-add chain that starts from the intercept and runs
// over k ascending; the shift is a ring head.  So the bits of a draw depend on its own PAI and y0 only, not on
// the batch or the build: the kernel (one wave per draw, lane i owns equation i) and the host twin return the
// same bits.  Built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ccmm_eig.h"  // EigSrc, kEigMaxN

namespace ccmm {

// ---- launch arithmetic (host, no HIP call)
constexpr int kCondMeanMaxN = 32;            // device path: N <= 32 (one lane per equation, half a wave at most) ...
constexpr int kCondMeanMaxNp = kEigMaxN;     // ... and N p <= 256, the range of the root and VMA kernels
constexpr int kCondMeanMaxWaves = 4;         // draws (waves) of a workgroup, at most
constexpr size_t kCondMeanLdsCap = 128 * 1024;  // dynamic LDS of a workgroup, at most

struct CondMeanPlan {
  int device;     // 1: the device path serves this shape; 0: the host twin
  int stride;     // doubles between the coefficient columns of two equations in LDS: 1 + N p made odd, so that
                  // the lanes' 8-byte reads of one k fall on distinct banks
  size_t per;     // doubles of one draw in LDS: N * stride coefficients and the ring of p + 1 blocks of N
  int waves;      // draws per workgroup
  int threads;    // 64 * waves
  size_t lds;     // dynamic LDS of a workgroup in bytes (a multiple of 16)
  long long grid; // workgroups: ceil(M / waves)
};
inline CondMeanPlan cond_mean_plan(int N, int p, long long M) {
  CondMeanPlan pl{};
  if (N < 1 || p < 1 || M < 1) return pl;
  const long long Np = (long long)N * p;
  pl.device = N <= kCondMeanMaxN && Np <= kCondMeanMaxNp;
  if (!pl.device) return pl;
  pl.stride = (int)((Np + 1) | 1);
  pl.per = ((size_t)N * pl.stride + (size_t)Np + N + 1) & ~(size_t)1;  // even: every draw's base stays 16-byte aligned
  const size_t fit = kCondMeanLdsCap / (pl.per * sizeof(double));
  pl.waves = (int)(fit < 1 ? 1 : (fit < (size_t)kCondMeanMaxWaves ? fit : (size_t)kCondMeanMaxWaves));
  if ((long long)pl.waves > M) pl.waves = (int)M;
  pl.threads = 64 * pl.waves;
  pl.lds = pl.per * sizeof(double) * pl.waves;
  pl.grid = (M + pl.waves - 1) / pl.waves;
  return pl;
}

// ---- the core
// Storage of one draw: coef[i * stride + r] = PAI(r, i), r = 0 .. N p (the global layout with the leading
// dimension replaced), ring[b * N + c]: block b of p + 1 blocks of N (the state and one free block).
// The group G has lane(), W, sync() (the group's writes to coef and ring become visible to its lanes) and
// any(bad), the OR over the lanes.  Returns 1 when a coefficient or intercept in rows 0 .. N p is not finite
// (mean = NaN), else 0.  y0: N p doubles.  mean: N doubles.
template <class G>
__host__ __device__ inline int cond_mean_core(const G& g, const double* PAI, int ld, int N, int p, int H,
                                              const double* y0, double* mean, double* coef, int stride,
                                              double* ring) {
  const int Np = N * p, R = Np + 1;
  int bad = 0;
  for (int e = g.lane(); e < R * N; e += G::W) {
    const int i = e / R, r = e - i * R;
    const double v = PAI[(size_t)i * ld + r];
    bad |= !(fabs(v) <= 1.79769313486231570815e308);
    coef[i * stride + r] = v;
  }
  for (int e = g.lane(); e < Np; e += G::W) ring[e] = y0[e];
  bad = g.any(bad);
  g.sync();
  if (bad) {
    for (int i = g.lane(); i < N; i += G::W) mean[i] = __builtin_nan("");
    return 1;
  }
  // the ring has p + 1 blocks: state block l is ring block (head + l) mod (p + 1), and the new y goes into the one
  // block that the step does not read, which then becomes the head
  int head = 0;
  for (int h = 0; h < H; ++h) {
    const int free = head == 0 ? p : head - 1;
    for (int i = g.lane(); i < N; i += G::W) {  // one pass on the device (W = 64 > N); N on the host twin
      const double* ci = coef + (size_t)i * stride;
      double acc = ci[0];
      int k = 1;
      for (int l = 0, b = head; l < p; ++l, b = b == p ? 0 : b + 1) {
        const double* x = ring + b * N;
        for (int c = 0; c < N; ++c, ++k) acc = __builtin_fma(ci[k], x[c], acc);
      }
      ring[free * N + i] = acc;
    }
    g.sync();
    head = free;
  }
  for (int i = g.lane(); i < N; i += G::W) mean[i] = ring[head * N + i];
  return 0;
}

// ---- the two builds
// y0 of draw m: y0 + (ny0 == 1 ? 0 : m) * N p
// host twin: M draws on at most 16 threads; mean[m * N + i]; info may be null
void cond_mean_host(int M, int N, int p, int H, const EigSrc& src, const double* y0, int ny0, double* mean, int* info);
// device: draws m = 0..M-1 at src, y0 (ny0 x N p), mean (M x N), info (M, not null), all on the device
hipError_t cond_mean_launch(hipStream_t st, int M, int N, int p, int H, const EigSrc& src, const double* y0, int ny0,
                            double* mean, int* info);

}  // namespace ccmm

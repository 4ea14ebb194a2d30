// Generalized impulse responses by antithetic simulation on the device (ccmm_girf.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ccmm {

struct GirfArgs {
  int M, N, p, H, nsim, bh, Ny;  // MCMC draws, variables, lags, horizons, shock paths, model
                                 // (bh: 0 linear, 1 block hybrid, 2 hybrid: the ring holds the Ny
                                 // shadow-rate variables and PAI has K + Ny p rows per equation)
  const double* PAI;             // device [M][N][K]
  const double* invA;            // device [M][N][N]
  const double* sqrtPHI;         // device [M][N][N] lower Cholesky of PHI
  const double* SV0;             // device [M][N] jump-off sqrtht
  const double* Xj;              // device [M][ldX] Xjumpoff
  int ldX;
  const uint8_t* actual;         // device [N] actualrateBlock (block hybrid) or null
  const int* yidx;               // device [Ny] ring variables (block hybrid: yields; hybrid: shadow rates)
  const uint8_t* yfloor;         // device [N] variables floored at the ELB in the output (ndxYIELDS) or null
  double elb, shock11;
  const double* z;               // device [M][nsim][H][N] or null (Philox)
  const double* svz;             // device [M][nsim][H][N] or null
  uint64_t seed;
  const uint8_t* cumcode;        // device [N] or null
  double np_;
  double* part;                  // device workspace [M][3][ceil(nsim/4)][H][N]
  double* out;                   // device [M][3][H][N]: baseline, +shock, -shock mean paths
  int force_generic;             // 1: the table-driven kernel even where a specialised one exists
  int m0;                        // Philox stream id of draw 0 (draw m takes m0 + m); z, svz, part and out are
                                 // indexed from 0 whatever m0 is
};

// ---- launch arithmetic (host, no HIP call; tests/launch_plans_main.cpp prints it)
constexpr int kGirfSims = 16;  // simulations per workgroup: 4 paths x 4 antithetic shock sets
constexpr int kGirfFastP = 12, kGirfFastN4 = 20;  // the shape k_girf_fast is compiled for (NY4 = 0, 4, 8)
constexpr int kGirfMaxKs = 96;  // largest k_girf<KS> bucket: K + Ny p + N <= 384 state rows

// dynamic LDS of k_girf<KS> (byte offsets): X [nks * 4][16] | logsv [4][N] | ybuf [N][16] | nrm [2][4][N] |
// rowtab [p][nks * 4] ints
struct GirfLds {
  size_t X, logsv, ybuf, nrm, rowtab, end;
};
inline GirfLds girf_lds(int N, int p, int nks) {
  GirfLds l{};
  l.logsv = l.X + (size_t)nks * 4 * kGirfSims * sizeof(double);
  l.ybuf = l.logsv + (size_t)4 * N * sizeof(double);
  l.nrm = l.ybuf + (size_t)N * kGirfSims * sizeof(double);
  l.rowtab = l.nrm + (size_t)8 * N * sizeof(double);
  l.end = l.rowtab + (size_t)p * nks * 4 * sizeof(int);
  return l;
}
// dynamic LDS of k_girf_fast<P, N4, NY4>: X [P (N4 + NY4) + N4 + 4][16] | logsv | ybuf | nrm as above, no table
inline GirfLds girf_fast_lds(int N, int P, int N4, int NY4) {
  GirfLds l{};
  l.logsv = l.X + (size_t)(P * (N4 + NY4) + N4 + 4) * kGirfSims * sizeof(double);
  l.ybuf = l.logsv + (size_t)4 * N * sizeof(double);
  l.nrm = l.ybuf + (size_t)N * kGirfSims * sizeof(double);
  l.rowtab = l.end = l.nrm + (size_t)8 * N * sizeof(double);
  return l;
}

// the kernel girf_launch takes for N variables, p lags and Ny ring variables (0: linear)
struct GirfPlan {
  int fast_ny4;  // NY4 of k_girf_fast<12, 20, NY4>, or -1: the table-driven k_girf<ks>
  int ks;        // k_girf<KS> bucket 32, 64 or 96 (0 with a fast kernel, or when nks exceeds the largest)
  int nks;       // 4-row k-steps of the generic state: ceil((1 + N p + Ny p + N) / 4)
  int threads;   // one wave per 16 equations
  size_t lds;    // dynamic LDS bytes of the kernel taken
};
inline GirfPlan girf_plan(int N, int p, int Ny, bool force_generic) {
  GirfPlan pl{};
  pl.nks = (1 + N * p + Ny * p + N + 3) / 4;
  pl.threads = 64 * ((N + 15) / 16);
  const int N4 = (N + 3) / 4 * 4, NY4 = (Ny + 3) / 4 * 4;
  if (!force_generic && p == kGirfFastP && N4 == kGirfFastN4 && NY4 <= 8) {
    pl.fast_ny4 = NY4;
    pl.lds = girf_fast_lds(N, p, N4, NY4).end;
    return pl;
  }
  pl.fast_ny4 = -1;
  pl.ks = pl.nks <= 32 ? 32 : (pl.nks <= 64 ? 64 : (pl.nks <= kGirfMaxKs ? 96 : 0));
  pl.lds = girf_lds(N, p, pl.nks).end;
  return pl;
}

hipError_t girf_launch(hipStream_t st, const GirfArgs& a);

}  // namespace ccmm

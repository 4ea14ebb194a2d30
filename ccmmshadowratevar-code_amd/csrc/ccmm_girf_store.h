// Generalized impulse responses of the stored draws of a chain set (ccmm_girf_store.hip, ccmm_chains_girf.hip):
// the inputs of the simulation (ccmm_girf.h GirfArgs) taken from the draw stores in place, the Rao-Blackwellised
// linear responses (generateGIRF2linear.m:175-216) and the series sets the scripts summarise.
//
//   k_girf_prep     one wave per stored draw: Xjumpoff (generateGIRF2linear.m:227-231,
//                   generateGIRF2blockhybrid.m:204-218, generateGIRF2hybrid.m:203-217), SV0 = the jump-off row of
//                   sqrtht_all, sqrtPHI = chol(ivech(PHI), 'lower')
//   k_girf_rb       one wave per stored draw (linear model): YhatRBdraws and IRF1RBdraws, cumulated
//   k_girf_collect  the mean paths of one pass -> the series-major segments post_summaries reads
//
// Draws are pooled over the C chains of a data slot, chain slowest: d = c * stored + m (the order of
// ccmm_chains_vma_summaries).  Draw d is simulated with Philox stream d whatever the pass it falls in.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ccmm {

// ---- plan arithmetic (host, no HIP call; tests/girf_store_plan_main.cpp prints it)
// the simulation workspace of one pass (part + out of GirfArgs): at most 1 GB = 1e9 bytes, inside the 2^30 bytes
// kVmaBufCap allows the buffers of a VMA pass
constexpr size_t kGirfPassCap = (size_t)1000000000;
constexpr int kGirfSets = 5;    // base, plus, minus, plus - base, minus - base
constexpr int kGirfRbSets = 2;  // YhatRBdraws, IRF1RBdraws (linear model)

// bytes of part [3][ceil(nsim / 4)][H][N] and out [3][H][N] of one draw
inline size_t girf_draw_bytes(int N, int H, int nsim) {
  const size_t nch = (size_t)(nsim + 3) / 4;
  return ((size_t)3 * nch * H * N + (size_t)3 * H * N) * sizeof(double);
}

struct GirfPassPlan {
  size_t per;     // workspace bytes of one draw
  int draws;      // draws per pass: the most within the cap and at least 1, or the caller's figure
  int npass;      // passes over n draws
  int last;       // draws of the last pass
  size_t bytes;   // workspace of a full pass
};
// n pooled draws; want > 0 overrides the draws per pass (clamped to n)
inline GirfPassPlan girf_pass_plan(long long n, int N, int H, int nsim, int want, size_t cap = kGirfPassCap) {
  GirfPassPlan pl{};
  pl.per = girf_draw_bytes(N, H, nsim);
  if (n < 1) return pl;
  long long fit = want > 0 ? want : (long long)(cap / pl.per);
  if (fit < 1) fit = 1;
  if (fit > n) fit = n;
  pl.draws = (int)fit;
  pl.npass = (int)((n + fit - 1) / fit);
  pl.last = (int)(n - (long long)(pl.npass - 1) * fit);
  pl.bytes = pl.per * (size_t)pl.draws;
  return pl;
}

// dynamic LDS of k_girf_prep (PHI / its factor, N x N) and of k_girf_rb (N coefficient columns of stride 1 + N p
// made odd, so that the lanes' reads of one k fall on distinct banks, and the ring of p + 1 blocks of N)
inline size_t girf_prep_lds(int N) { return (size_t)N * N * sizeof(double); }
inline int girf_rb_stride(int N, int p) { return (1 + N * p) | 1; }
inline size_t girf_rb_lds(int N, int p) {
  return ((size_t)N * girf_rb_stride(N, p) + (size_t)(p + 1) * N) * sizeof(double);
}

// ---- the kernels' arguments
struct GirfPrepArgs {
  int n, C, stored, cap;     // pooled draws C * stored; the chains' stores are cap draws apart
  int N, p, T;               // T: rows of one stored sqrtht draw (the set's largest T)
  int Ns, elbTmax, Ny, ring; // ring: 0 none (linear), 1 the Ny variables of yidx follow the lags in Xj
  int ldX;                   // 1 + N p + Ny p
  int svrow;                 // 0-based row of sqrtht: t0 - p
  int npatch;                // n = ndxIRFT0 - elbT0 - p: lag l of a shadow-rate variable is month npatch - 1 - l of
                             // the draw's shadow rates when that is >= 0
  const double* sPHI;        // the slot's first chain: [C][cap][N (N + 1) / 2]
  const double* sSqrtht;     // [C][cap][T N], t fastest
  const double* sShadow;     // [C][cap][elbTmax Ns], rate fastest; null without a patch
  const double* jump;        // [p][N]: the data of months t0, t0 - 1, ..
  const int* ndxS;           // [Ns] shadow-rate variables
  const int* yidx;           // [Ny] ring variables
  double* Xj;                // [n][ldX]
  double* SV0;               // [n][N]
  double* sqrtPHI;           // [n][N][N]: L(i, j) at i + j N, zeros above the diagonal
  int* info;                 // [n]: 1 = PHI not positive definite or not finite (the draw's outputs are NaN)
};

struct GirfRbArgs {
  int n, C, stored, cap, N, p, K, H;  // K: rows of one stored PAI column (1 + N p)
  const double* sPAI;      // [C][cap][N][K]
  const double* sInvA;     // [C][cap][N][N]
  const double* Xj;        // [n][ldX] of k_girf_prep
  int ldX;
  const int* info;         // [n] of k_girf_prep
  double shock11;
  const uint8_t* cumcode;  // [N] or null
  double np_;
  double* rb;              // [n][2][H][N]: YhatRBdraws, IRF1RBdraws
};

hipError_t girf_prep_launch(hipStream_t st, const GirfPrepArgs& a);
hipError_t girf_rb_launch(hipStream_t st, const GirfRbArgs& a);
// out [mc][3][H][N] of the pass that starts at pooled draw d0 -> seg [5][S][n], S = H N, series h N + i:
// seg[(set S + s) n + d0 + m]
hipError_t girf_collect_launch(hipStream_t st, int mc, int d0, int n, int S, const double* out, double* seg);
// rb [n][2][S] -> seg [2][S][n]
hipError_t girf_collect_rb_launch(hipStream_t st, int n, int S, const double* rb, double* seg);

}  // namespace ccmm

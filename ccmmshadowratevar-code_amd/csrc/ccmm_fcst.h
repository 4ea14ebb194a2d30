// Arguments, LDS budgets and the host launchers of the predictive-density kernels (their own translation unit,
// ccmm_fcst.hip, which launches every one of them).  The size and decision functions make no HIP call.
#pragma once
#include <algorithm>

#include "ccmm_internal.h"
#include "ccmm_elb.h"  // kElbNsMax

namespace ccmm {

constexpr int kFcstMaxN = 32;
constexpr int kMvnMaxD = 12;         // series at the ELB the censored scores take (mvn_lattice_cdf, ccmm_fcst_dev.h)
constexpr int kMvnPts = 64 * 1024;   // points of its lattice rule

struct GLNodes {  // Gauss-Legendre half rules (negative nodes) for n = 6, 12, 20 (Genz BVN)
  double x[3][10];
  double w[3][10];
};

struct FcstArgs {
  int B, N, p, K, H, Nd;
  int bh;                 // 1: block-hybrid companion (mcmcVARshadowrateBlockHybrid.m:147-159,566-625);
                          // 2: hybrid (mcmcVARhybridGibbs.m:160-172,566-635): PAI has Kx = K + Ns p
                          //    rows, the last Ns p multiply the Ns actual-rate lags max(shadow, ELB)
  int Kx;                 // rows of PAI used (K, or K + Ns p for the hybrid model)
  int Ns;                 // hybrid: shadow-rate variables
  const int* ndxS;        // hybrid: [Ns] their indices
  const double* PAI;      // [B][N][ldPAI]  (Kx x N column-major per chain, ld Kx or KP)
  int ldPAI;
  const double* invA;     // [B][N][N]
  const double* logSV;    // logSV0(c, i) = logSV[(c N + i) ldSV + (svT ? svT[slot c] - 1 : 0)]
  int ldSV;
  const int* svT;         // per-slot T (chain set: Vol_states(end,:) of the vintage) or nullptr
  const int* slot;        // [B] data slot of chain c, or nullptr (slot 0)
  const double* sqrtPHI;  // [B][N][N]
  const double* Xj;       // [B][ldXj] Xjumpoff: K states [1, y(T), .., y(T-p+1)]; block hybrid:
  int ldXj;               //   then p blocks of N actual-data lags Xj[K + l N + i] (:88-96,511-520);
                          //   hybrid: p blocks of Ns floored actual rates Xj[K + l Ns + s] (:111-121)
  const double* yreal;    // yrealized(:,1) of chain c at yreal + slot(c) * ldY
  int ldY;
  const uint8_t* ndxYields;  // [N]
  const uint8_t* recFloor;   // [N] linear model: variables floored inside the censored recursion
                             //   (nullptr: ndxYields, mcmcVAR.m:360-366; mcmcVARshadowrate.m:539-546
                             //   floors ndxOTHERYIELDS only)
  const uint8_t* actual;     // [N] actualrateBlock (bh) or nullptr
  double elb;
  const double* svz;      // randn(N, H*Nd) of chain c at svz + c * crnStride, or nullptr (Philox)
  const double* z;        // randn(N, H, Nd) of chain c at z + c * crnStride, or nullptr
  int64_t crnStride;
  uint64_t seed;
  uint32_t sweep;
  const uint32_t* ids;    // Philox stream id of chain c, or nullptr (c)
  double* fY;             // [B][Nd][H][N]  simulated paths (bh: uncensored)
  double* fYc;            // [B][Nd][H][N]  censored simulation (bh: yields floored at the ELB)
  double* yhat;           // [B][H][N]      zero-shock mean path (linear only)
  double* scores;         // [B][Nd][4]
  int* status;            // [B]  bit 1: NaN score (more than kMvnMaxD censored series)
  GLNodes gl;
  int mode;               // kFcst* bits below; 0 in production
  int hc;                 // horizons per shock chunk of k_fcst (fcst_paths_lds_doubles)
  double* sv1;            // [B][Nd][N] SV at horizon 1 of each draw (k_fcst -> k_fcst_scores)
  // doIRF1 (mcmcVARshadowrateBlockHybrid.m:627-664, mcmcVARhybridGibbs.m:638-675, mcmcVARshadowrate.m:588-605):
  // on when fY1p is set.  The draw's simulation run twice more on the same shocks, with the first variable's
  // structural shock at horizon 1 replaced by +irfScale / -irfScale (the value itself, not times the volatility)
  double irfScale;
  double* fY1p;           // [B][Nd][H][N]  raw plus paths (bh: the shadow recursion, unfloored; linear: ltitr)
  double* fY1m;           // [B][Nd][H][N]  raw minus paths
};

// bits of FcstArgs::mode: none selects what is computed; both are timing-only (CCMM_FCST_MODE, ablation build;
// results invalid): k_fcst_scores returns at once, k_fcst simulates no horizon
constexpr int kFcstNoScores = 1, kFcstNoHorizons = 2;

// k_fcst<kFcstRegN> (N <= 21, p <= 3 kFcstRegLags, not hybrid) holds each lane's PAI column
// entries for its lags in registers instead of staging PAI in LDS: the lag sums then read only
// the ring from LDS, and the workgroup's LDS drops from ~52 KB to ~18 KB (hc <= 16) so that
// eight waves share a CU instead of three.  Same fma order, same sums.
constexpr int kFcstRegN = 21, kFcstRegLags = 4;  // k_fcst<20>: the same for even N <= 20

__host__ __device__ inline bool fcst_reg_path(int N, int p, int bh) {
  return N <= kFcstRegN && p <= 3 * kFcstRegLags && bh != 2;
}

__host__ __device__ inline size_t fcst_paths_lds_doubles(int N, int Kx, int p, int hc, bool reg = false) {
  return (reg ? 0 : (size_t)Kx * N) + 2 * (size_t)N * N + 2 * (size_t)p * N + 3 * (size_t)hc * N;
}

__host__ __device__ inline size_t fcst_scores_lds_doubles(int N) {
  return 2 * (size_t)N * N + 6 * (size_t)N + kFcstMaxN * kFcstMaxN;
}

// horizons per shock chunk so that k_fcst's LDS fits one CU (at most H; at least 1)
// (the register path: at most 16 horizons, so that eight workgroups share a CU)
inline int fcst_chunk(int N, int Kx, int p, int H, bool reg = false) {
  int hc = reg ? std::min(H, 16) : H;
  while (hc > 1 && fcst_paths_lds_doubles(N, Kx, p, hc, reg) * sizeof(double) > kLdsCu) hc = (hc + 1) / 2;
  return hc;
}

// The IRF form k_fcst<RN, true> runs the plus and the minus recursion beside the baseline in the same wave; each
// has a ring pair of its own after the shock chunks (the linear model's plus / minus runs are the unfloored
// recursion only: one ring each):
//   [PAI Kx N (LDS form)] sqrtPHI N N | invA N N | ringl p N | ringc p N | W hc N | NU hc N | DV hc N |
//   bh = 0:  ringl+ p N | ringl- p N
//   bh > 0:  ringl+ p N | ringc+ p N | ringl- p N | ringc- p N
__host__ __device__ inline size_t fcst_irf_rings(int bh) { return bh ? 4 : 2; }

__host__ __device__ inline size_t fcst_irf_lds_doubles(int N, int Kx, int p, int hc, bool reg, int bh) {
  return fcst_paths_lds_doubles(N, Kx, p, hc, reg) + fcst_irf_rings(bh) * (size_t)p * N;
}

// fcst_chunk for the IRF form
inline int fcst_irf_chunk(int N, int Kx, int p, int H, bool reg, int bh) {
  int hc = reg ? std::min(H, 16) : H;
  while (hc > 1 && fcst_irf_lds_doubles(N, Kx, p, hc, reg, bh) * sizeof(double) > kLdsCu) hc = (hc + 1) / 2;
  return hc;
}

// the k_fcst<RN> instance launch_fcst takes: kFcstRegN - 1 (even N below kFcstRegN), kFcstRegN (the other
// register-path shapes) or 0 (PAI in LDS).  reg_opt: option fcst_reg
inline int fcst_variant(int N, int p, int bh, bool reg_opt) {
  const bool reg = fcst_reg_path(N, p, bh) && reg_opt;
  return !reg ? 0 : (N % 2 == 0 && N < kFcstRegN ? kFcstRegN - 1 : kFcstRegN);
}

// k_fcst<RN> then k_fcst_scores of one kept draw per chain; sets a.hc and a.sv1.  reg_opt: option fcst_reg.
// With a.fY1p set the IRF form k_fcst<RN, true> on the plan of fcst_irf_chunk / fcst_irf_lds_doubles; else the
// kernels, grid, LDS size and hc of the plain form.  Throws std::runtime_error when the paths' state does not fit one CU's LDS
hipError_t launch_fcst(hipStream_t st, FcstArgs& a, double* sv1, bool reg_opt);
// Xjumpoff of every chain from its Y slab (and, block hybrid / hybrid with Ns > 0, the slot's actual data); one
// workgroup per chain
// (a: sizes, slot, Ns, ndxS, elb and ldXj; Xj is written)
hipError_t launch_fcst_jumpoff(hipStream_t st, const FcstArgs& a, int TP, const int* Tslot, const double* ypool,
                               const int* yidx, double* Xj);
// the kept draw's paths a.fY, a.fYc (and yhat when given) into the running sums, its scores (and paths) into the
// store at index m
hipError_t launch_fcst_accum(hipStream_t st, const FcstArgs& a, int cap, int m, const double* yhat, double* sum,
                             double* sumc, double* sumhat, double* scStore, double* paths, double* pathsc);
// the kept draw's IRF1 records from a.fY, a.fY1p, a.fY1m (after launch_fcst): recP / recM [B][cap][H][N] at index
// m, the running sums sumP / sumM [B][H][N], and (when given) the raw paths into pathsP / pathsM at index m.
// cumcode: [N] rows cumulated over the horizons; tmp: [B][2][H][N] scratch
hipError_t launch_fcst_irf_accum(hipStream_t st, const FcstArgs& a, int cap, int m, const uint8_t* cumcode,
                                 double* recP, double* recM, double* sumP, double* sumM, double* tmp, double* pathsP,
                                 double* pathsM);

}  // namespace ccmm

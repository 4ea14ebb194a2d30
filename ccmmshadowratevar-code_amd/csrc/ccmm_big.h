// Large-system CTA (ccmm_big.hip, its own translation unit): host launchers used by
// ccmm_chains_sweep.hip when K > 512 or N > 32 (the S120 configuration N = 120, K = 1441).
#pragma once
#include "ccmm_internal.h"

namespace ccmm {

constexpr int kBigMaxN = 128;
constexpr int kBigMaxKP = 1536;

constexpr int kBSLd = 65;       // LDS row stride of the solve's 64 x 64 diagonal-block inverse
constexpr int kResSlices = 8;   // column slices of the residual phase X x
// staged twin (KP <= kStageMaxKP): the X'v and residual phases read the lag twin from LDS, 256 months
// (plus the p - 1 presample rows their lags reach) at a time, instead of one L2 load per product
constexpr int kStageMonths = 256;
constexpr int kStageMaxKP = 320;
__host__ __device__ inline int big_stage_rows(int p) { return kStageMonths + p; }

// dynamic LDS of k_cta_solve_big without a staged twin:
//   v [TP] | yv [KP] | rdl [KP] | Ls [64 x kBSLd] | part [kResSlices x TP]
inline size_t big_solve_lds_bytes(const Dims& d) {
  return (size_t)(d.TP + 2 * d.KP + 64 * kBSLd + kResSlices * d.TP) * sizeof(double);
}
// the staged twin after them: Ds [ncol x big_stage_rows(p)] | loff [KP ints]
inline size_t big_stage_lds_doubles(const Dims& d, int ncol) {
  return (size_t)ncol * big_stage_rows(d.p) + (d.KP + 1) / 2;
}
// The solve's choice between three branches: the twin (ncol columns) staged in LDS; a twin read from L2 because
// KP > kStageMaxKP (the kernel keeps kStageMaxKP / 64 column sums per wave); a twin read from L2 because the staged
// size exceeds one CU's LDS.  Without a twin the kernel reads X itself.  A shape whose unstaged size alone exceeds
// kLdsCu is not refused here: raising the LDS limit fails in big_launch_solve and the error is returned.
struct BigSolvePlan {
  bool staged;
  size_t lds;
};
inline BigSolvePlan big_solve_plan(const Dims& d, bool has_twin, int ncol) {
  const size_t lds = big_solve_lds_bytes(d);
  const size_t lds_st = lds + big_stage_lds_doubles(d, ncol) * sizeof(double);
  if (!has_twin || d.KP > kStageMaxKP || lds_st > kLdsCu) return BigSolvePlan{false, lds};
  return BigSolvePlan{true, lds_st};
}

// Column-major lag twin of the X slabs (X = [1, lags 1..p of the slab's data columns], the
// linear and hybrid designs of mcmcVAR.m:62-72 / mcmcVARhybridGibbs.m:69-84): column a of slab x
// is pool + x * slab + off[a] (rows t = 0..TP-1; off[0] -> a column of ones, off[a >= K] -> a zero
// column).  The slab is (T + p) x (N [+ Ns] + 2) doubles instead of KP x TP, so the Gram and the
// solve read a working set that stays in L2.  pool == nullptr: read X itself.
struct ColX {
  const double* pool;
  const int* off;
  long long slab;
  int ld;    // leading dimension of a twin column (off[a] = column * ld + row offset)
  int ncol;  // columns per twin (data, actual rates, ones, zeros)
};

// the three phases of the large CTA, in stream order.  CCMM_BIG_MASK (ablation build, timing only) drops phases
constexpr int kBigGram = 1, kBigChol = 2, kBigSolve = 4, kBigAll = kBigGram | kBigChol | kBigSolve;
// groups: ngroups x int4 systems (c*N + j) sharing one design X slab (-1 padded)
hipError_t big_launch_gram(hipStream_t st, const Dims& d, const int* Tslot, XSel xs, ChainState cs, const int4* groups,
                           int ngroups, ColX cx);
// Dinv: nmat x (KP/64) x 64 x 64 inverses of the Cholesky factor's diagonal blocks
hipError_t big_launch_chol(hipStream_t st, const Dims& d, const int* slotIV, const double* iVdiag, ChainState cs,
                           double* rdiag, double* Dinv);
// Ubuf: B x N x TP scratch (U = E A')
hipError_t big_launch_solve(hipStream_t st, const Dims& d, const int* Tslot, const double* iVb, XSel xs, ChainState cs,
                            const double* rdiag, RngArgs ra, double* Ubuf, const double* Dinv, ColX cx);

}  // namespace ccmm

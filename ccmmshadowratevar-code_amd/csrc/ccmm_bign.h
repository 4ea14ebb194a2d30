// Large-N Gibbs blocks (ccmm_bign.hip, its own translation unit): A-step, PHI and SV for
// 32 < N <= 128, used by ccmm_chains_sweep.hip in place of the per-chain small-matrix kernels.
// The sizes the launchers and the chain set take are host functions here, without HIP calls
// (tests/test_launch_plans.py checks them for every N of the path).
#pragma once
#include "ccmm_internal.h"

namespace ccmm {

constexpr int kBignMaxN = 128;  // the workgroup primitives hold one N x N matrix in LDS, rows <= 127
constexpr int kNL = 129;        // LDS row stride of an N x N matrix (odd: spreads banks)
constexpr int kCB = 16;         // panel / block width of wg_chol_inv (one MFMA block)

// doubles of SV scratch per chain: Q, L_0..L_T, M_0..M_T (N x N each), w_0..w_T; k_phi_big takes the first
// 3 N^2 of the same buffer (Lpost, L2, Sq)
inline size_t bign_sv_scratch(const Dims& d) {
  return (size_t)d.N * d.N * (1 + 2 * (size_t)(d.TP + 1)) + (size_t)(d.TP + 1) * d.N;
}

// padded Gram dimension of the A-step (64 for N <= 64, else 128): k_astep_gram writes whole 64 x 64 tiles
inline int bign_astep_npad(const Dims& d) { return d.N <= 64 ? 64 : 128; }

// LDS of k_astep_big: G [128 x kNL] | vec [128].  128 rows at every N: the 4 x 4 tiles of wg_chol read rows up
// to min(., 127) of the matrix before they mask them
inline size_t bign_astep_lds() { return (size_t)(kBignMaxN * kNL + 128) * sizeof(double); }
// LDS of k_astep_fin: As [N x N], column-major
inline size_t bign_astep_fin_lds(int N) { return (size_t)N * N * sizeof(double); }
// LDS of k_phi_big: M [128 x kNL]; wg_gram stages its chunks [32 x kNL] | weights [32] over the same region
// and writes the Gram after the last chunk
inline size_t bign_phi_lds() { return (size_t)(kBignMaxN * kNL) * sizeof(double); }
// LDS of k_sv_big: S [N x kNL] | Tb [kCB x 128] (wg_chol_inv) | vec [128] | vec2 [128]
inline size_t bign_sv_lds(int N) { return (size_t)(N * kNL + kCB * 128 + 256) * sizeof(double); }

// gbuf: B x (N - 1) x NPAD x NPAD (the weighted Grams of the N - 1 row regressions, k_astep_gram)
hipError_t bign_launch_astep(hipStream_t st, const Dims& d, const int* Tslot, ChainState cs, RngArgs ra,
                             double logy2offset, double* gbuf);
// scr: B x 3 x N x N
hipError_t bign_launch_phi(hipStream_t st, const Dims& d, const int* Tslot, int dPHI, const double* sPHI,
                           ChainState cs, double* scr);
// scr: B x bign_sv_scratch(d); cs.svobs / cs.svir from k_sv_mix
hipError_t bign_launch_sv(hipStream_t st, const Dims& d, const int* Tslot, const double* V0inv,
                          const double* V0invm, ChainState cs, RngArgs ra, double* scr);

}  // namespace ccmm

// Host-visible layouts, LDS sizes, launch decisions and host launchers of the per-sweep kernels of the
// generic (small-N) path: residuals, CTA weights, the A-step, the KSC indicators, PHI, the draw store and the
// drop-in helpers (ccmm_kernels.hip), the fused Gram + Cholesky (ccmm_gram_chol.hip) and the per-chain solve
// (ccmm_cta_solve.hip).  Each file is its own translation unit and launches every kernel it defines: the host units
// see launchers only, no kernel.  The size and decision functions make no HIP call (tests/launch_plans_main.cpp
// prints them on the host).
#pragma once
#include <algorithm>

#include "ccmm_internal.h"

namespace ccmm {

// ---------------------------------------------------------------- ccmm_gram_chol.hip
constexpr int kGcWaves = 8;
constexpr int kGcTC = 16;     // t rows per SYRK chunk
constexpr int kGcLdp = 17;    // LDS row stride of a 16 x 16 panel tile
// LDS row stride (doubles) of a Z chunk: 16 NT + 16, rows 32 banks apart (272 at NT = 16)
__host__ __device__ constexpr int gc_ldz(int NT) { return 16 * NT + 16; }
constexpr int kGcLdz = gc_ldz(16);

// column-major enumeration of the lower tiles of an NT x NT tile grid
__host__ __device__ constexpr int gc_tj(int NT, int g) {
  int tj = 0;
  while (tj < NT && g >= NT - tj) {
    g -= NT - tj;
    ++tj;
  }
  return tj;
}
__host__ __device__ constexpr int gc_ti(int NT, int g) {
  int tj = 0;
  while (tj < NT && g >= NT - tj) {
    g -= NT - tj;
    ++tj;
  }
  return tj + g;
}
__host__ __device__ constexpr int gc_tpw(int NT) { return (NT * (NT + 1) / 2 + kGcWaves - 1) / kGcWaves; }

struct GcArgs {
  const double* X;   // system's design, KP x TP column-major (ld TP)
  const double* w;   // sqrt weights, TP
  const double* iv;  // prior precision diagonal, KP
  double* L;         // KP x KP output
  double* rd;        // KP output
  int T, TP, KP;
  int mode;  // kGc* bits below; 0 in production
};
// bits of GcArgs::mode: none selects what is computed; all are timing-only (CCMM_GC_MODE, ablation build; results
// invalid): no SYRK, no Cholesky, no trailing update, no panel solve, no diagonal factor
constexpr int kGcNoSyrk = 1, kGcNoChol = 2, kGcNoTrailing = 4, kGcNoPanel = 8, kGcNoDiag = 16;

// LDS of k_gram_chol<NT>: max(SYRK stage Z0 | Z1 [kGcTC x gc_ldz(NT)], factor stage Dg | Pn[NT] [16 x kGcLdp])
inline size_t gram_chol_lds_bytes(int NT) {
  return (size_t)std::max(2 * kGcTC * gc_ldz(NT), (NT + 1) * 16 * kGcLdp) * sizeof(double);
}
bool gram_chol_supported(int NT);  // tile counts KP / 16 with a compiled kernel
hipError_t launch_gram_chol(int NT, hipStream_t st, Dims d, const int* Tslot, XSel xs, ChainState cs,
                            const double* iVdiag, double* rdiag, int mode);

// ---------------------------------------------------------------- ccmm_cta_solve.hip
constexpr int kSolveLd = 65;  // LDS row stride of the staged 64x64 diagonal block
// LDS of k_cta_solve2: v [TP] | yv [KP] | rdl [KP] | Ls [64 x kSolveLd] | Al [N x N] | Ael [N x N]
inline size_t cta_solve2_lds_bytes(int N, int KP, int TP) {
  return (size_t)(TP + 2 * KP + 64 * kSolveLd + 2 * N * N) * sizeof(double);
}
// k_cta_solve2<n_bucket(N)>, one workgroup per chain
hipError_t launch_cta_solve2(hipStream_t st, Dims d, const int* Tslot, const double* iVb, XSel xs, ChainState cs,
                             const double* rdiag, RngArgs ra);

// ---------------------------------------------------------------- ccmm_kernels.hip
// draw storage
struct Store {
  double* PAI;     // [B][cap][N][K]
  double* PHI;     // [B][cap][N(N+1)/2]
  double* invA;    // [B][cap][N][N]
  double* sqrtht;  // [B][cap][N][T]
  int cap, m, Tmax;
};

// one pass per design slab (k_resid_multi<n_bucket(N)>, LDS: PAI rows [K x NB]) once the chains fill the chip;
// at small B the per-equation k_resid's B N TP / 256 workgroups keep the slab loads in flight (0.12 -> ~0.01 ms
// at B = 1): the same fma order per equation, so E is bit-identical either way
constexpr int kResidMultiMinB = 16;
inline size_t resid_multi_lds_bytes(int N, int K) { return (size_t)K * n_bucket(N) * sizeof(double); }
inline bool resid_multi(int N, int K, int B) {
  return N <= 32 && resid_multi_lds_bytes(N, K) <= kLdsDefault && B > kResidMultiMinB;
}
hipError_t launch_resid(hipStream_t st, Dims d, const int* Tslot, XSel xs, ChainState cs);
hipError_t launch_cta_weights(hipStream_t st, Dims d, const int* Tslot, ChainState cs, int sqrt_form);

// LDS of k_astep / k_astep_w: regression blocks ii = 1..N-1 [ii (ii + 1) / 2 + ii] | Anew [N x N] | 8 doubles of
// slack | E [N x TP] at es_off when the chain's residuals fit beside them (N = 20, T = 750: 138 KB in all), else
// es_off = -1 and the kernel reads E from global memory
struct AstepPlan {
  size_t lds;
  int es_off;
};
inline AstepPlan astep_plan(int N, int TP) {
  const int total = (N - 1) * N * (N + 1) / 6 + N * (N - 1) / 2 + 8;
  const size_t lds = (size_t)(total + N * N) * sizeof(double);
  const size_t staged = lds + (size_t)N * TP * sizeof(double);
  return staged <= kLdsCu ? AstepPlan{staged, total + N * N} : AstepPlan{lds, -1};
}
// k_astep_w<20 / 32> (wave-parallel factorisations) or, serial, the one-thread-per-regression k_astep; same
// draws up to summation order inside the factorisation (identical update order, fma placement as written)
hipError_t launch_astep(bool serial, hipStream_t st, Dims d, const int* Tslot, ChainState cs, RngArgs ra,
                        double logy2offset, const int* gtab);

// LDS of k_phi: Lpost | Rz | Sq | Ph [N x (N + 1) each] | eta [N x (TP + 1)] (kPhiStageEta), the region wide
// enough for Z [N x (TP + dPHI)] after it (kPhiStageZ), when they fit
struct PhiPlan {
  size_t lds;
  int stage_eta;
};
// bits of stage_eta: what k_phi reads from LDS (the same products in the same order); none is timing-only
constexpr int kPhiStageEta = 1;  // eta staged with row stride TP + 1
constexpr int kPhiStageZ = 2;    // Z follows eta into the same region
// stage_mask (option phi_stage, default 3): the bits the plan may use, for comparing the three forms on one shape.
// Z is staged into the region eta has been read from, so kPhiStageZ without kPhiStageEta is no form of the kernel:
// masks 2 and 0 both mean "stage nothing".  The LDS size is that of the masked plan.
inline PhiPlan phi_plan(int N, int TP, int dPHI, int stage_mask = kPhiStageEta | kPhiStageZ) {
  const size_t lds = (size_t)(4 * N * (N + 1)) * sizeof(double);
  const size_t staged = lds + (size_t)N * (TP + 1) * sizeof(double);
  const size_t staged_z = lds + (size_t)N * std::max(TP + 1, TP + dPHI) * sizeof(double);
  if (!(stage_mask & kPhiStageEta)) stage_mask = 0;
  if (staged_z <= kLdsCu && (stage_mask & kPhiStageZ)) return PhiPlan{staged_z, kPhiStageEta | kPhiStageZ};
  if (staged <= kLdsCu && (stage_mask & kPhiStageEta)) return PhiPlan{staged, kPhiStageEta};
  return PhiPlan{lds, 0};
}
hipError_t launch_phi(hipStream_t st, Dims d, const int* Tslot, int dPHI, const double* sPHIall, ChainState cs,
                      int phi_stage);

// the untemplated kernels: one thread per element (k_store: a fixed 64 x B grid; the self-tests: one wave per probe)
hipError_t launch_sv_mix(hipStream_t st, Dims d, const int* Tslot, ChainState cs, RngArgs ra);
hipError_t launch_phi_gen(hipStream_t st, Dims d, const int* Tslot, int dPHI, ChainState cs, RngArgs ra);
hipError_t launch_store(hipStream_t st, Dims d, ChainState cs, Store s);
// sums and sums of squares of the stored PAI draws m0 <= m < m1, `per` entries of each of B chains
hipError_t launch_pai_moments(hipStream_t st, const double* sPAI, int cap, int m0, int m1, int per, int B, double* sum,
                              double* sumsq);
hipError_t launch_truncnorm(hipStream_t st, int n, const double* mu, const double* sig, double elb, const double* u,
                            double* out, uint8_t* flags);
hipError_t launch_rng_normals(hipStream_t st, RngArgs ra, int c, int block, int n, double* out);
hipError_t launch_mfma_selftest(hipStream_t st, const double* A, const double* B, double* D);
hipError_t launch_mfma_selftest_acc(hipStream_t st, const double* A, const double* B, const double* C, double* D,
                                    int nprobe);

}  // namespace ccmm

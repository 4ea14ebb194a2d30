// Device views, record layouts, LDS sizes, launch decisions and host launchers of the ELB shadow-rate step and
// its acceptance-sampling branch.  The kernels are defined in their own translation units, ccmm_elb.hip and
// ccmm_ps.hip, each with the launchers of every kernel it defines (those of the templated kernels pick, and so
// instantiate, the template arguments); this header is what the host side (ccmm_chains_elb.hip,
// ccmm_chains_sweep.hip) and the predictive-density kernels see: launchers, no kernel.  The size and decision
// functions make no HIP call (tests/launch_plans_main.cpp prints them on the host).
#pragma once
#include <algorithm>

#include "ccmm_internal.h"

namespace ccmm {

constexpr int kElbNsMax = 5;  // Ns = 5: the Krippner / Wu-Xia datasets at ELB > 0.25 (setShadowYields.m:1-5)
constexpr int kElbColMax = 128;  // 2 p Ns neighbour columns, two per lane

struct ElbDev {
  int Ns, p, elbTmax, passes;    // passes = gibbsburn + 1
  double elb;
  const int* ndxS;               // [Ns]
  const uint8_t* actual;         // [N] actualrateBlock
  const int* elbT0;              // [ndata]
  const int* elbT;               // [ndata]
  const uint8_t* sNaN;           // [ndata][elbTmax][Ns]  (t-major)
  const int* ncens;              // [ndata]
  const int* cens;               // [ndata][elbTmax] censored months in increasing order
  const double* Xactual;         // X pool (slot slabs first)
  // per chain scratch
  double* Phi;    // [B][N][N*p]   Phi[i][(l-1)N + q] = PAIshadow(1+(l-1)N+q, i)
  double* Y0;     // [B][elbTmax][N]  scratch: Yb - Yhatactual
  double* Yt;     // [B][elbTmax][N]  Yb: the chain's Y, censored shadow-rate cells at 0
  double* Et;     // [B][elbTmax][N]  ε_τ (stable residual form, see k_elb_prep)
  double* cond;   // [B][elbTmax][condStride]
  double* Scur;   // [B][elbTmax][Ns] shadow rates (in/out)
  int condStride;
  int kshadow, K;  // hybrid model: PAI rows kshadow..K-1 load the actual-rate lags (K > kshadow)
  int mode;        // kElb* bits below; 0 in production
  const double* yhat;  // [B][elbTmax][N] explicit YHAT0 (ccmm_gibbs_shadowrates) or nullptr
  uint8_t* flags;      // [B][passes][elbTmax][Ns] truncated-normal branch flags or nullptr
  // acceptance-sampling branch (mcmcVARshadowrateBlockHybrid.m:438-466, ccmm_ps.hip)
  int ps;              // 1: k_elb_prep / k_elb_cond also build the PS precision records
  double* EtPS;        // [B][elbTmax][N] residuals of the PS model (Yhatactual as intercept)
  const int* psFlag;   // [B] PS outcome of this sweep: > 0 accepted (k_elb_gibbs skips the chain)
  // gibbsdrawShadowratesB3 (ccmm_gibbs_shadowrates_b3): the VAR on Y itself with the intercept in the
  // state (base residuals in the PS model's form, yhat = 0) and, when Amon is set, a structural matrix
  // per window month, A_tau = B(2:Ny+1, :, tau)^-1 ([B][elbTmax][N][N], lower)
  int b3;
  const double* Amon;
  // 1: the structural matrices A (cs.A / Amon) are full -- the inverse of a general impact matrix
  // Psi(2:Ny+1, :) (ccmm_gibbs_shadowrates); 0: unit lower triangular (every sweep; invA's inverse)
  int Afull;
  // speculative Gibbs step (k_elb_gibbs_wf ASYNC / k_elb_gibbs_mp, small B): the passes start beside the PS
  // branch (ccmm_ps.hip) on another stream; k_ps_apply posts psState[c] = psEpoch << 1 | accepted, the
  // waves stop early once they see an accepted proposal (a poll, never a wait: the streams need not run
  // concurrently), the draw goes to ScurSpec, and k_elb_spec_select keeps it only where the PS branch
  // rejected -- the reference's order (PS first, the Gibbs draw as the fallback, :438-466), same draws
  int spec;
  const unsigned long long* psState;
  unsigned long long psEpoch;
  double* ScurSpec;  // [B][elbTmax][Ns]
};

// bits of ElbDev::mode: none selects what is computed; all are timing-only (CCMM_ELB_MODE, ablation build; a default
// build compiles them out; results invalid): no draws (fmin), fixed uniforms, cycle attribution of the ASYNC month
// body (CCMM_ELB_PROF), no record loads, no predecessor wait, no month sums, ub histogram of the draws
constexpr int kElbNoDraw = 1, kElbFixedU = 2, kElbProf = 64, kElbNoRecords = 128, kElbNoWait = 256, kElbNoSums = 512,
              kElbUbHist = 4096;

// condition record per censored month (doubles):
//   a_t [Ns] | beta1 [Ns][Ns-1] | sqrtOmega1 [Ns] | 1 / sqrtOmega1 [Ns] | Ω [Ns][Ns] | G [2p Ns][Ns]
// (1 / sqrtOmega1: the Gibbs kernels form ub = (elb - mu) / sig as a product, off the division's latency)
// G column col = kk*Ns + s': kk < p past lag kk+1, kk >= p future lead kk-p+1.
// With the PS branch (e.ps) the record continues (elb_cond_ps_off):
//   P [Ns][Ns] (the month's precision, Ω^-1) | b_PS [Ns] | gP [p Ns][Ns]
// b_PS = the PS model's linear term with every censored cell at 0; gP = the raw unit
// responses of the past neighbours (-gP = the off-diagonal precision blocks).
__host__ __device__ inline int elb_cond_head(int Ns) { return Ns + Ns * (Ns - 1) + 2 * Ns + Ns * Ns; }
__host__ __device__ inline int elb_cond_ps_off(int Ns, int p) {
  return elb_cond_head(Ns) + 2 * p * Ns * Ns;
}
__host__ __device__ inline int elb_cond_stride(int Ns, int p, int ps = 0) {
  return elb_cond_ps_off(Ns, p) + (ps ? Ns * Ns + Ns + p * Ns * Ns : 0);
}

constexpr int kElbPrepThreads = 512;
constexpr int kElbOctMinB = 384;  // k_elb_gibbs_oct from this many chains (option elb_oct = 1)
// k_elb_gibbs_mp (multi-CU wavefront, small B): granule exchange between the parts of a chain
constexpr int kElbMpMaxB = 64;  // auto: the multi-CU wavefront for B <= 64 chains
struct ElbXch {
  double* gran;                // [B][PARTS][elbTmax][NS] granules of 2 doubles {value, tag bits}
  unsigned long long epoch;    // launch counter (host): tags of older launches never match
};

constexpr int kPsWMax = 80;  // band width limit: Ns (p + 1) <= 80 (Ns = 5 with p = 12: 65)

struct PsDev {
  int nmax, W, NP;  // max censored cells over slots, band width, proposals per sweep
  double elb;
  double* L;        // [B][nmax][W]  L(i + j, i) at [i][j], zero beyond n
  double* ybar;     // [B][nmax]     L^-1 b
  int* cell;        // [B][nmax]     shadow-rate offset t Ns + a of censored cell i
  int* n;           // [B]           censored cells (0: PS skipped this sweep)
  int* acc;         // [B]           smallest accepted proposal (0-based), INT_MAX none
  int* flag;        // [B]           ndxAccept of this sweep (1-based), 0 none
  int* count;       // [B][2]        accepted sweeps: [0] burn-in, [1] kept (countELBaccept*)
  double* first;    // [B][Ns elbTmax] proposal 1 over the window (shadowrateProposals(:,:,1), kept as
                    //               missingrate, mcmcVARshadowrate.m:435); nullptr: not kept
  int per;          // Ns elbTmax
  unsigned long long* state;  // [B] speculative Gibbs step: epoch << 1 | accepted, posted by k_ps_apply
  unsigned long long epoch;   //     (nullptr / 0: no Gibbs step waits on the decision)
  // one unconstrained draw per sweep (ccmm_chains_set_elb_treatment): 0 the accept-first branch, 1 the
  // missing-data treatment (the draw becomes the data), 2 the alternate draw (block CCMM_RNG_PSALT)
  int draw1;
  double* out;      // [B][Ns elbTmax] where the draw goes: the chain's shadow rates / the missingrate buffer
};

constexpr int kPsChunk = 64;  // assembled band rows per LDS chunk

// band-width bucket (template argument W) of the largest cell window wmax <= kPsWMax
inline int ps_band_bucket(int wmax) { return wmax <= 16 ? 16 : wmax <= 32 ? 32 : wmax <= 48 ? 48 : wmax <= 64 ? 64 : 80; }
inline bool ps_supported_w(int W) { return W == 16 || W == 32 || W == 48 || W == 64 || W == 80; }

// LDS of k_ps_chol: win [W x W] | lv [W] | bb [W] | info [nmax ints]
inline size_t ps_chol_lds_bytes(int W, int nmax) {
  return (size_t)(W * W + 2 * W) * sizeof(double) + (size_t)nmax * sizeof(int);
}
// LDS of k_ps_chol_w: prow [kPsChunk x W] | pb [kPsChunk] | sL [W] | scens [elbTmax ints] | info [nmax ints]
__host__ __device__ inline size_t ps_chol_w_lds_bytes(int W, int elbTmax, int nmax) {
  return (size_t)(kPsChunk * W + kPsChunk + W) * sizeof(double) + (size_t)(elbTmax + nmax) * sizeof(int);
}
// LDS of k_ps_apply: zl [nmax], the proposal's normals
inline size_t ps_apply_lds_bytes(int nmax) { return (size_t)nmax * sizeof(double); }

// LDS of k_ps_draw1 (byte offsets): k_ps_chol_w's doubles prow | pb | sL, then ybl [nmax] (L^-1 b) | zl [nmax] (the
// draw's normals) | Ll [nmax x W] (the factor's band rows, when resident) | scens [elbTmax ints] | info [nmax ints]
// | cellL [nmax ints] (the cells' shadow-rate offsets)
struct PsDraw1Lds {
  size_t prow, pb, sL, ybl, zl, Ll, scens, info, cellL, end;
};
inline PsDraw1Lds ps_draw1_lds(int W, int elbTmax, int nmax, int resident) {
  const size_t D = sizeof(double), I = sizeof(int);
  PsDraw1Lds l{};
  l.pb = l.prow + (size_t)kPsChunk * W * D;
  l.sL = l.pb + kPsChunk * D;
  l.ybl = l.sL + W * D;
  l.zl = l.ybl + nmax * D;
  l.Ll = l.zl + nmax * D;
  l.scens = l.Ll + (resident ? (size_t)nmax * W * D : 0);
  l.info = l.scens + elbTmax * I;
  l.cellL = l.info + nmax * I;
  l.end = l.cellL + nmax * I;
  return l;
}
inline size_t ps_draw1_lds_bytes(int W, int elbTmax, int nmax, int resident) {
  return ps_draw1_lds(W, elbTmax, nmax, resident).end;
}
// whether k_ps_draw1 keeps the factor's band rows in LDS (else it reads them back from PsDev::L)
inline int ps_draw1_resident(int W, int elbTmax, int nmax) {
  return ps_draw1_lds_bytes(W, elbTmax, nmax, 1) <= kLdsCu ? 1 : 0;
}

// ---------------------------------------------------------------- launch decisions of the ELB step
// k_elb_prep.  LDS: X0 [2 + Np] | sPhi [N x (Np + 1)] (phi_lds bit 0: Phi staged when it fits; N = 20, p = 12:
// 40 KB; N = 120 reads it from e.Phi) | Z = Yb - yhat [elbTmax x N] | Yb [elbTmax x N] (bit 1: when they fit
// beside it; 52 KB at elbT = 165).  rows > 0 (small batches, bit 1 set): the window's residual rows over wg
// workgroups per chain, `rows` rows each
struct ElbPrepPlan {
  size_t lds;
  int phi_lds, rows, wg;
};
inline ElbPrepPlan elb_prep_plan(int N, int p, int elbTmax, int B) {
  const int Np = N * p;
  ElbPrepPlan pl{(size_t)(2 + Np + N * (Np + 1)) * sizeof(double), 1, 0, 1};
  if (pl.lds > kLdsCu) pl = ElbPrepPlan{(size_t)(2 + Np) * sizeof(double), 0, 0, 1};
  const size_t lds_zy = pl.lds + (size_t)2 * elbTmax * N * sizeof(double);
  if (pl.phi_lds && lds_zy <= kLdsCu) {
    pl.phi_lds |= 2;
    pl.lds = lds_zy;
  }
  if ((pl.phi_lds & 2) && B < 128) {
    const int per = std::max(1, 256 / B);
    pl.rows = std::max(16, (elbTmax + per - 1) / per);
    pl.wg = (elbTmax + pl.rows - 1) / pl.rows;
  }
  return pl;
}

// k_elb_cond.  LDS: Q [(p + 1) x Ns x N] | gS [(1 + 2 p Ns) x Ns] | Pm [Ns x Ns] | Om [Ns x Ns] | Wl [kb x N x Ns]
// | PS [N x p x Ns] | Al [N x N] (a_lds).  W_k of kb lags at once: all p + 1 when they fit the budget, a tuning
// choice that leaves a second workgroup room on the CU; A staged beside them when the whole stays within the
// default dynamic limit.  Two waves per censored month (BH N = 20: 1.30 -> 1.13 ms at B = 256); four when the
// month's staging fills a CU's LDS (N > 64)
constexpr size_t kElbCondLdsBudget = 96 * 1024;
struct ElbCondPlan {
  size_t lds;
  int threads, a_lds, kb;
};
inline ElbCondPlan elb_cond_plan(int N, int p, int Ns) {
  const size_t lds0 = (size_t)((p + 1) * Ns * N + (1 + 2 * p * Ns) * Ns + 2 * Ns * Ns + N * p * Ns) * sizeof(double);
  const size_t per_lag = (size_t)N * Ns * sizeof(double), lds_a = (size_t)N * N * sizeof(double);
  int kb = p + 1;
  while (kb > 1 && lds0 + kb * per_lag > kElbCondLdsBudget) --kb;
  const size_t lds = lds0 + kb * per_lag;
  const int a_lds = lds + lds_a <= kLdsDefault ? 1 : 0;
  return ElbCondPlan{lds + (a_lds ? lds_a : 0), N > 64 ? 256 : 128, a_lds, kb};
}

// LDS of k_elb_gibbs: Sl | Ul | Zl [elbTmax x Ns each] | Tm [elbTmax ints]
inline size_t elb_gibbs_lds_bytes(int elbTmax, int Ns) {
  return (size_t)3 * elbTmax * Ns * sizeof(double) + (size_t)elbTmax * sizeof(int);
}
// LDS of the wavefront kernels (byte offsets; host sizes and the kernels' pointers both come from these layouts):
// Sl [elbTmax x Ns] | Ul [W][elbTmax x Ns] | Zl [W][elbTmax x Ns] | Tm [elbTmax ints] | reach [elbTmax ints]
// | prog [nprog ints] | one int no kernel reads
struct ElbWaveLds {
  size_t Sl, Ul, Zl, Tm, reach, prog, spare, end;
};
__host__ __device__ inline ElbWaveLds elb_wave_lds(int elbTmax, int Ns, int W, int nprog) {
  const size_t pg = (size_t)elbTmax * Ns * sizeof(double), I = sizeof(int);
  ElbWaveLds l{};
  l.Ul = l.Sl + pg;
  l.Zl = l.Ul + W * pg;
  l.Tm = l.Zl + W * pg;
  l.reach = l.Tm + elbTmax * I;
  l.prog = l.reach + elbTmax * I;
  l.spare = l.prog + nprog * I;
  l.end = l.spare + I;
  return l;
}
// k_elb_gibbs_wf<NS, W, ASYNC>: W passes in flight, prog [2][W]
__host__ __device__ inline ElbWaveLds elb_wf_lds(int elbTmax, int Ns, int W) {
  return elb_wave_lds(elbTmax, Ns, W, 2 * W);
}
inline size_t elb_wf_lds_bytes(int elbTmax, int Ns, int W) { return elb_wf_lds(elbTmax, Ns, W).end; }
// k_elb_gibbs_mp<NS, WPC, PARTS>: WPC drawing waves per part, prog [WPC + 1] (the drawing waves, the importer)
__host__ __device__ inline ElbWaveLds elb_mp_lds(int elbTmax, int Ns, int WPC) {
  return elb_wave_lds(elbTmax, Ns, WPC, WPC + 1);
}
inline size_t elb_mp_lds_bytes(int elbTmax, int Ns, int WPC) { return elb_mp_lds(elbTmax, Ns, WPC).end; }
// k_elb_gibbs_oct (byte offsets): Sl [elbTmax x Ns] | Tm [elbTmax ints] | reach [elbTmax ints]
struct ElbOctLds {
  size_t Sl, Tm, reach, end;
};
__host__ __device__ inline ElbOctLds elb_oct_lds(int elbTmax, int Ns) {
  ElbOctLds l{};
  l.Tm = l.Sl + (size_t)elbTmax * Ns * sizeof(double);
  l.reach = l.Tm + elbTmax * sizeof(int);
  l.end = l.reach + elbTmax * sizeof(int);
  return l;
}
inline size_t elb_oct_lds_bytes(int elbTmax, int Ns) { return elb_oct_lds(elbTmax, Ns).end; }

// passes in flight of the wave kernels for option elb_waves = want: 1 (the sequential k_elb_gibbs), 4 or 8, and
// fewer when a long ELB window's passes do not fit the CU's LDS (8 -> 4 -> 1)
inline int elb_gibbs_waves(int elbTmax, int Ns, int want) {
  int W = want <= 1 ? 1 : (want < 8 ? 4 : 8);
  while (W > 1 && elb_wf_lds_bytes(elbTmax, Ns, W) > kLdsCu) W = (W == 8) ? 4 : 1;
  return W;
}

// the Gibbs kernel of a sweep (bit-identical draws whichever runs): the one-wave sequential kernel, W passes in
// flight on W waves (lock-step or with per-wave progress flags), the W = 8 wavefront over `parts` CUs per
// chain, or eight passes in flight inside one wave
enum ElbGibbsKernel { kElbGibbsSeq, kElbGibbsWf, kElbGibbsMp, kElbGibbsOct };
struct ElbGibbsPlan {
  ElbGibbsKernel kernel;
  int W;       // wf: 4 or 8
  bool async;  // wf
  int parts;   // mp: 2 or 4
};

// ---------------------------------------------------------------- launchers (ccmm_elb.hip)
inline bool elb_supported_ns(int Ns) { return Ns >= 1 && Ns <= kElbNsMax; }
hipError_t launch_elb_prep(hipStream_t st, const ElbPrepPlan& pl, Dims d, ElbDev e, XSel xs, ChainState cs);
hipError_t launch_elb_cond(hipStream_t st, const ElbCondPlan& pl, Dims d, ElbDev e, ChainState cs);
// xc: the granule exchange of kElbGibbsMp (unused otherwise)
hipError_t launch_elb_gibbs(hipStream_t st, const ElbGibbsPlan& pl, Dims d, ElbDev e, ChainState cs, RngArgs ra,
                            ElbXch xc);
// the speculative draw kept where the PS branch rejected; one workgroup per chain
hipError_t launch_elb_spec_select(hipStream_t st, ElbDev e, const int* slot, int B);
// the chains' X / Y slabs (and lag slabs dpool, lag twins dcpool when given) rebuilt from the new shadow rates
hipError_t launch_elb_rebuild(hipStream_t st, Dims d, ElbDev e, XSel xs, ChainState cs, int xslab0, double* dpool, int ldd,
                              int drows, double* dcpool, int dcld, long long dcslab);
hipError_t launch_elb_store(hipStream_t st, int B, ElbDev e, ChainState cs, double* out, int cap, int m);
// ---------------------------------------------------------------- launchers (ccmm_ps.hip)
// the fused draw k_ps_draw1<ps.W> (W <= 64)
hipError_t launch_ps_draw1(hipStream_t st, Dims d, ElbDev e, PsDev ps, ChainState cs, RngArgs ra);
// k_ps_chol_w<ps.W> (W <= 64; register window, one wave per chain) or, lds_window, k_ps_chol (same factor)
hipError_t launch_ps_chol(bool lds_window, hipStream_t st, Dims d, ElbDev e, PsDev ps, ChainState cs);
// prop: k_ps_prop<ps.W> over the ps.NP proposals; then k_ps_apply<ps.W, FORCED = ps.draw1 != 0>
hipError_t launch_ps_apply(bool prop, hipStream_t st, int B, ElbDev e, PsDev ps, RngArgs ra, int kept);
// proposal 1 (first, or NaN when null) and ndxAccept (flag, or 0 when null) of sweep m into the draw store
hipError_t launch_ps_first_store(hipStream_t st, int B, const double* first, const int* elbT, const int* slot,
                                 double* out, int per, int Ns, int cap, int m);
hipError_t launch_ps_store(hipStream_t st, const int* flag, int* out, int B, int cap, int m);

}  // namespace ccmm

// Compute_diagnostics (goVARshadowrateBlockHybrid.m:55-56, :313-316): the per-series core of Diagnostics.m
// (momentg :134-300, ineff :129-132, the one-chain psrf :28-127), shared by the kernel k_diag_series
// (ccmm_diagk.hip) and the host twin ccmm_diagnostics_host (ccmm_diag.cpp), and the launch arithmetic of the
// kernel.  Both units are built with -ffp-contract=off and run the same operations in the same order, so the
// device and the host return the same bits.  No HIP runtime call in this header.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CCMM_DIAG_HD __host__ __device__
#else
#define CCMM_DIAG_HD
#endif
#if defined(__clang__)
#define CCMM_DIAG_UNROLL _Pragma("unroll")
#else
#define CCMM_DIAG_UNROLL _Pragma("GCC unroll 16")
#endif

namespace ccmm {

constexpr int kDiagNStat = 11;  // pmean, pstd, nse, rne, nse1, rne1, nse2, rne2, nse3, rne3, psrf
constexpr int kDiagNG = 100;    // groups of momentg (:183)
constexpr int kDiagLags = 15;   // the widest taper reads rnn(0..14) (:271-280)
constexpr int kDiagWave = 64;   // one lane per series, one wave per workgroup
constexpr int kDiagAhead = 16;  // draws of one batch of loads; the next batch is in flight while one is used
constexpr size_t kDiagLdsCu = 160 * 1024;

// ---------------------------------------------------------------- launch arithmetic
// Workgroup bx of the grid's x, thread t: entry bx * 64 + t of chain blockIdx.y.  The 100 centred group means
// of a wave's 64 series are [100][64] doubles of LDS (element ig of lane l at ig * 64 + l: conflict-free by
// lane), 51 200 B, three workgroups per CU.
struct DiagPlan {
  int threads, waves;  // per workgroup
  int grid_x, grid_y;
  size_t lds;          // bytes per workgroup
  int per_cu;          // workgroups of one CU by LDS
};

inline DiagPlan diag_plan(int S, int C) {
  DiagPlan pl{};
  pl.waves = 1;
  pl.threads = kDiagWave * pl.waves;
  pl.grid_x = S > 0 ? (S + pl.threads - 1) / pl.threads : 0;
  pl.grid_y = C > 0 ? C : 0;
  pl.lds = (size_t)kDiagNG * pl.threads * sizeof(double);
  pl.per_cu = (int)(kDiagLdsCu / pl.lds);
  return pl;
}

CCMM_DIAG_HD inline long long diag_entry(long long bx, int thread) { return bx * kDiagWave + thread; }

// ccmm_diagnostics: series per upload block for M draws in a scratch of kDiagScratch doubles per buffer (a
// multiple of the 64 series of a wave, at least one wave)
constexpr long long kDiagScratch = 1ll << 23;  // 64 MB
inline int diag_block_series(int M) {
  const long long sb = kDiagScratch / (M > 0 ? M : 1) / kDiagWave * kDiagWave;
  return (int)(sb < kDiagWave ? kDiagWave : sb);
}

// ---------------------------------------------------------------- the core
// One series g[m * ld], m = 0..M-1 (M >= 100), to st[0..10].  cn(ig) is the series' own store of 100 doubles
// (LDS on the device, a local array on the host).
//
// momentg, statement by statement (Diagnostics.m:178-297) with ad = 1 (:209): td = tdd = nuse, tdn = tn,
// tnn = tvar.  The denominator's group means cd(ig) = gd / ns = 1 and bard = td / nuse = 1 (:226, :250), so
// cd(ig) - bard, and with it rdd, rnd, sdd and snd (:252-261, :274-281), are exactly zero and are dropped.
// psrf is the one-chain form (:75-85, :95-122): the first and the last floor(M / 3) draws as two sequences; the
// sequences' sums are taken during the pass over the draws, the centred sums in a second read of the two thirds.
template <class CN>
CCMM_DIAG_HD inline void diag_series(const double* g, long long ld, int M, CN cn, double* st) {
  const int ns = M / kDiagNG, nuse = ns * kDiagNG, n3 = M / 3;
  double tn = 0.0, tvar = 0.0, gn = 0.0, gnn = 0.0, s1 = 0.0, s2 = 0.0;
  int k = 0, ig = 0;
  // :204-231 for one draw, and the sums of psrf's two sequences (:104 mean)
  auto step = [&](int m, double x) {
    if (m < nuse) {  // draws beyond nuse are ignored by momentg (:190-191)
      gn = gn + x;
      gnn = gnn + x * x;
      if (++k == ns) {
        tn = tn + gn;
        tvar = tvar + gnn;
        cn(ig) = gn / ns;
        ++ig;
        gn = 0.0;
        gnn = 0.0;
        k = 0;
      }
    }
    if (m < n3) s1 = s1 + x;
    if (m >= M - n3) s2 = s2 + x;
  };
  // The loads do not depend on the sums: whole batches of kDiagAhead draws are requested without a condition,
  // and the next batch before the current one is used, so two batches are in flight; the rest draw by draw.
  const int nb = M / kDiagAhead;  // >= 6
  double v[kDiagAhead], nx[kDiagAhead];
CCMM_DIAG_UNROLL
  for (int u = 0; u < kDiagAhead; ++u) {
    v[u] = g[(long long)u * ld];
    nx[u] = 0.0;
  }
  for (int b = 0; b < nb; ++b) {
    const int m0 = b * kDiagAhead;
    if (b + 1 < nb) {
CCMM_DIAG_UNROLL
      for (int u = 0; u < kDiagAhead; ++u) nx[u] = g[(long long)(m0 + kDiagAhead + u) * ld];
    }
CCMM_DIAG_UNROLL
    for (int u = 0; u < kDiagAhead; ++u) step(m0 + u, v[u]);
CCMM_DIAG_UNROLL
    for (int u = 0; u < kDiagAhead; ++u) v[u] = nx[u];
  }
  for (int m = nb * kDiagAhead; m < M; ++m) step(m, g[(long long)m * ld]);
  const double td = (double)nuse;
  const double eg = tn / td;                 // :233
  const double varg = tvar / td - eg * eg;   // :234
  st[0] = eg;
  st[1] = varg > 0.0 ? sqrt(varg) : -1.0;    // :235-239
  double varnum = (tvar - 2.0 * eg * tn + td * (eg * eg)) / (td * td);  // :242
  st[2] = varnum > 0.0 ? sqrt(varnum) : -1.0;
  st[3] = varg / (nuse * varnum);            // :246
  // autocovariances of the centred group means, lags 0..14, each sum in ig order (:249-264); w holds
  // cn(ig), cn(ig - 1), ..
  const double barn = tn / nuse;
  double w[kDiagLags], ann[kDiagLags];
CCMM_DIAG_UNROLL
  for (int l = 0; l < kDiagLags; ++l) w[l] = ann[l] = 0.0;
  for (int i = 0; i < kDiagNG; ++i) {
    const double c = cn(i) - barn;
CCMM_DIAG_UNROLL
    for (int l = kDiagLags - 1; l > 0; --l) w[l] = w[l - 1];
    w[0] = c;
CCMM_DIAG_UNROLL
    for (int l = 0; l < kDiagLags; ++l)
      if (l <= i) ann[l] = ann[l] + c * w[l];
  }
CCMM_DIAG_UNROLL
  for (int l = 0; l < kDiagLags; ++l) ann[l] = ann[l] / kDiagNG;  // rnn(lag + 1)
  // tapered estimates (:271-295)
  const int taper[3] = {4, 8, 15};
CCMM_DIAG_UNROLL
  for (int mm = 0; mm < 3; ++mm) {
    const double am = (double)taper[mm];
    double snn = ann[0];
CCMM_DIAG_UNROLL
    for (int l = 1; l < kDiagLags; ++l)
      if (l < taper[mm]) {
        const double att = 1.0 - l / am;
        snn = snn + 2.0 * att * ann[l];
      }
    varnum = (double)ns * nuse * snn / (td * td);  // :281 with snd = sdd = 0
    st[4 + 2 * mm] = varnum > 0.0 ? sqrt(varnum) : -1.0;
    st[5 + 2 * mm] = varg / (nuse * varnum);
  }
  // psrf (:101-122) of the sequences g[0..n3-1] and g[M-n3..M-1], N = n3, M = 2
  const double mu1 = s1 / n3, mu2 = s2 / n3;
  const double* g2 = g + (long long)(M - n3) * ld;
  double ss1 = 0.0, ss2 = 0.0;
  constexpr int H = kDiagAhead / 2;
  const int np = n3 / H;
  for (int q = 0; q < np; ++q) {
    double a[H], b[H];
CCMM_DIAG_UNROLL
    for (int u = 0; u < H; ++u) {
      a[u] = g[(long long)(q * H + u) * ld];
      b[u] = g2[(long long)(q * H + u) * ld];
    }
CCMM_DIAG_UNROLL
    for (int u = 0; u < H; ++u) {
      const double x = a[u] - mu1, y = b[u] - mu2;
      ss1 = ss1 + x * x;
      ss2 = ss2 + y * y;
    }
  }
  for (int t = np * H; t < n3; ++t) {
    const double x = g[(long long)t * ld] - mu1, y = g2[(long long)t * ld] - mu2;
    ss1 = ss1 + x * x;
    ss2 = ss2 + y * y;
  }
  double W = 0.0;
  W = W + ss1;
  W = W + ss2;
  W = W / ((double)(n3 - 1) * 2);  // :107
  double mbar = 0.0;                // :111
  mbar = mbar + mu1;
  mbar = mbar + mu2;
  mbar = mbar / 2;
  double Bpn = 0.0;                 // :112-116
  const double x1 = mu1 - mbar, x2 = mu2 - mbar;
  Bpn = Bpn + x1 * x1;
  Bpn = Bpn + x2 * x2;
  Bpn = Bpn / (2 - 1);
  const double Sv = (double)(n3 - 1) / n3 * W + Bpn;                       // :119
  const double R = (double)(2 + 1) / 2 * Sv / W - (double)(n3 - 1) / 2 / n3;  // :120
  st[10] = sqrt(R);                                                        // :122
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- launchers (ccmm_diagk.hip)
// k_diag_series: series e of chain c is base[c * ld_chain + m * ld_draw + e], m = 0..M-1 (entry fastest);
// statistic k to out[(k * C + c) * S + e].  nvalid (device, C ints, or null): the entries e >= nvalid[c] of
// chain c are not computed; mask (device, S bytes, or null): the entries with mask[e] == 0 are not computed.
// Entries that are not computed get NaN in all 11 statistics.
hipError_t diag_launch(hipStream_t st, const double* base, long long ld_draw, long long ld_chain, int S, int C, int M,
                       const int* nvalid, const unsigned char* mask, double* out);
// in[s * M + m] -> out[m * S + s] (ccmm_diagnostics: host draws, series-major, to entry-fastest order)
hipError_t diag_transpose_launch(hipStream_t st, const double* in, int M, int S, double* out);
#endif

}  // namespace ccmm

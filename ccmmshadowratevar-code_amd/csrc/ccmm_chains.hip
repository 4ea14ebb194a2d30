// The chain set's set-up and data side (ccmm_chains.h): buffers and layouts, data slots and priors, the chain
// state, the parity exports and the profile, then their entry points.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ccmm_chains.h"

using namespace ccmm;

// the KernelId entries by name (ccmm_chains_kernel_times)
const char* const kKernelNames[KID_COUNT] = {
    "k_resid",       "k_cta_weights",   "k_cta_solve", "k_astep",    "k_sv_mix",   "k_sv_part",       "k_phi_gen",
    "k_phi",         "k_store",         "k_gram_chol", "k_elb_prep", "k_elb_cond", "k_elb_gibbs",     "k_elb_rebuild",
    "k_gram_chol_lag", "k_cta_solve_lag", "k_fcst",    "k_gram_big", "k_chol_big", "k_cta_solve_big", "k_astep_big",
    "k_sv_big",      "k_phi_big",       "k_ps_chol",   "k_ps_prop",
    "k_eig_maxroot", "k_stat_select", "k_diag_series", "k_girf_prep", "k_girf", "k_girf_rb", "k_girf_collect",
    "k_cond_mean",
    "k_vma",         "k_sum_ffr",     "k_gather_pai", "k_post_stats"};

void ccmm_chains::init(ccmm_ctx* c, const ccmm_chain_config& cf, int nX, int nY) {
  ctx = c;
  cfg = cf;
  opt = c->opt;
  bh = cf.model == CCMM_MODEL_BLOCKHYBRID || cf.model == CCMM_MODEL_HYBRID || cf.model == CCMM_MODEL_SHADOWRATE;
  // mcmcVARshadowrate.m: the ELB step of the block hybrid, one shadow-rate design for every
  // equation (no actual-rate block), the linear model's predictive density (:536-641)
  fcst_bh = bh && cf.model != CCMM_MODEL_SHADOWRATE;
  hybrid = cf.model == CCMM_MODEL_HYBRID;
  if (bh) {
    require(cf.Ns >= 1 && cf.Ns <= kElbNsMax, "Ns must be in [1, 5]");
    require(cf.elbTmax >= 0 && cf.elbTmax <= cf.T, "elbTmax must be in [0, T]");
    require(cf.elbTmax < 65536, "elbTmax must be < 65536");  // k_elb_gibbs month list
    require(cf.elb_gibbsburn >= 0, "elb_gibbsburn must be >= 0");
    require(2 * cf.p * cf.Ns <= kElbColMax, "2 p Ns must be <= 128");
    require(cf.p >= 1, "p must be >= 1");
  }
  require(cf.N >= 1 && cf.N <= kBigMaxN, "N must be in [1, 128]");
  if (hybrid)  // [1, lags of the N variables, lags of the Ns actual rates] (mcmcVARhybridGibbs.m:84)
    require(cf.K == cf.N * cf.p + 1 + cf.Ns * cf.p, "hybrid model: K must equal N*p+1+Ns*p");
  else
    require(cf.K == cf.N * cf.p + 1 || cf.p == 0, "K must equal N*p+1");
  require(cf.K >= 1 && cf.K <= 1536, "K must be in [1, 1536]");
  // one month: the block calls of the large-N path only (k_sv_big then makes one forward step; a data slot
  // still needs T >= 2, set_T); the small-path kernels are not run below two months
  require((cf.T >= 2 || (cf.T == 1 && cf.N > kMaxNSmall)) && cf.B >= 1 && cf.ndata >= 1, "bad T/B/ndata");
  d.N = cf.N;
  d.p = cf.p;
  d.K = cf.K;
  d.KP = round_up(cf.K, kTile);
  d.TP = round_up(cf.T, kTChunk);
  d.B = cf.B;
  d.nmat = cf.B * cf.N;
  require(d.KP <= kBigMaxKP, "this build supports K <= 1536");
  // KP > 256: the register-tiled fused Gram + Cholesky (k_gram_chol) stops at 16 tiles; the
  // large path takes every larger system (the hybrid model, K = 277, included)
  big = d.KP > 256 || cf.N > kMaxNSmall || opt[OPT_LARGE_PATH] != 0;
  nslabX = nX;
  nslabY = nY;
  const size_t B = cf.B, N = cf.N, KP = d.KP, TP = d.TP;
  hT.assign(cf.ndata, cf.T);
  have_slot.assign(cf.ndata, false);
  Tslot.alloc(cf.ndata);
  slot.alloc(B);
  xidx.alloc(B * N);
  yidx.alloc(B);
  status.alloc(B);
  Xpool.alloc((size_t)nX * KP * TP);
  Ypool.alloc((size_t)nY * N * TP);
  HIPCHECK(hipMemsetAsync(Xpool.p, 0, Xpool.n * sizeof(double), ctx->stream));
  HIPCHECK(hipMemsetAsync(Ypool.p, 0, Ypool.n * sizeof(double), ctx->stream));
  init_lag(nX);
  init_colx();
  iVdiag.alloc((size_t)cf.ndata * N * KP);
  iVb.alloc((size_t)cf.ndata * N * KP);
  sPHI.alloc((size_t)cf.ndata * N * N);
  V0inv.alloc((size_t)cf.ndata * N * N);
  V0invm.alloc((size_t)cf.ndata * N);
  PAI.alloc(B * N * KP);
  HIPCHECK(hipMemsetAsync(PAI.p, 0, PAI.n * sizeof(double), ctx->stream));
  A.alloc(B * N * N);
  invA.alloc(B * N * N);
  sqrtht.alloc(B * N * TP);
  h.alloc(B * N * TP);
  h0.alloc(B * N);
  sqrtPHI.alloc(B * N * N);
  PHI.alloc(B * N * N);
  E.alloc(B * N * TP);
  logy2.alloc(B * N * TP);
  eta.alloc(B * N * TP);
  svobs.alloc(B * N * TP);
  svir.alloc(B * N * TP);
  kai.alloc(B * N * TP);
  W.alloc(B * N * TP);
  ih2.alloc(B * N * TP);
  std::vector<int> zeros(cf.ndata, cf.T);
  HIPCHECK(hipMemcpyAsync(Tslot.p, zeros.data(), cf.ndata * sizeof(int), hipMemcpyHostToDevice,
                          ctx->stream));
  if (bh) init_elb();
  std::vector<int> sl(B, 0);
  set_slots(sl.data());
  HIPCHECK(hipMemsetAsync(status.p, 0, B * sizeof(int), ctx->stream));
  layout_crn();
}

// CRN layout (blocks in CCMM_RNG_* order, sizes from Tmax); the predictive-density
// block (mcmcVAR.m:302,306) is appended once ccmm_chains_set_fcst configured it
void ccmm_chains::layout_crn() {
  const ccmm_chain_config& cf = cfg;
  const int64_t N = cf.N;
  int64_t o = 0;
  const int64_t T = cf.T;
  crn_off[CCMM_RNG_PAI] = o;
  o += (int64_t)cf.K * N;
  crn_off[CCMM_RNG_A] = o;
  o += (int64_t)N * (N - 1) / 2;
  crn_off[CCMM_RNG_SVU] = o;
  o += (int64_t)N * T;
  crn_off[CCMM_RNG_SVZ] = o;
  o += (int64_t)N * (T + 1);
  crn_off[CCMM_RNG_PHI] = o;
  o += (int64_t)N * (T + cf.dPHI);
  if (bh) {
    crn_off[CCMM_RNG_ELB] = o;
    o += (int64_t)cf.Ns * cf.elbTmax * (cf.elb_gibbsburn + 1);
  }
  if (have_fcst) {
    crn_off[CCMM_RNG_FCST] = o;
    o += 2 * N * fH * fNd;
  }
  if (bh && ps_np > 0) {  // randn(nmiss, Nproposals), column-major with leading dimension nmiss
    crn_off[CCMM_RNG_PS] = o;
    o += (int64_t)cf.Ns * cf.elbTmax * ps_np;
  }
  if (bh && elb_alt) {  // randn(nmiss, 1) of the alternate draw (:471-475), last
    crn_off[CCMM_RNG_PSALT] = o;
    o += (int64_t)cf.Ns * cf.elbTmax;
  }
  crn_len = o;
}

// The lag path needs X = [1, lags 1..p of the N variables] (mcmcVAR.m:62-72), a
// supported tile count and D + weights resident in one CU's LDS.
void ccmm_chains::init_lag(int nX) {
  slot_lag.assign(cfg.ndata, false);
  lag_capable = false;
  if (cfg.p < 1 || cfg.K != cfg.N * cfg.p + 1) return;
  const int N = cfg.N;
  lagNT = (N * cfg.p + 15) / 16;
  ldd = (N % 2 == 0) ? N + 1 : N + 2;  // odd stride, spare zero column N
  drows = cfg.T + cfg.p + 4;  // SYRK k-steps read up to row T + p + 2
  if (!lag_supported_nt(lagNT) || N > 32 || 16 * lagNT + 1 > d.KP ||
      gl_lds_bytes(lagNT, drows, ldd, d.TP) > kLdsCu ||
      sl_lds_bytes(lagNT, drows, ldd, d.TP, n_bucket(N)) > kLdsCu)
    return;
  lag_capable = true;
  Dpool.alloc((size_t)nX * drows * ldd);
  HIPCHECK(hipMemsetAsync(Dpool.p, 0, Dpool.n * sizeof(double), ctx->stream));
  std::vector<int> cm(16 * lagNT);
  for (int a = 0; a < 16 * lagNT; ++a) {
    if (a < N * cfg.p) {
      const int l = a / N + 1, k = a % N;
      cm[a] = (cfg.p - l) * ldd + k;
    } else {
      cm[a] = N;  // spare zero column of row t
    }
  }
  dColmap.alloc(cm.size());
  HIPCHECK(hipMemcpy(dColmap.p, cm.data(), cm.size() * sizeof(int), hipMemcpyHostToDevice));
}

// the lag twin of the large path: columns 0..N-1 the data, N..N+Ns-1 the hybrid's actual-rate
// columns (mcmcVARhybridGibbs.m:77-84), then a column of ones (the intercept) and a zero column
// (padded coefficients); row p + t = month t, rows 0..p-1 the presample
void ccmm_chains::init_colx() {
  if (colx_capable || !big || cfg.p < 1) return;
  slot_colx.assign(cfg.ndata, false);
  const int N = cfg.N, p = cfg.p, ex = hybrid ? cfg.Ns : 0;
  if (cfg.K != N * p + 1 + ex * p) return;
  dcext = ex;
  dcld = round_up(d.TP + p, 8);
  dcslab = (size_t)(N + ex + 2) * dcld;
  Dcpool.alloc((size_t)nslabX * dcslab);
  HIPCHECK(hipMemsetAsync(Dcpool.p, 0, Dcpool.n * sizeof(double), ctx->stream));
  std::vector<int> off(d.KP);
  for (int a = 0; a < d.KP; ++a) {
    if (a == 0) {
      off[a] = (N + ex) * dcld;
    } else if (a >= cfg.K) {
      off[a] = (N + ex + 1) * dcld;
    } else if (a - 1 < N * p) {
      const int b = a - 1, l = b / N + 1, k = b % N;
      off[a] = k * dcld + p - l;
    } else {
      const int b = a - 1 - N * p, l = b / ex + 1, si = b % ex;
      off[a] = (N + si) * dcld + p - l;
    }
  }
  dXoff.alloc(d.KP);
  HIPCHECK(hipMemcpy(dXoff.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
  colx_capable = true;
}

// a slot's twin from its X (T x K): column k's rows from the lag-1 column one month later and the
// presample from X's first row; exact check against every entry of X
void ccmm_chains::try_upload_Dc(int slot, int T, const double* X) {
  if (!colx_capable) return;
  slot_colx[slot] = false;
  const int N = cfg.N, p = cfg.p, K = cfg.K, ex = dcext, nc = N + ex;
  std::vector<double> D(dcslab, 0.0);
  std::vector<int> off(K);
  HIPCHECK(hipMemcpy(off.data(), dXoff.p, K * sizeof(int), hipMemcpyDeviceToHost));
  auto colk = [&](int k, int l) { return k < N ? 1 + (l - 1) * N + k : 1 + N * p + (l - 1) * ex + (k - N); };
  for (int k = 0; k < nc; ++k) {
    for (int l = 1; l <= p; ++l) D[(size_t)k * dcld + p - l] = X[(size_t)colk(k, l) * T];  // rows 0..p-1
    for (int t = 1; t < T; ++t) D[(size_t)k * dcld + p + t - 1] = X[(size_t)colk(k, 1) * T + t];
  }
  for (int t = 0; t < d.TP + p; ++t) D[(size_t)nc * dcld + t] = 1.0;
  for (int a = 0; a < K; ++a)
    for (int t = 0; t < T; ++t)
      if (X[(size_t)a * T + t] != D[(size_t)off[a] + t]) return;
  HIPCHECK(hipMemcpy(Dcpool.p + (size_t)slot * dcslab, D.data(), D.size() * sizeof(double), hipMemcpyHostToDevice));
  slot_colx[slot] = true;
}

bool ccmm_chains::lag_active() const {
  if (!lag_capable || !opt[OPT_LAG]) return false;
  for (int s = 0; s < cfg.ndata; ++s)
    if (!slot_lag[s]) return false;
  return true;
}

// D (rows x ldd) of a slot from its X (T x K) and Y (T x N): rows 0..p-1 from the
// lags of X's first row, rows p.. = Y.  Exact check that X is that lag design.
void ccmm_chains::try_upload_D(int slot, int T, const double* Y, const double* X) {
  slot_lag[slot] = false;
  if (!lag_capable) return;
  const int N = cfg.N, p = cfg.p, K = cfg.K;
  std::vector<double> D((size_t)drows * ldd, 0.0);
  for (int l = 1; l <= p; ++l)
    for (int k = 0; k < N; ++k) D[(size_t)(p - l) * ldd + k] = X[(size_t)(1 + (l - 1) * N + k) * T];
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < N; ++k) D[(size_t)(t + p) * ldd + k] = Y[(size_t)k * T + t];
  for (int t = 0; t < T; ++t) {
    if (X[t] != 1.0) return;
    for (int a = 0; a < K - 1; ++a) {
      const int l = a / N + 1, k = a % N;
      if (X[(size_t)(1 + a) * T + t] != D[(size_t)(t + p - l) * ldd + k]) return;
    }
  }
  HIPCHECK(hipMemcpy(Dpool.p + (size_t)slot * drows * ldd, D.data(), D.size() * sizeof(double),
                     hipMemcpyHostToDevice));
  slot_lag[slot] = true;
}

// PREVdraw.X = X0, PREVdraw.Y = Y0 (mcmcVARshadowrateBlockHybrid.m:310-316)
void ccmm_chains::reset_chain_slabs() {
  if (!bh) return;
  std::vector<int> sl(cfg.B);
  HIPCHECK(hipMemcpy(sl.data(), slot.p, cfg.B * sizeof(int), hipMemcpyDeviceToHost));
  const size_t xs = (size_t)d.KP * d.TP, ys = (size_t)d.N * d.TP;
  for (int c = 0; c < cfg.B; ++c) {
    HIPCHECK(hipMemcpyAsync(Xpool.p + (size_t)(cfg.ndata + c) * xs, Xpool.p + (size_t)sl[c] * xs,
                            xs * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(Ypool.p + (size_t)(cfg.ndata + c) * ys, Ypool.p + (size_t)sl[c] * ys,
                            ys * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (colx_capable)
      HIPCHECK(hipMemcpyAsync(Dcpool.p + (size_t)(cfg.ndata + c) * dcslab, Dcpool.p + (size_t)sl[c] * dcslab,
                              dcslab * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (lag_capable) {
      const size_t ds = (size_t)drows * ldd;
      HIPCHECK(hipMemcpyAsync(Dpool.p + (size_t)(cfg.ndata + c) * ds, Dpool.p + (size_t)sl[c] * ds,
                              ds * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  HIPCHECK(hipStreamSynchronize(ctx->stream));
}

// default index maps for the sweep-level linear model: X/Y slab = data slot
void ccmm_chains::set_slots(const int* sl) {
  const int B = cfg.B, N = cfg.N;
  std::vector<int> xi((size_t)B * N), yi(B);
  for (int c = 0; c < B; ++c) {
    require(sl[c] >= 0 && sl[c] < cfg.ndata, "slot out of range");
    if (bh) {  // CTAsys designs: actual-rate block on the vintage's X, shadow block on the chain's
      yi[c] = cfg.ndata + c;
      for (int j = 0; j < N; ++j)
        xi[(size_t)c * N + j] = hActual[j] ? sl[c] : cfg.ndata + c;
    } else {
      yi[c] = sl[c];
      for (int j = 0; j < N; ++j) xi[(size_t)c * N + j] = sl[c];
    }
  }
  HIPCHECK(hipMemcpyAsync(slot.p, sl, B * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(hipMemcpyAsync(xidx.p, xi.data(), xi.size() * sizeof(int), hipMemcpyHostToDevice,
                          ctx->stream));
  build_groups(xi);
  HIPCHECK(hipMemcpyAsync(yidx.p, yi.data(), yi.size() * sizeof(int), hipMemcpyHostToDevice,
                          ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  resid_valid = false;
}

// systems of a chain that share one X slab, four per Gram workgroup (ccmm_big.hip)
void ccmm_chains::build_groups(const std::vector<int>& xi) {
  const int B = cfg.B, N = cfg.N;
  if (big) {
    std::vector<int4> g;
    for (int c = 0; c < B; ++c) {
      std::vector<bool> done(N, false);
      for (int j = 0; j < N; ++j) {
        if (done[j]) continue;
        int m[4] = {-1, -1, -1, -1}, n = 0;
        for (int q = j; q < N && n < 4; ++q)
          if (!done[q] && xi[(size_t)c * N + q] == xi[(size_t)c * N + j]) {
            m[n++] = c * N + q;
            done[q] = true;
          }
        g.push_back(int4{m[0], m[1], m[2], m[3]});
      }
    }
    nGroups = (int)g.size();
    bigGroups.alloc(g.size());
    HIPCHECK(hipMemcpy(bigGroups.p, g.data(), g.size() * sizeof(int4), hipMemcpyHostToDevice));
  }
}

void ccmm_chains::upload_X(int slab, int T, const double* X) {  // X: T x K column-major
  const int K = d.K, KP = d.KP, TP = d.TP;
  std::vector<double> buf((size_t)KP * TP, 0.0);
  for (int a = 0; a < K; ++a)
    for (int t = 0; t < T; ++t) buf[(size_t)a * TP + t] = X[(size_t)a * T + t];
  HIPCHECK(hipMemcpy(Xpool.p + (size_t)slab * KP * TP, buf.data(), buf.size() * sizeof(double),
                     hipMemcpyHostToDevice));
}
void ccmm_chains::upload_TN(double* dst, int nmat, int T, const double* src, double pad) {
  // nmat matrices of T x N (column-major) -> [m][N][TP]
  const int N = d.N, TP = d.TP;
  std::vector<double> buf((size_t)nmat * N * TP, pad);
  for (int m = 0; m < nmat; ++m)
    for (int i = 0; i < N; ++i)
      for (int t = 0; t < T; ++t)
        buf[((size_t)m * N + i) * TP + t] = src[((size_t)m * N + i) * T + t];
  HIPCHECK(hipMemcpy(dst, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
}
void ccmm_chains::download_TN(const double* srcd, int nmat, int T, double* dst) {
  const int N = d.N, TP = d.TP;
  std::vector<double> buf((size_t)nmat * N * TP);
  HIPCHECK(hipMemcpy(buf.data(), srcd, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int m = 0; m < nmat; ++m)
    for (int i = 0; i < N; ++i)
      for (int t = 0; t < T; ++t)
        dst[((size_t)m * N + i) * T + t] = buf[((size_t)m * N + i) * TP + t];
}
void ccmm_chains::upload_KN(double* dst, int nmat, const double* src, double pad) {
  const int N = d.N, K = d.K, KP = d.KP;
  std::vector<double> buf((size_t)nmat * N * KP, pad);
  for (int m = 0; m < nmat; ++m)
    for (int j = 0; j < N; ++j)
      for (int a = 0; a < K; ++a)
        buf[((size_t)m * N + j) * KP + a] = src[((size_t)m * N + j) * K + a];
  HIPCHECK(hipMemcpy(dst, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
}
void ccmm_chains::download_KN(const double* srcd, int nmat, double* dst) {
  const int N = d.N, K = d.K, KP = d.KP;
  std::vector<double> buf((size_t)nmat * N * KP);
  HIPCHECK(hipMemcpy(buf.data(), srcd, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int m = 0; m < nmat; ++m)
    for (int j = 0; j < N; ++j)
      for (int a = 0; a < K; ++a)
        dst[((size_t)m * N + j) * K + a] = buf[((size_t)m * N + j) * KP + a];
}

void ccmm_chains::set_slot_prior(int s, const double* iVd, const double* ivb, const double* sP,
                                 const double* h0mean, const double* h0vcvsqrt) {
  const int N = d.N;
  upload_KN(iVdiag.p + (size_t)s * N * d.KP, 1, iVd, 1.0);
  upload_KN(iVb.p + (size_t)s * N * d.KP, 1, ivb, 0.0);
  HIPCHECK(hipMemcpy(sPHI.p + (size_t)s * N * N, sP, N * N * sizeof(double), hipMemcpyHostToDevice));
  set_slot_h0(s, h0mean, h0vcvsqrt);
}
void ccmm_chains::set_slot_h0(int s, const double* h0mean, const double* h0vcvsqrt) {
  const int N = d.N;
  std::vector<double> V0(N * N, 0.0);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      double v = 0;
      for (int k = 0; k < N; ++k) v += h0vcvsqrt[i + k * N] * h0vcvsqrt[j + k * N];
      V0[i + j * N] = v;
    }
  std::vector<double> Vi = host_spd_inverse(V0, N);
  std::vector<double> m(N, 0.0);
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < N; ++k) m[i] += Vi[i + k * N] * h0mean[k];
  HIPCHECK(hipMemcpy(V0inv.p + (size_t)s * N * N, Vi.data(), N * N * sizeof(double),
                     hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(V0invm.p + (size_t)s * N, m.data(), N * sizeof(double), hipMemcpyHostToDevice));
}
void ccmm_chains::set_T(int s, int T) {
  require(T >= 2 && T <= cfg.T, "slot T out of range");
  hT[s] = T;
  HIPCHECK(hipMemcpy(Tslot.p + s, &T, sizeof(int), hipMemcpyHostToDevice));
}

ChainState ccmm_chains::view() {
  ChainState cs;
  cs.slot = slot.p;
  cs.PAI = PAI.p;
  cs.A = A.p;
  cs.invA = invA.p;
  cs.sqrtht = sqrtht.p;
  cs.h = h.p;
  cs.sqrtPHI = sqrtPHI.p;
  cs.PHI = PHI.p;
  cs.E = E.p;
  cs.logy2 = logy2.p;
  cs.eta = eta.p;
  cs.svobs = svobs.p;
  cs.svir = svir.p;
  cs.kai = kai.p;
  cs.W = W.p;
  cs.ih2 = ih2.p;
  cs.G = G.p;
  cs.svLd = svLd.p;
  cs.svw = svw.p;
  cs.Zphi = Zphi.p;
  cs.status = status.p;
  cs.Aelb = aswitch ? AelbD.p : nullptr;
  cs.atELB = aswitch ? atELBD.p : nullptr;
  return cs;
}

// The parity exports' common part: weights and k_gram_chol_lag at the current state in LagSel mode `mode`,
// every system's record left in G
void ccmm_chains::export_lag_gram(const char* inactive, int mode) {
  require(lag_active(), inactive);
  ensure_cta();
  ChainState cs = view();
  HIPCHECK(launch_cta_weights(ctx->stream, d, Tslot.p, cs, 1));
  LagSel ls = lagsel();
  ls.mode = mode;
  HIPCHECK(lag_launch_gram(lagNT, ctx->stream, gl_lds_bytes(lagNT, drows, ldd, d.TP), d, Tslot.p, ls, cs, iVdiag.p));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
}

// Parity export: the lag path's weighted Gram of every (chain, equation) system at the current
// state, [c b'; b M] (K x K, without the prior), decoded from the kernel's tile slots
void ccmm_chains::export_cta_gram(double* out) {
  export_lag_gram("ccmm_chains_get_cta_gram: the lag-structured CTA path is not active", kLagGramExport);
  const int NT = lagNT, NTILE = gl_ntile(NT), K = d.K, KL = K - 1;
  std::vector<double> o((size_t)gl_out_len(NT));
  for (int mat = 0; mat < d.nmat; ++mat) {
    HIPCHECK(hipMemcpy(o.data(), G.p + (size_t)mat * d.KP * d.KP, o.size() * sizeof(double),
                       hipMemcpyDeviceToHost));
    double* Gm = out + (size_t)mat * K * K;
    Gm[0] = o[(size_t)NTILE * 256];
    for (int a = 0; a < KL; ++a) Gm[1 + a] = Gm[(size_t)(1 + a) * K] = o[(size_t)NTILE * 256 + 1 + a];
    for (int gi = 0; gi < NTILE; ++gi) {
      const int ti = gl_ti(NT, gi), tj = gl_tj(NT, gi);
      for (int r = 0; r < 4; ++r)
        for (int lane = 0; lane < 64; ++lane) {
          const int row = 16 * tj + (lane >> 4) + 4 * r, col = 16 * ti + (lane & 15);  // upper tile (tj, ti)
          if (row < KL && col < KL) {
            const double v = o[(size_t)gi * 256 + 64 * r + lane];
            Gm[(size_t)(1 + row) + (size_t)(1 + col) * K] = v;
            Gm[(size_t)(1 + col) + (size_t)(1 + row) * K] = v;
          }
        }
    }
  }
}

// Parity export: the lag path's factor record of every (chain, equation) system at the current
// state as k_gram_chol_lag writes it (gl_out_len(NT) doubles per system: the factor tiles in
// slot layout, then [1 / L00, L(1 + a, 0)])
void ccmm_chains::export_cta_factor(double* out) {
  export_lag_gram("ccmm_chains_get_cta_factor: the lag-structured CTA path is not active", lagsel().mode);
  const size_t n = (size_t)gl_out_len(lagNT);
  for (int mat = 0; mat < d.nmat; ++mat)
    HIPCHECK(hipMemcpy(out + (size_t)mat * n, G.p + (size_t)mat * d.KP * d.KP, n * sizeof(double),
                       hipMemcpyDeviceToHost));
}

void ccmm_chains::ensure_aux() {
  if (!aux) HIPCHECK(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
  phiEv.ensure();
}

hipEvent_t ccmm_chains::get_event() {
  if (!evpool.empty()) {
    hipEvent_t e = evpool.back();
    evpool.pop_back();
    return e;
  }
  hipEvent_t e;
  HIPCHECK(hipEventCreate(&e));
  return e;
}

void ccmm_chains::collect_profile() {
  if (pending.empty()) return;
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  for (auto& e : pending) {
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, e.a, e.b));
    kms[e.kid] += ms;
    kcount[e.kid] += 1;
    evpool.push_back(e.a);
    evpool.push_back(e.b);
  }
  pending.clear();
}

ccmm_chains::~ccmm_chains() {
  // the side streams drain here; their events (phiEv, specEv, fcstEv, declared with the streams in ccmm_chains.h)
  // are destroyed after this body, with the members, so after the streams they were recorded on
  if (aux2) {
    (void)hipStreamSynchronize(aux2);
    (void)hipStreamDestroy(aux2);
  }
  if (aux) {
    (void)hipStreamSynchronize(aux);
    (void)hipStreamDestroy(aux);
  }
  if (mfma_ev) {
    PhaseLock& L = phase_lock(ctx->device, mfma_lock);
    std::lock_guard<std::mutex> g(L.m);
    if (L.last == mfma_ev) L.last = nullptr;
    (void)hipEventDestroy(mfma_ev);
  }
  for (auto& e : pending) {
    evpool.push_back(e.a);
    evpool.push_back(e.b);
  }
  for (auto e : evpool) (void)hipEventDestroy(e);
}

extern "C" {

ccmm_chains* ccmm_chains_create(ccmm_ctx* ctx, const ccmm_chain_config* cfg) {
  ccmm_chains* ch = nullptr;
  int rc = guarded([&] {
    require(ctx && cfg, "null argument");
    require(cfg->model == CCMM_MODEL_LINEAR || cfg->model == CCMM_MODEL_BLOCKHYBRID ||
                cfg->model == CCMM_MODEL_HYBRID || cfg->model == CCMM_MODEL_SHADOWRATE, "unknown model");
    HIPCHECK(hipSetDevice(ctx->device));
    ch = new ccmm_chains;
    const int extra = cfg->model != CCMM_MODEL_LINEAR ? cfg->B : 0;
    ch->init(ctx, *cfg, cfg->ndata + extra, cfg->ndata + extra);
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    const std::string ign = ignored_list();
    if (!ign.empty())  // a warning, not an error: the draws are valid, the switches had no effect
      set_last_error("default build: timing-only ablation switches ignored (" + ign + "); build libccmm_ablation.so to use them");
    return 0;
  });
  if (rc != 0) {
    delete ch;
    return nullptr;
  }
  return ch;
}

int ccmm_chains_set_option(ccmm_chains* ch, const char* name, int value) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    const int i = option_id(name);
    const int old = i >= 0 ? ch->opt[i] : 0;
    const int rc = set_opt(ch->opt, name, value);
    if (rc != CCMM_OK) return rc;
    if (i == OPT_LARGE_PATH && value != old) {  // the path's grouping of systems follows the choice
      require(!ch->have_state, "option large_path: set it before ccmm_chains_set_data / set_state");
      HIPCHECK(hipSetDevice(ch->ctx->device));
      ch->big = ch->d.KP > 256 || ch->cfg.N > kMaxNSmall || value != 0;
      ch->init_colx();
      std::vector<int> sl(ch->cfg.B);
      HIPCHECK(hipMemcpy(sl.data(), ch->slot.p, ch->cfg.B * sizeof(int), hipMemcpyDeviceToHost));
      ch->set_slots(sl.data());
    }
    if (i == OPT_SOLVE_SPLIT || i == OPT_SOLVE_ASYNC) ch->split_resident = -1;
    return CCMM_OK;
  });
}

int ccmm_chains_get_option(ccmm_chains* ch, const char* name, int* value) {
  if (!ch) {
    set_last_error("null argument");
    return CCMM_ERR_ARG;
  }
  return get_opt(ch->opt, name, value);
}

void ccmm_chains_destroy(ccmm_chains* ch) {
  if (!ch) return;
  (void)hipSetDevice(ch->ctx->device);
  (void)hipStreamSynchronize(ch->ctx->stream);
  delete ch;
}

int ccmm_chains_set_data(ccmm_chains* ch, int slot, int T, const double* Y, const double* X,
                         const double* iVdiag, const double* iVb, const double* sPHI,
                         const double* h0mean, const double* h0vcvsqrt) {
  return guarded([&] {
    require(ch && Y && X && iVdiag && iVb && sPHI && h0mean && h0vcvsqrt, "null argument");
    require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    ch->set_T(slot, T);
    ch->upload_X(slot, T, X);
    ch->try_upload_D(slot, T, Y, X);
    ch->try_upload_Dc(slot, T, X);
    ch->upload_TN(ch->Ypool.p + (size_t)slot * ch->d.N * ch->d.TP, 1, T, Y, 0.0);
    ch->set_slot_prior(slot, iVdiag, iVb, sPHI, h0mean, h0vcvsqrt);
    ch->have_slot[slot] = true;
    ch->resid_valid = false;
    return 0;
  });
}

int ccmm_chains_set_slots(ccmm_chains* ch, const int* slot_of_chain) {
  return guarded([&] {
    require(ch && slot_of_chain, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    ch->set_slots(slot_of_chain);
    return 0;
  });
}

int ccmm_chains_get_kai(ccmm_chains* ch, int8_t* kai) {
  return guarded([&] {
    require(ch && kai, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const int B = ch->d.B, N = ch->d.N, TP = ch->d.TP, T = ch->cfg.T;
    std::vector<int8_t> kk((size_t)B * N * TP);
    HIPCHECK(hipMemcpy(kk.data(), ch->kai.p, kk.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < B; ++c)
      for (int i = 0; i < N; ++i)
        for (int t = 0; t < T; ++t) kai[t + (size_t)T * (i + (size_t)N * c)] = kk[((size_t)c * N + i) * TP + t];
    return 0;
  });
}

int ccmm_chains_set_mfma_lock(ccmm_chains* ch, int id) {
  return guarded([&] {
    require(ch != nullptr && id >= 0, "bad argument");
    require(ch->mfma_ev == nullptr || id == ch->mfma_lock, "MFMA lock id already set");
    ch->mfma_lock = id;
    return 0;
  });
}

int ccmm_chains_set_rng_ids(ccmm_chains* ch, const uint32_t* ids) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    if (!ids) {
      ch->have_ids = false;
      return 0;
    }
    ch->rngIds.alloc(ch->cfg.B);
    HIPCHECK(hipMemcpy(ch->rngIds.p, ids, ch->cfg.B * sizeof(uint32_t), hipMemcpyHostToDevice));
    ch->have_ids = true;
    return 0;
  });
}

int ccmm_chains_get_status(ccmm_chains* ch, int* status) {
  return guarded([&] {
    require(ch && status, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    HIPCHECK(hipMemcpy(status, ch->status.p, ch->cfg.B * sizeof(int), hipMemcpyDeviceToHost));
    int any = 0;
    for (int c = 0; c < ch->cfg.B; ++c) any |= status[c] & ~CCMM_STATUS_INFO;  // bits 1, 64: informational
    return any ? 1 : 0;
  });
}

int ccmm_chains_set_state(ccmm_chains* ch, const double* PAI, const double* A,
                          const double* sqrtht, const double* h, const double* sqrtPHI) {
  return guarded([&] {
    require(ch && PAI && A && sqrtht && h && sqrtPHI, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const int B = ch->d.B, N = ch->d.N, T = ch->cfg.T;
    ch->upload_KN(ch->PAI.p, B, PAI, 0.0);
    HIPCHECK(hipMemcpy(ch->A.p, A, (size_t)B * N * N * sizeof(double), hipMemcpyHostToDevice));
    ch->upload_TN(ch->sqrtht.p, B, T, sqrtht, 1.0);
    ch->upload_TN(ch->h.p, B, T, h, 0.0);
    HIPCHECK(hipMemcpy(ch->sqrtPHI.p, sqrtPHI, (size_t)B * N * N * sizeof(double), hipMemcpyHostToDevice));
    if (ch->bh) {
      if (!ch->have_elb_model) {
        set_last_error("ccmm_chains_set_elb_model must be called before set_state");
        return CCMM_ERR_STATE;
      }
      for (int s = 0; s < ch->cfg.ndata; ++s)
        if (!ch->have_slot[s]) {
          set_last_error("ccmm_chains_set_data missing for a data slot");
          return CCMM_ERR_STATE;
        }
      ch->reset_chain_slabs();
    }
    ch->sweep = 0;
    ch->stored = 0;
    ch->mom_done = 0;  // the store restarts: the running PAI sums are re-based on reset (pai_moments)
    HIPCHECK(hipMemset(ch->status.p, 0, ch->cfg.B * sizeof(int)));
    if (ch->psCount.p) HIPCHECK(hipMemset(ch->psCount.p, 0, 2 * (size_t)ch->cfg.B * sizeof(int)));
    if (ch->have_fcst) ch->reset_fcst();
    ch->statRedraws.assign(ch->cfg.B, 0);
    ch->resid_valid = false;
    ch->have_state = true;
    return 0;
  });
}

int ccmm_chains_get_state(ccmm_chains* ch, double* PAI, double* A, double* invA, double* sqrtht,
                          double* h, double* sqrtPHI, double* PHI, double* RESID) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const int B = ch->d.B, N = ch->d.N, T = ch->cfg.T;
    const size_t nn = (size_t)B * N * N * sizeof(double);
    if (PAI) ch->download_KN(ch->PAI.p, B, PAI);
    if (A) HIPCHECK(hipMemcpy(A, ch->A.p, nn, hipMemcpyDeviceToHost));
    if (invA) HIPCHECK(hipMemcpy(invA, ch->invA.p, nn, hipMemcpyDeviceToHost));
    if (sqrtht) ch->download_TN(ch->sqrtht.p, B, T, sqrtht);
    if (h) ch->download_TN(ch->h.p, B, T, h);
    if (sqrtPHI) HIPCHECK(hipMemcpy(sqrtPHI, ch->sqrtPHI.p, nn, hipMemcpyDeviceToHost));
    if (PHI) HIPCHECK(hipMemcpy(PHI, ch->PHI.p, nn, hipMemcpyDeviceToHost));
    if (RESID) ch->download_TN(ch->E.p, B, T, RESID);
    return 0;
  });
}

int64_t ccmm_chains_crn_len(const ccmm_chains* ch) { return ch ? ch->crn_len : -1; }

int ccmm_chains_get_draws(ccmm_chains* ch, double* PAI_all, double* PHI_all, double* invA_all,
                          double* sqrtht_all, double* shadowrate_all) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const size_t B = ch->d.B, N = ch->d.N, K = ch->d.K, cap = ch->cfg.store_capacity;
    const size_t M = ch->stored, T = ch->cfg.T;
    auto fetch = [&](const DBuf<double>& src, size_t per, double* dst) {
      if (!dst || M == 0) return;
      std::vector<double> buf(B * cap * per);
      HIPCHECK(hipMemcpy(buf.data(), src.p, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
      // device [c][m][e] -> MATLAB M x (e...) x B, i.e. dst[m + M*(e + per*c)]
      for (size_t c = 0; c < B; ++c)
        for (size_t m = 0; m < M; ++m)
          for (size_t e = 0; e < per; ++e) dst[m + M * (e + per * c)] = buf[(c * cap + m) * per + e];
    };
    fetch(ch->sPAI, K * N, PAI_all);
    fetch(ch->sPHI_, N * (N + 1) / 2, PHI_all);
    fetch(ch->sInvA, N * N, invA_all);
    fetch(ch->sSqrtht, T * N, sqrtht_all);
    if (ch->bh && ch->cfg.elbTmax > 0) fetch(ch->sShadow, (size_t)ch->cfg.Ns * ch->cfg.elbTmax, shadowrate_all);
    ch->stored = 0;
    ch->mom_done = 0;
    return 0;
  });
}

int ccmm_chains_pai_moments(ccmm_chains* ch, int reset, double* sum, double* sumsq) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    const size_t B = ch->d.B, per = (size_t)ch->d.K * ch->d.N;
    if (!ch->paiMom.p || reset) {
      ch->paiMom.alloc(2 * B * per);
      HIPCHECK(hipMemsetAsync(ch->paiMom.p, 0, 2 * B * per * sizeof(double), ch->ctx->stream));
      ch->mom_done = 0;
    }
    require(ch->stored >= ch->mom_done, "ccmm_chains_pai_moments: the store was reset; call with reset != 0");
    if (ch->stored > ch->mom_done && ch->sPAI.p) {
      HIPCHECK(launch_pai_moments(ch->ctx->stream, ch->sPAI.p, ch->cfg.store_capacity, ch->mom_done, ch->stored,
                                  (int)per, (int)B, ch->paiMom.p, ch->paiMom.p + B * per));
      ch->mom_done = ch->stored;
    }
    if (sum || sumsq) {
      std::vector<double> buf(2 * B * per);
      HIPCHECK(hipMemcpyAsync(buf.data(), ch->paiMom.p, buf.size() * sizeof(double), hipMemcpyDeviceToHost,
                              ch->ctx->stream));
      HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
      // device [c][e] (e = a + K j) -> K x N x B
      if (sum) std::copy(buf.begin(), buf.begin() + B * per, sum);
      if (sumsq) std::copy(buf.begin() + B * per, buf.end(), sumsq);
    }
    return 0;
  });
}

int ccmm_chains_get_cta_gram(ccmm_chains* ch, double* G) {
  return guarded([&] {
    require(ch && G, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    ch->export_cta_gram(G);
    return 0;
  });
}

int ccmm_chains_get_cta_factor(ccmm_chains* ch, double* F) {
  return guarded([&] {
    require(ch && F, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    ch->export_cta_factor(F);
    return 0;
  });
}

int ccmm_chains_get_xy(ccmm_chains* ch, double* X, double* Y) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const int B = ch->d.B, N = ch->d.N, K = ch->d.K, KP = ch->d.KP, TP = ch->d.TP, T = ch->cfg.T;
    std::vector<int> sl(B);
    HIPCHECK(hipMemcpy(sl.data(), ch->slot.p, B * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<double> xb((size_t)KP * TP), yb((size_t)N * TP);
    for (int c = 0; c < B; ++c) {
      const int xs = ch->bh ? ch->cfg.ndata + c : sl[c];
      if (X) {
        HIPCHECK(hipMemcpy(xb.data(), ch->Xpool.p + (size_t)xs * KP * TP, xb.size() * sizeof(double),
                           hipMemcpyDeviceToHost));
        for (int a = 0; a < K; ++a)
          for (int t = 0; t < T; ++t) X[((size_t)c * K + a) * T + t] = xb[(size_t)a * TP + t];
      }
      if (Y) {
        HIPCHECK(hipMemcpy(yb.data(), ch->Ypool.p + (size_t)xs * N * TP, yb.size() * sizeof(double),
                           hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i)
          for (int t = 0; t < T; ++t) Y[((size_t)c * N + i) * T + t] = yb[(size_t)i * TP + t];
      }
    }
    return 0;
  });
}

int ccmm_chains_profile(ccmm_chains* ch, int enable) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    ch->collect_profile();
    ch->profiling = enable != 0;
    for (int k = 0; k < KID_COUNT; ++k) {
      ch->kms[k] = 0.0;
      ch->kcount[k] = 0;
    }
    return 0;
  });
}

int ccmm_chains_kernel_times(ccmm_chains* ch, int max, double* ms, int64_t* launches, char* names,
                             int names_len) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    ch->collect_profile();
    const int n = std::min<int>(max, KID_COUNT);
    for (int k = 0; k < n; ++k) {
      if (ms) ms[k] = ch->kms[k];
      if (launches) launches[k] = ch->kcount[k];
    }
    if (names && names_len > 0) {
      std::string s;
      for (int k = 0; k < KID_COUNT; ++k) {
        if (k) s += ";";
        s += kKernelNames[k];
      }
      std::strncpy(names, s.c_str(), names_len - 1);
      names[names_len - 1] = 0;
    }
    return KID_COUNT;
  });
}
}  // extern "C"

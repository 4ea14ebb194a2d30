// The block-level drop-ins of include/ccmm.h: each call builds a throw-away chain set (ccmm_chains.h) around its
// arguments, runs one block of the sweep on it and copies the result back.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ccmm_chains.h"
#include "ccmm_girf.h"

using namespace ccmm;

static ccmm_chain_config block_cfg(int B, int T, int N, int K) {
  ccmm_chain_config cf{};
  cf.model = CCMM_MODEL_LINEAR;
  cf.N = N;
  cf.p = 0;  // K free-form for the block call
  cf.K = K;
  cf.T = T;
  cf.B = B;
  cf.ndata = 1;
  cf.dPHI = N + 3;
  cf.rng_crn = 1;
  cf.logy2offset = 1e-3;
  cf.seed = 0;
  return cf;
}

// an optional CRN array of block `id` (n doubles per chain; nullptr: Philox) uploaded into dz, and the RngArgs on it
static RngArgs crn_args(ccmm_chains& ch, DBuf<double>& dz, const double* z, int64_t n, int id) {
  if (z && n > 0) {
    dz.alloc((size_t)ch.cfg.B * n);
    HIPCHECK(hipMemcpy(dz.p, z, dz.n * sizeof(double), hipMemcpyHostToDevice));
  }
  RngArgs ra = ch.rng_args(dz.p, n);
  ra.off[id] = 0;
  return ra;
}

extern "C" {

static int cta_impl(ccmm_ctx* ctx, int B, int T, int N, int K, const double* Y, int y_per_chain,
                    const double* X, int nx, int x_per_chain, const double* A, const double* Aelb,
                    const uint8_t* atELB, const double* sqrtht, const double* iVdiag, const double* iVb,
                    double* PAI, const double* z, int* status) {
  return guarded([&] {
    require(ctx && Y && X && A && sqrtht && iVdiag && iVb && PAI, "null argument");
    require(nx == 1 || nx == N, "nx must be 1 (CTA) or N (CTAsys)");
    require((Aelb == nullptr) == (atELB == nullptr), "Aelb and atELB go together");
    HIPCHECK(hipSetDevice(ctx->device));
    ccmm_chains ch;
    const int nX = nx * (x_per_chain ? B : 1), nY = y_per_chain ? B : 1;
    ch.init(ctx, block_cfg(B, T, N, K), nX, nY);
    if (Aelb) {
      require(!ch.big, "CTAsysAswitching: supported for K <= 256 and N <= 32");
      ch.aswitch = true;
      ch.AelbD.alloc((size_t)B * N * N);
      HIPCHECK(hipMemcpy(ch.AelbD.p, Aelb, (size_t)B * N * N * sizeof(double), hipMemcpyHostToDevice));
      std::vector<uint8_t> at((size_t)B * ch.d.TP, 0);
      for (int c = 0; c < B; ++c)
        for (int t = 0; t < T; ++t) at[(size_t)c * ch.d.TP + t] = atELB[t] ? 1 : 0;
      ch.atELBD.alloc(at.size());
      HIPCHECK(hipMemcpy(ch.atELBD.p, at.data(), at.size(), hipMemcpyHostToDevice));
    }
    for (int q = 0; q < nX; ++q) ch.upload_X(q, T, X + (size_t)q * T * K);
    ch.upload_TN(ch.Ypool.p, nY, T, Y, 0.0);
    std::vector<int> xi((size_t)B * N), yi(B);
    for (int c = 0; c < B; ++c) {
      yi[c] = y_per_chain ? c : 0;
      for (int j = 0; j < N; ++j) xi[(size_t)c * N + j] = (x_per_chain ? c * nx : 0) + (nx == 1 ? 0 : j);
    }
    HIPCHECK(hipMemcpy(ch.xidx.p, xi.data(), xi.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ch.yidx.p, yi.data(), yi.size() * sizeof(int), hipMemcpyHostToDevice));
    ch.build_groups(xi);
    ch.upload_KN(ch.iVdiag.p, 1, iVdiag, 1.0);
    ch.upload_KN(ch.iVb.p, 1, iVb, 0.0);
    HIPCHECK(hipMemcpy(ch.A.p, A, (size_t)B * N * N * sizeof(double), hipMemcpyHostToDevice));
    ch.upload_TN(ch.sqrtht.p, B, T, sqrtht, 1.0);
    ch.upload_KN(ch.PAI.p, B, PAI, 0.0);
    DBuf<double> dz;
    const RngArgs ra = crn_args(ch, dz, z, (int64_t)K * N, CCMM_RNG_PAI);
    ch.snapshot_pai();
    ch.run_cta(ra);
    ch.cta_fallback(ra);  // CTA.m:80-92 for the chains whose Cholesky failed
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    ch.download_KN(ch.PAI.p, B, PAI);
    std::vector<int> st(B);
    HIPCHECK(hipMemcpy(st.data(), ch.status.p, B * sizeof(int), hipMemcpyDeviceToHost));
    int any = 0;
    for (int c = 0; c < B; ++c) {
      if (status) status[c] = st[c] & 1;
      any |= st[c];
    }
    if (any & ~1) {
      set_last_error("posterior precision singular: QR fallback failed");
      return CCMM_ERR_NOTSPD;
    }
    if (any & 1) {
      set_last_error("switching to QR routine");  // CTA.m:82
      return CCMM_WARN_QR_FALLBACK;
    }
    return 0;
  });
}

int ccmm_cta(ccmm_ctx* ctx, int B, int T, int N, int K, const double* Y, int y_per_chain,
             const double* X, int nx, int x_per_chain, const double* A, const double* sqrtht,
             const double* iVdiag, const double* iVb, double* PAI, const double* z, int* status) {
  return cta_impl(ctx, B, T, N, K, Y, y_per_chain, X, nx, x_per_chain, A, nullptr, nullptr, sqrtht, iVdiag,
                  iVb, PAI, z, status);
}

int ccmm_cta_aswitching(ccmm_ctx* ctx, int B, int T, int N, int K, const double* Y, int y_per_chain,
                        const double* X, int nx, int x_per_chain, const double* A, const double* Aelb,
                        const uint8_t* atELB, const double* sqrtht, const double* iVdiag, const double* iVb,
                        double* PAI, const double* z, int* status) {
  if (!Aelb || !atELB) {
    set_last_error("null argument");
    return CCMM_ERR_ARG;
  }
  return cta_impl(ctx, B, T, N, K, Y, y_per_chain, X, nx, x_per_chain, A, Aelb, atELB, sqrtht, iVdiag, iVb,
                  PAI, z, status);
}

int ccmm_astep(ccmm_ctx* ctx, int B, int T, int N, const double* RESID, const double* sqrtht,
               const double* z, double* A, double* invA) {
  return guarded([&] {
    require(ctx && RESID && sqrtht && A && invA, "null argument");
    HIPCHECK(hipSetDevice(ctx->device));
    ccmm_chains ch;
    ch.init(ctx, block_cfg(B, T, N, 1), 1, 1);
    ch.upload_TN(ch.E.p, B, T, RESID, 0.0);
    ch.upload_TN(ch.sqrtht.p, B, T, sqrtht, 1.0);
    DBuf<double> dz;
    const RngArgs ra = crn_args(ch, dz, z, (int64_t)N * (N - 1) / 2, CCMM_RNG_A);
    ch.run_astep(ra);
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(A, ch.A.p, (size_t)B * N * N * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(invA, ch.invA.p, (size_t)B * N * N * sizeof(double), hipMemcpyDeviceToHost));
    return ch.check_status();
  });
}

int ccmm_sv_ksc(ccmm_ctx* ctx, int B, int T, int N, const double* logy2T, const double* hprevT,
                const double* sqrtPHI, const double* h0mean, const double* h0vcvsqrt,
                const double* u, const double* z, double* hT, double* h0, double* shocksT,
                int8_t* kai2) {
  return guarded([&] {
    require(ctx && logy2T && hprevT && sqrtPHI && h0mean && h0vcvsqrt, "null argument");
    HIPCHECK(hipSetDevice(ctx->device));
    ccmm_chains ch;
    ch.init(ctx, block_cfg(B, T, N, 1), 1, 1);
    // N x T (x B) -> internal [c][i][t]
    std::vector<double> tmp((size_t)B * N * T);
    auto transpose_in = [&](const double* src) {
      for (int c = 0; c < B; ++c)
        for (int t = 0; t < T; ++t)
          for (int i = 0; i < N; ++i)
            tmp[((size_t)c * N + i) * T + t] = src[((size_t)c * T + t) * N + i];
    };
    transpose_in(logy2T);
    ch.upload_TN(ch.logy2.p, B, T, tmp.data(), 0.0);
    transpose_in(hprevT);
    ch.upload_TN(ch.h.p, B, T, tmp.data(), 0.0);
    HIPCHECK(hipMemcpy(ch.sqrtPHI.p, sqrtPHI, (size_t)B * N * N * sizeof(double), hipMemcpyHostToDevice));
    ch.set_slot_h0(0, h0mean, h0vcvsqrt);
    // CRN: u (N x T) and z (N x (T+1)) per chain, packed into one buffer
    DBuf<double> dc;
    const int64_t nu = (int64_t)N * T, nzz = (int64_t)N * (T + 1);
    RngArgs ra = ch.rng_args(nullptr, 0);
    if (u || z) {
      require(u && z, "u and z must both be given or both NULL");
      std::vector<double> buf((size_t)B * (nu + nzz));
      for (int c = 0; c < B; ++c) {
        std::memcpy(&buf[(size_t)c * (nu + nzz)], u + (size_t)c * nu, nu * sizeof(double));
        std::memcpy(&buf[(size_t)c * (nu + nzz) + nu], z + (size_t)c * nzz, nzz * sizeof(double));
      }
      dc.alloc(buf.size());
      HIPCHECK(hipMemcpy(dc.p, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
      ra = ch.rng_args(dc.p, nu + nzz);
      ra.off[CCMM_RNG_SVU] = 0;
      ra.off[CCMM_RNG_SVZ] = nu;
    }
    ch.run_sv(ra);
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    auto transpose_out = [&](const double* dsrc, double* dst) {
      ch.download_TN(dsrc, B, T, tmp.data());
      for (int c = 0; c < B; ++c)
        for (int t = 0; t < T; ++t)
          for (int i = 0; i < N; ++i)
            dst[((size_t)c * T + t) * N + i] = tmp[((size_t)c * N + i) * T + t];
    };
    if (hT) transpose_out(ch.h.p, hT);
    if (shocksT) transpose_out(ch.eta.p, shocksT);
    if (h0) {
      // x_0 = h_1 - shock_1
      std::vector<double> hh((size_t)B * N * T), ee((size_t)B * N * T);
      ch.download_TN(ch.h.p, B, T, hh.data());
      ch.download_TN(ch.eta.p, B, T, ee.data());
      for (int c = 0; c < B; ++c)
        for (int i = 0; i < N; ++i)
          h0[(size_t)c * N + i] = hh[((size_t)c * N + i) * T] - ee[((size_t)c * N + i) * T];
    }
    if (kai2) {
      std::vector<int8_t> kk((size_t)B * N * ch.d.TP);
      HIPCHECK(hipMemcpy(kk.data(), ch.kai.p, kk.size(), hipMemcpyDeviceToHost));
      for (int c = 0; c < B; ++c)
        for (int t = 0; t < T; ++t)
          for (int i = 0; i < N; ++i)
            kai2[((size_t)c * T + t) * N + i] = kk[((size_t)c * N + i) * ch.d.TP + t];
    }
    return ch.check_status();
  });
}

int ccmm_phi_iw(ccmm_ctx* ctx, int B, int T, int N, const double* eta, const double* sPHI,
                int dPHI, const double* Zdraw, double* sqrtPHI, double* PHI) {
  return guarded([&] {
    require(ctx && eta && sPHI && sqrtPHI && PHI, "null argument");
    HIPCHECK(hipSetDevice(ctx->device));
    ccmm_chains ch;
    ccmm_chain_config cf = block_cfg(B, T, N, 1);
    cf.dPHI = dPHI;
    ch.init(ctx, cf, 1, 1);
    ch.upload_TN(ch.eta.p, B, T, eta, 0.0);
    HIPCHECK(hipMemcpy(ch.sPHI.p, sPHI, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice));
    DBuf<double> dz;
    const RngArgs ra = crn_args(ch, dz, Zdraw, (int64_t)N * (T + dPHI), CCMM_RNG_PHI);
    ch.run_phi(ra);
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(sqrtPHI, ch.sqrtPHI.p, (size_t)B * N * N * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(PHI, ch.PHI.p, (size_t)B * N * N * sizeof(double), hipMemcpyDeviceToHost));
    return ch.check_status();
  });
}

int ccmm_draw_trunc_normal_batch(ccmm_ctx* ctx, int n, const double* mu, const double* sig,
                                 double elb, const double* u, double* out, uint8_t* flags) {
  return guarded([&] {
    require(ctx && mu && sig && u && out && n >= 0, "null argument");
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(ctx->device));
    DBuf<double> dmu, dsig, du, dout;
    DBuf<uint8_t> dfl;
    dmu.alloc(n);
    dsig.alloc(n);
    du.alloc(n);
    dout.alloc(n);
    dfl.alloc(n);
    HIPCHECK(hipMemcpy(dmu.p, mu, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dsig.p, sig, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(du.p, u, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(launch_truncnorm(ctx->stream, n, dmu.p, dsig.p, elb, du.p, dout.p, dfl.p));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (flags) HIPCHECK(hipMemcpy(flags, dfl.p, n, hipMemcpyDeviceToHost));
    return 0;
  });
}

// gibbsdrawShadowrates (b3 = 0) and gibbsdrawShadowratesB3 (b3 = 1; Psi K x Ny x elbT per chain when
// psi3d, else K x Ny) on one chain set holding each call as a data slot
static int gibbs_shadowrates_impl(ccmm_ctx* ctx, int B, int Ny, int elbT, int Ns, int p, const uint8_t* ndxS,
                                  const uint8_t* sNaN, const double* Y, const double* STATE0,
                                  const double* YHAT0, const double* C, const double* Psi, const double* SVol,
                                  double elbBound, int Ndraws, int burnin, const double* u, double* out,
                                  uint8_t* flags, int b3, int psi3d) {
  return guarded([&] {
    require(ctx && ndxS && sNaN && Y && STATE0 && C && Psi && SVol && out, "null argument");
    require(B >= 1 && Ny >= 1 && Ny <= 128 && p >= 1 && elbT >= 1 && burnin >= 0, "bad size");
    require(Ndraws == 1, "Ndraws must be 1 (the value used at mcmcVARshadowrateBlockHybrid.m:436)");
    std::vector<int> nd;
    for (int i = 0; i < Ny; ++i)
      if (ndxS[i]) nd.push_back(i);
    if ((int)nd.size() != Ns) {  // gibbsdrawShadowrates.m:50-52
      set_last_error("dimension mismatch");
      return CCMM_ERR_DIM;
    }
    require(Ns >= 1 && Ns <= kElbNsMax, "Ns must be in [1, 5]");
    HIPCHECK(hipSetDevice(ctx->device));
    const int K = Ny * p + 1, T = elbT, passes = burnin + Ndraws;
    ccmm_chain_config cf{};
    cf.model = CCMM_MODEL_BLOCKHYBRID;
    cf.B = B;
    cf.N = Ny;
    cf.p = p;
    cf.T = T;
    cf.K = K;
    cf.ndata = B;  // one data slot per chain: its own Y window and STATE0
    cf.dPHI = Ny + 1;
    cf.logy2offset = 1e-3;
    cf.Ns = Ns;
    cf.elbTmax = T;
    cf.elb_gibbsburn = burnin;
    cf.elb = elbBound;
    cf.rng_crn = u ? 1 : 0;
    cf.seed = 0;
    ccmm_chains ch;
    ch.init(ctx, cf, 2 * B, 2 * B);
    const size_t KK = (size_t)K * K;
    std::vector<double> Xc((size_t)T * K, 0.0), Yc((size_t)T * Ny), ivd((size_t)K * Ny, 1.0),
        ivb((size_t)K * Ny, 0.0), sP((size_t)Ny * Ny, 0.0), h0m(Ny, 0.0), h0v((size_t)Ny * Ny, 0.0);
    for (int i = 0; i < Ny; ++i) sP[i + (size_t)i * Ny] = h0v[i + (size_t)i * Ny] = 1.0;
    std::vector<int> sl(B);
    for (int c = 0; c < B; ++c) {
      // X row 1 = STATE0 (elb.X0 = X(elbT0+1,:)', mcmcVARshadowrateBlockHybrid.m:417), Y = the window
      for (int k = 0; k < K; ++k) Xc[(size_t)k * T] = STATE0[(size_t)c * K + k];
      for (int t = 0; t < T; ++t)
        for (int i = 0; i < Ny; ++i) Yc[t + (size_t)i * T] = Y[((size_t)c * T + t) * Ny + i];
      ch.set_T(c, T);
      ch.upload_X(c, T, Xc.data());
      ch.upload_TN(ch.Ypool.p + (size_t)c * ch.d.N * ch.d.TP, 1, T, Yc.data(), 0.0);
      ch.set_slot_prior(c, ivd.data(), ivb.data(), sP.data(), h0m.data(), h0v.data());
      ch.have_slot[c] = true;
      sl[c] = c;
    }
    ch.set_slots(sl.data());
    std::vector<uint8_t> none(Ny, 0);
    ch.set_elb_model(nd.data(), none.data());
    for (int c = 0; c < B; ++c) ch.set_elb_slot(c, 0, sNaN);
    // state: PAI = C(2:Ny+1, :)' (elb.A rows, :404-407), A = Psi(2:Ny+1, :) \ I, sqrtht = SVol'
    std::vector<double> PAI((size_t)K * Ny * B), A((size_t)Ny * Ny * B, 0.0), sh((size_t)T * Ny * B),
        hh((size_t)T * Ny * B), sq((size_t)Ny * Ny * B, 0.0);
    // (host_struct_inverse: the triangular branch only when every impact matrix is lower triangular)
    const int nPsi = psi3d ? T : 1;
    bool lower = true;
    for (int c = 0; c < B && lower; ++c)
      for (int m = 0; m < nPsi && lower; ++m) {
        const double* Pc = Psi + ((size_t)c * nPsi + m) * K * Ny;
        for (int col = 1; col < Ny && lower; ++col)
          for (int r = 0; r < col; ++r)
            if (Pc[(1 + r) + (size_t)col * K] != 0.0) {
              lower = false;
              break;
            }
      }
    bool singular = false;
    std::vector<double> Am(psi3d ? (size_t)B * T * Ny * Ny : 0, 0.0);
    for (int c = 0; c < B; ++c) {
      const double* Cc = C + (size_t)c * KK;
      const double* Pc = Psi + (size_t)c * nPsi * K * Ny;
      for (int i = 0; i < Ny; ++i)
        for (int k = 0; k < K; ++k) PAI[((size_t)c * Ny + i) * K + k] = Cc[(1 + i) + (size_t)k * K];
      double* Ac = A.data() + (size_t)c * Ny * Ny;
      singular |= !host_struct_inverse(Pc, K, Ny, lower, Ac);
      for (int m = 0; m < (psi3d ? T : 0); ++m)
        singular |= !host_struct_inverse(Pc + (size_t)m * K * Ny, K, Ny, lower,
                                         Am.data() + ((size_t)c * T + m) * Ny * Ny);
      for (int i = 0; i < Ny; ++i) {
        sq[(size_t)c * Ny * Ny + i + (size_t)i * Ny] = 1.0;
        for (int t = 0; t < T; ++t) {
          const double v = SVol[((size_t)c * T + t) * Ny + i];
          sh[((size_t)c * Ny + i) * T + t] = v;
          hh[((size_t)c * Ny + i) * T + t] = 2.0 * std::log(v);
        }
      }
    }
    if (singular) {
      set_last_error(std::string(b3 ? "ccmm_gibbs_shadowrates_b3: B" : "ccmm_gibbs_shadowrates: Psi") +
                     "(2:Ny+1, :) is singular");
      return CCMM_ERR_ARG;
    }
    ch.elb_Afull = lower ? 0 : 1;
    ch.upload_KN(ch.PAI.p, B, PAI.data(), 0.0);
    HIPCHECK(hipMemcpy(ch.A.p, A.data(), A.size() * sizeof(double), hipMemcpyHostToDevice));
    ch.upload_TN(ch.sqrtht.p, B, T, sh.data(), 1.0);
    ch.upload_TN(ch.h.p, B, T, hh.data(), 0.0);
    HIPCHECK(hipMemcpy(ch.sqrtPHI.p, sq.data(), sq.size() * sizeof(double), hipMemcpyHostToDevice));
    ch.have_elb_model = true;
    ch.reset_chain_slabs();
    // YHAT0 (Ny x elbT per chain, or zeros) -> [B][elbT][Ny]
    DBuf<double> dyh;
    dyh.alloc((size_t)B * T * Ny);
    {
      std::vector<double> yh((size_t)B * T * Ny, 0.0);
      if (YHAT0) std::memcpy(yh.data(), YHAT0, yh.size() * sizeof(double));
      HIPCHECK(hipMemcpy(dyh.p, yh.data(), yh.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    ch.elb_yhat = dyh.p;
    ch.elb_b3 = b3;
    DBuf<double> dAm;
    if (psi3d) {
      dAm.alloc(Am.size());
      HIPCHECK(hipMemcpy(dAm.p, Am.data(), Am.size() * sizeof(double), hipMemcpyHostToDevice));
      ch.elb_Amon = dAm.p;
    }
    DBuf<uint8_t> dfl;
    if (flags) {
      dfl.alloc((size_t)B * passes * T * Ns);
      HIPCHECK(hipMemset(dfl.p, 0, dfl.n));
      ch.elb_flags = dfl.p;
    }
    DBuf<double> du;
    RngArgs ra = ch.rng_args(nullptr, 0);
    if (u) {  // rand(Ns, elbT, burnin + Ndraws) per chain (gibbsdrawShadowrates.m:173)
      du.alloc((size_t)B * Ns * T * passes);
      HIPCHECK(hipMemcpy(du.p, u, du.n * sizeof(double), hipMemcpyHostToDevice));
      ra = ch.rng_args(du.p, (int64_t)Ns * T * passes);
      ra.off[CCMM_RNG_ELB] = 0;
    }
    ch.run_elb(ra, false);
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(out, ch.eScur.p, (size_t)B * Ns * T * sizeof(double), hipMemcpyDeviceToHost));
    if (flags) HIPCHECK(hipMemcpy(flags, dfl.p, dfl.n, hipMemcpyDeviceToHost));
    return 0;
  });
}

int ccmm_gibbs_shadowrates(ccmm_ctx* ctx, int B, int Ny, int elbT, int Ns, int p, const uint8_t* ndxS,
                           const uint8_t* sNaN, const double* Y, const double* STATE0,
                           const double* YHAT0, const double* C, const double* Psi, const double* SVol,
                           double elbBound, int Ndraws, int burnin, const double* u, double* out,
                           uint8_t* flags) {
  return gibbs_shadowrates_impl(ctx, B, Ny, elbT, Ns, p, ndxS, sNaN, Y, STATE0, YHAT0, C, Psi, SVol, elbBound,
                                Ndraws, burnin, u, out, flags, 0, 0);
}

int ccmm_gibbs_shadowrates_b3(ccmm_ctx* ctx, int B, int Ny, int elbT, int Ns, int p, const uint8_t* ndxS,
                              const uint8_t* sNaN, const double* Y, const double* STATE0, const double* A,
                              const double* Bmat, int B3d, const double* SVol, double elbBound, int Ndraws,
                              int burnin, const double* u, double* out, uint8_t* flags) {
  return gibbs_shadowrates_impl(ctx, B, Ny, elbT, Ns, p, ndxS, sNaN, Y, STATE0, nullptr, A, Bmat, SVol,
                                elbBound, Ndraws, burnin, u, out, flags, 1, B3d ? 1 : 0);
}

// bh: 0 linear, 1 block hybrid (ring = ndxYields, actual = actualrateBlock), 2 hybrid (ring =
// ring_vars = ndxSHADOWRATE, PAI (K + Ns p) x N x M); the output floor is ndxYields in both
static int girf_impl(ccmm_ctx* ctx, int M, int N, int p, int H, int nsim, const double* PAI, const double* invA,
                     const double* sqrtPHI, const double* SV0, const double* Xjumpoff, int bh, const uint8_t* actual,
                     const uint8_t* ring_vars, const uint8_t* ndxYields, double elb, const uint8_t* cumcode,
                     double np_, double shock11, const double* z, const double* svz, uint64_t seed, double* yhat) {
  return guarded([&] {
    require(ctx && PAI && invA && sqrtPHI && SV0 && Xjumpoff && yhat, "null argument");
    require(M >= 1 && N >= 1 && N <= 32 && p >= 1 && H >= 1 && nsim >= 1, "bad dimensions (N <= 32)");
    require(bh != 1 || (actual && ndxYields), "block hybrid needs actual and ndxYields");
    require(bh != 2 || (ring_vars && ndxYields), "hybrid needs ndxShadow and ndxYields");
    require((z == nullptr) == (svz == nullptr), "z and svz: both or neither");
    HIPCHECK(hipSetDevice(ctx->device));
    const int K = N * p + 1;
    std::vector<int> yi;
    if (bh)
      for (int i = 0; i < N; ++i)
        if (ring_vars[i]) yi.push_back(i);
    const int Ny = (int)yi.size();
    require(bh == 0 || Ny >= 1, "no ring variables");
    const int ldX = K + Ny * p;
    const int ldP = (bh == 2) ? ldX : K;
    const GirfPlan plan = girf_plan(N, p, Ny, ctx->opt[OPT_GIRF_GENERIC] != 0);
    require(plan.nks <= kGirfMaxKs, "state too large for the GIRF kernel (K + Ny p + N <= 384)");
    // (the table-driven kernel keeps p rows of the state's row table beside the state: many lags of few variables)
    require(plan.lds <= kLdsCu, "the GIRF state and its row table do not fit LDS (p (K + Ny p + N) ints + the state)");
    const size_t nch = (size_t)(nsim + 3) / 4;
    DBuf<double> dPAI, dA, dS, dSV, dX, dZ, dSZ, dPart, dOut;
    DBuf<uint8_t> dAct, dCum, dFl;
    DBuf<int> dY;
    auto up = [&](auto& buf, const auto* src, size_t n) {
      buf.alloc(n);
      HIPCHECK(hipMemcpy(buf.p, src, n * sizeof(src[0]), hipMemcpyHostToDevice));
    };
    // PAI ldP x N x M column-major == [M][N][ldP]
    up(dPAI, PAI, (size_t)ldP * N * M);
    up(dA, invA, (size_t)N * N * M);
    up(dS, sqrtPHI, (size_t)N * N * M);
    up(dSV, SV0, (size_t)N * M);
    up(dX, Xjumpoff, (size_t)ldX * M);
    if (z) {
      up(dZ, z, (size_t)N * H * nsim * M);
      up(dSZ, svz, (size_t)N * H * nsim * M);
    }
    if (bh == 1) up(dAct, actual, (size_t)N);
    if (bh) {
      up(dY, yi.data(), yi.size());
      up(dFl, ndxYields, (size_t)N);
    }
    if (cumcode) up(dCum, cumcode, (size_t)N);
    dPart.alloc((size_t)M * 3 * nch * H * N);
    dOut.alloc((size_t)M * 3 * H * N);
    GirfArgs a{};
    a.M = M; a.N = N; a.p = p; a.H = H; a.nsim = nsim; a.bh = bh; a.Ny = Ny;
    a.PAI = dPAI.p; a.invA = dA.p; a.sqrtPHI = dS.p; a.SV0 = dSV.p; a.Xj = dX.p; a.ldX = ldX;
    a.actual = bh == 1 ? dAct.p : nullptr; a.yidx = bh ? dY.p : nullptr; a.yfloor = bh ? dFl.p : nullptr;
    a.elb = elb; a.shock11 = shock11;
    a.z = z ? dZ.p : nullptr; a.svz = z ? dSZ.p : nullptr; a.seed = seed;
    a.cumcode = cumcode ? dCum.p : nullptr; a.np_ = np_; a.part = dPart.p; a.out = dOut.p;
    a.force_generic = ctx->opt[OPT_GIRF_GENERIC];  // A/B of the specialised kernel
    HIPCHECK(girf_launch(ctx->stream, a));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(yhat, dOut.p, dOut.n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  });
}

int ccmm_girf(ccmm_ctx* ctx, int M, int N, int p, int H, int nsim, const double* PAI, const double* invA,
              const double* sqrtPHI, const double* SV0, const double* Xjumpoff, int bh, const uint8_t* actual,
              const uint8_t* ndxYields, double elb, const uint8_t* cumcode, double np_, double shock11,
              const double* z, const double* svz, uint64_t seed, double* yhat) {
  return girf_impl(ctx, M, N, p, H, nsim, PAI, invA, sqrtPHI, SV0, Xjumpoff, bh ? 1 : 0, actual, ndxYields,
                   ndxYields, elb, cumcode, np_, shock11, z, svz, seed, yhat);
}

int ccmm_girf_hybrid(ccmm_ctx* ctx, int M, int N, int p, int H, int nsim, const double* PAI, const double* invA,
                     const double* sqrtPHI, const double* SV0, const double* Xjumpoff, const uint8_t* ndxShadow,
                     const uint8_t* ndxYields, double elb, const uint8_t* cumcode, double np_, double shock11,
                     const double* z, const double* svz, uint64_t seed, double* yhat) {
  return girf_impl(ctx, M, N, p, H, nsim, PAI, invA, sqrtPHI, SV0, Xjumpoff, 2, nullptr, ndxShadow, ndxYields,
                   elb, cumcode, np_, shock11, z, svz, seed, yhat);
}

}  // extern "C"

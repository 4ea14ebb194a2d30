// The predictive density of a chain set's kept sweeps (ccmm_chains.h) and the summaries over kept draws, then
// their entry points and the ccmm_fcst drop-in.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ccmm_chains.h"
#include "ccmm_fcst_big.h"
#include "ccmm_post.h"

using namespace ccmm;

void ccmm_chains::set_fcst(int H, int Nd, const uint8_t* ndxYields, int keep) {
  const int N = cfg.N, p = cfg.p;
  require(cfg.p >= 1 && (cfg.K == N * p + 1 || (hybrid && cfg.K == N * p + 1 + cfg.Ns * p)),
          "predictive density needs K = N*p + 1 (hybrid: + Ns*p)");
  require(!hybrid || cfg.Ns <= kElbNsMax, "hybrid predictive density: Ns <= 5");
  // N > 32: the large-N unit (ccmm_fcst_big.hip), which serves the linear and block-hybrid forms
  require(!hybrid || N <= kFcstMaxN, "hybrid predictive density supports N <= 32");
  require(N <= kFcstBigMaxN, "predictive density supports N <= 128");
  require(H >= 1 && Nd >= 1, "H and Nd must be >= 1");
  require(cfg.store_capacity > 0, "predictive density needs store_capacity > 0 (one record per kept draw)");
  int nwx = 0;
  for (int i = 0; i < N; ++i) nwx += ndxYields[i] ? 0 : 1;
  require(nwx > 0 && nwx < N, "need at least one macro series and one yield");
  require(N > kFcstMaxN ? fcst_big_plan(N, p, H, Nd, fcst_bh ? 1 : 0).ok
                        : fcst_paths_lds_doubles(N, cfg.K, p, fcst_chunk(N, cfg.K, p, H)) * sizeof(double) <= kLdsCu,
          "forecast state does not fit LDS");
  if (bh && !hybrid)
    for (int i = 0; i < N; ++i)
      require(!(hActual[i] && ndxYields[i]), "a yield cannot be in the actual-rate block");
  if (hybrid)
    for (int a = 0; a < cfg.Ns; ++a)
      require(ndxYields[hNdxS[a]], "the shadow-rate variables must be yields (ndxYIELDS)");
  fH = H;
  fNd = Nd;
  fKeep = keep ? 1 : 0;
  fldXj = cfg.K + N * p;
  const size_t B = cfg.B, HN = (size_t)H * N, cap = cfg.store_capacity;
  fYields.alloc(N);
  HIPCHECK(hipMemcpy(fYields.p, ndxYields, N, hipMemcpyHostToDevice));
  fYreal.alloc((size_t)cfg.ndata * N);
  std::vector<double> nan((size_t)cfg.ndata * N, std::nan(""));
  HIPCHECK(hipMemcpy(fYreal.p, nan.data(), nan.size() * sizeof(double), hipMemcpyHostToDevice));
  have_fcst_slot.assign(cfg.ndata, false);
  fXj.alloc(B * fldXj);
  fY.alloc(B * Nd * HN);
  fYc.alloc(B * Nd * HN);
  fYhat.alloc(B * HN);
  fSc.alloc(B * Nd * 4);
  fStatus.alloc(B);
  fYsum.alloc(B * HN);
  fYcsum.alloc(B * HN);
  fYhatsum.alloc(B * HN);
  fScStore.alloc(B * cap * Nd * 4);
  if (fKeep) {
    fPaths.alloc(B * cap * Nd * HN);
    fPathsC.alloc(B * cap * Nd * HN);
  }
  fSv1.alloc(B * Nd * N);
  have_fcst = true;
  have_irf = false;  // (its buffers follow H, Nd and keep_paths: ccmm_chains_set_irf1 comes after this call)
  reset_fcst();
  layout_crn();
}

void ccmm_chains::set_irf1(double scale, const uint8_t* cumcode) {
  const int N = cfg.N, p = cfg.p, bhf = hybrid ? 2 : (fcst_bh ? 1 : 0);
  require(N <= kFcstMaxN, "doIRF1 supports N <= 32");
  // (the LDS form's plan, as set_fcst: no register-path shape is larger)
  require(fcst_irf_lds_doubles(N, cfg.K, p, fcst_irf_chunk(N, cfg.K, p, fH, false, bhf), false, bhf) * sizeof(double) <=
              kLdsCu,
          "forecast state does not fit LDS");
  const size_t B = cfg.B, HN = (size_t)fH * N, cap = cfg.store_capacity;
  std::vector<uint8_t> cc(N, 0);
  if (cumcode)
    for (int i = 0; i < N; ++i) cc[i] = cumcode[i] ? 1 : 0;
  fIrfCum.alloc(N);
  HIPCHECK(hipMemcpy(fIrfCum.p, cc.data(), N, hipMemcpyHostToDevice));
  fY1p.alloc(B * fNd * HN);
  fY1m.alloc(B * fNd * HN);
  fIrfP.alloc(B * cap * HN);
  fIrfM.alloc(B * cap * HN);
  fY1sumP.alloc(B * HN);
  fY1sumM.alloc(B * HN);
  fIrfTmp.alloc(B * 2 * HN);
  if (fKeep) {
    fPathsP.alloc(B * cap * fNd * HN);
    fPathsM.alloc(B * cap * fNd * HN);
  }
  irfScale = scale;
  have_irf = true;
  reset_fcst();
}
void ccmm_chains::reset_fcst() {
  const size_t HN = (size_t)fH * cfg.N, B = cfg.B;
  HIPCHECK(hipMemsetAsync(fYsum.p, 0, B * HN * sizeof(double), ctx->stream));
  HIPCHECK(hipMemsetAsync(fYcsum.p, 0, B * HN * sizeof(double), ctx->stream));
  HIPCHECK(hipMemsetAsync(fYhatsum.p, 0, B * HN * sizeof(double), ctx->stream));
  HIPCHECK(hipMemsetAsync(fStatus.p, 0, B * sizeof(int), ctx->stream));
  if (have_irf) {
    HIPCHECK(hipMemsetAsync(fY1sumP.p, 0, B * HN * sizeof(double), ctx->stream));
    HIPCHECK(hipMemsetAsync(fY1sumM.p, 0, B * HN * sizeof(double), ctx->stream));
  }
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  fstored = 0;
}

void ccmm_chains::join_fcst() {
  if (!fcst_pending) return;
  HIPCHECK(hipStreamWaitEvent(ctx->stream, fcstEv.join, 0));
  fcst_pending = false;
}

void ccmm_chains::run_fcst(const RngArgs& ra) {
  if (fstored >= cfg.store_capacity) throw ArgError("forecast store full: call ccmm_chains_get_fcst");
  hipStream_t fst = ctx->stream;
  // (small B only: with the chip full of the next sweep's Gram + Cholesky the overlap buys nothing)
  const bool overlap = opt[OPT_FCST_OVERLAP] != 0 && d.N <= kMaxNSmall && d.B <= kElbMpMaxB;
  if (overlap) {
    ensure_aux();
    fcstEv.ensure();
    HIPCHECK(hipEventRecord(fcstEv.fork, ctx->stream));
    HIPCHECK(hipStreamWaitEvent(aux, fcstEv.fork, 0));
    fst = aux;
  }
  const int N = d.N, B = d.B, H = fH, Nd = fNd;
  FcstArgs a{};
  a.B = B; a.N = N; a.p = cfg.p; a.H = H; a.Nd = Nd;
  a.bh = hybrid ? 2 : (fcst_bh ? 1 : 0);
  a.K = N * cfg.p + 1;
  a.Kx = cfg.K;
  a.Ns = hybrid ? cfg.Ns : 0;
  a.ndxS = hybrid ? dNdxS.p : nullptr;
  a.PAI = PAI.p; a.ldPAI = d.KP; a.invA = invA.p; a.logSV = h.p; a.ldSV = d.TP;
  a.svT = Tslot.p; a.slot = slot.p; a.sqrtPHI = sqrtPHI.p; a.Xj = fXj.p; a.ldXj = fldXj;
  a.yreal = fYreal.p; a.ldY = N; a.ndxYields = fYields.p; a.actual = fcst_bh ? dActual.p : nullptr;
  a.recFloor = have_rec_floor ? fRecFloor.p : nullptr;
  a.elb = cfg.elb;
  if (ra.crn) {
    a.svz = ra.crn + ra.off[CCMM_RNG_FCST];
    a.z = a.svz + (size_t)N * H * Nd;
    a.crnStride = ra.crn_chain_stride;
  }
  a.seed = cfg.seed; a.sweep = ra.sweep; a.ids = ra.ids;
  a.fY = fY.p; a.fYc = fYc.p; a.yhat = fYhat.p; a.scores = fSc.p; a.status = fStatus.p;
  if (have_irf) {
    a.irfScale = irfScale;
    a.fY1p = fY1p.p;
    a.fY1m = fY1m.p;
  }
  a.gl = gl_nodes();
  a.mode = env_ablation("CCMM_FCST_MODE", 0);  // timing-only (kFcstNoScores, kFcstNoHorizons)
  const XSel xs = xsel();
  launch(KID_FCST, [&] {
    HIPCHECK(launch_fcst_jumpoff(fst, a, d.TP, Tslot.p, xs.ypool, xs.yidx, fXj.p));
    if (N > kFcstMaxN)
      HIPCHECK(launch_fcst_big(fst, a, fSv1.p));
    else
      HIPCHECK(launch_fcst(fst, a, fSv1.p, opt[OPT_FCST_REG] != 0));
    HIPCHECK(launch_fcst_accum(fst, a, cfg.store_capacity, fstored, (fcst_bh || hybrid) ? nullptr : fYhat.p, fYsum.p,
                               fYcsum.p, fYhatsum.p, fScStore.p, fKeep ? fPaths.p : nullptr, fKeep ? fPathsC.p : nullptr));
    if (have_irf)
      HIPCHECK(launch_fcst_irf_accum(fst, a, cfg.store_capacity, fstored, fIrfCum.p, fIrfP.p, fIrfM.p, fY1sumP.p,
                                     fY1sumM.p, fIrfTmp.p, fKeep ? fPathsP.p : nullptr, fKeep ? fPathsM.p : nullptr));
  }, fst);
  ++fstored;
  if (overlap) {
    HIPCHECK(hipEventRecord(fcstEv.join, aux));
    fcst_pending = true;
  }
}

// ---------------------------------------------------------------- post-processing
// The common tail of the summaries: S series of n draws in A (device; B and ws: scratch of post_workspace_bytes),
// the statistics the caller asked for back on the host
static void summarise(hipStream_t st, int S, int n, double* A, double* B, DBuf<char>& ws, DBuf<double>& out,
                      const double* realized, int nq, const double* pct, double* mean, double* median, double* quant,
                      double* sdev, double* crps, bool nans = false) {
  const size_t wb = post_workspace_bytes(S, n);
  ws.alloc(wb);
  // device scratch: pct | realized | mean | median | sd | crps | quantiles
  out.alloc((size_t)nq + (size_t)S * (5 + nq));
  double* dp = out.p;
  double* dr = dp + nq;
  double* dm = dr + S;
  double* dmed = dm + S;
  double* dsd = dmed + S;
  double* dcr = dsd + S;
  double* dq = dcr + S;
  if (nq) HIPCHECK(hipMemcpy(dp, pct, nq * sizeof(double), hipMemcpyHostToDevice));
  if (realized) HIPCHECK(hipMemcpy(dr, realized, S * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(post_summaries(st, S, n, A, B, ws.p, wb, realized ? dr : nullptr, nq, dp,
                          dm, dmed, nq ? dq : nullptr, dsd, crps ? dcr : nullptr, nans));
  HIPCHECK(hipStreamSynchronize(st));
  auto get = [&](double* dst, const double* src, size_t cnt) {
    if (dst) HIPCHECK(hipMemcpy(dst, src, cnt * sizeof(double), hipMemcpyDeviceToHost));
  };
  get(mean, dm, S);
  get(median, dmed, S);
  get(sdev, dsd, S);
  get(crps, dcr, S);
  get(quant, dq, (size_t)S * nq);
}

void ccmm_chains::summaries(int source, int sl, const uint8_t* rows, const uint8_t* cumcode, const uint8_t* flo,
                            double fl, const double* realized, int nq, const double* pct, double* mean,
                            double* median, double* quant, double* sdev, double* crps) {
  require(sl >= 0 && sl < cfg.ndata, "slot out of range");
  require(nq >= 0 && (nq == 0 || pct), "bad quantile list");
  std::vector<int> hs(cfg.B);
  HIPCHECK(hipMemcpy(hs.data(), slot.p, cfg.B * sizeof(int), hipMemcpyDeviceToHost));
  int c0 = -1, C = 0;
  for (int c = 0; c < cfg.B; ++c)
    if (hs[c] == sl) {
      if (c0 < 0) c0 = c;
      require(c == c0 + C, "the chains of the slot must be contiguous");
      ++C;
    }
  require(C > 0, "no chain bound to the slot");
  const int N = cfg.N, K = cfg.K;
  int S = 0, n = 0;
  if (source == 0 || source == 1) {
    require(have_fcst && fKeep, "forecast paths were not kept (ccmm_chains_set_fcst keep_paths)");
    require(fstored > 0, "no forecast records");
    std::vector<int> rl;
    for (int i = 0; i < N; ++i)
      if (!rows || rows[i]) rl.push_back(i);
    require(!rl.empty(), "no rows selected");
    S = (int)rl.size() * fH;
    n = C * fstored * fNd;
    postRows.alloc(rl.size());
    HIPCHECK(hipMemcpy(postRows.p, rl.data(), rl.size() * sizeof(int), hipMemcpyHostToDevice));
    if (cumcode) {
      postCum.alloc(N);
      HIPCHECK(hipMemcpy(postCum.p, cumcode, N, hipMemcpyHostToDevice));
    }
    if (flo) {
      postFlo.alloc(N);
      HIPCHECK(hipMemcpy(postFlo.p, flo, N, hipMemcpyHostToDevice));
    }
    postA.alloc((size_t)S * n);
    HIPCHECK(post_gather_fcst(ctx->stream, source == 0 ? fPaths.p : fPathsC.p, c0, C, fstored, fNd, fH, N,
                              cfg.store_capacity, postRows.p, (int)rl.size(), cumcode ? postCum.p : nullptr,
                              flo ? postFlo.p : nullptr, fl, postA.p));
  } else if (source == 2) {
    require(stored > 0 && sPAI.p, "no stored draws");
    require(!flo, "a floor applies to forecast paths only");
    S = K * N;
    n = C * stored;
    postA.alloc((size_t)S * n);
    HIPCHECK(post_gather_pai(ctx->stream, sPAI.p, c0, C, stored, cfg.store_capacity, K * N, postA.p));
  } else if (source >= 3 && source <= 5) {
    // the other draw stores, [chain][capacity][entry] as sPAI: 3 sqrtht (Tmax x N, t fastest), 4 shadowrate_all and
    // 5 missingrate_all (Ns x elbTmax, rate fastest).  Their draws may be NaN (shadowrate_all under the missing-data
    // treatment, missingrate_all of a sweep without a PS proposal): the NaN rules of post_summaries
    require(!rows && !cumcode && !flo && !realized && !crps,
            "sources 3 to 5 take no rows, cumcode, floor, realized values or crps");
    require(stored > 0 && sPAI.p, "no stored draws");
    const double* src = sSqrtht.p;
    S = cfg.T * N;
    if (source != 3) {
      require(bh && cfg.elbTmax > 0 && sShadow.p, "no stored shadow rates");
      require(have_elb_slot[sl], "ccmm_chains_set_elb_slot was not called for the slot");
      require(source == 4 || (keep_first && sMissing.p), "source 5: missing rates were not kept");
      src = source == 4 ? sShadow.p : sMissing.p;
      S = cfg.Ns * cfg.elbTmax;
    }
    require(src != nullptr && S > 0, "no stored draws of the source");
    n = C * stored;
    postA.alloc((size_t)S * n);
    HIPCHECK(post_gather_pai(ctx->stream, src, c0, C, stored, cfg.store_capacity, S, postA.p));
    postB.alloc((size_t)S * n);
    summarise(ctx->stream, S, n, postA.p, postB.p, postWs, postOut, nullptr, nq, pct, mean, median, quant, sdev, nullptr,
              true);
    // the series that hold no draw (t >= T of the slot; months at or beyond its elbT): NaN in every statistic
    const double nan = std::nan("");
    for (int e = 0; e < S; ++e) {
      const bool live = source == 3 ? e % cfg.T < hT[sl] : e / cfg.Ns < hElbT[sl];
      if (live) continue;
      for (double* o : {mean, median, sdev})
        if (o) o[e] = nan;
      if (quant)
        for (int q = 0; q < nq; ++q) quant[(size_t)q * S + e] = nan;
    }
    return;
  } else {
    throw ArgError("source must be 0 (paths), 1 (censored paths), 2 (PAI draws), 3 (sqrtht), 4 (shadowrate_all) or "
                   "5 (missingrate_all)");
  }
  postB.alloc((size_t)S * n);
  summarise(ctx->stream, S, n, postA.p, postB.p, postWs, postOut, realized, nq, pct, mean, median, quant, sdev,
            crps);
}

extern "C" {

int ccmm_chains_set_fcst(ccmm_chains* ch, int H, int Nd, const uint8_t* ndxYields, int keep_paths) {
  return guarded([&] {
    require(ch && ndxYields, "null argument");
    require(!ch->bh || ch->have_elb_model, "ccmm_chains_set_elb_model must be called before set_fcst");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    ch->set_fcst(H, Nd, ndxYields, keep_paths);
    return 0;
  });
}

int ccmm_chains_set_fcst_slot(ccmm_chains* ch, int slot, const double* yrealized) {
  return guarded([&] {
    require(ch && yrealized, "null argument");
    require(ch->have_fcst, "ccmm_chains_set_fcst must be called first");
    require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    HIPCHECK(hipMemcpy(ch->fYreal.p + (size_t)slot * ch->cfg.N, yrealized, ch->cfg.N * sizeof(double),
                       hipMemcpyHostToDevice));
    ch->have_fcst_slot[slot] = true;
    return 0;
  });
}

int ccmm_chains_set_fcst_censor(ccmm_chains* ch, const uint8_t* floor_in_recursion) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->have_fcst, "ccmm_chains_set_fcst must be called first");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    if (!floor_in_recursion) {
      ch->have_rec_floor = false;
      return 0;
    }
    ch->fRecFloor.alloc(ch->cfg.N);
    HIPCHECK(hipMemcpy(ch->fRecFloor.p, floor_in_recursion, ch->cfg.N, hipMemcpyHostToDevice));
    ch->have_rec_floor = true;
    return 0;
  });
}

int ccmm_chains_set_irf1(ccmm_chains* ch, double scale, const uint8_t* cumcode) {
  if (ch && !ch->have_fcst) {
    set_last_error("ccmm_chains_set_fcst must be called before set_irf1");
    return CCMM_ERR_STATE;
  }
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(std::isfinite(scale), "IRF1scale must be finite");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    ch->set_irf1(scale, cumcode);
    return 0;
  });
}

int ccmm_chains_get_irf1(ccmm_chains* ch, double* drawsPlus, double* drawsMinus, double* y1sumPlus,
                         double* y1sumMinus, double* pathsPlus, double* pathsMinus) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->have_fcst && ch->have_irf, "ccmm_chains_set_irf1 was not called");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const size_t B = ch->cfg.B, Nd = ch->fNd, cap = ch->cfg.store_capacity, M = ch->fstored;
    const size_t HN = (size_t)ch->fH * ch->cfg.N;
    // device [c][m][..] with cap records per chain -> M records per chain, the device order inside a record
    auto fetch = [&](const DBuf<double>& src, double* dst, size_t rec) {
      if (!dst || !M) return;
      for (size_t c = 0; c < B; ++c)
        HIPCHECK(hipMemcpy(dst + c * M * rec, src.p + c * cap * rec, M * rec * sizeof(double), hipMemcpyDeviceToHost));
    };
    fetch(ch->fIrfP, drawsPlus, HN);
    fetch(ch->fIrfM, drawsMinus, HN);
    if (y1sumPlus) HIPCHECK(hipMemcpy(y1sumPlus, ch->fY1sumP.p, B * HN * sizeof(double), hipMemcpyDeviceToHost));
    if (y1sumMinus) HIPCHECK(hipMemcpy(y1sumMinus, ch->fY1sumM.p, B * HN * sizeof(double), hipMemcpyDeviceToHost));
    if ((pathsPlus || pathsMinus) && M) require(ch->fKeep != 0, "paths were not kept (keep_paths = 0)");
    fetch(ch->fPathsP, pathsPlus, Nd * HN);
    fetch(ch->fPathsM, pathsMinus, Nd * HN);
    return 0;
  });
}

int ccmm_chains_fcst_stored(const ccmm_chains* ch) { return ch && ch->have_fcst ? ch->fstored : -1; }

int ccmm_chains_get_fcst(ccmm_chains* ch, double* scores, double* fYsum, double* fYcsum,
                         double* yhatsum, double* paths, double* paths_censored) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->have_fcst, "ccmm_chains_set_fcst was not called");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const size_t B = ch->cfg.B, N = ch->cfg.N, H = ch->fH, Nd = ch->fNd;
    const size_t cap = ch->cfg.store_capacity, M = ch->fstored, HN = H * N;
    if (scores && M) {
      std::vector<double> buf(B * cap * Nd * 4);
      HIPCHECK(hipMemcpy(buf.data(), ch->fScStore.p, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
      // device [c][m][job][k] -> Nd x M x 4 x B
      for (size_t c = 0; c < B; ++c)
        for (size_t m = 0; m < M; ++m)
          for (size_t job = 0; job < Nd; ++job)
            for (size_t k = 0; k < 4; ++k)
              scores[job + Nd * (m + M * (k + 4 * c))] = buf[((c * cap + m) * Nd + job) * 4 + k];
    }
    auto sums = [&](const DBuf<double>& src, double* dst) {
      if (dst) HIPCHECK(hipMemcpy(dst, src.p, B * HN * sizeof(double), hipMemcpyDeviceToHost));
    };
    sums(ch->fYsum, fYsum);
    sums(ch->fYcsum, fYcsum);
    sums(ch->fYhatsum, yhatsum);
    auto fetch_paths = [&](const DBuf<double>& src, double* dst) {
      if (!dst || !M) return;
      require(ch->fKeep != 0, "paths were not kept (keep_paths = 0)");
      const size_t per = M * Nd * HN;  // N x H x Nd x M per chain: the device order
      for (size_t c = 0; c < B; ++c)
        HIPCHECK(hipMemcpy(dst + c * per, src.p + c * cap * Nd * HN, per * sizeof(double),
                           hipMemcpyDeviceToHost));
    };
    fetch_paths(ch->fPaths, paths);
    fetch_paths(ch->fPathsC, paths_censored);
    std::vector<int> st(B);
    HIPCHECK(hipMemcpy(st.data(), ch->fStatus.p, B * sizeof(int), hipMemcpyDeviceToHost));
    int rc = 0;
    for (int v : st)
      if (v & 2) rc = CCMM_WARN_MVNCDF;
    if (rc) set_last_error("censored log score with >= 4 series at the ELB (mvncdf) is NaN");
    ch->reset_fcst();
    return rc;
  });
}

int ccmm_draw_summaries(ccmm_ctx* ctx, int S, int n, const double* draws, const double* realized, int nq,
                        const double* pct, double* mean, double* median, double* quantiles, double* stdev,
                        double* crps) {
  return guarded([&] {
    require(ctx && draws, "null argument");
    require(S >= 1 && n >= 1, "S and n must be positive");  // sorted in batches of < 2^31 items
    require(nq >= 0 && (nq == 0 || pct), "bad quantile list");
    HIPCHECK(hipSetDevice(ctx->device));
    DBuf<double> A, Bs, out;
    DBuf<char> ws;
    A.alloc((size_t)S * n);
    Bs.alloc((size_t)S * n);
    HIPCHECK(hipMemcpy(A.p, draws, (size_t)S * n * sizeof(double), hipMemcpyHostToDevice));
    summarise(ctx->stream, S, n, A.p, Bs.p, ws, out, realized, nq, pct, mean, median, quantiles, stdev, crps);
    return 0;
  });
}

int ccmm_chains_summaries(ccmm_chains* ch, int source, int slot, const uint8_t* rows, const uint8_t* cumcode,
                          const double* realized, int nq, const double* pct, double* mean, double* median,
                          double* quantiles, double* stdev, double* crps) {
  return ccmm_chains_summaries_floor(ch, source, slot, rows, cumcode, nullptr, 0.0, realized, nq, pct, mean, median,
                                     quantiles, stdev, crps);
}

int ccmm_chains_summaries_floor(ccmm_chains* ch, int source, int slot, const uint8_t* rows, const uint8_t* cumcode,
                                const uint8_t* floor_rows, double floor, const double* realized, int nq,
                                const double* pct, double* mean, double* median, double* quantiles, double* stdev,
                                double* crps) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    ch->summaries(source, slot, rows, cumcode, floor_rows, floor, realized, nq, pct, mean, median, quantiles, stdev,
                  crps);
    return 0;
  });
}

// ccmm_fcst (irf = false), ccmm_fcst_irf1 and ccmm_fcst_big (big: the large-N unit at every N <= 128)
static int fcst_dropin(ccmm_ctx* ctx, int B, int N, int p, int H, int Nd, const double* PAI, const double* invA,
                       const double* logSV0, const double* sqrtPHI, const double* Xjumpoff, const double* yrealized,
                       const uint8_t* ndxYields, double elb, const double* svz, const double* z, uint64_t seed,
                       int sweep, double* fcstY, double* fcstYcensor, double* yhat, double* scores, int* status,
                       bool irf, double irf1scale, double* fcstY1plus, double* fcstY1minus, bool big = false) {
  return guarded([&] {
    require(!irf || (fcstY1plus && fcstY1minus), "null argument");
    require(!irf || std::isfinite(irf1scale), "IRF1scale must be finite");
    require(ctx && PAI && invA && logSV0 && sqrtPHI && Xjumpoff && yrealized && ndxYields &&
                fcstY && fcstYcensor && yhat && scores,
            "null argument");
    require(B > 0 && N > 0 && N <= (big ? kFcstBigMaxN : kFcstMaxN) && p > 0 && H > 0 && Nd > 0, "unsupported size");
    require(!big || (p <= kFcstBigMaxK / N && N * p + 1 <= kFcstBigMaxK), "unsupported size");
    require((svz == nullptr) == (z == nullptr), "svz and z must both be given or both NULL");
    const int K = N * p + 1;
    int nwx = 0;
    for (int i = 0; i < N; ++i) nwx += ndxYields[i] ? 0 : 1;
    require(nwx > 0 && nwx < N, "need at least one macro series and one yield");
    HIPCHECK(hipSetDevice(ctx->device));
    // (the LDS form's size even where the register path will run: it refuses no register-path shape, whose
    // largest, N = 21, p = 12 at hc = 1, is 253 * 21 + 2 * 441 + 2 * 252 + 63 = 6762 doubles, 53 KB)
    require(big ? fcst_big_plan(N, p, H, Nd, 0).ok
                : fcst_paths_lds_doubles(N, K, p, fcst_chunk(N, K, p, H)) * sizeof(double) <= kLdsCu,
            "forecast state does not fit LDS");
    require(!irf || fcst_irf_lds_doubles(N, K, p, fcst_irf_chunk(N, K, p, H, false, 0), false, 0) * sizeof(double) <= kLdsCu,
            "forecast state does not fit LDS");
    auto up = [&](DBuf<double>& d, const double* h, size_t n) {
      d.alloc(n);
      HIPCHECK(hipMemcpyAsync(d.p, h, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    };
    DBuf<double> dPAI, dinvA, dlog, dsq, dXj, dy, dsvz, dz, dfY, dfYc, dyhat, dsc, dsv1, dfYp, dfYm;
    DBuf<uint8_t> dmask;
    DBuf<int> dst;
    up(dPAI, PAI, (size_t)B * K * N);
    up(dinvA, invA, (size_t)B * N * N);
    up(dlog, logSV0, (size_t)B * N);
    up(dsq, sqrtPHI, (size_t)B * N * N);
    up(dXj, Xjumpoff, (size_t)B * K);
    up(dy, yrealized, (size_t)N);
    if (svz) {
      up(dsvz, svz, (size_t)B * N * H * Nd);
      up(dz, z, (size_t)B * N * H * Nd);
    }
    dmask.alloc(N);
    HIPCHECK(hipMemcpyAsync(dmask.p, ndxYields, N, hipMemcpyHostToDevice, ctx->stream));
    const size_t nout = (size_t)B * N * H * Nd;
    dfY.alloc(nout);
    dfYc.alloc(nout);
    dyhat.alloc((size_t)B * N * H);
    dsc.alloc((size_t)B * 4 * Nd);
    dst.alloc(B);
    HIPCHECK(hipMemsetAsync(dst.p, 0, B * sizeof(int), ctx->stream));
    FcstArgs a{};
    a.B = B; a.N = N; a.p = p; a.K = K; a.Kx = K; a.H = H; a.Nd = Nd; a.bh = 0;
    a.PAI = dPAI.p; a.ldPAI = K; a.invA = dinvA.p; a.logSV = dlog.p; a.ldSV = 1;
    a.svT = nullptr; a.slot = nullptr; a.sqrtPHI = dsq.p; a.Xj = dXj.p; a.ldXj = K;
    a.yreal = dy.p; a.ldY = 0; a.ndxYields = dmask.p; a.actual = nullptr; a.elb = elb;
    a.svz = svz ? dsvz.p : nullptr;
    a.z = svz ? dz.p : nullptr;
    a.crnStride = (int64_t)N * H * Nd;
    a.seed = seed; a.sweep = (uint32_t)sweep;
    a.fY = dfY.p; a.fYc = dfYc.p; a.yhat = dyhat.p; a.scores = dsc.p; a.status = dst.p;
    a.gl = gl_nodes();
    if (irf) {
      dfYp.alloc(nout);
      dfYm.alloc(nout);
      a.irfScale = irf1scale;
      a.fY1p = dfYp.p;
      a.fY1m = dfYm.p;
    }
    dsv1.alloc((size_t)B * Nd * N);
    if (big)
      HIPCHECK(launch_fcst_big(ctx->stream, a, dsv1.p));
    else
      HIPCHECK(launch_fcst(ctx->stream, a, dsv1.p, ctx->opt[OPT_FCST_REG] != 0));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(fcstY, dfY.p, nout * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(fcstYcensor, dfYc.p, nout * sizeof(double), hipMemcpyDeviceToHost));
    if (irf) {
      HIPCHECK(hipMemcpy(fcstY1plus, dfYp.p, nout * sizeof(double), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(fcstY1minus, dfYm.p, nout * sizeof(double), hipMemcpyDeviceToHost));
    }
    HIPCHECK(hipMemcpy(yhat, dyhat.p, (size_t)B * N * H * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(scores, dsc.p, (size_t)B * 4 * Nd * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> st(B);
    HIPCHECK(hipMemcpy(st.data(), dst.p, B * sizeof(int), hipMemcpyDeviceToHost));
    int rc = 0;
    for (int c = 0; c < B; ++c) {
      if (status) status[c] = st[c];
      if (st[c] & 2) rc = CCMM_WARN_MVNCDF;
    }
    if (rc) set_last_error("censored log score with >= 3 series at the ELB (mvncdf) is NaN");
    return rc;
  });
}

int ccmm_fcst(ccmm_ctx* ctx, int B, int N, int p, int H, int Nd, const double* PAI,
              const double* invA, const double* logSV0, const double* sqrtPHI,
              const double* Xjumpoff, const double* yrealized, const uint8_t* ndxYields,
              double elb, const double* svz, const double* z, uint64_t seed, int sweep,
              double* fcstY, double* fcstYcensor, double* yhat, double* scores, int* status) {
  return fcst_dropin(ctx, B, N, p, H, Nd, PAI, invA, logSV0, sqrtPHI, Xjumpoff, yrealized, ndxYields, elb, svz, z, seed,
                     sweep, fcstY, fcstYcensor, yhat, scores, status, false, 0.0, nullptr, nullptr);
}

int ccmm_fcst_big(ccmm_ctx* ctx, int B, int N, int p, int H, int Nd, const double* PAI,
                  const double* invA, const double* logSV0, const double* sqrtPHI,
                  const double* Xjumpoff, const double* yrealized, const uint8_t* ndxYields,
                  double elb, const double* svz, const double* z, uint64_t seed, int sweep,
                  double* fcstY, double* fcstYcensor, double* yhat, double* scores, int* status) {
  return fcst_dropin(ctx, B, N, p, H, Nd, PAI, invA, logSV0, sqrtPHI, Xjumpoff, yrealized, ndxYields, elb, svz, z, seed,
                     sweep, fcstY, fcstYcensor, yhat, scores, status, false, 0.0, nullptr, nullptr, true);
}

int ccmm_fcst_irf1(ccmm_ctx* ctx, int B, int N, int p, int H, int Nd, const double* PAI, const double* invA,
                   const double* logSV0, const double* sqrtPHI, const double* Xjumpoff, const double* yrealized,
                   const uint8_t* ndxYields, double elb, const double* svz, const double* z, uint64_t seed, int sweep,
                   double* fcstY, double* fcstYcensor, double* yhat, double* scores, int* status, double irf1scale,
                   double* fcstY1plus, double* fcstY1minus) {
  return fcst_dropin(ctx, B, N, p, H, Nd, PAI, invA, logSV0, sqrtPHI, Xjumpoff, yrealized, ndxYields, elb, svz, z, seed,
                     sweep, fcstY, fcstYcensor, yhat, scores, status, true, irf1scale, fcstY1plus, fcstY1minus);
}

}  // extern "C"

// Generalized impulse responses of the stored draws through the C ABI (ccmm_chains_girf, ccmm_chains_girf_inputs;
// generateGIRF2linear.m, generateGIRF2blockhybrid.m, generateGIRF2hybrid.m over the draws of doMCMC*.m).  The
// simulation is ccmm_girf.hip, the inputs, Rao-Blackwellised responses and series sets ccmm_girf_store.hip, the
// order statistics ccmm_post.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ccmm_chains.h"
#include "ccmm_girf.h"
#include "ccmm_girf_store.h"
#include "ccmm_post.h"

using namespace ccmm;

namespace {

// what one date needs of the chain set, checked before any allocation
struct GirfSetup {
  int c0 = 0, C = 0, n = 0;  // the slot's chains and its pooled draws
  int bh = 0, Ny = 0, ldX = 0, npatch = 0;
  std::vector<int> yi;           // ring variables, ascending
  std::vector<uint8_t> actual;   // block hybrid: the variables that are no yields
};

GirfSetup girf_setup(ccmm_chains* ch, int slot, int t0, const double* jump, const uint8_t* ndxYields, int H,
                     int nsim) {
  require(ch && jump, "null argument");
  require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
  const int N = ch->d.N, p = ch->cfg.p, model = ch->cfg.model;
  require(N <= 32, "the GIRF kernels serve N <= 32");
  require(p >= 1, "p must be >= 1");
  require(model != CCMM_MODEL_SHADOWRATE, "no GIRF for the shadowrate model (there is no generateGIRF2 script for it)");
  require(H >= 1 && nsim >= 1, "need H >= 1 and nsim >= 1");
  GirfSetup s;
  s.bh = model == CCMM_MODEL_BLOCKHYBRID ? 1 : (model == CCMM_MODEL_HYBRID ? 2 : 0);
  if (s.bh) {
    require(ndxYields != nullptr, "the shadow-rate models need ndxYields");
    require(ch->have_elb_model, "ccmm_chains_set_elb_model was not called");
  }
  if (s.bh == 1) {
    s.actual.resize(N);
    for (int i = 0; i < N; ++i) {
      if (ndxYields[i]) s.yi.push_back(i);
      s.actual[i] = !ndxYields[i];
    }
  } else if (s.bh == 2) {
    s.yi = ch->hNdxS;
    std::sort(s.yi.begin(), s.yi.end());
  }
  s.Ny = (int)s.yi.size();
  require(s.bh == 0 || s.Ny >= 1, "no ring variables");
  const int K = 1 + N * p;
  s.ldX = K + s.Ny * p;
  require(s.bh != 2 || ch->d.K == s.ldX, "hybrid model: K must equal N p + 1 + Ns p");
  const GirfPlan plan = girf_plan(N, p, s.Ny, ch->opt[OPT_GIRF_GENERIC] != 0);
  require(plan.nks <= kGirfMaxKs, "state too large for the GIRF kernel (K + Ny p + N <= 384)");
  require(plan.lds <= kLdsCu && girf_rb_lds(N, p) <= kLdsCu,
          "the GIRF state and its row table do not fit LDS (p (K + Ny p + N) ints + the state)");
  require(ch->stored > 0 && ch->sPAI.p, "no stored draws");
  require(ch->have_slot[slot], "ccmm_chains_set_data was not called for the slot");
  require(t0 - p >= 0 && t0 - p < ch->hT[slot], "t0 - p must be a row of the slot's T");
  if (s.bh) {
    require(ch->have_elb_slot[slot], "ccmm_chains_set_elb_slot was not called for the slot");
    s.npatch = t0 + 1 - ch->hElbT0[slot] - p;  // ndxIRFT0 - elbT0 - p
    if (s.npatch > 0) {
      require(s.npatch <= ch->cfg.elbTmax, "t0 lies beyond the shadow-rate store (n > elbTmax)");
      require(ch->sShadow.p != nullptr, "the chain set has no shadow-rate store");
    }
  }
  for (size_t e = 0; e < (size_t)p * N; ++e)
    require(std::abs(jump[e]) <= 1.79769313486231570815e308, "jump must be finite");
  HIPCHECK(hipSetDevice(ch->ctx->device));
  HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
  const int B = ch->cfg.B;
  std::vector<int> hs(B);
  HIPCHECK(hipMemcpy(hs.data(), ch->slot.p, B * sizeof(int), hipMemcpyDeviceToHost));
  s.c0 = -1;
  for (int c = 0; c < B; ++c)
    if (hs[c] == slot) {
      if (s.c0 < 0) s.c0 = c;
      require(c == s.c0 + s.C, "the chains of the slot must be contiguous");
      ++s.C;
    }
  require(s.C > 0, "no chain bound to the slot");
  s.n = s.C * ch->stored;
  return s;
}

// the device side of one date: the prep kernel's outputs for the n pooled draws
struct GirfInputs {
  DBuf<double> jump, Xj, SV0, sqrtPHI;
  DBuf<int> info, yidx;
};

void girf_prepare(ccmm_chains* ch, const GirfSetup& s, int t0, const double* jump, GirfInputs& in) {
  const int N = ch->d.N, p = ch->cfg.p;
  const size_t cap = ch->cfg.store_capacity;
  hipStream_t st = ch->ctx->stream;
  in.jump.alloc((size_t)p * N);
  in.Xj.alloc((size_t)s.n * s.ldX);
  in.SV0.alloc((size_t)s.n * N);
  in.sqrtPHI.alloc((size_t)s.n * N * N);
  in.info.alloc(s.n);
  HIPCHECK(hipMemcpy(in.jump.p, jump, (size_t)p * N * sizeof(double), hipMemcpyHostToDevice));
  if (s.Ny) {
    in.yidx.alloc(s.Ny);
    HIPCHECK(hipMemcpy(in.yidx.p, s.yi.data(), s.Ny * sizeof(int), hipMemcpyHostToDevice));
  }
  GirfPrepArgs a{};
  a.n = s.n; a.C = s.C; a.stored = ch->stored; a.cap = (int)cap;
  a.N = N; a.p = p; a.T = ch->cfg.T;
  a.Ns = ch->cfg.Ns; a.elbTmax = ch->cfg.elbTmax; a.Ny = s.Ny; a.ring = s.bh ? 1 : 0;
  a.ldX = s.ldX; a.svrow = t0 - p; a.npatch = s.npatch;
  a.sPHI = ch->sPHI_.p + (size_t)s.c0 * cap * (N * (N + 1) / 2);
  a.sSqrtht = ch->sSqrtht.p + (size_t)s.c0 * cap * ch->cfg.T * N;
  a.sShadow = (s.bh && s.npatch > 0) ? ch->sShadow.p + (size_t)s.c0 * cap * ch->cfg.Ns * ch->cfg.elbTmax : nullptr;
  a.jump = in.jump.p; a.ndxS = s.bh ? ch->dNdxS.p : nullptr; a.yidx = s.Ny ? in.yidx.p : nullptr;
  a.Xj = in.Xj.p; a.SV0 = in.SV0.p; a.sqrtPHI = in.sqrtPHI.p; a.info = in.info.p;
  ch->launch(KID_GIRFPREP, [&] { HIPCHECK(girf_prep_launch(st, a)); });
}

}  // namespace

extern "C" {

int ccmm_chains_girf_inputs(ccmm_chains* ch, int slot, int t0, const double* jump, const uint8_t* ndxYields,
                            double* Xj, double* SV0, double* sqrtPHI, int* info) {
  return guarded([&] {
    const GirfSetup s = girf_setup(ch, slot, t0, jump, ndxYields, 1, 1);
    const size_t N = ch->d.N;
    GirfInputs in;
    girf_prepare(ch, s, t0, jump, in);
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    auto down = [&](auto* dst, const auto& buf, size_t cnt) {
      if (dst) HIPCHECK(hipMemcpy(dst, buf.p, cnt * sizeof(*dst), hipMemcpyDeviceToHost));
    };
    down(Xj, in.Xj, (size_t)s.n * s.ldX);
    down(SV0, in.SV0, (size_t)s.n * N);
    down(sqrtPHI, in.sqrtPHI, (size_t)s.n * N * N);
    down(info, in.info, (size_t)s.n);
    if (ch->profiling) ch->collect_profile();
    return s.C;
  });
}

int ccmm_chains_poke_stored_phi(ccmm_chains* ch, int chain, int m, const double* vech) {
  return guarded([&] {
    require(ch && vech, "null argument");
    require(chain >= 0 && chain < ch->cfg.B && m >= 0 && m < ch->stored && ch->sPHI_.p, "no such stored draw");
    const size_t nv = (size_t)ch->d.N * (ch->d.N + 1) / 2;
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    HIPCHECK(hipMemcpy(ch->sPHI_.p + ((size_t)chain * ch->cfg.store_capacity + m) * nv, vech, nv * sizeof(double),
                       hipMemcpyHostToDevice));
    return 0;
  });
}

int ccmm_chains_girf(ccmm_chains* ch, int slot, int t0, const double* jump, int H, int nsim, int nscales,
                     const double* shock11, const uint8_t* cumcode, double np_, const uint8_t* ndxYields,
                     uint64_t seed, int draws_per_pass, int nq, const double* pct, int keep, double* median,
                     double* quantiles, double* rbMedian, double* rbQuantiles, double* draws, double* rbDraws,
                     int* nbad) {
  return guarded([&] {
    require(nscales >= 1 && shock11, "need nscales >= 1 and shock11");
    require(nq >= 0 && (nq == 0 || pct), "bad quantile list");
    require(draws_per_pass >= 0, "draws_per_pass must be >= 0");
    require(!keep || draws, "keep needs draws");
    const GirfSetup s = girf_setup(ch, slot, t0, jump, ndxYields, H, nsim);
    const int N = ch->d.N, p = ch->cfg.p, n = s.n, M = ch->stored, S = H * N;
    const size_t cap = ch->cfg.store_capacity, perP = (size_t)ch->d.K * N;
    const bool rb = s.bh == 0;
    const GirfPassPlan pl = girf_pass_plan(n, N, H, nsim, draws_per_pass);
    hipStream_t st = ch->ctx->stream;
    GirfInputs in;
    girf_prepare(ch, s, t0, jump, in);
    if (nbad) {
      HIPCHECK(hipStreamSynchronize(st));
      std::vector<int> fl(n);
      HIPCHECK(hipMemcpy(fl.data(), in.info.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
      *nbad = (int)std::count_if(fl.begin(), fl.end(), [](int f) { return f != 0; });
    }
    DBuf<double> dPart, dOut, dRb;
    DBuf<uint8_t> dAct, dFl, dCum;
    const size_t nch = (size_t)(nsim + 3) / 4;
    dPart.alloc((size_t)pl.draws * 3 * nch * S);
    dOut.alloc((size_t)pl.draws * 3 * S);
    auto up8 = [&](DBuf<uint8_t>& buf, const uint8_t* src) {
      buf.alloc(N);
      HIPCHECK(hipMemcpy(buf.p, src, N, hipMemcpyHostToDevice));
    };
    if (s.bh == 1) up8(dAct, s.actual.data());
    if (s.bh) up8(dFl, ndxYields);
    if (cumcode) up8(dCum, cumcode);
    if (rb) dRb.alloc((size_t)n * kGirfRbSets * S);
    const size_t segs = (size_t)kGirfSets * S * n;
    ch->postA.alloc(segs);
    ch->postB.alloc(segs);
    // device scratch of the statistics: pct | median | quantiles
    auto stats = [&](int sets, double* med, double* quant) {
      const int SS = sets * S;
      const size_t wb = post_workspace_bytes(SS, n);
      ch->postWs.alloc(wb);
      ch->postOut.alloc((size_t)nq + (size_t)SS * (1 + nq));
      double* dp = ch->postOut.p;
      double* dmed = dp + nq;
      double* dq = dmed + SS;
      if (nq) HIPCHECK(hipMemcpy(dp, pct, nq * sizeof(double), hipMemcpyHostToDevice));
      ch->launch(KID_POSTSTATS, [&] {
        HIPCHECK(post_summaries(st, SS, n, ch->postA.p, ch->postB.p, ch->postWs.p, wb, nullptr, nq, dp, nullptr, dmed,
                                nq ? dq : nullptr, nullptr, nullptr, true));
      });
      HIPCHECK(hipStreamSynchronize(st));
      if (med) HIPCHECK(hipMemcpy(med, dmed, (size_t)SS * sizeof(double), hipMemcpyDeviceToHost));
      // device [nq][sets S] -> host [sets][nq][S]
      if (quant)
        for (int q = 0; q < nq; ++q)
          for (int k = 0; k < sets; ++k)
            HIPCHECK(hipMemcpy(quant + ((size_t)k * nq + q) * S, dq + (size_t)q * SS + (size_t)k * S,
                               (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    };
    for (int sc = 0; sc < nscales; ++sc) {
      for (int d0 = 0; d0 < n; d0 += pl.draws) {
        const int mc = std::min(pl.draws, n - d0);
        // one launch group per chain: the chains' stores are cap, not stored, draws apart
        ch->launch(KID_GIRF, [&] {
          for (int d = d0; d < d0 + mc;) {
            const int c = d / M, m = d - c * M, cnt = std::min(M - m, d0 + mc - d);
            const size_t rec = (size_t)(s.c0 + c) * cap + m;
            GirfArgs a{};
            a.M = cnt; a.N = N; a.p = p; a.H = H; a.nsim = nsim; a.bh = s.bh; a.Ny = s.Ny;
            a.PAI = ch->sPAI.p + rec * perP;
            a.invA = ch->sInvA.p + rec * N * N;
            a.sqrtPHI = in.sqrtPHI.p + (size_t)d * N * N;
            a.SV0 = in.SV0.p + (size_t)d * N;
            a.Xj = in.Xj.p + (size_t)d * s.ldX;
            a.ldX = s.ldX;
            a.actual = s.bh == 1 ? dAct.p : nullptr;
            a.yidx = s.bh ? in.yidx.p : nullptr;
            a.yfloor = s.bh ? dFl.p : nullptr;
            a.elb = ch->cfg.elb; a.shock11 = shock11[sc]; a.seed = seed;
            a.cumcode = cumcode ? dCum.p : nullptr; a.np_ = np_;
            a.part = dPart.p + (size_t)(d - d0) * 3 * nch * S;
            a.out = dOut.p + (size_t)(d - d0) * 3 * S;
            a.force_generic = ch->opt[OPT_GIRF_GENERIC];
            a.m0 = d;
            HIPCHECK(girf_launch(st, a));
            d += cnt;
          }
        });
        ch->launch(KID_GIRFCOLLECT, [&] { HIPCHECK(girf_collect_launch(st, mc, d0, n, S, dOut.p, ch->postA.p)); });
        if (keep)
          HIPCHECK(hipMemcpyAsync(draws + ((size_t)sc * n + d0) * 3 * S, dOut.p, (size_t)mc * 3 * S * sizeof(double),
                                  hipMemcpyDeviceToHost, st));
      }
      stats(kGirfSets, median ? median + (size_t)sc * kGirfSets * S : nullptr,
            quantiles ? quantiles + (size_t)sc * kGirfSets * nq * S : nullptr);
      if (rb) {
        GirfRbArgs r{};
        r.n = n; r.C = s.C; r.stored = M; r.cap = (int)cap; r.N = N; r.p = p; r.K = ch->d.K; r.H = H;
        r.sPAI = ch->sPAI.p + (size_t)s.c0 * cap * perP;
        r.sInvA = ch->sInvA.p + (size_t)s.c0 * cap * N * N;
        r.Xj = in.Xj.p; r.ldX = s.ldX; r.info = in.info.p; r.shock11 = shock11[sc];
        r.cumcode = cumcode ? dCum.p : nullptr; r.np_ = np_; r.rb = dRb.p;
        ch->launch(KID_GIRFRB, [&] { HIPCHECK(girf_rb_launch(st, r)); });
        ch->launch(KID_GIRFCOLLECT, [&] { HIPCHECK(girf_collect_rb_launch(st, n, S, dRb.p, ch->postA.p)); });
        if (keep && rbDraws)
          HIPCHECK(hipMemcpyAsync(rbDraws + (size_t)sc * n * kGirfRbSets * S, dRb.p,
                                  (size_t)n * kGirfRbSets * S * sizeof(double), hipMemcpyDeviceToHost, st));
        stats(kGirfRbSets, rbMedian ? rbMedian + (size_t)sc * kGirfRbSets * S : nullptr,
              rbQuantiles ? rbQuantiles + (size_t)sc * kGirfRbSets * nq * S : nullptr);
      }
    }
    HIPCHECK(hipStreamSynchronize(st));
    if (ch->profiling) ch->collect_profile();
    return s.C;
  });
}

}  // extern "C"

// Maximum VAR roots through the C ABI (ccmm_max_var_root, ccmm_chains_max_var_roots) and check_stationarity
// in the chain set (ccmm_chains_set_stationarity; mcmcVAR.m:221-232, mcmcVARshadowrateBlockHybrid.m:333-347).
// The eigenvalue core and its kernel are ccmm_eig.h / ccmm_eig.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ccmm_chains.h"
#include "ccmm_eig.h"

using namespace ccmm;

void max_var_root_device_src(ccmm_ctx* ctx, int M, int N, int p, const EigSrc& src, DBuf<double>& root,
                             DBuf<int>& finfo, DBuf<double>& scr, double* maxroot, int* info) {
  if (M == 0) return;
  const int n = N * p;
  const EigPlan pl = eig_plan(n, M);
  const size_t per = (size_t)src.ld * N;  // doubles of one matrix from its start
  auto at = [&](long long m) { return src.PAI + (m % src.na) * src.sa + (m / src.na) * src.sb; };
  std::vector<int> fl(M, 2);
  if (pl.device) {
    root.alloc(M);
    finfo.alloc(M);
    scr.alloc(pl.scratch / sizeof(double));
    HIPCHECK(eig_launch(ctx->stream, M, N, p, src, root.p, finfo.p, scr.p));
    HIPCHECK(hipMemcpyAsync(maxroot, root.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipMemcpyAsync(fl.data(), finfo.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
  }
  // the host twin: every matrix of an order the device does not serve, else those that met the iteration cap
  std::vector<int> todo;
  for (int m = 0; m < M; ++m)
    if (fl[m] == 2) todo.push_back(m);
  if (!todo.empty()) {
    std::vector<double> buf(todo.size() * per), r(todo.size());
    std::vector<int> f(todo.size());
    if (!pl.device) HIPCHECK(hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < todo.size(); ++q)
      HIPCHECK(hipMemcpy(buf.data() + q * per, at(todo[q]), per * sizeof(double), hipMemcpyDeviceToHost));
    eig_host((int)todo.size(), N, p, EigSrc{buf.data(), src.ld, (int)todo.size(), (long long)per, 0}, r.data(),
             f.data());
    for (size_t q = 0; q < todo.size(); ++q) {
      maxroot[todo[q]] = r[q];
      fl[todo[q]] = f[q];
    }
  }
  if (info) std::memcpy(info, fl.data(), (size_t)M * sizeof(int));
}

// After the coefficient block of a sweep (run_cta + cta_fallback with attempt 0).  One synchronisation per
// root evaluation; the CTA kernels are launched exactly as in a sweep, for the whole set.
void ccmm_chains::run_stationarity(const RngArgs& ra0) {
  const int B = d.B, N = d.N, p = cfg.p;
  const int nPAI = N * d.KP, nE = N * d.TP;
  std::vector<double> root(B);
  std::vector<int> acc(B, 0);
  const EigSrc src{PAI.p, d.KP, B, (long long)nPAI, 0};
  std::vector<double> hostPAI, hostRoot;
  auto evaluate = [&] {  // accept the open chains whose root is below 1; returns the chains still open
    std::vector<int> todo;
    for (int c = 0; c < B; ++c)
      if (!acc[c]) todo.push_back(c);
    launch(KID_EIG, [&] {
      if ((int)todo.size() >= kEigHostBelow) {  // many chains: the kernel, on the whole set in place
        max_var_root_device_src(ctx, B, N, p, src, eigRoot, eigInfo, eigScr, root.data(), nullptr);
        return;
      }
      // few open chains: their PAI to the host twin (same bits as the kernel; ccmm_eig.h kEigHostBelow)
      hostPAI.resize(todo.size() * (size_t)nPAI);
      hostRoot.resize(todo.size());
      for (size_t q = 0; q < todo.size(); ++q)
        HIPCHECK(hipMemcpyAsync(hostPAI.data() + q * nPAI, PAI.p + (size_t)todo[q] * nPAI, nPAI * sizeof(double),
                                hipMemcpyDeviceToHost, ctx->stream));
      HIPCHECK(hipStreamSynchronize(ctx->stream));
      eig_host((int)todo.size(), N, p, EigSrc{hostPAI.data(), d.KP, (int)todo.size(), (long long)nPAI, 0},
               hostRoot.data(), nullptr);
      for (size_t q = 0; q < todo.size(); ++q) root[todo[q]] = hostRoot[q];
    });
    int open = 0;
    for (int c = 0; c < B; ++c) {
      if (!acc[c] && root[c] < 1.0) acc[c] = 1;  // NaN (non-finite PAI) is not accepted
      open += !acc[c];
    }
    return open;
  };
  int open = evaluate();
  for (int a = 1; open > 0; ++a) {
    if (a > stat_max) {  // the cap: the chains still open keep their last draw and are flagged
      std::vector<int> st(B);
      HIPCHECK(hipMemcpy(st.data(), status.p, B * sizeof(int), hipMemcpyDeviceToHost));
      for (int c = 0; c < B; ++c)
        if (!acc[c]) st[c] |= CCMM_STATUS_NONSTATIONARY;
      HIPCHECK(hipMemcpy(status.p, st.data(), B * sizeof(int), hipMemcpyHostToDevice));
      break;
    }
    statPAI.alloc(PAI.n);
    statE.alloc(E.n);
    statStatus.alloc(B);
    statAcc.alloc(B);
    HIPCHECK(hipMemcpyAsync(statPAI.p, PAI.p, PAI.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(statE.p, E.p, E.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(statStatus.p, status.p, B * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHECK(hipMemcpy(statAcc.p, acc.data(), B * sizeof(int), hipMemcpyHostToDevice));
    for (int c = 0; c < B; ++c) statRedraws[c] += !acc[c];
    RngArgs ra = ra0;
    ra.attempt = (uint32_t)a;
    snapshot_pai();  // the host QR branch redraws from the rejected PAI, as the device does
    run_cta(ra);
    cta_fallback(ra);
    launch(KID_STATSEL, [&] {
      HIPCHECK(eig_launch_stat_select(ctx->stream, B, nPAI, nE, statAcc.p, statPAI.p, statE.p, statStatus.p, PAI.p, E.p,
                                      status.p));
    });
    open = evaluate();
  }
}

extern "C" {

int ccmm_max_var_root(ccmm_ctx* ctx, int M, int N, int p, int K, const double* PAI, double* maxroot, int* info) {
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(M >= 0 && N >= 1 && p >= 1 && (long long)N * p + 1 <= K, "need M >= 0, N, p >= 1, K >= 1 + N p");
    require(M == 0 || (PAI && maxroot), "null argument");
    if (M == 0) return 0;
    if (!eig_plan(N * p, M).device) return ccmm_max_var_root_host(M, N, p, K, PAI, maxroot, info);
    HIPCHECK(hipSetDevice(ctx->device));
    DBuf<double> dP, root, scr;
    DBuf<int> finfo;
    const size_t per = (size_t)K * N;
    // uploads of at most 1 GB: the full run's 164 000 draws at N = 20, p = 12 are 6 GB
    const int step = (int)std::max<size_t>(1, std::min<size_t>(M, ((size_t)1 << 27) / per));
    dP.alloc((size_t)step * per);
    for (int m0 = 0; m0 < M; m0 += step) {
      const int mc = std::min(step, M - m0);
      HIPCHECK(hipMemcpyAsync(dP.p, PAI + (size_t)m0 * per, (size_t)mc * per * sizeof(double), hipMemcpyHostToDevice,
                              ctx->stream));
      max_var_root_device_src(ctx, mc, N, p, EigSrc{dP.p, K, mc, (long long)per, 0}, root, finfo, scr, maxroot + m0,
                              info ? info + m0 : nullptr);
    }
    return 0;
  });
}

int ccmm_chains_max_var_roots(ccmm_chains* ch, int slot, double* maxroot, int* info) {
  return guarded([&] {
    require(ch && maxroot, "null argument");
    require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
    require(ch->cfg.p >= 1, "p must be >= 1");
    require(ch->stored > 0 && ch->sPAI.p, "no stored draws");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const int B = ch->cfg.B;
    std::vector<int> hs(B);
    HIPCHECK(hipMemcpy(hs.data(), ch->slot.p, B * sizeof(int), hipMemcpyDeviceToHost));
    int c0 = -1, C = 0;
    for (int c = 0; c < B; ++c)
      if (hs[c] == slot) {
        if (c0 < 0) c0 = c;
        require(c == c0 + C, "the chains of the slot must be contiguous");
        ++C;
      }
    require(C > 0, "no chain bound to the slot");
    // store: [chain][capacity][K N]; output m * C + c: chain fastest
    const long long per = (long long)ch->d.K * ch->d.N;
    const EigSrc src{ch->sPAI.p + (size_t)c0 * ch->cfg.store_capacity * per, ch->d.K, C,
                     (long long)ch->cfg.store_capacity * per, per};
    max_var_root_device_src(ch->ctx, ch->stored * C, ch->d.N, ch->cfg.p, src, ch->eigRoot, ch->eigInfo, ch->eigScr,
                            maxroot, info);
    return C;
  });
}

int ccmm_chains_set_stationarity(ccmm_chains* ch, int enable, int max_attempts) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    if (enable) {
      require(!ch->cfg.rng_crn, "check_stationarity needs Philox mode: the CRN layout holds one randn(K, N) block per sweep");
      require(ch->cfg.p >= 1, "check_stationarity: p must be >= 1");
      require(max_attempts < (1 << 24), "max_attempts must be below 2^24");
    }
    ch->stat_on = enable != 0;
    ch->stat_max = max_attempts > 0 ? max_attempts : 1000;
    return 0;
  });
}

int ccmm_chains_get_stationarity(ccmm_chains* ch, int64_t* redraws) {
  return guarded([&] {
    require(ch && redraws, "null argument");
    for (int c = 0; c < ch->cfg.B; ++c) redraws[c] = c < (int)ch->statRedraws.size() ? ch->statRedraws[c] : 0;
    return 0;
  });
}

}  // extern "C"

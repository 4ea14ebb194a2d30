// Conditional mean paths through the C ABI (ccmm_cond_mean, ccmm_chains_cond_means;
// doVARshadowrateBlockHybridMissingData.m:433-468 thatMean of every kept draw).  The core and its kernel are
// ccmm_condmean.h / ccmm_condmean.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ccmm_chains.h"
#include "ccmm_condmean.h"

using namespace ccmm;

namespace {

void require_finite(const double* y0, size_t n) {
  for (size_t e = 0; e < n; ++e) require(std::isfinite(y0[e]), "y0 must be finite");
}

}  // namespace

extern "C" {

int ccmm_cond_mean(ccmm_ctx* ctx, int M, int N, int p, int K, int H, const double* PAI, const double* y0, int ny0,
                   double* mean, int* info) {
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(M >= 0 && N >= 1 && p >= 1 && H >= 1 && (long long)N * p + 1 <= K,
            "need M >= 0, N, p, H >= 1, K >= 1 + N p");
    require(ny0 == 1 || ny0 == M, "ny0 must be 1 or M");
    require(M == 0 || (PAI && y0 && mean), "null argument");
    if (M == 0) return 0;
    if (!cond_mean_plan(N, p, M).device) return ccmm_cond_mean_host(M, N, p, K, H, PAI, y0, ny0, mean, info);
    const size_t Np = (size_t)N * p, per = (size_t)K * N;
    require_finite(y0, (size_t)ny0 * Np);
    HIPCHECK(hipSetDevice(ctx->device));
    // uploads of at most 1 GB
    const int step = (int)std::max<size_t>(1, std::min<size_t>(M, ((size_t)1 << 27) / per));
    DBuf<double> dP, dY, dM;
    DBuf<int> dI;
    dP.alloc((size_t)step * per);
    dY.alloc(ny0 == 1 ? Np : (size_t)step * Np);
    dM.alloc((size_t)step * N);
    dI.alloc(step);
    std::vector<int> fl(step);
    if (ny0 == 1) HIPCHECK(hipMemcpyAsync(dY.p, y0, Np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    for (int m0 = 0; m0 < M; m0 += step) {
      const int mc = std::min(step, M - m0);
      HIPCHECK(hipMemcpyAsync(dP.p, PAI + (size_t)m0 * per, (size_t)mc * per * sizeof(double), hipMemcpyHostToDevice,
                              ctx->stream));
      if (ny0 != 1)
        HIPCHECK(hipMemcpyAsync(dY.p, y0 + (size_t)m0 * Np, (size_t)mc * Np * sizeof(double), hipMemcpyHostToDevice,
                                ctx->stream));
      HIPCHECK(cond_mean_launch(ctx->stream, mc, N, p, H, EigSrc{dP.p, K, mc, (long long)per, 0}, dY.p,
                                ny0 == 1 ? 1 : mc, dM.p, dI.p));
      HIPCHECK(hipMemcpyAsync(mean + (size_t)m0 * N, dM.p, (size_t)mc * N * sizeof(double), hipMemcpyDeviceToHost,
                              ctx->stream));
      HIPCHECK(hipMemcpyAsync(fl.data(), dI.p, (size_t)mc * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHECK(hipStreamSynchronize(ctx->stream));
      if (info) std::memcpy(info + m0, fl.data(), (size_t)mc * sizeof(int));
    }
    return 0;
  });
}

int ccmm_chains_cond_means(ccmm_chains* ch, int slot, int H, const double* y0, double* mean, int* info) {
  return guarded([&] {
    require(ch && y0 && mean, "null argument");
    require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
    require(H >= 1, "need H >= 1");
    require(ch->cfg.p >= 1, "p must be >= 1");
    require(ch->stored > 0 && ch->sPAI.p, "no stored draws");
    const int N = ch->d.N, p = ch->cfg.p, B = ch->cfg.B;
    const size_t Np = (size_t)N * p;
    require_finite(y0, Np);
    HIPCHECK(hipSetDevice(ch->ctx->device));
    hipStream_t st = ch->ctx->stream;
    HIPCHECK(hipStreamSynchronize(st));
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
    // store: [chain][capacity][K N]; output m * C + c: chain fastest, as ccmm_chains_max_var_roots
    const int n = ch->stored * C;
    const long long per = (long long)ch->d.K * N;
    const double* base = ch->sPAI.p + (size_t)c0 * ch->cfg.store_capacity * per;
    const EigSrc src{base, ch->d.K, C, (long long)ch->cfg.store_capacity * per, per};
    if (!cond_mean_plan(N, p, n).device) {  // a shape beyond the kernel: the stored draws to the host twin
      std::vector<double> host((size_t)n * per);
      for (int c = 0; c < C; ++c)
        for (int m = 0; m < ch->stored; ++m)
          HIPCHECK(hipMemcpy(host.data() + ((size_t)m * C + c) * per, base + ((size_t)c * ch->cfg.store_capacity + m) * per,
                             per * sizeof(double), hipMemcpyDeviceToHost));
      cond_mean_host(n, N, p, H, EigSrc{host.data(), ch->d.K, n, per, 0}, y0, 1, mean, info);
      return C;
    }
    ch->cmY0.alloc(Np);
    ch->cmMean.alloc((size_t)n * N);
    ch->cmInfo.alloc(n);
    HIPCHECK(hipMemcpyAsync(ch->cmY0.p, y0, Np * sizeof(double), hipMemcpyHostToDevice, st));
    ch->launch(KID_CONDMEAN, [&] { HIPCHECK(cond_mean_launch(st, n, N, p, H, src, ch->cmY0.p, 1, ch->cmMean.p, ch->cmInfo.p)); });
    HIPCHECK(hipMemcpyAsync(mean, ch->cmMean.p, (size_t)n * N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (info) HIPCHECK(hipMemcpy(info, ch->cmInfo.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    if (ch->profiling) ch->collect_profile();
    return C;
  });
}

}  // extern "C"

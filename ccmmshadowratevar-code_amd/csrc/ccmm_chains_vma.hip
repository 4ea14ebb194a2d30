// Impulse responses through the C ABI (ccmm_vma, ccmm_vma_form) and their per-vintage summaries over the
// stored draws of a chain set (ccmm_chains_vma_summaries; goVARshadowrateBlockHybrid.m:393-429 VMAmid / VMAtail,
// sumFFRmid / sumFFRtail).  The core and its kernels are ccmm_vma.h / ccmm_vma.hip, the order statistics
// ccmm_post.hip.
#include <algorithm>
#include <cstring>

#include "ccmm_chains.h"
#include "ccmm_post.h"
#include "ccmm_vma.h"

using namespace ccmm;

namespace {

// host PAI in chunks through the kernel: each chunk's upload and its draw-major result stay within kVmaBufCap
int vma_device(ccmm_ctx* ctx, int form, int M, int N, int p, int K, int H, const double* PAI, double* vma, int* info,
               double* kernel_ms) {
  HIPCHECK(hipSetDevice(ctx->device));
  const size_t per = (size_t)K * N, outper = (size_t)H * N * N;
  const size_t fit = kVmaBufCap / (std::max(per, outper) * sizeof(double));
  const int step = (int)std::max<size_t>(1, std::min<size_t>(M, fit));
  DBuf<double> dP, dV;
  DBuf<int> dI;
  dP.alloc((size_t)step * per);
  dV.alloc((size_t)step * outper);
  dI.alloc(step);
  std::vector<int> fl(step);
  hipEvent_t a = nullptr, b = nullptr;
  if (kernel_ms) {
    *kernel_ms = 0.0;
    HIPCHECK(hipEventCreate(&a));
    HIPCHECK(hipEventCreate(&b));
  }
  for (int m0 = 0; m0 < M; m0 += step) {
    const int mc = std::min(step, M - m0);
    HIPCHECK(hipMemcpyAsync(dP.p, PAI + (size_t)m0 * per, (size_t)mc * per * sizeof(double), hipMemcpyHostToDevice,
                            ctx->stream));
    if (kernel_ms) HIPCHECK(hipEventRecord(a, ctx->stream));
    HIPCHECK(vma_launch(ctx->stream, form, mc, N, p, EigSrc{dP.p, K, mc, (long long)per, 0}, 0, H, dV.p, dI.p));
    if (kernel_ms) HIPCHECK(hipEventRecord(b, ctx->stream));
    HIPCHECK(hipMemcpyAsync(vma + (size_t)m0 * outper, dV.p, (size_t)mc * outper * sizeof(double),
                            hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipMemcpyAsync(fl.data(), dI.p, (size_t)mc * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (info) std::memcpy(info + m0, fl.data(), (size_t)mc * sizeof(int));
    if (kernel_ms) {
      float ms = 0.f;
      HIPCHECK(hipEventElapsedTime(&ms, a, b));
      *kernel_ms += ms;
    }
  }
  if (kernel_ms) {
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
  return 0;
}

void check_vma_args(const ccmm_ctx* ctx, int M, int N, int p, int K, int H, const double* PAI, const double* vma) {
  require(ctx != nullptr, "null context");
  require(M >= 0 && N >= 1 && p >= 1 && H >= 1 && (long long)N * p + 1 <= K,
          "need M >= 0, N, p, H >= 1, K >= 1 + N p");
  require(M == 0 || (PAI && vma), "null argument");
}

}  // namespace

extern "C" {

int ccmm_vma(ccmm_ctx* ctx, int M, int N, int p, int K, int H, const double* PAI, double* vma, int* info) {
  return guarded([&] {
    check_vma_args(ctx, M, N, p, K, H, PAI, vma);
    if (M == 0) return 0;
    if (!vma_plan(N, p, M, H).device) return ccmm_vma_host(M, N, p, K, H, PAI, vma, info);
    return vma_device(ctx, 0, M, N, p, K, H, PAI, vma, info, nullptr);
  });
}

int ccmm_vma_form(ccmm_ctx* ctx, int form, int M, int N, int p, int K, int H, const double* PAI, double* vma,
                  int* info, double* kernel_ms) {
  return guarded([&] {
    check_vma_args(ctx, M, N, p, K, H, PAI, vma);
    require(form == 0 || form == 1, "form must be 0 (MFMA) or 1 (vector ALU)");
    require(M >= 1 && vma_plan(N, p, M, H).device, "ccmm_vma_form serves the device range only (N <= 32, N p <= 256)");
    return vma_device(ctx, form, M, N, p, K, H, PAI, vma, info, kernel_ms);
  });
}

int ccmm_chains_vma_summaries(ccmm_chains* ch, int slot, int H, int hslab, int nq, const double* pct,
                              double* vmaMedian, double* vmaQuantiles, int ffr, double* sumMedian,
                              double* sumQuantiles, int* nbad) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
    require(H >= 1 && hslab >= 0, "need H >= 1 and hslab >= 0");
    require(nq >= 0 && (nq == 0 || pct), "bad quantile list");
    require(ch->cfg.p >= 1, "p must be >= 1");
    require(ch->stored > 0 && ch->sPAI.p, "no stored draws");
    const int N = ch->d.N, p = ch->cfg.p, B = ch->cfg.B, NN = N * N;
    require(ffr >= -1 && ffr < N, "ffr out of range");
    require(ffr < 0 || sumMedian || sumQuantiles, "ffr >= 0 needs sumMedian or sumQuantiles");
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
    // store: [chain][capacity][K N]; draw d = cc * stored + m (chain slowest), the order post_gather_pai reads
    const int M = ch->stored, n = M * C;
    const long long per = (long long)ch->d.K * N;
    const EigSrc src{ch->sPAI.p + (size_t)c0 * ch->cfg.store_capacity * per, ch->d.K, M, per,
                     (long long)ch->cfg.store_capacity * per};
    VmaPlan pl = vma_plan(N, p, n, H);
    require(pl.device, "ccmm_chains_vma_summaries serves N <= 32 and N p <= 256");
    if (hslab > 0) {
      const int hsz = std::min(hslab, H);
      require((size_t)hsz * n * NN * sizeof(double) <= kVmaBufCap, "hslab: a buffer of one pass would exceed 1 GB");
      pl.hslab = hsz;
      pl.nslab = (H + hsz - 1) / hsz;
      pl.buf = (size_t)hsz * n * NN * sizeof(double);
    }
    const size_t cnt = pl.buf / sizeof(double);
    ch->vmaBuf.alloc(cnt);
    ch->vmaInfo.alloc(n);
    ch->postA.alloc(cnt);
    ch->postB.alloc(cnt);
    // device scratch of the statistics: pct | median | quantiles
    auto stats = [&](int S, double* med, double* quant, size_t ldq) {
      const size_t wb = post_workspace_bytes(S, n);
      ch->postWs.alloc(wb);
      ch->postOut.alloc((size_t)nq + (size_t)S * (1 + nq));
      double* dp = ch->postOut.p;
      double* dmed = dp + nq;
      double* dq = dmed + S;
      if (nq) HIPCHECK(hipMemcpy(dp, pct, nq * sizeof(double), hipMemcpyHostToDevice));
      ch->launch(KID_POSTSTATS, [&] {
        HIPCHECK(post_summaries(st, S, n, ch->postA.p, ch->postB.p, ch->postWs.p, wb, nullptr, nq, dp, nullptr, dmed,
                                nq ? dq : nullptr, nullptr, nullptr));
      });
      HIPCHECK(hipStreamSynchronize(st));
      if (med) HIPCHECK(hipMemcpy(med, dmed, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
      if (quant)
        for (int q = 0; q < nq; ++q)
          HIPCHECK(hipMemcpy(quant + (size_t)q * ldq, dq + (size_t)q * S, (size_t)S * sizeof(double),
                             hipMemcpyDeviceToHost));
    };
    for (int h0 = 0; h0 < H; h0 += pl.hslab) {
      const int h1 = std::min(H, h0 + pl.hslab), S = NN * (h1 - h0);
      ch->launch(KID_VMA, [&] { HIPCHECK(vma_launch(st, 0, n, N, p, src, h0, h1, ch->vmaBuf.p, ch->vmaInfo.p)); });
      ch->launch(KID_POSTGATHER, [&] { HIPCHECK(post_gather_pai(st, ch->vmaBuf.p, 0, C, M, M, S, ch->postA.p)); });
      stats(S, vmaMedian ? vmaMedian + (size_t)h0 * NN : nullptr, vmaQuantiles ? vmaQuantiles + (size_t)h0 * NN : nullptr,
            (size_t)NN * H);
    }
    if (nbad) {
      std::vector<int> fl(n);
      HIPCHECK(hipMemcpy(fl.data(), ch->vmaInfo.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
      *nbad = (int)std::count_if(fl.begin(), fl.end(), [](int f) { return f != 0; });
    }
    if (ffr >= 0) {
      ch->launch(KID_SUMFFR, [&] { HIPCHECK(vma_launch_sum_ffr(st, n, N, p, src, ffr, ch->postA.p)); });
      stats(N, sumMedian, sumQuantiles, (size_t)N);
    }
    if (ch->profiling) ch->collect_profile();
    return C;
  });
}

}  // extern "C"

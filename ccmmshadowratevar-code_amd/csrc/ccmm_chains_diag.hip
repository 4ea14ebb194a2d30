// Compute_diagnostics through the C ABI (goVARshadowrateBlockHybrid.m:313-316, Diagnostics.m): ccmm_diagnostics
// on host draws and ccmm_chains_diagnostics on the stored draws of a chain set, read in place.  The per-series
// core and the kernel are ccmm_diagk.h / ccmm_diagk.hip; the host twin is ccmm_diagnostics_host (ccmm_diag.cpp).
#include <algorithm>
#include <cstring>

#include "ccmm_chains.h"
#include "ccmm_diagk.h"

using namespace ccmm;

extern "C" {

int ccmm_diagnostics(ccmm_ctx* ctx, int M, int S, const double* draws, double* out) {
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(S >= 0 && (S == 0 || (draws && out)), "ccmm_diagnostics: S >= 0, draws and out required");
    require(M >= kDiagNG, "momentg: needs a larger number of ndraws");  // Diagnostics.m:185-187
    if (S == 0) return 0;
    HIPCHECK(hipSetDevice(ctx->device));
    // series blocks of a fixed scratch: the block as it lies on the host (series-major), its transpose
    // (entry fastest, what the kernel reads) and the block's 11 statistics
    const int sb = std::min(S, diag_block_series(M));
    DBuf<double> in, tr, res;
    in.alloc((size_t)sb * M);
    tr.alloc((size_t)sb * M);
    res.alloc((size_t)kDiagNStat * sb);
    std::vector<double> h((size_t)kDiagNStat * sb);
    for (int s0 = 0; s0 < S; s0 += sb) {
      const int sc = std::min(sb, S - s0);
      HIPCHECK(hipMemcpyAsync(in.p, draws + (size_t)s0 * M, (size_t)sc * M * sizeof(double), hipMemcpyHostToDevice,
                              ctx->stream));
      HIPCHECK(diag_transpose_launch(ctx->stream, in.p, M, sc, tr.p));
      HIPCHECK(diag_launch(ctx->stream, tr.p, sc, 0, sc, 1, M, nullptr, nullptr, res.p));
      HIPCHECK(hipMemcpyAsync(h.data(), res.p, (size_t)kDiagNStat * sc * sizeof(double), hipMemcpyDeviceToHost,
                              ctx->stream));
      HIPCHECK(hipStreamSynchronize(ctx->stream));
      for (int k = 0; k < kDiagNStat; ++k)
        std::memcpy(out + (size_t)k * S + s0, h.data() + (size_t)k * sc, (size_t)sc * sizeof(double));
    }
    return 0;
  });
}

int ccmm_chains_diagnostics(ccmm_chains* ch, int source, int slot, double* out) {
  return guarded([&] {
    require(ch && out, "null argument");
    require(source >= 0 && source <= 4, "source must be 0 (PAI), 1 (PHI), 2 (invA), 3 (sqrtht) or 4 (shadowrate)");
    require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
    require(ch->stored >= kDiagNG && ch->sPAI.p, "momentg: needs a larger number of ndraws");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const int B = ch->cfg.B, N = ch->d.N, K = ch->d.K, Tmax = ch->cfg.T;
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
    // store: [chain][capacity][entry]
    const double* src = nullptr;
    long long S = 0;
    const int* nvalid = nullptr;
    const uint8_t* mask = nullptr;
    switch (source) {
      case 0: src = ch->sPAI.p, S = (long long)K * N; break;
      case 1: src = ch->sPHI_.p, S = (long long)N * (N + 1) / 2; break;
      case 2: src = ch->sInvA.p, S = (long long)N * N; break;
      case 3: {  // Tmax x N, t fastest (k_store): the rows t >= T of the slot hold no draw
        src = ch->sSqrtht.p, S = (long long)Tmax * N;
        std::vector<uint8_t> m((size_t)S);
        for (long long e = 0; e < S; ++e) m[e] = (e % Tmax) < ch->hT[slot];
        ch->diagMask.alloc((size_t)S);
        HIPCHECK(hipMemcpy(ch->diagMask.p, m.data(), (size_t)S, hipMemcpyHostToDevice));
        mask = ch->diagMask.p;
        break;
      }
      default: {  // elbTmax x Ns, rate fastest (k_elb_store): the cells of the slot's sNaN within its elbT
        require(ch->bh && ch->cfg.elbTmax > 0 && ch->sShadow.p, "source 4: no stored shadow rates");
        require(ch->have_elb_slot[slot], "source 4: ccmm_chains_set_elb_slot was not called for the slot");
        src = ch->sShadow.p, S = (long long)ch->cfg.Ns * ch->cfg.elbTmax;
        mask = ch->dSNaN.p + (size_t)slot * S;
        const std::vector<int> cnt(C, ch->cfg.Ns * ch->hElbT[slot]);
        ch->diagCnt.alloc(C);
        HIPCHECK(hipMemcpy(ch->diagCnt.p, cnt.data(), C * sizeof(int), hipMemcpyHostToDevice));
        nvalid = ch->diagCnt.p;
      }
    }
    require(src != nullptr && S > 0 && S <= 0x7fffffff, "no stored draws of the source");
    const long long ldc = (long long)ch->cfg.store_capacity * S;
    const size_t nout = (size_t)kDiagNStat * C * S;
    ch->diagOut.alloc(nout);
    ch->launch(KID_DIAG, [&] {
      HIPCHECK(diag_launch(ch->ctx->stream, src + (size_t)c0 * ldc, S, ldc, (int)S, C, ch->stored, nvalid, mask,
                           ch->diagOut.p));
    });
    HIPCHECK(hipMemcpyAsync(out, ch->diagOut.p, nout * sizeof(double), hipMemcpyDeviceToHost, ch->ctx->stream));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    return C;
  });
}

}  // extern "C"

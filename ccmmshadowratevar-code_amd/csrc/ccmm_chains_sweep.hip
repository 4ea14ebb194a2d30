// The Gibbs blocks of one sweep of a chain set (ccmm_chains.h) on the small, lag and large paths, the draw
// store and the host QR fallback, then ccmm_chains_sweep.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

#include "ccmm_chains.h"
#include "ccmm_svpart.h"
#include "ccmm_bign.h"

using namespace ccmm;

// ---------------------------------------------------------- kernel launches
RngArgs ccmm_chains::rng_args(const double* dcrn, int64_t stride) const {
  RngArgs ra{};
  ra.crn = dcrn;
  ra.crn_chain_stride = stride;
  ra.seed = cfg.seed;
  ra.sweep = sweep;
  ra.ids = have_ids ? rngIds.p : nullptr;
  for (int i = 0; i < kRngBlocks; ++i) ra.off[i] = crn_off[i];
  return ra;
}

void ccmm_chains::ensure_cta() {
  if (!G.p) {
    G.alloc((size_t)d.nmat * d.KP * d.KP);
    // the fused NT = 18 path (256 < K <= 288, KP = 320) never writes rows / columns past 288:
    // they stay zero for k_cta_solve2's 64-row blocks
    HIPCHECK(hipMemsetAsync(G.p, 0, G.n * sizeof(double), ctx->stream));
  }
  rdiag.alloc((size_t)d.nmat * d.KP);
}
void ccmm_chains::run_resid() {
  launch(KID_RESID, [&] { HIPCHECK(launch_resid(ctx->stream, d, Tslot.p, xsel(), view())); });
  resid_valid = true;
}
void ccmm_chains::run_weights(const ChainState& cs, int sqrt_form) {
  launch(KID_WEIGHTS, [&] { HIPCHECK(launch_cta_weights(ctx->stream, d, Tslot.p, cs, sqrt_form)); });
}

void ccmm_chains::run_cta(const RngArgs& ra) {
  ensure_cta();
  ChainState cs = view();
  if (!resid_valid) run_resid();
  if (big) {
    run_cta_big(ra, cs);
    return;
  }
  if (lag_active()) {
    run_cta_lag(ra, cs);
    return;
  }
  // generic design (KP <= 256): the register-tiled fused Gram + Cholesky, then the per-chain solve
  const int fnt = d.KP / 16;
  require(gram_chol_supported(fnt), "k_gram_chol: unsupported KP");
  run_weights(cs, 1);
  launch(KID_GRAMCHOL, [&] {
    HIPCHECK(launch_gram_chol(fnt, ctx->stream, d, Tslot.p, xsel(), cs, iVdiag.p, rdiag.p, gc_mode));
  });
  join_fcst();  // the previous kept sweep's predictive density reads PAI
  launch(KID_SOLVE, [&] {
    HIPCHECK(launch_cta_solve2(ctx->stream, d, Tslot.p, iVb.p, xsel(), cs, rdiag.p, ra));
  });
}

// large-N blocks (N > 32; ccmm_bign.hip)
void ccmm_chains::run_astep_big(const RngArgs& ra) {
  const size_t np = (size_t)bign_astep_npad(d);
  bigW.alloc((size_t)d.B * (d.N - 1) * np * np);
  ChainState cs = view();
  launch(KID_ASTEPBIG, [&] {
    HIPCHECK(bign_launch_astep(ctx->stream, d, Tslot.p, cs, ra, cfg.logy2offset, bigW.p));
  });
}

// CTA for large systems (ccmm_big.hip): weights -> multi-equation MFMA Gram -> per-system
// blocked Cholesky -> per-chain sequential solve
void ccmm_chains::run_cta_big(const RngArgs& ra, const ChainState& cs) {
  Ubuf.alloc((size_t)d.B * d.N * d.TP);
  Dinv.alloc((size_t)d.nmat * d.KP * 64);
  PhaseScope phase(ctx->device, mfma_lock, ctx->stream, mfma_ev);
  run_weights(cs, 0);
  // (a phase CCMM_BIG_MASK drops still records its event pair)
  launch(KID_GRAMBIG, [&] {
    if (big_mask & kBigGram)
      HIPCHECK(big_launch_gram(ctx->stream, d, Tslot.p, xsel(), cs, bigGroups.p, nGroups, colx()));
  });
  launch(KID_CHOLBIG, [&] {
    if (big_mask & kBigChol) HIPCHECK(big_launch_chol(ctx->stream, d, slot.p, iVdiag.p, cs, rdiag.p, Dinv.p));
  });
  phase.release();
  join_fcst();  // the previous kept sweep's predictive density reads PAI
  launch(KID_SOLVEBIG, [&] {
    if (big_mask & kBigSolve)
      HIPCHECK(big_launch_solve(ctx->stream, d, Tslot.p, iVb.p, xsel(), cs, rdiag.p, ra, Ubuf.p, Dinv.p, colx()));
  });
}

// k_cta_solve_lag on two workgroups per chain (bit-identical draws; the halves spin on each other's
// X'v partials): only when all 2B workgroups can be resident at once, so no half waits on a partner
// that cannot start (auto: also B <= kSolveSplitMaxB, where the split pays)
bool ccmm_chains::solve_split_ok() {
  const int o = opt[OPT_SOLVE_SPLIT];
  if (o == 0 || (o < 0 && d.B > kSolveSplitMaxB)) return false;
  if (split_resident < 0) {
    const int nmax = n_bucket(d.N);
    split_resident = lag_solve_resident(lagNT, nmax, sl_lds_bytes(lagNT, drows, ldd, d.TP, nmax), opt[OPT_SOLVE_ASYNC]);
  }
  return 2 * d.B <= split_resident;
}

// CTA on the lag structure: sqrt weights -> Gram + Cholesky + inverse -> sequential solve
void ccmm_chains::run_cta_lag(const RngArgs& ra, const ChainState& cs) {
  run_weights(cs, 1);
  const LagSel ls = lagsel();
  const size_t lds_g = gl_lds_bytes(lagNT, drows, ldd, d.TP);
  const int nmax = n_bucket(d.N);
  const size_t lds_s = sl_lds_bytes(lagNT, drows, ldd, d.TP, nmax);
  PhaseScope phase(ctx->device, mfma_lock, ctx->stream, mfma_ev);  // same phase lock as run_cta_big
  launch(KID_GRAMLAG, [&] {
    HIPCHECK(lag_launch_gram(lagNT, ctx->stream, lds_g, d, Tslot.p, ls, cs, iVdiag.p));
  });
  phase.release();
  SolveXch xc{nullptr, nullptr, 0};
  if (solve_split_ok()) {
    if (!solveFlag.p) {
      solveXch.alloc((size_t)d.B * 2 * 2 * 256);
      solveFlag.alloc((size_t)d.B * 2);
      HIPCHECK(hipMemsetAsync(solveFlag.p, 0, (size_t)d.B * 2 * sizeof(uint64_t), ctx->stream));
    }
    xc = SolveXch{solveXch.p, (unsigned long long*)solveFlag.p, ++solve_epoch};
  }
  join_fcst();  // the previous kept sweep's predictive density reads PAI
  launch(KID_SOLVELAG, [&] {
    HIPCHECK(lag_launch_solve(lagNT, nmax, opt[OPT_SOLVE_ASYNC], ctx->stream, lds_s, d, Tslot.p, iVb.p, xsel(), ls,
                              cs, ra, xc));
  });
}

void ccmm_chains::run_astep(const RngArgs& ra) {
  if (d.N > kMaxNSmall) {
    run_astep_big(ra);
    return;
  }
  ChainState cs = view();
  const int N = d.N;
  if (!astepTab.p) {  // the 4 x 4 Gram tiles (ii, A, B) of astep_gram_tiles, largest ii first
    std::vector<int> tab(1, 0);
    for (int ii = N - 1; ii >= 1; --ii)
      for (int A = 0; 4 * A <= ii; ++A)
        for (int Bk = 0; Bk <= A && 4 * Bk < ii; ++Bk) tab.push_back(ii << 16 | A << 8 | Bk);
    tab[0] = (int)tab.size() - 1;
    astepTab.alloc(tab.size());
    HIPCHECK(hipMemcpy(astepTab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  launch(KID_ASTEP, [&] {
    HIPCHECK(launch_astep(opt[OPT_ASTEP_SERIAL] != 0, ctx->stream, d, Tslot.p, cs, ra, cfg.logy2offset, astepTab.p));
  });
}

// SV scratch of the partitioned sampler (ccmm_svpart.hip): block factors C_t, w_t,
// separator records, fill vectors g_t; matrices padded to the bucket size NN
void ccmm_chains::ensure_sv() {
  const size_t NN = sv_bucket(d.N);
  svLd.alloc((size_t)d.B * (d.TP + 1) * NN * NN);
  svw.alloc((size_t)d.B * (d.TP + 1) * NN);
  svSep.alloc((size_t)d.B * sv_sep_len(d.N));
  svG.alloc((size_t)2 * d.B * (d.TP + 1) * NN);  // fill vectors g | SV normals z
}

// KSC indicators, then the partitioned sampler (N <= 32) or the large-N sampler (ccmm_bign.hip)
void ccmm_chains::run_sv(const RngArgs& ra) {
  const bool bign = d.N > kMaxNSmall;
  if (bign)
    bigScr.alloc((size_t)d.B * bign_sv_scratch(d));
  else
    ensure_sv();
  ChainState cs = view();
  launch(KID_SVMIX, [&] { HIPCHECK(launch_sv_mix(ctx->stream, d, Tslot.p, cs, ra)); });
  if (bign)
    launch(KID_SVBIG, [&] {
      HIPCHECK(bign_launch_sv(ctx->stream, d, Tslot.p, V0inv.p, V0invm.p, cs, ra, bigScr.p));
    });
  else
    launch(KID_SVSAMPLE, [&] {
      HIPCHECK(sv_launch_part(d.N, ctx->stream, d, Tslot.p, V0inv.p, V0invm.p, cs, ra, svSep.p, svG.p, sv_mode,
                              opt[OPT_SV_NWG], opt[OPT_SV_MFMA] != 0));
    });
}

// the inverse-Wishart normals, then k_phi (N <= 32) or k_phi_big (always in stream order: sweep_once forks N <= 32 only)
void ccmm_chains::run_phi(const RngArgs& ra, hipStream_t on) {
  const bool bign = d.N > kMaxNSmall;
  hipStream_t st = on ? on : ctx->stream;
  Zphi.alloc((size_t)d.B * d.N * (d.TP + cfg.dPHI));
  if (bign) bigScr.alloc((size_t)d.B * bign_sv_scratch(d));  // >= 3 N^2 per chain
  ChainState cs = view();
  launch(KID_PHIGEN, [&] { HIPCHECK(launch_phi_gen(st, d, Tslot.p, cfg.dPHI, cs, ra)); }, st);
  if (bign)
    launch(KID_PHIBIG, [&] { HIPCHECK(bign_launch_phi(st, d, Tslot.p, cfg.dPHI, sPHI.p, cs, bigScr.p)); }, st);
  else
    launch(KID_PHI, [&] { HIPCHECK(launch_phi(st, d, Tslot.p, cfg.dPHI, sPHI.p, cs, opt[OPT_PHI_STAGE])); }, st);
}

void ccmm_chains::run_store() {
  if (cfg.store_capacity <= 0) return;
  if (stored >= cfg.store_capacity) throw ArgError("draw store full: call ccmm_chains_get_draws");
  const size_t B = d.B, N = d.N, K = d.K, cap = cfg.store_capacity;
  sPAI.alloc(B * cap * K * N);
  sPHI_.alloc(B * cap * N * (N + 1) / 2);
  sInvA.alloc(B * cap * N * N);
  sSqrtht.alloc(B * cap * (size_t)cfg.T * N);
  Store st{sPAI.p, sPHI_.p, sInvA.p, sSqrtht.p, cfg.store_capacity, stored, cfg.T};
  ChainState cs = view();
  launch(KID_STORE, [&] { HIPCHECK(launch_store(ctx->stream, d, cs, st)); });
  if (bh && cfg.elbTmax > 0) {
    sShadow.alloc(B * cap * cfg.Ns * cfg.elbTmax);
    ElbDev e = elb_view();
    launch(KID_STORE, [&] {
      if (elb_missing)  // shadowrate = NaN (:492; mcmcVARshadowrate.m:448)
        HIPCHECK(launch_ps_first_store(ctx->stream, d.B, nullptr, e.elbT, cs.slot, sShadow.p, cfg.Ns * cfg.elbTmax,
                                       cfg.Ns, cfg.store_capacity, stored));
      else
        HIPCHECK(launch_elb_store(ctx->stream, d.B, e, cs, sShadow.p, cfg.store_capacity, stored));
    });
    if (keep_first) {  // missingrate_all (mcmcVARshadowrate.m:498)
      sMissing.alloc(B * cap * cfg.Ns * cfg.elbTmax);
      ElbDev e2 = elb_view();
      launch(KID_STORE, [&] {
        HIPCHECK(launch_ps_first_store(ctx->stream, d.B,
                                       ((last_ps || elb_missing || elb_alt) && psFirst.p) ? psFirst.p : nullptr, e2.elbT,
                                       cs.slot, sMissing.p, cfg.Ns * cfg.elbTmax, cfg.Ns, cfg.store_capacity, stored));
      });
    }
    if (ps_np > 0) {  // stackAccept (:457): ndxAccept of the stored sweep, 0 = none / Gibbs
      sAccept.alloc(B * cap);
      launch(KID_STORE, [&] {
        HIPCHECK(launch_ps_store(ctx->stream, (last_ps && !elb_missing) ? psFlag.p : nullptr, sAccept.p, d.B,
                                 cfg.store_capacity, stored));
      });
    }
  }
  ++stored;
}

void ccmm_chains::snapshot_pai() {
  if (!opt[OPT_QR_FALLBACK]) return;
  paiPrev.alloc(PAI.n);
  HIPCHECK(hipMemcpyAsync(paiPrev.p, PAI.p, PAI.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
}

int ccmm_chains::cta_fallback(const RngArgs& ra) {
  if (!opt[OPT_QR_FALLBACK]) return 0;
  const bool force_qr = opt[OPT_FORCE_QR] != 0;
  const int B = d.B, N = d.N, K = d.K, KP = d.KP, TP = d.TP;
  std::vector<int> st(B);
  HIPCHECK(hipMemcpyAsync(st.data(), status.p, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  std::vector<int> bad;
  for (int c = 0; c < B; ++c)
    if (force_qr || (st[c] & 2)) bad.push_back(c);
  if (bad.empty()) return 0;
  auto dl = [&](const auto* src, size_t n, auto& dst) {
    dst.resize(n);
    HIPCHECK(hipMemcpy(dst.data(), src, n * sizeof(dst[0]), hipMemcpyDeviceToHost));
  };
  std::vector<int> hslot, hT, hxi, hyi;
  dl(slot.p, (size_t)B, hslot);
  dl(Tslot.p, (size_t)cfg.ndata, hT);
  dl(xidx.p, (size_t)B * N, hxi);
  dl(yidx.p, (size_t)B, hyi);
  zHost.alloc((size_t)K * N);
  // inputs of every flagged chain to the host, the redraws in parallel, PAI back
  struct Job {
    int c, T, fl = 0;
    std::vector<double> Y, A, Ae, sh, ivd, ivb, pai, z;
    std::vector<uint8_t> at;
    std::vector<std::vector<double>> X;
    std::vector<const double*> Xs;
  };
  std::vector<Job> jobs(bad.size());
  for (size_t q = 0; q < bad.size(); ++q) {
    Job& jb = jobs[q];
    const int c = bad[q], s = hslot[c];
    jb.c = c;
    jb.T = hT[s];
    dl(Ypool.p + (size_t)hyi[c] * N * TP, (size_t)N * TP, jb.Y);
    dl(A.p + (size_t)c * N * N, (size_t)N * N, jb.A);
    if (aswitch) {
      dl(AelbD.p + (size_t)c * N * N, (size_t)N * N, jb.Ae);
      dl(atELBD.p + (size_t)c * TP, (size_t)TP, jb.at);
    }
    dl(sqrtht.p + (size_t)c * N * TP, (size_t)N * TP, jb.sh);
    dl(iVdiag.p + (size_t)s * N * KP, (size_t)N * KP, jb.ivd);
    dl(iVb.p + (size_t)s * N * KP, (size_t)N * KP, jb.ivb);
    dl(paiPrev.p + (size_t)c * N * KP, (size_t)N * KP, jb.pai);
    HIPCHECK(launch_rng_normals(ctx->stream, ra, c, (int)CCMM_RNG_PAI, K * N, zHost.p));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    dl(zHost.p, (size_t)K * N, jb.z);
    jb.X.assign(N, {});
    jb.Xs.assign(N, nullptr);
    for (int j = 0; j < N; ++j) {
      int first = j;  // equations sharing a slab share the download
      for (int r = 0; r < j; ++r)
        if (hxi[(size_t)c * N + r] == hxi[(size_t)c * N + j]) {
          first = r;
          break;
        }
      if (first == j) dl(Xpool.p + (size_t)hxi[(size_t)c * N + j] * KP * TP, (size_t)KP * TP, jb.X[j]);
      jb.Xs[j] = jb.X[first].data();
    }
  }
  {
    std::atomic<size_t> next{0};
    auto work = [&] {
      for (size_t q; (q = next++) < jobs.size();) {
        Job& jb = jobs[q];
        jb.fl = host_cta_chain(N, K, jb.T, jb.Y.data(), TP, jb.Xs.data(), TP, jb.A.data(), jb.sh.data(), TP,
                               jb.ivd.data(), jb.ivb.data(), KP, jb.pai.data(), jb.z.data(), force_qr,
                               aswitch ? jb.Ae.data() : nullptr, aswitch ? jb.at.data() : nullptr);
      }
    };
    const unsigned nth = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    std::vector<std::thread> th;
    for (unsigned i = 1; i < std::min<size_t>(nth, jobs.size()); ++i) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
  }
  for (Job& jb : jobs) {
    HIPCHECK(hipMemcpy(PAI.p + (size_t)jb.c * N * KP, jb.pai.data(), (size_t)N * KP * sizeof(double),
                       hipMemcpyHostToDevice));
    st[jb.c] = (st[jb.c] & ~2) | ((jb.fl & 1) ? 1 : 0) | ((jb.fl & 2) ? 2 : 0);
    qr_count += (jb.fl & 1) ? 1 : 0;
  }
  HIPCHECK(hipMemcpy(status.p, st.data(), B * sizeof(int), hipMemcpyHostToDevice));
  run_resid();  // RESID of the redrawn coefficients for the A-step
  return (int)bad.size();
}

void ccmm_chains::sweep_once(const double* dcrn, int64_t stride, bool store) {
  const RngArgs ra = rng_args(dcrn, stride);
  snapshot_pai();
  run_cta(ra);
  cta_fallback(ra);
  if (stat_on) run_stationarity(ra);  // check_stationarity: redraw PAI while its companion's root is >= 1
  run_astep(ra);
  run_sv(ra);
  // block hybrid, N <= 32: the PHI block on the auxiliary stream beside the ELB step (the ELB kernels
  // read PAI, A, invA, sqrtht and the chain's data; PHI reads eta and writes sqrtPHI / PHI / Zphi)
  const bool fork = bh && cfg.elbTmax > 0 && d.N <= kMaxNSmall && opt[OPT_PHI_OVERLAP];
  if (fork) {
    ensure_aux();
    HIPCHECK(hipEventRecord(phiEv.fork, ctx->stream));
    HIPCHECK(hipStreamWaitEvent(aux, phiEv.fork, 0));
    run_phi(ra, aux);
    HIPCHECK(hipEventRecord(phiEv.join, aux));
    run_elb(ra, store);
    HIPCHECK(hipStreamWaitEvent(ctx->stream, phiEv.join, 0));
  } else {
    run_phi(ra);
    if (bh) run_elb(ra, store);
  }
  if (store) run_store();
  if (store && have_fcst) run_fcst(ra);
  ++sweep;
}

int ccmm_chains::check_status() {
  std::vector<int> st(d.B);
  HIPCHECK(hipMemcpy(st.data(), status.p, d.B * sizeof(int), hipMemcpyDeviceToHost));
  int any = 0;
  for (int v : st) any |= v & ~CCMM_STATUS_INFO;  // bits 1, 64: informational (valid draws)
  if (any) {
    HIPCHECK(hipMemset(status.p, 0, d.B * sizeof(int)));
    set_last_error("non positive-definite matrix in a Gibbs block (status bits " + std::to_string(any) + ")");
    return CCMM_ERR_NOTSPD;
  }
  return CCMM_OK;
}

extern "C" {

int ccmm_chains_sweep(ccmm_chains* ch, int nsweeps, const double* crn, int store) {
  return guarded([&] {
    require(ch != nullptr && nsweeps >= 0, "bad argument");
    if (!ch->have_state) {
      set_last_error("ccmm_chains_set_state must be called before sweeping");
      return CCMM_ERR_STATE;
    }
    for (int s = 0; s < ch->cfg.ndata; ++s)
      if (!ch->have_slot[s] || (ch->bh && !ch->have_elb_slot[s])) {
        set_last_error("ccmm_chains_set_data / set_elb_slot missing for a data slot");
        return CCMM_ERR_STATE;
      }
    if (ch->cfg.rng_crn) require(crn != nullptr, "chain set was created in CRN mode: crn required");
    if (ch->have_fcst && store)
      for (int s = 0; s < ch->cfg.ndata; ++s)
        if (!ch->have_fcst_slot[s]) {
          set_last_error("ccmm_chains_set_fcst_slot missing for a data slot");
          return CCMM_ERR_STATE;
        }
    HIPCHECK(hipSetDevice(ch->ctx->device));
    if (crn) {
      ch->crn.alloc((size_t)ch->d.B * nsweeps * ch->crn_len);
      HIPCHECK(hipMemcpyAsync(ch->crn.p, crn, (size_t)ch->d.B * nsweeps * ch->crn_len * sizeof(double),
                              hipMemcpyHostToDevice, ch->ctx->stream));
    }
    for (int m = 0; m < nsweeps; ++m) {
      const double* base = crn ? ch->crn.p + (size_t)m * ch->crn_len : nullptr;
      ch->sweep_once(base, (int64_t)nsweeps * ch->crn_len, store != 0);
    }
    ch->join_fcst();
    if (ch->profiling) ch->collect_profile();
    if (crn) {
      HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
      return ch->check_status();
    }
    return 0;
  });
}

int ccmm_chains_stored(const ccmm_chains* ch) { return ch ? ch->stored : -1; }

}  // extern "C"

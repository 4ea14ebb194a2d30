// The ELB step of a chain set (ccmm_chains.h): the shadow-rate model and its slots, the acceptance-sampling (PS)
// branch, the treatment of the ELB months and the speculative Gibbs step, then their entry points.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "ccmm_chains.h"

using namespace ccmm;

void ccmm_chains::init_elb() {
  const size_t B = cfg.B, N = cfg.N, Ns = cfg.Ns, ET = std::max(cfg.elbTmax, 1), nd = cfg.ndata;
  have_elb_slot.assign(nd, false);
  hSNaN.assign(nd, std::vector<uint8_t>((size_t)ET * Ns, 0));
  hNdxS.assign(Ns, 0);
  hActual.assign(N, 1);
  hElbT0.assign(nd, cfg.T);
  hElbT.assign(nd, 0);
  dNdxS.alloc(Ns);
  dActual.alloc(N);
  dElbT0.alloc(nd);
  dElbT.alloc(nd);
  dNcens.alloc(nd);
  dCens.alloc(nd * ET);
  dSNaN.alloc(nd * ET * Ns);
  HIPCHECK(hipMemset(dElbT.p, 0, nd * sizeof(int)));
  HIPCHECK(hipMemset(dNcens.p, 0, nd * sizeof(int)));
  HIPCHECK(hipMemset(dSNaN.p, 0, dSNaN.n));
  ePhi.alloc(B * N * N * cfg.p);
  eY0.alloc(B * ET * N);
  eYt.alloc(B * ET * N);
  eEt.alloc(B * ET * N);
  eCond.alloc(B * ET * (size_t)elb_cond_stride(cfg.Ns, cfg.p, ps_rec()));
  eScur.alloc(B * ET * Ns);
  HIPCHECK(hipMemset(eScur.p, 0, eScur.n * sizeof(double)));
}

ElbDev ccmm_chains::elb_view() const {
  ElbDev e{};
  e.Ns = cfg.Ns;
  e.p = cfg.p;
  e.elbTmax = std::max(cfg.elbTmax, 1);
  e.passes = cfg.elb_gibbsburn + 1;
  e.elb = cfg.elb;
  e.ndxS = dNdxS.p;
  e.actual = dActual.p;
  e.elbT0 = dElbT0.p;
  e.elbT = dElbT.p;
  e.sNaN = dSNaN.p;
  e.ncens = dNcens.p;
  e.cens = dCens.p;
  e.Xactual = Xpool.p;
  e.Phi = ePhi.p;
  e.Y0 = eY0.p;
  e.Yt = eYt.p;
  e.Et = eEt.p;
  e.cond = eCond.p;
  e.Scur = eScur.p;
  e.condStride = elb_cond_stride(cfg.Ns, cfg.p, ps_rec());
  e.kshadow = cfg.N * cfg.p + 1;
  e.K = cfg.K;
  e.mode = elb_mode;
  e.yhat = elb_yhat;
  e.flags = elb_flags;
  e.ps = 0;
  e.EtPS = eEtPS.p;
  e.psFlag = nullptr;
  e.b3 = elb_b3;
  e.Amon = elb_Amon;
  e.Afull = elb_Afull;
  e.spec = 0;
  e.psState = nullptr;
  e.psEpoch = 0;
  e.ScurSpec = nullptr;
  return e;
}

void ccmm_chains::set_elb_model(const int* ndxS, const uint8_t* actual) {
  const int N = cfg.N, Ns = cfg.Ns;
  for (int a = 0; a < Ns; ++a) {
    require(ndxS[a] >= 0 && ndxS[a] < N, "ndxS out of range");
    require(!actual[ndxS[a]], "a shadow-rate variable cannot be in the actual-rate block");
    if (a) require(ndxS[a] > ndxS[a - 1], "ndxS must be strictly increasing");
    hNdxS[a] = ndxS[a];
  }
  for (int i = 0; i < N; ++i) hActual[i] = actual[i] ? 1 : 0;
  HIPCHECK(hipMemcpy(dNdxS.p, hNdxS.data(), Ns * sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dActual.p, hActual.data(), N, hipMemcpyHostToDevice));
  have_elb_model = true;
  std::vector<int> sl(cfg.B);
  HIPCHECK(hipMemcpy(sl.data(), slot.p, cfg.B * sizeof(int), hipMemcpyDeviceToHost));
  set_slots(sl.data());
}

void ccmm_chains::set_elb_slot(int s, int elbT0, const uint8_t* sNaN) {
  const int Ns = cfg.Ns, ET = std::max(cfg.elbTmax, 1);
  const int T = hT[s];
  require(elbT0 >= 0, "elbT0 must be >= 0");
  const int elbT = std::max(0, T - elbT0);
  require(elbT <= cfg.elbTmax, "T - elbT0 exceeds elbTmax");
  std::vector<uint8_t> m((size_t)ET * Ns, 0);
  std::vector<int> cl(ET, 0);
  int nc = 0;
  for (int t = 0; t < elbT; ++t) {
    bool any = false;
    for (int a = 0; a < Ns; ++a) {
      const uint8_t v = sNaN[a + (size_t)Ns * t] ? 1 : 0;  // Ns x elbT column-major
      m[(size_t)t * Ns + a] = v;
      any |= v != 0;
    }
    if (any) cl[nc++] = t;
  }
  hElbT0[s] = elbT0;
  hElbT[s] = elbT;
  hSNaN[s] = m;
  ps_dirty = true;
  HIPCHECK(hipMemcpy(dSNaN.p + (size_t)s * ET * Ns, m.data(), m.size(), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dCens.p + (size_t)s * ET, cl.data(), ET * sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dNcens.p + s, &nc, sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dElbT0.p + s, &elbT0, sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dElbT.p + s, &elbT, sizeof(int), hipMemcpyHostToDevice));
  have_elb_slot[s] = true;
}

// ---------------------------------------------------------------- PS branch
void ccmm_chains::set_elb_ps(int np, int from_m) {
  require(np >= 0 && np <= (1 << 20), "Nproposals must be in [0, 2^20]");
  ps_np = np;
  ps_from_m = np > 0 ? from_m : -1;
  if (cfg.elbTmax > 0) {  // (no-op unless the records grow: the PS part)
    const size_t B = cfg.B, ET = std::max(cfg.elbTmax, 1);
    eCond.alloc(B * ET * (size_t)elb_cond_stride(cfg.Ns, cfg.p, ps_rec()));
  }
  ps_dirty = true;
  layout_crn();
}
void ccmm_chains::set_elb_treatment(bool missing, bool alternate, bool pair) {
  require(!(missing && alternate), "CCMM_ELB_TREAT_MISSING: alternate must be 0 (the draw is the treatment)");
  require(!alternate || cfg.model == CCMM_MODEL_BLOCKHYBRID,
          "the alternate draw is the block hybrid's (mcmcVARhybridGibbs.m:488-496 has it commented out)");
  require(!missing || elb_missing || ps_np == 0,
          "CCMM_ELB_TREAT_MISSING takes no PS proposals: call ccmm_chains_set_elb_ps(ch, 0, 0) first");
  require(stored == 0, "ccmm_chains_set_elb_treatment: call before storing draws");
  const bool was = elb_missing;
  elb_missing = missing;
  elb_alt = alternate;
  draw1_pair = pair;
  if (missing || alternate) keep_first = true;  // the draw is missingrate_all
  if (missing)
    set_elb_ps(1, 1);
  else
    set_elb_ps(was ? 0 : ps_np, was ? 0 : ps_from_m);
}
// band width of the censored-cell precision and the largest cell count over the slots
void ccmm_chains::ps_layout() {
  if (!ps_dirty) return;
  const int Ns = cfg.Ns, p = cfg.p, ET = std::max(cfg.elbTmax, 1);
  int wmax = 1, nmax = 1;
  for (int sl = 0; sl < cfg.ndata; ++sl) {
    if (!have_elb_slot[sl]) continue;
    std::vector<int> tcell;  // month of every censored cell, in cell order
    for (int t = 0; t < hElbT[sl]; ++t)
      for (int a = 0; a < Ns; ++a)
        if (hSNaN[sl][(size_t)t * Ns + a]) tcell.push_back(t);
    const int n = (int)tcell.size();
    nmax = std::max(nmax, n);
    int first = 0;  // first cell within p months before the current one
    for (int i = 0; i < n; ++i) {
      while (tcell[first] < tcell[i] - p) ++first;
      wmax = std::max(wmax, i - first + 1);
    }
  }
  require(wmax <= kPsWMax, "PS branch: censored-cell band width exceeds 80 (Ns (p + 1) too large)");
  psW = ps_band_bucket(wmax);
  ps_nmax = nmax;
  const size_t B = cfg.B;
  eEtPS.alloc(B * ET * cfg.N);
  psL.alloc(B * (size_t)nmax * psW);
  psY.alloc(B * (size_t)nmax);
  psCell.alloc(B * (size_t)nmax);
  psN.alloc(B);
  psFlag.alloc(B);
  HIPCHECK(hipMemset(psFlag.p, 0, B * sizeof(int)));
  if (!psAcc.p) {
    psAcc.alloc(B);
    std::vector<int> big(B, INT_MAX);
    HIPCHECK(hipMemcpy(psAcc.p, big.data(), B * sizeof(int), hipMemcpyHostToDevice));
  }
  if (!psCount.p) {
    psCount.alloc(2 * B);
    HIPCHECK(hipMemset(psCount.p, 0, 2 * B * sizeof(int)));
  }
  ps_dirty = false;
}
PsDev ccmm_chains::ps_view() const {
  PsDev ps{};
  ps.nmax = ps_nmax;
  ps.W = psW;
  ps.NP = ps_np;
  ps.elb = cfg.elb;
  ps.L = psL.p;
  ps.ybar = psY.p;
  ps.cell = psCell.p;
  ps.n = psN.p;
  ps.acc = psAcc.p;
  ps.flag = psFlag.p;
  ps.count = psCount.p;
  ps.per = cfg.Ns * std::max(cfg.elbTmax, 1);
  ps.first = (keep_first && !elb_missing && !elb_alt) ? psFirst.p : nullptr;  // (else: the draw's buffer)
  ps.state = psState.p;
  ps.epoch = ps_epoch;
  ps.draw1 = 0;
  ps.out = nullptr;
  return ps;
}

void ccmm_chains::run_ps(const RngArgs& ra, ElbDev& e, bool kept) {
  if (keep_first) psFirst.alloc((size_t)d.B * cfg.Ns * std::max(cfg.elbTmax, 1));
  const PsDev ps = ps_view();
  run_ps_chol(e, ps);
  if (ps.first) {  // proposal 1's uncensored cells are the window's data (the chain's current Y)
    HIPCHECK(hipMemcpyAsync(psFirst.p, e.Scur, (size_t)d.B * ps.per * sizeof(double), hipMemcpyDeviceToDevice,
                            ctx->stream));
  }
  run_ps_apply(e, ps, ra, kept, true);
  e.psFlag = psFlag.p;
}

// One unconstrained draw of the censored cells per chain from the sweep's condition records (draw1 = 1:
// the missing-data treatment, into the chain's shadow rates; 2: the alternate draw), kept in psFirst as
// the sweep's missingrate.  fused: k_ps_draw1 (W <= 64), else k_ps_chol(_w) then k_ps_apply taking
// proposal 1 unconditionally (the only form above 64; the timing probe runs both)
void ccmm_chains::run_draw1(const RngArgs& ra, const ElbDev& e, int draw1, bool fused) {
  ChainState cs = view();
  psFirst.alloc((size_t)d.B * cfg.Ns * std::max(cfg.elbTmax, 1));
  PsDev ps = ps_view();
  ps.draw1 = draw1;
  ps.out = draw1 == 1 ? e.Scur : psFirst.p;
  const size_t bytes = (size_t)d.B * ps.per * sizeof(double);
  if (draw1 == 2)  // the observed cells of missingrate are the window's data
    HIPCHECK(hipMemcpyAsync(psFirst.p, e.Scur, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if (fused && psW <= 64) {
    const int ET = std::max(cfg.elbTmax, 1);
    require(ps_draw1_lds_bytes(psW, ET, ps_nmax, ps_draw1_resident(psW, ET, ps_nmax)) <= kLdsCu,
            "PS branch: cell list does not fit LDS");
    require(ps_supported_w(psW), "PS band width");
    launch(KID_PSCHOL, [&] { HIPCHECK(launch_ps_draw1(ctx->stream, d, e, ps, cs, ra)); });
  } else {
    run_ps_chol(e, ps);
    run_ps_apply(e, ps, ra, false, false);
  }
  if (draw1 == 1)
    HIPCHECK(hipMemcpyAsync(psFirst.p, e.Scur, bytes, hipMemcpyDeviceToDevice, ctx->stream));
}

void ccmm_chains::run_ps_chol(const ElbDev& e, const PsDev& ps) {
  // register-window factorisation, one wave per chain (k_ps_chol_w), up to band width 64; option ps_chol_lds:
  // the first-generation k_ps_chol (LDS window) for every band width (same factor)
  const bool lds_window = psW > 64 || opt[OPT_PS_CHOL_LDS];
  require((lds_window ? ps_chol_lds_bytes(psW, ps_nmax) : ps_chol_w_lds_bytes(psW, e.elbTmax, ps_nmax)) <= kLdsCu,
          "PS branch: cell list does not fit LDS");
  require(ps_supported_w(psW), "PS band width");
  launch(KID_PSCHOL, [&] { HIPCHECK(launch_ps_chol(lds_window, ctx->stream, d, e, ps, view())); });
}

void ccmm_chains::run_ps_apply(const ElbDev& e, const PsDev& ps, const RngArgs& ra, bool kept, bool prop) {
  require(ps_supported_w(psW), "PS band width");
  launch(KID_PSPROP, [&] { HIPCHECK(launch_ps_apply(prop, ctx->stream, d.B, e, ps, ra, kept ? 1 : 0)); });
}

void ccmm_chains::run_elb(const RngArgs& ra, bool kept) {
  if (cfg.elbTmax <= 0) return;
  ChainState cs = view();
  ElbDev e = elb_view();
  const bool ps = ps_active() && !elb_missing;
  last_ps = ps ? 1 : 0;
  if (ps || elb_missing || elb_alt) {
    ps_layout();
    e = elb_view();
    e.ps = 1;
  }
  const int N = d.N, p = cfg.p, Ns = cfg.Ns;
  require(elb_supported_ns(Ns), "Ns must be in [1, 5]");
  const ElbPrepPlan prep = elb_prep_plan(N, p, cfg.elbTmax, d.B);
  launch(KID_ELBPREP, [&] { HIPCHECK(launch_elb_prep(ctx->stream, prep, d, e, xsel(), cs)); });
  const ElbCondPlan cond = elb_cond_plan(N, p, Ns);
  launch(KID_ELBCOND, [&] { HIPCHECK(launch_elb_cond(ctx->stream, cond, d, e, cs)); });
  // Gibbs passes: elb_waves passes in flight (k_elb_gibbs_wf, bit-identical draws), or the
  // one-wave sequential kernel (option elb_waves = 1)
  const int W = elb_gibbs_waves(e.elbTmax, Ns, opt[OPT_ELB_WAVES]);
  // eight passes in flight inside one wave (k_elb_gibbs_oct, bit-identical draws): the default;
  // option elb_oct = 0 selects the wave kernels
  // (the per-chain wave kernels keep shorter months at B < kElbOctMinB: one wave per chain cannot
  // fill the chip there, and a month costs the octet kernel more latency)
  const int elb_oct = opt[OPT_ELB_OCT];
  const bool use_oct =
      elb_oct && elb_oct_lds_bytes(e.elbTmax, Ns) <= kLdsCu && (elb_oct == 2 || d.B >= kElbOctMinB);
  // (option ps_chol_lds selects k_ps_chol, which only the unfused pair can run)
  if (elb_missing) run_draw1(ra, e, 1, !draw1_pair && !opt[OPT_PS_CHOL_LDS]);
  // speculative Gibbs step (option elb_spec, small B): the asynchronous wave kernels start beside the PS
  // branch on a stream of their own and stop once it accepts; the draw is kept only for a rejected PS
  // (the reference's order and draws: PS first, the Gibbs draw the fallback, :438-466)
  const bool spec = ps && opt[OPT_ELB_SPEC] && d.B <= kElbMpMaxB && !use_oct && W > 1 && opt[OPT_ELB_ASYNC] &&
                    elb_flags == nullptr;
  hipStream_t gst = ctx->stream;
  if (spec) {
    if (!aux2) HIPCHECK(hipStreamCreateWithFlags(&aux2, hipStreamNonBlocking));
    specEv.ensure();
    if (!psState.p) {
      psState.alloc(d.B);
      HIPCHECK(hipMemsetAsync(psState.p, 0, d.B * sizeof(unsigned long long), ctx->stream));
    }
    HIPCHECK(hipEventRecord(specEv.fork, ctx->stream));
    HIPCHECK(hipStreamWaitEvent(aux2, specEv.fork, 0));
    gst = aux2;
    eScurSpec.alloc(eScur.n);
    e.spec = 1;
    e.psState = psState.p;
    e.psEpoch = ++ps_epoch;
    e.ScurSpec = eScurSpec.p;
  } else if (ps) {
    run_ps(ra, e, kept);
  }
  if (!elb_missing) {  // (missing-data treatment: no Gibbs kernel, the draw is the data, :498)
    // the wavefront over 2 or 4 CUs per chain at small B (k_elb_gibbs_mp, bit-identical draws)
    const int parts = use_oct ? 1 : elb_parts(W);
    ElbXch xc{nullptr, 0};
    if (parts > 1) {
      elbXch.alloc((size_t)d.B * parts * e.elbTmax * Ns * 2);
      if (elbXchZeroed != elbXch.p) {  // tags start at zero (tags of a launch are >= 2^16)
        HIPCHECK(hipMemsetAsync(elbXch.p, 0, elbXch.n * sizeof(double), ctx->stream));
        elbXchZeroed = elbXch.p;
      }
      xc = ElbXch{elbXch.p, ++elb_epoch};
    }
    const ElbGibbsPlan gibbs{use_oct ? kElbGibbsOct : parts > 1 ? kElbGibbsMp : W > 1 ? kElbGibbsWf : kElbGibbsSeq, W,
                             opt[OPT_ELB_ASYNC] != 0, parts};
    launch(KID_ELBGIBBS, [&] { HIPCHECK(launch_elb_gibbs(gst, gibbs, d, e, cs, ra, xc)); }, gst);
  }
  if (spec) {  // the PS branch beside the Gibbs passes; k_ps_apply posts the decision they wait on
    ElbDev ep = e;
    ep.spec = 0;
    run_ps(ra, ep, kept);
    HIPCHECK(hipEventRecord(specEv.join, aux2));
    HIPCHECK(hipStreamWaitEvent(ctx->stream, specEv.join, 0));
    ep.spec = 1;  // (ep.psFlag: set by run_ps)
    HIPCHECK(launch_elb_spec_select(ctx->stream, ep, slot.p, d.B));
  }
  // the alternate draw (:470-475): this sweep's precision and linear term (the condition records above,
  // which hold the observed data only), into the missingrate buffer alone
  if (elb_alt) run_draw1(ra, e, 2, !opt[OPT_PS_CHOL_LDS]);
  launch(KID_ELBREBUILD, [&] {
    HIPCHECK(launch_elb_rebuild(ctx->stream, d, e, xsel(), cs, cfg.ndata, lag_capable ? Dpool.p : nullptr, ldd, drows,
                                colx_capable ? Dcpool.p : nullptr, dcld, (long long)dcslab));
  });
  resid_valid = false;  // X, Y changed: RESID is recomputed before the next CTA
}

// workgroups (CUs) per chain of the ELB wavefront: k_elb_gibbs_mp spreads the W = 8 passes in flight
// over 2 (or 4) CUs at small B, one drawing wave per SIMD, when every chain's parts can be resident
// together (option elb_parts; auto: 2 for B <= kElbMpMaxB)
int ccmm_chains::elb_parts(int W) {
  const int o = opt[OPT_ELB_PARTS];
  if (W != 8 || !opt[OPT_ELB_ASYNC] || o == 1 || cfg.elb_gibbsburn + 1 >= 65535) return 1;
  const int parts = o == 0 ? (d.B <= kElbMpMaxB ? 2 : 1) : (o >= 4 ? 4 : 2);
  if (parts == 1) return 1;
  int cus = 0;
  HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  // one workgroup of <= 384 threads per part, <= 110 KB of LDS: at least one per CU is resident
  return (d.B * parts <= cus) ? parts : 1;
}

extern "C" {

int ccmm_chains_record_elb_flags(ccmm_chains* ch, int enable) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->bh, "chain set was not created with CCMM_MODEL_BLOCKHYBRID / CCMM_MODEL_HYBRID");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    if (enable) {
      ch->dElbFlags.alloc((size_t)ch->d.B * (ch->cfg.elb_gibbsburn + 1) * std::max(ch->cfg.elbTmax, 1) *
                          ch->cfg.Ns);
      HIPCHECK(hipMemset(ch->dElbFlags.p, 0, ch->dElbFlags.n));
      ch->elb_flags = ch->dElbFlags.p;
    } else {
      ch->elb_flags = nullptr;
    }
    return 0;
  });
}

int ccmm_chains_get_elb_flags(ccmm_chains* ch, uint8_t* flags) {
  return guarded([&] {
    require(ch && flags, "null argument");
    require(ch->elb_flags != nullptr, "ccmm_chains_record_elb_flags(ch, 1) was not called");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    HIPCHECK(hipMemcpy(flags, ch->dElbFlags.p, ch->dElbFlags.n, hipMemcpyDeviceToHost));
    return 0;
  });
}

int ccmm_chains_set_elb_model(ccmm_chains* ch, const int* ndxS, const uint8_t* actual_block) {
  return guarded([&] {
    require(ch && ndxS, "null argument");
    require(ch->bh, "chain set was not created with CCMM_MODEL_BLOCKHYBRID / CCMM_MODEL_HYBRID");
    const bool no_block = ch->hybrid || ch->cfg.model == CCMM_MODEL_SHADOWRATE;
    require(actual_block || no_block, "null argument");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    std::vector<uint8_t> none(ch->cfg.N, 0);
    if (no_block) {
      for (int i = 0; actual_block && i < ch->cfg.N; ++i)
        require(!actual_block[i], "hybrid / shadow-rate model has no actual-rate block (pass NULL or zeros)");
      actual_block = none.data();
    }
    ch->set_elb_model(ndxS, actual_block);
    return 0;
  });
}

int ccmm_chains_set_elb_slot(ccmm_chains* ch, int slot, int elbT0, const uint8_t* sNaN) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->bh, "chain set was not created with CCMM_MODEL_BLOCKHYBRID");
    require(slot >= 0 && slot < ch->cfg.ndata, "slot out of range");
    require(ch->have_slot[slot], "ccmm_chains_set_data must be called before set_elb_slot");
    require(sNaN != nullptr || ch->hT[slot] <= elbT0, "null sNaN");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    ch->set_elb_slot(slot, elbT0, sNaN);
    return 0;
  });
}

int ccmm_chains_set_elb_ps(ccmm_chains* ch, int nproposals, int ps_from_m) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->bh, "chain set was not created with CCMM_MODEL_BLOCKHYBRID / CCMM_MODEL_HYBRID");
    require(nproposals == 0 || ps_from_m >= 1, "ps_from_m must be >= 1");
    require(!ch->elb_missing || nproposals == 0,
            "CCMM_ELB_TREAT_MISSING takes no PS proposals (ccmm_chains_set_elb_treatment)");
    if (ch->elb_missing) return 0;  // (the treatment's own single draw stays configured)
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    ch->set_elb_ps(nproposals, ps_from_m);
    return 0;
  });
}

int ccmm_chains_set_elb_treatment(ccmm_chains* ch, int treatment, int alternate) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->bh, "chain set has no ELB step (block-hybrid, hybrid and shadow-rate models only)");
    require(treatment == CCMM_ELB_TREAT_SHADOW || treatment == CCMM_ELB_TREAT_MISSING ||
                treatment == CCMM_ELB_TREAT_MISSING_PAIR,
            "unknown ELB treatment");
    require(alternate == 0 || alternate == 1, "alternate must be 0 or 1");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    ch->set_elb_treatment(treatment != CCMM_ELB_TREAT_SHADOW, alternate != 0,
                          treatment == CCMM_ELB_TREAT_MISSING_PAIR);
    return 0;
  });
}

int ccmm_ps_draw1_resident(int W, int elbTmax, int nmax) {
  return guarded([&] {
    require(W == 16 || W == 32 || W == 48 || W == 64, "W must be 16, 32, 48 or 64");
    require(elbTmax >= 0 && nmax >= 0, "negative size");
    return ps_draw1_resident(W, elbTmax, nmax);
  });
}

int ccmm_chains_get_ps(ccmm_chains* ch, int* countAccept, int* countAcceptBurnin, int* stackAccept) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->ps_np > 0, "ccmm_chains_set_elb_ps was not called");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const size_t B = ch->cfg.B, cap = ch->cfg.store_capacity, M = ch->stored;
    std::vector<int> cnt(2 * B, 0);
    if (ch->psCount.p) HIPCHECK(hipMemcpy(cnt.data(), ch->psCount.p, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < B; ++c) {
      if (countAcceptBurnin) countAcceptBurnin[c] = cnt[2 * c];
      if (countAccept) countAccept[c] = cnt[2 * c + 1];
    }
    if (stackAccept && M) {
      std::vector<int> buf(B * cap, 0);
      if (ch->sAccept.p) HIPCHECK(hipMemcpy(buf.data(), ch->sAccept.p, buf.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (size_t c = 0; c < B; ++c)
        for (size_t m = 0; m < M; ++m) stackAccept[m + M * c] = buf[c * cap + m];
    }
    return 0;
  });
}

int ccmm_chains_keep_missingrate(ccmm_chains* ch, int enable) {
  return guarded([&] {
    require(ch != nullptr, "null argument");
    require(ch->bh, "chain set has no ELB step (shadow-rate models only)");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    require(ch->stored == 0, "ccmm_chains_keep_missingrate: call before storing draws");
    ch->keep_first = enable != 0;
    return 0;
  });
}

int ccmm_chains_get_missingrate(ccmm_chains* ch, double* missingrate_all) {
  return guarded([&] {
    require(ch && missingrate_all, "null argument");
    require(ch->keep_first, "ccmm_chains_keep_missingrate was not enabled");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const size_t B = ch->cfg.B, cap = ch->cfg.store_capacity, M = ch->stored;
    const size_t per = (size_t)ch->cfg.Ns * ch->cfg.elbTmax;
    if (M == 0 || per == 0) return 0;
    std::vector<double> buf(B * cap * per);
    HIPCHECK(hipMemcpy(buf.data(), ch->sMissing.p, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < B; ++c)
      for (size_t m = 0; m < M; ++m)
        for (size_t e = 0; e < per; ++e) missingrate_all[m + M * (e + per * c)] = buf[(c * cap + m) * per + e];
    return 0;
  });
}

int ccmm_chains_get_ps_mean(ccmm_chains* ch, double* mean) {
  return guarded([&] {
    require(ch && mean, "null argument");
    require(ch->ps_np > 0 && ch->psL.p, "ccmm_chains_set_elb_ps was not called or no PS sweep ran");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    const size_t B = ch->cfg.B, nmax = ch->ps_nmax, W = ch->psW, per = (size_t)ch->cfg.Ns * ch->cfg.elbTmax;
    std::vector<double> L(B * nmax * W), yb(B * nmax);
    std::vector<int> cell(B * nmax), n(B);
    HIPCHECK(hipMemcpy(L.data(), ch->psL.p, L.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(yb.data(), ch->psY.p, yb.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(cell.data(), ch->psCell.p, cell.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(n.data(), ch->psN.p, n.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < B; ++c) {
      double* o = mean + c * per;
      for (size_t q = 0; q < per; ++q) o[q] = std::nan("");
      const double* Lc = L.data() + c * nmax * W;
      std::vector<double> x(n[c], 0.0);
      for (int i = n[c] - 1; i >= 0; --i) {  // x = L'^-1 ybar, band storage L(i + j, i) at [i][j]
        double v = yb[c * nmax + i];
        for (size_t j = 1; j < W && i + (int)j < n[c]; ++j) v -= Lc[(size_t)i * W + j] * x[i + j];
        x[i] = v / Lc[(size_t)i * W];
        o[cell[c * nmax + i]] = x[i];
      }
    }
    return 0;
  });
}

int ccmm_chains_get_shadowrate(ccmm_chains* ch, double* shadowrate) {
  return guarded([&] {
    require(ch && shadowrate, "null argument");
    require(ch->bh, "chain set was not created with CCMM_MODEL_BLOCKHYBRID");
    HIPCHECK(hipSetDevice(ch->ctx->device));
    HIPCHECK(hipStreamSynchronize(ch->ctx->stream));
    if (ch->cfg.elbTmax > 0)
      HIPCHECK(hipMemcpy(shadowrate, ch->eScur.p,
                         (size_t)ch->d.B * ch->cfg.Ns * ch->cfg.elbTmax * sizeof(double),
                         hipMemcpyDeviceToHost));
    return 0;
  });
}

}  // extern "C"

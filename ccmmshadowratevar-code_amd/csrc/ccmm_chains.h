// A device-resident chain set (ccmm_chains of include/ccmm.h): every member, block by block, and the
// methods' declarations.  The bodies are in the unit of their block: ccmm_chains.hip (set-up, data, state,
// exports, profile), ccmm_chains_sweep.hip (the Gibbs blocks of a sweep), ccmm_chains_elb.hip (ELB step,
// PS branch, treatment), ccmm_chains_fcst.hip (predictive density, summaries), ccmm_chains_eig.hip (maximum VAR
// roots, check_stationarity), ccmm_chains_diag.hip (Compute_diagnostics of the stored draws), ccmm_chains_vma.hip
// (impulse responses of the stored draws and their summaries), ccmm_chains_condmean.hip (conditional mean paths of
// the stored draws), ccmm_chains_girf.hip (generalized impulse responses of the stored draws).
#pragma once
#include "ccmm_host.h"
#include "ccmm_sweep.h"
#include "ccmm_elb.h"
#include "ccmm_lag.h"
#include "ccmm_big.h"
#include "ccmm_eig.h"

// hidden: the methods are called across the host units only, never from outside the library, so the calls
// bind at link time as they did inside one unit (no procedure-linkage stub, no lazy lookup at a first call)
struct __attribute__((visibility("hidden"))) ccmm_chains {
  ccmm_ctx* ctx = nullptr;
  ccmm_chain_config cfg{};
  ccmm::Dims d{};
  ccmm::Options opt;  // kernel forms and schedules (ccmm_chains_set_option), from the context at create

  // ---------------------------------------------------------------- data slots
  int nslabX = 0, nslabY = 0;
  std::vector<int> hT;
  std::vector<bool> have_slot;
  DBuf<int> Tslot, slot, xidx, yidx, status;
  DBuf<double> Xpool, Ypool, iVdiag, iVb, sPHI, V0inv, V0invm;

  // ---------------------------------------------------------------- chain state
  DBuf<double> PAI, A, invA, sqrtht, h, h0, sqrtPHI, PHI, E, logy2, eta, svobs, svir, W, ih2;
  DBuf<int8_t> kai;
  DBuf<double> G, rdiag, svLd, svw, svSep, svG, Zphi;
  DBuf<double> crn;
  int64_t crn_off[ccmm::kRngBlocks] = {};
  int64_t crn_len = 0;
  uint32_t sweep = 0;
  bool resid_valid = false;
  bool have_state = false;
  // Philox stream ids (counter word 1) per chain; default the chain index
  bool have_ids = false;
  DBuf<uint32_t> rngIds;
  // CTAsysAswitching (block-level drop-in only): second A matrix for the months at the ELB
  bool aswitch = false;
  DBuf<double> AelbD;
  DBuf<uint8_t> atELBD;
  // timing-only ablation of k_gram_chol (results invalid): the kGc* bits of ccmm_sweep.h
  int gc_mode = ccmm::env_ablation("CCMM_GC_MODE", 0);
  // the kSv* bits of ccmm_svpart.h (phase skips, timing-only bits, kSvFullRows): ablation build only
  int sv_mode = ccmm::env_ablation("CCMM_SV_MODE", 0);
  int mfma_lock = 0;  // MFMA phase lock id (ccmm_chains_set_mfma_lock) and the set's event in it
  hipEvent_t mfma_ev = nullptr;

  // ---------------------------------------------------------------- draw store
  int stored = 0;
  DBuf<double> sPAI, sPHI_, sInvA, sSqrtht, sShadow;
  DBuf<double> paiMom;  // running PAI sums | sums of squares (ccmm_chains_pai_moments)
  int mom_done = 0;     // stored draws already added to paiMom

  // ---------------------------------------------------------------- lag design
  // lag-structured design (ccmm_lag.hip): D slabs parallel to the X slabs
  bool lag_capable = false;
  int lagNT = 0, ldd = 0, drows = 0;
  std::vector<bool> slot_lag;
  DBuf<double> Dpool;
  DBuf<int> dColmap, astepTab;
  int lag_mode = ccmm::env_ablation("CCMM_LAG_MODE", 0);
  DBuf<double> solveXch;  // k_cta_solve_lag split: X'v half partials (SolveXch)
  DBuf<uint64_t> solveFlag;
  uint64_t solve_epoch = 0;
  int split_resident = -1;  // workgroups of the split solve resident at once (-1: not asked yet)

  // ---------------------------------------------------------------- lag twin
  // large path: column-major lag twin of every X slab (ccmm_big.h ColX), when each slab's X is
  // [1, lags 1..p of N (+ Ns) data columns]; k_elb_rebuild keeps the chains' twins current
  bool colx_capable = false;
  std::vector<bool> slot_colx;
  DBuf<double> Dcpool;
  DBuf<int> dXoff;
  int dcld = 0, dcext = 0;
  size_t dcslab = 0;

  // ---------------------------------------------------------------- large path
  // large-system CTA (ccmm_big.hip): K > 256 or N > 32, or option large_path
  bool big = false;
  int nGroups = 0;
  DBuf<int4> bigGroups;
  DBuf<double> Ubuf, Dinv, bigW, bigScr;
  int big_mask = ccmm::env_ablation("CCMM_BIG_MASK", ccmm::kBigAll);

  // ---------------------------------------------------------------- ELB model
  // block-hybrid ELB model (mcmcVARshadowrateBlockHybrid.m): X/Y slabs 0..ndata-1 hold
  // the vintages' actual data, slabs ndata + c the chain's shadow-rate data
  bool bh = false;
  // hybrid model (mcmcVARhybridGibbs.m): same chain layout as bh, one design per chain
  // (CTA, no actual-rate block), trailing columns = censored actual-rate lags
  bool hybrid = false;
  bool fcst_bh = false;  // block-hybrid companion in the predictive density (k_fcst a.bh)
  bool have_elb_model = false;
  std::vector<bool> have_elb_slot;
  std::vector<int> hNdxS, hElbT0, hElbT;
  std::vector<uint8_t> hActual;
  DBuf<int> dNdxS, dElbT0, dElbT, dNcens, dCens;
  DBuf<uint8_t> dActual, dSNaN;
  DBuf<double> ePhi, eY0, eYt, eEt, eCond, eScur;
  std::vector<std::vector<uint8_t>> hSNaN;  // per slot, elbTmax x Ns (t-major)
  const double* elb_yhat = nullptr;  // ccmm_gibbs_shadowrates: explicit YHAT0
  int elb_b3 = 0;                    // ccmm_gibbs_shadowrates_b3: no Y0 path, intercept in the state
  const double* elb_Amon = nullptr;  // ccmm_gibbs_shadowrates_b3: per-month structural matrices
  int elb_Afull = 0;                 // ccmm_gibbs_shadowrates*: A = inverse of a general impact matrix
  uint8_t* elb_flags = nullptr;      // drawTruncNormal branch flags of the last ELB step (or nullptr)
  DBuf<uint8_t> dElbFlags;
  // timing-only ablation of the ELB Gibbs kernels (results invalid): the kElb* bits of ccmm_elb.h
  int elb_mode = ccmm::env_ablation("CCMM_ELB_MODE", 0);
  DBuf<double> elbXch;  // k_elb_gibbs_mp exchange between a chain's parts, tagged by elb_epoch
  const double* elbXchZeroed = nullptr;
  unsigned long long elb_epoch = 0;

  // ---------------------------------------------------------------- PS / treatment
  // acceptance-sampling branch (ccmm_ps.hip): ps_np proposals per sweep from sweep
  // m = ps_from_m on (1-based, m = sweep + 1; the reference: m >= MCMCburnin/2, :435)
  int ps_np = 0, ps_from_m = -1, psW = 0, ps_nmax = 0;
  bool ps_dirty = true;
  // treatment of the ELB months (ccmm_chains_set_elb_treatment): elb_missing = every sweep takes one
  // unconstrained draw as the data (held as ps_np = 1 from sweep 1: the CRN record and the condition
  // records of set_elb_ps(1, .)); elb_alt = one more such draw per sweep, kept as missingrate only
  bool elb_missing = false, elb_alt = false;
  DBuf<double> eEtPS, psL, psY;
  DBuf<int> psCell, psN, psAcc, psFlag, psCount, sAccept;
  // missingrate_all (mcmcVARshadowrate.m:435, 498; mcmcVARhybridGibbs.m:486): keep proposal 1 of
  // every PS sweep in the draw store (ccmm_chains_keep_missingrate)
  bool keep_first = false;
  bool draw1_pair = false;  // CCMM_ELB_TREAT_MISSING_PAIR: the draw by k_ps_chol_w + k_ps_apply (timing)
  DBuf<double> psFirst, sMissing;
  int last_ps = 0;  // whether the last ELB step ran the PS branch (draw store bookkeeping)

  // ---------------------------------------------------------------- speculative step
  DBuf<unsigned long long> psState;  // PS decision per chain: ps_epoch << 1 | accepted (k_ps_apply)
  DBuf<double> eScurSpec;            // the speculative Gibbs draw (k_elb_spec_select)
  unsigned long long ps_epoch = 0;

  // ---------------------------------------------------------------- forecasts
  // predictive density of every stored sweep (mcmcVAR.m:298-381,
  // mcmcVARshadowrateBlockHybrid.m:550-669), kept on the device
  bool have_fcst = false;
  int fH = 0, fNd = 0, fKeep = 0, fstored = 0, fldXj = 0;
  DBuf<uint8_t> fYields, fRecFloor;
  bool have_rec_floor = false;
  std::vector<bool> have_fcst_slot;
  DBuf<double> fYreal, fXj, fY, fYc, fYhat, fSc, fYsum, fYcsum, fYhatsum, fScStore, fPaths, fPathsC, fSv1;
  DBuf<int> fStatus;
  // doIRF1 (ccmm_chains_set_irf1): the plus / minus simulations of every kept draw beside its predictive density.
  // fY1p / fY1m: the kept draw's raw paths; fIrfP / fIrfM: [B][cap][H][N] IRF1drawsPlus / Minus; fY1sumP / M:
  // [B][H][N] running sums of the floored (and cumulated) paths; fIrfTmp: k_fcst_irf_accum's scratch;
  // fPathsP / M: the raw paths of every kept draw (keep_paths)
  bool have_irf = false;
  double irfScale = 0.0;
  DBuf<uint8_t> fIrfCum;
  DBuf<double> fY1p, fY1m, fIrfP, fIrfM, fY1sumP, fY1sumM, fIrfTmp, fPathsP, fPathsM;
  // the predictive density of a kept sweep on the auxiliary stream (option fcst_overlap, N <= 32): it reads
  // the sweep's PAI, invA, h, sqrtPHI and the chain's Y, which the next sweep first rewrites in its CTA
  // solve (PAI), so it runs beside the next sweep's residual, weights and Gram + Cholesky; join_fcst()
  // orders the solve (and the end of every ccmm_chains_sweep call) after it.  Same kernels, same inputs.
  bool fcst_pending = false;

  // ---------------------------------------------------------------- post-processing scratch
  // summaries over the kept draws of the chains of one data slot (ccmm_post.hip)
  DBuf<double> postA, postB, postOut;
  DBuf<char> postWs;
  DBuf<int> postRows;
  DBuf<uint8_t> postCum, postFlo;

  // ---------------------------------------------------------------- QR fallback
  // CTA.m:80-92: a chain whose coefficient block met a non-positive Cholesky pivot
  // (status bit 2) is redrawn on the host (host_cta_chain: Cholesky, or the Householder QR
  // of Kailath's array where it fails) from the same previous draw and normals; status
  // bit 2 is then replaced by bit 1 ("QR fallback used", informational).  Option force_qr routes
  // every chain through the host QR branch (tests); qr_fallback = 0 disables the check.
  DBuf<double> paiPrev, zHost;
  int64_t qr_count = 0;

  // ---------------------------------------------------------------- maximum VAR root / stationarity
  // ccmm_chains_eig.hip: roots of the stored draws (ccmm_chains_max_var_roots) and check_stationarity
  // (mcmcVAR.m:221-232): after the coefficient block of a sweep the roots of the B new PAI, and while a
  // chain's root is >= 1 the block again for the whole set with the attempt's normals (RngArgs::attempt),
  // the accepted chains' PAI, E and status put back from a snapshot (k_stat_select)
  bool stat_on = false;
  int stat_max = 1000;
  std::vector<int64_t> statRedraws;
  DBuf<double> eigRoot, eigScr, statPAI, statE;
  DBuf<int> eigInfo, statAcc, statStatus;

  // ---------------------------------------------------------------- diagnostics
  // ccmm_chains_diag.hip: the 11 statistics of every stored series of one slot, the mask of the entries that
  // are computed (sqrtht rows of the slot's T) and the per-chain entry counts (shadow rates within elbT)
  DBuf<double> diagOut;
  DBuf<uint8_t> diagMask;
  DBuf<int> diagCnt;

  // ---------------------------------------------------------------- impulse responses
  // ccmm_chains_vma.hip: the draw-major responses of one horizon slab (k_vma) and the screen's flag per draw;
  // the segments and the sorted copy are postA / postB
  DBuf<double> vmaBuf;
  DBuf<int> vmaInfo;

  // ---------------------------------------------------------------- conditional mean paths
  // ccmm_chains_condmean.hip: the jump-off state, the mean of every stored draw (k_cond_mean) and the screen's flag
  DBuf<double> cmY0, cmMean;
  DBuf<int> cmInfo;

  // ---------------------------------------------------------------- profiling
  bool profiling = false;
  struct Ev {
    int kid;
    hipEvent_t a, b;
  };
  std::vector<Ev> pending;
  std::vector<hipEvent_t> evpool;
  double kms[KID_COUNT] = {};
  int64_t kcount[KID_COUNT] = {};

  // ---------------------------------------------------------------- streams
  // auxiliary stream of the sweep: the inverse-Wishart block runs on it beside the ELB step, which
  // reads none of its inputs or outputs (mcmcVARshadowrateBlockHybrid.m:386-392 vs :395-520); the
  // main stream waits for it before the draw store, the forecasts and the next sweep's SV block
  hipStream_t aux = nullptr;
  hipStream_t aux2 = nullptr;  // the speculative Gibbs step's stream
  // fork / join events of the PHI block (aux), the speculative Gibbs step (aux2), the forecasts (aux)
  EventPair phiEv, specEv, fcstEv;

  // ================================================================ ccmm_chains.hip
  ~ccmm_chains();
  void init(ccmm_ctx* c, const ccmm_chain_config& cf, int nX, int nY);
  void layout_crn();
  void init_lag(int nX);
  void init_colx();
  void try_upload_D(int slot, int T, const double* Y, const double* X);
  void try_upload_Dc(int slot, int T, const double* X);
  bool lag_active() const;
  void reset_chain_slabs();
  void set_slots(const int* sl);
  void build_groups(const std::vector<int>& xi);
  void upload_X(int slab, int T, const double* X);  // X: T x K column-major
  void upload_TN(double* dst, int nmat, int T, const double* src, double pad);
  void download_TN(const double* srcd, int nmat, int T, double* dst);
  void upload_KN(double* dst, int nmat, const double* src, double pad);
  void download_KN(const double* srcd, int nmat, double* dst);
  void set_slot_prior(int s, const double* iVd, const double* ivb, const double* sP, const double* h0mean,
                      const double* h0vcvsqrt);
  void set_slot_h0(int s, const double* h0mean, const double* h0vcvsqrt);
  void set_T(int s, int T);
  ccmm::ChainState view();
  void export_lag_gram(const char* inactive, int mode);
  void export_cta_gram(double* out);
  void export_cta_factor(double* out);
  void ensure_aux();
  hipEvent_t get_event();
  void collect_profile();
  ccmm::XSel xsel() const { return ccmm::XSel{Xpool.p, xidx.p, Ypool.p, yidx.p}; }
  ccmm::LagSel lagsel() const { return ccmm::LagSel{Dpool.p, xidx.p, dColmap.p, ldd, drows, cfg.p, lag_mode}; }
  ccmm::ColX colx() const {
    bool on = colx_capable && opt[ccmm::OPT_BIG_LAGX];
    for (int s = 0; on && s < cfg.ndata; ++s) on = slot_colx[s];
    return on ? ccmm::ColX{Dcpool.p, dXoff.p, (long long)dcslab, dcld, (int)(dcslab / dcld)}
              : ccmm::ColX{nullptr, nullptr, 0, 0, 0};
  }
  // one launch (or group of launches) under the profile's event pair when profiling is on
  template <class L>
  void launch(int kid, L&& fn, hipStream_t on = nullptr) {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st = on ? on : ctx->stream;
    if (profiling) {
      a = get_event();
      b = get_event();
      HIPCHECK(hipEventRecord(a, st));
    }
    fn();
    HIPCHECK(hipGetLastError());
    if (profiling) {
      HIPCHECK(hipEventRecord(b, st));
      pending.push_back({kid, a, b});
    }
  }

  // ================================================================ ccmm_chains_sweep.hip
  ccmm::RngArgs rng_args(const double* dcrn, int64_t stride) const;
  void ensure_cta();
  void run_resid();
  void run_weights(const ccmm::ChainState& cs, int sqrt_form);
  void run_cta(const ccmm::RngArgs& ra);
  void run_astep_big(const ccmm::RngArgs& ra);
  void run_cta_big(const ccmm::RngArgs& ra, const ccmm::ChainState& cs);
  bool solve_split_ok();
  void run_cta_lag(const ccmm::RngArgs& ra, const ccmm::ChainState& cs);
  void run_astep(const ccmm::RngArgs& ra);
  void ensure_sv();
  void run_sv(const ccmm::RngArgs& ra);
  void run_phi(const ccmm::RngArgs& ra, hipStream_t on = nullptr);
  void run_store();
  void snapshot_pai();
  int cta_fallback(const ccmm::RngArgs& ra);  // returns the chains redrawn
  void sweep_once(const double* dcrn, int64_t stride, bool store);
  int check_status();

  // ================================================================ ccmm_chains_elb.hip
  void init_elb();
  ccmm::ElbDev elb_view() const;
  void set_elb_model(const int* ndxS, const uint8_t* actual);
  void set_elb_slot(int s, int elbT0, const uint8_t* sNaN);
  void set_elb_ps(int np, int from_m);
  void set_elb_treatment(bool missing, bool alternate, bool pair);
  void ps_layout();
  ccmm::PsDev ps_view() const;
  bool ps_rec() const { return ps_np > 0 || elb_alt; }  // the condition records carry the PS part
  bool ps_active() const { return ps_np > 0 && ps_from_m > 0 && (int64_t)sweep + 1 >= ps_from_m; }
  void run_ps(const ccmm::RngArgs& ra, ccmm::ElbDev& e, bool kept);
  void run_draw1(const ccmm::RngArgs& ra, const ccmm::ElbDev& e, int draw1, bool fused);
  void run_ps_chol(const ccmm::ElbDev& e, const ccmm::PsDev& ps);
  void run_ps_apply(const ccmm::ElbDev& e, const ccmm::PsDev& ps, const ccmm::RngArgs& ra, bool kept, bool prop);
  void run_elb(const ccmm::RngArgs& ra, bool kept);
  int elb_parts(int W);

  // ================================================================ ccmm_chains_fcst.hip
  void set_fcst(int H, int Nd, const uint8_t* ndxYields, int keep);
  void set_irf1(double scale, const uint8_t* cumcode);
  void reset_fcst();
  void run_fcst(const ccmm::RngArgs& ra);
  void join_fcst();
  void summaries(int source, int sl, const uint8_t* rows, const uint8_t* cumcode, const uint8_t* flo, double fl,
                 const double* realized, int nq, const double* pct, double* mean, double* median, double* quant,
                 double* sdev, double* crps);

  // ================================================================ ccmm_chains_eig.hip
  void run_stationarity(const ccmm::RngArgs& ra);
};

// max |eig| of M companions whose PAI are on the device (src: ccmm_eig.h EigSrc), results on the host: the
// device kernel for N p <= kEigMaxN, the host twin for larger orders and for the matrices with info = 2.
// root / info / scr: the caller's device buffers, grown as needed.  info may be null.  (ccmm_chains_eig.hip)
void max_var_root_device_src(ccmm_ctx* ctx, int M, int N, int p, const ccmm::EigSrc& src, DBuf<double>& root,
                             DBuf<int>& finfo, DBuf<double>& scr, double* maxroot, int* info);

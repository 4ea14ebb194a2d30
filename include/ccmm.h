/*
 * ccmm.h — C ABI of libccmm, the MI355X-native Gibbs sweep of the CCMM
 * shadow-rate BVAR-SV (Carriero, Clark, Marcellino & Mertens).
 *
 * Drop-in boundary.  Each entry point replaces one MATLAB function (or loop)
 * of the reference (Allisterh/CCMMshadowrateVAR-code @ 2025-01-27); the
 * reference file:line it replaces is cited beside it.  The MATLAB signatures
 * stay unchanged: a MEX gateway marshals mxArrays into these
 * calls.  Plain C types only: pointers to column-major fp64 host arrays
 * (MATLAB layout), int sizes, and opaque handles.
 *
 * Conventions
 *  - Every matrix argument is column-major, exactly the MATLAB array shape
 *    quoted in the comment ("T x N" means T rows, N columns).  Batched
 *    arguments append the chain index as the slowest dimension ("x B").
 *  - Return codes: 0 = OK; > 0 = warning (mirrors MATLAB warning(): e.g.
 *    CCMM_WARN_QR_FALLBACK, CTA.m:82); < 0 = error (mirrors error(): e.g.
 *    CCMM_ERR_DIM, gibbsdrawShadowrates.m:51).  ccmm_last_error() returns a
 *    thread-local message for the last non-zero return on this thread.
 *  - Host buffers belong to the caller and are never freed by the library.
 *    Device buffers, RNG state and scratch belong to the context / chain set.
 *  - Reentrancy: one context is bound to one device and serialises its calls
 *    on its own HIP stream; distinct contexts may be driven from distinct
 *    threads or processes (one per GPU).
 *  - Random numbers: every drawing entry point takes either a CRN array (the
 *    host-injected common random numbers, in the reference's draw order and
 *    shape) or NULL, in which case the library draws from its counter-based
 *    Philox4x32-10 generator keyed by (seed, chain, sweep, block).
 */
#ifndef CCMM_H
#define CCMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCMM_ABI_VERSION 4  /* 4: ccmm_batch_out.shadowratePSRFchains, kernel options, status bit 64 */

/* return codes */
#define CCMM_OK 0
#define CCMM_WARN_QR_FALLBACK 1    /* CTA.m:80-92 "switching to QR routine" */
#define CCMM_WARN_ELBT0 2          /* mcmcVARshadowrateBlockHybrid.m:203-205 */
#define CCMM_WARN_MVNCDF 3         /* censored log score with more than 12 series at the ELB: score NaN (4..12: deterministic lattice estimate inside MATLAB mvncdf's QMC tolerance 1e-4) */
#define CCMM_ERR_DIM (-1)          /* gibbsdrawShadowrates.m:50-52 "dimension mismatch" */
#define CCMM_ERR_ARG (-2)          /* invalid argument / unsupported size */
#define CCMM_ERR_HIP (-3)          /* HIP runtime failure */
#define CCMM_ERR_NOTSPD (-4)       /* Cholesky failure in a block without fallback */
#define CCMM_ERR_STATE (-5)        /* call order violated (e.g. sweep before set_data) */

/* per-chain status bits (ccmm_chains_get_status) */
#define CCMM_STATUS_QR 1            /* CTA Cholesky failed, the host QR branch of CTA.m:80-92 redrew the chain (valid) */
#define CCMM_STATUS_CTA 2           /* CTA Cholesky pivot <= 0 without the QR repair (invalid draws) */
#define CCMM_STATUS_ASTEP 4         /* A-step Cholesky pivot <= 0 (invalid draws) */
#define CCMM_STATUS_SV 8            /* SV sampler pivot <= 0 (invalid draws) */
#define CCMM_STATUS_PHI 16          /* PHI Cholesky pivot <= 0 (invalid draws) */
#define CCMM_STATUS_HANDOFF 32      /* a device hand-off between workgroups / waves reached its spin cap (invalid) */
#define CCMM_STATUS_PS_GIBBS 64     /* the PS precision was not positive definite: the Gibbs draw served the
                                       sweep, as the reference's fallback (:462-463) does (valid) */
#define CCMM_STATUS_INFO (CCMM_STATUS_QR | CCMM_STATUS_PS_GIBBS)  /* informational bits */
#define CCMM_STATUS_PS 128          /* missing-data / alternate draw: precision not positive definite (invalid draws) */

/* model ids for the sweep-level API */
#define CCMM_MODEL_LINEAR 0        /* mcmcVAR.m */
#define CCMM_MODEL_BLOCKHYBRID 1   /* mcmcVARshadowrateBlockHybrid.m */
#define CCMM_MODEL_HYBRID 2        /* mcmcVARhybridGibbs.m: K = N*p + 1 + Ns*p, X = [1, lags, Xffrlags] */
#define CCMM_MODEL_SHADOWRATE 3    /* mcmcVARshadowrate.m: shadow-rate design for every equation, ELB step
                                      as the block hybrid, the linear model's predictive density */

/* RNG block ids (Philox counter word 3); also the order of the per-sweep CRN blocks */
#define CCMM_RNG_PAI 1   /* randn(K,N)            CTA.m:58 / CTAsys.m:58 */
#define CCMM_RNG_A 2     /* 19x randn(ii-1,1)     mcmcVAR.m:251 */
#define CCMM_RNG_SVU 3   /* rand(N,T)             SV mixture indicators */
#define CCMM_RNG_SVZ 4   /* randn(N,T+1)          SV joint draw h_0..h_T */
#define CCMM_RNG_PHI 5   /* randn(N,T+d_PHI)      mcmcVAR.m:268 */
#define CCMM_RNG_ELB 6   /* rand(Ns,elbT,101)     gibbsdrawShadowrates.m:173 */
#define CCMM_RNG_FCST 7  /* randn(N,H*Nd) then randn(N,H,Nd)  mcmcVAR.m:302,306 */
#define CCMM_RNG_PS 8    /* randn(nmiss,Nproposals)  PS proposals, mcmcVARshadowrateBlockHybrid.m:439-441 */
#define CCMM_RNG_PSALT 9 /* randn(nmiss,1)        the alternate draw, mcmcVARshadowrateBlockHybrid.m:471-475 */

/* treatment of the months at the ELB (ccmm_chains_set_elb_treatment) */
#define CCMM_ELB_TREAT_SHADOW 0   /* default: the censored cells are sampled below the bound (Gibbs / PS) */
#define CCMM_ELB_TREAT_MISSING 1  /* :481-499: one unconstrained draw per sweep becomes the data */
#define CCMM_ELB_TREAT_MISSING_PAIR 2  /* UNSUPPORTED, for tools/probe_missingdata.py only: as MISSING with the
                                          draw by the unfused kernel pair (k_ps_chol_w then k_ps_apply) instead
                                          of k_ps_draw1, same bits.  Not part of the interface: it may change
                                          or go without a new CCMM_ABI_VERSION */

typedef struct ccmm_ctx ccmm_ctx;
typedef struct ccmm_chains ccmm_chains;

/* ---------------------------------------------------------------- context */
int ccmm_abi_version(void);
const char* ccmm_last_error(void);
/* Environment.  A default build reads NO environment variable: kernel forms and schedules are the
 * explicit options below.  Timing-only ablation variables (CCMM_CHOL_SKIP, CCMM_SOLVE_SKIP, CCMM_SV_SKIP,
 * CCMM_GC_MODE, CCMM_LAG_MODE, CCMM_BIG_MASK, CCMM_ELB_MODE, the ablation bits of CCMM_SV_MODE,
 * CCMM_FCST_MODE, CCMM_POISON) leave the draws invalid and, like the options' CCMM_* defaults, are read
 * only by a build with -DCCMM_ABLATION (`make ablation`: libccmm_ablation.so); ccmm_ablation_build()
 * returns 1 there.  ccmm_env_ignored() returns how many CCMM_* variables the library knows are set and
 * ignored (names comma-separated in buf, len bytes with the terminator; buf may be NULL), and
 * ccmm_chains_create() leaves the same list in ccmm_last_error() as a warning. */
int ccmm_ablation_build(void);
int ccmm_env_ignored(char* buf, int len);
/* Kernel options: choices between kernel forms and schedules, set explicitly per context (inherited by
 * the chain sets created on it afterwards and used by the block-level drop-ins) or per chain set.
 * Schedules give bit-identical draws: solve_split (-1 auto, 0, 1), solve_async (0/1), sv_nwg (0 auto,
 * 1, 2, 4), elb_waves (1, 4, 8), elb_oct (0, 1 auto, 2), elb_async (0/1), elb_parts (0 auto, 1, 2, 4:
 * workgroups per chain of the ELB wavefront), fcst_reg (0/1), phi_overlap (0/1), qr_fallback (0/1),
 * big_lagx (0/1: the large path reads the column-major lag twin of a lag-structured X; set before
 * ccmm_chains_set_data), phi_stage (a mask on what the PHI kernel for N <= 32 keeps in LDS when it fits: 3 the
 * shocks and the normals, 1 the shocks only, 0 or 2 neither; the same products in the same order).
 * Forms run the same algorithm in another summation order (or the QR branch): lag (0/1), large_path
 * (0/1; set before ccmm_chains_set_data), astep_serial, ps_chol_lds, sv_mfma (0/1), force_qr,
 * girf_generic.  CCMM_ERR_ARG for an unknown name or a value out of range. */
int ccmm_option_count(void);
const char* ccmm_option_name(int i);
/* The value a new context starts from (host only): the built-in default in a default build, whatever the
 * environment holds; the ablation build's CCMM_* override. */
int ccmm_option_default(const char* name, int* value);
int ccmm_device_count(void);
/* Create a context bound to HIP device `device`.  Returns NULL on failure. */
ccmm_ctx* ccmm_create(int device);
void ccmm_destroy(ccmm_ctx* ctx);
int ccmm_synchronize(ccmm_ctx* ctx);
int ccmm_set_option(ccmm_ctx* ctx, const char* name, int value);
int ccmm_get_option(ccmm_ctx* ctx, const char* name, int* value);

/* --------------------------------------------------- block-level drop-ins */

/* Triangular (CTA) draw of the VAR coefficients, batched over B chains.
 * Replaces CTA.m:1-98 (called at mcmcVAR.m:228, mcmcVARhybridGibbs.m:376) and
 * CTAsys.m:1-108 (called at mcmcVARshadowrateBlockHybrid.m:343).
 *   Y      T x N (x B if y_per_chain)
 *   X      T x K x nx (x B if x_per_chain); equation j uses slab (nx==1 ? 0 : j)
 *          nx == 1 is CTA, nx == N is CTAsys
 *   A      N x N x B   unit lower triangular A_
 *   sqrtht T x N x B
 *   iVdiag K x N       diagonal of the block-diagonal prior precision iV (mcmcVAR.m:186)
 *   iVb    K x N       iVb_prior reshaped to K x N
 *   PAI    K x N x B   in: previous draw (columns j+1..N used by CTAsys); out: new draw
 *   z      K x N x B   randn(K,N) of CTA.m:58, or NULL (Philox, block CCMM_RNG_PAI, sweep 0)
 *   status B           per-chain status (0 ok, 1 QR fallback used), may be NULL
 * A chain whose posterior precision fails the device Cholesky is redrawn on the host by
 * the QR branch of CTA.m:80-92 (Householder QR of Kailath's array; same previous draw and
 * normals); the call then returns CCMM_WARN_QR_FALLBACK.  CCMM_ERR_NOTSPD only when the
 * QR factor itself is singular.
 * Supports 1 <= N <= 128, K <= 1536. */
int ccmm_cta(ccmm_ctx* ctx, int B, int T, int N, int K,
             const double* Y, int y_per_chain,
             const double* X, int nx, int x_per_chain,
             const double* A, const double* sqrtht,
             const double* iVdiag, const double* iVb,
             double* PAI, const double* z, int* status);

/* CTAsysAswitching.m:1-123 (the Aelb shadow-rate model's coefficient block): as ccmm_cta with
 * CTAsys designs, but the months with atELB[t] != 0 use the second A matrix Aelb in the residual
 * map and the weights (CTAsysAswitching.m:61-80: kron(Aelb_(j:N,j), XatELB) stacked over
 * kron(A_(j:N,j), XawayELB)).  Aelb N x N x B, atELB T bytes (logical, shared by the chains).
 * The QR branch (:82-93) is the host fallback of ccmm_cta with the same two-matrix map.
 * Supports N <= 32, K <= 256. */
int ccmm_cta_aswitching(ccmm_ctx* ctx, int B, int T, int N, int K,
                        const double* Y, int y_per_chain,
                        const double* X, int nx, int x_per_chain,
                        const double* A, const double* Aelb, const uint8_t* atELB,
                        const double* sqrtht, const double* iVdiag, const double* iVb,
                        double* PAI, const double* z, int* status);

/* A-matrix draw, flat prior (mcmcVAR.m:236-254 == mcmcVARshadowrateBlockHybrid.m:354-372).
 *   RESID T x N x B, sqrtht T x N x B, z (N(N-1)/2) x B or NULL
 *   A out N x N x B (unit lower), invA out N x N x B (A_\I, mcmcVAR.m:254) */
int ccmm_astep(ccmm_ctx* ctx, int B, int T, int N, const double* RESID, const double* sqrtht,
               const double* z, double* A, double* invA);

/* Stochastic-volatility block: KSC 7-component mixture indicators and joint
 * draw of the random-walk log variances with correlated shocks.  Replaces the
 * em-matlabbox call StochVolKSCcorrsqrt (mcmcVAR.m:261,
 * mcmcVARshadowrateBlockHybrid.m:379, mcmcVARhybridGibbs.m:405).
 *   logy2T N x T x B (logy2'), hprevT N x T x B (Vol_states'), sqrtPHI N x N x B lower,
 *   h0mean N, h0vcvsqrt N x N, u N x T x B or NULL, z N x (T+1) x B or NULL
 *   hT out N x T x B, h0 out N x B, shocksT out N x T x B, kai2 out N x T x B (int8, 1..7) */
int ccmm_sv_ksc(ccmm_ctx* ctx, int B, int T, int N, const double* logy2T, const double* hprevT,
                const double* sqrtPHI, const double* h0mean, const double* h0vcvsqrt,
                const double* u, const double* z, double* hT, double* h0, double* shocksT,
                int8_t* kai2);

/* Inverse-Wishart draw of the SV shock covariance (mcmcVAR.m:268-274).
 *   eta T x N x B, sPHI N x N, dPHI, Zdraw N x (T+dPHI) x B or NULL
 *   sqrtPHI out N x N x B (lower Cholesky of PHI_), PHI out N x N x B */
int ccmm_phi_iw(ccmm_ctx* ctx, int B, int T, int N, const double* eta, const double* sPHI,
                int dPHI, const double* Zdraw, double* sqrtPHI, double* PHI);

/* Gibbs draw of the ELB-censored shadow rates given the VAR state space, batched over B
 * independent calls.  Replaces gibbsdrawShadowrates.m:1-245 (called at
 * mcmcVARshadowrateBlockHybrid.m:436,462,494 and mcmcVARhybridGibbs.m:481,513).
 *   ndxS   Ny (logical)            sNaN  Ns x elbT (logical; censored cells)
 *   Y      Ny x elbT x B           the window, previous shadow values in censored cells
 *   STATE0 K x B (K = Ny p + 1)    YHAT0 Ny x elbT x B or NULL (zeros)
 *   C      K x K x B  (elb.A)      Psi   K x Ny x B (elb.B: invA in rows 2..Ny+1)
 *   SVol   Ny x elbT x B           u     Ns x elbT x (burnin + Ndraws) x B uniforms
 *                                        (rand(rndStream, Ns, elbT, .), :173) or NULL (Philox)
 *   out    Ns x elbT x Ndraws x B  flags Ns x elbT x (burnin + Ndraws) x B (drawTruncNormal
 *                                        branches, as ccmm_draw_trunc_normal) or NULL
 * Ndraws must be 1 (the reference's only use).  Evaluated in the stable residual form of the
 * device ELB step (ccmm_elb.hip): the same conditional moments as the QR formulation of
 * gibbsdrawShadowrates.m:74-145 in exact arithmetic, on the structural matrix A = Psi(2:Ny+1, :)^-1.
 * Any invertible impact matrix: a lower-triangular one (every reference caller passes invA,
 * mcmcVARshadowrateBlockHybrid.m:418) by forward substitution, a general one by Gauss-Jordan with
 * partial pivoting and the conditionals on the full A.  CCMM_ERR_ARG when Psi(2:Ny+1, :) is
 * singular; CCMM_ERR_DIM: sum(ndxS) != Ns (gibbsdrawShadowrates.m:50-52). */
int ccmm_gibbs_shadowrates(ccmm_ctx* ctx, int B, int Ny, int elbT, int Ns, int p, const uint8_t* ndxS,
                           const uint8_t* sNaN, const double* Y, const double* STATE0,
                           const double* YHAT0, const double* C, const double* Psi, const double* SVol,
                           double elbBound, int Ndraws, int burnin, const double* u, double* out,
                           uint8_t* flags);

/* gibbsdrawShadowratesB3 (gibbsdrawShadowratesB3.m:1-231, the 12-argument signature
 * (Y, STATE0, ndxS, sNaN, p, A, B, SVol, elbBound, Ndraws, burnin, rndStream)), batched over B calls:
 * the same Gibbs passes with the VAR run on Y itself (intercept in the state, STATElag starting at
 * STATE0, no deterministic Y0 path: :171-185) and an impact matrix that may vary by month.
 *   A      K x K x B (the companion with intercept)
 *   Bmat   K x Ny x elbT x B when B3d != 0 (B(:,:,t), :49-62), else K x Ny x B (repeated over t);
 *          rows 2..Ny+1 any invertible matrix (as ccmm_gibbs_shadowrates' Psi; every caller's B = invA)
 * The other arguments as ccmm_gibbs_shadowrates (no YHAT0).  The reference's only caller
 * (mcmcVARshadowrateBlockHybridAelb.m:451-452, 469-470) passes 13 arguments to this 12-parameter
 * function and cannot run as shipped; this entry serves the function itself. */
int ccmm_gibbs_shadowrates_b3(ccmm_ctx* ctx, int B, int Ny, int elbT, int Ns, int p, const uint8_t* ndxS,
                              const uint8_t* sNaN, const double* Y, const double* STATE0, const double* A,
                              const double* Bmat, int B3d, const double* SVol, double elbBound, int Ndraws,
                              int burnin, const double* u, double* out, uint8_t* flags);

/* One draw from N(mu, sig^2) truncated to (-inf, elb] by inverse CDF
 * (drawTruncNormal.m:31-86) with a pre-drawn uniform u (the numeric-stream
 * form of drawTruncNormal.m:47-48).  flags (may be NULL): bit0 = |sig| > 1e-10
 * branch taken, bit1 = PHIbar > eps branch taken.  Host-side scalar; the
 * device form runs inside the block-hybrid sweep (k_elb_gibbs). */
double ccmm_draw_trunc_normal(double mu, double sig, double elb, double u, uint8_t* flags);

/* Batched device evaluation of drawTruncNormal over n independent cells. */
int ccmm_draw_trunc_normal_batch(ccmm_ctx* ctx, int n, const double* mu, const double* sig,
                                 double elb, const double* u, double* out, uint8_t* flags);

/* --------------------------------------------------- sweep-level (device-resident) */

typedef struct {
  int model;              /* CCMM_MODEL_* */
  int N, p, K;            /* K = N*p + 1 */
  int T;                  /* max T over data slots */
  int B;                  /* number of chains */
  int ndata;              /* number of data slots (vintages) */
  int dPHI;               /* N + 3 (mcmcVAR.m:164) */
  int rng_crn;            /* 1: sweeps read CRN arrays from the host; 0: Philox */
  int store_capacity;     /* kept draws stored per chain (0: no storage) */
  double logy2offset;     /* getKSC7values offset (ext; this build declares 1e-3) */
  uint64_t seed;          /* Philox key */
  /* CCMM_MODEL_BLOCKHYBRID only (ignored otherwise) */
  int Ns;                 /* number of shadow-rate variables, 1..5 (Nshadowrates; 5 with the Krippner / Wu-Xia data at ELB > 0.25) */
  int elbTmax;            /* max over data slots of elbT = T - elbT0 */
  int elb_gibbsburn;      /* Gibbs burn-in passes per sweep (gibbsdrawShadowrates call, :436: 100) */
  double elb;             /* ELBbound */
} ccmm_chain_config;

ccmm_chains* ccmm_chains_create(ccmm_ctx* ctx, const ccmm_chain_config* cfg);
void ccmm_chains_destroy(ccmm_chains* ch);
/* Kernel options of one chain set (see ccmm_set_option; initialised from its context at create). */
int ccmm_chains_set_option(ccmm_chains* ch, const char* name, int value);
int ccmm_chains_get_option(ccmm_chains* ch, const char* name, int* value);

/* Data slot `slot`: one vintage's design (mcmcVAR.m:62-72, 186; 164-169).
 *   Y T x N, X T x K, iVdiag K x N, iVb K x N, sPHI N x N, h0mean N, h0vcvsqrt N x N */
int ccmm_chains_set_data(ccmm_chains* ch, int slot, int T, const double* Y, const double* X,
                         const double* iVdiag, const double* iVb, const double* sPHI,
                         const double* h0mean, const double* h0vcvsqrt);
/* slot_of_chain B ints (default: all chains use slot 0). */
int ccmm_chains_set_slots(ccmm_chains* ch, const int* slot_of_chain);
/* Chain state PREVdraw (mcmcVAR.m:197-206, 386-392): PAI K x N x B, A N x N x B,
 * sqrtht T x N x B, h (Vol_states) T x N x B, sqrtPHI N x N x B.  Resets the sweep counter. */
int ccmm_chains_set_state(ccmm_chains* ch, const double* PAI, const double* A,
                          const double* sqrtht, const double* h, const double* sqrtPHI);
/* Philox stream id of every chain (counter word 1; B values; NULL restores the default,
 * the chain index).  A batch driver keys chains by their global (vintage, chain) unit so
 * draws do not depend on how units are sharded over GPUs or packed into chain sets. */
int ccmm_chains_set_rng_ids(ccmm_chains* ch, const uint32_t* ids);
/* Opt-in MFMA phase lock (id > 0; 0 = none).  Chain sets on one device given the same id
 * serialise the MFMA Gram + Cholesky phase of their coefficient block (large-system path,
 * K > 512 or N > 32) through a cross-stream event.  Groups of chains driven on separate
 * contexts then fall out of step, and the per-chain sequential blocks of one group (CTA
 * solve, SV recursion, ELB Gibbs) overlap another group's MFMA phase.  Draws are unchanged. */
int ccmm_chains_set_mfma_lock(ccmm_chains* ch, int id);
/* KSC mixture indicators of the last SV block (T x N x B int8, 1..7; the draw of the
 * em-matlabbox sampler, mcmcVAR.m:261). */
int ccmm_chains_get_kai(ccmm_chains* ch, int8_t* kai);
/* Record the drawTruncNormal branch flags (as ccmm_draw_trunc_normal: bit0 |sig| > 1e-10,
 * bit1 PHIbar > eps) of every ELB step; get_elb_flags returns the last sweep's as
 * Ns x elbTmax x (gibbsburn + 1) x B uint8 (0 for uncensored cells). */
int ccmm_chains_record_elb_flags(ccmm_chains* ch, int enable);
int ccmm_chains_get_elb_flags(ccmm_chains* ch, uint8_t* flags);
/* Per-chain status word since set_state (B ints, OR of CCMM_STATUS_*: 2 CTA Cholesky, 4 A-step
 * Cholesky, 8 SV sampler, 16 PHI Cholesky found a non-positive pivot; the block
 * then continued with a unit pivot, so the chain's draws are invalid; 32: a device hand-off
 * between workgroups or waves reached its spin cap, never expected).  A CTA Cholesky
 * failure is repaired within the sweep by the host QR branch of CTA.m:80-92, which
 * replaces bit 2 by bit 1 ("QR fallback used", informational: the draws are valid); bit 64
 * (informational) marks a sweep whose PS precision failed and whose Gibbs draw served instead.
 * Returns 1 if any chain carries a bit outside CCMM_STATUS_INFO, 0 otherwise; the batch driver re-runs
 * flagged units (goVARshadowrateBlockHybrid.m:287-310). */
int ccmm_chains_get_status(ccmm_chains* ch, int* status);
/* Any output pointer may be NULL.  invA, PHI, RESID are those of the last sweep. */
int ccmm_chains_get_state(ccmm_chains* ch, double* PAI, double* A, double* invA, double* sqrtht,
                          double* h, double* sqrtPHI, double* PHI, double* RESID);
/* CRN doubles consumed per chain per sweep (blocks in CCMM_RNG_* order). */
int64_t ccmm_chains_crn_len(const ccmm_chains* ch);
/* Run nsweeps Gibbs sweeps (the body of `while m < MCMCreps`, mcmcVAR.m:195-398,
 * excluding the predictive block).  crn: B x nsweeps x crn_len (chain slowest) or
 * NULL in Philox mode.  store != 0 stores each sweep's draw (post-burn-in
 * semantics of mcmcVAR.m:278-292) into the on-device draw buffer.  Asynchronous
 * with respect to the host unless crn != NULL. */
int ccmm_chains_sweep(ccmm_chains* ch, int nsweeps, const double* crn, int store);
/* Number of stored draws per chain so far. */
int ccmm_chains_stored(const ccmm_chains* ch);
/* Copy stored draws out in the reference layout (mcmcVAR.m:178-181, 289-292;
 * mcmcVARshadowrateBlockHybrid.m:284-288, 536-543):
 *   PAI_all M x K x N x B, PHI_all M x N(N+1)/2 x B, invA_all M x N x N x B,
 *   sqrtht_all M x T x N x B, shadowrate_all M x Ns x elbTmax x B (block-hybrid;
 *   NaN beyond a vintage's elbT).  Any pointer may be NULL.  Resets the store. */
int ccmm_chains_get_draws(ccmm_chains* ch, double* PAI_all, double* PHI_all, double* invA_all,
                          double* sqrtht_all, double* shadowrate_all);
/* Running moments of the stored PAI draws on the device (the PAImean / PAIstdev accumulation of
 * goVARshadowrateBlockHybrid.m:376-377 without copying every draw to the host): adds the draws stored
 * so far (in store order, x then x * x, one rounding each) to per-chain running sums, reset first when
 * reset != 0; copies the sums out (K x N x B each) when the pointers are non-NULL.  Does not reset the
 * store (call before ccmm_chains_get_draws). */
int ccmm_chains_pai_moments(ccmm_chains* ch, int reset, double* sum, double* sumsq);

/* ---- predictive density inside the chain set (post-burn-in block of
 *      mcmcVAR.m:298-381 and mcmcVARshadowrateBlockHybrid.m:550-669) ----
 * Once configured, every stored sweep (ccmm_chains_sweep with store != 0) also
 * simulates Nd forecast paths of H horizons per chain from the chain's draw, without
 * leaving the device: Xjumpoff from the chain's resident data (block hybrid: shadow-rate
 * lags plus the vintage's actual-rate lags, :511-520), SV paths, the companion recursion
 * (linear: ltitr + censored simulation + zero-shock mean path; block hybrid: one
 * simulation on the K + Nyields p states with the actual rates max(shadow, ELB), :615-623)
 * and the one-step log scores (logscoreGaussian.m, logscoreGaussianCensored.m).
 * CRN mode appends randn(N, H*Nd) and randn(N, H, Nd) (block CCMM_RNG_FCST) to every
 * sweep's CRN record.  Linear, shadow-rate (linear forecast form) and block-hybrid models: N <= 128 (N <= 32:
 * one wave per draw, ccmm_fcst.hip; 32 < N <= 128: the draws batched as MFMA columns, ccmm_fcst_big.hip; same
 * records, same CRN and Philox layout).  Hybrid model: N <= 32 ("hybrid predictive density supports N <= 32").
 * ccmm_chains_set_irf1 is refused at N > 32 ("doIRF1 supports N <= 32").
 *   ndxYields N bytes (ndxYIELDS), keep_paths != 0 keeps every path for quantiles/CRPS.
 * Call after set_elb_model (block hybrid) and before sweeping. */
int ccmm_chains_set_fcst(ccmm_chains* ch, int H, int Nd, const uint8_t* ndxYields, int keep_paths);
/* yrealized(:,1) of data slot `slot` (N values; goVARshadowrateBlockHybrid.m:267-283,
 * shadow rates floored at the ELB by the caller). */
int ccmm_chains_set_fcst_slot(ccmm_chains* ch, int slot, const double* yrealized);
/* Linear predictive density: the variables floored at the ELB inside the censored
 * simulation (N bytes; NULL restores the default ndxYields, mcmcVAR.m:360-366).
 * mcmcVARshadowrate.m:539-546 floors ndxOTHERYIELDS only. */
int ccmm_chains_set_fcst_censor(ccmm_chains* ch, const uint8_t* floor_in_recursion);
/* Kept draws with a forecast record so far (-1: not configured). */
int ccmm_chains_fcst_stored(const ccmm_chains* ch);
/* Copy out and reset the forecast records of the M kept draws so far:
 *   scores   Nd x M x 4 x B: (:,:,k,c) reshaped to fcstNdraws x 1 is, for k = 0..3,
 *            fcstLogscoreDraws (uncensored Gaussian), fcstLogscoreELBdraws (censored; the
 *            block-hybrid fcstLogscoreDraws, :588-593), fcstLogscoreXdraws, fcstLogscoreIdraws
 *   fYsum    N x H x B  sum over the M x Nd paths (linear fcstYdraws; block hybrid the
 *            uncensored fcstShadowrateDraws)
 *   fYcsum   N x H x B  sum of the censored paths (linear fcstYcensorDraws; block hybrid
 *            fcstYdraws with the yields floored at the ELB, :697-700)
 *   yhatsum  N x H x B  sum of the zero-shock mean paths (linear yhatdraws; zero for bh)
 *   paths, paths_censored  N x H x Nd x M x B (only with keep_paths)
 * Any pointer may be NULL.  Censored scores with 4..12 series at the ELB use a deterministic
 * lattice estimate of mvncdf (MATLAB: randomised QMC, absolute tolerance 1e-4); returns
 * CCMM_WARN_MVNCDF when some censored score needed mvncdf in more than 12 dimensions (NaN). */
int ccmm_chains_get_fcst(ccmm_chains* ch, double* scores, double* fYsum, double* fYcsum,
                         double* yhatsum, double* paths, double* paths_censored);
/* ---- doIRF1: the impulse responses computed inside the sampler (mcmcVARshadowrateBlockHybrid.m:627-664,
 *      702-737; mcmcVARhybridGibbs.m:638-675, 713-748; mcmcVARshadowrate.m:588-605, 649-684) ----
 * Every kept draw's predictive simulation is run twice more on the same shocks, with the structural shock of
 * variable 1 (index 0) at horizon 1 replaced by +scale and by -scale (the value itself, not times the
 * volatility); no random number is drawn that the predictive density does not draw.  Block hybrid and hybrid:
 * the baseline's recursion with the actual rates max(shadow, ELB); mcmcVARshadowrate (and the linear model): the
 * linear recursion without a floor (ltitr, :596, 602).  Afterwards, per kept draw: the yields (ndxYields) of the
 * plus, minus and baseline paths floored at the ELB, irfdraws = floored plus (minus) - floored baseline, the rows
 * of cumcode cumulated over the horizons (cumsum(., 2)), the mean over the Nd draws.
 *   scale    IRF1scale (finite, else CCMM_ERR_ARG)
 *   cumcode  N bytes (IRFcumcode as a mask) or NULL (no row cumulated)
 * Call after ccmm_chains_set_fcst (else CCMM_ERR_STATE; a later set_fcst turns it off again) and before
 * sweeping; every model.  The predictive density's own records are those of a chain set without it. */
int ccmm_chains_set_irf1(ccmm_chains* ch, double scale, const uint8_t* cumcode);
/* Copy out (without resetting) the IRF1 records of the M kept draws so far; ccmm_chains_get_fcst resets them
 * together with the forecast records, so call this first.
 *   drawsPlus, drawsMinus    N x H x M x B  IRF1drawsPlus / IRF1drawsMinus (IRF1plus = their mean over M)
 *   y1sumPlus, y1sumMinus    N x H x B  sum over the M x Nd floored plus / minus paths, cumcode rows cumulated
 *                            (fcstY1hatPlus / Minus = the sum / (M Nd))
 *   pathsPlus, pathsMinus    N x H x Nd x M x B  fcstYdraws1plus / minus as simulated (raw: not floored, not
 *                            cumulated); only with keep_paths
 * Any pointer may be NULL. */
int ccmm_chains_get_irf1(ccmm_chains* ch, double* drawsPlus, double* drawsMinus, double* y1sumPlus,
                         double* y1sumMinus, double* pathsPlus, double* pathsMinus);

/* ---- shadow-rate models: block-hybrid (mcmcVARshadowrateBlockHybrid.m) and
 *      hybrid (mcmcVARhybridGibbs.m) ----
 * Hybrid: every equation uses the chain's X = [1, lags of the shadow-rate data,
 * Xffrlags] (CTA, mcmcVARhybridGibbs.m:376); the trailing Ns*p columns of the
 * slot X are the actual-rate lags floored at the ELB (:77-84) and stay fixed;
 * the ELB step adds Yhatactual = Xffrlags * PAI(Kshadow+1:end,:) (:429-431) and
 * uses PAI(1:Kshadow,:) in the companion matrix (:435-437).  actual_block must be
 * NULL (or all zero) for the hybrid model.
 * Data slot X/Y (ccmm_chains_set_data) are the vintage's ACTUAL data (X0, Y0,
 * :310-316); every chain keeps its own shadow-rate copy, reset to the slot's
 * data by ccmm_chains_set_state.  Equations with actual_block[j] != 0 use the
 * slot's X (CTAsys design of the actual-rate block), the others the chain's.
 *
 * ndxS: Ns strictly increasing 0-based shadow-rate variable indices (ndxSHADOWRATE);
 * actual_block: N bytes, actualrateBlock (:80-84).  Call before set_state. */
int ccmm_chains_set_elb_model(ccmm_chains* ch, const int* ndxS, const uint8_t* actual_block);
/* Per vintage: elbT0 (first VAR row, 0-based, of the ELB window; :176-183) and
 * sNaN Ns x elbT (column-major, elbT = T_slot - elbT0): nonzero where the shadow
 * rate is censored (data <= ELB, :163-171).  Call after ccmm_chains_set_data. */
int ccmm_chains_set_elb_slot(ccmm_chains* ch, int slot, int elbT0, const uint8_t* sNaN);
/* Acceptance-sampling branch of the ELB step (mcmcVARshadowrateBlockHybrid.m:435-466):
 * from sweep m >= ps_from_m (1-based; the reference: m >= MCMCburnin/2, i.e.
 * ps_from_m = ceil(MCMCburnin/2)) every sweep first draws nproposals (elb.Nproposals =
 * 1e3, :188) unconstrained proposals of the censored cells from their joint Gaussian
 * given the VAR — the em-matlabbox sampler VARTVPSVprecisionsamplerNaN (:439-441), restated
 * as the precision sampler y_m = L' \ (L \ b + z_k), P = L L' — and accepts the first
 * whose censored cells all lie below the ELB (:446-452); otherwise the Gibbs draw of
 * gibbsdrawShadowrates serves the sweep (:462-463).  CRN mode appends randn(nmiss,
 * nproposals) (block CCMM_RNG_PS, nmiss x nproposals column-major, sized Ns elbTmax
 * nproposals) to every sweep's record.  nproposals = 0: Gibbs every sweep (default).
 * Requires Ns (p + 1) <= 80. */
int ccmm_chains_set_elb_ps(ccmm_chains* ch, int nproposals, int ps_from_m);
/* Treatment of the ELB months (doELBsampling / doELBsampleAlternate of the reference samplers); call after
 * ccmm_chains_set_elb_model and before ccmm_chains_set_state.
 * CCMM_ELB_TREAT_MISSING (doELBsampling = false: mcmcVARshadowrateBlockHybrid.m:481-499,
 * mcmcVARhybridGibbs.m:499-518, mcmcVARshadowrate.m:442-459; block-hybrid, hybrid and shadow-rate
 * models): every sweep's ELB step takes one unconstrained draw of the censored cells from the precision
 * sampler and writes it over them whether or not it lies below the bound; no Gibbs kernel runs.
 * alternate must be 0, ccmm_chains_set_elb_ps with nproposals > 0 is refused (either call order) and the
 * censored-cell band width must be <= 80.  The CRN record is the one ccmm_chains_set_elb_ps(ch, 1, .)
 * gives (the CCMM_RNG_ELB block present and unread, the draw's normals the first nmiss of CCMM_RNG_PS);
 * under Philox the draw takes the numbers of proposal 1 of a PS sweep.  A precision that is not positive
 * definite sets CCMM_STATUS_PS and leaves the cells as they were.  Stored sweeps keep shadowrate_all NaN
 * (:492) and the draw as missingrate (ccmm_chains_get_missingrate; no ccmm_chains_keep_missingrate
 * call needed); ccmm_chains_get_shadowrate returns the imputed path; the counts of ccmm_chains_get_ps
 * stay 0.
 * CCMM_ELB_TREAT_SHADOW with alternate = 1 (doELBsampleAlternate, block hybrid only, :470-475): after the
 * sweep's ELB step one more unconstrained draw from the same precision and the observed data is stored
 * as missingrate and enters nothing else; chain state and all other draws are those of the run without
 * it.  CRN mode appends a block CCMM_RNG_PSALT of Ns elbTmax normals last; Philox uses block id 9 with
 * the per-cell numbering of CCMM_RNG_PS.  The status word can differ from that run's: where the sweep's own
 * PS precision is not positive definite (CCMM_STATUS_PS_GIBBS, informational: the Gibbs draw serves the
 * sweep) the alternate draw factors the same precision, fails too and sets CCMM_STATUS_PS, so a run that is
 * valid without alternate is reported invalid with it (that sweep's missingrate is then the state's copy,
 * not a draw). */
int ccmm_chains_set_elb_treatment(ccmm_chains* ch, int treatment, int alternate);
/* Host-only: 1 if the one-draw kernel (k_ps_draw1) keeps the band factor of nmax censored cells of band
 * width W (16, 32, 48 or 64) in LDS over an ELB window of elbTmax months, 0 if it reads it back from
 * global memory. */
int ccmm_ps_draw1_resident(int W, int elbTmax, int nmax);
/* PS bookkeeping (:303-305, 453-460): countAccept / countAcceptBurnin B ints since set_state
 * (sweeps whose proposal was accepted after / during burn-in), stackAccept M x B ints
 * (ndxAccept of each stored draw, 0 = no proposal accepted or Gibbs sweep; M = stored draws;
 * call before ccmm_chains_get_draws, which resets the store).  Any pointer may be NULL. */
int ccmm_chains_get_ps(ccmm_chains* ch, int* countAccept, int* countAcceptBurnin, int* stackAccept);
/* missingrate_all (mcmcVARshadowrate.m:270, 435, 498; mcmcVARhybridGibbs.m:332, 486): with enable != 0
 * every stored sweep also keeps proposal 1 of its PS branch (shadowrateProposals(:,:,1): the censored cells
 * from the sampler, the others the window's data); a sweep that ran the Gibbs branch stores NaN (:406).
 * Call before the first stored sweep.  get_missingrate: M x Ns x elbTmax x B, NaN beyond a vintage's
 * window; call before ccmm_chains_get_draws (which resets the store).  The block-hybrid driver keeps
 * missingrate NaN (doELBsampleAlternate = false, mcmcVARshadowrateBlockHybrid.m:470-478). */
int ccmm_chains_keep_missingrate(ccmm_chains* ch, int enable);
int ccmm_chains_get_missingrate(ccmm_chains* ch, double* missingrate_all);
/* Parity diagnostic of the PS branch: the conditional mean P^-1 b of the censored cells that
 * the last PS sweep's proposals were drawn around (VARTVPSVprecisionsamplerNaN at z = 0,
 * mcmcVARshadowrateBlockHybrid.m:439-441), Ns x elbTmax x B, NaN outside the censored cells
 * (the device's banded factor, back-substituted on the host). */
int ccmm_chains_get_ps_mean(ccmm_chains* ch, double* mean);
/* Parity diagnostic: the device's weighted Gram of every CTA system at the chain set's current
 * state (A, sqrtht, X), K x K x N x B: [c b'; b M] with c = sum_t w_t, b = X~' w, M = X~' diag(w) X~
 * (CTA.m:73 without the prior), exactly as the lag-structured coefficient kernel forms it before
 * the factorisation.  Only when that path is active (linear / block-hybrid models, N <= 32). */
int ccmm_chains_get_cta_gram(ccmm_chains* ch, double* G);
/* Parity diagnostic: the factor record of every CTA system at the current state as the lag-structured
 * kernel writes it, (NT (NT + 1) / 2 * 256 + 256) doubles per system (NT = ceil((K - 1) / 16)), systems
 * ordered (equation, chain): the 16 x 16 factor tiles in slot order (slot g = column-major enumeration of
 * the lower tile pairs (ti, tj); element (row (lane >> 4) + 4 r, column lane & 15) at g 256 + 64 r + lane;
 * off-diagonal slots the unit block factor's blocks, diagonal slots the inverses of the diagonal
 * factor tiles, transposed), then [1 / L00, L(1 + a, 0) for a = 0..16 NT - 1].  Same path as
 * ccmm_chains_get_cta_gram. */
int ccmm_chains_get_cta_factor(ccmm_chains* ch, double* F);
/* Current shadow rates, Ns x elbTmax x B (the last sweep's draw). */
int ccmm_chains_get_shadowrate(ccmm_chains* ch, double* shadowrate);
/* Current per-chain data: X T x K x B, Y T x N x B (block-hybrid: the chain's
 * shadow-rate X/Y, PREVdraw.X/Y; linear: the slot's data).  Either may be NULL. */
int ccmm_chains_get_xy(ccmm_chains* ch, double* X, double* Y);
/* Per-kernel device time (HIP events on the chain set's stream) accumulated
 * while profiling is on.  names: ';'-separated list written into buf. */
int ccmm_chains_profile(ccmm_chains* ch, int enable);
int ccmm_chains_kernel_times(ccmm_chains* ch, int max, double* ms, int64_t* launches,
                             char* names, int names_len);

/* ------------------------------------------------------------ post-processing
 * Per-vintage summaries of kept draws (goVARshadowrateBlockHybrid.m:349-480), on the
 * device: for each series the mean, median, quantiles at pct[0..nq-1] (MATLAB prctile:
 * the i-th sorted draw sits at percentile 100 (i - 0.5)/n, linear in between), std(., 1)
 * and, when realized is given, crpsDraws (the CRPS of the draws' empirical distribution,
 * mean|x - y| - sum_ij |x_i - x_j| / (2 n^2); em-matlabbox source absent).  Outputs
 * mean/median/stdev/crps S, quantiles S x nq (series fastest); any may be NULL. */
/* Host draws n x S (each series' n draws contiguous), realized S or NULL. */
int ccmm_draw_summaries(ccmm_ctx* ctx, int S, int n, const double* draws, const double* realized, int nq,
                        const double* pct, double* mean, double* median, double* quantiles, double* stdev,
                        double* crps);
/* The kept draws of the chains bound to data slot `slot` (contiguous chain indices), pooled:
 *   source 0  forecast paths (keep_paths; linear fcstYdraws, block hybrid the uncensored
 *             shadow-rate paths), series = selected rows x H (row fastest), draws = chains x
 *             kept records x Nd
 *   source 1  censored forecast paths (linear fcstYcensorDraws, block hybrid fcstYdraws)
 *   source 2  PAI draws, series = K x N, draws = chains x stored draws
 *   source 3  sqrtht draws, series = Tmax x N (t fastest); a series at t >= T of the slot holds no draw
 *   source 4  shadowrate_all, series = Ns x elbTmax (rate fastest); the months at or beyond the slot's elbT
 *             hold no draw
 *   source 5  missingrate_all, as source 4; an argument error unless missing rates were kept
 *             (ccmm_chains_keep_missingrate, or the missing / alternate treatment of the ELB months)
 * rows: N bytes selecting the variables (NULL: all); cumcode: N bytes, cumsum over the
 * horizons for those variables first (:353-355; NULL: none).
 * Sources 3 to 5 (doVARshadowrateBlockHybridMissingData.m:223-244, 475-478) read the store in place and take
 * no rows, cumcode, realized, crps or floor: passing one is an argument error.  A series without a draw is NaN
 * in every statistic.  Their draws may be NaN (shadowrate_all under the missing-data treatment, missingrate_all
 * of a kept sweep without a PS proposal) and then follow MATLAB: mean, stdev and median are NaN as soon as one
 * draw of the series is NaN; the quantiles are prctile over the other draws, NaN when there are none.  Sources 0
 * to 2 run the kernel without these rules, as before. */
int ccmm_chains_summaries(ccmm_chains* ch, int source, int slot, const uint8_t* rows, const uint8_t* cumcode,
                          const double* realized, int nq, const double* pct, double* mean, double* median,
                          double* quantiles, double* stdev, double* crps);
/* As ccmm_chains_summaries, with the forecast paths of the variables selected by floor_rows (N
 * bytes) floored at `floor` first, y(y < floor) = floor, before any cumsum: the shadow-rate
 * VAR's draws (mcmcVARshadowrate.m:642-645 fcstYdraws, yields floored on the uncensored paths;
 * :676-681 fcstYcensorDraws, shadow rates floored on the censored paths) summarised by
 * goVARshadowrate.m:356-478.  Sources 0 and 1 only. */
int ccmm_chains_summaries_floor(ccmm_chains* ch, int source, int slot, const uint8_t* rows, const uint8_t* cumcode,
                                const uint8_t* floor_rows, double floor, const double* realized, int nq,
                                const double* pct, double* mean, double* median, double* quantiles, double* stdev,
                                double* crps);

/* ------------------------------------------------------------ maximum VAR root
 * max(abs(eig(comp))) of the N p x N p companion matrix of each of M coefficient matrices
 * (goVARshadowrateBlockHybrid.m:382-392 drawsMaxVARroot; mcmcVAR.m:221-232 check_stationarity): rows
 * 1..N p of PAI (K x N column-major, K >= 1 + N p, M matrices K N doubles apart) transposed on top, the
 * shifted identity below.  fp64 Householder reduction to Hessenberg form and implicit double-shift QR,
 * eigenvalues only.  maxroot: M doubles.  info: M ints, 0 converged, 1 a NaN or Inf among the n x N
 * coefficients (maxroot = NaN, nothing iterated), 2 the cap of 30 n QR iterations was reached (never seen;
 * maxroot = the largest modulus deflated by then); may be NULL. */
/* On the CPU (at most 16 threads); needs no context and no GPU. */
int ccmm_max_var_root_host(int M, int N, int p, int K, const double* PAI, double* maxroot, int* info);
/* Host PAI; on the device for N p <= 256 (one wave per matrix, bit-identical to the host function),
 * on the CPU for larger N p and for any matrix the device returned info = 2 for. */
int ccmm_max_var_root(ccmm_ctx* ctx, int M, int N, int p, int K, const double* PAI, double* maxroot, int* info);
/* The stored PAI draws of the chains bound to data slot `slot` (contiguous chain indices), read in place
 * on the device: maxroot[m * C + c] for stored draw m (slowest) and the slot's c-th chain (fastest),
 * stored x C values; info likewise or NULL.  Returns C (> 0), or a negative error code.  The draw store is
 * left as it is. */
int ccmm_chains_max_var_roots(ccmm_chains* ch, int slot, double* maxroot, int* info);

/* ------------------------------------------------------------ impulse responses (VMA)
 * drawsVMA(:,:,h,m) = (comp^h)(1:N,1:N), h = 1..H, of each of M coefficient matrices
 * (goVARshadowrateBlockHybrid.m:393-408), PAI as for the maximum root (K x N column-major, K >= 1 + N p; the
 * intercept row and the rows beyond 1 + N p are ignored).  Computed as the recursion
 * Psi_h = sum_l Phi_l Psi_{h-l} (Psi_0 = I, Phi_l = PAI(1 + (l-1) N + (1:N), :)'), the as-written product with
 * its exact zeros removed, in fp64 with one fused multiply-add chain per element (lags ascending, columns
 * ascending within a lag).  vma: N x N x H x M doubles in MATLAB order (vma[((m H + h-1) N + j) N + i] =
 * Psi_h(i, j) of matrix m).  info: M ints, 0, or 1 for a NaN or Inf among the N p x N coefficients; may be
 * NULL.  A matrix with info = 1 is NaN in every entry of every horizon; the reference's product gives NaN (or
 * keeps finite entries) at h = 1 where the non-finite coefficient does not reach and NaN everywhere from
 * h = 2 on: h = 1 is the one documented difference. */
/* On the CPU (at most 16 threads); needs no context and no GPU. */
int ccmm_vma_host(int M, int N, int p, int K, int H, const double* PAI, double* vma, int* info);
/* Host PAI, uploaded in chunks; on the device for N <= 32 and N p <= 256 (one workgroup per matrix on the FP64
 * MFMA, bit-identical to the host function), on the CPU for any larger shape. */
int ccmm_vma(ccmm_ctx* ctx, int M, int N, int p, int K, int H, const double* PAI, double* vma, int* info);
/* As ccmm_vma on the device range only, with the kernel form chosen: 0 the MFMA product (ccmm_vma's), 1 the
 * same chains on the vector ALU (the same bits); kernel_ms (or NULL): the device time of the kernel launches
 * alone.  The comparison entry of tools/probe_vma.py. */
int ccmm_vma_form(ccmm_ctx* ctx, int form, int M, int N, int p, int K, int H, const double* PAI, double* vma,
                  int* info, double* kernel_ms);
/* VMAmid / VMAtail and sumFFRmid / sumFFRtail (:409-429) of the stored PAI draws of the chains bound to data
 * slot `slot` (contiguous chain indices), read in place and pooled over the slot's C chains (stored x C draws):
 * per slab of horizons the responses of every draw (draw-major), their transposition into per-series segments
 * and the median and MATLAB prctile of each series (as ccmm_chains_summaries).  hslab: horizons per slab, 0 for
 * the most that keeps every buffer of a pass within 1 GB; the results do not depend on it.  vmaMedian: N N H;
 * vmaQuantiles: N N H x nq, series fastest; either may be NULL.  ffr >= 0 (0-based variable; -1: none) also
 * gives, per equation n, the statistics of sum_{l=0..p-1} PAI(1 + l N + ffr, n) (plain adds, ascending lag):
 * sumMedian N, sumQuantiles N x nq.  nbad (or NULL): the draws with a NaN or Inf coefficient (their responses
 * are NaN and enter the statistics as such).  N <= 32 and N p <= 256 only.  Returns C (> 0), or a negative
 * error code.  The draw store is left as it is. */
int ccmm_chains_vma_summaries(ccmm_chains* ch, int slot, int H, int hslab, int nq, const double* pct,
                              double* vmaMedian, double* vmaQuantiles, int ffr, double* sumMedian,
                              double* sumQuantiles, int* nbad);

/* ------------------------------------------------------------ conditional mean paths
 * thatMean of doVARshadowrateBlockHybridMissingData.m:433-468 (and doVARshadowrateMissingData.m) for each of M
 * coefficient matrices: x_H(1:N) of the recursion x_0 = y0, x_{h+1} = c~ + comp x_h with comp the N p x N p
 * companion matrix and c~ = [PAI(0,:)'; 0].  The reference writes ((I - comp) \ (I - comp^H)) c~ + comp^H y0, the
 * same vector whenever I - comp is nonsingular; cond(I - comp) is 2-3e6 on the reference's data, so the recursion
 * is also the more accurate form.  PAI as for the maximum root (K x N column-major, K >= 1 + N p; rows beyond
 * 1 + N p are ignored).  y0: ny0 x N p doubles, p blocks of N in the order of the companion state (block 0 is
 * multiplied by lag 1), whatever they hold; ny0 = 1 (one y0 for all draws) or M.  The reference fills y0 with
 * YdataELB(:), YdataELB = data(meanjumpoff-(p-1):meanjumpoff,:)', which is oldest month first while the
 * companion state is newest first; the functions here take y0 as given, and samplers.doVARMissingData builds it
 * as the reference writes it.  Every equation of a step is one fp64 fused multiply-add chain that starts from the
 * intercept and runs over the state ascending.  mean: N x M doubles (mean[m N + i]).  info: M ints, 0, or 1 for a
 * NaN or Inf among rows 0 .. N p of the matrix (that draw's mean is NaN); may be NULL.  A non-finite y0 is an
 * argument error. */
/* On the CPU (at most 16 threads); needs no context and no GPU. */
int ccmm_cond_mean_host(int M, int N, int p, int K, int H, const double* PAI, const double* y0, int ny0,
                        double* mean, int* info);
/* Host inputs; on the device for N <= 32 and N p <= 256 (one wave per matrix, bit-identical to the host
 * function), on the CPU for any larger shape. */
int ccmm_cond_mean(ccmm_ctx* ctx, int M, int N, int p, int K, int H, const double* PAI, const double* y0, int ny0,
                   double* mean, int* info);
/* The stored PAI draws of the chains bound to data slot `slot` (contiguous chain indices), read in place, one
 * y0 (N p doubles) for all: mean[(m C + c) N + i] for stored draw m and the slot's c-th chain, the order of
 * ccmm_chains_max_var_roots; info likewise or NULL.  Returns C (> 0), or a negative error code.  The draw store
 * is left as it is. */
int ccmm_chains_cond_means(ccmm_chains* ch, int slot, int H, const double* y0, double* mean, int* info);

/* check_stationarity (mcmcVAR.m:221-232, mcmcVARshadowrateBlockHybrid.m:333-347): with enable != 0 every
 * sweep computes the maximum VAR root of each chain's new PAI after the coefficient block and, while a chain's
 * root is >= 1 (or not finite), draws its coefficient block again from the rejected PAI with fresh normals; the
 * chains already accepted keep their draw.  One host synchronisation per sweep and one more per redraw round
 * (few open chains go to the host function, many to the kernel: same bits).  The reference loops without
 * bound; here a chain still non-stationary after max_attempts redraws (<= 0: the default, 1000; at most 2^24 - 1)
 * keeps its last draw and gets CCMM_STATUS_NONSTATIONARY.
 * Normals: attempt 0 is the sweep's ordinary draw (every counter as without the option).  Redraw a >= 1 of a
 * chain takes its CCMM_RNG_PAI normals from the Philox counter (pair index, chain id, sweep,
 * CCMM_RNG_PAI | a << 8): word 3 of attempt 0 is the block id alone (< 256), so the streams are disjoint and a
 * function of (seed, chain id, sweep, a) only.  Philox mode only: CCMM_ERR_ARG on a CRN chain set (its layout
 * holds one randn(K, N) block per sweep).  Off (the default) launches nothing and changes nothing. */
#define CCMM_STATUS_NONSTATIONARY 256  /* check_stationarity: max_attempts redraws exhausted (invalid draws) */
int ccmm_chains_set_stationarity(ccmm_chains* ch, int enable, int max_attempts);
/* redraws: B values, the coefficient blocks drawn again per chain since ccmm_chains_set_state. */
int ccmm_chains_get_stationarity(ccmm_chains* ch, int64_t* redraws /* B */);

/* ------------------------------------------------------------ batch run (the vintage loop)
 * ccmm_run_batch replaces the parfor over vintages of goVARshadowrateBlockHybrid.m:258-517
 * (goVARhybrid.m:258 for the hybrid model, goVAR.m:242 for the linear one) for the vintages
 * handed to this process: ONE device-resident chain set holds every vintage as a data slot with
 * `nchains` chains; each chain runs `burnin` + MCMCdraws sweeps (mcmcVARshadowrateBlockHybrid.m:
 * 56-58, 306-689) and every kept sweep simulates fcstNdraws / MCMCdraws forecast paths on the
 * device (:550-625).  The ELB step is the Gibbs sampler for m < ceil(burnin / 2) and the
 * accept-first PS proposals after (:433-466; hybrid: PS at every sweep, mcmcVARhybridGibbs.m:458;
 * Nproposals = 0: Gibbs every sweep).  Philox streams: chain c of vintage v is keyed by
 * unit(v) * nchains + c (+ 1000003 per retry), so results do not depend on how vintages are
 * sharded over processes.  Failure recovery (goVARshadowrateBlockHybrid.m:287-310): a vintage
 * whose chains flagged a non-SPD pivot (ccmm_chains_get_status bits other than 1) is re-run from
 * its initial state on fresh streams, up to max_retries times; after that its outputs are NaN.
 * The setup of each vintage (data matrices, Minnesota prior, initial PREVdraw) is the caller's:
 * the MATLAB driver's own code computes it (mcmcVARshadowrateBlockHybrid.m:30-295, :308-317). */
typedef struct {
  int T;                        /* VAR rows (thisT - p) */
  const double* Y;              /* T x N (actual data, :62-72) */
  const double* X;              /* T x K */
  const double* iVdiag;         /* K x N (diagonal of iV, mcmcVAR.m:186) */
  const double* iVb;            /* K x N */
  const double* sPHI;           /* N x N */
  const double* h0mean;         /* N     Vol_0mean */
  const double* h0vcvsqrt;      /* N x N Vol_0vcvsqrt */
  const double* PAI0;           /* K x N  PREVdraw.PAI at m == 0 (X\Y, :308) */
  const double* sqrtht0;        /* T x N  PREVdraw.sqrtht at m == 0 (AR residuals, :313) */
  const double* h0init;         /* T x N  PREVdraw.Vol_states at m == 0 (2 log(sqrtht0), :314), or NULL:
                                   computed here */
  int elbT0;                    /* shadow-rate models: first VAR row (0-based) of the ELB window */
  const uint8_t* sNaN;          /* Ns x (T - elbT0) censored cells (may be NULL when T == elbT0) */
  const double* yrealized;      /* N x H (goVARshadowrateBlockHybrid.m:267-283, floored at the ELB) */
  uint32_t unit;                /* global vintage index (Philox stream key) */
} ccmm_vintage;

typedef struct {
  int model;                    /* CCMM_MODEL_LINEAR, _BLOCKHYBRID or _HYBRID */
  int N, p;                     /* K = N p + 1 (+ Ns p for the hybrid model) */
  int Ns;                       /* shadow-rate models: number of shadow rates */
  const int* ndxS;              /* Ns 0-based ndxSHADOWRATE */
  const uint8_t* actual_block;  /* N bytes, actualrateBlock (block hybrid; NULL otherwise) */
  const uint8_t* ndxYields;     /* N bytes, ndxYIELDS (forecast censoring) */
  int nchains;                  /* chains per vintage */
  int MCMCdraws;                /* kept sweeps per chain */
  int burnin;                   /* burn-in sweeps per chain (the reference: MCMCdraws) */
  int gibbsburn;                /* Gibbs passes per ELB step before the kept one (100) */
  int Nproposals;               /* elb.Nproposals (1000); 0: Gibbs ELB step every sweep */
  int fcstNdraws;               /* multiple of MCMCdraws (:123-126) */
  int H;                        /* fcstNhorizons */
  double elb;                   /* ELBbound */
  uint64_t seed;                /* rndStream seed */
  int chunk;                    /* sweeps per device call (host synchronisation points) */
  int max_retries;
  int postprocess;              /* keep every kept draw and path in HBM; device summaries */
  int nq;                       /* number of quantiles (postprocess) */
  const double* pct;            /* nq percentiles (setQuantiles) */
  const uint8_t* cumcode;       /* N bytes or NULL: cumsum over horizons (:353-355) */
} ccmm_batch_config;

typedef struct {                /* V = number of vintages; any pointer may be NULL */
  double* logscore;             /* 4 x V log mean exp over the fcstNdraws * nchains one-step score
                                   draws (k as ccmm_chains_get_fcst: 1 = fcstYmvlogscore, 2 = X,
                                   3 = I; :437-447) */
  double* fcstYhat;             /* N x H x V mean censored path (:450) */
  double* fcstShadowYhat;       /* N x H x V mean uncensored (shadow-rate) path */
  double* PAImean;              /* K x N x V (:376) */
  double* PAIstdev;             /* K x N x V std(., 1) (:377) */
  double* shadowrate_all;       /* MCMCdraws x Ns x elbTmax x nchains x V kept shadow rates */
  int* countELBaccept;          /* V (countAccept + countAcceptBurnin over the vintage's chains) */
  int* attempts;                /* V: runs used (> max_retries + 1: failed, outputs NaN) */
  /* postprocess != 0 (goVARshadowrateBlockHybrid.m:349-480) */
  double* fcstYmedian;          /* N x H x V */
  double* fcstYcrps;            /* N x H x V */
  double* fcstYquantiles;       /* N x H x nq x V */
  double* fcstYcummedian;       /* N x H x V (cumcode applied to paths and yrealized) */
  double* fcstYcumcrps;         /* N x H x V */
  double* fcstYcumquantiles;    /* N x H x nq x V */
  double* fcstShadowYmedian;    /* Ny x H x V (rows ndxYields) */
  double* fcstShadowYquantiles; /* Ny x H x nq x V */
  double* PAImedian;            /* K x N x V */
  double* PAIquantiles;         /* K x N x nq x V */
  double* scoreDraws;           /* (fcstNdraws * nchains) x 4 x V, order (Nd, kept draw, chain) */
  double* shadowratePSRF;       /* Ns x V (shadow-rate models): ccmm_shadowrate_psrf of the vintage's kept
                                   shadow rates (goVARshadowrateBlockHybrid.m:322-325; the reference's
                                   one-chain statistic, averaged over the vintage's chains) */
  double* shadowratePSRFchains; /* Ns x V: ccmm_shadowrate_psrf_chains (psrf across the vintage's chains;
                                   NaN for one chain) -- not in the reference's output */
} ccmm_batch_out;

int ccmm_run_batch(ccmm_ctx* ctx, const ccmm_batch_config* cfg, int V, const ccmm_vintage* vintages,
                   ccmm_batch_out* out);

/* ------------------------------------------------------------ GIRF
 * Generalized impulse responses by antithetic simulation, batched over M MCMC draws
 * (generateGIRF2linear.m / generateGIRF2blockhybrid.m:199-259 with antitheticSim and
 * simVAR / simVARshadowrateBlockHybrid): per draw, nsim shock paths (SV paths
 * exp(cumsum(sqrtPHI randn)/2)) x 4 antithetic sets (+-z .* SV^{+-1} .* SV0) x 3 scenarios
 * (shock11 = 0, +shock11, -shock11 added to variable 1 at horizon 1), mapped by invA and
 * simulated over H horizons (bh != 0: actual-rate states max(shadow, ELB), yields floored at
 * the ELB in the output), cumcode variables cumsum / np, averaged over the 4 nsim paths.
 *   PAI K x N x M, invA N x N x M, sqrtPHI N x N x M (chol(PHI, 'lower')), SV0 N x M (jump-off
 *   sqrtht), Xjumpoff (K + Ny p) x M (linear: K), actual / ndxYields N bytes (bh), cumcode N
 *   bytes or NULL; z, svz N x H x nsim x M (randn(N, H, nsim), randn(N, H*nsim)) or both NULL
 *   (Philox keyed by (seed, draw)).
 *   yhat out N x H x 3 x M: fcstYHATdraws, fcstYHATdraws1plus, fcstYHATdraws1minus.
 * N <= 32. */
int ccmm_girf(ccmm_ctx* ctx, int M, int N, int p, int H, int nsim, const double* PAI, const double* invA,
              const double* sqrtPHI, const double* SV0, const double* Xjumpoff, int bh, const uint8_t* actual,
              const uint8_t* ndxYields, double elb, const uint8_t* cumcode, double np_, double shock11,
              const double* z, const double* svz, uint64_t seed, double* yhat);

/* generateGIRF2hybrid.m:176-259 (simVARhybrid, :361-386): the hybrid model's GIRFs.  The state
 * holds [1, p lags of y, p lags of the Ns actual (shadow-rate) variables]; the companion rows are
 * the full hybrid PAI (:226-227: fcstA(ndxfcstY,:) = PAIdraws), the actual-rate states are
 * max(shadow, ELB) (:373-375) and the output floors ndxYields (:378-381).
 *   PAI (K + Ns p) x N x M (K = N p + 1), Xjumpoff (K + Ns p) x M, ndxShadow / ndxYields N bytes;
 *   the rest as ccmm_girf. */
int ccmm_girf_hybrid(ccmm_ctx* ctx, int M, int N, int p, int H, int nsim, const double* PAI, const double* invA,
                     const double* sqrtPHI, const double* SV0, const double* Xjumpoff, const uint8_t* ndxShadow,
                     const uint8_t* ndxYields, double elb, const uint8_t* cumcode, double np_, double shock11,
                     const double* z, const double* svz, uint64_t seed, double* yhat);

/* The GIRFs of the stored draws of the chains bound to data slot `slot` (contiguous chain indices), read in place
 * and pooled over the slot's C chains, chain slowest: draw d = c stored + m, n = C stored draws (the full-sample
 * study: generateGIRF2linear.m / generateGIRF2blockhybrid.m / generateGIRF2hybrid.m over the draws of doMCMC*.m,
 * by the set's model; the shadowrate model has no such script and is refused).  One date, nscales shock sizes.
 *   t0: 0-based row of the data at irfDate (ndxIRFT0 - 1); jump: p x N doubles, jump[l N + j] = data(t0 - l, j),
 *   the months t0, t0 - 1, ..; SV0 is row t0 - p of the draw's sqrtht, sqrtPHI the lower Cholesky factor of its
 *   PHI, Xjumpoff [1, the p months, the ring of the yields (block hybrid) or of the shadow-rate variables (hybrid)],
 *   where with n' = t0 + 1 - elbT0 - p > 0 the shadow-rate variables of month t0 - l are month n' - 1 - l of the
 *   draw's shadow rates when that is >= 0 (generateGIRF2blockhybrid.m:204-218).
 *   ndxYields: N bytes (the shadow-rate models; NULL for the linear model): the ring and the actual-rate block of
 *   the block hybrid (actual = not a yield), the output floor of both.  cumcode: N bytes or NULL.
 *   Draw d is simulated by ccmm_girf's kernels with Philox stream d of `seed`, in passes whose workspace stays
 *   within 1 GB (draws_per_pass > 0: that many draws per pass); the results do not depend on the pass size.
 * Outputs (any may be NULL), series i + N h, per scale s:
 *   median    [nscales][5][H N]: fcstYhat, fcstYhat1plus, fcstYhat1minus, IRF1plus, IRF1minus (medians over the
 *             draws of base, plus, minus, plus - base, minus - base);  quantiles [nscales][5][nq][H N] (MATLAB
 *             prctile at pct);
 *   rbMedian  [nscales][2][H N], rbQuantiles [nscales][2][nq][H N] (linear model): YhatRB and IRF1RB
 *             (generateGIRF2linear.m:175-216), every equation one fp64 fma chain over the state ascending;
 *   draws     [nscales][n][3][H][N] (keep != 0): fcstYHATdraws, fcstYHATdraws1plus, fcstYHATdraws1minus;
 *   rbDraws   [nscales][n][2][H][N] (keep != 0, linear model): YhatRBdraws, IRF1RBdraws;
 *   nbad      the draws whose PHI is not positive definite or not finite (their paths are NaN).
 * N <= 32 and K + Ny p + N <= 384.  Returns C (> 0), or a negative error code.  The draw store is left as it is. */
int ccmm_chains_girf(ccmm_chains* ch, int slot, int t0, const double* jump, int H, int nsim, int nscales,
                     const double* shock11, const uint8_t* cumcode, double np_, const uint8_t* ndxYields,
                     uint64_t seed, int draws_per_pass, int nq, const double* pct, int keep, double* median,
                     double* quantiles, double* rbMedian, double* rbQuantiles, double* draws, double* rbDraws,
                     int* nbad);
/* What ccmm_chains_girf feeds the simulation, for every pooled draw: Xj [n][ldX] (ldX = 1 + N p + Ny p), SV0
 * [n][N], sqrtPHI [n][N][N] (column-major per draw, zeros above the diagonal), info [n] (1: PHI not positive
 * definite or not finite, the draw's three outputs NaN); any may be NULL.  Returns C. */
int ccmm_chains_girf_inputs(ccmm_chains* ch, int slot, int t0, const double* jump, const uint8_t* ndxYields,
                            double* Xj, double* SV0, double* sqrtPHI, int* info);

/* Test hook (tests/test_gpu_girf_store.py): overwrites the stored vech(PHI), N (N + 1) / 2 doubles, of stored draw
 * m of chain `chain`, so that a draw whose PHI is not positive definite -- which the sampler never produces --
 * reaches ccmm_chains_girf's screen. */
int ccmm_chains_poke_stored_phi(ccmm_chains* ch, int chain, int m, const double* vech);

/* ------------------------------------------------------------ diagnostics */

/* psrf(X) of DiagnosticsShadowrate.m:34-128 (== Diagnostics.m:28; Brooks & Gelman 1998, square-root
 * form): X n x D x M, M sequences of n draws of D variables; M == 1 splits the one chain into its
 * first and last floor(n/3) draws (:82-91).  R out: D.  Host computation.  CCMM_ERR_ARG "Too few
 * samples" as :103-105 when a sequence would be empty. */
int ccmm_psrf(int n, int D, int M, const double* X, double* R);

/* shadowratePSRF(:, vintage) of goVARshadowrateBlockHybrid.m:322-325 (goVARhybrid.m:322-323,
 * goVARshadowrate.m:332-333): for each shadow rate s, DiagnosticsShadowrate(shadowrate_all(:, s,
 * ELBdummy(startELB:thisT, s))) = the mean of psrf over the rate's censored months (NaN when there
 * are none).  draws M x Ns x ldT x C (the kept shadow rates of C chains; the first elbT months are
 * the vintage's window), mask Ns x elbT (ELBdummy(startELB:thisT, :)', = elb.sNaN).  The reference's
 * one-chain statistic (first / last thirds, :82-91) for every chain, averaged over the C chains, so the
 * value keeps the reference's meaning for any C.  out: Ns (NaN where psrf would stop with 'Too few
 * samples': M < 3).  The
 * reference's DiagnosticsShadowrate also evaluates ineff() (momentg), which errors below 100 draws
 * (Diagnostics.m momentg 'needs a larger number of ndraws'); its result is not an output and the
 * check is not reproduced. */
int ccmm_shadowrate_psrf(int M, int Ns, int elbT, int ldT, int C, const double* draws, const uint8_t* mask,
                         double* out);
/* The multi-chain form (no reference counterpart; parity unpinned beyond the psrf formula): per cell,
 * psrf over the C chains as its M-draw sequences (Brooks-Gelman across chains), averaged over the rate's
 * months at the ELB as ccmm_shadowrate_psrf.  out: Ns, NaN when C < 2 or M < 2. */
int ccmm_shadowrate_psrf_chains(int M, int Ns, int elbT, int ldT, int C, const double* draws, const uint8_t* mask,
                                double* out);

/* Compute_diagnostics (goVARshadowrateBlockHybrid.m:55-56, :313-316): Diagnostics.m per series of kept draws.
 * 11 statistics per series, in this order:
 *   pmean, pstd, nse, rne, nse1, rne1, nse2, rne2, nse3, rne3  momentg (Diagnostics.m:134-300): Geweke's
 *     numerical standard errors and relative numerical efficiencies, iid and at 4 / 8 / 15 % tapers, from
 *     NG = 100 groups of ns = floor(M / 100) draws (draws beyond 100 ns are ignored, :190-191);
 *     pstd, nse* = -1 where the variance estimate is not positive (:235-236, :243, :282-283)
 *   psrf  the one-chain form of psrf (:75-85, :95-122): first against last floor(M / 3) draws
 * The inefficiency factors of ineff (:129-132) are 1 / rne1, 1 / rne2, 1 / rne3.  A constant series gives
 * pstd = -1 and NaN rne* and psrf (0 / 0), as the reference's arithmetic does.  The device kernel
 * (k_diag_series: one lane per series, one coalesced pass over the draws, the 100 group means in LDS) and the
 * host twin run the same operations in the same order and return the same bits. */
#define CCMM_DIAG_NSTAT 11
/* Host twin, no context and no GPU, at most 16 threads.  Series s, draw m at draws[m * ld_draw +
 * s * ld_series]; out 11 x S, statistic k of series s at out[k * S + s].  M < 100: CCMM_ERR_ARG "momentg: needs
 * a larger number of ndraws" (:185-187). */
int ccmm_diagnostics_host(int M, int S, long long ld_draw, long long ld_series, const double* draws, double* out);
/* host draws, MATLAB layout ndraw x nvar (column-major, series s at draws + s*M), uploaded in series blocks of
 * a fixed scratch; out 11 x S as ccmm_diagnostics_host(M, S, 1, M, ..), bit for bit */
int ccmm_diagnostics(ccmm_ctx* ctx, int M, int S, const double* draws, double* out /* 11 x S */);
/* the stored draws of the chains bound to data slot `slot`, read in place; the store is left as it is.
 * Needs ccmm_chains_stored >= 100 and the slot's chains contiguous (c0 .. c0 + C - 1).  source: 0 PAI
 * (S = K N), 1 PHI (S = N (N + 1) / 2), 2 invA (S = N N; the caller selects the free elements,
 * Diagnostics.m:19), 3 sqrtht (S = T N with T of the chain config, t fastest; rows t >= T of the slot are not
 * computed), 4 shadow rates (shadow-rate models; S = Ns elbTmax, rate fastest; only the cells of the slot's
 * sNaN within its elbT are computed, the cells DiagnosticsShadowrate looks at).  Entries that are not
 * computed are NaN in all 11 statistics.  out[(k * C + c) * S + e]: statistic k, chain c0 + c, entry e, with
 * room for 11 * C * S doubles (C <= B).  Returns C. */
int ccmm_chains_diagnostics(ccmm_chains* ch, int source, int slot, double* out);

/* Predictive density of one kept draw per chain, batched over B chains.
 * Replaces the doPredictiveDensity block mcmcVAR.m:298-381 (same simulation in
 * mcmcVARshadowrateBlockHybrid.m:550-669), including logscoreGaussian.m:15-20 and
 * logscoreGaussianCensored.m:13-88.  Companion form with K = N*p + 1
 * (mcmcVAR.m:108-115).
 *   PAI K x N x B, invA N x N x B, logSV0 N x B (= Vol_states(end,:)', log
 *   variances), sqrtPHI N x N x B, Xjumpoff K x B, yrealized N (first column),
 *   ndxYields N (1 = yield, censored at elb), svz N x (H*Nd) x B (mcmcVAR.m:302)
 *   and z N x H x Nd x B (:306) or both NULL (Philox, block CCMM_RNG_FCST,
 *   counter sweep = `sweep`).
 * Outputs: fcstY, fcstYcensor N x H x Nd x B (fcstYdraws / fcstYcensorDraws),
 *   yhat N x H x B (yhatdraws), scores 4 x Nd x B = (fcstLogscoreDraws,
 *   fcstLogscoreELBdraws, fcstLogscoreXdraws, fcstLogscoreIdraws).
 * Returns CCMM_WARN_MVNCDF when some censored score needed mvncdf in more than 12
 * dimensions (that score is NaN; status[c] bit 1 marks the chain). */
int ccmm_fcst(ccmm_ctx* ctx, int B, int N, int p, int H, int Nd, const double* PAI,
              const double* invA, const double* logSV0, const double* sqrtPHI,
              const double* Xjumpoff, const double* yrealized, const uint8_t* ndxYields,
              double elb, const double* svz, const double* z, uint64_t seed, int sweep,
              double* fcstY, double* fcstYcensor, double* yhat, double* scores, int* status);
/* ccmm_fcst (N <= 32) on the kernels of the large-N path: 1 <= N <= 128, K = N*p + 1 <= 1536, same arguments,
 * same outputs, the same normals in Philox mode; the sums of the companion recursion and of the scores run in
 * another order, so the outputs agree with ccmm_fcst to rounding, not bit for bit. */
int ccmm_fcst_big(ccmm_ctx* ctx, int B, int N, int p, int H, int Nd, const double* PAI,
                  const double* invA, const double* logSV0, const double* sqrtPHI,
                  const double* Xjumpoff, const double* yrealized, const uint8_t* ndxYields,
                  double elb, const double* svz, const double* z, uint64_t seed, int sweep,
                  double* fcstY, double* fcstYcensor, double* yhat, double* scores, int* status);
/* ccmm_fcst with the doIRF1 simulations of mcmcVARshadowrate.m:588-605: the linear recursion (ltitr) twice more
 * on the draw's shocks, the structural shock of variable 1 (index 0) at horizon 1 replaced by +irf1scale and by
 * -irf1scale.  fcstY1plus, fcstY1minus N x H x Nd x B (fcstYdraws1plus / fcstYdraws1minus as simulated, laid out
 * like fcstY).  Every output of ccmm_fcst is the one ccmm_fcst returns on the same inputs. */
int ccmm_fcst_irf1(ccmm_ctx* ctx, int B, int N, int p, int H, int Nd, const double* PAI, const double* invA,
                   const double* logSV0, const double* sqrtPHI, const double* Xjumpoff, const double* yrealized,
                   const uint8_t* ndxYields, double elb, const double* svz, const double* z, uint64_t seed, int sweep,
                   double* fcstY, double* fcstYcensor, double* yhat, double* scores, int* status, double irf1scale,
                   double* fcstY1plus, double* fcstY1minus);

/* D16x16 = A16x4 * B4x16 computed by one v_mfma_f64_16x16x4_f64 with the operand
 * and accumulator lane maps the CTA SYRK kernel relies on (all column-major). */
int ccmm_selftest_mfma_f64(ccmm_ctx* ctx, const double* A16x4, const double* B4x16, double* D16x16);
/* nprobe independent D = C + A B (one v_mfma_f64_16x16x4_f64 each, caller-given accumulator),
 * probe q at A16x4 + 64 q, B4x16 + 64 q, C16x16 / D16x16 + 256 q: measures the instruction's
 * internal summation order and rounding points (tools/probe_mfma_order.py). */
int ccmm_selftest_mfma_f64_acc(ccmm_ctx* ctx, int nprobe, const double* A16x4, const double* B4x16,
                               const double* C16x16, double* D16x16);

#ifdef __cplusplus
}
#endif
#endif /* CCMM_H */

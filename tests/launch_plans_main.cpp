// Prints the launch plans and LDS layouts that the library's headers compute, one line per query read
// from standard input (tests/test_launch_plans.py).  Host code only: no HIP runtime call.
//
//   cond N p Ns                -> threads a_lds kb lds
//   waves elbTmax Ns want      -> W
//   prep N p elbTmax B         -> lds phi_lds rows wg
//   wf elbTmax Ns W            -> bytes, then name:offset of every region in layout order
//   mp elbTmax Ns WPC          -> the same for k_elb_gibbs_mp
//   oct elbTmax Ns             -> the same for k_elb_gibbs_oct
//   draw1 W elbTmax nmax res   -> the same for k_ps_draw1
//   misc N K KP TP dPHI        -> n_bucket, the A-step and PHI plans, whether the other kernels' LDS fits a CU
//   phi N TP dPHI mask         -> the LDS bytes and stage bits launch_phi takes with option phi_stage = mask
//   fcst N p H bh reg_opt      -> fcst_reg_path, fcst_chunk (register form, LDS form), the k_fcst<RN> instance and the
//                                 chunk and LDS bytes launch_fcst takes with option fcst_reg = reg_opt (Kx = N p + 1)
//   girf N p Ny generic        -> girf_plan: fast NY4 (-1: table-driven), k_girf<KS> bucket, nks, threads, LDS bytes
//   girfg N p nks              -> bytes, then name:offset of every region of k_girf<KS>
//   girff N NY4                -> the same for k_girf_fast<12, 20, NY4>
//   philox idx chain sweep block seedlo seedhi -> the four output words (hex) of Rng::raw(block, idx >> 1), the
//                                 counter and key of the library's Philox4x32-10 normals and uniforms
//   bign N TP                  -> bign_astep_npad, the LDS bytes of k_astep_big, k_astep_fin, k_phi_big and k_sv_big,
//                                 bign_sv_scratch (doubles per chain)
//   bsolve N p K KP TP twin ncol -> big_solve_plan: staged, LDS bytes; then big_solve_lds_bytes and
//                                 big_stage_lds_doubles on their own
#include <cstdio>
#include <cstring>

#include "ccmm_big.h"
#include "ccmm_bign.h"
#include "ccmm_elb.h"
#include "ccmm_fcst.h"
#include "ccmm_girf.h"
#include "ccmm_lag.h"
#include "ccmm_sweep.h"

using namespace ccmm;

static void wave(const ElbWaveLds& l) {
  std::printf("%zu Sl:%zu Ul:%zu Zl:%zu Tm:%zu reach:%zu prog:%zu spare:%zu\n", l.end, l.Sl, l.Ul, l.Zl, l.Tm,
              l.reach, l.prog, l.spare);
}

int main() {
  char cmd[16];
  int a, b, c, d, e, f, g;
  unsigned u[6];
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "cond") && std::scanf("%d %d %d", &a, &b, &c) == 3) {
      const ElbCondPlan pl = elb_cond_plan(a, b, c);
      std::printf("%d %d %d %zu\n", pl.threads, pl.a_lds, pl.kb, pl.lds);
    } else if (!std::strcmp(cmd, "waves") && std::scanf("%d %d %d", &a, &b, &c) == 3) {
      std::printf("%d\n", elb_gibbs_waves(a, b, c));
    } else if (!std::strcmp(cmd, "prep") && std::scanf("%d %d %d %d", &a, &b, &c, &d) == 4) {
      const ElbPrepPlan pl = elb_prep_plan(a, b, c, d);
      std::printf("%zu %d %d %d\n", pl.lds, pl.phi_lds, pl.rows, pl.wg);
    } else if (!std::strcmp(cmd, "wf") && std::scanf("%d %d %d", &a, &b, &c) == 3) {
      wave(elb_wf_lds(a, b, c));
    } else if (!std::strcmp(cmd, "mp") && std::scanf("%d %d %d", &a, &b, &c) == 3) {
      wave(elb_mp_lds(a, b, c));
    } else if (!std::strcmp(cmd, "oct") && std::scanf("%d %d", &a, &b) == 2) {
      const ElbOctLds l = elb_oct_lds(a, b);
      std::printf("%zu Sl:%zu Tm:%zu reach:%zu\n", l.end, l.Sl, l.Tm, l.reach);
    } else if (!std::strcmp(cmd, "draw1") && std::scanf("%d %d %d %d", &a, &b, &c, &d) == 4) {
      const PsDraw1Lds l = ps_draw1_lds(a, b, c, d);
      std::printf("%zu prow:%zu pb:%zu sL:%zu ybl:%zu zl:%zu Ll:%zu scens:%zu info:%zu cellL:%zu\n", l.end, l.prow,
                  l.pb, l.sL, l.ybl, l.zl, l.Ll, l.scens, l.info, l.cellL);
    } else if (!std::strcmp(cmd, "misc") && std::scanf("%d %d %d %d %d", &a, &b, &c, &d, &e) == 5) {
      const AstepPlan as = astep_plan(a, d);
      const PhiPlan ph = phi_plan(a, d, e);
      // (the last three: whether the generic CTA kernels, the score kernel and the lag solve fit one CU's LDS)
      std::printf("%d %zu %d %zu %d %d %d %d\n", n_bucket(a), as.lds, as.es_off, ph.lds, ph.stage_eta,
                  (int)(std::max(gram_chol_lds_bytes(c / 16), cta_solve2_lds_bytes(a, c, d)) <= kLdsCu &&
                        resid_multi_lds_bytes(a, b) <= kLdsCu),
                  (int)(fcst_scores_lds_doubles(a) * sizeof(double) <= kLdsCu),
                  (int)(sl_lds_bytes(1, d + 8, a + 1, d, n_bucket(a)) <= kLdsCu));
    } else if (!std::strcmp(cmd, "phi") && std::scanf("%d %d %d %d", &a, &b, &c, &d) == 4) {
      const PhiPlan ph = phi_plan(a, b, c, d);
      std::printf("%zu %d\n", ph.lds, ph.stage_eta);
    } else if (!std::strcmp(cmd, "fcst") && std::scanf("%d %d %d %d %d", &a, &b, &c, &d, &e) == 5) {
      const int Kx = a * b + 1;
      const bool reg = fcst_reg_path(a, b, d) && e;
      const int hc = fcst_chunk(a, Kx, b, c, reg);
      std::printf("%d %d %d %d %d %zu\n", (int)fcst_reg_path(a, b, d), fcst_chunk(a, Kx, b, c, true),
                  fcst_chunk(a, Kx, b, c, false), fcst_variant(a, b, d, e != 0), hc,
                  fcst_paths_lds_doubles(a, Kx, b, hc, reg) * sizeof(double));
    } else if (!std::strcmp(cmd, "girf") && std::scanf("%d %d %d %d", &a, &b, &c, &d) == 4) {
      const GirfPlan pl = girf_plan(a, b, c, d != 0);
      std::printf("%d %d %d %d %zu\n", pl.fast_ny4, pl.ks, pl.nks, pl.threads, pl.lds);
    } else if (!std::strcmp(cmd, "girfg") && std::scanf("%d %d %d", &a, &b, &c) == 3) {
      const GirfLds l = girf_lds(a, b, c);
      std::printf("%zu X:%zu logsv:%zu ybuf:%zu nrm:%zu rowtab:%zu\n", l.end, l.X, l.logsv, l.ybuf, l.nrm, l.rowtab);
    } else if (!std::strcmp(cmd, "girff") && std::scanf("%d %d", &a, &b) == 2) {
      const GirfLds l = girf_fast_lds(a, kGirfFastP, kGirfFastN4, b);
      std::printf("%zu X:%zu logsv:%zu ybuf:%zu nrm:%zu\n", l.end, l.X, l.logsv, l.ybuf, l.nrm);
    } else if (!std::strcmp(cmd, "bign") && std::scanf("%d %d", &a, &b) == 2) {
      const Dims dm{a, 1, a + 1, round_up(a + 1, 64), b, 1, a};
      std::printf("%d %zu %zu %zu %zu %zu\n", bign_astep_npad(dm), bign_astep_lds(), bign_astep_fin_lds(a), bign_phi_lds(),
                  bign_sv_lds(a), bign_sv_scratch(dm));
    } else if (!std::strcmp(cmd, "bsolve") && std::scanf("%d %d %d %d %d %d %d", &a, &b, &c, &d, &e, &f, &g) == 7) {
      const Dims dm{a, b, c, d, e, 1, a};
      const BigSolvePlan pl = big_solve_plan(dm, f != 0, g);
      std::printf("%d %zu %zu %zu\n", (int)pl.staged, pl.lds, big_solve_lds_bytes(dm), big_stage_lds_doubles(dm, g));
    } else if (!std::strcmp(cmd, "philox") && std::scanf("%u %u %u %u %u %u", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5]) == 6) {
      Rng rng{};
      rng.seed = ((uint64_t)u[5] << 32) | u[4];
      rng.chain = u[1];
      rng.sweep = u[2];
      const u32x4 r = rng.raw((int)u[3], u[0] >> 1);
      std::printf("%08x %08x %08x %08x\n", r.x, r.y, r.z, r.w);
    } else {
      std::fprintf(stderr, "bad query: %s\n", cmd);
      return 2;
    }
  }
  return 0;
}

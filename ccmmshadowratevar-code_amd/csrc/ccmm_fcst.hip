// Predictive density of one kept draw per chain (mcmcVAR.m:298-381,
// mcmcVARshadowrateBlockHybrid.m:550-669): SV shock paths, the linear companion
// simulation (ltitr), the censored simulation, the Rao-Blackwellised mean path
// and the one-step predictive log scores (logscoreGaussian.m,
// logscoreGaussianCensored.m).
//
// k_fcst: one single-wave workgroup per (forecast draw nn, chain), plus one for the linear
// model's zero-shock mean path: PAI (Kx x N) staged in LDS, the lag state a ring of p blocks of N
// values in LDS (the companion shift x(1+N+r) <- x(1+r) becomes a head-pointer move), the shock
// side of the simulation formed ahead of the recursion in chunks of horizons.  k_fcst_scores: the
// four one-step log scores of each draw, one single-wave workgroup per (draw, chain), over an
// N x N LDS scratch (N <= 32): ~N^3 flop per draw.
#include <stdexcept>

#include "ccmm_fcst_dev.h"  // the normal cdfs, the mvncdf rules and censored_llf2 (shared with ccmm_fcst_big.hip)

namespace ccmm {

// The lattice rule of mvn_lattice_cdf (moved to ccmm_fcst_dev.h with the other mvncdf rules, which k_fcst_scores_big
// shares) stays written out in this unit, where tests/test_oracle_fcst.py reads its generators and point count;
// the compiler holds both equal to what the shared function uses.
namespace lattice_rule {
constexpr int kMvnPts = 64 * 1024;
constexpr const double alpha[kMvnMaxD - 1] = {1.4142135623730951, 1.7320508075688772, 2.2360679774997898,
                                              2.6457513110645907, 3.3166247903554, 3.605551275463989,
                                              4.123105625617661, 4.358898943540674, 4.795831523312719,
                                              5.385164807134504, 5.5677643628300215};
constexpr bool same_generators() {
  for (int i = 0; i < kMvnMaxD - 1; ++i)
    if (alpha[i] != kMvnAlpha[i]) return false;
  return true;
}
static_assert(kMvnPts == ccmm::kMvnPts && same_generators(), "the lattice rule written out here is not the one in use");
}  // namespace lattice_rule

// in-place lower Cholesky of an n x n LDS matrix (ld = kFcstMaxN); false if not SPD.
// Called by all 64 lanes of a wave with identical arguments: lane r computes row j + 1 + r
// of column j (n <= 32: one pass), every entry with the same operation order as the
// serial column-by-column form, so the factor is bit-identical to it.
__device__ bool chol_lds(double* M, int n, int lane) {
  for (int j = 0; j < n; ++j) {
    double s = M[j + j * kFcstMaxN];
    for (int k = 0; k < j; ++k) s -= M[j + k * kFcstMaxN] * M[j + k * kFcstMaxN];
    if (!(s > 0.0)) return false;
    const double dj = sqrt(s);
    const int i = j + 1 + lane;
    double v = 0.0;
    if (i < n) {
      v = M[i + j * kFcstMaxN];
      for (int k = 0; k < j; ++k) v -= M[i + k * kFcstMaxN] * M[j + k * kFcstMaxN];
      v = v / dj;
    }
    wave_lds_sync();
    if (lane == 0) M[j + j * kFcstMaxN] = dj;
    if (i < n) M[i + j * kFcstMaxN] = v;
    wave_lds_sync();
  }
  return true;
}

// Omega = S(rows) S(rows)' for the index list rows[0..n) of S = invA diag(sv) (lower
// triangular): M = chol(Omega, 'lower') (the chol(sqrtOmega(ndx,:)*sqrtOmega(ndx,:)')
// of mcmcVAR.m:342,347 and logscoreGaussianCensored.m:54-56).  Lanes split the Gram
// entries (same k order per entry as the serial loop).
__device__ bool gram_rows_chol(const double* invA, const double* sv, const int* rows, int n,
                               int N, double* M, int lane) {
  wave_lds_sync();
  for (int e = lane; e < n * n; e += 64) {
    const int a = e / n, b = e - a * n;
    if (b > a) continue;
    const int ra = rows[a], rb = rows[b];
    const int kmax = ra < rb ? ra : rb;
    double s = 0.0;
    for (int k = 0; k <= kmax; ++k) s += invA[ra + k * N] * invA[rb + k * N] * sv[k] * sv[k];
    M[a + b * kFcstMaxN] = s;
    M[b + a * kFcstMaxN] = s;
  }
  wave_lds_sync();
  return chol_lds(M, n, lane);
}

// logscoreGaussian.m:15-20 with lower-triangular L (ld kFcstMaxN), dev = y - mu (overwritten)
__device__ double score_gauss(const double* L, int n, double* dev, double logdet) {
  double ss = 0.0;
  for (int i = 0; i < n; ++i) {
    double v = dev[i];
    for (int k = 0; k < i; ++k) v -= L[i + k * kFcstMaxN] * dev[k];
    v /= L[i + i * kFcstMaxN];
    dev[i] = v;
    ss += v * v;
  }
  return -0.5 * (n * 1.8378770664093454836 + logdet + ss);
}

__device__ double logdet_chol(const double* L, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += log(L[i + i * kFcstMaxN]);
  return 2.0 * s;
}

// logscoreGaussianCensored.m:13-88 as written.  sel[0..n) = the series scored (in
// order), cens[i] whether series sel[i] may be censored.  Four or more series at the ELB: the
// deterministic lattice estimate above (MATLAB mvncdf's randomised QMC, tolerance 1e-4); NaN (and
// *unsupported) above kMvnMaxD.
__device__ double score_censored(const double* invA, const double* sv, const double* mu,
                                 const double* y, const int* sel, const uint8_t* cens, int n,
                                 int N, double elb, double* M, double* dev, int* order,
                                 const GLNodes& gl, bool* unsupported, int lane) {
  int noff = 0, nat = 0;
  for (int i = 0; i < n; ++i)
    if (!(cens[i] && y[sel[i]] <= elb)) order[noff++] = sel[i];
  for (int i = 0; i < n; ++i)
    if (cens[i] && y[sel[i]] <= elb) { order[noff + nat] = sel[i]; ++nat; }
  if (nat > kMvnMaxD) { *unsupported = true; return NAN; }
  if (!gram_rows_chol(invA, sv, order, n, N, M, lane)) return NAN;
  double llf1 = 0.0;
  double y21[kMvnMaxD], yat[kMvnMaxD];
  for (int a = 0; a < nat; ++a) { y21[a] = mu[order[noff + a]]; yat[a] = y[order[noff + a]]; }
  if (noff > 1) {
    for (int i = 0; i < noff; ++i) dev[i] = y[order[i]] - mu[order[i]];
    llf1 = score_gauss(M, noff, dev, logdet_chol(M, noff));  // dev now z1
    for (int a = 0; a < nat; ++a)
      for (int k = 0; k < noff; ++k) y21[a] += M[(noff + a) + k * kFcstMaxN] * dev[k];
  }
  return llf1 + censored_llf2(nat, yat, y21, M + noff + noff * kFcstMaxN, gl, lane);
}

// Linear model (mcmcVAR.m:298-381): ring l = the linear simulation, ring c = the
// censored simulation (yields floored inside the recursion, :354-372), plus the
// zero-shock mean path.  Block hybrid (mcmcVARshadowrateBlockHybrid.m:566-625): ONE
// simulation on the Nstates = K + Nyields p state; ring l holds the shadow lags, ring c
// the same lags with every yield replaced by its actual rate max(y, ELB) (:623, the
// actual-rate states fcstX0(ndxfcstActual)); the actual-rate equations read ring c (their
// PAIactual on the yield lags, PAIshadow zero there: :567-574), the others ring l.
//
// k_fcst: one single-wave workgroup per (forecast draw, chain) -- job Nd is the linear model's
// zero-shock mean path.  The shock side of the simulation does not depend on the simulated
// path, so it is formed for a chunk of hc horizons at once by all 64 lanes before the
// recursion: the SV normals and their sqrtPHI products, the log-volatility random walk
// (mcmcVAR.m:302-312), the structural shocks w = sv .* z and their impact nu = invA w.  The
// recursion itself (one horizon after the other) then only carries the companion product
// fcstA * state, its 2 N p lag products spread over G lane groups (lane = i + N g takes the lags
// l = g mod G) whose partials lane i adds by shuffles.  The draw's SV at horizon 1 goes to
// a.sv1 for k_fcst_scores.
//

// IRF (doIRF1: BlockHybrid.m:627-664, mcmcVARhybridGibbs.m:638-675, mcmcVARshadowrate.m:588-605): the draw's
// simulation twice more on the same shocks, w(1,1) = +a.irfScale and -a.irfScale; only horizon 1's nu = invA w
// differs.  The three recursions (r = 0 baseline, 1 plus, 2 minus) run interleaved in the wave, horizon by horizon,
// on the same coefficients, Xj, NUb and syncs, each on a ring pair and accumulators of its own (layout:
// ccmm_fcst.h fcst_irf_lds_doubles).  Block hybrid / hybrid: the baseline's recursion with max(shadow, ELB) in the
// actual-rate ring; linear: the unfloored recursion only (ltitr, mcmcVARshadowrate.m:596, 602).  The baseline's
// operations and their order are those of the plain form.
template <int RN, bool IRF = false>
__global__ __launch_bounds__(64, 2) void k_fcst(FcstArgs a) {
  extern __shared__ double sm[];
  const int job = blockIdx.x, c = blockIdx.y;
  const int N = a.N, K = a.K, p = a.p, H = a.H, Nd = a.Nd, Kx = a.Kx, hc = a.hc;
  const int lane = threadIdx.x;
  const int njobs = a.bh ? Nd : Nd + 1;
  if (job >= njobs) return;
  const bool mean_path = job == Nd;
  constexpr bool REG = RN > 0;
  constexpr int NR = IRF ? 3 : 1;  // recursions of the job
  double* sPAI = sm;                          // Kx x N (column i = equation i); none when REG
  double* sSq = sPAI + (REG ? 0 : (size_t)Kx * N);  // sqrtPHI, N x N column-major
  double* sinvA = sSq + N * N;                // invA, N x N column-major
  double* ringl = sinvA + N * N;              // p x N
  double* ringc = ringl + p * N;              // p x N
  double* Wb = ringc + p * N;                 // hc x N: zz, then w = sv .* zz
  double* NUb = Wb + (size_t)hc * N;          // hc x N: sqrtPHI dev, then nu = invA w
  double* DVb = NUb + (size_t)hc * N;         // hc x N: the SV normals dev
  const int sl = a.slot ? a.slot[c] : 0;
  const bool hy = a.bh == 2;
  const double* PAIc = a.PAI + (size_t)c * a.ldPAI * N;
  if (!REG)
    for (int e = lane; e < Kx * N; e += 64) {
      const int j = e / Kx, k = e - j * Kx;
      sPAI[e] = PAIc[(size_t)j * a.ldPAI + k];
    }
  const double* Xj = a.Xj + (size_t)c * a.ldXj;
  for (int e = lane; e < N * N; e += 64) {
    sinvA[e] = a.invA[(size_t)c * N * N + e];
    sSq[e] = a.sqrtPHI[(size_t)c * N * N + e];
  }
  int hs[kElbNsMax] = {-1, -1, -1, -1, -1};  // hybrid: indices of the shadow-rate variables
  if (hy)
    for (int q = 0; q < a.Ns && q < kElbNsMax; ++q) hs[q] = a.ndxS[q];
  const int tsv = a.svT ? a.svT[sl] - 1 : 0;
  const double* svz = a.svz ? a.svz + (size_t)c * a.crnStride : nullptr;
  const double* zc = a.z ? a.z + (size_t)c * a.crnStride : nullptr;
  const bool isact = a.bh == 1 && lane < N && a.actual[lane];
  const bool isyield = lane < N && a.ndxYields[lane];
  const bool isrec = lane < N && (a.recFloor ? a.recFloor[lane] : a.ndxYields[lane]);
  Rng rng;
  rng.crn = nullptr;
  rng.seed = a.seed;
  rng.chain = a.ids ? a.ids[c] : (uint32_t)c;
  rng.sweep = a.sweep;
  const int nsv = N * H * Nd;
  // IRF: the plus and minus rings, p x N each (linear: ringl only, rC[r] is not read)
  double* rL[NR];
  double* rC[NR];
  rL[0] = ringl;
  rC[0] = ringc;
  const bool dual = !IRF || a.bh != 0;  // recursions 1, 2 carry an actual-rate ring
#pragma unroll
  for (int r = 1; r < NR; ++r) {
    rL[r] = DVb + (size_t)hc * N + (size_t)(r - 1) * (a.bh ? 2 : 1) * p * N;
    rC[r] = a.bh ? rL[r] + p * N : rL[r];
  }
  // ring blocks: slot (head - l) mod p holds lag l+1 (l = 0..p-1)
  for (int e = lane; e < p * N; e += 64) {
    const int l = e / N, j = e - l * N;  // lag l+1 goes to slot (-l) mod p
    const int slot = (l == 0) ? 0 : p - l;
    ringl[slot * N + j] = Xj[1 + e];
    // block hybrid: yields carry their actual-rate lags (Xjumpoff(K+1:end), :93-96);
    // hybrid: the shadow-rate variables carry theirs (Xjumpoff(Kshadow+1:end), :111-121)
    double cv = Xj[1 + e];
    if (a.bh == 1 && a.ndxYields[j]) cv = Xj[K + e];
    if (hy)
      for (int q = 0; q < a.Ns && q < kElbNsMax; ++q)
        if (hs[q] == j) cv = Xj[K + l * a.Ns + q];
    ringc[slot * N + j] = cv;
#pragma unroll
    for (int r = 1; r < NR; ++r) {  // the same jump-off (fcstX0 = Xjumpoff, :632, 648)
      if (a.bh) rC[r][slot * N + j] = cv;
      rL[r][slot * N + j] = Xj[1 + e];
    }
  }
  double nu1[NR];  // IRF: nu(lane) of horizon 1 in the plus / minus run (lanes < N)
#pragma unroll
  for (int r = 0; r < NR; ++r) nu1[r] = 0.0;
  double logsv = (lane < N) ? a.logSV[((size_t)c * N + lane) * a.ldSV + tsv] : 0.0;
  const int G = N <= 21 ? 3 : (N <= 32 ? 2 : 1);  // lane groups of the lag sums (G N <= 64)
  const int g = lane / N, gi = lane - g * N;
  const double* pcol = sPAI + (size_t)(g < G ? gi : 0) * Kx;
  // REG: lane (gi, g) holds PAI(1 + l N + j, gi) for its lags l = g + G m, and the intercept
  double cf[REG ? kFcstRegLags : 1][REG ? RN : 1];
  double c0 = 0.0;
  if (REG) {
    const double* pg = PAIc + (size_t)(g < G ? gi : 0) * a.ldPAI;
    c0 = pg[0];
#pragma unroll
    for (int m = 0; m < (REG ? kFcstRegLags : 1); ++m) {
      const int l = g + G * m;
#pragma unroll
      for (int j = 0; j < (REG ? RN : 1); ++j)
        cf[m][j] = (g < G && l < p && j < N) ? pg[1 + l * N + j] : 0.0;
    }
  }
  int head = 0;
  __syncthreads();
  for (int h0 = 0; h0 < ((a.mode & kFcstNoHorizons) ? 0 : H); h0 += hc) {
    const int nh = min(hc, H - h0);
    if (!mean_path) {
      // SV normals randn(N, H*Nd) column hh + job H (mcmcVAR.m:302) and the shock normals
      // randn(N, H, Nd) (:306) of the chunk's horizons
      for (int q = lane; q < nh * N; q += 64) {
        const int hh = h0 + q / N, i = q - (q / N) * N;
        const int col = hh + job * H;
        DVb[q] = svz ? svz[(size_t)col * N + i] : rng.normal(CCMM_RNG_FCST, (uint32_t)(col * N + i));
        const size_t zi = ((size_t)job * H + hh) * N + i;
        Wb[q] = zc ? zc[zi] : rng.normal(CCMM_RNG_FCST, (uint32_t)(nsv + zi));
      }
      wave_lds_sync();
      for (int q = lane; q < nh * N; q += 64) {  // sqrtPHI * dev, j in order
        const int hq = q / N, i = q - hq * N;
        const double* dv = DVb + (size_t)hq * N;
        double shock = 0.0;
        for (int j = 0; j < N; ++j) shock = fma(sSq[i + j * N], dv[j], shock);
        NUb[q] = shock;
      }
      wave_lds_sync();
      if (lane < N)  // the log-volatility random walk and w = sv .* z
        for (int hq = 0; hq < nh; ++hq) {
          logsv += NUb[hq * N + lane];
          const double sv = exp(logsv * 0.5);
          Wb[hq * N + lane] *= sv;
          if (h0 + hq == 0) a.sv1[((size_t)c * Nd + job) * N + lane] = sv;
        }
      wave_lds_sync();
      for (int q = lane; q < nh * N; q += 64) {  // nu = invA w (invA unit lower, j = 0..i)
        const int hq = q / N, i = q - hq * N;
        const double* wv = Wb + (size_t)hq * N;
        double nu = 0.0;
        for (int j = 0; j <= i; ++j) nu = fma(sinvA[i + j * N], wv[j], nu);
        NUb[q] = nu;
      }
      wave_lds_sync();
      if (IRF && h0 == 0 && lane < N) {  // horizon 1: nushocks(1,1,nn) = +-IRF1scale, then invA_ * nushocks (:630-631, 646-647)
#pragma unroll
        for (int r = 1; r < NR; ++r) {
          const double w0 = r == 1 ? a.irfScale : -a.irfScale;
          double nu = 0.0;
          for (int j = 0; j <= lane; ++j) nu = fma(sinvA[lane + j * N], j == 0 ? w0 : Wb[j], nu);
          nu1[r] = nu;
        }
      }
    }
    for (int hq = 0; hq < nh; ++hq) {
      const int hh = h0 + hq;
      // fcstA * state on the lane groups
      double sl2[NR], sc[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) sl2[r] = sc[r] = 0.0;
      if (REG) {
        if (g < G) {
          if (g == 0) {
#pragma unroll
            for (int r = 0; r < NR; ++r) sl2[r] = sc[r] = Xj[0] * c0;
          }
#pragma unroll
          for (int m = 0; m < (REG ? kFcstRegLags : 1); ++m) {
            const int l = g + G * m;
            if (l < p) {
              int slot = head - l;
              slot += (slot < 0) ? p : 0;
              const double* rl[NR];
              const double* rc[NR];
#pragma unroll
              for (int r = 0; r < NR; ++r) {
                rl[r] = rL[r] + slot * N;
                rc[r] = rC[r] + slot * N;
              }
              if (RN % 2 == 0) {  // N even: the ring rows are 16-byte aligned, two lags' entries a read
#pragma unroll
                for (int j = 0; j < (REG ? RN : 1); j += 2)
                  if (j < N) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) {
                      const double2 vl = *reinterpret_cast<const double2*>(rl[r] + j);
                      if (r == 0 || dual) {
                        const double2 vc = *reinterpret_cast<const double2*>(rc[r] + j);
                        sl2[r] = fma(cf[m][j], vl.x, sl2[r]);
                        sc[r] = fma(cf[m][j], vc.x, sc[r]);
                        sl2[r] = fma(cf[m][j + 1], vl.y, sl2[r]);
                        sc[r] = fma(cf[m][j + 1], vc.y, sc[r]);
                      } else {
                        sl2[r] = fma(cf[m][j], vl.x, sl2[r]);
                        sl2[r] = fma(cf[m][j + 1], vl.y, sl2[r]);
                      }
                    }
                  }
              } else {
#pragma unroll
                for (int j = 0; j < (REG ? RN : 1); ++j)
                  if (j < N) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) {
                      sl2[r] = fma(cf[m][j], rl[r][j], sl2[r]);
                      if (r == 0 || dual) sc[r] = fma(cf[m][j], rc[r][j], sc[r]);
                    }
                  }
              }
            }
          }
        }
      } else if (g < G) {
        if (g == 0) {  // constant state stays 1 (fcstA(1,1) = 1)
#pragma unroll
          for (int r = 0; r < NR; ++r) sl2[r] = sc[r] = Xj[0] * pcol[0];
        }
        for (int l = g; l < p; l += G) {
          int slot = head - l;
          slot += (slot < 0) ? p : 0;
          const double* rl[NR];
          const double* rc[NR];
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            rl[r] = rL[r] + slot * N;
            rc[r] = rC[r] + slot * N;
          }
          const double* pc = pcol + 1 + l * N;
#pragma unroll 4
          for (int j = 0; j < N; ++j) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
              sl2[r] = fma(pc[j], rl[r][j], sl2[r]);
              if (r == 0 || dual) sc[r] = fma(pc[j], rc[r][j], sc[r]);
            }
          }
          if (hy)  // fcstA(ndxfcstY, Kshadow+1:end) on the actual-rate ring (:626)
            for (int q = 0; q < a.Ns && q < kElbNsMax; ++q) {
#pragma unroll
              for (int r = 0; r < NR; ++r) sl2[r] = fma(pcol[K + l * a.Ns + q], rc[r][hs[q]], sl2[r]);
            }
        }
      }
      // every group's partial is read before any lane adds (lane i + N is also the source of
      // lane i's group-2 partial through lane i + 2N ... and must still hold its own)
      double pl[NR][2], pcs[NR][2];
#pragma unroll
      for (int r = 0; r < NR; ++r) pl[r][0] = pl[r][1] = pcs[r][0] = pcs[r][1] = 0.0;
      for (int q = 1; q < G; ++q) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          pl[r][q - 1] = __shfl(sl2[r], lane + q * N, 64);
          if (r == 0 || dual) pcs[r][q - 1] = __shfl(sc[r], lane + q * N, 64);
        }
      }
      for (int q = 1; q < G; ++q) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          sl2[r] += pl[r][q - 1];
          sc[r] += pcs[r][q - 1];
        }
      }
      double yl = 0.0, yc = 0.0;
      double yx[NR], ycx[NR];  // IRF: the plus / minus values (entries 1, 2)
#pragma unroll
      for (int r = 0; r < NR; ++r) yx[r] = ycx[r] = 0.0;
      if (lane < N) {
        const double nu = mean_path ? 0.0 : NUb[hq * N + lane];
        if (hy) {
          yl = sl2[0] + nu;
          yc = (isyield && yl < a.elb) ? a.elb : yl;  // yields floored (:707-711); ring: max(shadow, ELB) (:634)
        } else if (a.bh) {
          yl = (isact ? sc[0] : sl2[0]) + nu;         // fcstA * fcstX0 + fcstB * shocks (:615)
          yc = (isyield && yl < a.elb) ? a.elb : yl;  // actual rate max(shadow, ELB) (:623)
        } else {
          yl = sl2[0] + nu;
          yc = sc[0] + nu;
          if (isrec && yc < a.elb) yc = a.elb;        // censored simulation (mcmcVAR.m:360-366)
        }
        if (mean_path) {
          a.yhat[((size_t)c * H + hh) * N + lane] = yl;
        } else {
          const size_t o = (((size_t)c * Nd + job) * H + hh) * N + lane;
          a.fY[o] = yl;
          a.fYc[o] = yc;
          if (IRF) {  // fcstYdraws1plus / fcstYdraws1minus as simulated (:639, 657); linear: no floor inside
#pragma unroll
            for (int r = 1; r < NR; ++r) {
              const double nux = hh == 0 ? nu1[r] : nu;
              yx[r] = (isact ? sc[r] : sl2[r]) + nux;  // (isact: block hybrid only)
              ycx[r] = (isyield && yx[r] < a.elb) ? a.elb : yx[r];
            }
            a.fY1p[o] = yx[IRF ? 1 : 0];
            a.fY1m[o] = yx[IRF ? 2 : 0];
          }
        }
      }
      wave_lds_sync();  // every lane has read the oldest lag block before it is overwritten
      head = (head + 1 == p) ? 0 : head + 1;
      if (lane < N) {
        ringl[head * N + lane] = yl;
        ringc[head * N + lane] = yc;
#pragma unroll
        for (int r = 1; r < NR; ++r) {
          rL[r][head * N + lane] = yx[r];
          if (dual) rC[r][head * N + lane] = ycx[r];
        }
      }
      wave_lds_sync();
    }
  }
}

// One-step predictive log scores of draw `job` of chain c (mcmcVAR.m:326-352; block hybrid
// :577-608), one single-wave workgroup per (draw, chain): every lane runs the same scalar algebra
// (uniform control flow, identical LDS writes); the trivariate mvncdf quadrature and the lattice
// rule spread their nodes over the lanes.  Reads the draw's SV at horizon 1 (a.sv1, k_fcst).

__global__ __launch_bounds__(64) void k_fcst_scores(FcstArgs a) {
  extern __shared__ double sm[];
  const int job = blockIdx.x, c = blockIdx.y;
  const int N = a.N, K = a.K, Kx = a.Kx, Nd = a.Nd;
  const int lane = threadIdx.x;
  if (job >= Nd || (a.mode & kFcstNoScores)) return;
  double* invA = sm;                  // N x N
  double* mu = invA + N * N;          // muY (N)
  double* y = mu + N;                 // yrealized(:,1) (N)
  double* sv1 = y + N;                // SV at horizon 1 (N)
  double* dev = sv1 + N;              // N
  int* order = (int*)(dev + N);       // N ints
  int* sel = (int*)(dev + 2 * N);     // N ints
  uint8_t* cens = (uint8_t*)(sel + N);  // N bytes (same N-double slot)
  double* M = dev + 3 * N;            // kFcstMaxN^2
  int* syl = (int*)(M + kFcstMaxN * kFcstMaxN);  // yield flags (N ints in N doubles)
  const int sl = a.slot ? a.slot[c] : 0;
  for (int e = lane; e < N * N; e += 64) invA[e] = a.invA[(size_t)c * N * N + e];
  if (lane < N) {
    y[lane] = a.yreal[(size_t)sl * a.ldY + lane];
    sv1[lane] = a.sv1[((size_t)c * Nd + job) * N + lane];
    syl[lane] = a.ndxYields[lane];
  }
  __syncthreads();
  // muY = fcstA(ndxfcstY, :) * Xjumpoff (mcmcVAR.m:326-328; block hybrid :577-580: the actual-rate
  // equations read the yields' actual-rate lags)
  const double* Xj = a.Xj + (size_t)c * a.ldXj;
  const double* PAIc = a.PAI + (size_t)c * a.ldPAI * N;
  if (lane < N) {
    const int i = lane;
    const bool act = a.bh == 1 && a.actual[i];
    const double* col = PAIc + (size_t)i * a.ldPAI;
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
      const double xv = (act && k > 0 && syl[(k - 1) % N]) ? Xj[K + k - 1] : Xj[k];
      s += col[k] * xv;
    }
    for (int k = K; k < Kx; ++k) s += col[k] * Xj[k];  // hybrid: actual-rate lags (:592-594)
    mu[i] = s;
  }
  __syncthreads();
  int nx = 0, ni = 0, natelb = 0;
  for (int i = 0; i < N; ++i) {
    if (a.ndxYields[i]) {
      ++ni;
      natelb += (y[i] <= a.elb);
    } else {
      ++nx;
    }
  }
  double sc[4];
  bool unsupported = false;
  // (1) full vector: sqrtOmegaY = invA diag(sv1) is lower triangular, logdet = sum logSV(:,1)
  {
    double ld = 0.0;
    for (int i = 0; i < N; ++i) {
      M[i + i * kFcstMaxN] = sv1[i];  // unit-diagonal invA times sv
      for (int r2 = i + 1; r2 < N; ++r2) M[r2 + i * kFcstMaxN] = invA[r2 + i * N] * sv1[i];
      ld += 2.0 * log(sv1[i]);
      dev[i] = y[i] - mu[i];
    }
    sc[0] = score_gauss(M, N, dev, ld);
  }
  // (2) censored full vector (ndxYIELDS censorable); the block-hybrid fcstLogscoreDraws
  if (natelb > 0) {
    for (int i = 0; i < N; ++i) {
      order[i] = i;
      cens[i] = a.ndxYields[i];
    }
    for (int i = 0; i < N; ++i) sel[i] = i;
    sc[1] = score_censored(invA, sv1, mu, y, sel, cens, N, N, a.elb, M, dev, order, a.gl, &unsupported, lane);
  } else {
    sc[1] = sc[0];
  }
  // (3) macro block
  {
    int q = 0;
    for (int i = 0; i < N; ++i)
      if (!a.ndxYields[i]) sel[q++] = i;
    if (gram_rows_chol(invA, sv1, sel, nx, N, M, lane)) {
      for (int i = 0; i < nx; ++i) dev[i] = y[sel[i]] - mu[sel[i]];
      sc[2] = score_gauss(M, nx, dev, logdet_chol(M, nx));
    } else {
      sc[2] = NAN;
    }
  }
  // (4) yields block: every yield censorable
  {
    int q = 0;
    for (int i = 0; i < N; ++i)
      if (a.ndxYields[i]) {
        sel[q] = i;
        cens[q] = 1;
        ++q;
      }
    if (natelb > 0) {
      sc[3] = score_censored(invA, sv1, mu, y, sel, cens, ni, N, a.elb, M, dev, order, a.gl, &unsupported, lane);
    } else if (gram_rows_chol(invA, sv1, sel, ni, N, M, lane)) {
      for (int i = 0; i < ni; ++i) dev[i] = y[sel[i]] - mu[sel[i]];
      sc[3] = score_gauss(M, ni, dev, logdet_chol(M, ni));
    } else {
      sc[3] = NAN;
    }
  }
  if (lane == 0) {
    for (int q = 0; q < 4; ++q) a.scores[((size_t)c * Nd + job) * 4 + q] = sc[q];
    if (unsupported) atomicOr(&a.status[c], 2);
  }
}

// Xjumpoff of every chain from its resident data (mcmcVAR.m:108-115;
// mcmcVARshadowrateBlockHybrid.m:511-520): [1, y(T), ..., y(T-p+1)] from the chain's Y
// slab (block hybrid: the shadow-rate data), then p blocks of N lags of the slot's
// actual data (the block-hybrid actual-rate states, data(Nobs-(l-1), ndxYIELDS)).
// Hybrid (Ns > 0): the tail holds p blocks of the Ns shadow-rate variables' actual data floored at
// the ELB, XjumpoffActualYieldLags (mcmcVARhybridGibbs.m:111-121, 536).
__global__ void k_fcst_jumpoff(int N, int p, int K, int TP, const int* __restrict__ Tslot,
                               const int* __restrict__ slot, const double* __restrict__ ypool,
                               const int* __restrict__ yidx, int ldXj, double* __restrict__ Xj, int Ns,
                               const int* __restrict__ ndxS, double elb) {
  const int c = blockIdx.x;
  const int s = slot[c];
  const int T = Tslot[s];
  const double* Ych = ypool + (size_t)yidx[c] * N * TP;
  const double* Ysl = ypool + (size_t)s * N * TP;
  for (int e = threadIdx.x; e < ldXj; e += blockDim.x) {
    double v = 1.0;
    if (e > 0 && e < K) {
      const int q = e - 1, l = q / N, i = q - l * N;
      v = Ych[(size_t)i * TP + T - 1 - l];
    } else if (e >= K && Ns > 0) {
      const int q = e - K, l = q / Ns, si = q - l * Ns;
      v = 0.0;
      if (l < p) {
        const double yv = Ysl[(size_t)ndxS[si] * TP + T - 1 - l];
        v = yv < elb ? elb : yv;
      }
    } else if (e >= K) {
      const int q = e - K, l = q / N, i = q - l * N;
      v = Ysl[(size_t)i * TP + T - 1 - l];
    }
    Xj[(size_t)c * ldXj + e] = v;
  }
}

// Per kept draw: running sums of the paths over the Nd draws (the means of
// mcmcVAR.m:400-414 / BlockHybrid.m:693-742), the score draws into the store at index m
// (fcstLogscore*Draws(:, thisMCMCdraw)), and optionally the paths themselves.
__global__ void k_fcst_accum(int N, int H, int Nd, int cap, int m, const double* __restrict__ fY,
                             const double* __restrict__ fYc, const double* __restrict__ yhat,
                             const double* __restrict__ sc, double* __restrict__ sum,
                             double* __restrict__ sumc, double* __restrict__ sumhat,
                             double* __restrict__ scStore, double* __restrict__ paths,
                             double* __restrict__ pathsc) {
  const int c = blockIdx.x;
  const size_t HN = (size_t)H * N, per = (size_t)Nd * HN;
  const double* y = fY + (size_t)c * per;
  const double* yc = fYc + (size_t)c * per;
  for (size_t q = threadIdx.x; q < HN; q += blockDim.x) {
    double a = 0.0, b = 0.0;
    for (int job = 0; job < Nd; ++job) {
      a += y[(size_t)job * HN + q];
      b += yc[(size_t)job * HN + q];
    }
    sum[(size_t)c * HN + q] += a;
    sumc[(size_t)c * HN + q] += b;
    if (yhat) sumhat[(size_t)c * HN + q] += yhat[(size_t)c * HN + q];
  }
  for (int q = threadIdx.x; q < Nd * 4; q += blockDim.x)
    scStore[((size_t)c * cap + m) * Nd * 4 + q] = sc[(size_t)c * Nd * 4 + q];
  if (paths)
    for (size_t q = threadIdx.x; q < per; q += blockDim.x) {
      paths[((size_t)c * cap + m) * per + q] = y[q];
      pathsc[((size_t)c * cap + m) * per + q] = yc[q];
    }
}

// Per kept draw, the IRF1 records (BlockHybrid.m:702-737, mcmcVARhybridGibbs.m:713-748, mcmcVARshadowrate.m:
// 649-684), one workgroup per chain: the yields of the plus, minus and baseline paths floored at the ELB, irfdraws =
// floored plus (minus) - floored baseline, its mean over the Nd draws (summed in draw order) into recP / recM at
// index m, the sum over the draws of the floored plus (minus) paths into sumP / sumM; the rows of cumcode run as
// cumulative sums over the horizons (cumsum(., 2)) in all four.  Three passes: the sums over the draws of every
// entry (h, i) (into the record and tmp, [B][2][H][N]); the running sums of the cumulated rows, one thread per
// (row, array) with eight horizons' loads in flight; the division and the update of the running sums.  Optionally
// the raw paths into the store.
__global__ void k_fcst_irf_accum(int N, int H, int Nd, int cap, int m, double elb, const uint8_t* __restrict__ yields,
                                 const uint8_t* __restrict__ cum, const double* __restrict__ fY,
                                 const double* __restrict__ fYp, const double* __restrict__ fYm,
                                 double* __restrict__ recP, double* __restrict__ recM, double* __restrict__ sumP,
                                 double* __restrict__ sumM, double* __restrict__ tmp, double* __restrict__ pathsP,
                                 double* __restrict__ pathsM) {
  const int c = blockIdx.x;
  const size_t HN = (size_t)H * N, per = (size_t)Nd * HN;
  const double* y = fY + (size_t)c * per;
  const double* yp = fYp + (size_t)c * per;
  const double* ym = fYm + (size_t)c * per;
  double* arr[4] = {recP + ((size_t)c * cap + m) * HN, recM + ((size_t)c * cap + m) * HN, tmp + (size_t)c * 2 * HN,
                    tmp + (size_t)c * 2 * HN + HN};
  for (size_t q = threadIdx.x; q < HN; q += blockDim.x) {
    const bool fl = yields[q % N] != 0;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int job = 0; job < Nd; ++job) {
      double b = y[(size_t)job * HN + q], up = yp[(size_t)job * HN + q], um = ym[(size_t)job * HN + q];
      if (fl) {
        b = b < elb ? elb : b;
        up = up < elb ? elb : up;
        um = um < elb ? elb : um;
      }
      v[0] += up - b;
      v[1] += um - b;
      v[2] += up;
      v[3] += um;
    }
    for (int k = 0; k < 4; ++k) arr[k][q] = v[k];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 4 * N; t += blockDim.x) {
    const int k = t / N, i = t - k * N;
    if (!cum[i]) continue;
    double* x = arr[k] + i;
    double run = 0.0;
    for (int h0 = 0; h0 < H; h0 += 8) {
      double v[8];
      for (int u = 0; u < 8; ++u) v[u] = h0 + u < H ? x[(size_t)(h0 + u) * N] : 0.0;
      for (int u = 0; u < 8; ++u)
        if (h0 + u < H) {
          run += v[u];
          x[(size_t)(h0 + u) * N] = run;
        }
    }
  }
  __syncthreads();
  for (size_t q = threadIdx.x; q < HN; q += blockDim.x) {
    arr[0][q] /= Nd;
    arr[1][q] /= Nd;
    sumP[(size_t)c * HN + q] += arr[2][q];
    sumM[(size_t)c * HN + q] += arr[3][q];
  }
  if (pathsP)
    for (size_t q = threadIdx.x; q < per; q += blockDim.x) {
      pathsP[((size_t)c * cap + m) * per + q] = yp[q];
      pathsM[((size_t)c * cap + m) * per + q] = ym[q];
    }
}


// ------------------------------------------------------------------ host launchers
// the paths (one single-wave workgroup per (draw, chain); job Nd = the linear model's mean path) then the scores
hipError_t launch_fcst(hipStream_t st, FcstArgs& a, double* sv1, bool reg_opt) {
  const bool reg = fcst_reg_path(a.N, a.p, a.bh) && reg_opt;
  const bool irf = a.fY1p != nullptr;
  a.hc = irf ? fcst_irf_chunk(a.N, a.Kx, a.p, a.H, reg, a.bh) : fcst_chunk(a.N, a.Kx, a.p, a.H, reg);
  a.sv1 = sv1;
  const size_t lp = (irf ? fcst_irf_lds_doubles(a.N, a.Kx, a.p, a.hc, reg, a.bh)
                         : fcst_paths_lds_doubles(a.N, a.Kx, a.p, a.hc, reg)) * sizeof(double);
  const size_t ls = fcst_scores_lds_doubles(a.N) * sizeof(double);
  if (lp > kLdsCu) throw std::runtime_error("forecast state does not fit LDS");
  const dim3 g(a.bh ? a.Nd : a.Nd + 1, a.B);
  const int rn = fcst_variant(a.N, a.p, a.bh, reg_opt);
  hipError_t e;
  if (irf)
    e = rn == kFcstRegN - 1 ? launch_k(k_fcst<kFcstRegN - 1, true>, g, dim3(64), lp, true, st, a)
        : rn == kFcstRegN   ? launch_k(k_fcst<kFcstRegN, true>, g, dim3(64), lp, true, st, a)
                            : launch_k(k_fcst<0, true>, g, dim3(64), lp, true, st, a);
  else
    e = rn == kFcstRegN - 1 ? launch_k(k_fcst<kFcstRegN - 1>, g, dim3(64), lp, true, st, a)
        : rn == kFcstRegN   ? launch_k(k_fcst<kFcstRegN>, g, dim3(64), lp, true, st, a)
                            : launch_k(k_fcst<0>, g, dim3(64), lp, true, st, a);
  if (e != hipSuccess) return e;
  return launch_k(k_fcst_scores, dim3(a.Nd, a.B), dim3(64), ls, true, st, a);
}

hipError_t launch_fcst_jumpoff(hipStream_t st, const FcstArgs& a, int TP, const int* Tslot, const double* ypool,
                               const int* yidx, double* Xj) {
  return launch_k(k_fcst_jumpoff, dim3(a.B), dim3(256), 0, false, st, a.N, a.p, a.K, TP, Tslot, a.slot, ypool, yidx, a.ldXj,
                  Xj, a.Ns, a.ndxS, a.elb);
}

hipError_t launch_fcst_accum(hipStream_t st, const FcstArgs& a, int cap, int m, const double* yhat, double* sum,
                             double* sumc, double* sumhat, double* scStore, double* paths, double* pathsc) {
  return launch_k(k_fcst_accum, dim3(a.B), dim3(256), 0, false, st, a.N, a.H, a.Nd, cap, m, a.fY, a.fYc, yhat, a.scores, sum, sumc,
                  sumhat, scStore, paths, pathsc);
}

hipError_t launch_fcst_irf_accum(hipStream_t st, const FcstArgs& a, int cap, int m, const uint8_t* cumcode,
                                 double* recP, double* recM, double* sumP, double* sumM, double* tmp, double* pathsP,
                                 double* pathsM) {
  return launch_k(k_fcst_irf_accum, dim3(a.B), dim3(256), 0, false, st, a.N, a.H, a.Nd, cap, m, a.elb, a.ndxYields, cumcode,
                  (const double*)a.fY, (const double*)a.fY1p, (const double*)a.fY1m, recP, recM, sumP, sumM, tmp, pathsP,
                  pathsM);
}

}  // namespace ccmm

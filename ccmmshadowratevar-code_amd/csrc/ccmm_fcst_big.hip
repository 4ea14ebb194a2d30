// Predictive density of one kept draw per chain on the large-N path (32 < N <= 128, K <= 1536; the arithmetic of
// ccmm_fcst.hip, mcmcVAR.m:298-381 and mcmcVARshadowrateBlockHybrid.m:550-625): the linear form (bh = 0, with
// recFloor) and the block-hybrid form (bh = 1).  The hybrid form and the IRF form are not served.
//
// k_fcst_big: PAI (1.38 MB per chain at N = 120, p = 12) is streamed from L2 / HBM once per horizon and workgroup,
// and the recursions that share it are the columns of v_mfma_f64_16x16x4_f64 (lane l: A(l & 15, l >> 4),
// B(l >> 4, l & 15), D((l >> 4) + 4 r, l & 15)): rows = 16 equations per wave, contraction = the lag state,
// columns = recursions.  A draw is a column pair as in k_fcst (ring l, ring c): linear model the unfloored and the
// floored recursion, block hybrid the shadow lags and the actual-rate lags max(shadow, ELB), whose sums the
// equations of the actual-rate block take; the linear model's zero-shock mean path is one more column.  The
// contraction walks the ring slots (lag = head - slot) and, inside a lag, blocks of 16 variables, four MFMA steps
// each: step s of lane group g = l >> 4 takes variable 16 jb + 4 s + g, from PAI in its stored layout (column i =
// equation i; nothing at or beyond row 1 + N p is read) and from the column's ring in LDS.  The intercept seeds
// the accumulator.  Rows beyond N, variables beyond N and columns beyond the chain's last enter as zeros.
// The shock side (sqrtPHI * dev, the log-volatility random walk, nu = invA (sv .* z)) is formed ahead of the
// recursion for a chunk of hc horizons by all threads, sqrtPHI and invA read from global memory.
//
// k_fcst_scores_big: the four one-step log scores of a draw, one workgroup of 256 threads per (draw, chain) over
// one 128 x kNL LDS matrix: the triangular factor invA diag(sv1) itself for the full vector, Gram + wg_chol
// (ccmm_bign_dev.h) for the macro block, the yields and the censored orderings; the censored part on the trailing
// block of at most kMvnMaxD series by wave 0 with the rules of ccmm_fcst_dev.h.
#include <stdexcept>

#include "ccmm_bign_dev.h"
#include "ccmm_fcst_big.h"
#include "ccmm_fcst_dev.h"

namespace ccmm {

__global__ __launch_bounds__(512) void k_fcst_big(FcstArgs a, int cols) {
  extern __shared__ double sm[];
  const int c = blockIdx.y;
  const int N = a.N, K = a.K, p = a.p, H = a.H, Nd = a.Nd, hc = a.hc;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, rt = tid >> 6;
  const int c0 = blockIdx.x * cols;                        // first column of the workgroup (even)
  const int ncl = min(cols, fcst_big_columns(Nd, a.bh) - c0);  // its columns
  const int jd0 = c0 >> 1;                                 // first draw
  const int ndl = max(0, min(cols >> 1, Nd - jd0));        // its draws (the mean path's column has none)
  const int RS = fcst_big_ring_stride(N, p);
  const size_t hcN = (size_t)hc * N;
  double* ring = sm;                            // cols x RS: slot (head - l) mod p of a column holds lag l + 1
  double* Ab = ring + (size_t)cols * RS;        // (cols / 2) x hc x N: the SV normals, then w = sv .* z
  double* Bb = Ab + (size_t)(cols >> 1) * hcN;  // (cols / 2) x hc x N: sqrtPHI dev, then nu = invA w
  double* Ls = Bb + (size_t)(cols >> 1) * hcN;  // (cols / 2) x N: log volatilities of the last horizon
  const int sl = a.slot ? a.slot[c] : 0;
  const double* PAIc = a.PAI + (size_t)c * a.ldPAI * N;
  const double* Xj = a.Xj + (size_t)c * a.ldXj;
  const double* invA = a.invA + (size_t)c * N * N;
  const double* sqrtPHI = a.sqrtPHI + (size_t)c * N * N;
  const int tsv = a.svT ? a.svT[sl] - 1 : 0;
  const double* svz = a.svz ? a.svz + (size_t)c * a.crnStride : nullptr;
  const double* zc = a.z ? a.z + (size_t)c * a.crnStride : nullptr;
  Rng rng;
  rng.crn = nullptr;
  rng.seed = a.seed;
  rng.chain = a.ids ? a.ids[c] : (uint32_t)c;
  rng.sweep = a.sweep;
  const int nsv = N * H * Nd;
  // the jump-off: ring l the K states, ring c (odd columns) the same with, block hybrid, the yields' actual-rate
  // lags (Xjumpoff(K+1:end)); columns beyond the chain's last are zero
  for (int e = tid; e < cols * p * N; e += NT) {
    const int col = e / (p * N), q = e - col * (p * N);
    const int l = q / N, j = q - l * N;
    const int slot = (l == 0) ? 0 : p - l;
    double v = 0.0;
    if (col < ncl) v = ((col & 1) && a.bh == 1 && a.ndxYields[j]) ? Xj[K + q] : Xj[1 + q];
    ring[(size_t)col * RS + slot * N + j] = v;
  }
  for (int e = tid; e < ndl * N; e += NT) {
    const int i = e % N;
    Ls[e] = a.logSV[((size_t)c * N + i) * a.ldSV + tsv];
  }
  // this lane's MFMA operands: A row = equation ai, B column = bcol; D rows di[r], column bcol
  const int g = lane >> 4, bcol = lane & 15;
  const int ai = rt * 16 + bcol;
  const bool aok = ai < N;
  const double* pa = PAIc + (size_t)(aok ? ai : 0) * a.ldPAI + 1;
  // with cols = 8 the MFMA's columns 8..15 have no ring: they enter as zeros and nothing is read for them
  const bool bok = bcol < cols;
  const double* rb = ring + (size_t)(bok ? bcol : 0) * RS;
  const int njb = (N + 15) / 16;
  const int gcol = c0 + bcol;
  const bool cok = bcol < ncl;
  const bool odd = bcol & 1;
  const bool mean_path = !a.bh && gcol == 2 * Nd;
  const int dl = bcol >> 1, job = jd0 + dl;
  double seed[4];
  bool rok[4], isact[4], isyield[4], isrec[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = rt * 16 + g + 4 * r;
    rok[r] = i < N && cok;
    seed[r] = i < N ? Xj[0] * PAIc[(size_t)i * a.ldPAI] : 0.0;  // constant state stays 1 (fcstA(1,1) = 1)
    isact[r] = i < N && a.bh == 1 && a.actual[i];
    isyield[r] = i < N && a.ndxYields[i];
    isrec[r] = i < N && (a.recFloor ? a.recFloor[i] : a.ndxYields[i]);
  }
  int head = 0;
  __syncthreads();
  for (int h0 = 0; h0 < H; h0 += hc) {
    const int nh = min(hc, H - h0);
    const int nq = ndl * nh * N;
    // SV normals randn(N, H*Nd) column hh + job H (mcmcVAR.m:302) of the chunk's horizons
    for (int q = tid; q < nq; q += NT) {
      const int d = q / (nh * N), r2 = q - d * (nh * N), hq = r2 / N, i = r2 - hq * N;
      const int col = h0 + hq + (jd0 + d) * H;
      Ab[d * hcN + hq * N + i] = svz ? svz[(size_t)col * N + i] : rng.normal(CCMM_RNG_FCST, (uint32_t)(col * N + i));
    }
    __syncthreads();
    for (int q = tid; q < nq; q += NT) {  // sqrtPHI * dev, j in order
      const int d = q / (nh * N), r2 = q - d * (nh * N), hq = r2 / N, i = r2 - hq * N;
      const double* dv = Ab + d * hcN + hq * N;
      double shock = 0.0;
      for (int j = 0; j < N; ++j) shock = fma(sqrtPHI[i + (size_t)j * N], dv[j], shock);
      Bb[d * hcN + hq * N + i] = shock;
    }
    __syncthreads();
    // the log-volatility random walk and w = sv .* z with the shock normals randn(N, H, Nd) (:306)
    for (int e = tid; e < ndl * N; e += NT) {
      const int d = e / N, i = e - d * N, jb = jd0 + d;
      double logsv = Ls[e];
      for (int hq = 0; hq < nh; ++hq) {
        const int hh = h0 + hq;
        logsv += Bb[d * hcN + hq * N + i];
        const double sv = exp(logsv * 0.5);
        const size_t zi = ((size_t)jb * H + hh) * N + i;
        const double zv = zc ? zc[zi] : rng.normal(CCMM_RNG_FCST, (uint32_t)(nsv + zi));
        Ab[d * hcN + hq * N + i] = zv * sv;
        if (hh == 0) a.sv1[((size_t)c * Nd + jb) * N + i] = sv;
      }
      Ls[e] = logsv;
    }
    __syncthreads();
    for (int q = tid; q < nq; q += NT) {  // nu = invA w (invA unit lower, j = 0..i)
      const int d = q / (nh * N), r2 = q - d * (nh * N), hq = r2 / N, i = r2 - hq * N;
      const double* wv = Ab + d * hcN + hq * N;
      double nu = 0.0;
      for (int j = 0; j <= i; ++j) nu = fma(invA[i + (size_t)j * N], wv[j], nu);
      Bb[d * hcN + hq * N + i] = nu;
    }
    __syncthreads();
    for (int hq = 0; hq < nh; ++hq) {
      const int hh = h0 + hq;
      // fcstA * state of the workgroup's columns
      dbl4 acc = dbl4{seed[0], seed[1], seed[2], seed[3]};
      for (int slot = 0; slot < p; ++slot) {
        int l = head - slot;
        l += (l < 0) ? p : 0;
        const double* pl = pa + (size_t)l * N;
        const double* rl = rb + slot * N;
        for (int jb = 0; jb < njb; ++jb) {
          double av[4], bv[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int j = jb * 16 + 4 * s + g;
            av[s] = (aok && j < N) ? pl[j] : 0.0;
            bv[s] = (bok && j < N) ? rl[j] : 0.0;
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
        }
      }
      double keep[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = rt * 16 + g + 4 * r;
        const double own = acc[r], oth = __shfl_xor(own, 1, 64);  // the pair's other ring
        const double sumL = odd ? oth : own, sumC = odd ? own : oth;
        keep[r] = 0.0;
        if (rok[r]) {
          const double nu = mean_path ? 0.0 : Bb[dl * hcN + hq * N + i];
          double yl, yc;
          if (a.bh) {
            yl = (isact[r] ? sumC : sumL) + nu;               // fcstA * fcstX0 + fcstB * shocks (:615)
            yc = (isyield[r] && yl < a.elb) ? a.elb : yl;     // actual rate max(shadow, ELB) (:623)
          } else {
            yl = sumL + nu;
            yc = sumC + nu;
            if (isrec[r] && yc < a.elb) yc = a.elb;           // censored simulation (mcmcVAR.m:360-366)
          }
          if (mean_path) {
            a.yhat[((size_t)c * H + hh) * N + i] = yl;
            keep[r] = yl;
          } else {
            const size_t o = (((size_t)c * Nd + job) * H + hh) * N + i;
            if (odd) a.fYc[o] = yc; else a.fY[o] = yl;
            keep[r] = odd ? yc : yl;
          }
        }
      }
      __syncthreads();  // every wave has read the oldest lag block before it is overwritten
      head = (head + 1 == p) ? 0 : head + 1;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rok[r]) ring[(size_t)bcol * RS + head * N + rt * 16 + g + 4 * r] = keep[r];
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- scores
// M = chol(S(rows) S(rows)') for the index list rows[0..n) of S = invA diag(sv) (invA of the chain in global
// memory, lower triangular), in LDS row-major with row stride kNL: the Gram entries spread over the threads (k in
// order per entry), then wg_chol.  Called by the whole workgroup; false on a non-positive pivot.
__device__ bool wg_gram_rows_chol(const double* __restrict__ invA, const double* sv, const int* rows, int n, int N,
                                  double* M, int* bad) {
  __syncthreads();
  if (threadIdx.x == 0) *bad = 0;
  for (int e = threadIdx.x; e < n * n; e += kFcstBigScoreThreads) {
    const int aa = e / n, bb = e - aa * n;
    if (bb > aa) continue;
    const int ra = rows[aa], rb = rows[bb];
    const int kmax = ra < rb ? ra : rb;
    double s = 0.0;
    for (int k = 0; k <= kmax; ++k) s += invA[ra + (size_t)k * N] * invA[rb + (size_t)k * N] * sv[k] * sv[k];
    M[aa * kNL + bb] = s;
  }
  __syncthreads();
  wg_chol<kFcstBigScoreThreads>(M, n, bad);
  return *bad == 0;
}

// logscoreGaussian.m:15-20 with the lower-triangular L (LDS, row stride kNL) and dev = y - mu (LDS, overwritten by
// L^{-1} dev); have_ld: logdet is given, else 2 sum log diag(L).  Called by wave 0; every lane returns the score.
__device__ double wave_score_gauss(const double* L, int n, double* dev, bool have_ld, double logdet) {
  const int lane = threadIdx.x & 63;
  wave_lds_sync();
  wave_trsv_lower(L, kNL, dev, n);
  wave_lds_sync();
  double ss = 0.0, ld = 0.0;
  for (int i = lane; i < n; i += 64) {
    ss += dev[i] * dev[i];
    if (!have_ld) ld += log(L[i * kNL + i]);
  }
  ss = wave_sum(ss);
  if (!have_ld) logdet = 2.0 * wave_sum(ld);
  return -0.5 * (n * 1.8378770664093454836 + logdet + ss);
}

// logscoreGaussianCensored.m:13-88 as score_censored of ccmm_fcst.hip: sel[0..n) = the series scored, cens[i]
// whether series sel[i] may be censored.  Called by the whole workgroup; the result is in *out after the call.
__device__ void wg_score_censored(const double* __restrict__ invA, const double* sv, const double* mu, const double* y,
                                  const int* sel, const uint8_t* cens, int n, int N, double elb, double* M, double* Ms,
                                  double* dev, int* order, int* flags, const GLNodes& gl, double* out) {
  const int tid = threadIdx.x, lane = tid & 63;
  __syncthreads();
  int noff = 0, nat = 0;
  for (int i = 0; i < n; ++i) noff += !(cens[i] && y[sel[i]] <= elb);
  nat = n - noff;
  if (tid == 0) {
    int a = 0, b = noff;
    for (int i = 0; i < n; ++i) {
      if (cens[i] && y[sel[i]] <= elb) order[b++] = sel[i];
      else order[a++] = sel[i];
    }
  }
  if (nat > kMvnMaxD) {
    if (tid == 0) {
      flags[1] = 1;
      *out = NAN;
    }
    __syncthreads();
    return;
  }
  const bool spd = wg_gram_rows_chol(invA, sv, order, n, N, M, flags);  // (its first barrier publishes order)
  if (tid < 64) {
    double res = NAN;
    if (spd) {
      double llf1 = 0.0;
      double y21[kMvnMaxD], yat[kMvnMaxD];
      for (int a = 0; a < kMvnMaxD; ++a) {
        y21[a] = a < nat ? mu[order[noff + a]] : 0.0;
        yat[a] = a < nat ? y[order[noff + a]] : 0.0;
      }
      if (noff > 1) {
        for (int i = lane; i < noff; i += 64) dev[i] = y[order[i]] - mu[order[i]];
        llf1 = wave_score_gauss(M, noff, dev, false, 0.0);  // dev now z1
        for (int a = 0; a < kMvnMaxD; ++a) {
          if (a < nat) {
            double s = 0.0;
            for (int k = lane; k < noff; k += 64) s += M[(noff + a) * kNL + k] * dev[k];
            y21[a] += wave_sum(s);
          }
        }
      }
      for (int e = lane; e < nat * nat; e += 64) {  // the trailing block, column-major with ld kFcstMaxN
        const int aa = e / nat, bb = e - aa * nat;
        Ms[aa + bb * kFcstMaxN] = M[(noff + aa) * kNL + noff + bb];
      }
      wave_lds_sync();
      res = llf1 + censored_llf2(nat, yat, y21, Ms, gl, lane);
    }
    if (lane == 0) *out = res;
  }
  __syncthreads();
}

// One-step predictive log scores of draw `job` of chain c (mcmcVAR.m:326-352; block hybrid :577-608), as
// k_fcst_scores.  Reads the draw's SV at horizon 1 (a.sv1, k_fcst_big).
__global__ __launch_bounds__(kFcstBigScoreThreads) void k_fcst_scores_big(FcstArgs a) {
  extern __shared__ double sm[];
  const int job = blockIdx.x, c = blockIdx.y;
  const int N = a.N, K = a.K, Nd = a.Nd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* M = sm;                            // 128 x kNL, row-major
  double* mu = M + kBignMaxN * kNL;          // muY
  double* y = mu + 128;                      // yrealized(:,1)
  double* sv1 = y + 128;                     // SV at horizon 1
  double* dev = sv1 + 128;
  double* Ms = dev + 128;                    // kMvnMaxD columns of kFcstMaxN: the censored block for the mvncdf rules
  double* res = Ms + kMvnMaxD * kFcstMaxN;   // 8: the four scores
  int* order = (int*)(res + 8);              // 128
  int* sel = order + 128;                    // 128
  int* flags = sel + 128;                    // 8: [0] non-positive pivot, [1] more than kMvnMaxD series at the ELB
  uint8_t* cens = (uint8_t*)(flags + 8);     // 128
  uint8_t* yl8 = cens + 128;                 // 128: ndxYields
  const int sl = a.slot ? a.slot[c] : 0;
  const double* invA = a.invA + (size_t)c * N * N;
  const double* Xj = a.Xj + (size_t)c * a.ldXj;
  const double* PAIc = a.PAI + (size_t)c * a.ldPAI * N;
  if (tid < N) {
    y[tid] = a.yreal[(size_t)sl * a.ldY + tid];
    sv1[tid] = a.sv1[((size_t)c * Nd + job) * N + tid];
    yl8[tid] = a.ndxYields[tid];
  }
  if (tid < 8) flags[tid] = 0;
  __syncthreads();
  // muY = fcstA(ndxfcstY, :) * Xjumpoff (mcmcVAR.m:326-328; block hybrid :577-580: the actual-rate equations read
  // the yields' actual-rate lags): a wave per equation, the K products spread over its lanes
  for (int i = wave; i < N; i += kFcstBigScoreThreads / 64) {
    const bool act = a.bh == 1 && a.actual[i];
    const double* col = PAIc + (size_t)i * a.ldPAI;
    double s = 0.0;
    for (int k = lane; k < K; k += 64) {
      const double xv = (act && k > 0 && yl8[(k - 1) % N]) ? Xj[K + k - 1] : Xj[k];
      s += col[k] * xv;
    }
    s = wave_sum(s);
    if (lane == 0) mu[i] = s;
  }
  __syncthreads();
  int nx = 0, ni = 0, natelb = 0;
  for (int i = 0; i < N; ++i) {
    if (yl8[i]) {
      ++ni;
      natelb += (y[i] <= a.elb);
    } else {
      ++nx;
    }
  }
  // (1) full vector: sqrtOmegaY = invA diag(sv1) is lower triangular, logdet = sum logSV(:,1)
  for (int e = tid; e < N * N; e += kFcstBigScoreThreads) {
    const int k = e / N, i = e - k * N;  // (i fastest: invA is column-major)
    if (i > k) M[i * kNL + k] = invA[e] * sv1[k];
    else if (i == k) M[i * kNL + i] = sv1[i];  // unit-diagonal invA times sv
  }
  if (tid < N) dev[tid] = y[tid] - mu[tid];
  __syncthreads();
  if (wave == 0) {
    double ld = 0.0;
    for (int i = lane; i < N; i += 64) ld += 2.0 * log(sv1[i]);
    ld = wave_sum(ld);
    const double s = wave_score_gauss(M, N, dev, true, ld);
    if (lane == 0) res[0] = s;
  }
  __syncthreads();
  // (2) censored full vector (ndxYIELDS censorable); the block-hybrid fcstLogscoreDraws
  if (natelb > 0) {
    if (tid < N) {
      sel[tid] = tid;
      cens[tid] = yl8[tid];
    }
    wg_score_censored(invA, sv1, mu, y, sel, cens, N, N, a.elb, M, Ms, dev, order, flags, a.gl, res + 1);
  } else if (tid == 0) {
    res[1] = res[0];
  }
  // (3) macro block
  __syncthreads();
  if (tid == 0) {
    int q = 0;
    for (int i = 0; i < N; ++i)
      if (!yl8[i]) sel[q++] = i;
  }
  if (wg_gram_rows_chol(invA, sv1, sel, nx, N, M, flags)) {
    if (wave == 0) {
      for (int i = lane; i < nx; i += 64) dev[i] = y[sel[i]] - mu[sel[i]];
      const double s = wave_score_gauss(M, nx, dev, false, 0.0);
      if (lane == 0) res[2] = s;
    }
  } else if (tid == 0) {
    res[2] = NAN;
  }
  // (4) yields block: every yield censorable
  __syncthreads();
  if (tid == 0) {
    int q = 0;
    for (int i = 0; i < N; ++i)
      if (yl8[i]) {
        sel[q] = i;
        cens[q] = 1;
        ++q;
      }
  }
  if (natelb > 0) {
    wg_score_censored(invA, sv1, mu, y, sel, cens, ni, N, a.elb, M, Ms, dev, order, flags, a.gl, res + 3);
  } else if (wg_gram_rows_chol(invA, sv1, sel, ni, N, M, flags)) {
    if (wave == 0) {
      for (int i = lane; i < ni; i += 64) dev[i] = y[sel[i]] - mu[sel[i]];
      const double s = wave_score_gauss(M, ni, dev, false, 0.0);
      if (lane == 0) res[3] = s;
    }
  } else if (tid == 0) {
    res[3] = NAN;
  }
  __syncthreads();
  if (tid == 0) {
    for (int q = 0; q < 4; ++q) a.scores[((size_t)c * Nd + job) * 4 + q] = res[q];
    if (flags[1]) atomicOr(&a.status[c], 2);
  }
}

// ------------------------------------------------------------------ host launcher
hipError_t launch_fcst_big(hipStream_t st, FcstArgs& a, double* sv1) {
  if (a.bh == 2 || a.fY1p) throw std::runtime_error("the large-N predictive density serves the linear and block-hybrid forms");
  const FcstBigPlan pl = fcst_big_plan(a.N, a.p, a.H, a.Nd, a.bh);
  if (!pl.ok) throw std::runtime_error("forecast state does not fit LDS");
  a.hc = pl.hc;
  a.sv1 = sv1;
  const hipError_t e = launch_k(k_fcst_big, dim3(pl.tiles, a.B), dim3(64 * pl.waves), pl.lds, true, st, a, pl.cols);
  if (e != hipSuccess) return e;
  return launch_k(k_fcst_scores_big, dim3(a.Nd, a.B), dim3(kFcstBigScoreThreads), pl.lds_scores, true, st, a);
}

}  // namespace ccmm

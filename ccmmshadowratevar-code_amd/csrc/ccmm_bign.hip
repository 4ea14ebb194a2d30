// Gibbs blocks for large N (33 <= N <= 128; the S120 configuration N = 120):
//
//   k_astep_big  (chain, row ii): the weighted Gram of RESID(:, 0:ii) with weights
//                1 / sqrtht(:, ii)^2 (ZZ and Zz of mcmcVAR.m:240-244), Cholesky, the two
//                triangular solves and the draw of A(ii, 0:ii-1) (:245-252)
//   k_astep_fin  (chain): invA = A \ I (:254), logy2 = log((RESID A')^2 + offset) (:259)
//   k_phi_big    (chain): the inverse-Wishart draw of mcmcVAR.m:268-274
//   k_sv_big     (chain): KSC-mixture SV draw of h_0..h_T with the time-ordered block
//                Cholesky factor of the block-tridiagonal posterior precision
//                (oracle.sv_draw_sequential; the declared convention for N > 32, the
//                reference's sampler lives in the absent em-matlabbox):
//                  M_t = L_{t-1}^{-1} Q,  L_t = chol(D_t - M_t' M_t),
//                  w_t = L_t^{-1} (b_t + M_t' w_{t-1}),
//                  x_T = L_T^{-T}(w_T + z_T),  x_t = L_t^{-T}(w_t + z_t + M_{t+1} x_{t+1})
//
// The N x N matrices (115 KB at N = 120) no longer fit a CU's LDS several at a time, so
// one of them lives in LDS (row-major, ld = 129 doubles) and the rest in per-chain global
// scratch (L2 resident).  Workgroup primitives below: an LDS-staged Gram with 4 x 4
// register tiles, a blocked Cholesky (16-wide panels, kPB: one wave factors the diagonal
// block with readlane broadcasts, all threads update), blocked triangular solves.
// ccmm_bign.h holds kNL, kCB and every dynamic-LDS size with the kernel's layout beside it.
#include "ccmm_bign_dev.h"  // kPB, wg_chol, wave_trsv_lower (and ccmm_bign.h)

#include <cstdlib>

namespace ccmm {

constexpr int kGC = 32;    // Gram t-chunk

// ---------------------------------------------------------------- Gram
// G(a, b) = sum_{t < T} w(t) x_t(a) x_t(b) for the lower triangle a >= b of m x m (m <= 128),
// x_t(a) = src[a * sa + t * st]; w = nullptr: unit weights, else w[t * sw].  G: LDS (ld kNL),
// ALIASED with the staging area (written after the last chunk).  Returns after a barrier.
template <int NT>
__device__ void wg_gram(double* G, const double* __restrict__ src, int sa, int st, int m, int T,
                        const double* __restrict__ w, int sw) {
  constexpr int NTL = (32 * 33 / 2 + NT - 1) / NT;  // 4 x 4 tiles per thread (m <= 128)
  double* stage = G;                                // [kGC][kNL] + weights [kGC]
  double* wst = G + kGC * kNL;
  const int tid = threadIdx.x;
  const int mt = (m + 3) / 4;
  const int ntile = mt * (mt + 1) / 2;
  int ta[NTL], tb[NTL];
#pragma unroll
  for (int q = 0; q < NTL; ++q) {
    int tile = tid + NT * q, ti = 0;
    if (tile < ntile) {
      while (tile > ti) {
        tile -= ti + 1;
        ++ti;
      }
      ta[q] = ti * 4;
      tb[q] = tile * 4;
    } else {
      ta[q] = -1;
      tb[q] = 0;
    }
  }
  double acc[NTL][16];
#pragma unroll
  for (int q = 0; q < NTL; ++q)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[q][e] = 0.0;
  for (int t0 = 0; t0 < T; t0 += kGC) {
    const int nt = min(kGC, T - t0);
    if (st == 1) {  // t contiguous for fixed a
      for (int e = tid; e < m * kGC; e += NT) {
        const int a = e / kGC, tt = e - a * kGC;
        stage[tt * kNL + a] = (tt < nt) ? src[(size_t)a * sa + t0 + tt] : 0.0;
      }
    } else {        // a contiguous for fixed t
      for (int e = tid; e < m * kGC; e += NT) {
        const int tt = e / m, a = e - tt * m;
        stage[tt * kNL + a] = (tt < nt) ? src[(size_t)a * sa + (size_t)(t0 + tt) * st] : 0.0;
      }
    }
    for (int tt = tid; tt < kGC; tt += NT) wst[tt] = (tt < nt) ? (w ? w[(size_t)(t0 + tt) * sw] : 1.0) : 0.0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NTL; ++q) {
      if (ta[q] < 0) continue;
      for (int tt = 0; tt < kGC; ++tt) {
        const double* row = stage + tt * kNL;
        const double wv = wst[tt];
        double xa[4], xb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xa[i] = row[min(ta[q] + i, 127)] * wv;
          xb[i] = row[min(tb[q] + i, 127)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[q][i * 4 + jj] = fma(xa[i], xb[jj], acc[q][i * 4 + jj]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NTL; ++q) {
    if (ta[q] < 0) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int a = ta[q] + i, b = tb[q] + jj;
        if (a < m && b <= a) G[a * kNL + b] = acc[q][i * 4 + jj];
      }
  }
  __syncthreads();
}

// (the blocked Cholesky wg_chol and the forward solve wave_trsv_lower: ccmm_bign_dev.h)
// v <- L^{-T} v, as wave_trsv_lower.  Called by wave 0 only.
__device__ void wave_trsv_lower_t(const double* L, int ld, double* v, int n) {
  const int lane = threadIdx.x & 63;
  double r0 = lane < n ? v[lane] : 0.0, r1 = lane + 64 < n ? v[lane + 64] : 0.0;
  for (int k = n - 1; k >= 0; --k) {
    const double vk = (k < 64 ? readlane_d(r0, k) : readlane_d(r1, k - 64)) / L[(size_t)k * ld + k];
    if (k < 64 && lane == k) r0 = vk;
    if (k >= 64 && lane == k - 64) r1 = vk;
    if (lane < k) r0 = fma(-L[(size_t)k * ld + lane], vk, r0);
    if (lane + 64 < k) r1 = fma(-L[(size_t)k * ld + lane + 64], vk, r1);
  }
  if (lane < n) v[lane] = r0;
  if (lane + 64 < n) v[lane + 64] = r1;
}

// ================================================================ A-step
// One workgroup per (row ii = 1..N-1, chain).  Regressors RESID(:, 0:ii-1) / sqrtht(:, ii),
// regressand RESID(:, ii) / sqrtht(:, ii): the (ii+1) x (ii+1) weighted Gram of RESID(:, 0:ii)
// with weights 1 / sqrtht(:, ii)^2 holds ZZ (leading block) and Zz (last row).
// The weighted Grams of the A-step on FP64 MFMA: for every chain and row ii = 1..N-1,
// G_ii = RESID' diag(1 / sqrtht(:, ii)^2) RESID over the lower 64 x 64 tiles of NPAD x NPAD
// (mcmcVAR.m:240-244: ZZ = the leading ii x ii block, Zz = row ii).  One workgroup = one tile of
// FOUR rows ii sharing the chain's residuals: the RESID panels are staged once in LDS and each wave
// applies its own row's weights (the structure of k_gram_big).  Tiles wholly beyond the group's
// largest ii are skipped.  Per entry the sum over t is one fma chain in t order, (x_a w) x_b: the
// order of the scalar wg_gram it replaces.
constexpr int kAC = 32;    // t rows per staged chunk
constexpr int kALd = 80;   // LDS row stride of the staged panels
__global__ __launch_bounds__(256) void k_astep_gram(Dims d, const int* __restrict__ Tslot, ChainState cs,
                                                   double* __restrict__ gbuf, int NPAD) {
  __shared__ double Pa[kAC][kALd];
  __shared__ double Pb[kAC][kALd];
  __shared__ double Wl[4][kAC];
  const int N = d.N, TP = d.TP;
  const int ngr = (N - 1 + 3) / 4;
  const int c = blockIdx.y / ngr, gr = blockIdx.y - c * ngr;
  const int ii0 = 1 + 4 * gr;
  int tile = blockIdx.x, ti = 0;
  while (tile > ti) {
    tile -= ti + 1;
    ++ti;
  }
  const int tj = tile;
  const int a0 = ti * 64, b0 = tj * 64;
  if (a0 > min(ii0 + 3, N - 1)) return;  // no row of this tile is needed by the group's systems
  const int T = Tslot[cs.slot[c]];
  const double* E = cs.E + (size_t)c * N * TP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int myii = ii0 + wave;
  const int lcol = tid & 63, lt0 = (tid >> 6) * 8;
  dbl4 acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = dbl4{0.0, 0.0, 0.0, 0.0};
  const int nchunks = (T + kAC - 1) / kAC;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int t0 = ch * kAC;
    {
      const int ca = a0 + lcol, cb = b0 + lcol;
      const double* xa = E + (size_t)min(ca, N - 1) * TP;
      const double* xb = E + (size_t)min(cb, N - 1) * TP;
      double va[8], vb[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t = t0 + lt0 + q;
        va[q] = (ca < N && t < T) ? xa[t] : 0.0;
        vb[q] = (cb < N && t < T) ? xb[t] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        Pa[lt0 + q][lcol] = va[q];
        Pb[lt0 + q][lcol] = vb[q];
      }
      if (tid < 4 * kAC) {
        const int e = tid >> 5, t = tid & 31;
        const int ii = ii0 + e;
        double wv = 0.0;
        if (ii < N && t0 + t < T) {
          const double h = cs.sqrtht[((size_t)c * N + ii) * TP + t0 + t];
          wv = 1.0 / (h * h);
        }
        Wl[e][t] = wv;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kAC / 4; ++kk) {
      const int kr = kk * 4 + (lane >> 4);
      const double wv = Wl[wave][kr];
      double fa[4], fb[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        fb[x] = Pb[kr][x * 16 + (lane & 15)];       // MFMA A operand: rows = b
        fa[x] = Pa[kr][x * 16 + (lane & 15)] * wv;  // MFMA B operand: cols = a (weighted)
      }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
          acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[x], fa[y], acc[x][y], 0, 0, 0);
    }
    __syncthreads();
  }
  if (myii >= N) return;
  // D[row = b][col = a]: lane holds rows (lane >> 4) + 4 r of block x, column lane & 15 of block y
  double* G = gbuf + ((size_t)c * (N - 1) + (myii - 1)) * NPAD * NPAD;
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + x * 16 + (lane >> 4) + 4 * r;
        const int a = a0 + y * 16 + (lane & 15);
        G[(size_t)b * NPAD + a] = acc[x][y][r];
      }
}

__global__ __launch_bounds__(256) void k_astep_big(Dims d, const int* __restrict__ Tslot,
                                                   ChainState cs, RngArgs ra, const double* __restrict__ gbuf,
                                                   int NPAD) {
  extern __shared__ double sm[];
  const int ii = blockIdx.x + 1, c = blockIdx.y;
  const int N = d.N, TP = d.TP;
  const int T = Tslot[cs.slot[c]];
  const int tid = threadIdx.x;
  const Rng rng = ra.make(c);
  double* G = sm;                    // (ii+1) x (ii+1), ld kNL
  double* vec = sm + 128 * kNL;      // ii
  // the weighted Gram of RESID(:, 0:ii) (k_astep_gram), lower triangle into LDS
  {
    const double* Gs = gbuf + ((size_t)c * (N - 1) + (ii - 1)) * NPAD * NPAD;
    const int m = ii + 1;
    for (int e = tid; e < m * m; e += 256) {
      const int b = e / m, a = e - b * m;
      if (a >= b) G[a * kNL + b] = Gs[(size_t)b * NPAD + a];
    }
    __syncthreads();
  }
  const int n = ii;
  for (int a = tid; a < n; a += 256) vec[a] = G[n * kNL + a];  // Zz
  __syncthreads();
  int bad = 0;
  wg_chol<256>(G, n, &bad);
  if (tid < 64) {
    wave_trsv_lower(G, kNL, vec, n);  // tilde = L \ Zz   (sqrtiVAlpha_post' \ Zz)
    const int zoff = ii * (ii - 1) / 2;
    for (int r = tid; r < n; r += 64) vec[r] += rng.normal(CCMM_RNG_A, (uint32_t)(zoff + r));
    wave_trsv_lower_t(G, kNL, vec, n);  // alpha = L' \ (tilde + z)
  }
  __syncthreads();
  double* Ac = cs.A + (size_t)c * N * N;
  for (int q = tid; q < n; q += 256) Ac[ii + q * N] = -vec[q];
  if (bad && tid == 0) atomicOr(&cs.status[c], 4);
}

// invA = A \ I and logy2 = log((RESID A')^2 + offset); unit diagonal / zero upper of A.
__global__ __launch_bounds__(256) void k_astep_fin(Dims d, const int* __restrict__ Tslot, ChainState cs,
                                                   double logy2offset) {
  extern __shared__ double sm[];
  const int c = blockIdx.x;
  const int N = d.N, TP = d.TP;
  const int T = Tslot[cs.slot[c]];
  const int tid = threadIdx.x;
  double* Ac = cs.A + (size_t)c * N * N;
  double* As = sm;  // N x N column-major
  for (int q = tid; q < N * N; q += 256) {
    const int r = q % N, col = q / N;
    const double v = (r == col) ? 1.0 : (r > col ? Ac[q] : 0.0);
    As[q] = v;
    Ac[q] = v;
  }
  __syncthreads();
  double* Ai = cs.invA + (size_t)c * N * N;
  for (int col = tid; col < N; col += 256) {  // forward substitution, column col
    for (int r = 0; r < N; ++r) {
      double s = (r == col) ? 1.0 : 0.0;
      if (r > col)
        for (int q = col; q < r; ++q) s = fma(-As[r + q * N], Ai[q + col * N], s);
      Ai[r + col * N] = (r >= col) ? s : 0.0;
    }
  }
  const double* E = cs.E + (size_t)c * N * TP;
  double* ly = cs.logy2 + (size_t)c * N * TP;
  for (int q = tid; q < N * TP; q += 256) {
    const int i = q / TP, t = q - i * TP;
    double s = 0.0;
    if (t < T)
      for (int k = 0; k <= i; ++k) s = fma(E[(size_t)k * TP + t], As[i + k * N], s);
    ly[q] = (t < T) ? log(s * s + logy2offset) : 0.0;
  }
}

// ================================================================ PHI (inverse Wishart)
// mcmcVAR.m:268-274 with scr = 3 N x N per chain (row-major, ld N): Lpost, L2 = chol(Z Z')'
// (R = L2'), Sq.  1024 threads per chain.
__global__ __launch_bounds__(1024) void k_phi_big(Dims d, const int* __restrict__ Tslot, int dPHI,
                                                  const double* __restrict__ sPHIall, ChainState cs,
                                                  double* __restrict__ scr) {
  extern __shared__ double sm[];
  const int c = blockIdx.x;
  const int s = cs.slot[c];
  const int N = d.N, TP = d.TP;
  const int T = Tslot[s];
  const int TZ = T + dPHI, TZmax = TP + dPHI;
  const int tid = threadIdx.x;
  double* M = sm;  // N x N, ld kNL
  double* Lp = scr + (size_t)c * 3 * N * N;
  double* L2 = Lp + N * N;
  double* Sq = L2 + N * N;
  const double* sP = sPHIall + (size_t)s * N * N;
  int bad = 0;
  // Lpost = chol(s_PHI + eta'eta, 'lower')
  wg_gram<1024>(M, cs.eta + (size_t)c * N * TP, TP, 1, N, T, nullptr, 0);
  for (int e = tid; e < N * N; e += 1024) {
    const int r = e / N, col = e - r * N;
    if (col <= r) M[r * kNL + col] += sP[r + col * N];
  }
  __syncthreads();
  wg_chol<1024>(M, N, &bad);
  for (int e = tid; e < N * N; e += 1024) Lp[e] = M[(e / N) * kNL + e % N];
  __syncthreads();
  // R = chol(Zdraw Zdraw') (upper) = L2'
  wg_gram<1024>(M, cs.Zphi + (size_t)c * N * TZmax, 1, N, N, TZ, nullptr, 0);
  wg_chol<1024>(M, N, &bad);
  for (int e = tid; e < N * N; e += 1024) L2[e] = M[(e / N) * kNL + e % N];
  __syncthreads();
  // sqrtPHI_ = Lpost / R: Sq L2' = Lpost, row r by forward substitution (thread per row)
  for (int r = tid; r < N; r += 1024) {
    for (int col = 0; col < N; ++col) {
      double v = (col <= r) ? Lp[r * N + col] : 0.0;
      for (int q = 0; q < col; ++q) v = fma(-Sq[r * N + q], L2[col * N + q], v);
      Sq[r * N + col] = v / L2[col * N + col];
    }
  }
  __syncthreads();
  // PHI_ = Sq Sq'
  double* PHI = cs.PHI + (size_t)c * N * N;
  for (int e = tid; e < N * N; e += 1024) {
    const int r = e / N, col = e - r * N;
    if (col > r) continue;
    double v = 0.0;
    for (int q = 0; q < N; ++q) v = fma(Sq[r * N + q], Sq[col * N + q], v);
    M[r * kNL + col] = v;
    PHI[r + col * N] = v;
    PHI[col + r * N] = v;
  }
  __syncthreads();
  wg_chol<1024>(M, N, &bad);
  double* sqo = cs.sqrtPHI + (size_t)c * N * N;
  for (int e = tid; e < N * N; e += 1024) {
    const int r = e % N, col = e / N;
    sqo[e] = (col <= r) ? M[r * kNL + col] : 0.0;
  }
  if (bad && tid == 0) atomicOr(&cs.status[c], 16);
}

// ================================================================ Cholesky + inverse (LDS)
// S (n x n lower, ld kNL, n <= 128) <- L^{-1} for S = L L': blocked right-looking Cholesky
// with 16-wide panels, the inverse built row block by row block as the panels complete.
//   panel i (rows p0 .. p0+15):
//     wave 0: factor the diagonal block, invert it (Dv_i) and store Dv_i over it
//     all:    L(r, panel) = S(r, panel) Dv_i' for the blocks below;
//             T = L(block i, 0:p0) Linv(0:p0, 0:p0)                   (Tb)
//     all:    trailing update;  Linv(block i, 0:p0) = -Dv_i T
// The block products run on MFMA, one 16 x 16 block per wave.  Only the lower triangle is read
// (the upper triangle of S may hold anything; diagonal blocks are masked).  Tb: LDS scratch,
// kCB x 128 doubles (kCB = 16, ccmm_bign.h).

template <int NT>
__device__ void wg_chol_inv(double* S, int n, double* Tb, int* bad) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // wave 0: factor the diagonal block at q0 (qw rows) and store its inverse Dv over it
  auto diag = [&](int q0, int qw) {
      double row[kCB], dv[kCB], ipk[kCB];
#pragma unroll
      for (int m = 0; m < kCB; ++m) row[m] = (lane < qw && m <= lane) ? S[(q0 + lane) * kNL + q0 + m] : 0.0;
#pragma unroll
      for (int kk = 0; kk < kCB; ++kk) {
        ipk[kk] = 1.0;
        if (kk < qw) {
          double dkk = readlane_d(row[kk], kk);
          if (!(dkk > 0.0)) {
            *bad = 1;
            dkk = 1.0;
          }
          // 1 / sqrt(d): hardware estimate + two Newton steps, no IEEE sqrt / division on the
          // serial pivot chain; L_kk = d / sqrt(d), and 1 / L_kk is kept for the inverse below
          double ip = __builtin_amdgcn_rsq(dkk);
          const double hd = 0.5 * dkk;
          ip = ip * fma(-hd * ip, ip, 1.5);
          ip = ip * fma(-hd * ip, ip, 1.5);
          ipk[kk] = ip;
          if (lane == kk) row[kk] = dkk * ip;
          if (lane > kk) row[kk] *= ip;
          const double lik = row[kk];
#pragma unroll
          for (int m = kk + 1; m < kCB; ++m) {
            const double lmk = readlane_d(lik, m);
            if (lane >= m) row[m] = fma(-lik, lmk, row[m]);
          }
        }
      }
      // Dv = L_b^{-1}, lane r holding row r: right-looking over the rows k of L_b
#pragma unroll
      for (int c = 0; c < kCB; ++c) dv[c] = (lane == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < kCB; ++k) {
        if (k < qw) {
          if (lane == k) {
            const double il = ipk[k];
#pragma unroll
            for (int c = 0; c <= k; ++c) dv[c] *= il;
          }
          const double lrk = row[k];
#pragma unroll
          for (int c = 0; c <= k; ++c) {
            const double dkc = readlane_d(dv[c], k);
            if (lane > k) dv[c] = fma(-lrk, dkc, dv[c]);
          }
        }
      }
      if (lane < qw)
#pragma unroll
        for (int m = 0; m < kCB; ++m)
          if (m <= lane) S[(q0 + lane) * kNL + q0 + m] = dv[m];
  };
  if (wave == 0) diag(0, min(kCB, n));
  for (int p0 = 0; p0 < n; p0 += kCB) {
    const int pw = min(kCB, n - p0);
    __syncthreads();
    // 16 x 16 blocks on v_mfma_f64_16x16x4 (A(lr, lq), B(lq, lr), D(lq + 4 r, lr)), one block task
    // per wave round robin; Dv(r, q) = S(p0 + r, p0 + q), q <= r
    const int lr = lane & 15, lq = lane >> 4;
    const int NB = (n + 15) >> 4, pb = p0 >> 4;
    // (a) L(I, pb) = S(I, pb) Dv', I > pb;  (b) T(J) = sum_{K=J}^{pb-1} L(pb, K) Linv(K, J), J < pb
    const int na = NB - 1 - pb;
    for (int task = wave; task < na + pb; task += NT / 64) {
      dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
      if (task < na) {
        const int I = pb + 1 + task, r = 16 * I + lr;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int q = 4 * kk + lq;
          const double x = (r < n && q < pw) ? S[r * kNL + p0 + q] : 0.0;
          const double y = (q <= lr && lr < pw) ? S[(p0 + lr) * kNL + p0 + q] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int row = 16 * I + lq + 4 * r4;
          if (row < n && lr < pw) S[row * kNL + p0 + lr] = acc[r4];
        }
      } else {
        const int J = task - na;
        for (int K = J; K < pb; ++K)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const int q = 4 * kk + lq;
            const double x = (lr < pw) ? S[(p0 + lr) * kNL + 16 * K + q] : 0.0;
            const double y = (K > J || lr <= q) ? S[(16 * K + q) * kNL + 16 * J + lr] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
          }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) Tb[(lq + 4 * r4) * 128 + 16 * J + lr] = acc[r4];
      }
    }
    __syncthreads();
    // (c) S(I, I2) -= L(I, pb) L(I2, pb)', pb < I2 <= I;  (d) Linv(pb, J) = -Dv T(J), J < pb
    const int mb = NB - 1 - pb, nc = mb * (mb + 1) / 2;
    // wave 0 takes task 0 only (when there is a next diagonal block to factor); the rest go
    // round robin over waves 1..7
    const bool la = pb + 1 < NB;
    const int t0 = la ? (wave == 0 ? 0 : wave) : wave, tstep = la ? (wave == 0 ? (1 << 30) : NT / 64 - 1) : NT / 64;
    for (int task = t0; task < nc + pb; task += tstep) {
      dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
      if (task < nc) {
        int x0 = 0, y0 = task;
        while (y0 > x0) {
          y0 -= x0 + 1;
          ++x0;
        }
        const int I = pb + 1 + x0, I2 = pb + 1 + y0;
        const int ra = 16 * I + lr, rb = 16 * I2 + lr;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int q = 4 * kk + lq;
          const double x = (ra < n && q < pw) ? S[ra * kNL + p0 + q] : 0.0;
          const double y = (rb < n && q < pw) ? S[rb * kNL + p0 + q] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int row = 16 * I + lq + 4 * r4;
          if (row < n && rb < n) S[row * kNL + rb] -= acc[r4];
        }
        if (task == 0) {
          // look-ahead: task 0 is the trailing update of the next diagonal block (wave 0's
          // first task), so wave 0 factors and inverts it now, beside the other waves' tasks
          wave_lds_sync();
          diag(p0 + kCB, min(kCB, n - p0 - kCB));
        }
      } else {
        const int J = task - nc;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int q = 4 * kk + lq;
          const double x = (q <= lr && lr < pw) ? S[(p0 + lr) * kNL + p0 + q] : 0.0;
          const double y = (q < pw) ? Tb[q * 128 + 16 * J + lr] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int row = p0 + lq + 4 * r4;
          if (row < n) S[row * kNL + 16 * J + lr] = -acc[r4];
        }
      }
    }
  }
  __syncthreads();
}

// ================================================================ SV (time-ordered sampler)
// Per chain (kSvNT threads).  scratch per chain (row-major, ld N): Q = PHI^{-1}; Lt[t] =
// L_t^{-1}; Mt[t] = M_t = L_{t-1}^{-1} Q; w[t].  Per block t:
//   M_t = Linv_{t-1} Q (MFMA, Linv_{t-1} in LDS, Q in registers) -> LDS over Linv_{t-1}
//   G = M_t' M_t (MFMA from LDS, in registers)
//   S = D_t - G, r = b_t + M_t' w_{t-1}             -> Linv_t = chol(S)^{-1} (wg_chol_inv)
//   w_t = Linv_t r
// backward: x_t = Linv_t' (w_t + z_t + M_{t+1} x_{t+1}).
constexpr int kSvNT = 512;

__global__ __launch_bounds__(kSvNT) void k_sv_big(Dims d, const int* __restrict__ Tslot,
                                                  const double* __restrict__ V0inv,
                                                  const double* __restrict__ V0invm, ChainState cs,
                                                  RngArgs ra, double* __restrict__ scr, size_t scr_stride,
                                                  int skip) {
  extern __shared__ double sm[];
  constexpr int NT = kSvNT;
  const int c = blockIdx.x;
  const int s = cs.slot[c];
  const int N = d.N, TP = d.TP;
  const int T = Tslot[s];
  const int tid = threadIdx.x;
  const Rng rng = ra.make(c);
  const size_t NN = (size_t)N * N;
  double* Q = scr + (size_t)c * scr_stride;
  double* Lt = Q + NN;                        // (T+1) x NN: Linv_t
  double* Mt = Lt + (size_t)(TP + 1) * NN;    // (T+1) x NN
  double* wv = Mt + (size_t)(TP + 1) * NN;    // (T+1) x N
  double* S = sm;                             // N x N, ld kNL
  double* Tb = sm + N * kNL;                  // kCB x 128
  double* vec = Tb + kCB * 128;               // 128
  double* vec2 = vec + 128;                   // 128
  const double* obs = cs.svobs + (size_t)c * N * TP;
  const double* irv = cs.svir + (size_t)c * N * TP;
  int bad = 0;
  const int gj = tid >> 3, gq = tid & 7;  // 8-lane group per row / column gj (64 groups)
  // Q = PHI^{-1} = sqrtPHI^{-T} sqrtPHI^{-1}: invert sqrtPHI (lower) column-wise into Lt[0]
  {
    const double* sq = cs.sqrtPHI + (size_t)c * NN;  // column-major lower
    double* Li = Lt;                                 // scratch: Li(r, col) at r * N + col
    for (int col = tid; col < N; col += NT)
      for (int r = 0; r < N; ++r) {
        double v = (r == col) ? 1.0 : 0.0;
        if (r > col)
          for (int q = col; q < r; ++q) v = fma(-sq[r + q * N], Li[q * N + col], v);
        Li[r * N + col] = (r >= col) ? v / sq[r + r * N] : 0.0;
      }
    __syncthreads();
    for (int e = tid; e < N * N; e += NT) {
      const int a = e / N, b = e - a * N;
      double v = 0.0;
      for (int r = max(a, b); r < N; ++r) v = fma(Li[r * N + a], Li[r * N + b], v);
      Q[e] = v;
    }
    __syncthreads();
  }
  const double* V0 = V0inv + (size_t)s * NN;
  // MFMA operands (v_mfma_f64_16x16x4: A(lr, lq), B(lq, lr), D(lq + 4 r, lr)); N <= 128 is NB <= 8
  // blocks of 16.  Wave J owns column block J of M_t = Linv_{t-1} Q: Q's column block is the same
  // at every step, so it stays in registers for the whole forward pass (qb[4 K + kk] = Q(16 K +
  // 4 kk + lq, 16 J + lr)).
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int NB = (N + 15) >> 4;
  double qb[32];
#pragma unroll
  for (int K = 0; K < 8; ++K)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int r = 16 * K + 4 * kk + lq, col = 16 * wave + lr;
      qb[4 * K + kk] = (r < N && col < N) ? Q[r * N + col] : 0.0;
    }
  // ---- forward: t = 0 .. T.  Entering step t >= 1 the LDS matrix holds Linv_{t-1}.
  for (int t = 0; t <= T; ++t) {
    double* Mcur = Mt + (size_t)t * NN;
    if (t > 0) {
      // M_t = Linv_{t-1} Q: block (I, J) = sum_{K <= I} Linv(I, K) Q(K, J) (Linv lower), each
      // block straight to global Mt[t]; the LDS copy replaces Linv_{t-1} after the barrier
      if (wave < NB && !(skip & 1)) {
        const int col = 16 * wave + lr;
#pragma unroll 1
        for (int I = 0; I < NB; ++I) {
          dbl4 mb = dbl4{0.0, 0.0, 0.0, 0.0};
          const int r = 16 * I + lr;
#pragma unroll
          for (int K = 0; K < 8; ++K)
            if (K <= I) {
#pragma unroll
              for (int kk = 0; kk < 4; ++kk) {
                const int cix = 16 * K + 4 * kk + lq;
                const double a = (r < N && cix <= r) ? S[r * kNL + cix] : 0.0;
                mb = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qb[4 * K + kk], mb, 0, 0, 0);
              }
            }
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int row = 16 * I + lq + 4 * r4;
            if (row < N && col < N) Mcur[row * N + col] = mb[r4];
          }
        }
      }
      __syncthreads();  // every read of Linv_{t-1} (kept in global Lt[t-1]) is done
      for (int e = tid; e < N * N; e += NT) {
        const int a = e / N, b = e - a * N;
        S[a * kNL + b] = Mcur[e];
      }
      __syncthreads();
      // G = M_t' M_t, lower blocks (A, B), B <= A, round robin over the waves; the rhs
      // b_t = obs_t ir_t + M_t' w_{t-1} (8 lanes per entry) from the same LDS copy of M_t
      dbl4 g[5];
      const int npair = NB * (NB + 1) / 2;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        g[j] = dbl4{0.0, 0.0, 0.0, 0.0};
        const int pr = wave + 8 * j;
        if (pr < npair && !(skip & 2)) {
          int A = 0, Bb = pr;
          while (Bb > A) {
            Bb -= A + 1;
            ++A;
          }
          const int ca = 16 * A + lr, cb = 16 * Bb + lr;
          for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              const int k = 16 * I + 4 * kk + lq;
              const double a = (k < N && ca < N) ? S[k * kNL + ca] : 0.0;
              const double b = (k < N && cb < N) ? S[k * kNL + cb] : 0.0;
              g[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, g[j], 0, 0, 0);
            }
        }
      }
      {
        const double* wp = wv + (size_t)(t - 1) * N;
        for (int a0 = 0; a0 < N; a0 += NT / 8) {
          const int a = a0 + gj;
          double v = 0.0;
          if (a < N)
            for (int i = gq; i < N; i += 8) v = fma(S[i * kNL + a], wp[i], v);
          v += dpp_d<0xB1>(v);
          v += dpp_d<0x4E>(v);
          v += dpp_d<0x141>(v);
          if (a < N && gq == 0) vec[a] = v + obs[(size_t)a * TP + t - 1] * irv[(size_t)a * TP + t - 1];
        }
      }
      __syncthreads();  // every read of M_t in LDS is done
      // S = D_t - G, D_t = 2Q + diag(ir_t) (t < T), D_T = Q + diag(ir_T)
      const double qf = (t == T) ? 1.0 : 2.0;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int pr = wave + 8 * j;
        if (pr < npair) {
          int A = 0, Bb = pr;
          while (Bb > A) {
            Bb -= A + 1;
            ++A;
          }
          const int b = 16 * Bb + lr;
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int a = 16 * A + lq + 4 * r4;
            if (a < N && b <= a) {
              double v = qf * Q[a * N + b] - g[j][r4];
              if (a == b) v += irv[(size_t)a * TP + t - 1];
              S[a * kNL + b] = v;
            }
          }
        }
      }
    } else {
      // S = D_0 = V0inv + Q; b_0 = V0inv h0mean
      for (int e = tid; e < N * N; e += NT) {
        const int a = e / N, b = e - a * N;
        if (b <= a) S[a * kNL + b] = V0[a + b * N] + Q[e];
      }
      for (int a = tid; a < N; a += NT) vec[a] = V0invm[(size_t)s * N + a];
    }
    __syncthreads();
    if (!(skip & 4)) wg_chol_inv<NT>(S, N, Tb, &bad);
    // w_t = Linv_t r (8 lanes per row), Linv_t -> global
    double* Lcur = Lt + (size_t)t * NN;
    for (int a0 = 0; a0 < N; a0 += NT / 8) {
      const int a = a0 + gj;
      double v = 0.0;
      if (a < N && !(skip & 8))
        for (int k = gq; k <= a; k += 8) v = fma(S[a * kNL + k], vec[k], v);
      v += dpp_d<0xB1>(v);
      v += dpp_d<0x4E>(v);
      v += dpp_d<0x141>(v);
      if (a < N && gq == 0) wv[(size_t)t * N + a] = v;
    }
    if (!(skip & 32))
      for (int e = tid; e < N * N; e += NT) {  // transposed: column b of Linv_t contiguous
        const int b = e / N, a = e - b * N;
        Lcur[e] = (b <= a) ? S[a * kNL + b] : 0.0;
      }
    __syncthreads();
  }
  // ---- backward: x_T = Linv_T'(w_T + z_T); x_t = Linv_t'(w_t + z_t + M_{t+1} x_{t+1})
  double* hout = cs.h + (size_t)c * N * TP;
  double* eta = cs.eta + (size_t)c * N * TP;
  double* sqh = cs.sqrtht + (size_t)c * N * TP;
  // Both products read rows of 8 lanes (M_{t+1} row a, Linv_t' row a = Linv_t column a, stored
  // transposed), and the next step's rows are loaded into registers while this step is computed,
  // so no global round trip sits between two steps of the recursion.
  constexpr int kRB = 16;  // row elements per lane (N <= 128: j = gq + 8 k)
  double pm[2][kRB], pl[2][kRB];
  auto load_m = [&](int tt) {  // M_{tt+1} rows a = gj, gj + 64 (zero at tt = T)
    const double* Mn = Mt + (size_t)(tt + 1) * NN;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < kRB; ++k) {
        const int a = 64 * h + gj, j = gq + 8 * k;
        pm[h][k] = (tt < T && a < N && j < N) ? Mn[a * N + j] : 0.0;
      }
  };
  auto load_l = [&](int tt) {  // Linv_tt(i, a), i >= a: row a of the transposed store
    const double* Li = Lt + (size_t)tt * NN;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < kRB; ++k) {
        const int a = 64 * h + gj, i = gq + 8 * k;
        pl[h][k] = (a < N && i < N && i >= a) ? Li[a * N + i] : 0.0;
      }
  };
  if (!(skip & 16)) {
    load_m(T);
    load_l(T);
  }
  // x_{T+1} := 0: the t = T product multiplies it by zero rows, and 0 * (stale LDS) may be NaN
  for (int a = tid; a < 128; a += NT) vec2[a] = 0.0;
  __syncthreads();
  for (int t = (skip & 16) ? -1 : T; t >= 0; --t) {
    // v = w_t + z_t + M_{t+1} x_{t+1}  (x_{t+1} in vec2)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int a = 64 * h + gj;
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < kRB; ++k) {
        const int j = gq + 8 * k;
        if (j < N) v = fma(pm[h][k], vec2[j], v);
      }
      v += dpp_d<0xB1>(v);
      v += dpp_d<0x4E>(v);
      v += dpp_d<0x141>(v);
      if (a < N && gq == 0)
        vec[a] = v + wv[(size_t)t * N + a] + rng.normal(CCMM_RNG_SVZ, (uint32_t)(a + N * t));
    }
    if (t > 0) load_m(t - 1);
    __syncthreads();
    // x_t(a) = sum_{i >= a} Linv_t(i, a) v(i)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int a = 64 * h + gj;
      double x = 0.0;
#pragma unroll
      for (int k = 0; k < kRB; ++k) {
        const int i = gq + 8 * k;
        if (i < N) x = fma(pl[h][k], vec[i], x);
      }
      x += dpp_d<0xB1>(x);
      x += dpp_d<0x4E>(x);
      x += dpp_d<0x141>(x);
      if (a < N && gq == 0) {
        if (t >= 1) {
          hout[(size_t)a * TP + t - 1] = x;
          sqh[(size_t)a * TP + t - 1] = exp(0.5 * x);
        }
        if (t < T) eta[(size_t)a * TP + t] = vec2[a] - x;  // shock of period t+1: h_{t+1} - h_t
        vec2[a] = x;  // every other read of vec2 precedes the barrier above
      }
    }
    if (t > 0) load_l(t - 1);
    __syncthreads();
  }
  if (bad && tid == 0) atomicOr(&cs.status[c], 8);
}

// ================================================================ host launchers
hipError_t bign_launch_astep(hipStream_t st, const Dims& d, const int* Tslot, ChainState cs, RngArgs ra,
                             double logy2offset, double* gbuf) {
  const int NPAD = bign_astep_npad(d);
  const int nt = NPAD / 64;
  const int ngr = (d.N - 1 + 3) / 4;
  hipError_t e = launch_k(k_astep_gram, dim3(nt * (nt + 1) / 2, d.B * ngr), dim3(256), 0, false, st, d, Tslot, cs, gbuf,
                          NPAD);
  if (e != hipSuccess) return e;
  e = launch_k(k_astep_big, dim3(d.N - 1, d.B), dim3(256), bign_astep_lds(), true, st, d, Tslot, cs, ra, gbuf, NPAD);
  if (e != hipSuccess) return e;
  return launch_k(k_astep_fin, dim3(d.B), dim3(256), bign_astep_fin_lds(d.N), true, st, d, Tslot, cs, logy2offset);
}

hipError_t bign_launch_phi(hipStream_t st, const Dims& d, const int* Tslot, int dPHI, const double* sPHI,
                           ChainState cs, double* scr) {
  return launch_k(k_phi_big, dim3(d.B), dim3(1024), bign_phi_lds(), true, st, d, Tslot, dPHI, sPHI, cs, scr);
}

hipError_t bign_launch_sv(hipStream_t st, const Dims& d, const int* Tslot, const double* V0inv,
                          const double* V0invm, ChainState cs, RngArgs ra, double* scr) {
  // CCMM_SV_SKIP: timing ablation of k_sv_big phases (1 M_t, 2 M_t'M_t, 4 Cholesky + inverse,
  // 8 forward product, 16 backward pass, 32 Linv_t store); results are wrong when set
  static const int skip = env_ablation("CCMM_SV_SKIP", 0);
  return launch_k(k_sv_big, dim3(d.B), dim3(kSvNT), bign_sv_lds(d.N), true, st, d, Tslot, V0inv, V0invm, cs, ra, scr,
                  bign_sv_scratch(d), skip);
}

}  // namespace ccmm

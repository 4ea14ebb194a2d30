// The GIRF inputs, Rao-Blackwellised responses and series sets of the stored draws (ccmm_girf_store.h).
// Built with -ffp-contract=off: every fused operation is an explicit fma(), so a draw's bits depend on its own
// stored values only, not on the batch or the pass it falls in.
#include "ccmm_girf_store.h"
#include "ccmm_internal.h"

namespace ccmm {

namespace {

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// one wave per pooled draw d = c * stored + m
__global__ __launch_bounds__(64) void k_girf_prep(GirfPrepArgs a) {
  extern __shared__ double sm[];  // PHI, then its factor: (i, j) at i + j N
  const int d = blockIdx.x, lane = threadIdx.x;
  const int c = d / a.stored, m = d - c * a.stored;
  const size_t rec = (size_t)c * a.cap + m;
  const int N = a.N, Np = N * a.p, nv = N * (N + 1) / 2;
  const double* ph = a.sPHI + rec * nv;
  int bad = 0;
  for (int e = lane; e < N * N; e += 64) {  // ivech: column cc of the lower triangle starts at cc N - cc (cc - 1) / 2
    const int i = e % N, j = e / N, r = i > j ? i : j, cc = i > j ? j : i;
    const double v = ph[cc * N - cc * (cc - 1) / 2 + (r - cc)];
    bad |= !finite_d(v);
    sm[e] = v;
  }
  bad = __any(bad);
  wave_lds_sync();
  // left-looking Cholesky, lane i owns row i: s = PHI(i, j) - sum_{k < j} L(i, k) L(j, k), k ascending, one fma
  // each; L(j, j) = sqrt(s_j), L(i, j) = s_i / L(j, j)
  for (int j = 0; j < N && !bad; ++j) {
    double s = 0.0;
    const bool mine = lane >= j && lane < N;
    if (mine) {
      s = sm[lane + j * N];
      for (int k = 0; k < j; ++k) s = fma(-sm[lane + k * N], sm[j + k * N], s);
    }
    const double piv = __shfl(s, j, 64);
    if (!(piv > 0.0) || !finite_d(piv)) {
      bad = 1;  // the same for every lane
      break;
    }
    const double dd = sqrt(piv);
    int b = 0;
    if (mine) {
      const double v = lane == j ? dd : s / dd;
      b = !finite_d(v);
      sm[lane + j * N] = v;
    }
    bad = __any(b);
    wave_lds_sync();
  }
  const double nan = __builtin_nan("");
  double* L = a.sqrtPHI + (size_t)d * N * N;
  for (int e = lane; e < N * N; e += 64) {
    const int i = e % N, j = e / N;
    L[e] = bad ? nan : (i >= j ? sm[e] : 0.0);
  }
  const double* sv = a.sSqrtht + rec * (size_t)a.T * N + a.svrow;
  for (int i = lane; i < N; i += 64) a.SV0[(size_t)d * N + i] = bad ? nan : sv[(size_t)i * a.T];
  const double* sh = a.sShadow ? a.sShadow + rec * (size_t)a.Ns * a.elbTmax : nullptr;
  double* X = a.Xj + (size_t)d * a.ldX;
  for (int e = lane; e < a.ldX; e += 64) {
    double v = 1.0;
    if (e > 0) {
      int l, j;
      if (e <= Np) {
        l = (e - 1) / N;
        j = e - 1 - l * N;
      } else {
        const int q = e - 1 - Np;
        l = q / a.Ny;
        j = a.yidx[q - l * a.Ny];
      }
      v = a.jump[l * N + j];
      const int mo = a.npatch - 1 - l;  // month of the draw's shadow rates that lag l falls on
      if (sh && mo >= 0)
        for (int s = 0; s < a.Ns; ++s)
          if (a.ndxS[s] == j) v = sh[s + (size_t)a.Ns * mo];
    }
    X[e] = bad ? nan : v;
  }
  if (lane == 0) a.info[d] = bad ? 1 : 0;
}

// one wave per pooled draw, lane i owns equation i.  LDS: coef[i * stride + r] = PAI(r, i) | ring of p + 1 blocks
// of N (state block l is ring block (head + l) mod (p + 1); the new y goes into the free block, the next head)
__global__ __launch_bounds__(64) void k_girf_rb(GirfRbArgs a, int stride) {
  extern __shared__ double sm[];
  const int d = blockIdx.x, lane = threadIdx.x;
  const int c = d / a.stored, m = d - c * a.stored;
  const size_t rec = (size_t)c * a.cap + m;
  const int N = a.N, p = a.p, H = a.H, R = 1 + N * p;
  double* coef = sm;
  double* ring = sm + (size_t)N * stride;
  double* Y = a.rb + (size_t)d * 2 * H * N;
  double* I = Y + (size_t)H * N;
  if (a.info[d]) {
    for (int e = lane; e < 2 * H * N; e += 64) Y[e] = __builtin_nan("");
    return;
  }
  const double* P = a.sPAI + rec * (size_t)a.K * N;
  const double* iA = a.sInvA + rec * (size_t)N * N;
  const double* Xj = a.Xj + (size_t)d * a.ldX;
  for (int e = lane; e < R * N; e += 64) {
    const int i = e / R, r = e - i * R;
    coef[i * stride + r] = P[(size_t)i * a.K + r];
  }
  const bool cum = a.cumcode && lane < N && a.cumcode[lane];
  for (int path = 0; path < 2; ++path) {
    // YhatRBdraws: the state is the jump-off; IRF1RBdraws: invA(:, 1) shock11 in the first block, zeros behind it
    for (int e = lane; e < N * p; e += 64) ring[e] = path == 0 ? Xj[1 + e] : (e < N ? iA[e] * a.shock11 : 0.0);
    wave_lds_sync();
    double* out = path == 0 ? Y : I;
    double run = 0.0;
    int head = 0;
    for (int h = 0; h < H; ++h) {
      const int free = head == 0 ? p : head - 1;
      if (lane < N) {
        const double* ci = coef + (size_t)lane * stride;
        double acc = path == 0 ? ci[0] : 0.0;
        int k = 1;
        for (int l = 0, b = head; l < p; ++l, b = b == p ? 0 : b + 1) {
          const double* x = ring + b * N;
          for (int cc = 0; cc < N; ++cc, ++k) acc = fma(ci[k], x[cc], acc);
        }
        ring[free * N + lane] = acc;
        double v = path == 0 ? acc : ring[head * N + lane];  // the response of horizon h is the state before the step
        if (cum) {
          run += v;
          v = run / a.np_;
        }
        out[(size_t)h * N + lane] = v;
      }
      wave_lds_sync();
      head = free;
    }
  }
}

// seg[(set S + s) n + d0 + m], m fastest over the threads
__global__ void k_girf_collect(int mc, int d0, int n, int S, const double* __restrict__ out, double* __restrict__ seg) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)mc * S) return;
  const int s = (int)(q / mc), m = (int)(q - (size_t)s * mc);
  const double* o = out + (size_t)m * 3 * S + s;
  const double base = o[0], plus = o[S], minus = o[2 * (size_t)S];
  double* g = seg + (size_t)s * n + d0 + m;
  const size_t set = (size_t)S * n;
  g[0] = base;
  g[set] = plus;
  g[2 * set] = minus;
  g[3 * set] = plus - base;
  g[4 * set] = minus - base;
}

__global__ void k_girf_collect_rb(int n, int S, const double* __restrict__ rb, double* __restrict__ seg) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)n * S) return;
  const int s = (int)(q / n), m = (int)(q - (size_t)s * n);
  const double* o = rb + (size_t)m * 2 * S + s;
  seg[(size_t)s * n + m] = o[0];
  seg[((size_t)S + s) * n + m] = o[S];
}

}  // namespace

hipError_t girf_prep_launch(hipStream_t st, const GirfPrepArgs& a) {
  return launch_k(k_girf_prep, dim3(a.n), dim3(64), girf_prep_lds(a.N), false, st, a);
}

hipError_t girf_rb_launch(hipStream_t st, const GirfRbArgs& a) {
  const size_t lds = girf_rb_lds(a.N, a.p);
  return launch_k(k_girf_rb, dim3(a.n), dim3(64), lds, lds > kLdsDefault, st, a, girf_rb_stride(a.N, a.p));
}

hipError_t girf_collect_launch(hipStream_t st, int mc, int d0, int n, int S, const double* out, double* seg) {
  const size_t nt = (size_t)mc * S;
  return launch_k(k_girf_collect, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, false, st, mc, d0, n, S, out, seg);
}

hipError_t girf_collect_rb_launch(hipStream_t st, int n, int S, const double* rb, double* seg) {
  const size_t nt = (size_t)n * S;
  return launch_k(k_girf_collect_rb, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, false, st, n, S, rb, seg);
}

}  // namespace ccmm

// Impulse responses (VMA coefficients) of VAR coefficient draws (ccmm_vma.hip): for each of M matrices PAI
// (K x N column-major), Psi_h = (comp^h)(1:N, 1:N), h = 1..H, comp the N p x N p companion matrix
// (goVARshadowrateBlockHybrid.m:393-408 drawsVMA).
//
// The lower block of the companion is a shift, so comp^h (:, 1:N) = [Psi_h; Psi_{h-1}; ...; Psi_{h-p+1}] and
//
//   Psi_h = sum_{l = 1..p} Phi_l Psi_{h-l},   Psi_0 = I,  Psi_{<0} = 0,   Phi_l = PAI(1 + (l-1) N + (1:N), :)':
//
// the as-written dense product with its exact zeros removed.  With A = [Phi_1 .. Phi_p] (N x N p) and the ring
// R_h = [Psi_{h-1}; ..; Psi_{h-p}] (N p x N) a horizon is the one product Psi_h = A R_h.
//
// One core, two builds.  vma_core below is written once for a lane group G: it stages A, screens the input,
// runs the recursion from h = 1 and writes the horizons of the window.  The group supplies the product: the
// device groups (ccmm_vma.hip) one 16 x 16 tile per wave on v_mfma_f64_16x16x4_f64, or one element chain per
// thread on the vector ALU; the host twin (W = 1) an fma chain per element.  Every element of Psi_h is one
// accumulator chain over k = 0 .. 4 ceil(N p / 4) - 1 ascending (lags ascending, columns ascending within a
// lag, zeros beyond N p), each step one fused multiply-add -- the order inside the MFMA is four fused
// multiply-adds in k order (tools/probe_mfma_order.py) -- and every lag is multiplied through, the zero ring
// blocks at h < p included.  So the bits of a draw depend on its own PAI only, not on the batch, the window or
// the build.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ccmm_eig.h"  // EigSrc, kEigMaxN

namespace ccmm {

// ---- launch arithmetic (host, no HIP call)
constexpr int kVmaMaxN = 32;                      // device path: N <= 32 (at most 2 x 2 tiles of 16 x 16) ...
constexpr int kVmaMaxNp = kEigMaxN;               // ... and N p <= 256, the order the root kernel serves
constexpr size_t kVmaStage = 16;                  // LDS beside A and the ring: the screen's flag
constexpr size_t kVmaBufCap = (size_t)1 << 30;    // every buffer of one pass (draw-major, segments, sorted): <= 1 GB

struct VmaPlan {
  int device;   // 1: the device path serves this shape; 0: the host twin
  int tiles;    // 16 x 16 output tiles, one wave each: ceil(N / 16)^2
  int threads;  // workgroup size: 64 tiles; one workgroup per draw
  size_t lds;   // dynamic LDS of a workgroup: A (N x N p) and the ring (N p x N) in doubles, plus kVmaStage
  int hslab;    // horizons per pass: the most whose n N N hslab doubles stay within the cap, at least 1
  int nslab;    // passes: ceil(H / hslab)
  int last;     // horizons of the last pass
  size_t buf;   // bytes of one buffer of a full pass
};
inline VmaPlan vma_plan(int N, int p, long long n, int H, size_t cap = kVmaBufCap) {
  VmaPlan pl{};
  if (N < 1 || p < 1 || n < 1 || H < 1) return pl;
  const long long Np = (long long)N * p;
  pl.device = N <= kVmaMaxN && Np <= kVmaMaxNp;
  const int nt = (N + 15) / 16;
  pl.tiles = nt * nt;
  pl.threads = 64 * pl.tiles;
  pl.lds = 2 * (size_t)N * (size_t)Np * sizeof(double) + kVmaStage;
  const size_t per = (size_t)n * N * N * sizeof(double);  // one horizon of every draw
  const size_t fit = cap / per;
  pl.hslab = fit < 1 ? 1 : (fit < (size_t)H ? (int)fit : H);
  pl.nslab = (H + pl.hslab - 1) / pl.hslab;
  pl.last = H - (pl.nslab - 1) * pl.hslab;
  pl.buf = per * pl.hslab;
  return pl;
}

// ---- the core
// LDS / host layout: A[k N + i] = Phi(i, k) (i fastest), ring[s N N + c N + j] = Psi_{h}(c, j) in block s = h mod p
// (j fastest).  The group G has lane(), sync(), W and
//   product(A, ring, N, p, h)   Psi_h = A R_h into ring block h mod p (which holds Psi_{h-p}, read by the product)
//   flag(stage, bad)            the OR of `bad` over the lanes, through *stage
template <class G>
__host__ __device__ inline int vma_core(const G& g, const double* PAI, int ld, int N, int p, int h0, int h1,
                                        double* out, double* A, double* ring, int* stage) {
  const int Np = N * p, NN = N * N;
  // A(i, k) = PAI(1 + k, i); the screen over the same N p x N coefficients (the intercept row is ignored)
  int bad = 0;
  for (int e = g.lane(); e < Np * N; e += G::W) {
    const int k = e % Np, i = e / Np;
    const double v = PAI[(size_t)i * ld + 1 + k];
    bad |= !(fabs(v) <= 1.79769313486231570815e308);
    A[k * N + i] = v;
  }
  bad = g.flag(stage, bad);
  if (bad) {
    const double nan = __builtin_nan("");
    for (int e = g.lane(); e < (h1 - h0) * NN; e += G::W) out[e] = nan;
    return 1;
  }
  // Psi_0 = I in block 0, Psi_{<0} = 0
  for (int e = g.lane(); e < Np * N; e += G::W) ring[e] = (e < NN && e / N == e % N) ? 1.0 : 0.0;
  g.sync();
  for (int h = 1; h <= h1; ++h) {
    g.product(A, ring, N, p, h);
    if (h > h0) {  // horizon h is entry h - 1 of the H horizons: out[(h - 1 - h0)][j][i], i fastest
      const double* src = ring + (size_t)(h % p) * NN;
      double* dst = out + (size_t)(h - 1 - h0) * NN;
      for (int e = g.lane(); e < NN; e += G::W) dst[e] = src[(e % N) * N + e / N];
    }
  }
  return 0;
}

// the host twin's group: one lane; every element one fma chain in the kernel's k order
struct VmaSerial {
  static constexpr int W = 1;
  double* tmp;  // N x N
  inline int lane() const { return 0; }
  inline void sync() const {}
  inline int flag(int*, int bad) const { return bad; }
  void product(const double* A, double* ring, int N, int p, int h) const;
};

// ---- the two builds
// host twin: M draws on at most 16 threads; vma[m][h][j][i] for the H horizons; info may be null
void vma_host(int M, int N, int p, int H, const EigSrc& src, double* vma, int* info);
// device: draws m = 0..M-1 at src (device), horizons [h0, h1) of each into out[m][h - h0][j][i] (device), info[m]
// (device, not null).  form 0: the MFMA product, 1: the vector-ALU product (the same bits)
hipError_t vma_launch(hipStream_t st, int form, int M, int N, int p, const EigSrc& src, int h0, int h1, double* out,
                      int* info);
// sumFFR: dst[n * M + m] = sum_{l = 0..p-1} PAI_m(1 + l N + ffr, n), plain adds in ascending lag (device)
hipError_t vma_launch_sum_ffr(hipStream_t st, int M, int N, int p, const EigSrc& src, int ffr, double* dst);

}  // namespace ccmm

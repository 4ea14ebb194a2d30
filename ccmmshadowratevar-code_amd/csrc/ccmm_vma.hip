// Batched impulse responses of VAR coefficient draws: the device kernels and the host twin of ccmm_vma.h.
//
// Mapping.  One workgroup per draw.  A = [Phi_1 .. Phi_p] (N x N p) and the ring of the last p responses
// (N p x N) stay in LDS for the whole recursion (77 KB at N = 20, p = 12; 131 KB at N = 32, p = 8), so a
// horizon reads nothing from memory and writes N^2 doubles.  Each horizon is one N x N x N p product on
// v_mfma_f64_16x16x4_f64: one wave per 16 x 16 output tile (at most four), operand and accumulator lane maps
// those of ccmm_selftest_mfma_f64 (lane l: A(l & 15, l >> 4), B(l >> 4, l & 15), D((l >> 4) + 4 r, l & 15)),
// tile edges and the k remainder read as zeros.  One accumulator chain per tile over k ascending.  The new
// block replaces the oldest one of the ring, which the product still reads: a barrier separates the two.  The
// horizons of the window go out draw-major, V[draw][h][j][i], i fastest across the lanes.
//
// k_vma_valu is the same recursion on the vector ALU (one element chain per thread, explicit fma in the same k
// order): the comparison form of DESIGN §12, bit-identical.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

#include "../../include/ccmm.h"
#include "ccmm_err.h"
#include "ccmm_internal.h"
#include "ccmm_vma.h"

namespace ccmm {

// host twin: element (i, j) of Psi_h, one chain over the padded k range
void VmaSerial::product(const double* A, double* ring, int N, int p, int h) const {
  const int Np = N * p, NN = N * N, Np4 = (Np + 3) / 4 * 4;
  const int s0 = (h - 1) % p;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      double acc = 0.0;
      int k = 0;
      for (int lag = 0; lag < p; ++lag) {
        const int s = s0 - lag < 0 ? s0 - lag + p : s0 - lag;
        const double* blk = ring + (size_t)s * NN;
        for (int c = 0; c < N; ++c, ++k) acc = std::fma(A[k * N + i], blk[c * N + j], acc);
      }
      for (; k < Np4; ++k) acc = std::fma(0.0, 0.0, acc);
      tmp[i * N + j] = acc;
    }
  double* dst = ring + (size_t)(h % p) * NN;
  for (int e = 0; e < NN; ++e) dst[e] = tmp[e];
}

namespace {

__host__ __device__ inline const double* vma_src(const EigSrc& s, long long m) {
  return s.PAI + (m % s.na) * s.sa + (m / s.na) * s.sb;
}

// the workgroup as a lane group: what the two device forms share
struct VmaGroupBase {
  __device__ inline int lane() const { return threadIdx.x; }
  __device__ inline void sync() const { __syncthreads(); }
  __device__ inline int flag(int* stage, int bad) const {
    if (threadIdx.x == 0) *stage = 0;
    __syncthreads();
    if (bad) *stage = 1;
    __syncthreads();
    return *stage;
  }
};

// one wave per 16 x 16 tile on the MFMA
template <int THREADS>
struct VmaMfma : VmaGroupBase {
  static constexpr int W = THREADS;
  __device__ inline void product(const double* A, double* ring, int N, int p, int h) const {
    const int Np = N * p, NN = N * N, nk = (Np + 3) / 4;
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = THREADS == 64 ? 1 : 2;
    const int ti = wave % nt, tj = wave / nt;
    const int lr = l & 15, lq = l >> 4;
    const int i = 16 * ti + lr, j = 16 * tj + lr;
    const bool iok = i < N, jok = j < N;
    const int s0 = (h - 1) % p;
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    int k = lq, c = lq, s = s0;
    while (c >= N) {
      c -= N;
      s = s == 0 ? p - 1 : s - 1;
    }
    for (int ks = 0; ks < nk; ++ks) {
      const bool kok = k < Np;
      const double a = (iok && kok) ? A[k * N + i] : 0.0;
      const double b = (jok && kok) ? ring[s * NN + c * N + j] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      k += 4;
      c += 4;
      while (c >= N) {
        c -= N;
        s = s == 0 ? p - 1 : s - 1;
      }
    }
    __syncthreads();  // every wave has read block h mod p (Psi_{h-p}) before it is replaced
    double* dst = ring + (h % p) * NN;
    if (jok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int io = 16 * ti + lq + 4 * r;
        if (io < N) dst[io * N + j] = acc[r];
      }
    }
    __syncthreads();
  }
};

// one element chain per thread on the vector ALU, the same k order
template <int THREADS>
struct VmaValu : VmaGroupBase {
  static constexpr int W = THREADS;
  static constexpr int kPer = (kVmaMaxN * kVmaMaxN + THREADS - 1) / THREADS;
  __device__ inline void product(const double* A, double* ring, int N, int p, int h) const {
    const int Np = N * p, NN = N * N;
    const int s0 = (h - 1) % p;
    double acc[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int e = threadIdx.x + q * THREADS;  // e = i N + j
      acc[q] = 0.0;
      if (e < NN) {
        const int i = e / N, j = e % N;
        double v = 0.0;
        int k = 0;
        for (int lag = 0; lag < p; ++lag) {
          const int s = s0 - lag < 0 ? s0 - lag + p : s0 - lag;
          const double* blk = ring + s * NN + j;
          for (int c = 0; c < N; ++c, ++k) v = __builtin_fma(A[k * N + i], blk[c * N], v);
        }
        if (Np & 3) v = __builtin_fma(0.0, 0.0, v);  // the zero steps of the k remainder (-0 becomes +0)
        acc[q] = v;
      }
    }
    __syncthreads();
    double* dst = ring + (h % p) * NN;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int e = threadIdx.x + q * THREADS;
      if (e < NN) dst[e] = acc[q];
    }
    __syncthreads();
  }
};

template <class G>
__global__ __launch_bounds__(G::W) void k_vma(int M, int N, int p, EigSrc src, int h0, int h1, double* __restrict__ out,
                                              int* __restrict__ info) {
  extern __shared__ double vma_lds[];
  const long long m = blockIdx.x;
  if (m >= M) return;
  const int Np = N * p;
  double* A = vma_lds;
  double* ring = A + (size_t)N * Np;
  int* stage = reinterpret_cast<int*>(ring + (size_t)N * Np);
  const G g;
  const int fl = vma_core(g, vma_src(src, m), src.ld, N, p, h0, h1, out + (size_t)m * (h1 - h0) * N * N, A, ring, stage);
  if (threadIdx.x == 0) info[m] = fl;
}

__global__ __launch_bounds__(256) void k_sum_ffr(int M, int N, int p, EigSrc src, int ffr, double* __restrict__ dst) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (long long)M * N) return;
  const long long m = q / N;
  const int n = (int)(q % N);
  const double* col = vma_src(src, m) + (size_t)n * src.ld + 1 + ffr;
  double s = col[0];
  for (int l = 1; l < p; ++l) s = s + col[(size_t)l * N];
  dst[(size_t)n * M + m] = s;
}

template <class G>
hipError_t vma_launch_g(hipStream_t st, size_t lds, int M, int N, int p, const EigSrc& src, int h0, int h1, double* out,
                        int* info) {
  return launch_k(k_vma<G>, dim3(M), dim3(G::W), lds, lds > kLdsDefault, st, M, N, p, src, h0, h1, out, info);
}

}  // namespace

hipError_t vma_launch(hipStream_t st, int form, int M, int N, int p, const EigSrc& src, int h0, int h1, double* out,
                      int* info) {
  const VmaPlan pl = vma_plan(N, p, M, h1);
  if (!pl.device || h0 < 0 || h0 >= h1 || (form != 0 && form != 1)) return hipErrorInvalidValue;
  if (form == 1) return vma_launch_g<VmaValu<256>>(st, pl.lds, M, N, p, src, h0, h1, out, info);
  if (pl.tiles == 1) return vma_launch_g<VmaMfma<64>>(st, pl.lds, M, N, p, src, h0, h1, out, info);
  return vma_launch_g<VmaMfma<256>>(st, pl.lds, M, N, p, src, h0, h1, out, info);
}

hipError_t vma_launch_sum_ffr(hipStream_t st, int M, int N, int p, const EigSrc& src, int ffr, double* dst) {
  const long long total = (long long)M * N;
  return launch_k(k_sum_ffr, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, false, st, M, N, p, src, ffr, dst);
}

void vma_host(int M, int N, int p, int H, const EigSrc& src, double* vma, int* info) {
  const size_t Np = (size_t)N * p, NN = (size_t)N * N;
  std::atomic<int> next{0};
  auto work = [&] {
    std::vector<double> A(N * Np), ring(N * Np), tmp(NN);
    const VmaSerial g{tmp.data()};
    int stage = 0;
    for (int m; (m = next++) < M;) {
      const int fl = vma_core(g, vma_src(src, m), src.ld, N, p, 0, H, vma + (size_t)m * H * NN, A.data(), ring.data(),
                              &stage);
      if (info) info[m] = fl;
    }
  };
  const unsigned nth = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
  std::vector<std::thread> th;
  for (unsigned i = 1; i < std::min<unsigned>(nth, (unsigned)M); ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

}  // namespace ccmm

extern "C" int ccmm_vma_host(int M, int N, int p, int K, int H, const double* PAI, double* vma, int* info) {
  if (M < 0 || N < 1 || p < 1 || H < 1 || (long long)N * p + 1 > K || (M > 0 && (!PAI || !vma))) {
    ccmm::set_last_error("ccmm_vma_host: need M >= 0, N, p, H >= 1, K >= 1 + N p, PAI and vma");
    return CCMM_ERR_ARG;
  }
  try {
    ccmm::vma_host(M, N, p, H, ccmm::EigSrc{PAI, K, M > 0 ? M : 1, (long long)K * N, 0}, vma, info);
  } catch (const std::exception& e) {  // allocation or thread start
    ccmm::set_last_error(e.what());
    return CCMM_ERR_HIP;
  }
  return CCMM_OK;
}

// Spectral radius of VAR companion matrices (ccmm_eig.hip): max |eig(comp)| of the n x n companion,
// n = N p, of each of M coefficient matrices PAI (K x N column-major), in fp64, eigenvalues only.
//
//   reduce   Householder reduction to upper Hessenberg form (Martin & Wilkinson 1968, "orthes")
//   iterate  implicit double-shift QR on the active window (Francis 1961; Martin, Peters & Wilkinson 1970,
//            "hqr"; Golub & Van Loan, Matrix Computations, alg. 7.5.1), nothing outside the window updated
//   blocks   the moduli of a deflated 2 x 2 block from its standardised form (real Schur form with equal
//            diagonal when the pair is complex; Bai & Demmel 1993, as in LAPACK's dlanv2)
//
// One core, two builds.  eig_core below is written once for a "lane group" G of G::W lanes: the device
// build runs it with one wave per matrix (W = 64), the host twin with W = 1.  The lanes split the
// elementwise work of every reflector (one column or one row of the update per lane, the inner sum of a
// column or row in a fixed serial order), and every quantity that steers the iteration (norms, shifts,
// reflectors, deflation tests) is computed by every lane from the same stored elements.  There is no
// cross-lane reduction, so each stored element sees the same operations in the same order whatever W is:
// the two builds agree bit for bit.  The unit is compiled with -ffp-contract=off and uses + - * / sqrt and
// fabs only (each correctly rounded on both sides); no library hypot.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ccmm {

// ---- launch arithmetic (host, no HIP call)
constexpr int kEigMaxN = 256;             // largest companion order of the device path
constexpr int kEigWaves = 4;              // matrices (waves) per workgroup
constexpr int kEigItsPerRow = 30;         // QR iterations per matrix are capped at kEigItsPerRow * n
constexpr size_t kEigScratchCap = (size_t)1 << 30;  // scratch of one launch: at most 1 GB
// check_stationarity evaluates a few roots per sweep, and one matrix is a dependent chain: at order 240 a wave
// needs 0.36 s whether the launch holds 1 or 1000 matrices, one host thread 16 ms.  Below this many
// open chains the sweep takes the host twin (16 threads, same bits), from it on the kernel.
constexpr int kEigHostBelow = 352;

struct EigPlan {
  int device;      // 1: the device path serves this order; 0: the host twin
  int threads;     // workgroup size: kEigWaves waves, one matrix each
  int chunk;       // matrices per launch (scratch of a launch <= kEigScratchCap)
  int launches;    // ceil(M / chunk)
  int grid;        // workgroups of a full launch: ceil(chunk / kEigWaves)
  size_t lds;      // static LDS bytes of a workgroup: one reflector of kEigMaxN doubles per wave
  size_t scratch;  // scratch bytes of a launch: n^2 doubles per matrix in flight
};
inline EigPlan eig_plan(int n, int M) {
  EigPlan pl{};
  pl.threads = 64 * kEigWaves;
  pl.lds = (size_t)kEigWaves * kEigMaxN * sizeof(double);
  pl.device = n >= 1 && n <= kEigMaxN && M >= 1;
  if (!pl.device) return pl;
  const size_t per = (size_t)n * n * sizeof(double);
  const size_t fit = kEigScratchCap / per;  // >= 2048 at n = 256
  pl.chunk = (size_t)M < fit ? M : (int)fit;
  pl.launches = (M + pl.chunk - 1) / pl.chunk;
  pl.grid = (pl.chunk + kEigWaves - 1) / kEigWaves;
  pl.scratch = (size_t)pl.chunk * per;
  return pl;
}

// ---- addressing
// the working matrix: column-major, leading dimension ld
struct EigMat {
  double* a;
  int ld;
  __host__ __device__ inline double& operator()(int i, int j) const { return a[(size_t)j * ld + i]; }
};
// the host twin's lane group: one lane, nothing to order
struct EigSerial {
  static constexpr int W = 1;
  __host__ __device__ inline int lane() const { return 0; }
  __host__ __device__ inline void sync() const {}
};

__host__ __device__ inline double eig_sign(double a, double b) { return b >= 0.0 ? fabs(a) : -fabs(a); }
__host__ __device__ inline double eig_max(double a, double b) { return a > b ? a : b; }
__host__ __device__ inline double eig_min(double a, double b) { return a < b ? a : b; }
// sqrt(a^2 + b^2) without overflow, in operations both builds round alike
__host__ __device__ inline double eig_pythag(double a, double b) {
  const double x = fabs(a), y = fabs(b);
  const double w = eig_max(x, y), z = eig_min(x, y);
  if (z == 0.0) return w;
  const double t = z / w;
  return w * sqrt(1.0 + t * t);
}

// larger modulus of the two eigenvalues of [a b; c d], from the standardised block
__host__ __device__ inline double eig_block_modulus(double a, double b, double c, double d) {
  const double eps = 2.220446049250313e-16;
  if (c == 0.0) {
  } else if (b == 0.0) {  // swap rows and columns
    const double t = d;
    d = a;
    a = t;
    b = -c;
    c = 0.0;
  } else if (a - d == 0.0 && (b > 0.0) != (c > 0.0)) {  // already standard: complex pair
  } else {
    const double temp = a - d;
    double p = 0.5 * temp;
    const double bcmax = eig_max(fabs(b), fabs(c));
    const double bcmis = eig_min(fabs(b), fabs(c)) * eig_sign(1.0, b) * eig_sign(1.0, c);
    const double scale = eig_max(fabs(p), bcmax);
    double z = p / scale * p + bcmax / scale * bcmis;
    if (z >= 4.0 * eps) {  // real eigenvalues
      z = p + eig_sign(sqrt(scale) * sqrt(z), p);
      a = d + z;
      d = d - bcmax / z * bcmis;
      b = b - c;
      c = 0.0;
    } else {  // complex, or real and almost equal: make the diagonal equal
      const double sigma = b + c;
      const double tau = eig_pythag(sigma, temp);
      const double cs = sqrt(0.5 * (1.0 + fabs(sigma) / tau));
      const double sn = -(p / (tau * cs)) * eig_sign(1.0, sigma);
      const double aa = a * cs + b * sn, bb = -a * sn + b * cs;
      const double cc = c * cs + d * sn, dd = -c * sn + d * cs;
      a = aa * cs + cc * sn;
      b = bb * cs + dd * sn;
      c = -aa * sn + cc * cs;
      d = -bb * sn + dd * cs;
      const double mid = 0.5 * (a + d);
      a = mid;
      d = mid;
      if (c != 0.0) {
        if (b != 0.0) {
          if ((b > 0.0) == (c > 0.0)) {  // real: reduce to upper triangular
            const double sab = sqrt(fabs(b)), sac = sqrt(fabs(c));
            p = eig_sign(sab * sac, c);
            a = mid + p;
            d = mid - p;
            b = b - c;
            c = 0.0;
          }
        } else {
          b = -c;
          c = 0.0;
        }
      }
    }
  }
  if (c == 0.0) return eig_max(fabs(a), fabs(d));
  return eig_pythag(a, sqrt(fabs(b)) * sqrt(fabs(c)));
}

// 1 when the n x N coefficient block of PAI (rows 1..n of K, leading dimension ld) holds a NaN or an Inf.
// Every lane reads every element: the answer is uniform without a reduction.
template <class G>
__host__ __device__ inline int eig_screen(const G& g, const double* PAI, int ld, int N, int n) {
  int bad = 0;
  for (int j = 0; j < N; ++j)
    for (int i = 1; i <= n; ++i) {
      const double v = PAI[(size_t)j * ld + i];
      bad |= !(fabs(v) <= 1.79769313486231570815e308);
    }
  return bad;
}

// H <- companion of PAI: rows 0..N-1 = PAI(1:1+n, :)', the shifted identity below
template <class G>
__host__ __device__ inline void eig_fill(const G& g, const EigMat& H, const double* PAI, int ld, int N, int n) {
  for (int j = 0; j < n; ++j)
    for (int i = g.lane(); i < n; i += G::W) H(i, j) = i < N ? PAI[(size_t)i * ld + 1 + j] : (i - N == j ? 1.0 : 0.0);
  g.sync();
}

// Householder reduction of H to upper Hessenberg form.  ort: n doubles shared by the lane group.
template <class G>
__host__ __device__ inline void eig_hessenberg(const G& g, const EigMat& H, int n, double* ort) {
  for (int k = 0; k + 2 < n; ++k) {
    const int m = k + 1;
    // column k below the diagonal -> ort (one element per lane), then its 1-norm by every lane
    for (int i = m + g.lane(); i < n; i += G::W) ort[i] = H(i, k);
    g.sync();
    double scale = 0.0;
    for (int i = m; i < n; ++i) scale = scale + fabs(ort[i]);
    if (scale == 0.0) {
      g.sync();
      continue;
    }
    g.sync();
    for (int i = m + g.lane(); i < n; i += G::W) ort[i] = ort[i] / scale;
    g.sync();
    double h = 0.0;
    for (int i = n - 1; i >= m; --i) h = h + ort[i] * ort[i];
    const double om = ort[m];
    const double gg = -eig_sign(sqrt(h), om);
    h = h - om * gg;
    g.sync();
    if (g.lane() == 0) ort[m] = om - gg;
    g.sync();
    // (I - u u' / h) H: one column per lane
    for (int j = m + g.lane(); j < n; j += G::W) {
      double f = 0.0;
      for (int i = n - 1; i >= m; --i) f = f + ort[i] * H(i, j);
      f = f / h;
      for (int i = m; i < n; ++i) H(i, j) = H(i, j) - f * ort[i];
    }
    g.sync();
    // H (I - u u' / h): one row per lane
    for (int i = g.lane(); i < n; i += G::W) {
      double f = 0.0;
      for (int j = n - 1; j >= m; --j) f = f + ort[j] * H(i, j);
      f = f / h;
      for (int j = m; j < n; ++j) H(i, j) = H(i, j) - f * ort[j];
    }
    // column k: the reflector maps it to (scale gg) e_m
    for (int i = m + g.lane(); i < n; i += G::W) H(i, k) = i == m ? scale * gg : 0.0;
    g.sync();
  }
}

// Implicit double-shift QR on the Hessenberg matrix H, eigenvalues only.  Returns max |lambda| in *rho;
// the return value is 0, or 2 when kEigItsPerRow * n iterations did not deflate every eigenvalue.
template <class G>
__host__ __device__ inline int eig_qr(const G& g, const EigMat& H, int n, double* rho) {
  const double eps = 2.220446049250313e-16;
  double norm = 0.0;  // fallback scale of the deflation test
  for (int j = 0; j < n; ++j)
    for (int i = 0; i <= (j + 1 < n ? j + 1 : n - 1); ++i) norm = norm + fabs(H(i, j));
  double best = 0.0;
  int hi = n - 1, its = 0, stall = 0;
  const int cap = kEigItsPerRow * n;
  while (hi >= 0) {
    // the lowest negligible subdiagonal element of the window
    int l = hi;
    for (; l > 0; --l) {
      double s = fabs(H(l - 1, l - 1)) + fabs(H(l, l));
      if (s == 0.0) s = norm;
      if (fabs(H(l, l - 1)) <= eps * s) break;
    }
    if (l == hi) {  // one real root
      best = eig_max(best, fabs(H(hi, hi)));
      hi -= 1;
      stall = 0;
      continue;
    }
    if (l == hi - 1) {  // a 2 x 2 block
      best = eig_max(best, eig_block_modulus(H(hi - 1, hi - 1), H(hi - 1, hi), H(hi, hi - 1), H(hi, hi)));
      hi -= 2;
      stall = 0;
      continue;
    }
    if (its >= cap) {
      *rho = best;
      return 2;
    }
    ++its;
    ++stall;
    // shifts: the eigenvalues of the trailing 2 x 2 block, or an exceptional pair every tenth stalled pass
    double x = H(hi, hi), y = H(hi - 1, hi - 1), w = H(hi, hi - 1) * H(hi - 1, hi);
    if (stall % 10 == 0) {
      const double s = fabs(H(hi, hi - 1)) + fabs(H(hi - 1, hi - 2));
      x = x + 0.75 * s;
      y = x;
      w = -0.4375 * s * s;
    }
    // start row m: two consecutive small subdiagonal elements
    int m = hi - 2;
    double p = 0.0, q = 0.0, r = 0.0;
    for (; m >= l; --m) {
      const double z = H(m, m);
      const double rr = x - z, ss = y - z;
      p = (rr * ss - w) / H(m + 1, m) + H(m, m + 1);
      q = H(m + 1, m + 1) - z - rr - ss;
      r = H(m + 2, m + 1);
      const double s = fabs(p) + fabs(q) + fabs(r);
      if (s != 0.0) {
        p = p / s;
        q = q / s;
        r = r / s;
      }
      if (m == l) break;
      const double u = fabs(H(m, m - 1)) * (fabs(q) + fabs(r));
      const double v = fabs(p) * (fabs(H(m - 1, m - 1)) + fabs(z) + fabs(H(m + 1, m + 1)));
      if (u <= eps * v) break;
    }
    g.sync();
    // chase the bulge down the window
    for (int k = m; k < hi; ++k) {
      const bool three = k != hi - 1;
      double sc = 1.0;
      if (k != m) {
        p = H(k, k - 1);
        q = H(k + 1, k - 1);
        r = three ? H(k + 2, k - 1) : 0.0;
        sc = fabs(p) + fabs(q) + fabs(r);
        if (sc != 0.0) {
          p = p / sc;
          q = q / sc;
          r = r / sc;
        }
      }
      g.sync();  // every lane has read column k - 1 before lane 0 rewrites it
      if (sc == 0.0) continue;
      const double s = eig_sign(sqrt(p * p + q * q + r * r), p);
      if (s == 0.0) continue;  // p = q = r = 0 at k = m: nothing to reflect
      if (g.lane() == 0) {
        if (k != m) {
          H(k, k - 1) = -s * sc;
          H(k + 1, k - 1) = 0.0;
          if (three) H(k + 2, k - 1) = 0.0;
        } else if (l != m) {
          H(k, k - 1) = -H(k, k - 1);
        }
      }
      p = p + s;
      const double hx = p / s, hy = q / s, hz = r / s;
      q = q / p;
      r = r / p;
      // rows k..k+2, columns k..hi: one column per lane
      for (int j = k + g.lane(); j <= hi; j += G::W) {
        double t = H(k, j) + q * H(k + 1, j);
        if (three) {
          t = t + r * H(k + 2, j);
          H(k + 2, j) = H(k + 2, j) - t * hz;
        }
        H(k + 1, j) = H(k + 1, j) - t * hy;
        H(k, j) = H(k, j) - t * hx;
      }
      g.sync();
      // columns k..k+2, rows l..min(hi, k+3): one row per lane
      const int last = hi < k + 3 ? hi : k + 3;
      for (int i = l + g.lane(); i <= last; i += G::W) {
        double t = hx * H(i, k) + hy * H(i, k + 1);
        if (three) {
          t = t + hz * H(i, k + 2);
          H(i, k + 2) = H(i, k + 2) - t * r;
        }
        H(i, k + 1) = H(i, k + 1) - t * q;
        H(i, k) = H(i, k) - t;
      }
      g.sync();
    }
  }
  *rho = best;
  return 0;
}

// max |eig| of the companion of one PAI.  H: n x n scratch; ort: n doubles.  info: 0 converged, 1 non-finite
// input (NaN returned, nothing iterated), 2 iteration cap (the largest modulus deflated so far returned)
template <class G>
__host__ __device__ inline int eig_core(const G& g, const double* PAI, int ld, int N, int p, const EigMat& H,
                                        double* ort, double* maxroot) {
  const int n = N * p;
  if (eig_screen(g, PAI, ld, N, n)) {
    *maxroot = __builtin_nan("");
    return 1;
  }
  eig_fill(g, H, PAI, ld, N, n);
  eig_hessenberg(g, H, n, ort);
  return eig_qr(g, H, n, maxroot);
}

// ---- the two builds
// where matrix m of a batch starts: PAI + (m % na) * sa + (m / na) * sb, leading dimension ld
struct EigSrc {
  const double* PAI;
  int ld, na;
  long long sa, sb;
};

// host twin: M matrices on at most 16 threads.  info may be null.
void eig_host(int M, int N, int p, const EigSrc& src, double* maxroot, int* info);
// device: PAI, maxroot, info (not null) and scratch (eig_plan(n, M).scratch bytes) on the device
hipError_t eig_launch(hipStream_t st, int M, int N, int p, const EigSrc& src, double* maxroot, int* info,
                      double* scratch);
// check_stationarity: the chains with acc[c] != 0 take PAI [nPAI], E [nE] and the status word back from the snapshot
hipError_t eig_launch_stat_select(hipStream_t st, int B, int nPAI, int nE, const int* acc, const double* sPAI,
                                  const double* sE, const int* sStatus, double* PAI, double* E, int* status);

}  // namespace ccmm

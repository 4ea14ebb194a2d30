// Pure host arithmetic of libccmm: no HIP call and no chain set (declarations in ccmm_host.h, ccmm_draw_trunc_normal
// in include/ccmm.h).  Built with the flags of the other host units: the host draw is pinned to fractions of an ulp.
#include <algorithm>
#include <cmath>

#include "ccmm_host.h"

using namespace ccmm;

// small dense host helpers (N <= 128): lower Cholesky and SPD inverse, column-major
void host_chol(std::vector<double>& A, int n) {
  for (int j = 0; j < n; ++j) {
    double s = A[j + j * n];
    for (int k = 0; k < j; ++k) s -= A[j + k * n] * A[j + k * n];
    if (!(s > 0)) throw ArgError("matrix not positive definite");
    const double d = std::sqrt(s);
    A[j + j * n] = d;
    for (int i = j + 1; i < n; ++i) {
      double v = A[i + j * n];
      for (int k = 0; k < j; ++k) v -= A[i + k * n] * A[j + k * n];
      A[i + j * n] = v / d;
    }
    for (int i = 0; i < j; ++i) A[i + j * n] = 0.0;
  }
}

std::vector<double> host_spd_inverse(const std::vector<double>& A, int n) {
  std::vector<double> L = A;
  host_chol(L, n);
  std::vector<double> inv(n * n, 0.0);
  for (int col = 0; col < n; ++col) {
    std::vector<double> x(n, 0.0);
    for (int i = 0; i < n; ++i) {  // L y = e_col
      double v = (i == col) ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) v -= L[i + k * n] * x[k];
      x[i] = v / L[i + i * n];
    }
    for (int i = n - 1; i >= 0; --i) {  // L' z = y
      double v = x[i];
      for (int k = i + 1; k < n; ++k) v -= L[k + i * n] * x[k];
      x[i] = v / L[i + i * n];
    }
    for (int i = 0; i < n; ++i) inv[i + col * n] = x[i];
  }
  return inv;
}

// Gauss-Legendre nodes/weights by Newton on P_n (host, once); negative half
GLNodes make_gl_nodes() {
  GLNodes g{};
  const int ns[3] = {6, 12, 20};
  for (int r = 0; r < 3; ++r) {
    const int n = ns[r];
    for (int i = 0; i < n / 2; ++i) {
      double x = -std::cos(M_PI * (i + 0.75) / (n + 0.5));
      double dp = 0.0;
      for (int it = 0; it < 100; ++it) {
        double p0 = 1.0, p1 = x;
        for (int k = 2; k <= n; ++k) {
          const double p2 = ((2.0 * k - 1.0) * x * p1 - (k - 1.0) * p0) / k;
          p0 = p1;
          p1 = p2;
        }
        dp = n * (x * p1 - p0) / (x * x - 1.0);
        const double dx = p1 / dp;
        x -= dx;
        if (std::fabs(dx) < 1e-17) break;
      }
      g.x[r][i] = x;
      g.w[r][i] = 2.0 / ((1.0 - x * x) * dp * dp);
    }
  }
  return g;
}

const GLNodes& gl_nodes() {
  static const GLNodes gl = make_gl_nodes();
  return gl;
}

// A = Psi(2:Ny+1, :) \ I: forward substitution when the impact matrix is lower triangular (every
// reference caller passes invA, mcmcVARshadowrateBlockHybrid.m:418); otherwise Gauss-Jordan with
// partial pivoting, and the ELB kernels take the full structural matrix (gibbsdrawShadowrates.m:49-58,
// 74-95 QR-factor M = Cpowerp Psi diag(SVol) for any Psi: the same conditionals)
bool host_struct_inverse(const double* Pc, int K, int Ny, bool lower, double* Ac) {
  if (lower) {
    for (int col = 0; col < Ny; ++col)
      for (int r = col; r < Ny; ++r) {
        double v = (r == col) ? 1.0 : 0.0;
        for (int q = col; q < r; ++q) v -= Pc[(1 + r) + (size_t)q * K] * Ac[q + (size_t)col * Ny];
        Ac[r + (size_t)col * Ny] = v / Pc[(1 + r) + (size_t)r * K];
      }
    return true;
  }
  std::vector<double> M((size_t)Ny * Ny), I((size_t)Ny * Ny, 0.0);
  for (int col = 0; col < Ny; ++col) {
    I[col + (size_t)col * Ny] = 1.0;
    for (int r = 0; r < Ny; ++r) M[r + (size_t)col * Ny] = Pc[(1 + r) + (size_t)col * K];
  }
  for (int col = 0; col < Ny; ++col) {
    int piv = col;
    for (int r = col + 1; r < Ny; ++r)
      if (std::fabs(M[r + (size_t)col * Ny]) > std::fabs(M[piv + (size_t)col * Ny])) piv = r;
    if (!(std::fabs(M[piv + (size_t)col * Ny]) > 0.0)) return false;
    if (piv != col)
      for (int q = 0; q < Ny; ++q) {
        std::swap(M[col + (size_t)q * Ny], M[piv + (size_t)q * Ny]);
        std::swap(I[col + (size_t)q * Ny], I[piv + (size_t)q * Ny]);
      }
    const double ip = 1.0 / M[col + (size_t)col * Ny];
    for (int q = 0; q < Ny; ++q) {
      M[col + (size_t)q * Ny] *= ip;
      I[col + (size_t)q * Ny] *= ip;
    }
    for (int r = 0; r < Ny; ++r) {
      if (r == col) continue;
      const double f = M[r + (size_t)col * Ny];
      if (f == 0.0) continue;
      for (int q = 0; q < Ny; ++q) {
        M[r + (size_t)q * Ny] -= f * M[col + (size_t)q * Ny];
        I[r + (size_t)q * Ny] -= f * I[col + (size_t)q * Ny];
      }
    }
  }
  std::copy(I.begin(), I.end(), Ac);
  return true;
}

// erfcinv on the host (Giles 2010 single-precision seed + Halley refinement)
double host_erfcinv(double y) {
  if (y <= 0.0) return INFINITY;
  if (y >= 2.0) return -INFINITY;
  // work with x = erfinv(1 - y) using the symmetric form for accuracy near 0
  const bool upper = y > 1.0;
  const double yy = upper ? 2.0 - y : y;  // yy in (0, 1]
  if (yy < 1e-30) {
    // deep tail: asymptotic seed erfc(x) ~ exp(-x^2)/(x sqrt(pi)), then Newton on log erfc
    const double ly = std::log(yy);
    double x = std::sqrt(-ly);
    for (int it = 0; it < 4; ++it) x = std::sqrt(-ly - std::log(1.7724538509055159 * x));
    for (int it = 0; it < 3; ++it) {
      const double e = std::erfc(x);
      const double f = std::log(e) - ly;
      const double df = -1.1283791670955126 * std::exp(-x * x) / e;
      x -= f / df;
    }
    return upper ? -x : x;
  }
  // seed: Giles' approximation of erfinv(1 - yy)
  double w = -std::log(yy * (2.0 - yy));
  double p;
  if (w < 6.25) {
    w -= 3.125;
    p = -3.6444120640178196996e-21;
    p = -1.685059138182016589e-19 + p * w;
    p = 1.2858480715256400167e-18 + p * w;
    p = 1.115787767802518096e-17 + p * w;
    p = -1.333171662854620906e-16 + p * w;
    p = 2.0972767875968561637e-17 + p * w;
    p = 6.6376381343583238325e-15 + p * w;
    p = -4.0545662729752068639e-14 + p * w;
    p = -8.1519341976054721522e-14 + p * w;
    p = 2.6335093153082322977e-12 + p * w;
    p = -1.2975133253453532498e-11 + p * w;
    p = -5.4154120542946279317e-11 + p * w;
    p = 1.051212273321532285e-09 + p * w;
    p = -4.1126339803469836976e-09 + p * w;
    p = -2.9070369957882005086e-08 + p * w;
    p = 4.2347877827932403518e-07 + p * w;
    p = -1.3654692000834678645e-06 + p * w;
    p = -1.3882523362786468719e-05 + p * w;
    p = 0.0001867342080340571352 + p * w;
    p = -0.00074070253416626697512 + p * w;
    p = -0.0060336708714301490533 + p * w;
    p = 0.24015818242558961693 + p * w;
    p = 1.6536545626831027356 + p * w;
  } else if (w < 16.0) {
    w = std::sqrt(w) - 3.25;
    p = 2.2137376921775787049e-09;
    p = 9.0756561938885390979e-08 + p * w;
    p = -2.7517406297064545428e-07 + p * w;
    p = 1.8239629214389227755e-08 + p * w;
    p = 1.5027403968909827627e-06 + p * w;
    p = -4.013867526981545969e-06 + p * w;
    p = 2.9234449089955446044e-06 + p * w;
    p = 1.2475304481671778723e-05 + p * w;
    p = -4.7318229009055733981e-05 + p * w;
    p = 6.8284851459573175448e-05 + p * w;
    p = 2.4031110387097893999e-05 + p * w;
    p = -0.0003550375203628474796 + p * w;
    p = 0.00095328937973738049703 + p * w;
    p = -0.0016882755560235047313 + p * w;
    p = 0.0024914420961078508066 + p * w;
    p = -0.0037512085075692412107 + p * w;
    p = 0.005370914553590063617 + p * w;
    p = 1.0052589676941592334 + p * w;
    p = 3.0838856104922207635 + p * w;
  } else {
    w = std::sqrt(w) - 5.0;
    p = -2.7109920616438573243e-11;
    p = -2.5556418169965252055e-10 + p * w;
    p = 1.5076572693500548083e-09 + p * w;
    p = -3.7894654401267369937e-09 + p * w;
    p = 7.6157012080783393804e-09 + p * w;
    p = -1.4960026627149240478e-08 + p * w;
    p = 2.9147953450901080826e-08 + p * w;
    p = -6.7711997758452339498e-08 + p * w;
    p = 2.2900482228026654717e-07 + p * w;
    p = -9.9298272942317002539e-07 + p * w;
    p = 4.5260625972231537039e-06 + p * w;
    p = -1.9681778105531670567e-05 + p * w;
    p = 7.5995277030017761139e-05 + p * w;
    p = -0.00021503011930044477347 + p * w;
    p = -0.00013871931833623122026 + p * w;
    p = 1.0103004648645343977 + p * w;
    p = 4.8499064014085844221 + p * w;
  }
  double x = p * (1.0 - yy);  // erfinv(1 - yy) >= 0
  // Halley refinement on erfc(x) = yy
  for (int it = 0; it < 3; ++it) {
    const double f = std::erfc(x) - yy;
    const double dfx = -1.1283791670955126 * std::exp(-x * x);  // d/dx erfc
    const double d2 = -2.0 * x * dfx;
    x -= f / (dfx - 0.5 * f * d2 / dfx);
  }
  return upper ? -x : x;
}

extern "C" double ccmm_draw_trunc_normal(double mu, double sig, double elb, double u, uint8_t* flags) {
  const double tol = 1e-10;
  const double eps = 2.220446049250313080847e-16;
  sig = std::fabs(sig);
  if (sig > tol) {
    const double ub = (elb - mu) / sig;
    const double PHIbar = 0.5 * std::erfc(-std::sqrt(0.5) * ub);
    double zz;
    if (PHIbar > eps) {
      zz = -std::sqrt(2.0) * host_erfcinv(2.0 * u * PHIbar);
      if (flags) *flags = 3;
    } else {
      zz = ub;
      if (flags) *flags = 1;
    }
    return mu + sig * zz;
  }
  if (flags) *flags = 0;
  return mu;
}

// Device functions shared by the predictive-density score kernels (k_fcst_scores of ccmm_fcst.hip, N <= 32, and
// k_fcst_scores_big of ccmm_fcst_big.hip, N <= 128): the normal cdf, Genz's bivariate and trivariate rules, the
// lattice mvncdf and the censored part of logscoreGaussianCensored.m on a trailing Cholesky block of at most
// kMvnMaxD x kMvnMaxD (leading dimension kFcstMaxN).  Every function that takes `lane` is called by all 64 lanes
// of one wave with identical arguments.
#pragma once
#include "ccmm_fcst.h"

namespace ccmm {

__device__ inline double ncdf(double x) { return 0.5 * erfc(-x * 0.70710678118654752440); }

// Genz (2004) BVNU: P(X > dh, Y > dk), correlation r (Drezner & Wesolowsky 1990 form)
__device__ inline double bvnu(double dh, double dk, double r, const GLNodes& gl) {
  int ng, lg;
  const double ar = fabs(r);
  if (ar < 0.3) { ng = 0; lg = 3; }
  else if (ar < 0.75) { ng = 1; lg = 6; }
  else { ng = 2; lg = 10; }
  double h = dh, k = dk, hk = h * k, bvn = 0.0;
  const double twopi = 6.283185307179586477;
  if (ar < 0.925) {
    const double hs = (h * h + k * k) * 0.5, asr = asin(r);
    for (int i = 0; i < lg; ++i) {
      double sn = sin(asr * (gl.x[ng][i] + 1.0) * 0.5);
      bvn += gl.w[ng][i] * exp((sn * hk - hs) / (1.0 - sn * sn));
      sn = sin(asr * (-gl.x[ng][i] + 1.0) * 0.5);
      bvn += gl.w[ng][i] * exp((sn * hk - hs) / (1.0 - sn * sn));
    }
    return fmax(0.0, fmin(1.0, bvn * asr / (2.0 * twopi) + ncdf(-h) * ncdf(-k)));
  }
  if (r < 0) { k = -k; hk = -hk; }
  if (ar < 1.0) {
    const double as = (1.0 - r) * (1.0 + r);
    double a = sqrt(as);
    const double bs = (h - k) * (h - k);
    const double c = (4.0 - hk) / 8.0, d = (12.0 - hk) / 16.0;
    bvn = a * exp(-(bs / as + hk) * 0.5) *
          (1.0 - c * (bs - as) * (1.0 - d * bs / 5.0) / 3.0 + c * d * as * as / 5.0);
    if (hk > -160.0) {
      const double b = sqrt(bs);
      bvn -= exp(-hk * 0.5) * sqrt(twopi) * ncdf(-b / a) * b * (1.0 - c * bs * (1.0 - d * bs / 5.0) / 3.0);
    }
    a *= 0.5;
    for (int i = 0; i < lg; ++i) {
      for (int sgn = -1; sgn <= 1; sgn += 2) {
        double xs = a * (sgn * gl.x[ng][i] + 1.0);
        xs *= xs;
        const double rs = sqrt(1.0 - xs);
        bvn += a * gl.w[ng][i] *
               (exp(-bs / (2.0 * xs) - hk / (1.0 + rs)) / rs - exp(-(bs / xs + hk) * 0.5) * (1.0 + c * xs * (1.0 + d * xs)));
      }
    }
    bvn = -bvn / twopi;
  }
  // the result clamped to [0, 1] as Genz's BVNU returns it (BVNU = MAX(0, MIN(1, BVN))) and
  // MATLAB's bivariate mvncdf with it: far in the tails the cancellation below can leave a
  // probability of order -1e-17, whose log would turn the draw's score (and the vintage's log
  // mean exp) into NaN
  if (r > 0) return fmax(0.0, fmin(1.0, bvn + ncdf(-fmax(h, k))));
  bvn = -bvn;
  if (k > h) bvn += ncdf(k) - ncdf(h);
  return fmax(0.0, fmin(1.0, bvn));
}

// A composite 20-point Gauss-Legendre rule on [brk[0], brk[nb-1]] split at the interior break points, every
// segment on panels graded geometrically towards both of its ends: panel j of a side spans
// [w0 (2^j - 1), min(w0 (2^(j+1) - 1), half)] from that end (half = half the segment).  Called by all 64 lanes of
// a wave with identical arguments: the (segment, side, panel, node) evaluations are spread over the lanes;
// returns this lane's part of sum f(z, weight) * (panel half-width), the caller adds the lanes up.
struct GradedRule {
  double brk[6];
  int nb;
  double w0;
};

template <class F>
__device__ double graded_gl20(const GradedRule& g, const GLNodes& gl, int lane, F f) {
  const double w0 = g.w0;
  const int nb = g.nb;
  // panels per side of each segment
  int npan[5];
  int total = 0;
  for (int sgm = 0; sgm + 1 < nb; ++sgm) {
    const double half = 0.5 * (g.brk[sgm + 1] - g.brk[sgm]);
    int n = 0;
    double pos = 0.0, w = fmin(w0, half);
    while (pos < half) {
      pos += fmin(w, half - pos);
      w *= 2.0;
      ++n;
    }
    npan[sgm] = n;
    total += 2 * n * 20;
  }
  double acc = 0.0;
  for (int q = lane; q < total; q += 64) {
    int rem = q, sgm = 0;
    while (rem >= 2 * npan[sgm] * 20) { rem -= 2 * npan[sgm] * 20; ++sgm; }
    const int side = rem / (npan[sgm] * 20);
    rem -= side * npan[sgm] * 20;
    const int j = rem / 20, node = rem - j * 20;
    const double a0 = g.brk[sgm], a1 = g.brk[sgm + 1];
    const double half = 0.5 * (a1 - a0);
    const double wj = fmin(w0, half) * exp2((double)j);
    const double u0 = (j == 0) ? 0.0 : fmin(w0, half) * (exp2((double)j) - 1.0);
    const double u1 = fmin(u0 + wj, half);
    const double c = 0.5 * (u0 + u1), r = 0.5 * (u1 - u0);
    const int i = node >> 1;
    const double sg = (node & 1) ? 1.0 : -1.0;
    const double u = c + sg * r * gl.x[2][i];
    const double z = side == 0 ? a0 + u : a1 - u;
    acc += f(z, gl.w[2][i]) * r;
  }
  return acc;
}

// P(X <= h, Y <= k) for standard normals with correlation r, to relative accuracy: the conditional integral
// int_lo^h phi(z) Phi((k - r z) / s) dz, s = sqrt(1 - r^2).  For the deep tails, where BVNU's absolute 1e-16
// (the accuracy Genz states, and MATLAB's mvncdf has) leaves the logarithm of the probability no digits or
// turns it into log(0).  The integrand is log-concave with its mode in [min(r k, 0), max(r k, 0)] (clipped
// at h) and curvature at least 1, so below lo = min(h, r k, 0) - 9 lies 1e-19 of it at most; it is split at
// r k (its peak, of width s, where Phi is small), at k / r (where the inner argument changes sign; panels down
// to a quarter of the transition's width s / |r|) and at 0.  Called by all 64 lanes with identical arguments.
__device__ inline double bvn_cond(double h, double k, double r, const GLNodes& gl, int lane) {
  if (r == 0.0) return ncdf(h) * ncdf(k);
  const double s = sqrt((1.0 - r) * (1.0 + r));
  if (!(s > 0.0)) return r > 0.0 ? ncdf(fmin(h, k)) : fmax(0.0, ncdf(h) - ncdf(-k));
  const double hi = fmin(h, 40.0);
  double cand[3] = {r * k, k / r, 0.0};
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j + 1 < 3 - i; ++j)
      if (cand[j] > cand[j + 1]) { const double t = cand[j]; cand[j] = cand[j + 1]; cand[j + 1] = t; }
  GradedRule g;
  g.w0 = fmax(fmin(1e-4, 0.25 * s / fabs(r)), 1e-12);
  g.nb = 0;
  g.brk[g.nb++] = fmin(fmin(hi, r * k), 0.0) - 9.0;
  for (int i = 0; i < 3; ++i)
    if (cand[i] > g.brk[g.nb - 1] + 1e-12 && cand[i] < hi - 1e-12) g.brk[g.nb++] = cand[i];
  g.brk[g.nb++] = hi;
  const double acc = graded_gl20(g, gl, lane, [&](double z, double w) {
    return w * exp(-0.5 * z * z) * ncdf((k - r * z) / s);
  });
  return fmax(0.0, fmin(1.0, wave_sum(acc) * 0.39894228040143267794));
}

// below this BVNU's absolute accuracy no longer gives the log score its 1e-9: bvn_cond takes over
constexpr double kBvnRelFloor = 1e-7;

// Trivariate normal P(X <= x), X ~ N(0, L L') with L lower 3x3 (ld kFcstMaxN at M):
// P = int_{lo}^{x1/L11} phi(z) BVN(h(z), k(z); rho) dz with the conditional
// bivariate of (X2, X3) | z (Genz BVN inside).  The integrand steps where h or k
// changes sign, so the outer interval is split there and each segment integrated
// on graded panels (graded_gl20, w0 = 1e-4).  The lower limit lo = min(-10, b - 5), b = x1 / L11, leaves
// out at most exp(-37.5) = 5e-17 of the Gaussian weight at b (Phi(-10) = 8e-24 for b >= -5), so that the
// logarithm keeps its digits for b far in the tail as well; b <= -38.6: Phi(b) is 0 in fp64.
// MATLAB's mvncdf (trivariate rule, absolute tolerance 1e-8) is the reference.
// Called by all 64 lanes of a wave with identical arguments.
__device__ inline double tvn_cdf(const double* x, const double* M, const GLNodes& gl, int lane) {
  const double l11 = M[0], l21 = M[1], l31 = M[2];
  const double l22 = M[1 + kFcstMaxN], l32 = M[2 + kFcstMaxN], l33 = M[2 + 2 * kFcstMaxN];
  const double s3 = sqrt(l32 * l32 + l33 * l33), rho = l32 / s3;
  const double b = x[0] / l11;
  if (b <= -38.6) return 0.0;
  const double lo = fmin(-10.0, b - 5.0);
  GradedRule g;
  g.w0 = 1e-4;
  g.nb = 0;
  g.brk[g.nb++] = lo;
  double cand[2] = {l21 != 0.0 ? x[1] / l21 : lo, l31 != 0.0 ? x[2] / l31 : lo};
  if (cand[0] > cand[1]) { const double t = cand[0]; cand[0] = cand[1]; cand[1] = t; }
  for (int i = 0; i < 2; ++i)
    if (cand[i] > g.brk[g.nb - 1] + 1e-12 && cand[i] < b - 1e-12) g.brk[g.nb++] = cand[i];
  g.brk[g.nb++] = b;
  const double acc = graded_gl20(g, gl, lane, [&](double z, double w) {
    const double h = (x[1] - l21 * z) / l22, k = (x[2] - l31 * z) / s3;
    return w * exp(-0.5 * z * z) * bvnu(-h, -k, rho, gl);
  });
  return fmax(0.0, fmin(1.0, wave_sum(acc) * 0.39894228040143267794));  // Genz TVNU: MAX(0, MIN(1, TVN))
}

// P(X <= x) for X ~ N(0, L L'), L lower d x d (ld kFcstMaxN), 4 <= d <= kMvnMaxD: MATLAB's mvncdf
// integrates four or more dimensions by randomised quasi-Monte Carlo (absolute error tolerance
// 1e-4), which no restatement can reproduce draw for draw.  This is a deterministic estimate
// inside that tolerance: Genz's separation of variables (e_1 = Phi(x_1 / L_11), then
// y_{i-1} = Phi^-1(w_{i-1} e_{i-1}), e_i = Phi((x_i - sum_j L_ij y_j) / L_ii), integrand
// e_1 ... e_d) on a fixed rank-1 lattice of kMvnPts points (generators frac(sqrt(prime_i)),
// tent-periodised) spread over the lanes, summed by one wave reduction.  Typical error ~1e-7 at 65536 points
// (tests: against an independent randomised lattice rule at 1e-6, and bit-level against the
// oracle's restatement of this rule, oracle/ccmm_oracle_fcst.mvn_lattice_cdf).
// (the generators and kMvnPts are written out in ccmm_fcst.hip, which holds them equal to kMvnAlpha and the
// header's kMvnPts at compile time: tests/test_oracle_fcst.py reads them there)
constexpr double kMvnAlpha[kMvnMaxD - 1] = {1.4142135623730951, 1.7320508075688772, 2.2360679774997898,
                                            2.6457513110645907, 3.3166247903554, 3.605551275463989,
                                            4.123105625617661, 4.358898943540674, 4.795831523312719,
                                            5.385164807134504, 5.5677643628300215};
__device__ inline double mvn_lattice_cdf(const double* x, const double* M, int d, int lane) {
  const double alpha[kMvnMaxD - 1] = {kMvnAlpha[0], kMvnAlpha[1], kMvnAlpha[2], kMvnAlpha[3], kMvnAlpha[4], kMvnAlpha[5],
                                      kMvnAlpha[6], kMvnAlpha[7], kMvnAlpha[8], kMvnAlpha[9], kMvnAlpha[10]};
  const double e1 = ncdf(x[0] / M[0]);
  if (!(e1 > 0.0)) return 0.0;
  double acc = 0.0;
  for (int q = lane; q < kMvnPts; q += 64) {
    double yv[kMvnMaxD];
    double e = e1, f = e1;
    for (int i = 1; i < d && f > 0.0; ++i) {
      double w = (double)(q + 1) * alpha[i - 1];
      w -= floor(w);
      w = fabs(2.0 * w - 1.0);
      const double pw = fmin(fmax(w * e, 1e-300), 1.0 - 1e-16);
      yv[i - 1] = normcdfinv(pw);
      double sdot = 0.0;
      for (int j = 0; j < i; ++j) sdot = fma(M[i + j * kFcstMaxN], yv[j], sdot);
      e = ncdf((x[i] - sdot) / M[i + i * kFcstMaxN]);
      f *= e;
    }
    acc += f;
  }
  return fmax(0.0, fmin(1.0, wave_sum(acc) / (double)kMvnPts));
}

// The censored part of logscoreGaussianCensored.m:57-88: log P(X <= yat - y21) for X ~ N(0, L L'), L the trailing
// nat x nat block of the Cholesky factor (lower, ld kFcstMaxN at Mt), 1 <= nat <= kMvnMaxD: the univariate cdf,
// Genz's bivariate rule (bvn_cond in the deep tail), the trivariate rule, the lattice estimate from four series on
__device__ inline double censored_llf2(int nat, const double* yat, const double* y21, const double* Mt,
                                       const GLNodes& gl, int lane) {
  const double l11 = Mt[0];
  if (nat == 1) return log(ncdf((yat[0] - y21[0]) / l11));
  if (nat == 2) {
    // Sigma22 = L22 L22': sd1 = l11, cov = l11 l21, var2 = l21^2 + l22^2
    const double l21 = Mt[1];
    const double l22 = Mt[1 + kFcstMaxN];
    const double s2 = sqrt(l21 * l21 + l22 * l22);
    const double rho = l21 / s2;
    const double h = (yat[0] - y21[0]) / l11, k = (yat[1] - y21[1]) / s2;
    double P = bvnu(-h, -k, rho, gl);
    if (P < kBvnRelFloor) P = bvn_cond(h, k, rho, gl, lane);
    return log(P);
  }
  if (nat == 3) {
    const double xv[3] = {yat[0] - y21[0], yat[1] - y21[1], yat[2] - y21[2]};
    return log(tvn_cdf(xv, Mt, gl, lane));
  }
  double xv[kMvnMaxD];
  for (int a = 0; a < nat; ++a) xv[a] = yat[a] - y21[a];
  return log(mvn_lattice_cdf(xv, Mt, nat, lane));
}

}  // namespace ccmm

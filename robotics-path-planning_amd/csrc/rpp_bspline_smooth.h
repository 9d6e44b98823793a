// rpp_bspline_smooth.h -- the smoothing fit of approximate_b_spline_path, host + device source like rpp_bspline.h.
// Reference: 10_path_planning_00_bspline_path.py  approximate_b_spline_path :12-56 -- UnivariateSpline(distances, x, k=degree,
//            s=s) and the same for y, then _evaluate_spline :99-108.
//
// UnivariateSpline is Dierckx's fpcurf with unit weights, reached twice: first with the storage limit nest = max(m / 2,
// 2 (k + 1)) (integer division), and, when the knot loop stops at n == nest with fp - s >= acc, once more with nest = m + k + 1
// from the knots, interval sums and counts it had, nplus set back to 1.  One function here does both: at n == nest it raises
// the limit and goes on.  tol = 0.001, acc = tol * s, maxit = 20, nmin = 2 (k + 1), nmax = m + k + 1.
//
// Restated exactly (the knot vector equals FITPACK's): which data sites become knots.  Per round: the least-squares spline on
// the current knots; stop when |fp - s| < acc or fp < s; at n == nmax the knots become bspline_knots and the loop runs once
// more; else nplus = 1 on the first round, later npl1 = 2 nplus, and if fpold - fp > acc npl1 = (int)(nplus * (fp - s) /
// (fpold - fp)) (a quotient of 2^31 or more converts to INT_MIN, as cvttsd2si does), nplus = min(2 nplus, max(npl1, nplus / 2,
// 1)); the interval sums fpint from one walk over the data (a data point at t[l] closes an interval: half its term each side);
// then nplus times, without new residuals: the first interval of the strictly largest fpint among those with nrdata > 0 gets
// the data site u[maxbeg + maxpt / 2] (maxbeg = sum of nrdata[j] + 1 before it, plus one) as a knot, counts maxpt / 2 and
// maxpt - maxpt / 2 - 1, and fpint split as fpmax * count / maxpt; stop adding at n == nmax or n == nest.  Where no interval
// qualifies (every interval that still holds data has a zero fpint) FITPACK's fpknot reads variables it never set; here the
// round adds no further knot, and a round that adds none ends the fit with the least-squares spline on the current knots and
// ier = 1.
//
// This file's own arithmetic (scipy's FITPACK is not one arithmetic), in this order:
//   givens(piv, ww)   store = |piv|; store >= ww: r = ww / piv, dd = store * sqrt(1.0 + r * r); else r = piv / ww,
//                     dd = ww * sqrt(1.0 + r * r);  cos = ww / dd, sin = piv / dd, ww = dd
//   rota(a, b)        a' = cos * a - sin * b,  b' = cos * b + sin * a
//   least squares     data rows in order, the k + 1 values of bspline_values; for i = 0 .. k with h[i] != 0.0: givens(h[i],
//                     A[j][0]), rota(yi, z[j]), rota(h[i1], A[j][i1 - i]) for i1 = i+1 .. k;  fp = fp + yi * yi after the row
//   back-substitution c[n-1] = z[n-1] / A[n-1][0]; i = n-2 .. 0: store = z[i]; store = store - c[i+l] * A[i][l], l = 1 ..
//                     min(width - 1, n-1-i); c[i] = store / A[i][0]
//   residual          term = 0.0; term = term + c[l0+j] * q[it][j], j = 0 .. k; d = term - y[it]; d * d
//   jumps             fac = nrint / (t[n-k-1] - t[k]); per interior knot t[l]: h[j] = t[l] - t[l+j-k-1], h[j+k+1] = t[l] -
//                     t[l+j+1]; prod = h[j]; prod = prod * h[j+i] * fac, i = 1 .. k; b[row][j] = (t[lp+k+1] - t[lp]) / prod
//   smoothing step    pinv = 1.0 / p; row `it` of b times pinv rotated into a copy G (k + 2 wide) of the band, rows it ..
//                     n-k-2, shifting h left after each; back-substitution of width k + 2; fp from the residuals
//   root search       p = (n-k-1) / sum A[i][0]; bracket (0, fp0 - s), (inf, fp_inf - s); FITPACK's logic with con1 = 0.1,
//                     con9 = 0.9, con4 = 0.04, ich1, ich3 and the rational step fprati; ier 2 on non-monotone values, 3 after
//                     maxit.  In the "p too small" branch the test is Dierckx's `p >= p3`.
// tests/bspline_smooth_oracle.py states the same in Python; the two are bit-identical.  No FMA contraction may be applied.
//
// Workspace of one fit: kSmoothPlanes planes of m entries each, plane P's entry i at w[P * stride + i] -- 0 z, 1 fpint,
// 2 nrdata (int32), 3 .. 8 q, 9 .. 14 A, 15 .. 21 G, 22 .. 28 b --; t holds m + k + 1 knots, c m coefficients.
#pragma once
#include "rpp_bspline.h"

namespace rpp {

constexpr int kBsplineSingular = 3;   // RRTX_BSPLINE_SINGULAR: a coefficient of the smoothing fit is not finite
constexpr int kSmoothPlanes = 29;
constexpr int kSmoothMaxit = 20;

struct SmoothInfo {   // rrtx_bspline_axis_record
  int32_t n_knots, ier;   // ier: 0, -1 the interpolating spline, -2 the least-squares polynomial, 2, 3 as FITPACK's, 1 no knot could be added
  double fp, p;           // the sum of squared residuals; the smoothing parameter (+inf without a root search)
  int32_t rounds, iters;  // knot rounds (least-squares fits) and root-search steps
};

#define RPP_SM_Z(i) w[(i)]
#define RPP_SM_FPINT(i) w[stride + (i)]
#define RPP_SM_NRDATA(i) ((int32_t*)(w + 2 * stride))[(i)]
#define RPP_SM_Q(i, j) w[(int64_t)(3 + (j)) * stride + (i)]
#define RPP_SM_A(i, j) w[(int64_t)(9 + (j)) * stride + (i)]
#define RPP_SM_G(i, j) w[(int64_t)(15 + (j)) * stride + (i)]
#define RPP_SM_B(i, j) w[(int64_t)(22 + (j)) * stride + (i)]

RPP_HD static inline void smooth_givens(double piv, double& ww, double& cs, double& sn) {
  const double store = fabs(piv);
  double dd;
  if (store >= ww) {
    const double r = ww / piv;
    dd = store * sqrt(1.0 + r * r);
  } else {
    const double r = piv / ww;
    dd = ww * sqrt(1.0 + r * r);
  }
  cs = ww / dd;
  sn = piv / dd;
  ww = dd;
}

RPP_HD static inline void smooth_rota(double cs, double sn, double& a, double& b) {
  const double s1 = a, s2 = b;
  b = cs * s2 + sn * s1;
  a = cs * s1 - sn * s2;
}

// c from the band (A, width k + 1) with the right-hand side z, or from (G, width k + 2) with c itself
template <bool WIDE>
RPP_HD static inline void smooth_back(double* w, int64_t stride, int n, int width, double* c) {
#define RPP_SM_M(i, j) (WIDE ? RPP_SM_G(i, j) : RPP_SM_A(i, j))
#define RPP_SM_R(i) (WIDE ? c[(i)] : RPP_SM_Z(i))
  c[n - 1] = RPP_SM_R(n - 1) / RPP_SM_M(n - 1, 0);
  for (int i = n - 2; i >= 0; i--) {
    double store = RPP_SM_R(i);
    const int i1 = width - 1 < n - 1 - i ? width - 1 : n - 1 - i;
    for (int l = 1; l <= i1; l++) store = store - c[i + l] * RPP_SM_M(i, l);
    c[i] = store / RPP_SM_M(i, 0);
  }
#undef RPP_SM_M
#undef RPP_SM_R
}

RPP_HD static inline double smooth_least_squares(const double* u, const double* y, int m, const double* t, int n, int k, double* w,
                                                 int64_t stride, double* c) {
  const int k1 = k + 1, nk1 = n - k - 1;
  for (int i = 0; i < nk1; i++) {
    RPP_SM_Z(i) = 0.0;
    for (int j = 0; j < k1; j++) RPP_SM_A(i, j) = 0.0;
  }
  double fp = 0.0;
  int l = k;
  for (int it = 0; it < m; it++) {
    const double xi = u[it];
    double yi = y[it];
    while (!(xi < t[l + 1] || l == nk1 - 1)) l++;
    double h[kBsplineMaxDegree + 1];
    bspline_values(t, l, k, xi, h);
    for (int i = 0; i < k1; i++) RPP_SM_Q(it, i) = h[i];
    int j = l - k;
    for (int i = 0; i < k1; i++, j++) {
      const double piv = h[i];
      if (piv == 0.0) continue;
      double cs, sn;
      smooth_givens(piv, RPP_SM_A(j, 0), cs, sn);
      smooth_rota(cs, sn, yi, RPP_SM_Z(j));
      if (i == k) break;
      int i2 = 0;
      for (int i1 = i + 1; i1 < k1; i1++) {
        i2++;
        smooth_rota(cs, sn, h[i1], RPP_SM_A(j, i2));
      }
    }
    fp = fp + yi * yi;
  }
  smooth_back<false>(w, stride, nk1, k1, c);
  return fp;
}

// The squared residual of data point `it`; lz is the knot cursor of the walk, *crossed whether the point closed an interval
RPP_HD static inline double smooth_residual(const double* u, const double* y, const double* t, int n, int k, const double* w,
                                            int64_t stride, const double* c, int it, int& lz, bool* crossed) {
  const int nk1 = n - k - 1;
  *crossed = false;
  if (!(u[it] < t[lz] || lz > nk1 - 1)) {
    *crossed = true;
    lz++;
  }
  const int l0 = lz - k - 1;
  double term = 0.0;
  for (int j = 0; j <= k; j++) term = term + c[l0 + j] * RPP_SM_Q(it, j);
  const double d = term - y[it];
  return d * d;
}

// fpknot; returns the new n (n itself when no interval qualifies)
RPP_HD static inline int smooth_add_knot(const double* u, double* t, int n, int k, double* w, int64_t stride, int nrint) {
  double fpmax = 0.0;
  int jbegin = 1, number = -1, maxpt = 0, maxbeg = 0;
  for (int j = 0; j < nrint; j++) {
    const int jpoint = RPP_SM_NRDATA(j);
    if (!(fpmax >= RPP_SM_FPINT(j) || jpoint == 0)) {
      fpmax = RPP_SM_FPINT(j);
      number = j;
      maxpt = jpoint;
      maxbeg = jbegin;
    }
    jbegin += jpoint + 1;
  }
  if (number < 0) return n;
  const int ihalf = maxpt / 2 + 1, nrx = maxbeg + ihalf, nxt = number + 1;
  for (int jj = nrint - 1; jj >= nxt; jj--) {
    RPP_SM_FPINT(jj + 1) = RPP_SM_FPINT(jj);
    RPP_SM_NRDATA(jj + 1) = RPP_SM_NRDATA(jj);
    t[jj + k + 1] = t[jj + k];
  }
  RPP_SM_NRDATA(number) = ihalf - 1;
  RPP_SM_NRDATA(nxt) = maxpt - ihalf;
  const double am = (double)maxpt;
  RPP_SM_FPINT(number) = fpmax * (double)(ihalf - 1) / am;
  RPP_SM_FPINT(nxt) = fpmax * (double)(maxpt - ihalf) / am;
  t[nxt + k] = u[nrx - 1];
  return n + 1;
}

RPP_HD static inline void smooth_jumps(const double* t, int n, int k, double* w, int64_t stride) {
  const int k1 = k + 1, k2 = k + 2, nk1 = n - k - 1;
  const double fac = (double)(nk1 - k) / (t[nk1] - t[k]);
  double h[2 * (kBsplineMaxDegree + 1)];
  for (int l = k1; l < nk1; l++) {
    const int row = l - k1;
    for (int j = 0; j < k1; j++) {
      h[j] = t[l] - t[l + j - k1];
      h[j + k1] = t[l] - t[l + j + 1];
    }
    int lp = row;
    for (int j = 0; j < k2; j++, lp++) {
      double prod = h[j];
      for (int i = 1; i <= k; i++) prod = prod * h[j + i] * fac;
      RPP_SM_B(row, j) = (t[lp + k1] - t[lp]) / prod;
    }
  }
}

RPP_HD static inline double smooth_rational(double& p1, double& f1, double p2, double f2, double& p3, double& f3) {
  double p;
  if (p3 > 0.0) {
    const double h1 = f1 * (f2 - f3), h2 = f2 * (f3 - f1), h3 = f3 * (f1 - f2);
    p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3);
  } else {
    p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3);
  }
  if (f2 < 0.0) {
    p3 = p2;
    f3 = f2;
  } else {
    p1 = p2;
    f1 = f2;
  }
  return p;
}

// The coefficients c of the smoothing spline with parameter p on the knots t, and its fp
RPP_HD static inline double smooth_step(const double* u, const double* y, int m, const double* t, int n, int k, double* w,
                                        int64_t stride, double p, double* c) {
  const int k1 = k + 1, k2 = k + 2, nk1 = n - k - 1, n8 = n - 2 * k1;
  const double pinv = 1.0 / p;
  for (int i = 0; i < nk1; i++) {
    c[i] = RPP_SM_Z(i);
    RPP_SM_G(i, k1) = 0.0;
    for (int j = 0; j < k1; j++) RPP_SM_G(i, j) = RPP_SM_A(i, j);
  }
  double h[kBsplineMaxDegree + 3];
  for (int it = 0; it < n8; it++) {
    for (int i = 0; i < k2; i++) h[i] = RPP_SM_B(it, i) * pinv;
    double yi = 0.0;
    for (int j = it; j < nk1; j++) {
      const double piv = h[0];
      double cs, sn;
      smooth_givens(piv, RPP_SM_G(j, 0), cs, sn);
      smooth_rota(cs, sn, yi, c[j]);
      if (j == nk1 - 1) break;
      int i2 = k1;
      if (j + 1 > n8) i2 = nk1 - j - 1;
      for (int i = 0; i < i2; i++) {
        smooth_rota(cs, sn, h[i + 1], RPP_SM_G(j, i + 1));
        h[i] = h[i + 1];
      }
      h[i2] = 0.0;
    }
  }
  smooth_back<true>(w, stride, nk1, k2, c);
  double fp = 0.0;
  int lz = k1;
  bool crossed;
  for (int it = 0; it < m; it++) fp = fp + smooth_residual(u, y, t, n, k, w, stride, c, it, lz, &crossed);
  return fp;
}

// One axis: the m values y over the strictly increasing u, degree k (m > k), s > 0.  Writes info->n_knots knots into t and
// n_knots - k - 1 coefficients into c.
RPP_HD static inline void bspline_smooth_fit(const double* u, const double* y, int m, int k, double s, double* w, int64_t stride,
                                             double* t, double* c, SmoothInfo* info) {
  const int k1 = k + 1, nmin = 2 * k1, nmax = m + k1;
  int nest = m / 2 > nmin ? m / 2 : nmin;
  const double acc = 0.001 * s;
  int n = nmin, nplus = 0, ier = 0, rounds = 0;
  double fpold = 0.0, fp0 = 0.0, fp = 0.0, fpms = 0.0;
  RPP_SM_NRDATA(0) = m - 2;
  bool done = false;
  for (int round = 0; round < 2 * m + 8; round++) {
    if (n == nmin) ier = -2;
    int nrint = n - nmin + 1;
    for (int j = 0; j < k1; j++) {
      t[j] = u[0];
      t[n - 1 - j] = u[m - 1];
    }
    fp = smooth_least_squares(u, y, m, t, n, k, w, stride, c);
    rounds++;
    if (ier == -2) fp0 = fp;
    fpms = fp - s;
    if (fabs(fpms) < acc) {
      done = true;
      break;
    }
    if (fpms < 0.0) break;
    if (n == nmax) {
      ier = -1;
      done = true;
      break;
    }
    if (n == nest) {   // the first pass returns ier = 1 here; the second goes on with the full storage
      nest = nmax;
      ier = 1;
    }
    if (ier != 0) {
      nplus = 1;
      ier = 0;
    } else {
      int npl1 = nplus * 2;
      if (fpold - fp > acc) {
        const double v = (double)nplus * fpms / (fpold - fp);
        npl1 = v < 2147483648.0 ? (int)v : INT32_MIN;
      }
      int mx = npl1 > nplus / 2 ? npl1 : nplus / 2;
      if (mx < 1) mx = 1;
      nplus = nplus * 2 < mx ? nplus * 2 : mx;
    }
    fpold = fp;
    {   // the interval sums
      double fpart = 0.0;
      int i = 0, lz = k1;
      bool crossed;
      for (int it = 0; it < m; it++) {
        const double term = smooth_residual(u, y, t, n, k, w, stride, c, it, lz, &crossed);
        fpart = fpart + term;
        if (crossed) {
          const double store = term * 0.5;
          RPP_SM_FPINT(i) = fpart - store;
          i++;
          fpart = store;
        }
      }
      RPP_SM_FPINT(nrint - 1) = fpart;
    }
    for (int l = 0; l < nplus; l++) {
      const int n2 = smooth_add_knot(u, t, n, k, w, stride, nrint);
      if (n2 == n) {   // FITPACK's fpknot is undefined here; this definition: no further knot in this round, and a round that
        if (l == 0) {  // adds none ends the fit on the current knots
          ier = 1;
          done = true;
        }
        break;
      }
      n = n2;
      nrint++;
      if (n == nmax) {
        bspline_knots(u, m, k, t);
        break;
      }
      if (n == nest) break;
    }
    if (done) break;
  }
  const int nk1 = n - k1;
  info->n_knots = n;
  info->rounds = rounds;
  info->iters = 0;
  info->p = HUGE_VAL;
  if (done || ier == -2) {
    info->ier = ier;
    info->fp = fp;
    return;
  }
  smooth_jumps(t, n, k, w, stride);
  double p1 = 0.0, f1 = fp0 - s, p3 = -1.0, f3 = fpms, p = 0.0;
  for (int i = 0; i < nk1; i++) p = p + RPP_SM_A(i, 0);
  p = (double)nk1 / p;
  int ich1 = 0, ich3 = 0, iters = 0;
  ier = 0;
  for (int it = 1; it <= kSmoothMaxit; it++) {
    fp = smooth_step(u, y, m, t, n, k, w, stride, p, c);
    iters = it;
    fpms = fp - s;
    if (fabs(fpms) < acc) break;
    if (it == kSmoothMaxit) {
      ier = 3;
      break;
    }
    const double p2 = p, f2 = fpms;
    if (ich3 == 0) {
      if (!(f2 - f3 > acc)) {   // the initial choice of p is too large
        p3 = p2;
        f3 = f2;
        p = p * 0.04;
        if (p <= p1) p = p1 * 0.9 + p2 * 0.1;
        continue;
      }
      if (f2 < 0.0) ich3 = 1;
    }
    if (ich1 == 0) {
      if (!(f1 - f2 > acc)) {   // the initial choice of p is too small
        p1 = p2;
        f1 = f2;
        p = p / 0.04;
        if (p3 < 0.0) continue;
        if (p >= p3) p = p2 * 0.1 + p3 * 0.9;
        continue;
      }
      if (f2 > 0.0) ich1 = 1;
    }
    if (f2 >= f1 || f2 <= f3) {
      ier = 2;
      break;
    }
    p = smooth_rational(p1, f1, p2, f2, p3, f3);
  }
  info->ier = ier;
  info->fp = fp;
  info->p = p;
  info->iters = iters;
}

#undef RPP_SM_Z
#undef RPP_SM_FPINT
#undef RPP_SM_NRDATA
#undef RPP_SM_Q
#undef RPP_SM_A
#undef RPP_SM_G
#undef RPP_SM_B

// q = {v, dv, ddv} of one axis: the spline (t, c) of n knots at x
template <int K>
RPP_HD static inline void bspline_axis_eval_k(const double* t, int n, const double* c, double x, double* q) {
  const int mu = bspline_span(t, n - K - 1, K, x);
  double wt[3][K + 1];
  bspline_weights<K, true>(t, mu, x, wt[0], wt[1], wt[2]);
  double pc[K + 1];
#pragma unroll
  for (int r = 0; r <= K; r++) pc[r] = c[mu - K + r];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    double a = pc[0] * wt[d][0];
#pragma unroll
    for (int r = 1; r <= K; r++) a = a + pc[r] * wt[d][r];
    q[d] = a;
  }
}

RPP_HD static inline void bspline_axis_eval(const double* t, int n, const double* c, int k, double x, double* q) {
  switch (k) {
    case 1: bspline_axis_eval_k<1>(t, n, c, x, q); break;
    case 2: bspline_axis_eval_k<2>(t, n, c, x, q); break;
    case 3: bspline_axis_eval_k<3>(t, n, c, x, q); break;
    case 4: bspline_axis_eval_k<4>(t, n, c, x, q); break;
    default: bspline_axis_eval_k<5>(t, n, c, x, q); break;
  }
}

// The point of a course whose axes have knot vectors of their own: out = {x, y, heading, curvature} as bspline_eval
RPP_HD static inline void bspline_smooth_eval(const double* tx, int nx, const double* cx, const double* ty, int ny, const double* cy,
                                              int k, double v, double* out) {
  double qx[3], qy[3];
  bspline_axis_eval(tx, nx, cx, k, v, qx);
  bspline_axis_eval(ty, ny, cy, k, v, qy);
  const double q[6] = {qx[0], qy[0], qx[1], qy[1], qx[2], qy[2]};
  bspline_point(q, out);
}

}  // namespace rpp

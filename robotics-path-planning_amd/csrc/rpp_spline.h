// rpp_spline.h -- natural cubic spline course through waypoints, host + device source like rpp_lqr.h.
// Reference: 10_path_planning_00_cubic_spline_path.py
//   CubicSpline1D.__init__ :48-73 (b and d :69-71), calc_position :93-94, calc_first_derivative :117,
//   calc_second_derivative :139, __search_index :146, __calc_B :171-172,
//   CubicSpline2D.__calc_s :240-246, calc_curvature :289, calc_yaw :309, calc_spline_course :313-325.
//
// Arithmetic: every double outside the solve of `c` is the reference's on glibc 2.35 + numpy: np.hypot = rpp_glibc_hypot,
// np.cumsum = a left-to-right sum, `** 2.0`, `** 3.0`, `** 2` and `** (3 / 2)` on numpy doubles = libm pow
// (rpp_glibc_pow), math.atan2 = rpp_glibc_atan2, and every product and sum rounded where the reference's expression
// rounds it (no FMA contraction may be applied to this file).
//
// The solve.  The reference takes c from np.linalg.solve(A, B): LAPACK's pivoted LU as OpenBLAS runs it on the host's
// CPU, which is not one arithmetic.  A caller that wants the reference's c hands it in; otherwise c is
// this file's Thomas recurrence over the interior rows i = 1 .. n-2 (diagonally dominant, no pivoting), in this order:
//   h[i]   = s[i+1] - s[i]
//   B[i]   = 3.0 * (a[i+1] - a[i]) / h[i] - 3.0 * (a[i] - a[i-1]) / h[i-1]
//   diag   = 2.0 * (h[i-1] + h[i]), sub = h[i-1], sup = h[i]
//   row 1:  den = diag,                 cp[1] = sup / den, dp[1] = B[1] / den
//   row i:  den = diag - sub * cp[i-1], cp[i] = sup / den, dp[i] = (B[i] - sub * dp[i-1]) / den
//   c[n-1] = 0.0, c[n-2] = dp[n-2], c[i] = dp[i] - cp[i] * c[i+1] for i = n-3 .. 1, c[0] = 0.0
// tests/spline_oracle.py states the same in Python; the two are bit-identical.
#pragma once
#include "rpp_core.h"

namespace rpp {

constexpr int kSplineOk = 0;           // RRTX_SPLINE_OK
constexpr int kSplineDegenerate = 1;   // RRTX_SPLINE_DEGENERATE: some h[i] == 0 (the reference divides by zero)
constexpr int kSplineRefRaises = 2;    // RRTX_SPLINE_REF_RAISES: the last sample parameter rounds onto s[-1] (IndexError)

// x ** y of a numpy double x >= 0 and y > 0: libm pow; pow(+0, y) = +0
RPP_HD static inline double spline_pow(double x, double y) {
  if (x == 0.0) return 0.0;
  return rpp_glibc_pow(x, y);
}

// s = [0] + np.cumsum(np.hypot(np.diff(x), np.diff(y))) of n >= 1 waypoints (CubicSpline2D.__calc_s; Spline2D.__calc_s of
// 10_path_planning_00_spline_2d.py :19-23 is the same statement, and rpp_bspline.h takes it from here)
RPP_HD static inline void spline_chord_sum(const double* x, const double* y, int n, double* s) {
  double acc = 0.0;
  s[0] = 0.0;
  for (int i = 0; i + 1 < n; i++) {
    acc = acc + rpp_glibc_hypot(x[i + 1] - x[i], y[i + 1] - y[i]);
    s[i + 1] = acc;
  }
}

// len(np.arange(0, s_end, ds)) for s_end > 0, ds > 0: ceil(s_end / ds) of the rounded quotient
RPP_HD static inline int64_t arange_count(double s_end, double ds) {
  const double q = s_end / ds;
  int64_t k = (int64_t)q;
  if ((double)k < q) k++;
  return k;
}

// One axis `a` (x or y) of one course of n >= 2 waypoints: the knots s (CubicSpline2D.__calc_s), then c -- copied from
// c_in when given, else the Thomas recurrence above -- then b and d (:69-71).  s, b, c, d hold n doubles each; b[n-1]
// and d[n-1] are zeroed (the reference's lists have n - 1 entries).  The forward sweep keeps cp in d and dp in c.
// Returns kSplineOk or kSplineDegenerate (nothing but s is valid then).
RPP_HD static inline int spline_fit_axis(const double* x, const double* y, const double* a, int n, const double* c_in,
                                         double* s, double* b, double* c, double* d) {
  spline_chord_sum(x, y, n, s);
  for (int i = 0; i + 1 < n; i++)
    if (s[i + 1] - s[i] == 0.0) return kSplineDegenerate;
  if (c_in) {
    for (int i = 0; i < n; i++) c[i] = c_in[i];
  } else {
    c[0] = 0.0;
    c[n - 1] = 0.0;
    for (int i = 1; i + 1 < n; i++) {
      const double h0 = s[i] - s[i - 1], h1 = s[i + 1] - s[i];
      const double B = 3.0 * (a[i + 1] - a[i]) / h1 - 3.0 * (a[i] - a[i - 1]) / h0;
      const double diag = 2.0 * (h0 + h1);
      double den, dp;
      if (i == 1) {
        den = diag;
        dp = B / den;
      } else {
        den = diag - h0 * d[i - 1];
        dp = (B - h0 * c[i - 1]) / den;
      }
      d[i] = h1 / den;
      c[i] = dp;
    }
    for (int i = n - 3; i >= 1; i--) c[i] = c[i] - d[i] * c[i + 1];
  }
  for (int i = 0; i + 1 < n; i++) {
    const double h = s[i + 1] - s[i];
    d[i] = (c[i + 1] - c[i]) / (3.0 * h);
    b[i] = 1.0 / h * (a[i + 1] - a[i]) - h / 3.0 * (2.0 * c[i] + c[i + 1]);
  }
  b[n - 1] = 0.0;
  d[n - 1] = 0.0;
  return kSplineOk;
}

// arange_count, with the reference's failure: sample k is
// 0 + k * ds (numpy fills start + i * delta with delta = (0 + ds) - 0).  *status becomes kSplineRefRaises, and the
// count 0, when the last sample is not below s_end: bisect then lands on the last knot and the reference's b[i] raises.
RPP_HD static inline int64_t spline_count(double s_end, double ds, int* status) {
  const int64_t k = arange_count(s_end, ds);
  if (k > 0 && (double)(k - 1) * ds >= s_end) {
    *status = kSplineRefRaises;
    return 0;
  }
  return k;
}

// The course's point at parameter t (0 <= t < s[n-1]): out = {x, y, yaw, curvature}
RPP_HD static inline void spline_eval(const double* s, const double* ax, const double* bx, const double* cx,
                                      const double* dx, const double* ay, const double* by, const double* cy,
                                      const double* dy, int n, double t, double* out) {
  // bisect.bisect(s, t) - 1 (:146)
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (t < s[mid])
      hi = mid;
    else
      lo = mid + 1;
  }
  const int i = lo - 1;
  const double u = t - s[i];
  const double u2 = spline_pow(u, 2.0), u3 = spline_pow(u, 3.0);
  out[0] = ax[i] + bx[i] * u + cx[i] * u2 + dx[i] * u3;                  // :93-94
  out[1] = ay[i] + by[i] * u + cy[i] * u2 + dy[i] * u3;
  const double x1 = bx[i] + 2.0 * cx[i] * u + 3.0 * dx[i] * u2;          // :117
  const double y1 = by[i] + 2.0 * cy[i] * u + 3.0 * dy[i] * u2;
  const double x2 = 2.0 * cx[i] + 6.0 * dx[i] * u;                       // :139
  const double y2 = 2.0 * cy[i] + 6.0 * dy[i] * u;
  out[2] = rpp_glibc_atan2(y1, x1);                                      // :309
  out[3] = (y2 * x1 - x2 * y1) / spline_pow(py_sq(x1) + py_sq(y1), 1.5);   // :289
}

}  // namespace rpp

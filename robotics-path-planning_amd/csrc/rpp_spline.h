// rpp_spline.h -- natural cubic spline course through waypoints, host + device source like rpp_lqr.h.
// Reference: 10_path_planning_00_cubic_spline_path.py
//   CubicSpline1D.__init__ :48-73 (b and d :69-71), calc_position :93-94, calc_first_derivative :117,
//   calc_second_derivative :139, __search_index :146, __calc_B :171-172,
//   CubicSpline2D.__calc_s :240-246, calc_curvature :289, calc_yaw :309, calc_spline_course :313-325; the range tests of the
//   pointwise methods :86-89.
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

// One spline over knots the caller supplies (CubicSpline1D.__init__ :48-73; s strictly increasing is the caller's to report,
// an equal pair is found here): c -- copied from c_in when given, else the Thomas recurrence above -- then b and d
// (:69-71).  b, c, d hold n doubles each; b[n-1] and d[n-1] are zeroed (the reference's lists have n - 1 entries).  The
// forward sweep keeps cp in d and dp in c.  Returns kSplineOk or kSplineDegenerate (some h[i] == 0: nothing is valid then).
RPP_HD static inline int spline_fit_knots(const double* s, const double* a, int n, const double* c_in, double* b, double* c,
                                          double* d) {
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

// One axis `a` (x or y) of one course of n >= 2 waypoints: the knots s (CubicSpline2D.__calc_s), then spline_fit_knots over
// them.  s, b, c, d hold n doubles each.  Returns kSplineOk or kSplineDegenerate (nothing but s is valid then).
RPP_HD static inline int spline_fit_axis(const double* x, const double* y, const double* a, int n, const double* c_in,
                                         double* s, double* b, double* c, double* d) {
  spline_chord_sum(x, y, n, s);
  return spline_fit_knots(s, a, n, c_in, b, c, d);
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

// bisect.bisect(s, t) - 1 (:146) for s[0] <= t < s[n-1]: the segment 0 .. n-2 that holds t
RPP_HD static inline int spline_segment(const double* s, int n, double t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (t < s[mid])
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo - 1;
}

// One axis on segment i at u = t - s[i], u2 = u ** 2.0, u3 = u ** 3.0: p = {position :93-94, first derivative :117, second
// derivative :139}
RPP_HD static inline void spline_axis_forms(const double* a, const double* b, const double* c, const double* d, int i, double u,
                                            double u2, double u3, double* p) {
  p[0] = a[i] + b[i] * u + c[i] * u2 + d[i] * u3;
  p[1] = b[i] + 2.0 * c[i] * u + 3.0 * d[i] * u2;
  p[2] = 2.0 * c[i] + 6.0 * d[i] * u;
}

// calc_curvature :289 of the first (x1, y1) and second (x2, y2) derivatives
RPP_HD static inline double spline_curvature(double x1, double y1, double x2, double y2) {
  return (y2 * x1 - x2 * y1) / spline_pow(py_sq(x1) + py_sq(y1), 1.5);
}

// The course's point at parameter t (0 <= t < s[n-1]): out = {x, y, yaw, curvature}
RPP_HD static inline void spline_eval(const double* s, const double* ax, const double* bx, const double* cx,
                                      const double* dx, const double* ay, const double* by, const double* cy,
                                      const double* dy, int n, double t, double* out) {
  const int i = spline_segment(s, n, t);
  const double u = t - s[i];
  const double u2 = spline_pow(u, 2.0), u3 = spline_pow(u, 3.0);
  double px[3], py[3];
  spline_axis_forms(ax, bx, cx, dx, i, u, u2, u3, px);
  spline_axis_forms(ay, by, cy, dy, i, u, u2, u3, py);
  out[0] = px[0];
  out[1] = py[0];
  out[2] = rpp_glibc_atan2(py[1], px[1]);   // :309
  out[3] = spline_curvature(px[1], py[1], px[2], py[2]);
}

// ---- pointwise queries at a caller's parameter (the classes' calc_* methods :75-140, :248-310) ----
constexpr int kSplineQOk = 0;          // RRTX_SPLINE_Q_OK
constexpr int kSplineQOutside = 1;     // RRTX_SPLINE_Q_OUTSIDE: t < s[0] or t > s[n-1] (+-inf too): the reference returns None
constexpr int kSplineQRefRaises = 2;   // RRTX_SPLINE_Q_REF_RAISES: t == s[n-1] or t is NaN: both range tests are false, bisect
                                       // lands on the last knot and the reference's self.b[i] raises IndexError
constexpr int kSplineQNoSpline = 3;    // RRTX_SPLINE_Q_NO_SPLINE: the course is kSplineDegenerate (the caller's to tell)

// What the reference does with parameter t on a spline over the knots s (:86-91); only kSplineQOk may be evaluated
RPP_HD static inline int spline_query_class(const double* s, int n, double t) {
  if (t < s[0] || t > s[n - 1]) return kSplineQOutside;
  if (!(t < s[n - 1])) return kSplineQRefRaises;
  return kSplineQOk;
}

// u ** y of a query, y = 2.0 or 3.0 and u >= 0: libm pow as spline_pow takes it.  A caller's parameter can lie one ulp above a
// knot at 0, which a sampled k * ds does not: where libm's result is below 2^-1022 (u < 2^-511 for y = 2.0, u < 2^-340.7 for
// 3.0) it leaves through its underflow handlers, which rpp_glibc_pow does not restate (it raises its flag and returns NaN).
// There the power is the product u * u (* u) as the hardware rounds it: 0.0 wherever libm's is 0.0 (u < 2^-537.5 / 2^-358.4),
// and in the subnormal window between the two within one unit of the last place of libm's.
RPP_HD static inline double spline_query_pow(double u, double y) {
  if (u == 0.0) return 0.0;
  int underflow = 0;
  const double r = rpp_glibc_pow_raw(u, y, &underflow);
  if (!underflow) return r;
  return y == 2.0 ? u * u : u * u * u;
}

// The spline at a parameter t that spline_query_class answers with kSplineQOk.
//   AXES == 2: out = {x, y, yaw, curvature, dx, dy, ddx, ddy} (ay .. dy: the second axis)
//   AXES == 1: out = {y, dy, ddy} of the axis ax .. dx (ay .. dy are not read)
// The forms are spline_eval's; the powers are spline_query_pow's.  t may be -0.0 (the reference's -0.0 < s[0] is false):
// u = -0.0 then, and numpy's u ** 2.0 is +0.0 but u ** 3.0 is -0.0, so u3 takes the sign of u here; a sampled parameter
// k * ds is never a negative zero.
template <int AXES>
RPP_HD static inline void spline_query(const double* s, const double* ax, const double* bx, const double* cx, const double* dx,
                                       const double* ay, const double* by, const double* cy, const double* dy, int n, double t,
                                       double* out) {
  const int i = spline_segment(s, n, t);
  const double u = t - s[i];
  const double u2 = spline_query_pow(u, 2.0), u3 = __builtin_copysign(spline_query_pow(u, 3.0), u);
  double px[3];
  spline_axis_forms(ax, bx, cx, dx, i, u, u2, u3, px);
  if (AXES == 1) {
    out[0] = px[0];
    out[1] = px[1];
    out[2] = px[2];
    return;
  }
  double py[3];
  spline_axis_forms(ay, by, cy, dy, i, u, u2, u3, py);
  out[0] = px[0];
  out[1] = py[0];
  out[2] = rpp_glibc_atan2(py[1], px[1]);
  out[3] = spline_curvature(px[1], py[1], px[2], py[2]);
  out[4] = px[1];
  out[5] = py[1];
  out[6] = px[2];
  out[7] = py[2];
}

}  // namespace rpp

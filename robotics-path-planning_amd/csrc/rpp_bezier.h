// rpp_bezier.h -- Bezier curve between two poses or over given control points, host + device source like rpp_spline.h.
// Reference: 10_path_planning_00_bazier_path.py
//   calc_4points_bezier_path :25-30 (control points from two poses), calc_bezier_path :46 (np.linspace(0, 1, n_points)),
//   bernstein_poly :61, bezier :72-73, bezier_derivatives_control_points :89-94, curvature :107.
//
// Arithmetic: every double is the reference's on glibc 2.35 + numpy: np.hypot = rpp_glibc_hypot, np.cos / np.sin of a scalar
// = libm's, `t ** i`, `(1 - t) ** (n - i)`, `dx ** 2` and `** (3 / 2)` on numpy doubles = libm pow (rpp_glibc_pow, every
// exponent, 0 and 1 included: no shortcut is taken), scipy.special.comb(n, i) = the exact binomial coefficient, np.sum over
// the rows of w_i * P_i = a left-to-right sum per axis that starts from numpy's identity 0.0 (0.0 + w_0 P_0 + ...: a sum of
// nothing but -0.0 comes out as +0.0, as the reference's does), and
// every product and sum rounded where the reference's expression rounds it (no FMA contraction may be applied to this file).
// The pow replica leaves its domain (NaN) where |y ln x| >= 512; the weights never get there (t >= 1 / 4095, exponents
// <= 15), a derivative would with a non-zero magnitude below 1e-111.
//
// yaw = math.atan2(dy, dx), the curve's length (the left-to-right sum of math.hypot over consecutive points) and
// kmax = np.max(np.abs(k)) are this package's own definitions: the script returns none of the three.
//
// A weight depends on (n_points, degree, k, i) and on no curve, so one table serves a whole batch: row k holds, for the
// curve's m control points, the m weights of degree m - 1, then the m - 1 of degree m - 2 (first derivative), then the
// m - 2 of degree m - 3 (second derivative): 3 m - 3 doubles.
#pragma once
#include "rpp_core.h"

namespace rpp {

constexpr int kBezierMinCp = 3;         // degree 1 makes the reference's second-derivative call raise
constexpr int kBezierMaxCp = 16;        // comb(n, i) is exact in a double far beyond; 15 is the degree the tests cover
constexpr int kBezierMaxPoints = 4096;  // points per curve

// On the device the table is read through the constant address space where the row is the same in every lane (stage 1):
// nothing writes it while a curve kernel runs, so a weight is one scalar load for the wave.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const double __attribute__((address_space(4)))* BezierRow;
#else
typedef const double* BezierRow;
#endif

constexpr int bezier_row_len(int m) { return 3 * m - 3; }   // (constexpr: the host API sizes the table with it too)

// np.linspace(0, 1, n_points)[k]: k * step with step = 1.0 / (n_points - 1), and the last entry the stop itself
RPP_HD static inline double bezier_t(int k, int n_points) {
  return k == n_points - 1 ? 1.0 : (double)k * (1.0 / (double)(n_points - 1));
}

// float(C(n, i)) for 0 <= i <= n <= 30: C(n - i + j, j) for j = 1 .. i, each step an exact integer division
RPP_HD static inline double bezier_comb(int n, int i) {
  uint32_t c = 1;
  for (int j = 1; j <= i; j++) c = c * (uint32_t)(n - i + j) / (uint32_t)j;
  return (double)c;
}

// bernstein_poly(n, i, t) :61
RPP_HD static inline double bezier_weight(int n, int i, double t) {
  return (bezier_comb(n, i) * rpp_glibc_pow(t, (double)i)) * rpp_glibc_pow(1.0 - t, (double)(n - i));
}

// Entry j of row k of the table for m control points and n_points parameters
RPP_HD static inline double bezier_table_entry(int n_points, int m, int k, int j) {
  int deg = m - 1;
  if (j >= m) {
    j -= m;
    deg = m - 2;
    if (j >= m - 1) {
      j -= m - 1;
      deg = m - 3;
    }
  }
  return bezier_weight(deg, j, bezier_t(k, n_points));
}

// calc_4points_bezier_path :25-30: P[8] = the four control points as rows (x, y)
RPP_HD static inline void bezier_cp4(double sx, double sy, double syaw, double ex, double ey, double eyaw, double offset,
                                     double* P) {
  const double dist = rpp_glibc_hypot(sx - ex, sy - ey) / offset;
  P[0] = sx;
  P[1] = sy;
  P[2] = sx + dist * rpp_glibc_cos(syaw);
  P[3] = sy + dist * rpp_glibc_sin(syaw);
  P[4] = ex - dist * rpp_glibc_cos(eyaw);
  P[5] = ey - dist * rpp_glibc_sin(eyaw);
  P[6] = ex;
  P[7] = ey;
}

// The curve's point of one table row `w`: o = {x, y, dx, dy, ddx, ddy}; nder = 0 stops after the point, 1 after the
// first derivative.  One pass over the control points: the derivative control points D1_j = n (P_j+1 - P_j) :92 and
// D2_j = (n - 1) (D1_j+1 - D1_j) are formed as the pass reaches them, so no array of them exists.  M > 0 fixes the number
// of control points at compile time (P may then live in registers); M == 0 takes m.
template <int M, class Row>
RPP_HD static inline void bezier_eval(const double* P, int m_rt, Row w, int nder, double* o) {
  const int m = M ? M : m_rt;
  const double fn = (double)(m - 1), fn1 = (double)(m - 2);
  double x = 0.0, y = 0.0, dx = 0.0, dy = 0.0, ddx = 0.0, ddy = 0.0;   // :73 np.sum starts every sum at 0.0
  double px = 0.0, py = 0.0, ex0 = 0.0, ey0 = 0.0;   // P_j-1 and D1_j-2
#pragma unroll
  for (int j = 0; j < m; j++) {
    const double qx = P[2 * j], qy = P[2 * j + 1];
    const double w0 = w[j];
    x = x + w0 * qx;
    y = y + w0 * qy;
    if (nder >= 1 && j >= 1) {
      const double ex = fn * (qx - px), ey = fn * (qy - py);   // D1_j-1
      const double w1 = w[m + j - 1];
      dx = dx + w1 * ex;
      dy = dy + w1 * ey;
      if (nder >= 2 && j >= 2) {
        const double gx = fn1 * (ex - ex0), gy = fn1 * (ey - ey0);   // D2_j-2
        const double w2 = w[2 * m - 1 + j - 2];
        ddx = ddx + w2 * gx;
        ddy = ddy + w2 * gy;
      }
      ex0 = ex;
      ey0 = ey;
    }
    px = qx;
    py = qy;
  }
  o[0] = x;
  o[1] = y;
  o[2] = dx;
  o[3] = dy;
  o[4] = ddx;
  o[5] = ddy;
}

// curvature :107; a zero denominator gives numpy's nan (0 / 0) or inf
RPP_HD static inline double bezier_curvature(double dx, double dy, double ddx, double ddy) {
  return (dx * ddy - dy * ddx) / rpp_glibc_pow(rpp_glibc_pow(dx, 2.0) + rpp_glibc_pow(dy, 2.0), 1.5);
}

// np.max(np.abs(k)) as a running value that starts at 0.0: a NaN stays
RPP_HD static inline double bezier_kmax_step(double km, double k) {
  const double a = dabs(k);
  return (a != a || a > km) ? a : km;
}

// Stage 1 of one curve: the walk over its n_points points for the length and, when wanted, the largest |curvature|
template <int M, class Row>
RPP_HD static inline void bezier_walk(const double* P, int m_rt, Row table, int n_points, bool want_k, double* length,
                                      double* kmax) {
  const int row = bezier_row_len(M ? M : m_rt);
  double len = 0.0, km = 0.0, lx = 0.0, ly = 0.0, o[6];
  for (int k = 0; k < n_points; k++) {
    bezier_eval<M>(P, m_rt, table + (int64_t)k * row, want_k ? 2 : 0, o);
    if (k > 0) len += py_hypot(o[0] - lx, o[1] - ly);
    lx = o[0];
    ly = o[1];
    if (want_k) km = bezier_kmax_step(km, bezier_curvature(o[2], o[3], o[4], o[5]));
  }
  *length = len;
  *kmax = km;
}

}  // namespace rpp

// rpp_bspline.h -- interpolating B-spline courses of degree 1 .. 5 through waypoints, host + device source like rpp_spline.h.
// Reference: 10_path_planning_00_bspline_path.py  interpolate_b_spline_path :59-88, _calc_distance_vector :91-96,
//            _evaluate_spline :99-108;  10_path_planning_00_spline_2d.py  Spline2D :12-28, the driver loop :45-54.
//
// The reference's doubles, bit for bit (glibc 2.35 + numpy): the waypoint parameter (np.hypot = rpp_glibc_hypot, a
// left-to-right sum, for bspline_path the division by the last entry), the knot vector that FITPACK with s = 0 and
// make_interp_spline's not-a-knot default both choose, the sample parameters of np.linspace and np.arange, and interp1d's
// linear kind (np.interp).  No FMA contraction may be applied to this file.
//
// This file's own definition (scipy's FITPACK is not one arithmetic): the coefficients and the evaluation.
//   basis      N = {1.0}; for j = 1 .. k: left[j] = x - t[mu+1-j], right[j] = t[mu+j] - x, saved = 0.0,
//              for r = 0 .. j-1: temp = N[r] / (right[r+1] + left[j-r]); N[r] = saved + right[r+1] * temp;
//              saved = left[j-r] * temp;  then N[j] = saved.  The rows of degree k-2, k-1 and k are kept.
//   derivative den[r] = t[mu+1+r] - t[mu-k+1+r], a1[r] = Nk1[r] / den[r]        r = 0 .. k-1
//              D1[r] = k * (a1[r-1] - a1[r])                                      r = 0 .. k
//              a2[r] = Nk2[r] / (t[mu+1+r] - t[mu-k+2+r])                         r = 0 .. k-2
//              E[r] = (k-1) * (a2[r-1] - a2[r]), b[r] = E[r] / den[r]             r = 0 .. k-1
//              D2[r] = k * (b[r-1] - b[r])                                        r = 0 .. k
//              a term whose index is outside its range is 0.0; degree 1 has D2 = 0.0
//   dot        acc = c[mu-k] * w[0]; acc = acc + c[mu-k+r] * w[r], r = 1 .. k
//   fit        band rows A[i][j] = N_j(u_i) with k sub- and k super-diagonals; Gaussian elimination without pivoting (the
//              matrix is totally positive under the Schoenberg-Whitney conditions, which these knots meet by construction):
//              for p = 0 .. m-2, r = p+1 .. min(p+k, m-1): l = A[r][p] / A[p][p]; A[r][p] = l;
//              A[r][c] = A[r][c] - l * A[p][c], c = p+1 .. min(p+k, m-1).  Per axis y[r] = y[r] - A[r][p] * y[p] in the same
//              order, then for i = m-1 .. 0: acc = y[i]; acc = acc - A[i][c] * y[c], c = i+1 .. min(i+k, m-1); y[i] = acc / A[i][i].
// tests/bspline_oracle.py states the same in Python; the two are bit-identical.
#pragma once
#include "rpp_spline.h"

namespace rpp {

constexpr int kBsplineOk = 0;           // RRTX_BSPLINE_OK
constexpr int kBsplineDegenerate = 1;   // RRTX_BSPLINE_DEGENERATE: the waypoint parameter is not strictly increasing
constexpr int kBsplineTooFew = 2;       // RRTX_BSPLINE_TOO_FEW: waypoints <= degree
constexpr int kBsplineMaxDegree = 5;
constexpr int kBsplineNormalised = 0;   // RRTX_BSPLINE_PARAM_NORMALISED: _calc_distance_vector, u in [0, 1]
constexpr int kBsplineChord = 1;        // RRTX_BSPLINE_PARAM_CHORD: Spline2D.__calc_s; degree 1 is interp1d's linear kind
constexpr int kBsplineLinspace = 0;     // RRTX_BSPLINE_SAMPLE_LINSPACE: np.linspace(0.0, u[-1], count)
constexpr int kBsplineArange = 1;       // RRTX_BSPLINE_SAMPLE_ARANGE: np.arange(0, s[-1], ds)
constexpr int kBsplineExplicit = 2;     // RRTX_BSPLINE_SAMPLE_EXPLICIT: the caller's sample parameters

// The waypoint parameter of m >= 2 waypoints into u[m]; kBsplineOk or kBsplineDegenerate (u not strictly increasing: some
// chord is zero, or vanishes against the sum; all waypoints equal leaves u at zeros)
RPP_HD static inline int bspline_parameter(const double* x, const double* y, int m, int param, double* u) {
  spline_chord_sum(x, y, m, u);
  if (param == kBsplineNormalised) {
    const double last = u[m - 1];
    if (last != 0.0)
      for (int i = 0; i < m; i++) u[i] = u[i] / last;   // distances /= distances[-1] (:95)
  }
  for (int i = 0; i + 1 < m; i++)
    if (!(u[i + 1] > u[i])) return kBsplineDegenerate;
  return kBsplineOk;
}

// The m + k + 1 knots of m > k waypoint parameters: clamped ends, interior the data sites (odd k) or their midpoints (even k)
RPP_HD static inline void bspline_knots(const double* u, int m, int k, double* t) {
  for (int i = 0; i <= k; i++) {
    t[i] = u[0];
    t[m + i] = u[m - 1];
  }
  const int ni = m - k - 1;
  if (k & 1) {
    for (int i = 0; i < ni; i++) t[k + 1 + i] = u[(k + 1) / 2 + i];
  } else {
    for (int i = 0; i < ni; i++) t[k + 1 + i] = (u[k / 2 + i] + u[k / 2 + i + 1]) / 2.0;
  }
}

// mu in [k, m-1] with t[mu] <= x < t[mu+1]; x at (or past) the last knot gets the last non-empty span m - 1
RPP_HD static inline int bspline_span(const double* t, int m, int k, double x) {
  int lo = k, hi = m;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (x < t[mid])
      hi = mid;
    else
      lo = mid;
  }
  return lo;
}

// The K + 1 weights of c[mu-K .. mu] for the value (N) and, with DERIV, the first and second derivative (D1, D2) at x on
// span mu.  Every loop has a compile-time bound, so the arrays live in registers.
template <int K, bool DERIV>
RPP_HD static inline void bspline_weights(const double* t, int mu, double x, double* N, double* D1, double* D2) {
  double Nk1[K], Nk2[K > 1 ? K - 1 : 1], tl[K + 1], tr[K + 1], left[K + 1], right[K + 1];
  N[0] = 1.0;
  if (K == 1) Nk1[0] = 1.0;
  if (K == 2) Nk2[0] = 1.0;
#pragma unroll
  for (int j = 1; j <= K; j++) {
    tl[j] = t[mu + 1 - j];
    tr[j] = t[mu + j];
    left[j] = x - tl[j];
    right[j] = tr[j] - x;
    double saved = 0.0;
#pragma unroll
    for (int r = 0; r < j; r++) {
      const double temp = N[r] / (right[r + 1] + left[j - r]);
      N[r] = saved + right[r + 1] * temp;
      saved = left[j - r] * temp;
    }
    N[j] = saved;
    if (DERIV && j == K - 1) {
#pragma unroll
      for (int r = 0; r <= j; r++) Nk1[r] = N[r];
    }
    if (DERIV && j == K - 2) {
#pragma unroll
      for (int r = 0; r <= j; r++) Nk2[r] = N[r];
    }
  }
  if (!DERIV) return;
  double den[K], a1[K];
#pragma unroll
  for (int r = 0; r < K; r++) {
    den[r] = tr[r + 1] - tl[K - r];
    a1[r] = Nk1[r] / den[r];
  }
#pragma unroll
  for (int r = 0; r <= K; r++) D1[r] = (double)K * ((r >= 1 ? a1[r >= 1 ? r - 1 : 0] : 0.0) - (r < K ? a1[r < K ? r : 0] : 0.0));
  if (K == 1) {
    D2[0] = 0.0;
    D2[1] = 0.0;
    return;
  }
  constexpr int K1 = K > 1 ? K - 1 : 1;
  double a2[K1], b[K];
#pragma unroll
  for (int r = 0; r < K1; r++) a2[r] = Nk2[r] / (tr[r + 1] - tl[K1 - r]);
#pragma unroll
  for (int r = 0; r < K; r++) {
    const double E = (double)(K - 1) * ((r >= 1 ? a2[r >= 1 ? r - 1 : 0] : 0.0) - (r < K1 ? a2[r < K1 ? r : 0] : 0.0));
    b[r] = E / den[r];
  }
#pragma unroll
  for (int r = 0; r <= K; r++) D2[r] = (double)K * ((r >= 1 ? b[r >= 1 ? r - 1 : 0] : 0.0) - (r < K ? b[r < K ? r : 0] : 0.0));
}

// The values N[0 .. k] alone, k at run time (the collocation rows of the fit)
RPP_HD static inline void bspline_values(const double* t, int mu, int k, double x, double* N) {
  switch (k) {
    case 1: bspline_weights<1, false>(t, mu, x, N, nullptr, nullptr); break;
    case 2: bspline_weights<2, false>(t, mu, x, N, nullptr, nullptr); break;
    case 3: bspline_weights<3, false>(t, mu, x, N, nullptr, nullptr); break;
    case 4: bspline_weights<4, false>(t, mu, x, N, nullptr, nullptr); break;
    default: bspline_weights<5, false>(t, mu, x, N, nullptr, nullptr); break;
  }
}

// q = {x, y, dx, dy, ddx, ddy} of the spline (t, cx, cy) over m waypoints at v
template <int K>
RPP_HD static inline void bspline_eval_k(const double* t, int m, const double* cx, const double* cy, double v, double* q) {
  const int mu = bspline_span(t, m, K, v);
  double w[3][K + 1];
  bspline_weights<K, true>(t, mu, v, w[0], w[1], w[2]);
  double px[K + 1], py[K + 1];
#pragma unroll
  for (int r = 0; r <= K; r++) {
    px[r] = cx[mu - K + r];
    py[r] = cy[mu - K + r];
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    double ax = px[0] * w[d][0], ay = py[0] * w[d][0];
#pragma unroll
    for (int r = 1; r <= K; r++) {
      ax = ax + px[r] * w[d][r];
      ay = ay + py[r] * w[d][r];
    }
    q[2 * d] = ax;
    q[2 * d + 1] = ay;
  }
}

// interp1d(kind="linear") over the waypoints (s, ax, ay) at v.  For real one-dimensional data interp1d hands the call to
// np.interp: j is the last waypoint with s[j] <= v; at or past the last waypoint the value is the last waypoint's, on a
// waypoint exactly that waypoint's, else slope * (v - s[j]) + a[j] with slope = (a[j+1] - a[j]) / (s[j+1] - s[j]).  The
// derivatives are the slopes of that interval (the last interval at the end) and zero.
RPP_HD static inline void bspline_eval_linear(const double* s, const double* ax, const double* ay, int m, double v, double* q) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (v < s[mid])
      hi = mid;
    else
      lo = mid + 1;
  }
  const int j = lo - 1;
  const int i = j < 0 ? 0 : (j > m - 2 ? m - 2 : j);
  const double h = s[i + 1] - s[i];
  const double sx = (ax[i + 1] - ax[i]) / h, sy = (ay[i + 1] - ay[i]) / h;
  if (j < 0) {
    q[0] = ax[0];
    q[1] = ay[0];
  } else if (j >= m - 1) {
    q[0] = ax[m - 1];
    q[1] = ay[m - 1];
  } else if (s[j] == v) {
    q[0] = ax[j];
    q[1] = ay[j];
  } else {
    q[0] = sx * (v - s[j]) + ax[j];
    q[1] = sy * (v - s[j]) + ay[j];
  }
  q[2] = sx;
  q[3] = sy;
  q[4] = 0.0;
  q[5] = 0.0;
}

// out = {x, y, heading, curvature} from q = {x, y, dx, dy, ddx, ddy}.  The curvature keeps the script's exponent
// (:107, np.power(dx * dx + dy * dy, 2.0 / 3.0)): it is not the geometric 3 / 2.
RPP_HD static inline void bspline_point(const double* q, double* out) {
  out[0] = q[0];
  out[1] = q[1];
  out[2] = rpp_glibc_atan2(q[3], q[2]);
  out[3] = (q[5] * q[2] - q[4] * q[3]) / spline_pow(q[2] * q[2] + q[3] * q[3], 2.0 / 3.0);
}

// The course's point at parameter v: out = {x, y, heading, curvature}
RPP_HD static inline void bspline_eval(const double* u, const double* ax, const double* ay, const double* t, const double* cx,
                                       const double* cy, int m, int k, int param, double v, double* out) {
  double q[6];
  if (param == kBsplineChord && k == 1) {
    bspline_eval_linear(u, ax, ay, m, v, q);
  } else {
    switch (k) {
      case 1: bspline_eval_k<1>(t, m, cx, cy, v, q); break;
      case 2: bspline_eval_k<2>(t, m, cx, cy, v, q); break;
      case 3: bspline_eval_k<3>(t, m, cx, cy, v, q); break;
      case 4: bspline_eval_k<4>(t, m, cx, cy, v, q); break;
      default: bspline_eval_k<5>(t, m, cx, cy, v, q); break;
    }
  }
  bspline_point(q, out);
}

// Coefficients of one course of m > k waypoints: the band matrix in ab -- plane d = j - i + k of row i at ab[d * stride + i],
// 2 k + 1 planes -- factored once, then cx and cy (each m doubles) by substitution from the waypoints ax, ay
RPP_HD static inline void bspline_fit(const double* u, const double* t, int m, int k, const double* ax, const double* ay,
                                      double* ab, int64_t stride, double* cx, double* cy) {
  for (int d = 0; d <= 2 * k; d++)
    for (int i = 0; i < m; i++) ab[d * stride + i] = 0.0;
  for (int i = 0; i < m; i++) {
    const int mu = bspline_span(t, m, k, u[i]);
    double N[kBsplineMaxDegree + 1];
    bspline_values(t, mu, k, u[i], N);
    for (int r = 0; r <= k; r++) {
      const int d = mu - i + r;   // column mu - k + r
      if (d >= 0 && d <= 2 * k) ab[d * stride + i] = N[r];
    }
    cx[i] = ax[i];
    cy[i] = ay[i];
  }
#define RPP_BS_A(i, j) ab[(int64_t)((j) - (i) + k) * stride + (i)]
  for (int p = 0; p + 1 < m; p++) {
    const double piv = RPP_BS_A(p, p);
    const int last = p + k < m - 1 ? p + k : m - 1;
    for (int r = p + 1; r <= last; r++) {
      const double l = RPP_BS_A(r, p) / piv;
      RPP_BS_A(r, p) = l;
      for (int c = p + 1; c <= last; c++) RPP_BS_A(r, c) = RPP_BS_A(r, c) - l * RPP_BS_A(p, c);
    }
  }
  for (int axis = 0; axis < 2; axis++) {
    double* y = axis ? cy : cx;
    for (int p = 0; p + 1 < m; p++) {
      const int last = p + k < m - 1 ? p + k : m - 1;
      for (int r = p + 1; r <= last; r++) y[r] = y[r] - RPP_BS_A(r, p) * y[p];
    }
    for (int i = m - 1; i >= 0; i--) {
      const int last = i + k < m - 1 ? i + k : m - 1;
      double acc = y[i];
      for (int c = i + 1; c <= last; c++) acc = acc - RPP_BS_A(i, c) * y[c];
      y[i] = acc / RPP_BS_A(i, i);
    }
  }
#undef RPP_BS_A
}

// Sample i of `count`: np.linspace(0.0, stop, count) -- i * step with step = stop / (count - 1), the last entry stop itself,
// count 1 gives 0.0, and numpy's other branch i / (count - 1) * stop when the step underflows to zero --, np.arange(0, stop,
// ds) -- i * ds --, or the caller's us[i]
RPP_HD static inline double bspline_sample(int mode, double stop, int64_t count, double ds, const double* us, int64_t i) {
  if (mode == kBsplineExplicit) return us[i];
  if (mode == kBsplineArange) return (double)i * ds;
  if (count == 1) return 0.0;
  if (i == count - 1) return stop;
  const double div = (double)(count - 1);
  const double step = stop / div;
  if (step == 0.0) return (double)i / div * stop;
  return (double)i * step;
}

}  // namespace rpp

// bspline_smooth.hip.h -- the smoothing fit of approximate_b_spline_path for batches of waypoint lists (gfx950): for every
// course what approximate_b_spline_path(x, y, n, degree, s) of 10_path_planning_00_bspline_path.py :12-56 returns.  Scalar
// pieces: csrc/rpp_bspline_smooth.h (the fit) and csrc/rpp_bspline.h (parameter, basis, samples, heading and curvature).
//
// Two kernels around the host's prefix sum, as bspline_batch.hip.h:
//   bspline_smooth_fit_kernel   one lane per (course, axis), lane 2 c + axis: the waypoint parameter, then the knot loop and the
//                               root search of its axis, sequential by nature.  The lane writes its axis' knots, coefficients
//                               and record; axis 0's lane also writes the course's record and resets its hit word (the two
//                               lanes of a course are neighbours in one wave and exchange their "not finite" flag by a
//                               shuffle).  Everything a lane reads back it wrote itself.  A course with s == 0 is the
//                               interpolating fit of bspline_fit_kernel, made by axis 0's lane for both axes.
//   bspline_smooth_eval_kernel  one lane per output point, shaped like bspline_eval_kernel; each axis has its own span search
//                               and basis, because the two axes have knot vectors of their own.
// Workspace, waypoint CSR layout, W = waypoints of the batch: tab holds 2 x 31 planes of W doubles, axis after axis -- 0 the
// waypoint parameter, 1 the coefficients, 2 .. 30 the planes of rpp_bspline_smooth.h (z, fpint, nrdata, q, the band, its wide
// copy, the jumps); 62 planes, 496 bytes per waypoint --; the knots of axis a of course c, at most m + 6 doubles, start at
// knots[a (W + 6 n) + wp_off[c] + 6 c]; arec holds the axis records, axis-major.
#pragma once
#include "bspline_batch.hip.h"
#include "rpp_bspline_smooth.h"

namespace rppbs {

constexpr int SMOOTH_AXIS_PLANES = 2 + rpp::kSmoothPlanes;
constexpr int SMOOTH_TAB_PLANES = 2 * SMOOTH_AXIS_PLANES;
static_assert(rpp::kSmoothPlanes >= 2 * rpp::kBsplineMaxDegree + 1, "the interpolating fit's band fits the smoothing fit's planes");

struct SmoothArgs {
  Args a;                  // tab: [SMOOTH_TAB_PLANES][W]; knots: [2][W + KNOT_SLACK * n]
  const double* s;         // [n] or [1]
  int32_t s_per_course;
  rpp::SmoothInfo* arec;   // [2][n]
};

__global__ __launch_bounds__(FIT_TPB) void bspline_smooth_fit_kernel(SmoothArgs sa) {
  const Args& a = sa.a;
  const int64_t lane = (int64_t)blockIdx.x * FIT_TPB + threadIdx.x;
  const int64_t c = lane >> 1;
  const int axis = (int)(lane & 1);
  if (c >= a.n) return;   // the two lanes of a course leave together
  const int64_t w0 = a.wp_off[c];
  const int m = (int)(a.wp_off[c + 1] - w0);   // 2 <= m <= MAX_WAYPOINTS (host)
  const int k = course_degree(a, c);           // 1 <= k <= 5 (host)
  const double s = sa.s[sa.s_per_course ? c : 0];
  const int64_t knot_plane = a.W + KNOT_SLACK * a.n;
  double* u = a.tab + (int64_t)axis * SMOOTH_AXIS_PLANES * a.W + w0;
  double* cf = u + a.W;
  double* w = u + 2 * a.W;
  double* t = a.knots + axis * knot_plane + w0 + KNOT_SLACK * c;
  int st = rpp::bspline_parameter(a.x + w0, a.y + w0, m, rpp::kBsplineNormalised, u);
  if (st == rpp::kBsplineOk && m <= k) st = rpp::kBsplineTooFew;
  rpp::SmoothInfo info;
  info.n_knots = 0;
  info.ier = 0;
  info.fp = 0.0;
  info.p = 0.0;
  info.rounds = 0;
  info.iters = 0;
  int bad = 0;
  if (st != rpp::kBsplineOk) {
    sa.arec[axis * a.n + c] = info;
  } else if (s == 0.0) {
    if (axis == 0) {   // the interpolating spline, exactly as bspline_fit_kernel makes it
      double* cy = cf + (int64_t)SMOOTH_AXIS_PLANES * a.W;
      double* ty = t + knot_plane;
      rpp::bspline_knots(u, m, k, t);
      rpp::bspline_fit(u, t, m, k, a.x + w0, a.y + w0, w, a.W, cf, cy);
      for (int i = 0; i < m + k + 1; i++) ty[i] = t[i];
      info.n_knots = m + k + 1;
      info.ier = -1;
      info.p = __builtin_huge_val();
      sa.arec[c] = info;
      sa.arec[a.n + c] = info;
    }
  } else {
    rpp::bspline_smooth_fit(u, (axis ? a.y : a.x) + w0, m, k, s, w, a.W, t, cf, &info);
    for (int i = 0; i < info.n_knots - k - 1; i++)
      if (!isfinite(cf[i])) bad = 1;
    sa.arec[axis * a.n + c] = info;
  }
  const int other = __shfl_xor(bad, 1);
  if (axis != 0) return;
  if (st == rpp::kBsplineOk && (bad | other)) st = rpp::kBsplineSingular;
  Record r;
  r.status = st;
  r.degree = k;
  r.n_points = 0;
  r.length = 0.0;
  if (st == rpp::kBsplineOk) {
    r.length = u[m - 1];
    const int mode = course_mode(a, c);
    if (mode == rpp::kBsplineLinspace)
      r.n_points = a.count[a.per_course ? c : 0];
    else if (mode == rpp::kBsplineArange)
      r.n_points = rpp::arange_count(r.length, a.ds[a.per_course ? c : 0]);
    else
      r.n_points = a.us_off[c + 1] - a.us_off[c];
  }
  a.rec[c] = r;
  if (a.hit) a.hit[c] = r.n_points > 0 ? -1 : -2;
}

// The lanes past the last point, and hit[], as in bspline_eval_kernel
template <bool STORE, int CHECK>
__global__ __launch_bounds__(TPB) void bspline_smooth_eval_kernel(SmoothArgs sa) {
  const Args& a = sa.a;
  int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int64_t total = a.pt_off[a.n];
  const bool live = idx < total;
  if (!live) {
    if (!CHECK) return;
    idx = total - 1;   // the launch has total > 0
  }
  const int64_t lo = rppc::csr_row(a.pt_off, a.n, idx);   // the course of this point
  const int64_t w0 = a.wp_off[lo];
  const int m = (int)(a.wp_off[lo + 1] - w0);
  const int k = course_degree(a, lo);
  const int64_t i = idx - a.pt_off[lo];
  const double* u = a.tab + w0;
  const int mode = course_mode(a, lo);
  const double v = rpp::bspline_sample(mode, u[m - 1], a.pt_off[lo + 1] - a.pt_off[lo],
                                       mode == rpp::kBsplineArange ? a.ds[a.per_course ? lo : 0] : 0.0,
                                       mode == rpp::kBsplineExplicit ? a.us + a.us_off[lo] : nullptr, i);
  const int64_t knot_plane = a.W + KNOT_SLACK * a.n;
  const double* tx = a.knots + w0 + KNOT_SLACK * lo;
  const double* cx = u + a.W;
  double p[4];
  rpp::bspline_smooth_eval(tx, sa.arec[lo].n_knots, cx, tx + knot_plane, sa.arec[a.n + lo].n_knots,
                           cx + (int64_t)SMOOTH_AXIS_PLANES * a.W, k, v, p);
  if (STORE && live) {
    for (int q = 0; q < 4; q++) a.out[q * total + idx] = p[q];
    a.out[4 * total + idx] = v;
  }
  if (CHECK) rppc::check_point<CHECK>(a.obs, a.n_obs, a.omap, a.hit, lo, p[0], p[1]);
}

}  // namespace rppbs

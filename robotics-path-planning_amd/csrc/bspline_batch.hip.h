// bspline_batch.hip.h -- interpolating B-spline courses of degree 1 .. 5 through batches of waypoint lists (gfx950): for every
// course what interpolate_b_spline_path(x, y, n, degree) of 10_path_planning_00_bspline_path.py :59-108 returns, or what the
// driver loop of 10_path_planning_00_spline_2d.py :45-54 collects from Spline2D.  Scalar pieces: csrc/rpp_bspline.h.
//
// Two kernels with a CSR layout on each side, as spline_batch.hip.h:
//   bspline_fit_kernel   one lane per course: the waypoint parameter, the knots, the collocation matrix in band form, its
//                        factorisation without pivoting and the two substitutions; the lane also writes the course's record
//                        -- status, degree, point count, u[-1] or s[-1] -- and resets its hit word.  The sweeps are sequential
//                        per course.  Everything a lane reads back it wrote itself: no lane reads another lane's stores.
//   offsets              exclusive sum of the point counts into int64 offsets (host).
//   bspline_eval_kernel  one lane per output point: binary search of the point index in the offsets, the sample parameter of
//                        its mode, the span by binary search over the knots, then the basis with its two derivatives in
//                        registers (rpp::bspline_weights<K>: every loop bound is a compile-time constant, the degree selects
//                        the instantiation), the dot products, heading and curvature.  STORE writes x, y, yaw, k, u; CHECK
//                        tests the point against the obstacle list and takes the lowest index touched into hit[course].
// Workspace, waypoint CSR layout, W = waypoints of the batch: tab holds 14 planes of W doubles -- 0 the waypoint parameter,
// 1 cx, 2 cy, 3 .. 13 the band planes d = j - i + k (2 k + 1 of them are used) --; the knots of course c, m + k + 1 <= m + 6
// doubles, start at knots[wp_off[c] + 6 c].
#pragma once
#include "curve_check.hip.h"
#include "rpp_bspline.h"

namespace rppbs {

constexpr int TPB = 256;
constexpr int FIT_TPB = 64;           // one lane per course and long sequential sweeps: small blocks spread the courses over the CUs
constexpr int MAX_WAYPOINTS = 4096;   // per course: bounds one lane's sequential sweep (include/rrtx.h)
constexpr int TAB_PLANES = 3 + 2 * rpp::kBsplineMaxDegree + 1;
constexpr int KNOT_SLACK = rpp::kBsplineMaxDegree + 1;
using rppc::CHECK_NONE, rppc::CHECK_LINEAR, rppc::CHECK_INDEX;   // the eval kernels' CHECK (curve_check.hip.h)

struct Record {   // rrtx_bspline_record
  int32_t status, degree;
  int64_t n_points;
  double length;   // u[-1] (1.0) or s[-1]; 0.0 unless status is OK
};

struct Args {
  int64_t n;                 // courses
  int64_t W;                 // waypoints in all = wp_off[n]
  const int64_t* wp_off;     // [n + 1]
  const double *x, *y;       // [W]
  const int32_t* degree;     // [n] or [1]
  int32_t degree_per_course;
  int32_t param;             // rpp::kBsplineNormalised / kBsplineChord
  int32_t mode;              // rpp::kBsplineLinspace / kBsplineArange / kBsplineExplicit
  const int32_t* mode_of;    // [n] a mode per course, or nullptr: `mode` for all
  int32_t per_course;        // count or ds: one per course, else one for the batch
  const int64_t* count;      // linspace: [n] or [1]
  const double* ds;          // arange: [n] or [1]
  const int64_t* us_off;     // explicit: [n + 1]
  const double* us;          // explicit: [us_off[n]]
  double* tab;               // [TAB_PLANES][W]
  double* knots;             // [W + KNOT_SLACK * n]
  Record* rec;               // [n]
  const int64_t* pt_off;     // [n + 1]
  double* out;               // [5][pt_off[n]]: x, y, yaw, k, u
  const double* obs;         // [n_obs] rows (ox, oy, thr), thr = (size + robot_radius) ** 2 from the host
  int64_t n_obs;
  int32_t* hit;              // [n]  fit: -1 (OK) / -2 (no points); eval: the lowest obstacle index touched
  rppo::Map omap;            // CHECK_INDEX: the grid over the same list
};

__device__ inline int course_degree(const Args& a, int64_t c) { return a.degree[a.degree_per_course ? c : 0]; }
__device__ inline int course_mode(const Args& a, int64_t c) { return a.mode_of ? a.mode_of[c] : a.mode; }

__global__ __launch_bounds__(FIT_TPB) void bspline_fit_kernel(Args a) {
  const int64_t c = (int64_t)blockIdx.x * FIT_TPB + threadIdx.x;
  if (c >= a.n) return;
  const int64_t w0 = a.wp_off[c];
  const int m = (int)(a.wp_off[c + 1] - w0);   // 2 <= m <= MAX_WAYPOINTS (host)
  const int k = course_degree(a, c);           // 1 <= k <= 5 (host)
  double* u = a.tab + w0;
  double* cx = a.tab + a.W + w0;
  double* cy = a.tab + 2 * a.W + w0;
  double* t = a.knots + w0 + KNOT_SLACK * c;
  int st = rpp::bspline_parameter(a.x + w0, a.y + w0, m, a.param, u);
  if (st == rpp::kBsplineOk && m <= k) st = rpp::kBsplineTooFew;
  Record r;
  r.status = st;
  r.degree = k;
  r.n_points = 0;
  r.length = 0.0;
  if (st == rpp::kBsplineOk) {
    rpp::bspline_knots(u, m, k, t);
    rpp::bspline_fit(u, t, m, k, a.x + w0, a.y + w0, a.tab + 3 * a.W + w0, a.W, cx, cy);
    r.length = u[m - 1];
    const int mode = course_mode(a, c);
    if (mode == rpp::kBsplineLinspace)
      r.n_points = a.count[a.per_course ? c : 0];
    else if (mode == rpp::kBsplineArange)
      r.n_points = rpp::arange_count(r.length, a.ds[a.per_course ? c : 0]);
    else
      r.n_points = a.us_off[c + 1] - a.us_off[c];
  } else {   // no spline: the coefficients a caller reads back are zero
    for (int i = 0; i < m; i++) {
      cx[i] = 0.0;
      cy[i] = 0.0;
    }
  }
  a.rec[c] = r;
  if (a.hit) a.hit[c] = r.n_points > 0 ? -1 : -2;
}

// The lanes past the last point, and hit[]: curve_check.hip.h
template <bool STORE, int CHECK>
__global__ __launch_bounds__(TPB) void bspline_eval_kernel(Args a) {
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
  double p[4];
  rpp::bspline_eval(u, a.x + w0, a.y + w0, a.knots + w0 + KNOT_SLACK * lo, u + a.W, u + 2 * a.W, m, k, a.param, v, p);
  if (STORE && live) {
    for (int q = 0; q < 4; q++) a.out[q * total + idx] = p[q];
    a.out[4 * total + idx] = v;
  }
  if (CHECK) rppc::check_point<CHECK>(a.obs, a.n_obs, a.omap, a.hit, lo, p[0], p[1]);
}

}  // namespace rppbs

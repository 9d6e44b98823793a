// spline_batch.hip.h -- cubic-spline courses through batches of waypoint lists (gfx950): for every course what
// calc_spline_course(x, y, ds) of 10_path_planning_00_cubic_spline_path.py :313-325 returns.  Scalar pieces: csrc/rpp_spline.h.
//
// Courses differ in waypoints and in points, so the work is two kernels with a CSR layout on each side:
//   spline_fit_kernel   one lane per (course, axis): the knots s (np.hypot, left-to-right sum), c by the Thomas recurrence or
//                       copied from the caller's, b and d; the axis-0 lane also writes the course's record -- status, point
//                       count len(np.arange(0, s[-1], ds)), s[-1] -- and resets its hit word.  The recurrences are sequential
//                       per course and axis; the two lanes of a course run the same trip counts.  Each axis keeps a knot
//                       plane of its own, so no lane reads what another wrote.
//   offsets             exclusive sum of the point counts into int64 offsets (host).
//   spline_eval_kernel  one lane per output point: binary search of the point index in the offsets, t = k * ds,
//                       bisect_right over the course's knots, then position, derivatives, yaw and curvature (spline_eval).
//                       STORE writes x, y, yaw, k, t; CHECK tests the point against the obstacle list (rpp_collide.h) and
//                       takes the lowest obstacle index any point of the course touches into hit[course].
// After a run the splines stay on the device, and answer at parameters of the caller's choosing (the classes' calc_* methods):
//   spline_query_kernel  one lane per query of a CSR list per spline (q_off, t): the spline of the lane is found in q_off as
//                        spline_eval_kernel finds its course in pt_off (rows may be empty), the parameter is classified
//                        (spline_query_class: outside the knots, on the last knot or NaN, no spline) and only then
//                        evaluated (spline_query).  Planes of Q doubles -- AXES 2: x, y, yaw, k (DERIV: dx, dy, ddx, ddy);
//                        AXES 1: y (DERIV: dy, ddy) -- and a status plane; every value of a query that is not answered
//                        is NaN.  Knots and coefficients come from global memory; no atomics, no lane reads another's.
//   spline_fit1d_kernel  one lane per spline over knots the caller supplies (CubicSpline1D): the host puts the knots into
//                        plane 0 and the values into x; the lane writes planes 2 .. 4 and the record.
// The coefficient table is eight planes of W doubles (W = waypoints of the batch), waypoint CSR layout:
//   0 s (axis x's), 1 s (axis y's copy), 2 bx, 3 cx, 4 dx, 5 by, 6 cy, 7 dy;  a = the waypoints themselves.
#pragma once
#include "curve_check.hip.h"
#include "rpp_spline.h"

namespace rppsp {

constexpr int TPB = 256;
constexpr int MAX_WAYPOINTS = 4096;   // per course: bounds one lane's sequential sweep (include/rrtx.h)
using rppc::CHECK_NONE, rppc::CHECK_LINEAR, rppc::CHECK_INDEX, rppc::csr_row;   // spline_eval_kernel's CHECK (curve_check.hip.h)

struct Record {   // rrtx_spline_record
  int32_t status, reserved;
  int64_t n_points;
  double length;   // s[-1]
};

struct Args {
  int64_t n;               // courses
  int64_t W;               // waypoints in all = wp_off[n]
  const int64_t* wp_off;   // [n + 1]
  const double *x, *y;     // [W]
  const double* ds;        // [n] or [1]
  int32_t ds_per_course;
  const double *cx, *cy;   // [W] the caller's c, or nullptr: the Thomas recurrence
  double* tab;             // [8][W]
  Record* rec;             // [n]
  const int64_t* pt_off;   // [n + 1]
  double* out;             // [5][pt_off[n]]: x, y, yaw, k, s
  const double* obs;       // [n_obs] rows (ox, oy, thr), thr = (size + robot_radius) ** 2 from the host
  int64_t n_obs;
  int32_t* hit;            // [n]  fit: -1 (RRTX_SPLINE_OK) / -2 (no points); eval: the lowest obstacle index touched
  rppo::Map omap;          // CHECK_INDEX: the grid over the same list
};

__device__ inline double course_ds(const Args& a, int64_t c) { return a.ds[a.ds_per_course ? c : 0]; }

__global__ __launch_bounds__(TPB) void spline_fit_kernel(Args a) {
  const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (idx >= 2 * a.n) return;
  const int64_t c = idx >> 1;
  const int axis = (int)(idx & 1);
  const int64_t w0 = a.wp_off[c];
  const int n = (int)(a.wp_off[c + 1] - w0);   // 2 <= n <= MAX_WAYPOINTS (host)
  const double* wa = (axis ? a.y : a.x) + w0;
  const double* cin = a.cx ? (axis ? a.cy : a.cx) + w0 : nullptr;
  double* s = a.tab + (int64_t)axis * a.W + w0;
  double* b = a.tab + (int64_t)(2 + 3 * axis) * a.W + w0;
  int st = rpp::spline_fit_axis(a.x + w0, a.y + w0, wa, n, cin, s, b, b + a.W, b + 2 * a.W);
  if (st != rpp::kSplineOk)   // no spline: the c a caller reads back is zero
    for (int i = 0; i < n; i++) b[a.W + i] = 0.0;
  if (axis) return;
  Record r;
  r.status = st;
  r.reserved = 0;
  r.length = s[n - 1];
  r.n_points = st == rpp::kSplineOk ? rpp::spline_count(r.length, course_ds(a, c), &st) : 0;
  r.status = st;
  a.rec[c] = r;
  if (a.hit) a.hit[c] = st == rpp::kSplineOk ? -1 : -2;
}

// The lanes past the last point, and hit[]: curve_check.hip.h
template <bool STORE, int CHECK>
__global__ __launch_bounds__(TPB) void spline_eval_kernel(Args a) {
  int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int64_t total = a.pt_off[a.n];
  const bool live = idx < total;
  if (!live) {
    if (!CHECK) return;
    idx = total - 1;   // the launch has total > 0
  }
  const int64_t lo = csr_row(a.pt_off, a.n, idx);   // the course of this point
  const int64_t w0 = a.wp_off[lo];
  const int n = (int)(a.wp_off[lo + 1] - w0);
  const double t = (double)(idx - a.pt_off[lo]) * course_ds(a, lo);
  const double* tb = a.tab + w0;
  double p[4];
  rpp::spline_eval(tb, a.x + w0, tb + 2 * a.W, tb + 3 * a.W, tb + 4 * a.W, a.y + w0, tb + 5 * a.W, tb + 6 * a.W, tb + 7 * a.W,
                   n, t, p);
  if (STORE && live) {
    for (int q = 0; q < 4; q++) a.out[q * total + idx] = p[q];
    a.out[4 * total + idx] = t;
  }
  if (CHECK) rppc::check_point<CHECK>(a.obs, a.n_obs, a.omap, a.hit, lo, p[0], p[1]);
}

struct QueryArgs {
  int64_t n;               // splines of the last fit
  int64_t W;               // their waypoints (knots) in all
  int64_t Q;               // queries in all = q_off[n]
  const int64_t* wp_off;   // [n + 1]
  const int64_t* q_off;    // [n + 1]
  const double* t;         // [Q]
  const double *x, *y;     // [W] the a of each axis (y is not read with one axis)
  const double* tab;       // [8][W]
  const Record* rec;       // [n]
  double* out;             // [planes][Q]
  int32_t* status;         // [Q] RRTX_SPLINE_Q_*
};

template <int AXES, bool DERIV>
__global__ __launch_bounds__(TPB) void spline_query_kernel(QueryArgs a) {
  constexpr int VALUES = AXES == 2 ? 8 : 3;                                   // what spline_query writes
  constexpr int PLANES = AXES == 2 ? (DERIV ? 8 : 4) : (DERIV ? 3 : 1);       // what is stored
  const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (idx >= a.Q) return;
  const int64_t c = csr_row(a.q_off, a.n, idx);
  const int64_t w0 = a.wp_off[c];
  const int n = (int)(a.wp_off[c + 1] - w0);
  const double t = a.t[idx];
  const double* tb = a.tab + w0;
  double p[VALUES];
  const int st = a.rec[c].status == rpp::kSplineDegenerate ? rpp::kSplineQNoSpline : rpp::spline_query_class(tb, n, t);
  if (st == rpp::kSplineQOk) {
    rpp::spline_query<AXES>(tb, a.x + w0, tb + 2 * a.W, tb + 3 * a.W, tb + 4 * a.W, a.y + w0, tb + 5 * a.W, tb + 6 * a.W,
                            tb + 7 * a.W, n, t, p);
  } else {
    for (int q = 0; q < VALUES; q++) p[q] = __builtin_nan("");
  }
  for (int q = 0; q < PLANES; q++) a.out[q * a.Q + idx] = p[q];
  a.status[idx] = st;
}

struct Fit1dArgs {
  int64_t n;               // splines
  int64_t W;               // knots in all
  const int64_t* wp_off;   // [n + 1]
  const double* a;         // [W] the values
  const double* c;         // [W] the caller's c, or nullptr: the Thomas recurrence
  double* tab;             // [8][W]: plane 0 holds the knots (host); planes 2 .. 4 are written here
  Record* rec;             // [n]
};

__global__ __launch_bounds__(TPB) void spline_fit1d_kernel(Fit1dArgs a) {
  const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (c >= a.n) return;
  const int64_t w0 = a.wp_off[c];
  const int n = (int)(a.wp_off[c + 1] - w0);   // 2 <= n <= MAX_WAYPOINTS (host)
  const double* s = a.tab + w0;
  double* b = a.tab + 2 * a.W + w0;
  const int st = rpp::spline_fit_knots(s, a.a + w0, n, a.c ? a.c + w0 : nullptr, b, b + a.W, b + 2 * a.W);
  if (st != rpp::kSplineOk)   // no spline: the c a caller reads back is zero
    for (int i = 0; i < n; i++) b[a.W + i] = 0.0;
  Record r;
  r.status = st;
  r.reserved = 0;
  r.n_points = 0;
  r.length = s[n - 1];
  a.rec[c] = r;
}

}  // namespace rppsp

// rpp_lqr.h -- LQR steer of LQR-RRT* (rrt_09), host + device source like rpp_core.h.
// Reference: /root/reference/src_path_planning/10_path_planning_01_rrt_09_lqr_rrt_star.py (rrt_09); its LQRPlanner is,
//   line for line, the one of 10_path_planning_00_lqr_path.py :15-114 (the batch form: steer_batch.hip.h)
//   LQRPlanner.lqr_planning :944-986, solve_dare / dlqr :988-1018, get_system_model :1020-1026,
//   sample_path :1157-1172, steer :1174-1192, check_collision :1292-1305, calc_new_cost :1432-1442.
//
// The gain.  With A = [[0.1, 1], [0, 0.1]], B = [0, 1]^T, Q = I, R = I, solve_dare multiplies ELEMENTWISE (numpy `*` on
// arrays, :996) and stops on its second pass with X = [[1.0101, 0], [0, 1]]; dlqr then takes
// K = inv(B^T X B + R) (B^T X A) = (1 / (1 + 1)) [0, 0.1] = [0.0, 0.05] (bits 0x0p+0, 0x1.999999999999ap-5), the same
// for every call (tests/golden/lqr_kat.npz records K and X).
// So a steer is the scalar recurrence on the state x = from - to (numpy matmul rounding, tests/golden/lqr_kat.npz):
//   u   = -(0.0 * x0 + 0.05 * x1)
//   x0' = fma(0.1, x0, x1) + 0.0 * u        (OpenBLAS rounds row 0 of A @ x fused)
//   x1' = (0.0 * x0 + 0.1 * x1) + u
// appended as (x0' + gx, x1' + gy) while `time <= 100.0` (time += 0.1) until hypot(goal - point) <= 0.1.  The rollout
// is then resampled: t_k = k * step for k < ceil(1 / step) (np.arange(0, 1, step)), p = t * w[i+1] + (1 - t) * w[i].
// The polyline of an edge is therefore a pure function of (from, to, step): a node stores its edge's endpoints and the
// polyline is regenerated wherever it is needed (kernel, final course, Node.path_x).
#pragma once
#include "rpp_core.h"

namespace rpp {

constexpr double kLqrK0 = 0.0, kLqrK1 = 0.05;   // the constant dlqr gain (see above)
constexpr double kLqrDt = 0.1, kLqrMaxTime = 100.0, kLqrGoalDist = 0.1;

// number of resampling parameters per rollout segment: len(np.arange(0.0, 1.0, step)) = ceil(1 / step)
static inline int lqr_nt(double step) {
  const double q = 1.0 / step;
  int n = (int)q;
  if ((double)n < q) n++;
  return n;
}

// One step of the closed loop x' = A x + B u with u = -K x, rounded as above.  The one copy of the recurrence.
RPP_HD static inline void lqr_step(double* x0, double* x1) {
  const double u = -(kLqrK0 * *x0 + kLqrK1 * *x1);
  const double n0 = __builtin_fma(0.1, *x0, *x1) + 0.0 * u;
  const double n1 = (0.0 * *x0 + 0.1 * *x1) + u;
  *x0 = n0;
  *x1 = n1;
}

// lqr_planning :944-986 (= 10_path_planning_00_lqr_path.py :24-66) with MAX_TIME and GOAL_DIST as arguments.  Calls
// seg(wx, wy, rx, ry) for every rollout segment, previous point -> new point, in order; returns the number of rollout
// points (len(rx): >= 2), or 0 when the rollout never gets within goal_dist (lqr_planning returns [], []).  `time`
// gains 0.1 per pass, so max_time <= 100.0 bounds the rollout at 1001 segments.
template <class S>
RPP_HD static inline int lqr_rollout(double sx, double sy, double gx, double gy, double max_time, double goal_dist,
                                     S&& seg) {
  double x0 = sx - gx, x1 = sy - gy;
  double wx = sx, wy = sy;   // previous rollout point
  int nw = 1;
  double time = 0.0;
  while (time <= max_time) {
    time += kLqrDt;
    lqr_step(&x0, &x1);
    const double rx = x0 + gx, ry = x1 + gy;
    seg(wx, wy, rx, ry);
    wx = rx;
    wy = ry;
    nw++;
    if (py_hypot(gx - rx, gy - ry) <= goal_dist) return nw;
  }
  return 0;
}

// One LQR rollout from (sx, sy) to (gx, gy), resampled with `nt` points per segment of parameter step `step`.
// Calls pt(k, px, py) for every resampled point in order (k = 0 ..), returns the number of rollout points
// (len(wx): >= 2), or 0 when the rollout never gets within goal_dist (lqr_planning returns [], []).
template <class F>
RPP_HD static inline int lqr_walk(double sx, double sy, double gx, double gy, double step, int nt, double max_time,
                                  double goal_dist, F&& pt) {
  int k = 0;
  return lqr_rollout(sx, sy, gx, gy, max_time, goal_dist, [&](double wx, double wy, double rx, double ry) {
    // segment (wx, wy) -> (rx, ry) of sample_path :1161-1165
    for (int j = 0; j < nt; j++) {
      const double t = (double)j * step;
      pt(k++, t * rx + (1.0 - t) * wx, t * ry + (1.0 - t) * wy);
    }
  });
}

// rrt_09's own LQRPlanner: MAX_TIME = 100.0, GOAL_DIST = 0.1 (:938-940)
template <class F>
RPP_HD static inline int lqr_walk(double sx, double sy, double gx, double gy, double step, int nt, F&& pt) {
  return lqr_walk(sx, sy, gx, gy, step, nt, kLqrMaxTime, kLqrGoalDist, pt);
}

// Point k of a rollout's polyline on its own, for a caller that knows the point count from lqr_walk / lqr_rollout: the
// recurrence is run to rollout segment k / nt without the goal test, then interpolated as sample_path does.  nt == 0:
// the rollout's own point k (rx[k], ry[k]).
RPP_HD static inline void lqr_point(double sx, double sy, double gx, double gy, double step, int nt, int k, double* x,
                                    double* y) {
  double x0 = sx - gx, x1 = sy - gy;
  const int seg = nt > 0 ? k / nt : k;
  for (int i = 0; i < seg; i++) lqr_step(&x0, &x1);
  const double wx = seg > 0 ? x0 + gx : sx, wy = seg > 0 ? x1 + gy : sy;
  if (nt == 0) {
    *x = wx;
    *y = wy;
    return;
  }
  lqr_step(&x0, &x1);
  const double rx = x0 + gx, ry = x1 + gy;
  const double t = (double)(k - seg * nt) * step;
  *x = t * rx + (1.0 - t) * wx;
  *y = t * ry + (1.0 - t) * wy;
}

// What every caller of steer / calc_new_cost needs from one edge, nothing stored: point count, endpoint px[-1],
// sum of the course lengths (Python's left-to-right sum from int 0), point-sampled collision (check_collision, thr =
// (size + robot_radius) ** 2 per obstacle).  ok = 0: the reference's rollout failed (steer raises IndexError at px[-1],
// calc_new_cost returns inf).
struct LqrEdge {
  int ok, np, coll;
  double ex, ey, len;
};

RPP_HD static inline LqrEdge lqr_edge(double sx, double sy, double gx, double gy, double step, int nt, const double* ox,
                                      const double* oy, const double* othr, int m) {
  LqrEdge e;
  e.coll = 0;
  e.len = 0.0;
  double px = 0.0, py = 0.0;
  const int nw = lqr_walk(sx, sy, gx, gy, step, nt, [&](int k, double qx, double qy) {
    if (k > 0) e.len += py_hypot(qx - px, qy - py);
    px = qx;
    py = qy;
    if (!e.coll)
      for (int o = 0; o < m; o++) {
        const double dx = ox[o] - qx, dy = oy[o] - qy;
        if (dx * dx + dy * dy <= othr[o]) {
          e.coll = 1;
          break;
        }
      }
  });
  e.ok = nw > 0;
  e.np = nw > 0 ? (nw - 1) * nt : 0;
  e.ex = px;
  e.ey = py;
  return e;
}

// The edge's polyline into (px, py) (at most cap points; returns the full count, 0 = failed rollout).
RPP_HD static inline int lqr_polyline(double sx, double sy, double gx, double gy, double step, int nt, double* px,
                                      double* py, int cap) {
  const int nw = lqr_walk(sx, sy, gx, gy, step, nt, [&](int k, double qx, double qy) {
    if (k < cap) {
      px[k] = qx;
      py[k] = qy;
    }
  });
  return nw > 0 ? (nw - 1) * nt : 0;
}

}  // namespace rpp

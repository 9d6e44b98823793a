// rpp_track.h -- scalar core of the closed-loop stage of closed-loop RRT* (rrt_10), host and device source.
// Reference: /root/reference/src_path_planning/10_path_planning_01_rrt_10_closed_loop_rrt_star.py (rrt_10)
//   State / update :1215-1232, PIDControl :1244-1252, pure_pursuit_control :1255-1283, calc_target_index :1286-1304,
//   closed_loop_prediction :1307-1372, set_stop_point :1375-1417, extend_path :1430-1445,
//   check_tracking_path_is_feasible :1526-1564, get_goal_indexes :1566-1582, search_best_feasible_path :1495-1524.
// The model constants are module globals there (:1592-1607); here they are fields of Params with those defaults.
// Arithmetic: doubles bit-identical to CPython 3.10 / numpy on glibc 2.35 -- math.cos / sin / atan2 / tan through the
// lifted libm (glibc235_fma_math.h), math.hypot = rpp::py_hypot, np.hypot = rpp_glibc_hypot (glibc's own hypot, which is
// NOT math.hypot), angle_mod = numpy `%` (rpp::angle_mod_pi).  No FMA contraction may be applied to this file.
// rpp_glibc_tan is stated for |x| <= 0.79 (its argument is delta, clamped to +-steer_max, 40 deg by default); a larger
// steer_max raises the out-of-domain flag (Record::ood) instead of returning a wrong number.
#pragma once
#include "rpp_core.h"
#include "rpp_dubins.h"
#include "rpp_obsgrid.h"

namespace rppt {

struct Params {
  double target_speed, yaw_th, xy_th, invalid_travel_ratio;                 // ClosedLoopRRTStar.__init__ :1458-1476
  double dt, L, steer_max, accel_max, Kp, Lf, T, goal_dis, stop_speed;      // module globals :1592-1607
};

struct State {
  double x, y, yaw, v;
};

// which of the four tests of check_tracking_path_is_feasible refused the roll-out (:1542-1562)
constexpr int F_REACH = 1, F_ANGLE = 2, F_LONG = 4, F_COLL = 8;
// speed_profile entries (:1376-1413) as codes: the profile only ever holds these five values
constexpr signed char SP_FWD = 0, SP_BACK = 1, SP_ZERO = 2, SP_STOP = 3, SP_STOP_BACK = 4;
constexpr int EXT_MAX = 64;   // extend_path appends int(Lf / 0.1) + 1 points (6 with the default Lf); more than this is refused

struct Record {          // what check_tracking_path_is_feasible returned for one candidate
  int32_t find;          // find_goal as returned (:1564)
  int32_t n;             // len(t)
  int32_t fail;          // F_* bits
  int32_t ood;           // 1: the libm replica left its stated domain (tan beyond 0.79), 2: the reference raises (course < 3 points),
                         // 3: the course exceeds the kernel's capacity (device only)
  double tlast;          // t[-1]
};

RPP_HD static inline double speed_of(signed char code, const Params& P) {
  switch (code) {
    case SP_FWD: return P.target_speed;
    case SP_BACK: return -P.target_speed;
    case SP_ZERO: return 0.0;
    case SP_STOP: return P.stop_speed;
    default: return -P.stop_speed;
  }
}

// update :1224-1232
RPP_HD static inline void update(State& s, double a, double delta, const Params& P, int* ood) {
  const double nx = s.x + s.v * rpp_glibc_cos(s.yaw) * P.dt;
  const double ny = s.y + s.v * rpp_glibc_sin(s.yaw) * P.dt;
  const double nyaw = s.yaw + s.v / P.L * rpp_glibc_tan_ood(delta, ood) * P.dt;
  s.x = nx;
  s.y = ny;
  s.yaw = rpp::angle_mod_pi(nyaw);
  s.v = s.v + a * P.dt;
}

// PIDControl :1244-1252
RPP_HD static inline double pid(double target, double current, const Params& P) {
  double a = P.Kp * (target - current);
  if (a > P.accel_max)
    a = P.accel_max;
  else if (a < -P.accel_max)
    a = -P.accel_max;
  return a;
}

// the look-ahead walk of calc_target_index :1295-1301 (math.hypot)
RPP_HD static inline int lookahead(const double* cx, const double* cy, int n, int ind, double Lf) {
  double L = 0.0;
  while (Lf > L && (ind + 1) < n) {
    L += rpp::py_hypot(cx[ind + 1] - cx[ind], cy[ind + 1] - cy[ind]);
    ind += 1;
  }
  return ind;
}

// calc_target_index :1286-1293, the scan: d = np.hypot(dx, dy), min(d), np.argmin(d) (first minimum)
RPP_HD static inline int nearest_scan(const State& s, const double* cx, const double* cy, int n, double* mindis) {
  double best = rpp::dinf();
  int bi = 0;
  for (int i = 0; i < n; i++) {
    const double d = rpp_glibc_hypot(s.x - cx[i], s.y - cy[i]);
    if (d < best) {
      best = d;
      bi = i;
    }
  }
  *mindis = best;
  return bi;
}

// pure_pursuit_control :1255-1283 after the scan (ind0, the arg-min)
RPP_HD static inline double pure_pursuit(const State& s, const double* cx, const double* cy, int n, int pind, int ind0,
                                         const Params& P, int* ind_out) {
  int ind = lookahead(cx, cy, n, ind0, P.Lf);
  if (pind >= ind) ind = pind;
  double tx, ty;
  if (ind < n) {
    tx = cx[ind];
    ty = cy[ind];
  } else {
    tx = cx[n - 1];
    ty = cy[n - 1];
    ind = n - 1;
  }
  double alpha = rpp_glibc_atan2(ty - s.y, tx - s.x) - s.yaw;
  if (s.v <= 0.0) alpha = rpp::kPi - alpha;   // back
  double delta = rpp_glibc_atan2(2.0 * P.L * rpp_glibc_sin(alpha) / P.Lf, 1.0);
  if (delta > P.steer_max)
    delta = P.steer_max;
  else if (delta < -P.steer_max)
    delta = -P.steer_max;
  *ind_out = ind;
  return delta;
}

// One trip of the loop of closed_loop_prediction :1325-1353 after the scan.  Returns 1 when the goal test breaks the
// loop (BEFORE the state is appended, :1343-1345); otherwise the caller appends (s, time, *ai, *di).
RPP_HD static inline int step(State& s, int& target_ind, double& time, const double* cx, const double* cy,
                              const signed char* sp, int n, int ind0, double dis, double gx, double gy, const Params& P,
                              double* ai, double* di, int* ood) {
  int ind;
  *di = pure_pursuit(s, cx, cy, n, target_ind, ind0, P, &ind);
  target_ind = ind;
  const double maxdis = 0.5;
  const double lim = maxdis - 0.1;
  const double md = lim < dis ? lim : dis;   // min(dis, maxdis - 0.1)
  double target_speed = speed_of(sp[target_ind], P);
  target_speed = target_speed * (maxdis - md) / maxdis;
  *ai = pid(target_speed, s.v, P);
  update(s, *ai, *di, P, ood);
  if (rpp::dabs(s.v) <= P.stop_speed && target_ind <= n - 2) target_ind += 1;
  time = time + P.dt;
  return rpp::py_hypot(s.x - gx, s.y - gy) <= P.goal_dis ? 1 : 0;
}

// extend_path :1430-1445: appends the points behind cx / cy / cyaw[n - 1]; returns the new length (n >= 3), or -1 when
// more than EXT_MAX points would be appended
RPP_HD static inline int extend_path(double* cx, double* cy, double* cyaw, int n, const Params& P) {
  const double dl = 0.1;
  const double q = P.Lf / dl;
  if (!(q < (double)EXT_MAX)) return -1;
  const int cnt = (int)q + 1;
  const double move_direction = rpp_glibc_atan2(cy[n - 1] - cy[n - 3], cx[n - 1] - cx[n - 3]);
  const bool is_back = rpp::dabs(move_direction - cyaw[n - 1]) >= rpp::kPi / 2.0;
  const double idl = is_back ? dl * -1 : dl;
  for (int k = 0; k < cnt; k++) {
    cx[n] = cx[n - 1] + idl * rpp_glibc_cos(cyaw[n - 1]);
    cy[n] = cy[n - 1] + idl * rpp_glibc_sin(cyaw[n - 1]);
    cyaw[n] = cyaw[n - 1];
    n++;
  }
  return n;
}

// is_back of one course segment, set_stop_point :1384-1391: bit 0 is_back, bit 1 dx == 0 and dy == 0 (`continue`)
RPP_HD static inline int segment_flags(const double* cx, const double* cy, const double* cyaw, int i) {
  const double dx = cx[i + 1] - cx[i], dy = cy[i + 1] - cy[i];
  const double move_direction = rpp_glibc_atan2(dy, dx);
  const int is_back = rpp::dabs(move_direction - cyaw[i]) >= rpp::kPi / 2.0;
  return is_back | ((dx == 0.0 && dy == 0.0) ? 2 : 0);
}

// set_stop_point :1375-1413 from the per-segment flags (sp[i] holds segment_flags(i) on entry, i < n - 1)
RPP_HD static inline void stop_points(signed char* sp, int n) {
  bool forward = true, is_back = false;
  for (int i = 0; i < n - 1; i++) {
    const int f = sp[i];
    sp[i] = SP_FWD;
    is_back = f & 1;
    if (f & 2) continue;
    sp[i] = is_back ? SP_BACK : SP_FWD;
    if (is_back && forward) {
      sp[i] = SP_ZERO;
      forward = false;
    } else if (!is_back && !forward) {
      sp[i] = SP_ZERO;
      forward = true;
    }
  }
  sp[0] = SP_ZERO;
  sp[n - 1] = is_back ? SP_STOP_BACK : SP_STOP;
}

// origin_travel :1550: sum(np.hypot(np.diff(cx), np.diff(cy))), a sequential Python sum
RPP_HD static inline double origin_travel(const double* cx, const double* cy, int n) {
  double s = 0.0;
  for (int i = 0; i + 1 < n; i++) s = s + rpp_glibc_hypot(cx[i + 1] - cx[i], cy[i + 1] - cy[i]);
  return s;
}

// the tests of check_tracking_path_is_feasible :1542-1562 on the finished roll-out
RPP_HD static inline void judge(Record* r, int reached, double last_yaw_mod, double goal_yaw, double vsum, double origin,
                                int hit, const Params& P) {
  int fail = reached ? 0 : F_REACH;
  if (rpp::dabs(last_yaw_mod - goal_yaw) >= P.yaw_th * 10.0) fail |= F_ANGLE;
  const double travel = P.dt * vsum;
  if ((travel / origin) >= P.invalid_travel_ratio) fail |= F_LONG;
  if (hit) fail |= F_COLL;
  r->fail = fail;
  r->find = fail == 0;
}

// selection rule of search_best_feasible_path :1504-1513: `best_time >= t[-1]` lets a later candidate win a tie
RPP_HD static inline bool better(int find, double tlast, double best_time) { return find && best_time >= tlast; }

// ---- courses read in place from a producer's device buffers (rrtx_tracker_run_from) ------------------------------------
// Record::ood there also takes 4: a pose component of the course is not finite (the host path refuses the whole batch for
// this; here the host never sees the points), and 5: the selection left the course out, its points were not read.
constexpr int OOD_NOT_FINITE = 4, OOD_SKIPPED = 5;
constexpr int SEL_ALL = 0, SEL_FREE = 1, SEL_MASK = 2;   // include/rrtx.h RRTX_SELECT_*

// NaN or +-inf
RPP_HD static inline bool not_finite(double v) { return (rpp::d2b(v) & 0x7ff0000000000000ULL) == 0x7ff0000000000000ULL; }

// Whether `select` keeps a course: hit is its entry of the producer's hits (SEL_FREE), mask its byte (SEL_MASK)
RPP_HD static inline bool course_selected(int select, int32_t hit, uint8_t mask) {
  return select == SEL_ALL || (select == SEL_FREE ? hit == -1 : mask != 0);
}

// The ood code of one course of `len` points, `cap` the longest course the kernel holds.  Asked twice: before the points
// are read (any_not_finite = false; non-zero: they are not read) and after, with what reading them found.
RPP_HD static inline int course_ood(bool selected, int64_t len, int64_t cap, bool any_not_finite) {
  if (!selected) return OOD_SKIPPED;
  if (len < 3) return 2;   // cy[-3] :1435 raises IndexError
  if (len > cap) return 3;
  return any_not_finite ? OOD_NOT_FINITE : 0;
}

// The same decision on one thread, reading the points only when the first answer is 0 (host checks)
RPP_HD static inline int course_ood_scan(bool selected, int64_t len, int64_t cap, const double* x, const double* y,
                                         const double* yaw) {
  const int gate = course_ood(selected, len, cap, false);
  if (gate) return gate;
  bool bad = false;
  for (int64_t q = 0; q < len; q++) bad = bad || not_finite(x[q]) || not_finite(y[q]) || not_finite(yaw[q]);
  return course_ood(selected, len, cap, bad);
}

// search_best_feasible_path :1504-1513 over the g records of one group, in order: the position of the complete (ood == 0)
// feasible record with the smallest t[-1], the later one of equal times; -1 none.  Records with ood != 0 are passed over
// (TrackResult.best() raises on them instead).
RPP_HD static inline int64_t group_pick(const Record* rec, int64_t g) {
  double best_time = rpp::dinf();
  int64_t win = -1;
  for (int64_t k = 0; k < g; k++)
    if (rec[k].ood == 0 && better(rec[k].find, rec[k].tlast, best_time)) {
      best_time = rec[k].tlast;
      win = k;
    }
  return win;
}

// get_goal_indexes :1566-1582 for one node
RPP_HD static inline bool is_candidate(double x, double y, double yaw, double gx, double gy, double gyaw, const Params& P) {
  return rpp::py_hypot(x - gx, y - gy) <= P.xy_th && rpp::dabs(yaw - gyaw) <= P.yaw_th;
}

// ---- the collision test of a roll-out (F_COLL): "some circle touches some appended point", an OR over the points -------------
// The OR does not depend on the order the points are tested in, nor on when.  The kernels' lane-per-obstacle form (at most 64
// circles) tests every point as it is appended; the obstacle-index form (rrt_track.hip.h CHECK_INDEX, any number of circles)
// defers: the point of step cnt is parked in lane pend_lane(cnt), and a wave-wide flush -- every lane asks
// rppo::point_first_hit for its own parked point -- runs when the 64 lanes are full and once behind the loop for the rest.
// The index's dependent loads (cell_start, then the items) so leave the serial step loop: one flush per 64 steps.
constexpr int PEND = 64;   // parked points of a wave, one per lane
// the lane that parks the point of step cnt (cnt = 0 is the start state)
RPP_HD static inline int pend_lane(int cnt) { return cnt & (PEND - 1); }
// whether a flush of all PEND lanes is due once `cnt` points have been appended
RPP_HD static inline bool pend_flush_due(int cnt) { return cnt > 0 && (cnt & (PEND - 1)) == 0; }
// whether `lane` still parks an untested point behind a loop that appended cnt points (the final flush)
RPP_HD static inline bool pend_final(int lane, int cnt) { return lane < (cnt & (PEND - 1)); }

// every circle of the list against the point at once: the reference's check_collision :321-334 per point
struct LinearCheck {
  const double *ox, *oy, *othr;
  int m;
  RPP_HD void point(int, double x, double y, int* hit) const {
    for (int o = 0; o < m; o++) {
      const double dx = ox[o] - x, dy = oy[o] - y;
      if (dx * dx + dy * dy <= othr[o]) *hit = 1;
    }
  }
  RPP_HD void finish(int, int*) const {}
};

// the deferred form on one thread, lane by lane as the kernel does it wave-wide
struct DeferredIndexCheck {
  rppo::Map map;
  double px[PEND], py[PEND];
  RPP_HD void flush(int lanes, int* hit) const {
    for (int l = 0; l < lanes; l++)
      if (rppo::point_first_hit(map, px[l], py[l]) >= 0) *hit = 1;
  }
  RPP_HD void point(int cnt, double x, double y, int* hit) {
    px[pend_lane(cnt)] = x;
    py[pend_lane(cnt)] = y;
    if (pend_flush_due(cnt + 1)) flush(PEND, hit);
  }
  RPP_HD void finish(int cnt, int* hit) const {
    for (int l = 0; l < PEND; l++)
      if (pend_final(l, cnt) && rppo::point_first_hit(map, px[l], py[l]) >= 0) *hit = 1;
  }
};

// check_tracking_path_is_feasible :1526-1564 on one thread (host tests; the kernel runs the same pieces wave-wide).
// cx / cy / cyaw: the course in driving order (start ... goal), n points, with room for EXT_MAX more; sp: n + EXT_MAX.
// out[7] (x, y, yaw, v, t, a, d; each `cap` doubles) may be null.  start: the state the roll-out begins in; the default
// is the reference's hard-coded State(-0.0, -0.0, 0.0, 0.0) (:1309).
// `check` answers the collision test: check.point(cnt, x, y, &hit) per appended point, check.finish(cnt, &hit) once behind
// the loop (LinearCheck, DeferredIndexCheck above).
template <class Check>
RPP_HD static inline void track_course_with(double* cx, double* cy, double* cyaw, signed char* sp, int n, Check& check,
                                            const Params& P, double* const* out, int cap, Record* r,
                                            State start = State{-0.0, -0.0, 0.0, 0.0}) {
  r->find = 0;
  r->n = 0;
  r->fail = 0;
  r->ood = 0;
  r->tlast = 0.0;
  if (n < 3) {   // cy[-3] :1435 raises IndexError
    r->ood = 2;
    return;
  }
  const double gx = cx[n - 1], gy = cy[n - 1], gyaw = cyaw[n - 1];
  n = extend_path(cx, cy, cyaw, n, P);
  if (n < 0) {
    r->ood = 1;
    return;
  }
  for (int i = 0; i < n - 1; i++) sp[i] = (signed char)segment_flags(cx, cy, cyaw, i);
  stop_points(sp, n);
  State s = start;
  double time = 0.0, vsum = 0.0, last_yaw = 0.0, tlast = 0.0;
  int cnt = 0, hit = 0, ood = 0, reached = 0;
  auto append = [&](double a, double d) {
    if (out && cnt < cap) {
      out[0][cnt] = s.x;
      out[1][cnt] = s.y;
      out[2][cnt] = rpp::angle_mod_pi(s.yaw);   // :1540
      out[3][cnt] = s.v;
      out[4][cnt] = time;
      out[5][cnt] = a;
      out[6][cnt] = d;
    }
    check.point(cnt, s.x, s.y, &hit);
    vsum = vsum + rpp::dabs(s.v);
    last_yaw = s.yaw;
    tlast = time;
    cnt++;
  };
  append(0.0, 0.0);
  double dis;
  int target_ind = lookahead(cx, cy, n, nearest_scan(s, cx, cy, n, &dis), P.Lf);
  while (P.T >= time) {
    const int ind0 = nearest_scan(s, cx, cy, n, &dis);
    double ai, di;
    if (step(s, target_ind, time, cx, cy, sp, n, ind0, dis, gx, gy, P, &ai, &di, &ood)) {
      reached = 1;
      break;
    }
    append(ai, di);
    if (ood) break;
  }
  check.finish(cnt, &hit);
  r->n = cnt;
  r->tlast = tlast;
  r->ood = ood;
  judge(r, reached, rpp::angle_mod_pi(last_yaw), gyaw, vsum, origin_travel(cx, cy, n), hit, P);
}

RPP_HD static inline void track_course(double* cx, double* cy, double* cyaw, signed char* sp, int n, const double* ox,
                                       const double* oy, const double* othr, int m, const Params& P, double* const* out,
                                       int cap, Record* r, State start = State{-0.0, -0.0, 0.0, 0.0}) {
  LinearCheck check = {ox, oy, othr, m};
  track_course_with(cx, cy, cyaw, sp, n, check, P, out, cap, r, start);
}

}  // namespace rppt

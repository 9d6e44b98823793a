// rrt_track.hip.h -- closed-loop stage of closed-loop RRT* (rrt_10) on planned Reeds-Shepp trees (gfx950).
// Reference: /root/reference/src_path_planning/10_path_planning_01_rrt_10_closed_loop_rrt_star.py (rrt_10)
//   ClosedLoopRRTStar.planning :1478-1493, search_best_feasible_path :1495-1524, check_tracking_path_is_feasible
//   :1526-1564, get_goal_indexes :1566-1582; the scalar pieces are csrc/rpp_track.h.
//
// Three kernels on the trees the planner kernel left on the device (nothing is copied to the host in between):
//   track_list_kernel  one wave per instance: the get_goal_indexes nodes in index order (ballot compaction), appended
//                      as (instance, candidate) jobs to one device-wide job list;
//   track_roll_kernel  persistent waves that take jobs from the list with an atomic counter (roll-outs differ by 10x in
//                      length: ~200 steps when the goal is reached, 2 001 on a time-out).  A job walks the parents and
//                      lays the course out (generate_final_course :1199-1207 reversed, then extend_path), sets the
//                      speed profile and rolls the unicycle along it.  Per step the lanes share the np.hypot scan of
//                      the course (first minimum, lowest index), the look-ahead walk and the state update are
//                      wave-uniform (every lane computes them), and lane k tests the new point against obstacle k, so
//                      check_collision is a running flag of the roll-out.  It records {find_goal, len(t), t[-1], failed
//                      tests} per candidate;
//   track_pick_kernel  one thread per instance: the feasible candidate with the smallest t[-1], the later one on ties.
// A second launch of track_roll_kernel (store = 1) re-runs each winner alone and stores its seven arrays: the
// roll-out is deterministic, so this costs one extra roll-out per instance instead of 2 002 x 7 doubles per candidate.
//
// track_courses_kernel is the same roll-out on courses given as data (rrtx_tracker_run, BatchTrack): its front end reads a
// course from the caller's CSR arrays instead of walking a tree; everything behind the laid-out course is roll_course, one
// text for both kernels.  The tree front end itself (the parent walk and the copy of the polylines) is lay_course, which
// goal_roll_kernel (goal_track.hip.h: the same stage for many goals per tree) calls as well.
//
// Capacities: a course (with its extension) of up to LDS_PTS points is held in LDS (x, y; the speed profile always is, one
// byte per point), up to SLAB_PTS points in the wave's global slab; a longer one sets RRTX_ST_OVERFLOW for the instance.
// Obstacles: at most 64 per instance (the Reeds-Shepp planner's tile) in the lane-per-obstacle form (CHECK_LINEAR); every
// roll kernel also comes in an obstacle-index form (CHECK_INDEX) that takes a shared list of up to 2^20 circles: the data
// kernels the tracker's obstacle index, track_roll_kernel and goal_roll_kernel the handle's obstacle map.
#pragma once
#include "curve_check.hip.h"
#include "rpp_track.h"
#include "rrt_rs.hip.h"

namespace rppt {

constexpr int TPB = 64;
constexpr int LDS_PTS = 512;
constexpr int SLAB_PTS = 1024;
constexpr int MAX_STEPS = 1 << 22;   // never spin on the device whatever T / dt is
constexpr int ST_OVERFLOW = 4, ST_RAISES = 32, ST_OOD = 16;   // include/rrtx.h status bits (OOD reported as UNSUPPORTED)
// how a roll-out tests its points against the circles: lane k against circle k (at most 64), or every lane's parked point
// through the obstacle index (rpp_obsgrid.h point_first_hit, rpp_track.h pend_*: any number of circles)
using rppc::CHECK_LINEAR, rppc::CHECK_INDEX;

struct Outcome {      // per instance
  int32_t flag;       // search_best_feasible_path found a feasible roll-out
  int32_t winner;     // its position in the candidate list (-1 none)
  int32_t n_cand;
  int32_t len;        // len(t) of the winner (x / y / yaw hold len + 1 values: the goal pose is appended, :1519-1521)
  int32_t node;       // the winner's node index
  int32_t status;     // 0, or RRTX_ST_OVERFLOW / RRTX_ST_REF_RAISES / RRTX_ST_UNSUPPORTED bits
};

struct TrackArgs {
  const rppk::Inst* inst;
  const double *x, *y, *yaw;
  const int32_t* parent;
  const int64_t* poff;
  const int32_t* plen;
  int64_t stride;
  const double* const* pool;   // [inst][3]: this instance's polyline pool (x, y, yaw)
  const double *ox, *oy, *othr;
  Params P;
  int32_t n_inst;
  int32_t* cand;       // [inst][stride]
  Record* rec;         // [inst][stride]
  int32_t* jobs;       // [2 * job]: instance, candidate position
  int32_t* counters;   // 0: jobs listed, 1: queue head
  double* slab;        // [block][3][SLAB_PTS]
  Outcome* outc;       // [inst]
  double* out;         // winners' arrays: instance i owns 7 x (len + 1) doubles at out_off[i]
  const int64_t* out_off;
};

__global__ __launch_bounds__(TPB) void track_list_kernel(TrackArgs a) {
  const int inst = blockIdx.x, lane = threadIdx.x;
  const rppk::Inst* I = a.inst + inst;
  const int64_t off = (int64_t)inst * a.stride;
  const int n = (I->status & (ST_OVERFLOW | ST_RAISES | ST_OOD)) ? 0 : I->n;   // a tree that did not finish has no candidates
  const double gx = I->goal[0], gy = I->goal[1], gyaw = I->goal[2];
  int k = 0;
  for (int base = 0; base < n; base += TPB) {
    const int i = base + lane;
    const bool c = i < n && is_candidate(a.x[off + i], a.y[off + i], a.yaw[off + i], gx, gy, gyaw, a.P);
    const unsigned long long b = __ballot(c);
    if (c) a.cand[off + k + __popcll(b & ((1ULL << lane) - 1ULL))] = i;
    k += __popcll(b);
  }
  int jb = 0;
  if (lane == 0) {
    jb = atomicAdd(a.counters, k);
    Outcome o = {0, -1, k, 0, -1, 0};
    a.outc[inst] = o;
  }
  jb = __shfl(jb, 0);
  for (int q = lane; q < k; q += TPB) {
    a.jobs[2 * (jb + q)] = inst;
    a.jobs[2 * (jb + q) + 1] = q;
  }
}

__global__ void track_pick_kernel(TrackArgs a) {
  const int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= a.n_inst) return;
  const int64_t off = (int64_t)inst * a.stride;
  Outcome o = a.outc[inst];
  double best_time = rpp::dinf();
  for (int k = 0; k < o.n_cand; k++) {
    const Record r = a.rec[off + k];
    if (r.ood == 1) o.status |= ST_OOD;
    if (r.ood == 2) o.status |= ST_RAISES;
    if (r.ood == 3) o.status |= ST_OVERFLOW;
    if (better(r.find, r.tlast, best_time)) {   // :1510
      best_time = r.tlast;
      o.winner = k;
      o.len = r.n;
      o.node = a.cand[off + k];
    }
  }
  if (o.status) {   // never a wrong answer: an instance with a refused candidate reports no winner
    o.winner = -1;
    o.len = 0;
    o.node = -1;
  }
  o.flag = o.winner >= 0;
  a.outc[inst] = o;
  if (o.flag) {
    const int j = atomicAdd(a.counters + 2, 1);
    a.jobs[2 * j] = inst;
    a.jobs[2 * j + 1] = o.winner;
  }
}

// Everything of one job after its course is laid out, shared by the two roll kernels: extend_path on lane 0, segment_flags one
// lane per segment, stop_points, the closed_loop_prediction loop (:1307-1372) with the wave-shared np.hypot scan, the running
// collision flag (lane k against obstacle k), judge, and with o7 != nullptr the store of the seven arrays (array q at
// o7 + q * os, at most ocap entries each).  Called by the whole wave with r.ood == 0 after the lanes wrote cx / cy / gcw[0 ..
// total - 1] (not yet synchronised); cx / cy hold total + EXT_MAX points, lsp and s_n are the block's LDS.  ob: this lane has
// an obstacle (obx, oby, its threshold obt).  s: the state the roll-out starts in.
// CHECK_INDEX: ob / obx / oby / obt are not read; mp is the index over the list.  Lane pend_lane(cnt) parks the point of step
// cnt (s is wave-uniform: one select per coordinate), every 64 steps and once behind the loop -- however it ended -- each lane
// asks point_first_hit for its own parked point.  The store pass (o7 != nullptr) writes no record and tests nothing.
template <int CHECK>
__device__ __forceinline__ void roll_course(double* cx, double* cy, double* gcw, signed char* lsp, int32_t* s_n, int total,
                                            double gx, double gy, double gyaw, bool ob, double obx, double oby, double obt,
                                            const Params& P, State s, double* o7, int ocap, int64_t os, Record& r,
                                            const rppo::Map* mp = nullptr) {
  const int lane = threadIdx.x;
  __syncthreads();
  if (lane == 0) *s_n = extend_path(cx, cy, gcw, total, P);
  __syncthreads();
  const int n = *s_n;
  if (n < 0) r.ood = 1;
  if (!r.ood) {
    for (int i = lane; i < n - 1; i += TPB) lsp[i] = (signed char)segment_flags(cx, cy, gcw, i);
    __syncthreads();
    if (lane == 0) stop_points(lsp, n);
    __syncthreads();
    // ---- closed_loop_prediction :1307-1372
    double time = 0.0, vsum = 0.0, last_yaw = 0.0, tlast = 0.0;
    int cnt = 0, hit = 0, ood = 0, reached = 0;
    double ppx = 0.0, ppy = 0.0;   // CHECK_INDEX: the point this lane parks
    auto append = [&](double ai, double di) {
      if (o7 && lane == 0 && cnt < ocap) {
        o7[cnt] = s.x;
        o7[os + cnt] = s.y;
        o7[2 * os + cnt] = rpp::angle_mod_pi(s.yaw);   // :1540
        o7[3 * os + cnt] = s.v;
        o7[4 * os + cnt] = time;
        o7[5 * os + cnt] = ai;
        o7[6 * os + cnt] = di;
      }
      if constexpr (CHECK == CHECK_LINEAR) {
        if (ob) {
          const double dx = obx - s.x, dy = oby - s.y;
          if (dx * dx + dy * dy <= obt) hit = 1;
        }
      } else if (!o7) {
        const bool mine = lane == pend_lane(cnt);
        ppx = mine ? s.x : ppx;
        ppy = mine ? s.y : ppy;
      }
      vsum = vsum + rpp::dabs(s.v);
      last_yaw = s.yaw;
      tlast = time;
      cnt++;
      if constexpr (CHECK == CHECK_INDEX) {
        if (!o7 && pend_flush_due(cnt) && rppo::point_first_hit(*mp, ppx, ppy) >= 0) hit = 1;
      }
    };
    // calc_target_index :1286-1293: the lanes share the np.hypot scan; first minimum, lowest index
    auto scan = [&](double* dis) {
      double best = rpp::dinf();
      int bi = 0x7fffffff;
      for (int i = lane; i < n; i += TPB) {
        const double d = rpp_glibc_hypot(s.x - cx[i], s.y - cy[i]);
        if (d < best) {
          best = d;
          bi = i;
        }
      }
      rppr::wave_argmin(best, bi);
      *dis = best;
      return bi == 0x7fffffff ? 0 : bi;
    };
    append(0.0, 0.0);
    double dis;
    int target_ind = lookahead(cx, cy, n, scan(&dis), P.Lf);
    while (P.T >= time && cnt < MAX_STEPS) {
      const int ind0 = scan(&dis);
      double ai, di;
      if (step(s, target_ind, time, cx, cy, lsp, n, ind0, dis, gx, gy, P, &ai, &di, &ood)) {
        reached = 1;
        break;
      }
      append(ai, di);
      if (ood) break;
    }
    r.n = cnt;
    r.tlast = tlast;
    r.ood = ood ? 1 : 0;
    if constexpr (CHECK == CHECK_INDEX) {   // the final flush: reached, ood, time-out and MAX_STEPS all come through here
      if (!o7 && pend_final(lane, cnt) && rppo::point_first_hit(*mp, ppx, ppy) >= 0) hit = 1;
    }
    const int any_hit = __ballot(hit) != 0ULL;
    judge(&r, reached, rpp::angle_mod_pi(last_yaw), gyaw, vsum, origin_travel(cx, cy, n), any_hit, P);
  }
}

// The course of one candidate node in driving order (generate_final_course :1199-1207 reversed): the start pose, the
// polylines root -> node, the goal pose; shared by track_roll_kernel and goal_roll_kernel (goal_track.hip.h).  Called by the
// whole wave.  Returns the number of points and sets r.ood (3: more than the slab holds, 2: fewer than 3 points, cy[-3]
// :1435 raises IndexError); with r.ood == 0 the points are written (not yet synchronised) to cx / cy -- on entry the slab's
// columns, switched here to the LDS columns lcx / lcy when the extended course fits them -- and the yaws to gcw.
__device__ __forceinline__ int lay_course(const int32_t* parent, const int64_t* poff, const int32_t* plen, int64_t off, int stride,
                                          const double* px, const double* py, const double* pw, int node, const double* start,
                                          double gx, double gy, double gyaw, double* lcx, double* lcy, double* gcw, double*& cx,
                                          double*& cy, Record& r) {
  const int lane = threadIdx.x;
  int total = 2, depth = 0;
  for (int nd = node; parent[off + nd] >= 0 && depth <= stride; nd = parent[off + nd], depth++) total += plen[off + nd];
  if (total + EXT_MAX > SLAB_PTS || depth > stride) r.ood = 3;
  if (total < 3) r.ood = 2;   // cy[-3] :1435 raises IndexError
  if (r.ood) return total;
  if (total + EXT_MAX <= LDS_PTS) {
    cx = lcx;
    cy = lcy;
  }
  int end = total - 1;
  for (int nd = node; parent[off + nd] >= 0; nd = parent[off + nd]) {
    const int pl = plen[off + nd];
    const int64_t po = poff[off + nd];
    end -= pl;
    for (int q = lane; q < pl; q += TPB) {
      cx[end + q] = px[po + q];
      cy[end + q] = py[po + q];
      gcw[end + q] = pw[po + q];
    }
  }
  if (lane == 0) {
    cx[0] = start[0];
    cy[0] = start[1];
    gcw[0] = start[2];
    cx[total - 1] = gx;
    cy[total - 1] = gy;
    gcw[total - 1] = gyaw;
  }
  return total;
}

// store = 0: jobs are (instance, candidate), counters[0] of them, records written; store = 1: jobs are the winners
// (counters[2] of them), arrays written.
// CHECK_INDEX: the handle holds an obstacle map (every instance's rows are empty); mp is that map, a.ox / oy / othr are not read
template <int CHECK>
__global__ __launch_bounds__(TPB) void track_roll_kernel(TrackArgs a, int store, rppo::Map mp) {
  __shared__ double lcx[LDS_PTS], lcy[LDS_PTS];
  __shared__ signed char lsp[SLAB_PTS];
  __shared__ int32_t s_job, s_n;
  const int lane = threadIdx.x;
  const Params P = a.P;
  const int total_jobs = store ? a.counters[2] : a.counters[0];
  double* gcx = a.slab + (int64_t)blockIdx.x * 3 * SLAB_PTS;
  double* gcy = gcx + SLAB_PTS;
  double* gcw = gcy + SLAB_PTS;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_job = atomicAdd(a.counters + 1, 1);
    __syncthreads();
    const int job = s_job;
    if (job >= total_jobs) break;
    const int inst = a.jobs[2 * job], k = a.jobs[2 * job + 1];
    const int64_t off = (int64_t)inst * a.stride;
    const rppk::Inst* I = a.inst + inst;
    const int node = a.cand[off + k];
    Record r = {0, 0, 0, 0, 0.0};
    const double gx = I->goal[0], gy = I->goal[1], gyaw = I->goal[2];
    double *cx = gcx, *cy = gcy;
    const int total = lay_course(a.parent, a.poff, a.plen, off, (int)a.stride, a.pool[3 * inst], a.pool[3 * inst + 1], a.pool[3 * inst + 2],
                                 node, I->start, gx, gy, gyaw, lcx, lcy, gcw, cx, cy, r);
    if (!r.ood) {
      int m = 0;
      double obx = 0.0, oby = 0.0, obt = -1.0;
      if constexpr (CHECK == CHECK_LINEAR) {
        m = I->obs_m;
        if (lane < m) {
          obx = a.ox[I->obs_base + lane];
          oby = a.oy[I->obs_base + lane];
          obt = a.othr[I->obs_base + lane];
        }
      }
      double* o7 = nullptr;
      int ocap = 0;
      if (store) {
        ocap = a.outc[inst].len;
        o7 = a.out + a.out_off[inst];
      }
      const int64_t os = (int64_t)ocap + 1;
      const State s0 = {-0.0, -0.0, 0.0, 0.0};
      roll_course<CHECK>(cx, cy, gcw, lsp, &s_n, total, gx, gy, gyaw, lane < m, obx, oby, obt, P, s0, o7, ocap, os, r, &mp);
      if (o7 && lane == 0 && r.find && r.n == ocap) {   // :1519-1521: the goal pose behind x, y, yaw only
        o7[r.n] = gx;
        o7[os + r.n] = gy;
        o7[2 * os + r.n] = gyaw;
      }
    }
    if (!store && lane == 0) a.rec[off + k] = r;
  }
}

// ---- courses given as data (rrtx_tracker_run): the same roll-out on CSR courses of the caller ----------------------------
struct CourseArgs {
  int64_t n;                   // courses
  const int64_t* off;          // [n + 1] CSR into x / y / yaw, driving order
  const double *x, *y, *yaw;
  const double* per_course;    // nullptr, or [n][3]: target_speed, yaw_th, invalid_travel_ratio
  const double* start;         // nullptr, or [n][4]: x, y, yaw, v
  const double *ox, *oy;       // obstacle rows
  const double* othr;          // (radius + robot_radius) ** 2: row obs index + course * thr_stride
  const int64_t* obs_off;      // nullptr (every course tests rows 0 .. m_shared - 1), or [n + 1] CSR into the rows
  int64_t thr_stride;          // m_shared when one list is shared and robot_radius is per course, else 0
  int32_t m_shared;
  Params P;
  Record* rec;                 // [n]
  int32_t* counter;            // queue head
  double* slab;                // [block][3][SLAB_PTS]
  double* out;                 // store = 1: seven arrays of out_total doubles each, course i at arr_off[i], rec[i].n entries
  const int64_t* arr_off;
  int64_t out_total;
};

// store = 0: one Record per course; store = 1: every course whose record has ood == 0 is rolled out again and its seven
// arrays are stored.  A course of fewer than 3 points reports ood = 2, one of more than SLAB_PTS - EXT_MAX points ood = 3.
// CHECK_INDEX: mp is the index over the shared list; a.ox / oy / othr / obs_off are not read.
template <int CHECK>
__global__ __launch_bounds__(TPB) void track_courses_kernel(CourseArgs a, int store, rppo::Map mp) {
  __shared__ double lcx[LDS_PTS], lcy[LDS_PTS];
  __shared__ signed char lsp[SLAB_PTS];
  __shared__ int32_t s_job, s_n;
  const int lane = threadIdx.x;
  double* gcx = a.slab + (int64_t)blockIdx.x * 3 * SLAB_PTS;
  double* gcy = gcx + SLAB_PTS;
  double* gcw = gcy + SLAB_PTS;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_job = atomicAdd(a.counter, 1);
    __syncthreads();
    const int64_t c = s_job;
    if (c >= a.n) break;
    if (store && a.rec[c].ood) continue;
    Record r = {0, 0, 0, 0, 0.0};
    const int64_t b = a.off[c], len = a.off[c + 1] - b;
    if (len + EXT_MAX > SLAB_PTS) r.ood = 3;
    if (len < 3) r.ood = 2;   // cy[-3] :1435 raises IndexError
    if (!r.ood) {
      const int total = (int)len;
      double *cx = gcx, *cy = gcy;
      if (total + EXT_MAX <= LDS_PTS) {
        cx = lcx;
        cy = lcy;
      }
      for (int q = lane; q < total; q += TPB) {
        cx[q] = a.x[b + q];
        cy[q] = a.y[b + q];
        gcw[q] = a.yaw[b + q];
      }
      const double gx = a.x[b + total - 1], gy = a.y[b + total - 1], gyaw = a.yaw[b + total - 1];   // :1531
      Params P = a.P;
      if (a.per_course) {
        P.target_speed = a.per_course[3 * c];
        P.yaw_th = a.per_course[3 * c + 1];
        P.invalid_travel_ratio = a.per_course[3 * c + 2];
      }
      State s0 = {-0.0, -0.0, 0.0, 0.0};   // :1309
      if (a.start) {
        s0.x = a.start[4 * c];
        s0.y = a.start[4 * c + 1];
        s0.yaw = a.start[4 * c + 2];
        s0.v = a.start[4 * c + 3];
      }
      int m = 0;
      double obx = 0.0, oby = 0.0, obt = -1.0;
      if constexpr (CHECK == CHECK_LINEAR) {
        const int64_t ob = a.obs_off ? a.obs_off[c] : 0;
        m = a.obs_off ? (int)(a.obs_off[c + 1] - ob) : a.m_shared;
        if (lane < m) {
          obx = a.ox[ob + lane];
          oby = a.oy[ob + lane];
          obt = a.othr[ob + c * a.thr_stride + lane];
        }
      }
      double* o7 = nullptr;
      int ocap = 0;
      if (store) {
        ocap = a.rec[c].n;
        o7 = a.out + a.arr_off[c];
      }
      roll_course<CHECK>(cx, cy, gcw, lsp, &s_n, total, gx, gy, gyaw, lane < m, obx, oby, obt, P, s0, o7, ocap, a.out_total, r, &mp);
    }
    if (!store && lane == 0) a.rec[c] = r;
  }
}

// ---- courses read in place from a producer's device buffers (rrtx_tracker_run_from) -----------------------------------------
struct SourceArgs {
  CourseArgs c;            // off / x / y / yaw point into the producer's buffers; everything else is the tracker's
  int32_t select;          // SEL_*
  const int32_t* hit;      // SEL_FREE: the producer's hits, [n]
  const uint8_t* mask;     // SEL_MASK: [n]
  double* goal;            // [n][3]: the last point of every complete course (NaN otherwise), store = 0
  int64_t group;           // 0, or the courses per group
  int32_t* winner;         // [n / group]: track_group_pick_kernel's answer, a course index or -1
  double* wgoal;           // [n / group][3]: the winner's last point (NaN without one)
  int32_t winners_only;    // store = 1: only the group winners are rolled out again
};

// track_courses_kernel on a producer's points: the same queue, LDS / slab split, roll_course and store pass.  What differs: a
// course the selection leaves out reports ood = 5 and its offsets and points are not read; while a course is copied into
// LDS / the slab every x, y and yaw is tested for finiteness (one wave-wide OR, no second pass over the points), and a
// course with a non-finite component reports ood = 4.  The host path refuses such a batch whole; here the host never sees
// the points.  CHECK as track_courses_kernel.
template <int CHECK>
__global__ __launch_bounds__(TPB) void track_source_kernel(SourceArgs s, int store, rppo::Map mp) {
  __shared__ double lcx[LDS_PTS], lcy[LDS_PTS];
  __shared__ signed char lsp[SLAB_PTS];
  __shared__ int32_t s_job, s_n;
  const CourseArgs& a = s.c;
  const int lane = threadIdx.x;
  double* gcx = a.slab + (int64_t)blockIdx.x * 3 * SLAB_PTS;
  double* gcy = gcx + SLAB_PTS;
  double* gcw = gcy + SLAB_PTS;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_job = atomicAdd(a.counter, 1);
    __syncthreads();
    const int64_t c = s_job;
    if (c >= a.n) break;
    if (store && a.rec[c].ood) continue;
    if (store && s.winners_only && s.winner[c / s.group] != (int32_t)c) continue;
    Record r = {0, 0, 0, 0, 0.0};
    const bool sel = course_selected(s.select, s.select == SEL_FREE ? s.hit[c] : 0, s.select == SEL_MASK ? s.mask[c] : 0);
    int64_t b = 0, len = 0;
    if (sel) {
      b = a.off[c];
      len = a.off[c + 1] - b;
    }
    constexpr int64_t CAP = SLAB_PTS - EXT_MAX;
    r.ood = course_ood(sel, len, CAP, false);
    const int total = (int)len;
    double *cx = gcx, *cy = gcy;
    if (!r.ood) {
      if (total + EXT_MAX <= LDS_PTS) {
        cx = lcx;
        cy = lcy;
      }
      bool bad = false;
      for (int q = lane; q < total; q += TPB) {
        const double vx = a.x[b + q], vy = a.y[b + q], vw = a.yaw[b + q];
        bad = bad || not_finite(vx) || not_finite(vy) || not_finite(vw);
        cx[q] = vx;
        cy[q] = vy;
        gcw[q] = vw;
      }
      r.ood = course_ood(sel, len, CAP, __ballot(bad) != 0ULL);
    }
    double gx = rpp::b2d(0x7ff8000000000000ULL), gy = gx, gyaw = gx;
    if (!r.ood) {
      gx = a.x[b + total - 1], gy = a.y[b + total - 1], gyaw = a.yaw[b + total - 1];   // :1531
      Params P = a.P;
      if (a.per_course) {
        P.target_speed = a.per_course[3 * c];
        P.yaw_th = a.per_course[3 * c + 1];
        P.invalid_travel_ratio = a.per_course[3 * c + 2];
      }
      State s0 = {-0.0, -0.0, 0.0, 0.0};   // :1309
      if (a.start) {
        s0.x = a.start[4 * c];
        s0.y = a.start[4 * c + 1];
        s0.yaw = a.start[4 * c + 2];
        s0.v = a.start[4 * c + 3];
      }
      int m = 0;
      double obx = 0.0, oby = 0.0, obt = -1.0;
      if constexpr (CHECK == CHECK_LINEAR) {
        const int64_t ob = a.obs_off ? a.obs_off[c] : 0;
        m = a.obs_off ? (int)(a.obs_off[c + 1] - ob) : a.m_shared;
        if (lane < m) {
          obx = a.ox[ob + lane];
          oby = a.oy[ob + lane];
          obt = a.othr[ob + c * a.thr_stride + lane];
        }
      }
      double* o7 = nullptr;
      int ocap = 0;
      if (store) {
        ocap = a.rec[c].n;
        o7 = a.out + a.arr_off[c];
      }
      roll_course<CHECK>(cx, cy, gcw, lsp, &s_n, total, gx, gy, gyaw, lane < m, obx, oby, obt, P, s0, o7, ocap, a.out_total, r, &mp);
    }
    if (!store && lane == 0) {
      a.rec[c] = r;
      s.goal[3 * c] = gx;
      s.goal[3 * c + 1] = gy;
      s.goal[3 * c + 2] = gyaw;
    }
  }
}

// One thread per group of s.group consecutive courses: group_pick over its records, and the winner's last point
__global__ void track_group_pick_kernel(SourceArgs s) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= s.c.n / s.group) return;
  const int64_t k = group_pick(s.c.rec + j * s.group, s.group);
  const int64_t w = k < 0 ? -1 : j * s.group + k;
  s.winner[j] = (int32_t)w;
  for (int q = 0; q < 3; q++) s.wgoal[3 * j + q] = w < 0 ? rpp::b2d(0x7ff8000000000000ULL) : s.goal[3 * w + q];
}

}  // namespace rppt

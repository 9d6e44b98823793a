// goal_track.hip.h -- rrtx_track_goals: rrt_10's closed-loop stage on the planned Reeds-Shepp trees for MANY goals (gfx950).
// Reference: rrt_10 ClosedLoopRRTStar.planning :1488-1493 with self.end = Node(*g): get_goal_indexes :1566-1582,
// search_best_feasible_path :1495-1524, check_tracking_path_is_feasible :1526-1564; the scalar rules are csrc/rpp_goaltrack.h,
// the roll-out is rrt_track.hip.h's roll_course, the course layout its lay_course -- one text each with rrtx_track_planned.
//
// A query is an (instance, goal) pair, row major (rpp_goalq.h's map).  Plain launches on the handle's stream, no grid barrier:
//   goal_cand_kernel(fill = 0)  one wave per query (resident waves loop over the queries): lane l tests nodes l, l + 64, ... of
//                               the query's instance against the query's goal; writes the candidate count (COUNT_NO_TREE for a
//                               tree that did not finish)
//   -- the host takes the exclusive sum of the counts (candidate_offsets) --
//   goal_cand_kernel(fill = 1)  the same scan; ballot / popcount compaction stores the node indices in ascending order at
//                               cand[cand_off[q] + k] and the job's query at job_query[cand_off[q] + k]
//   goal_roll_kernel(store = 0) persistent one-wave workgroups, jobs from an atomic counter (roll-outs differ 10x in length, the
//                               candidates per query 0 .. 40): job j is candidate j; lays the course out with the start pose in
//                               front and the QUERY'S goal behind, rolls it out against the instance's obstacle rows, writes rec[j]
//   goal_pick_kernel            one thread per query: rppgt::pick over rec[cand_off[q] .. cand_off[q + 1]); winners are appended
//                               to the store pass's job list
//   -- the host takes the exclusive sum of len + 1 over the flagged queries (array_offsets) --
//   goal_roll_kernel(store = 1) the winners again, their seven arrays stored with the goal pose behind x, y, yaw: memory is
//                               bounded by the winners' lengths, not by 2 002 x 7 doubles per candidate
// Capacities are track_roll_kernel's (LDS_PTS, SLAB_PTS, 64 obstacles per instance, or the handle's obstacle map of any number
// of circles); at most 2^24 candidates per call (host check).
#pragma once
#include "rpp_goaltrack.h"
#include "rrt_track.hip.h"

namespace rppgt {

constexpr int TPB = rppt::TPB;

struct GoalTrackArgs {
  const rppk::Inst* inst;
  const double *x, *y, *yaw;
  const int32_t* parent;
  const int64_t* poff;
  const int32_t* plen;
  int64_t stride;
  const double* const* pool;   // [inst][3]: this instance's polyline pool (x, y, yaw)
  const double *ox, *oy, *othr;
  rppt::Params P;
  int32_t n_inst, n_goals, per_instance;
  int64_t nq;
  const double* goals;         // (n_goals, 3) shared, or (n_inst, n_goals, 3)
  int32_t* count;              // [nq]
  const int64_t* cand_off;     // [nq + 1]
  int32_t* cand;               // [candidates]: node indices
  int32_t* job_query;          // [candidates]: the query of candidate j
  rppt::Record* rec;           // [candidates]
  int32_t n_jobs;              // candidates in all
  int32_t* counters;           // 0: queue head of the roll launches, 1: winners listed
  int32_t* win_query;          // [nq]: the queries with a winner, in no particular order
  double* slab;                // [block][3][SLAB_PTS]
  Outcome* outc;               // [nq]
  double* out;                 // seven planes of out_total doubles; query q owns len + 1 entries at arr_off[q] of each
  const int64_t* arr_off;      // [nq + 1]
  int64_t out_total;
};

__global__ __launch_bounds__(TPB) void goal_cand_kernel(GoalTrackArgs a, int fill) {
  const int lane = threadIdx.x;
  for (int64_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
    const int inst = rppq::inst_of(q, a.n_goals);
    const rppk::Inst* I = a.inst + inst;
    if (!rppq::tree_ok(I->status)) {
      if (!fill && lane == 0) a.count[q] = COUNT_NO_TREE;
      continue;
    }
    const int64_t off = (int64_t)inst * a.stride;
    const double* g = a.goals + 3 * rppq::goal_row(q, a.n_goals, a.per_instance);
    const double gx = g[0], gy = g[1], gyaw = g[2];
    const int n = I->n < (int)a.stride ? I->n : (int)a.stride;
    const int64_t base_out = fill ? a.cand_off[q] : 0;
    const int room = fill ? (int)(a.cand_off[q + 1] - base_out) : 0;
    int k = 0;
    for (int base = 0; base < n; base += TPB) {
      const int i = base + lane;
      const bool c = i < n && goal_candidate(a.x[off + i], a.y[off + i], a.yaw[off + i], gx, gy, gyaw, a.P);
      const unsigned long long b = __ballot(c);
      if (fill && c) {
        const int pos = k + __popcll(b & ((1ULL << lane) - 1ULL));
        if (pos < room) {   // the same scan as the count pass: always true; never a store outside the query's slots
          a.cand[base_out + pos] = i;
          a.job_query[base_out + pos] = (int32_t)q;
        }
      }
      k += __popcll(b);
    }
    if (!fill && lane == 0) a.count[q] = k;
  }
}

// store = 0: job j is candidate j (n_jobs of them), rec[j] written; store = 1: job j is query win_query[j] (counters[1] of
// them), the winner's arrays written.
// CHECK_INDEX: the handle holds an obstacle map (every instance's rows are empty); mp is that map, a.ox / oy / othr are not read
template <int CHECK>
__global__ __launch_bounds__(TPB) void goal_roll_kernel(GoalTrackArgs a, int store, rppo::Map mp) {
  __shared__ double lcx[rppt::LDS_PTS], lcy[rppt::LDS_PTS];
  __shared__ signed char lsp[rppt::SLAB_PTS];
  __shared__ int32_t s_job, s_n;
  const int lane = threadIdx.x;
  const rppt::Params P = a.P;
  const int total_jobs = store ? a.counters[1] : a.n_jobs;
  double* gcx = a.slab + (int64_t)blockIdx.x * 3 * rppt::SLAB_PTS;
  double* gcy = gcx + rppt::SLAB_PTS;
  double* gcw = gcy + rppt::SLAB_PTS;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_job = atomicAdd(a.counters, 1);
    __syncthreads();
    const int job = s_job;
    if (job >= total_jobs) break;
    int64_t q, j;   // the query, and its candidate's slot
    if (store) {
      q = a.win_query[job];
      j = a.cand_off[q] + a.outc[q].winner;
    } else {
      j = job;
      q = a.job_query[j];
    }
    const int inst = rppq::inst_of(q, a.n_goals);
    const int64_t off = (int64_t)inst * a.stride;
    const rppk::Inst* I = a.inst + inst;
    const int node = a.cand[j];
    const double* g = a.goals + 3 * rppq::goal_row(q, a.n_goals, a.per_instance);
    const double gx = g[0], gy = g[1], gyaw = g[2];
    rppt::Record r = {0, 0, 0, 0, 0.0};
    double *cx = gcx, *cy = gcy;
    const int total = rppt::lay_course(a.parent, a.poff, a.plen, off, (int)a.stride, a.pool[3 * inst], a.pool[3 * inst + 1],
                                       a.pool[3 * inst + 2], node, I->start, gx, gy, gyaw, lcx, lcy, gcw, cx, cy, r);
    if (!r.ood) {
      int m = 0;
      double obx = 0.0, oby = 0.0, obt = -1.0;
      if constexpr (CHECK == rppt::CHECK_LINEAR) {
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
        ocap = a.outc[q].len;
        o7 = a.out + a.arr_off[q];
      }
      const rppt::State s0 = {-0.0, -0.0, 0.0, 0.0};   // :1309
      rppt::roll_course<CHECK>(cx, cy, gcw, lsp, &s_n, total, gx, gy, gyaw, lane < m, obx, oby, obt, P, s0, o7, ocap, a.out_total, r, &mp);
      if (o7 && lane == 0 && r.find && r.n == ocap) {   // :1519-1521: the goal pose behind x, y, yaw; the other four end in NaN
        const double nan = rpp::b2d(0x7ff8000000000000ULL);
        o7[r.n] = gx;
        o7[a.out_total + r.n] = gy;
        o7[2 * a.out_total + r.n] = gyaw;
        for (int c = 3; c < 7; c++) o7[c * a.out_total + r.n] = nan;
      }
    }
    if (!store && lane == 0) a.rec[j] = r;
  }
}

__global__ void goal_pick_kernel(GoalTrackArgs a) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.nq) return;
  const int64_t b = a.cand_off[q], n = a.cand_off[q + 1] - b;
  const Outcome o = pick(a.rec + b, a.cand + b, n, a.count[q] == COUNT_NO_TREE);
  a.outc[q] = o;
  if (o.flag) a.win_query[atomicAdd(a.counters + 1, 1)] = (int32_t)q;
}

}  // namespace rppgt

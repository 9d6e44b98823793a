// goal_query.hip.h -- rrtx_query_goals: the best path from each instance's start to MANY goals, read off the finished
// trees of a planned handle (rules: rpp_goalq.h).  Queries are (instance, goal) pairs in row-major order.
//   goal_solve_point_kernel   rrt_04: one 256-thread workgroup per query, workgroups loop over the queries.  The query is
//                             best_goal_node's composition -- scan_hits, exact_dedup, eval_edges, first_min of
//                             rrt_kernels.hip.h, the same device functions -- with the goal taken from the goal table and
//                             the hit list in the WORKGROUP's own scratch row, so that many queries of one instance run
//                             at once: nothing of Inst is written, Ctx::hits is not touched.
//   goal_solve_pose_kernel    rrt_05 / rrt_06: one wave per query; every lane tests nodes lane, lane + 64, .. against both
//                             thresholds with the exact hypot of the planners' own goal search and keeps its (cost, index)
//                             minimum; one butterfly merges the lanes.
//   goal_count_kernel         one lane per query: the points of its course (0 without an answer)
//   goal_gather_kernel        one wave per query: the course to offsets[q] .., in the requested order
// Capacity: a point query keeps its distinct candidates in LDS (rppk::NU_MAX = 512).  A query with more is answered
// ST_OVERFLOW (no node), never with a node picked from a part of the candidates.
#pragma once
#include <hip/hip_runtime.h>

#include "course_gather.hip.h"
#include "rpp_goalq.h"
#include "rrt_dubins.hip.h"
#include "rrt_kernels.hip.h"

namespace rppq {

constexpr int TPB_POINT = rppk::TPB, TPB_WAVE = 64;

struct QueryArgs {
  rppk::Ctx c;              // the handle's launch context, read only: tree columns, obstacle table, steer parameters
  int32_t n_inst, n_goals, per_instance, kind;
  const double* goals;      // rows (x, y, yaw): (n_goals, 3) or (n_inst, n_goals, 3)
  double xy_th, yaw_th;     // pose trees
  const double* yaw;        // pose trees: [inst][stride]
  int32_t* scratch;         // point trees: one row of c.stride hit slots per workgroup of the solve launch
  Record* rec;              // [query]
  // courses
  int32_t ncol, order;
  const int32_t* plen;
  const int64_t* poff;
  const double* const* pool;   // [instance][3]
  const int64_t* pool_cap;     // [instance]
  int32_t* count;              // [query]
  const int64_t* off;          // [query + 1]
  double *ox, *oy, *oyaw;
};

__device__ inline int64_t n_queries(const QueryArgs& a) { return (int64_t)a.n_inst * a.n_goals; }
__device__ inline int64_t nodes_of(const QueryArgs& a, int i) {
  const int64_t n = a.c.inst[i].n;
  return n < 0 ? 0 : (n < a.c.stride ? n : a.c.stride);
}

__global__ __launch_bounds__(TPB_POINT) void goal_solve_point_kernel(QueryArgs a) {
  __shared__ rppk::Sh sh;
  const rppk::Ctx& c = a.c;
  const int tid = threadIdx.x;
  int32_t* hits = a.scratch + (int64_t)blockIdx.x * c.stride;
  const int64_t nq = n_queries(a);
  int staged = -1, om = 0;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {   // block-uniform
    const int i = inst_of(q, a.n_goals);
    const rppk::Inst* I = c.inst + i;
    if (!tree_ok(I->status)) {
      if (tid == 0) a.rec[q] = empty_record(ST_NO_TREE, 0);
      continue;
    }
    __syncthreads();   // the previous query's reads of sh are over
    if (staged != i) {
      const int ob = __builtin_amdgcn_readfirstlane(I->obs_base);
      om = __builtin_amdgcn_readfirstlane(I->obs_m);
      om = om < 0 ? 0 : (om > rppk::MAX_OBS ? rppk::MAX_OBS : om);
      for (int k = tid; k < om; k += TPB_POINT) {
        sh.ox[k] = c.ox[ob + k];
        sh.oy[k] = c.oy[ob + k];
        sh.othr[k] = c.othr[ob + k];
      }
      staged = i;
    }
    if (tid == 0) {
      sh.overflow = 0;
      sh.flag = 0;
    }
    __syncthreads();
    const int64_t tree = (int64_t)i * c.stride;
    const double *x = c.x + tree, *y = c.y + tree, *cost = c.cost + tree;
    const int n = (int)nodes_of(a, i);
    const double* g = a.goals + 3 * goal_row(q, a.n_goals, a.per_instance);
    const double gx = g[0], gy = g[1];
    // best_goal_node (rrt_kernels.hip.h) from here on, with (gx, gy) for Inst::goal
    const double thr = c.expand_dis * c.expand_dis * (1.0 + rppk::FILTER_EPS);
    const int kraw = rppk::scan_hits(x, y, n, gx, gy, thr, hits, sh);
    rppk::exact_dedup(x, y, gx, gy, c.expand_dis, 1, hits, kraw, sh);
    const int nu = sh.nu;
    if (sh.overflow) {   // block-uniform: exact_dedup ended on a barrier
      if (tid == 0) a.rec[q] = empty_record(ST_OVERFLOW, nu);
      continue;
    }
    if (nu == 0) {
      if (tid == 0) a.rec[q] = empty_record(ST_NONE, 0);
      continue;
    }
    rppk::eval_edges(c, om, x, y, nu, 0, gx, gy, sh);
    int safe = 0;
    for (int e = tid; e < nu; e += TPB_POINT) {
      const int s = sh.usafe[e];
      safe += s ? 1 : 0;
      sh.uaux[e] = s ? cost[sh.uidx[e]] + sh.uval[e] : rpp::dinf();   // cost + calc_dist_to_goal :1303-1305
    }
    if (safe) atomicAdd(&sh.flag, safe);
    __syncthreads();
    double mn;
    int sel;
    rppk::first_min(nu, sh, mn, sel);   // ends on a barrier
    if (tid == 0) {
      Best b = best_none();
      if (sel >= 0 && sel < nu) offer(b, mn, sh.uidx[sel]);
      a.rec[q] = make_record(KIND_POINT, b, nu, sh.flag);
    }
  }
}

__global__ __launch_bounds__(TPB_WAVE) void goal_solve_pose_kernel(QueryArgs a) {
  const rppk::Ctx& c = a.c;
  const int lane = threadIdx.x;
  const int64_t nq = n_queries(a);
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const int i = inst_of(q, a.n_goals);
    if (!tree_ok(c.inst[i].status)) {
      if (lane == 0) a.rec[q] = empty_record(ST_NO_TREE, 0);
      continue;
    }
    const int64_t tree = (int64_t)i * c.stride;
    const double *x = c.x + tree, *y = c.y + tree, *cost = c.cost + tree, *yaw = a.yaw + tree;
    const int n = (int)nodes_of(a, i);
    const double* g = a.goals + 3 * goal_row(q, a.n_goals, a.per_instance);
    const double gx = g[0], gy = g[1], gyaw = g[2];
    Best b = best_none();
    int near = 0;
    for (int k = lane; k < n; k += TPB_WAVE) {
      if (rpp::py_hypot(x[k] - gx, y[k] - gy) <= a.xy_th && rpp::dabs(yaw[k] - gyaw) <= a.yaw_th) {
        near++;
        offer(b, cost[k], k);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      Best ob;
      ob.key = __shfl_xor(b.key, o);
      ob.idx = __shfl_xor(b.idx, o);
      merge(b, ob);
      near += __shfl_xor(near, o);
    }
    if (lane == 0) a.rec[q] = make_record(KIND_POSE, b, near, 0);
  }
}

__device__ inline rppc::Chain chain_of(const QueryArgs& a, int i) {
  rppc::Chain ch;
  const int64_t base = (int64_t)i * a.c.stride;
  ch.parent = a.c.parent + base;
  ch.plen = a.plen + base;
  ch.poff = a.poff + base;
  ch.n_nodes = nodes_of(a, i);
  ch.pool_cap = a.pool_cap[i];
  return ch;
}

__global__ __launch_bounds__(256) void goal_count_kernel(QueryArgs a) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_queries(a)) return;
  const int i = inst_of(q, a.n_goals);
  const int32_t node = a.rec[q].status == ST_OK ? a.rec[q].node : -1;
  int64_t n = 0;
  if (node >= 0)
    n = a.kind == KIND_POSE ? pose_points(chain_of(a, i), node)
                            : point_count(a.c.parent + (int64_t)i * a.c.stride, nodes_of(a, i), node);
  a.count[q] = (int32_t)(n > 0x7fffffffLL ? 0x7fffffffLL : n);
}

__global__ __launch_bounds__(TPB_WAVE) void goal_gather_kernel(QueryArgs a) {
  __shared__ rppc::Round round;
  const int lane = threadIdx.x;
  const int64_t nq = n_queries(a);
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {   // block-uniform
    const int64_t o = a.off[q], total = a.off[q + 1] - o;
    const int32_t node = a.rec[q].node;
    if (total <= 0 || node < 0) continue;
    const int i = inst_of(q, a.n_goals);
    const double* g = a.goals + 3 * goal_row(q, a.n_goals, a.per_instance);
    if (a.kind == KIND_POINT) {
      const int64_t base = (int64_t)i * a.c.stride;
      if (lane == 0)
        rppc::trunc_walk(a.c.x + base, a.c.y + base, a.c.parent + base, nodes_of(a, i), node, g, a.ox + o, a.oy + o, a.order,
                         total);
      continue;
    }
    const rppc::Chain ch = chain_of(a, i);
    const double* src[3] = {a.pool[3 * i], a.pool[3 * i + 1], a.pool[3 * i + 2]};
    double* dst[3] = {a.ox + o, a.oy + o, a.ncol == 3 ? a.oyaw + o : nullptr};
    rppc::pose_course(ch, src, dst, a.ncol, a.order, total, g, a.c.inst[i].start, node, round, lane);
  }
}

}  // namespace rppq

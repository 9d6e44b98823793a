// course_gather.hip.h -- rrtx_gather_courses: every planned (or smoothed) course of a handle into one CSR result on the
// device, in two launches with the host's exclusive sum between them (the pattern of spline_run and tracker_run_from).
//   course_count_kernel   one lane per instance: its point count (0 without a path)
//   course_gather_kernel  one one-wave workgroup per instance: x, y (and yaw) to offsets[i] .., in the requested order
// The index arithmetic is rpp_course.h's; nothing here computes on a coordinate.
#pragma once
#include <hip/hip_runtime.h>

#include "rpp_course.h"
#include "rrt_kernels.hip.h"

namespace rppc {

constexpr int TPB = 64;
constexpr int SRC_FLAT = 0;   // rows (x, y) in a per-instance buffer, the count in an int32 column
constexpr int SRC_POSE = 1;   // the polyline pool of the pose planners

struct GatherArgs {
  int32_t n_inst, src, order, ncol;   // ncol: 2, or 3 with the yaw column (SRC_POSE of RRTX_ALGO_RS)
  const rppk::Inst* inst;             // status, goal / start, goal_node, n
  int32_t need_path;                  // 1: an instance without RRTX_ST_PATH owns no points (planned courses)
  // SRC_FLAT
  const double* flat_xy;              // instance i: flat_xy + i * flat_stride doubles
  int64_t flat_stride;
  const int32_t* flat_n;              // instance i: flat_n[i * flat_n_stride]
  int64_t flat_n_stride;
  int64_t flat_cap;                   // rows of a buffer: a larger count is RRTX_ST_PATH_TRUNC (walk) or clamped
  int32_t walk_trunc;                 // 1: a count above flat_cap is walked up x / y / parent
  const double *x, *y;
  // both
  const int32_t* parent;
  int64_t stride;                     // nodes per instance of x / y / parent / plen / poff
  // SRC_POSE
  const int32_t* plen;
  const int64_t* poff;
  const double* const* pool;          // [instance][3]: the instance's slab of the x, y and yaw pool
  const int64_t* pool_cap;            // [instance]
  // results
  int32_t* count;                     // [instance], written by the count kernel
  const int64_t* off;                 // [instance + 1], read by the gather kernel
  double *ox, *oy, *oyaw;
};

__device__ inline Chain chain_of(const GatherArgs& a, int i) {
  Chain c;
  const int64_t base = (int64_t)i * a.stride;
  c.parent = a.parent + base;
  c.plen = a.plen + base;
  c.poff = a.poff + base;
  const int64_t n = a.inst[i].n;
  c.n_nodes = n < a.stride ? n : a.stride;
  c.pool_cap = a.pool_cap[i];
  return c;
}

// the point count of instance i of a flat source, as both kernels see it
__device__ inline int64_t flat_count(const GatherArgs& a, int i, bool* walk) {
  int64_t n = a.flat_n[(int64_t)i * a.flat_n_stride];
  *walk = false;
  if (n < 0) n = 0;
  if (n > a.flat_cap) {
    if (a.walk_trunc && (a.inst[i].status & RRTX_ST_PATH_TRUNC)) *walk = true;
    else n = a.flat_cap;
  }
  return n;
}

__global__ __launch_bounds__(256) void course_count_kernel(GatherArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_inst) return;
  int64_t n = 0;
  if (!a.need_path || (a.inst[i].status & RRTX_ST_PATH)) {
    if (a.src == SRC_POSE) {
      n = pose_count(chain_of(a, i), a.inst[i].goal_node);
    } else {
      bool walk;
      n = flat_count(a, i, &walk);
    }
  }
  a.count[i] = (int32_t)(n > 0x7fffffffLL ? 0x7fffffffLL : n);
}

// One pose course by one wave: the two end rows, then the chain from `goal_node` in rounds of ROUND nodes listed through
// `round` (LDS) and copied with all lanes.  Block-uniform arguments.
__device__ inline void pose_course(const Chain& c, const double* const* src, double* const* dst, int ncol, int order,
                                   int64_t total, const double* goal, const double* start, int32_t goal_node, Round& round,
                                   int lane) {
  if (lane == 0) pose_ends(goal, start, dst, ncol, order, total);
  int32_t nd = goal_node;
  int64_t k = 1, steps = 0;
  while (nd >= 0) {   // block-uniform: every lane reads the same round
    if (lane == 0) pose_round_fill(c, nd, k, steps, round);
    __syncthreads();
    pose_round_copy(round, src, dst, ncol, order, total, lane, TPB);
    nd = round.next;
    k = round.k_next;
    steps = round.steps;
    __syncthreads();   // the next fill overwrites the round
  }
}

__global__ __launch_bounds__(TPB) void course_gather_kernel(GatherArgs a) {
  __shared__ Round round;
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= a.n_inst) return;
  const int64_t o = a.off[i], total = a.off[i + 1] - o;
  if (total <= 0) return;   // block-uniform
  if (a.src == SRC_FLAT) {
    bool walk;
    const int64_t n = flat_count(a, i, &walk);
    if (n != total) return;   // the count kernel decided the rows this instance owns
    if (walk) {
      const int64_t base = (int64_t)i * a.stride, nn = a.inst[i].n;
      if (lane == 0)
        trunc_walk(a.x + base, a.y + base, a.parent + base, nn < a.stride ? nn : a.stride, a.inst[i].goal_node, a.inst[i].goal,
                   a.ox + o, a.oy + o, a.order, total);
    } else {
      flat_copy(a.flat_xy + (int64_t)i * a.flat_stride, a.ox + o, a.oy + o, a.order, total, lane, TPB);
    }
    return;
  }
  const Chain c = chain_of(a, i);
  const double* src[3] = {a.pool[3 * i], a.pool[3 * i + 1], a.pool[3 * i + 2]};
  double* dst[3] = {a.ox + o, a.oy + o, a.ncol == 3 ? a.oyaw + o : nullptr};
  pose_course(c, src, dst, a.ncol, a.order, total, a.inst[i].goal, a.inst[i].start, a.inst[i].goal_node, round, lane);
}

}  // namespace rppc

// rpp_course.h -- where the k-th point of a planned course comes from: the index arithmetic of rrtx_gather_courses, shared
// by course_gather.hip.h (one wave per instance) and tests/native/course_host_check.cpp (the same routines, lane after lane).
// A course is stated in planning order (goal -> start, as planning() returns it); RRTX_ORDER_DRIVING writes the same rows
// reversed.  Two sources:
//   point planners  the instance's path buffer, rows (x, y); when the plan marked it RRTX_ST_PATH_TRUNC the buffer holds
//                   the first path_cap rows only and the course is walked: [goal] + the nodes up the parent chain
//                   (generate_final_course, rrt_04:1117-1125)
//   pose planners   [goal] + the edge polyline of every node up the parent chain, each reversed, + [start]
//                   (rrt_05:1512-1521, rrt_06:1643-1651); the polylines live in the instance's slab of the pool
// No arithmetic on a coordinate anywhere: every double is copied.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RPPC_HD __host__ __device__ inline
#else
#define RPPC_HD inline
#endif

namespace rppc {

constexpr int ORDER_PLANNING = 0, ORDER_DRIVING = 1;
constexpr int ROUND = 64;   // chain nodes listed per round (one per lane of the wave that copies them)

// the row of a course of `total` points that its planning-order point k is written to
RPPC_HD int64_t dst_row(int order, int64_t total, int64_t k) { return order == ORDER_DRIVING ? total - 1 - k : k; }

// ---- pose planners ---------------------------------------------------------------------------------------------------
// One instance's tree columns (node index -> parent, polyline length and offset into the slab) and its slab
struct Chain {
  const int32_t* parent;
  const int32_t* plen;
  const int64_t* poff;
  int64_t n_nodes;    // nodes of the tree: a node index outside [0, n_nodes) ends a walk, and no walk takes more steps
  int64_t pool_cap;   // points of the slab: a polyline that does not lie inside it is skipped by count and copy alike
};

RPPC_HD bool node_ok(const Chain& c, int64_t nd) { return nd >= 0 && nd < c.n_nodes; }
// the polyline length of node nd as count and copy both see it
RPPC_HD int64_t edge_len(const Chain& c, int64_t nd) {
  const int64_t l = c.plen[nd], o = c.poff[nd];
  return (l > 0 && o >= 0 && o + l <= c.pool_cap) ? l : 0;
}

// 2 + the polyline lengths up the chain from goal_node (the root's own polyline is not part of the course)
RPPC_HD int64_t pose_count(const Chain& c, int32_t goal_node) {
  int64_t total = 2, steps = 0;
  for (int64_t nd = goal_node; node_ok(c, nd) && c.parent[nd] >= 0 && steps < c.n_nodes; nd = c.parent[nd], steps++)
    total += edge_len(c, nd);
  return total;
}

// One round of the walk: up to ROUND chain nodes, for each the offset of its polyline in the slab, its length, and the
// planning-order index k0 of the first point it contributes; `next` is the node the following round starts at (-1: the
// walk is over) and k_next the index after the round's last point.
struct Round {
  int32_t n;
  int32_t next;
  int64_t k_next, steps;
  int32_t len[ROUND];
  int64_t off[ROUND], k0[ROUND];
};

// Filled by one lane.  `nd` and `k` are the round's first node and first index (the first round: goal_node and 1),
// `steps` the steps walked so far.
RPPC_HD void pose_round_fill(const Chain& c, int32_t nd0, int64_t k, int64_t steps, Round& r) {
  int n = 0;
  int64_t nd = nd0;
  while (n < ROUND && node_ok(c, nd) && c.parent[nd] >= 0 && steps < c.n_nodes) {
    const int64_t l = edge_len(c, nd);
    r.len[n] = (int32_t)l;
    r.off[n] = c.poff[nd];
    r.k0[n] = k;
    k += l;
    n++;
    steps++;
    nd = c.parent[nd];
  }
  r.n = n;
  r.k_next = k;
  r.steps = steps;
  r.next = (n == ROUND && node_ok(c, nd) && c.parent[nd] >= 0 && steps < c.n_nodes) ? (int32_t)nd : -1;
}

// Lane `lane` of `lanes` copies its share of a round: point q of a node's reversed polyline is point len - 1 - q of the
// stored one.  src / dst: `ncol` columns (x, y[, yaw]); dst columns start at the course's first row.  Rows outside
// [1, total - 1) are not written (the count of this gather decided `total`).
RPPC_HD void pose_round_copy(const Round& r, const double* const* src, double* const* dst, int ncol, int order, int64_t total,
                             int lane, int lanes) {
  for (int j = 0; j < r.n; j++) {
    const int64_t len = r.len[j], off = r.off[j], k0 = r.k0[j];
    for (int64_t q = lane; q < len; q += lanes) {
      const int64_t k = k0 + q;
      if (k < 1 || k >= total - 1) continue;
      const int64_t row = dst_row(order, total, k), s = off + (len - 1 - q);
      for (int col = 0; col < ncol; col++) dst[col][row] = src[col][s];
    }
  }
}

// the two rows that are no polyline point: the goal pose first, the start pose last (planning order)
RPPC_HD void pose_ends(const double* goal, const double* start, double* const* dst, int ncol, int order, int64_t total) {
  if (total < 2) return;
  const int64_t rg = dst_row(order, total, 0), rs = dst_row(order, total, total - 1);
  for (int col = 0; col < ncol; col++) {
    dst[col][rg] = goal[col];
    dst[col][rs] = start[col];
  }
}

// ---- point planners ----------------------------------------------------------------------------------------------------
// Lane `lane` of `lanes` copies its share of the `total` rows (x, y) of a path buffer
RPPC_HD void flat_copy(const double* src_xy, double* dx, double* dy, int order, int64_t total, int lane, int lanes) {
  for (int64_t k = lane; k < total; k += lanes) {
    const int64_t row = dst_row(order, total, k);
    dx[row] = src_xy[2 * k];
    dy[row] = src_xy[2 * k + 1];
  }
}

// A path deeper than its buffer, by one lane: row 0 the goal, row k >= 1 the node k - 1 steps up the chain from goal_node,
// the root included (rrt_04:1117-1125).  `total` is the plan's path_n; rows the walk does not reach are not written.
RPPC_HD void trunc_walk(const double* x, const double* y, const int32_t* parent, int64_t n_nodes, int32_t goal_node,
                        const double* goal, double* dx, double* dy, int order, int64_t total) {
  if (total < 1) return;
  dx[dst_row(order, total, 0)] = goal[0];
  dy[dst_row(order, total, 0)] = goal[1];
  int64_t k = 1;
  for (int64_t nd = goal_node; k < total && nd >= 0 && nd < n_nodes; nd = parent[nd], k++) {
    const int64_t row = dst_row(order, total, k);
    dx[row] = x[nd];
    dy[row] = y[nd];
  }
}

}  // namespace rppc

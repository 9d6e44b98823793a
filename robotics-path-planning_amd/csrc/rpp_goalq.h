// rpp_goalq.h -- the scalar rules of rrtx_query_goals: which node of a finished tree answers "the best path to goal g",
// and how many points that path has.  Shared by goal_query.hip.h (the kernels) and tests/native/goal_query_host_check.cpp
// (the same routines on the CPU).  The answer is what the tail of the reference's planning() computes with self.end = g:
//   point trees (rrt_04)      search_best_goal_node :1284-1312: among the safe candidates the lowest key
//                             cost + calc_dist_to_goal, first in list order among equals (= the lowest index, the
//                             candidate list being ascending); `is not None` at :1080: index 0 is an answer
//   pose trees (rrt_05 / 06)  search_best_goal_node rrt_05:1691-1712, rrt_06:1815-1836: the lowest node cost inside both
//                             thresholds, first index among equals; `if last_index:` (rrt_05:1451, rrt_06:1565) makes
//                             index 0 "no path"
// Both rules are a minimum over (key, index) pairs, so candidates may be offered in any order and in any number of
// rounds.  Chain walks and pose counts are rpp_course.h's.
#pragma once
#include <cstdint>

#include "rpp_course.h"

#if defined(__HIPCC__)
#define RPPQ_HD __host__ __device__ inline
#else
#define RPPQ_HD inline
#endif

namespace rppq {

// status of one (instance, goal) query: the values of RRTX_GOALQ_* in include/rrtx.h
constexpr int ST_OK = 0, ST_NONE = 1, ST_NO_TREE = 2, ST_OVERFLOW = 3;
constexpr int KIND_POINT = 0, KIND_POSE = 1;
constexpr int32_t NO_INDEX = 0x7fffffff;

// the record of one query as the solve kernel writes it
struct Record {
  double cost;      // the key of the answer (+inf without one)
  int32_t node;     // the answer node, -1: none
  int32_t n_near;   // distinct candidates
  int32_t n_safe;   // point trees: candidates whose edge to the goal is free and ends inside the play area; pose trees 0
  int32_t status;   // ST_*
};
static_assert(sizeof(Record) == 24, "one record is three 8-byte words");

RPPQ_HD double inf() { return __builtin_inf(); }

// an instance whose tree can be asked: planned to the end, and stopped by no failure bit (RRTX_ST_OVERFLOW 4,
// RRTX_ST_UNSUPPORTED 16, RRTX_ST_REF_RAISES 32)
RPPQ_HD bool tree_ok(int32_t inst_status) { return (inst_status & 1) && !(inst_status & (4 | 16 | 32)); }

// the running minimum over (key, index): a lower key wins, the lower index among equal keys.  A NaN key never wins.
struct Best {
  double key;
  int32_t idx;
};
RPPQ_HD Best best_none() { return Best{inf(), NO_INDEX}; }
RPPQ_HD bool better(double key, int32_t idx, const Best& b) { return key < b.key || (key == b.key && idx < b.idx); }
RPPQ_HD void offer(Best& b, double key, int32_t idx) {
  if (better(key, idx, b)) {
    b.key = key;
    b.idx = idx;
  }
}
RPPQ_HD void merge(Best& b, const Best& o) { offer(b, o.key, o.idx); }

// the answer node of a finished minimum, -1: none.  A candidate with a key of +inf is none (a point tree's unsafe
// candidates are offered with that key, as best_goal_node does).
RPPQ_HD int32_t answer(int kind, const Best& b) {
  if (!(b.key < inf()) || b.idx == NO_INDEX || b.idx < 0) return -1;
  if (kind == KIND_POSE && b.idx == 0) return -1;   // `if last_index:`
  return b.idx;
}

RPPQ_HD Record make_record(int kind, const Best& b, int32_t n_near, int32_t n_safe) {
  Record r;
  r.node = answer(kind, b);
  r.cost = r.node >= 0 ? b.key : inf();
  r.n_near = n_near;
  r.n_safe = n_safe;
  r.status = r.node >= 0 ? ST_OK : ST_NONE;
  return r;
}
RPPQ_HD Record empty_record(int status, int32_t n_near) {
  Record r;
  r.node = -1;
  r.cost = inf();
  r.n_near = n_near;
  r.n_safe = 0;
  r.status = status;
  return r;
}

// query q of an n_inst x n_goals batch (row major): its instance, and the row of its goal in the goal table
// ((n_goals, 3) shared by every instance, or (n_inst, n_goals, 3))
RPPQ_HD int32_t inst_of(int64_t q, int32_t n_goals) { return (int32_t)(q / n_goals); }
RPPQ_HD int64_t goal_row(int64_t q, int32_t n_goals, int per_instance) { return per_instance ? q : q % n_goals; }

// points of a point tree's course: the goal, then every node from `node` up to and including the root
// (generate_final_course, rrt_04:1117-1125); 0 without an answer.  No walk takes more than n_nodes steps.
RPPQ_HD int64_t point_count(const int32_t* parent, int64_t n_nodes, int32_t node) {
  if (node < 0 || node >= n_nodes) return 0;
  int64_t total = 1, steps = 0;
  for (int64_t nd = node; nd >= 0 && nd < n_nodes && steps < n_nodes; nd = parent[nd], steps++) total++;
  return total;
}
// points of a pose tree's course (rrt_05:1512-1521, rrt_06:1643-1651): rpp_course.h's count; 0 without an answer
RPPQ_HD int64_t pose_points(const rppc::Chain& c, int32_t node) { return node < 0 ? 0 : rppc::pose_count(c, node); }

}  // namespace rppq

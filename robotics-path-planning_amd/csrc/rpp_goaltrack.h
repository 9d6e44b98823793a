// rpp_goaltrack.h -- the scalar rules of rrtx_track_goals: rrt_10's closed-loop stage asked of a finished tree for many
// goals.  Shared by goal_track.hip.h (the kernels), rrtx_api_goaltrack.inc (the host's sums) and
// tests/native/goal_track_host_check.cpp (the same routines on the CPU).  For a query (instance, goal g) the answer is what
//   path_indexs = self.get_goal_indexes(); self.search_best_feasible_path(path_indexs)        (rrt_10 :1488-1493)
// returns with self.end = Node(*g):
//   candidates   rpp_track.h's is_candidate against g, ascending node index; a goal with a NaN or +-inf component has none
//   pick         track_pick_kernel's loop as a function: over the records in candidate order `flag and best_time >= t[-1]`
//                (:1510, the later candidate wins a tie); a refused record (ood 1 / 2 / 3) sets its status bit and the query
//                then has no winner -- never a wrong answer
//   offsets      candidates: the exclusive sum of the counts; arrays: the exclusive sum of len + 1 over the flagged queries
// The query -> (instance, goal row) map is rpp_goalq.h's.
#pragma once
#include <cstdint>

#include "rpp_goalq.h"
#include "rpp_track.h"

namespace rppgt {

// include/rrtx.h status bits (RRTX_ST_OVERFLOW, RRTX_ST_UNSUPPORTED, RRTX_ST_REF_RAISES)
constexpr int ST_OVERFLOW = 4, ST_OOD = 16, ST_RAISES = 32;
constexpr int32_t COUNT_NO_TREE = -1;              // the count pass's mark of a query on an unfinished tree
constexpr int64_t MAX_CANDIDATES = 1LL << 24;      // of one call, all queries together

struct Outcome {      // per query: rrtx_goal_track_outcome
  int32_t flag;       // search_best_feasible_path found a feasible roll-out
  int32_t winner;     // its position in the query's candidate list (-1 none)
  int32_t n_cand;
  int32_t len;        // len(t) of the winner (x / y / yaw hold len + 1 values: the goal pose is appended, :1519-1521)
  int32_t node;       // the winner's node index (-1 none)
  int32_t status;     // 0, or RRTX_ST_OVERFLOW / RRTX_ST_REF_RAISES / RRTX_ST_UNSUPPORTED bits
  int32_t no_tree;    // the instance's tree did not finish: nothing was asked of it
  int32_t reserved;
  double t_last;      // t[-1] of the winner, +inf without one
};
static_assert(sizeof(Outcome) == 40, "eight words and a double");

// a goal get_goal_indexes can find a node for: every component finite (math.hypot / abs of a NaN or an infinity compare False)
RPP_HD static inline bool goal_finite(double gx, double gy, double gyaw) {
  return !rppt::not_finite(gx) && !rppt::not_finite(gy) && !rppt::not_finite(gyaw);
}

// get_goal_indexes :1566-1582 for one node and one goal
RPP_HD static inline bool goal_candidate(double x, double y, double yaw, double gx, double gy, double gyaw, const rppt::Params& P) {
  return goal_finite(gx, gy, gyaw) && rppt::is_candidate(x, y, yaw, gx, gy, gyaw, P);
}

// the pick over the n records of one query, in candidate order (cand: their node indices)
RPP_HD static inline Outcome pick(const rppt::Record* rec, const int32_t* cand, int64_t n, int no_tree) {
  Outcome o = {0, -1, (int32_t)n, 0, -1, 0, no_tree ? 1 : 0, 0, rpp::dinf()};
  double best_time = rpp::dinf();
  for (int64_t k = 0; k < n; k++) {
    const rppt::Record r = rec[k];
    if (r.ood == 1) o.status |= ST_OOD;
    if (r.ood == 2) o.status |= ST_RAISES;
    if (r.ood == 3) o.status |= ST_OVERFLOW;
    if (rppt::better(r.find, r.tlast, best_time)) {   // :1510
      best_time = r.tlast;
      o.winner = (int32_t)k;
      o.len = r.n;
      o.node = cand[k];
    }
  }
  if (o.status) {   // a refused candidate: the reference raises, or its answer is unknown
    o.winner = -1;
    o.len = 0;
    o.node = -1;
    best_time = rpp::dinf();
  }
  o.flag = o.winner >= 0;
  o.t_last = best_time;
  return o;
}

// The sums below are taken on the host between two launches (rpp_goalq.h's qualifier: host and device).
// candidates of a query from what the count pass wrote
RPPQ_HD int64_t count_of(int32_t mark) { return mark > 0 ? mark : 0; }

// off[0 .. nq]: the exclusive sum of the counts.  Returns the total, or -1 as soon as it exceeds `cap` (off is then unfinished)
RPPQ_HD int64_t candidate_offsets(const int32_t* count, int64_t nq, int64_t cap, int64_t* off) {
  int64_t tot = 0;
  for (int64_t q = 0; q < nq; q++) {
    off[q] = tot;
    tot += count_of(count[q]);
    if (tot > cap) return -1;
  }
  off[nq] = tot;
  return tot;
}

// off[0 .. nq]: the exclusive sum of len + 1 over the queries with a flag (their x / y / yaw entries).  Returns the total
RPPQ_HD int64_t array_offsets(const Outcome* o, int64_t nq, int64_t* off) {
  int64_t tot = 0;
  for (int64_t q = 0; q < nq; q++) {
    off[q] = tot;
    if (o[q].flag) tot += (int64_t)o[q].len + 1;
  }
  off[nq] = tot;
  return tot;
}

}  // namespace rppgt

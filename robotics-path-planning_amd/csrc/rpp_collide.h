// rpp_collide.h -- check_collision of the pose planners for one point of a curve, host + device.
// Reference: 10_path_planning_01_rrt_05_rrt_star_dubins_path.py check_collision :1625-1638 and its copy in rrt_06
//   :1749-1762: for every obstacle, in list order, min over the curve's points of dx * dx + dy * dy <= (size + r) ** 2.
// "min over the points <= thr" is "some point <= thr", so the obstacle at which the reference's loop stops is the lowest
// index any single point touches: first_hit per point, a minimum over the curve's points (steer_batch.hip.h steer_fill).
#pragma once
#include "rpp_core.h"

namespace rpp {

// On the device the rows are read through the constant address space: nothing writes the list while a kernel runs, and the
// row index is the same in every lane still in the loop, so each row is one scalar load (s_load_dwordx4 + x2) for the wave.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const double __attribute__((address_space(4)))* ObsRows;
#else
typedef const double* ObsRows;
#endif

// The first row of `rows` -- m packed rows (ox, oy, thr), thr = (size + robot_radius) ** 2 made on the host -- that the
// point (x, y) touches, or -1.  Two products and one add, as the reference writes them (the build has -ffp-contract=off).
RPP_HD inline int32_t first_hit(const double* rows, int64_t m, double x, double y) {
  const ObsRows obs = (ObsRows)rows;
  for (int64_t j = 0; j < m; j++) {
    const double dx = obs[3 * j] - x, dy = obs[3 * j + 1] - y;
    if (dx * dx + dy * dy <= obs[3 * j + 2]) return (int32_t)j;
  }
  return -1;
}

// The choice among the n >= 1 candidate curves of one pair (steer_batch.hip.h steer_select_free): key[i] is what the kind's
// own planner minimises, hit[i] the candidate's first_hit minimum (-1: free).  *chosen: the free candidate with the smallest
// key, the first in list order among equal keys (a strict <, as paths.index(min(...)) and `best > cost` pick it); where
// none is free, the same choice over all candidates: the planner's own curve.  *rank: the position of the chosen candidate
// when the candidates are ordered by key, list order among equal keys (0 <=> it is the planner's own curve).
RPP_HD inline void pick_free(const double* key, const int32_t* hit, int n, int* chosen, int* rank, int* n_free) {
  int best = 0, bfree = -1, nf = 0;
  for (int i = 0; i < n; i++) {
    if (key[i] < key[best]) best = i;
    if (hit[i] != -1) continue;
    nf++;
    if (bfree < 0 || key[i] < key[bfree]) bfree = i;
  }
  const int ch = bfree >= 0 ? bfree : best;
  int r = 0;
  for (int i = 0; i < n; i++)
    if (key[i] < key[ch] || (key[i] == key[ch] && i < ch)) r++;
  *chosen = ch;
  *rank = r;
  *n_free = nf;
}

}  // namespace rpp

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

}  // namespace rpp

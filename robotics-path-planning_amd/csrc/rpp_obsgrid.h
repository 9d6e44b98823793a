// rpp_obsgrid.h -- the rules of the obstacle map (rrtx_set_obstacle_map): a uniform grid over the circle list of one
// handle, from which rppk::rrt_plan_map_kernel refills its LDS obstacle tile per edge group.  Shared by obstacle_map.hip.h
// (the build kernels), rrt_kernels.hip.h (the query boxes), the host API (geometry, reach) and
// tests/native/obsgrid_host_check.cpp (the same routines on the CPU).
//
// check_collision (rrt_04:1216-1230, rrt_01:220-240) answers "does any circle hold any point of the edge", so the verdict
// does not depend on the order or on the subset of circles tested, as long as no circle that can hit is left out.  The
// grid only ever leaves out circles that cannot hit:
//   geometry   the sampling square [lo, hi]^2 of rand_area (lo = min, hi = max), n x n cells of side (hi - lo) / n with
//              n = clamp(ceil(sqrt(m)), 8, 1024): about one circle per cell.  A side that is not a positive finite
//              number is replaced by 1.
//   cell_of    floor((v - origin) / cell) clamped to [0, n - 1].  Subtraction, division by a positive number, floor and
//              the clamp are all monotone (non-decreasing) in v whatever the rounding, so a <= b gives cell(a) <= cell(b).
//              Circles and query boxes go through this one function.
//   reach      rho = a + a * 2^-40 + 2^-500 with a = |size + robot_radius| (the reference's test is
//              d^2 <= (size + robot_radius)**2: a negative sum still blocks).  A point p is hit when
//              fl(fl(dx^2) + fl(dy^2)) <= thr with dx = fl(ox - px) and thr = pow(a, 2) (< 1 ULP); that bounds
//              |ox - px| by a (1 + 2^-50), or by 2^-537 where the squares underflow, so rho exceeds it as a real number.
//   register   a circle is listed in every cell of range_of(ox - rho, ox + rho, oy - rho, oy + rho).
//   query      a box that contains p has a range that contains cell(p).
// Conservative: p hit by the circle gives ox - rho <= px as real numbers, rounding is monotone and px is a double, so
// fl(ox - rho) <= px and cell(fl(ox - rho)) <= cell(px); likewise above, and for y.  cell(p) is therefore one of the
// circle's cells and one of the box's cells: the walk over the box meets the circle.
//   wide       a circle whose range holds more than WIDE_CELLS cells is listed once, in the wide list, which every box
//              walks; memory is O(m * WIDE_CELLS + cells) at the worst whatever the radii.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RPPO_HD __host__ __device__ inline
#else
#define RPPO_HD inline
#endif

namespace rppo {

constexpr int32_t AXIS_MIN = 8, AXIS_MAX = 1024;   // cells per axis
constexpr int32_t WIDE_CELLS = 32;                 // a circle over more cells goes to the wide list
constexpr int64_t M_MAX = 1 << 20;                 // circles of one map (BatchSteer's limit)

struct Geom {
  double x0, y0, cell;   // origin and side of a cell
  int32_t nx, ny;
};

// one circle as the map kernel reads it: a cell is a contiguous run of these
struct alignas(32) Item {
  double ox, oy, thr;   // thr = (size + robot_radius) ** 2, the double the tile path computes
  int64_t index;        // row of the circle in the caller's list
};
static_assert(sizeof(Item) == 32, "one item is 32 bytes");

// one circle as the build kernels read it
struct Circle {
  double ox, oy, thr, rho;
};

struct Range {
  int32_t cx0, cx1, cy0, cy1;   // inclusive
};

// cells per axis for m circles: the smallest k with k * k >= m, clamped; `forced` > 0 (test knob) takes its place
RPPO_HD int32_t axis_cells(int64_t m, int32_t forced) {
  if (forced > 0) return forced > AXIS_MAX ? AXIS_MAX : forced;
  int64_t k = AXIS_MIN;
  while (k < AXIS_MAX && k * k < m) k++;
  return (int32_t)k;
}

RPPO_HD Geom geometry(double rand_min, double rand_max, int64_t m, int32_t forced) {
  Geom g;
  const double lo = rand_min < rand_max ? rand_min : rand_max, hi = rand_min < rand_max ? rand_max : rand_min;
  g.nx = g.ny = axis_cells(m, forced);
  g.x0 = g.y0 = lo;
  g.cell = (hi - lo) / (double)g.nx;
  if (!(g.cell > 0.0) || !(g.cell < __builtin_inf())) g.cell = 1.0;
  return g;
}

RPPO_HD int32_t cell_of(double v, double origin, double cell, int32_t n) {
  const double q = __builtin_floor((v - origin) / cell);
  if (!(q > 0.0)) return 0;   // below the grid, -0.0
  if (q >= (double)(n - 1)) return n - 1;
  return (int32_t)q;
}

RPPO_HD double reach(double size, double robot_radius) {
  const double a = __builtin_fabs(size + robot_radius);
  return a + a * 0x1p-40 + 0x1p-500;
}

RPPO_HD Range range_of(const Geom& g, double xlo, double xhi, double ylo, double yhi) {
  Range r;
  r.cx0 = cell_of(xlo, g.x0, g.cell, g.nx);
  r.cx1 = cell_of(xhi, g.x0, g.cell, g.nx);
  r.cy0 = cell_of(ylo, g.y0, g.cell, g.ny);
  r.cy1 = cell_of(yhi, g.y0, g.cell, g.ny);
  return r;
}
RPPO_HD Range circle_range(const Geom& g, double ox, double oy, double rho) {
  return range_of(g, ox - rho, ox + rho, oy - rho, oy + rho);
}
RPPO_HD int64_t range_cells(const Range& r) { return (int64_t)(r.cx1 - r.cx0 + 1) * (int64_t)(r.cy1 - r.cy0 + 1); }
RPPO_HD bool is_wide(const Range& r) { return range_cells(r) > WIDE_CELLS; }

// row-major cell number
RPPO_HD int64_t cell_id(const Geom& g, int32_t cx, int32_t cy) { return (int64_t)cy * g.nx + cx; }

}  // namespace rppo

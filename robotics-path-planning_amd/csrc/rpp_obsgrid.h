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

// ---- the obstacle index of the curve objects (rrtx_steer / rrtx_spline / rrtx_bspline): one point against the same grid ------
// The linear loop rpp::first_hit (rpp_collide.h) answers "the lowest row of the list that the point touches".  The grid answers
// the same question from two runs, because every run is in ascending circle index (obstacle_map.hip.h sorts them):
//   geometry_box   a circle list has no rand_area, so the grid lies over the box of the circle centres: origin (xmin, ymin),
//                  n = axis_cells(m, forced) cells per axis of side max(xmax - xmin, ymax - ymin) / n, repaired to 1 where that
//                  is not a positive finite number (a box of zero width: all centres equal; a difference that overflows).
//                  Circles register as above (reach, circle_range, is_wide), by the same build kernels.
//   query          a point p hit by circle j gives cell(p) in j's range (the argument above), so j is listed in the run of
//                  cell(p) or, being wide, in the wide run.  Every circle that hits p is therefore in one of the two runs, and
//                  the lowest index among them is min(first hit of cell(p)'s run, first hit of the wide run): a run in
//                  ascending index gives its lowest hitting index at its first hit.  The wide walk may stop at the first
//                  record whose index exceeds the best so far: nothing behind it is lower.
//   outside        the clamp of cell_of puts a point outside the box into an edge cell c.  cell_of is monotone, so
//                  cell(fl(ox - rho)) <= cell(p) <= cell(fl(ox + rho)) still holds for a hit point, clamped values included:
//                  the circle's clamped range contains c.  Nothing in the argument needs p inside the grid.
//   not finite     a NaN coordinate gives q = NaN and cell 0, +-inf gives an edge cell; dx is then NaN or +-inf, dx * dx + dy * dy
//                  is NaN or +inf, and `<= thr` is false for every finite thr: no record hits, as in the linear loop.
//   -0.0           cell_of sends -0.0 (and every q <= 0) to cell 0 as before; the test itself only squares differences.
//   test           first_hit's own: dx = ox - x, dy = oy - y, dx * dx + dy * dy <= thr (no contraction: -ffp-contract=off), with
//                  Item.thr the very double of the linear rows, the host's (size + robot_radius) ** 2.
// The linear loop serves a list instead -- never an error, these lists are accepted as they are -- when
//   a circle's thr or reach is not finite (an infinite thr hits points the reach cannot bound),
//   a run is longer than RUN_MAX: obsmap_sort_kernel ranks a run with run^2 comparisons by one wave, so 2^20 coincident circles
//     would cost 10^12 of them; 4096 bounds a run at 1.7 * 10^7.  The host has every count after the first build launch and
//     decides before the fill,
//   the list is empty.
constexpr int32_t RUN_MAX = 4096;

// Which of the two serves a list of m circles (include/rrtx.h RRTX_OBSIDX_*, RRTX_OBSIDX_REASON_*): `finite` -- every thr and
// reach is; `longest_run` -- the records of the fullest cell or of the wide list, whichever is more (0 while unknown)
constexpr int32_t IDX_AUTO = 0, IDX_ON = 1, IDX_OFF = 2, IDX_MIN = 256;
constexpr int32_t WHY_USED = 0, WHY_OFF = 1, WHY_BELOW = 2, WHY_RUN_TOO_LONG = 3, WHY_NOT_FINITE = 4, WHY_EMPTY = 5;
RPPO_HD int32_t index_reason(int32_t mode, int64_t m, bool finite, int64_t longest_run) {
  if (m <= 0) return WHY_EMPTY;
  if (mode == IDX_OFF) return WHY_OFF;
  if (mode == IDX_AUTO && m <= IDX_MIN) return WHY_BELOW;
  if (!finite) return WHY_NOT_FINITE;
  if (longest_run > RUN_MAX) return WHY_RUN_TOO_LONG;
  return WHY_USED;
}

RPPO_HD Geom geometry_box(double xmin, double xmax, double ymin, double ymax, int64_t m, int32_t forced) {
  Geom g;
  g.nx = g.ny = axis_cells(m, forced);
  g.x0 = xmin;
  g.y0 = ymin;
  const double wx = xmax - xmin, wy = ymax - ymin;
  g.cell = (wx > wy ? wx : wy) / (double)g.nx;
  if (!(g.cell > 0.0) || !(g.cell < __builtin_inf())) g.cell = 1.0;
  return g;
}

// the built grid as a kernel reads it: cell_start has nx * ny + 2 entries, run nx * ny is the wide list
struct Map {
  Geom g;
  const int32_t* cell_start;
  const Item* items;
};

// The lowest circle index whose circle the point (x, y) touches, or -1: what rpp::first_hit returns for the list the map
// was built from.  Every lane walks the run of its own cell; an Item is 32 aligned bytes (two 16-byte loads).
RPPO_HD int32_t point_first_hit(const Map& mp, double x, double y) {
  const int64_t cells = (int64_t)mp.g.nx * mp.g.ny;
  const int64_t id = cell_id(mp.g, cell_of(x, mp.g.x0, mp.g.cell, mp.g.nx), cell_of(y, mp.g.y0, mp.g.cell, mp.g.ny));
  int64_t best = -1;
  for (int32_t i = mp.cell_start[id], e = mp.cell_start[id + 1]; i < e; i++) {
    const Item it = mp.items[i];
    const double dx = it.ox - x, dy = it.oy - y;
    if (dx * dx + dy * dy <= it.thr) {
      best = it.index;
      break;
    }
  }
  for (int32_t i = mp.cell_start[cells], e = mp.cell_start[cells + 1]; i < e; i++) {
    const Item it = mp.items[i];
    if (best >= 0 && it.index > best) break;
    const double dx = it.ox - x, dy = it.oy - y;
    if (dx * dx + dy * dy <= it.thr) {
      best = it.index;
      break;
    }
  }
  return (int32_t)best;
}

}  // namespace rppo

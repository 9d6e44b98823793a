// rpp_armnav.h -- joint-space occupancy grid of a planar N-link arm among circles and the greedy best-first search on the
// torus grid, host + device source like rpp_spline.h and rpp_bezier.h.
// Reference: 02_arm_obstacle_navigation.py
//   detect_collision :46-76, get_occupancy_grid :79-110, astar_torus :113-184, find_neighbors :187-209,
//   calc_heuristic_map :221-233, NLinkArm.update_points :257-262.
//
// Everything the reference returns is integers (grid cells 0 / 1, route cells, marks 0..6); doubles enter through
// comparisons only.  The forms, as numpy evaluates them on glibc 2.35:
//   theta_list[i]             ((2 * i) * pi) / M for i from -M // 2 (floor division: -(M + 1) / 2 for odd M)
//   np.cos / np.sin (scalar)  libm's (rpp_glibc_cos / rpp_glibc_sin)
//   np.linalg.norm (2-vector) sqrt(fma(y, y, x * x))
//   ndarray.dot (2-vector)    fma(a1, b1, a0 * b0): fused on the second product
// and every other product, quotient and sum rounded where the reference's expression rounds it (no FMA contraction may be
// applied to this file).  The grid sets two joint angles on an N-link arm (:98), so link 1 has angle t_i and every later
// link t_i + t_j (np.sum of the two-element list).
//
// Search state of one query, in LDS on the device and in plain memory in the host check:
//   h[M * M]     uint8   the heuristic (at most 2 M - 2 <= 254)
//   cell[M * M]  uint8   bits 0-2 the mark 0..6, bit 3 open, bits 4-5 which neighbour of its parent the cell is, bit 6 has a parent
//   rowmin[M]    uint32  the smallest (h << 8 | j) over the open cells of row i, kArmRowEmpty when none is open
// np.argmin takes the first cell in row-major order among the smallest h: that is the smallest (h, i, j), and over the rows
// the smallest arm_pop_key.
#pragma once
#include "rpp_core.h"

namespace rpp {

constexpr int kArmMinM = 2, kArmMaxM = 128;
constexpr int kArmMaxLinks = 16, kArmMaxCircles = 1024;
constexpr int kArmRoute = 0, kArmNoRoute = 1;
constexpr uint32_t kArmMark = 7, kArmOpen = 8, kArmDirShift = 4, kArmHasParent = 64;
constexpr uint32_t kArmRowEmpty = 0xffffffffu;
static_assert(2 * kArmMaxM - 2 <= 255, "the heuristic fits a byte");
static_assert(kArmMaxM <= 256, "a column index fits the low byte of a row key");

// Link lengths and circles are the same for every cell of a scene: on the device they are read through the constant
// address space, one scalar load for the wave.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const double __attribute__((address_space(4)))* ArmRow;
#else
typedef const double* ArmRow;
#endif

// ---------------------------------------------------------------- occupancy grid
// theta_list[i] :95
RPP_HD static inline double arm_theta(int i, int M) {
  const int first = -((M + 1) / 2);   // -M // 2
  return ((double)(2 * (first + i)) * 3.141592653589793) / (double)M;
}

// detect_collision :46-76 of the segment a -> b against every circle (rows x, y, radius): true when one is touched
RPP_HD static inline bool arm_link_hits(double ax, double ay, double bx, double by, ArmRow circ, int n_circ) {
  const double lx = bx - ax, ly = by - ay;
  const double mag = __builtin_sqrt(__builtin_fma(ly, ly, lx * lx));   // :65
  const double ux = lx / mag, uy = ly / mag;
  for (int c = 0; c < n_circ; c++) {
    const double cx = circ[3 * c], cy = circ[3 * c + 1], r = circ[3 * c + 2];
    const double qx = cx - ax, qy = cy - ay;
    const double proj = __builtin_fma(qy, uy, qx * ux);   // :67
    double px, py;
    if (proj <= 0.0) {
      px = ax;
      py = ay;
    } else if (proj >= mag) {
      px = bx;
      py = by;
    } else {
      px = ax + (lx * proj) / mag;   // :73
      py = ay + (ly * proj) / mag;
    }
    const double dx = px - cx, dy = py - cy;
    if (!(__builtin_sqrt(__builtin_fma(dy, dy, dx * dx)) > r)) return true;   // :74 (a NaN distance collides, as there)
  }
  return false;
}

// One cell of get_occupancy_grid :96-109: (c1, s1) = cos, sin of t_i, (c12, s12) of t_i + t_j
RPP_HD static inline int arm_cell(double c1, double s1, double c12, double s12, ArmRow len, int n_links, ArmRow circ,
                                  int n_circ) {
  double ax = 0.0, ay = 0.0;
  for (int k = 0; k < n_links; k++) {
    const double L = len[k];
    const double bx = ax + L * (k ? c12 : c1), by = ay + L * (k ? s12 : s1);   // :259-260
    if (arm_link_hits(ax, ay, bx, by, circ, n_circ)) return 1;
    ax = bx;
    ay = by;
  }
  return 0;
}

// ---------------------------------------------------------------- heuristic
RPP_HD static inline int arm_min5(int a, int b, int c, int d, int e) {
  int m = a < b ? a : b;
  m = c < m ? c : m;
  m = d < m ? d : m;
  return e < m ? e : m;
}

// calc_heuristic_map(M, goal)[i][j] :221-233.  The in-place row-major loop reads four border cells per cell; each holds
// either its first value o() or its final one, by where the loop stands: the bottom row and the right column are always
// still o() (or the cell itself), the top row and the left column are final except for the cell itself.  So a cell needs
// the final (0, 0), then its row-0 and column-0 cells: three dependent steps and no loop.
RPP_HD static inline int arm_heuristic(int M, int gi, int gj, int i, int j) {
  const int di0 = gi, diM = M - 1 - gi, dj0 = gj, djM = M - 1 - gj;   // |0 - g|, |M - 1 - g| per axis (0 <= g < M)
  const int di = i < gi ? gi - i : i - gi, dj = j < gj ? gj - j : j - gj;
  const int o00 = dj0 + di0;
  const int f00 = arm_min5(o00, 1 + (dj0 + diM), M + o00, 1 + (djM + di0), M + o00);
  if (i == 0 && j == 0) return f00;
  const int o0j = dj + di0, oi0 = dj0 + di;
  const int f0j = arm_min5(o0j, 1 + (dj + diM), M + o0j, j + 1 + (djM + di0), M - j + f00);
  if (i == 0) return f0j;
  const int fi0 = arm_min5(oi0, i + 1 + (dj0 + diM), M - i + f00, 1 + (djM + di), M + oi0);
  if (j == 0) return fi0;
  return arm_min5(dj + di, i + 1 + (dj + diM), M - i + f0j, j + 1 + (djM + di), M - j + fi0);
}

// ---------------------------------------------------------------- search
struct ArmState {
  uint8_t* h;
  uint8_t* cell;
  uint32_t* rowmin;
};

RPP_HD static inline uint32_t arm_row_key(uint32_t h, int j) { return (h << 8) | (uint32_t)j; }
// (h, i, j) of a row's minimum as one number; kArmRowEmpty stays the largest
RPP_HD static inline uint32_t arm_pop_key(uint32_t rowmin, int i) {
  return rowmin == kArmRowEmpty ? kArmRowEmpty : ((rowmin >> 8) << 16) | ((uint32_t)i << 8) | (rowmin & 0xffu);
}
RPP_HD static inline uint32_t arm_umin(uint32_t a, uint32_t b) { return b < a ? b : a; }

// The state before the first trip, once every cell holds its grid byte and h: astar_torus :130-140
RPP_HD static inline void arm_search_begin(const ArmState& s, int M, int si, int sj, int gi, int gj) {
  const int sc = si * M + sj, gc = gi * M + gj;
  s.cell[sc] = (uint8_t)(4 | kArmOpen);
  s.cell[gc] = (uint8_t)((s.cell[gc] & ~kArmMark) | 5);   // start == goal: 5, and open
  s.rowmin[si] = arm_row_key(s.h[sc], sj);
}

// One trip after its pop (:151-163): the popped cell, which is not the goal, is marked 2 and closed, and its neighbours
// up, down, left, right (find_neighbors, wrap-around) are opened where their mark is 0 or 5.  rowmin of the rows above and
// below is lowered; the popped cell's own row is left to the caller's rescan.
// The reference rewrites grid[start] = 4 and grid[goal] = 5 at the top of every trip (:142-143).  Neither changes what a
// later trip does: the start is closed and 2 is as little expandable as 4, and the goal, once opened (3), is the only cell
// with h = 0 and so the next pop, which ends the loop.  arm_search_end writes both once, as the last trip did.
RPP_HD static inline void arm_search_expand(const ArmState& s, int M, int ci, int cj) {
  const int cur = ci * M + cj;
  s.cell[cur] = (uint8_t)((s.cell[cur] & ~(kArmMark | kArmOpen)) | 2);
  const int up = ci ? ci - 1 : M - 1, dn = ci + 1 < M ? ci + 1 : 0;
  const int lf = cj ? cj - 1 : M - 1, rt = cj + 1 < M ? cj + 1 : 0;
  const int ni[4] = {up, dn, ci, ci}, nj[4] = {cj, cj, lf, rt};
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const int n = ni[d] * M + nj[d];
    const uint32_t b = s.cell[n];
    const uint32_t mark = b & kArmMark;
    if (mark == 0 || mark == 5) {
      s.cell[n] = (uint8_t)(3 | kArmOpen | kArmHasParent | ((uint32_t)d << kArmDirShift));
      if (d < 2) s.rowmin[ni[d]] = arm_umin(s.rowmin[ni[d]], arm_row_key(s.h[n], nj[d]));
    }
  }
}

// The cell whose neighbour number `d` the cell (i, j) is
RPP_HD static inline void arm_parent(int M, int d, int& i, int& j) {
  if (d == 0)
    i = i + 1 < M ? i + 1 : 0;
  else if (d == 1)
    i = i ? i - 1 : M - 1;
  else if (d == 2)
    j = j + 1 < M ? j + 1 : 0;
  else
    j = j ? j - 1 : M - 1;
}

// After the loop (:142-143 of the last trip, :165-175): the cells of the route, 0 when the goal was never opened
RPP_HD static inline int arm_search_end(const ArmState& s, int M, int si, int sj, int gi, int gj) {
  const int sc = si * M + sj, gc = gi * M + gj;
  s.cell[sc] = (uint8_t)((s.cell[sc] & ~kArmMark) | 4);
  s.cell[gc] = (uint8_t)((s.cell[gc] & ~kArmMark) | 5);
  if (!(s.cell[gc] & kArmOpen)) return 0;
  int n = 1, i = gi, j = gj;
  while ((s.cell[i * M + j] & kArmHasParent) && n <= M * M) {   // (the parents are a tree: the bound never binds)
    arm_parent(M, (s.cell[i * M + j] >> kArmDirShift) & 3, i, j);
    n++;
  }
  return n;
}

// The route of n cells, start first, as cell numbers i * M + j into out[0..n), and its cells after the first marked 6
RPP_HD static inline void arm_route_write(const ArmState& s, int M, int gi, int gj, int n, uint16_t* out) {
  int i = gi, j = gj;
  for (int k = n - 1; k >= 0; k--) {
    const int c = i * M + j;
    out[k] = (uint16_t)c;
    const uint32_t b = s.cell[c];
    if (k > 0) {
      s.cell[c] = (uint8_t)((b & ~kArmMark) | 6);
      arm_parent(M, (b >> kArmDirShift) & 3, i, j);
    }
  }
}

}  // namespace rpp

// armnav_batch.hip.h -- batched arm navigation (gfx950): for many scenes the joint-space occupancy grid of
// get_occupancy_grid, and for many (scene, start, goal) queries what astar_torus returns and leaves behind, of
// 02_arm_obstacle_navigation.py.  Scalar pieces: csrc/rpp_armnav.h.
//
//   armnav_trig_kernel    one lane per grid index i: cos and sin of theta_list[i], the table every scene of the call shares.
//   armnav_grid_kernel    one lane per cell (i, j) of one scene; a block lies within one scene, so the scene's link lengths
//                         and circles are the same for the whole wave and come through scalar loads.  cos / sin of t_i come
//                         from the table, those of t_i + t_j are the cell's own.  One byte per cell.
//   armnav_search_kernel  one wave per query, the whole search state in LDS (rpp_armnav.h: h and the cell byte, M * M
//                         bytes each, and a row minimum per row: 33 280 bytes at M = 128).  A trip is
//                           pop     every lane turns the minima of its rows i = lane, lane + 64 into (h, i, j) keys; the
//                                   wave's smallest, by shuffles, is np.argmin's cell
//                           expand  lane 0 closes it and opens its neighbours (arm_search_expand): the four are visited in
//                                   order, and at M = 2 two of them are the same cell
//                           rescan  the wave rebuilds the minimum of the popped row, the only one a close can raise
//                         and the loop is bounded by M * M + 1 trips.  Then lane 0 walks the parents for the route's length,
//                         takes that many cells of the route pool with one atomic add on the pool's cursor, and writes the
//                         route and its marks; a route that does not fit is not written, the cursor still counts it, and
//                         the host runs the batch again with a pool of the size the cursor asked for.  The marked grid is
//                         written by the whole wave when asked for.
#pragma once
#include "rpp_armnav.h"

namespace rppan {

constexpr int TPB = 256;    // trig and grid kernels
constexpr int WAVE = 64;    // search kernel: one wave per block
constexpr int MAX_M = rpp::kArmMaxM;
static_assert(MAX_M <= 2 * WAVE, "a lane owns at most two rows and two cells of a row");

struct Rec {   // per query
  int32_t status, n_route, pops, reserved;
  int64_t off;   // first cell of the route in the pool; -1: no room (or no route)
};

struct GridArgs {
  int32_t M;
  int32_t blocks_per_scene;
  const int64_t* link_off;   // [n_scenes + 1]
  const double* link_len;
  const int64_t* obs_off;    // [n_scenes + 1]
  const double* obs_xyr;     // rows (x, y, radius)
  const double* trig;        // [M][2] cos, sin of theta_list[i]
  uint8_t* grids;            // [n_scenes][M * M]
};

struct SearchArgs {
  int32_t M;
  int64_t n;
  const uint8_t* grids;      // [n_scenes][M * M] bytes 0..6
  const int32_t* scene;      // [n] or nullptr: scene 0
  const int32_t* start;      // [n][2]
  const int32_t* goal;       // [n][2]
  Rec* rec;                  // [n]
  uint16_t* pool;            // [pool_cap] route cells i * M + j
  int64_t pool_cap;
  unsigned long long* cursor;   // cells asked of the pool so far
  uint8_t* marks;            // [n][M * M] or nullptr
};

__global__ __launch_bounds__(TPB) void armnav_trig_kernel(int32_t M, double* trig) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= M) return;
  const double t = rpp::arm_theta(i, M);
  trig[2 * i] = rpp_glibc_cos(t);
  trig[2 * i + 1] = rpp_glibc_sin(t);
}

__global__ __launch_bounds__(TPB) void armnav_grid_kernel(GridArgs a) {
  const int M = a.M;
  const int64_t scene = blockIdx.x / (uint32_t)a.blocks_per_scene;
  const int c = (int)(blockIdx.x % (uint32_t)a.blocks_per_scene) * TPB + threadIdx.x;
  if (c >= M * M) return;
  const int i = c / M, j = c - i * M;
  const double t12 = rpp::arm_theta(i, M) + rpp::arm_theta(j, M);   // np.sum([t_i, t_j])
  const double c12 = rpp_glibc_cos(t12), s12 = rpp_glibc_sin(t12);
  const int64_t l0 = a.link_off[scene], o0 = a.obs_off[scene];
  const int n_links = (int)(a.link_off[scene + 1] - l0), n_circ = (int)(a.obs_off[scene + 1] - o0);
  a.grids[scene * (int64_t)(M * M) + c] = (uint8_t)rpp::arm_cell(a.trig[2 * i], a.trig[2 * i + 1], c12, s12,
                                                                (rpp::ArmRow)(a.link_len + l0), n_links,
                                                                (rpp::ArmRow)(a.obs_xyr + 3 * o0), n_circ);
}

__device__ inline uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = rpp::arm_umin(v, (uint32_t)__shfl_xor((int)v, off));
  return v;
}

__global__ __launch_bounds__(WAVE) void armnav_search_kernel(SearchArgs a) {
  __shared__ uint8_t s_h[MAX_M * MAX_M];
  __shared__ uint8_t s_cell[MAX_M * MAX_M];
  __shared__ uint32_t s_rowmin[MAX_M];
  const int64_t q = blockIdx.x;
  if (q >= a.n) return;
  const int lane = threadIdx.x;
  const int M = a.M, MM = M * M;
  const int si = a.start[2 * q], sj = a.start[2 * q + 1], gi = a.goal[2 * q], gj = a.goal[2 * q + 1];   // inside [0, M) (host)
  const uint8_t* grid = a.grids + (int64_t)(a.scene ? a.scene[q] : 0) * MM;
  const rpp::ArmState st{s_h, s_cell, s_rowmin};

  for (int c = lane; c < MM; c += WAVE) {
    const int i = c / M;
    s_cell[c] = grid[c];
    s_h[c] = (uint8_t)rpp::arm_heuristic(M, gi, gj, i, c - i * M);
  }
  for (int i = lane; i < M; i += WAVE) s_rowmin[i] = rpp::kArmRowEmpty;
  __syncthreads();
  if (lane == 0) rpp::arm_search_begin(st, M, si, sj, gi, gj);
  __syncthreads();

  const uint32_t goal_cell = ((uint32_t)gi << 8) | (uint32_t)gj;
  int pops = 0;
  for (int trip = 0; trip <= MM; trip++) {   // every trip but the last closes a cell for good
    uint32_t key = rpp::arm_pop_key(lane < M ? s_rowmin[lane] : rpp::kArmRowEmpty, lane);
    if (lane + WAVE < M) key = rpp::arm_umin(key, rpp::arm_pop_key(s_rowmin[lane + WAVE], lane + WAVE));
    key = wave_min(key);
    if (key == rpp::kArmRowEmpty || (key & 0xffffu) == goal_cell) break;   // the same in every lane
    const int ci = (int)((key >> 8) & 0xffu), cj = (int)(key & 0xffu);
    pops++;
    if (lane == 0) rpp::arm_search_expand(st, M, ci, cj);
    __syncthreads();
    const uint8_t* row_cell = s_cell + ci * M;
    const uint8_t* row_h = s_h + ci * M;
    uint32_t rk = rpp::kArmRowEmpty;
    if (lane < M && (row_cell[lane] & rpp::kArmOpen)) rk = rpp::arm_row_key(row_h[lane], lane);
    if (lane + WAVE < M && (row_cell[lane + WAVE] & rpp::kArmOpen)) rk = rpp::arm_umin(rk, rpp::arm_row_key(row_h[lane + WAVE], lane + WAVE));
    rk = wave_min(rk);
    if (lane == 0) s_rowmin[ci] = rk;
    __syncthreads();
  }

  if (lane == 0) {
    const int n = rpp::arm_search_end(st, M, si, sj, gi, gj);
    Rec r;
    r.status = n ? rpp::kArmRoute : rpp::kArmNoRoute;
    r.n_route = n;
    r.pops = pops;
    r.reserved = 0;
    r.off = -1;
    if (n) {
      const int64_t off = (int64_t)atomicAdd(a.cursor, (unsigned long long)n);
      if (off + n <= a.pool_cap) {
        r.off = off;
        rpp::arm_route_write(st, M, gi, gj, n, a.pool + off);
      }
    }
    a.rec[q] = r;
  }
  if (a.marks) {
    __syncthreads();
    uint8_t* out = a.marks + q * (int64_t)MM;
    for (int c = lane; c < MM; c += WAVE) out[c] = (uint8_t)(s_cell[c] & rpp::kArmMark);
  }
}

}  // namespace rppan

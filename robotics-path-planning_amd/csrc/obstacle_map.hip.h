// obstacle_map.hip.h -- builds the obstacle map of rrtx_set_obstacle_map on the device (the rules: rpp_obsgrid.h).
//
//   obsmap_count_kernel   one lane per circle: one atomicAdd per covered cell (or one on the wide counter)
//   -- the host takes the exclusive sum of the counts (cell_start; the pattern of rrtx_gather_courses) --
//   obsmap_fill_kernel    one lane per circle: its record into a slot of every covered cell, in arrival order
//   obsmap_sort_kernel    one wave per run: every record to its rank by circle index, into the final item array
//
// The launches do not depend on m (grid-stride loops).  Run number `cells` is the wide list, stored behind the last cell:
// cell_start has cells + 2 entries.  A run sorted by circle index makes the structure reproducible: the fill order is
// whatever the atomics gave, the item array is not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rpp_obsgrid.h"

namespace rppom {

constexpr int TPB = 256, BLOCKS = 1024;

// the run a circle's record goes to for cell (cx, cy) of its range; wide circles have the one run `cells`
__global__ __launch_bounds__(TPB) void obsmap_count_kernel(const rppo::Circle* __restrict__ in, int64_t m, rppo::Geom g,
                                                           int32_t* __restrict__ count) {
  const int64_t cells = (int64_t)g.nx * g.ny;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < m; i += (int64_t)gridDim.x * TPB) {
    const rppo::Circle c = in[i];
    const rppo::Range r = rppo::circle_range(g, c.ox, c.oy, c.rho);
    if (rppo::is_wide(r)) {
      atomicAdd(&count[cells], 1);
      continue;
    }
    for (int32_t cy = r.cy0; cy <= r.cy1; cy++)
      for (int32_t cx = r.cx0; cx <= r.cx1; cx++) atomicAdd(&count[rppo::cell_id(g, cx, cy)], 1);
  }
}

// cursor[]: zeroed, cells + 1 entries; raw[]: the item array in arrival order
__global__ __launch_bounds__(TPB) void obsmap_fill_kernel(const rppo::Circle* __restrict__ in, int64_t m, rppo::Geom g,
                                                          const int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor,
                                                          rppo::Item* __restrict__ raw) {
  const int64_t cells = (int64_t)g.nx * g.ny;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < m; i += (int64_t)gridDim.x * TPB) {
    const rppo::Circle c = in[i];
    rppo::Item it;
    it.ox = c.ox;
    it.oy = c.oy;
    it.thr = c.thr;
    it.index = i;
    const rppo::Range r = rppo::circle_range(g, c.ox, c.oy, c.rho);
    if (rppo::is_wide(r)) {
      raw[cell_start[cells] + atomicAdd(&cursor[cells], 1)] = it;
      continue;
    }
    for (int32_t cy = r.cy0; cy <= r.cy1; cy++)
      for (int32_t cx = r.cx0; cx <= r.cx1; cx++) {
        const int64_t id = rppo::cell_id(g, cx, cy);
        raw[cell_start[id] + atomicAdd(&cursor[id], 1)] = it;
      }
  }
}

// One wave per run (grid-stride over the cells + 1 runs): a record's place is the number of records of its run with a
// lower circle index (a circle is listed once per run).
__global__ __launch_bounds__(TPB) void obsmap_sort_kernel(int64_t runs, const int32_t* __restrict__ cell_start,
                                                          const rppo::Item* __restrict__ raw, rppo::Item* __restrict__ items) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)TPB + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * TPB) >> 6;
  for (int64_t run = wave; run < runs; run += nwaves) {
    const int64_t a = cell_start[run], b = cell_start[run + 1];
    for (int64_t i = a + lane; i < b; i += 64) {
      const rppo::Item it = raw[i];
      int64_t rank = 0;
      for (int64_t j = a; j < b; j++) rank += raw[j].index < it.index ? 1 : 0;
      items[a + rank] = it;
    }
  }
}

}  // namespace rppom

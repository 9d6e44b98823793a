// curve_check.hip.h -- the obstacle-check stage of the kernels with one lane per point of a curve (gfx950): steer_fill,
// spline_eval_kernel, bspline_eval_kernel and bspline_smooth_eval_kernel.  The curves lie in a CSR layout (off[r] <= idx <
// off[r + 1] for the points of row r); every point is tested against one list of circles and the lowest obstacle index a
// row touches goes into hit[row].  The rules of the test itself are rpp_collide.h and rpp_obsgrid.h.
#pragma once
#include "rpp_collide.h"
#include "rpp_obsgrid.h"

namespace rppc {

// A kernel's CHECK: no obstacle test, the linear loop over the rows (rpp::first_hit), or the obstacle index
// (rppo::point_first_hit).  A template parameter and not a branch: a launch without the index carries none of its registers.
constexpr int CHECK_NONE = 0, CHECK_LINEAR = 1, CHECK_INDEX = 2;

// The row r of a CSR offset array with off[r] <= idx < off[r + 1], for 0 <= idx < off[n] (rows without entries are skipped over)
__device__ inline int64_t csr_row(const int64_t* off, int64_t n, int64_t idx) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= idx)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// The obstacle test of one point (x, y) of `row`, by every lane of the wave: the lowest index touched goes into hit[row].
// Every lane: with CHECK a lane past the last point does not leave its kernel but stays as a copy of the last point (the same
// row, the same answer), so that it takes part in the shuffles below.  (That opening stays written out in the four kernels:
// as a function it costs steer_fill<KIND_BEZIER, true, CHECK> two VGPRs.)
// hit[] is read as unsigned for the minimum: -1 (free) is then the largest value, and -2 belongs to rows without points.
template <int CHECK>
__device__ inline void check_point(const double* obs, int64_t n_obs, const rppo::Map& omap, int32_t* hit, int64_t row, double x,
                                   double y) {
  // The obstacle index is the same in every lane still in first_hit's loop, and a lane leaves the loop at its first
  // hit: the wave is done with the list as soon as all its lanes have one.
  const uint32_t NONE = 0xffffffffu;
  // With the index every lane walks the run of its own cell instead: the answer is the same int32.
  const uint32_t h = (uint32_t)(CHECK == CHECK_INDEX ? rppo::point_first_hit(omap, x, y) : rpp::first_hit(obs, n_obs, x, y));
  if (!__any(h != NONE)) return;
  uint32_t* out = (uint32_t*)hit;
  const int r = (int)row;   // n <= 2^30
  const int r0 = __shfl(r, 0);
  if (__all(r == r0)) {   // the wave lies within one curve (the common case for long curves): one atomic
    uint32_t m = h;
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
      m = o < m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(out + r0, m);
  } else if (h != NONE) {
    atomicMin(out + r, h);
  }
}

}  // namespace rppc

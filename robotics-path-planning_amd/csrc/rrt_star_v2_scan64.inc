// One streaming pass over x[0..n), y[0..n) (wave-contiguous quarters, 16-byte non-temporal loads):
//  NEAR:    indices with dx*dx+dy*dy <= thr about (qx,qy), ascending, into hits[] (global) and, with their
//           coordinates, into sh.u.hit (first HW per wave);
//  NEAREST: argmin of dx*dx+dy*dy about (sx,sy) with the winner's coordinates and the runner-up value.
template <bool NEAR, bool NEAREST>
__device__ __forceinline__ int scan2(const double* __restrict__ x, const double* __restrict__ y, int n, double qx,
                                     double qy, double thr, double sx, double sy, int32_t* __restrict__ hits, Sh2& sh,
                                     int& ni, double& gbest, double& gsecond, double& nqx, double& nqy) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int per = roundup_i((n + NW - 1) / NW, WAVE_STRIDE);
  const int ws = w * per;
  const int we = ws + per;
  const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int cnt = 0;
  double best = rpp::dinf(), second = rpp::dinf(), bx = 0.0, by = 0.0;
  int bidx = 0x7fffffff;
  for (int base = ws; base < we && base < n; base += WAVE_STRIDE) {
    v2d xv[UNROLL], yv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const int i0 = base + u * 128 + lane * 2;
      xv[u] = stream2(x + i0);
      yv[u] = stream2(y + i0);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const int i0 = base + u * 128 + lane * 2;
      if (NEAREST) {
        {
          double dx = xv[u].x - sx, dy = yv[u].x - sy;
          double d = dx * dx + dy * dy;
          bool lt = d < best;
          second = lt ? best : (d < second ? d : second);
          bidx = lt ? i0 : bidx;
          bx = lt ? xv[u].x : bx;
          by = lt ? yv[u].x : by;
          best = lt ? d : best;
        }
        {
          double dx = xv[u].y - sx, dy = yv[u].y - sy;
          double d = dx * dx + dy * dy;
          bool lt = d < best;
          second = lt ? best : (d < second ? d : second);
          bidx = lt ? i0 + 1 : bidx;
          bx = lt ? xv[u].y : bx;
          by = lt ? yv[u].y : by;
          best = lt ? d : best;
        }
      }
      if (NEAR) {
        double dx0 = xv[u].x - qx, dy0 = yv[u].x - qy;
        double dx1 = xv[u].y - qx, dy1 = yv[u].y - qy;
        bool h0 = (dx0 * dx0 + dy0 * dy0) <= thr;
        bool h1 = (dx1 * dx1 + dy1 * dy1) <= thr;
        uint64_t m0 = __ballot(h0), m1 = __ballot(h1);
        if ((m0 | m1) != 0ull) {
          int pos = cnt + __popcll(m0 & lt_mask) + __popcll(m1 & lt_mask);
          if (h0) {
            hits[ws + pos] = i0;
            if (pos < HW) {
              Hit& H = sh.u.hit[w * HW + pos];
              H.x = xv[u].x;
              H.y = yv[u].x;
              H.idx = i0;
            }
            pos++;
          }
          if (h1) {
            hits[ws + pos] = i0 + 1;
            if (pos < HW) {
              Hit& H = sh.u.hit[w * HW + pos];
              H.x = xv[u].y;
              H.y = yv[u].y;
              H.idx = i0 + 1;
            }
          }
          cnt += __popcll(m0) + __popcll(m1);
        }
      }
    }
  }
  if (NEAR && lane == 0) {
    sh.wave_cnt[w] = cnt;
    sh.wave_start[w] = ws;
  }
  if (NEAREST) {
    block_argmin_xy(best, bidx, second, bx, by, sh, gbest, ni, gsecond, nqx, nqy);  // barriers publish wave_cnt
  } else {
    lds_barrier();
  }
  int total = 0;
  if (NEAR) {
#pragma unroll
    for (int k = 0; k < NW; k++) total += sh.wave_cnt[k];
  }
  return total;
}

// h-th hit of the concatenated ascending list: index and coordinates (LDS capture, else global read back)
__device__ __forceinline__ void hit_at2(const double* __restrict__ x, const double* __restrict__ y,
                                        const int32_t* __restrict__ hits, const Sh2& sh, int h, int& idx, double& hx,
                                        double& hy) {
  int k = 0;
#pragma unroll
  for (int j = 0; j < NW - 1; j++) {
    if (k == j && h >= sh.wave_cnt[j]) {
      h -= sh.wave_cnt[j];
      k = j + 1;
    }
  }
  if (h < HW) {
    const Hit& H = sh.u.hit[k * HW + h];
    idx = H.idx;
    hx = H.x;
    hy = H.y;
  } else {
    idx = hits[sh.wave_start[k] + h];
    hx = x[idx];
    hy = y[idx];
  }
}

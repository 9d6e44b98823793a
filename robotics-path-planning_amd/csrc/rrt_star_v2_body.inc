// rrt_star_v2_body.inc -- latency-lean RRT* iteration kernel (rrt_04 semantics, search_until_max_iter=True).
//
// Same algorithm, results and HBM layout as rrt_kernels.hip.h (which stays the general path: rrt_01, early-exit
// RRT*, the final goal search), restructured around one measurement: with ~1000 instances streaming their node
// arrays, a dependent global load costs several thousand cycles, and the v1 iteration had ~19 of them on its
// critical path.  Here everything an iteration decides on is carried in LDS / registers:
//   * the scan captures the coordinates of what it finds (nearest node, near-ball hits), so nothing is read back;
//   * each distinct near candidate becomes an LDS record {idx, x, y, cost, first_child, d2, hypot, flags}, filled
//     once (cost / first_child loads overlap the edge evaluation), used by choose_parent, rewire and as the root
//     of the cost propagation;
//   * the cost propagation (rrt_04:1379-1384) walks child lists level by level with frontier entries
//     {idx, cost, x, y, first_child} in LDS: one global round trip per level and sibling, and it refreshes the
//     LDS cost of later rewire candidates it passes, so the sequential rewire order (:1357-1373) needs no re-read;
//   * the nearest-node query of iteration i+1 rides on the near-ball pass of iteration i (see scan_fused in v1).
// What is left on the critical path per iteration: ~1 round trip per successful rewire (sibling links) plus
// ~1 per propagated tree level.
namespace RRT2_NS {

using rppk::Ctx;
using rppk::Inst;
using rppk::FILTER_EPS;
using rppk::v2d;
using rppk::stream2;
using rppk::roundup_i;

constexpr int TPB = RRT2_TPB;
constexpr int NW = TPB / 64;
#ifndef RRT2_UNROLL
#define RRT2_UNROLL 4
#endif
constexpr int UNROLL = RRT2_UNROLL;   // 16-byte load pairs in flight per lane during a streaming pass
constexpr int WAVE_STRIDE = 128 * UNROLL;
constexpr int MAX_OBS = RRT2_MAXOBS;   // obstacle tile capacity in LDS
constexpr int NU = RRT2_NU;            // distinct near candidates held in LDS
constexpr int EBD = RRT2_EBD;          // candidates per edge-evaluation pass (2*EBD edge slots)
constexpr int HW = RRT2_HW;            // near-ball hits per wave captured in LDS (more -> read back from the global list)
constexpr int FCAP = RRT2_FCAP;        // frontier entries per propagation level in LDS (more -> one-lane fallback walk)
constexpr int WPS = RRT2_WPS;          // launch bound: waves per SIMD

struct Hit {
  double x, y;
  int32_t idx, pad;
};
struct Front {
  double c, x, y;
  int32_t idx, fc;
};
struct WalkEnt {   // sibling stack of the depth-first cost walk (propagate_scalar)
  double cp;
  int32_t node, pad;
};

struct Sh2 {
  rpp::MT rng;
  double ox[MAX_OBS], oy[MAX_OBS], othr[MAX_OBS];
  union {
    Hit hit[NW * HW];          // scan -> de-dup
    rpp::Edge edge[2 * EBD];   // edge evaluation
    WalkEnt walk[2 * FCAP * (int)(sizeof(Front) / sizeof(WalkEnt))];   // cost propagation
  } u;
  rpp::Edge e0;                // extension edge / re-steer of a moved node
  double cval[TPB];
  int32_t cflag[TPB];
  int32_t uidx[NU], ufc[NU], uflag[NU];
  double ux[NU], uy[NU], ucur[NU], uval[NU], uhyp[NU], uex[NU], uey[NU];
  double red_best[NW], red_second[NW], red_x[NW], red_y[NW];
  int32_t red_idx[NW], wave_cnt[NW], wave_start[NW];
  double rx, ry, nx, ny;
  int32_t flag, nu, nvalid, overflow, ecoll0;
  int32_t fa, fb, fover, fcount;
  int32_t n_rw, n_pr, moved, last_fc;
  int32_t om;           // this instance's obstacle count, for the loops of the iteration body (uni_i on read)
  long long stat[15];   // per-launch counters, lane 0 only (kept out of the register file)
};

__device__ __forceinline__ void lds_barrier() { __syncthreads(); }  // lowers to s_waitcnt lgkmcnt(0); s_barrier
// a block-uniform value moved to the scalar register file (state carried across iterations must not cost VGPRs)
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uni_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ double uni_d(double v) {
  const uint64_t b = rpp::d2b(v);
  const uint32_t lo = uni_u((uint32_t)b), hi = uni_u((uint32_t)(b >> 32));
  return rpp::b2d(((uint64_t)hi << 32) | lo);
}

// block-wide argmin of (value, index) with lowest-index tie break, carrying the winner's coordinates
// and the runner-up value (filter margin test).
__device__ __forceinline__ void block_argmin_xy(double best, int bidx, double second, double bx, double by, Sh2& sh,
                                                double& gbest, int& gidx, double& gsecond, double& gx, double& gy) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double b = best;
  int bi = bidx;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    double ob = __shfl_xor(b, o);
    int oi = __shfl_xor(bi, o);
    bool take = (ob < b) || (ob == b && oi < bi);
    b = take ? ob : b;
    bi = take ? oi : bi;
  }
  double s = (bidx == bi) ? second : best;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    double os = __shfl_xor(s, o);
    s = os < s ? os : s;
  }
  const uint64_t own = __ballot(bidx == bi);
  const int owner = own ? (__ffsll((long long)own) - 1) : 0;
  const double wx = __shfl(bx, owner), wy = __shfl(by, owner);
  if (lane == 0) {
    sh.red_best[w] = b;
    sh.red_idx[w] = bi;
    sh.red_second[w] = s;
    sh.red_x[w] = wx;
    sh.red_y[w] = wy;
  }
  lds_barrier();
  double gb = sh.red_best[0];
  int gi = sh.red_idx[0], gw = 0;
#pragma unroll
  for (int k = 1; k < NW; k++) {
    double ob = sh.red_best[k];
    int oi = sh.red_idx[k];
    bool take = (ob < gb) || (ob == gb && oi < gi);
    gb = take ? ob : gb;
    gi = take ? oi : gi;
    gw = take ? k : gw;
  }
  double gs = rpp::dinf();
#pragma unroll
  for (int k = 0; k < NW; k++) {
    double c = (sh.red_idx[k] == gi) ? sh.red_second[k] : sh.red_best[k];
    gs = c < gs ? c : gs;
  }
  gbest = gb;
  gidx = gi;
  gsecond = gs;
  gx = sh.red_x[gw];
  gy = sh.red_y[gw];
  lds_barrier();
}

__device__ __forceinline__ int block_min_int(int v, Sh2& sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    int ov = __shfl_xor(v, o);
    v = ov < v ? ov : v;
  }
  if (lane == 0) sh.red_idx[w] = v;
  lds_barrier();
  int r = sh.red_idx[0];
#pragma unroll
  for (int k = 1; k < NW; k++) r = sh.red_idx[k] < r ? sh.red_idx[k] : r;
  lds_barrier();
  return r;
}

// true when the predicate holds on any thread of the workgroup (uses sh.flag; two barriers unless one wave)
__device__ __forceinline__ bool block_any(bool pred, Sh2& sh) {
  const uint64_t m = __ballot(pred);
  if (NW == 1) return m != 0ull;
  if (threadIdx.x == 0) sh.flag = 0;
  lds_barrier();
  if ((threadIdx.x & 63) == 0 && m != 0ull) sh.flag = 1;
  lds_barrier();
  return sh.flag != 0;
}

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

// ---- 16-bit first stage (integer form) -----------------------------------------------------------------------
// The same pass over xq[] = (x16 | y16 << 16), 4 bytes per node: q = rint((coord - q_lo) * q_inv) - 32768 as a signed
// 16-bit value (rppk::quant16).  The query points are rounded to the same grid, so a squared distance is exact integer
// arithmetic in grid units: one saturating packed subtract and one 2-way dot product per (node, query),
//     d = v_pk_sub_i16(node, query) clamp;  d2 = v_dot2_i32_i16(d, d)          (read as u32; at most 2^31)
// Node and query each sit within half a grid step per coordinate of their true position, so a true distance differs
// from the grid distance by less than sqrt(2) steps: c.q_m = 1.4375 q_step (rrtx_api.hip).  A saturated component
// (more than 32767 steps: half the map) reports a LOWER bound >= 32767^2 = QSAT of the grid distance, which keeps both
// uses sound: near-ball hits ({d2 <= (r + q_m)^2}: a superset, every hit re-tested from the f64 coordinates) never
// saturate, and a nearest result is accepted only when best < QSAT (the winner itself is exact) and the runner-up --
// exact or a lower bound -- is more than 2 q_m further; otherwise a second 16-bit pass gathers every node within 2 q_m
// of the best grid distance and decides on their f64 coordinates, and a query it cannot take (a saturated best: the
// first iterations of a tree) goes to the f64 pass (scan2).
// Streaming: each lane keeps QD 16-byte non-temporal loads in flight (a ring: the slot just consumed is re-issued QD
// slots ahead), so a wave has QD KiB outstanding all through the pass instead of a load-wait-compute cadence.  QD = 6:
// same-box A/B of 3 / 4 / 5 / 6 / 8 / 12 gave 6 the best step time twice (3..8 within 3-6 % of each other, 12 clearly
// worse: 23.7 vs 20.5 s -- deeper queues raise the latency of everything else the CU's waves wait for).
// NEAREST tracks (best, runner-up) per lane and the 4-node GROUP (one 16-byte load) the best came from; the caller
// finds the node inside the group from the group's f64 coordinates, which it needs anyway (resolve_group).
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef short s2v __attribute__((ext_vector_type(2)));
#ifndef RRT2_QDEPTH
#define RRT2_QDEPTH 6
#endif
#ifndef RRT2_QDEPTH1
#define RRT2_QDEPTH1 2
#endif
// the one-wave shape runs up to four query sets per pass (below): two loads in flight per lane leave the loop's registers to
// them (ring depths 4 and 6 measured the same step time with two sets: with 16 waves per CU the other waves' loads fill the
// memory pipeline), deeper rings put scratch reloads and full drains into the loop (tools/loop_spill_check.sh)
constexpr int QD1 = RRT2_QDEPTH1;   // ring depth of the pass with further query sets (one-wave shape)
constexpr int QD0 = RRT2_QDEPTH;    // ... of every other pass
constexpr int QSLOT = 256;                       // nodes per wave and ring slot
constexpr uint32_t QSAT = 32767u * 32767u;
constexpr int HWF = HW * (int)(sizeof(Hit) / sizeof(int32_t));   // hit indices per wave captured in LDS

__device__ __forceinline__ uint32_t qdist(uint32_t node, uint32_t query) {
  const s2v d = __builtin_elementwise_sub_sat(__builtin_bit_cast(s2v, node), __builtin_bit_cast(s2v, query));
  uint32_t r;
  asm("v_dot2_i32_i16 %0, %1, %1, 0" : "=v"(r) : "v"(d));    // the three-operand form: one instruction
  return r;
}
__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) { return min(min(a, b), c); }
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) { return max(min(a, b), min(max(a, b), c)); }

// Goal duplicates (SURVEY R6): once a node sits exactly on the goal, every goal sample appends another node with the same
// coordinates -- thousands by the end of a 100 k-node tree -- and every near ball that reaches the goal holds them all.
// They all carry the value of the FIRST of them (`first_goal`), collapse onto it in the `.index` step (:1337) and change
// nothing but the length of near_inds.  With gz >= 0 (= first_goal) the pass therefore records, of the nodes in the
// goal's grid cell (packed value gq), only first_goal itself and COUNTS the others that fall in the ball (zcnt); the
// caller checks the count against the number of exact duplicates it has appended (Inst.goal_dups) -- a different node
// sharing the cell makes it too large, and the pass is repeated with everything recorded.
// Further query sets of a pass (KS of them; one-wave shape only): set j holds the near ball of iteration i + 1 + j,
// speculated about that iteration's sample, and the nearest query of the sample after it -- see "several iterations per
// pass" in the kernel below.
#ifndef RRT2_SPECK
#define RRT2_SPECK 3
#endif
constexpr int KSM = RRT2_SPECK;   // query sets per pass beyond the iteration's own
struct SpecQ {
  uint32_t qq, thr, sq;    // in: packed ball centre, squared ball radius (grid units; 0 with a far centre = set unused), packed nearest query
  int off, cap;            // in: where in hits[] the ball's hits go (ascending), and how many fit
  int cnt;                 // out: nodes in the ball (entries past cap are not stored)
  int grp;                 // out: 4-node group of the nearest node of sq, its and the runner-up's squared grid distance
  double best, second;
};
__device__ __forceinline__ uint32_t umin4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return min(umin3(a, b, c), d); }

// (explicit scalars per set, no arrays: arrays reached through pointers kept the register allocator from holding the
// load ring of the loop below in registers)
struct SpecRun {   // per-lane running state of one further set
  uint32_t best, second;
  int bgrp, cnt;
};
#define RRT2_SET_NEAREST(E, R)                                              \
  {                                                                         \
    const uint32_t c0 = R.best;                                             \
    R.second = min(R.second, umed3(R.best, E[0], E[1]));                    \
    R.best = umin3(R.best, E[0], E[1]);                                     \
    R.second = min(R.second, umed3(R.best, E[2], E[3]));                    \
    R.best = umin3(R.best, E[2], E[3]);                                     \
    R.bgrp = R.best < c0 ? sb : R.bgrp;                                     \
  }
#define RRT2_SET_DIST(QQ2, D)                                               \
  _Pragma("unroll") for (int j = 0; j < 4; j++) {                           \
    D[j] = qdist(v[j], QQ2);                                                \
    if (MASK) D[j] = (i0 + j < n) ? D[j] : 0xffffffffu;                     \
  }
#define RRT2_SET_ANY(D, THR2) (umin4(D[0], D[1], D[2], D[3]) <= THR2)
#define RRT2_SET_RECORD(D, THR2, OFF2, R)                                   \
  {                                                                         \
    bool g[4];                                                              \
    uint64_t m2[4];                                                         \
    uint64_t any2 = 0ull;                                                   \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                         \
      g[j] = D[j] <= THR2;                                                  \
      m2[j] = __ballot(g[j]);                                               \
      any2 |= m2[j];                                                        \
    }                                                                       \
    if (any2 != 0ull) {                                                     \
      int pos = R.cnt;                                                      \
      int tot = 0;                                                          \
      _Pragma("unroll") for (int j = 0; j < 4; j++) {                       \
        pos += __popcll(m2[j] & lt_mask);                                   \
        tot += __popcll(m2[j]);                                             \
      }                                                                     \
      _Pragma("unroll") for (int j = 0; j < 4; j++) {                       \
        if (g[j]) {                                                         \
          if (pos < cap2) hits[OFF2 + pos] = i0 + j;                        \
          pos++;                                                            \
        }                                                                   \
      }                                                                     \
      R.cnt += tot;                                                         \
    }                                                                       \
  }

template <bool NEAR, bool NEAREST, bool MASK, int KS = 0>
__device__ __forceinline__ void scan2q_slot(const v4u v, const int sb, const int l4, const int n, const uint32_t qq,
                                            const uint32_t thr, const uint32_t sq, const uint64_t lt_mask,
                                            int32_t* __restrict__ hits, const int ws, int32_t* lhit, int& cnt,
                                            uint32_t& best, uint32_t& second, int& bgrp, const uint32_t gq, const int gz,
                                            int& zcnt, const uint32_t thra, const uint32_t sqa, const int offa, SpecRun& ra,
                                            const uint32_t thrb, const uint32_t sqb, const int offb, SpecRun& rb,
                                            const uint32_t thrc, const uint32_t sqc, const int offc, SpecRun& rc,
                                            const int cap2) {
  // sb: first node of the slot (wave-uniform), l4 = 4 * lane; this lane's nodes are i0 .. i0 + 3.  The path every slot
  // takes tracks the nearest node's SLOT (bgrp = sb, a scalar operand) and leaves the per-lane index to the hit path and
  // the masked last round: a per-lane value that is live through the loop gets spilled, and its reload in front of the
  // loop makes the compiler drain the load ring at the top of every round (s_waitcnt vmcnt(0) on the main path).
  const int i0 = sb + l4;
  // Five centres for eight queries: the ball of set a is about the sample whose nearest query is the pass's own (sq), the
  // ball of set b about set a's nearest query, the ball of set c about set b's (ball j of the kernel's chain is about
  // sample i + 1 + j, nearest query j about sample i + 2 + j) -- one distance per (node, centre) serves both.
  uint32_t dq[4], d1[4], d2[4], d3[4], d4[4];
  RRT2_SET_DIST(qq, dq)
  if (NEAREST) RRT2_SET_DIST(sq, d1)
  if (KS > 0) RRT2_SET_DIST(sqa, d2)
  if (KS > 1) RRT2_SET_DIST(sqb, d3)
  if (KS > 2) RRT2_SET_DIST(sqc, d4)
  if (KS > 0) RRT2_SET_NEAREST(d2, ra)
  if (KS > 1) RRT2_SET_NEAREST(d3, rb)
  if (KS > 2) RRT2_SET_NEAREST(d4, rc)
  if (NEAREST) {
    // second smallest of {best, second, a, b} with best <= second: min(second, med3(best, a, b))
    const uint32_t b0 = best;
    second = min(second, umed3(best, d1[0], d1[1]));
    best = umin3(best, d1[0], d1[1]);
    second = min(second, umed3(best, d1[2], d1[3]));
    best = umin3(best, d1[2], d1[3]);
    bgrp = best < b0 ? sb : bgrp;
  }
  if (NEAR) {
    // A slot without a hit -- all but a handful per pass -- costs one comparison per ball and ONE ballot + branch:
    // the per-node ballots, the goal-cell bookkeeping and the ordered compaction run only behind it (thr, thr2 < 2^32 - 1,
    // so a masked entry never hits).
    bool lany = RRT2_SET_ANY(dq, thr);
    if (KS > 0) lany = lany || RRT2_SET_ANY(d1, thra);
    if (KS > 1) lany = lany || RRT2_SET_ANY(d2, thrb);
    if (KS > 2) lany = lany || RRT2_SET_ANY(d3, thrc);
    if (__ballot(lany) != 0ull) {
      bool hh[4];
      uint64_t mm[4];
      uint64_t any = 0ull;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        hh[j] = dq[j] <= thr;
        if (gz >= 0) {
          const uint64_t mg = __ballot(hh[j] && v[j] == gq);
          if (mg != 0ull) {   // hits in the goal's cell (rare per slot): keep first_goal, count the rest
            const bool skip = hh[j] && v[j] == gq && (i0 + j) != gz;
            zcnt += __popcll(__ballot(skip));
            hh[j] = hh[j] && !skip;
          }
        }
        mm[j] = __ballot(hh[j]);
        any |= mm[j];
      }
      if (any != 0ull) {
        int pos = cnt;
        int tot = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          pos += __popcll(mm[j] & lt_mask);
          tot += __popcll(mm[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (hh[j]) {
            hits[ws + pos] = i0 + j;
            if (pos < HWF) lhit[pos] = i0 + j;
            pos++;
          }
        }
        cnt += tot;
      }
      if (KS > 0) RRT2_SET_RECORD(d1, thra, offa, ra)
      if (KS > 1) RRT2_SET_RECORD(d2, thrb, offb, rb)
      if (KS > 2) RRT2_SET_RECORD(d3, thrc, offc, rc)
    }
  }
}

// qq / sq: packed grid positions (rppk::quant16) of the near-ball centre and of the nearest query; thr: squared ball
// radius in grid units.  Returns the number of near-ball hits; ggrp = first index of the 4-node group holding the
// nearest node, gbest / gsecond = its and the runner-up's squared grid distance.
// gz >= 0: goal-cell skip (see scan2q_slot); *zskip = in-ball nodes of the goal's cell other than node gz (block total).
template <bool NEAR, bool NEAREST, int KS = 0>
__device__ __forceinline__ int scan2q(const uint32_t* __restrict__ xq, int n, uint32_t qq, uint32_t thr, uint32_t sq,
                                      int32_t* __restrict__ hits, Sh2& sh, int& ggrp, double& gbest,
                                      double& gsecond, uint32_t gq = 0u, int gz = -1, int* zskip = nullptr,
                                      SpecQ* sp = nullptr) {
  // (KS > 0: built for the one-wave shape -- every hit of a further ball goes to one ascending list; never asked for otherwise)
  static_assert(KS <= 3, "three further sets at most");
  // (the balls' centres are implied: ball a about sq, ball b about set a's nearest query, ball c about set b's -- SpecQ::qq
  // is what the caller believes them to be and is not read here)
  const uint32_t thra = KS > 0 ? sp[0].thr : 0u, sqa = KS > 0 ? sp[0].sq : 0u;
  const uint32_t thrb = KS > 1 ? sp[1].thr : 0u, sqb = KS > 1 ? sp[1].sq : 0u;
  const uint32_t thrc = KS > 2 ? sp[2].thr : 0u, sqc = KS > 2 ? sp[2].sq : 0u;
  const int offa = KS > 0 ? sp[0].off : 0, offb = KS > 1 ? sp[1].off : 0, offc = KS > 2 ? sp[2].off : 0;
  const int cap2 = KS > 0 ? sp[0].cap : 0;
  SpecRun ra = {0xffffffffu, 0xffffffffu, 0x7ffffffc, 0}, rb = ra, rc = ra;
  const int lane = threadIdx.x & 63;
  const int w = NW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int per = roundup_i((n + NW - 1) / NW, QSLOT);
  const int ws = w * per;
  const int wend = (ws + per < n) ? ws + per : n;
  const int nsl = wend > ws ? (wend - ws + QSLOT - 1) / QSLOT : 0;   // slots of this wave
  const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int32_t* lhit = reinterpret_cast<int32_t*>(sh.u.hit) + w * HWF;
  int cnt = 0, zcnt = 0;
  uint32_t best = 0xffffffffu, second = 0xffffffffu;
  int bgrp = 0x7ffffffc;
  if (NEAR && gz >= 0 && threadIdx.x == 0) sh.fa = 0;   // block total of zcnt (published by the barriers below)
  if (NEAR && gz >= 0 && NW > 1) lds_barrier();
  if (nsl > 0) {
    const v4u* pv = reinterpret_cast<const v4u*>(xq + ws) + lane;   // slot s = pv[64 * s]
    const int last = nsl - 1;
    constexpr int QD = KS > 0 ? QD1 : QD0;
    const int rounds = (nsl + QD - 1) / QD;
    v4u q[QD];
#pragma unroll
    for (int u = 0; u < QD; u++) q[u] = __builtin_nontemporal_load(pv + 64 * (u < last ? u : last));
    // every round but the last: all QD slots are whole; a slot is consumed, then re-issued QD slots ahead (loads are
    // unconditional -- a conditional load would make the compiler drain the queue -- and clamped to the last slot)
    int s0 = 0;
    for (int r = 0; r + 1 < rounds; r++, s0 += QD) {
#pragma unroll
      for (int u = 0; u < QD; u++) {
        const int s = s0 + u;
        scan2q_slot<NEAR, NEAREST, false, KS>(q[u], ws + s * QSLOT, lane * 4, n, qq, thr, sq, lt_mask, hits, ws, lhit,
                                              cnt, best, second, bgrp, gq, gz, zcnt, thra, sqa, offa, ra, thrb, sqb, offb, rb,
                                              thrc, sqc, offc, rc, cap2);
        const int nx = s + QD;
        q[u] = __builtin_nontemporal_load(pv + 64 * (nx < last ? nx : last));
      }
    }
    // last round: up to QD slots, the final one possibly partial; nothing more to load
#pragma unroll
    for (int u = 0; u < QD; u++) {
      const int s = s0 + u;
      if (s < nsl)
        scan2q_slot<NEAR, NEAREST, true, KS>(q[u], ws + s * QSLOT, lane * 4, n, qq, thr, sq, lt_mask, hits, ws, lhit,
                                             cnt, best, second, bgrp, gq, gz, zcnt, thra, sqa, offa, ra, thrb, sqb, offb, rb,
                                             thrc, sqc, offc, rc, cap2);
    }
  }
  if (NEAR && lane == 0) {
    sh.wave_cnt[w] = cnt;
    sh.wave_start[w] = ws;
    if (gz >= 0 && zcnt) atomicAdd(&sh.fa, zcnt);
  }
  // slot -> this lane's 4-node group in it
  if (NEAREST) bgrp = bgrp == 0x7ffffffc ? bgrp : bgrp + lane * 4;
  if (KS > 0) ra.bgrp = ra.bgrp == 0x7ffffffc ? ra.bgrp : ra.bgrp + lane * 4;
  if (KS > 1) rb.bgrp = rb.bgrp == 0x7ffffffc ? rb.bgrp : rb.bgrp + lane * 4;
  if (KS > 2) rc.bgrp = rc.bgrp == 0x7ffffffc ? rc.bgrp : rc.bgrp + lane * 4;
  if (NEAREST) {
    double t0, t1;
    block_argmin_xy((double)best, bgrp, (double)second, 0.0, 0.0, sh, gbest, ggrp, gsecond, t0, t1);
  } else {
    lds_barrier();
  }
  if (KS > 0) {
    double t0, t1;
    block_argmin_xy((double)ra.best, ra.bgrp, (double)ra.second, 0.0, 0.0, sh, sp[0].best, sp[0].grp, sp[0].second, t0, t1);
    sp[0].cnt = ra.cnt;
  }
  if (KS > 1) {
    double t0, t1;
    block_argmin_xy((double)rb.best, rb.bgrp, (double)rb.second, 0.0, 0.0, sh, sp[1].best, sp[1].grp, sp[1].second, t0, t1);
    sp[1].cnt = rb.cnt;
  }
  if (KS > 2) {
    double t0, t1;
    block_argmin_xy((double)rc.best, rc.bgrp, (double)rc.second, 0.0, 0.0, sh, sp[2].best, sp[2].grp, sp[2].second, t0, t1);
    sp[2].cnt = rc.cnt;
  }
  int total = 0;
  if (NEAR) {
#pragma unroll
    for (int k = 0; k < NW; k++) total += sh.wave_cnt[k];
    if (zskip) *zskip = gz >= 0 ? sh.fa : 0;
  }
  return total;
}

// ---- Grid index of the 16-bit mirror (one-wave shape; DESIGN 5.1 "grid index") ----------------------------------------
// Once the tree is dense a pass reads 4 n bytes to find a handful of nodes: the near ball holds ~8 of 10^5, the nearest
// node is a fraction of a metre away.  The index keys every node on the top bits of its xq[] value -- the same square, the
// same clamping as the mirror -- so a query reads the counts of the few cells that cover it (one round trip) and their
// entries {node, xq} (a second one), and applies to them exactly the grid test of the streaming pass.  A pass over the
// index has the contract of scan2q: the ball's hits in ascending index order with exact counts, the nearest node's
// 4-node group with the lowest index among equals, and a runner-up that is the true one or a lower bound of it.
// Left out of the index: the exact goal duplicates (SURVEY R6; all at the goal's xq value with indices above first_goal,
// `excl` of them), so the goal's cell stays small; a ball that reaches them counts them like the streaming pass does.
struct GridS {
  int32_t* cnt;     // [gcells] entries per cell
  int32_t* blk;     // [gcells] overflow block + 1 (0: none)
  uint64_t* ent;    // [gcells][GRID_CAP0] {node | xq << 32}
  uint64_t* pool;   // [pool_blocks][GRID_CAP1]
  int sh, gn, pool_blocks, pool_next, excl, min_n;
  uint32_t goal_q;
  int ok;           // 0: the index is off, or incomplete for the rest of the launch -- every pass streams
  int merge;        // 1: a pass gathers for all its centres together (RRTX_GRID_MERGE)
  int bytes, nodes; // what the last pass read: bytes and nodes (entries) it tested
};
constexpr int GRID_CAP0 = rppk::GRID_CAP0, GRID_CAP1 = rppk::GRID_CAP1, GRID_CAPT = GRID_CAP0 + GRID_CAP1;
constexpr int GE = 4;   // entries per lane a window gathers: 256 at most
static_assert(GRID_CAPT <= 64, "a cell's entries fit one wave");

__device__ __forceinline__ int grid_cell(const GridS& g, uint32_t q) {
  const uint32_t u = q ^ 0x80008000u;   // unsigned grid coordinates
  return (int)((u >> (16 + g.sh)) * (uint32_t)g.gn + ((u & 0xffffu) >> g.sh));
}
__device__ __forceinline__ uint64_t grid_entry(int node, uint32_t q) { return (uint64_t)(uint32_t)node | ((uint64_t)q << 32); }

// The index of nodes [0, n) from xq[] (every launch starts with it: resume and re-plan need nothing else).  Appends go
// through grid_insert, a node that rewire moves through grid_remove + grid_insert.
__device__ __forceinline__ void grid_build(GridS& g, const uint32_t* __restrict__ xq, const double* x, const double* y,
                                           int n, double gx, double gy, int first_goal) {
  const int lane = threadIdx.x & 63;
  const int cells = g.gn * g.gn;
  for (int i = lane; i < cells; i += 64) {
    g.cnt[i] = 0;
    g.blk[i] = 0;
  }
  g.pool_next = 0;
  g.excl = 0;
  __threadfence();
  const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    bool on = i < n;
    const uint32_t q = on ? xq[i] : 0u;
    if (on && first_goal >= 0 && q == g.goal_q && i != first_goal && x[i] == gx && y[i] == gy) on = false;
    g.excl += __popcll(__ballot(i < n && !on));
    const int cell = grid_cell(g, q);
    const int k = on ? atomicAdd(&g.cnt[cell], 1) : 0;
    const uint64_t nb = __ballot(on && k == GRID_CAP0);   // cells that need their overflow block now
    if (on && k == GRID_CAP0) {
      const int b = g.pool_next + __popcll(nb & lt_mask) + 1;
      if (b <= g.pool_blocks) g.blk[cell] = b;
    }
    g.pool_next += __popcll(nb);
    __threadfence();
    if (on && k < GRID_CAP0) {
      g.ent[(int64_t)cell * GRID_CAP0 + k] = grid_entry(i, q);
    } else if (on && k < GRID_CAPT) {
      const int b = g.blk[cell];
      if (b > 0) g.pool[(int64_t)(b - 1) * GRID_CAP1 + (k - GRID_CAP0)] = grid_entry(i, q);
    }
  }
  if (g.pool_next > g.pool_blocks) g.ok = 0;
  __threadfence();
}

// Node `node` at packed position q joins its cell (every lane calls; lane 0 stores).  A cell past both blocks keeps
// counting: the passes that need it stream.
__device__ __forceinline__ void grid_insert(GridS& g, int node, uint32_t q) {
  const int cell = grid_cell(g, q);
  const int k = g.cnt[cell];
  int b = g.blk[cell];
  const uint64_t e = grid_entry(node, q);
  if (k < GRID_CAP0) {
    if (threadIdx.x == 0) g.ent[(int64_t)cell * GRID_CAP0 + k] = e;
  } else if (k < GRID_CAPT) {
    if (b == 0) {
      if (g.pool_next >= g.pool_blocks) {
        g.ok = 0;
        return;
      }
      b = ++g.pool_next;
      if (threadIdx.x == 0) g.blk[cell] = b;
    }
    if (threadIdx.x == 0) g.pool[(int64_t)(b - 1) * GRID_CAP1 + (k - GRID_CAP0)] = e;
  }
  if (threadIdx.x == 0) g.cnt[cell] = k + 1;
}

// Node `node`, at packed position q until now, leaves its cell: the cell's last entry takes its place.
__device__ __forceinline__ void grid_remove(GridS& g, int node, uint32_t q) {
  const int lane = threadIdx.x & 63;
  const int cell = grid_cell(g, q);
  const int k = g.cnt[cell], b = g.blk[cell];
  if (k > GRID_CAPT) {
    g.ok = 0;
    return;
  }
  uint64_t* p = lane < GRID_CAP0 ? g.ent + (int64_t)cell * GRID_CAP0 + lane
                                 : (b > 0 ? g.pool + (int64_t)(b - 1) * GRID_CAP1 + (lane - GRID_CAP0) : nullptr);
  const bool mine = lane < k && p != nullptr;
  const uint64_t e = mine ? *p : 0ull;
  const uint64_t m = __ballot(mine && (int)(uint32_t)e == node);
  if (m == 0ull) {   // not in the index (a left-out goal duplicate): the index is incomplete from here
    g.ok = 0;
    return;
  }
  const int j = __ffsll((long long)m) - 1;
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)e, k - 1), hi = (uint32_t)__shfl((int)(uint32_t)(e >> 32), k - 1);
  if (lane == j) *p = (uint64_t)lo | ((uint64_t)hi << 32);
  if (lane == 0) g.cnt[cell] = k - 1;
}

// The tests of one centre on the entries the lanes hold for it (every other slot: d = 0xffffffff, ei = 0x7fffffff).
// BALL: the entries with grid distance <= thr, ascending, at hits[off ..] (first `cap`) and lhit[] (first HWF; nullptr:
// none); gz >= 0 applies the goal-cell rule of scan2q_slot (zcnt).  NEAREST: (best, runner-up, group) over the window,
// runner-up capped at D^2 (D: distance to the nearest cell outside the window, a lower bound of any node there); the
// answer stands only when best + 2 q_m (+ 1 step for the roundings of the caller's test) lies inside D -- then both the
// winner and every decision the caller takes on the runner-up are those of the full pass.  Returns 1: answered, 0: the
// index cannot answer (the caller streams), 2: the nearest query needs a wider window (wbest: the best distance seen).
__device__ __forceinline__ int grid_tests(const GridS& g, uint32_t cq, int D, bool ball, uint32_t thr, bool nearest,
                                          const uint32_t (&ev)[GE], const int (&ei)[GE], const uint32_t (&d)[GE],
                                          int32_t* __restrict__ hits, int off, int cap, int32_t* lhit, int32_t* ltmp,
                                          int gz, int& cnt, int& zcnt, uint32_t& best, uint32_t& second, int& grp,
                                          uint32_t& wbest) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  if (ball) {
    // the left-out goal duplicates lie at goal_q: counted with gz >= 0, else they would be hits the index cannot list
    const bool zin = g.excl > 0 && qdist(g.goal_q, cq) <= thr;
    if (zin && gz < 0) return 0;
    int z = zin ? g.excl : 0, H = 0;
    bool hh[GE];
#pragma unroll
    for (int k = 0; k < GE; k++) {
      hh[k] = d[k] <= thr;   // thr < 2^32 - 1: an empty slot never hits
      if (gz >= 0) {
        const bool skip = hh[k] && ev[k] == g.goal_q && ei[k] != gz;
        z += __popcll(__ballot(skip));
        hh[k] = hh[k] && !skip;
      }
      const uint64_t m = __ballot(hh[k]);
      if (hh[k]) ltmp[H + __popcll(m & lt_mask)] = ei[k];
      H += __popcll(m);
    }
    lds_barrier();
    // ascending order: a hit's place is the number of hits with a lower index
    for (int h0 = 0; h0 < H; h0 += 64) {
      if (h0 + lane < H) {
        const int me = ltmp[h0 + lane];
        int r = 0;
        for (int j = 0; j < H; j++) r += ltmp[j] < me ? 1 : 0;
        if (r < cap) hits[off + r] = me;
        if (lhit && r < HWF) lhit[r] = me;
      }
    }
    lds_barrier();
    cnt = H;
    zcnt = z;
  }
  if (!nearest) return 1;
  uint32_t b = 0xffffffffu, s = 0xffffffffu;
  int bi = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < GE; k++) {
    if (d[k] < b || (d[k] == b && ei[k] < bi)) {
      s = b;
      b = d[k];
      bi = ei[k];
    } else {
      s = min(s, d[k]);
    }
  }
  uint32_t wb = b;
  int wi = bi;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t ob = (uint32_t)__shfl_xor((int)wb, o);
    const int oi = __shfl_xor(wi, o);
    const bool take = ob < wb || (ob == wb && oi < wi);
    wb = take ? ob : wb;
    wi = take ? oi : wi;
  }
  uint32_t ws = bi == wi ? s : b;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ws = min(ws, (uint32_t)__shfl_xor((int)ws, o));
  // the left-out duplicates tie with first_goal (in the index, lower index): a runner-up at the goal's distance
  if (g.excl > 0) ws = min(ws, qdist(g.goal_q, cq));
  wbest = wb;
  if (wb < QSAT && (double)D > __builtin_sqrt((double)wb) + 4.0) {
    best = wb;
    second = min(ws, (uint32_t)(D * D));
    grp = wi & ~3;
    return 1;
  }
  return 2;
}

// The square window [centre - rw, centre + rw] in cells: false when it holds more than 64.  D: grid_tests.
__device__ __forceinline__ bool grid_window(const GridS& g, uint32_t cq, int rw, int& x0, int& y0, int& nwx, int& nc, int& D) {
  const int ux = (int)((cq ^ 0x80008000u) & 0xffffu), uy = (int)((cq ^ 0x80008000u) >> 16);
  x0 = max(ux - rw, 0) >> g.sh;
  y0 = max(uy - rw, 0) >> g.sh;
  const int x1 = min(ux + rw, 65535) >> g.sh, y1 = min(uy + rw, 65535) >> g.sh;
  nwx = x1 - x0 + 1;
  nc = nwx * (y1 - y0 + 1);
  if (nc > 64) return false;
  D = 32767;
  if (x0 > 0) D = min(D, ux - (x0 << g.sh) + 1);
  if (x1 < g.gn - 1) D = min(D, ((x1 + 1) << g.sh) - ux);
  if (y0 > 0) D = min(D, uy - (y0 << g.sh) + 1);
  if (y1 < g.gn - 1) D = min(D, ((y1 + 1) << g.sh) - uy);
  return true;
}

// window half-width of the next attempt of a nearest query: past best + margin when a node was found, else threefold
__device__ __forceinline__ int grid_grow(uint32_t wb, int rw) { return wb < QSAT ? (int)__builtin_sqrt((double)wb) + 6 : 3 * rw + 1; }

// One centre of a pass over the index, by itself: the cells of its window (at most 64, at most 256 entries), one round
// trip for their counts and one for their entries, then grid_tests; a nearest query whose window must grow tries twice
// more (three attempts in all; first_attempt = 1: the merged gather of grid_pass made the first).  False: the index
// cannot answer (the caller streams).
__device__ __forceinline__ bool grid_centre(const GridS& g, uint32_t cq, int rw, bool ball, uint32_t thr, bool nearest,
                                            int32_t* __restrict__ hits, int off, int cap, int32_t* lhit, int32_t* ltmp,
                                            int gz, int& cnt, int& zcnt, uint32_t& best, uint32_t& second, int& grp,
                                            int& bytes, int& nodes, int first_attempt = 0) {
  const int lane = threadIdx.x & 63;
  for (int attempt = first_attempt; attempt < 3; attempt++) {
    int x0, y0, nwx, nc, D;
    if (!grid_window(g, cq, rw, x0, y0, nwx, nc, D)) return false;
    int cell = 0, cn = 0, cb = 0;
    if (lane < nc) {
      cell = (y0 + lane / nwx) * g.gn + x0 + lane % nwx;
      cn = g.cnt[cell];
      cb = g.blk[cell];
    }
    if (__ballot(cn > GRID_CAPT) != 0ull) return false;
    int inc = cn;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    const int tot = __shfl(inc, 63);
    bytes += 8 * nc + 8 * tot;
    nodes += tot;
    if (tot > 64 * GE) return false;
    const int pre = inc - cn;
    const uint64_t* ptr[GE];
#pragma unroll
    for (int k = 0; k < GE; k++) ptr[k] = nullptr;
    for (uint64_t nz = __ballot(cn > 0); nz != 0ull; nz &= nz - 1) {
      const int j = __ffsll((long long)nz) - 1;
      const int pj = __builtin_amdgcn_readlane(pre, j), cj = __builtin_amdgcn_readlane(cn, j);
      const int ej = __builtin_amdgcn_readlane(cell, j), bj = __builtin_amdgcn_readlane(cb, j);
#pragma unroll
      for (int k = 0; k < GE; k++) {
        const int r = lane + 64 * k - pj;
        if (r >= 0 && r < cj)
          ptr[k] = r < GRID_CAP0 ? g.ent + (int64_t)ej * GRID_CAP0 + r : g.pool + (int64_t)(bj - 1) * GRID_CAP1 + (r - GRID_CAP0);
      }
    }
    uint32_t ev[GE], d[GE];
    int ei[GE];
#pragma unroll
    for (int k = 0; k < GE; k++) {
      const uint64_t e = ptr[k] ? *ptr[k] : 0ull;
      ei[k] = ptr[k] ? (int)(uint32_t)e : 0x7fffffff;
      ev[k] = (uint32_t)(e >> 32);
      d[k] = ptr[k] ? qdist(ev[k], cq) : 0xffffffffu;
    }
    uint32_t wb = 0xffffffffu;
    const int r = grid_tests(g, cq, D, ball && attempt == 0, thr, nearest, ev, ei, d, hits, off, cap, lhit, ltmp, gz, cnt,
                             zcnt, best, second, grp, wb);
    if (r != 2) return r == 1;
    rw = grid_grow(wb, rw);
    ball = false;
  }
  return false;
}

// A centre of a pass: what is asked about it, and the answers.
struct GCen {
  uint32_t cq, thr;      // packed centre; ball threshold
  int rw;                // window half-width (grid steps)
  bool on, ball, nearest;
  int off, cap, gz;      // ball: list offset and room in hits[], goal-cell rule
  int32_t* lhit;         // ball: the LDS copy of the list (nullptr: none)
  int cnt, zcnt, grp;    // answers (grid_tests)
  uint32_t best, second;
};

// All centres of a pass together (RRTX_GRID_MERGE): one lane per (centre, cell) pair of every window and one round trip for
// all their counts; a prefix sum over the pairs gives every entry a slot (GE per lane, each slot remembers its centre;
// a slot finds its pair by a binary search of the prefix array in the pass's LDS scratch) and one more round trip loads
// them all; then each centre runs grid_tests on its own slots -- the same entries, so the same answers and the same
// bytes as the per-centre passes.  Returns 1: every centre is answered, except the nearest queries flagged in `grow`
// (bit c; ce[c].best = the best distance seen), whose window must grow: grid_centre goes on with them from the second
// attempt; 0: the index cannot answer (the caller streams); -1: the windows do not fit one gather (more than 64 pairs or
// 256 entries in all, or one window too large): nothing was answered, the per-centre passes decide.
template <int NC>
__device__ __forceinline__ int grid_merged(const GridS& g, GCen (&ce)[NC], int32_t* __restrict__ hits, int32_t* ltmp,
                                           int& bytes, int& nodes, uint32_t& grow) {
  const int lane = threadIdx.x & 63;
  int D[NC], npairs = 0;
  int cid = -1, cell = 0, cn = 0, cb = 0;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    D[c] = 0;
    if (!ce[c].on) continue;
    int x0, y0, nwx, nc;
    if (!grid_window(g, ce[c].cq, ce[c].rw, x0, y0, nwx, nc, D[c])) return -1;
    const int l = lane - npairs;
    if (l >= 0 && l < nc) {
      cid = c;
      cell = (y0 + l / nwx) * g.gn + x0 + l % nwx;
    }
    npairs += nc;
  }
  if (npairs > 64) return -1;
  if (cid >= 0) {
    cn = g.cnt[cell];
    cb = g.blk[cell];
  }
  if (__ballot(cn > GRID_CAPT) != 0ull) return 0;
  int inc = cn;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  const int tot = __shfl(inc, 63);
  if (tot > 64 * GE) return -1;
  bytes += 8 * npairs + 8 * tot;
  nodes += tot;
  ltmp[lane] = inc;
  ltmp[64 + lane] = cell;
  ltmp[128 + lane] = cb;
  ltmp[192 + lane] = cid;
  lds_barrier();
  uint32_t ev[GE];
  int ei[GE], sc[GE];
  const uint64_t* ptr[GE];
#pragma unroll
  for (int k = 0; k < GE; k++) {
    const int slot = lane + 64 * k;
    ptr[k] = nullptr;
    sc[k] = -1;
    if (slot < tot) {
      int j = 0;   // the first pair whose inclusive prefix passes the slot (tot = the last prefix > slot: j <= 63)
#pragma unroll
      for (int st = 32; st >= 1; st >>= 1)
        if (ltmp[j + st - 1] <= slot) j += st;
      const int r = slot - (j > 0 ? ltmp[j - 1] : 0);
      const int ej = ltmp[64 + j], bj = ltmp[128 + j];
      sc[k] = ltmp[192 + j];
      ptr[k] = r < GRID_CAP0 ? g.ent + (int64_t)ej * GRID_CAP0 + r : g.pool + (int64_t)(bj - 1) * GRID_CAP1 + (r - GRID_CAP0);
    }
  }
#pragma unroll
  for (int k = 0; k < GE; k++) {
    const uint64_t e = ptr[k] ? *ptr[k] : 0ull;
    ei[k] = (int)(uint32_t)e;
    ev[k] = (uint32_t)(e >> 32);
  }
  lds_barrier();   // the prefix arrays are read: grid_tests takes the scratch
  grow = 0u;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (!ce[c].on) continue;
    uint32_t d[GE];
    int eic[GE];
#pragma unroll
    for (int k = 0; k < GE; k++) {
      const bool mine = sc[k] == c;
      eic[k] = mine ? ei[k] : 0x7fffffff;
      d[k] = mine ? qdist(ev[k], ce[c].cq) : 0xffffffffu;
    }
    uint32_t wb = 0xffffffffu;
    const int r = grid_tests(g, ce[c].cq, D[c], ce[c].ball, ce[c].thr, ce[c].nearest, ev, eic, d, hits, ce[c].off, ce[c].cap,
                             ce[c].lhit, ltmp, ce[c].gz, ce[c].cnt, ce[c].zcnt, ce[c].best, ce[c].second, ce[c].grp, wb);
    if (r == 0) return 0;
    if (r == 2) {
      grow |= 1u << c;
      ce[c].best = wb;
    }
  }
  return 1;
}

// A pass of scan2q's contract (same arguments and outputs) answered from the index; false: it cannot be (the caller
// streams, which rewrites every output).  rwn: window half-width (grid steps) to start a nearest query with.
template <bool NEAR, bool NEAREST, int KS>
__device__ __forceinline__ bool grid_pass(GridS& g, int rwn, uint32_t qq, uint32_t thr, uint32_t sq,
                                          int32_t* __restrict__ hits, Sh2& sh, int& ggrp, double& gbest, double& gsecond,
                                          int gz, int* zskip, SpecQ* sp, int& total) {
  int32_t* lhit = reinterpret_cast<int32_t*>(sh.u.hit);
  int32_t* ltmp = lhit + HWF;
  static_assert(sizeof(sh.u) >= sizeof(int32_t) * (HWF + 64 * GE), "LDS scratch of a grid pass");
  int bytes = 0, nodes = 0;
  uint32_t b, s;
  int gr, zc = 0, cnt = 0;
  if (g.merge) {
    // centre 0: the pass's own ball; centre 1 + j: as in the loop below
    GCen ce[KS + 2];
    ce[0].on = NEAR;
    ce[0].cq = qq; ce[0].thr = thr; ce[0].rw = (int)__builtin_sqrt((double)thr) + 1;
    ce[0].ball = true; ce[0].nearest = false;
    ce[0].off = 0; ce[0].cap = 0x7fffffff; ce[0].gz = gz; ce[0].lhit = lhit;
    ce[0].cnt = 0; ce[0].zcnt = 0; ce[0].grp = 0x7ffffffc; ce[0].best = ce[0].second = 0xffffffffu;
#pragma unroll
    for (int j = 0; j <= KS; j++) {
      GCen& e = ce[1 + j];
      const int jo = j < KS ? j : 0;
      e.cq = j == 0 ? sq : sp[j > 0 ? j - 1 : 0].sq;
      e.nearest = j == 0 ? NEAREST : sp[j > 0 ? j - 1 : 0].thr != 0u;
      e.thr = j < KS ? sp[jo].thr : 0u;
      e.ball = e.thr != 0u;
      e.on = e.nearest || e.ball;
      e.rw = max(e.ball ? (int)__builtin_sqrt((double)e.thr) + 1 : 0, e.nearest ? rwn : 0);
      e.off = KS > 0 ? sp[jo].off : 0;
      e.cap = KS > 0 ? sp[jo].cap : 0;
      e.gz = -1;
      e.lhit = nullptr;
      e.cnt = 0; e.zcnt = 0; e.grp = 0x7ffffffc; e.best = e.second = 0xffffffffu;
    }
    uint32_t grow = 0u;
    const int r = grid_merged<KS + 2>(g, ce, hits, ltmp, bytes, nodes, grow);
    if (r == 0) return false;
    if (r == 1) {
#pragma unroll
      for (int j = 0; j <= KS; j++) {
        GCen& e = ce[1 + j];
        if (grow >> (1 + j) & 1u) {   // a nearest query whose window must grow: by itself, from the second attempt
          int bc, bz;
          const uint32_t wb = e.best;
          e.best = e.second = 0xffffffffu;
          if (!grid_centre(g, e.cq, grid_grow(wb, e.rw), false, 0u, true, hits, 0, 0, nullptr, ltmp, -1, bc, bz, e.best,
                           e.second, e.grp, bytes, nodes, 1))
            return false;
        }
        if (j == 0) {
          if (NEAREST) {
            gbest = (double)e.best;
            gsecond = (double)e.second;
            ggrp = e.grp;
          }
        } else {
          sp[j - 1].best = (double)e.best;
          sp[j - 1].second = (double)e.second;
          sp[j - 1].grp = e.grp;
        }
        if (j < KS) sp[j < KS ? j : 0].cnt = e.cnt;
      }
      if (NEAR && threadIdx.x == 0) {
        sh.wave_cnt[0] = ce[0].cnt;
        sh.wave_start[0] = 0;
        sh.fa = ce[0].zcnt;
      }
      lds_barrier();
      if (NEAR && zskip) *zskip = gz >= 0 ? ce[0].zcnt : 0;
      total = NEAR ? ce[0].cnt : 0;
      g.bytes = bytes;
      g.nodes = nodes;
      return true;
    }
    // the windows do not fit one gather: per-centre passes, from the start
  }
  if (NEAR) {
    const int rw = (int)__builtin_sqrt((double)thr) + 1;
    if (!grid_centre(g, qq, rw, true, thr, false, hits, 0, 0x7fffffff, lhit, ltmp, gz, cnt, zc, b, s, gr, bytes, nodes))
      return false;
  }
  // centre j: the nearest query of the pass (j = 0, sq) or of set j - 1 (sp[j - 1].sq), and the ball of set j about it
#pragma unroll
  for (int j = 0; j <= KS; j++) {
    const uint32_t cq = j == 0 ? sq : sp[j > 0 ? j - 1 : 0].sq;
    const bool nq = j == 0 ? NEAREST : sp[j > 0 ? j - 1 : 0].thr != 0u;   // (a set with thr 0 is unused)
    const uint32_t bthr = j < KS ? sp[j < KS ? j : 0].thr : 0u;
    uint32_t bb = 0xffffffffu, bs = 0xffffffffu;
    int bg = 0x7ffffffc, bc = 0, bz = 0;
    if (nq || bthr != 0u) {
      const int rw = max(bthr != 0u ? (int)__builtin_sqrt((double)bthr) + 1 : 0, nq ? rwn : 0);
      const int jo = j < KS ? j : 0;
      if (!grid_centre(g, cq, rw, bthr != 0u, bthr, nq, hits, KS > 0 ? sp[jo].off : 0, KS > 0 ? sp[jo].cap : 0, nullptr,
                       ltmp, -1, bc, bz, bb, bs, bg, bytes, nodes))
        return false;
    }
    if (j == 0) {
      if (NEAREST) {
        gbest = (double)bb;
        gsecond = (double)bs;
        ggrp = bg;
      }
    } else {
      sp[j - 1].best = (double)bb;
      sp[j - 1].second = (double)bs;
      sp[j - 1].grp = bg;
    }
    if (j < KS) sp[j < KS ? j : 0].cnt = bc;
  }
  if (NEAR && threadIdx.x == 0) {
    sh.wave_cnt[0] = cnt;
    sh.wave_start[0] = 0;
    sh.fa = zc;
  }
  lds_barrier();
  if (NEAR && zskip) *zskip = gz >= 0 ? zc : 0;
  total = NEAR ? cnt : 0;
  g.bytes = bytes;
  g.nodes = nodes;
  return true;
}

// scan2q, answered from the grid index when the instance has one (one-wave shape, trees of at least min_n nodes) and it
// can answer exactly; g.bytes / g.nodes: what the pass read
template <bool NEAR, bool NEAREST, int KS = 0>
__device__ __forceinline__ int scan2g(GridS& g, int rwn, const uint32_t* __restrict__ xq, int n, uint32_t qq, uint32_t thr,
                                      uint32_t sq, int32_t* __restrict__ hits, Sh2& sh, int& ggrp, double& gbest,
                                      double& gsecond, uint32_t gq = 0u, int gz = -1, int* zskip = nullptr,
                                      SpecQ* sp = nullptr) {
  if constexpr (NW == 1) {
    if (g.ok && n >= g.min_n) {
      int total = 0;
      if (grid_pass<NEAR, NEAREST, KS>(g, rwn, qq, thr, sq, hits, sh, ggrp, gbest, gsecond, gz, zskip, sp, total))
        return total;
    }
  }
  g.bytes = 4 * n;
  g.nodes = n;
  return scan2q<NEAR, NEAREST, KS>(xq, n, qq, thr, sq, hits, sh, ggrp, gbest, gsecond, gq, gz, zskip, sp);
}

// The node of the group [grp, grp + 4) whose grid distance to the query `sq` is `best`; lanes 0..3 of every wave hold
// the f64 coordinates (hx, hy) of the group's nodes, lane L those of node grp + (L & 3) (n = tree size the pass saw).  False when no node matches (the
// caller then repeats the query one stage down).
__device__ __forceinline__ bool resolve_group(const Ctx& c, int grp, int n, double hx, double hy, uint32_t sq,
                                              uint32_t best, int& ni, double& nx, double& ny) {
  const int lane = threadIdx.x & 63;
  bool m = false;
  if (lane < 4 && grp + lane < n) m = qdist(rppk::quant16(c, hx, hy), sq) == best;
  const uint64_t mk = __ballot(m);
  if (mk == 0ull) return false;
  const int j = __ffsll((long long)mk) - 1;
  ni = grp + j;
  nx = __shfl(hx, j);
  ny = __shfl(hy, j);
  return true;
}

// h-th hit of a 16-bit pass (scan2q, the grid index, a ride): index from the LDS capture (else the global list),
// coordinates gathered in f64
__device__ __forceinline__ void hit_at2q(const double* __restrict__ x, const double* __restrict__ y,
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
  idx = (h < HWF) ? reinterpret_cast<const int32_t*>(sh.u.hit)[k * HWF + h] : hits[sh.wave_start[k] + h];
  hx = x[idx];
  hy = y[idx];
}

// Exact re-check (dx**2 + dy**2 <= r**2 with the reference's libm pow) + the `.index` de-dup of rrt_04:1337,
// producing the candidate records.  cost / first_child of each distinct candidate are requested here and first
// used after the edge evaluation.
__device__ __forceinline__ void build_candidates(const double* __restrict__ x, const double* __restrict__ y,
                                                 const double* __restrict__ cost,
                                                 const int32_t* __restrict__ first_child, double qx, double qy,
                                                 double thr_exact, const int32_t* hits, int kraw, Sh2& sh,
                                                 int& pend_p, double& pend_cost, int& pend_fc) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  pend_p = -1;
  pend_cost = 0.0;
  pend_fc = -1;
  if (tid == 0) {
    sh.nu = 0;
    sh.nvalid = 0;
  }
  lds_barrier();
  // Fast mode: the reference's value v = dx**2 + dy**2 (libm pow) is within 2^-51 relative of vf = dx*dx + dy*dy
  // (correctly rounded squares), so
  //   * vf outside [r2 (1 - eps), r2 (1 + eps)], eps = 2^-47, decides `v <= r**2` (:1335-1337) without pow;
  //   * two hits can hold the SAME v (the `.index` collapse) only if their vf differ by less than eps vf; hits with
  //     identical coordinates certainly do -- the duplicated goal nodes of SURVEY R6: an iteration that extends from
  //     the goal sees every one of them (thousands by the end of a 100 k-node tree), so the raw list is walked in
  //     chunks of NFAST hits, each compared with the distinct candidates found so far and with its own chunk.
  // A hit in the band, or a close pair with different coordinates, sends the whole list to the exact evaluation below
  // (the boundary case, not the rule).
  constexpr int NFAST = TPB < NU ? TPB : NU;
  {
    bool exact = false;
    for (int base = 0; base < kraw && !exact; base += NFAST) {
      const int h = base + tid;
      const bool act = tid < NFAST && h < kraw;
      int idx = -1;
      double vf = 0.0, hx = 0.0, hy = 0.0;
      int st = 0;   // 0 outside, 1 inside, 2 in the band
      if (act) {
        hit_at2q(x, y, hits, sh, h, idx, hx, hy);
        vf = rpp::fast_d2(hx - qx, hy - qy);
        st = vf <= thr_exact * (1.0 - FILTER_EPS) ? 1 : (vf > thr_exact * (1.0 + FILTER_EPS) ? 0 : 2);
        sh.cval[tid] = vf;
        sh.uex[tid] = hx;   // scratch until the edge evaluation fills uex / uey
        sh.uey[tid] = hy;
      }
      sh.cflag[tid] = st;
      lds_barrier();
      const int nu = sh.nu;
      bool need = st == 2, first = st == 1;
      if (st == 1) {
        for (int u = 0; u < nu && first; u++) {   // candidates of earlier chunks (uval holds their vf)
          const double vt = sh.uval[u];
          const double dv = vt > vf ? vt - vf : vf - vt;
          if (dv <= FILTER_EPS * vf) {
            if (sh.ux[u] == hx && sh.uy[u] == hy)
              first = false;
            else
              need = true;
          }
        }
        for (int t = 0; t < tid && first; t++) {   // earlier hits of this chunk
          if (sh.cflag[t] == 0) continue;
          const double vt = sh.cval[t];
          const double dv = vt > vf ? vt - vf : vf - vt;
          if (dv <= FILTER_EPS * vf) {
            if (sh.uex[t] == hx && sh.uey[t] == hy)
              first = false;   // same coordinates as an earlier hit: same value, that one holds it
            else
              need = true;     // different nodes, values possibly equal: decide with the exact form
          }
        }
      }
      if (block_any(need, sh)) {
        exact = true;
        break;
      }
      const uint64_t mf = __ballot(first), mv = __ballot(st == 1);
      if (lane == 0) {
        sh.red_idx[w] = __popcll(mf);
        atomicAdd(&sh.nvalid, __popcll(mv));
      }
      lds_barrier();
      int off = nu, tot = nu;
#pragma unroll
      for (int k = 0; k < NW; k++) {
        if (k < w) off += sh.red_idx[k];
        tot += sh.red_idx[k];
      }
      if (first) {
        const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        const int p = off + __popcll(mf & lt_mask);
        if (p < NU) {
          sh.uval[p] = vf;
          sh.uidx[p] = idx;
          sh.ux[p] = hx;
          sh.uy[p] = hy;
          if (kraw <= NFAST) {
            // single chunk (the common case): keep the two loads in flight, the caller stores them into the record
            // after the edge evaluation that does not need them
            pend_p = p;
            pend_cost = cost[idx];
            pend_fc = first_child[idx];
          } else {
            sh.ucur[p] = cost[idx];
            sh.ufc[p] = first_child[idx];
          }
        }
      }
      lds_barrier();
      if (tid == 0) {
        if (tot > NU) {
          sh.overflow = 1;
          tot = NU;
        }
        sh.nu = tot;
      }
      lds_barrier();
    }
    if (!exact) return;
    pend_p = -1;
    if (tid == 0) {
      sh.nu = 0;
      sh.nvalid = 0;
    }
    lds_barrier();
  }
  for (int base = 0; base < kraw; base += TPB) {
    const int h = base + tid;
    int idx = -1;
    double v = 0.0, hx = 0.0, hy = 0.0;
    bool valid = false;
    if (h < kraw) {
      hit_at2q(x, y, hits, sh, h, idx, hx, hy);
      v = rpp::py_d2(hx - qx, hy - qy);
      valid = v <= thr_exact;
    }
    const int nu = sh.nu;
    bool cand = valid;
    if (cand) {
      for (int u = 0; u < nu; u++) {
        if (sh.uval[u] == v) {
          cand = false;
          break;
        }
      }
    }
    sh.cval[tid] = v;
    sh.cflag[tid] = cand ? 1 : 0;
    lds_barrier();
    bool first = cand;
    if (cand) {
      for (int t = 0; t < tid; t++) {
        if (sh.cflag[t] && sh.cval[t] == v) {
          first = false;
          break;
        }
      }
    }
    const uint64_t mf = __ballot(first), mv = __ballot(valid);
    if (lane == 0) {
      sh.red_idx[w] = __popcll(mf);
      atomicAdd(&sh.nvalid, __popcll(mv));
    }
    lds_barrier();
    int off = nu;
#pragma unroll
    for (int k = 0; k < NW; k++)
      if (k < w) off += sh.red_idx[k];
    int tot = nu;
#pragma unroll
    for (int k = 0; k < NW; k++) tot += sh.red_idx[k];
    if (first) {
      const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
      const int p = off + __popcll(mf & lt_mask);
      if (p < NU) {
        sh.uval[p] = v;
        sh.uidx[p] = idx;
        sh.ux[p] = hx;
        sh.uy[p] = hy;
        if (kraw <= TPB) {
          // single chunk (the common case): keep the two loads in flight, the caller stores them into the record
          // after the edge evaluation that does not need them
          pend_p = p;
          pend_cost = cost[idx];
          pend_fc = first_child[idx];
        } else {
          sh.ucur[p] = cost[idx];
          sh.ufc[p] = first_child[idx];
        }
      }
    }
    lds_barrier();
    if (tid == 0) {
      if (tot > NU) {
        sh.overflow = 1;
        tot = NU;
      }
      sh.nu = tot;
    }
    lds_barrier();
  }
}

// check_collision (rrt_04:1216-1230) of one edge against one obstacle with the edge's points taken along the straight line
// from `f` with the step (sx, sy) -- an approximation of the reference's polyline to a few ULP -- and a tolerance band about
// the threshold: 1 = some point is inside by more than tol (a hit whatever the exact points are), 0 = every point is
// outside by more than tol, 2 = a point lies in the band (only the exact polyline can tell).
__device__ __forceinline__ int edge_hits_obstacle_band(const rpp::Edge& e, bool snapped, double ox, double oy, double thr,
                                                       double tol) {
  double px = e.fx, py = e.fy;
  double dx = ox - px, dy = oy - py;
  double dmin = dx * dx + dy * dy;
  for (int i = 0; i < e.n_expand; i++) {
    px += e.sx;
    py += e.sy;
    dx = ox - px;
    dy = oy - py;
    const double dd = dx * dx + dy * dy;
    dmin = dd < dmin ? dd : dmin;
  }
  if (snapped) {
    dx = ox - e.tx;
    dy = oy - e.ty;
    const double dd = dx * dx + dy * dy;
    dmin = dd < dmin ? dd : dmin;
  }
  return dmin <= thr - tol ? 1 : (dmin <= thr + tol ? 2 : 0);
}

// Obstacles that can matter to a candidate edge of this iteration (one-wave shape, om <= 64): bit k of the wave-uniform
// result is CLEAR only when obstacle k gives 0 in edge_hits_obstacle_band and false in rpp::edge_hits_obstacle for every
// edge eval_edges_dual2 / eval_edges_back2 test, so leaving it out changes no flag.  Lane k tests
//     |n - o_k|  <=  sqrt(othr_k + tolmax) + R + slack            (a NaN anywhere keeps the obstacle)
// about the new node n = (nx, ny), with R = sqrt(r2):
//   * every point such an edge tests lies within R + delta of n.  A candidate u entered the list with |u - n|^2 <= r2 up
//     to 2^-46 relative (build_candidates: vf <= r2 (1 - eps) in the fast mode, the reference's v <= r2 in the exact one;
//     v and vf are within 2^-51 relative of the true square), so u is in the ball; n is its centre; the winner's end
//     point w (eval_edges_back2's origin) is a point of the edge u_sel -> n; the ball is convex, so the segments u - n
//     and w - u are inside.  The points walked are f + i s with i <= n_expand and n_expand res <= d: on the segment up to
//     the rounding of n_expand < 2^31 additions, each below 2^-53 of a coordinate -> delta < 2^-21 (|n| + R) per axis;
//     the exact polyline's step res (cos, sin) differs from res (dx, dy) / d by a few ULP of res, n_expand times:
//     below 2^-50 R.  Both are far inside the relative part of the slack, 1e-5 (1 + |n| + |o| + R);
//   * band test: non-zero needs dmin <= othr + tol with tol = 1e-10 (1 + |fx| + |fy| + |ox| + |oy|) (4 + othr); f is in
//     the ball, |fx| + |fy| <= |nx| + |ny| + 2 (R + delta), so tol <= tolmax as written below (its factor 2 pays for delta
//     and the roundings);
//   * the roundings of this test and of the dd = dx dx + dy dy it stands in for are relative 2^-50: the absolute 1e-3 map
//     units and the relative part leave them ten orders of magnitude.
// A culled obstacle therefore has every tested point further than sqrt(othr + tolmax) + ~1e-3 from its centre.
__device__ __forceinline__ uint64_t obstacle_mask(int om, double nx, double ny, double r2, const Sh2& sh) {
  const int k = threadIdx.x & 63;
  bool keep = false;
  if (k < om) {
    const double ox = sh.ox[k], oy = sh.oy[k], thr = sh.othr[k];
    const double R = __builtin_sqrt(r2);
    const double mag = 1.0 + rpp::dabs(nx) + rpp::dabs(ny) + rpp::dabs(ox) + rpp::dabs(oy);
    const double tolmax = 2e-10 * (mag + 2.0 * R) * (4.0 + thr);
    const double reach = __builtin_sqrt(thr + tolmax) + R + (1e-3 + 1e-5 * (mag + R));
    const double dx = ox - nx, dy = oy - ny;
    keep = !(__builtin_sqrt(dx * dx + dy * dy) > reach);
  }
  return __ballot(keep);
}

// The exact form of a candidate edge (eval_edges_dual2): the reference's atan2 / cos / sin, the sequential additions and
// the snap test; `e` gets the exact step, end point and snap bit.
__device__ __forceinline__ void edge_exact_steer(rpp::Edge& e, double res) {
  const double dx = e.tx - e.fx, dy = e.ty - e.fy;
  const double theta = rpp_glibc_atan2(dy, dx);
  e.sx = res * rpp_glibc_cos(theta);
  e.sy = res * rpp_glibc_sin(theta);
  double px = e.fx, py = e.fy;
  for (int i = 0; i < e.n_expand; i++) {
    px += e.sx;
    py += e.sy;
  }
  const int snapped = rpp::py_hypot(e.tx - px, e.ty - py) <= res;
  e.ex = snapped ? e.tx : px;
  e.ey = snapped ? e.ty : py;
  e.snapped = snapped;
}

// Both directions of every candidate edge (see eval_edges_dual in v1), coordinates from the LDS records:
// choose_parent's steer(node -> new) :1265 and rewire's steer(new -> node) :1359 with their collision tests.
//
// WITHOUT the libm calls in the usual case.  steer (:1086-1115) needs theta = atan2, cos, sin only for the polyline points
// p_i = from + i * res * (cos theta, sin theta); what the callers use of an edge is (a) its length d = hypot (no libm),
// (b) n_expand = floor(d / res) (no libm), (c) whether the walk ends snapped on the target -- hypot(target - p_n) <= res,
// i.e. d - n res <= res up to the roundings of the n additions -- and then the end point IS the target, (d) the collision
// verdict over the points.  (res cos theta, res sin theta) equals res (dx, dy) / d to a few ULP, so:
//   * d - n res <= res (1 - 1e-9) decides "snapped" (the reference's sum differs from n res d-hat by ~n ULP);
//   * the points along the straight line decide the collision test against an obstacle unless the closest point lies
//     within `tol` (~1e-7: 10^6 times the differences in play) of the obstacle's threshold (edge_hits_obstacle_band).
// An edge with either decision in doubt -- in practice the edge from the NEAREST node, whose length is 8 x 0.25 = 2.0 give
// or take an ULP, in about every second iteration -- is evaluated again exactly as before (atan2 / cos / sin replicas, the
// sequential additions, the exact test), by its own lane alone instead of all candidates' lanes diverging in the replicas.
//
// `cull` (one-wave shape only, obstacle_mask above): one edge per lane, held in registers, against the obstacles of `omask`
// alone -- no (edge, obstacle) pair decoding, no re-read of the edge, and nothing at all to test when the mask is empty
// (an edge in doubt about its snap still takes its exact steer).  Same flags and end points as the pair loops.
__device__ __forceinline__ void eval_edges_dual2(const Ctx& c, int om, int nu, double nx, double ny, Sh2& sh,
                                                 bool cull, uint64_t omask) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // 4 waves: direction = w>>1 (even waves work, odd ones only take part in the pair loops); 2 waves: direction = w;
  // 1 wave: direction = lane>>5 (both half-waves run the same instruction stream)
  static_assert(NW != 1 || EBD <= 32, "one-wave shape: both directions share a wave");
  const int kind = (NW >= 4) ? (w >> 1) : (NW == 2 ? w : (lane >> 5));
  const int trig = (NW >= 4) ? (w & 1) : 0;
  const int el = (NW == 1) ? (lane & 31) : lane;
  for (int base = 0; base < nu; base += EBD) {
    const int nb = (nu - base) < EBD ? (nu - base) : EBD;
    const bool act = el < nb && w < 4 && trig == 0;
    rpp::Edge& E = sh.u.edge[kind * EBD + (el & (EBD - 1))];
    bool unsure = false;
    if (act) {
      const double ux = sh.ux[base + el], uy = sh.uy[base + el];
      const double fx = kind ? nx : ux, fy = kind ? ny : uy, tx = kind ? ux : nx, ty = kind ? uy : ny;
      const double dx = tx - fx, dy = ty - fy;
      const double d = rpp::py_hypot(dx, dy);
      const int ne = (int)__builtin_floor(d / c.res);
      const double sc = d > 0.0 ? c.res / d : 0.0;
      E.sx = sc * dx;
      E.sy = sc * dy;
      E.fx = fx; E.fy = fy; E.tx = tx; E.ty = ty;
      E.n_expand = ne;
      if (kind == 0) sh.uhyp[base + el] = d;
      // snapped unless the remaining distance is within 1e-9 res of res (then only the exact additions can tell)
      unsure = !(d - (double)ne * c.res <= c.res * (1.0 - 1e-9));
      E.ex = tx;
      E.ey = ty;
      E.snapped = unsure ? 4 : 1;   // bit 2: to be evaluated exactly
      sh.cflag[kind * EBD + el] = 0;   // collision flags of this pass
    }
    if (NW == 1 && cull) {
      if (act) {
        rpp::Edge ed;
        ed.fx = E.fx; ed.fy = E.fy; ed.sx = E.sx; ed.sy = E.sy; ed.tx = E.tx; ed.ty = E.ty;
        ed.ex = ed.tx; ed.ey = ed.ty;
        ed.n_expand = E.n_expand;
        ed.snapped = 1;
        int hit = 0, band = 0;
        if (!unsure) {
          for (uint64_t m = omask; m; m &= m - 1) {
            const int k = __builtin_ctzll(m);
            const double tol = 1e-10 * (1.0 + rpp::dabs(ed.fx) + rpp::dabs(ed.fy) + rpp::dabs(sh.ox[k]) + rpp::dabs(sh.oy[k])) *
                               (4.0 + sh.othr[k]);
            const int r = edge_hits_obstacle_band(ed, true, sh.ox[k], sh.oy[k], sh.othr[k], tol);
            hit |= r == 1;
            band |= r == 2;
          }
        }
        if (unsure || (band && !hit)) {
          edge_exact_steer(ed, c.res);
          E.sx = ed.sx;
          E.sy = ed.sy;
          E.ex = ed.ex;
          E.ey = ed.ey;
          E.snapped = ed.snapped | 16;
          hit = 0;
          for (uint64_t m = omask; m; m &= m - 1) {
            const int k = __builtin_ctzll(m);
            if (rpp::edge_hits_obstacle(ed, sh.ox[k], sh.oy[k], sh.othr[k])) hit = 1;
          }
        }
        sh.cflag[kind * EBD + el] = hit;
      }
      lds_barrier();
    } else {
    lds_barrier();
    for (int p = tid; p < 2 * nb * om; p += TPB) {
      const int q = p / om, k = p - q * om;
      const int kk = q / nb, e = q - kk * nb;
      const int slot = kk * EBD + e;
      const rpp::Edge& ed = sh.u.edge[slot];
      if (ed.snapped & 4) continue;   // goes through the exact form anyway
      const double tol = 1e-10 * (1.0 + rpp::dabs(ed.fx) + rpp::dabs(ed.fy) + rpp::dabs(sh.ox[k]) + rpp::dabs(sh.oy[k])) *
                         (4.0 + sh.othr[k]);
      const int r = edge_hits_obstacle_band(ed, true, sh.ox[k], sh.oy[k], sh.othr[k], tol);
      if (r == 1) sh.cflag[slot] = 1;
      if (r == 2) atomicOr(&sh.u.edge[slot].snapped, 8);   // bit 3: an obstacle in the band
    }
    lds_barrier();
    // ---- the exact form for edges left in doubt (and not already known to collide)
    const bool redo = act && ((E.snapped & 4) || ((E.snapped & 8) && !sh.cflag[kind * EBD + el]));
    if (block_any(redo, sh)) {
      if (redo) {
        rpp::Edge ed = E;
        edge_exact_steer(ed, c.res);
        E.sx = ed.sx;
        E.sy = ed.sy;
        E.ex = ed.ex;
        E.ey = ed.ey;
        E.snapped = ed.snapped | 16;   // bit 4: exact polyline in place
        sh.cflag[kind * EBD + el] = 0;
      }
      lds_barrier();
      for (int p = tid; p < 2 * nb * om; p += TPB) {
        const int q = p / om, k = p - q * om;
        const int kk = q / nb, e = q - kk * nb;
        const int slot = kk * EBD + e;
        if (!(sh.u.edge[slot].snapped & 16)) continue;
        rpp::Edge ee = sh.u.edge[slot];
        ee.snapped &= 1;
        if (rpp::edge_hits_obstacle(ee, sh.ox[k], sh.oy[k], sh.othr[k])) sh.cflag[slot] = 1;
      }
      lds_barrier();
    }
    }
    if (tid < nb) {
      const rpp::Edge& f = sh.u.edge[tid];
      const rpp::Edge& b = sh.u.edge[EBD + tid];
      sh.uex[base + tid] = f.ex;
      sh.uey[base + tid] = f.ey;
      const int s0 = (!sh.cflag[tid]) && rpp::in_play_area(c.has_play, c.play_area, f.ex, f.ey);
      const int s1 = (!sh.cflag[EBD + tid]) && rpp::in_play_area(c.has_play, c.play_area, b.ex, b.ey);
      const int s2 = (b.ex == b.tx) && (b.ey == b.ty);
      sh.uflag[base + tid] = s0 | (s1 << 1) | (s2 << 2);
    }
    lds_barrier();
  }
}

// backward edges only, from the true new-node position (the winning edge did not snap): refresh bits 1,2 + uhyp
// (`cull`: as in eval_edges_dual2 -- w is a point of the winning edge, inside the ball obstacle_mask covers)
__device__ __forceinline__ void eval_edges_back2(const Ctx& c, int om, int nu, double wx, double wy, Sh2& sh,
                                                 bool cull, uint64_t omask) {
  const int tid = threadIdx.x;
  for (int base = 0; base < nu; base += 2 * EBD) {
    const int nb = (nu - base) < 2 * EBD ? (nu - base) : 2 * EBD;
    if (NW == 1 && cull) {
      if (tid < nb) {
        rpp::Edge ed;
        rpp::steer(&ed, wx, wy, sh.ux[base + tid], sh.uy[base + tid], rpp::dinf(), c.res);
        sh.u.edge[tid] = ed;
        sh.uhyp[base + tid] = rpp::py_hypot(sh.ux[base + tid] - wx, sh.uy[base + tid] - wy);
        int hit = 0;
        for (uint64_t m = omask; m; m &= m - 1) {
          const int k = __builtin_ctzll(m);
          if (rpp::edge_hits_obstacle(ed, sh.ox[k], sh.oy[k], sh.othr[k])) hit = 1;
        }
        sh.cflag[tid] = hit;
      }
      lds_barrier();
    } else {
    if (tid < nb) {
      rpp::steer(&sh.u.edge[tid], wx, wy, sh.ux[base + tid], sh.uy[base + tid], rpp::dinf(), c.res);
      sh.uhyp[base + tid] = rpp::py_hypot(sh.ux[base + tid] - wx, sh.uy[base + tid] - wy);
      sh.cflag[tid] = 0;
    }
    lds_barrier();
    for (int p = tid; p < nb * om; p += TPB) {
      const int e = p / om, k = p - e * om;
      if (rpp::edge_hits_obstacle(sh.u.edge[e], sh.ox[k], sh.oy[k], sh.othr[k])) sh.cflag[e] = 1;
    }
    lds_barrier();
    }
    if (tid < nb) {
      const rpp::Edge& e = sh.u.edge[tid];
      const int s = (!sh.cflag[tid]) && rpp::in_play_area(c.has_play, c.play_area, e.ex, e.ey);
      const int s2 = (e.ex == e.tx) && (e.ey == e.ty);
      sh.uflag[base + tid] = (sh.uflag[base + tid] & 1) | (s << 1) | (s2 << 2);
    }
    lds_barrier();
  }
}

// ---- scalar-path tree walks -------------------------------------------------------------------------------------
// A dependent VECTOR load costs 1.1 - 1.7 us while the other waves of the CU stream (it queues behind their loads in
// the CU's vector memory pipeline); a SCALAR load of the same address takes the scalar data path to L2 and costs
// 0.35 - 0.4 us under the same load (tools/ubench/lat_ubench.hip, profiles/r2_lat_ubench.txt).  The pointer chases of
// rewire -- a node's sibling links, the cost propagation over its subtree -- read one address at a time, so they run
// on the scalar unit: s_load with glc (served by L2, never by a stale scalar-cache line; the scalar cache is not
// coherent with vector stores).  The arrays are written by THIS wave's vector stores only, which reach L2 before
// `s_waitcnt vmcnt(0)` returns; the callers place that wait where an earlier store of the iteration could be read.
__device__ __forceinline__ void sload3(const int32_t* pa, const int32_t* pb, const int32_t* pc, int& a, int& b,
                                       int& c) {
  uint32_t ra, rb, rc;
  asm volatile(
      "s_load_dword %0, %3, 0x0 glc\n\ts_load_dword %1, %4, 0x0 glc\n\ts_load_dword %2, %5, 0x0 glc\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&s"(ra), "=&s"(rb), "=&s"(rc)
      : "s"(pa), "s"(pb), "s"(pc)
      : "memory");
  a = (int)ra;
  b = (int)rb;
  c = (int)rc;
}
// {next_sib, first_child, elen} of one node: one scalar round trip
__device__ __forceinline__ void sload_node(const int32_t* next_sib, const int32_t* first_child, const double* elen,
                                           int node, int& nxs, int& fcc, double& el) {
  const int32_t* pa = next_sib + node;
  const int32_t* pb = first_child + node;
  const double* pc = elen + node;
  uint32_t ra, rb;
  uint64_t rc;
  asm volatile(
      "s_load_dword %0, %3, 0x0 glc\n\ts_load_dword %1, %4, 0x0 glc\n\ts_load_dwordx2 %2, %5, 0x0 glc\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&s"(ra), "=&s"(rb), "=&s"(rc)
      : "s"(pa), "s"(pb), "s"(pc)
      : "memory");
  nxs = (int)ra;
  fcc = (int)rb;
  el = rpp::b2d(rc);
}

constexpr int CE = (NU + 63) / 64;   // near candidates per lane when a wave holds the candidate list in registers

// Inst::phase[PROP_WALK_SLOT] (a slot no phase timer of this kernel uses) counts the walks propagate_lanes finished,
// plus PROP_WALK_FULL for each one whose pending list ran full (rrtx_get_phase_cycles; tests and diagnostics)
constexpr int PROP_WALK_SLOT = 10;
// Obstacle-cull counts (diagnostic build only; this kernel stamps no phase 12 and no phase 15, their spans -- the overflow
// check and the loop head -- fall to the next stamp, "sample"): Inst::phase[CULL_POP_SLOT] sums the popcounts of the
// masks, Inst::phase[CULL_EVAL_SLOT] counts the iterations that evaluated candidate edges under a mask (low 32 bits) and
// those whose mask was empty (from bit 32 on).  Both halves are at most the plan's iteration count summed over the
// instances: tools/phase_profile.py prints them only while that sum is below 2^32 (the low half cannot have carried).
constexpr int CULL_POP_SLOT = 12, CULL_EVAL_SLOT = 15;
#ifdef RRTX_PHASE_TIMERS
#define CULL_COUNT(m) do { if (threadIdx.x == 0) { ph_[CULL_POP_SLOT] += (int64_t)__popcll(m); \
                                                   ph_[CULL_EVAL_SLOT] += 1ll + ((m) ? 0ll : (1ll << 32)); } } while (0)
#else
#define CULL_COUNT(m) do { } while (0)
#endif
constexpr unsigned long long PROP_WALK_FULL = 1ull << 40;
// set bits of m below this lane
__device__ __forceinline__ int lanes_below(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// The rest of a cost walk with one sibling chain per lane (one-wave shape).  Every round trip gathers {next_sib,
// first_child, elen} of up to 64 nodes, one per lane: a node's first child continues its lane's chain (at the node's new
// cost), its next sibling joins the LDS list of pending chains (at the parent's cost), and idle lanes take pending
// chains at the start of each round.  The rounds are bounded by the height of the first-child / next-sibling tree, not
// by the node count: in the long tail of propagations (thousands of nodes, DESIGN 5.2) that is several times fewer
// round trips, each a dependent vector gather.  (cur, cp) and st[0, sp) are what the scalar walk left.  Returns the nodes
// rewritten, or -1 when more than `cap` chains are pending.  Near candidates' LDS costs are not refreshed: the caller
// re-reads them.
__device__ __forceinline__ int propagate_lanes(double* __restrict__ cost, const int32_t* first_child,
                                               const int32_t* next_sib, const double* elen, int cur, double cp,
                                               Sh2& sh, int sp, int cap) {
  const int lane = threadIdx.x & 63;
  WalkEnt* st = sh.u.walk;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // lane 0's stores of this rewire, before other lanes read
  sh.cflag[lane] = lane == 0 ? cur : -1;
  sh.cval[lane] = cp;
  int cnt = 0;
  for (;;) {
    int vn = sh.cflag[lane];
    const uint64_t idle = __ballot(vn < 0);
    const int take = min(__popcll(idle), sp);
    const int r = lanes_below(idle);
    if (vn < 0 && r < take) {
      vn = st[sp - 1 - r].node;
      sh.cval[lane] = st[sp - 1 - r].cp;
    }
    sp -= take;
    const uint64_t act = __ballot(vn >= 0);
    if (act == 0ull) break;
    int nxs = -1, fcc = -1;
    double el = 0.0;
    if (vn >= 0) {
      nxs = next_sib[(uint32_t)vn];
      fcc = first_child[(uint32_t)vn];
      el = elen[(uint32_t)vn];
    }
    const double vcp = sh.cval[lane];
    const double nc = vcp + el;   // calc_new_cost :1375-1377
    if (vn >= 0) cost[(uint32_t)vn] = nc;
    cnt += __popcll(act);
    const bool fork = fcc >= 0 && nxs >= 0;
    const uint64_t fm = __ballot(fork);
    if (sp + __popcll(fm) > cap) return -1;
    if (fork) {
      const int k = sp + lanes_below(fm);
      st[k].cp = vcp;
      st[k].node = nxs;
    }
    sp += __popcll(fm);
    sh.cflag[lane] = fcc >= 0 ? fcc : nxs;
    if (fcc >= 0) sh.cval[lane] = nc;
    __builtin_amdgcn_wave_barrier();
  }
  return cnt;
}

// propagate_cost_to_leaves (rrt_04:1379-1384) as a depth-first walk on the scalar unit, run by ONE wave (all lanes in
// step, values uniform): every descendant of the rewired node gets cost = parent cost + elen (the cached hypot of
// calc_new_cost :1375-1377), written by lane 0.  A descendant that is itself a near candidate of this iteration has
// its LDS cost refreshed on the way (the sequential order of :1357-1373 reads it later); my_uidx[k] = index of the
// candidate lane + 64 k (or -1).  A walk still running after vec_after nodes (>= 0) goes on with propagate_lanes, and
// `reread` tells the caller to refresh the later candidates' LDS costs from cost[].  Returns the nodes rewritten, or -1
// when the sibling stack (LDS, at most cap entries) is full: the caller redoes the subtree with the global-stack walk
// (recomputation is idempotent).
__device__ __forceinline__ int propagate_scalar(double* __restrict__ cost, const int32_t* first_child,
                                                const int32_t* next_sib, const double* elen, int root_fc,
                                                double root_cost, Sh2& sh, const int (&my_uidx)[CE], int vec_after,
                                                int cap, bool& reread, unsigned long long* walks) {
  WalkEnt* st = sh.u.walk;
  constexpr int CAP = 2 * FCAP * (int)(sizeof(Front) / sizeof(WalkEnt));
  cap = min(cap, CAP);
  const int lane = threadIdx.x & 63;
  int sp = 0, cnt = 0;
  int cur = root_fc;
  double cp = root_cost;
  for (;;) {
    if (cur < 0) {
      if (sp == 0) break;
      sp--;
      cur = __builtin_amdgcn_readfirstlane(st[sp].node);
      cp = st[sp].cp;
      continue;
    }
    if (vec_after >= 0 && cnt >= vec_after) {
      reread = true;
      const int r = propagate_lanes(cost, first_child, next_sib, elen, cur, cp, sh, sp, cap);
      if (lane == 0) atomicAdd(walks, r < 0 ? PROP_WALK_FULL : 1ull);   // no return value: nothing waits on it
      return r < 0 ? -1 : cnt + r;
    }
    int nxs, fcc;
    double el;
    sload_node(next_sib, first_child, elen, cur, nxs, fcc, el);
    const double nc = cp + el;   // calc_new_cost :1375-1377
    if (lane == 0) cost[cur] = nc;
#pragma unroll
    for (int k = 0; k < CE; k++)
      if (my_uidx[k] == cur) sh.ucur[lane + 64 * k] = nc;
    cnt++;
    if (fcc >= 0) {
      if (nxs >= 0) {
        if (sp >= cap) return -1;
        if (lane == 0) {
          st[sp].cp = cp;
          st[sp].node = nxs;
        }
        sp++;
      }
      cur = fcc;
      cp = nc;
    } else {
      cur = nxs;
    }
  }
  return cnt;
}

// ---------------------------------------------------------------------------
// Near and nearest queries start at the 16-bit mirror xq[] (the grid index in the one-wave shape, else streaming:
// scan2g); a nearest query that stage cannot decide goes to the f64 pass (scan2), then the exact ** 2 rescan.
__global__ __launch_bounds__(TPB, WPS) void rrt_star_kernel_v2(Ctx c, int iters) {
  __shared__ Sh2 sh;
  const int inst = c.inst_map ? c.inst_map[blockIdx.x] : blockIdx.x;
  const int tid = threadIdx.x;
  Inst* I = c.inst + inst;
  if (I->status & 1) return;
  const int64_t off = (int64_t)inst * c.stride;
  double* __restrict__ x = c.x + off;
  double* __restrict__ y = c.y + off;
  double* __restrict__ cost = c.cost + off;
  int32_t* parent = c.parent + off;
  int32_t* first_child = c.first_child + off;
  int32_t* next_sib = c.next_sib + off;
  int32_t* prev_sib = c.prev_sib + off;
  int32_t* hits = c.hits + off;
  int32_t* stack = c.stack + off;
  double* __restrict__ elen = c.elen + off;
  uint32_t* __restrict__ xq = c.xq + off;
  const double qm = c.q_m;
  const double qinv = c.q_inv;   // world -> grid units of the 16-bit mirror
  const double qm_grid = c.q_m * c.q_inv;
  const uint32_t goal_q = rppk::quant16(c, I->goal[0], I->goal[1]);   // the goal's grid cell
  int q_amb = 0;            // the fused 16-bit pass could not decide the pending nearest query ...
  uint32_t q_amb_bq = 0u;   // ... and this bounds the nearest node's squared grid distance (candidate pass, below)
  int first_goal = I->first_goal;
  int goal_dups = I->goal_dups;   // exact duplicates of node first_goal appended so far (valid while first_goal >= 0)

  for (int i = tid; i < 624; i += TPB) sh.rng.mt[i] = I->rng.mt[i];
  // this instance's obstacle rows, block-uniform.  The candidate-edge helpers take the count as an argument, the two loops
  // of the iteration body read it back from sh.om: with that split the streaming loops keep their ring of loads in flight
  // (tools/loop_spill_check.sh) and no shape spills more SGPRs than with one shared list
  const int om = uni_i(I->obs_m);
  {
    const int ob = uni_i(I->obs_base);
    for (int i = tid; i < om; i += TPB) {
      sh.ox[i] = c.ox[ob + i];
      sh.oy[i] = c.oy[ob + i];
      sh.othr[i] = c.othr[ob + i];
    }
    if (tid == 0) {
      sh.rng.pos = I->rng.pos;
      sh.overflow = 0;
      sh.om = om;
    }
  }
  lds_barrier();
  int n = __builtin_amdgcn_readfirstlane(I->n), it = __builtin_amdgcn_readfirstlane(I->it);   // block-uniform: keep them scalar
  const double gx = I->goal[0], gy = I->goal[1];
  rpp::Sobol sob = I->sobol;
  // grid index of the mirror (one-wave shape): rebuilt from xq[] at every launch, kept current at every xq[] write
  GridS gs = {};
  gs.ok = 0;
  if constexpr (NW == 1) {
    if (c.grid) {
      const int64_t gi = (int64_t)inst;
      gs.cnt = c.gcnt + gi * c.gcells;
      gs.blk = c.gblk + gi * c.gcells;
      gs.ent = c.gent + gi * c.gcells * GRID_CAP0;
      gs.pool = c.gpool + gi * c.gpool_blocks * GRID_CAP1;
      gs.sh = c.gsh;
      gs.gn = c.gn;
      gs.pool_blocks = c.gpool_blocks;
      gs.min_n = c.grid_min;
      gs.merge = c.grid_merge;
      gs.goal_q = goal_q;
      gs.ok = 1;
      grid_build(gs, xq, x, y, n, gx, gy, first_goal);
    }
  }
  if (tid == 0)
    for (int k = 0; k < 15; k++) sh.stat[k] = 0;
#define ST_ADD(k, v) do { if (tid == 0) sh.stat[k] += (long long)(v); } while (0)
  enum { S_ITER, S_EU, S_ER, S_NH, S_NU, S_RW, S_PR, S_SN, S_AB, S_AB2, S_EX, S_NUMAX, S_FB, S_QA, S_RIDE };
  int have_sample = 0, have_nearest = 0, ni = 0;
  double gbest = 0.0, gsecond = 0.0, nqx = 0.0, nqy = 0.0;   // nearest node of the current sample (block-uniform)
  int stop = 0;
  // ---- Several iterations per pass (one-wave shape, 16-bit stage; Ctx::spec2 = RRTX_SPEC2: 0 switches it off, 1..KSM
  // = further iterations a pass may serve) ------------------------------------------------------------------------------
  // Once the tree is dense the nearest node is closer than expand_dis, so steer() snaps onto the sample (:1108-1113):
  // the new node of iteration i+k IS sample i+k, and samples do not depend on the tree.  The pass of iteration i
  // therefore answers, from one read of xq[]: near(i) and nearest(i+1) as before, and for j = 0 .. ks-1 -- speculating
  // that iteration i+1+j's node lands on its sample -- the near ball of that iteration about its sample (radius of the
  // smallest tree it can meet, n+1: a superset for every later size, re-checked exactly like any hit list; hits into the
  // free tail of hits[]) and the nearest query of the sample after it.  Iteration i+1+j then needs no pass when its node
  // is bit for bit the speculated centre: the nodes appended since the pass join the ball by the grid test the pass
  // applies, in index order, and are folded into the nearest answer of the next sample.  A rejected extension in
  // between costs nothing (one node fewer to fold).  Anything else -- an unsnapped extension, a moved node, a ball that
  // reaches the goal's grid cell (the duplicate counting of scan2q_slot), a full list -- falls back to a pass of its own,
  // which starts the scheme again; samples are drawn ahead in stream order and used in that order whatever happens.
  // Bytes per iteration: 4 n -> 4 n / (1 + ks) while every iteration rides.
  // What the scheme carries from iteration to iteration lives in the instance's own global memory (the free tail of
  // hits[]: 256 doubles at hits[stride - 2560]), written by lane 0 and read back with wave-uniform loads -- a few loads
  // per iteration against a register file that the streaming loop needs whole: G[0..3 | 4..7] ring of samples drawn
  // ahead (x | y), G[8..11 | 12..15] nodes appended since the pass, G[16 + 8 e ..] set record e of a ring of four:
  // {centre x, y, nearest best, runner-up (world units squared), ball hits (-1: no ball), list offset, nearest group
  // (-1: none), best squared grid distance}.  Registers keep the ring heads and counts only.
  constexpr int SPEC_CAPS = 2048 / (KSM > 0 ? KSM : 1);   // hits[stride - 2048, stride): the balls' hit lists
  const int spec_base = (int)c.stride - 2048;
  double* __restrict__ G = reinterpret_cast<double*>(hits + ((int)c.stride - 2560));
  const int KS_RUN = NW == 1 ? (c.spec2 < KSM ? c.spec2 : KSM) : 0;
  const bool SPEC_ON = KS_RUN > 0;
  constexpr int KA = KSM > 0 ? KSM : 1;
  static_assert(KSM <= 3, "rings of four");
  int nq = 0, qhead = 0;                               // samples drawn ahead beyond the one in sh.rx / sh.ry
  int ns = 0, shead = 0;                               // query sets not yet used
  int na = 0;                                          // nodes appended since the pass: indices B_n .. B_n + na - 1
  int B_n = 0;                                         // tree size the pass scanned
  uint32_t B_thr = 0u;
  // the sample of the next iteration into sh.rx / sh.ry (the front of the queue, else a new draw); tid 0 writes
  auto take_next_sample = [&]() {
    if (nq > 0) {
      if (tid == 0) {
        sh.rx = G[qhead];
        sh.ry = G[4 + qhead];
      }
      qhead = (qhead + 1) & 3;
      nq--;
    } else if (tid == 0) {
      rppk::draw_sample(c, sh, sob, gx, gy);
    }
  };
  // Nearest node of the queue's front sample: the pass's answer (set record at shead) over [0, B_n) + the na nodes
  // appended since (indices B_n ..; the lowest index wins among equals, :1200).  The margin logic of fold_new_node below
  // with the nearest of the new nodes.  Returns 1 with the node in (ni, nqx, nqy), 2 when the 16-bit stage cannot
  // decide (o_bq bounds the squared grid distance), else 0.
  auto fold_n2 = [&](uint32_t& o_bq) -> int {
    const double* R = G + 16 + 8 * shead;
    const double s2x = G[qhead], s2y = G[4 + qhead];
    const double nb = R[2], nsec = R[3], grpd = R[6], bqd = R[7];
    double axv[4], ayv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      axv[j] = G[8 + j];
      ayv[j] = G[12 + j];
    }
    o_bq = 0xffffffffu;
    if (grpd < 0.0) return 0;
    if (first_goal >= 0 && s2x == gx && s2y == gy) {   // d == 0 on the goal, min() keeps the lowest index (:1200)
      ni = first_goal;
      nqx = gx;
      nqy = gy;
      gbest = 0.0;
      gsecond = rpp::dinf();
      return 1;
    }
    double dl = rpp::dinf(), lx = 0.0, ly = 0.0;
    int li = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (j < na) {
        const double dxl = axv[j] - s2x, dyl = ayv[j] - s2y;
        const double d1 = __builtin_sqrt(dxl * dxl + dyl * dyl);
        if (d1 < dl) {
          dl = d1;
          li = B_n + j;
          lx = axv[j];
          ly = ayv[j];
        }
      }
    }
    const double db = __builtin_sqrt(nb), ds = __builtin_sqrt(nsec);
    const uint32_t bq = (uint32_t)bqd;
    const int grp = (int)grpd;
    gbest = 1.0;
    gsecond = rpp::dinf();
    if (dl < db - qm) {
      ni = li;
      nqx = lx;
      nqy = ly;
      return 1;
    }
    if (ds - db > 2.0 * qm && dl > db + qm && bq < QSAT) {
      const double hx = x[grp + (tid & 3)], hy = y[grp + (tid & 3)];   // the group's nodes (padding is readable)
      if (resolve_group(c, grp, B_n, hx, hy, rppk::quant16(c, s2x, s2y), bq, ni, nqx, nqy)) return 1;
    }
    o_bq = bq;
    return bq < QSAT ? 2 : 0;
  };
  PH_DECL

  for (int step = 0; step < iters && it < c.max_iter && !stop; step++, it++) {
    ST_ADD(S_ITER, 1);
    // ---------------- sample :1132-1153
    if (!have_sample) {
      take_next_sample();
      lds_barrier();
    }
    const double rx = sh.rx, ry = sh.ry;
    have_sample = 0;
    PH(0);
    // ---------------- nearest :1197-1202
    ST_ADD(S_AB2, 16 * (int64_t)n);   // + 24 per obstacle, added per iteration at the end of the launch
    const double r2 = c.r2tab[n + 1];   // find_near_nodes radius for this tree size (requested early, used later)
    const double r2b = SPEC_ON ? c.r2tab[n + 2] : 0.0;   // ... and for the next one (speculated balls: the largest they can need)
    if (!have_nearest) {
      bool done = false;
      if (first_goal >= 0 && rx == gx && ry == gy) {
        // the sample is the goal and nodes lie exactly on it: d == 0 there, min() keeps the lowest index (:1200)
        ni = first_goal;
        nqx = gx;
        nqy = gy;
        gbest = 0.0;
        gsecond = rpp::dinf();
        done = true;
      } else {
        const uint32_t sq = rppk::quant16(c, rx, ry);
        // upper bound (squared grid units) of the nearest node's grid distance: from the fused pass of the previous
        // iteration when it was the one that could not decide (q_amb), else from a nearest pass now
        uint32_t bq = q_amb_bq;
        bool bound = q_amb != 0;
        if (!bound) {
          int grp;
          double fb, fs;
          scan2g<false, true>(gs, (int)(__builtin_sqrt(r2) * qinv) + 1, xq, n, 0u, 0u, sq, hits, sh, grp, fb, fs);
          ST_ADD(S_SN, gs.nodes);
          ST_ADD(S_AB, gs.bytes + 64);
          if (fb < (double)QSAT) {
            // accepted when the winner is exact (not saturated) and the runner-up is more than 2 q_m further
            if ((__builtin_sqrt(fs) - __builtin_sqrt(fb)) > 2.0 * qm_grid) {
              const int gl = grp + (tid & 3);
              const double hx = x[gl], hy = y[gl];   // the group's nodes (padding past n is readable)
              if (resolve_group(c, grp, n, hx, hy, sq, (uint32_t)fb, ni, nqx, nqy)) {
                gbest = 1.0;
                gsecond = rpp::dinf();
                done = true;
              }
            }
            if (!done) {
              bq = (uint32_t)fb;
              bound = true;
            }
          }
        }
        if (!done && bound) {
          // Undecided at 16 bits: the true nearest node lies within 2 q_m of the best grid distance, so a second
          // 16-bit pass collects every node inside that ball (a handful) and the decision is made on their f64
          // coordinates -- 4 bytes per node instead of the 16 of the f64 pass.
          const double rb = __builtin_sqrt((double)bq) + 2.0 * qm_grid;
          const double tb = rb * rb + 1.0;
          if (tb < (double)QSAT) {
            ST_ADD(S_QA, 1);
            int d0;
            double d1, d2;
            const int kc = scan2g<true, false>(gs, 0, xq, n, sq, (uint32_t)tb, 0u, hits, sh, d0, d1, d2);
            ST_ADD(S_SN, gs.nodes);
            ST_ADD(S_AB, gs.bytes + 16 * (int64_t)kc);
            double best = rpp::dinf(), second = rpp::dinf(), bx = 0.0, by = 0.0;
            int bidx = 0x7fffffff;
            for (int h = tid; h < kc; h += TPB) {
              int idx;
              double hx, hy;
              hit_at2q(x, y, hits, sh, h, idx, hx, hy);
              const double d = rpp::fast_d2(hx - rx, hy - ry);
              if (d < best || (d == best && idx < bidx)) {
                second = best;
                best = d;
                bidx = idx;
                bx = hx;
                by = hy;
              } else if (d < second) {
                second = d;
              }
            }
            lds_barrier();
            block_argmin_xy(best, bidx, second, bx, by, sh, gbest, ni, gsecond, nqx, nqy);
            if (gbest != 0.0 && gsecond <= gbest * (1.0 + FILTER_EPS)) {
              // candidates inside the filter margin of the minimum: the exact ** 2 decides, lowest index on ties (:1200)
              ST_ADD(S_EX, 1);
              const double lim = gbest * (1.0 + FILTER_EPS);
              best = rpp::dinf();
              bidx = 0x7fffffff;
              for (int h = tid; h < kc; h += TPB) {
                int idx;
                double hx, hy;
                hit_at2q(x, y, hits, sh, h, idx, hx, hy);
                if (rpp::fast_d2(hx - rx, hy - ry) > lim) continue;
                const double d = rpp::py_d2(hx - rx, hy - ry);
                if (d < best || (d == best && idx < bidx)) {
                  best = d;
                  bidx = idx;
                  bx = hx;
                  by = hy;
                }
              }
              lds_barrier();
              block_argmin_xy(best, bidx, rpp::dinf(), bx, by, sh, d1, ni, d2, nqx, nqy);
            }
            gbest = 1.0;
            gsecond = rpp::dinf();
            done = true;
          }
        }
      }
      if (!done) {
        ST_ADD(S_FB, 1);
        scan2<false, true>(x, y, n, 0.0, 0.0, 0.0, rx, ry, hits, sh, ni, gbest, gsecond, nqx, nqy);
        ST_ADD(S_SN, n);
        ST_ADD(S_AB, 16 * (int64_t)n);
      }
    }
    have_nearest = 0;
    q_amb = 0;
    if (gbest != 0.0 && gsecond <= gbest * (1.0 + FILTER_EPS)) {
      // two candidates inside the filter margin: decide with the exact ** 2 (rare)
      ST_ADD(S_EX, 1);
      int d0;
      double d1, d2, d3, d4;
      const int kraw = scan2<true, false>(x, y, n, rx, ry, gbest * (1.0 + FILTER_EPS), 0.0, 0.0, hits, sh, d0, d1, d2,
                                          d3, d4);
      double best = rpp::dinf(), second = rpp::dinf(), bx = 0.0, by = 0.0;
      int bidx = 0x7fffffff;
      for (int h = tid; h < kraw; h += TPB) {
        int idx;
        double hx, hy;
        hit_at2(x, y, hits, sh, h, idx, hx, hy);
        const double d = rpp::py_d2(hx - rx, hy - ry);
        if (d < best || (d == best && idx < bidx)) {
          best = d;
          bidx = idx;
          bx = hx;
          by = hy;
        }
      }
      lds_barrier();
      block_argmin_xy(best, bidx, second, bx, by, sh, d1, ni, d2, nqx, nqy);
    }
    PH(1);

    // ---------------- steer + collision of the extension :1051-1059
    // Without libm calls in the usual case, like the candidate edges (eval_edges_dual2): once the tree is dense the nearest
    // node is closer than expand_dis, the walk of :1100-1106 ends within one resolution of the sample and :1108-1113 snaps
    // the new node ONTO the sample.  "Snapped" is certain when d - n res <= res (1 - 1e-9), and the points along the
    // straight line decide the collision test unless an obstacle's threshold lies within `tol` of the closest point.
    // Anything in doubt -- a nearest node further than expand_dis (the new node is then the walk's end point: cos / sin
    // needed), the remaining distance at the resolution, an obstacle in the band -- takes the exact form below.
    if (tid == 0) {
      const double dx = rx - nqx, dy = ry - nqy;
      const double d = rpp::py_hypot(dx, dy);
      const int ne = (int)__builtin_floor(d / c.res);
      const bool sure = d <= c.expand_dis && d - (double)ne * c.res <= c.res * (1.0 - 1e-9);
      const double sc = d > 0.0 ? c.res / d : 0.0;
      sh.e0.fx = nqx; sh.e0.fy = nqy; sh.e0.tx = rx; sh.e0.ty = ry;
      sh.e0.sx = sc * dx;
      sh.e0.sy = sc * dy;
      sh.e0.n_expand = ne;
      sh.e0.ex = rx;
      sh.e0.ey = ry;
      sh.e0.snapped = 1;
      sh.ecoll0 = 0;
      sh.fb = sure ? 0 : 1;   // 1: the exact form has to decide
      sh.nx = rx;
      sh.ny = ry;
      sh.flag = rpp::in_play_area(c.has_play, c.play_area, rx, ry) ? 1 : 0;
    }
    lds_barrier();
    if (!sh.fb && sh.flag) {
      for (int k = tid, mk = uni_i(sh.om); k < mk; k += TPB) {
        const double tol = 1e-10 * (1.0 + rpp::dabs(nqx) + rpp::dabs(nqy) + rpp::dabs(sh.ox[k]) + rpp::dabs(sh.oy[k])) *
                           (4.0 + sh.othr[k]);
        const int r = edge_hits_obstacle_band(sh.e0, true, sh.ox[k], sh.oy[k], sh.othr[k], tol);
        if (r == 1) sh.ecoll0 = 1;
        if (r == 2) sh.fb = 2;   // an obstacle in the band
      }
    }
    lds_barrier();
    const bool ext_exact = sh.fb != 0;
    if (!ext_exact && sh.flag) {
      ST_ADD(S_EU, 1);
      ST_ADD(S_ER, 1);
    }
    lds_barrier();
    if (ext_exact) {
      const int w = tid >> 6, lane = tid & 63;
      // waves 0 and 1, lane 0: same distance/angle, cos on one SIMD and sin on another (one-wave shape: lane 0 both)
      if (lane == 0 && w < 2) {
        const double dx = rx - nqx, dy = ry - nqy;
        const double d = rpp::py_hypot(dx, dy);
        const double theta = rpp_glibc_atan2(dy, dx);
        if (NW == 1) sh.e0.sy = c.res * rpp_glibc_sin(theta);
        if (w == 0) {
          double ext = c.expand_dis;
          if (ext > d) ext = d;
          sh.e0.n_expand = (int)__builtin_floor(ext / c.res);
          sh.e0.sx = c.res * rpp_glibc_cos(theta);
          sh.e0.fx = nqx; sh.e0.fy = nqy; sh.e0.tx = rx; sh.e0.ty = ry;
        } else {
          sh.e0.sy = c.res * rpp_glibc_sin(theta);
        }
      }
      lds_barrier();
      if (tid == 0) {
        double px = nqx, py = nqy;
        const double sx = sh.e0.sx, sy = sh.e0.sy;
        for (int i = 0; i < sh.e0.n_expand; i++) {
          px += sx;
          py += sy;
        }
        const int snapped = rpp::py_hypot(rx - px, ry - py) <= c.res;
        sh.e0.ex = snapped ? rx : px;
        sh.e0.ey = snapped ? ry : py;
        sh.e0.snapped = snapped;
        sh.ecoll0 = 0;
        sh.nx = sh.e0.ex;
        sh.ny = sh.e0.ey;
        sh.flag = rpp::in_play_area(c.has_play, c.play_area, sh.e0.ex, sh.e0.ey) ? 1 : 0;
      }
      lds_barrier();
    }
    PH(2);
    const double nx = sh.nx, ny = sh.ny;
    const int inplay = sh.flag;
    if (inplay && ext_exact) {
      ST_ADD(S_EU, 1);
      ST_ADD(S_ER, 1);
      for (int k = tid, mk = uni_i(sh.om); k < mk; k += TPB)
        if (rpp::edge_hits_obstacle(sh.e0, sh.ox[k], sh.oy[k], sh.othr[k])) sh.ecoll0 = 1;
    }
    lds_barrier();
    const int accepted = inplay && !sh.ecoll0;
    int nnear = -1;
    PH(3);

    if (accepted) {
      // ---------------- find_near_nodes :1314-1338 (+ nearest query of the next iteration, same pass)
      // the ball speculated by the previous iteration's pass is this iteration's near query (n == spec_n + 1)
      bool use_spec = false;
      int spec_k0 = 0, spec_off0 = 0;
      if (SPEC_ON && ns > 0) {
        const double* R = G + 16 + 8 * shead;
        const double cx0 = R[0], cy0 = R[1], k0 = R[4], o0 = R[5];
        use_spec = uni_i(k0 >= 0.0 && nx == cx0 && ny == cy0) != 0;
        spec_k0 = uni_i((int)k0);
        spec_off0 = uni_i((int)o0);
      }
      bool did_spec = false;
      const int do_pf = !use_spec && (step + 1 < iters) && (it + 1 < c.max_iter);
      int kraw;
      int pf_ni = 0;
      double pf_best = 0.0, pf_second = 0.0, pf_x = 0.0, pf_y = 0.0;
      int zskip = 0;                     // goal duplicates inside the 16-bit ball that the pass counted instead of recording
      const int zgate = (first_goal >= 0 && goal_dups > 0) ? first_goal : -1;
      uint32_t pf_sq = 0u, pf_bq = 0u;   // 16-bit stage: packed query, best squared grid distance,
      int pf_grp = -1, pf_n = 0;         // the winner's 4-node group (unresolved while >= 0) and the tree size scanned
      bool pf_goal = false;
      int64_t pass_b = 0, pass_n = n;    // 16-bit stage: bytes and nodes its passes read
      if (use_spec) {
        // the nodes appended since that pass join the ball by the pass's own grid test, in index order
        int k2 = spec_k0;
        const int off0 = spec_off0;
        const uint32_t cq = rppk::quant16(c, nx, ny);
        double axv[KA], ayv[KA];
#pragma unroll
        for (int j = 0; j < KA; j++) {
          axv[j] = G[8 + j];
          ayv[j] = G[12 + j];
        }
#pragma unroll
        for (int j = 0; j < KA; j++) {
          if (uni_i(j < na && qdist(rppk::quant16(c, axv[j], ayv[j]), cq) <= B_thr)) {
            if (tid == 0) hits[off0 + k2] = B_n + j;
            k2++;
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int32_t* lhit = reinterpret_cast<int32_t*>(sh.u.hit);
        for (int h = tid; h < k2 && h < HWF; h += TPB) lhit[h] = hits[off0 + h];
        if (tid == 0) {
          sh.wave_cnt[0] = k2;
          sh.wave_start[0] = off0;
        }
        lds_barrier();
        kraw = k2;
        ST_ADD(S_RIDE, 1);
        ST_ADD(S_AB, 16 * (int64_t)kraw + 16);
      } else {
        ns = 0;
        na = 0;
        // ball radius r + m in the mirror's metric, rounded up
        const double rr = __builtin_sqrt(r2) + qm;
        const double thr_gd = rr * rr * qinv * qinv * (1.0 + 1e-6) + 1.0;    // the same in (integer) grid units
        const uint32_t thr_gi = thr_gd < 4.0e9 ? (uint32_t)thr_gd : 4000000000u;
        const int rw_gi = (int)__builtin_sqrt((double)thr_gi) + 1;   // its window half-width (grid index)
        if (do_pf) {
          take_next_sample();
          lds_barrier();
          have_sample = 1;
          pf_goal = first_goal >= 0 && sh.rx == gx && sh.ry == gy;
        }
        if (do_pf && !pf_goal) {
          pf_sq = rppk::quant16(c, sh.rx, sh.ry);
          // further query sets: the following iterations' balls about their samples, up to the first that reaches the
          // goal's grid cell (or the end of this launch)
          int kmax = 0;
          if (SPEC_ON && n >= 256) {
            kmax = iters - step - 2 < c.max_iter - it - 2 ? iters - step - 2 : c.max_iter - it - 2;
            kmax = kmax < 0 ? 0 : (kmax > KS_RUN ? KS_RUN : kmax);
          }
          kmax = uni_i(kmax);
          if constexpr (NW == 1 && KSM > 0) {
            uint32_t thr2 = 0u;
            if (kmax > 0) {
              const double rr2 = __builtin_sqrt(r2b) + qm;
              const double tg2 = rr2 * rr2 * qinv * qinv * (1.0 + 1e-6) + 1.0;
              thr2 = tg2 < 4.0e9 ? (uint32_t)tg2 : 4000000000u;
              if (uni_i(qdist(goal_q, pf_sq) <= thr2)) kmax = 0;
            }
            if (kmax > 0) {
              // samples i + 2 .. i + 1 + kmax, next in the stream, behind those already queued: lane 0 draws them
              // through sh.rx / sh.ry and puts them in the ring
              const double p1x = sh.rx, p1y = sh.ry;
              if (nq < kmax) {
                lds_barrier();
                if (tid == 0) {
                  for (int j = nq; j < kmax; j++) {
                    rppk::draw_sample(c, sh, sob, gx, gy);
                    G[(qhead + j) & 3] = sh.rx;
                    G[4 + ((qhead + j) & 3)] = sh.ry;
                  }
                  sh.rx = p1x;
                  sh.ry = p1y;
                }
                nq = kmax;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lds_barrier();
              }
              double qxv[KA], qyv[KA];
#pragma unroll
              for (int j = 0; j < KA; j++) {
                qxv[j] = G[(qhead + j) & 3];
                qyv[j] = G[4 + ((qhead + j) & 3)];
              }
              // ball j is about sample i + 1 + j: p1 for j = 0, the queue's entry j - 1 after that
              int ks = kmax;
#pragma unroll
              for (int j = 1; j < KA; j++)
                if (uni_i(j < ks && qdist(goal_q, rppk::quant16(c, qxv[j - 1], qyv[j - 1])) <= thr2)) ks = j;
              SpecQ sp[KA];
#pragma unroll
              for (int j = 0; j < KA; j++) {
                const bool on = j < ks;
                const double cxj = j == 0 ? p1x : qxv[j > 0 ? j - 1 : 0], cyj = j == 0 ? p1y : qyv[j > 0 ? j - 1 : 0];
                sp[j].qq = on ? rppk::quant16(c, cxj, cyj) : pf_sq;
                sp[j].thr = on ? thr2 : 0u;    // unused set: radius 0 about a centre whose hits nobody reads
                sp[j].sq = rppk::quant16(c, on ? qxv[j] : p1x, on ? qyv[j] : p1y);
                sp[j].off = spec_base + j * SPEC_CAPS;
                sp[j].cap = SPEC_CAPS;
                if (tid == 0) {   // the record's centre now: nothing of the queue has to stay in registers over the pass
                  double* R = G + 16 + 8 * j;
                  R[0] = cxj;
                  R[1] = cyj;
                  R[5] = (double)sp[j].off;
                }
              }
              kraw = scan2g<true, true, KSM>(gs, rw_gi, xq, n, rppk::quant16(c, nx, ny), thr_gi, pf_sq, hits, sh, pf_ni,
                                             pf_best, pf_second, goal_q, zgate, &zskip, sp);
              pass_b = gs.bytes;
              pass_n = gs.nodes;
              did_spec = true;
              B_n = n;
              B_thr = uni_u(thr2);
              ns = ks;
              shead = 0;
              na = 0;
              if (tid == 0) {
                const double qs2 = c.q_step * c.q_step;
#pragma unroll
                for (int j = 0; j < KA; j++) {
                  const bool on = j < ks;
                  double* R = G + 16 + 8 * j;
                  R[2] = sp[j].best * qs2;
                  R[3] = sp[j].second * qs2;
                  R[4] = (on && sp[j].cnt + j + 1 <= SPEC_CAPS) ? (double)sp[j].cnt : -1.0;   // room for the nodes appended before it is used
                  R[6] = on ? (double)sp[j].grp : -1.0;
                  R[7] = sp[j].best;
                }
              }
            }
          }
          if (!did_spec) {
            kraw = scan2g<true, true>(gs, rw_gi, xq, n, rppk::quant16(c, nx, ny), thr_gi, pf_sq, hits, sh, pf_ni, pf_best,
                                      pf_second, goal_q, zgate, &zskip);
            pass_b = gs.bytes;
            pass_n = gs.nodes;
          }
          if (zskip > goal_dups) {   // a different node shares the goal's grid cell: record everything
            kraw = scan2g<true, true>(gs, rw_gi, xq, n, rppk::quant16(c, nx, ny), thr_gi, pf_sq, hits, sh, pf_ni, pf_best,
                                      pf_second);
            zskip = 0;
            ST_ADD(S_AB, gs.bytes);
          }
          pf_bq = (uint32_t)pf_best;
          pf_grp = pf_ni;
          pf_n = n;
          // f64 coordinates of the provisional nearest node's 4-node group (lanes 0..3): requested now, resolved
          // after the candidate phases
          pf_x = x[pf_grp + (tid & 3)];
          pf_y = y[pf_grp + (tid & 3)];
          pf_best *= c.q_step * c.q_step;   // squared grid units -> squared world units (fold logic below)
          pf_second *= c.q_step * c.q_step;
        } else {
          int d0;
          double d1, d2;
          kraw = scan2g<true, false>(gs, rw_gi, xq, n, rppk::quant16(c, nx, ny), thr_gi, 0u, hits, sh, d0, d1, d2, goal_q,
                                     zgate, &zskip);
          pass_b = gs.bytes;
          pass_n = gs.nodes;
          if (zskip > goal_dups) {
            kraw = scan2g<true, false>(gs, rw_gi, xq, n, rppk::quant16(c, nx, ny), thr_gi, 0u, hits, sh, d0, d1, d2);
            zskip = 0;
            ST_ADD(S_AB, gs.bytes);
          }
        }
        ST_ADD(S_AB, pass_b + 16 * (int64_t)kraw + 16);
      }
      ST_ADD(S_SN, pass_n);
      ST_ADD(S_AB2, 16 * (int64_t)n);
      // Fold of the node this iteration appends (position ax, ay, index aidx) into the pass's provisional nearest node
      // of the next sample: margin test in the distance metric, the appended node's distance is exact.  Returns 1 with
      // the nearest node in (o_ni, o_x, o_y), or 0 when the 16-bit stage could not decide (the next iteration's nearest
      // step takes the query on).
      auto fold_new_node = [&](double ax, double ay, int aidx, int& o_ni, double& o_x, double& o_y) -> int {
        if (pf_goal) {
          o_ni = first_goal;
          o_x = gx;
          o_y = gy;
          return 1;
        }
        const double dxl = ax - sh.rx, dyl = ay - sh.ry;
        const double dl = __builtin_sqrt(dxl * dxl + dyl * dyl);
        const double db = __builtin_sqrt(pf_best), ds = __builtin_sqrt(pf_second);
        if (dl < db - qm) {
          o_ni = aidx;
          o_x = ax;
          o_y = ay;
          return 1;
        }
        // the winner is exact only below the saturation bound; find it inside its group
        if (ds - db > 2.0 * qm && dl > db + qm && pf_bq < QSAT)
          return resolve_group(c, pf_grp, pf_n, pf_x, pf_y, pf_sq, pf_bq, o_ni, o_x, o_y) ? 1 : 0;
        return 0;
      };
      PH(4);
      int pend_p, pend_fc;
      double pend_cost;
      build_candidates(x, y, cost, first_child, nx, ny, r2, hits, kraw, sh, pend_p, pend_cost, pend_fc);
      PH(5);
      const int nu = sh.nu;
      int nvalid = sh.nvalid;
      // the goal duplicates the pass did not record carry first_goal's value: in near_inds iff it is (:1335-1337)
      double vgoal = -1.0;   // first_goal's exact value when duplicates were skipped
      if (zskip > 0) {
        vgoal = rpp::py_d2(gx - nx, gy - ny);
        if (vgoal <= r2) nvalid += zskip;
      }
      nnear = nu;
      ST_ADD(S_NH, nvalid);
      ST_ADD(S_NU, nu);
      if (tid == 0 && nu > sh.stat[S_NUMAX]) sh.stat[S_NUMAX] = nu;
      ST_ADD(S_AB, 48 * (int64_t)nu + 28);
      ST_ADD(S_AB2, 48 * (int64_t)nu + 28);
      // ---------------- choose_parent :1242-1282 (+ speculative backward edges)
      int have = 0, sel = -1;
      double min_cost = rpp::dinf();
      // obstacles that reach the near ball (one-wave shape): the only ones this iteration's candidate edges can meet
      bool cull = false;
      uint64_t omask = 0;
      if constexpr (NW == 1) {
        if (nu > 0 && c.obs_cull && om <= 64) {
          cull = true;
          omask = obstacle_mask(om, nx, ny, r2, sh);
          CULL_COUNT(omask);
        }
      }
      if (nu > 0) {
        ST_ADD(S_EU, nu);
        ST_ADD(S_ER, nvalid);
        eval_edges_dual2(c, om, nu, nx, ny, sh, cull, omask);
        if (pend_p >= 0) {
          sh.ucur[pend_p] = pend_cost;
          sh.ufc[pend_p] = pend_fc;
        }
        lds_barrier();
        PH(6);
        double best = rpp::dinf(), second = rpp::dinf(), gs, t0, t1;
        int bidx = 0x7fffffff;
        for (int e = tid; e < nu; e += TPB) {
          const double d = (sh.uflag[e] & 1) ? sh.ucur[e] + sh.uhyp[e] : rpp::dinf();   // near.cost + hypot :1269
          if (d < best) {
            best = d;
            bidx = e;
          }
        }
        block_argmin_xy(best, bidx, second, 0.0, 0.0, sh, min_cost, sel, gs, t0, t1);   // first minimum :1272-1278
        have = min_cost < rpp::dinf();
        PH(7);
      }
      double wx = nx, wy = ny, wcost;
      int wparent;
      if (have) {
        wx = sh.uex[sel];
        wy = sh.uey[sel];
        wcost = min_cost;
        wparent = sh.uidx[sel];
        const int newidx = n;
        lds_barrier();
        // ---------------- rewire (before append) :1340-1373
        ST_ADD(S_EU, nu);
        ST_ADD(S_ER, nvalid);
        if (wx != nx || wy != ny) eval_edges_back2(c, om, nu, wx, wy, sh, cull, omask);
        for (int e = tid; e < nu; e += TPB) sh.uval[e] = wcost + sh.uhyp[e];   // edge_node.cost :1362
        if (tid == 0) {
          sh.n_rw = 0;
          sh.n_pr = 0;
          sh.moved = 0;
          sh.last_fc = -1;
        }
        lds_barrier();
        PH(8);
        // candidate indices in registers of wave 0 (the cost walk refreshes candidates it passes)
        int my_uidx[CE];
#pragma unroll
        for (int k = 0; k < CE; k++) my_uidx[k] = ((tid & 63) + 64 * k < nu) ? sh.uidx[(tid & 63) + 64 * k] : -1;
        for (int e0 = 0; e0 < nu;) {
          int cand = 0x7fffffff;
          for (int e = e0 + tid; e < nu; e += TPB) {
            if ((sh.uflag[e] & 2) && sh.ucur[e] > sh.uval[e]) {   // no_collision and improved_cost :1366-1368
              cand = e;
              break;
            }
          }
          const int es = block_min_int(cand, sh);
          if (es == 0x7fffffff) break;
          if (tid < 64) {
            // wave 0, every lane in step: scalar loads, lane 0 stores
            const int u = __builtin_amdgcn_readfirstlane(sh.uidx[es]);
            // stores of an earlier rewire of this iteration (sibling links, child lists) have reached L2
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int par, pv, nxs;
            sload3(parent + u, prev_sib + u, next_sib + u, par, pv, nxs);
            if (tid == 0) {
              // the identity re-pointing of :1369-1372 with integer links: leave the old parent's child list ...
              if (pv >= 0) {
                next_sib[pv] = nxs;
              } else {
                first_child[par] = nxs;
              }
              if (nxs >= 0) prev_sib[nxs] = pv;
            }
            if (pv < 0) {
#pragma unroll
              for (int k = 0; k < CE; k++)
                if (my_uidx[k] == par) sh.ufc[(tid & 63) + 64 * k] = nxs;
            }
            int moved_now = 0;
            if (!(sh.uflag[es] & 4)) {
              // steer(new -> node) stopped short of the node: node_list[i] = edge_node moves it (rare; lane 0, vector path)
              moved_now = 1;
              const uint32_t q_old = gs.ok ? rppk::quant16(c, sh.ux[es], sh.uy[es]) : 0u;   // where the index has it
              if (tid == 0) {
                rpp::steer(&sh.e0, wx, wy, sh.ux[es], sh.uy[es], rpp::dinf(), c.res);
                x[u] = sh.e0.ex;
                y[u] = sh.e0.ey;
                xq[u] = rppk::quant16(c, sh.e0.ex, sh.e0.ey);
                // near_inds may hold an index AGAIN (nodes at equal distance collapse onto the first, :1337).  Once a
                // node has moved, later visits are no longer void: the moved node is re-steered to where it lies now, and
                // descendants whose cost rose may qualify on a repeated visit.  That raw-list walk lives in the general
                // kernel (rppk::rewire_raw_walk): an iteration that moves a node while its raw list has repeats ends this
                // kernel's work on the instance (RRTX_ST_UNSUPPORTED in the status word) and rrtx_plan plans the instance
                // again on the general kernel, from its staged start state.  Rare: needs an inexact path_resolution and
                // a distance tie in the same near set.
                if (nvalid > nu) sh.overflow = 2;
                const bool was_on_goal = sh.ux[es] == gx && sh.uy[es] == gy;
                sh.ux[es] = sh.e0.ex;
                sh.uy[es] = sh.e0.ey;
                sh.moved = (u == first_goal || was_on_goal || (sh.e0.ex == gx && sh.e0.ey == gy))
                               ? 3 : (sh.moved | 1);   // 3: the bookkeeping of nodes lying on the goal is void
                // its own edge and its children's edges changed length
                elen[u] = rpp::py_hypot(sh.e0.ex - wx, sh.e0.ey - wy);
                for (int ch = sh.ufc[es]; ch >= 0; ch = next_sib[ch])
                  elen[ch] = rpp::py_hypot(x[ch] - sh.e0.ex, y[ch] - sh.e0.ey);
              }
              if (NW == 1 && gs.ok) {   // the moved node changes cell (the index keeps it at the new xq[] value)
                lds_barrier();
                grid_remove(gs, u, q_old);
                if (gs.ok) grid_insert(gs, u, rppk::quant16(c, sh.ux[es], sh.uy[es]));
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              }
            }
            const double ec = sh.uval[es];
            const int root_fc = __builtin_amdgcn_readfirstlane(sh.ufc[es]);
            if (tid == 0) {
              if (!moved_now) elen[u] = sh.uhyp[es];
              cost[u] = ec;
              sh.ucur[es] = ec;
              // ... and become a child of the node about to be appended
              parent[u] = newidx;
              prev_sib[u] = -1;
              next_sib[u] = sh.last_fc;
              if (sh.last_fc >= 0) prev_sib[sh.last_fc] = u;
              sh.last_fc = u;
              sh.n_rw++;
            }
            if (moved_now) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the children's new elen
            PH(13);
            bool reread = false;
            int np = propagate_scalar(cost, first_child, next_sib, elen, root_fc, ec, sh, my_uidx,   // :1373
                                      NW == 1 ? c.prop_vec : -1, NW == 1 ? c.prop_cap : (1 << 30), reread,
                                      (unsigned long long*)&I->phase[PROP_WALK_SLOT]);
            if (np < 0) {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              if (tid == 0) sh.fcount = rppk::propagate(x, y, cost, first_child, next_sib, stack, u);
              np = sh.fcount;
              reread = true;
            }
            if (reread) {
              // later candidates may be descendants of the node just rewired: refresh their costs
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              for (int e = es + 1 + tid; e < nu; e += 64)
                if (sh.uflag[e] & 2) sh.ucur[e] = cost[sh.uidx[e]];
            }
            if (tid == 0) sh.n_pr += np;
            PH(14);
          }
          lds_barrier();
          e0 = es + 1;
        }
        if (tid == 0) {
          // append :1065
          x[newidx] = wx;
          y[newidx] = wy;
          xq[newidx] = rppk::quant16(c, wx, wy);
          cost[newidx] = wcost;
          elen[newidx] = sh.uhyp[sel];   // == hypot(new - parent) from the position the node ends up at
          first_child[newidx] = sh.last_fc;
          // link under the chosen parent; its current first child is in the LDS record (kept current above)
          const int f = sh.ufc[sel];
          parent[newidx] = wparent;
          prev_sib[newidx] = -1;
          next_sib[newidx] = f;
          if (f >= 0) prev_sib[f] = newidx;
          first_child[wparent] = newidx;
        }
        // the index: an exact goal duplicate (first_goal >= 0 already) stays out of it, counted instead
        if (gs.ok) {
          if (first_goal >= 0 && wx == gx && wy == gy)
            gs.excl++;
          else
            grid_insert(gs, newidx, rppk::quant16(c, wx, wy));
        }
        lds_barrier();
        PH(9);
        ST_ADD(S_RW, sh.n_rw);
        ST_ADD(S_PR, sh.n_pr);
        n++;
      } else {
        // choose_parent returned None: append the extension as it is (:1066-1067)
        if (tid == 0) {
          x[n] = nx;
          y[n] = ny;
          xq[n] = rppk::quant16(c, nx, ny);
          const double el = rpp::py_hypot(nx - nqx, ny - nqy);
          elen[n] = el;
          cost[n] = cost[ni] + el;   // :1054-1056
          first_child[n] = -1;
          rppk::link_child(parent, first_child, next_sib, prev_sib, n, ni);
          sh.moved = 0;
        }
        if (gs.ok) {
          if (first_goal >= 0 && nx == gx && ny == gy)
            gs.excl++;
          else
            grid_insert(gs, n, rppk::quant16(c, nx, ny));
        }
        n++;
        lds_barrier();
      }
      const int moved = uni_i(sh.moved);
      if (moved & 2) first_goal = -2;   // a node on the goal moved (or one moved onto it): lowest index unknown
      if ((moved & 2) && gs.excl > 0) gs.ok = 0;   // ... and the goal duplicates the index left out count as nodes again
      if (wx == gx && wy == gy) {
        if (first_goal == -1) {
          first_goal = n - 1;
          goal_dups = 0;
        } else if (first_goal >= 0) {
          goal_dups++;
        }
      }
      if (do_pf && !moved) {
        have_nearest = fold_new_node(wx, wy, n - 1, pf_ni, pf_x, pf_y);
        if (!have_nearest && pf_bq < QSAT) {   // the best OLD node bounds the nearest distance (the new node can only be nearer)
          q_amb = 1;
          q_amb_bq = pf_bq;
        }
        pf_best = pf_goal ? 0.0 : 1.0;
        pf_second = rpp::dinf();
      }
      if (tid == 0 && inst == c.trace_inst) {
        c.tr_rx[it] = rx;
        c.tr_ry[it] = ry;
        c.tr_near[it] = ni;
        c.tr_nn[it] = nnear;
        c.tr_kind[it] = have ? 2 : 1;
      }
      ni = pf_ni;
      gbest = pf_best;
      gsecond = pf_second;
      nqx = pf_x;
      nqy = pf_y;
      if (SPEC_ON) {
        if (moved) {
          ns = 0;
          na = 0;
        } else if ((use_spec || did_spec) && na < 4) {
          // the node just appended joins the list of nodes the pass has not seen
          if (tid == 0) {
            G[8 + na] = wx;
            G[12 + na] = wy;
          }
          na++;
        }
        if (use_spec && ns > 0) {
          // this iteration rode on an earlier pass: the next sample's nearest node from that pass + the new nodes
          uint32_t fbq;
          const int fr = uni_i(fold_n2(fbq));
          have_nearest = fr == 1;
          if (fr == 2) {   // the best OLD node bounds the nearest distance: candidate pass at the next nearest step
            q_amb = 1;
            q_amb_bq = uni_u(fbq);
          }
          shead = (shead + 1) & 3;
          ns--;
        }
      }
    } else {
      if (tid == 0 && inst == c.trace_inst) {
        c.tr_rx[it] = rx;
        c.tr_ry[it] = ry;
        c.tr_near[it] = ni;
        c.tr_nn[it] = nnear;
        c.tr_kind[it] = 0;
      }
      // rejected extension: this iteration's speculated ball is void, the later sets are not (one node fewer to fold)
      if (SPEC_ON && ns > 0) {
        uint32_t fbq;
        const int fr = uni_i(fold_n2(fbq));
        have_nearest = fr == 1;
        if (fr == 2) {
          q_amb = 1;
          q_amb_bq = uni_u(fbq);
        }
        shead = (shead + 1) & 3;
        ns--;
      }
    }
    PH(11);
    if (sh.overflow) stop = 1;
  }

  // write back state; the final goal search (rrt_04:1080-1084) is done by the v1 kernel
  lds_barrier();
  for (int i = tid; i < 624; i += TPB) I->rng.mt[i] = sh.rng.mt[i];
  if (tid == 0) {
    I->rng.pos = sh.rng.pos;
    I->sobol = sob;
    I->first_goal = first_goal;
    I->goal_dups = goal_dups;
    I->n = n;
    I->it = it;
    if (sh.overflow == 1) I->status |= 4 | 1;
    if (sh.overflow == 2) I->status |= 16 | 1;
    I->iterations += sh.stat[S_ITER];
    I->edges_unique += sh.stat[S_EU];
    I->edges_ref += sh.stat[S_ER];
    I->near_hits += sh.stat[S_NH];
    I->near_unique += sh.stat[S_NU];
    I->rewires += sh.stat[S_RW];
    I->propagated += sh.stat[S_PR];
    I->scan_nodes += sh.stat[S_SN];
    const int64_t tile_b = 24 * (int64_t)I->obs_m * sh.stat[S_ITER];   // the obstacle tile, read every iteration
    I->alg_bytes += sh.stat[S_AB] + tile_b;
    I->alg_bytes2 += sh.stat[S_AB2] + tile_b;
    I->exact_rescans += sh.stat[S_EX];
    I->f32_fallbacks += sh.stat[S_FB];
    I->q16_fallbacks += sh.stat[S_QA];
    I->rides += sh.stat[S_RIDE];
    if (sh.stat[S_NUMAX] > I->nu_max) I->nu_max = sh.stat[S_NUMAX];
    PH_STORE(I);
    c.results[inst].n_nodes = n;
    c.results[inst].status = I->status;
  }
}

#undef ST_ADD
#undef CULL_COUNT
}  // namespace RRT2_NS

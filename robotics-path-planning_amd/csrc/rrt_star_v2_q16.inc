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

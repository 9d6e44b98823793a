// rrt_samples.hip.h -- the sample stream of the RRT* iteration kernel (rrt_star_v2_body.inc), drawn ahead of the plan.
//
// get_random_node / get_random_node_sobol (rrt_04:1132-1153) consume the instance's generators in stream order, exactly
// one sample per iteration, whatever the tree does.  rrt_sample_stream_kernel therefore draws all max_iter samples of
// every instance before the first iteration launch, one wave per instance, into Ctx::samp ([instance][iteration] ->
// (x, y), 16 bytes), and leaves the generators in Inst::rng / Inst::sobol as they stand after those draws.  The
// iteration kernel reads samp[it] and holds neither generator.
//
// Every value is bit for bit what rppk::draw_sample returns for that draw: the same rpp::mt_randint_0_100, rpp::mt_uniform
// and rpp::sobol_next run here, on a window of tempered words (MTWin) instead of the state itself.  Per 624 words:
//   * all lanes regenerate the state (mt_twist_lane: three dependent thirds, out of place) and temper it;
//   * lane 0 walks the words that decide where samples start (randint(0, 100) with its rejection loop, the Sobol step):
//     sample_walk, one list entry per sample;
//   * all lanes turn list entries into coordinates (sample_emit: the four words of the two uniform() calls).
// The functions of a lane index compile for the host as well (tests/native/sample_stream_check.cpp).
#pragma once
#include "rpp_core.h"

namespace rppss {

constexpr int MTN = 624;
constexpr int LCAP = 256;   // list entries (samples) per round of the walk
constexpr int32_t KIND_GOAL = -1, KIND_SOBOL = -2;   // list entry >= 0: window position of the first uniform() word

// One third of mt_twist for lane `lane` of `nl`, from the state `o` into the state `w` (o != w).  Third 0: words 0 .. 226
// (old words only); third 1: words 227 .. 453 (new words 0 .. 226); third 2: words 454 .. 623 (new words 227 .. 396 and,
// for word 623, new word 0).  The caller orders the thirds (a barrier between them on the device).
RPP_HD static inline void mt_twist_lane(const uint32_t* o, uint32_t* w, int third, int lane, int nl) {
  const int lo = third == 0 ? 0 : third == 1 ? 227 : 454, hi = third == 0 ? 227 : third == 1 ? 454 : 624;
  for (int kk = lo + lane; kk < hi; kk += nl) {
    const uint32_t nxt = kk == 623 ? w[0] : o[kk + 1];
    const uint32_t y = (o[kk] & 0x80000000U) | (nxt & 0x7fffffffU);
    const uint32_t far = kk < 227 ? o[kk + 397] : w[kk - 227];
    w[kk] = far ^ (y >> 1) ^ ((y & 1U) ? 0x9908b0dfU : 0U);
  }
}

// A window of tempered words of the stream, read in order by rpp::mt_randint_0_100 / rpp::mt_uniform (found through
// this overload of mt_next).  `end` bounds the window: a draw that ran past it would read zeros, which takes a run of
// more than 600 rejected randint words (probability 0.21 ** 600) -- the serial form has no such bound.
struct MTWin {
  const uint32_t* w;
  int32_t pos, end;
};
RPP_HD static inline uint32_t mt_next(MTWin* s) {
  const int32_t p = s->pos++;
  return p < s->end ? s->w[p] : 0u;
}

// draw_sample up to its uniform() calls: the kind of the next sample (KIND_GOAL, KIND_SOBOL with the point in q, or the
// window position of the first of the four uniform words, which the window then skips).
RPP_HD static inline int32_t sample_walk(MTWin* w, int goal_sample_rate, int sampler, rpp::Sobol* sob, double q[2]) {
  if (rpp::mt_randint_0_100(w) > goal_sample_rate) {
    if (sampler == 1) {
      rpp::sobol_next(sob, q);
      return KIND_SOBOL;
    }
    const int32_t p = w->pos;
    w->pos += 4;
    return p;
  }
  return KIND_GOAL;
}

// ... and the rest of it: the sample of a list entry (draw_sample's own expressions)
RPP_HD static inline void sample_emit(const uint32_t* tw, int32_t tw_end, int32_t kind, const double* q, double rand_min,
                                      double rand_max, double gx, double gy, double* rx, double* ry) {
  if (kind == KIND_GOAL) {
    *rx = gx;
    *ry = gy;
  } else if (kind == KIND_SOBOL) {
    *rx = rand_min + q[0] * (rand_max - rand_min);
    *ry = rand_min + q[1] * (rand_max - rand_min);
  } else {
    MTWin u = {tw, kind, tw_end};
    *rx = rpp::mt_uniform(&u, rand_min, rand_max);
    *ry = rpp::mt_uniform(&u, rand_min, rand_max);
  }
}

#if defined(__HIPCC__)
struct ShS {
  uint32_t raw[2][MTN];   // the state the window's first half comes from, and the one after it
  uint32_t tw[2 * MTN];   // tempered words of both
  double lq[LCAP][2];     // list: Sobol points
  int32_t lkind[LCAP];    // list: kinds
  int32_t nl, pos;
};

// One wave per instance (c.inst_map selects them; nullptr = identity): samp[inst][0 .. max_iter) and the generators' end state
__global__ __launch_bounds__(64) void rrt_sample_stream_kernel(rppk::Ctx c) {
  __shared__ ShS sh;
  const int inst = c.inst_map ? c.inst_map[blockIdx.x] : blockIdx.x;
  const int lane = threadIdx.x;
  rppk::Inst* I = c.inst + inst;
  double* __restrict__ out = c.samp + (int64_t)inst * c.max_iter * 2;
  const double gx = I->goal[0], gy = I->goal[1];
  for (int i = lane; i < MTN; i += 64) {
    const uint32_t v = I->rng.mt[i];
    sh.raw[0][i] = v;
    sh.tw[i] = rpp::mt_temper(v);
  }
  rpp::Sobol sob = I->sobol;   // lane 0's copy is the one that steps
  int pos = __builtin_amdgcn_readfirstlane(I->rng.pos);
  __syncthreads();
  // the state after raw[0] into raw[1], tempered into the window's second half
  auto regenerate = [&]() {
    for (int third = 0; third < 3; third++) {
      mt_twist_lane(sh.raw[0], sh.raw[1], third, lane, 64);
      __syncthreads();
    }
    for (int i = lane; i < MTN; i += 64) sh.tw[MTN + i] = rpp::mt_temper(sh.raw[1][i]);
    __syncthreads();
  };
  regenerate();
  int cnt = 0;
  while (cnt < c.max_iter) {
    if (lane == 0) {
      MTWin w = {sh.tw, pos, 2 * MTN};
      int nl = 0;
      while (w.pos < MTN && nl < LCAP && cnt + nl < c.max_iter) {
        sh.lkind[nl] = sample_walk(&w, c.goal_sample_rate, c.sampler, &sob, sh.lq[nl]);
        nl++;
      }
      sh.nl = nl;
      sh.pos = w.pos;
    }
    __syncthreads();
    const int nl = __builtin_amdgcn_readfirstlane(sh.nl);
    pos = __builtin_amdgcn_readfirstlane(sh.pos);
    for (int j = lane; j < nl; j += 64) {
      double rx, ry;
      sample_emit(sh.tw, 2 * MTN, sh.lkind[j], sh.lq[j], c.rand_min, c.rand_max, gx, gy, &rx, &ry);
      reinterpret_cast<rppk::v2d*>(out)[cnt + j] = rppk::v2d{rx, ry};
    }
    cnt += nl;
    __syncthreads();   // the list and the window are free again
    if (cnt < c.max_iter && pos >= MTN) {
      for (int i = lane; i < MTN; i += 64) {
        sh.raw[0][i] = sh.raw[1][i];
        sh.tw[i] = sh.tw[MTN + i];
      }
      __syncthreads();
      regenerate();
      pos -= MTN;
    }
  }
  // mt_next regenerates lazily: a stream that ends on the last word of a state leaves that state with pos == 624
  const int half = pos <= MTN ? 0 : 1;
  for (int i = lane; i < MTN; i += 64) I->rng.mt[i] = sh.raw[half][i];
  if (lane == 0) {
    I->rng.pos = pos - half * MTN;
    I->sobol = sob;
  }
}
#endif

}  // namespace rppss

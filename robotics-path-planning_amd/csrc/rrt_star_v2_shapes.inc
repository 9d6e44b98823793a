using rppk::Ctx;
using rppk::Inst;
using rppk::Kid;
using rppk::Node;
using rppk::GHead;
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
  double nx, ny;
  int32_t flag, nu, nvalid, overflow, ecoll0;
  int32_t fa, fb, fover, fcount;
  int32_t n_rw, n_pr, moved, last_fc;
  int32_t om;           // this instance's obstacle count, for the loops of the iteration body (uni_i on read)
  long long stat[15];   // per-launch counters, lane 0 only (kept out of the register file)
  // one-wave shape, several iterations per pass (rrt_star_v2_kernel.inc): the nodes appended since the pass and the
  // ring of four set records; lane 0 writes, every lane reads
  double ax[4], ay[4];
  double set[4][8];
  int32_t b_n;      // tree size the pass scanned: the nodes appended since have the indices b_n ..
  uint32_t b_thr;   // threshold of the speculated balls (grid units)
};

__device__ __forceinline__ void lds_barrier() { __syncthreads(); }  // lowers to s_waitcnt lgkmcnt(0); s_barrier
// a block-uniform value moved to the scalar register file (state carried across iterations must not cost VGPRs)
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uni_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// ... in the one-wave shape only (the larger shapes' register tables are better off with the value where it is)
__device__ __forceinline__ uint32_t uni1_u(uint32_t v) { return NW == 1 ? uni_u(v) : v; }
__device__ __forceinline__ double uni_d(double v) {
  const uint64_t b = rpp::d2b(v);
  const uint32_t lo = uni_u((uint32_t)b), hi = uni_u((uint32_t)(b >> 32));
  return rpp::b2d(((uint64_t)hi << 32) | lo);
}

// ---- Integer operations across the 64 lanes of a wave that take no address register ------------------------------------
// __shfl* lowers to ds_bpermute_b32, whose lane-constant byte address ((lane +- o) << 2) is one more VGPR live across
// whatever surrounds the call: in the one-wave kernel it went to scratch and came back in front of every use (DESIGN
// 6.0h).  A DPP operand needs none: four row shifts scan the 16 lanes of a row, two row broadcasts carry the rows' last
// lanes on, and lane 63 then holds the reduction of the wave (v_readlane: the answer is a scalar).  Lanes that a step
// does not reach take the operation's identity (the `old` operand).  Every lane of the wave must be active.  All of them
// are integer operations under a total order: whatever the reduction tree, the bits are the same.
template <class Op>
__device__ __forceinline__ int wave_scan(int v, const int id, Op op) {
  v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x111, 0xf, 0xf, false));   // row_shr:1
  v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x118, 0xf, 0xf, false));   // row_shr:8
  v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1 and 3
  v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2 and 3
  return v;
}
// inclusive prefix sum over the lanes, and the wave's total from it
__device__ __forceinline__ int wave_prefix_sum(int v) {
  return wave_scan(v, 0, [](int a, int b) { return a + b; });
}
__device__ __forceinline__ int wave_total(int inclusive) { return __builtin_amdgcn_readlane(inclusive, 63); }
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane(
      wave_scan((int)v, -1, [](int a, int b) { return (int)min((uint32_t)a, (uint32_t)b); }), 63);
}
__device__ __forceinline__ int wave_imin(int v) {
  return __builtin_amdgcn_readlane(wave_scan(v, 0x7fffffff, [](int a, int b) { return min(a, b); }), 63);
}
// argmin of (value, index): the lowest index wins among equal values
__device__ __forceinline__ void wave_argmin(uint32_t v, int idx, uint32_t& wv, int& wi) {
  wv = wave_umin(v);
  wi = wave_imin(v == wv ? idx : 0x7fffffff);
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

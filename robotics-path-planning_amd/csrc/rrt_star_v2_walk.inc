// ---- scalar-path tree walks -------------------------------------------------------------------------------------
// A dependent VECTOR load costs 1.1 - 1.7 us while the other waves of the CU stream (it queues behind their loads in
// the CU's vector memory pipeline); a SCALAR load of the same address takes the scalar data path to L2 and costs
// 0.35 - 0.4 us under the same load (tools/ubench/lat_ubench.hip, profiles/r2_lat_ubench.txt).  The pointer chases of
// rewire -- a node's sibling links, the cost propagation over its subtree -- read one address at a time, so they run
// on the scalar unit: s_load with glc (served by L2, never by a stale scalar-cache line; the scalar cache is not
// coherent with vector stores).  The records are written by THIS wave's vector stores only, which reach L2 before
// `s_waitcnt vmcnt(0)` returns; the callers place that wait where an earlier store of the iteration could be read.
// the links of one node for a rewire -- parent, previous and next sibling -- in one scalar load of the 32-byte half that
// holds them: one round trip on one line
typedef uint32_t v8u __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void sload_links(const Node* nd, int node, int& par, int& pv, int& nxs) {
  const Node* p = nd + node;
  v8u r;
  asm volatile("s_load_dwordx8 %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(p) : "memory");
  nxs = (int)r[1];
  par = (int)r[6];
  pv = (int)r[7];
}
// the walk record of one node (the first 16 bytes of its line): one scalar load, one round trip on one line
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void sload_node(const Node* nd, int node, int& nxs, int& fcc, double& el) {
  const Node* p = nd + node;
  v4u r;
  asm volatile("s_load_dwordx4 %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(p) : "memory");
  fcc = (int)r.x;
  nxs = (int)r.y;
  el = rpp::b2d((uint64_t)r.z | ((uint64_t)r.w << 32));
}
// Sample i of the instance's stream S (Ctx::samp, rrt_samples.hip.h), a block-uniform value: the stream was written
// before the launch and is constant during it, so the scalar cache may serve it (no glc); four samples share a line
__device__ __forceinline__ void sload_sample(const v2d* S, int i, double& sx, double& sy) {
  const v2d* p = S + __builtin_amdgcn_readfirstlane(i);
  v4u r;
  asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(p) : "memory");
  sx = rpp::b2d((uint64_t)r.x | ((uint64_t)r.y << 32));
  sy = rpp::b2d((uint64_t)r.z | ((uint64_t)r.w << 32));
}
// ... and three of them in one round trip
__device__ __forceinline__ void sload_samples3(const v2d* S, int i0, int i1, int i2, double* sx, double* sy) {
  const v2d *p0 = S + __builtin_amdgcn_readfirstlane(i0), *p1 = S + __builtin_amdgcn_readfirstlane(i1),
            *p2 = S + __builtin_amdgcn_readfirstlane(i2);
  v4u a, b, d;
  asm volatile("s_load_dwordx4 %0, %3, 0x0\n\ts_load_dwordx4 %1, %4, 0x0\n\ts_load_dwordx4 %2, %5, 0x0\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(b), "=&s"(d)
               : "s"(p0), "s"(p1), "s"(p2)
               : "memory");
  sx[0] = rpp::b2d((uint64_t)a.x | ((uint64_t)a.y << 32));
  sy[0] = rpp::b2d((uint64_t)a.z | ((uint64_t)a.w << 32));
  sx[1] = rpp::b2d((uint64_t)b.x | ((uint64_t)b.y << 32));
  sy[1] = rpp::b2d((uint64_t)b.z | ((uint64_t)b.w << 32));
  sx[2] = rpp::b2d((uint64_t)d.x | ((uint64_t)d.y << 32));
  sy[2] = rpp::b2d((uint64_t)d.z | ((uint64_t)d.w << 32));
}

constexpr int CE = (NU + 63) / 64;  // near candidates per lane when a wave holds the candidate list in registers

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
// The rest of a cost walk with one sibling chain per lane (one-wave shape).  Every round trip gathers the records of
// up to 64 nodes, one 16-byte load per lane: a node's first child continues its lane's chain (at the node's new
// cost), its next sibling joins the LDS list of pending chains (at the parent's cost), and idle lanes take pending
// chains at the start of each round.  The rounds are bounded by the height of the first-child / next-sibling tree, not
// by the node count: in the long tail of propagations (thousands of nodes, DESIGN 5.2) that is several times fewer
// round trips, each a dependent vector gather.  (cur, cp) and st[0, sp) are what the scalar walk left.  Returns the nodes
// rewritten, or -1 when more than `cap` chains are pending.  Near candidates' LDS costs are not refreshed: the caller
// re-reads them.
__device__ __forceinline__ int propagate_lanes(Node* nd, int cur, double cp, Sh2& sh, int sp, int cap) {
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
      const Kid k = nd[(uint32_t)vn].k;
      nxs = k.next_sib;
      fcc = k.first_child;
      el = k.elen;
    }
    const double vcp = sh.cval[lane];
    const double nc = vcp + el;   // calc_new_cost :1375-1377
    if (vn >= 0) nd[(uint32_t)vn].cost = nc;
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
// `reread` tells the caller to refresh the later candidates' LDS costs from the records.  Returns the nodes rewritten, or -1
// when the sibling stack (LDS, at most cap entries) is full: the caller redoes the subtree with the global-stack walk
// (recomputation is idempotent).
__device__ __forceinline__ int propagate_scalar(Node* nd, int root_fc, double root_cost, Sh2& sh,
                                                const int (&my_uidx)[CE], int vec_after, int cap, bool& reread,
                                                unsigned long long* walks) {
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
      const int r = propagate_lanes(nd, cur, cp, sh, sp, cap);
      if (lane == 0) atomicAdd(walks, r < 0 ? PROP_WALK_FULL : 1ull);   // no return value: nothing waits on it
      return r < 0 ? -1 : cnt + r;
    }
    int nxs, fcc;
    double el;
    sload_node(nd, cur, nxs, fcc, el);
    const double nc = cp + el;   // calc_new_cost :1375-1377
    if (lane == 0) nd[cur].cost = nc;
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

// The record forms of rppk::propagate and rppk::link_child (the general kernel and the other planners keep the array
// forms).  The global-stack walk that redoes a subtree whose sibling stack ran full: one lane, explicit stack, every
// descendant of `root` gets cost = parent cost + elen, the value calc_new_cost (rrt_04:1375-1377) computes.
__device__ inline int propagate_rec(Node* nd, int32_t* __restrict__ stack, int root) {
  int sp = 0, count = 0;
  stack[sp++] = root;
  while (sp) {
    const int p = stack[--sp];
    const double cp = nd[p].cost;
    for (int ch = nd[p].k.first_child; ch >= 0; ch = nd[ch].k.next_sib) {
      nd[ch].cost = cp + nd[ch].k.elen;
      stack[sp++] = ch;
      count++;
    }
  }
  return count;
}
__device__ inline void link_child_rec(Node* nd, int ch, int par) {
  nd[ch].parent = par;
  nd[ch].prev_sib = -1;
  if (par >= 0) {
    const int f = nd[par].k.first_child;
    nd[ch].k.next_sib = f;
    if (f >= 0) nd[f].prev_sib = ch;
    nd[par].k.first_child = ch;
  } else {
    nd[ch].k.next_sib = -1;
  }
}

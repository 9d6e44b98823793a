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
  GHead* head;      // [gcells] {entries per cell, overflow block + 1 (0: none)}: one 8-byte load
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

// a cell's head: count and overflow block in one 8-byte load
__device__ __forceinline__ GHead ld_head(const GHead* p) { return *p; }
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
    g.head[i] = GHead{0, 0};
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
    const int k = on ? atomicAdd(&g.head[cell].cnt, 1) : 0;
    const uint64_t nb = __ballot(on && k == GRID_CAP0);   // cells that need their overflow block now
    if (on && k == GRID_CAP0) {
      const int b = g.pool_next + __popcll(nb & lt_mask) + 1;
      if (b <= g.pool_blocks) g.head[cell].blk = b;
    }
    g.pool_next += __popcll(nb);
    __threadfence();
    if (on && k < GRID_CAP0) {
      g.ent[(int64_t)cell * GRID_CAP0 + k] = grid_entry(i, q);
    } else if (on && k < GRID_CAPT) {
      const int b = g.head[cell].blk;
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
  const GHead hd = ld_head(g.head + cell);
  const int k = hd.cnt;
  int b = hd.blk;
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
    }
    if (threadIdx.x == 0) g.pool[(int64_t)(b - 1) * GRID_CAP1 + (k - GRID_CAP0)] = e;
  }
  if (threadIdx.x == 0) g.head[cell] = GHead{k + 1, b};
}

// Node `node`, at packed position q until now, leaves its cell: the cell's last entry takes its place.
__device__ __forceinline__ void grid_remove(GridS& g, int node, uint32_t q) {
  const int lane = threadIdx.x & 63;
  const int cell = grid_cell(g, q);
  const GHead hd = ld_head(g.head + cell);
  const int k = hd.cnt, b = hd.blk;
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
  if (lane == 0) g.head[cell].cnt = k - 1;
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
  uint32_t wb;
  int wi;
  wave_argmin(b, bi, wb, wi);
  uint32_t ws = wave_umin(bi == wi ? s : b);
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
  cq = uni_u(cq);
  thr = uni_u(thr);
  for (int attempt = first_attempt; attempt < 3; attempt++) {
    int x0, y0, nwx, nc, D;
    rw = uni_i(rw);
    if (!grid_window(g, cq, rw, x0, y0, nwx, nc, D)) return false;
    D = uni_i(D);
    int cell = 0, cn = 0, cb = 0;
    if (lane < nc) {
      cell = (y0 + lane / nwx) * g.gn + x0 + lane % nwx;
      const GHead hd = ld_head(g.head + cell);
      cn = hd.cnt;
      cb = hd.blk;
    }
    if (__ballot(cn > GRID_CAPT) != 0ull) return false;
    const int inc = wave_prefix_sum(cn);
    const int tot = wave_total(inc);
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
    D[c] = uni_i(D[c]);
    const int l = lane - npairs;
    if (l >= 0 && l < nc) {
      cid = c;
      cell = (y0 + l / nwx) * g.gn + x0 + l % nwx;
    }
    npairs += nc;
  }
  if (npairs > 64) return -1;
  if (cid >= 0) {
    const GHead hd = ld_head(g.head + cell);
    cn = hd.cnt;
    cb = hd.blk;
  }
  if (__ballot(cn > GRID_CAPT) != 0ull) return 0;
  const int inc = wave_prefix_sum(cn);
  const int tot = wave_total(inc);
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
  // the pass's own centres, threshold and window are wave-uniform: as scalars they are operands of every qdist and
  // compare below, not registers that live (or go to scratch) across the centres
  qq = uni_u(qq);
  thr = uni_u(thr);
  sq = uni_u(sq);
  rwn = uni_i(rwn);
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

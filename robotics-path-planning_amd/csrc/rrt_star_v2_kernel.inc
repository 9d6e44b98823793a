// ---------------------------------------------------------------------------
#define ST_ADD(k, v) do { if (threadIdx.x == 0) sh.stat[k] += (long long)(v); } while (0)
enum { S_ITER, S_EU, S_ER, S_NH, S_NU, S_RW, S_PR, S_SN, S_AB, S_AB2, S_EX, S_NUMAX, S_FB, S_QA, S_RIDE };   // per-launch counters (Sh2::stat, lane 0)
// a ball of squared radius r2 (world units) + the mirror's margin qm as a threshold in integer grid units, rounded up
__device__ __forceinline__ uint32_t ball_thr_grid(double r2, double qm, double qinv) {
  const double rr = __builtin_sqrt(r2) + qm;
  const double thr_gd = rr * rr * qinv * qinv * (1.0 + 1e-6) + 1.0;
  return thr_gd < 4.0e9 ? (uint32_t)thr_gd : 4000000000u;
}
// Goal shortcut: when the sample (sx, sy) is the goal and nodes lie exactly on it, d == 0 there and min() keeps the lowest
// index (:1200), first_goal
__device__ __forceinline__ bool on_goal(int first_goal, double gx, double gy, double sx, double sy) {
  return first_goal >= 0 && sx == gx && sy == gy;
}
__device__ __forceinline__ void nearest_on_goal(int first_goal, double gx, double gy, int& ni, double& nx, double& ny,
                                                double& best, double& second) {
  ni = first_goal;
  nx = gx;
  ny = gy;
  best = 0.0;
  second = rpp::dinf();
}
// Block-wide argmin over a pass's hit list h = 0 .. k-1: at(h, idx, hx, hy) fetches a hit, keep(hx, hy) filters, dist(hx, hy)
// values it; the lowest index wins among equals (:1200); the runner-up value is tracked only with SECOND.
template <bool SECOND, class At, class Keep, class Dist>
__device__ __forceinline__ void hit_argmin(int k, At at, Keep keep, Dist dist, Sh2& sh, double& gbest, int& gidx,
                                           double& gsecond, double& gx, double& gy) {
  double best = rpp::dinf(), second = rpp::dinf(), bx = 0.0, by = 0.0;
  int bidx = 0x7fffffff;
  for (int h = threadIdx.x; h < k; h += TPB) {
    int idx;
    double hx, hy;
    at(h, idx, hx, hy);
    if (!keep(hx, hy)) continue;
    const double d = dist(hx, hy);
    if (d < best || (d == best && idx < bidx)) {
      if (SECOND) second = best;
      best = d;
      bidx = idx;
      bx = hx;
      by = hy;
    } else if (SECOND && d < second) {
      second = d;
    }
  }
  lds_barrier();
  block_argmin_xy(best, bidx, second, bx, by, sh, gbest, gidx, gsecond, gx, gy);
}
// Margin test of a nearest answer of the 16-bit stage (best db, runner-up ds: distances in world units; bq: the best squared
// grid distance; the winner lies in the 4-node group grp of a tree of gn nodes) against the nearest node appended since the
// pass (distance dl, exact; index li at lx, ly).  Returns 1 with the nearest node in (ni, nx, ny), else 0: undecided.
// group(hx, hy) gives lane L the coordinates of node grp + (L & 3).
template <class Group>
__device__ __forceinline__ int margin_fold(const Ctx& c, double qm, double dl, int li, double lx, double ly, double db,
                                           double ds, uint32_t bq, int grp, int gn, uint32_t sq, Group group, int& ni,
                                           double& nx, double& ny) {
  if (dl < db - qm) {
    ni = li;
    nx = lx;
    ny = ly;
    return 1;
  }
  // the winner is exact only below the saturation bound; find it inside its group
  if (ds - db > 2.0 * qm && dl > db + qm && bq < QSAT) {
    double hx, hy;
    group(hx, hy);
    return resolve_group(c, grp, gn, hx, hy, sq, bq, ni, nx, ny) ? 1 : 0;
  }
  return 0;
}
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
  // one line per node: cost, the links and elen live here during the launch (built from cost[], kid[], parent[],
  // prev_sib[] below, written back to them at the end); x[], y[], xq[] stay current as arrays at every write too
  Node* nd = c.node + off;
  int32_t* hits = c.hits + off;
  int32_t* stack = c.stack + off;
  uint32_t* __restrict__ xq = c.xq + off;
  const double qm = c.q_m;
  const double qinv = c.q_inv;   // world -> grid units of the 16-bit mirror
  const double qm_grid = c.q_m * c.q_inv;
  const uint32_t goal_q = uni_u(rppk::quant16(c, I->goal[0], I->goal[1]));   // the goal's grid cell (a scalar: every qdist and compare takes it as an operand)
  int q_amb = 0;            // the fused 16-bit pass could not decide the pending nearest query ...
  uint32_t q_amb_bq = 0u;   // ... and this bounds the nearest node's squared grid distance (candidate pass, below)
  int first_goal = I->first_goal;
  int goal_dups = I->goal_dups;   // exact duplicates of node first_goal appended so far (valid while first_goal >= 0)

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
      sh.overflow = 0;
      sh.om = om;
    }
  }
  lds_barrier();
  int n = __builtin_amdgcn_readfirstlane(I->n), it = __builtin_amdgcn_readfirstlane(I->it);   // block-uniform: keep them scalar
  const double gx = I->goal[0], gy = I->goal[1];
  // the samples of this instance, drawn before the plan's first launch (rrt_samples.hip.h): iteration `it` consumes S[it]
  const v2d* S = reinterpret_cast<const v2d*>(c.samp) + (int64_t)inst * c.max_iter;
  // grid index of the mirror (one-wave shape): rebuilt from xq[] at every launch, kept current at every xq[] write
  GridS gs = {};
  gs.ok = 0;
  if constexpr (NW == 1) {
    if (c.grid) {
      const int64_t gi = (int64_t)inst;
      gs.head = c.ghead + gi * c.gcells;
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
  // the records of nodes [0, n) from the arrays, 64 nodes per wave and round (like the index: resume and re-plan need
  // nothing else)
  {
    const double* cost = c.cost + off;
    const Kid* kid = c.kid + off;
    const int32_t* parent = c.parent + off;
    const int32_t* prev_sib = c.prev_sib + off;
    for (int i = tid; i < n; i += TPB) {
      Node r;
      r.k = kid[i];
      r.cost = cost[i];
      r.parent = parent[i];
      r.prev_sib = prev_sib[i];
      r.x = x[i];
      r.y = y[i];
      r.xq = xq[i];
      r.pad[0] = r.pad[1] = r.pad[2] = 0u;
      nd[i] = r;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // in L2 before a scalar load of another wave asks for them
    lds_barrier();
  }
  if (tid == 0) {
    for (int k = 0; k < 15; k++) sh.stat[k] = 0;
    sh.b_n = 0;
    sh.b_thr = 0u;
  }
  int have_nearest = 0, ni = 0;
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
  // which starts the scheme again; the samples ahead are S[it + 1 ..], read where they are needed.
  // Bytes per iteration: 4 n -> 4 n / (1 + ks) while every iteration rides.
  // What the scheme carries from iteration to iteration lives in LDS (Sh2, in the room the generator's state left),
  // written by lane 0 and read by every lane of the one wave -- no global round trip, and nothing of it in a register
  // file that the streaming loop needs whole: sh.ax / sh.ay nodes appended since the pass, sh.set[e] set record e of a
  // ring of four: {centre x, y, nearest best, runner-up (world units squared), ball hits (-1: no ball), list offset,
  // nearest group (-1: none), best squared grid distance}.  Registers keep the ring head and counts only.  The balls'
  // hit lists stay in the free tail of hits[].
  constexpr int SPEC_CAPS = 2048 / (KSM > 0 ? KSM : 1);   // hits[stride - 2048, stride): the balls' hit lists
  const int spec_base = (int)c.stride - 2048;
  const int KS_RUN = NW == 1 ? (c.spec2 < KSM ? c.spec2 : KSM) : 0;
  const bool SPEC_ON = KS_RUN > 0;
  constexpr int KA = KSM > 0 ? KSM : 1;
  static_assert(KSM <= 3, "rings of four");
  int ns = 0, shead = 0;                               // query sets not yet used
  int na = 0;                                          // nodes appended since the pass: indices B_n .. B_n + na - 1
  // the tree size the pass scanned and the balls' threshold: Sh2::b_n / b_thr (lane 0 writes at the pass, read where used)
  // Nearest node of the next iteration's sample: the pass's answer (set record at shead) over [0, B_n) + the na nodes
  // appended since (indices B_n ..; the lowest index wins among equals, :1200).  margin_fold with the nearest of
  // the new nodes.  Returns 1 with the node in (ni, nqx, nqy), 2 when the 16-bit stage cannot
  // decide (o_bq bounds the squared grid distance), else 0.
  auto fold_n2 = [&](uint32_t& o_bq) -> int {
    const double* R = sh.set[shead];
    double s2x, s2y;
    sload_sample(S, it + 1, s2x, s2y);
    const double nb = R[2], nsec = R[3], grpd = R[6], bqd = R[7];
    const int B_n = uni_i(sh.b_n);
    double axv[4], ayv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      axv[j] = sh.ax[j];
      ayv[j] = sh.ay[j];
    }
    o_bq = 0xffffffffu;
    if (grpd < 0.0) return 0;
    if (on_goal(first_goal, gx, gy, s2x, s2y)) {
      nearest_on_goal(first_goal, gx, gy, ni, nqx, nqy, gbest, gsecond);
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
    if (margin_fold(c, qm, dl, li, lx, ly, db, ds, bq, grp, B_n, rppk::quant16(c, s2x, s2y),
                    [&](double& hx, double& hy) { hx = x[grp + (tid & 3)]; hy = y[grp + (tid & 3)]; },   // padding is readable
                    ni, nqx, nqy))
      return 1;
    o_bq = bq;
    return bq < QSAT ? 2 : 0;
  };
  PH_DECL

  for (int step = 0; step < iters && it < c.max_iter && !stop; step++, it++) {
    ST_ADD(S_ITER, 1);
    // ---------------- sample :1132-1153
    double rx, ry;
    sload_sample(S, it, rx, ry);
    PH(0);
    // ---------------- nearest :1197-1202
    ST_ADD(S_AB2, 16 * (int64_t)n);   // + 24 per obstacle, added per iteration at the end of the launch
    const double r2 = c.r2tab[n + 1];   // find_near_nodes radius for this tree size (requested early, used later)
    const double r2b = SPEC_ON ? c.r2tab[n + 2] : 0.0;   // ... and for the next one (speculated balls: the largest they can need)
    if (!have_nearest) {
      bool done = false;
      if (on_goal(first_goal, gx, gy, rx, ry)) {
        nearest_on_goal(first_goal, gx, gy, ni, nqx, nqy, gbest, gsecond);
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
            const auto at = [&](int h, int& idx, double& hx, double& hy) { hit_at2q(nd, hits, sh, h, idx, hx, hy); };
            hit_argmin<true>(kc, at, [](double, double) { return true; },
                             [=](double hx, double hy) { return rpp::fast_d2(hx - rx, hy - ry); }, sh, gbest, ni, gsecond, nqx, nqy);
            if (gbest != 0.0 && gsecond <= gbest * (1.0 + FILTER_EPS)) {
              // candidates inside the filter margin of the minimum: the exact ** 2 decides, lowest index on ties (:1200)
              ST_ADD(S_EX, 1);
              const double lim = gbest * (1.0 + FILTER_EPS);
              hit_argmin<false>(kc, at, [=](double hx, double hy) { return !(rpp::fast_d2(hx - rx, hy - ry) > lim); },
                                [=](double hx, double hy) { return rpp::py_d2(hx - rx, hy - ry); }, sh, d1, ni, d2, nqx, nqy);
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
      hit_argmin<false>(kraw, [&](int h, int& idx, double& hx, double& hy) { hit_at2(x, y, hits, sh, h, idx, hx, hy); },
                        [](double, double) { return true; }, [=](double hx, double hy) { return rpp::py_d2(hx - rx, hy - ry); },
                        sh, d1, ni, d2, nqx, nqy);
    }
    PH(1);

    // ---------------- steer + collision of the extension :1051-1059
    // Without libm calls in the usual case, like the candidate edges (eval_edges_dual2): once the tree is dense the nearest
    // node is closer than expand_dis, the walk of :1100-1106 ends within one resolution of the sample and :1108-1113 snaps
    // the new node ONTO the sample.  "Snapped" is certain when rpp::snap_certain says so (rpp_core.h), and the points along the
    // straight line decide the collision test unless an obstacle's threshold lies within `tol` of the closest point.
    // Anything in doubt -- a nearest node further than expand_dis (the new node is then the walk's end point: cos / sin
    // needed), the remaining distance at the resolution, an obstacle in the band -- takes the exact form below.
    if (tid == 0) {
      const double dx = rx - nqx, dy = ry - nqy;
      const double d = rpp::py_hypot(dx, dy);
      const int ne = (int)__builtin_floor(d / c.res);
      const bool sure = d <= c.expand_dis && rpp::snap_certain(d, ne, c.res, nqx, nqy, rx, ry);
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
        const double* R = sh.set[shead];
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
      double p1x = 0.0, p1y = 0.0;       // the next iteration's sample (read with do_pf)
      int64_t pass_b = 0, pass_n = n;    // 16-bit stage: bytes and nodes its passes read
      if (use_spec) {
        // the nodes appended since that pass join the ball by the pass's own grid test, in index order
        int k2 = spec_k0;
        const int off0 = spec_off0;
        const int B_n = uni_i(sh.b_n);
        const uint32_t B_thr = uni_u(sh.b_thr);
        const uint32_t cq = rppk::quant16(c, nx, ny);
        double axv[KA], ayv[KA];
#pragma unroll
        for (int j = 0; j < KA; j++) {
          axv[j] = sh.ax[j];
          ayv[j] = sh.ay[j];
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
        const uint32_t thr_gi = uni1_u(ball_thr_grid(r2, qm, qinv));
        const int rw_gi = (int)__builtin_sqrt((double)thr_gi) + 1;   // its window half-width (grid index)
        if (do_pf) {
          sload_sample(S, it + 1, p1x, p1y);
          pf_goal = on_goal(first_goal, gx, gy, p1x, p1y);
        }
        if (do_pf && !pf_goal) {
          pf_sq = uni1_u(rppk::quant16(c, p1x, p1y));
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
              thr2 = uni_u(ball_thr_grid(r2b, qm, qinv));
              if (uni_i(qdist(goal_q, pf_sq) <= thr2)) kmax = 0;
            }
            if (kmax > 0) {
              // samples i + 2 .. i + 1 + kmax, next in the stream (an entry past kmax is read nowhere: the last sample's copy)
              double qxv[KA], qyv[KA];
#pragma unroll
              for (int j = 0; j < KA; j++) qxv[j] = qyv[j] = 0.0;
              if constexpr (KA == 3) {
                sload_samples3(S, it + 2, it + 2 + (1 < kmax ? 1 : kmax - 1), it + 2 + (2 < kmax ? 2 : kmax - 1), qxv, qyv);
              } else {
#pragma unroll
                for (int j = 0; j < KA; j++) sload_sample(S, it + 2 + (j < kmax ? j : kmax - 1), qxv[j], qyv[j]);
              }
              // ball j is about sample i + 1 + j: p1 for j = 0, entry j - 1 of those after that
              int ks = kmax;
#pragma unroll
              for (int j = 1; j < KA; j++)
                if (uni_i(j < ks && qdist(goal_q, rppk::quant16(c, qxv[j - 1], qyv[j - 1])) <= thr2)) ks = j;
              SpecQ sp[KA];
#pragma unroll
              for (int j = 0; j < KA; j++) {
                const bool on = j < ks;
                const double cxj = j == 0 ? p1x : qxv[j > 0 ? j - 1 : 0], cyj = j == 0 ? p1y : qyv[j > 0 ? j - 1 : 0];
                sp[j].qq = uni_u(on ? rppk::quant16(c, cxj, cyj) : pf_sq);   // wave-uniform: scalars (the pass reads them as operands)
                sp[j].thr = on ? thr2 : 0u;    // unused set: radius 0 about a centre whose hits nobody reads
                sp[j].sq = uni_u(rppk::quant16(c, on ? qxv[j] : p1x, on ? qyv[j] : p1y));
                sp[j].off = spec_base + j * SPEC_CAPS;
                sp[j].cap = SPEC_CAPS;
                if (tid == 0) {   // the record's centre now: nothing of the queue has to stay in registers over the pass
                  double* R = sh.set[j];
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
              ns = ks;
              shead = 0;
              na = 0;
              if (tid == 0) {
                sh.b_n = n;
                sh.b_thr = thr2;
                const double qs2 = c.q_step * c.q_step;
#pragma unroll
                for (int j = 0; j < KA; j++) {
                  const bool on = j < ks;
                  double* R = sh.set[j];
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
          nearest_on_goal(first_goal, gx, gy, o_ni, o_x, o_y, pf_best, pf_second);
          return 1;
        }
        const double dxl = ax - p1x, dyl = ay - p1y;
        const double dl = __builtin_sqrt(dxl * dxl + dyl * dyl);
        const double db = __builtin_sqrt(pf_best), ds = __builtin_sqrt(pf_second);
        return margin_fold(c, qm, dl, aidx, ax, ay, db, ds, pf_bq, pf_grp, pf_n, pf_sq,
                           [&](double& hx, double& hy) { hx = pf_x; hy = pf_y; }, o_ni, o_x, o_y);
      };
      PH(4);
      int pend_p, pend_fc;
      double pend_cost;
      build_candidates(nd, nx, ny, r2, hits, kraw, sh, pend_p, pend_cost, pend_fc);
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
            sload_links(nd, u, par, pv, nxs);
            if (tid == 0) {
              // the identity re-pointing of :1369-1372 with integer links: leave the old parent's child list ...
              if (pv >= 0) {
                nd[pv].k.next_sib = nxs;
              } else {
                nd[par].k.first_child = nxs;
              }
              if (nxs >= 0) nd[nxs].prev_sib = pv;
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
                nd[u].x = sh.e0.ex;
                nd[u].y = sh.e0.ey;
                nd[u].xq = rppk::quant16(c, sh.e0.ex, sh.e0.ey);
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
                nd[u].k.elen = rpp::py_hypot(sh.e0.ex - wx, sh.e0.ey - wy);
                for (int ch = sh.ufc[es]; ch >= 0; ch = nd[ch].k.next_sib)
                  nd[ch].k.elen = rpp::py_hypot(nd[ch].x - sh.e0.ex, nd[ch].y - sh.e0.ey);
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
              if (!moved_now) nd[u].k.elen = sh.uhyp[es];
              nd[u].cost = ec;
              sh.ucur[es] = ec;
              // ... and become a child of the node about to be appended
              nd[u].parent = newidx;
              nd[u].prev_sib = -1;
              nd[u].k.next_sib = sh.last_fc;
              if (sh.last_fc >= 0) nd[sh.last_fc].prev_sib = u;
              sh.last_fc = u;
              sh.n_rw++;
            }
            if (moved_now) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the children's new elen
            PH(13);
            bool reread = false;
            int np = propagate_scalar(nd, root_fc, ec, sh, my_uidx,   // :1373
                                      NW == 1 ? c.prop_vec : -1, NW == 1 ? c.prop_cap : (1 << 30), reread,
                                      (unsigned long long*)&I->phase[PROP_WALK_SLOT]);
            if (np < 0) {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              if (tid == 0) sh.fcount = propagate_rec(nd, stack, u);
              np = sh.fcount;
              reread = true;
            }
            if (reread) {
              // later candidates may be descendants of the node just rewired: refresh their costs
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              for (int e = es + 1 + tid; e < nu; e += 64)
                if (sh.uflag[e] & 2) sh.ucur[e] = nd[sh.uidx[e]].cost;
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
          // link under the chosen parent; its current first child is in the LDS record (kept current above).  The node's
          // own line in one go; elen == hypot(new - parent) from the position the node ends up at
          const int f = sh.ufc[sel];
          Node r;
          r.k = Kid{sh.last_fc, f, sh.uhyp[sel]};
          r.cost = wcost;
          r.parent = wparent;
          r.prev_sib = -1;
          r.x = wx;
          r.y = wy;
          r.xq = rppk::quant16(c, wx, wy);
          r.pad[0] = r.pad[1] = r.pad[2] = 0u;
          nd[newidx] = r;
          if (f >= 0) nd[f].prev_sib = newidx;
          nd[wparent].k.first_child = newidx;
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
          nd[n].k.elen = el;
          nd[n].cost = nd[ni].cost + el;   // :1054-1056
          nd[n].k.first_child = -1;
          nd[n].x = nx;
          nd[n].y = ny;
          nd[n].xq = rppk::quant16(c, nx, ny);
          link_child_rec(nd, n, ni);
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
            sh.ax[na] = wx;
            sh.ay[na] = wy;
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
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // lane 0's last stores into the records, before any lane reads them
  lds_barrier();
  // cost, the links and elen of nodes [0, n) from the records to the arrays, whichever way the loop ended: the general
  // kernel, the getters and a next launch read the arrays
  {
    double* __restrict__ cost = c.cost + off;
    Kid* __restrict__ kid = c.kid + off;
    int32_t* __restrict__ parent = c.parent + off;
    int32_t* __restrict__ prev_sib = c.prev_sib + off;
    for (int i = tid; i < n; i += TPB) {
      const Kid k = nd[i].k;
      const double ci = nd[i].cost;
      const int pa = nd[i].parent, ps = nd[i].prev_sib;
      kid[i] = k;
      cost[i] = ci;
      parent[i] = pa;
      prev_sib[i] = ps;
    }
  }
  if (tid == 0) {
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

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
// coordinates gathered in f64 from the node's line, one 16-byte load
__device__ __forceinline__ void hit_at2q(const Node* nd, const int32_t* __restrict__ hits, const Sh2& sh, int h, int& idx,
                                         double& hx, double& hy) {
  int k = 0;
#pragma unroll
  for (int j = 0; j < NW - 1; j++) {
    if (k == j && h >= sh.wave_cnt[j]) {
      h -= sh.wave_cnt[j];
      k = j + 1;
    }
  }
  idx = (h < HWF) ? reinterpret_cast<const int32_t*>(sh.u.hit)[k * HWF + h] : hits[sh.wave_start[k] + h];
  const v2d xy = *reinterpret_cast<const v2d*>(&nd[idx].x);
  hx = xy.x;
  hy = xy.y;
}

// Exact re-check (dx**2 + dy**2 <= r**2 with the reference's libm pow) + the `.index` de-dup of rrt_04:1337,
// producing the candidate records.  cost / first child of each distinct candidate are requested here (from the line the
// coordinates came from) and first used after the edge evaluation.
__device__ __forceinline__ void build_candidates(const Node* nd, double qx, double qy,
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
        hit_at2q(nd, hits, sh, h, idx, hx, hy);
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
            pend_cost = nd[idx].cost;
            pend_fc = nd[idx].k.first_child;
          } else {
            sh.ucur[p] = nd[idx].cost;
            sh.ufc[p] = nd[idx].k.first_child;
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
      hit_at2q(nd, hits, sh, h, idx, hx, hy);
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
          pend_cost = nd[idx].cost;
          pend_fc = nd[idx].k.first_child;
        } else {
          sh.ucur[p] = nd[idx].cost;
          sh.ufc[p] = nd[idx].k.first_child;
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
//   * rpp::snap_certain (rpp_core.h) decides "snapped": d - n res <= res less a slack that grows with n and with the
//     coordinates (the reference's sum differs from n res d-hat by up to n ULP of the largest coordinate);
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
      // snapped unless the remaining distance is within the rule's slack of res (then only the exact additions can tell)
      unsure = !rpp::snap_certain(d, ne, c.res, fx, fy, tx, ty);
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

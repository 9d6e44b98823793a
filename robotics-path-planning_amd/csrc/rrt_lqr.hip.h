// rrt_lqr.hip.h -- LQR-RRT* iteration kernel (gfx950).
// Reference: /root/reference/src_path_planning/10_path_planning_01_rrt_09_lqr_rrt_star.py (rrt_09)
//   planning :1120-1155, steer :1174-1192 (csrc/rpp_lqr.h), check_collision :1292-1305, find_near_nodes :1371-1395,
//   choose_parent :1315-1355, rewire :1397-1430, calc_new_cost :1432-1442, propagate_cost_to_leaves :1444-1450,
//   search_best_goal_node :1357-1369, generate_final_course :1194-1203.
//
// One 64-lane wave per planning instance (a workgroup of one wave: __syncthreads is a wave barrier).  The tree lives in
// global memory as SoA: x, y, cost, parent, child lists (the records kid[] and prev_sib) and per node the endpoints of
// the edge that created its current entry (LqrArgs::ef: from x, from y, to x, to y -- the polyline is regenerated from
// them, rpp_lqr.h; no polyline pool).  The obstacle tile sits in LDS.
//
//   sample           lane 0 (MT19937 / Sobol replicas), broadcast through LDS
//   nearest          lanes over nodes, first minimum of (dx)**2 + (dy)**2, wave reduction
//   first steer      every lane the same edge (wave-uniform; 3-5 rollout steps)
//   near             lanes over nodes, ballot-ordered compaction of the raw list, `dist_list.index(d)` per entry
//   choose_parent    one lane per near entry: rollout, lengths, collision, endpoint; nothing else stored
//   rewire           one lane per near entry up front (new node -> entry); the sequential part compares costs and steers
//                    again only an entry whose node an earlier rewire of the same loop moved
//   propagate        level order, one lane per frontier node, each with its own rollout; bounded by the node count (a
//                    parent cycle -- the reference recurses without end -- stops the instance with RRTX_ST_REF_RAISES)
//   goal search      lanes over nodes, `.index` quirk, lowest-cost first index, index 0 = none
#pragma once
#include "rpp_lqr.h"
#include "rrt_kernels.hip.h"

namespace rppl {

using rppk::Ctx;
using rppk::Inst;
constexpr int TPB = 64;
constexpr int MAX_OBS = rppk::MAX_OBS;

struct LqrArgs {
  double* ef;          // [inst][stride][4] edge endpoints of each node (from x, from y, to x, to y)
  int32_t* nl;         // [inst][stride] near list (raw entries, `.index` applied)
  double* dscr;        // [inst][stride] distances of the raw near / goal lists
  double *cex, *cey, *clen;   // [inst][stride] per near entry: endpoint and course length of its edge
  int32_t* cflag;      // [inst][stride] per near entry: 0 blocked, 1 feasible, 2 rollout failed
  int32_t* moved;      // [inst][stride] iteration stamp (it + 1) of the last rewire that moved a node
  double step, goal_xy_th;
  int32_t nt;          // ceil(1 / step): resampling parameters per rollout segment
};

struct ShL {
  rpp::MT rng;
  double ox[MAX_OBS], oy[MAX_OBS], othr[MAX_OBS];
  double rx, ry;
  int32_t qtail, flag;
};

__device__ __forceinline__ void wave_argmin(double& v, int& i) {
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ov < v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

// compacts the nodes j < n with pred(j) into list[0..) in index order (dist[] gets d(j)); returns the count
template <class P>
__device__ __forceinline__ int compact(int n, int32_t* list, double* dist, P&& pred) {
  const int lane = threadIdx.x;
  int k = 0;
  for (int base = 0; base < n; base += 64) {
    const int j = base + lane;
    double d = 0.0;
    const bool hit = j < n && pred(j, d);
    const uint64_t m = __ballot(hit);
    if (hit) {
      const int pos = k + __popcll(m & ((1ull << lane) - 1ull));
      list[pos] = j;
      dist[pos] = d;
    }
    k += __popcll(m);
  }
  __syncthreads();
  return k;
}

// `[dl.index(d) for d in dl if ...]`: each entry becomes the first entry with the same distance (lanes over entries;
// every equal distance is itself in the list, and only at a lower position); tmp: scratch of k entries
__device__ __forceinline__ void apply_index_quirk(int k, int32_t* list, const double* dist, int32_t* tmp) {
  for (int e = threadIdx.x; e < k; e += 64) {
    const double d = dist[e];
    int32_t m = list[e];
    for (int q = 0; q < e; q++)
      if (dist[q] == d) {
        m = list[q];
        break;
      }
    tmp[e] = m;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < k; e += 64) list[e] = tmp[e];
  __syncthreads();
}

__global__ __launch_bounds__(TPB) void rrt_lqr_kernel(Ctx c, LqrArgs la, int iters) {
  __shared__ ShL sh;
  const int inst = c.inst_map ? c.inst_map[blockIdx.x] : blockIdx.x;
  const int tid = threadIdx.x;
  Inst* I = c.inst + inst;
  if (I->status & 1) return;
  const int64_t off = (int64_t)inst * c.stride;
  double* __restrict__ x = c.x + off;
  double* __restrict__ y = c.y + off;
  double* __restrict__ cost = c.cost + off;
  int32_t* parent = c.parent + off;
  rppk::Kid* kid = c.kid + off;
  int32_t* prev_sib = c.prev_sib + off;
  int32_t* queue = c.stack + off;
  double* ef = la.ef + 4 * off;
  int32_t* nl = la.nl + off;
  double* dscr = la.dscr + off;
  double* cex = la.cex + off;
  double* cey = la.cey + off;
  double* clen = la.clen + off;
  int32_t* cflag = la.cflag + off;
  int32_t* moved = la.moved + off;

  for (int i = tid; i < 624; i += TPB) sh.rng.mt[i] = I->rng.mt[i];
  const int ob = __builtin_amdgcn_readfirstlane(I->obs_base), om = __builtin_amdgcn_readfirstlane(I->obs_m);
  for (int i = tid; i < om; i += TPB) {
    sh.ox[i] = c.ox[ob + i];
    sh.oy[i] = c.oy[ob + i];
    sh.othr[i] = c.othr[ob + i];
  }
  if (tid == 0) {
    sh.rng.pos = I->rng.pos;
    sh.flag = 0;
  }
  __syncthreads();
  int n = I->n, it = I->it;
  rpp::Sobol sob = I->sobol;
  const double gx = I->goal[0], gy = I->goal[1];
  const double step = la.step;
  const int nt = la.nt;
  int64_t s_iter = 0, s_e = 0, s_nh = 0, s_rw = 0, s_pr = 0, s_sn = 0;
  int done = 0, raises = 0;

  auto edge = [&](double fx, double fy, double tx, double ty, int m) {
    return rpp::lqr_edge(fx, fy, tx, ty, step, nt, sh.ox, sh.oy, sh.othr, m);
  };
  // search_best_goal_node :1357-1369 -> index, or -1 (index 0 counts as none: `if last_index:`)
  auto goal_search = [&]() -> int {
    const int k = compact(n, nl, dscr, [&](int j, double& d) {
      d = rpp::py_hypot(x[j] - gx, y[j] - gy);
      return d <= la.goal_xy_th;
    });
    double best = rpp::dinf();
    int bi = 0x7fffffff;
    for (int e = tid; e < k; e += TPB) {
      const double d = dscr[e];
      bool canon = true;
      for (int q = 0; q < e && canon; q++) canon = dscr[q] != d;
      const int j = nl[e];
      if (canon && (cost[j] < best || bi == 0x7fffffff)) {
        best = cost[j];
        bi = j;
      }
    }
    // first minimum over the canonical entries in list order = lowest index among the minimal costs
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ov < best || (ov == best && oi < bi))) {
        best = ov;
        bi = oi;
      }
    }
    __syncthreads();
    return (bi == 0x7fffffff || bi == 0) ? -1 : bi;
  };
  // generate_final_course :1194-1203 + get_path_length, lane 0; polylines regenerated into cex / cey
  auto write_path = [&](int gi) {
    if (tid != 0) return;
    double* out = c.path_xy + (int64_t)inst * c.path_cap * 2;
    int np = 0, trunc = 0;
    double len = 0.0, lx = gx, ly = gy;
    auto put = [&](double px, double py) {
      if (np > 0) len += rpp::py_hypot(px - lx, py - ly);
      if (np < c.path_cap) {
        out[2 * np] = px;
        out[2 * np + 1] = py;
      } else {
        trunc = 1;
      }
      np++;
      lx = px;
      ly = py;
    };
    put(gx, gy);
    for (int nd = gi, guard = 0; parent[nd] >= 0 && guard <= n; nd = parent[nd], guard++) {
      const double* e = ef + 4 * nd;
      const int cnt = rpp::lqr_polyline(e[0], e[1], e[2], e[3], step, nt, cex, cey, (int)c.stride);
      for (int q = (cnt < c.stride ? cnt : (int)c.stride) - 1; q >= 0; q--) put(cex[q], cey[q]);
    }
    put(I->start[0], I->start[1]);
    I->path_n = np;
    I->goal_node = gi;
    I->status |= 2 | (trunc ? 8 : 0);
    c.results[inst].path_cost = len;
  };

  for (int stepi = 0; stepi < iters && it < c.max_iter && !done; stepi++, it++) {
    s_iter++;
    // ---------------- sample :1124-1127
    if (tid == 0) rppk::draw_sample(c, sh, sob, gx, gy);
    __syncthreads();
    const double rx = sh.rx, ry = sh.ry;
    // ---------------- nearest :1272-1277
    double best = rpp::dinf();
    int ni = 0x7fffffff;
    for (int j = tid; j < n; j += TPB) {
      const double d = rpp::py_d2(x[j] - rx, y[j] - ry);
      if (d < best || (ni == 0x7fffffff && !(d > best))) {
        best = d;
        ni = j;
      }
    }
    wave_argmin(best, ni);
    s_sn += n;
    // ---------------- steer :1129 + check_collision :1131
    const rpp::LqrEdge e0 = edge(x[ni], y[ni], rx, ry, om);
    s_e++;
    if (!e0.ok) {
      raises = 1;
      break;
    }
    const double ex = e0.ex, ey = e0.ey;
    int truthy = 1, nnear = -1;
    if (!e0.coll) {
      // ---------------- find_near_nodes :1371-1395 (radius table indexed by len(node_list) + 1)
      const double r2 = c.r2tab[n + 1];
      const int K = compact(n, nl, dscr, [&](int j, double& d) {
        d = rpp::py_d2(x[j] - ex, y[j] - ey);
        return d <= r2;
      });
      apply_index_quirk(K, nl, dscr, cflag);
      nnear = K;
      s_nh += K;
      s_sn += n;
      if (K == 0) {
        truthy = 0;
      } else {
        // ---------------- choose_parent :1315-1355, one lane per entry
        int bad = 0;
        for (int k = tid; k < K; k += TPB) {
          const int i = nl[k];
          const rpp::LqrEdge e = edge(x[i], y[i], ex, ey, om);
          bad |= !e.ok;
          const bool feas = e.ok && !e.coll && rpp::in_play_area(c.has_play, c.play_area, e.ex, e.ey);
          clen[k] = feas ? cost[i] + e.len : rpp::dinf();
          cex[k] = e.ex;
          cey[k] = e.ey;
        }
        s_e += K;
        if (__any(bad)) {
          raises = 1;
          break;
        }
        __syncthreads();
        double mc = rpp::dinf();
        int ks = 0x7fffffff;
        for (int k = tid; k < K; k += TPB)
          if (clen[k] < mc || (ks == 0x7fffffff && !(clen[k] > mc))) {
            mc = clen[k];
            ks = k;
          }
        wave_argmin(mc, ks);
        if (!(mc < rpp::dinf())) {
          truthy = 0;
        } else {
          // steer once more from the chosen parent (the same edge as candidate ks) and append :1352-1354, :1133
          const int p = nl[ks];
          const int nn = n;
          const double nx = cex[ks], ny = cey[ks];
          __syncthreads();
          if (tid == 0) {
            x[nn] = nx;
            y[nn] = ny;
            cost[nn] = mc;
            ef[4 * nn] = x[p];
            ef[4 * nn + 1] = y[p];
            ef[4 * nn + 2] = ex;
            ef[4 * nn + 3] = ey;
            kid[nn].first_child = -1;
            moved[nn] = 0;
            rppk::link_child(parent, kid, prev_sib, nn, p);
          }
          n++;
          __syncthreads();
          // ---------------- rewire :1397-1430: every entry's edge (new node -> entry) up front
          for (int k = tid; k < K; k += TPB) {
            const int i = nl[k];
            const rpp::LqrEdge e = edge(nx, ny, x[i], y[i], om);
            cflag[k] = !e.ok ? 2 : (!e.coll && rpp::in_play_area(c.has_play, c.play_area, e.ex, e.ey)) ? 1 : 0;
            cex[k] = e.ex;
            cey[k] = e.ey;
            clen[k] = e.len;
          }
          s_e += K;
          __syncthreads();
          const int stamp = it + 1;
          for (int k = 0; k < K && !raises; k++) {
            const int i = nl[k];
            int fl = cflag[k];
            double len = clen[k], tx = cex[k], ty = cey[k];
            if (moved[i] == stamp) {   // moved by an earlier rewire of this loop: steer to where it lies now
              const rpp::LqrEdge e = edge(nx, ny, x[i], y[i], om);
              fl = !e.ok ? 2 : (!e.coll && rpp::in_play_area(c.has_play, c.play_area, e.ex, e.ey)) ? 1 : 0;
              len = e.len;
              tx = e.ex;
              ty = e.ey;
              s_e++;
            }
            if (fl == 2) {
              raises = 1;
              break;
            }
            const double ecost = cost[nn] + len;
            if (!(fl == 1 && cost[i] > ecost)) continue;
            s_rw++;
            const double ox0 = x[i], oy0 = y[i];
            __syncthreads();
            if (tid == 0) {
              rppk::unlink_child(parent, kid, prev_sib, i);
              rppk::link_child(parent, kid, prev_sib, i, nn);
              x[i] = tx;
              y[i] = ty;
              cost[i] = ecost;
              ef[4 * i] = nx;
              ef[4 * i + 1] = ny;
              ef[4 * i + 2] = ox0;
              ef[4 * i + 3] = oy0;
              moved[i] = stamp;
              queue[0] = i;
              sh.qtail = 1;
            }
            __syncthreads();
            // ---------------- propagate_cost_to_leaves :1444-1450, level order
            int head = 0, tail = 1;
            while (head < tail) {
              for (int q = head + tid; q < tail; q += TPB) {
                const int f = queue[q];
                for (int ch = kid[f].first_child; ch >= 0; ch = kid[ch].next_sib) {
                  const rpp::LqrEdge e = edge(x[f], y[f], x[ch], y[ch], 0);
                  cost[ch] = e.ok ? cost[f] + e.len : rpp::dinf();
                  const int slot = atomicAdd(&sh.qtail, 1);
                  if (slot < n) queue[slot] = ch;
                }
              }
              __syncthreads();
              head = tail;
              tail = sh.qtail;
              if (tail > n) {   // more visits than nodes: the parent graph has a cycle
                raises = 1;
                break;
              }
            }
            s_pr += tail - 1;
          }
          if (raises) break;
        }
      }
    }
    if (inst == c.trace_inst && tid == 0) {
      c.tr_rx[it] = rx;
      c.tr_ry[it] = ry;
      c.tr_near[it] = ni;
      c.tr_nn[it] = nnear;
    }
    // ---------------- early exit :1139-1142 (planning's own keyword, not the constructor's)
    if (!c.until_max && truthy) {
      s_sn += n;
      const int gi = goal_search();
      if (gi >= 0) {
        write_path(gi);
        done = 1;
      }
      __syncthreads();
    }
  }
  if (raises) {
    done = 1;
  } else if (!done && it >= c.max_iter) {
    // ---------------- after the loop :1146-1153
    s_sn += n;
    const int gi = goal_search();
    if (gi >= 0) write_path(gi);
    done = 1;
  }
  __syncthreads();
  for (int i = tid; i < 624; i += TPB) I->rng.mt[i] = sh.rng.mt[i];
  if (tid == 0) {
    I->rng.pos = sh.rng.pos;
    I->sobol = sob;
    I->n = n;
    I->it = it;
    if (done) I->status |= 1;
    if (raises) I->status |= 32;
    I->iterations += s_iter;
    I->edges_unique += s_e;
    I->edges_ref += s_e;
    I->near_hits += s_nh;
    I->rewires += s_rw;
    I->propagated += s_pr;
    I->scan_nodes += s_sn;
    c.results[inst].n_nodes = n;
    c.results[inst].status = I->status;
  }
}

// Node.path_x / path_y of every node of one instance, regenerated from the edge records, one thread per node:
// pass 1 (px == nullptr) writes the point counts, pass 2 the points at the offsets the host summed
__global__ void lqr_polylines_kernel(const double* ef, const int32_t* parent, int n, double step, int nt, int32_t* cnt,
                                     const int64_t* poff, double* px, double* py) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* e = ef + 4 * (int64_t)i;
  if (parent[i] < 0) {
    if (!px) cnt[i] = 0;
    return;
  }
  if (!px) {
    cnt[i] = rpp::lqr_polyline(e[0], e[1], e[2], e[3], step, nt, nullptr, nullptr, 0);
    return;
  }
  rpp::lqr_polyline(e[0], e[1], e[2], e[3], step, nt, px + poff[i], py + poff[i], cnt[i]);
}

}  // namespace rppl

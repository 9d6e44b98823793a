// steer_batch.hip.h -- the steering functions as batch kernels of their own (gfx950): shortest Dubins / Reeds-Shepp
// curve between many pose pairs, and the LQR rollout between many point pairs, without a planner around them.
// Reference: /root/reference/src_path_planning/10_path_planning_00_dubins_path.py plan_dubins_path :109-197 and
//   10_path_planning_00_reeds_shepp_path.py reeds_shepp_path_planning :506-515 (the same functions, line for line, as the
//   copies inside rrt_05 / rrt_06); the scalar pieces are csrc/rpp_dubins.h and csrc/rpp_rs.h.
//   10_path_planning_00_lqr_path.py LQRPlanner.lqr_planning :24-66 (= rrt_09 :944-986) with rrt_09's sample_path
//   :1157-1172, steer :1174-1192, check_collision :1292-1305 and calc_new_cost :1432-1442; scalar pieces csrc/rpp_lqr.h.
//
// Path lengths differ per pair, so the work is two stages with a CSR layout between them:
//   stage 1  steer_dubins_solve  one lane per pair: dubins_prepare over the ordered word list -> word, segment lengths,
//                                point count; the prepared DubinsPlan goes to global memory when points are wanted.
//            steer_rs_solve      16 lanes per pair, 4 pairs per wave: lane t evaluates the variants t, t + 16, t + 32 of the
//                                48 (12 word families x 4 symmetries) and writes its candidate records into the pair's
//                                table in LDS; lane 0 of the pair then runs set_path's de-duplication and
//                                paths.index(min(...)) over that table in the reference's order.  A variant that raises or
//                                reports "step size too large" hides every later one: the table is read in order, so
//                                the later variants are computed speculatively and never looked at.
//            steer_rs_course     (points wanted) one lane per pair: generate_local_course prepared for random access.
//            steer_lqr_solve     one lane per pair: the rollout once for its point count (a rollout that fails costs its
//                                1001 steps and nothing else), then once more for the end point and the length.  No
//                                per-pair record goes to stage 2: the pair's two points are the record.
//   offsets  exclusive prefix sum of the point counts (host, one int32 per pair down, one int64 per pair up).
//   stage 2  steer_fill          one lane per output point: binary search of the point index in offsets, then
//                                dubins_point / rs_point / lqr_point, which are random-access by point index (lqr_point
//                                re-runs the recurrence to the point's segment: <= 10 steps at the reference's
//                                settings, 19 with goal_dist = 0).  STORE writes the
//                                point (a Bezier point with its curvature when that is wanted: bezier_eval on row k of
//                                the weight table, which neighbouring lanes read at neighbouring rows); CHECK tests it against the obstacle list (rpp_collide.h) and takes the lowest
//                                obstacle index any point of the pair touches into hit[pair].
//            steer_bezier_solve  one lane per pair, after bezier_weights_kernel has filled the solve's weight table
//                                (rpp_bezier.h): the control points from the poses (or as given), written as the pair's
//                                stage-2 record; then the walk over the n_points points -- the same trip count in every
//                                lane, the table row at a wave-uniform address -- for the length and, when curvature is
//                                wanted, the largest |curvature|.  <4> keeps the control points in registers; <0> (any
//                                other number of given control points) reads them back from the record.
//   candidates  steer_rs_all / steer_dubins_all, steer_select_free, steer_gather_points (at the end of this file): every
//                                candidate curve of a pair instead of the shortest one -- calc_paths :483-503 of the
//                                Reeds-Shepp script -- through the same course and fill kernels, and the choice of the
//                                shortest candidate that touches no obstacle.
// Lengths-only is stage 1 alone (no plan, no course, no offsets) -- unless an obstacle list is set: then stage 1 runs as
// for points and stage 2 runs with CHECK alone, so no point is ever written.
// Product mode: pair p of ns x ng is (start p / ng, goal p % ng), formed here; the host never builds the product.
#pragma once
#include "curve_check.hip.h"
#include "rpp_bezier.h"
#include "rpp_lqr.h"
#include "rpp_rs.h"

namespace rppsb {

constexpr int KIND_DUBINS = 0, KIND_RS = 1;   // include/rrtx.h RRTX_STEER_DUBINS / RRTX_STEER_RS
constexpr int KIND_LQR = 2;                   // not a value of the ABI: rrtx_steer_solve_lqr is this kind's entry point
constexpr int KIND_BEZIER = 3;                // neither: rrtx_steer_solve_bezier / rrtx_steer_solve_bezier_cp
constexpr int ST_OK = 0, ST_NO_PATH = 1, ST_RAISES_ZERODIV = 2, ST_RAISES_VALUE = 3;   // include/rrtx.h RRTX_STEER_*
constexpr int TPB = 256;            // steer_dubins_solve, steer_rs_course, steer_fill
constexpr int RS_TPB = 64;          // steer_rs_solve: one wave
constexpr int RS_LANES = 16;        // lanes per pair
constexpr int RS_PAIRS = RS_TPB / RS_LANES;
using rppc::CHECK_NONE, rppc::CHECK_LINEAR, rppc::CHECK_INDEX, rppc::csr_row;   // steer_fill's CHECK (curve_check.hip.h)
constexpr int RS_KEPT = 3;          // table state: set_path kept this candidate (0 none, 1 candidate, 2 step too large)

struct Args {
  const double* starts;   // (ns, 3); LQR: (ns, 2)
  const double* goals;    // (ng, 3); pair mode: (n, 3); LQR: 2 columns
  const double* curv;     // one value per pair, or nullptr: curv0
  double curv0, step;
  double max_time, goal_dist;   // LQR: MAX_TIME, GOAL_DIST of the LQRPlanner
  int32_t nt;             // LQR: resampling parameters per rollout segment (rpp::lqr_nt), 0 = the raw rollout
  int64_t n, ng;          // pairs; product mode: goals per start
  int32_t product, want_points;
  int32_t order[6];       // Dubins: the words to try, in this order (the first wins ties)
  int32_t n_order;
  int32_t* status;        // [n]
  int32_t* nseg;          // [n]  LQR: rollout points len(rx)
  double* total;          // [n]  the absolute values of seglen added up in segment order; LQR: see steer_lqr_solve
  double* seglen;         // [n][5] as the reference returns them (divided by the curvature)
  char* modes;            // [n][8] letters, NUL padded
  int32_t* npts;          // [n]
  rpp::DubinsPlan* dplan; // [n]
  rpp::RsCourse* course;  // [n]
  double* ends;           // [n][2]  LQR: the last point
  int32_t* flag;          // set when any pair is not ST_OK
  const int64_t* offsets; // [n + 1]
  double *px, *py, *pyaw; // [offsets[n]]
  // collision check (nullptr / 0 without an obstacle list)
  const double* obs;      // [n_obs] rows (ox, oy, thr), thr = (size + robot_radius) ** 2 from the host
  int64_t n_obs;
  int32_t* hit;           // [n]  stage 1: -1 (ST_OK) / -2 (no curve); stage 2: the lowest obstacle index touched
  rppo::Map omap;         // CHECK_INDEX: the grid over the same list
  // Bezier (curv / curv0 hold the offset per pair / of all pairs)
  const double* bez_w;    // [bez_np][3 bez_m - 3] the weight table of this solve
  double* bez_cp;         // [n][bez_m][2] control points: stage 1 writes them, or finds them there (bez_given)
  double* pk;             // [offsets[n]] curvature per point, or nullptr
  double* kmax;           // [n] max |curvature| over the curve's points, or nullptr
  int32_t bez_m, bez_np;  // control points per curve, points per curve
  int32_t bez_given;      // the control points came from the host
  // every candidate of a pair (steer_*_all below): the records, counts, offsets and hits above are then per candidate, n
  // counts candidates, and poses and curvature are those of the candidate's pair
  const int32_t* cand_pair;   // [n] the pair of each candidate, or nullptr: a record per pair
  int8_t* pdir;               // [offsets[n]] Reeds-Shepp: Path.directions per point, or nullptr
};

__device__ inline void pair_poses(const Args& a, int64_t p, double* s, double* g) {
  const int64_t si = a.product ? p / a.ng : p, gi = a.product ? p % a.ng : p;
  for (int i = 0; i < 3; i++) {
    s[i] = a.starts[3 * si + i];
    g[i] = a.goals[3 * gi + i];
  }
}
__device__ inline double pair_curv(const Args& a, int64_t p) { return a.curv ? a.curv[p] : a.curv0; }
// the pair whose poses and curvature record r is built from
__device__ inline int64_t record_pair(const Args& a, int64_t r) { return a.cand_pair ? a.cand_pair[r] : r; }
__device__ inline void pair_xy(const Args& a, int64_t p, double* s, double* g) {   // LQR: rows (x, y)
  const int64_t si = a.product ? p / a.ng : p, gi = a.product ? p % a.ng : p;
  for (int i = 0; i < 2; i++) {
    s[i] = a.starts[2 * si + i];
    g[i] = a.goals[2 * gi + i];
  }
}

// ---- Dubins, stage 1 ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void steer_dubins_solve(Args a) {
  const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (p >= a.n) return;
  double s[3], g[3];
  pair_poses(a, p, s, g);
  const double curv = pair_curv(a, p);
  rpp::DubinsPlan P;
  rpp::dubins_prepare(&P, s[0], s[1], s[2], g[0], g[1], g[2], curv, a.order, a.n_order, true);
  char* m = a.modes + 8 * p;
  double* sl = a.seglen + 5 * p;
  for (int i = 0; i < 8; i++) m[i] = 0;
  sl[3] = sl[4] = 0.0;
  if (!P.ok) {   // no word of the list is feasible (the reference fails on b_mode = None)
    sl[0] = sl[1] = sl[2] = 0.0;
    a.status[p] = ST_NO_PATH;
    a.nseg[p] = 0;
    a.total[p] = 0.0;
    a.npts[p] = 0;
    if (a.hit) a.hit[p] = -2;
    atomicOr(a.flag, 1);
    return;
  }
  double tot = 0.0;
  for (int i = 0; i < 3; i++) {
    const double l = P.len[i] / curv;   // :315
    sl[i] = l;
    tot += rpp::dabs(l);
    const int md = P.mode[i];
    m[i] = md == 0 ? 'L' : (md == 1 ? 'S' : 'R');
  }
  a.status[p] = ST_OK;
  a.nseg[p] = 3;
  a.total[p] = tot;
  a.npts[p] = P.total;
  if (a.hit) a.hit[p] = -1;
  if (a.want_points) a.dplan[p] = P;
}

// ---- Reeds-Shepp, stage 1 -----------------------------------------------------------------------------------------
// The candidate table of one pair (what rs_plan keeps as st[48], d[48][5], ct[48][6] in one lane's private memory)
struct RsTable {
  double d[48][5];
  double L[48];        // sum |d| in segment order (set_path :1063)
  int32_t st[48];      // rs_variant's return value; RS_KEPT once set_path has taken the candidate
  int32_t n[48];
  uint32_t code[48];   // rs_code of the word: equal codes <=> equal ctypes lists
  char ct[48][8];
};

// set_path :1061-1080 over the variants in the reference's order + paths.index(min(paths, key=abs(L))) :1436, as
// rpp::rs_select does it, with the kept list held in the table itself (st == RS_KEPT, L) instead of two private arrays.
// Returns the chosen k, -1: None, < -1: the reference raises.
__device__ inline int rs_select_lds(RsTable& T, double step, double maxc) {
  int np = 0;
  for (int k = 0; k < 48; k++) {
    const int s = T.st[k];
    if (s == 0) continue;
    if (s < 0) return s;    // -3 / -4: raised inside this variant
    if (s == 2) return -1;  // "Step size too large": generate_path returns [] there and then
    const double L = T.L[k];
    const uint32_t code = T.code[k];
    bool skip = false;
    for (int i = 0; i < k; i++)
      if (T.st[i] == RS_KEPT && T.code[i] == code && (T.L[i] - L) <= step) skip = true;
    if (skip || L <= step) continue;
    T.st[k] = RS_KEPT;
    np++;
  }
  if (np == 0) return -1;
  int bi = -1;
  double bl = 0.0;
  for (int k = 0; k < 48; k++) {
    if (T.st[k] != RS_KEPT) continue;
    const double l = rpp::dabs(T.L[k] / maxc);
    if (bi < 0 || l < bl) {   // strict: the first of equal lengths, as list.index finds it
      bl = l;
      bi = k;
    }
  }
  return bi;
}

__global__ __launch_bounds__(RS_TPB) void steer_rs_solve(Args a) {
  __shared__ RsTable tab[RS_PAIRS];
  const int grp = threadIdx.x / RS_LANES, t = threadIdx.x % RS_LANES;
  const int64_t p = (int64_t)blockIdx.x * RS_PAIRS + grp;
  const bool live = p < a.n;
  RsTable& T = tab[grp];
  double s[3], g[3], maxc = 1.0;
  rpp::RsFrame F;
  if (live) {
    pair_poses(a, p, s, g);
    maxc = pair_curv(a, p);
    rpp::rs_frame(s[0], s[1], s[2], g[0], g[1], g[2], maxc, a.step, &F);
    const double sdth = rpp_glibc_sin(F.dth), cdth = rpp_glibc_cos(F.dth);
    for (int j = 0; j < 48 / RS_LANES; j++) {
      const int k = t + RS_LANES * j;   // k = 4 * word family + symmetry, the reference's order
      double d[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      char ct[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int nn = 0;
      const int st = rpp::rs_variant_sc(k >> 2, k & 3, F, sdth, cdth, d, ct, &nn);
      T.st[k] = st;
      T.n[k] = nn;
      for (int i = 0; i < 5; i++) T.d[k][i] = d[i];
      for (int i = 0; i < 8; i++) T.ct[k][i] = ct[i];
      T.L[k] = st == 1 ? rpp::rs_sum_abs(d, nn) : 0.0;
      T.code[k] = st == 1 ? rpp::rs_code(ct) : 0u;
    }
  }
  __syncthreads();
  if (!live || t != 0) return;
  const int sel = rs_select_lds(T, F.step, maxc);
  char* m = a.modes + 8 * p;
  double* sl = a.seglen + 5 * p;
  for (int i = 0; i < 8; i++) m[i] = 0;
  for (int i = 0; i < 5; i++) sl[i] = 0.0;
  a.npts[p] = 0;
  if (sel < 0) {
    a.status[p] = sel == -1 ? ST_NO_PATH : (sel == -3 ? ST_RAISES_ZERODIV : ST_RAISES_VALUE);
    a.nseg[p] = 0;
    a.total[p] = 0.0;
    if (a.hit) a.hit[p] = -2;
    atomicOr(a.flag, 1);
    return;
  }
  const int nl = T.n[sel];
  double tot = 0.0;
  for (int i = 0; i < nl; i++) {
    const double l = T.d[sel][i] / maxc;   // :1420
    sl[i] = l;
    tot += rpp::dabs(l);
    m[i] = T.ct[sel][i];
  }
  a.status[p] = ST_OK;
  a.nseg[p] = nl;
  a.total[p] = tot;
  if (a.hit) a.hit[p] = -1;
  if (a.want_points) {   // the chosen word in curvature units, for steer_rs_course
    rpp::RsCourse& C = a.course[p];
    for (int i = 0; i < 5; i++) C.len[i] = T.d[sel][i];
    for (int i = 0; i < 6; i++) C.ct[i] = T.ct[sel][i];
    C.nl = nl;
  }
}

__global__ __launch_bounds__(TPB) void steer_rs_course(Args a) {
  const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (p >= a.n || (!a.cand_pair && a.status[p] != ST_OK)) return;   // (every candidate has a word)
  rpp::RsCourse& C = a.course[p];
  double len[5];
  char ct[6];
  for (int i = 0; i < 5; i++) len[i] = C.len[i];
  for (int i = 0; i < 6; i++) ct[i] = C.ct[i];
  const int nl = C.nl;
  double s[3], g[3];
  const int64_t pr = record_pair(a, p);
  pair_poses(a, pr, s, g);
  rpp::rs_course(len, ct, nl, s[0], s[1], s[2], pair_curv(a, pr), a.step, &C);
  a.npts[p] = C.total;
}

// ---- LQR, stage 1 -------------------------------------------------------------------------------------------------
// total[p] is Python's left-to-right sum of math.hypot over consecutive points: of the resampled points (nt > 0; what
// steer :1189 adds to the cost and calc_new_cost :1440 returns), or of the rollout points themselves (nt == 0; the
// lqr_path script returns no length, this one is the project's definition).  ends[p] is px[-1], py[-1] -- the last
// resampled point, which is not the last rollout point (sample_path leaves that one out) -- or rx[-1], ry[-1].
__global__ __launch_bounds__(TPB) void steer_lqr_solve(Args a) {
  const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (p >= a.n) return;
  double s[2], g[2];
  pair_xy(a, p, s, g);
  const int nw = rpp::lqr_rollout(s[0], s[1], g[0], g[1], a.max_time, a.goal_dist, [](double, double, double, double) {});
  a.nseg[p] = nw;
  if (nw == 0) {   // "Cannot found path": lqr_planning returns [], []
    a.status[p] = ST_NO_PATH;
    a.total[p] = 0.0;
    a.npts[p] = 0;
    a.ends[2 * p] = a.ends[2 * p + 1] = 0.0;
    if (a.hit) a.hit[p] = -2;
    atomicOr(a.flag, 1);
    return;
  }
  double len = 0.0, ex = 0.0, ey = 0.0;
  if (a.nt > 0) {
    rpp::lqr_walk(s[0], s[1], g[0], g[1], a.step, a.nt, a.max_time, a.goal_dist, [&](int k, double qx, double qy) {
      if (k > 0) len += rpp::py_hypot(qx - ex, qy - ey);
      ex = qx;
      ey = qy;
    });
  } else {
    rpp::lqr_rollout(s[0], s[1], g[0], g[1], a.max_time, a.goal_dist, [&](double wx, double wy, double rx, double ry) {
      len += rpp::py_hypot(rx - wx, ry - wy);
      ex = rx;
      ey = ry;
    });
  }
  a.status[p] = ST_OK;
  a.total[p] = len;
  a.npts[p] = a.nt > 0 ? (nw - 1) * a.nt : nw;
  a.ends[2 * p] = ex;
  a.ends[2 * p + 1] = ey;
  if (a.hit) a.hit[p] = -1;
}

// ---- Bezier, the weight table and stage 1 ----------------------------------------------------------------------------
// One entry per thread, with the pow replica, so that no curve ever calls pow for a weight and the table does not depend on
// the host's libm.  At the reference's sizes (100 points, 4 control points) it is 900 doubles; it stays in global memory:
// stage 1 reads a row at a wave-uniform address through the constant address space (scalar loads), stage 2 reads 9 to 45
// doubles of a table the L2 holds whole (<= 1.4 MB at 4096 points x 16 control points, 7.2 KB at the reference's).
__global__ __launch_bounds__(TPB) void bezier_weights_kernel(double* w, int32_t n_points, int32_t m) {
  const int row = rpp::bezier_row_len(m);
  const int idx = blockIdx.x * TPB + threadIdx.x;   // n_points * row <= 4096 * 45
  if (idx >= n_points * row) return;
  w[idx] = rpp::bezier_table_entry(n_points, m, idx / row, idx % row);
}

template <int M>
__global__ __launch_bounds__(TPB) void steer_bezier_solve(Args a) {
  const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (p >= a.n) return;
  const int m = M ? M : a.bez_m;
  double* rec = a.bez_cp + 2 * (int64_t)m * p;
  const rpp::BezierRow table = (rpp::BezierRow)a.bez_w;
  double len, km;
  if (M == 4) {
    double P[8];
    if (a.bez_given) {
      for (int i = 0; i < 8; i++) P[i] = rec[i];
    } else {
      double s[3], g[3];
      pair_poses(a, p, s, g);
      rpp::bezier_cp4(s[0], s[1], s[2], g[0], g[1], g[2], pair_curv(a, p), P);
      for (int i = 0; i < 8; i++) rec[i] = P[i];
    }
    rpp::bezier_walk<4>(P, 4, table, a.bez_np, a.kmax != nullptr, &len, &km);
  } else {
    rpp::bezier_walk<0>(rec, m, table, a.bez_np, a.kmax != nullptr, &len, &km);
  }
  a.status[p] = ST_OK;
  a.nseg[p] = m;
  a.total[p] = len;
  a.npts[p] = a.bez_np;
  if (a.kmax) a.kmax[p] = km;
  if (a.hit) a.hit[p] = -1;
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------
// <KIND, true, CHECK_NONE> is the fill kernel alone.  The lanes past the last point, and hit[]: curve_check.hip.h.
template <int KIND, bool STORE, int CHECK>
__global__ __launch_bounds__(TPB) void steer_fill(Args a) {
  int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int64_t total = a.offsets[a.n];
  const bool live = idx < total;
  if (!live) {
    if (!CHECK) return;
    idx = total - 1;   // the launch has total > 0
  }
  const int64_t lo = csr_row(a.offsets, a.n, idx);   // the pair (or candidate) the point belongs to
  const int k = (int)(idx - a.offsets[lo]);
  double x, y, yaw = 0.0, kk = 0.0;
  if (KIND == KIND_DUBINS) {
    rpp::dubins_point(a.dplan[lo], k, pair_curv(a, record_pair(a, lo)), &x, &y, &yaw);
  } else if (KIND == KIND_RS) {
    rpp::rs_point(a.course[lo], k, &x, &y, &yaw);
    if (STORE && live && a.pdir) a.pdir[idx] = (int8_t)rpp::rs_point_dir(a.course[lo], k);
  } else if (KIND == KIND_LQR) {
    double s[2], g[2];
    pair_xy(a, lo, s, g);
    rpp::lqr_point(s[0], s[1], g[0], g[1], a.step, a.nt, k, &x, &y);
  } else {
    const int m = a.bez_m;
    double o[6];
    rpp::bezier_eval<0>(a.bez_cp + 2 * (int64_t)m * lo, m, a.bez_w + (int64_t)k * rpp::bezier_row_len(m),
                        STORE ? (a.pk ? 2 : 1) : 0, o);
    x = o[0];
    y = o[1];
    if (STORE) {
      yaw = rpp_glibc_atan2(o[3], o[2]);
      if (a.pk) kk = rpp::bezier_curvature(o[2], o[3], o[4], o[5]);
    }
  }
  if (STORE && live) {
    a.px[idx] = x;
    a.py[idx] = y;
    if (KIND != KIND_LQR) a.pyaw[idx] = yaw;   // an LQR course has no yaw
    if (KIND == KIND_BEZIER && a.pk) a.pk[idx] = kk;
  }
  if (CHECK) rppc::check_point<CHECK>(a.obs, a.n_obs, a.omap, a.hit, lo, x, y);
}

// ---- every candidate curve of a pair, and the shortest one that is free -------------------------------------------------
// Reference: 10_path_planning_00_reeds_shepp_path.py calc_paths :483-503 -- the whole list set_path :141-159 kept, of which
//   reeds_shepp_path_planning :506-515 is the minimum; for Dubins the candidate of list entry w is what plan_dubins_path
//   (10_path_planning_00_dubins_path.py :109-197) returns with selected_types=[w].
// The layout is CSR twice: pairs -> candidates (cand_off) and candidates -> points (Args::offsets).
//   count   steer_rs_all<false> / steer_dubins_all<false>: status and the number of candidates per pair.
//   emit    <true>, after the host's prefix sum: one record per candidate at cand_off[pair] + its place in the list, in the
//           per-candidate arrays of an Args whose n is the number of candidates and whose cand_pair leads back to the pair.
//   course, fill   steer_rs_course and steer_fill over those Args: a candidate is a curve like any other.
//   select  steer_select_free: one lane per pair walks its candidates' keys and hits (rpp::pick_free) and writes the chosen
//           candidate's record as the pair's row of an ordinary result; steer_gather_points then copies its points.
constexpr int CAND_MAX_WORDS = 16;   // entries of a Dubins word list (duplicates are candidates of their own)

struct CandArgs {
  int64_t n_pairs;
  int32_t order[CAND_MAX_WORDS];   // Dubins: the word list
  int32_t n_order;
  int32_t* status;           // [n_pairs]
  int32_t* ncand;            // [n_pairs]
  const int64_t* cand_off;   // [n_pairs + 1]
  int32_t* pair;             // [n candidates] = Args::cand_pair
  int32_t* variant;          // RS: 4 * word family + symmetry; Dubins: the position in the word list
  double* key;               // what the kind's planner minimises: RS abs(L / maxc) (= Path.L), Dubins the cost of :1220
  int32_t *chosen, *rank, *nfree;   // [n_pairs] steer_select_free; chosen: a candidate index, -1 where the pair has none
};

// 16 lanes per pair evaluate the 48 variants into the pair's table and lane 0 runs set_path's walk, as in steer_rs_solve;
// then every RS_KEPT entry is a candidate, in table order (the order set_path appended them in).  The emit pass evaluates
// the table again instead of keeping 48 entries per pair between the passes: nothing is sized by the worst case.
template <bool EMIT>
__global__ __launch_bounds__(RS_TPB) void steer_rs_all(Args a, CandArgs c) {
  __shared__ RsTable tab[RS_PAIRS];
  __shared__ int32_t sel_of[RS_PAIRS];
  const int grp = threadIdx.x / RS_LANES, t = threadIdx.x % RS_LANES;
  const int64_t p = (int64_t)blockIdx.x * RS_PAIRS + grp;
  const bool live = p < c.n_pairs;
  RsTable& T = tab[grp];
  double s[3], g[3], maxc = 1.0;
  rpp::RsFrame F;
  if (live) {
    pair_poses(a, p, s, g);
    maxc = pair_curv(a, p);
    rpp::rs_frame(s[0], s[1], s[2], g[0], g[1], g[2], maxc, a.step, &F);
    const double sdth = rpp_glibc_sin(F.dth), cdth = rpp_glibc_cos(F.dth);
    for (int j = 0; j < 48 / RS_LANES; j++) {
      const int k = t + RS_LANES * j;
      double d[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      char ct[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int nn = 0;
      const int st = rpp::rs_variant_sc(k >> 2, k & 3, F, sdth, cdth, d, ct, &nn);
      T.st[k] = st;
      T.n[k] = nn;
      for (int i = 0; i < 5; i++) T.d[k][i] = d[i];
      for (int i = 0; i < 8; i++) T.ct[k][i] = ct[i];
      T.L[k] = st == 1 ? rpp::rs_sum_abs(d, nn) : 0.0;
      T.code[k] = st == 1 ? rpp::rs_code(ct) : 0u;
    }
  }
  __syncthreads();
  if (live && t == 0) {
    const int sel = rs_select_lds(T, F.step, maxc);   // < 0: raised or [] -- whatever was kept before is hidden
    sel_of[grp] = sel;
    if (!EMIT) {
      int nc = 0;
      if (sel >= 0)
        for (int k = 0; k < 48; k++) nc += T.st[k] == RS_KEPT;
      c.ncand[p] = nc;
      c.status[p] = sel >= 0 ? ST_OK : (sel == -1 ? ST_NO_PATH : (sel == -3 ? ST_RAISES_ZERODIV : ST_RAISES_VALUE));
      if (sel < 0) atomicOr(a.flag, 1);
    }
  }
  if (!EMIT) return;
  __syncthreads();
  if (!live || sel_of[grp] < 0) return;
  for (int j = 0; j < 48 / RS_LANES; j++) {   // lane t emits the kept ones of its own three variants
    const int k = t + RS_LANES * j;
    if (T.st[k] != RS_KEPT) continue;
    int place = 0;
    for (int i = 0; i < k; i++) place += T.st[i] == RS_KEPT;
    const int64_t ci = c.cand_off[p] + place;
    const int nl = T.n[k];
    char* m = a.modes + 8 * ci;
    double* sl = a.seglen + 5 * ci;
    double tot = 0.0;
    for (int i = 0; i < 8; i++) m[i] = i < nl ? T.ct[k][i] : 0;
    for (int i = 0; i < 5; i++) {
      const double l = i < nl ? T.d[k][i] / maxc : 0.0;   // :500
      sl[i] = l;
      tot += rpp::dabs(l);
    }
    c.pair[ci] = (int32_t)p;
    c.variant[ci] = k;
    c.key[ci] = rpp::dabs(T.L[k] / maxc);   // :501, and the key of :512
    a.nseg[ci] = nl;
    a.total[ci] = tot;
    a.npts[ci] = 0;
    if (a.hit) a.hit[ci] = -1;
    if (a.want_points) {
      rpp::RsCourse& C = a.course[ci];
      for (int i = 0; i < 5; i++) C.len[i] = T.d[k][i];
      for (int i = 0; i < 6; i++) C.ct[i] = T.ct[k][i];
      C.nl = nl;
    }
  }
}

// One lane per pair: one DubinsPlan per feasible entry of the word list, each prepared as a list of that one word.
template <bool EMIT>
__global__ __launch_bounds__(TPB) void steer_dubins_all(Args a, CandArgs c) {
  const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (p >= c.n_pairs) return;
  double s[3], g[3];
  pair_poses(a, p, s, g);
  const double curv = pair_curv(a, p);
  int nc = 0;
  for (int q = 0; q < c.n_order; q++) {
    rpp::DubinsPlan P;
    rpp::dubins_candidate(&P, s[0], s[1], s[2], g[0], g[1], g[2], curv, c.order[q]);
    if (!P.ok) continue;
    if (EMIT) {
      const int64_t ci = c.cand_off[p] + nc;
      char* m = a.modes + 8 * ci;
      double* sl = a.seglen + 5 * ci;
      for (int i = 0; i < 8; i++) m[i] = 0;
      sl[3] = sl[4] = 0.0;
      double tot = 0.0;
      for (int i = 0; i < 3; i++) {
        const double l = P.len[i] / curv;   // :315
        sl[i] = l;
        tot += rpp::dabs(l);
        const int md = P.mode[i];
        m[i] = md == 0 ? 'L' : (md == 1 ? 'S' : 'R');
      }
      c.pair[ci] = (int32_t)p;
      c.variant[ci] = q;
      c.key[ci] = rpp::dubins_key(P);
      a.nseg[ci] = 3;
      a.total[ci] = tot;
      a.npts[ci] = P.total;
      if (a.hit) a.hit[ci] = -1;
      if (a.want_points) a.dplan[ci] = P;
    }
    nc++;
  }
  if (!EMIT) {
    c.ncand[p] = nc;
    c.status[p] = nc ? ST_OK : ST_NO_PATH;
    if (!nc) atomicOr(a.flag, 1);
  }
}

// One lane per pair.  ca: the candidates' Args (records and hits in); pa: an ordinary per-pair result (row out).  A pair
// without candidates gets the row steer_*_solve writes for its status.
__global__ __launch_bounds__(TPB) void steer_select_free(Args pa, Args ca, CandArgs c) {
  const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (p >= c.n_pairs) return;
  const int64_t c0 = c.cand_off[p];
  const int nc = (int)(c.cand_off[p + 1] - c0);
  char* m = pa.modes + 8 * p;
  double* sl = pa.seglen + 5 * p;
  c.rank[p] = 0;
  c.nfree[p] = 0;
  if (nc == 0) {
    c.chosen[p] = -1;
    for (int i = 0; i < 8; i++) m[i] = 0;
    for (int i = 0; i < 5; i++) sl[i] = 0.0;
    pa.nseg[p] = 0;
    pa.total[p] = 0.0;
    pa.npts[p] = 0;
    pa.hit[p] = -2;
    return;
  }
  int ch, rank, nfree;
  rpp::pick_free(c.key + c0, ca.hit + c0, nc, &ch, &rank, &nfree);
  const int64_t ci = c0 + ch;
  c.chosen[p] = (int32_t)ci;
  c.rank[p] = rank;
  c.nfree[p] = nfree;
  for (int i = 0; i < 8; i++) m[i] = ca.modes[8 * ci + i];
  for (int i = 0; i < 5; i++) sl[i] = ca.seglen[5 * ci + i];
  pa.nseg[p] = ca.nseg[ci];
  pa.total[p] = ca.total[ci];
  pa.npts[p] = ca.npts[ci];
  pa.hit[p] = ca.hit[ci];
}

// One lane per point of the chosen curves: the point the candidates' fill launch already computed
__global__ __launch_bounds__(TPB) void steer_gather_points(Args pa, Args ca, CandArgs c) {
  const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (idx >= pa.offsets[pa.n]) return;
  const int64_t p = csr_row(pa.offsets, pa.n, idx);
  const int64_t src = ca.offsets[c.chosen[p]] + (idx - pa.offsets[p]);
  pa.px[idx] = ca.px[src];
  pa.py[idx] = ca.py[src];
  pa.pyaw[idx] = ca.pyaw[src];
}

}  // namespace rppsb

// rrtx_api.hip -- host side of the C ABI declared in include/rrtx.h.
// Owns device memory, uploads parameters / RNG state, launches the planner
// kernel in bounded chunks of iterations on the handle's HIP stream, and copies
// results back.  There is no CPU planning path in this library.
// This file holds the planner handle; the other objects and the handle-free calls are included at its end, one file each.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <functional>
#include <mutex>
#include <new>
#include <set>
#include <vector>

#include "rrtx_host.h"
#include "rrt_kernels.hip.h"
#include "obstacle_map.hip.h"
#include "rrt_star_v2.hip.h"
#include "rrt_samples.hip.h"
#include "rrt_informed.hip.h"
#include "rrt_dubins.hip.h"
#include "rrt_rs.hip.h"
#include "rrt_bitstar.hip.h"
#include "rrt_bitstar_wave.hip.h"
#include "path_smooth.hip.h"
#include "rrt_lqr.hip.h"
#include "rrt_track.hip.h"
#include "course_gather.hip.h"
#include "goal_query.hip.h"
#include "goal_track.hip.h"
#include "steer_batch.hip.h"
#include "spline_batch.hip.h"
#include "bspline_batch.hip.h"
#include "bspline_smooth.hip.h"
#include "armnav_batch.hip.h"
#include "armik_batch.hip.h"
#include "armdh_batch.hip.h"

using rppk::Ctx;
using rppk::Inst;
using rppk::Result;

static_assert(sizeof(rppt::Params) == sizeof(rrtx_track_params), "rrtx_track_params mirrors rppt::Params");
static_assert(sizeof(rppt::Outcome) == sizeof(rrtx_track_outcome), "rrtx_track_outcome mirrors rppt::Outcome");
static_assert(sizeof(rppt::Record) == sizeof(rrtx_track_record), "rrtx_track_record mirrors rppt::Record");
static_assert(sizeof(rppgt::Outcome) == sizeof(rrtx_goal_track_outcome), "rrtx_goal_track_outcome mirrors rppgt::Outcome");
static_assert(rppc::CHECK_NONE == 0 && rppc::CHECK_LINEAR == 1 && rppc::CHECK_INDEX == 2, "with_store_check (rrtx_host.h) counts as the kernels do");

// What a build of the obstacle grid leaves on the device (build_obstacle_grid, rrtx_api_obsmap.inc): cell_start (cells + 2
// entries, the last run is the wide list) and the sorted records
struct ObsGrid {
  DevBuf cell_start, items;
  rppo::Geom g = {0.0, 0.0, 1.0, 0, 0};
  int64_t m = 0, n_items = 0, n_wide = 0;
  double build_ms = 0.0;

  // the grid as the point-query kernels read it (rpp_obsgrid.h point_first_hit)
  rppo::Map map() const { return rppo::Map{g, cell_start.as<const int32_t>(), items.as<const rppo::Item>()}; }
};

struct rrtx_handle : DevObj {
  rrtx_params p;
  Ctx c;
  int64_t stride = 0;
  int n_inst = 0;
  int m_max = 0;                // largest obstacle count of any instance (capacity and workgroup-shape decisions)
  bool planned = false;
  std::vector<Inst> host_inst;  // staging for seeds / starts / obstacle rows before the first plan
  std::vector<double> obst;     // every instance's obstacle rows (x, y, size) as given, in device-table order
  // device obstacle table: ox, oy, othr and the sizes (path smoothing) of all rows, `obs_cap` rows each, one allocation
  DevBuf obs_buf;
  int64_t obs_cap = 0;
  // the obstacle map (rrtx_set_obstacle_map, rrtx_api_obsmap.inc): while `on`, every instance's rows of the table are empty
  // and the plans run rppk::rrt_plan_map_kernel on `items`
  struct ObsMapState {
    bool on = false;
    ObsGrid grid;
    int tile = rppk::MAX_OBS;
  } om;
  int trace_inst = -1;    // instance the next plan traces (rrtx_enable_trace)
  int traced_inst = -1;   // instance whose trace the last completed plan recorded; -1 none
  rrtx_stats stats;
  int64_t phase[16] = {0};
  std::vector<void*> allocs;   // the fixed-size tables (dalloc); buffers that are regrown are DevBuf members
  // one rrtx_plan in progress (rrtx_plan_begin / rrtx_plan_step; rrtx_plan = begin + steps until nothing is pending)
  struct Run {
    int stage = 0;   // 0 none, 1 RRT* iteration-kernel launches, 2 launches of the planner's main kernel
    std::chrono::steady_clock::time_point t0;
    double kms = 0.0, kms_main = -1.0;
    int64_t launches = 0, launches_main = 0, steps = 0, v2_done_it = 0;
    bool use_v2 = false, bit_wave = false;
    int v2_tpb = 0;
    int bit_grid = 0;   // BIT*, one wave per instance: waves per launch at most
    std::vector<Result> res;
    std::vector<int32_t> pending;   // BIT*: instances not finished yet (the device-side work queue of the next launch)
  } run;
  int32_t *bit_queue = nullptr, *bit_qhead = nullptr;   // BIT*: device copy of `pending`, queue head counter
  int bit_trip_bound = 20000;    // BIT*: trips of plan()'s loop per instance and launch (rrt_bitstar_wave.hip.h)
  Inst* d_inst0 = nullptr;       // device copy of host_inst (the staged start state of every instance)
  bool inst_dirty = true;        // host_inst changed since d_inst0 was written
  rppk::StatsAcc* d_acc = nullptr;
  // native RCCL gather of the result table (rrtx_rccl_*): communicator of this rank, world size, receive buffer
  void* rccl_comm = nullptr;
  int rccl_world = 0, rccl_rank = 0;
  DevBuf rccl_recv;
  int chunk_iters = 32768;       // iterations per launch of the other planner kernels
  int32_t* inst_map = nullptr;   // device: instance ids of a partial re-plan (overflow retry)
  // pose planners: where an instance's edge polylines live -- the handle's pool (slab = instance), or a larger pool
  // allocated for instances that outgrew it (slab = position in that re-plan)
  struct PoolLoc {
    double *px = nullptr, *py = nullptr, *pyaw = nullptr;
    int64_t cap = 0, slab = 0;
    // the instance's slab of column `col` (px, py or pyaw), from its point `off` on
    const double* at(const double* col, int64_t off = 0) const { return col + slab * cap + off; }
  };
  std::vector<PoolLoc> pool_loc;
  // the enlarged pools of the overflow re-plan (x4, x16): kept on the handle and used again by later rrtx_plan calls
  // when they are large enough (slabs >= instances to re-plan), so repeated plans do not grow device memory
  struct BigPool {
    DevBuf px, py, pyaw;
    int64_t cap = 0;
    int slabs = 0;
  } big[2];
  int32_t* pool_slot = nullptr;  // device copy of the slab numbers of a re-plan
  int64_t stats_retried = 0;
  int informed_eager = 0;        // rrt_07 kernel: 1 = collision-test every near candidate (reference order), 0 = cheapest first
  int v2_chunk_iters = 131072;  // iterations per launch of the RRT* iteration kernel (rrt_star_v2_body.inc)
  double* cbest = nullptr;  // informed RRT*: best path length so far per instance (device)
  std::vector<rppi::InformedArgs> iargs;   // informed RRT*: per-instance rotation C / c_min**2 (centre filled at plan time)
  std::vector<double> icmin;               // informed RRT*: per-instance c_min as handed in
  rppi::InformedArgs* d_iargs = nullptr;
  rppd::DubArgs da;         // RRT*-Dubins device arrays
  rppb::BitArgs ba;         // BIT* device arrays
  rppl::LqrArgs la;         // LQR-RRT* device arrays (edge endpoints, near-entry scratch)
  std::vector<rpp::BitCfg> bcfg;
  // path smoothing on the planned paths (rrtx_smooth_planned)
  double* sm_osz = nullptr;   // obstacle sizes as given (no robot radius), device: the fourth column of obs_buf
  double* sm_xy = nullptr;    // [inst][sm_stride][2]
  int32_t *sm_n = nullptr, *sm_status = nullptr;
  int32_t* sm_obs = nullptr;  // [inst][2]: the rows (base, count) each path is smoothed against
  int64_t sm_stride = 0;
  bool smoothed = false;
  int rs_cost = 0;            // RRTX_ALGO_RS: RRTX_RS_COST_* of the next plan (rrtx_set_rs_cost)
  // closed-loop stage on the planned trees (rrtx_track_planned, rrt_track.hip.h)
  struct Track {
    int32_t *cand = nullptr, *jobs = nullptr, *counters = nullptr;
    rppt::Record* rec = nullptr;
    rppt::Outcome* outc = nullptr;
    const double** pool = nullptr;
    double* slab = nullptr;
    DevBuf out;   // the winners' arrays: its size depends on the plan, so it alone of the tracking buffers is regrown
    int64_t* out_off = nullptr;
    int blocks = 0;
    bool valid = false;
    std::vector<rppt::Outcome> h_outc;
    std::vector<int64_t> h_off;
    double ms = 0.0;
  } tk;
  // the courses of the current plan, gathered into one CSR result (rrtx_gather_courses, course_gather.hip.h); the
  // buffers grow and never shrink
  struct Courses {
    DevBuf count, off, x, y, yaw, pool;
    bool valid = false, has_yaw = false;
    int which = 0, order = 0;
    int64_t n_points = 0;
    uint64_t generation = 0;   // completed gathers so far: what an rrtx_track_source of RRTX_SRC_PLANNER names
    std::vector<int64_t> h_off;
    double kernel_ms = 0.0;
  } cs;
  // the last rrtx_query_goals on the current plan and the courses gathered from it (goal_query.hip.h): buffers of their
  // own, so that the gathered courses of rrtx_gather_courses stay what they are; they grow and never shrink
  struct GoalQ {
    DevBuf goals, rec, scratch, count, off, x, y, yaw, pool;
    bool valid = false, gathered = false, has_yaw = false;
    int n_goals = 0, per_instance = 0, order = 0;
    double xy_th = 0.0, yaw_th = 0.0;
    int64_t n_points = 0;
    uint64_t generation = 0;   // completed queries so far
    std::vector<rppq::Record> h_rec;
    std::vector<int64_t> h_off;
    double solve_ms = 0.0, gather_ms = 0.0;
  } gq;
  // the last rrtx_track_goals on the current plan (goal_track.hip.h): buffers of its own, neither tk's nor gq's; they grow and
  // never shrink
  struct GoalTrack {
    DevBuf goals, count, cand_off, cand, job_query, rec, counters, win_query, slab, outc, out, arr_off, pool;
    bool valid = false, has_arrays = false;
    int n_goals = 0;
    int64_t n_cand = 0, n_steps = 0;
    std::vector<rppgt::Outcome> h_outc;
    std::vector<int64_t> h_cand_off, h_arr_off;
    double list_ms = 0.0, roll_ms = 0.0, store_ms = 0.0;
  } gt;
};

template <class T>
static int dalloc(rrtx_handle* h, T** p, size_t count) {
  void* q = nullptr;
  HIPCHK(h, hipMalloc(&q, count * sizeof(T)));
  h->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// Inputs of a plan are fixed from rrtx_plan_begin to the end of that plan: a re-plan inside it restarts instances from
// host_inst, and the BIT* table uploaded by rrtx_plan_begin points into the obstacle table.  The setters refuse meanwhile.
static int refuse_in_plan(rrtx_handle* h, const char* fn) {
  if (h->run.stage == 0) return RRTX_OK;
  h->err = std::string(fn) + ": a plan is in progress";
  return RRTX_E_STATE;
}

// The entry points that read the handle's obstacle table (path smoothing, goal queries) do not read the obstacle map
static int refuse_with_map(rrtx_handle* h, const char* fn) {
  if (!h->om.on) return RRTX_OK;
  h->err = std::string(fn) + ": the handle holds an obstacle map (rrtx_set_obstacle_map), which this call does not read";
  return RRTX_E_STATE;
}

// Device obstacle table of at least `rows` rows (contents are not kept: the caller uploads every row afterwards)
static int obs_reserve(rrtx_handle* h, int64_t rows) {
  if (rows <= h->obs_cap) return RRTX_OK;
  DevBuf fresh;
  if (int rc = h->reserve(fresh, sizeof(double) * 4 * (size_t)rows)) return rc;   // the handle keeps its current table and lists
  h->obs_buf = std::move(fresh);
  h->obs_cap = rows;
  h->c.ox = h->obs_buf.as<double>();
  h->c.oy = h->c.ox + rows;
  h->c.othr = h->c.ox + 2 * rows;
  h->sm_osz = h->obs_buf.as<double>() + 3 * rows;
  return RRTX_OK;
}

// Uploads `rows` obstacle rows (AoS x, y, size) as the SoA table ox / oy / othr (+ sizes for path smoothing) and keeps
// them in h->obst.  On failure the handle keeps its previous table and lists: the caller changes no instance.
static int obs_upload(rrtx_handle* h, const double* oxyr, int64_t rows) {
  HIPCHK(h, hipSetDevice(h->device));
  int rc = obs_reserve(h, rows);
  if (rc) return rc;
  std::vector<double> t(4 * (size_t)h->obs_cap, 0.0);
  for (int64_t k = 0; k < rows; k++) {
    t[k] = oxyr[3 * k];
    t[h->obs_cap + k] = oxyr[3 * k + 1];
    t[2 * h->obs_cap + k] = py_sq_host(oxyr[3 * k + 2] + h->p.robot_radius);  // (size+robot_radius)**2  rrt_04:1227
    t[3 * h->obs_cap + k] = oxyr[3 * k + 2];
  }
  HIPCHK(h, hipMemcpy(h->obs_buf.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
  h->obst.assign(oxyr, oxyr + 3 * (size_t)rows);
  return RRTX_OK;
}

// One timed launch on the handle's stream: `queue` queues the kernel; with copy_results every instance's Result comes back
// into run.res.  Waits for the launch and adds its time and count to the run.
template <class Queue>
static int timed_launch(rrtx_handle* h, bool copy_results, Queue&& queue) {
  rrtx_handle::Run& R = h->run;
  float ms = 0.f;
  int rc = h->timed(&ms, queue, [&]() -> int {
    if (copy_results)
      HIPCHK(h, hipMemcpyAsync(R.res.data(), h->c.results, sizeof(Result) * h->n_inst, hipMemcpyDeviceToHost, h->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  R.kms += ms;
  R.launches++;
  return RRTX_OK;
}

// ---- RRT* (rrt_04, search_until_max_iter): iteration-kernel launches ------------------------------------------------
// One pass of the latency-lean iteration kernel over `nblk` instances (c.inst_map selects them; nullptr = 0..nblk-1),
// in chunks of h->v2_chunk_iters iterations, workgroup shape tpb in {64, 128, 256}.
// The kernel's three shapes (rrt_star_v2.hip.h), widest first: threads per instance, near-candidate capacity (RRT2_NU), obstacle
// tile (RRT2_MAXOBS), the batch size above which the shape is chosen (8 / 16 workgroups per CU wanted resident) and the kernel.
struct V2Shape { int tpb, nu, max_obs, min_batch; void (*kernel)(Ctx, int); };
static const V2Shape V2_SHAPES[3] = {
    {rppk2::TPB, rppk2::NU, rppk2::MAX_OBS, 0, rppk2::rrt_star_kernel_v2},
    {rppk2s::TPB, rppk2s::NU, rppk2s::MAX_OBS, 1280, rppk2s::rrt_star_kernel_v2},
    {rppk2t::TPB, rppk2t::NU, rppk2t::MAX_OBS, 2560, rppk2t::rrt_star_kernel_v2}};
static const V2Shape& v2_shape(int tpb) {   // any other value: the 256-thread shape
  for (const V2Shape& s : V2_SHAPES)
    if (s.tpb == tpb) return s;
  return V2_SHAPES[0];
}
static int launch_rrt_star_v2_once(rrtx_handle* h, const Ctx& c, int nblk, int tpb) {
  const V2Shape& s = v2_shape(tpb);
  return timed_launch(h, false, [&] { hipLaunchKernelGGL(s.kernel, dim3(nblk), dim3(s.tpb), 0, h->stream, c, h->v2_chunk_iters); });
}
// The sample stream of `nblk` instances of `c` (c.inst_map selects them), from their staged start state: every sample of
// the plan into c.samp, the generators' end state into c.inst.  Timed with the plan's kernels, not counted as a launch.
static int launch_sample_stream(rrtx_handle* h, const Ctx& c, int nblk) {
  float ms = 0.f;
  int rc = h->timed(&ms, [&] { hipLaunchKernelGGL(rppss::rrt_sample_stream_kernel, dim3(nblk), dim3(64), 0, h->stream, c); });
  if (rc) return rc;
  h->run.kms += ms;
  return RRTX_OK;
}
static int launch_rrt_star_v2(rrtx_handle* h, const Ctx& c, int nblk, int tpb) {
  for (int64_t done_it = 0; done_it < c.max_iter; done_it += h->v2_chunk_iters) {
    int rc = launch_rrt_star_v2_once(h, c, nblk, tpb);
    if (rc) return rc;
  }
  return RRTX_OK;
}

// The knobs of the rrt_04 iteration kernel's one-wave shape, from the environment into the launch context
static void rrt_star_knobs(Ctx& c) {
  // rrt_04 kernel, one-wave shape: a streaming pass serves up to 1 + spec2 iterations (clamped to the kernel's RRT2_SPECK;
  // RRTX_SPEC2=0: one pass per iteration)
  c.spec2 = 8;
  if (const char* e = getenv("RRTX_SPEC2")) c.spec2 = atoi(e) > 0 ? atoi(e) : 0;
  // rrt_04 kernel, one-wave shape: near and nearest queries from the grid index (RRTX_GRID=0: the streaming pass only);
  // below grid_min nodes a pass streams (RRTX_GRID_MIN: test knob, 0 = from the first node)
  c.grid = c.ghead != nullptr;
  if (const char* e = getenv("RRTX_GRID")) c.grid = c.grid && atoi(e) != 0;
  c.grid_min = 4096;
  if (const char* e = getenv("RRTX_GRID_MIN")) c.grid_min = atoi(e) > 0 ? atoi(e) : 0;
  // rrt_04 kernel, one-wave shape: a cost propagation still running after prop_vec nodes continues one sibling chain per
  // lane (RRTX_PROP_VEC, < 0: one node per round trip throughout); RRTX_PROP_CAP: test knob, fewer pending chains in LDS
  c.prop_vec = 8;
  if (const char* e = getenv("RRTX_PROP_VEC")) c.prop_vec = atoi(e);
  c.prop_cap = 1 << 30;
  if (const char* e = getenv("RRTX_PROP_CAP")) c.prop_cap = atoi(e) > 0 ? atoi(e) : 0;
  // rrt_04 kernel, one-wave shape: the candidate edges of an iteration are tested against the obstacles that reach the
  // near ball of its new node only (RRTX_OBS_CULL=0: against every obstacle, in (edge, obstacle) pairs)
  c.obs_cull = 1;
  if (const char* e = getenv("RRTX_OBS_CULL")) c.obs_cull = atoi(e) != 0;
  // rrt_04 kernel, one-wave shape: a pass over the grid index gathers for all its centres together (RRTX_GRID_MERGE=0:
  // centre after centre, two round trips each)
  c.grid_merge = 1;
  if (const char* e = getenv("RRTX_GRID_MERGE")) c.grid_merge = atoi(e) != 0;
}

// Expected size of the largest near set of a plan, for a tree that fills the sampling square evenly:
// density * pi * r(n)^2 with r(n) of rrt_04:1329-1334 -> pi * min(ccd^2 ln n, n expand_dis^2) / area, largest at
// n = max_iter + 1; a Poisson tail (6 sigma + 8) on top.  Trees are not even (obstacles, unexplored corners), so this
// only steers the first choice of shape: an instance that still overflows is planned again on the next larger shape.
static int estimate_near_capacity(const rrtx_params& p) {
  const double n = (double)p.max_iter + 1.0;
  const double side = fabs(p.rand_max - p.rand_min);
  const double area = side * side > 1e-12 ? side * side : 1e-12;
  double a = p.connect_circle_dist * p.connect_circle_dist * log(n > 2.0 ? n : 2.0), b = n * p.expand_dis * p.expand_dis;
  const double lam = M_PI * (a < b ? a : b) / area;
  const double cap = lam + 6.0 * sqrt(lam) + 8.0;
  return cap > 1e6 ? 1000000 : (int)cap;
}

static void rccl_release(rrtx_handle* h);   // rrtx_api_rccl.inc
static void handle_register(const rrtx_handle* h);     // rrtx_api_courses.inc
static void handle_unregister(const rrtx_handle* h);

extern "C" {

int rrtx_abi_version(void) { return RRTX_ABI_VERSION; }

int rrtx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* rrtx_last_error(rrtx_handle* h) { return h ? h->err.c_str() : "null handle"; }

void rrtx_destroy(rrtx_handle* h) {
  if (!h) return;
  handle_unregister(h);
  hipSetDevice(h->device);
  rccl_release(h);
  for (void* q : h->allocs) hipFree(q);
  delete h;   // the DevBuf members, then the events and the stream
}

static inline bool is_dubins(int algo) { return algo == RRTX_ALGO_DUBINS || algo == RRTX_ALGO_RRT_DUBINS; }
// planners whose nodes are poses with a stored edge polyline (rrt_03 / rrt_05 / rrt_06)
static inline bool is_pose_tree(int algo) { return is_dubins(algo) || algo == RRTX_ALGO_RS; }

int rrtx_create(const rrtx_params* p, rrtx_handle** out) {
  if (!p || !out) return RRTX_E_INVALID;
  *out = nullptr;
  if (p->abi_version != RRTX_ABI_VERSION) return RRTX_E_INVALID;
  if (p->algo != RRTX_ALGO_RRT && p->algo != RRTX_ALGO_RRT_STAR && p->algo != RRTX_ALGO_INFORMED && p->algo != RRTX_ALGO_DUBINS && p->algo != RRTX_ALGO_BITSTAR && p->algo != RRTX_ALGO_RRT_DUBINS && p->algo != RRTX_ALGO_RS && p->algo != RRTX_ALGO_LQR_RRT_STAR) return RRTX_E_INVALID;
  if (p->algo == RRTX_ALGO_LQR_RRT_STAR && !(p->step_size > 0.0)) return RRTX_E_INVALID;
  if (p->algo == RRTX_ALGO_RS && (!(p->step_size > 0.0) || !(p->curvature > 0.0))) return RRTX_E_INVALID;
  if (p->n_instances < 1 || p->max_iter < 0 || !(p->path_resolution > 0.0) || !(p->expand_dis >= 0.0))
    return RRTX_E_INVALID;
  rrtx_handle* h = new rrtx_handle();
  int rc = h->open(p->device, "rrtx_create");
  if (rc == RRTX_E_NO_DEVICE) {   // no handle without a device: there is no message to read
    delete h;
    return rc;
  }
  h->p = *p;
  h->n_inst = p->n_instances;
  memset(&h->stats, 0, sizeof(h->stats));
  memset(&h->c, 0, sizeof(h->c));
  // Iterations per kernel launch.  A launch ends when its slowest instance does, so short chunks leave the chip
  // part idle at the end of every launch: 1024-iteration chunks cost the C2 batch 9 % (103 launches) against one launch,
  // 16384-iteration chunks (7 launches) still 1.9 % (18.47 vs 18.12 s, same box).  A plan of up to 131072 iterations
  // (32768 for the other kernels) is ONE launch now -- C2's 105000 iterations: 18 s of kernel time.
  if (const char* e = getenv("RRTX_CHUNK_ITERS")) {
    h->chunk_iters = atoi(e) > 0 ? atoi(e) : 32768;
    h->v2_chunk_iters = h->chunk_iters;
  }
  *out = h;  // returned even on failure, of open() or below, so the caller can read last_error, then destroy
  handle_register(h);
  if (rc) return rc;
  // node capacity: start + one node per iteration; padded so each wave's 512-node stride stays inside
  // (rrt_06: try_goal_path :1572-1582 can append a second node per iteration)
  const int64_t cap = (p->algo == RRTX_ALGO_RS ? 2 : 1) * (int64_t)p->max_iter + 2;
  h->stride = (cap + 511) / 512 * 512 + 2560;
  const size_t tot = (size_t)h->stride * h->n_inst;
  Ctx& c = h->c;
  if ((rc = dalloc(h, &c.inst, h->n_inst))) return rc;
  if ((rc = dalloc(h, &c.x, tot))) return rc;
  if ((rc = dalloc(h, &c.y, tot))) return rc;
  if ((rc = dalloc(h, &c.cost, tot))) return rc;
  if ((rc = dalloc(h, &c.parent, tot))) return rc;
  if ((rc = dalloc(h, &c.kid, tot))) return rc;   // {first child, next sibling, parent-edge length} per node
  if ((rc = dalloc(h, &c.prev_sib, tot))) return rc;
  if ((rc = dalloc(h, &c.hits, tot))) return rc;
  if ((rc = dalloc(h, &c.stack, tot))) return rc;
  if (p->algo == RRTX_ALGO_INFORMED) {
    // float mirror of the coordinates for the prefiltered streaming passes of the rrt_07 kernel (rrt_informed.hip.h)
    if ((rc = dalloc(h, &c.xf, tot))) return rc;
    if ((rc = dalloc(h, &c.yf, tot))) return rc;
  }
  if (p->algo == RRTX_ALGO_RRT_STAR && p->search_until_max_iter) {
    c.has_elen = 1;   // kid[].elen: cached parent-edge lengths (cost propagation)
    if ((rc = dalloc(h, &c.xq, tot))) return rc;     // 16-bit mirror (first stage of the streaming pass)
    if ((rc = dalloc(h, &c.node, tot))) return rc;   // one 64-byte line per node: the iteration kernel's working format
    // the sample stream (rrt_samples.hip.h): 16 bytes per instance and iteration
    if ((rc = dalloc(h, &c.samp, 2 * (size_t)(p->max_iter > 0 ? p->max_iter : 1) * h->n_inst))) return rc;
    // grid index of the mirror (DESIGN 5.1 "grid index"): cells sized for about 6 nodes each at the final tree size,
    // 512 grid steps at the least (128 x 128 cells); an overflow block per 128 nodes of capacity
    int gsh = 9;
    while (gsh < 15 && (int64_t)(65536 >> gsh) * (65536 >> gsh) * 6 > cap) gsh++;
    c.gsh = gsh;
    c.gn = 65536 >> gsh;
    c.gcells = c.gn * c.gn;
    c.gpool_blocks = (int32_t)(cap / 128 + 16);
    const size_t gc = (size_t)c.gcells * h->n_inst;
    if ((rc = dalloc(h, &c.ghead, gc))) return rc;
    if ((rc = dalloc(h, &c.gent, gc * rppk::GRID_CAP0))) return rc;
    if ((rc = dalloc(h, &c.gpool, (size_t)c.gpool_blocks * rppk::GRID_CAP1 * h->n_inst))) return rc;
  }
  if (p->algo == RRTX_ALGO_INFORMED)
    if ((rc = dalloc(h, &c.xq, tot))) return rc;     // 16-bit mirror: the one pass per iteration of the rrt_07 kernel
  if ((rc = dalloc(h, &c.results, h->n_inst))) return rc;
  c.path_cap = (int32_t)(cap + 1 < 8192 ? cap + 1 : 8192);
  if (p->algo == RRTX_ALGO_LQR_RRT_STAR) c.path_cap = 4096;   // paths are edge polylines (~20 points per edge)
  if ((rc = dalloc(h, &c.path_xy, (size_t)h->n_inst * c.path_cap * 2))) return rc;
  double* dr2;
  if ((rc = obs_reserve(h, rppk::MAX_OBS))) return rc;   // every instance starts on the empty shared list
  if ((rc = dalloc(h, &dr2, (size_t)cap + 2))) return rc;
  c.r2tab = dr2;
  c.stride = h->stride;
  c.algo = p->algo;
  c.sampler = p->sampler;
  c.goal_sample_rate = p->goal_sample_rate;
  c.max_iter = p->max_iter;
  c.has_play = p->has_play_area;
  c.until_max = p->search_until_max_iter;
  c.rand_min = p->rand_min;
  c.rand_max = p->rand_max;
  c.expand_dis = p->expand_dis;
  c.res = p->path_resolution;
  for (int i = 0; i < 4; i++) c.play_area[i] = p->play_area[i];
  c.trace_inst = -1;
  // find_near_nodes radius schedule (rrt_04:1329-1334, :1337): r(nnode)**2 with this host's libm,
  // exactly the expression the reference evaluates per iteration; it depends on nnode only.
  std::vector<double> r2((size_t)cap + 2, 0.0);
  for (int64_t nn = 1; nn < cap + 2; nn++) {
    double r;
    if (p->algo == RRTX_ALGO_INFORMED) {
      r = 50.0 * libm_sqrt(libm_log((double)nn) / (double)nn);   // rrt_07:1139, indexed by len(node_list), no cap
    } else {
      r = p->connect_circle_dist * libm_sqrt(libm_log((double)nn) / (double)nn);
      if (p->expand_dis < r) r = p->expand_dis;
    }
    r2[nn] = py_sq_host(r);
  }
  if (p->algo == RRTX_ALGO_INFORMED) {
    if ((rc = dalloc(h, &h->cbest, h->n_inst))) return rc;
    if ((rc = dalloc(h, &h->d_iargs, h->n_inst))) return rc;
    h->iargs.resize(h->n_inst);
    h->icmin.assign(h->n_inst, p->informed_c_min);
    for (int i = 0; i < h->n_inst; i++) {
      for (int k = 0; k < 4; k++) h->iargs[i].rot[k] = p->informed_rot[k];
      h->iargs[i].c_min2 = py_sq_host(p->informed_c_min);   // c_min ** 2 rrt_07:1147
    }
  }
  memset(&h->ba, 0, sizeof(h->ba));
  if (p->algo == RRTX_ALGO_BITSTAR) {
    rppb::BitArgs& b = h->ba;
    if ((rc = dalloc(h, &b.cfg, h->n_inst))) return rc;
    if ((rc = dalloc(h, &b.dslab, (size_t)rppb::DSLAB * h->n_inst))) return rc;
    if ((rc = dalloc(h, &b.islab, (size_t)rppb::ISLAB * h->n_inst))) return rc;
    if ((rc = dalloc(h, &b.out_i, (size_t)8 * h->n_inst))) return rc;
    if ((rc = dalloc(h, &b.out_g, h->n_inst))) return rc;
    b.trace_inst = -1;
    h->bcfg.resize(h->n_inst);
    for (int i = 0; i < h->n_inst; i++) {
      rpp::BitCfg& c2 = h->bcfg[i];
      memset(&c2, 0, sizeof(c2));
      c2.start[0] = p->start[0]; c2.start[1] = p->start[1];
      c2.goal[0] = p->goal[0]; c2.goal[1] = p->goal[1];
      c2.rand_min = p->rand_min; c2.rand_max = p->rand_max;
      for (int k = 0; k < 4; k++) c2.rot[k] = p->informed_rot[k];
      c2.c_min = p->informed_c_min;
      c2.c_min2 = py_sq_host(p->informed_c_min);
      c2.num_cells = std::ceil((p->rand_max - p->rand_min) / 0.01);   // RTree num_cells (rrt_08:42-44, :165-168)
      c2.max_iter = p->max_iter;
    }
  }
  memset(&h->la, 0, sizeof(h->la));
  if (p->algo == RRTX_ALGO_LQR_RRT_STAR) {
    // node capacity max_iter + 1 (one node per iteration at most, rrt_09:1133); the edge record of a node is its four
    // endpoints, from which the polyline is regenerated (rpp_lqr.h)
    rppl::LqrArgs& a = h->la;
    if ((rc = dalloc(h, &a.ef, 4 * tot))) return rc;
    if ((rc = dalloc(h, &a.nl, tot))) return rc;
    if ((rc = dalloc(h, &a.dscr, tot))) return rc;
    if ((rc = dalloc(h, &a.cex, tot))) return rc;
    if ((rc = dalloc(h, &a.cey, tot))) return rc;
    if ((rc = dalloc(h, &a.clen, tot))) return rc;
    if ((rc = dalloc(h, &a.cflag, tot))) return rc;
    if ((rc = dalloc(h, &a.moved, tot))) return rc;
    a.step = p->step_size;
    a.nt = rpp::lqr_nt(p->step_size);
    a.goal_xy_th = p->goal_xy_th;
  }
  memset(&h->da, 0, sizeof(h->da));
  if (is_pose_tree(p->algo)) {
    rppd::DubArgs& d = h->da;
    d.plain = p->algo == RRTX_ALGO_RRT_DUBINS;
    // polyline points per instance (edges replaced by rewire stay allocated; rrt_06 edges run all the way to the
    // sample at step_size spacing and are longer)
    int64_t ppn = p->algo == RRTX_ALGO_RS ? 160 : 128;   // polyline points per node, on average
    if (const char* e = getenv("RRTX_POOL_POINTS_PER_NODE"))   // test knob: a small pool exercises the re-plan below
      if (atoi(e) > 0) ppn = atoi(e);
    d.pool_cap = ppn * cap + 8192;
    if ((rc = dalloc(h, &d.yaw, tot))) return rc;
    if ((rc = dalloc(h, &d.poff, tot))) return rc;
    if ((rc = dalloc(h, &d.plen, tot))) return rc;
    if ((rc = dalloc(h, &d.pool_x, (size_t)d.pool_cap * h->n_inst))) return rc;
    if ((rc = dalloc(h, &d.pool_y, (size_t)d.pool_cap * h->n_inst))) return rc;
    if ((rc = dalloc(h, &d.pool_used, h->n_inst))) return rc;
    d.curvature = p->curvature;
    d.goal_yaw_th = p->goal_yaw_th;
    d.goal_xy_th = p->goal_xy_th;
  }
  if (p->algo == RRTX_ALGO_RS) {
    rppd::DubArgs& d = h->da;
    d.step_size = p->step_size;
    if ((rc = dalloc(h, &d.pool_yaw, (size_t)d.pool_cap * h->n_inst))) return rc;
    if ((rc = dalloc(h, &d.dscr, tot))) return rc;
  }
  if (is_dubins(p->algo)) {
    rppd::DubArgs& d = h->da;
    if ((rc = dalloc(h, &d.spx, (size_t)rppd::PMAX * h->n_inst))) return rc;
    if ((rc = dalloc(h, &d.spy, (size_t)rppd::PMAX * h->n_inst))) return rc;
    if ((rc = dalloc(h, &d.plans, (size_t)rppd::NUD * h->n_inst))) return rc;
    if ((rc = dalloc(h, &d.rawslot, tot))) return rc;
  }
  HIPCHK(h, hipMemcpy(dr2, r2.data(), r2.size() * sizeof(double), hipMemcpyHostToDevice));
  // default per-instance state: ctor start/goal, RNG seeded with the instance number
  h->host_inst.resize(h->n_inst);
  for (int i = 0; i < h->n_inst; i++) {
    Inst& I = h->host_inst[i];
    memset(&I, 0, sizeof(I));
    rpp::mt_seed_u64(&I.rng, (uint64_t)i);
    for (int k = 0; k < 3; k++) {
      I.start[k] = p->start[k];
      I.goal[k] = p->goal[k];
    }
  }
  return RRTX_OK;
}

int rrtx_set_obstacles(rrtx_handle* h, const double* oxyr, int32_t m) {
  if (!h || m < 0 || (m > 0 && !oxyr)) return RRTX_E_INVALID;
  if (int rc = refuse_in_plan(h, "rrtx_set_obstacles")) return rc;
  if (m > rppk::MAX_OBS) {
    h->err = "more than 256 obstacles";
    return RRTX_E_INVALID;
  }
  if (h->p.algo == RRTX_ALGO_RS && m > rppr::MAX_OBS) {
    h->err = "RRTX_ALGO_RS: more than 64 obstacles";
    return RRTX_E_INVALID;
  }
  // the shared list: every instance owns rows 0 .. m-1
  int rc = obs_upload(h, oxyr, m);
  if (rc) return rc;
  for (Inst& I : h->host_inst)
    if (I.obs_base != 0 || I.obs_m != m) {
      I.obs_base = 0;
      I.obs_m = m;
      h->inst_dirty = true;
    }
  h->m_max = m;
  h->om.on = false;   // back on the tile
  return RRTX_OK;
}

int rrtx_set_instance_obstacles(rrtx_handle* h, const int32_t* offsets, const double* oxyr) {
  if (!h) return RRTX_E_INVALID;
  if (int rc = refuse_in_plan(h, "rrtx_set_instance_obstacles")) return rc;
  if (!offsets) {
    h->err = "rrtx_set_instance_obstacles: offsets is NULL";
    return RRTX_E_INVALID;
  }
  const int B = h->n_inst;
  const int lim = h->p.algo == RRTX_ALGO_RS ? rppr::MAX_OBS : rppk::MAX_OBS;
  char msg[160];
  if (offsets[0] != 0) {
    snprintf(msg, sizeof(msg), "rrtx_set_instance_obstacles: instance 0: offsets[0] = %d, expected 0", offsets[0]);
    h->err = msg;
    return RRTX_E_INVALID;
  }
  int m_max = 0;
  for (int i = 0; i < B; i++) {
    const int64_t cnt = (int64_t)offsets[i + 1] - offsets[i];
    if (cnt < 0) {
      snprintf(msg, sizeof(msg), "rrtx_set_instance_obstacles: instance %d: offsets decrease (%d -> %d)", i, offsets[i],
               offsets[i + 1]);
      h->err = msg;
      return RRTX_E_INVALID;
    }
    if (cnt > lim) {
      snprintf(msg, sizeof(msg), "rrtx_set_instance_obstacles: instance %d: %lld obstacles, more than %d%s", i,
               (long long)cnt, lim, lim == rppk::MAX_OBS ? "" : " (RRTX_ALGO_RS)");
      h->err = msg;
      return RRTX_E_INVALID;
    }
    if (cnt > m_max) m_max = (int)cnt;
  }
  const int64_t total = offsets[B];
  if (total > 0 && !oxyr) {
    snprintf(msg, sizeof(msg), "rrtx_set_instance_obstacles: oxyr is NULL, %lld rows expected", (long long)total);
    h->err = msg;
    return RRTX_E_INVALID;
  }
  int rc = obs_upload(h, oxyr, total);
  if (rc) return rc;
  for (int i = 0; i < B; i++) {
    Inst& I = h->host_inst[i];
    I.obs_base = offsets[i];
    I.obs_m = offsets[i + 1] - offsets[i];
  }
  h->inst_dirty = true;
  h->m_max = m_max;
  h->om.on = false;   // back on the tile
  return RRTX_OK;
}

int rrtx_set_rng_state(rrtx_handle* h, int32_t instance, const uint32_t* mt624, int32_t pos) {
  if (!h || !mt624 || instance < 0 || instance >= h->n_inst || pos < 0 || pos > 624) return RRTX_E_INVALID;
  if (int rc = refuse_in_plan(h, "rrtx_set_rng_state")) return rc;
  h->inst_dirty = true;
  memcpy(h->host_inst[instance].rng.mt, mt624, 624 * 4);
  h->host_inst[instance].rng.pos = pos;
  return RRTX_OK;
}

int rrtx_get_rng_state(rrtx_handle* h, int32_t instance, uint32_t* mt624, int32_t* pos) {
  if (!h || !mt624 || !pos || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (h->planned) {
    HIPCHK(h, hipSetDevice(h->device));
    rpp::MT r;
    HIPCHK(h, hipMemcpy(&r, &h->c.inst[instance].rng, sizeof(r), hipMemcpyDeviceToHost));
    memcpy(mt624, r.mt, 624 * 4);
    *pos = r.pos;
  } else {
    memcpy(mt624, h->host_inst[instance].rng.mt, 624 * 4);
    *pos = h->host_inst[instance].rng.pos;
  }
  return RRTX_OK;
}

int rrtx_seed_instances(rrtx_handle* h, int32_t first, int32_t count, const uint64_t* seeds) {
  if (!h || !seeds || first < 0 || count < 0 || first + count > h->n_inst) return RRTX_E_INVALID;
  if (int rc = refuse_in_plan(h, "rrtx_seed_instances")) return rc;
  h->inst_dirty = true;
  for (int i = 0; i < count; i++) rpp::mt_seed_u64(&h->host_inst[first + i].rng, seeds[i]);
  return RRTX_OK;
}

int rrtx_set_instance(rrtx_handle* h, int32_t instance, const double* start3, const double* goal3) {
  if (!h || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (int rc = refuse_in_plan(h, "rrtx_set_instance")) return rc;
  h->inst_dirty = true;
  Inst& I = h->host_inst[instance];
  if (start3) {
    I.start[0] = start3[0];
    I.start[1] = start3[1];
    if (is_pose_tree(h->p.algo)) I.start[2] = start3[2];   // yaw (rrt_05:1406, rrt_06:1518)
    if (h->p.algo == RRTX_ALGO_BITSTAR) {
      h->bcfg[instance].start[0] = start3[0];
      h->bcfg[instance].start[1] = start3[1];
    }
  }
  if (goal3) {
    I.goal[0] = goal3[0];
    I.goal[1] = goal3[1];
    if (is_pose_tree(h->p.algo)) I.goal[2] = goal3[2];
    if (h->p.algo == RRTX_ALGO_BITSTAR) {
      h->bcfg[instance].goal[0] = goal3[0];
      h->bcfg[instance].goal[1] = goal3[1];
    }
  }
  return RRTX_OK;
}

int rrtx_set_instance_rotation(rrtx_handle* h, int32_t instance, const double* rot4, double c_min) {
  if (!h || !rot4 || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (int rc = refuse_in_plan(h, "rrtx_set_instance_rotation")) return rc;
  if (h->p.algo == RRTX_ALGO_INFORMED) {
    for (int k = 0; k < 4; k++) h->iargs[instance].rot[k] = rot4[k];
    h->iargs[instance].c_min2 = py_sq_host(c_min);   // c_min ** 2 rrt_07:1147
    h->icmin[instance] = c_min;
    return RRTX_OK;
  }
  if (h->p.algo != RRTX_ALGO_BITSTAR) return RRTX_E_STATE;
  rpp::BitCfg& c2 = h->bcfg[instance];
  for (int k = 0; k < 4; k++) c2.rot[k] = rot4[k];
  c2.c_min = c_min;
  c2.c_min2 = py_sq_host(c_min);
  return RRTX_OK;
}

int rrtx_enable_trace(rrtx_handle* h, int32_t instance) {
  if (!h || instance < -1 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (int rc = refuse_in_plan(h, "rrtx_enable_trace")) return rc;
  h->trace_inst = instance;
  if (instance >= 0 && !h->c.tr_rx) {
    int rc;
    const size_t n = (size_t)h->p.max_iter + 1;
    if ((rc = dalloc(h, &h->c.tr_rx, n))) return rc;
    if ((rc = dalloc(h, &h->c.tr_ry, n))) return rc;
    if ((rc = dalloc(h, &h->c.tr_near, n))) return rc;
    if ((rc = dalloc(h, &h->c.tr_nn, n))) return rc;
    if ((rc = dalloc(h, &h->c.tr_kind, n))) return rc;
    HIPCHK(h, hipMemset(h->c.tr_kind, 0, sizeof(int32_t) * n));
  }
  h->c.trace_inst = instance;
  return RRTX_OK;
}

// ---- one plan: rrtx_plan_begin, rrtx_plan_step, plan_finish ---------------------------------------------------------
// Every tree of `nblk` instances of `c` (c.inst_map selects them; nullptr = 0..nblk-1) back to its root node, from the
// instance's record in c.inst; waits for it.
static int init_trees(rrtx_handle* h, const Ctx& c, int nblk) {
  hipLaunchKernelGGL(rppk::rrt_init_kernel, dim3(64, nblk), dim3(256), 0, h->stream, c);
  hipLaunchKernelGGL(rppk::rrt_root_kernel, dim3((nblk + 63) / 64), dim3(64), 0, h->stream, c, nblk);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return RRTX_OK;
}

// Queues one launch of the planner's main kernel (not BIT*'s) over `nblk` instances of `c`, h->chunk_iters iterations
// each at most.  `da`: the pose planners' arrays and polyline pool (a re-plan hands in its larger pool); informed RRT*
// runs on the 2048-slot shape when `informed_large`, else on the product shape.
static void queue_main_kernel(rrtx_handle* h, const Ctx& c, int nblk, const rppd::DubArgs& da, bool informed_large) {
  if (c.algo == RRTX_ALGO_INFORMED && !informed_large)
    hipLaunchKernelGGL((rppi::rrt_informed_kernel<rppi::NUI_SMALL, 4>), dim3(nblk), dim3(rppi::TPB), 0, h->stream, c,
                       h->d_iargs, h->cbest, h->chunk_iters, h->informed_eager);
  else if (c.algo == RRTX_ALGO_INFORMED)
    hipLaunchKernelGGL((rppi::rrt_informed_kernel<rppi::NUI_LARGE, 1>), dim3(nblk), dim3(rppi::TPB), 0, h->stream, c,
                       h->d_iargs, h->cbest, h->chunk_iters, h->informed_eager);
  else if (is_dubins(c.algo))
    hipLaunchKernelGGL(rppd::rrt_dubins_kernel, dim3(nblk), dim3(rppd::TPB), 0, h->stream, c, da, h->chunk_iters);
  else if (c.algo == RRTX_ALGO_RS && h->om.on)
    hipLaunchKernelGGL(rppr::rrt_rs_map_kernel, dim3(nblk), dim3(rppr::TPB), 0, h->stream, c, da, h->chunk_iters, h->om.grid.map());
  else if (c.algo == RRTX_ALGO_RS)
    hipLaunchKernelGGL(rppr::rrt_rs_kernel, dim3(nblk), dim3(rppr::TPB), 0, h->stream, c, da, h->chunk_iters);
  else if (c.algo == RRTX_ALGO_LQR_RRT_STAR)
    hipLaunchKernelGGL(rppl::rrt_lqr_kernel, dim3(nblk), dim3(rppl::TPB), 0, h->stream, c, h->la, h->chunk_iters);
  else if (h->om.on)
    hipLaunchKernelGGL(rppk::rrt_plan_map_kernel, dim3(nblk), dim3(rppk::TPB), 0, h->stream, c, h->chunk_iters,
                       rppk::ObsMap{h->om.grid.items.as<const rppo::Item>(), h->om.grid.cell_start.as<const int32_t>(), h->om.grid.g,
                                    h->om.grid.g.nx * h->om.grid.g.ny, h->om.tile});
  else
    hipLaunchKernelGGL(rppk::rrt_plan_kernel, dim3(nblk), dim3(rppk::TPB), 0, h->stream, c, h->chunk_iters);
}

// Plans the instances `ids` again, from their staged start state, after the main kernel left them with a condition that
// a larger table or another kernel resolves (plan_finish).  `reset(i)` queues the planner's own reset of instance i;
// `prelude(cr, nr)` runs before the main kernel, on the Ctx of the re-plan (its workgroup k plans ids[k]); the main kernel
// (queue_main_kernel with `da`, `informed_large`) is launched until every id is RRTX_ST_DONE.  `label` names the re-plan
// in the error of its guard.  Either hook may be empty.
static int replan(rrtx_handle* h, const std::vector<int32_t>& ids, const char* label, const rppd::DubArgs& da,
                  bool informed_large, const std::function<int(int32_t)>& reset,
                  const std::function<int(const Ctx&, int)>& prelude) {
  const int nr = (int)ids.size();
  int rc;
  if (!h->inst_map && (rc = dalloc(h, &h->inst_map, h->n_inst))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->inst_map, ids.data(), sizeof(int32_t) * nr, hipMemcpyHostToDevice, h->stream));
  for (int32_t i : ids) {
    HIPCHK(h, hipMemcpyAsync(h->c.inst + i, &h->host_inst[i], sizeof(Inst), hipMemcpyHostToDevice, h->stream));
    if (reset && (rc = reset(i))) return rc;
  }
  Ctx cr = h->c;
  cr.inst_map = h->inst_map;
  if ((rc = init_trees(h, cr, nr))) return rc;   // also the end of the host -> device copies above
  if (prelude && (rc = prelude(cr, nr))) return rc;
  for (int64_t guard = 0;; guard++) {
    if ((rc = timed_launch(h, true, [&] { queue_main_kernel(h, cr, nr, da, informed_large); }))) return rc;
    bool all = true;
    for (int32_t i : ids)
      if (!(h->run.res[i].status & RRTX_ST_DONE)) all = false;
    if (all) break;
    if (guard > (int64_t)h->p.max_iter / h->chunk_iters + 8) {
      h->err = std::string("planner kernel did not converge to DONE (") + label + ")";
      return RRTX_E_STATE;
    }
  }
  h->stats_retried += nr;
  return RRTX_OK;
}

static int plan_finish(rrtx_handle* h);

int rrtx_plan_begin(rrtx_handle* h) {
  if (!h) return RRTX_E_INVALID;
  h->run = rrtx_handle::Run();
  rrtx_handle::Run& R = h->run;
  R.t0 = std::chrono::steady_clock::now();
  h->planned = false;
  h->smoothed = false;     // rrtx_get_smoothed_path: the previous plan's smoothed paths are not this plan's
  h->tk.valid = false;     // the same for the tracked trajectories
  h->cs.valid = false;     // and for the gathered courses (rrtx_gather_courses)
  h->gq.valid = false;     // and for the goal queries asked of the previous plan's trees (rrtx_query_goals)
  h->gt.valid = false;     // and for the closed-loop answers to many goals (rrtx_track_goals)
  h->traced_inst = -1;     // rrtx_get_trace: nothing recorded until this plan completes
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());   // uploads made through the null stream (obstacles, tables) are complete
  Ctx& c = h->c;
  const int B = h->n_inst;
  h->stats_retried = 0;
  // f32-mirror margin of the rrt_07 kernel = 2^-20 * the largest coordinate magnitude a node or sample is assumed to have
  // (see scan_nearest_f32); its informed samples are not clipped to the sampling square, so twice that (the kernel checks
  // and falls back)
  {
    double mag = fabs(c.rand_min) > fabs(c.rand_max) ? fabs(c.rand_min) : fabs(c.rand_max);
    for (int i = 0; i < B; i++) {
      const Inst& I = h->host_inst[i];
      const double v[4] = {I.start[0], I.start[1], I.goal[0], I.goal[1]};
      for (double q : v)
        if (fabs(q) > mag) mag = fabs(q);
    }
    if (c.algo == RRTX_ALGO_INFORMED) mag *= 2.0;
    c.f32_m = ldexp(mag > 1.0 ? mag : 1.0, -20);
    // 16-bit mirror: the square [lo, hi]^2 that holds every node and sample (sampling square, starts, goals; nodes are
    // convex combinations of those).  Quantisation error <= step/2 per coordinate -> a point moves by <= step/sqrt(2);
    // node and query are both on the grid -> distance error < sqrt(2) steps; the arithmetic is exact (integer).
    double lo = c.rand_min < c.rand_max ? c.rand_min : c.rand_max, hi = c.rand_min < c.rand_max ? c.rand_max : c.rand_min;
    for (int i = 0; i < B; i++) {
      const Inst& I = h->host_inst[i];
      const double v[4] = {I.start[0], I.start[1], I.goal[0], I.goal[1]};
      for (double q : v) {
        if (q < lo) lo = q;
        if (q > hi) hi = q;
      }
    }
    if (c.algo == RRTX_ALGO_INFORMED) {
      // rrt_07's informed samples are not clipped to the sampling square (the ellipse of :1145-1159 may reach past it) and
      // a node may step expand_dis beyond its sample: an eighth of the range on every side.  A node that still leaves the
      // grid switches its instance to the f32 / f64 passes (rrt_informed.hip.h)
      double frac = 0.125;
      if (const char* e = getenv("RRTX_Q16_PAD")) frac = atof(e);   // test knob: a negative margin makes nodes leave the grid
      const double pad = frac * (hi - lo > 1e-9 ? hi - lo : 1.0) + (frac >= 0.0 ? fabs(c.expand_dis) : 0.0);
      lo -= pad;
      hi += pad;
    }
    const double range = hi - lo > 1e-9 ? hi - lo : 1.0;
    c.q_lo = lo;
    c.q_step = range / 65535.0;
    c.q_inv = 65535.0 / range;
    c.q_m = 1.4375 * c.q_step;   // node AND query rounded to the grid: sqrt(2) steps (scan2q)
  }
  if (const char* e = getenv("RRTX_F32"))
    if (atoi(e) == 0 && c.algo == RRTX_ALGO_INFORMED) c.xf = c.yf = nullptr;   // informed kernel: f64 passes only
  if (const char* e = getenv("RRTX_Q16"))
    if (atoi(e) == 0 && c.algo == RRTX_ALGO_INFORMED) c.xq = nullptr;   // informed kernel: no 16-bit first stage
  rrt_star_knobs(c);
  // The staged per-instance start state (RNG, start / goal) lives on the device too: uploaded when the host changed it,
  // copied device -> device at every plan (2.7 KB per instance: 44 MB of pageable-memory upload per plan of 16 384 instances)
  if (!h->d_inst0) {
    int rc2 = dalloc(h, &h->d_inst0, B);
    if (rc2) return rc2;
    h->inst_dirty = true;
  }
  if (h->inst_dirty) {
    HIPCHK(h, hipMemcpyAsync(h->d_inst0, h->host_inst.data(), sizeof(Inst) * B, hipMemcpyHostToDevice, h->stream));
    h->inst_dirty = false;
  }
  HIPCHK(h, hipMemcpyAsync(c.inst, h->d_inst0, sizeof(Inst) * B, hipMemcpyDeviceToDevice, h->stream));
  int rc = init_trees(h, c, B);
  if (rc) return rc;
  R.res.assign(B, Result());
  if (c.algo == RRTX_ALGO_BITSTAR) {
    // BIT*: one launch, one lane per instance (rrt_bitstar.hip.h); obstacle thresholds are size ** 2 (rrt_08:381)
    for (int i = 0; i < B; i++) {
      const Inst& I = h->host_inst[i];
      h->bcfg[i].m = I.obs_m;
      h->bcfg[i].ox = c.ox + I.obs_base;
      h->bcfg[i].oy = c.oy + I.obs_base;
      h->bcfg[i].othr = c.othr + I.obs_base;
    }
    HIPCHK(h, hipMemcpyAsync(h->ba.cfg, h->bcfg.data(), sizeof(rpp::BitCfg) * B, hipMemcpyHostToDevice, h->stream));
    if (h->trace_inst >= 0 && !h->ba.tr_a) {
      if ((rc = dalloc(h, &h->ba.tr_a, 1 << 16))) return rc;
      if ((rc = dalloc(h, &h->ba.tr_b, 1 << 16))) return rc;
      h->ba.tr_cap = 1 << 16;
    }
    h->ba.trace_inst = h->trace_inst;
    // one wave per instance when the per-vertex state fits LDS (rrt_bitstar_wave.hip.h); else one lane per instance
    const char* bk = getenv("RRTX_BITSTAR");
    R.bit_wave = h->m_max <= rppb::OB && c.max_iter + 2 <= rppb::VL && !(bk && !strcmp(bk, "lane"));
    // as many waves as the chip keeps resident (LDS: 9 workgroups per CU), never more than there are instances
    R.bit_grid = h->n_cu * 9;
    if (const char* e = getenv("RRTX_BITSTAR_GRID")) R.bit_grid = atoi(e) > 0 ? atoi(e) : R.bit_grid;
    if (!h->bit_queue) {
      if ((rc = dalloc(h, &h->bit_queue, B))) return rc;
      if ((rc = dalloc(h, &h->bit_qhead, 1))) return rc;
      if ((rc = dalloc(h, &h->ba.save_i, (size_t)8 * B))) return rc;
    }
    if (const char* e = getenv("RRTX_BITSTAR_TRIPS")) h->bit_trip_bound = atoi(e) > 0 ? atoi(e) : 20000;
    R.pending.resize(B);
    for (int i = 0; i < B; i++) R.pending[i] = i;
    // Queue order = longest expected run first: BIT* run times have a heavy tail (p99 = 8 x the mean) and grow as start and
    // goal get closer (a small informed set is resampled densely: correlation -0.36 with the distance over 400 instances of
    // the C4 generator), so the instances most likely to be the last ones running start first.  Results do not depend on it.
    if (!getenv("RRTX_BITSTAR_FIFO"))
      std::stable_sort(R.pending.begin(), R.pending.end(),
                       [&](int32_t a, int32_t b) { return h->bcfg[a].c_min < h->bcfg[b].c_min; });
  }
  // RRT* with search_until_max_iter: the latency-lean iteration kernel runs every iteration; the general kernel
  // below then only performs the final goal search (rrt_04:1080-1084).  RRTX_KERNEL=v1 forces the general kernel.
  const char* kv = getenv("RRTX_KERNEL");
  // With an obstacle map the map variant of the general kernel runs every iteration: no iteration kernel, no shape retry.
  R.use_v2 = c.algo == RRTX_ALGO_RRT_STAR && c.until_max && !(kv && !strcmp(kv, "v1")) && !h->om.on;
  if (R.use_v2) {
    // workgroup shape: fewer threads per instance once more instances want to be resident (8 / 16 workgroups per CU),
    // as long as the shape's obstacle tile and near-candidate capacity fit the problem
    const int need_nu = estimate_near_capacity(h->p);
    int tpb = V2_SHAPES[0].tpb;
    const int m = h->m_max;   // every instance's list must fit the shape's obstacle tile
    for (const V2Shape& s : V2_SHAPES)
      if (B > s.min_batch && m <= s.max_obs && need_nu <= s.nu) tpb = s.tpb;
    if (const char* e = getenv("RRTX_TPB")) {
      const V2Shape& s = v2_shape(atoi(e));
      tpb = m <= s.max_obs ? s.tpb : V2_SHAPES[0].tpb;
    }
    R.v2_tpb = tpb;
  }
  if (c.algo == RRTX_ALGO_INFORMED) {
    std::vector<double> inf(B, INFINITY);
    HIPCHK(h, hipMemcpyAsync(h->cbest, inf.data(), sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // `inf` is a local
  }
  // on the handle's own stream: it is a non-blocking stream, work queued on the null stream is not ordered with it
  if (is_pose_tree(c.algo)) {
    HIPCHK(h, hipMemsetAsync(h->da.pool_used, 0, sizeof(int64_t) * B, h->stream));
    h->pool_loc.assign(B, rrtx_handle::PoolLoc());
    for (int i = 0; i < B; i++) {
      rrtx_handle::PoolLoc& pl = h->pool_loc[i];
      pl.px = h->da.pool_x; pl.py = h->da.pool_y; pl.pyaw = h->da.pool_yaw;
      pl.cap = h->da.pool_cap; pl.slab = i;
    }
    h->da.pool_slot = nullptr;
  }
  if (const char* e = getenv("RRTX_RS_EAGER")) h->da.eager = atoi(e) != 0;
  h->da.rs_cost = h->rs_cost;
  if (const char* e = getenv("RRTX_INFORMED_EAGER")) h->informed_eager = atoi(e) != 0;   // rrt_07: test every near candidate like the reference
  if (const char* e = getenv("RRTX_INFORMED_EXACT_SEG"))   // rrt_07 test knob: no tolerance bands -- every verdict from the exact segment form, every candidate list from the exact **2 form
    h->informed_eager = (h->informed_eager & 1) | (atoi(e) != 0 ? 6 : 0);
  h->da.lazy = 0;
  h->da.filter = 1;
  if (const char* e = getenv("RRTX_DUBINS_FILTER")) h->da.filter = atoi(e) != 0;
  if (const char* e = getenv("RRTX_DUBINS_LAZY")) h->da.lazy = atoi(e) != 0;
  if (c.algo == RRTX_ALGO_INFORMED) {
    for (int i = 0; i < B; i++) {
      const Inst& I = h->host_inst[i];
      h->iargs[i].xc[0] = (I.start[0] + I.goal[0]) / 2.0;   // x_center rrt_07:1056-1057
      h->iargs[i].xc[1] = (I.start[1] + I.goal[1]) / 2.0;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_iargs, h->iargs.data(), sizeof(rppi::InformedArgs) * B, hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // RRT* iteration kernel: every sample of the plan is drawn now, from the staged generators (part of the plan's time:
  // the stream depends on the seeds)
  if (R.use_v2 && (rc = launch_sample_stream(h, c, B))) return rc;
  R.stage = R.use_v2 ? 1 : 2;
  return RRTX_OK;
}

// One step of the plan in progress; a negative return leaves the run to rrtx_plan_step, which ends it
static int plan_step(rrtx_handle* h, int32_t* n_pending) {
  rrtx_handle::Run& R = h->run;
  HIPCHK(h, hipSetDevice(h->device));
  Ctx& c = h->c;
  const int B = h->n_inst;
  R.steps++;
  if (n_pending) *n_pending = B;
  if (R.stage == 1) {
    // RRT* (rrt_04, search_until_max_iter): one launch of the iteration kernel = v2_chunk_iters iterations of every instance
    int rc = launch_rrt_star_v2_once(h, c, B, R.v2_tpb);
    if (rc) return rc;
    R.v2_done_it += h->v2_chunk_iters;
    if (R.v2_done_it >= c.max_iter) {
      R.kms_main = R.kms;
      R.launches_main = R.launches;
      R.stage = 2;   // the general kernel then performs the final goal search (rrt_04:1080-1084)
    }
    return RRTX_OK;
  }
  if (c.algo == RRTX_ALGO_BITSTAR) {
    // One BOUNDED launch over the pending instances: persistent waves pull them from the device-side queue; an instance
    // that uses up its trips is carried over (its state stays in its slab) and queued again for the next launch
    const int np = (int)R.pending.size();
    const int32_t zero = 0;
    HIPCHK(h, hipMemcpyAsync(h->bit_queue, R.pending.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->bit_qhead, &zero, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    rppb::BitArgs ba = h->ba;
    ba.queue = h->bit_queue;
    ba.qhead = h->bit_qhead;
    ba.n_pending = np;
    ba.trip_bound = h->bit_trip_bound;
    const int grid = R.bit_grid < np ? R.bit_grid : np;
    int rc = timed_launch(h, true, [&] {
      if (R.bit_wave)
        hipLaunchKernelGGL(rppb::bitstar_wave_kernel, dim3(grid), dim3(64), 0, h->stream, ba, c.inst, c.results, B);
      else
        hipLaunchKernelGGL(rppb::bitstar_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, ba, c.inst, c.results, B);
    });
    if (rc) return rc;
    std::vector<int32_t> left;
    for (int32_t i : R.pending)
      if (!(R.res[i].status & RRTX_ST_DONE)) left.push_back(i);
    R.pending.swap(left);
    if (n_pending) *n_pending = (int32_t)R.pending.size();
    if (!R.pending.empty()) {
      if (R.launches > 4000000LL / h->bit_trip_bound + 16) {
        h->err = "BIT* kernel did not converge to DONE";
        return RRTX_E_STATE;
      }
      return RRTX_OK;
    }
    return plan_finish(h);
  }
  int rc = timed_launch(h, true, [&] { queue_main_kernel(h, c, B, h->da, false); });
  if (rc) return rc;
  int left = 0;
  for (int i = 0; i < B; i++)
    if (!(R.res[i].status & RRTX_ST_DONE)) left++;
  if (n_pending) *n_pending = left;
  if (left) {
    if (R.launches > (int64_t)h->p.max_iter / h->chunk_iters + 8 + R.launches_main) {
      h->err = "planner kernel did not converge to DONE";
      return RRTX_E_STATE;
    }
    return RRTX_OK;
  }
  return plan_finish(h);
}

int rrtx_plan_step(rrtx_handle* h, int32_t* n_pending) {
  if (!h) return RRTX_E_INVALID;
  if (h->run.stage == 0) return RRTX_E_STATE;
  const int rc = plan_step(h, n_pending);
  if (rc < 0) {   // an error ends the plan: its results are not valid
    h->run.stage = 0;
    h->planned = false;
  }
  return rc;
}

// Everything after the last instance has finished its main kernel: re-plans of instances that outgrew a fixed table, the
// counters, the return code
static int plan_finish(rrtx_handle* h) {
  rrtx_handle::Run& R = h->run;
  Ctx& c = h->c;
  const int B = h->n_inst;
  R.stage = 0;
  auto with_status = [&](int32_t bit) {   // the instances whose status word carries `bit`
    std::vector<int32_t> ids;
    for (int i = 0; i < B; i++)
      if (R.res[i].status & bit) ids.push_back(i);
    return ids;
  };
  int rc;
  // RRT* iteration kernel: an instance whose near set outgrew the LDS candidate table of its workgroup shape
  // (RRTX_ST_OVERFLOW) is planned again, from its staged start state, on the next larger shape (44 -> 128 -> 256
  // candidates), and finally by the general kernel (512).  Same results as a first plan on that shape: every shape
  // runs the same statements.
  if (R.use_v2 && !getenv("RRTX_NO_RETRY")) {
    // plans the instances `redo` again: shape = workgroup shape of the iteration kernel, 0 = general kernel alone
    auto replan_on = [&](const std::vector<int32_t>& redo, int shape) {
      return replan(h, redo, "retry", h->da, false, nullptr, [&](const Ctx& cr, int nr) {
        if (!shape) return (int)RRTX_OK;   // the general kernel draws its own samples
        // replan() staged the generators again: the same stream, and their end state back into the instances
        if (int rs = launch_sample_stream(h, cr, nr)) return rs;
        return launch_rrt_star_v2(h, cr, nr, shape);
      });
    };
    int shape = R.v2_tpb;   // 0 = general kernel
    for (;;) {
      const std::vector<int32_t> redo = with_status(RRTX_ST_OVERFLOW);
      if (redo.empty() || shape == 0) break;
      shape = shape == 64 ? 128 : shape == 128 ? 256 : 0;
      if (shape && h->m_max > v2_shape(shape).max_obs) continue;
      if ((rc = replan_on(redo, shape))) return rc;
    }
    // rewire moved a node while near_inds had repeated entries (rrt_04:1337 with :1372): the iteration kernel does not
    // walk the raw list (RRTX_ST_UNSUPPORTED in its status word), the general kernel does (rppk::rewire_raw_walk)
    const std::vector<int32_t> redo = with_status(RRTX_ST_UNSUPPORTED);
    if (!redo.empty() && (rc = replan_on(redo, 0))) return rc;
  }
  // Pose planners (rrt_03 / rrt_05 / rrt_06): an instance that ran out of polyline pool (edges replaced by rewire stay
  // allocated) is planned again, from its staged start state, with a pool four times as large -- twice if need be.
  // Overflows of the other fixed tables (near candidates, points per edge) are not helped by that and stay reported.
  if (is_pose_tree(c.algo) && !getenv("RRTX_NO_RETRY")) {
    int64_t big_cap = h->da.pool_cap;
    for (int attempt = 0; attempt < 2; attempt++) {
      const std::vector<int32_t> redo = with_status(RRTX_ST_OVERFLOW);
      if (redo.empty()) break;
      const int nr = (int)redo.size();
      big_cap *= 4;
      rrtx_handle::BigPool& bp = h->big[attempt];
      if (bp.cap != big_cap || bp.slabs < nr) {
        // (re)allocate this level: nothing of the CURRENT plan lives in it yet (its users are decided below), and the
        // previous plan's polylines are gone with the re-initialisation above
        bp = rrtx_handle::BigPool();
        const size_t bytes = sizeof(double) * (size_t)big_cap * nr;
        if (bp.px.reserve(bytes) != hipSuccess || bp.py.reserve(bytes) != hipSuccess ||
            (c.algo == RRTX_ALGO_RS && bp.pyaw.reserve(bytes) != hipSuccess)) {
          (void)hipGetLastError();   // no room for the larger pool: the instances keep their RRTX_ST_OVERFLOW
          bp = rrtx_handle::BigPool();
          break;
        }
        bp.cap = big_cap;
        bp.slabs = nr;
      }
      if (!h->pool_slot && (rc = dalloc(h, &h->pool_slot, B))) return rc;
      std::vector<int32_t> slot(B, 0);
      for (int k = 0; k < nr; k++) slot[redo[k]] = k;
      HIPCHK(h, hipMemcpyAsync(h->pool_slot, slot.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
      rppd::DubArgs dr = h->da;
      dr.pool_x = bp.px.as<double>(); dr.pool_y = bp.py.as<double>(); dr.pool_yaw = bp.pyaw.as<double>();
      dr.pool_cap = big_cap;
      dr.pool_slot = h->pool_slot;
      rc = replan(h, redo, "pool retry", dr, false, [&](int32_t i) -> int {
        HIPCHK(h, hipMemsetAsync(h->da.pool_used + i, 0, sizeof(int64_t), h->stream));
        return RRTX_OK;
      }, nullptr);
      if (rc) return rc;
      for (int k = 0; k < nr; k++) {
        rrtx_handle::PoolLoc& pl = h->pool_loc[redo[k]];
        pl.px = dr.pool_x; pl.py = dr.pool_y; pl.pyaw = dr.pool_yaw;
        pl.cap = big_cap; pl.slab = k;
      }
    }
  }
  // Informed RRT*: the near radius of rrt_07:1139 is not capped, so a near set can outgrow the 512 LDS candidate slots
  // of the product shape; those instances are planned again, from their staged start state, on the 2048-slot shape
  // (one workgroup per CU).  Same statements, same results as a first plan on that shape.
  if (c.algo == RRTX_ALGO_INFORMED && !getenv("RRTX_NO_RETRY")) {
    const std::vector<int32_t> redo = with_status(RRTX_ST_OVERFLOW);
    if (!redo.empty()) {
      const double inf1 = INFINITY;
      rc = replan(h, redo, "overflow retry", h->da, true, [&](int32_t i) -> int {
        HIPCHK(h, hipMemcpyAsync(h->cbest + i, &inf1, sizeof(double), hipMemcpyHostToDevice, h->stream));
        return RRTX_OK;
      }, nullptr);
      if (rc) return rc;
    }
  }
  // aggregate counters
  // summed on the device (rppk::stats_reduce_kernel): one small record comes back instead of every Inst
  if (!h->d_acc && (rc = dalloc(h, &h->d_acc, 1))) return rc;
  rppk::StatsAcc acc;
  HIPCHK(h, hipMemsetAsync(h->d_acc, 0, sizeof(rppk::StatsAcc), h->stream));
  hipLaunchKernelGGL(rppk::stats_reduce_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, c.inst, B, h->d_acc);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(&acc, h->d_acc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  rrtx_stats& s = h->stats;
  memset(&s, 0, sizeof(s));
  s.iterations = acc.sum[0];
  s.edges_unique = acc.sum[1];
  s.edges_ref = acc.sum[2];
  s.near_hits = acc.sum[3];
  s.near_unique = acc.sum[4];
  s.rewires = acc.sum[5];
  s.propagated = acc.sum[6];
  s.scan_nodes = acc.sum[7];
  s.algorithmic_bytes = acc.sum[8];
  s.exact_rescans = acc.sum[9];
  s.algorithmic_bytes_two_scan = acc.sum[10];
  s.total_nodes = acc.sum[11];
  s.f32_fallbacks = acc.sum[12];
  s.q16_fallbacks = acc.sum[13];
  s.passes_shared = acc.sum[14];
  s.near_unique_max = acc.nu_max;
  for (int k = 0; k < 16; k++) h->phase[k] = acc.phase[k];
  const bool overflow = (acc.status_or & RRTX_ST_OVERFLOW) != 0, unsupported = (acc.status_or & RRTX_ST_UNSUPPORTED) != 0,
             raises = (acc.status_or & RRTX_ST_REF_RAISES) != 0;
  s.launches = R.launches;
  s.kernel_ms = R.kms;
  s.launches_main = R.kms_main >= 0.0 ? R.launches_main : R.launches;
  s.kernel_ms_main = R.kms_main >= 0.0 ? R.kms_main : R.kms;
  s.replanned = h->stats_retried;
  s.main_shape = R.use_v2 ? R.v2_tpb
                        : c.algo == RRTX_ALGO_INFORMED ? rppi::TPB
                        : is_dubins(c.algo)            ? rppd::TPB
                        : c.algo == RRTX_ALGO_RS       ? rppr::TPB
                        : c.algo == RRTX_ALGO_BITSTAR  ? 64
                        : c.algo == RRTX_ALGO_LQR_RRT_STAR ? rppl::TPB
                                                       : rppk::TPB;
  s.main_f32 = R.use_v2 ? 1 : 0;   // kept for the ABI v5 layout: 1 whenever the RRT* iteration kernel ran
  s.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - R.t0).count();
  h->planned = true;
  h->traced_inst = h->trace_inst;
  // Per-instance conditions are per-instance results: the status word of each instance carries them
  // (rrtx_get_results), the other instances' trees are complete and valid.
  if (overflow || raises || unsupported) {
    h->err.clear();
    if (overflow)
      h->err += "RRTX_ST_OVERFLOW: a fixed on-device capacity was exceeded (near-candidate list, polyline pool, or a "
                "BIT* slab); ";
    if (raises)
      h->err += "RRTX_ST_REF_RAISES: the reference raises inside reeds_shepp_path_planning (ZeroDivisionError "
                "rrt_06:1183/:1207 or a math domain error); ";
    if (unsupported) h->err += "RRTX_ST_UNSUPPORTED: a reference code path the kernel does not restate was reached; ";
    if (raises && c.algo == RRTX_ALGO_LQR_RRT_STAR)
      h->err += "(LQR-RRT*: an LQR rollout never reached its target, IndexError rrt_09:1184, or a rewire closed a parent "
                "cycle); ";
    h->err += "the affected instances carry the bit in their status word and have no result, all others are complete";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

int rrtx_plan(rrtx_handle* h) {
  int rc = rrtx_plan_begin(h);
  if (rc < 0) return rc;
  while (h->run.stage != 0) rc = rrtx_plan_step(h, nullptr);   // a negative return ends the run
  return rc;
}

int rrtx_set_launch_bound(rrtx_handle* h, int32_t iterations) {
  if (!h || iterations < 1) return RRTX_E_INVALID;
  if (h->run.stage != 0) return RRTX_E_STATE;
  h->chunk_iters = iterations;
  h->v2_chunk_iters = iterations;
  h->bit_trip_bound = iterations;
  return RRTX_OK;
}

int rrtx_get_tree(rrtx_handle* h, int32_t instance, double* x, double* y, double* cost, int32_t* parent, int32_t cap,
                  int32_t* n_out) {
  if (!h || instance < 0 || instance >= h->n_inst || !n_out) return RRTX_E_INVALID;
  if (!h->planned) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  Result r;
  HIPCHK(h, hipMemcpy(&r, h->c.results + instance, sizeof(r), hipMemcpyDeviceToHost));
  *n_out = r.n_nodes;
  if ((x || y || cost || parent) && cap < r.n_nodes) return RRTX_E_CAPACITY;
  if (h->p.algo == RRTX_ALGO_BITSTAR) {
    // tree.vertices in insertion order: coordinates of the grid ids (rrt_08:115-135), g-scores, `nodes` parents
    const int n = r.n_nodes;
    std::vector<double> vid(n), vg(n), vpar(n);
    std::vector<int32_t> vh(n);
    const double* d = h->ba.dslab + (int64_t)instance * rppb::DSLAB + 3LL * rppb::SC + 3LL * rppb::LC;
    HIPCHK(h, hipMemcpy(vid.data(), d, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(vg.data(), d + rppb::VC, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(vpar.data(), d + 3LL * rppb::VC, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(vh.data(), h->ba.islab + (int64_t)instance * rppb::ISLAB, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    const rpp::BitCfg& bc = h->bcfg[instance];
    for (int i = 0; i < n; i++) {
      const double c1 = std::floor(vid[i] / bc.num_cells), c0 = std::floor((vid[i] - c1 * bc.num_cells) / 1);
      if (x) x[i] = bc.rand_min + 0.01 * c0;
      if (y) y[i] = bc.rand_min + 0.01 * c1;
      if (cost) cost[i] = vg[i];
      if (parent) {
        parent[i] = -1;
        if (vh[i])
          for (int j = 0; j < n; j++)
            if (vid[j] == vpar[i]) parent[i] = j;
      }
    }
    return RRTX_OK;
  }
  const int64_t off = (int64_t)instance * h->stride;
  if (x) HIPCHK(h, hipMemcpy(x, h->c.x + off, sizeof(double) * r.n_nodes, hipMemcpyDeviceToHost));
  if (y) HIPCHK(h, hipMemcpy(y, h->c.y + off, sizeof(double) * r.n_nodes, hipMemcpyDeviceToHost));
  if (cost) HIPCHK(h, hipMemcpy(cost, h->c.cost + off, sizeof(double) * r.n_nodes, hipMemcpyDeviceToHost));
  if (parent) HIPCHK(h, hipMemcpy(parent, h->c.parent + off, sizeof(int32_t) * r.n_nodes, hipMemcpyDeviceToHost));
  return RRTX_OK;
}

// generate_final_course of the pose planners: [goal] + reversed edge polylines up the parent chain + [start], `ncol` values
// per point: the pool columns `cols` of the instance (x and y, or yaw) and components comp0 .. of the goal and start poses.
// `out` NULL: the point count alone.
static int final_course(rrtx_handle* h, int32_t instance, const Inst& I, const double* const* cols, int ncol, int comp0,
                        double* out, int32_t cap_points, int32_t* n_out) {
  const int n = I.n;
  const int64_t off = (int64_t)instance * h->stride;
  std::vector<int32_t> par(n), plen(n);
  std::vector<int64_t> poff(n);
  HIPCHK(h, hipMemcpy(par.data(), h->c.parent + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(plen.data(), h->da.plen + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(poff.data(), h->da.poff + off, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  int64_t total = 2;
  for (int nd = I.goal_node; par[nd] >= 0; nd = par[nd]) total += plen[nd];
  *n_out = (int32_t)total;
  if (!out) return RRTX_OK;
  if (cap_points < total) return RRTX_E_CAPACITY;
  for (int j = 0; j < ncol; j++) out[j] = I.goal[comp0 + j];
  int64_t k = 1;
  std::vector<double> buf;
  for (int nd = I.goal_node; par[nd] >= 0; nd = par[nd]) {
    buf.resize(plen[nd]);
    for (int j = 0; j < ncol; j++) {
      HIPCHK(h, hipMemcpy(buf.data(), h->pool_loc[instance].at(cols[j], poff[nd]), sizeof(double) * plen[nd], hipMemcpyDeviceToHost));
      for (int q = plen[nd] - 1; q >= 0; q--) out[ncol * (k + plen[nd] - 1 - q) + j] = buf[q];
    }
    k += plen[nd];
  }
  for (int j = 0; j < ncol; j++) out[ncol * k + j] = I.start[comp0 + j];
  return RRTX_OK;
}

int rrtx_get_path(rrtx_handle* h, int32_t instance, double* xy, int32_t cap_points, int32_t* n_out) {
  if (!h || instance < 0 || instance >= h->n_inst || !n_out) return RRTX_E_INVALID;
  if (!h->planned) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  Inst I;
  HIPCHK(h, hipMemcpy(&I, h->c.inst + instance, sizeof(I), hipMemcpyDeviceToHost));
  if (!(I.status & RRTX_ST_PATH)) {
    *n_out = 0;
    return RRTX_OK;
  }
  if (h->p.algo == RRTX_ALGO_BITSTAR) {
    int32_t oi[8];
    HIPCHK(h, hipMemcpy(oi, h->ba.out_i + 8 * instance, sizeof(oi), hipMemcpyDeviceToHost));
    *n_out = oi[3];
    if (!xy || oi[3] == 0) return RRTX_OK;
    if (cap_points < oi[3]) return RRTX_E_CAPACITY;
    const double* d = h->ba.dslab + (int64_t)instance * rppb::DSLAB + 3LL * rppb::SC + 3LL * rppb::LC + 5LL * rppb::VC +
                      2LL * rppb::EC;
    HIPCHK(h, hipMemcpy(xy, d, sizeof(double) * 2 * oi[3], hipMemcpyDeviceToHost));
    return RRTX_OK;
  }
  if (is_pose_tree(h->p.algo)) {   // rrt_05:1512-1521
    const rrtx_handle::PoolLoc& pl = h->pool_loc[instance];
    const double* cols[2] = {pl.px, pl.py};
    return final_course(h, instance, I, cols, 2, 0, xy, cap_points, n_out);
  }
  *n_out = I.path_n;
  if (!xy) return RRTX_OK;
  if (cap_points < I.path_n) return RRTX_E_CAPACITY;
  if (!(I.status & RRTX_ST_PATH_TRUNC)) {
    HIPCHK(h, hipMemcpy(xy, h->c.path_xy + (int64_t)instance * h->c.path_cap * 2, sizeof(double) * 2 * I.path_n,
                        hipMemcpyDeviceToHost));
    return RRTX_OK;
  }
  // deeper than the on-device path buffer: walk the parent array on the host (rrt_04:1117-1125)
  const int n = I.n;
  std::vector<double> x(n), y(n);
  std::vector<int32_t> par(n);
  const int64_t off = (int64_t)instance * h->stride;
  HIPCHK(h, hipMemcpy(x.data(), h->c.x + off, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(y.data(), h->c.y + off, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(par.data(), h->c.parent + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  int k = 0;
  xy[0] = I.goal[0];
  xy[1] = I.goal[1];
  k = 1;
  for (int nd = I.goal_node;; nd = par[nd]) {
    xy[2 * k] = x[nd];
    xy[2 * k + 1] = y[nd];
    k++;
    if (par[nd] < 0) break;
  }
  return RRTX_OK;
}

int rrtx_get_results(rrtx_handle* h, double* path_cost, int32_t* n_nodes, int32_t* status) {
  if (!h) return RRTX_E_INVALID;
  if (!h->planned && h->run.stage == 0) return RRTX_E_STATE;   // between steps of a plan: the records of the finished instances are final
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<Result> r(h->n_inst);
  HIPCHK(h, hipMemcpy(r.data(), h->c.results, sizeof(Result) * h->n_inst, hipMemcpyDeviceToHost));
  for (int i = 0; i < h->n_inst; i++) {
    if (path_cost) path_cost[i] = (r[i].status & RRTX_ST_PATH) ? r[i].path_cost : INFINITY;
    if (n_nodes) n_nodes[i] = r[i].n_nodes;
    if (status) status[i] = r[i].status;
  }
  return RRTX_OK;
}

int rrtx_results_device_ptr(rrtx_handle* h, void** dptr, int64_t* bytes) {
  if (!h || !dptr || !bytes) return RRTX_E_INVALID;
  *dptr = (void*)h->c.results;
  *bytes = (int64_t)sizeof(Result) * h->n_inst;
  return RRTX_OK;
}

int rrtx_copy_results_device(rrtx_handle* h, void* dst_device, int64_t bytes) {
  if (!h || !dst_device) return RRTX_E_INVALID;
  if (!h->planned) return RRTX_E_STATE;
  if (bytes < (int64_t)sizeof(Result) * h->n_inst) return RRTX_E_CAPACITY;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(dst_device, h->c.results, sizeof(Result) * h->n_inst, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return RRTX_OK;
}

int rrtx_get_yaw(rrtx_handle* h, int32_t instance, double* yaw, int32_t cap) {
  if (!h || !yaw || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (!h->planned || !is_pose_tree(h->p.algo)) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  Result r;
  HIPCHK(h, hipMemcpy(&r, h->c.results + instance, sizeof(r), hipMemcpyDeviceToHost));
  if (cap < r.n_nodes) return RRTX_E_CAPACITY;
  HIPCHK(h, hipMemcpy(yaw, h->da.yaw + (int64_t)instance * h->stride, sizeof(double) * r.n_nodes, hipMemcpyDeviceToHost));
  return RRTX_OK;
}

int rrtx_get_path_yaw(rrtx_handle* h, int32_t instance, double* yaw, int32_t cap_points, int32_t* n_out) {
  if (!h || instance < 0 || instance >= h->n_inst || !n_out) return RRTX_E_INVALID;
  if (!h->planned || h->p.algo != RRTX_ALGO_RS) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  Inst I;
  HIPCHK(h, hipMemcpy(&I, h->c.inst + instance, sizeof(I), hipMemcpyDeviceToHost));
  *n_out = 0;
  if (!(I.status & RRTX_ST_PATH)) return RRTX_OK;
  return final_course(h, instance, I, &h->pool_loc[instance].pyaw, 1, 2, yaw, cap_points, n_out);   // rrt_06:1643-1651
}

// LQR-RRT*: Node.path_x / path_y regenerated on the device from each node's edge endpoints (rpp_lqr.h, the same code
// the planner kernel runs); the root has none
static int lqr_polylines(rrtx_handle* h, int32_t instance, int32_t* plen, int32_t cap_nodes, double* px, double* py,
                         int64_t cap_points, int64_t* n_points_out) {
  Result r;
  HIPCHK(h, hipMemcpy(&r, h->c.results + instance, sizeof(r), hipMemcpyDeviceToHost));
  const int n = r.n_nodes;
  const int64_t off = (int64_t)instance * h->stride;
  int32_t* dcnt = nullptr;
  int64_t* doff = nullptr;
  double *dx = nullptr, *dy = nullptr;
  auto release = [&]() {
    if (dcnt) (void)hipFree(dcnt);
    if (doff) (void)hipFree(doff);
    if (dx) (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
  };
  if (hipMalloc((void**)&dcnt, sizeof(int32_t) * (n + 1)) != hipSuccess ||
      hipMalloc((void**)&doff, sizeof(int64_t) * (n + 1)) != hipSuccess) {
    release();
    h->err = "rrtx_get_polylines: device allocation failed";
    return RRTX_E_HIP;
  }
  const double* ef = h->la.ef + 4 * off;
  const int32_t* par = h->c.parent + off;
  hipLaunchKernelGGL(rppl::lqr_polylines_kernel, dim3((n + 63) / 64), dim3(64), 0, h->stream, ef, par, n, h->la.step,
                     h->la.nt, dcnt, (const int64_t*)nullptr, (double*)nullptr, (double*)nullptr);
  std::vector<int32_t> cnt(n);
  std::vector<int64_t> po(n + 1, 0);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
      hipMemcpy(cnt.data(), dcnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost) != hipSuccess) {
    release();
    h->err = "rrtx_get_polylines: count pass failed";
    return RRTX_E_HIP;
  }
  for (int i = 0; i < n; i++) po[i + 1] = po[i] + cnt[i];
  const int64_t total = po[n];
  *n_points_out = total;
  if ((!plen && !px && !py) || total == 0) {
    release();
    if ((plen || px || py) && cap_nodes < n) return RRTX_E_CAPACITY;
    for (int i = 0; plen && i < n; i++) plen[i] = cnt[i];
    return RRTX_OK;
  }
  if (cap_nodes < n || cap_points < total) {
    release();
    return RRTX_E_CAPACITY;
  }
  std::vector<double> bx(total), by(total);
  if (hipMalloc((void**)&dx, sizeof(double) * total) != hipSuccess || hipMalloc((void**)&dy, sizeof(double) * total) != hipSuccess ||
      hipMemcpy(doff, po.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice) != hipSuccess) {
    release();
    h->err = "rrtx_get_polylines: device allocation failed";
    return RRTX_E_HIP;
  }
  hipLaunchKernelGGL(rppl::lqr_polylines_kernel, dim3((n + 63) / 64), dim3(64), 0, h->stream, ef, par, n, h->la.step,
                     h->la.nt, dcnt, (const int64_t*)doff, dx, dy);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess &&
                  hipMemcpy(bx.data(), dx, sizeof(double) * total, hipMemcpyDeviceToHost) == hipSuccess &&
                  hipMemcpy(by.data(), dy, sizeof(double) * total, hipMemcpyDeviceToHost) == hipSuccess;
  release();
  if (!ok) {
    h->err = "rrtx_get_polylines: point pass failed";
    return RRTX_E_HIP;
  }
  for (int i = 0; plen && i < n; i++) plen[i] = cnt[i];
  for (int64_t q = 0; q < total; q++) {
    if (px) px[q] = bx[q];
    if (py) py[q] = by[q];
  }
  return RRTX_OK;
}

int rrtx_get_polylines(rrtx_handle* h, int32_t instance, int32_t* plen, int32_t cap_nodes, double* px, double* py,
                       int64_t cap_points, int64_t* n_points_out) {
  if (!h || !n_points_out || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (!h->planned || !(is_pose_tree(h->p.algo) || h->p.algo == RRTX_ALGO_LQR_RRT_STAR)) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->p.algo == RRTX_ALGO_LQR_RRT_STAR) return lqr_polylines(h, instance, plen, cap_nodes, px, py, cap_points, n_points_out);
  Result r;
  HIPCHK(h, hipMemcpy(&r, h->c.results + instance, sizeof(r), hipMemcpyDeviceToHost));
  const int n = r.n_nodes;
  const int64_t off = (int64_t)instance * h->stride;
  std::vector<int32_t> pl(n);
  std::vector<int64_t> po(n);
  HIPCHK(h, hipMemcpy(pl.data(), h->da.plen + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(po.data(), h->da.poff + off, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  int64_t total = 0;
  for (int i = 0; i < n; i++) total += pl[i];
  *n_points_out = total;
  if (!plen && !px && !py) return RRTX_OK;
  if (cap_nodes < n || cap_points < total) return RRTX_E_CAPACITY;
  int64_t used = 0;
  HIPCHK(h, hipMemcpy(&used, h->da.pool_used + instance, sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<double> bx(used), by(used);
  if (used) {
    const rrtx_handle::PoolLoc& pl = h->pool_loc[instance];
    HIPCHK(h, hipMemcpy(bx.data(), pl.at(pl.px), sizeof(double) * used, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(by.data(), pl.at(pl.py), sizeof(double) * used, hipMemcpyDeviceToHost));
  }
  int64_t w = 0;
  for (int i = 0; i < n; i++) {
    if (plen) plen[i] = pl[i];
    for (int q = 0; q < pl[i]; q++) {
      if (px) px[w] = bx[po[i] + q];
      if (py) py[w] = by[po[i] + q];
      w++;
    }
  }
  return RRTX_OK;
}

int rrtx_get_sobol_index(rrtx_handle* h, int32_t instance, int64_t* index) {
  if (!h || !index || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (!h->planned) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  rpp::Sobol s;
  HIPCHK(h, hipMemcpy(&s, &h->c.inst[instance].sobol, sizeof(s), hipMemcpyDeviceToHost));
  *index = s.index;
  return RRTX_OK;
}

int rrtx_get_stats(rrtx_handle* h, rrtx_stats* st) {
  if (!h || !st) return RRTX_E_INVALID;
  *st = h->stats;
  return RRTX_OK;
}

int rrtx_get_phase_cycles(rrtx_handle* h, int64_t* out16) {
  if (!h || !out16) return RRTX_E_INVALID;
  memcpy(out16, h->phase, sizeof(h->phase));
  return RRTX_OK;
}

int rrtx_get_sample_stream(rrtx_handle* h, int32_t instance, int32_t first, int32_t count, double* out_xy) {
  if (!h || instance < 0 || instance >= h->n_inst || first < 0 || count < 0 || (count > 0 && !out_xy)) return RRTX_E_INVALID;
  if (!h->planned || !h->c.samp || h->stats.main_f32 != 1) return RRTX_E_STATE;   // no plan of the iteration kernel to read
  if ((int64_t)first + count > h->c.max_iter) return RRTX_E_INVALID;
  if (!count) return RRTX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(out_xy, h->c.samp + 2 * ((int64_t)instance * h->c.max_iter + first), sizeof(double) * 2 * (size_t)count,
                      hipMemcpyDeviceToHost));
  return RRTX_OK;
}

int rrtx_get_trace(rrtx_handle* h, double* rnd_x, double* rnd_y, int32_t* nearest, int32_t* n_near, int32_t cap,
                   int32_t* n_out) {
  if (!h || !n_out) return RRTX_E_INVALID;
  // the rows are those of the instance the last completed plan traced
  if (!h->planned || h->trace_inst < 0 || h->traced_inst != h->trace_inst) return RRTX_E_STATE;
  const bool want = rnd_x || rnd_y || nearest || n_near;   // all NULL: the row count alone
  HIPCHK(h, hipSetDevice(h->device));
  if (h->p.algo == RRTX_ALGO_BITSTAR) {   // rnd_x / rnd_y carry the ids of the popped edges (bestEdge[0], bestEdge[1])
    int32_t oi[8];
    HIPCHK(h, hipMemcpy(oi, h->ba.out_i + 8 * h->trace_inst, sizeof(oi), hipMemcpyDeviceToHost));
    *n_out = oi[6];
    if ((want && cap < oi[6]) || oi[6] > h->ba.tr_cap) return RRTX_E_CAPACITY;
    if (rnd_x) HIPCHK(h, hipMemcpy(rnd_x, h->ba.tr_a, sizeof(double) * oi[6], hipMemcpyDeviceToHost));
    if (rnd_y) HIPCHK(h, hipMemcpy(rnd_y, h->ba.tr_b, sizeof(double) * oi[6], hipMemcpyDeviceToHost));
    return RRTX_OK;
  }
  Inst I;
  HIPCHK(h, hipMemcpy(&I, h->c.inst + h->trace_inst, sizeof(I), hipMemcpyDeviceToHost));
  const int n = I.it;
  *n_out = n;
  if (want && cap < n) return RRTX_E_CAPACITY;
  if (rnd_x) HIPCHK(h, hipMemcpy(rnd_x, h->c.tr_rx, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (rnd_y) HIPCHK(h, hipMemcpy(rnd_y, h->c.tr_ry, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (nearest) HIPCHK(h, hipMemcpy(nearest, h->c.tr_near, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (n_near) HIPCHK(h, hipMemcpy(n_near, h->c.tr_nn, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return RRTX_OK;
}

int rrtx_get_trace_kind(rrtx_handle* h, int32_t* kind, int32_t cap, int32_t* n_out) {
  if (!h || !n_out) return RRTX_E_INVALID;
  if (!h->planned || h->trace_inst < 0 || h->traced_inst != h->trace_inst || !h->c.tr_kind) return RRTX_E_STATE;
  if (h->p.algo != RRTX_ALGO_RRT && h->p.algo != RRTX_ALGO_RRT_STAR) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  Inst I;
  HIPCHK(h, hipMemcpy(&I, h->c.inst + h->trace_inst, sizeof(I), hipMemcpyDeviceToHost));
  *n_out = I.it;
  if (kind && cap < I.it) return RRTX_E_CAPACITY;
  if (kind) HIPCHK(h, hipMemcpy(kind, h->c.tr_kind, sizeof(int32_t) * I.it, hipMemcpyDeviceToHost));
  return RRTX_OK;
}

// ---- path smoothing (rrt_04:1447-1479)
static int smooth_status_rc(const std::vector<int32_t>& st, std::string* err) {
  for (int32_t v : st) {
    if (v == rpps::SM_CAPACITY) {
      if (err) *err = "path smoothing: polyline or obstacle list exceeds the on-device capacity";
      return RRTX_E_OVERFLOW;
    }
    if (v == rpps::SM_ZERODIV) {
      if (err) *err = "path smoothing: the reference raises ZeroDivisionError on this input (zero-length pair)";
      return RRTX_E_STATE;
    }
  }
  return RRTX_OK;
}


int rrtx_smooth_planned(rrtx_handle* h, int32_t max_iter) {
  if (!h || max_iter < 0) return RRTX_E_INVALID;
  if (int rc = refuse_with_map(h, "rrtx_smooth_planned")) return rc;   // first: RRTX_E_STATE either way, and this one says why
  if (!h->planned || (h->p.algo != RRTX_ALGO_RRT && h->p.algo != RRTX_ALGO_RRT_STAR && h->p.algo != RRTX_ALGO_LQR_RRT_STAR))
    return RRTX_E_STATE;
  if (h->m_max > rpps::MOB) return RRTX_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  const int B = h->n_inst;
  int rc;
  if (!h->sm_xy) {
    h->sm_stride = rpps::PC;
    if ((rc = dalloc(h, &h->sm_xy, (size_t)2 * h->sm_stride * B))) return rc;
    if ((rc = dalloc(h, &h->sm_n, B))) return rc;
    if ((rc = dalloc(h, &h->sm_status, B))) return rc;
    if ((rc = dalloc(h, &h->sm_obs, (size_t)2 * B))) return rc;
  }
  // each instance's path against its obstacle rows as set NOW (sizes as given: h->sm_osz) -- the table may have been
  // replaced since the plan, and the rows the planned Inst records name are then stale
  std::vector<int32_t> rows((size_t)2 * B);
  for (int i = 0; i < B; i++) {
    rows[2 * i] = h->host_inst[i].obs_base;
    rows[2 * i + 1] = h->host_inst[i].obs_m;
  }
  HIPCHK(h, hipMemcpyAsync(h->sm_obs, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice, h->stream));
  Ctx& c = h->c;
  const int64_t istride = (int64_t)(sizeof(Inst) / sizeof(int32_t));
  rpps::SmoothArgs a{c.path_xy, c.path_cap, &c.inst[0].path_n, istride,
                     &c.inst[0].rng, (int64_t)sizeof(Inst), c.ox, c.oy, h->sm_osz, h->sm_obs, 2, max_iter,
                     h->sm_xy, h->sm_stride, h->sm_n, h->sm_status};
  hipLaunchKernelGGL(rpps::smooth_kernel, dim3(B), dim3(64), 0, h->stream, a, B);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::vector<int32_t> st(B);
  HIPCHK(h, hipMemcpy(st.data(), h->sm_status, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  h->smoothed = true;
  if (h->cs.which == RRTX_COURSE_SMOOTHED) h->cs.valid = false;   // gathered from the previous smoothing run
  return smooth_status_rc(st, &h->err);
}

int rrtx_get_smoothed_path(rrtx_handle* h, int32_t instance, double* xy, int32_t cap_points, int32_t* n_out) {
  if (!h || !n_out || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (!h->smoothed) return RRTX_E_STATE;
  int32_t n = 0;
  HIPCHK(h, hipMemcpy(&n, h->sm_n + instance, sizeof(n), hipMemcpyDeviceToHost));
  *n_out = n;
  if (!xy || n == 0) return RRTX_OK;
  if (cap_points < n) return RRTX_E_CAPACITY;
  HIPCHK(h, hipMemcpy(xy, h->sm_xy + (size_t)2 * h->sm_stride * instance, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
  return RRTX_OK;
}

// ---- closed-loop stage of rrt_10 on the planned Reeds-Shepp trees (rrt_track.hip.h) ----------------------------------
int rrtx_set_rs_cost(rrtx_handle* h, int32_t mode) {
  if (!h || (mode != RRTX_RS_COST_EUCLID && mode != RRTX_RS_COST_PATH)) return RRTX_E_INVALID;
  if (h->p.algo != RRTX_ALGO_RS) return RRTX_E_STATE;
  int rc = refuse_in_plan(h, "rrtx_set_rs_cost");
  if (rc) return rc;
  h->rs_cost = mode;
  return RRTX_OK;
}

int rrtx_track_planned(rrtx_handle* h, const rrtx_track_params* tp) {
  if (!h || !tp) return RRTX_E_INVALID;
  if (!h->planned || h->p.algo != RRTX_ALGO_RS) return RRTX_E_STATE;
  int rc = refuse_in_plan(h, "rrtx_track_planned");
  if (rc) return rc;
  if (!track_params_ok(tp)) return fail(h, RRTX_E_INVALID, std::string("rrtx_track_planned: ") + TRACK_PARAMS_MSG);
  HIPCHK(h, hipSetDevice(h->device));
  rrtx_handle::Track& K = h->tk;
  const int B = h->n_inst;
  const size_t tot = (size_t)h->stride * B;
  K.valid = false;
  if (!K.cand) {
    const int64_t want = (int64_t)h->n_cu * 16;
    K.blocks = (int)((int64_t)tot < want ? (int64_t)tot : want);
    if (K.blocks < 1) K.blocks = 1;
    if ((rc = dalloc(h, &K.cand, tot))) return rc;
    if ((rc = dalloc(h, &K.rec, tot))) return rc;
    if ((rc = dalloc(h, &K.jobs, 2 * tot))) return rc;
    if ((rc = dalloc(h, &K.counters, 4))) return rc;
    if ((rc = dalloc(h, &K.outc, B))) return rc;
    if ((rc = dalloc(h, &K.pool, (size_t)3 * B))) return rc;
    if ((rc = dalloc(h, &K.out_off, B))) return rc;
    if ((rc = dalloc(h, &K.slab, (size_t)K.blocks * 3 * rppt::SLAB_PTS))) return rc;
  }
  std::vector<const double*> pp((size_t)3 * B);
  for (int i = 0; i < B; i++) {
    const rrtx_handle::PoolLoc& pl = h->pool_loc[i];
    pp[3 * i] = pl.at(pl.px);
    pp[3 * i + 1] = pl.at(pl.py);
    pp[3 * i + 2] = pl.at(pl.pyaw);
  }
  HIPCHK(h, hipMemcpyAsync(K.pool, pp.data(), sizeof(double*) * pp.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(K.counters, 0, sizeof(int32_t) * 4, h->stream));
  rppt::TrackArgs a;
  memset(&a, 0, sizeof(a));
  a.inst = h->c.inst;
  a.x = h->c.x;
  a.y = h->c.y;
  a.yaw = h->da.yaw;
  a.parent = h->c.parent;
  a.poff = h->da.poff;
  a.plen = h->da.plen;
  a.stride = h->stride;
  a.pool = K.pool;
  a.ox = h->c.ox;
  a.oy = h->c.oy;
  a.othr = h->c.othr;
  memcpy(&a.P, tp, sizeof(a.P));
  a.n_inst = B;
  a.cand = K.cand;
  a.rec = K.rec;
  a.jobs = K.jobs;
  a.counters = K.counters;
  a.slab = K.slab;
  a.outc = K.outc;
  a.out_off = K.out_off;
  K.h_outc.resize(B);
  K.h_off.assign(B, 0);
  // with an obstacle map every instance's rows are empty: the roll-outs ask the map, whose thr carries robot_radius as the rows do
  const rppo::Map mp = h->om.on ? h->om.grid.map() : rppo::Map{};
  float ms = 0.f;
  rc = h->timed(&ms, [&] {
    hipLaunchKernelGGL(rppt::track_list_kernel, dim3(B), dim3(rppt::TPB), 0, h->stream, a);
    if (h->om.on)
      hipLaunchKernelGGL((rppt::track_roll_kernel<rppt::CHECK_INDEX>), dim3(K.blocks), dim3(rppt::TPB), 0, h->stream, a, 0, mp);
    else
      hipLaunchKernelGGL((rppt::track_roll_kernel<rppt::CHECK_LINEAR>), dim3(K.blocks), dim3(rppt::TPB), 0, h->stream, a, 0, mp);
    hipLaunchKernelGGL(rppt::track_pick_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, a);
  }, [&]() -> int {
    HIPCHK(h, hipMemcpyAsync(K.h_outc.data(), K.outc, sizeof(rppt::Outcome) * B, hipMemcpyDeviceToHost, h->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  K.ms = ms;
  // the winners' arrays: 7 x (len + 1) doubles per instance with a feasible roll-out, packed
  int64_t need = 0;
  int winners = 0;
  for (int i = 0; i < B; i++) {
    K.h_off[i] = need;
    if (K.h_outc[i].flag) {
      need += 7 * ((int64_t)K.h_outc[i].len + 1);
      winners++;
    }
  }
  if ((rc = h->reserve(K.out, sizeof(double) * (size_t)need))) return rc;
  if (winners) {
    a.out = K.out.as<double>();
    HIPCHK(h, hipMemcpyAsync(K.out_off, K.h_off.data(), sizeof(int64_t) * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(K.counters + 1, 0, sizeof(int32_t), h->stream));
    rc = h->timed(&ms, [&] {
      const dim3 grid(winners < K.blocks ? winners : K.blocks);
      if (h->om.on)
        hipLaunchKernelGGL((rppt::track_roll_kernel<rppt::CHECK_INDEX>), grid, dim3(rppt::TPB), 0, h->stream, a, 1, mp);
      else
        hipLaunchKernelGGL((rppt::track_roll_kernel<rppt::CHECK_LINEAR>), grid, dim3(rppt::TPB), 0, h->stream, a, 1, mp);
    });
    if (rc) return rc;
    K.ms += ms;
  }
  K.valid = true;
  for (int i = 0; i < B; i++)
    if (K.h_outc[i].status) return RRTX_PARTIAL;
  return RRTX_OK;
}

int rrtx_get_track_outcome(rrtx_handle* h, int32_t instance, rrtx_track_outcome* out) {
  if (!h || !out || instance < 0 || instance >= h->n_inst) return RRTX_E_INVALID;
  if (!h->planned || !h->tk.valid) return RRTX_E_STATE;
  memcpy(out, &h->tk.h_outc[instance], sizeof(*out));
  return RRTX_OK;
}

int rrtx_get_track_arrays(rrtx_handle* h, int32_t instance, double* x, double* y, double* yaw, double* v, double* t,
                          double* a, double* d, int32_t cap) {
  if (!h || instance < 0 || instance >= h->n_inst || !x || !y || !yaw || !v || !t || !a || !d) return RRTX_E_INVALID;
  if (!h->planned || !h->tk.valid) return RRTX_E_STATE;
  const rppt::Outcome& o = h->tk.h_outc[instance];
  if (!o.flag) return RRTX_E_STATE;
  if (cap < o.len + 1) return RRTX_E_CAPACITY;
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t os = (int64_t)o.len + 1;
  std::vector<double> buf((size_t)(7 * os));
  HIPCHK(h, hipMemcpy(buf.data(), h->tk.out.as<double>() + h->tk.h_off[instance], sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
  double* dst[7] = {x, y, yaw, v, t, a, d};
  for (int k = 0; k < 7; k++) memcpy(dst[k], buf.data() + k * os, sizeof(double) * (size_t)(k < 3 ? os : os - 1));
  return RRTX_OK;
}

int rrtx_get_track_records(rrtx_handle* h, int32_t instance, int32_t* cand, rrtx_track_record* rec, int32_t cap) {
  if (!h || instance < 0 || instance >= h->n_inst || !cand || !rec) return RRTX_E_INVALID;
  if (!h->planned || !h->tk.valid) return RRTX_E_STATE;
  const int n = h->tk.h_outc[instance].n_cand;
  if (cap < n) return RRTX_E_CAPACITY;
  if (!n) return RRTX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t off = (int64_t)instance * h->stride;
  HIPCHK(h, hipMemcpy(cand, h->tk.cand + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(rec, h->tk.rec + off, sizeof(rrtx_track_record) * n, hipMemcpyDeviceToHost));
  return RRTX_OK;
}

int rrtx_get_track_stats(rrtx_handle* h, double* kernel_ms, int64_t* steps) {
  if (!h || !kernel_ms || !steps) return RRTX_E_INVALID;
  if (!h->planned || !h->tk.valid) return RRTX_E_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<rppt::Record> rec((size_t)h->stride * h->n_inst);
  HIPCHK(h, hipMemcpy(rec.data(), h->tk.rec, sizeof(rppt::Record) * rec.size(), hipMemcpyDeviceToHost));
  int64_t s = 0;
  for (int i = 0; i < h->n_inst; i++) {
    for (int k = 0; k < h->tk.h_outc[i].n_cand; k++) s += rec[(size_t)i * h->stride + k].n;
    if (h->tk.h_outc[i].flag) s += h->tk.h_outc[i].len;
  }
  *kernel_ms = h->tk.ms;
  *steps = s;
  return RRTX_OK;
}

}  // extern "C"

#include "rrtx_api_obsmap.inc"
#include "rrtx_api_tools.inc"
#include "rrtx_api_rccl.inc"
#include "rrtx_api_steer.inc"
#include "rrtx_api_spline.inc"
#include "rrtx_api_bspline.inc"
#include "rrtx_api_courses.inc"
#include "rrtx_api_goalq.inc"
#include "rrtx_api_goaltrack.inc"
#include "rrtx_api_tracker.inc"   // after the four producers: rrtx_tracker_run_from reads their objects
#include "rrtx_api_armnav.inc"
#include "rrtx_api_armik.inc"
#include "rrtx_api_armdh.inc"

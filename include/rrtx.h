/*
 * rrtx.h -- C ABI of the MI355X-native batched RRT / RRT* planner.
 *
 * The reference (gouldberg/robotics-path-planning) has no FFI layer: its
 * boundary is the Python class surface `RRT(...).planning(animation)` and the
 * attributes callers read afterwards.  This ABI is what a ctypes
 * binding on the reference side calls in place of the body of
 *   10_path_planning_01_rrt_01_simple.py   RRT.planning            :71-101
 *   10_path_planning_01_rrt_04_rrt_star.py RRT.planning            :1036-1084
 *   10_path_planning_01_rrt_07_informed_rrt_star.py RRT.informed_rrt_star_search :1044-1108
 *   10_path_planning_01_rrt_05_rrt_star_dubins_path.py RRT.planning :1416-1456
 *   10_path_planning_01_rrt_08_batch_informed_rrt_star.py BITStar.plan :236-331
 * Each entry point names the reference interface it replaces.  Plain pointers
 * and sizes only; the caller owns every host buffer, the library owns device
 * memory behind the opaque handle.  Every function returns 0 or a negative
 * RRTX_E_* code and never throws.  A handle is bound to one device and is not
 * thread safe (one host thread per handle; multi-GPU = one handle per device).
 * There is NO CPU fallback: without a usable gfx950 device rrtx_create fails
 * with RRTX_E_NO_DEVICE.
 */
#ifndef RRTX_H
#define RRTX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RRTX_ABI_VERSION 6   /* 6: rrtx_set_instance_obstacles (and RRTX_ALGO_LQR_RRT_STAR: a new algo value, no layout change; the rrtx_steer_* and
                                rrtx_tracker_* entry points: new functions on objects of their own, no layout change; later additions of
                                the same kind: rrtx_steer_set_obstacles, rrtx_steer_get_hits, rrtx_steer_solve_lqr, rrtx_steer_get_ends,
                                rrtx_steer_solve_bezier, rrtx_steer_solve_bezier_cp, rrtx_steer_get_curvature, rrtx_steer_get_kmax,
                                rrtx_steer_get_control_points, rrtx_steer_solve_all, rrtx_steer_get_cand_counts,
                                rrtx_steer_get_cand_summary, rrtx_steer_get_cand_points, rrtx_steer_select_free, rrtx_tracker_run_from,
                                rrtx_tracker_get_winners, rrtx_tracker_get_goals, rrtx_*_get_generation, rrtx_gather_courses, rrtx_get_course_counts,
                                rrtx_get_courses, rrtx_get_course_generation, RRTX_SRC_PLANNER, rrtx_query_goals and its getters,
                                rrtx_set_obstacle_map and its getters, rrtx_*_set_obstacle_index and their getters, the tracker's included); 5: rrtx_stats.passes_shared; 2: rrtx_params.step_size, RRTX_ALGO_RS, rrtx_get_path_yaw; 3: RRTX_PARTIAL,
                                rrtx_copy_results_device, per-instance yaw and informed rotation; 4: rrtx_plan_many,
                                rrtx_selfcheck, rrtx_stats.main_shape / main_f32, rrtx_plan_begin / _step, rrtx_set_launch_bound,
                                RRTX_ST_REF_HANGS, rrtx_rccl_* */

enum {
  RRTX_PARTIAL = 1,        /* rrtx_plan only: the call completed, but at least one instance stopped with RRTX_ST_OVERFLOW,
                              RRTX_ST_UNSUPPORTED or RRTX_ST_REF_RAISES in its status word (rrtx_get_results); every
                              other instance is complete and valid.  Not an error: errors are negative. */
  RRTX_OK = 0,
  RRTX_E_INVALID = -1,     /* bad argument / unsupported parameter combination */
  RRTX_E_NO_DEVICE = -2,   /* no HIP device, or not gfx950 */
  RRTX_E_HIP = -3,         /* HIP runtime error, see rrtx_last_error */
  RRTX_E_CAPACITY = -4,    /* caller buffer too small */
  RRTX_E_STATE = -5,       /* call order (e.g. get_tree before plan) */
  RRTX_E_OVERFLOW = -6     /* a whole-call capacity was exceeded (path smoothing); per-instance overflows of rrtx_plan are
                              reported as RRTX_PARTIAL + RRTX_ST_OVERFLOW */
};

enum { RRTX_ALGO_RRT = 0,       /* rrt_01 RRT.planning :71-101 */
       RRTX_ALGO_RRT_STAR = 1,  /* rrt_04 RRT.planning :1036-1084 */
       RRTX_ALGO_INFORMED = 2,  /* rrt_07 RRT.informed_rrt_star_search :1044-1108 */
       RRTX_ALGO_DUBINS = 3,    /* rrt_05 RRT.planning :1416-1456 (RRT*-Dubins; start[2]/goal[2] = yaw) */
       RRTX_ALGO_BITSTAR = 4,   /* rrt_08 BITStar.plan :236-331 (max_iter = maxIter; rand_area = randArea) */
       RRTX_ALGO_RRT_DUBINS = 5 /* rrt_03 RRT.planning :1420-1456 (RRT with Dubins steer; poses, curvature and goal
                                   thresholds as RRTX_ALGO_DUBINS; sampler SOBOL = the 3-D point of :1545-1563) */,
       RRTX_ALGO_RS = 6         /* rrt_06 RRT.planning :1530-1570 (RRT*-Reeds-Shepp incl. try_goal_path :1572-1582; poses,
                                   curvature, step_size and goal thresholds; node capacity 2 * max_iter + 2; the sampler is
                                   always get_random_node :1658-1666, as in the reference's loop :1539) */ };
/* rrt_09 LQRRRTStar.planning :1120-1155 (LQR-RRT*): steer = LQR rollout + resampling (rpp_lqr.h).  Reads step_size,
   goal_xy_th, expand_dis, connect_circle_dist, play_area, robot_radius, sampler and search_until_max_iter (the
   `search_until_max_iter` keyword of planning()); node capacity max_iter + 1; RRTX_ST_REF_RAISES where the reference
   raises (an LQR rollout that never reaches its target: IndexError at :1184).  Paths: rrtx_get_path; edge polylines:
   rrtx_get_polylines (regenerated from each node's edge endpoints). */
#define RRTX_ALGO_LQR_RRT_STAR 7
enum { RRTX_SAMPLER_MT = 0,     /* get_random_node        rrt_04:1132-1139 */
       RRTX_SAMPLER_SOBOL = 1   /* get_random_node_sobol  rrt_04:1142-1153 */ };

/* per-instance status bits (rrtx_get_results) */
enum { RRTX_ST_DONE = 1, RRTX_ST_PATH = 2, RRTX_ST_OVERFLOW = 4, RRTX_ST_PATH_TRUNC = 8,
       RRTX_ST_UNSUPPORTED = 16 /* a reference code path the device kernel does not restate was reached; the instance
                                   stops there instead of continuing differently.  No planner sets it in a result any
                                   more: the one such path (rrt_04 rewire visiting a MOVED node again, :1337 with :1372)
                                   is walked by the general kernel, to which rrtx_plan hands such instances over
                                   (rrtx_stats.replanned); kept as a guard */,
       RRTX_ST_REF_RAISES = 32  /* RRTX_ALGO_RS: the reference raises here (ZeroDivisionError :1183/:1207 or ValueError from
                                   math.acos/asin) inside reeds_shepp_path_planning; the instance stops, no path */,
       RRTX_ST_REF_HANGS = 64   /* RRTX_ALGO_BITSTAR, set together with RRTX_ST_OVERFLOW: the reference does not terminate on
                                   this instance.  plan() adds samples only `if iterations != 0` (rrt_08:215); when no edge
                                   ever connects (a start walled in by obstacles: every connect() fails and `continue`s past
                                   the iteration counter, :283) both queues run dry a second time with the tree, the samples
                                   and the RNG unchanged, and the same round repeats for ever.  The device proves that at the
                                   second arrival and stops the instance there */ };

/* Constructor arguments of the reference classes (rrt_04:951-1000, rrt_01:32-69). */
typedef struct rrtx_params {
  int32_t abi_version;           /* RRTX_ABI_VERSION */
  int32_t algo;                  /* RRTX_ALGO_* */
  int32_t sampler;               /* sobol_sampler (rrt_04:962) */
  int32_t goal_sample_rate;      /* rrt_04:958 */
  int32_t max_iter;              /* rrt_04:959 */
  int32_t has_play_area;         /* play_area is not None (rrt_04:981) */
  int32_t search_until_max_iter; /* rrt_04:964 */
  int32_t n_instances;           /* independent planning instances resident on the device */
  int32_t device;                /* HIP device ordinal */
  int32_t reserved_i[7];
  double start[3];               /* start [x,y,(yaw)] rrt_04:977 */
  double goal[3];                /* goal  [x,y,(yaw)] rrt_04:978 */
  double rand_min, rand_max;     /* rand_area rrt_04:979-980 */
  double expand_dis;             /* rrt_04:985 */
  double path_resolution;        /* rrt_04:986 */
  double play_area[4];           /* xmin xmax ymin ymax (rrt_04:944-949) */
  double robot_radius;           /* rrt_04:991 */
  double connect_circle_dist;    /* rrt_04:998 */
  /* RRTX_ALGO_INFORMED only: upper-left 2x2 of the rotation `c` (numpy SVD, rrt_07:1061-1068), row major, and
   * c_min = math.hypot(start - goal) (rrt_07:1054); the host computes both exactly as the reference does. */
  double informed_rot[4];
  double informed_c_min;
  /* RRTX_ALGO_DUBINS / RRTX_ALGO_RRT_DUBINS only (rrt_05:1371-1373, 1411-1413; rrt_03:1381-1383, 1416-1418) */
  double curvature, goal_yaw_th, goal_xy_th;
  /* RRTX_ALGO_RS only: step_size of the Reeds-Shepp interpolation (rrt_06:1484, :1525) */
  double step_size;
  double reserved_d[3];
} rrtx_params;

/* Aggregate counters over all instances of the last rrtx_plan(). */
typedef struct rrtx_stats {
  int64_t iterations;        /* loop iterations executed (rrt_04:1044) */
  int64_t edges_unique;      /* collision-checked edge expansions actually evaluated on the device */
  int64_t edges_ref;         /* check_collision calls the reference would have made (repeated near indices counted) */
  int64_t near_hits;         /* sum of len(near_inds) (rrt_04:1337) */
  int64_t near_unique;       /* distinct indices among them */
  int64_t rewires;           /* rrt_04:1368 successes */
  int64_t propagated;        /* nodes rewritten by propagate_cost_to_leaves (rrt_04:1379-1384) */
  int64_t scan_nodes;        /* nodes visited by nearest/near/goal scans */
  int64_t algorithmic_bytes; /* bytes this implementation's algorithm must move: RRTX_ALGO_RRT_STAR 4*n per pass over the
                                16-bit coordinate mirror (16*n per f64 pass: its nearest-query fallbacks and the other
                                algorithms) + 16 per hit gathered + 48*k + 24*M + 44; the near pass of iteration i also
                                serves the nearest query of i+1 */
  int64_t exact_rescans;     /* nearest scans re-done with exact ** 2 (tie within filter margin) */
  int64_t total_nodes;
  int64_t launches;          /* kernel launches */
  double kernel_ms;          /* HIP-event time of all planner-kernel launches on the handle's stream */
  double plan_ms;            /* host wall time of rrtx_plan */
  int64_t algorithmic_bytes_two_scan; /* SURVEY.md 8d formula as written: 32*n + 48*k + 24*M + 28 per accepted iteration */
  int64_t near_unique_max;   /* largest number of distinct near candidates any iteration of any instance produced */
  int64_t f32_fallbacks;     /* RRTX_ALGO_RRT_STAR iteration kernel: nearest queries the 16-bit stage could not decide and
                                that took the f64 pass (a saturated grid distance: the first iterations of a tree) */
  int64_t q16_fallbacks;     /* nearest queries the 16-bit first stage could not decide on grid distances (decided by a
                                second 16-bit pass that collects the candidates + their f64 coordinates) */
  /* the DOMINANT kernel alone (RRTX_ALGO_RRT_STAR with search_until_max_iter: rrt_star_kernel_v2, whose launches a
   * rocprofv3 --kernel-trace --stats summary lists separately from the final goal-search launch; the other algorithms:
   * their one planner kernel = the totals above) */
  int64_t launches_main;
  double kernel_ms_main;
  int64_t replanned;         /* instances planned a second time from their staged start state: a near set that outgrew its
                                workgroup shape's table, a polyline pool that ran out, or an rrt_04 rewire that moved a
                                node while near_inds held repeated indices (raw-list walk of the general kernel) */
  int32_t main_shape;        /* threads per workgroup (= per planning instance) of the dominant kernel as launched:
                                RRTX_ALGO_RRT_STAR iteration kernel 64 / 128 / 256 (picked from the instance count, the
                                obstacle count, the estimated near-set size and RRTX_TPB); the other planners' fixed shape */
  int32_t main_f32;          /* kept for the layout: 1 whenever the RRTX_ALGO_RRT_STAR iteration kernel ran, else 0 */
  int64_t passes_shared;     /* RRTX_ALGO_RRT_STAR iteration kernel, 64-thread shape: iterations whose near query was answered
                                by the streaming pass of an earlier iteration (the ball speculated about the sample, on which
                                steer() snaps the new node once the tree is dense; up to three iterations ride on one pass):
                                no pass of their own, 0 bytes of xq[] */
} rrtx_stats;

typedef struct rrtx_handle rrtx_handle;

/* Call order on a handle.  rrtx_create, then any setters, then rrtx_plan (or rrtx_plan_begin + rrtx_plan_step until it
 * reports 0), then the getters; then setters and plans again, as often as wanted.  Every plan starts from the staged
 * per-instance state (obstacles, start / goal, rotation, RNG state) and from nothing else: no result of an earlier plan
 * on the handle changes a later one.
 *  - Before the first completed plan, and from rrtx_plan_begin until the step that reports 0, the getters of a plan's
 *    results (tree, path, path_yaw, yaw, polylines, copy_results_device, sobol_index, trace, trace_kind), rrtx_smooth_planned
 *    and rrtx_get_smoothed_path return RRTX_E_STATE; rrtx_get_results alone is valid between steps.
 *  - From rrtx_plan_begin until the end of that plan every setter returns RRTX_E_STATE and changes nothing:
 *    rrtx_set_obstacles, rrtx_set_instance_obstacles, rrtx_set_obstacle_map, rrtx_seed_instances, rrtx_set_rng_state, rrtx_set_instance,
 *    rrtx_set_instance_rotation, rrtx_enable_trace, rrtx_set_launch_bound (a re-plan inside the plan restarts instances
 *    from the staged state, and device tables of the plan point into the obstacle table).
 *  - rrtx_plan_begin (and so rrtx_plan) while a plan is in progress is accepted: it abandons that plan -- no launch of it
 *    is in flight between two calls, its results are gone -- and begins a new one from the staged state.
 *  - rrtx_get_smoothed_path belongs to the plan that rrtx_smooth_planned smoothed: after another rrtx_plan it returns
 *    RRTX_E_STATE until rrtx_smooth_planned has run again.
 *  - Getters with a capacity: when the caller's buffers are too small they return RRTX_E_CAPACITY, write nothing into them
 *    and leave the needed size in *n_out; with every data pointer NULL they return the size and RRTX_OK. */

/* replaces RRT.__init__ (rrt_04:951-1000); allocates device state for n_instances trees of max_iter+1 nodes. */
int rrtx_create(const rrtx_params* p, rrtx_handle** out);
/* obstacle_list ctor argument (rrt_04:989): m rows of (ox, oy, size), AoS in; converted to SoA + thresholds
 * (size+robot_radius)**2 (rrt_04:1227) on the host.  Shared by all instances of the handle.  RRTX_E_STATE between
 * rrtx_plan_begin and the end of that plan, like every setter. */
int rrtx_set_obstacles(rrtx_handle* h, const double* oxyr, int32_t m);
/* Per-instance obstacle lists (a batch over many maps in one handle): offsets has n_instances + 1 entries (CSR), instance i
 * owns the rows oxyr[3*offsets[i] .. 3*offsets[i+1]) of (ox, oy, size), taken as rrtx_set_obstacles takes them.  Replaces
 * every instance's list; a later rrtx_set_obstacles puts every instance back on one shared list.  RRTX_E_INVALID (the
 * message names the instance) for offsets[0] != 0, decreasing offsets, oxyr == NULL with rows to read, an instance with
 * more than 256 obstacles (RRTX_ALGO_RS: 64); RRTX_E_STATE between rrtx_plan_begin and the end of that plan.  Workgroup
 * shapes and capacities follow the largest list; rrtx_smooth_planned smooths each path against its instance's list. */
int rrtx_set_instance_obstacles(rrtx_handle* h, const int32_t* offsets, const double* oxyr);
/* The obstacle map: any number of circles up to 2^20 for RRTX_ALGO_RRT and RRTX_ALGO_RRT_STAR (rrt_01 / rrt_02 / rrt_04) and for
 * RRTX_ALGO_RS (rrt_06, and rrt_10 with RRTX_RS_COST_PATH: see the end of this comment), shared by all instances.
 * rrtx_set_obstacles and rrtx_set_instance_obstacles keep their limits (256, RRTX_ALGO_RS 64): they
 * stage the list in the kernels' obstacle tile.  This call builds, on the device, a uniform grid over the list instead (cells
 * over the sampling square of rand_min / rand_max, about one circle per cell; a circle is listed in every cell its square
 * [ox +- rho] x [oy +- rho] overlaps, rho = |size + robot_radius| rounded up, and in a "wide" list once it would cover more than
 * 32 cells), and rrtx_plan, rrtx_plan_begin / _step and rrtx_plan_many then run a variant of the general planner kernel that
 * refills its tile, for every group of edges, from the cells the group's bounding box covers.  The verdict of check_collision
 * is "any circle hit", so trees, paths, results, trace, RNG state, Sobol index and the decision counters of rrtx_stats are those
 * of a plan that tested every circle; rrtx_stats.algorithmic_bytes counts the records the gathers read, main_shape is the general
 * kernel's.  m <= 256 is allowed.  A later rrtx_set_obstacles or rrtx_set_instance_obstacles drops the map and returns the
 * handle to the tile; a map cannot be combined with per-instance lists.
 * RRTX_E_INVALID (the message names which) for a NULL handle, oxyr == NULL with m > 0, m < 0 or m > 2^20, an entry that is not
 * finite, and a handle of another algo; RRTX_E_STATE between rrtx_plan_begin and the end of that plan; all of them before any
 * device call.  A failure leaves the handle, and the map or lists it holds, as they were.
 * Not served while the handle holds a map (RRTX_E_STATE, the message names the map): rrtx_smooth_planned and rrtx_query_goals,
 * which read the obstacle table.  Test knobs: RRTX_OBSMAP_CELLS (cells per axis; 1 = every box streams the whole list),
 * RRTX_OBSMAP_TILE (records per tile, below 256).
 * RRTX_ALGO_RS: the same grid (its geometry is the sampling square's; Reeds-Shepp arcs that leave the square and circles that
 * lie outside it fall into the edge cells, which the rules cover).  The planner kernel has no tile to refill: every point of an
 * edge asks the grid "does any circle hold this point" from the run of its own cell and the wide list, which is the verdict
 * of rrt_06's check_collision :1748-1762.  rrtx_track_planned and rrtx_track_goals then test their roll-outs against the map
 * as well; RRTX_OBSMAP_TILE is not read. */
int rrtx_set_obstacle_map(rrtx_handle* h, const double* oxyr, int64_t m);
typedef struct rrtx_obstacle_map_info {
  double x0, y0, cell;   /* origin of the grid and side of a cell */
  int32_t nx, ny;        /* cells per axis */
  int64_t n_circles;     /* m */
  int64_t n_items;       /* records in the cells (a circle counts once per cell it is listed in) */
  int64_t n_wide;        /* circles in the wide list */
  double build_ms;       /* device time of the three build kernels */
} rrtx_obstacle_map_info;
/* one record of the map, 32 bytes: the circle, its threshold (size + robot_radius) ** 2 and its row in the caller's list */
typedef struct rrtx_obstacle_item {
  double ox, oy, thr;
  int64_t index;
} rrtx_obstacle_item;
/* RRTX_E_STATE without a map */
int rrtx_get_obstacle_map_info(rrtx_handle* h, rrtx_obstacle_map_info* info);
/* The map as built: cell_start[nx * ny + 1] (CSR over the cells, row-major: cell = cy * nx + cx), the n_items records of the
 * cells (a cell's records are contiguous and in ascending `index`) and the n_wide records of the wide list (ascending
 * `index`).  Any pointer may be NULL; RRTX_E_CAPACITY when a buffer is smaller than the info says; RRTX_E_STATE without a map. */
int rrtx_get_obstacle_map(rrtx_handle* h, int32_t* cell_start, rrtx_obstacle_item* items, int64_t cap_items,
                          rrtx_obstacle_item* wide, int64_t cap_wide);
/* hand over / take back CPython's `random.getstate()[1]` (624 words + position) for one instance, so that
 * the device consumes the stream exactly as random.randint / random.uniform would (rrt_04:1133-1136). */
int rrtx_set_rng_state(rrtx_handle* h, int32_t instance, const uint32_t* mt624, int32_t pos);
/* Before the first completed plan: the staged state.  After a plan: the state that plan (and rrtx_smooth_planned after it)
 * left on the device -- also when a new state has been staged since with rrtx_set_rng_state / rrtx_seed_instances: a staged
 * state is what the NEXT plan starts from, and cannot be read back before that plan has run.  To continue an instance's
 * stream over two plans (the reference's planning() called twice without reseeding), read the state after the first plan
 * and stage it with rrtx_set_rng_state: without that, the next plan starts from the state staged last, not from where
 * the previous plan stopped. */
int rrtx_get_rng_state(rrtx_handle* h, int32_t instance, uint32_t* mt624, int32_t* pos);
/* convenience: state after `random.seed(seed)` for instances first..first+count-1 */
int rrtx_seed_instances(rrtx_handle* h, int32_t first, int32_t count, const uint64_t* seeds);
/* per-instance start / goal for batches (default: the ctor's): x, y and, for the pose planners (RRTX_ALGO_DUBINS /
 * _RRT_DUBINS / _RS), yaw in element 2 (rrt_05:1406-1407, rrt_06:1518-1519).  Either pointer may be NULL. */
int rrtx_set_instance(rrtx_handle* h, int32_t instance, const double* start3, const double* goal3);
/* Per-instance rotation `C` (upper-left 2x2, row major) and c_min, computed by the host with numpy exactly as the
 * reference does for that instance's start / goal (default: the ctor's informed_rot / informed_c_min):
 * RRTX_ALGO_BITSTAR cMin = hypot(start-goal)/1.5 and C of rrt_08:189-202; RRTX_ALGO_INFORMED c_min = hypot(start-goal)
 * and C of rrt_07:1054-1068 (the ellipse centre follows rrtx_set_instance). */
int rrtx_set_instance_rotation(rrtx_handle* h, int32_t instance, const double* rot4, double c_min);
/* replaces the body of RRT.planning(animation=False) for every instance; blocking.  Returns RRTX_OK, RRTX_PARTIAL
 * (see above) or a negative error. */
int rrtx_plan(rrtx_handle* h);
/* The same plan in BOUNDED launches (load balance / a service that must not wait for its slowest instance).
 * rrtx_plan_begin uploads the instances' start state; every rrtx_plan_step queues ONE kernel launch over the instances that
 * are not finished, waits for it and reports in *n_pending how many instances still need another launch (0 = the plan is
 * complete: the step that reaches 0 also runs the overflow re-plans and returns what rrtx_plan would have returned).  A
 * launch is bounded by rrtx_set_launch_bound (default: RRT* iteration kernel 131072 iterations, the other tree planners
 * 32768, BIT* 20000 trips of plan()'s loop :243): an instance that has used its share stores its state on the device and is
 * carried into the next launch -- results do not depend on the bound.  Between steps rrtx_get_results is valid: an instance
 * with RRTX_ST_DONE in its status word is final, whatever the others still do.  A negative return from rrtx_plan_step
 * ends the plan: its results are not valid (the getters return RRTX_E_STATE).  rrtx_plan = begin + steps until 0.
 * BIT* launches run persistent waves over a device-side work queue of the pending instances (rrt_bitstar_wave.hip.h). */
int rrtx_plan_begin(rrtx_handle* h);
int rrtx_plan_step(rrtx_handle* h, int32_t* n_pending);
/* iterations (BIT*: loop trips) one launch may spend on one instance; RRTX_E_STATE while a plan is in progress.  The
 * one-lane BIT* kernel (problems whose vertex state exceeds LDS, RRTX_BITSTAR=lane) is not bounded: its plan is one launch. */
int rrtx_set_launch_bound(rrtx_handle* h, int32_t iterations);
/* Multi-GPU in one process ("one handle per device, driven from one process with N threads"): plans the n
 * handles concurrently, one host thread per handle (each bound to its handle's device; two handles may share a device),
 * and returns when all have finished.  rcs[i] (may be NULL) = what rrtx_plan(handles[i]) returned; the return value is
 * the most severe of them (a negative error, else RRTX_PARTIAL, else RRTX_OK).  Instances are independent, so sharding a
 * batch over handles changes no result: instance j of handle i is the instance it would be in one large handle with the
 * same seed / start / goal.  The handles must be distinct. */
int rrtx_plan_many(rrtx_handle** handles, int32_t n, int32_t* rcs);
/* Multi-GPU with one process per GPU, without any host framework: the ONE collective of the path -- an ncclAllGather of the
 * 16-byte result records {f64 path_cost, i32 n_nodes, i32 status}, device to device over RCCL / xGMI.  RCCL is
 * opened with dlopen at first use (librrtx.so does not link it).  rank 0 calls rrtx_rccl_unique_id and hands the 128 bytes to
 * the other ranks by the host's own means (a file, MPI, a torch store); every rank calls rrtx_rccl_init on its handle (same
 * n_instances on every rank), plans, then rrtx_rccl_gather_results: world * n_instances entries, rank-major -- the table
 * rrtx_get_results gives for one rank, for all of them.  No reference counterpart (the reference is one process). */
int rrtx_rccl_unique_id(void* id128);
int rrtx_rccl_init(rrtx_handle* h, const void* id128, int32_t rank, int32_t world);
int rrtx_rccl_gather_results(rrtx_handle* h, double* path_cost, int32_t* n_nodes, int32_t* status);
/* rrt.node_list as SoA: x, y, cost (f64), parent (i32, -1 = None); any pointer may be NULL. */
int rrtx_get_tree(rrtx_handle* h, int32_t instance, double* x, double* y, double* cost, int32_t* parent,
                  int32_t cap, int32_t* n_out);
/* return value of planning(): n_out points [x,y] goal -> start (rrt_04:1117-1125); n_out = 0 <=> None. */
int rrtx_get_path(rrtx_handle* h, int32_t instance, double* xy, int32_t cap_points, int32_t* n_out);
/* per-instance result table {path_cost = get_path_length(path) (rrt_04:1391-1399), n_nodes, status};
 * this 16-byte record is what multi-GPU runs gather over RCCL. */
int rrtx_get_results(rrtx_handle* h, double* path_cost, int32_t* n_nodes, int32_t* status);
/* device pointer + byte size of the packed result table (n_instances x {f64 cost, i32 n, i32 status}) */
int rrtx_results_device_ptr(rrtx_handle* h, void** dptr, int64_t* bytes);
/* the same table copied device -> device into a caller-owned device buffer (e.g. the tensor an RCCL all_gather sends):
 * no round trip through host memory; `bytes` = capacity of dst_device (>= 16 * n_instances) */
int rrtx_copy_results_device(rrtx_handle* h, void* dst_device, int64_t bytes);
/* RRTX_ALGO_DUBINS: node yaw (rrt_05 Node.yaw) and the stored edge polylines (Node.path_x / path_y, :1472-1474):
 * plen[i] points per node, concatenated in node order into px/py. */
int rrtx_get_yaw(rrtx_handle* h, int32_t instance, double* yaw, int32_t cap);
/* RRTX_ALGO_RS: third column of generate_final_course (rrt_06:1643-1651), same points as rrtx_get_path */
int rrtx_get_path_yaw(rrtx_handle* h, int32_t instance, double* yaw, int32_t cap_points, int32_t* n_out);
int rrtx_get_polylines(rrtx_handle* h, int32_t instance, int32_t* plen, int32_t cap_nodes, double* px, double* py,
                       int64_t cap_points, int64_t* n_points_out);
/* Sobol index (RRT.sobol_inter_, rrt_04:995,1148) after planning.  Every plan restarts the sequence at index 0, as a newly
 * constructed reference planner does: the index is not carried from one plan on the handle to the next and cannot be staged. */
int rrtx_get_sobol_index(rrtx_handle* h, int32_t instance, int64_t* index);
int rrtx_get_stats(rrtx_handle* h, rrtx_stats* st);
/* optional per-iteration trace of one instance (debug/parity harness): call before rrtx_plan; instance -1 switches it off.
 * The trace getters return the rows of the instance that the last completed plan traced: after rrtx_enable_trace on a
 * planned handle (another instance, or the first time) they return RRTX_E_STATE until the next plan has completed.
 * rows: rnd_x, rnd_y (f64), nearest, n_near_unique (i32; -1 when the iteration stopped before the near query) */
int rrtx_enable_trace(rrtx_handle* h, int32_t instance);
int rrtx_get_trace(rrtx_handle* h, double* rnd_x, double* rnd_y, int32_t* nearest, int32_t* n_near,
                   int32_t cap, int32_t* n_out);
/* RRTX_ALGO_RRT / RRTX_ALGO_RRT_STAR, same rows: what the iteration appended -- 0 nothing, 1 the extension edge itself
 * (rrt_01:85-96; rrt_04:1066-1067, choose_parent returned None), 2 a node under a chosen parent (rrt_04:1062-1065).  With
 * rnd / nearest this lets the host rebuild Node.path_x / path_y exactly as the reference holds them (draw data). */
int rrtx_get_trace_kind(rrtx_handle* h, int32_t* kind, int32_t cap, int32_t* n_out);
/* RRTX_ALGO_RRT_STAR with search_until_max_iter (the iteration kernel): samples first .. first + count - 1 of the stream the
 * last plan drew for `instance` before its first launch, out_xy[2 k] = x, out_xy[2 k + 1] = y of sample first + k; sample i
 * is the one iteration i consumed (parity harness).  first + count <= max_iter; RRTX_E_STATE without such a plan. */
int rrtx_get_sample_stream(rrtx_handle* h, int32_t instance, int32_t first, int32_t count, double* out_xy);
/* diagnostic builds only (-DRRTX_PHASE_TIMERS): shader-clock cycles per kernel phase summed over instances
 * (0 sample, 1 nearest scan, 2 steer, 3 extension collision, 4 near scan, 5 exact re-check + de-dup,
 *  6 choose_parent edges, 7 choose_parent costs, 8 rewire edges, 9 rewire resolve + propagate + append,
 *  11 bookkeeping, 12 goal search, 15 loop overhead; the rrt_04 iteration kernel, rrt_star_v2, keeps obstacle-cull counts in
 *  12 and 15 instead, see tools/phase_profile.py); all zero in the shipped build. */
int rrtx_get_phase_cycles(rrtx_handle* h, int64_t* out16);
const char* rrtx_last_error(rrtx_handle* h);
void rrtx_destroy(rrtx_handle* h);

/* library-level */
int rrtx_abi_version(void);
int rrtx_device_count(void);
/* Evaluate the device scalar core on arrays (parity harness for the glibc/CPython arithmetic replicas):
 * op 0: math.hypot(a,b)  1: a**2  2: math.sin(a)  3: math.cos(a)  4: math.atan2(a,b)
 * op 5: steer end x of (0,0)->(a,b) with extend=inf, res=0.25   6: sqrt(a)  7: a/b */
/* Path smoothing: replaces path_smoothing(path, max_iter, obstacle_list) (rrt_04:1447-1479; get_path_length :1391,
 * get_target_point :1401, line_collision_check :1423 -- the infinite-line distance test is kept), which every driver
 * runs right after planning() on the path it returned, drawing from the same MT19937 stream (rrt_04:1558-1559).
 *
 * rrtx_smooth_paths: a batch of polylines from the host.  Job j: path_n[j] points at paths_xy + 2*j*in_stride
 * (goal -> start order as planning() returns them), RNG state mt_words[624*j .. ], mt_pos[j] (advanced in place, so
 * random.getstate() afterwards equals the reference's); result out_n[j] points at out_xy + 2*j*out_stride;
 * status[j] = 0 ok, 1 capacity (more than 512 points / 256 obstacles), 2 the reference raises ZeroDivisionError.
 * obst_xyr = m rows (ox, oy, size) -- sizes as given, no robot radius (:1441). */
int rrtx_smooth_paths(int32_t device, int32_t n_jobs, const double* paths_xy, const int32_t* path_n, int32_t in_stride,
                      int32_t max_iter, const double* obst_xyr, int32_t m, uint32_t* mt_words, int32_t* mt_pos,
                      double* out_xy, int32_t out_stride, int32_t* out_n, int32_t* status);
/* The same on the paths a handle just planned (RRTX_ALGO_RRT / RRTX_ALGO_RRT_STAR), entirely on the device: every
 * instance's path is smoothed continuing that instance's RNG stream (rrtx_get_rng_state afterwards = after smoothing). */
int rrtx_smooth_planned(rrtx_handle* h, int32_t max_iter);
int rrtx_get_smoothed_path(rrtx_handle* h, int32_t instance, double* xy, int32_t cap_points, int32_t* n_out);

/* ---- every course of the batch in one gather on the device (csrc/course_gather.hip.h, csrc/rpp_course.h) ------------------
 * rrtx_get_path, rrtx_get_path_yaw and rrtx_get_smoothed_path serve one instance per call.  rrtx_gather_courses builds the
 * courses of ALL instances on the device as one CSR result -- offsets (n_instances + 1) into flat x, y (and yaw) -- with two
 * kernel launches and a number of host <-> device copies that depends neither on the batch size nor on the depth of a
 * tree; the getters below fetch it in one copy per column, and rrtx_tracker_run_from reads it where it lies
 * (RRTX_SRC_PLANNER).  Every double is the one the per-instance getters return.
 * which: RRTX_COURSE_PLANNED for every planner rrtx_get_path serves (a path the plan marked RRTX_ST_PATH_TRUNC is walked up
 * the parent array on the device); RRTX_COURSE_SMOOTHED needs a completed rrtx_smooth_planned since the plan.  An instance
 * without RRTX_ST_PATH owns no points.  Only RRTX_ALGO_RS planned courses have a yaw column.
 * The buffers live on the handle and are reused (they grow, never shrink); every completed gather increments the
 * generation (0 before the first).  More than 2^28 points in all: RRTX_E_CAPACITY.
 * Checked before any launch: RRTX_E_INVALID for a NULL handle or an unknown which / order; RRTX_E_STATE without a
 * completed plan, between rrtx_plan_begin and the end of that plan, and for RRTX_COURSE_SMOOTHED without a smoothing run.
 * A new plan (for RRTX_COURSE_SMOOTHED also a new smoothing run) invalidates the gathered courses: the two getters then
 * return RRTX_E_STATE until the next gather. */
#define RRTX_COURSE_PLANNED 0    /* what rrtx_get_path (+ rrtx_get_path_yaw for RRTX_ALGO_RS) returns */
#define RRTX_COURSE_SMOOTHED 1   /* what rrtx_get_smoothed_path returns */
#define RRTX_ORDER_PLANNING 0    /* goal -> start, as planning() returns it */
#define RRTX_ORDER_DRIVING 1     /* the same rows reversed */
int rrtx_gather_courses(rrtx_handle* h, int32_t which, int32_t order);
/* Of the last gather: offsets (n_instances + 1 entries, may be NULL), the point count, whether there is a yaw column, the
 * HIP-event time of the two kernels; any pointer may be NULL. */
int rrtx_get_course_counts(rrtx_handle* h, int64_t* offsets, int64_t* n_points, int32_t* has_yaw, double* kernel_ms);
/* The flat columns of the last gather (cap = doubles available in each; RRTX_E_CAPACITY when too small); any pointer may be
 * NULL, and yaw must be NULL when the gather has no yaw column (RRTX_E_STATE otherwise). */
int rrtx_get_courses(rrtx_handle* h, double* x, double* y, double* yaw, int64_t cap);
int rrtx_get_course_generation(rrtx_handle* h, uint64_t* generation);

/* ---- the best path to many goals from the planned trees (csrc/goal_query.hip.h, csrc/rpp_goalq.h) ----------------------
 * After a plan every node of a tree carries the cost of the best known route from the instance's start.  rrtx_query_goals
 * asks every instance's finished tree for the path to n_goals goals: for instance i and goal g the answer is what the tail
 * of the reference's planning() computes on that tree with self.end (rrt_04: and self.goal_node) replaced by g --
 *   RRTX_ALGO_RRT_STAR         search_best_goal_node rrt_04:1284-1312 + generate_final_course :1117-1125; node 0 can answer
 *   RRTX_ALGO_DUBINS / _RS     search_best_goal_node rrt_05:1691-1712 / rrt_06:1815-1836 with `if last_index:` (node 0 is
 *                              no answer) + generate_final_course rrt_05:1512-1521 / rrt_06:1643-1651 (RS: a yaw column)
 * bit for bit.  Nothing of the plan changes: tree, RNG state, goal, path, results and the gathered courses of
 * rrtx_gather_courses stay what they are.  Every other algo (RRTX_ALGO_RS with RRTX_RS_COST_PATH, rrt_10, included: its
 * goal rule is get_goal_indexes): RRTX_E_INVALID.
 * goals: rows (x, y, yaw), n_goals of them shared by all instances (per_instance = 0) or n_instances * n_goals, instance
 * major (per_instance = 1); any double is accepted (NaN and +-inf find nothing).  xy_th / yaw_th: the pose planners'
 * goal_xy_th / goal_yaw_th for this call; NaN = the handle's own.  Queries are (instance, goal) pairs in row-major order.
 * Returns RRTX_OK, or RRTX_PARTIAL when a query has RRTX_GOALQ_OVERFLOW (more than 512 distinct candidates inside
 * expand_dis of the goal: that query has no node, every other query is answered).  Checked before any HIP call:
 * RRTX_E_INVALID for a NULL handle / goals, an unserved algo, n_goals < 1, per_instance not 0 / 1, more than
 * RRTX_GOALQ_MAX_QUERIES queries; RRTX_E_STATE without a completed plan or while one is in progress.  A new plan drops the
 * answers: the getters return RRTX_E_STATE, rrtx_gather_goal_courses RRTX_E_INVALID, until the next query. */
#define RRTX_GOALQ_OK 0        /* node >= 0, cost = the answer's key */
#define RRTX_GOALQ_NONE 1      /* the reference finds no path to this goal on this tree */
#define RRTX_GOALQ_NO_TREE 2   /* the instance is not RRTX_ST_DONE or carries RRTX_ST_OVERFLOW / _UNSUPPORTED / _REF_RAISES */
#define RRTX_GOALQ_OVERFLOW 3
#define RRTX_GOALQ_MAX_QUERIES (1 << 24)
int rrtx_query_goals(rrtx_handle* h, int32_t n_goals, int32_t per_instance, const double* goals, double xy_th, double yaw_th);
/* The records of the last query, n_instances * n_goals of each: the answer node (-1 none), its cost (rrt_04: cost +
 * distance to the goal; +inf without a node), the number of distinct candidates, of safe ones (rrt_04; else 0), the status.
 * Any pointer may be NULL; with all five NULL only *n_queries is written.  cap = entries available in each. */
int rrtx_get_goal_query(rrtx_handle* h, int32_t* node, double* cost, int32_t* n_near, int32_t* n_safe, int32_t* status,
                        int64_t cap, int64_t* n_queries);
/* The courses of the last query as one CSR result over the queries, in RRTX_ORDER_PLANNING (goal -> start) or _DRIVING:
 * count, the host's exclusive sum, gather -- the pattern and the limits of rrtx_gather_courses, in buffers of their own. */
int rrtx_gather_goal_courses(rrtx_handle* h, int32_t order);
/* offsets: n_instances * n_goals + 1 entries */
int rrtx_get_goal_course_counts(rrtx_handle* h, int64_t* offsets, int64_t* n_points, int32_t* has_yaw);
int rrtx_get_goal_courses(rrtx_handle* h, double* x, double* y, double* yaw, int64_t cap);
/* HIP-event time of the last query's solve launch and of its last gather's two launches (0 without a gather) */
int rrtx_get_goal_query_kernel_ms(rrtx_handle* h, double* solve_ms, double* gather_ms);

/* ---- closed-loop RRT* (rrt_10 = 10_path_planning_01_rrt_10_closed_loop_rrt_star.py) -----------------------------------
 * Tree phase: RRTX_ALGO_RS with expand_dis = +inf (rrt_10's class has no expand_dis attribute, so find_near_nodes
 * :522-531 does not clamp its radius) and rrtx_set_rs_cost(h, RRTX_RS_COST_PATH): rrt_10's RRTStarReedsShepp inherits
 * choose_parent / rewire / propagate_cost_to_leaves from RRTStar and they call ITS calc_new_cost (:1153-1161, the
 * Reeds-Shepp length), where rrt_06's single class ends up with the Euclidean one defined last.
 * Closed-loop stage: rrtx_track_planned after a plan of RRTX_ALGO_RS (either cost), entirely on the device
 * (csrc/rrt_track.hip.h).  Valid again after every re-plan; the getters refer to the last rrtx_track_planned. */
#define RRTX_RS_COST_EUCLID 0
#define RRTX_RS_COST_PATH 1
/* which of the tests of check_tracking_path_is_feasible (:1542-1562) refused a candidate */
#define RRTX_TRACK_FAIL_REACH 1
#define RRTX_TRACK_FAIL_ANGLE 2
#define RRTX_TRACK_FAIL_LONG 4
#define RRTX_TRACK_FAIL_COLLISION 8
typedef struct rrtx_track_params {
  double target_speed, yaw_th, xy_th, invalid_travel_ratio;              /* ClosedLoopRRTStar.__init__ :1458-1476 */
  double dt, L, steer_max, accel_max, Kp, Lf, T, goal_dis, stop_speed;   /* module globals :1592-1607; steer_max <= 0.79 */
} rrtx_track_params;
typedef struct rrtx_track_outcome {
  int32_t flag;      /* a feasible roll-out exists (the first element of planning()'s tuple) */
  int32_t winner;    /* its position in the candidate list, -1 none */
  int32_t n_cand;    /* len(get_goal_indexes()) */
  int32_t len;       /* len(t) of the winner; x / y / yaw hold len + 1 values (goal pose appended, :1519-1521) */
  int32_t node;      /* the winner's node index, -1 none */
  int32_t status;    /* 0, RRTX_ST_OVERFLOW (a course longer than 960 points), RRTX_ST_REF_RAISES (the reference raises:
                        a candidate course of fewer than 3 points, :1435) or RRTX_ST_UNSUPPORTED (tan outside the replica's
                        domain); with any of them set the instance reports no winner */
} rrtx_track_outcome;
typedef struct rrtx_track_record {   /* what check_tracking_path_is_feasible returned for one candidate */
  int32_t find_goal, len, fail, ood;
  double t_last;
} rrtx_track_record;
int rrtx_set_rs_cost(rrtx_handle* h, int32_t mode);
int rrtx_track_planned(rrtx_handle* h, const rrtx_track_params* tp);
int rrtx_get_track_outcome(rrtx_handle* h, int32_t instance, rrtx_track_outcome* out);
/* x, y, yaw: len + 1 doubles each; v, t, a, d: len doubles each (cap = doubles available in every array) */
int rrtx_get_track_arrays(rrtx_handle* h, int32_t instance, double* x, double* y, double* yaw, double* v, double* t,
                          double* a, double* d, int32_t cap);
/* candidate node indices and their records, n_cand of each */
int rrtx_get_track_records(rrtx_handle* h, int32_t instance, int32_t* cand, rrtx_track_record* rec, int32_t cap);
/* HIP-event time of the kernels of the last rrtx_track_planned, and the roll-out steps they ran (both launches) */
int rrtx_get_track_stats(rrtx_handle* h, double* kernel_ms, int64_t* steps);

/* ---- the closed-loop stage for MANY goals from the planned trees (csrc/goal_track.hip.h, csrc/rpp_goaltrack.h) ---------------
 * After a plan of RRTX_ALGO_RS (either cost): for every instance i and goal g = (x, y, yaw) what
 *   path_indexs = self.get_goal_indexes(); self.search_best_feasible_path(path_indexs)          (rrt_10 :1488-1493)
 * returns on i's finished node_list with self.end = Node(*g) and tp's tracking parameters (xy_th / yaw_th select the
 * candidates): candidates in ascending node index, each one's course (start pose, polylines root -> candidate, g) rolled out
 * towards g against the instance's own obstacle rows, the feasible roll-out with the smallest t[-1] wins, the later candidate
 * among equal times.  A goal is any double; one with a NaN or an infinity finds no candidate.  Nothing of the plan changes, and
 * neither do the answers of rrtx_track_planned or rrtx_query_goals; the buffers are this call's own.
 * Queries are (instance, goal) pairs, row major; `goals` is (n_goals, 3) shared (per_instance = 0) or (n_instances, n_goals, 3).
 * A query with a refused candidate has no winner and carries the status bit (as rrtx_track_outcome.status); its records stay
 * readable.  An instance whose tree did not finish (RRTX_GOALQ_NO_TREE's condition) answers no_tree = 1.
 * Returns RRTX_OK, or RRTX_PARTIAL when some query carries a status.  Checked in this order before any device call:
 * RRTX_E_INVALID for a NULL handle / tp / goals, n_goals < 1, per_instance not 0 / 1, more than RRTX_GOALQ_MAX_QUERIES queries
 * or track parameters rrtx_track_planned refuses; RRTX_E_STATE for another algo, without a completed plan or while one is in
 * progress.  RRTX_E_CAPACITY for more than 2^24 candidates in all.  A new plan drops the answers (getters: RRTX_E_STATE).
 * Launches and copies per call do not depend on the number of instances, goals, candidates or on the depth of a tree. */
typedef struct rrtx_goal_track_outcome {
  int32_t flag;      /* a feasible roll-out exists (the first element of the tuple) */
  int32_t winner;    /* its position in the query's candidate list, -1 none */
  int32_t n_cand;    /* len(get_goal_indexes()) */
  int32_t len;       /* len(t) of the winner; x / y / yaw hold len + 1 values (goal pose appended, :1519-1521) */
  int32_t node;      /* the winner's node index, -1 none */
  int32_t status;    /* 0, or RRTX_ST_OVERFLOW / RRTX_ST_REF_RAISES / RRTX_ST_UNSUPPORTED as rrtx_track_outcome.status */
  int32_t no_tree;   /* 1: the instance's tree did not finish, nothing was asked of it */
  int32_t reserved;
  double t_last;     /* t[-1] of the winner, +inf without one */
} rrtx_goal_track_outcome;
/* want_arrays = 0: records and outcomes only (no store launch; rrtx_get_goal_track_arrays then returns RRTX_E_STATE) */
int rrtx_track_goals(rrtx_handle* h, const rrtx_track_params* tp, int32_t n_goals, int32_t per_instance, const double* goals,
                     int32_t want_arrays);
/* out: one outcome per query; cand_offsets: n_queries + 1 entries into the candidate records; arr_offsets: n_queries + 1,
 * the exclusive sum of len + 1 over the queries with a flag (cap = queries the buffers hold; NULL buffers are skipped).
 * n_steps = arr_offsets[n_queries]. */
int rrtx_get_goal_track(rrtx_handle* h, rrtx_goal_track_outcome* out, int64_t* cand_offsets, int64_t* arr_offsets, int64_t cap,
                        int64_t* n_queries, int64_t* n_candidates, int64_t* n_steps);
/* candidate node indices and their records, n_candidates of each, query after query */
int rrtx_get_goal_track_records(rrtx_handle* h, int32_t* cand_node, rrtx_track_record* rec, int64_t cap);
/* n_steps doubles each: a flagged query owns len + 1 entries at its arr_offset; x, y, yaw fill them (the goal pose last),
 * v, t, a, d fill len and leave the last one NaN */
int rrtx_get_goal_track_arrays(rrtx_handle* h, double* x, double* y, double* yaw, double* v, double* t, double* a, double* d,
                               int64_t cap);
/* RRTX_ALGO_RS: the yaw column of the stored edge polylines (Node.path_yaw), the points of rrtx_get_polylines in its order */
int rrtx_get_polyline_yaw(rrtx_handle* h, int32_t instance, double* pyaw, int64_t cap_points);
/* HIP-event times of the last call: the two candidate launches, roll + pick, and the store launch (0 without one) */
int rrtx_get_goal_track_kernel_ms(rrtx_handle* h, double* list_ms, double* roll_ms, double* store_ms);

/* ---- batched Dubins / Reeds-Shepp curves between pose pairs, without a planner (csrc/steer_batch.hip.h) -------------------
 * Replaces plan_dubins_path (10_path_planning_00_dubins_path.py :109-197) and reeds_shepp_path_planning
 * (10_path_planning_00_reeds_shepp_path.py :506-515) called once per pair: every double is the reference's, bit for bit.
 * (The LQR steer, the reference's third, is served by the same object: rrtx_steer_solve_lqr below; so are Bezier curves,
 * the fourth way of joining two poses: rrtx_steer_solve_bezier and rrtx_steer_solve_bezier_cp further below.)
 * The steer object is independent of rrtx_handle; it owns the device buffers of its solves and reuses them from call to
 * call (they grow, never shrink).  One host thread per object.  Call order: create, then solve, then the getters of that
 * solve, then solve again, as often as wanted; a getter before the first solve returns RRTX_E_STATE. */
typedef struct rrtx_steer rrtx_steer;
#define RRTX_STEER_DUBINS 0
#define RRTX_STEER_RS 1
/* per-pair status */
#define RRTX_STEER_OK 0
#define RRTX_STEER_NO_PATH 1          /* RS: the reference returns (None,) * 5; Dubins: no word of the list is feasible */
#define RRTX_STEER_RAISES_ZERODIV 2   /* RS: the reference raises ZeroDivisionError */
#define RRTX_STEER_RAISES_VALUE 3     /* RS: the reference raises ValueError (math.asin) */
/* A steer object on HIP device `device`.  Without a usable gfx950 device the return value is RRTX_E_NO_DEVICE and *out is
 * still an object (to be destroyed like any other): its solves check their arguments and then return RRTX_E_NO_DEVICE. */
int rrtx_steer_create(int32_t device, rrtx_steer** out);
void rrtx_steer_destroy(rrtx_steer* s);
/* The message of the last call on `s` that failed; for s == NULL the last failure of a steer call of this thread that had no object. */
const char* rrtx_steer_last_error(rrtx_steer* s);
/* Solves a batch.  product == 0: n pairs, pair p = (starts[p], goals[p]); ng is not read.  product == 1: the n * ng pairs
 * of n starts and ng goals, pair p = (starts[p / ng], goals[p % ng]), formed on the device.  Poses are rows (x, y, yaw).
 * curvature: one value (curvature_per_pair == 0) or one per pair.  step_size: RS as the reference takes it; Dubins
 * interpolates at the reference's default 0.1 and refuses any other value.  word_order (Dubins only, else NULL):
 * selected_types as an ordered list of n_words (0..6) indices into LSL, RSR, LSR, RSL, RLR, LRL -- the first of equal
 * lengths wins, in list order; NULL = all six in that order.  want_points == 0: lengths only (the fast path; no
 * polyline, no offsets).
 * Returns RRTX_OK, or RRTX_PARTIAL when some pair's status is not RRTX_STEER_OK (the other pairs are complete).
 * RRTX_E_INVALID, before any HIP call: a NULL pointer, n < 0 (product: ng < 0), more than 2^30 pairs, an unknown kind,
 * step_size <= 0, a Dubins step_size != 0.1, n_words outside 0..6 or a word index outside 0..5, a word order with RS, a pose
 * or curvature that is not finite, |x|, |y| or |yaw| above 1e6, a curvature <= 0, or poses so far apart for the
 * curvature and step that one curve could exceed 2^22 points. */
int rrtx_steer_solve(rrtx_steer* s, int32_t kind, int32_t product, int64_t n, int64_t ng, const double* starts,
                     const double* goals, const double* curvature, int32_t curvature_per_pair, double step_size,
                     const int32_t* word_order, int32_t n_words, int32_t want_points);
/* Pairs of the last solve, and its polyline points in all (0 after a lengths-only solve). */
int rrtx_steer_get_counts(rrtx_steer* s, int64_t* n_pairs, int64_t* n_points);
/* Per pair of the last solve; any pointer may be NULL.  length: the curve's length, the absolute values of
 * its seg_len entries added up in segment order; seg_len: rows of 5 (n_seg used, lengths as the reference returns them, i.e. divided by the
 * curvature); modes: rows of 8 chars, the mode letters NUL padded; offsets: n_pairs + 1 entries (CSR: pair p owns the points
 * offsets[p] .. offsets[p + 1] - 1; a pair without a path owns none) -- RRTX_E_STATE after a lengths-only solve. */
int rrtx_steer_get_summary(rrtx_steer* s, int32_t* status, double* length, int32_t* n_seg, double* seg_len, char* modes,
                           int64_t* offsets);
/* The flat x, y, yaw arrays of the last solve (cap = doubles available in each; RRTX_E_CAPACITY when too small); a Bezier
 * solve has the curvature beside them: rrtx_steer_get_curvature. */
int rrtx_steer_get_points(rrtx_steer* s, double* x, double* y, double* yaw, int64_t cap);
/* HIP-event time of the kernels of the last solve (both stages, the obstacle check included; the prefix sum between them is
 * not kernel time) */
int rrtx_steer_get_kernel_ms(rrtx_steer* s, double* kernel_ms);
/* The obstacle list every later solve on `s` tests its curves against, until it is set again: m rows (x, y, size), copied
 * (the caller's array need not outlive the call), any m up to 2^20 -- the planners' obstacle limits do not apply here.
 * m == 0 turns the check off.  The test is check_collision of the pose planners (rrt_05:1625-1638, rrt_06:1749-1762) on the
 * curve's own points: for each obstacle in list order, min over the points of dx * dx + dy * dy <= (size + robot_radius) ** 2.
 * A negative size is accepted (the reference squares it).  With a list set, a solve with want_points == 0 still computes
 * every point on the device, but stores none: no point arrays and no offsets exist afterwards.
 * RRTX_E_INVALID, before any HIP call: s NULL, m < 0, m > 2^20, obstacles NULL with m > 0, an entry or robot_radius that is
 * not finite. */
int rrtx_steer_set_obstacles(rrtx_steer* s, const double* obstacles, int64_t m, double robot_radius);
/* Per pair of the last solve: -1 the reference's check_collision returns True for the pair's curve (free); j >= 0 the index
 * of the obstacle at which its loop returns False (the lowest index any point of the curve touches); -2 the pair has no
 * curve (status != RRTX_STEER_OK), nothing was tested.  RRTX_E_STATE before the first solve and when the last solve ran
 * with no obstacle list set. */
int rrtx_steer_get_hits(rrtx_steer* s, int32_t* hit);
/* ---- the obstacle index of the curve objects (csrc/rpp_obsgrid.h point_first_hit) ----------------------------------------------
 * rrtx_steer_*, rrtx_spline_run and rrtx_bspline_run / _approximate test every curve point against the obstacle list.  The
 * linear loop reads all m rows per point; the index is the uniform grid of rrtx_set_obstacle_map built over the list itself
 * (the box of the circle centres, about one circle per cell, the same build kernels), and a point then reads the run of its
 * own cell and the wide list only.  Every run is in ascending row order, so the answer is the same int32 as the linear loop's,
 * bit for bit: hits, candidates' hits and rrtx_steer_select_free's choice do not depend on the mode.
 * Mode per object: RRTX_OBSIDX_AUTO (the default) uses the index when the list has more than RRTX_OBSIDX_MIN rows, _ON always,
 * _OFF never.  The linear loop serves a list whatever the mode -- never an error -- when the list is empty, when a circle's
 * (size + robot_radius) ** 2 or reach is not finite, and when a cell or the wide list would hold more than 4096 records
 * (coincident circles; the build ranks a run with run^2 comparisons).
 * A steer object builds the index in rrtx_steer_set_obstacles (and in rrtx_steer_set_obstacle_index when the mode asks for one
 * that was not built), not per solve; setting the same rows with the same robot_radius again keeps the build.  The spline
 * objects get their list per run and build per run; equal rows and radius reuse the last build.
 * Test knob: RRTX_OBSMAP_CELLS (cells per axis), as for rrtx_set_obstacle_map. */
#define RRTX_OBSIDX_AUTO 0
#define RRTX_OBSIDX_ON 1
#define RRTX_OBSIDX_OFF 2
#define RRTX_OBSIDX_MIN 256
/* rrtx_obstacle_index_info.reason: why the list of the object is served as it is */
#define RRTX_OBSIDX_REASON_USED 0           /* the index serves it */
#define RRTX_OBSIDX_REASON_OFF 1            /* the mode is RRTX_OBSIDX_OFF */
#define RRTX_OBSIDX_REASON_BELOW 2          /* RRTX_OBSIDX_AUTO and no more than RRTX_OBSIDX_MIN rows */
#define RRTX_OBSIDX_REASON_RUN_TOO_LONG 3   /* a cell or the wide list of more than 4096 records */
#define RRTX_OBSIDX_REASON_NOT_FINITE 4     /* a threshold or reach that is not finite */
#define RRTX_OBSIDX_REASON_EMPTY 5          /* no list */
typedef struct rrtx_obstacle_index_info {
  int32_t mode;     /* RRTX_OBSIDX_* */
  int32_t used;     /* 1: the index serves the object's list, 0: the linear loop */
  int32_t reason;   /* RRTX_OBSIDX_REASON_* */
  int32_t reserved;
  rrtx_obstacle_map_info map;   /* the grid when used, zero otherwise */
} rrtx_obstacle_index_info;
/* RRTX_E_INVALID for a NULL object or a mode that is not RRTX_OBSIDX_*.  Takes effect at once for the list a steer object
 * holds, and at the next run of a spline object. */
int rrtx_steer_set_obstacle_index(rrtx_steer* s, int32_t mode);
/* For the list the object holds (steer) or the last run's list (spline objects; reason RRTX_OBSIDX_REASON_EMPTY before one) */
int rrtx_steer_get_obstacle_index_info(rrtx_steer* s, rrtx_obstacle_index_info* info);
/* The index as built, shaped like rrtx_get_obstacle_map; RRTX_E_STATE when the index does not serve the list */
int rrtx_steer_get_obstacle_index(rrtx_steer* s, int32_t* cell_start, rrtx_obstacle_item* items, int64_t cap_items,
                                  rrtx_obstacle_item* wide, int64_t cap_wide);

/* ---- every candidate curve of a pair, and the shortest one that is free (csrc/steer_batch.hip.h steer_*_all) ---------------
 * rrtx_steer_solve_all restates calc_paths (10_path_planning_00_reeds_shepp_path.py :483-503): for RRTX_STEER_RS every Path
 * that set_path :141-159 kept for the pair, in the list's order -- reeds_shepp_path_planning :506-515, which rrtx_steer_solve
 * serves, is the minimum over that list.  For RRTX_STEER_DUBINS the candidates are one per entry of the word list, in list
 * order, where the word is feasible: candidate w is what plan_dubins_path (10_path_planning_00_dubins_path.py :109-197)
 * returns with selected_types=[w], bit for bit; a word listed twice is two candidates.
 * Arguments, checks and return values are those of rrtx_steer_solve, except that the word list may hold up to 16 entries.
 * A pair whose status is not RRTX_STEER_OK has no candidates.  The result is CSR twice -- pairs -> candidates -> points -- and
 * sized from the counts; more than 2^31 - 1 candidates in all is RRTX_E_OVERFLOW.  With a list set by
 * rrtx_steer_set_obstacles every candidate is tested as rrtx_steer_solve tests the one curve.  The solve replaces the
 * result of an earlier rrtx_steer_solve* on `s` (its getters return RRTX_E_STATE until rrtx_steer_select_free or another
 * solve), and a later rrtx_steer_solve* replaces the candidates. */
int rrtx_steer_solve_all(rrtx_steer* s, int32_t kind, int32_t product, int64_t n, int64_t ng, const double* starts,
                         const double* goals, const double* curvature, int32_t curvature_per_pair, double step_size,
                         const int32_t* word_order, int32_t n_words, int32_t want_points);
/* Pairs, candidates and candidate points (0 without points) of the last rrtx_steer_solve_all and the HIP-event time of its
 * kernels; any pointer may be NULL. */
int rrtx_steer_get_cand_counts(rrtx_steer* s, int64_t* n_pairs, int64_t* n_candidates, int64_t* n_points, double* kernel_ms);
/* Any pointer may be NULL.  Per pair: status, cand_offsets (n_pairs + 1: pair p owns the candidates cand_offsets[p] ..
 * cand_offsets[p + 1] - 1).  Per candidate, in the reference's list order: pair; variant (RS: 4 * word family + symmetry of
 * generate_path :366-421, 0..47; Dubins: the position in the word list); n_seg, seg_len (rows of 5), modes (rows of 8) and
 * length as rrtx_steer_get_summary gives them for one curve (Path.lengths, Path.ctypes after :500); key: what the kind's
 * planner minimises -- RS abs(L / maxc), which is Path.L after :501; Dubins the cost of :1220 in curvature units; hit as
 * rrtx_steer_get_hits (RRTX_E_STATE without an obstacle list); offsets (n_candidates + 1) into the point arrays
 * (RRTX_E_STATE without points). */
int rrtx_steer_get_cand_summary(rrtx_steer* s, int32_t* status, int64_t* cand_offsets, int32_t* pair, int32_t* variant,
                                int32_t* n_seg, double* seg_len, char* modes, double* length, double* key, int32_t* hit,
                                int64_t* offsets);
/* The flat x, y, yaw of all candidates and Path.directions (+1 / -1 per point, interpolate :480; Dubins: all +1). */
int rrtx_steer_get_cand_points(rrtx_steer* s, double* x, double* y, double* yaw, int8_t* directions, int64_t cap);
/* After an rrtx_steer_solve_all with an obstacle list (else RRTX_E_STATE): per pair, the free candidate (hit == -1) with
 * the smallest key, the first in list order among equal keys; where no candidate is free, the same choice among all of
 * them, which is the curve of rrtx_steer_solve with its hit; a pair without candidates keeps the row rrtx_steer_solve
 * gives it.  The chosen curves become the result of `s` as if rrtx_steer_solve had found them: rrtx_steer_get_counts,
 * _get_summary, _get_points (when the candidates have points), _get_hits and _get_kernel_ms (all launches since the
 * rrtx_steer_solve_all) serve them.  chosen (the candidate's index, -1 where the pair has none), rank (the position of the
 * chosen candidate among the pair's candidates ordered by key, list order among equal keys: 0 <=> the curve of
 * rrtx_steer_solve) and n_free are (n_pairs,) arrays, any may be NULL.  Returns RRTX_OK or RRTX_PARTIAL as rrtx_steer_solve. */
int rrtx_steer_select_free(rrtx_steer* s, int32_t* chosen, int32_t* rank, int32_t* n_free);

/* ---- the third steering function on the same object: LQR rollouts between point pairs (csrc/steer_batch.hip.h, csrc/rpp_lqr.h)
 * Replaces LQRPlanner.lqr_planning (10_path_planning_00_lqr_path.py :24-66, the same lines as rrt_09 :944-986) called once per
 * pair, and rrt_09's edge around it: sample_path :1157-1172, the cost of steer :1189 / calc_new_cost :1432-1442 and
 * check_collision :1292-1305.  Every double is the reference's, bit for bit, for the reference's model (DT = 0.1, Q = R = I:
 * the gain is the constant [0, 0.05]).  It has an entry point of its own and no kind value: rrtx_steer_solve goes on refusing
 * any kind but the two above.  Rows of starts and goals are (x, y); product as for rrtx_steer_solve.
 * step_size > 0: the resampled rollout of rrt_09 -- ceil(1 / step_size) points per rollout segment, the last rollout point
 * left out; the end point is the last resampled point and the length Python's left-to-right sum of math.hypot over
 * consecutive resampled points.  step_size == 0: the raw rollout rx, ry; the end point is its last point and the length the
 * same sum over consecutive rollout points (the script returns no length: this one is this library's definition).
 * max_time, goal_dist: the planner's MAX_TIME and GOAL_DIST (100.0 and 0.1 in the reference).
 * Per-pair status: RRTX_STEER_OK, or RRTX_STEER_NO_PATH where the reference prints "Cannot found path" and returns [], [].
 * The getters above serve the result: n_seg is the number of rollout points len(rx), seg_len and modes are zero-filled,
 * offsets / points and hits as for the other kinds (with a list set by rrtx_steer_set_obstacles: -1 free, j >= 0, -2 no
 * path); a rollout has no yaw, so rrtx_steer_get_points with a non-NULL yaw returns RRTX_E_STATE after this solve.
 * Returns RRTX_OK or RRTX_PARTIAL as rrtx_steer_solve does.  RRTX_E_INVALID, before any HIP call: a NULL pointer, n < 0
 * (product: ng < 0), more than 2^30 pairs, a coordinate that is not finite or above 1e6 in magnitude, step_size NaN, negative
 * or in (0, 1e-3) (a segment has at most 1000 points), max_time NaN, negative or above 100.0 (a rollout has at most 1002
 * points), goal_dist NaN (a negative one is legal: every pair is RRTX_STEER_NO_PATH). */
int rrtx_steer_solve_lqr(rrtx_steer* s, int32_t product, int64_t n, int64_t ng, const double* starts /* (n, 2) */,
                         const double* goals /* (n or ng, 2) */, double step_size, double max_time, double goal_dist,
                         int32_t want_points);
/* The end point of every pair of the last solve, rows (x, y); zeros where the pair has no path.  RRTX_E_STATE unless the
 * last solve was rrtx_steer_solve_lqr. */
int rrtx_steer_get_ends(rrtx_steer* s, double* ends /* (n, 2) */);

/* ---- the fourth way of joining two poses on the same object: Bezier curves (csrc/steer_batch.hip.h, csrc/rpp_bezier.h) -----
 * Replaces calc_4points_bezier_path (10_path_planning_00_bazier_path.py :12-34) and calc_bezier_path :37-49 called once per
 * curve, with bezier :64-73 on the derivative control points :76-94 and curvature :97-107 at every point.  Every double of
 * the control points, the points, the derivatives and the curvature is the reference's, bit for bit (scipy.special.comb is
 * the exact binomial coefficient; no scipy is involved).  Entry points of their own and no kind value, as for LQR.
 * rrtx_steer_solve_bezier: poses are rows (x, y, yaw), product as for rrtx_steer_solve; the four control points are
 * start, start + dist * (cos, sin)(start yaw), goal - dist * (cos, sin)(goal yaw), goal with dist = hypot(start - goal) /
 * offset; offsets: one offset per pair, or NULL: offset0 for all.  A negative offset is legal, as in the reference.
 * rrtx_steer_solve_bezier_cp: n curves of m control points each, rows (x, y): calc_bezier_path for any degree m - 1.
 * Every curve has n_points points at the parameters np.linspace(0, 1, n_points) (the reference's 100).
 * This library's own definitions (the script returns none of them): yaw = atan2(dy, dx) of the first derivative; length =
 * Python's left-to-right sum of math.hypot over consecutive points; kmax = the largest |curvature| over the curve's points,
 * NaN if any is NaN (coinciding control points: a zero first derivative gives numpy's nan or inf, not an error).
 * Per-pair status is always RRTX_STEER_OK, so the return value is RRTX_OK.  The getters above serve the result: n_seg is m,
 * seg_len and modes are zero-filled, offsets[p] = p * n_points, points with yaw, hits as for the other kinds.
 * want_points == 0: length (and kmax) only; with an obstacle list set the points are computed and tested but not stored.
 * want_curvature != 0: kmax per curve, and with want_points the curvature per point.
 * RRTX_E_INVALID, before any HIP call (so also without a device): a NULL pointer, n < 0 (product: ng < 0), more than 2^30
 * pairs, n_points outside 2..4096, n * n_points above 2^28, m outside 3..16 (degree 1 makes the reference's
 * second-derivative call raise), a coordinate or yaw that is not finite or above 1e6 in magnitude, an offset that is not
 * finite or below 1e-6 in magnitude. */
int rrtx_steer_solve_bezier(rrtx_steer* s, int32_t product, int64_t n, int64_t ng, const double* starts /* (n, 3) */,
                            const double* goals /* (n or ng, 3) */, double offset0, const double* offsets /* or NULL */,
                            int32_t n_points, int32_t want_points, int32_t want_curvature);
int rrtx_steer_solve_bezier_cp(rrtx_steer* s, int64_t n, int32_t m, const double* control_points /* (n, m, 2) */,
                               int32_t n_points, int32_t want_points, int32_t want_curvature);
/* The flat curvature array of the last solve, parallel to rrtx_steer_get_points (cap as there).  RRTX_E_STATE unless the
 * last solve was a Bezier solve with want_points and want_curvature. */
int rrtx_steer_get_curvature(rrtx_steer* s, double* k, int64_t cap);
/* kmax of every curve of the last solve.  RRTX_E_STATE unless the last solve was a Bezier solve with want_curvature. */
int rrtx_steer_get_kmax(rrtx_steer* s, double* kmax /* (n,) */);
/* The control points of every curve of the last solve, as the device computed (or received) them, and their number per
 * curve; either pointer may be NULL.  RRTX_E_STATE unless the last solve was a Bezier solve. */
int rrtx_steer_get_control_points(rrtx_steer* s, double* control_points /* (n, m, 2) */, int32_t* m);

/* ---- batched closed-loop tracking of courses given as data, without a planner (csrc/rrt_track.hip.h) ----------------------
 * For every course of a batch: what ClosedLoopRRTStar.check_tracking_path_is_feasible(path) (rrt_10:1526-1564) returns,
 * every double the reference's.  A course is given in driving order (start ... goal; the reference receives it reversed),
 * its goal is its last point (:1531), and the roll-out starts at the reference's State(-0.0, -0.0, 0.0, 0.0) (:1309)
 * unless start_state is given.  The tracker is independent of rrtx_handle; it owns the device buffers of its runs and
 * reuses them from call to call (they grow, never shrink).  One host thread per object.  Call order: create, run, the
 * getters of that run, run again, as often as wanted; a getter before the first run returns RRTX_E_STATE. */
typedef struct rrtx_tracker rrtx_tracker;
/* As rrtx_steer_create: without a usable gfx950 device the return value is RRTX_E_NO_DEVICE and *out is still an object
 * (to be destroyed like any other): its runs check their arguments and then return RRTX_E_NO_DEVICE. */
int rrtx_tracker_create(int32_t device, rrtx_tracker** out);
void rrtx_tracker_destroy(rrtx_tracker* t);
/* The message of the last call on `t` that failed; for t == NULL the last failure of a tracker call of this thread that had no object. */
const char* rrtx_tracker_last_error(rrtx_tracker* t);
typedef struct rrtx_track_batch {
  int64_t n;                      /* courses */
  const int64_t* offsets;         /* n + 1, CSR into x / y / yaw, driving order */
  const double *x, *y, *yaw;
  const double* per_course;       /* NULL, or n rows (target_speed, yaw_th, invalid_travel_ratio) overriding tp's */
  const double* start_state;      /* NULL (the reference's -0.0, -0.0, 0, 0), or n rows (x, y, yaw, v) */
  const double* obstacles;        /* rows (x, y, radius) */
  const int64_t* obs_offsets;     /* NULL: one list of n_obstacles rows for every course; else n + 1 CSR entries */
  int64_t n_obstacles;
  const double* robot_radius;     /* one value, or n values when robot_radius_per_course != 0 */
  int32_t robot_radius_per_course;
  int32_t want_arrays;
} rrtx_track_batch;
/* Rolls every course out (tp->xy_th is not read).  Collision thresholds are (radius + robot_radius) ** 2, computed on the
 * host as rrtx_set_obstacles computes them.  Per course a rrtx_track_record; ood: 0 complete, 1 tan outside the replica's
 * domain, 2 the reference raises (a course of fewer than 3 points, :1435), 3 a course of more than 960 points.  With
 * want_arrays every course with ood == 0 owns len entries in each of the seven arrays (x, y, yaw, v, t, a, d as the
 * reference returns them; no goal pose is appended, that is search_best_feasible_path's doing); others own none.
 * Returns RRTX_OK, or RRTX_PARTIAL when some record has ood != 0 (every other course is complete).  n == 0 is a valid
 * empty run.  RRTX_E_INVALID, before any HIP call (also on a host without a device): a NULL pointer (obstacles may be
 * NULL when n_obstacles is 0, and x / y / yaw when the courses hold no point in all), n_obstacles < 0, n < 0 or n > 2^30,
 * offsets or obs_offsets that do not start at 0 or that decrease, obs_offsets[n] > n_obstacles, more than 2^31 - 1 points in all, a pose, obstacle,
 * radius, start state or per-course value that is not finite, more than 64 obstacles in one list (unless the tracker's
 * obstacle index is on, rrtx_tracker_set_obstacle_index below), or parameters outside
 * dt > 0, 0 <= T, T / dt <= 1e6, Lf > 0, L > 0, 0 <= steer_max <= 0.79 (as rrtx_track_planned).  After these checks a host
 * without a device gets RRTX_E_NO_DEVICE. */
int rrtx_tracker_run(rrtx_tracker* t, const rrtx_track_params* tp, const rrtx_track_batch* b);
/* Courses of the last run, and the roll-out steps (the sum of len over the courses with ood == 0). */
int rrtx_tracker_get_counts(rrtx_tracker* t, int64_t* n_courses, int64_t* n_steps);
/* rec: n_courses records; arr_offsets (may be NULL): n_courses + 1 entries, the exclusive sum of len over the courses with ood == 0 */
int rrtx_tracker_get_records(rrtx_tracker* t, rrtx_track_record* rec, int64_t* arr_offsets);
/* The seven flat arrays of the last run, n_steps doubles each; any pointer may be NULL (cap = doubles available in each;
 * RRTX_E_CAPACITY when too small).  RRTX_E_STATE after a run with want_arrays == 0. */
int rrtx_tracker_get_arrays(rrtx_tracker* t, double* x, double* y, double* yaw, double* v, double* tt, double* a, double* d,
                            int64_t cap);
/* HIP-event time of the kernels of the last run (both launches) */
int rrtx_tracker_get_kernel_ms(rrtx_tracker* t, double* kernel_ms);
/* ---- the obstacle index of the tracker (csrc/rpp_obsgrid.h point_first_hit, csrc/rpp_track.h pend_*) -------------------------
 * A tracker on which nothing is set tests lane k of a wave against obstacle k: at most 64 obstacles in one list, more is
 * RRTX_E_INVALID.  With RRTX_OBSIDX_ON the shared list of rrtx_tracker_run and rrtx_tracker_run_from goes through the index
 * of rrtx_steer_set_obstacle_index instead (the same build, the same rules) and may hold 0 .. 2^20 rows.  The TRACK_FAIL_COLL
 * bit is an OR over the trajectory points of "some circle touches this point", and the index answers that per point for the
 * whole list, so every record and array is what the 64-lane form gives where both apply, bit for bit.
 * Mode: RRTX_OBSIDX_OFF (the state of a new tracker) or RRTX_OBSIDX_ON.  RRTX_OBSIDX_AUTO is refused: it would have to accept
 * lists that a tracker with nothing set refuses today, so the choice is the caller's.  RRTX_E_INVALID for AUTO, any other
 * value and a NULL tracker.  Takes effect at the next run.
 * In mode ON, among the argument checks of a run (before any HIP call, also on a host without a device): RRTX_E_INVALID for
 * obs_offsets != NULL (the index serves the shared list only), for more than 2^20 rows, and for
 * robot_radius_per_course != 0 with n_obstacles > 0 (an item holds one threshold per circle).  Then by list: no rows --
 * reason RRTX_OBSIDX_REASON_EMPTY, nothing is tested; the index is usable -- used = 1; it is not (RRTX_OBSIDX_REASON_NOT_FINITE,
 * _RUN_TOO_LONG) and the list has at most 64 rows -- the lane-per-obstacle form runs, used = 0 with that reason; it is not
 * and the list has more rows -- RRTX_E_INVALID naming the reason, nothing is launched and the last run and its getters
 * stay as they were.  The build is kept while the rows, the radius and RRTX_OBSMAP_CELLS stay what they were. */
int rrtx_tracker_set_obstacle_index(rrtx_tracker* t, int32_t mode);
/* What served the list of the last completed run (reason RRTX_OBSIDX_REASON_EMPTY before one), and the mode as set */
int rrtx_tracker_get_obstacle_index_info(rrtx_tracker* t, rrtx_obstacle_index_info* info);
/* The index of the last completed run as built, shaped like rrtx_steer_get_obstacle_index; RRTX_E_STATE when the index did
 * not serve it */
int rrtx_tracker_get_obstacle_index(rrtx_tracker* t, int32_t* cell_start, rrtx_obstacle_item* items, int64_t cap_items,
                                    rrtx_obstacle_item* wide, int64_t cap_wide);

/* ---- tracking the courses a producer left on the device (csrc/rrt_track.hip.h: track_source_kernel) ----------------------
 * rrt_10 keeps its whole chain on the device for its own tree: candidates, roll-outs, search_best_feasible_path
 * (:1495-1524), then only the winner's arrays.  rrtx_tracker_run_from gives the batch objects the same shape: the tracker
 * reads the points of the last solve of an rrtx_steer, rrtx_spline or rrtx_bspline where they lie, during the call only
 * (it returns after its own stream has synchronised, so the producer may be reused or destroyed afterwards).
 * Every completed solve / run of a producer increments its generation; the getters below read it (RRTX_E_INVALID for a
 * NULL pointer; 0 before the first completed solve). */
int rrtx_steer_get_generation(rrtx_steer* s, uint64_t* generation);
#define RRTX_SRC_STEER 1
#define RRTX_SRC_SPLINE 2
#define RRTX_SRC_BSPLINE 3
#define RRTX_SRC_PLANNER 4      /* object = rrtx_handle*: the courses of its last rrtx_gather_courses */
#define RRTX_SELECT_ALL 0
#define RRTX_SELECT_FREE 1   /* courses whose hit == -1; RRTX_E_STATE if the source ran without an obstacle list */
#define RRTX_SELECT_MASK 2   /* mask[i] != 0 */
typedef struct rrtx_track_source {
  int32_t kind, select;     /* RRTX_SRC_*, RRTX_SELECT_* */
  const void* object;       /* rrtx_steer* / rrtx_spline* / rrtx_bspline* / rrtx_handle* */
  uint64_t generation;      /* must equal the object's: else RRTX_E_STATE, nothing launched */
  const uint8_t* mask;      /* host, n bytes, RRTX_SELECT_MASK only */
  int64_t group;            /* 0, or a group size g >= 1 with n % g == 0: courses [j g, (j + 1) g) are group j */
  int32_t arrays_of;        /* 0 every complete course (as rrtx_tracker_run), 1 the group winners only (group > 0) */
} rrtx_track_source;
/* As rrtx_tracker_run on the courses of `src`: b carries everything but the courses (b->offsets, x, y, yaw must be NULL and
 * b->n the source's course count).  Records, arr_offsets, arrays, counts and the kernel time come from the getters above.
 * ood takes two more values: 4 a pose component of the course is not finite (the host path refuses such a batch; here the
 * host never sees the points), 5 the selection left the course out (its points were not read).  Neither owns entries.
 * Returns RRTX_OK, or RRTX_PARTIAL when some ood is 1 .. 4; ood = 5 alone is RRTX_OK.
 * With group = g one decision per group follows the records on the device: search_best_feasible_path (:1504-1513) over the
 * group's courses in order -- among the records with ood == 0 and find_goal set the smallest t_last, the later course of
 * equal times, -1 none.  Courses with ood != 0 are passed over.  With arrays_of = 1 only the winners are rolled out again:
 * arr_offsets is the exclusive sum of len over the winners, every other course owns no entries.
 * Checked in this order.  RRTX_E_INVALID before any HIP call: a NULL pointer, an unknown kind, select or arrays_of,
 * non-NULL course pointers in b, group < 0 or n % group != 0, arrays_of = 1 without a group, a mask missing or given
 * without RRTX_SELECT_MASK, and everything rrtx_tracker_run checks of the remaining fields.  RRTX_E_NO_DEVICE for a
 * tracker without a device.  RRTX_E_INVALID when the source is on another device.  RRTX_E_STATE: the source has no
 * completed run, the generation is stale, the source ran without points (lengths-only, records-only, one-dimensional
 * splines), the last steer solve was an LQR solve (a rollout has no yaw) or an rrtx_steer_solve_all not followed by
 * rrtx_steer_select_free, RRTX_SELECT_FREE on a source without hits.  Then RRTX_E_INVALID when b->n is not the source's
 * course count.  Nothing is launched before all of them passed.
 * RRTX_SRC_PLANNER: the object must be a planner handle alive in this process (RRTX_E_INVALID otherwise, with the argument
 * checks), b->n its instance count and generation that of rrtx_get_course_generation.  RRTX_E_STATE when there is no gather,
 * when the handle has planned (or, for smoothed courses, smoothed) again since, when the gather has no yaw column or was
 * made in RRTX_ORDER_PLANNING (the tracker drives the course), and for RRTX_SELECT_FREE (a planner's courses carry no
 * hits).  An instance without a path is a course of length 0: ood = 2, or 5 when the mask leaves it out. */
int rrtx_tracker_run_from(rrtx_tracker* t, const rrtx_track_params* tp, const rrtx_track_source* src,
                          const rrtx_track_batch* b);
/* The winners of the last rrtx_tracker_run_from with a group: winner (may be NULL) n / g course indices, -1 where a group
 * has none.  RRTX_E_STATE after a run without a group. */
int rrtx_tracker_get_winners(rrtx_tracker* t, int32_t* winner, int64_t* n_groups);
/* The goal poses (:1531) of the last rrtx_tracker_run_from, rows (x, y, yaw): with a group the last point of every
 * winner (n / g rows), without one the last point of every course (n rows); NaN where there is no winner, or the course
 * has ood 2 .. 5.  search_best_feasible_path appends the winner's row to x, y, yaw (:1519-1521).  RRTX_E_STATE after
 * rrtx_tracker_run. */
int rrtx_tracker_get_goals(rrtx_tracker* t, double* goals);

/* ---- batched cubic-spline courses through waypoints, without a planner (csrc/spline_batch.hip.h, csrc/rpp_spline.h) ---------
 * For every course of a batch: what calc_spline_course(x, y, ds) (10_path_planning_00_cubic_spline_path.py :313-325) returns --
 * rx, ry, ryaw, rk, s: a natural cubic spline over the chord length, sampled every ds.  Point counts, offsets and s are the
 * reference's bit for bit.  With the spline coefficient c given (cx, cy: the reference's sx.c and sy.c) x, y, yaw and k are
 * the reference's doubles bit for bit as well.  Without it c is this library's own definition: the Thomas recurrence of
 * csrc/rpp_spline.h over the interior rows, because the reference's np.linalg.solve is not one arithmetic; the
 * result then agrees with the reference to rounding (about 1e-13 in position), not bit for bit.
 * The spline object is independent of rrtx_handle; it owns the device buffers of its runs and reuses them from call to call
 * (they grow, never shrink).  One host thread per object.  Call order: create, run, the getters of that run, run again, as
 * often as wanted; a getter before the first run returns RRTX_E_STATE. */
typedef struct rrtx_spline rrtx_spline;
/* per-course status */
#define RRTX_SPLINE_OK 0
#define RRTX_SPLINE_DEGENERATE 1   /* two consecutive waypoints coincide (h[i] == 0): the reference divides by zero and returns
                                      inf / nan garbage.  The course owns no points. */
#define RRTX_SPLINE_REF_RAISES 2   /* the last sample parameter (len - 1) * ds rounds onto s[-1]: bisect lands on the last knot
                                      and the reference raises IndexError at self.b[i].  The course owns no points. */
#define RRTX_SPLINE_MAX_WAYPOINTS 4096       /* per course */
#define RRTX_SPLINE_MAX_POINTS 268435456LL   /* per call (2^28), over all courses */
typedef struct rrtx_spline_record {
  int32_t status;     /* RRTX_SPLINE_* */
  int32_t reserved;
  int64_t n_points;   /* len(np.arange(0, s[-1], ds)); 0 unless status is RRTX_SPLINE_OK */
  double length;      /* s[-1] */
} rrtx_spline_record;
typedef struct rrtx_spline_batch {
  int64_t n;                  /* courses */
  const int64_t* offsets;     /* n + 1, CSR into x / y (and cx / cy) */
  const double *x, *y;        /* the waypoints */
  const double* ds;           /* one value, or n values when ds_per_course != 0 */
  int32_t ds_per_course;
  int32_t want_arrays;        /* 0: records (and hits) only, no point is stored */
  const double *cx, *cy;      /* both NULL: c by the Thomas recurrence on the device; else n_c values each, c as data */
  int64_t n_c;                /* must equal offsets[n] when cx / cy are given */
  const double* obstacles;    /* rows (x, y, size) */
  int64_t n_obstacles;        /* 0: no collision check; at most 2^20 */
  double robot_radius;
} rrtx_spline_batch;
/* As rrtx_steer_create: without a usable gfx950 device the return value is RRTX_E_NO_DEVICE and *out is still an object
 * (to be destroyed like any other): its runs check their arguments and then return RRTX_E_NO_DEVICE. */
int rrtx_spline_create(int32_t device, rrtx_spline** out);
void rrtx_spline_destroy(rrtx_spline* s);
/* The message of the last call on `s` that failed; for s == NULL the last failure of a spline call of this thread that had no object. */
const char* rrtx_spline_last_error(rrtx_spline* s);
/* Fits and samples every course.  With obstacles every point is tested by check_collision of the pose planners (rrt_05:1625-1638,
 * the form rrtx_steer_set_obstacles describes); thresholds are (size + robot_radius) ** 2, computed on the host.
 * Returns RRTX_OK, or RRTX_PARTIAL when some record's status is not RRTX_SPLINE_OK (every other course is complete).  n == 0 is
 * a valid empty run.  RRTX_E_INVALID, before any HIP call (also on a host without a device): a NULL pointer (obstacles may be
 * NULL when n_obstacles is 0), n < 0 or n > 2^30, offsets that do not start at 0 or that decrease, a course of fewer than 2 or
 * more than RRTX_SPLINE_MAX_WAYPOINTS waypoints, one of cx / cy without the other, n_c != offsets[n], n_obstacles < 0 or
 * > 2^20, a coordinate, c, obstacle entry or robot_radius that is not finite, a coordinate above 1e6 in magnitude, a ds that
 * is not finite or not > 0, or more than RRTX_SPLINE_MAX_POINTS points in all -- estimated before the run from the host's own
 * hypot (one point of slack per course), and checked again on the counts the device returns.  After these checks a host
 * without a device gets RRTX_E_NO_DEVICE. */
int rrtx_spline_run(rrtx_spline* s, const rrtx_spline_batch* b);
/* rec: the n records of the last run; offsets (may be NULL): n + 1 entries, the exclusive sum of n_points; n_courses, n_points,
 * kernel_ms (each may be NULL): the course count, offsets[n], and the HIP-event time of the kernels of the run (fit and
 * evaluation; the prefix sum between them is not kernel time).  rec may be NULL to read the counts alone. */
int rrtx_spline_get_records(rrtx_spline* s, rrtx_spline_record* rec, int64_t* offsets, int64_t* n_courses, int64_t* n_points,
                            double* kernel_ms);
/* The flat arrays of the last run, n_points doubles each, any pointer may be NULL: what calc_spline_course returns as rx, ry,
 * ryaw, rk and s, course after course (cap = doubles available in each; RRTX_E_CAPACITY when too small).  RRTX_E_STATE
 * after a run with want_arrays == 0. */
int rrtx_spline_get_points(rrtx_spline* s, double* x, double* y, double* yaw, double* k, double* t, int64_t cap);
/* c as the last run used it, offsets[n] doubles per axis in the waypoint layout (zeros for a course whose status is
 * RRTX_SPLINE_DEGENERATE); cap = doubles available in each. */
int rrtx_spline_get_c(rrtx_spline* s, double* cx, double* cy, int64_t cap);
/* Per course of the last run: -1 no point of the course touches an obstacle (free); j >= 0 the lowest index of the list any
 * point touches; -2 the course owns no points (status != RRTX_SPLINE_OK, or no sample), nothing was tested.  RRTX_E_STATE when
 * the last run had no obstacle list. */
int rrtx_spline_get_hits(rrtx_spline* s, int32_t* hit);
/* The obstacle index (see rrtx_steer_set_obstacle_index) of rrtx_spline_run */
int rrtx_spline_set_obstacle_index(rrtx_spline* s, int32_t mode);
int rrtx_spline_get_obstacle_index_info(rrtx_spline* s, rrtx_obstacle_index_info* info);
/* Completed rrtx_spline_run / rrtx_spline_fit1d calls on `s` so far (rrtx_track_source.generation) */
int rrtx_spline_get_generation(rrtx_spline* s, uint64_t* generation);

/* -- pointwise queries at the caller's parameters: the methods of CubicSpline1D (:75-140) and CubicSpline2D (:248-310) --
 * The splines of the last completed rrtx_spline_run or rrtx_spline_fit1d stay on the device and answer, per spline, a list
 * of parameters of the caller's choosing (csrc/spline_batch.hip.h: spline_query_kernel, one lane per query).  With c given,
 * every value is the reference's double bit for bit; a parameter of -0.0 is accepted as the reference accepts it. */
/* per-query status */
#define RRTX_SPLINE_Q_OK 0
#define RRTX_SPLINE_Q_OUTSIDE 1      /* t < s[0] or t > s[-1] (+-inf too): the reference returns None */
#define RRTX_SPLINE_Q_REF_RAISES 2   /* t == s[-1], or t is NaN: both range tests are false, bisect lands on the last knot and
                                        the reference raises IndexError at self.b[i] */
#define RRTX_SPLINE_Q_NO_SPLINE 3    /* the spline's status is RRTX_SPLINE_DEGENERATE */
typedef struct rrtx_spline_fit1d_batch {
  int64_t n;                /* splines */
  const int64_t* offsets;   /* n + 1, CSR into knots / values (and c) */
  const double* knots;      /* CubicSpline1D's x: ascending within a spline */
  const double* values;     /* CubicSpline1D's y */
  const double* c;          /* NULL: c by the Thomas recurrence on the device; else n_c values, c as data */
  int64_t n_c;              /* must equal offsets[n] when c is given */
} rrtx_spline_fit1d_batch;
typedef struct rrtx_spline_query_batch {
  int64_t n;                  /* must be the number of splines of the last run / fit1d */
  const int64_t* q_offsets;   /* n + 1, CSR into t: the queries of each spline (a spline may have none) */
  const double* t;            /* the parameters: any double */
  int32_t want_derivatives;   /* != 0: the first and second derivatives are stored as well */
  int32_t reserved;
} rrtx_spline_query_batch;
/* Fits one-dimensional splines (CubicSpline1D(knots, values)) of 2 .. RRTX_SPLINE_MAX_WAYPOINTS knots each, and replaces the
 * splines of the object as a rrtx_spline_run does.  Afterwards rrtx_spline_get_records gives n_points 0 and length =
 * the last knot, rrtx_spline_get_c gives c in cx and leaves cy untouched, and rrtx_spline_get_points and
 * rrtx_spline_get_hits return RRTX_E_STATE.  Returns RRTX_OK, or RRTX_PARTIAL when some spline is RRTX_SPLINE_DEGENERATE (two equal
 * consecutive knots).  RRTX_E_INVALID, before any HIP call and with a message that names the spline: a knot below its
 * predecessor (the reference's ValueError), a knot, value or c that is not finite, a knot or value above 1e6 in magnitude;
 * and as rrtx_spline_run: NULL pointers, n, offsets, the knot counts, n_c. */
int rrtx_spline_fit1d(rrtx_spline* s, const rrtx_spline_fit1d_batch* b);
/* Answers Q = q_offsets[n] queries against the splines of the last completed rrtx_spline_run or rrtx_spline_fit1d (a course
 * whose record says RRTX_SPLINE_REF_RAISES has a spline and answers: that status speaks about ds).  Q == 0 is a valid empty
 * call.  Returns RRTX_OK, or RRTX_PARTIAL when some query's status is not RRTX_SPLINE_Q_OK.  Checked in this order, before any
 * HIP call: what the batch alone shows (RRTX_E_INVALID: a NULL pointer -- t may be NULL when Q is 0 --, n < 0 or > 2^30,
 * q_offsets that do not start at 0 or that decrease, more than RRTX_SPLINE_MAX_POINTS queries), then RRTX_E_STATE without a
 * completed run, then RRTX_E_INVALID when n is not the number of splines of that run. */
int rrtx_spline_query(rrtx_spline* s, const rrtx_spline_query_batch* b);
/* The planes of the last rrtx_spline_query, Q entries each in the order of t, any pointer may be NULL (cap = entries available
 * in each; RRTX_E_CAPACITY when too small).  After rrtx_spline_run: x, y (calc_position), yaw (calc_yaw), k (calc_curvature),
 * and dx, dy, ddx, ddy (sx / sy.calc_first_derivative, calc_second_derivative).  After rrtx_spline_fit1d: y, dy, ddy
 * (calc_position, calc_first_derivative, calc_second_derivative); x, yaw, k, dx, ddx must be NULL (RRTX_E_STATE otherwise).
 * Every value of a query whose status is not RRTX_SPLINE_Q_OK is NaN.  A derivative plane asked of a query made with
 * want_derivatives == 0 returns RRTX_E_STATE, as does a call without a completed query. */
int rrtx_spline_get_query(rrtx_spline* s, double* x, double* y, double* yaw, double* k, double* dx, double* dy, double* ddx,
                          double* ddy, int32_t* status, int64_t cap);
/* n_queries, axes (2 after rrtx_spline_run, 1 after rrtx_spline_fit1d), has_derivatives and the HIP-event time of the kernel
 * of the last rrtx_spline_query; each may be NULL. */
int rrtx_spline_get_query_info(rrtx_spline* s, int64_t* n_queries, int32_t* axes, int32_t* has_derivatives, double* kernel_ms);

/* ---- batched interpolating B-spline courses of degree 1 .. 5 through waypoints (csrc/bspline_batch.hip.h, csrc/rpp_bspline.h)
 * For every course of a batch: what interpolate_b_spline_path(x, y, n_path_points, degree) of 10_path_planning_00_bspline_path.py
 * :59-108 returns -- x, y, heading, curvature -- (param NORMALISED, sample LINSPACE), or what the driver loop of
 * 10_path_planning_00_spline_2d.py :45-54 collects from Spline2D(x, y, kind) (param CHORD, sample ARANGE, degree 1 / 2 / 3 for
 * "linear" / "quadratic" / "cubic").  The reference's bit for bit: the waypoint parameter, the knot vector, the sample
 * parameters, counts and offsets, and x and y of the linear kind.  The B-spline coefficients and the evaluation are this
 * library's own definition (banded elimination without pivoting, Cox-de Boor recurrences in a stated order: csrc/rpp_bspline.h),
 * because scipy's FITPACK is not one arithmetic; they agree with the reference to rounding.  The curvature keeps
 * the script's exponent 2.0 / 3.0 (:107).  The smoothing fit (approximate_b_spline_path with s != 0) is
 * rrtx_bspline_approximate on the same object, below.
 * The object is independent of rrtx_handle; it owns the device buffers of its runs and reuses them from call to call (they
 * grow, never shrink).  One host thread per object.  Call order: create, run, the getters of that run, run again, as often as
 * wanted; a getter before the first run returns RRTX_E_STATE. */
typedef struct rrtx_bspline rrtx_bspline;
/* per-course status */
#define RRTX_BSPLINE_OK 0
#define RRTX_BSPLINE_DEGENERATE 1   /* the waypoint parameter is not strictly increasing: two consecutive waypoints coincide (or
                                       all do).  FITPACK and interp1d both raise.  The course owns no points. */
#define RRTX_BSPLINE_TOO_FEW 2      /* waypoints <= degree: the reference raises.  The course owns no points. */
#define RRTX_BSPLINE_PARAM_NORMALISED 0   /* _calc_distance_vector: scalar np.hypot per chord, np.cumsum, divided by the last */
#define RRTX_BSPLINE_PARAM_CHORD 1        /* Spline2D.__calc_s: the chord length; degree 1 is interp1d's linear kind */
#define RRTX_BSPLINE_SAMPLE_LINSPACE 0    /* np.linspace(0.0, u[-1], count) */
#define RRTX_BSPLINE_SAMPLE_ARANGE 1      /* np.arange(0, s[-1], ds) */
#define RRTX_BSPLINE_SAMPLE_EXPLICIT 2    /* the caller's sample parameters, a CSR list per course */
#define RRTX_BSPLINE_MAX_DEGREE 5
#define RRTX_BSPLINE_MAX_WAYPOINTS 4096       /* per course */
#define RRTX_BSPLINE_MAX_POINTS 268435456LL   /* per call (2^28), over all courses */
typedef struct rrtx_bspline_record {
  int32_t status;     /* RRTX_BSPLINE_* */
  int32_t degree;
  int64_t n_points;   /* 0 unless status is RRTX_BSPLINE_OK */
  double length;      /* the last waypoint parameter: 1.0 (NORMALISED) or s[-1] (CHORD); 0.0 unless status is RRTX_BSPLINE_OK */
} rrtx_bspline_record;
typedef struct rrtx_bspline_batch {
  int64_t n;                    /* courses */
  const int64_t* offsets;       /* n + 1, CSR into x / y */
  const double *x, *y;          /* the waypoints */
  const int32_t* degree;        /* one value, or n values when degree_per_course != 0; each 1 .. RRTX_BSPLINE_MAX_DEGREE */
  int32_t degree_per_course;
  int32_t param;                /* RRTX_BSPLINE_PARAM_* */
  int32_t sample;               /* RRTX_BSPLINE_SAMPLE_*: the sampling mode of every course, unless sample_of is given */
  int32_t sample_per_course;    /* count / ds: n values, else one */
  const int32_t* sample_of;     /* NULL, or n values RRTX_BSPLINE_SAMPLE_*: a sampling mode per course (count, ds and u_offsets
                                   are read only for the courses whose mode uses them) */
  const int64_t* count;         /* LINSPACE: the number of points, each >= 1 */
  const double* ds;             /* ARANGE: the step, each finite and > 0 */
  const int64_t* u_offsets;     /* EXPLICIT: n + 1, CSR into u */
  const double* u;              /* EXPLICIT: the sample parameters, finite; outside [0, length] the end piece is extended */
  int32_t want_arrays;          /* 0: records (and hits) only, no point is stored */
  int32_t reserved;
  const double* obstacles;      /* rows (x, y, size) */
  int64_t n_obstacles;          /* 0: no collision check; at most 2^20 */
  double robot_radius;
} rrtx_bspline_batch;
/* As rrtx_spline_create: without a usable gfx950 device the return value is RRTX_E_NO_DEVICE and *out is still an object
 * (to be destroyed like any other): its runs check their arguments and then return RRTX_E_NO_DEVICE. */
int rrtx_bspline_create(int32_t device, rrtx_bspline** out);
void rrtx_bspline_destroy(rrtx_bspline* s);
/* The message of the last call on `s` that failed; for s == NULL the last failure of a call of this thread that had no object. */
const char* rrtx_bspline_last_error(rrtx_bspline* s);
/* Fits and samples every course.  With obstacles every point is tested as rrtx_spline_run tests it.  Returns RRTX_OK, or
 * RRTX_PARTIAL when some record's status is not RRTX_BSPLINE_OK (every other course is complete).  n == 0 is a valid empty run.
 * RRTX_E_INVALID, before any HIP call (also on a host without a device): a NULL pointer that the mode needs (obstacles may be
 * NULL when n_obstacles is 0), n < 0 or n > 2^30, offsets (or u_offsets) that do not start at 0 or that decrease, a course of
 * fewer than 2 or more than RRTX_BSPLINE_MAX_WAYPOINTS waypoints, a degree outside 1 .. 5, param or sample not one of the
 * values above, a count < 1, a ds that is not finite or not > 0, a coordinate, sample parameter, obstacle entry or
 * robot_radius that is not finite, a coordinate above 1e6 in magnitude, n_obstacles < 0 or > 2^20, or more than
 * RRTX_BSPLINE_MAX_POINTS points in all (for ARANGE estimated before the run from the host's own hypot, one point of slack per
 * course, and checked again on the counts the device returns).  After these checks a host without a device gets
 * RRTX_E_NO_DEVICE. */
int rrtx_bspline_run(rrtx_bspline* s, const rrtx_bspline_batch* b);
/* rec: the n records of the last run; offsets (may be NULL): n + 1 entries, the exclusive sum of n_points; n_courses, n_points,
 * n_knots (each may be NULL): the course count, offsets[n], and the knots of all courses (after rrtx_bspline_approximate: of
 * both axes of all courses).  rec may be NULL. */
int rrtx_bspline_get_records(rrtx_bspline* s, rrtx_bspline_record* rec, int64_t* offsets, int64_t* n_courses, int64_t* n_points,
                             int64_t* n_knots);
/* The flat arrays of the last run, n_points doubles each, any pointer may be NULL: x, y, heading, curvature and the sample
 * parameter, course after course (cap = doubles available in each; RRTX_E_CAPACITY when too small).  RRTX_E_STATE after a
 * run with want_arrays == 0. */
int rrtx_bspline_get_points(rrtx_bspline* s, double* x, double* y, double* yaw, double* k, double* u, int64_t cap);
/* The splines of the last run, any pointer may be NULL.  knot_offsets: n + 1 entries, CSR into knots; a course whose status is
 * RRTX_BSPLINE_OK has waypoints + degree + 1 knots, any other none (cap_knots = doubles available in knots).  cx, cy: the
 * B-spline coefficients in the waypoint layout, offsets[n] doubles per axis, zeros for a course without a spline (cap_wp =
 * doubles available in each). */
int rrtx_bspline_get_coefficients(rrtx_bspline* s, int64_t* knot_offsets, double* knots, int64_t cap_knots, double* cx, double* cy,
                                  int64_t cap_wp);
/* Per course of the last run: -1 no point of the course touches an obstacle (free); j >= 0 the lowest index of the list any
 * point touches; -2 the course owns no points, nothing was tested.  RRTX_E_STATE when the last run had no obstacle list. */
int rrtx_bspline_get_hits(rrtx_bspline* s, int32_t* hit);
/* The obstacle index (see rrtx_steer_set_obstacle_index) of rrtx_bspline_run and rrtx_bspline_approximate */
int rrtx_bspline_set_obstacle_index(rrtx_bspline* s, int32_t mode);
int rrtx_bspline_get_obstacle_index_info(rrtx_bspline* s, rrtx_obstacle_index_info* info);
/* HIP-event time of the kernels of the last run (fit and evaluation; the prefix sum between them is not kernel time) */
int rrtx_bspline_get_kernel_ms(rrtx_bspline* s, double* kernel_ms);
/* Completed rrtx_bspline_run / rrtx_bspline_approximate calls on `s` so far (rrtx_track_source.generation) */
int rrtx_bspline_get_generation(rrtx_bspline* s, uint64_t* generation);

/* ---- the smoothing fit of approximate_b_spline_path (csrc/bspline_smooth.hip.h, csrc/rpp_bspline_smooth.h) -------------------
 * approximate_b_spline_path(x, y, n_path_points, degree, s) of 10_path_planning_00_bspline_path.py :12-56 for every course:
 * UnivariateSpline(distances, x, k=degree, s=s) and the same for y -- Dierckx's fpcurf as scipy drives it, adaptive knots at data
 * sites and a root search on the smoothing parameter --, then _evaluate_spline.  The two axes of a course have knot vectors
 * of their own.  The knot vectors are FITPACK's; the coefficients are this library's own arithmetic (Givens rotations in a stated
 * order) and agree with scipy to a measured tolerance.  A course with s == 0 gets the interpolating spline of
 * rrtx_bspline_run, bit for bit. */
#define RRTX_BSPLINE_SINGULAR 3     /* a coefficient of the smoothing fit is not finite.  The course owns no points. */
typedef struct rrtx_bspline_axis_record {
  int32_t n_knots;    /* knots of this axis' spline; it has n_knots - degree - 1 coefficients.  0 without a spline */
  int32_t ier;        /* FITPACK's: 0 the smoothing spline, -1 the interpolating spline, -2 the least-squares polynomial, 2 the
                         root search met non-monotone values, 3 it took its 20 steps; with 2 and 3 the last approximation is
                         kept, as scipy keeps it (it warns); 1 no interval could take a further knot (FITPACK leaves that case
                         undefined): the least-squares spline on the knots so far */
  double fp;          /* the sum of squared residuals */
  double p;           /* the smoothing parameter; +inf where no root search ran (ier -1, -2, or a least-squares spline) */
  int32_t rounds;     /* knot rounds: least-squares fits */
  int32_t iters;      /* root-search steps */
} rrtx_bspline_axis_record;
typedef struct rrtx_bspline_smooth_batch {
  rrtx_bspline_batch run;       /* as for rrtx_bspline_run; param must be RRTX_BSPLINE_PARAM_NORMALISED */
  const double* s;              /* the smoothing factor: one value, or n values when s_per_course != 0; finite and >= 0 */
  int32_t s_per_course;
  int32_t reserved;
} rrtx_bspline_smooth_batch;
/* As rrtx_bspline_run, with its argument checks and these: sb->s not NULL, every s finite and >= 0, param NORMALISED.  Returns
 * RRTX_OK or RRTX_PARTIAL.  Afterwards rrtx_bspline_get_records, _get_points, _get_hits and _get_kernel_ms answer as after
 * rrtx_bspline_run, except that n_knots of rrtx_bspline_get_records is the sum over both axes of every course; rrtx_bspline_get_coefficients returns RRTX_E_STATE (there is no one knot vector per course); the splines
 * come from the two getters below, which in turn return RRTX_E_STATE after rrtx_bspline_run. */
int rrtx_bspline_approximate(rrtx_bspline* s, const rrtx_bspline_smooth_batch* sb);
/* rec: 2 n records of the last approximate run, axis-major: n of x, then n of y. */
int rrtx_bspline_get_axis_records(rrtx_bspline* s, rrtx_bspline_axis_record* rec, int64_t cap);
/* The splines of one axis (0 x, 1 y) of the last approximate run, any pointer may be NULL.  knot_offsets, coef_offsets: n + 1
 * entries each, CSR into knots and coefficients; n_knots, n_coefs: their last entries.  cap_knots / cap_coefs: doubles
 * available (RRTX_E_CAPACITY when too small).  A course without a spline has none of either. */
int rrtx_bspline_get_axis_splines(rrtx_bspline* s, int32_t axis, int64_t* knot_offsets, double* knots, int64_t cap_knots,
                                  int64_t* coef_offsets, double* coefficients, int64_t cap_coefs, int64_t* n_knots, int64_t* n_coefs);

/* ---- batched arm navigation: joint-space occupancy grids and searches on the torus grid, without a planner
 * (csrc/armnav_batch.hip.h, csrc/rpp_armnav.h) ---------------------------------------------------------------------------------
 * The two functions of 02_arm_obstacle_navigation.py for many scenes and many queries in one call: get_occupancy_grid (:79-110)
 * marks every cell (i, j) of the M x M joint space of a planar N-link arm where a link touches a circle, and astar_torus
 * (:113-184) runs a greedy best-first search with 4-neighbour wrap-around from a start cell to a goal cell.  Everything returned
 * is integers -- grid cells 0 / 1, route cells, the marks 0..6 the search leaves in its grid, the number of cells it closed --
 * and every one of them is the reference's.
 * The object is independent of rrtx_handle; it owns its device buffers, keeps the grids of the last rrtx_armnav_occupancy or
 * rrtx_armnav_set_grids on the device and reuses everything from call to call.  One object serves one thread at a time. */
typedef struct rrtx_armnav rrtx_armnav;

#define RRTX_ARMNAV_ROUTE 0      /* a route was found */
#define RRTX_ARMNAV_NO_ROUTE 1   /* the goal was never opened: the reference prints "No route found." and returns [] (:165-167) */
#define RRTX_ARMNAV_MIN_M 2
#define RRTX_ARMNAV_MAX_M 128              /* the search state of one query lives in the LDS of one wave */
#define RRTX_ARMNAV_MAX_LINKS 16           /* per scene */
#define RRTX_ARMNAV_MAX_CIRCLES 1024       /* per scene */
#define RRTX_ARMNAV_MAX_CELLS 268435456LL  /* scenes x M^2 per call (2^28) */
#define RRTX_ARMNAV_MAX_QUERIES 1048576LL  /* per call (2^20) */

/* The object is handed out on RRTX_E_NO_DEVICE too (destroy it as usual): its calls then check their arguments and fail. */
int rrtx_armnav_create(int32_t device, rrtx_armnav** out);
void rrtx_armnav_destroy(rrtx_armnav* a);
/* The message of the last call on `a` that failed; for a == NULL the last failure of a call of this thread that had no object. */
const char* rrtx_armnav_last_error(rrtx_armnav* a);

/* get_occupancy_grid(arm, obstacles, M) (:79-110, with NLinkArm.update_points :257-262 and detect_collision :46-76) for n_scenes
 * scenes at once.  Scene s has the link lengths link_len[link_off[s] .. link_off[s + 1]) and the circles, rows (x, y, radius),
 * obs_xyr[3 * obs_off[s] .. 3 * obs_off[s + 1]).  As in the reference the grid varies the first two joint angles and leaves the
 * others at what the two-element angle list gives them: link 1 at theta_list[i], every later link at theta_list[i] + theta_list[j].
 * The grids stay on the device for rrtx_armnav_search; rrtx_armnav_get_grids reads them.
 * RRTX_E_INVALID, before any device call and also without a device: M outside 2..128, n_scenes < 1 or n_scenes * M * M > 2^28, a
 * NULL array, offsets that do not start at 0 or decrease, a scene with no link or more than 16, a length that is not finite, is
 * zero (the reference divides by it) or above 1e6 in magnitude (negative lengths are legal), more than 1024 circles in a scene, a
 * circle entry that is not finite, a negative radius. */
int rrtx_armnav_occupancy(rrtx_armnav* a, int32_t M, int64_t n_scenes, const int64_t* link_off, const double* link_len,
                          const int64_t* obs_off, const double* obs_xyr);
/* Grids given as data, n_scenes * M * M bytes, as astar_torus (:113) takes any ndarray: 0 free, 1 obstacle, 2..6 the marks of an
 * earlier search.  RRTX_E_INVALID: the shape as above, bytes NULL, a byte above 6. */
int rrtx_armnav_set_grids(rrtx_armnav* a, int32_t M, int64_t n_scenes, const uint8_t* bytes);
/* The grids on the device, n_scenes * M * M bytes (cap = bytes available).  RRTX_E_STATE before a call that brought grids. */
int rrtx_armnav_get_grids(rrtx_armnav* a, uint8_t* bytes, int64_t cap);

/* astar_torus(grid, start_node, goal_node) (:113-184, with find_neighbors :187-209 and calc_heuristic_map :221-233) for
 * n_queries queries at once: query q searches a copy of grid scene[q] (scene == NULL: grid 0) from the cell start_ij[2 q],
 * start_ij[2 q + 1] to the cell goal_ij[2 q], goal_ij[2 q + 1].  The grids themselves are not changed; with want_marks the
 * grid each query leaves behind (marks 0..6) is kept for rrtx_armnav_get_marks.
 * RRTX_E_INVALID, also without a device: n_queries < 0 or > 2^20, a NULL array, a start or goal index outside [0, M) (numpy would
 * wrap a negative index; this call refuses it), a scene index outside the scenes.  RRTX_E_STATE: no grids. */
int rrtx_armnav_search(rrtx_armnav* a, int64_t n_queries, const int32_t* scene, const int32_t* start_ij, const int32_t* goal_ij,
                       int32_t want_marks);
/* Per query of the last search, any pointer may be NULL: status RRTX_ARMNAV_*, the cells of the route (0 without one), the cells
 * the search closed (trips of the loop :141 that did not end it); n_queries and n_cells, the cells of all routes. */
int rrtx_armnav_get_counts(rrtx_armnav* a, int32_t* status, int32_t* n_route, int32_t* pops, int64_t* n_queries, int64_t* n_cells);
/* The routes of the last search, start first and goal last as the reference returns them (:169-171): offsets[n_queries + 1] into
 * the rows (i, j) of cells_ij (cap = rows available); either pointer may be NULL. */
int rrtx_armnav_get_routes(rrtx_armnav* a, int64_t* offsets, int32_t* cells_ij, int64_t cap);
/* The grid every query left behind, n_queries * M * M bytes (cap = bytes available): 0 free, 1 obstacle, 2 closed (:151),
 * 3 opened (:163), 4 the start, 5 the goal (:142-143), 6 the route after its first cell (:175).  RRTX_E_STATE after a search
 * with want_marks = 0. */
int rrtx_armnav_get_marks(rrtx_armnav* a, uint8_t* marks, int64_t cap);
/* HIP-event time of the kernels of the last rrtx_armnav_occupancy and of the last rrtx_armnav_search. */
int rrtx_armnav_get_kernel_ms(rrtx_armnav* a, double* grid_ms, double* search_ms);

/* ---- batched inverse kinematics of planar arms: the Jacobian inverse method and the driver's P-control loop, without a planner
 * (csrc/armik_batch.hip.h, csrc/rpp_armik.h) -----------------------------------------------------------------------------------
 * inverse_kinematics (:71-85) of 00_simple_2d_inverse_kinematics_01.py and the loop of its driver cell (:189-200) for many
 * queries in one call; every query has its own arm (1..16 links), start angles and Cartesian goal.  Forward kinematics, the
 * Jacobian, the distance test and the whole P-control loop are the reference's doubles; the step pinv(J) @ errors is this
 * library's own closed form with a stated rank rule, so solves agree with the reference's LAPACK step to a measured
 * tolerance where the iteration is short, and not at all where it is chaotic.
 * The object is independent of the others; it owns its device buffers and reuses them.  One object serves one thread at a time. */
typedef struct rrtx_armik rrtx_armik;

#define RRTX_ARMIK_FOUND 0       /* solve: distance < goal_dist; move: the loop ended, distance <= goal_dist */
#define RRTX_ARMIK_NOT_FOUND 1   /* solve: max_iterations trips without it; the angles are returned as they stand (:85) */
#define RRTX_ARMIK_NONFINITE 2   /* solve: a step made an angle NaN or infinite, or a sum of angles reached 105 414 357 rad, where the \
                                    device's sin / cos end; the lane stopped there with the angles as they stand, iterations = \
                                    max_iterations, end and distance those of the last trip that computed them; \
                                    move: the same bound on a sum of angles, which only a huge Kp * dt can reach -- the \
                                    loop stopped there, n_steps counts the step that left */
#define RRTX_ARMIK_STEP_CAP 3    /* move: max_steps steps and still distance > goal_dist (the reference would not return) */
#define RRTX_ARMIK_MAX_LINKS 16
#define RRTX_ARMIK_MAX_QUERIES 1048576LL       /* per call (2^20) */
#define RRTX_ARMIK_MAX_ITERATIONS 1000000
#define RRTX_ARMIK_MAX_STEPS 10000000
#define RRTX_ARMIK_MAX_WAVES 65536             /* an explicit `waves` of rrtx_armik_solve */
#define RRTX_ARMIK_MAX_TRAJECTORY 268435456LL  /* doubles of all trajectories of one move (2^28) */

typedef struct rrtx_armik_batch {
  int64_t n_arms;
  const int64_t* link_off;     /* n_arms + 1, CSR into link_len */
  const double* link_len;      /* zero and negative lengths are legal: nothing divides by a length */
  int64_t n;                   /* queries */
  const int32_t* arm;          /* n, the arm of each query; NULL: arm 0 */
  const double* angles;        /* the start angles, query after query, as many as the query's arm has links */
  const double* goals;         /* n rows (x, y) */
  const double* goal_angles;   /* rrtx_armik_move only: joint_goal_angles in the layout of angles */
  double goal_dist;            /* 0.1 in the script */
} rrtx_armik_batch;

/* The object is handed out on RRTX_E_NO_DEVICE too (destroy it as usual): its calls then check their arguments and fail. */
int rrtx_armik_create(int32_t device, rrtx_armik** out);
void rrtx_armik_destroy(rrtx_armik* a);
/* The message of the last call on `a` that failed; for a == NULL the last failure of a call of this thread that had no object. */
const char* rrtx_armik_last_error(rrtx_armik* a);
/* inverse_kinematics(link_lengths, joint_angles, goal_pos) with N_ITERATIONS = max_iterations for every query.  waves: the
 * number of persistent waves launched, exactly (each lane takes queries from a cursor until it is spent; a wave that finds it
 * spent at once leaves); 0: as many as the device holds, never more than ceil(n / 64).  The results do not depend on it.  Returns RRTX_OK, or RRTX_PARTIAL when some status is not
 * RRTX_ARMIK_FOUND (every query is complete).  RRTX_E_INVALID, before any HIP call and also without a device: a NULL pointer
 * (arm may be NULL), n_arms < 1, an arm of no link or more than 16, a length, angle or goal coordinate that is not finite or
 * above 1e6 in magnitude, n < 0 or > 2^20, arm[q] outside the arms, goal_dist not > 0, max_iterations outside 1..1e6,
 * waves < 0 or > 65536. */
int rrtx_armik_solve(rrtx_armik* a, const rrtx_armik_batch* b, int32_t max_iterations, int32_t waves);
/* The driver's loop for every query: while distance > goal_dist: angles += Kp * ang_diff(goal_angles, angles) * dt.  A query that
 * starts within goal_dist takes no step.  With want_arrays the angles and the distance after every step are kept for
 * rrtx_armik_get_trajectory: a first pass counts the steps, a second fills; nothing is truncated (RRTX_E_CAPACITY above 2^28
 * doubles).  Returns RRTX_OK, or RRTX_PARTIAL when some status is RRTX_ARMIK_STEP_CAP or RRTX_ARMIK_NONFINITE.  RRTX_E_INVALID as above, and for
 * max_steps outside 1..1e7, Kp or dt not finite. */
int rrtx_armik_move(rrtx_armik* a, const rrtx_armik_batch* b, double Kp, double dt, int32_t max_steps, int32_t want_arrays);
/* Per query of the last solve or move, any pointer may be NULL: status RRTX_ARMIK_*; count: the value of `iteration` at the
 * return (max_iterations when not found), or the steps of the move; end_xy rows (x, y): the last current_pos / end effector
 * computed; distance: its distance to the goal; n_queries and n_angles, the doubles of rrtx_armik_get_angles. */
int rrtx_armik_get_records(rrtx_armik* a, int32_t* status, int32_t* count, double* end_xy, double* distance, int64_t* n_queries,
                           int64_t* n_angles);
/* The angles each query ended with: offsets[n_queries + 1] into angles (cap = doubles available); either may be NULL. */
int rrtx_armik_get_angles(rrtx_armik* a, int64_t* offsets, double* angles, int64_t cap);
/* The trajectories of the last move: step_offsets[n + 1] into distance, angle_offsets[n + 1] into angles (step after step, N
 * angles each); any pointer may be NULL.  RRTX_E_STATE after a move with want_arrays = 0 or after a solve. */
int rrtx_armik_get_trajectory(rrtx_armik* a, int64_t* step_offsets, int64_t* angle_offsets, double* angles, double* distance,
                              int64_t cap_steps, int64_t cap_angles);
/* HIP-event time of the kernels of the last run (both passes of a move with arrays) and the waves it launched. */
int rrtx_armik_get_kernel_ms(rrtx_armik* a, double* kernel_ms, int32_t* waves);

/* ---- batched kinematics of n-link arms in 3-D given by Denavit-Hartenberg rows: forward kinematics with the Jacobian and the
 * pose functions, and the Newton-Raphson / Levenberg-Marquardt inverse kinematics, without a planner
 * (csrc/armdh_batch.hip.h, csrc/rpp_armdh.h) -----------------------------------------------------------------------------------
 * forward_kinematics, rot2euler2, rot2euler, rot2quat, quat2rpy and inverse_kinematics of 01_forward_inverse_kinematics.py (and
 * of its class-style twin 01_forward_inverse_kinematics_orig.py) for many queries in one call; every query has its own arm (1..8
 * rows [theta, alpha, a, d], the classic DH matrix), joint angles and reference pose.  Forward kinematics, the Jacobian, the pose
 * functions, diff_pose, K_zyz and the update are the reference's doubles; the step is this library's own definition (one-sided
 * Jacobi SVD with numpy's cut for newton, Cholesky for lm), so solves agree with the reference's LAPACK steps to a
 * measured tolerance away from singular poses and the fold of rot2euler2.
 * The object is independent of the others; it owns its device buffers and reuses them.  One object serves one thread at a time. */
typedef struct rrtx_armdh rrtx_armdh;

#define RRTX_ARMDH_OK 0
#define RRTX_ARMDH_NONFINITE 1        /* an angle became NaN or infinite, or a theta reached 105 414 357 rad, where the device's \
                                         sin / cos end; the lane stopped there with the angles as they stand (forward: the \
                                         record, the transforms and the Jacobian of the query are zero) */
#define RRTX_ARMDH_NO_CONVERGENCE 2   /* newton: 30 Jacobi sweeps that all rotated; lm: a Cholesky pivot that is not > 0; the \
                                         lane stopped before that step */
#define RRTX_ARMDH_NEWTON 0
#define RRTX_ARMDH_LM 1
#define RRTX_ARMDH_MAX_LINKS 8
#define RRTX_ARMDH_MAX_QUERIES 1048576LL   /* per call (2^20) */
#define RRTX_ARMDH_MAX_ITERATIONS 1000000

typedef struct rrtx_armdh_batch {
  int64_t n_arms;
  const int64_t* link_off;   /* n_arms + 1, CSR in links into dh */
  const double* dh;          /* 4 doubles per link: theta, alpha, a, d */
  int64_t n;                 /* queries */
  const int32_t* arm;        /* n, the arm of each query; NULL: arm 0 */
  const double* angles;      /* the joint angles that replace column 0, query after query, as many as the query's arm has links;
                                NULL: the arms' own column 0 */
  const double* ref_pose;    /* rrtx_armdh_solve only: n rows x, y, z, alpha, beta, gamma */
} rrtx_armdh_batch;

/* The object is handed out on RRTX_E_NO_DEVICE too (destroy it as usual): its calls then check their arguments and fail. */
int rrtx_armdh_create(int32_t device, rrtx_armdh** out);
void rrtx_armdh_destroy(rrtx_armdh* a);
/* The message of the last call on `a` that failed; for a == NULL the last failure of a call of this thread that had no object. */
const char* rrtx_armdh_last_error(rrtx_armdh* a);
/* forward_kinematics(link_list) and the pose functions of the last transform for every query.  Returns RRTX_OK, or RRTX_PARTIAL
 * when some status is not RRTX_ARMDH_OK (every other query is complete).  RRTX_E_INVALID, before any HIP call and also without a
 * device: a NULL pointer (arm and angles may be NULL), n_arms < 1, an arm of no link or more than 8, a DH entry or angle that is
 * not finite or above 1e6 in magnitude, n < 0 or > 2^20, arm[q] outside the arms. */
int rrtx_armdh_forward(rrtx_armdh* a, const rrtx_armdh_batch* b);
/* inverse_kinematics(iter_cnt, link_list, ref_ee_pose) without the drawing for every query: exactly iter_cnt trips of
 * theta += step / step_div (200 in the script, 100 in its twin), method RRTX_ARMDH_NEWTON (the live code) or RRTX_ARMDH_LM (the
 * variant of :423-428, eps its damping), then one more forward pass for the pose.  There is no convergence test, as in the
 * reference.  Returns as rrtx_armdh_forward; RRTX_E_INVALID also for ref_pose NULL or an entry not finite or above 1e6,
 * iter_cnt outside 1..1e6, step_div zero or not finite, a method other than the two, eps not > 0 or not finite with lm. */
int rrtx_armdh_solve(rrtx_armdh* a, const rrtx_armdh_batch* b, int32_t iter_cnt, double step_div, int32_t method, double eps);
/* Per query of the last call, any pointer may be NULL: status RRTX_ARMDH_*; values 16 doubles a query -- after a forward the
 * position (3), rot2euler2 (3), rot2euler (3), rot2quat (4) and quat2rpy of it (3); after a solve the pose x, y, z, alpha, beta,
 * gamma of the returned angles (6), pose_error = ref - pose (6) and 4 zeros; kappa_max (the largest sigma_1 / smallest kept
 * sigma the solve met) and n_cut (the trips on which a singular value was cut), both of newton solves and 0 otherwise;
 * n_queries and n_links, the number of links of all queries. */
int rrtx_armdh_get_records(rrtx_armdh* a, int32_t* status, double* values, double* kappa_max, int32_t* n_cut, int64_t* n_queries,
                           int64_t* n_links);
/* The angles each query of the last solve ended with, as the script leaves them in link_list: offsets[n_queries + 1] into
 * angles (cap = doubles available); either may be NULL.  After a forward only the offsets exist (angles: RRTX_E_STATE). */
int rrtx_armdh_get_angles(rrtx_armdh* a, int64_t* offsets, double* angles, int64_t cap);
/* The global transforms of the last forward, 16 doubles (4 x 4 row-major) per link, query after query in the offsets of
 * rrtx_armdh_get_angles (cap = doubles available).  RRTX_E_STATE after a solve. */
int rrtx_armdh_get_transforms(rrtx_armdh* a, double* transforms, int64_t cap);
/* The Jacobians of the last forward: for query q the (6, N) matrix row-major at 6 * offsets[q] (cap = doubles available).
 * RRTX_E_STATE after a solve. */
int rrtx_armdh_get_jacobians(rrtx_armdh* a, double* jacobians, int64_t cap);
/* HIP-event time of the kernel of the last call and the waves it launched. */
int rrtx_armdh_get_kernel_ms(rrtx_armdh* a, double* kernel_ms, int32_t* waves);

/* parity harness: out[i] = op(a[i], b[i]) evaluated on the device.  op 0 math.hypot, 1 x**2, 2 sin, 3 cos, 4 atan2,
 * 5 steer end x (rrt_04:1086-1115), 6 sqrt, 7 a/b, 8 acos, 9 asin, 10 checksum of the Reeds-Shepp steer
 * (0,0,0) -> (a, b, a+b) (rrt_06:1426-1441, csrc/rpp_rs.h), 11 math.tan(a) (|a| <= 0.79), 12 np.hypot(a, b).
 * op 13: the cross-lane integer helpers of the one-wave RRT* kernel (csrc/rrt_star_v2_shapes.inc), each 64-lane group of
 * the input by itself: a[i] a uint32 value, b[i] an int32 index, n a multiple of 64, and out holds 5 n doubles:
 * out[i] the inclusive prefix sum of a over the group (mod 2^32, as int32), out[n + i] the group's total, out[2 n + i] and
 * out[3 n + i] value and index of the argmin of (a, b) with the lowest index among equal values, out[4 n + i] min(a). */
int rrtx_selftest_math(int32_t device, int32_t op, const double* a, const double* b, double* out, int64_t n);

/* Run-time check of the arithmetic contract: "identical to the reference on this host" holds while
 * the host's libm -- the one the reference's CPython calls -- returns what the device's operation-by-operation replicas
 * of glibc 2.35's x86-64 FMA variants return.  Evaluates n_per_fn seeded arguments per function on the device and with
 * the HOST's libm, over the argument ranges the planners use, and counts the results that differ in any bit:
 * mismatches8[0..7] = pow(x, 2), sin, cos, atan2, acos, asin, sqrt, a / b.  Returns RRTX_OK when the check ran (whatever it
 * found).  All zero: doubles are bit-identical to the reference run on this host.  Otherwise the planners still run and
 * are self-consistent, but match the reference only up to the few-ULP differences between the two libm builds (integer
 * results can then differ at near-ties).  math.hypot is CPython's own algorithm, not libm's: the Python host checks it
 * (and float ** 2) against the interpreter itself with rrtx_selftest_math (robotics-path-planning_amd/_abi.py selfcheck). */
int rrtx_selfcheck(int32_t device, int32_t n_per_fn, int64_t* mismatches8);

#ifdef __cplusplus
}
#endif
#endif

"""ctypes binding of librrtx.so (the C ABI in include/rrtx.h).

There is no Python or CPU fallback: if the shared library is missing, or no
gfx950 device is usable, planning raises.  Build with
`make -C robotics-path-planning_amd/csrc` (or `__graft_entry__.build()`).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RRTX_LIB") or os.path.join(_HERE, "librrtx.so")

RRTX_ABI_VERSION = 6
ALGO_RRT, ALGO_RRT_STAR, ALGO_INFORMED, ALGO_DUBINS, ALGO_BITSTAR, ALGO_RRT_DUBINS, ALGO_RS = 0, 1, 2, 3, 4, 5, 6
ALGO_LQR_RRT_STAR = 7   # include/rrtx.h: #define RRTX_ALGO_LQR_RRT_STAR
SAMPLER_MT, SAMPLER_SOBOL = 0, 1
ST_DONE, ST_PATH, ST_OVERFLOW, ST_PATH_TRUNC, ST_UNSUPPORTED, ST_REF_RAISES, ST_REF_HANGS = 1, 2, 4, 8, 16, 32, 64
ST_FAILED = ST_OVERFLOW | ST_UNSUPPORTED | ST_REF_RAISES   # the instance stopped without a result
RRTX_PARTIAL = 1
ERRORS = {1: "RRTX_PARTIAL", 0: "OK", -1: "RRTX_E_INVALID", -2: "RRTX_E_NO_DEVICE", -3: "RRTX_E_HIP", -4: "RRTX_E_CAPACITY",
          -5: "RRTX_E_STATE", -6: "RRTX_E_OVERFLOW"}

EXPORTS = ["rrtx_abi_version", "rrtx_device_count", "rrtx_create", "rrtx_set_obstacles", "rrtx_set_instance_obstacles", "rrtx_set_rng_state",
           "rrtx_get_rng_state", "rrtx_seed_instances", "rrtx_set_instance", "rrtx_set_instance_rotation", "rrtx_plan", "rrtx_get_tree",
           "rrtx_get_path", "rrtx_get_results", "rrtx_results_device_ptr", "rrtx_copy_results_device", "rrtx_get_sobol_index", "rrtx_get_yaw", "rrtx_get_polylines", "rrtx_get_stats",
           "rrtx_enable_trace", "rrtx_get_trace", "rrtx_get_trace_kind", "rrtx_get_sample_stream", "rrtx_get_phase_cycles", "rrtx_last_error", "rrtx_destroy", "rrtx_selftest_math",
           "rrtx_smooth_paths", "rrtx_smooth_planned", "rrtx_get_smoothed_path", "rrtx_get_path_yaw", "rrtx_selfcheck", "rrtx_plan_many", "rrtx_plan_begin", "rrtx_plan_step",
           "rrtx_set_launch_bound", "rrtx_rccl_unique_id", "rrtx_rccl_init", "rrtx_rccl_gather_results",
           "rrtx_set_rs_cost", "rrtx_track_planned", "rrtx_get_track_outcome", "rrtx_get_track_arrays", "rrtx_get_track_records",
           "rrtx_get_track_stats",
           "rrtx_steer_create", "rrtx_steer_destroy", "rrtx_steer_last_error", "rrtx_steer_solve", "rrtx_steer_get_counts",
           "rrtx_steer_get_summary", "rrtx_steer_get_points", "rrtx_steer_get_kernel_ms", "rrtx_steer_set_obstacles",
           "rrtx_steer_get_hits", "rrtx_steer_solve_lqr", "rrtx_steer_get_ends",
           "rrtx_steer_solve_bezier", "rrtx_steer_solve_bezier_cp", "rrtx_steer_get_curvature", "rrtx_steer_get_kmax",
           "rrtx_steer_get_control_points",
           "rrtx_steer_solve_all", "rrtx_steer_get_cand_counts", "rrtx_steer_get_cand_summary", "rrtx_steer_get_cand_points",
           "rrtx_steer_select_free",
           "rrtx_tracker_create", "rrtx_tracker_destroy", "rrtx_tracker_last_error", "rrtx_tracker_run",
           "rrtx_tracker_get_counts", "rrtx_tracker_get_records", "rrtx_tracker_get_arrays", "rrtx_tracker_get_kernel_ms",
           "rrtx_tracker_run_from", "rrtx_tracker_get_winners", "rrtx_tracker_get_goals", "rrtx_steer_get_generation",
           "rrtx_spline_get_generation", "rrtx_bspline_get_generation",
           "rrtx_gather_courses", "rrtx_get_course_counts", "rrtx_get_courses", "rrtx_get_course_generation",
           "rrtx_query_goals", "rrtx_get_goal_query", "rrtx_gather_goal_courses", "rrtx_get_goal_course_counts",
           "rrtx_get_goal_courses", "rrtx_get_goal_query_kernel_ms",
           "rrtx_track_goals", "rrtx_get_goal_track", "rrtx_get_goal_track_records", "rrtx_get_goal_track_arrays",
           "rrtx_get_goal_track_kernel_ms", "rrtx_get_polyline_yaw",
           "rrtx_spline_create", "rrtx_spline_destroy", "rrtx_spline_last_error", "rrtx_spline_run", "rrtx_spline_get_records",
           "rrtx_spline_get_points", "rrtx_spline_get_c", "rrtx_spline_get_hits",
           "rrtx_spline_fit1d", "rrtx_spline_query", "rrtx_spline_get_query", "rrtx_spline_get_query_info",
           "rrtx_bspline_create", "rrtx_bspline_destroy", "rrtx_bspline_last_error", "rrtx_bspline_run", "rrtx_bspline_get_records",
           "rrtx_bspline_get_points", "rrtx_bspline_get_coefficients", "rrtx_bspline_get_hits", "rrtx_bspline_get_kernel_ms",
           "rrtx_bspline_approximate", "rrtx_bspline_get_axis_records", "rrtx_bspline_get_axis_splines",
           "rrtx_armnav_create", "rrtx_armnav_destroy", "rrtx_armnav_last_error", "rrtx_armnav_occupancy", "rrtx_armnav_set_grids",
           "rrtx_armnav_get_grids", "rrtx_armnav_search", "rrtx_armnav_get_counts", "rrtx_armnav_get_routes",
           "rrtx_armnav_get_marks", "rrtx_armnav_get_kernel_ms",
           "rrtx_armik_create", "rrtx_armik_destroy", "rrtx_armik_last_error", "rrtx_armik_solve", "rrtx_armik_move",
           "rrtx_armik_get_records", "rrtx_armik_get_angles", "rrtx_armik_get_trajectory", "rrtx_armik_get_kernel_ms",
           "rrtx_armdh_create", "rrtx_armdh_destroy", "rrtx_armdh_last_error", "rrtx_armdh_forward", "rrtx_armdh_solve",
           "rrtx_armdh_get_records", "rrtx_armdh_get_angles", "rrtx_armdh_get_transforms", "rrtx_armdh_get_jacobians",
           "rrtx_armdh_get_kernel_ms",
           "rrtx_set_obstacle_map", "rrtx_get_obstacle_map_info", "rrtx_get_obstacle_map",
           "rrtx_steer_set_obstacle_index", "rrtx_steer_get_obstacle_index_info", "rrtx_steer_get_obstacle_index",
           "rrtx_spline_set_obstacle_index", "rrtx_spline_get_obstacle_index_info",
           "rrtx_bspline_set_obstacle_index", "rrtx_bspline_get_obstacle_index_info",
           "rrtx_tracker_set_obstacle_index", "rrtx_tracker_get_obstacle_index_info", "rrtx_tracker_get_obstacle_index"]
OBSIDX_AUTO, OBSIDX_ON, OBSIDX_OFF, OBSIDX_MIN = 0, 1, 2, 256                          # include/rrtx.h: #define RRTX_OBSIDX_*
OBSIDX_REASONS = ("used", "off", "below the threshold", "run too long", "non-finite reach", "empty")   # RRTX_OBSIDX_REASON_*
OBSTACLE_TILE_MAX, OBSTACLE_MAP_MAX = 256, 1 << 20   # csrc MAX_OBS (rrtx_set_obstacles), rpp_obsgrid.h M_MAX (rrtx_set_obstacle_map)
OBSTACLE_TILE_MAX_RS = 64                            # csrc rppr::MAX_OBS: the tile of RRTX_ALGO_RS (rrtx_set_obstacles)
OBSTACLE_MAP_ALGOS = (0, 1, ALGO_RS)                 # RRTX_ALGO_RRT, RRTX_ALGO_RRT_STAR, RRTX_ALGO_RS
STEER_DUBINS, STEER_RS = 0, 1                                                      # include/rrtx.h: #define RRTX_STEER_*
STEER_LQR = 2   # this binding's own name for "solved by rrtx_steer_solve_lqr": the C ABI has an entry point, not a kind value
STEER_BEZIER = 3   # likewise: rrtx_steer_solve_bezier / rrtx_steer_solve_bezier_cp
BEZIER_MIN_CP, BEZIER_MAX_CP, BEZIER_MAX_POINTS = 3, 16, 4096   # csrc/rpp_bezier.h
STEER_OK, STEER_NO_PATH, STEER_RAISES_ZERODIV, STEER_RAISES_VALUE = 0, 1, 2, 3
DUBINS_WORDS = ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")   # _PATH_TYPE_MAP order: the word indices of rrtx_steer_solve
RS_COST_EUCLID, RS_COST_PATH = 0, 1     # include/rrtx.h: #define RRTX_RS_COST_*
TRACK_FAIL_REACH, TRACK_FAIL_ANGLE, TRACK_FAIL_LONG, TRACK_FAIL_COLLISION = 1, 2, 4, 8   # #define RRTX_TRACK_FAIL_*
OOD_DOMAIN, OOD_RAISES, OOD_OVERFLOW, OOD_NOT_FINITE, OOD_SKIPPED = 1, 2, 3, 4, 5        # rrtx_track_record.ood
SRC_STEER, SRC_SPLINE, SRC_BSPLINE, SRC_PLANNER = 1, 2, 3, 4                             # #define RRTX_SRC_*
COURSE_PLANNED, COURSE_SMOOTHED = 0, 1                                                   # #define RRTX_COURSE_*
ORDER_PLANNING, ORDER_DRIVING = 0, 1                                                     # #define RRTX_ORDER_*
GOALQ_OK, GOALQ_NONE, GOALQ_NO_TREE, GOALQ_OVERFLOW = 0, 1, 2, 3                           # #define RRTX_GOALQ_*
GOALQ_MAX_QUERIES, GOALQ_MAX_CANDIDATES = 1 << 24, 512                                   # the second: csrc NU_MAX
SELECT_ALL, SELECT_FREE, SELECT_MASK = 0, 1, 2                                          # #define RRTX_SELECT_*
SPLINE_OK, SPLINE_DEGENERATE, SPLINE_REF_RAISES = 0, 1, 2                                # #define RRTX_SPLINE_*
SPLINE_MAX_WAYPOINTS, SPLINE_MAX_POINTS = 4096, 1 << 28
SPLINE_Q_OK, SPLINE_Q_OUTSIDE, SPLINE_Q_REF_RAISES, SPLINE_Q_NO_SPLINE = 0, 1, 2, 3        # #define RRTX_SPLINE_Q_*
BSPLINE_OK, BSPLINE_DEGENERATE, BSPLINE_TOO_FEW = 0, 1, 2                                 # #define RRTX_BSPLINE_*
BSPLINE_SINGULAR = 3                                                                     # rrtx_bspline_approximate only
BSPLINE_PARAM_NORMALISED, BSPLINE_PARAM_CHORD = 0, 1
BSPLINE_SAMPLE_LINSPACE, BSPLINE_SAMPLE_ARANGE, BSPLINE_SAMPLE_EXPLICIT = 0, 1, 2
BSPLINE_MAX_DEGREE, BSPLINE_MAX_WAYPOINTS, BSPLINE_MAX_POINTS = 5, 4096, 1 << 28
ARMNAV_ROUTE, ARMNAV_NO_ROUTE = 0, 1                                                     # #define RRTX_ARMNAV_*
ARMNAV_MIN_M, ARMNAV_MAX_M, ARMNAV_MAX_LINKS, ARMNAV_MAX_CIRCLES = 2, 128, 16, 1024
ARMNAV_MAX_CELLS, ARMNAV_MAX_QUERIES = 1 << 28, 1 << 20
ARMIK_FOUND, ARMIK_NOT_FOUND, ARMIK_NONFINITE, ARMIK_STEP_CAP = 0, 1, 2, 3                # #define RRTX_ARMIK_*
ARMIK_MAX_LINKS, ARMIK_MAX_QUERIES, ARMIK_MAX_ITERATIONS, ARMIK_MAX_STEPS, ARMIK_MAX_TRAJECTORY = 16, 1 << 20, 1000000, 10000000, 1 << 28
ARMIK_MAX_WAVES = 1 << 16
ARMDH_OK, ARMDH_NONFINITE, ARMDH_NO_CONVERGENCE = 0, 1, 2                                 # #define RRTX_ARMDH_*
ARMDH_NEWTON, ARMDH_LM = 0, 1
ARMDH_MAX_LINKS, ARMDH_MAX_QUERIES, ARMDH_MAX_ITERATIONS = 8, 1 << 20, 1000000


class Params(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("algo", C.c_int32), ("sampler", C.c_int32),
                ("goal_sample_rate", C.c_int32), ("max_iter", C.c_int32), ("has_play_area", C.c_int32),
                ("search_until_max_iter", C.c_int32), ("n_instances", C.c_int32), ("device", C.c_int32),
                ("reserved_i", C.c_int32 * 7),
                ("start", C.c_double * 3), ("goal", C.c_double * 3),
                ("rand_min", C.c_double), ("rand_max", C.c_double),
                ("expand_dis", C.c_double), ("path_resolution", C.c_double),
                ("play_area", C.c_double * 4), ("robot_radius", C.c_double),
                ("connect_circle_dist", C.c_double), ("informed_rot", C.c_double * 4),
                ("informed_c_min", C.c_double), ("curvature", C.c_double), ("goal_yaw_th", C.c_double),
                ("goal_xy_th", C.c_double), ("step_size", C.c_double), ("reserved_d", C.c_double * 3)]


class TrackParams(C.Structure):
    """rrtx_track_params: ClosedLoopRRTStar's keywords (rrt_10:1458-1476) and the model globals (:1592-1607)."""
    _fields_ = [(k, C.c_double) for k in ("target_speed", "yaw_th", "xy_th", "invalid_travel_ratio", "dt", "L", "steer_max",
                                          "accel_max", "Kp", "Lf", "T", "goal_dis", "stop_speed")]


TRACK_DEFAULTS = dict(target_speed=10.0 / 3.6, yaw_th=float(np.deg2rad(3.0)), xy_th=0.5, invalid_travel_ratio=5.0, dt=0.05,
                      L=0.9, steer_max=float(np.deg2rad(40.0)), accel_max=5.0, Kp=2.0, Lf=0.5, T=100.0, goal_dis=0.5,
                      stop_speed=0.5)


class TrackOutcome(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("flag", "winner", "n_cand", "len", "node", "status")]


TRACK_RECORD = np.dtype([("find_goal", np.int32), ("len", np.int32), ("fail", np.int32), ("ood", np.int32),
                         ("t_last", np.float64)])


class GoalTrackOutcome(C.Structure):
    """rrtx_goal_track_outcome: the answer of one (instance, goal) query of rrtx_track_goals."""
    _fields_ = [(k, C.c_int32) for k in ("flag", "winner", "n_cand", "len", "node", "status", "no_tree", "reserved")] + \
               [("t_last", C.c_double)]


GOAL_TRACK_OUTCOME = np.dtype([(k, np.int32) for k in ("flag", "winner", "n_cand", "len", "node", "status", "no_tree", "reserved")] +
                              [("t_last", np.float64)])


class TrackBatch(C.Structure):
    """rrtx_track_batch: the courses of one rrtx_tracker_run (pointers into arrays the caller keeps alive)."""
    _fields_ = [("n", C.c_int64), ("offsets", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("yaw", C.c_void_p),
                ("per_course", C.c_void_p), ("start_state", C.c_void_p), ("obstacles", C.c_void_p),
                ("obs_offsets", C.c_void_p), ("n_obstacles", C.c_int64), ("robot_radius", C.c_void_p),
                ("robot_radius_per_course", C.c_int32), ("want_arrays", C.c_int32)]


class TrackSource(C.Structure):
    """rrtx_track_source: the producer whose device-resident courses one rrtx_tracker_run_from tracks."""
    _fields_ = [("kind", C.c_int32), ("select", C.c_int32), ("object", C.c_void_p), ("generation", C.c_uint64),
                ("mask", C.c_void_p), ("group", C.c_int64), ("arrays_of", C.c_int32)]


def on_device(v):
    """points="device" / arrays="device": solve as with True, fetch no point array, leave the courses to BatchTrack.run."""
    return isinstance(v, str) and v == "device"


class DeviceCourses:
    """The courses a producer's solve left on the device: the owning native object (Steer, Spline, BSpline, or a planner
    Handle after gather_courses), its RRTX_SRC_* kind and the generation of that solve.  BatchTrack.run reads them where they lie; the native call refuses
    them (RRTX_E_STATE) once the owner has solved again."""

    def __init__(self, kind, owner):
        self.kind, self.owner, self.generation = kind, owner, owner.generation()


SPLINE_RECORD = np.dtype([("status", np.int32), ("reserved", np.int32), ("n_points", np.int64), ("length", np.float64)])


class SplineBatch(C.Structure):
    """rrtx_spline_batch: the courses of one rrtx_spline_run (pointers into arrays the caller keeps alive)."""
    _fields_ = [("n", C.c_int64), ("offsets", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("ds", C.c_void_p),
                ("ds_per_course", C.c_int32), ("want_arrays", C.c_int32), ("cx", C.c_void_p), ("cy", C.c_void_p),
                ("n_c", C.c_int64), ("obstacles", C.c_void_p), ("n_obstacles", C.c_int64), ("robot_radius", C.c_double)]


class SplineFit1dBatch(C.Structure):
    """rrtx_spline_fit1d_batch: the one-dimensional splines of one rrtx_spline_fit1d."""
    _fields_ = [("n", C.c_int64), ("offsets", C.c_void_p), ("knots", C.c_void_p), ("values", C.c_void_p), ("c", C.c_void_p),
                ("n_c", C.c_int64)]


class SplineQueryBatch(C.Structure):
    """rrtx_spline_query_batch: the parameters of one rrtx_spline_query, a CSR list per spline."""
    _fields_ = [("n", C.c_int64), ("q_offsets", C.c_void_p), ("t", C.c_void_p), ("want_derivatives", C.c_int32),
                ("reserved", C.c_int32)]


BSPLINE_RECORD = np.dtype([("status", np.int32), ("degree", np.int32), ("n_points", np.int64), ("length", np.float64)])


class BSplineBatch(C.Structure):
    """rrtx_bspline_batch: the courses of one rrtx_bspline_run (pointers into arrays the caller keeps alive)."""
    _fields_ = [("n", C.c_int64), ("offsets", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("degree", C.c_void_p),
                ("degree_per_course", C.c_int32), ("param", C.c_int32), ("sample", C.c_int32), ("sample_per_course", C.c_int32),
                ("sample_of", C.c_void_p), ("count", C.c_void_p), ("ds", C.c_void_p), ("u_offsets", C.c_void_p), ("u", C.c_void_p),
                ("want_arrays", C.c_int32), ("reserved", C.c_int32), ("obstacles", C.c_void_p), ("n_obstacles", C.c_int64),
                ("robot_radius", C.c_double)]


BSPLINE_AXIS_RECORD = np.dtype([("n_knots", np.int32), ("ier", np.int32), ("fp", np.float64), ("p", np.float64),
                                ("rounds", np.int32), ("iters", np.int32)])


class BSplineSmoothBatch(C.Structure):
    """rrtx_bspline_smooth_batch: the courses of one rrtx_bspline_approximate -- the run batch, and the smoothing factors."""
    _fields_ = [("run", BSplineBatch), ("s", C.c_void_p), ("s_per_course", C.c_int32), ("reserved", C.c_int32)]


class ArmIKBatch(C.Structure):
    """rrtx_armik_batch: the queries of one rrtx_armik_solve / rrtx_armik_move (pointers into arrays the caller keeps alive)."""
    _fields_ = [("n_arms", C.c_int64), ("link_off", C.c_void_p), ("link_len", C.c_void_p), ("n", C.c_int64), ("arm", C.c_void_p),
                ("angles", C.c_void_p), ("goals", C.c_void_p), ("goal_angles", C.c_void_p), ("goal_dist", C.c_double)]


class ArmDHBatch(C.Structure):
    """rrtx_armdh_batch: the queries of one rrtx_armdh_forward / rrtx_armdh_solve (pointers into arrays the caller keeps alive)."""
    _fields_ = [("n_arms", C.c_int64), ("link_off", C.c_void_p), ("dh", C.c_void_p), ("n", C.c_int64), ("arm", C.c_void_p),
                ("angles", C.c_void_p), ("ref_pose", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("edges_unique", C.c_int64), ("edges_ref", C.c_int64),
                ("near_hits", C.c_int64), ("near_unique", C.c_int64), ("rewires", C.c_int64),
                ("propagated", C.c_int64), ("scan_nodes", C.c_int64), ("algorithmic_bytes", C.c_int64),
                ("exact_rescans", C.c_int64), ("total_nodes", C.c_int64), ("launches", C.c_int64),
                ("kernel_ms", C.c_double), ("plan_ms", C.c_double), ("algorithmic_bytes_two_scan", C.c_int64),
                ("near_unique_max", C.c_int64), ("f32_fallbacks", C.c_int64), ("q16_fallbacks", C.c_int64),
                ("launches_main", C.c_int64), ("kernel_ms_main", C.c_double), ("replanned", C.c_int64),
                ("main_shape", C.c_int32), ("main_f32", C.c_int32), ("passes_shared", C.c_int64)]


# the C prefixes of the device objects besides the planner handle: rrtx_<prefix>_create / _destroy / _last_error
DEVICE_OBJECTS = ("steer", "tracker", "spline", "bspline", "armnav", "armik", "armdh")


class RrtxError(RuntimeError):
    pass


class ObstacleMapInfo(C.Structure):
    """rrtx_obstacle_map_info"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("cell", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("n_circles", C.c_int64), ("n_items", C.c_int64), ("n_wide", C.c_int64), ("build_ms", C.c_double)]


def tracker_obstacle_index_mode(obstacle_index):
    """The `obstacle_index` keyword of BatchTrack as an RRTX_OBSIDX_* mode: True or False.  None (automatic) is refused: it
    would have to accept lists that a tracker with nothing set refuses."""
    if obstacle_index is True or obstacle_index is False:
        return OBSIDX_ON if obstacle_index else OBSIDX_OFF
    raise ValueError("BatchTrack: obstacle_index is True or False, got %r" % (obstacle_index,))


class ObstacleIndexInfo(C.Structure):
    """rrtx_obstacle_index_info"""
    _fields_ = [("mode", C.c_int32), ("used", C.c_int32), ("reason", C.c_int32), ("reserved", C.c_int32),
                ("map", ObstacleMapInfo)]


def obstacle_index_mode(obstacle_index):
    """The `obstacle_index` keyword of BatchSteer, BatchSpline and BatchBSpline as an RRTX_OBSIDX_* mode: None = the index
    when the list has more than OBSIDX_MIN circles, True = always, False = never."""
    if obstacle_index is None:
        return OBSIDX_AUTO
    if obstacle_index is True or obstacle_index is False:
        return OBSIDX_ON if obstacle_index else OBSIDX_OFF
    raise ValueError("obstacle_index is None, True or False, got %r" % (obstacle_index,))


# rrtx_obstacle_item: one 32-byte record of the obstacle map
OBSTACLE_ITEM = np.dtype([("ox", np.float64), ("oy", np.float64), ("thr", np.float64), ("index", np.int64)])


def use_obstacle_map(obstacle_map, n_obstacles, limit=OBSTACLE_TILE_MAX):
    """The `obstacle_map` keyword of the planners: None = the map when the list does not fit the tile (`limit` circles:
    OBSTACLE_TILE_MAX, or OBSTACLE_TILE_MAX_RS for the Reeds-Shepp planners), True, False."""
    if obstacle_map is None:
        return n_obstacles > limit
    if obstacle_map is True or obstacle_map is False:
        return obstacle_map
    raise ValueError("obstacle_map is None, True or False, got %r" % (obstacle_map,))


_lib = None


def load():
    """Load librrtx.so; raises RrtxError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RrtxError("librrtx.so not built (%s); run `make -C robotics-path-planning_amd/csrc` -- there is no "
                        "CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64p = C.c_void_p, C.c_int32, C.POINTER(C.c_int64)
    L.rrtx_abi_version.restype = C.c_int
    L.rrtx_device_count.restype = C.c_int
    L.rrtx_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.rrtx_set_obstacles.argtypes = [vp, vp, i32]
    L.rrtx_set_instance_obstacles.argtypes = [vp, vp, vp]
    L.rrtx_set_obstacle_map.argtypes = [vp, vp, C.c_int64]
    L.rrtx_get_obstacle_map_info.argtypes = [vp, C.POINTER(ObstacleMapInfo)]
    L.rrtx_get_obstacle_map.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int64]
    for obj in ("steer", "spline", "bspline"):
        getattr(L, "rrtx_%s_set_obstacle_index" % obj).argtypes = [vp, i32]
        getattr(L, "rrtx_%s_get_obstacle_index_info" % obj).argtypes = [vp, C.POINTER(ObstacleIndexInfo)]
    L.rrtx_steer_get_obstacle_index.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int64]
    L.rrtx_set_rng_state.argtypes = [vp, i32, vp, i32]
    L.rrtx_get_rng_state.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.rrtx_seed_instances.argtypes = [vp, i32, i32, vp]
    L.rrtx_set_instance.argtypes = [vp, i32, vp, vp]
    L.rrtx_set_instance_rotation.argtypes = [vp, i32, vp, C.c_double]
    L.rrtx_plan.argtypes = [vp]
    L.rrtx_get_tree.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.rrtx_get_path.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.rrtx_get_results.argtypes = [vp, vp, vp, vp]
    L.rrtx_results_device_ptr.argtypes = [vp, C.POINTER(vp), i64p]
    L.rrtx_copy_results_device.argtypes = [vp, vp, C.c_int64]
    L.rrtx_get_sobol_index.argtypes = [vp, i32, i64p]
    L.rrtx_get_yaw.argtypes = [vp, i32, vp, i32]
    L.rrtx_get_polylines.argtypes = [vp, i32, vp, i32, vp, vp, C.c_int64, i64p]
    L.rrtx_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.rrtx_enable_trace.argtypes = [vp, i32]
    L.rrtx_get_trace.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.rrtx_get_trace_kind.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.rrtx_get_sample_stream.argtypes = [vp, i32, i32, i32, vp]
    L.rrtx_get_phase_cycles.argtypes = [vp, vp]
    L.rrtx_last_error.argtypes = [vp]
    L.rrtx_last_error.restype = C.c_char_p
    L.rrtx_destroy.argtypes = [vp]
    L.rrtx_destroy.restype = None
    L.rrtx_selftest_math.argtypes = [i32, i32, vp, vp, vp, C.c_int64]
    L.rrtx_smooth_paths.argtypes = [i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp]
    L.rrtx_smooth_planned.argtypes = [vp, i32]
    L.rrtx_get_smoothed_path.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.rrtx_get_path_yaw.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.rrtx_selfcheck.argtypes = [i32, i32, vp]
    L.rrtx_set_rs_cost.argtypes = [vp, i32]
    L.rrtx_track_planned.argtypes = [vp, C.POINTER(TrackParams)]
    L.rrtx_get_track_outcome.argtypes = [vp, i32, C.POINTER(TrackOutcome)]
    L.rrtx_get_track_arrays.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32]
    L.rrtx_get_track_records.argtypes = [vp, i32, vp, vp, i32]
    L.rrtx_get_track_stats.argtypes = [vp, C.POINTER(C.c_double), i64p]
    L.rrtx_plan_many.argtypes = [vp, i32, vp]
    L.rrtx_plan_begin.argtypes = [vp]
    L.rrtx_plan_step.argtypes = [vp, C.POINTER(i32)]
    L.rrtx_set_launch_bound.argtypes = [vp, i32]
    L.rrtx_rccl_unique_id.argtypes = [vp]
    L.rrtx_rccl_init.argtypes = [vp, vp, i32, i32]
    L.rrtx_rccl_gather_results.argtypes = [vp, vp, vp, vp]
    L.rrtx_steer_solve.argtypes = [vp, i32, i32, C.c_int64, C.c_int64, vp, vp, vp, i32, C.c_double, vp, i32, i32]
    L.rrtx_steer_get_counts.argtypes = [vp, i64p, i64p]
    L.rrtx_steer_get_summary.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.rrtx_steer_get_points.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.rrtx_steer_get_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.rrtx_steer_set_obstacles.argtypes = [vp, vp, C.c_int64, C.c_double]
    L.rrtx_steer_get_hits.argtypes = [vp, vp]
    L.rrtx_steer_solve_lqr.argtypes = [vp, i32, C.c_int64, C.c_int64, vp, vp, C.c_double, C.c_double, C.c_double, i32]
    L.rrtx_steer_get_ends.argtypes = [vp, vp]
    L.rrtx_steer_solve_bezier.argtypes = [vp, i32, C.c_int64, C.c_int64, vp, vp, C.c_double, vp, i32, i32, i32]
    L.rrtx_steer_solve_bezier_cp.argtypes = [vp, C.c_int64, i32, vp, i32, i32, i32]
    L.rrtx_steer_get_curvature.argtypes = [vp, vp, C.c_int64]
    L.rrtx_steer_get_kmax.argtypes = [vp, vp]
    L.rrtx_steer_get_control_points.argtypes = [vp, vp, C.POINTER(i32)]
    L.rrtx_steer_solve_all.argtypes = L.rrtx_steer_solve.argtypes
    L.rrtx_steer_get_cand_counts.argtypes = [vp, i64p, i64p, i64p, C.POINTER(C.c_double)]
    L.rrtx_steer_get_cand_summary.argtypes = [vp] * 12
    L.rrtx_steer_get_cand_points.argtypes = [vp, vp, vp, vp, vp, C.c_int64]
    L.rrtx_steer_select_free.argtypes = [vp, vp, vp, vp]
    L.rrtx_tracker_run.argtypes = [vp, C.POINTER(TrackParams), C.POINTER(TrackBatch)]
    L.rrtx_tracker_get_counts.argtypes = [vp, i64p, i64p]
    L.rrtx_tracker_get_records.argtypes = [vp, vp, vp]
    L.rrtx_tracker_get_arrays.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64]
    L.rrtx_tracker_get_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.rrtx_tracker_run_from.argtypes = [vp, C.POINTER(TrackParams), C.POINTER(TrackSource), C.POINTER(TrackBatch)]
    L.rrtx_tracker_get_winners.argtypes = [vp, vp, i64p]
    L.rrtx_tracker_get_goals.argtypes = [vp, vp]
    L.rrtx_tracker_set_obstacle_index.argtypes = [vp, i32]
    L.rrtx_tracker_get_obstacle_index_info.argtypes = [vp, C.POINTER(ObstacleIndexInfo)]
    L.rrtx_tracker_get_obstacle_index.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int64]
    L.rrtx_gather_courses.argtypes = [vp, i32, i32]
    L.rrtx_get_course_counts.argtypes = [vp, vp, i64p, C.POINTER(i32), C.POINTER(C.c_double)]
    L.rrtx_get_courses.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.rrtx_get_course_generation.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rrtx_query_goals.argtypes = [vp, i32, i32, vp, C.c_double, C.c_double]
    L.rrtx_get_goal_query.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, i64p]
    L.rrtx_gather_goal_courses.argtypes = [vp, i32]
    L.rrtx_get_goal_course_counts.argtypes = [vp, vp, i64p, C.POINTER(i32)]
    L.rrtx_get_goal_courses.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.rrtx_get_goal_query_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rrtx_track_goals.argtypes = [vp, C.POINTER(TrackParams), i32, i32, vp, i32]
    L.rrtx_get_goal_track.argtypes = [vp, vp, vp, vp, C.c_int64, i64p, i64p, i64p]
    L.rrtx_get_goal_track_records.argtypes = [vp, vp, vp, C.c_int64]
    L.rrtx_get_goal_track_arrays.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64]
    L.rrtx_get_polyline_yaw.argtypes = [vp, i32, vp, C.c_int64]
    L.rrtx_get_goal_track_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rrtx_spline_run.argtypes = [vp, C.POINTER(SplineBatch)]
    L.rrtx_spline_get_records.argtypes = [vp, vp, vp, i64p, i64p, C.POINTER(C.c_double)]
    L.rrtx_spline_get_points.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64]
    L.rrtx_spline_get_c.argtypes = [vp, vp, vp, C.c_int64]
    L.rrtx_spline_get_hits.argtypes = [vp, vp]
    L.rrtx_spline_fit1d.argtypes = [vp, C.POINTER(SplineFit1dBatch)]
    L.rrtx_spline_query.argtypes = [vp, C.POINTER(SplineQueryBatch)]
    L.rrtx_spline_get_query.argtypes = [vp] + [vp] * 8 + [vp, C.c_int64]
    L.rrtx_spline_get_query_info.argtypes = [vp, i64p, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double)]
    L.rrtx_bspline_run.argtypes = [vp, C.POINTER(BSplineBatch)]
    L.rrtx_bspline_get_records.argtypes = [vp, vp, vp, i64p, i64p, i64p]
    L.rrtx_bspline_get_points.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64]
    L.rrtx_bspline_get_coefficients.argtypes = [vp, vp, vp, C.c_int64, vp, vp, C.c_int64]
    L.rrtx_bspline_get_hits.argtypes = [vp, vp]
    L.rrtx_bspline_get_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.rrtx_bspline_approximate.argtypes = [vp, C.POINTER(BSplineSmoothBatch)]
    L.rrtx_bspline_get_axis_records.argtypes = [vp, vp, C.c_int64]
    L.rrtx_bspline_get_axis_splines.argtypes = [vp, i32, vp, vp, C.c_int64, vp, vp, C.c_int64, i64p, i64p]
    L.rrtx_armnav_occupancy.argtypes = [vp, i32, C.c_int64, vp, vp, vp, vp]
    L.rrtx_armnav_set_grids.argtypes = [vp, i32, C.c_int64, vp]
    L.rrtx_armnav_get_grids.argtypes = [vp, vp, C.c_int64]
    L.rrtx_armnav_search.argtypes = [vp, C.c_int64, vp, vp, vp, i32]
    L.rrtx_armnav_get_counts.argtypes = [vp, vp, vp, vp, i64p, i64p]
    L.rrtx_armnav_get_routes.argtypes = [vp, vp, vp, C.c_int64]
    L.rrtx_armnav_get_marks.argtypes = [vp, vp, C.c_int64]
    L.rrtx_armnav_get_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rrtx_armik_solve.argtypes = [vp, C.POINTER(ArmIKBatch), i32, i32]
    L.rrtx_armik_move.argtypes = [vp, C.POINTER(ArmIKBatch), C.c_double, C.c_double, i32, i32]
    L.rrtx_armik_get_records.argtypes = [vp, vp, vp, vp, vp, i64p, i64p]
    L.rrtx_armik_get_angles.argtypes = [vp, vp, vp, C.c_int64]
    L.rrtx_armik_get_trajectory.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int64]
    L.rrtx_armik_get_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32)]
    L.rrtx_armdh_forward.argtypes = [vp, C.POINTER(ArmDHBatch)]
    L.rrtx_armdh_solve.argtypes = [vp, C.POINTER(ArmDHBatch), i32, C.c_double, i32, C.c_double]
    L.rrtx_armdh_get_records.argtypes = [vp, vp, vp, vp, vp, i64p, i64p]
    L.rrtx_armdh_get_angles.argtypes = [vp, vp, vp, C.c_int64]
    L.rrtx_armdh_get_transforms.argtypes = [vp, vp, C.c_int64]
    L.rrtx_armdh_get_jacobians.argtypes = [vp, vp, C.c_int64]
    L.rrtx_armdh_get_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32)]
    not_int = {"rrtx_destroy", "rrtx_last_error", "rrtx_abi_version", "rrtx_device_count"}   # the last two are set above
    for obj in DEVICE_OBJECTS:
        create, destroy, last_error, get_generation = ("rrtx_%s_%s" % (obj, f) for f in ("create", "destroy", "last_error", "get_generation"))
        getattr(L, create).argtypes = [i32, C.POINTER(vp)]
        getattr(L, destroy).argtypes = [vp]
        getattr(L, destroy).restype = None
        getattr(L, last_error).argtypes = [vp]
        getattr(L, last_error).restype = C.c_char_p
        not_int |= {destroy, last_error}
        if get_generation in EXPORTS:
            getattr(L, get_generation).argtypes = [vp, C.POINTER(C.c_uint64)]
    for f in EXPORTS:
        if f not in not_int:
            getattr(L, f).restype = C.c_int
    if L.rrtx_abi_version() != RRTX_ABI_VERSION:
        raise RrtxError("librrtx.so ABI version mismatch")
    _lib = L
    return L


def pack_instance_obstacles(lists):
    """One obstacle list of (x, y, size) rows per instance -> (offsets, oxyr): CSR as rrtx_set_instance_obstacles takes
    it, int32 offsets of len(lists) + 1 entries and float64 rows of shape (offsets[-1], 3)."""
    rows = []
    for i, lst in enumerate(lists):
        r = [[float(v) for v in o] for o in lst]
        if any(len(o) != 3 for o in r):
            raise ValueError("instance %d: every obstacle is (x, y, size)" % i)
        rows.append(np.array(r, dtype=np.float64).reshape(-1, 3))
    offsets = np.zeros(len(rows) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    oxyr = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 3)), dtype=np.float64)
    return offsets, oxyr


def unpack_instance_obstacles(offsets, oxyr):
    """Inverse of pack_instance_obstacles: one list of (x, y, size) tuples per instance."""
    return [[tuple(float(v) for v in r) for r in oxyr[offsets[i]:offsets[i + 1]]] for i in range(len(offsets) - 1)]


class RrtxParityWarning(UserWarning):
    """The host's arithmetic (libm / CPython math) is not the one the device replicas restate: results are
    self-consistent but match a reference run ON THIS HOST only up to libm's few-ULP differences."""


_selfchecked = {}
SELFCHECK_FUNCS = ("pow(x,2)", "sin", "cos", "atan2", "acos", "asin", "sqrt", "a/b", "math.hypot", "float**2")


def selfcheck(device=0, n=4096, warn=True):
    """Run-time check of the arithmetic contract, once per process and device: the device's libm
    replicas against the host's libm (rrtx_selfcheck, native), and the two CPython-specific forms -- math.hypot
    (CPython 3.10's own algorithm) and float ** 2 -- against THIS interpreter.  Returns {function: mismatches}; with
    `warn`, emits RrtxParityWarning when any is non-zero.  RRTX_SELFCHECK=0 skips the automatic call made by the first
    Handle of a process."""
    import math
    import warnings
    if device in _selfchecked:
        return _selfchecked[device]
    L = load()
    mm = np.zeros(8, dtype=np.int64)
    rc = L.rrtx_selfcheck(int(device), int(n), mm.ctypes.data)
    if rc != 0:
        raise RrtxError("rrtx_selfcheck: %s" % ERRORS.get(rc, rc))
    rng = np.random.RandomState(20240607)
    a = rng.uniform(-300.0, 300.0, n)
    b = rng.uniform(-300.0, 300.0, n)
    a[::5] /= 4096.0
    hyp = selftest_math(0, a, b, device)
    sq = selftest_math(1, a, b, device)
    res = {SELFCHECK_FUNCS[k]: int(mm[k]) for k in range(8)}
    res["math.hypot"] = int(sum(1 for i in range(n) if math.hypot(float(a[i]), float(b[i])) != float(hyp[i])))
    res["float**2"] = int(sum(1 for i in range(n) if float(a[i]) ** 2 != float(sq[i])))
    _selfchecked[device] = res
    bad = {k: v for k, v in res.items() if v}
    if bad and warn:
        warnings.warn("librrtx: device arithmetic differs from this host's on %s of %d arguments each: results are "
                      "identical to the reference only on glibc 2.35 (x86-64 FMA variants) + CPython 3.10; here they "
                      "agree to libm's few-ULP differences and integer results can differ at near-ties"
                      % (bad, n), RrtxParityWarning, stacklevel=2)
    return res


class Handle:
    """Thin RAII wrapper over rrtx_handle*."""

    def __init__(self, algo, start, goal, rand_area, expand_dis, path_resolution, goal_sample_rate, max_iter,
                 play_area=None, robot_radius=0.0, sampler=SAMPLER_MT, connect_circle_dist=50.0,
                 search_until_max_iter=False, n_instances=1, device=0, informed_rot=None, informed_c_min=0.0,
                 curvature=1.0, goal_yaw_th=0.0, goal_xy_th=0.0, step_size=0.0):
        self.L = load()
        p = Params()
        p.abi_version = RRTX_ABI_VERSION
        p.algo, p.sampler = int(algo), int(sampler)
        p.goal_sample_rate, p.max_iter = int(goal_sample_rate), int(max_iter)
        p.has_play_area = 0 if play_area is None else 1
        p.search_until_max_iter = int(bool(search_until_max_iter))
        p.n_instances, p.device = int(n_instances), int(device)
        for i in range(min(3, len(start))):
            p.start[i] = float(start[i])
        for i in range(min(3, len(goal))):
            p.goal[i] = float(goal[i])
        p.rand_min, p.rand_max = float(rand_area[0]), float(rand_area[1])
        p.expand_dis, p.path_resolution = float(expand_dis), float(path_resolution)
        if play_area is not None:
            for i in range(4):
                p.play_area[i] = float(play_area[i])
        p.robot_radius = float(robot_radius)
        p.connect_circle_dist = float(connect_circle_dist)
        if informed_rot is not None:
            for i in range(4):
                p.informed_rot[i] = float(informed_rot[i])
        p.informed_c_min = float(informed_c_min)
        p.curvature, p.goal_yaw_th, p.goal_xy_th = float(curvature), float(goal_yaw_th), float(goal_xy_th)
        p.step_size = float(step_size)
        self.params = p
        self.n_instances = int(n_instances)
        self.max_iter = int(max_iter)
        self._h = C.c_void_p()
        rc = self.L.rrtx_create(C.byref(p), C.byref(self._h))
        if rc != 0:
            msg = self.L.rrtx_last_error(self._h).decode() if self._h else ""
            if self._h:
                self.L.rrtx_destroy(self._h)
                self._h = C.c_void_p()
            raise RrtxError("rrtx_create: %s %s" % (ERRORS.get(rc, rc), msg))
        if os.environ.get("RRTX_SELFCHECK", "1") != "0" and int(device) not in _selfchecked:
            selfcheck(int(device))   # once per process and device: warns when this host's libm is not the replicated one

    def _chk(self, rc, what):
        if rc < 0:
            raise RrtxError("%s: %s %s" % (what, ERRORS.get(rc, rc), self.L.rrtx_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self.L.rrtx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_obstacles(self, obstacle_list):
        a = np.ascontiguousarray(np.array([[float(v) for v in o] for o in obstacle_list], dtype=np.float64)
                                 .reshape(-1, 3))
        self._chk(self.L.rrtx_set_obstacles(self._h, a.ctypes.data, len(a)), "rrtx_set_obstacles")

    def set_obstacle_map(self, obstacle_list):
        """Any number of circles up to 2**20 through the obstacle map (rrtx_set_obstacle_map); "rrt" / "rrt_star" and the
        Reeds-Shepp planners ("rrt_star_reeds_shepp", "closed_loop_rrt_star") only."""
        a = np.ascontiguousarray(np.array([[float(v) for v in o] for o in obstacle_list], dtype=np.float64)
                                 .reshape(-1, 3))
        self._chk(self.L.rrtx_set_obstacle_map(self._h, a.ctypes.data if len(a) else None, len(a)), "rrtx_set_obstacle_map")

    def load_obstacles(self, obstacle_list, obstacle_map=None):
        """set_obstacle_map or set_obstacles as the planners' `obstacle_map` keyword says (use_obstacle_map); returns
        whether the handle holds a map now."""
        use = use_obstacle_map(obstacle_map, len(obstacle_list))
        if use:
            self.set_obstacle_map(obstacle_list)
        else:
            self.set_obstacles(obstacle_list)
        return use

    def obstacle_map_info(self):
        """rrtx_get_obstacle_map_info as a dict."""
        info = ObstacleMapInfo()
        self._chk(self.L.rrtx_get_obstacle_map_info(self._h, C.byref(info)), "rrtx_get_obstacle_map_info")
        return {k: getattr(info, k) for k, _ in ObstacleMapInfo._fields_}

    def obstacle_map(self):
        """(cell_start[nx * ny + 1], items, wide): the map as built; items and wide are OBSTACLE_ITEM records."""
        info = self.obstacle_map_info()
        cell_start = np.zeros(info["nx"] * info["ny"] + 1, dtype=np.int32)
        items = np.zeros(info["n_items"], dtype=OBSTACLE_ITEM)
        wide = np.zeros(info["n_wide"], dtype=OBSTACLE_ITEM)
        self._chk(self.L.rrtx_get_obstacle_map(self._h, cell_start.ctypes.data, items.ctypes.data if len(items) else None,
                                               len(items), wide.ctypes.data if len(wide) else None, len(wide)),
                  "rrtx_get_obstacle_map")
        return cell_start, items, wide

    def set_instance_obstacles(self, lists):
        """One obstacle list of (x, y, size) rows per instance (rrtx_set_instance_obstacles)."""
        if len(lists) != self.n_instances:
            raise ValueError("set_instance_obstacles: %d lists for %d instances" % (len(lists), self.n_instances))
        offsets, oxyr = pack_instance_obstacles(lists)
        self._chk(self.L.rrtx_set_instance_obstacles(self._h, offsets.ctypes.data, oxyr.ctypes.data if len(oxyr) else None),
                  "rrtx_set_instance_obstacles")

    def set_rng_state(self, instance, pystate):
        """pystate = random.getstate()"""
        words = np.array(pystate[1][:624], dtype=np.uint32)
        self._chk(self.L.rrtx_set_rng_state(self._h, instance, words.ctypes.data, int(pystate[1][624])),
                  "rrtx_set_rng_state")

    def get_rng_state(self, instance, gauss_next=None):
        words = np.zeros(624, dtype=np.uint32)
        pos = C.c_int32()
        self._chk(self.L.rrtx_get_rng_state(self._h, instance, words.ctypes.data, C.byref(pos)), "rrtx_get_rng_state")
        return (3, tuple(int(w) for w in words) + (int(pos.value),), gauss_next)

    def seed_instances(self, seeds, first=0):
        s = np.ascontiguousarray(np.array([abs(int(v)) for v in seeds], dtype=np.uint64))
        self._chk(self.L.rrtx_seed_instances(self._h, first, len(s), s.ctypes.data), "rrtx_seed_instances")

    def set_instance(self, instance, start=None, goal=None):
        """Per-instance start / goal: [x, y] or, for the pose planners, [x, y, yaw] (a missing yaw keeps the ctor's)."""
        def vec(v, dflt):
            w = [float(q) for q in v]
            return (C.c_double * 3)(*(w + [float(dflt[i]) for i in range(len(w), 3)]))
        s = vec(start, self.params.start) if start is not None else None
        g = vec(goal, self.params.goal) if goal is not None else None
        self._chk(self.L.rrtx_set_instance(self._h, instance, C.cast(s, C.c_void_p) if s else None,
                                           C.cast(g, C.c_void_p) if g else None), "rrtx_set_instance")

    def set_instance_rotation(self, instance, rot4, c_min):
        r = (C.c_double * 4)(*[float(v) for v in rot4])
        self._chk(self.L.rrtx_set_instance_rotation(self._h, instance, C.cast(r, C.c_void_p), float(c_min)),
                  "rrtx_set_instance_rotation")

    def enable_trace(self, instance):
        self._chk(self.L.rrtx_enable_trace(self._h, instance), "rrtx_enable_trace")

    def plan(self, strict=False):
        """Returns 0, or RRTX_PARTIAL when some instances stopped with a status bit of ST_FAILED (the other instances
        are complete; see get_results / last_error).  Raises for errors only -- and, with strict=True (what the
        single-instance drop-in classes use), for RRTX_PARTIAL as well."""
        rc = self.L.rrtx_plan(self._h)
        self._chk(rc, "rrtx_plan")
        if rc == RRTX_PARTIAL and strict:
            raise RrtxError("rrtx_plan: %s" % self.last_error())
        return rc

    def set_launch_bound(self, iterations):
        """Iterations (BIT*: trips of plan()'s loop) one kernel launch may spend on one instance."""
        self._chk(self.L.rrtx_set_launch_bound(self._h, int(iterations)), "rrtx_set_launch_bound")

    def plan_begin(self):
        self._chk(self.L.rrtx_plan_begin(self._h), "rrtx_plan_begin")

    def plan_step(self):
        """One bounded launch; returns (return code, instances still pending).  pending == 0: the plan is complete and the
        return code is rrtx_plan's (0 or RRTX_PARTIAL).  get_results() is valid between steps."""
        n = C.c_int32()
        rc = self.L.rrtx_plan_step(self._h, C.byref(n))
        self._chk(rc, "rrtx_plan_step")
        return rc, n.value

    def rccl_init(self, unique_id, rank, world):
        """Join the RCCL communicator of a multi-process run (unique_id: the 128 bytes of `rccl_unique_id()` made by rank 0)."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.rrtx_rccl_init(self._h, C.cast(buf, C.c_void_p), int(rank), int(world)), "rrtx_rccl_init")
        self._rccl_world = int(world)

    def rccl_gather_results(self):
        """(path_cost, n_nodes, status) of ALL ranks, rank-major: one ncclAllGather of the 16-byte records, device to device."""
        n = self.n_instances * self._rccl_world
        pc = np.zeros(n); nn = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
        self._chk(self.L.rrtx_rccl_gather_results(self._h, pc.ctypes.data, nn.ctypes.data, st.ctypes.data),
                  "rrtx_rccl_gather_results")
        return pc, nn, st

    def last_error(self):
        return self.L.rrtx_last_error(self._h).decode()

    def get_tree(self, instance=0):
        n = C.c_int32()
        self._chk(self.L.rrtx_get_tree(self._h, instance, None, None, None, None, 0, C.byref(n)), "rrtx_get_tree")
        k = n.value
        x = np.zeros(k); y = np.zeros(k); cost = np.zeros(k); parent = np.zeros(k, dtype=np.int32)
        self._chk(self.L.rrtx_get_tree(self._h, instance, x.ctypes.data, y.ctypes.data, cost.ctypes.data,
                                       parent.ctypes.data, k, C.byref(n)), "rrtx_get_tree")
        return x, y, cost, parent

    def get_path(self, instance=0):
        n = C.c_int32()
        self._chk(self.L.rrtx_get_path(self._h, instance, None, 0, C.byref(n)), "rrtx_get_path")
        if n.value == 0:
            return None
        xy = np.zeros((n.value, 2))
        self._chk(self.L.rrtx_get_path(self._h, instance, xy.ctypes.data, n.value, C.byref(n)), "rrtx_get_path")
        return xy

    def get_path_yaw(self, instance=0):
        """RRTX_ALGO_RS: the yaw column of the final course (rrt_06:1643-1651), one value per point of get_path."""
        n = C.c_int32()
        self._chk(self.L.rrtx_get_path_yaw(self._h, instance, None, 0, C.byref(n)), "rrtx_get_path_yaw")
        if n.value == 0:
            return None
        yaw = np.zeros(n.value)
        self._chk(self.L.rrtx_get_path_yaw(self._h, instance, yaw.ctypes.data, n.value, C.byref(n)), "rrtx_get_path_yaw")
        return yaw

    def get_results(self):
        B = self.n_instances
        pc = np.zeros(B); nn = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
        self._chk(self.L.rrtx_get_results(self._h, pc.ctypes.data, nn.ctypes.data, st.ctypes.data),
                  "rrtx_get_results")
        return pc, nn, st

    def results_device_ptr(self):
        p = C.c_void_p(); b = C.c_int64()
        self._chk(self.L.rrtx_results_device_ptr(self._h, C.byref(p), C.byref(b)), "rrtx_results_device_ptr")
        return p.value, b.value

    def copy_results_device(self, dst_device_ptr, nbytes):
        """Result table device -> device (dst = e.g. torch tensor .data_ptr() on this handle's device)."""
        self._chk(self.L.rrtx_copy_results_device(self._h, C.c_void_p(int(dst_device_ptr)), int(nbytes)),
                  "rrtx_copy_results_device")

    def get_yaw(self, instance=0):
        n = C.c_int32()
        self._chk(self.L.rrtx_get_tree(self._h, instance, None, None, None, None, 0, C.byref(n)), "rrtx_get_tree")
        yaw = np.zeros(n.value)
        self._chk(self.L.rrtx_get_yaw(self._h, instance, yaw.ctypes.data, n.value), "rrtx_get_yaw")
        return yaw

    def get_polylines(self, instance=0):
        n = C.c_int32()
        self._chk(self.L.rrtx_get_tree(self._h, instance, None, None, None, None, 0, C.byref(n)), "rrtx_get_tree")
        tot = C.c_int64()
        self._chk(self.L.rrtx_get_polylines(self._h, instance, None, 0, None, None, 0, C.byref(tot)), "rrtx_get_polylines")
        plen = np.zeros(n.value, dtype=np.int32); px = np.zeros(tot.value); py = np.zeros(tot.value)
        self._chk(self.L.rrtx_get_polylines(self._h, instance, plen.ctypes.data, n.value, px.ctypes.data, py.ctypes.data,
                                            tot.value, C.byref(tot)), "rrtx_get_polylines")
        return plen, px, py

    def get_polyline_yaw(self, instance=0):
        """RRTX_ALGO_RS: Node.path_yaw of every node, concatenated as get_polylines concatenates path_x / path_y."""
        tot = C.c_int64()
        self._chk(self.L.rrtx_get_polylines(self._h, instance, None, 0, None, None, 0, C.byref(tot)), "rrtx_get_polylines")
        pyaw = np.zeros(tot.value)
        self._chk(self.L.rrtx_get_polyline_yaw(self._h, instance, pyaw.ctypes.data, tot.value), "rrtx_get_polyline_yaw")
        return pyaw

    # ---- closed-loop stage of rrt_10 (rrtx_track_planned) on a planned RRTX_ALGO_RS handle
    def set_rs_cost(self, mode):
        self._chk(self.L.rrtx_set_rs_cost(self._h, mode), "rrtx_set_rs_cost")

    def track_planned(self, **kw):
        """Keywords: the fields of rrtx_track_params (defaults TRACK_DEFAULTS).  Returns 0 or RRTX_PARTIAL."""
        p = dict(TRACK_DEFAULTS)
        for k, v in kw.items():
            if k not in p:
                raise TypeError("track_planned: unknown keyword %r" % k)
            p[k] = float(v)
        rc = self.L.rrtx_track_planned(self._h, C.byref(TrackParams(**p)))
        if rc != RRTX_PARTIAL:
            self._chk(rc, "rrtx_track_planned")
        return rc

    def get_track_outcome(self, instance=0):
        o = TrackOutcome()
        self._chk(self.L.rrtx_get_track_outcome(self._h, instance, C.byref(o)), "rrtx_get_track_outcome")
        return {k: int(getattr(o, k)) for k, _ in TrackOutcome._fields_}

    def get_track_arrays(self, instance=0):
        """(x, y, yaw, v, t, a, d) of the instance's best feasible roll-out, or None when there is none."""
        o = self.get_track_outcome(instance)
        if not o["flag"]:
            return None
        n = o["len"]
        arr = [np.zeros(n + 1) for _ in range(7)]
        self._chk(self.L.rrtx_get_track_arrays(self._h, instance, *[q.ctypes.data for q in arr], n + 1), "rrtx_get_track_arrays")
        return tuple(q if k < 3 else q[:n] for k, q in enumerate(arr))

    def get_track_records(self, instance=0):
        """(candidate node indices, records as a TRACK_RECORD array), in candidate order."""
        n = self.get_track_outcome(instance)["n_cand"]
        cand = np.zeros(n, dtype=np.int32)
        rec = np.zeros(n, dtype=TRACK_RECORD)
        if n:
            self._chk(self.L.rrtx_get_track_records(self._h, instance, cand.ctypes.data, rec.ctypes.data, n), "rrtx_get_track_records")
        return cand, rec

    def get_track_stats(self):
        ms, st = C.c_double(), C.c_int64()
        self._chk(self.L.rrtx_get_track_stats(self._h, C.byref(ms), C.byref(st)), "rrtx_get_track_stats")
        return dict(kernel_ms=ms.value, steps=st.value)

    def get_sobol_index(self, instance=0):
        v = C.c_int64()
        self._chk(self.L.rrtx_get_sobol_index(self._h, instance, C.byref(v)), "rrtx_get_sobol_index")
        return v.value

    def smooth_planned(self, max_iter):
        self._chk(self.L.rrtx_smooth_planned(self._h, int(max_iter)), "rrtx_smooth_planned")

    def get_smoothed_path(self, instance):
        n = C.c_int32()
        self._chk(self.L.rrtx_get_smoothed_path(self._h, instance, None, 0, C.byref(n)), "rrtx_get_smoothed_path")
        if n.value == 0:
            return None
        xy = np.zeros((n.value, 2))
        self._chk(self.L.rrtx_get_smoothed_path(self._h, instance, xy.ctypes.data, n.value, C.byref(n)),
                  "rrtx_get_smoothed_path")
        return xy

    # ---- every course of the batch in one gather on the device (rrtx_gather_courses)
    @property
    def _s(self):
        """The native object, under the name the other producers of device-resident courses use (track.pack_source)."""
        return self._h

    def gather_courses(self, which=COURSE_PLANNED, order=ORDER_PLANNING):
        self._chk(self.L.rrtx_gather_courses(self._h, int(which), int(order)), "rrtx_gather_courses")

    def generation(self):
        """Completed gathers on this handle so far (rrtx_track_source.generation)."""
        g = C.c_uint64()
        self._chk(self.L.rrtx_get_course_generation(self._h, C.byref(g)), "rrtx_get_course_generation")
        return g.value

    def get_course_counts(self):
        """(offsets (n_instances + 1,), n_points, has_yaw, kernel_ms) of the last gather."""
        off = np.zeros(self.n_instances + 1, dtype=np.int64)
        n, hy, ms = C.c_int64(), C.c_int32(), C.c_double()
        self._chk(self.L.rrtx_get_course_counts(self._h, off.ctypes.data, C.byref(n), C.byref(hy), C.byref(ms)),
                  "rrtx_get_course_counts")
        return off, n.value, bool(hy.value), ms.value

    def get_courses(self, n_points, has_yaw):
        """The flat (x, y, yaw) of the last gather; yaw is None without a yaw column."""
        x, y = np.zeros(n_points), np.zeros(n_points)
        yaw = np.zeros(n_points) if has_yaw else None
        self._chk(self.L.rrtx_get_courses(self._h, x.ctypes.data, y.ctypes.data, None if yaw is None else yaw.ctypes.data,
                                          n_points), "rrtx_get_courses")
        return x, y, yaw

    # ---- the best path to many goals from the planned trees (rrtx_query_goals)
    def query_goals(self, goals, per_instance, xy_th=None, yaw_th=None):
        """goals: (g, 3) shared, or (n_instances, g, 3) with per_instance; thresholds None = the handle's own.  Returns
        (rc, n_goals): rc 0 or RRTX_PARTIAL (a query with GOALQ_OVERFLOW)."""
        g = np.ascontiguousarray(goals, dtype=np.float64)
        n_goals = g.shape[-2]
        nan = float("nan")
        rc = self.L.rrtx_query_goals(self._h, int(n_goals), 1 if per_instance else 0, g.ctypes.data,
                                     nan if xy_th is None else float(xy_th), nan if yaw_th is None else float(yaw_th))
        self._chk(rc, "rrtx_query_goals")
        return rc, n_goals

    def get_goal_query(self, n_goals):
        """(node, cost, n_near, n_safe, status) of the last query, each (n_instances, n_goals)."""
        nq = self.n_instances * int(n_goals)
        node, near, safe, st = (np.zeros(nq, dtype=np.int32) for _ in range(4))
        cost, n = np.zeros(nq), C.c_int64()
        self._chk(self.L.rrtx_get_goal_query(self._h, node.ctypes.data, cost.ctypes.data, near.ctypes.data, safe.ctypes.data,
                                             st.ctypes.data, nq, C.byref(n)), "rrtx_get_goal_query")
        return tuple(a.reshape(self.n_instances, int(n_goals)) for a in (node, cost, near, safe, st))

    def gather_goal_courses(self, order=ORDER_PLANNING):
        self._chk(self.L.rrtx_gather_goal_courses(self._h, int(order)), "rrtx_gather_goal_courses")

    def get_goal_courses(self, n_goals):
        """(offsets (n_instances * n_goals + 1,), x, y, yaw or None) of the last gather."""
        off = np.zeros(self.n_instances * int(n_goals) + 1, dtype=np.int64)
        n, hy = C.c_int64(), C.c_int32()
        self._chk(self.L.rrtx_get_goal_course_counts(self._h, off.ctypes.data, C.byref(n), C.byref(hy)),
                  "rrtx_get_goal_course_counts")
        x, y = np.zeros(n.value), np.zeros(n.value)
        yaw = np.zeros(n.value) if hy.value else None
        self._chk(self.L.rrtx_get_goal_courses(self._h, x.ctypes.data, y.ctypes.data, None if yaw is None else yaw.ctypes.data,
                                               n.value), "rrtx_get_goal_courses")
        return off, x, y, yaw

    # ---- rrt_10's closed-loop stage for many goals from the planned trees (rrtx_track_goals)
    def track_goals(self, goals, per_instance, arrays=True, **kw):
        """goals: (g, 3) shared, or (n_instances, g, 3) with per_instance; keywords: the fields of rrtx_track_params
        (defaults TRACK_DEFAULTS).  Returns (rc, n_goals): rc 0 or RRTX_PARTIAL (a query with a refused candidate)."""
        p = dict(TRACK_DEFAULTS)
        for k, v in kw.items():
            if k not in p:
                raise TypeError("track_goals: unknown keyword %r" % k)
            p[k] = float(v)
        g = np.ascontiguousarray(goals, dtype=np.float64)
        n_goals = g.shape[-2]
        rc = self.L.rrtx_track_goals(self._h, C.byref(TrackParams(**p)), int(n_goals), 1 if per_instance else 0, g.ctypes.data,
                                     1 if arrays else 0)
        if rc != RRTX_PARTIAL:
            self._chk(rc, "rrtx_track_goals")
        return rc, n_goals

    def get_goal_track(self):
        """(outcomes (nq,) GOAL_TRACK_OUTCOME, cand_offsets (nq + 1,), arr_offsets (nq + 1,)) of the last track_goals."""
        nq, nc, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.rrtx_get_goal_track(self._h, None, None, None, 0, C.byref(nq), C.byref(nc), C.byref(ns)),
                  "rrtx_get_goal_track")
        out = np.zeros(nq.value, dtype=GOAL_TRACK_OUTCOME)
        co, ao = np.zeros(nq.value + 1, dtype=np.int64), np.zeros(nq.value + 1, dtype=np.int64)
        self._chk(self.L.rrtx_get_goal_track(self._h, out.ctypes.data, co.ctypes.data, ao.ctypes.data, nq.value, None, None, None),
                  "rrtx_get_goal_track")
        return out, co, ao

    def get_goal_track_records(self, n_candidates):
        """(candidate node indices, records as a TRACK_RECORD array) of the last track_goals, query after query."""
        cand = np.zeros(int(n_candidates), dtype=np.int32)
        rec = np.zeros(int(n_candidates), dtype=TRACK_RECORD)
        self._chk(self.L.rrtx_get_goal_track_records(self._h, cand.ctypes.data, rec.ctypes.data, int(n_candidates)),
                  "rrtx_get_goal_track_records")
        return cand, rec

    def get_goal_track_arrays(self, n_steps):
        """x, y, yaw, v, t, a, d of the last track_goals, n_steps doubles each (a query's len + 1 entries at its arr_offset)."""
        arr = [np.full(int(n_steps), np.nan, dtype=np.float64) for _ in range(7)]
        self._chk(self.L.rrtx_get_goal_track_arrays(self._h, *[q.ctypes.data for q in arr], int(n_steps)),
                  "rrtx_get_goal_track_arrays")
        return arr

    def get_goal_track_kernel_ms(self):
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self.L.rrtx_get_goal_track_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(c)), "rrtx_get_goal_track_kernel_ms")
        return a.value, b.value, c.value

    def get_goal_query_kernel_ms(self):
        s, g = C.c_double(), C.c_double()
        self._chk(self.L.rrtx_get_goal_query_kernel_ms(self._h, C.byref(s), C.byref(g)), "rrtx_get_goal_query_kernel_ms")
        return s.value, g.value

    def get_stats(self):
        s = Stats()
        self._chk(self.L.rrtx_get_stats(self._h, C.byref(s)), "rrtx_get_stats")
        return {k: getattr(s, k) for k, _ in Stats._fields_ if k != "reserved"}

    def get_phase_cycles(self):
        out = np.zeros(16, dtype=np.int64)
        self._chk(self.L.rrtx_get_phase_cycles(self._h, out.ctypes.data), "rrtx_get_phase_cycles")
        return out

    def get_trace(self):
        n = C.c_int32()
        cap = max(self.max_iter + 1, 1 << 16)
        rx = np.zeros(cap); ry = np.zeros(cap); ne = np.zeros(cap, dtype=np.int32); nn = np.zeros(cap, dtype=np.int32)
        self._chk(self.L.rrtx_get_trace(self._h, rx.ctypes.data, ry.ctypes.data, ne.ctypes.data, nn.ctypes.data, cap,
                                        C.byref(n)), "rrtx_get_trace")
        k = n.value
        return rx[:k], ry[:k], ne[:k], nn[:k]

    def get_trace_kind(self):
        """Per iteration (rrt_01 / rrt_02 / rrt_04): 0 nothing appended, 1 the extension edge itself, 2 under a chosen parent."""
        n = C.c_int32()
        cap = max(self.max_iter + 1, 1 << 16)
        kind = np.zeros(cap, dtype=np.int32)
        self._chk(self.L.rrtx_get_trace_kind(self._h, kind.ctypes.data, cap, C.byref(n)), "rrtx_get_trace_kind")
        return kind[:n.value]

    def get_sample_stream(self, instance, first, count):
        """(count, 2) samples first .. first + count - 1 of the stream the last plan of the RRT* iteration kernel drew for
        `instance` (sample i is the one iteration i consumed)."""
        out = np.zeros((count, 2))
        self._chk(self.L.rrtx_get_sample_stream(self._h, instance, first, count, out.ctypes.data), "rrtx_get_sample_stream")
        return out


class _DevObject:
    """What the wrappers of the device objects besides the planner handle share: the native pointer self._s, created by
    rrtx_<_prefix>_create and destroyed by close(), and the check that turns a negative return code into an RrtxError with
    the object's last message.  Also a context manager."""
    _prefix = None   # the C prefix: "steer" for rrtx_steer_*

    def __init__(self, device=0):
        self.L = load()
        self._s = C.c_void_p()
        rc = self._fn("create")(int(device), C.byref(self._s))
        if rc != 0:
            msg = self._fn("last_error")(self._s).decode()
            self.close()
            raise RrtxError("rrtx_%s_create: %s %s" % (self._prefix, ERRORS.get(rc, rc), msg))

    def _fn(self, name):
        return getattr(self.L, "rrtx_%s_%s" % (self._prefix, name))

    def close(self):
        if getattr(self, "_s", None):
            self._fn("destroy")(self._s)
            self._s = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            raise RrtxError("%s: %s %s" % (what, ERRORS.get(rc, rc), self._fn("last_error")(self._s).decode()))
        return rc

    # the obstacle index of the steer, spline and bspline objects (rrtx_<prefix>_set_obstacle_index)
    def set_obstacle_index(self, obstacle_index):
        """None, True or False (obstacle_index_mode)."""
        self._chk(self._fn("set_obstacle_index")(self._s, obstacle_index_mode(obstacle_index)),
                  "rrtx_%s_set_obstacle_index" % self._prefix)

    def obstacle_index_info(self):
        """rrtx_<prefix>_get_obstacle_index_info as a dict: mode, used (bool), reason (one of OBSIDX_REASONS) and the fields
        of rrtx_obstacle_map_info (zero unless used)."""
        info = ObstacleIndexInfo()
        self._chk(self._fn("get_obstacle_index_info")(self._s, C.byref(info)), "rrtx_%s_get_obstacle_index_info" % self._prefix)
        out = {"mode": info.mode, "used": bool(info.used), "reason": OBSIDX_REASONS[info.reason]}
        out.update({k: getattr(info.map, k) for k, _ in ObstacleMapInfo._fields_})
        return out


class Steer(_DevObject):
    """Thin RAII wrapper over rrtx_steer* (batched Dubins / Reeds-Shepp curves between pose pairs, LQR rollouts between
    point pairs); also a context manager.  It owns the device buffers of its solves, so repeated solves of any kind
    reuse them."""

    _prefix = "steer"

    def __init__(self, device=0):
        self.n_obstacles = 0
        super().__init__(device)

    def generation(self):
        """Completed solves of this object so far: what a DeviceCourses of its last solve carries."""
        g = C.c_uint64()
        self._chk(self.L.rrtx_steer_get_generation(self._s, C.byref(g)), "rrtx_steer_get_generation")
        return g.value

    def solve(self, kind, starts, goals, curvature, step_size, word_order=None, points=True, product=False,
              _fn="rrtx_steer_solve"):
        """starts / goals: float64 arrays (n, 3) -- product: (ns, 3) and (ng, 3); curvature: a float or one value per pair;
        word_order: None or a sequence of Dubins word indices.  Returns 0 or RRTX_PARTIAL."""
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        n_pairs = len(st) * len(go) if product else len(st)
        if not product and len(go) != len(st):
            raise ValueError("solve: %d starts for %d goals" % (len(st), len(go)))
        per_pair = np.ndim(curvature) > 0   # (np.ascontiguousarray makes a scalar 1-d)
        cv = np.ascontiguousarray(curvature, dtype=np.float64).reshape(-1)
        if per_pair and len(cv) != n_pairs:
            raise ValueError("solve: %d curvatures for %d pairs" % (len(cv), n_pairs))
        wo = None if word_order is None else np.ascontiguousarray(word_order, dtype=np.int32).reshape(-1)
        self._keep = (st, go, cv, wo)
        return self._chk(getattr(self.L, _fn)(self._s, int(kind), int(bool(product)), len(st), len(go), st.ctypes.data,
                                              go.ctypes.data, cv.ctypes.data, int(per_pair), float(step_size),
                                              None if wo is None else wo.ctypes.data, 0 if wo is None else len(wo),
                                              int(bool(points))), _fn)

    def solve_all(self, kind, starts, goals, curvature, step_size, word_order=None, points=True, product=False):
        """As solve(), for every candidate curve of every pair (rrtx_steer_solve_all); word_order may repeat a word."""
        return self.solve(kind, starts, goals, curvature, step_size, word_order=word_order, points=points, product=product,
                          _fn="rrtx_steer_solve_all")

    def cand_counts(self):
        """(pairs, candidates, candidate points, kernel ms) of the last solve_all."""
        n, m, k, ms = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        self._chk(self.L.rrtx_steer_get_cand_counts(self._s, C.byref(n), C.byref(m), C.byref(k), C.byref(ms)),
                  "rrtx_steer_get_cand_counts")
        return n.value, m.value, k.value, ms.value

    def cand_summary(self, hits=False, offsets=True):
        """dict of the last solve_all: status (n,), cand_offsets (n + 1,); per candidate pair, variant, n_seg, seg_len (m, 5),
        modes (m,) bytes, length, key; hit with hits=True and offsets (m + 1,) with offsets=True, else None."""
        n, m, _, _ = self.cand_counts()
        d = dict(status=np.zeros(n, dtype=np.int32), cand_offsets=np.zeros(n + 1, dtype=np.int64),
                 pair=np.zeros(m, dtype=np.int32), variant=np.zeros(m, dtype=np.int32), n_seg=np.zeros(m, dtype=np.int32),
                 seg_len=np.zeros((m, 5)), modes=np.zeros(m, dtype="S8"), length=np.zeros(m), key=np.zeros(m),
                 hit=np.zeros(m, dtype=np.int32) if hits else None, offsets=np.zeros(m + 1, dtype=np.int64) if offsets else None)
        order = ("status", "cand_offsets", "pair", "variant", "n_seg", "seg_len", "modes", "length", "key", "hit", "offsets")
        self._chk(self.L.rrtx_steer_get_cand_summary(self._s, *[None if d[k] is None else d[k].ctypes.data for k in order]),
                  "rrtx_steer_get_cand_summary")
        return d

    def cand_offsets(self):
        """(n + 1,) int64: pair p owns the candidates cand_offsets[p] .. cand_offsets[p + 1] - 1 (no device copy)."""
        n, _, _, _ = self.cand_counts()
        off = np.zeros(n + 1, dtype=np.int64)
        self._chk(self.L.rrtx_steer_get_cand_summary(self._s, None, off.ctypes.data, *([None] * 9)),
                  "rrtx_steer_get_cand_summary")
        return off

    def cand_points(self):
        """The flat (x, y, yaw, directions int8) of the last solve_all."""
        _, _, k, _ = self.cand_counts()
        x = np.zeros(k); y = np.zeros(k); w = np.zeros(k); d = np.zeros(k, dtype=np.int8)
        self._chk(self.L.rrtx_steer_get_cand_points(self._s, x.ctypes.data, y.ctypes.data, w.ctypes.data, d.ctypes.data, k),
                  "rrtx_steer_get_cand_points")
        return x, y, w, d

    def select_free(self):
        """rrtx_steer_select_free on the last solve_all: (rc, chosen, rank, n_free); the chosen curves are then the result
        summary(), points() and hits() serve."""
        n, _, _, _ = self.cand_counts()
        ch = np.zeros(n, dtype=np.int32); rk = np.zeros(n, dtype=np.int32); nf = np.zeros(n, dtype=np.int32)
        rc = self._chk(self.L.rrtx_steer_select_free(self._s, ch.ctypes.data, rk.ctypes.data, nf.ctypes.data),
                       "rrtx_steer_select_free")
        return rc, ch, rk, nf

    def solve_lqr(self, starts, goals, step_size, max_time=100.0, goal_dist=0.1, points=True, product=False):
        """starts / goals: float64 arrays (n, 2) -- product: (ns, 2) and (ng, 2); step_size > 0: the resampled rollout,
        0: the raw one.  Returns 0 or RRTX_PARTIAL."""
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        if not product and len(go) != len(st):
            raise ValueError("solve_lqr: %d starts for %d goals" % (len(st), len(go)))
        self._keep = (st, go)
        return self._chk(self.L.rrtx_steer_solve_lqr(self._s, int(bool(product)), len(st), len(go), st.ctypes.data,
                                                     go.ctypes.data, float(step_size), float(max_time), float(goal_dist),
                                                     int(bool(points))), "rrtx_steer_solve_lqr")

    def solve_bezier(self, starts, goals, offset, n_points=100, points=True, curvature=True, product=False):
        """starts / goals: float64 arrays (n, 3) -- product: (ns, 3) and (ng, 3); offset: a float or one value per pair."""
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        n_pairs = len(st) * len(go) if product else len(st)
        if not product and len(go) != len(st):
            raise ValueError("solve_bezier: %d starts for %d goals" % (len(st), len(go)))
        per_pair = np.ndim(offset) > 0
        of = np.ascontiguousarray(offset, dtype=np.float64).reshape(-1)
        if per_pair and len(of) != n_pairs:
            raise ValueError("solve_bezier: %d offsets for %d pairs" % (len(of), n_pairs))
        self._keep = (st, go, of)
        return self._chk(self.L.rrtx_steer_solve_bezier(self._s, int(bool(product)), len(st), len(go), st.ctypes.data,
                                                        go.ctypes.data, float(of[0]) if len(of) else 0.0,
                                                        of.ctypes.data if per_pair else None, int(n_points),
                                                        int(bool(points)), int(bool(curvature))), "rrtx_steer_solve_bezier")

    def solve_bezier_cp(self, control_points, n_points=100, points=True, curvature=True):
        """control_points: float64 array (n, m, 2), or (m, 2) for one curve."""
        cp = np.ascontiguousarray(control_points, dtype=np.float64)
        if cp.ndim == 2:
            cp = cp[None]
        if cp.ndim != 3 or cp.shape[2] != 2:
            raise ValueError("solve_bezier_cp: control_points is (n, m, 2), not %r" % (cp.shape,))
        self._keep = (cp,)
        return self._chk(self.L.rrtx_steer_solve_bezier_cp(self._s, cp.shape[0], cp.shape[1], cp.ctypes.data, int(n_points),
                                                           int(bool(points)), int(bool(curvature))),
                         "rrtx_steer_solve_bezier_cp")

    def curvature(self):
        """The flat curvature per point of the last solve, a Bezier one with points and curvature."""
        _, m = self.counts()
        k = np.zeros(m)
        self._chk(self.L.rrtx_steer_get_curvature(self._s, k.ctypes.data, m), "rrtx_steer_get_curvature")
        return k

    def kmax(self):
        """(n,) largest |curvature| per curve of the last solve, a Bezier one with curvature."""
        n, _ = self.counts()
        km = np.zeros(n)
        self._chk(self.L.rrtx_steer_get_kmax(self._s, km.ctypes.data), "rrtx_steer_get_kmax")
        return km

    def control_points(self):
        """(n, m, 2) control points of the last solve, a Bezier one."""
        n, _ = self.counts()
        m = C.c_int32()
        self._chk(self.L.rrtx_steer_get_control_points(self._s, None, C.byref(m)), "rrtx_steer_get_control_points")
        cp = np.zeros((n, m.value, 2))
        self._chk(self.L.rrtx_steer_get_control_points(self._s, cp.ctypes.data, None), "rrtx_steer_get_control_points")
        return cp

    def ends(self):
        """(n, 2) end points of the last solve, an LQR one."""
        n, _ = self.counts()
        e = np.zeros((n, 2))
        self._chk(self.L.rrtx_steer_get_ends(self._s, e.ctypes.data), "rrtx_steer_get_ends")
        return e

    def set_obstacles(self, obstacle_list, robot_radius=0.0):
        """The (x, y, size) rows every later solve tests its curves against (any number up to 2^20); an empty list turns
        the check off."""
        ob = np.ascontiguousarray(obstacle_list, dtype=np.float64).reshape(-1, 3)
        self._chk(self.L.rrtx_steer_set_obstacles(self._s, ob.ctypes.data if len(ob) else None, len(ob),
                                                  float(robot_radius)), "rrtx_steer_set_obstacles")
        self.n_obstacles = len(ob)

    def obstacle_index(self):
        """(info, cell_start, items, wide) of the index over the object's list, as Handle.obstacle_map gives the planners'."""
        info = self.obstacle_index_info()
        cell_start = np.zeros(info["nx"] * info["ny"] + 1, dtype=np.int32)
        items, wide = np.zeros(info["n_items"], dtype=OBSTACLE_ITEM), np.zeros(info["n_wide"], dtype=OBSTACLE_ITEM)
        self._chk(self.L.rrtx_steer_get_obstacle_index(self._s, cell_start.ctypes.data, items.ctypes.data if len(items) else None,
                                                       len(items), wide.ctypes.data if len(wide) else None, len(wide)),
                  "rrtx_steer_get_obstacle_index")
        return info, cell_start, items, wide

    def hits(self):
        """(n,) int32 of the last solve: -1 free, j >= 0 the first obstacle of the list the curve touches, -2 no curve."""
        n, _ = self.counts()
        hit = np.zeros(n, dtype=np.int32)
        self._chk(self.L.rrtx_steer_get_hits(self._s, hit.ctypes.data), "rrtx_steer_get_hits")
        return hit

    def counts(self):
        n, m = C.c_int64(), C.c_int64()
        self._chk(self.L.rrtx_steer_get_counts(self._s, C.byref(n), C.byref(m)), "rrtx_steer_get_counts")
        return n.value, m.value

    def summary(self, offsets=True):
        """(status, length, n_seg, seg_len (n, 5), modes (n,) bytes, offsets (n + 1,) or None) of the last solve."""
        n, _ = self.counts()
        status = np.zeros(n, dtype=np.int32); length = np.zeros(n); nseg = np.zeros(n, dtype=np.int32)
        seglen = np.zeros((n, 5)); modes = np.zeros(n, dtype="S8")
        off = np.zeros(n + 1, dtype=np.int64) if offsets else None
        self._chk(self.L.rrtx_steer_get_summary(self._s, status.ctypes.data, length.ctypes.data, nseg.ctypes.data,
                                                seglen.ctypes.data, modes.ctypes.data, off.ctypes.data if offsets else None),
                  "rrtx_steer_get_summary")
        return status, length, nseg, seglen, modes, off

    def points(self, yaw=True):
        """The flat (x, y, yaw) of the last solve; yaw=False (an LQR solve has none): (x, y, None)."""
        _, m = self.counts()
        x = np.zeros(m); y = np.zeros(m); w = np.zeros(m) if yaw else None
        self._chk(self.L.rrtx_steer_get_points(self._s, x.ctypes.data, y.ctypes.data, w.ctypes.data if yaw else None, m),
                  "rrtx_steer_get_points")
        return x, y, w

    def kernel_ms(self):
        ms = C.c_double()
        self._chk(self.L.rrtx_steer_get_kernel_ms(self._s, C.byref(ms)), "rrtx_steer_get_kernel_ms")
        return ms.value


class Tracker(_DevObject):
    """Thin RAII wrapper over rrtx_tracker* (batched closed-loop tracking of courses given as data); also a context
    manager.  It owns the device buffers of its runs, so repeated runs reuse them."""

    _prefix = "tracker"

    def set_obstacle_index(self, obstacle_index):
        """True or False (tracker_obstacle_index_mode): rrtx_tracker_set_obstacle_index takes RRTX_OBSIDX_ON and _OFF only."""
        self._chk(self.L.rrtx_tracker_set_obstacle_index(self._s, tracker_obstacle_index_mode(obstacle_index)),
                  "rrtx_tracker_set_obstacle_index")

    def obstacle_index(self):
        """(info, cell_start, items, wide) of the index that served the last run, as Steer.obstacle_index gives a steer's."""
        info = self.obstacle_index_info()
        cell_start = np.zeros(info["nx"] * info["ny"] + 1, dtype=np.int32)
        items, wide = np.zeros(info["n_items"], dtype=OBSTACLE_ITEM), np.zeros(info["n_wide"], dtype=OBSTACLE_ITEM)
        self._chk(self.L.rrtx_tracker_get_obstacle_index(self._s, cell_start.ctypes.data, items.ctypes.data if len(items) else None,
                                                         len(items), wide.ctypes.data if len(wide) else None, len(wide)),
                  "rrtx_tracker_get_obstacle_index")
        return info, cell_start, items, wide

    def run(self, params, batch):
        """params: TrackParams; batch: TrackBatch (its arrays are kept alive by the caller).  Returns 0 or RRTX_PARTIAL."""
        return self._chk(self.L.rrtx_tracker_run(self._s, C.byref(params), C.byref(batch)), "rrtx_tracker_run")

    def run_from(self, params, source, batch):
        """params: TrackParams; source: TrackSource; batch: TrackBatch without courses.  Returns 0 or RRTX_PARTIAL."""
        return self._chk(self.L.rrtx_tracker_run_from(self._s, C.byref(params), C.byref(source), C.byref(batch)),
                         "rrtx_tracker_run_from")

    def winners(self):
        """(n / group,) int32: the winning course of every group of the last run_from, -1 none."""
        g = C.c_int64()
        self._chk(self.L.rrtx_tracker_get_winners(self._s, None, C.byref(g)), "rrtx_tracker_get_winners")
        w = np.zeros(g.value, dtype=np.int32)
        self._chk(self.L.rrtx_tracker_get_winners(self._s, w.ctypes.data, None), "rrtx_tracker_get_winners")
        return w

    def goals(self, rows):
        """(rows, 3): the goal poses of the last run_from -- one per group with a group, else one per course."""
        go = np.full((rows, 3), np.nan)
        self._chk(self.L.rrtx_tracker_get_goals(self._s, go.ctypes.data), "rrtx_tracker_get_goals")
        return go

    def counts(self):
        n, m = C.c_int64(), C.c_int64()
        self._chk(self.L.rrtx_tracker_get_counts(self._s, C.byref(n), C.byref(m)), "rrtx_tracker_get_counts")
        return n.value, m.value

    def records(self):
        """(records (n,) TRACK_RECORD, arr_offsets (n + 1,)) of the last run."""
        n, _ = self.counts()
        rec = np.zeros(n, dtype=TRACK_RECORD)
        off = np.zeros(n + 1, dtype=np.int64)
        self._chk(self.L.rrtx_tracker_get_records(self._s, rec.ctypes.data, off.ctypes.data), "rrtx_tracker_get_records")
        return rec, off

    def arrays(self):
        """The seven flat arrays x, y, yaw, v, t, a, d of the last run."""
        _, m = self.counts()
        arr = [np.zeros(m) for _ in range(7)]
        self._chk(self.L.rrtx_tracker_get_arrays(self._s, *[q.ctypes.data for q in arr], m), "rrtx_tracker_get_arrays")
        return arr

    def kernel_ms(self):
        ms = C.c_double()
        self._chk(self.L.rrtx_tracker_get_kernel_ms(self._s, C.byref(ms)), "rrtx_tracker_get_kernel_ms")
        return ms.value


class Spline(_DevObject):
    """Thin RAII wrapper over rrtx_spline* (batched cubic-spline courses through waypoints); also a context manager.  It
    owns the device buffers of its runs, so repeated runs reuse them."""

    _prefix = "spline"

    def generation(self):
        """Completed solves of this object so far: what a DeviceCourses of its last solve carries."""
        g = C.c_uint64()
        self._chk(self.L.rrtx_spline_get_generation(self._s, C.byref(g)), "rrtx_spline_get_generation")
        return g.value

    def run(self, batch):
        """batch: SplineBatch (its arrays are kept alive by the caller).  Returns 0 or RRTX_PARTIAL."""
        return self._chk(self.L.rrtx_spline_run(self._s, C.byref(batch)), "rrtx_spline_run")

    def records(self):
        """(records (n,) SPLINE_RECORD, offsets (n + 1,), kernel_ms) of the last run."""
        n, m, ms = C.c_int64(), C.c_int64(), C.c_double()
        self._chk(self.L.rrtx_spline_get_records(self._s, None, None, C.byref(n), C.byref(m), C.byref(ms)),
                  "rrtx_spline_get_records")
        rec = np.zeros(n.value, dtype=SPLINE_RECORD)
        off = np.zeros(n.value + 1, dtype=np.int64)
        self._chk(self.L.rrtx_spline_get_records(self._s, rec.ctypes.data, off.ctypes.data, None, None, None),
                  "rrtx_spline_get_records")
        return rec, off, ms.value

    def points(self, m):
        """The five flat arrays x, y, yaw, k, s of the last run, m = offsets[-1] doubles each."""
        arr = [np.zeros(m) for _ in range(5)]
        self._chk(self.L.rrtx_spline_get_points(self._s, *[q.ctypes.data for q in arr], m), "rrtx_spline_get_points")
        return arr

    def c(self, w):
        """(cx, cy) as the last run used them, w = waypoints of the batch."""
        cx, cy = np.zeros(w), np.zeros(w)
        self._chk(self.L.rrtx_spline_get_c(self._s, cx.ctypes.data, cy.ctypes.data, w), "rrtx_spline_get_c")
        return cx, cy

    def hits(self, n):
        hit = np.zeros(n, dtype=np.int32)
        self._chk(self.L.rrtx_spline_get_hits(self._s, hit.ctypes.data), "rrtx_spline_get_hits")
        return hit

    def fit1d(self, batch):
        """batch: SplineFit1dBatch (its arrays are kept alive by the caller).  Returns 0 or RRTX_PARTIAL."""
        return self._chk(self.L.rrtx_spline_fit1d(self._s, C.byref(batch)), "rrtx_spline_fit1d")

    def c1d(self, w):
        """c of the last fit1d, w = knots of the batch."""
        c = np.zeros(w)
        self._chk(self.L.rrtx_spline_get_c(self._s, c.ctypes.data, None, w), "rrtx_spline_get_c")
        return c

    def query(self, batch):
        """batch: SplineQueryBatch (its arrays are kept alive by the caller).  Returns 0 or RRTX_PARTIAL."""
        return self._chk(self.L.rrtx_spline_query(self._s, C.byref(batch)), "rrtx_spline_query")

    def query_planes(self):
        """(planes, status, kernel_ms) of the last query: planes is a dict of (Q,) arrays -- x, y, yaw, k and, when asked
        for, dx, dy, ddx, ddy; y and dy, ddy after a fit1d -- and status (Q,) int32."""
        q, axes, der, ms = C.c_int64(), C.c_int32(), C.c_int32(), C.c_double()
        self._chk(self.L.rrtx_spline_get_query_info(self._s, C.byref(q), C.byref(axes), C.byref(der), C.byref(ms)),
                  "rrtx_spline_get_query_info")
        names = ("x", "y", "yaw", "k", "dx", "dy", "ddx", "ddy")
        want = (("x", "y", "yaw", "k") if axes.value == 2 else ("y",)) + \
            ((("dx", "dy", "ddx", "ddy") if axes.value == 2 else ("dy", "ddy")) if der.value else ())
        planes = {k: np.zeros(q.value) for k in want}
        status = np.zeros(q.value, dtype=np.int32)
        self._chk(self.L.rrtx_spline_get_query(self._s, *[planes[k].ctypes.data if k in planes else None for k in names],
                                               status.ctypes.data, q.value), "rrtx_spline_get_query")
        return planes, status, ms.value


class BSpline(_DevObject):
    """Thin RAII wrapper over rrtx_bspline* (batched interpolating B-spline courses through waypoints); also a context
    manager.  It owns the device buffers of its runs, so repeated runs reuse them."""

    _prefix = "bspline"

    def generation(self):
        """Completed solves of this object so far: what a DeviceCourses of its last solve carries."""
        g = C.c_uint64()
        self._chk(self.L.rrtx_bspline_get_generation(self._s, C.byref(g)), "rrtx_bspline_get_generation")
        return g.value

    def run(self, batch):
        """batch: BSplineBatch (its arrays are kept alive by the caller).  Returns 0 or RRTX_PARTIAL."""
        return self._chk(self.L.rrtx_bspline_run(self._s, C.byref(batch)), "rrtx_bspline_run")

    def records(self):
        """(records (n,) BSPLINE_RECORD, offsets (n + 1,), n_knots, kernel_ms) of the last run."""
        n, m, nk, ms = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        self._chk(self.L.rrtx_bspline_get_records(self._s, None, None, C.byref(n), C.byref(m), C.byref(nk)),
                  "rrtx_bspline_get_records")
        rec = np.zeros(n.value, dtype=BSPLINE_RECORD)
        off = np.zeros(n.value + 1, dtype=np.int64)
        self._chk(self.L.rrtx_bspline_get_records(self._s, rec.ctypes.data, off.ctypes.data, None, None, None),
                  "rrtx_bspline_get_records")
        self._chk(self.L.rrtx_bspline_get_kernel_ms(self._s, C.byref(ms)), "rrtx_bspline_get_kernel_ms")
        return rec, off, nk.value, ms.value

    def points(self, m):
        """The five flat arrays x, y, yaw, k, u of the last run, m = offsets[-1] doubles each."""
        arr = [np.zeros(m) for _ in range(5)]
        self._chk(self.L.rrtx_bspline_get_points(self._s, *[q.ctypes.data for q in arr], m), "rrtx_bspline_get_points")
        return arr

    def coefficients(self, n, n_knots, w):
        """(knot_offsets (n + 1,), knots, cx, cy) of the last run; w = waypoints of the batch."""
        koff = np.zeros(n + 1, dtype=np.int64)
        knots, cx, cy = np.zeros(n_knots), np.zeros(w), np.zeros(w)
        self._chk(self.L.rrtx_bspline_get_coefficients(self._s, koff.ctypes.data, knots.ctypes.data, n_knots, cx.ctypes.data,
                                                       cy.ctypes.data, w), "rrtx_bspline_get_coefficients")
        return koff, knots, cx, cy

    def hits(self, n):
        hit = np.zeros(n, dtype=np.int32)
        self._chk(self.L.rrtx_bspline_get_hits(self._s, hit.ctypes.data), "rrtx_bspline_get_hits")
        return hit

    def approximate(self, batch):
        """batch: BSplineSmoothBatch (its arrays are kept alive by the caller).  Returns 0 or RRTX_PARTIAL."""
        return self._chk(self.L.rrtx_bspline_approximate(self._s, C.byref(batch)), "rrtx_bspline_approximate")

    def axis_records(self, n):
        """(2, n) BSPLINE_AXIS_RECORD of the last approximate run: row 0 the x axis, row 1 the y axis."""
        rec = np.zeros((2, n), dtype=BSPLINE_AXIS_RECORD)
        self._chk(self.L.rrtx_bspline_get_axis_records(self._s, rec.ctypes.data, 2 * n), "rrtx_bspline_get_axis_records")
        return rec

    def axis_splines(self, axis, n):
        """(knot_offsets (n + 1,), knots, coef_offsets (n + 1,), coefficients) of one axis of the last approximate run."""
        nk, nc = C.c_int64(), C.c_int64()
        what = "rrtx_bspline_get_axis_splines"
        self._chk(self.L.rrtx_bspline_get_axis_splines(self._s, axis, None, None, 0, None, None, 0, C.byref(nk), C.byref(nc)), what)
        koff, coff = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        knots, coefs = np.zeros(nk.value), np.zeros(nc.value)
        self._chk(self.L.rrtx_bspline_get_axis_splines(self._s, axis, koff.ctypes.data, knots.ctypes.data, nk.value, coff.ctypes.data,
                                                       coefs.ctypes.data, nc.value, None, None), what)
        return koff, knots, coff, coefs


class ArmNav(_DevObject):
    """Thin RAII wrapper over rrtx_armnav* (batched joint-space occupancy grids of a planar arm and searches on them); also a
    context manager.  It owns the device buffers of its calls and keeps the grids of the last occupancy() / set_grids()."""

    _prefix = "armnav"

    def occupancy(self, M, link_off, link_len, obs_off, obs_xyr):
        """CSR scenes: int64 offsets of n_scenes + 1 entries, float64 lengths, float64 rows (x, y, radius)."""
        self._chk(self.L.rrtx_armnav_occupancy(self._s, int(M), len(link_off) - 1, link_off.ctypes.data, link_len.ctypes.data,
                                               obs_off.ctypes.data, obs_xyr.ctypes.data if len(obs_xyr) else None),
                  "rrtx_armnav_occupancy")

    def set_grids(self, grids):
        """grids: contiguous uint8 (n_scenes, M, M)."""
        self._chk(self.L.rrtx_armnav_set_grids(self._s, grids.shape[1], grids.shape[0], grids.ctypes.data), "rrtx_armnav_set_grids")

    def grids(self, n_scenes, M):
        out = np.zeros((n_scenes, M, M), dtype=np.uint8)
        self._chk(self.L.rrtx_armnav_get_grids(self._s, out.ctypes.data, out.size), "rrtx_armnav_get_grids")
        return out

    def search(self, scene, starts, goals, want_marks):
        """scene: int32 (n,) or None; starts / goals: contiguous int32 (n, 2)."""
        self._chk(self.L.rrtx_armnav_search(self._s, len(starts), None if scene is None else scene.ctypes.data,
                                            starts.ctypes.data if len(starts) else None, goals.ctypes.data if len(goals) else None,
                                            int(bool(want_marks))), "rrtx_armnav_search")

    def counts(self):
        """(status, n_route, pops) int32 (n,) each, of the last search."""
        n, m = C.c_int64(), C.c_int64()
        self._chk(self.L.rrtx_armnav_get_counts(self._s, None, None, None, C.byref(n), C.byref(m)), "rrtx_armnav_get_counts")
        out = [np.zeros(n.value, dtype=np.int32) for _ in range(3)]
        self._chk(self.L.rrtx_armnav_get_counts(self._s, *[q.ctypes.data for q in out], None, None), "rrtx_armnav_get_counts")
        return tuple(out) + (m.value,)

    def routes(self, n, n_cells):
        """(offsets (n + 1,) int64, cells (n_cells, 2) int32) of the last search."""
        off = np.zeros(n + 1, dtype=np.int64)
        cells = np.zeros((n_cells, 2), dtype=np.int32)
        self._chk(self.L.rrtx_armnav_get_routes(self._s, off.ctypes.data, cells.ctypes.data if n_cells else None, n_cells),
                  "rrtx_armnav_get_routes")
        return off, cells

    def marks(self, n, M):
        out = np.zeros((n, M, M), dtype=np.uint8)
        self._chk(self.L.rrtx_armnav_get_marks(self._s, out.ctypes.data, out.size), "rrtx_armnav_get_marks")
        return out

    def kernel_ms(self):
        g, s = C.c_double(), C.c_double()
        self._chk(self.L.rrtx_armnav_get_kernel_ms(self._s, C.byref(g), C.byref(s)), "rrtx_armnav_get_kernel_ms")
        return g.value, s.value


class ArmIK(_DevObject):
    """Thin RAII wrapper over rrtx_armik* (batched inverse kinematics of planar arms and the driver's P-control loop); also a
    context manager.  It owns the device buffers of its calls."""

    _prefix = "armik"

    @staticmethod
    def _batch(link_off, link_len, arm, angles, goals, goal_angles, goal_dist):
        """Contiguous arrays: int64 link_off (n_arms + 1,), float64 link_len, int32 arm (n,) or None, float64 angles (flat, query
        after query), float64 goals (n, 2), float64 goal_angles (flat) or None."""
        b = ArmIKBatch()
        b.n_arms, b.link_off, b.link_len = len(link_off) - 1, link_off.ctypes.data, link_len.ctypes.data
        b.n, b.arm = len(goals), None if arm is None else arm.ctypes.data
        b.angles, b.goals = angles.ctypes.data, goals.ctypes.data
        b.goal_angles = None if goal_angles is None else goal_angles.ctypes.data
        b.goal_dist = float(goal_dist)
        return b

    def solve(self, link_off, link_len, arm, angles, goals, goal_dist, max_iterations, waves):
        """Returns the call's code: 0, or RRTX_PARTIAL when some query was not found."""
        b = self._batch(link_off, link_len, arm, angles, goals, None, goal_dist)
        return self._chk(self.L.rrtx_armik_solve(self._s, C.byref(b), int(max_iterations), int(waves)), "rrtx_armik_solve")

    def move(self, link_off, link_len, arm, angles, goal_angles, goals, goal_dist, Kp, dt, max_steps, want_arrays):
        b = self._batch(link_off, link_len, arm, angles, goals, goal_angles, goal_dist)
        return self._chk(self.L.rrtx_armik_move(self._s, C.byref(b), float(Kp), float(dt), int(max_steps), int(bool(want_arrays))),
                         "rrtx_armik_move")

    def records(self):
        """(status int32 (n,), count int32 (n,), end (n, 2), distance (n,)) of the last run."""
        n, m = C.c_int64(), C.c_int64()
        self._chk(self.L.rrtx_armik_get_records(self._s, None, None, None, None, C.byref(n), C.byref(m)), "rrtx_armik_get_records")
        status, count = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        end, dist = np.zeros((n.value, 2)), np.zeros(n.value)
        self._chk(self.L.rrtx_armik_get_records(self._s, status.ctypes.data, count.ctypes.data, end.ctypes.data, dist.ctypes.data,
                                                None, None), "rrtx_armik_get_records")
        return status, count, end, dist, m.value

    def angles(self, n, n_angles):
        """(offsets (n + 1,) int64, angles (n_angles,)) of the last run."""
        off, ang = np.zeros(n + 1, dtype=np.int64), np.zeros(n_angles)
        self._chk(self.L.rrtx_armik_get_angles(self._s, off.ctypes.data, ang.ctypes.data if n_angles else None, n_angles),
                  "rrtx_armik_get_angles")
        return off, ang

    def trajectory(self, n):
        """(step offsets (n + 1,), angle offsets (n + 1,), angles, distance) of the last move with arrays."""
        so, ao = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        self._chk(self.L.rrtx_armik_get_trajectory(self._s, so.ctypes.data, ao.ctypes.data, None, None, 0, 0), "rrtx_armik_get_trajectory")
        ang, dist = np.zeros(int(ao[n])), np.zeros(int(so[n]))
        if len(dist):
            self._chk(self.L.rrtx_armik_get_trajectory(self._s, None, None, ang.ctypes.data, dist.ctypes.data, len(dist), len(ang)),
                      "rrtx_armik_get_trajectory")
        return so, ao, ang, dist

    def kernel_ms(self):
        ms, w = C.c_double(), C.c_int32()
        self._chk(self.L.rrtx_armik_get_kernel_ms(self._s, C.byref(ms), C.byref(w)), "rrtx_armik_get_kernel_ms")
        return ms.value, w.value


class ArmDH(_DevObject):
    """Thin RAII wrapper over rrtx_armdh* (batched forward and inverse kinematics of DH arms in 3-D); also a context manager.
    It owns the device buffers of its calls."""

    _prefix = "armdh"

    @staticmethod
    def _batch(link_off, dh, arm, angles, n, ref_pose):
        """Contiguous arrays: int64 link_off (n_arms + 1,), float64 dh (links, 4), int32 arm (n,) or None, float64 angles (flat,
        query after query) or None, float64 ref_pose (n, 6) or None."""
        b = ArmDHBatch()
        b.n_arms, b.link_off, b.dh = len(link_off) - 1, link_off.ctypes.data, dh.ctypes.data
        b.n, b.arm = int(n), None if arm is None else arm.ctypes.data
        b.angles = None if angles is None else angles.ctypes.data
        b.ref_pose = None if ref_pose is None else ref_pose.ctypes.data
        return b

    def forward(self, link_off, dh, arm, angles, n):
        """Returns the call's code: 0, or RRTX_PARTIAL when some status is not ARMDH_OK."""
        b = self._batch(link_off, dh, arm, angles, n, None)
        return self._chk(self.L.rrtx_armdh_forward(self._s, C.byref(b)), "rrtx_armdh_forward")

    def solve(self, link_off, dh, arm, angles, ref_pose, iter_cnt, step_div, method, eps):
        b = self._batch(link_off, dh, arm, angles, len(ref_pose), ref_pose)
        return self._chk(self.L.rrtx_armdh_solve(self._s, C.byref(b), int(iter_cnt), float(step_div), int(method), float(eps)),
                         "rrtx_armdh_solve")

    def records(self):
        """(status int32 (n,), values (n, 16), kappa_max (n,), n_cut int32 (n,), n_links) of the last run."""
        n, m = C.c_int64(), C.c_int64()
        self._chk(self.L.rrtx_armdh_get_records(self._s, None, None, None, None, C.byref(n), C.byref(m)), "rrtx_armdh_get_records")
        status, n_cut = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        values, kappa = np.zeros((n.value, 16)), np.zeros(n.value)
        self._chk(self.L.rrtx_armdh_get_records(self._s, status.ctypes.data, values.ctypes.data, kappa.ctypes.data, n_cut.ctypes.data,
                                                None, None), "rrtx_armdh_get_records")
        return status, values, kappa, n_cut, m.value

    def angles(self, n, n_links, want_angles=True):
        """(offsets (n + 1,) int64, angles (n_links,) or None) of the last run."""
        off = np.zeros(n + 1, dtype=np.int64)
        ang = np.zeros(n_links) if want_angles else None
        self._chk(self.L.rrtx_armdh_get_angles(self._s, off.ctypes.data, ang.ctypes.data if (want_angles and n_links) else None, n_links),
                  "rrtx_armdh_get_angles")
        return off, ang

    def transforms(self, n_links):
        t = np.zeros((n_links, 4, 4))
        self._chk(self.L.rrtx_armdh_get_transforms(self._s, t.ctypes.data if n_links else None, t.size), "rrtx_armdh_get_transforms")
        return t

    def jacobians(self, n_links):
        j = np.zeros(6 * n_links)
        self._chk(self.L.rrtx_armdh_get_jacobians(self._s, j.ctypes.data if n_links else None, j.size), "rrtx_armdh_get_jacobians")
        return j

    def kernel_ms(self):
        ms, w = C.c_double(), C.c_int32()
        self._chk(self.L.rrtx_armdh_get_kernel_ms(self._s, C.byref(ms), C.byref(w)), "rrtx_armdh_get_kernel_ms")
        return ms.value, w.value


def rccl_unique_id():
    """The 128-byte ncclUniqueId of a new communicator (rank 0 makes it and hands it to the other ranks)."""
    L = load()
    buf = (C.c_char * 128)()
    rc = L.rrtx_rccl_unique_id(C.cast(buf, C.c_void_p))
    if rc != 0:
        raise RrtxError("rrtx_rccl_unique_id: %s (librccl.so not loadable?)" % ERRORS.get(rc, rc))
    return bytes(buf)


def plan_many(handles, strict=False):
    """rrtx_plan_many: plans the handles concurrently, one native host thread each (one handle per device = multi-GPU in
    one process).  Returns the per-handle return codes (0 / RRTX_PARTIAL); raises on an error of any of them."""
    L = load()
    n = len(handles)
    arr = (C.c_void_p * n)(*[h._h for h in handles])
    rcs = (C.c_int32 * n)()
    rc = L.rrtx_plan_many(C.cast(arr, C.c_void_p), n, C.cast(rcs, C.c_void_p))
    for h, r in zip(handles, rcs):
        h._chk(int(r), "rrtx_plan_many")
    if rc < 0:
        raise RrtxError("rrtx_plan_many: %s" % ERRORS.get(rc, rc))
    if strict and rc == RRTX_PARTIAL:
        raise RrtxError("rrtx_plan_many: %s" % "; ".join(h.last_error() for h, r in zip(handles, rcs) if r == RRTX_PARTIAL))
    return [int(r) for r in rcs]


def smooth_paths(paths, max_iter, obstacles, rng_states, device=0):
    """Batched path_smoothing (rrt_04:1447-1479) on the GPU.  paths: list of (n_i, 2) arrays; rng_states: list of
    (mt624 uint32 array, pos).  Returns (list of smoothed (k_i, 2) arrays, list of advanced (mt624, pos), status array)."""
    L = load()
    nj = len(paths)
    stride_in = max(2, max(len(p) for p in paths))
    pin = np.zeros((nj, stride_in, 2))
    pn = np.zeros(nj, dtype=np.int32)
    for j, p in enumerate(paths):
        a = np.asarray(p, dtype=np.float64).reshape(-1, 2)
        pin[j, :len(a)] = a
        pn[j] = len(a)
    obst = np.ascontiguousarray(np.asarray(obstacles, dtype=np.float64).reshape(-1, 3))
    words = np.ascontiguousarray(np.stack([np.asarray(s[0], dtype=np.uint32)[:624] for s in rng_states]))
    pos = np.array([int(s[1]) for s in rng_states], dtype=np.int32)
    stride_out = stride_in + int(max_iter) + 2
    stride_out = min(stride_out, 512)
    out = np.zeros((nj, stride_out, 2))
    on = np.zeros(nj, dtype=np.int32)
    st = np.zeros(nj, dtype=np.int32)
    rc = L.rrtx_smooth_paths(int(device), nj, pin.ctypes.data, pn.ctypes.data, stride_in, int(max_iter),
                             obst.ctypes.data, len(obst), words.ctypes.data, pos.ctypes.data, out.ctypes.data,
                             stride_out, on.ctypes.data, st.ctypes.data)
    if rc != 0:
        raise RrtxError("rrtx_smooth_paths: %s (status %s)" % (ERRORS.get(rc, rc), st.tolist()))
    return [out[j, :on[j]].copy() for j in range(nj)], [(words[j].copy(), int(pos[j])) for j in range(nj)], st


def selftest_math(op, a, b, device=0):
    L = load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    out = np.zeros((5,) + a.shape if op == 13 else a.shape, dtype=np.float64)   # op 13: five results per element (rrtx.h)
    rc = L.rrtx_selftest_math(device, op, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size)
    if rc != 0:
        raise RrtxError("rrtx_selftest_math: %s" % ERRORS.get(rc, rc))
    return out

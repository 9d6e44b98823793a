"""Importable alias of the `robotics-path-planning_amd` package (hyphenated directory name).

Per-script drop-in modules: `rrt_amd.rrt_01` ... `rrt_amd.rrt_10` carry exactly the names the reference script of that
number defines for its driver cell (`RRT`, `BITStar`, `Node`, `path_smoothing`, `get_path_length`), so a driver written
against `10_path_planning_01_rrt_04_rrt_star.py` runs after `from rrt_amd.rrt_04 import *`.  `rrt_amd.dubins_path`, `rrt_amd.reeds_shepp_path`
and `rrt_amd.lqr_path` do the same for the three stand-alone steering scripts (`plan_dubins_path`, `reeds_shepp_path_planning`,
`LQRPlanner`), `rrt_amd.reeds_shepp_calc_paths` for the Reeds-Shepp script's `calc_paths` and `Path` (every candidate curve), `rrt_amd.cubic_spline_path` for the cubic-spline script (`calc_spline_course`, `CubicSpline1D`, `CubicSpline2D`), `rrt_amd.bspline_path` and
`rrt_amd.spline_2d` for the two scipy spline scripts (`interpolate_b_spline_path` and its helpers; `Spline2D`), `rrt_amd.bspline_path_smoothing`
for the same B-spline script with its smoothing fit (`approximate_b_spline_path` for any `s`), `rrt_amd.bazier_path` for the
Bezier script (`calc_4points_bezier_path`, `calc_bezier_path` and its pointwise helpers), `rrt_amd.arm_obstacle_navigation` for the
arm script (`NLinkArm`, `get_occupancy_grid`, `astar_torus` and its helpers), `rrt_amd.simple_2d_inverse_kinematics` for the two
planar inverse-kinematics scripts (`inverse_kinematics`, `forward_kinematics`, `jacobian_inverse`, `NLinkArm` and their helpers),
`rrt_amd.forward_inverse_kinematics` and `rrt_amd.forward_inverse_kinematics_orig` for the two DH-arm scripts (`forward_kinematics`,
`inverse_kinematics`, the pose functions; `Link`, `NLinkArm`)."""
import importlib
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _root not in sys.path:
    sys.path.insert(0, _root)
_pkg = importlib.import_module("robotics-path-planning_amd")
_abi = _pkg._abi
planner = importlib.import_module("robotics-path-planning_amd.planner")
steer = importlib.import_module("robotics-path-planning_amd.steer")
track = importlib.import_module("robotics-path-planning_amd.track")
spline = importlib.import_module("robotics-path-planning_amd.spline")
bspline = importlib.import_module("robotics-path-planning_amd.bspline")
armnav = importlib.import_module("robotics-path-planning_amd.armnav")
armik = importlib.import_module("robotics-path-planning_amd.armik")
armdh = importlib.import_module("robotics-path-planning_amd.armdh")
RRT = _pkg.RRT
RRTStar = _pkg.RRTStar
RRTSobol = _pkg.RRTSobol
RRTStarDubins = _pkg.RRTStarDubins
RRTDubins = _pkg.RRTDubins
RRTStarReedsShepp = _pkg.RRTStarReedsShepp
path_smoothing = _pkg.path_smoothing
BITStar = _pkg.BITStar
bitstar_rotation = _pkg.bitstar_rotation
InformedRRTStar = _pkg.InformedRRTStar
LQRRRTStar = _pkg.LQRRRTStar
ClosedLoopRRTStar = _pkg.ClosedLoopRRTStar
informed_rotation = _pkg.informed_rotation
BatchPlanner = _pkg.BatchPlanner
PlannerCourses = _pkg.PlannerCourses
GoalQueryResult = _pkg.GoalQueryResult
GoalTrackResult = _pkg.GoalTrackResult
BatchSteer = _pkg.BatchSteer
SteerCandidates = _pkg.SteerCandidates
BatchTrack = _pkg.BatchTrack
BatchSpline = _pkg.BatchSpline
SplineQueryResult = _pkg.SplineQueryResult
BatchBSpline = _pkg.BatchBSpline
BSplineResult = _pkg.BSplineResult
BSplineSmoothResult = _pkg.BSplineSmoothResult
BatchArmNav = _pkg.BatchArmNav
BatchArmIK = _pkg.BatchArmIK
ArmIKResult = _pkg.ArmIKResult
ArmMoveResult = _pkg.ArmMoveResult
BatchArmDH = _pkg.BatchArmDH
ArmDHResult = _pkg.ArmDHResult
ArmDHForward = _pkg.ArmDHForward
Node = _pkg.Node
AreaBounds = _pkg.AreaBounds
get_path_length = _pkg.get_path_length
InformedNode = planner.InformedNode
DubinsNode = planner.DubinsNode

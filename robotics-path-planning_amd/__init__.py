"""MI355X-native batched RRT / RRT* planner (host mirror of the reference classes).

The directory name carries a hyphen (it mirrors the upstream repository name), so
import it with importlib, or through the `rrt_amd` shim at the repository root:

    import rrt_amd                       # == importlib.import_module("robotics-path-planning_amd")
    rrt = rrt_amd.RRTStar(start, goal, obstacle_list, rand_area, ...)
    path = rrt.planning(animation=False)

Submodules: planner (RRT = rrt_01's class, RRTStar = rrt_04's class, BatchPlanner), steer (BatchSteer: batched Dubins /
Reeds-Shepp curves between pose pairs), track (BatchTrack: batched closed-loop tracking of courses given as data),
spline (BatchSpline: batched cubic-spline courses through waypoints, the step from a path to a course, and pointwise queries
at the caller's parameters),
bspline (BatchBSpline: batched interpolating and smoothing B-spline courses of degree 1 .. 5, the reference's two scipy scripts),
armnav (BatchArmNav: batched joint-space occupancy grids of a planar arm and searches on the torus grid),
armik (BatchArmIK: batched Jacobian inverse kinematics of planar arms and the P-control move to the angles found),
armdh (BatchArmDH: batched forward kinematics, Jacobians and 6-DoF inverse kinematics of DH arms in 3-D),
_abi (ctypes binding of include/rrtx.h), csrc/ (HIP kernels + C ABI sources).
"""
from . import _abi  # noqa: F401
from .planner import (RRT, RRTSobol, RRTStar, RRTStarDubins, RRTDubins, RRTStarReedsShepp, BITStar, bitstar_rotation, InformedRRTStar, LQRRRTStar, ClosedLoopRRTStar, BatchPlanner, PlannerCourses, GoalQueryResult, GoalTrackResult, Node, AreaBounds, get_path_length, path_smoothing,  # noqa: F401
                      informed_rotation)
from .steer import BatchSteer, SteerCandidates  # noqa: F401
from .track import BatchTrack  # noqa: F401
from .spline import BatchSpline, SplineQueryResult  # noqa: F401
from .bspline import BatchBSpline, BSplineResult, BSplineSmoothResult  # noqa: F401
from .armnav import BatchArmNav  # noqa: F401
from .armik import BatchArmIK, ArmIKResult, ArmMoveResult  # noqa: F401
from .armdh import BatchArmDH, ArmDHResult, ArmDHForward  # noqa: F401

__all__ = ["RRT", "RRTSobol", "RRTStar", "RRTStarDubins", "RRTDubins", "RRTStarReedsShepp", "BITStar", "InformedRRTStar", "LQRRRTStar", "ClosedLoopRRTStar", "BatchPlanner", "PlannerCourses", "GoalQueryResult", "GoalTrackResult", "BatchSteer", "SteerCandidates", "BatchTrack", "BatchSpline", "SplineQueryResult", "BatchBSpline", "BSplineResult", "BSplineSmoothResult", "BatchArmNav", "BatchArmIK", "ArmIKResult", "ArmMoveResult", "BatchArmDH", "ArmDHResult", "ArmDHForward", "Node", "AreaBounds", "get_path_length", "path_smoothing"]

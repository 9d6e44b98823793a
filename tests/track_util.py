"""Shared helpers of the closed-loop RRT* (rrt_10) tests: golden loading and the course of a candidate."""
import glob
import json
import os

import numpy as np

import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
PORDER = ["target_speed", "yaw_th", "xy_th", "invalid_travel_ratio", "dt", "L", "steer_max", "accel_max", "Kp", "Lf", "T",
          "goal_dis", "stop_speed"]
# which golden shows which branch of rrt_10 (kept by tools/gen_golden_closed_loop.py only when the reference shows it):
#   drv_s0 .. drv_s7  the driver cell; all return flag=True, every one has candidates refused for the final angle (fail
#                     bit 2), s1 / s3 / s4 / s6 / s7 hold roll-outs that ran to the time limit (len(t) = 2002, bit 1)
#   none_s9           no candidate: the (False, None, ...) tuple
#   coll_s2, coll_s3  robot_radius > 0 with an obstacle on the tracked path: roll-outs refused for collision (bit 8);
#                     coll_s3 also starts away from the origin and every candidate is refused: flag=False WITH candidates
#   long_s4           invalid_travel_ratio = 1.0: "path is too long" (bit 4)
#   yaw_s6            yaw_th = 0.3 deg: "final angle is bad" (bit 2) on nearly every candidate
#   gyaw_s5 / s15 / s16   goal yaw 180 / 180 / -179 deg: the tracked yaw wraps, candidates that reach the goal are refused for the
#                     final angle alone (fail = 2); s5 and s16 return (False, None, ...) with candidates, s15 flag=True
#   start_s7          a start pose away from the origin (the roll-out still starts at (-0.0, -0.0, 0, 0))
#   map_a_s11, map_b_s12   two maps for the per-instance-obstacle batch
BRANCH_GOLDENS = {1: "rrt10_drv_s7", 2: "rrt10_drv_s5", 4: "rrt10_long_s4", 8: "rrt10_coll_s2"}


def goldens():
    return sorted(glob.glob(os.path.join(GOLD, "rrt10_*.npz")))


def load(path):
    g = np.load(path)
    kw = json.loads(str(g["kwargs"]))
    model = json.loads(str(g["model"]))
    return g, kw, model


def course(g, node, kw):
    """The course of check_tracking_path_is_feasible in driving order: start, polylines root -> node, goal."""
    par = g["parent"]
    off = np.concatenate([[0], np.cumsum(g["plen"])])
    chain, nd = [], int(node)
    while par[nd] >= 0:
        chain.append(nd)
        nd = int(par[nd])
    cx, cy, cw = [kw["start"][0]], [kw["start"][1]], [kw["start"][2]]
    for nd in reversed(chain):
        a, b = off[nd], off[nd + 1]
        cx += list(g["px"][a:b])
        cy += list(g["py"][a:b])
        cw += list(g["pyaw"][a:b])
    cx.append(kw["goal"][0])
    cy.append(kw["goal"][1])
    cw.append(kw["goal"][2])
    return cx, cy, cw


def job(params, obstacles, robot_radius, cx, cy, cw):
    obs = [[o[0], o[1], (o[2] + robot_radius) ** 2] for o in obstacles]
    return np.concatenate([[params[q] for q in PORDER], [len(obs)], np.array(obs, dtype=np.float64).reshape(-1),
                           [len(cx)], cx, cy, cw]).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)

"""Shared by tests/test_lqr_steer_host.py and tests/test_gpu_lqr_steer.py -- TEST INFRASTRUCTURE: the expected values of
a batched LQR steer, from tests/lqr_oracle.py (exact fused row 0, CPython's math.hypot) with MAX_TIME and GOAL_DIST as
arguments, and the known-answer files."""
import math
import os

import numpy as np

import lqr_oracle
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
_cache = {}


def kat(name):
    """tests/golden/<name>.npz as a dict of arrays, loaded once and never written."""
    if name not in _cache:
        with np.load(os.path.join(GOLD, name + ".npz")) as g:
            _cache[name] = {k: g[k] for k in g.files}
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rollout(sx, sy, gx, gy, max_time=100.0, goal_dist=0.1):
    """lqr_planning (10_path_planning_00_lqr_path.py :24-66) with the planner's two attributes as arguments; the step is
    lqr_oracle's."""
    rx, ry = [sx], [sy]
    x0, x1 = sx - gx, sy - gy
    time = 0.0
    while time <= max_time:
        time += 0.1
        u = -(lqr_oracle.K[0] * x0 + lqr_oracle.K[1] * x1)
        x0, x1 = lqr_oracle.fma(0.1, x0, x1) + 0.0 * u, (0.0 * x0 + 0.1 * x1) + u
        rx.append(x0 + gx)
        ry.append(x1 + gy)
        if math.hypot(gx - rx[-1], gy - ry[-1]) <= goal_dist:
            return rx, ry
    return [], []


def hypot_sum(x, y):
    """Python's left-to-right sum of math.hypot over consecutive points"""
    return float(sum([math.hypot(x[j + 1] - x[j], y[j + 1] - y[j]) for j in range(len(x) - 1)]))


def expected(pair, step, max_time=100.0, goal_dist=0.1):
    """What one pair of a batch must give: dict(n_seg, x, y, end, length); step None: the raw rollout."""
    sx, sy, gx, gy = (float(v) for v in pair)
    wx, wy = rollout(sx, sy, gx, gy, max_time, goal_dist)
    if not wx:
        return dict(n_seg=0, x=[], y=[], end=(0.0, 0.0), length=0.0)
    if step is None:
        return dict(n_seg=len(wx), x=wx, y=wy, end=(wx[-1], wy[-1]), length=hypot_sum(wx, wy))
    px, py, cl = lqr_oracle.sample_path(wx, wy, step)
    return dict(n_seg=len(wx), x=px, y=py, end=(px[-1], py[-1]), length=float(sum(cl)))


def first_hit(x, y, obs, robot_radius):
    """rrt_09's check_collision :1292-1305, called with growing lists: -1, or the first obstacle at which it refuses."""
    for j, (ox, oy, size) in enumerate(obs):
        d = [(ox - a) * (ox - a) + (oy - b) * (oy - b) for a, b in zip(x, y)]
        if min(d) <= (size + robot_radius) ** 2:
            return j
    return -1

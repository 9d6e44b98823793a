"""Plain-Python restatement of the Bezier script (10_path_planning_00_bazier_path.py) as BatchSteer("bezier") defines its
results, one statement per rounding:

    control points   calc_4points_bezier_path :25-30 -- np.hypot (glibc's hypot, not CPython's), math.cos / math.sin
    parameters       np.linspace(0, 1, n) :46 -- k * (1.0 / (n - 1)), the last entry 1.0
    weight           bernstein_poly :61 -- (float(C(n, i)) * pow(t, i)) * pow(1.0 - t, n - i), libm pow for every exponent
    point            bezier :72-73 -- per axis 0.0 + w_0 P_0 + w_1 P_1 + ..., left to right (np.sum over rows starts from
                     its identity 0.0: a sum of nothing but -0.0 is +0.0)
    derivatives      bezier_derivatives_control_points :89-94 -- float(n) * (P_j+1 - P_j), subtract then multiply; dx, dy,
                     ddx, ddy are the point form on those control points
    curvature        :107 -- (dx ddy - dy ddx) / pow(pow(dx, 2.0) + pow(dy, 2.0), 1.5); numpy's nan / inf for a zero
                     denominator

and this package's own definitions, which the script has no counterpart for: yaw = math.atan2(dy, dx), length = the
left-to-right sum of math.hypot over consecutive points, kmax = np.max(np.abs(k)).
No scipy: scipy.special.comb(n, i) is float(math.comb(n, i)).  All values are Python floats."""
import math

import numpy as np


def linspace(n):
    step = 1.0 / (n - 1)
    return [k * step for k in range(n - 1)] + [1.0]


def weight(n, i, t):
    return (float(math.comb(n, i)) * math.pow(t, float(i))) * math.pow(1.0 - t, float(n - i))


def control_points4(sx, sy, syaw, ex, ey, eyaw, offset):
    """The four control points as a list of (x, y)"""
    dist = float(np.hypot(np.float64(sx - ex), np.float64(sy - ey))) / offset
    return [(sx, sy),
            (sx + dist * math.cos(syaw), sy + dist * math.sin(syaw)),
            (ex - dist * math.cos(eyaw), ey - dist * math.sin(eyaw)),
            (ex, ey)]


def point(t, cps):
    """bezier(t, control_points) -> (x, y)"""
    n = len(cps) - 1
    x = y = 0.0
    for i, (px, py) in enumerate(cps):
        w = weight(n, i, t)
        x = x + w * px
        y = y + w * py
    return x, y


def derivative_cps(cps):
    """The control points of the derivative curve"""
    n = float(len(cps) - 1)
    return [(n * (cps[j + 1][0] - cps[j][0]), n * (cps[j + 1][1] - cps[j][1])) for j in range(len(cps) - 1)]


def div(num, den):
    """num / den as a numpy double divides"""
    if den != 0.0:
        return num / den
    return math.nan if (num == 0.0 or num != num) else math.copysign(math.inf, num) * math.copysign(1.0, den)


def curvature(dx, dy, ddx, ddy):
    return div(dx * ddy - dy * ddx, math.pow(math.pow(dx, 2.0) + math.pow(dy, 2.0), 1.5))


def curve(cps, n_points=100):
    """dict(x, y, dx, dy, ddx, ddy, yaw, k: lists of n_points floats; length, kmax: floats; cp: the control points)"""
    cps = [(float(a), float(b)) for a, b in cps]
    d1 = derivative_cps(cps)
    d2 = derivative_cps(d1)
    out = {key: [] for key in ("x", "y", "dx", "dy", "ddx", "ddy", "yaw", "k")}
    for t in linspace(n_points):
        x, y = point(t, cps)
        dx, dy = point(t, d1)
        ddx, ddy = point(t, d2)
        for key, v in (("x", x), ("y", y), ("dx", dx), ("dy", dy), ("ddx", ddx), ("ddy", ddy)):
            out[key].append(v)
        out["yaw"].append(math.atan2(dy, dx))
        out["k"].append(curvature(dx, dy, ddx, ddy))
    length = 0.0
    for i in range(1, n_points):
        length = length + math.hypot(out["x"][i] - out["x"][i - 1], out["y"][i] - out["y"][i - 1])
    out["length"] = length
    out["kmax"] = float(np.max(np.abs(np.array(out["k"]))))
    out["cp"] = cps
    return out


def curve4(sx, sy, syaw, ex, ey, eyaw, offset, n_points=100):
    return curve(control_points4(float(sx), float(sy), float(syaw), float(ex), float(ey), float(eyaw), float(offset)),
                 n_points)


def first_hit(xs, ys, obstacles, robot_radius):
    """check_collision of the pose planners (rrt_05 :1625-1638) as BatchSteer reports it: the first circle of the list
    that any point touches, else -1"""
    for j, (ox, oy, size) in enumerate(obstacles):
        thr = (size + robot_radius) ** 2
        for px, py in zip(xs, ys):
            dx, dy = ox - px, oy - py
            if dx * dx + dy * dy <= thr:
                return j
    return -1


def batch(curves):
    """The flat form BatchSteer returns for a list of curve() dicts with one n_points: dict(x, y, yaw, k, dx, dy, ddx, ddy
    flat arrays; length, kmax (n,); cp (n, m, 2); offsets)"""
    out = {key: np.array([v for c in curves for v in c[key]], dtype=np.float64)
           for key in ("x", "y", "yaw", "k", "dx", "dy", "ddx", "ddy")}
    out["length"] = np.array([c["length"] for c in curves], dtype=np.float64)
    out["kmax"] = np.array([c["kmax"] for c in curves], dtype=np.float64)
    out["cp"] = np.array([c["cp"] for c in curves], dtype=np.float64).reshape(len(curves), -1, 2)
    off = np.zeros(len(curves) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c["x"]) for c in curves])
    out["offsets"] = off
    return out

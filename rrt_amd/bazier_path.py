"""Names of 10_path_planning_00_bazier_path.py as its driver cell uses them.  The MI355X mirror: calc_4points_bezier_path
and calc_bezier_path are a batch of one on robotics-path-planning_amd/steer.py (same arguments, same return shapes and
types, the script's doubles bit for bit); no CPU fallback.  The pointwise helpers (bernstein_poly, bezier,
bezier_derivatives_control_points, curvature) are host arithmetic: a point at an arbitrary t needs no device.  No scipy:
the binomial coefficient is math.comb."""
import math

import numpy as np

from . import steer as _s

_steer = None


def _bs():
    global _steer
    if _steer is None:
        _steer = _s.BatchSteer("bezier")
    return _steer


def calc_4points_bezier_path(sx, sy, syaw, ex, ey, eyaw, offset):
    """(path (100, 2), control_points (4, 2)) between the poses (sx, sy, syaw) and (ex, ey, eyaw)."""
    res = _bs().plan([[sx, sy, syaw]], [[ex, ey, eyaw]], offset=float(offset), curvature=False)
    return res.path(0)


def calc_bezier_path(control_points, n_points=100):
    """The (n_points, 2) points of the curve over control_points (m, 2), 3 <= m <= 16."""
    res = _bs().plan_control_points(np.asarray(control_points, dtype=np.float64)[None], n_points=n_points, curvature=False)
    return res.path(0)[0]


def bernstein_poly(n, i, t):
    """C(n, i) t^i (1 - t)^(n - i)"""
    return float(math.comb(n, i)) * t ** i * (1 - t) ** (n - i)


def bezier(t, control_points):
    """The point at parameter t in [0, 1] of the curve over control_points, as an array (x, y)."""
    cps = np.asarray(control_points, dtype=np.float64)
    deg = len(cps) - 1
    return np.sum([bernstein_poly(deg, i, t) * cps[i] for i in range(deg + 1)], axis=0)


def bezier_derivatives_control_points(control_points, n_derivatives):
    """{0: control_points, 1: those of the first derivative, ..., n_derivatives: ...}: the derivative of a Bezier curve
    of degree n is the Bezier curve over n * (P[j + 1] - P[j])."""
    w = {0: control_points}
    for d in range(n_derivatives):
        cur = np.asarray(w[d])
        w[d + 1] = (len(cur) - 1) * np.diff(cur, axis=0)
    return w


def curvature(dx, dy, ddx, ddy):
    """Signed curvature from the first and second derivatives at one point"""
    return (dx * ddy - dy * ddx) / (dx ** 2 + dy ** 2) ** (3 / 2)


__all__ = ['calc_4points_bezier_path', 'calc_bezier_path', 'bernstein_poly', 'bezier',
           'bezier_derivatives_control_points', 'curvature']

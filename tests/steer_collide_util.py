"""Shared by the obstacle-check tests of BatchSteer: the golden rows, the C oracle's curve of a row, and check_collision
(rrt_05:1625-1638 = rrt_06:1749-1762) evaluated in IEEE doubles the way the reference writes it."""
import os

import numpy as np

import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
WORDS = ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")


def load_kat():
    g = np.load(os.path.join(GOLD, "steer_collide_kat.npz"))
    return {f: g[f] for f in g.files}


def obstacle_list(g, l):
    return g["ob"][int(g["ob_off"][l]):int(g["ob_off"][l + 1])]


def thresholds(obs, rr):
    """Packed (ox, oy, thr) rows, thr = (size + robot_radius) ** 2 as Python computes it (:1635)."""
    out = np.array(obs, dtype=np.float64).reshape(-1, 3).copy()
    out[:, 2] = [(float(s) + float(rr)) ** 2 for s in out[:, 2]]
    return out


def oracle_curve(kind, inp):
    """(x, y) of the C oracle for a golden row (kind "d": 7 columns, "r": 8), or None where there is no curve."""
    import oracle
    a = [float(v) for v in inp]
    if kind == "d":
        px, py, _, _, _ = oracle.dubins(*a, cap=16384)
        return px, py
    try:
        px, py, _, _, _ = oracle.reeds_shepp(*a)
    except (ZeroDivisionError, ValueError):
        return None
    return None if px is None else (px, py)


def ref_hit(xy, obs, rr):
    """-2 / -1 / the first obstacle at which the reference's loop returns False.  numpy's float64 subtract, multiply and
    add are the IEEE operations of Python's floats, one rounding each (no fused multiply-add across ufuncs)."""
    if xy is None:
        return -2
    x, y = np.asarray(xy[0], dtype=np.float64), np.asarray(xy[1], dtype=np.float64)
    t = thresholds(obs, rr)
    if len(t) == 0 or len(x) == 0:
        return -1
    dx, dy = t[:, 0:1] - x[None, :], t[:, 1:2] - y[None, :]
    touched = np.nonzero(np.min(dx * dx + dy * dy, axis=1) <= t[:, 2])[0]
    return int(touched[0]) if len(touched) else -1

"""Shared by tests/test_spline_host.py and tests/test_gpu_spline.py -- TEST INFRASTRUCTURE: the known-answer file of
BatchSpline (tools/gen_golden_spline.py), its courses in the forms the tests hand around, and the oracle's answers for
them, each computed once and never written."""
import os

import numpy as np

import spline_oracle
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
_cache = {}

# The largest gap between solve="device" (the Thomas recurrence) and the reference's np.linalg.solve allowed on the courses
# of spline_kat.npz: 16 x the gap measured when the file was generated (5.68e-14, 2.22e-15, 4.82e-15), the margin covering
# a file regenerated on another host.  x / y absolute, yaw modulo 2 pi, curvature relative to max(1, |k|).
TOL_XY, TOL_YAW, TOL_K = 9.1e-13, 3.6e-14, 7.7e-14


def kat():
    """tests/golden/spline_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "spline_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def courses():
    """The golden courses as a list of (x, y) arrays"""
    g = kat()
    wo = g["wp_off"]
    return [(g["wp_x"][wo[i]:wo[i + 1]], g["wp_y"][wo[i]:wo[i + 1]]) for i in range(len(wo) - 1)]


def given_c():
    """The reference's (sx.c, sy.c) per golden course"""
    g = kat()
    wo = g["wp_off"]
    return [(g["cx"][wo[i]:wo[i + 1]], g["cy"][wo[i]:wo[i + 1]]) for i in range(len(wo) - 1)]


def oracle(solver):
    """spline_oracle.batch over the golden courses with their ds: solver "thomas", "numpy" or "given" (the golden's c)"""
    key = "oracle_" + solver
    if key not in _cache:
        _cache[key] = spline_oracle.batch(courses(), kat()["ds"], given_c() if solver == "given" else solver)
    return _cache[key]


def gaps(x, y, yaw, k):
    """(xy, yaw, k) worst gaps of flat arrays against the golden's"""
    g = kat()
    dyaw = np.abs(np.asarray(yaw) - g["ryaw"]) % (2.0 * np.pi)
    dyaw = np.minimum(dyaw, 2.0 * np.pi - dyaw)
    return (float(max(np.max(np.abs(np.asarray(x) - g["rx"])), np.max(np.abs(np.asarray(y) - g["ry"])))),
            float(np.max(dyaw)),
            float(np.max(np.abs(np.asarray(k) - g["rk"]) / np.maximum(1.0, np.abs(g["rk"])))))


def assert_same(got, want, what, keys=("x", "y", "yaw", "k", "s")):
    """got: a SplineResult, want: a dict of spline_oracle.batch (or the same keys): bit for bit"""
    assert np.array_equal(got.offsets, want["offsets"]), what
    for key in keys:
        a, b = bits(getattr(got, key)), bits(want[key])
        assert a.shape == b.shape, (what, key)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (what, key, len(bad), int(bad[0]))


def random_courses(seed, n, lo=2, hi=40):
    """n seeded courses of lo .. hi waypoints, chords of 0.5 .. 2.5, and a ds per course"""
    rs = np.random.RandomState(seed)
    out, ds = [], []
    for i in range(n):
        m = int(rs.randint(lo, hi + 1))
        th = np.cumsum(rs.uniform(-1.0, 1.0, m)) + rs.uniform(0, 2 * np.pi)
        step = rs.uniform(0.5, 2.5, m)
        out.append((np.cumsum(step * np.cos(th)) + rs.uniform(-20, 20), np.cumsum(step * np.sin(th)) + rs.uniform(-20, 20)))
        ds.append([0.1, 0.2, 0.25, 0.5][i % 4])
    return out, np.array(ds)

"""Shared by tests/test_spline_query_host.py and tests/test_gpu_spline_query.py -- TEST INFRASTRUCTURE: the known-answer file
of BatchSpline.query / fit1d (tools/gen_golden_spline_query.py), its splines and parameters in the forms the tests hand
around, and the oracle's answers for them, each computed once and never written."""
import os

import numpy as np

import spline_query_oracle as QO
import util
from spline_util import bits  # noqa: F401

GOLD = os.path.join(util.ROOT, "tests", "golden")
_cache = {}

# golden key of each plane
KEYS2 = dict(x="rx", y="ry", yaw="ryaw", k="rk", dx="rdx", dy="rdy", ddx="rddx", ddy="rddy")
KEYS1 = dict(y="p_y", dy="p_dy", ddy="p_ddy")

# The largest gap between the default solve (the Thomas recurrence) and the reference's np.linalg.solve allowed on the
# queries of spline_query_kat.npz, 2-D and 1-D together: 16 x the gap measured when the file was generated (7.11e-15,
# 2.22e-15, 4.57e-15, 1.78e-15, 3.55e-15), the margin covering a file regenerated on another host.  Position
# absolute, yaw modulo 2 pi, curvature and the first and second derivatives relative to max(1, |value|).
TOL_POS, TOL_YAW, TOL_K, TOL_D1, TOL_D2 = 1.2e-13, 3.6e-14, 7.4e-14, 2.9e-14, 5.7e-14


def kat():
    """tests/golden/spline_query_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "spline_query_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def _rows(off, *flat):
    return [tuple(a[off[i]:off[i + 1]] for a in flat) for i in range(len(off) - 1)]


def courses():
    """The golden's 2-D courses as a list of (x, y) arrays"""
    g = kat()
    return _rows(g["wp_off"], g["wp_x"], g["wp_y"])


def given_c():
    """The reference's (sx.c, sy.c) per golden course"""
    g = kat()
    return _rows(g["wp_off"], g["cx"], g["cy"])


def splines():
    """The golden's 1-D splines as a list of (knots, values) arrays"""
    g = kat()
    return _rows(g["k_off"], g["knots"], g["values"])


def given_c1():
    """The reference's c per golden 1-D spline"""
    g = kat()
    return [r[0] for r in _rows(g["k_off"], g["c1"])]


def oracle2(solver):
    """spline_query_oracle.batch over the golden courses and their parameters: solver "thomas", "numpy" or "given" (the golden's c)"""
    key = "o2_" + solver
    if key not in _cache:
        g = kat()
        fits = [QO.fit2d(x, y, given_c()[i] if solver == "given" else solver) for i, (x, y) in enumerate(courses())]
        _cache[key] = QO.batch(fits, g["q_off"], g["q_t"])
    return _cache[key]


def oracle1(solver):
    """The same over the golden's 1-D splines"""
    key = "o1_" + solver
    if key not in _cache:
        g = kat()
        fits = [QO.fit1d(kn, va, given_c1()[i] if solver == "given" else solver) for i, (kn, va) in enumerate(splines())]
        _cache[key] = QO.batch(fits, g["p_off"], g["p_t"])
    return _cache[key]


def _rel(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(a) - b) / np.maximum(1.0, np.abs(b))
    return float(np.nanmax(d)) if len(d) else 0.0


def gaps(two, one):
    """(position, yaw, k, first, second) worst gaps to the golden of `two` (the planes of the 2-D queries) and `one` (of the
    1-D queries): dicts or objects with the planes as flat arrays.  Queries the golden does not answer (NaN) do not count:
    their statuses are compared elsewhere."""
    g = kat()

    def get(o, k):
        return np.asarray(o[k] if isinstance(o, dict) else getattr(o, k))
    with np.errstate(invalid="ignore"):
        pos = max(float(np.nanmax(np.abs(get(two, "x") - g["rx"]))), float(np.nanmax(np.abs(get(two, "y") - g["ry"]))),
                  float(np.nanmax(np.abs(get(one, "y") - g["p_y"]))))
        dyaw = np.abs(get(two, "yaw") - g["ryaw"]) % (2.0 * np.pi)
        dyaw = float(np.nanmax(np.minimum(dyaw, 2.0 * np.pi - dyaw)))
    return (pos, dyaw, _rel(get(two, "k"), g["rk"]),
            max(_rel(get(two, "dx"), g["rdx"]), _rel(get(two, "dy"), g["rdy"]), _rel(get(one, "dy"), g["p_dy"])),
            max(_rel(get(two, "ddx"), g["rddx"]), _rel(get(two, "ddy"), g["rddy"]), _rel(get(one, "ddy"), g["p_ddy"])))


def gaps_of_thomas():
    return gaps(oracle2("thomas"), oracle1("thomas"))


def assert_planes(got, want, what, names, status="status"):
    """got: a SplineQueryResult (or a dict), want: a dict of spline_query_oracle.batch, or the golden with `names` (plane
    -> key of want) and its status key: statuses equal, every plane bit for bit (NaN payloads aside: a NaN is a NaN)"""
    def get(o, k):
        return np.asarray(o[k] if isinstance(o, dict) else getattr(o, k))
    assert np.array_equal(get(got, "status"), want[status]), what
    for plane, key in names.items():
        a, b = get(got, plane), np.asarray(want[key])
        assert a.shape == b.shape, (what, plane)
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan), (what, plane, "NaN where the other has a value")
        bad = np.nonzero((bits(a) != bits(b)) & ~nan)[0]
        assert len(bad) == 0, (what, plane, len(bad), int(bad[0]))

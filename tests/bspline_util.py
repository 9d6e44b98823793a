"""Shared by tests/test_bspline_host.py and tests/test_gpu_bspline.py -- TEST INFRASTRUCTURE: the known-answer file of
BatchBSpline (tools/gen_golden_bspline.py), its courses in the forms the tests hand around, and the oracle's answers for them,
each computed once and never written."""
import os

import numpy as np

import bspline_oracle as O
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
_cache = {}
LINSPACE, ARANGE, EXPLICIT = 0, 1, 2

# The largest gap between this package's definition (tests/bspline_oracle.py, bit-identical to the device) and the reference's
# scipy on the courses of bspline_kat.npz, per degree, measured when the file was generated: the coefficients relative to
# max(1, |c|), x / y absolute, yaw modulo 2 pi, curvature relative to max(1, |k|).  Degrees 1 .. 5; spline_2d returns x and y
# only and has degrees 1 .. 3 (its degree 1 is bit for bit, hence 0; degree 1 of bspline_path has the waypoints themselves as
# coefficients on both sides and no curvature).  The figures of degree 3 and of spline_2d's degree 2 come from the courses
# with coordinates near 1e4, where one ULP of a position is 1.8e-12.  The tests allow MARGIN x the figure: the reference's
# side moves by a few ULP with another BLAS or FITPACK build (the margin of 5.14).
MARGIN = 16.0
GAP_BSP = {
    "c": {1: 0.0, 2: 2.14e-15, 3: 4.23e-15, 4: 7.77e-15, 5: 1.71e-14},
    "xy": {1: 1.78e-15, 2: 1.14e-13, 3: 7.28e-12, 4: 5.68e-14, 5: 5.68e-14},
    "yaw": {1: 4.33e-15, 2: 2.20e-14, 3: 5.58e-12, 4: 2.13e-14, 5: 2.26e-13},
    "k": {1: 0.0, 2: 1.12e-12, 3: 1.88e-10, 4: 8.93e-13, 5: 4.94e-12},
}
GAP_S2D = {
    "c": {2: 3.33e-16, 3: 1.33e-15},
    "xy": {1: 0.0, 2: 3.64e-12, 3: 7.11e-15},
}


def kat():
    """tests/golden/bspline_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "bspline_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def select(script):
    """The indices of the golden courses of script 0 (bspline_path) or 1 (spline_2d)"""
    return np.nonzero(kat()["script"] == script)[0]


def courses(idx):
    g = kat()
    wo = g["wp_off"]
    return [(g["wp_x"][wo[i]:wo[i + 1]], g["wp_y"][wo[i]:wo[i + 1]]) for i in idx]


def gold(idx, key, off="pt_off"):
    """The golden's flat array `key` restricted to the courses idx (off: the CSR it lies in)"""
    g = kat()
    o = g[off]
    parts = [g[key][o[i]:o[i + 1]] for i in idx]
    return np.concatenate(parts) if parts else np.zeros(0)


def samples(idx):
    """The explicit sample lists of the courses idx: the golden's ru where the mode is EXPLICIT, else None"""
    g = kat()
    return [g["ru"][g["pt_off"][i]:g["pt_off"][i + 1]] if g["mode"][i] == EXPLICIT else None for i in idx]


def run_kwargs(script):
    """The keywords of BatchBSpline.interpolate (script 0) or .spline2d (script 1) that run the golden courses of that
    script in one batch, and of bspline_oracle.batch likewise: (courses, device keywords, oracle keywords)"""
    g, idx = kat(), select(script)
    us = samples(idx)
    deg = g["degree"][idx]
    if script == 0:
        cnt = np.maximum(g["count"][idx], 1)    # a placeholder where the samples are data
        return courses(idx), dict(n_path_points=cnt, degree=deg, u=us), dict(degree=deg, param=O.NORMALISED, n_path_points=cnt, u=us)
    ds = np.where(g["ds"][idx] > 0.0, g["ds"][idx], 1.0)
    kinds = [{1: "linear", 2: "quadratic", 3: "cubic"}[int(k)] for k in deg]
    return courses(idx), dict(ds=ds, kind=kinds, u=us), dict(degree=deg, param=O.CHORD, ds=ds, u=us)


def oracle(script):
    """The oracle's batch over the golden courses of one script"""
    key = "oracle_%d" % script
    if key not in _cache:
        crs, _, kw = run_kwargs(script)
        _cache[key] = O.batch(crs, **kw)
    return _cache[key]


def gaps(script, got):
    """{quantity: {degree: worst gap}} of `got` (a BSplineResult or an oracle batch dict over the golden courses of the
    script) against the golden's recorded reference"""
    g, idx = kat(), select(script)
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    cx, cy = (got["cx"], got["cy"]) if isinstance(got, dict) else got.coefficients
    off = get("offsets")
    wo = np.concatenate([[0], np.cumsum(np.diff(g["wp_off"])[idx])])
    out = {q: {} for q in (("c", "xy", "yaw", "k") if script == 0 else ("c", "xy"))}

    def worst(q, k, v):
        out[q][k] = max(out[q].get(k, 0.0), float(v))
    for j, i in enumerate(idx):
        k = int(g["degree"][i])
        a, b = int(off[j]), int(off[j + 1])
        pa, pb = int(g["pt_off"][i]), int(g["pt_off"][i + 1])
        assert b - a == pb - pa, (i, b - a, pb - pa)
        worst("xy", k, max(np.max(np.abs(get("x")[a:b] - g["rx"][pa:pb])), np.max(np.abs(get("y")[a:b] - g["ry"][pa:pb]))))
        if script == 0 or k > 1:
            ws, we = int(g["wp_off"][i]), int(g["wp_off"][i + 1])
            for mine, ref in ((cx[wo[j]:wo[j + 1]], g["cx"][ws:we]), (cy[wo[j]:wo[j + 1]], g["cy"][ws:we])):
                worst("c", k, np.max(np.abs(mine - ref) / np.maximum(1.0, np.abs(ref))))
        if script == 0:
            dyaw = np.abs(get("yaw")[a:b] - g["ryaw"][pa:pb]) % (2.0 * np.pi)
            worst("yaw", k, np.max(np.minimum(dyaw, 2.0 * np.pi - dyaw)))
            rk = g["rk"][pa:pb]
            worst("k", k, np.max(np.abs(get("k")[a:b] - rk) / np.maximum(1.0, np.abs(rk))))
    return out


def within(script, got, what):
    """Asserts the gaps of `got` within MARGIN x the written figures; returns them"""
    seen = gaps(script, got)
    table = GAP_BSP if script == 0 else GAP_S2D
    for q, per in seen.items():
        for k, v in per.items():
            assert v <= MARGIN * table[q][k], (what, q, k, v, table[q][k])
    return seen


ARRAYS = ("x", "y", "yaw", "k", "u")


def assert_same(got, want, what, keys=ARRAYS, spline=True):
    """got: a BSplineResult, want: a dict of bspline_oracle.batch: records, and with `spline` knots and coefficients, and
    the arrays named, bit for bit"""
    assert np.array_equal(got.status, want["status"]), what
    assert np.array_equal(got.degree, want["degree"]), what
    assert np.array_equal(got.n_points, want["n_points"]), what
    assert np.array_equal(bits(got.length), bits(want["length"])), what
    assert np.array_equal(got.offsets, want["offsets"]), what
    if spline:
        assert np.array_equal(got.knot_offsets, want["knot_offsets"]) and np.array_equal(got.wp_offsets, want["wp_offsets"]), what
        for a, b, name in ((got.knots, want["knots"], "knots"), (got.coefficients[0], want["cx"], "cx"), (got.coefficients[1], want["cy"], "cy")):
            assert np.array_equal(bits(a), bits(b)), (what, name)
    for key in keys:
        a, b = bits(getattr(got, key)), bits(want[key])
        assert a.shape == b.shape, (what, key)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (what, key, len(bad), int(bad[0]))


def random_courses(seed, n, lo=2, hi=40):
    """n seeded courses of lo .. hi waypoints with chords of 0.5 .. 2.5, a degree 1 .. 5 and a point count per course"""
    rs = np.random.RandomState(seed)
    out, deg, cnt = [], [], []
    for i in range(n):
        m = int(rs.randint(lo, hi + 1))
        th = np.cumsum(rs.uniform(-1.0, 1.0, m)) + rs.uniform(0, 2 * np.pi)
        step = rs.uniform(0.5, 2.5, m)
        out.append((np.cumsum(step * np.cos(th)) + rs.uniform(-20, 20), np.cumsum(step * np.sin(th)) + rs.uniform(-20, 20)))
        deg.append(1 + i % 5)
        cnt.append([1, 2, 37, 100][i % 4])
    return out, np.array(deg, dtype=np.int32), np.array(cnt, dtype=np.int64)

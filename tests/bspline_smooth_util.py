"""Shared by tests/test_bspline_smooth_host.py and tests/test_gpu_bspline_smooth.py -- TEST INFRASTRUCTURE: the known-answer
file of BatchBSpline.approximate (tools/gen_golden_bspline_smooth.py), the batch the tests run (its courses and a few corners),
and the oracle's answers for it, each computed once and never written."""
import os

import numpy as np

import bspline_smooth_oracle as S
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
_cache = {}

# The largest gap between this package's definition (tests/bspline_smooth_oracle.py, bit-identical to the device) and the
# reference's scipy on the courses of bspline_smooth_kat.npz, per degree, measured when the file was generated: the
# coefficients relative to max(1, |c|), x / y absolute, yaw modulo 2 pi, curvature relative to max(1, |k|).  The knot vectors
# are equal bit for bit on every axis.  Degrees 1 and 2 have coefficients equal to scipy's bit for bit on these courses (the
# rotations are FITPACK's in FITPACK's order, and the basis values of these degrees round alike on both sides), hence 0.0;
# degree 1 has the same x and y and no curvature on either side.  The tests allow MARGIN x the figure: the reference's side
# moves by a few ULP with another BLAS or FITPACK build (the margin of 5.14 and 5.19).
MARGIN = 16.0
GAP = {
    "c": {1: 0.0, 2: 0.0, 3: 1.84e-14, 4: 1.10e-13, 5: 5.43e-14},
    "xy": {1: 0.0, 2: 3.55e-15, 3: 8.53e-14, 4: 1.14e-13, 5: 4.26e-13},
    "yaw": {1: 2.50e-15, 2: 6.66e-15, 3: 2.62e-13, 4: 5.69e-13, 5: 2.49e-14},
    "k": {1: 0.0, 2: 1.71e-13, 3: 3.73e-12, 4: 1.15e-11, 5: 6.27e-12},
}


def kat():
    """tests/golden/bspline_smooth_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "bspline_smooth_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def golden_batch():
    """(courses, degree, s, count) of the golden courses; s holds None where the script's default was passed"""
    g = kat()
    wo = g["wp_off"]
    crs = [(g["wp_x"][wo[i]:wo[i + 1]], g["wp_y"][wo[i]:wo[i + 1]]) for i in range(len(g["degree"]))]
    s = [None if np.isnan(v) else float(v) for v in g["s"]]
    return crs, [int(v) for v in g["degree"]], s, [int(v) for v in g["count"]]


def corners():
    """(courses, degree, s, count): what the golden file cannot hold -- statuses other than OK, s == 0, the smallest
    courses, one point and two points per course"""
    rs = np.random.RandomState(77)

    def walk(m, scale=2.0):
        th = np.cumsum(rs.normal(0.0, 0.5, m)) + rs.uniform(0, 2 * np.pi)
        step = scale * rs.uniform(0.5, 1.5, m)
        return np.cumsum(step * np.cos(th)) + rs.uniform(-5, 5), np.cumsum(step * np.sin(th)) + rs.uniform(-5, 5)
    crs, deg, s, cnt = [], [], [], []

    def add(c, k, sv, n):
        crs.append(c)
        deg.append(k)
        s.append(sv)
        cnt.append(n)
    for k in range(1, 6):                        # s == 0 beside the others: the interpolating spline
        add(walk(9 + k), k, 0.0, 50)
    add(walk(64), 3, 0.0, 37)
    x, y = walk(8)
    x[4], y[4] = x[3], y[3]
    add((x, y), 3, 0.5, 50)                      # DEGENERATE: two consecutive waypoints coincide
    add((np.full(5, 1.5), np.full(5, -2.0)), 2, None, 50)     # DEGENERATE: all waypoints equal
    add(walk(3), 3, 0.5, 50)                     # TOO_FEW
    add(walk(5), 5, None, 50)                    # TOO_FEW
    add(walk(2), 1, 0.5, 50)                     # m = k + 1 = 2: the smallest course there is
    add(walk(2), 1, 0.0, 3)
    for k in range(1, 6):                        # one and two points; s between the polynomial's fp and the interpolant's
        add(walk(12, 0.3), k, 1.0e-4, 1 + k % 2)
    for k in range(1, 6):
        add(walk(40), k, [0.05, None, 2.0, 0.5, 1.0][k - 1], 50)
    add(([0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]), 3, 0.5, 50)   # a straight line: fp0 is rounding only
    # the paths of the root search and of the knot loop that the courses above do not take (test_oracle_paths_are_all_taken
    # holds each of them to its path)
    add(branch_course(), 4, 0.5, 50)             # "p too small" with a finite bracket: p / 0.04 passes p3 and is pulled back
    add(([-1.71, -3.32, -4.61, -5.49, -7.3, -7.53, -7.89], [-1.12, -2.63, -3.08, -3.63, -5.82, -8.75, -10.73]), 3, 1.0e-7, 50)   # ier 3 on x
    add(([0.69, 0.85, 1.29, 0.59, 2.3, 4.45, 6.65, 8.07, 9.28, 9.48, 10.34, 11.82],
         [-2.04, -3.94, -5.57, -7.31, -9.47, -10.42, -10.4, -8.87, -6.81, -5.51, -4.35, -3.86]), 1, 1.0e-9, 50)               # ier 3 on y
    tiny = ([0.0, 1.1, 2.3, 2.9, 4.2, 5.0, 5.4], [0.3, 1.2, 0.7, -0.4, 0.1, 1.5, 2.2])
    add(tiny, 3, 1.0e-40, 50)                    # s below the interpolant's rounding: a root search that ends on ier 2
    # s equal to the fp of x's second knot round (one interior knot; neither depends on s): accepted inside the knot loop
    x, y = walk(14)
    u = S.B.parameter(x.tolist(), y.tolist(), S.B.NORMALISED)
    k, m = 3, len(x)
    t = [0.0] * (m + k + 2)
    c, z, fpint, nrdata = [0.0] * (m + 1), [0.0] * (m + 1), [0.0] * (m + 1), [0] * (m + 1)
    A, q = [[0.0] * (k + 1) for _ in range(m + 1)], [[0.0] * (k + 1) for _ in range(m)]
    n = 2 * k + 2
    for j in range(k + 1):
        t[j], t[n - 1 - j] = u[0], u[m - 1]
    S.least_squares(u, x.tolist(), t, n, k, A, z, q, c)
    S.interval_sums(u, x.tolist(), t, n, k, q, c, fpint)
    nrdata[0] = m - 2
    n = S.add_knot(u, t, n, k, fpint, nrdata, 1)
    for j in range(k + 1):
        t[n - 1 - j] = u[m - 1]
    add((x, y), k, S.least_squares(u, x.tolist(), t, n, k, A, z, q, c), 50)
    return crs, deg, s, cnt


def branch_course():
    """The course of DESIGN 5.21's root-search finding: draw 328 of seed 5 (16 waypoints; degree 4, s = 0.5)"""
    rs = np.random.RandomState(5)
    for ci in range(329):
        m = int(rs.randint(4, 60))
        th = np.cumsum(rs.normal(0, 0.5, m)) + rs.uniform(0, 6.28)
        step = rs.uniform(0.5, 2.5, m)
    return np.cumsum(step * np.cos(th)), np.cumsum(step * np.sin(th))


def full_batch():
    """The golden courses and then the corners, as one batch: (courses, degree, s, count, number of golden courses)"""
    a, b = golden_batch(), corners()
    return a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3], len(a[0])


def oracle_full():
    """bspline_smooth_oracle.batch over full_batch()"""
    if "oracle" not in _cache:
        crs, deg, s, cnt, _ = full_batch()
        _cache["oracle"] = S.batch(crs, n_path_points=cnt, degree=deg, s=s)
    return _cache["oracle"]


def axis_of(got, a):
    """dict(knots, knot_offsets, coefficients, coef_offsets, ier, fp, p, rounds, iters) of axis a of an oracle batch or of a
    BSplineSmoothResult"""
    if isinstance(got, dict):
        return got["axis%d" % a]
    return {key: getattr(got, key)[a] for key in ("knots", "knot_offsets", "coefficients", "coef_offsets", "ier", "fp", "p",
                                                  "rounds", "iters")}


def gaps(got, n_gold):
    """{quantity: {degree: worst gap}} of the first n_gold courses of `got` (an oracle batch or a BSplineSmoothResult whose
    batch begins with the golden courses) against the golden's recorded reference; the knot vectors must be equal"""
    g = kat()
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    off = get("offsets")
    out = {q: {} for q in ("c", "xy", "yaw", "k")}

    def worst(q, k, v):
        out[q][k] = max(out[q].get(k, 0.0), float(v))
    for a, name in enumerate("xy"):
        ax = axis_of(got, a)
        for i in range(n_gold):
            k = int(g["degree"][i])
            ka, kb = int(g["knot_off_" + name][i]), int(g["knot_off_" + name][i + 1])
            t = ax["knots"][ax["knot_offsets"][i]:ax["knot_offsets"][i + 1]]
            assert np.array_equal(bits(t), bits(g["knots_" + name][ka:kb])), ("knots", name, i)
            ref = g["coefs_" + name][g["coef_off_" + name][i]:g["coef_off_" + name][i + 1]]
            mine = ax["coefficients"][ax["coef_offsets"][i]:ax["coef_offsets"][i + 1]]
            assert len(mine) == len(ref), ("coefficients", name, i)
            worst("c", k, np.max(np.abs(mine - ref) / np.maximum(1.0, np.abs(ref))))
    for i in range(n_gold):
        k = int(g["degree"][i])
        a, b = int(off[i]), int(off[i + 1])
        pa, pb = int(g["pt_off"][i]), int(g["pt_off"][i + 1])
        assert b - a == pb - pa, (i, b - a, pb - pa)
        worst("xy", k, max(np.max(np.abs(get("x")[a:b] - g["rx"][pa:pb])), np.max(np.abs(get("y")[a:b] - g["ry"][pa:pb]))))
        dyaw = np.abs(get("yaw")[a:b] - g["ryaw"][pa:pb]) % (2.0 * np.pi)
        worst("yaw", k, np.max(np.minimum(dyaw, 2.0 * np.pi - dyaw)))
        rk = g["rk"][pa:pb]
        worst("k", k, np.max(np.abs(get("k")[a:b] - rk) / np.maximum(1.0, np.abs(rk))))
    return out


def within(got, n_gold, what):
    """Asserts the gaps of `got` within MARGIN x the written figures; returns them"""
    seen = gaps(got, n_gold)
    for q, per in seen.items():
        for k, v in per.items():
            assert v <= MARGIN * GAP[q][k], (what, q, k, v, GAP[q][k])
    return seen


ARRAYS = ("x", "y", "yaw", "k", "u")


def assert_same(got, want, what, keys=ARRAYS, sel=None):
    """got: a BSplineSmoothResult, want: a dict of bspline_smooth_oracle.batch (restricted to the courses sel, in that
    order, when given): records, axis records, knots, coefficients, and the arrays named, bit for bit"""
    idx = np.arange(len(want["status"])) if sel is None else np.asarray(sel)
    assert len(got) == len(idx), what
    for key in ("status", "degree", "n_points"):
        assert np.array_equal(getattr(got, key), want[key][idx]), (what, key, getattr(got, key), want[key][idx])
    assert np.array_equal(bits(got.length), bits(want["length"][idx])), what

    def pick(flat, off):
        parts = [flat[off[i]:off[i + 1]] for i in idx]
        return np.concatenate(parts) if parts else np.zeros(0)
    assert np.array_equal(got.offsets, np.concatenate([[0], np.cumsum(want["n_points"][idx])])), what
    for a in (0, 1):
        w, g = want["axis%d" % a], axis_of(got, a)
        for key in ("ier", "rounds", "iters"):
            assert np.array_equal(g[key], w[key][idx]), (what, a, key, g[key], w[key][idx])
        for key in ("fp", "p"):
            assert np.array_equal(bits(g[key]), bits(w[key][idx])), (what, a, key)
        assert np.array_equal(np.diff(g["knot_offsets"]), np.diff(w["knot_offsets"])[idx]), (what, a, "knot counts")
        assert np.array_equal(np.diff(g["coef_offsets"]), np.diff(w["coef_offsets"])[idx]), (what, a, "coefficient counts")
        assert np.array_equal(bits(g["knots"]), bits(pick(w["knots"], w["knot_offsets"]))), (what, a, "knots")
        assert np.array_equal(bits(g["coefficients"]), bits(pick(w["coefficients"], w["coef_offsets"]))), (what, a, "coefficients")
    for key in keys:
        a, b = bits(getattr(got, key)), bits(pick(want[key], want["offsets"]))
        assert a.shape == b.shape, (what, key)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (what, key, len(bad), int(bad[0]))

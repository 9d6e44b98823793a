"""Shared by tests/test_bezier_host.py and tests/test_gpu_bezier.py -- TEST INFRASTRUCTURE: the known-answer file of
BatchSteer("bezier") (tools/gen_golden_bezier.py), its curves grouped the way the tests solve them, and the oracle's answers
for them, each computed once and never written."""
import os

import numpy as np

import bezier_oracle
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
TAGS = ("driver", "random", "n_points", "same_pose", "axis_yaw", "negative_offset", "far", "signed_zero", "collinear",
        "degree")
POINT_KEYS = ("x", "y", "dx", "dy", "ddx", "ddy", "k")
_cache = {}


def kat():
    """tests/golden/bezier_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "bezier_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Bit for bit, with NaN equal to NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def assert_same(a, b, what):
    if not same(a, b):
        a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
        assert a.shape == b.shape, (what, a.shape, b.shape)
        bad = np.nonzero((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b)))[0]
        raise AssertionError("%s: %d of %d differ, first at %d: %r != %r" % (what, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))


def n_pose():
    return len(kat()["pose"])


def control_points(i):
    """The golden's control points of curve i, (m, 2)"""
    g = kat()
    if i < n_pose():
        return g["pose_cp"][i]
    j = i - n_pose()
    return g["cp_xy"][g["cp_off"][j]:g["cp_off"][j + 1]]


def golden_curve(i):
    g = kat()
    a, b = int(g["pt_off"][i]), int(g["pt_off"][i + 1])
    return {key: g[key][a:b] for key in POINT_KEYS}


def oracle_curve(i):
    """bezier_oracle.curve of golden curve i, from its poses (or its control points)"""
    key = ("oracle", i)
    if key not in _cache:
        g = kat()
        n = int(g["n_points"][i])
        if i < n_pose():
            _cache[key] = bezier_oracle.curve4(*[float(v) for v in g["pose"][i]], n_points=n)
        else:
            _cache[key] = bezier_oracle.curve(control_points(i), n)
    return _cache[key]


def pose_groups():
    """{n_points: indices of the pose curves with that many points}"""
    g = kat()
    out = {}
    for i in range(n_pose()):
        out.setdefault(int(g["n_points"][i]), []).append(i)
    return out


def cp_groups():
    """{(m, n_points): indices of the control-point curves}"""
    g = kat()
    out = {}
    for i in range(n_pose(), len(g["n_points"])):
        out.setdefault((len(control_points(i)), int(g["n_points"][i])), []).append(i)
    return out


def obstacles(name):
    """(list of (x, y, size) rows, robot_radius, expected hit per golden curve) of the list "first", "last" or "none" """
    g = kat()
    return g["obs_" + name], float(g["rr"]), g["hit_" + name]


def random_poses(seed, n, lo=0.0, hi=20.0):
    """(starts (n, 3), goals (n, 3), offsets (n,)) seeded"""
    rs = np.random.RandomState(seed)

    def poses():
        return np.stack([rs.uniform(lo, hi, n), rs.uniform(lo, hi, n), rs.uniform(-np.pi, np.pi, n)], axis=1)
    return poses(), poses(), rs.uniform(1.0, 5.0, n)


def oracle_batch(starts, goals, offsets, n_points):
    """bezier_oracle.batch of pose pairs (pair mode); offsets a float or one per pair"""
    cs = []
    for i in range(len(starts)):
        o = float(offsets) if np.ndim(offsets) == 0 else float(offsets[i])
        cs.append(bezier_oracle.curve4(*[float(v) for v in starts[i]], *[float(v) for v in goals[i]], o, n_points=n_points))
    return bezier_oracle.batch(cs)


def oracle_hits(ob, obstacle_list, robot_radius):
    """first_hit per curve of an oracle batch"""
    off = ob["offsets"]
    obs = [tuple(float(v) for v in r) for r in obstacle_list]
    return np.array([bezier_oracle.first_hit(ob["x"][off[i]:off[i + 1]].tolist(), ob["y"][off[i]:off[i + 1]].tolist(), obs,
                                             robot_radius) for i in range(len(off) - 1)], dtype=np.int32)


def assert_result(res, ob, what, curvature=True, points=True):
    """A SteerResult against an oracle batch: everything the result holds, bit for bit"""
    assert np.all(res.status == 0) and res.rc == 0, what
    assert_same(res.length, ob["length"], what + " length")
    assert_same(res.control_points, ob["cp"], what + " control points")
    if curvature:
        assert_same(res.kmax, ob["kmax"], what + " kmax")
    else:
        assert res.kmax is None and res.k is None, what
    if points:
        assert np.array_equal(res.offsets, ob["offsets"]), what
        for key in ("x", "y", "yaw"):
            assert_same(getattr(res, key), ob[key], what + " " + key)
        if curvature:
            assert_same(res.k, ob["k"], what + " k")
    else:
        assert res.x is None and res.y is None and res.yaw is None and res.k is None and res.offsets is None, what

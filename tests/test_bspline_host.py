"""Batched B-spline courses (rrtx_bspline_*, BatchBSpline, rrt_amd.bspline_path, rrt_amd.spline_2d): everything that can be
checked without a device -- the oracle against the reference's recorded numbers, numpy's linspace and arange against the
oracle's sample lists, the scalar core of csrc/rpp_bspline.h compiled for the host (plainly and with sanitizers) and run as the
kernels run it, the ABI surface, the argument checks made before any HIP call, that there is no CPU fallback, and what the
drop-ins refuse."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bspline_oracle as O
import bspline_util as U
import util

CSRC = os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc")
NEW_FUNCS = ("rrtx_bspline_create", "rrtx_bspline_destroy", "rrtx_bspline_last_error", "rrtx_bspline_run",
             "rrtx_bspline_get_records", "rrtx_bspline_get_points", "rrtx_bspline_get_coefficients", "rrtx_bspline_get_hits",
             "rrtx_bspline_get_kernel_ms")


def test_golden_file_holds_the_cases():
    g = U.kat()
    n = len(g["script"])
    assert n == 65 and n % 64 != 0 and os.path.getsize(os.path.join(U.GOLD, "bspline_kat.npz")) < 1 << 20
    m = np.diff(g["wp_off"])
    bsp, s2d = U.select(0), U.select(1)
    for k in range(1, 6):      # every degree with one polynomial piece, one interior knot, two
        assert {k + 1, k + 2, k + 3} <= set(m[bsp][g["degree"][bsp] == k].tolist()), k
    for k in range(1, 4):
        assert {k + 1, k + 2, k + 3} <= set(m[s2d][g["degree"][s2d] == k].tolist()), k
    assert np.max(m) == 200 and {64, 65} <= set(m.tolist())
    assert {1, 2, 50, 257} <= set(g["count"][bsp].tolist()) and {0.05, 0.1, 0.5} <= set(g["ds"][s2d].tolist())
    assert np.max(np.abs(g["wp_x"])) > 9.0e3                                # coordinates near 1e4
    n_pt = np.diff(g["pt_off"])
    assert np.any((g["mode"] == U.ARANGE) & (n_pt == 1))                    # ds > s[-1]: a single point
    crs = U.courses(range(n))
    assert any(x.tolist() == [-1.0, 3.0, 4.0, 2.0, 1.0] for x, _ in crs)    # the two scripts' own driver inputs
    assert sum(x.tolist() == [-2.5, 0.0, 2.5, 5.0, 7.5, 3.0, -1.0] for x, _ in crs) == 3
    for i in np.nonzero(g["mode"] == U.EXPLICIT)[0]:                        # samples on both ends and on every interior knot
        us = set(g["ru"][g["pt_off"][i]:g["pt_off"][i + 1]].tolist())
        wu = g["wp_u"][g["wp_off"][i]:g["wp_off"][i + 1]]
        inner = O.knots(wu.tolist(), int(g["degree"][i]))[int(g["degree"][i]) + 1:len(wu)]
        assert {0.0, float(wu[-1])} <= us and set(inner) <= us and len(inner) > 0, i
    assert set(g["degree"][g["mode"] == U.EXPLICIT].tolist()) == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("script", (0, 1))
def test_oracle_has_the_references_parameters_knots_samples_and_counts(script):
    """Bit for bit: the waypoint parameter, the knot vector (FITPACK's for bspline_path, make_interp_spline's for spline_2d),
    the sample lists and the counts"""
    g, o, idx = U.kat(), U.oracle(script), U.select(script)
    assert np.all(o["status"] == O.OK) and np.array_equal(o["degree"], g["degree"][idx])
    assert np.array_equal(o["n_points"], np.diff(g["pt_off"])[idx])
    assert np.array_equal(U.bits(o["u"]), U.bits(U.gold(idx, "ru")))
    wp_u = np.concatenate([r["wp_u"] for r in o["per_course"]])
    assert np.array_equal(U.bits(wp_u), U.bits(U.gold(idx, "wp_u", "wp_off")))
    assert np.array_equal(U.bits(o["length"]), U.bits([g["wp_u"][g["wp_off"][i + 1] - 1] for i in idx]))
    seen = 0
    for j, i in enumerate(idx):
        ref = g["knots"][g["knot_off"][i]:g["knot_off"][i + 1]]
        if script == 1 and g["degree"][i] == 1:
            assert len(ref) == 0          # interp1d(kind="linear") holds no spline object
            continue
        assert np.array_equal(U.bits(ref), U.bits(o["per_course"][j]["knots"])), i
        seen += 1
    assert seen >= 15


def test_oracle_linear_kind_is_the_reference_bit_for_bit():
    g, o, idx = U.kat(), U.oracle(1), U.select(1)
    lin = [j for j, i in enumerate(idx) if g["degree"][i] == 1]
    assert len(lin) >= 5 and any(g["mode"][idx[j]] == U.EXPLICIT for j in lin)
    for j in lin:
        a, b = o["offsets"][j], o["offsets"][j + 1]
        pa, pb = g["pt_off"][idx[j]], g["pt_off"][idx[j] + 1]
        assert np.array_equal(U.bits(o["x"][a:b]), U.bits(g["rx"][pa:pb])), idx[j]
        assert np.array_equal(U.bits(o["y"][a:b]), U.bits(g["ry"][pa:pb])), idx[j]


@pytest.mark.parametrize("script", (0, 1))
def test_oracle_is_within_the_written_gaps_of_the_reference(script):
    """Coefficients, x, y, yaw and k per degree against the reference's scipy: within MARGIN x the figures written in
    bspline_util, which are the ones measured (a figure cannot be widened without this test noticing)"""
    seen = U.within(script, U.oracle(script), "oracle")
    table = U.GAP_BSP if script == 0 else U.GAP_S2D
    for q, per in sorted(seen.items()):
        print("script %d %-3s " % (script, q) + "  ".join("k=%d %.3e" % kv for kv in sorted(per.items())))
        for k, v in per.items():
            assert table[q][k] <= 1.01 * v + 1e-300, (q, k, v, table[q][k])


def test_sample_lists_are_numpys_linspace_and_arange():
    g = U.kat()
    idx = U.select(0)
    lin = [(float(g["wp_u"][g["wp_off"][i + 1] - 1]), int(g["count"][i])) for i in idx if g["mode"][i] == U.LINSPACE]
    ara = [(float(g["wp_u"][g["wp_off"][i + 1] - 1]), float(g["ds"][i])) for i in U.select(1) if g["mode"][i] == U.ARANGE]
    rs = np.random.RandomState(519)
    for _ in range(3000):
        lin.append((1.0 if rs.rand() < 0.5 else float(rs.uniform(1e-3, 300.0)), int(rs.choice([1, 2, 3, 50, 257, rs.randint(1, 2000)]))))
        ds = float(rs.choice([0.05, 0.1, 0.2, 0.25, 0.5, 1.0 / 3.0, rs.uniform(0.01, 2.0)]))
        ara.append((float(rs.uniform(0.01, 300.0)) if rs.rand() < 0.7 else ds * int(rs.randint(1, 400)), ds))
    lin += [(5e-324, 7), (1.0, 1), (0.3, 2)]     # a step that underflows takes numpy's other branch
    for stop, n in lin:
        want, got = np.linspace(0.0, stop, n), O.linspace(stop, n)
        assert len(got) == len(want) and np.array_equal(U.bits(got), U.bits(want)), (stop, n)
    for stop, ds in ara:
        want, got = np.arange(0, stop, ds), O.arange(stop, ds)
        assert len(got) == len(want) and np.array_equal(U.bits(got), U.bits(want)), (stop, ds)
        assert not got or got[-1] <= stop      # the last sample never passes the last knot


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    """tests/native/bspline_host_check.cpp as a program of its own, built plainly and with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("bspline_host_" + request.param)
    exe = str(d / "bspline_host_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"] + san + ["-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "bspline_host_check.cpp"), "-o", exe], check=True)

    def run(cases):
        """cases: (x, y, degree, param, mode, count, ds, us) -> list of dict(status, n, length, knots, cx, cy, x, y, yaw, k, u)"""
        rows = []
        for x, y, k, param, mode, count, ds, us in cases:
            us = [] if us is None else us
            rows += [[len(x), k, param, mode, count, ds, len(us)], x, y, us]
        np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1) for r in rows]).tofile(str(d / "in.bin"))
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = np.fromfile(str(d / "out.bin"), dtype=np.float64)
        res, pos = [], 0
        for x, *_ in cases:
            m, cnt, nk = len(x), int(out[pos + 1]), int(out[pos + 3])
            r = dict(status=int(out[pos]), n=cnt, length=out[pos + 2], knots=out[pos + 4:pos + 4 + nk])
            pos += 4 + nk
            r["cx"], r["cy"] = out[pos:pos + m], out[pos + m:pos + 2 * m]
            pos += 2 * m
            for q, key in enumerate(U.ARRAYS):
                r[key] = out[pos + q * cnt:pos + (q + 1) * cnt]
            pos += 5 * cnt
            res.append(r)
        assert pos == len(out)
        return res
    return run


def assert_core_equals_oracle(got, want, what):
    assert got["status"] == want["status"] and got["n"] == len(want["u"]), what
    assert U.bits(got["length"]) == U.bits(want["length"]), what
    assert np.array_equal(U.bits(got["knots"]), U.bits(want["knots"])), what
    if want["status"] == O.OK:
        assert np.array_equal(U.bits(got["cx"]), U.bits(want["cx"])) and np.array_equal(U.bits(got["cy"]), U.bits(want["cy"])), what
    else:
        assert not np.any(got["cx"]) and not np.any(got["cy"]), what
    for key in U.ARRAYS:
        assert np.array_equal(U.bits(got[key]), U.bits(want[key])), (what, key)


def test_scalar_core_equals_the_oracle_on_the_golden_courses(host_check):
    """csrc/rpp_bspline.h on the CPU, as the kernels use it: parameter, knots, band fit, count, every point by index"""
    g = U.kat()
    cases, want = [], []
    for script in (0, 1):
        idx, o = U.select(script), U.oracle(script)
        for j, (i, (x, y), us) in enumerate(zip(idx, U.courses(idx), U.samples(idx))):
            cases.append((x, y, int(g["degree"][i]), script, int(g["mode"][i]), max(int(g["count"][i]), 1), float(g["ds"][i]) or 1.0, us))
            want.append(o["per_course"][j])
    for i, (r, w) in enumerate(zip(host_check(cases), want)):
        assert_core_equals_oracle(r, w, i)


def test_scalar_core_corners_and_statuses(host_check):
    """One polynomial piece and one interior knot for every degree, both parameters, n_path_points 1 and 2, the last sample on
    the last knot, explicit samples on the interior knots; then coinciding waypoints, all waypoints equal and too few"""
    rs = np.random.RandomState(5)
    cases = []
    for k in range(1, 6):
        for m in (k + 1, k + 2, 9):
            x, y = np.cumsum(rs.uniform(0.3, 2.0, m)), np.cumsum(rs.uniform(-1.0, 1.0, m))
            for param in (O.NORMALISED, O.CHORD):
                end = O.parameter(x, y, param)[-1]
                inner = O.knots(O.parameter(x, y, param), k)[k + 1:m]
                cases += [(x, y, k, param, U.LINSPACE, 1, 1.0, None), (x, y, k, param, U.LINSPACE, 2, 1.0, None),
                          (x, y, k, param, U.LINSPACE, 33, 1.0, None), (x, y, k, param, U.ARANGE, 1, end / 8.0, None),
                          (x, y, k, param, U.EXPLICIT, 1, 1.0, [0.0, end] + list(inner) + [0.5 * end])]
    bad = [([0.0, 1.0, 1.0, 2.0, 3.0], [0.0, 1.0, 1.0, 0.0, 1.0], 3), ([2.0] * 4, [1.0] * 4, 2), ([0.0, 1.0, 2.0], [0.0, 1.0, 0.0], 3),
           ([0.0, 1.0], [0.0, 0.0], 2), ([0.0, 1.0, 2.0, 3.0, 4.0], [0.0, 1.0, 0.0, 1.0, 0.0], 5)]
    for x, y, k in bad:
        cases += [(x, y, k, O.NORMALISED, U.LINSPACE, 10, 1.0, None), (x, y, k, O.CHORD, U.ARANGE, 1, 0.1, None)]
    got = host_check(cases)
    for i, (r, (x, y, k, param, mode, count, ds, us)) in enumerate(zip(got, cases)):
        kw = dict(n_path_points=count) if mode == U.LINSPACE else dict(ds=ds) if mode == U.ARANGE else dict(u=us)
        assert_core_equals_oracle(r, O.course(x, y, k, param, **kw), i)
    assert [r["status"] for r in got[-10:]] == [O.DEGENERATE] * 4 + [O.TOO_FEW] * 6 and all(r["n"] == 0 for r in got[-10:])
    # the last sample of np.linspace is the last knot itself, and the spline passes through the last waypoint there
    r, (x, y, *_) = got[2], cases[2]
    assert r["u"][-1] == 1.0 and abs(r["x"][-1] - x[-1]) < 1e-12 and abs(r["y"][-1] - y[-1]) < 1e-12


def test_oracle_interpolates_and_degree_1_has_no_curvature():
    """The spline passes through its waypoints (at the waypoint parameters, handed over as samples) for every degree"""
    rs = np.random.RandomState(9)
    for k in range(1, 6):
        m = 12
        x, y = np.cumsum(rs.uniform(0.3, 2.0, m)), np.cumsum(rs.uniform(-1.0, 1.0, m))
        for param in (O.NORMALISED, O.CHORD):
            r = O.course(x, y, k, param, u=O.parameter(x, y, param))
            assert np.max(np.abs(np.array(r["x"]) - x)) < 1e-12 and np.max(np.abs(np.array(r["y"]) - y)) < 1e-12, (k, param)
            if k == 1:
                assert not np.any(r["k"])


def test_bspline_entry_points_declared_exported_and_bound():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    assert int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1)) == A.RRTX_ABI_VERSION == 6
    raw = C.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    L = A.load()
    assert L.rrtx_abi_version() == 6
    for fn in NEW_FUNCS:
        assert re.search(r"\b%s\(" % fn, hdr), fn
        assert hasattr(raw, fn), fn
        assert fn in A.EXPORTS and getattr(L, fn).argtypes is not None, fn
    vals = dict(re.findall(r"#define (RRTX_BSPLINE_[A-Z_]+) (\d+)", hdr))
    for name in ("OK", "DEGENERATE", "TOO_FEW", "PARAM_NORMALISED", "PARAM_CHORD", "SAMPLE_LINSPACE", "SAMPLE_ARANGE",
                 "SAMPLE_EXPLICIT", "MAX_DEGREE", "MAX_WAYPOINTS", "MAX_POINTS"):
        assert int(vals["RRTX_BSPLINE_" + name]) == getattr(A, "BSPLINE_" + name), name
    assert (A.BSPLINE_OK, A.BSPLINE_DEGENERATE, A.BSPLINE_TOO_FEW) == (O.OK, O.DEGENERATE, O.TOO_FEW) == (0, 1, 2)
    # the ctypes mirrors are laid out as the C compiler lays the structs out
    fields = re.search(r"typedef struct rrtx_bspline_batch \{(.*?)\} rrtx_bspline_batch;", hdr, re.S).group(1)
    names = re.findall(r"\b([A-Za-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in A.BSplineBatch._fields_]
    assert C.sizeof(A.BSplineBatch) == 128 and A.BSPLINE_RECORD.itemsize == 24
    rec = re.search(r"typedef struct rrtx_bspline_record \{(.*?)\} rrtx_bspline_record;", hdr, re.S).group(1)
    assert re.findall(r"\b([A-Za-z_]+)(?=;)", re.sub(r"/\*.*?\*/", "", rec, flags=re.S)) == list(A.BSPLINE_RECORD.names)
    assert rrt_amd.BatchBSpline is rrt_amd.bspline.BatchBSpline and rrt_amd.BSplineResult is rrt_amd.bspline.BSplineResult


@pytest.fixture()
def bspline_obj():
    """A raw rrtx_bspline*: handed out with or without a device, so that the argument checks can be reached."""
    import rrt_amd
    L = rrt_amd._abi.load()
    s = C.c_void_p()
    rc = L.rrtx_bspline_create(0, C.byref(s))
    assert rc in (0, -2) and s.value
    yield L, s, rc
    L.rrtx_bspline_destroy(s)


TWO = [([0.0, 1.0, 2.0, 3.5], [0.0, 1.0, 0.0, 0.5]), ([5.0, 6.0, 7.0, 9.0, 9.5], [1.0, 1.5, 1.0, 0.0, 2.0])]
INVALID = {
    "one_waypoint": dict(waypoints=[([0.0], [0.0]), TWO[1]]),
    "empty_course": dict(waypoints=(np.array([0, 4, 4]), np.arange(4.0), np.zeros(4))),
    "offsets_not_from_zero": dict(waypoints=(np.array([1, 3, 7]), np.arange(7.0), np.zeros(7))),
    "offsets_decrease": dict(waypoints=(np.array([0, 5, 3, 7]), np.arange(7.0), np.zeros(7))),
    "nan_coordinate": dict(waypoints=[([0.0, float("nan"), 2.0], [0.0, 1.0, 0.0]), TWO[1]]),
    "inf_coordinate": dict(waypoints=[TWO[0], ([5.0, 6.0, 7.0, 9.0], [1.0, float("inf"), 1.0, 0.0])]),
    "coordinate_above_1e6": dict(waypoints=[TWO[0], ([5.0, 6.0, 2.0e6, 9.0], [1.0, 1.5, 1.0, 0.0])]),
    "degree_0": dict(degree=0),
    "degree_6": dict(degree=6),
    "degree_per_course_6": dict(degree=[3, 6]),
    "n_path_points_0": dict(n_path_points=0),
    "n_path_points_negative_per_course": dict(n_path_points=[5, -1]),
    "ds_zero": dict(n_path_points=None, ds=0.0),
    "ds_negative": dict(n_path_points=None, ds=-0.1),
    "ds_nan": dict(n_path_points=None, ds=float("nan")),
    "ds_per_course_zero": dict(n_path_points=None, ds=[0.1, 0.0]),
    "sample_nan": dict(n_path_points=None, u=[[0.0, float("nan")], [0.5]]),
    "sample_inf_in_a_mixed_batch": dict(u=[None, [float("inf")]]),
    "param_unknown": dict(param=2),
    "too_many_waypoints": dict(waypoints=[(np.arange(4097.0), np.zeros(4097))]),
    "obstacle_nan": dict(obstacle_list=[(1.0, float("nan"), 0.5)]),
    "robot_radius_inf": dict(obstacle_list=[(1.0, 1.0, 0.5)], robot_radius=float("inf")),
    "too_many_points_linspace": dict(n_path_points=1 << 28),
    "too_many_points_arange": dict(waypoints=[([0.0, 9.0e5], [0.0, 0.0])] * 4, degree=1, param=1, n_path_points=None, ds=0.01),
}
VALID = {
    "defaults": dict(),
    "every_degree_per_course": dict(degree=[1, 4]),
    "n_path_points_per_course": dict(n_path_points=[1, 257]),
    "chord_arange": dict(param=1, n_path_points=None, ds=[0.1, 0.5]),
    "samples_as_data": dict(n_path_points=None, u=[[0.0, 0.25, 1.0], []]),
    "samples_for_one_course": dict(u=[None, [0.0, 1.0]]),
    "most_waypoints": dict(waypoints=[(np.arange(4096.0), np.zeros(4096))], degree=5),
    "with_obstacles_records_only": dict(obstacle_list=[(1.0, 1.0, 0.5)], robot_radius=0.2, arrays=False),
    "no_courses": dict(waypoints=[]),
    "coinciding_waypoints": dict(waypoints=[([0.0, 1.0, 1.0, 2.0], [0.0, 0.0, 0.0, 1.0])]),
    "too_few_waypoints": dict(waypoints=[([0.0, 1.0, 2.0], [0.0, 0.0, 1.0])], degree=3),
}


def run_raw(L, s, kw):
    import rrt_amd
    args = dict(waypoints=TWO, n_path_points=10)
    args.update(kw)
    b, keep = rrt_amd.bspline.pack_batch(**args)
    return L.rrtx_bspline_run(s, C.byref(b))


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_call(bspline_obj, case):
    L, s, _ = bspline_obj
    rc = run_raw(L, s, INVALID[case])
    assert rc == -1, (case, rc)   # RRTX_E_INVALID, with or without a device
    assert len(L.rrtx_bspline_last_error(s)) > 0, case


def test_null_pointers_are_refused(bspline_obj):
    import rrt_amd
    P = rrt_amd.bspline.pack_batch
    L, s, _ = bspline_obj
    b, keep = P(TWO, n_path_points=10)
    assert L.rrtx_bspline_run(None, C.byref(b)) == -1 and len(L.rrtx_bspline_last_error(None)) > 0
    assert L.rrtx_bspline_run(s, None) == -1
    for kw, fields in ((dict(n_path_points=10), ("offsets", "x", "y", "degree", "count")), (dict(ds=0.1), ("ds",)),
                       (dict(u=[[0.5], [0.5]]), ("u_offsets", "u")), (dict(n_path_points=10, u=[None, [0.5]]), ("count", "u_offsets", "u")),
                       (dict(n_path_points=10, obstacle_list=[(0.0, 0.0, 1.0)]), ("obstacles",))):
        for field in fields:
            b, keep = P(TWO, **kw)
            setattr(b, field, None)
            assert L.rrtx_bspline_run(s, C.byref(b)) == -1, (kw, field)
    assert L.rrtx_bspline_create(0, None) == -1 and L.rrtx_bspline_create(-1, C.byref(C.c_void_p())) == -1


@pytest.mark.parametrize("case", sorted(VALID))
def test_legal_arguments_pass_the_checks(bspline_obj, case):
    """Without a device a call that passes every check ends at the `usable` test (RRTX_E_NO_DEVICE); with one it runs."""
    L, s, created = bspline_obj
    rc = run_raw(L, s, VALID[case])
    if created == -2:
        assert rc == -2 and b"no CPU fallback" in L.rrtx_bspline_last_error(s), (case, rc)
    else:
        assert rc in (0, 1), (case, rc, L.rrtx_bspline_last_error(s))


def test_getters_need_a_run(bspline_obj):
    L, s, _ = bspline_obj
    buf = np.zeros(8)
    ms = C.c_double()
    assert L.rrtx_bspline_get_records(s, None, None, None, None, None) == -5   # RRTX_E_STATE
    assert L.rrtx_bspline_get_points(s, buf.ctypes.data, None, None, None, None, 8) == -5
    assert L.rrtx_bspline_get_coefficients(s, None, buf.ctypes.data, 8, buf.ctypes.data, buf.ctypes.data, 8) == -5
    assert L.rrtx_bspline_get_hits(s, buf.ctypes.data) == -5
    assert L.rrtx_bspline_get_kernel_ms(s, C.byref(ms)) == -5
    assert L.rrtx_bspline_get_records(None, None, None, None, None, None) == -1
    assert L.rrtx_bspline_get_kernel_ms(None, C.byref(ms)) == -1
    assert len(L.rrtx_bspline_last_error(s)) > 0


def test_getters_capacity_and_state_with_a_device(bspline_obj):
    """With a device: buffers that are too small, points after a run without arrays, hits after a run without obstacles"""
    import rrt_amd
    L, s, created = bspline_obj
    if created != 0:
        return   # without a device no run completes; the state errors above are all that can be reached
    b, keep = rrt_amd.bspline.pack_batch(TWO, n_path_points=10, arrays=False)
    assert L.rrtx_bspline_run(s, C.byref(b)) == 0
    buf = np.zeros(64)
    assert L.rrtx_bspline_get_points(s, buf.ctypes.data, None, None, None, None, 64) == -5
    assert L.rrtx_bspline_get_hits(s, buf.ctypes.data) == -5
    assert L.rrtx_bspline_get_coefficients(s, None, buf.ctypes.data, 3, None, None, 0) == -4    # RRTX_E_CAPACITY
    assert L.rrtx_bspline_get_coefficients(s, None, None, 0, buf.ctypes.data, buf.ctypes.data, 8) == -4
    b, keep = rrt_amd.bspline.pack_batch(TWO, n_path_points=10)
    assert L.rrtx_bspline_run(s, C.byref(b)) == 0
    assert L.rrtx_bspline_get_points(s, buf.ctypes.data, None, None, None, None, 19) == -4


def test_waypoint_and_sample_forms_pack_to_the_same_batch():
    import rrt_amd
    B = rrt_amd.bspline
    pairs = [TWO[0], (tuple(TWO[1][0]), tuple(TWO[1][1]))]
    arrays = [np.stack([np.array(x, dtype=float), np.array(y, dtype=float)], axis=1) for x, y in pairs]
    csr = (np.array([0, 4, 9]), np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]))
    want = B.pack_batch(pairs, n_path_points=7)[1]
    assert want["offsets"].tolist() == [0, 4, 9] and want["count"].tolist() == [7] and want["sample_of"] is None
    for form in (arrays, csr):
        got = B.pack_batch(form, n_path_points=7)[1]
        assert all(np.array_equal(got[k], want[k]) for k in ("offsets", "x", "y", "degree", "count"))
    b, keep = B.pack_batch(pairs, degree=[2, 5], n_path_points=[3, 9])
    assert (b.degree_per_course, b.sample_per_course, b.sample, b.param) == (1, 1, 0, 0) and keep["degree"].dtype == np.int32
    # samples as data: a list per course and the CSR pair are the same; None keeps the batch's mode for that course
    a = B.pack_batch(pairs, u=[[0.0, 0.5], [1.0]])
    c = B.pack_batch(pairs, u=(np.array([0, 2, 3]), np.array([0.0, 0.5, 1.0])))
    assert a[0].sample == c[0].sample == 2 and np.array_equal(a[1]["u"], c[1]["u"]) and np.array_equal(a[1]["u_offsets"], c[1]["u_offsets"])
    mixed = B.pack_batch(pairs, ds=0.1, param=1, u=[None, [0.0, 2.0]])
    assert mixed[1]["sample_of"].tolist() == [1, 2] and mixed[1]["u_offsets"].tolist() == [0, 0, 2] and mixed[0].sample == 1
    for kw in (dict(), dict(n_path_points=5, ds=0.1), dict(n_path_points=[1, 2, 3]), dict(degree=[1, 2, 3], n_path_points=5),
               dict(u=[[0.5]]), dict(u=[None, [0.5]]), dict(degree=2.5, n_path_points=5)):
        with pytest.raises(ValueError):
            B.pack_batch(pairs, **kw)
    with pytest.raises(ValueError):
        B.pack_batch([([0.0, 1.0], [0.0])], n_path_points=5)


def test_bspline_result_host_side():
    """course(i), is_free(i), free, what a course without points raises, the explicit samples' range check, and the hand-over
    to the tracker -- a BSplineResult built from the oracle"""
    import rrt_amd
    A, B = rrt_amd._abi, rrt_amd.bspline
    o = U.oracle(0)
    n = len(o["status"])
    rec = np.zeros(n, dtype=A.BSPLINE_RECORD)
    rec["n_points"], rec["length"], rec["degree"] = o["n_points"], o["length"], o["degree"]
    hit = np.full(n, -1, dtype=np.int32)
    hit[1] = 4
    res = B.BSplineResult(rec, o["offsets"], tuple(o[k] for k in U.ARRAYS), o["knots"], o["knot_offsets"], (o["cx"], o["cy"]),
                          o["wp_offsets"], hit)
    for i in (0, 5, n - 1):
        c = res.course(i)
        assert len(c) == 4 and [len(q) for q in c] == [int(o["n_points"][i])] * 4
        assert c[0].tolist() == o["per_course"][i]["x"] and c[3].tolist() == o["per_course"][i]["k"]
    assert res.is_free(0) is True and res.is_free(1) is False and int(np.sum(res.free)) == n - 1 and len(res) == n
    res.status[2], res.status[3], res.hit[2] = A.BSPLINE_DEGENERATE, A.BSPLINE_TOO_FEW, -2
    for i in (2, 3):
        with pytest.raises(A.RrtxError):
            res.course(i)
        with pytest.raises(A.RrtxError):
            res.is_free(i)
    assert not res.free[2]
    bare = B.BSplineResult(rec, o["offsets"], None, o["knots"], o["knot_offsets"], (o["cx"], o["cy"]), o["wp_offsets"])
    with pytest.raises(A.RrtxError):
        bare.course(0)
    with pytest.raises(A.RrtxError):
        bare.free
    off, x, y, yaw = rrt_amd.track._csr(res)
    assert off is not None and np.array_equal(x, o["x"]) and np.array_equal(yaw, o["yaw"])
    # samples outside [0, length] of a course that has a spline: ValueError, as interp1d raises
    st, length = np.array([0, 1, 0], dtype=np.int32), np.array([1.0, 0.0, 2.5])
    B._check_range(np.array([0, 2, 3, 5]), np.array([0.0, 1.0, 9.0, 0.0, 2.5]), st, length)
    for us in ([0.0, 1.0000000000000002, 9.0, 0.0, 2.5], [0.0, 1.0, 9.0, -1e-300, 2.5]):
        with pytest.raises(ValueError):
            B._check_range(np.array([0, 2, 3, 5]), np.array(us), st, length)


def test_dropin_modules_have_the_reference_names():
    import rrt_amd.bspline_path as bp
    import rrt_amd.spline_2d as s2
    assert bp.__all__ == ["approximate_b_spline_path", "interpolate_b_spline_path", "plot_curvature"]
    assert str(inspect.signature(bp.interpolate_b_spline_path)) == "(x, y, n_path_points, degree=3)"
    assert str(inspect.signature(bp.approximate_b_spline_path)) == "(x, y, n_path_points, degree=3, s=None)"
    assert callable(bp._calc_distance_vector) and callable(bp._evaluate_spline)
    assert s2.__all__ == ["Spline2D"] and str(inspect.signature(s2.Spline2D.__init__)) == "(self, x, y, kind='cubic')"
    x, y = [-1.0, 3.0, 4.0, 2.0, 1.0], [0.0, -3.0, 1.0, 1.0, 3.0]
    assert np.array_equal(U.bits(bp._calc_distance_vector(x, y)), U.bits(O.parameter(x, y, O.NORMALISED)))
    sp = s2.Spline2D(x, y, kind="quadratic")
    assert isinstance(sp.s, list) and np.array_equal(U.bits(sp.s), U.bits(O.parameter(x, y, O.CHORD))) and len(sp.ds) == 4


def test_dropin_refuses_the_smoothing_fit_and_plots():
    import rrt_amd.bspline_path as bp
    x, y = [-1.0, 3.0, 4.0, 2.0, 1.0], [0.0, -3.0, 1.0, 1.0, 3.0]
    for kw in (dict(), dict(s=None), dict(s=0.5), dict(s=5)):
        with pytest.raises(NotImplementedError, match="smoothing"):
            bp.approximate_b_spline_path(x, y, 50, **kw)
    with pytest.raises(ValueError):
        bp.plot_curvature(x, y, [0.0] * 5, [0.0] * 5)


def test_spline2d_raises_value_error_out_of_range():
    """Before any device call: calc_position outside [0, s[-1]], too few waypoints for the kind, coinciding waypoints"""
    import rrt_amd.spline_2d as s2
    x, y = [-2.5, 0.0, 2.5, 5.0, 7.5, 3.0, -1.0], [0.7, -6, -5, -3.5, 0.0, 5.0, -2.0]
    sp = s2.Spline2D(x, y, kind="cubic")
    for s in (-1e-9, float(sp.s[-1]) * (1 + 1e-15), [0.0, 1.0, 1e9], np.array([[0.5, -3.0]])):
        with pytest.raises(ValueError, match="interpolation range"):
            sp.calc_position(s)
    with pytest.raises(ValueError):
        s2.Spline2D([0.0, 1.0, 2.0], [0.0, 1.0, 0.0], kind="cubic")
    with pytest.raises(ValueError):
        s2.Spline2D([0.0, 1.0, 1.0, 2.0], [0.0, 1.0, 1.0, 0.0], kind="linear")
    with pytest.raises(NotImplementedError):
        s2.Spline2D(x, y, kind="nearest")


def test_package_imports_no_scipy():
    code = ("import sys; sys.path.insert(0, %r); import rrt_amd, rrt_amd.bspline_path, rrt_amd.spline_2d; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('matplotlib', 'scipy')]; assert not bad, bad" % util.ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_no_cpu_fallback():
    import rrt_amd
    import rrt_amd.bspline_path as bp
    import rrt_amd.spline_2d as s2
    if rrt_amd._abi.load().rrtx_device_count() > 0:
        return   # with a device the GPU suite covers the calls
    with pytest.raises(rrt_amd._abi.RrtxError):
        rrt_amd.BatchBSpline()
    with pytest.raises(rrt_amd._abi.RrtxError):
        bp.interpolate_b_spline_path([0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 0.0, 1.0], 10)
    with pytest.raises(rrt_amd._abi.RrtxError):
        s2.Spline2D([0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 0.0, 1.0]).calc_position(0.5)

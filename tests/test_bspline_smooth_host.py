"""The smoothing fit of approximate_b_spline_path (rrtx_bspline_approximate, BatchBSpline.approximate,
rrt_amd.bspline_path_smoothing): everything that can be checked without a device -- the golden file's cases, the oracle
against the reference's recorded numbers (knot vectors equal, the rest within the written gaps), the oracle's invariants, the
scalar core of csrc/rpp_bspline_smooth.h compiled for the host (plainly and with sanitizers) and run as the kernels run it, the
ABI surface, the argument checks made before any HIP call, and the new drop-in's names."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bspline_oracle as B
import bspline_smooth_oracle as S
import bspline_smooth_util as U
import util

CSRC = os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc")
NEW_FUNCS = ("rrtx_bspline_approximate", "rrtx_bspline_get_axis_records", "rrtx_bspline_get_axis_splines")
KINDS = ("driver", "s_none", "deg1", "deg2", "deg3", "deg4", "deg5", "m=k+1", "m=k+2", "m=k+3", "axes_differ", "second_stage",
         "nplus>=4", "interp_knots_smoothed", "polynomial", "scale0.3", "scale2", "scale10", "near1e4", "m200")


def test_golden_file_holds_the_cases():
    g = U.kat()
    n = len(g["degree"])
    assert n >= 65 and os.path.getsize(os.path.join(U.GOLD, "bspline_smooth_kat.npz")) < 1 << 20
    seen = set(",".join(g["kinds"].tolist()).split(","))
    assert set(KINDS) <= seen, set(KINDS) - seen
    assert not np.any(g["warned_x"]) and not np.any(g["warned_y"])
    m = np.diff(g["wp_off"])
    assert np.max(m) == 200 and np.max(np.abs(g["wp_x"])) > 9.0e3
    crs, deg, s, cnt = U.golden_batch()
    drv = [i for i in range(n) if crs[i][0].tolist() == [-1.0, 3.0, 4.0, 2.0, 1.0] and s[i] == 0.5 and deg[i] == 3 and cnt[i] == 50]
    assert len(drv) == 1 and "driver" in g["kinds"][drv[0]]
    for k in range(1, 6):
        assert {k + 1, k + 2, k + 3} <= set(m[g["degree"] == k].tolist()), k
    # the labels are facts about the recorded splines: check the ones that can be read off the file
    nk = np.stack([np.diff(g["knot_off_x"]), np.diff(g["knot_off_y"])])
    for i in range(n):
        kinds, k = g["kinds"][i].split(","), int(g["degree"][i])
        assert ("axes_differ" in kinds) == (nk[0, i] != nk[1, i]), i
        assert ("second_stage" in kinds) == bool(np.max(nk[:, i]) > max(m[i] // 2, 2 * k + 2)), i
        if "polynomial" in kinds:
            assert np.min(nk[:, i]) == 2 * k + 2 and m[i] > k + 1, i
        if "interp_knots_smoothed" in kinds:
            assert np.max(nk[:, i]) == m[i] + k + 1, i
    # and the ones that only the course of the fit shows, from the oracle (whose knots equal the file's, see below)
    o = U.oracle_full()
    for i in range(n):
        kinds, k = g["kinds"][i].split(","), int(g["degree"][i])
        u = B.parameter(crs[i][0], crs[i][1], B.NORMALISED)
        sv = float(m[i]) if s[i] is None else s[i]
        traces = [[], []]
        fits = [S.fit(u, list(crs[i][a]), k, sv, traces[a]) for a in (0, 1)]
        assert ("nplus>=4" in kinds) == any(tr and max(tr) >= 4 for tr in traces), i
        smoothed = [f["n"] == m[i] + k + 1 and f["ier"] == 0 and f["iters"] > 0 for f in fits]
        assert ("interp_knots_smoothed" in kinds) == any(smoothed), i
        assert [f["n"] for f in fits] == [a["n"] for a in o["per_course"][i]["axes"]]


def test_oracle_has_the_references_knots_and_is_within_the_written_gaps():
    """The knot vectors equal scipy's bit for bit (U.gaps asserts it for every axis); coefficients, x, y, yaw and k per degree
    are within MARGIN x the figures written in bspline_smooth_util, which are the ones measured (a figure cannot be widened
    without this test noticing)"""
    o = U.oracle_full()
    n_gold = U.full_batch()[4]
    assert np.all(o["status"][:n_gold] == S.OK)
    assert np.array_equal(o["n_points"][:n_gold], np.diff(U.kat()["pt_off"]))
    seen = U.within(o, n_gold, "oracle")
    for q, per in sorted(seen.items()):
        print("%-3s " % q + "  ".join("k=%d %.3e" % kv for kv in sorted(per.items())))
        for k, v in per.items():
            assert U.GAP[q][k] <= 1.01 * v + 1e-300, (q, k, v, U.GAP[q][k])


def test_oracle_invariants():
    """|fp - s| < 0.001 s where a smoothing or least-squares spline was accepted; fp <= s on the polynomial; the interior
    knots are data sites (but for the interpolation knots of an even degree, which are midpoints); statuses and s == 0"""
    o = U.oracle_full()
    crs, deg, s, cnt, n_gold = U.full_batch()
    kinds = {-2: 0, -1: 0, 0: 0}
    for i, r in enumerate(o["per_course"]):
        m, k = len(crs[i][0]), deg[i]
        sv = float(m) if s[i] is None else s[i]
        if r["status"] != S.OK:
            assert r["axes"][0]["n"] == r["axes"][1]["n"] == 0 and r["x"] == [] and o["length"][i] == 0.0
            continue
        assert len(r["x"]) == cnt[i] and o["length"][i] == 1.0
        u = B.parameter(crs[i][0], crs[i][1], B.NORMALISED)
        for ax in r["axes"]:
            n = ax["n"]
            assert 2 * k + 2 <= n <= m + k + 1 and len(ax["c"]) == n - k - 1 and ax["ier"] in (0, -1, -2, 2, 3)
            assert ax["ier"] <= 0 or i >= n_gold        # the root search stops early on a few corners only
            kinds[ax["ier"]] = kinds.get(ax["ier"], 0) + 1
            if sv == 0.0:
                assert (ax["ier"], n, ax["fp"], ax["rounds"], ax["iters"]) == (-1, m + k + 1, 0.0, 0, 0)
                continue
            if ax["ier"] == 0:
                assert abs(ax["fp"] - sv) < 0.001 * sv, (i, ax["fp"], sv)
            if ax["ier"] == -2:
                assert n == 2 * k + 2 and ax["fp"] <= sv and ax["iters"] == 0 and math.isinf(ax["p"]), (i, ax["fp"], sv)
            if ax["iters"] > 0:
                assert 0.0 < ax["p"] < math.inf
            inner = ax["t"][k + 1:n - k - 1]
            assert ax["t"][:k + 1] == [0.0] * (k + 1) and ax["t"][n - k - 1:] == [1.0] * (k + 1)
            assert all(b > a for a, b in zip(inner, inner[1:]))
            if n < m + k + 1 or k % 2:
                assert set(inner) <= set(u[1:-1]), i
    assert min(kinds[q] for q in (0, -1, -2)) >= 7 and kinds[2] >= 1 and kinds[3] >= 2, kinds
    assert sorted(set(o["status"].tolist())) == [S.OK, S.DEGENERATE, S.TOO_FEW]
    assert o["axis0"]["iters"].max() >= 10 and o["axis0"]["rounds"].max() >= 15


def test_s_zero_is_the_interpolating_oracle():
    crs, deg, s, cnt, _ = U.full_batch()
    o = U.oracle_full()
    zero = [i for i in range(len(crs)) if s[i] == 0.0]
    assert len(zero) >= 6
    for i in zero:
        want = B.course(crs[i][0], crs[i][1], deg[i], B.NORMALISED, n_path_points=cnt[i])
        got = o["per_course"][i]
        assert got["axes"][0]["t"] == want["knots"] == got["axes"][1]["t"]
        assert got["axes"][0]["c"] == want["cx"] and got["axes"][1]["c"] == want["cy"]
        for key in U.ARRAYS:
            assert np.array_equal(U.bits(got[key]), U.bits(want[key])), (i, key)


def test_oracle_paths_are_all_taken():
    """Every path of the knot loop and of the root search that a fit can take is taken by some axis of the batch that the
    host program and the device are compared on -- so a header that differs from the oracle on one of them cannot pass.
    The "initial choice of p is too small" branch with a finite upper bracket replaces p when p >= p3 (Dierckx's text; a
    restatement that tests p <= p3 ends on ier = 2 where FITPACK converges): the course of that finding
    reaches the branch, is pulled back inside the bracket there and converges."""
    o = U.oracle_full()
    crs, deg, s, cnt, n_gold = U.full_batch()
    events = set()
    for r in o["per_course"]:
        for ax in r["axes"]:
            events |= ax["events"]
    assert {"p_too_large", "p_too_small_unbracketed", "p_too_small_bracketed", "p_too_small_pulled_back", "second_stage",
            "accepted_within_acc_in_knot_loop"} <= events, events
    iers = set(int(v) for a in (0, 1) for v in o["axis%d" % a]["ier"])
    assert {0, -1, -2, 2, 3} <= iers
    bx, by = U.branch_course()
    i = [j for j in range(n_gold, len(crs)) if len(crs[j][0]) == 16 and np.array_equal(crs[j][0], bx)][0]
    assert deg[i] == 4 and s[i] == 0.5 and np.array_equal(crs[i][1], by)
    axes = o["per_course"][i]["axes"]
    assert any("p_too_small_pulled_back" in ax["events"] for ax in axes)
    assert all(ax["ier"] == 0 and abs(ax["fp"] - 0.5) < 0.0005 for ax in axes) and max(ax["iters"] for ax in axes) >= 4
    # the corner built for it is accepted inside the knot loop, as a least-squares spline with one interior knot
    acc = [ax for r in o["per_course"][n_gold:] for ax in r["axes"] if "accepted_within_acc_in_knot_loop" in ax["events"] and ax["ier"] == 0]
    assert any(ax["n"] == 2 * 3 + 3 and ax["rounds"] == 2 and math.isinf(ax["p"]) for ax in acc)
    # an interval without residual takes no knot (FITPACK's fpknot is undefined there): add_knot returns n unchanged
    t, fpint, nrdata = [0.0] * 12, [0.0, 0.0, 1.0], [3, 2, 0]
    assert S.add_knot([0.1 * j for j in range(9)], t, 10, 3, fpint, nrdata, 3) == 10 and nrdata == [3, 2, 0]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    """tests/native/bspline_smooth_host_check.cpp as a program of its own, built plainly and with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("bspline_smooth_host_" + request.param)
    exe = str(d / "bspline_smooth_host_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"] + san + ["-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "bspline_smooth_host_check.cpp"), "-o", exe], check=True)

    def run(crs, deg, s, cnt):
        rows = []
        for (x, y), k, sv, n in zip(crs, deg, s, cnt):
            rows += [[len(x), k, float(len(x)) if sv is None else sv, n, -1], x, y]
        np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1) for r in rows]).tofile(str(d / "in.bin"))
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = np.fromfile(str(d / "out.bin"), dtype=np.float64)
        res, pos = [], 0
        for k in deg:
            r = dict(status=int(out[pos]), n=int(out[pos + 1]), length=out[pos + 2], axes=[])
            pos += 3
            for a in (0, 1):
                nk = int(out[pos])
                ax = dict(n=nk, ier=int(out[pos + 1]), fp=out[pos + 2], p=out[pos + 3], rounds=int(out[pos + 4]), iters=int(out[pos + 5]))
                pos += 6
                nc = nk - k - 1 if nk else 0
                ax["t"], ax["c"] = out[pos:pos + nk], out[pos + nk:pos + nk + nc]
                pos += nk + nc
                r["axes"].append(ax)
            for q, key in enumerate(U.ARRAYS):
                r[key] = out[pos + q * r["n"]:pos + (q + 1) * r["n"]]
            pos += 5 * r["n"]
            res.append(r)
        assert pos == len(out)
        return res
    return run


def test_scalar_core_equals_the_oracle(host_check):
    """csrc/rpp_bspline_smooth.h on the CPU, as the kernels use it, over the golden courses and the corners: statuses, axis
    records, knots, coefficients and every point, bit for bit"""
    crs, deg, s, cnt, _ = U.full_batch()
    o = U.oracle_full()
    got = host_check(crs, deg, s, cnt)
    for i, (r, w) in enumerate(zip(got, o["per_course"])):
        assert r["status"] == w["status"] and r["n"] == len(w["u"]) and U.bits(r["length"]) == U.bits(o["length"][i]), i
        for a in (0, 1):
            ga, wa = r["axes"][a], w["axes"][a]
            assert (ga["n"], ga["ier"], ga["rounds"], ga["iters"]) == (wa["n"], wa["ier"], wa["rounds"], wa["iters"]), (i, a, ga, wa["ier"])
            assert U.bits(ga["fp"]) == U.bits(wa["fp"]) and U.bits(ga["p"]) == U.bits(wa["p"]), (i, a)
            assert np.array_equal(U.bits(ga["t"]), U.bits(wa["t"])), (i, a)
            assert np.array_equal(U.bits(ga["c"]), U.bits(wa["c"])), (i, a)
        for key in U.ARRAYS:
            assert np.array_equal(U.bits(r[key]), U.bits(w[key])), (i, key)


def test_entry_points_declared_exported_and_bound():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    assert int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1)) == A.RRTX_ABI_VERSION == 6
    raw = C.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    L = A.load()
    for fn in NEW_FUNCS:
        assert re.search(r"\b%s\(" % fn, hdr), fn
        assert hasattr(raw, fn), fn
        assert fn in A.EXPORTS and getattr(L, fn).argtypes is not None, fn
    assert int(re.search(r"#define RRTX_BSPLINE_SINGULAR (\d+)", hdr).group(1)) == A.BSPLINE_SINGULAR == S.SINGULAR == 3
    # the ctypes mirrors are laid out as the C compiler lays the structs out; the run batch and its record keep their sizes
    fields = re.search(r"typedef struct rrtx_bspline_smooth_batch \{(.*?)\} rrtx_bspline_smooth_batch;", hdr, re.S).group(1)
    names = re.findall(r"\b([A-Za-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in A.BSplineSmoothBatch._fields_] == ["run", "s", "s_per_course", "reserved"]
    assert C.sizeof(A.BSplineBatch) == 128 and A.BSPLINE_RECORD.itemsize == 24
    assert C.sizeof(A.BSplineSmoothBatch) == 144 and A.BSplineSmoothBatch.s.offset == 128
    rec = re.search(r"typedef struct rrtx_bspline_axis_record \{(.*?)\} rrtx_bspline_axis_record;", hdr, re.S).group(1)
    assert re.findall(r"\b([A-Za-z_]+)(?=;)", re.sub(r"/\*.*?\*/", "", rec, flags=re.S)) == list(A.BSPLINE_AXIS_RECORD.names)
    assert A.BSPLINE_AXIS_RECORD.itemsize == 32
    src = "#include <stdio.h>\n#include \"rrtx.h\"\nint main(void) { printf(\"%zu %zu %zu %zu\", sizeof(rrtx_bspline_batch), " \
          "sizeof(rrtx_bspline_record), sizeof(rrtx_bspline_smooth_batch), sizeof(rrtx_bspline_axis_record)); return 0; }\n"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "sz.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(d, "sz.c"), "-o", os.path.join(d, "sz")], check=True)
        assert subprocess.run([os.path.join(d, "sz")], capture_output=True, text=True).stdout.split() == ["128", "24", "144", "32"]
    assert rrt_amd.BSplineSmoothResult is rrt_amd.bspline.BSplineSmoothResult and issubclass(rrt_amd.BSplineSmoothResult, rrt_amd.BSplineResult)
    sig = str(inspect.signature(rrt_amd.BatchBSpline.approximate))
    assert sig == "(self, waypoints, n_path_points=None, degree=3, s=None, u=None, obstacle_list=None, robot_radius=0.0, arrays=True)"


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
    "s_negative": dict(s=-0.5),
    "s_nan": dict(s=float("nan")),
    "s_inf": dict(s=float("inf")),
    "s_per_course_negative": dict(s=[0.5, -1e-300]),
    "s_per_course_nan": dict(s=[float("nan"), 0.5]),
    "one_waypoint": dict(waypoints=[([0.0], [0.0]), TWO[1]]),
    "offsets_decrease": dict(waypoints=(np.array([0, 5, 3, 7]), np.arange(7.0), np.zeros(7))),
    "nan_coordinate": dict(waypoints=[([0.0, float("nan"), 2.0], [0.0, 1.0, 0.0]), TWO[1]]),
    "coordinate_above_1e6": dict(waypoints=[TWO[0], ([5.0, 6.0, 2.0e6, 9.0], [1.0, 1.5, 1.0, 0.0])]),
    "degree_6": dict(degree=6),
    "n_path_points_0": dict(n_path_points=0),
    "sample_nan": dict(n_path_points=None, u=[[0.0, float("nan")], [0.5]]),
    "too_many_waypoints": dict(waypoints=[(np.arange(4097.0), np.zeros(4097))]),
    "obstacle_nan": dict(obstacle_list=[(1.0, float("nan"), 0.5)]),
    "too_many_points": dict(n_path_points=1 << 28),
}
VALID = {
    "defaults_s_none": dict(),
    "s_scalar": dict(s=0.5),
    "s_zero": dict(s=0.0),
    "s_per_course_with_none": dict(s=[None, 0.0]),
    "every_degree_per_course": dict(degree=[1, 4], s=[0.01, 2.0]),
    "samples_as_data": dict(n_path_points=None, u=[[0.0, 0.25, 1.0], []]),
    "with_obstacles_records_only": dict(obstacle_list=[(1.0, 1.0, 0.5)], robot_radius=0.2, arrays=False),
    "no_courses": dict(waypoints=[]),
    "coinciding_waypoints": dict(waypoints=[([0.0, 1.0, 1.0, 2.0], [0.0, 0.0, 0.0, 1.0])]),
    "too_few_waypoints": dict(waypoints=[([0.0, 1.0, 2.0], [0.0, 0.0, 1.0])], degree=3),
}


def run_raw(L, s, kw):
    import rrt_amd
    args = dict(waypoints=TWO, n_path_points=10)
    args.update(kw)
    sb, keep = rrt_amd.bspline.pack_smooth_batch(**args)
    return L.rrtx_bspline_approximate(s, C.byref(sb))


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_call(bspline_obj, case):
    L, s, _ = bspline_obj
    rc = run_raw(L, s, INVALID[case])
    assert rc == -1, (case, rc)   # RRTX_E_INVALID, with or without a device
    assert L.rrtx_bspline_last_error(s).startswith(b"rrtx_bspline_approximate: "), case


def test_null_pointers_and_the_parameter_are_refused(bspline_obj):
    import rrt_amd
    P = rrt_amd.bspline.pack_smooth_batch
    L, s, _ = bspline_obj
    sb, keep = P(TWO, 0.5, n_path_points=10)
    assert L.rrtx_bspline_approximate(None, C.byref(sb)) == -1 and len(L.rrtx_bspline_last_error(None)) > 0
    assert L.rrtx_bspline_approximate(s, None) == -1
    sb.s = None
    assert L.rrtx_bspline_approximate(s, C.byref(sb)) == -1 and b"s is NULL" in L.rrtx_bspline_last_error(s)
    for field in ("offsets", "x", "y", "degree", "count"):
        sb, keep = P(TWO, 0.5, n_path_points=10)
        setattr(sb.run, field, None)
        assert L.rrtx_bspline_approximate(s, C.byref(sb)) == -1, field
    sb, keep = P(TWO, 0.5, n_path_points=10)
    sb.run.param = rrt_amd._abi.BSPLINE_PARAM_CHORD     # the chord-length parameter is spline_2d's: NORMALISED only
    assert L.rrtx_bspline_approximate(s, C.byref(sb)) == -1 and b"NORMALISED" in L.rrtx_bspline_last_error(s)
    with pytest.raises(ValueError):
        P(TWO, [0.5, 0.5, 0.5], n_path_points=10)


@pytest.mark.parametrize("case", sorted(VALID))
def test_legal_arguments_pass_the_checks(bspline_obj, case):
    """Without a device a call that passes every check ends at the `usable` test (RRTX_E_NO_DEVICE); with one it runs."""
    L, s, created = bspline_obj
    rc = run_raw(L, s, VALID[case])
    if created == -2:
        assert rc == -2 and b"no CPU fallback" in L.rrtx_bspline_last_error(s), (case, rc)
    else:
        assert rc in (0, 1), (case, rc, L.rrtx_bspline_last_error(s))


def test_getters_and_their_state_order(bspline_obj):
    """Before any run every getter returns RRTX_E_STATE; with a device: the axis getters answer only after an approximate
    run, get_coefficients only after a plain run, and too small buffers are RRTX_E_CAPACITY"""
    import rrt_amd
    L, s, created = bspline_obj
    buf, ibuf = np.zeros(64), np.zeros(8, dtype=np.int64)
    nk, nc = C.c_int64(), C.c_int64()
    arec = np.zeros(4, dtype=rrt_amd._abi.BSPLINE_AXIS_RECORD)
    assert L.rrtx_bspline_get_axis_records(s, arec.ctypes.data, 4) == -5    # RRTX_E_STATE
    assert L.rrtx_bspline_get_axis_splines(s, 0, None, None, 0, None, None, 0, C.byref(nk), C.byref(nc)) == -5
    assert L.rrtx_bspline_get_axis_records(None, arec.ctypes.data, 4) == -1
    assert L.rrtx_bspline_get_axis_splines(None, 0, None, None, 0, None, None, 0, None, None) == -1
    if created != 0:
        return   # without a device no run completes
    b, keep = rrt_amd.bspline.pack_batch(TWO, n_path_points=10)
    assert L.rrtx_bspline_run(s, C.byref(b)) == 0
    assert L.rrtx_bspline_get_axis_records(s, arec.ctypes.data, 4) == -5
    assert L.rrtx_bspline_get_axis_splines(s, 0, None, None, 0, None, None, 0, C.byref(nk), C.byref(nc)) == -5
    assert L.rrtx_bspline_get_coefficients(s, ibuf.ctypes.data, buf.ctypes.data, 64, None, None, 0) == 0
    sb, keep = rrt_amd.bspline.pack_smooth_batch(TWO, 0.5, n_path_points=10)
    assert L.rrtx_bspline_approximate(s, C.byref(sb)) == 0
    assert L.rrtx_bspline_get_coefficients(s, ibuf.ctypes.data, buf.ctypes.data, 64, None, None, 0) == -5
    assert L.rrtx_bspline_get_records(s, None, None, None, None, None) == 0
    assert L.rrtx_bspline_get_axis_records(s, arec.ctypes.data, 3) == -4    # RRTX_E_CAPACITY
    assert L.rrtx_bspline_get_axis_records(s, arec.ctypes.data, 4) == 0 and np.all(arec["n_knots"] >= 8)
    assert L.rrtx_bspline_get_axis_splines(s, 2, None, None, 0, None, None, 0, None, None) == -1
    assert L.rrtx_bspline_get_axis_splines(s, 1, None, None, 0, None, None, 0, C.byref(nk), C.byref(nc)) == 0
    assert nk.value == int(arec["n_knots"][2:].sum()) and nc.value == nk.value - 8
    assert L.rrtx_bspline_get_axis_splines(s, 1, None, buf.ctypes.data, nk.value - 1, None, None, 0, None, None) == -4
    assert L.rrtx_bspline_get_axis_splines(s, 1, None, None, 0, None, buf.ctypes.data, nc.value - 1, None, None) == -4
    assert L.rrtx_bspline_run(s, C.byref(b)) == 0
    assert L.rrtx_bspline_get_axis_records(s, arec.ctypes.data, 4) == -5


def test_smooth_result_host_side():
    """A BSplineSmoothResult built from the oracle: course(i), what a course without points raises, the hand-over to the
    tracker"""
    import rrt_amd
    A, Bm = rrt_amd._abi, rrt_amd.bspline
    o = U.oracle_full()
    n = len(o["status"])
    rec = np.zeros(n, dtype=A.BSPLINE_RECORD)
    for key in ("status", "n_points", "length", "degree"):
        rec[key] = o[key]
    arec = np.zeros((2, n), dtype=A.BSPLINE_AXIS_RECORD)
    axes = []
    for a in (0, 1):
        ax = o["axis%d" % a]
        for key in ("ier", "fp", "p", "rounds", "iters"):
            arec[a][key] = ax[key]
        axes.append((ax["knot_offsets"], ax["knots"], ax["coef_offsets"], ax["coefficients"]))
    res = Bm.BSplineSmoothResult(rec, o["offsets"], tuple(o[k] for k in U.ARRAYS), axes, arec, None)
    assert len(res) == n and len(res.knots) == 2 and res.coef_offsets[1][-1] == len(res.coefficients[1])
    assert np.array_equal(res.ier[0], o["axis0"]["ier"]) and np.array_equal(res.p[1], o["axis1"]["p"])
    c = res.course(0)
    assert len(c) == 4 and c[0].tolist() == o["per_course"][0]["x"] and c[3].tolist() == o["per_course"][0]["k"]
    bad = [i for i in range(n) if o["status"][i] != S.OK]
    assert len(bad) == 4
    for i in bad:
        with pytest.raises(A.RrtxError):
            res.course(i)
    res.status[0] = A.BSPLINE_SINGULAR
    with pytest.raises(A.RrtxError, match="not finite"):
        res.course(0)
    off, x, y, yaw = rrt_amd.track._csr(res)
    assert off is not None and np.array_equal(x, o["x"]) and np.array_equal(yaw, o["yaw"])


def test_dropin_has_the_reference_names_and_imports_no_scipy():
    import rrt_amd.bspline_path as bp
    import rrt_amd.bspline_path_smoothing as bs
    assert bs.__all__ == ["approximate_b_spline_path", "interpolate_b_spline_path", "plot_curvature"]
    assert str(inspect.signature(bs.approximate_b_spline_path)) == "(x, y, n_path_points, degree=3, s=None)"
    assert str(inspect.signature(bs.interpolate_b_spline_path)) == "(x, y, n_path_points, degree=3)"
    assert str(inspect.signature(bs.plot_curvature)) == "(x_list, y_list, heading_list, curvature, k=0.01, c='-c', label='Curvature')"
    assert bs.interpolate_b_spline_path is bp.interpolate_b_spline_path and bs.plot_curvature is bp.plot_curvature
    assert "bspline_path_smoothing" in bp.__doc__ and "rrt_amd.bspline_path " in bs.__doc__
    code = ("import sys; sys.path.insert(0, %r); import rrt_amd, rrt_amd.bspline_path_smoothing; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('matplotlib', 'scipy')]; assert not bad, bad" % util.ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("bspline_smooth_oracle.py", "bspline_smooth_util.py", "test_gpu_bspline_smooth.py"):
        assert not re.search(r"^\s*(import|from) scipy", open(os.path.join(util.ROOT, "tests", name)).read(), re.M), name


def test_no_cpu_fallback():
    import rrt_amd
    import rrt_amd.bspline_path_smoothing as bs
    if rrt_amd._abi.load().rrtx_device_count() > 0:
        return   # with a device the GPU suite covers the calls
    with pytest.raises(rrt_amd._abi.RrtxError):
        bs.approximate_b_spline_path([-1.0, 3.0, 4.0, 2.0, 1.0], [0.0, -3.0, 1.0, 1.0, 3.0], 50, s=0.5)

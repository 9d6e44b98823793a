"""Batched closed-loop tracking of courses given as data (rrtx_tracker_*, BatchTrack): everything that can be checked
without a device -- the ABI surface, the argument checks made before any HIP call, track_course with its start-state
argument against the reference's numbers of tests/golden/track_batch_kat.npz, and the Python input normalisation."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import util
import track_util as tu

CSRC = os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc")
# RRTX_TEST_SANITIZE=1: the same run under AddressSanitizer + UndefinedBehaviorSanitizer (as tests/test_track_host.py)
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if os.environ.get("RRTX_TEST_SANITIZE") else []
TRACKER_FUNCS = ("rrtx_tracker_create", "rrtx_tracker_destroy", "rrtx_tracker_last_error", "rrtx_tracker_run",
                 "rrtx_tracker_get_counts", "rrtx_tracker_get_records", "rrtx_tracker_get_arrays",
                 "rrtx_tracker_get_kernel_ms")
E_INVALID, E_NO_DEVICE = -1, -2


def test_tracker_entry_points_declared_exported_bound_and_mirrored():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    assert int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1)) == A.RRTX_ABI_VERSION == 6
    raw = C.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    L = A.load()
    assert L.rrtx_abi_version() == 6
    for fn in TRACKER_FUNCS:
        assert re.search(r"\b%s\(" % fn, hdr), fn
        assert hasattr(raw, fn), fn
        assert fn in A.EXPORTS and getattr(L, fn).argtypes is not None, fn
    fields = re.search(r"typedef struct rrtx_track_batch \{(.*?)\} rrtx_track_batch;", hdr, re.S).group(1)
    names = re.findall(r"\b([A-Za-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f for f, _ in A.TrackBatch._fields_]
    # 2 x int64, 9 pointers, 2 x int32 -- no padding on LP64
    assert C.sizeof(A.TrackBatch) == 2 * 8 + 9 * C.sizeof(C.c_void_p) + 2 * 4 == 96


@pytest.fixture()
def tracker_obj():
    """A raw rrtx_tracker*: handed out with or without a device, so that the argument checks can be reached."""
    import rrt_amd
    L = rrt_amd._abi.load()
    t = C.c_void_p()
    rc = L.rrtx_tracker_create(0, C.byref(t))
    assert rc in (0, E_NO_DEVICE) and t.value
    if rc == E_NO_DEVICE:
        assert L.rrtx_tracker_last_error(t)
    yield L, t
    L.rrtx_tracker_destroy(t)


def base_batch():
    """Two valid courses of 3 and 4 points, one shared obstacle."""
    return dict(n=2, offsets=np.array([0, 3, 7], dtype=np.int64), x=np.linspace(0.0, 1.2, 7), y=np.zeros(7), yaw=np.zeros(7),
                per_course=None, start_state=None, obstacles=np.array([[5.0, 5.0, 1.0]]), obs_offsets=None, n_obstacles=1,
                robot_radius=np.zeros(1), robot_radius_per_course=0, want_arrays=1)


def with_field(name, row, col, value, shape):
    a = np.zeros(shape)
    a[row, col] = value
    return {name: a}


NAN, INF = float("nan"), float("inf")
INVALID = {
    "null_tracker": dict(obj=None),
    "null_params": dict(params=None),
    "null_batch": dict(batch=None),
    "null_offsets": dict(offsets=None),
    "null_x": dict(x=None),
    "null_y": dict(y=None),
    "null_yaw": dict(yaw=None),
    "null_obstacles": dict(obstacles=None),
    "null_robot_radius": dict(robot_radius=None),
    "negative_n": dict(n=-1),
    "n_above_2_30": dict(n=(1 << 30) + 1),
    "offsets_do_not_start_at_0": dict(offsets=np.array([1, 3, 7], dtype=np.int64)),
    "offsets_decrease": dict(offsets=np.array([0, 4, 3], dtype=np.int64)),
    "more_than_2_31_points": dict(offsets=np.array([0, 3, 1 << 31], dtype=np.int64)),
    "pose_x_nan": dict(x=np.array([0.0, 0.2, NAN, 0.6, 0.8, 1.0, 1.2])),
    "pose_y_inf": dict(y=np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, INF])),
    "pose_yaw_nan": dict(yaw=np.array([NAN, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])),
    "obstacle_nan": dict(obstacles=np.array([[5.0, NAN, 1.0]])),
    "obstacle_radius_inf": dict(obstacles=np.array([[5.0, 5.0, INF]])),
    "robot_radius_nan": dict(robot_radius=np.array([NAN])),
    "robot_radius_per_course_inf": dict(robot_radius=np.array([0.0, INF]), robot_radius_per_course=1),
    "start_state_nan": with_field("start_state", 1, 3, NAN, (2, 4)),
    "per_course_inf": with_field("per_course", 1, 0, INF, (2, 3)),
    "65_obstacles_in_the_shared_list": dict(obstacles=np.ones((65, 3)), n_obstacles=65),
    "65_obstacles_in_one_course_list": dict(obstacles=np.ones((66, 3)), n_obstacles=66,
                                            obs_offsets=np.array([0, 1, 66], dtype=np.int64)),
    "obs_offsets_do_not_start_at_0": dict(obs_offsets=np.array([1, 1, 1], dtype=np.int64)),
    "obs_offsets_decrease": dict(obstacles=np.ones((2, 3)), n_obstacles=2, obs_offsets=np.array([0, 2, 1], dtype=np.int64)),
    "obs_offsets_beyond_the_rows": dict(obs_offsets=np.array([0, 1, 2], dtype=np.int64)),
    "negative_n_obstacles": dict(n_obstacles=-1),
    "dt_zero": dict(tp=dict(dt=0.0)),
    "T_negative": dict(tp=dict(T=-1.0)),
    "T_over_dt_above_1e6": dict(tp=dict(T=100.0, dt=1e-5)),
    "Lf_zero": dict(tp=dict(Lf=0.0)),
    "L_zero": dict(tp=dict(L=0.0)),
    "steer_max_above_0_79": dict(tp=dict(steer_max=0.8)),
    "steer_max_negative": dict(tp=dict(steer_max=-0.1)),
    "target_speed_nan": dict(tp=dict(target_speed=NAN)),
}


def call_run(L, t, over):
    import rrt_amd
    A = rrt_amd._abi
    kw = base_batch()
    tp = dict(A.TRACK_DEFAULTS)
    over = dict(over)
    tp.update(over.pop("tp", {}))
    obj = over.pop("obj", t)
    no_params = "params" in over and over.pop("params") is None
    no_batch = "batch" in over and over.pop("batch") is None
    kw.update(over)
    ptr = {k: (None if v is None else v.ctypes.data) for k, v in kw.items() if isinstance(v, np.ndarray) or v is None}
    scal = {k: v for k, v in kw.items() if k not in ptr}
    b = A.TrackBatch(**scal, **ptr)
    rc = L.rrtx_tracker_run(obj, None if no_params else C.byref(A.TrackParams(**tp)), None if no_batch else C.byref(b))
    return rc, obj, kw     # kw keeps the arrays alive until the call has returned


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_call(tracker_obj, case):
    L, t = tracker_obj
    rc, obj, _ = call_run(L, t, INVALID[case])
    assert rc == E_INVALID, (case, rc)
    assert len(L.rrtx_tracker_last_error(obj)) > 0, case


def test_valid_batch_without_a_device_is_no_device_and_getters_refuse(tracker_obj):
    import rrt_amd
    L, t = tracker_obj
    n, m = C.c_int64(), C.c_int64()
    assert L.rrtx_tracker_get_counts(t, C.byref(n), C.byref(m)) == -5      # RRTX_E_STATE before the first run
    if L.rrtx_device_count() > 0:
        pytest.skip("a GPU is present")
    rc, _, _ = call_run(L, t, {})
    assert rc == E_NO_DEVICE
    assert b"no usable gfx950 device" in L.rrtx_tracker_last_error(t)
    rc, _, _ = call_run(L, t, dict(n=0, offsets=np.zeros(1, dtype=np.int64)))   # the empty run is checked the same way
    assert rc == E_NO_DEVICE
    with pytest.raises(rrt_amd._abi.RrtxError):      # no CPU fallback
        rrt_amd.BatchTrack()


# ---- host core ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("track_batch") / "track_batch_host_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-Wall", "-Werror=array-bounds"] + SAN +
                   ["-I", CSRC, os.path.join(util.ROOT, "tests", "native", "track_batch_host_check.cpp"), "-o", out], check=True)
    return out


def kat_vectors(g):
    """Per vector of a track_kat-style file: (params, obstacles, robot_radius, cx, cy, cyaw in driving order, start state)."""
    model = json.loads(str(g["model"]))
    po, oo, out = 0, 0, []
    for i, (rr, ts, yth, ratio) in enumerate(g["rows"]):
        n, m = int(g["npath"][i]), int(g["nobs"][i])
        cx, cy, cw = (g[k][po:po + n][::-1].copy() for k in ("path_x", "path_y", "path_yaw"))   # stored goal -> start
        po += n
        obs = [tuple(r) for r in g["obs"][oo:oo + m]]
        oo += m
        params = dict(model, target_speed=float(ts), yaw_th=float(yth), xy_th=0.5, invalid_travel_ratio=float(ratio))
        start = g["start_state"][i] if "start_state" in getattr(g, "files", g) else np.array([-0.0, -0.0, 0.0, 0.0])
        out.append((params, obs, float(rr), cx, cy, cw, start))
    return out


def test_golden_holds_the_wanted_cases():
    g = np.load(os.path.join(tu.GOLD, "track_batch_kat.npz"))
    assert os.path.getsize(os.path.join(tu.GOLD, "track_batch_kat.npz")) < 256 * 1024
    npath, out, nobs = g["npath"], g["out"], g["nobs"]
    for n in (3, 448, 449, 700, 960):
        assert np.sum(npath == n) >= 2, n
    slab = npath >= 449
    assert np.any(slab & ((out[:, 2] & 1) == 0)) and np.any(slab & (out[:, 1] == 2002))
    default = np.array([-0.0, -0.0, 0.0, 0.0]).view(np.uint64)
    preset = np.any(np.ascontiguousarray(g["start_state"]).view(np.uint64) != default, axis=1)
    assert preset.sum() >= 24 and set(g["start_state"][preset][:, 3].tolist()) == {0.0, 1.0, -0.5}
    i64 = int(np.nonzero(nobs == 64)[0][0])
    assert nobs[i64 + 1] == 63 and npath[i64] == npath[i64 + 1]
    assert out[i64, 2] & 8 and not out[i64 + 1, 2] & 8


def test_host_core_with_start_state_reproduces_the_batch_vectors(exe, tmp_path):
    g = np.load(os.path.join(tu.GOLD, "track_batch_kat.npz"))
    jobs = []
    for params, obs, rr, cx, cy, cw, start in kat_vectors(g):
        thr = [[o[0], o[1], (o[2] + rr) ** 2] for o in obs]
        jobs.append(np.concatenate([[params[q] for q in tu.PORDER], start, [len(thr)],
                                    np.array(thr, dtype=np.float64).reshape(-1), [len(cx)], cx, cy, cw]).astype(np.float64))
    np.concatenate(jobs).tofile(str(tmp_path / "jobs.bin"))
    subprocess.run([exe, str(tmp_path / "jobs.bin"), str(tmp_path / "out.bin")], check=True)
    out = np.fromfile(str(tmp_path / "out.bin"), dtype=np.float64)
    pos = 0
    for i in range(len(jobs)):
        find, n, fail, ood, tl = out[pos:pos + 5]
        n = int(n)
        arr = out[pos + 5:pos + 5 + 7 * n].reshape(7, n)
        pos += 5 + 7 * n
        assert ood == 0
        assert [int(find), n, int(fail)] == g["out"][i].tolist(), "vector %d" % i
        assert np.array_equal(tu.bits(np.concatenate([[tl], arr[[0, 1, 2, 3, 5, 6], -1]])), tu.bits(g["last"][i])), "vector %d" % i
        sums = [float(sum(arr[r].tolist())) for r in (0, 1, 2, 3, 5, 6)]     # sequential sums over every element
        assert np.array_equal(tu.bits(sums), tu.bits(g["sums"][i])), "vector %d sums" % i
    assert pos == len(out) and len(jobs) >= 36


# ---- Python input normalisation ----------------------------------------------------------------------------------------
class SteerStub:
    """The fields of SteerResult that BatchTrack reads."""

    def __init__(self, offsets, x, y, yaw):
        self.offsets, self.x, self.y, self.yaw = offsets, x, y, yaw


def batch_contents(b, keep):
    import rrt_amd
    out = {f: getattr(b, f) for f, t in rrt_amd._abi.TrackBatch._fields_ if t is not C.c_void_p}
    for f, t in rrt_amd._abi.TrackBatch._fields_:
        if t is C.c_void_p:
            assert (getattr(b, f) is None) == (keep[f] is None), f
            if keep[f] is not None:
                assert getattr(b, f) == keep[f].ctypes.data and keep[f].flags["C_CONTIGUOUS"], f
            out[f] = None if keep[f] is None else (keep[f].dtype.str, keep[f].tobytes())
    return out


def test_three_course_forms_give_identical_batches():
    import rrt_amd
    pack_batch = rrt_amd.track.pack_batch
    trip = [([0.0, 0.2, 0.4], [0.0, 0.1, 0.2], [0.5, 0.5, 0.5]), ([], [], []), ([1.0, 2.0, 3.0, 4.0], [0.0] * 4, [-0.0] * 4)]
    off = np.array([0, 3, 3, 7])
    x, y, yaw = (np.concatenate([np.asarray(t[k], dtype=np.float64) for t in trip]) for k in range(3))
    kw = dict(obstacle_list=[(5, 5, 1), (3, 6, 2)], robot_radius=[0.0, 0.1, 0.2], yaw_th=[0.05, 0.06, 0.07],
              start_state=(1.0, -1.0, 0.3, 0.5))
    got = [batch_contents(*[r[i] for i in (0, 2)]) for r in (pack_batch(trip, **kw), pack_batch((off, x, y, yaw), **kw),
                                                               pack_batch((off.astype(np.int32), x.tolist(), y, yaw), **kw),
                                                               pack_batch(SteerStub(off, x, y, yaw), **kw))]
    assert got[0] == got[1] == got[2] == got[3]
    c = got[0]
    assert c["n"] == 3 and c["n_obstacles"] == 2 and c["robot_radius_per_course"] == 1 and c["want_arrays"] == 1
    assert c["offsets"] == ("<i8", off.astype(np.int64).tobytes()) and c["obs_offsets"] is None
    with pytest.raises(ValueError):
        pack_batch(SteerStub(None, None, None, None))        # a lengths-only SteerResult holds no courses


def test_scalar_and_per_course_keywords_broadcast():
    import rrt_amd
    pack_batch = rrt_amd.track.pack_batch
    trip = [([0.0, 0.2, 0.4], [0.0] * 3, [0.0] * 3)] * 3
    b, scalars, keep = pack_batch(trip, robot_radius=0.25, target_speed=2.0, yaw_th=0.1, invalid_travel_ratio=3.0, arrays=False)
    assert keep["per_course"] is None and b.per_course is None and b.robot_radius_per_course == 0 and b.want_arrays == 0
    assert scalars == dict(target_speed=2.0, yaw_th=0.1, invalid_travel_ratio=3.0) and keep["robot_radius"].tolist() == [0.25]
    assert keep["start_state"] is None and b.start_state is None
    b, scalars, keep = pack_batch(trip, target_speed=[1.0, 2.0, 3.0], yaw_th=0.1, invalid_travel_ratio=3.0,
                                  start_state=[-0.0, -0.0, 0.0, 0.0])
    assert keep["per_course"].tolist() == [[1.0, 0.1, 3.0], [2.0, 0.1, 3.0], [3.0, 0.1, 3.0]]
    assert keep["start_state"].shape == (3, 4) and np.all(np.signbit(keep["start_state"][:, :2]))
    b, _, keep = pack_batch(trip, course_obstacles=[[(1, 2, 3)], [], [(4, 5, 6), (7, 8, 9)]])
    assert keep["obs_offsets"].dtype == np.int64 and keep["obs_offsets"].tolist() == [0, 1, 1, 3] and b.n_obstacles == 3
    assert keep["goals"].tolist() == [[0.4, 0.0, 0.0]] * 3
    for bad in (dict(robot_radius=[0.1, 0.2]), dict(yaw_th=[0.1] * 4), dict(start_state=np.zeros((2, 4))),
                dict(course_obstacles=[[]] * 2)):
        with pytest.raises(ValueError):
            pack_batch(trip, **bad)


def test_obstacle_list_with_course_obstacles_raises():
    import rrt_amd
    pack_batch = rrt_amd.track.pack_batch
    trip = [([0.0, 0.2, 0.4], [0.0] * 3, [0.0] * 3)]
    with pytest.raises(ValueError):
        pack_batch(trip, obstacle_list=[(5, 5, 1)], course_obstacles=[[(5, 5, 1)]])


def test_best_takes_the_later_of_equal_times_and_appends_its_goal():
    import rrt_amd
    TrackResult = rrt_amd.track.TrackResult
    rec = np.zeros(5, dtype=rrt_amd._abi.TRACK_RECORD)
    rec["find_goal"] = [1, 1, 0, 1, 1]
    rec["len"] = [2, 2, 2, 2, 2]
    rec["t_last"] = [0.1, 0.05, 0.01, 0.05, 0.2]
    off = np.arange(0, 11, 2)
    arrays = [np.arange(10.0) + 100 * k for k in range(7)]
    arrays[4] = np.array([0.0, 0.1, 0.0, 0.05, 0.0, 0.01, 0.0, 0.05, 0.0, 0.2])      # t: t[-1] = t_last
    goals = np.arange(15.0).reshape(5, 3) + 0.5
    res = TrackResult(rec, off, arrays, goals)
    flag, x, y, yaw, v, t, a, d = res.best()
    assert flag is True and x == [6.0, 7.0, 9.5] and y == [106.0, 107.0, 10.5] and yaw == [206.0, 207.0, 11.5]   # course 3, not 1
    assert v == [306.0, 307.0] and t == [0.0, 0.05] and a == [506.0, 507.0] and d == [606.0, 607.0]
    assert res.best([3, 1])[1] == [2.0, 3.0, 3.5]          # in the order given: now course 1 is the later one
    assert res.best([0, 4])[1] == [0.0, 1.0, 0.5]
    assert res.best([2]) == (False, None, None, None, None, None, None, None)
    assert res.best([]) == (False, None, None, None, None, None, None, None)
    assert res.feasible(2)[0] is False and res.feasible(2)[5] == [0.0, 0.01]
    rec["ood"] = [0, 2, 3, 1, 0]
    res = TrackResult(rec, off, arrays, goals, course_len=np.array([5, 2, 961, 5, 5]))
    with pytest.raises(IndexError):
        res.feasible(1)
    for i in (2, 3):
        with pytest.raises(rrt_amd._abi.RrtxError):
            res.feasible(i)
    with pytest.raises(IndexError):
        res.best()

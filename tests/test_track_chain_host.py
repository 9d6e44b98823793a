"""Tracking courses a producer left on the device (rrtx_tracker_run_from, BatchTrack.run(device_result)): everything that
can be checked without a device -- the ABI surface, the argument checks made before any HIP call, the per-course decision
and the per-group pick of csrc/rpp_track.h compiled for the CPU, and the Python keyword handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import util
import track_util as tu

CSRC = os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc")
NATIVE = os.path.join(util.ROOT, "tests", "native")
# RRTX_TEST_SANITIZE=1: the same run under AddressSanitizer + UndefinedBehaviorSanitizer (as tests/test_track_batch_host.py)
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if os.environ.get("RRTX_TEST_SANITIZE") else []
NEW_FUNCS = ("rrtx_tracker_run_from", "rrtx_tracker_get_winners", "rrtx_tracker_get_goals", "rrtx_steer_get_generation",
             "rrtx_spline_get_generation", "rrtx_bspline_get_generation")
E_INVALID, E_NO_DEVICE, E_STATE = -1, -2, -5
NAN, INF = float("nan"), float("inf")


def test_new_entry_points_declared_exported_bound_and_mirrored():
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
    fields = re.search(r"typedef struct rrtx_track_source \{(.*?)\} rrtx_track_source;", hdr, re.S).group(1)
    names = re.findall(r"\b([A-Za-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f for f, _ in A.TrackSource._fields_]
    # 2 x int32, pointer, uint64, pointer, int64, int32 and 4 bytes of tail padding on LP64
    assert C.sizeof(A.TrackSource) == 2 * 4 + 8 + 8 + 8 + 8 + 4 + 4 == 48
    for name, value in (("SRC_STEER", 1), ("SRC_SPLINE", 2), ("SRC_BSPLINE", 3), ("SELECT_ALL", 0), ("SELECT_FREE", 1),
                        ("SELECT_MASK", 2)):
        assert int(re.search(r"#define RRTX_%s (\d+)" % name, hdr).group(1)) == getattr(A, name) == value
    assert (A.OOD_NOT_FINITE, A.OOD_SKIPPED) == (rrt_amd.track.OOD_NOT_FINITE, rrt_amd.track.OOD_SKIPPED) == (4, 5)


@pytest.fixture()
def objs():
    """A raw rrtx_tracker* and a raw rrtx_steer* as the source: both are handed out with or without a device."""
    import rrt_amd
    L = rrt_amd._abi.load()
    t, s = C.c_void_p(), C.c_void_p()
    assert L.rrtx_tracker_create(0, C.byref(t)) in (0, E_NO_DEVICE) and t.value
    assert L.rrtx_steer_create(0, C.byref(s)) in (0, E_NO_DEVICE) and s.value
    yield L, t, s
    L.rrtx_steer_destroy(s)
    L.rrtx_tracker_destroy(t)


def base_batch():
    """Four courses (their points are the source's), one shared obstacle."""
    return dict(n=4, offsets=None, x=None, y=None, yaw=None, per_course=None, start_state=None,
                obstacles=np.array([[5.0, 5.0, 1.0]]), obs_offsets=None, n_obstacles=1, robot_radius=np.zeros(1),
                robot_radius_per_course=0, want_arrays=1)


def with_field(name, row, col, value, shape):
    a = np.zeros(shape)
    a[row, col] = value
    return {name: a}


ONES = np.ones(4, dtype=np.uint8)
INVALID = {
    "null_tracker": dict(obj=None),
    "null_params": dict(params=None),
    "null_source": dict(source=None),
    "null_batch": dict(batch=None),
    "null_object": dict(src=dict(object=None)),
    "unknown_kind_0": dict(src=dict(kind=0)),
    "unknown_kind_4": dict(src=dict(kind=4)),
    "unknown_select": dict(src=dict(select=3)),
    "unknown_arrays_of": dict(src=dict(group=2, arrays_of=2)),
    "course_offsets_given": dict(offsets=np.zeros(5, dtype=np.int64)),
    "course_x_given": dict(x=np.zeros(1)),
    "course_y_given": dict(y=np.zeros(1)),
    "course_yaw_given": dict(yaw=np.zeros(1)),
    "group_negative": dict(src=dict(group=-1)),
    "n_not_a_multiple_of_group": dict(src=dict(group=3)),
    "arrays_of_winners_without_a_group": dict(src=dict(arrays_of=1)),
    "mask_missing": dict(src=dict(select=2)),
    "mask_without_select_mask": dict(src=dict(select=0, mask=ONES)),
    "mask_with_select_free": dict(src=dict(select=1, mask=ONES)),
    "null_obstacles": dict(obstacles=None),
    "null_robot_radius": dict(robot_radius=None),
    "negative_n": dict(n=-1),
    "n_above_2_30": dict(n=(1 << 30) + 1),
    "obstacle_nan": dict(obstacles=np.array([[5.0, NAN, 1.0]])),
    "robot_radius_per_course_inf": dict(robot_radius=np.array([0.0, 0.0, 0.0, INF]), robot_radius_per_course=1),
    "start_state_nan": with_field("start_state", 1, 3, NAN, (4, 4)),
    "per_course_inf": with_field("per_course", 1, 0, INF, (4, 3)),
    "65_obstacles_in_the_shared_list": dict(obstacles=np.ones((65, 3)), n_obstacles=65),
    "65_obstacles_in_one_course_list": dict(obstacles=np.ones((66, 3)), n_obstacles=66,
                                            obs_offsets=np.array([0, 1, 66, 66, 66], dtype=np.int64)),
    "obs_offsets_do_not_start_at_0": dict(obs_offsets=np.array([1, 1, 1, 1, 1], dtype=np.int64)),
    "obs_offsets_decrease": dict(obstacles=np.ones((2, 3)), n_obstacles=2, obs_offsets=np.array([0, 2, 1, 2, 2], dtype=np.int64)),
    "obs_offsets_beyond_the_rows": dict(obs_offsets=np.array([0, 1, 2, 2, 2], dtype=np.int64)),
    "negative_n_obstacles": dict(n_obstacles=-1),
    "dt_zero": dict(tp=dict(dt=0.0)),
    "T_over_dt_above_1e6": dict(tp=dict(T=100.0, dt=1e-5)),
    "steer_max_above_0_79": dict(tp=dict(steer_max=0.8)),
    "target_speed_nan": dict(tp=dict(target_speed=NAN)),
}


def call_run_from(L, t, s, over):
    import rrt_amd
    A = rrt_amd._abi
    kw = base_batch()
    tp = dict(A.TRACK_DEFAULTS)
    over = dict(over)
    tp.update(over.pop("tp", {}))
    obj = over.pop("obj", t)
    sf = dict(kind=A.SRC_STEER, select=A.SELECT_ALL, object=s, generation=0, mask=None, group=0, arrays_of=0)
    sf.update(over.pop("src", {}))
    mask = sf["mask"]
    if mask is not None:
        sf["mask"] = mask.ctypes.data
    no = {k: (k in over and over.pop(k) is None) for k in ("params", "source", "batch")}
    kw.update(over)
    ptr = {k: (None if v is None else v.ctypes.data) for k, v in kw.items() if isinstance(v, np.ndarray) or v is None}
    scal = {k: v for k, v in kw.items() if k not in ptr}
    b = A.TrackBatch(**scal, **ptr)
    rc = L.rrtx_tracker_run_from(obj, None if no["params"] else C.byref(A.TrackParams(**tp)),
                                 None if no["source"] else C.byref(A.TrackSource(**sf)), None if no["batch"] else C.byref(b))
    return rc, obj, (kw, mask)     # the arrays stay alive until the call has returned


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_call(objs, case):
    L, t, s = objs
    rc, obj, _ = call_run_from(L, t, s, INVALID[case])
    assert rc == E_INVALID, (case, rc)
    assert len(L.rrtx_tracker_last_error(obj)) > 0, case


def test_valid_call_is_no_device_without_one_and_state_for_a_source_that_never_solved(objs):
    L, t, s = objs
    gen = C.c_uint64(7)
    assert L.rrtx_steer_get_generation(s, C.byref(gen)) == 0 and gen.value == 0      # no completed solve yet
    assert L.rrtx_steer_get_generation(s, None) == E_INVALID and L.rrtx_steer_get_generation(None, C.byref(gen)) == E_INVALID
    g = C.c_int64()
    assert L.rrtx_tracker_get_winners(t, None, C.byref(g)) == E_STATE                # before the first run
    assert L.rrtx_tracker_get_goals(t, np.zeros(3).ctypes.data) == E_STATE
    for over in ({}, dict(src=dict(group=2, arrays_of=1)), dict(src=dict(select=2, mask=ONES)), dict(src=dict(select=1))):
        rc, _, _ = call_run_from(L, t, s, over)
        if L.rrtx_device_count() > 0:        # with a device the checks go on to the source's state
            assert rc == E_STATE and b"no completed run" in L.rrtx_tracker_last_error(t)
        else:
            assert rc == E_NO_DEVICE and b"no usable gfx950 device" in L.rrtx_tracker_last_error(t)


# ---- host core ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("track_chain") / "track_chain_host_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-Wall", "-Werror=array-bounds"] + SAN +
                   ["-I", CSRC, "-I", os.path.join(NATIVE, "fake_hip"), os.path.join(NATIVE, "track_chain_host_check.cpp"),
                    "-o", out], check=True)
    return out


def run_exe(exe, mode, doubles, tmp_path):
    np.asarray(doubles, dtype=np.float64).tofile(str(tmp_path / "jobs.bin"))
    subprocess.run([exe, mode, str(tmp_path / "jobs.bin"), str(tmp_path / "out.bin")], check=True)
    return np.fromfile(str(tmp_path / "out.bin"), dtype=np.float64)


def test_per_course_decision(exe, tmp_path):
    """Lengths 0, 2, 3, 960, 961; a NaN or +-inf in each of x, y, yaw at the first, a middle and the last index; and a
    deselected course that holds a NaN: 5, not 4 (the program also decides deselected courses behind NULL pointers)."""
    jobs, want = [], []

    def add(selected, n, expect, poison=None):
        xyz = [np.linspace(0.0, 1.0, n), np.zeros(n), np.full(n, 0.25)]
        if poison:
            xyz[poison[0]][poison[1]] = poison[2]
        jobs.append(np.concatenate([[selected, 960, n]] + xyz))
        want.append(expect)
    for n, expect in ((0, 2), (2, 2), (3, 0), (960, 0), (961, 3)):
        add(1, n, expect)
    for n in (3, 449, 960):
        for comp in range(3):
            for idx in (0, n // 2, n - 1):
                for v in (NAN, INF, -INF):
                    add(1, n, 4, (comp, idx, v))
    add(0, 10, 5, (0, 4, NAN))
    add(0, 2, 5)
    add(0, 961, 5)
    add(1, 2, 2, (1, 1, NAN))         # too short before anything is read
    add(1, 961, 3, (2, 0, INF))
    got = run_exe(exe, "ood", np.concatenate(jobs), tmp_path)
    assert got.tolist() == [float(w) for w in want] and len(want) == 5 + 81 + 5


# A pose pair BatchSteer("dubins").plan accepts whose curve is not finite: start and goal at one place, and a subnormal
# curvature (the entry point asks for 0 < c <= 1e300 only), by which dubins_interp_t divides sin, 1 - cos and the length.
NON_FINITE_DUBINS = (0.0, 0.0, 0.3, 0.0, 0.0, 1.0, 1e-310)


def test_an_accepted_dubins_pair_gives_a_non_finite_course(exe, tmp_path):
    """What tests/test_gpu_track_chain.py puts between ordinary pairs, confirmed on the CPU with the kernel's own routines:
    the curve is prepared, has 62 points, 61 of them NaN, and the per-course decision is 4; the same pair at curvature 1e-300
    and at 1.0 is finite."""
    rows = np.array([NON_FINITE_DUBINS, NON_FINITE_DUBINS[:6] + (1e-300,), NON_FINITE_DUBINS[:6] + (1.0,)])
    assert np.all(np.abs(rows[:, :6]) <= 1e6) and np.all((rows[:, 6] > 0.0) & (rows[:, 6] <= 1e300))      # steer_check's bounds
    got = run_exe(exe, "dubins", rows.reshape(-1), tmp_path).reshape(3, 4)
    assert got.tolist() == [[1.0, 62.0, 61.0, 4.0], [1.0, 62.0, 0.0, 0.0], [1.0, 62.0, 0.0, 0.0]]


def python_pick(find, ood, t_last, indices):
    """TrackResult.best(indices) restated: search_best_feasible_path (rrt_10:1495-1524), passing over ood != 0."""
    best_time, win = float("inf"), -1
    for i in indices:
        if ood[i] == 0 and find[i] and best_time >= t_last[i]:
            best_time, win = t_last[i], i
    return win


def test_group_pick_equals_the_python_rule(exe, tmp_path):
    """The 240 records of tests/golden/track_kat.npz (track_batch_kat.npz holds 36) cut into groups of 1, 7 (the last one
    of 2: 240 is no multiple of 7) and 240.  Equal values of t_last are written into pairs of feasible records so that
    equal times meet at the first, a middle and the last position of groups, and some records get ood 1 .. 5, winners of
    their group among them."""
    g = np.load(os.path.join(tu.GOLD, "track_kat.npz"))
    n = len(g["out"])
    assert n == 240
    find = g["out"][:, 0].astype(np.int64)
    t_last = g["last"][:, 0].copy()
    ood = np.zeros(n, dtype=np.int64)
    feas = np.nonzero(find)[0]
    assert len(feas) >= 60
    tmin = 0.5 * float(t_last[feas][t_last[feas] > 0.0].min())   # below every positive time of the file
    for j in range(0, n // 7):            # a tie of the smallest time at positions 0 and 6, 3 and 6, 0 and 3 in turn
        a, b = ((0, 6), (3, 6), (0, 3))[j % 3]
        for q in (a, b):
            find[7 * j + q] = 1
            t_last[7 * j + q] = tmin * (1.0 + (j % 5) / 8.0)
    ood[np.arange(5, n, 11)] = 1 + np.arange(len(np.arange(5, n, 11))) % 5
    ood[[0, 6, 21, 27]] = (2, 4, 3, 5)    # tied winners of groups 0 and 3 lose their record
    sizes = {1: [1] * n, 7: [7] * (n // 7) + [n % 7], 240: [n]}
    for gsz, cut in sizes.items():
        got = run_exe(exe, "pick", np.concatenate([[n], np.stack([find, ood, t_last], axis=1).reshape(-1), [len(cut)], cut]),
                      tmp_path)
        starts = np.concatenate([[0], np.cumsum(cut)])
        want = [python_pick(find, ood, t_last, range(starts[k], starts[k + 1])) for k in range(len(cut))]
        assert got.astype(np.int64).tolist() == want, gsz
        assert any(w >= 0 for w in want)
    want7 = [python_pick(find, ood, t_last, range(7 * k, 7 * k + 7)) for k in range(n // 7)]
    pair = [((0, 6), (3, 6), (0, 3))[k % 3] for k in range(n // 7)]
    decided = {w % 7 for k, w in enumerate(want7) if w >= 0 and w % 7 == pair[k][1] and ood[7 * k + pair[k][0]] == 0}
    assert decided == {3, 6}        # groups won by the later of two equal times, at a middle and at the last position


# ---- Python ---------------------------------------------------------------------------------------------------------------
def test_device_keywords_with_host_courses_raise():
    import rrt_amd
    bt = rrt_amd.BatchTrack.__new__(rrt_amd.BatchTrack)      # no device is needed to be refused
    trip = [([0.0, 0.2, 0.4], [0.0] * 3, [0.0] * 3)] * 2
    for kw in (dict(select="free"), dict(select=[True, False]), dict(group=2), dict(group=True), dict(arrays="best")):
        with pytest.raises(ValueError):
            bt.run(trip, **kw)


def test_device_points_are_refused_for_lqr_and_for_candidates():
    import rrt_amd
    A = rrt_amd._abi
    bs = rrt_amd.BatchSteer.__new__(rrt_amd.BatchSteer)
    bs.kind = A.STEER_LQR
    with pytest.raises(ValueError, match="no yaw"):
        bs.plan(np.zeros((1, 2)), np.ones((1, 2)), points="device")
    bs.kind = A.STEER_RS
    with pytest.raises(ValueError, match="plan_free"):
        bs.candidates(np.zeros((1, 3)), np.ones((1, 3)), 1.0, points="device")


class Owner:
    """What pack_source reads of a producer's native object."""
    _s = C.c_void_p(0x1000)

    def generation(self):
        return 3


def test_pack_source_fills_the_struct():
    import rrt_amd
    A = rrt_amd._abi
    pack_source = rrt_amd.track.pack_source
    dc = A.DeviceCourses(A.SRC_SPLINE, Owner())
    src, keep = pack_source(dc, 6)
    assert (src.kind, src.select, src.object, src.generation, src.mask, src.group, src.arrays_of) == (2, 0, 0x1000, 3, None, 0, 0)
    src, keep = pack_source(dc, 6, select="free", group=3, arrays="best")
    assert (src.select, src.mask, src.group, src.arrays_of) == (A.SELECT_FREE, None, 3, 1)
    src, keep = pack_source(dc, 6, select=np.array([1, 0, 0, 2, 0, 1]), group=2, arrays=False)
    assert src.select == A.SELECT_MASK and src.mask == keep["mask"].ctypes.data and src.arrays_of == 0
    assert keep["mask"].dtype == np.uint8 and keep["mask"].tolist() == [1, 0, 0, 1, 0, 1]
    for bad in (dict(select="all"), dict(select=[True] * 5), dict(group=0), dict(arrays="best")):
        with pytest.raises(ValueError):
            pack_source(dc, 6, **bad)


def test_statuses_4_and_5_have_messages_of_their_own():
    import rrt_amd
    TrackResult, RrtxError = rrt_amd.track.TrackResult, rrt_amd._abi.RrtxError
    rec = np.zeros(4, dtype=rrt_amd._abi.TRACK_RECORD)
    rec["ood"] = [1, 4, 5, 0]
    rec["len"] = [0, 0, 0, 2]
    res = TrackResult(rec, np.array([0, 0, 0, 0, 2]), [np.arange(2.0)] * 7, np.zeros((4, 3)))
    with pytest.raises(RrtxError, match="tan replica"):
        res.feasible(0)
    with pytest.raises(RrtxError, match="not finite") as e4:
        res.feasible(1)
    with pytest.raises(RrtxError, match="left out by select") as e5:
        res.feasible(2)
    assert "tan replica" not in str(e4.value) and "tan replica" not in str(e5.value)
    assert res.feasible(3)[0] is False and res.winner is None
    with pytest.raises(RrtxError):
        res.best_of(0)                    # a run without a group has no winners


def test_best_of_reads_the_device_pick_and_appends_the_goal():
    import rrt_amd
    TrackResult = rrt_amd.track.TrackResult
    rec = np.zeros(4, dtype=rrt_amd._abi.TRACK_RECORD)
    rec["find_goal"] = [1, 1, 0, 0]
    rec["len"] = [2, 2, 2, 2]
    rec["t_last"] = [0.05, 0.05, 0.05, 0.05]
    arrays = [np.arange(2.0) + 10 * k for k in range(7)]          # arrays="best": only course 1 owns entries
    arrays[4] = np.array([0.0, 0.05])
    goals = np.full((4, 3), np.nan)
    goals[1] = (7.0, 8.0, 9.0)
    fetched = []

    def lazy():
        fetched.append(1)
        return goals
    res = TrackResult(rec, np.array([0, 0, 2, 2, 2]), arrays, lazy, winner=np.array([1, -1], dtype=np.int32), group=2)
    assert not fetched
    assert res.best_of(0) == (True, [0.0, 1.0, 7.0], [10.0, 11.0, 8.0], [20.0, 21.0, 9.0], [30.0, 31.0], [0.0, 0.05],
                              [50.0, 51.0], [60.0, 61.0], (7.0, 8.0, 9.0))
    assert res.best_of(1) == (False,) + (None,) * 8 and fetched == [1]
    with pytest.raises(rrt_amd._abi.RrtxError, match="no winner"):
        res.feasible(0)

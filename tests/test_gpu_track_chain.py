"""Tracking courses where a producer left them on the device (points="device" / arrays="device", rrtx_tracker_run_from).
The yardstick is the host path the goldens pin: for the same inputs run(device_result) and run(host_result) must agree bit
for bit in every record column, the offsets, the seven arrays, rc and steps -- the same roll_course runs on the same
doubles, so no tolerance is needed.  Every chain test first asserts that the result holds no point array and has
device_courses: "device" is truthy, and without the feature the producers would silently fetch the points."""
import warnings

import numpy as np
import pytest

import util  # noqa: F401
import bezier_util as zu
import bspline_util as bu
import spline_util as su
import track_util as tu

pytestmark = pytest.mark.gpu
REC_FIELDS = ("find_goal", "length", "fail", "status")
ARRAYS = ("x", "y", "yaw", "v", "t", "a", "d")
CIRCLES = [(3.0, 3.0, 0.5), (8.0, 2.0, 1.0), (-2.0, 5.0, 0.7), (12.0, 12.0, 1.5)]
PARTIAL = 1


@pytest.fixture(scope="module")
def bt():
    import rrt_amd
    with rrt_amd.BatchTrack(T=20.0) as b:      # at most 401 steps a roll-out: the comparison is of code paths, not of the model
        yield b


@pytest.fixture(scope="module")
def steers():
    import rrt_amd
    made = {k: rrt_amd.BatchSteer(k) for k in ("dubins", "rs", "bezier")}
    yield made
    for s in made.values():
        s.close()


def assert_same_records(a, b, what="", rows=None):
    for f in REC_FIELDS:
        assert np.array_equal(getattr(a, f)[rows] if rows is not None else getattr(a, f), getattr(b, f)), (what, f)
    assert np.array_equal(tu.bits(a.t_last[rows] if rows is not None else a.t_last), tu.bits(b.t_last)), (what, "t_last")


def assert_same_run(dev, host, what=""):
    assert_same_records(dev, host, what)
    assert np.array_equal(dev.offsets, host.offsets), what
    for k in ARRAYS:
        assert np.array_equal(tu.bits(getattr(dev, k)), tu.bits(getattr(host, k))), (what, k)
    assert dev.rc == host.rc and dev.steps == host.steps and len(dev) == len(host), what


def assert_on_device(res, what=""):
    assert res.x is None and res.y is None and res.yaw is None and res.device_courses is not None, what


def track_kw(n, variant, first):
    """Keywords of run() for n courses.  "shared": one obstacle list, and robot radius, thresholds and start states per
    course (each roll-out starts at its course's first pose `first`, moving); "lists": an obstacle list per course (none,
    one, ... up to three rows), scalars, and the reference's start state."""
    rs = np.random.RandomState(n + len(variant))
    if variant == "shared":
        return dict(obstacle_list=CIRCLES, robot_radius=rs.uniform(0.0, 0.4, n), target_speed=rs.uniform(1.5, 4.0, n),
                    yaw_th=rs.uniform(0.02, 0.3, n), invalid_travel_ratio=rs.uniform(1.2, 6.0, n),
                    start_state=np.concatenate([first, rs.uniform(0.0, 1.0, (n, 1))], axis=1))
    lists = [[(rs.uniform(-5, 15), rs.uniform(-5, 15), rs.uniform(0.2, 1.5)) for _ in range(i % 4)] for i in range(n)]
    return dict(course_obstacles=lists, robot_radius=0.25, start_state=None)


def chain(bt, produce, first, what, complete=1):
    """produce(points) solves on one producer: the host result is tracked, then the device result, under both keyword sets."""
    seen = set()
    for variant in ("shared", "lists"):
        host_res = produce(True)
        assert host_res.x is not None and getattr(host_res, "device_courses", None) is None, what
        kw = track_kw(len(host_res.status), variant, first)
        host = bt.run(host_res, **kw)
        dev_res = produce("device")
        assert_on_device(dev_res, what)
        assert np.array_equal(dev_res.offsets, host_res.offsets) and np.array_equal(dev_res.status, host_res.status), what
        dev = bt.run(dev_res, **kw)
        assert_same_run(dev, host, (what, variant))
        assert dev.kernel_ms > 0.0 and np.sum(dev.status == 0) >= complete, (what, variant)
        for i in np.nonzero(dev.status == 0)[0][:3]:      # the lazily fetched goals are the courses' last points
            assert np.array_equal(tu.bits(dev.goals[i]), tu.bits(host.goals[i])), (what, i)
        seen |= set(dev.status.tolist())
    return seen


# ---- 1. every source --------------------------------------------------------------------------------------------------------
def steer_kat():
    import os
    g = np.load(os.path.join(tu.GOLD, "steer_kat.npz"))
    return {k: g[k] for k in g.files}


def test_dubins_plan_with_pairs_without_a_curve(bt, steers):
    import rrt_amd
    g = steer_kat()
    keys = [tuple(g["d_sel"][i][:g["d_nsel"][i]]) if g["d_nsel"][i] >= 0 else None for i in range(len(g["d_n"]))]
    rows = [i for i in range(len(keys)) if keys[i] is not None and g["d_n"][i] < 0]
    assert rows
    key = keys[rows[0]]                   # a word list under which some pairs of the file have no curve ...
    sel = [rrt_amd._abi.DUBINS_WORDS[w] for w in key]
    inp = g["d_inp"]                      # ... applied to every pair of the file
    seen = chain(bt, lambda p: steers["dubins"].plan(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy(), selected_types=sel, points=p),
                 inp[:, 0:3], "dubins plan", complete=8)
    assert {0, 2} <= seen                 # status-2 rows sit between complete ones


def test_reeds_shepp_plan(bt, steers):
    inp = steer_kat()["r_inp"]
    chain(bt, lambda p: steers["rs"].plan(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy(), step_size=0.05, points=p), inp[:, 0:3],
          "rs plan", complete=8)


def test_bezier_plan_and_control_points(bt, steers):
    pose = zu.kat()["pose"][:40]
    chain(bt, lambda p: steers["bezier"].plan(pose[:, 0:3], pose[:, 3:6], pose[:, 6].copy(), n_points=37, points=p),
          pose[:, 0:3], "bezier plan", complete=20)
    (m, npts), idx = sorted(zu.cp_groups().items(), key=lambda kv: -len(kv[1]))[0]
    cps = np.stack([zu.control_points(i) for i in idx])
    first = np.concatenate([cps[:, 0, :], np.zeros((len(cps), 1))], axis=1)
    chain(bt, lambda p: steers["bezier"].plan_control_points(cps, n_points=max(npts, 3), points=p), first, "bezier control points")


@pytest.mark.parametrize("kind", ["dubins", "rs"])
def test_plan_free_with_obstacles(bt, steers, kind):
    g = steer_kat()
    inp = g["d_inp"][:32] if kind == "dubins" else g["r_inp"]
    step = {} if kind == "dubins" else dict(step_size=0.2)
    obs = [(float(inp[:, 3].mean()), float(inp[:, 4].mean()), 1.0), (1.0, 1.0, 0.4)]
    chain(bt, lambda p: steers[kind].plan_free(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy(), obstacle_list=obs, robot_radius=0.2,
                                               points=p, **step), inp[:, 0:3], kind + " plan_free", complete=4)


def first_poses(courses):
    return np.array([[c[0][0], c[1][0], np.arctan2(c[1][1] - c[1][0], c[0][1] - c[0][0])] for c in courses])


def test_spline_run(bt):
    import rrt_amd
    crs, g = su.courses(), su.kat()
    with rrt_amd.BatchSpline() as sp:
        seen = chain(bt, lambda a: sp.run(crs, ds=g["ds"], obstacle_list=g["obs"], robot_radius=float(g["rr"]), arrays=a),
                     first_poses(crs), "spline run", complete=8)
    assert 0 in seen


@pytest.mark.parametrize("call", ["interpolate", "spline2d", "approximate"])
def test_bspline_calls(bt, call):
    import rrt_amd
    crs, kw, _ = bu.run_kwargs(1 if call == "spline2d" else 0)
    if call == "approximate":
        kw = dict(n_path_points=kw["n_path_points"], degree=kw["degree"], u=kw["u"], s=[0.5 * (i % 3) for i in range(len(crs))])
    with rrt_amd.BatchBSpline() as bs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # approximate() names fits that stopped early
            chain(bt, lambda a: getattr(bs, call)(crs, obstacle_list=CIRCLES, robot_radius=0.1, arrays=a, **kw),
                  first_poses(crs), "bspline " + call, complete=4)


# ---- 2. capacity boundaries, 3. more jobs than resident blocks ---------------------------------------------------------------
@pytest.mark.parametrize("n_points,status", [(2, 2), (3, 0), (448, 0), (449, 0), (960, 0), (961, 3)])
def test_capacity_boundaries(bt, steers, n_points, status):
    """Refused below 3 points, LDS up to 448, the slab from 449, the cap at 960, refused above it: each row the host path's."""
    st, go, off = zu.random_poses(n_points, 5)
    host = bt.run(steers["bezier"].plan(st, go, off, n_points=n_points), obstacle_list=CIRCLES, robot_radius=0.2)
    res = steers["bezier"].plan(st, go, off, n_points=n_points, points="device")
    assert_on_device(res)
    dev = bt.run(res, obstacle_list=CIRCLES, robot_radius=0.2)
    assert dev.status.tolist() == [status] * 5
    assert_same_run(dev, host, n_points)
    assert dev.rc == (PARTIAL if status else 0) and (dev.steps > 0) == (status == 0)


def test_more_jobs_than_resident_blocks(bt, steers):
    """4 320 curves of 50 points, above the 4 096 blocks of 256 CUs x 16: every block takes further jobs from the queue."""
    st, go, off = zu.random_poses(11, 4320, hi=12.0)
    host = bt.run(steers["bezier"].plan(st, go, off, n_points=50), obstacle_list=CIRCLES, robot_radius=0.2, arrays=False)
    res = steers["bezier"].plan(st, go, off, n_points=50, points="device")
    assert_on_device(res)
    dev = bt.run(res, obstacle_list=CIRCLES, robot_radius=0.2, arrays=False)
    assert len(dev) == 4320 and dev.x is None and np.all(dev.status == 0)
    assert_same_records(dev, host)
    assert dev.steps == host.steps and dev.rc == host.rc == 0 and np.array_equal(dev.offsets, host.offsets)


# ---- 4. a non-finite course -----------------------------------------------------------------------------------------------------
def test_a_non_finite_course_gets_status_4_and_its_neighbours_are_untouched(bt, steers):
    """A Dubins pair with a subnormal curvature is accepted by the planner and its curve is NaN from the second point on
    (confirmed on the CPU by tests/test_track_chain_host.py).  The host path refuses the whole batch for it; on the device
    that course alone gets status 4 and owns nothing, and the others are what the host path gives without it."""
    import rrt_amd
    from test_track_chain_host import NON_FINITE_DUBINS
    inp = steer_kat()["d_inp"][:12]
    at = 5
    rows = np.insert(inp, at, NON_FINITE_DUBINS, axis=0)
    others = np.arange(13) != at
    kw = track_kw(13, "shared", rows[:, 0:3])
    sub = {k: (v[others] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    dub = steers["dubins"]
    host = bt.run(dub.plan(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy()), **sub)
    assert host.rc == 0 and np.all(host.status == 0)
    with_it = dub.plan(rows[:, 0:3], rows[:, 3:6], rows[:, 6].copy())
    a, b = int(with_it.offsets[at]), int(with_it.offsets[at + 1])
    assert with_it.status[at] == 0 and b - a == 62 and not np.any(np.isfinite(with_it.x[a + 1:b]))      # the device's curve too
    with pytest.raises(rrt_amd._abi.RrtxError, match="not finite"):
        bt.run(with_it, **kw)
    res = dub.plan(rows[:, 0:3], rows[:, 3:6], rows[:, 6].copy(), points="device")
    assert_on_device(res)
    dev = bt.run(res, **kw)
    assert dev.rc == PARTIAL and dev.status.tolist() == [0] * at + [4] + [0] * (12 - at)
    assert dev.length[at] == 0 and dev.offsets[at] == dev.offsets[at + 1] and dev.find_goal[at] == 0
    with pytest.raises(rrt_amd._abi.RrtxError, match="not finite"):
        dev.feasible(at)
    assert_same_records(dev, host, "neighbours", np.nonzero(others)[0])
    assert np.array_equal(np.diff(dev.offsets)[others], np.diff(host.offsets)) and dev.steps == host.steps
    for k in ARRAYS:
        assert np.array_equal(tu.bits(getattr(dev, k)), tu.bits(getattr(host, k))), k


# ---- 5. stale and wrong-state sources ------------------------------------------------------------------------------------------
def test_stale_and_wrong_state_sources_launch_nothing(bt, steers):
    import rrt_amd
    RrtxError = rrt_amd._abi.RrtxError
    st, go, off = zu.random_poses(3, 6)
    bz = steers["bezier"]
    good = bt.run(bz.plan(st, go, off, n_points=20, points="device"))
    good_goals = good.goals.copy()         # fetched now: the tracker keeps them until its next run only
    ms = bt._tracker.kernel_ms()
    counts = bt._tracker.counts()
    old = bz.plan(st, go, off, n_points=20, points="device")
    bz.plan(st, go, off, n_points=20, points="device")              # the producer solves again: `old` is stale
    with pytest.raises(RrtxError, match="stale"):
        bt.run(old)
    lean = bz.plan(st, go, off, n_points=20, points=False)
    lean.device_courses = rrt_amd._abi.DeviceCourses(rrt_amd._abi.SRC_STEER, bz._steer)      # a source without points
    with pytest.raises(RrtxError, match="no points"):
        bt.run(lean)
    bare = bz.plan(st, go, off, n_points=20, points="device")       # planned without obstacles
    with pytest.raises(RrtxError, match="obstacle list"):
        bt.run(bare, select="free")
    assert bt._tracker.kernel_ms() == ms and bt._tracker.counts() == counts      # nothing was launched, the last run stands
    # a producer re-solved or destroyed after the run leaves the result as it is
    with rrt_amd.BatchSteer("bezier") as own:
        res = bt.run(own.plan(st, go, off, n_points=20, points="device"))
        before = [getattr(res, k).copy() for k in REC_FIELDS + ARRAYS]
        own.plan(go, st, off, n_points=33)
    for k, v in zip(REC_FIELDS + ARRAYS, before):
        assert np.array_equal(getattr(res, k), v), k
    assert_same_run(res, good)
    assert np.array_equal(tu.bits(res.goals), tu.bits(good_goals))      # fetched from the tracker, not from the producer
    dead = rrt_amd.BatchSteer("bezier")
    late = dead.plan(st, go, off, n_points=20, points="device")
    dead.close()
    with pytest.raises(RrtxError):
        bt.run(late)                     # the destroyed producer's result is refused, not read


# ---- 6. selection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["free", "mask"])
def test_selection_leaves_the_others_unread(bt, steers, how):
    inp = steer_kat()["r_inp"]
    n = len(inp)
    obs = [(float(inp[:, 3].mean()), float(inp[:, 4].mean()), 1.5), (1.0, 1.0, 0.8)]
    args = (inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy())
    host_res = steers["rs"].plan(*args, step_size=0.2, obstacle_list=obs, robot_radius=0.2)
    keep = host_res.free if how == "free" else (np.arange(n) % 3 != 1)
    assert 0 < keep.sum() < n
    kw = track_kw(n, "shared", inp[:, 0:3])
    trip = [(host_res.x[a:b], host_res.y[a:b], host_res.yaw[a:b]) for a, b in zip(host_res.offsets[:-1], host_res.offsets[1:])]
    rows = np.nonzero(keep)[0]
    host = bt.run([trip[i] for i in rows], **{k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    res = steers["rs"].plan(*args, step_size=0.2, obstacle_list=obs, robot_radius=0.2, points="device")
    assert_on_device(res)
    dev = bt.run(res, select="free" if how == "free" else keep, **kw)
    out = np.nonzero(~keep)[0]
    assert np.all(dev.status[out] == 5) and np.all(dev.length[out] == 0) and np.all(np.diff(dev.offsets)[out] == 0)
    assert_same_records(dev, host, how, rows)
    assert np.array_equal(np.diff(dev.offsets)[rows], np.diff(host.offsets)) and dev.steps == host.steps
    for k in ARRAYS:
        assert np.array_equal(tu.bits(getattr(dev, k)), tu.bits(getattr(host, k))), k
    assert dev.rc == host.rc and (dev.rc == 0) == bool(np.all(host.status == 0))


# ---- 7. groups --------------------------------------------------------------------------------------------------------------------
def python_pick(res, indices):
    best_time, win = float("inf"), -1
    for i in indices:
        if res.status[i] == 0 and res.find_goal[i] and best_time >= res.t_last[i]:
            best_time, win = res.t_last[i], i
    return win


def test_groups_pick_on_the_device_and_best_arrays(steers):
    import rrt_amd
    rs = np.random.RandomState(7)
    ns, ng = 16, 12
    starts = np.stack([rs.uniform(-1, 1, ns), rs.uniform(-1, 1, ns), rs.uniform(-0.5, 0.5, ns)], axis=1)
    goals = np.stack([rs.uniform(4, 12, ng), rs.uniform(-6, 6, ng), rs.uniform(-1.0, 1.0, ng)], axis=1)
    goals[6:] = goals[:6]         # every goal twice: whichever course wins a group, its twin has the same t_last
    obs = [(6.0, 0.0, 1.0), (9.0, 3.0, 0.8), (5.0, -4.0, 0.6)]
    plan = dict(step_size=0.2, product=True, obstacle_list=obs, robot_radius=0.2)
    state = np.repeat(np.concatenate([starts, np.zeros((ns, 1))], axis=1), ng, axis=0)
    kw = dict(obstacle_list=obs, robot_radius=0.2, start_state=state, yaw_th=0.2)
    with rrt_amd.BatchTrack(T=30.0) as bt:
        host = bt.run(steers["rs"].plan_free(starts, goals, 1.0, **plan), **kw)
        res = steers["rs"].plan_free(starts, goals, 1.0, points="device", **plan)
        assert_on_device(res)
        full = bt.run(res, group=True, **kw)
        assert_same_run(full, host)
        assert full.group == ng and len(full.winner) == ns
        want = [python_pick(host, range(j * ng, (j + 1) * ng)) for j in range(ns)]
        assert full.winner.tolist() == want and sum(w >= 0 for w in want) >= 4
        for w in want:                # every group with a winner is decided by the later of two equal times
            if w >= 0:
                assert w % ng >= 6 and host.find_goal[w - 6] and tu.bits(host.t_last[w - 6]) == tu.bits(host.t_last[w]), w
        for j in range(ns):
            done = [i for i in range(j * ng, (j + 1) * ng) if host.status[i] == 0]
            ref = host.best(indices=done)
            got = full.best_of(j)
            assert got[0] is ref[0]
            if ref[0]:
                for a, b in zip(got[1:8], ref[1:]):
                    assert np.array_equal(tu.bits(a), tu.bits(b)), j
                assert np.array_equal(tu.bits(got[8]), tu.bits(host.goals[want[j]])), j      # the course's last point
            else:
                assert got[1:] == (None,) * 8
        res = steers["rs"].plan_free(starts, goals, 1.0, points="device", **plan)
        best = bt.run(res, group=ng, arrays="best", **kw)
        assert_same_records(best, host)
        assert best.winner.tolist() == want
        owns = np.diff(best.offsets)
        wins = np.array([w for w in want if w >= 0])
        assert np.array_equal(np.nonzero(owns)[0], wins) and np.array_equal(owns[wins], host.length[wins])
        assert best.steps == int(host.length[wins].sum()) == len(best.x)
        for w in wins:
            a, b, c, d = best.offsets[w], best.offsets[w + 1], host.offsets[w], host.offsets[w + 1]
            for k in ARRAYS:
                assert np.array_equal(tu.bits(getattr(best, k)[a:b]), tu.bits(getattr(host, k)[c:d])), (w, k)
        for j in range(ns):
            if want[j] < 0:
                assert np.all(owns[j * ng:(j + 1) * ng] == 0) and best.best_of(j)[0] is False
            else:
                assert best.best_of(j) == full.best_of(j)


# ---- 8. reuse ---------------------------------------------------------------------------------------------------------------------
def test_one_tracker_alternates_host_and_device_runs(steers):
    import rrt_amd
    RrtxError = rrt_amd._abi.RrtxError
    bz = steers["bezier"]
    sets = {n: zu.random_poses(20 + n, n, hi=12.0) for n in (40, 6, 90, 12)}

    def plan(n, points):
        st, go, off = sets[n]
        return bz.plan(st, go, off, n_points=30, points=points)
    with rrt_amd.BatchTrack(T=20.0) as ref, rrt_amd.BatchTrack(T=20.0) as b:
        want = {n: ref.run(plan(n, True), obstacle_list=CIRCLES, robot_radius=0.2) for n in sets}
        first = b.run(plan(40, True), obstacle_list=CIRCLES, robot_radius=0.2)                 # host, 40
        assert_same_run(first, want[40])
        with pytest.raises(RrtxError):
            b._tracker.winners()                                                                # a host run has no winners
        dev = b.run(plan(6, "device"), obstacle_list=CIRCLES, robot_radius=0.2)                 # device, shrinking to 6
        assert_same_run(dev, want[6])
        assert b._tracker.counts() == (6, want[6].steps)
        with pytest.raises(RrtxError):
            b._tracker.winners()
        grouped = b.run(plan(90, "device"), obstacle_list=CIRCLES, robot_radius=0.2, group=9)   # grouped, growing to 90
        assert_same_run(grouped, want[90])
        assert len(grouped.winner) == 10 and b._tracker.counts() == (90, want[90].steps)
        assert grouped.winner.tolist() == [python_pick(want[90], range(9 * j, 9 * j + 9)) for j in range(10)]
        with pytest.raises(RrtxError, match="run again"):
            dev.goals                                                                           # its goals were never fetched
        last = b.run(plan(12, True), obstacle_list=CIRCLES, robot_radius=0.2)                   # host again, 12
        assert_same_run(last, want[12])
        assert last.winner is None and b._tracker.counts() == (12, want[12].steps)
        with pytest.raises(RrtxError):
            b._tracker.winners()
        with pytest.raises(RrtxError):
            b._tracker.goals(12)

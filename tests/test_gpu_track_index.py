"""The tracker's obstacle index on the GPU (track_courses_kernel / track_source_kernel<CHECK_INDEX>,
rrtx_tracker_set_obstacle_index, BatchTrack(obstacle_index=True)): the reference's records against lists of 65, 300 and 1 000
circles bit for bit, ON against OFF wherever both apply, a circle forged onto one single sample of a roll-out at the steps
around the 64-step flush of the deferred check, the touching circle at the rows around the old limit of 64, and the
expectation dx*dx + dy*dy <= (size + r)**2 in IEEE doubles over the device's own arrays.  Every comparison is exact."""
import os

import numpy as np
import pytest

import obsindex_util as OI
import track_util as tu
import util  # noqa: F401
from test_gpu_track_batch import ARRAYS, assert_same_arrays, assert_same_records, assert_vector, csr_inputs
from test_track_batch_host import kat_vectors

pytestmark = pytest.mark.gpu
F_COLL = 8
LISTS = (65, 300, 1000)


@pytest.fixture(scope="module")
def on(gpu):
    import rrt_amd
    with rrt_amd.BatchTrack(obstacle_index=True) as b:
        yield b


@pytest.fixture(scope="module")
def on20(gpu):
    """T = 20: at most 402 samples a roll-out, for the tests whose expectation is computed per circle in numpy"""
    import rrt_amd
    with rrt_amd.BatchTrack(T=20.0, obstacle_index=True) as b:
        yield b


@pytest.fixture(scope="module")
def off(gpu):
    import rrt_amd
    with rrt_amd.BatchTrack() as b:
        yield b


def load(name):
    g = np.load(os.path.join(tu.GOLD, name))
    return {k: g[k] for k in g.files}


def city(seed, m, lo, hi, smin, smax):
    rs = np.random.RandomState(seed)
    return np.column_stack([rs.uniform(lo, hi, m), rs.uniform(lo, hi, m), rs.uniform(smin, smax, m)])


def course_kw(vecs):
    return dict(courses=[(v[3], v[4], v[5]) for v in vecs], target_speed=[v[0]["target_speed"] for v in vecs],
                yaw_th=[v[0]["yaw_th"] for v in vecs], invalid_travel_ratio=[v[0]["invalid_travel_ratio"] for v in vecs],
                start_state=np.array([v[6] for v in vecs]).reshape(-1, 4))


def expected_coll(res, circles, rr):
    """Per course: some circle touches some stored point -- numpy's dx*dx + dy*dy <= (size + r)**2 over the device's arrays."""
    hit = OI.first_hit_linear(circles, rr, res.x, res.y) >= 0
    return np.array([hit[a:b].any() for a, b in zip(res.offsets[:-1], res.offsets[1:])])


def assert_coll_is(res, base, coll, what=""):
    """res is the unobstructed `base` with the collision bit where `coll` says, and find_goal following fail."""
    assert np.array_equal(res.fail, base.fail | np.where(coll, F_COLL, 0)), what
    assert np.array_equal(res.find_goal, (res.fail == 0).astype(res.find_goal.dtype)), what
    assert np.array_equal(res.length, base.length) and np.array_equal(res.status, base.status), what
    assert np.array_equal(tu.bits(res.t_last), tu.bits(base.t_last)), what


# ---- the reference's answers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", LISTS)
def test_golden_rows_with_the_index(on, m):
    g = load("track_index_kat.npz")
    vecs = kat_vectors(g)
    want = dict(out=g["out_%d" % m], last=g["last_%d" % m], sums=g["sums_%d" % m])
    res = on.run(obstacle_list=g["obs_%d" % m], robot_radius=0.1, **course_kw(vecs))
    assert res.rc == 0 and len(res) == len(vecs) >= 16
    info = res.obstacle_index
    assert info["used"] and info["reason"] == "used" and info["mode"] == OI.ON and info["n_circles"] == m
    for i in range(len(vecs)):
        assert_vector(res, i, want, i)
    assert np.array_equal((res.fail & F_COLL) != 0, g["first_%d" % m] >= 0)
    assert np.any((g["first_%d" % m] >= 64) & ((res.fail & F_COLL) != 0))       # blocked by a row past the old limit alone
    lean = on.run(obstacle_list=g["obs_%d" % m], robot_radius=0.1, arrays=False, **course_kw(vecs))
    assert_same_records(lean, res, m)
    assert lean.x is None and np.array_equal(lean.offsets, res.offsets)


# ---- ON against OFF -----------------------------------------------------------------------------------------------------------------
def test_every_vector_with_1_to_64_obstacles_on_equals_off(on, off):
    vecs = [v for v in kat_vectors(load("track_batch_kat.npz")) if 1 <= len(v[1]) <= 64]
    assert len(vecs) >= 8 and {len(v[1]) for v in vecs} >= {1, 63, 64}
    seen = set()
    for v in vecs:
        kw = dict(obstacle_list=v[1], robot_radius=v[2], **course_kw([v]))
        a, b = on.run(**kw), off.run(**kw)
        assert a.obstacle_index["used"] and (b.obstacle_index["used"], b.obstacle_index["reason"]) == (False, "off")
        assert_same_records(a, b, len(v[1]))
        assert_same_arrays(a, b, len(v[1]))
        seen.add(bool(a.fail[0] & F_COLL))
    assert seen == {True, False}


# ---- a circle on one single sample ------------------------------------------------------------------------------------------------
LONG = (np.linspace(0.0, 479.5, 960), np.zeros(960), np.zeros(960))     # never reached within 100 s
SHORT = (np.array([0.0, 0.1, 0.2]), np.zeros(3), np.zeros(3))           # reached by the first step: one sample
MOVING = [0.0, 0.0, 0.0, 1.0]                                           # v = 1: no two samples coincide


@pytest.mark.parametrize("n", [1, 2, 64, 65, 129, 2002])
def test_a_circle_on_one_sample_of_the_roll_out(gpu, n):
    import rrt_amd
    dt = 0.05
    with rrt_amd.BatchTrack(T=(n - 2) * dt + dt / 2 if n > 1 else 100.0, dt=dt, obstacle_index=True) as bt:
        kw = dict(courses=[SHORT if n == 1 else LONG], start_state=MOVING)
        base = bt.run(**kw)
        assert base.length[0] == n == len(base.x) and base.status[0] == 0 and base.obstacle_index is None
        assert not base.fail[0] & F_COLL
        ks = sorted({k for k in (0, 1, 62, 63, 64, 65, n - 2, n - 1) if 0 <= k < n})
        size = 5e-4
        for k in ks:
            for shift, touches in ((0.0, True), (1e-3, False)):
                circle = np.array([[base.x[k], base.y[k] + shift, size]])
                dx, dy = circle[0, 0] - base.x, circle[0, 1] - base.y      # the test's own premise, on the CPU
                touched = np.nonzero(dx * dx + dy * dy <= size ** 2)[0]
                assert touched.tolist() == ([k] if touches else []), (n, k, shift)
                res = bt.run(obstacle_list=circle, robot_radius=0.0, **kw)
                assert res.obstacle_index["used"]
                assert_coll_is(res, base, np.array([touches]), (n, k, shift))
                assert_same_arrays(res, base, (n, k, shift))


# ---- the rows around the old limit ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def few(on20):
    """Four courses of the golden and their unobstructed run (T = 20)."""
    vecs = kat_vectors(load("track_index_kat.npz"))[:4]
    kw = course_kw(vecs)
    return kw, on20.run(**kw)


@pytest.mark.parametrize("m", [65, 257, 1000, 20000])
def test_the_touching_circle_at_the_rows_around_64(on20, few, monkeypatch, m):
    on = on20
    kw, base = few
    lo = min(base.x.min(), base.y.min()) - 1.0
    hi = max(base.x.max(), base.y.max()) + 1.0
    k = int(base.offsets[0] + base.length[0] // 2)             # a sample in the middle of course 0
    x0, y0 = base.x[:base.offsets[1]], base.y[:base.offsets[1]]
    cells = {65: (None, 1, 7, None), 257: (1, None, None, 7), 1000: (7, 1, None, 1), 20000: (None, 7, 7, None)}[m]
    for row, rr, forced in zip((0, 63, 64, m - 1), (0.0, 0.25, 0.0, 0.25), cells):
        c = city(m + row, m, lo, hi, 0.005, 0.02)
        # course 0 is touched by row `row` alone: the dots that would touch it move onto a dot that does not
        dx, dy = c[:, 0][:, None] - x0[None, :], c[:, 1][:, None] - y0[None, :]
        near = np.any(dx * dx + dy * dy <= ((c[:, 2] + rr + 1e-6) ** 2)[:, None], axis=1)
        assert 0 < near.sum() < m // 2 or not near.any()
        c[near] = c[np.nonzero(~near)[0][0]]
        c[row] = (base.x[k], base.y[k], 0.01)
        if forced:
            monkeypatch.setenv("RRTX_OBSMAP_CELLS", str(forced))
        else:
            monkeypatch.delenv("RRTX_OBSMAP_CELLS", raising=False)
        res = on.run(obstacle_list=c, robot_radius=rr, **kw)
        info = res.obstacle_index
        assert info["used"] and info["n_circles"] == m and info["nx"] == (forced or OI.OM.axis_cells(m)), (m, row)
        assert_same_arrays(res, base, (m, row))
        coll = expected_coll(res, c, rr)
        assert coll[0] and OI.first_hit_linear(np.delete(c, row, axis=0), rr, x0, y0).max() == -1, (m, row)
        assert_coll_is(res, base, coll, (m, row, rr, forced))


def test_a_wide_circle_as_the_only_hit_and_a_course_outside_the_box(on20, few):
    on = on20
    kw, base = few
    k = int(base.offsets[1] - 1)                                # the last sample of course 0
    rs = np.random.RandomState(3)
    dots = np.column_stack([rs.uniform(-20, 20, 300) + base.x[k], rs.uniform(-20, 20, 300) + base.y[k], np.full(300, 1e-9)])
    dots[150, :2] = base.x[k] + 0.3, base.y[k] - 0.2
    wide = dots.copy()
    wide[150, 2] = 9.0                                          # over 9 x 9 of the 18 x 18 cells
    away = city(5, 300, 100.0 + abs(base.x).max(), 110.0 + abs(base.x).max(), 0.1, 0.5)     # every course is outside its box
    reach = away.copy()
    reach[299, 2] = float(np.hypot(away[299, 0] - base.x[k], away[299, 1] - base.y[k])) + 0.5
    for name, c, n_wide in (("dots", dots, 0), ("wide", wide, 1), ("away", away, 0), ("reach", reach, 1)):
        res = on.run(obstacle_list=c, robot_radius=0.0, **kw)
        assert res.obstacle_index["used"] and res.obstacle_index["n_wide"] == n_wide, name
        coll = expected_coll(res, c, 0.0)
        assert coll[0] == (n_wide == 1), name
        if name == "wide":
            assert OI.first_hit_linear(np.delete(c, 150, axis=0), 0.0, res.x, res.y).max() == -1     # the only hit
        assert_coll_is(res, base, coll, name)
        assert_same_arrays(res, base, name)


# ---- the index as built, and the batch size -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,rr", [(65, 0.0), (1000, 0.25)])
def test_index_read_back_equals_the_restatement(on20, few, m, rr):
    on = on20
    kw, base = few
    c = city(m, m, -10.0, 30.0, 0.05, 0.4)
    c[m // 2, 2] = 30.0                                                     # one for the wide list
    res = on.run(obstacle_list=c, robot_radius=rr, arrays=False, **kw)
    info = OI.assert_index_equals(on._tracker, c, rr)
    assert info == res.obstacle_index and info["n_wide"] == 1


def test_more_courses_than_resident_waves_against_1000_circles(on):
    g = load("track_kat.npz")
    vecs = kat_vectors(g)
    c = city(77, 1000, -30.0, 40.0, 0.02, 0.08)
    kw = dict(courses=[(v[3], v[4], v[5]) for v in vecs], target_speed=[v[0]["target_speed"] for v in vecs],
              yaw_th=[v[0]["yaw_th"] for v in vecs], invalid_travel_ratio=[v[0]["invalid_travel_ratio"] for v in vecs])
    first = on.run(obstacle_list=c, robot_radius=0.1, **kw)
    assert len(first) == 240 and first.rc == 0
    coll = expected_coll(first, c, 0.1)
    assert np.array_equal((first.fail & F_COLL) != 0, coll) and 20 <= coll.sum() <= 220
    many = csr_inputs(vecs, 18)
    del many["course_obstacles"], many["robot_radius"]
    res = on.run(obstacle_list=c, robot_radius=0.1, arrays=False, **many)
    assert len(res) == 4320 and res.rc == 0 and res.obstacle_index["used"]
    for f in ("find_goal", "length", "fail", "status"):
        assert np.array_equal(getattr(res, f).reshape(18, 240), np.tile(getattr(first, f), (18, 1))), f
    assert np.array_equal(tu.bits(res.t_last).reshape(18, 240), np.tile(tu.bits(first.t_last), (18, 1)))


# ---- the chains -----------------------------------------------------------------------------------------------------------------------
def python_pick(res, indices):
    best_time, win = float("inf"), -1
    for i in indices:
        if res.status[i] == 0 and res.find_goal[i] and best_time >= res.t_last[i]:
            best_time, win = res.t_last[i], i
    return win


def test_steer_chain_on_the_device_equals_the_host_path(on):
    import rrt_amd
    rs = np.random.RandomState(11)
    ns, ng = 6, 8
    starts = np.column_stack([rs.uniform(44, 56, ns), rs.uniform(44, 56, ns), rs.uniform(-np.pi, np.pi, ns)])
    goals = np.column_stack([rs.uniform(44, 56, ng), rs.uniform(44, 56, ng), rs.uniform(-np.pi, np.pi, ng)])
    L = city(12, 1000, 0.0, 100.0, 0.1, 0.5)
    plan = dict(step_size=0.2, product=True, obstacle_list=L, robot_radius=0.1)
    state = np.repeat(np.concatenate([starts, np.zeros((ns, 1))], axis=1), ng, axis=0)
    kw = dict(obstacle_list=L, robot_radius=0.1, yaw_th=0.3)
    with rrt_amd.BatchSteer("rs", obstacle_index=True) as bs:
        host_res = bs.plan(starts, goals, 1.0, **plan)
        rows = np.nonzero(host_res.free)[0]
        assert 4 <= len(rows) < ns * ng
        trip = [(host_res.x[a:b], host_res.y[a:b], host_res.yaw[a:b]) for a, b in zip(host_res.offsets[:-1], host_res.offsets[1:])]
        host = on.run([trip[i] for i in rows], start_state=state[rows], **kw)
        res = bs.plan(starts, goals, 1.0, points="device", **plan)
        assert res.x is None and res.device_courses is not None and res.obstacle_index["used"]
        dev = on.run(res, select="free", group=True, start_state=state, **kw)
    assert dev.obstacle_index["used"] and dev.obstacle_index["n_circles"] == 1000 and host.obstacle_index["used"]
    out = np.setdiff1d(np.arange(ns * ng), rows)
    assert np.all(dev.status[out] == 5) and np.all(np.diff(dev.offsets)[out] == 0)
    for f in ("find_goal", "length", "fail", "status"):
        assert np.array_equal(getattr(dev, f)[rows], getattr(host, f)), f
    assert np.array_equal(tu.bits(dev.t_last[rows]), tu.bits(host.t_last))
    assert np.array_equal(np.diff(dev.offsets)[rows], np.diff(host.offsets)) and dev.steps == host.steps
    for k in ARRAYS:
        assert np.array_equal(tu.bits(getattr(dev, k)), tu.bits(getattr(host, k))), k
    assert np.array_equal((host.fail & F_COLL) != 0, expected_coll(host, L, 0.1))
    assert dev.group == ng and dev.winner.tolist() == [python_pick(dev, range(j * ng, (j + 1) * ng)) for j in range(ns)]


def test_planner_courses_on_the_device_equal_the_host_path(on20):
    from test_gpu_courses import rs_planner
    on = on20
    bp, g = rs_planner([42, 43, 44, 45])
    L = np.concatenate([np.array([tuple(o) for o in g["obstacles"]], dtype=np.float64).reshape(-1, 3),
                        city(13, 1000, -50.0, 70.0, 0.01, 0.05)])
    try:
        bp.plan()
        host_c = bp.courses(order="driving")
        found = np.nonzero(host_c.found)[0]
        assert len(found)
        trip = [tuple(host_c.course(i)[:, k] for k in range(3)) for i in found]
        want = on.run(trip, obstacle_list=L, robot_radius=0.05)
        c = bp.courses(order="driving", arrays="device")
        assert c.x is None and c.device_courses is not None
        dev = on.run(c, select=c.found, obstacle_list=L, robot_radius=0.05)
    finally:
        bp.close()
    assert dev.obstacle_index["used"] and dev.obstacle_index["n_circles"] == len(L) > 1000
    for f in ("find_goal", "length", "fail", "status"):
        assert np.array_equal(getattr(dev, f)[found], getattr(want, f)), f
    assert np.array_equal(tu.bits(dev.t_last[found]), tu.bits(want.t_last)) and dev.steps == want.steps > 0
    for k in ARRAYS:
        assert np.array_equal(tu.bits(getattr(dev, k)), tu.bits(getattr(want, k))), k
    assert np.array_equal((want.fail & F_COLL) != 0, expected_coll(want, L, 0.05))


# ---- the fallbacks and the life of an object ------------------------------------------------------------------------------------------
def test_a_non_finite_threshold_on_a_short_list_gives_the_off_answer(on20, few):
    import rrt_amd
    kw, base = few
    c = np.array([[base.x[5], base.y[5] + 3.0, 0.2], [500.0, 500.0, 1e200], [-40.0, 3.0, 0.5]])     # (1e200) ** 2 = inf: it holds every point
    a = on20.run(obstacle_list=c, robot_radius=0.0, **kw)
    with rrt_amd.BatchTrack(T=20.0) as off20:
        b = off20.run(obstacle_list=c, robot_radius=0.0, **kw)
    assert (a.obstacle_index["used"], a.obstacle_index["reason"], a.obstacle_index["nx"]) == (False, "non-finite reach", 0)
    assert_same_records(a, b)
    assert_same_arrays(a, b)
    assert np.all(a.fail & F_COLL)


def test_a_long_run_on_a_long_list_is_refused_and_the_last_run_stands(gpu, few):
    import rrt_amd
    kw, base = few
    c = city(21, 70, -10.0, 30.0, 0.1, 0.5)
    with rrt_amd.BatchTrack(T=20.0, obstacle_index=True) as bt:
        before = bt.run(obstacle_list=c, robot_radius=0.1, **kw)
        T = bt._tracker
        state = (T.counts(), T.kernel_ms(), T.obstacle_index_info())
        with pytest.raises(rrt_amd._abi.RrtxError, match="run too long"):
            bt.run(obstacle_list=np.tile([[1.0, 2.0, 0.5]], (5000, 1)), robot_radius=0.1, **kw)
        assert (T.counts(), T.kernel_ms(), T.obstacle_index_info()) == state          # nothing was launched
        rec, offs = T.records()
        assert np.array_equal(rec["fail"], before.fail) and np.array_equal(offs, before.offsets)
        for got, k in zip(T.arrays(), ARRAYS):
            assert np.array_equal(tu.bits(got), tu.bits(getattr(before, k))), k
        OI.assert_index_equals(T, c, 0.1)                                              # the index of the last run, too
        again = bt.run(obstacle_list=c, robot_radius=0.1, **kw)                        # and the tracker goes on
        assert_same_records(again, before)


def test_nothing_goes_stale_over_the_life_of_a_tracker(gpu, few):
    import rrt_amd
    kw, base = few
    a, b = city(31, 65, -10.0, 30.0, 0.2, 0.8), city(32, 400, -10.0, 30.0, 0.1, 0.4)
    with rrt_amd.BatchTrack(T=20.0, obstacle_index=True) as bt:
        def run(c, rr):
            res = bt.run(obstacle_list=c, robot_radius=rr, **kw)
            assert np.array_equal((res.fail & F_COLL) != 0, expected_coll(res, c, rr))
            return res
        r1 = run(a, 0.1)
        assert r1.obstacle_index["used"] and r1.obstacle_index["n_circles"] == 65
        OI.assert_index_equals(bt._tracker, a, 0.1)
        r2 = run(b, 0.1)                                                        # a changed list: built again
        assert r2.obstacle_index["n_circles"] == 400
        OI.assert_index_equals(bt._tracker, b, 0.1)
        run(b, 0.5)                                                             # the same list, another radius
        built = OI.assert_index_equals(bt._tracker, b, 0.5)["build_ms"]
        assert run(b, 0.5).obstacle_index["build_ms"] == built                  # equal rows and radius: the build is kept
        bt.obstacle_index = False
        with pytest.raises(rrt_amd._abi.RrtxError, match="more than 64 obstacles in one list"):
            bt.run(obstacle_list=a, robot_radius=0.1, **kw)                     # OFF refuses 65 rows as ever
        r3 = bt.run(obstacle_list=a[:64], robot_radius=0.1, **kw)
        assert (r3.obstacle_index["used"], r3.obstacle_index["reason"]) == (False, "off")
        bt.obstacle_index = True
        r4 = run(a[:64], 0.1)
        assert r4.obstacle_index["used"]
        assert_same_records(r4, r3)
        assert bt.run(**kw).obstacle_index is None                              # no list: nothing is tested
        assert bt._tracker.obstacle_index_info()["reason"] == "empty"

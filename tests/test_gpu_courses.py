"""BatchPlanner.courses(): every planned course of a batch from one gather on the device (rrtx_gather_courses).  The
yardstick is the per-instance API the goldens pin -- path(i), get_path_yaw, smooth() -- and, for the chain into the
tracker, BatchTrack.run on host triples: the gather copies doubles and computes none, so everything is compared bit for bit."""

import numpy as np
import pytest

import util
import track_util as tu

pytestmark = pytest.mark.gpu
E_STATE = -5
REC_FIELDS = ("find_goal", "length", "fail", "status")
ARRAYS = ("x", "y", "yaw", "v", "t", "a", "d")
LQR_OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
BIT_OBS = [(5, 5, 0.5), (9, 6, 1), (7, 5, 1), (1, 5, 1), (3, 6, 1), (7, 9, 1)]


def rs_planner(seeds, **over):
    import rrt_amd
    g = util.load_golden(util.GOLDEN + "/rrt06_drv_s42_it200.npz")
    kw = dict(expand_dis=3.0, goal_sample_rate=10, max_iter=200, robot_radius=0.6, search_until_max_iter=True, curvature=2.0,
              step_size=0.1)
    kw.update(over)
    bp = rrt_amd.BatchPlanner("rrt_star_reeds_shepp", seeds, list(g["start"]), list(g["goal"]),
                              [tuple(o) for o in g["obstacles"]], list(g["rand_area"]), **kw)
    return bp, g


def per_instance(bp):
    """The courses through the per-instance getters: path(i) is np.column_stack([get_path, get_path_yaw]) for rrt_06."""
    return [bp.path(i) for i in range(len(bp.seeds))]


def assert_courses_equal(c, ref, what=""):
    assert len(c) == len(ref) and c.offsets[0] == 0 and c.offsets[-1] == len(c.x) == len(c.y), what
    assert c.found.tolist() == [p is not None for p in ref], what
    for i, p in enumerate(ref):
        got = c.course(i)
        if p is None:
            assert got is None and c.n_points[i] == 0 and c.offsets[i] == c.offsets[i + 1], (what, i)   # owns no points
        else:
            assert got.shape == p.shape and np.array_equal(tu.bits(got), tu.bits(p)), (what, i)


def check_rs_batch(bp, g, golden_scene=True):
    bp.plan()
    assert not bp.partial
    ref = per_instance(bp)
    c = bp.courses()
    assert c.yaw is not None and len(c.yaw) == len(c.x) and c.order == "planning" and c.kernel_ms > 0.0
    assert c.found.any()
    assert_courses_equal(c, ref, "planning")
    d = bp.courses(order="driving")
    assert np.array_equal(d.offsets, c.offsets)
    assert_courses_equal(d, [None if p is None else p[::-1] for p in ref], "driving")
    if golden_scene:                                         # 200 iterations: the golden's run, and a batch of both kinds
        assert not c.found.all()
        assert c.found[0] and np.array_equal(c.course(0), g["path"])
        assert d.yaw[:c.n_points[0]].tolist() == g["path"][::-1, 2].tolist()
    o, x, y = c.as_csr()
    assert o is c.offsets and x is c.x and y is c.y


def test_rrt06_courses_equal_the_per_instance_getters():
    bp, g = rs_planner([42, 43, 44, 45])
    try:
        check_rs_batch(bp, g)
    finally:
        bp.close()


@pytest.mark.parametrize("ppn,max_iter", [(2, 200), (1, 400)])
def test_rrt06_courses_of_replanned_instances_come_from_the_enlarged_pools(monkeypatch, ppn, max_iter):
    """The pool holds ppn points per node of capacity + 8192: at 2 and 200 iterations (the setting of
    test_gpu_polyline_pool_overflow_is_replanned_with_a_larger_pool) these four seeds still fit, at 1 and 400 iterations
    some do not, are planned again in the enlarged pool, and their courses are read from there."""
    monkeypatch.setenv("RRTX_POOL_POINTS_PER_NODE", str(ppn))
    bp, g = rs_planner([42, 43, 44, 45], max_iter=max_iter)
    try:
        check_rs_batch(bp, g, golden_scene=max_iter == 200)
        if max_iter == 400:
            assert 0 < bp.stats()["replanned"] < 4 * 2       # some instances moved (each at most twice), not all of them
    finally:
        bp.close()


def test_rrt05_courses_have_no_yaw():
    import rrt_amd
    g = util.load_golden(util.GOLDEN + "/rrt05_drv_s42_it500.npz")
    bp = rrt_amd.BatchPlanner("rrt_star_dubins", [42, 43, 44, 45], list(g["start"]), list(g["goal"]),
                              [tuple(o) for o in g["obstacles"]], list(g["rand_area"]), goal_sample_rate=10, max_iter=500,
                              search_until_max_iter=True, curvature=1.0)
    try:
        bp.plan()
        ref = per_instance(bp)
        for order in ("planning", "driving"):
            c = bp.courses(order=order)
            assert c.yaw is None and c.found.any()
            assert_courses_equal(c, [p if p is None or order == "planning" else p[::-1] for p in ref], order)
        with pytest.raises(ValueError, match="no yaw"):
            bp.courses(order="driving", arrays="device")
    finally:
        bp.close()


def point_planner(algo):
    """A small batch on the scene and iteration count of the planner's GPU parity test; the last instance's goal lies
    inside an obstacle (no path), and for rrt_star one instance starts on its goal (the two coinciding rows)."""
    import rrt_amd
    n = 6
    seeds = list(range(101, 101 + n))
    kw = dict(seeds=seeds)
    if algo in ("rrt", "rrt_star"):
        c2 = util.c2_kwargs(1500)
        ox, oy, _ = c2["obstacles"][0]
        starts, goals = [list(c2["start"]) for _ in seeds], [list(c2["goal"]) for _ in seeds]
        goals[-1] = [float(ox), float(oy)]
        if algo == "rrt_star":
            starts[2], goals[2] = [0.0, 0.0], [0.0, 0.0]
        kw.update(start=c2["start"], goal=c2["goal"], obstacle_list=c2["obstacles"], rand_area=c2["rand_area"], expand_dis=2.0,
                  path_resolution=0.25, goal_sample_rate=5, max_iter=1500, search_until_max_iter=algo == "rrt_star",
                  starts=starts, goals=goals)
    elif algo == "informed":
        k7 = util.informed_kwargs_from_golden(util.load_golden(util.GOLDEN + "/rrt07_drv_mt_s42_it2000.npz"))
        goals = [list(k7["goal"]) for _ in seeds]
        goals[-1] = [float(k7["obstacles"][0][0]), float(k7["obstacles"][0][1])]
        kw.update(start=k7["start"], goal=k7["goal"], obstacle_list=k7["obstacles"], rand_area=k7["rand_area"], expand_dis=0.5,
                  goal_sample_rate=10, max_iter=600, goals=goals)
    elif algo == "bitstar":
        goals = [[3.0, 8.0] for _ in seeds]
        goals[-1] = [9.0, 6.0]
        kw.update(start=[-1.0, 0.0], goal=[3.0, 8.0], obstacle_list=BIT_OBS, rand_area=[-2.0, 15.0], max_iter=80, goals=goals)
    else:
        goals = [[6.0, 10.0] for _ in seeds]
        goals[-1] = [3.0, 8.0]
        kw.update(seeds=list(range(1, n + 1)),           # the rrt_09 driver's scene: its goldens' seeds 1 and 2 find paths
                  start=[0.0, 0.0], goal=[6.0, 10.0], obstacle_list=LQR_OBS, rand_area=[-2, 15], expand_dis=3.0,
                  goal_sample_rate=10, max_iter=500, sobol_sampler=True, goal_xy_th=0.5, step_size=0.2,
                  search_until_max_iter=True, goals=goals)
    return rrt_amd.BatchPlanner(algo, **kw)


@pytest.mark.parametrize("algo", ["rrt", "rrt_star", "informed", "bitstar", "lqr_rrt_star"])
def test_point_planner_courses(algo):
    bp = point_planner(algo)
    try:
        bp.plan()
        ref = per_instance(bp)
        assert ref[-1] is None and any(p is not None for p in ref)
        if algo == "rrt_star":
            assert ref[2].tolist() == [[0.0, 0.0], [0.0, 0.0]]           # the shortest course there is
        c = bp.courses()
        assert c.yaw is None
        assert_courses_equal(c, ref, algo)
        assert_courses_equal(bp.courses(order="driving"), [None if p is None else p[::-1] for p in ref], algo + " driving")
    finally:
        bp.close()


def test_smoothed_courses_and_untouched_random_streams():
    made = [point_planner("rrt") for _ in range(2)]      # rrt_star's coinciding pair is where the reference's smoothing raises
    try:
        a, b = made
        for bp in made:
            bp.plan()
        a.courses()                                   # gathers before, between and after: none of them draws a number
        sm_a = a.smooth(100)
        c = a.courses("smoothed")
        d = a.courses("smoothed", order="driving")
        b.handles[0].smooth_planned(100)              # the run that never gathers: the per-instance getter
        sm_b = [b.handles[0].get_smoothed_path(i) for i in range(len(b.seeds))]
        assert [p is None for p in sm_a] == [p is None for p in sm_b] and any(p is not None for p in sm_a)
        for i, (pa, pb) in enumerate(zip(sm_a, sm_b)):
            assert pa is None or np.array_equal(tu.bits(pa), tu.bits(pb)), i
        assert_courses_equal(c, sm_a, "smoothed")
        assert_courses_equal(d, [None if p is None else p[::-1] for p in sm_a], "smoothed driving")
        for i in range(len(a.seeds)):
            assert a.rng_state(i) == b.rng_state(i), i
    finally:
        for bp in made:
            bp.close()


def test_state_rules_and_generation():
    import rrt_amd
    bp, _ = rs_planner([42, 43, 44, 45])
    h = bp.handles[0]
    L = h.L
    try:
        with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
            bp.courses()                               # no completed plan
        bp.plan()
        with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
            bp.courses("smoothed")                     # no smoothing run (and rrt_06 has none)
        assert h.generation() == 0
        dev = bp.courses(order="driving", arrays="device")
        assert h.generation() == 1 and dev.x is None and dev.device_courses.generation == 1
        bp.courses()
        assert h.generation() == 2
        n = len(bp.courses().x)
        assert h.generation() == 3
        assert L.rrtx_get_courses(h._h, None, None, None, n - 1) == -4           # RRTX_E_CAPACITY
        assert L.rrtx_get_courses(h._h, None, None, None, n) == 0
        for hh in bp.handles:
            hh.seed_instances([52, 53, 54, 55])
        bp.plan()                                      # other seeds: the gathered courses are the previous plan's
        assert L.rrtx_get_course_counts(h._h, None, None, None, None) == E_STATE
        assert L.rrtx_get_courses(h._h, None, None, None, 1 << 28) == E_STATE
        assert h.generation() == 3
        with rrt_amd.BatchTrack(T=20.0) as bt:
            with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
                bt.run(dev, select=dev.found)          # device-resident courses from before the re-plan
            fresh = bp.courses(order="driving", arrays="device")
            assert h.generation() == 4 and L.rrtx_get_course_counts(h._h, None, None, None, None) == 0
            with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
                bt.run(dev, select=dev.found)          # still the old generation
            assert len(bt.run(fresh, select=fresh.found, arrays=False)) == 4
    finally:
        bp.close()


def test_sharded_planner_equals_one_handle():
    seeds = list(range(42, 49))
    one, _ = rs_planner(seeds)
    many, _ = rs_planner(seeds, devices=[0, 0, 0])
    try:
        assert len(many.handles) == 3
        one.plan()
        many.plan()
        for order in ("planning", "driving"):
            a, b = one.courses(order=order), many.courses(order=order)
            assert np.array_equal(a.offsets, b.offsets) and a.found.any()
            for k in ("x", "y", "yaw"):
                assert np.array_equal(tu.bits(getattr(a, k)), tu.bits(getattr(b, k))), (order, k)
        with pytest.raises(ValueError, match="sharded"):
            many.courses(order="driving", arrays="device")
    finally:
        one.close()
        many.close()


def test_chain_into_the_tracker_equals_the_host_path():
    import rrt_amd
    bp, g = rs_planner([42, 43, 44, 45])
    obst = [tuple(o) for o in g["obstacles"]]
    try:
        bp.plan()
        host = bp.courses(order="driving")
        found = np.nonzero(host.found)[0]
        lost = np.nonzero(~host.found)[0]
        assert len(found) and len(lost)
        trip = [tuple(host.course(i)[:, k] for k in range(3)) for i in found]
        with rrt_amd.BatchTrack(T=20.0) as bt:
            want = bt.run(trip, obstacle_list=obst, robot_radius=0.6, arrays=True)
            c = bp.courses(order="driving", arrays="device")
            assert c.x is None and c.y is None and c.yaw is None and c.device_courses.kind == rrt_amd._abi.SRC_PLANNER
            assert np.array_equal(c.found, host.found)
            dev = bt.run(c, select=c.found, obstacle_list=obst, robot_radius=0.6, arrays=True)
            for f in REC_FIELDS:
                assert np.array_equal(getattr(dev, f)[found], getattr(want, f)), f
            assert np.array_equal(tu.bits(dev.t_last[found]), tu.bits(want.t_last))
            assert (dev.status[lost] == 5).all() and dev.rc == want.rc == 0
            assert np.array_equal(np.diff(dev.offsets)[found], np.diff(want.offsets)) and (np.diff(dev.offsets)[lost] == 0).all()
            assert dev.offsets[-1] == want.offsets[-1] and dev.steps == want.steps > 0
            for k in ARRAYS:
                assert np.array_equal(tu.bits(getattr(dev, k)), tu.bits(getattr(want, k))), k
            assert np.array_equal(tu.bits(dev.goals[found]), tu.bits(want.goals))
            # a PlannerCourses with host arrays goes the host path: the found instances cut out by the caller
            cut = rrt_amd.PlannerCourses(np.concatenate([[0], np.cumsum(host.n_points[found])]),
                                         *[np.concatenate([host.course(i)[:, k] for i in found]) for k in range(3)], "driving")
            again = bt.run(cut, obstacle_list=obst, robot_radius=0.6)
            assert np.array_equal(again.offsets, want.offsets) and np.array_equal(tu.bits(again.x), tu.bits(want.x))
            allc = bt.run(c, obstacle_list=obst, robot_radius=0.6, arrays=True)      # without select
            assert (allc.status[lost] == 2).all() and allc.rc == 1
            assert np.array_equal(allc.status[found], want.status)
            for k in ARRAYS:
                assert np.array_equal(tu.bits(getattr(allc, k)), tu.bits(getattr(want, k))), k
            with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
                bt.run(c, select="free", obstacle_list=obst)                         # a planner's courses carry no hits
            # the native call refuses what BatchPlanner.courses(arrays="device") refuses in Python
            bp.courses(order="planning")
            stale = rrt_amd.PlannerCourses(host.offsets, None, None, None, "driving", 0.0,
                                           rrt_amd._abi.DeviceCourses(rrt_amd._abi.SRC_PLANNER, bp.handles[0]))
            with pytest.raises(rrt_amd._abi.RrtxError, match="planning order"):
                bt.run(stale, select=host.found)
        with pytest.raises(ValueError, match="order='driving'"):
            bp.courses(arrays="device")
    finally:
        bp.close()
    g5 = util.load_golden(util.GOLDEN + "/rrt05_drv_s42_it500.npz")
    b5 = rrt_amd.BatchPlanner("rrt_star_dubins", [42, 43], list(g5["start"]), list(g5["goal"]),
                              [tuple(o) for o in g5["obstacles"]], list(g5["rand_area"]), goal_sample_rate=10, max_iter=500,
                              search_until_max_iter=True, curvature=1.0)
    try:
        b5.plan()
        with pytest.raises(ValueError, match="no yaw"):
            b5.courses(order="driving", arrays="device")
        c5 = b5.courses(order="driving")
        forged = rrt_amd.PlannerCourses(c5.offsets, None, None, None, "driving", 0.0,
                                        rrt_amd._abi.DeviceCourses(rrt_amd._abi.SRC_PLANNER, b5.handles[0]))
        with rrt_amd.BatchTrack(T=20.0) as bt, pytest.raises(rrt_amd._abi.RrtxError, match="no yaw"):
            bt.run(forged, select=c5.found)
    finally:
        b5.close()

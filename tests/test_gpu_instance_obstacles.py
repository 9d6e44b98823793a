"""GPU (-m gpu): per-instance obstacle maps (rrtx_set_instance_obstacles, BatchPlanner(instance_obstacles=...)).

Instance i with its own list must plan exactly what the oracle plans for that list and seed, on every planner and every
kernel shape.  Lists are ordered so that an empty or sparse map comes right before a dense one: a kernel that loops to the
batch's largest count would read its neighbour's circles and leave the oracle's tree.  The shared list set through
set_instance_obstacles for every instance plans what set_obstacles plans, decision counters included."""
import numpy as np
import pytest

import util
from test_gpu_grid_index import DECISIONS

pytestmark = pytest.mark.gpu


def _scaled_map(map_seed, m, lo, hi, rmax=2.5):
    """util.synth_map moved from [0, 100]^2 into [lo, hi]^2."""
    s = (hi - lo) / 100.0
    return [(lo + x * s, lo + y * s, r * s) for x, y, r in util.synth_map(map_seed, m, rmax=rmax)]


def _rng_equal(state, mt):
    return tuple(state[1][:624]) == tuple(mt.mt) and state[1][624] == mt.pos


def _batch(algo, seeds, lists, **kw):
    import rrt_amd
    bp = rrt_amd.BatchPlanner(algo, seeds, kw.pop("start"), kw.pop("goal"), None, kw.pop("rand_area"),
                              instance_obstacles=lists, **kw)
    try:
        bp.plan()
    except Exception:
        bp.close()
        raise
    return bp


def _tree_path_rng_equal(bp, i, r, what):
    util.assert_tree_equal(bp.tree(i), (r["x"], r["y"], r["cost"], r["parent"]), what)
    p = bp.path(i)
    assert (p is None) == (r["path"] is None), what
    if p is not None:
        assert np.array_equal(p if p.shape[1] == 2 else p[:, :2], r["path"]), what
    assert _rng_equal(bp.rng_state(i), r["rng"]), what


def _c2_lists(limit):
    """Counts 0 / small / the shape's tile limit, sparse right before dense."""
    counts = [0, limit, 3, limit, 0, 20]
    return [util.synth_map(map_seed=i, m=c) for i, c in enumerate(counts)]


@pytest.mark.parametrize("shape,limit", [("64", 56), ("128", 64), ("256", 256), ("v1", 256)])
def test_gpu_rrt_star_instance_maps_equal_oracle(gpu, monkeypatch, shape, limit):
    """rrt_04 on each iteration-kernel shape and on the general kernel, about 1 500 iterations of C2."""
    if shape == "v1":
        monkeypatch.setenv("RRTX_KERNEL", "v1")
    else:
        monkeypatch.setenv("RRTX_TPB", shape)
    kw = util.c2_kwargs(1500)
    lists = _c2_lists(limit)
    seeds = [11, 12, 13, 14, 15, 16]
    bp = _batch("rrt_star", seeds, lists, start=kw["start"], goal=kw["goal"], rand_area=kw["rand_area"],
                expand_dis=kw["expand_dis"], path_resolution=kw["path_resolution"], max_iter=1500,
                search_until_max_iter=True)
    try:
        if shape != "v1":
            assert bp.stats()["main_shape"] == int(shape)
        for i, s in enumerate(seeds):
            k2 = dict(kw, obstacles=lists[i])
            _tree_path_rng_equal(bp, i, util.run_oracle(k2, s), "rrt_04 %s instance %d" % (shape, i))
    finally:
        bp.close()


@pytest.mark.parametrize("name", ["rrt01_drv_s42", "rrt02_drv_s42"])
def test_gpu_rrt_instance_maps_equal_oracle(gpu, name):
    """rrt_01 (MT) and rrt_02 (Sobol) with the goldens' configuration, one map per instance."""
    g = util.load_golden(util.GOLDEN + "/%s.npz" % name)
    kw = util.kwargs_from_golden(g)
    lo, hi = kw["rand_area"]
    lists = [[], list(kw["obstacles"]), [], _scaled_map(1, 40, lo, hi, rmax=1.5), kw["obstacles"][:2]]
    seeds = [42, 1, 2, 3, 4]
    bp = _batch("rrt", seeds, lists, start=kw["start"], goal=kw["goal"], rand_area=kw["rand_area"],
                expand_dis=kw["expand_dis"], path_resolution=kw["path_resolution"],
                goal_sample_rate=kw["goal_sample_rate"], max_iter=kw["max_iter"], play_area=kw["play_area"],
                robot_radius=kw["robot_radius"], sobol_sampler=bool(kw["sobol"]),
                connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=bool(kw["search_until_max_iter"]))
    try:
        for i, s in enumerate(seeds):
            _tree_path_rng_equal(bp, i, util.run_oracle(dict(kw, obstacles=lists[i]), s), "%s instance %d" % (name, i))
    finally:
        bp.close()


def test_gpu_informed_instance_maps_equal_oracle(gpu):
    """rrt_07, a 200-circle map between an empty one and the golden's."""
    import glob
    import os
    import oracle
    g = util.load_golden(sorted(glob.glob(os.path.join(util.GOLDEN, "rrt07*.npz")))[0])
    kw = util.informed_kwargs_from_golden(g)
    lo, hi = kw["rand_area"]
    lists = [[], _scaled_map(5, 200, lo, hi, rmax=0.8), list(kw["obstacles"]), []]
    seeds = [3, 4, 5, 6]
    bp = _batch("informed", seeds, lists, start=kw["start"], goal=kw["goal"], rand_area=kw["rand_area"],
                expand_dis=kw["expand_dis"], goal_sample_rate=kw["goal_sample_rate"], max_iter=kw["max_iter"],
                sobol_sampler=bool(kw["sobol"]))
    try:
        for i, s in enumerate(seeds):
            r = oracle.plan_informed(seed=s, **dict(kw, obstacles=lists[i]))
            _tree_path_rng_equal(bp, i, r, "rrt_07 instance %d" % i)
    finally:
        bp.close()


@pytest.mark.parametrize("algo", ["rrt_star_dubins", "rrt_dubins"])
def test_gpu_dubins_instance_maps_equal_oracle(gpu, algo):
    """rrt_05 and rrt_03: trees, yaws, polylines and paths per instance map."""
    import oracle
    g = util.load_golden(util.GOLDEN + "/rrt05_drv_s42_it150.npz")
    obst = [tuple(float(v) for v in o) for o in g["obstacles"]]
    ra = [float(v) for v in g["rand_area"]]
    lists = [[], obst, [], _scaled_map(2, 30, ra[0], ra[1], rmax=1.5), obst[:1]]
    seeds = [42, 3, 4, 5, 6]
    bp = _batch(algo, seeds, lists, start=list(g["start"]), goal=list(g["goal"]), rand_area=ra, goal_sample_rate=10,
                max_iter=300, search_until_max_iter=True, curvature=1.0)
    plan = oracle.plan_dubins if algo == "rrt_star_dubins" else oracle.plan_rrt_dubins
    try:
        for i, s in enumerate(seeds):
            r = plan(list(g["start"]), list(g["goal"]), lists[i], ra, 300, seed=s)
            _tree_path_rng_equal(bp, i, r, "%s instance %d" % (algo, i))
            assert np.array_equal(bp.yaw(i), r["yaw"])
            assert np.array_equal(bp.polylines(i)[1], r["poly_x"])
    finally:
        bp.close()


def test_gpu_reeds_shepp_instance_maps_equal_oracle(gpu):
    """rrt_06 with up to 64 circles per instance."""
    import oracle
    g6 = util.load_golden(util.GOLDEN + "/rrt06_drv_s42_it200.npz")
    obst = [tuple(float(v) for v in o) for o in g6["obstacles"]]
    ra = [float(v) for v in g6["rand_area"]]
    lists = [[], _scaled_map(3, 64, ra[0], ra[1], rmax=0.8), obst]
    seeds = [42, 8, 9]
    bp = _batch("rrt_star_reeds_shepp", seeds, lists, start=list(g6["start"]), goal=list(g6["goal"]), rand_area=ra,
                expand_dis=3.0, goal_sample_rate=10, max_iter=200, robot_radius=0.6, search_until_max_iter=True,
                curvature=2.0, step_size=0.1)
    try:
        for i, s in enumerate(seeds):
            r = oracle.plan_rrt_rs(list(g6["start"]), list(g6["goal"]), lists[i], ra, 200, seed=s, curvature=2.0,
                                   robot_radius=0.6, step_size=0.1)
            _tree_path_rng_equal(bp, i, r, "rrt_06 instance %d" % i)
            assert np.array_equal(bp.yaw(i), r["yaw"])
            p = bp.path(i)
            if p is not None:
                assert np.array_equal(p[:, 2], r["path_yaw"])
    finally:
        bp.close()


@pytest.mark.parametrize("kernel", ["wave", "lane"])
def test_gpu_bitstar_instance_maps_equal_oracle(gpu, monkeypatch, kernel):
    """rrt_08 on the one-wave kernel and on the one-lane kernel (rpp::BitCfg points at the instance's rows)."""
    import oracle
    if kernel == "lane":
        monkeypatch.setenv("RRTX_BITSTAR", "lane")
    base = [(5, 5, 0.5), (9, 6, 1), (7, 5, 1), (1, 5, 1), (3, 6, 1), (7, 9, 1)]
    lists = [[], base, [], [(6, 6, 3)] + base[:2], base[3:]]
    seeds = [1000, 1001, 1002, 1003, 1004]
    start, goal = [0.0, 0.0], [12.0, 12.0]
    bp = _batch("bitstar", seeds, lists, start=start, goal=goal, rand_area=[-2.0, 15.0], max_iter=80)
    try:
        for i, s in enumerate(seeds):
            r = oracle.plan_bitstar(start, goal, lists[i], [-2, 15], 80, seed=s)
            _, _, cost, _ = bp.tree(i)
            assert np.array_equal(cost, r["g_scores"]), (kernel, i)
            p = bp.path(i)
            assert (p is None and len(r["path"]) == 0) or np.array_equal(p, r["path"]), (kernel, i)
            assert _rng_equal(bp.rng_state(i), r["rng"]), (kernel, i)
    finally:
        bp.close()


def _handle(kw, n):
    import rrt_amd
    A = rrt_amd._abi
    return A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                    kw["goal_sample_rate"], kw["max_iter"], robot_radius=kw["robot_radius"],
                    connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=True, n_instances=n)


def _collect(h, n):
    h.plan(strict=True)
    return dict(stats=h.get_stats(), trees=[h.get_tree(i) for i in range(n)], paths=[h.get_path(i) for i in range(n)])


def test_gpu_same_list_everywhere_equals_set_obstacles(gpu, monkeypatch):
    """set_instance_obstacles with one list for every instance = set_obstacles: trees, paths, decision counters."""
    monkeypatch.setenv("RRTX_TPB", "64")
    kw = util.c2_kwargs(3000)
    seeds = [1, 2, 3, 4]
    outs = []
    for per in (False, True):
        h = _handle(kw, len(seeds))
        try:
            if per:
                h.set_instance_obstacles([kw["obstacles"]] * len(seeds))
            else:
                h.set_obstacles(kw["obstacles"])
            h.seed_instances(seeds)
            outs.append(_collect(h, len(seeds)))
        finally:
            h.close()
    a, b = outs
    for i in range(len(seeds)):
        util.assert_tree_equal(a["trees"][i], b["trees"][i], "instance %d" % i)
        assert np.array_equal(a["paths"][i], b["paths"][i])
    for k in DECISIONS:
        assert a["stats"][k] == b["stats"][k], k


def test_gpu_near_set_overflow_replan_keeps_each_instance_map(gpu, monkeypatch):
    """The overflow scene of the near-set re-plan test on the 64-thread shape: overflowing instances not at index 0, their
    neighbours on other maps.  Re-planned instances restart from the staged state and keep their own list."""
    monkeypatch.setenv("RRTX_TPB", "64")
    kw = dict(util.C2)
    drv = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
    kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15], expand_dis=3.0, path_resolution=0.5, max_iter=700,
              robot_radius=0.8)
    lists = [[(20, 20, 1)], drv, [], drv, [(1, 4, 1), (5, 9, 1)], drv]
    seeds = [1, 2, 3, 4, 5, 6]
    bp = _batch("rrt_star", seeds, lists, start=kw["start"], goal=kw["goal"], rand_area=kw["rand_area"],
                expand_dis=3.0, path_resolution=0.5, max_iter=700, robot_radius=0.8, search_until_max_iter=True)
    try:
        assert not bp.partial
        assert bp.stats()["replanned"] > 0
        for i, s in enumerate(seeds):
            _tree_path_rng_equal(bp, i, util.run_oracle(dict(kw, obstacles=lists[i]), s), "overflow instance %d" % i)
    finally:
        bp.close()


def test_gpu_polyline_pool_retry_keeps_each_instance_map(gpu, monkeypatch):
    """rrt_05 with a pool small enough that instances are re-planned with the x4 / x16 pools."""
    import oracle
    g = util.load_golden(util.GOLDEN + "/rrt05_drv_s42_it500.npz")
    obst = [tuple(float(v) for v in o) for o in g["obstacles"]]
    ra = [float(v) for v in g["rand_area"]]
    monkeypatch.setenv("RRTX_POOL_POINTS_PER_NODE", "4")
    lists = [[], obst, obst[:2], obst]
    seeds = [42, 43, 44, 45]
    bp = _batch("rrt_star_dubins", seeds, lists, start=list(g["start"]), goal=list(g["goal"]), rand_area=ra,
                expand_dis=float(g["expand_dis"]), goal_sample_rate=int(g["goal_sample_rate"]), max_iter=1500,
                robot_radius=float(g["robot_radius"]), connect_circle_dist=float(g["connect_circle_dist"]),
                search_until_max_iter=True, curvature=float(g["curvature"]), goal_yaw_th=float(g["goal_yaw_th"]),
                goal_xy_th=float(g["goal_xy_th"]))
    try:
        assert not bp.partial
        assert bp.stats()["replanned"] > 0
        for i, s in enumerate(seeds):
            r = oracle.plan_dubins(list(g["start"]), list(g["goal"]), lists[i], ra, 1500, seed=s)
            _tree_path_rng_equal(bp, i, r, "pool retry instance %d" % i)
            assert np.array_equal(bp.polylines(i)[1], r["poly_x"])
    finally:
        bp.close()


def test_gpu_bounded_plan_with_instance_maps_equals_one_shot(gpu, monkeypatch):
    """plan_begin / plan_step in bounded launches (RRTX_CHUNK_ITERS) = one plan; set_instance_obstacles is refused while
    a plan is in progress."""
    import rrt_amd
    kw = util.c2_kwargs(1500)
    lists = _c2_lists(56)
    seeds = [21, 22, 23, 24, 25, 26]
    outs = []
    for chunk in (None, "400"):
        if chunk:
            monkeypatch.setenv("RRTX_CHUNK_ITERS", chunk)
        h = _handle(kw, len(seeds))
        try:
            h.set_instance_obstacles(lists)
            h.seed_instances(seeds)
            if chunk:
                h.plan_begin()
                with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
                    h.set_instance_obstacles(lists)
                while h.plan_step()[1] > 0:
                    pass
                outs.append(dict(trees=[h.get_tree(i) for i in range(len(seeds))],
                                 paths=[h.get_path(i) for i in range(len(seeds))]))
            else:
                outs.append(_collect(h, len(seeds)))
        finally:
            h.close()
    for i in range(len(seeds)):
        util.assert_tree_equal(outs[0]["trees"][i], outs[1]["trees"][i], "bounded instance %d" % i)
        assert (outs[0]["paths"][i] is None) == (outs[1]["paths"][i] is None)
        if outs[0]["paths"][i] is not None:
            assert np.array_equal(outs[0]["paths"][i], outs[1]["paths"][i])


def test_gpu_batch_planner_sharded_and_smoothed_per_instance(gpu, tmp_path):
    """devices=[0, 0] = devices=[0]; smooth() continues each instance's stream against its own list; export_npz writes
    the lists."""
    import oracle
    obst = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
    lists = [obst, [], obst[:3], [(6, 2, 1)], obst, [(2, 9, 1.5)]]
    seeds = [1234, 5, 7, 8, 9, 10]
    kw = dict(start=[0, 0], goal=[6.0, 10.0], rand_area=[-2, 15], expand_dis=1.0, path_resolution=0.1,
              goal_sample_rate=5, max_iter=500, play_area=[0, 10, 0, 14], robot_radius=0.6, connect_circle_dist=50.0,
              search_until_max_iter=True)
    one = _batch("rrt_star", seeds, lists, **dict(kw))
    two = _batch("rrt_star", seeds, lists, devices=[0, 0], **dict(kw))
    try:
        for i in range(len(seeds)):
            util.assert_tree_equal(one.tree(i), two.tree(i), "sharded instance %d" % i)
            assert one.rng_state(i) == two.rng_state(i)
        states = [one.rng_state(i) for i in range(len(seeds))]
        paths = [one.path(i) for i in range(len(seeds))]
        sm1, sm2 = one.smooth(300), two.smooth(300)
        for i in range(len(seeds)):
            assert (sm1[i] is None) == (sm2[i] is None)
            if paths[i] is None:
                continue
            rng = oracle.mt_from_pystate(states[i])
            want = oracle.path_smoothing(paths[i], 300, lists[i], rng)
            assert np.array_equal(sm1[i], want) and np.array_equal(sm2[i], want), i
            assert _rng_equal(one.rng_state(i), rng), i
        z = np.load(one.export_npz(str(tmp_path / "t.npz")))
        for k in range(len(seeds)):
            assert np.array_equal(z["obstacles_%d" % k], np.array(lists[k], dtype=np.float64).reshape(-1, 3))
    finally:
        one.close()
        two.close()


def test_gpu_instance_obstacle_refusals_leave_the_handle_usable(gpu):
    import rrt_amd
    A = rrt_amd._abi
    kw = util.c2_kwargs(300)
    h = _handle(kw, 3)
    try:
        h.set_instance_obstacles([[], kw["obstacles"], []])
        h.seed_instances([1, 2, 3])
        ref = _collect(h, 3)
        big = util.synth_map(1, 257)
        with pytest.raises(A.RrtxError, match="instance 2"):
            h.set_instance_obstacles([[], [], big])
        L = h.L
        for offs, what in (([1, 1, 1, 1], "instance 0"), ([0, 2, 1, 1], "instance 1")):
            o = np.array(offs, dtype=np.int32)
            rows = np.zeros((3, 3))
            assert L.rrtx_set_instance_obstacles(h._h, o.ctypes.data, rows.ctypes.data) == -1
            assert what in L.rrtx_last_error(h._h).decode()
        o = np.array([0, 0, 2, 2], dtype=np.int32)
        assert L.rrtx_set_instance_obstacles(h._h, o.ctypes.data, None) == -1
        again = _collect(h, 3)
        for i in range(3):
            util.assert_tree_equal(again["trees"][i], ref["trees"][i], "after refusals, instance %d" % i)
    finally:
        h.close()
    g6 = util.load_golden(util.GOLDEN + "/rrt06_drv_s42_it200.npz")
    ra = [float(v) for v in g6["rand_area"]]
    h = A.Handle(A.ALGO_RS, list(g6["start"]), list(g6["goal"]), ra, 3.0, 0.5, 10, 50, robot_radius=0.6,
                 search_until_max_iter=True, n_instances=2, curvature=2.0, step_size=0.1)
    try:
        with pytest.raises(A.RrtxError, match="instance 1"):
            h.set_instance_obstacles([[], _scaled_map(3, 65, ra[0], ra[1], rmax=0.5)])
        h.set_instance_obstacles([[], _scaled_map(3, 64, ra[0], ra[1], rmax=0.5)])
        h.seed_instances([1, 2])
        h.plan(strict=True)
    finally:
        h.close()


def test_gpu_shared_list_export_has_no_obstacle_keys_and_smoothing_follows_current_lists(gpu, tmp_path):
    """export_npz keeps the keys of a shared-list batch; smooth() after new lists were set (no re-plan) smooths each
    planned path against the lists set now, as it does for a shared list."""
    import oracle
    import rrt_amd
    obst = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
    seeds = [1234, 5, 7]
    kw = dict(expand_dis=1.0, path_resolution=0.1, goal_sample_rate=5, max_iter=500, play_area=[0, 10, 0, 14],
              robot_radius=0.6, connect_circle_dist=50.0, search_until_max_iter=True)
    bp = rrt_amd.BatchPlanner("rrt_star", seeds, [0, 0], [6.0, 10.0], obst, [-2, 15], **kw)
    try:
        bp.plan()
        z = np.load(bp.export_npz(str(tmp_path / "shared.npz")))
        assert not [k for k in z.files if k.startswith("obstacles")]
        states = [bp.rng_state(i) for i in range(3)]
        paths = [bp.path(i) for i in range(3)]
        later = [[(6, 2, 1)], obst[:2], []]
        bp.h.set_instance_obstacles(later)
        sm = bp.smooth(200)
        for i in range(3):
            if paths[i] is None:
                continue
            want = oracle.path_smoothing(paths[i], 200, later[i], oracle.mt_from_pystate(states[i]))
            assert np.array_equal(sm[i], want), i
    finally:
        bp.close()

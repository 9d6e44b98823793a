"""LQR-RRT* (rrt_09) on the GPU: the drop-in class and module against the reference's goldens, batches against the
pure-Python oracle (tests/lqr_oracle.py), per-instance maps, sharding over handles and bounded launches."""
import glob
import json
import os
import random

import numpy as np
import pytest

import util
import lqr_oracle

pytestmark = pytest.mark.gpu
GOLD = os.path.join(util.ROOT, "tests", "golden")
DRV_OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]


def rrt09_goldens():
    return sorted(glob.glob(os.path.join(GOLD, "rrt09_*.npz")))


def ctor_kwargs(g):
    kw = json.loads(str(g["kwargs"]))
    kw["obstacle_list"] = [tuple(o) for o in kw["obstacle_list"]]
    return kw


def oracle_plan(kw, seed, until_max=True):
    o = lqr_oracle.LQROracle(**kw)
    rng = random.Random()
    rng.seed(seed)
    p = o.planning(rng, until_max)
    return o, p, rng


@pytest.mark.parametrize("path", rrt09_goldens(), ids=lambda p: os.path.basename(p)[:-4])
@pytest.mark.parametrize("module", ["planner", "rrt_09"])
def test_golden_plan_bit_identical(path, module):
    import rrt_amd
    import rrt_amd.rrt_09 as m09
    g = np.load(path)
    cls, smooth = (rrt_amd.LQRRRTStar, rrt_amd.path_smoothing) if module == "planner" else (m09.LQRRRTStar, m09.path_smoothing)
    kw = ctor_kwargs(g)
    random.seed(int(g["seed"]))
    rrt = cls(**kw)
    path_out = rrt.planning(animation=False, search_until_max_iter=bool(g["until_max"]))
    st = random.getstate()[1]
    assert np.array_equal(np.array(st[:624], dtype=np.uint32), g["mt_after"]) and st[624] == int(g["mt_pos_after"])
    nodes = list(rrt.node_list)
    x = np.array([n.x for n in nodes])
    y = np.array([n.y for n in nodes])
    assert np.array_equal(x.view(np.uint64), g["x"].view(np.uint64))
    assert np.array_equal(y.view(np.uint64), g["y"].view(np.uint64))
    assert np.array_equal(np.array([n.cost for n in nodes]).view(np.uint64), g["cost"].view(np.uint64))
    idx = {id(n): i for i, n in enumerate(nodes)}
    assert [idx[id(n.parent)] if n.parent is not None else -1 for n in nodes] == list(g["parent"])
    assert [len(n.path_x) for n in nodes] == list(g["plen"])
    assert np.array_equal(np.array([v for n in nodes for v in n.path_x]), g["px"])
    assert np.array_equal(np.array([v for n in nodes for v in n.path_y]), g["py"])
    if kw["sobol_sampler"]:
        assert rrt.sobol_inter_ == int(g["sobol_index"])
    pp = np.zeros((0, 2)) if path_out is None else np.array(path_out)
    assert np.array_equal(pp, g["path"])
    if path_out is not None:
        sp = smooth(path_out, int(g["smooth_iter"]), kw["obstacle_list"])
        assert np.array_equal(np.array(sp), g["smoothed"])
        st = random.getstate()[1]
        assert np.array_equal(np.array(st[:624], dtype=np.uint32), g["mt_after_smooth"])
        assert st[624] == int(g["mt_pos_after_smooth"])


def check_batch_vs_oracle(bp, kw, seeds, starts, goals, until_max):
    pc, nn, status = bp.plan()
    for i, s in enumerate(seeds):
        okw = dict(kw, start=starts[i], goal=goals[i])
        o, p, rng = oracle_plan(okw, s, until_max)
        x, y, cost, parent = bp.tree(i)
        what = "instance %d seed %d" % (i, s)
        assert np.array_equal(x, np.array(o.x, dtype=np.float64)), what
        assert np.array_equal(y, np.array(o.y, dtype=np.float64)), what
        assert np.array_equal(cost, np.array(o.cost, dtype=np.float64)), what
        assert np.array_equal(parent, np.array(o.parent)), what
        got = bp.path(i)
        assert (got is None) == (p is None), what
        if p is not None:
            assert np.array_equal(got, np.array(p, dtype=np.float64)), what
            assert pc[i] == lqr_oracle.get_path_length(p), what
        assert bp.rng_state(i)[1] == rng.getstate()[1], what


def batch_kwargs(**over):
    kw = dict(obstacle_list=DRV_OBS, rand_area=[-2, 15], expand_dis=3.0, goal_sample_rate=10, max_iter=150,
              play_area=None, robot_radius=0.0, sobol_sampler=True, connect_circle_dist=50.0, goal_xy_th=0.5,
              step_size=0.2)
    kw.update(over)
    return kw


def mixed_ends(n, seed):
    rs = np.random.RandomState(seed)
    starts = [[float(v) for v in rs.uniform(-1, 2, 2)] for _ in range(n)]
    goals = [[float(a), float(b)] for a, b in zip(rs.uniform(5, 12, n), rs.uniform(8, 13, n))]
    return starts, goals


@pytest.mark.parametrize("sobol", [True, False])
def test_batch_matches_oracle_both_samplers(sobol):
    import rrt_amd
    n = 256
    seeds = list(range(100, 100 + n))
    starts, goals = mixed_ends(n, 3 if sobol else 4)
    kw = batch_kwargs(sobol_sampler=sobol)
    bp = rrt_amd.BatchPlanner("lqr_rrt_star", seeds, starts[0], goals[0], starts=starts, goals=goals,
                              search_until_max_iter=True, **kw)
    try:
        check_batch_vs_oracle(bp, kw, seeds, starts, goals, True)
    finally:
        bp.close()


@pytest.mark.parametrize("over,until_max", [(dict(), False), (dict(play_area=[-1, 12, -1, 13]), True),
                                            (dict(robot_radius=0.3), True), (dict(sobol_sampler=False), False)])
def test_batch_variants_match_oracle(over, until_max):
    import rrt_amd
    n = 48
    seeds = list(range(7, 7 + n))
    starts, goals = mixed_ends(n, 11)
    kw = batch_kwargs(**over)
    bp = rrt_amd.BatchPlanner("lqr_rrt_star", seeds, starts[0], goals[0], starts=starts, goals=goals,
                              search_until_max_iter=until_max, **kw)
    try:
        check_batch_vs_oracle(bp, kw, seeds, starts, goals, until_max)
    finally:
        bp.close()


def test_instance_obstacles_equal_single_map_plans():
    import rrt_amd
    maps = [DRV_OBS, DRV_OBS[:3], [(4, 4, 1.5), (8, 8, 1)], [], util.synth_map(5, 12)]
    seeds = [3, 4, 5, 6, 7]
    kw = batch_kwargs()
    kw.pop("obstacle_list")
    bp = rrt_amd.BatchPlanner("lqr_rrt_star", seeds, [0, 0], [6.0, 10.0], None, instance_obstacles=maps, **kw)
    try:
        bp.plan()
        for i, (s, mp) in enumerate(zip(seeds, maps)):
            one = rrt_amd.BatchPlanner("lqr_rrt_star", [s], [0, 0], [6.0, 10.0], mp, **kw)
            try:
                one.plan()
                for a, b in zip(bp.tree(i), one.tree(0)):
                    assert np.array_equal(a, b), "instance %d" % i
                pa, pb = bp.path(i), one.path(0)
                assert (pa is None) == (pb is None) and (pa is None or np.array_equal(pa, pb))
            finally:
                one.close()
    finally:
        bp.close()


def test_three_handles_equal_one_handle():
    import rrt_amd
    seeds = list(range(20, 44))
    starts, goals = mixed_ends(len(seeds), 5)
    kw = batch_kwargs()
    one = rrt_amd.BatchPlanner("lqr_rrt_star", seeds, starts[0], goals[0], starts=starts, goals=goals, **kw)
    three = rrt_amd.BatchPlanner("lqr_rrt_star", seeds, starts[0], goals[0], starts=starts, goals=goals,
                                 devices=[0, 0, 0], **kw)
    try:
        r1, r3 = one.plan(), three.plan()
        for a, b in zip(r1, r3):
            assert np.array_equal(a, b)
        for i in range(len(seeds)):
            for a, b in zip(one.tree(i), three.tree(i)):
                assert np.array_equal(a, b)
            for a, b in zip(one.polylines(i), three.polylines(i)):
                assert np.array_equal(a, b)
        s1, s3 = one.smooth(200), three.smooth(200)
        for a, b in zip(s1, s3):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    finally:
        one.close()
        three.close()


def test_bounded_odd_steps_equal_one_shot():
    import rrt_amd
    A = rrt_amd._abi
    seeds = list(range(50, 66))

    def make():
        h = A.Handle(A.ALGO_LQR_RRT_STAR, [0, 0], [6.0, 10.0], [-2, 15], 3.0, 0.5, 10, 300, sampler=A.SAMPLER_SOBOL,
                     search_until_max_iter=True, n_instances=len(seeds), goal_xy_th=0.5, step_size=0.2)
        h.set_obstacles(DRV_OBS)
        h.seed_instances(seeds)
        return h
    h1, h2 = make(), make()
    try:
        h1.plan(strict=True)
        h2.set_launch_bound(37)
        h2.plan_begin()
        steps = 0
        while True:
            rc, pending = h2.plan_step()
            steps += 1
            if pending == 0:
                break
            assert steps < 100
        assert steps > 2
        for a, b in zip(h1.get_results(), h2.get_results()):
            assert np.array_equal(a, b)
        for i in range(len(seeds)):
            for a, b in zip(h1.get_tree(i), h2.get_tree(i)):
                assert np.array_equal(a, b)
            assert h1.get_rng_state(i)[1] == h2.get_rng_state(i)[1]
    finally:
        h1.close()
        h2.close()


def test_batch_export_and_smooth():
    import rrt_amd
    seeds = [1, 2]
    kw = batch_kwargs(max_iter=500)
    bp = rrt_amd.BatchPlanner("lqr_rrt_star", seeds, [0, 0], [6.0, 10.0], search_until_max_iter=True, **kw)
    try:
        bp.plan()
        sm = bp.smooth(1000)
        for i, s in enumerate(seeds):
            g = np.load(os.path.join(GOLD, "rrt09_drv_s%d.npz" % s))
            assert np.array_equal(bp.path(i), g["path"])
            assert np.array_equal(sm[i], g["smoothed"])
            st = bp.rng_state(i)[1]
            assert np.array_equal(np.array(st[:624], dtype=np.uint32), g["mt_after_smooth"])
            assert st[624] == int(g["mt_pos_after_smooth"])
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            f = bp.export_npz(os.path.join(d, "lqr.npz"))
            z = np.load(f)
            assert np.array_equal(z["x_0"], bp.tree(0)[0])
    finally:
        bp.close()

"""Closed-loop RRT* (rrt_10) on the GPU: `ClosedLoopRRTStar` and `rrt_amd.rrt_10` against every rrt10_* golden (tree, RNG
state, candidate list, per-candidate records, the returned 8-tuple: bit for bit), batches against the single-instance class,
shards, per-instance maps and a re-plan on a reused handle.  Which golden covers which branch: tests/track_util.py."""
import os
import random

import numpy as np
import pytest

import track_util as tu

pytestmark = pytest.mark.gpu


def driver_kwargs():
    g, kw, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s0.npz"))
    return kw


def plan_single(mod_cls, kw, seed):
    random.seed(seed)
    obj = mod_cls(**kw)
    out = obj.planning(animation=False)
    return obj, out, random.getstate()


def check_tuple(out, g):
    flag = out[0]
    assert bool(flag) == bool(g["flag"])
    for k, name in enumerate(("out_x", "out_y", "out_yaw", "out_v", "out_t", "out_a", "out_d")):
        if not flag:
            assert out[k + 1] is None
        else:
            assert isinstance(out[k + 1], list)
            assert np.array_equal(tu.bits(out[k + 1]), tu.bits(g[name])), name


@pytest.mark.parametrize("entry", ["class", "module"])
@pytest.mark.parametrize("path", tu.goldens(), ids=lambda p: os.path.basename(p)[:-4])
def test_reproduces_reference_plan(path, entry):
    import rrt_amd
    import rrt_amd.rrt_10
    g, kw, _ = tu.load(path)
    cls = rrt_amd.ClosedLoopRRTStar if entry == "class" else rrt_amd.rrt_10.ClosedLoopRRTStar
    obj, out, st = plan_single(cls, kw, int(g["seed"]))
    x, y, cost, parent = obj.tree
    assert np.array_equal(tu.bits(x), tu.bits(g["x"])) and np.array_equal(tu.bits(y), tu.bits(g["y"]))
    assert np.array_equal(tu.bits(obj.yaw), tu.bits(g["yaw"]))
    assert np.array_equal(tu.bits(cost), tu.bits(g["cost"]))
    assert np.array_equal(np.asarray(parent), g["parent"])
    plen, px, py = obj.polylines
    assert np.array_equal(np.asarray(plen), g["plen"])
    assert np.array_equal(tu.bits(px), tu.bits(g["px"])) and np.array_equal(tu.bits(py), tu.bits(g["py"]))
    assert len(obj.node_list) == len(g["x"])
    assert np.array_equal(np.array(st[1][:624], dtype=np.uint32), g["mt_after"]) and st[1][624] == int(g["mt_pos_after"])
    assert obj.get_goal_indexes() == g["cand"].tolist()
    rec = obj.records
    assert rec["find_goal"].tolist() == g["cand_find"].tolist()
    assert rec["len"].tolist() == g["cand_len"].tolist()
    assert rec["fail"].tolist() == g["cand_fail"].tolist()
    assert np.array_equal(tu.bits(rec["t_last"]), tu.bits(g["cand_tlast"]))
    check_tuple(out, g)


def batch(seeds, kw, **extra):
    import rrt_amd
    args = dict(seeds=seeds, start=kw["start"], goal=kw["goal"], obstacle_list=kw["obstacle_list"], rand_area=kw["rand_area"],
                max_iter=kw["max_iter"], connect_circle_dist=kw["connect_circle_dist"], robot_radius=kw["robot_radius"])
    args.update(extra)
    return rrt_amd.BatchPlanner("closed_loop_rrt_star", **args)


def track_kw(kw):
    return {k: kw[k] for k in tu.PORDER[:4]}


def same_result(bp, i, ref):
    obj, out = ref
    assert np.array_equal(tu.bits(bp.tree(i)[0]), tu.bits(obj.tree[0])) and np.array_equal(tu.bits(bp.tree(i)[2]), tu.bits(obj.tree[2]))
    cand, rec = bp.track_records(i)
    assert cand.tolist() == obj.get_goal_indexes() and rec.tobytes() == obj.records.tobytes()
    tr = bp.trajectory(i)
    assert (tr is not None) == bool(out[0])
    if tr is not None:
        for a, b in zip(tr, out[1:]):
            assert np.array_equal(tu.bits(a), tu.bits(b))


def test_batch_of_256_equals_single_instance_class_and_goldens():
    """Every one of the 256 instances against the single-instance class seeded the same way (tree, candidates, full
    records, trajectory); seeds 0..7 are the driver-cell goldens and are compared with those as well, full records."""
    import rrt_amd
    kw = driver_kwargs()
    seeds = list(range(256))
    bp = batch(seeds, kw)
    try:
        bp.plan()
        flags = bp.track(**track_kw(kw))
        for s in range(8):
            g, _, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s%d.npz" % s))
            assert bool(flags[s]) == bool(g["flag"])
            cand, rec = bp.track_records(s)
            assert cand.tolist() == g["cand"].tolist()
            assert rec["find_goal"].tolist() == g["cand_find"].tolist() and rec["len"].tolist() == g["cand_len"].tolist()
            assert rec["fail"].tolist() == g["cand_fail"].tolist()
            assert np.array_equal(tu.bits(rec["t_last"]), tu.bits(g["cand_tlast"]))
            for a, name in zip(bp.trajectory(s), ("out_x", "out_y", "out_yaw", "out_v", "out_t", "out_a", "out_d")):
                assert np.array_equal(tu.bits(a), tu.bits(g[name])), (s, name)
        for s in seeds:
            obj, out, _ = plan_single(rrt_amd.ClosedLoopRRTStar, kw, s)
            assert bool(flags[s]) == bool(out[0]), s
            same_result(bp, s, (obj, out))
    finally:
        bp.close()


def test_track_refuses_other_planners_and_export_has_trajectory_keys(tmp_path):
    import rrt_amd
    kw = driver_kwargs()
    other = rrt_amd.BatchPlanner("rrt_star_reeds_shepp", seeds=[1], start=kw["start"], goal=kw["goal"],
                                 obstacle_list=kw["obstacle_list"], rand_area=kw["rand_area"], max_iter=20)
    try:
        other.plan()
        with pytest.raises(ValueError):
            other.track()
        f = other.export_npz(str(tmp_path / "rs.npz"))
        assert not [k for k in np.load(f).files if k.startswith("track_")]      # this algorithm's keys only
    finally:
        other.close()
    kw["max_iter"] = 100
    bp = batch([11, 9], kw)
    try:
        bp.plan()
        f = bp.export_npz(str(tmp_path / "untracked.npz"))
        assert not [k for k in np.load(f).files if k.startswith("track_")]      # nothing before track()
        bp.track(**track_kw(kw))
        z = np.load(bp.export_npz(str(tmp_path / "tracked.npz")))
        g, _, _ = tu.load(os.path.join(tu.GOLD, "rrt10_map_a_s11.npz"))        # seed 11, max_iter 100
        assert bool(z["track_flag_0"]) == bool(g["flag"])
        for name in ("x", "y", "yaw", "v", "t", "a", "d"):
            assert np.array_equal(tu.bits(z["track_%s_0" % name]), tu.bits(g["out_" + name])), name
            assert "track_%s_1" % name in z.files
    finally:
        bp.close()


def test_sharded_batch_equals_unsharded():
    import rrt_amd
    kw = driver_kwargs()
    kw["max_iter"] = 80
    seeds = list(range(20, 32))
    ndev = rrt_amd._abi.load().rrtx_device_count()
    devices = [0, 1] if ndev > 1 else [0, 0]
    a, b = batch(seeds, kw), batch(seeds, kw, devices=devices)
    try:
        a.plan(); b.plan()
        fa, fb = a.track(**track_kw(kw)), b.track(**track_kw(kw))
        assert fa.tolist() == fb.tolist()
        for i in range(len(seeds)):
            ca, ra = a.track_records(i)
            cb, rb = b.track_records(i)
            assert ca.tolist() == cb.tolist() and ra.tobytes() == rb.tobytes()
            ta, tb = a.trajectory(i), b.trajectory(i)
            assert (ta is None) == (tb is None)
            if ta is not None:
                assert all(np.array_equal(tu.bits(p), tu.bits(q)) for p, q in zip(ta, tb))
    finally:
        a.close(); b.close()


def test_per_instance_maps_equal_their_single_map_plans():
    names = ["rrt10_map_a_s11", "rrt10_map_b_s12", "rrt10_coll_s2"]
    gs = [tu.load(os.path.join(tu.GOLD, n + ".npz")) for n in names]
    assert gs[0][1]["max_iter"] == gs[1][1]["max_iter"] and gs[0][1]["robot_radius"] == gs[1][1]["robot_radius"]
    # one robot radius per handle: the collision golden (radius 0.3) is planned in a batch of its own radius
    for grp in ([0, 1], [2]):
        kw = gs[grp[0]][1]
        bp = batch([int(gs[i][0]["seed"]) for i in grp], kw, obstacle_list=None,
                   instance_obstacles=[gs[i][1]["obstacle_list"] for i in grp])
        try:
            bp.plan()
            bp.track(**track_kw(kw))
            for j, i in enumerate(grp):
                g = gs[i][0]
                cand, rec = bp.track_records(j)
                assert cand.tolist() == g["cand"].tolist() and rec["fail"].tolist() == g["cand_fail"].tolist()
                tr = bp.trajectory(j)
                assert (tr is not None) == bool(g["flag"])
                for a, name in zip(tr, ("out_x", "out_y", "out_yaw", "out_v", "out_t", "out_a", "out_d")):
                    assert np.array_equal(tu.bits(a), tu.bits(g[name])), (names[i], name)
        finally:
            bp.close()


def test_track_after_replan_on_the_same_handle():
    import rrt_amd
    kw = driver_kwargs()
    bp = batch([0, 1], kw)
    try:
        bp.plan()
        bp.track(**track_kw(kw))
        first = [bp.trajectory(i) for i in range(2)]
        for h, (lo, hi) in zip(bp.handles, bp.shards):
            h.seed_instances([2, 3][lo:hi])
        bp.plan()
        with pytest.raises(rrt_amd._abi.RrtxError):
            bp.trajectory(0)        # RRTX_E_STATE: the previous plan's trajectories are not this plan's
        bp.track(**track_kw(kw))
        for i, s in enumerate((2, 3)):
            g, _, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s%d.npz" % s))
            for a, name in zip(bp.trajectory(i), ("out_x", "out_y", "out_yaw", "out_v", "out_t", "out_a", "out_d")):
                assert np.array_equal(tu.bits(a), tu.bits(g[name])), (s, name)
        assert not np.array_equal(first[0][0], bp.trajectory(0)[0])
    finally:
        bp.close()


def test_device_tan_and_hypot_replicas():
    import math
    import rrt_amd
    L = rrt_amd._abi.load()
    rs = np.random.RandomState(5)
    n = 200000
    a = rs.uniform(-0.79, 0.79, n)
    b = rs.uniform(-25, 25, n)
    out = np.zeros(n)
    assert L.rrtx_selftest_math(0, 11, a.ctypes.data, b.ctypes.data, out.ctypes.data, n) == 0
    assert np.array_equal(tu.bits(out), tu.bits([math.tan(float(v)) for v in a]))
    c = rs.uniform(-25, 25, n)
    assert L.rrtx_selftest_math(0, 12, c.ctypes.data, b.ctypes.data, out.ctypes.data, n) == 0
    assert np.array_equal(tu.bits(out), tu.bits(np.hypot(c, b)))

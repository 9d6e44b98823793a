"""GPU (-m gpu): the 64-byte line per node (rppk::Node) of the rrt_04 iteration kernel.  During a launch the candidate
gather, the rewire links, the three cost walks and the append work on the records alone; the prologue builds them from
cost[], kid[], parent[], prev_sib[], x[], y[], xq[] and the epilogue writes cost and the links back, so every getter, the
general kernel and a next launch read the arrays as before.  get_tree reads the arrays: every comparison below is also a
test of the write-back.  Scenes and helpers are those of test_gpu_kid_records.py; the shapes are the smallest at which
each path runs."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_kid_records as kid
import util

pytestmark = pytest.mark.gpu

SEEDS = kid.SEEDS


def _env(monkeypatch, tpb="64", **env):
    kid._env(monkeypatch, **env)
    monkeypatch.setenv("RRTX_TPB", tpb)
    if "RRTX_GRID" in env:
        monkeypatch.setenv("RRTX_GRID", env["RRTX_GRID"])
    else:
        monkeypatch.delenv("RRTX_GRID", raising=False)


def _handle(kw, n):
    import rrt_amd
    A = rrt_amd._abi
    h = A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                 kw["goal_sample_rate"], kw["max_iter"], play_area=kw["play_area"], robot_radius=kw["robot_radius"],
                 connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=kw["search_until_max_iter"],
                 n_instances=n)
    h.set_obstacles(kw["obstacles"])
    return h


def _read(h, n):
    return dict(stats=h.get_stats(), results=h.get_results(), trees=[h.get_tree(i) for i in range(n)],
                paths=[h.get_path(i) for i in range(n)])


def test_gpu_node_walks_equal_oracle(gpu, monkeypatch):
    """C2 at 3 000 iterations: the scalar walk alone, the lane walk from the first node, and the lane walk with a pending
    list of 4 chains (the global-stack walk redoes the subtrees that outgrow it) -- all on the records -- each equal the
    oracle: trees, paths, counters."""
    kw = util.c2_kwargs(3000)
    refs = [kid._oracle_c2(3000, s) for s in SEEDS]
    for vec, cap in (("-1", None), ("0", None), ("0", "4")):
        _env(monkeypatch, RRTX_PROP_VEC=vec, RRTX_PROP_CAP=cap, RRTX_GRID_MIN="256")
        out, done, full = kid._plan(kw, SEEDS)
        what = "RRTX_PROP_VEC=%s RRTX_PROP_CAP=%s" % (vec, cap)
        print("%s: %d walks finished by the lanes, %d with a full pending list" % (what, done, full))
        assert out["stats"]["propagated"] > 0 and out["stats"]["rewires"] > 0
        kid._equals_oracle(out, refs, what)
        if vec == "-1":
            assert (done, full) == (0, 0)
        elif cap is None:
            assert done > 0 and full == 0, (done, full)
        else:
            assert full > 0, (done, full)   # the redo walk on the records has run


def test_gpu_node_resume_across_launches(gpu, monkeypatch):
    """1 500 iterations in launches of 97: every launch builds the records from the arrays and writes them back.  Equal to
    the one-launch plan (passes_shared depends on where launches end) and to the oracle."""
    kw = util.c2_kwargs(1500)
    refs = [kid._oracle_c2(1500, s) for s in SEEDS]
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="256")
    one, _, _ = kid._plan(kw, SEEDS)
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="256", RRTX_CHUNK_ITERS="97")
    chunked, _, _ = kid._plan(kw, SEEDS)
    assert chunked["stats"]["launches"] >= one["stats"]["launches"] + 15   # 1 500 iterations in launches of 97
    kid._same(chunked, one, "RRTX_CHUNK_ITERS=97 vs one launch", skip=("passes_shared",))
    kid._equals_oracle(one, refs, "one launch")
    kid._equals_oracle(chunked, refs, "launches of 97")


@pytest.mark.parametrize("res,rate,scene,seed", [(0.05, 60, "diag", 5), (0.05, 95, "diag", 8), (0.1, 20, "drv", 20),
                                                 (0.3, 20, "drv", 30), (0.05, 20, "diag", 19507)])
def test_gpu_node_moved_node_equals_oracle(gpu, monkeypatch, res, rate, scene, seed):
    """The problems of test_gpu_kid_moved_node_equals_oracle, 400 iterations, index on from the first node: a rewire moves
    a node, so the record's x, y and xq, its elen, its children's elen (from the children's record coordinates) and its
    cell change.  No instance is left UNSUPPORTED."""
    import oracle
    kw = dict(util.C2)
    if scene == "diag":
        kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)])
    else:
        kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15], obstacles=kid.DRV_OBSTACLES)
    kw.update(expand_dis=3.0, path_resolution=res, goal_sample_rate=rate, connect_circle_dist=50.0, max_iter=400,
              robot_radius=0.0)
    L = oracle.lib()
    m0, r0, m1, r1 = C.c_long(), C.c_long(), C.c_long(), C.c_long()
    L.orc_moved_counters(C.byref(m0), C.byref(r0))
    r = util.run_oracle(kw, seed, exact_pow=True)
    L.orc_moved_counters(C.byref(m1), C.byref(r1))
    assert m1.value - m0.value > 0   # the branch is reached
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="0")
    out, _, _ = kid._plan(kw, [seed, seed + 1000])
    util.assert_tree_equal(out["trees"][0], (r["x"], r["y"], r["cost"], r["parent"]), "moved-node problem")
    assert (out["paths"][0] is None) == (r["path"] is None)
    if r["path"] is not None:
        assert np.array_equal(out["paths"][0], r["path"])
    assert not (out["results"][2] & 16).any()   # no instance left as UNSUPPORTED


@pytest.mark.parametrize("tpb", ["128", "256"])
def test_gpu_node_larger_shapes_equal_oracle(gpu, monkeypatch, tpb):
    """C2 at 1 500 iterations on the 128- and the 256-thread shape: the same body, the records written by wave 0 and
    gathered by every wave."""
    kw = util.c2_kwargs(1500)
    _env(monkeypatch, tpb=tpb)
    out, _, _ = kid._plan(kw, SEEDS)
    kid._equals_oracle(out, [kid._oracle_c2(1500, s) for s in SEEDS], "RRTX_TPB=" + tpb)


def test_gpu_node_overflow_replan_equals_oracle(gpu, monkeypatch):
    """The scene of test_gpu_kid_general_kernel_on_the_same_records: near sets outgrow the 44 candidate slots of the
    64-thread shape (its launch ends early and still writes its records back), the instances are planned again on the
    larger shapes.  Trees equal the oracle's."""
    kw = dict(util.C2)
    kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15], expand_dis=3.0, path_resolution=0.5, max_iter=700,
              obstacles=kid.DRV_OBSTACLES, robot_radius=0.8)
    _env(monkeypatch)
    seeds = list(range(1, 9))
    out, _, _ = kid._plan(kw, seeds)
    assert out["stats"]["near_unique_max"] > 44
    for i, s in enumerate(seeds):
        r = util.run_oracle(kw, s, exact_pow=True)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "seed %d" % s)


def test_gpu_node_reused_handle_keeps_no_stale_record(gpu, monkeypatch):
    """Plan, change the seeds, plan again on the same handle (1 500 iterations).  Between the plans get_path and the
    smoothing call return what they return on a handle that planned the first seeds only; the second plan equals a fresh
    handle's and the oracle's: no record of the first plan survives."""
    kw = util.c2_kwargs(1500)
    s1, s2 = list(SEEDS), [s + 20 for s in SEEDS]
    n = len(s1)
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="256")

    def first_plan_values(h):
        paths = [h.get_path(i) for i in range(n)]
        h.smooth_planned(50)
        return paths, [h.get_smoothed_path(i) for i in range(n)]

    def same_paths(a, b, what):
        for pa, pb in zip(a, b):
            assert (pa is None) == (pb is None), what
            if pa is not None:
                assert np.array_equal(pa, pb), what

    h = _handle(kw, n)
    try:
        h.seed_instances(s1)
        h.plan(strict=True)
        want_paths, want_smooth = first_plan_values(h)
    finally:
        h.close()
    h = _handle(kw, n)
    try:
        h.seed_instances(s2)
        h.plan(strict=True)
        fresh2 = _read(h, n)
    finally:
        h.close()
    h = _handle(kw, n)
    try:
        h.seed_instances(s1)
        h.plan(strict=True)
        first = _read(h, n)
        h.seed_instances(s2)   # staged for the next plan
        got_paths, got_smooth = first_plan_values(h)
        h.plan(strict=True)
        second = _read(h, n)
    finally:
        h.close()
    refs1 = [kid._oracle_c2(1500, s) for s in s1]
    kid._equals_oracle(first, refs1, "first plan")
    same_paths(got_paths, [r["path"] for r in refs1], "get_path between the plans")
    same_paths(got_paths, want_paths, "get_path between the plans vs a handle planned once")
    same_paths(got_smooth, want_smooth, "smoothed paths between the plans vs a handle planned once")
    print("paths found by the first plan: %d of %d" % (sum(p is not None for p in got_paths), n))
    kid._same(second, fresh2, "second plan vs a fresh handle")
    kid._equals_oracle(second, [kid._oracle_c2(1500, s) for s in s2], "second plan")


def test_gpu_node_no_index_equals_oracle(gpu, monkeypatch):
    """RRTX_GRID=0 at 1 500 iterations: the streaming passes read xq[], x[], y[] while the candidates come from the
    records."""
    kw = util.c2_kwargs(1500)
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID="0")
    out, _, _ = kid._plan(kw, SEEDS)
    kid._equals_oracle(out, [kid._oracle_c2(1500, s) for s in SEEDS], "RRTX_GRID=0")


def test_gpu_node_informed_planner_is_untouched(gpu):
    """One Informed RRT* golden plan: the kernel that shares the launch context but has no records."""
    path = min(util.golden_files("rrt07"), key=lambda p: len(util.load_golden(p)["x"]))
    g = util.load_golden(path)
    kw = util.informed_kwargs_from_golden(g)
    out = util.run_gpu_informed(kw, [int(g["seed"])], trace_instance=0)
    d = util.first_trace_divergence(out["trace"], g["tr_rnd_x"], g["tr_rnd_y"], g["tr_nearest"])
    assert d is None, "first divergent iteration %d" % d
    util.assert_tree_equal(out["trees"][0], (g["x"], g["y"], g["cost"], g["parent"]), g["name"])
    p = out["paths"][0]
    if len(g["path"]) == 0:
        assert p is None
    else:
        assert p is not None and np.array_equal(p, g["path"])

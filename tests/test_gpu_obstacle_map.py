"""GPU (-m gpu): the obstacle map (rrtx_set_obstacle_map) -- any number of circles up to 2**20 for rrt_01 / rrt_02 / rrt_04.
The index alone against the Python restatement (tests/obsmap_util.py), and plans on it: bit for bit the reference's goldens,
the oracle's trees, paths, RNG state and decision counters, the same answers whatever the tile size and the cell count, the
same answers as the 256-circle tile where both apply, and the handle's life between map, larger map, tile and map again."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import obsmap_util as OM
import util

pytestmark = pytest.mark.gpu

WIDE3 = [(30.0, 70.0, 14.0), (70.0, 30.0, 14.0), (50.0, 50.0, 9.0)]
_cache = {}


def base():
    if "base" not in _cache:
        _cache["base"] = util.synth_map(13, 1000, 0.3, 0.9)
    return _cache["base"]


def c2(max_iter, obstacles, **upd):
    kw = util.c2_kwargs(max_iter)
    kw["obstacles"] = obstacles
    kw.update(upd)
    return kw


def oracle(kw, seed):
    """One oracle plan per (problem, seed), shared by the tests that need it."""
    key = (repr(sorted((k, v) for k, v in kw.items() if k != "obstacles")), len(kw["obstacles"]),
           hash(tuple(map(tuple, kw["obstacles"]))), seed)
    if key not in _cache:
        _cache[key] = util.run_oracle(kw, seed, exact_pow=True)
    return _cache[key]


def make_handle(kw, n):
    import rrt_amd
    A = rrt_amd._abi
    return A.Handle({"rrt": A.ALGO_RRT, "rrt_star": A.ALGO_RRT_STAR}[kw["algo"]], kw["start"], kw["goal"], kw["rand_area"],
                    kw["expand_dis"], kw["path_resolution"], kw["goal_sample_rate"], kw["max_iter"],
                    play_area=kw["play_area"], robot_radius=kw["robot_radius"],
                    sampler=A.SAMPLER_SOBOL if kw["sobol"] else A.SAMPLER_MT,
                    connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=kw["search_until_max_iter"],
                    n_instances=n)


def plan(kw, seeds, use_map=True):
    h = make_handle(kw, len(seeds))
    try:
        (h.set_obstacle_map if use_map else h.set_obstacles)(kw["obstacles"])
        h.seed_instances(seeds)
        h.plan(strict=True)
        out = util.read_planned(h, len(seeds), sobol=bool(kw["sobol"]))
        if use_map:
            out["info"] = h.obstacle_map_info()
            assert out["stats"]["main_shape"] == 256            # the general kernel's shape, whatever the plan
    finally:
        h.close()
    return out


def same(a, b, what):
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        util.assert_tree_equal(ta, tb, "%s, instance %d" % (what, i))
    for pa, pb in zip(a["paths"], b["paths"]):
        assert (pa is None) == (pb is None), what
        if pa is not None:
            assert np.array_equal(pa, pb), what
    for ra, rb in zip(a["results"], b["results"]):
        assert np.array_equal(ra, rb), what
    assert a["rng"] == b["rng"], what
    assert a.get("sobol_index") == b.get("sobol_index"), what
    for k in OM.DECISIONS:
        assert a["stats"][k] == b["stats"][k], (what, k)


def equals_oracle(kw, seeds, out, what):
    tot = {k: 0 for k in OM.DECISIONS if k != "iterations"}
    nodes = []
    for i, s in enumerate(seeds):
        r = oracle(kw, s)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "%s seed %d" % (what, s))
        assert (out["paths"][i] is None) == (r["path"] is None), what
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"]), what
        assert out["results"][1][i] == len(r["x"]) and bool(out["results"][2][i] & 2) == (r["path"] is not None)
        assert out["rng"][i][1] == tuple(int(w) for w in r["rng"].mt) + (int(r["rng"].pos),), what
        for k in tot:
            tot[k] += r["stats"][k]
        nodes.append(len(r["x"]))
    for k in tot:
        assert out["stats"][k] == tot[k], (what, k)
    return nodes


# ---- 1. the index alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m0", "m1", "m257", "base", "m20000", "base_wide"])
def test_gpu_index_equals_restatement(gpu, name):
    circles = {"m0": [], "m1": [(40.0, 60.0, 2.0)], "m257": util.synth_map(4, 257), "base": base(),
               "m20000": util.synth_map(3, 20000, 0.05, 0.2), "base_wide": base() + WIDE3}[name]
    for rr in (0.0, 0.25):
        kw = c2(10, circles, robot_radius=rr)
        h = make_handle(kw, 1)
        try:
            h.set_obstacle_map(circles)
            info = OM.assert_map_equals(h, kw["rand_area"], circles, rr)
        finally:
            h.close()
        assert info["n_wide"] == (3 if name == "base_wide" else 0)
        assert info["nx"] == {"m0": 8, "m1": 8, "m257": 17, "base": 32, "m20000": 142, "base_wide": 32}[name]


# ---- 2. the reference's goldens ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nodes", [("obsmap_rrt04_m1000_s5", 955), ("obsmap_rrt04_m1000_s5_early", 464),
                                        ("obsmap_rrt01_m1000_s5", 458)])
def test_gpu_goldens_bit_for_bit(gpu, name, nodes):
    import os
    g = util.load_golden(os.path.join(util.GOLDEN, name + ".npz"))
    kw = util.kwargs_from_golden(g)
    assert len(kw["obstacles"]) == 1000 and kw["obstacles"] == [tuple(map(float, o)) for o in base()] and kw["max_iter"] == 1500
    assert len(g["x"]) == nodes and len(g["path"]) == 89
    out = plan(kw, [int(g["seed"])])
    util.assert_tree_equal(out["trees"][0], (g["x"], g["y"], g["cost"] if kw["algo"] == "rrt_star" else None, g["parent"]), name)
    assert np.array_equal(out["paths"][0], g["path"])
    st = out["rng"][0]
    assert st[1][624] == int(g["rng_pos_after"]) and st[1][0] == int(g["rng_word0_after"])
    assert out["results"][1][0] == nodes and out["results"][2][0] & 2
    equals_oracle(kw, [int(g["seed"])], out, name)


# ---- 3. the oracle, more ground ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("until", [1, 0])
def test_gpu_robot_radius_equals_oracle(gpu, until):
    kw = c2(4000, base(), robot_radius=0.25, search_until_max_iter=until)
    nodes = equals_oracle(kw, [5, 6], plan(kw, [5, 6]), "robot_radius 0.25")
    if until:
        assert nodes == [2422, 2494]


def test_gpu_sobol_play_area_equals_oracle(gpu):
    kw = c2(1500, base(), sobol=1, play_area=[0, 100, 0, 100])
    out = plan(kw, [5])
    assert equals_oracle(kw, [5], out, "sobol, play area") == [1076] and out["paths"][0] is not None
    assert out["sobol_index"][0] > 0


def test_gpu_wide_list_equals_oracle(gpu):
    kw = c2(4000, base() + WIDE3)
    out = plan(kw, [5, 6])
    assert out["info"]["n_wide"] == 3
    assert equals_oracle(kw, [5, 6], out, "wide list") == [2385, 2270]
    assert all(p is not None for p in out["paths"])


def test_gpu_20000_circles_equal_oracle(gpu):
    kw = c2(4000, util.synth_map(3, 20000, 0.05, 0.2))
    out = plan(kw, [5])
    assert equals_oracle(kw, [5], out, "20 000 circles") == [1958] and out["paths"][0] is not None


def test_gpu_rrt_equals_oracle(gpu):
    kw = c2(3000, base(), algo="rrt", search_until_max_iter=0)
    out = plan(kw, [5, 6, 7])
    assert equals_oracle(kw, [5, 6, 7], out, "rrt") == [458, 744, 253]
    assert all(p is not None for p in out["paths"])


# ---- 4. many tiles per box -----------------------------------------------------------------------------------------------
def crowded_kw():
    return c2(500, util.synth_map(13, 4000, 0.02, 0.08), expand_dis=20.0, path_resolution=0.5)


def nodes_with_crowded_box(tree, kw):
    """Nodes k whose box of half-width min(expand_dis, 50 sqrt(ln(k + 1) / (k + 1))) holds more than 256 circle centres."""
    o = np.asarray(kw["obstacles"])
    count = 0
    for k in range(len(tree[0])):
        half = min(kw["expand_dis"], 50.0 * math.sqrt(math.log(k + 1) / (k + 1)))
        inside = (np.abs(o[:, 0] - tree[0][k]) <= half) & (np.abs(o[:, 1] - tree[1][k]) <= half)
        count += int(inside.sum() > 256)
    return count


def test_gpu_many_tiles_per_box_equal_oracle(gpu):
    kw = crowded_kw()
    out = plan(kw, [5, 6])
    nodes = equals_oracle(kw, [5, 6], out, "many tiles per box")
    assert nodes == [482, 484]
    for i in range(2):
        assert nodes_with_crowded_box(out["trees"][i], kw) >= 30      # a condition on the input, not a measurement
    assert out["stats"]["rewires"] == 166 + 127


# ---- 5. the knobs change nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["golden", "crowded"])
def test_gpu_knobs_change_nothing(gpu, monkeypatch, case):
    kw, seeds = (c2(1500, base()), [5]) if case == "golden" else (crowded_kw(), [5])
    default = plan(kw, seeds)
    equals_oracle(kw, seeds, default, case)
    for knob, value in (("RRTX_OBSMAP_TILE", "8"), ("RRTX_OBSMAP_CELLS", "1"), ("RRTX_OBSMAP_CELLS", "1024")):
        monkeypatch.setenv(knob, value)
        got = plan(kw, seeds)
        monkeypatch.delenv(knob)
        same(got, default, "%s, %s=%s" % (case, knob, value))
        if knob == "RRTX_OBSMAP_CELLS":
            assert got["info"]["nx"] == got["info"]["ny"] == int(value)
            if value == "1":                                          # one cell: every box streams the whole list
                assert got["info"]["n_items"] == len(kw["obstacles"]) and got["info"]["n_wide"] == 0
                assert got["stats"]["algorithmic_bytes"] > default["stats"]["algorithmic_bytes"]


# ---- 6. the same answers as the tile where both apply --------------------------------------------------------------------
@pytest.mark.parametrize("until", [1, 0])
def test_gpu_map_equals_tile_at_256(gpu, monkeypatch, until):
    kw = util.c2_kwargs(1500, m=256, map_seed=13)
    kw["search_until_max_iter"] = until
    seeds = [5, 6]
    on_map = plan(kw, seeds)
    equals_oracle(kw, seeds, on_map, "m = 256 through the map")
    same(plan(kw, seeds, use_map=False), on_map, "tile, default dispatch")
    monkeypatch.setenv("RRTX_KERNEL", "v1")
    tile = plan(kw, seeds, use_map=False)
    assert tile["stats"]["main_shape"] == 256
    same(tile, on_map, "tile, RRTX_KERNEL=v1")
    same(plan(kw, seeds), on_map, "map, RRTX_KERNEL=v1")


# ---- 7. moved nodes ------------------------------------------------------------------------------------------------------
def test_gpu_moved_nodes_equal_oracle(gpu):
    import oracle as orc
    kw = dict(util.C2)
    kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], expand_dis=3.0, path_resolution=0.05, goal_sample_rate=60,
              connect_circle_dist=50.0, max_iter=1500, robot_radius=0.0)
    rng = random.Random(99)
    filler = []
    while len(filler) < 300:
        x, y, r = rng.uniform(-2, 12), rng.uniform(-2, 12), rng.uniform(0.01, 0.05)
        if min(math.hypot(x - px, y - py) for px, py in (kw["start"], kw["goal"])) > 0.5:
            filler.append((x, y, r))
    kw["obstacles"] = [(3.0, 3.0, 1.0)] + filler
    L = orc.lib()
    seeds = [5, 1005]
    for s in seeds:
        m0, r0, m1, r1 = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        L.orc_moved_counters(C.byref(m0), C.byref(r0))
        oracle(kw, s)
        L.orc_moved_counters(C.byref(m1), C.byref(r1))
        assert m1.value - m0.value >= 10          # rewire_raw_walk and the back-edge re-evaluation run under the map
    equals_oracle(kw, seeds, plan(kw, seeds), "moved nodes")


# ---- 8. lifecycle --------------------------------------------------------------------------------------------------------
def test_gpu_map_larger_map_tile_and_map_again_on_one_handle(gpu):
    map_a, map_b, tile = base(), util.synth_map(3, 20000, 0.05, 0.2), util.synth_map(7, 50)
    kw = c2(1500, map_a)
    seeds = [5, 6]
    fresh = {"a": plan(kw, seeds), "b": plan(dict(kw, obstacles=map_b), seeds),
             "t": plan(dict(kw, obstacles=tile), seeds, use_map=False)}
    h = make_handle(kw, len(seeds))
    try:
        h.seed_instances(seeds)
        for step, (which, lst) in enumerate((("a", map_a), ("b", map_b), ("t", tile), ("a", map_a))):
            (h.set_obstacles if which == "t" else h.set_obstacle_map)(lst)
            h.seed_instances(seeds)
            h.plan(strict=True)
            got = util.read_planned(h, len(seeds))
            same(got, fresh[which], "step %d (%s)" % (step, which))
            if which == "t":
                with pytest.raises(Exception, match="no obstacle map"):
                    h.obstacle_map_info()
                assert got["stats"]["main_f32"] == 1                  # back on the iteration kernel
            else:
                OM.assert_map_equals(h, kw["rand_area"], lst)
    finally:
        h.close()


def test_gpu_plan_in_steps_and_set_mid_plan(gpu):
    import rrt_amd
    A = rrt_amd._abi
    kw = c2(1500, base())
    seeds = [5, 6]
    one_shot = plan(kw, seeds)
    h = make_handle(kw, len(seeds))
    try:
        h.set_obstacle_map(kw["obstacles"])
        h.seed_instances(seeds)
        h.set_launch_bound(400)
        h.plan_begin()
        rc = h.L.rrtx_set_obstacle_map(h._h, None, 0)
        assert rc == -5 and "in progress" in h.last_error()          # RRTX_E_STATE; the running plan goes on
        steps = 0
        while True:
            rc, pending = h.plan_step()
            steps += 1
            if pending == 0:
                break
        assert steps >= 4
        same(util.read_planned(h, len(seeds)), one_shot, "plan in bounded steps")
        with pytest.raises(A.RrtxError, match="obstacle map"):
            h.smooth_planned(10)
        assert h.L.rrtx_query_goals(h._h, 1, 0, np.array([1.0, 2.0, 0.0]).ctypes.data, math.nan, math.nan) == -5
        assert "obstacle map" in h.last_error()
    finally:
        h.close()


def test_gpu_batch_planner_shards_and_drop_in(gpu):
    import os
    import rrt_amd
    import rrt_amd.rrt_04
    kw = c2(1500, base())
    seeds = [5, 6, 7, 8]
    args = ("rrt_star", seeds, kw["start"], kw["goal"], kw["obstacles"], kw["rand_area"])
    opts = dict(expand_dis=kw["expand_dis"], path_resolution=kw["path_resolution"], max_iter=1500, search_until_max_iter=True)
    got = []
    for devices in (None, [0, 0]):
        bp = rrt_amd.BatchPlanner(*args, devices=devices, **opts)
        try:
            assert bp.has_obstacle_map
            bp.plan()
            got.append(([bp.tree(i) for i in range(4)], [bp.path(i) for i in range(4)], bp.results(), bp.stats()))
            for call in (lambda: bp.smooth(10), lambda: bp.query_goals([[50.0, 50.0]])):
                with pytest.raises(ValueError, match="obstacle map"):
                    call()
        finally:
            bp.close()
    for i in range(4):
        util.assert_tree_equal(got[0][0][i], got[1][0][i], "sharded, instance %d" % i)
        assert np.array_equal(got[0][1][i], got[1][1][i])
    for ra, rb in zip(got[0][2], got[1][2]):
        assert np.array_equal(ra, rb)
    for k in OM.DECISIONS:
        assert got[0][3][k] == got[1][3][k], k
    r = oracle(kw, 5)
    util.assert_tree_equal(got[0][0][0], (r["x"], r["y"], r["cost"], r["parent"]), "batch, seed 5")
    with pytest.raises(rrt_amd._abi.RrtxError, match="256"):
        rrt_amd.BatchPlanner(*args, obstacle_map=False, **opts)
    # the drop-in class: 1 000 circles plan where they raised before, and give the reference's path
    g = util.load_golden(os.path.join(util.GOLDEN, "obsmap_rrt04_m1000_s5.npz"))
    random.seed(5)
    p = rrt_amd.rrt_04.RRT(start=kw["start"], goal=kw["goal"], obstacle_list=base(), rand_area=kw["rand_area"], expand_dis=2.0,
                           path_resolution=0.25, goal_sample_rate=5, max_iter=1500, sobol_sampler=False,
                           search_until_max_iter=True)
    path = p.planning(animation=False)
    assert np.array_equal(np.array(path), g["path"])
    assert random.getstate()[1][624] == int(g["rng_pos_after"])
    p = rrt_amd.rrt_04.RRT(start=kw["start"], goal=kw["goal"], obstacle_list=base(), rand_area=kw["rand_area"])
    p.obstacle_map = False
    with pytest.raises(rrt_amd._abi.RrtxError, match="256"):
        p.planning(animation=False)


def test_gpu_other_planners_refuse_the_map(gpu):
    import rrt_amd
    A = rrt_amd._abi
    c_min, c = rrt_amd.informed_rotation([2.0, 2.0], [98.0, 98.0])
    h = A.Handle(A.ALGO_INFORMED, [2.0, 2.0], [98.0, 98.0], [0.0, 100.0], 2.0, 1.0, 5, 100,
                 informed_rot=[c[0, 0], c[0, 1], c[1, 0], c[1, 1]], informed_c_min=c_min)
    try:
        with pytest.raises(A.RrtxError, match="RRTX_ALGO_RRT"):
            h.set_obstacle_map(base())
        with pytest.raises(A.RrtxError, match="256"):
            h.set_obstacles(base())
    finally:
        h.close()

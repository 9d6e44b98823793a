"""GPU (-m gpu): the per-iteration obstacle cull of the rrt_04 iteration kernel's one-wave shape (RRTX_OBS_CULL).  With
the cull the candidate edges of an iteration are tested against the obstacles that reach the near ball of its new node
only, one edge per lane; without it (RRTX_OBS_CULL=0) every edge meets every obstacle of the tile in (edge, obstacle)
pairs.  Either way trees, costs, parents, paths, result tables and every decision counter are the same, and equal to the
oracle."""
import math

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

DECISIONS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations",
             "exact_rescans", "f32_fallbacks", "q16_fallbacks", "passes_shared")


def _run(monkeypatch, kw, seeds, cull):
    monkeypatch.setenv("RRTX_TPB", "64")
    monkeypatch.setenv("RRTX_OBS_CULL", cull)
    out = util.run_gpu_batch(kw, seeds)
    assert out["stats"]["main_shape"] == 64   # the cull exists in the one-wave shape only
    return out


def _same(a, b, what):
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        util.assert_tree_equal(ta, tb, "%s, instance %d" % (what, i))
    for pa, pb in zip(a["paths"], b["paths"]):
        assert (pa is None) == (pb is None), what
        if pa is not None:
            assert np.array_equal(pa, pb), what
    for ra, rb in zip(a["results"], b["results"]):
        assert np.array_equal(ra, rb), what
    for k in DECISIONS:
        assert a["stats"][k] == b["stats"][k], (what, k)


def _oracle(kw, seeds, out, what):
    tot = {k: 0 for k in ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated")}
    for i, s in enumerate(seeds):
        r = util.run_oracle(kw, s, exact_pow=True)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "%s seed %d" % (what, s))
        assert (out["paths"][i] is None) == (r["path"] is None)
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"])
        for k in tot:
            tot[k] += r["stats"][k]
    for k in tot:
        assert out["stats"][k] == tot[k], (what, k)


def _on_off_oracle(monkeypatch, kw, seeds, what):
    on = _run(monkeypatch, kw, seeds, "1")
    off = _run(monkeypatch, kw, seeds, "0")
    _same(on, off, "%s, RRTX_OBS_CULL=1 vs 0" % what)
    _oracle(kw, seeds, on, what)
    return on


def _obstacles_near_nodes(tree, obstacles, margin):
    """Per node of the tree: how many obstacles lie within size + margin of it."""
    x, y = np.asarray(tree[0]), np.asarray(tree[1])
    o = np.asarray(obstacles, dtype=np.float64)
    d = np.hypot(x[:, None] - o[None, :, 0], y[:, None] - o[None, :, 1])
    return (d <= o[None, :, 2] + margin).sum(axis=1)


def test_gpu_cull_c2_equals_oracle(gpu, monkeypatch):
    """The C2 map (50 obstacles) at 6 000 iterations, four seeds: most iterations have an empty mask."""
    kw = util.c2_kwargs(6000)
    _on_off_oracle(monkeypatch, kw, [11, 12, 13, 14], "C2")


def test_gpu_cull_crowded_map_equals_oracle(gpu, monkeypatch):
    """56 obstacles (the one-wave shape's tile limit) of radius 3 - 6 on the 100 x 100 map and near balls up to 6 wide
    (expand_dis 6, 2 000 iterations: the ball never shrinks below 3.7): non-empty masks are the rule and many hold several
    bits.  Checked on the tree the plan built -- every node was a new node once, and its ball was at least as wide as
    the plan's last one: with that smallest radius over 40 % of the nodes have an obstacle in reach and over 10 % have two
    or more (the masks themselves, built from each iteration's own wider ball, hold more)."""
    kw = util.c2_kwargs(2000)
    kw["obstacles"] = util.synth_map(5, 56, rmin=3.0, rmax=6.0)
    kw["expand_dis"] = 6.0
    seeds = [21, 22, 23]
    on = _on_off_oracle(monkeypatch, kw, seeds, "crowded map")
    n = len(on["trees"][0][0])
    r_last = min(kw["expand_dis"], kw["connect_circle_dist"] * math.sqrt(math.log(n + 1) / (n + 1)))
    near = _obstacles_near_nodes(on["trees"][0], kw["obstacles"], r_last)
    assert (near >= 1).mean() > 0.4, (near >= 1).mean()
    assert (near >= 2).mean() > 0.1, (near >= 2).mean()


def test_gpu_cull_robot_radius_equals_oracle(gpu, monkeypatch):
    """robot_radius > 0: the thresholds the mask is built from are (size + robot_radius) ** 2."""
    kw = util.c2_kwargs(5000)
    kw["robot_radius"] = 0.8
    _on_off_oracle(monkeypatch, kw, [31, 32], "robot_radius 0.8")


@pytest.mark.parametrize("res,rate,scene,seed", [(0.05, 60, "diag", 5), (0.1, 20, "drv", 20), (0.3, 20, "drv", 30)])
def test_gpu_cull_moved_nodes_equal_oracle(gpu, monkeypatch, res, rate, scene, seed):
    """Scenes where rewire moves nodes: the winning edge does not snap, the backward edges are evaluated again from its end
    point (eval_edges_back2) under the same mask.  Near balls of radius 3 on maps 14 - 17 wide: dense masks."""
    kw = dict(util.C2)
    if scene == "diag":
        kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)])
    else:
        kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15],
                  obstacles=[(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)])
    kw.update(expand_dis=3.0, path_resolution=res, goal_sample_rate=rate, connect_circle_dist=50.0, max_iter=1500,
              robot_radius=0.0)
    _on_off_oracle(monkeypatch, kw, [seed, seed + 1000], "moved nodes")


def test_gpu_cull_goal_heavy_equals_oracle(gpu, monkeypatch):
    """Half the samples on the goal: thousands of exact goal duplicates, candidate lists that take several edge passes."""
    kw = util.c2_kwargs(6000)
    kw["goal_sample_rate"] = 50
    _on_off_oracle(monkeypatch, kw, [41, 42], "goal-heavy")


def test_gpu_cull_instance_maps_equal_oracle(gpu, monkeypatch):
    """A batch with one obstacle map per instance (0, 3, 20 and 56 obstacles, sparse next to crowded): each instance's
    mask comes from its own tile."""
    import rrt_amd
    monkeypatch.setenv("RRTX_TPB", "64")
    kw = util.c2_kwargs(2500)
    lists = [[], util.synth_map(1, 56), util.synth_map(2, 3), util.synth_map(5, 56, rmin=4.0, rmax=9.0), util.synth_map(4, 20)]
    seeds = [51, 52, 53, 54, 55]
    got = {}
    for cull in ("1", "0"):
        monkeypatch.setenv("RRTX_OBS_CULL", cull)
        bp = rrt_amd.BatchPlanner("rrt_star", seeds, kw["start"], kw["goal"], None, kw["rand_area"], instance_obstacles=lists,
                                  expand_dis=kw["expand_dis"], path_resolution=kw["path_resolution"], max_iter=2500,
                                  search_until_max_iter=True)
        try:
            bp.plan()
            assert bp.stats()["main_shape"] == 64
            got[cull] = dict(trees=[bp.tree(i) for i in range(len(seeds))], paths=[bp.path(i) for i in range(len(seeds))],
                             stats=bp.stats())
        finally:
            bp.close()
    for i, s in enumerate(seeds):
        util.assert_tree_equal(got["1"]["trees"][i], got["0"]["trees"][i], "instance maps, RRTX_OBS_CULL=1 vs 0, instance %d" % i)
        r = util.run_oracle(dict(kw, obstacles=lists[i]), s)
        util.assert_tree_equal(got["1"]["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "instance maps, instance %d" % i)
        pa, pb = got["1"]["paths"][i], got["0"]["paths"][i]
        assert (pa is None) == (pb is None) == (r["path"] is None)
        if pa is not None:
            assert np.array_equal(pa, pb)
            assert np.array_equal(pa if pa.shape[1] == 2 else pa[:, :2], r["path"])
    for k in DECISIONS:
        assert got["1"]["stats"][k] == got["0"]["stats"][k], k

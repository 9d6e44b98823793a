"""GPU (-m gpu): the grid index of the rrt_04 iteration kernel's 16-bit stage (one-wave shape, RRTX_GRID).  A pass answered
from the index must be indistinguishable from the streaming pass: same trees, paths and decision counters, equal to the
oracle.  RRTX_GRID_MIN=0 lets the index answer from the first node, so small problems exercise it too."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

DECISIONS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations",
             "exact_rescans", "f32_fallbacks", "q16_fallbacks", "passes_shared")


def _run(monkeypatch, kw, seeds, grid, grid_min=None):
    monkeypatch.setenv("RRTX_TPB", "64")
    monkeypatch.setenv("RRTX_GRID", grid)
    if grid_min is None:
        monkeypatch.delenv("RRTX_GRID_MIN", raising=False)
    else:
        monkeypatch.setenv("RRTX_GRID_MIN", grid_min)
    return util.run_gpu_batch(kw, seeds)


def _same(a, b, what):
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        util.assert_tree_equal(ta, tb, "%s, instance %d" % (what, i))
    for pa, pb in zip(a["paths"], b["paths"]):
        assert (pa is None) == (pb is None), what
        if pa is not None:
            assert np.array_equal(pa, pb), what
    for k in DECISIONS:
        assert a["stats"][k] == b["stats"][k], (what, k)


def _oracle(kw, seeds, out, what, exact_pow=True):
    for i, s in enumerate(seeds):
        r = util.run_oracle(kw, s, exact_pow=exact_pow)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "%s seed %d" % (what, s))
        assert (out["paths"][i] is None) == (r["path"] is None)
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"])


def test_gpu_grid_full_size_equals_streaming_and_oracle(gpu, monkeypatch):
    """C2 at full size (105 000 iterations) on the bench's shape: the index on and off give identical trees, paths and
    decision counters, equal to the oracle -- and the index answers most passes (the kernel reads a small fraction of the
    bytes the streaming passes read)."""
    kw = util.c2_kwargs(105000)
    on = _run(monkeypatch, kw, [1], "1")
    off = _run(monkeypatch, kw, [1], "0")
    _same(on, off, "RRTX_GRID=1 vs 0")
    assert on["stats"]["q16_fallbacks"] > 0
    b_on, b_off = on["stats"]["algorithmic_bytes"], off["stats"]["algorithmic_bytes"]
    assert b_on * 5 < b_off, (b_on, b_off)
    r = util.run_oracle(kw, 1, exact_pow=False)
    util.assert_tree_equal(on["trees"][0], (r["x"], r["y"], r["cost"], r["parent"]), "seed 1, 105k, grid")
    assert np.array_equal(on["paths"][0], r["path"])
    for k in ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations"):
        assert on["stats"][k] == r["stats"][k], k


@pytest.mark.parametrize("res,rate,scene,seed", [(0.05, 60, "diag", 5), (0.1, 20, "drv", 20), (0.3, 20, "drv", 30)])
def test_gpu_grid_moved_nodes_equal_oracle(gpu, monkeypatch, res, rate, scene, seed):
    """Scenes where rewire moves nodes (tools/find_moved_node.py), the index on from the first node: a moved node changes
    cell in the index.  (Their near balls hold a large part of these small maps, so many passes stream.)"""
    kw = dict(util.C2)
    if scene == "diag":
        kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)])
    else:
        kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15],
                  obstacles=[(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)])
    kw.update(expand_dis=3.0, path_resolution=res, goal_sample_rate=rate, connect_circle_dist=50.0, max_iter=1500,
              robot_radius=0.0)
    seeds = [seed, seed + 1000]
    on = _run(monkeypatch, kw, seeds, "1", "0")
    off = _run(monkeypatch, kw, seeds, "0")
    _same(on, off, "moved nodes, RRTX_GRID=1 vs 0")
    _oracle(kw, seeds, on, "moved nodes, grid")


def test_gpu_grid_goal_duplicates_equal_oracle(gpu, monkeypatch):
    """A goal-heavy plan: thousands of exact goal duplicates stay out of the index and are counted like the streaming
    pass counts them."""
    kw = util.c2_kwargs(8000)
    kw["goal_sample_rate"] = 40
    seeds = [3, 4]
    on = _run(monkeypatch, kw, seeds, "1", "0")
    off = _run(monkeypatch, kw, seeds, "0")
    _same(on, off, "goal duplicates, RRTX_GRID=1 vs 0")
    assert on["stats"]["algorithmic_bytes"] * 2 < off["stats"]["algorithmic_bytes"]
    _oracle(kw, seeds, on, "goal duplicates, grid")


def test_gpu_grid_fallback_large_obstacles_equals_oracle(gpu, monkeypatch):
    """Large obstacles: samples deep inside them are far from every node, the nearest query's window passes its cap and
    the pass streams -- the answers stay those of the streaming pass."""
    kw = dict(util.C2)
    kw.update(obstacles=[(30, 30, 14), (70, 65, 16), (25, 75, 10), (75, 20, 9)], max_iter=8000)
    seeds = [5, 6]
    on = _run(monkeypatch, kw, seeds, "1", "0")
    off = _run(monkeypatch, kw, seeds, "0")
    _same(on, off, "large obstacles, RRTX_GRID=1 vs 0")
    _oracle(kw, seeds, on, "large obstacles, grid")

"""GPU (-m gpu): the merged gather of a pass over the grid index (rrt_04 iteration kernel, one-wave shape,
RRTX_GRID_MERGE).  With it a pass loads the cell counts of all its centres -- its own ball, the next sample's nearest
query, the speculative sets' balls and nearest queries -- in one round trip and their entries in a second one; without it
(RRTX_GRID_MERGE=0) centre after centre, two round trips each.  The entries a centre tests are the same either way, so
trees, paths, every decision counter and the bytes the passes read are the same, equal to the streaming pass
(RRTX_GRID=0) and to the oracle."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

DECISIONS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations",
             "exact_rescans", "f32_fallbacks", "q16_fallbacks", "passes_shared")


def _run(monkeypatch, kw, seeds, merge, grid="1", grid_min="0"):
    monkeypatch.setenv("RRTX_TPB", "64")
    monkeypatch.setenv("RRTX_GRID", grid)
    monkeypatch.setenv("RRTX_GRID_MERGE", merge)
    if grid_min is None:
        monkeypatch.delenv("RRTX_GRID_MIN", raising=False)
    else:
        monkeypatch.setenv("RRTX_GRID_MIN", grid_min)
    out = util.run_gpu_batch(kw, seeds)
    assert out["stats"]["main_shape"] == 64   # the index exists in the one-wave shape only
    return out


def _same(a, b, what, bytes_too=False):
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        util.assert_tree_equal(ta, tb, "%s, instance %d" % (what, i))
    for pa, pb in zip(a["paths"], b["paths"]):
        assert (pa is None) == (pb is None), what
        if pa is not None:
            assert np.array_equal(pa, pb), what
    for ra, rb in zip(a["results"], b["results"]):
        assert np.array_equal(ra, rb), what
    for k in DECISIONS + (("algorithmic_bytes", "scan_nodes") if bytes_too else ()):
        assert a["stats"][k] == b["stats"][k], (what, k)


def _oracle(kw, seeds, out, what, exact_pow=True):
    for i, s in enumerate(seeds):
        r = util.run_oracle(kw, s, exact_pow=exact_pow)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "%s seed %d" % (what, s))
        assert (out["paths"][i] is None) == (r["path"] is None)
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"])


def _three_ways(monkeypatch, kw, seeds, what, grid_min="0"):
    """merged == per-centre (bytes included) == streaming == oracle; returns (merged, streaming)."""
    on = _run(monkeypatch, kw, seeds, "1", grid_min=grid_min)
    off = _run(monkeypatch, kw, seeds, "0", grid_min=grid_min)
    stream = _run(monkeypatch, kw, seeds, "1", grid="0", grid_min=grid_min)
    _same(on, off, "%s, RRTX_GRID_MERGE=1 vs 0" % what, bytes_too=True)
    _same(on, stream, "%s, RRTX_GRID_MERGE=1 vs RRTX_GRID=0" % what)
    _oracle(kw, seeds, on, what)
    return on, stream


def test_gpu_merge_c2_equals_oracle(gpu, monkeypatch):
    """C2 at 8 000 iterations, four seeds, the index on from the first node."""
    kw = util.c2_kwargs(8000)
    on, stream = _three_ways(monkeypatch, kw, [11, 12, 13, 14], "C2")
    assert on["stats"]["algorithmic_bytes"] < stream["stats"]["algorithmic_bytes"]   # the index answered passes


def test_gpu_merge_full_size_same_as_per_centre(gpu, monkeypatch):
    """C2 at full size (105 000 iterations) with the default switch-over to the index: the regime the bench runs, late-plan
    windows of 2 x 2 to 3 x 3 cells, five centres per pass."""
    kw = util.c2_kwargs(105000)
    on = _run(monkeypatch, kw, [1], "1", grid_min=None)
    off = _run(monkeypatch, kw, [1], "0", grid_min=None)
    _same(on, off, "full size, RRTX_GRID_MERGE=1 vs 0", bytes_too=True)
    assert on["stats"]["passes_shared"] > on["stats"]["iterations"] // 2   # the speculative sets are in use
    r = util.run_oracle(kw, 1, exact_pow=False)
    util.assert_tree_equal(on["trees"][0], (r["x"], r["y"], r["cost"], r["parent"]), "seed 1, 105k, merged gather")
    assert np.array_equal(on["paths"][0], r["path"])


def test_gpu_merge_slow_path_young_trees(gpu, monkeypatch):
    """The slow path, forced: RRTX_GRID_MIN=0 indexes trees from the first node, whose near balls (radius expand_dis) and
    nearest windows are wide -- the windows of a pass's centres together pass 64 cells, so the pass falls back to the
    per-centre gathers, and nearest queries far from every node grow their window by themselves after the merged
    attempt.  Short plans, so that young trees are all there is."""
    kw = util.c2_kwargs(1500)
    _three_ways(monkeypatch, kw, [21, 22, 23, 24], "young trees")


def test_gpu_merge_slow_path_large_obstacles(gpu, monkeypatch):
    """Large obstacles: samples deep inside them are far from every node, their nearest window grows past the merged
    attempt or passes its cap (the pass streams)."""
    kw = dict(util.C2)
    kw.update(obstacles=[(30, 30, 14), (70, 65, 16), (25, 75, 10), (75, 20, 9)], max_iter=8000)
    _three_ways(monkeypatch, kw, [5, 6], "large obstacles")


def test_gpu_merge_speculative_sets_reach_goal_cell(gpu, monkeypatch):
    """A goal-heavy plan: two samples in five are the goal, so the speculative sets' balls reach the goal's cell all the
    time (the sets end there, the left-out goal duplicates are counted by the goal-cell rule)."""
    kw = util.c2_kwargs(8000)
    kw["goal_sample_rate"] = 40
    _three_ways(monkeypatch, kw, [3, 4], "goal cell")


@pytest.mark.parametrize("res,rate,scene,seed", [(0.05, 60, "diag", 5), (0.1, 20, "drv", 20), (0.3, 20, "drv", 30)])
def test_gpu_merge_moved_nodes_equal_oracle(gpu, monkeypatch, res, rate, scene, seed):
    """Scenes where rewire moves nodes (they change cell in the index between passes)."""
    kw = dict(util.C2)
    if scene == "diag":
        kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)])
    else:
        kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15],
                  obstacles=[(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)])
    kw.update(expand_dis=3.0, path_resolution=res, goal_sample_rate=rate, connect_circle_dist=50.0, max_iter=1500,
              robot_radius=0.0)
    _three_ways(monkeypatch, kw, [seed, seed + 1000], "moved nodes")

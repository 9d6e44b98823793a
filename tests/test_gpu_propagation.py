"""GPU (-m gpu): cost propagation of the rrt_04 iteration kernel's one-wave shape.  A walk still running after
RRTX_PROP_VEC nodes on the scalar path goes on with one sibling chain per lane (RRTX_PROP_VEC=-1: the scalar path
throughout, RRTX_PROP_VEC=0: the lanes from the first node).  Whichever path a walk takes, and when its LDS list of pending
chains is full (RRTX_PROP_CAP) and the global-stack walk redoes it, trees, paths and every decision counter are the same,
and equal to the oracle."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

DECISIONS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations",
             "exact_rescans", "f32_fallbacks", "q16_fallbacks", "passes_shared")


def _run(monkeypatch, kw, seeds, vec, cap=None, chunk=None):
    monkeypatch.setenv("RRTX_TPB", "64")
    monkeypatch.setenv("RRTX_PROP_VEC", vec)
    for var, val in (("RRTX_PROP_CAP", cap), ("RRTX_CHUNK_ITERS", chunk)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    return util.run_gpu_batch(kw, seeds)


def _same(a, b, what, skip=()):
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        util.assert_tree_equal(ta, tb, "%s, instance %d" % (what, i))
    for pa, pb in zip(a["paths"], b["paths"]):
        assert (pa is None) == (pb is None), what
        if pa is not None:
            assert np.array_equal(pa, pb), what
    for k in DECISIONS:
        if k not in skip:
            assert a["stats"][k] == b["stats"][k], (what, k)


def _oracle(kw, seeds, out, what):
    for i, s in enumerate(seeds):
        r = util.run_oracle(kw, s, exact_pow=True)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "%s seed %d" % (what, s))
        assert (out["paths"][i] is None) == (r["path"] is None)
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"])


def _stats_oracle(kw, seeds, out):
    tot = {k: 0 for k in ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated")}
    for s in seeds:
        r = util.run_oracle(kw, s, exact_pow=True)
        for k in tot:
            tot[k] += r["stats"][k]
    for k in tot:
        assert out["stats"][k] == tot[k], k


def test_gpu_prop_full_size_c2_paths_agree(gpu, monkeypatch):
    """C2 at full size (105 000 iterations), where propagations of thousands of nodes happen: the default switch-over,
    the lanes from the first node and the scalar path alone give the same trees, paths and counters.  (The default build
    is compared with the oracle at this size by the full-size tests of test_gpu_parity.py.)"""
    kw = util.c2_kwargs(105000)
    seeds = [1, 2, 3]
    scalar = _run(monkeypatch, kw, seeds, "-1")
    assert scalar["stats"]["propagated"] > 20 * scalar["stats"]["iterations"] // 2
    _same(_run(monkeypatch, kw, seeds, "8"), scalar, "RRTX_PROP_VEC=8 vs -1")
    _same(_run(monkeypatch, kw, seeds, "0"), scalar, "RRTX_PROP_VEC=0 vs -1")


@pytest.mark.parametrize("vec", ["0", "8"])
def test_gpu_prop_c2_equals_oracle(gpu, monkeypatch, vec):
    """C2 at 8 000 iterations, four seeds: trees, paths and the oracle's counters."""
    kw = util.c2_kwargs(8000)
    seeds = [11, 12, 13, 14]
    out = _run(monkeypatch, kw, seeds, vec)
    _oracle(kw, seeds, out, "RRTX_PROP_VEC=%s" % vec)
    _stats_oracle(kw, seeds, out)
    _same(out, _run(monkeypatch, kw, seeds, "-1"), "RRTX_PROP_VEC=%s vs -1" % vec)


def test_gpu_prop_goal_heavy_equals_oracle(gpu, monkeypatch):
    """Half the samples on the goal: the exact goal duplicates hang as long sibling chains under a few parents, and
    rewires under them move wide levels (more than 64 chains at once: the pending list in LDS)."""
    kw = util.c2_kwargs(6000)
    kw["goal_sample_rate"] = 50
    seeds = [21, 22]
    out = _run(monkeypatch, kw, seeds, "0")
    _oracle(kw, seeds, out, "goal-heavy")
    _same(out, _run(monkeypatch, kw, seeds, "-1"), "goal-heavy, RRTX_PROP_VEC=0 vs -1")


@pytest.mark.parametrize("res,rate,scene,seed", [(0.05, 60, "diag", 5), (0.1, 20, "drv", 20), (0.3, 20, "drv", 30)])
def test_gpu_prop_moved_nodes_equal_oracle(gpu, monkeypatch, res, rate, scene, seed):
    """Scenes where rewire moves nodes (their own and their children's edge lengths change before the walk)."""
    kw = dict(util.C2)
    if scene == "diag":
        kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)])
    else:
        kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15],
                  obstacles=[(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)])
    kw.update(expand_dis=3.0, path_resolution=res, goal_sample_rate=rate, connect_circle_dist=50.0, max_iter=1500,
              robot_radius=0.0)
    seeds = [seed, seed + 1000]
    out = _run(monkeypatch, kw, seeds, "0")
    _oracle(kw, seeds, out, "moved nodes")
    _same(out, _run(monkeypatch, kw, seeds, "-1"), "moved nodes, RRTX_PROP_VEC=0 vs -1")


@pytest.mark.parametrize("cap", ["0", "1", "3"])
def test_gpu_prop_pending_list_full(gpu, monkeypatch, cap):
    """A pending list forced small: walks that outgrow it are redone by the global-stack walk, with the same results."""
    kw = util.c2_kwargs(8000)
    seeds = [31, 32]
    full = _run(monkeypatch, kw, seeds, "0", cap=cap)
    _same(full, _run(monkeypatch, kw, seeds, "-1"), "RRTX_PROP_CAP=%s vs the scalar path" % cap)
    _oracle(kw, seeds, full, "RRTX_PROP_CAP=%s" % cap)


def test_gpu_prop_resume_across_launches(gpu, monkeypatch):
    """A plan split into launches of 700 iterations (RRTX_CHUNK_ITERS) equals the one-launch plan.  (passes_shared
    depends on where launches end: a launch starts without speculated passes.)"""
    kw = util.c2_kwargs(6000)
    seeds = [41, 42]
    one = _run(monkeypatch, kw, seeds, "0")
    _same(_run(monkeypatch, kw, seeds, "0", chunk="700"), one, "RRTX_CHUNK_ITERS=700 vs one launch", skip=("passes_shared",))
    _oracle(kw, seeds, one, "resume")


def _walks(monkeypatch, kw, seeds, vec, cap=None):
    """(walks the lanes finished, walks whose pending list ran full) of one plan, from the kernel's counter slot."""
    import rrt_amd
    A = rrt_amd._abi
    monkeypatch.setenv("RRTX_TPB", "64")
    monkeypatch.setenv("RRTX_PROP_VEC", vec)
    if cap is None:
        monkeypatch.delenv("RRTX_PROP_CAP", raising=False)
    else:
        monkeypatch.setenv("RRTX_PROP_CAP", cap)
    h = A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                 kw["goal_sample_rate"], kw["max_iter"], robot_radius=0.0, connect_circle_dist=50.0,
                 search_until_max_iter=True, n_instances=len(seeds))
    h.set_obstacles(kw["obstacles"])
    h.seed_instances(seeds)
    h.plan()
    v = int(h.get_phase_cycles()[10])
    return v & ((1 << 40) - 1), v >> 40


def test_gpu_prop_lane_walks_run_and_finish(gpu, monkeypatch):
    """The lane walk runs and finishes: at full size with the default switch-over, in the goal-heavy scene from the first
    node, and never with RRTX_PROP_VEC=-1.  A pending list forced to 3 entries runs full, and then nothing finishes."""
    kw = util.c2_kwargs(105000)
    done, full = _walks(monkeypatch, kw, [1, 2], "8")
    assert done > 1000 and full == 0, (done, full)
    assert _walks(monkeypatch, kw, [1, 2], "-1") == (0, 0)
    kg = util.c2_kwargs(6000)
    kg["goal_sample_rate"] = 50
    done, full = _walks(monkeypatch, kg, [21, 22], "0")
    assert done > 100 and full == 0, (done, full)
    done, full = _walks(monkeypatch, util.c2_kwargs(8000), [31, 32], "0", cap="3")
    assert full > 0, (done, full)

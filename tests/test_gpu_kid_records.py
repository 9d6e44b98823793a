"""GPU (-m gpu): the 16-byte node record {first_child, next_sib, elen} (rppk::Kid) and the 8-byte grid cell head
{cnt, blk} (rppk::GHead) of the rrt_04 iteration kernel.  Every tree walk -- the scalar walk, the lane walk, the
global-stack walk that redoes a subtree -- and every query and insert of the grid index reads and writes these records;
whichever path runs, trees, paths and decision counters are the same and equal the oracle's."""
import ctypes as C
import functools

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

DECISIONS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations",
             "exact_rescans", "f32_fallbacks", "q16_fallbacks", "passes_shared")
WALK_SLOT, WALK_FULL_SHIFT = 10, 40   # rrtx_get_phase_cycles: walks the lanes finished | walks whose pending list ran full << 40
SEEDS = (51, 52)
DRV_OBSTACLES = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]


@functools.lru_cache(maxsize=None)
def _oracle_c2(max_iter, seed):
    """The oracle's plan of C2 at max_iter iterations: computed once, shared by the tests, never modified."""
    return util.run_oracle(util.c2_kwargs(max_iter), seed, exact_pow=True)


def _env(monkeypatch, **env):
    monkeypatch.setenv("RRTX_TPB", "64")
    for var in ("RRTX_PROP_VEC", "RRTX_PROP_CAP", "RRTX_CHUNK_ITERS", "RRTX_GRID_MIN"):
        if var in env and env[var] is not None:
            monkeypatch.setenv(var, env[var])
        else:
            monkeypatch.delenv(var, raising=False)


def _plan(kw, seeds):
    """util.run_gpu_batch plus the kernel's walk counters: (result dict, walks finished by the lanes, walks whose pending
    list ran full)."""
    import rrt_amd
    A = rrt_amd._abi
    h = A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                 kw["goal_sample_rate"], kw["max_iter"], play_area=kw["play_area"], robot_radius=kw["robot_radius"],
                 connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=kw["search_until_max_iter"],
                 n_instances=len(seeds))
    try:
        h.set_obstacles(kw["obstacles"])
        h.seed_instances(list(seeds))
        h.plan(strict=True)
        out = dict(stats=h.get_stats(), results=h.get_results(), trees=[h.get_tree(i) for i in range(len(seeds))],
                   paths=[h.get_path(i) for i in range(len(seeds))])
        v = int(h.get_phase_cycles()[WALK_SLOT])
    finally:
        h.close()
    return out, v & ((1 << WALK_FULL_SHIFT) - 1), v >> WALK_FULL_SHIFT


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


def _equals_oracle(out, refs, what):
    for i, r in enumerate(refs):
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "%s, instance %d" % (what, i))
        assert (out["paths"][i] is None) == (r["path"] is None), what
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"]), what
    for k in ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated"):
        assert out["stats"][k] == sum(r["stats"][k] for r in refs), (what, k)


def test_gpu_kid_walks_agree_and_equal_oracle(gpu, monkeypatch):
    """C2 at 3 000 iterations, the packed cell heads answering from a tree of 256 nodes on: the scalar walk alone
    (RRTX_PROP_VEC=-1), the lane walk from the first node (0) and the lane walk with a pending list of 4 chains (the
    global-stack walk redoes the subtrees that outgrow it, on the same records) give the same trees, paths and counters,
    and they are the oracle's."""
    kw = util.c2_kwargs(3000)
    refs = [_oracle_c2(3000, s) for s in SEEDS]
    _env(monkeypatch, RRTX_PROP_VEC="-1", RRTX_GRID_MIN="256")
    scalar, done, full = _plan(kw, SEEDS)
    assert (done, full) == (0, 0)
    assert scalar["stats"]["propagated"] > 0 and scalar["stats"]["rewires"] > 0
    _equals_oracle(scalar, refs, "RRTX_PROP_VEC=-1")
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="256")
    lanes, done, full = _plan(kw, SEEDS)
    assert done > 0 and full == 0, (done, full)
    _same(lanes, scalar, "RRTX_PROP_VEC=0 vs -1")
    _equals_oracle(lanes, refs, "RRTX_PROP_VEC=0")
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_PROP_CAP="4", RRTX_GRID_MIN="256")
    capped, done, full = _plan(kw, SEEDS)
    print("RRTX_PROP_CAP=4: %d walks finished by the lanes, %d with a full pending list" % (done, full))
    assert full > 0, (done, full)   # the case tests the redo only if a pending list ran full
    _same(capped, scalar, "RRTX_PROP_CAP=4 vs the scalar path")
    _equals_oracle(capped, refs, "RRTX_PROP_CAP=4")


def test_gpu_kid_resume_across_launches(gpu, monkeypatch):
    """1 500 iterations in launches of 97 (RRTX_CHUNK_ITERS): every launch rebuilds the index into the packed heads, the
    node records persist.  Equal to the one-launch plan (passes_shared depends on where launches end) and to the
    oracle."""
    kw = util.c2_kwargs(1500)
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="256")
    one, _, _ = _plan(kw, SEEDS)
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="256", RRTX_CHUNK_ITERS="97")
    chunked, _, _ = _plan(kw, SEEDS)
    _same(chunked, one, "RRTX_CHUNK_ITERS=97 vs one launch", skip=("passes_shared",))
    _equals_oracle(one, [_oracle_c2(1500, s) for s in SEEDS], "one launch")


@pytest.mark.parametrize("res,rate,scene,seed", [(0.05, 60, "diag", 5), (0.05, 95, "diag", 8), (0.1, 20, "drv", 20),
                                                 (0.3, 20, "drv", 30), (0.05, 20, "diag", 19507)])
def test_gpu_kid_moved_node_equals_oracle(gpu, monkeypatch, res, rate, scene, seed):
    """The problems of test_gpu_rewire_moved_node_equals_oracle (an inexact path_resolution: a rewire moves a node) on
    the 64-thread shape, lane walk from the first node, index on from the first node: the moved node's children get
    their elen rewritten along the record chain, the node changes cell.  An instance the shape hands on (a moved node
    in a near set with repeats) is planned again by the general kernel, on the same records."""
    import oracle
    kw = dict(util.C2)
    if scene == "diag":
        kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)])
    else:
        kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15], obstacles=DRV_OBSTACLES)
    kw.update(expand_dis=3.0, path_resolution=res, goal_sample_rate=rate, connect_circle_dist=50.0, max_iter=400,
              robot_radius=0.0)
    L = oracle.lib()
    m0, r0, m1, r1 = C.c_long(), C.c_long(), C.c_long(), C.c_long()
    L.orc_moved_counters(C.byref(m0), C.byref(r0))
    r = util.run_oracle(kw, seed, exact_pow=True)
    L.orc_moved_counters(C.byref(m1), C.byref(r1))
    assert m1.value - m0.value > 0   # the branch is reached
    _env(monkeypatch, RRTX_PROP_VEC="0", RRTX_GRID_MIN="0")
    out, _, _ = _plan(kw, [seed, seed + 1000])
    util.assert_tree_equal(out["trees"][0], (r["x"], r["y"], r["cost"], r["parent"]), "moved-node problem")
    assert (out["paths"][0] is None) == (r["path"] is None)
    if r["path"] is not None:
        assert np.array_equal(out["paths"][0], r["path"])
    assert not (out["results"][2] & 16).any()   # no instance left as UNSUPPORTED


def test_gpu_kid_general_kernel_on_the_same_records(gpu, monkeypatch):
    """The scene of test_gpu_near_set_overflow_is_replanned_on_a_larger_shape: near sets outgrow the 44 candidate slots
    of the 64-thread shape, so the instances are planned again by the larger shapes, whose walks and child lists use the
    same records.  Trees equal the oracle's."""
    kw = dict(util.C2)
    kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15], expand_dis=3.0, path_resolution=0.5, max_iter=700,
              obstacles=DRV_OBSTACLES, robot_radius=0.8)
    _env(monkeypatch)
    seeds = list(range(1, 9))
    out, _, _ = _plan(kw, seeds)
    assert out["stats"]["near_unique_max"] > 44
    for i, s in enumerate(seeds):
        r = util.run_oracle(kw, s, exact_pow=True)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "seed %d" % s)

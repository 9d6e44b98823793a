"""GPU (-m gpu): the state a pass over the grid index keeps and leaves behind (rrt_04 iteration kernel, one-wave shape).
The pass's centres and thresholds are wave-uniform scalars, its reductions run on DPP operands, and what it carries from
centre to centre must come out exactly as when all of it sat in per-lane registers.  Every case pins trees, paths,
results, RNG state and the decision counters against the oracle bit for bit, with the index on from the first node
(RRTX_TPB=64 RRTX_GRID_MIN=0), for every number of further query sets a pass may serve (RRTX_SPEC2 = 0 .. 3) and for the
merged and the per-centre gather (RRTX_GRID_MERGE = 1, 0)."""
import functools

import numpy as np
import pytest

import graze_util as G
import test_gpu_grid_merge as gm
import util
from test_gpu_graze import _rng_equal

pytestmark = pytest.mark.gpu

ORACLE_COUNTERS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations")
COMBOS = [(s, m) for s in ("0", "1", "2", "3") for m in ("1", "0")]
ARENA_SEEDS = (1, 2, 3, 4, 5, 6)


def _freeze(kw):
    return tuple(sorted((k, tuple(map(tuple, v)) if k == "obstacles" else (tuple(v) if isinstance(v, list) else v))
                        for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _oracle_frozen(frozen, seed):
    """One oracle plan per (scene, seed): computed once, shared by the cases, never modified."""
    kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in frozen}
    return util.run_oracle(kw, seed, exact_pow=True)


def _refs(kw, seeds):
    return [_oracle_frozen(_freeze(kw), s) for s in seeds]


def _arena(max_iter=3000):
    """the 20 x 20 arena of test_gpu_graze.py: dense within ~100 nodes, so the index answers nearly every pass"""
    kw = dict(G._arena())
    kw["max_iter"] = max_iter
    return kw


def _c2_prefix(max_iter=3000):
    kw = util.c2_kwargs(max_iter)
    kw["obstacles"] = kw["obstacles"][:16]
    return kw


def _env(monkeypatch, spec2, merge, tpb="64", chunk=None):
    monkeypatch.setenv("RRTX_TPB", tpb)
    monkeypatch.setenv("RRTX_GRID_MIN", "0")
    monkeypatch.setenv("RRTX_SPEC2", spec2)
    monkeypatch.setenv("RRTX_GRID_MERGE", merge)
    monkeypatch.delenv("RRTX_GRID", raising=False)
    if chunk is None:
        monkeypatch.delenv("RRTX_CHUNK_ITERS", raising=False)
    else:
        monkeypatch.setenv("RRTX_CHUNK_ITERS", chunk)


def _equals_oracle(out, refs, what, shape=64):
    assert out["stats"]["main_shape"] == shape, what
    for i, r in enumerate(refs):
        w = "%s, instance %d" % (what, i)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), w)
        assert (out["paths"][i] is None) == (r["path"] is None), w
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"]), w
        assert _rng_equal(out["rng"][i], r["rng"]), w
        assert out["results"][1][i] == len(r["x"]), w   # n_nodes of the result record
        assert not (out["results"][2][i] & (4 | 16)), w   # no overflow, not left as UNSUPPORTED
    for k in ORACLE_COUNTERS:
        assert out["stats"][k] == sum(r["stats"][k] for r in refs), (what, k)


@pytest.mark.parametrize("spec2,merge", COMBOS)
def test_gpu_pass_state_arena_equals_oracle(gpu, monkeypatch, spec2, merge):
    """3 000 iterations, 6 seeds, the 20 x 20 arena.  Past ~1 100 nodes a near ball of this arena holds more than the 44
    candidates of the one-wave shape (50 at 1 200 nodes, counted on the oracle's trees), so these plans leave the shape
    with an overflow and are planned again on a larger one: the case pins the pass state up to that hand-over and the
    hand-over itself.  The 700-iteration case below stays on the one-wave shape to the end."""
    kw = _arena()
    _env(monkeypatch, spec2, merge)
    out = util.run_gpu_batch(kw, list(ARENA_SEEDS))
    print("replanned instances:", out["stats"]["replanned"], "passes_shared:", out["stats"]["passes_shared"])
    _equals_oracle(out, _refs(kw, ARENA_SEEDS), "arena RRTX_SPEC2=%s RRTX_GRID_MERGE=%s" % (spec2, merge))


@pytest.mark.parametrize("spec2,merge", COMBOS)
def test_gpu_pass_state_arena_one_wave_to_the_end(gpu, monkeypatch, spec2, merge):
    """The arena at 700 iterations: the largest near ball holds 32 distinct nodes (counted on the oracle's trees), so no
    instance leaves the one-wave shape, and from 256 nodes on iterations ride on earlier passes."""
    kw = _arena(700)
    _env(monkeypatch, spec2, merge)
    out = util.run_gpu_batch(kw, list(ARENA_SEEDS))
    _equals_oracle(out, _refs(kw, ARENA_SEEDS), "arena, 700 iterations, RRTX_SPEC2=%s RRTX_GRID_MERGE=%s" % (spec2, merge))
    assert out["stats"]["replanned"] == 0
    assert out["stats"]["near_unique_max"] <= 44
    if spec2 != "0":
        assert out["stats"]["passes_shared"] > 0
    else:
        assert out["stats"]["passes_shared"] == 0


@pytest.mark.parametrize("spec2,merge", COMBOS)
def test_gpu_pass_state_c2_prefix_equals_oracle(gpu, monkeypatch, spec2, merge):
    """A 16-circle prefix of the C2 map at 3 000 iterations."""
    kw = _c2_prefix()
    seeds = (1, 2, 3, 4)
    _env(monkeypatch, spec2, merge)
    out = util.run_gpu_batch(kw, list(seeds))
    _equals_oracle(out, _refs(kw, seeds), "C2 prefix RRTX_SPEC2=%s RRTX_GRID_MERGE=%s" % (spec2, merge))


@pytest.mark.parametrize("spec2,merge", COMBOS)
def test_gpu_pass_state_resumed_launches_equal_oracle(gpu, monkeypatch, spec2, merge):
    """The arena plan in launches of 97 iterations: whatever a pass parks outside the registers is rebuilt per launch."""
    kw = _arena()
    _env(monkeypatch, spec2, merge, chunk="97")
    out = util.run_gpu_batch(kw, list(ARENA_SEEDS))
    assert out["stats"]["launches"] >= 3000 // 97
    _equals_oracle(out, _refs(kw, ARENA_SEEDS), "arena in launches of 97, RRTX_SPEC2=%s RRTX_GRID_MERGE=%s" % (spec2, merge))


@pytest.mark.parametrize("spec2,merge", COMBOS)
def test_gpu_pass_state_moved_node_equals_oracle(gpu, monkeypatch, spec2, merge):
    """One moved-node problem (the first scene of test_gpu_grid_merge.py): rewire moves nodes between passes."""
    res, rate, scene, seed = 0.05, 60, "diag", 5
    kw = dict(util.C2)
    kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)])
    kw.update(expand_dis=3.0, path_resolution=res, goal_sample_rate=rate, connect_circle_dist=50.0, max_iter=1500,
              robot_radius=0.0)
    seeds = (seed, seed + 1000)
    _env(monkeypatch, spec2, merge)
    out = util.run_gpu_batch(kw, list(seeds))
    _equals_oracle(out, _refs(kw, seeds), "moved nodes RRTX_SPEC2=%s RRTX_GRID_MERGE=%s" % (spec2, merge))


@pytest.mark.parametrize("spec2,merge", COMBOS)
def test_gpu_pass_state_goal_cell_equals_oracle(gpu, monkeypatch, spec2, merge):
    """The goal-heavy plan of test_gpu_merge_speculative_sets_reach_goal_cell (two samples in five are the goal), at
    3 000 iterations: the speculated balls reach the goal's cell all the time."""
    kw = util.c2_kwargs(3000)
    kw["goal_sample_rate"] = 40
    seeds = (3, 4)
    _env(monkeypatch, spec2, merge)
    out = util.run_gpu_batch(kw, list(seeds))
    _equals_oracle(out, _refs(kw, seeds), "goal cell RRTX_SPEC2=%s RRTX_GRID_MERGE=%s" % (spec2, merge))


@pytest.mark.parametrize("spec2,merge", COMBOS)
def test_gpu_pass_state_reused_handle_changed_seeds(gpu, monkeypatch, spec2, merge):
    """Plan, change the seeds, plan again on the same handle: the second plan equals the oracle's for the new seeds."""
    import rrt_amd
    A = rrt_amd._abi
    kw = _arena(1500)
    s1, s2 = (1, 2, 3), (11, 12, 13)
    _env(monkeypatch, spec2, merge)
    h = A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                 kw["goal_sample_rate"], kw["max_iter"], play_area=kw["play_area"], robot_radius=kw["robot_radius"],
                 connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=kw["search_until_max_iter"],
                 n_instances=len(s1))
    try:
        h.set_obstacles(kw["obstacles"])
        outs = []
        for seeds in (s1, s2):
            h.seed_instances(list(seeds))
            h.plan(strict=True)
            n = len(seeds)
            outs.append(dict(stats=h.get_stats(), results=h.get_results(), trees=[h.get_tree(i) for i in range(n)],
                             paths=[h.get_path(i) for i in range(n)], rng=[h.get_rng_state(i) for i in range(n)]))
    finally:
        h.close()
    for out, seeds, what in zip(outs, (s1, s2), ("first plan", "second plan")):
        refs = _refs(kw, seeds)
        for i, r in enumerate(refs):
            w = "%s, instance %d, RRTX_SPEC2=%s RRTX_GRID_MERGE=%s" % (what, i, spec2, merge)
            util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), w)
            assert (out["paths"][i] is None) == (r["path"] is None), w
            if r["path"] is not None:
                assert np.array_equal(out["paths"][i], r["path"]), w
            assert _rng_equal(out["rng"][i], r["rng"]), w


def test_gpu_pass_state_merge_reads_the_same_bytes(gpu, monkeypatch):
    """The arena: algorithmic_bytes and scan_nodes are equal between the merged and the per-centre gather, and so is every
    decision counter (the helpers of test_gpu_grid_merge.py)."""
    kw = _arena()
    on = gm._run(monkeypatch, kw, list(ARENA_SEEDS), "1")
    off = gm._run(monkeypatch, kw, list(ARENA_SEEDS), "0")
    gm._same(on, off, "arena, RRTX_GRID_MERGE=1 vs 0", bytes_too=True)
    assert on["stats"]["algorithmic_bytes"] == off["stats"]["algorithmic_bytes"]
    assert on["stats"]["scan_nodes"] == off["stats"]["scan_nodes"]


@pytest.mark.parametrize("tpb", ["128", "256"])
def test_gpu_pass_state_other_shapes_equal_oracle(gpu, monkeypatch, tpb):
    """The 128- and the 256-thread shape share the kernel's source and the helpers' file: they still equal the oracle."""
    kw = _arena()
    _env(monkeypatch, "3", "1", tpb=tpb)
    out = util.run_gpu_batch(kw, list(ARENA_SEEDS))
    _equals_oracle(out, _refs(kw, ARENA_SEEDS), "arena RRTX_TPB=" + tpb, shape=int(tpb))

"""GPU (-m gpu): the tolerance-band verdicts of the rrt_04 iteration kernel and the rrt_07 kernel on forged grazing maps.

Both kernels decide almost every collision verdict from approximate points and hand a verdict to the exact form
(atan2 / cos / sin) only when a circle's threshold lies within a band of the closest distance**2.  The hand-over is
written in three places for rrt_04 -- the extension edge, the one-wave cull path, the pair loops with their redo pass --
and once for rrt_07 (test_candidates).  On the suite's random maps no pair ever enters the band (test_graze_host.py
counts zero), so these tests plan on maps forged by graze_util: tens to thousands of pairs inside the band per instance,
on both sides of the threshold, at every call site, on edges no other circle decides (the floors are checked on the CPU
by test_graze_host.py for exactly these scenes and seeds).  Every instance has its own map.  Trees, costs, parents, paths,
RNG state and the decision counters equal the oracle's bit for bit, under every kernel shape and knob that changes the
route a verdict takes."""
import numpy as np
import pytest

import graze_util as G
import util

pytestmark = pytest.mark.gpu

ORACLE_COUNTERS = ("edges_ref", "edges_unique", "near_hits", "near_unique", "rewires", "propagated", "iterations")


def _rng_equal(state, mt):
    return tuple(state[1][:624]) == tuple(mt.mt) and state[1][624] == mt.pos


@pytest.fixture(scope="module")
def forged():
    """scene -> (kw, seeds, maps, oracle runs): forged and planned on the CPU once, shared by the tests, never changed."""
    cache = {}

    def get(scene):
        if scene not in cache:
            if scene == "rrt_07":
                planner, (kw, seeds, total) = "informed", G.rrt07_scene()
            else:
                planner, (kw, seeds, total) = "rrt_star", G.rrt04_scenes()[scene]
            maps = [G.forge(planner, kw, s, total) for s in seeds]
            runs = [G.run(planner, kw, s, m, graze=False) for s, m in zip(seeds, maps)]
            cache[scene] = (kw, seeds, maps, runs)
        return cache[scene]
    return get


def _plan(algo, kw, seeds, maps):
    import rrt_amd
    if algo == "informed":
        bp = rrt_amd.BatchPlanner("informed", list(seeds), kw["start"], kw["goal"], None, kw["rand_area"],
                                  instance_obstacles=maps, expand_dis=kw["expand_dis"],
                                  goal_sample_rate=kw["goal_sample_rate"], max_iter=kw["max_iter"],
                                  sobol_sampler=bool(kw["sobol"]))
    else:
        bp = rrt_amd.BatchPlanner("rrt_star", list(seeds), kw["start"], kw["goal"], None, kw["rand_area"],
                                  instance_obstacles=maps, expand_dis=kw["expand_dis"],
                                  path_resolution=kw["path_resolution"], goal_sample_rate=kw["goal_sample_rate"],
                                  max_iter=kw["max_iter"], robot_radius=kw["robot_radius"],
                                  connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=True)
    try:
        bp.plan()
        n = len(seeds)
        return dict(trees=[bp.tree(i) for i in range(n)], paths=[bp.path(i) for i in range(n)],
                    rng=[bp.rng_state(i) for i in range(n)], stats=bp.stats())
    finally:
        bp.close()


def _equals_oracle(out, seeds, runs, what, counters=ORACLE_COUNTERS):
    for i, (s, r) in enumerate(zip(seeds, runs)):
        w = "%s, seed %d" % (what, s)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), w)
        p = out["paths"][i]
        assert (p is None) == (r["path"] is None), w
        if p is not None:
            assert np.array_equal(p if p.shape[1] == 2 else p[:, :2], r["path"]), w
        assert _rng_equal(out["rng"][i], r["rng"]), w
    for k in counters:
        assert out["stats"][k] == sum(r["stats"][k] for r in runs), (what, k)


def _equal_runs(a, b, what, counters):
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        util.assert_tree_equal(ta, tb, "%s, instance %d" % (what, i))
    for pa, pb in zip(a["paths"], b["paths"]):
        assert (pa is None) == (pb is None), what
        if pa is not None:
            assert np.array_equal(pa, pb), what
    assert a["rng"] == b["rng"], what
    for k in counters:
        assert a["stats"][k] == b["stats"][k], (what, k)


# (RRTX_TPB, RRTX_OBS_CULL): the one-wave shape with the cull path (one edge per lane, half-wave direction split) and
# with the pair loops, the two-wave and the four-wave shape (pair loops, direction per wave / per wave pair)
SHAPES = (("64", "1"), ("64", "0"), ("128", None), ("256", None))


@pytest.mark.parametrize("scene", ["arena", "arena_res03_rr02", "moved_nodes", "c2_prefix"])
def test_gpu_rrt04_grazing_maps_equal_oracle(gpu, monkeypatch, forged, scene):
    """Each scene of graze_util.rrt04_scenes() on every shape of the iteration kernel: equal to the oracle, and (hence,
    but the message is more useful) to each other."""
    kw, seeds, maps, runs = forged(scene)
    first = None
    for tpb, cull in SHAPES:
        monkeypatch.setenv("RRTX_TPB", tpb)
        if cull is None:
            monkeypatch.delenv("RRTX_OBS_CULL", raising=False)
        else:
            monkeypatch.setenv("RRTX_OBS_CULL", cull)
        what = "%s, RRTX_TPB=%s RRTX_OBS_CULL=%s" % (scene, tpb, cull)
        out = _plan("rrt_star", kw, seeds, maps)
        assert out["stats"]["main_shape"] == int(tpb), what
        _equals_oracle(out, seeds, runs, what)
        if first is None:
            first = out
        else:
            _equal_runs(out, first, what + " vs the first shape", ORACLE_COUNTERS)


def test_gpu_rrt04_grazing_map_of_200_circles_equals_oracle(gpu, monkeypatch, forged):
    """200 circles: more than the one- and two-wave tiles hold, the 256-thread shape with several circles per lane."""
    kw, seeds, maps, runs = forged("arena200")
    assert len(maps[0]) == 200
    monkeypatch.setenv("RRTX_TPB", "256")
    out = _plan("rrt_star", kw, seeds, maps)
    assert out["stats"]["main_shape"] == 256
    _equals_oracle(out, seeds, runs, "arena200")


def test_gpu_rrt04_grazing_maps_without_speculation_and_grid(gpu, monkeypatch, forged):
    """RRTX_SPEC2=0 and RRTX_GRID=0: every iteration streams its own pass and no extension edge is evaluated ahead of
    its turn -- the band verdicts arrive by the plain route, same trees and the same decisions as by the default one."""
    kw, seeds, maps, runs = forged("arena")
    monkeypatch.setenv("RRTX_TPB", "64")
    dflt = _plan("rrt_star", kw, seeds, maps)
    monkeypatch.setenv("RRTX_SPEC2", "0")
    monkeypatch.setenv("RRTX_GRID", "0")
    out = _plan("rrt_star", kw, seeds, maps)
    assert out["stats"]["main_shape"] == 64
    _equals_oracle(out, seeds, runs, "arena, RRTX_SPEC2=0 RRTX_GRID=0")
    _equal_runs(out, dflt, "arena, RRTX_SPEC2=0 RRTX_GRID=0 vs default", ORACLE_COUNTERS)


def test_gpu_rrt07_grazing_maps_equal_oracle(gpu, monkeypatch, forged):
    """rrt_07 on circles tangent to the segments candidate -> new node: the default route (band, then the exact end
    point for the candidates left in doubt), every verdict from the exact form (RRTX_INFORMED_EXACT_SEG=1) and every
    near candidate tested as the reference does (RRTX_INFORMED_EAGER=1): three times the oracle's trees."""
    kw, seeds, maps, runs = forged("rrt_07")
    # the device tests fewer segments than the reference unless told to be eager: edges_unique is its own count
    counters = ("edges_ref", "near_hits", "near_unique", "rewires", "iterations")
    dflt = _plan("informed", kw, seeds, maps)
    _equals_oracle(dflt, seeds, runs, "rrt_07 default", counters)
    for knob in ("RRTX_INFORMED_EXACT_SEG", "RRTX_INFORMED_EAGER"):
        monkeypatch.setenv(knob, "1")
        out = _plan("informed", kw, seeds, maps)
        monkeypatch.delenv(knob)
        _equals_oracle(out, seeds, runs, "rrt_07 %s=1" % knob, counters)
        _equal_runs(out, dflt, "rrt_07 %s=1 vs default" % knob, counters)

"""Host (-m "not gpu"): the forged grazing maps of tests/graze_util.py do what tests/test_gpu_graze.py relies on.

The GPU tests compare the kernels with the oracle on these maps; that says something about the tolerance-band hand-over
of the kernels only if the maps really put circles inside the band, on both sides of the threshold, at every call site
of the collision test, and on edges no other circle decides outright.  The oracle counts exactly that (grazing pairs,
rrt_oracle.c), so the floors below are checked here, on the CPU, for every scene and seed the GPU tests plan."""
import numpy as np
import pytest

import graze_util as G
import oracle

# per scene, summed over its seeds
FLOOR_IN = 20        # grazing pairs at or below the threshold (the pair collides)
FLOOR_OUT = 20       # grazing pairs above it
FLOOR_EXACT = 10     # edges with a grazing circle and no outright hit: the kernel MUST take the exact form
FLOOR_SITE = 3       # grazing pairs at each of: short extension edge, choose_parent, rewire
SITES = ("ext_short", "choose_parent", "rewire")


def _totals(planner, kw, seeds, total):
    tot = {}
    for s in seeds:
        r = G.run(planner, kw, s, G.forge(planner, kw, s, total))
        G.add_stats(tot, r["stats"])
    return G.graze_counts(tot)


def _check_floors(c, what):
    print(what, c)
    assert c["in"] >= FLOOR_IN, (what, c)
    assert c["out"] >= FLOOR_OUT, (what, c)
    assert c["exact"] >= FLOOR_EXACT, (what, c)
    for s in SITES:
        assert c[s] >= FLOOR_SITE, (what, s, c)


@pytest.mark.parametrize("scene", sorted(G.rrt04_scenes()))
def test_forged_rrt04_maps_meet_the_floors(scene):
    kw, seeds, total = G.rrt04_scenes()[scene]
    for s in seeds:
        obs = G.forge("rrt_star", kw, s, total)
        assert len(obs) == total and obs[:len(kw["obstacles"])] == [tuple(map(float, o)) for o in kw["obstacles"]]
    _check_floors(_totals("rrt_star", kw, seeds, total), scene)


def test_forged_rrt07_maps_meet_the_floors():
    kw, seeds, total = G.rrt07_scene()
    for s in seeds:
        assert len(G.forge("informed", kw, s, total)) == total
    _check_floors(_totals("informed", kw, seeds, total), "rrt_07")


def test_unforged_maps_count_no_grazing_pair():
    """What the suite had before: on the scenes' own maps (and the full C2 map) no pair comes near the band."""
    import util
    runs = [("rrt_star", kw, s) for kw, seeds, _ in G.rrt04_scenes().values() for s in seeds]
    runs += [("rrt_star", util.c2_kwargs(1500), s) for s in (1, 2)]
    kw7, seeds7, _ = G.rrt07_scene()
    runs += [("informed", kw7, s) for s in seeds7]
    for planner, kw, s in runs:
        r = G.run(planner, kw, s, kw["obstacles"])
        assert all(r["stats"][k] == 0 for k in G.GRAZE_KEYS), (planner, s, G.graze_counts(r["stats"]))


def test_counters_are_off_by_default_and_change_no_result():
    kw, seeds, total = G.rrt04_scenes()["arena"]
    obs = G.forge("rrt_star", kw, seeds[0], total)
    on = G.run("rrt_star", kw, seeds[0], obs, graze=True, edge_log=True)
    off = G.run("rrt_star", kw, seeds[0], obs, graze=False)
    assert all(off["stats"][k] == 0 for k in G.GRAZE_KEYS) and "edges" not in off
    for k in ("x", "y", "cost", "parent"):
        assert np.array_equal(on[k], off[k]), k
    assert tuple(on["rng"].mt) == tuple(off["rng"].mt) and on["rng"].pos == off["rng"].pos
    for k, _ in oracle.Stats._fields_:
        if k not in G.GRAZE_KEYS:
            assert on["stats"][k] == off["stats"][k], k
    # one log row per collision test the reference makes, grazing circles per row = the pair counters
    assert len(on["edges"]) == on["stats"]["edges_ref"]
    c = G.graze_counts(on["stats"])
    assert int(on["edges"][:, 9].sum()) == c["in"] + c["out"]


def test_pair_classification_on_a_hand_made_edge():
    """One edge, one circle: start (0, 0) -> goal sample (1, 0), resolution 0.25, circle centre straight above the point
    (0.5, 0) at height h, size 0.5.  Closest distance**2 is h**2, threshold 0.25,
    tol = 1e-10 (1 + 0 + 0 + 0.5 + h) (4 + 0.25) ~ 8.5e-10: h = 0.5 and 0.5 (1 +- 1e-10) graze (dmin - thr ~ 1e-10),
    h = 0.5 (1 +- 1e-8) do not (1e-8 > tol / 2); below 0.5 is "in", above is "out"."""
    kw = dict(algo="rrt_star", start=[0, 0], goal=[1, 0], rand_area=[0, 1], expand_dis=2.0, path_resolution=0.25,
              goal_sample_rate=100, max_iter=1, search_until_max_iter=True)
    want = {0.5: ("in", 1), 0.5 * (1 - 1e-10): ("in", 1), 0.5 * (1 + 1e-10): ("out", 1), 0.5 * (1 - 1e-8): ("in", 0),
            0.5 * (1 + 1e-8): ("out", 0)}
    for h, (side, n) in want.items():
        r = oracle.plan(seed=1, graze=True, obstacles=[(0.5, h, 0.5)], **kw)
        st = r["stats"]
        other = "out" if side == "in" else "in"
        # the extension edge, and the same polyline once more as the edge start -> goal of search_best_goal_node
        for site in ("ext_short", "goal"):
            assert st["graze_%s_%s" % (side, site)] == n and st["graze_%s_%s" % (other, site)] == 0, (h, site, st)
            assert st["graze_exact_%s" % site] == n, (h, site, st)
        # a free extension edge becomes a node: choose_parent walks start -> node, rewire the same points backwards
        for site in ("choose_parent", "rewire"):
            assert st["graze_out_%s" % site] == (n if side == "out" else 0) and st["graze_in_%s" % site] == 0, (h, site, st)
        assert st["graze_in_ext_long"] == 0 and st["graze_out_ext_long"] == 0
        assert len(r["x"]) == (1 if side == "in" else 2), h          # the verdict itself: "in" collides


def test_forger_is_reproducible():
    kw, seeds, total = G.rrt04_scenes()["moved_nodes"]
    a = G.forge("rrt_star", kw, seeds[1], total)
    kw7, seeds7, total7 = G.rrt07_scene()
    a7 = G.forge("informed", kw7, seeds7[1], total7)
    G._forge.cache_clear()
    assert G.forge("rrt_star", kw, seeds[1], total) == a
    assert G.forge("informed", kw7, seeds7[1], total7) == a7

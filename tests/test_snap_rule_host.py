"""CPU: the ground tests/test_gpu_fine_resolution.py stands on.

1. The oracle reproduces the reference's goldens at path_resolution 0.001 and at rand_area [1000, 1100] (the fineres_*
   files of tools/gen_golden_fine_resolution.py) bit for bit: tree, path, check_collision count, RNG state, trace.  Until
   these the oracle was pinned to the reference at resolutions of 0.05 and more, on maps at the origin, only.
2. Conditions on the GPU scenes (on the inputs, not measurements of the kernel): every seed of the "fine" scene holds at
   least 3 edges which the snap rule the kernel had before (1e-9 res, fixed: snap_util.rule_parent) calls certainly snapped
   and the oracle's exact steer does not snap, over the seeds at least one at choose_parent and one at rewire; the rule in
   rpp_core.h (snap_util.rule_new) misjudges none, in any scene; the goldens are these scenes; the moved-nodes scene moves
   nodes.
"""
import os

import numpy as np
import pytest

import snap_util as S
import util

GOLDENS = {"fineres_rrt04_s5": ("fine", 5), "fineres_rrt04_s7": ("fine", 7), "fineres_rrt01_s5": ("fine_rrt", 5),
           "fineres_rrt04_off1000_s6": ("offset_1000", 6)}


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_oracle_matches_reference_golden_at_fine_resolution(name):
    g = util.load_golden(os.path.join(util.GOLDEN, name + ".npz"))
    kw = util.kwargs_from_golden(g)
    scene, seed = GOLDENS[name]
    want = S.SCENES[scene][0]
    assert int(g["seed"]) == seed and all(kw[k] == (want[k] if k != "obstacles" else [tuple(o) for o in want[k]])
                                          for k in kw if k != "play_area"), "the golden is not the scene the GPU plans"
    assert kw["path_resolution"] == (0.01 if "off1000" in name else 0.001) and kw["max_iter"] == 300
    r = util.run_oracle(kw, seed, exact_pow=True, trace=True)
    util.assert_tree_equal((r["x"], r["y"], r["cost"], r["parent"]),
                           (g["x"], g["y"], g["cost"] if kw["algo"] == "rrt_star" else None, g["parent"]), name)
    assert len(g["path"]) > 0 and r["path"] is not None and np.array_equal(r["path"], g["path"])
    assert r["stats"]["edges_ref"] == int(g["ref_edges"])
    assert r["rng"].pos == int(g["rng_pos_after"]) and r["rng"].mt[0] == int(g["rng_word0_after"])
    n = len(g["tr_nearest"])
    assert n > 0 and np.array_equal(r["tr_nearest"][:n], g["tr_nearest"])
    assert np.array_equal(r["tr_rnd_x"][:n], g["tr_rnd_x"]) and np.array_equal(r["tr_rnd_y"][:n], g["tr_rnd_y"])


@pytest.mark.parametrize("scene", sorted(S.SCENES))
def test_scene_conditions(scene):
    kw, seeds, parent_condition = S.SCENES[scene]
    assert kw["max_iter"] <= 300 and 2 <= len(seeds) <= 3
    at_choose = at_rewire = 0
    for s in seeds:
        old, new, r = S.count(kw, s)
        print("%s seed %d: the parent's rule misjudges %r, the new rule %r (site -> edges), %d nodes" % (scene, s, old, new, len(r["x"])))
        assert sum(new.values()) == 0, (scene, s, new)
        assert r["path"] is not None and len(r["x"]) >= 100
        if parent_condition:
            assert sum(old.values()) >= 3, (scene, s, old)
        at_choose += old[S.S_CHOOSE]
        at_rewire += old[S.S_REWIRE]
    if parent_condition:
        assert at_choose >= 1 and at_rewire >= 1
    if scene == "moved":
        for s in seeds:
            assert S.moved_nodes(kw, s) >= 10, s


def test_the_rules_differ_only_by_the_slack():
    """rule_new is rule_parent less a slack that vanishes with n and the coordinates: at the origin with n = 0 they agree,
    and what rule_new calls certain rule_parent calls certain too."""
    rng = np.random.default_rng(3)
    for _ in range(20000):
        res = float(rng.choice([0.25, 0.05, 0.001]))
        fx, fy = (float(v) for v in rng.uniform(-1e4, 1e4, 2))
        d = float(rng.uniform(0, 3000 * res))
        th = float(rng.uniform(-np.pi, np.pi))
        tx, ty = fx + d * np.cos(th), fy + d * np.sin(th)
        ne = int(np.floor(d / res))
        if S.rule_new(d, ne, res, fx, fy, tx, ty):
            assert S.rule_parent(d, ne, res)
    assert S.rule_new(0.1, 0, 0.25, 0.0, 0.0, 0.1, 0.0) and not S.rule_new(0.25 * (1 - 1e-10), 0, 0.25, 0.0, 0.0, 0.25, 0.0)

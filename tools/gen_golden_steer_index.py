"""Golden generator of the obstacle index of BatchSteer: curves among 1 000 circles, where the check goes through
the index.  Runs the reference's stand-alone curve functions (plan_dubins_path, reeds_shepp_path_planning) and the reference's
own check_collision (rrt_05 :1625-1638 for Dubins rows, rrt_06 :1749-1762 for Reeds-Shepp rows, each cross-checked against the
other), all loaded through oracle/ref_loader.py as tools/gen_golden_steer_collide.py does, and writes
tests/golden/steer_index_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_steer_index.py

Inputs and `hit` only: ob (1000, 3) = util.synth_map(13, 1000, 0.3, 0.9), rr = 0.1, d_inp (300, 7) = (sx, sy, syaw, gx, gy,
gyaw, curvature), r_inp (300, 8) = (..., curvature, step_size), d_hit / r_hit (300,) int32: -1 check_collision returns True,
j >= 0 the shortest prefix ob[:j + 1] at which it returns False, -2 the reference has no curve.  Starts lie in [5, 95]^2, the
goal 0.5 .. 4 units away; curvature 1, Reeds-Shepp step 0.2; random.Random(21) draws the Dubins rows, (22) the others."""
import math
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_steer_collide as G  # noqa: E402  (the loader set-up, the curve functions and the two check_collision copies)
import util  # noqa: E402

RR = 0.1


def first_refused(g, kind, xy, obs):
    """The shortest prefix of obs the reference refuses, by bisection: check_collision walks the list in order and returns
    False at the first circle that holds a point, so "obs[:j] is refused" is monotone in j.  Both ends are checked."""
    node = types.SimpleNamespace(path_x=xy[0], path_y=xy[1])
    lo, hi = 0, len(obs)          # obs[:lo] accepted, obs[:hi] refused
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if g.chk[kind](node, obs[:mid], RR):
            lo = mid
        else:
            hi = mid
    assert g.chk[kind](node, obs[:hi - 1], RR) and not g.chk[kind](node, obs[:hi], RR)
    return hi - 1


def row(rng):
    sx, sy, syaw = rng.uniform(5, 95), rng.uniform(5, 95), rng.uniform(-math.pi, math.pi)
    d, a = rng.uniform(0.5, 4.0), rng.uniform(-math.pi, math.pi)
    return sx, sy, syaw, sx + d * math.cos(a), sy + d * math.sin(a), rng.uniform(-math.pi, math.pi), 1.0


def main():
    g = G.Gen()
    obs = [tuple(float(v) for v in o) for o in util.synth_map(13, 1000, 0.3, 0.9)]
    out = {"ob": np.array(obs), "rr": np.float64(RR)}
    for kind, seed in (("d", 21), ("r", 22)):
        rng = random.Random(seed)
        inps, hits = [], []
        for _ in range(300):
            inp = row(rng) + ((0.2,) if kind == "r" else ())
            xy = g.curve(kind, inp)
            if xy is None:
                h = -2
            elif g.free(kind, xy, obs, RR):
                h = -1
            else:
                h = first_refused(g, kind, xy, obs)
            inps.append(inp)
            hits.append(h)
        hits = np.array(hits, dtype=np.int32)
        print("%s: %d free, %d blocked, %d without a curve, highest hit %d" %
              (kind, np.sum(hits == -1), np.sum(hits >= 0), np.sum(hits == -2), hits.max()))
        assert np.sum(hits == -1) >= 100 and np.sum(hits >= 0) >= 100
        out[kind + "_inp"] = np.array(inps, dtype=np.float64)
        out[kind + "_hit"] = hits
    np.savez_compressed(os.path.join(G.GOLD, "steer_index_kat.npz"), **out)


if __name__ == "__main__":
    main()

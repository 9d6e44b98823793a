"""The libm-free snap decision of the rrt_04 iteration kernel (rpp::snap_certain) restated in Python, the
scenes that put it to the test, and a counter of the edges of an oracle run that a rule gets wrong.

steer() ends ON its target when, after n = floor(d / res) sequential additions of res (cos theta, sin theta), the target is
within res of the walk's end.  The kernel answers "certainly snapped" from d - n res alone wherever that is safely below
res and hands the rest to the exact form.  A rule MISJUDGES an edge when it answers "certainly snapped" and the oracle's
exact steer does not snap: the kernel then puts a node onto the target which the reference leaves at the walk's end.

  rule_parent   d - n res <= res (1 - 1e-9): the margin the kernel had before, fixed and relative to res alone.  Kept here
                as history; it is what the scenes below were chosen against.
  rule_new      the same less (2 n M + 16 d) 2^-52, M = |fx| + |fy| + |tx| + |ty| -- csrc/rpp_core.h, term for term.

Pure Python plus the oracle; every float operation is a single IEEE operation in the order the C++ has them.
"""
import ctypes as C
import math
import random

import numpy as np

import oracle
import util

S_EXT_SHORT, S_EXT_LONG, S_CHOOSE, S_REWIRE, S_GOAL = range(5)
ONE_MINUS = 1.0 - 1e-9          # the parent's margin


def rule_parent(d, ne, res, fx=0.0, fy=0.0, tx=0.0, ty=0.0):
    return d - float(ne) * res <= res * ONE_MINUS


def rule_new(d, ne, res, fx, fy, tx, ty):
    m = abs(fx) + abs(fy) + abs(tx) + abs(ty)
    slack = (2.0 * float(ne) * m + 16.0 * d) * 2.0 ** -52
    return d - float(ne) * res <= res * ONE_MINUS - slack


_steer = None


def exact_steer(fx, fy, tx, ty, extend, res):
    """(points, snapped) of the oracle's steer (rrt_04:1086-1115) for one edge."""
    global _steer
    if _steer is None:
        L = oracle.lib()
        L.orc_steer_polyline.restype = C.c_int
        L.orc_steer_polyline.argtypes = [C.c_double] * 6 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _steer = L.orc_steer_polyline
    end = np.zeros(2)
    sn = C.c_int(0)
    n = _steer(fx, fy, tx, ty, extend, res, end.ctypes.data, end.ctypes.data, 0, end.ctypes.data, C.byref(sn))
    return n, sn.value


def misjudged(edges, res, rule):
    """site -> number of edge-log rows that `rule` calls certainly snapped and the oracle's exact steer does not snap (or
    walks another number of steps).  The rows the kernel puts the question to: the extension edge when the nearest node is
    within expand_dis (a longer one always takes the exact form), every choose_parent and every rewire edge."""
    out = {S_EXT_SHORT: 0, S_CHOOSE: 0, S_REWIRE: 0}
    for row in edges:
        site = int(row[0])
        if site not in out:
            continue
        fx, fy, tx, ty, ext = (float(v) for v in row[2:7])
        d = math.hypot(tx - fx, ty - fy)
        if not d <= ext:
            continue
        ne = int(math.floor(d / res))
        if not rule(d, ne, res, fx, fy, tx, ty):
            continue
        n, snapped = exact_steer(fx, fy, tx, ty, ext, res)
        assert n == int(row[7])
        if not (snapped == 1 and n == ne + 2):
            out[site] += 1
    return out


def count(kw, seed):
    """(misjudged by the parent's rule, misjudged by the new rule, the oracle run) for one seed of a scene."""
    r = oracle.plan(seed=seed, edge_log=True, **kw)
    res = kw["path_resolution"]
    return misjudged(r["edges"], res, rule_parent), misjudged(r["edges"], res, rule_new), r


# ---- scenes: tests/test_snap_rule_host.py checks their conditions on the CPU, tests/test_gpu_fine_resolution.py plans them
def circles(lo, n=20, rmin=2.0, rmax=5.0, map_seed=3, keep_clear=()):
    """n circles of radius rmin..rmax in the 100 x 100 square whose lower corner is (lo, lo), from a private Random;
    none within 3 of a point of keep_clear."""
    rng = random.Random(map_seed)
    obs = []
    while len(obs) < n:
        x, y, r = lo + rng.uniform(0, 100), lo + rng.uniform(0, 100), rng.uniform(rmin, rmax)
        if all(math.hypot(x - px, y - py) > r + 3.0 for px, py in keep_clear):
            obs.append((x, y, r))
    return obs


def fine_scene(lo=0.0, res=0.001, algo="rrt_star", max_iter=300):
    """100 x 100 map at (lo, lo), 20 circles, expand_dis 3.0: an extension walks up to 3 / res steps, and the edge back from
    the nearest node is 3.0 give or take the walk's drift -- at the snap limit, where the rule has to know its own reach."""
    kw = dict(util.C2)
    start, goal = [lo + 5.0, lo + 5.0], [lo + 90.0, lo + 90.0]
    kw.update(algo=algo, start=start, goal=goal, rand_area=[lo, lo + 100.0], expand_dis=3.0, path_resolution=res,
              goal_sample_rate=5, connect_circle_dist=50.0, max_iter=max_iter, search_until_max_iter=1,
              obstacles=circles(lo, keep_clear=(start, goal)))
    if algo == "rrt":
        kw["search_until_max_iter"] = 0
    return kw


def moved_scene(res=0.002, max_iter=300):
    """Small area, goal sampled 60 % of the time (tests/test_gpu_obstacle_map.py's moved-nodes scene): rewire moves nodes,
    and the back edges are evaluated again from the winner's end point -- under the snap rule at res = 0.002.  Few seeds
    move a node within 300 iterations (23 of the first 400); SCENES names three that do, dozens of times each."""
    kw = dict(util.C2)
    kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], expand_dis=3.0, path_resolution=res, goal_sample_rate=60,
              connect_circle_dist=50.0, max_iter=max_iter, robot_radius=0.0, obstacles=[(3.0, 3.0, 1.0)])
    return kw


def moved_nodes(kw, seed):
    """How many times rewire MOVED a node (its steer ended short of the node it rewired) in one oracle run."""
    L = oracle.lib()
    m0, r0, m1, r1 = C.c_long(), C.c_long(), C.c_long(), C.c_long()
    L.orc_moved_counters(C.byref(m0), C.byref(r0))
    util.run_oracle(kw, seed)
    L.orc_moved_counters(C.byref(m1), C.byref(r1))
    return m1.value - m0.value


FINE_SEEDS = (5, 6, 7)
SCENES = {
    # name: (kw, seeds, the counter condition of the parent's rule applies)
    "fine": (fine_scene(), FINE_SEEDS, True),
    "fine_rrt": (fine_scene(algo="rrt"), FINE_SEEDS, False),
    "offset_1000": (fine_scene(lo=1000.0, res=0.01), (5, 6), False),
    "offset_-10100": (fine_scene(lo=-10100.0, res=0.01), (5, 6), False),
    "moved": (moved_scene(), (53, 66, 130), False),
}

"""Shared by tests/test_armnav_host.py and tests/test_gpu_armnav.py -- TEST INFRASTRUCTURE: the known-answer file of
BatchArmNav (tools/gen_golden_armnav.py) and the oracle's answers, each computed once and never written."""
import os

import numpy as np

import armnav_oracle
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
TAGS = ("driver", "same", "goal_on_obstacle", "start_on_obstacle", "walled", "wrap_i", "wrap_j", "wrap_both", "random")
DRIVER_LINKS = [0.5, 0.5, 0.3, 0.5, 0.1]
DRIVER_OBSTACLES = [[1.75, 0.75, 0.6], [0.55, 1.5, 0.5], [0, -1, 0.7], [0, -0.6, 0.4], [-1, 1., 0.3]]
DRIVER_QUERY = ((10, 50), (58, 56))
_cache = {}


def kat():
    """tests/golden/armnav_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "armnav_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def n_scenes():
    return len(kat()["scene_M"])


def scene_M(s):
    return int(kat()["scene_M"][s])


def scene_grid(s):
    """(M, M) uint8, read-only"""
    g = kat()
    M = scene_M(s)
    a = g["grids"][g["grid_off"][s]:g["grid_off"][s + 1]].reshape(M, M)
    a.setflags(write=False)
    return a


def scene_arm(s):
    """(link lengths, circles as rows x, y, radius) of an arm scene"""
    g = kat()
    return (g["link_len"][g["link_off"][s]:g["link_off"][s + 1]].tolist(),
            g["obs_xyr"][g["obs_off"][s]:g["obs_off"][s + 1]].reshape(-1, 3).tolist())


def scenes_of(M, kind=None):
    g = kat()
    return [s for s in range(n_scenes()) if scene_M(s) == M and (kind is None or g["scene_kind"][s] == kind)]


def all_M():
    return sorted(set(kat()["scene_M"].tolist()))


def queries_of(M):
    g = kat()
    return [q for q in range(len(g["q_scene"])) if scene_M(int(g["q_scene"][q])) == M]


def query(q):
    """dict(scene, start, goal, tag, pops, route as a list of tuples, marks (M, M) or None)"""
    g = kat()
    s = int(g["q_scene"][q])
    M = scene_M(s)
    off = int(g["q_marks_off"][q])
    r = g["route_ij"][g["route_off"][q]:g["route_off"][q + 1]]
    return dict(scene=s, M=M, start=tuple(g["q_start"][q].tolist()), goal=tuple(g["q_goal"][q].tolist()), tag=TAGS[g["q_tag"][q]],
                pops=int(g["q_pops"][q]), route=[tuple(c) for c in r.tolist()],
                marks=None if off < 0 else g["marks"][off:off + M * M].reshape(M, M))


def heuristic_cases():
    """[(M, goal, (M, M) map)]"""
    g = kat()
    return [(int(g["h_M"][k]), tuple(g["h_goal"][k].tolist()), g["h_flat"][g["h_off"][k]:g["h_off"][k + 1]].reshape(int(g["h_M"][k]), -1))
            for k in range(len(g["h_M"]))]


def heuristic_phases(M, goal):
    """calc_heuristic_map by whole-array steps (the drop-in module's).  tests/test_armnav_host.py holds it against the oracle's
    loop; the sweeps use it because the loop costs M * M interpreter steps per goal."""
    import rrt_amd.arm_obstacle_navigation as an
    return an.calc_heuristic_map(M, goal)


def oracle_search(grid, start, goal):
    """armnav_oracle.search with the heuristic by phases: (route, marks as (M, M) uint8, pops)"""
    M = len(grid)
    key = ("h", M, tuple(goal))
    if key not in _cache:
        _cache[key] = heuristic_phases(M, goal)
    route, marks, pops = armnav_oracle.search(grid, start, goal, h=_cache[key])
    return route, np.array(marks, dtype=np.uint8), pops


def oracle_query(q):
    """The oracle's answer to golden query q, with its own loop heuristic"""
    key = ("oq", q)
    if key not in _cache:
        c = query(q)
        route, marks, pops = armnav_oracle.search(scene_grid(c["scene"]), c["start"], c["goal"])
        _cache[key] = (route, np.array(marks, dtype=np.uint8), pops)
    return _cache[key]


def cycled(M, n, shift=0):
    """n golden queries of one M: its queries in turn from number `shift` on, round and round"""
    qs = queries_of(M)
    return [qs[(shift + k) % len(qs)] for k in range(n)]

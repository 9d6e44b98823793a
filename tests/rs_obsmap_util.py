"""Shared by the tests of the obstacle map under the Reeds-Shepp planners (rrt_06 / rrt_10) and by
tools/gen_golden_rs_obstacle_map.py: the scenes, one oracle plan per (problem, seed), and the comparisons."""
import math
import random

import numpy as np

START, GOAL, RAND_AREA = [0.0, 0.0, 0.0], [6.0, 9.0, math.pi / 2], [-2, 20]
MAX_ITER, CCD, MAP_SEED, SEEDS = 150, 50.0, 13, list(range(8))
# m -> (rmin, rmax, robot_radius): the radii shrink with the count, so the plans stay possible
SCENES = {65: (0.1, 0.4, 0.1), 300: (0.03, 0.12, 0.05), 1000: (0.01, 0.05, 0.03), 5000: (0.002, 0.01, 0.01)}
# nodes of the oracle's tree per seed 0..7, and of the same runs with no circle
NODES = {65: [18, 22, 37, 7, 33, 24, 8, 32], 300: [15, 23, 30, 36, 36, 27, 15, 27], 1000: [19, 6, 25, 25, 34, 34, 25, 46],
         5000: [26, 47, 47, 54, 42, 47, 64, 69], 0: [47, 49, 57, 63, 57, 55, 91, 92]}
FOUND = {65: 6, 300: 8, 1000: 7, 5000: 8}
# the closed-loop goldens (tools/gen_golden_rs_obstacle_map.py): rrt_10 on the 300-circle scene
CL_MAX_ITER = 40

_cache = {}


def scene(seed, m, rmin, rmax):
    """m circles: x, y uniform in [-2, 20], r uniform in [rmin, rmax], kept when more than r + 1.5 from start and goal."""
    rng = random.Random(seed)
    out = []
    while len(out) < m:
        x, y, r = rng.uniform(-2, 20), rng.uniform(-2, 20), rng.uniform(rmin, rmax)
        if all(math.hypot(x - px, y - py) > r + 1.5 for px, py in ((0.0, 0.0), (6.0, 9.0))):
            out.append((x, y, r))
    return out


def problem(m, **upd):
    """The plan of one scene as keywords of oracle.plan_rrt_rs (and of plan() below)."""
    if m:
        rmin, rmax, rr = SCENES[m]
        obstacles = scene(MAP_SEED, m, rmin, rmax)
    else:
        obstacles, rr = [], 0.0
    kw = dict(start=START, goal=GOAL, obstacles=obstacles, rand_area=RAND_AREA, max_iter=MAX_ITER, curvature=1.0,
              robot_radius=rr, expand_dis=3.0, connect_circle_dist=CCD, step_size=0.2)
    kw.update(upd)
    return kw


def oracle(kw, seed):
    """One oracle plan per (problem, seed), computed once and left unchanged."""
    import oracle as orc
    key = (repr(sorted((k, v) for k, v in kw.items() if k != "obstacles")), len(kw["obstacles"]),
           hash(tuple(map(tuple, kw["obstacles"]))), seed)
    if key not in _cache:
        k2 = dict(kw)
        _cache[key] = orc.plan_rrt_rs(k2.pop("start"), k2.pop("goal"), k2.pop("obstacles"), k2.pop("rand_area"),
                                      k2.pop("max_iter"), seed=seed, **k2)
    return _cache[key]


def make_handle(kw, n, device=0):
    import rrt_amd
    A = rrt_amd._abi
    return A.Handle(A.ALGO_RS, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], 0.5, 10, kw["max_iter"],
                    robot_radius=kw["robot_radius"], connect_circle_dist=kw["connect_circle_dist"],
                    search_until_max_iter=True, n_instances=n, device=device, curvature=kw["curvature"],
                    goal_yaw_th=float(np.deg2rad(1.0)), goal_xy_th=0.5, step_size=kw["step_size"])


def read(h, n):
    import util
    return util.read_planned(h, n, yaws=True, polys=True, path_yaws=True)


def plan(kw, seeds, use_map=True, starts=None, goals=None):
    """The trees of `seeds` on the GPU through the C ABI; with the map, `info` is the map's header."""
    h = make_handle(kw, len(seeds))
    try:
        (h.set_obstacle_map if use_map else h.set_obstacles)(kw["obstacles"])
        h.seed_instances(seeds)
        for i in range(len(seeds) if starts is not None else 0):
            h.set_instance(i, starts[i], goals[i])
        h.plan(strict=True)
        out = read(h, len(seeds))
        if use_map:
            out["info"] = h.obstacle_map_info()
    finally:
        h.close()
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b, what):
    """Two GPU results: trees, yaws, polylines, paths, results and RNG state, bit for bit."""
    import util
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        util.assert_tree_equal(ta, tb, "%s, instance %d" % (what, i))
        assert np.array_equal(bits(a["yaws"][i]), bits(b["yaws"][i])), what
        for pa, pb in zip(a["polys"][i], b["polys"][i]):
            assert np.array_equal(pa, pb), what
        assert (a["paths"][i] is None) == (b["paths"][i] is None), what
        if a["paths"][i] is not None:
            assert np.array_equal(a["paths"][i], b["paths"][i]) and np.array_equal(a["path_yaws"][i], b["path_yaws"][i]), what
    for ra, rb in zip(a["results"], b["results"]):
        assert np.array_equal(ra, rb), what
    assert a["rng"] == b["rng"], what


def equals_oracle(kw, seeds, out, what, starts=None, goals=None):
    """x, y, yaw, cost, parent, polylines, path and RNG state of every instance against the oracle, bit for bit; returns
    the node counts."""
    import util
    nodes = []
    for i, s in enumerate(seeds):
        r = oracle(kw if starts is None else dict(kw, start=starts[i], goal=goals[i]), s)
        w = "%s, seed %d" % (what, s)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), w)
        assert np.array_equal(bits(out["yaws"][i]), bits(r["yaw"])), w
        plen, px, py = out["polys"][i]
        assert np.array_equal(plen, r["poly_len"]) and np.array_equal(bits(px), bits(r["poly_x"])), w
        assert np.array_equal(bits(py), bits(r["poly_y"])), w
        assert (out["paths"][i] is None) == (r["path"] is None), w
        if r["path"] is not None:
            assert np.array_equal(out["paths"][i], r["path"]) and np.array_equal(out["path_yaws"][i], r["path_yaw"]), w
        assert out["results"][1][i] == len(r["x"]) and bool(out["results"][2][i] & 2) == (r["path"] is not None), w
        assert out["rng"][i][1] == tuple(int(v) for v in r["rng"].mt) + (int(r["rng"].pos),), w
        nodes.append(len(r["x"]))
    return nodes


def differs(ra, rb):
    """Two oracle results hold different trees."""
    return len(ra["x"]) != len(rb["x"]) or not (np.array_equal(ra["x"], rb["x"]) and np.array_equal(ra["y"], rb["y"])
                                                and np.array_equal(ra["parent"], rb["parent"]))

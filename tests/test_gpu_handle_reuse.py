"""GPU (-m gpu): ONE handle, many plans, CHANGED inputs between them -- every planner kernel.

rrtx.h promises that every plan starts from the staged per-instance state and from nothing else.  A second plan on the
same inputs cannot check that: whatever the first plan left behind is then the right state.  Here every plan of a sequence
differs from the one before it for every instance (other seeds, another map, another table size, per-instance lists,
moved starts and goals, a continued random stream, another launch bound), at least one plan leaves every tree shorter
than before (a stale tail in every array) and one longer, and every instance of every plan is compared with the CPU
oracle run on exactly the inputs staged for that plan: integers and doubles bit for bit, the RNG state word for word.
A fresh handle planned once on the same inputs is a second check, for what the oracle does not produce only (the
integer counters of rrtx_stats, main_shape, replanned, launches).

Sections: A sequences per planner, B re-plans inside a plan followed by other plans, C BatchPlanner over several
handles, D the call-order contract of rrtx.h.  A test stops at the first unexpected return code: the wrappers raise,
the handle is closed, nothing further is launched on it."""
import ctypes as C
import math
import random
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import rrt_amd
import util
from rrt_amd import _abi

pytestmark = pytest.mark.gpu

DRV = [(5.0, 5.0, 1.0), (3.0, 6.0, 2.0), (3.0, 8.0, 2.0), (3.0, 10.0, 2.0), (7.0, 5.0, 2.0), (9.0, 5.0, 2.0), (8.0, 10.0, 1.0)]
BIT_OBS = [(5.0, 5.0, 0.5), (9.0, 6.0, 1.0), (7.0, 5.0, 1.0), (1.0, 5.0, 1.0), (3.0, 6.0, 1.0), (7.0, 9.0, 1.0)]
TIMES = ("kernel_ms", "plan_ms", "kernel_ms_main")            # the only rrtx_stats fields that are not integers
ORACLE_COUNTERS = ("edges_ref", "near_hits", "near_unique", "rewires", "propagated", "iterations")
ONE_LAUNCH = 1 << 20
N = 8
E_STATE, E_CAPACITY = (next(k for k, v in _abi.ERRORS.items() if v == n) for n in ("RRTX_E_STATE", "RRTX_E_CAPACITY"))


# ------------------------------------------------------------------------------------------------ inputs
def _clear(pt, obs, margin):
    return all((pt[0] - ox) ** 2 + (pt[1] - oy) ** 2 > (r + margin) ** 2 for ox, oy, r in obs)


def _free_map(seed, m, lo, hi, rmin, rmax, keep, margin):
    """m circles in [lo, hi]^2, none within `margin` of a point of `keep` (starts and goals stay in free space)."""
    rng = random.Random(seed)
    obs = []
    while len(obs) < m:
        o = (rng.uniform(lo, hi), rng.uniform(lo, hi), rng.uniform(rmin, rmax))
        if all(_clear(p, [o], margin) for p in keep):
            obs.append(o)
    return obs


def _case(name, algo, kw, start, goal, m1, m2, list_counts, moves, env=None, bounds=(37, 101), radii=(0.3, 1.2),
          seeds=None):
    """One planner's sequence.  kw: the planner's constants; m1 / m2: the two shared maps (m2 has more rows); list_counts:
    rows per instance of the per-instance lists (more than 256 in all: the device table is reallocated); moves:
    {instance: (start, goal)}."""
    lo, hi = kw["rand_area"]
    keep = [start, goal] + [p for mv in moves.values() for p in mv if p is not None]
    pool = _free_map(1000 + len(name), max(list_counts), lo, hi, radii[0], radii[1], keep, 1.2)
    lists = [pool[:c] if i % 2 else pool[len(pool) - c:] for i, c in enumerate(list_counts)]
    assert sum(list_counts) > 256 and 0 in list_counts and len(m2) > len(m1) and len(list_counts) == N
    for p in keep:
        assert _clear(p, m1, 0.7) and _clear(p, m2, 0.7), (name, p)
    return dict(name=name, algo=algo, kw=kw, start=list(start), goal=list(goal), m1=m1, m2=m2, lists=lists, moves=moves,
                env=env or {}, bounds=bounds,
                seeds=seeds or ([101 + i for i in range(N)], [211 + 3 * i for i in range(N)]))


def _drv_case(name, algo, kw, start, goal, m1, moves, env=None, m2_extra=33, counts=(0, 64, 30, 64, 7, 64, 20, 40),
              rmax=0.9, seeds=None, list_radii=(0.05, 0.25)):
    keep = [start, goal] + [p for mv in moves.values() for p in mv if p is not None]
    m2 = list(m1) + _free_map(77, m2_extra, -2.0, 15.0, 0.3, rmax, keep, 1.2)
    return _case(name, algo, kw, start, goal, list(m1), m2, list(counts), moves, env, radii=list_radii, seeds=seeds)


def _cases():
    out = []
    base = dict(rand_area=[-2.0, 15.0], expand_dis=1.0, path_resolution=0.1, goal_sample_rate=5, max_iter=500,
                play_area=None, robot_radius=0.6, sobol=0, connect_circle_dist=50.0, search_until_max_iter=0)
    # rrt_01 / rrt_02: the drivers' scene (goldens rrt01_drv_s42 / rrt02_drv_s42); starts and goals outside rand_area
    far = {1: ([-3.5, -3.0], None), 4: (None, [16.5, 12.0]), N - 1: ([1.0, 13.0], [13.0, 1.0])}
    out.append(_drv_case("rrt-mt", "rrt", dict(base), [0.0, 0.0], [6.0, 10.0], DRV, far,
                         list_radii=(0.2, 0.6)))
    out.append(_drv_case("rrt-sobol", "rrt", dict(base, sobol=1), [0.0, 0.0], [6.0, 10.0], DRV, far,
                         list_radii=(0.2, 0.6)))
    # rrt_04: C2 (goldens rrt04_c2_*), 1 500 iterations; m2 crosses the obstacle tile of the 64- and the 128-thread shape
    c2 = dict(rand_area=[0.0, 100.0], expand_dis=2.0, path_resolution=0.25, goal_sample_rate=5, max_iter=1500,
              play_area=None, robot_radius=0.0, sobol=0, connect_circle_dist=50.0, search_until_max_iter=1)
    far2 = {1: ([-8.0, -5.0], None), 4: (None, [104.0, 101.0]), N - 1: ([10.0, 90.0], [90.0, 10.0])}
    keep2 = [[2.0, 2.0], [98.0, 98.0], [-8.0, -5.0], [104.0, 101.0], [10.0, 90.0], [90.0, 10.0]]
    m1 = [o for o in util.synth_map(7, 50) if all(_clear(p, [o], 1.0) for p in keep2)]
    m2 = _free_map(8, 70, 0.0, 100.0, 2.0, 6.0, keep2, 1.5)
    for nm, env, until in (("rrt_star-64", {"RRTX_TPB": "64"}, 1), ("rrt_star-128", {"RRTX_TPB": "128"}, 1),
                           ("rrt_star-256", {"RRTX_TPB": "256"}, 1), ("rrt_star-v1", {"RRTX_KERNEL": "v1"}, 1),
                           ("rrt_star-v1-early", {"RRTX_KERNEL": "v1"}, 0)):
        out.append(_case(nm, "rrt_star", dict(c2, search_until_max_iter=until), [2.0, 2.0], [98.0, 98.0], m1, m2,
                         [0, 50, 20, 56, 3, 56, 40, 50], far2, env, radii=(0.5, 2.5)))
    # rrt_07: the driver's scene (golden rrt07_drv_mt_s42_it2000), 600 iterations
    inf = dict(rand_area=[-2.0, 15.0], expand_dis=0.5, goal_sample_rate=10, max_iter=600, sobol=0)
    out.append(_drv_case("informed", "informed", inf, [0.0, 0.0], [6.0, 10.0], DRV, far, counts=(0, 90, 30, 64, 7, 64, 20, 40)))
    # pose planners: goldens rrt05_drv_s42_it500, rrt03_drv_s42_it200_sobol, rrt06_drv_s42_it200; moved poses with yaw
    yth = float(np.deg2rad(1.0))
    pose_moves = {1: ([1.0, -1.0, 0.7], None), 4: (None, [12.0, 3.0, -1.2]), N - 1: ([-1.0, 2.0, 2.0], [11.0, 12.0, 1.0])}
    d5 = dict(rand_area=[-2.0, 15.0], expand_dis=3.0, path_resolution=0.5, goal_sample_rate=10, max_iter=300,
              robot_radius=0.0, connect_circle_dist=50.0, search_until_max_iter=1, curvature=1.0, goal_yaw_th=yth,
              goal_xy_th=0.5, sobol=0)
    out.append(_drv_case("rrt_star_dubins", "rrt_star_dubins", d5, [0.0, 0.0, 0.0], [10.0, 10.0, 0.0], DRV[:6], pose_moves))
    d3 = dict(d5, expand_dis=0.0, sobol=1)
    out.append(_drv_case("rrt_dubins", "rrt_dubins", d3, [0.0, 0.0, 0.0], [10.0, 10.0, 0.0], DRV[:6], pose_moves))
    d6 = dict(d5, max_iter=150, robot_radius=0.6, curvature=2.0, step_size=0.1)
    out.append(_drv_case("rrt_star_reeds_shepp", "rrt_star_reeds_shepp", d6, [0.0, 0.0, 0.0], [10.0, 9.0, 0.0], DRV,
                         pose_moves))
    # rrt_08: the C4 scene (test_gpu_bitstar_batch_c4_style_equals_oracle); every list within the one-wave kernel's 64
    bit = dict(rand_area=[-2.0, 15.0], max_iter=80)
    bit_moves = {1: ([-1.0, 13.0], None), 4: (None, [13.5, 2.0]), N - 1: ([2.0, 1.0], [11.0, 13.0])}
    # tree.vertices holds maxIter or maxIter + 1 entries whatever the map: the seeds are picked (with the oracle) so that
    # all of S1 give 81 vertices on M1, and all of S2 80 on M1 and 81 on M2 -- every tree shrinks at plan 2 and grows at 3
    bit_seeds = ([300, 301, 303, 304, 306, 311, 312, 313], [308, 310, 317, 319, 325, 330, 334, 347])
    bit_counts = (0, 64, 6, 60, 20, 64, 6, 50)
    assert max(bit_counts) <= 64 and bit["max_iter"] + 2 <= 128     # beyond either, rrtx_plan falls back to the lane kernel
    for nm, env in (("bitstar-wave", {}), ("bitstar-lane", {"RRTX_BITSTAR": "lane"})):
        out.append(_drv_case(nm, "bitstar", dict(bit), [0.0, 0.0], [12.0, 12.0], BIT_OBS, bit_moves, env, m2_extra=24,
                             counts=bit_counts, rmax=0.6, seeds=bit_seeds))
    # rrt_09: the batches of test_gpu_lqr.py
    lq = dict(rand_area=[-2.0, 15.0], expand_dis=3.0, path_resolution=0.5, goal_sample_rate=10, max_iter=300,
              play_area=None, robot_radius=0.0, sobol=0, connect_circle_dist=50.0, goal_xy_th=0.5, step_size=0.2,
              search_until_max_iter=1)
    lq_moves = {1: ([1.5, -1.0], None), 4: (None, [12.0, 12.5]), N - 1: ([-1.0, 2.0], [11.0, 9.0])}
    out.append(_drv_case("lqr_rrt_star", "lqr_rrt_star", lq, [0.0, 0.0], [6.0, 10.0], DRV, lq_moves))
    return out


CASES = {c["name"]: c for c in _cases()}


# ------------------------------------------------------------------------------------------------ the oracle side
def _oracle_one(a):
    """One instance of one plan on the CPU oracle -> plain arrays (picklable).  inp: dict(rng=("seed", s) | ("state",
    624 words + position), obs, start, goal)."""
    algo, kw, inp = a
    import oracle
    start, goal, obs = inp["start"], inp["goal"], inp["obs"]
    if algo == "lqr_rrt_star":
        import lqr_oracle
        o = lqr_oracle.LQROracle(start, goal, obs, kw["rand_area"], kw["expand_dis"], kw["goal_sample_rate"],
                                 kw["max_iter"], kw["play_area"], kw["robot_radius"], bool(kw["sobol"]),
                                 kw["connect_circle_dist"], kw["goal_xy_th"], kw["step_size"])
        rng = random.Random()
        if inp["rng"][0] == "seed":
            rng.seed(inp["rng"][1])
        else:
            rng.setstate((3, tuple(inp["rng"][1]), None))
        rows = []
        p = o.planning(rng, bool(kw["search_until_max_iter"]), trace=rows)
        polys = [o.polyline(i) for i in range(len(o.x))]
        return dict(x=np.array(o.x, dtype=np.float64), y=np.array(o.y, dtype=np.float64),
                    cost=np.array(o.cost, dtype=np.float64), parent=np.array(o.parent, dtype=np.int32),
                    path=None if p is None else np.array(p, dtype=np.float64),
                    path_cost=None if p is None else lqr_oracle.get_path_length(p), rng=tuple(rng.getstate()[1]),
                    poly_len=np.array([len(q[0]) for q in polys], dtype=np.int32),
                    poly_x=np.array([v for q in polys for v in q[0]], dtype=np.float64),
                    poly_y=np.array([v for q in polys for v in q[1]], dtype=np.float64), sobol_index=o.sob_index,
                    near_total=None,
                    trace=(np.array([t[0] for t in rows], dtype=np.float64), np.array([t[1] for t in rows], dtype=np.float64),
                           np.array([t[2] for t in rows], dtype=np.int32), np.array([t[3] for t in rows], dtype=np.int32)))
    rng = oracle.mt_from_seed(inp["rng"][1]) if inp["rng"][0] == "seed" else oracle.mt_from_pystate((3, inp["rng"][1], None))
    if algo in ("rrt", "rrt_star"):
        r = oracle.plan(algo=algo, start=start, goal=goal, obstacles=obs, rng=rng, exact_pow=True, trace=True, **kw)
        out = dict(stats=r["stats"], sobol_index=r["stats"]["sobol_index"], near_total=r["stats"]["near_unique"],
                   trace=(r["tr_rnd_x"], r["tr_rnd_y"], r["tr_nearest"], r["tr_n_near"]))
        if r["path"] is not None and algo == "rrt_star":
            p = r["path"]
            out["path_cost"] = sum(math.hypot(p[j + 1][0] - p[j][0], p[j + 1][1] - p[j][1]) for j in range(len(p) - 1)) + 0.0
    elif algo == "informed":
        r = oracle.plan_informed(start, goal, obs, kw["rand_area"], kw["expand_dis"], kw["goal_sample_rate"],
                                 kw["max_iter"], bool(kw["sobol"]), rng=rng, trace=True)
        out = dict(near_total=r["stats"]["near_unique"],
                   trace=(r["tr_rnd_x"], r["tr_rnd_y"], r["tr_nearest"], r["tr_n_near"]))
        if r["path"] is not None:
            out["path_cost"] = r["c_best"]
    elif algo == "bitstar":
        r = oracle.plan_bitstar(start, goal, obs, kw["rand_area"], kw["max_iter"], rng=rng)
        assert r["error"] == 0
        ids = r["vertex_ids"]
        cells = float(math.ceil((kw["rand_area"][1] - kw["rand_area"][0]) / 0.01))
        c1 = np.floor(ids / cells)
        c0 = np.floor((ids - c1 * cells) / 1)
        par = np.array([-1 if q < 0 else int(np.nonzero(ids == q)[0][0]) for q in r["parent_ids"]], dtype=np.int32)
        return dict(x=kw["rand_area"][0] + 0.01 * c0, y=kw["rand_area"][0] + 0.01 * c1, cost=r["g_scores"], parent=par,
                    path=r["path"] if len(r["path"]) else None, rng=tuple(r["rng"].mt) + (r["rng"].pos,),
                    trace=(r["tr_e0"], r["tr_e1"]))
    else:
        common = dict(rng=rng, trace=True, curvature=kw["curvature"], robot_radius=kw["robot_radius"], goal_yaw_th=kw["goal_yaw_th"],
                      goal_xy_th=kw["goal_xy_th"], search_until_max_iter=bool(kw["search_until_max_iter"]))
        if algo == "rrt_star_dubins":
            r = oracle.plan_dubins(start, goal, obs, kw["rand_area"], kw["max_iter"], goal_sample_rate=kw["goal_sample_rate"],
                                   expand_dis=kw["expand_dis"], connect_circle_dist=kw["connect_circle_dist"], **common)
        elif algo == "rrt_dubins":
            r = oracle.plan_rrt_dubins(start, goal, obs, kw["rand_area"], kw["max_iter"],
                                       goal_sample_rate=kw["goal_sample_rate"], sobol=bool(kw["sobol"]), **common)
        else:
            r = oracle.plan_rrt_rs(start, goal, obs, kw["rand_area"], kw["max_iter"], expand_dis=kw["expand_dis"],
                                   connect_circle_dist=kw["connect_circle_dist"], step_size=kw["step_size"], **common)
        out = dict(yaw=r["yaw"], poly_len=r["poly_len"], poly_x=r["poly_x"], poly_y=r["poly_y"],
                   near_total=r["stats"]["near_unique"], trace=(r["tr_rx"], r["tr_ry"], r["tr_nearest"], r["tr_n_near"]))
        if algo == "rrt_dubins" and kw["sobol"]:
            out["sobol_index"] = r["sobol_index"]
        if algo == "rrt_star_reeds_shepp":
            out["path_yaw"] = r["path_yaw"]
    out.update(x=r["x"], y=r["y"], cost=r["cost"], parent=r["parent"], path=r["path"],
               rng=tuple(r["rng"].mt) + (r["rng"].pos,))
    return out


def _same_result(a, b):
    if len(a["x"]) != len(b["x"]) or (a["path"] is None) != (b["path"] is None):
        return False
    return all(np.array_equal(a[k], b[k]) for k in ("x", "y", "cost", "parent")) and \
        (a["path"] is None or np.array_equal(a["path"], b["path"]))


def _steps(P):
    """The sequence as data: per step the setter calls (replayable on a fresh handle), whether the plan runs through
    plan_begin / plan_step, and how each instance's inputs change.  Every step changes one kind of input, except step 5:
    set_instance moves SOME instances only, and an unmoved instance with nothing else changed would repeat plan 4b --
    the one situation in which stale state passes unnoticed.  So step 5 also continues every instance's random stream."""
    s1, s2 = P["seeds"]
    k1, k2 = P["bounds"]
    return [
        dict(label="1 seeds S1, map M1", ops=[("set_obstacles", P["m1"]), ("seed_instances", s1)], stepped=False),
        dict(label="2 reseeded S2", ops=[("seed_instances", s2), ("set_launch_bound", k1)], stepped=True),
        dict(label="3 larger map M2", ops=[("set_obstacles", P["m2"])], stepped=False),
        dict(label="4a per-instance lists", ops=[("set_instance_obstacles", P["lists"]), ("set_launch_bound", ONE_LAUNCH)],
             stepped=True),
        dict(label="4b back to M1", ops=[("set_obstacles", P["m1"])], stepped=False),
        dict(label="5 moved instances, stream continued", ops=[("continue_rng",)] + [("move", i, s, g) for i, (s, g) in
                                                                                      sorted(P["moves"].items())]
             + [("set_launch_bound", k2)], stepped=False),
        dict(label="6 stream continued", ops=[("continue_rng",)], stepped=True),
    ]


def _build(P, steps=None):
    """Inputs and oracle results of every instance of every plan, and the preconditions of the sequence -- from the
    oracle's outputs alone, before anything runs on the GPU."""
    steps = _steps(P) if steps is None else steps
    cur = [dict(rng=None, obs=[], start=list(P["start"]), goal=list(P["goal"])) for _ in range(N)]
    refs = []
    with ProcessPoolExecutor(max_workers=8) as ex:
        for k, st in enumerate(steps):
            for op in st["ops"]:
                if op[0] == "set_obstacles":
                    for c in cur:
                        c["obs"] = list(op[1])
                elif op[0] == "set_instance_obstacles":
                    for c, lst in zip(cur, op[1]):
                        c["obs"] = list(lst)
                elif op[0] == "seed_instances":
                    for c, s in zip(cur, op[1]):
                        c["rng"] = ("seed", s)
                elif op[0] == "continue_rng":
                    for c, r in zip(cur, refs[k - 1]):
                        c["rng"] = ("state", r["rng"])
                elif op[0] == "move":
                    _, i, s, g = op
                    if s is not None:
                        cur[i]["start"] = list(s)
                    if g is not None:
                        cur[i]["goal"] = list(g)
            st["inputs"] = [dict(c) for c in cur]
            refs.append(list(ex.map(_oracle_one, [(P["algo"], P["kw"], dict(c)) for c in cur])))
    nn = np.array([[len(r["x"]) for r in plan] for plan in refs])
    shrinks = [k for k in range(1, len(refs)) if (nn[k] < nn[k - 1]).all()]
    grows = [k for k in range(1, len(refs)) if (nn[k] > nn[k - 1]).all()]
    assert shrinks, "%s: no plan leaves every tree shorter than the plan before it: %s" % (P["name"], nn.tolist())
    assert grows, "%s: no plan leaves every tree longer than the plan before it: %s" % (P["name"], nn.tolist())
    for k in range(1, len(refs)):
        for i in range(N):
            assert not _same_result(refs[k][i], refs[k - 1][i]), "%s: plan %d repeats plan %d for instance %d" % (
                P["name"], k, k - 1, i)
    return steps, refs


# ------------------------------------------------------------------------------------------------ the GPU side
def _rot(algo, start, goal):
    import rrt_amd
    cm, c = (rrt_amd.informed_rotation if algo == "informed" else rrt_amd.bitstar_rotation)(start, goal)
    return [c[0, 0], c[0, 1], c[1, 0], c[1, 1]], cm


def _make_handle(P, n=N, max_iter=None):
    import rrt_amd
    A = rrt_amd._abi
    kw, algo = P["kw"], P["algo"]
    mi = kw["max_iter"] if max_iter is None else max_iter
    sampler = A.SAMPLER_SOBOL if kw.get("sobol") else A.SAMPLER_MT
    if algo == "informed":
        rot, cm = _rot(algo, P["start"], P["goal"])
        return A.Handle(A.ALGO_INFORMED, P["start"], P["goal"], kw["rand_area"], kw["expand_dis"], 1.0,
                        kw["goal_sample_rate"], mi, sampler=sampler, n_instances=n, informed_rot=rot, informed_c_min=cm)
    if algo == "bitstar":
        rot, cm = _rot(algo, P["start"], P["goal"])
        return A.Handle(A.ALGO_BITSTAR, P["start"], P["goal"], kw["rand_area"], 2.0, 1.0, 0, mi, n_instances=n,
                        informed_rot=rot, informed_c_min=cm)
    code = {"rrt": A.ALGO_RRT, "rrt_star": A.ALGO_RRT_STAR, "rrt_star_dubins": A.ALGO_DUBINS, "rrt_dubins": A.ALGO_RRT_DUBINS,
            "rrt_star_reeds_shepp": A.ALGO_RS, "lqr_rrt_star": A.ALGO_LQR_RRT_STAR}[algo]
    return A.Handle(code, P["start"], P["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                    kw["goal_sample_rate"], mi, play_area=kw.get("play_area"), robot_radius=kw["robot_radius"],
                    sampler=sampler, connect_circle_dist=kw["connect_circle_dist"],
                    search_until_max_iter=kw["search_until_max_iter"], n_instances=n, curvature=kw.get("curvature", 1.0),
                    goal_yaw_th=kw.get("goal_yaw_th", 0.0), goal_xy_th=kw.get("goal_xy_th", 0.0),
                    step_size=kw.get("step_size", 0.0))


def _apply(h, P, ops, inputs, prev_refs, from_handle):
    """The setter calls of one step.  continue_rng: the state each instance's last plan left -- read from the handle
    (the reused one), or the oracle's, which that plan was checked against (a fresh handle has no earlier plan)."""
    for op in ops:
        if op[0] == "continue_rng":
            for i in range(N):
                h.set_rng_state(i, h.get_rng_state(i) if from_handle else (3, prev_refs[i]["rng"], None))
        elif op[0] == "move":
            _, i, s, g = op
            h.set_instance(i, s, g)
            if P["algo"] in ("informed", "bitstar"):
                rot, cm = _rot(P["algo"], inputs[i]["start"], inputs[i]["goal"])
                h.set_instance_rotation(i, rot, cm)
        else:
            getattr(h, op[0])(op[1])


def _plan(h, stepped):
    """rrtx_plan, or plan_begin + plan_step until nothing is pending; returns the number of steps (0: rrtx_plan)."""
    if not stepped:
        assert h.plan() == 0, h.last_error()
        return 0
    h.plan_begin()
    steps = 0
    while True:
        rc, pending = h.plan_step()     # raises on a negative code: nothing further is launched
        steps += 1
        if pending == 0:
            assert rc == 0, h.last_error()
            return steps
        assert steps < 100000


def _read(h, P, n=N):
    algo = P["algo"]
    pose = algo in ("rrt_star_dubins", "rrt_dubins", "rrt_star_reeds_shepp")
    sob = bool(P["kw"].get("sobol")) and algo in ("rrt", "rrt_star", "rrt_dubins", "lqr_rrt_star")
    return util.read_planned(h, n, yaws=pose, polys=pose or algo == "lqr_rrt_star",
                             path_yaws=algo == "rrt_star_reeds_shepp", sobol=sob)


def _check(P, out, refs, what, ids=None):
    """Every instance of a plan against the oracle: integers exact, doubles bit for bit, the RNG state word for word."""
    A = _abi
    pc, nn, st = out["results"]
    ids = range(len(refs)) if ids is None else ids
    for i in ids:
        r, w = refs[i], "%s, %s, instance %d" % (P["name"], what, i)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), w)
        assert nn[i] == len(r["x"]) and st[i] & A.ST_DONE and not st[i] & A.ST_FAILED, w
        p = out["paths"][i]
        assert (p is None) == (r["path"] is None) and bool(st[i] & A.ST_PATH) == (r["path"] is not None), w
        if p is not None:
            assert np.array_equal(p, r["path"]), w
            if "path_cost" in r:
                assert pc[i] == r["path_cost"], w
            if "path_yaw" in r:
                assert np.array_equal(out["path_yaws"][i], r["path_yaw"]), w
        else:
            assert math.isinf(pc[i]), w
        assert tuple(out["rng"][i][1]) == tuple(r["rng"]), "%s: RNG state (position %d, oracle %d)" % (
            w, out["rng"][i][1][624], r["rng"][624])
        if "yaw" in r:
            assert np.array_equal(out["yaws"][i], r["yaw"]), w
        if "poly_len" in r:
            plen, px, py = out["polys"][i]
            assert np.array_equal(plen, r["poly_len"]) and np.array_equal(px, r["poly_x"]) and \
                np.array_equal(py, r["poly_y"]), w
        if "sobol_index" in out and "sobol_index" in r:
            assert out["sobol_index"][i] == r["sobol_index"], w
    assert out["stats"]["total_nodes"] == int(sum(len(r["x"]) for r in refs)), what
    if P["algo"] == "rrt_star":
        for k in ORACLE_COUNTERS:
            assert out["stats"][k] == sum(r["stats"][k] for r in refs), (P["name"], what, k)


def _assert_trace(got, r, what):
    """The rows of rrtx_get_trace against the oracle's.  Tree planners: sample and nearest node bit for bit.  n_near: the
    device counts the DISTINCT near indices (rrtx.h), the oracles of rrt_01 .. rrt_07 record len(near_inds) with its
    repeats and sum the distinct ones in Stats.near_unique -- so: -1 (no near query) in the same rows, never more than
    the oracle's count, and the plan's total equal to near_unique.  The rrt_09 oracle's near list has no repeats: equal
    row by row.  BIT*: the two ids of every popped edge."""
    want = r["trace"]
    if len(want) == 2:
        assert len(got[0]) == len(want[0]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
        return
    for k in range(3):
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), "%s: trace column %d" % (what, k)
    g, w = got[3], want[3]
    assert len(g) == len(w), what
    if r["near_total"] is None:
        assert np.array_equal(g, w), "%s: n_near" % what
    else:
        assert np.array_equal(g < 0, w < 0) and (g <= w).all(), "%s: n_near %s, oracle %s" % (what, g[:40], w[:40])
        assert int(g[g >= 0].sum()) == r["near_total"], "%s: n_near sums to %d, oracle near_unique %d" % (
            what, int(g[g >= 0].sum()), r["near_total"])


def _expected_shape(P, m_max):
    """main_shape as rrtx_stats documents it for a batch of N instances: RRTX_TPB's shape while its obstacle tile (56 /
    64 / 256) holds the largest list, else 256; the general kernel and the other planners: their fixed shape."""
    env, algo = P["env"], P["algo"]
    if algo == "rrt_star" and P["kw"]["search_until_max_iter"] and env.get("RRTX_KERNEL") != "v1":
        t = int(env.get("RRTX_TPB", "256"))
        return 64 if t == 64 and m_max <= 56 else 128 if t == 128 and m_max <= 64 else 256
    return {"rrt": 256, "rrt_star": 256, "informed": 256, "rrt_star_dubins": 256, "rrt_dubins": 256,
            "rrt_star_reeds_shepp": 64, "bitstar": 64, "lqr_rrt_star": 64}[algo]


def _assert_counters_equal(a, b, what):
    for k in a:
        if k not in TIMES:
            assert a[k] == b[k], "%s: rrtx_stats.%s %s on the reused handle, %s on a fresh one" % (what, k, a[k], b[k])


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", sorted(CASES))
def test_changed_plans_on_one_handle_equal_the_oracle(gpu, monkeypatch, name):
    """Section A.  Seven plans on one handle, each with one kind of input changed (see _steps), each compared with the
    oracle for all instances; counters, main_shape, replanned and launches equal a fresh handle's that plans once.
    Step 3 of the issue asks for a reallocated obstacle table through set_obstacles; the table starts at the 256 rows
    set_obstacles accepts at most, so the per-instance lists of 4a (more than 256 rows in all) are what reallocates it,
    and 4b's set_obstacles then writes the new table."""
    P = CASES[name]
    steps, refs = _build(P)
    for k, v in P["env"].items():
        monkeypatch.setenv(k, v)
    h = _make_handle(P)
    try:
        bound = None
        for k, st in enumerate(steps):
            what = "plan " + st["label"]
            _apply(h, P, st["ops"], st["inputs"], refs[k - 1] if k else None, True)
            bound = dict([op[:2] for op in st["ops"] if op[0] == "set_launch_bound"]).get("set_launch_bound", bound)
            nsteps = _plan(h, st["stepped"])
            out = _read(h, P)
            _check(P, out, refs[k], what)
            m_max = max(len(c["obs"]) for c in st["inputs"])
            assert out["stats"]["main_shape"] == _expected_shape(P, m_max), what
            longest = max(r["stats"]["iterations"] for r in refs[k]) if P["algo"] in ("rrt", "rrt_star") else ONE_LAUNCH
            if P["env"].get("RRTX_BITSTAR") == "lane":
                # the one-lane BIT* kernel is not bounded (rrtx.h): one launch, whatever the bound
                assert out["stats"]["launches"] == 1 and nsteps in (0, 1), what
            elif st["stepped"] and bound is not None and bound < min(ONE_LAUNCH, longest):
                assert nsteps > 1 and out["stats"]["launches"] > 1, what      # the bound holds: the plan spans launches
            if name == "bitstar-wave" and bound is not None and bound < ONE_LAUNCH:
                assert out["stats"]["launches"] > 1, what    # main_shape is 64 for both BIT* kernels: this one is bounded
            f = _make_handle(P)
            try:
                for j in range(k + 1):
                    _apply(f, P, steps[j]["ops"], steps[j]["inputs"], refs[j - 1] if j else None, False)
                _plan(f, False)
                fresh = _read(f, P)
            finally:
                f.close()
            _check(P, fresh, refs[k], what + " (fresh handle)")
            _assert_counters_equal(out["stats"], fresh["stats"], "%s, %s" % (name, what))
    finally:
        h.close()


def test_rrt_star_kernel_shapes_in_turn_on_one_handle(gpu, monkeypatch):
    """rrt_04 on ONE handle at 64 -> 256 -> 64 -> 128 -> general kernel -> 64 threads per instance (RRTX_TPB / RRTX_KERNEL
    are read by rrtx_plan_begin), other seeds every time, the dense and the sparse map in turn, the grid index of the
    one-wave shape in use from 256 nodes on (RRTX_GRID_MIN): the 64-thread shape's grid index and the speculation records
    in the tail of hits[] are used again after other shapes wrote the arrays.  main_shape names the shape that ran."""
    P = CASES["rrt_star-64"]
    monkeypatch.setenv("RRTX_GRID_MIN", "256")
    order = [("64", None, 64), ("256", None, 256), ("64", None, 64), ("128", None, 128), (None, "v1", 256), ("64", None, 64)]
    sparse = P["m1"][:20]
    steps = [dict(label="shape %s" % (t or k), stepped=bool(j % 2),
                  ops=[("set_obstacles", sparse if j % 2 else P["m1"]), ("seed_instances", [31 + 10 * j + i for i in range(N)])])
             for j, (t, k, _) in enumerate(order)]
    steps, refs = _build(P, steps)
    h = _make_handle(P)
    try:
        h.set_launch_bound(401)
        for j, (st, (tpb, kern, shape)) in enumerate(zip(steps, order)):
            monkeypatch.delenv("RRTX_TPB", raising=False)
            monkeypatch.delenv("RRTX_KERNEL", raising=False)
            if tpb:
                monkeypatch.setenv("RRTX_TPB", tpb)
            if kern:
                monkeypatch.setenv("RRTX_KERNEL", kern)
            _apply(h, P, st["ops"], st["inputs"], None, True)
            _plan(h, st["stepped"])
            out = _read(h, P)
            assert out["stats"]["main_shape"] == shape, st["label"]
            _check(P, out, refs[j], "plan %d, %s" % (j, st["label"]))
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ B
def _walled(start):
    """A map on which no tree leaves its root: the start lies inside a circle, every extension collides."""
    return [(float(start[0]), float(start[1]), 1.5)]


def _replan_sequence(P, plans, expect_replanned, n, max_iter=None):
    """plans: per plan (per-instance obstacle lists, seeds).  Every plan on ONE handle against the oracle, and
    replanned / launches / every integer counter against a fresh handle: the counters are per plan."""
    steps = [dict(label="plan %d" % j, stepped=False, ops=[("set_instance_obstacles", lists), ("seed_instances", seeds)])
             for j, (lists, seeds) in enumerate(plans)]
    cur_refs = []
    kw = dict(P["kw"], max_iter=P["kw"]["max_iter"] if max_iter is None else max_iter)
    with ProcessPoolExecutor(max_workers=8) as ex:
        for lists, seeds in plans:
            cur_refs.append(list(ex.map(_oracle_one, [(P["algo"], kw, dict(rng=("seed", s), obs=list(o), start=P["start"],
                                                                           goal=P["goal"])) for o, s in zip(lists, seeds)])))
    P2 = dict(P, kw=kw)
    h = _make_handle(P2, n)
    got = []
    try:
        for j, st in enumerate(steps):
            for op in st["ops"]:
                getattr(h, op[0])(op[1])
            assert h.plan() == 0, h.last_error()
            out = _read(h, P2, n)
            _check(P2, out, cur_refs[j], st["label"])
            f = _make_handle(P2, n)
            try:
                for op in st["ops"]:
                    getattr(f, op[0])(op[1])
                assert f.plan() == 0, f.last_error()
                fresh = f.get_stats()
            finally:
                f.close()
            _assert_counters_equal(out["stats"], fresh, "%s, %s" % (P["name"], st["label"]))
            assert expect_replanned[j](out["stats"]["replanned"]), (st["label"], out["stats"]["replanned"])
            got.append(out["stats"]["replanned"])
    finally:
        h.close()
    return got, cur_refs


@pytest.mark.parametrize("order", ["replanned-first", "replanned-last"])
def test_near_set_overflow_replan_then_other_plans(gpu, monkeypatch, order):
    """The scene of test_gpu_near_set_overflow_is_replanned_on_a_larger_shape on the 64-thread shape (near sets outgrow
    its 44 candidate slots: instances are planned again on the larger shapes, through inst_map), before and after a plan
    on which nothing is re-planned (no tree leaves its root), and a mixed plan in which only some instances are."""
    monkeypatch.setenv("RRTX_TPB", "64")
    kw = dict(rand_area=[-2.0, 15.0], expand_dis=3.0, path_resolution=0.5, goal_sample_rate=5, max_iter=700,
              play_area=None, robot_radius=0.8, sobol=0, connect_circle_dist=50.0, search_until_max_iter=1)
    P = dict(name="rrt_star overflow", algo="rrt_star", kw=kw, start=[0.0, 0.0], goal=[6.0, 10.0], env={"RRTX_TPB": "64"})
    n = 6
    over = ([DRV] * n, [1 + i for i in range(n)])
    calm = ([_walled(P["start"])] * n, [51 + i for i in range(n)])
    mixed = ([DRV if i % 2 else _walled(P["start"]) for i in range(n)], [71 + i for i in range(n)])
    if order == "replanned-first":
        plans, exp = [over, calm, mixed], [lambda r: r > 0, lambda r: r == 0, lambda r: 0 < r]
    else:
        plans, exp = [calm, over, calm], [lambda r: r == 0, lambda r: r > 0, lambda r: r == 0]
    _replan_sequence(P, plans, exp, n)


def _moved_nodes(kw, obs, start, goal, seed):
    """How many nodes rrt_04's rewire MOVES in this plan (steer stops short of the node, :1372), by the oracle's counter."""
    import oracle
    L = oracle.lib()
    m0, r0, m1, r1 = C.c_long(), C.c_long(), C.c_long(), C.c_long()
    L.orc_moved_counters(C.byref(m0), C.byref(r0))
    oracle.plan(algo="rrt_star", start=start, goal=goal, obstacles=obs, rng=oracle.mt_from_seed(seed), exact_pow=True, **kw)
    L.orc_moved_counters(C.byref(m1), C.byref(r1))
    return m1.value - m0.value


@pytest.mark.parametrize("order", ["replanned-first", "replanned-last"])
@pytest.mark.parametrize("rate,seed", [(95, 8), (20, 19507)])
def test_moved_node_replan_then_other_plans(gpu, order, rate, seed):
    """The moved-node problems of test_gpu_rewire_moved_node_equals_oracle ('diag' scene, path_resolution 0.05): the
    iteration kernel leaves the instance as RRTX_ST_UNSUPPORTED and rrtx_plan hands it to the general kernel alone
    (rewire_raw_walk) after the iteration kernel wrote the arrays -- a re-plan route of its own.  One handle: a plan with
    that instance among three that move no node, and plans in which no instance moves a node (by the oracle's counter:
    without a moved node nothing can be UNSUPPORTED, and 401 nodes cannot outgrow the 256 candidate slots), in both
    orders.  Only an instance that moves a node can be re-planned."""
    kw = dict(rand_area=[-2.0, 12.0], expand_dis=3.0, path_resolution=0.05, goal_sample_rate=rate, max_iter=400,
              play_area=None, robot_radius=0.0, sobol=0, connect_circle_dist=50.0, search_until_max_iter=1)
    obs, start, goal = [(3.0, 3.0, 1.0)], [0.0, 0.0], [6.0, 8.0]
    P = dict(name="rrt_star moved node", algo="rrt_star", kw=kw, start=start, goal=goal, env={})
    n = 4
    over, calm, calm2 = [2, seed, 3, 4], [5, 6, 7, 9], [10, 11, 13, 14]
    assert [_moved_nodes(kw, obs, start, goal, s) > 0 for s in over] == [False, True, False, False]
    assert not any(_moved_nodes(kw, obs, start, goal, s) for s in calm + calm2)
    if order == "replanned-first":
        plans, exp = [over, calm, over], [lambda r: r == 1, lambda r: r == 0, lambda r: r == 1]
    else:
        plans, exp = [calm, over, calm2], [lambda r: r == 0, lambda r: r == 1, lambda r: r == 0]
    _replan_sequence(P, [([obs] * n, sd) for sd in plans], exp, n)


def test_informed_overflow_replan_then_other_plans(gpu, monkeypatch):
    """The scene of test_gpu_informed_near_set_overflow_is_replanned_on_the_large_shape (near sets beyond 512 candidates:
    planned again on the 2 048-slot shape, cbest reset per instance), then a plan without a re-plan, then both kinds in
    one plan."""
    obst = [(2.5, 2.5, 0.3), (1.0, 3.5, 0.25), (3.8, 1.2, 0.25)]
    kw = dict(rand_area=[0.0, 5.0], expand_dis=0.08, goal_sample_rate=10, max_iter=1500, sobol=0)
    P = dict(name="informed overflow", algo="informed", kw=kw, start=[0.5, 0.5], goal=[4.5, 4.5], env={})
    n = 4
    walled = [(0.5, 0.5, 0.2)]
    plans = [([obst] * n, [3, 4, 5, 6]), ([walled] * n, [13, 14, 15, 16]), ([obst, walled, obst, walled], [23, 24, 25, 26]),
             ([walled] * n, [33, 34, 35, 36])]
    got, refs = _replan_sequence(P, plans, [lambda r: r > 0, lambda r: r == 0, lambda r: 0 < r <= 2,
                                                          lambda r: r == 0], n)
    assert all(len(r["x"]) > 900 for r in refs[0])


@pytest.mark.parametrize("algo", ["rrt_star_dubins", "rrt_star_reeds_shepp"])
def test_pool_retry_sets_of_different_sizes_on_one_handle(gpu, monkeypatch, algo):
    """Polyline-pool re-plans (RRTX_POOL_POINTS_PER_NODE shrinks the pool) of 2, then 1, then all instances on one handle:
    the smaller set uses the enlarged pool kept from the plan before, the larger one reallocates it.  An instance whose
    final edges alone hold more points than the pool has room for must have been re-planned (the oracle's polylines say
    so); instances on the walled map keep their root and are not.  Trees, yaws, polylines and paths of both kinds equal
    the oracle after every plan."""
    P = CASES[algo]
    ppn = 4 if algo == "rrt_star_dubins" else 2
    monkeypatch.setenv("RRTX_POOL_POINTS_PER_NODE", str(ppn))
    n, mi = 6, (1000 if algo == "rrt_star_dubins" else 500)
    cap = (2 if algo == "rrt_star_reeds_shepp" else 1) * mi + 2
    pool = ppn * cap + 8192
    wall, m = _walled(P["start"]), (P["m1"] if algo == "rrt_star_dubins" else P["m1"][:1])
    plans = [([m, wall, wall, m, wall, wall], [42 + i for i in range(n)]),
             ([wall, wall, m, wall, wall, wall], [52 + i for i in range(n)]),
             ([m] * n, [62 + i for i in range(n)])]
    sure = []
    # the oracle's final polylines give a lower bound of the pool use (edges replaced by rewire stay allocated)
    kw = dict(P["kw"], max_iter=mi)
    with ProcessPoolExecutor(max_workers=8) as ex:
        for lists, seeds in plans:
            rs = list(ex.map(_oracle_one, [(P["algo"], kw, dict(rng=("seed", s), obs=list(o), start=P["start"], goal=P["goal"]))
                                           for o, s in zip(lists, seeds)]))
            sure.append(sum(1 for r in rs if int(r["poly_len"].sum()) > pool))
    assert sure[0] == 2 and sure[1] == 1 and sure[2] == n, sure
    got, _ = _replan_sequence(P, plans, [lambda r, j=j: r >= sure[j] for j in range(3)], n, max_iter=mi)
    # rrtx_stats.replanned counts an instance once per attempt (pool x4, then x16); the walled instances never
    assert all(sure[j] <= got[j] <= 2 * sure[j] for j in range(3)), (got, sure)


# ------------------------------------------------------------------------------------------------ C
def test_batch_planner_over_three_handles_plans_twice(gpu, tmp_path):
    """BatchPlanner(devices=[0, 0, 0]): two plans through rrtx_plan_many with every shard reseeded in between; the second
    plan's concatenated results, smooth() (against oracle.path_smoothing continuing each instance's post-plan stream) and
    export_npz are the second plan's."""
    import oracle
    import rrt_amd
    n = 10
    kw = dict(rand_area=[-2.0, 15.0], expand_dis=1.0, path_resolution=0.1, goal_sample_rate=5, max_iter=500,
              play_area=[0, 10, 0, 14], robot_radius=0.6, sobol=0, connect_circle_dist=50.0, search_until_max_iter=1)
    s1, s2 = [1234 + i for i in range(n)], [77 + 2 * i for i in range(n)]
    args = [("rrt_star", kw, dict(rng=("seed", s), obs=DRV, start=[0.0, 0.0], goal=[6.0, 10.0])) for s in s1 + s2]
    with ProcessPoolExecutor(max_workers=8) as ex:
        refs = list(ex.map(_oracle_one, args))
    r1, r2 = refs[:n], refs[n:]
    assert all(not _same_result(a, b) for a, b in zip(r1, r2)) and sum(r["path"] is not None for r in r2) >= n // 2
    bp = rrt_amd.BatchPlanner("rrt_star", s1, [0, 0], [6.0, 10.0], DRV, [-2, 15], expand_dis=1.0, path_resolution=0.1,
                              goal_sample_rate=5, max_iter=500, play_area=[0, 10, 0, 14], robot_radius=0.6,
                              connect_circle_dist=50.0, search_until_max_iter=True, devices=[0, 0, 0])
    P = dict(name="sharded rrt_star", algo="rrt_star", kw=kw)
    try:
        def read():
            pc, nn, st = bp.results()
            return dict(results=(pc, nn, st), stats=bp.stats(), trees=[bp.tree(i) for i in range(n)],
                        paths=[bp.path(i) for i in range(n)], rng=[bp.rng_state(i) for i in range(n)])
        bp.plan()
        _check(P, read(), r1, "first plan")
        bp.smooth(200)                       # the first plan's smoothed paths must not survive the second plan
        for h, (lo, hi) in zip(bp.handles, bp.shards):
            h.seed_instances(s2[lo:hi])
        bp.plan()
        _check(P, read(), r2, "second plan")
        z = np.load(bp.export_npz(str(tmp_path / "second.npz")))
        for i in range(n):
            assert np.array_equal(z["x_%d" % i], r2[i]["x"]) and np.array_equal(z["parent_%d" % i], r2[i]["parent"])
            assert np.array_equal(z["path_%d" % i], np.zeros((0, 2)) if r2[i]["path"] is None else r2[i]["path"])
        sm = bp.smooth(300)
        for i in range(n):
            if r2[i]["path"] is None:
                assert sm[i] is None
                continue
            rng = oracle.mt_from_pystate((3, r2[i]["rng"], None))
            want = oracle.path_smoothing(r2[i]["path"], 300, DRV, rng)
            assert np.array_equal(sm[i], want), "smoothed path of instance %d" % i
            assert tuple(bp.rng_state(i)[1]) == tuple(rng.mt) + (rng.pos,)
    finally:
        bp.close()


# ------------------------------------------------------------------------------------------------ D
def _rc(L, h, fn, *args):
    return getattr(L, fn)(h._h, *args)


def _plan_getters(L, h, dst):
    """name -> return code of every getter that needs a completed plan, called with valid arguments.  dst: (device
    pointer, bytes) of a device buffer that holds a result table (another handle's)."""
    n32, n64 = C.c_int32(), C.c_int64()
    buf = np.zeros(1 << 16)
    ibuf = np.zeros(1 << 16, dtype=np.int32)
    return {
        "get_tree": _rc(L, h, "rrtx_get_tree", 0, None, None, None, None, 0, C.byref(n32)),
        "get_path": _rc(L, h, "rrtx_get_path", 0, None, 0, C.byref(n32)),
        "get_path_yaw": _rc(L, h, "rrtx_get_path_yaw", 0, None, 0, C.byref(n32)),
        "get_yaw": _rc(L, h, "rrtx_get_yaw", 0, buf.ctypes.data, len(buf)),
        "get_polylines": _rc(L, h, "rrtx_get_polylines", 0, None, 0, None, None, 0, C.byref(n64)),
        "copy_results_device": _rc(L, h, "rrtx_copy_results_device", C.c_void_p(dst[0]), dst[1]),
        "get_sobol_index": _rc(L, h, "rrtx_get_sobol_index", 0, C.byref(n64)),
        "get_trace": _rc(L, h, "rrtx_get_trace", None, None, None, None, 0, C.byref(n32)),
        "get_trace_kind": _rc(L, h, "rrtx_get_trace_kind", ibuf.ctypes.data, len(ibuf), C.byref(n32)),
        "get_smoothed_path": _rc(L, h, "rrtx_get_smoothed_path", 0, None, 0, C.byref(n32)),
        "smooth_planned": _rc(L, h, "rrtx_smooth_planned", 10),
    }


CONTRACT = {"rrt_star": "rrt_star-256", "rrt_star_dubins": "rrt_star_dubins", "bitstar": "bitstar-wave",
            "lqr_rrt_star": "lqr_rrt_star"}
# getters that answer RRTX_E_STATE for this planner at any time (the wrong planner for them)
NEVER = {"rrt_star": {"get_path_yaw", "get_yaw", "get_polylines"},
         "rrt_star_dubins": {"get_path_yaw", "get_trace_kind", "get_smoothed_path", "smooth_planned"},
         "bitstar": {"get_path_yaw", "get_yaw", "get_polylines", "get_trace_kind", "get_smoothed_path", "smooth_planned"},
         "lqr_rrt_star": {"get_path_yaw", "get_yaw", "get_trace_kind"}}


@pytest.mark.parametrize("algo", sorted(CONTRACT))
def test_call_order_contract(gpu, algo):
    """Section D, the call-order paragraph of rrtx.h: getters before the first plan and between plan_begin and the last
    step, setters while a plan is in progress, smoothed paths and traces of an earlier plan, capacities, and
    rrtx_get_rng_state after a new state was staged."""
    import rrt_amd
    A = rrt_amd._abi
    L = A.load()
    P = dict(CASES[CONTRACT[algo]])
    inp = [dict(rng=("seed", 5 + i), obs=P["m1"], start=P["start"], goal=P["goal"]) for i in range(3)]
    refs = [_oracle_one((P["algo"], P["kw"], c)) for c in inp]
    h = _make_handle(P, 3)
    other = _make_handle(P, 3)               # never planned: its result table is the device buffer results are copied into
    try:
        dst = other.results_device_ptr()
        h.set_obstacles(P["m1"])
        h.seed_instances([5, 6, 7])
        h.enable_trace(0)
        # before the first plan
        rcs = _plan_getters(L, h, dst)
        assert all(rc == E_STATE for rc in rcs.values()), rcs
        assert L.rrtx_get_results(h._h, None, None, None) == E_STATE
        pend = C.c_int32()
        assert L.rrtx_plan_step(h._h, C.byref(pend)) == E_STATE
        # a plan in progress: bounded launches, so that it is still in progress after the first step
        h.set_launch_bound(7)
        h.plan_begin()
        rc, pending = h.plan_step()
        assert rc == 0 and pending > 0
        obs = np.ascontiguousarray(np.array(P["m2"], dtype=np.float64))
        # first of all the one that could free the table a running plan reads: refused, or the test ends here -- the handle
        # is closed without another step
        assert L.rrtx_set_obstacles(h._h, obs.ctypes.data, len(obs)) == E_STATE, "rrtx_set_obstacles accepted mid-plan"
        assert "in progress" in h.last_error()
        seeds = np.array([9, 9, 9], dtype=np.uint64)
        offs = np.zeros(4, dtype=np.int32)
        words = np.zeros(624, dtype=np.uint32)
        xy = (C.c_double * 3)(1.0, 1.0, 0.0)
        rot = (C.c_double * 4)(1.0, 0.0, 0.0, 1.0)
        mid = {"set_instance_obstacles": L.rrtx_set_instance_obstacles(h._h, offs.ctypes.data, None),
               "seed_instances": L.rrtx_seed_instances(h._h, 0, 3, seeds.ctypes.data),
               "set_instance": L.rrtx_set_instance(h._h, 1, C.cast(xy, C.c_void_p), None),
               "set_rng_state": L.rrtx_set_rng_state(h._h, 1, words.ctypes.data, 624),
               "set_instance_rotation": L.rrtx_set_instance_rotation(h._h, 1, C.cast(rot, C.c_void_p), 1.0),
               "enable_trace": L.rrtx_enable_trace(h._h, 1),
               "set_launch_bound": L.rrtx_set_launch_bound(h._h, 1000)}
        assert all(rc == E_STATE for rc in mid.values()), mid
        rcs = _plan_getters(L, h, dst)
        assert all(rc == E_STATE for rc in rcs.values()), rcs
        pc, nn, st = h.get_results()                         # valid between steps
        assert len(st) == 3
        steps = 1
        while pending:
            rc, pending = h.plan_step()
            steps += 1
            assert steps < 100000
        assert rc == 0
        # the refused setters changed nothing: the plan is the oracle's for the inputs staged before it
        out = _read(h, P, 3)
        _check(P, out, refs, "plan with refused setters")
        rcs = _plan_getters(L, h, dst)
        ok = {k for k, rc in rcs.items() if rc == 0}
        assert ok == set(rcs) - NEVER[algo] - {"get_smoothed_path"}, rcs
        assert all(rcs[k] == E_STATE for k in NEVER[algo]), rcs
        # trace of instance 0 = the oracle's; then another instance: nothing until a plan has traced it
        _assert_trace(h.get_trace(), refs[0], "trace of instance 0")
        h.enable_trace(2)
        n32 = C.c_int32()
        assert L.rrtx_get_trace(h._h, None, None, None, None, 0, C.byref(n32)) == E_STATE
        smooths = "smooth_planned" not in NEVER[algo]
        if smooths:
            assert L.rrtx_get_smoothed_path(h._h, 0, None, 0, C.byref(n32)) == 0     # smoothed by _plan_getters above
        # item 4: a state staged on a planned handle is not read back before the next plan
        after = [h.get_rng_state(i) for i in range(3)]
        h.seed_instances([15, 16, 17])
        assert [h.get_rng_state(i) for i in range(3)] == after
        if not smooths:                      # (rrtx_smooth_planned above continued the streams of the planners it serves)
            assert tuple(after[1][1]) == tuple(refs[1]["rng"])
        # second plan: other seeds, instance 2 traced
        h.set_launch_bound(ONE_LAUNCH)
        assert h.plan() == 0
        inp2 = [dict(c, rng=("seed", 15 + i)) for i, c in enumerate(inp)]
        refs2 = [_oracle_one((P["algo"], P["kw"], c)) for c in inp2]
        out2 = _read(h, P, 3)
        _check(P, out2, refs2, "second plan")
        assert L.rrtx_get_smoothed_path(h._h, 0, None, 0, C.byref(n32)) == E_STATE     # item 1: not this plan's
        _assert_trace(h.get_trace(), refs2[2], "trace of instance 2")
        # capacities: one short -> RRTX_E_CAPACITY, the needed size in *n_out, nothing written; NULL pointers -> the size
        GUARD = -12345.0
        n_nodes = len(refs2[2]["x"])
        x = np.full(n_nodes + 3, GUARD)
        par = np.full(n_nodes + 3, -777, dtype=np.int32)
        assert L.rrtx_get_tree(h._h, 2, x.ctypes.data, None, None, par.ctypes.data, n_nodes - 1, C.byref(n32)) == E_CAPACITY
        assert n32.value == n_nodes and (x == GUARD).all() and (par == -777).all()
        assert L.rrtx_get_tree(h._h, 2, None, None, None, None, 0, C.byref(n32)) == 0 and n32.value == n_nodes
        assert L.rrtx_get_tree(h._h, 2, x.ctypes.data, None, None, par.ctypes.data, n_nodes, C.byref(n32)) == 0
        assert (x[n_nodes:] == GUARD).all() and (par[n_nodes:] == -777).all() and np.array_equal(x[:n_nodes], refs2[2]["x"])
        with_path = [i for i in range(3) if refs2[i]["path"] is not None]
        for i in with_path[:1]:
            k = len(refs2[i]["path"])
            xy2 = np.full((k + 2, 2), GUARD)
            assert L.rrtx_get_path(h._h, i, xy2.ctypes.data, k - 1, C.byref(n32)) == E_CAPACITY
            assert n32.value == k and (xy2 == GUARD).all()
            assert L.rrtx_get_path(h._h, i, None, 0, C.byref(n32)) == 0 and n32.value == k
            assert L.rrtx_get_path(h._h, i, xy2.ctypes.data, k, C.byref(n32)) == 0
            assert (xy2[k:] == GUARD).all() and np.array_equal(xy2[:k], refs2[i]["path"])
        if "poly_len" in refs2[2]:
            tot = int(refs2[2]["poly_len"].sum())
            n64 = C.c_int64()
            plen = np.full(n_nodes + 2, -777, dtype=np.int32)
            px = np.full(tot + 2, GUARD)
            py = np.full(tot + 2, GUARD)
            for cn, cp in ((n_nodes, tot - 1), (n_nodes - 1, tot)):
                assert L.rrtx_get_polylines(h._h, 2, plen.ctypes.data, cn, px.ctypes.data, py.ctypes.data, cp,
                                            C.byref(n64)) == E_CAPACITY
                assert n64.value == tot and (plen == -777).all() and (px == GUARD).all() and (py == GUARD).all()
            assert L.rrtx_get_polylines(h._h, 2, None, 0, None, None, 0, C.byref(n64)) == 0 and n64.value == tot
            assert L.rrtx_get_polylines(h._h, 2, plen.ctypes.data, n_nodes, px.ctypes.data, py.ctypes.data, tot,
                                        C.byref(n64)) == 0
            assert (plen[n_nodes:] == -777).all() and (px[tot:] == GUARD).all() and np.array_equal(px[:tot], refs2[2]["poly_x"])
        k = len(refs2[2]["trace"][0])
        assert k > 1
        a, b = np.full(k + 2, GUARD), np.full(k + 2, GUARD)
        ne, nr = np.full(k + 2, -777, dtype=np.int32), np.full(k + 2, -777, dtype=np.int32)
        bufs = (a.ctypes.data, b.ctypes.data, ne.ctypes.data, nr.ctypes.data)
        assert L.rrtx_get_trace(h._h, *bufs, k - 1, C.byref(n32)) == E_CAPACITY
        assert n32.value == k and (a == GUARD).all() and (b == GUARD).all() and (ne == -777).all() and (nr == -777).all()
        assert L.rrtx_get_trace(h._h, None, None, None, None, 0, C.byref(n32)) == 0 and n32.value == k
        assert L.rrtx_get_trace(h._h, *bufs, k, C.byref(n32)) == 0
        assert (a[k:] == GUARD).all() and (b[k:] == GUARD).all() and (ne[k:] == -777).all() and (nr[k:] == -777).all()
        _assert_trace((a[:k], b[:k], ne[:k], nr[:k]), refs2[2], "trace read with an exact capacity")
        if algo == "rrt_star":
            states = [h.get_rng_state(i) for i in range(3)]
            h.smooth_planned(100)
            import oracle
            for i in with_path:
                want = oracle.path_smoothing(refs2[i]["path"], 100, P["m1"], oracle.mt_from_pystate(states[i]))
                k = len(want)
                s = np.full((k + 2, 2), GUARD)
                assert L.rrtx_get_smoothed_path(h._h, i, s.ctypes.data, k - 1, C.byref(n32)) == E_CAPACITY
                assert n32.value == k and (s == GUARD).all()
                assert L.rrtx_get_smoothed_path(h._h, i, None, 0, C.byref(n32)) == 0 and n32.value == k
                assert L.rrtx_get_smoothed_path(h._h, i, s.ctypes.data, k, C.byref(n32)) == 0
                assert (s[k:] == GUARD).all() and np.array_equal(s[:k], want), "smoothed path of instance %d" % i
        # the trace switched off
        h.enable_trace(-1)
        assert L.rrtx_get_trace(h._h, None, None, None, None, 0, C.byref(n32)) == E_STATE
    finally:
        h.close()
        other.close()


def _two_plans(P, n=3):
    """A handle on map M1 and the oracle's results for seeds 5.. and 15.. on it."""
    refs = [[_oracle_one((P["algo"], P["kw"], dict(rng=("seed", s0 + i), obs=P["m1"], start=P["start"], goal=P["goal"])))
             for i in range(n)] for s0 in (5, 15)]
    h = _make_handle(P, n)
    h.set_obstacles(P["m1"])
    return h, refs


def test_smoothed_paths_do_not_outlive_their_plan(gpu):
    """rrtx_get_smoothed_path after another rrtx_plan: RRTX_E_STATE until rrtx_smooth_planned has run on THAT plan, then
    that plan's smoothed paths (oracle.path_smoothing continuing each instance's stream) -- never the previous plan's."""
    import oracle
    P = CASES["rrt-mt"]
    h, refs = _two_plans(P)
    try:
        h.seed_instances([5, 6, 7])
        assert h.plan() == 0
        h.smooth_planned(200)
        first = [h.get_smoothed_path(i) for i in range(3)]
        assert any(p is not None for p in first)
        h.seed_instances([15, 16, 17])
        assert h.plan() == 0
        n32 = C.c_int32()
        for i in range(3):
            assert h.L.rrtx_get_smoothed_path(h._h, i, None, 0, C.byref(n32)) == E_STATE, \
                "instance %d: the smoothed path of the previous plan is handed out (%d points)" % (i, n32.value)
        states = [h.get_rng_state(i) for i in range(3)]
        h.smooth_planned(200)
        for i in range(3):
            got = h.get_smoothed_path(i)
            if refs[1][i]["path"] is None:
                assert got is None
            else:
                want = oracle.path_smoothing(refs[1][i]["path"], 200, P["m1"], oracle.mt_from_pystate(states[i]))
                assert np.array_equal(got, want), "instance %d" % i
    finally:
        h.close()


@pytest.mark.parametrize("name", ["rrt_star-256", "bitstar-wave"])
def test_trace_getters_wait_for_a_plan_that_traced_the_instance(gpu, name):
    """rrtx_enable_trace on a planned handle (first time, or another instance): the trace getters return RRTX_E_STATE, not
    rows that were never recorded for that instance, until the next plan completes; then the oracle's trace of it."""
    P = CASES[name]
    h, refs = _two_plans(P)
    n32 = C.c_int32()
    try:
        h.seed_instances([5, 6, 7])
        assert h.plan() == 0
        h.enable_trace(1)                    # nothing was traced by the plan above
        assert h.L.rrtx_get_trace(h._h, None, None, None, None, 0, C.byref(n32)) == E_STATE, \
            "%d rows of a trace that no plan recorded" % n32.value
        h.seed_instances([15, 16, 17])
        assert h.plan() == 0
        _assert_trace(h.get_trace(), refs[1][1], "trace of instance 1")
        h.enable_trace(2)                    # the rows on the device are instance 1's
        assert h.L.rrtx_get_trace(h._h, None, None, None, None, 0, C.byref(n32)) == E_STATE
        h.enable_trace(1)                    # ... and still are
        _assert_trace(h.get_trace(), refs[1][1], "trace of instance 1")
        h.enable_trace(-1)
        assert h.L.rrtx_get_trace(h._h, None, None, None, None, 0, C.byref(n32)) == E_STATE
    finally:
        h.close()

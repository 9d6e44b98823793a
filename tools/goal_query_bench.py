"""Many goals per planned tree: BatchPlanner.query_goals on one device, beside the plain-Python rules on one core.

    python tools/goal_query_bench.py [--instances 4096] [--goals 256] [--reps 5] [--sample 64]

Two batches of --instances seeds, each planned once: the rrt_04 driver scene (tests/golden/rrt04_drv_mt_s1234.npz) at 500
iterations and the rrt_06 driver scene (rrt06_drv_s42_it200.npz) at 200.  The goals are a square grid of --goals points over
rand_area, shared by all instances; the rrt_06 queries take the grid points at yaw 0 with thresholds widened to
goal_xy_th = 1.5 and goal_yaw_th = 0.6 so that paths are found.  Per batch:
  records   query_goals(goals, paths=False): the HIP-event time of the solve launch (median of --reps calls after a
            warm-up) and the wall time of one call
  paths     query_goals(goals): solve + count + gather, kernel time and wall time alike (rrt_06: over the first
            --path-goals grid points only -- its courses are long, and a result is capped at 2^28 points)
  oracle    tests/goal_query_oracle.py on tree(i) for --sample of the same queries, one core: ms per query.  The sampled
            answers are compared with the device's before anything is reported.
Prints one JSON line.  Nothing here gates anything."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed_calls(fn, reps):
    """(median kernel ms, median wall ms) of `reps` calls after one warm-up; fn returns a GoalQueryResult."""
    kern, wall = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        if rep:
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(res.kernel_ms)
    return statistics.median(kern), statistics.median(wall), res


def measure(bp, goals, reps, sample, fetch, oracle_query, path_goals, **th):
    n = len(bp.seeds)
    t0 = time.perf_counter()
    bp.plan()
    plan_ms = 1e3 * (time.perf_counter() - t0)
    rk, rw, rec = timed_calls(lambda: bp.query_goals(goals, paths=False, **th), reps)
    pk, pw, full = timed_calls(lambda: bp.query_goals(goals[:path_goals], **th), reps)
    rng = np.random.default_rng(1)
    picks = [(int(rng.integers(n)), int(rng.integers(len(goals)))) for _ in range(sample)]
    data = [fetch(i) for i, _ in picks]                 # the trees come off the device before the clock starts
    t0 = time.perf_counter()
    want = [oracle_query(d, goals[j]) for d, (_, j) in zip(data, picks)]
    oracle_ms = 1e3 * (time.perf_counter() - t0) / max(1, sample)
    for (i, j), w in zip(picks, want):
        assert (rec.node[i, j], rec.status[i, j]) == (w["node"], w["status"]) and rec.cost[i, j] == w["cost"], (i, j)
    return {"instances": n, "goals": len(goals), "queries": n * len(goals), "found": int(rec.found.sum()),
            "nodes_mean": float(np.mean(bp.results()[1])), "plan_wall_ms": plan_ms,
            "records_kernel_ms": rk, "records_wall_ms": rw,
            "paths_goals": int(path_goals), "paths_points": int(full.offsets[-1]), "paths_kernel_ms": pk, "paths_wall_ms": pw,
            "oracle_ms_per_query": oracle_ms, "oracle_sample": sample}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--goals", type=int, default=256)
    ap.add_argument("--path-goals", type=int, default=16, help="rrt_06: goals of the call that gathers the courses")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    import goal_query_oracle as gq
    import rrt_amd
    import util
    seeds = list(range(42, 42 + a.instances))
    side = max(1, int(round(a.goals ** 0.5)))
    out = {"reps": a.reps}

    g = util.load_golden(util.GOLDEN + "/rrt04_drv_mt_s1234.npz")
    kw = util.kwargs_from_golden(g)
    lo, hi = kw["rand_area"]
    axis = np.linspace(lo, hi, side)
    grid = np.array([[x, y] for x in axis for y in axis])
    bp = rrt_amd.BatchPlanner("rrt_star", seeds, kw["start"], kw["goal"], kw["obstacles"], kw["rand_area"],
                              expand_dis=kw["expand_dis"], path_resolution=kw["path_resolution"],
                              goal_sample_rate=kw["goal_sample_rate"], max_iter=500, play_area=kw["play_area"],
                              robot_radius=kw["robot_radius"], search_until_max_iter=True)
    try:
        out["rrt_04"] = measure(bp, grid, a.reps, a.sample, bp.tree,
                                lambda tree, q: gq.query_rrt_star(tree, q, kw["expand_dis"], kw["path_resolution"], kw["obstacles"],
                                                                  kw["robot_radius"], kw["play_area"]), len(grid))
    finally:
        bp.close()

    g = util.load_golden(util.GOLDEN + "/rrt06_drv_s42_it200.npz")
    obst = [tuple(o) for o in g["obstacles"]]
    lo, hi = (float(v) for v in g["rand_area"])
    axis = np.linspace(lo, hi, side)
    poses = np.array([[x, y, 0.0] for x in axis for y in axis])
    th = dict(goal_xy_th=1.5, goal_yaw_th=0.6)
    bp = rrt_amd.BatchPlanner("rrt_star_reeds_shepp", seeds, list(g["start"]), list(g["goal"]), obst, list(g["rand_area"]),
                              expand_dis=3.0, goal_sample_rate=10, max_iter=200, robot_radius=0.6, search_until_max_iter=True,
                              curvature=2.0, step_size=0.1)
    try:
        def fetch(i):
            x, y, cost, parent = bp.tree(i)
            return (x, y, bp.yaw(i), cost, parent), bp.polylines(i)

        def pose_oracle(data, q):
            return gq.query_pose(data[0], data[1], q, list(g["start"]), 1.5, 0.6, False)
        out["rrt_06"] = measure(bp, poses, a.reps, a.sample, fetch, pose_oracle, min(a.path_goals, len(poses)), **th)
        out["rrt_06"].update(th)
    finally:
        bp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

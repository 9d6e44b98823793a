"""Reading a planned batch: the per-instance getters against one gather on the device, in one process on one device.

    python tools/course_bench.py [--instances 4096] [--reps 5] [--T 100.0]

Two batches of --instances seeds: the rrt_06 driver scene (tests/golden/rrt06_drv_s42_it200.npz) at 200 iterations and the
rrt_04 driver scene (rrt04_drv_mt_s1234.npz) at 500.  Each is planned once; then, per way, the median wall time of --reps
reads after one warm-up:
  loop     [bp.path(i) for i in range(n)]: rrtx_get_path (+ rrtx_get_path_yaw) per instance -- the only way before
           rrtx_gather_courses existed, and still in the build
  gather   bp.courses(): one gather per handle, one copy per column
  chain    (rrt_06 only) bp.courses(order="driving", arrays="device") followed by BatchTrack.run(..., select=found,
           arrays=False): the courses never leave the device
and the HIP-event time of the gather's two kernels.  The loop and the gather are compared point for point before anything
is timed.  Prints one JSON line.  Nothing here gates anything."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def median_ms(fn, reps):
    out = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:      # the first run warms up
            out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def measure(bp, reps, track=None):
    n = len(bp.seeds)
    t0 = time.perf_counter()
    bp.plan()
    plan_ms = 1e3 * (time.perf_counter() - t0)
    ref = [bp.path(i) for i in range(n)]
    c = bp.courses()
    for i, p in enumerate(ref):
        q = c.course(i)
        assert (p is None) == (q is None) and (p is None or np.array_equal(p, q)), i
    kern = []

    def gather():
        kern.append(bp.courses().kernel_ms)
    out = {"instances": n, "found": int(c.found.sum()), "points": int(c.offsets[-1]), "plan_wall_ms": plan_ms,
           "loop_wall_ms": median_ms(lambda: [bp.path(i) for i in range(n)], reps), "gather_wall_ms": median_ms(gather, reps),
           "gather_kernel_ms": statistics.median(kern[1:])}
    if track is not None:
        bt, kw = track

        def chain():
            d = bp.courses(order="driving", arrays="device")
            return bt.run(d, select=d.found, arrays=False, **kw)
        out["chain_wall_ms"] = median_ms(chain, reps)
        res = chain()
        out["chain_tracked"] = int(np.sum(res.status != 5))
        out["chain_feasible"] = int(np.sum(res.find_goal[res.status == 0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--T", type=float, default=100.0, help="the tracker's time limit per roll-out (the model global T)")
    a = ap.parse_args()
    import rrt_amd
    import util
    seeds = list(range(42, 42 + a.instances))
    out = {"reps": a.reps, "T": a.T}
    g = util.load_golden(util.GOLDEN + "/rrt06_drv_s42_it200.npz")
    obst = [tuple(o) for o in g["obstacles"]]
    bp = rrt_amd.BatchPlanner("rrt_star_reeds_shepp", seeds, list(g["start"]), list(g["goal"]), obst, list(g["rand_area"]),
                              expand_dis=3.0, goal_sample_rate=10, max_iter=200, robot_radius=0.6, search_until_max_iter=True,
                              curvature=2.0, step_size=0.1)
    try:
        with rrt_amd.BatchTrack(T=a.T) as bt:
            out["rrt_06"] = measure(bp, a.reps, (bt, dict(obstacle_list=obst, robot_radius=0.6)))
    finally:
        bp.close()
    g = util.load_golden(util.GOLDEN + "/rrt04_drv_mt_s1234.npz")
    kw = util.kwargs_from_golden(g)
    bp = rrt_amd.BatchPlanner("rrt_star", seeds, kw["start"], kw["goal"], kw["obstacles"], kw["rand_area"],
                              expand_dis=kw["expand_dis"], path_resolution=kw["path_resolution"],
                              goal_sample_rate=kw["goal_sample_rate"], max_iter=500, play_area=kw["play_area"],
                              robot_radius=kw["robot_radius"], search_until_max_iter=True)
    try:
        out["rrt_04"] = measure(bp, a.reps)
    finally:
        bp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

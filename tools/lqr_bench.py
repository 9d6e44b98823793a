"""Throughput of LQR-RRT* (rrt_09) on one GPU: plans per second for a batch of independent instances.

    python tools/lqr_bench.py [--instances 4096] [--runs 5] [--warmup 1] [--c2-iter 3000] [--oracle-plans 2]

Two workloads: the reference's driver cell (start (0, 0), goal (6, 10), its seven obstacles, Sobol sampler, 500
iterations, all of them run: planning()'s default search_until_max_iter=True) with per-instance seeds, and a C2-like map
(tests/util.c2_kwargs: its 50-obstacle map on [0, 100]^2, start (2, 2), goal (98, 98), expand_dis 2, MT sampler) at
about 3 000 iterations.  Kernel time is the HIP-event time the library records for its planner launches
(rrtx_stats.kernel_ms); a warm-up plan first, then the median of several timed plans.  CPU baseline: the pure-Python
oracle (tests/lqr_oracle.py) on this host, single core, labelled as such -- it restates the reference statement by
statement, so its per-plan time is of the reference's order (the reference itself is not run here).  Prints one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import util  # noqa: E402
import lqr_oracle  # noqa: E402
import rrt_amd  # noqa: E402

DRV_OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]


def workloads(c2_iter):
    drv = dict(start=[0, 0], goal=[6.0, 10.0], obstacle_list=DRV_OBS, rand_area=[-2, 15], expand_dis=3.0,
               goal_sample_rate=10, max_iter=500, sobol_sampler=True, connect_circle_dist=50.0, goal_xy_th=0.5,
               step_size=0.2)
    c2 = util.c2_kwargs(c2_iter)
    c2w = dict(start=list(c2["start"]), goal=list(c2["goal"]), obstacle_list=[tuple(o) for o in c2["obstacles"]],
               rand_area=list(c2["rand_area"]), expand_dis=c2["expand_dis"], goal_sample_rate=c2["goal_sample_rate"],
               max_iter=c2_iter, sobol_sampler=False, connect_circle_dist=50.0, goal_xy_th=0.5, step_size=0.2)
    return {"driver_cell": drv, "c2_like": c2w}


def gpu_run(kw, n, runs, warmup):
    seeds = list(range(1, n + 1))
    kms, walls = [], []
    for r in range(warmup + runs):
        bp = rrt_amd.BatchPlanner("lqr_rrt_star", seeds, kw["start"], kw["goal"], kw["obstacle_list"], kw["rand_area"],
                                  expand_dis=kw["expand_dis"], goal_sample_rate=kw["goal_sample_rate"],
                                  max_iter=kw["max_iter"], sobol_sampler=kw["sobol_sampler"],
                                  connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=True,
                                  goal_xy_th=kw["goal_xy_th"], step_size=kw["step_size"])
        try:
            t0 = time.perf_counter()
            _, nn, st = bp.plan()
            wall = time.perf_counter() - t0
            s = bp.stats()
        finally:
            bp.close()
        if r >= warmup:
            kms.append(s["kernel_ms"])
            walls.append(wall)
    k = statistics.median(kms)
    return dict(instances=n, kernel_ms_median=k, kernel_ms_runs=kms, plan_s_median=statistics.median(walls),
                plans_per_s_kernel=n / (k / 1e3), mean_nodes=float(nn.mean()), failed=int(((st & 4) | (st & 32) != 0).sum()))


def oracle_run(kw, plans):
    okw = {k: v for k, v in kw.items()}
    t = []
    for s in range(1, plans + 1):
        o = lqr_oracle.LQROracle(**okw)
        rng = random.Random(s)
        t0 = time.perf_counter()
        o.planning(rng, True)
        t.append(time.perf_counter() - t0)
    return dict(plans=plans, s_per_plan=statistics.median(t), plans_per_s=1.0 / statistics.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--c2-instances", type=int, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--c2-iter", type=int, default=3000)
    ap.add_argument("--oracle-plans", type=int, default=2)
    a = ap.parse_args()
    out = {"metric": "lqr_rrt_star_plans_per_s"}
    for name, kw in workloads(a.c2_iter).items():
        n = a.instances if name == "driver_cell" or a.c2_instances is None else a.c2_instances
        r = gpu_run(kw, n, a.runs, a.warmup)
        if a.oracle_plans > 0:
            r["cpu_python_oracle_1core"] = oracle_run(kw, a.oracle_plans)
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Throughput of BatchArmNav on one GPU: occupancy-grid cells per second over a sweep of scenes, and searches per second over
a sweep of queries.

    python tools/armnav_bench.py [--scenes 1,64,4096] [--queries 1,1024,65536] [--runs 5] [--warmup 1] [--oracle-queries 200]

The scenes: the arm of the script's driver cell (5 links) at M = 100, the first scene with the driver's five circles, the others
with five seeded random circles each.  The queries: seeded random start / goal pairs on the driver grid, marks=False.  Kernel
time is the HIP-event time the library records (trig + grid kernels; search kernel, both passes when the route pool had to
grow); a warm-up first, then the median of several runs.  wall_s is one occupancy() / plan() end to end: packing, upload,
kernels, and the copy of the grids / routes back.  CPU baseline: the pure-Python oracle (tests/armnav_oracle.py) on this host,
single core, on one scene and on the first few hundred of the same queries, labelled as such -- the reference itself is not
run here.  Nothing is promised and nothing gates.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import armnav_oracle  # noqa: E402
import rrt_amd  # noqa: E402

M = 100
LINKS = [0.5, 0.5, 0.3, 0.5, 0.1]
OBSTACLES = [[1.75, 0.75, 0.6], [0.55, 1.5, 0.5], [0, -1, 0.7], [0, -0.6, 0.4], [-1, 1., 0.3]]


def median_of(call, runs, warmup):
    kms, walls, res = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        res, ms = call()
        wall = time.perf_counter() - t0
        if r >= warmup:
            kms.append(ms)
            walls.append(wall)
    return statistics.median(kms), statistics.median(walls), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="1,64,4096")
    ap.add_argument("--queries", default="1,1024,65536")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-queries", type=int, default=200)
    a = ap.parse_args()
    rs = np.random.RandomState(20261019)
    n_max = max(int(v) for v in a.scenes.split(","))
    layouts = [OBSTACLES] + [np.stack([rs.uniform(-2, 2, 5), rs.uniform(-2, 2, 5), rs.uniform(0.2, 0.7, 5)], axis=1).tolist()
                             for _ in range(n_max - 1)]
    q_max = max(int(v) for v in a.queries.split(","))
    starts, goals = rs.randint(0, M, (q_max, 2)), rs.randint(0, M, (q_max, 2))
    out = {"metric": "armnav", "M": M, "links": len(LINKS), "circles_per_scene": 5, "occupancy": [], "plan": []}
    with rrt_amd.BatchArmNav(M=M) as nav:
        for n in (int(v) for v in a.scenes.split(",")):
            k, w, grids = median_of(lambda: (nav.occupancy(LINKS, layouts[:n]), nav.grid_ms), a.runs, a.warmup)
            out["occupancy"].append(dict(scenes=n, kernel_ms_median=k, wall_s_median=w, cells_per_s_kernel=n * M * M / (k / 1e3),
                                         occupied_fraction=float(grids.mean())))
        grid = nav.occupancy(LINKS, [OBSTACLES])[0]
        for n in (int(v) for v in a.queries.split(",")):
            def call():
                r = nav.plan(starts[:n], goals[:n], marks=False)
                return r, r.kernel_ms
            k, w, res = median_of(call, a.runs, a.warmup)
            out["plan"].append(dict(queries=n, kernel_ms_median=k, wall_s_median=w, queries_per_s_kernel=n / (k / 1e3),
                                    cells_closed=int(res.pops.sum()), cells_closed_per_s_kernel=float(res.pops.sum()) / (k / 1e3),
                                    found_fraction=float(res.found.mean())))
    if a.oracle_queries > 0:
        t0 = time.perf_counter()
        og = np.array(armnav_oracle.occupancy_grid(LINKS, OBSTACLES, M), dtype=np.uint8)
        dt_grid = time.perf_counter() - t0
        k = min(a.oracle_queries, q_max)
        t0 = time.perf_counter()
        routes = [armnav_oracle.search(og, starts[i], goals[i])[0] for i in range(k)]
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(og, grid)) and all(routes[i] == res.route(i) for i in range(min(k, len(res))))
        out["cpu_python_oracle_1core"] = dict(grid_seconds=dt_grid, grid_cells_per_s=M * M / dt_grid, queries=k, search_seconds=dt,
                                              queries_per_s=k / dt, equals_device=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Throughput of BatchArmIK on one GPU: inverse-kinematics iterations and queries per second on the driver arm.

    python tools/armik_bench.py [--queries 65536] [--max-iterations 10000] [--runs 5] [--warmup 1] [--oracle-queries 500]

The batch: the arm and the start angles of the script's driver cell (5 links), seeded goals from the area of get_random_goal
(the square of side 15 round the origin), max_iterations = 10 000.  Kernel time is the HIP-event time the library records; a
warm-up first, then the median of several runs; wall_s is one solve() / move() end to end (packing, upload, kernel, copies
back).  Reported: the default number of persistent waves; the same batch with one lane per query (queries / 64 waves, no lane
ever refills) as the cost of the tail, and with a quarter of those waves (every lane refills about three times); move() on the found queries with and without the trajectory arrays; and the pure-Python
oracle (tests/armik_oracle.py) on one core of this host on the first few hundred of the same goals, labelled as such -- the
reference itself is not run here.  Nothing is promised and nothing gates.  Prints one JSON line.
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

import armik_oracle  # noqa: E402
import rrt_amd  # noqa: E402

LINKS = [0.5, 1.5, 1.8, 1.2, 0.5]
ANGLES = [1.6, -1.6, 0.8, -0.5, 0.6]


def median_of(call, runs, warmup):
    kms, walls, res = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        res = call()
        wall = time.perf_counter() - t0
        if r >= warmup:
            kms.append(res.kernel_ms)
            walls.append(wall)
    return statistics.median(kms), statistics.median(walls), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--max-iterations", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-queries", type=int, default=500)
    a = ap.parse_args()
    rs = np.random.RandomState(20261019)
    Q = a.queries
    goals = 15.0 * rs.random_sample((Q, 2)) - 7.5
    out = {"metric": "armik", "links": len(LINKS), "queries": Q, "max_iterations": a.max_iterations}
    with rrt_amd.BatchArmIK(max_iterations=a.max_iterations) as ik:
        res = None
        for name, waves in (("solve_default_waves", None), ("solve_one_lane_per_query", (Q + 63) // 64),
                            ("solve_four_queries_per_lane", max(1, (Q + 255) // 256))):
            ik.waves = waves
            k, w, res = median_of(lambda: ik.solve(LINKS, ANGLES, goals), a.runs, a.warmup)
            trips = int(res.iterations.sum())   # by the iteration counts the records report
            out[name] = dict(waves=res.waves, kernel_ms_median=k, wall_s_median=w, iterations=trips,
                             iterations_per_s_kernel=trips / (k / 1e3), queries_per_s_kernel=Q / (k / 1e3),
                             found_fraction=float(res.found.mean()), at_the_cap_fraction=float((res.iterations == a.max_iterations).mean()))
        idx = np.nonzero(res.found)[0]
        starts = np.tile(ANGLES, (len(idx), 1))
        for name, arrays in (("move_with_arrays", True), ("move_records_only", False)):
            k, w, mv = median_of(lambda: ik.move(LINKS, starts, res.angles[idx], goals[idx], arrays=arrays), a.runs, a.warmup)
            steps = int(mv.n_steps.sum())
            out[name] = dict(queries=len(idx), kernel_ms_median=k, wall_s_median=w, steps=steps, steps_per_s_kernel=steps / (k / 1e3),
                             reached_fraction=float(mv.reached.mean()))
    if a.oracle_queries > 0:
        n = min(a.oracle_queries, Q)
        t0 = time.perf_counter()
        ora = [armik_oracle.solve(LINKS, ANGLES, goals[i], 0.1, a.max_iterations) for i in range(n)]
        dt = time.perf_counter() - t0
        trips = sum(o["iterations"] for o in ora)
        same = all(o["status"] == int(res.status[i]) and o["iterations"] == int(res.iterations[i]) and
                   np.array_equal(np.array(o["angles"]), res.angles[i], equal_nan=True) for i, o in enumerate(ora))
        out["cpu_python_oracle_1core"] = dict(queries=n, seconds=dt, iterations=trips, iterations_per_s=trips / dt, queries_per_s=n / dt,
                                              equals_device=bool(same))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

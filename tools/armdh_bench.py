"""Throughput of BatchArmDH on one GPU: inverse-kinematics trips and targets per second on the script's 6-axis arm.

    python tools/armdh_bench.py [--queries 65536] [--iter-cnt 500] [--runs 5] [--warmup 1] [--oracle-queries 200]

The batch: the arm of the script's driver cell, seeded starts in [-1, 1]^6, and as targets the poses (a forward pass of the device)
of configurations within 0.5 rad of the starts; 500 trips of theta += step / 200, newton and lm (eps = 1e-5).  Kernel time is the
HIP-event time the library records; a warm-up first, then the median of several runs; wall_s is one solve() end to end (packing,
upload, kernel, copies back).  Beside it the pure-Python oracle (tests/armdh_oracle.py) on one core of this host on the first
few hundred of the same targets, labelled as such -- the reference itself is not run here.  Nothing is promised and nothing gates.
Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import armdh_oracle  # noqa: E402
import rrt_amd  # noqa: E402

HP = math.pi / 2.
ARM = [[0., HP, 0., 0.13156], [0., 0., -0.1104, 0.], [0., 0., -0.096, 0.], [0., HP, 0., 0.06639], [0., -HP, 0., 0.07318], [0., 0., 0., 0.0436]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--iter-cnt", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-queries", type=int, default=200)
    a = ap.parse_args()
    rs = np.random.RandomState(20261019)
    Q = a.queries
    starts = rs.uniform(-1.0, 1.0, (Q, 6))
    near = starts + rs.uniform(-0.5, 0.5, (Q, 6))
    out = {"metric": "armdh", "links": 6, "queries": Q, "iter_cnt": a.iter_cnt, "step_div": 200.0}
    with rrt_amd.BatchArmDH() as dh:
        t0 = time.perf_counter()
        fw = dh.forward(ARM, near)
        out["forward"] = dict(kernel_ms=fw.kernel_ms, wall_s=time.perf_counter() - t0)
        refs = np.ascontiguousarray(np.concatenate([fw.position, fw.euler2], axis=1))
        for method in ("newton", "lm"):
            kms, walls, res = [], [], None
            for r in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                res = dh.solve(ARM, starts, refs, iter_cnt=a.iter_cnt, method=method)
                wall = time.perf_counter() - t0
                if r >= a.warmup:
                    kms.append(res.kernel_ms)
                    walls.append(wall)
            k, w = statistics.median(kms), statistics.median(walls)
            trips = Q * a.iter_cnt
            rec = dict(kernel_ms_median=k, wall_s_median=w, trips_per_s_kernel=trips / (k / 1e3), targets_per_s_kernel=Q / (k / 1e3),
                       ok_fraction=float(res.ok.mean()), pose_error_median=float(np.median(np.max(np.abs(res.pose_error), axis=1))),
                       kappa_max_median=float(np.median(res.kappa_max)))
            n = min(a.oracle_queries, Q)
            if n > 0:
                t0 = time.perf_counter()
                ora = [armdh_oracle.solve([[starts[i][j]] + ARM[j][1:] for j in range(6)], refs[i].tolist(), a.iter_cnt, 200.0, method, 1e-5)
                       for i in range(n)]
                dt = time.perf_counter() - t0
                same = all(o["status"] == int(res.status[i]) and np.array_equal(np.array(o["angles"]), res.angles[i], equal_nan=True)
                           for i, o in enumerate(ora))
                rec["cpu_python_oracle_1core"] = dict(queries=n, seconds=dt, trips_per_s=n * a.iter_cnt / dt, targets_per_s=n / dt,
                                                      equals_device=bool(same))
            out[method] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Throughput of BatchSpline on one GPU: spline-course points per second for a batch of waypoint lists.

    python tools/spline_bench.py [--courses 65536] [--runs 5] [--warmup 1] [--oracle-courses 2000]

The batch: seeded random courses of 8 to 40 waypoints with chords of 0.5 to 2.5 (about 36 m and 360 points each at ds = 0.1),
solve="device".  Three shapes: records only (the fit kernel alone), with arrays (fit + evaluation, five doubles stored per
point), and records + hits against 50 circles (fit + evaluation + collision check, nothing stored).  Kernel time is the
HIP-event time the library records for its two kernels (SplineResult.kernel_ms); a warm-up run first, then the median of
several timed runs.  wall_s is one run() with arrays end to end: packing, upload, both kernels, the prefix sum on the host and
the copy of the arrays back.  CPU baseline: the pure-Python oracle (tests/spline_oracle.py) on this host, single core, on the
first few thousand of the same courses, labelled as such -- it restates the reference statement by statement, so its
rate is of the reference's order (the reference itself is not run here).  Prints one JSON line.
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

import spline_oracle  # noqa: E402
import rrt_amd  # noqa: E402


def make_batch(n, seed=20261019):
    rs = np.random.RandomState(seed)
    m = rs.randint(8, 41, n)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(m)
    W = int(off[-1])
    course = np.repeat(np.arange(n), m)
    first = np.zeros(W, dtype=bool)
    first[off[:-1]] = True

    def cumsum_per_course(v):
        c = np.cumsum(v)
        base = (c - v)[off[:-1]]
        return c - base[course]
    th = cumsum_per_course(np.where(first, rs.uniform(0, 2 * np.pi, W), rs.uniform(-1.0, 1.0, W)))
    step = rs.uniform(0.5, 2.5, W)
    x = cumsum_per_course(step * np.cos(th)) + rs.uniform(0, 100, n)[course]
    y = cumsum_per_course(step * np.sin(th)) + rs.uniform(0, 100, n)[course]
    obs = np.stack([rs.uniform(0, 100, 50), rs.uniform(0, 100, 50), rs.uniform(0.5, 2.0, 50)], axis=1)
    return off, x, y, obs


def timed(bs, csr, runs, warmup, **kw):
    kms, walls, res = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        res = bs.run(csr, ds=0.1, **kw)
        wall = time.perf_counter() - t0
        if r >= warmup:
            kms.append(res.kernel_ms)
            walls.append(wall)
    k = statistics.median(kms)
    pts = int(res.n_points.sum())
    return dict(kernel_ms_median=k, kernel_ms_runs=kms, wall_s_median=statistics.median(walls), points=pts,
                points_per_s_kernel=pts / (k / 1e3)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--courses", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-courses", type=int, default=2000)
    a = ap.parse_args()
    off, x, y, obs = make_batch(a.courses)
    csr = (off, x, y)
    out = {"metric": "spline_points_per_s", "courses": a.courses, "waypoints": int(off[-1]), "ds": 0.1}
    with rrt_amd.BatchSpline() as bs:
        out["records_only"], _ = timed(bs, csr, a.runs, a.warmup, arrays=False)
        out["with_arrays"], res = timed(bs, csr, a.runs, a.warmup)
        out["hits_50_obstacles"], hits = timed(bs, csr, a.runs, a.warmup, arrays=False, obstacle_list=obs.tolist(), robot_radius=0.3)
    out["free_fraction"] = float(np.mean(hits.free))
    out["partial"] = int(np.sum(res.status != 0))
    if a.oracle_courses > 0:
        k = min(a.oracle_courses, a.courses)
        courses = [(x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]) for i in range(k)]
        t0 = time.perf_counter()
        o = spline_oracle.batch(courses, 0.1, "thomas")
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(o["x"].view(np.uint64), res.x[:len(o["x"])].view(np.uint64))
                    and np.array_equal(o["k"].view(np.uint64), res.k[:len(o["k"])].view(np.uint64)))
        out["cpu_python_oracle_1core"] = dict(courses=k, points=int(o["offsets"][-1]), seconds=dt,
                                              points_per_s=float(o["offsets"][-1] / dt), equals_device=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

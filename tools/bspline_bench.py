"""Throughput of BatchBSpline on one GPU: B-spline course points per second for a batch of waypoint lists.

    python tools/bspline_bench.py [--courses 65536] [--runs 5] [--warmup 1] [--oracle-courses 300]

The batch: seeded random courses of 8 to 40 waypoints with chords of 0.5 to 2.5, degrees 1 .. 5 in turn.  Two entry points:
interpolate() with 100 points per course, and spline2d() with ds = 0.1 (kinds linear / quadratic / cubic in turn, about 360
points per course).  Three shapes each: records only (the fit kernel alone), with arrays (fit + evaluation, five doubles stored
per point), and records + hits against 50 circles (fit + evaluation + collision check, nothing stored).  Kernel time is the
HIP-event time the library records for its two kernels (BSplineResult.kernel_ms); a warm-up run first, then the median of
several timed runs.  wall_s is one call with arrays end to end.  CPU baseline: the pure-Python oracle
(tests/bspline_oracle.py) on this host, single core, on the first few hundred of the same courses, labelled as such.  Prints
one JSON line.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bspline_oracle  # noqa: E402
import rrt_amd  # noqa: E402
from spline_bench import make_batch  # noqa: E402


def timed(call, runs, warmup, **kw):
    kms, walls, res = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        res = call(**kw)
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
    ap.add_argument("--oracle-courses", type=int, default=300)
    a = ap.parse_args()
    off, x, y, obs = make_batch(a.courses)
    csr = (off, x, y)
    deg = (1 + np.arange(a.courses) % 5).astype(np.int32)
    kinds = [("linear", "quadratic", "cubic")[i % 3] for i in range(a.courses)]
    out = {"metric": "bspline_points_per_s", "courses": a.courses, "waypoints": int(off[-1])}
    with rrt_amd.BatchBSpline() as bb:
        for name, call in (("interpolate_100_points", lambda **kw: bb.interpolate(csr, 100, degree=deg, **kw)),
                           ("spline2d_ds_0.1", lambda **kw: bb.spline2d(csr, ds=0.1, kind=kinds, **kw))):
            o = {}
            o["records_only"], _ = timed(call, a.runs, a.warmup, arrays=False)
            o["with_arrays"], res = timed(call, a.runs, a.warmup)
            o["hits_50_obstacles"], hits = timed(call, a.runs, a.warmup, arrays=False, obstacle_list=obs.tolist(), robot_radius=0.3)
            o["free_fraction"] = float(np.mean(hits.free))
            o["partial"] = int(np.sum(res.status != 0))
            if a.oracle_courses > 0:
                k = min(a.oracle_courses, a.courses)
                courses = [(x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]) for i in range(k)]
                t0 = time.perf_counter()
                if name.startswith("interpolate"):
                    w = bspline_oracle.batch(courses, deg[:k], bspline_oracle.NORMALISED, n_path_points=100)
                else:
                    w = bspline_oracle.batch(courses, [bspline_oracle.KINDS[q] for q in kinds[:k]], bspline_oracle.CHORD, ds=0.1)
                dt = time.perf_counter() - t0
                same = bool(np.array_equal(w["x"].view(np.uint64), res.x[:len(w["x"])].view(np.uint64))
                            and np.array_equal(w["k"].view(np.uint64), res.k[:len(w["k"])].view(np.uint64)))
                o["cpu_python_oracle_1core"] = dict(courses=k, points=int(w["offsets"][-1]), seconds=dt,
                                                    points_per_s=float(w["offsets"][-1] / dt), equals_device=same)
            out[name] = o
    print(json.dumps(out))


if __name__ == "__main__":
    main()

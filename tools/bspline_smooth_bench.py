"""Throughput of BatchBSpline.approximate on one GPU: smoothing fits per second for a batch of waypoint lists.

    python tools/bspline_smooth_bench.py [--courses 65536] [--runs 5] [--warmup 1] [--oracle-courses 300]

The batch: the seeded random courses of tools/bspline_bench.py, 8 to 40 waypoints with chords of 0.5 to 2.5; degree 3, 100
points per course, s = 0.5 and s = None (each course's waypoint count).  Two shapes each: records only (the fit kernel alone)
and with arrays (fit + evaluation, five doubles stored per point).  Kernel time is the HIP-event time the library records for
its two kernels (BSplineSmoothResult.kernel_ms); a warm-up run first, then the median of several timed runs.  wall_s is one
call with arrays end to end.  CPU baseline: the pure-Python oracle (tests/bspline_smooth_oracle.py) on this host, single core,
on the first few hundred of the same courses, labelled as such.  Prints one JSON line.  Nothing here is a promise or a gate.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bspline_smooth_oracle  # noqa: E402
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
    return dict(kernel_ms_median=k, kernel_ms_runs=kms, wall_s_median=statistics.median(walls), points=int(res.n_points.sum()),
                fits_per_s_kernel=2 * len(res) / (k / 1e3)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--courses", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-courses", type=int, default=300)
    a = ap.parse_args()
    off, x, y, _ = make_batch(a.courses)
    csr = (off, x, y)
    out = {"metric": "bspline_smooth_axis_fits_per_s", "courses": a.courses, "waypoints": int(off[-1]), "degree": 3}
    warnings.simplefilter("ignore", RuntimeWarning)      # axes whose root search stops early are counted below
    with rrt_amd.BatchBSpline() as bb:
        for name, s in (("s_0.5", 0.5), ("s_none", None)):
            def call(**kw):
                return bb.approximate(csr, 100, degree=3, s=s, **kw)
            o = {}
            o["records_only"], _ = timed(call, a.runs, a.warmup, arrays=False)
            o["with_arrays"], res = timed(call, a.runs, a.warmup)
            o["partial"] = int(np.sum(res.status != 0))
            ier = np.concatenate(res.ier)
            o["ier_counts"] = {str(int(v)): int(c) for v, c in zip(*np.unique(ier, return_counts=True))}
            o["mean_knots"] = float(np.mean(np.concatenate([np.diff(q) for q in res.knot_offsets])))
            o["mean_rounds"] = float(np.mean(np.concatenate(res.rounds)))
            o["mean_root_steps"] = float(np.mean(np.concatenate(res.iters)))
            if a.oracle_courses > 0:
                k = min(a.oracle_courses, a.courses)
                courses = [(x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]) for i in range(k)]
                t0 = time.perf_counter()
                w = bspline_smooth_oracle.batch(courses, n_path_points=100, degree=3, s=s)
                dt = time.perf_counter() - t0
                nc = int(w["axis0"]["coef_offsets"][-1])
                same = bool(np.array_equal(w["x"].view(np.uint64), res.x[:len(w["x"])].view(np.uint64))
                            and np.array_equal(w["k"].view(np.uint64), res.k[:len(w["k"])].view(np.uint64))
                            and np.array_equal(w["axis0"]["coefficients"].view(np.uint64), res.coefficients[0][:nc].view(np.uint64)))
                o["cpu_python_oracle_1core"] = dict(courses=k, seconds=dt, fits_per_s=2 * k / dt, equals_device=same)
            out[name] = o
    print(json.dumps(out))


if __name__ == "__main__":
    main()

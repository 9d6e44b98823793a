"""Throughput of BatchSpline.query on one GPU: pointwise queries per second against fitted cubic splines.

    python tools/spline_query_bench.py [--runs 5] [--warmup 1] [--oracle-queries 20000] [--small]

Two shapes, solve="device", parameters uniform between the first and the last knot (every one is answered):
  many_courses  65 536 seeded courses of 8 to 40 waypoints (tools/spline_bench.py's batch), 64 queries each
  one_long      one course of 4 096 waypoints, 2^22 queries
each timed without and with derivatives (4 and 8 planes stored).  Kernel time is the HIP-event time the library records for
spline_query_kernel (SplineQueryResult.kernel_ms): a warm-up call first, then the median of several timed calls; the wall
time beside it is one query() end to end -- packing, upload of the parameters, the kernel, the copy of every plane back.  CPU
baseline: the pure-Python oracle (tests/spline_query_oracle.py) on this host, single core, on the first queries of the same
batch, labelled as such -- it restates the reference statement by statement, so its rate is of the reference's order (the
reference itself is not run here).  --small divides both shapes by 64 (a functional run).  Prints one JSON line.
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

import spline_query_oracle as QO  # noqa: E402
import rrt_amd  # noqa: E402
from spline_bench import make_batch  # noqa: E402


def timed(bs, q, runs, warmup, derivatives):
    kms, walls, res = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        res = bs.query(q, derivatives=derivatives)
        wall = time.perf_counter() - t0
        if r >= warmup:
            kms.append(res.kernel_ms)
            walls.append(wall)
    k = statistics.median(kms)
    n = len(res.s)
    return dict(kernel_ms_median=k, kernel_ms_runs=kms, wall_s_median=statistics.median(walls), queries=n,
                queries_per_s_kernel=n / (k / 1e3), answered=int(np.sum(res.valid))), res


def shape(bs, csr, per_course, a, seed):
    off, x, y = csr
    n = len(off) - 1
    fit = bs.fit(csr)
    rs = np.random.RandomState(seed)
    q_off = np.arange(n + 1, dtype=np.int64) * per_course
    t = rs.uniform(0.0, 1.0, n * per_course) * np.repeat(fit.total_length, per_course)
    t = np.minimum(t, np.repeat(np.nextafter(fit.total_length, 0.0), per_course))
    out = dict(courses=n, waypoints=int(off[-1]), fit_kernel_ms=fit.kernel_ms)
    out["position_yaw_curvature"], _ = timed(bs, (q_off, t), a.runs, a.warmup, False)
    out["with_derivatives"], res = timed(bs, (q_off, t), a.runs, a.warmup, True)
    if a.oracle_queries > 0:
        k = max(1, min(a.oracle_queries // per_course, n)) if per_course < a.oracle_queries else 1
        m = min(per_course, a.oracle_queries)
        t0 = time.perf_counter()
        fits = [QO.fit2d(x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]) for i in range(k)]
        t_fit = time.perf_counter() - t0
        sel = np.concatenate([np.arange(q_off[i], q_off[i] + m) for i in range(k)])
        t0 = time.perf_counter()
        o = QO.batch(fits, np.arange(k + 1) * m, t[sel])
        dt = time.perf_counter() - t0
        same = all(np.array_equal(o[p].view(np.uint64), getattr(res, p)[sel].view(np.uint64)) for p in QO.PLANES[2])
        out["cpu_python_oracle_1core"] = dict(courses=k, queries=len(sel), fit_seconds=t_fit, seconds=dt,
                                              queries_per_s=len(sel) / dt, equals_device=bool(same))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-queries", type=int, default=20000)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    div = 64 if a.small else 1
    out = {"metric": "spline_queries_per_s", "library": os.path.basename(rrt_amd._abi.LIB_PATH)}
    with rrt_amd.BatchSpline() as bs:
        off, x, y, _ = make_batch(65536 // div)
        out["many_courses"] = shape(bs, (off, x, y), 64, a, 1)
        w = 4096 // div
        rs = np.random.RandomState(7)
        th = np.cumsum(rs.uniform(-1.0, 1.0, w))
        step = rs.uniform(0.5, 2.5, w)
        one = (np.array([0, w], dtype=np.int64), np.cumsum(step * np.cos(th)), np.cumsum(step * np.sin(th)))
        out["one_long"] = shape(bs, one, (1 << 22) // div, a, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

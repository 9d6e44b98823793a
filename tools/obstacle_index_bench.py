"""The obstacle check of the batched curves and splines, linear loop against obstacle index.

    python tools/obstacle_index_bench.py [--pairs 65536] [--courses 4096] [--reps 5] [--m 16,50,...] [--out FILE]

Sweeps the number of circles m over maps of [0, 100]^2 in the style of tests/util.synth_map whose radii shrink with the count
(0.3 .. 0.9 at m = 1000, times sqrt(1000 / m): the covered share of the plane stays what it is), and measures, with the index
OFF and ON in turn in one process on one object:
  dubins / rs   BatchSteer.plan(points=False) with the list: the collision-free cost-matrix path
  *_plan_free   BatchSteer.plan_free(points=False): every candidate curve tested
  spline        BatchSpline.run(arrays=False): records and hits
Pose pairs start in [5, 95]^2 with the goal 0.5 .. 4 away, curvature 1, Reeds-Shepp step 0.2; spline courses have 8 waypoints
with chords of 1 .. 3, ds = 0.1.  The figure is HIP-event kernel time of the whole solve (stage 1 and the fill with its check;
for a spline the fit and the evaluation), the median of --reps solves after one warm-up, the two modes alternating.  Both hit
arrays of a row are compared in the same run ("equal").  build_ms is the device time of the three build kernels;
records_per_point is the mean number of index records read per curve point, from the restatement of tests/obsindex_util.py
over a sample of the Dubins curves' own points.  Above --linear-cap circles the linear leg runs on an eighth of the batch and its
time is scaled by 8: the row says so ("linear_scaled").  Prints one JSON line per m, and "crossover": per workload the
smallest m of the sweep from which on the index is not slower.  Needs a device: there is no CPU fallback."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def shrinking_map(seed, m):
    rng = random.Random(seed)
    k = (1000.0 / m) ** 0.5
    return np.array([(rng.uniform(0, 100), rng.uniform(0, 100), rng.uniform(0.3, 0.9) * k) for _ in range(m)])


def pose_pairs(n, seed):
    rs = np.random.RandomState(seed)
    st = np.column_stack([rs.uniform(5, 95, n), rs.uniform(5, 95, n), rs.uniform(-np.pi, np.pi, n)])
    d, a = rs.uniform(0.5, 4.0, n), rs.uniform(-np.pi, np.pi, n)
    return st, np.column_stack([st[:, 0] + d * np.cos(a), st[:, 1] + d * np.sin(a), rs.uniform(-np.pi, np.pi, n)])


def courses(n, seed, wp=8):
    rs = np.random.RandomState(seed)
    th = np.cumsum(rs.uniform(-0.8, 0.8, (n, wp)), axis=1) + rs.uniform(0, 2 * np.pi, (n, 1))
    step = rs.uniform(1.0, 3.0, (n, wp))
    x = np.cumsum(step * np.cos(th), axis=1) + rs.uniform(10, 90, (n, 1))
    y = np.cumsum(step * np.sin(th), axis=1) + rs.uniform(10, 90, (n, 1))
    return np.arange(n + 1, dtype=np.int64) * wp, x.reshape(-1), y.reshape(-1)


def measure(obj, solve, reps, linear_div):
    """solve(mode_is_index, div) -> a result; (ms linear, ms index, hits equal, info of the indexed run)"""
    t = {False: [], True: []}
    last = {}
    for rep in range(reps + 1):
        for mode in (False, True):
            obj.obstacle_index = mode
            res = solve(linear_div if not mode else 1)
            if rep:
                t[mode].append(res.kernel_ms * (linear_div if not mode else 1))
            last[mode] = res
    obj.obstacle_index = None
    n = len(last[False].hit)
    return (statistics.median(t[False]), statistics.median(t[True]), bool(np.array_equal(last[False].hit, last[True].hit[:n])),
            last[True].obstacle_index)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--courses", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", default="16,32,50,64,128,256,512,1000,3000,10000,30000,100000")
    ap.add_argument("--linear-cap", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rrt_amd
    import obsindex_util as OI
    ms = [int(v) for v in args.m.split(",")]
    st, go = pose_pairs(args.pairs, 1)
    crs = courses(args.courses, 2)
    steer = {"dubins": rrt_amd.BatchSteer("dubins"), "rs": rrt_amd.BatchSteer("rs")}
    spline = rrt_amd.BatchSpline()
    rows = []
    for m in ms:
        ob = shrinking_map(7, m)
        div = 8 if m > args.linear_cap else 1
        row = {"m": m, "pairs": args.pairs, "courses": args.courses, "reps": args.reps, "linear_scaled": div > 1,
               "linear_batch_divisor": div}
        for kind, bs in steer.items():
            step = 0.1 if kind == "dubins" else 0.2
            for what, fn in ((kind, bs.plan), (kind + "_plan_free", bs.plan_free)):
                lin, idx, same, info = measure(bs, lambda d, fn=fn: fn(st[:len(st) // d], go[:len(go) // d], 1.0, step_size=step,
                                                                       points=False, obstacle_list=ob, robot_radius=0.1),
                                               args.reps, div)
                row[what] = {"linear_ms": round(lin, 4), "index_ms": round(idx, 4), "equal": same}
            row["build_ms"] = round(info["build_ms"], 4)
            row["grid"] = [info["nx"], info["n_items"], info["n_wide"]]
            if kind == "dubins":
                bs.obstacle_index = True
                res = bs.plan(st[:64], go[:64], 1.0, obstacle_list=ob, robot_radius=0.1)
                bs.obstacle_index = None
                index = OI.build(ob, 0.1)
                pick = np.random.RandomState(3).choice(len(res.x), min(2000, len(res.x)), replace=False)
                got = [OI.point_first_hit(index, ob, 0.1, res.x[i], res.y[i]) for i in pick]
                row["records_per_point"] = round(float(np.mean([r for _, r in got])), 2)
                row["free_fraction"] = round(float(np.mean(res.hit == -1)), 3)
        lin, idx, same, _ = measure(spline, lambda d: spline.run((crs[0][:args.courses // d + 1], crs[1][:8 * (args.courses // d)],
                                                                  crs[2][:8 * (args.courses // d)]), ds=0.1, arrays=False,
                                                                 obstacle_list=ob, robot_radius=0.1), args.reps, div)
        row["spline"] = {"linear_ms": round(lin, 4), "index_ms": round(idx, 4), "equal": same}
        rows.append(row)
        print(json.dumps(row), flush=True)
    cross = {}
    for what in ("dubins", "dubins_plan_free", "rs", "rs_plan_free", "spline"):
        ok = [r[what]["index_ms"] <= r[what]["linear_ms"] for r in rows]
        first = next((i for i in range(len(ok)) if all(ok[i:])), None)
        cross[what] = None if first is None else rows[first]["m"]
    summary = {"crossover": cross, "all_equal": all(r[w]["equal"] for r in rows for w in cross)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": rows, "summary": summary}, f, indent=1)
    for b in steer.values():
        b.close()
    spline.close()


if __name__ == "__main__":
    main()

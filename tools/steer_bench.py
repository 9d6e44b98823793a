"""Throughput of the batched Dubins / Reeds-Shepp curves (BatchSteer): pairs/s for lengths-only and for points.

    python tools/steer_bench.py [--pairs 1048576] [--reps 5] [--cpu-pairs 2000] [--obstacles M] [--kind lqr|bezier] [--all]

Random pairs in the pose box of the known-answer vectors ([-2, 15]^2, any yaw), curvature 1, Reeds-Shepp step 0.2.  The
GPU figure is HIP-event kernel time (stage 1, and stage 1 + fill), the median of --reps solves after one warm-up solve;
transfers and the host prefix sum are reported separately as wall time.  Beside it: the C oracle (oracle.dubins /
oracle.reeds_shepp, which always builds the points) on one core over a subsample of the same pairs.  Prints one JSON
line per kind.  Needs a device: there is no CPU fallback.

--obstacles M (default 0: the output above, unchanged) adds the obstacle check against M seeded circles in the same box
(radius 0.2 .. 0.8): "check_lengths_*" is points=False with the list set (the collision-free cost-matrix path),
"check_points_*" is points=True with it, "plan_wall_ms" of each variant is one whole BatchSteer.plan() call (transfers
and result arrays included), and "free_fraction" the share of pairs whose curve touches nothing.

--kind lqr (default: the two curve kinds, the output above, unchanged) measures BatchSteer("lqr") alone: random point pairs
in the same box, rrt_09's step 0.2, the same variants; the one-core figure beside it is tests/lqr_oracle.edge (pure Python)
on a subsample of the same pairs.

--kind bezier measures BatchSteer("bezier") alone: the same pose pairs, offset 3.0, 100 points per curve.  One JSON line
with a row per variant -- "lengths" (points=False, curvature=False), "lengths_kmax" (points=False), "points" (x, y, yaw
and k per point), and with --obstacles M "check_lengths" and "check_points" -- each with the HIP-event kernel time (weight
table, stage 1, fill; the median of --reps calls after one warm-up) and the wall time of the whole BatchSteer.plan() call
beside it; then tests/bezier_oracle.curve4 (pure Python) on one core over a subsample of the same pairs.

--all measures every candidate curve of a pair (BatchSteer.candidates / plan_free) for the two curve kinds, against
--obstacles M circles (default 12 in this mode): "candidates_lengths" (points=False, no list), "candidates_check" (points=False
with the list: every candidate's points computed and tested, none stored), "candidates_points" (stored and tested),
"plan_free" and "plan_free_points" (the same two plus the selection and the gather), and "plan_check" (plan(points=False)
with the list) for comparison -- HIP-event kernel time, the median of --reps solves after one warm-up, on the binding's
solve calls (no result arrays are copied back).  Beside them the candidates and points per pair, "free_fraction" of plan(),
"free_fraction_plan_free", and "rows_changed": the share of pairs whose row plan_free moved to another candidate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pairs(n, seed):
    rs = np.random.RandomState(seed)
    p = np.empty((n, 6))
    p[:, [0, 1, 3, 4]] = rs.uniform(-2, 15, (n, 4))
    p[:, [2, 5]] = rs.uniform(-np.pi, np.pi, (n, 2))
    return p


def bench_bezier(args):
    import rrt_amd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bezier_oracle
    p = pairs(args.pairs, 11)
    out = {"kind": "bezier", "pairs": args.pairs, "reps": args.reps, "n_points": 100, "offset": 3.0}
    rows = [("lengths", dict(points=False, curvature=False)), ("lengths_kmax", dict(points=False)), ("points", dict())]
    if args.obstacles > 0:
        rs = np.random.RandomState(9)
        circles = np.stack([rs.uniform(-2, 15, args.obstacles), rs.uniform(-2, 15, args.obstacles),
                            rs.uniform(0.2, 0.8, args.obstacles)], axis=1)
        out["obstacles"] = args.obstacles
        rows += [("check_lengths", dict(points=False, obstacle_list=circles)), ("check_points", dict(obstacle_list=circles))]
    with rrt_amd.BatchSteer("bezier") as bs:
        for name, kw in rows:
            ms, wall = [], []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                res = bs.plan(p[:, 0:3], p[:, 3:6], offset=3.0, n_points=100, **kw)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(res.kernel_ms)
                if "obstacle_list" in kw:
                    out["free_fraction"] = float(np.mean(res.free))
                res = None
            med = float(np.median(ms[1:]))
            out[name + "_kernel_ms"] = med
            out[name + "_pairs_per_s"] = args.pairs / (med * 1e-3)
            out[name + "_plan_wall_ms"] = float(np.median(wall[1:]))
    m = min(args.cpu_pairs, args.pairs)
    t0 = time.perf_counter()
    for i in range(m):
        bezier_oracle.curve4(*[float(v) for v in p[i]], 3.0, n_points=100)
    dt = time.perf_counter() - t0
    out["cpu_oracle"] = "tests/bezier_oracle.curve4 (pure Python)"
    out["cpu_oracle_pairs"] = m
    out["cpu_oracle_pairs_per_s_one_core"] = m / dt
    print(json.dumps(out), flush=True)


def bench_all(args):
    import rrt_amd
    m = args.obstacles or 12
    rs = np.random.RandomState(9)
    circles = np.stack([rs.uniform(-2, 15, m), rs.uniform(-2, 15, m), rs.uniform(0.2, 0.8, m)], axis=1)
    for kind in ("dubins", "rs"):
        p = pairs(args.pairs, {"dubins": 7, "rs": 8}[kind])
        step = 0.1 if kind == "dubins" else 0.2
        out = {"kind": kind, "mode": "all", "pairs": args.pairs, "reps": args.reps, "obstacles": m}
        with rrt_amd.BatchSteer(kind) as bs:
            S = bs._steer
            rows = [("candidates_lengths", "all", False, None), ("candidates_check", "all", False, circles),
                    ("candidates_points", "all", True, circles), ("plan_free", "free", False, circles),
                    ("plan_free_points", "free", True, circles), ("plan_check", "plan", False, circles)]
            for name, what, points, obs in rows:
                S.set_obstacles(np.zeros((0, 3)) if obs is None else obs)
                ms, wall = [], []
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    if what == "plan":
                        S.solve(bs.kind, p[:, 0:3], p[:, 3:6], 1.0, step, points=points)
                        ms.append(S.kernel_ms())
                    else:
                        S.solve_all(bs.kind, p[:, 0:3], p[:, 3:6], 1.0, step, points=points)
                        if what == "free":
                            _, _, rank, n_free = S.select_free()
                            ms.append(S.kernel_ms())
                        else:
                            ms.append(S.cand_counts()[3])
                    wall.append((time.perf_counter() - t0) * 1e3)
                med = float(np.median(ms[1:]))
                out[name + "_kernel_ms"] = med
                out[name + "_pairs_per_s"] = args.pairs / (med * 1e-3)
                out[name + "_solve_wall_ms"] = float(np.median(wall[1:]))
                if name == "candidates_points":
                    _, nc, npts, _ = S.cand_counts()
                    out["candidates_per_pair"] = nc / args.pairs
                    out["candidate_points_per_pair"] = npts / args.pairs
                if name == "plan_free":
                    out["rows_changed"] = float(np.mean(rank > 0))
                    out["free_fraction_plan_free"] = float(np.mean(n_free > 0))
                if what == "plan":
                    out["free_fraction"] = float(np.mean(S.hits() == -1))
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=2000)
    ap.add_argument("--obstacles", type=int, default=0)
    ap.add_argument("--kind", choices=("curves", "lqr", "bezier"), default="curves")
    ap.add_argument("--all", action="store_true")
    args = ap.parse_args()
    if args.all:
        return bench_all(args)
    if args.kind == "bezier":
        return bench_bezier(args)
    import oracle
    import rrt_amd
    lqr = args.kind == "lqr"
    for kind in (("lqr",) if lqr else ("dubins", "rs")):
        p = pairs(args.pairs, {"dubins": 7, "rs": 8, "lqr": 10}[kind])
        cols = (slice(0, 2), slice(3, 5)) if lqr else (slice(0, 3), slice(3, 6))   # LQR rows are (x, y): no yaw
        curv = () if lqr else (1.0,)
        out = {"kind": kind, "pairs": args.pairs, "reps": args.reps}
        with rrt_amd.BatchSteer(kind) as bs:
            for points in (False, True):
                ms, wall = [], []
                res = None
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    if lqr:
                        res = bs._steer.solve_lqr(p[:, cols[0]], p[:, cols[1]], 0.2, points=points)
                    else:
                        res = bs._steer.solve(bs.kind, p[:, 0:3], p[:, 3:6], 1.0, 0.1 if kind == "dubins" else 0.2, points=points)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(bs._steer.kernel_ms())
                k = "points" if points else "lengths"
                med = float(np.median(ms[1:]))
                out[k + "_kernel_ms"] = med
                out[k + "_pairs_per_s"] = args.pairs / (med * 1e-3)
                out[k + "_solve_wall_ms"] = float(np.median(wall[1:]))
                if points:
                    out["n_points"] = bs._steer.counts()[1]
                    out["points_per_s"] = out["n_points"] / (med * 1e-3)
            if args.obstacles > 0:
                rs = np.random.RandomState(9)
                circles = np.stack([rs.uniform(-2, 15, args.obstacles), rs.uniform(-2, 15, args.obstacles),
                                    rs.uniform(0.2, 0.8, args.obstacles)], axis=1)
                out["obstacles"] = args.obstacles
                for k, points, obs in (("points", True, None), ("check_lengths", False, circles), ("check_points", True, circles)):
                    ms, wall = [], []
                    for rep in range(args.reps + 1):
                        t0 = time.perf_counter()
                        res = bs.plan(p[:, cols[0]], p[:, cols[1]], *curv, points=points, obstacle_list=obs)
                        wall.append((time.perf_counter() - t0) * 1e3)
                        ms.append(res.kernel_ms)
                    if obs is not None:
                        out[k + "_kernel_ms"] = float(np.median(ms[1:]))
                        out[k + "_pairs_per_s"] = args.pairs / (out[k + "_kernel_ms"] * 1e-3)
                        out["free_fraction"] = float(np.mean(res.free))
                    out[k + "_plan_wall_ms"] = float(np.median(wall[1:]))
                    res = None
        m = min(args.cpu_pairs, args.pairs)
        if lqr:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import lqr_oracle
            t0 = time.perf_counter()
            for i in range(m):
                lqr_oracle.edge(float(p[i, 0]), float(p[i, 1]), float(p[i, 3]), float(p[i, 4]), 0.2)
            dt = time.perf_counter() - t0
            out["cpu_oracle"] = "tests/lqr_oracle.edge (pure Python)"
        else:
            fn = oracle.dubins if kind == "dubins" else oracle.reeds_shepp
            t0 = time.perf_counter()
            for i in range(m):
                a = [float(v) for v in p[i]]
                try:
                    fn(*a, 1.0)
                except (ZeroDivisionError, ValueError):
                    pass
            dt = time.perf_counter() - t0
        out["cpu_oracle_pairs"] = m
        out["cpu_oracle_pairs_per_s_one_core"] = m / dt
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the obstacle map costs and buys under the Reeds-Shepp planner: 4 096 instances x 150 iterations of the plan of
tests/rs_obsmap_util.py (start (0, 0, 0), goal (6, 9, pi/2), rand_area [-2, 20]) on its scenes,

  m = 64       through the tile (rrt_rs_kernel) and through the map (rrt_rs_map_kernel) -- the same kernel body with and
               without the index: what the index costs where it is not needed
  m = 300, 1 000, 5 000, 100 000   through the map (the tile cannot hold them)

HIP-event kernel time of the plan (rrtx_stats.kernel_ms), median of 5 after a warm-up, plans/s and the map's build time; then
"closed_loop_rrt_star" at m = 64, tile against map: the kernel time of track().  No figure is promised and none gates anything.

Usage: python tools/rs_map_bench.py [--instances 4096] [--iters 150] [--repeats 5] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import rs_obsmap_util as R  # noqa: E402

# (circles, path): the scenes of the tests, and one of 10^5 circles (BIG: rmin, rmax, robot_radius) whose radii shrink likewise
SHAPES = [(64, "tile"), (64, "map"), (300, "map"), (1000, "map"), (5000, "map"), (100000, "map")]
BIG = (0.0005, 0.002, 0.002)


def circles_of(m):
    if m == 64:
        rmin, rmax, rr = R.SCENES[65]
        return R.scene(R.MAP_SEED, 65, rmin, rmax)[:64], rr
    rmin, rmax, rr = R.SCENES.get(m, BIG)
    return R.scene(R.MAP_SEED, m, rmin, rmax), rr


def run_plan(m, path, a):
    circles, rr = circles_of(m)
    kw = R.problem(0, obstacles=circles, robot_radius=rr, max_iter=a.iters)
    seeds = list(range(a.instances))
    h = R.make_handle(kw, a.instances)
    try:
        (h.set_obstacle_map if path == "map" else h.set_obstacles)(circles)
        info = h.obstacle_map_info() if path == "map" else None
        ms = []
        for rep in range(a.repeats + 1):          # the first is the warm-up
            h.seed_instances(seeds)
            h.plan()
            st = h.get_stats()
            if rep:
                ms.append(st["kernel_ms"])
        found = int((h.get_results()[2] & 2 != 0).sum())
    finally:
        h.close()
    med = statistics.median(ms)
    return dict(m=m, path=path, kernel_ms_median=med, kernel_ms=ms, plans_per_s=a.instances / (med / 1e3), paths_found=found,
                replanned=st["replanned"], total_nodes=st["total_nodes"],
                map_build_ms=None if info is None else info["build_ms"],
                map_cells=None if info is None else info["nx"] * info["ny"],
                map_items=None if info is None else info["n_items"], map_wide=None if info is None else info["n_wide"])


def run_track(use_map, a):
    import rrt_amd
    circles, rr = circles_of(64)
    bp = rrt_amd.BatchPlanner("closed_loop_rrt_star", seeds=list(range(a.instances)), start=R.START, goal=R.GOAL,
                              obstacle_list=circles, rand_area=R.RAND_AREA, max_iter=a.iters, robot_radius=rr,
                              obstacle_map=use_map)
    tree_ms, track_ms = [], []
    try:
        for rep in range(a.repeats + 1):
            bp.h.seed_instances(bp.seeds)
            bp.plan()
            flags = bp.track()
            ts = bp.h.get_track_stats()
            if rep:
                tree_ms.append(bp.stats()["kernel_ms"])
                track_ms.append(ts["kernel_ms"])
    finally:
        bp.close()
    return dict(m=64, path="map" if use_map else "tile", tree_ms_median=statistics.median(tree_ms),
                track_ms_median=statistics.median(track_ms), track_ms=track_ms, rollout_steps=ts["steps"],
                feasible=int(flags.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rows, tracks = [], []
    for m, path in SHAPES:
        row = run_plan(m, path, a)
        rows.append(row)
        print("plan  m=%-7d %-4s kernel %9.2f ms  %10.1f plans/s  build %s ms  cells %s  records %s  paths %d/%d  replanned %d"
              % (m, path, row["kernel_ms_median"], row["plans_per_s"],
                 "-" if row["map_build_ms"] is None else "%.2f" % row["map_build_ms"], row["map_cells"], row["map_items"],
                 row["paths_found"], a.instances, row["replanned"]), flush=True)
    for use_map in (False, True):
        row = run_track(use_map, a)
        tracks.append(row)
        print("track m=64      %-4s tree %9.2f ms  track %9.2f ms  %d roll-out steps  feasible %d/%d"
              % (row["path"], row["tree_ms_median"], row["track_ms_median"], row["rollout_steps"], row["feasible"], a.instances),
              flush=True)
    out = dict(instances=a.instances, iters=a.iters, repeats=a.repeats, plan=rows, track=tracks)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

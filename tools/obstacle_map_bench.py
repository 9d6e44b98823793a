#!/usr/bin/env python3
"""What the obstacle map (rrtx_set_obstacle_map) costs and what it buys: 4 096 instances x 2 000 iterations of the C2
configuration on synth_map-style maps,

  m = 256      through the tile (RRTX_KERNEL=v1: the general kernel) and through the map -- the same kernel body with and
               without the index: what the index costs where it is not needed
  m = 1 000, 10 000, 100 000   through the map (the tile cannot hold them)

HIP-event kernel time of the plan (rrtx_stats.kernel_ms), median of 5 after a warm-up; plans/s, the map's build time, the
records gathered per iteration, and beside them the CPU oracle on one core over a few of the same plans.  No figure is
promised and none gates anything.

Usage: python tools/obstacle_map_bench.py [--instances 4096] [--iters 2000] [--repeats 5] [--oracle-plans 2] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import util  # noqa: E402

# radii shrink with the count so that every map leaves the same share of the square free (about 6 % covered)
SHAPES = [(256, 0.5, 1.2, "tile"), (256, 0.5, 1.2, "map"), (1000, 0.25, 0.6, "map"), (10000, 0.08, 0.19, "map"),
          (100000, 0.025, 0.06, "map")]


def gathered_records(st, n_instances):
    """Obstacle bytes of rrtx_stats.algorithmic_bytes: what is left when the node scans (16 B a node), the candidate
    gathers (48 B each) and the appended nodes (28 B each) are taken off -- 24 B per tile entry and iteration on the tile,
    32 B per gathered record on the map."""
    return st["algorithmic_bytes"] - 16 * st["scan_nodes"] - 48 * st["near_unique"] - 28 * (st["total_nodes"] - n_instances)


def run_shape(m, rmin, rmax, path, a):
    import rrt_amd
    A = rrt_amd._abi
    kw = util.c2_kwargs(a.iters)
    kw["obstacles"] = util.synth_map(13, m, rmin, rmax)
    if path == "tile":
        os.environ["RRTX_KERNEL"] = "v1"
    else:
        os.environ.pop("RRTX_KERNEL", None)
    seeds = list(range(1, a.instances + 1))
    h = A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                 kw["goal_sample_rate"], kw["max_iter"], connect_circle_dist=kw["connect_circle_dist"],
                 search_until_max_iter=True, n_instances=a.instances)
    try:
        (h.set_obstacle_map if path == "map" else h.set_obstacles)(kw["obstacles"])
        info = h.obstacle_map_info() if path == "map" else None
        ms = []
        for rep in range(a.repeats + 1):          # the first is the warm-up
            h.seed_instances(seeds)
            h.plan()
            st = h.get_stats()
            if rep:
                ms.append(st["kernel_ms"])
        med = statistics.median(ms)
        found = int((h.get_results()[2] & 2 != 0).sum())
    finally:
        h.close()
        os.environ.pop("RRTX_KERNEL", None)
    obstacle_bytes = gathered_records(st, a.instances)
    row = dict(m=m, path=path, kernel_ms_median=med, kernel_ms=ms, plans_per_s=a.instances / (med / 1e3), paths_found=found,
               obstacle_units_per_iteration=obstacle_bytes / (24.0 if path == "tile" else 32.0) / st["iterations"],
               map_build_ms=None if info is None else info["build_ms"],
               map_cells=None if info is None else info["nx"] * info["ny"],
               map_items=None if info is None else info["n_items"], map_wide=None if info is None else info["n_wide"])
    t0 = time.time()
    for s in seeds[:a.oracle_plans]:
        util.run_oracle(kw, s, exact_pow=True)
    row["oracle_plans_per_s_one_core"] = a.oracle_plans / (time.time() - t0) if a.oracle_plans else None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle-plans", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rows = []
    for m, rmin, rmax, path in SHAPES:
        row = run_shape(m, rmin, rmax, path, a)
        rows.append(row)
        print("m=%-7d %-4s kernel %9.1f ms  %9.1f plans/s  build %s ms  %8.1f records/iteration  oracle %.2f plans/s (one core)  "
              "paths %d/%d" % (m, path, row["kernel_ms_median"], row["plans_per_s"],
                               "-" if row["map_build_ms"] is None else "%.2f" % row["map_build_ms"],
                               row["obstacle_units_per_iteration"], row["oracle_plans_per_s_one_core"] or 0.0,
                               row["paths_found"], a.instances), flush=True)
    out = dict(instances=a.instances, iters=a.iters, repeats=a.repeats, rows=rows)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

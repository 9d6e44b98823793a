"""Closed-loop RRT* (rrt_10) throughput on one GPU: 4 096 driver-cell instances (rrt_10:1610-1661, max_iter=150), HIP-event
time of the tree launch and of the tracking launches separately, median of 5 after a warm-up; plans/s and roll-out
steps/s of the tracking kernel.  The reference does not exist on the GPU machine: its per-plan time on the same seeds is
measured on the build host by `python tools/gen_golden_closed_loop.py time 0 1 2 3` (DESIGN.md 5.10 records it).

    python tools/closed_loop_bench.py [--instances 4096] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rrt_amd  # noqa: E402

OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=150)
    a = ap.parse_args()
    bp = rrt_amd.BatchPlanner("closed_loop_rrt_star", seeds=list(range(a.instances)), start=[0.0, 0.0, 0.0],
                              goal=[6.0, 9.0, float(np.deg2rad(90.0))], obstacle_list=OBS, rand_area=[-2, 20],
                              max_iter=a.max_iter)
    tree_ms, track_ms, steps = [], [], 0
    try:
        for rep in range(a.reps + 1):
            for h, (lo, hi) in zip(bp.handles, bp.shards):
                h.seed_instances(bp.seeds[lo:hi])
            bp.plan()
            flags = bp.track()
            per = [h.get_track_stats() for h in bp.handles]     # shards run side by side: the slowest one's time
            if rep:      # the first pass is the warm-up
                tree_ms.append(bp.stats()["kernel_ms"])
                track_ms.append(max(p["kernel_ms"] for p in per))
            steps = sum(p["steps"] for p in per)
    finally:
        bp.close()
    t1, t2 = statistics.median(tree_ms), statistics.median(track_ms)
    print(json.dumps(dict(instances=a.instances, max_iter=a.max_iter, tree_ms=t1, track_ms=t2, feasible=int(flags.sum()),
                          plans_per_s=a.instances / ((t1 + t2) * 1e-3), rollout_steps=steps,
                          rollout_steps_per_s=steps / (t2 * 1e-3))))


if __name__ == "__main__":
    main()

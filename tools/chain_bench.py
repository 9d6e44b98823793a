"""Plan, then track: the hand-over between BatchSteer and BatchTrack three ways, in one process on one device.

    python tools/chain_bench.py [--starts 4096] [--goals 64] [--reps 5] [--T 20.0]

starts x goals Reeds-Shepp pairs (2^18 by default) are planned with plan_free(product=True) against 12 circles, then every
chosen curve is tracked from its start pose:
  host    points=True, run(result, arrays=False): the points come to the host and go up again (the behaviour before
          points="device" existed);
  device  points="device", run(result, arrays=False): the tracker reads the points where the planner left them;
  best    points="device", run(result, select="free", group=True, arrays="best"): only the free curves are tracked, the best
          goal of every start is picked on the device and only the winners' arrays come back.
Per way: the wall time of the whole chain and the summed HIP-event kernel time (planner + tracker), each the median of
--reps runs after one warm-up, and the bytes the courses and results move across PCIe, computed from the counts.  Prints one
JSON line.  Nothing here gates anything."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=4096)
    ap.add_argument("--goals", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--T", type=float, default=20.0, help="the tracker's time limit per roll-out (the model global T)")
    a = ap.parse_args()
    import rrt_amd
    rs = np.random.RandomState(1)
    ns, ng = a.starts, a.goals
    starts = np.stack([rs.uniform(-2, 2, ns), rs.uniform(-2, 2, ns), rs.uniform(-np.pi, np.pi, ns)], axis=1)
    goals = np.stack([rs.uniform(4, 14, ng), rs.uniform(-8, 8, ng), rs.uniform(-np.pi, np.pi, ng)], axis=1)
    circles = [(rs.uniform(2, 12), rs.uniform(-7, 7), rs.uniform(0.4, 1.2)) for _ in range(12)]
    state = np.repeat(np.concatenate([starts, np.zeros((ns, 1))], axis=1), ng, axis=0)
    plan_kw = dict(step_size=0.2, product=True, obstacle_list=circles, robot_radius=0.3)
    track_kw = dict(obstacle_list=circles, robot_radius=0.3, start_state=state)
    ways = {"host": (True, dict(arrays=False)), "device": ("device", dict(arrays=False)),
            "best": ("device", dict(select="free", group=True, arrays="best"))}
    out = {"pairs": ns * ng, "starts": ns, "goals": ng, "reps": a.reps, "T": a.T}
    with rrt_amd.BatchSteer("rs") as bs, rrt_amd.BatchTrack(T=a.T) as bt:
        for name, (points, kw) in ways.items():
            wall, kern = [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                plan = bs.plan_free(starts, goals, 1.0, points=points, **plan_kw)
                res = bt.run(plan, **track_kw, **kw)
                dt = time.perf_counter() - t0
                if rep:      # the first run warms up
                    wall.append(1e3 * dt)
                    kern.append(plan.kernel_ms + res.kernel_ms)
            n, pts = len(res), int(plan.offsets[-1])
            moved = {"points_d2h": 24 * pts if points is True else 0, "points_h2d": (24 * pts + 8 * (n + 1)) if points is True else 0,
                     "records_d2h": 24 * n, "arrays_d2h": 0 if res.x is None else 56 * res.steps,
                     "winners_goals_d2h": 0 if res.winner is None else 28 * len(res.winner)}
            out[name] = {"wall_ms": statistics.median(wall), "kernel_ms": statistics.median(kern), "points": pts,
                         "tracked": int(np.sum(res.status != rrt_amd.track.OOD_SKIPPED)), "steps": res.steps,
                         "pcie_bytes": moved, "pcie_bytes_total": int(sum(moved.values()))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Throughput of the stand-alone tracker (BatchTrack): roll-out steps/s for records only and with arrays.

    python tools/track_bench.py [--courses 65536] [--reps 5]

Reeds-Shepp courses (curvature 1, step 0.2) from the origin to seeded random poses in [-6, 8]^2 with any yaw, made with
BatchSteer; pairs without a path are dropped.  The figure is HIP-event kernel time (the records launch, and the records +
arrays launches), the median of --reps runs after one warm-up run; transfers and the host prefix sum are reported separately
as wall time.  Steps are the roll-out steps of one pass over the courses (the sum of len(t)); the arrays figure divides the
same steps by the time of both launches.  Prints one JSON line.  Needs a device: there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def courses(n, seed):
    import rrt_amd
    rs = np.random.RandomState(seed)
    goals = np.stack([rs.uniform(-6, 8, n), rs.uniform(-6, 8, n), rs.uniform(-np.pi, np.pi, n)], axis=1)
    with rrt_amd.BatchSteer("rs") as bs:
        sr = bs.plan(np.zeros((n, 3)), goals, 1.0)
    keep = np.nonzero(np.diff(sr.offsets) >= 3)[0]
    idx = np.concatenate([np.arange(sr.offsets[i], sr.offsets[i + 1]) for i in keep])
    off = np.concatenate([[0], np.cumsum(np.diff(sr.offsets)[keep])])
    return off, sr.x[idx], sr.y[idx], sr.yaw[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--courses", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import rrt_amd
    csr = courses(args.courses, 9)
    out = {"courses": len(csr[0]) - 1, "points": int(csr[0][-1]), "reps": args.reps}
    with rrt_amd.BatchTrack() as bt:
        for arrays in (False, True):
            ms, wall = [], []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                res = bt.run(csr, arrays=arrays)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(res.kernel_ms)
            k = "arrays" if arrays else "records"
            med = float(np.median(ms[1:]))
            out["steps"] = res.steps
            out["reached"] = int(np.sum(res.find_goal))
            out[k + "_kernel_ms"] = med
            out[k + "_steps_per_s"] = res.steps / (med * 1e-3)
            out[k + "_run_wall_ms"] = float(np.median(wall[1:]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

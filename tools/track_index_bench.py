"""What the tracker's obstacle index costs (BatchTrack(obstacle_index=True)): roll-out steps/s of the records
launch with the lane-per-obstacle check (OFF) and with the index (ON), on the course workload of tools/track_bench.py.

    python tools/track_index_bench.py [--courses 16384] [--reps 5]

Maps: m circles spread over the box of the courses, [-8, 10]^2, with radii that shrink with the count (0.4 / sqrt(m) ..
1.2 / sqrt(m)), robot radius 0.1.  OFF and ON alternate in one process at m = 0, 16 and 64 -- where both apply -- and ON runs
alone at m = 65, 1 000, 10^4 and 10^5.  Before anything is timed the two `fail` columns are compared.  Per map: HIP-event
kernel ms of the records launch (the median of --reps runs after one warm-up run), roll-out steps/s, the build's ms, and the
records read per trajectory point (the walk of rppo::point_first_hit restated over the index read back, on a sample of the
stored points of 64 courses).  Prints one JSON line per map.  Needs a device: there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from track_bench import courses  # noqa: E402

BOTH, ON_ONLY = (0, 16, 64), (65, 1000, 10 ** 4, 10 ** 5)
RR = 0.1


def circles(m, seed=5):
    rs = np.random.RandomState(seed + m)
    return np.column_stack([rs.uniform(-8, 10, m), rs.uniform(-8, 10, m), rs.uniform(0.4, 1.2, m) / np.sqrt(max(m, 1))])


def cell_of(v, origin, cell, n):
    q = np.floor((v - origin) / cell)
    return int(min(max(q, 0.0), n - 1)) if q == q else 0


def reads_per_point(index, x, y):
    """Records the walk of point_first_hit reads, averaged over the points"""
    info, start, items, wide = index
    total = 0
    for px, py in zip(x, y):
        k = cell_of(py, info["y0"], info["cell"], info["ny"]) * info["nx"] + cell_of(px, info["x0"], info["cell"], info["nx"])
        best = -1
        for it in items[start[k]:start[k + 1]]:
            total += 1
            dx, dy = it["ox"] - px, it["oy"] - py
            if dx * dx + dy * dy <= it["thr"]:
                best = int(it["index"])
                break
        for it in wide:
            if best >= 0 and it["index"] > best:
                break
            total += 1
            dx, dy = it["ox"] - px, it["oy"] - py
            if dx * dx + dy * dy <= it["thr"]:
                break
    return total / max(len(x), 1)


def timed(bt, csr, ob, reps):
    ms = []
    for _ in range(reps + 1):
        res = bt.run(csr, obstacle_list=ob, robot_radius=RR, arrays=False)
        ms.append(res.kernel_ms)
    return res, float(np.median(ms[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--courses", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import rrt_amd
    csr = courses(args.courses, 9)
    sample = (csr[0][:65], csr[1][:csr[0][64]], csr[2][:csr[0][64]], csr[3][:csr[0][64]])
    with rrt_amd.BatchTrack() as off, rrt_amd.BatchTrack(obstacle_index=True) as on:
        for m in BOTH + ON_ONLY:
            ob = circles(m)
            out = {"m": m, "courses": len(csr[0]) - 1, "reps": args.reps}
            first = on.run(csr, obstacle_list=ob, robot_radius=RR, arrays=False)
            if m in BOTH:      # the two fail columns before anything is timed
                ref = off.run(csr, obstacle_list=ob, robot_radius=RR, arrays=False)
                out["fail_equal"] = bool(np.array_equal(first.fail, ref.fail) and np.array_equal(first.length, ref.length))
                if not out["fail_equal"]:
                    print(json.dumps(out), flush=True)
                    return 1
            order = ("off", "on", "off", "on") if m in BOTH else ("on",)
            ms = {"off": [], "on": []}
            for which in order:      # alternating in one process
                res, med = timed(off if which == "off" else on, csr, ob, args.reps)
                ms[which].append(med)
            out["steps"] = res.steps
            out["blocked"] = int(np.sum((first.fail & 8) != 0))
            for which in ("off", "on"):
                if ms[which]:
                    out[which + "_kernel_ms"] = ms[which]
                    out[which + "_steps_per_s"] = res.steps / (min(ms[which]) * 1e-3)
            info = first.obstacle_index
            if info is not None and info["used"]:
                out["build_ms"] = info["build_ms"]
                out["cells"] = info["nx"]
                pts = on.run(sample, obstacle_list=ob, robot_radius=RR)
                step = max(len(pts.x) // 2000, 1)
                out["records_per_point"] = reads_per_point(on._tracker.obstacle_index(), pts.x[::step], pts.y[::step])
            print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""rrt_10's closed-loop stage for many goals per planned tree: BatchPlanner.track_goals on one device, beside the best route
without it and the oracle on one core.

    python tools/goal_track_bench.py [--instances 4096] [--max-iter 150] [--reps 5] [--sample 64]

--instances driver-cell trees (rrt_10:1610-1661) are planned once.  The goals are the 4 x 4 x 4 grid x in {2, 6, 10, 14}, y in
{0, 4, 8, 12}, yaw in {-1.57, 0, 0.8, 1.57}, shared by all instances, asked with xy_th = 3.0 and yaw_th = 0.8.
  records   track_goals(goals, arrays=False): HIP-event times of the list launches, of roll + pick, and the wall time of one
            call (median of --reps after a warm-up); candidates, roll-out steps of the roll launch and its steps/s
  arrays    track_goals(goals): the same with the store launch and the winners' arrays fetched
  route     without track_goals, for --sample instances: fetch each tree, build every candidate course of every goal in
            Python, push them through BatchTrack.run and pick per goal on the host -- wall time, to be scaled by
            instances / sample.  (It reads the polylines' yaw through polyline_yaw(), which arrived with track_goals.)
  oracle    tests/goal_track_oracle.py (candidates, courses and pick in Python, roll-outs through the compiled host core on
            ONE thread) over --sample queries: ms per query.  The sampled answers and the route's are compared with the device's
            before anything is reported.
Prints one JSON line.  Nothing here gates anything.  tools/closed_loop_bench.py in the same session gives track_roll_kernel's
steps/s to read the roll launch's against."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
TH = dict(xy_th=3.0, yaw_th=0.8)


def timed_calls(fn, reps):
    kern, wall = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        if rep:
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(res.kernel_ms)
    return [statistics.median(k[c] for k in kern) for c in range(3)], statistics.median(wall), res


def device_tree(bp, i):
    x, y, _, parent = bp.tree(i)
    plen, px, py = bp.polylines(i)
    return dict(x=x, y=y, yaw=bp.yaw(i), parent=parent, plen=plen, px=px, py=py, pyaw=bp.polyline_yaw(i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    import goal_track_oracle as gt
    import rrt_amd
    A = rrt_amd._abi
    start = [0.0, 0.0, 0.0]
    goals = np.array([[x, y, w] for x in (2.0, 6.0, 10.0, 14.0) for y in (0.0, 4.0, 8.0, 12.0) for w in (-1.57, 0.0, 0.8, 1.57)])
    n, g = a.instances, len(goals)
    bp = rrt_amd.BatchPlanner("closed_loop_rrt_star", seeds=list(range(n)), start=start, goal=[6.0, 9.0, float(np.deg2rad(90.0))],
                              obstacle_list=OBS, rand_area=[-2, 20], max_iter=a.max_iter)
    try:
        t0 = time.perf_counter()
        bp.plan()
        plan_ms = 1e3 * (time.perf_counter() - t0)
        rk, rw, rec = timed_calls(lambda: bp.track_goals(goals, arrays=False, **TH), a.reps)
        ak, aw, full = timed_calls(lambda: bp.track_goals(goals, **TH), a.reps)
        roll_steps = int(rec.cand_len.sum())
        out = {"instances": n, "max_iter": a.max_iter, "goals": g, "queries": n * g, "reps": a.reps, "plan_wall_ms": plan_ms,
               "candidates": int(rec.cand_offsets[-1]), "flagged": int(rec.flag.sum()), "refused": int((rec.status != 0).sum()),
               "roll_steps": roll_steps, "store_steps": int(full.len[full.flag].sum()),
               "records_list_ms": rk[0], "records_roll_pick_ms": rk[1], "records_wall_ms": rw,
               "roll_steps_per_s": roll_steps / (rk[1] * 1e-3),
               "arrays_list_ms": ak[0], "arrays_roll_pick_ms": ak[1], "arrays_store_ms": ak[2], "arrays_wall_ms": aw}
        # ---- the route without track_goals, on a sample of instances
        P = dict(A.TRACK_DEFAULTS, **TH)
        sample = list(range(0, n, max(1, n // a.sample)))[:a.sample]
        bt = rrt_amd.BatchTrack()
        try:
            t0 = time.perf_counter()
            cx, cy, cw, off, spans = [], [], [], [0], []
            for i in sample:
                tree = device_tree(bp, i)
                po = np.concatenate([[0], np.cumsum(tree["plen"])])
                for j in range(g):
                    cand = gt.candidates(tree, goals[j], TH["xy_th"], TH["yaw_th"])
                    spans.append((i, j, cand, len(off) - 1))
                    for c in cand:
                        x, y, w = gt.course(tree, c, start, goals[j], po)
                        cx += x
                        cy += y
                        cw += w
                        off.append(len(cx))
            res = bt.run((np.array(off, dtype=np.int64), np.array(cx), np.array(cy), np.array(cw)), obstacle_list=OBS, robot_radius=0.0,
                         yaw_th=TH["yaw_th"], arrays=False)
            picks = []
            for i, j, cand, at in spans:
                rows = [(res.find_goal[at + k], res.length[at + k], res.fail[at + k], res.status[at + k], res.t_last[at + k])
                        for k in range(len(cand))]
                picks.append(gt.pick(cand, rows))
            out["route_sample_instances"] = len(sample)
            out["route_sample_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            out["route_scaled_wall_ms"] = out["route_sample_wall_ms"] * n / len(sample)
        finally:
            bt.close()
        for (i, j, cand, _), w in zip(spans, picks):
            assert (rec.flag[i, j], rec.winner[i, j], rec.node[i, j], rec.status[i, j]) == (w["flag"], w["winner"], w["node"], w["status"]), (i, j)
        # ---- the oracle on one core
        os.environ["GOAL_TRACK_THREADS"] = "1"
        with tempfile.TemporaryDirectory() as d:
            exe = gt.build(d)
            rng = np.random.default_rng(1)
            pairs = [(int(rng.integers(n)), int(rng.integers(g))) for _ in range(a.sample)]
            trees = [device_tree(bp, i) for i, _ in pairs]           # the trees come off the device before the clock starts
            t0 = time.perf_counter()
            want = gt.answer(exe, d, [(t, start, OBS, 0.0, goals[j]) for t, (_, j) in zip(trees, pairs)], P)
            out["oracle_ms_per_query"] = 1e3 * (time.perf_counter() - t0) / max(1, len(pairs))
            out["oracle_sample"] = len(pairs)
        for (i, j), w in zip(pairs, want):
            assert (full.flag[i, j], full.winner[i, j], full.len[i, j]) == (w["flag"], w["winner"], w["len"]), (i, j)
            tr = full.trajectory(i, j)
            assert (tr is None) == (w["arr"] is None) and (tr is None or np.array_equal(tr[0], w["arr"][0]))
    finally:
        bp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Golden generator of closed-loop RRT* (rrt_10): runs the reference class itself (loaded through oracle/ref_loader.py,
patched at run time: the rrt_10 file is added to ref_loader.FILES, and KEEP_ASSIGN is replaced by {"show_animation"}
for this load, because the shared set keeps the name `v` and rrt_10:1762 assigns `v = [state.v]` at module level).
Writes tests/golden/rrt10_*.npz and tests/golden/track_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_closed_loop.py               # every configuration below, then the KAT
    python tools/gen_golden_closed_loop.py drv_s0 kat    # only these
    python tools/gen_golden_closed_loop.py time 0 1 2    # no files: the reference's seconds per driver-cell plan, these seeds

Per plan: inputs, the tree (x, y, yaw, cost, parent, polylines), the RNG state after the call, the candidate indices
of get_goal_indexes, per candidate what check_tracking_path_is_feasible returned (find_goal, len(t), t[-1]) and which
of its four tests failed (read from the messages it prints, by wrapping the method), and the returned 8-tuple.
A configuration meant to show a branch is only written when the reference shows it (WANT below).

Where this departs from a plain reading of the plan for these goldens:
  * "no candidate exists": max_iter=1 already yields a candidate with most seeds (try_goal_path reaches the goal from the
    first node), so the case is max_iter=2 with seed 9, whose first two samples collide.
  * "a goal yaw that makes the final-angle test fail": goal yaw 180 deg / -179 deg (gyaw_*): the tracked yaw is wrapped into
    [-pi, pi) and ends near the other sign, so candidates that reach the goal are refused for the angle alone (fail = 2);
    gyaw_s5 and gyaw_s16 return (False, None, ...) WITH candidates.  yaw_s6 shows the same test through a small yaw_th.
  * track_kat.npz holds synthetic courses only.  The courses of the plans are not stored a second time: each plan golden holds
    its tree and polylines, from which tests/track_util.course() rebuilds every candidate's course, and
    tests/test_track_host.py runs all of them through the host core against the per-candidate records.
"""
import contextlib
import io
import json
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["rrt_10"] = "10_path_planning_01_rrt_10_closed_loop_rrt_star.py"
GOLD = os.path.join(ROOT, "tests", "golden")

# rrt_10:1592-1607
MODEL = dict(dt=0.05, L=0.9, steer_max=float(np.deg2rad(40.0)), accel_max=5.0, Kp=2.0, Lf=0.5, T=100.0, goal_dis=0.5,
             stop_speed=0.5)
DRIVER_OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
# the driver cell, rrt_10:1610-1661
DRIVER = dict(start=[0.0, 0.0, float(np.deg2rad(0.0))], goal=[6.0, 9.0, float(np.deg2rad(90.0))],
              obstacle_list=DRIVER_OBS, rand_area=[-2, 20], max_iter=150, connect_circle_dist=50.0, robot_radius=0.0,
              target_speed=10.0 / 3.6, yaw_th=float(np.deg2rad(3.0)), xy_th=0.5, invalid_travel_ratio=5.0)

F_REACH, F_ANGLE, F_LONG, F_COLL = 1, 2, 4, 8
MSG = (("cannot reach goal", F_REACH), ("final angle is bad", F_ANGLE), ("path is too long", F_LONG),
       ("This path is collision", F_COLL))


def load():
    keep = ref_loader.KEEP_ASSIGN
    ref_loader.KEEP_ASSIGN = {"show_animation"}
    try:
        mod = ref_loader.load("rrt_10")
    finally:
        ref_loader.KEEP_ASSIGN = keep
    for k, v in MODEL.items():
        setattr(mod, k, v)
    mod.animation = False
    return mod


def wrap_feasible(obj, records):
    orig = obj.check_tracking_path_is_feasible

    def wrapped(path):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = orig(path)
        text = buf.getvalue()
        fail = 0
        for msg, bit in MSG:
            if msg in text:
                fail |= bit
        find_goal, x, y, yaw, v, t, a, d = out
        records.append(dict(path=path, find=bool(find_goal), n=len(t), tlast=float(t[-1]), fail=fail,
                            last=[float(x[-1]), float(y[-1]), float(yaw[-1]), float(v[-1]), float(a[-1]), float(d[-1])],
                            sums=[float(sum(x)), float(sum(y)), float(sum(yaw)), float(sum(v)), float(sum(a)),
                                  float(sum(d))]))
        return out
    obj.check_tracking_path_is_feasible = wrapped


def run_plan(mod, kw, seed):
    random.seed(seed)
    obj = mod.ClosedLoopRRTStar(**kw)
    records, cands = [], []
    wrap_feasible(obj, records)
    orig_idx = obj.get_goal_indexes

    def idx():
        r = orig_idx()
        cands.extend(int(i) for i in r)
        return r
    obj.get_goal_indexes = idx
    with contextlib.redirect_stdout(io.StringIO()):
        flag, x, y, yaw, v, t, a, d = obj.planning(animation=False)
    st = random.getstate()
    nodes = obj.node_list
    index = {id(nd): i for i, nd in enumerate(nodes)}
    out = dict(seed=seed, kwargs=json.dumps(kw), model=json.dumps(MODEL),
               x=np.array([float(n.x) for n in nodes]), y=np.array([float(n.y) for n in nodes]),
               yaw=np.array([float(n.yaw) for n in nodes]), cost=np.array([float(n.cost) for n in nodes]),
               parent=np.array([index[id(n.parent)] if n.parent is not None else -1 for n in nodes], dtype=np.int32),
               plen=np.array([len(n.path_x) for n in nodes], dtype=np.int32),
               px=np.array([float(q) for n in nodes for q in n.path_x]),
               py=np.array([float(q) for n in nodes for q in n.path_y]),
               pyaw=np.array([float(q) for n in nodes for q in n.path_yaw]),
               mt_after=np.array(st[1][:624], dtype=np.uint32), mt_pos_after=st[1][624],
               cand=np.array(cands, dtype=np.int32),
               cand_find=np.array([r["find"] for r in records], dtype=np.int32),
               cand_len=np.array([r["n"] for r in records], dtype=np.int32),
               cand_tlast=np.array([r["tlast"] for r in records], dtype=np.float64),
               cand_fail=np.array([r["fail"] for r in records], dtype=np.int32),
               cand_last=np.array([r["last"] for r in records], dtype=np.float64).reshape(-1, 6),
               cand_sums=np.array([r["sums"] for r in records], dtype=np.float64).reshape(-1, 6),
               flag=int(bool(flag)))
    for name, arr in (("out_x", x), ("out_y", y), ("out_yaw", yaw), ("out_v", v), ("out_t", t), ("out_a", a),
                      ("out_d", d)):
        out[name] = np.array([] if arr is None else [float(q) for q in arr], dtype=np.float64)
    return out


def kat(mod, n=240):
    """(course -> outcome) vectors of check_tracking_path_is_feasible on Reeds-Shepp courses from the origin to random
    poses (one or two chained segments), against random obstacle sets / thresholds.  The courses of the planned trees
    are covered by the plan goldens themselves (tree + per-candidate records)."""
    rs = np.random.RandomState(10)
    rows, obs_rows, nob, cxs, cys, cws, ncs, outs, lasts, sums = [], [], [], [], [], [], [], [], [], []
    i = 0
    while i < n:
        legs = 1 + (i % 2)
        pose = [0.0, 0.0, 0.0] if i % 5 else [float(rs.uniform(-1, 1)), float(rs.uniform(-1, 1)), float(rs.uniform(-1, 1))]
        px, py, pw = [], [], []
        ok = True
        for _ in range(legs):
            to = [pose[0] + float(rs.uniform(-6, 8)), pose[1] + float(rs.uniform(-6, 8)), float(rs.uniform(-math.pi, math.pi))]
            qx, qy, qw, _, _ = mod.reeds_shepp_path_planning(pose[0], pose[1], pose[2], to[0], to[1], to[2], 1.0, 0.2)
            if not qx:
                ok = False
                break
            px.append(list(qx))
            py.append(list(qy))
            pw.append(list(qw))
            pose = [qx[-1], qy[-1], qw[-1]]
        if not ok:
            continue
        end = [pose[0], pose[1], pose[2] + (0.0 if i % 7 else 0.9)]
        path = [end]
        for qx, qy, qw in zip(reversed(px), reversed(py), reversed(pw)):
            for a, b, c in zip(reversed(qx), reversed(qy), reversed(qw)):
                path.append([a, b, c])
        path.append([px[0][0], py[0][0], pw[0][0]])
        m = int(rs.randint(0, 5))
        obs = [(float(rs.uniform(-4, 8)), float(rs.uniform(-4, 8)), float(rs.uniform(0.2, 1.2))) for _ in range(m)]
        rr = float([0.0, 0.0, 0.3, 0.5][i % 4])
        ts = float([10.0 / 3.6, 5.0 / 3.6, 20.0 / 3.6][i % 3])
        yth = float(np.deg2rad([3.0, 1.0, 6.0][(i // 3) % 3]))
        ratio = float([5.0, 1.0, 1.3, 2.0][(i // 2) % 4])
        obj = mod.ClosedLoopRRTStar([0.0, 0.0, 0.0], end, obs, [-2, 20], robot_radius=rr, target_speed=ts, yaw_th=yth,
                                    invalid_travel_ratio=ratio)
        recs = []
        wrap_feasible(obj, recs)
        obj.check_tracking_path_is_feasible(path)
        r = recs[0]
        rows.append([rr, ts, yth, ratio])
        nob.append(m)
        obs_rows += [list(o) for o in obs]
        ncs.append(len(path))
        cxs += [float(p[0]) for p in path]
        cys += [float(p[1]) for p in path]
        cws += [float(p[2]) for p in path]
        outs.append([int(r["find"]), r["n"], r["fail"]])
        lasts.append([r["tlast"]] + r["last"])
        sums.append(r["sums"])
        i += 1
        if i % 20 == 0:
            print("kat", i, flush=True)
    np.savez_compressed(os.path.join(GOLD, "track_kat.npz"), model=json.dumps(MODEL), rows=np.array(rows),
                        nobs=np.array(nob, dtype=np.int32), obs=np.array(obs_rows, dtype=np.float64).reshape(-1, 3),
                        npath=np.array(ncs, dtype=np.int32), path_x=np.array(cxs), path_y=np.array(cys),
                        path_yaw=np.array(cws), out=np.array(outs, dtype=np.int32), last=np.array(lasts),
                        sums=np.array(sums))
    o = np.array(outs)
    print("kat: %d vectors, feasible %d, fail masks %s" % (len(o), int(o[:, 0].sum()), sorted(set(o[:, 2].tolist()))))


MAP_B = [(5, 5, 1), (4, 6, 1), (4, 8, 1), (4, 10, 1), (6, 5, 1), (7, 5, 1), (8, 6, 1), (8, 8, 1), (8, 10, 1)]

# name, overrides of the driver cell, seed, what the reference has to show for the file to be kept
CONFIGS = [("drv_s%d" % s, {}, s, "flag") for s in range(8)] + [
    ("none_s9", dict(max_iter=2), 9, "none"),
    ("coll_s2", dict(robot_radius=0.3, obstacle_list=DRIVER_OBS + [(1.5, 0.2, 0.25)], max_iter=100), 2, F_COLL),
    ("coll_s3", dict(robot_radius=0.2, obstacle_list=DRIVER_OBS + [(0.0, 0.0, 0.1)], start=[0.0, -1.5, 0.0],
                     max_iter=100), 3, F_COLL),
    ("long_s4", dict(invalid_travel_ratio=1.0, max_iter=100), 4, F_LONG),
    ("gyaw_s5", dict(goal=[6.0, 9.0, float(np.deg2rad(180.0))]), 5, "wrap"),
    ("gyaw_s15", dict(goal=[6.0, 9.0, float(np.deg2rad(180.0))]), 15, "wrap"),
    ("gyaw_s16", dict(goal=[6.0, 9.0, float(np.deg2rad(-179.0))]), 16, "wrap"),
    ("yaw_s6", dict(yaw_th=float(np.deg2rad(0.3)), max_iter=100), 6, F_ANGLE),
    ("start_s7", dict(start=[1.0, -1.0, float(np.deg2rad(20.0))], max_iter=100), 7, "any"),
    ("map_a_s11", dict(max_iter=100), 11, "any"),
    ("map_b_s12", dict(obstacle_list=MAP_B, max_iter=100), 12, "any"),
]


def time_reference(mod, seeds):
    import time
    for s in seeds:
        t0 = time.perf_counter()
        res = run_plan(mod, dict(DRIVER), s)
        print("seed %d: %.1f s per plan (%d nodes, %d candidates)" % (s, time.perf_counter() - t0, len(res["x"]),
                                                                    len(res["cand"])), flush=True)


def main():
    os.makedirs(GOLD, exist_ok=True)
    mod = load()
    only = sys.argv[1:]
    if only and only[0] == "time":
        return time_reference(mod, [int(v) for v in only[1:]] or list(range(8)))
    for name, over, seed, want in CONFIGS:
        if only and name not in only:
            continue
        kw = dict(DRIVER)
        kw.update(over)
        res = run_plan(mod, kw, seed)
        fails = res["cand_fail"]
        # "wrap": a goal yaw next to +-pi -- a candidate that reached the goal and whose only failed test is the final angle
        shown = {"flag": res["flag"] == 1, "none": len(res["cand"]) == 0 and res["flag"] == 0,
                 "any": len(res["cand"]) > 0, "wrap": bool(np.any(fails == F_ANGLE))}.get(want)
        if shown is None:
            shown = bool(np.any(fails & want))
        print(name, len(res["x"]), "nodes", len(res["cand"]), "candidates, flag", res["flag"], "len(t)",
              len(res["out_t"]), "fail masks", fails.tolist(), "lens", res["cand_len"].tolist(),
              "KEPT" if shown else "NOT KEPT (does not show %r)" % (want,), flush=True)
        if shown:
            np.savez_compressed(os.path.join(GOLD, "rrt10_%s.npz" % name), **res)
    if not only or "kat" in only:
        kat(mod)


if __name__ == "__main__":
    main()

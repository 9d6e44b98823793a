"""Golden generator of BatchPlanner.track_goals (rrtx_track_goals): runs the reference's ClosedLoopRRTStar, and per goal
sets `end`, `xy_th`, `yaw_th` on the finished planner and calls get_goal_indexes() + search_best_feasible_path(), the tail
of planning() (rrt_10:1488-1493).  Writes tests/golden/goal_track_kat.npz (data only).  Build host only (needs the
reference checkout); the loader and the message-reading wrapper are tools/gen_golden_closed_loop.py's.

    python tools/gen_golden_goal_track.py

Trees: "main" is the driver cell with seed 3 and max_iter=100, stored in the file (tree, polylines, kwargs).  Two further
trees are re-planned from the kwargs and seed of existing goldens (rrt10_coll_s2, rrt10_map_b_s12); the generator asserts
that its tree equals the stored one bit for bit and the file only names the golden.

Per call `c<k>` (one tree, one parameter set, g goals):
  c<k>_tree, c<k>_params (target_speed, yaw_th, xy_th, invalid_travel_ratio), c<k>_goals (g, 3)
  c<k>_cand_off (g + 1), c<k>_cand: the candidate nodes of every query, flat
  c<k>_find / _len / _tlast / _fail / _ood / _last / _sums: one row per candidate.  ood = 2 marks a candidate whose course the
      reference raises on (fewer than 3 points, extend_path :1435); its other columns are 0
  c<k>_raises (g): the reference's call raised; c<k>_flag (g), c<k>_winner (g): position in the query's candidate list, -1
  c<k>_wlen (g): len(t) of the winner (0 none); c<k>_arr_off (g + 1): exclusive sum of wlen + 1 over the flagged queries
  c<k>_out (7, arr_off[-1]): x, y, yaw (wlen + 1 entries: the goal pose appended) and v, t, a, d (wlen, then one NaN)
The winner position is found by applying :1510 (`flag and best_time >= t[-1]`) to the records; the generator asserts that
this position reproduces the tuple search_best_feasible_path returned.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_closed_loop import DRIVER, GOLD, MODEL, load, wrap_feasible  # noqa: E402

REF_TH = (float(np.deg2rad(3.0)), 0.5)      # yaw_th, xy_th of the reference
GRID = [[float(x), float(y), float(w)] for x in (2, 6, 10, 14) for y in (0, 4, 8, 12) for w in (0.0, 1.57)]
ODD = [[float("nan"), 4.0, 0.0], [6.0, float("inf"), 1.57]]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def plan(mod, kw, seed):
    random.seed(seed)
    obj = mod.ClosedLoopRRTStar(**kw)
    with contextlib.redirect_stdout(io.StringIO()):
        mod.RRTStarReedsShepp.planning(obj, animation=False)      # the tree only (:1485)
    return obj


def tree_of(obj):
    nodes = obj.node_list
    index = {id(nd): i for i, nd in enumerate(nodes)}
    return dict(x=np.array([float(n.x) for n in nodes]), y=np.array([float(n.y) for n in nodes]),
                yaw=np.array([float(n.yaw) for n in nodes]),
                parent=np.array([index[id(n.parent)] if n.parent is not None else -1 for n in nodes], dtype=np.int32),
                plen=np.array([len(n.path_x) for n in nodes], dtype=np.int32),
                px=np.array([float(q) for n in nodes for q in n.path_x]),
                py=np.array([float(q) for n in nodes for q in n.path_y]),
                pyaw=np.array([float(q) for n in nodes for q in n.path_yaw]))


def ask(obj, goal, records):
    """One query: (candidates, records, raised, returned tuple or None)."""
    obj.end = obj.Node(goal[0], goal[1], goal[2])
    del records[:]
    with contextlib.redirect_stdout(io.StringIO()):
        cands = [int(i) for i in obj.get_goal_indexes()]
        raised, ret = False, None
        try:
            ret = obj.search_best_feasible_path(cands)
        except IndexError:
            raised = True
    recs = [dict(r, ood=0) for r in records]
    if raised:   # the records of the candidates the loop did not reach, one by one
        recs = []
        for ind in cands:
            del records[:]
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    obj.check_tracking_path_is_feasible(obj.generate_final_course(ind))
                recs.append(dict(records[0], ood=0))
            except IndexError:
                recs.append(dict(find=False, n=0, tlast=0.0, fail=0, ood=2, last=[0.0] * 6, sums=[0.0] * 6))
    assert len(recs) == len(cands)
    return cands, recs, raised, ret


def call(mod, obj, params, goals, out, key, tree):
    ts, yth, xyth, ratio = params
    obj.target_speed, obj.yaw_th, obj.xy_th, obj.invalid_travel_ratio = ts, yth, xyth, ratio
    records = []
    wrap_feasible(obj, records)
    off, cand, rows, raises, flags, winners, wlens, arr_off, cols = [0], [], [], [], [], [], [], [0], [[] for _ in range(7)]
    for goal in goals:
        cands, recs, raised, ret = ask(obj, goal, records)
        best, win = float("inf"), -1
        for k, r in enumerate(recs):                       # :1510
            if r["find"] and best >= r["tlast"]:
                best, win = r["tlast"], k
        if raised:
            win = -1
        else:
            assert bool(ret[0]) == (win >= 0), (goal, ret[0], win)
        wl = 0
        if win >= 0:
            _, x, y, yaw, v, t, a, d = ret
            r = recs[win]
            wl = len(t)
            # the returned tuple is the record at `win`: same length, end time, last state and sums (x, y, yaw before the append)
            assert wl == r["n"] and float(t[-1]) == r["tlast"] and len(x) == wl + 1
            assert [float(x[-2]), float(y[-2]), float(yaw[-2]), float(v[-1]), float(a[-1]), float(d[-1])] == r["last"]
            assert [float(sum(x[:-1])), float(sum(y[:-1])), float(sum(yaw[:-1]))] == r["sums"][:3]
            assert [float(x[-1]), float(y[-1]), float(yaw[-1])] == [float(q) for q in goal]
            for c, arr in zip(cols, (x, y, yaw, list(v) + [math.nan], list(t) + [math.nan], list(a) + [math.nan],
                                     list(d) + [math.nan])):
                c += [float(q) for q in arr]
            arr_off.append(arr_off[-1] + wl + 1)
        else:
            arr_off.append(arr_off[-1])
        cand += cands
        rows += recs
        off.append(len(cand))
        raises.append(int(raised))
        flags.append(int(win >= 0))
        winners.append(win)
        wlens.append(wl)
    obj.check_tracking_path_is_feasible = type(obj).check_tracking_path_is_feasible.__get__(obj)
    out[key + "_tree"] = tree
    out[key + "_params"] = np.array(params, dtype=np.float64)
    out[key + "_goals"] = np.array(goals, dtype=np.float64).reshape(-1, 3)
    out[key + "_cand_off"] = np.array(off, dtype=np.int64)
    out[key + "_cand"] = np.array(cand, dtype=np.int32)
    for name, col, dt in (("find", "find", np.int32), ("len", "n", np.int32), ("tlast", "tlast", np.float64),
                          ("fail", "fail", np.int32), ("ood", "ood", np.int32)):
        out["%s_%s" % (key, name)] = np.array([r[col] for r in rows], dtype=dt)
    out[key + "_last"] = np.array([r["last"] for r in rows], dtype=np.float64).reshape(-1, 6)
    out[key + "_sums"] = np.array([r["sums"] for r in rows], dtype=np.float64).reshape(-1, 6)
    out[key + "_raises"] = np.array(raises, dtype=np.int32)
    out[key + "_flag"] = np.array(flags, dtype=np.int32)
    out[key + "_winner"] = np.array(winners, dtype=np.int32)
    out[key + "_wlen"] = np.array(wlens, dtype=np.int32)
    out[key + "_arr_off"] = np.array(arr_off, dtype=np.int64)
    out[key + "_out"] = np.array(cols, dtype=np.float64).reshape(7, -1)
    n = np.diff(off)
    print(key, tree, "params", params, "goals", len(goals), "candidates", n.tolist(), "flags", flags, "winners", winners,
          "raises", raises, "fail masks", sorted(set(int(r["fail"]) for r in rows)), "steps", int(sum(wlens)), flush=True)


def main():
    mod = load()
    out = dict(model=json.dumps(MODEL))
    ts, ratio = DRIVER["target_speed"], DRIVER["invalid_travel_ratio"]
    # ---- the mandatory tree
    kw = dict(DRIVER, max_iter=100)
    obj = plan(mod, kw, 3)
    tr = tree_of(obj)
    print("main:", len(tr["x"]), "nodes", flush=True)
    out["main_seed"] = 3
    out["main_kwargs"] = json.dumps(kw)
    for k, v in tr.items():
        out["main_" + k] = v
    own = [list(map(float, kw["goal"]))]
    near = [[float(tr["x"][n] + 0.1), float(tr["y"][n] - 0.1), float(tr["yaw"][n] + 0.01)]
            for n in (5, 20, 40, 64, 80, 100) if n < len(tr["x"])]
    call(mod, obj, (ts, REF_TH[0], REF_TH[1], ratio), own + near, out, "c0", "main")
    call(mod, obj, (ts, REF_TH[0], REF_TH[1], 1.0), own, out, "c1", "main")
    call(mod, obj, (ts, 0.8, 3.0, ratio), GRID + ODD, out, "c2", "main")
    call(mod, obj, (ts, 1.6, 5.0, ratio), GRID + ODD, out, "c3", "main")
    # ---- two further trees, re-planned from existing goldens
    k = 4
    for name in ("rrt10_coll_s2", "rrt10_map_b_s12"):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        gkw = json.loads(str(g["kwargs"]))
        obj = plan(mod, gkw, int(g["seed"]))
        tr = tree_of(obj)
        for col in ("x", "y", "yaw", "px", "py", "pyaw"):
            assert np.array_equal(bits(tr[col]), bits(g[col])), (name, col)
        assert np.array_equal(tr["parent"], g["parent"]) and np.array_equal(tr["plen"], g["plen"]), name
        own = [list(map(float, gkw["goal"]))]
        few = [[2.0, 0.0, 0.0], [6.0, 8.0, 1.57], [6.0, 12.0, 1.57], [10.0, 8.0, 1.57], [2.0, 4.0, 0.0]]
        call(mod, obj, (gkw["target_speed"], gkw["yaw_th"], gkw["xy_th"], gkw["invalid_travel_ratio"]), own, out, "c%d" % k, name)
        call(mod, obj, (gkw["target_speed"], 0.8, 3.0, gkw["invalid_travel_ratio"]), few, out, "c%d" % (k + 1), name)
        k += 2
    out["n_calls"] = k
    path = os.path.join(GOLD, "goal_track_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()

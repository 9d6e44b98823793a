"""BatchPlanner.track_goals (rrtx_track_goals) without a GPU: tests/goal_track_oracle.py on the golden trees against the
reference's own answers (tests/golden/goal_track_kat.npz), the conditions that file has to show, csrc/rpp_goaltrack.h compiled
for the CPU (pick rule, both exclusive sums, the candidate test on goals that are no numbers), the ABI surface, the argument
checks that need no device, and the Python ValueErrors."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import goal_track_oracle as gt
import track_util as tu
import util

KAT = os.path.join(tu.GOLD, "goal_track_kat.npz")
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if os.environ.get("RRTX_TEST_SANITIZE") else []
NEW_FUNCS = ("rrtx_track_goals", "rrtx_get_goal_track", "rrtx_get_goal_track_records", "rrtx_get_goal_track_arrays",
             "rrtx_get_goal_track_kernel_ms", "rrtx_get_polyline_yaw")
E_INVALID, E_STATE = -1, -5
TREE_KEYS = ("x", "y", "yaw", "parent", "plen", "px", "py", "pyaw")


@pytest.fixture(scope="module")
def golden():
    return np.load(KAT)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return gt.build(tmp_path_factory.mktemp("goal_track"), SAN)


def calls_of(g):
    return ["c%d" % c for c in range(int(g["n_calls"]))]


def tree_of(g, name):
    if name == "main":
        return {k: g["main_" + k] for k in TREE_KEYS}, json.loads(str(g["main_kwargs"]))
    t, kw, _ = tu.load(os.path.join(tu.GOLD, name + ".npz"))
    return {k: t[k] for k in TREE_KEYS}, kw


def run_exe(exe, mode, data, tmp_path):
    fin, fout = str(tmp_path / (mode + "_in.bin")), str(tmp_path / (mode + "_out.bin"))
    np.asarray(data, dtype=np.float64).tofile(fin)
    subprocess.run([exe, mode, fin, fout], check=True)
    return np.fromfile(fout, dtype=np.float64)


# ---- the oracle against the reference ---------------------------------------------------------------------------------------------
def test_oracle_reproduces_every_golden_call(golden, exe, tmp_path):
    g = golden
    model = json.loads(str(g["model"]))
    assert len(calls_of(g)) >= 8 and str(g["c0_tree"]) == "main" and int(g["main_seed"]) == 3
    assert json.loads(str(g["main_kwargs"]))["max_iter"] == 100 and len(g["main_x"]) == 111
    for key in calls_of(g):
        tree, kw = tree_of(g, str(g[key + "_tree"]))
        P = dict(model, **dict(zip(tu.PORDER[:4], g[key + "_params"].tolist())))
        ans = gt.answer(exe, tmp_path, [(tree, kw["start"], kw["obstacle_list"], kw["robot_radius"], goal) for goal in g[key + "_goals"]], P)
        co, ao = g[key + "_cand_off"], g[key + "_arr_off"]
        assert ao[-1] == g[key + "_out"].shape[1] == int((g[key + "_wlen"] + 1)[g[key + "_flag"] != 0].sum())
        for q, a in enumerate(ans):
            s, what = slice(co[q], co[q + 1]), (key, q)
            assert np.array_equal(a["cand"], g[key + "_cand"][s]), what
            for col, name in enumerate(("find", "len", "fail", "ood")):
                assert np.array_equal(a["rec"][:, col], g["%s_%s" % (key, name)][s]), (what, name)
            assert np.array_equal(tu.bits(a["rec"][:, 4]), tu.bits(g[key + "_tlast"][s])), what
            assert (a["flag"], a["winner"], a["len"]) == (int(g[key + "_flag"][q]), int(g[key + "_winner"][q]), int(g[key + "_wlen"][q])), what
            assert bool(a["status"] & gt.ST_REF_RAISES) == bool(g[key + "_raises"][q]) and not a["status"] & ~gt.ST_REF_RAISES, what
            if a["flag"]:
                assert np.array_equal(tu.bits(a["arr"]), tu.bits(g[key + "_out"][:, ao[q]:ao[q + 1]])), what
                assert np.array_equal(tu.bits(a["arr"][[0, 1, 2, 3, 5, 6], [-2, -2, -2, -2, -2, -2]]), tu.bits(g[key + "_last"][co[q] + a["winner"]]))
                sums = [float(sum(a["arr"][r, :-1].tolist())) for r in (0, 1, 2, 3, 5, 6)]
                assert np.array_equal(tu.bits(sums), tu.bits(g[key + "_sums"][co[q] + a["winner"]])), what
            else:
                assert ao[q] == ao[q + 1]


def test_golden_set_shows_every_condition(golden):
    g = golden
    n, raises, flag, winner, fails, first_tie, own = [], [], [], [], set(), False, False
    below_and_above = none_feasible = False
    for key in calls_of(g):
        co = g[key + "_cand_off"]
        for q, goal in enumerate(g[key + "_goals"]):
            s = slice(co[q], co[q + 1])
            cnt = int(co[q + 1] - co[q])
            n.append(cnt)
            raises.append(int(g[key + "_raises"][q]))
            flag.append(int(g[key + "_flag"][q]))
            winner.append(int(g[key + "_winner"][q]))
            fails |= set(int(f) for f in g[key + "_fail"][s])
            nodes = g[key + "_cand"][s]
            below_and_above |= cnt > 0 and nodes.min() < 64 <= nodes.max()                          # (c)
            feasible = g[key + "_find"][s] != 0
            none_feasible |= cnt > 0 and not feasible.any() and not raises[-1] and not flag[-1]     # (f)
            if flag[-1]:
                tl = g[key + "_tlast"][s]
                ties = np.nonzero(feasible & (tl == tl[feasible].min()))[0]
                first_tie |= len(ties) >= 2 and winner[-1] == ties[-1]                              # (e)
            if not np.isfinite(goal).all():
                assert cnt == 0 and not flag[-1] and not raises[-1]                                 # (a) NaN and +inf
        if key == "c0":
            kw = json.loads(str(g["main_kwargs"]))
            own = g["c0_goals"][0].tolist() == kw["goal"] and g["c0_params"][1:3].tolist() == [math.radians(3.0), 0.5] and n[0] == 31   # (i)
    goals = np.concatenate([g[k + "_goals"] for k in calls_of(g)])
    assert np.isnan(goals).any() and np.isposinf(goals).any() and 0 in n                            # (a)
    assert 1 in n and any(2 <= c <= 8 for c in n) and any(c >= 27 for c in n)                       # (b)
    assert below_and_above                                                                          # (c)
    assert any(w > 0 for w in winner)                                                               # (d)
    assert first_tie and none_feasible and any(raises) and own                                      # (e) (f) (g) (i)
    assert all(any(f & bit for f in fails) for bit in (1, 2, 4, 8))                                 # (h)
    assert os.path.getsize(KAT) < 1000000


# ---- rpp_goaltrack.h on the CPU ---------------------------------------------------------------------------------------------------
def pick_rows(n, no_tree, rows):
    return [n, no_tree] + [v for r in rows for v in r]


def test_pick_rule_ties_refusals_and_the_empty_list(exe, tmp_path):
    ok = lambda t, node, n=300, find=1: [find, n, 0 if find else 2, 0, t, node]      # noqa: E731
    queries = [
        pick_rows(3, 0, [ok(11.0, 5), ok(12.0, 6), ok(11.0, 9)]),                     # two equal times: the later wins
        pick_rows(6, 0, [ok(9.5, 1), ok(9.0, 2), ok(9.0, 3, find=0), ok(9.0, 4), ok(9.0, 7, n=181), ok(9.0, 8, n=182)]),   # four
        pick_rows(3, 0, [ok(11.0, 5), [0, 0, 0, 2, 0.0, 0], ok(10.0, 9)]),            # one refused record (the reference raises)
        pick_rows(2, 0, [[0, 0, 0, 3, 0.0, 4], [0, 7, 0, 1, 0.3, 5]]),                # overflow and out-of-domain together
        pick_rows(0, 0, []),                                                          # no candidate
        pick_rows(0, 1, []),                                                          # no tree
        pick_rows(2, 0, [ok(5.0, 3, find=0), ok(4.0, 4, find=0)]),                    # candidates, none feasible
        pick_rows(1, 0, [ok(float("inf"), 3)]),                                       # `inf >= inf`: a feasible roll-out of infinite time wins
    ]
    out = run_exe(exe, "pick", np.concatenate(queries), tmp_path).reshape(-1, 8)
    inf = float("inf")
    want = [[1, 2, 3, 300, 9, 0, 0, 11.0], [1, 5, 6, 182, 8, 0, 0, 9.0], [0, -1, 3, 0, -1, 32, 0, inf], [0, -1, 2, 0, -1, 4 | 16, 0, inf],
            [0, -1, 0, 0, -1, 0, 0, inf], [0, -1, 0, 0, -1, 0, 1, inf], [0, -1, 2, 0, -1, 0, 0, inf], [1, 0, 1, 300, 3, 0, 0, inf]]
    assert out.tolist() == want
    for q, w in zip(queries, want):                                                   # and the plain-Python pick agrees
        rows = np.array(q[2:]).reshape(-1, 6)
        a = gt.pick(rows[:, 5].astype(int), [tuple(r[:5]) for r in rows])
        assert [a["flag"], a["winner"], a["n_cand"], a["len"], a["node"], a["status"], a["t_last"]] == w[:6] + [w[7]]


def test_both_exclusive_sums(exe, tmp_path):
    counts = [3, 0, -1, 5, 1]                                                         # -1: the no-tree mark counts nothing
    fl = [(1, 220), (0, 0), (0, 0), (1, 2002), (0, 17)]                               # len of an unflagged query is not counted
    data = [5, 1 << 24] + counts + [v for p in fl for v in p]
    out = run_exe(exe, "sums", data, tmp_path).tolist()
    assert out == [9, 0, 3, 3, 3, 8, 9, 221 + 2003, 0, 221, 221, 221, 2224, 2224]
    out = run_exe(exe, "sums", [5, 8] + counts + [v for p in fl for v in p], tmp_path).tolist()
    assert out[0] == -1 and out[1] == 2224                                            # more candidates than the cap: refused
    out = run_exe(exe, "sums", [5, 9] + counts + [v for p in fl for v in p], tmp_path).tolist()
    assert out[0] == 9
    assert run_exe(exe, "sums", [0, 4], tmp_path).tolist() == [0, 0, 0, 0]            # no query at all


def test_candidate_test_equals_get_goal_indexes_and_odd_goals_find_nothing(golden, exe, tmp_path):
    g = golden
    tree = {k: g["main_" + k] for k in TREE_KEYS}
    nan, inf = float("nan"), float("inf")
    odd = [[nan, 4.0, 0.0], [4.0, nan, 0.0], [4.0, 4.0, nan], [inf, 4.0, 0.0], [4.0, -inf, 0.0], [4.0, 4.0, inf], [-inf, inf, nan],
           [1e308, 4.0, 0.0], [4.0, -1.7e308, 0.0], [4.0, 4.0, 1e308], [1e300, 1e300, 0.0]]
    goals = np.concatenate([g["c2_goals"], np.array(odd), np.column_stack([tree["x"], tree["y"], tree["yaw"]])[::9]])
    for xy_th, yaw_th in ((0.5, math.radians(3.0)), (3.0, 0.8), (5.0, 1.6), (0.0, 0.0)):
        data = np.concatenate([[xy_th, yaw_th, len(tree["x"])], tree["x"], tree["y"], tree["yaw"], [len(goals)], goals.reshape(-1)])
        out = run_exe(exe, "cand", data, tmp_path).astype(np.int64).tolist()
        pos = 0
        for j, goal in enumerate(goals):
            want = gt.candidates(tree, goal, xy_th, yaw_th)
            assert out[pos] == len(want) and out[pos + 1:pos + 1 + len(want)] == want, (xy_th, j)
            pos += 1 + len(want)
            if not np.isfinite(goal).all() or np.abs(goal).max() > 1e200:
                assert want == []
        assert pos == len(out)
    assert gt.candidates(tree, [float(tree["x"][9]), float(tree["y"][9]), float(tree["yaw"][9])], 0.0, 0.0) != []   # thresholds are `<=`


def test_course_layout_and_refusals_of_the_host_core(golden, exe, tmp_path):
    g = golden
    tree, kw = tree_of(g, "main")
    model = json.loads(str(g["model"]))
    P = dict(model, **dict(zip(tu.PORDER[:4], g["c2_params"].tolist())))
    goal = [2.0, 0.0, 0.0]
    root = gt.course(tree, 0, kw["start"], goal)
    assert [len(c) for c in root] == [2, 2, 2] and [c[0] for c in root] == kw["start"] and [c[-1] for c in root] == goal
    node = int(np.nonzero(tree["parent"] > 0)[0][0])                                  # a node two edges below the root
    cx, cy, cw = gt.course(tree, node, kw["start"], goal)
    par = int(tree["parent"][node])
    assert len(cx) == 2 + int(tree["plen"][node]) + int(tree["plen"][par])
    off = np.concatenate([[0], np.cumsum(tree["plen"])])
    assert cx[1:1 + int(tree["plen"][par])] == tree["px"][off[par]:off[par + 1]].tolist()          # root -> node: the parent's edge first
    long_course = [np.linspace(0.0, 50.0, 961).tolist(), [0.0] * 961, [0.0] * 961]
    jobs = [tu.job(P, kw["obstacle_list"], 0.0, *c) for c in (root, (cx, cy, cw), long_course, [v[:960] for v in long_course])]
    res = gt.roll(exe, tmp_path, jobs)
    assert [r[3] for r in res] == [2, 0, 3, 0] and res[0][:3] == (0, 0, 0) and res[1][1] > 0       # raises, rolled, too long, just fits


# ---- ABI and Python ---------------------------------------------------------------------------------------------------------------
def test_new_entry_points_declared_exported_mirrored_and_version_still_6():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    assert int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1)) == A.RRTX_ABI_VERSION == 6
    raw = C.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    L = A.load()
    for fn in NEW_FUNCS:
        assert re.search(r"\bint %s\(" % fn, hdr), fn
        assert hasattr(raw, fn), fn
        assert fn in A.EXPORTS and getattr(L, fn).argtypes is not None and getattr(L, fn).restype is C.c_int, fn
    fields = re.search(r"typedef struct rrtx_goal_track_outcome \{(.*?)\} rrtx_goal_track_outcome;", hdr, re.S).group(1)
    names = re.findall(r"\b([A-Za-z_]+)(?=;)", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f for f, _ in A.GoalTrackOutcome._fields_] == list(A.GOAL_TRACK_OUTCOME.names)
    assert C.sizeof(A.GoalTrackOutcome) == A.GOAL_TRACK_OUTCOME.itemsize == 40 and A.GoalTrackOutcome.t_last.offset == 32
    assert A.GOAL_TRACK_OUTCOME.fields["t_last"][1] == 32
    src = open(os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc", "rpp_goaltrack.h")).read()
    assert "constexpr int ST_OVERFLOW = 4, ST_OOD = 16, ST_RAISES = 32;" in src
    assert (A.ST_OVERFLOW, A.ST_UNSUPPORTED, A.ST_REF_RAISES) == (gt.ST_OVERFLOW, gt.ST_UNSUPPORTED, gt.ST_REF_RAISES) == (4, 16, 32)
    assert rrt_amd.GoalTrackResult is rrt_amd.planner.GoalTrackResult and hasattr(rrt_amd.BatchPlanner, "track_goals")


def test_argument_and_state_checks_come_before_any_device_call():
    import rrt_amd
    A = rrt_amd._abi
    L = A.load()
    goals = np.zeros((4, 3))
    tp = A.TrackParams(**A.TRACK_DEFAULTS)
    n, ms = C.c_int64(), C.c_double()
    assert L.rrtx_track_goals(None, C.byref(tp), 4, 0, goals.ctypes.data, 1) == E_INVALID
    assert L.rrtx_get_goal_track(None, None, None, None, 0, C.byref(n), C.byref(n), C.byref(n)) == E_INVALID
    assert L.rrtx_get_goal_track_records(None, None, None, 0) == E_INVALID
    assert L.rrtx_get_goal_track_arrays(None, None, None, None, None, None, None, None, 0) == E_INVALID
    assert L.rrtx_get_goal_track_kernel_ms(None, C.byref(ms), C.byref(ms), C.byref(ms)) == E_INVALID
    assert L.rrtx_get_polyline_yaw(None, 0, goals.ctypes.data, 12) == E_INVALID
    if L.rrtx_device_count() == 0:
        return                                                              # rrtx_create hands out no handle without a device
    bad_tp = A.TrackParams(**dict(A.TRACK_DEFAULTS, steer_max=1.0))
    for algo in (A.ALGO_RRT, A.ALGO_RRT_STAR, A.ALGO_DUBINS):
        h = A.Handle(algo, [0.0, 0.0, 0.0], [6.0, 7.0, 0.0], [-2.0, 15.0], 3.0, 0.5, 10, 20, n_instances=2)
        try:
            assert L.rrtx_track_goals(h._h, C.byref(tp), 0, 0, goals.ctypes.data, 1) == E_INVALID          # arguments first ...
            assert L.rrtx_track_goals(h._h, C.byref(tp), 4, 0, goals.ctypes.data, 1) == E_STATE            # ... then the algo
            assert b"RRTX_ALGO_RS" in L.rrtx_last_error(h._h)
        finally:
            h.close()
    h = A.Handle(A.ALGO_RS, [0.0, 0.0, 0.0], [6.0, 7.0, 1.5], [-2.0, 15.0], 3.0, 0.5, 10, 20, curvature=1.0,
                 goal_yaw_th=0.02, goal_xy_th=0.5, step_size=0.2, n_instances=4)
    try:
        for args in ((None, 4, 0, goals.ctypes.data), (C.byref(tp), 4, 0, None), (C.byref(tp), 0, 0, goals.ctypes.data),
                     (C.byref(tp), -3, 0, goals.ctypes.data), (C.byref(tp), 4, 2, goals.ctypes.data), (C.byref(tp), 4, -1, goals.ctypes.data),
                     (C.byref(tp), (1 << 22) + 1, 0, goals.ctypes.data), (C.byref(bad_tp), 4, 0, goals.ctypes.data)):
            assert L.rrtx_track_goals(h._h, *args, 1) == E_INVALID, args[1:3]
        assert b"steer_max" in L.rrtx_last_error(h._h)
        for cost in (A.RS_COST_EUCLID, A.RS_COST_PATH):                                                    # either cost, never planned
            h.set_rs_cost(cost)
            assert L.rrtx_track_goals(h._h, C.byref(tp), 4, 0, goals.ctypes.data, 1) == E_STATE
            assert b"no completed plan" in L.rrtx_last_error(h._h)
        assert L.rrtx_get_goal_track(h._h, None, None, None, 0, C.byref(n), C.byref(n), C.byref(n)) == E_STATE
        assert L.rrtx_get_goal_track_records(h._h, None, None, 0) == E_STATE
        assert L.rrtx_get_goal_track_arrays(h._h, None, None, None, None, None, None, None, 0) == E_STATE
        assert L.rrtx_get_goal_track_kernel_ms(h._h, C.byref(ms), C.byref(ms), C.byref(ms)) == E_STATE
        L.rrtx_plan_begin(h._h)                                                                            # a plan in progress
        assert L.rrtx_track_goals(h._h, C.byref(tp), 4, 0, goals.ctypes.data, 1) == E_STATE
        assert b"in progress" in L.rrtx_last_error(h._h)
    finally:
        h.close()


def forged_planner(algo, closed_loop=False, n=3):
    import rrt_amd
    bp = rrt_amd.BatchPlanner.__new__(rrt_amd.BatchPlanner)                  # refused before any handle is touched
    bp.algo, bp.closed_loop, bp.handles, bp.seeds, bp.shards = algo, closed_loop, [None], [0] * n, [(0, n)]
    return bp


def test_value_errors_need_no_device():
    import rrt_amd
    A = rrt_amd._abi
    goals = np.zeros((4, 3))
    for algo in (A.ALGO_RRT, A.ALGO_RRT_STAR, A.ALGO_DUBINS, A.ALGO_RS, A.ALGO_INFORMED, A.ALGO_BITSTAR, A.ALGO_RRT_DUBINS, A.ALGO_LQR_RRT_STAR):
        with pytest.raises(ValueError, match="closed_loop_rrt_star"):
            forged_planner(algo).track_goals(goals)
    with pytest.raises(TypeError, match="unknown keyword"):
        forged_planner(A.ALGO_RS, closed_loop=True).track_goals(goals, speed=1.0)
    with pytest.raises(ValueError, match="'rrt_star', 'rrt_star_dubins', 'rrt_star_reeds_shepp'"):
        forged_planner(A.ALGO_RS, closed_loop=True).query_goals(goals)       # query_goals goes on refusing rrt_10 trees
    T = rrt_amd.planner.goal_query_table                                     # the goal table is query_goals': its errors too
    for bad in (np.zeros(3), np.zeros((4, 4)), np.zeros((0, 3)), np.zeros((2, 4, 3)), np.zeros((3, 0, 3))):
        with pytest.raises(ValueError, match="goals"):
            T(bad, 3, True, 0.0)
    t, per = T([[1.0, 2.0], [3.0, float("nan")]], 3, True, 1.5)
    assert not per and t.shape == (2, 3) and t[:, 2].tolist() == [1.5, 1.5]


def test_goal_track_result_built_by_hand():
    import rrt_amd
    A = rrt_amd._abi
    out = np.zeros(4, dtype=A.GOAL_TRACK_OUTCOME)
    out["flag"], out["winner"], out["len"], out["node"] = [1, 0, 1, 1], [1, -1, 0, 0], [2, 0, 3, 1], [7, -1, 4, 9]
    out["n_cand"], out["status"], out["t_last"] = [2, 1, 1, 1], [0, 32, 0, 0], [5.0, np.inf, 5.0, 4.0]
    rec = np.zeros(5, dtype=A.TRACK_RECORD)
    rec["ood"][2] = 2
    ao = np.array([0, 3, 3, 7, 9])
    arrays = [np.arange(9.0) + 10 * k for k in range(7)]
    res = rrt_amd.GoalTrackResult(out, (2, 2), [0, 2, 3, 4, 5], np.array([5, 7, 0, 4, 9], dtype=np.int32), rec, ao, arrays, (1.0, 2.0, 3.0))
    assert res.shape == (2, 2) and res.flag.tolist() == [[True, False], [True, True]] and res.partial
    assert res.best_goal().tolist() == [0, 1]                                # the smallest t_last among the flagged goals
    x, y, yaw, v, t, a, d = res.trajectory(1, 0)
    assert x.tolist() == [3.0, 4.0, 5.0, 6.0] and v.tolist() == [33.0, 34.0, 35.0] and len(yaw) == 4 and len(d) == 3
    assert res.trajectory(0, 1) is None and res.trajectory(-1, -1)[0].tolist() == [7.0, 8.0]
    cand, r = res.records(0, 1)
    assert cand.tolist() == [0] and r["ood"].tolist() == [2] and res.cand_ood.tolist() == [0, 0, 2, 0, 0]
    with pytest.raises(IndexError):
        res.records(2, 0)
    bare = rrt_amd.GoalTrackResult(out, (2, 2), [0, 2, 3, 4, 5], np.array([5, 7, 0, 4, 9], dtype=np.int32), rec)
    assert bare.arr_offsets is None and bare.x is None
    with pytest.raises(ValueError, match="arrays=False"):
        bare.trajectory(0, 0)
    none = np.zeros(2, dtype=A.GOAL_TRACK_OUTCOME)
    none["t_last"] = np.inf
    assert rrt_amd.GoalTrackResult(none, (1, 2), [0, 0, 0], np.zeros(0, np.int32), rec[:0]).best_goal().tolist() == [-1]

"""BatchPlanner.track_goals on the device: rrt_10's closed-loop stage for many goals from the planned trees
(rrtx_track_goals).  The yardsticks are the reference's own answers (tests/golden/goal_track_kat.npz,
tools/gen_golden_goal_track.py), the planner's own track() at its own goal, and tests/goal_track_oracle.py (the rules in plain
Python, the roll-out through the compiled host core) on the trees read back from the device.  Everything is compared bit for
bit: there are no tolerances."""
import json
import os

import numpy as np
import pytest

import goal_track_oracle as gt
import track_util as tu

pytestmark = pytest.mark.gpu
KAT = os.path.join(tu.GOLD, "goal_track_kat.npz")
FIELDS = ("flag", "winner", "n_cand", "len", "node", "status")


@pytest.fixture(scope="module")
def golden():
    return np.load(KAT)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return gt.build(tmp_path_factory.mktemp("goal_track"))


def planner(seeds, kw, **extra):
    import rrt_amd
    args = dict(seeds=seeds, start=kw["start"], goal=kw["goal"], obstacle_list=kw["obstacle_list"], rand_area=kw["rand_area"],
                max_iter=kw["max_iter"], connect_circle_dist=kw["connect_circle_dist"], robot_radius=kw["robot_radius"])
    args.update(extra)
    return rrt_amd.BatchPlanner("closed_loop_rrt_star", **args)


def device_tree(bp, i):
    x, y, _, parent = bp.tree(i)
    plen, px, py = bp.polylines(i)
    return dict(x=x, y=y, yaw=bp.yaw(i), parent=parent, plen=plen, px=px, py=py, pyaw=bp.polyline_yaw(i))


def assert_query(res, i, j, want, what):
    """Query (i, j) of a GoalTrackResult against an oracle answer (goal_track_oracle.answer's dict)."""
    cand, rec = res.records(i, j)
    assert np.array_equal(cand, want["cand"]), what
    got = np.column_stack([rec["find_goal"], rec["len"], rec["fail"], rec["ood"]])
    assert np.array_equal(got, want["rec"][:, :4].astype(np.int64)), what
    assert np.array_equal(tu.bits(rec["t_last"]), tu.bits(want["rec"][:, 4])), what
    for k in FIELDS:
        assert int(getattr(res, k)[i, j]) == int(want[k]), (what, k)
    assert tu.bits([res.t_last[i, j]])[0] == tu.bits([want["t_last"]])[0], what
    if res.arr_offsets is not None:
        tr = res.trajectory(i, j)
        assert (tr is None) == (want["arr"] is None), what
        if tr is not None:
            for k, a in enumerate(tr):
                assert np.array_equal(tu.bits(a), tu.bits(want["arr"][k, :len(a)])), (what, k)
            q = i * res.shape[1] + j
            flat = np.stack([getattr(res, n)[res.arr_offsets[q]:res.arr_offsets[q + 1]] for n in res.ARRAYS])
            assert np.array_equal(tu.bits(flat), tu.bits(want["arr"])), what     # the NaN slots included


# ---- 1. the reference's answers -------------------------------------------------------------------------------------------------
def golden_trees(g):
    names = sorted(set(str(g["c%d_tree" % c]) for c in range(int(g["n_calls"]))))
    out = {}
    for name in names:
        if name == "main":
            out[name] = (json.loads(str(g["main_kwargs"])), int(g["main_seed"]), {k: g["main_" + k] for k in
                                                                                ("x", "y", "yaw", "parent", "plen", "px", "py", "pyaw")})
        else:
            t, kw, _ = tu.load(os.path.join(tu.GOLD, name + ".npz"))
            out[name] = (kw, int(t["seed"]), {k: t[k] for k in ("x", "y", "yaw", "parent", "plen", "px", "py", "pyaw")})
    return out


@pytest.mark.parametrize("name", ["main", "rrt10_coll_s2", "rrt10_map_b_s12"])
def test_golden_calls_equal_the_reference(golden, name):
    g = golden
    kw, seed, tree = golden_trees(g)[name]
    model = json.loads(str(g["model"]))
    bp = planner([seed], kw)
    try:
        bp.plan()
        dev = device_tree(bp, 0)
        for k in ("x", "y", "yaw", "px", "py", "pyaw"):
            assert np.array_equal(tu.bits(dev[k]), tu.bits(tree[k])), k
        assert np.array_equal(dev["parent"], tree["parent"]) and np.array_equal(dev["plen"], tree["plen"])
        calls = [c for c in range(int(g["n_calls"])) if str(g["c%d_tree" % c]) == name]
        assert calls
        for c in calls:
            key = "c%d" % c
            P = dict(model, **dict(zip(tu.PORDER[:4], g[key + "_params"].tolist())))
            goals = g[key + "_goals"]
            res = bp.track_goals(goals, **P)
            co, ao = g[key + "_cand_off"], g[key + "_arr_off"]
            assert res.shape == (1, len(goals)) and np.array_equal(res.cand_offsets, co) and np.array_equal(res.arr_offsets, ao)
            assert np.array_equal(res.cand_node, g[key + "_cand"])
            assert np.array_equal(res.cand_find, g[key + "_find"]) and np.array_equal(res.cand_len, g[key + "_len"])
            assert np.array_equal(res.cand_fail, g[key + "_fail"]) and np.array_equal(res.cand_ood, g[key + "_ood"])
            assert np.array_equal(tu.bits(res.cand_t_last), tu.bits(g[key + "_tlast"]))
            assert np.array_equal(res.flag[0], g[key + "_flag"] != 0) and np.array_equal(res.winner[0], g[key + "_winner"])
            assert np.array_equal(res.len[0], g[key + "_wlen"]) and np.array_equal(res.n_cand[0], np.diff(co))
            assert np.array_equal(res.status[0] != 0, g[key + "_raises"] != 0)
            assert np.array_equal(res.status[0][g[key + "_raises"] != 0] & gt.ST_REF_RAISES, np.full(int(g[key + "_raises"].sum()), 32))
            assert res.partial == bool(g[key + "_raises"].any()) and not res.no_tree.any()
            node = [int(g[key + "_cand"][co[j] + w]) if w >= 0 else -1 for j, w in enumerate(g[key + "_winner"])]
            assert res.node[0].tolist() == node
            flat = np.stack([getattr(res, n) for n in res.ARRAYS])
            assert np.array_equal(tu.bits(flat), tu.bits(g[key + "_out"])), key
            for j in np.nonzero(res.flag[0])[0]:                                     # the candidates' last states: from the winners' arrays
                tr = res.trajectory(0, int(j))
                w = co[j] + res.winner[0, j]
                assert np.array_equal(tu.bits([tr[0][-2], tr[1][-2], tr[2][-2], tr[3][-1], tr[5][-1], tr[6][-1]]), tu.bits(g[key + "_last"][w]))
            for j in np.nonzero(~res.flag[0])[0]:
                assert res.trajectory(0, int(j)) is None and np.isinf(res.t_last[0, j])
    finally:
        bp.close()


# ---- 2. the planner's own goal against track() ----------------------------------------------------------------------------------
def snapshot(bp):
    n = len(bp.seeds)
    c = bp.courses()
    return dict(results=bp.results(), paths=[bp.path(i) for i in range(n)], rng=[bp.rng_state(i) for i in range(n)],
                trees=[bp.tree(i) for i in range(n)], courses=(c.offsets, c.x, c.y, c.yaw))


def assert_snapshots_equal(a, b):
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a["results"], b["results"]))
    assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a["paths"], b["paths"]))
    assert a["rng"] == b["rng"]
    assert all(np.array_equal(p, q) for s, t in zip(a["trees"], b["trees"]) for p, q in zip(s, t))
    assert all(np.array_equal(p, q) for p, q in zip(a["courses"], b["courses"]))


def track_answers(bp):
    n = len(bp.seeds)
    return [(bp.track_outcome(i), bp.track_records(i), bp.trajectory(i)) for i in range(n)]


def assert_own_goal(res, answers):
    for i, (o, (cand, rec), tr) in enumerate(answers):
        for k in FIELDS:
            assert int(getattr(res, k)[i, 0]) == int(o[k]), (i, k)
        c2, r2 = res.records(i, 0)
        assert np.array_equal(c2, cand) and r2.tobytes() == rec.tobytes(), i
        t2 = res.trajectory(i, 0)
        assert (t2 is None) == (tr is None), i
        if tr is not None:
            assert all(np.array_equal(tu.bits(p), tu.bits(q)) for p, q in zip(t2, tr)), i
            assert tu.bits([res.t_last[i, 0]])[0] == tu.bits([tr[4][-1]])[0]


@pytest.mark.parametrize("order", ["track_first", "goals_first"])
def test_own_goal_equals_track_in_both_call_orders_and_changes_nothing(order):
    _, kw, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s0.npz"))
    kw["max_iter"] = 120
    bp = planner(list(range(8)), kw)
    try:
        bp.plan()
        before = snapshot(bp)
        tk = {k: kw[k] for k in tu.PORDER[:4]}
        own = [kw["goal"]]
        if order == "track_first":
            flags = bp.track(**tk)
            first = track_answers(bp)
            res = bp.track_goals(own, **tk)
            assert_own_goal(res, first)
            again = track_answers(bp)                                                # the later call left track()'s answers alone
        else:
            res = bp.track_goals(own, **tk)
            flags = bp.track(**tk)
            again = track_answers(bp)
            assert_own_goal(res, again)
            res2 = bp.track_goals(own, **tk)                                         # and track() left these alone: asked again, the same
            assert res2.flag.tolist() == res.flag.tolist() and np.array_equal(tu.bits(res2.x), tu.bits(res.x))
            first = again
        assert res.flag[:, 0].tolist() == flags.tolist() and flags.any()
        for (o1, (c1, r1), t1), (o2, (c2, r2), t2) in zip(first, again):
            assert o1 == o2 and np.array_equal(c1, c2) and r1.tobytes() == r2.tobytes()
            assert (t1 is None) == (t2 is None) and (t1 is None or all(np.array_equal(tu.bits(p), tu.bits(q)) for p, q in zip(t1, t2)))
        assert res.best_goal().tolist() == np.where(flags, 0, -1).tolist()
        assert_snapshots_equal(before, snapshot(bp))
    finally:
        bp.close()


# ---- 3. a batch against the oracle ------------------------------------------------------------------------------------------------
DRIVER_OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
MAP_B = [(5, 5, 1), (4, 6, 1), (4, 8, 1), (4, 10, 1), (6, 5, 1), (7, 5, 1), (8, 6, 1), (8, 8, 1), (8, 10, 1)]
MAP_C = [(6, 3, 1.5), (10, 8, 2), (2, 9, 1.5), (12, 2, 1)]
GRID_TH = dict(xy_th=3.0, yaw_th=0.8)


def test_batch_with_own_starts_and_maps_equals_the_oracle(exe, tmp_path):
    import rrt_amd
    n = 8
    maps = [DRIVER_OBS] * n
    maps[2], maps[5] = MAP_B, MAP_C
    starts = [[0.25 * i, -0.2 * i, 0.05 * i] for i in range(n)]
    kw = dict(start=starts[0], goal=[6.0, 9.0, float(np.deg2rad(90.0))], obstacle_list=None, rand_area=[-2, 20], max_iter=100,
              connect_circle_dist=50.0, robot_radius=0.2)
    goals = np.array([[x, y, w] for x in np.linspace(0.0, 15.0, 10) for y in np.linspace(-1.0, 13.0, 10)
                      for w in (-2.4, -1.57, -0.8, 0.0, 0.8, 1.57)])
    assert goals.shape == (600, 3)
    bp = planner(list(range(31, 31 + n)), kw, starts=starts, instance_obstacles=maps)
    try:
        bp.plan()
        assert not bp.partial
        res = bp.track_goals(goals, **GRID_TH)
        A = rrt_amd._abi
        resident = 16 * 256
        assert res.shape == (n, 600) and n * 600 > resident and res.cand_offsets[-1] > resident    # both loops wrap
        assert res.flag.any() and not res.flag.all() and not res.no_tree.any()
        trees = [device_tree(bp, i) for i in range(n)]
        for i in range(n):                                                           # every query: the candidate lists
            for j in range(600):
                q = i * 600 + j
                want = gt.candidates(trees[i], goals[j], 3.0, 0.8)
                assert res.n_cand[i, j] == len(want) and res.cand_node[res.cand_offsets[q]:res.cand_offsets[q + 1]].tolist() == want, (i, j)
        P = dict(A.TRACK_DEFAULTS, **GRID_TH)
        sample = [(int(q) // 600, int(q) % 600) for q in np.random.default_rng(7).choice(n * 600, 600, replace=False)]
        want = gt.answer(exe, tmp_path, [(trees[i], starts[i], maps[i], 0.2, goals[j]) for i, j in sample], P)
        for (i, j), w in zip(sample, want):
            assert_query(res, i, j, w, "instance %d goal %d" % (i, j))
        seen = set(int(w["n_cand"]) for w in want)
        assert 0 in seen and max(seen) >= 10 and any(w["flag"] and w["winner"] > 0 for w in want)
        flagged = np.where(res.flag, res.t_last, np.inf)
        assert res.best_goal().tolist() == [int(np.argmin(r)) if np.isfinite(r).any() else -1 for r in flagged]
    finally:
        bp.close()


# ---- 4. shapes of the goal table ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_planners():
    _, kw, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s0.npz"))
    kw["max_iter"] = 100
    one, two = planner([3, 4, 5], kw), planner([3, 4, 5], kw, devices=[0, 0])
    one.plan()
    two.plan()
    yield one, two
    one.close()
    two.close()


def assert_same_result(a, b, arrays=True):
    for k in FIELDS + ("no_tree", "cand_offsets", "cand_node", "cand_find", "cand_len", "cand_fail", "cand_ood"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(tu.bits(a.t_last), tu.bits(b.t_last)) and np.array_equal(tu.bits(a.cand_t_last), tu.bits(b.cand_t_last))
    if arrays:
        assert np.array_equal(a.arr_offsets, b.arr_offsets)
        for name in a.ARRAYS:
            assert np.array_equal(tu.bits(getattr(a, name)), tu.bits(getattr(b, name))), name


@pytest.mark.parametrize("g", [1, 63, 64, 65])
def test_goal_counts_shared_and_per_instance_goals_sharding_and_records_only(shape_planners, g):
    import rrt_amd
    one, two = shape_planners
    goals = np.random.default_rng(g).uniform([-1.0, -1.0, -1.6], [14.0, 13.0, 1.6], (g, 3))
    goals[0] = [6.0, 8.0, 1.57]
    shared = one.track_goals(goals, **GRID_TH)
    assert shared.shape == (3, g) and len(shared.cand_offsets) == 3 * g + 1 == len(shared.arr_offsets)
    assert shared.arr_offsets[-1] == len(shared.x) == len(shared.d) == int((shared.len + 1)[shared.flag].sum()) and shared.flag.any()
    assert shared.kernel_ms[0] > 0.0 and shared.kernel_ms[1] > 0.0 and shared.kernel_ms[2] > 0.0
    assert_same_result(shared, one.track_goals(np.repeat(goals[None], 3, axis=0), **GRID_TH))
    assert_same_result(shared, two.track_goals(goals, **GRID_TH))                    # two handles, concatenated
    assert_same_result(shared, two.track_goals(np.repeat(goals[None], 3, axis=0), **GRID_TH))
    own_yaw = np.column_stack([goals[:, :2], np.full(g, one.handles[0].params.goal[2])])
    assert_same_result(one.track_goals(goals[:, :2], **GRID_TH), one.track_goals(own_yaw, **GRID_TH))   # a missing yaw: the planner's
    bare = one.track_goals(goals, arrays=False, **GRID_TH)
    assert_same_result(shared, bare, arrays=False)
    assert bare.arr_offsets is None and bare.x is None and bare.t is None and bare.kernel_ms[2] == 0.0
    with pytest.raises(ValueError, match="arrays=False"):
        bare.trajectory(0, 0)
    with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
        one.handles[0].get_goal_track_arrays(1)


# ---- 5. state ----------------------------------------------------------------------------------------------------------------
def test_refused_for_other_planners_and_before_plan():
    import rrt_amd
    A = rrt_amd._abi
    _, kw, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s0.npz"))
    goals = np.array([[6.0, 8.0, 1.57]])
    for algo in ("rrt", "rrt_star", "rrt_star_dubins", "rrt_star_reeds_shepp", "informed"):
        pose = algo.endswith(("dubins", "shepp"))
        bp = rrt_amd.BatchPlanner(algo, [1], [0.0, 0.0, 0.0] if pose else [0.0, 0.0], [6.0, 9.0, 1.5] if pose else [6.0, 9.0],
                                  DRIVER_OBS, [-2, 15], max_iter=30)
        try:
            bp.plan()
            with pytest.raises(ValueError, match="closed_loop_rrt_star"):
                bp.track_goals(goals)
            rc = A.load().rrtx_track_goals(bp.handles[0]._h, A.C.byref(A.TrackParams(**A.TRACK_DEFAULTS)), 1, 0, goals.ctypes.data, 1)
            assert rc == (0 if algo == "rrt_star_reeds_shepp" else -5), algo       # RRTX_ALGO_RS either cost, as rrtx_track_planned
        finally:
            bp.close()
    kw["max_iter"] = 40
    bp = planner([1, 2], kw)
    try:
        with pytest.raises(A.RrtxError, match="RRTX_E_STATE"):
            bp.track_goals(goals)                                                    # before plan()
        with pytest.raises(ValueError, match="'rrt_star', 'rrt_star_dubins', 'rrt_star_reeds_shepp'"):
            bp.query_goals(goals)                                                    # and query_goals goes on refusing rrt_10 trees
    finally:
        bp.close()


def test_a_replan_drops_the_answers_and_a_new_call_answers_for_the_new_trees(exe, tmp_path):
    import rrt_amd
    A = rrt_amd._abi
    _, kw, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s0.npz"))
    kw["max_iter"] = 100
    goals = np.array([[6.0, 8.0, 1.57], [2.0, 12.0, 0.0], [10.0, 4.0, 0.0]])
    bp = planner([5, 6], kw)
    try:
        bp.plan()
        first = bp.track_goals(goals, **GRID_TH)
        h = bp.handles[0]
        h.seed_instances([15, 16])
        bp.plan()                                                                    # other trees on the same handle
        for call in (h.get_goal_track, lambda: h.get_goal_track_records(1), lambda: h.get_goal_track_arrays(1), h.get_goal_track_kernel_ms):
            with pytest.raises(A.RrtxError, match="RRTX_E_STATE"):
                call()
        res = bp.track_goals(goals, **GRID_TH)
        assert not np.array_equal(res.cand_node, first.cand_node)
        P = dict(A.TRACK_DEFAULTS, **GRID_TH)
        trees = [device_tree(bp, i) for i in range(2)]
        want = gt.answer(exe, tmp_path, [(trees[i], kw["start"], kw["obstacle_list"], kw["robot_radius"], g) for i in range(2) for g in goals], P)
        for q, w in enumerate(want):
            assert_query(res, q // 3, q % 3, w, "query %d" % q)
    finally:
        bp.close()


def test_an_unfinished_instance_answers_no_tree_beside_answered_neighbours(exe, tmp_path, monkeypatch):
    """A polyline pool too small for the tree (RRTX_POOL_POINTS_PER_NODE) without the re-plan on a larger one (RRTX_NO_RETRY),
    the setup of test_gpu_goal_query's NO_TREE case carried to the pose planners: the instances on the driver map overflow, the
    two whose map leaves only a corner free stay small and finish."""
    import rrt_amd
    A = rrt_amd._abi
    monkeypatch.setenv("RRTX_POOL_POINTS_PER_NODE", "1")
    monkeypatch.setenv("RRTX_NO_RETRY", "1")
    corner = [(9.5, 9.5, 11.0)]
    maps = [DRIVER_OBS, corner, DRIVER_OBS, corner]
    kw = dict(start=[0.0, 0.0, 0.0], goal=[6.0, 9.0, 1.57], obstacle_list=None, rand_area=[-2, 20], max_iter=400,
              connect_circle_dist=50.0, robot_radius=0.0)
    bp = planner([1, 2, 3, 4], kw, instance_obstacles=maps)
    try:
        bp.plan()
        _, nn, st = bp.results()
        bad = (st & A.ST_FAILED) != 0
        assert bp.partial and bad[0] and bad[2] and not bad[1::2].all() and (nn[~bad] > 3).all()
        goals = np.array([[1.5, -1.5, 0.0], [-1.0, 1.0, 1.5], [6.0, 9.0, 1.57]])           # none takes the root for a candidate
        th = dict(xy_th=2.0, yaw_th=1.0)
        res = bp.track_goals(goals, **th)
        assert res.no_tree[bad].all() and not res.no_tree[~bad].any() and (res.status[bad] == 0).all()
        assert (res.n_cand[bad] == 0).all() and not res.flag[bad].any() and (res.node[bad] == -1).all() and np.isinf(res.t_last[bad]).all()
        P = dict(A.TRACK_DEFAULTS, **th)
        for i in np.nonzero(~bad)[0]:
            tree = device_tree(bp, int(i))
            want = gt.answer(exe, tmp_path, [(tree, kw["start"], maps[i], 0.0, g) for g in goals], P)
            assert any(w["n_cand"] > 0 for w in want)
            for j, w in enumerate(want):
                assert_query(res, int(i), j, w, "instance %d goal %d" % (i, j))
    finally:
        bp.close()


def test_a_goal_on_the_start_pose_is_ref_raises_for_that_query_only(exe, tmp_path):
    import rrt_amd
    A = rrt_amd._abi
    _, kw, _ = tu.load(os.path.join(tu.GOLD, "rrt10_drv_s0.npz"))
    kw["max_iter"] = 100
    goals = np.array([[6.0, 8.0, 1.57], kw["start"], [6.0, 9.0, 1.57]])
    bp = planner([3, 8], kw)
    try:
        bp.plan()
        h = bp.handles[0]
        rc, _ = h.track_goals(goals, False)
        assert rc == A.RRTX_PARTIAL and "refused candidate" in h.last_error()
        res = bp.track_goals(goals)
        assert res.partial and (res.status[:, 1] == A.ST_REF_RAISES).all() and (res.status[:, [0, 2]] == 0).all()
        assert not res.flag[:, 1].any() and (res.winner[:, 1] == -1).all() and res.flag[:, 2].any()
        for i in range(2):
            cand, rec = res.records(i, 1)
            assert cand[0] == 0 and rec["ood"][0] == A.OOD_RAISES and res.trajectory(i, 1) is None
            assert (rec["ood"][1:] == 0).all()                                      # the query's other records stay readable
        P = dict(A.TRACK_DEFAULTS)
        trees = [device_tree(bp, i) for i in range(2)]
        want = gt.answer(exe, tmp_path, [(trees[i], kw["start"], kw["obstacle_list"], kw["robot_radius"], g) for i in range(2) for g in goals], P)
        for q, w in enumerate(want):
            assert_query(res, q // 3, q % 3, w, "query %d" % q)
        assert h.track_goals(goals[[0, 2]], False)[0] == 0
    finally:
        bp.close()

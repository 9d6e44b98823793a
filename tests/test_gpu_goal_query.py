"""BatchPlanner.query_goals on the device: the best path to many goals from the planned trees (rrtx_query_goals).  The
yardsticks are the reference's own answers (tests/golden/goal_query_kat.npz, tools/gen_golden_goal_query.py), the planner's
own path(i) at its own goal, and the plain-Python rules of tests/goal_query_oracle.py run on tree(i).  Everything is
compared bit for bit: the queries select nodes and copy doubles; the one computed double, rrt_04's cost + distance, is
the reference's expression."""
import numpy as np
import pytest

import goal_query_oracle as gq
import util
from test_goal_query_host import POINT_CASES, POSE_CASES, bits, point_cfg, pose_cfg

pytestmark = pytest.mark.gpu
DRIVER_OBST = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]


@pytest.fixture(scope="module")
def golden():
    return util.load_golden(util.GOLDEN + "/goal_query_kat.npz")


def assert_result_equals(res, i, want, ncol, what=""):
    """Row i of a GoalQueryResult against packed oracle / golden arrays (node, cost, n_near, status, offsets, points and,
    when present, n_safe), the courses in res.order."""
    g = res.shape[1]
    for k in ("node", "n_near", "status") + (("n_safe",) if "n_safe" in want else ()):
        assert np.array_equal(getattr(res, k)[i], want[k]), (what, k)
    assert np.array_equal(bits(res.cost[i]), bits(want["cost"])), what
    assert np.array_equal(res.found[i], want["status"] == 0), what
    off = res.offsets[i * g:(i + 1) * g + 1]
    assert np.array_equal(off - off[0], want["offsets"]), what
    pts = want["points"] if res.order == "planning" else gq.reverse_courses(want["offsets"], want["points"])
    cols = [res.x, res.y] + ([res.yaw] if ncol == 3 else [])
    assert (res.yaw is None) == (ncol == 2), what
    got = np.column_stack([c[off[0]:off[-1]] for c in cols])
    assert got.shape == pts.shape and np.array_equal(bits(got), bits(pts)), what


def golden_rows(g, name, sfx=""):
    want = {k: g["%s_%s%s" % (name, k, sfx)] for k in ("node", "cost", "n_near", "status", "offsets", "points")}
    want["n_safe"] = g[name + "_n_safe"] if sfx == "" else np.zeros_like(want["node"])
    return want


# ---- 1. the reference's answers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POINT_CASES)
def test_rrt04_queries_equal_the_reference(golden, name):
    import rrt_amd
    g, c = golden, point_cfg(golden, name)
    bp = rrt_amd.BatchPlanner("rrt_star", [int(c["seed"]), int(c["seed"]) + 1], list(g[name + "_start"]), list(g[name + "_goal"]),
                              c["obstacles"], list(g[name + "_rand_area"]), expand_dis=c["expand_dis"],
                              path_resolution=c["path_resolution"], goal_sample_rate=int(c["goal_sample_rate"]),
                              max_iter=int(c["max_iter"]), play_area=c["play_area"], robot_radius=c["robot_radius"],
                              sobol_sampler=bool(c["sobol"]), connect_circle_dist=c["connect_circle_dist"],
                              search_until_max_iter=bool(c["until_max"]))
    try:
        bp.plan()
        assert len(bp.tree(0)[0]) == int(g[name + "_n_nodes"])
        want = golden_rows(g, name)
        for order in ("planning", "driving"):
            res = bp.query_goals(g[name + "_goals"], order=order)
            assert res.shape == (2, len(want["node"])) and res.order == order and res.kernel_ms > 0.0 and not res.partial
            assert_result_equals(res, 0, want, 2, name + " " + order)
        k = int(np.nonzero(want["status"] == 0)[0][0])
        a, b = want["offsets"][k], want["offsets"][k + 1]
        assert np.array_equal(res.course(0, k), want["points"][a:b][::-1])          # driving = the planning rows reversed
        assert res.course(0, len(want["node"]) - 1) is None                         # the inf goal
    finally:
        bp.close()


@pytest.mark.parametrize("name", POSE_CASES)
def test_pose_queries_equal_the_reference(golden, name):
    import rrt_amd
    g, c = golden, pose_cfg(golden, name)
    rs = name == "r0"
    kw = dict(expand_dis=c["expand_dis"], goal_sample_rate=int(c["goal_sample_rate"]), max_iter=int(c["max_iter"]),
              robot_radius=c["robot_radius"], connect_circle_dist=c["connect_circle_dist"], search_until_max_iter=True,
              curvature=c["curvature"], goal_yaw_th=c["goal_yaw_th"], goal_xy_th=c["goal_xy_th"])
    if rs:
        kw["step_size"] = c["step_size"]
    bp = rrt_amd.BatchPlanner("rrt_star_reeds_shepp" if rs else "rrt_star_dubins", [int(c["seed"])], list(g[name + "_start"]),
                              list(g[name + "_goal"]), c["obstacles"], list(g[name + "_rand_area"]), **kw)
    try:
        bp.plan()
        assert len(bp.tree(0)[0]) == int(g[name + "_n_nodes"])
        for t, (xy, yw) in enumerate(g[name + "_th"]):
            th = {} if t == 0 else dict(goal_xy_th=float(xy), goal_yaw_th=float(yw))      # t0: the planner's own
            for order in ("planning", "driving"):
                res = bp.query_goals(g[name + "_goals"], order=order, **th)
                assert_result_equals(res, 0, golden_rows(g, name, "_t%d" % t), 3 if rs else 2, "%s t%d %s" % (name, t, order))
    finally:
        bp.close()


# ---- 2. the planner's own goal ---------------------------------------------------------------------------------------------
def own_goal_planner(algo, until_max):
    import rrt_amd
    seeds = list(range(1, 7))
    if algo == "rrt_star":
        goals = [[6.0, 10.0], [6.0, 10.0], [9.0, 12.0], [3.0, 8.0], [0.0, 0.0], [14.0, 2.0]]   # [3]: inside an obstacle; [4]: the start
        return rrt_amd.BatchPlanner(algo, seeds, [0.0, 0.0], [6.0, 10.0], DRIVER_OBST, [-2, 15], expand_dis=3.0, path_resolution=0.5,
                                    goal_sample_rate=5, max_iter=250, robot_radius=0.8, search_until_max_iter=until_max,
                                    goals=goals), goals
    rs = algo == "rrt_star_reeds_shepp"
    seeds = [11, 13, 39, 12, 17, 20]                 # 13 and 39 reach the default goal under rrt_05, 11 and 13 under rrt_06
    goals = [[10.0, 9.0, 0.0]] * 3 + [[6.0, 12.0, 1.0], [3.0, 8.0, 0.0], [0.0, 0.0, 0.0]]
    kw = dict(step_size=0.1, curvature=2.0, robot_radius=0.6) if rs else dict(curvature=1.0)
    return rrt_amd.BatchPlanner(algo, seeds, [0.0, 0.0, 0.0], [10.0, 9.0, 0.0], DRIVER_OBST if rs else DRIVER_OBST[:6], [-2, 15],
                                expand_dis=3.0, goal_sample_rate=10, max_iter=200 if rs else 300, search_until_max_iter=until_max,
                                goals=goals, **kw), goals


@pytest.mark.parametrize("until_max", [True, False])
@pytest.mark.parametrize("algo", ["rrt_star", "rrt_star_dubins", "rrt_star_reeds_shepp"])
def test_query_at_the_own_goal_is_the_planned_path(algo, until_max):
    bp, own = own_goal_planner(algo, until_max)
    try:
        bp.plan()
        n = len(bp.seeds)
        goals = np.array(own, dtype=np.float64)[:, None, :]                         # (n, 1, 2 | 3): each instance's own goal
        res = bp.query_goals(goals)
        paths = [bp.path(i) for i in range(n)]
        assert res.found[:, 0].tolist() == [p is not None for p in paths] and any(p is not None for p in paths)
        for i, p in enumerate(paths):
            got = res.course(i, 0)
            assert (got is None) == (p is None)
            if p is not None:
                assert got.shape == p.shape and np.array_equal(bits(got), bits(p)), (algo, i)
        pc, _, _ = bp.results()
        if algo != "rrt_star":                       # the pose planners' path_cost is the answer node's cost
            assert np.array_equal(bits(res.cost[res.found[:, 0], 0]), bits(pc[res.found[:, 0]]))
    finally:
        bp.close()


# ---- 3. per-instance maps, starts and goals against the oracle module -------------------------------------------------------
def test_per_instance_everything_equals_the_oracle_module():
    import rrt_amd
    rng = np.random.default_rng(2024)
    n, g = 8, 300
    maps = [[(float(rng.uniform(1, 13)), float(rng.uniform(1, 13)), float(rng.uniform(0.5, 1.8))) for _ in range(3 + i)] for i in range(n)]
    starts = [[float(-1.0 + 0.25 * i), float(-1.5 + 0.1 * i)] for i in range(n)]
    goals = rng.uniform(-3.0, 16.0, (n, g, 2))
    goals[:, 0] = np.array(starts)                                                  # a goal on each instance's start
    bp = rrt_amd.BatchPlanner("rrt_star", list(range(11, 11 + n)), starts[0], [12.0, 12.0], None, [-2, 15], expand_dis=2.5,
                              path_resolution=0.4, goal_sample_rate=5, max_iter=160, robot_radius=0.3, search_until_max_iter=True,
                              play_area=[-2.5, 14.0, -2.5, 15.5], starts=starts, instance_obstacles=maps)
    try:
        bp.plan()
        assert not bp.partial
        res = bp.query_goals(goals)
        assert n * g > 4 * 256                       # more queries than workgroups the solve launch makes resident: the loop wraps
        assert res.found.any() and not res.found.all() and (res.node[:, 0] <= 0).all()   # the root or, where a circle covers it, none
        for i in range(n):
            tree = bp.tree(i)
            want = gq.pack([gq.query_rrt_star(tree, q, 2.5, 0.4, maps[i], 0.3, [-2.5, 14.0, -2.5, 15.5]) for q in goals[i]])
            assert_result_equals(res, i, want, 2, "instance %d" % i)
    finally:
        bp.close()


# ---- 4. shapes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_planners():
    import rrt_amd
    kw = dict(expand_dis=3.0, path_resolution=0.5, goal_sample_rate=5, max_iter=200, robot_radius=0.8, search_until_max_iter=True)
    one = rrt_amd.BatchPlanner("rrt_star", [3, 4, 5], [0.0, 0.0], [6.0, 10.0], DRIVER_OBST, [-2, 15], **kw)
    two = rrt_amd.BatchPlanner("rrt_star", [3, 4, 5], [0.0, 0.0], [6.0, 10.0], DRIVER_OBST, [-2, 15], devices=[0, 0], **kw)
    one.plan()
    two.plan()
    yield one, two
    one.close()
    two.close()


RECORDS = ("node", "cost", "n_near", "n_safe", "status", "found")


def assert_same_result(a, b, arrays=True):
    for k in RECORDS:
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
    if arrays:
        assert np.array_equal(a.offsets, b.offsets) and np.array_equal(bits(a.x), bits(b.x)) and np.array_equal(bits(a.y), bits(b.y))


@pytest.mark.parametrize("g", [1, 63, 64, 65])
def test_goal_counts_shared_and_per_instance_goals_sharding_and_records_only(shape_planners, g):
    one, two = shape_planners
    goals = np.random.default_rng(g).uniform(-2.0, 15.0, (g, 2))
    goals[0] = [1.0, 1.0]                                                           # beside the start: found
    shared = one.query_goals(goals)
    assert shared.shape == (3, g) and len(shared.offsets) == 3 * g + 1 and shared.offsets[-1] == len(shared.x) == len(shared.y)
    assert shared.found.any()
    assert_same_result(shared, one.query_goals(np.repeat(goals[None], 3, axis=0)))
    assert_same_result(shared, two.query_goals(goals))                              # two handles, concatenated
    assert_same_result(shared, two.query_goals(np.repeat(goals[None], 3, axis=0)))
    bare = one.query_goals(goals, paths=False)
    assert_same_result(shared, bare, arrays=False)
    assert bare.offsets is None and bare.x is None and bare.y is None and bare.yaw is None
    for i in range(3):                                                              # and row i is the oracle's on tree(i)
        want = gq.pack([gq.query_rrt_star(one.tree(i), q, 3.0, 0.5, DRIVER_OBST, 0.8) for q in goals])
        assert_result_equals(shared, i, want, 2, "g=%d instance %d" % (g, i))


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------------
def test_more_candidates_than_the_kernel_holds_is_overflow_never_a_wrong_node():
    """a query keeps its distinct candidates in LDS (512); one with more is answered GOALQ_OVERFLOW, the call
    is partial, and every other query of the call is answered exactly -- the one just under the capacity included."""
    import rrt_amd
    A = rrt_amd._abi
    obst = [(3.6, 0.4, 0.2)]
    # the planner's own goal lies far outside: its own goal search stays small; the small connect_circle_dist keeps the near sets small
    bp = rrt_amd.BatchPlanner("rrt_star", [5], [2.0, 2.0], [30.0, 30.0], obst, [0.0, 4.0], expand_dis=3.0, path_resolution=0.5,
                              goal_sample_rate=0, max_iter=1500, connect_circle_dist=1.0, search_until_max_iter=True)
    try:
        bp.plan()
        assert bp.failed() == []
        tree = bp.tree(0)
        x, y = tree[0], tree[1]
        assert len(x) > 1200

        def distinct(goal):
            return len(set(gq.point_candidates(x, y, goal, 3.0)[0]))
        assert distinct((2.0, 2.0)) > A.GOALQ_MAX_CANDIDATES                        # checked here, on the CPU
        ts = np.linspace(-2.0, 2.0, 161)
        counts = [distinct((t, t)) for t in ts]
        under = max((c, k) for k, c in enumerate(counts) if c <= A.GOALQ_MAX_CANDIDATES)
        assert A.GOALQ_MAX_CANDIDATES - 40 <= under[0]                              # just under the capacity
        goals = np.array([[2.0, 2.0], [ts[under[1]]] * 2, [-1.0, -1.0], [ts[under[1] + 1]] * 2])
        res = bp.query_goals(goals)
        want = [gq.query_rrt_star(tree, q, 3.0, 0.5, obst, 0.0) for q in goals]
        over = [w["n_near"] > A.GOALQ_MAX_CANDIDATES for w in want]
        assert over == [True, False, False, True] and want[1]["n_near"] == under[0] and want[1]["status"] == 0
        assert res.partial and res.status[0].tolist() == [A.GOALQ_OVERFLOW, A.GOALQ_OK, want[2]["status"], A.GOALQ_OVERFLOW]
        assert res.node[0, 0] == res.node[0, 3] == -1 and res.course(0, 0) is None and np.isinf(res.cost[0, 0])
        for k in (1, 2):
            assert (res.node[0, k], res.n_near[0, k], res.n_safe[0, k]) == (want[k]["node"], want[k]["n_near"], want[k]["n_safe"])
            assert res.cost[0, k] == want[k]["cost"]
            assert (want[k]["course"] is None and res.course(0, k) is None) or np.array_equal(res.course(0, k), want[k]["course"])
        assert bp.handles[0].query_goals(np.array([[2.0, 2.0, 0.0]]), False)[0] == A.RRTX_PARTIAL
        assert "RRTX_GOALQ_OVERFLOW" in bp.handles[0].last_error()
        assert bp.handles[0].query_goals(np.array([[-1.0, -1.0, 0.0]]), False)[0] == 0
    finally:
        bp.close()


# ---- 6. state -------------------------------------------------------------------------------------------------------------------
def snapshot(bp):
    n = len(bp.seeds)
    c = bp.courses()
    return dict(results=bp.results(), paths=[bp.path(i) for i in range(n)], rng=[bp.rng_state(i) for i in range(n)],
                trees=[bp.tree(i) for i in range(n)], courses=(c.offsets, c.x, c.y))


def assert_snapshots_equal(a, b):
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a["results"], b["results"]))
    assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a["paths"], b["paths"]))
    assert a["rng"] == b["rng"]
    assert all(np.array_equal(p, q) for s, t in zip(a["trees"], b["trees"]) for p, q in zip(s, t))
    assert all(np.array_equal(p, q) for p, q in zip(a["courses"], b["courses"]))


def test_a_query_changes_nothing_of_the_plan_and_follows_the_call_order():
    import rrt_amd
    bp, _ = own_goal_planner("rrt_star", True)
    try:
        with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
            bp.query_goals([[1.0, 1.0]])                                            # before plan()
        bp.plan()
        before = snapshot(bp)
        held = bp.courses()                                                         # a PlannerCourses gathered before the queries
        a = bp.query_goals([[1.0, 1.0], [6.0, 10.0], [12.0, 12.0]])
        b = bp.query_goals([[9.0, 12.0]], order="driving")                          # a second query, other goals
        assert a.shape == (6, 3) and b.shape == (6, 1) and a.found.any() and b.found.any()
        assert_snapshots_equal(before, snapshot(bp))
        again = bp.courses()
        assert np.array_equal(held.offsets, again.offsets) and np.array_equal(held.x, again.x)
        a2 = bp.query_goals([[1.0, 1.0], [6.0, 10.0], [12.0, 12.0]])
        assert_same_result(a, a2)
        h = bp.handles[0]
        h.query_goals(np.array([[1.0, 1.0, 0.0]]), False)
        bp.plan()                                                                   # the answers belonged to the previous plan
        with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_INVALID"):
            h.gather_goal_courses()
        with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_STATE"):
            h.get_goal_query(1)
        assert_same_result(a, bp.query_goals([[1.0, 1.0], [6.0, 10.0], [12.0, 12.0]]))   # the same plan again: the same answers
    finally:
        bp.close()


def test_an_overflowed_instance_has_no_tree_and_its_neighbours_are_answered(monkeypatch):
    """The small-capacity setup of test_gpu_parity: the 64-thread shape without the re-plan on a larger shape."""
    import rrt_amd
    A = rrt_amd._abi
    monkeypatch.setenv("RRTX_TPB", "64")
    monkeypatch.setenv("RRTX_NO_RETRY", "1")
    seeds = list(range(1, 9))
    starts = [[0.0, 0.0]] * 7 + [[5.0, 5.0]]                                        # the last start lies inside an obstacle
    bp = rrt_amd.BatchPlanner("rrt_star", seeds, [0.0, 0.0], [6.0, 10.0], DRIVER_OBST, [-2, 15], expand_dis=3.0, path_resolution=0.5,
                              goal_sample_rate=5, max_iter=700, robot_radius=0.8, search_until_max_iter=True, starts=starts)
    try:
        bp.plan()
        _, nn, st = bp.results()
        bad = (st & A.ST_FAILED) != 0
        assert bp.partial and bad.any() and not bad.all() and not bad[7] and nn[7] == 1
        goals = np.array([[5.5, 3.0], [1.0, 1.0], [6.0, 10.0]])
        res = bp.query_goals(goals)
        assert (res.status[bad] == A.GOALQ_NO_TREE).all() and (res.node[bad] == -1).all() and not res.found[bad].any()
        assert not res.partial
        for i in np.nonzero(~bad)[0]:
            want = gq.pack([gq.query_rrt_star(bp.tree(int(i)), q, 3.0, 0.5, DRIVER_OBST, 0.8) for q in goals])
            assert_result_equals(res, int(i), want, 2, "instance %d" % i)
    finally:
        bp.close()


def test_other_planners_are_refused():
    import rrt_amd
    bp = rrt_amd.BatchPlanner("rrt", [1, 2], [0.0, 0.0], [6.0, 10.0], DRIVER_OBST, [-2, 15], max_iter=50)
    cl = rrt_amd.BatchPlanner("closed_loop_rrt_star", [1], [0.0, 0.0, 0.0], [6.0, 7.0, 1.5], DRIVER_OBST, [-2, 20], max_iter=20)
    try:
        bp.plan()
        cl.plan()
        for p in (bp, cl):
            with pytest.raises(ValueError, match="'rrt_star', 'rrt_star_dubins', 'rrt_star_reeds_shepp'"):
                p.query_goals([[1.0, 1.0]])
        with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_E_INVALID"):
            cl.handles[0].query_goals(np.zeros((1, 3)), False)                      # the C ABI refuses rrt_10's tree too
    finally:
        bp.close()
        cl.close()

"""Batched arm navigation on the device (BatchArmNav, rrt_amd.arm_obstacle_navigation): the kernels of csrc/armnav_batch.hip.h
against the reference's recorded integers (tests/golden/armnav_kat.npz) and against the oracle (tests/armnav_oracle.py).  The
shapes are the smallest at which the kernels can go wrong: M = 2 and 3 (the wrap neighbours coincide), 64 and 65 (the row minima
at the wave's edge), 128 (the LDS limit), batches of 1, 63, 64 and 65 queries that point at different grids."""
import numpy as np
import pytest

import armnav_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nav(gpu):
    import rrt_amd
    with rrt_amd.BatchArmNav(M=100) as n:
        yield n


def grids_of(M):
    """(scene numbers, their golden grids stacked) of one M"""
    ss = U.scenes_of(M)
    return ss, np.stack([U.scene_grid(s) for s in ss])


def assert_queries(res, qs, what):
    """A result against the golden queries it answers: status, route, cells closed, and the marked grid -- the reference's where
    the file holds it, the oracle's everywhere"""
    assert len(res) == len(qs), what
    assert np.array_equal(res.offsets, np.concatenate([[0], np.cumsum(res.n_route)])), what
    for k, q in enumerate(qs):
        c = U.query(q)
        w = (what, k, q, c["tag"])
        assert res.route(k) == c["route"] and int(res.n_route[k]) == len(c["route"]), w
        assert int(res.status[k]) == (0 if c["route"] else 1) and bool(res.found[k]) == bool(c["route"]), w
        assert int(res.pops[k]) == c["pops"], w
        if res.marks is not None:
            assert np.array_equal(res.marks[k], U.oracle_query(q)[1]), w
            if c["marks"] is not None:
                assert np.array_equal(res.marks[k], c["marks"]), w


def plan_golden(nav, M, qs, marks=True, set_grids=True):
    ss, grids = grids_of(M)
    nav.M = M
    starts = [U.query(q)["start"] for q in qs]
    goals = [U.query(q)["goal"] for q in qs]
    scene = [ss.index(U.query(q)["scene"]) for q in qs]
    return nav.plan(starts, goals, scene=scene, grids=grids if set_grids else None, marks=marks)


@pytest.mark.parametrize("M", U.all_M())
def test_grids_equal_the_goldens(nav, M):
    """Every arm scene of one M in one call: scenes of different link and circle counts side by side"""
    ss = U.scenes_of(M, 0)
    nav.M = M
    got = nav.occupancy([U.scene_arm(s)[0] for s in ss], [U.scene_arm(s)[1] for s in ss])
    assert got.shape == (len(ss), M, M) and got.dtype == np.uint8
    for k, s in enumerate(ss):
        assert np.array_equal(got[k], U.scene_grid(s)), "scene %d: %d cells differ" % (s, int(np.sum(got[k] != U.scene_grid(s))))
    if len(ss) == 1:   # one arm for every scene: the flat form of link_lengths
        again = nav.occupancy(U.scene_arm(ss[0])[0], [U.scene_arm(ss[0])[1]] * 3)
        assert again.shape == (3, M, M) and all(np.array_equal(again[k], U.scene_grid(ss[0])) for k in range(3))


@pytest.mark.parametrize("M", U.all_M())
def test_all_golden_queries(nav, M):
    qs = U.queries_of(M)
    assert len({U.query(q)["scene"] for q in qs}) > 1 or M == 100
    assert_queries(plan_golden(nav, M, qs), qs, "M %d" % M)


@pytest.mark.parametrize("n", (1, 63, 64, 65))
@pytest.mark.parametrize("M", (2, 3, 64, 65, 128))
def test_batch_sizes(nav, M, n):
    qs = U.cycled(M, n, shift=n)
    assert_queries(plan_golden(nav, M, qs), qs, "M %d, %d queries" % (M, n))


@pytest.mark.parametrize("tag", ("walled", "same", "goal_on_obstacle", "start_on_obstacle"))
def test_named_queries(nav, tag):
    n_all = len(U.kat()["q_scene"])
    for M in (5, 33, 100):
        qs = [q for q in U.queries_of(M) if U.query(q)["tag"] == tag]
        assert qs or (tag == "walled" and M == 100), (M, tag)
        if not qs:
            continue
        res = plan_golden(nav, M, qs)
        assert_queries(res, qs, "%s at M %d" % (tag, M))
        for k, q in enumerate(qs):
            c = U.query(q)
            if tag == "walled":
                assert res.route(k) == [] and res.status[k] == 1 and not res.found[k] and res.marks[k][c["goal"]] == 5
            elif tag == "same":
                assert res.route(k) == [c["goal"]] and res.pops[k] == 0 and res.marks[k][c["goal"]] == 5
                assert np.array_equal(np.delete(res.marks[k].reshape(-1), c["goal"][0] * M + c["goal"][1]),
                                      np.delete(U.scene_grid(c["scene"]).reshape(-1), c["goal"][0] * M + c["goal"][1]))
            elif tag == "goal_on_obstacle":
                assert U.scene_grid(c["scene"])[c["goal"]] == 1 and (not res.found[k] or res.marks[k][c["goal"]] == 6)
            else:
                assert U.scene_grid(c["scene"])[c["start"]] == 1 and res.marks[k][c["start"]] == 4
    assert n_all > 300


def test_kept_grids_equal_grids_given_as_data_and_marked_grids_are_searched(nav):
    M = 17
    ss = U.scenes_of(M, 0)
    qs = [q for q in U.queries_of(M) if U.query(q)["scene"] in ss]
    nav.M = M
    nav.occupancy([U.scene_arm(s)[0] for s in ss], [U.scene_arm(s)[1] for s in ss])
    starts, goals = [U.query(q)["start"] for q in qs], [U.query(q)["goal"] for q in qs]
    scene = [ss.index(U.query(q)["scene"]) for q in qs]
    kept = nav.plan(starts, goals, scene=scene)                                               # the grids occupancy() left
    assert_queries(kept, qs, "kept grids")
    given = nav.plan(starts, goals, scene=scene, grids=np.stack([U.scene_grid(s) for s in ss]))
    for key in ("status", "n_route", "pops", "offsets", "cells", "marks"):
        assert np.array_equal(getattr(kept, key), getattr(given, key)), key
    # one-to-one: as many grids as queries and no scene list; the grids are earlier results, marks 2..6 and all
    with_route = [k for k in range(len(qs)) if kept.found[k] and kept.pops[k] > 2]
    walled = [q for q in U.queries_of(M) if U.query(q)["tag"] == "walled"][:1]
    marked = [kept.marks[k] for k in with_route[:4]] + [U.oracle_query(q)[1] for q in walled]
    assert {v for m in marked for v in np.unique(m).tolist()} == {0, 1, 2, 3, 4, 5, 6}
    st = [starts[with_route[(k + 1) % len(with_route)]] for k in range(len(marked))]
    go = [goals[with_route[(k + 2) % len(with_route)]] for k in range(len(marked))]
    res = nav.plan(st, go, grids=np.stack(marked))
    for k in range(len(marked)):
        route, marks, pops = U.oracle_search(marked[k], st[k], go[k])
        assert res.route(k) == route and int(res.pops[k]) == pops and np.array_equal(res.marks[k], marks), k
    # a single grid, two-dimensional, and no scene list: every query searches it
    one = nav.plan(st, go, grids=marked[0])
    for k in range(len(st)):
        route, marks, pops = U.oracle_search(marked[0], st[k], go[k])
        assert one.route(k) == route and np.array_equal(one.marks[k], marks), k


def test_one_object_reused(gpu):
    """M = 100 then M = 5; a large batch then a small one; marks=False then True: every call serves what it wrote itself"""
    import rrt_amd
    with rrt_amd.BatchArmNav(M=100) as nav:
        big = U.cycled(100, 130)
        res = plan_golden(nav, 100, big, marks=False)
        assert res.marks is None
        assert_queries(res, big, "M 100, 130 queries, no marks")
        with pytest.raises(rrt_amd._abi.RrtxError):
            nav._nav.marks(len(big), 100)                                                     # RRTX_E_STATE after marks=False
        small = U.queries_of(5)[:3]
        assert_queries(plan_golden(nav, 5, small), small, "M 5 after M 100")
        again = U.cycled(100, 2, shift=1)
        assert_queries(plan_golden(nav, 100, again), again, "M 100, 2 queries, marks")
        nav.M = 5
        ss = U.scenes_of(5, 0)
        got = nav.occupancy([U.scene_arm(s)[0] for s in ss], [U.scene_arm(s)[1] for s in ss])  # a smaller grid call after larger ones
        assert all(np.array_equal(got[k], U.scene_grid(s)) for k, s in enumerate(ss))
        none = nav.plan(np.zeros((0, 2)), np.zeros((0, 2)), scene=[])
        assert len(none) == 0 and none.offsets.tolist() == [0] and none.marks.shape == (0, 5, 5)
        with pytest.raises(rrt_amd._abi.RrtxError):
            nav.plan([[0, -1]], [[1, 1]], scene=[0])                                                     # numpy would wrap; refused


def test_seeded_sweep_on_the_driver_grid(nav):
    """2 000 random queries on the driver grid against the oracle, in one call"""
    rs = np.random.RandomState(20021)
    n = 2000
    grid = U.scene_grid(0)
    starts, goals = rs.randint(0, 100, (n, 2)), rs.randint(0, 100, (n, 2))
    res = nav.plan(starts, goals, grids=grid)
    assert res.marks.shape == (n, 100, 100)
    found = 0
    for k in range(n):
        route, marks, pops = U.oracle_search(grid, tuple(starts[k]), tuple(goals[k]))
        assert res.route(k) == route and int(res.pops[k]) == pops, (k, starts[k], goals[k])
        assert np.array_equal(res.marks[k], marks), (k, starts[k], goals[k])
        found += bool(route)
    assert 100 < found < n and int(res.found.sum()) == found


def test_route_pool_second_pass(gpu):
    """A fresh object whose first batch asks for more route cells than its first route pool holds (4 M per query): a corridor
    that winds through the whole grid.  The batch runs a second time with the pool it asked for; nothing is cut short."""
    import rrt_amd
    M = 16
    grid = np.zeros((M, M), dtype=np.uint8)
    grid[1::2, :] = 1                      # walls on the odd rows ...
    for r in range(1, M, 2):
        grid[r, (M - 2) if (r // 2) % 2 == 0 else 1] = 0   # ... with one gap each, at alternating ends
    grid[M - 1, :] = 1                     # and no way round over the edge
    grid[:, 0], grid[:, M - 1] = 1, 1
    start, goal = (0, 1), (M - 2, 1)
    route, marks, pops = U.oracle_search(grid, start, goal)
    assert len(route) > 4 * M
    with rrt_amd.BatchArmNav(M=M) as nav:
        res = nav.plan([start] * 5, [goal] * 5, grids=grid)
        for k in range(5):
            assert res.route(k) == route and int(res.pops[k]) == pops and np.array_equal(res.marks[k], marks)


def test_dropin_module_on_the_driver_run(gpu, capsys):
    import rrt_amd.arm_obstacle_navigation as an
    arm = an.NLinkArm(U.DRIVER_LINKS, [0.0] * 5)
    grid = an.get_occupancy_grid(arm, U.DRIVER_OBSTACLES, 100)
    assert grid.dtype == np.int64 and np.array_equal(grid, U.scene_grid(0))
    q = [q for q in U.queries_of(100) if U.query(q)["tag"] == "driver"][0]
    route = an.astar_torus(grid, *U.DRIVER_QUERY)
    assert route == U.query(q)["route"] and len(route) == 347 and isinstance(route[0], tuple)
    assert np.array_equal(grid, U.query(q)["marks"])                                          # marked in place
    assert "The route found covers 347 grid cells." in capsys.readouterr().out
    walled = [q for q in U.queries_of(33) if U.query(q)["tag"] == "walled"][0]
    c = U.query(walled)
    g = U.scene_grid(c["scene"]).astype(np.int64)
    assert an.astar_torus(g, c["start"], c["goal"]) == [] and np.array_equal(g, c["marks"])
    assert "No route found." in capsys.readouterr().out

"""GPU (-m gpu): the obstacle map under the Reeds-Shepp planners -- "rrt_star_reeds_shepp" (rrt_06) and "closed_loop_rrt_star"
(rrt_10) plan, track and track_goals among any number of circles up to 2**20.  Trees against the oracle and against goldens
made by the reference classes on 300 circles, bit for bit; the same answers as the 64-circle tile where both apply, whatever
the cell count, with a wide circle, with circles and arcs outside the sampling square, with edges of more than 64 points; the
launch paths (pool re-plan, bounded steps, shards, a reused handle); the closed-loop stage and track_goals on the map against
the tile, the goldens and the CPU restatement; what stays refused."""
import glob
import math
import os
import random

import numpy as np
import pytest

import goal_track_oracle as gt
import obsmap_util as OM
import rs_obsmap_util as R
import track_util as tu
import util

pytestmark = pytest.mark.gpu

WIDE = (3.0, 14.0, 3.0)            # 6 x 6 cells of the 18 x 18 grid over [-2, 20]^2: more than 32, so it goes to the wide list
FIELDS = ("flag", "winner", "n_cand", "len", "node", "status")


# ---- G1. tree parity on the four scenes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", sorted(R.SCENES))
def test_gpu_trees_equal_the_oracle(gpu, m):
    import rrt_amd
    kw = R.problem(m)
    bp = rrt_amd.BatchPlanner("rrt_star_reeds_shepp", R.SEEDS, kw["start"], kw["goal"], kw["obstacles"], kw["rand_area"],
                              expand_dis=kw["expand_dis"], max_iter=kw["max_iter"], robot_radius=kw["robot_radius"],
                              connect_circle_dist=kw["connect_circle_dist"], search_until_max_iter=True, curvature=1.0,
                              step_size=0.2)
    try:
        assert bp.has_obstacle_map                                        # more than 64 circles: the keyword's default
        bp.plan()
        out = R.read(bp.h, len(R.SEEDS))
        assert R.equals_oracle(kw, R.SEEDS, out, "m = %d" % m) == R.NODES[m]
        for i, s in enumerate(R.SEEDS):
            r = R.oracle(kw, s)
            p = bp.path(i)
            assert (p is None) == (r["path"] is None)
            if p is not None:
                assert np.array_equal(p, np.column_stack([r["path"], r["path_yaw"]]))
        info = OM.assert_map_equals(bp.h, kw["rand_area"], kw["obstacles"], kw["robot_radius"])
        assert info["n_circles"] == m
    finally:
        bp.close()


# ---- G2. the reference's goldens ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["class", "module"])
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(util.GOLDEN, "obsmap_rs_m300_s*.npz"))),
                         ids=lambda p: os.path.basename(p)[:-4])
def test_gpu_reeds_shepp_goldens_bit_for_bit(gpu, path, entry):
    import rrt_amd
    import rrt_amd.rrt_06
    g = util.load_golden(path)
    cls = rrt_amd.RRTStarReedsShepp if entry == "class" else rrt_amd.rrt_06.RRT
    random.seed(int(g["seed"]))
    p = cls(start=list(g["start"]), goal=list(g["goal"]), obstacle_list=[tuple(o) for o in g["obstacles"]],
            rand_area=list(g["rand_area"]), expand_dis=3.0, path_resolution=0.5, goal_sample_rate=10, max_iter=int(g["max_iter"]),
            play_area=None, robot_radius=float(g["robot_radius"]), sobol_sampler=True, connect_circle_dist=50.0,
            search_until_max_iter=False, curvature=1.0, goal_yaw_th=float(np.deg2rad(1.0)), goal_xy_th=0.5, step_size=0.2)
    assert len(p.obstacle_list) == 300 and p.obstacle_map is None
    path3 = p.planning(animation=False)
    util.assert_tree_equal(p.tree, (g["x"], g["y"], g["cost"], g["parent"]), g["name"])
    assert np.array_equal(R.bits(p.yaw), R.bits(g["yaw"]))
    plen, px, py = p.polylines
    assert np.array_equal(plen, g["poly_len"]) and np.array_equal(R.bits(px), R.bits(g["poly_x"]))
    assert np.array_equal(R.bits(py), R.bits(g["poly_y"]))
    assert (path3 is not None) == bool(g["path_found"])
    if path3 is not None:
        assert np.array_equal(R.bits(np.array(path3)), R.bits(g["path"]))
    st = random.getstate()
    assert st[1][624] == int(g["rng_pos_after"]) and st[1][0] == int(g["rng_word0_after"])
    p.obstacle_map = False
    with pytest.raises(rrt_amd._abi.RrtxError, match="more than 256 obstacles"):     # 300 circles: the general limit comes first
        p.planning(animation=False)
    p.obstacle_list = p.obstacle_list[:65]
    with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_ALGO_RS: more than 64 obstacles"):
        p.planning(animation=False)


# ---- G3. map = tile -----------------------------------------------------------------------------------------------------------
def test_gpu_map_equals_tile_at_64(gpu):
    kw = R.problem(65)
    kw["obstacles"] = kw["obstacles"][:64]
    on_map, on_tile = R.plan(kw, R.SEEDS), R.plan(kw, R.SEEDS, use_map=False)
    R.same(on_tile, on_map, "64 circles, tile against map")
    R.equals_oracle(kw, R.SEEDS, on_map, "64 circles")
    for k in ("rewires", "near_hits", "iterations"):
        assert on_map["stats"][k] == on_tile["stats"][k], k


# ---- G4. the cell knob and the wide list --------------------------------------------------------------------------------------
def test_gpu_cell_knob_changes_nothing(gpu, monkeypatch):
    kw = R.problem(300)
    default = R.plan(kw, R.SEEDS)
    assert default["info"]["nx"] == 18
    for cells in ("1", "7"):
        monkeypatch.setenv("RRTX_OBSMAP_CELLS", cells)
        got = R.plan(kw, R.SEEDS)
        monkeypatch.delenv("RRTX_OBSMAP_CELLS")
        assert got["info"]["nx"] == got["info"]["ny"] == int(cells)
        R.same(got, default, "RRTX_OBSMAP_CELLS=" + cells)


@pytest.mark.parametrize("at", [0, 300])
def test_gpu_wide_circle_equals_oracle(gpu, at):
    kw = R.problem(300)
    seeds = [1, 2, 3]
    lst = list(kw["obstacles"])
    lst.insert(at, WIDE)
    wide = dict(kw, obstacles=lst)
    for s in seeds:
        assert R.differs(R.oracle(wide, s), R.oracle(kw, s)), s              # the wide circle rejected an edge of this plan
    out = R.plan(wide, seeds)
    assert out["info"]["n_wide"] == 1 and out["info"]["n_circles"] == 301
    R.equals_oracle(wide, seeds, out, "wide circle at list index %d" % at)


# ---- G5. circles and arcs outside the sampling square -------------------------------------------------------------------------
def outside_scene():
    rng = random.Random(5)
    inside, outside = [], []

    def free(x, y, r, d):
        return all(math.hypot(x - px, y - py) > r + d for px, py in ((0.5, 5.0), (8.0, 5.0)))
    while len(inside) < 50:
        x, y, r = rng.uniform(0, 10), rng.uniform(0, 10), rng.uniform(0.05, 0.15)
        if free(x, y, r, 1.0):
            inside.append((x, y, r))
    while len(outside) < 20:
        k = len(outside)
        if k < 10:
            x, y = rng.uniform(-3, -0.3), rng.uniform(0, 10)
        elif k < 15:
            x, y = rng.uniform(0, 10), rng.uniform(10.2, 12)
        else:
            x, y = rng.uniform(0, 10), rng.uniform(-2, -0.2)
        r = rng.uniform(0.2, 0.4)
        if free(x, y, r, 0.6):
            outside.append((x, y, r))
    return inside, outside


def test_gpu_circles_outside_the_square_equal_oracle(gpu):
    inside, outside = outside_scene()
    assert len(inside + outside) == 70 and sum(c[0] < 0 for c in outside) == 10 and sum(not 0 <= c[1] <= 10 for c in outside) == 10
    kw = R.problem(0, start=[0.5, 5.0, math.pi], goal=[8.0, 5.0, 0.0], rand_area=[0, 10], robot_radius=0.05)
    full, cut = dict(kw, obstacles=inside + outside), dict(kw, obstacles=inside)
    seeds = [1, 2, 3, 5]
    for s in seeds:
        assert R.differs(R.oracle(full, s), R.oracle(cut, s)), s             # an outside circle rejected an edge
    r = R.oracle(full, 2)
    assert r["poly_x"].min() < 0.0                                           # and accepted arcs leave the square
    out = R.plan(full, seeds)
    R.equals_oracle(full, seeds, out, "outside the square")
    assert (out["info"]["x0"], out["info"]["y0"]) == (0.0, 0.0) and out["info"]["nx"] == 9


# ---- G6. edges of more than 64 points -----------------------------------------------------------------------------------------
def test_gpu_edges_of_more_than_64_points_equal_oracle(gpu):
    kw = R.problem(300, step_size=0.05)
    seeds = [0, 1, 3]
    for s in seeds:
        r = R.oracle(kw, s)
        assert r["poly_len"].max() > 64                                      # an accepted edge: a lane handles several points
        assert R.differs(r, R.oracle(R.problem(0, step_size=0.05), s)), s
    R.equals_oracle(kw, seeds, R.plan(kw, seeds), "step_size 0.05")


# ---- G7. handle life and launch paths -----------------------------------------------------------------------------------------
def test_gpu_pool_regrowth_with_a_map(gpu, monkeypatch):
    # the smallest pool holds 1 point per node slot (2 * max_iter + 2 of them) + 8192: at step_size 0.01 the kept polylines
    # of seeds 3, 4 and 7 alone are longer, those of seed 2 are not
    kw = R.problem(300, step_size=0.01)
    seeds = [2, 3, 4, 7]
    small = 1 * (2 * kw["max_iter"] + 2) + 8192
    assert [int(R.oracle(kw, s)["poly_len"].sum()) > small for s in seeds] == [False, True, True, True]
    want = R.plan(kw, seeds)
    assert want["stats"]["replanned"] == 0
    monkeypatch.setenv("RRTX_POOL_POINTS_PER_NODE", "1")
    got = R.plan(kw, seeds)
    assert got["stats"]["replanned"] > 0                                     # the re-plan on the larger pool ran the map kernel too
    R.same(got, want, "pool regrowth")
    R.equals_oracle(kw, seeds, got, "pool regrowth")


def test_gpu_bounded_steps_and_a_setter_mid_plan(gpu):
    kw = R.problem(300)
    one_shot = R.plan(kw, R.SEEDS)
    h = R.make_handle(kw, len(R.SEEDS))
    try:
        h.set_obstacle_map(kw["obstacles"])
        h.seed_instances(R.SEEDS)
        h.set_launch_bound(40)
        h.plan_begin()
        assert h.L.rrtx_set_obstacle_map(h._h, None, 0) == -5 and "in progress" in h.last_error()   # RRTX_E_STATE; the plan goes on
        one = np.array([[1.0, 2.0, 0.5]])
        assert h.L.rrtx_set_obstacles(h._h, one.ctypes.data, 1) == -5
        steps = 0
        while True:
            rc, pending = h.plan_step()
            steps += 1
            if pending == 0:
                break
        assert steps >= 3
        R.same(R.read(h, len(R.SEEDS)), one_shot, "bounded steps")
    finally:
        h.close()


def test_gpu_map_larger_map_tile_and_map_again_on_one_handle(gpu):
    import rrt_amd
    lists = {"a": R.problem(300)["obstacles"], "b": R.problem(1000)["obstacles"], "t": R.problem(65)["obstacles"][:64]}
    kw = R.problem(300)                                                      # one robot radius per handle
    seeds = [0, 1, 2, 3]
    fresh = {k: R.plan(dict(kw, obstacles=v), seeds, use_map=k != "t") for k, v in lists.items()}
    h = R.make_handle(kw, len(seeds))
    try:
        for step, which in enumerate("abta"):
            (h.set_obstacles if which == "t" else h.set_obstacle_map)(lists[which])
            h.seed_instances(seeds)
            h.plan(strict=True)
            R.same(R.read(h, len(seeds)), fresh[which], "step %d (%s)" % (step, which))    # a re-plan on a reused handle
            if which == "t":
                with pytest.raises(Exception, match="no obstacle map"):
                    h.obstacle_map_info()
            else:
                OM.assert_map_equals(h, kw["rand_area"], lists[which], kw["robot_radius"])
        with pytest.raises(rrt_amd._abi.RrtxError, match="RRTX_ALGO_RS: more than 64 obstacles"):
            h.set_obstacles(R.problem(65)["obstacles"])                       # the tile's limit is what it was
        assert h.obstacle_map_info()["n_circles"] == 300                      # and the refusal left the map
    finally:
        h.close()


def test_gpu_own_starts_and_goals_and_shards(gpu):
    import rrt_amd
    kw = R.problem(300)
    seeds = [0, 1, 2, 3]
    starts = [[0.1 * i, -0.1 * i, 0.05 * i] for i in range(4)]
    goals = [[6.0 + 0.1 * i, 9.0 - 0.1 * i, math.pi / 2 - 0.02 * i] for i in range(4)]
    out = R.plan(kw, seeds, starts=starts, goals=goals)
    R.equals_oracle(kw, seeds, out, "own starts and goals", starts=starts, goals=goals)
    got = []
    for devices in (None, [0, 0]):
        bp = rrt_amd.BatchPlanner("rrt_star_reeds_shepp", seeds, kw["start"], kw["goal"], kw["obstacles"], kw["rand_area"],
                                  max_iter=kw["max_iter"], robot_radius=kw["robot_radius"], search_until_max_iter=True,
                                  curvature=1.0, step_size=0.2, starts=starts, goals=goals, devices=devices)
        try:
            assert bp.has_obstacle_map
            bp.plan()
            got.append(([bp.tree(i) for i in range(4)], [bp.path(i) for i in range(4)], [bp.rng_state(i) for i in range(4)]))
            for h in bp.handles:
                OM.assert_map_equals(h, kw["rand_area"], kw["obstacles"], kw["robot_radius"])     # every shard built its own
            c = bp.courses()
            for i in range(4):
                p, q = bp.path(i), c.course(i)
                assert (p is None) == (q is None)
                if p is not None:
                    assert np.array_equal(tu.bits(p), tu.bits(q))
        finally:
            bp.close()
    for i in range(4):
        util.assert_tree_equal(got[0][0][i], got[1][0][i], "sharded, instance %d" % i)
        util.assert_tree_equal(got[0][0][i], out["trees"][i], "BatchPlanner, instance %d" % i)
        assert (got[0][1][i] is None) == (got[1][1][i] is None)
        if got[0][1][i] is not None:
            assert np.array_equal(got[0][1][i], got[1][1][i])
        assert got[0][2][i] == got[1][2][i]


# ---- G8 .. G10: the closed-loop stage -----------------------------------------------------------------------------------------
def closed_loop(seeds, circles, rr, max_iter, **extra):
    import rrt_amd
    return rrt_amd.BatchPlanner("closed_loop_rrt_star", seeds=seeds, start=R.START, goal=R.GOAL, obstacle_list=circles,
                                rand_area=R.RAND_AREA, max_iter=max_iter, connect_circle_dist=R.CCD, robot_radius=rr, **extra)


def test_gpu_closed_loop_tile_against_map_at_64(gpu):
    rmin, rmax, rr = R.SCENES[65]
    circles = R.scene(R.MAP_SEED, 65, rmin, rmax)[:64]
    a, b = closed_loop(R.SEEDS, circles, rr, 60, obstacle_map=False), closed_loop(R.SEEDS, circles, rr, 60, obstacle_map=True)
    try:
        assert not a.has_obstacle_map and b.has_obstacle_map
        a.plan()
        b.plan()
        fa, fb = a.track(), b.track()
        assert fa.tolist() == fb.tolist()
        n_cand = hit = 0
        for i in range(len(R.SEEDS)):
            util.assert_tree_equal(a.tree(i), b.tree(i), "instance %d" % i)
            ca, ra = a.track_records(i)
            cb, rb = b.track_records(i)
            assert ca.tolist() == cb.tolist() and ra.tobytes() == rb.tobytes()
            n_cand += len(ca)
            hit += int(np.sum((ra["fail"] & 8) != 0))
            ta, tb = a.trajectory(i), b.trajectory(i)
            assert (ta is None) == (tb is None)
            if ta is not None:
                assert all(np.array_equal(tu.bits(p), tu.bits(q)) for p, q in zip(ta, tb))
        assert n_cand > 0 and 0 < hit < n_cand            # the check decided something, both ways
        goals = np.array([[6.0, 9.0, math.pi / 2], [5.5, 8.5, 1.4], [9.0, 6.0, 0.3], [2.0, 10.0, 2.0]])
        ga, gb = a.track_goals(goals, xy_th=2.0, yaw_th=0.6), b.track_goals(goals, xy_th=2.0, yaw_th=0.6)
        for k in FIELDS + ("no_tree", "cand_offsets", "cand_node", "cand_find", "cand_len", "cand_fail", "cand_ood", "arr_offsets"):
            assert np.array_equal(getattr(ga, k), getattr(gb, k)), k
        assert np.array_equal(tu.bits(ga.t_last), tu.bits(gb.t_last)) and np.array_equal(tu.bits(ga.cand_t_last), tu.bits(gb.cand_t_last))
        for name in ga.ARRAYS:
            assert getattr(ga, name).tobytes() == getattr(gb, name).tobytes(), name
        assert ga.cand_offsets[-1] > 0 and np.any(ga.cand_fail & 8) and not np.all(ga.cand_fail & 8)
    finally:
        a.close()
        b.close()


@pytest.fixture(scope="module")
def track_exe(tmp_path_factory):
    return gt.build(tmp_path_factory.mktemp("rs_obsmap_track"))


CL_GOLDENS = sorted(glob.glob(os.path.join(util.GOLDEN, "obsmap_cl_m300_s*.npz")))


def test_closed_loop_goldens_hold_both_collision_verdicts():
    fails = np.concatenate([tu.load(p)[0]["cand_fail"] for p in CL_GOLDENS])
    assert np.any(fails & 8) and np.any((fails & 8) == 0)


@pytest.mark.parametrize("entry", ["class", "module"])
@pytest.mark.parametrize("path", CL_GOLDENS, ids=lambda p: os.path.basename(p)[:-4])
def test_gpu_closed_loop_goldens_bit_for_bit(gpu, track_exe, tmp_path, path, entry):
    import rrt_amd
    import rrt_amd.rrt_10
    g, kw, model = tu.load(path)
    assert len(kw["obstacle_list"]) == 300
    cls = rrt_amd.ClosedLoopRRTStar if entry == "class" else rrt_amd.rrt_10.ClosedLoopRRTStar
    random.seed(int(g["seed"]))
    obj = cls(**kw)
    out = obj.planning(animation=False)
    st = random.getstate()
    x, y, cost, parent = obj.tree
    assert np.array_equal(tu.bits(x), tu.bits(g["x"])) and np.array_equal(tu.bits(y), tu.bits(g["y"]))
    assert np.array_equal(tu.bits(obj.yaw), tu.bits(g["yaw"])) and np.array_equal(tu.bits(cost), tu.bits(g["cost"]))
    assert np.array_equal(np.asarray(parent), g["parent"])
    plen, px, py = obj.polylines
    assert np.array_equal(np.asarray(plen), g["plen"])
    assert np.array_equal(tu.bits(px), tu.bits(g["px"])) and np.array_equal(tu.bits(py), tu.bits(g["py"]))
    assert np.array_equal(np.array(st[1][:624], dtype=np.uint32), g["mt_after"]) and st[1][624] == int(g["mt_pos_after"])
    assert obj.get_goal_indexes() == g["cand"].tolist()
    rec = obj.records
    assert rec["find_goal"].tolist() == g["cand_find"].tolist() and rec["len"].tolist() == g["cand_len"].tolist()
    assert rec["fail"].tolist() == g["cand_fail"].tolist()
    assert np.array_equal(tu.bits(rec["t_last"]), tu.bits(g["cand_tlast"]))
    assert bool(out[0]) == bool(g["flag"])
    for k, name in enumerate(("out_x", "out_y", "out_yaw", "out_v", "out_t", "out_a", "out_d")):
        if not out[0]:
            assert out[k + 1] is None
        else:
            assert np.array_equal(tu.bits(out[k + 1]), tu.bits(g[name])), name
    if entry == "class":
        # the per-candidate records against the CPU restatement: the course of every candidate through the host tracker core
        params = dict(model)
        params.update({k: kw[k] for k in tu.PORDER[:4]})
        jobs = [tu.job(params, kw["obstacle_list"], kw["robot_radius"], *tu.course(g, c, kw)) for c in g["cand"]]
        for k, (find, n, fail, ood, tl, _) in enumerate(gt.roll(track_exe, tmp_path, jobs)):
            assert ood == 0 and (find, n, fail) == (int(rec["find_goal"][k]), int(rec["len"][k]), int(rec["fail"][k])), k
            assert tu.bits([tl])[0] == tu.bits([rec["t_last"][k]])[0], k


def test_gpu_closed_loop_batch_on_the_map(gpu, tmp_path):
    """One batch over the golden seeds: tree, candidates, records, trajectory and export against the goldens."""
    gs = [tu.load(p) for p in CL_GOLDENS]
    kw = gs[0][1]
    seeds = [int(g["seed"]) for g, _, _ in gs]
    bp = closed_loop(seeds, kw["obstacle_list"], kw["robot_radius"], kw["max_iter"], devices=[0, 0])
    try:
        assert bp.has_obstacle_map
        bp.plan()
        flags = bp.track(**{k: kw[k] for k in tu.PORDER[:4]})
        z = np.load(bp.export_npz(str(tmp_path / "cl.npz")))
        for i, (g, _, _) in enumerate(gs):
            assert bool(flags[i]) == bool(g["flag"])
            x, y, cost, parent = bp.tree(i)
            for got, name in ((x, "x"), (y, "y"), (cost, "cost"), (bp.yaw(i), "yaw")):
                assert np.array_equal(tu.bits(got), tu.bits(g[name])), (i, name)
            assert np.array_equal(np.asarray(parent), g["parent"])
            plen, px, py = bp.polylines(i)
            assert np.array_equal(np.asarray(plen), g["plen"])
            assert np.array_equal(tu.bits(px), tu.bits(g["px"])) and np.array_equal(tu.bits(py), tu.bits(g["py"]))
            assert np.array_equal(tu.bits(bp.polyline_yaw(i)), tu.bits(g["pyaw"]))
            st = bp.rng_state(i)
            assert np.array_equal(np.array(st[1][:624], dtype=np.uint32), g["mt_after"]) and st[1][624] == int(g["mt_pos_after"])
            cand, rec = bp.track_records(i)
            assert cand.tolist() == g["cand"].tolist() and rec["fail"].tolist() == g["cand_fail"].tolist()
            assert rec["find_goal"].tolist() == g["cand_find"].tolist()
            assert rec["len"].tolist() == g["cand_len"].tolist() and np.array_equal(tu.bits(rec["t_last"]), tu.bits(g["cand_tlast"]))
            tr = bp.trajectory(i)
            assert (tr is not None) == bool(g["flag"])
            assert bool(z["track_flag_%d" % i]) == bool(g["flag"])
            if tr is not None:
                for a, name in zip(tr, ("out_x", "out_y", "out_yaw", "out_v", "out_t", "out_a", "out_d")):
                    assert np.array_equal(tu.bits(a), tu.bits(g[name])), (i, name)
                    assert np.array_equal(tu.bits(z["track_%s_%d" % (name[4:], i)]), tu.bits(g[name])), (i, name)
        assert len(bp.results()[0]) == len(seeds)
    finally:
        bp.close()


def test_gpu_track_goals_on_300_circles_equals_the_oracle(gpu, track_exe, tmp_path):
    import rrt_amd
    rmin, rmax, rr = R.SCENES[300]
    circles = R.scene(R.MAP_SEED, 300, rmin, rmax)
    seeds = [1, 7, 8]
    bp = closed_loop(seeds, circles, rr, R.CL_MAX_ITER)
    try:
        bp.plan()
        goals = np.array([[6.0, 9.0, math.pi / 2], [5.5, 8.5, 1.4], [9.0, 6.0, 0.3], [2.0, 10.0, 2.0]])
        th = dict(xy_th=2.0, yaw_th=0.6)
        res = bp.track_goals(goals, **th)
        P = dict(rrt_amd._abi.TRACK_DEFAULTS, **th)
        trees = []
        for i in range(len(seeds)):
            x, y, _, parent = bp.tree(i)
            plen, px, py = bp.polylines(i)
            trees.append(dict(x=x, y=y, yaw=bp.yaw(i), parent=parent, plen=plen, px=px, py=py, pyaw=bp.polyline_yaw(i)))
        pairs = [(i, j) for i in range(len(seeds)) for j in range(len(goals))]
        want = gt.answer(track_exe, tmp_path, [(trees[i], R.START, circles, rr, goals[j]) for i, j in pairs], P)
        fails = []
        for (i, j), w in zip(pairs, want):
            cand, rec = res.records(i, j)
            assert np.array_equal(cand, w["cand"]), (i, j)
            got = np.column_stack([rec["find_goal"], rec["len"], rec["fail"], rec["ood"]])
            assert np.array_equal(got, w["rec"][:, :4].astype(np.int64)), (i, j)
            assert np.array_equal(tu.bits(rec["t_last"]), tu.bits(w["rec"][:, 4])), (i, j)
            for k in FIELDS:
                assert int(getattr(res, k)[i, j]) == int(w[k]), (i, j, k)
            tr = res.trajectory(i, j)
            assert (tr is None) == (w["arr"] is None), (i, j)
            if tr is not None:
                for k, a in enumerate(tr):
                    assert np.array_equal(tu.bits(a), tu.bits(w["arr"][k, :len(a)])), (i, j, k)
            fails += rec["fail"].tolist()
        fails = np.array(fails)
        assert len(fails) > 0 and np.any(fails & 8) and np.any((fails & 8) == 0)
    finally:
        bp.close()


# ---- G11. what stays refused --------------------------------------------------------------------------------------------------
def test_gpu_smooth_and_query_goals_stay_refused_with_a_map(gpu):
    import rrt_amd
    kw = R.problem(300, max_iter=20)
    bp = rrt_amd.BatchPlanner("rrt_star_reeds_shepp", [0, 1], kw["start"], kw["goal"], kw["obstacles"], kw["rand_area"],
                              max_iter=20, robot_radius=kw["robot_radius"], search_until_max_iter=True, curvature=1.0)
    try:
        bp.plan()
        for call in (lambda: bp.smooth(10), lambda: bp.query_goals([[5.0, 5.0, 0.0]])):
            with pytest.raises(ValueError, match="obstacle map.*64"):
                call()
        h = bp.h
        assert h.L.rrtx_query_goals(h._h, 1, 0, np.array([1.0, 2.0, 0.0]).ctypes.data, math.nan, math.nan) == -5
        assert "obstacle map" in h.last_error()
        assert h.L.rrtx_smooth_planned(h._h, 10) == -5 and "obstacle map" in h.last_error()
        # the argument checks of rrtx_set_obstacle_map on this handle (they need a handle, so a device): RRTX_E_INVALID, and
        # the map of the plan stays
        one = np.array([[1.0, 2.0, 0.5]])
        bad = np.array([[1.0, 2.0, 0.5], [3.0, np.nan, 0.5]])
        for ptr, m, word in ((None, 1, "NULL"), (one.ctypes.data, (1 << 20) + 1, "2^20"), (bad.ctypes.data, 2, "not finite")):
            assert h.L.rrtx_set_obstacle_map(h._h, ptr, m) == -1 and word in h.last_error(), word
        assert h.obstacle_map_info()["n_circles"] == 300
        c_min, c = rrt_amd.informed_rotation([0.0, 0.0], [6.0, 7.0])
        hi = rrt_amd._abi.Handle(rrt_amd._abi.ALGO_INFORMED, [0.0, 0.0], [6.0, 7.0], [-2.0, 15.0], 0.5, 1.0, 10, 20,
                                 informed_rot=[c[0, 0], c[0, 1], c[1, 0], c[1, 1]], informed_c_min=c_min)
        try:
            assert hi.L.rrtx_set_obstacle_map(hi._h, one.ctypes.data, 1) == -1 and "RRTX_ALGO_RRT" in hi.last_error()
        finally:
            hi.close()
        h.set_instance_obstacles([[(1.0, 1.0, 0.1)], []])                     # per-instance lists cannot be combined with a
        with pytest.raises(rrt_amd._abi.RrtxError, match="no obstacle map"):    # map: they drop it
            h.obstacle_map_info()
    finally:
        bp.close()

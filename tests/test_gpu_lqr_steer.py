"""BatchSteer("lqr") on the GPU: the reference's numbers (tests/golden/lqr_kat.npz: rrt_09's edges; lqr_steer_kat.npz: the
lqr_path script's rollouts, its control cases and rrt_09's check_collision), the pure-Python oracle at the wave and block
edges of the kernels, product mode, one steer object shared by the kinds, the drop-in module and the tracker's refusal.
Every comparison of doubles is one of bit patterns."""
import numpy as np
import pytest

import lqr_steer_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bs(gpu):
    import rrt_amd
    with rrt_amd.BatchSteer("lqr") as b:
        yield b


def check_batch(res, exp, points=True):
    """One result against the expected dicts of lqr_steer_util.expected, pair by pair"""
    import rrt_amd
    A = rrt_amd._abi
    assert len(res) == len(exp)
    assert res.status.tolist() == [A.STEER_OK if e["n_seg"] else A.STEER_NO_PATH for e in exp]
    assert res.rc == (A.RRTX_PARTIAL if any(e["n_seg"] == 0 for e in exp) else 0)
    assert res.n_seg.tolist() == [e["n_seg"] for e in exp]
    assert np.array_equal(U.bits(res.end), U.bits([e["end"] for e in exp]))
    assert np.array_equal(U.bits(res.length), U.bits([e["length"] for e in exp]))
    assert res.yaw is None and res.seg_len.any() == False and set(res.modes) <= {""}   # noqa: E712
    if not points:
        assert res.x is None and res.y is None and res.offsets is None
        return
    assert np.diff(res.offsets).tolist() == [len(e["x"]) for e in exp]
    assert np.array_equal(U.bits(res.x), U.bits([v for e in exp for v in e["x"]]))
    assert np.array_equal(U.bits(res.y), U.bits([v for e in exp for v in e["y"]]))


def test_rrt09_edges_bit_identical(bs):
    """lqr_kat.npz: the 300 edges of the reference's steer, one call per step size"""
    g = U.kat("lqr_kat")
    rows = g["rows"]
    p_off = np.concatenate([[0], np.cumsum(g["np"])])
    for step in sorted(set(rows[:, 4].tolist())):
        idx = np.nonzero(rows[:, 4] == step)[0]
        res = bs.plan(rows[idx, 0:2], rows[idx, 2:4], step_size=step)
        assert res.rc == 0 and not res.status.any()
        assert np.array_equal(res.n_seg, g["nw"][idx])
        assert np.array_equal(np.diff(res.offsets), g["np"][idx])
        want = np.concatenate([np.arange(p_off[i], p_off[i + 1]) for i in idx])
        assert np.array_equal(U.bits(res.x), U.bits(g["px"][want]))
        assert np.array_equal(U.bits(res.y), U.bits(g["py"][want]))
        assert np.array_equal(U.bits(res.end), U.bits(g["ends"][idx, 0:2]))
        assert np.array_equal(U.bits(res.length), U.bits(g["ends"][idx, 2]))
    i = int(idx[0])
    px, py, cl = res.path(0)
    c_off = int(p_off[i]) - i   # an edge of n points has n - 1 course lengths
    assert np.array_equal(U.bits(cl), U.bits(g["clen"][c_off:c_off + len(px) - 1]))


def test_script_rollouts_bit_identical(bs):
    """lqr_steer_kat.npz (a): LQRPlanner.lqr_planning's rx, ry; the length is the package's definition"""
    g = U.kat("lqr_steer_kat")
    a = g["a_pairs"]
    res = bs.plan(a[:, 0:2], a[:, 2:4], resample=False)
    assert res.rc == 0 and np.array_equal(res.n_seg, g["a_n"]) and np.array_equal(np.diff(res.offsets), g["a_n"])
    assert np.array_equal(U.bits(res.x), U.bits(g["a_rx"])) and np.array_equal(U.bits(res.y), U.bits(g["a_ry"]))
    last = res.offsets[1:] - 1
    assert np.array_equal(U.bits(res.end), U.bits(np.stack([g["a_rx"][last], g["a_ry"][last]], axis=1)))
    want = [U.hypot_sum(g["a_rx"][a0:a1].tolist(), g["a_ry"][a0:a1].tolist()) for a0, a1 in zip(res.offsets, res.offsets[1:])]
    assert np.array_equal(U.bits(res.length), U.bits(want))
    rx, ry = res.path(3)
    assert isinstance(rx, list) and rx == g["a_rx"][res.offsets[3]:res.offsets[4]].tolist()


def test_control_cases(bs):
    """lqr_steer_kat.npz (b): MAX_TIME and GOAL_DIST as the issue measured them on the reference"""
    import rrt_amd
    A = rrt_amd._abi
    g = U.kat("lqr_steer_kat")
    p = g["b_pairs"]
    assert g["b_n"].tolist() == [[0, 2, 0], [0, 2, 0], [19, 2, 19], [14, 2, 18], [4, 2, 8], [0, 0, 0]]
    off = 0
    for (mt, gd), n in zip(g["b_ctl"], g["b_n"]):
        res = bs.plan(p[:, 0:2], p[:, 2:4], resample=False, max_time=float(mt), goal_dist=float(gd))
        assert res.n_seg.tolist() == n.tolist() == np.diff(res.offsets).tolist(), (mt, gd)
        assert res.status.tolist() == [A.STEER_OK if k else A.STEER_NO_PATH for k in n], (mt, gd)
        assert res.rc == (0 if n.all() else A.RRTX_PARTIAL)
        tot = int(n.sum())
        assert np.array_equal(U.bits(res.x), U.bits(g["b_rx"][off:off + tot])), (mt, gd)
        assert np.array_equal(U.bits(res.y), U.bits(g["b_ry"][off:off + tot])), (mt, gd)
        off += tot
        for i in range(3):
            if not n[i]:
                assert res.path(i) == ([], [])


@pytest.mark.parametrize("points", [True, False])
def test_obstacle_check_matches_check_collision(bs, points):
    """lqr_steer_kat.npz (c): the first circle at which rrt_09's check_collision refuses the edge"""
    g = U.kat("lqr_steer_kat")
    cp, hit = g["c_pairs"], g["c_hit"]
    for step in sorted(set(g["c_step"].tolist())):
        idx = np.nonzero(g["c_step"] == step)[0]
        res = bs.plan(cp[idx, 0:2], cp[idx, 2:4], step_size=step, points=points, obstacle_list=g["c_obs"],
                      robot_radius=float(g["c_rr"]))
        assert res.hit.tolist() == hit[idx].tolist(), step
        assert res.free.tolist() == (hit[idx] == -1).tolist()
        assert (res.x is None) == (not points)
        assert res.is_free(0) == (hit[idx[0]] == -1)


def edge_pairs(n, seed):
    rs = np.random.RandomState(seed)
    p = np.concatenate([rs.uniform(-2, 15, (n, 2)), rs.uniform(-2, 15, (n, 2))], axis=1)
    p[::7, 2:] = p[::7, :2] + rs.uniform(-1, 1, (len(p[::7]), 2)) * 0.05   # one segment: within GOAL_DIST at once
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_against_the_oracle_at_wave_and_block_edges(bs, n):
    p = edge_pairs(n, 100 + n)
    step = [0.2, 0.15, 0.3, 0.07, 0.25][n % 5]
    exp = [U.expected(q, step) for q in p]
    check_batch(bs.plan(p[:, 0:2], p[:, 2:4], step_size=step), exp)
    check_batch(bs.plan(p[:, 0:2], p[:, 2:4], step_size=step, points=False), exp, points=False)
    raw = [U.expected(q, None) for q in p]
    check_batch(bs.plan(p[:, 0:2], p[:, 2:4], resample=False), raw)


def test_a_curve_spans_blocks_and_a_wave_spans_curves(bs):
    """goal_dist = 0.0 and step_size = 0.07: 18 segments of 15 points = 270 points, more than one 256-thread block of the
    fill / check kernel, beside edges of one segment (15 points, start == goal), several of which share a wave."""
    rs = np.random.RandomState(5)
    p = np.concatenate([rs.uniform(-2, 15, (40, 2)), rs.uniform(-2, 15, (40, 2))], axis=1)
    short = np.arange(40) % 4 != 1
    p[short, 2:] = p[short, :2]
    exp = [U.expected(q, 0.07, 100.0, 0.0) for q in p]
    counts = [len(e["x"]) for e in exp]
    assert max(counts) > 256 and min(counts) < 64 and counts[1] == 270
    obs = [(float(rs.uniform(-2, 15)), float(rs.uniform(-2, 15)), float(rs.uniform(0.3, 1.2))) for _ in range(12)]
    hit = [U.first_hit(e["x"], e["y"], obs, 0.25) for e in exp]
    assert sum(h >= 0 for h in hit) >= 5 and sum(h == -1 for h in hit) >= 5
    for points in (True, False):
        res = bs.plan(p[:, 0:2], p[:, 2:4], step_size=0.07, goal_dist=0.0, points=points, obstacle_list=obs,
                      robot_radius=0.25)
        check_batch(res, exp, points=points)
        assert res.hit.tolist() == hit
    check_batch(bs.plan(p[:, 0:2], p[:, 2:4], step_size=0.07, goal_dist=0.0), exp)   # the list is cleared again
    # a batch in which some rollouts never arrive: they own no points, and the check skips them
    exp = [U.expected(q, 0.2, 0.0, 0.1) for q in p]
    assert 0 < sum(e["n_seg"] == 0 for e in exp) < 40
    res = bs.plan(p[:, 0:2], p[:, 2:4], max_time=0.0, obstacle_list=obs, robot_radius=0.25)
    check_batch(res, exp)
    assert res.hit.tolist() == [U.first_hit(e["x"], e["y"], obs, 0.25) if e["n_seg"] else -2 for e in exp]
    with pytest.raises(IndexError):
        res.is_free(1)


def test_product_mode_equals_the_pairs_one_by_one(bs):
    rs = np.random.RandomState(17)
    s, g = rs.uniform(-2, 15, (3, 2)), rs.uniform(-2, 15, (5, 2))
    obs = [(float(rs.uniform(0, 13)), float(rs.uniform(0, 13)), float(rs.uniform(0.5, 1.5))) for _ in range(10)]
    res = bs.plan(s, g, product=True, points=False, obstacle_list=obs, robot_radius=0.2)
    full = bs.plan(s, g, product=True, obstacle_list=obs, robot_radius=0.2)
    assert res.shape == (3, 5) and len(res) == 15 and res.x is None
    for p in range(15):
        one = bs.plan(s[p // 5:p // 5 + 1], g[p % 5:p % 5 + 1], obstacle_list=obs, robot_radius=0.2)
        for r in (res, full):
            assert U.bits(r.length)[p] == U.bits(one.length)[0] and r.n_seg[p] == one.n_seg[0] and r.hit[p] == one.hit[0]
            assert np.array_equal(U.bits(r.end[p]), U.bits(one.end[0]))
        a, b = full.offsets[p], full.offsets[p + 1]
        assert np.array_equal(U.bits(full.x[a:b]), U.bits(one.x)) and np.array_equal(U.bits(full.y[a:b]), U.bits(one.y))
    exp = [U.expected((s[p // 5, 0], s[p // 5, 1], g[p % 5, 0], g[p % 5, 1]), 0.2) for p in range(15)]
    check_batch(full, exp)
    assert 0 < int(np.sum(res.hit != -1)) < 15
    m = res.length_matrix(free_only=True)
    assert m.shape == (3, 5)
    assert np.array_equal(np.isposinf(m), (res.hit != -1).reshape(3, 5))
    assert np.array_equal(U.bits(m[~np.isposinf(m)]), U.bits(res.length.reshape(3, 5)[~np.isposinf(m)]))
    assert np.array_equal(U.bits(res.length_matrix()), U.bits(res.length.reshape(3, 5)))


def test_one_steer_object_serves_the_kinds_in_turn(gpu):
    """dubins -> lqr -> dubins -> lqr on one rrtx_steer with different n: each answer is a fresh object's"""
    import rrt_amd
    A = rrt_amd._abi
    rs = np.random.RandomState(23)

    def poses(n):
        return np.concatenate([rs.uniform(-2, 15, (n, 2)), rs.uniform(-np.pi, np.pi, (n, 1))], axis=1)

    def dubins(S, st, go):
        rc = S.solve(A.STEER_DUBINS, st, go, 1.0, 0.1)
        return (rc,) + tuple(S.summary()) + tuple(S.points())

    def lqr(S, st, go, step):
        rc = S.solve_lqr(st, go, step)
        status, length, nseg, seglen, modes, off = S.summary()
        assert not seglen.any() and set(modes.tolist()) <= {b""}
        with pytest.raises(A.RrtxError, match="RRTX_E_STATE"):
            S.points()   # a rollout has no yaw
        x, y, _ = S.points(yaw=False)
        return rc, status, length, nseg, off, x, y, S.ends()

    def same(a, b):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            u, v = np.asarray(u), np.asarray(v)
            assert u.shape == v.shape and u.tobytes() == v.tobytes()

    jobs = [("d", poses(40), poses(40)), ("l", poses(130)[:, :2].copy(), poses(130)[:, :2].copy(), 0.2),
            ("d", poses(7), poses(7)), ("l", poses(9)[:, :2].copy(), poses(9)[:, :2].copy(), 0.0)]
    with A.Steer(0) as shared:
        for job in jobs:
            fn = dubins if job[0] == "d" else lqr
            got = fn(shared, *job[1:])
            if job[0] == "d":
                with pytest.raises(A.RrtxError, match="RRTX_E_STATE"):
                    shared.ends()   # the last solve was not an LQR solve
            with A.Steer(0) as fresh:
                same(got, fn(fresh, *job[1:]))


def test_dropin_planner_reproduces_the_control_cases(gpu, capsys):
    import rrt_amd.lqr_path as lp
    g = U.kat("lqr_steer_kat")
    planner = lp.LQRPlanner()
    off = 0
    for (mt, gd), n in zip(g["b_ctl"], g["b_n"]):
        planner.MAX_TIME, planner.GOAL_DIST = float(mt), float(gd)
        for p, k in zip(g["b_pairs"], n):
            capsys.readouterr()
            rx, ry = planner.lqr_planning(float(p[0]), float(p[1]), float(p[2]), float(p[3]), show_animation=False)
            assert isinstance(rx, list) and isinstance(ry, list) and len(rx) == len(ry) == k
            assert capsys.readouterr().out == ("" if k else "Cannot found path\n")
            assert np.array_equal(U.bits(rx), U.bits(g["b_rx"][off:off + k]))
            assert np.array_equal(U.bits(ry), U.bits(g["b_ry"][off:off + k]))
            off += k


def test_wrong_keywords_for_the_kind(bs):
    import rrt_amd
    p = np.zeros((1, 2))
    with pytest.raises(ValueError):
        bs.plan(p, p, 1.0)
    with pytest.raises(ValueError):
        bs.plan(p, p, selected_types=["LSL"])
    with rrt_amd.BatchSteer("dubins") as d:
        with pytest.raises(TypeError):
            d.plan(np.zeros((1, 3)), np.ones((1, 3)))
        with pytest.raises(ValueError):
            d.plan(np.zeros((1, 3)), np.ones((1, 3)), 1.0, resample=False)


def test_tracker_refuses_an_lqr_result(bs):
    import rrt_amd
    res = bs.plan([[0.0, 0.0]], [[6.0, 10.0]])
    with rrt_amd.BatchTrack() as bt:
        with pytest.raises(ValueError, match="yaw"):
            bt.run(res)

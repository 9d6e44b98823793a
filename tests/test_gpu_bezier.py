"""BatchSteer("bezier") on the GPU: the reference's numbers (tests/golden/bezier_kat.npz), the pure-Python oracle at the wave
and block edges of the kernels, product mode and the filtered cost matrix, the points=False variants, control points of
every supported degree, one steer object shared by the kinds, the tracker and the drop-in module.
Every comparison of doubles is one of bit patterns, NaN equal to NaN."""
import numpy as np
import pytest

import bezier_oracle as O
import bezier_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bs(gpu):
    import rrt_amd
    with rrt_amd.BatchSteer("bezier") as b:
        yield b


def golden_flat(idx, key):
    return np.concatenate([U.golden_curve(i)[key] for i in idx])


def oracle_of(idx):
    return O.batch([U.oracle_curve(i) for i in idx])


def check_golden(res, idx, what):
    """x, y, k and the control points against the file; yaw, length and kmax (this package's definitions) against the oracle"""
    for key in ("x", "y", "k"):
        U.assert_same(getattr(res, key), golden_flat(idx, key), "%s %s" % (what, key))
    U.assert_same(res.control_points, np.array([U.control_points(i) for i in idx]), what + " control points")
    U.assert_result(res, oracle_of(idx), what)
    assert res.n_seg.tolist() == [len(U.control_points(i)) for i in idx] and not res.seg_len.any()


def test_golden_file_bit_identical(bs):
    """The whole file: one call per n_points value of the pose curves and per (m, n_points) of the control-point curves,
    each with the obstacle list "first"; the other two lists with points=False"""
    g = U.kat()
    groups = [("poses n_points=%d" % n, idx) for n, idx in sorted(U.pose_groups().items())]
    groups += [("m=%d n_points=%d" % key, idx) for key, idx in sorted(U.cp_groups().items())]
    assert sorted(i for _, idx in groups for i in idx) == list(range(len(g["n_points"])))

    def solve(idx, name, points):
        obs, rr, want = U.obstacles(name)
        n = int(g["n_points"][idx[0]])
        if idx[0] < U.n_pose():
            p = g["pose"][idx]
            res = bs.plan(p[:, 0:3], p[:, 3:6], offset=p[:, 6], n_points=n, points=points, obstacle_list=obs, robot_radius=rr)
        else:
            res = bs.plan_control_points(np.array([U.control_points(i) for i in idx]), n_points=n, points=points,
                                         obstacle_list=obs, robot_radius=rr)
        assert res.hit.tolist() == want[idx].tolist(), (name, idx[0])
        return res
    for what, idx in groups:
        check_golden(solve(idx, "first", True), idx, what)
        for name in ("last", "none"):
            U.assert_result(solve(idx, name, False), oracle_of(idx), "%s %s" % (what, name), points=False)
    a, b, j = (int(v) for v in g["lone"])   # a circle at the first point only, one at the last point only
    assert g["hit_first"][a] == j and g["hit_last"][b] == j


EDGE_PAIRS = (1, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def edge_oracle():
    """257 seeded pose pairs and their oracle curves per n_points: the batches below are prefixes"""
    st, go, off = U.random_poses(11, max(EDGE_PAIRS))
    cache = {}

    def get(n_points):
        if n_points not in cache:
            cache[n_points] = [O.curve4(*st[i], *go[i], float(off[i]), n_points=n_points) for i in range(len(st))]
        return cache[n_points]
    return st, go, off, get


@pytest.mark.parametrize("n_points", [2, 64, 65, 100])
def test_launch_shape_edges(bs, edge_oracle, n_points):
    """n_points = 2: many curves per wave; 64: every wave inside one curve (the single atomic); 65, 100: waves straddle
    curves.  With and without obstacles."""
    st, go, off, get = edge_oracle
    curves = get(n_points)
    rs = np.random.RandomState(n_points)
    obs = np.stack([rs.uniform(0, 20, 12), rs.uniform(0, 20, 12), rs.uniform(0.2, 1.2, 12)], axis=1)
    hits = U.oracle_hits(O.batch(curves), obs, 0.3)   # a curve's hit does not depend on its batch
    for n in EDGE_PAIRS:
        ob = O.batch(curves[:n])
        what = "n=%d n_points=%d" % (n, n_points)
        U.assert_result(bs.plan(st[:n], go[:n], offset=off[:n], n_points=n_points), ob, what)
        res = bs.plan(st[:n], go[:n], offset=off[:n], n_points=n_points, obstacle_list=obs, robot_radius=0.3)
        U.assert_result(res, ob, what + " checked")
        assert res.hit.tolist() == hits[:n].tolist(), what
    assert np.sum(hits == -1) > 10 and np.sum(hits >= 0) > 10 and len(set(hits.tolist())) > 4


def test_product_mode_and_the_filtered_cost_matrix(bs):
    st, _, _ = U.random_poses(21, 3)
    go, _, _ = U.random_poses(22, 5)
    rs = np.random.RandomState(23)
    obs = np.stack([rs.uniform(0, 20, 6), rs.uniform(0, 20, 6), rs.uniform(0.5, 1.5, 6)], axis=1)
    prod = bs.plan(st, go, offset=2.5, n_points=50, product=True, obstacle_list=obs, robot_radius=0.2)
    ps, pg = np.repeat(st, 5, axis=0), np.tile(go, (3, 1))
    pair = bs.plan(ps, pg, offset=2.5, n_points=50, obstacle_list=obs, robot_radius=0.2)
    assert prod.shape == (3, 5) and pair.shape is None
    for key in ("x", "y", "yaw", "k", "length", "kmax", "control_points"):
        U.assert_same(getattr(prod, key), getattr(pair, key), key)
    assert prod.hit.tolist() == pair.hit.tolist()
    ob = U.oracle_batch(ps, pg, 2.5, 50)
    U.assert_result(prod, ob, "product")
    hit = U.oracle_hits(ob, obs, 0.2)
    assert prod.hit.tolist() == hit.tolist() and 0 < int(np.sum(hit == -1)) < 15
    c = float(np.median(ob["kmax"]))   # the median of 15 distinct values: 7 curves bend harder
    want = np.where((hit == -1) & (ob["kmax"] <= c), ob["length"], np.inf).reshape(3, 5)
    got = prod.length_matrix(free_only=True, max_curvature=c)
    U.assert_same(got, want, "length_matrix")
    assert 0 < int(np.sum(ob["kmax"] > c)) < 15 and 0 < int(np.sum(np.isinf(got))) < 15
    U.assert_same(prod.length_matrix(), ob["length"].reshape(3, 5), "plain matrix")
    # lengths only, per-pair offsets in product order
    offs = np.linspace(1.0, 4.5, 15)
    cost = bs.plan(st, go, offset=offs, n_points=50, points=False, product=True)
    U.assert_same(cost.length, U.oracle_batch(ps, pg, offs, 50)["length"], "per-pair offsets")


def test_points_false_variants(bs):
    import rrt_amd
    st, go, off = U.random_poses(31, 70)
    ob = U.oracle_batch(st, go, off, 100)
    rs = np.random.RandomState(32)
    obs = np.stack([rs.uniform(0, 20, 10), rs.uniform(0, 20, 10), rs.uniform(0.3, 1.0, 10)], axis=1)
    S = bs._steer
    full = bs.plan(st, go, offset=off)
    assert S.counts() == (70, 7000)
    # stage 1 alone
    res = bs.plan(st, go, offset=off, points=False)
    U.assert_result(res, ob, "points=False", points=False)
    assert S.counts() == (70, 0) and res.hit is None
    U.assert_same(res.length, full.length, "length")
    U.assert_same(res.kmax, full.kmax, "kmax")
    # checked, nothing stored
    chk = bs.plan(st, go, offset=off, obstacle_list=obs, robot_radius=0.1)
    res = bs.plan(st, go, offset=off, points=False, obstacle_list=obs, robot_radius=0.1)
    U.assert_result(res, ob, "points=False checked", points=False)
    assert res.hit.tolist() == chk.hit.tolist() == U.oracle_hits(ob, obs, 0.1).tolist() and S.counts() == (70, 0)
    assert 0 < int(np.sum(res.free)) < 70
    buf = np.zeros(7000)
    assert S.L.rrtx_steer_get_points(S._s, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 7000) == -5   # RRTX_E_STATE
    assert S.L.rrtx_steer_get_curvature(S._s, buf.ctypes.data, 7000) == -5
    # no curvature: no k, no kmax
    for points in (True, False):
        res = bs.plan(st, go, offset=off, curvature=False, points=points)
        U.assert_result(res, ob, "curvature=False", curvature=False, points=points)
        assert S.L.rrtx_steer_get_curvature(S._s, buf.ctypes.data, 7000) == -5
        assert S.L.rrtx_steer_get_kmax(S._s, buf.ctypes.data) == -5
    with pytest.raises(rrt_amd._abi.RrtxError):
        res.length_matrix()
    with pytest.raises(rrt_amd._abi.RrtxError):
        res.path(0)


@pytest.mark.parametrize("m", [3, 4, 8, 16])
def test_control_points_of_every_degree(bs, m):
    g = U.kat()
    rs = np.random.RandomState(40 + m)
    for n_points in (2, 33, 300):
        idx = U.cp_groups()[(m, n_points)]
        extra = [np.cumsum(rs.uniform(-2.0, 2.0, (m, 2)), axis=0) + rs.uniform(0, 20, 2) for _ in range(66)]
        cps = np.array([U.control_points(i) for i in idx] + extra)
        res = bs.plan_control_points(cps, n_points=n_points)
        ob = O.batch([U.oracle_curve(i) for i in idx] + [O.curve(c, n_points) for c in extra])
        U.assert_result(res, ob, "m=%d n_points=%d" % (m, n_points))
        for q, i in enumerate(idx):   # the golden rows
            a, b = res.offsets[q], res.offsets[q + 1]
            for key in ("x", "y", "k"):
                U.assert_same(getattr(res, key)[a:b], U.golden_curve(i)[key], "golden %d %s" % (i, key))
        path, cp = res.path(len(idx))
        assert path.shape == (n_points, 2) and np.array_equal(cp, extra[0])


def test_one_object_serves_the_kinds_in_turn(gpu):
    """Dubins -> Bezier (large) -> LQR -> Bezier (small): nothing of an earlier solve shows in a later one"""
    import rrt_amd
    A = rrt_amd._abi
    st, go, off = U.random_poses(51, 200)
    rs = np.random.RandomState(52)
    obs = np.stack([rs.uniform(0, 20, 8), rs.uniform(0, 20, 8), rs.uniform(0.3, 1.0, 8)], axis=1)

    def fresh(n, n_points, **kw):
        with rrt_amd.BatchSteer("bezier") as f:
            return f.plan(st[:n], go[:n], offset=off[:n], n_points=n_points, **kw)
    with rrt_amd.BatchSteer("dubins") as shared:
        S = shared._steer
        shared.plan(st, go, 1.0, obstacle_list=obs, robot_radius=0.2)
        shared.kind = A.STEER_BEZIER
        big = shared.plan(st, go, offset=off, n_points=120, obstacle_list=obs, robot_radius=0.2)
        ends = np.zeros((200, 2))
        assert S.L.rrtx_steer_get_ends(S._s, ends.ctypes.data) == -5   # RRTX_E_STATE after Bezier
        shared.kind = A.STEER_LQR
        shared.plan(st[:150, :2], go[:150, :2], obstacle_list=obs)
        buf = np.zeros(8)
        assert S.L.rrtx_steer_get_kmax(S._s, buf.ctypes.data) == -5 and S.L.rrtx_steer_get_control_points(S._s, None, None) == -5
        shared.kind = A.STEER_BEZIER
        small = shared.plan(st[:37], go[:37], offset=off[:37], n_points=45, obstacle_list=obs, robot_radius=0.2)
        bare = shared.plan(st[:90], go[:90], offset=off[:90], n_points=45)   # the list is cleared again
    for got, want in ((big, fresh(200, 120, obstacle_list=obs, robot_radius=0.2)),
                      (small, fresh(37, 45, obstacle_list=obs, robot_radius=0.2)), (bare, fresh(90, 45))):
        for key in ("x", "y", "yaw", "k", "length", "kmax", "control_points"):
            U.assert_same(getattr(got, key), getattr(want, key), key)
        assert np.array_equal(got.offsets, want.offsets)
        assert (got.hit is None) == (want.hit is None) and (got.hit is None or got.hit.tolist() == want.hit.tolist())
    assert bare.hit is None and 0 < int(np.sum(big.hit >= 0)) < 200
    U.assert_result(small, U.oracle_batch(st[:37], go[:37], off[:37], 45), "small after large")


def test_tracker_takes_the_result_and_the_dropin_is_the_script(bs):
    import rrt_amd
    import rrt_amd.bazier_path as bz
    st, go, off = U.random_poses(61, 6)
    res = bs.plan(st, go, offset=off, n_points=60)
    with rrt_amd.BatchTrack(T=20.0) as bt:
        a = bt.run(res)
        b = bt.run([res.course(i)[:3] for i in range(len(res))])
    assert len(a) == 6 and np.array_equal(a.offsets, b.offsets) and a.find_goal.tolist() == b.find_goal.tolist()
    for key in ("x", "y", "yaw", "v", "t", "length"):
        U.assert_same(getattr(a, key), getattr(b, key), "tracked " + key)
    # the script's driver pair
    g = U.kat()
    start_x, start_y, start_yaw = 10.0, 1.0, float(np.radians(180.0))
    end_x, end_y, end_yaw = -0.0, -3.0, float(np.radians(-45.0))
    for i, offset in enumerate(np.arange(1.0, 5.0, 1.0)):
        path, control_points = bz.calc_4points_bezier_path(start_x, start_y, start_yaw, end_x, end_y, end_yaw, offset)
        assert path.shape == (100, 2) and control_points.shape == (4, 2)
        assert path.T[0][0] == start_x and path.T[1][0] == start_y and path.T[0][-1] == end_x and path.T[1][-1] == end_y
        want = U.golden_curve(i)
        U.assert_same(path, np.stack([want["x"], want["y"]], axis=1), "driver path, offset %g" % offset)
        U.assert_same(control_points, g["pose_cp"][i], "driver control points")
        U.assert_same(bz.calc_bezier_path(control_points, n_points=100), path, "calc_bezier_path")
    i = U.n_pose() + 1   # a general control-point set through the drop-in
    want = U.golden_curve(i)
    U.assert_same(bz.calc_bezier_path(U.control_points(i), n_points=int(g["n_points"][i])),
                  np.stack([want["x"], want["y"]], axis=1), "calc_bezier_path, golden control points")

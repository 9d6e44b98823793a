"""The obstacle index of BatchSteer / BatchSpline / BatchBSpline on the GPU (steer_fill<KIND, STORE, CHECK_INDEX>
and its counterparts, rrtx_*_set_obstacle_index): the index read back equals the restatement of tests/obsindex_util.py
exactly, the golden rows the reference made equal `hit` bit for bit, and with the index ON every result equals the one
with the index OFF and check_collision evaluated in IEEE doubles over the device's own points -- at the shapes at which the
per-lane walk, the wave minimum and the cross-workgroup atomic minimum can go wrong.  Every comparison of hit is exact."""
import os
import warnings

import numpy as np
import pytest

import obsindex_util as OI
import steer_collide_util as scu
import spline_util
import bspline_util
import util

pytestmark = pytest.mark.gpu
GOLD = os.path.join(util.ROOT, "tests", "golden")
FILL_TPB = 256   # csrc/steer_batch.hip.h TPB: one lane per curve point
FAR = (500.0, 500.0, 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ref_hits(res_x, res_y, offsets, obs, rr, status=None):
    """check_collision over the device's own points, per curve: -2 no curve / no points, -1 free, else the first circle."""
    out = []
    for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        if (status is not None and status[i] != 0) or b == a:
            out.append(-2)
        else:
            out.append(scu.ref_hit((res_x[a:b], res_y[a:b]), obs, rr))
    return np.array(out, dtype=np.int32)


def city(seed, m, lo=0.0, hi=100.0, smin=0.3, smax=0.9):
    rs = np.random.RandomState(seed)
    return np.column_stack([rs.uniform(lo, hi, m), rs.uniform(lo, hi, m), rs.uniform(smin, smax, m)])


def pose_pairs(seed, n, lo=5.0, hi=95.0):
    rs = np.random.RandomState(seed)
    st = np.column_stack([rs.uniform(lo, hi, n), rs.uniform(lo, hi, n), rs.uniform(-np.pi, np.pi, n)])
    d, a = rs.uniform(0.5, 6.0, n), rs.uniform(-np.pi, np.pi, n)
    go = np.column_stack([st[:, 0] + d * np.cos(a), st[:, 1] + d * np.sin(a), rs.uniform(-np.pi, np.pi, n)])
    return st, go


@pytest.fixture(scope="module")
def steers(gpu):
    import rrt_amd
    out = {k: rrt_amd.BatchSteer(k) for k in ("dubins", "rs", "lqr", "bezier")}
    yield out
    for b in out.values():
        b.close()


def both(bs, call):
    """call() with the index ON and OFF: (on, off), the info checked."""
    bs.obstacle_index = True
    on = call()
    bs.obstacle_index = False
    off = call()
    bs.obstacle_index = None
    assert on.obstacle_index["used"] and on.obstacle_index["reason"] == "used" and on.obstacle_index["mode"] == OI.ON
    assert not off.obstacle_index["used"] and off.obstacle_index["reason"] == "off" and off.obstacle_index["nx"] == 0
    return on, off


# ---- the index as built ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,rr,wide,offset,forced", [(1, 0.0, 0, False, 0), (257, 0.25, 3, False, 0), (1000, 0.0, 3, False, 0),
                                                     (1000, 0.25, 0, True, 0), (20000, 0.25, 5, False, 0),
                                                     (1000, 0.0, 3, False, 1), (1000, 0.25, 3, True, 7)])
def test_index_read_back_equals_the_restatement(gpu, monkeypatch, m, rr, wide, offset, forced):
    import rrt_amd
    c = city(m, m, smin=0.05 if m > 5000 else 0.3, smax=0.3 if m > 5000 else 0.9)
    if offset:
        c[:, 0] += 1000.0
        c[:, 1] -= 10100.0
    for k in range(wide):                                                 # some for the wide list
        c[(k * (m // wide)) % m, 2] = 30.0 + k
    if forced:
        monkeypatch.setenv("RRTX_OBSMAP_CELLS", str(forced))
    with rrt_amd._abi.Steer() as S:
        S.set_obstacle_index(True)
        S.set_obstacles(c, rr)
        info = OI.assert_index_equals(S, c, rr, forced)
        assert info["nx"] == (forced or OI.OM.axis_cells(m))
        if not forced:
            assert info["n_wide"] == wide
        if offset:
            assert 1000.0 <= info["x0"] <= 1100.0 and -10100.0 <= info["y0"] <= -10000.0


# ---- the reference's answers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["d", "r"])
def test_golden_rows_with_the_index(steers, kind):
    z = np.load(os.path.join(GOLD, "steer_index_kat.npz"))
    inp, want, ob, rr = z[kind + "_inp"], z[kind + "_hit"], z["ob"], float(z["rr"])
    bs = steers["dubins" if kind == "d" else "rs"]
    kw = dict(obstacle_list=ob, robot_radius=rr, step_size=0.1 if kind == "d" else 0.2)

    def call(points):
        return lambda: bs.plan(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy(), points=points, **kw)
    for points in (True, False):
        on, off = both(bs, call(points))
        assert on.hit.dtype == np.int32 and np.array_equal(on.hit, want) and np.array_equal(off.hit, want), points
        assert np.array_equal(on.free, want == -1) and np.array_equal(on.hit == -2, on.status != 0)
    auto = call(False)()                                   # 1000 circles: AUTO takes the index
    assert auto.obstacle_index["used"] and auto.obstacle_index["mode"] == OI.AUTO and np.array_equal(auto.hit, want)
    assert auto.obstacle_index["n_circles"] == 1000 and auto.obstacle_index["nx"] == 32


# ---- ON == OFF == check_collision over the device's points, every kind ----------------------------------------------------
@pytest.mark.parametrize("kind", ["dubins", "rs", "lqr", "bezier"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_every_kind_on_equals_off_equals_the_oracle(steers, kind, n):
    bs = steers[kind]
    ob = city(5, 1000, smin=0.3, smax=1.2)
    st, go = pose_pairs(n, n)
    if kind == "lqr":
        args, kw = (st[:, :2], go[:, :2]), {}
    elif kind == "bezier":
        args, kw = (st, go), dict(offset=3.0, n_points=37)
    else:
        args, kw = (st, go, 1.0), {}
    on, off = both(bs, lambda: bs.plan(*args, obstacle_list=ob, robot_radius=0.2, **kw))
    want = ref_hits(on.x, on.y, on.offsets, ob, 0.2, on.status)
    assert np.array_equal(on.hit, want) and np.array_equal(off.hit, want)
    assert np.array_equal(bits(on.x), bits(off.x)) and np.array_equal(bits(on.y), bits(off.y))
    lean, _ = both(bs, lambda: bs.plan(*args, obstacle_list=ob, robot_radius=0.2, points=False, **kw))
    assert np.array_equal(lean.hit, want) and lean.x is None                   # points=True and False agree
    if n == 65:
        assert np.sum(want == -1) >= 5 and np.sum(want >= 0) >= 5


def test_control_points_product_and_length_matrix(steers):
    bs = steers["bezier"]
    ob = city(6, 150, 0.0, 30.0, 0.2, 0.6)
    rs = np.random.RandomState(3)
    cps = rs.uniform(0, 30, (40, 1, 2)) + rs.uniform(-4, 4, (40, 5, 2))
    on, off = both(bs, lambda: bs.plan_control_points(cps, n_points=50, obstacle_list=ob, robot_radius=0.1))
    want = ref_hits(on.x, on.y, on.offsets, ob, 0.1)
    assert np.array_equal(on.hit, want) and np.array_equal(off.hit, want) and 0 < np.sum(want == -1) < 40
    d = steers["dubins"]
    st, go = pose_pairs(11, 9, 2.0, 28.0)[0], pose_pairs(12, 7, 2.0, 28.0)[0]
    go = np.concatenate([st[:4] + [1.5, 1.0, 0.3], go[:3]])                   # some goals a short way from a start
    on, off = both(d, lambda: d.plan(st, go, 1.0, points=False, product=True, obstacle_list=ob, robot_radius=0.1))
    assert np.array_equal(on.hit, off.hit) and 0 < np.sum(on.hit == -1) < 63
    assert np.array_equal(bits(on.length_matrix(free_only=True)), bits(off.length_matrix(free_only=True)))


@pytest.mark.parametrize("kind", ["dubins", "rs"])
def test_candidates_and_plan_free(steers, kind):
    bs = steers[kind]
    ob = city(8, 800, smin=0.3, smax=1.0)
    st, go = pose_pairs(21, 50)
    on, off = both(bs, lambda: bs.candidates(st, go, 1.0, obstacle_list=ob, robot_radius=0.15))
    want = ref_hits(on.x, on.y, on.offsets, ob, 0.15)
    assert np.array_equal(on.hit, want) and np.array_equal(off.hit, want) and np.array_equal(on.cand_offsets, off.cand_offsets)
    assert 0 < np.sum(want == -1) < len(want)
    for points in (True, False):
        on, off = both(bs, lambda: bs.plan_free(st, go, 1.0, points=points, obstacle_list=ob, robot_radius=0.15))
        for col in ("hit", "rank", "n_candidates", "n_free", "status"):
            assert np.array_equal(getattr(on, col), getattr(off, col)), col
        assert np.array_equal(bits(on.length), bits(off.length)) and on.rank.max() > 0
        if points:
            assert np.array_equal(on.hit, ref_hits(on.x, on.y, on.offsets, ob, 0.15, on.status))


# ---- shapes ----------------------------------------------------------------------------------------------------------
def line_cps(x0, y0, x1, y1):
    """control points of a straight Bezier curve: the points run from (x0, y0) to (x1, y1)"""
    t = np.linspace(0.0, 1.0, 4)[:, None]
    return (np.array([[x0, y0]]) * (1 - t) + np.array([[x1, y1]]) * t)[None]


def background(m, seed=2):
    """m circles far from the strip y < 20 the test curves run in, centres in [0, 100] x [40, 100]"""
    c = city(seed, m)
    c[:, 1] = 40.0 + 0.6 * c[:, 1]
    return c


def line_hits(bs, cps, n_points, ob, rr=0.0):
    on, off = both(bs, lambda: bs.plan_control_points(cps, n_points=n_points, obstacle_list=ob, robot_radius=rr))
    want = ref_hits(on.x, on.y, on.offsets, ob, rr)
    assert np.array_equal(on.hit, want) and np.array_equal(off.hit, want), (on.hit, off.hit, want)
    lean, _ = both(bs, lambda: bs.plan_control_points(cps, n_points=n_points, points=False, curvature=False, obstacle_list=ob,
                                                      robot_radius=rr))
    assert np.array_equal(lean.hit, want)
    return want


@pytest.mark.parametrize("total", [FILL_TPB - 1, FILL_TPB, FILL_TPB + 1])
def test_point_totals_around_a_fill_workgroup(steers, total):
    ob = background(300)
    ob[299] = (99.0, 5.0, 0.5)                                            # at the very end of the line
    assert line_hits(steers["bezier"], line_cps(0, 5, 99, 5), total, ob).tolist() == [299]
    half = np.concatenate([line_cps(0, 5, 99, 5), line_cps(0, 9, 99, 9)])  # two curves: a wave that spans both at odd totals
    n = total // 2 + 1
    assert line_hits(steers["bezier"], half, n, ob).tolist() == [299, -1]


@pytest.mark.parametrize("where", ["first", "last"])
def test_one_long_curve_over_three_workgroups(steers, where):
    ob = background(300)
    ob[150] = (0.2, 5.0, 0.3) if where == "first" else (99.8, 5.0, 0.3)  # reaches a handful of points of one workgroup only
    cps = line_cps(0, 5, 100, 5)
    want = line_hits(steers["bezier"], cps, 3 * FILL_TPB, ob)
    assert want.tolist() == [150]
    xs = np.linspace(0, 100, 3 * FILL_TPB)
    touched = np.nonzero((xs - ob[150, 0]) ** 2 <= 0.09)[0]
    assert 0 < len(touched) < 8 and (touched.max() < FILL_TPB if where == "first" else touched.min() >= 2 * FILL_TPB)


def test_touched_by_the_last_circle_of_1000_only(steers):
    ob = background(1000)
    ob[999] = (50.0, 5.0, 0.4)
    assert line_hits(steers["bezier"], line_cps(0, 5, 100, 5), 300, ob).tolist() == [999]
    assert line_hits(steers["bezier"], line_cps(0, 9, 100, 9), 300, ob).tolist() == [-1]


@pytest.mark.parametrize("wide_first", [True, False])
def test_wide_circle_against_a_cell_hit(steers, wide_first):
    ob = background(600)
    small, wide = (50.0, 5.0, 0.4), (50.0, 5.0, 30.0)                      # both hold points of the line; the second is in the wide list
    ob[100], ob[400] = (wide, small) if wide_first else (small, wide)
    bs = steers["bezier"]
    assert line_hits(bs, line_cps(0, 5, 100, 5), 300, ob).tolist() == [100]
    info = bs.plan_control_points(line_cps(0, 5, 100, 5), n_points=10, obstacle_list=ob).obstacle_index
    assert info["used"] and info["n_wide"] == 1
    # a curve that only the wide circle reaches, and one that neither reaches
    assert line_hits(bs, line_cps(0, 30, 100, 30), 300, ob).tolist() == [100 if wide_first else 400]


def test_curve_outside_the_box_of_the_centres(steers):
    ob = city(4, 400, 0.0, 10.0, 0.05, 0.2)                               # centres in [0, 10]^2
    ob[:, 0] = np.minimum(ob[:, 0], 9.0)
    ob[77] = (10.0, 5.0, 3.0)                                             # the edge circle: reaches x = 13
    bs = steers["bezier"]
    assert line_hits(bs, line_cps(12.5, -20, 12.5, 30), 200, ob).tolist() == [77]      # wholly outside the box
    assert line_hits(bs, line_cps(13.5, -20, 13.5, 30), 200, ob).tolist() == [-1]
    assert line_hits(bs, line_cps(-50, 5, 60, 5), 500, ob)[0] >= 0                     # enters, crosses and leaves


# ---- the spline objects ------------------------------------------------------------------------------------------------
def test_batch_spline_on_equals_off_equals_the_oracle(gpu):
    import rrt_amd
    courses, ds = spline_util.random_courses(5, 33)
    ob = city(9, 700, -40.0, 60.0, 0.05, 0.3)
    with rrt_amd.BatchSpline() as sp:
        on, off = both(sp, lambda: sp.run(courses, ds=ds, obstacle_list=ob, robot_radius=0.1))
        want = ref_hits(on.x, on.y, on.offsets, ob, 0.1)
        assert np.array_equal(on.hit, want) and np.array_equal(off.hit, want) and 0 < np.sum(want == -1) < 33
        lean, _ = both(sp, lambda: sp.run(courses, ds=ds, obstacle_list=ob, robot_radius=0.1, arrays=False))
        assert np.array_equal(lean.hit, want)
        auto = sp.run(courses, ds=ds, obstacle_list=ob, robot_radius=0.1, arrays=False)
        assert auto.obstacle_index["used"] and np.array_equal(auto.hit, want)
        small = sp.run(courses, ds=ds, obstacle_list=ob[:256], robot_radius=0.1, arrays=False)
        assert small.obstacle_index["reason"] == "below the threshold" and not small.obstacle_index["used"]
        assert sp.run(courses, ds=ds, arrays=False).obstacle_index is None


@pytest.mark.parametrize("call", ["interpolate", "spline2d", "approximate"])
def test_batch_bspline_on_equals_off_equals_the_oracle(gpu, call):
    import rrt_amd
    courses, _, _ = bspline_util.random_courses(7, 21, lo=6)
    ob = city(10, 700, -40.0, 60.0, 0.05, 0.3)
    kw = dict(interpolate=dict(n_path_points=77, degree=3), spline2d=dict(ds=0.3), approximate=dict(n_path_points=77, s=0.5))[call]
    with rrt_amd.BatchBSpline() as b, warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                        # approximate(): a fit that stops early says so
        on, off = both(b, lambda: getattr(b, call)(courses, obstacle_list=ob, robot_radius=0.1, **kw))
        want = ref_hits(on.x, on.y, on.offsets, ob, 0.1)
        assert np.array_equal(on.hit, want) and np.array_equal(off.hit, want) and 0 < np.sum(want == -1) < 21
        lean, _ = both(b, lambda: getattr(b, call)(courses, obstacle_list=ob, robot_radius=0.1, arrays=False, **kw))
        assert np.array_equal(lean.hit, want)


# ---- the life of an object, the fallbacks, the chain ------------------------------------------------------------------
def test_nothing_goes_stale_over_the_life_of_an_object(gpu):
    import rrt_amd
    st, go = pose_pairs(31, 80)
    a, b = city(41, 500, smin=0.3, smax=1.2), city(42, 900, smin=0.3, smax=1.2)
    with rrt_amd.BatchSteer("dubins") as bs:
        def solve(ob, rr):
            res = bs.plan(st, go, 1.0, obstacle_list=ob, robot_radius=rr)
            assert np.array_equal(res.hit, ref_hits(res.x, res.y, res.offsets, ob, rr, res.status))
            return res
        r1 = solve(a, 0.1)
        assert r1.obstacle_index["used"] and r1.obstacle_index["n_circles"] == 500
        OI.assert_index_equals(bs._steer, a, 0.1)
        r2 = solve(b, 0.1)                                                    # another list
        assert r2.obstacle_index["n_circles"] == 900 and not np.array_equal(r1.hit, r2.hit)
        OI.assert_index_equals(bs._steer, b, 0.1)
        r3 = solve(b, 0.6)                                                    # the same list, another radius
        OI.assert_index_equals(bs._steer, b, 0.6)
        assert np.sum(r3.hit >= 0) > np.sum(r2.hit >= 0)
        built = r3.obstacle_index["build_ms"]
        assert solve(b, 0.6).obstacle_index["build_ms"] == built              # the same rows and radius: not built again
        bs.obstacle_index = False
        r4 = solve(b, 0.6)
        assert (r4.obstacle_index["used"], r4.obstacle_index["reason"]) == (False, "off") and np.array_equal(r4.hit, r3.hit)
        bs.obstacle_index = True
        r5 = solve(b, 0.6)
        assert r5.obstacle_index["used"] and np.array_equal(r5.hit, r3.hit)
        r6 = solve(a[:100], 0.1)                                              # ON serves a short list too
        assert r6.obstacle_index["used"] and r6.obstacle_index["n_circles"] == 100
        bs.obstacle_index = None
        r7 = solve(a[:100], 0.1)
        assert r7.obstacle_index["reason"] == "below the threshold" and np.array_equal(r7.hit, r6.hit)
        assert bs.plan(st, go, 1.0).obstacle_index is None                    # no list


@pytest.mark.parametrize("case", ["run too long", "non-finite reach"])
def test_fallbacks_give_the_linear_answer(gpu, case):
    import rrt_amd
    st, go = pose_pairs(51, 40, 2.0, 28.0)
    if case == "run too long":
        ob = np.tile([[float(st[3, 0]), float(st[3, 1]), 0.5]], (5000, 1))   # coincident, on a start pose
    else:
        ob = city(52, 300, 0.0, 30.0, 0.3, 1.0)
        ob[200] = (15.0, 15.0, 1e200)                                         # (size + r) ** 2 is inf: it holds every point
    with rrt_amd.BatchSteer("dubins", obstacle_index=True) as bs:
        res = bs.plan(st, go, 1.0, obstacle_list=ob, robot_radius=0.0)
        assert (res.obstacle_index["used"], res.obstacle_index["reason"], res.obstacle_index["nx"]) == (False, case, 0)
        if case == "run too long":
            want = ref_hits(res.x, res.y, res.offsets, ob[:1], 0.0, res.status)      # 5000 copies of one circle
            assert want[3] == 0
        else:
            want = ref_hits(res.x, res.y, res.offsets, ob[:200], 0.0, res.status)    # circle 200 holds whatever none before it does
            want[want == -1] = 200
            assert np.sum(want == 200) > 0 and np.sum((want >= 0) & (want < 200)) > 0
        assert np.array_equal(res.hit, want)
        with pytest.raises(rrt_amd._abi.RrtxError, match="does not serve"):
            bs._steer.obstacle_index()
    with rrt_amd.BatchSpline(obstacle_index=True) as sp:
        courses, ds = spline_util.random_courses(3, 5)
        assert sp.run(courses, ds=ds, obstacle_list=ob, arrays=False).obstacle_index["reason"] == case


def test_tracker_chain_on_an_indexed_result(steers):
    import rrt_amd
    bs = steers["rs"]
    z = np.load(os.path.join(GOLD, "steer_index_kat.npz"))
    inp, ob = z["r_inp"][:60], z["ob"]
    kw = dict(obstacle_list=[(50.0, 50.0, 1.0)], robot_radius=0.2)
    with rrt_amd.BatchTrack() as bt:
        out = []
        for mode in (True, False):
            bs.obstacle_index = mode
            res = bs.plan(inp[:, 0:3], inp[:, 3:6], 1.0, step_size=0.2, obstacle_list=ob, robot_radius=0.1, points="device")
            assert res.obstacle_index["used"] == mode
            out.append((res.hit.copy(), bt.run(res, select="free", **kw)))
        bs.obstacle_index = None
    (h1, t1), (h2, t2) = out
    assert np.array_equal(h1, h2) and 0 < np.sum(h1 == -1) < 60
    for col in ("find_goal", "length", "fail", "status", "offsets"):
        assert np.array_equal(getattr(t1, col), getattr(t2, col)), col
    assert np.array_equal(bits(t1.t_last), bits(t2.t_last)) and np.array_equal(bits(t1.x), bits(t2.x))
    assert np.sum(t1.status == 5) >= np.sum(h1 >= 0) > 0                      # left out by `select`

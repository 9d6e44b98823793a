"""Pointwise queries of the cubic splines on the GPU (BatchSpline.fit / fit1d / query, rrtx_spline_fit1d / rrtx_spline_query,
the classes of rrt_amd.cubic_spline_path): the reference's recorded answers with c given, the device solve against its
Python definition and against the reference to the measured tolerance, a query at the run's own sample parameters, the CSR
layout with empty rows and a degenerate course over many launch blocks, a course whose run status is REF_RAISES, a handle
used for several fits and queries, and the drop-in classes on the script's driver cells.  Comparisons of doubles are of
uint64 views unless a tolerance is named."""
import numpy as np
import pytest

import spline_oracle
import spline_query_oracle as QO
import spline_query_util as U
import spline_util

pytestmark = pytest.mark.gpu
SAME2 = {k: k for k in QO.PLANES[2]}
SAME1 = {k: k for k in QO.PLANES[1]}


@pytest.fixture(scope="module")
def bs():
    import rrt_amd
    with rrt_amd.BatchSpline() as b:
        yield b


def knots_values():
    return [k for k, _ in U.splines()], [v for _, v in U.splines()]


def test_c_given_is_the_reference_bit_for_bit(bs):
    """Every plane and every status of the golden, 2-D and 1-D: with -0.0, every knot and its neighbours, the last knot,
    the infinities and NaN among the parameters"""
    import rrt_amd
    g = U.kat()
    fit = bs.fit(U.courses(), c=(g["cx"], g["cy"]))
    assert not np.any(fit.status == rrt_amd._abi.SPLINE_DEGENERATE) and fit.x is None
    q = bs.query((g["q_off"], g["q_t"]), derivatives=True)
    assert q.rc == rrt_amd._abi.RRTX_PARTIAL and np.array_equal(U.bits(q.s), U.bits(g["q_t"])) and np.array_equal(q.offsets, g["q_off"])
    U.assert_planes(q, g, "2-D, c given", U.KEYS2, "q_status")
    assert np.array_equal(q.valid, g["q_status"] == 0)
    plain = bs.query((g["q_off"], g["q_t"]))
    assert plain.dx is None and plain.dy is None and plain.ddx is None and plain.ddy is None
    U.assert_planes(plain, g, "2-D, c given, no derivatives", {k: U.KEYS2[k] for k in ("x", "y", "yaw", "k")}, "q_status")
    # the list form is the same batch
    rows = bs.query([t for (t,) in U._rows(g["q_off"], g["q_t"])], derivatives=True)
    U.assert_planes(rows, g, "2-D, list form", U.KEYS2, "q_status")

    kn, va = knots_values()
    fit = bs.fit1d(kn, va, c=g["c1"])
    assert fit.rc == 0 and np.all(fit.n_points == 0) and fit.total_length.tolist() == [k[-1] for k in kn]
    assert np.array_equal(U.bits(fit.c[0]), U.bits(g["c1"])) and fit.c[1] is None
    q = bs.query((g["p_off"], g["p_t"]), derivatives=True)
    assert q.x is None and q.yaw is None and q.k is None and q.dx is None
    U.assert_planes(q, g, "1-D, c given", U.KEYS1, "p_status")
    plain = bs.query((g["p_off"], g["p_t"]))
    assert plain.dy is None and plain.ddy is None
    U.assert_planes(plain, g, "1-D, c given, no derivatives", {"y": "p_y"}, "p_status")


def test_device_solve_is_the_thomas_oracle_and_close_to_the_reference(bs):
    g = U.kat()
    bs.fit(U.courses())
    two = bs.query((g["q_off"], g["q_t"]), derivatives=True)
    U.assert_planes(two, U.oracle2("thomas"), "2-D, device solve", SAME2)
    kn, va = knots_values()
    fit = bs.fit1d((g["k_off"], g["knots"]), (g["k_off"], g["values"]))   # the CSR form
    assert np.array_equal(U.bits(fit.c[0]), U.bits(np.concatenate([QO.fit1d(k, v)["c"][0] for k, v in zip(kn, va)])))
    one = bs.query((g["p_off"], g["p_t"]), derivatives=True)
    U.assert_planes(one, U.oracle1("thomas"), "1-D, device solve", SAME1)
    # against the reference: the statuses exact, the values to the measured tolerance
    assert np.array_equal(two.status, g["q_status"]) and np.array_equal(one.status, g["p_status"])
    gap = U.gaps(two, one)
    print("device solve against the reference: position %.3e yaw %.3e k %.3e first %.3e second %.3e" % gap)
    for got, tol in zip(gap, (U.TOL_POS, U.TOL_YAW, U.TOL_K, U.TOL_D1, U.TOL_D2)):
        assert got <= tol, gap


def test_numpy_solve_is_the_oracle_with_numpys_solve(bs):
    """The exact mode: np.linalg.solve in this process on both sides"""
    g = U.kat()
    bs.fit(U.courses(), solve="numpy")
    U.assert_planes(bs.query((g["q_off"], g["q_t"]), derivatives=True), U.oracle2("numpy"), "2-D, numpy solve", SAME2)
    kn, va = knots_values()
    bs.fit1d(kn, va, solve="numpy")
    U.assert_planes(bs.query((g["p_off"], g["p_t"]), derivatives=True), U.oracle1("numpy"), "1-D, numpy solve", SAME1)


def test_query_at_the_runs_own_parameters_is_the_run(bs):
    """No golden: after run(courses, ds) with arrays, query at k * ds returns the run's x, y, yaw, k"""
    courses, ds = spline_util.random_courses(31, 40)
    res = bs.run(courses, ds=ds)
    assert res.rc == 0 and res.offsets[-1] > 4000
    q = bs.query((res.offsets, res.s))
    assert q.rc == 0 and np.all(q.status == 0)
    for key in ("x", "y", "yaw", "k"):
        assert np.array_equal(U.bits(getattr(q, key)), U.bits(getattr(res, key))), key


@pytest.fixture(scope="module")
def layout():
    """131 seeded courses, the one in the middle degenerate; query counts cycle through 0, 1, 63, 64, 65, 300 with the first
    and the last row empty and 65 on the degenerate course; parameters from below the first knot to beyond the last, the
    ends among them.  -> (courses, q_off, t, the oracle's answers)"""
    courses, _ = spline_util.random_courses(131, 131)
    x, y = courses[65]
    courses[65] = (np.concatenate([x[:2], x[1:]]), np.concatenate([y[:2], y[1:]]))   # waypoint 1 twice
    counts = [(0, 1, 63, 64, 65, 300)[i % 6] for i in range(131)]
    counts[65], counts[130] = 65, 0
    rs = np.random.RandomState(77)
    ts = []
    for (x, y), m in zip(courses, counts):
        end = spline_oracle.knots(x.tolist(), y.tolist())[-1]
        t = rs.uniform(-0.5, end + 0.5, m)
        if m >= 63:
            t[:3] = 0.0, end, np.nextafter(end, 0.0)
        ts.append(t)
    q_off = np.zeros(132, dtype=np.int64)
    q_off[1:] = np.cumsum(counts)
    t = np.concatenate(ts)
    fits = [QO.fit2d(x, y) for x, y in courses]
    return courses, q_off, t, QO.batch(fits, q_off, t)


@pytest.mark.parametrize("derivatives", [False, True])
def test_layout_empty_rows_and_a_degenerate_course(bs, layout, derivatives):
    import rrt_amd
    A = rrt_amd._abi
    courses, q_off, t, want = layout
    assert q_off[1] == 0 and q_off[-1] == q_off[-2] and q_off[-1] > 30 * 256 and {2, 40} <= {len(c[0]) for c in courses}
    assert np.any(np.diff(q_off) % 64 != 0)   # waves straddle courses
    fit = bs.fit(courses)
    assert fit.rc == A.RRTX_PARTIAL and fit.status[65] == A.SPLINE_DEGENERATE and np.sum(fit.status == A.SPLINE_DEGENERATE) == 1
    q = bs.query((q_off, t), derivatives=derivatives)
    assert q.rc == A.RRTX_PARTIAL
    mine = q.of(65)
    assert len(mine["s"]) == 65 and np.all(mine["status"] == A.SPLINE_Q_NO_SPLINE) and np.all(np.isnan(mine["x"]))
    assert {A.SPLINE_Q_OK, A.SPLINE_Q_OUTSIDE, A.SPLINE_Q_REF_RAISES, A.SPLINE_Q_NO_SPLINE} == set(q.status.tolist())
    names = SAME2 if derivatives else {k: k for k in ("x", "y", "yaw", "k")}
    U.assert_planes(q, want, "layout", names)
    assert (q.dx is None) == (not derivatives)
    assert q.of(0)["s"].size == 0 and q.of(130)["x"].size == 0 and q.of(5)["x"].size == 300


def test_a_course_whose_run_status_is_ref_raises_answers(bs):
    """Three waypoints on a line with s[-1] = 0.1 + 0.2 and ds = 0.1: the fourth sample 3 * 0.1 rounds onto the last knot, so
    the run has no points (REF_RAISES) -- which speaks about ds, not about the fit: the spline is there and answers.  (The
    [0, 1, 2, 3] line with ds = 0.5 of spline_kat.npz keeps its stop out and is an OK run of 6 points; it answers as well.)"""
    import rrt_amd
    A = rrt_amd._abi
    x, y = [0.0, 0.1, 0.30000000000000004], [0.0, 0.0, 0.0]
    assert spline_oracle.spline_course(x, y, 0.1)["status"] == spline_oracle.REF_RAISES
    res = bs.run([(x, y)], ds=0.1)
    assert res.rc == A.RRTX_PARTIAL and res.status.tolist() == [A.SPLINE_REF_RAISES] and res.n_points.tolist() == [0]
    end = res.total_length[0]
    t = np.array([0.0, 0.05, 0.1, 0.25, np.nextafter(end, 0.0), end])
    q = bs.query(t, derivatives=True)
    assert q.status.tolist() == [0, 0, 0, 0, 0, A.SPLINE_Q_REF_RAISES] and q.rc == A.RRTX_PARTIAL
    U.assert_planes(q, QO.batch([QO.fit2d(x, y)], [0, 6], t), "REF_RAISES course", SAME2)
    assert np.allclose(q.x[:5], t[:5], rtol=0, atol=1e-15) and not np.any(q.y[:5]) and not np.any(q.yaw[:5])
    x, y = [0.0, 1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0]
    ok = bs.run([(x, y)], ds=0.5)
    assert ok.status.tolist() == [0] and ok.n_points.tolist() == [6]
    t = np.array([0.0, 0.5, 2.5, np.nextafter(3.0, 0.0), 3.0])
    q = bs.query(t, derivatives=True)
    assert q.status.tolist() == [0, 0, 0, 0, A.SPLINE_Q_REF_RAISES]
    U.assert_planes(q, QO.batch([QO.fit2d(x, y)], [0, 5], t), "the golden's line", SAME2)


def test_one_handle_several_fits_and_queries():
    import rrt_amd
    A = rrt_amd._abi
    courses, _ = spline_util.random_courses(5, 6, 3, 9)
    fits = [QO.fit2d(x, y) for x, y in courses]
    rs = np.random.RandomState(3)
    small = rs.uniform(0.0, 3.0, 7)
    large = rs.uniform(-1.0, 8.0, 1000)
    kn, va = [np.arange(5), [0.0, 0.5, 2.0]], [[1.7, -6, 5, 6.5, 0.0], [1.0, -1.0, 0.5]]
    with rrt_amd.BatchSpline() as h:
        with pytest.raises(A.RrtxError, match="RRTX_E_STATE"):
            h.query(small)
        h.fit(courses)
        a = h.query(small)                 # one array for every spline
        b = h.query(large, derivatives=True)
        off2, t2 = np.array([0, 1, 2], dtype=np.int64), np.zeros(2)
        with pytest.raises(A.RrtxError, match="number of splines"):   # n is 2, the fit has 6 splines
            h._spline.query(A.SplineQueryBatch(n=2, q_offsets=off2.ctypes.data, t=t2.ctypes.data, want_derivatives=0, reserved=0))
        with pytest.raises(ValueError):
            h.query([small] * 5)
        fit = h.fit1d(kn, va)
        c = h.query([np.linspace(0.0, 5.0), np.array([0.25, 2.0, -0.0])], derivatives=True)
        e = h.query([[], []])              # Q == 0
        e2 = h.query(np.zeros(0))
    assert a.offsets.tolist() == [0, 7, 14, 21, 28, 35, 42] and b.offsets[-1] == 6000
    U.assert_planes(a, QO.batch(fits, a.offsets, a.s), "first query", {k: k for k in ("x", "y", "yaw", "k")})
    U.assert_planes(b, QO.batch(fits, b.offsets, b.s), "second, larger query", SAME2)
    assert fit.rc == 0 and fit.total_length.tolist() == [4.0, 2.0]
    U.assert_planes(c, QO.batch([QO.fit1d(k, v) for k, v in zip(kn, va)], c.offsets, c.s), "after fit1d", SAME1)
    assert c.status[-1] == 0 and c.status[:50].tolist() == [0] * 40 + [A.SPLINE_Q_OUTSIDE] * 10   # 40 * 5 / 49 > 4
    for empty in (e, e2):
        assert empty.rc == 0 and empty.status.size == 0 and empty.y.size == 0 and empty.offsets.tolist() == [0, 0, 0]


def test_fit1d_degenerate_and_refusals(bs):
    import rrt_amd
    A = rrt_amd._abi
    fit = bs.fit1d([[0.0, 1.0, 1.0, 2.0], [0.0, 1.0, 2.0]], [[0.0, 1.0, 2.0, 3.0], [1.0, 0.0, 1.0]])
    assert fit.rc == A.RRTX_PARTIAL and fit.status.tolist() == [A.SPLINE_DEGENERATE, 0] and not np.any(fit.c[0][:4])
    q = bs.query([[0.5, 1.5], [0.5, 1.5]])
    assert q.status.tolist() == [A.SPLINE_Q_NO_SPLINE] * 2 + [0, 0] and np.all(np.isnan(q.y[:2])) and q.rc == A.RRTX_PARTIAL
    U.assert_planes(q, QO.batch([QO.fit1d([0.0, 1.0, 1.0, 2.0], [0.0, 1.0, 2.0, 3.0]), QO.fit1d([0.0, 1.0, 2.0], [1.0, 0.0, 1.0])],
                                q.offsets, q.s), "degenerate 1-D", {"y": "y"})
    with pytest.raises(A.RrtxError, match="spline 1.*ascending"):
        bs.fit1d([[0.0, 1.0], [0.0, 2.0, 1.0]], [[0.0, 1.0], [0.0, 1.0, 2.0]])
    with pytest.raises(A.RrtxError, match="RRTX_E_STATE"):   # a refused fit leaves no splines behind the Python object
        bs.query([[0.5], [0.5]])


def test_dropin_classes_on_the_scripts_driver_cells(bs):
    """CubicSpline1D on np.linspace(0.0, 5.0) with its None tail, CubicSpline2D in the script's loop: the exact mode
    (np.linalg.solve in this process) against the oracle bit for bit, against the golden to the tolerance, and the reference's
    exceptions"""
    import rrt_amd
    import rrt_amd.cubic_spline_path as cs
    g = U.kat()
    x = np.arange(5)
    y = [1.7, -6, 5, 6.5, 0.0]
    sp = cs.CubicSpline1D(x, y)
    xi = np.linspace(0.0, 5.0)
    yi = [sp.calc_position(v) for v in xi]
    assert np.array_equal(U.bits(xi), U.bits(g["drv_t"]))
    none = np.isnan(g["drv_y"])
    assert [v is None for v in yi] == none.tolist() and none[-1] and not none[0]
    got = np.array([np.nan if v is None else v for v in yi])
    assert np.nanmax(np.abs(got - g["drv_y"])) <= U.TOL_POS
    f = QO.fit1d(x, y, "numpy")
    want = QO.batch([f], [0, len(xi)], xi)
    assert np.array_equal(U.bits(got[~none]), U.bits(want["y"][~none]))
    assert np.array_equal(U.bits(sp.c), U.bits(f["c"][0])) and np.array_equal(U.bits(sp.b), U.bits(f["b"][0]))
    assert np.array_equal(U.bits(sp.d), U.bits(f["d"][0])) and sp.a == y and sp.nx == 5 and sp.x is x and sp.y is y
    # the array form: one call, NaN where the scalar form returns None or raises
    arr = sp.calc_position(xi)
    assert np.array_equal(np.isnan(arr), none) and np.array_equal(U.bits(arr[~none]), U.bits(got[~none]))
    assert np.array_equal(U.bits(sp.calc_first_derivative(xi)[~none]), U.bits(want["dy"][~none]))
    assert np.isnan(sp.calc_second_derivative(np.array([4.0, np.nan, -1.0]))).all()
    assert sp.calc_position(-0.0) == 1.7 and sp.calc_position(-1e-300) is None and sp.calc_second_derivative(9.0) is None
    for bad in (4.0, float("nan")):
        for fn in (sp.calc_position, sp.calc_first_derivative, sp.calc_second_derivative):
            with pytest.raises(IndexError, match="list index out of range"):
                fn(bad)
    with pytest.raises(ValueError, match="x coordinates must be sorted in ascending order"):
        cs.CubicSpline1D([0.0, 2.0, 1.0], y[:3])

    # the 2-D cell, as the script writes it
    x = [-2.5, 0.0, 2.5, 5.0, 7.5, 3.0, -1.0]
    y = [0.7, -6, 5, 6.5, 0.0, 5.0, -2.0]
    ds = 0.1
    sp2 = cs.CubicSpline2D(x, y)
    s = np.arange(0, sp2.s[-1], ds)
    rx, ry, ryaw, rk = [], [], [], []
    for i_s in s:
        ix, iy = sp2.calc_position(i_s)
        rx.append(ix)
        ry.append(iy)
        ryaw.append(sp2.calc_yaw(i_s))
        rk.append(sp2.calc_curvature(i_s))
    o = spline_oracle.spline_course(x, y, ds, "numpy")
    for got, key in ((rx, "rx"), (ry, "ry"), (ryaw, "ryaw"), (rk, "rk"), (s, "s")):
        assert np.array_equal(U.bits(got), U.bits(o[key])), key
    k = spline_util.kat()
    i = [j for j, (cx_, _) in enumerate(spline_util.courses()) if cx_.tolist() == x][0]
    a, b = k["pt_off"][i], k["pt_off"][i + 1]
    assert k["ds"][i] == ds and np.max(np.abs(np.array(rx) - k["rx"][a:b])) <= spline_util.TOL_XY
    assert np.max(np.abs(np.array(rk) - k["rk"][a:b]) / np.maximum(1.0, np.abs(k["rk"][a:b]))) <= spline_util.TOL_K
    # the sample cell again: another object has used the handle since, the first one still answers
    assert sp.calc_position(xi[3]) == yi[3]
    assert np.array_equal(U.bits(sp2.s), U.bits(o["knots"])) and np.array_equal(U.bits(sp2.sx.c), U.bits(o["cx"]))
    assert sp2.sx.x is sp2.s and sp2.sy.y is y and len(sp2.ds) == 6
    t = s[17]
    f2 = QO.fit2d(x, y, "numpy")
    w = QO.query(f2, t)[1]
    assert sp2.sx.calc_first_derivative(t) == w["dx"] and sp2.sy.calc_second_derivative(t) == w["ddy"]
    assert sp2.sy.calc_position(t) == w["y"] and sp2.sx.calc_position(1e9) is None
    end = sp2.s[-1]
    assert sp2.calc_position(-1.0) == (None, None) and sp2.calc_position(np.nextafter(end, np.inf)) == (None, None)
    for fn in (sp2.calc_yaw, sp2.calc_curvature):
        with pytest.raises(TypeError):
            fn(-1.0)
        with pytest.raises(IndexError, match="list index out of range"):
            fn(end)
    with pytest.raises(IndexError):
        sp2.calc_position(float("nan"))
    px, py = sp2.calc_position(np.array([0.0, end, -1.0, 1.0]))
    assert np.isnan(px).tolist() == [False, True, True, False] and px[0] == -2.5 and py[0] == 0.7
    assert np.isnan(sp2.calc_yaw(np.array([end]))).all() and np.isnan(sp2.calc_curvature(np.array([np.inf]))).all()
    with pytest.raises(rrt_amd._abi.RrtxError):
        cs.CubicSpline2D([0.0, 1.0, 1.0], [0.0, 0.0, 0.0])

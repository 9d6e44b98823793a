"""Batched cubic-spline courses on the GPU (BatchSpline, rrtx_spline_*): the reference's recorded courses with c given, the
device solve against its Python definition and against the reference to the measured tolerance, the exact mode, a batch
over many launch blocks, a degenerate course, the collision check, a handle used twice, the hand-over to BatchTrack and
the drop-in function.  Comparisons of doubles are of uint64 views unless a tolerance is named."""
import numpy as np
import pytest

import spline_oracle
import spline_util as U

pytestmark = pytest.mark.gpu
ARRAYS = ("x", "y", "yaw", "k", "s")


@pytest.fixture(scope="module")
def bs():
    import rrt_amd
    with rrt_amd.BatchSpline() as b:
        yield b


@pytest.fixture(scope="module")
def flat_c():
    g = U.kat()
    return g["cx"], g["cy"]


def assert_records(res, want, what):
    assert np.array_equal(res.status, want["status"]), what
    assert np.array_equal(res.n_points, want["n_points"]), what
    assert np.array_equal(U.bits(res.total_length), U.bits(want["total_length"])), what
    assert np.array_equal(res.offsets, want["offsets"]), what


def test_c_given_is_the_reference_bit_for_bit(bs, flat_c):
    """All golden courses in one batch: 65 courses (no multiple of 64) of 2 .. 200 waypoints, a ds per course"""
    g = U.kat()
    assert len(g["ds"]) % 64 != 0 and len(set(g["ds"].tolist())) > 1
    res = bs.run(U.courses(), ds=g["ds"], c=flat_c)
    assert res.rc == 0 and np.all(res.status == 0)
    assert np.array_equal(res.offsets, g["pt_off"]) and np.array_equal(U.bits(res.total_length), U.bits(g["length"]))
    for key, gk in zip(ARRAYS, ("rx", "ry", "ryaw", "rk", "s")):
        assert np.array_equal(U.bits(getattr(res, key)), U.bits(g[gk])), key
    assert np.array_equal(U.bits(res.c[0]), U.bits(g["cx"])) and np.array_equal(U.bits(res.c[1]), U.bits(g["cy"]))
    # the CSR form and the (n_i, 2) arrays are the same batch
    csr = bs.run((g["wp_off"], g["wp_x"], g["wp_y"]), ds=g["ds"], c=flat_c)
    rows = bs.run([np.stack([x, y], axis=1) for x, y in U.courses()], ds=g["ds"], c=flat_c)
    for other in (csr, rows):
        U.assert_same(other, dict(offsets=res.offsets, **{k: getattr(res, k) for k in ARRAYS}), "waypoint form")


def test_device_solve_is_the_thomas_oracle_and_close_to_the_reference(bs):
    g, o = U.kat(), U.oracle("thomas")
    res = bs.run(U.courses(), ds=g["ds"])
    assert res.rc == 0
    assert_records(res, o, "device solve")
    U.assert_same(res, o, "device solve")
    assert np.array_equal(U.bits(res.c[0]), U.bits(np.concatenate(o["cx"])))
    assert np.array_equal(U.bits(res.c[1]), U.bits(np.concatenate(o["cy"])))
    # against the reference: counts and s exact, the rest to the measured tolerance
    assert np.array_equal(res.offsets, g["pt_off"]) and np.array_equal(U.bits(res.s), U.bits(g["s"]))
    gap = U.gaps(res.x, res.y, res.yaw, res.k)
    print("device solve against the reference: xy %.3e yaw %.3e k %.3e" % gap)
    assert gap[0] <= U.TOL_XY and gap[1] <= U.TOL_YAW and gap[2] <= U.TOL_K, gap


def test_numpy_solve_is_the_oracle_with_numpys_solve(bs):
    """The exact mode: np.linalg.solve in this process on both sides"""
    g = U.kat()
    res = bs.run(U.courses(), ds=g["ds"], solve="numpy")
    o = spline_oracle.batch(U.courses(), g["ds"], "numpy")
    assert res.rc == 0
    assert_records(res, o, "numpy solve")
    U.assert_same(res, o, "numpy solve")


def test_batch_over_many_blocks_and_records_only(bs):
    """About 300 random courses of 2 .. 40 waypoints (three blocks of the fit kernel, a few hundred of the evaluation)"""
    courses, ds = U.random_courses(2025, 301)
    o = spline_oracle.batch(courses, ds, "thomas")
    assert 2.0e4 < o["offsets"][-1] < 1.2e5 and {2, 40} <= {len(c[0]) for c in courses}
    res = bs.run(courses, ds=ds)
    assert res.rc == 0
    assert_records(res, o, "random batch")
    U.assert_same(res, o, "random batch")
    rec = bs.run(courses, ds=ds, arrays=False)
    assert_records(rec, o, "records only")
    assert rec.x is None and rec.y is None and rec.yaw is None and rec.k is None and rec.s is None


def test_degenerate_course_in_the_middle(bs):
    import rrt_amd
    A = rrt_amd._abi
    courses, ds = U.random_courses(7, 9, 3, 12)
    x, y = courses[4]
    bad = list(courses)
    bad[4] = (np.concatenate([x[:2], x[1:]]), np.concatenate([y[:2], y[1:]]))   # waypoint 1 twice
    res = bs.run(bad, ds=ds, obstacle_list=[(0.0, 0.0, 1.0)])
    assert res.rc == A.RRTX_PARTIAL
    assert res.status.tolist() == [0] * 4 + [A.SPLINE_DEGENERATE] + [0] * 4
    assert res.n_points[4] == 0 and res.offsets[4] == res.offsets[5] and res.hit[4] == -2
    assert not np.any(res.c[0][res.wp_offsets[4]:res.wp_offsets[5]])
    with pytest.raises(A.RrtxError):
        res.course(4)
    without = bs.run(courses[:4] + courses[5:], ds=np.delete(ds, 4))
    assert without.rc == 0
    assert np.array_equal(np.delete(res.offsets, 4), without.offsets)
    for k in ARRAYS:
        assert np.array_equal(U.bits(getattr(res, k)), U.bits(getattr(without, k))), k


def test_hits_are_the_references(bs, flat_c):
    g = U.kat()
    obs, rr = [tuple(r) for r in g["obs"].tolist()], float(g["rr"])
    res = bs.run(U.courses(), ds=g["ds"], c=flat_c, obstacle_list=obs, robot_radius=rr)
    sel = g["hit_courses"]
    assert np.array_equal(res.hit[sel], g["hit"])
    assert np.array_equal(res.free[sel], g["hit"] == -1)
    assert [res.is_free(int(i)) for i in sel] == (g["hit"] == -1).tolist()
    assert res.hit[int(g["lone"][0])] == len(obs) - 1     # touched by the last circle only, at one point
    rec = bs.run(U.courses(), ds=g["ds"], c=flat_c, obstacle_list=obs, robot_radius=rr, arrays=False)
    assert rec.x is None and np.array_equal(rec.hit, res.hit)
    # every course of the batch, against the oracle's check on the reference's points
    o = U.oracle("given")
    want = [spline_oracle.first_hit(p["rx"], p["ry"], obs, rr) for p in o["per_course"]]
    assert res.hit.tolist() == want
    assert bs.run(U.courses(), ds=g["ds"], c=flat_c).hit is None


def test_one_handle_twice_the_second_batch_larger():
    import rrt_amd
    small, ds_s = U.random_courses(11, 5, 2, 6)
    large, ds_l = U.random_courses(12, 70, 10, 40)
    obs = [(0.0, 0.0, 2.0), (5.0, 5.0, 1.0)]
    with rrt_amd.BatchSpline() as h:
        a = h.run(small, ds=ds_s, obstacle_list=obs)
        b = h.run(large, ds=ds_l, obstacle_list=obs)
    assert b.offsets[-1] > 8 * a.offsets[-1]
    for got, (courses, ds) in ((a, (small, ds_s)), (b, (large, ds_l))):
        with rrt_amd.BatchSpline() as fresh:
            want = fresh.run(courses, ds=ds, obstacle_list=obs)
        U.assert_same(got, dict(offsets=want.offsets, **{k: getattr(want, k) for k in ARRAYS}), "reused handle")
        assert np.array_equal(got.hit, want.hit) and np.array_equal(got.status, want.status)
        assert np.array_equal(U.bits(got.c[0]), U.bits(want.c[0]))
        U.assert_same(got, spline_oracle.batch(courses, ds, "thomas"), "reused handle against the oracle")


def test_tracker_takes_a_spline_result(bs):
    import rrt_amd
    courses, _ = U.random_courses(3, 3, 5, 9)
    res = bs.run(courses, ds=0.1)
    assert np.all(np.diff(res.offsets) <= 960) and np.all(np.diff(res.offsets) >= 3)
    with rrt_amd.BatchTrack() as bt:
        direct = bt.run(res)
        trip = [tuple(q[res.offsets[i]:res.offsets[i + 1]] for q in (res.x, res.y, res.yaw)) for i in range(3)]
        listed = bt.run(trip)
    for f in ("find_goal", "length", "fail", "status"):
        assert np.array_equal(getattr(direct, f), getattr(listed, f)), f
    assert np.array_equal(U.bits(direct.t_last), U.bits(listed.t_last)) and np.array_equal(direct.offsets, listed.offsets)
    for k in ("x", "y", "yaw", "v", "t", "a", "d"):
        assert np.array_equal(U.bits(getattr(direct, k)), U.bits(getattr(listed, k))), k
    assert np.all(direct.status == 0) and direct.steps > 0


def test_dropin_function_is_a_numpy_solve_batch_of_one(bs):
    import rrt_amd.cubic_spline_path as cs
    x = [-2.5, 0.0, 2.5, 5.0, 7.5, 3.0, -1.0]
    y = [0.7, -6, 5, 6.5, 0.0, 5.0, -2.0]
    got = cs.calc_spline_course(x, y, ds=0.1)
    want = bs.run([(x, y)], ds=0.1, solve="numpy").course(0)
    assert len(got) == 5 and all(isinstance(q, list) for q in got)
    for a, b in zip(got, want):
        assert np.array_equal(U.bits(a), U.bits(b))
    o = spline_oracle.spline_course(x, y, 0.1, "numpy")
    assert np.array_equal(U.bits(got[0]), U.bits(o["rx"])) and np.array_equal(U.bits(got[3]), U.bits(o["rk"]))

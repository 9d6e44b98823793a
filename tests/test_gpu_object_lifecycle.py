"""The seven device objects besides the planner handle on the GPU (Steer, Tracker, Spline, BSpline, ArmNav, ArmIK, ArmDH): the
lifecycle they share (create, context manager, two alive at once), what a fresh object answers, and for each the smallest
legal run read back through the getters that copy from the device.  Every expected result is the one the object's own GPU
test states for that input, through that test's helpers and golden data; nothing here is a new oracle.

The tracker's golden data hold no course shorter than 17 points, so the golden check runs the shortest of them; a
three-point course is tracked as well, and must come out the same, bit for bit, from two trackers alive side by side."""
import os

import numpy as np
import pytest

import armdh_util
import armik_util
import armnav_util
import bspline_oracle
import bspline_util
import spline_oracle
import spline_util
import test_gpu_armdh
import test_gpu_armik
import test_gpu_armnav
import test_gpu_spline
import test_gpu_track_batch
import track_util
import util
from test_track_batch_host import kat_vectors

pytestmark = pytest.mark.gpu
OBJECTS = ("steer", "tracker", "spline", "bspline", "armnav", "armik", "armdh")


def abi():
    import rrt_amd
    return rrt_amd._abi


def state_error(call, fn, text):
    """`call` raises what a getter raises before its run: RRTX_E_STATE under the getter's name"""
    with pytest.raises(abi().RrtxError) as e:
        call()
    assert str(e.value).startswith("%s: RRTX_E_STATE %s: %s" % (fn, fn, text)), str(e.value)


def fresh(prefix, o):
    """What a just-created object answers to the getters that need no run (csrc/rrtx_api_<prefix>.inc)"""
    if prefix == "steer":
        assert o.generation() == 0 and o.n_obstacles == 0
        state_error(o.kernel_ms, "rrtx_steer_get_kernel_ms", "no completed solve")
    elif prefix == "tracker":
        state_error(o.kernel_ms, "rrtx_tracker_get_kernel_ms", "no completed run")
    elif prefix in ("spline", "bspline"):
        assert o.generation() == 0
    elif prefix == "armnav":
        assert o.kernel_ms() == (0.0, 0.0)
    else:   # armik, armdh: no time, no waves
        assert o.kernel_ms() == (0.0, 0)


@pytest.mark.parametrize("prefix", OBJECTS)
def test_create_close_and_two_alive_at_once(gpu, prefix):
    A = abi()
    cls = {c._prefix: c for c in (A.Steer, A.Tracker, A.Spline, A.BSpline, A.ArmNav, A.ArmIK, A.ArmDH)}[prefix]
    with cls() as a:
        assert a._s.value
        with cls(device=0) as b:
            assert b._s.value and b._s.value != a._s.value
            fresh(prefix, b)
        assert not b._s
        fresh(prefix, a)   # the other's end took nothing from this one
    assert not a._s
    a.close()
    c = cls()
    c.close()
    c.close()
    assert not c._s


def test_steer_one_pair_with_points(gpu):
    import rrt_amd
    g = np.load(os.path.join(util.ROOT, "tests", "golden", "dubins_kat.npz"))
    k = 0
    lo = int(np.sum(g["n"][:k]))
    with rrt_amd.BatchSteer("dubins") as s:
        res = s.plan(g["inp"][k:k + 1, 0:3], g["inp"][k:k + 1, 3:6], 1.0)
        assert s._steer.generation() == 1 and s._steer.kernel_ms() == res.kernel_ms > 0.0
    n = int(g["n"][k])
    assert res.rc == 0 and len(res) == 1 and res.offsets.tolist() == [0, n] and int(res.status[0]) == 0
    assert np.array_equal(res.x, g["poly_x"][lo:lo + n]) and np.array_equal(res.y, g["poly_y"][lo:lo + n])
    assert np.array_equal(res.seg_len[:, :3], g["lengths"][k:k + 1]) and int(res.n_seg[0]) == 3
    assert res.modes == [str(g["mode"][k])]
    assert res.yaw[-1] == g["end"][k, 2] and res.x[-1] == g["end"][k, 0]
    ln = g["lengths"][k]
    assert res.length[0] == abs(ln[0]) + abs(ln[1]) + abs(ln[2])


def test_tracker_shortest_golden_course_and_a_three_point_course(gpu):
    import rrt_amd
    g = np.load(os.path.join(track_util.GOLD, "track_kat.npz"))
    g = {k: g[k] for k in g.files}
    vecs = kat_vectors(g)
    i = min(range(len(vecs)), key=lambda j: len(vecs[j][3]))
    assert len(vecs[i][3]) == 17
    course = (np.array([0.0, 1.0, 2.0]), np.array([0.0, 0.0, 0.5]), np.array([0.0, 0.0, 0.4]))
    with rrt_amd.BatchTrack() as a, rrt_amd.BatchTrack() as b:
        res = test_gpu_track_batch.run_vectors(a, [vecs[i]])
        assert len(res) == 1 and res.rc == 0 and a._tracker.kernel_ms() == res.kernel_ms > 0.0
        test_gpu_track_batch.assert_vector(res, 0, g, i)
        one, two = a.run([course]), b.run([course])
    assert len(one) == 1 and one.offsets.tolist() == [0, len(one.x)] and one.steps == len(one.x)
    test_gpu_track_batch.assert_same_records(one, two, "two trackers")
    test_gpu_track_batch.assert_same_arrays(one, two, "two trackers")


def test_spline_one_course_of_three_waypoints(gpu):
    import rrt_amd
    g = spline_util.kat()
    k = 3
    course, ds = spline_util.courses()[k], g["ds"][k:k + 1]
    assert len(course[0]) == 3
    want = spline_oracle.batch([course], ds, "thomas")
    with rrt_amd.BatchSpline() as s:
        res = s.run([course], ds=ds)
        assert s._spline.generation() == 1
    assert res.rc == 0
    test_gpu_spline.assert_records(res, want, "three waypoints")
    spline_util.assert_same(res, want, "three waypoints")
    assert np.array_equal(spline_util.bits(res.c[0]), spline_util.bits(np.concatenate(want["cx"])))
    assert np.array_equal(spline_util.bits(res.c[1]), spline_util.bits(np.concatenate(want["cy"])))
    # the reference's own course: counts and s exact
    lo, hi = g["pt_off"][k], g["pt_off"][k + 1]
    assert int(res.n_points[0]) == hi - lo and np.array_equal(spline_util.bits(res.s), spline_util.bits(g["s"][lo:hi]))


def test_bspline_one_course_of_three_waypoints(gpu):
    import rrt_amd
    g = bspline_util.kat()
    crs, kw, okw = bspline_util.run_kwargs(0)
    j = 3   # the golden course 3 of bspline_path: three waypoints, degree 2
    assert len(crs[j][0]) == 3 and int(kw["degree"][j]) == 2
    cut = lambda v: v[j:j + 1]
    want = bspline_oracle.batch([crs[j]], degree=cut(okw["degree"]), param=okw["param"], n_path_points=cut(okw["n_path_points"]),
                                u=cut(okw["u"]))
    with rrt_amd.BatchBSpline() as b:
        res = b.interpolate([crs[j]], cut(kw["n_path_points"]), degree=cut(kw["degree"]), u=cut(kw["u"]))
        assert b._bs.generation() == 1 and res.kernel_ms > 0.0
    assert res.rc == 0 and int(res.status[0]) == 0
    bspline_util.assert_same(res, want, "three waypoints")
    i = int(bspline_util.select(0)[j])
    assert int(res.n_points[0]) == g["pt_off"][i + 1] - g["pt_off"][i]
    assert np.array_equal(bspline_util.bits(res.u), bspline_util.bits(bspline_util.gold([i], "ru")))


def test_armnav_one_query_on_a_two_by_two_grid(gpu):
    import rrt_amd
    M = 2
    q = next(q for q in armnav_util.queries_of(M) if len(armnav_util.query(q)["route"]) > 1)
    with rrt_amd.BatchArmNav(M=M) as nav:
        res = test_gpu_armnav.plan_golden(nav, M, [q])
        test_gpu_armnav.assert_queries(res, [q], "M 2, one query")
        assert res.marks is not None and res.marks.shape == (1, M, M)
        ss, grids = test_gpu_armnav.grids_of(M)
        assert np.array_equal(nav._nav.grids(len(ss), M), grids)
        # the arm scenes of this M: the grid kernel, read back through the same getter
        arms = armnav_util.scenes_of(M, 0)
        got = nav.occupancy([armnav_util.scene_arm(s)[0] for s in arms], [armnav_util.scene_arm(s)[1] for s in arms])
    for k, s in enumerate(arms):
        assert np.array_equal(got[k], armnav_util.scene_grid(s)), s


def test_armik_one_query_of_a_two_link_arm(gpu):
    import rrt_amd
    q = test_gpu_armik.queries_of_n(2)[0]
    with rrt_amd.BatchArmIK(max_iterations=test_gpu_armik.IT) as ik:
        res = test_gpu_armik.solve_golden(ik, [q])
        ms, waves = ik._ik.kernel_ms()
    test_gpu_armik.assert_solves(res, [q], "one query, two links")
    assert res.angles.shape == (1, 2) and ms == res.kernel_ms > 0.0 and waves == res.waves == 1


def test_armdh_one_query_of_a_two_link_arm(gpu):
    import rrt_amd
    k = next(k for k in range(armdh_util.n_forward()) if len(armdh_util.forward(k)["dh"]) == 2)
    with rrt_amd.BatchArmDH() as dh:
        fw = dh.forward([armdh_util.forward(k)["dh"]])
        ms, waves = dh._dh.kernel_ms()
    test_gpu_armdh.check_forward(fw, [k], "one query, two links")
    assert ms == fw.kernel_ms > 0.0 and waves == 1

"""The smoothing fit of approximate_b_spline_path on the GPU (BatchBSpline.approximate, rrtx_bspline_approximate): the golden
courses and the corners in one batch against the Python definition bit for bit and against the reference to the measured
gaps, s == 0 against interpolate(), records only with an obstacle list, a handle used again with a smaller and a larger batch,
the hand-over to BatchTrack and the drop-in module.  Comparisons of doubles are of uint64 views unless a gap is named."""
import warnings

import numpy as np
import pytest

import bspline_smooth_oracle as S
import bspline_smooth_util as U
import bspline_oracle as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bb():
    import rrt_amd
    with rrt_amd.BatchBSpline() as b:
        yield b


@pytest.fixture(scope="module")
def full(bb):
    """The golden courses and the corners in one batch, run once"""
    crs, deg, s, cnt, n_gold = U.full_batch()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = bb.approximate(crs, cnt, degree=deg, s=s)
    return res, crs, deg, s, cnt, n_gold, [w for w in caught if issubclass(w.category, RuntimeWarning)]


def test_full_batch_is_the_oracle_bit_for_bit(full):
    """About 100 courses, 2 lanes each: more than one 64-lane block; statuses DEGENERATE and TOO_FEW and courses with s == 0
    side by side with the others.  Records, axis records, knots, coefficients and the five arrays equal the oracle."""
    res, crs, deg, s, cnt, n_gold, _ = full
    want = U.oracle_full()
    assert 2 * len(crs) > 128 and res.rc == 1      # RRTX_PARTIAL: four courses have no spline
    assert sorted(set(res.status.tolist())) == [S.OK, S.DEGENERATE, S.TOO_FEW]
    U.assert_same(res, want, "full batch")
    assert res.kernel_ms > 0.0 and np.array_equal(res.wp_offsets, np.concatenate([[0], np.cumsum([len(x) for x, _ in crs])]))


def test_one_warning_names_the_axes_whose_root_search_stopped_early(bb, full):
    """ier 2 and 3 raise nothing and keep the approximation; one RuntimeWarning per call names how many axes"""
    res, crs, deg, s, cnt, n_gold, caught = full
    want = U.oracle_full()
    early = int(sum(np.sum(want["axis%d" % a]["ier"] > 0) for a in (0, 1)))
    assert early >= 4 and len(caught) == 1 and ("on %d axes" % early) in str(caught[0].message)
    assert {2, 3} <= set(res.ier[0].tolist()) | set(res.ier[1].tolist())
    sel = [i for i in range(n_gold, len(crs)) if max(want["axis0"]["ier"][i], want["axis1"]["ier"][i]) == 3][:1]
    with pytest.warns(RuntimeWarning, match="on 1 axes") as rec:
        one = bb.approximate([crs[i] for i in sel], 50, degree=[deg[i] for i in sel], s=[s[i] for i in sel])
    assert len(rec) == 1 and one.rc == 0 and sorted([int(one.ier[0][0]), int(one.ier[1][0])]) == [0, 3] and len(one.x) == 50
    assert int(one.iters[0][0]) == 20 or int(one.iters[1][0]) == 20
    with warnings.catch_warnings():
        warnings.simplefilter("error")       # and none where every search converges
        bb.approximate(crs[:n_gold], cnt[:n_gold], degree=deg[:n_gold], s=s[:n_gold])


def test_full_batch_is_close_to_the_reference(full):
    """The knot vectors of every golden axis equal scipy's bit for bit; coefficients, x, y, yaw and k within the written gaps"""
    res, n_gold = full[0], full[5]
    seen = U.within(res, n_gold, "device")
    print("; ".join("%s %s" % (q, " ".join("%.2e" % v for _, v in sorted(per.items()))) for q, per in sorted(seen.items())))


def test_s_zero_is_interpolate_bit_for_bit(bb, full):
    res, crs, deg, s, cnt, _, _ = full
    zero = [i for i in range(len(crs)) if s[i] == 0.0]
    assert len(zero) >= 6
    ref = bb.interpolate([crs[i] for i in zero], [cnt[i] for i in zero], degree=[deg[i] for i in zero])
    assert ref.rc == 0
    for j, i in enumerate(zero):
        t = ref.knots[ref.knot_offsets[j]:ref.knot_offsets[j + 1]]
        wa, wb = ref.wp_offsets[j], ref.wp_offsets[j + 1]
        for a in (0, 1):
            assert np.array_equal(U.bits(res.knots[a][res.knot_offsets[a][i]:res.knot_offsets[a][i + 1]]), U.bits(t)), (i, a)
            assert np.array_equal(U.bits(res.coefficients[a][res.coef_offsets[a][i]:res.coef_offsets[a][i + 1]]),
                                  U.bits(ref.coefficients[a][wa:wb])), (i, a)
            assert res.ier[a][i] == -1 and res.fp[a][i] == 0.0 and np.isinf(res.p[a][i])
        for key in U.ARRAYS:
            assert np.array_equal(U.bits(getattr(res, key)[res.offsets[i]:res.offsets[i + 1]]),
                                  U.bits(getattr(ref, key)[ref.offsets[j]:ref.offsets[j + 1]])), (i, key)


def test_records_only_gives_the_same_hits(bb, full):
    """arrays=False with an obstacle list: the same hit as with arrays, and what the oracle's points give"""
    res, crs, deg, s, cnt, _, _ = full
    want = U.oracle_full()
    sel = list(range(0, len(crs), 3))
    pts = [(want["per_course"][i]["x"], want["per_course"][i]["y"]) for i in sel if want["per_course"][i]["x"]]
    obs = [(px[len(px) // 2], py[len(py) // 2], 0.05) for px, py in pts[:8]] + [(1.0e3, 1.0e3, 1.0)]
    kw = dict(degree=[deg[i] for i in sel], s=[s[i] for i in sel], obstacle_list=obs, robot_radius=0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a = bb.approximate([crs[i] for i in sel], [cnt[i] for i in sel], **kw)
        b = bb.approximate([crs[i] for i in sel], [cnt[i] for i in sel], arrays=False, **kw)
    assert b.x is None and a.x is not None and np.array_equal(a.hit, b.hit) and np.array_equal(a.status, b.status)
    hit = [B.first_hit(want["per_course"][i]["x"], want["per_course"][i]["y"], obs, 0.1) if want["per_course"][i]["x"] else -2
           for i in sel]
    assert np.array_equal(a.hit, np.array(hit, dtype=np.int32))
    assert np.sum(a.hit >= 0) >= 8 and np.sum(a.hit == -1) >= 1 and np.sum(a.hit == -2) >= 1
    U.assert_same(a, want, "with obstacles", sel=sel)
    U.assert_same(b, want, "records only", keys=(), sel=sel)
    assert a.is_free(int(np.nonzero(a.hit == -1)[0][0])) and np.array_equal(a.free, a.hit == -1)


def test_handle_used_again_with_a_smaller_and_a_larger_batch(bb, full):
    res, crs, deg, s, cnt, n_gold, _ = full
    want = U.oracle_full()
    small = [5, 0, n_gold + 6, 17]                 # a DEGENERATE course among them
    r1 = bb.approximate([crs[i] for i in small], [cnt[i] for i in small], degree=[deg[i] for i in small], s=[s[i] for i in small])
    U.assert_same(r1, want, "smaller batch", sel=small)
    plain = bb.interpolate([crs[0]], 7)            # the other entry point in between: its own buffers' sizes
    assert plain.rc == 0 and len(plain.x) == 7
    big = list(range(len(crs))) + list(range(len(crs) - 1, -1, -1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        r2 = bb.approximate([crs[i] for i in big], [cnt[i] for i in big], degree=[deg[i] for i in big], s=[s[i] for i in big])
    U.assert_same(r2, want, "larger batch", sel=big)


def test_scalar_s_none_and_explicit_samples(bb):
    """s as one value for the batch and as None (each course's waypoint count); sample parameters as data"""
    crs, deg, s, cnt, _ = U.full_batch()
    sel = [i for i in range(len(crs)) if 6 <= len(crs[i][0]) <= 40][:12]
    part = [crs[i] for i in sel]
    k = [deg[i] for i in sel]
    for sv in (0.5, None):
        res = bb.approximate(part, 21, degree=k, s=sv)
        U.assert_same(res, S.batch(part, n_path_points=21, degree=k, s=sv), "s=%r" % (sv,))
    us = [np.array([0.0, 1.0, 0.5, 0.25, 0.999]) for _ in sel]
    res = bb.approximate(part, degree=k, s=0.05, u=us)
    U.assert_same(res, S.batch(part, degree=k, s=0.05, u=us), "explicit samples")
    with pytest.raises(ValueError, match="interpolation range"):
        bb.approximate(part[:1], degree=3, s=0.5, u=[[0.0, 1.5]])


def test_tracker_takes_a_smooth_result(bb):
    import rrt_amd
    crs, deg, s, cnt, _ = U.full_batch()
    sel = [i for i in range(len(crs)) if 6 <= len(crs[i][0]) <= 9 and deg[i] >= 2 and s[i] != 0.0][:3]
    assert len(sel) == 3
    res = bb.approximate([crs[i] for i in sel], 60, degree=3, s=0.01)
    assert res.rc == 0 and np.all(np.diff(res.offsets) == 60)
    with rrt_amd.BatchTrack() as bt:
        direct = bt.run(res)
        trip = [tuple(q[res.offsets[i]:res.offsets[i + 1]] for q in (res.x, res.y, res.yaw)) for i in range(3)]
        listed = bt.run(trip)
    for f in ("find_goal", "length", "fail", "status"):
        assert np.array_equal(getattr(direct, f), getattr(listed, f)), f
    for k in ("x", "y", "yaw", "v", "t"):
        assert np.array_equal(U.bits(getattr(direct, k)), U.bits(getattr(listed, k))), k
    assert len(direct.status) == 3 and direct.steps > 0


def test_dropin_is_a_batch_of_one(bb):
    """rrt_amd.bspline_path_smoothing.approximate_b_spline_path on the driver's call and on s=None, against the oracle and
    the reference's recorded arrays"""
    import rrt_amd.bspline_path_smoothing as bs
    x, y = [-1.0, 3.0, 4.0, 2.0, 1.0], [0.0, -3.0, 1.0, 1.0, 3.0]
    g = U.kat()
    crs, deg, s, cnt = U.golden_batch()
    for kw, sv in ((dict(s=0.5), 0.5), (dict(), None)):
        got = bs.approximate_b_spline_path(x, y, 50, **kw)
        want = S.course(x, y, 3, sv, n_path_points=50)
        assert len(got) == 4
        for q, key in zip(got, ("x", "y", "yaw", "k")):
            assert np.array_equal(U.bits(q), U.bits(want[key])), (kw, key)
        i = [j for j in range(len(crs)) if crs[j][0].tolist() == x and s[j] == sv and deg[j] == 3][0]
        pa, pb = g["pt_off"][i], g["pt_off"][i + 1]
        assert np.max(np.abs(got[0] - g["rx"][pa:pb])) <= U.MARGIN * U.GAP["xy"][3]
        assert np.max(np.abs(got[1] - g["ry"][pa:pb])) <= U.MARGIN * U.GAP["xy"][3]
    rix = bs.interpolate_b_spline_path(x, y, 50)
    zero = bs.approximate_b_spline_path(x, y, 50, s=0.0)
    assert all(np.array_equal(U.bits(a), U.bits(b)) for a, b in zip(rix, zero))

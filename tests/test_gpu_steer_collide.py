"""BatchSteer's obstacle check on the GPU (steer_fill<KIND, STORE, CHECK>, rrtx_steer_set_obstacles / _get_hits): the
reference's own answers (steer_collide_kat.npz), check_collision evaluated in IEEE doubles over the C oracle's curves, and
the shapes at which the per-point check, the wave minimum and the cross-workgroup atomic minimum can go wrong.  Every
comparison of hit is exact.  One obstacle list holds per solve, so golden rows are solved one call per (kind, step,
obstacle list, robot_radius)."""
import os

import numpy as np
import pytest

import util
import steer_collide_util as scu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(util.ROOT, "tests", "golden")
OK = 0
FILL_TPB = 256   # csrc/steer_batch.hip.h TPB: one lane per curve point, four waves per workgroup
WAVE = 64
FAR = (500.0, 500.0, 1.0)   # never touched
STEP = {"d": 0.1, "r": 0.2}
NAME = {"d": "dubins", "r": "rs"}


@pytest.fixture(scope="module")
def steers(gpu):
    import rrt_amd
    out = {"d": rrt_amd.BatchSteer("dubins"), "r": rrt_amd.BatchSteer("rs")}
    yield out
    for b in out.values():
        b.close()


@pytest.fixture(scope="module")
def kat():
    return scu.load_kat()


@pytest.fixture(scope="module")
def base_map(kat):
    return scu.obstacle_list(kat, 0)


def plan(steers, kind, inp, **kw):
    """inp rows: pose, pose, curvature (and for "r" the step, which must be one value)."""
    inp = np.asarray(inp, dtype=np.float64).reshape(len(inp), -1)
    if kind == "r" and inp.shape[1] > 7:
        assert len(set(inp[:, 7].tolist())) <= 1
        kw.setdefault("step_size", float(inp[0, 7]) if len(inp) else None)
    return steers[kind].plan(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy(), **kw)


# ---- the reference's answers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["d", "r"])
def test_every_golden_row(kat, steers, kind):
    import rrt_amd
    inp, lst, rr, want = (kat[kind + "_" + f] for f in ("inp", "list", "rr", "hit"))
    step = inp[:, 7] if kind == "r" else np.full(len(inp), 0.1)
    sel = [tuple(kat["d_sel"][i][:kat["d_nsel"][i]]) if kind == "d" and kat["d_nsel"][i] >= 0 else None for i in range(len(inp))]
    groups = sorted(set(zip(step.tolist(), lst.tolist(), rr.tolist(), sel)), key=str)
    seen = 0
    for g in groups:
        rows = [i for i in range(len(inp)) if (step[i], lst[i], rr[i], sel[i]) == g]
        kw = dict(obstacle_list=scu.obstacle_list(kat, g[1]), robot_radius=g[2])
        if g[3] is not None:
            kw["selected_types"] = [rrt_amd._abi.DUBINS_WORDS[w] for w in g[3]]
        for points in (True, False):
            res = plan(steers, kind, inp[rows], points=points, **kw)
            assert res.hit.dtype == np.int32 and res.hit.tolist() == want[rows].tolist(), (g[:3], points, kat[kind + "_tag"][rows])
            assert np.array_equal(res.free, want[rows] == -1)
            assert np.array_equal(res.hit == -2, res.status != OK)
        seen += len(rows)
    assert seen == len(inp) == 47
    tags = kat[kind + "_tag"].tolist()
    assert tags.count("graze_free") == tags.count("graze_hit") == 4 and want.tolist().count(999) == 1
    assert np.sum(want == -2) == 1 and np.sum(want == -1) >= 10 and np.sum(want > 0) >= 10


@pytest.mark.parametrize("kind", ["d", "r"])
def test_is_free_is_check_collision(kat, steers, base_map, kind):
    inp = kat[kind + "_inp"]
    rows = [i for i in range(len(inp)) if kat[kind + "_tag"][i] == "map" and (kind == "d" or inp[i, 7] == 0.2)]
    res = plan(steers, kind, inp[rows], obstacle_list=base_map)
    for j, i in enumerate(rows):
        assert res.is_free(j) is (int(kat[kind + "_hit"][i]) == -1)
    last = len(inp) - 1   # the row without a curve
    kw = dict(selected_types=["RLR", "LRL"]) if kind == "d" else {}
    res = plan(steers, kind, inp[last:last + 1], obstacle_list=base_map, **kw)
    assert res.hit.tolist() == [-2] and res.free.tolist() == [False]
    if kind == "d":
        with pytest.raises(TypeError):
            res.is_free(0)
    else:
        assert res.path(0) == (None,) * 5 and res.is_free(0) is False


@pytest.mark.parametrize("kind", ["d", "r"])
def test_points_and_lengths_only_agree_and_the_points_are_unchanged(kat, steers, base_map, kind):
    import rrt_amd
    g = np.load(os.path.join(GOLD, "dubins_kat.npz" if kind == "d" else "rs_kat.npz"))
    inp = g["inp"][:130, :7] if kind == "r" else np.hstack([g["inp"][:130], np.ones((130, 1))])
    plain = plan(steers, kind, inp)
    full = plan(steers, kind, inp, obstacle_list=base_map, robot_radius=0.2)
    lean = plan(steers, kind, inp, points=False, obstacle_list=base_map, robot_radius=0.2)
    assert plain.hit is None and np.array_equal(full.hit, lean.hit) and len(set(full.hit.tolist())) > 5
    assert lean.x is None and lean.offsets is None and lean.rc == full.rc == plain.rc
    for f in ("status", "length", "n_seg", "seg_len", "offsets", "x", "y", "yaw"):
        assert np.array_equal(getattr(full, f), getattr(plain, f)), f
    for f in ("status", "length", "n_seg", "seg_len"):
        assert np.array_equal(getattr(lean, f), getattr(plain, f)), f
    assert full.modes == plain.modes == lean.modes
    S = steers[kind]._steer   # after the lengths-only solve there are no point arrays and no offsets, checked or not
    assert S.counts() == (130, 0)
    with pytest.raises(rrt_amd._abi.RrtxError):
        S.points()
    with pytest.raises(rrt_amd._abi.RrtxError):
        S.summary(offsets=True)
    assert full.kernel_ms > 0.0 and lean.kernel_ms > 0.0


# ---- batch shapes -----------------------------------------------------------------------------------------------------
N_SINGLE = 66


@pytest.fixture(scope="module")
def singles(steers, base_map):
    """The first N_SINGLE pairs of each curve KAT solved one pair per call against the base map: hit and point count."""
    out = {}
    for kind in ("d", "r"):
        g = np.load(os.path.join(GOLD, "dubins_kat.npz" if kind == "d" else "rs_kat.npz"))
        inp = g["inp"][:N_SINGLE, :7] if kind == "r" else np.hstack([g["inp"][:N_SINGLE], np.ones((N_SINGLE, 1))])
        hit, cnt = [], []
        for i in range(N_SINGLE):
            r = plan(steers, kind, inp[i:i + 1], obstacle_list=base_map, robot_radius=0.1)
            hit.append(int(r.hit[0]))
            cnt.append(len(r.x))
        out[kind] = (inp, np.array(hit, dtype=np.int32), np.array(cnt))
        assert np.sum(out[kind][1] == -1) >= 5 and np.sum(out[kind][1] >= 0) >= 5
    assert np.sum(out["r"][1] == -2) >= 2
    return out


@pytest.mark.parametrize("kind", ["d", "r"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_the_wave_equal_single_solves(singles, steers, base_map, kind, n):
    inp, hit, _ = singles[kind]
    for points in (True, False):
        res = plan(steers, kind, inp[:n], points=points, obstacle_list=base_map, robot_radius=0.1)
        assert np.array_equal(res.hit, hit[:n]), points


@pytest.mark.parametrize("kind", ["d", "r"])
@pytest.mark.parametrize("rem", [0, 1, FILL_TPB - 1])
def test_point_totals_around_a_fill_workgroup_boundary(singles, steers, base_map, kind, rem):
    """Point totals FILL_TPB * k + rem: the last workgroup is full, holds one point, or lacks one."""
    inp, hit, cnt = singles[kind]
    pre = np.concatenate([[0], np.cumsum(cnt)])
    pick = None
    for a in range(N_SINGLE):
        for b in range(a + 1, N_SINGLE + 1):
            t = pre[b] - pre[a]
            if t > FILL_TPB and t % FILL_TPB == rem:
                pick = (a, b)
                break
        if pick:
            break
    assert pick is not None, "no run of KAT pairs with %d points modulo %d" % (rem, FILL_TPB)
    rows = list(range(*pick))
    res = plan(steers, kind, inp[rows], obstacle_list=base_map, robot_radius=0.1)
    assert len(res.x) % FILL_TPB == rem and len(res.x) > FILL_TPB
    assert np.array_equal(res.hit, hit[rows])
    lean = plan(steers, kind, inp[rows], points=False, obstacle_list=base_map, robot_radius=0.1)
    assert np.array_equal(lean.hit, hit[rows])


def test_rows_without_a_curve_at_both_ends(singles, steers, base_map):
    inp, hit, _ = singles["r"]
    empty = [i for i in range(N_SINGLE) if hit[i] == -2]
    full = [i for i in range(N_SINGLE) if hit[i] != -2]
    rows = [empty[0]] + full[:5] + [empty[1], empty[0]] + full[5:9] + [empty[1]]
    for points in (True, False):
        res = plan(steers, "r", inp[rows], points=points, obstacle_list=base_map, robot_radius=0.1)
        assert np.array_equal(res.hit, hit[rows]) and res.hit[0] == res.hit[-1] == -2
        assert np.array_equal(res.hit == -2, res.status != OK)


# ---- one long curve: the minimum across waves and across workgroups ------------------------------------------------------
LONG = {"d": (0.0, 0.0, 0.0, 60.0, 5.0, 0.3, 1.0), "r": (0.0, 0.0, 0.0, 60.0, 5.0, 0.3, 1.0, 0.1)}


@pytest.fixture(scope="module")
def long_curve():
    """Per kind: the pair, its oracle curve (between 2 and 3 fill workgroups of points), and touch(k): a small circle
    that touches the curve's point k and at most its direct neighbours (checked with the reference arithmetic)."""
    out = {}
    for kind in ("d", "r"):
        xy = scu.oracle_curve(kind, LONG[kind])
        n = len(xy[0])
        assert 2 * FILL_TPB < n <= 3 * FILL_TPB, n

        def touch(k, xy=xy):
            o = (float(xy[0][k]) + 0.01, float(xy[1][k]) - 0.01, 0.03)
            d = (o[0] - xy[0]) * (o[0] - xy[0]) + (o[1] - xy[1]) * (o[1] - xy[1])
            hits = np.nonzero(d <= o[2] ** 2)[0]     # (a Reeds-Shepp segment end can sit closer than a step to its neighbour)
            assert k in hits and np.all(np.abs(hits - k) <= 1), (k, hits)
            return o
        out[kind] = (np.array([LONG[kind]]), xy, n, touch)
    return out


@pytest.mark.parametrize("kind", ["d", "r"])
def test_one_curve_over_three_workgroups_hit_in_the_last_and_in_the_first(long_curve, steers, kind):
    inp, xy, n, touch = long_curve[kind]
    first, last = touch(7), touch(n - 3)     # workgroup 0 and workgroup 2
    assert (n - 3) // FILL_TPB == 2
    cases = [([FAR, last], 1), ([FAR, first], 1), ([FAR, last, first], 1), ([FAR, first, last], 1), ([last, FAR], 0),
             ([FAR, FAR, FAR], -1), ([FAR, FAR, touch(n - 1)], 2), ([FAR, touch(0)], 1), ([touch(2 * FILL_TPB), touch(FILL_TPB - 1)], 0)]
    for obs, want in cases:
        assert scu.ref_hit(xy, obs, 0.0) == want
        for points in (True, False):
            res = plan(steers, kind, inp, points=points, obstacle_list=obs)
            assert len(res) == 1 and res.hit.tolist() == [want], (obs, points)
            if points:
                assert len(res.x) == n


@pytest.mark.parametrize("kind", ["d", "r"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_obstacle_counts_only_the_last_touched(long_curve, steers, kind, m):
    inp, xy, n, touch = long_curve[kind]
    obs = [(FAR[0] + j, FAR[1], FAR[2]) for j in range(m - 1)] + [touch(300)]
    res = plan(steers, kind, inp, points=False, obstacle_list=obs)
    assert res.hit.tolist() == [m - 1] == [scu.ref_hit(xy, obs, 0.0)]
    res = plan(steers, kind, inp, points=False, obstacle_list=obs[:-1] if m > 1 else [FAR])
    assert res.hit.tolist() == [-1]
    res = plan(steers, kind, inp, points=False, obstacle_list=[])     # m == 0 after a non-empty list: the check is off
    assert res.hit is None


@pytest.mark.parametrize("kind", ["d", "r"])
@pytest.mark.parametrize("j", [0, 62, 63, 64, 256])
def test_two_neighbouring_obstacles_touched_in_different_waves(long_curve, steers, kind, j):
    """Obstacle j is touched by a point of a later wave than obstacle j + 1: the answer is j whatever runs first."""
    inp, xy, n, touch = long_curve[kind]
    ka, kb = 5 * WAVE + 9, WAVE + 3
    assert ka // WAVE != kb // WAVE and ka // FILL_TPB != kb // FILL_TPB
    obs = [(FAR[0] + i, FAR[1], FAR[2]) for i in range(j)] + [touch(ka), touch(kb)]
    assert scu.ref_hit(xy, obs, 0.0) == j
    for points in (True, False):
        assert plan(steers, kind, inp, points=points, obstacle_list=obs).hit.tolist() == [j]
    # the same with a second, short curve in the batch, so that a wave holds points of two pairs
    short = np.array(LONG[kind])
    short[3:6] = (1.0, 1.0, 0.5)
    res = plan(steers, kind, np.array([short, LONG[kind], short]), obstacle_list=obs)
    sh = scu.ref_hit(scu.oracle_curve(kind, short), obs, 0.0)
    assert res.hit.tolist() == [sh, j, sh]


# ---- product mode, sweeps, re-plans, tracking ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["d", "r"])
def test_product_mode_equals_the_explicit_pairs_and_masks_the_matrix(steers, base_map, kind):
    g = np.load(os.path.join(GOLD, "dubins_kat.npz" if kind == "d" else "rs_kat.npz"))
    st, go = g["inp"][:5, 0:3], g["inp"][20:27, 3:6]
    curv = np.linspace(0.5, 2.0, 35)
    bs = steers[kind]
    prod = bs.plan(st, go, curv.copy(), points=False, product=True, obstacle_list=base_map, robot_radius=0.15)
    flat = bs.plan(np.repeat(st, 7, axis=0), np.tile(go, (5, 1)), curv.copy(), obstacle_list=base_map, robot_radius=0.15)
    assert np.array_equal(prod.hit, flat.hit) and np.any(prod.free) and not np.all(prod.free)
    m = prod.length_matrix(free_only=True)
    assert m.shape == (5, 7) and np.array_equal(np.isinf(m), ~prod.free.reshape(5, 7))
    assert np.array_equal(m[~np.isinf(m)], prod.length_matrix()[prod.free.reshape(5, 7)])
    assert np.array_equal(prod.length_matrix(), flat.length.reshape(5, 7))


def sweep_pairs(n, seed):
    rs = np.random.RandomState(seed)
    p = np.empty((n, 6))
    p[:, [0, 1, 3, 4]] = rs.uniform(-2, 15, (n, 4))
    p[:, [2, 5]] = rs.uniform(-np.pi, np.pi, (n, 2))
    near = np.arange(n) % 9 == 0
    p[near, 3:5] = p[near, 0:2] + rs.uniform(-0.5, 0.5, (int(near.sum()), 2))
    return p


def sweep_map(seed, m=30):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-2, 15, m), rs.uniform(-2, 15, m), rs.uniform(0.1, 0.5, m)], axis=1)


SWEEP = {"d": (81, 91, 0.1), "r": (82, 92, 0.15)}   # pair seed, map seed, step


@pytest.mark.parametrize("kind", ["d", "r"])
def test_sweep_against_the_oracle_curves(steers, kind):
    """2 000 pairs x 30 circles; both outcomes must occur in their hundreds (counted on the reference side)."""
    n = 2000
    pseed, mseed, step = SWEEP[kind]
    p = sweep_pairs(n, pseed)
    curv = np.array([1.0, 0.5, 2.0, 1.3])[np.arange(n) % 4]
    obs = sweep_map(mseed)
    rr = 0.05
    inp = np.hstack([p, curv[:, None]] + ([np.full((n, 1), step)] if kind == "r" else []))
    want = np.array([scu.ref_hit(scu.oracle_curve(kind, inp[i]), obs, rr) for i in range(n)], dtype=np.int32)
    assert np.sum(want == -1) >= 200 and np.sum(want >= 0) >= 200 and len(set(want.tolist())) >= 25, np.bincount(want + 2)
    lean = plan(steers, kind, inp, points=False, obstacle_list=obs, robot_radius=rr)
    bad = np.nonzero(lean.hit != want)[0]
    assert len(bad) == 0, (bad[:10], lean.hit[bad[:10]], want[bad[:10]])
    full = plan(steers, kind, inp, obstacle_list=obs, robot_radius=rr)
    assert np.array_equal(full.hit, want)


@pytest.mark.parametrize("kind", ["d", "r"])
def test_replans_on_one_object_leave_nothing_stale(singles, base_map, kind):
    import rrt_amd
    inp, hit, _ = singles[kind]
    other = sweep_map(93, 300)
    want_other = np.array([scu.ref_hit(scu.oracle_curve(kind, np.append(inp[i], 0.2) if kind == "r" else inp[i]), other, 0.0)
                           for i in range(N_SINGLE)], dtype=np.int32)
    assert len(set(want_other.tolist())) > 5
    with rrt_amd.BatchSteer(NAME[kind]) as bs:
        def go(rows, **kw):
            return bs.plan(inp[rows, 0:3], inp[rows, 3:6], inp[rows, 6].copy(), **kw)
        allr = list(range(N_SINGLE))
        assert go(allr[:3], points=False).hit is None
        assert np.array_equal(go(allr, obstacle_list=base_map, robot_radius=0.1).hit, hit)
        assert np.array_equal(go(allr, points=False, obstacle_list=other).hit, want_other)         # a longer list
        rows = [40, 2, 17, 5]
        assert np.array_equal(go(rows, obstacle_list=base_map, robot_radius=0.1).hit, hit[rows])   # a shorter one, fewer pairs
        assert np.array_equal(go(rows[::-1], points=False, obstacle_list=other[:7]).hit,
                              [scu.ref_hit(scu.oracle_curve(kind, np.append(inp[i], 0.2) if kind == "r" else inp[i]), other[:7], 0.0)
                               for i in rows[::-1]])
        cleared = go(rows)                                                                         # the list cleared
        assert cleared.hit is None
        with pytest.raises(rrt_amd._abi.RrtxError):
            bs._steer.hits()
        assert np.array_equal(go(allr[::-1], points=False, obstacle_list=base_map, robot_radius=0.1).hit, hit[::-1])


def test_free_reeds_shepp_curves_go_to_the_tracker(singles, steers, base_map):
    """Curve -> obstacle check -> tracking feasibility without a planner in between."""
    import rrt_amd
    inp, hit, _ = singles["r"]
    res = plan(steers, "r", inp[:24], obstacle_list=base_map, robot_radius=0.1)
    free = np.nonzero(res.free)[0]
    assert 3 <= len(free) < 24
    cnt = np.diff(res.offsets)[free]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    take = np.concatenate([np.arange(res.offsets[i], res.offsets[i + 1]) for i in free])
    start = np.stack([res.x[res.offsets[free]], res.y[res.offsets[free]], res.yaw[res.offsets[free]], np.zeros(len(free))], axis=1)
    with rrt_amd.BatchTrack() as bt:
        tr = bt.run((off, res.x[take], res.y[take], res.yaw[take]), obstacle_list=base_map[:8], robot_radius=0.1,
                    start_state=start)
    assert len(tr) == len(free) and len(tr.find_goal) == len(free) and np.all(tr.length > 0) and tr.steps == int(tr.offsets[-1])

"""Every candidate curve of a pair and the shortest free one on the GPU (BatchSteer.candidates / plan_free,
rrtx_steer_solve_all / _select_free, rrt_amd.reeds_shepp_calc_paths): the reference's calc_paths lists
(tests/golden/steer_all_kat.npz), plan(selected_types=[w]) for Dubins, the host build of the scalar core on random pairs, the
batch shapes at which the double CSR layout can go wrong, and the selection against plan() and against a pick written here.
Every comparison is bit-exact."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import util
import steer_collide_util as scu
from test_steer_all_host import build_check

pytestmark = pytest.mark.gpu
GOLD = os.path.join(util.ROOT, "tests", "golden")
OK, NO_PATH, ZERODIV, VALUE = 0, 1, 2, 3
FILL_TPB = 256   # csrc/steer_batch.hip.h TPB: one lane per output point
FAR = [(500.0, 500.0, 1.0)]   # never touched
WORDS = ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")
RESULT_FIELDS = ("status", "length", "n_seg", "seg_len", "offsets", "x", "y", "yaw", "hit")


@pytest.fixture(scope="module")
def steers(gpu):
    import rrt_amd
    out = {"d": rrt_amd.BatchSteer("dubins"), "r": rrt_amd.BatchSteer("rs")}
    yield out
    for b in out.values():
        b.close()


@pytest.fixture(scope="module")
def kat():
    g = np.load(os.path.join(GOLD, "steer_all_kat.npz"))
    return {f: g[f] for f in g.files}


def cand(bs, inp, **kw):
    """inp rows: pose, pose, curvature, step (one value)."""
    inp = np.asarray(inp, dtype=np.float64).reshape(-1, 8)
    assert len(set(inp[:, 7].tolist())) <= 1
    kw.setdefault("step_size", float(inp[0, 7]) if len(inp) else 0.2)
    return bs.candidates(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy(), **kw)


def per_pair(res):
    """A batch of candidates as one comparable record per pair: nothing in it depends on where the pair sits in the batch."""
    out = []
    for i in range(len(res)):
        cs = []
        for c in res.of(i):
            assert res.pair[c] == i
            rec = [int(res.variant[c]), res.modes[c], int(res.n_seg[c]), res.seg_len[c].tobytes(), res.length[c].tobytes(),
                   res.key[c].tobytes(), None if res.hit is None else int(res.hit[c])]
            if res.x is not None:
                a, b = int(res.offsets[c]), int(res.offsets[c + 1])
                rec += [res.x[a:b].tobytes(), res.y[a:b].tobytes(), res.yaw[a:b].tobytes(), res.directions[a:b].tobytes()]
            cs.append(tuple(rec))
        assert len(cs) == res.n_candidates[i]
        out.append((int(res.status[i]), tuple(cs)))
    return out


def seq_abs_sum(lengths):
    t = 0.0
    for v in lengths:
        t += abs(float(v))
    return t


def expected_status(kat, i):
    n = int(kat["n_cand"][i])
    return OK if n > 0 else (NO_PATH if n == 0 else (ZERODIV if str(kat["err"][i]) == "ZeroDivisionError" else VALUE))


def check_golden_rows(res, rows, kat):
    assert res.cand_offsets.dtype == np.int64 and res.offsets.dtype == np.int64 and res.directions.dtype == np.int8
    assert len(res) == len(rows) and res.cand_offsets[-1] == len(res.pair) and res.offsets[-1] == len(res.x)
    for j, i in enumerate(rows):
        assert int(res.status[j]) == expected_status(kat, i), (i, res.status[j])
        g0, g1 = int(kat["cand_off"][i]), int(kat["cand_off"][i + 1])
        assert res.n_candidates[j] == g1 - g0 == len(res.of(j)), (i, res.n_candidates[j], g1 - g0)
        for c, gc in zip(res.of(j), range(g0, g1)):
            nl = int(kat["c_nlen"][gc])
            assert res.modes[c] == str(kat["c_mode"][gc]) and res.n_seg[c] == nl and 0 <= res.variant[c] < 48, (i, gc)
            assert res.seg_len[c].tobytes() == kat["c_lengths"][gc].tobytes(), (i, gc)
            assert res.key[c] == kat["c_L"][gc] and res.length[c] == seq_abs_sum(kat["c_lengths"][gc][:nl]), (i, gc)
            a, b = int(kat["c_off"][gc]), int(kat["c_off"][gc + 1])
            ra, rb = int(res.offsets[c]), int(res.offsets[c + 1])
            assert rb - ra == b - a, (i, gc)
            for f in ("x", "y", "yaw", "directions"):
                assert np.array_equal(getattr(res, f)[ra:rb], kat[f][a:b]), (i, gc, f)
        assert list(np.diff(res.variant[res.of(j).start:res.of(j).stop]) > 0) == [True] * max(g1 - g0 - 1, 0)   # list order


def golden_paths(kat, i):
    out = []
    for gc in range(int(kat["cand_off"][i]), int(kat["cand_off"][i + 1])):
        a, b = int(kat["c_off"][gc]), int(kat["c_off"][gc + 1])
        out.append((kat["c_lengths"][gc][:kat["c_nlen"][gc]].tolist(), list(str(kat["c_mode"][gc])), float(kat["c_L"][gc]),
                    kat["x"][a:b].tolist(), kat["y"][a:b].tolist(), kat["yaw"][a:b].tolist(), kat["directions"][a:b].tolist()))
    return out


def as_tuples(paths):
    for p in paths:
        assert type(p.lengths) is list and type(p.x) is list and type(p.L) is float and type(p.directions) is list
        assert all(type(v) is float for v in p.lengths + p.x[:2] + p.yaw[:2]) and all(type(v) is int for v in p.directions[:2])
    return [(p.lengths, p.ctypes, p.L, p.x, p.y, p.yaw, p.directions) for p in paths]


# ---- the reference's lists -----------------------------------------------------------------------------------------------
def test_every_golden_row_in_one_call_per_step(kat, steers):
    seen = 0
    for step in sorted(set(kat["inp"][:, 7].tolist())):
        rows = [i for i in range(len(kat["inp"])) if kat["inp"][i, 7] == step]
        res = cand(steers["r"], kat["inp"][rows])
        check_golden_rows(res, rows, kat)
        assert res.hit is None and res.rc == (1 if any(kat["n_cand"][i] <= 0 for i in rows) else 0)
        for j, i in enumerate(rows):
            if kat["n_cand"][i] >= 0:
                assert as_tuples(res.paths(j)) == golden_paths(kat, i), i
            else:
                with pytest.raises(ZeroDivisionError if str(kat["err"][i]) == "ZeroDivisionError" else ValueError):
                    res.paths(j)
        seen += len(rows)
    assert seen == 77


def test_every_golden_row_as_a_batch_of_one(kat, steers):
    for i in range(len(kat["inp"])):
        check_golden_rows(cand(steers["r"], kat["inp"][i:i + 1]), [i], kat)


def test_dropin_calc_paths(kat):
    import rrt_amd.reeds_shepp_calc_paths as cp
    assert tuple(kat["inp"][0]) == (-1.0, -4.0, float(np.deg2rad(-20.0)), 5.0, 5.0, float(np.deg2rad(25.0)), 0.1, 0.05)
    paths = cp.calc_paths(*[float(v) for v in kat["inp"][0]])   # the script's driver poses
    assert all(isinstance(p, cp.Path) for p in paths) and as_tuples(paths) == golden_paths(kat, 0) and len(paths) == 5
    empty = int(np.nonzero(kat["n_cand"] == 0)[0][0])
    assert cp.calc_paths(*[float(v) for v in kat["inp"][empty]]) == []
    for name, exc in (("ZeroDivisionError", ZeroDivisionError), ("ValueError", ValueError)):
        i = int(np.nonzero(kat["err"] == name)[0][0])
        with pytest.raises(exc):
            cp.calc_paths(*[float(v) for v in kat["inp"][i]])


# ---- Dubins: the candidate of word w is plan(selected_types=[w]) ----------------------------------------------------------
def test_dubins_candidates_are_the_single_word_plans(steers):
    g = np.load(os.path.join(GOLD, "steer_kat.npz"))
    inp = g["d_inp"]
    bs = steers["d"]
    args = (inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy())
    res = bs.candidates(*args)
    single = [bs.plan(*args, selected_types=[w]) for w in WORDS]
    assert np.all(res.directions == 1) and res.directions.dtype == np.int8 and len(res.directions) == len(res.x)
    total = 0
    for i in range(len(inp)):
        feasible = [q for q in range(6) if single[q].status[i] == OK]
        assert res.variant[res.of(i).start:res.of(i).stop].tolist() == feasible, i
        assert res.status[i] == (OK if feasible else NO_PATH)
        for c, q in zip(res.of(i), feasible):
            s = single[q]
            a, b = int(s.offsets[i]), int(s.offsets[i + 1])
            ra, rb = int(res.offsets[c]), int(res.offsets[c + 1])
            assert res.modes[c] == s.modes[i] == WORDS[q] and res.n_seg[c] == 3
            assert res.seg_len[c].tobytes() == s.seg_len[i].tobytes() and res.length[c] == s.length[i]
            for f in ("x", "y", "yaw"):
                assert np.array_equal(getattr(res, f)[ra:rb], getattr(s, f)[a:b]), (i, q, f)
            tup = res.paths(i)[c - res.of(i).start]
            assert np.array_equal(tup[0], s.path(i)[0]) and tup[3:] == s.path(i)[3:]
        total += len(feasible)
    assert total == len(res.pair) > 3 * len(inp)
    # plan()'s own choice is the first candidate with the smallest key
    best = bs.plan(*args)
    for i in range(len(inp)):
        c = min(res.of(i), key=lambda c: (res.key[c], c))   # (all six words: every pair has a feasible one)
        assert res.modes[c] == best.modes[i] and res.length[c] == best.length[i]


def test_dubins_lists_with_a_duplicate_and_without_a_feasible_word(steers):
    g = np.load(os.path.join(GOLD, "steer_kat.npz"))
    bs = steers["d"]
    inp = g["d_inp"][:12]
    args = (inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy())
    res = bs.candidates(*args, selected_types=["LSL", "RSR", "LSL"])
    plain = bs.candidates(*args, selected_types=["LSL", "RSR"])
    for i in range(len(inp)):
        want = per_pair(plain)[i][1]
        twice = tuple((2,) + w[1:] for w in want if w[0] == 0)   # the LSL candidate once more, at list position 2
        assert per_pair(res)[i][1] == want + twice, i
    assert np.sum(res.variant == 2) == np.sum(res.variant == 0) > 0
    none = [i for i in range(len(g["d_n"])) if g["d_n"][i] == -1 and g["d_nsel"][i] > 0]
    assert len(none) >= 3
    for i in none:
        sel = [WORDS[w] for w in g["d_sel"][i][:g["d_nsel"][i]]]
        r = bs.candidates(g["d_inp"][i:i + 1, 0:3], g["d_inp"][i:i + 1, 3:6], float(g["d_inp"][i, 6]), selected_types=sel,
                          obstacle_list=FAR)
        assert r.status.tolist() == [NO_PATH] and r.n_candidates.tolist() == [0] and r.paths(0) == [] and r.rc == 1
        assert len(r.pair) == len(r.x) == len(r.hit) == 0 and r.cand_offsets.tolist() == [0, 0] and r.offsets.tolist() == [0]
        f = bs.plan_free(g["d_inp"][i:i + 1, 0:3], g["d_inp"][i:i + 1, 3:6], float(g["d_inp"][i, 6]), selected_types=sel,
                         obstacle_list=FAR)
        p = bs.plan(g["d_inp"][i:i + 1, 0:3], g["d_inp"][i:i + 1, 3:6], float(g["d_inp"][i, 6]), selected_types=sel,
                    obstacle_list=FAR)
        assert_same_result(f, p)
        assert f.hit.tolist() == [-2] and f.n_candidates.tolist() == f.n_free.tolist() == f.rank.tolist() == [0]
    r = bs.candidates(inp[:, 0:3], inp[:, 3:6], 1.0, selected_types=[])   # an empty list: no pair has a candidate
    assert r.n_candidates.tolist() == [0] * 12 and np.all(r.status == NO_PATH)


def assert_same_result(a, b):
    for f in RESULT_FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.modes == b.modes and a.rc == b.rc and a.shape == b.shape and a.kind == b.kind


# ---- shapes at which the layout can go wrong --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(kat, steers):
    """The golden rows at step 0.5 twice over (104 pairs) with a map that touches some candidates: inputs, the batch solved
    whole (checked against the goldens above for its first half), and its per-pair records."""
    rows = [i for i in range(len(kat["inp"])) if kat["inp"][i, 7] == 0.5]
    inp = np.concatenate([kat["inp"][rows], kat["inp"][rows[::-1]]])
    obs = np.stack([np.linspace(-1, 14, 16), np.linspace(14, -1, 16) * 0.7 + 2.0, np.full(16, 0.6)], axis=1)
    res = cand(steers["r"], inp, obstacle_list=obs, robot_radius=0.1)
    assert np.sum(res.hit == -1) > 20 and np.sum(res.hit >= 0) > 20
    return inp, obs, res, per_pair(res)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65])
def test_batch_sizes_around_the_pairs_of_a_wave(pool, steers, n):
    inp, obs, _, want = pool
    for points in (True, False):
        res = cand(steers["r"], inp[:n], points=points, obstacle_list=obs, robot_radius=0.1)
        got = per_pair(res)
        assert [(s, tuple(c[:7] for c in cs)) for s, cs in got] == [(s, tuple(c[:7] for c in cs)) for s, cs in want[:n]]
        if points:
            assert got == want[:n]
        else:
            assert res.x is None and res.offsets is None and res.directions is None


def test_pairs_without_candidates_first_last_and_in_the_middle(pool, steers):
    inp, obs, whole, want = pool
    empty = [i for i in range(len(inp)) if whole.n_candidates[i] == 0]
    full = [i for i in range(len(inp)) if whole.n_candidates[i] > 0]
    assert {int(whole.status[i]) for i in empty} == {NO_PATH, VALUE}
    rows = empty[:2] + full[:5] + empty[2:5] + full[5:9] + empty[5:7]
    for points in (True, False):
        res = cand(steers["r"], inp[rows], points=points, obstacle_list=obs, robot_radius=0.1)
        assert res.n_candidates[0] == res.n_candidates[-1] == res.n_candidates[8] == 0
        cut = 11 if points else 7
        assert [(s, tuple(c[:cut] for c in cs)) for s, cs in per_pair(res)] == [(want[i][0], tuple(c[:cut] for c in want[i][1])) for i in rows]
    only = cand(steers["r"], inp[empty], obstacle_list=obs)     # no candidate in the whole batch
    assert len(only.pair) == 0 and len(only.x) == 0 and only.cand_offsets.tolist() == [0] * (len(empty) + 1)
    assert steers["r"].plan_free(inp[empty, 0:3], inp[empty, 3:6], inp[empty, 6].copy(), step_size=0.5, obstacle_list=obs).hit.tolist() == [-2] * len(empty)


@pytest.mark.parametrize("total", [255, 256, 257])
def test_candidate_totals_around_a_workgroup_of_the_course_launch(pool, steers, total):
    inp, obs, whole, want = pool
    cnt = whole.n_candidates
    full = [i for i in range(len(inp)) if cnt[i] > 0]
    rows, left = [], total
    for i in itertools.cycle(full):
        if left - cnt[i] < 8:
            break
        rows.append(i)
        left -= cnt[i]
    tail = next(t for k in (1, 2, 3) for t in itertools.combinations_with_replacement(full[:40], k) if sum(cnt[list(t)]) == left)
    rows += list(tail)
    res = cand(steers["r"], inp[rows], obstacle_list=obs, robot_radius=0.1)
    assert len(res.pair) == total and res.cand_offsets[-1] == total
    assert per_pair(res) == [want[i] for i in rows]


@pytest.mark.parametrize("rem", [0, 1, FILL_TPB - 1])
def test_point_totals_around_a_fill_workgroup_boundary(pool, steers, rem):
    inp, obs, whole, want = pool
    pts = np.array([whole.offsets[whole.cand_offsets[i + 1]] - whole.offsets[whole.cand_offsets[i]] for i in range(len(inp))])
    pre = np.concatenate([[0], np.cumsum(pts)])
    pick = next(((a, b) for a in range(len(inp)) for b in range(a + 1, len(inp) + 1)
                 if pre[b] - pre[a] > FILL_TPB and (pre[b] - pre[a]) % FILL_TPB == rem), None)
    assert pick is not None, "no run of pool pairs with %d points modulo %d" % (rem, FILL_TPB)
    rows = list(range(*pick))
    res = cand(steers["r"], inp[rows], obstacle_list=obs, robot_radius=0.1)
    assert len(res.x) % FILL_TPB == rem and len(res.x) > FILL_TPB
    assert per_pair(res) == [want[i] for i in rows]
    lean = cand(steers["r"], inp[rows], points=False, obstacle_list=obs, robot_radius=0.1)
    assert np.array_equal(lean.hit, res.hit)


@pytest.mark.parametrize("kind", ["d", "r"])
def test_product_mode_and_per_pair_curvature_equal_the_explicit_pairs(steers, kind):
    g = np.load(os.path.join(GOLD, "dubins_kat.npz" if kind == "d" else "rs_kat.npz"))
    st, go = g["inp"][:5, 0:3], g["inp"][20:27, 3:6]
    curv = np.linspace(0.5, 2.0, 35)
    bs = steers[kind]
    obs = [(5.0, 5.0, 1.5), (10.0, 3.0, 1.0)]
    prod = bs.candidates(st, go, curv.copy(), product=True, obstacle_list=obs)
    flat = bs.candidates(np.repeat(st, 7, axis=0), np.tile(go, (5, 1)), curv.copy(), obstacle_list=obs)
    assert prod.shape == (5, 7) and flat.shape is None and per_pair(prod) == per_pair(flat) and len(prod.pair) > 70
    for i in (0, 17, 34):   # each pair alone, with its own curvature as the scalar
        one = bs.candidates(np.repeat(st, 7, axis=0)[i:i + 1], np.tile(go, (5, 1))[i:i + 1], float(curv[i]), obstacle_list=obs)
        assert per_pair(one)[0] == per_pair(flat)[i]
    pf = bs.plan_free(st, go, curv.copy(), points=False, product=True, obstacle_list=obs)
    ff = bs.plan_free(np.repeat(st, 7, axis=0), np.tile(go, (5, 1)), curv.copy(), obstacle_list=obs)
    for f in ("status", "length", "n_seg", "seg_len", "hit", "rank", "n_free", "n_candidates"):
        assert np.array_equal(getattr(pf, f), getattr(ff, f)), f
    m = pf.length_matrix(free_only=True)
    assert m.shape == (5, 7) and np.array_equal(np.isinf(m), ~pf.free.reshape(5, 7))
    plain = bs.plan(st, go, curv.copy(), points=False, product=True, obstacle_list=obs)
    assert np.sum(np.isinf(m)) <= np.sum(np.isinf(plain.length_matrix(free_only=True)))


def test_a_small_batch_after_a_large_one_leaves_nothing_stale(pool, kat):
    import rrt_amd
    inp, obs, _, want = pool
    with rrt_amd.BatchSteer("rs") as bs:
        big = cand(bs, inp, obstacle_list=obs, robot_radius=0.1)
        assert per_pair(big) == want
        rows = [40, 2, 17, 5]
        small = cand(bs, inp[rows], obstacle_list=obs, robot_radius=0.1)
        assert per_pair(small) == [want[i] for i in rows]
        bare = cand(bs, inp[rows[::-1]], points=False)          # the list cleared, no points
        assert bare.hit is None and bare.x is None
        assert [c[:6] for _, cs in per_pair(bare) for c in cs] == [c[:6] for i in rows[::-1] for c in want[i][1]]
        with pytest.raises(rrt_amd._abi.RrtxError):
            bs._steer.select_free()                              # no obstacle list: nothing to select by
        with pytest.raises(rrt_amd._abi.RrtxError):
            bs._steer.summary()                                  # the candidates replaced the plain result
        plain = bs.plan(inp[rows, 0:3], inp[rows, 3:6], inp[rows, 6].copy(), step_size=0.5)
        with pytest.raises(rrt_amd._abi.RrtxError):
            bs._steer.cand_counts()                              # and a plain solve replaces the candidates
        again = cand(bs, inp[rows], obstacle_list=obs, robot_radius=0.1)
        assert per_pair(again) == [want[i] for i in rows] and len(plain) == 4
        with pytest.raises(ValueError):
            bs.plan_free(inp[:2, 0:3], inp[:2, 3:6], 1.0)           # an obstacle list is required
        with pytest.raises(TypeError):
            bs.candidates(inp[:2, 0:3], inp[:2, 3:6])               # curvature
    with rrt_amd.BatchSteer("lqr") as bs:
        with pytest.raises(ValueError):
            bs.candidates(inp[:2, 0:2], inp[:2, 3:5], 1.0)


# ---- selection --------------------------------------------------------------------------------------------------------------
def sweep_pairs(n, seed):
    rs = np.random.RandomState(seed)
    p = np.empty((n, 6))
    p[:, [0, 1, 3, 4]] = rs.uniform(-2, 15, (n, 4))
    p[:, [2, 5]] = rs.uniform(-np.pi, np.pi, (n, 2))
    near = np.arange(n) % 9 == 0
    p[near, 3:5] = p[near, 0:2] + rs.uniform(-0.5, 0.5, (int(near.sum()), 2))
    return p


def random_map(seed, m=12):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(0, 13, m), rs.uniform(0, 13, m), rs.uniform(0.3, 1.2, m)], axis=1)


STEP = {"d": 0.1, "r": 0.2}


@pytest.fixture(scope="module")
def on_a_map(steers):
    """Per kind: 400 random pairs among 12 circles -- the inputs, plan(), candidates() and plan_free() of them."""
    out = {}
    for kind, seed in (("d", 71), ("r", 72)):
        p = sweep_pairs(400, seed)
        curv = np.array([1.0, 0.5, 2.0, 1.3])[np.arange(400) % 4]
        obs = random_map(seed + 10)
        a = (p[:, 0:3], p[:, 3:6], curv)
        kw = dict(step_size=STEP[kind], obstacle_list=obs, robot_radius=0.05)
        bs = steers[kind]
        out[kind] = (a, kw, bs.plan(*a, **kw), bs.candidates(*a, **kw), bs.plan_free(*a, **kw))
    return out


@pytest.mark.parametrize("kind", ["d", "r"])
def test_an_obstacle_no_curve_touches_leaves_plan(steers, on_a_map, kind):
    """Property (a): with an obstacle list that no curve touches, plan_free equals plan in every array."""
    a, kw, _, cands, _ = on_a_map[kind]
    for points in (True, False):
        far = dict(kw, obstacle_list=FAR, points=points)
        free, plain = steers[kind].plan_free(*a, **far), steers[kind].plan(*a, **far)
        assert_same_result(free, plain)
        assert np.all(free.rank == 0) and np.array_equal(free.n_free, free.n_candidates)
        assert np.array_equal(free.n_candidates, cands.n_candidates) and free.rank.dtype == np.int32
        assert np.array_equal(free.hit == -1, free.status == OK) and free.kernel_ms > 0.0


@pytest.mark.parametrize("kind", ["d", "r"])
def test_rows_whose_shortest_curve_is_free_are_plans_rows(on_a_map, kind):
    """Property (b): every row with plan().free[i] true is identical in both results."""
    _, _, plain, _, free = on_a_map[kind]
    keep = np.nonzero(plain.free)[0]
    assert 50 < len(keep) < 350
    for i in keep:
        for f in ("status", "length", "n_seg", "seg_len", "hit"):
            assert np.array_equal(getattr(free, f)[i], getattr(plain, f)[i]), (i, f)
        assert free.modes[i] == plain.modes[i] and free.rank[i] == 0
        for f in ("x", "y", "yaw"):
            assert np.array_equal(getattr(free, f)[free.offsets[i]:free.offsets[i + 1]],
                                  getattr(plain, f)[plain.offsets[i]:plain.offsets[i + 1]]), (i, f)
    assert np.array_equal(free.status, plain.status) and np.all(free.free[keep])
    moved = np.nonzero(free.free & ~plain.free)[0]       # what the feature is for
    assert len(moved) > 10 and np.all(free.rank[moved] > 0) and np.all(free.n_free[moved] > 0)
    stuck = np.nonzero(~free.free)[0]                    # no free candidate: plan()'s row with its hit
    for i in stuck:
        for f in ("status", "length", "n_seg", "seg_len", "hit"):
            assert np.array_equal(getattr(free, f)[i], getattr(plain, f)[i]), (i, f)
    assert np.all(free.n_free[stuck] == 0) and np.all(free.rank[stuck] == 0)


@pytest.mark.parametrize("kind", ["d", "r"])
def test_plan_free_is_a_pick_over_the_candidates_own_columns(on_a_map, kind):
    """The pick written out on the host over candidates()'s key and hit: the free candidate smallest by the key plan()
    minimises (the `key` column: for "rs" abs(L / maxc), which can differ from `length` in the last bit), the first in
    list order among equal keys; none free: the same over all candidates."""
    _, _, _, cands, free = on_a_map[kind]
    ranked = 0
    for i in range(len(cands)):
        cs = list(cands.of(i))
        assert free.n_candidates[i] == len(cs)
        if not cs:
            assert free.status[i] != OK and free.hit[i] == -2 and free.length[i] == 0.0 and free.rank[i] == free.n_free[i] == 0
            assert free.offsets[i + 1] == free.offsets[i]
            continue
        order = sorted(cs, key=lambda c: (cands.key[c], c))
        ok = [c for c in order if cands.hit[c] == -1]
        c = ok[0] if ok else order[0]
        assert free.rank[i] == order.index(c) and free.n_free[i] == len(ok), i
        assert free.hit[i] == cands.hit[c] and free.length[i] == cands.length[c] and free.modes[i] == cands.modes[c], i
        assert free.n_seg[i] == cands.n_seg[c] and np.array_equal(free.seg_len[i], cands.seg_len[c]), i
        a, b = int(cands.offsets[c]), int(cands.offsets[c + 1])
        fa, fb = int(free.offsets[i]), int(free.offsets[i + 1])
        for f in ("x", "y", "yaw"):
            assert np.array_equal(getattr(free, f)[fa:fb], getattr(cands, f)[a:b]), (i, f)
        ranked += free.rank[i] > 0
    assert ranked > 10 and free.offsets[-1] == len(free.x)


@pytest.mark.parametrize("kind", ["d", "r"])
def test_hit_of_every_candidate_is_check_collision_on_its_points(on_a_map, kind):
    _, kw, _, cands, _ = on_a_map[kind]
    want = np.array([scu.ref_hit((cands.x[cands.offsets[c]:cands.offsets[c + 1]], cands.y[cands.offsets[c]:cands.offsets[c + 1]]),
                                 kw["obstacle_list"], kw["robot_radius"]) for c in range(len(cands.pair))], dtype=np.int32)
    assert cands.hit.dtype == np.int32 and np.array_equal(cands.hit, want)
    assert np.sum(want == -1) > 200 and np.sum(want >= 0) > 200 and len(set(want.tolist())) >= 8


@pytest.mark.parametrize("kind", ["d", "r"])
def test_forged_circles_move_the_choice_and_circles_on_all_leave_plan(steers, on_a_map, kind):
    a, kw, _, cands, _ = on_a_map[kind]
    bs = steers[kind]
    done = 0
    for i in range(len(cands)):
        cs = sorted(cands.of(i), key=lambda c: (cands.key[c], c))
        if len(cs) < 2 or cands.key[cs[0]] == cands.key[cs[1]]:
            continue
        xy = {c: (cands.x[cands.offsets[c]:cands.offsets[c + 1]], cands.y[cands.offsets[c]:cands.offsets[c + 1]]) for c in cs}
        circle = None
        for k in range(len(xy[cs[0]][0])):   # a point only the shortest candidate passes
            o = (float(xy[cs[0]][0][k]), float(xy[cs[0]][1][k]), 0.02)
            if all(scu.ref_hit(xy[c], [o], 0.0) == -1 for c in cs[1:]):
                circle = o
                break
        if circle is None:
            continue
        one = (a[0][i:i + 1], a[1][i:i + 1], float(a[2][i]))
        lst = FAR + [circle]
        free = bs.plan_free(*one, step_size=STEP[kind], obstacle_list=lst)
        plain = bs.plan(*one, step_size=STEP[kind], obstacle_list=lst)
        assert plain.hit.tolist() == [1] and free.hit.tolist() == [-1] and free.rank.tolist() == [1]
        assert free.n_free.tolist() == [len(cs) - 1] and free.length[0] == cands.length[cs[1]] and free.modes[0] == cands.modes[cs[1]]
        assert np.array_equal(free.x, xy[cs[1]][0]) and np.array_equal(free.y, xy[cs[1]][1])
        # a circle on the start pose is on every candidate: plan()'s row with its hit
        lst = FAR + [(float(one[0][0, 0]), float(one[0][0, 1]), 0.02)]
        free = bs.plan_free(*one, step_size=STEP[kind], obstacle_list=lst)
        assert_same_result(free, bs.plan(*one, step_size=STEP[kind], obstacle_list=lst))
        assert free.hit.tolist() == [1] and free.rank.tolist() == [0] and free.n_free.tolist() == [0]
        done += 1
        if done == 6:
            break
    assert done == 6


@pytest.mark.parametrize("kind", ["d", "r"])
def test_without_points_every_per_pair_column_is_the_same(steers, on_a_map, kind):
    import rrt_amd
    a, kw, _, cands, free = on_a_map[kind]
    lean = steers[kind].plan_free(*a, points=False, **kw)
    for f in ("status", "length", "n_seg", "seg_len", "hit", "rank", "n_candidates", "n_free"):
        assert np.array_equal(getattr(lean, f), getattr(free, f)), f
    assert lean.modes == free.modes and lean.x is None and lean.offsets is None and lean.rc == free.rc
    S = steers[kind]._steer
    assert S.counts() == (400, 0) and S.cand_counts()[2] == 0
    with pytest.raises(rrt_amd._abi.RrtxError):
        S.points()
    with pytest.raises(rrt_amd._abi.RrtxError):
        S.cand_points()
    lc = steers[kind].candidates(*a, points=False, **kw)
    assert np.array_equal(lc.hit, cands.hit) and np.array_equal(lc.key, cands.key) and lc.offsets is None


def test_the_result_goes_to_the_tracker(steers, on_a_map):
    """Curve -> the shortest free candidate -> tracking feasibility, without a planner in between."""
    import rrt_amd
    a, kw, _, _, whole = on_a_map["r"]
    free = steers["r"].plan_free(a[0][:24], a[1][:24], a[2][:24].copy(), **kw)
    for f in ("status", "length", "hit", "rank"):
        assert np.array_equal(getattr(free, f), getattr(whole, f)[:24]), f
    with rrt_amd.BatchTrack() as bt:
        tr = bt.run(free)
    assert len(tr) == len(tr.find_goal) == 24 and tr.steps == int(tr.offsets[-1])


# ---- random sweep against the host build of the scalar core ---------------------------------------------------------------
def test_sweep_against_the_host_build_of_the_scalar_core(steers, tmp_path):
    """2 000 pairs: counts, variants, words, lengths, keys, points, yaws and directions."""
    n = 2000
    p = sweep_pairs(n, 73)
    curv = np.array([0.1, 0.5, 1.0, 2.0])[np.arange(n) % 4]
    inp = np.hstack([p, curv[:, None], np.full((n, 1), 0.3)])
    exe = build_check(str(tmp_path))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    inp.astype(np.float64).tofile(fin)
    subprocess.run([exe, "print", fin, fout], check=True)
    res = cand(steers["r"], inp)
    blob = open(fout, "rb").read()
    pos, ncand, many = 0, 0, 0
    for i in range(n):
        st, nc = struct.unpack_from("<ii", blob, pos)
        pos += 8
        assert (int(res.status[i]), int(res.n_candidates[i])) == (st, nc), i
        for c in res.of(i):
            variant, nl, npts = struct.unpack_from("<iii", blob, pos)
            pos += 12
            modes = blob[pos:pos + 8].rstrip(b"\0").decode()
            pos += 8
            vals = np.frombuffer(blob, dtype=np.float64, count=7 + 3 * npts, offset=pos)
            pos += 8 * (7 + 3 * npts)
            dirs = np.frombuffer(blob, dtype=np.int8, count=npts, offset=pos)
            pos += npts
            a, b = int(res.offsets[c]), int(res.offsets[c + 1])
            assert (int(res.variant[c]), int(res.n_seg[c]), b - a, res.modes[c]) == (variant, nl, npts, modes), (i, c)
            assert res.seg_len[c].tobytes() == vals[:5].tobytes() and res.length[c] == vals[5] and res.key[c] == vals[6], (i, c)
            assert np.array_equal(res.x[a:b], vals[7:7 + npts]) and np.array_equal(res.y[a:b], vals[7 + npts:7 + 2 * npts]), (i, c)
            assert np.array_equal(res.yaw[a:b], vals[7 + 2 * npts:]) and np.array_equal(res.directions[a:b], dirs), (i, c)
        ncand += nc
        many += nc >= 10
    assert pos == len(blob) and ncand == len(res.pair) > 4 * n and many >= 1
    assert np.sum(res.status == NO_PATH) > 5 and set(res.directions.tolist()) == {1, -1}

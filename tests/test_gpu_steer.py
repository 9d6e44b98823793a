"""Batched Dubins / Reeds-Shepp curves on the GPU (BatchSteer, rrtx_steer_*): the reference's known-answer vectors, the C
oracle on random pairs, the batch shapes at which the two-stage CSR layout can go wrong, and the two drop-in modules.
Every comparison is bit-exact."""
import os

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
GOLD = os.path.join(util.ROOT, "tests", "golden")
OK, NO_PATH, ZERODIV, VALUE = 0, 1, 2, 3
FILL_TPB = 256   # csrc/steer_batch.hip.h TPB: one lane per output point


def starts_of(off, n):
    return np.concatenate([[0], np.cumsum(np.maximum(n, 0))])[:-1] if off is None else off


@pytest.fixture(scope="module")
def kats():
    d = np.load(os.path.join(GOLD, "dubins_kat.npz"))
    r = np.load(os.path.join(GOLD, "rs_kat.npz"))
    s = np.load(os.path.join(GOLD, "steer_kat.npz"))
    return {k: {f: g[f] for f in g.files} for k, g in (("dubins", d), ("rs", r), ("steer", s))}


@pytest.fixture(scope="module")
def steers():
    import rrt_amd
    out = {"dubins": rrt_amd.BatchSteer("dubins"), "rs": rrt_amd.BatchSteer("rs")}
    yield out
    for b in out.values():
        b.close()


def seq_abs_sum(lengths):
    """The `length` column: the absolute segment lengths (as the reference returns them) added up in order."""
    t = 0.0
    for v in lengths:
        t += abs(float(v))
    return t


def rs_expected_status(n, mode):
    if n > 0:
        return OK
    if n == 0:
        return NO_PATH
    return ZERODIV if str(mode) == "ZeroDivisionError" else VALUE


def check_rs_rows(res, rows, g, px, py, pyaw, goff):
    """res: the batch solved for the golden rows `rows` (indices into g); goff: start of each golden row's points."""
    for j, k in enumerate(rows):
        n = int(g["n"][k])
        assert int(res.status[j]) == rs_expected_status(n, g["mode"][k]), (k, res.status[j])
        a, b = int(res.offsets[j]), int(res.offsets[j + 1])
        assert b - a == max(n, 0), (k, b - a, n)
        if n <= 0:
            assert res.modes[j] == "" and len(res.lengths[j]) == 0 and res.length[j] == 0.0
            continue
        nl = int(g["n_len"][k])
        assert res.modes[j] == str(g["mode"][k]), k
        assert np.array_equal(res.lengths[j], g["lengths"][k][:nl]) and res.length[j] == seq_abs_sum(g["lengths"][k][:nl]), k
        o = int(goff[k])
        assert np.array_equal(res.x[a:b], px[o:o + n]) and np.array_equal(res.y[a:b], py[o:o + n]), k
        assert np.array_equal(res.yaw[a:b], pyaw[o:o + n]), k


def test_all_dubins_known_answers_in_one_call(kats, steers):
    g = kats["dubins"]
    inp = g["inp"]
    res = steers["dubins"].plan(inp[:, 0:3], inp[:, 3:6], 1.0)
    assert res.rc == 0 and len(res) == 400
    assert np.array_equal(np.diff(res.offsets), g["n"])
    assert np.array_equal(res.x, g["poly_x"]) and np.array_equal(res.y, g["poly_y"])
    assert np.array_equal(res.seg_len[:, :3], g["lengths"]) and np.all(res.n_seg == 3) and np.all(res.status == OK)
    assert res.modes == [str(m) for m in g["mode"]]
    assert np.array_equal(res.yaw[res.offsets[1:] - 1], g["end"][:, 2])
    assert np.array_equal(res.x[res.offsets[1:] - 1], g["end"][:, 0])
    ln = g["lengths"]
    assert np.array_equal(res.length, np.abs(ln[:, 0]) + np.abs(ln[:, 1]) + np.abs(ln[:, 2]))


def test_all_reeds_shepp_known_answers_one_call_per_step(kats, steers):
    import rrt_amd
    g = kats["rs"]
    inp = g["inp"]
    goff = starts_of(None, g["n"])
    steps = sorted(set(inp[:, 7].tolist()))
    assert len(steps) >= 2
    seen = 0
    for step in steps:
        rows = np.nonzero(inp[:, 7] == step)[0]
        res = steers["rs"].plan(inp[rows, 0:3], inp[rows, 3:6], inp[rows, 6].copy(), step_size=step)
        bad = int(np.sum(g["n"][rows] <= 0))
        assert res.rc == (rrt_amd._abi.RRTX_PARTIAL if bad else 0)
        check_rs_rows(res, rows, g, g["poly_x"], g["poly_y"], g["poly_yaw"], goff)
        seen += len(rows)
    assert seen == 600
    assert np.sum(g["n"] == 0) > 0 and np.sum(g["n"] < 0) > 0   # the golden holds both kinds of rows without a path


def test_steer_kat_dubins_selected_types_and_curvatures(kats, steers):
    """Curvatures 0.5 / 2.0, the yaw column, start = goal, near goals, ordered selected_types lists and the lists
    without a feasible word (the reference raises TypeError there: status NO_PATH, no points)."""
    import rrt_amd
    g = kats["steer"]
    inp, n = g["d_inp"], g["d_n"]
    goff = starts_of(None, n)
    keys = [tuple(g["d_sel"][i][:g["d_nsel"][i]]) if g["d_nsel"][i] >= 0 else None for i in range(len(n))]
    assert any(k is not None and list(k) != sorted(k) for k in keys) and np.sum(n < 0) >= 2
    for key in sorted(set(keys), key=str):
        rows = [i for i in range(len(n)) if keys[i] == key]
        sel = None if key is None else [rrt_amd._abi.DUBINS_WORDS[w] for w in key]
        res = steers["dubins"].plan(inp[rows, 0:3], inp[rows, 3:6], inp[rows, 6].copy(), selected_types=sel)
        assert res.rc == (rrt_amd._abi.RRTX_PARTIAL if np.any(n[rows] < 0) else 0), key
        for j, k in enumerate(rows):
            a, b = int(res.offsets[j]), int(res.offsets[j + 1])
            if n[k] < 0:
                assert res.status[j] == NO_PATH and a == b and res.modes[j] == "", k
                with pytest.raises(TypeError):
                    res.path(j)
                continue
            o = int(goff[k])
            assert res.status[j] == OK and b - a == n[k], k
            assert res.modes[j] == str(g["d_mode"][k]) and np.array_equal(res.lengths[j], g["d_lengths"][k]), k
            assert np.array_equal(res.x[a:b], g["d_x"][o:o + n[k]]) and np.array_equal(res.y[a:b], g["d_y"][o:o + n[k]]), k
            assert np.array_equal(res.yaw[a:b], g["d_yaw"][o:o + n[k]]), k


def test_steer_kat_reeds_shepp_driver_call_and_fine_step(kats, steers):
    g = kats["steer"]
    inp = g["r_inp"]
    gg = dict(n=g["r_n"], mode=g["r_mode"], n_len=g["r_n_len"], lengths=g["r_lengths"])
    assert tuple(inp[0, 6:8]) == (0.1, 0.05) and np.any((inp[:, 6] == 2.0) & (inp[:, 7] == 0.05))
    assert set(inp[:, 7].tolist()) == {0.05}
    res = steers["rs"].plan(inp[:, 0:3], inp[:, 3:6], inp[:, 6].copy(), step_size=0.05)
    check_rs_rows(res, range(len(inp)), gg, g["r_x"], g["r_y"], g["r_yaw"], starts_of(None, g["r_n"]))


# ---- batch shapes ---------------------------------------------------------------------------------------------------
N_SINGLE = 66


@pytest.fixture(scope="module")
def singles(kats, steers):
    """The first N_SINGLE pairs of each KAT solved one pair per call (curvature 1 / the row's; RS at step 0.2 for every
    row, whatever step the golden used): what every batch of the same pairs must reproduce."""
    out = {}
    for kind in ("dubins", "rs"):
        inp = kats[kind]["inp"][:N_SINGLE]
        curv = np.ones(N_SINGLE) if kind == "dubins" else inp[:, 6].copy()
        rows = []
        for i in range(N_SINGLE):
            r = steers[kind].plan(inp[i:i + 1, 0:3], inp[i:i + 1, 3:6], float(curv[i]))
            rows.append((int(r.status[0]), r.modes[0], r.lengths[0], float(r.length[0]), r.x.copy(), r.y.copy(), r.yaw.copy()))
        out[kind] = (inp, curv, rows)
    return out


def assert_batch_equals_singles(res, rows, ref_rows):
    assert len(res) == len(rows)
    for j, i in enumerate(rows):
        st, mode, lens, length, x, y, yaw = ref_rows[i]
        a, b = int(res.offsets[j]), int(res.offsets[j + 1])
        assert int(res.status[j]) == st and res.modes[j] == mode and res.length[j] == length, (j, i)
        assert np.array_equal(res.lengths[j], lens), (j, i)
        assert np.array_equal(res.x[a:b], x) and np.array_equal(res.y[a:b], y) and np.array_equal(res.yaw[a:b], yaw), (j, i)


@pytest.mark.parametrize("kind", ["dubins", "rs"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_the_wave_equal_single_solves(singles, steers, kind, n):
    inp, curv, ref = singles[kind]
    res = steers[kind].plan(inp[:n, 0:3], inp[:n, 3:6], curv[:n].copy())
    assert_batch_equals_singles(res, list(range(n)), ref)


def test_rows_without_points_at_both_ends(singles, steers):
    """Zero-length CSR rows first and last (NO_PATH / raising Reeds-Shepp pairs), and two of them side by side."""
    inp, curv, ref = singles["rs"]
    empty = [i for i in range(N_SINGLE) if ref[i][0] != OK]
    full = [i for i in range(N_SINGLE) if ref[i][0] == OK]
    assert len(empty) >= 2
    rows = [empty[0]] + full[:5] + [empty[1], empty[0]] + full[5:9] + [empty[1]]
    res = steers["rs"].plan(inp[rows, 0:3], inp[rows, 3:6], curv[rows].copy())
    assert res.offsets[0] == res.offsets[1] == 0 and res.offsets[-1] == res.offsets[-2] == len(res.x)
    assert_batch_equals_singles(res, rows, ref)


@pytest.mark.parametrize("kind", ["dubins", "rs"])
@pytest.mark.parametrize("rem", [0, 1, FILL_TPB - 1])
def test_point_totals_around_a_fill_workgroup_boundary(singles, steers, kind, rem):
    """Batches whose total point count is a multiple of the fill kernel's workgroup, one more, and one less."""
    inp, curv, ref = singles[kind]
    cnt = np.array([len(r[4]) for r in ref])
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
    res = steers[kind].plan(inp[rows, 0:3], inp[rows, 3:6], curv[rows].copy())
    assert len(res.x) % FILL_TPB == rem and len(res.x) > FILL_TPB
    assert_batch_equals_singles(res, rows, ref)


@pytest.mark.parametrize("kind", ["dubins", "rs"])
def test_product_mode_equals_the_explicit_pairs(kats, steers, kind):
    inp = kats[kind]["inp"]
    st, go = inp[:5, 0:3], inp[20:27, 3:6]
    curv = np.linspace(0.5, 2.0, 35)
    prod = steers[kind].plan(st, go, curv.copy(), product=True)
    flat = steers[kind].plan(np.repeat(st, 7, axis=0), np.tile(go, (5, 1)), curv.copy())
    assert len(prod) == 35 and prod.length_matrix().shape == (5, 7)
    assert np.array_equal(prod.length_matrix().reshape(-1), flat.length)
    for f in ("status", "n_seg", "seg_len", "offsets", "x", "y", "yaw"):
        assert np.array_equal(getattr(prod, f), getattr(flat, f)), f
    assert prod.modes == flat.modes
    i, j = 3, 4
    one = steers[kind].plan(st[i:i + 1], go[j:j + 1], float(curv[i * 7 + j]))
    assert one.length[0] == prod.length_matrix()[i, j]


@pytest.mark.parametrize("kind", ["dubins", "rs"])
def test_lengths_only_gives_the_same_summary(kats, steers, kind):
    inp = kats[kind]["inp"][:130]
    curv = 1.0 if kind == "dubins" else inp[:, 6].copy()
    full = steers[kind].plan(inp[:, 0:3], inp[:, 3:6], curv)
    lean = steers[kind].plan(inp[:, 0:3], inp[:, 3:6], curv, points=False)
    assert lean.x is None and lean.offsets is None and lean.rc == full.rc
    for f in ("status", "length", "n_seg", "seg_len"):
        assert np.array_equal(getattr(lean, f), getattr(full, f)), f
    assert lean.modes == full.modes


def sweep_pairs(n, seed):
    rs = np.random.RandomState(seed)
    p = np.empty((n, 6))
    p[:, [0, 1, 3, 4]] = rs.uniform(-2, 15, (n, 4))
    p[:, [2, 5]] = rs.uniform(-np.pi, np.pi, (n, 2))
    near = np.arange(n) % 9 == 0
    p[near, 3:5] = p[near, 0:2] + rs.uniform(-0.5, 0.5, (int(near.sum()), 2))
    return p


def test_dubins_sweep_against_the_oracle(steers):
    import oracle
    n = 2000
    p = sweep_pairs(n, 71)
    curv = np.array([1.0, 0.5, 2.0, 1.3])[np.arange(n) % 4]
    res = steers["dubins"].plan(p[:, 0:3], p[:, 3:6], curv.copy())
    assert res.rc == 0
    for i in range(n):
        px, py, pyaw, mode, ln = oracle.dubins(*[float(v) for v in p[i]], float(curv[i]), cap=16384)
        a, b = int(res.offsets[i]), int(res.offsets[i + 1])
        assert b - a == len(px) and res.modes[i] == mode, i
        assert np.array_equal(res.lengths[i], ln) and res.length[i] == seq_abs_sum(ln), i
        assert np.array_equal(res.x[a:b], px) and np.array_equal(res.y[a:b], py) and np.array_equal(res.yaw[a:b], pyaw), i


def test_reeds_shepp_sweep_against_the_oracle(steers):
    import oracle
    n = 2000
    p = sweep_pairs(n, 72)
    p[::13, 5] = p[::13, 2]                  # equal yaws: where the reference's degenerate cases live
    p[::26, 4] = p[::26, 1]
    curv = np.array([1.0, 0.5, 2.0, 1.3])[np.arange(n) % 4]
    res = steers["rs"].plan(p[:, 0:3], p[:, 3:6], curv.copy(), step_size=0.15)
    for i in range(n):
        args = [float(v) for v in p[i]] + [float(curv[i]), 0.15]
        a, b = int(res.offsets[i]), int(res.offsets[i + 1])
        try:
            px, py, pyaw, mode, ln = oracle.reeds_shepp(*args)
        except ZeroDivisionError:
            assert res.status[i] == ZERODIV and a == b, i
            continue
        except ValueError:
            assert res.status[i] == VALUE and a == b, i
            continue
        if px is None:
            assert res.status[i] == NO_PATH and a == b, i
            continue
        assert res.status[i] == OK and b - a == len(px) and res.modes[i] == mode, i
        assert np.array_equal(res.lengths[i], ln), i
        assert res.length[i] == seq_abs_sum(ln), i
        assert np.array_equal(res.x[a:b], px) and np.array_equal(res.y[a:b], py) and np.array_equal(res.yaw[a:b], pyaw), i


@pytest.mark.parametrize("kind", ["dubins", "rs"])
def test_second_plan_on_regrown_buffers_has_nothing_stale(singles, kind):
    """A small batch, a larger one (every buffer regrows), then a smaller one again on the same object."""
    import rrt_amd
    inp, curv, ref = singles[kind]
    with rrt_amd.BatchSteer(kind) as bs:
        for rows in (list(range(3)), list(range(N_SINGLE)), [40, 2, 17, 5], list(range(N_SINGLE - 1, -1, -1)), [9]):
            res = bs.plan(inp[rows, 0:3], inp[rows, 3:6], curv[rows].copy())
            assert_batch_equals_singles(res, rows, ref)
            lean = bs.plan(inp[rows, 0:3], inp[rows, 3:6], curv[rows].copy(), points=False)
            assert np.array_equal(lean.length, res.length) and np.array_equal(lean.status, res.status)


def test_dropin_functions_return_the_reference_tuples(kats):
    from rrt_amd.dubins_path import plan_dubins_path
    from rrt_amd.reeds_shepp_path import reeds_shepp_path_planning
    g = kats["dubins"]
    off = 0
    for k in range(6):
        n = int(g["n"][k])
        px, py, pyaw, mode, ln = plan_dubins_path(*[float(v) for v in g["inp"][k]], 1.0)
        assert isinstance(px, np.ndarray) and isinstance(py, np.ndarray) and isinstance(pyaw, np.ndarray)
        assert isinstance(mode, list) and all(isinstance(m, str) and len(m) == 1 for m in mode) and isinstance(ln, list)
        assert np.array_equal(px, g["poly_x"][off:off + n]) and np.array_equal(py, g["poly_y"][off:off + n])
        assert "".join(mode) == str(g["mode"][k]) and ln == g["lengths"][k].tolist() and pyaw[-1] == g["end"][k][2]
        off += n
    s = kats["steer"]
    k = int(np.nonzero(s["d_nsel"] > 1)[0][0])
    sel = [("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")[w] for w in s["d_sel"][k][:s["d_nsel"][k]]]
    o, n = int(starts_of(None, s["d_n"])[k]), int(s["d_n"][k])
    px, py, pyaw, mode, ln = plan_dubins_path(*[float(v) for v in s["d_inp"][k]], selected_types=sel)
    assert np.array_equal(px, s["d_x"][o:o + n]) and np.array_equal(pyaw, s["d_yaw"][o:o + n]) and "".join(mode) == str(s["d_mode"][k])
    r = kats["rs"]
    goff = starts_of(None, r["n"])
    done = {"path": 0, "none": 0, "ZeroDivisionError": 0, "ValueError": 0}
    for k in range(len(r["n"])):
        n, a = int(r["n"][k]), [float(v) for v in r["inp"][k]]
        what = "path" if n > 0 else ("none" if n == 0 else str(r["mode"][k]))
        if done[what] >= 2:
            continue
        done[what] += 1
        if n < 0:
            with pytest.raises(ZeroDivisionError if what == "ZeroDivisionError" else ValueError):
                reeds_shepp_path_planning(*a)
        elif n == 0:
            assert reeds_shepp_path_planning(*a) == (None, None, None, None, None)
        else:
            px, py, pyaw, mode, ln = reeds_shepp_path_planning(*a)
            assert all(isinstance(v, list) for v in (px, py, pyaw, mode, ln)) and isinstance(px[0], float)
            o = int(goff[k])
            assert px == r["poly_x"][o:o + n].tolist() and py == r["poly_y"][o:o + n].tolist()
            assert pyaw == r["poly_yaw"][o:o + n].tolist() and "".join(mode) == str(r["mode"][k])
            assert ln == r["lengths"][k][:int(r["n_len"][k])].tolist()
    assert done["path"] == 2 and done["none"] >= 1 and done["ZeroDivisionError"] + done["ValueError"] >= 2

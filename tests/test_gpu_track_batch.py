"""Batched closed-loop tracking of courses given as data on the GPU (BatchTrack, rrtx_tracker_*): the reference's
known-answer vectors, every candidate course of the rrt_10 goldens, the capacities of the kernel (LDS / slab / refused) with
reference values, and the batch shapes at which a persistent-wave job queue can go wrong.  Every comparison is of uint64
views; no vector is skipped."""
import os

import numpy as np
import pytest

import util
import track_util as tu
from test_track_batch_host import kat_vectors

pytestmark = pytest.mark.gpu
DEFAULT_STATE = np.array([-0.0, -0.0, 0.0, 0.0])
REC_FIELDS = ("find_goal", "length", "fail", "status")
ARRAYS = ("x", "y", "yaw", "v", "t", "a", "d")


@pytest.fixture(scope="module")
def bt():
    import rrt_amd
    with rrt_amd.BatchTrack() as b:
        yield b


def run_vectors(bt, vecs, arrays=True):
    """One run() of track_kat-style vectors: everything per course."""
    starts = np.array([v[6] for v in vecs]).reshape(-1, 4)
    preset = np.any(tu.bits(starts) != tu.bits(DEFAULT_STATE))
    return bt.run([(v[3], v[4], v[5]) for v in vecs], course_obstacles=[v[1] for v in vecs],
                  robot_radius=[v[2] for v in vecs], target_speed=[v[0]["target_speed"] for v in vecs],
                  yaw_th=[v[0]["yaw_th"] for v in vecs], invalid_travel_ratio=[v[0]["invalid_travel_ratio"] for v in vecs],
                  start_state=starts if preset else None, arrays=arrays)


def assert_vector(res, j, g, i):
    """Course j of `res` against vector i of a track_kat-style file: the record, t[-1], the last state and the sums."""
    assert int(res.status[j]) == 0, (j, i)
    assert [int(res.find_goal[j]), int(res.length[j]), int(res.fail[j])] == g["out"][i].tolist(), "vector %d" % i
    a, b = int(res.offsets[j]), int(res.offsets[j + 1])
    assert b - a == int(g["out"][i][1]), "vector %d" % i
    last = [res.t_last[j]] + [getattr(res, k)[b - 1] for k in ("x", "y", "yaw", "v", "a", "d")]
    assert np.array_equal(tu.bits(last), tu.bits(g["last"][i])), "vector %d last state" % i
    assert tu.bits([res.t[b - 1]])[0] == tu.bits([res.t_last[j]])[0], "vector %d t[-1]" % i
    sums = [float(sum(getattr(res, k)[a:b].tolist())) for k in ("x", "y", "yaw", "v", "a", "d")]   # sequential Python sums
    assert np.array_equal(tu.bits(sums), tu.bits(g["sums"][i])), "vector %d sums" % i


def assert_same_records(a, b, what=""):
    for f in REC_FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    assert np.array_equal(tu.bits(a.t_last), tu.bits(b.t_last)), (what, "t_last")


def assert_same_arrays(a, b, what=""):
    assert np.array_equal(a.offsets, b.offsets), what
    for k in ARRAYS:
        assert np.array_equal(tu.bits(getattr(a, k)), tu.bits(getattr(b, k))), (what, k)


@pytest.fixture(scope="module")
def kat(bt):
    """track_kat.npz, its vectors, and all of them tracked in one run with arrays (shared; nobody changes it)."""
    g = np.load(os.path.join(tu.GOLD, "track_kat.npz"))
    g = {k: g[k] for k in g.files}
    vecs = kat_vectors(g)
    return g, vecs, run_vectors(bt, vecs)


def csr_inputs(vecs, copies):
    """The keywords of run() for `copies` repetitions of the vectors, as CSR arrays."""
    n = np.array([len(v[3]) for v in vecs])
    off = np.concatenate([[0], np.cumsum(np.tile(n, copies))])
    x, y, yaw = (np.tile(np.concatenate([v[k] for v in vecs]), copies) for k in (3, 4, 5))
    return dict(courses=(off, x, y, yaw), course_obstacles=[v[1] for v in vecs] * copies,
                robot_radius=np.tile([v[2] for v in vecs], copies),
                target_speed=np.tile([v[0]["target_speed"] for v in vecs], copies),
                yaw_th=np.tile([v[0]["yaw_th"] for v in vecs], copies),
                invalid_travel_ratio=np.tile([v[0]["invalid_travel_ratio"] for v in vecs], copies))


def test_all_known_answers_in_one_run(kat):
    g, vecs, res = kat
    assert len(res) == len(vecs) == 240 and res.rc == 0 and res.kernel_ms > 0.0
    for i in range(240):
        assert_vector(res, i, g, i)
    assert res.steps == int(g["out"][:, 1].sum()) == 106853 == len(res.x) == len(res.d)
    assert np.array_equal(res.offsets, np.concatenate([[0], np.cumsum(g["out"][:, 1])]))
    find, x, y, yaw, v, t, a, d = res.feasible(7)
    lo, hi = int(res.offsets[7]), int(res.offsets[8])
    assert find is bool(g["out"][7][0]) and isinstance(x, list) and x == res.x[lo:hi].tolist() and d == res.d[lo:hi].tolist()


def test_candidates_and_winners_of_the_planner_goldens(bt):
    courses_seen = steps_seen = 0
    for path in tu.goldens():
        g, kw, model = tu.load(path)
        assert {k: float(v) for k, v in bt.model.items()} == model
        courses = [tu.course(g, c, kw) for c in g["cand"]]
        res = bt.run(courses, obstacle_list=kw["obstacle_list"], robot_radius=kw["robot_radius"],
                     target_speed=kw["target_speed"], yaw_th=kw["yaw_th"], invalid_travel_ratio=kw["invalid_travel_ratio"])
        name = os.path.basename(path)
        assert res.rc == 0 and len(res) == len(g["cand"]) and np.all(res.status == 0), name
        assert np.array_equal(res.find_goal, g["cand_find"]) and np.array_equal(res.length, g["cand_len"]), name
        assert np.array_equal(res.fail, g["cand_fail"]), name
        assert np.array_equal(tu.bits(res.t_last), tu.bits(g["cand_tlast"])), name
        end = res.offsets[1:] - 1
        last = np.stack([getattr(res, k)[end] for k in ("x", "y", "yaw", "v", "a", "d")], axis=1).reshape(-1, 6)
        assert np.array_equal(tu.bits(last), tu.bits(g["cand_last"].reshape(-1, 6))), name
        best = res.best()
        assert best[0] is bool(g["flag"]), name
        for k, got in zip(ARRAYS, best[1:]):
            if g["flag"]:
                assert np.array_equal(tu.bits(got), tu.bits(g["out_" + k])), (name, k)
            else:
                assert got is None, (name, k)
        if name == "rrt10_none_s9.npz":      # no candidate: the empty run
            assert len(res) == 0 and res.steps == 0 and len(res.x) == 0 and res.offsets.tolist() == [0]
        courses_seen += len(res)
        steps_seen += res.steps
    assert (courses_seen, steps_seen) == (561, 276856)


def test_capacity_boundaries_start_states_and_64_obstacles(bt):
    import rrt_amd
    g = np.load(os.path.join(tu.GOLD, "track_batch_kat.npz"))
    g = {k: g[k] for k in g.files}
    vecs = kat_vectors(g)
    n = np.array([len(v[3]) for v in vecs])
    for want in (3, 448, 449, 700, 960):
        assert np.sum(n == want) >= 2
    i448, i960 = int(np.nonzero(n == 448)[0][0]), int(np.nonzero(n == 960)[0][0])
    v = vecs[i448]
    two = (v[0], v[1], v[2], v[3][:2], v[4][:2], v[5][:2], v[6])                      # the reference raises IndexError
    v = vecs[i960]
    step = [v[k][-1] + (v[k][-1] - v[k][-2]) for k in (3, 4)]
    too_long = (v[0], v[1], v[2], np.append(v[3], step[0]), np.append(v[4], step[1]), np.append(v[5], v[5][-1]), v[6])
    assert len(too_long[3]) == 961
    # the refused courses sit between accepted ones: behind the 448-point course and behind the first 960-point course
    order = []
    for i in range(len(vecs)):
        order.append(i)
        if i == i448:
            order.append("two")
        if i == i960:
            order.append("long")
    res = run_vectors(bt, [two if i == "two" else too_long if i == "long" else vecs[i] for i in order])
    assert res.rc == rrt_amd._abi.RRTX_PARTIAL
    for j, i in enumerate(order):
        if i == "two":
            assert res.status[j] == 2 and res.offsets[j] == res.offsets[j + 1] and res.length[j] == 0
            with pytest.raises(IndexError):
                res.feasible(j)
        elif i == "long":
            assert res.status[j] == 3 and res.offsets[j] == res.offsets[j + 1] and res.length[j] == 0
            with pytest.raises(rrt_amd._abi.RrtxError):
                res.feasible(j)
        else:
            assert_vector(res, j, g, i)
    assert res.steps == int(g["out"][:, 1].sum())
    # the preset start states were used: the roll-out's first sample is the state given
    j = order.index(int(np.nonzero(np.any(tu.bits(g["start_state"]) != tu.bits(DEFAULT_STATE), axis=1))[0][0]))
    a = int(res.offsets[j])
    assert np.array_equal(tu.bits([res.x[a], res.y[a], res.v[a]]), tu.bits(g["start_state"][order[j]][[0, 1, 3]]))
    i64 = int(np.nonzero(g["nobs"] == 64)[0][0])
    assert res.fail[order.index(i64)] & 8 and not res.fail[order.index(i64 + 1)] & 8


def test_more_jobs_than_resident_waves(bt, kat):
    """240 vectors x 18 = 4 320 courses, above the 4 096 blocks of 256 CUs x 16: every wave takes further jobs from the queue."""
    g, vecs, first = kat
    res = bt.run(arrays=False, **csr_inputs(vecs, 18))
    assert len(res) == 4320 and res.rc == 0 and res.x is None
    for f in REC_FIELDS:
        col = getattr(res, f).reshape(18, 240)
        assert np.array_equal(col, np.tile(getattr(first, f), (18, 1))), f
    assert np.array_equal(tu.bits(res.t_last).reshape(18, 240), np.tile(tu.bits(first.t_last), (18, 1)))
    assert res.steps == 18 * first.steps


def test_records_only_gives_the_same_records(bt, kat):
    import rrt_amd
    g, vecs, full = kat
    lean = run_vectors(bt, vecs, arrays=False)
    assert_same_records(lean, full)
    assert all(getattr(lean, k) is None for k in ARRAYS) and np.array_equal(lean.offsets, full.offsets)
    with pytest.raises(rrt_amd._abi.RrtxError):
        bt._tracker.arrays()          # RRTX_E_STATE: the last run stored no arrays
    with pytest.raises(rrt_amd._abi.RrtxError):
        lean.feasible(0)


def test_reused_tracker_describes_the_last_run_only(kat):
    import rrt_amd
    g, vecs, full = kat
    with rrt_amd.BatchTrack() as b:
        res = run_vectors(b, vecs)
        assert_same_records(res, full, "240")
        assert_same_arrays(res, full, "240")
        one = run_vectors(b, vecs[5:6])
        assert len(one) == 1 and b._tracker.counts() == (1, int(full.length[5]))
        assert_vector(one, 0, g, 5)
        many = b.run(**csr_inputs(vecs, 18))
        assert len(many) == 4320 and b._tracker.counts() == (4320, 18 * full.steps)
        lo, hi = 17 * full.steps, 18 * full.steps
        for k in ARRAYS:      # the last copy's arrays, behind regrown buffers
            assert np.array_equal(tu.bits(getattr(many, k)[lo:hi]), tu.bits(getattr(full, k))), k
        none = b.run([])
        assert len(none) == 0 and none.rc == 0 and b._tracker.counts() == (0, 0) and none.offsets.tolist() == [0]
        assert len(none.x) == 0 and none.best() == (False, None, None, None, None, None, None, None)
        again = run_vectors(b, vecs[:3])
        for i in range(3):
            assert_vector(again, i, g, i)


def test_steer_result_goes_straight_in(bt):
    import rrt_amd
    rs = np.random.RandomState(5)
    goals = np.stack([rs.uniform(-6, 8, 64), rs.uniform(-6, 8, 64), rs.uniform(-np.pi, np.pi, 64)], axis=1)
    with rrt_amd.BatchSteer("rs") as bs:
        sr = bs.plan(np.zeros((64, 3)), goals, 1.0)
    assert np.sum(sr.status == 0) >= 32
    direct = bt.run(sr, obstacle_list=[(3.0, 3.0, 0.5)], robot_radius=0.2)
    trip = [(sr.x[a:b].tolist(), sr.y[a:b].tolist(), sr.yaw[a:b].tolist()) for a, b in zip(sr.offsets[:-1], sr.offsets[1:])]
    listed = bt.run(trip, obstacle_list=[(3.0, 3.0, 0.5)], robot_radius=0.2)
    assert len(direct) == 64 and direct.steps > 0 and np.any(direct.find_goal == 1)
    assert_same_records(direct, listed)
    assert_same_arrays(direct, listed)
    empty = np.diff(sr.offsets) == 0
    assert np.all(direct.status[empty] == 2) and np.all(direct.status[~empty] == 0)
    assert direct.rc == (rrt_amd._abi.RRTX_PARTIAL if empty.any() else 0)


def test_default_start_state_is_the_reference_state(bt, kat):
    g, vecs, full = kat
    sub = vecs[:24]
    kw = dict(courses=[(v[3], v[4], v[5]) for v in sub], obstacle_list=[(2.0, 1.0, 0.4)], robot_radius=0.1)
    default = bt.run(start_state=None, **kw)
    explicit = bt.run(start_state=np.tile(DEFAULT_STATE, (24, 1)), **kw)
    assert_same_records(default, explicit)
    assert_same_arrays(default, explicit)
    first = default.offsets[:-1]
    assert np.all(np.signbit(default.x[first])) and np.all(np.signbit(default.y[first]))      # (-0.0, -0.0)
    assert np.all(np.signbit(explicit.x[first])) and np.all(np.signbit(explicit.y[first]))
    moved = bt.run(start_state=[0.5, -0.5, 0.1, 1.0], **kw)
    assert np.array_equal(moved.x[moved.offsets[:-1]], np.full(24, 0.5)) and not np.array_equal(moved.t_last, default.t_last)

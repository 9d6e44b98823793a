"""Batched inverse kinematics on the device (BatchArmIK, rrt_amd.simple_2d_inverse_kinematics): the kernels of
csrc/armik_batch.hip.h against the oracle bit for bit (tests/armik_oracle.py states the package's own step), against the
reference within the measured tolerance where the two are comparable (tests/armik_util.py), and the moves against the
reference's recorded trajectories bit for bit.  The shapes are the smallest at which the kernels can go wrong: N = 1, 2, 7, 8, 9,
15, 16 where numpy's sum changes form, arms of different N in one call, batches of 1, 63, 64, 65, and few persistent waves so that
every lane refills from the cursor and the last refill is partial."""
import numpy as np
import pytest

import armik_oracle as O
import armik_util as U

pytestmark = pytest.mark.gpu
IT = U.GOLDEN_ITERATIONS


def bits(v):
    return np.asarray(v, dtype=np.float64).reshape(-1).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def ik(gpu):
    import rrt_amd
    with rrt_amd.BatchArmIK(max_iterations=IT) as s:
        yield s


def solve_golden(ik, qs, waves=None):
    """Golden solves qs in one call, every query with its own arm"""
    cs = [U.solve(q) for q in qs]
    ik.waves, ik.max_iterations = waves, IT
    return ik.solve([c["L"] for c in cs], [c["ang0"] for c in cs], [c["goal"] for c in cs], arm=list(range(len(cs))))


def assert_solves(res, qs, what):
    """A result against the oracle bit for bit, and against the reference where the query is comparable"""
    assert len(res) == len(qs), what
    n_bad = 0
    for k, q in enumerate(qs):
        o = U.oracle_solve(q)
        w = (what, k, q, U.solve(q)["tag"])
        assert int(res.status[k]) == o["status"] and bool(res.found[k]) == (o["status"] == O.FOUND), w
        assert int(res.iterations[k]) == o["iterations"], w
        assert same_bits(res.angles_of(k), o["angles"]), w
        assert same_bits(res.end[k], o["end"]) and same_bits(res.distance[k], o["distance"]), w
        U.assert_comparable_within(q, res.angles_of(k), res.found[k], res.iterations[k], what)
        n_bad += o["status"] != O.FOUND
    assert res.partial == (n_bad > 0), what


def queries_of_n(n):
    return [q for q in range(U.n_solves()) if len(U.solve(q)["L"]) == n]


def test_all_golden_solves_in_one_call(ik):
    """293 queries, arms of 1 .. 16 links side by side, 0-iteration, few-iteration and cap queries in the same waves"""
    qs = list(range(U.n_solves()))
    res = solve_golden(ik, qs)
    assert_solves(res, qs, "all")
    assert res.partial and res.angles.ndim == 1 and res.offsets[-1] == len(res.angles)
    it = res.iterations
    assert np.any(it == 0) and np.any((it > 0) & (it < 16)) and np.any(it == IT)
    angles, found = res.result(0)
    assert isinstance(found, bool) and same_bits(angles, U.oracle_solve(0)["angles"])


@pytest.mark.parametrize("n", (1, 2, 7, 8, 9, 15, 16))
def test_link_counts_where_the_sum_changes_form(ik, n):
    qs = queries_of_n(n)
    assert len(qs) >= 20
    res = solve_golden(ik, qs)
    assert_solves(res, qs, "N %d" % n)
    assert res.angles.shape == (len(qs), n)


@pytest.mark.parametrize("count", (1, 63, 64, 65))
def test_batch_sizes(ik, count):
    qs = [(5 * k + count) % U.n_solves() for k in range(count)]
    assert_solves(solve_golden(ik, qs), qs, "%d queries" % count)


@pytest.mark.parametrize("waves,count", ((1, 130), (1, 257), (2, 3)))
def test_few_waves_refill_from_the_cursor(ik, waves, count):
    """One wave for 130 and for 257 queries: every lane refills, the last refill is partial.  Two waves for 3: an explicit
    `waves` is what is launched, so one wave finds the cursor spent on its first ask and leaves without a record"""
    qs = [(3 * k) % U.n_solves() for k in range(count)]
    res = solve_golden(ik, qs, waves=waves)
    assert_solves(res, qs, "waves %d, %d queries" % (waves, count))
    assert res.waves == waves


def test_the_refill_does_not_change_a_result(ik):
    qs = [(3 * k) % U.n_solves() for k in range(257)]
    one, three, dflt = (solve_golden(ik, qs, waves=w) for w in (1, 3, None))
    assert (one.waves, three.waves) == (1, 3) and dflt.waves == 5
    for other in (three, dflt):
        for key in ("status", "iterations", "end", "distance", "_flat", "offsets"):
            assert same_bits(getattr(one, key).astype(np.float64), getattr(other, key).astype(np.float64)), key


def test_mixed_iteration_counts_in_one_wave(ik):
    """64 queries of one wave: found at once, found in a few trips, and 200 trips without it"""
    pick = lambda f: [q for q in range(U.n_solves()) if f(U.oracle_solve(q))]   # noqa: E731
    qs = (pick(lambda o: o["iterations"] == 0)[:8] + pick(lambda o: 0 < o["iterations"] < 10)[:40]
          + pick(lambda o: o["status"] == O.NOT_FOUND)[:16])
    assert len(qs) == 64
    res = solve_golden(ik, qs, waves=1)
    assert_solves(res, qs, "mixed")
    assert sorted(set(res.status.tolist())) == [O.FOUND, O.NOT_FOUND]


def test_all_zero_start(ik):
    """The script's commented-out start: row 0 of J is exactly zero and the step takes the rank-1 form"""
    zero = [U.step(k) for k in range(U.n_steps()) if U.step(k)["kind"] == 1]
    assert sorted(len(c["L"]) for c in zero) == [2, 5]
    ik.waves, ik.max_iterations = None, IT
    res = ik.solve([c["L"] for c in zero], [c["ang"] for c in zero], [c["goal"] for c in zero])
    for k, c in enumerate(zero):
        o = O.solve(c["L"], c["ang"], c["goal"], 0.1, IT)
        assert (int(res.status[k]), int(res.iterations[k])) == (o["status"], o["iterations"])
        assert same_bits(res.angles_of(k), o["angles"]) and same_bits(res.distance[k], o["distance"])
        assert np.all(np.isfinite(res.angles_of(k)))


def test_far_goals_are_partial_and_the_other_queries_complete(ik):
    """Goals 1e5 units away (steps of thousands of turns: the replicas' large-argument paths; one query leaves their domain)
    among ordinary queries: RRTX_PARTIAL, and every other query of the call complete"""
    far, want = U.far_goal_queries()
    near = queries_of_n(5)[:24]
    cs = [U.solve(q) for q in near]
    ik.waves, ik.max_iterations = 2, IT
    res = ik.solve([L for L, _, _ in far] + [c["L"] for c in cs], [a for _, a, _ in far] + [c["ang0"] for c in cs],
                   [g for _, _, g in far] + [c["goal"] for c in cs])
    assert res.partial and len(res) == len(far) + len(near)
    for k, o in enumerate(want):
        assert (int(res.status[k]), int(res.iterations[k])) == (o["status"], IT), k
        assert same_bits(res.angles_of(k), o["angles"]) and same_bits(res.end[k], o["end"]) and same_bits(res.distance[k], o["distance"]), k
    assert O.NONFINITE in res.status[:len(far)] and O.NOT_FOUND in res.status[:len(far)]
    for k, q in enumerate(near):
        o = U.oracle_solve(q)
        assert int(res.status[len(far) + k]) == o["status"] and same_bits(res.angles_of(len(far) + k), o["angles"]), q


def move_golden(ik, ms, **kw):
    cs = [U.move(m) for m in ms]
    return ik.move([c["L"] for c in cs], [c["ang0"] for c in cs], [c["gang"] for c in cs], [c["goal"] for c in cs],
                   arm=list(range(len(cs))), **kw)


def test_all_golden_moves_are_the_references_bit_for_bit(ik):
    ms = list(range(U.n_moves()))
    res = move_golden(ik, ms)
    lean = move_golden(ik, ms, arrays=False)
    assert not res.partial and lean.traj_offsets is None
    for k, m in enumerate(ms):
        c = U.move(m)
        steps = len(c["tdist"])
        ta, td = res.trajectory(k)
        assert int(res.status[k]) == O.FOUND and bool(res.reached[k]) and int(res.n_steps[k]) == steps, (m, c["tag"])
        assert ta.shape == (steps, len(c["L"])) and same_bits(ta, c["tang"]) and same_bits(td, c["tdist"]), (m, c["tag"])
        assert same_bits(res.angles_of(k), c["tang"][-1] if steps else c["ang0"]), m
        o = U.oracle_move(m)
        assert same_bits(res.end[k], o["end"]) and same_bits(res.distance[k], o["distance"]), m
    for key in ("status", "n_steps", "end", "distance", "_flat", "offsets"):   # arrays=False: the same records
        assert same_bits(getattr(res, key).astype(np.float64), getattr(lean, key).astype(np.float64)), key
    assert res.traj_offsets[-1] == res.n_steps.sum() and np.any(res.n_steps == 0)
    with pytest.raises(ValueError):
        lean.trajectory(0)


def test_step_cap(ik):
    ms = list(range(U.n_moves()))
    res = move_golden(ik, ms, max_steps=3)
    assert res.partial
    for k, m in enumerate(ms):
        c = U.move(m)
        steps = min(3, len(c["tdist"]))
        assert int(res.status[k]) == (O.STEP_CAP if len(c["tdist"]) > 3 else O.FOUND) and int(res.n_steps[k]) == steps, m
        ta, td = res.trajectory(k)   # complete rows for the queries that end in time, three rows for the rest
        assert same_bits(ta, c["tang"][:steps]) and same_bits(td, c["tdist"][:steps]), m
    assert O.STEP_CAP in res.status and O.FOUND in res.status


def test_a_huge_gain_leaves_the_domain_of_sin_and_cos(ik):
    """Kp = 1e9: one step throws the angles past 105 414 357 rad, where the device's sin / cos end; the loop stops there with
    RRTX_ARMIK_NONFINITE, the step counted and the last pose kept -- as the oracle states it"""
    ms = [m for m in range(U.n_moves()) if len(U.move(m)["tdist"])][:6] + [m for m in range(U.n_moves()) if not len(U.move(m)["tdist"])][:1]
    res = move_golden(ik, ms, Kp=1.0e9)
    assert res.partial
    for k, m in enumerate(ms):
        c = U.move(m)
        o = O.move(c["L"], c["ang0"], c["gang"], c["goal"], Kp=1.0e9)
        assert (int(res.status[k]), int(res.n_steps[k])) == (o["status"], o["n_steps"]), m
        assert same_bits(res.angles_of(k), o["angles"]) and same_bits(res.end[k], o["end"]) and same_bits(res.distance[k], o["distance"]), m
        ta, td = res.trajectory(k)
        assert same_bits(ta, o["traj_angles"]) and same_bits(td, o["traj_distance"]), m
    assert O.NONFINITE in res.status and O.FOUND in res.status


def test_follow_line_walks_script_02s_rounds(ik):
    """Three goals in one batch, five rounds each: the chain against the oracle's bit for bit; sub-goals and round 0 are the
    reference's"""
    g = U.kat()
    ik.waves, ik.max_iterations = None, IT
    angles, rounds = ik.follow_line(U.DRIVER_LINKS, U.DRIVER_ANGLES, g["fl_goal"])
    assert angles.shape == (3, 5) and len(rounds) == 5
    for r in range(3):
        want, end = O.follow_line(U.DRIVER_LINKS, U.DRIVER_ANGLES, g["fl_goal"][r].tolist(), max_iterations=IT)
        assert same_bits(angles[r], end), r
        for i, (sub, s, m, moved) in enumerate(rounds):
            w = want[i]
            assert same_bits(sub[r], w["goal"]) and same_bits(sub[r], U.solve(int(g["fl_solve"][r, i]))["goal"]), (r, i)
            assert int(s.status[r]) == w["solve"]["status"] and int(s.iterations[r]) == w["solve"]["iterations"], (r, i)
            assert same_bits(s.angles_of(r), w["solve"]["angles"]), (r, i)
            assert (r in moved) == (w["move"] is not None), (r, i)
            if w["move"] is not None:
                k = moved.tolist().index(r)
                assert int(m.n_steps[k]) == w["move"]["n_steps"] and same_bits(m.angles_of(k), w["move"]["angles"]), (r, i)
        assert int(rounds[0][1].iterations[r]) == 0 and int(rounds[0][2].n_steps[r]) == 0
    # each recorded round on its own, from the reference's own start: the comparable rule for the solve (the moves, from the
    # reference's own joint_goal_angles, are among the golden moves)
    qs = [int(q) for q in g["fl_solve"].reshape(-1)]
    assert_solves(solve_golden(ik, qs), qs, "rounds of script 02")


def test_one_object_reused(gpu):
    """16 links then 2; 257 queries then 1; move after solve and solve again: every call serves what it wrote itself"""
    import rrt_amd
    with rrt_amd.BatchArmIK(max_iterations=IT) as ik:
        big = [queries_of_n(16)[k % 22] for k in range(257)]
        assert_solves(solve_golden(ik, big), big, "N 16, 257 queries")
        small = queries_of_n(2)[:1]
        assert_solves(solve_golden(ik, small), small, "N 2, 1 query")
        with pytest.raises(rrt_amd._abi.RrtxError):
            ik._ik.trajectory(1)                                                          # RRTX_E_STATE after a solve
        ms = [m for m in range(U.n_moves()) if len(U.move(m)["tdist"])][:3]
        res = move_golden(ik, ms)
        for k, m in enumerate(ms):
            assert same_bits(res.trajectory(k)[1], U.move(m)["tdist"]), m
        again = queries_of_n(16)[:5] + queries_of_n(1)[:5]
        assert_solves(solve_golden(ik, again), again, "solve after move")
        none = ik.solve(U.DRIVER_LINKS, U.DRIVER_ANGLES, np.zeros((0, 2)))
        assert len(none) == 0 and none.offsets.tolist() == [0] and not none.partial
        one_arm = ik.solve(U.DRIVER_LINKS, U.DRIVER_ANGLES, [U.solve(q)["goal"] for q in range(U.n_solves()) if U.solve(q)["tag"] == "driver_area"])
        drv = [q for q in range(U.n_solves()) if U.solve(q)["tag"] == "driver_area"]   # one arm, one start row broadcast
        assert one_arm.angles.shape == (len(drv), 5)
        assert_solves(one_arm, drv, "driver area, one arm broadcast")
        with pytest.raises(rrt_amd._abi.RrtxError):
            ik.solve(U.DRIVER_LINKS, U.DRIVER_ANGLES, [[float("nan"), 0.0]])
        ik.waves = 0
        with pytest.raises(rrt_amd._abi.RrtxError):
            ik.solve(U.DRIVER_LINKS, U.DRIVER_ANGLES, [[1.0, 2.0]])                       # waves >= 1 when given


def test_dropin_module_is_a_batch_of_one(gpu, capsys):
    import rrt_amd.simple_2d_inverse_kinematics as ik
    ik.N_ITERATIONS = IT
    try:
        qs = queries_of_n(5)[:4] + [q for q in range(U.n_solves()) if U.solve(q)["tag"] == "driver_area"][:6] + queries_of_n(16)[:2]
        for q in qs:
            c, o = U.solve(q), U.oracle_solve(q)
            ik.N_LINKS = len(c["L"])
            angles, found = ik.inverse_kinematics(c["L"], np.array(c["ang0"]), np.array(c["goal"]))
            out = capsys.readouterr().out
            assert isinstance(found, bool) and found == (o["status"] == O.FOUND) and same_bits(angles, o["angles"]), q
            assert (("Solution found in %d iterations." % o["iterations"]) in out) == found, q
            U.assert_comparable_within(q, angles, found, o["iterations"], "drop-in")
    finally:
        ik.N_ITERATIONS, ik.N_LINKS = 10000, 5

"""Shared by tests/test_armik_host.py and tests/test_gpu_armik.py -- TEST INFRASTRUCTURE: the known-answer file of BatchArmIK
(tools/gen_golden_armik.py), the oracle's answers, each computed once and never written, and the two tolerances of the
comparison with the reference's LAPACK step.

The step pinv(J) @ errors is this package's own closed form (csrc/rpp_armik.h), so agreement with the reference is measured
where it is defined:
  TOL_STEP    the largest max|delta - delta_ref| / (kappa * max|delta_ref|) over the golden steps, kappa = sigma_1 / sigma_2 from
              numpy's recorded singular values (1 for rank 1); steps with kappa > 1e6, and steps on which the definition's rank
              decision differs from numpy's (sigma_2 <= 1e-15 sigma_1 is rank 1 there), are outside it
  TOL_SOLVE   the largest absolute angle deviation over the comparable solves (the reference finished in at most 16 iterations
              and no visited distance lies within 1e-9 of 0.1), which must also agree exactly in found and iterations
Each constant is 16 x the gap the generator's run printed; test_tolerances_are_the_measured_ones holds gap <= TOL <= 64 gap."""
import os

import numpy as np

import armik_oracle as O
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
TAGS = ("random", "start_within", "beyond_reach", "driver_area", "one_link", "follow_round")
MOVE_TAGS = ("found_query", "no_step", "wraps", "follow_round")
DRIVER_LINKS = [0.5, 1.5, 1.8, 1.2, 0.5]
DRIVER_ANGLES = [1.6, -1.6, 0.8, -0.5, 0.6]
GOLDEN_ITERATIONS = 200
KAPPA_MAX = 1.0e6
TOL_STEP = 1.72e-14    # 16 x 1.073e-15, the generator's print
TOL_SOLVE = 1.76e-10   # 16 x 1.101e-11
_cache = {}


def kat():
    """tests/golden/armik_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "armik_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def _rows(off, k, *names):
    g = kat()
    a, b = int(g[off][k]), int(g[off][k + 1])
    return [g[n][a:b].tolist() for n in names]


def n_steps():
    return len(kat()["st_dist"])


def step(k):
    """dict(L, ang, goal, pos, err, dist, J0, J1, P0, P1, delta, sv, kind) of golden step k"""
    g = kat()
    L, ang, J0, J1, P0, P1, delta = _rows("st_off", k, "st_L", "st_ang", "st_J0", "st_J1", "st_P0", "st_P1", "st_delta")
    return dict(L=L, ang=ang, J0=J0, J1=J1, P0=P0, P1=P1, delta=delta, goal=g["st_goal"][k].tolist(), pos=g["st_pos"][k].tolist(),
                err=g["st_err"][k].tolist(), dist=float(g["st_dist"][k]), sv=g["st_sv"][k].tolist(), kind=int(g["st_kind"][k]))


def n_solves():
    return len(kat()["so_iter"])


def solve(q):
    """dict(L, ang0, goal, ang, found, iters, tag, comparable) of golden solve q"""
    g = kat()
    L, ang0, ang = _rows("so_off", q, "so_L", "so_ang0", "so_ang")
    return dict(L=L, ang0=ang0, ang=ang, goal=g["so_goal"][q].tolist(), found=bool(g["so_found"][q]), iters=int(g["so_iter"][q]),
                tag=TAGS[g["so_tag"][q]], comparable=bool(g["so_comparable"][q]))


def n_moves():
    return len(kat()["mv_tag"])


def move(m):
    """dict(L, ang0, gang, goal, tag, tdist [steps], tang [steps][N]) of golden move m"""
    g = kat()
    L, ang0, gang = _rows("mv_off", m, "mv_L", "mv_ang0", "mv_gang")
    tdist = g["mv_tdist"][g["mv_step_off"][m]:g["mv_step_off"][m + 1]]
    tang = g["mv_tang"][g["mv_tang_off"][m]:g["mv_tang_off"][m + 1]].reshape(len(tdist), len(L))
    return dict(L=L, ang0=ang0, gang=gang, goal=g["mv_goal"][m].tolist(), tag=MOVE_TAGS[g["mv_tag"][m]], tdist=tdist, tang=tang)


def oracle_solve(q):
    """The oracle's answer to golden solve q at the golden file's 200 iterations"""
    key = ("os", q)
    if key not in _cache:
        c = solve(q)
        _cache[key] = O.solve(c["L"], c["ang0"], c["goal"], 0.1, GOLDEN_ITERATIONS)
    return _cache[key]


def oracle_move(m):
    key = ("om", m)
    if key not in _cache:
        c = move(m)
        _cache[key] = O.move(c["L"], c["ang0"], c["gang"], c["goal"])
    return _cache[key]


def far_goal_queries():
    """40 seeded queries whose goals lie 1e5 units away: huge steps, angles up to 1e8 rad and beyond.  None is ever found; at 200
    iterations one of them leaves the domain of the device's sin / cos (NONFINITE).  [(L, angles, goal)], and the oracle's
    answers at 200 iterations"""
    if "far" not in _cache:
        rs = np.random.RandomState(5)
        qs = []
        for _ in range(40):
            n = int(rs.choice([2, 3, 5, 8, 16]))
            L, a = rs.uniform(0.3, 2.0, n).tolist(), rs.uniform(-3, 3, n).tolist()
            th = rs.uniform(-3, 3)
            qs.append((L, a, [1e5 * np.cos(th), 1e5 * np.sin(th)]))
        _cache["far"] = (qs, [O.solve(L, a, goal, 0.1, GOLDEN_ITERATIONS) for L, a, goal in qs])
    return _cache["far"]


def numpy_rank(c):
    """The rank np.linalg.pinv gave J of golden step c: singular values at or below 1e-15 of the largest are cut"""
    return sum(1 for s in c["sv"][:min(2, len(c["L"]))] if s > 1e-15 * c["sv"][0])


def step_gap():
    """(gap, steps excluded, steps): the measure TOL_STEP bounds, with the oracle's step on the reference's own J and errors"""
    gap, excluded = 0.0, 0
    for k in range(n_steps()):
        c = step(k)
        delta, rank = O.step_delta(c["J0"], c["J1"], c["err"][0], c["err"][1])
        r_np = numpy_rank(c)
        kappa = c["sv"][0] / c["sv"][1] if r_np == 2 else 1.0
        if rank != r_np or kappa > KAPPA_MAX:
            excluded += 1
            continue
        ref = np.array(c["delta"])
        gap = max(gap, float(np.max(np.abs(np.array(delta) - ref)) / (kappa * np.max(np.abs(ref)))))
    return gap, excluded, n_steps()


def solve_gap():
    """The measure TOL_SOLVE bounds; found and iterations of the comparable solves must be the reference's"""
    gap = 0.0
    for q in range(n_solves()):
        c = solve(q)
        if c["comparable"]:
            o = oracle_solve(q)
            assert (o["status"] == O.FOUND) == c["found"] and o["iterations"] == c["iters"], (q, o["status"], o["iterations"], c["iters"])
            gap = max(gap, float(np.max(np.abs(np.array(o["angles"]) - np.array(c["ang"])))))
    return gap


def assert_comparable_within(q, angles, found, iterations, what):
    """A solve of golden query q against the reference, by the rule above"""
    c = solve(q)
    if c["comparable"]:
        assert bool(found) == c["found"] and int(iterations) == c["iters"], (what, q)
        dev = float(np.max(np.abs(np.asarray(angles) - np.array(c["ang"]))))
        assert dev <= TOL_SOLVE, (what, q, dev)

"""Shared by tests/test_armdh_host.py and tests/test_gpu_armdh.py -- TEST INFRASTRUCTURE: the known-answer file of BatchArmDH
(tools/gen_golden_armdh.py), the oracle's answers, each computed once and never written, and the tolerances of the comparison with
the reference's LAPACK steps.

The step is this package's own definition (csrc/rpp_armdh.h), so agreement with the reference is measured where it is defined:
  TOL_STEP[m]    the largest max|delta - delta_ref| / (kappa * max|delta_ref|) over the golden steps; newton: kappa = sigma_1 / the
                 smallest singular value numpy kept, and steps with a singular value within a factor 2 of numpy's cut
                 (1e-15 sigma_1) are outside it; lm: kappa of the matrix M
  TOL_SOLVE[m]   the largest absolute deviation of the final angles over the comparable solves of 100 trips: along the
                 reference's path the fold distance | |atan2(T12, T02)| - pi/2 | and the gimbal distance hypot(T02, T12) stay at or
                 above 0.05 and kappa_eff of J at or below 1e3 (newton) or 1e4 (lm: beyond it
                 M's condition passes 1e8 and Cholesky parts from the reference's SVD inverse by 1e-8 rad)
  TOL_DRIVER[m]  the same deviation on the script's own driver solve (zero start, exactly singular, 500 trips), which has its own
                 tag and is outside the fences
Each constant is 16 x the gap the generator's run printed; test_tolerances_are_the_measured_ones holds gap <= TOL <= 64 gap."""
import os

import numpy as np

import armdh_oracle as O
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
TAGS = ("random", "driver", "orig", "hard_singular", "hard_far", "short_arm")
METHODS = ("newton", "lm")
ARM_N = (1, 2, 5, 6, 7, 8)
HP = np.pi / 2.
SCRIPT_ARM = [[0., HP, 0., 0.13156], [0., 0., -0.1104, 0.], [0., 0., -0.096, 0.], [0., HP, 0., 0.06639], [0., -HP, 0., 0.07318],
              [0., 0., 0., 0.0436]]
DRIVER_REF = [0.15, 0.2, 0.1, 0.0, 0.0, 0.2]
EPS_LM = 1e-5
KAPPA_FENCE, KAPPA_FENCE_LM, FOLD_FENCE, GIMBAL_FENCE = 1.0e3, 1.0e4, 0.05, 0.05
GAP_STEP = (4.927e-15, 6.461e-16)     # the generator's print, (newton, lm)
GAP_SOLVE = (6.217e-15, 6.159e-12)
GAP_DRIVER = (1.679e-09, 1.008e-13)
TOL_STEP = (7.88e-14, 1.03e-14)       # 16 x the gap, each
TOL_SOLVE = (9.95e-14, 9.85e-11)
TOL_DRIVER = (2.69e-08, 1.61e-12)
_cache = {}
OTHER_HOST = "this host's arithmetic is not the golden host's (README): the doubles of the reference can differ here"


def kat():
    """tests/golden/armdh_kat.npz as a dict of arrays"""
    if "kat" not in _cache:
        with np.load(os.path.join(GOLD, "armdh_kat.npz")) as g:
            _cache["kat"] = {k: g[k] for k in g.files}
    return _cache["kat"]


def n_forward():
    return len(kat()["fw_pos"])


def forward(k):
    """dict(dh [N][4], T (N, 4, 4), J [6][N], pos, e2, e, quat, rpy) of golden forward record k"""
    g = kat()
    a, b = int(g["fw_off"][k]), int(g["fw_off"][k + 1])
    return dict(dh=g["fw_dh"][a:b].tolist(), T=g["fw_T"][a:b], J=g["fw_Jt"][a:b].T.tolist(), pos=g["fw_pos"][k], e2=g["fw_e2"][k],
                e=g["fw_e"][k], quat=g["fw_quat"][k], rpy=g["fw_rpy"][k])


def n_steps():
    return len(kat()["st_keff"])


def step(k):
    """dict(J [6][N], diff, K, delta, delta_lm, sv, keff, kM) of golden step k"""
    g = kat()
    a, b = int(g["st_off"][k]), int(g["st_off"][k + 1])
    return dict(J=g["st_Jt"][a:b].T.tolist(), diff=g["st_diff"][k].tolist(), K=g["st_K"][k].tolist(), delta=g["st_delta"][a:b],
                delta_lm=g["st_delta_lm"][a:b], sv=g["st_sv"][k], keff=float(g["st_keff"][k]), kM=float(g["st_kM"][k]))


def n_solves():
    return len(kat()["so_iter"])


def solve(q):
    """dict(dh, ref, ang, method, iters, div, tag, kmax, fold, gimbal, comparable) of golden solve q"""
    g = kat()
    a, b = int(g["so_off"][q]), int(g["so_off"][q + 1])
    return dict(dh=g["so_dh"][a:b].tolist(), ang=g["so_ang"][a:b], ref=g["so_ref"][q].tolist(), method=int(g["so_method"][q]),
                iters=int(g["so_iter"][q]), div=float(g["so_div"][q]), tag=TAGS[g["so_tag"][q]], kmax=float(g["so_kmax"][q]),
                fold=float(g["so_fold"][q]), gimbal=float(g["so_gimbal"][q]), comparable=bool(g["so_comparable"][q]))


def oracle_forward(k):
    key = ("of", k)
    if key not in _cache:
        _cache[key] = O.forward_record(forward(k)["dh"])
    return _cache[key]


def oracle_solve(q, iters=None):
    """The oracle's answer to golden solve q (at its own trip count, or at `iters`)"""
    c = solve(q)
    key = ("os", q, iters or c["iters"])
    if key not in _cache:
        _cache[key] = O.solve(c["dh"], c["ref"], iters or c["iters"], c["div"], METHODS[c["method"]], EPS_LM)
    return _cache[key]


def near_cut(c):
    n = len(c["J"][0])
    return any(0.5e-15 * c["sv"][0] < s < 2e-15 * c["sv"][0] for s in c["sv"][:min(6, n)])


def step_gap(method):
    """(gap, steps excluded, steps): the measure TOL_STEP[method] bounds, with the oracle's step on the reference's own J, K, diff"""
    gap, excluded = 0.0, 0
    for k in range(n_steps()):
        c = step(k)
        if method == 0 and near_cut(c):
            excluded += 1
            continue
        delta, status, _, _ = O.step(c["J"], c["K"], c["diff"], METHODS[method], EPS_LM)
        assert status == O.OK, (k, status)
        ref = c["delta_lm"] if method else c["delta"]
        kappa = c["kM"] if method else c["keff"]
        gap = max(gap, float(np.max(np.abs(np.array(delta) - ref)) / (kappa * np.max(np.abs(ref)))))
    return gap, excluded, n_steps()


def comparable_solves(method):
    return [q for q in range(n_solves()) if solve(q)["method"] == method and solve(q)["tag"] != "driver" and solve(q)["comparable"]]


def solve_gap(method):
    """The measure TOL_SOLVE[method] bounds"""
    return max(float(np.max(np.abs(np.array(oracle_solve(q)["angles"]) - solve(q)["ang"]))) for q in comparable_solves(method))


def driver_solve(method):
    return [q for q in range(n_solves()) if solve(q)["method"] == method and solve(q)["tag"] == "driver"][0]


def driver_gap(method):
    q = driver_solve(method)
    return float(np.max(np.abs(np.array(oracle_solve(q)["angles"]) - solve(q)["ang"])))


def bad_status_queries():
    """[(dh, ref, iters, div, method, eps, status)], each legal at the interface: a step that leaves the finite numbers (the smallest
    divisor there is), a step that takes a theta beyond the domain of the replicas' sin / cos (finite, past 105 414 357 rad), and an lm
    system whose pivot is not positive (eps so small that M of an 8-link arm is singular in doubles)"""
    return [(SCRIPT_ARM, DRIVER_REF, 3, 5e-324, "newton", 1e-5, O.NONFINITE),
            (SCRIPT_ARM, [1e6, -1e6, 1e6, 0.0, 0.0, 0.0], 40, 1e-6, "newton", 1e-5, O.NONFINITE),
            ([r[:] for r in SCRIPT_ARM] + [[0.2, 0.0, 0.0, 0.0]] * 2, DRIVER_REF + [], 5, 200.0, "lm", 1e-300, O.NO_CONVERGENCE)]


def mixed_status_cases():
    """[(good golden solves, dh, ref, iters, div, method, eps, status)] for one call in which iter_cnt, step_div, method and eps are
    shared: the bad query is bad by its own data (a target 1e6 away whose first step passes 105 414 357 rad; an 8-link arm
    whose M is singular in doubles under eps = 1e-300), the good ones -- golden solves on the script's arm -- stay OK"""
    good = [q for q in range(n_solves()) if solve(q)["tag"] == "random" and [r[1:] for r in solve(q)["dh"]] == [r[1:] for r in SCRIPT_ARM]][:3]
    b = bad_status_queries()
    return [(good, SCRIPT_ARM, b[1][1], 5, 0.01, "newton", 1e-5, O.NONFINITE), (good,) + b[2]]

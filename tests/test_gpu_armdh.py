"""Batched DH-arm kinematics on the device (BatchArmDH, rrt_amd.forward_inverse_kinematics and its _orig twin): the kernels of
csrc/armdh_batch.hip.h against the reference's recorded forward passes bit for bit, against the oracle bit for bit
(tests/armdh_oracle.py states the package's own step), and against the reference's solves within the measured tolerances where
the two are comparable (tests/armdh_util.py).  The shapes are the smallest at which the kernels can go wrong: N = 1, 2, 5, 6, 7, 8
in calls of their own and side by side, batches of 1, 63, 64 and 65 (one wave a block), 1, 2 and 100 trips, both methods, both
step divisors."""
import numpy as np
import pytest

import armdh_oracle as O
import armdh_util as U

pytestmark = pytest.mark.gpu


def bits(v):
    return np.asarray(v, dtype=np.float64).reshape(-1).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def dh(gpu):
    import rrt_amd
    with rrt_amd.BatchArmDH() as s:
        yield s


def check_forward(fw, k_of, what):
    """Query i of a forward result against golden record k_of[i], bit for bit; quat and rpy where the reference has them"""
    assert len(fw) == len(k_of) and not fw.partial, what
    for i, k in enumerate(k_of):
        c = U.forward(k)
        w = (what, i, k, U.OTHER_HOST)
        assert fw.status[i] == O.OK, w
        assert same_bits(fw.transforms_of(i), c["T"]) and same_bits(fw.jacobian_of(i), c["J"]), w
        assert same_bits(fw.position[i], c["pos"]) and same_bits(fw.euler2[i], c["e2"]) and same_bits(fw.euler[i], c["e"]), w
        if np.all(np.isfinite(c["quat"])):
            assert same_bits(fw.quat[i], c["quat"]), w
            if np.all(np.isfinite(c["rpy"])):
                assert same_bits(fw.rpy[i], c["rpy"]), w


def run_solves(dh, qs, iters=None):
    """Golden solves qs (one method, one divisor) in one call, every query with its own arm"""
    cs = [U.solve(q) for q in qs]
    assert len({(c["method"], c["div"], c["iters"]) for c in cs}) == 1
    return dh.solve([c["dh"] for c in cs], None, [c["ref"] for c in cs], iter_cnt=iters or cs[0]["iters"], step_div=cs[0]["div"],
                    method=U.METHODS[cs[0]["method"]], eps=U.EPS_LM)


def check_solves(res, qs, what, iters=None):
    """A result against the oracle bit for bit, and at the goldens' own trip count against the reference where comparable"""
    assert len(res) == len(qs), what
    n_bad = 0
    for i, q in enumerate(qs):
        c, o = U.solve(q), U.oracle_solve(q, iters)
        w = (what, i, q, c["tag"])
        assert int(res.status[i]) == o["status"] and int(res.n_cut[i]) == o["n_cut"] and same_bits(res.kappa_max[i], o["kappa_max"]), w
        assert same_bits(res.angles_of(i), o["angles"]) and same_bits(res.pose[i], o["pose"]) and same_bits(res.pose_error[i], o["pose_error"]), w
        if iters is None and c["tag"] != "driver" and c["comparable"]:
            dev = float(np.max(np.abs(res.angles_of(i) - c["ang"])))
            assert dev <= U.TOL_SOLVE[c["method"]], (w, dev)
        n_bad += o["status"] != O.OK
    assert res.partial == (n_bad > 0), what


def group(method, div=200.0, n=None):
    return [q for q in range(U.n_solves()) if (lambda c: c["method"] == method and c["div"] == div and c["iters"] == 100
                                               and (n is None or len(c["dh"]) == n))(U.solve(q))]


def test_all_golden_forward_records_in_one_call(dh):
    """480 queries, arms of 1 .. 8 links side by side, thetas up to 1e6 rad"""
    ks = list(range(U.n_forward()))
    fw = dh.forward([U.forward(k)["dh"] for k in ks])
    check_forward(fw, ks, "all")


@pytest.mark.parametrize("n", U.ARM_N)
def test_forward_per_link_count(dh, n):
    """One arm of N links with (Q, N) joint angles that replace column 0"""
    ks = [k for k in range(U.n_forward()) if len(U.forward(k)["dh"]) == n][:12]
    for k in ks[:3]:
        c = U.forward(k)
        same = [j for j in ks if [r[1:] for r in U.forward(j)["dh"]] == [r[1:] for r in c["dh"]]]
        arm = [[123.0] + r[1:] for r in c["dh"]]   # column 0 is replaced
        fw = dh.forward(arm, np.array([[r[0] for r in U.forward(j)["dh"]] for j in same]))
        check_forward(fw, same, "N = %d" % n)


@pytest.mark.parametrize("batch", (1, 63, 64, 65))
def test_forward_batch_sizes(dh, batch):
    ks = [(7 * i) % U.n_forward() for i in range(batch)]
    check_forward(dh.forward([U.forward(k)["dh"] for k in ks]), ks, "batch of %d" % batch)


@pytest.mark.parametrize("method", (0, 1))
def test_all_golden_solves_of_100_trips(dh, method):
    """Arms of 1 .. 8 links side by side: against the oracle bit for bit, against the reference within TOL_SOLVE where comparable"""
    qs = group(method)
    assert {len(U.solve(q)["dh"]) for q in qs} == set(U.ARM_N) and sum(U.solve(q)["comparable"] for q in qs) >= 15
    check_solves(run_solves(dh, qs), qs, U.METHODS[method])


@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("n", U.ARM_N)
def test_solves_per_link_count(dh, n, method):
    qs = group(method, n=n)[:4]
    assert qs
    check_solves(run_solves(dh, qs), qs, "N = %d" % n)


def test_solves_with_the_twins_divisor(dh):
    qs = group(0, div=100.0)
    assert len(qs) >= 3
    check_solves(run_solves(dh, qs), qs, "/100")


@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("iters", (1, 2))
def test_one_and_two_trips(dh, iters, method):
    qs = group(method)[::3]
    check_solves(run_solves(dh, qs, iters), qs, "%d trips" % iters, iters)


@pytest.mark.parametrize("batch", (1, 63, 64, 65))
def test_solve_batch_sizes(dh, batch):
    """The same golden queries over and over: the last block of 65 holds one lane"""
    for method in (0, 1):
        base = group(method)
        qs = [base[i % len(base)] for i in range(batch)]
        check_solves(run_solves(dh, qs), qs, "batch of %d, %s" % (batch, U.METHODS[method]))


@pytest.mark.parametrize("method", (0, 1))
def test_the_scripts_driver_solve(dh, method):
    """Zero start (exactly singular), ref_ee_pose = [0.15, 0.2, 0.1, 0, 0, 0.2], 500 trips"""
    q = U.driver_solve(method)
    res = dh.solve(U.SCRIPT_ARM, None, U.DRIVER_REF, method=U.METHODS[method])   # the defaults are the script's
    check_solves(res, [q], "driver")
    dev = float(np.max(np.abs(res.result(0) - U.solve(q)["ang"])))
    print("%s: driver deviation %.3e" % (U.METHODS[method], dev))
    assert dev <= U.TOL_DRIVER[method]
    if method == 0:
        assert res.n_cut[0] >= 1 and res.kappa_max[0] > 1e4


def test_bad_queries_among_good_ones(dh):
    """A step that takes a theta beyond the domain of sin / cos, and an lm pivot that is not positive, each among good queries of
    the same call: the call is partial, the bad query reports its status, the others are complete"""
    for good, arm, ref, iters, div, method, eps, status in U.mixed_status_cases():
        cs = [U.solve(q) for q in good]
        arms, refs = [cs[0]["dh"], arm, cs[1]["dh"], cs[2]["dh"]], [cs[0]["ref"], ref, cs[1]["ref"], cs[2]["ref"]]
        res = dh.solve(arms, None, refs, iter_cnt=iters, step_div=div, method=method, eps=eps)
        assert res.partial and res.status.tolist() == [O.OK, status, O.OK, O.OK], method
        for i in range(4):
            o = O.solve(arms[i], refs[i], iters, div, method, eps)
            assert o["status"] == res.status[i] and same_bits(res.angles_of(i), o["angles"]), (method, i)
            assert same_bits(res.pose[i], o["pose"]) and same_bits(res.pose_error[i], o["pose_error"]), (method, i)


def test_a_batch_split_into_two_calls_gives_the_same_bits(dh):
    for method in (0, 1):
        qs = group(method)
        whole = run_solves(dh, qs)
        cut = len(qs) // 3
        a, b = run_solves(dh, qs[:cut]), run_solves(dh, qs[cut:])
        assert same_bits(whole._flat, np.concatenate([a._flat, b._flat]))
        assert same_bits(whole.pose, np.concatenate([a.pose, b.pose])) and same_bits(whole.kappa_max, np.concatenate([a.kappa_max, b.kappa_max]))
        assert np.array_equal(whole.status, np.concatenate([a.status, b.status])) and np.array_equal(whole.n_cut, np.concatenate([a.n_cut, b.n_cut]))
    ks = list(range(0, U.n_forward(), 3))
    arms = [U.forward(k)["dh"] for k in ks]
    whole, a, b = dh.forward(arms), dh.forward(arms[:70]), dh.forward(arms[70:])
    assert same_bits(whole.transforms, np.concatenate([a.transforms, b.transforms])) and same_bits(whole._jac, np.concatenate([a._jac, b._jac]))


def test_dropin_modules_run_on_the_scripts_link_list(dh):
    import rrt_amd.forward_inverse_kinematics as fk
    import rrt_amd.forward_inverse_kinematics_orig as fo
    link_list = [list(r) for r in U.SCRIPT_ARM]
    q = U.driver_solve(0)
    fk.inverse_kinematics(500, link_list, U.DRIVER_REF)
    assert same_bits([r[0] for r in link_list], U.oracle_solve(q)["angles"])   # mutated in place, as the script does
    assert [r[1:] for r in link_list] == [r[1:] for r in U.SCRIPT_ARM]
    loc, glob, J = fk.forward_kinematics(link_list)
    want = O.forward_record(link_list)
    assert len(loc) == len(glob) == 6 and J.shape == (6, 6) and same_bits(glob, want["transforms"]) and same_bits(J, want["J"])
    assert same_bits(fk.rot2euler2(glob[-1]), U.oracle_solve(q)["pose"][3:])
    q = group(0, div=100.0)[0]
    c = U.solve(q)
    arm = fo.NLinkArm([list(r) for r in c["dh"]])
    arm.inverse_kinematics(100, c["ref"])
    assert same_bits([lk.dh_params_[0] for lk in arm.link_list], U.oracle_solve(q)["angles"])
    assert float(np.max(np.abs(np.array([lk.dh_params_[0] for lk in arm.link_list]) - c["ang"]))) <= U.TOL_SOLVE[0]
    assert same_bits(arm.forward_kinematics(), U.oracle_solve(q)["pose"]) and same_bits(arm.basic_jacobian(), O.forward(arm._rows())[1])

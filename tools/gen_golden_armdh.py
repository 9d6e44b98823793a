"""Golden generator of BatchArmDH: runs the reference's own functions of 01_forward_inverse_kinematics.py and
01_forward_inverse_kinematics_orig.py, loaded through oracle/ref_loader.py (the file names are added to ref_loader.FILES at run
time; the per-trip print is swallowed), and writes tests/golden/armdh_kat.npz.  Build host only (needs the reference checkout).

    python tools/gen_golden_armdh.py

inverse_kinematics (:387-438) is walked statement by statement with the reference's own forward_kinematics and rot2euler2 to
record what it visits, and the walk is held against the function itself (newton, /200) and against NLinkArm.inverse_kinematics
(/100).  The Levenberg-Marquardt lines are comments inside the function (:423-428) and live code in the check cell (:582-587):
the walk states them as written there, with eps the argument.

Arrays only.  CSR offsets are in links.
Forward records (n_fw): fw_off (n_fw + 1,) into fw_dh (links, 4) [theta, alpha, a, d], fw_T (links, 4, 4) the global transforms,
fw_Jt (links, 6) the columns of J; fw_pos (n_fw, 3), fw_e2 rot2euler2, fw_e rot2euler, fw_quat (n_fw, 4), fw_rpy (NaN where the
reference raises on the square root of a negative number).
Steps (n_st states along the reference's trajectories): st_off into st_Jt (links, 6), st_delta (numpy's newton step
dot(dot(pinv(J), K_alpha), diff)) and st_delta_lm (the lm step, eps = 1e-5); st_diff (n_st, 6), st_K (n_st, 3, 3), st_sv (n_st, 6)
numpy's singular values of J (zero-padded), st_keff sigma_1 / the smallest one numpy kept, st_kM the condition number of the lm
matrix.
Solves (n_so): so_off into so_dh (links, 4; column 0 the start) and so_ang (the thetas the reference left in link_list);
so_ref (n_so, 6), so_method (0 newton, 1 lm), so_iter, so_div, so_tag (TAGS), so_kmax, so_fold, so_gimbal (the fence quantities
along the reference's path) and so_comparable.
The gaps of the tolerances (tests/armdh_util.py) are printed at the end.
"""
import contextlib
import io
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_loader  # noqa: E402

ref_loader.FILES["dh_01"] = "01_forward_inverse_kinematics.py"
ref_loader.FILES["dh_01_orig"] = "01_forward_inverse_kinematics_orig.py"
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ("random", "driver", "orig", "hard_singular", "hard_far", "short_arm")
HP = math.pi / 2.
# the script's three link_list settings in its live column order [theta, alpha, a, d] (:496-503 as written; :505-521 are
# written [a, alpha, d, theta] and are read here the way transformation_matrix reads them: column for column)
SCRIPT_ARMS = [
    [[0., HP, 0., 0.13156], [0., 0., -0.1104, 0.], [0., 0., -0.096, 0.], [0., HP, 0., 0.06639], [0., -HP, 0., 0.07318], [0., 0., 0., 0.0436]],
    [[0., 0., 0.05, 0.], [0.05, HP, 0., 0.], [0., 0., 0.05, 0.], [0., 0., 0.05, 0.], [0., 0., 0.05, 0.], [0., 0., 0.05, 0.]],
    [[0., 0., 0.05, 0.], [0.05, HP, 0., 0.], [0., 0., 0.05, HP], [0.05, 0., 0., 0.], [0.05, 0., 0., 0.], [0.05, 0., 0., 0.]],
]
DRIVER_REF = [0.15, 0.2, 0.1, 0, 0, 0.2]
ARM_N = (1, 2, 5, 6, 7, 8)
SOLVE_ITER = 100
EPS_LM = 1e-5
KAPPA_FENCE, KAPPA_FENCE_LM, FOLD_FENCE, GIMBAL_FENCE = 1.0e3, 1.0e4, 0.05, 0.05


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def random_arm(rs, n):
    return [[0.0, float(rs.choice([0.0, HP, -HP, rs.uniform(-1.5, 1.5)])), float(rs.uniform(-0.15, 0.15)), float(rs.uniform(-0.15, 0.15))]
            for _ in range(n)]


def with_angles(arm, ang):
    return [[float(t)] + list(row[1:]) for row, t in zip(arm, ang)]


def forward_record(ref, dh):
    ll = [list(r) for r in dh]
    _, glob, J = ref.forward_kinematics(ll)
    T = glob[-1]
    try:
        quat = ref.rot2quat(T)
        with np.errstate(all="ignore"):
            rpy = ref.quat2rpy(quat)
    except (ValueError, ZeroDivisionError):
        quat, rpy = (math.nan,) * 4, (math.nan,) * 3
    return dict(dh=np.array(dh, dtype=np.float64), T=np.array(glob), Jt=np.array(J).T.copy(), pos=np.array(T[0:3, 3]),
                e2=np.array(ref.rot2euler2(T), dtype=np.float64), e=np.array(ref.rot2euler(T), dtype=np.float64),
                quat=np.array(quat, dtype=np.float64), rpy=np.array(rpy, dtype=np.float64))


def walk(ref, dh, ref_pose, iter_cnt, method, div, every):
    """inverse_kinematics :387-438 statement by statement -> (thetas, states every `every` trips, kmax, fold, gimbal)"""
    link_list = [list(r) for r in dh]
    states = []
    kmax, fold, gimbal = 0.0, math.inf, math.inf
    for cnt in range(iter_cnt):
        _, glob, J = ref.forward_kinematics(link_list)
        T = glob[-1]
        x, y, z = T[0:3, 3]
        alpha, beta, gamma = ref.rot2euler2(T)
        ee_pose = [x, y, z, alpha, beta, gamma]
        diff_pose = np.array(ref_pose) - np.array(ee_pose)
        K_zyz = np.array([
            [0, -math.sin(alpha), math.cos(alpha) * math.sin(beta)],
            [0, math.cos(alpha), math.sin(alpha) * math.sin(beta)],
            [1, 0, math.cos(beta)]])
        K_alpha = np.identity(6)
        K_alpha[3:, 3:] = K_zyz
        d_newton = np.dot(np.dot(np.linalg.pinv(J), K_alpha), np.array(diff_pose))
        weight_mat = np.diag([1., 1., 1., math.pi / 2., math.pi / 2., math.pi / 2.])
        identity_mat = np.identity(len(link_list))   # the script's 6 is its arm's N
        jv = np.dot(K_alpha, J)
        M = np.dot(np.dot(jv.T, weight_mat), jv) + EPS_LM * identity_mat
        tmp = np.linalg.pinv(M)
        d_lm = np.dot(np.dot(np.dot(tmp, jv.T), weight_mat), np.array(diff_pose))
        delta = d_lm if method == 1 else d_newton
        sv = np.linalg.svd(J, compute_uv=False)
        kept = sv[sv > 1e-15 * sv[0]]
        keff = float(sv[0] / kept[-1]) if len(kept) else 0.0
        kmax = max(kmax, keff)
        fold = min(fold, abs(abs(math.atan2(T[1][2], T[0][2])) - math.pi / 2))
        gimbal = min(gimbal, math.hypot(T[0][2], T[1][2]))
        if cnt % every == 0:
            svM = np.linalg.svd(M, compute_uv=False)
            states.append(dict(Jt=np.array(J).T.copy(), diff=np.array(diff_pose), K=K_zyz.copy(), delta=np.array(d_newton),
                               delta_lm=np.array(d_lm), sv=np.concatenate([sv, np.zeros(6 - len(sv))]), keff=keff,
                               kM=float(svM[0] / svM[-1])))
        for i in range(len(link_list)):
            link_list[i][0] += delta[i] / div
    return [r[0] for r in link_list], states, kmax, fold, gimbal


def main():
    ref = ref_loader.load("dh_01")
    orig = ref_loader.load("dh_01_orig")
    rs = np.random.RandomState(20261)
    fw, steps, solves = [], [], []

    # ---- forward records
    for n in ARM_N:
        for k in range(96 if n <= 2 else 72):
            arm = SCRIPT_ARMS[k % 3][:n] if (n <= 6 and k % 2 == 0) else random_arm(rs, n)
            scale = [1.0, 3.2, 50.0, 4.0e3, 2.0e4, 1.0e6][k % 6]
            ang = rs.uniform(-scale, scale, n)
            if k == 65:
                ang = np.zeros(n)
            fw.append(forward_record(ref, with_angles(arm, ang)))

    # ---- solves (and the steps they visit)
    def add_solve(arm, start, ref_pose, method, iters, div, tag, every, check=None):
        dh = with_angles(arm, start)
        ang, states, kmax, fold, gimbal = walk(ref, dh, ref_pose, iters, method, div, every)
        if check is not None:
            assert np.array_equal(np.array(check(dh)), np.array(ang), equal_nan=True), "the walk is not the function"
        comparable = fold >= FOLD_FENCE and gimbal >= GIMBAL_FENCE and kmax <= (KAPPA_FENCE_LM if method == 1 else KAPPA_FENCE) and bool(np.all(np.isfinite(ang)))
        steps.extend(states)
        solves.append(dict(dh=np.array(dh), ang=np.array(ang), ref=np.array(ref_pose, dtype=np.float64), method=method, iters=iters,
                           div=div, tag=TAGS.index(tag), kmax=kmax, fold=fold, gimbal=gimbal, comparable=comparable))

    def by_function(dh):
        ll = [list(r) for r in dh]
        quiet(ref.inverse_kinematics, SOLVE_ITER, ll, list(cur_ref))
        return [r[0] for r in ll]

    def by_class(dh):
        arm = orig.NLinkArm([list(r) for r in dh])
        quiet(arm.inverse_kinematics, SOLVE_ITER, list(cur_ref))
        return [lk.dh_params_[0] for lk in arm.link_list]

    def reachable(arm, start):
        """the pose of a configuration within 0.5 rad of the start"""
        near = np.array(start) + rs.uniform(-0.5, 0.5, len(start))
        T = ref.forward_kinematics(with_angles(arm, near))[1][-1]
        return [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])] + [float(v) for v in ref.rot2euler2(T)]

    for method in (0, 1):
        for k in range(24):
            n = 6 if k < 14 else (7, 8, 7, 8, 6, 6, 7, 8, 6, 6)[k - 14]
            arm = SCRIPT_ARMS[0] if (n == 6 and k % 2 == 0) else (SCRIPT_ARMS[2] if (n == 6 and k % 4 == 1) else random_arm(rs, n))
            start = rs.uniform(-1, 1, n)
            cur_ref = reachable(arm, start)
            add_solve(arm, start, cur_ref, method, SOLVE_ITER, 200.0, "random", 7,
                      check=by_function if (method == 0 and k < 6) else None)
        for n in (1, 2, 5):
            arm = random_arm(rs, n)
            start = rs.uniform(-1, 1, n)
            add_solve(arm, start, reachable(arm, start), method, SOLVE_ITER, 200.0, "short_arm", 5)
        # tagged hard cases: the exactly singular zero start, and a target out of reach
        add_solve(SCRIPT_ARMS[0], np.zeros(6), DRIVER_REF, method, SOLVE_ITER, 200.0, "hard_singular", 5)
        add_solve(SCRIPT_ARMS[1], np.zeros(6), [0.3, -0.2, 0.4, 1.0, -2.0, 3.0], method, SOLVE_ITER, 200.0, "hard_far", 5)
        # the script's own driver solve
        add_solve(SCRIPT_ARMS[0], np.zeros(6), DRIVER_REF, method, 500, 200.0, "driver", 25)
    for k in range(4):
        start = rs.uniform(-1, 1, 6)
        cur_ref = reachable(SCRIPT_ARMS[0], start)
        add_solve(SCRIPT_ARMS[0], start, cur_ref, 0, SOLVE_ITER, 100.0, "orig", 10, check=by_class)

    def csr(items, key):
        off = np.zeros(len(items) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(it[key]) for it in items])
        return off

    out = dict(
        fw_off=csr(fw, "dh"), fw_dh=np.concatenate([f["dh"] for f in fw]), fw_T=np.concatenate([f["T"] for f in fw]),
        fw_Jt=np.concatenate([f["Jt"] for f in fw]), fw_pos=np.array([f["pos"] for f in fw]), fw_e2=np.array([f["e2"] for f in fw]),
        fw_e=np.array([f["e"] for f in fw]), fw_quat=np.array([f["quat"] for f in fw]), fw_rpy=np.array([f["rpy"] for f in fw]),
        st_off=csr(steps, "Jt"), st_Jt=np.concatenate([s["Jt"] for s in steps]), st_delta=np.concatenate([s["delta"] for s in steps]),
        st_delta_lm=np.concatenate([s["delta_lm"] for s in steps]), st_diff=np.array([s["diff"] for s in steps]),
        st_K=np.array([s["K"] for s in steps]), st_sv=np.array([s["sv"] for s in steps]), st_keff=np.array([s["keff"] for s in steps]),
        st_kM=np.array([s["kM"] for s in steps]),
        so_off=csr(solves, "dh"), so_dh=np.concatenate([s["dh"] for s in solves]), so_ang=np.concatenate([s["ang"] for s in solves]),
        so_ref=np.array([s["ref"] for s in solves]), so_method=np.array([s["method"] for s in solves], dtype=np.int32),
        so_iter=np.array([s["iters"] for s in solves], dtype=np.int32), so_div=np.array([s["div"] for s in solves]),
        so_tag=np.array([s["tag"] for s in solves], dtype=np.int32), so_kmax=np.array([s["kmax"] for s in solves]),
        so_fold=np.array([s["fold"] for s in solves]), so_gimbal=np.array([s["gimbal"] for s in solves]),
        so_comparable=np.array([s["comparable"] for s in solves], dtype=np.bool_))
    path = os.path.join(GOLD, "armdh_kat.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; %d forward records, %d steps, %d solves" % (path, os.path.getsize(path), len(fw), len(steps), len(solves)))

    import armdh_util as U
    U._cache.clear()
    for m, name in ((0, "newton"), (1, "lm")):
        gap, excluded, total = U.step_gap(m)
        print("%s: step gap %.3e (%d of %d steps excluded)" % (name, gap, excluded, total))
        sel = [q for q in range(U.n_solves()) if U.solve(q)["method"] == m and U.solve(q)["tag"] != "driver"]
        comp = [q for q in sel if U.solve(q)["comparable"]]
        print("%s: solve gap %.3e over %d comparable of %d" % (name, U.solve_gap(m), len(comp), len(sel)))
        print("%s: driver gap %.3e" % (name, U.driver_gap(m)))


if __name__ == "__main__":
    main()

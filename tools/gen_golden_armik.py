"""Golden generator of BatchArmIK: runs the reference's own functions of 00_simple_2d_inverse_kinematics_01.py and
00_simple_2d_inverse_kinematics_02_straight_control.py, loaded through oracle/ref_loader.py (the file names are added to
ref_loader.FILES at run time; the module globals N_LINKS and N_ITERATIONS are set per call, Kp = 2 and dt = 0.1 as the scripts
set them; plt is replaced by a do-nothing stub), and writes tests/golden/armik_kat.npz.  Build host only (needs the reference
checkout).

    python tools/gen_golden_armik.py

The scripts' driver cells are module-level code and cannot be called; their loops (:189-200 of script 01, :186-213 of script
02) are walked here statement by statement with the reference's own NLinkArm, ang_diff and distance_to_goal.  The trip of
inverse_kinematics (:75-84) is walked the same way to record what it visits, and the walk is held against the function itself
(same angles, same flag, the iteration count it prints).

Arrays only.  CSR offsets are in links.
Steps (n_st states (L, angles, goal) along the reference's trajectories, and the all-zero starts): st_off (n_st + 1,) into
st_L, st_ang, st_J0, st_J1 (the rows of J handed to pinv), st_P0, st_P1 (the columns of pinv(J)) and st_delta
(matmul(pinv, errors)); st_goal, st_pos (current_pos), st_err (n_st, 2), st_dist, st_sv (n_st, 2) numpy's singular values of J
(the second 0 for N = 1), st_kind (0 on a trajectory, 1 an all-zero start).
Solves (n_so, N_ITERATIONS = 200): so_off into so_L, so_ang0 (start) and so_ang (returned); so_goal, so_found, so_iter (the
value of `iteration` at the return, 200 when not found), so_tag (TAGS), so_comparable (finished in at most 16 iterations and no
visited distance within 1e-9 of 0.1).
Moves (n_mv): mv_off into mv_L, mv_ang0 and mv_gang (joint_goal_angles: the reference's own solution); mv_goal, mv_tag
(MOVE_TAGS), mv_step_off (n_mv + 1,) into mv_tdist (distance after every step), mv_tang_off (n_mv + 1,) into mv_tang (the angles
after every step).
Script 02 (3 goals x 5 rounds on the driver arm): fl_goal (3, 2), fl_solve (3, 5) and fl_move (3, 5) the numbers of the rounds
among the solves and the moves (-1: the round has no move), fl_end (3, 5) the joint angles after each round.
The gaps of the two tolerances (tests/armik_util.py) are printed at the end.
"""
import contextlib
import io
import os
import random
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_loader  # noqa: E402

ref_loader.FILES["ik_01"] = "00_simple_2d_inverse_kinematics_01.py"
ref_loader.FILES["ik_02"] = "00_simple_2d_inverse_kinematics_02_straight_control.py"
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ("random", "start_within", "beyond_reach", "driver_area", "one_link", "follow_round")
MOVE_TAGS = ("found_query", "no_step", "wraps", "follow_round")
DRIVER_LINKS = [0.5, 1.5, 1.8, 1.2, 0.5]
DRIVER_ANGLES = [1.6, -1.6, 0.8, -0.5, 0.6]
ARM_N = (1, 2, 3, 5, 7, 8, 9, 15, 16)
N_ITERATIONS = 200
GOAL_DIST = 0.1   # the literal of :78 and :189


class Nothing:
    """plt: every attribute and every call gives it back"""
    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


def load(short):
    ref = ref_loader.load(short)
    ref.plt = Nothing()
    ref.Kp, ref.dt, ref.N_ITERATIONS = 2, 0.1, N_ITERATIONS
    return ref


def walk_solve(ref, L, ang0, goal):
    """inverse_kinematics :75-84 statement by statement -> (angles, found, iterations, states, distances)"""
    ref.N_LINKS = len(L)
    seen = []
    pinv = np.linalg.pinv

    def keeping(J, *a, **k):
        seen.append(np.array(J))
        return pinv(J, *a, **k)
    ang = np.array(ang0, dtype=np.float64)
    goal = np.array(goal, dtype=np.float64)
    states, dists = [], []
    found, iters = False, N_ITERATIONS
    np.linalg.pinv = keeping
    try:
        for it in range(N_ITERATIONS):
            pos = ref.forward_kinematics(L, ang)
            err, dist = ref.distance_to_goal(pos, goal)
            dists.append(float(dist))
            if dist < GOAL_DIST:
                found, iters = True, it
                break
            del seen[:]
            P = ref.jacobian_inverse(L, ang)
            J = seen[0]
            delta = np.matmul(P, err)
            sv = np.linalg.svd(J, compute_uv=False)
            states.append(dict(L=list(L), ang=ang.copy(), goal=goal.copy(), pos=np.array(pos, dtype=np.float64), err=np.array(err),
                               dist=float(dist), J=J, P=np.array(P), delta=np.array(delta), sv=sv, kind=0))
            ang = ang + delta
    finally:
        np.linalg.pinv = pinv
    # the function itself
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        r_ang, r_found = ref.inverse_kinematics(L, np.array(ang0, dtype=np.float64), goal)
    assert bool(r_found) == found and np.array_equal(np.asarray(r_ang), ang, equal_nan=True), "the walk is not the function"
    m = re.search(r"Solution found in (\d+) iterations", out.getvalue())
    assert (int(m.group(1)) == iters) if found else (m is None)
    return ang, found, iters, states, dists


def walk_move(ref, L, ang0, gang, goal):
    """The driver's loop :174-200 -> (angles after every step, distance after every step)"""
    ref.N_LINKS = len(L)
    arm = ref.NLinkArm(L, np.array(ang0, dtype=np.float64), goal)
    goal_pos = np.array(arm.goal)
    joint_angles = np.array(ang0, dtype=np.float64)
    errors, distance = ref.distance_to_goal(arm.end_effector, goal_pos)
    ta, td = [], []
    if distance > GOAL_DIST:
        while distance > GOAL_DIST:
            joint_angles = joint_angles + ref.Kp * ref.ang_diff(gang, joint_angles) * ref.dt
            arm.update_joints(joint_angles)
            errors, distance = ref.distance_to_goal(arm.end_effector, goal_pos)
            ta.append(np.array(joint_angles))
            td.append(float(distance))
            assert len(td) < 100000
    return ta, td


def main():
    import armik_oracle as O
    import armik_util as U
    os.makedirs(GOLD, exist_ok=True)
    ref = load("ik_01")
    ref2 = load("ik_02")
    rs = np.random.RandomState(7001)
    solves, steps, moves = [], [], []
    n_big = [0]

    def add_solve(L, ang0, goal, tag, keep_steps=0):
        ang, found, iters, states, dists = walk_solve(ref, L, ang0, goal)
        comparable = found and iters <= 16 and not any(abs(d - GOAL_DIST) <= 1e-9 for d in dists)
        solves.append(dict(L=list(L), ang0=np.array(ang0, dtype=np.float64), goal=np.array(goal, dtype=np.float64), ang=ang,
                           found=found, iters=iters, tag=tag, comparable=comparable))
        steps.extend(states[:keep_steps])
        big = [i for i, st in enumerate(states) if float(np.max(np.abs(st["ang"]))) > 1.0e3]
        if big and n_big[0] < 6:   # angles beyond 1e3 rad: the steps round the first of them
            n_big[0] += 1
            steps.extend(states[max(keep_steps, big[0] - 2):big[0] + 4])
        return solves[-1], states

    def rand_arm(n):
        return [float(v) for v in rs.uniform(0.3, 2.0, n)]

    def goal_within(L, frac):
        r, t = frac * sum(L) * np.sqrt(rs.uniform(0.0, 1.0)), rs.uniform(-np.pi, np.pi)
        return [float(r * np.cos(t)), float(r * np.sin(t))]

    found_queries = []
    for n in ARM_N:
        L = rand_arm(n)
        for k in range(22):
            ang0 = rs.uniform(-np.pi, np.pi, n)
            if n == 1:   # a 1-link arm reaches a circle: goals near it, some close enough to be found
                t = ang0[0] + rs.uniform(-0.6, 0.6)
                r = L[0] + rs.uniform(-0.08, 0.08)
                goal = [float(r * np.cos(t)), float(r * np.sin(t))]
            else:
                goal = goal_within(L, 0.95)
            q, states = add_solve(L, ang0, goal, "one_link" if n == 1 else "random", keep_steps=8 if k < 8 else 0)
            if k in (8, 9):   # two whole trajectories per arm, long and chaotic ones as they come
                steps.extend(states[:40])
            if q["found"]:
                found_queries.append(q)
    # the driver arm and the area of get_random_goal, by the reference's own function
    random.seed(7002)
    for k in range(70):
        q, states = add_solve(DRIVER_LINKS, DRIVER_ANGLES, ref.get_random_goal(), "driver_area", keep_steps=6 if k < 10 else 0)
        if q["found"]:
            found_queries.append(q)
    # starts already within 0.1: the goal a little off the start's own end effector
    for n in (1, 2, 5, 16):
        L = rand_arm(n)
        ang0 = rs.uniform(-np.pi, np.pi, n)
        ref.N_LINKS = n
        pos = ref.forward_kinematics(L, ang0)
        q, _ = add_solve(L, ang0, [float(pos[0] + 0.03), float(pos[1] - 0.05)], "start_within")
        assert q["found"] and q["iters"] == 0
    # goals beyond the reach: never found
    for n in (1, 2, 3, 5, 8, 16):
        L = rand_arm(n)
        t = rs.uniform(-np.pi, np.pi)
        q, states = add_solve(L, rs.uniform(-np.pi, np.pi, n), [float(1.6 * sum(L) * np.cos(t)), float(1.6 * sum(L) * np.sin(t))],
                              "beyond_reach")
        assert not q["found"] and q["iters"] == N_ITERATIONS
        steps.extend(states[:30])
    # the all-zero start: row 0 of J is exactly zero
    for n in (2, 5):
        L = rand_arm(n) if n == 2 else DRIVER_LINKS
        _, _, _, states, _ = walk_solve(ref, L, np.zeros(n), goal_within(L, 0.8))
        assert np.all(states[0]["J"][0] == 0.0)
        states[0]["kind"] = 1
        steps.append(states[0])

    # moves: the driver's loop on found queries with the reference's own joint_goal_angles
    def add_move(L, ang0, gang, goal, tag):
        ta, td = walk_move(ref, L, ang0, gang, goal)
        moves.append(dict(L=list(L), ang0=np.array(ang0, dtype=np.float64), gang=np.array(gang, dtype=np.float64),
                          goal=np.array(goal, dtype=np.float64), ta=ta, td=td, tag=tag))
        return moves[-1]
    short = [q for q in found_queries if 0 < q["iters"]]
    order = sorted(range(len(short)), key=lambda i: (len(short[i]["L"]), i))
    picked = [short[i] for i in order[::max(1, len(order) // 36)]][:36]
    for q in picked:
        turns = float(np.max(np.abs(q["ang"] - q["ang0"]))) > 4 * np.pi
        add_move(q["L"], q["ang0"], q["ang"], q["goal"], "wraps" if turns else "found_query")
    if not any(m["tag"] == "wraps" for m in moves):
        far = [q for q in found_queries if float(np.max(np.abs(q["ang"] - q["ang0"]))) > 4 * np.pi]
        add_move(far[0]["L"], far[0]["ang0"], far[0]["ang"], far[0]["goal"], "wraps")
    q0 = [q for q in solves if q["tag"] == "start_within"][1]
    assert add_move(q0["L"], q0["ang0"], q0["ang"], q0["goal"], "no_step")["td"] == []

    # script 02: five rounds for three goals
    fl_goal, fl_solve, fl_move, fl_end = [], [], [], []
    random.seed(7003)
    n_step = 5
    for g in range(3):
        goal_pos_orig = np.array(ref2.get_random_goal()).T
        joint_angles = np.array(DRIVER_ANGLES)
        ref2.N_LINKS = 5
        arm = ref2.NLinkArm(DRIVER_LINKS, joint_angles, goal_pos_orig)
        end_effector_orig = arm.end_effector
        vec_to_follow = goal_pos_orig - end_effector_orig
        row_s, row_m, row_e = [], [], []
        for i in range(n_step):
            goal_current = end_effector_orig + 1 / n_step * i * vec_to_follow
            q, _ = add_solve(DRIVER_LINKS, joint_angles, goal_current, "follow_round")
            with contextlib.redirect_stdout(io.StringIO()):
                a2, f2 = ref2.inverse_kinematics(DRIVER_LINKS, joint_angles, goal_current)   # script 02's copy is the same function
            assert bool(f2) == q["found"] and np.array_equal(a2, q["ang"])
            row_s.append(len(solves) - 1)
            if q["found"]:
                m = add_move(DRIVER_LINKS, joint_angles, q["ang"], goal_current, "follow_round")
                if m["ta"]:
                    joint_angles = m["ta"][-1]
                row_m.append(len(moves) - 1)
            else:
                row_m.append(-1)
            row_e.append(np.array(joint_angles))
        fl_goal.append(goal_pos_orig)
        fl_solve.append(row_s)
        fl_move.append(row_m)
        fl_end.append(row_e)

    n_cmp = sum(q["comparable"] for q in solves)
    print("%d solves (%d found, %d comparable), %d steps (largest |angle| %.3g), %d moves (%d steps in all)" % (
        len(solves), sum(q["found"] for q in solves), n_cmp, len(steps), max(float(np.max(np.abs(s["ang"]))) for s in steps),
        len(moves), sum(len(m["td"]) for m in moves)))
    assert 3 * n_cmp >= len(solves), "fewer than a third of the solves are comparable"
    assert max(float(np.max(np.abs(s["ang"]))) for s in steps) > 1.0e3

    def csr(rows):
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        return off, (np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1) for r in rows]) if rows else np.zeros(0))
    st_off, st_L = csr([s["L"] for s in steps])
    so_off, so_L = csr([q["L"] for q in solves])
    mv_off, mv_L = csr([m["L"] for m in moves])
    mv_step_off, mv_tdist = csr([m["td"] for m in moves])
    mv_tang_off, mv_tang = csr([np.array(m["ta"]).reshape(-1) for m in moves])
    dst = os.path.join(GOLD, "armik_kat.npz")
    np.savez_compressed(
        dst, st_off=st_off, st_L=st_L, st_ang=csr([s["ang"] for s in steps])[1], st_J0=csr([s["J"][0] for s in steps])[1],
        st_J1=csr([s["J"][1] for s in steps])[1], st_P0=csr([s["P"][:, 0] for s in steps])[1],
        st_P1=csr([s["P"][:, 1] for s in steps])[1], st_delta=csr([s["delta"] for s in steps])[1],
        st_goal=np.array([s["goal"] for s in steps]), st_pos=np.array([s["pos"] for s in steps]),
        st_err=np.array([s["err"] for s in steps]), st_dist=np.array([s["dist"] for s in steps]),
        st_sv=np.array([[s["sv"][0], s["sv"][1] if len(s["sv"]) > 1 else 0.0] for s in steps]),
        st_kind=np.array([s["kind"] for s in steps], dtype=np.int32),
        so_off=so_off, so_L=so_L, so_ang0=csr([q["ang0"] for q in solves])[1], so_ang=csr([q["ang"] for q in solves])[1],
        so_goal=np.array([q["goal"] for q in solves]), so_found=np.array([q["found"] for q in solves], dtype=np.bool_),
        so_iter=np.array([q["iters"] for q in solves], dtype=np.int32),
        so_tag=np.array([TAGS.index(q["tag"]) for q in solves], dtype=np.int32),
        so_comparable=np.array([q["comparable"] for q in solves], dtype=np.bool_),
        mv_off=mv_off, mv_L=mv_L, mv_ang0=csr([m["ang0"] for m in moves])[1], mv_gang=csr([m["gang"] for m in moves])[1],
        mv_goal=np.array([m["goal"] for m in moves]), mv_tag=np.array([MOVE_TAGS.index(m["tag"]) for m in moves], dtype=np.int32),
        mv_step_off=mv_step_off, mv_tdist=mv_tdist, mv_tang_off=mv_tang_off, mv_tang=mv_tang,
        fl_goal=np.array(fl_goal), fl_solve=np.array(fl_solve, dtype=np.int32), fl_move=np.array(fl_move, dtype=np.int32),
        fl_end=np.array(fl_end))
    print("%d bytes" % os.path.getsize(dst))
    U._cache.clear()
    gap, excluded, n_steps = U.step_gap()
    print("TOL_STEP gap %.3e (%d of %d steps excluded)" % (gap, excluded, n_steps))
    assert 20 * excluded <= n_steps, "more than 5 % of the golden steps are outside the step comparison"
    print("TOL_SOLVE gap %.3e" % U.solve_gap())
    assert O.FOUND == 0


if __name__ == "__main__":
    main()

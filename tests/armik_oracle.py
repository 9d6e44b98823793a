"""TEST ORACLE of BatchArmIK: a plain-Python restatement of inverse_kinematics, forward_kinematics, the matrix J of
jacobian_inverse, distance_to_goal and the driver's loop of 00_simple_2d_inverse_kinematics_01.py (:71-118, :189-200), with the
arithmetic forms numpy takes written out on Python floats -- np.sum of a slice as numpy's pairwise sum, np.cos / np.sin as
math.cos / math.sin, the floored `%` -- and np.hypot taken from numpy itself (it is libm's hypot, not math.hypot's algorithm).

The step pinv(J) @ errors is NOT restated: step_w is this package's own closed form with its rank rule, operation for operation
what the top of csrc/rpp_armik.h states (tests/test_armik_host.py holds the two bit-identical, and measures the step against the
reference's recorded one)."""
import math
import struct

import numpy as np

FOUND, NOT_FOUND, NONFINITE, STEP_CAP = 0, 1, 2, 3
RANK_EPS = 2.0 ** -40
PI = math.pi
TRIG_MAX = struct.unpack("<d", struct.pack("<Q", 0x419921FB << 32))[0]   # 105 414 357.85...: where the device's libm replicas end


def hypot(x, y):
    return float(np.hypot(x, y))


def np_sum(a, n):
    """np.sum(a[:n]) for a list of floats, 0 <= n <= 16"""
    if n < 8:
        r = 0.0
        for k in range(n):
            r = r + a[k]
        return r
    r = [a[k] for k in range(8)]
    i = 8
    while i + 8 <= n:
        for k in range(8):
            r[k] = r[k] + a[i + k]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + a[i]
        i += 1
    return 0.0 + res


def forward(L, ang, goal, terms):
    """-> (x, y, ex, ey, dist, t0, t1): current_pos, errors, distance, and with `terms` the terms L[j] * sin(S_j), L[j] * cos(S_j);
    None when a prefix sum is not finite or lies at or beyond TRIG_MAX"""
    n = len(L)
    x = y = 0.0
    t0, t1 = [0.0] * n, [0.0] * n
    for i in range(0 if terms else 1, n + 1):
        S = np_sum(ang, i)
        if not abs(S) < TRIG_MAX:
            return None
        sn, cs = math.sin(S), math.cos(S)
        if i > 0:
            x = x + L[i - 1] * cs
            y = y + L[i - 1] * sn
        if terms and i < n:
            t0[i] = L[i] * sn
            t1[i] = L[i] * cs
    ex, ey = goal[0] - x, goal[1] - y
    return x, y, ex, ey, hypot(ex, ey), t0, t1


def jacobian(t0, t1):
    """J (two rows) from its terms: every column its own left-to-right chain"""
    n = len(t0)
    j0, j1 = [0.0] * n, [0.0] * n
    for i in range(n):
        a0 = a1 = 0.0
        for j in range(i, n):
            a0 = a0 - t0[j]
            a1 = a1 + t1[j]
        j0[i], j1[i] = a0, a1
    return j0, j1


def step_w(j0, j1, e0, e1):
    """-> (w0, w1, rank): this package's definition of pinv(J) @ e as J^T w"""
    n = len(j0)
    a = b = c = 0.0
    for i in range(n):
        u, v = j0[i], j1[i]
        a = a + u * u
        b = b + u * v
        c = c + v * v
    tr = a + c
    det = a * c - b * b
    if tr == 0.0:
        return 0.0, 0.0, 0
    if n == 1 or not det > RANK_EPS * (tr * tr):
        q = tr * tr
        return (a * e0 + b * e1) / q, (b * e0 + c * e1) / q, 1
    return (c * e0 - b * e1) / det, (a * e1 - b * e0) / det, 2


def step_delta(j0, j1, e0, e1):
    w0, w1, rank = step_w(j0, j1, e0, e1)
    return [j0[i] * w0 + j1[i] * w1 for i in range(len(j0))], rank


def solve(L, ang, goal, goal_dist=0.1, max_iterations=10000):
    """-> dict(status, iterations, angles, end, distance): inverse_kinematics :71-85"""
    L = [float(v) for v in L]
    ang = [float(v) for v in ang]
    goal = (float(goal[0]), float(goal[1]))
    x = y = dist = 0.0
    for it in range(max_iterations):
        f = forward(L, ang, goal, True)
        if f is None:   # the angles have left the domain: the last pose computed is reported
            return dict(status=NONFINITE, iterations=max_iterations, angles=ang, end=(x, y), distance=dist)
        x, y, ex, ey, dist, t0, t1 = f
        if dist < goal_dist:
            return dict(status=FOUND, iterations=it, angles=ang, end=(x, y), distance=dist)
        j0, j1 = jacobian(t0, t1)
        delta, _ = step_delta(j0, j1, ex, ey)
        ang = [ang[i] + delta[i] for i in range(len(L))]
        if not all(math.isfinite(v) for v in ang):
            return dict(status=NONFINITE, iterations=max_iterations, angles=ang, end=(x, y), distance=dist)
    return dict(status=NOT_FOUND, iterations=max_iterations, angles=ang, end=(x, y), distance=dist)


def angle_mod(x):
    return (x + PI) % (2 * PI) - PI


def move(L, ang, goal_ang, goal, Kp=2.0, dt=0.1, goal_dist=0.1, max_steps=100000):
    """-> dict(status, n_steps, angles, end, distance, traj_angles [n_steps][N], traj_distance [n_steps]): the loop :189-200"""
    L = [float(v) for v in L]
    ang = [float(v) for v in ang]
    goal_ang = [float(v) for v in goal_ang]
    goal = (float(goal[0]), float(goal[1]))
    Kp, dt = float(Kp), float(dt)
    x, y, _, _, dist, _, _ = forward(L, ang, goal, False)
    ta, td = [], []
    steps = 0
    while dist > goal_dist and steps < max_steps:
        ang = [a + (Kp * angle_mod(g - a)) * dt for a, g in zip(ang, goal_ang)]
        f = forward(L, ang, goal, False)
        if f is not None:
            x, y, _, _, dist, _, _ = f
        ta.append(ang)
        td.append(dist)
        steps += 1
        if f is None:   # a huge Kp * dt took the angles out of the domain: the step is counted, the last pose is kept
            return dict(status=NONFINITE, n_steps=steps, angles=ang, end=(x, y), distance=dist, traj_angles=ta, traj_distance=td)
    return dict(status=STEP_CAP if dist > goal_dist else FOUND, n_steps=steps, angles=ang, end=(x, y), distance=dist,
                traj_angles=ta, traj_distance=td)


def follow_line(L, ang, goal, n_step=5, goal_dist=0.1, max_iterations=10000, Kp=2.0, dt=0.1, max_steps=100000):
    """Script 02's loop :186-213 -> list of dict(goal, solve, move or None) per round, and the angles reached"""
    L = [float(v) for v in L]
    ang = [float(v) for v in ang]
    x0, y0, _, _, _, _, _ = forward(L, ang, (0.0, 0.0), False)
    vx, vy = float(goal[0]) - x0, float(goal[1]) - y0
    rounds = []
    for i in range(n_step):
        sub = (x0 + 1 / n_step * i * vx, y0 + 1 / n_step * i * vy)
        s = solve(L, ang, sub, goal_dist, max_iterations)
        m = None
        if s["status"] == FOUND:
            m = move(L, ang, s["angles"], sub, Kp, dt, goal_dist, max_steps)
            ang = m["angles"]
        rounds.append(dict(goal=sub, solve=s, move=m))
    return rounds, ang

"""Batched inverse kinematics of planar N-link arms on the GPU: the Jacobian inverse method for many (arm, start angles, goal)
queries in one call, the driver's P-control loop that moves the arm to the angles found, and script 02's straight-line
following built from the two.

    ik = BatchArmIK()
    res = ik.solve([0.5, 1.5, 1.8, 1.2, 0.5], [1.6, -1.6, 0.8, -0.5, 0.6], goals)      # one arm, one start, (Q, 2) goals
    res.result(3)                                                                      # the script's (joint_angles, True / False)
    mv = ik.move(links, starts, res.angles, goals)                                     # P control towards the angles found

For every query solve() does what inverse_kinematics(link_lengths, joint_angles, goal_pos) of
00_simple_2d_inverse_kinematics_01.py (:71-85) does, and move() what the loop of its driver cell (:189-200) does.  Forward
kinematics, the Jacobian, the distance test and all of move() are the reference's doubles (on the golden host, README).  The step
pinv(J) @ errors is this package's own closed form with a stated rank rule (csrc/rpp_armik.h): the reference takes
full Newton steps through LAPACK's SVD and the iteration is chaotic, so short solves agree with it to a measured tolerance and
long ones need not agree at all.

There is no CPU fallback: without a device BatchArmIK raises RrtxError.
"""
import numpy as np

from . import _abi


def pack_arms(link_lengths):
    """(link_off int64 (n_arms + 1,), link_len float64): one arm (a flat sequence of numbers) or a list of arms"""
    one = len(link_lengths) > 0 and np.ndim(link_lengths[0]) == 0
    arms = [np.asarray(a, dtype=np.float64).reshape(-1) for a in ([link_lengths] if one else list(link_lengths))]
    link_off = np.zeros(len(arms) + 1, dtype=np.int64)
    if arms:
        link_off[1:] = np.cumsum([len(a) for a in arms])
    return link_off, np.ascontiguousarray(np.concatenate(arms) if arms else np.zeros(0), dtype=np.float64)


class _Rows:
    """What the results share: CSR angles, or (Q, N) when every query's arm has the same N"""

    def __len__(self):
        return len(self.status)

    def angles_of(self, i):
        return self._flat[int(self.offsets[i]):int(self.offsets[i + 1])]

    def _shape(self, offsets, flat):
        self.offsets, self._flat = offsets, flat
        n = np.diff(offsets)
        self.angles = flat.reshape(len(n), int(n[0])) if len(n) and np.all(n == n[0]) else flat


class ArmIKResult(_Rows):
    """One batch of solves.  Per query: status (ARMIK_FOUND, ARMIK_NOT_FOUND, ARMIK_NONFINITE: an angle is not finite, or a sum
    of angles reached 105 414 357 rad, where the device's sin / cos end), found, iterations (the value of
    `iteration` at the return; max_iterations when not found), end (Q, 2) the last current_pos computed, distance; angles: the
    joint angles returned -- (Q, N) when all arms have one N, else flat with offsets (Q + 1,); partial: some query was not
    found; kernel_ms, waves."""

    def __init__(self, status, iterations, end, distance, offsets, flat, partial=False, kernel_ms=0.0, waves=0):
        self.status, self.iterations, self.end, self.distance = status, iterations, end, distance
        self._shape(offsets, flat)
        self.partial, self.kernel_ms, self.waves = partial, kernel_ms, waves

    @property
    def found(self):
        return self.status == _abi.ARMIK_FOUND

    def result(self, i):
        """What inverse_kinematics returns for query i: (joint_angles, solution_found)"""
        return self.angles_of(i).copy(), bool(self.status[i] == _abi.ARMIK_FOUND)


class ArmMoveResult(_Rows):
    """One batch of moves.  Per query: status (ARMIK_FOUND: the loop ended; ARMIK_STEP_CAP: max_steps reached; ARMIK_NONFINITE:
    a step -- only a huge Kp * dt can -- took a sum of angles past 105 414 357 rad, where the device's sin / cos end), n_steps, end
    (Q, 2) the end effector, distance, angles (as ArmIKResult); with arrays the trajectory: traj_offsets (Q + 1,) into
    traj_distance (the distance after every step) and traj_angle_offsets (Q + 1,) into traj_angles (the angles after every step),
    else None; partial; kernel_ms."""

    def __init__(self, status, n_steps, end, distance, offsets, flat, traj=None, partial=False, kernel_ms=0.0):
        self.status, self.n_steps, self.end, self.distance = status, n_steps, end, distance
        self._shape(offsets, flat)
        self.traj_offsets, self.traj_angle_offsets, self.traj_angles, self.traj_distance = traj if traj else (None,) * 4
        self.partial, self.kernel_ms = partial, kernel_ms

    @property
    def reached(self):
        return self.status == _abi.ARMIK_FOUND

    def trajectory(self, i):
        """(angles (n_steps, N), distance (n_steps,)) of query i after every step"""
        if self.traj_offsets is None:
            raise ValueError("ArmMoveResult: the batch was run with arrays=False")
        d = self.traj_distance[int(self.traj_offsets[i]):int(self.traj_offsets[i + 1])]
        a = self.traj_angles[int(self.traj_angle_offsets[i]):int(self.traj_angle_offsets[i + 1])]
        return a.reshape(len(d), int(self.offsets[i + 1] - self.offsets[i])), d


class BatchArmIK:
    """Inverse kinematics and P-control moves for batches of planar arms of 1 .. 16 links; device buffers are kept between
    calls.  goal_dist: the script's 0.1; max_iterations: its N_ITERATIONS; waves: the number of persistent waves solve()
    launches, exactly (default: as many as the device holds, at most one lane per query) -- results do not depend on it."""

    def __init__(self, goal_dist=0.1, max_iterations=10000, waves=None, device=0):
        self.goal_dist, self.max_iterations, self.waves = float(goal_dist), int(max_iterations), waves
        self._ik = _abi.ArmIK(device)

    def close(self):
        self._ik.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _pack(self, link_lengths, joint_angles, goals, arm, *more):
        link_off, link_len = pack_arms(link_lengths)
        n_arms = len(link_off) - 1
        go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        Q = len(go)
        if arm is None:
            if n_arms > 1 and n_arms != Q:
                raise ValueError("BatchArmIK: %d arms and %d queries: say which arm each query moves" % (n_arms, Q))
            ar = np.arange(Q, dtype=np.int32) if n_arms > 1 else None
        else:
            ar = np.ascontiguousarray(arm, dtype=np.int32).reshape(-1)
            if len(ar) != Q:
                raise ValueError("BatchArmIK: %d arm indices for %d queries" % (len(ar), Q))
        inside = ar is None or not len(ar) or (ar.min() >= 0 and ar.max() < n_arms)
        n_of = np.diff(link_off)[ar if ar is not None else np.zeros(Q, dtype=np.int64)] if (inside and n_arms) else None
        flats = []
        for a in (joint_angles,) + more:
            flats.append(self._angles(a, n_of, ar, n_arms, Q) if n_of is not None else np.zeros(0))
        return (link_off, link_len, ar, go) + tuple(flats)

    @staticmethod
    def _angles(a, n_of, ar, n_arms, Q):
        """Flat angles, query after query.  a: (Q, N), a flat array of sum N values, a list of Q rows, or one row per arm (or
        one row) that is broadcast"""
        total = int(n_of.sum())
        if isinstance(a, np.ndarray) and a.size == total and total and (a.ndim == 1 or a.shape[0] == Q):
            return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        rows = [np.asarray(r, dtype=np.float64).reshape(-1) for r in (a if np.ndim(a[0]) else [a])] if len(a) else []
        if len(rows) == Q and all(len(r) == n for r, n in zip(rows, n_of)):
            pass
        elif len(rows) == n_arms:   # one row per arm
            rows = [rows[0 if ar is None else int(s)] for s in (range(Q) if ar is None else ar)]
        else:
            raise ValueError("BatchArmIK: %d rows of angles for %d queries and %d arms" % (len(rows), Q, n_arms))
        if any(len(r) != n for r, n in zip(rows, n_of)):
            raise ValueError("BatchArmIK: a row of angles is not as long as its arm")
        return np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0), dtype=np.float64)

    def solve(self, link_lengths, joint_angles, goals, arm=None):
        """link_lengths: one arm (1 .. 16 lengths) or a list of arms; joint_angles: (Q, N), or one row per arm that is
        broadcast; goals: (Q, 2); arm[q]: the arm of query q when there are several (default: query q moves arm q when there
        are as many arms as queries)."""
        link_off, link_len, ar, go, ang = self._pack(link_lengths, joint_angles, goals, arm)
        waves = 0 if self.waves is None else (int(self.waves) if int(self.waves) >= 1 else -1)
        rc = self._ik.solve(link_off, link_len, ar, ang, go, self.goal_dist, self.max_iterations, waves)
        status, count, end, dist, n_angles = self._ik.records()
        off, flat = self._ik.angles(len(go), n_angles)
        ms, w = self._ik.kernel_ms()
        return ArmIKResult(status, count, end, dist, off, flat, rc == _abi.RRTX_PARTIAL, ms, w)

    def move(self, link_lengths, joint_angles, joint_goal_angles, goals, Kp=2, dt=0.1, max_steps=100000, arrays=True, arm=None):
        """The driver's loop for every query: while distance > goal_dist: joint_angles += Kp * ang_diff(joint_goal_angles,
        joint_angles) * dt.  arrays=False: no trajectory is produced."""
        link_off, link_len, ar, go, ang, gang = self._pack(link_lengths, joint_angles, goals, arm, joint_goal_angles)
        return self._move(link_off, link_len, ar, go, ang, gang, self.goal_dist, Kp, dt, max_steps, arrays)

    def _move(self, link_off, link_len, ar, go, ang, gang, goal_dist, Kp, dt, max_steps, arrays):
        rc = self._ik.move(link_off, link_len, ar, ang, gang, go, goal_dist, Kp, dt, max_steps, arrays)
        status, count, end, dist, n_angles = self._ik.records()
        off, flat = self._ik.angles(len(go), n_angles)
        traj = self._ik.trajectory(len(go)) if arrays else None
        return ArmMoveResult(status, count, end, dist, off, flat, traj, rc == _abi.RRTX_PARTIAL, self._ik.kernel_ms()[0])

    def _end_effectors(self, link_off, link_len, ar, go, ang):
        """NLinkArm.update_points for every query, in the device's doubles: the library has no entry point for forward
        kinematics alone, and a move reports the pose it starts from when it takes no step -- under a goal_dist above every
        distance none does.  Returns the ArmMoveResult (.end the end effectors, .offsets the CSR offsets of the angles)."""
        return self._move(link_off, link_len, ar, go, ang, ang, 1.0e300, 0.0, 0.0, 1, False)

    def follow_line(self, link_lengths, joint_angles, goals, n_step=5, arm=None, Kp=2, dt=0.1, max_steps=100000):
        """Script 02's loop (:186-213) for every query: n_step rounds of solve() then move() over the whole batch, each round
        warm-started from the angles the last one reached.  Round i aims at end_effector_orig + 1 / n_step * i * vec_to_follow,
        so round 0 finds at once and the final goal itself is never a sub-goal; a query whose solve fails in a round skips
        that round's move.  Returns (angles reached -- CSR flat, or (Q, N) --, rounds: a list of (sub-goals (Q, 2),
        ArmIKResult, ArmMoveResult of the queries that moved or None, their numbers))."""
        link_off, link_len, ar, go, ang = self._pack(link_lengths, joint_angles, goals, arm)
        Q = len(go)
        first = self._end_effectors(link_off, link_len, ar, go, ang)
        first_end = first.end   # end_effector_orig
        vec = go - first_end
        rounds = []
        off = first.offsets
        for i in range(int(n_step)):
            sub = np.ascontiguousarray(first_end + 1 / n_step * i * vec)
            s = self.solve(link_lengths, ang, sub, arm=ar)
            idx = np.nonzero(s.found)[0]   # a query whose solve failed skips the round's move
            m = None
            if len(idx):
                sel = np.concatenate([np.arange(off[q], off[q + 1]) for q in idx])
                m = self._move(link_off, link_len, None if ar is None else np.ascontiguousarray(ar[idx]), np.ascontiguousarray(sub[idx]),
                               np.ascontiguousarray(ang[sel]), np.ascontiguousarray(s._flat[sel]), self.goal_dist, Kp, dt, max_steps, False)
                ang = ang.copy()
                ang[sel] = m._flat
            rounds.append((sub, s, m, idx))
        n = np.diff(off)
        return (ang.reshape(Q, int(n[0])) if Q and np.all(n == n[0]) else ang), rounds

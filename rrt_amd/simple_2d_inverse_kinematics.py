"""Names of 00_simple_2d_inverse_kinematics_01.py and 00_simple_2d_inverse_kinematics_02_straight_control.py as their driver
cells use them.  The MI355X mirror: inverse_kinematics is a batch of one on robotics-path-planning_amd/armik.py (same arguments,
same return types; its step is the package's closed form of pinv(J) @ errors); no CPU fallback.  NLinkArm,
forward_kinematics, jacobian_inverse, distance_to_goal, ang_diff, angle_mod and get_random_goal are a few lines of host
arithmetic: one pose needs no device.  As in the scripts the functions read N_LINKS and N_ITERATIONS from this module -- set
N_LINKS to the arm's link count before calling them.  No matplotlib: nothing is drawn."""
import numpy as np

from . import armik as _a

Kp = 2
dt = 0.1
N_ITERATIONS = 10000
N_LINKS = 5
_solver = None


def angle_mod(x, zero_2_2pi=False, degree=False):
    """x wrapped into [-pi, pi), or into [0, 2 pi) with zero_2_2pi; a float for a float, else a flat array"""
    is_float = isinstance(x, float)
    x = np.asarray(x).flatten()
    if degree:
        x = np.deg2rad(x)
    mod_angle = x % (2 * np.pi) if zero_2_2pi else (x + np.pi) % (2 * np.pi) - np.pi
    if degree:
        mod_angle = np.rad2deg(mod_angle)
    return mod_angle.item() if is_float else mod_angle


class NLinkArm(object):
    """A planar arm of len(link_lengths) links with a goal: points[k] is the end of link k (points[0] the base at the origin)."""

    def __init__(self, link_lengths, joint_angles, goal):
        self.n_links = len(link_lengths)
        if self.n_links != len(joint_angles):
            raise ValueError()
        self.link_lengths = np.array(link_lengths)
        self.joint_angles = np.array(joint_angles)
        self.points = [[0, 0] for _ in range(self.n_links + 1)]
        self.lim = sum(link_lengths)
        self.goal = np.array(goal).T
        self.update_points()

    def update_joints(self, joint_angles):
        self.joint_angles = joint_angles
        self.update_points()

    def update_points(self):
        for k in range(self.n_links):
            a = np.sum(self.joint_angles[:k + 1])
            self.points[k + 1][0] = self.points[k][0] + self.link_lengths[k] * np.cos(a)
            self.points[k + 1][1] = self.points[k][1] + self.link_lengths[k] * np.sin(a)
        self.end_effector = np.array(self.points[self.n_links]).T


def inverse_kinematics(link_lengths, joint_angles, goal_pos):
    """(joint_angles, solution_found) of the Jacobian inverse method from joint_angles towards goal_pos, at most N_ITERATIONS
    trips; found means the end effector is within 0.1 of the goal.  Computed on the device."""
    global _solver
    if _solver is None:
        _solver = _a.BatchArmIK()
    _solver.goal_dist, _solver.max_iterations = 0.1, int(N_ITERATIONS)
    L = [float(v) for v in link_lengths][:N_LINKS]
    res = _solver.solve(L, [[float(v) for v in joint_angles]], [[float(goal_pos[0]), float(goal_pos[1])]])
    angles, found = res.result(0)
    if found:
        print("Solution found in %d iterations." % int(res.iterations[0]))
    return angles, found


def forward_kinematics(link_lengths, joint_angles):
    """The end effector [x, y] of the first N_LINKS links"""
    x = y = 0
    for i in range(1, N_LINKS + 1):
        a = np.sum(joint_angles[:i])
        x += link_lengths[i - 1] * np.cos(a)
        y += link_lengths[i - 1] * np.sin(a)
    return np.array([x, y]).T


def jacobian_inverse(link_lengths, joint_angles):
    """The pseudo-inverse, by numpy on the host, of the script's 2 x N_LINKS matrix: column i sums the links i .. N_LINKS - 1,
    each at the sum of the angles before it.  (inverse_kinematics does not call it: the device takes its own closed-form step.)"""
    J = np.zeros((2, N_LINKS))
    for i in range(N_LINKS):
        for j in range(i, N_LINKS):
            a = np.sum(joint_angles[:j])
            J[0, i] -= link_lengths[j] * np.sin(a)
            J[1, i] += link_lengths[j] * np.cos(a)
    return np.linalg.pinv(J)


def distance_to_goal(current_pos, goal_pos):
    """(errors [dx, dy], their length) from current_pos to goal_pos"""
    d = np.array([goal_pos[0] - current_pos[0], goal_pos[1] - current_pos[1]])
    return d.T, np.hypot(d[0], d[1])


def ang_diff(theta1, theta2):
    """theta1 - theta2 wrapped into [-pi, pi)"""
    return angle_mod(theta1 - theta2)


def get_random_goal():
    """A point of the square of side 15 round the origin, x drawn first, from Python's global generator"""
    import random
    side = 15.0
    return [side * random.random() - side / 2.0 for _ in range(2)]


__all__ = ['angle_mod', 'NLinkArm', 'inverse_kinematics', 'forward_kinematics', 'jacobian_inverse', 'distance_to_goal', 'ang_diff',
           'get_random_goal', 'Kp', 'dt', 'N_ITERATIONS', 'N_LINKS']

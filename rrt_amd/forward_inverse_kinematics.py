"""Names of 01_forward_inverse_kinematics.py as its cells use them.  The MI355X mirror: forward_kinematics and
inverse_kinematics are batches of one on robotics-path-planning_amd/armdh.py (same arguments, same return types; the step of
inverse_kinematics is the package's own definition); no CPU fallback.  transformation_matrix, basic_jacobian and the
pose functions are a few lines of host arithmetic: one matrix needs no device.  A link is a row [theta, alpha, a, d], the
script's live column order.  plot=True is refused: nothing is drawn, and no matplotlib is imported."""
import math
import random

import numpy as np

from . import armdh as _a

_solver = None


def _device():
    global _solver
    if _solver is None:
        _solver = _a.BatchArmDH()
    return _solver


def random_val(min_val, max_val):
    return min_val + random.random() * (max_val - min_val)


def _flag(T):
    return -1 if T[0, 3] < 0 else 1


def rot2quat(transmat):
    """(qw, qx, qy, qz) of the rotation part; the vector part changes sign with a negative x of the translation, as in the script"""
    T, f = transmat, _flag(transmat)
    qw = 0.5 * math.sqrt(1 + T[0, 0] + T[1, 1] + T[2, 2])
    return qw, f * (T[2, 1] - T[1, 2]) / (4 * qw), f * (T[0, 2] - T[2, 0]) / (4 * qw), f * (T[1, 0] - T[0, 1]) / (4 * qw)


def quat2rpy(quat):
    qw, qx, qy, qz = quat
    s, c = 2 * (qy * qz + qw * qx), 1 - 2 * (qx ** 2 + qy ** 2)
    return (math.atan2(s, c), math.atan2(-2 * (qx * qz - qw * qy), math.sqrt(4 * (qy * qz + qw * qx) ** 2 + c ** 2)),
            math.atan2(2 * (qx * qy + qw * qz), 1 - 2 * (qy ** 2 + qz ** 2)))


def rot2euler(transmat):
    T, f = transmat, _flag(transmat)
    return (math.atan2(f * math.sqrt(T[0, 2] ** 2 + T[1, 2] ** 2), T[2, 2]), math.atan2(f * T[1, 2], f * T[0, 2]),
            math.atan2(f * T[2, 1], -1 * f * T[2, 0]))


def rot2euler2(transmat):
    """ZYZ angles with the first one folded into [-pi/2, pi/2]"""
    T = transmat
    alpha = math.atan2(T[1][2], T[0][2])
    for shift in (math.pi, -math.pi):
        if not (-math.pi / 2 <= alpha <= math.pi / 2):
            alpha = math.atan2(T[1][2], T[0][2]) + shift
    sa, ca = math.sin(alpha), math.cos(alpha)
    return alpha, math.atan2(T[0][2] * ca + T[1][2] * sa, T[2][2]), math.atan2(-T[0][0] * sa + T[1][0] * ca, -T[0][1] * sa + T[1][1] * ca)


def transformation_matrix(link_params):
    """The classic (distal) DH matrix of a row [theta, alpha, a, d]"""
    theta, alpha, a, d = link_params[0], link_params[1], link_params[2], link_params[3]
    st, ct, sa, ca = math.sin(theta), math.cos(theta), math.sin(alpha), math.cos(alpha)
    return np.array([[ct, -st * ca, st * sa, a * ct], [st, ct * ca, -ct * sa, a * st], [0, sa, ca, d], [0, 0, 0, 1]])


def basic_jacobian(trans_prev, ee_pos):
    z = np.array(trans_prev[0:3, 2])
    return np.hstack((np.cross(z, ee_pos - np.array(trans_prev[0:3, 3])), z))


def forward_kinematics(link_list):
    """(local transforms, global transforms, the 6 x N Jacobian); the global transforms and the Jacobian are computed on the
    device"""
    fw = _device().forward(np.asarray(link_list, dtype=np.float64))
    if not fw.ok[0]:
        raise ValueError("forward_kinematics: a theta at or beyond 105 414 357 rad")
    return [transformation_matrix(r) for r in link_list], [t.copy() for t in fw.transforms_of(0)], fw.jacobian_of(0).copy()


def inverse_kinematics(iter_cnt, link_list, ref_ee_pose, plot=False, plot_anim=False, save_path=None, method="newton", eps=1e-5,
                       step_div=200.0):
    """iter_cnt trips of theta += step / 200 towards ref_ee_pose; column 0 of link_list is changed in place, as in the script.
    Computed on the device.  plot=True is refused."""
    if plot or plot_anim:
        raise ValueError("inverse_kinematics: nothing is drawn here; call it with plot=False and draw the returned link_list")
    res = _device().solve(np.asarray(link_list, dtype=np.float64), None, ref_ee_pose, iter_cnt=iter_cnt, step_div=step_div, method=method,
                          eps=eps)
    for row, t in zip(link_list, res.result(0)):
        row[0] = float(t)
    return res


__all__ = ['random_val', 'rot2quat', 'quat2rpy', 'rot2euler', 'rot2euler2', 'transformation_matrix', 'basic_jacobian',
           'forward_kinematics', 'inverse_kinematics']

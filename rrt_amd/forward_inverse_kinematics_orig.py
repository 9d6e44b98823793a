"""Names of 01_forward_inverse_kinematics_orig.py as its cells use them: Link and NLinkArm over rows [theta, alpha, a, d].  The
MI355X mirror: NLinkArm.forward_kinematics, basic_jacobian and inverse_kinematics (theta += step / 100, the twin's setting) are
batches of one on robotics-path-planning_amd/armdh.py; no CPU fallback.  The angle bookkeeping (send_angles, update_joint_angles,
get_angles, convert_joint_angles_sim_to_mycobot) is host arithmetic.  plot=True is refused: nothing is drawn."""
import math

import numpy as np

from . import forward_inverse_kinematics as _f
from .forward_inverse_kinematics import random_val  # noqa: F401

PLOT_AREA = 0.5


def _wrapped(angle):
    """angle brought into [-pi, pi] by whole turns, one at a time as the script does"""
    while angle > math.pi:
        angle -= 2 * math.pi
    while angle < -math.pi:
        angle += 2 * math.pi
    return angle


class Link:
    def __init__(self, dh_params):
        self.dh_params_ = dh_params

    def transformation_matrix(self):
        return _f.transformation_matrix(self.dh_params_)

    @staticmethod
    def basic_jacobian(trans_prev, ee_pos):
        return _f.basic_jacobian(trans_prev, np.asarray(ee_pos))


class NLinkArm:
    def __init__(self, dh_params_list):
        self.link_list = [Link(p) for p in dh_params_list]

    def _rows(self):
        return [lk.dh_params_ for lk in self.link_list]

    @staticmethod
    def convert_joint_angles_sim_to_mycobot(joint_angles):
        conv_mul = [-1.0, -1.0, 1.0, -1.0, -1.0, -1.0]
        conv_add = [0.0, -math.pi / 2, 0.0, -math.pi / 2, math.pi / 2, 0.0]
        return [_wrapped(a * m + c) for a, m, c in zip(joint_angles, conv_mul, conv_add)]

    def transformation_matrix(self):
        return _f.forward_kinematics(self._rows())[1][-1]

    def forward_kinematics(self, plot=False):
        if plot:
            raise ValueError("NLinkArm.forward_kinematics: nothing is drawn here")
        T = self.transformation_matrix()
        return [T[0, 3], T[1, 3], T[2, 3], *_f.rot2euler2(T)]

    def basic_jacobian(self):
        return _f.forward_kinematics(self._rows())[2]

    def euler_angle(self):
        return _f.rot2euler2(self.transformation_matrix())

    def inverse_kinematics(self, iter_cnt, ref_ee_pose, plot=False, plot_anim=False, save_path=None):
        """iter_cnt trips of theta += step / 100; the links' theta are changed in place"""
        return _f.inverse_kinematics(iter_cnt, self._rows(), ref_ee_pose, plot=plot, plot_anim=plot_anim, step_div=100.0)

    def send_angles(self, joint_angle_list):
        for lk, a in zip(self.link_list, joint_angle_list):
            lk.dh_params_[0] = a

    def update_joint_angles(self, diff_joint_angle_list):
        for lk, d in zip(self.link_list, diff_joint_angle_list):
            lk.dh_params_[0] += d

    def get_angles(self):
        return [_wrapped(lk.dh_params_[0]) for lk in self.link_list]


__all__ = ['Link', 'NLinkArm', 'random_val', 'PLOT_AREA']

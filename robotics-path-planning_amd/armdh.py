"""Batched kinematics of n-link arms in 3-D on the GPU: Denavit-Hartenberg chains, the 6 x N Jacobian, the pose functions and the
Newton-Raphson / Levenberg-Marquardt inverse kinematics for many (arm, joint angles, reference pose) queries in one call.

    dh = BatchArmDH()
    fw = dh.forward(link_list, joint_angles)                 # one arm of rows [theta, alpha, a, d], (Q, N) joint angles
    fw.transforms_of(3)[-1], fw.jacobian_of(3), fw.euler2[3]
    res = dh.solve(link_list, starts, ref_ee_poses)          # the script's 500 trips of theta += step / 200
    res.result(3)                                            # the joint angles as the script leaves them in link_list

For every query forward() does what forward_kinematics(link_list) of 01_forward_inverse_kinematics.py (:223-245) returns, plus
rot2euler2, rot2euler, rot2quat and quat2rpy of the last transform; solve() does what inverse_kinematics (:367-438) does without
the drawing.  Forward kinematics, the Jacobian, the pose functions, diff_pose, K_zyz and the update are the reference's doubles
(on the golden host, README).  The step is this package's own definition (csrc/rpp_armdh.h): a one-sided Jacobi SVD
with numpy's cut for "newton", the script's commented formula solved by Cholesky for "lm"; solves agree with the reference to a
measured tolerance away from singular poses and the fold of rot2euler2.

There is no CPU fallback: without a device BatchArmDH raises RrtxError.
"""
import numpy as np

from . import _abi

METHODS = {"newton": _abi.ARMDH_NEWTON, "lm": _abi.ARMDH_LM}


def pack_dh_arms(arms):
    """(link_off int64 (n_arms + 1,), dh float64 (links, 4)): one arm (an (N, 4) array of rows [theta, alpha, a, d]) or a list of
    arms"""
    one = len(arms) > 0 and np.ndim(arms[0]) == 1
    rows = [np.asarray(a, dtype=np.float64) for a in ([arms] if one else list(arms))]
    for r in rows:
        if r.ndim != 2 or r.shape[1] != 4:
            raise ValueError("BatchArmDH: an arm is an (N, 4) array of rows [theta, alpha, a, d]")
    link_off = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        link_off[1:] = np.cumsum([len(r) for r in rows])
    return link_off, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4)), dtype=np.float64)


class _Rows:
    """What the results share: CSR offsets in links"""

    def __len__(self):
        return len(self.status)

    def _span(self, i):
        return int(self.offsets[i]), int(self.offsets[i + 1])

    @property
    def ok(self):
        return self.status == _abi.ARMDH_OK


class ArmDHForward(_Rows):
    """One batch of forward passes.  Per query: status (ARMDH_OK, or ARMDH_NONFINITE: a theta at or beyond 105 414 357 rad, where
    the device's sin / cos end -- the query's outputs are zero), position (Q, 3), euler2 (rot2euler2), euler (rot2euler), quat
    (rot2quat; NaN where the interpreter raises on the square root of a negative number), rpy (quat2rpy of it); offsets (Q + 1,) in
    links into transforms (links, 4, 4), the global transforms, and 6 * offsets into the flat Jacobians; partial; kernel_ms."""

    def __init__(self, status, values, offsets, transforms, jac, partial=False, kernel_ms=0.0):
        self.status, self.offsets, self.transforms, self._jac = status, offsets, transforms, jac
        self.position, self.euler2, self.euler = values[:, 0:3], values[:, 3:6], values[:, 6:9]
        self.quat, self.rpy = values[:, 9:13], values[:, 13:16]
        self.partial, self.kernel_ms = partial, kernel_ms

    def transforms_of(self, i):
        """transmat_global_list of query i, (N, 4, 4)"""
        a, b = self._span(i)
        return self.transforms[a:b]

    def jacobian_of(self, i):
        """basic_jacobian_mat of query i, (6, N)"""
        a, b = self._span(i)
        return self._jac[6 * a:6 * b].reshape(6, b - a)


class ArmDHResult(_Rows):
    """One batch of solves.  Per query: status (ARMDH_OK; ARMDH_NONFINITE: an angle left the finite numbers or reached
    105 414 357 rad; ARMDH_NO_CONVERGENCE: the Jacobi sweep cap or a Cholesky pivot <= 0 -- the lane stopped there, the angles as
    they stand), pose (Q, 6) x, y, z, alpha, beta, gamma from one more forward pass over the returned angles, pose_error =
    ref - pose, kappa_max and n_cut (newton: the largest sigma_1 / smallest kept sigma met, and the trips on which a singular
    value was cut); angles: (Q, N) when all arms have one N, else flat with offsets (Q + 1,); partial; kernel_ms."""

    def __init__(self, status, values, kappa_max, n_cut, offsets, flat, partial=False, kernel_ms=0.0):
        self.status, self.pose, self.pose_error = status, values[:, 0:6], values[:, 6:12]
        self.kappa_max, self.n_cut, self.offsets, self._flat = kappa_max, n_cut, offsets, flat
        n = np.diff(offsets)
        self.angles = flat.reshape(len(n), int(n[0])) if len(n) and np.all(n == n[0]) else flat
        self.partial, self.kernel_ms = partial, kernel_ms

    def angles_of(self, i):
        a, b = self._span(i)
        return self._flat[a:b]

    def result(self, i):
        """The joint angles of query i as inverse_kinematics leaves them in column 0 of link_list"""
        return self.angles_of(i).copy()


class BatchArmDH:
    """Forward and inverse kinematics for batches of DH arms of 1 .. 8 links; device buffers are kept between calls."""

    def __init__(self, device=0):
        self._dh = _abi.ArmDH(device)

    def close(self):
        self._dh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @staticmethod
    def _pack(arms, joint_angles, arm, Q=None):
        """-> (link_off, dh, arm int32 or None, flat angles or None, Q)"""
        link_off, dh = pack_dh_arms(arms)
        n_arms = len(link_off) - 1
        ar = None if arm is None else np.ascontiguousarray(arm, dtype=np.int32).reshape(-1)
        rows = None
        if joint_angles is not None:
            ja = joint_angles
            rows = [np.asarray(r, dtype=np.float64).reshape(-1) for r in (ja if (len(ja) and np.ndim(ja[0])) else [ja])]
        if Q is None:
            Q = len(ar) if ar is not None else (len(rows) if rows is not None else n_arms)
        if ar is None and n_arms > 1:
            if n_arms != Q:
                raise ValueError("BatchArmDH: %d arms and %d queries: say which arm each query moves" % (n_arms, Q))
            ar = np.arange(Q, dtype=np.int32)
        if ar is not None and len(ar) != Q:
            raise ValueError("BatchArmDH: %d arm indices for %d queries" % (len(ar), Q))
        flat = None
        if rows is not None:
            inside = ar is None or not len(ar) or (ar.min() >= 0 and ar.max() < n_arms)
            want = int(np.diff(link_off)[ar if ar is not None else np.zeros(Q, dtype=np.int64)].sum()) if (inside and n_arms) else None
            if len(rows) == 1 and Q != 1 and want != len(rows[0]):   # one row for every query
                rows = rows * Q
            elif len(rows) == 1 and Q != 1:                          # flat, query after query
                pass
            elif len(rows) != Q:
                raise ValueError("BatchArmDH: %d rows of angles for %d queries" % (len(rows), Q))
            flat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0), dtype=np.float64)
            if want is not None and want != len(flat):
                raise ValueError("BatchArmDH: the joint angles are not as many as the links of the queries' arms")
        return link_off, dh, ar, flat, Q

    def forward(self, arms, joint_angles=None, arm=None):
        """arms: one arm ((N, 4) rows [theta, alpha, a, d]) or a list of arms; joint_angles: (Q, N) (or a list of Q rows) that
        replace column 0 per query, None: the arms' own column 0, one query per arm; arm[q]: the arm of query q when there are
        several (default: query q moves arm q)."""
        link_off, dh, ar, flat, Q = self._pack(arms, joint_angles, arm)
        rc = self._dh.forward(link_off, dh, ar, flat, Q)
        status, values, _, _, n_links = self._dh.records()
        off, _ = self._dh.angles(Q, n_links, want_angles=False)
        return ArmDHForward(status, values, off, self._dh.transforms(n_links), self._dh.jacobians(n_links),
                            rc == _abi.RRTX_PARTIAL, self._dh.kernel_ms()[0])

    def solve(self, arms, joint_angles, ref_ee_pose, iter_cnt=500, step_div=200.0, method="newton", eps=1e-5, arm=None):
        """inverse_kinematics(iter_cnt, link_list, ref_ee_pose) for every query: exactly iter_cnt trips of theta += step /
        step_div (200 in the script, 100 in its _orig twin), no convergence test.  ref_ee_pose: (Q, 6) rows x, y, z, alpha,
        beta, gamma, or one row for all queries; joint_angles: the starts, as in forward (None: the arms' column 0)."""
        if method not in METHODS:
            raise ValueError("BatchArmDH: method is 'newton' or 'lm'")
        ref = np.ascontiguousarray(ref_ee_pose, dtype=np.float64).reshape(-1, 6)
        Q = None
        if len(ref) != 1:
            Q = len(ref)
        link_off, dh, ar, flat, Q = self._pack(arms, joint_angles, arm, Q)
        if len(ref) == 1 and Q != 1:
            ref = np.ascontiguousarray(np.tile(ref, (Q, 1)))
        rc = self._dh.solve(link_off, dh, ar, flat, ref, iter_cnt, step_div, METHODS[method], eps)
        status, values, kappa, n_cut, n_links = self._dh.records()
        off, ang = self._dh.angles(Q, n_links)
        return ArmDHResult(status, values, kappa, n_cut, off, ang, rc == _abi.RRTX_PARTIAL, self._dh.kernel_ms()[0])

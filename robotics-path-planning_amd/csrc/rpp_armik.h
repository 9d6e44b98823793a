// rpp_armik.h -- Jacobian inverse kinematics of a planar N-link arm and the driver's P-control loop, host + device source like
// rpp_armnav.h and rpp_spline.h.
// Reference: 00_simple_2d_inverse_kinematics_01.py (script 01; 00_simple_2d_inverse_kinematics_02_straight_control.py has the
// same functions)
//   angle_mod :14-32, NLinkArm.update_points :59-68, inverse_kinematics :71-85, forward_kinematics :88-93,
//   jacobian_inverse :96-105, distance_to_goal :108-111, ang_diff :114-118, the driver's loop :189-200.
//
// What is the reference's, double for double (no FMA contraction may be applied to this file):
//   np.sum(joint_angles[:i])   numpy's pairwise sum (ik_sum): 0.0 for the empty slice; left to right from 0.0 below 8 elements;
//                              from 8 up eight accumulators r[k] = a[k], r[k] += a[8 + k] once 16 are reached,
//                              ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the remainder added left to right
//   forward_kinematics         x = 0; x = x + L[i - 1] * cos(S_i) for i = 1 .. N, S_i = np.sum(joint_angles[:i]); update_points
//                              is the same chain.  np.cos / np.sin of a scalar are libm's (rpp_glibc_cos / rpp_glibc_sin) --
//                              up to |S| < 105 414 357.85 (high word below 0x419921fb), where the replicas end: libm goes on
//                              to its arbitrary-precision reduction there, the replicas do not restate it.  A trip that meets
//                              such a sum, or one that is not finite, stops the query: kIkNonfinite, the angles as they stand
//   J (before pinv)            the script's own slices: J[0, i] = 0, then J[0, i] -= L[j] * sin(S_j) for j = i .. N - 1 in that
//                              order, with S_j the sum of the first j angles (not j + 1); J[1, i] += L[j] * cos(S_j) likewise.
//                              Every column is its own left-to-right chain.  S_0 .. S_N and their sin / cos are formed once a
//                              trip and serve both (S_1 .. S_N the position, S_0 .. S_{N-1} the terms of J)
//   distance_to_goal           errors = goal - current_pos per axis, np.hypot = rpp_glibc_hypot; the tests distance < goal_dist
//                              (inverse_kinematics) and distance > goal_dist (the driver) as written
//   the driver's update        a + (Kp * angle_mod(goal - a)) * dt, angle_mod(x) = (x + pi) % (2 pi) - pi with numpy's floored `%`
//
// What is THIS PACKAGE'S OWN DEFINITION: the step joint_angles + matmul(pinv(J), errors).  np.linalg.pinv is LAPACK's SVD and
// not one arithmetic; here the step is a closed form for the 2 x N matrix, operation by operation (ik_step; e = errors):
//   a = sum J0i * J0i, b = sum J0i * J1i, c = sum J1i * J1i      each left to right over i from 0.0, products rounded first
//   tr = a + c, det = a * c - b * b
//   rank 0   tr == 0 (J is all zero):                    w = (0, 0)
//   rank 1   N == 1, or not det > 2^-40 * (tr * tr):     q = tr * tr, w = ((a * e0 + b * e1) / q, (b * e0 + c * e1) / q)
//   rank 2   otherwise:                                  w = ((c * e0 - b * e1) / det, (a * e1 - b * e0) / det)
//   delta_i = J0i * w0 + J1i * w1, angle_i = angle_i + delta_i
// The rank-1 form is J^T v (v^T e) / lambda_1 for J J^T = lambda_1 v v^T, where lambda_1 = tr and v v^T = J J^T / tr: no root
// and no rotation is needed.  A 2 x 1 matrix always has rank 1 and its det is rounding noise; a J with an exactly zero row
// (all angles 0) has det == 0.  2^-40 is a condition number of 2^20: beyond it det holds fewer than 12 bits.  numpy's own cut
// (sigma_2 <= 1e-15 sigma_1) cannot be decided from J J^T in doubles, so steps on which the two decisions differ are outside the
// comparison with the reference (tests/armik_util.py).  tests/armik_oracle.py states the same operations in Python.
#pragma once
#include "rpp_dubins.h"   // np_mod, angle_mod_pi

namespace rpp {

constexpr int kIkMaxLinks = 16;
constexpr int kIkFound = 0, kIkNotFound = 1, kIkNonfinite = 2, kIkStepCap = 3;
constexpr int kIkGoOn = -1;
constexpr double kIkRankEps = 9.094947017729282e-13;   // 2^-40

// One lane's array of up to 16 doubles: element k lies k * stride doubles on (stride 1 on the host, the wave's width in
// lane-striped LDS)
struct IkVec {
  double* p;
  int stride;
  RPP_HD double& operator[](int k) const { return p[k * stride]; }
};

struct IkPose {
  double x, y;     // current_pos
  double ex, ey;   // errors
  double dist;
};

RPP_HD static inline bool ik_finite(double v) { return (d2b(v) & 0x7ff0000000000000ULL) != 0x7ff0000000000000ULL; }
// inside the domain of rpp_glibc_sin / rpp_glibc_cos (NaN and the infinities are outside)
RPP_HD static inline bool ik_trig_domain(double S) { return (uint32_t)((d2b(S) >> 32) & 0x7fffffffu) < 0x419921fbu; }

// np.sum(a[:n]) for 0 <= n <= 16
RPP_HD static inline double ik_sum(const IkVec& a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int k = 0; k < n; k++) r = r + a[k];
    return r;
  }
  double r[8];
#pragma unroll
  for (int k = 0; k < 8; k++) r[k] = a[k];
  int i = 8;
  for (; i + 8 <= n; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = r[k] + a[i + k];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) res = res + a[i];
  return 0.0 + res;   // the reduction starts from the identity
}

// forward_kinematics / update_points and distance_to_goal; with TERMS the terms of J, L[j] * sin(S_j) and L[j] * cos(S_j),
// are left in j0[j] and j1[j] for ik_jacobian.  false, and p untouched, when a prefix sum lies outside the replicas' domain
template <bool TERMS>
RPP_HD static inline bool ik_forward(const IkVec& ang, const IkVec& len, int n, double gx, double gy, const IkVec& j0,
                                     const IkVec& j1, IkPose& p) {
  double x = 0.0, y = 0.0;
  for (int i = 0; i <= n; i++) {
    if (!TERMS && i == 0) continue;
    const double S = ik_sum(ang, i);
    if (!ik_trig_domain(S)) return false;
    const double sn = rpp_glibc_sin(S), cs = rpp_glibc_cos(S);
    if (i > 0) {
      const double L = len[i - 1];
      x = x + L * cs;
      y = y + L * sn;
    }
    if (TERMS && i < n) {
      const double L = len[i];
      j0[i] = L * sn;
      j1[i] = L * cs;
    }
  }
  p.x = x;
  p.y = y;
  p.ex = gx - x;
  p.ey = gy - y;
  p.dist = rpp_glibc_hypot(p.ex, p.ey);
  return true;
}

// J from its terms, in place: column i reads the terms i .. N - 1 and is written over term i, which no later column reads
RPP_HD static inline void ik_jacobian(const IkVec& j0, const IkVec& j1, int n) {
  for (int i = 0; i < n; i++) {
    double a0 = 0.0, a1 = 0.0;
    for (int j = i; j < n; j++) {
      a0 = a0 - j0[j];
      a1 = a1 + j1[j];
    }
    j0[i] = a0;
    j1[i] = a1;
  }
}

// (w0, w1) of the step and the rank the rule chose
RPP_HD static inline int ik_step_w(const IkVec& j0, const IkVec& j1, int n, double e0, double e1, double& w0, double& w1) {
  double a = 0.0, b = 0.0, c = 0.0;
  for (int i = 0; i < n; i++) {
    const double u = j0[i], v = j1[i];
    a = a + u * u;
    b = b + u * v;
    c = c + v * v;
  }
  const double tr = a + c;
  const double det = a * c - b * b;
  if (tr == 0.0) {
    w0 = 0.0;
    w1 = 0.0;
    return 0;
  }
  if (n == 1 || !(det > kIkRankEps * (tr * tr))) {
    const double q = tr * tr;
    w0 = (a * e0 + b * e1) / q;
    w1 = (b * e0 + c * e1) / q;
    return 1;
  }
  w0 = (c * e0 - b * e1) / det;
  w1 = (a * e1 - b * e0) / det;
  return 2;
}

// angles += J^T w; false when an angle left the finite numbers
RPP_HD static inline bool ik_step(const IkVec& ang, const IkVec& j0, const IkVec& j1, int n, double e0, double e1) {
  double w0, w1;
  ik_step_w(j0, j1, n, e0, e1, w0, w1);
  bool finite = true;
  for (int i = 0; i < n; i++) {
    const double v = ang[i] + (j0[i] * w0 + j1[i] * w1);
    ang[i] = v;
    finite = finite && ik_finite(v);
  }
  return finite;
}

// One trip of inverse_kinematics :75-84: kIkFound (the angles are the answer), kIkNonfinite (the step made an angle that is
// not finite, or the angles have left the replicas' domain; p is then the last pose that was computed), or kIkGoOn
RPP_HD static inline int ik_trip(const IkVec& ang, const IkVec& len, const IkVec& j0, const IkVec& j1, int n, double gx,
                                 double gy, double goal_dist, IkPose& p) {
  if (!ik_forward<true>(ang, len, n, gx, gy, j0, j1, p)) return kIkNonfinite;
  if (p.dist < goal_dist) return kIkFound;
  ik_jacobian(j0, j1, n);
  return ik_step(ang, j0, j1, n, p.ex, p.ey) ? kIkGoOn : kIkNonfinite;
}

// One step of the driver's loop :195-198: the update towards goal_ang, then the pose.  For |Kp * dt| <= 1
// angles that start within 1e6 stay within pi of where they started and their sums inside the replicas' domain; a huge
// Kp * dt can leave it: false then (p untouched), and the caller stops with kIkNonfinite
RPP_HD static inline bool ik_move_step(const IkVec& ang, const IkVec& len, const IkVec& goal_ang, int n, double gx, double gy,
                                       double Kp, double dt, IkPose& p) {
  for (int i = 0; i < n; i++) {
    const double a = ang[i];
    ang[i] = a + (Kp * angle_mod_pi(goal_ang[i] - a)) * dt;
  }
  return ik_forward<false>(ang, len, n, gx, gy, ang, ang, p);
}

}  // namespace rpp

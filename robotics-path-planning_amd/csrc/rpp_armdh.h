// rpp_armdh.h -- n-link arm in 3-D: Denavit-Hartenberg chains, the 6 x N Jacobian, the pose functions and the Newton-Raphson /
// Levenberg-Marquardt inverse kinematics, host + device source like rpp_armik.h.
// Reference: 01_forward_inverse_kinematics.py (rot2quat :89, quat2rpy :109, rot2euler :120, rot2euler2 :141,
// transformation_matrix :161, basic_jacobian :212, forward_kinematics :223, inverse_kinematics :367, the Levenberg-Marquardt
// variant :582-587) and its class-style twin 01_forward_inverse_kinematics_orig.py (the same arithmetic, step / 100).
//
// What is the reference's, double for double (no FMA contraction may be applied to this file; fused products are explicit):
//   transformation_matrix   st, ct, sa, ca = libm's sin / cos (rpp_glibc_sin / rpp_glibc_cos; sa, ca are formed once per query);
//                           the entries as written: (-st) * ca, st * sa, a * ct, st, ct * ca, (-ct) * sa, a * st, 0, sa, ca, d,
//                           0, 0, 0, 1
//   np.dot of two 4 x 4     C[i][j] = acc, acc = 0.0, acc = fma(A[i][k], B[k][j], acc) for k = 0 .. 3, all 16 entries, the row
//                           0 0 0 1 included (tests/test_armdh_host.py pins that form on the golden host)
//   forward_kinematics      the chain from the identity; the reference walks it twice with identical results, here once: before
//                           link i is multiplied on, the prefix's origin T[0:3, 3] and z axis T[0:3, 2] are kept
//   basic_jacobian          d = ee_pos - pos_prev per axis; np.cross(z, d) unfused: z1 * d2 - z2 * d1, z2 * d0 - z0 * d2,
//                           z0 * d1 - z1 * d0; rows 3 .. 5 are z
//   rot2euler2              alpha = atan2(T12, T02); when not -pi/2 <= alpha <= pi/2 the atan2 again + pi, and when still not,
//                           the atan2 again - pi; beta and gamma as written (sin / cos of alpha are libm's)
//   rot2euler, rot2quat, quat2rpy   as written; ** 2 is pow(|x|, 2.0) (py_sq), sqrt is IEEE (a negative argument gives NaN
//                           where the interpreter raises)
//   diff_pose, K_zyz        ref - pose per entry; K = [[0, -sin(alpha), cos(alpha) * sin(beta)], [0, cos(alpha),
//                           sin(alpha) * sin(beta)], [1, 0, cos(beta)]]
//   the update              theta[k] = theta[k] + delta[k] / step_div
// sin / cos of a theta exist up to |theta| < 105 414 357.85 (rpp_armik.h); a trip that meets a theta at or beyond it, or one
// that is not finite, stops the query with kDhNonfinite, the angles as they stand.
//
// What is THIS PACKAGE'S OWN DEFINITION: the step.  np.linalg.pinv is LAPACK's SVD and not one arithmetic.
//   e            e[0..2] = diff[0..2]; e[3 + r] = (K[r][0] * diff[3] + K[r][1] * diff[4]) + K[r][2] * diff[5], the zeros and the one
//                of K multiplied like the rest (the reference forms (pinv . K_alpha) . diff: another rounding)
//   newton       one-sided Jacobi on the six rows of J (vectors of length N), V = the 6 x 6 identity, F = the sum of all J[r][k]^2
//                (r outer, k inner, from 0.0, products rounded first).
//                A sweep visits the pairs (p, q), p < q, p outer, q inner.  For a pair: a = sum J[p][k]^2, b = sum J[q][k]^2,
//                c = sum J[p][k] * J[q][k], each left to right over k from 0.0.  The pair is skipped when c == 0, or
//                |c| <= 2^-50 * sqrt(a * b), or a <= 2^-120 * F, or b <= 2^-120 * F (a row below 2^-60 of the matrix is cut
//                by the rule below whatever it points at, and in a rank-deficient J it would never come to rest).
//                Otherwise zeta = (b - a) / (2 * c), t = sign(zeta) / (|zeta| + sqrt(1 + zeta * zeta)) with sign(0) = +1,
//                cs = 1 / sqrt(1 + t * t), sn = cs * t, and for the rows of J and likewise the columns p, q of V:
//                (x_p, x_q) = (cs * x_p - sn * x_q, sn * x_p + cs * x_q).
//                Sweeps end after one without a rotation; after 30 sweeps that all rotated the trip fails: kDhNoConvergence.
//                s_i = sum J[i][k]^2 (left to right), sigma_i = sqrt(s_i), sigma_max the largest; row i is kept when
//                sigma_i > 1e-15 * sigma_max (numpy's cut).  w_i = (V[0][i] * e[0] + V[1][i] * e[1] + ... + V[5][i] * e[5]) / s_i,
//                summed left to right from 0.0; delta[k] = the sum over the kept i in ascending order, from 0.0, of J[i][k] * w_i.
//                kappa = sigma_max / the smallest kept sigma (0 when nothing is kept); the trip counts as cut when fewer than
//                min(6, N) rows are kept.
//   lm           jv[r][k] = J[r][k] for r < 3, jv[3 + r][k] = (K[r][0] * J[3][k] + K[r][1] * J[4][k]) + K[r][2] * J[5][k];
//                W = (1, 1, 1, pi/2, pi/2, pi/2); for i >= j: M[i][j] = the sum over r = 0 .. 5, left to right from 0.0, of
//                (jv[r][i] * W[r]) * jv[r][j], and eps added to the diagonal afterwards; rhs[i] = the same sum of
//                (jv[r][i] * W[r]) * diff[r] (diff, not e: the script's formula).  Cholesky by columns j = 0 .. N - 1:
//                s = M[j][j], s = s - L[j][k] * L[j][k] for k < j ascending; not s > 0: kDhNoConvergence; L[j][j] = sqrt(s);
//                for i > j: s = M[i][j], s = s - L[i][k] * L[j][k] for k < j, L[i][j] = s / L[j][j].  y[i] = (rhs[i] minus
//                L[i][k] * y[k] for k < i ascending) / L[i][i], i ascending; delta[i] = (y[i] minus L[k][i] * delta[k] for
//                k = i + 1 .. N - 1 ascending) / L[i][i], i descending.
// tests/armdh_oracle.py states the same operations in Python.
#pragma once
#include "rpp_dubins.h"

namespace rpp {

constexpr int kDhMaxLinks = 8;
constexpr int kDhOk = 0, kDhNonfinite = 1, kDhNoConvergence = 2;
constexpr int kDhNewton = 0, kDhLm = 1;
constexpr int kDhMaxSweeps = 30;
constexpr double kDhPairEps = 8.881784197001252e-16;    // 2^-50
constexpr double kDhRowEps = 7.52316384526264e-37;      // 2^-120
constexpr double kDhCut = 1e-15;
constexpr double kDhHalfPi = 1.5707963267948966, kDhPi = 3.141592653589793;
// One lane's doubles: element k lies k * stride doubles on (stride 1 on the host, the wave's width in lane-striped LDS)
// theta, sin / cos of alpha, a, d per link; J row-major 6 x 8; delta is written over row 0 of J once a column of J has been
// read for the last time
constexpr int kDhTh = 0, kDhSa = 8, kDhCa = 16, kDhA = 24, kDhD = 32, kDhJ = 40, kDhDelta = kDhJ, kDhM = 88;
constexpr int kDhLaneDoublesNewton = 88, kDhLaneDoublesLm = 124;   // lm: + the 36 of the lower triangle of M

struct DhVec {
  double* p;
  int stride;
  RPP_HD double& operator[](int k) const { return p[k * stride]; }
};

struct DhStats {
  double kappa_max;
  int n_cut;
};

RPP_HD static inline bool dh_finite(double v) { return (d2b(v) & 0x7ff0000000000000ULL) != 0x7ff0000000000000ULL; }
RPP_HD static inline bool dh_trig_domain(double S) { return (uint32_t)((d2b(S) >> 32) & 0x7fffffffu) < 0x419921fbu; }

// the lane's arm: sin / cos of alpha once
RPP_HD static inline void dh_load_arm(const DhVec& s, int n, const double* dh /* [n][4] theta alpha a d */) {
  for (int i = 0; i < n; i++) {
    const double al = dh[4 * i + 1];
    s[kDhTh + i] = dh[4 * i];
    s[kDhSa + i] = rpp_glibc_sin(al);
    s[kDhCa + i] = rpp_glibc_cos(al);
    s[kDhA + i] = dh[4 * i + 2];
    s[kDhD + i] = dh[4 * i + 3];
  }
}

// forward_kinematics: T the last global transform, J the Jacobian; with STORE the global transforms go to tf[i][4][4].  false
// when a theta lies outside the replicas' domain (T and J are then unfinished)
template <bool STORE>
RPP_HD static inline bool dh_forward(const DhVec& s, int n, double (&T)[4][4], double* tf) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) T[i][j] = i == j ? 1.0 : 0.0;
  for (int l = 0; l < n; l++) {
    const double th = s[kDhTh + l];
    if (!dh_trig_domain(th)) return false;
    const double st = rpp_glibc_sin(th), ct = rpp_glibc_cos(th);
    const double sa = s[kDhSa + l], ca = s[kDhCa + l], a = s[kDhA + l], d = s[kDhD + l];
    const double B[4][4] = {{ct, (-st) * ca, st * sa, a * ct}, {st, ct * ca, (-ct) * sa, a * st}, {0.0, sa, ca, d}, {0.0, 0.0, 0.0, 1.0}};
#pragma unroll
    for (int r = 0; r < 3; r++) {
      s[kDhJ + r * 8 + l] = T[r][3];         // pos_prev
      s[kDhJ + (3 + r) * 8 + l] = T[r][2];   // z_axis_prev
    }
    double R[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) acc = __builtin_fma(T[i][k], B[k][j], acc);
        R[i][j] = acc;
      }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        T[i][j] = R[i][j];
        if (STORE) tf[l * 16 + i * 4 + j] = R[i][j];
      }
  }
  for (int l = 0; l < n; l++) {
    const double d0 = T[0][3] - s[kDhJ + 0 * 8 + l], d1 = T[1][3] - s[kDhJ + 1 * 8 + l], d2 = T[2][3] - s[kDhJ + 2 * 8 + l];
    const double z0 = s[kDhJ + 3 * 8 + l], z1 = s[kDhJ + 4 * 8 + l], z2 = s[kDhJ + 5 * 8 + l];
    s[kDhJ + 0 * 8 + l] = z1 * d2 - z2 * d1;
    s[kDhJ + 1 * 8 + l] = z2 * d0 - z0 * d2;
    s[kDhJ + 2 * 8 + l] = z0 * d1 - z1 * d0;
  }
  return true;
}

RPP_HD static inline void dh_rot2euler2(const double (&T)[4][4], double& alpha, double& beta, double& gamma) {
  alpha = rpp_glibc_atan2(T[1][2], T[0][2]);
  if (!(-kDhHalfPi <= alpha && alpha <= kDhHalfPi)) alpha = rpp_glibc_atan2(T[1][2], T[0][2]) + kDhPi;
  if (!(-kDhHalfPi <= alpha && alpha <= kDhHalfPi)) alpha = rpp_glibc_atan2(T[1][2], T[0][2]) - kDhPi;
  const double sA = rpp_glibc_sin(alpha), cA = rpp_glibc_cos(alpha);
  beta = rpp_glibc_atan2(T[0][2] * cA + T[1][2] * sA, T[2][2]);
  gamma = rpp_glibc_atan2((-T[0][0]) * sA + T[1][0] * cA, (-T[0][1]) * sA + T[1][1] * cA);
}

RPP_HD static inline void dh_rot2euler(const double (&T)[4][4], double* o) {
  const double flag = T[0][3] < 0 ? -1.0 : 1.0;
  o[0] = rpp_glibc_atan2(flag * __builtin_sqrt(py_sq(T[0][2]) + py_sq(T[1][2])), T[2][2]);
  o[1] = rpp_glibc_atan2(flag * T[1][2], flag * T[0][2]);
  o[2] = rpp_glibc_atan2(flag * T[2][1], (-1.0 * flag) * T[2][0]);
}

RPP_HD static inline void dh_rot2quat(const double (&T)[4][4], double* q) {
  const double flag = T[0][3] < 0 ? -1.0 : 1.0;
  const double qw = 0.5 * __builtin_sqrt(((1.0 + T[0][0]) + T[1][1]) + T[2][2]);
  q[0] = qw;
  q[1] = flag * (T[2][1] - T[1][2]) / (4.0 * qw);
  q[2] = flag * (T[0][2] - T[2][0]) / (4.0 * qw);
  q[3] = flag * (T[1][0] - T[0][1]) / (4.0 * qw);
}

RPP_HD static inline void dh_quat2rpy(const double* q, double* o) {
  const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  o[0] = rpp_glibc_atan2(2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (py_sq(qx) + py_sq(qy)));
  o[1] = rpp_glibc_atan2(-2.0 * (qx * qz - qw * qy),
                         __builtin_sqrt(4.0 * py_sq(qy * qz + qw * qx) + py_sq(1.0 - 2.0 * (py_sq(qx) + py_sq(qy)))));
  o[2] = rpp_glibc_atan2(2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (py_sq(qy) + py_sq(qz)));
}

// x, y, z, alpha, beta, gamma of the last transform
RPP_HD static inline void dh_pose(const double (&T)[4][4], double* pose) {
  pose[0] = T[0][3];
  pose[1] = T[1][3];
  pose[2] = T[2][3];
  dh_rot2euler2(T, pose[3], pose[4], pose[5]);
}

RPP_HD static inline void dh_kzyz(double alpha, double beta, double (&K)[3][3]) {
  const double sA = rpp_glibc_sin(alpha), cA = rpp_glibc_cos(alpha), sB = rpp_glibc_sin(beta), cB = rpp_glibc_cos(beta);
  K[0][0] = 0.0, K[0][1] = -sA, K[0][2] = cA * sB;
  K[1][0] = 0.0, K[1][1] = cA, K[1][2] = sA * sB;
  K[2][0] = 1.0, K[2][1] = 0.0, K[2][2] = cB;
}

// the newton step from J (destroyed) and e into delta; kDhOk or kDhNoConvergence
RPP_HD static inline int dh_step_newton(const DhVec& s, int n, const double (&e)[6], double& kappa, bool& cut) {
  double V[6][6];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) V[i][j] = i == j ? 1.0 : 0.0;
  double F = 0.0;
  for (int r = 0; r < 6; r++)
    for (int k = 0; k < n; k++) {
      const double v = s[kDhJ + r * 8 + k];
      F = F + v * v;
    }
  const double floor_ = kDhRowEps * F;
  bool rotated = true;
  for (int sweep = 0; sweep < kDhMaxSweeps && rotated; sweep++) {
    rotated = false;
#pragma unroll
    for (int p = 0; p < 5; p++)
#pragma unroll
      for (int q = p + 1; q < 6; q++) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int k = 0; k < n; k++) {
          const double u = s[kDhJ + p * 8 + k], v = s[kDhJ + q * 8 + k];
          a = a + u * u;
          b = b + v * v;
          c = c + u * v;
        }
        if (c == 0.0 || dabs(c) <= kDhPairEps * __builtin_sqrt(a * b) || a <= floor_ || b <= floor_) continue;
        rotated = true;
        const double zeta = (b - a) / (2.0 * c);
        const double t = (zeta < 0.0 ? -1.0 : 1.0) / (dabs(zeta) + __builtin_sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / __builtin_sqrt(1.0 + t * t), sn = cs * t;
        for (int k = 0; k < n; k++) {
          const double u = s[kDhJ + p * 8 + k], v = s[kDhJ + q * 8 + k];
          s[kDhJ + p * 8 + k] = cs * u - sn * v;
          s[kDhJ + q * 8 + k] = sn * u + cs * v;
        }
#pragma unroll
        for (int r = 0; r < 6; r++) {
          const double u = V[r][p], v = V[r][q];
          V[r][p] = cs * u - sn * v;
          V[r][q] = sn * u + cs * v;
        }
      }
  }
  if (rotated) return kDhNoConvergence;
  double sq[6], sg[6], smax = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double a = 0.0;
    for (int k = 0; k < n; k++) {
      const double u = s[kDhJ + i * 8 + k];
      a = a + u * u;
    }
    sq[i] = a;
    sg[i] = __builtin_sqrt(a);
    if (sg[i] > smax) smax = sg[i];
  }
  double w[6], smin = 0.0;
  int kept = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const bool keep = sg[i] > kDhCut * smax;
    double dot = 0.0;
#pragma unroll
    for (int r = 0; r < 6; r++) dot = dot + V[r][i] * e[r];
    w[i] = keep ? dot / sq[i] : 0.0;
    if (keep) {
      if (kept == 0 || sg[i] < smin) smin = sg[i];
      kept++;
    } else {
      sq[i] = 0.0;   // marks the row as cut
    }
  }
  for (int k = 0; k < n; k++) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++)
      if (sq[i] != 0.0) acc = acc + s[kDhJ + i * 8 + k] * w[i];
    s[kDhDelta + k] = acc;
  }
  kappa = kept ? smax / smin : 0.0;
  cut = kept < (n < 6 ? n : 6);
  return kDhOk;
}

RPP_HD static inline int dh_tri(int i, int j) { return kDhM + i * (i + 1) / 2 + j; }

// the lm step from J (overwritten by jv), K and diff into delta; kDhOk or kDhNoConvergence
RPP_HD static inline int dh_step_lm(const DhVec& s, int n, const double (&K)[3][3], const double (&diff)[6], double eps) {
  const double W[6] = {1.0, 1.0, 1.0, kDhHalfPi, kDhHalfPi, kDhHalfPi};
  for (int k = 0; k < n; k++) {
    const double j3 = s[kDhJ + 3 * 8 + k], j4 = s[kDhJ + 4 * 8 + k], j5 = s[kDhJ + 5 * 8 + k];
#pragma unroll
    for (int r = 0; r < 3; r++) s[kDhJ + (3 + r) * 8 + k] = (K[r][0] * j3 + K[r][1] * j4) + K[r][2] * j5;
  }
  for (int i = 0; i < n; i++) {
    double wi[6];
#pragma unroll
    for (int r = 0; r < 6; r++) wi[r] = s[kDhJ + r * 8 + i] * W[r];
    for (int j = 0; j <= i; j++) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < 6; r++) acc = acc + wi[r] * s[kDhJ + r * 8 + j];
      s[dh_tri(i, j)] = i == j ? acc + eps : acc;
    }
  }
  for (int i = 0; i < n; i++) {   // rhs[i] reads column i of jv alone and takes its place in row 0
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 6; r++) acc = acc + (s[kDhJ + r * 8 + i] * W[r]) * diff[r];
    s[kDhDelta + i] = acc;
  }
  for (int j = 0; j < n; j++) {
    double d = s[dh_tri(j, j)];
    for (int k = 0; k < j; k++) {
      const double l = s[dh_tri(j, k)];
      d = d - l * l;
    }
    if (!(d > 0.0)) return kDhNoConvergence;
    d = __builtin_sqrt(d);
    s[dh_tri(j, j)] = d;
    for (int i = j + 1; i < n; i++) {
      double v = s[dh_tri(i, j)];
      for (int k = 0; k < j; k++) v = v - s[dh_tri(i, k)] * s[dh_tri(j, k)];
      s[dh_tri(i, j)] = v / d;
    }
  }
  for (int i = 0; i < n; i++) {
    double v = s[kDhDelta + i];
    for (int k = 0; k < i; k++) v = v - s[dh_tri(i, k)] * s[kDhDelta + k];
    s[kDhDelta + i] = v / s[dh_tri(i, i)];
  }
  for (int i = n - 1; i >= 0; i--) {
    double v = s[kDhDelta + i];
    for (int k = i + 1; k < n; k++) v = v - s[dh_tri(k, i)] * s[kDhDelta + k];
    s[kDhDelta + i] = v / s[dh_tri(i, i)];
  }
  return kDhOk;
}

// the step alone, from a J that lies in s already (the tests drive it with the reference's recorded J)
template <int METHOD>
RPP_HD static inline int dh_step(const DhVec& s, int n, const double (&K)[3][3], const double (&diff)[6], double eps, double& kappa,
                                 bool& cut) {
  kappa = 0.0;
  cut = false;
  if (METHOD == kDhLm) return dh_step_lm(s, n, K, diff, eps);
  double e[6];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    e[r] = diff[r];
    e[3 + r] = (K[r][0] * diff[3] + K[r][1] * diff[4]) + K[r][2] * diff[5];
  }
  return dh_step_newton(s, n, e, kappa, cut);
}

// One trip of inverse_kinematics :388-438: kDhOk (the angles moved on), kDhNonfinite or kDhNoConvergence (the angles as they
// stood, but for kDhNonfinite after an update that left the finite numbers)
template <int METHOD>
RPP_HD static inline int dh_trip(const DhVec& s, int n, const double* ref, double step_div, double eps, DhStats& st) {
  double T[4][4];
  if (!dh_forward<false>(s, n, T, nullptr)) return kDhNonfinite;
  double pose[6], diff[6], K[3][3];
  dh_pose(T, pose);
#pragma unroll
  for (int r = 0; r < 6; r++) diff[r] = ref[r] - pose[r];
  dh_kzyz(pose[3], pose[4], K);
  double kappa;
  bool cut;
  const int rc = dh_step<METHOD>(s, n, K, diff, eps, kappa, cut);
  if (rc != kDhOk) return rc;
  if (kappa > st.kappa_max) st.kappa_max = kappa;
  st.n_cut += cut ? 1 : 0;
  bool finite = true;
  for (int k = 0; k < n; k++) {
    const double v = s[kDhTh + k] + s[kDhDelta + k] / step_div;
    s[kDhTh + k] = v;
    finite = finite && dh_finite(v);
  }
  return finite ? kDhOk : kDhNonfinite;
}

// All of inverse_kinematics without the drawing, then one more forward pass: pose (zeros when the final angles lie outside the
// domain) and pose_error = ref - pose.  Returns the status
template <int METHOD>
RPP_HD static inline int dh_solve(const DhVec& s, int n, const double* ref, int iter_cnt, double step_div, double eps, DhStats& st,
                                  double* pose, double* pose_error) {
  st.kappa_max = 0.0;
  st.n_cut = 0;
  int status = kDhOk;
  for (int it = 0; it < iter_cnt; it++) {
    status = dh_trip<METHOD>(s, n, ref, step_div, eps, st);
    if (status != kDhOk) break;
  }
  double T[4][4];
  if (dh_forward<false>(s, n, T, nullptr)) {
    dh_pose(T, pose);
  } else {
    status = kDhNonfinite;
    for (int r = 0; r < 6; r++) pose[r] = 0.0;
  }
  for (int r = 0; r < 6; r++) pose_error[r] = ref[r] - pose[r];
  return status;
}

}  // namespace rpp

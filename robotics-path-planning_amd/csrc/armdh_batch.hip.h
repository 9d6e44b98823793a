// armdh_batch.hip.h -- batched kinematics of n-link arms in 3-D given by Denavit-Hartenberg rows (gfx950): for many (arm, joint
// angles) queries what forward_kinematics and the pose functions of 01_forward_inverse_kinematics.py return, and for many (arm,
// start angles, reference pose) queries its inverse_kinematics, Newton-Raphson or Levenberg-Marquardt.  Scalar pieces:
// csrc/rpp_armdh.h.
//
//   armdh_forward_kernel         one query per lane: the record (position, the three angle conventions, the quaternion), the
//                                Jacobian and the CSR global transforms
//   armdh_solve_kernel<METHOD>   one query per lane, exactly iter_cnt trips: every lane of a call runs the same count, so there
//                                is no device-side cursor and no refill; a lane whose status is not OK idles to the end
// Per-lane state indexed by link at run time -- theta, sin / cos of alpha, a, d (5 x 8), J (6 x 8) and for lm the lower triangle
// of M (36) -- is lane-striped LDS: element k of lane l at [k * 64 + l], conflict-free 8-byte accesses, 44 KB (newton, forward)
// or 62 KB (lm) per wave.  One wave per block.  V of the Jacobi sweeps (6 x 6) is indexed by constants after unrolling and
// lives in registers.
#pragma once
#include "rpp_armdh.h"

namespace rppdh {

constexpr int WAVE = 64;

struct Rec {   // per query
  int32_t status;
  int32_t n_cut;       // solve, newton
  double kappa_max;    // solve, newton
  double v[16];        // forward: pos 3, rot2euler2 3, rot2euler 3, rot2quat 4, quat2rpy 3; solve: pose 6, pose_error 6
};

struct Args {
  int64_t n;                 // queries
  const int64_t* arm_off;    // [n_arms + 1] in links
  const double* dh;          // [links][4] theta alpha a d
  const int32_t* arm;        // [n] or nullptr: arm 0
  const int64_t* ang_off;    // [n + 1] into ang_in / ang_out, in links
  const double* ang_in;      // nullptr: the arms' own column 0
  const double* ref;         // solve: [n][6]
  double* ang_out;           // solve
  double* tf;                // forward: [links of all queries][16]
  double* jac;               // forward: per query (6, N) row-major at 6 * ang_off[q]
  Rec* rec;                  // [n]
  int32_t iter_cnt;
  double step_div, eps;
};

// the lane's arm and angles into its LDS columns; returns N
__device__ inline int load_query(const Args& a, int64_t q, const rpp::DhVec& s) {
  const int64_t l0 = a.arm_off[a.arm ? a.arm[q] : 0];
  const int64_t a0 = a.ang_off[q];
  const int n = (int)(a.ang_off[q + 1] - a0);   // 1 .. 8, the arm's link count (host)
  rpp::dh_load_arm(s, n, a.dh + 4 * l0);
  if (a.ang_in)
    for (int k = 0; k < n; k++) s[rpp::kDhTh + k] = a.ang_in[a0 + k];
  return n;
}

__global__ __launch_bounds__(WAVE) void armdh_forward_kernel(Args a) {
  __shared__ double lds[rpp::kDhLaneDoublesNewton * WAVE];
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * WAVE + lane;
  if (q >= a.n) return;
  const rpp::DhVec s{&lds[lane], WAVE};
  const int n = load_query(a, q, s);
  const int64_t a0 = a.ang_off[q];
  Rec r;
  r.n_cut = 0;
  r.kappa_max = 0.0;
  for (int i = 0; i < 16; i++) r.v[i] = 0.0;
  double T[4][4];
  if (rpp::dh_forward<true>(s, n, T, a.tf + 16 * a0)) {
    r.status = rpp::kDhOk;
    r.v[0] = T[0][3], r.v[1] = T[1][3], r.v[2] = T[2][3];
    rpp::dh_rot2euler2(T, r.v[3], r.v[4], r.v[5]);
    rpp::dh_rot2euler(T, &r.v[6]);
    rpp::dh_rot2quat(T, &r.v[9]);
    rpp::dh_quat2rpy(&r.v[9], &r.v[13]);
    for (int row = 0; row < 6; row++)
      for (int k = 0; k < n; k++) a.jac[6 * a0 + row * n + k] = s[rpp::kDhJ + row * 8 + k];
  } else {   // a theta outside the domain of sin / cos: the transforms written so far are cleared, like the Jacobian
    r.status = rpp::kDhNonfinite;
    for (int i = 0; i < 16 * n; i++) a.tf[16 * a0 + i] = 0.0;
    for (int i = 0; i < 6 * n; i++) a.jac[6 * a0 + i] = 0.0;
  }
  a.rec[q] = r;
}

template <int METHOD>
__global__ __launch_bounds__(WAVE) void armdh_solve_kernel(Args a) {
  __shared__ double lds[(METHOD == rpp::kDhLm ? rpp::kDhLaneDoublesLm : rpp::kDhLaneDoublesNewton) * WAVE];
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * WAVE + lane;
  if (q >= a.n) return;
  const rpp::DhVec s{&lds[lane], WAVE};
  const int n = load_query(a, q, s);
  double ref[6];
#pragma unroll
  for (int i = 0; i < 6; i++) ref[i] = a.ref[6 * q + i];
  Rec r;
  for (int i = 12; i < 16; i++) r.v[i] = 0.0;
  rpp::DhStats st;
  r.status = rpp::dh_solve<METHOD>(s, n, ref, a.iter_cnt, a.step_div, a.eps, st, &r.v[0], &r.v[6]);
  r.n_cut = st.n_cut;
  r.kappa_max = st.kappa_max;
  const int64_t a0 = a.ang_off[q];
  for (int k = 0; k < n; k++) a.ang_out[a0 + k] = s[rpp::kDhTh + k];
  a.rec[q] = r;
}

}  // namespace rppdh

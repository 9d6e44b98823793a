// armik_batch.hip.h -- batched inverse kinematics of planar arms (gfx950): for many (arm, start angles, goal) queries what
// inverse_kinematics of 00_simple_2d_inverse_kinematics_01.py returns, and for many (arm, start angles, goal angles, goal)
// queries the driver's P-control loop.  Scalar pieces: csrc/rpp_armik.h.
//
//   armik_solve_kernel        one query per lane, persistent waves over a device-side cursor.  The iteration counts of a batch
//                             spread from 0 to the cap, so a lane that finishes writes its record and, at the next trip
//                             boundary, takes the next query with an atomicAdd on the cursor; the wave leaves when the cursor is
//                             spent and all its lanes are done.  Two nested bounded loops: a refill round ends as soon as one
//                             lane finished (at most max_iterations trips: every working lane finishes within that many), and
//                             every round but the last finishes at least one query (at most n + 1 rounds).
//   armik_move_kernel<STORE>  one query per lane, at most max_steps steps.  STORE = false counts the steps and writes the final
//                             record; STORE = true also writes the angles and the distance after every step at the offsets the
//                             host summed from those counts.
// Per-lane state -- angles, lengths and the two rows of J (solve) or the goal angles (move), up to 16 doubles each, indexed by
// link at run time -- is lane-striped LDS: element k of lane l at [k * 64 + l], 8 KB per array per wave, conflict-free 8-byte
// accesses.  One wave per block.
#pragma once
#include "rpp_armik.h"

namespace rppik {

constexpr int WAVE = 64;
constexpr int MAX_LINKS = rpp::kIkMaxLinks;

struct Rec {   // per query
  int32_t status;
  int32_t count;      // solve: iterations; move: steps
  double x, y;        // the last current_pos / end effector
  double dist;
};

struct Args {
  int64_t n;                   // queries
  const int64_t* arm_off;      // [n_arms + 1] into len
  const double* len;
  const int32_t* arm;          // [n] or nullptr: arm 0
  const int64_t* ang_off;      // [n + 1] into ang_in / ang_out (and goal_ang)
  const double* ang_in;
  const double* goal_ang;      // move
  const double* goal;          // [n][2]
  double* ang_out;
  Rec* rec;                    // [n]
  unsigned long long* cursor;  // solve: the next query to hand out
  double goal_dist;
  int32_t max_count;           // max_iterations / max_steps
  double Kp, dt;               // move
  const int64_t* step_off;     // move<true>: [n + 1] steps before query q
  const int64_t* tang_off;     // move<true>: [n + 1] trajectory angles before query q
  double* traj_ang;
  double* traj_dist;
};

// the lane's arm and angles into its LDS columns; returns N
__device__ inline int load_query(const Args& a, int64_t q, const rpp::IkVec& ang, const rpp::IkVec& len) {
  const int64_t l0 = a.arm_off[a.arm ? a.arm[q] : 0];
  const int64_t a0 = a.ang_off[q];
  const int n = (int)(a.ang_off[q + 1] - a0);   // 1 .. 16, the arm's link count (host)
  for (int k = 0; k < n; k++) {
    ang[k] = a.ang_in[a0 + k];
    len[k] = a.len[l0 + k];
  }
  return n;
}

__device__ inline void store_query(const Args& a, int64_t q, const rpp::IkVec& ang, int n, int status, int count,
                                   const rpp::IkPose& p) {
  const int64_t a0 = a.ang_off[q];
  for (int k = 0; k < n; k++) a.ang_out[a0 + k] = ang[k];
  Rec r;
  r.status = status;
  r.count = count;
  r.x = p.x;
  r.y = p.y;
  r.dist = p.dist;
  a.rec[q] = r;
}

__global__ __launch_bounds__(WAVE) void armik_solve_kernel(Args a) {
  __shared__ double s[4][MAX_LINKS * WAVE];
  const int lane = threadIdx.x;
  const rpp::IkVec ang{&s[0][lane], WAVE}, len{&s[1][lane], WAVE}, j0{&s[2][lane], WAVE}, j1{&s[3][lane], WAVE};
  const int max_it = a.max_count;
  int64_t q = -1;        // the lane's query; -1: none
  bool spent = false;    // the cursor ran out when this lane last asked
  int n = 0, it = 0;
  rpp::IkPose p;
  p.x = p.y = p.ex = p.ey = p.dist = 0.0;

  for (int64_t round = 0; round <= a.n; round++) {
    if (q < 0 && !spent) {
      const int64_t t = (int64_t)atomicAdd(a.cursor, 1ULL);
      if (t < a.n) {
        q = t;
        n = load_query(a, q, ang, len);
        it = 0;
        p.x = p.y = p.ex = p.ey = p.dist = 0.0;
      } else {
        spent = true;
      }
    }
    if (!__any(q >= 0)) break;
    for (int trip = 0; trip < max_it; trip++) {
      bool finished = false;
      if (q >= 0) {
        const int r = rpp::ik_trip(ang, len, j0, j1, n, a.goal[2 * q], a.goal[2 * q + 1], a.goal_dist, p);
        int status = rpp::kIkGoOn;
        if (r == rpp::kIkFound) {
          status = rpp::kIkFound;
        } else if (r == rpp::kIkNonfinite) {
          status = rpp::kIkNonfinite;
          it = max_it;
        } else if (++it >= max_it) {
          status = rpp::kIkNotFound;
        }
        if (status != rpp::kIkGoOn) {
          store_query(a, q, ang, n, status, it, p);
          q = -1;
          finished = true;
        }
      }
      if (__any(finished)) break;
    }
  }
}

template <bool STORE>
__global__ __launch_bounds__(WAVE) void armik_move_kernel(Args a) {
  __shared__ double s[3][MAX_LINKS * WAVE];
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * WAVE + lane;
  if (q >= a.n) return;
  const rpp::IkVec ang{&s[0][lane], WAVE}, len{&s[1][lane], WAVE}, gang{&s[2][lane], WAVE};
  const int n = load_query(a, q, ang, len);
  const int64_t a0 = a.ang_off[q];
  for (int k = 0; k < n; k++) gang[k] = a.goal_ang[a0 + k];
  const double gx = a.goal[2 * q], gy = a.goal[2 * q + 1];
  rpp::IkPose p;
  p.x = p.y = p.ex = p.ey = p.dist = 0.0;
  bool domain = rpp::ik_forward<false>(ang, len, n, gx, gy, ang, ang, p);   // the inputs the host admits start inside the domain
  // STORE: the rows of this query, as many as the counting pass reported (the host summed them)
  const int64_t s0 = STORE ? a.step_off[q] : 0, t0 = STORE ? a.tang_off[q] : 0;
  const int room = STORE ? (int)(a.step_off[q + 1] - s0) : 0;
  int steps = 0;
  int status = rpp::kIkFound;
  for (int k = 0; k < a.max_count; k++) {
    if (!domain || !(p.dist > a.goal_dist)) break;
    domain = rpp::ik_move_step(ang, len, gang, n, gx, gy, a.Kp, a.dt, p);
    if (STORE && steps < room) {
      for (int i = 0; i < n; i++) a.traj_ang[t0 + (int64_t)steps * n + i] = ang[i];
      a.traj_dist[s0 + steps] = p.dist;
    }
    steps++;
  }
  if (p.dist > a.goal_dist) status = rpp::kIkStepCap;
  if (!domain) status = rpp::kIkNonfinite;
  store_query(a, q, ang, n, status, steps, p);
}

}  // namespace rppik

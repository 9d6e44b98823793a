// rrtx_api_armik.inc -- rrtx_armik_*: batched Jacobian inverse kinematics of planar arms and the driver's P-control loop
// (armik_batch.hip.h: armik_solve_kernel, armik_move_kernel); included by rrtx_api.hip
struct rrtx_armik : DevObj {
  // device buffers, grown on demand
  DevBuf arm_off, len, arm, ang_off, ang_in, goal_ang, goal, ang_out, rec, cursor, step_off, tang_off, traj_ang, traj_dist;
  // the last run
  int kind = 0;   // 0 none, 1 solve, 2 move
  bool has_traj = false;
  int64_t n = 0, n_angles = 0, n_steps = 0, n_tang = 0;
  int32_t waves = 0;
  double kernel_ms = 0.0;
  std::vector<rppik::Rec> h_rec;
  std::vector<int64_t> h_ang_off, h_step_off, h_tang_off;
};

static_assert(rpp::kIkMaxLinks == RRTX_ARMIK_MAX_LINKS, "the link limit of the header is the kernel's");
static_assert(rpp::kIkFound == RRTX_ARMIK_FOUND && rpp::kIkNotFound == RRTX_ARMIK_NOT_FOUND &&
                  rpp::kIkNonfinite == RRTX_ARMIK_NONFINITE && rpp::kIkStepCap == RRTX_ARMIK_STEP_CAP,
              "the statuses of the header are the kernel's");

static bool armik_all_within(const double* v, int64_t count, double bound) {
  for (int64_t i = 0; i < count; i++)
    if (!std::isfinite(v[i]) || std::fabs(v[i]) > bound) return false;
  return true;
}

// The checks both runs share; fills h_ang_off.  nullptr when the batch is legal
static const char* armik_batch_msg(rrtx_armik* a, const rrtx_armik_batch* b, bool move) {
  if (!b) return "the batch is NULL";
  if (b->n_arms < 1 || b->n_arms > RRTX_ARMIK_MAX_QUERIES) return "n_arms is below 1 or above 2^20";
  if (!b->link_off || !b->link_len) return "link_off or link_len is NULL";
  if (!csr_ok(b->link_off, b->n_arms)) return "link_off does not start at 0 or decreases";
  for (int64_t s = 0; s < b->n_arms; s++) {
    const int64_t nl = b->link_off[s + 1] - b->link_off[s];
    if (nl < 1 || nl > RRTX_ARMIK_MAX_LINKS) return "an arm with fewer than 1 or more than 16 links";
  }
  if (!armik_all_within(b->link_len, b->link_off[b->n_arms], 1.0e6)) return "a link length is not finite or above 1e6 in magnitude";
  if (b->n < 0 || b->n > RRTX_ARMIK_MAX_QUERIES) return "n is negative or above 2^20";
  if (!(b->goal_dist > 0.0) || !std::isfinite(b->goal_dist)) return "goal_dist is not a finite number above 0";
  if (b->n > 0 && (!b->angles || !b->goals)) return "angles or goals is NULL";
  if (b->n > 0 && move && !b->goal_angles) return "goal_angles is NULL";
  a->h_ang_off.assign((size_t)b->n + 1, 0);
  for (int64_t q = 0; q < b->n; q++) {
    const int64_t s = b->arm ? b->arm[q] : 0;
    if (s < 0 || s >= b->n_arms) return "an arm index outside the arms";
    a->h_ang_off[(size_t)q + 1] = a->h_ang_off[(size_t)q] + (b->link_off[s + 1] - b->link_off[s]);
  }
  const int64_t NA = a->h_ang_off[(size_t)b->n];
  if (!armik_all_within(b->angles, NA, 1.0e6)) return "a joint angle is not finite or above 1e6 in magnitude";
  if (move && !armik_all_within(b->goal_angles, NA, 1.0e6)) return "a goal angle is not finite or above 1e6 in magnitude";
  if (!armik_all_within(b->goals, 2 * b->n, 1.0e6)) return "a goal coordinate is not finite or above 1e6 in magnitude";
  return nullptr;
}

// uploads what both runs read and fills the kernel's arguments
static int armik_stage(rrtx_armik* a, const rrtx_armik_batch* b, bool move, rppik::Args& k) {
  int rc;
  const size_t N = (size_t)b->n, NA = (size_t)a->h_ang_off[N];
  if ((rc = a->upload(a->arm_off, b->link_off, sizeof(int64_t) * ((size_t)b->n_arms + 1)))) return rc;
  if ((rc = a->upload(a->len, b->link_len, sizeof(double) * (size_t)b->link_off[b->n_arms]))) return rc;
  if (b->arm && (rc = a->upload(a->arm, b->arm, sizeof(int32_t) * N))) return rc;
  if ((rc = a->upload(a->ang_off, a->h_ang_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
  if ((rc = a->upload(a->ang_in, b->angles, sizeof(double) * NA))) return rc;
  if (move && (rc = a->upload(a->goal_ang, b->goal_angles, sizeof(double) * NA))) return rc;
  if ((rc = a->upload(a->goal, b->goals, sizeof(double) * 2 * N))) return rc;
  if ((rc = a->reserve(a->ang_out, sizeof(double) * NA))) return rc;
  if ((rc = a->reserve(a->rec, sizeof(rppik::Rec) * N))) return rc;
  memset(&k, 0, sizeof(k));
  k.n = b->n;
  k.arm_off = a->arm_off.as<const int64_t>();
  k.len = a->len.as<const double>();
  k.arm = b->arm ? a->arm.as<const int32_t>() : nullptr;
  k.ang_off = a->ang_off.as<const int64_t>();
  k.ang_in = a->ang_in.as<const double>();
  k.goal_ang = move ? a->goal_ang.as<const double>() : nullptr;
  k.goal = a->goal.as<const double>();
  k.ang_out = a->ang_out.as<double>();
  k.rec = a->rec.as<rppik::Rec>();
  k.goal_dist = b->goal_dist;
  return RRTX_OK;
}

static void armik_begin(rrtx_armik* a, int64_t n) {
  a->kind = 0;
  a->has_traj = false;
  a->n = n;
  a->n_angles = a->h_ang_off[(size_t)n];
  a->n_steps = a->n_tang = 0;
  a->waves = 0;
  a->kernel_ms = 0.0;
  a->h_rec.assign((size_t)n, rppik::Rec());
}

static int armik_partial(rrtx_armik* a, const char* fn, const char* what) {
  for (const rppik::Rec& r : a->h_rec)
    if (r.status != RRTX_ARMIK_FOUND) {
      a->err = std::string(fn) + what;
      return RRTX_PARTIAL;
    }
  return RRTX_OK;
}

static int armik_solve(rrtx_armik* a, const rrtx_armik_batch* b, int32_t max_iterations, int32_t waves) {
  const char* fn = "rrtx_armik_solve: ";
  auto bad = [&](const char* m) { return fail(a, RRTX_E_INVALID, std::string(fn) + m); };
  if (!a) return bad("the inverse kinematics object is NULL");
  if (const char* m = armik_batch_msg(a, b, false)) return bad(m);
  if (max_iterations < 1 || max_iterations > RRTX_ARMIK_MAX_ITERATIONS) return bad("max_iterations is outside 1..1e6");
  if (waves < 0 || waves > RRTX_ARMIK_MAX_WAVES) return bad("waves is below 1 or above 2^16");
  if (int nd = a->need_device(fn)) return nd;

  armik_begin(a, b->n);
  if (b->n == 0) {
    a->kind = 1;
    return RRTX_OK;
  }
  HIPCHK(a, hipSetDevice(a->device));
  rppik::Args k;
  int rc;
  if ((rc = armik_stage(a, b, false, k))) return rc;
  if ((rc = a->reserve(a->cursor, sizeof(unsigned long long)))) return rc;
  k.cursor = a->cursor.as<unsigned long long>();
  k.max_count = max_iterations;
  // waves given: that many are launched.  The default: as many as the device holds at once (the kernel's LDS decides), never
  // more than one lane per query
  int64_t nw = waves;
  if (nw == 0) {
    int per_cu = 0;
    HIPCHK(a, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rppik::armik_solve_kernel, rppik::WAVE, 0));
    nw = std::min<int64_t>((int64_t)std::max(1, per_cu) * std::max(1, a->n_cu), (b->n + rppik::WAVE - 1) / rppik::WAVE);
  }
  a->waves = (int32_t)nw;
  const size_t N = (size_t)b->n;
  float ms = 0.f;
  HIPCHK(a, hipMemsetAsync(a->cursor.p, 0, sizeof(unsigned long long), a->stream));
  rc = a->timed(&ms, [&] { hipLaunchKernelGGL(rppik::armik_solve_kernel, dim3((unsigned)nw), dim3(rppik::WAVE), 0, a->stream, k); },
                [&]() -> int {
                  HIPCHK(a, hipMemcpyAsync(a->h_rec.data(), a->rec.p, sizeof(rppik::Rec) * N, hipMemcpyDeviceToHost, a->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  a->kernel_ms = ms;
  a->kind = 1;
  return armik_partial(a, fn, "some queries were not found or left the finite numbers (see the status column)");
}

static int armik_move(rrtx_armik* a, const rrtx_armik_batch* b, double Kp, double dt, int32_t max_steps, int32_t want_arrays) {
  const char* fn = "rrtx_armik_move: ";
  auto bad = [&](const char* m) { return fail(a, RRTX_E_INVALID, std::string(fn) + m); };
  if (!a) return bad("the inverse kinematics object is NULL");
  if (const char* m = armik_batch_msg(a, b, true)) return bad(m);
  if (max_steps < 1 || max_steps > RRTX_ARMIK_MAX_STEPS) return bad("max_steps is outside 1..1e7");
  if (!std::isfinite(Kp) || !std::isfinite(dt)) return bad("Kp or dt is not finite");
  if (int nd = a->need_device(fn)) return nd;

  armik_begin(a, b->n);
  a->h_step_off.assign((size_t)b->n + 1, 0);
  a->h_tang_off.assign((size_t)b->n + 1, 0);
  if (b->n == 0) {
    a->has_traj = want_arrays != 0;
    a->kind = 2;
    return RRTX_OK;
  }
  HIPCHK(a, hipSetDevice(a->device));
  rppik::Args k;
  int rc;
  if ((rc = armik_stage(a, b, true, k))) return rc;
  k.max_count = max_steps;
  k.Kp = Kp;
  k.dt = dt;
  const size_t N = (size_t)b->n;
  const unsigned blocks = (unsigned)((b->n + rppik::WAVE - 1) / rppik::WAVE);
  a->waves = (int32_t)blocks;
  auto records = [&]() -> int {
    HIPCHK(a, hipMemcpyAsync(a->h_rec.data(), a->rec.p, sizeof(rppik::Rec) * N, hipMemcpyDeviceToHost, a->stream));
    return RRTX_OK;
  };
  float ms = 0.f;
  // counts first
  rc = a->timed(&ms, [&] { hipLaunchKernelGGL(rppik::armik_move_kernel<false>, dim3(blocks), dim3(rppik::WAVE), 0, a->stream, k); }, records);
  if (rc) return rc;
  a->kernel_ms = ms;
  if (want_arrays) {
    for (size_t q = 0; q < N; q++) {
      const int64_t steps = a->h_rec[q].count, nl = a->h_ang_off[q + 1] - a->h_ang_off[q];
      a->h_step_off[q + 1] = a->h_step_off[q] + steps;
      a->h_tang_off[q + 1] = a->h_tang_off[q] + steps * nl;
    }
    a->n_steps = a->h_step_off[N];
    a->n_tang = a->h_tang_off[N];
    if (a->n_steps + a->n_tang > RRTX_ARMIK_MAX_TRAJECTORY)
      return fail(a, RRTX_E_CAPACITY, std::string(fn) + "the trajectories hold more than 2^28 doubles: run with want_arrays = 0 or fewer queries");
    if (a->n_steps > 0) {
      // then the fill, at the offsets the counts give
      if ((rc = a->upload(a->step_off, a->h_step_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
      if ((rc = a->upload(a->tang_off, a->h_tang_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
      if ((rc = a->reserve(a->traj_ang, sizeof(double) * (size_t)a->n_tang))) return rc;
      if ((rc = a->reserve(a->traj_dist, sizeof(double) * (size_t)a->n_steps))) return rc;
      k.step_off = a->step_off.as<const int64_t>();
      k.tang_off = a->tang_off.as<const int64_t>();
      k.traj_ang = a->traj_ang.as<double>();
      k.traj_dist = a->traj_dist.as<double>();
      std::vector<rppik::Rec> first = a->h_rec;
      rc = a->timed(&ms, [&] { hipLaunchKernelGGL(rppik::armik_move_kernel<true>, dim3(blocks), dim3(rppik::WAVE), 0, a->stream, k); }, records);
      if (rc) return rc;
      a->kernel_ms += ms;
      for (size_t q = 0; q < N; q++)
        if (first[q].count != a->h_rec[q].count) return fail(a, RRTX_E_HIP, std::string(fn) + "the fill took other step counts than the counting pass");
    }
    a->has_traj = true;
  }
  a->kind = 2;
  return armik_partial(a, fn, "some queries reached max_steps or left the domain of sin / cos (see the status column)");
}

extern "C" {

int rrtx_armik_create(int32_t device, rrtx_armik** out) { return create_object(device, out, "rrtx_armik_create"); }
void rrtx_armik_destroy(rrtx_armik* a) { destroy_object(a); }
const char* rrtx_armik_last_error(rrtx_armik* a) { return last_error_of(a); }

int rrtx_armik_solve(rrtx_armik* a, const rrtx_armik_batch* b, int32_t max_iterations, int32_t waves) {
  const int rc = guarded(a, "rrtx_armik_solve", [&] { return armik_solve(a, b, max_iterations, waves); });
  if (rc < 0 && a) a->kind = 0;
  return rc;
}

int rrtx_armik_move(rrtx_armik* a, const rrtx_armik_batch* b, double Kp, double dt, int32_t max_steps, int32_t want_arrays) {
  const int rc = guarded(a, "rrtx_armik_move", [&] { return armik_move(a, b, Kp, dt, max_steps, want_arrays); });
  if (rc < 0 && a) a->kind = 0;
  return rc;
}

int rrtx_armik_get_records(rrtx_armik* a, int32_t* status, int32_t* count, double* end_xy, double* distance, int64_t* n_queries,
                           int64_t* n_angles) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armik_get_records: the inverse kinematics object is NULL");
  if (!a->kind) return fail(a, RRTX_E_STATE, "rrtx_armik_get_records: no completed run");
  for (int64_t q = 0; q < a->n; q++) {
    const rppik::Rec& r = a->h_rec[(size_t)q];
    if (status) status[q] = r.status;
    if (count) count[q] = r.count;
    if (end_xy) end_xy[2 * q] = r.x, end_xy[2 * q + 1] = r.y;
    if (distance) distance[q] = r.dist;
  }
  if (n_queries) *n_queries = a->n;
  if (n_angles) *n_angles = a->n_angles;
  return RRTX_OK;
}

int rrtx_armik_get_angles(rrtx_armik* a, int64_t* offsets, double* angles, int64_t cap) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armik_get_angles: the inverse kinematics object is NULL");
  if (!a->kind) return fail(a, RRTX_E_STATE, "rrtx_armik_get_angles: no completed run");
  if (offsets) memcpy(offsets, a->h_ang_off.data(), sizeof(int64_t) * ((size_t)a->n + 1));
  if (angles && a->n_angles > 0) {
    if (cap < a->n_angles) return fail(a, RRTX_E_CAPACITY, "rrtx_armik_get_angles: the buffer is too small");
    return a->fetch(angles, a->ang_out.p, sizeof(double) * (size_t)a->n_angles);
  }
  return RRTX_OK;
}

int rrtx_armik_get_trajectory(rrtx_armik* a, int64_t* step_offsets, int64_t* angle_offsets, double* angles, double* distance,
                              int64_t cap_steps, int64_t cap_angles) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armik_get_trajectory: the inverse kinematics object is NULL");
  if (a->kind != 2) return fail(a, RRTX_E_STATE, "rrtx_armik_get_trajectory: no completed move");
  if (!a->has_traj) return fail(a, RRTX_E_STATE, "rrtx_armik_get_trajectory: the last move was run with want_arrays = 0");
  if (step_offsets) memcpy(step_offsets, a->h_step_off.data(), sizeof(int64_t) * ((size_t)a->n + 1));
  if (angle_offsets) memcpy(angle_offsets, a->h_tang_off.data(), sizeof(int64_t) * ((size_t)a->n + 1));
  if ((angles && cap_angles < a->n_tang) || (distance && cap_steps < a->n_steps))
    return fail(a, RRTX_E_CAPACITY, "rrtx_armik_get_trajectory: a buffer is too small");
  if (a->n_steps > 0) {
    int rc;
    if (angles && (rc = a->fetch(angles, a->traj_ang.p, sizeof(double) * (size_t)a->n_tang))) return rc;
    if (distance && (rc = a->fetch(distance, a->traj_dist.p, sizeof(double) * (size_t)a->n_steps))) return rc;
  }
  return RRTX_OK;
}

int rrtx_armik_get_kernel_ms(rrtx_armik* a, double* kernel_ms, int32_t* waves) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armik_get_kernel_ms: the inverse kinematics object is NULL");
  if (kernel_ms) *kernel_ms = a->kernel_ms;
  if (waves) *waves = a->waves;
  return RRTX_OK;
}

}  // extern "C"

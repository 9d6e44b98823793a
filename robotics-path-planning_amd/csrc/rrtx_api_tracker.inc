// rrtx_api_tracker.inc -- rrtx_tracker_*: batched closed-loop tracking of courses given as data (rrt_track.hip.h,
// track_courses_kernel); included by rrtx_api.hip
struct rrtx_tracker : DevObj {
  // device buffers, grown on demand
  DevBuf off, x, y, yaw, per_course, start, ox, oy, othr, obs_off, rec, counter, slab, out, arr_off;
  // the last run
  bool ran = false, has_arrays = false;
  int64_t n = 0, n_steps = 0;
  double kernel_ms = 0.0;
  std::vector<rppt::Record> h_rec;
  std::vector<int64_t> h_arr_off;
};

extern "C" {

int rrtx_tracker_create(int32_t device, rrtx_tracker** out) {
  if (!out) return fail<rrtx_tracker>(nullptr, RRTX_E_INVALID, "rrtx_tracker_create: out is NULL");
  *out = nullptr;
  if (device < 0) return fail<rrtx_tracker>(nullptr, RRTX_E_INVALID, "rrtx_tracker_create: negative device ordinal");
  rrtx_tracker* t = new (std::nothrow) rrtx_tracker();
  if (!t) return fail<rrtx_tracker>(nullptr, RRTX_E_HIP, "rrtx_tracker_create: out of host memory");
  *out = t;   // returned on failure too: the caller reads the message, and runs still check their arguments
  return t->open(device, "rrtx_tracker_create");
}

void rrtx_tracker_destroy(rrtx_tracker* t) {
  if (!t) return;
  if (t->usable) hipSetDevice(t->device);
  delete t;   // the buffers, then the events and the stream
}

const char* rrtx_tracker_last_error(rrtx_tracker* t) { return t ? t->err.c_str() : null_object_err.c_str(); }

static int tracker_run(rrtx_tracker* t, const rrtx_track_params* tp, const rrtx_track_batch* b) {
  const char* fn = "rrtx_tracker_run: ";
  auto bad = [&](const char* m) { return fail(t, RRTX_E_INVALID, std::string(fn) + m); };
  if (!t) return bad("the tracker is NULL");
  if (!tp || !b) return bad("the parameters or the batch is NULL");
  if (b->n < 0 || b->n > (1LL << 30)) return bad("n is negative or above 2^30");
  if (!b->offsets || !b->robot_radius) return bad("offsets or robot_radius is NULL");
  const int64_t n = b->n;
  if (!csr_ok(b->offsets, n)) return bad("offsets do not start at 0 or decrease");
  const int64_t pts = b->offsets[n];
  if (pts > 0x7fffffffLL) return bad("more than 2^31 - 1 points in all");
  if (pts > 0 && (!b->x || !b->y || !b->yaw)) return bad("x, y or yaw is NULL");
  if (b->n_obstacles < 0) return bad("n_obstacles is negative");
  if (b->n_obstacles > 0 && !b->obstacles) return bad("obstacles is NULL");
  if (b->obs_offsets) {
    if (!csr_ok(b->obs_offsets, n)) return bad("obs_offsets do not start at 0 or decrease");
    if (b->obs_offsets[n] > b->n_obstacles) return bad("obs_offsets end beyond n_obstacles");
    for (int64_t i = 0; i < n; i++)
      if (b->obs_offsets[i + 1] - b->obs_offsets[i] > rppt::TPB) return bad("more than 64 obstacles in one list");
  } else if (b->n_obstacles > rppt::TPB) {
    return bad("more than 64 obstacles in one list");
  }
  if (!track_params_ok(tp)) return bad(TRACK_PARAMS_MSG);
  const int64_t n_rr = b->robot_radius_per_course ? n : 1;
  if (!all_finite(b->x, pts) || !all_finite(b->y, pts) || !all_finite(b->yaw, pts)) return bad("a pose component is not finite");
  if (!all_finite(b->obstacles, 3 * b->n_obstacles)) return bad("an obstacle component is not finite");
  if (!all_finite(b->robot_radius, n_rr)) return bad("a robot radius is not finite");
  if (b->start_state && !all_finite(b->start_state, 4 * n)) return bad("a start state component is not finite");
  if (b->per_course && !all_finite(b->per_course, 3 * n)) return bad("a per-course value is not finite");
  if (!all_finite(&tp->target_speed, sizeof(*tp) / sizeof(double))) return bad("a parameter is not finite");
  if (!t->usable) return fail(t, RRTX_E_NO_DEVICE, std::string(fn) + "no usable gfx950 device (there is no CPU fallback)");

  t->ran = false;
  t->has_arrays = false;
  t->n = n;
  t->n_steps = 0;
  t->kernel_ms = 0.0;
  t->h_rec.clear();
  t->h_arr_off.assign((size_t)n + 1, 0);
  if (n == 0) {
    t->has_arrays = b->want_arrays != 0;
    t->ran = true;
    return RRTX_OK;
  }
  // obstacle table: SoA x, y and the thresholds (radius + robot_radius) ** 2 by the planners' routine; one threshold row per
  // obstacle row, or with one shared list and a radius per course n rows of the list's thresholds
  const int64_t rows = b->obs_offsets ? b->obs_offsets[n] : b->n_obstacles;
  const bool thr_per_course = !b->obs_offsets && b->robot_radius_per_course && rows > 0;
  std::vector<double> ox((size_t)rows), oy((size_t)rows), othr((size_t)(thr_per_course ? rows * n : rows));
  for (int64_t k = 0; k < rows; k++) {
    ox[k] = b->obstacles[3 * k];
    oy[k] = b->obstacles[3 * k + 1];
  }
  if (b->obs_offsets) {
    for (int64_t i = 0; i < n; i++)
      for (int64_t k = b->obs_offsets[i]; k < b->obs_offsets[i + 1]; k++)
        othr[k] = py_sq_host(b->obstacles[3 * k + 2] + b->robot_radius[b->robot_radius_per_course ? i : 0]);
  } else if (thr_per_course) {
    for (int64_t i = 0; i < n; i++)
      for (int64_t k = 0; k < rows; k++) othr[i * rows + k] = py_sq_host(b->obstacles[3 * k + 2] + b->robot_radius[i]);
  } else {
    for (int64_t k = 0; k < rows; k++) othr[k] = py_sq_host(b->obstacles[3 * k + 2] + b->robot_radius[0]);
  }

  HIPCHK(t, hipSetDevice(t->device));
  int rc;
  const size_t N = (size_t)n;
  const int64_t want = (int64_t)t->n_cu * 16;   // 16 blocks of one wave per CU, as track_roll_kernel
  int blocks = (int)(n < want ? n : want);
  if (blocks < 1) blocks = 1;
  if ((rc = t->upload(t->off, b->offsets, sizeof(int64_t) * (N + 1)))) return rc;
  if ((rc = t->upload(t->x, b->x, sizeof(double) * (size_t)pts))) return rc;
  if ((rc = t->upload(t->y, b->y, sizeof(double) * (size_t)pts))) return rc;
  if ((rc = t->upload(t->yaw, b->yaw, sizeof(double) * (size_t)pts))) return rc;
  if (b->per_course && (rc = t->upload(t->per_course, b->per_course, sizeof(double) * 3 * N))) return rc;
  if (b->start_state && (rc = t->upload(t->start, b->start_state, sizeof(double) * 4 * N))) return rc;
  if ((rc = t->upload(t->ox, ox.data(), sizeof(double) * ox.size()))) return rc;
  if ((rc = t->upload(t->oy, oy.data(), sizeof(double) * oy.size()))) return rc;
  if ((rc = t->upload(t->othr, othr.data(), sizeof(double) * othr.size()))) return rc;
  if (b->obs_offsets && (rc = t->upload(t->obs_off, b->obs_offsets, sizeof(int64_t) * (N + 1)))) return rc;
  if ((rc = t->reserve(t->rec, sizeof(rppt::Record) * N))) return rc;
  if ((rc = t->reserve(t->counter, sizeof(int32_t)))) return rc;
  if ((rc = t->reserve(t->slab, sizeof(double) * (size_t)blocks * 3 * rppt::SLAB_PTS))) return rc;
  HIPCHK(t, hipMemsetAsync(t->counter.p, 0, sizeof(int32_t), t->stream));

  rppt::CourseArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.off = t->off.as<const int64_t>();
  a.x = t->x.as<const double>();
  a.y = t->y.as<const double>();
  a.yaw = t->yaw.as<const double>();
  a.per_course = b->per_course ? t->per_course.as<const double>() : nullptr;
  a.start = b->start_state ? t->start.as<const double>() : nullptr;
  a.ox = t->ox.as<const double>();
  a.oy = t->oy.as<const double>();
  a.othr = t->othr.as<const double>();
  a.obs_off = b->obs_offsets ? t->obs_off.as<const int64_t>() : nullptr;
  a.thr_stride = thr_per_course ? rows : 0;
  a.m_shared = b->obs_offsets ? 0 : (int32_t)rows;
  memcpy(&a.P, tp, sizeof(a.P));
  a.rec = t->rec.as<rppt::Record>();
  a.counter = t->counter.as<int32_t>();
  a.slab = t->slab.as<double>();

  // first launch: the records
  t->h_rec.resize(N);
  float ms = 0.f;
  rc = t->timed(&ms, [&] { hipLaunchKernelGGL(rppt::track_courses_kernel, dim3(blocks), dim3(rppt::TPB), 0, t->stream, a, 0); }, [&]() -> int {
    HIPCHK(t, hipMemcpyAsync(t->h_rec.data(), t->rec.p, sizeof(rppt::Record) * N, hipMemcpyDeviceToHost, t->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  t->kernel_ms = ms;

  // arr_offsets: exclusive sum of len over the complete courses
  int64_t tot = 0;
  bool partial = false;
  for (size_t i = 0; i < N; i++) {
    t->h_arr_off[i] = tot;
    if (t->h_rec[i].ood)
      partial = true;
    else
      tot += t->h_rec[i].n;
  }
  t->h_arr_off[N] = tot;
  t->n_steps = tot;

  if (b->want_arrays) {
    if (tot > 0) {
      if ((rc = t->reserve(t->out, sizeof(double) * 7 * (size_t)tot))) return rc;
      if ((rc = t->upload(t->arr_off, t->h_arr_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
      HIPCHK(t, hipMemsetAsync(t->counter.p, 0, sizeof(int32_t), t->stream));
      a.out = t->out.as<double>();
      a.arr_off = t->arr_off.as<const int64_t>();
      a.out_total = tot;
      rc = t->timed(&ms, [&] { hipLaunchKernelGGL(rppt::track_courses_kernel, dim3(blocks), dim3(rppt::TPB), 0, t->stream, a, 1); });
      if (rc) return rc;
      t->kernel_ms += ms;
    }
    t->has_arrays = true;
  }
  t->ran = true;
  if (partial) {
    t->err = std::string(fn) + "some courses are too short, too long or left the replica's domain (see the ood column)";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

int rrtx_tracker_run(rrtx_tracker* t, const rrtx_track_params* tp, const rrtx_track_batch* b) {
  try {   // host allocations (records, offsets, messages) must not throw across the ABI
    return tracker_run(t, tp, b);
  } catch (const std::exception& e) {
    if (t) t->ran = false;
    return fail(t, RRTX_E_HIP, std::string("rrtx_tracker_run: ") + e.what());
  }
}

int rrtx_tracker_get_counts(rrtx_tracker* t, int64_t* n_courses, int64_t* n_steps) {
  if (!t || !n_courses || !n_steps) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_counts: a NULL pointer");
  if (!t->ran) return fail(t, RRTX_E_STATE, "rrtx_tracker_get_counts: no completed run");
  *n_courses = t->n;
  *n_steps = t->n_steps;
  return RRTX_OK;
}

int rrtx_tracker_get_records(rrtx_tracker* t, rrtx_track_record* rec, int64_t* arr_offsets) {
  if (!t || !rec) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_records: a NULL pointer");
  if (!t->ran) return fail(t, RRTX_E_STATE, "rrtx_tracker_get_records: no completed run");
  if (t->n) memcpy(rec, t->h_rec.data(), sizeof(rrtx_track_record) * (size_t)t->n);
  if (arr_offsets) memcpy(arr_offsets, t->h_arr_off.data(), sizeof(int64_t) * ((size_t)t->n + 1));
  return RRTX_OK;
}

int rrtx_tracker_get_arrays(rrtx_tracker* t, double* x, double* y, double* yaw, double* v, double* tt, double* a, double* d,
                            int64_t cap) {
  if (!t) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_arrays: the tracker is NULL");
  if (!t->ran || !t->has_arrays) return fail(t, RRTX_E_STATE, "rrtx_tracker_get_arrays: no completed run with arrays");
  if (cap < t->n_steps) return fail(t, RRTX_E_CAPACITY, "rrtx_tracker_get_arrays: the buffers are too small");
  if (t->n_steps == 0) return RRTX_OK;
  const size_t tot = (size_t)t->n_steps;
  HIPCHK(t, hipSetDevice(t->device));
  double* dst[7] = {x, y, yaw, v, tt, a, d};
  for (int k = 0; k < 7; k++)
    if (dst[k]) HIPCHK(t, hipMemcpy(dst[k], t->out.as<const double>() + k * tot, sizeof(double) * tot, hipMemcpyDeviceToHost));
  return RRTX_OK;
}

int rrtx_tracker_get_kernel_ms(rrtx_tracker* t, double* kernel_ms) {
  if (!t || !kernel_ms) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_kernel_ms: a NULL pointer");
  if (!t->ran) return fail(t, RRTX_E_STATE, "rrtx_tracker_get_kernel_ms: no completed run");
  *kernel_ms = t->kernel_ms;
  return RRTX_OK;
}

}  // extern "C"

// rrtx_api_courses.inc -- rrtx_gather_courses and its getters: every course of a planned handle in one CSR result, gathered
// on the device (course_gather.hip.h); included by rrtx_api.hip after the planner handle, before the tracker that reads it.
// Per gather: two launches, one device -> host copy (the counts) and at most two host -> device copies (the offsets, the
// pose planners' slab pointers); per rrtx_get_courses one copy per column.  None of them depends on the batch size or
// on the depth of a tree.

// The planner handles alive in this process.  rrtx_tracker_run_from is handed its source as a const void*: for the other
// kinds a wrong pointer is the caller's fault alone, but a handle is the one source that a GPU-less host cannot create, so
// "is this a handle" is answered here, before anything of it is read.
static std::mutex live_handles_mu;
static std::set<const void*> live_handles;
static void handle_register(const rrtx_handle* h) {
  std::lock_guard<std::mutex> g(live_handles_mu);
  live_handles.insert(h);
}
static void handle_unregister(const rrtx_handle* h) {
  std::lock_guard<std::mutex> g(live_handles_mu);
  live_handles.erase(h);
}
static bool handle_is_live(const void* p) {
  std::lock_guard<std::mutex> g(live_handles_mu);
  return live_handles.count(p) != 0;
}

static int gather_courses(rrtx_handle* h, int32_t which, int32_t order) {
  const char* fn = "rrtx_gather_courses: ";
  if (!h) return fail(h, RRTX_E_INVALID, std::string(fn) + "the handle is NULL");
  if (which != RRTX_COURSE_PLANNED && which != RRTX_COURSE_SMOOTHED) return fail(h, RRTX_E_INVALID, std::string(fn) + "unknown which");
  if (order != RRTX_ORDER_PLANNING && order != RRTX_ORDER_DRIVING) return fail(h, RRTX_E_INVALID, std::string(fn) + "unknown order");
  if (int rc = refuse_in_plan(h, "rrtx_gather_courses")) return rc;
  if (!h->planned) return fail(h, RRTX_E_STATE, std::string(fn) + "no completed plan");
  if (which == RRTX_COURSE_SMOOTHED && !h->smoothed)
    return fail(h, RRTX_E_STATE, std::string(fn) + "rrtx_smooth_planned has not completed since the plan");
  rrtx_handle::Courses& K = h->cs;
  K.valid = false;
  HIPCHK(h, hipSetDevice(h->device));
  const int B = h->n_inst;
  const size_t N = (size_t)B;
  const int algo = h->p.algo;
  const bool pose = which == RRTX_COURSE_PLANNED && is_pose_tree(algo);
  const bool has_yaw = pose && algo == RRTX_ALGO_RS;
  int rc;
  rppc::GatherArgs a;
  memset(&a, 0, sizeof(a));
  a.n_inst = B;
  a.order = order;
  a.ncol = has_yaw ? 3 : 2;
  a.inst = h->c.inst;
  a.parent = h->c.parent;
  a.stride = h->stride;
  if (which == RRTX_COURSE_SMOOTHED) {
    a.src = rppc::SRC_FLAT;
    a.flat_xy = h->sm_xy;
    a.flat_stride = 2 * h->sm_stride;
    a.flat_n = h->sm_n;
    a.flat_n_stride = 1;
    a.flat_cap = h->sm_stride;
  } else if (pose) {
    a.src = rppc::SRC_POSE;
    a.need_path = 1;
    a.plen = h->da.plen;
    a.poff = h->da.poff;
    // where each instance's polylines live: the handle's pool, or the enlarged pool of its re-plan
    std::vector<const double*> pp(3 * N);
    std::vector<int64_t> cap(N);
    for (int i = 0; i < B; i++) {
      const rrtx_handle::PoolLoc& pl = h->pool_loc[i];
      pp[3 * (size_t)i] = pl.at(pl.px);
      pp[3 * (size_t)i + 1] = pl.at(pl.py);
      pp[3 * (size_t)i + 2] = has_yaw ? pl.at(pl.pyaw) : nullptr;
      cap[i] = pl.cap;
    }
    // one upload: the pointers, then the capacities
    std::vector<int64_t> both(4 * N);
    memcpy(both.data(), pp.data(), sizeof(double*) * 3 * N);
    memcpy(both.data() + 3 * N, cap.data(), sizeof(int64_t) * N);
    static_assert(sizeof(double*) == sizeof(int64_t), "the slab pointers and capacities share one upload");
    if ((rc = h->upload(K.pool, both.data(), sizeof(int64_t) * both.size()))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));   // `both` is a local
    a.pool = K.pool.as<const double* const>();
    a.pool_cap = K.pool.as<const int64_t>() + 3 * N;
  } else if (algo == RRTX_ALGO_BITSTAR) {
    a.src = rppc::SRC_FLAT;
    a.need_path = 1;
    a.flat_xy = h->ba.dslab + 3LL * rppb::SC + 3LL * rppb::LC + 5LL * rppb::VC + 2LL * rppb::EC;   // as rrtx_get_path
    a.flat_stride = rppb::DSLAB;
    a.flat_n = h->ba.out_i + 3;
    a.flat_n_stride = 8;
    a.flat_cap = rppb::PC;
  } else {
    a.src = rppc::SRC_FLAT;
    a.need_path = 1;
    a.flat_xy = h->c.path_xy;
    a.flat_stride = 2 * (int64_t)h->c.path_cap;
    a.flat_n = &h->c.inst[0].path_n;
    a.flat_n_stride = (int64_t)(sizeof(Inst) / sizeof(int32_t));
    a.flat_cap = h->c.path_cap;
    a.walk_trunc = 1;
    a.x = h->c.x;
    a.y = h->c.y;
  }
  if ((rc = h->reserve(K.count, sizeof(int32_t) * N))) return rc;
  a.count = K.count.as<int32_t>();

  // first launch: the counts
  std::vector<int32_t> cnt(N);
  float ms = 0.f;
  rc = h->timed(&ms, [&] { hipLaunchKernelGGL(rppc::course_count_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, a); },
                [&]() -> int {
                  HIPCHK(h, hipMemcpyAsync(cnt.data(), K.count.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, h->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  K.kernel_ms = ms;
  K.h_off.assign(N + 1, 0);
  int64_t tot = 0;
  for (size_t i = 0; i < N; i++) {
    K.h_off[i] = tot;
    tot += cnt[i];
    if (tot > (1LL << 28)) return fail(h, RRTX_E_CAPACITY, std::string(fn) + "more than 2^28 points in all");
  }
  K.h_off[N] = tot;

  // second launch: the points
  if (tot > 0) {
    if ((rc = h->upload(K.off, K.h_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
    if ((rc = h->reserve(K.x, sizeof(double) * (size_t)tot))) return rc;
    if ((rc = h->reserve(K.y, sizeof(double) * (size_t)tot))) return rc;
    if (has_yaw && (rc = h->reserve(K.yaw, sizeof(double) * (size_t)tot))) return rc;
    a.off = K.off.as<const int64_t>();
    a.ox = K.x.as<double>();
    a.oy = K.y.as<double>();
    a.oyaw = has_yaw ? K.yaw.as<double>() : nullptr;
    rc = h->timed(&ms, [&] { hipLaunchKernelGGL(rppc::course_gather_kernel, dim3(B), dim3(rppc::TPB), 0, h->stream, a); });
    if (rc) return rc;
    K.kernel_ms += ms;
  } else {
    // every course is empty: the offsets are on the device all the same (the tracker reads them there)
    if ((rc = h->reserve(K.off, sizeof(int64_t) * (N + 1)))) return rc;
    HIPCHK(h, hipMemsetAsync(K.off.p, 0, sizeof(int64_t) * (N + 1), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  K.which = which;
  K.order = order;
  K.has_yaw = has_yaw;
  K.n_points = tot;
  K.valid = true;
  K.generation++;
  return RRTX_OK;
}

// the gathered courses are those of the handle's current plan (and smoothing run)
static bool courses_current(const rrtx_handle* h) {
  return h->cs.valid && h->planned && h->run.stage == 0 && (h->cs.which != RRTX_COURSE_SMOOTHED || h->smoothed);
}

extern "C" {

int rrtx_gather_courses(rrtx_handle* h, int32_t which, int32_t order) {
  return guarded(h, "rrtx_gather_courses", [&] { return gather_courses(h, which, order); }, [&] { if (h) h->cs.valid = false; });
}

int rrtx_get_course_counts(rrtx_handle* h, int64_t* offsets, int64_t* n_points, int32_t* has_yaw, double* kernel_ms) {
  if (!h) return fail(h, RRTX_E_INVALID, "rrtx_get_course_counts: the handle is NULL");
  if (!courses_current(h)) return fail(h, RRTX_E_STATE, "rrtx_get_course_counts: no gathered courses of the current plan");
  if (offsets) memcpy(offsets, h->cs.h_off.data(), sizeof(int64_t) * h->cs.h_off.size());
  if (n_points) *n_points = h->cs.n_points;
  if (has_yaw) *has_yaw = h->cs.has_yaw ? 1 : 0;
  if (kernel_ms) *kernel_ms = h->cs.kernel_ms;
  return RRTX_OK;
}

int rrtx_get_courses(rrtx_handle* h, double* x, double* y, double* yaw, int64_t cap) {
  if (!h) return fail(h, RRTX_E_INVALID, "rrtx_get_courses: the handle is NULL");
  if (!courses_current(h)) return fail(h, RRTX_E_STATE, "rrtx_get_courses: no gathered courses of the current plan");
  if (yaw && !h->cs.has_yaw) return fail(h, RRTX_E_STATE, "rrtx_get_courses: the gathered courses have no yaw");
  if (cap < h->cs.n_points) return fail(h, RRTX_E_CAPACITY, "rrtx_get_courses: the buffers are too small");
  if (h->cs.n_points == 0) return RRTX_OK;
  const size_t bytes = sizeof(double) * (size_t)h->cs.n_points;
  int rc;
  if (x && (rc = h->fetch(x, h->cs.x.p, bytes))) return rc;
  if (y && (rc = h->fetch(y, h->cs.y.p, bytes))) return rc;
  if (yaw && (rc = h->fetch(yaw, h->cs.yaw.p, bytes))) return rc;
  return RRTX_OK;
}

int rrtx_get_course_generation(rrtx_handle* h, uint64_t* generation) {
  if (!h || !generation) return fail(h, RRTX_E_INVALID, "rrtx_get_course_generation: a NULL pointer");
  *generation = h->cs.generation;
  return RRTX_OK;
}

}  // extern "C"

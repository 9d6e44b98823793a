// rrtx_api_tracker.inc -- rrtx_tracker_*: batched closed-loop tracking of courses given as data (rrt_track.hip.h,
// track_courses_kernel) or left on the device by a producer (track_source_kernel, track_group_pick_kernel); included by
// rrtx_api.hip after the producers' files
struct rrtx_tracker : DevObj {
  // device buffers, grown on demand
  DevBuf off, x, y, yaw, per_course, start, ox, oy, othr, obs_off, rec, counter, slab, out, arr_off;
  // the last run
  bool ran = false, has_arrays = false;
  int64_t n = 0, n_steps = 0;
  double kernel_ms = 0.0;
  std::vector<rppt::Record> h_rec;
  std::vector<int64_t> h_arr_off;
  // the last run when it was rrtx_tracker_run_from
  DevBuf mask, goal, winner, wgoal;
  bool from = false;
  int64_t group = 0;
  std::vector<int32_t> h_winner;
  // the obstacle index (rrtx_tracker_set_obstacle_index): the build over the last list given in mode ON, and what served the
  // last completed run -- a refused run leaves ix_used / ix_reason, and with them the getters, as they were
  ObsIndex oi;
  int ix_used = 0, ix_reason = RRTX_OBSIDX_REASON_EMPTY;
  rrtx_tracker() { oi.mode = RRTX_OBSIDX_OFF; }
};

// Mode ON, among the argument checks (before any HIP call): what the index cannot take, or nullptr
static const char* tracker_index_refusal(const rrtx_track_batch* b) {
  if (b->obs_offsets) return "the obstacle index serves the shared list only (obs_offsets must be NULL)";
  if (b->n_obstacles > rppo::M_MAX) return "more than 2^20 obstacles in the shared list";
  if (b->robot_radius_per_course && b->n_obstacles > 0)
    return "the obstacle index holds one threshold per circle: a robot radius per course cannot go with an obstacle list";
  return nullptr;
}

// After every check of a run, before anything of the last run is touched: the index over the shared list in mode ON.
// *indexed: CHECK_INDEX serves the run.  A list of more than 64 rows that the index cannot serve is RRTX_E_INVALID.
static int tracker_index_decide(rrtx_tracker* t, const rrtx_track_batch* b, const char* fn, bool* indexed, int* reason) {
  *indexed = false;
  if (t->oi.mode != RRTX_OBSIDX_ON) {
    *reason = rppo::index_reason(rppo::IDX_OFF, b->obs_offsets ? b->obs_offsets[b->n] : b->n_obstacles, true, 0);
    return RRTX_OK;
  }
  if (int rc = obsindex_set_list(t, t->oi, b->obstacles, b->n_obstacles, b->robot_radius[0])) return rc;
  *reason = t->oi.reason;
  *indexed = t->oi.used != 0;
  if (!*indexed && b->n_obstacles > rppt::TPB)
    return fail(t, RRTX_E_INVALID,
                std::string(fn) + "the obstacle index cannot serve this list (" +
                    (*reason == RRTX_OBSIDX_REASON_RUN_TOO_LONG ? "run too long: a cell or the wide list would hold more than 4096 records"
                                                                : "a threshold or reach of a circle is not finite") +
                    ") and the lane-per-obstacle check takes at most 64 obstacles");
  return RRTX_OK;
}

// What both runs say of an obstacle list that is wrong (rrtx_host.h; the count has no limit of its own here)
static const ObsListText TRACK_OBS_TEXT = {"n_obstacles is negative", nullptr, "obstacles is NULL", "an obstacle component is not finite",
                                           "a robot radius is not finite"};

// The shape of a run's obstacle lists, among the argument checks: the list itself, then what the index takes in mode ON or
// the lane-per-obstacle check otherwise.  bad(text) records the refusal and returns its code.
template <class Bad>
static int tracker_check_obstacles(const rrtx_tracker* t, const rrtx_track_batch* b, int64_t n, Bad&& bad) {
  if (const char* m = obstacle_list_shape_error(b->obstacles, b->n_obstacles, INT64_MAX, TRACK_OBS_TEXT)) return bad(m);
  if (t->oi.mode == RRTX_OBSIDX_ON) {
    if (const char* m = tracker_index_refusal(b)) return bad(m);
  } else if (b->obs_offsets) {
    if (!csr_ok(b->obs_offsets, n)) return bad("obs_offsets do not start at 0 or decrease");
    if (b->obs_offsets[n] > b->n_obstacles) return bad("obs_offsets end beyond n_obstacles");
    for (int64_t i = 0; i < n; i++)
      if (b->obs_offsets[i + 1] - b->obs_offsets[i] > rppt::TPB) return bad("more than 64 obstacles in one list");
  } else if (b->n_obstacles > rppt::TPB) {
    return bad("more than 64 obstacles in one list");
  }
  return RRTX_OK;
}

// The obstacle table of a run, built, uploaded and entered into a: SoA x, y and the thresholds (radius + robot_radius) ** 2 by
// the planners' routine; one threshold row per obstacle row, or with one shared list and a radius per course n rows of the
// list's thresholds (the index form reads none of it: its items hold the circles)
static int tracker_obstacle_table(rrtx_tracker* t, const rrtx_track_batch* b, int64_t n, bool indexed, rppt::CourseArgs& a) {
  const int64_t rows = indexed ? 0 : b->obs_offsets ? b->obs_offsets[n] : b->n_obstacles;
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
  int rc;
  if ((rc = t->upload(t->ox, ox.data(), sizeof(double) * ox.size()))) return rc;
  if ((rc = t->upload(t->oy, oy.data(), sizeof(double) * oy.size()))) return rc;
  if ((rc = t->upload(t->othr, othr.data(), sizeof(double) * othr.size()))) return rc;
  if (b->obs_offsets && (rc = t->upload(t->obs_off, b->obs_offsets, sizeof(int64_t) * ((size_t)n + 1)))) return rc;
  a.ox = t->ox.as<const double>();
  a.oy = t->oy.as<const double>();
  a.othr = t->othr.as<const double>();
  a.obs_off = b->obs_offsets ? t->obs_off.as<const int64_t>() : nullptr;
  a.thr_stride = thr_per_course ? rows : 0;
  a.m_shared = b->obs_offsets ? 0 : (int32_t)rows;
  return RRTX_OK;
}

// What else both runs put into a besides the courses: the per-course values, the parameters, the obstacle table, and the
// records and workspace of `blocks` waves (the counter cleared)
static int tracker_common_args(rrtx_tracker* t, const rrtx_track_params* tp, const rrtx_track_batch* b, int64_t n, bool indexed,
                               int blocks, rppt::CourseArgs& a) {
  const size_t N = (size_t)n;
  int rc;
  if (b->per_course && (rc = t->upload(t->per_course, b->per_course, sizeof(double) * 3 * N))) return rc;
  if (b->start_state && (rc = t->upload(t->start, b->start_state, sizeof(double) * 4 * N))) return rc;
  if ((rc = tracker_obstacle_table(t, b, n, indexed, a))) return rc;
  if ((rc = t->reserve(t->rec, sizeof(rppt::Record) * N))) return rc;
  if ((rc = t->reserve(t->counter, sizeof(int32_t)))) return rc;
  if ((rc = t->reserve(t->slab, sizeof(double) * (size_t)blocks * 3 * rppt::SLAB_PTS))) return rc;
  HIPCHK(t, hipMemsetAsync(t->counter.p, 0, sizeof(int32_t), t->stream));
  a.n = n;
  a.per_course = b->per_course ? t->per_course.as<const double>() : nullptr;
  a.start = b->start_state ? t->start.as<const double>() : nullptr;
  memcpy(&a.P, tp, sizeof(a.P));
  a.rec = t->rec.as<rppt::Record>();
  a.counter = t->counter.as<int32_t>();
  a.slab = t->slab.as<double>();
  return RRTX_OK;
}

static_assert(rppt::SEL_ALL == RRTX_SELECT_ALL && rppt::SEL_FREE == RRTX_SELECT_FREE && rppt::SEL_MASK == RRTX_SELECT_MASK,
              "the selections of the header are the core's");

extern "C" {

int rrtx_tracker_create(int32_t device, rrtx_tracker** out) { return create_object(device, out, "rrtx_tracker_create"); }
void rrtx_tracker_destroy(rrtx_tracker* t) { destroy_object(t); }
const char* rrtx_tracker_last_error(rrtx_tracker* t) { return last_error_of(t); }

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
  if (int orc = tracker_check_obstacles(t, b, n, bad)) return orc;
  if (!track_params_ok(tp)) return bad(TRACK_PARAMS_MSG);
  const int64_t n_rr = b->robot_radius_per_course ? n : 1;
  if (!all_finite(b->x, pts) || !all_finite(b->y, pts) || !all_finite(b->yaw, pts)) return bad("a pose component is not finite");
  if (const char* m = obstacle_list_value_error(b->obstacles, b->n_obstacles, b->robot_radius, n_rr, TRACK_OBS_TEXT)) return bad(m);
  if (b->start_state && !all_finite(b->start_state, 4 * n)) return bad("a start state component is not finite");
  if (b->per_course && !all_finite(b->per_course, 3 * n)) return bad("a per-course value is not finite");
  if (!all_finite(&tp->target_speed, sizeof(*tp) / sizeof(double))) return bad("a parameter is not finite");
  if (int nd = t->need_device(fn)) return nd;
  bool indexed = false;
  int ix_reason = 0;
  if (int irc = tracker_index_decide(t, b, fn, &indexed, &ix_reason)) return irc;

  t->ran = false;
  t->has_arrays = false;
  t->ix_used = indexed;
  t->ix_reason = ix_reason;
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

  rppt::CourseArgs a;
  memset(&a, 0, sizeof(a));
  if ((rc = tracker_common_args(t, tp, b, n, indexed, blocks, a))) return rc;
  a.off = t->off.as<const int64_t>();
  a.x = t->x.as<const double>();
  a.y = t->y.as<const double>();
  a.yaw = t->yaw.as<const double>();

  // first launch: the records
  t->h_rec.resize(N);
  float ms = 0.f;
  const rppo::Map mp = indexed ? t->oi.map() : rppo::Map{};
  auto roll = [&](int store) {
    if (indexed)
      hipLaunchKernelGGL((rppt::track_courses_kernel<rppt::CHECK_INDEX>), dim3(blocks), dim3(rppt::TPB), 0, t->stream, a, store, mp);
    else
      hipLaunchKernelGGL((rppt::track_courses_kernel<rppt::CHECK_LINEAR>), dim3(blocks), dim3(rppt::TPB), 0, t->stream, a, store, mp);
  };
  rc = t->timed(&ms, [&] { roll(0); }, [&]() -> int {
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
      rc = t->timed(&ms, [&] { roll(1); });
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
  return guarded(t, "rrtx_tracker_run", [&] {
    const int rc = tracker_run(t, tp, b);
    if (t && rc >= 0) t->from = false, t->group = 0;   // this run has no winners and no goals to serve
    return rc;
  }, [&] { if (t) t->ran = false; });
}

}  // extern "C"

// ---- rrtx_tracker_run_from: the courses of a producer's last solve, read where they lie ----------------------------------------
namespace {
// What the tracker needs of a producer's last solve, whichever of the four objects it is
struct TrackSourceView {
  int device = 0;
  bool ran = false, has_points = false, has_hits = false;
  const char* no_run = "the source has no completed run";
  const char* no_points = "the source ran without points";
  uint64_t generation = 0;
  int64_t n = 0, n_points = 0;
  const int64_t* off = nullptr;                              // device, n + 1
  const double *x = nullptr, *y = nullptr, *yaw = nullptr;   // device, n_points each
  const int32_t* d_hit = nullptr;                            // device (steer) ...
  const int32_t* h_hit = nullptr;                            // ... or host (spline, bspline), n
};

TrackSourceView track_source_view(int32_t kind, const void* object) {
  TrackSourceView v;
  if (kind == RRTX_SRC_STEER) {
    const rrtx_steer* s = (const rrtx_steer*)object;
    v.device = s->device;
    v.ran = s->solved;
    if (s->cand_solved) v.no_run = "the last steer solve was rrtx_steer_solve_all and rrtx_steer_select_free has not followed";
    v.has_points = s->has_points && s->kind != rppsb::KIND_LQR;
    if (s->kind == rppsb::KIND_LQR) v.no_points = "the last steer solve was an LQR solve: a rollout has no yaw";
    else v.no_points = "the last steer solve was lengths-only, it has no points";
    v.has_hits = s->has_hits;
    v.generation = s->generation;
    v.n = s->n;
    v.n_points = s->n_points;
    v.off = s->offsets.as<const int64_t>();
    v.x = s->px.as<const double>();
    v.y = s->py.as<const double>();
    v.yaw = s->pyaw.as<const double>();
    v.d_hit = s->hit.as<const int32_t>();
  } else if (kind == RRTX_SRC_SPLINE) {
    const rrtx_spline* s = (const rrtx_spline*)object;
    v.device = s->device;
    v.ran = s->ran;
    v.has_points = s->has_arrays && s->axes == 2;
    v.no_points = s->axes == 2 ? "the last spline run was records-only, it has no points" : "one-dimensional splines are no courses";
    v.has_hits = s->has_hits;
    v.generation = s->generation;
    v.n = s->n;
    v.n_points = s->n_points;
    v.off = s->pt_off.as<const int64_t>();
    v.x = s->out.as<const double>();
    v.y = v.x + s->n_points;
    v.yaw = v.x + 2 * s->n_points;
    v.h_hit = s->h_hit.data();
  } else if (kind == RRTX_SRC_PLANNER) {
    const rrtx_handle* h = (const rrtx_handle*)object;
    v.device = h->device;
    v.ran = h->planned && h->run.stage == 0 && h->cs.generation > 0;
    v.no_run = "the planner has no completed plan with gathered courses (rrtx_gather_courses)";
    // a gather of another plan (or smoothing run) is stale whatever its number
    v.generation = courses_current(h) ? h->cs.generation : ~h->cs.generation;
    v.has_points = h->cs.has_yaw && h->cs.order == RRTX_ORDER_DRIVING;
    v.no_points = !h->cs.has_yaw ? "the gathered courses have no yaw (only RRTX_ALGO_RS planned courses do)"
                                 : "the courses were gathered in planning order, the tracker drives them: gather RRTX_ORDER_DRIVING";
    v.has_hits = false;
    v.n = h->n_inst;
    v.n_points = h->cs.n_points;
    v.off = h->cs.off.as<const int64_t>();
    v.x = h->cs.x.as<const double>();
    v.y = h->cs.y.as<const double>();
    v.yaw = h->cs.yaw.as<const double>();
  } else {
    const rrtx_bspline* s = (const rrtx_bspline*)object;
    v.device = s->device;
    v.ran = s->ran;
    v.has_points = s->has_arrays;
    v.no_points = "the last B-spline run was records-only, it has no points";
    v.has_hits = s->has_hits;
    v.generation = s->generation;
    v.n = s->n;
    v.n_points = s->n_points;
    v.off = s->pt_off.as<const int64_t>();
    v.x = s->out.as<const double>();
    v.y = v.x + s->n_points;
    v.yaw = v.x + 2 * s->n_points;
    v.h_hit = s->h_hit.data();
  }
  return v;
}
}  // namespace

static int tracker_run_from(rrtx_tracker* t, const rrtx_track_params* tp, const rrtx_track_source* src, const rrtx_track_batch* b) {
  const char* fn = "rrtx_tracker_run_from: ";
  auto bad = [&](const char* m) { return fail(t, RRTX_E_INVALID, std::string(fn) + m); };
  auto state = [&](const char* m) { return fail(t, RRTX_E_STATE, std::string(fn) + m); };
  if (!t) return bad("the tracker is NULL");
  if (!tp || !src || !b) return bad("the parameters, the source or the batch is NULL");
  if (src->kind != RRTX_SRC_STEER && src->kind != RRTX_SRC_SPLINE && src->kind != RRTX_SRC_BSPLINE && src->kind != RRTX_SRC_PLANNER)
    return bad("unknown source kind");
  if (src->select != RRTX_SELECT_ALL && src->select != RRTX_SELECT_FREE && src->select != RRTX_SELECT_MASK) return bad("unknown select");
  if (src->arrays_of != 0 && src->arrays_of != 1) return bad("unknown arrays_of");
  if (!src->object) return bad("the source object is NULL");
  if (src->kind == RRTX_SRC_PLANNER && !handle_is_live(src->object)) return bad("the source object is no planner handle of this process");
  if (b->offsets || b->x || b->y || b->yaw) return bad("offsets, x, y and yaw must be NULL: the courses are the source's");
  if (b->n < 0 || b->n > (1LL << 30)) return bad("n is negative or above 2^30");
  const int64_t n = b->n;
  if (src->group < 0) return bad("group is negative");
  if (src->group > 0 && n % src->group != 0) return bad("n is not a multiple of group");
  if (src->arrays_of == 1 && src->group == 0) return bad("arrays_of = 1 needs a group");
  if (src->select == RRTX_SELECT_MASK && !src->mask) return bad("mask is NULL");
  if (src->select != RRTX_SELECT_MASK && src->mask) return bad("a mask is given without RRTX_SELECT_MASK");
  // as rrtx_tracker_run, of the fields that remain
  if (!b->robot_radius) return bad("robot_radius is NULL");
  if (int orc = tracker_check_obstacles(t, b, n, bad)) return orc;
  if (!track_params_ok(tp)) return bad(TRACK_PARAMS_MSG);
  const int64_t n_rr = b->robot_radius_per_course ? n : 1;
  if (const char* m = obstacle_list_value_error(b->obstacles, b->n_obstacles, b->robot_radius, n_rr, TRACK_OBS_TEXT)) return bad(m);
  if (b->start_state && !all_finite(b->start_state, 4 * n)) return bad("a start state component is not finite");
  if (b->per_course && !all_finite(b->per_course, 3 * n)) return bad("a per-course value is not finite");
  if (!all_finite(&tp->target_speed, sizeof(*tp) / sizeof(double))) return bad("a parameter is not finite");
  if (int nd = t->need_device(fn)) return nd;
  const TrackSourceView v = track_source_view(src->kind, src->object);
  if (v.device != t->device) return bad("the source is on another device");
  if (!v.ran) return state(v.no_run);
  if (v.generation != src->generation) return state("the generation is stale: the source has solved again since");
  if (!v.has_points) return state(v.no_points);
  if (src->select == RRTX_SELECT_FREE && !v.has_hits)
    return state(src->kind == RRTX_SRC_PLANNER ? "RRTX_SELECT_FREE, but a planner's courses carry no hits"
                                               : "RRTX_SELECT_FREE, but the source ran without an obstacle list");
  if (n != v.n) return bad("n is not the source's course count");
  bool indexed = false;
  int ix_reason = 0;
  if (int irc = tracker_index_decide(t, b, fn, &indexed, &ix_reason)) return irc;

  const int64_t g = src->group, n_groups = g ? n / g : 0;
  const bool winners_only = src->arrays_of == 1;
  t->ran = false;
  t->has_arrays = false;
  t->ix_used = indexed;
  t->ix_reason = ix_reason;
  t->from = true;
  t->group = g;
  t->n = n;
  t->n_steps = 0;
  t->kernel_ms = 0.0;
  t->h_rec.clear();
  t->h_arr_off.assign((size_t)n + 1, 0);
  t->h_winner.assign((size_t)n_groups, -1);
  if (n == 0) {
    t->has_arrays = b->want_arrays != 0;
    t->ran = true;
    return RRTX_OK;
  }
  // the selection as the kernel reads it: the caller's mask, a steer's hits on the device, or a mask made of a spline's
  // hits (they live on the host, where a course without a sample is marked -2)
  int select = src->select;
  std::vector<uint8_t> free_mask;
  const uint8_t* h_mask = src->mask;
  if (select == RRTX_SELECT_FREE && !v.d_hit) {
    free_mask.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) free_mask[(size_t)i] = v.h_hit[i] == -1;
    h_mask = free_mask.data();
    select = RRTX_SELECT_MASK;
  }

  HIPCHK(t, hipSetDevice(t->device));
  int rc;
  const size_t N = (size_t)n;
  const int64_t want = (int64_t)t->n_cu * 16;   // 16 blocks of one wave per CU, as track_roll_kernel
  int blocks = (int)(n < want ? n : want);
  if (blocks < 1) blocks = 1;
  // a source without a single point never put its offsets on the device: every course is empty
  const int64_t* d_off = v.off;
  if (v.n_points == 0) {
    if ((rc = t->reserve(t->off, sizeof(int64_t) * (N + 1)))) return rc;
    HIPCHK(t, hipMemsetAsync(t->off.p, 0, sizeof(int64_t) * (N + 1), t->stream));
    d_off = t->off.as<const int64_t>();
  }
  if (select == RRTX_SELECT_MASK && (rc = t->upload(t->mask, h_mask, N))) return rc;
  if ((rc = t->reserve(t->goal, sizeof(double) * 3 * N))) return rc;
  if (g && (rc = t->reserve(t->winner, sizeof(int32_t) * (size_t)n_groups))) return rc;
  if (g && (rc = t->reserve(t->wgoal, sizeof(double) * 3 * (size_t)n_groups))) return rc;

  rppt::SourceArgs sa;
  memset(&sa, 0, sizeof(sa));
  rppt::CourseArgs& a = sa.c;
  if ((rc = tracker_common_args(t, tp, b, n, indexed, blocks, a))) return rc;
  a.off = d_off;
  a.x = v.x;
  a.y = v.y;
  a.yaw = v.yaw;
  sa.select = select;
  sa.hit = select == RRTX_SELECT_FREE ? v.d_hit : nullptr;
  sa.mask = select == RRTX_SELECT_MASK ? t->mask.as<const uint8_t>() : nullptr;
  sa.goal = t->goal.as<double>();
  sa.group = g;
  sa.winner = g ? t->winner.as<int32_t>() : nullptr;
  sa.wgoal = g ? t->wgoal.as<double>() : nullptr;

  // first launch: the records, and with a group the pick over them
  t->h_rec.resize(N);
  float ms = 0.f;
  const rppo::Map mp = indexed ? t->oi.map() : rppo::Map{};
  auto roll = [&](int store) {
    if (indexed)
      hipLaunchKernelGGL((rppt::track_source_kernel<rppt::CHECK_INDEX>), dim3(blocks), dim3(rppt::TPB), 0, t->stream, sa, store, mp);
    else
      hipLaunchKernelGGL((rppt::track_source_kernel<rppt::CHECK_LINEAR>), dim3(blocks), dim3(rppt::TPB), 0, t->stream, sa, store, mp);
  };
  rc = t->timed(&ms, [&] {
    roll(0);
    if (g) hipLaunchKernelGGL(rppt::track_group_pick_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, t->stream, sa);
  }, [&]() -> int {
    HIPCHK(t, hipMemcpyAsync(t->h_rec.data(), t->rec.p, sizeof(rppt::Record) * N, hipMemcpyDeviceToHost, t->stream));
    if (g) HIPCHK(t, hipMemcpyAsync(t->h_winner.data(), t->winner.p, sizeof(int32_t) * (size_t)n_groups, hipMemcpyDeviceToHost, t->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  t->kernel_ms = ms;

  // arr_offsets: exclusive sum of len over the courses that own entries (the complete ones, or of those the winners)
  int64_t tot = 0;
  bool partial = false;
  for (size_t i = 0; i < N; i++) {
    t->h_arr_off[i] = tot;
    const int ood = t->h_rec[i].ood;
    if (ood && ood != rppt::OOD_SKIPPED) partial = true;
    if (!ood && (!winners_only || t->h_winner[i / (size_t)g] == (int32_t)i)) tot += t->h_rec[i].n;
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
      sa.winners_only = winners_only ? 1 : 0;
      rc = t->timed(&ms, [&] { roll(1); });
      if (rc) return rc;
      t->kernel_ms += ms;
    }
    t->has_arrays = true;
  }
  t->ran = true;
  if (partial) {
    t->err = std::string(fn) + "some courses are too short, too long, not finite or left the replica's domain (see the ood column)";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

extern "C" {

int rrtx_tracker_run_from(rrtx_tracker* t, const rrtx_track_params* tp, const rrtx_track_source* src, const rrtx_track_batch* b) {
  return guarded(t, "rrtx_tracker_run_from", [&] { return tracker_run_from(t, tp, src, b); }, [&] { if (t) t->ran = false; });
}

int rrtx_tracker_get_winners(rrtx_tracker* t, int32_t* winner, int64_t* n_groups) {
  if (!t) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_winners: the tracker is NULL");
  if (!t->ran || !t->from || t->group == 0) return fail(t, RRTX_E_STATE, "rrtx_tracker_get_winners: no completed run with a group");
  if (n_groups) *n_groups = (int64_t)t->h_winner.size();
  if (winner && !t->h_winner.empty()) memcpy(winner, t->h_winner.data(), sizeof(int32_t) * t->h_winner.size());
  return RRTX_OK;
}

int rrtx_tracker_get_goals(rrtx_tracker* t, double* goals) {
  if (!t || !goals) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_goals: a NULL pointer");
  if (!t->ran || !t->from) return fail(t, RRTX_E_STATE, "rrtx_tracker_get_goals: no completed rrtx_tracker_run_from");
  const size_t rows = t->group ? t->h_winner.size() : (size_t)t->n;
  if (rows == 0) return RRTX_OK;
  return t->fetch(goals, t->group ? t->wgoal.p : t->goal.p, sizeof(double) * 3 * rows);
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
  double* dst[7] = {x, y, yaw, v, tt, a, d};
  for (int k = 0; k < 7; k++)
    if (dst[k])
      if (int rc = t->fetch(dst[k], t->out.as<const double>() + k * tot, sizeof(double) * tot)) return rc;
  return RRTX_OK;
}

int rrtx_tracker_set_obstacle_index(rrtx_tracker* t, int32_t mode) {
  const char* fn = "rrtx_tracker_set_obstacle_index: ";
  if (!t) return fail(t, RRTX_E_INVALID, std::string(fn) + "the tracker is NULL");
  if (mode != RRTX_OBSIDX_ON && mode != RRTX_OBSIDX_OFF)
    return fail(t, RRTX_E_INVALID, std::string(fn) + "mode is RRTX_OBSIDX_ON or RRTX_OBSIDX_OFF (RRTX_OBSIDX_AUTO would have to "
                                                     "accept lists that the default refuses)");
  t->oi.mode = mode;
  return RRTX_OK;
}

int rrtx_tracker_get_obstacle_index_info(rrtx_tracker* t, rrtx_obstacle_index_info* info) {
  if (!t || !info) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_obstacle_index_info: a NULL pointer");
  memset(info, 0, sizeof(*info));
  info->mode = t->oi.mode;
  info->used = t->ix_used;
  info->reason = t->ix_reason;
  if (t->ix_used) obstacle_grid_info(t->oi.grid, &info->map);
  return RRTX_OK;
}

int rrtx_tracker_get_obstacle_index(rrtx_tracker* t, int32_t* cell_start, rrtx_obstacle_item* items, int64_t cap_items,
                                    rrtx_obstacle_item* wide, int64_t cap_wide) {
  const char* fn = "rrtx_tracker_get_obstacle_index: ";
  if (!t) return fail(t, RRTX_E_INVALID, std::string(fn) + "the tracker is NULL");
  if (!t->ix_used) return fail(t, RRTX_E_STATE, std::string(fn) + "the obstacle index did not serve the last run");
  return obstacle_grid_fetch(t, t->oi.grid, fn, cell_start, items, cap_items, wide, cap_wide);
}

int rrtx_tracker_get_kernel_ms(rrtx_tracker* t, double* kernel_ms) {
  if (!t || !kernel_ms) return fail(t, RRTX_E_INVALID, "rrtx_tracker_get_kernel_ms: a NULL pointer");
  if (!t->ran) return fail(t, RRTX_E_STATE, "rrtx_tracker_get_kernel_ms: no completed run");
  *kernel_ms = t->kernel_ms;
  return RRTX_OK;
}

}  // extern "C"

// rrtx_api_spline.inc -- rrtx_spline_*: batched cubic-spline courses through waypoints (spline_batch.hip.h:
// spline_fit_kernel, spline_eval_kernel), one-dimensional splines over the caller's knots (spline_fit1d_kernel) and
// pointwise queries against either (spline_query_kernel); included by rrtx_api.hip

// ---- what rrtx_spline and rrtx_bspline share: courses fitted through waypoints, then sampled into a CSR list of points --------
struct CourseObj : DevObj {
  DevBuf pt_off, out, obs, hit;   // device buffers, grown on demand
  // the last run
  bool ran = false, has_arrays = false, has_hits = false;
  int64_t n = 0, n_wp = 0, n_points = 0;
  double kernel_ms = 0.0;
  uint64_t generation = 0;   // completed runs, rrtx_*_get_generation
  std::vector<int64_t> h_off;
  std::vector<int32_t> h_hit;
  ObsIndex oi;   // the obstacle index over the last run's list

  // a run begins, its arguments checked: nothing of the last one is served any more
  void begin_run(int64_t n_courses, int64_t n_waypoints) {
    ran = has_arrays = has_hits = false;
    n = n_courses;
    n_wp = n_waypoints;
    n_points = 0;
    kernel_ms = 0.0;
    h_hit.clear();
    h_off.assign((size_t)n + 1, 0);
  }

  // The second stage of a run, once the fit's records gave h_off and n_points: launch(store, check) queues the eval kernel
  // over `a` (check: rppc::CHECK_*), whose point offsets, output planes and obstacle list are set here; the hits come back
  // with it.  Without a point or without anything to do for one, the hits are what the fit left.
  template <class Args, class Launch>
  int eval_stage(Args& a, bool store, int64_t n_obs, Launch&& launch) {
    const size_t N = (size_t)n;
    const bool check = n_obs > 0;
    const int ck = !check ? rppc::CHECK_NONE : oi.used ? rppc::CHECK_INDEX : rppc::CHECK_LINEAR;
    int rc;
    if (check) h_hit.resize(N);
    if (n_points > 0 && (store || check)) {
      if (store && (rc = reserve(out, sizeof(double) * 5 * (size_t)n_points))) return rc;
      if ((rc = upload(pt_off, h_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
      a.pt_off = pt_off.as<const int64_t>();
      a.out = store ? out.as<double>() : nullptr;
      a.obs = check ? obs.as<const double>() : nullptr;
      a.n_obs = n_obs;
      if (ck == rppc::CHECK_INDEX) a.omap = oi.map();
      float ms = 0.f;
      rc = timed(&ms, [&] { launch(store, ck); }, [&]() -> int {
        if (check) HIPCHK(this, hipMemcpyAsync(h_hit.data(), hit.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, stream));
        return RRTX_OK;
      });
      if (rc) return rc;
      kernel_ms += ms;
    } else if (check) {
      HIPCHK(this, hipMemcpy(h_hit.data(), hit.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    }
    has_arrays = store;
    has_hits = check;
    ran = true;
    return RRTX_OK;
  }
};

// What both objects say of an obstacle list that is wrong (rrtx_host.h)
static const ObsListText COURSE_OBS_TEXT = {"n_obstacles is negative or above 2^20", "n_obstacles is negative or above 2^20",
                                            "obstacles is NULL", "an obstacle entry is not finite", "robot_radius is not finite"};

// The getters of both; fn: "rrtx_spline_get_points: ", noun: "spline" or "bspline"
static int course_null(const char* fn, const char* noun) {
  return fail<CourseObj>(nullptr, RRTX_E_INVALID, std::string(fn) + "the " + noun + " object is NULL");
}

// the checks of rrtx_*_get_records, and what both return: offsets and counts (any may be NULL)
static int course_get_counts(CourseObj* s, const char* fn, const char* noun, int64_t* offsets, int64_t* n_courses, int64_t* n_points) {
  if (!s) return course_null(fn, noun);
  if (!s->ran) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed run");
  if (offsets) memcpy(offsets, s->h_off.data(), sizeof(int64_t) * ((size_t)s->n + 1));
  if (n_courses) *n_courses = s->n;
  if (n_points) *n_points = s->n_points;
  return RRTX_OK;
}

// the five planes of the points: x, y, yaw, k and the parameter (any may be NULL)
static int course_get_points(CourseObj* s, const char* fn, const char* noun, double* x, double* y, double* yaw, double* k, double* t,
                             int64_t cap) {
  if (!s) return course_null(fn, noun);
  if (!s->ran || !s->has_arrays) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed run with arrays");
  if (cap < s->n_points) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  if (s->n_points == 0) return RRTX_OK;
  const size_t tot = (size_t)s->n_points;
  double* dst[5] = {x, y, yaw, k, t};
  for (int q = 0; q < 5; q++)
    if (dst[q])
      if (int rc = s->fetch(dst[q], s->out.as<const double>() + q * tot, sizeof(double) * tot)) return rc;
  return RRTX_OK;
}

static int course_get_hits(CourseObj* s, const char* fn, const char* noun, int32_t* hit) {
  if (!s) return course_null(fn, noun);
  if (!s->ran) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed run");
  if (!s->has_hits) return fail(s, RRTX_E_STATE, std::string(fn) + "the last run had no obstacle list");
  if (s->n == 0) return RRTX_OK;
  if (!hit) return fail(s, RRTX_E_INVALID, std::string(fn) + "hit is NULL");
  memcpy(hit, s->h_hit.data(), sizeof(int32_t) * (size_t)s->n);
  return RRTX_OK;
}

static int course_get_generation(CourseObj* s, const char* fn, uint64_t* generation) {
  if (!s || !generation) return fail(s, RRTX_E_INVALID, std::string(fn) + "a NULL pointer");
  *generation = s->generation;
  return RRTX_OK;
}

struct rrtx_spline : CourseObj {
  DevBuf wp_off, x, y, ds, cx, cy, tab, rec, q_off, q_t, q_out, q_status;   // device buffers, grown on demand
  int axes = 2;   // the last run, or fit1d: axes == 1 (generation counts both)
  // the last query against it
  bool queried = false, q_deriv = false;
  int64_t n_q = 0;
  double query_ms = 0.0;
  std::vector<rppsp::Record> h_rec;
  std::vector<int32_t> h_qst;
};

static_assert(sizeof(rppsp::Record) == sizeof(rrtx_spline_record), "rrtx_spline_record mirrors rppsp::Record");
static_assert(rppsp::MAX_WAYPOINTS == RRTX_SPLINE_MAX_WAYPOINTS, "the waypoint limit of the header is the kernel's");
static_assert(rpp::kSplineQOk == RRTX_SPLINE_Q_OK && rpp::kSplineQOutside == RRTX_SPLINE_Q_OUTSIDE &&
                  rpp::kSplineQRefRaises == RRTX_SPLINE_Q_REF_RAISES && rpp::kSplineQNoSpline == RRTX_SPLINE_Q_NO_SPLINE,
              "the query statuses of the header are the core's");

inline double (*volatile libm_hypot)(double, double) = hypot;

static int spline_run(rrtx_spline* s, const rrtx_spline_batch* b) {
  const char* fn = "rrtx_spline_run: ";
  auto bad = [&](const char* m) { return fail(s, RRTX_E_INVALID, std::string(fn) + m); };
  if (!s) return bad("the spline object is NULL");
  if (!b) return bad("the batch is NULL");
  if (b->n < 0 || b->n > (1LL << 30)) return bad("n is negative or above 2^30");
  if (!b->offsets || !b->ds) return bad("offsets or ds is NULL");
  const int64_t n = b->n;
  if (!csr_ok(b->offsets, n)) return bad("offsets do not start at 0 or decrease");
  const int64_t W = b->offsets[n];
  if (W > 0 && (!b->x || !b->y)) return bad("x or y is NULL");
  for (int64_t i = 0; i < n; i++) {
    const int64_t m = b->offsets[i + 1] - b->offsets[i];
    if (m < 2) return bad("a course of fewer than 2 waypoints");
    if (m > RRTX_SPLINE_MAX_WAYPOINTS) return bad("a course of more than 4096 waypoints");
  }
  if ((b->cx != nullptr) != (b->cy != nullptr)) return bad("one of cx, cy is NULL and the other is not");
  if (b->cx && b->n_c != W) return bad("n_c is not the number of waypoints");
  if (const char* m = obstacle_list_shape_error(b->obstacles, b->n_obstacles, 1LL << 20, COURSE_OBS_TEXT)) return bad(m);
  if (!all_finite(b->x, W) || !all_finite(b->y, W)) return bad("a coordinate is not finite");
  for (int64_t i = 0; i < W; i++)
    if (std::fabs(b->x[i]) > 1.0e6 || std::fabs(b->y[i]) > 1.0e6) return bad("a coordinate is above 1e6 in magnitude");
  if (b->cx && (!all_finite(b->cx, W) || !all_finite(b->cy, W))) return bad("a c value is not finite");
  if (const char* m = obstacle_list_value_error(b->obstacles, b->n_obstacles, &b->robot_radius, 1, COURSE_OBS_TEXT)) return bad(m);
  const int64_t n_ds = b->ds_per_course ? n : 1;
  for (int64_t i = 0; i < n_ds; i++)
    if (!std::isfinite(b->ds[i]) || !(b->ds[i] > 0.0)) return bad("a ds is not finite or not > 0");
  // the points in all, from the host's own hypot: one point of slack per course against the device's knots
  double est = 0.0;
  for (int64_t i = 0; i < n; i++) {
    double len = 0.0;
    for (int64_t k = b->offsets[i]; k + 1 < b->offsets[i + 1]; k++) len += libm_hypot(b->x[k + 1] - b->x[k], b->y[k + 1] - b->y[k]);
    est += std::ceil(len / b->ds[b->ds_per_course ? i : 0]) + 1.0;
    if (est > (double)RRTX_SPLINE_MAX_POINTS + (double)n) return bad("more than 2^28 points in all");
  }
  if (int nd = s->need_device(fn)) return nd;

  s->begin_run(n, W);
  s->queried = false;
  s->axes = 2;
  s->h_rec.clear();
  if (n == 0) {
    s->has_arrays = b->want_arrays != 0;
    s->has_hits = b->n_obstacles > 0;
    s->ran = true;
    return RRTX_OK;
  }
  // obstacle table: packed rows (ox, oy, thr), thr = (size + robot_radius) ** 2 by the planners' routine
  const int64_t n_obs = b->n_obstacles;
  std::vector<double> rows;
  pack_obstacle_rows(b->obstacles, n_obs, b->robot_radius, rows);
  // the obstacle index over the same list (rpp_obsgrid.h): built per run, kept while the rows and the radius stay
  if (int irc = obsindex_set_list(s, s->oi, b->obstacles, n_obs, b->robot_radius)) return irc;

  HIPCHK(s, hipSetDevice(s->device));
  int rc;
  const size_t N = (size_t)n;
  if ((rc = s->upload(s->wp_off, b->offsets, sizeof(int64_t) * (N + 1)))) return rc;
  if ((rc = s->upload(s->x, b->x, sizeof(double) * (size_t)W))) return rc;
  if ((rc = s->upload(s->y, b->y, sizeof(double) * (size_t)W))) return rc;
  if ((rc = s->upload(s->ds, b->ds, sizeof(double) * (size_t)n_ds))) return rc;
  if (b->cx) {
    if ((rc = s->upload(s->cx, b->cx, sizeof(double) * (size_t)W))) return rc;
    if ((rc = s->upload(s->cy, b->cy, sizeof(double) * (size_t)W))) return rc;
  }
  if ((rc = s->upload(s->obs, rows.data(), sizeof(double) * rows.size()))) return rc;
  if ((rc = s->reserve(s->tab, sizeof(double) * 8 * (size_t)W))) return rc;
  if ((rc = s->reserve(s->rec, sizeof(rppsp::Record) * N))) return rc;
  if (n_obs > 0 && (rc = s->reserve(s->hit, sizeof(int32_t) * N))) return rc;

  rppsp::Args a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.W = W;
  a.wp_off = s->wp_off.as<const int64_t>();
  a.x = s->x.as<const double>();
  a.y = s->y.as<const double>();
  a.ds = s->ds.as<const double>();
  a.ds_per_course = b->ds_per_course != 0;
  a.cx = b->cx ? s->cx.as<const double>() : nullptr;
  a.cy = b->cx ? s->cy.as<const double>() : nullptr;
  a.tab = s->tab.as<double>();
  a.rec = s->rec.as<rppsp::Record>();
  a.hit = n_obs > 0 ? s->hit.as<int32_t>() : nullptr;

  // the fit, and its records
  s->h_rec.resize(N);
  float ms = 0.f;
  const unsigned fit_blocks = (unsigned)((2 * n + rppsp::TPB - 1) / rppsp::TPB);
  rc = s->timed(&ms, [&] { hipLaunchKernelGGL(rppsp::spline_fit_kernel, dim3(fit_blocks), dim3(rppsp::TPB), 0, s->stream, a); },
                [&]() -> int {
                  HIPCHK(s, hipMemcpyAsync(s->h_rec.data(), s->rec.p, sizeof(rppsp::Record) * N, hipMemcpyDeviceToHost, s->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  s->kernel_ms = ms;

  // offsets: exclusive sum of the point counts
  int64_t tot = 0;
  bool partial = false;
  for (size_t i = 0; i < N; i++) {
    s->h_off[i] = tot;
    if (s->h_rec[i].status != RRTX_SPLINE_OK) partial = true;
    tot += s->h_rec[i].n_points;
    if (tot > RRTX_SPLINE_MAX_POINTS) return bad("more than 2^28 points in all");
  }
  s->h_off[N] = tot;
  s->n_points = tot;

  rc = s->eval_stage(a, b->want_arrays != 0, n_obs, [&](bool store, int check) {
    with_store_check(store, check, [&](auto st, auto ck) {
      const unsigned blocks = (unsigned)((tot + rppsp::TPB - 1) / rppsp::TPB);
      hipLaunchKernelGGL((rppsp::spline_eval_kernel<decltype(st)::value, decltype(ck)::value>), dim3(blocks), dim3(rppsp::TPB), 0,
                         s->stream, a);
    });
  });
  if (rc) return rc;
  // a course with no sample (s[-1] / ds underflows to 0) was tested against nothing
  for (size_t i = 0; s->has_hits && i < N; i++)
    if (s->h_rec[i].n_points == 0) s->h_hit[i] = -2;
  if (partial) {
    s->err = std::string(fn) + "some courses have coinciding waypoints, or a last sample on the last knot (see the status column)";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

static int spline_fit1d(rrtx_spline* s, const rrtx_spline_fit1d_batch* b) {
  const char* fn = "rrtx_spline_fit1d: ";
  auto bad = [&](const std::string& m) { return fail(s, RRTX_E_INVALID, std::string(fn) + m); };
  if (!s) return bad("the spline object is NULL");
  if (!b) return bad("the batch is NULL");
  if (b->n < 0 || b->n > (1LL << 30)) return bad("n is negative or above 2^30");
  if (!b->offsets) return bad("offsets is NULL");
  const int64_t n = b->n;
  if (!csr_ok(b->offsets, n)) return bad("offsets do not start at 0 or decrease");
  const int64_t W = b->offsets[n];
  if (W > 0 && (!b->knots || !b->values)) return bad("knots or values is NULL");
  if (b->c && b->n_c != W) return bad("n_c is not the number of knots");
  for (int64_t i = 0; i < n; i++) {
    const int64_t w0 = b->offsets[i], m = b->offsets[i + 1] - w0;
    const std::string who = "spline " + std::to_string(i);
    if (m < 2) return bad(who + " has fewer than 2 knots");
    if (m > RRTX_SPLINE_MAX_WAYPOINTS) return bad(who + " has more than 4096 knots");
    if (!all_finite(b->knots + w0, m) || !all_finite(b->values + w0, m)) return bad(who + ": a knot or a value is not finite");
    for (int64_t k = 0; k < m; k++)
      if (std::fabs(b->knots[w0 + k]) > 1.0e6 || std::fabs(b->values[w0 + k]) > 1.0e6)
        return bad(who + ": a knot or a value is above 1e6 in magnitude");
    for (int64_t k = 0; k + 1 < m; k++)
      if (b->knots[w0 + k + 1] < b->knots[w0 + k]) return bad(who + ": the knots must be sorted in ascending order");
    if (b->c && !all_finite(b->c + w0, m)) return bad(who + ": a c value is not finite");
  }
  if (int nd = s->need_device(fn)) return nd;

  s->begin_run(n, W);
  s->queried = false;
  s->axes = 1;
  s->h_rec.clear();
  if (n == 0) {
    s->ran = true;
    return RRTX_OK;
  }
  HIPCHK(s, hipSetDevice(s->device));
  int rc;
  const size_t N = (size_t)n;
  if ((rc = s->upload(s->wp_off, b->offsets, sizeof(int64_t) * (N + 1)))) return rc;
  if ((rc = s->upload(s->x, b->values, sizeof(double) * (size_t)W))) return rc;
  if (b->c && (rc = s->upload(s->cx, b->c, sizeof(double) * (size_t)W))) return rc;
  if ((rc = s->reserve(s->tab, sizeof(double) * 8 * (size_t)W))) return rc;
  if ((rc = s->reserve(s->rec, sizeof(rppsp::Record) * N))) return rc;
  // the knots are plane 0 of the table, where the two-axis fit puts its chord sums
  HIPCHK(s, hipMemcpyAsync(s->tab.p, b->knots, sizeof(double) * (size_t)W, hipMemcpyHostToDevice, s->stream));

  rppsp::Fit1dArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.W = W;
  a.wp_off = s->wp_off.as<const int64_t>();
  a.a = s->x.as<const double>();
  a.c = b->c ? s->cx.as<const double>() : nullptr;
  a.tab = s->tab.as<double>();
  a.rec = s->rec.as<rppsp::Record>();
  s->h_rec.resize(N);
  float ms = 0.f;
  const unsigned blocks = (unsigned)((n + rppsp::TPB - 1) / rppsp::TPB);
  rc = s->timed(&ms, [&] { hipLaunchKernelGGL(rppsp::spline_fit1d_kernel, dim3(blocks), dim3(rppsp::TPB), 0, s->stream, a); },
                [&]() -> int {
                  HIPCHK(s, hipMemcpyAsync(s->h_rec.data(), s->rec.p, sizeof(rppsp::Record) * N, hipMemcpyDeviceToHost, s->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  s->kernel_ms = ms;
  s->ran = true;
  for (size_t i = 0; i < N; i++)
    if (s->h_rec[i].status != RRTX_SPLINE_OK) {
      s->err = std::string(fn) + "some splines have two equal consecutive knots (see the status column)";
      return RRTX_PARTIAL;
    }
  return RRTX_OK;
}

template <int AXES, bool DERIV>
static void spline_launch_query(int64_t total, hipStream_t stream, const rppsp::QueryArgs& a) {
  const unsigned blocks = (unsigned)((total + rppsp::TPB - 1) / rppsp::TPB);
  hipLaunchKernelGGL((rppsp::spline_query_kernel<AXES, DERIV>), dim3(blocks), dim3(rppsp::TPB), 0, stream, a);
}

// planes of one query: x, y, yaw, k (+ dx, dy, ddx, ddy), or y (+ dy, ddy)
static int spline_query_planes(int axes, bool deriv) { return axes == 2 ? (deriv ? 8 : 4) : (deriv ? 3 : 1); }

static int spline_query(rrtx_spline* s, const rrtx_spline_query_batch* b) {
  const char* fn = "rrtx_spline_query: ";
  auto bad = [&](const char* m) { return fail(s, RRTX_E_INVALID, std::string(fn) + m); };
  if (!s) return bad("the spline object is NULL");
  if (!b) return bad("the batch is NULL");
  // what can be said of the batch alone, then the state, then the batch against the state
  if (b->n < 0 || b->n > (1LL << 30)) return bad("n is negative or above 2^30");
  if (!b->q_offsets) return bad("q_offsets is NULL");
  const int64_t n = b->n;
  if (!csr_ok(b->q_offsets, n)) return bad("q_offsets do not start at 0 or decrease");
  const int64_t Q = b->q_offsets[n];
  if (Q > RRTX_SPLINE_MAX_POINTS) return bad("more than 2^28 queries");
  if (Q > 0 && !b->t) return bad("t is NULL");
  if (!s->ran) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed run or fit1d");
  if (n != s->n) return bad("n is not the number of splines of the last run");
  if (int nd = s->need_device(fn)) return nd;

  s->queried = false;
  s->q_deriv = b->want_derivatives != 0;
  s->n_q = Q;
  s->query_ms = 0.0;
  s->h_qst.clear();
  if (Q == 0) {
    s->queried = true;
    return RRTX_OK;
  }
  HIPCHK(s, hipSetDevice(s->device));
  int rc;
  const int planes = spline_query_planes(s->axes, s->q_deriv);
  if ((rc = s->upload(s->q_off, b->q_offsets, sizeof(int64_t) * ((size_t)n + 1)))) return rc;
  if ((rc = s->upload(s->q_t, b->t, sizeof(double) * (size_t)Q))) return rc;
  if ((rc = s->reserve(s->q_out, sizeof(double) * (size_t)planes * (size_t)Q))) return rc;
  if ((rc = s->reserve(s->q_status, sizeof(int32_t) * (size_t)Q))) return rc;

  rppsp::QueryArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.W = s->n_wp;
  a.Q = Q;
  a.wp_off = s->wp_off.as<const int64_t>();
  a.q_off = s->q_off.as<const int64_t>();
  a.t = s->q_t.as<const double>();
  a.x = s->x.as<const double>();
  a.y = s->axes == 2 ? s->y.as<const double>() : a.x;
  a.tab = s->tab.as<const double>();
  a.rec = s->rec.as<const rppsp::Record>();
  a.out = s->q_out.as<double>();
  a.status = s->q_status.as<int32_t>();
  s->h_qst.resize((size_t)Q);
  float ms = 0.f;
  rc = s->timed(&ms, [&] {
    if (s->axes == 2 && s->q_deriv)
      spline_launch_query<2, true>(Q, s->stream, a);
    else if (s->axes == 2)
      spline_launch_query<2, false>(Q, s->stream, a);
    else if (s->q_deriv)
      spline_launch_query<1, true>(Q, s->stream, a);
    else
      spline_launch_query<1, false>(Q, s->stream, a);
  }, [&]() -> int {
    HIPCHK(s, hipMemcpyAsync(s->h_qst.data(), s->q_status.p, sizeof(int32_t) * (size_t)Q, hipMemcpyDeviceToHost, s->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  s->query_ms = ms;
  s->queried = true;
  for (int64_t i = 0; i < Q; i++)
    if (s->h_qst[(size_t)i] != RRTX_SPLINE_Q_OK) {
      s->err = std::string(fn) + "some queries are outside their spline, on its last knot, NaN, or have no spline (see the status plane)";
      return RRTX_PARTIAL;
    }
  return RRTX_OK;
}

extern "C" {

int rrtx_spline_create(int32_t device, rrtx_spline** out) { return create_object(device, out, "rrtx_spline_create"); }
void rrtx_spline_destroy(rrtx_spline* s) { destroy_object(s); }
const char* rrtx_spline_last_error(rrtx_spline* s) { return last_error_of(s); }

int rrtx_spline_run(rrtx_spline* s, const rrtx_spline_batch* b) {
  return guarded(s, "rrtx_spline_run", [&] { return new_generation(s, spline_run(s, b)); }, [&] { if (s) s->ran = false; });
}

int rrtx_spline_get_records(rrtx_spline* s, rrtx_spline_record* rec, int64_t* offsets, int64_t* n_courses, int64_t* n_points,
                            double* kernel_ms) {
  if (int rc = course_get_counts(s, "rrtx_spline_get_records: ", "spline", offsets, n_courses, n_points)) return rc;
  if (rec && s->n) memcpy(rec, s->h_rec.data(), sizeof(rrtx_spline_record) * (size_t)s->n);
  if (kernel_ms) *kernel_ms = s->kernel_ms;
  return RRTX_OK;
}

int rrtx_spline_get_points(rrtx_spline* s, double* x, double* y, double* yaw, double* k, double* t, int64_t cap) {
  return course_get_points(s, "rrtx_spline_get_points: ", "spline", x, y, yaw, k, t, cap);
}

int rrtx_spline_get_c(rrtx_spline* s, double* cx, double* cy, int64_t cap) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_spline_get_c: the spline object is NULL");
  if (!s->ran) return fail(s, RRTX_E_STATE, "rrtx_spline_get_c: no completed run");
  if (cap < s->n_wp) return fail(s, RRTX_E_CAPACITY, "rrtx_spline_get_c: the buffers are too small");
  if (s->n_wp == 0) return RRTX_OK;
  const size_t W = (size_t)s->n_wp;
  int rc;
  if (cx && (rc = s->fetch(cx, s->tab.as<const double>() + 3 * W, sizeof(double) * W))) return rc;
  if (cy && s->axes == 2 && (rc = s->fetch(cy, s->tab.as<const double>() + 6 * W, sizeof(double) * W))) return rc;
  return RRTX_OK;
}

int rrtx_spline_set_obstacle_index(rrtx_spline* s, int32_t mode) {
  return obsindex_set_mode(s, s ? &s->oi : nullptr, mode, "rrtx_spline_set_obstacle_index: ", false);
}

int rrtx_spline_get_obstacle_index_info(rrtx_spline* s, rrtx_obstacle_index_info* info) {
  return obsindex_get_info(s, s ? &s->oi : nullptr, info, "rrtx_spline_get_obstacle_index_info: ");
}

int rrtx_spline_get_hits(rrtx_spline* s, int32_t* hit) { return course_get_hits(s, "rrtx_spline_get_hits: ", "spline", hit); }

int rrtx_spline_get_generation(rrtx_spline* s, uint64_t* generation) {
  return course_get_generation(s, "rrtx_spline_get_generation: ", generation);
}

int rrtx_spline_fit1d(rrtx_spline* s, const rrtx_spline_fit1d_batch* b) {
  return guarded(s, "rrtx_spline_fit1d", [&] { return new_generation(s, spline_fit1d(s, b)); }, [&] { if (s) s->ran = false; });
}

int rrtx_spline_query(rrtx_spline* s, const rrtx_spline_query_batch* b) {
  return guarded(s, "rrtx_spline_query", [&] { return spline_query(s, b); }, [&] { if (s) s->queried = false; });
}

int rrtx_spline_get_query(rrtx_spline* s, double* x, double* y, double* yaw, double* k, double* dx, double* dy, double* ddx,
                          double* ddy, int32_t* status, int64_t cap) {
  const char* fn = "rrtx_spline_get_query: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the spline object is NULL");
  if (!s->ran || !s->queried) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed query");
  if (s->axes == 1 && (x || yaw || k || dx || ddx))
    return fail(s, RRTX_E_STATE, std::string(fn) + "one-dimensional splines have the planes y, dy and ddy only");
  if (!s->q_deriv && (dx || dy || ddx || ddy))
    return fail(s, RRTX_E_STATE, std::string(fn) + "the query was made without derivatives");
  if (cap < s->n_q) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  if (s->n_q == 0) return RRTX_OK;
  const size_t Q = (size_t)s->n_q;
  double* two[8] = {x, y, yaw, k, dx, dy, ddx, ddy};
  double* one[3] = {y, dy, ddy};
  double** dst = s->axes == 2 ? two : one;
  const int planes = spline_query_planes(s->axes, s->q_deriv);
  for (int q = 0; q < planes; q++)
    if (dst[q])
      if (int rc = s->fetch(dst[q], s->q_out.as<const double>() + q * Q, sizeof(double) * Q)) return rc;
  if (status) memcpy(status, s->h_qst.data(), sizeof(int32_t) * Q);
  return RRTX_OK;
}

int rrtx_spline_get_query_info(rrtx_spline* s, int64_t* n_queries, int32_t* axes, int32_t* has_derivatives, double* kernel_ms) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_spline_get_query_info: the spline object is NULL");
  if (!s->ran || !s->queried) return fail(s, RRTX_E_STATE, "rrtx_spline_get_query_info: no completed query");
  if (n_queries) *n_queries = s->n_q;
  if (axes) *axes = s->axes;
  if (has_derivatives) *has_derivatives = s->q_deriv ? 1 : 0;
  if (kernel_ms) *kernel_ms = s->query_ms;
  return RRTX_OK;
}

}  // extern "C"

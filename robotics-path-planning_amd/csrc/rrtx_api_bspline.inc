// rrtx_api_bspline.inc -- rrtx_bspline_*: batched B-spline courses through waypoints, interpolating (bspline_batch.hip.h:
// bspline_fit_kernel, bspline_eval_kernel) and smoothing (bspline_smooth.hip.h: bspline_smooth_fit_kernel,
// bspline_smooth_eval_kernel); included by rrtx_api.hip
struct rrtx_bspline : CourseObj {   // rrtx_api_spline.inc; generation counts runs and approximations
  DevBuf wp_off, x, y, degree, mode_of, count, ds, us_off, us, tab, knots, rec, sm, arec;   // device buffers, grown on demand
  bool smooth = false;   // the last run was rrtx_bspline_approximate
  int64_t n_knots = 0;
  std::vector<rppbs::Record> h_rec;
  std::vector<int64_t> h_wp_off, h_knot_off;
  std::vector<rpp::SmoothInfo> h_arec;   // [2][n], axis-major
};

static_assert(sizeof(rppbs::Record) == sizeof(rrtx_bspline_record), "rrtx_bspline_record mirrors rppbs::Record");
static_assert(rppbs::MAX_WAYPOINTS == RRTX_BSPLINE_MAX_WAYPOINTS, "the waypoint limit of the header is the kernel's");
static_assert(rpp::kBsplineMaxDegree == RRTX_BSPLINE_MAX_DEGREE, "the degree limit of the header is the core's");
static_assert(sizeof(rpp::SmoothInfo) == sizeof(rrtx_bspline_axis_record), "rrtx_bspline_axis_record mirrors rpp::SmoothInfo");
static_assert(rpp::kBsplineOk == RRTX_BSPLINE_OK && rpp::kBsplineDegenerate == RRTX_BSPLINE_DEGENERATE &&
                  rpp::kBsplineTooFew == RRTX_BSPLINE_TOO_FEW && rpp::kBsplineSingular == RRTX_BSPLINE_SINGULAR,
              "the statuses of the header are the core's");
static_assert(rpp::kBsplineNormalised == RRTX_BSPLINE_PARAM_NORMALISED && rpp::kBsplineChord == RRTX_BSPLINE_PARAM_CHORD &&
                  rpp::kBsplineLinspace == RRTX_BSPLINE_SAMPLE_LINSPACE && rpp::kBsplineArange == RRTX_BSPLINE_SAMPLE_ARANGE &&
                  rpp::kBsplineExplicit == RRTX_BSPLINE_SAMPLE_EXPLICIT,
              "the modes of the header are the core's");

// rrtx_bspline_run (sb NULL) and rrtx_bspline_approximate (sb the smoothing batch, b its run part)
static int bspline_run(rrtx_bspline* s, const rrtx_bspline_batch* b, const rrtx_bspline_smooth_batch* sb, const char* fn) {
  auto bad = [&](const char* m) { return fail(s, RRTX_E_INVALID, std::string(fn) + m); };
  if (!s) return bad("the bspline object is NULL");
  if (!b) return bad("the batch is NULL");
  if (b->n < 0 || b->n > (1LL << 30)) return bad("n is negative or above 2^30");
  if (!b->offsets || !b->degree) return bad("offsets or degree is NULL");
  if (b->param != RRTX_BSPLINE_PARAM_NORMALISED && b->param != RRTX_BSPLINE_PARAM_CHORD) return bad("param is not RRTX_BSPLINE_PARAM_*");
  if (b->sample < RRTX_BSPLINE_SAMPLE_LINSPACE || b->sample > RRTX_BSPLINE_SAMPLE_EXPLICIT) return bad("sample is not RRTX_BSPLINE_SAMPLE_*");
  const int64_t n = b->n;
  if (!csr_ok(b->offsets, n)) return bad("offsets do not start at 0 or decrease");
  const int64_t W = b->offsets[n];
  if (W > 0 && (!b->x || !b->y)) return bad("x or y is NULL");
  for (int64_t i = 0; i < n; i++) {
    const int64_t m = b->offsets[i + 1] - b->offsets[i];
    if (m < 2) return bad("a course of fewer than 2 waypoints");
    if (m > RRTX_BSPLINE_MAX_WAYPOINTS) return bad("a course of more than 4096 waypoints");
  }
  const int64_t n_deg = b->degree_per_course ? n : 1;
  for (int64_t i = 0; i < n_deg; i++)
    if (b->degree[i] < 1 || b->degree[i] > RRTX_BSPLINE_MAX_DEGREE) return bad("a degree is not 1 .. 5");
  if (const char* m = obstacle_list_shape_error(b->obstacles, b->n_obstacles, 1LL << 20, COURSE_OBS_TEXT)) return bad(m);
  if (!all_finite(b->x, W) || !all_finite(b->y, W)) return bad("a coordinate is not finite");
  for (int64_t i = 0; i < W; i++)
    if (std::fabs(b->x[i]) > 1.0e6 || std::fabs(b->y[i]) > 1.0e6) return bad("a coordinate is above 1e6 in magnitude");
  if (const char* m = obstacle_list_value_error(b->obstacles, b->n_obstacles, &b->robot_radius, 1, COURSE_OBS_TEXT)) return bad(m);
  const int64_t n_s = sb && sb->s_per_course ? n : 1;
  if (sb) {
    if (!sb->s) return bad("s is NULL");
    if (b->param != RRTX_BSPLINE_PARAM_NORMALISED) return bad("param is not RRTX_BSPLINE_PARAM_NORMALISED");
    for (int64_t i = 0; i < n_s; i++)
      if (!std::isfinite(sb->s[i]) || !(sb->s[i] >= 0.0)) return bad("an s is not finite or negative");
  }
  // the sampling modes' own arguments, and the points in all
  auto mode_of = [&](int64_t i) { return b->sample_of ? b->sample_of[i] : b->sample; };
  bool any_lin = false, any_ara = false, any_exp = false;
  for (int64_t i = 0; i < n; i++) {
    const int mo = mode_of(i);
    if (mo < RRTX_BSPLINE_SAMPLE_LINSPACE || mo > RRTX_BSPLINE_SAMPLE_EXPLICIT) return bad("a sample_of entry is not RRTX_BSPLINE_SAMPLE_*");
    any_lin |= mo == RRTX_BSPLINE_SAMPLE_LINSPACE;
    any_ara |= mo == RRTX_BSPLINE_SAMPLE_ARANGE;
    any_exp |= mo == RRTX_BSPLINE_SAMPLE_EXPLICIT;
  }
  if (any_lin && !b->count) return bad("count is NULL");
  if (any_ara && !b->ds) return bad("ds is NULL");
  if (any_exp && !b->u_offsets) return bad("u_offsets is NULL");
  const int64_t n_smp = b->sample_per_course ? n : 1;
  int64_t n_us = 0;
  if (any_exp) {
    if (!csr_ok(b->u_offsets, n)) return bad("u_offsets do not start at 0 or decrease");
    n_us = b->u_offsets[n];
    if (n_us > RRTX_BSPLINE_MAX_POINTS) return bad("more than 2^28 points in all");
    if (n_us > 0 && !b->u) return bad("u is NULL");
    if (!all_finite(b->u, n_us)) return bad("a sample parameter is not finite");
  }
  double est = 0.0;
  const char* many = "more than 2^28 points in all";
  for (int64_t i = 0; i < n; i++) {
    const int mo = mode_of(i);
    const int64_t j = b->sample_per_course ? i : 0;
    if (mo == RRTX_BSPLINE_SAMPLE_LINSPACE) {
      if (b->count[j] < 1) return bad("an n_path_points (count) is below 1");
      est += (double)b->count[j];
    } else if (mo == RRTX_BSPLINE_SAMPLE_ARANGE) {
      if (!std::isfinite(b->ds[j]) || !(b->ds[j] > 0.0)) return bad("a ds is not finite or not > 0");
      double len = 0.0;   // from the host's own hypot: one point of slack per course against the device's sum
      for (int64_t k = b->offsets[i]; k + 1 < b->offsets[i + 1]; k++) len += libm_hypot(b->x[k + 1] - b->x[k], b->y[k + 1] - b->y[k]);
      if (b->param == RRTX_BSPLINE_PARAM_NORMALISED) len = 1.0;
      est += std::ceil(len / b->ds[j]) + 1.0;
    } else {
      est += (double)(b->u_offsets[i + 1] - b->u_offsets[i]);
    }
    if (est > (double)RRTX_BSPLINE_MAX_POINTS + (double)n) return bad(many);
  }
  if (int nd = s->need_device(fn)) return nd;

  s->begin_run(n, W);
  s->smooth = sb != nullptr;
  s->h_arec.clear();
  s->n_knots = 0;
  s->h_rec.clear();
  s->h_knot_off.assign((size_t)n + 1, 0);
  s->h_wp_off.assign(b->offsets, b->offsets + n + 1);
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
  if ((rc = s->upload(s->degree, b->degree, sizeof(int32_t) * (size_t)n_deg))) return rc;
  if (b->sample_of && (rc = s->upload(s->mode_of, b->sample_of, sizeof(int32_t) * N))) return rc;
  if (any_lin && (rc = s->upload(s->count, b->count, sizeof(int64_t) * (size_t)n_smp))) return rc;
  if (any_ara && (rc = s->upload(s->ds, b->ds, sizeof(double) * (size_t)n_smp))) return rc;
  if (any_exp) {
    if ((rc = s->upload(s->us_off, b->u_offsets, sizeof(int64_t) * (N + 1)))) return rc;
    if ((rc = s->upload(s->us, b->u, sizeof(double) * (size_t)n_us))) return rc;
  }
  if ((rc = s->upload(s->obs, rows.data(), sizeof(double) * rows.size()))) return rc;
  const size_t planes = sb ? rppbs::SMOOTH_TAB_PLANES : rppbs::TAB_PLANES, knot_planes = sb ? 2 : 1;
  if ((rc = s->reserve(s->tab, sizeof(double) * planes * (size_t)W))) return rc;
  if ((rc = s->reserve(s->knots, sizeof(double) * knot_planes * ((size_t)W + rppbs::KNOT_SLACK * N)))) return rc;
  if (sb) {
    if ((rc = s->upload(s->sm, sb->s, sizeof(double) * (size_t)n_s))) return rc;
    if ((rc = s->reserve(s->arec, sizeof(rpp::SmoothInfo) * 2 * N))) return rc;
  }
  if ((rc = s->reserve(s->rec, sizeof(rppbs::Record) * N))) return rc;
  if (n_obs > 0 && (rc = s->reserve(s->hit, sizeof(int32_t) * N))) return rc;

  rppbs::Args a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.W = W;
  a.wp_off = s->wp_off.as<const int64_t>();
  a.x = s->x.as<const double>();
  a.y = s->y.as<const double>();
  a.degree = s->degree.as<const int32_t>();
  a.degree_per_course = b->degree_per_course != 0;
  a.param = b->param;
  a.mode = b->sample;
  a.mode_of = b->sample_of ? s->mode_of.as<const int32_t>() : nullptr;
  a.per_course = b->sample_per_course != 0;
  a.count = s->count.as<const int64_t>();
  a.ds = s->ds.as<const double>();
  a.us_off = s->us_off.as<const int64_t>();
  a.us = s->us.as<const double>();
  a.tab = s->tab.as<double>();
  a.knots = s->knots.as<double>();
  a.rec = s->rec.as<rppbs::Record>();
  a.hit = n_obs > 0 ? s->hit.as<int32_t>() : nullptr;
  rppbs::SmoothArgs sa;
  memset(&sa, 0, sizeof(sa));
  if (sb) {
    sa.s = s->sm.as<const double>();
    sa.s_per_course = sb->s_per_course != 0;
    sa.arec = s->arec.as<rpp::SmoothInfo>();
    s->h_arec.resize(2 * N);
  }

  // the fit, and its records
  s->h_rec.resize(N);
  float ms = 0.f;
  const unsigned fit_blocks = (unsigned)(((sb ? 2 * n : n) + rppbs::FIT_TPB - 1) / rppbs::FIT_TPB);
  rc = s->timed(&ms, [&] {
    if (sb) {
      sa.a = a;
      hipLaunchKernelGGL(rppbs::bspline_smooth_fit_kernel, dim3(fit_blocks), dim3(rppbs::FIT_TPB), 0, s->stream, sa);
    } else {
      hipLaunchKernelGGL(rppbs::bspline_fit_kernel, dim3(fit_blocks), dim3(rppbs::FIT_TPB), 0, s->stream, a);
    }
  }, [&]() -> int {
    HIPCHK(s, hipMemcpyAsync(s->h_rec.data(), s->rec.p, sizeof(rppbs::Record) * N, hipMemcpyDeviceToHost, s->stream));
    if (sb) HIPCHK(s, hipMemcpyAsync(s->h_arec.data(), s->arec.p, sizeof(rpp::SmoothInfo) * 2 * N, hipMemcpyDeviceToHost, s->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  s->kernel_ms = ms;

  // offsets: exclusive sums of the point counts and of the knot counts
  int64_t tot = 0, knots = 0;
  bool partial = false;
  for (size_t i = 0; i < N; i++) {
    s->h_off[i] = tot;
    s->h_knot_off[i] = knots;
    if (s->h_rec[i].status != RRTX_BSPLINE_OK) partial = true;
    else if (!sb) knots += (b->offsets[i + 1] - b->offsets[i]) + s->h_rec[i].degree + 1;
    if (sb) knots += s->h_arec[i].n_knots + s->h_arec[N + i].n_knots;
    tot += s->h_rec[i].n_points;
    if (tot > RRTX_BSPLINE_MAX_POINTS) return bad(many);
  }
  s->h_off[N] = tot;
  s->h_knot_off[N] = knots;
  s->n_points = tot;
  s->n_knots = knots;

  rc = s->eval_stage(a, b->want_arrays != 0, n_obs, [&](bool store, int check) {
    const unsigned blocks = (unsigned)((tot + rppbs::TPB - 1) / rppbs::TPB);
    sa.a = a;
    with_store_check(store, check, [&](auto st, auto ck) {
      constexpr bool STORE = decltype(st)::value;
      constexpr int CHECK = decltype(ck)::value;
      if (sb)
        hipLaunchKernelGGL((rppbs::bspline_smooth_eval_kernel<STORE, CHECK>), dim3(blocks), dim3(rppbs::TPB), 0, s->stream, sa);
      else
        hipLaunchKernelGGL((rppbs::bspline_eval_kernel<STORE, CHECK>), dim3(blocks), dim3(rppbs::TPB), 0, s->stream, a);
    });
  });
  if (rc) return rc;
  if (partial) {
    s->err = std::string(fn) + "some courses have coinciding waypoints, no more waypoints than their degree, or no finite fit (see the status column)";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

extern "C" {

int rrtx_bspline_create(int32_t device, rrtx_bspline** out) { return create_object(device, out, "rrtx_bspline_create"); }
void rrtx_bspline_destroy(rrtx_bspline* s) { destroy_object(s); }
const char* rrtx_bspline_last_error(rrtx_bspline* s) { return last_error_of(s); }

int rrtx_bspline_run(rrtx_bspline* s, const rrtx_bspline_batch* b) {
  return guarded(s, "rrtx_bspline_run", [&] { return new_generation(s, bspline_run(s, b, nullptr, "rrtx_bspline_run: ")); },
                 [&] { if (s) s->ran = false; });
}

int rrtx_bspline_approximate(rrtx_bspline* s, const rrtx_bspline_smooth_batch* sb) {
  return guarded(s, "rrtx_bspline_approximate", [&] {
    return new_generation(s, bspline_run(s, sb ? &sb->run : nullptr, sb, "rrtx_bspline_approximate: "));
  }, [&] { if (s) s->ran = false; });
}

int rrtx_bspline_get_axis_records(rrtx_bspline* s, rrtx_bspline_axis_record* rec, int64_t cap) {
  const char* fn = "rrtx_bspline_get_axis_records: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the bspline object is NULL");
  if (!s->ran || !s->smooth) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed rrtx_bspline_approximate");
  if (s->n == 0) return RRTX_OK;
  if (!rec) return fail(s, RRTX_E_INVALID, std::string(fn) + "rec is NULL");
  if (cap < 2 * s->n) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the buffer is too small");
  memcpy(rec, s->h_arec.data(), sizeof(rrtx_bspline_axis_record) * 2 * (size_t)s->n);
  return RRTX_OK;
}

int rrtx_bspline_get_axis_splines(rrtx_bspline* s, int32_t axis, int64_t* knot_offsets, double* knots, int64_t cap_knots,
                                  int64_t* coef_offsets, double* coefficients, int64_t cap_coefs, int64_t* n_knots, int64_t* n_coefs) {
  const char* fn = "rrtx_bspline_get_axis_splines: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the bspline object is NULL");
  if (!s->ran || !s->smooth) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed rrtx_bspline_approximate");
  if (axis != 0 && axis != 1) return fail(s, RRTX_E_INVALID, std::string(fn) + "axis is not 0 or 1");
  return guarded(s, "rrtx_bspline_get_axis_splines", [&]() -> int {
    const size_t W = (size_t)s->n_wp, N = (size_t)s->n;
    std::vector<int64_t> koff(N + 1, 0), coff(N + 1, 0);
    for (size_t c = 0; c < N; c++) {
      const int nk = s->h_arec[axis * N + c].n_knots;
      koff[c + 1] = koff[c] + nk;
      coff[c + 1] = coff[c] + (nk > 0 ? nk - s->h_rec[c].degree - 1 : 0);
    }
    if (n_knots) *n_knots = koff[N];
    if (n_coefs) *n_coefs = coff[N];
    if (knots && cap_knots < koff[N]) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the knot buffer is too small");
    if (coefficients && cap_coefs < coff[N]) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the coefficient buffer is too small");
    if (knot_offsets) memcpy(knot_offsets, koff.data(), sizeof(int64_t) * (N + 1));
    if (coef_offsets) memcpy(coef_offsets, coff.data(), sizeof(int64_t) * (N + 1));
    if (W == 0 || (!knots && !coefficients)) return RRTX_OK;
    const size_t plane = W + rppbs::KNOT_SLACK * N;
    std::vector<double> raw(plane > W ? plane : W);
    if (knots && koff[N] > 0) {   // the device keeps a course's knots at wp_off + 6 c of the axis' plane: packed here
      if (int rc = s->fetch(raw.data(), s->knots.as<const double>() + axis * plane, sizeof(double) * plane)) return rc;
      for (size_t c = 0; c < N; c++)
        if (koff[c + 1] > koff[c])
          memcpy(knots + koff[c], raw.data() + s->h_wp_off[c] + rppbs::KNOT_SLACK * c, sizeof(double) * (size_t)(koff[c + 1] - koff[c]));
    }
    if (coefficients && coff[N] > 0) {
      if (int rc = s->fetch(raw.data(), s->tab.as<const double>() + ((size_t)axis * rppbs::SMOOTH_AXIS_PLANES + 1) * W, sizeof(double) * W))
        return rc;
      for (size_t c = 0; c < N; c++)
        if (coff[c + 1] > coff[c])
          memcpy(coefficients + coff[c], raw.data() + s->h_wp_off[c], sizeof(double) * (size_t)(coff[c + 1] - coff[c]));
    }
    return RRTX_OK;
  });
}

int rrtx_bspline_get_records(rrtx_bspline* s, rrtx_bspline_record* rec, int64_t* offsets, int64_t* n_courses, int64_t* n_points,
                             int64_t* n_knots) {
  if (int rc = course_get_counts(s, "rrtx_bspline_get_records: ", "bspline", offsets, n_courses, n_points)) return rc;
  if (rec && s->n) memcpy(rec, s->h_rec.data(), sizeof(rrtx_bspline_record) * (size_t)s->n);
  if (n_knots) *n_knots = s->n_knots;
  return RRTX_OK;
}

int rrtx_bspline_get_points(rrtx_bspline* s, double* x, double* y, double* yaw, double* k, double* u, int64_t cap) {
  return course_get_points(s, "rrtx_bspline_get_points: ", "bspline", x, y, yaw, k, u, cap);
}

int rrtx_bspline_get_coefficients(rrtx_bspline* s, int64_t* knot_offsets, double* knots, int64_t cap_knots, double* cx, double* cy,
                                  int64_t cap_wp) {
  const char* fn = "rrtx_bspline_get_coefficients: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the bspline object is NULL");
  if (!s->ran) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed run");
  if (s->smooth) return fail(s, RRTX_E_STATE, std::string(fn) + "the last run was rrtx_bspline_approximate: its axes have knot vectors of their own (rrtx_bspline_get_axis_splines)");
  if (knots && cap_knots < s->n_knots) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the knot buffer is too small");
  if ((cx || cy) && cap_wp < s->n_wp) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the coefficient buffers are too small");
  if (knot_offsets) memcpy(knot_offsets, s->h_knot_off.data(), sizeof(int64_t) * ((size_t)s->n + 1));
  if (s->n_wp == 0) return RRTX_OK;
  const size_t W = (size_t)s->n_wp, N = (size_t)s->n;
  return guarded(s, "rrtx_bspline_get_coefficients", [&]() -> int {
    int rc;
    if (knots && s->n_knots > 0) {   // the device keeps a course's knots at wp_off + 6 c: packed here
      std::vector<double> raw(W + rppbs::KNOT_SLACK * N);
      if ((rc = s->fetch(raw.data(), s->knots.p, sizeof(double) * raw.size()))) return rc;
      for (size_t c = 0; c < N; c++) {
        const int64_t cnt = s->h_knot_off[c + 1] - s->h_knot_off[c];
        if (cnt > 0) memcpy(knots + s->h_knot_off[c], raw.data() + s->h_wp_off[c] + rppbs::KNOT_SLACK * c, sizeof(double) * (size_t)cnt);
      }
    }
    if (cx && (rc = s->fetch(cx, s->tab.as<const double>() + W, sizeof(double) * W))) return rc;
    if (cy && (rc = s->fetch(cy, s->tab.as<const double>() + 2 * W, sizeof(double) * W))) return rc;
    return RRTX_OK;
  });
}

int rrtx_bspline_set_obstacle_index(rrtx_bspline* s, int32_t mode) {
  return obsindex_set_mode(s, s ? &s->oi : nullptr, mode, "rrtx_bspline_set_obstacle_index: ", false);
}

int rrtx_bspline_get_obstacle_index_info(rrtx_bspline* s, rrtx_obstacle_index_info* info) {
  return obsindex_get_info(s, s ? &s->oi : nullptr, info, "rrtx_bspline_get_obstacle_index_info: ");
}

int rrtx_bspline_get_hits(rrtx_bspline* s, int32_t* hit) { return course_get_hits(s, "rrtx_bspline_get_hits: ", "bspline", hit); }

int rrtx_bspline_get_generation(rrtx_bspline* s, uint64_t* generation) {
  return course_get_generation(s, "rrtx_bspline_get_generation: ", generation);
}

int rrtx_bspline_get_kernel_ms(rrtx_bspline* s, double* kernel_ms) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_bspline_get_kernel_ms: the bspline object is NULL");
  if (!s->ran) return fail(s, RRTX_E_STATE, "rrtx_bspline_get_kernel_ms: no completed run");
  if (!kernel_ms) return fail(s, RRTX_E_INVALID, "rrtx_bspline_get_kernel_ms: kernel_ms is NULL");
  *kernel_ms = s->kernel_ms;
  return RRTX_OK;
}

}  // extern "C"

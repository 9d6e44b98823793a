// rrtx_api_steer.inc -- rrtx_steer_*: batched Dubins / Reeds-Shepp / Bezier curves between pose pairs and LQR rollouts
// between point pairs (steer_batch.hip.h); included by rrtx_api.hip
struct rrtx_steer : DevObj {
  // device buffers, grown on demand and shared by the kinds: a solve writes every entry it later serves
  DevBuf starts, goals, curv, status, nseg, total, seglen, modes, npts, plan, offsets, px, py, pyaw, flag, obs, hit, ends;
  DevBuf bez_w, bez_cp, pk, kmax;   // Bezier: weight table, control points (n, m, 2), curvature per point, max |curvature|
  // the obstacle list of rrtx_steer_set_obstacles: packed rows (ox, oy, thr); it goes to the device at the next solve
  std::vector<double> h_obs;
  bool obs_dirty = false;
  ObsIndex oi;   // the obstacle index over the same list, built by rrtx_steer_set_obstacles
  // the last solve
  bool solved = false, has_points = false, has_hits = false;
  bool has_k = false;   // a Bezier solve with want_curvature
  int bez_m = 0;        // a Bezier solve: control points per curve
  int kind = rppsb::KIND_DUBINS;
  int64_t n = 0, n_points = 0;
  double kernel_ms = 0.0;
  uint64_t generation = 0;   // completed solves (every entry point that writes the buffers above), rrtx_steer_get_generation
  std::vector<int64_t> h_offsets;
  // the last rrtx_steer_solve_all: every candidate of every pair.  Pair-level status is `status` above; everything per
  // candidate lives in buffers of its own, so that rrtx_steer_select_free can write an ordinary result beside them.
  DevBuf c_ncand, c_off, c_pair, c_variant, c_key, c_nseg, c_total, c_seglen, c_modes, c_npts, c_plan, c_hit, c_poff, c_px, c_py,
      c_pyaw, c_pdir, c_chosen, c_rank, c_nfree;
  bool cand_solved = false, cand_points = false, cand_hits = false;
  int cand_kind = rppsb::KIND_DUBINS, cand_flag = 0;
  int64_t cand_pairs = 0, n_cand = 0, cand_n_points = 0;
  double cand_ms = 0.0;
  rppsb::Args cand_args;    // the candidates' Args of that solve (device pointers into the buffers above)
  rppsb::CandArgs cand_c;
  std::vector<int64_t> h_cand_off, h_cand_poff;
};

namespace {
// stage 2 with or without the stores and the obstacle check; one of the two is wanted
// check: rppsb::CHECK_*
template <int KIND>
void steer_launch_fill(bool store, int check, unsigned blocks, hipStream_t stream, const rppsb::Args& a) {
  with_store_check(store, check, [&](auto st, auto ck) {
    hipLaunchKernelGGL((rppsb::steer_fill<KIND, decltype(st)::value, decltype(ck)::value>), dim3(blocks), dim3(rppsb::TPB), 0, stream, a);
  });
}

// how a fill launch of `s` tests its points: the object's list and, where it serves the list, the index, into a
int steer_check_mode(const rrtx_steer* s, int64_t n_obs, rppsb::Args& a) {
  if (n_obs <= 0) return rppsb::CHECK_NONE;
  if (!s->oi.used) return rppsb::CHECK_LINEAR;
  a.omap = s->oi.map();
  return rppsb::CHECK_INDEX;
}

// One solve, its arguments already checked by its entry point
struct SteerJob {
  const char* fn;
  int kind;   // rppsb::KIND_*
  int32_t product;
  int64_t n, ng;
  const double *starts, *goals;   // rows of 3 (x, y, yaw); LQR: rows of 2
  const double* curvature;        // not LQR
  int32_t curvature_per_pair;
  double step_size;               // LQR: 0 = the raw rollout
  const int32_t* word_order;
  int32_t n_words, want_points;
  double max_time, goal_dist;     // LQR
};
}  // namespace

extern "C" {

int rrtx_steer_create(int32_t device, rrtx_steer** out) { return create_object(device, out, "rrtx_steer_create"); }
void rrtx_steer_destroy(rrtx_steer* s) { destroy_object(s); }
const char* rrtx_steer_last_error(rrtx_steer* s) { return last_error_of(s); }

static int steer_run(rrtx_steer* s, const SteerJob& j);

// What rrtx_steer_solve and rrtx_steer_solve_all check of their arguments, before any HIP call; max_words: the longest word
// list the entry point takes
static int steer_check(rrtx_steer* s, const char* fn, int32_t kind, int32_t product, int64_t n, int64_t ng, const double* starts,
                       const double* goals, const double* curvature, int32_t curvature_per_pair, double step_size,
                       const int32_t* word_order, int32_t n_words, int32_t max_words) {
  auto bad = [&](const char* m) { return fail(s, RRTX_E_INVALID, std::string(fn) + m); };
  if (!s) return bad("the steer object is NULL");
  if (kind != RRTX_STEER_DUBINS && kind != RRTX_STEER_RS) return bad("unknown kind");
  if (!starts || !goals || !curvature) return bad("starts, goals or curvature is NULL");
  if (n < 0 || (product && ng < 0)) return bad("a negative batch size");
  if (!(step_size > 0.0)) return bad("step_size must be > 0");
  if (kind == RRTX_STEER_DUBINS && step_size != rpp::kDubinsStep)
    return bad("Dubins curves are interpolated at the reference's default step_size = 0.1; another step is not supported");
  if (word_order) {
    if (kind != RRTX_STEER_DUBINS) return bad("a word order applies to Dubins curves only");
    if (n_words < 0 || n_words > max_words) return bad(max_words == 6 ? "n_words outside 0..6" : "n_words outside 0..16");
    for (int i = 0; i < n_words; i++)
      if (word_order[i] < 0 || word_order[i] > 5) return bad("a word index outside 0..5");
  }
  const int64_t n_goals = product ? ng : n;
  if (n > (1LL << 30) || n_goals > (1LL << 30) || (product && n && ng && n > (1LL << 30) / ng))
    return bad("more than 2^30 pairs");
  const int64_t np = product ? n * ng : n;
  // Every pose and curvature is looked at once here: a curve's point count grows with distance x curvature / step, and the
  // kernels count points in loops, so an absurd input must never reach them.
  double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
  for (int side = 0; side < 2; side++) {
    const double* q = side ? goals : starts;
    const int64_t rows = side ? n_goals : n;
    for (int64_t i = 0; i < rows; i++)
      for (int c = 0; c < 3; c++) {
        const double v = q[3 * i + c];
        if (!(fabs(v) <= 1e6)) return bad("a pose component is not finite or exceeds 1e6 in magnitude");
        if (c < 2) {
          lo[c] = v < lo[c] ? v : lo[c];
          hi[c] = v > hi[c] ? v : hi[c];
        }
      }
  }
  double cmin = 1e300, cmax = 0.0;
  const int64_t nc = curvature_per_pair ? np : 1;
  for (int64_t i = 0; i < nc; i++) {
    const double c = curvature[i];
    if (!(c > 0.0) || !(c <= 1e300)) return bad("a curvature is not finite or not > 0");
    cmin = c < cmin ? c : cmin;
    cmax = c > cmax ? c : cmax;
  }
  if (np > 0) {
    const double D = hypot(hi[0] - lo[0], hi[1] - lo[1]);
    const double pts = kind == RRTX_STEER_DUBINS ? (D * cmax + 20.0) / rpp::kDubinsStep
                                                 : D / step_size + 20.0 / (step_size * cmin);
    if (!(pts <= 4194304.0)) return bad("the poses are so far apart for this curvature and step that a curve could exceed 2^22 points");
  }
  return RRTX_OK;
}

static int steer_solve(rrtx_steer* s, int32_t kind, int32_t product, int64_t n, int64_t ng, const double* starts,
                       const double* goals, const double* curvature, int32_t curvature_per_pair, double step_size,
                       const int32_t* word_order, int32_t n_words, int32_t want_points) {
  const char* fn = "rrtx_steer_solve: ";
  if (int rc = steer_check(s, fn, kind, product, n, ng, starts, goals, curvature, curvature_per_pair, step_size, word_order,
                           n_words, 6))
    return rc;
  const SteerJob job = {fn, kind, product, n, ng, starts, goals, curvature, curvature_per_pair, step_size, word_order, n_words,
                        want_points, 0.0, 0.0};
  return steer_run(s, job);
}

// What every solve does once its arguments are checked: buffers, stage 1, the prefix sum, stage 2.
static int steer_run(rrtx_steer* s, const SteerJob& j) {
  const char* fn = j.fn;
  const int kind = j.kind;
  const bool lqr = kind == rppsb::KIND_LQR;
  const int32_t product = j.product, want_points = j.want_points;
  const int64_t n = j.n, ng = j.ng, n_goals = product ? ng : n, np = product ? n * ng : n;
  const int64_t nc = lqr ? 0 : (j.curvature_per_pair ? np : 1);
  const size_t row = sizeof(double) * (lqr ? 2 : 3);
  const double *starts = j.starts, *goals = j.goals, *curvature = j.curvature;
  if (int nd = s->need_device(fn)) return nd;
  // With an obstacle list the curves' points are computed (stage 1 as for points, then the fill kernel) whether or not
  // they are stored.
  const int64_t n_obs = (int64_t)(s->h_obs.size() / 3);
  const bool stage2 = want_points || n_obs > 0;

  s->solved = false;
  s->has_points = false;
  s->has_hits = false;
  s->has_k = false;
  s->cand_solved = false;   // the inputs the candidates point into are overwritten
  s->kind = kind;
  s->n = np;
  s->n_points = 0;
  s->kernel_ms = 0.0;
  s->h_offsets.clear();
  if (np == 0) {
    s->has_points = want_points != 0;
    s->has_hits = n_obs > 0;
    s->h_offsets.assign(1, 0);
    s->solved = true;
    return RRTX_OK;
  }
  HIPCHK(s, hipSetDevice(s->device));
  int rc;
  const size_t N = (size_t)np;
  if ((rc = s->reserve(s->starts, row * (size_t)n))) return rc;
  if ((rc = s->reserve(s->goals, row * (size_t)n_goals))) return rc;
  if ((rc = s->reserve(s->status, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->nseg, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->total, sizeof(double) * N))) return rc;
  if (lqr) {   // no curvature, segments or modes; and no stage-2 record: a pair's two points are the record
    if ((rc = s->reserve(s->ends, sizeof(double) * 2 * N))) return rc;
  } else {
    if ((rc = s->reserve(s->curv, sizeof(double) * (size_t)nc))) return rc;
    if ((rc = s->reserve(s->seglen, sizeof(double) * 5 * N))) return rc;
    if ((rc = s->reserve(s->modes, 8 * N))) return rc;
  }
  if ((rc = s->reserve(s->npts, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->flag, sizeof(int32_t)))) return rc;
  if (stage2) {
    const size_t rec = kind == rppsb::KIND_DUBINS ? sizeof(rpp::DubinsPlan) : sizeof(rpp::RsCourse);
    if (!lqr && (rc = s->reserve(s->plan, rec * N))) return rc;
    if ((rc = s->reserve(s->offsets, sizeof(int64_t) * (N + 1)))) return rc;
  }
  if (n_obs > 0) {
    if ((rc = s->reserve(s->hit, sizeof(int32_t) * N))) return rc;
    if (s->obs_dirty) {
      if ((rc = s->reserve(s->obs, sizeof(double) * s->h_obs.size()))) return rc;
      HIPCHK(s, hipMemcpyAsync(s->obs.p, s->h_obs.data(), sizeof(double) * s->h_obs.size(), hipMemcpyHostToDevice, s->stream));
      s->obs_dirty = false;
    }
  }
  HIPCHK(s, hipMemcpyAsync(s->starts.p, starts, row * (size_t)n, hipMemcpyHostToDevice, s->stream));
  HIPCHK(s, hipMemcpyAsync(s->goals.p, goals, row * (size_t)n_goals, hipMemcpyHostToDevice, s->stream));
  if (!lqr) HIPCHK(s, hipMemcpyAsync(s->curv.p, curvature, sizeof(double) * (size_t)nc, hipMemcpyHostToDevice, s->stream));
  HIPCHK(s, hipMemsetAsync(s->flag.p, 0, sizeof(int32_t), s->stream));

  rppsb::Args a;
  memset(&a, 0, sizeof(a));
  a.starts = s->starts.as<const double>();
  a.goals = s->goals.as<const double>();
  if (lqr) {
    a.max_time = j.max_time;
    a.goal_dist = j.goal_dist;
    a.nt = j.step_size > 0.0 ? rpp::lqr_nt(j.step_size) : 0;
    a.ends = s->ends.as<double>();
  } else {
    a.curv = j.curvature_per_pair ? s->curv.as<const double>() : nullptr;
    a.curv0 = curvature[0];
  }
  a.step = j.step_size;
  a.n = np;
  a.ng = product ? ng : 1;
  a.product = product ? 1 : 0;
  a.want_points = stage2 ? 1 : 0;
  a.n_order = j.word_order ? j.n_words : 6;
  for (int i = 0; i < 6; i++) a.order[i] = (j.word_order && i < j.n_words) ? j.word_order[i] : i;
  a.status = s->status.as<int32_t>();
  a.nseg = s->nseg.as<int32_t>();
  a.total = s->total.as<double>();
  a.seglen = s->seglen.as<double>();
  a.modes = s->modes.as<char>();
  a.npts = s->npts.as<int32_t>();
  a.dplan = s->plan.as<rpp::DubinsPlan>();
  a.course = s->plan.as<rpp::RsCourse>();
  a.flag = s->flag.as<int32_t>();
  if (n_obs > 0) {
    a.obs = s->obs.as<const double>();
    a.n_obs = n_obs;
    a.hit = s->hit.as<int32_t>();
  }

  // stage 1
  const unsigned blk = (unsigned)((np + rppsb::TPB - 1) / rppsb::TPB);
  int32_t flag = 0;
  std::vector<int32_t> cnt(stage2 ? N : 0);
  float ms = 0.f;
  rc = s->timed(&ms, [&] {
    if (lqr) {
      hipLaunchKernelGGL(rppsb::steer_lqr_solve, dim3(blk), dim3(rppsb::TPB), 0, s->stream, a);
    } else if (kind == rppsb::KIND_DUBINS) {
      hipLaunchKernelGGL(rppsb::steer_dubins_solve, dim3(blk), dim3(rppsb::TPB), 0, s->stream, a);
    } else {
      hipLaunchKernelGGL(rppsb::steer_rs_solve, dim3((unsigned)((np + rppsb::RS_PAIRS - 1) / rppsb::RS_PAIRS)),
                         dim3(rppsb::RS_TPB), 0, s->stream, a);
      if (stage2) hipLaunchKernelGGL(rppsb::steer_rs_course, dim3(blk), dim3(rppsb::TPB), 0, s->stream, a);
    }
  }, [&]() -> int {
    HIPCHK(s, hipMemcpyAsync(&flag, s->flag.p, sizeof(flag), hipMemcpyDeviceToHost, s->stream));
    if (stage2) HIPCHK(s, hipMemcpyAsync(cnt.data(), s->npts.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  s->kernel_ms = ms;

  if (stage2) {
    // offsets: exclusive prefix sum of the point counts
    s->h_offsets.resize(N + 1);
    int64_t tot = 0;
    for (size_t i = 0; i < N; i++) {
      s->h_offsets[i] = tot;
      tot += cnt[i] > 0 ? cnt[i] : 0;
    }
    s->h_offsets[N] = tot;
    s->n_points = want_points ? tot : 0;
    if (tot > 0) {
      if (want_points) {
        if ((rc = s->reserve(s->px, sizeof(double) * (size_t)tot))) return rc;
        if ((rc = s->reserve(s->py, sizeof(double) * (size_t)tot))) return rc;
        if (!lqr && (rc = s->reserve(s->pyaw, sizeof(double) * (size_t)tot))) return rc;
      }
      if ((tot + rppsb::TPB - 1) / rppsb::TPB > 0x7fffffffLL)
        return fail(s, RRTX_E_OVERFLOW, std::string(fn) + "more polyline points than one launch can fill");
      HIPCHK(s, hipMemcpyAsync(s->offsets.p, s->h_offsets.data(), sizeof(int64_t) * (N + 1), hipMemcpyHostToDevice, s->stream));
      a.offsets = s->offsets.as<const int64_t>();
      if (want_points) {
        a.px = s->px.as<double>();
        a.py = s->py.as<double>();
        a.pyaw = lqr ? nullptr : s->pyaw.as<double>();
      }
      const unsigned fblk = (unsigned)((tot + rppsb::TPB - 1) / rppsb::TPB);
      rc = s->timed(&ms, [&] {
        if (lqr)
          steer_launch_fill<rppsb::KIND_LQR>(want_points != 0, steer_check_mode(s, n_obs, a), fblk, s->stream, a);
        else if (kind == rppsb::KIND_DUBINS)
          steer_launch_fill<rppsb::KIND_DUBINS>(want_points != 0, steer_check_mode(s, n_obs, a), fblk, s->stream, a);
        else
          steer_launch_fill<rppsb::KIND_RS>(want_points != 0, steer_check_mode(s, n_obs, a), fblk, s->stream, a);
      });
      if (rc) return rc;
      s->kernel_ms += ms;
    }
    if (!want_points) s->h_offsets.clear();   // a lengths-only solve keeps no offsets, checked or not
    s->has_points = want_points != 0;
  }
  s->has_hits = n_obs > 0;
  s->solved = true;
  if (flag) {
    s->err = std::string(fn) + "some pairs have no path or are cases where the reference raises (see the status column)";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

static int steer_solve_lqr(rrtx_steer* s, int32_t product, int64_t n, int64_t ng, const double* starts, const double* goals,
                           double step_size, double max_time, double goal_dist, int32_t want_points) {
  const char* fn = "rrtx_steer_solve_lqr: ";
  auto bad = [&](const char* m) { return fail(s, RRTX_E_INVALID, std::string(fn) + m); };
  if (!s) return bad("the steer object is NULL");
  if (!starts || !goals) return bad("starts or goals is NULL");
  if (n < 0 || (product && ng < 0)) return bad("a negative batch size");
  const int64_t n_goals = product ? ng : n;
  if (n > (1LL << 30) || n_goals > (1LL << 30) || (product && n && ng && n > (1LL << 30) / ng))
    return bad("more than 2^30 pairs");
  for (int side = 0; side < 2; side++) {
    const double* q = side ? goals : starts;
    const int64_t vals = 2 * (side ? n_goals : n);
    for (int64_t i = 0; i < vals; i++)
      if (!(fabs(q[i]) <= 1e6)) return bad("a coordinate is not finite or exceeds 1e6 in magnitude");
  }
  // a segment is resampled at ceil(1 / step_size) parameters: the bound keeps it at <= 1000 points
  if (!(step_size >= 0.0) || (step_size > 0.0 && step_size < 1e-3))
    return bad("step_size must be 0 (the raw rollout) or >= 1e-3");
  // the rollout loop runs while time <= max_time: the reference's 100.0 bounds it at 1001 steps
  if (!(max_time >= 0.0 && max_time <= rpp::kLqrMaxTime)) return bad("max_time must lie in 0 .. 100");
  if (goal_dist != goal_dist) return bad("goal_dist is NaN");   // a negative one is legal: no rollout ever arrives
  const SteerJob job = {fn, rppsb::KIND_LQR, product, n, ng, starts, goals, nullptr, 0, step_size, nullptr, 0, want_points,
                        max_time, goal_dist};
  return steer_run(s, job);
}

int rrtx_steer_solve(rrtx_steer* s, int32_t kind, int32_t product, int64_t n, int64_t ng, const double* starts,
                     const double* goals, const double* curvature, int32_t curvature_per_pair, double step_size,
                     const int32_t* word_order, int32_t n_words, int32_t want_points) {
  return guarded(s, "rrtx_steer_solve", [&] {
    return new_generation(s, steer_solve(s, kind, product, n, ng, starts, goals, curvature, curvature_per_pair, step_size,
                                         word_order, n_words, want_points));
  }, [&] { if (s) s->solved = false; });
}

int rrtx_steer_solve_lqr(rrtx_steer* s, int32_t product, int64_t n, int64_t ng, const double* starts, const double* goals,
                         double step_size, double max_time, double goal_dist, int32_t want_points) {
  return guarded(s, "rrtx_steer_solve_lqr", [&] {
    return new_generation(s, steer_solve_lqr(s, product, n, ng, starts, goals, step_size, max_time, goal_dist, want_points));
  }, [&] { if (s) s->solved = false; });
}

// ---- Bezier ---------------------------------------------------------------------------------------------------------
namespace {
struct BezierJob {
  const char* fn;
  int32_t product;
  int64_t n, ng;
  const double *starts, *goals;   // rows (x, y, yaw); nullptr with control points
  double offset0;
  const double* offsets;          // one per pair, or nullptr: offset0
  const double* cp;               // (n, m, 2), or nullptr with poses
  int32_t m, n_points, want_points, want_curvature;
};
}  // namespace

// The weight table and stage 1, then stage 2 over offsets[p] = p * n_points
static int steer_run_bezier(rrtx_steer* s, const BezierJob& j) {
  const char* fn = j.fn;
  const int64_t n_goals = j.product ? j.ng : j.n, np = j.product ? j.n * j.ng : j.n;
  const int32_t m = j.m, n_points = j.n_points;
  if (int nd = s->need_device(fn)) return nd;
  const int64_t n_obs = (int64_t)(s->h_obs.size() / 3);
  const bool want_points = j.want_points != 0, want_k = j.want_curvature != 0, stage2 = want_points || n_obs > 0;

  s->solved = false;
  s->has_points = false;
  s->has_hits = false;
  s->has_k = false;
  s->cand_solved = false;   // the inputs the candidates point into are overwritten
  s->kind = rppsb::KIND_BEZIER;
  s->bez_m = m;
  s->n = np;
  s->n_points = 0;
  s->kernel_ms = 0.0;
  s->h_offsets.clear();
  if (np == 0) {
    s->has_points = want_points;
    s->has_hits = n_obs > 0;
    s->has_k = want_k;
    s->h_offsets.assign(1, 0);
    s->solved = true;
    return RRTX_OK;
  }
  HIPCHK(s, hipSetDevice(s->device));
  int rc;
  const size_t N = (size_t)np, row = (size_t)rpp::bezier_row_len(m);
  const int64_t tot = np * (int64_t)n_points;   // <= 2^28
  if ((rc = s->reserve(s->status, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->nseg, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->total, sizeof(double) * N))) return rc;
  if ((rc = s->reserve(s->npts, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->bez_cp, sizeof(double) * 2 * (size_t)m * N))) return rc;
  if ((rc = s->reserve(s->bez_w, sizeof(double) * row * (size_t)n_points))) return rc;
  if (want_k && (rc = s->reserve(s->kmax, sizeof(double) * N))) return rc;
  if (n_obs > 0) {
    if ((rc = s->reserve(s->hit, sizeof(int32_t) * N))) return rc;
    if (s->obs_dirty) {
      if ((rc = s->upload(s->obs, s->h_obs.data(), sizeof(double) * s->h_obs.size()))) return rc;
      s->obs_dirty = false;
    }
  }
  if (j.cp) {
    if ((rc = s->upload(s->bez_cp, j.cp, sizeof(double) * 2 * (size_t)m * N))) return rc;
  } else {
    if ((rc = s->upload(s->starts, j.starts, sizeof(double) * 3 * (size_t)j.n))) return rc;
    if ((rc = s->upload(s->goals, j.goals, sizeof(double) * 3 * (size_t)n_goals))) return rc;
    if (j.offsets && (rc = s->upload(s->curv, j.offsets, sizeof(double) * N))) return rc;
  }

  rppsb::Args a;
  memset(&a, 0, sizeof(a));
  a.starts = s->starts.as<const double>();
  a.goals = s->goals.as<const double>();
  a.curv = j.offsets ? s->curv.as<const double>() : nullptr;
  a.curv0 = j.offset0;
  a.n = np;
  a.ng = j.product ? j.ng : 1;
  a.product = j.product ? 1 : 0;
  a.want_points = stage2 ? 1 : 0;
  a.status = s->status.as<int32_t>();
  a.nseg = s->nseg.as<int32_t>();
  a.total = s->total.as<double>();
  a.npts = s->npts.as<int32_t>();
  a.bez_w = s->bez_w.as<const double>();
  a.bez_cp = s->bez_cp.as<double>();
  a.kmax = want_k ? s->kmax.as<double>() : nullptr;
  a.bez_m = m;
  a.bez_np = n_points;
  a.bez_given = j.cp ? 1 : 0;
  if (n_obs > 0) {
    a.obs = s->obs.as<const double>();
    a.n_obs = n_obs;
    a.hit = s->hit.as<int32_t>();
  }

  const unsigned blk = (unsigned)((np + rppsb::TPB - 1) / rppsb::TPB);
  const unsigned wblk = (unsigned)(((size_t)n_points * row + rppsb::TPB - 1) / rppsb::TPB);
  float ms = 0.f;
  rc = s->timed(&ms, [&] {
    hipLaunchKernelGGL(rppsb::bezier_weights_kernel, dim3(wblk), dim3(rppsb::TPB), 0, s->stream, s->bez_w.as<double>(),
                       n_points, m);
    if (m == 4)
      hipLaunchKernelGGL(rppsb::steer_bezier_solve<4>, dim3(blk), dim3(rppsb::TPB), 0, s->stream, a);
    else
      hipLaunchKernelGGL(rppsb::steer_bezier_solve<0>, dim3(blk), dim3(rppsb::TPB), 0, s->stream, a);
  });
  if (rc) return rc;
  s->kernel_ms = ms;

  if (stage2) {
    s->h_offsets.resize(N + 1);
    for (size_t i = 0; i <= N; i++) s->h_offsets[i] = (int64_t)i * n_points;   // every curve has n_points points
    s->n_points = want_points ? tot : 0;
    if (want_points) {
      if ((rc = s->reserve(s->px, sizeof(double) * (size_t)tot))) return rc;
      if ((rc = s->reserve(s->py, sizeof(double) * (size_t)tot))) return rc;
      if ((rc = s->reserve(s->pyaw, sizeof(double) * (size_t)tot))) return rc;
      if (want_k && (rc = s->reserve(s->pk, sizeof(double) * (size_t)tot))) return rc;
      a.px = s->px.as<double>();
      a.py = s->py.as<double>();
      a.pyaw = s->pyaw.as<double>();
      a.pk = want_k ? s->pk.as<double>() : nullptr;
    }
    if ((rc = s->upload(s->offsets, s->h_offsets.data(), sizeof(int64_t) * (N + 1)))) return rc;
    a.offsets = s->offsets.as<const int64_t>();
    const unsigned fblk = (unsigned)((tot + rppsb::TPB - 1) / rppsb::TPB);
    rc = s->timed(&ms, [&] { steer_launch_fill<rppsb::KIND_BEZIER>(want_points, steer_check_mode(s, n_obs, a), fblk, s->stream, a); });
    if (rc) return rc;
    s->kernel_ms += ms;
    if (!want_points) s->h_offsets.clear();
    s->has_points = want_points;
  }
  s->has_hits = n_obs > 0;
  s->has_k = want_k;
  s->solved = true;
  return RRTX_OK;
}

// what both Bezier entry points check of their shared arguments; nullptr: fine
static const char* bezier_shape_bad(int64_t np, int32_t n_points) {
  if (n_points < 2 || n_points > rpp::kBezierMaxPoints) return "n_points outside 2..4096";
  if (np > (1LL << 28) / n_points) return "more than 2^28 points (n * n_points)";
  return nullptr;
}

static int steer_solve_bezier(rrtx_steer* s, int32_t product, int64_t n, int64_t ng, const double* starts,
                              const double* goals, double offset0, const double* offsets, int32_t n_points,
                              int32_t want_points, int32_t want_curvature) {
  const char* fn = "rrtx_steer_solve_bezier: ";
  auto bad = [&](const char* m) { return fail(s, RRTX_E_INVALID, std::string(fn) + m); };
  if (!s) return bad("the steer object is NULL");
  if (!starts || !goals) return bad("starts or goals is NULL");
  if (n < 0 || (product && ng < 0)) return bad("a negative batch size");
  const int64_t n_goals = product ? ng : n;
  if (n > (1LL << 30) || n_goals > (1LL << 30) || (product && n && ng && n > (1LL << 30) / ng))
    return bad("more than 2^30 pairs");
  const int64_t np = product ? n * ng : n;
  if (const char* m = bezier_shape_bad(np, n_points)) return bad(m);
  for (int side = 0; side < 2; side++) {
    const double* q = side ? goals : starts;
    const int64_t vals = 3 * (side ? n_goals : n);
    for (int64_t i = 0; i < vals; i++)
      if (!(fabs(q[i]) <= 1e6)) return bad("a pose component is not finite or exceeds 1e6 in magnitude");
  }
  // dist = hypot / offset: a negative offset is legal in the reference (the control points move the other way)
  const int64_t no = offsets ? np : 1;
  for (int64_t i = 0; i < no; i++) {
    const double o = offsets ? offsets[i] : offset0;
    if (!std::isfinite(o) || fabs(o) < 1e-6) return bad("an offset is not finite or smaller than 1e-6 in magnitude");
  }
  const BezierJob job = {fn, product, n, ng, starts, goals, offset0, offsets, nullptr, 4, n_points, want_points, want_curvature};
  return steer_run_bezier(s, job);
}

static int steer_solve_bezier_cp(rrtx_steer* s, int64_t n, int32_t m, const double* control_points, int32_t n_points,
                                 int32_t want_points, int32_t want_curvature) {
  const char* fn = "rrtx_steer_solve_bezier_cp: ";
  auto bad = [&](const char* msg) { return fail(s, RRTX_E_INVALID, std::string(fn) + msg); };
  if (!s) return bad("the steer object is NULL");
  if (!control_points) return bad("control_points is NULL");
  if (n < 0) return bad("a negative batch size");
  if (n > (1LL << 30)) return bad("more than 2^30 curves");
  if (m < rpp::kBezierMinCp || m > rpp::kBezierMaxCp) return bad("m (control points per curve) outside 3..16");
  if (const char* msg = bezier_shape_bad(n, n_points)) return bad(msg);
  for (int64_t i = 0; i < 2 * (int64_t)m * n; i++)
    if (!(fabs(control_points[i]) <= 1e6)) return bad("a coordinate is not finite or exceeds 1e6 in magnitude");
  const BezierJob job = {fn, 0, n, 0, nullptr, nullptr, 0.0, nullptr, control_points, m, n_points, want_points, want_curvature};
  return steer_run_bezier(s, job);
}

int rrtx_steer_solve_bezier(rrtx_steer* s, int32_t product, int64_t n, int64_t ng, const double* starts, const double* goals,
                            double offset0, const double* offsets, int32_t n_points, int32_t want_points,
                            int32_t want_curvature) {
  return guarded(s, "rrtx_steer_solve_bezier", [&] {
    return new_generation(s, steer_solve_bezier(s, product, n, ng, starts, goals, offset0, offsets, n_points, want_points,
                                                want_curvature));
  }, [&] { if (s) s->solved = false; });
}

int rrtx_steer_solve_bezier_cp(rrtx_steer* s, int64_t n, int32_t m, const double* control_points, int32_t n_points,
                               int32_t want_points, int32_t want_curvature) {
  return guarded(s, "rrtx_steer_solve_bezier_cp", [&] {
    return new_generation(s, steer_solve_bezier_cp(s, n, m, control_points, n_points, want_points, want_curvature));
  }, [&] { if (s) s->solved = false; });
}

int rrtx_steer_get_curvature(rrtx_steer* s, double* k, int64_t cap) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_curvature: the steer object is NULL");
  if (!s->solved || s->kind != rppsb::KIND_BEZIER || !s->has_k || !s->has_points)
    return fail(s, RRTX_E_STATE, "rrtx_steer_get_curvature: no completed Bezier solve with points and curvature");
  if (cap < s->n_points) return fail(s, RRTX_E_CAPACITY, "rrtx_steer_get_curvature: the buffer is too small");
  if (s->n_points == 0) return RRTX_OK;
  if (!k) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_curvature: k is NULL");
  return s->fetch(k, s->pk.p, sizeof(double) * (size_t)s->n_points);
}

int rrtx_steer_get_kmax(rrtx_steer* s, double* kmax) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_kmax: the steer object is NULL");
  if (!s->solved || s->kind != rppsb::KIND_BEZIER || !s->has_k)
    return fail(s, RRTX_E_STATE, "rrtx_steer_get_kmax: no completed Bezier solve with curvature");
  if (s->n == 0) return RRTX_OK;
  if (!kmax) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_kmax: kmax is NULL");
  return s->fetch(kmax, s->kmax.p, sizeof(double) * (size_t)s->n);
}

int rrtx_steer_get_control_points(rrtx_steer* s, double* control_points, int32_t* m) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_control_points: the steer object is NULL");
  if (!s->solved || s->kind != rppsb::KIND_BEZIER)
    return fail(s, RRTX_E_STATE, "rrtx_steer_get_control_points: no completed Bezier solve");
  if (m) *m = s->bez_m;
  if (s->n == 0 || !control_points) return RRTX_OK;
  return s->fetch(control_points, s->bez_cp.p, sizeof(double) * 2 * (size_t)s->bez_m * (size_t)s->n);
}

int rrtx_steer_get_ends(rrtx_steer* s, double* ends) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_ends: the steer object is NULL");
  if (!s->solved) return fail(s, RRTX_E_STATE, "rrtx_steer_get_ends: no completed solve");
  if (s->kind != rppsb::KIND_LQR) return fail(s, RRTX_E_STATE, "rrtx_steer_get_ends: the last solve was not an LQR solve");
  if (s->n == 0) return RRTX_OK;
  if (!ends) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_ends: ends is NULL");
  return s->fetch(ends, s->ends.p, sizeof(double) * 2 * (size_t)s->n);
}

int rrtx_steer_get_counts(rrtx_steer* s, int64_t* n_pairs, int64_t* n_points) {
  if (!s || !n_pairs || !n_points) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_counts: a NULL pointer");
  if (!s->solved) return fail(s, RRTX_E_STATE, "rrtx_steer_get_counts: no completed solve");
  *n_pairs = s->n;
  *n_points = s->n_points;
  return RRTX_OK;
}

int rrtx_steer_get_summary(rrtx_steer* s, int32_t* status, double* length, int32_t* n_seg, double* seg_len, char* modes,
                           int64_t* offsets) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_summary: the steer object is NULL");
  if (!s->solved) return fail(s, RRTX_E_STATE, "rrtx_steer_get_summary: no completed solve");
  if (offsets && !s->has_points)
    return fail(s, RRTX_E_STATE, "rrtx_steer_get_summary: the last solve was lengths-only, it has no offsets");
  if (offsets) memcpy(offsets, s->h_offsets.data(), sizeof(int64_t) * s->h_offsets.size());
  if (s->n == 0) return RRTX_OK;
  const size_t N = (size_t)s->n;
  int rc;
  if (status && (rc = s->fetch(status, s->status.p, sizeof(int32_t) * N))) return rc;
  if (length && (rc = s->fetch(length, s->total.p, sizeof(double) * N))) return rc;
  if (n_seg && (rc = s->fetch(n_seg, s->nseg.p, sizeof(int32_t) * N))) return rc;
  if (s->kind == rppsb::KIND_LQR || s->kind == rppsb::KIND_BEZIER) {   // a rollout or a Bezier curve has neither: zero-filled
    if (seg_len) memset(seg_len, 0, sizeof(double) * 5 * N);
    if (modes) memset(modes, 0, 8 * N);
    return RRTX_OK;
  }
  if (seg_len && (rc = s->fetch(seg_len, s->seglen.p, sizeof(double) * 5 * N))) return rc;
  if (modes && (rc = s->fetch(modes, s->modes.p, 8 * N))) return rc;
  return RRTX_OK;
}

int rrtx_steer_get_points(rrtx_steer* s, double* x, double* y, double* yaw, int64_t cap) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_points: the steer object is NULL");
  if (!s->solved || !s->has_points) return fail(s, RRTX_E_STATE, "rrtx_steer_get_points: no completed solve with points");
  if (yaw && s->kind == rppsb::KIND_LQR) return fail(s, RRTX_E_STATE, "rrtx_steer_get_points: an LQR rollout has no yaw, pass NULL");
  if (cap < s->n_points) return fail(s, RRTX_E_CAPACITY, "rrtx_steer_get_points: the buffers are too small");
  if (s->n_points == 0) return RRTX_OK;
  const size_t bytes = sizeof(double) * (size_t)s->n_points;
  int rc;
  if (x && (rc = s->fetch(x, s->px.p, bytes))) return rc;
  if (y && (rc = s->fetch(y, s->py.p, bytes))) return rc;
  if (yaw && (rc = s->fetch(yaw, s->pyaw.p, bytes))) return rc;
  return RRTX_OK;
}

int rrtx_steer_set_obstacles(rrtx_steer* s, const double* obstacles, int64_t m, double robot_radius) {
  const char* fn = "rrtx_steer_set_obstacles: ";
  auto bad = [&](const char* msg) { return fail(s, RRTX_E_INVALID, std::string(fn) + msg); };
  if (!s) return bad("the steer object is NULL");
  static const ObsListText text = {"a negative obstacle count", "more than 2^20 obstacles", "obstacles is NULL",
                                   "an obstacle entry is not finite", "robot_radius is not finite"};
  if (const char* e = obstacle_list_shape_error(obstacles, m, 1LL << 20, text)) return bad(e);
  if (const char* e = obstacle_list_value_error(obstacles, m, &robot_radius, 1, text, true)) return bad(e);
  return guarded(s, "rrtx_steer_set_obstacles", [&] {
    std::vector<double> t;
    pack_obstacle_rows(obstacles, m, robot_radius, t);   // (size+robot_radius)**2  rrt_05:1635
    s->h_obs.swap(t);
    s->obs_dirty = true;
    return obsindex_set_list(s, s->oi, obstacles, m, robot_radius);
  });
}

int rrtx_steer_set_obstacle_index(rrtx_steer* s, int32_t mode) {
  return obsindex_set_mode(s, s ? &s->oi : nullptr, mode, "rrtx_steer_set_obstacle_index: ", true);
}

int rrtx_steer_get_obstacle_index_info(rrtx_steer* s, rrtx_obstacle_index_info* info) {
  return obsindex_get_info(s, s ? &s->oi : nullptr, info, "rrtx_steer_get_obstacle_index_info: ");
}

int rrtx_steer_get_obstacle_index(rrtx_steer* s, int32_t* cell_start, rrtx_obstacle_item* items, int64_t cap_items,
                                  rrtx_obstacle_item* wide, int64_t cap_wide) {
  const char* fn = "rrtx_steer_get_obstacle_index: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the steer object is NULL");
  if (!s->oi.used) return fail(s, RRTX_E_STATE, std::string(fn) + "the obstacle index does not serve the object's list");
  return obstacle_grid_fetch(s, s->oi.grid, fn, cell_start, items, cap_items, wide, cap_wide);
}

int rrtx_steer_get_hits(rrtx_steer* s, int32_t* hit) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_hits: the steer object is NULL");
  if (!s->solved) return fail(s, RRTX_E_STATE, "rrtx_steer_get_hits: no completed solve");
  if (!s->has_hits) return fail(s, RRTX_E_STATE, "rrtx_steer_get_hits: the last solve ran without an obstacle list");
  if (s->n == 0) return RRTX_OK;
  if (!hit) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_hits: hit is NULL");
  return s->fetch(hit, s->hit.p, sizeof(int32_t) * (size_t)s->n);
}

// ---- every candidate curve of a pair, and the shortest one that is free ----------------------------------------------------
// exclusive prefix sum of counts (negative ones count as none) into off[0 .. n]; returns the total
static int64_t steer_prefix(const std::vector<int32_t>& cnt, std::vector<int64_t>& off) {
  off.resize(cnt.size() + 1);
  int64_t tot = 0;
  for (size_t i = 0; i < cnt.size(); i++) {
    off[i] = tot;
    tot += cnt[i] > 0 ? cnt[i] : 0;
  }
  off[cnt.size()] = tot;
  return tot;
}

static int steer_solve_all(rrtx_steer* s, int32_t kind, int32_t product, int64_t n, int64_t ng, const double* starts,
                           const double* goals, const double* curvature, int32_t curvature_per_pair, double step_size,
                           const int32_t* word_order, int32_t n_words, int32_t want_points) {
  const char* fn = "rrtx_steer_solve_all: ";
  if (int rc = steer_check(s, fn, kind, product, n, ng, starts, goals, curvature, curvature_per_pair, step_size, word_order,
                           n_words, rppsb::CAND_MAX_WORDS))
    return rc;
  if (int nd = s->need_device(fn)) return nd;
  const int64_t n_goals = product ? ng : n, np = product ? n * ng : n;
  const int64_t nc = curvature_per_pair ? np : 1;
  const int64_t n_obs = (int64_t)(s->h_obs.size() / 3);
  const bool stage2 = want_points || n_obs > 0;
  const bool dubins = kind == RRTX_STEER_DUBINS;

  s->solved = false;   // `status` and the inputs are this solve's now
  s->cand_solved = false;
  s->cand_points = want_points != 0;
  s->cand_hits = n_obs > 0;
  s->cand_kind = kind;
  s->cand_flag = 0;
  s->cand_pairs = np;
  s->n_cand = 0;
  s->cand_n_points = 0;
  s->cand_ms = 0.0;
  s->h_cand_off.assign(1, 0);
  s->h_cand_poff.assign(1, 0);
  if (np == 0) {
    s->cand_solved = true;
    return RRTX_OK;
  }
  HIPCHK(s, hipSetDevice(s->device));
  int rc;
  const size_t N = (size_t)np;
  if ((rc = s->reserve(s->status, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->c_ncand, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->c_off, sizeof(int64_t) * (N + 1)))) return rc;
  if ((rc = s->reserve(s->flag, sizeof(int32_t)))) return rc;
  if (n_obs > 0 && s->obs_dirty) {
    if ((rc = s->upload(s->obs, s->h_obs.data(), sizeof(double) * s->h_obs.size()))) return rc;
    s->obs_dirty = false;
  }
  if ((rc = s->upload(s->starts, starts, sizeof(double) * 3 * (size_t)n))) return rc;
  if ((rc = s->upload(s->goals, goals, sizeof(double) * 3 * (size_t)n_goals))) return rc;
  if ((rc = s->upload(s->curv, curvature, sizeof(double) * (size_t)nc))) return rc;
  HIPCHK(s, hipMemsetAsync(s->flag.p, 0, sizeof(int32_t), s->stream));

  rppsb::Args& a = s->cand_args;
  rppsb::CandArgs& c = s->cand_c;
  memset(&a, 0, sizeof(a));
  memset(&c, 0, sizeof(c));
  a.starts = s->starts.as<const double>();
  a.goals = s->goals.as<const double>();
  a.curv = curvature_per_pair ? s->curv.as<const double>() : nullptr;
  a.curv0 = curvature[0];
  a.step = step_size;
  a.ng = product ? ng : 1;
  a.product = product ? 1 : 0;
  a.want_points = stage2 ? 1 : 0;
  a.flag = s->flag.as<int32_t>();
  c.n_pairs = np;
  c.n_order = word_order ? n_words : 6;
  for (int i = 0; i < rppsb::CAND_MAX_WORDS; i++) c.order[i] = (word_order && i < n_words) ? word_order[i] : (i < 6 ? i : 0);
  c.status = s->status.as<int32_t>();
  c.ncand = s->c_ncand.as<int32_t>();

  // count, prefix sum, emit
  const unsigned blk = (unsigned)((np + rppsb::TPB - 1) / rppsb::TPB);
  const unsigned rblk = (unsigned)((np + rppsb::RS_PAIRS - 1) / rppsb::RS_PAIRS);
  std::vector<int32_t> cnt(N);
  int32_t flag = 0;
  float ms = 0.f;
  rc = s->timed(&ms, [&] {
    if (dubins)
      hipLaunchKernelGGL(rppsb::steer_dubins_all<false>, dim3(blk), dim3(rppsb::TPB), 0, s->stream, a, c);
    else
      hipLaunchKernelGGL(rppsb::steer_rs_all<false>, dim3(rblk), dim3(rppsb::RS_TPB), 0, s->stream, a, c);
  }, [&]() -> int {
    HIPCHK(s, hipMemcpyAsync(&flag, s->flag.p, sizeof(flag), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipMemcpyAsync(cnt.data(), s->c_ncand.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  s->cand_ms = ms;
  s->cand_flag = flag;
  const int64_t NC = steer_prefix(cnt, s->h_cand_off);
  if (NC > 0x7fffffffLL) return fail(s, RRTX_E_OVERFLOW, std::string(fn) + "more than 2^31 - 1 candidates");
  s->n_cand = NC;
  s->h_cand_poff.assign((size_t)NC + 1, 0);
  if (NC > 0) {
    const size_t M = (size_t)NC;
    if ((rc = s->upload(s->c_off, s->h_cand_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
    if ((rc = s->reserve(s->c_pair, sizeof(int32_t) * M))) return rc;
    if ((rc = s->reserve(s->c_variant, sizeof(int32_t) * M))) return rc;
    if ((rc = s->reserve(s->c_key, sizeof(double) * M))) return rc;
    if ((rc = s->reserve(s->c_nseg, sizeof(int32_t) * M))) return rc;
    if ((rc = s->reserve(s->c_total, sizeof(double) * M))) return rc;
    if ((rc = s->reserve(s->c_seglen, sizeof(double) * 5 * M))) return rc;
    if ((rc = s->reserve(s->c_modes, 8 * M))) return rc;
    if ((rc = s->reserve(s->c_npts, sizeof(int32_t) * M))) return rc;
    if (n_obs > 0 && (rc = s->reserve(s->c_hit, sizeof(int32_t) * M))) return rc;
    if (stage2) {
      if ((rc = s->reserve(s->c_plan, (dubins ? sizeof(rpp::DubinsPlan) : sizeof(rpp::RsCourse)) * M))) return rc;
      if ((rc = s->reserve(s->c_poff, sizeof(int64_t) * (M + 1)))) return rc;
    }
    c.cand_off = s->c_off.as<const int64_t>();
    c.pair = s->c_pair.as<int32_t>();
    c.variant = s->c_variant.as<int32_t>();
    c.key = s->c_key.as<double>();
    a.n = NC;
    a.cand_pair = s->c_pair.as<const int32_t>();
    a.nseg = s->c_nseg.as<int32_t>();
    a.total = s->c_total.as<double>();
    a.seglen = s->c_seglen.as<double>();
    a.modes = s->c_modes.as<char>();
    a.npts = s->c_npts.as<int32_t>();
    a.dplan = s->c_plan.as<rpp::DubinsPlan>();
    a.course = s->c_plan.as<rpp::RsCourse>();
    if (n_obs > 0) {
      a.obs = s->obs.as<const double>();
      a.n_obs = n_obs;
      a.hit = s->c_hit.as<int32_t>();
    }
    const unsigned cblk = (unsigned)((NC + rppsb::TPB - 1) / rppsb::TPB);
    std::vector<int32_t> pcnt(stage2 ? M : 0);
    rc = s->timed(&ms, [&] {
      if (dubins) {
        hipLaunchKernelGGL(rppsb::steer_dubins_all<true>, dim3(blk), dim3(rppsb::TPB), 0, s->stream, a, c);
      } else {
        hipLaunchKernelGGL(rppsb::steer_rs_all<true>, dim3(rblk), dim3(rppsb::RS_TPB), 0, s->stream, a, c);
        if (stage2) hipLaunchKernelGGL(rppsb::steer_rs_course, dim3(cblk), dim3(rppsb::TPB), 0, s->stream, a);
      }
    }, [&]() -> int {
      if (stage2) HIPCHK(s, hipMemcpyAsync(pcnt.data(), s->c_npts.p, sizeof(int32_t) * M, hipMemcpyDeviceToHost, s->stream));
      return RRTX_OK;
    });
    if (rc) return rc;
    s->cand_ms += ms;
    if (stage2) {
      const int64_t tot = steer_prefix(pcnt, s->h_cand_poff);
      s->cand_n_points = want_points ? tot : 0;
      if (tot > 0) {
        if ((tot + rppsb::TPB - 1) / rppsb::TPB > 0x7fffffffLL)
          return fail(s, RRTX_E_OVERFLOW, std::string(fn) + "more polyline points than one launch can fill");
        if (want_points) {
          if ((rc = s->reserve(s->c_px, sizeof(double) * (size_t)tot))) return rc;
          if ((rc = s->reserve(s->c_py, sizeof(double) * (size_t)tot))) return rc;
          if ((rc = s->reserve(s->c_pyaw, sizeof(double) * (size_t)tot))) return rc;
          if (!dubins && (rc = s->reserve(s->c_pdir, (size_t)tot))) return rc;
          a.px = s->c_px.as<double>();
          a.py = s->c_py.as<double>();
          a.pyaw = s->c_pyaw.as<double>();
          a.pdir = dubins ? nullptr : s->c_pdir.as<int8_t>();
        }
        if ((rc = s->upload(s->c_poff, s->h_cand_poff.data(), sizeof(int64_t) * (M + 1)))) return rc;
        a.offsets = s->c_poff.as<const int64_t>();
        const unsigned fblk = (unsigned)((tot + rppsb::TPB - 1) / rppsb::TPB);
        rc = s->timed(&ms, [&] {
          if (dubins)
            steer_launch_fill<rppsb::KIND_DUBINS>(want_points != 0, steer_check_mode(s, n_obs, a), fblk, s->stream, a);
          else
            steer_launch_fill<rppsb::KIND_RS>(want_points != 0, steer_check_mode(s, n_obs, a), fblk, s->stream, a);
        });
        if (rc) return rc;
        s->cand_ms += ms;
      }
    }
  }
  if (!want_points) s->h_cand_poff.assign(1, 0);   // as a lengths-only solve: no offsets are kept
  s->cand_solved = true;
  if (flag) {
    s->err = std::string(fn) + "some pairs have no candidate: no path, or cases where the reference raises (see the status column)";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

int rrtx_steer_solve_all(rrtx_steer* s, int32_t kind, int32_t product, int64_t n, int64_t ng, const double* starts,
                         const double* goals, const double* curvature, int32_t curvature_per_pair, double step_size,
                         const int32_t* word_order, int32_t n_words, int32_t want_points) {
  return guarded(s, "rrtx_steer_solve_all", [&] {
    return new_generation(s, steer_solve_all(s, kind, product, n, ng, starts, goals, curvature, curvature_per_pair, step_size,
                                             word_order, n_words, want_points));
  }, [&] { if (s) s->cand_solved = false; });
}

int rrtx_steer_get_cand_counts(rrtx_steer* s, int64_t* n_pairs, int64_t* n_candidates, int64_t* n_points, double* kernel_ms) {
  if (!s) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_cand_counts: the steer object is NULL");
  if (!s->cand_solved) return fail(s, RRTX_E_STATE, "rrtx_steer_get_cand_counts: no completed rrtx_steer_solve_all");
  if (n_pairs) *n_pairs = s->cand_pairs;
  if (n_candidates) *n_candidates = s->n_cand;
  if (n_points) *n_points = s->cand_n_points;
  if (kernel_ms) *kernel_ms = s->cand_ms;
  return RRTX_OK;
}

int rrtx_steer_get_cand_summary(rrtx_steer* s, int32_t* status, int64_t* cand_offsets, int32_t* pair, int32_t* variant,
                                int32_t* n_seg, double* seg_len, char* modes, double* length, double* key, int32_t* hit,
                                int64_t* offsets) {
  const char* fn = "rrtx_steer_get_cand_summary: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the steer object is NULL");
  if (!s->cand_solved) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed rrtx_steer_solve_all");
  if (offsets && !s->cand_points) return fail(s, RRTX_E_STATE, std::string(fn) + "the last solve was without points, it has no offsets");
  if (hit && !s->cand_hits) return fail(s, RRTX_E_STATE, std::string(fn) + "the last solve ran without an obstacle list");
  if (cand_offsets) memcpy(cand_offsets, s->h_cand_off.data(), sizeof(int64_t) * s->h_cand_off.size());
  if (offsets) memcpy(offsets, s->h_cand_poff.data(), sizeof(int64_t) * s->h_cand_poff.size());
  if (s->cand_pairs == 0) return RRTX_OK;
  int rc;
  if (status && (rc = s->fetch(status, s->status.p, sizeof(int32_t) * (size_t)s->cand_pairs))) return rc;
  const size_t M = (size_t)s->n_cand;
  if (M == 0) return RRTX_OK;
  if (pair && (rc = s->fetch(pair, s->c_pair.p, sizeof(int32_t) * M))) return rc;
  if (variant && (rc = s->fetch(variant, s->c_variant.p, sizeof(int32_t) * M))) return rc;
  if (n_seg && (rc = s->fetch(n_seg, s->c_nseg.p, sizeof(int32_t) * M))) return rc;
  if (seg_len && (rc = s->fetch(seg_len, s->c_seglen.p, sizeof(double) * 5 * M))) return rc;
  if (modes && (rc = s->fetch(modes, s->c_modes.p, 8 * M))) return rc;
  if (length && (rc = s->fetch(length, s->c_total.p, sizeof(double) * M))) return rc;
  if (key && (rc = s->fetch(key, s->c_key.p, sizeof(double) * M))) return rc;
  if (hit && (rc = s->fetch(hit, s->c_hit.p, sizeof(int32_t) * M))) return rc;
  return RRTX_OK;
}

int rrtx_steer_get_cand_points(rrtx_steer* s, double* x, double* y, double* yaw, int8_t* directions, int64_t cap) {
  const char* fn = "rrtx_steer_get_cand_points: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the steer object is NULL");
  if (!s->cand_solved || !s->cand_points) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed rrtx_steer_solve_all with points");
  if (cap < s->cand_n_points) return fail(s, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  if (s->cand_n_points == 0) return RRTX_OK;
  const size_t cnt = (size_t)s->cand_n_points;
  int rc;
  if (x && (rc = s->fetch(x, s->c_px.p, sizeof(double) * cnt))) return rc;
  if (y && (rc = s->fetch(y, s->c_py.p, sizeof(double) * cnt))) return rc;
  if (yaw && (rc = s->fetch(yaw, s->c_pyaw.p, sizeof(double) * cnt))) return rc;
  if (directions) {
    if (s->cand_kind == RRTX_STEER_DUBINS)
      memset(directions, 1, cnt);   // a Dubins curve is driven forwards throughout
    else if ((rc = s->fetch(directions, s->c_pdir.p, cnt)))
      return rc;
  }
  return RRTX_OK;
}

static int steer_select_free(rrtx_steer* s, int32_t* chosen, int32_t* rank, int32_t* n_free) {
  const char* fn = "rrtx_steer_select_free: ";
  if (!s) return fail(s, RRTX_E_INVALID, std::string(fn) + "the steer object is NULL");
  if (!s->cand_solved) return fail(s, RRTX_E_STATE, std::string(fn) + "no completed rrtx_steer_solve_all");
  if (!s->cand_hits) return fail(s, RRTX_E_STATE, std::string(fn) + "the candidates were solved without an obstacle list");
  const int64_t np = s->cand_pairs;
  const bool want_points = s->cand_points;
  s->solved = false;
  s->has_points = false;
  s->has_hits = false;
  s->has_k = false;
  s->kind = s->cand_kind;
  s->n = np;
  s->n_points = 0;
  s->kernel_ms = s->cand_ms;
  s->h_offsets.clear();
  if (np == 0) {
    s->has_points = want_points;
    s->has_hits = true;
    s->h_offsets.assign(1, 0);
    s->solved = true;
    return RRTX_OK;
  }
  HIPCHK(s, hipSetDevice(s->device));
  int rc;
  const size_t N = (size_t)np;
  if ((rc = s->reserve(s->nseg, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->total, sizeof(double) * N))) return rc;
  if ((rc = s->reserve(s->seglen, sizeof(double) * 5 * N))) return rc;
  if ((rc = s->reserve(s->modes, 8 * N))) return rc;
  if ((rc = s->reserve(s->npts, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->hit, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->c_chosen, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->c_rank, sizeof(int32_t) * N))) return rc;
  if ((rc = s->reserve(s->c_nfree, sizeof(int32_t) * N))) return rc;
  if (s->n_cand == 0 && (rc = s->upload(s->c_off, s->h_cand_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
  rppsb::Args pa;
  memset(&pa, 0, sizeof(pa));
  pa.n = np;
  pa.nseg = s->nseg.as<int32_t>();
  pa.total = s->total.as<double>();
  pa.seglen = s->seglen.as<double>();
  pa.modes = s->modes.as<char>();
  pa.npts = s->npts.as<int32_t>();
  pa.hit = s->hit.as<int32_t>();
  rppsb::CandArgs c = s->cand_c;
  c.cand_off = s->c_off.as<const int64_t>();
  c.chosen = s->c_chosen.as<int32_t>();
  c.rank = s->c_rank.as<int32_t>();
  c.nfree = s->c_nfree.as<int32_t>();
  const rppsb::Args& ca = s->cand_args;
  const unsigned blk = (unsigned)((np + rppsb::TPB - 1) / rppsb::TPB);
  std::vector<int32_t> cnt(want_points ? N : 0);
  float ms = 0.f;
  rc = s->timed(&ms, [&] {
    hipLaunchKernelGGL(rppsb::steer_select_free, dim3(blk), dim3(rppsb::TPB), 0, s->stream, pa, ca, c);
  }, [&]() -> int {
    if (want_points) HIPCHK(s, hipMemcpyAsync(cnt.data(), s->npts.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s->stream));
    if (chosen) HIPCHK(s, hipMemcpyAsync(chosen, s->c_chosen.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s->stream));
    if (rank) HIPCHK(s, hipMemcpyAsync(rank, s->c_rank.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s->stream));
    if (n_free) HIPCHK(s, hipMemcpyAsync(n_free, s->c_nfree.p, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s->stream));
    return RRTX_OK;
  });
  if (rc) return rc;
  s->kernel_ms += ms;
  if (want_points) {
    const int64_t tot = steer_prefix(cnt, s->h_offsets);
    s->n_points = tot;
    if (tot > 0) {
      if ((rc = s->reserve(s->px, sizeof(double) * (size_t)tot))) return rc;
      if ((rc = s->reserve(s->py, sizeof(double) * (size_t)tot))) return rc;
      if ((rc = s->reserve(s->pyaw, sizeof(double) * (size_t)tot))) return rc;
      if ((rc = s->upload(s->offsets, s->h_offsets.data(), sizeof(int64_t) * (N + 1)))) return rc;
      pa.offsets = s->offsets.as<const int64_t>();
      pa.px = s->px.as<double>();
      pa.py = s->py.as<double>();
      pa.pyaw = s->pyaw.as<double>();
      const unsigned fblk = (unsigned)((tot + rppsb::TPB - 1) / rppsb::TPB);   // <= the candidates' fill launch
      rc = s->timed(&ms, [&] {
        hipLaunchKernelGGL(rppsb::steer_gather_points, dim3(fblk), dim3(rppsb::TPB), 0, s->stream, pa, ca, c);
      });
      if (rc) return rc;
      s->kernel_ms += ms;
    }
    s->has_points = true;
  }
  s->has_hits = true;
  s->solved = true;
  if (s->cand_flag) {
    s->err = std::string(fn) + "some pairs have no path or are cases where the reference raises (see the status column)";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

int rrtx_steer_select_free(rrtx_steer* s, int32_t* chosen, int32_t* rank, int32_t* n_free) {
  return guarded(s, "rrtx_steer_select_free", [&] { return new_generation(s, steer_select_free(s, chosen, rank, n_free)); },
                 [&] { if (s) s->solved = false; });
}

int rrtx_steer_get_generation(rrtx_steer* s, uint64_t* generation) {
  if (!s || !generation) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_generation: a NULL pointer");
  *generation = s->generation;
  return RRTX_OK;
}

int rrtx_steer_get_kernel_ms(rrtx_steer* s, double* kernel_ms) {
  if (!s || !kernel_ms) return fail(s, RRTX_E_INVALID, "rrtx_steer_get_kernel_ms: a NULL pointer");
  if (!s->solved) return fail(s, RRTX_E_STATE, "rrtx_steer_get_kernel_ms: no completed solve");
  *kernel_ms = s->kernel_ms;
  return RRTX_OK;
}

}  // extern "C"

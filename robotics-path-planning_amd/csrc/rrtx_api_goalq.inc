// rrtx_api_goalq.inc -- rrtx_query_goals and its getters: the best path to many goals from the finished trees of a
// planned handle (goal_query.hip.h); included by rrtx_api.hip after rrtx_api_courses.inc.
// Per query call: one host -> device copy (the goals), one launch, one device -> host copy (the records).  Per gather:
// two launches, one device -> host copy (the counts) and at most two host -> device copies (the offsets, the pose
// planners' slab pointers); per rrtx_get_goal_courses one copy per column.  None of them depends on the number of
// instances, of goals, or on the depth of a tree.

static const char* const GOALQ_ALGOS_MSG =
    "served for RRTX_ALGO_RRT_STAR (\"rrt_star\"), RRTX_ALGO_DUBINS (\"rrt_star_dubins\") and RRTX_ALGO_RS with the Euclidean "
    "cost (\"rrt_star_reeds_shepp\") only";

static bool goalq_served(const rrtx_handle* h) {
  const int algo = h->p.algo;
  return algo == RRTX_ALGO_RRT_STAR || algo == RRTX_ALGO_DUBINS || (algo == RRTX_ALGO_RS && h->rs_cost == RRTX_RS_COST_EUCLID);
}

// the tree columns and parameters every kernel of a query reads
static void goalq_args(rrtx_handle* h, rppq::QueryArgs& a) {
  const rrtx_handle::GoalQ& Q = h->gq;
  memset(&a, 0, sizeof(a));
  a.c = h->c;
  a.n_inst = h->n_inst;
  a.n_goals = Q.n_goals;
  a.per_instance = Q.per_instance;
  a.kind = h->p.algo == RRTX_ALGO_RRT_STAR ? rppq::KIND_POINT : rppq::KIND_POSE;
  a.goals = Q.goals.as<const double>();
  a.xy_th = Q.xy_th;
  a.yaw_th = Q.yaw_th;
  a.yaw = h->da.yaw;
  a.rec = Q.rec.as<rppq::Record>();
  a.plen = h->da.plen;
  a.poff = h->da.poff;
}

static int query_goals(rrtx_handle* h, int32_t n_goals, int32_t per_instance, const double* goals, double xy_th, double yaw_th) {
  const std::string fn = "rrtx_query_goals: ";
  if (!h) return fail(h, RRTX_E_INVALID, fn + "the handle is NULL");
  if (!goalq_served(h)) return fail(h, RRTX_E_INVALID, fn + GOALQ_ALGOS_MSG);
  if (n_goals < 1) return fail(h, RRTX_E_INVALID, fn + "n_goals < 1");
  if (per_instance != 0 && per_instance != 1) return fail(h, RRTX_E_INVALID, fn + "per_instance is 0 or 1");
  if (!goals) return fail(h, RRTX_E_INVALID, fn + "goals is NULL");
  const int64_t nq = (int64_t)h->n_inst * n_goals;
  if (nq > RRTX_GOALQ_MAX_QUERIES) return fail(h, RRTX_E_INVALID, fn + "more than 2^24 queries (instances x goals)");
  if (int rc = refuse_in_plan(h, "rrtx_query_goals")) return rc;
  if (!h->planned) return fail(h, RRTX_E_STATE, fn + "no completed plan");
  if (int rc = refuse_with_map(h, "rrtx_query_goals")) return rc;
  rrtx_handle::GoalQ& Q = h->gq;
  Q.valid = Q.gathered = false;
  HIPCHK(h, hipSetDevice(h->device));
  Q.n_goals = n_goals;
  Q.per_instance = per_instance;
  Q.xy_th = xy_th == xy_th ? xy_th : h->p.goal_xy_th;       // NaN: the planner's own
  Q.yaw_th = yaw_th == yaw_th ? yaw_th : h->p.goal_yaw_th;
  int rc;
  const size_t rows = (size_t)(per_instance ? nq : n_goals);
  if ((rc = h->upload(Q.goals, goals, sizeof(double) * 3 * rows))) return rc;
  if ((rc = h->reserve(Q.rec, sizeof(rppq::Record) * (size_t)nq))) return rc;
  rppq::QueryArgs a;
  goalq_args(h, a);
  const bool point = a.kind == rppq::KIND_POINT;
  // Resident workgroups loop over the queries.  A point query's workgroup owns one scratch row of `stride` hit slots:
  // at most 4 workgroups per CU, and no more rows than 256 MiB hold
  int64_t grid = point ? 4LL * (h->n_cu > 0 ? h->n_cu : 256) : 16LL * (h->n_cu > 0 ? h->n_cu : 256);
  if (point) {
    const int64_t row_bytes = (int64_t)sizeof(int32_t) * (h->stride > 0 ? h->stride : 1);
    const int64_t fit = (256LL << 20) / row_bytes;
    if (grid > fit) grid = fit > 0 ? fit : 1;
  }
  if (grid > nq) grid = nq;
  if (point) {
    if ((rc = h->reserve(Q.scratch, sizeof(int32_t) * (size_t)grid * (size_t)h->stride))) return rc;
    a.scratch = Q.scratch.as<int32_t>();
  }
  Q.h_rec.resize((size_t)nq);
  float ms = 0.f;
  rc = h->timed(&ms,
                [&] {
                  if (point)
                    hipLaunchKernelGGL(rppq::goal_solve_point_kernel, dim3((unsigned)grid), dim3(rppq::TPB_POINT), 0, h->stream, a);
                  else
                    hipLaunchKernelGGL(rppq::goal_solve_pose_kernel, dim3((unsigned)grid), dim3(rppq::TPB_WAVE), 0, h->stream, a);
                },
                [&]() -> int {
                  HIPCHK(h, hipMemcpyAsync(Q.h_rec.data(), Q.rec.p, sizeof(rppq::Record) * (size_t)nq, hipMemcpyDeviceToHost, h->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;   // the timed section waited: `goals` has been read
  Q.solve_ms = ms;
  Q.gather_ms = 0.0;
  Q.valid = true;
  Q.generation++;
  int64_t over = 0;
  for (const rppq::Record& r : Q.h_rec) over += r.status == rppq::ST_OVERFLOW;
  if (over) {
    h->err = fn + std::to_string(over) + " queries have more than " + std::to_string(rppk::NU_MAX) +
             " distinct candidates (RRTX_GOALQ_OVERFLOW); every other query is answered";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

// the handle holds the answers of a query asked of its current plan
static bool goalq_current(const rrtx_handle* h) { return h->gq.valid && h->planned && h->run.stage == 0; }

static int gather_goal_courses(rrtx_handle* h, int32_t order) {
  const std::string fn = "rrtx_gather_goal_courses: ";
  if (!h) return fail(h, RRTX_E_INVALID, fn + "the handle is NULL");
  if (order != RRTX_ORDER_PLANNING && order != RRTX_ORDER_DRIVING) return fail(h, RRTX_E_INVALID, fn + "unknown order");
  if (int rc = refuse_in_plan(h, "rrtx_gather_goal_courses")) return rc;
  rrtx_handle::GoalQ& Q = h->gq;
  if (!goalq_current(h)) {
    if (Q.generation > 0 && !Q.valid) return fail(h, RRTX_E_INVALID, fn + "the handle has planned again since the query: its answers are gone");
    return fail(h, RRTX_E_STATE, fn + "no rrtx_query_goals on the current plan");
  }
  Q.gathered = false;
  HIPCHK(h, hipSetDevice(h->device));
  const int B = h->n_inst;
  const size_t N = (size_t)B, NQ = N * (size_t)Q.n_goals;
  const bool has_yaw = h->p.algo == RRTX_ALGO_RS;
  int rc;
  rppq::QueryArgs a;
  goalq_args(h, a);
  a.order = order;
  a.ncol = has_yaw ? 3 : 2;
  if (a.kind == rppq::KIND_POSE) {
    // where each instance's polylines live: as rrtx_gather_courses finds them
    std::vector<int64_t> both(4 * N);
    static_assert(sizeof(double*) == sizeof(int64_t), "the slab pointers and capacities share one upload");
    for (int i = 0; i < B; i++) {
      const rrtx_handle::PoolLoc& pl = h->pool_loc[i];
      const double* pp[3] = {pl.at(pl.px), pl.at(pl.py), has_yaw ? pl.at(pl.pyaw) : nullptr};
      memcpy(both.data() + 3 * (size_t)i, pp, sizeof(pp));
      both[3 * N + (size_t)i] = pl.cap;
    }
    if ((rc = h->upload(Q.pool, both.data(), sizeof(int64_t) * both.size()))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));   // `both` is a local
    a.pool = Q.pool.as<const double* const>();
    a.pool_cap = Q.pool.as<const int64_t>() + 3 * N;
  }
  if ((rc = h->reserve(Q.count, sizeof(int32_t) * NQ))) return rc;
  a.count = Q.count.as<int32_t>();

  std::vector<int32_t> cnt(NQ);
  float ms = 0.f;
  rc = h->timed(&ms, [&] { hipLaunchKernelGGL(rppq::goal_count_kernel, dim3((unsigned)((NQ + 255) / 256)), dim3(256), 0, h->stream, a); },
                [&]() -> int {
                  HIPCHK(h, hipMemcpyAsync(cnt.data(), Q.count.p, sizeof(int32_t) * NQ, hipMemcpyDeviceToHost, h->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  Q.gather_ms = ms;
  Q.h_off.assign(NQ + 1, 0);
  int64_t tot = 0;
  for (size_t q = 0; q < NQ; q++) {
    Q.h_off[q] = tot;
    tot += cnt[q];
    if (tot > (1LL << 28)) return fail(h, RRTX_E_CAPACITY, fn + "more than 2^28 points in all");
  }
  Q.h_off[NQ] = tot;
  if (tot > 0) {
    if ((rc = h->upload(Q.off, Q.h_off.data(), sizeof(int64_t) * (NQ + 1)))) return rc;
    if ((rc = h->reserve(Q.x, sizeof(double) * (size_t)tot))) return rc;
    if ((rc = h->reserve(Q.y, sizeof(double) * (size_t)tot))) return rc;
    if (has_yaw && (rc = h->reserve(Q.yaw, sizeof(double) * (size_t)tot))) return rc;
    a.off = Q.off.as<const int64_t>();
    a.ox = Q.x.as<double>();
    a.oy = Q.y.as<double>();
    a.oyaw = has_yaw ? Q.yaw.as<double>() : nullptr;
    int64_t grid = 16LL * (h->n_cu > 0 ? h->n_cu : 256);
    if (grid > (int64_t)NQ) grid = (int64_t)NQ;
    rc = h->timed(&ms, [&] { hipLaunchKernelGGL(rppq::goal_gather_kernel, dim3((unsigned)grid), dim3(rppq::TPB_WAVE), 0, h->stream, a); });
    if (rc) return rc;   // the timed section waited: the offsets have been read
    Q.gather_ms += ms;
  }
  Q.order = order;
  Q.has_yaw = has_yaw;
  Q.n_points = tot;
  Q.gathered = true;
  return RRTX_OK;
}

extern "C" {

int rrtx_query_goals(rrtx_handle* h, int32_t n_goals, int32_t per_instance, const double* goals, double xy_th, double yaw_th) {
  return guarded(h, "rrtx_query_goals", [&] { return query_goals(h, n_goals, per_instance, goals, xy_th, yaw_th); },
                 [&] { if (h) h->gq.valid = false; });
}

int rrtx_get_goal_query(rrtx_handle* h, int32_t* node, double* cost, int32_t* n_near, int32_t* n_safe, int32_t* status,
                        int64_t cap, int64_t* n_queries) {
  const char* fn = "rrtx_get_goal_query: ";
  if (!h) return fail(h, RRTX_E_INVALID, std::string(fn) + "the handle is NULL");
  if (!goalq_current(h)) return fail(h, RRTX_E_STATE, std::string(fn) + "no rrtx_query_goals on the current plan");
  const int64_t nq = (int64_t)h->gq.h_rec.size();
  if (n_queries) *n_queries = nq;
  if (!node && !cost && !n_near && !n_safe && !status) return RRTX_OK;
  if (cap < nq) return fail(h, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  for (int64_t q = 0; q < nq; q++) {
    const rppq::Record& r = h->gq.h_rec[(size_t)q];
    if (node) node[q] = r.node;
    if (cost) cost[q] = r.cost;
    if (n_near) n_near[q] = r.n_near;
    if (n_safe) n_safe[q] = r.n_safe;
    if (status) status[q] = r.status;
  }
  return RRTX_OK;
}

int rrtx_gather_goal_courses(rrtx_handle* h, int32_t order) {
  return guarded(h, "rrtx_gather_goal_courses", [&] { return gather_goal_courses(h, order); }, [&] { if (h) h->gq.gathered = false; });
}

int rrtx_get_goal_course_counts(rrtx_handle* h, int64_t* offsets, int64_t* n_points, int32_t* has_yaw) {
  const char* fn = "rrtx_get_goal_course_counts: ";
  if (!h) return fail(h, RRTX_E_INVALID, std::string(fn) + "the handle is NULL");
  if (!goalq_current(h) || !h->gq.gathered) return fail(h, RRTX_E_STATE, std::string(fn) + "no gathered goal courses of the current plan");
  if (offsets) memcpy(offsets, h->gq.h_off.data(), sizeof(int64_t) * h->gq.h_off.size());
  if (n_points) *n_points = h->gq.n_points;
  if (has_yaw) *has_yaw = h->gq.has_yaw ? 1 : 0;
  return RRTX_OK;
}

int rrtx_get_goal_courses(rrtx_handle* h, double* x, double* y, double* yaw, int64_t cap) {
  const char* fn = "rrtx_get_goal_courses: ";
  if (!h) return fail(h, RRTX_E_INVALID, std::string(fn) + "the handle is NULL");
  if (!goalq_current(h) || !h->gq.gathered) return fail(h, RRTX_E_STATE, std::string(fn) + "no gathered goal courses of the current plan");
  if (yaw && !h->gq.has_yaw) return fail(h, RRTX_E_STATE, std::string(fn) + "the gathered courses have no yaw");
  if (cap < h->gq.n_points) return fail(h, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  if (h->gq.n_points == 0) return RRTX_OK;
  const size_t bytes = sizeof(double) * (size_t)h->gq.n_points;
  int rc;
  if (x && (rc = h->fetch(x, h->gq.x.p, bytes))) return rc;
  if (y && (rc = h->fetch(y, h->gq.y.p, bytes))) return rc;
  if (yaw && (rc = h->fetch(yaw, h->gq.yaw.p, bytes))) return rc;
  return RRTX_OK;
}

int rrtx_get_goal_query_kernel_ms(rrtx_handle* h, double* solve_ms, double* gather_ms) {
  if (!h) return fail(h, RRTX_E_INVALID, "rrtx_get_goal_query_kernel_ms: the handle is NULL");
  if (!goalq_current(h)) return fail(h, RRTX_E_STATE, "rrtx_get_goal_query_kernel_ms: no rrtx_query_goals on the current plan");
  if (solve_ms) *solve_ms = h->gq.solve_ms;
  if (gather_ms) *gather_ms = h->gq.gather_ms;
  return RRTX_OK;
}

}  // extern "C"

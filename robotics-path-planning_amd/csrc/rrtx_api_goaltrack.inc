// rrtx_api_goaltrack.inc -- rrtx_track_goals and its getters: rrt_10's closed-loop stage for many goals from the finished
// trees of a planned handle (goal_track.hip.h); included by rrtx_api.hip after rrtx_api_goalq.inc.
// Per call: one host -> device copy (the goals, with the instances' pool pointers behind them), the count launch and the
// counts copy, the offsets copy, the fill, roll and pick launches and the outcomes copy, and with arrays the array-offsets
// copy and the store launch.  None of them depends on the number of instances, goals, candidates or on the depth of a tree.

static int track_goals(rrtx_handle* h, const rrtx_track_params* tp, int32_t n_goals, int32_t per_instance, const double* goals,
                       int32_t want_arrays) {
  const std::string fn = "rrtx_track_goals: ";
  if (!h) return fail(h, RRTX_E_INVALID, fn + "the handle is NULL");
  if (!tp) return fail(h, RRTX_E_INVALID, fn + "the parameters are NULL");
  if (!goals) return fail(h, RRTX_E_INVALID, fn + "goals is NULL");
  if (n_goals < 1) return fail(h, RRTX_E_INVALID, fn + "n_goals < 1");
  if (per_instance != 0 && per_instance != 1) return fail(h, RRTX_E_INVALID, fn + "per_instance is 0 or 1");
  const int64_t nq = (int64_t)h->n_inst * n_goals;
  if (nq > RRTX_GOALQ_MAX_QUERIES) return fail(h, RRTX_E_INVALID, fn + "more than 2^24 queries (instances x goals)");
  if (!track_params_ok(tp)) return fail(h, RRTX_E_INVALID, fn + TRACK_PARAMS_MSG);
  if (h->p.algo != RRTX_ALGO_RS)
    return fail(h, RRTX_E_STATE, fn + "served for RRTX_ALGO_RS (\"closed_loop_rrt_star\", \"rrt_star_reeds_shepp\") only");
  if (int rc = refuse_in_plan(h, "rrtx_track_goals")) return rc;
  if (!h->planned) return fail(h, RRTX_E_STATE, fn + "no completed plan");
  rrtx_handle::GoalTrack& G = h->gt;
  G.valid = G.has_arrays = false;
  HIPCHK(h, hipSetDevice(h->device));
  const int B = h->n_inst;
  const size_t N = (size_t)B, NQ = (size_t)nq;
  const size_t rows = per_instance ? NQ : (size_t)n_goals;
  int rc;
  // the goals, and behind them where each instance's polylines live (as rrtx_track_planned finds them): one upload
  static_assert(sizeof(double*) == sizeof(double), "the goals and the pool pointers share one upload");
  std::vector<double> both(3 * rows + 3 * N);
  memcpy(both.data(), goals, sizeof(double) * 3 * rows);
  for (int i = 0; i < B; i++) {
    const rrtx_handle::PoolLoc& pl = h->pool_loc[i];
    const double* pp[3] = {pl.at(pl.px), pl.at(pl.py), pl.at(pl.pyaw)};
    memcpy(both.data() + 3 * rows + 3 * (size_t)i, pp, sizeof(pp));
  }
  if ((rc = h->upload(G.goals, both.data(), sizeof(double) * both.size()))) return rc;
  if ((rc = h->reserve(G.count, sizeof(int32_t) * NQ))) return rc;
  if ((rc = h->reserve(G.counters, sizeof(int32_t) * 2))) return rc;
  if ((rc = h->reserve(G.outc, sizeof(rppgt::Outcome) * NQ))) return rc;
  if ((rc = h->reserve(G.win_query, sizeof(int32_t) * NQ))) return rc;
  HIPCHK(h, hipMemsetAsync(G.counters.p, 0, sizeof(int32_t) * 2, h->stream));

  rppgt::GoalTrackArgs a;
  memset(&a, 0, sizeof(a));
  a.inst = h->c.inst;
  a.x = h->c.x;
  a.y = h->c.y;
  a.yaw = h->da.yaw;
  a.parent = h->c.parent;
  a.poff = h->da.poff;
  a.plen = h->da.plen;
  a.stride = h->stride;
  a.pool = (const double* const*)(G.goals.as<const double>() + 3 * rows);
  a.ox = h->c.ox;
  a.oy = h->c.oy;
  a.othr = h->c.othr;
  memcpy(&a.P, tp, sizeof(a.P));
  a.n_inst = B;
  a.n_goals = n_goals;
  a.per_instance = per_instance;
  a.nq = nq;
  a.goals = G.goals.as<const double>();
  a.count = G.count.as<int32_t>();
  a.counters = G.counters.as<int32_t>();
  a.win_query = G.win_query.as<int32_t>();
  a.outc = G.outc.as<rppgt::Outcome>();

  const int64_t resident = 16LL * (h->n_cu > 0 ? h->n_cu : 256);   // one-wave workgroups, 16 per CU
  const unsigned cand_grid = (unsigned)(nq < resident ? nq : resident);
  // ---- count
  std::vector<int32_t> cnt(NQ);
  float ms = 0.f;
  rc = h->timed(&ms, [&] { hipLaunchKernelGGL(rppgt::goal_cand_kernel, dim3(cand_grid), dim3(rppgt::TPB), 0, h->stream, a, 0); },
                [&]() -> int {
                  HIPCHK(h, hipMemcpyAsync(cnt.data(), G.count.p, sizeof(int32_t) * NQ, hipMemcpyDeviceToHost, h->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;   // the timed section waited: `both` has been read
  G.list_ms = ms;
  G.roll_ms = G.store_ms = 0.0;
  G.h_cand_off.assign(NQ + 1, 0);
  const int64_t tot = rppgt::candidate_offsets(cnt.data(), nq, rppgt::MAX_CANDIDATES, G.h_cand_off.data());
  if (tot < 0) return fail(h, RRTX_E_CAPACITY, fn + "more than 2^24 candidates in all");
  if ((rc = h->upload(G.cand_off, G.h_cand_off.data(), sizeof(int64_t) * (NQ + 1)))) return rc;
  a.cand_off = G.cand_off.as<const int64_t>();
  a.n_jobs = (int32_t)tot;
  int roll_blocks = (int)(tot < resident ? tot : resident);
  if (roll_blocks < 1) roll_blocks = 1;
  if (tot > 0) {
    if ((rc = h->reserve(G.cand, sizeof(int32_t) * (size_t)tot))) return rc;
    if ((rc = h->reserve(G.job_query, sizeof(int32_t) * (size_t)tot))) return rc;
    if ((rc = h->reserve(G.rec, sizeof(rppt::Record) * (size_t)tot))) return rc;
    if ((rc = h->reserve(G.slab, sizeof(double) * (size_t)roll_blocks * 3 * rppt::SLAB_PTS))) return rc;
    a.cand = G.cand.as<int32_t>();
    a.job_query = G.job_query.as<int32_t>();
    a.rec = G.rec.as<rppt::Record>();
    a.slab = G.slab.as<double>();
    // ---- fill
    rc = h->timed(&ms, [&] { hipLaunchKernelGGL(rppgt::goal_cand_kernel, dim3(cand_grid), dim3(rppgt::TPB), 0, h->stream, a, 1); });
    if (rc) return rc;
    G.list_ms += ms;
  }
  // ---- roll and pick
  // with an obstacle map every instance's rows are empty: the roll-outs ask the map, whose thr carries robot_radius as the rows do
  const rppo::Map mp = h->om.on ? h->om.grid.map() : rppo::Map{};
  auto roll = [&](int blocks, int store) {
    if (h->om.on)
      hipLaunchKernelGGL((rppgt::goal_roll_kernel<rppt::CHECK_INDEX>), dim3(blocks), dim3(rppgt::TPB), 0, h->stream, a, store, mp);
    else
      hipLaunchKernelGGL((rppgt::goal_roll_kernel<rppt::CHECK_LINEAR>), dim3(blocks), dim3(rppgt::TPB), 0, h->stream, a, store, mp);
  };
  G.h_outc.resize(NQ);
  rc = h->timed(&ms,
                [&] {
                  if (tot > 0) roll(roll_blocks, 0);
                  hipLaunchKernelGGL(rppgt::goal_pick_kernel, dim3((unsigned)((NQ + 255) / 256)), dim3(256), 0, h->stream, a);
                },
                [&]() -> int {
                  HIPCHK(h, hipMemcpyAsync(G.h_outc.data(), G.outc.p, sizeof(rppgt::Outcome) * NQ, hipMemcpyDeviceToHost, h->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;   // the timed section waited: the offsets have been read
  G.roll_ms = ms;
  G.h_arr_off.assign(NQ + 1, 0);
  const int64_t steps = rppgt::array_offsets(G.h_outc.data(), nq, G.h_arr_off.data());
  int64_t winners = 0, refused = 0;
  for (const rppgt::Outcome& o : G.h_outc) {
    winners += o.flag != 0;
    refused += o.status != 0;
  }
  // ---- store: the winners again, their arrays kept
  if (want_arrays && winners > 0) {
    if ((rc = h->reserve(G.out, sizeof(double) * 7 * (size_t)steps))) return rc;
    if ((rc = h->upload(G.arr_off, G.h_arr_off.data(), sizeof(int64_t) * (NQ + 1)))) return rc;
    HIPCHK(h, hipMemsetAsync(G.counters.p, 0, sizeof(int32_t), h->stream));   // the queue head; counters[1] keeps the winners listed
    a.out = G.out.as<double>();
    a.arr_off = G.arr_off.as<const int64_t>();
    a.out_total = steps;
    const int blocks = (int)(winners < roll_blocks ? winners : roll_blocks);
    rc = h->timed(&ms, [&] { roll(blocks, 1); });
    if (rc) return rc;   // the timed section waited: the array offsets have been read
    G.store_ms = ms;
  }
  G.n_goals = n_goals;
  G.n_cand = tot;
  G.n_steps = steps;
  G.has_arrays = want_arrays != 0;
  G.valid = true;
  if (refused) {
    h->err = fn + std::to_string(refused) + " queries have a refused candidate (a course of fewer than 3 points, one longer than " +
             std::to_string(rppt::SLAB_PTS - rppt::EXT_MAX) + " points, or tan outside the replica's domain) and no winner; " +
             "every other query is answered";
    return RRTX_PARTIAL;
  }
  return RRTX_OK;
}

// the handle holds the answers of a call on its current plan
static bool goaltrack_current(const rrtx_handle* h) { return h->gt.valid && h->planned && h->run.stage == 0; }

extern "C" {

int rrtx_track_goals(rrtx_handle* h, const rrtx_track_params* tp, int32_t n_goals, int32_t per_instance, const double* goals,
                     int32_t want_arrays) {
  return guarded(h, "rrtx_track_goals", [&] { return track_goals(h, tp, n_goals, per_instance, goals, want_arrays); },
                 [&] { if (h) h->gt.valid = false; });
}

int rrtx_get_goal_track(rrtx_handle* h, rrtx_goal_track_outcome* out, int64_t* cand_offsets, int64_t* arr_offsets, int64_t cap,
                        int64_t* n_queries, int64_t* n_candidates, int64_t* n_steps) {
  const char* fn = "rrtx_get_goal_track: ";
  if (!h) return fail(h, RRTX_E_INVALID, std::string(fn) + "the handle is NULL");
  if (!goaltrack_current(h)) return fail(h, RRTX_E_STATE, std::string(fn) + "no rrtx_track_goals on the current plan");
  const rrtx_handle::GoalTrack& G = h->gt;
  const int64_t nq = (int64_t)G.h_outc.size();
  if (n_queries) *n_queries = nq;
  if (n_candidates) *n_candidates = G.n_cand;
  if (n_steps) *n_steps = G.n_steps;
  if (!out && !cand_offsets && !arr_offsets) return RRTX_OK;
  if (cap < nq) return fail(h, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  if (out) memcpy(out, G.h_outc.data(), sizeof(rrtx_goal_track_outcome) * (size_t)nq);
  if (cand_offsets) memcpy(cand_offsets, G.h_cand_off.data(), sizeof(int64_t) * ((size_t)nq + 1));
  if (arr_offsets) memcpy(arr_offsets, G.h_arr_off.data(), sizeof(int64_t) * ((size_t)nq + 1));
  return RRTX_OK;
}

int rrtx_get_goal_track_records(rrtx_handle* h, int32_t* cand_node, rrtx_track_record* rec, int64_t cap) {
  const char* fn = "rrtx_get_goal_track_records: ";
  if (!h) return fail(h, RRTX_E_INVALID, std::string(fn) + "the handle is NULL");
  if (!goaltrack_current(h)) return fail(h, RRTX_E_STATE, std::string(fn) + "no rrtx_track_goals on the current plan");
  const int64_t n = h->gt.n_cand;
  if (cap < n) return fail(h, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  if (n == 0) return RRTX_OK;
  int rc;
  if (cand_node && (rc = h->fetch(cand_node, h->gt.cand.p, sizeof(int32_t) * (size_t)n))) return rc;
  if (rec && (rc = h->fetch(rec, h->gt.rec.p, sizeof(rrtx_track_record) * (size_t)n))) return rc;
  return RRTX_OK;
}

int rrtx_get_goal_track_arrays(rrtx_handle* h, double* x, double* y, double* yaw, double* v, double* t, double* a, double* d,
                               int64_t cap) {
  const char* fn = "rrtx_get_goal_track_arrays: ";
  if (!h) return fail(h, RRTX_E_INVALID, std::string(fn) + "the handle is NULL");
  if (!goaltrack_current(h) || !h->gt.has_arrays)
    return fail(h, RRTX_E_STATE, std::string(fn) + "no rrtx_track_goals with arrays on the current plan");
  const int64_t tot = h->gt.n_steps;
  if (cap < tot) return fail(h, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  if (tot == 0) return RRTX_OK;
  double* dst[7] = {x, y, yaw, v, t, a, d};
  for (int k = 0; k < 7; k++)
    if (dst[k])
      if (int rc = h->fetch(dst[k], h->gt.out.as<const double>() + (size_t)k * (size_t)tot, sizeof(double) * (size_t)tot)) return rc;
  return RRTX_OK;
}

int rrtx_get_polyline_yaw(rrtx_handle* h, int32_t instance, double* pyaw, int64_t cap_points) {
  const char* fn = "rrtx_get_polyline_yaw: ";
  if (!h || !pyaw || instance < 0 || instance >= h->n_inst) return fail(h, RRTX_E_INVALID, std::string(fn) + "a NULL pointer or no such instance");
  if (!h->planned || h->p.algo != RRTX_ALGO_RS) return fail(h, RRTX_E_STATE, std::string(fn) + "no completed plan of RRTX_ALGO_RS");
  HIPCHK(h, hipSetDevice(h->device));
  Result r;
  HIPCHK(h, hipMemcpy(&r, h->c.results + instance, sizeof(r), hipMemcpyDeviceToHost));
  const size_t n = (size_t)(r.n_nodes > 0 ? r.n_nodes : 0);
  const int64_t off = (int64_t)instance * h->stride;
  std::vector<int32_t> pl(n);
  std::vector<int64_t> po(n);
  int rc;
  if ((rc = h->fetch(pl.data(), h->da.plen + off, sizeof(int32_t) * n))) return rc;
  if ((rc = h->fetch(po.data(), h->da.poff + off, sizeof(int64_t) * n))) return rc;
  int64_t total = 0, used = 0;
  for (size_t i = 0; i < n; i++) total += pl[i];
  if (cap_points < total) return fail(h, RRTX_E_CAPACITY, std::string(fn) + "the buffer is too small");
  if ((rc = h->fetch(&used, h->da.pool_used + instance, sizeof(int64_t)))) return rc;
  std::vector<double> bw((size_t)(used > 0 ? used : 0));
  const rrtx_handle::PoolLoc& loc = h->pool_loc[instance];
  if ((rc = h->fetch(bw.data(), loc.at(loc.pyaw), sizeof(double) * bw.size()))) return rc;
  int64_t w = 0;
  for (size_t i = 0; i < n; i++)
    for (int q = 0; q < pl[i]; q++) {
      if (po[i] + q >= (int64_t)bw.size()) return fail(h, RRTX_E_STATE, std::string(fn) + "a polyline lies outside the pool");
      pyaw[w++] = bw[(size_t)(po[i] + q)];
    }
  return RRTX_OK;
}

int rrtx_get_goal_track_kernel_ms(rrtx_handle* h, double* list_ms, double* roll_ms, double* store_ms) {
  if (!h) return fail(h, RRTX_E_INVALID, "rrtx_get_goal_track_kernel_ms: the handle is NULL");
  if (!goaltrack_current(h)) return fail(h, RRTX_E_STATE, "rrtx_get_goal_track_kernel_ms: no rrtx_track_goals on the current plan");
  if (list_ms) *list_ms = h->gt.list_ms;
  if (roll_ms) *roll_ms = h->gt.roll_ms;
  if (store_ms) *store_ms = h->gt.store_ms;
  return RRTX_OK;
}

}  // extern "C"

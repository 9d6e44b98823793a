// rrtx_api_armnav.inc -- rrtx_armnav_*: batched joint-space occupancy grids of a planar arm and greedy best-first searches on
// them (armnav_batch.hip.h: armnav_trig_kernel, armnav_grid_kernel, armnav_search_kernel); included by rrtx_api.hip
struct rrtx_armnav : DevObj {
  // device buffers, grown on demand
  DevBuf link_off, link_len, obs_off, obs_xyr, trig, grids, scene, start, goal, rec, pool, cursor, marks;
  // the grids a search runs on: the shape is kept from the moment its arguments were accepted, the bytes are on the
  // device once has_grids is set
  int32_t M = 0;
  int64_t n_scenes = 0;
  bool has_grids = false;
  // the last search
  bool ran = false, has_marks = false;
  int32_t ran_M = 0;
  int64_t n = 0, n_cells = 0, pool_cap = 0;
  double grid_ms = 0.0, search_ms = 0.0;
  std::vector<rppan::Rec> h_rec;
};

static_assert(rpp::kArmMinM == RRTX_ARMNAV_MIN_M && rpp::kArmMaxM == RRTX_ARMNAV_MAX_M, "the grid limits of the header are the kernel's");
static_assert(rpp::kArmMaxLinks == RRTX_ARMNAV_MAX_LINKS && rpp::kArmMaxCircles == RRTX_ARMNAV_MAX_CIRCLES, "the scene limits of the header are the kernel's");
static_assert(rpp::kArmRoute == RRTX_ARMNAV_ROUTE && rpp::kArmNoRoute == RRTX_ARMNAV_NO_ROUTE, "the statuses of the header are the kernel's");

// M and n_scenes of a call that brings grids; nullptr when they are legal
static const char* armnav_shape_msg(int32_t M, int64_t n_scenes) {
  if (M < RRTX_ARMNAV_MIN_M || M > RRTX_ARMNAV_MAX_M) return "M is outside 2..128";
  if (n_scenes < 1 || n_scenes > RRTX_ARMNAV_MAX_CELLS / ((int64_t)M * M)) return "n_scenes is below 1, or scenes x M^2 is above 2^28";
  return nullptr;
}

static int armnav_occupancy(rrtx_armnav* a, int32_t M, int64_t n_scenes, const int64_t* link_off, const double* link_len,
                            const int64_t* obs_off, const double* obs_xyr) {
  const char* fn = "rrtx_armnav_occupancy: ";
  auto bad = [&](const char* m) { return fail(a, RRTX_E_INVALID, std::string(fn) + m); };
  if (!a) return bad("the arm navigation object is NULL");
  if (const char* m = armnav_shape_msg(M, n_scenes)) return bad(m);
  if (!link_off || !link_len || !obs_off) return bad("link_off, link_len or obs_off is NULL");
  if (!csr_ok(link_off, n_scenes) || !csr_ok(obs_off, n_scenes)) return bad("offsets do not start at 0 or decrease");
  for (int64_t s = 0; s < n_scenes; s++) {
    const int64_t nl = link_off[s + 1] - link_off[s], nc = obs_off[s + 1] - obs_off[s];
    if (nl < 1 || nl > RRTX_ARMNAV_MAX_LINKS) return bad("a scene with fewer than 1 or more than 16 links");
    if (nc > RRTX_ARMNAV_MAX_CIRCLES) return bad("a scene with more than 1024 circles");
  }
  const int64_t NL = link_off[n_scenes], NC = obs_off[n_scenes];
  if (NC > 0 && !obs_xyr) return bad("obs_xyr is NULL");
  for (int64_t k = 0; k < NL; k++)
    if (!std::isfinite(link_len[k]) || link_len[k] == 0.0 || std::fabs(link_len[k]) > 1.0e6)
      return bad("a link length is not finite, zero (the reference divides by it) or above 1e6 in magnitude");
  if (!all_finite(obs_xyr, 3 * NC)) return bad("a circle entry is not finite");
  for (int64_t k = 0; k < NC; k++)
    if (obs_xyr[3 * k + 2] < 0.0) return bad("a circle of negative radius");
  a->M = M;
  a->n_scenes = n_scenes;
  a->has_grids = false;
  a->grid_ms = 0.0;
  if (int nd = a->need_device(fn)) return nd;

  HIPCHK(a, hipSetDevice(a->device));
  int rc;
  const size_t S = (size_t)n_scenes, MM = (size_t)M * M;
  if ((rc = a->upload(a->link_off, link_off, sizeof(int64_t) * (S + 1)))) return rc;
  if ((rc = a->upload(a->link_len, link_len, sizeof(double) * (size_t)NL))) return rc;
  if ((rc = a->upload(a->obs_off, obs_off, sizeof(int64_t) * (S + 1)))) return rc;
  if ((rc = a->upload(a->obs_xyr, obs_xyr, sizeof(double) * 3 * (size_t)NC))) return rc;
  if ((rc = a->reserve(a->trig, sizeof(double) * 2 * (size_t)M))) return rc;
  if ((rc = a->reserve(a->grids, S * MM))) return rc;

  rppan::GridArgs g;
  memset(&g, 0, sizeof(g));
  g.M = M;
  g.blocks_per_scene = (int32_t)((MM + rppan::TPB - 1) / rppan::TPB);
  g.link_off = a->link_off.as<const int64_t>();
  g.link_len = a->link_len.as<const double>();
  g.obs_off = a->obs_off.as<const int64_t>();
  g.obs_xyr = a->obs_xyr.as<const double>();
  g.trig = a->trig.as<const double>();
  g.grids = a->grids.as<uint8_t>();
  const unsigned blocks = (unsigned)(S * (size_t)g.blocks_per_scene);   // at most 2^28 / 4
  float ms = 0.f;
  rc = a->timed(&ms, [&] {
    hipLaunchKernelGGL(rppan::armnav_trig_kernel, dim3(1), dim3(rppan::TPB), 0, a->stream, M, a->trig.as<double>());
    hipLaunchKernelGGL(rppan::armnav_grid_kernel, dim3(blocks), dim3(rppan::TPB), 0, a->stream, g);
  });
  if (rc) return rc;
  a->grid_ms = ms;
  a->has_grids = true;
  return RRTX_OK;
}

static int armnav_set_grids(rrtx_armnav* a, int32_t M, int64_t n_scenes, const uint8_t* bytes) {
  const char* fn = "rrtx_armnav_set_grids: ";
  auto bad = [&](const char* m) { return fail(a, RRTX_E_INVALID, std::string(fn) + m); };
  if (!a) return bad("the arm navigation object is NULL");
  if (const char* m = armnav_shape_msg(M, n_scenes)) return bad(m);
  if (!bytes) return bad("bytes is NULL");
  const size_t total = (size_t)n_scenes * (size_t)M * M;
  for (size_t k = 0; k < total; k++)
    if (bytes[k] > 6) return bad("a grid byte above 6");
  a->M = M;
  a->n_scenes = n_scenes;
  a->has_grids = false;
  a->grid_ms = 0.0;
  if (int nd = a->need_device(fn)) return nd;
  HIPCHK(a, hipSetDevice(a->device));
  if (int rc = a->upload(a->grids, bytes, total)) return rc;
  HIPCHK(a, hipStreamSynchronize(a->stream));   // the caller's bytes are free again
  a->has_grids = true;
  return RRTX_OK;
}

static int armnav_search(rrtx_armnav* a, int64_t n, const int32_t* scene, const int32_t* start_ij, const int32_t* goal_ij,
                         int32_t want_marks) {
  const char* fn = "rrtx_armnav_search: ";
  auto bad = [&](const char* m) { return fail(a, RRTX_E_INVALID, std::string(fn) + m); };
  if (!a) return bad("the arm navigation object is NULL");
  if (n < 0 || n > RRTX_ARMNAV_MAX_QUERIES) return bad("n_queries is negative or above 2^20");
  if (n > 0 && (!start_ij || !goal_ij)) return bad("start_ij or goal_ij is NULL");
  if (a->M == 0) return fail(a, RRTX_E_STATE, std::string(fn) + "no grids: call rrtx_armnav_occupancy or rrtx_armnav_set_grids first");
  const int32_t M = a->M;
  for (int64_t k = 0; k < 2 * n; k++)
    if (start_ij[k] < 0 || start_ij[k] >= M || goal_ij[k] < 0 || goal_ij[k] >= M) return bad("a start or goal index outside [0, M)");
  for (int64_t k = 0; scene && k < n; k++)
    if (scene[k] < 0 || scene[k] >= a->n_scenes) return bad("a scene index outside the scenes");
  if (int nd = a->need_device(fn)) return nd;
  if (!a->has_grids) return fail(a, RRTX_E_STATE, std::string(fn) + "the last call that brought grids failed");

  a->ran = false;
  a->has_marks = false;
  a->n = n;
  a->n_cells = 0;
  a->ran_M = M;
  a->search_ms = 0.0;
  a->h_rec.assign((size_t)n, rppan::Rec());
  if (n == 0) {
    a->has_marks = want_marks != 0;
    a->ran = true;
    return RRTX_OK;
  }
  HIPCHK(a, hipSetDevice(a->device));
  int rc;
  const size_t N = (size_t)n, MM = (size_t)M * M;
  if (scene && (rc = a->upload(a->scene, scene, sizeof(int32_t) * N))) return rc;
  if ((rc = a->upload(a->start, start_ij, sizeof(int32_t) * 2 * N))) return rc;
  if ((rc = a->upload(a->goal, goal_ij, sizeof(int32_t) * 2 * N))) return rc;
  if ((rc = a->reserve(a->rec, sizeof(rppan::Rec) * N))) return rc;
  if ((rc = a->reserve(a->cursor, sizeof(unsigned long long)))) return rc;
  if (want_marks && (rc = a->reserve(a->marks, N * MM))) return rc;
  // the route pool: room for 4 M cells per query to begin with, kept from call to call; a batch that asks for more runs
  // a second time with exactly what it asked for
  int64_t cap = std::max<int64_t>(a->pool_cap, std::min<int64_t>(n * 4 * M, n * (int64_t)MM));

  rppan::SearchArgs s;
  memset(&s, 0, sizeof(s));
  s.M = M;
  s.n = n;
  s.grids = a->grids.as<const uint8_t>();
  s.scene = scene ? a->scene.as<const int32_t>() : nullptr;
  s.start = a->start.as<const int32_t>();
  s.goal = a->goal.as<const int32_t>();
  s.rec = a->rec.as<rppan::Rec>();
  s.cursor = a->cursor.as<unsigned long long>();
  s.marks = want_marks ? a->marks.as<uint8_t>() : nullptr;
  for (int pass = 0; pass < 2; pass++) {
    if (cap > a->pool_cap) {
      a->pool_cap = 0;
      if ((rc = a->reserve(a->pool, sizeof(uint16_t) * (size_t)cap))) return rc;
      a->pool_cap = cap;
    }
    s.pool = a->pool.as<uint16_t>();
    s.pool_cap = a->pool_cap;
    unsigned long long asked = 0;
    float ms = 0.f;
    HIPCHK(a, hipMemsetAsync(a->cursor.p, 0, sizeof(unsigned long long), a->stream));
    rc = a->timed(&ms, [&] { hipLaunchKernelGGL(rppan::armnav_search_kernel, dim3((unsigned)n), dim3(rppan::WAVE), 0, a->stream, s); },
                  [&]() -> int {
                    HIPCHK(a, hipMemcpyAsync(&asked, a->cursor.p, sizeof(asked), hipMemcpyDeviceToHost, a->stream));
                    HIPCHK(a, hipMemcpyAsync(a->h_rec.data(), a->rec.p, sizeof(rppan::Rec) * N, hipMemcpyDeviceToHost, a->stream));
                    return RRTX_OK;
                  });
    if (rc) return rc;
    a->search_ms += ms;
    a->n_cells = (int64_t)asked;
    if ((int64_t)asked <= a->pool_cap) break;
    if (pass == 1) return fail(a, RRTX_E_HIP, std::string(fn) + "the second pass asked for more route cells than the first");
    cap = (int64_t)asked;
  }
  a->has_marks = want_marks != 0;
  a->ran = true;
  return RRTX_OK;
}

extern "C" {

int rrtx_armnav_create(int32_t device, rrtx_armnav** out) { return create_object(device, out, "rrtx_armnav_create"); }
void rrtx_armnav_destroy(rrtx_armnav* a) { destroy_object(a); }
const char* rrtx_armnav_last_error(rrtx_armnav* a) { return last_error_of(a); }

int rrtx_armnav_occupancy(rrtx_armnav* a, int32_t M, int64_t n_scenes, const int64_t* link_off, const double* link_len,
                          const int64_t* obs_off, const double* obs_xyr) {
  return guarded(a, "rrtx_armnav_occupancy", [&] { return armnav_occupancy(a, M, n_scenes, link_off, link_len, obs_off, obs_xyr); });
}

int rrtx_armnav_set_grids(rrtx_armnav* a, int32_t M, int64_t n_scenes, const uint8_t* bytes) {
  return guarded(a, "rrtx_armnav_set_grids", [&] { return armnav_set_grids(a, M, n_scenes, bytes); });
}

int rrtx_armnav_get_grids(rrtx_armnav* a, uint8_t* bytes, int64_t cap) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armnav_get_grids: the arm navigation object is NULL");
  if (!a->has_grids) return fail(a, RRTX_E_STATE, "rrtx_armnav_get_grids: no grids on the device");
  const int64_t total = a->n_scenes * (int64_t)a->M * a->M;
  if (!bytes) return fail(a, RRTX_E_INVALID, "rrtx_armnav_get_grids: bytes is NULL");
  if (cap < total) return fail(a, RRTX_E_CAPACITY, "rrtx_armnav_get_grids: the buffer is too small");
  return a->fetch(bytes, a->grids.p, (size_t)total);
}

int rrtx_armnav_search(rrtx_armnav* a, int64_t n_queries, const int32_t* scene, const int32_t* start_ij, const int32_t* goal_ij,
                       int32_t want_marks) {
  const int rc = guarded(a, "rrtx_armnav_search", [&] { return armnav_search(a, n_queries, scene, start_ij, goal_ij, want_marks); });
  if (rc == RRTX_E_HIP && a) a->ran = false;
  return rc;
}

int rrtx_armnav_get_counts(rrtx_armnav* a, int32_t* status, int32_t* n_route, int32_t* pops, int64_t* n_queries, int64_t* n_cells) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armnav_get_counts: the arm navigation object is NULL");
  if (!a->ran) return fail(a, RRTX_E_STATE, "rrtx_armnav_get_counts: no completed search");
  for (int64_t q = 0; q < a->n; q++) {
    const rppan::Rec& r = a->h_rec[(size_t)q];
    if (status) status[q] = r.status;
    if (n_route) n_route[q] = r.n_route;
    if (pops) pops[q] = r.pops;
  }
  if (n_queries) *n_queries = a->n;
  if (n_cells) *n_cells = a->n_cells;
  return RRTX_OK;
}

int rrtx_armnav_get_routes(rrtx_armnav* a, int64_t* offsets, int32_t* cells_ij, int64_t cap) {
  return guarded(a, "rrtx_armnav_get_routes", [&]() -> int {
    if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armnav_get_routes: the arm navigation object is NULL");
    if (!a->ran) return fail(a, RRTX_E_STATE, "rrtx_armnav_get_routes: no completed search");
    if (cells_ij && cap < a->n_cells) return fail(a, RRTX_E_CAPACITY, "rrtx_armnav_get_routes: the buffer is too small");
    std::vector<uint16_t> pool;
    if (cells_ij && a->n_cells > 0) {
      pool.resize((size_t)a->n_cells);
      if (int rc = a->fetch(pool.data(), a->pool.p, sizeof(uint16_t) * pool.size())) return rc;
    }
    // the pool holds the routes in the order the waves finished; the rows go out in query order
    int64_t tot = 0;
    const int32_t M = a->ran_M;
    for (int64_t q = 0; q < a->n; q++) {
      const rppan::Rec& r = a->h_rec[(size_t)q];
      if (offsets) offsets[q] = tot;
      for (int32_t k = 0; cells_ij && k < r.n_route; k++) {
        const int32_t c = pool[(size_t)(r.off + k)];
        cells_ij[2 * (tot + k)] = c / M;
        cells_ij[2 * (tot + k) + 1] = c % M;
      }
      tot += r.n_route;
    }
    if (offsets) offsets[a->n] = tot;
    return RRTX_OK;
  });
}

int rrtx_armnav_get_marks(rrtx_armnav* a, uint8_t* marks, int64_t cap) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armnav_get_marks: the arm navigation object is NULL");
  if (!a->ran) return fail(a, RRTX_E_STATE, "rrtx_armnav_get_marks: no completed search");
  if (!a->has_marks) return fail(a, RRTX_E_STATE, "rrtx_armnav_get_marks: the last search was run with want_marks = 0");
  const int64_t total = a->n * (int64_t)a->ran_M * a->ran_M;
  if (total == 0) return RRTX_OK;
  if (!marks) return fail(a, RRTX_E_INVALID, "rrtx_armnav_get_marks: marks is NULL");
  if (cap < total) return fail(a, RRTX_E_CAPACITY, "rrtx_armnav_get_marks: the buffer is too small");
  return a->fetch(marks, a->marks.p, (size_t)total);
}

int rrtx_armnav_get_kernel_ms(rrtx_armnav* a, double* grid_ms, double* search_ms) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armnav_get_kernel_ms: the arm navigation object is NULL");
  if (grid_ms) *grid_ms = a->grid_ms;
  if (search_ms) *search_ms = a->search_ms;
  return RRTX_OK;
}

}  // extern "C"

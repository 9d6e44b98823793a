// rrtx_api_obsmap.inc -- rrtx_set_obstacle_map and its getters: the uniform grid over a handle's circle list from which
// rppk::rrt_plan_map_kernel refills its obstacle tile (rules: rpp_obsgrid.h, build kernels: obstacle_map.hip.h); included by
// rrtx_api.hip after the planner handle.  The same build (build_obstacle_grid) serves the obstacle index of rrtx_steer,
// rrtx_spline and rrtx_bspline (ObsIndex below; their files are included after this one).
// Per build: one host -> device copy (the circles), three launches with the host's exclusive sum of the per-cell counts
// between the first and the second (one device -> host and one host -> device copy of cells + 2 integers).  None of them
// depends on the number of circles.

// The one build routine, for the planner handle's map and the obstacle index of the curve objects: the grid `g` over the
// circles `in`, on o's device and stream, into `out` -- which is written only when the build is complete, so a failure leaves
// what it held.  run_max > 0: a run (a cell's, or the wide list) of more records than that ends the build after the count
// launch, before the fill and the run^2 sort; *too_long says so and the call returns RRTX_OK with `out` untouched.
static int build_obstacle_grid(DevObj* o, const std::vector<rppo::Circle>& in, const rppo::Geom& g, int64_t run_max, ObsGrid* out,
                               bool* too_long) {
  const int64_t m = (int64_t)in.size();
  const int64_t cells = (int64_t)g.nx * g.ny, runs = cells + 1;   // the last run is the wide list
  if (too_long) *too_long = false;
  HIPCHK(o, hipSetDevice(o->device));
  // The circles, the counts and the unsorted records live for this call only.
  int rc;
  DevBuf f_in, f_count, f_start, f_raw, f_items;
  if ((rc = o->reserve(f_in, sizeof(rppo::Circle) * (size_t)(m > 0 ? m : 1)))) return rc;
  if ((rc = o->reserve(f_count, sizeof(int32_t) * (size_t)runs))) return rc;
  if ((rc = o->reserve(f_start, sizeof(int32_t) * (size_t)(runs + 1)))) return rc;
  if (m > 0) HIPCHK(o, hipMemcpyAsync(f_in.p, in.data(), sizeof(rppo::Circle) * (size_t)m, hipMemcpyHostToDevice, o->stream));
  const rppo::Circle* d_in = f_in.as<const rppo::Circle>();
  int32_t* d_count = f_count.as<int32_t>();
  std::vector<int32_t> count((size_t)runs), start((size_t)runs + 1);
  float ms0 = 0.f, ms1 = 0.f;
  HIPCHK(o, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)runs, o->stream));
  rc = o->timed(&ms0, [&] { hipLaunchKernelGGL(rppom::obsmap_count_kernel, dim3(rppom::BLOCKS), dim3(rppom::TPB), 0, o->stream, d_in, m, g, d_count); },
                [&]() -> int {
                  HIPCHK(o, hipMemcpyAsync(count.data(), d_count, sizeof(int32_t) * (size_t)runs, hipMemcpyDeviceToHost, o->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  int64_t total = 0;
  for (int64_t k = 0; k < runs; k++) {
    if (run_max > 0 && count[k] > run_max) {
      if (too_long) *too_long = true;
      return RRTX_OK;
    }
    start[k] = (int32_t)total;
    total += count[k];
  }
  start[runs] = (int32_t)total;   // at most m * WIDE_CELLS = 2^25 records
  const int64_t n_wide = count[cells], n_items = total - n_wide;
  if ((rc = o->reserve(f_raw, sizeof(rppo::Item) * (size_t)(total > 0 ? total : 1)))) return rc;
  if ((rc = o->reserve(f_items, sizeof(rppo::Item) * (size_t)(total > 0 ? total : 1)))) return rc;
  HIPCHK(o, hipMemcpyAsync(f_start.p, start.data(), sizeof(int32_t) * (size_t)(runs + 1), hipMemcpyHostToDevice, o->stream));
  HIPCHK(o, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)runs, o->stream));   // the fill's cursors
  rc = o->timed(&ms1, [&] {
    hipLaunchKernelGGL(rppom::obsmap_fill_kernel, dim3(rppom::BLOCKS), dim3(rppom::TPB), 0, o->stream, d_in, m, g,
                       f_start.as<const int32_t>(), d_count, f_raw.as<rppo::Item>());
    hipLaunchKernelGGL(rppom::obsmap_sort_kernel, dim3(rppom::BLOCKS), dim3(rppom::TPB), 0, o->stream, runs,
                       f_start.as<const int32_t>(), f_raw.as<const rppo::Item>(), f_items.as<rppo::Item>());
  });
  if (rc) return rc;
  out->cell_start = std::move(f_start);
  out->items = std::move(f_items);
  out->g = g;
  out->m = m;
  out->n_items = n_items;
  out->n_wide = n_wide;
  out->build_ms = (double)ms0 + (double)ms1;
  return RRTX_OK;
}

static void obstacle_grid_info(const ObsGrid& M, rrtx_obstacle_map_info* info) {
  info->x0 = M.g.x0;
  info->y0 = M.g.y0;
  info->cell = M.g.cell;
  info->nx = M.g.nx;
  info->ny = M.g.ny;
  info->n_circles = M.m;
  info->n_items = M.n_items;
  info->n_wide = M.n_wide;
  info->build_ms = M.build_ms;
}

// The grid as built, into the caller's buffers (any may be NULL); `fn`: "rrtx_get_obstacle_map: "
template <class Obj>
static int obstacle_grid_fetch(Obj* o, const ObsGrid& M, const char* fn, int32_t* cell_start, rrtx_obstacle_item* items,
                               int64_t cap_items, rrtx_obstacle_item* wide, int64_t cap_wide) {
  static_assert(sizeof(rrtx_obstacle_item) == sizeof(rppo::Item), "rrtx_obstacle_item mirrors rppo::Item");
  if ((items && cap_items < M.n_items) || (wide && cap_wide < M.n_wide))
    return fail(o, RRTX_E_CAPACITY, std::string(fn) + "the buffers are too small");
  const int64_t cells = (int64_t)M.g.nx * M.g.ny;
  int rc;
  if (cell_start && (rc = o->fetch(cell_start, M.cell_start.p, sizeof(int32_t) * (size_t)(cells + 1)))) return rc;
  if (items && (rc = o->fetch(items, M.items.p, sizeof(rppo::Item) * (size_t)M.n_items))) return rc;
  if (wide && (rc = o->fetch(wide, M.items.as<rppo::Item>() + M.n_items, sizeof(rppo::Item) * (size_t)M.n_wide))) return rc;
  return RRTX_OK;
}

// test knob: cells per axis
static int obsmap_forced_cells() {
  if (const char* e = getenv("RRTX_OBSMAP_CELLS")) return atoi(e) > 0 ? atoi(e) : 0;
  return 0;
}

// ---- the obstacle index of rrtx_steer, rrtx_spline and rrtx_bspline (rules: rpp_obsgrid.h point_first_hit) --------------------
// One list, one robot radius, one mode: whether the index serves them, why not, and the build.  A build is kept for as long
// as the rows, the radius and the cells knob stay what they were.
struct ObsIndex {
  int mode = RRTX_OBSIDX_AUTO;
  int used = 0, reason = RRTX_OBSIDX_REASON_EMPTY;
  std::vector<double> raw;   // the rows (x, y, size) as given
  double radius = 0.0;
  int forced = 0;            // RRTX_OBSMAP_CELLS of the build
  int tried = 0;             // what building for `raw` gave: 0 not tried, else 1 + the reason (USED: `grid` holds it)
  ObsGrid grid;

  rppo::Map map() const { return grid.map(); }
};

// The decision for the list X holds, with a build where the mode wants one and none was tried for this list
static_assert(rppo::IDX_AUTO == RRTX_OBSIDX_AUTO && rppo::IDX_ON == RRTX_OBSIDX_ON && rppo::IDX_OFF == RRTX_OBSIDX_OFF &&
                  rppo::IDX_MIN == RRTX_OBSIDX_MIN && rppo::WHY_USED == RRTX_OBSIDX_REASON_USED &&
                  rppo::WHY_OFF == RRTX_OBSIDX_REASON_OFF && rppo::WHY_BELOW == RRTX_OBSIDX_REASON_BELOW &&
                  rppo::WHY_RUN_TOO_LONG == RRTX_OBSIDX_REASON_RUN_TOO_LONG &&
                  rppo::WHY_NOT_FINITE == RRTX_OBSIDX_REASON_NOT_FINITE && rppo::WHY_EMPTY == RRTX_OBSIDX_REASON_EMPTY,
              "the modes and reasons of the header are the rules'");

static int obsindex_decide(DevObj* o, ObsIndex& X) {
  const int64_t m = (int64_t)(X.raw.size() / 3);
  X.used = 0;
  X.reason = rppo::index_reason(X.mode, m, true, 0);   // what needs no build to know
  if (X.reason != rppo::WHY_USED) return RRTX_OK;
  if (!X.tried) {
    std::vector<rppo::Circle> in((size_t)m);
    std::vector<double> rows;
    pack_obstacle_rows(X.raw.data(), m, X.radius, rows);
    double lo[2] = {X.raw[0], X.raw[1]}, hi[2] = {X.raw[0], X.raw[1]};
    bool finite = true;
    for (int64_t k = 0; k < m; k++) {
      in[k].ox = rows[3 * k];
      in[k].oy = rows[3 * k + 1];
      in[k].thr = rows[3 * k + 2];
      in[k].rho = rppo::reach(X.raw[3 * k + 2], X.radius);
      finite = finite && std::isfinite(in[k].rho) && std::isfinite(in[k].thr);
      lo[0] = in[k].ox < lo[0] ? in[k].ox : lo[0];
      hi[0] = in[k].ox > hi[0] ? in[k].ox : hi[0];
      lo[1] = in[k].oy < lo[1] ? in[k].oy : lo[1];
      hi[1] = in[k].oy > hi[1] ? in[k].oy : hi[1];
    }
    bool too_long = false;
    if (finite) {
      const rppo::Geom g = rppo::geometry_box(lo[0], hi[0], lo[1], hi[1], m, X.forced);
      if (int rc = build_obstacle_grid(o, in, g, rppo::RUN_MAX, &X.grid, &too_long)) return rc;
    }
    X.tried = 1 + rppo::index_reason(rppo::IDX_ON, m, finite, too_long ? (int64_t)rppo::RUN_MAX + 1 : 0);
  }
  X.reason = X.tried - 1;
  X.used = X.reason == rppo::WHY_USED;
  return RRTX_OK;
}

// A (new) list for the object: m rows (x, y, size).  Equal rows, radius and cells knob keep what was built.
static int obsindex_set_list(DevObj* o, ObsIndex& X, const double* oxyr, int64_t m, double radius) {
  const int forced = obsmap_forced_cells();
  const bool same = X.raw.size() == (size_t)(3 * m) && forced == X.forced && memcmp(&radius, &X.radius, sizeof(double)) == 0 &&
                    (m == 0 || memcmp(oxyr, X.raw.data(), sizeof(double) * 3 * (size_t)m) == 0);
  if (!same) {
    X.raw.assign(oxyr, oxyr + 3 * (size_t)m);
    X.radius = radius;
    X.forced = forced;
    X.tried = 0;
  }
  if (!o->usable) return X.used = 0, RRTX_OK;   // no device: the solve answers that
  return obsindex_decide(o, X);
}

template <class Obj>
static int obsindex_set_mode(Obj* o, ObsIndex* X, int32_t mode, const char* fn, bool decide_now) {
  if (!o) return fail(o, RRTX_E_INVALID, std::string(fn) + "the object is NULL");
  if (mode != RRTX_OBSIDX_AUTO && mode != RRTX_OBSIDX_ON && mode != RRTX_OBSIDX_OFF)
    return fail(o, RRTX_E_INVALID, std::string(fn) + "mode is not RRTX_OBSIDX_AUTO, _ON or _OFF");
  X->mode = mode;
  if (!decide_now || !o->usable) return RRTX_OK;
  return guarded(o, fn, [&] { return obsindex_decide(o, *X); });
}

template <class Obj>
static int obsindex_get_info(Obj* o, const ObsIndex* X, rrtx_obstacle_index_info* info, const char* fn) {
  if (!o || !info) return fail(o, RRTX_E_INVALID, std::string(fn) + "a NULL pointer");
  memset(info, 0, sizeof(*info));
  info->mode = X->mode;
  info->used = X->used;
  info->reason = X->reason;
  if (X->used) obstacle_grid_info(X->grid, &info->map);
  return RRTX_OK;
}

static int set_obstacle_map(rrtx_handle* h, const double* oxyr, int64_t m) {
  const std::string fn = "rrtx_set_obstacle_map: ";
  if (!h) return fail(h, RRTX_E_INVALID, fn + "the handle is NULL");
  if (h->p.algo != RRTX_ALGO_RRT && h->p.algo != RRTX_ALGO_RRT_STAR && h->p.algo != RRTX_ALGO_RS)
    return fail(h, RRTX_E_INVALID, fn + "served for RRTX_ALGO_RRT, RRTX_ALGO_RRT_STAR and RRTX_ALGO_RS only (every other planner keeps its obstacle limit)");
  if (m < 0) return fail(h, RRTX_E_INVALID, fn + "m < 0");
  if (m > rppo::M_MAX) return fail(h, RRTX_E_INVALID, fn + "more than 2^20 obstacles");
  if (m > 0 && !oxyr) return fail(h, RRTX_E_INVALID, fn + "oxyr is NULL");
  if (m > 0 && !all_finite(oxyr, 3 * m)) return fail(h, RRTX_E_INVALID, fn + "an obstacle entry is not finite");
  if (int rc = refuse_in_plan(h, "rrtx_set_obstacle_map")) return rc;
  if (int rc = h->need_device("rrtx_set_obstacle_map: ")) return rc;

  rrtx_handle::ObsMapState& M = h->om;
  // test knobs: cells per axis (1: one cell, every box streams the whole list) and records per tile
  int tile = rppk::MAX_OBS;
  const int forced = obsmap_forced_cells();
  if (const char* e = getenv("RRTX_OBSMAP_TILE")) tile = atoi(e) > 0 && atoi(e) < rppk::MAX_OBS ? atoi(e) : rppk::MAX_OBS;
  const rppo::Geom g = rppo::geometry(h->p.rand_min, h->p.rand_max, m, forced);
  std::vector<rppo::Circle> in((size_t)m);
  for (int64_t k = 0; k < m; k++) {
    in[k].ox = oxyr[3 * k];
    in[k].oy = oxyr[3 * k + 1];
    in[k].thr = py_sq_host(oxyr[3 * k + 2] + h->p.robot_radius);   // (size+robot_radius)**2  rrt_04:1227, as obs_upload
    in[k].rho = rppo::reach(oxyr[3 * k + 2], h->p.robot_radius);
    if (!std::isfinite(in[k].rho) || !std::isfinite(in[k].thr))
      return fail(h, RRTX_E_INVALID, fn + "size + robot_radius of an obstacle is not finite");
  }
  // The map is built into buffers of its own and handed to the handle when it is complete: a failure leaves the handle,
  // and the map it may hold, as they were.
  if (int rc = build_obstacle_grid(h, in, g, 0, &M.grid, nullptr)) return rc;
  // built: the handle takes the map, every instance's rows of the table are empty
  M.tile = tile;
  M.on = true;
  for (Inst& I : h->host_inst)
    if (I.obs_base != 0 || I.obs_m != 0) {
      I.obs_base = 0;
      I.obs_m = 0;
      h->inst_dirty = true;
    }
  h->m_max = 0;
  h->obst.assign(oxyr, oxyr + 3 * (size_t)m);
  return RRTX_OK;
}

extern "C" {

int rrtx_set_obstacle_map(rrtx_handle* h, const double* oxyr, int64_t m) {
  return guarded(h, "rrtx_set_obstacle_map", [&] { return set_obstacle_map(h, oxyr, m); });
}

int rrtx_get_obstacle_map_info(rrtx_handle* h, rrtx_obstacle_map_info* info) {
  if (!h || !info) return fail(h, RRTX_E_INVALID, "rrtx_get_obstacle_map_info: a NULL pointer");
  if (!h->om.on) return fail(h, RRTX_E_STATE, "rrtx_get_obstacle_map_info: the handle holds no obstacle map");
  obstacle_grid_info(h->om.grid, info);
  return RRTX_OK;
}

int rrtx_get_obstacle_map(rrtx_handle* h, int32_t* cell_start, rrtx_obstacle_item* items, int64_t cap_items,
                          rrtx_obstacle_item* wide, int64_t cap_wide) {
  if (!h) return fail(h, RRTX_E_INVALID, "rrtx_get_obstacle_map: the handle is NULL");
  if (!h->om.on) return fail(h, RRTX_E_STATE, "rrtx_get_obstacle_map: the handle holds no obstacle map");
  return obstacle_grid_fetch(h, h->om.grid, "rrtx_get_obstacle_map: ", cell_start, items, cap_items, wide, cap_wide);
}

}  // extern "C"

// rrtx_api_obsmap.inc -- rrtx_set_obstacle_map and its getters: the uniform grid over a handle's circle list from which
// rppk::rrt_plan_map_kernel refills its obstacle tile (rules: rpp_obsgrid.h, build kernels: obstacle_map.hip.h); included by
// rrtx_api.hip after the planner handle.
// Per call: one host -> device copy (the circles), three launches with the host's exclusive sum of the per-cell counts
// between the first and the second (one device -> host and one host -> device copy of cells + 2 integers).  None of them
// depends on the number of circles.

static int set_obstacle_map(rrtx_handle* h, const double* oxyr, int64_t m) {
  const std::string fn = "rrtx_set_obstacle_map: ";
  if (!h) return fail(h, RRTX_E_INVALID, fn + "the handle is NULL");
  if (h->p.algo != RRTX_ALGO_RRT && h->p.algo != RRTX_ALGO_RRT_STAR)
    return fail(h, RRTX_E_INVALID, fn + "served for RRTX_ALGO_RRT and RRTX_ALGO_RRT_STAR only (every other planner keeps its obstacle limit)");
  if (m < 0) return fail(h, RRTX_E_INVALID, fn + "m < 0");
  if (m > rppo::M_MAX) return fail(h, RRTX_E_INVALID, fn + "more than 2^20 obstacles");
  if (m > 0 && !oxyr) return fail(h, RRTX_E_INVALID, fn + "oxyr is NULL");
  if (m > 0 && !all_finite(oxyr, 3 * m)) return fail(h, RRTX_E_INVALID, fn + "an obstacle entry is not finite");
  if (int rc = refuse_in_plan(h, "rrtx_set_obstacle_map")) return rc;
  if (int rc = h->need_device("rrtx_set_obstacle_map: ")) return rc;

  rrtx_handle::ObsMapState& M = h->om;
  // test knobs: cells per axis (1: one cell, every box streams the whole list) and records per tile
  int forced = 0, tile = rppk::MAX_OBS;
  if (const char* e = getenv("RRTX_OBSMAP_CELLS")) forced = atoi(e) > 0 ? atoi(e) : 0;
  if (const char* e = getenv("RRTX_OBSMAP_TILE")) tile = atoi(e) > 0 && atoi(e) < rppk::MAX_OBS ? atoi(e) : rppk::MAX_OBS;
  const rppo::Geom g = rppo::geometry(h->p.rand_min, h->p.rand_max, m, forced);
  const int64_t cells = (int64_t)g.nx * g.ny, runs = cells + 1;   // the last run is the wide list
  std::vector<rppo::Circle> in((size_t)m);
  for (int64_t k = 0; k < m; k++) {
    in[k].ox = oxyr[3 * k];
    in[k].oy = oxyr[3 * k + 1];
    in[k].thr = py_sq_host(oxyr[3 * k + 2] + h->p.robot_radius);   // (size+robot_radius)**2  rrt_04:1227, as obs_upload
    in[k].rho = rppo::reach(oxyr[3 * k + 2], h->p.robot_radius);
    if (!std::isfinite(in[k].rho) || !std::isfinite(in[k].thr))
      return fail(h, RRTX_E_INVALID, fn + "size + robot_radius of an obstacle is not finite");
  }
  HIPCHK(h, hipSetDevice(h->device));
  // The map is built into buffers of its own and handed to the handle when it is complete: a failure leaves the handle,
  // and the map it may hold, as they were.  The circles, the counts and the unsorted records live for this call only.
  int rc;
  DevBuf f_in, f_count, f_start, f_raw, f_items;
  if ((rc = h->reserve(f_in, sizeof(rppo::Circle) * (size_t)(m > 0 ? m : 1)))) return rc;
  if ((rc = h->reserve(f_count, sizeof(int32_t) * (size_t)runs))) return rc;
  if ((rc = h->reserve(f_start, sizeof(int32_t) * (size_t)(runs + 1)))) return rc;
  if (m > 0) HIPCHK(h, hipMemcpyAsync(f_in.p, in.data(), sizeof(rppo::Circle) * (size_t)m, hipMemcpyHostToDevice, h->stream));
  const rppo::Circle* d_in = f_in.as<const rppo::Circle>();
  int32_t* d_count = f_count.as<int32_t>();
  std::vector<int32_t> count((size_t)runs), start((size_t)runs + 1);
  float ms0 = 0.f, ms1 = 0.f;
  HIPCHK(h, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)runs, h->stream));
  rc = h->timed(&ms0, [&] { hipLaunchKernelGGL(rppom::obsmap_count_kernel, dim3(rppom::BLOCKS), dim3(rppom::TPB), 0, h->stream, d_in, m, g, d_count); },
                [&]() -> int {
                  HIPCHK(h, hipMemcpyAsync(count.data(), d_count, sizeof(int32_t) * (size_t)runs, hipMemcpyDeviceToHost, h->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  int64_t total = 0;
  for (int64_t k = 0; k < runs; k++) {
    start[k] = (int32_t)total;
    total += count[k];
  }
  start[runs] = (int32_t)total;   // at most m * WIDE_CELLS = 2^25 records
  const int64_t n_wide = count[cells], n_items = total - n_wide;
  if ((rc = h->reserve(f_raw, sizeof(rppo::Item) * (size_t)(total > 0 ? total : 1)))) return rc;
  if ((rc = h->reserve(f_items, sizeof(rppo::Item) * (size_t)(total > 0 ? total : 1)))) return rc;
  HIPCHK(h, hipMemcpyAsync(f_start.p, start.data(), sizeof(int32_t) * (size_t)(runs + 1), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)runs, h->stream));   // the fill's cursors
  rc = h->timed(&ms1, [&] {
    hipLaunchKernelGGL(rppom::obsmap_fill_kernel, dim3(rppom::BLOCKS), dim3(rppom::TPB), 0, h->stream, d_in, m, g,
                       f_start.as<const int32_t>(), d_count, f_raw.as<rppo::Item>());
    hipLaunchKernelGGL(rppom::obsmap_sort_kernel, dim3(rppom::BLOCKS), dim3(rppom::TPB), 0, h->stream, runs,
                       f_start.as<const int32_t>(), f_raw.as<const rppo::Item>(), f_items.as<rppo::Item>());
  });
  if (rc) return rc;
  // built: the handle takes the map, every instance's rows of the table are empty
  M.cell_start = std::move(f_start);
  M.items = std::move(f_items);
  M.g = g;
  M.m = m;
  M.n_items = n_items;
  M.n_wide = n_wide;
  M.tile = tile;
  M.build_ms = (double)ms0 + (double)ms1;
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
  const rrtx_handle::ObsMapState& M = h->om;
  info->x0 = M.g.x0;
  info->y0 = M.g.y0;
  info->cell = M.g.cell;
  info->nx = M.g.nx;
  info->ny = M.g.ny;
  info->n_circles = M.m;
  info->n_items = M.n_items;
  info->n_wide = M.n_wide;
  info->build_ms = M.build_ms;
  return RRTX_OK;
}

int rrtx_get_obstacle_map(rrtx_handle* h, int32_t* cell_start, rrtx_obstacle_item* items, int64_t cap_items,
                          rrtx_obstacle_item* wide, int64_t cap_wide) {
  static_assert(sizeof(rrtx_obstacle_item) == sizeof(rppo::Item), "rrtx_obstacle_item mirrors rppo::Item");
  if (!h) return fail(h, RRTX_E_INVALID, "rrtx_get_obstacle_map: the handle is NULL");
  if (!h->om.on) return fail(h, RRTX_E_STATE, "rrtx_get_obstacle_map: the handle holds no obstacle map");
  const rrtx_handle::ObsMapState& M = h->om;
  if ((items && cap_items < M.n_items) || (wide && cap_wide < M.n_wide))
    return fail(h, RRTX_E_CAPACITY, "rrtx_get_obstacle_map: the buffers are too small");
  const int64_t cells = (int64_t)M.g.nx * M.g.ny;
  int rc;
  if (cell_start && (rc = h->fetch(cell_start, M.cell_start.p, sizeof(int32_t) * (size_t)(cells + 1)))) return rc;
  if (items && (rc = h->fetch(items, M.items.p, sizeof(rppo::Item) * (size_t)M.n_items))) return rc;
  if (wide && (rc = h->fetch(wide, M.items.as<rppo::Item>() + M.n_items, sizeof(rppo::Item) * (size_t)M.n_wide))) return rc;
  return RRTX_OK;
}

}  // extern "C"

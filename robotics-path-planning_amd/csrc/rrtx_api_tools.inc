// rrtx_api_tools.inc -- the calls that take no object: rrtx_smooth_paths, rrtx_selftest_math, rrtx_selfcheck
// (included by rrtx_api.hip).  They run on any device: none of them asks for gfx950.
extern "C" {

int rrtx_smooth_paths(int32_t device, int32_t n_jobs, const double* paths_xy, const int32_t* path_n, int32_t in_stride,
                      int32_t max_iter, const double* obst_xyr, int32_t m, uint32_t* mt_words, int32_t* mt_pos,
                      double* out_xy, int32_t out_stride, int32_t* out_n, int32_t* status) {
  if (n_jobs < 1 || !paths_xy || !path_n || in_stride < 1 || max_iter < 0 || m < 0 || (m && !obst_xyr) || !mt_words ||
      !mt_pos || !out_xy || out_stride < 1 || !out_n || !status || m > rpps::MOB)
    return RRTX_E_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return RRTX_E_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return RRTX_E_HIP;
  std::vector<rpp::MT> rng(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    memcpy(rng[j].mt, mt_words + (size_t)j * 624, 624 * 4);
    rng[j].pos = mt_pos[j];
  }
  std::vector<double> ox(m + 1), oy(m + 1), osz(m + 1);
  for (int k = 0; k < m; k++) {
    ox[k] = obst_xyr[3 * k];
    oy[k] = obst_xyr[3 * k + 1];
    osz[k] = obst_xyr[3 * k + 2];
  }
  const int32_t obs_rows[2] = {0, m};   // every job: rows 0 .. m-1 (obs_stride 0)
  const size_t b_in = sizeof(double) * 2 * (size_t)in_stride * n_jobs, b_out = sizeof(double) * 2 * (size_t)out_stride * n_jobs,
               b_obs = sizeof(double) * (m + 1), b_job = sizeof(int32_t) * n_jobs, b_rng = sizeof(rpp::MT) * n_jobs;
  DevBuf d_in, d_out, d_ox, d_oy, d_osz, d_n, d_on, d_st, d_obs, d_rng;
  const std::pair<DevBuf*, size_t> want[] = {{&d_in, b_in}, {&d_out, b_out}, {&d_ox, b_obs}, {&d_oy, b_obs}, {&d_osz, b_obs},
                                             {&d_n, b_job}, {&d_on, b_job}, {&d_st, b_job}, {&d_obs, sizeof(obs_rows)}, {&d_rng, b_rng}};
  bool ok = true;
  for (const auto& w : want) ok = ok && w.first->reserve(w.second) == hipSuccess;
  std::vector<int32_t> st(n_jobs, 0);
  ok = ok && hipMemcpy(d_in.p, paths_xy, b_in, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_ox.p, ox.data(), b_obs, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_oy.p, oy.data(), b_obs, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_osz.p, osz.data(), b_obs, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_n.p, path_n, b_job, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_obs.p, obs_rows, sizeof(obs_rows), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_rng.p, rng.data(), b_rng, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    rpps::SmoothArgs a{d_in.as<double>(), in_stride, d_n.as<int32_t>(), 1, d_rng.as<rpp::MT>(), (int64_t)sizeof(rpp::MT),
                       d_ox.as<double>(), d_oy.as<double>(), d_osz.as<double>(), d_obs.as<int32_t>(), 0,
                       max_iter, d_out.as<double>(), out_stride, d_on.as<int32_t>(), d_st.as<int32_t>()};
    hipLaunchKernelGGL(rpps::smooth_kernel, dim3(n_jobs), dim3(64), 0, 0, a, n_jobs);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(out_xy, d_out.p, b_out, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(out_n, d_on.p, b_job, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(st.data(), d_st.p, b_job, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(rng.data(), d_rng.p, b_rng, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (!ok) return RRTX_E_HIP;
  for (int j = 0; j < n_jobs; j++) {
    memcpy(mt_words + (size_t)j * 624, rng[j].mt, 624 * 4);
    mt_pos[j] = rng[j].pos;
    status[j] = st[j];
  }
  return smooth_status_rc(st, nullptr);
}

}  // extern "C"

// op 13 of rrtx_selftest_math: one 64-thread workgroup per 64-lane group (n is a multiple of 64: every lane is active)
__global__ __launch_bounds__(64) void selftest_wave_ops_kernel(const double* a, const double* b, double* o, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)64 + threadIdx.x;
  const uint32_t v = (uint32_t)a[i];
  const int idx = (int)b[i];
  const int inc = rppk2t::wave_prefix_sum((int)v);
  uint32_t wv;
  int wi;
  rppk2t::wave_argmin(v, idx, wv, wi);
  o[i] = (double)inc;
  o[n + i] = (double)rppk2t::wave_total(inc);
  o[2 * n + i] = (double)wv;
  o[3 * n + i] = (double)wi;
  o[4 * n + i] = (double)rppk2t::wave_umin(v);
}

extern "C" {

int rrtx_selftest_math(int32_t device, int32_t op, const double* a, const double* b, double* out, int64_t n) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RRTX_E_NO_DEVICE;
  if (!a || !b || !out || n < 0) return RRTX_E_INVALID;
  const bool wave_ops = op == 13;
  if (wave_ops && n % 64 != 0) return RRTX_E_INVALID;
  const int64_t n_out = wave_ops ? 5 * n : n;
  if (hipSetDevice(device) != hipSuccess) return RRTX_E_HIP;
  double *da = nullptr, *db = nullptr, *dout = nullptr;
  int rc = RRTX_OK;
  if (hipMalloc(&da, n * 8) != hipSuccess || hipMalloc(&db, n * 8) != hipSuccess ||
      hipMalloc(&dout, n_out * 8) != hipSuccess)
    rc = RRTX_E_HIP;
  if (!rc && (hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(db, b, n * 8, hipMemcpyHostToDevice) != hipSuccess))
    rc = RRTX_E_HIP;
  if (!rc && wave_ops) {
    if (n > 0) hipLaunchKernelGGL(selftest_wave_ops_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, 0, da, db, dout, n);
    if (hipDeviceSynchronize() != hipSuccess) rc = RRTX_E_HIP;
  } else if (!rc) {
    hipLaunchKernelGGL(rppk::selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, da, db, dout, n);
    if (hipDeviceSynchronize() != hipSuccess) rc = RRTX_E_HIP;
  }
  if (!rc && hipMemcpy(out, dout, n_out * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = RRTX_E_HIP;
  hipFree(da);
  hipFree(db);
  hipFree(dout);
  return rc;
}

int rrtx_selfcheck(int32_t device, int32_t n_per_fn, int64_t* mismatches8) {
  if (!mismatches8 || n_per_fn < 1 || n_per_fn > (1 << 22)) return RRTX_E_INVALID;
  const int64_t n = n_per_fn;
  std::vector<double> a(n), b(n), out(n);
  // splitmix64 -> uniform in [0, 1): the same arguments on every host
  uint64_t sm = 0x9e3779b97f4a7c15ULL;
  auto u01 = [&]() {
    uint64_t z = (sm += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
  };
  // selftest op, argument ranges: coordinates differences up to a few hundred, angles within a few turns (Dubins /
  // Reeds-Shepp sums, 2*pi*a/b of the unit-ball sample), |x| <= 1 for the inverse functions
  struct Fn { int op; double lo_a, hi_a, lo_b, hi_b; } fns[8] = {
      {1, -300.0, 300.0, 0.0, 1.0}, {2, -20.0, 20.0, 0.0, 1.0}, {3, -20.0, 20.0, 0.0, 1.0}, {4, -300.0, 300.0, -300.0, 300.0},
      {8, -1.0, 1.0, 0.0, 1.0},     {9, -1.0, 1.0, 0.0, 1.0},   {6, 0.0, 1.0e5, 0.0, 1.0},  {7, -300.0, 300.0, -300.0, 300.0}};
  for (int f = 0; f < 8; f++) {
    for (int64_t i = 0; i < n; i++) {
      a[i] = fns[f].lo_a + (fns[f].hi_a - fns[f].lo_a) * u01();
      b[i] = fns[f].lo_b + (fns[f].hi_b - fns[f].lo_b) * u01();
      if (i % 7 == 3 && (fns[f].op == 1 || fns[f].op == 4)) a[i] *= 1.0 / 1024.0;   // small arguments too
    }
    int rc = rrtx_selftest_math(device, fns[f].op, a.data(), b.data(), out.data(), n);
    if (rc) return rc;
    int64_t bad = 0;
    for (int64_t i = 0; i < n; i++) {
      double r;
      switch (fns[f].op) {
        case 1: r = py_sq_host(a[i]); break;
        case 2: r = libm_sin(a[i]); break;
        case 3: r = libm_cos(a[i]); break;
        case 4: r = libm_atan2(a[i], b[i]); break;
        case 8: r = libm_acos(a[i]); break;
        case 9: r = libm_asin(a[i]); break;
        case 6: r = libm_sqrt(a[i]); break;
        default: r = a[i] / b[i]; break;
      }
      if (memcmp(&r, &out[i], 8) != 0) bad++;
    }
    mismatches8[f] = bad;
  }
  return RRTX_OK;
}

}  // extern "C"

// rrtx_api_armdh.inc -- rrtx_armdh_*: batched forward kinematics and inverse kinematics of DH arms in 3-D
// (armdh_batch.hip.h: armdh_forward_kernel, armdh_solve_kernel); included by rrtx_api.hip
struct rrtx_armdh : DevObj {
  // device buffers, grown on demand
  DevBuf arm_off, dh, arm, ang_off, ang_in, ref, ang_out, tf, jac, rec;
  // the last run
  int kind = 0;   // 0 none, 1 forward, 2 solve
  int64_t n = 0, n_links = 0;
  int32_t waves = 0;
  double kernel_ms = 0.0;
  std::vector<rppdh::Rec> h_rec;
  std::vector<int64_t> h_ang_off;
};

static_assert(rpp::kDhMaxLinks == RRTX_ARMDH_MAX_LINKS, "the link limit of the header is the kernel's");
static_assert(rpp::kDhOk == RRTX_ARMDH_OK && rpp::kDhNonfinite == RRTX_ARMDH_NONFINITE && rpp::kDhNoConvergence == RRTX_ARMDH_NO_CONVERGENCE,
              "the statuses of the header are the kernel's");
static_assert(rpp::kDhNewton == RRTX_ARMDH_NEWTON && rpp::kDhLm == RRTX_ARMDH_LM, "the methods of the header are the kernel's");
static_assert(sizeof(double) * rpp::kDhLaneDoublesLm * rppdh::WAVE <= 65536, "the per-wave state fits the static LDS of a block");

static bool armdh_all_within(const double* v, int64_t count, double bound) {
  for (int64_t i = 0; i < count; i++)
    if (!std::isfinite(v[i]) || std::fabs(v[i]) > bound) return false;
  return true;
}

// The checks both runs share; fills h_ang_off.  nullptr when the batch is legal
static const char* armdh_batch_msg(rrtx_armdh* a, const rrtx_armdh_batch* b, bool solve) {
  if (!b) return "the batch is NULL";
  if (b->n_arms < 1 || b->n_arms > RRTX_ARMDH_MAX_QUERIES) return "n_arms is below 1 or above 2^20";
  if (!b->link_off || !b->dh) return "link_off or dh is NULL";
  if (!csr_ok(b->link_off, b->n_arms)) return "link_off does not start at 0 or decreases";
  for (int64_t s = 0; s < b->n_arms; s++) {
    const int64_t nl = b->link_off[s + 1] - b->link_off[s];
    if (nl < 1 || nl > RRTX_ARMDH_MAX_LINKS) return "an arm with fewer than 1 or more than 8 links";
  }
  if (!armdh_all_within(b->dh, 4 * b->link_off[b->n_arms], 1.0e6)) return "a DH entry is not finite or above 1e6 in magnitude";
  if (b->n < 0 || b->n > RRTX_ARMDH_MAX_QUERIES) return "n is negative or above 2^20";
  if (b->n > 0 && solve && !b->ref_pose) return "ref_pose is NULL";
  a->h_ang_off.assign((size_t)b->n + 1, 0);
  for (int64_t q = 0; q < b->n; q++) {
    const int64_t s = b->arm ? b->arm[q] : 0;
    if (s < 0 || s >= b->n_arms) return "an arm index outside the arms";
    a->h_ang_off[(size_t)q + 1] = a->h_ang_off[(size_t)q] + (b->link_off[s + 1] - b->link_off[s]);
  }
  if (b->angles && !armdh_all_within(b->angles, a->h_ang_off[(size_t)b->n], 1.0e6)) return "a joint angle is not finite or above 1e6 in magnitude";
  if (solve && !armdh_all_within(b->ref_pose, 6 * b->n, 1.0e6)) return "an entry of ref_pose is not finite or above 1e6 in magnitude";
  return nullptr;
}

// uploads what both runs read and fills the kernel's arguments
static int armdh_stage(rrtx_armdh* a, const rrtx_armdh_batch* b, bool solve, rppdh::Args& k) {
  int rc;
  const size_t N = (size_t)b->n, NL = (size_t)a->h_ang_off[N];
  if ((rc = a->upload(a->arm_off, b->link_off, sizeof(int64_t) * ((size_t)b->n_arms + 1)))) return rc;
  if ((rc = a->upload(a->dh, b->dh, sizeof(double) * 4 * (size_t)b->link_off[b->n_arms]))) return rc;
  if (b->arm && (rc = a->upload(a->arm, b->arm, sizeof(int32_t) * N))) return rc;
  if ((rc = a->upload(a->ang_off, a->h_ang_off.data(), sizeof(int64_t) * (N + 1)))) return rc;
  if (b->angles && (rc = a->upload(a->ang_in, b->angles, sizeof(double) * NL))) return rc;
  if (solve && (rc = a->upload(a->ref, b->ref_pose, sizeof(double) * 6 * N))) return rc;
  if (solve && (rc = a->reserve(a->ang_out, sizeof(double) * NL))) return rc;
  if (!solve && (rc = a->reserve(a->tf, sizeof(double) * 16 * NL))) return rc;
  if (!solve && (rc = a->reserve(a->jac, sizeof(double) * 6 * NL))) return rc;
  if ((rc = a->reserve(a->rec, sizeof(rppdh::Rec) * N))) return rc;
  memset(&k, 0, sizeof(k));
  k.n = b->n;
  k.arm_off = a->arm_off.as<const int64_t>();
  k.dh = a->dh.as<const double>();
  k.arm = b->arm ? a->arm.as<const int32_t>() : nullptr;
  k.ang_off = a->ang_off.as<const int64_t>();
  k.ang_in = b->angles ? a->ang_in.as<const double>() : nullptr;
  k.ref = solve ? a->ref.as<const double>() : nullptr;
  k.ang_out = solve ? a->ang_out.as<double>() : nullptr;
  k.tf = solve ? nullptr : a->tf.as<double>();
  k.jac = solve ? nullptr : a->jac.as<double>();
  k.rec = a->rec.as<rppdh::Rec>();
  return RRTX_OK;
}

static int armdh_run(rrtx_armdh* a, const rrtx_armdh_batch* b, bool solve, int32_t iter_cnt, double step_div, int32_t method, double eps) {
  const char* fn = solve ? "rrtx_armdh_solve: " : "rrtx_armdh_forward: ";
  auto bad = [&](const char* m) { return fail(a, RRTX_E_INVALID, std::string(fn) + m); };
  if (!a) return bad("the DH-arm object is NULL");
  if (const char* m = armdh_batch_msg(a, b, solve)) return bad(m);
  if (solve) {
    if (iter_cnt < 1 || iter_cnt > RRTX_ARMDH_MAX_ITERATIONS) return bad("iter_cnt is outside 1..1e6");
    if (!std::isfinite(step_div) || step_div == 0.0) return bad("step_div is zero or not finite");
    if (method != RRTX_ARMDH_NEWTON && method != RRTX_ARMDH_LM) return bad("method is neither RRTX_ARMDH_NEWTON nor RRTX_ARMDH_LM");
    if (method == RRTX_ARMDH_LM && (!(eps > 0.0) || !std::isfinite(eps))) return bad("eps is not a finite number above 0");
  }
  if (int nd = a->need_device(fn)) return nd;

  a->kind = 0;
  a->n = b->n;
  a->n_links = a->h_ang_off[(size_t)b->n];
  a->waves = 0;
  a->kernel_ms = 0.0;
  a->h_rec.assign((size_t)b->n, rppdh::Rec());
  if (b->n == 0) {
    a->kind = solve ? 2 : 1;
    return RRTX_OK;
  }
  HIPCHK(a, hipSetDevice(a->device));
  rppdh::Args k;
  int rc;
  if ((rc = armdh_stage(a, b, solve, k))) return rc;
  k.iter_cnt = iter_cnt;
  k.step_div = step_div;
  k.eps = eps;
  const size_t N = (size_t)b->n;
  const unsigned blocks = (unsigned)((b->n + rppdh::WAVE - 1) / rppdh::WAVE);
  a->waves = (int32_t)blocks;
  float ms = 0.f;
  rc = a->timed(&ms,
                [&] {
                  if (!solve)
                    hipLaunchKernelGGL(rppdh::armdh_forward_kernel, dim3(blocks), dim3(rppdh::WAVE), 0, a->stream, k);
                  else if (method == RRTX_ARMDH_LM)
                    hipLaunchKernelGGL(rppdh::armdh_solve_kernel<rpp::kDhLm>, dim3(blocks), dim3(rppdh::WAVE), 0, a->stream, k);
                  else
                    hipLaunchKernelGGL(rppdh::armdh_solve_kernel<rpp::kDhNewton>, dim3(blocks), dim3(rppdh::WAVE), 0, a->stream, k);
                },
                [&]() -> int {
                  HIPCHK(a, hipMemcpyAsync(a->h_rec.data(), a->rec.p, sizeof(rppdh::Rec) * N, hipMemcpyDeviceToHost, a->stream));
                  return RRTX_OK;
                });
  if (rc) return rc;
  a->kernel_ms = ms;
  a->kind = solve ? 2 : 1;
  for (const rppdh::Rec& r : a->h_rec)
    if (r.status != RRTX_ARMDH_OK) {
      a->err = std::string(fn) + "some queries left the finite numbers or the domain of sin / cos, or a step did not converge (see the status column)";
      return RRTX_PARTIAL;
    }
  return RRTX_OK;
}

// one device array of the last run into the caller's buffer
static int armdh_fetch(rrtx_armdh* a, const char* fn, int kind, const char* state_msg, DevBuf rrtx_armdh::*src, double* dst, int64_t per_link,
                       int64_t cap) {
  if (!a) return fail(a, RRTX_E_INVALID, std::string(fn) + ": the DH-arm object is NULL");
  if (a->kind != kind) return fail(a, RRTX_E_STATE, std::string(fn) + state_msg);
  const int64_t count = per_link * a->n_links;
  if (dst && count > 0) {
    if (cap < count) return fail(a, RRTX_E_CAPACITY, std::string(fn) + ": the buffer is too small");
    return a->fetch(dst, (a->*src).p, sizeof(double) * (size_t)count);
  }
  return RRTX_OK;
}

extern "C" {

int rrtx_armdh_create(int32_t device, rrtx_armdh** out) { return create_object(device, out, "rrtx_armdh_create"); }
void rrtx_armdh_destroy(rrtx_armdh* a) { destroy_object(a); }
const char* rrtx_armdh_last_error(rrtx_armdh* a) { return last_error_of(a); }

int rrtx_armdh_forward(rrtx_armdh* a, const rrtx_armdh_batch* b) {
  const int rc = guarded(a, "rrtx_armdh_forward", [&] { return armdh_run(a, b, false, 0, 0.0, 0, 0.0); });
  if (rc < 0 && a) a->kind = 0;
  return rc;
}

int rrtx_armdh_solve(rrtx_armdh* a, const rrtx_armdh_batch* b, int32_t iter_cnt, double step_div, int32_t method, double eps) {
  const int rc = guarded(a, "rrtx_armdh_solve", [&] { return armdh_run(a, b, true, iter_cnt, step_div, method, eps); });
  if (rc < 0 && a) a->kind = 0;
  return rc;
}

int rrtx_armdh_get_records(rrtx_armdh* a, int32_t* status, double* values, double* kappa_max, int32_t* n_cut, int64_t* n_queries,
                           int64_t* n_links) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armdh_get_records: the DH-arm object is NULL");
  if (!a->kind) return fail(a, RRTX_E_STATE, "rrtx_armdh_get_records: no completed run");
  for (int64_t q = 0; q < a->n; q++) {
    const rppdh::Rec& r = a->h_rec[(size_t)q];
    if (status) status[q] = r.status;
    if (values) memcpy(values + 16 * q, r.v, sizeof(r.v));
    if (kappa_max) kappa_max[q] = r.kappa_max;
    if (n_cut) n_cut[q] = r.n_cut;
  }
  if (n_queries) *n_queries = a->n;
  if (n_links) *n_links = a->n_links;
  return RRTX_OK;
}

int rrtx_armdh_get_angles(rrtx_armdh* a, int64_t* offsets, double* angles, int64_t cap) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armdh_get_angles: the DH-arm object is NULL");
  if (!a->kind) return fail(a, RRTX_E_STATE, "rrtx_armdh_get_angles: no completed run");
  if (offsets) memcpy(offsets, a->h_ang_off.data(), sizeof(int64_t) * ((size_t)a->n + 1));
  if (!angles) return RRTX_OK;
  return armdh_fetch(a, "rrtx_armdh_get_angles", 2, ": the last run was a forward, which returns no angles", &rrtx_armdh::ang_out, angles, 1, cap);
}

int rrtx_armdh_get_transforms(rrtx_armdh* a, double* transforms, int64_t cap) {
  return armdh_fetch(a, "rrtx_armdh_get_transforms", 1, ": no completed forward", &rrtx_armdh::tf, transforms, 16, cap);
}

int rrtx_armdh_get_jacobians(rrtx_armdh* a, double* jacobians, int64_t cap) {
  return armdh_fetch(a, "rrtx_armdh_get_jacobians", 1, ": no completed forward", &rrtx_armdh::jac, jacobians, 6, cap);
}

int rrtx_armdh_get_kernel_ms(rrtx_armdh* a, double* kernel_ms, int32_t* waves) {
  if (!a) return fail(a, RRTX_E_INVALID, "rrtx_armdh_get_kernel_ms: the DH-arm object is NULL");
  if (kernel_ms) *kernel_ms = a->kernel_ms;
  if (waves) *waves = a->waves;
  return RRTX_OK;
}

}  // extern "C"

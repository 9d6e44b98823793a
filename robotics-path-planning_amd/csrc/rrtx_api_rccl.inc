// rrtx_api_rccl.inc -- several GPUs: rrtx_rccl_* and rrtx_plan_many (included by rrtx_api.hip)
// RCCL, opened with dlopen at first use (rrtx_rccl_*): no link-time dependency, nothing loaded by single-GPU users
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only: the functions are resolved with dlsym at first use (no link-time dependency)

#include <thread>

namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string err;
};
RcclApi* rccl_api() {
  static RcclApi api;
  if (api.lib || !api.err.empty()) return &api;
  for (const char* nm : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    api.lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (api.lib) break;
  }
  if (!api.lib) {
    api.err = std::string("librccl.so not loadable: ") + (dlerror() ? dlerror() : "?");
    return &api;
  }
  api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
  api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
  api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
  api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
  api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
  if (!api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy) {
    api.err = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy";
    api.lib = nullptr;
  }
  return &api;
}
}  // namespace

// rrtx_destroy: the handle's communicator, if it has one
static void rccl_release(rrtx_handle* h) {
  if (!h->rccl_comm) return;
  RcclApi* a = rccl_api();
  if (a->lib) a->CommDestroy((ncclComm_t)h->rccl_comm);
}

extern "C" {

// ---- native RCCL: the one collective of the path (SURVEY 8e: ncclAllGather of the 16-byte result records over xGMI) ----------

int rrtx_rccl_unique_id(void* id128) {
  if (!id128) return RRTX_E_INVALID;
  RcclApi* a = rccl_api();
  if (!a->lib) return RRTX_E_STATE;
  ncclUniqueId id;
  if (a->GetUniqueId(&id) != ncclSuccess) return RRTX_E_HIP;
  memcpy(id128, &id, sizeof(id));
  return RRTX_OK;
}

int rrtx_rccl_init(rrtx_handle* h, const void* id128, int32_t rank, int32_t world) {
  if (!h || !id128 || world < 1 || rank < 0 || rank >= world) return RRTX_E_INVALID;
  RcclApi* a = rccl_api();
  if (!a->lib) {
    h->err = a->err;
    return RRTX_E_STATE;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (h->rccl_comm) {
    a->CommDestroy((ncclComm_t)h->rccl_comm);
    h->rccl_comm = nullptr;
  }
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclComm_t comm = nullptr;
  const ncclResult_t r = a->CommInitRank(&comm, world, id, rank);
  if (r != ncclSuccess) {
    h->err = std::string("ncclCommInitRank: ") + (a->GetErrorString ? a->GetErrorString(r) : "error");
    return RRTX_E_HIP;
  }
  h->rccl_comm = (void*)comm;
  h->rccl_world = world;
  h->rccl_rank = rank;
  return h->reserve(h->rccl_recv, sizeof(Result) * (size_t)h->n_inst * world);   // every init: a later one may have a larger world
}

int rrtx_rccl_gather_results(rrtx_handle* h, double* path_cost, int32_t* n_nodes, int32_t* status) {
  if (!h) return RRTX_E_INVALID;
  if (!h->planned || !h->rccl_comm) return RRTX_E_STATE;
  RcclApi* a = rccl_api();
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = sizeof(Result) * (size_t)h->n_inst;
  // device -> device: the table the planner kernels wrote is what the collective sends
  const ncclResult_t r = a->AllGather(h->c.results, h->rccl_recv.p, bytes, ncclInt8, (ncclComm_t)h->rccl_comm, h->stream);
  if (r != ncclSuccess) {
    h->err = std::string("ncclAllGather: ") + (a->GetErrorString ? a->GetErrorString(r) : "error");
    return RRTX_E_HIP;
  }
  const size_t tot = (size_t)h->n_inst * h->rccl_world;
  std::vector<Result> all(tot);
  HIPCHK(h, hipMemcpyAsync(all.data(), h->rccl_recv.p, sizeof(Result) * tot, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < tot; i++) {
    if (path_cost) path_cost[i] = (all[i].status & RRTX_ST_PATH) ? all[i].path_cost : INFINITY;
    if (n_nodes) n_nodes[i] = all[i].n_nodes;
    if (status) status[i] = all[i].status;
  }
  return RRTX_OK;
}

int rrtx_plan_many(rrtx_handle** handles, int32_t n, int32_t* rcs) {
  if (!handles || n < 1) return RRTX_E_INVALID;
  for (int i = 0; i < n; i++)
    if (!handles[i]) return RRTX_E_INVALID;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < i; j++)
      if (handles[i] == handles[j]) return RRTX_E_INVALID;   // a handle is not thread safe
  std::vector<int> rc(n, RRTX_OK);
  if (n == 1) {
    rc[0] = rrtx_plan(handles[0]);
  } else {
    std::vector<std::thread> th;
    th.reserve(n);
    for (int i = 0; i < n; i++) th.emplace_back([&rc, handles, i]() { rc[i] = rrtx_plan(handles[i]); });
    for (auto& t : th) t.join();
  }
  int worst = RRTX_OK;
  for (int i = 0; i < n; i++) {
    if (rcs) rcs[i] = rc[i];
    if (rc[i] < 0 && (worst >= 0 || rc[i] < worst)) worst = rc[i];
    else if (rc[i] == RRTX_PARTIAL && worst == RRTX_OK) worst = RRTX_PARTIAL;
  }
  return worst;
}

}  // extern "C"

// rrtx_host.h -- the host-only core under the eight opaque objects of include/rrtx.h (rrtx_handle, rrtx_steer,
// rrtx_tracker, rrtx_spline, rrtx_bspline, rrtx_armnav, rrtx_armik, rrtx_armdh): one check macro, one device buffer, one
// device probe, one timed section, one lifecycle (create_object, destroy_object, last_error_of) and one guard against
// exceptions for the seven objects besides the planner handle, and the host helpers more than one object uses.  No kernels
// and no rpp* types: tests/native/host_core_check.cpp compiles it for the CPU against a fake HIP runtime and reaches the
// failure paths no GPU run can.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rrtx.h"

// libm through volatile pointers: the compiler must not fold pow(x, 2.0) into x*x
// (glibc's pow is not correctly rounded and the reference's `**2` goes through it).
inline double (*volatile libm_pow)(double, double) = pow;
inline double (*volatile libm_log)(double) = log;
inline double (*volatile libm_sqrt)(double) = sqrt;
inline double (*volatile libm_sin)(double) = sin;
inline double (*volatile libm_cos)(double) = cos;
inline double (*volatile libm_atan2)(double, double) = atan2;
inline double (*volatile libm_acos)(double) = acos;
inline double (*volatile libm_asin)(double) = asin;

inline double py_sq_host(double x) {
  if (x == 0.0) return 0.0;
  return libm_pow(std::fabs(x), 2.0);
}

inline bool all_finite(const double* v, int64_t count) {
  for (int64_t i = 0; i < count; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// starts at 0 and never decreases
inline bool csr_ok(const int64_t* off, int64_t n) {
  if (off[0] != 0) return false;
  for (int64_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}

// An obstacle list as a caller hands it over: m rows (x, y, size) and the robot radius (or one radius per course).  The
// checks come in two steps, because the entry points check other arguments between them; each returns the caller's own
// text for the first thing that is wrong, or nullptr.
struct ObsListText {
  const char *negative, *too_many, *null, *row, *radius;
};
inline const char* obstacle_list_shape_error(const double* oxyr, int64_t m, int64_t m_max, const ObsListText& t) {
  if (m < 0) return t.negative;
  if (m > m_max) return t.too_many;
  if (m > 0 && !oxyr) return t.null;
  return nullptr;
}
// radius_first: which of the two a list with both faults is refused for
inline const char* obstacle_list_value_error(const double* oxyr, int64_t m, const double* radius, int64_t n_radius,
                                             const ObsListText& t, bool radius_first = false) {
  if (radius_first && !all_finite(radius, n_radius)) return t.radius;
  if (!all_finite(oxyr, 3 * m)) return t.row;
  return all_finite(radius, n_radius) ? nullptr : t.radius;
}

// The rows as the kernels read them: (ox, oy, thr), thr = (size + robot_radius) ** 2 by the planners' routine
inline void pack_obstacle_rows(const double* oxyr, int64_t m, double radius, std::vector<double>& rows) {
  rows.resize(3 * (size_t)m);
  for (int64_t k = 0; k < m; k++) {
    rows[3 * k] = oxyr[3 * k];
    rows[3 * k + 1] = oxyr[3 * k + 1];
    rows[3 * k + 2] = py_sq_host(oxyr[3 * k + 2] + radius);
  }
}

// The kernels with one lane per point of a curve come as <STORE, CHECK>, CHECK one of rppc::CHECK_* (curve_check.hip.h:
// 0 none, 1 the linear loop, 2 the obstacle index).  Calls f with the pair as constants; one of store and check is wanted,
// so <false, 0> does not exist: without either the call is f(false, 1).
template <class F>
void with_store_check(bool store, int check, F&& f) {
  using std::bool_constant;
  using std::integral_constant;
  if (store && check == 2)
    f(bool_constant<true>{}, integral_constant<int, 2>{});
  else if (store && check)
    f(bool_constant<true>{}, integral_constant<int, 1>{});
  else if (store)
    f(bool_constant<true>{}, integral_constant<int, 0>{});
  else if (check == 2)
    f(bool_constant<false>{}, integral_constant<int, 2>{});
  else
    f(bool_constant<false>{}, integral_constant<int, 1>{});
}

// the tracking parameters rrtx_track_planned and rrtx_tracker_run accept, and what they say otherwise
inline bool track_params_ok(const rrtx_track_params* tp) {
  return tp->dt > 0.0 && tp->T >= 0.0 && tp->T / tp->dt <= 1.0e6 && tp->Lf > 0.0 && tp->L > 0.0 && tp->steer_max >= 0.0 &&
         tp->steer_max <= 0.79;
}
inline const char* const TRACK_PARAMS_MSG = "needs dt > 0, T / dt <= 1e6, Lf > 0, L > 0, 0 <= steer_max <= 0.79";

// the message of a call that was handed no object
inline thread_local std::string null_object_err;

// Records `msg` on the object (or for rrtx_*_last_error(NULL)) and returns rc
template <class Obj>
int fail(Obj* o, int rc, const std::string& msg) {
  (o ? o->err : null_object_err) = msg;
  return rc;
}

// A solve or run that completed (RRTX_OK or RRTX_PARTIAL) wrote the object's device buffers anew: what an
// rrtx_track_source names by its generation.  Returns rc.
template <class Obj>
int new_generation(Obj* o, int rc) {
  if (o && rc >= 0) o->generation++;
  return rc;
}

// Calls HIP; on an error records `#expr: message` on the object and returns RRTX_E_HIP from the calling function
#define HIPCHK(obj, expr)                                                                              \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(obj, RRTX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Device memory grown on demand: movable, not copyable, freed when destroyed or assigned to
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(bytes, o.bytes);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
  // At least `want` bytes; contents are not kept, and a failure leaves the buffer empty.  A caller that must keep what it
  // has on failure reserves into a fresh DevBuf and moves that in on success.
  hipError_t reserve(size_t want) {
    if (want <= bytes) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) p = nullptr;
    else bytes = want;
    return e;
  }
};

// What every object owns on its device: the stream its work is queued on, the two events of a timed section, and the
// message of its last failure.  Buffer members of a derived object are released before the stream and events are.
struct DevObj {
  int device = 0;
  bool usable = false;   // open() found a gfx950 device and created the stream and events
  int n_cu = 0;          // compute units of the device
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;

  DevObj() = default;
  DevObj(const DevObj&) = delete;
  DevObj& operator=(const DevObj&) = delete;
  ~DevObj() { close(); }

  // `who` names the caller in the message when there is no gfx950 device (RRTX_ALLOW_ANY_ARCH: any device)
  int open(int dev, const char* who) {
    device = dev;
    int ndev = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || dev < 0 || dev >= ndev ||
        hipGetDeviceProperties(&prop, dev) != hipSuccess ||
        (!strstr(prop.gcnArchName, "gfx950") && !getenv("RRTX_ALLOW_ANY_ARCH")))
      return fail(this, RRTX_E_NO_DEVICE, std::string(who) + ": no usable gfx950 device (there is no CPU fallback)");
    n_cu = prop.multiProcessorCount;
    HIPCHK(this, hipSetDevice(dev));
    HIPCHK(this, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(this, hipEventCreate(&ev0));
    HIPCHK(this, hipEventCreate(&ev1));
    usable = true;
    return RRTX_OK;
  }

  // Releases what open() created, however far it got
  void close() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
    ev0 = ev1 = nullptr;
    stream = nullptr;
    usable = false;
  }

  int reserve(DevBuf& b, size_t bytes) {
    const hipError_t e = b.reserve(bytes);
    if (e != hipSuccess) return fail(this, RRTX_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    return RRTX_OK;
  }

  // `bytes` of host data into b (grown as needed), queued on the stream
  int upload(DevBuf& b, const void* src, size_t bytes) {
    if (!bytes) return RRTX_OK;
    if (int rc = reserve(b, bytes)) return rc;
    HIPCHK(this, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, stream));
    return RRTX_OK;
  }

  // `bytes` of device memory into host memory, blocking
  int fetch(void* dst, const void* src, size_t bytes) {
    if (!bytes) return RRTX_OK;
    HIPCHK(this, hipSetDevice(device));
    HIPCHK(this, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RRTX_OK;
  }

  // What a run or solve answers on an object whose open() found no device, 0 otherwise; `fn_colon`: "rrtx_x_run: "
  int need_device(const char* fn_colon) {
    if (usable) return RRTX_OK;
    return fail(this, RRTX_E_NO_DEVICE, std::string(fn_colon) + "no usable gfx950 device (there is no CPU fallback)");
  }

  // One timed section on the stream: `queue` queues the kernels between the two events, `copies` the device -> host copies
  // that ride the same synchronisation (it returns a code; non-zero ends the section).  Waits, then *ms = the kernels' time.
  template <class Queue, class Copies>
  int timed(float* ms, Queue&& queue, Copies&& copies) {
    HIPCHK(this, hipEventRecord(ev0, stream));
    queue();
    HIPCHK(this, hipGetLastError());
    HIPCHK(this, hipEventRecord(ev1, stream));
    if (int rc = copies()) return rc;
    HIPCHK(this, hipStreamSynchronize(stream));
    HIPCHK(this, hipEventElapsedTime(ms, ev0, ev1));
    return RRTX_OK;
  }
  template <class Queue>
  int timed(float* ms, Queue&& queue) {
    return timed(ms, queue, []() -> int { return RRTX_OK; });
  }
};

// ---- the lifecycle of the seven objects besides the planner handle: rrtx_X_create, rrtx_X_destroy, rrtx_X_last_error --------
// `fn`: the entry point's name, without a colon
template <class T>
int create_object(int32_t device, T** out, const char* fn) {
  if (!out) return fail<T>(nullptr, RRTX_E_INVALID, std::string(fn) + ": out is NULL");
  *out = nullptr;
  if (device < 0) return fail<T>(nullptr, RRTX_E_INVALID, std::string(fn) + ": negative device ordinal");
  T* o = new (std::nothrow) T();
  if (!o) return fail<T>(nullptr, RRTX_E_HIP, std::string(fn) + ": out of host memory");
  *out = o;   // returned on failure too: the caller reads the message, and calls still check their arguments
  return o->open(device, fn);
}

template <class T>
void destroy_object(T* o) {
  if (!o) return;
  if (o->usable) (void)hipSetDevice(o->device);
  delete o;   // the buffers, then the events and the stream
}

template <class T>
const char* last_error_of(T* o) {
  return o ? o->err.c_str() : null_object_err.c_str();
}

// Nothing may throw across the ABI (host allocations: records, offsets, messages).  Returns body(); a std::exception becomes
// RRTX_E_HIP with the message "<fn>: <what>", after on_throw() has taken away what the failed call may have half written.
// What a returned error code invalidates is the entry point's own business.
template <class Obj, class Body, class OnThrow>
int guarded(Obj* o, const char* fn, Body&& body, OnThrow&& on_throw) {
  try {
    return body();
  } catch (const std::exception& e) {
    on_throw();
    return fail(o, RRTX_E_HIP, std::string(fn) + ": " + e.what());
  }
}
template <class Obj, class Body>
int guarded(Obj* o, const char* fn, Body&& body) {
  return guarded(o, fn, body, [] {});
}

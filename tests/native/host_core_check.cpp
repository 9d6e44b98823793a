// csrc/rrtx_host.h against the fake runtime of tests/native/fake_hip: the allocation- and creation-failure paths of the
// device buffer, the device-object base, the timed section, the objects' shared lifecycle and the guard against exceptions,
// which no GPU run can reach.  Built by tests/test_host_core.py
// with ASan + UBSan; prints "ok" and exits 0, or names the first check that failed.
#include <cstdio>

#include "rrtx_host.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      failures++;                                                    \
    }                                                                \
  } while (0)

static bool starts_with(const std::string& s, const char* prefix) { return s.rfind(prefix, 0) == 0; }

// the calls logged since `from`, joined with spaces
static std::string calls_since(size_t from) {
  std::string r;
  for (size_t i = from; i < fake_hip.log.size(); i++) r += (i > from ? " " : "") + fake_hip.log[i];
  return r;
}

static void reserve_happy_path() {
  DevObj o;
  DevBuf b;
  CHECK(o.reserve(b, 0) == RRTX_OK && fake_hip.mallocs == 0 && b.p == nullptr);   // nothing asked of an empty buffer
  CHECK(o.reserve(b, 64) == RRTX_OK && b.bytes == 64 && fake_hip.live_allocs == 1);
  void* p64 = b.p;
  CHECK(o.reserve(b, 32) == RRTX_OK && b.p == p64 && b.bytes == 64 && fake_hip.mallocs == 1);   // large enough: untouched
  const size_t at = fake_hip.log.size();
  CHECK(o.reserve(b, 128) == RRTX_OK && b.bytes == 128);
  CHECK(calls_since(at) == "hipFree hipMalloc");   // frees first, then allocates
  CHECK(fake_hip.live_allocs == 1 && fake_hip.mallocs == 2 && fake_hip.frees == 1);
  CHECK(b.as<double>() == (double*)b.p);
}

static void reserve_with_a_failing_allocation() {
  DevObj o;
  DevBuf b;
  CHECK(o.reserve(b, 64) == RRTX_OK);
  fake_hip.fail_malloc = 1;
  CHECK(o.reserve(b, 128) == RRTX_E_HIP);
  CHECK(starts_with(o.err, "hipMalloc"));
  CHECK(b.p == nullptr && b.bytes == 0 && fake_hip.live_allocs == 0);   // left empty, the old memory released
  CHECK(o.reserve(b, 128) == RRTX_OK && b.bytes == 128 && fake_hip.live_allocs == 1);   // and usable again
}

static void reserve_fresh_then_move_keeps_the_old_buffer_on_failure() {
  DevObj o;
  DevBuf b;
  CHECK(o.reserve(b, 64) == RRTX_OK);
  void* const p = b.p;
  for (int failing = 1; failing >= 0; failing--) {
    fake_hip.fail_malloc = failing;
    DevBuf fresh;
    const int rc = o.reserve(fresh, 128);
    if (rc == RRTX_OK) b = std::move(fresh);
    if (failing) CHECK(rc == RRTX_E_HIP && b.p == p && b.bytes == 64 && fake_hip.live_allocs == 1);
    else CHECK(rc == RRTX_OK && b.bytes == 128 && fresh.p == nullptr && fake_hip.live_allocs == 1);
  }
}

static void moved_from_buffer_frees_nothing() {
  DevObj o;
  const int frees = fake_hip.frees;
  {
    DevBuf a;
    CHECK(o.reserve(a, 16) == RRTX_OK);
    DevBuf b(std::move(a));
    CHECK(a.p == nullptr && a.bytes == 0 && b.bytes == 16);
  }
  CHECK(fake_hip.frees == frees + 1 && fake_hip.live_allocs == 0);   // once, by the buffer that took it over
}

// open() with the n-th creation failing: close() releases exactly what was created, a second close() nothing
static void open_fails(int fail_stream, int fail_event, int streams_made, int events_made) {
  DevObj o;
  fake_hip.fail_stream = fail_stream;
  fake_hip.fail_event = fail_event;
  CHECK(o.open(0, "check") == RRTX_E_HIP);
  CHECK(!o.usable && starts_with(o.err, fail_stream ? "hipStreamCreateWithFlags" : "hipEventCreate"));
  CHECK(fake_hip.live_streams == streams_made && fake_hip.live_events == events_made);
  size_t at = fake_hip.log.size();
  o.close();
  CHECK(fake_hip.live_streams == 0 && fake_hip.live_events == 0);
  CHECK((int)(fake_hip.log.size() - at) == streams_made + events_made);
  at = fake_hip.log.size();
  o.close();
  CHECK(fake_hip.log.size() == at && !o.usable);
  fake_hip.fail_stream = fake_hip.fail_event = 0;
}

static void open_and_the_device_probe() {
  {
    DevObj o;
    CHECK(o.open(0, "check") == RRTX_OK && o.usable && o.n_cu == 256 && o.device == 0);
    CHECK(fake_hip.live_streams == 1 && fake_hip.live_events == 2);
  }   // the destructor closes
  CHECK(fake_hip.live_streams == 0 && fake_hip.live_events == 0);
  DevObj o;
  CHECK(o.open(1, "check") == RRTX_E_NO_DEVICE && !o.usable);   // one device: ordinal 1 is out of range
  CHECK(o.err == "check: no usable gfx950 device (there is no CPU fallback)");
  fake_hip.arch = "gfx942";
  CHECK(o.open(0, "check") == RRTX_E_NO_DEVICE && fake_hip.live_streams == 0);
  fake_hip.arch = "gfx950";
  fake_hip.devices = 0;
  CHECK(o.open(0, "check") == RRTX_E_NO_DEVICE);
  fake_hip.devices = 1;
}

static void timed_section() {
  DevObj o;
  CHECK(o.open(0, "check") == RRTX_OK);
  float ms = 0.f;
  size_t at = fake_hip.log.size();
  int rc = o.timed(&ms, [] { fake_hip.log.push_back("queue"); }, []() -> int {
    fake_hip.log.push_back("copies");
    return RRTX_OK;
  });
  CHECK(rc == RRTX_OK && ms == 1.5f);
  CHECK(calls_since(at) == "hipEventRecord queue hipGetLastError hipEventRecord copies hipStreamSynchronize hipEventElapsedTime");
  at = fake_hip.log.size();
  CHECK(o.timed(&ms, [] { fake_hip.log.push_back("queue"); }) == RRTX_OK);   // without copies: the same order
  CHECK(calls_since(at) == "hipEventRecord queue hipGetLastError hipEventRecord hipStreamSynchronize hipEventElapsedTime");
  // a launch error: the section ends there
  at = fake_hip.log.size();
  bool copied = false;
  rc = o.timed(&ms, [] { fake_hip.last_error = hipErrorLaunchFailure; }, [&]() -> int {
    copied = true;
    return RRTX_OK;
  });
  CHECK(rc == RRTX_E_HIP && !copied && starts_with(o.err, "hipGetLastError()"));
  CHECK(calls_since(at) == "hipEventRecord hipGetLastError");
  // a failing copy callback ends it with its code
  CHECK(o.timed(&ms, [] {}, []() -> int { return RRTX_E_STATE; }) == RRTX_E_STATE);
  // upload: grows the buffer, copies the bytes, does nothing for none
  DevBuf b;
  const double src[3] = {1.0, 2.0, 3.0};
  CHECK(o.upload(b, src, 0) == RRTX_OK && b.p == nullptr);
  CHECK(o.upload(b, src, sizeof(src)) == RRTX_OK && b.bytes == sizeof(src) && memcmp(b.p, src, sizeof(src)) == 0);
  fake_hip.fail_malloc = 1;
  CHECK(o.upload(b, src, 2 * sizeof(src)) == RRTX_E_HIP && b.p == nullptr);
}

static void the_shared_helpers() {
  CHECK(fail<DevObj>(nullptr, RRTX_E_INVALID, "no object") == RRTX_E_INVALID && null_object_err == "no object");
  const double v[3] = {0.0, -1.0, INFINITY};
  CHECK(all_finite(v, 2) && !all_finite(v, 3) && all_finite(nullptr, 0));
  const int64_t up[3] = {0, 2, 2}, down[3] = {0, 2, 1}, late[2] = {1, 2};
  CHECK(csr_ok(up, 2) && !csr_ok(down, 2) && !csr_ok(late, 1));
  CHECK(py_sq_host(-3.0) == 9.0 && py_sq_host(0.0) == 0.0);
  rrtx_track_params tp;
  memset(&tp, 0, sizeof(tp));
  tp.dt = 0.1, tp.T = 100.0, tp.Lf = 2.0, tp.L = 2.9, tp.steer_max = 0.785;
  CHECK(track_params_ok(&tp));
  tp.steer_max = 0.8;
  CHECK(!track_params_ok(&tp));
  tp.steer_max = 0.785, tp.dt = NAN;
  CHECK(!track_params_ok(&tp));
}

// with_store_check reaches <STORE, CHECK> for the five pairs the kernels exist for; (false, none) falls to <false, linear>
static void store_check_dispatch() {
  const struct { bool store; int check; bool want_store; int want_check; } cases[6] = {
      {true, 2, true, 2}, {true, 1, true, 1}, {true, 0, true, 0}, {false, 2, false, 2}, {false, 1, false, 1}, {false, 0, false, 1}};
  for (const auto& c : cases) {
    int calls = 0;
    with_store_check(c.store, c.check, [&](auto st, auto ck) {
      static_assert(decltype(st)::value || decltype(ck)::value != 0, "<false, none> is never instantiated");
      calls++;
      CHECK(decltype(st)::value == c.want_store && decltype(ck)::value == c.want_check);
    });
    CHECK(calls == 1);
  }
}

static void obstacle_rows_are_packed() {
  std::vector<double> rows(7, -1.0);
  pack_obstacle_rows(nullptr, 0, 0.5, rows);
  CHECK(rows.empty());
  // one row; a negative size + radius; a size whose square overflows
  const double one[3] = {1.5, -2.5, 0.75};
  pack_obstacle_rows(one, 1, 0.25, rows);
  CHECK(rows.size() == 3 && rows[0] == 1.5 && rows[1] == -2.5 && rows[2] == py_sq_host(0.75 + 0.25) && rows[2] == 1.0);
  const double three[9] = {0.0, 1.0, 0.5, 2.0, 3.0, -1.0, 4.0, 5.0, 1e200};
  pack_obstacle_rows(three, 3, -2.0, rows);
  CHECK(rows.size() == 9);
  for (int k = 0; k < 3; k++) {
    CHECK(rows[3 * k] == three[3 * k] && rows[3 * k + 1] == three[3 * k + 1]);
    CHECK(rows[3 * k + 2] == py_sq_host(three[3 * k + 2] + -2.0));
  }
  CHECK(rows[2] == 2.25 && rows[5] == 9.0 && std::isinf(rows[8]) && rows[8] > 0.0);
}

static void obstacle_list_checks_refuse_in_the_callers_words() {
  const ObsListText t = {"negative", "too many", "null", "row", "radius"};
  const double ok[6] = {0.0, 1.0, 0.5, 2.0, 3.0, 0.5}, nan_row[6] = {0.0, 1.0, 0.5, 2.0, NAN, 0.5};
  const double r = 0.5, nan_r = NAN, rr[2] = {0.5, INFINITY};
  const int64_t cap = 1LL << 20;
  auto is = [](const char* got, const char* want) { return got && std::string(got) == want; };
  CHECK(is(obstacle_list_shape_error(ok, -1, cap, t), "negative"));
  CHECK(is(obstacle_list_shape_error(ok, cap + 1, cap, t), "too many"));
  CHECK(is(obstacle_list_shape_error(nullptr, 1, cap, t), "null"));
  CHECK(obstacle_list_shape_error(nullptr, 0, cap, t) == nullptr);   // no rows: no pointer needed
  CHECK(obstacle_list_shape_error(ok, 2, cap, t) == nullptr && obstacle_list_shape_error(ok, cap, cap, t) == nullptr);
  CHECK(obstacle_list_shape_error(ok, cap + 1, INT64_MAX, t) == nullptr);   // a caller without a limit of its own
  CHECK(is(obstacle_list_value_error(nan_row, 2, &r, 1, t), "row"));
  CHECK(is(obstacle_list_value_error(ok, 2, &nan_r, 1, t), "radius"));
  CHECK(is(obstacle_list_value_error(ok, 2, rr, 2, t), "radius") && obstacle_list_value_error(ok, 2, rr, 1, t) == nullptr);
  CHECK(obstacle_list_value_error(ok, 2, &r, 1, t) == nullptr && obstacle_list_value_error(nullptr, 0, &r, 1, t) == nullptr);
  CHECK(obstacle_list_value_error(nan_row, 1, &r, 1, t) == nullptr);   // the NaN lies in the second row
  // both wrong: the rows are named first, unless the caller checks the radius first
  CHECK(is(obstacle_list_value_error(nan_row, 2, &nan_r, 1, t), "row"));
  CHECK(is(obstacle_list_value_error(nan_row, 2, &nan_r, 1, t, true), "radius"));
  CHECK(is(obstacle_list_value_error(nan_row, 2, &r, 1, t, true), "row"));
}

// what an object of the C ABI looks like to the shared lifecycle: a DevObj with buffers and a result flag
struct Probe : DevObj {
  DevBuf b;
  bool ran = true;
  // host memory that can be told to run out
  static inline bool fail_new = false;
  static void* operator new(size_t n, const std::nothrow_t&) noexcept { return fail_new ? nullptr : malloc(n); }
  static void operator delete(void* p, const std::nothrow_t&) noexcept { free(p); }
  static void operator delete(void* p) noexcept { free(p); }
};

static void create_object_refuses_and_creates() {
  Probe* p = (Probe*)0x1;
  CHECK(create_object<Probe>(0, nullptr, "probe_create") == RRTX_E_INVALID);
  CHECK(std::string(last_error_of<Probe>(nullptr)) == "probe_create: out is NULL");
  CHECK(create_object(-1, &p, "probe_create") == RRTX_E_INVALID && p == nullptr);
  CHECK(std::string(last_error_of<Probe>(nullptr)) == "probe_create: negative device ordinal");
  Probe::fail_new = true;
  CHECK(create_object(0, &p, "probe_create") == RRTX_E_HIP && p == nullptr);
  Probe::fail_new = false;
  CHECK(std::string(last_error_of<Probe>(nullptr)) == "probe_create: out of host memory");

  CHECK(create_object(0, &p, "probe_create") == RRTX_OK && p && p->usable && p->device == 0);
  CHECK(std::string(last_error_of(p)).empty());
  CHECK(fake_hip.live_streams == 1 && fake_hip.live_events == 2);
  destroy_object(p);
  CHECK(fake_hip.live_streams == 0 && fake_hip.live_events == 0);

  // a failing stream creation, then a failing second event creation: the object comes back with the message
  for (int second_event = 0; second_event < 2; second_event++) {
    fake_hip.fail_stream = second_event ? 0 : 1;
    fake_hip.fail_event = second_event ? 2 : 0;
    p = nullptr;
    CHECK(create_object(0, &p, "probe_create") == RRTX_E_HIP && p != nullptr && !p->usable);
    CHECK(starts_with(last_error_of(p), second_event ? "hipEventCreate" : "hipStreamCreateWithFlags"));
    destroy_object(p);
    CHECK(fake_hip.live_streams == 0 && fake_hip.live_events == 0 && fake_hip.live_allocs == 0);
    fake_hip.fail_stream = fake_hip.fail_event = 0;
  }

  // no device: still an object, whose calls check their arguments and then refuse
  fake_hip.devices = 0;
  p = nullptr;
  CHECK(create_object(0, &p, "probe_create") == RRTX_E_NO_DEVICE && p != nullptr && !p->usable);
  CHECK(std::string(last_error_of(p)) == "probe_create: no usable gfx950 device (there is no CPU fallback)");
  CHECK(p->need_device("probe_run: ") == RRTX_E_NO_DEVICE);
  CHECK(p->err == "probe_run: no usable gfx950 device (there is no CPU fallback)");
  const size_t at = fake_hip.log.size();
  destroy_object(p);
  CHECK(calls_since(at).find("hipSetDevice") == std::string::npos);   // an unusable object never selects a device
  fake_hip.devices = 1;
}

static void destroy_object_releases_in_order() {
  size_t at = fake_hip.log.size();
  destroy_object<Probe>(nullptr);
  CHECK(fake_hip.log.size() == at);
  Probe* p = nullptr;
  CHECK(create_object(0, &p, "probe_create") == RRTX_OK);
  CHECK(p->need_device("probe_run: ") == RRTX_OK && p->err.empty());
  CHECK(p->reserve(p->b, 32) == RRTX_OK);
  at = fake_hip.log.size();
  destroy_object(p);   // the device, the buffers, then the events and the stream
  CHECK(calls_since(at) == "hipSetDevice hipFree hipEventDestroy hipEventDestroy hipStreamDestroy");
  CHECK(fake_hip.live_allocs == 0 && fake_hip.live_streams == 0 && fake_hip.live_events == 0);
}

static void guarded_entry_points() {
  Probe o;
  int thrown = 0;
  auto on_throw = [&] { thrown++, o.ran = false; };
  // a body's code passes through, and nothing is taken away
  CHECK(guarded(&o, "fn", [] { return (int)RRTX_OK; }, on_throw) == RRTX_OK);
  CHECK(guarded(&o, "fn", [] { return (int)RRTX_PARTIAL; }, on_throw) == RRTX_PARTIAL);
  CHECK(guarded(&o, "fn", [] { return (int)RRTX_E_STATE; }, on_throw) == RRTX_E_STATE);
  CHECK(guarded(&o, "fn", [&] { return fail(&o, RRTX_E_HIP, "the body's own"); }, on_throw) == RRTX_E_HIP);
  CHECK(thrown == 0 && o.ran && o.err == "the body's own");
  // a throw becomes a code and a message, after on_throw has run once
  CHECK(guarded(&o, "fn", []() -> int { throw std::bad_alloc(); }, on_throw) == RRTX_E_HIP);
  CHECK(thrown == 1 && !o.ran && o.err == "fn: std::bad_alloc");
  // without on_throw, and without an object
  o.err.clear();
  CHECK(guarded(&o, "fn2", []() -> int { throw std::bad_alloc(); }) == RRTX_E_HIP && o.err == "fn2: std::bad_alloc");
  CHECK(guarded((Probe*)nullptr, "fn3", []() -> int { throw std::bad_alloc(); }) == RRTX_E_HIP);
  CHECK(std::string(last_error_of<Probe>(nullptr)) == "fn3: std::bad_alloc");
  CHECK(guarded((Probe*)nullptr, "fn3", [] { return (int)RRTX_PARTIAL; }) == RRTX_PARTIAL);
}

static void fetch_copies_device_memory() {
  Probe o;
  CHECK(o.open(0, "check") == RRTX_OK);
  const double src[3] = {1.0, 2.0, 3.0};
  CHECK(o.upload(o.b, src, sizeof(src)) == RRTX_OK);
  double dst[3] = {0.0, 0.0, 0.0};
  size_t at = fake_hip.log.size();
  CHECK(o.fetch(dst, o.b.p, sizeof(dst)) == RRTX_OK && memcmp(dst, src, sizeof(src)) == 0);
  CHECK(calls_since(at) == "hipSetDevice hipMemcpy");
  at = fake_hip.log.size();
  CHECK(o.fetch(nullptr, nullptr, 0) == RRTX_OK && fake_hip.log.size() == at);   // nothing to copy: no call at all
}

int main() {
  reserve_happy_path();
  reserve_with_a_failing_allocation();
  reserve_fresh_then_move_keeps_the_old_buffer_on_failure();
  moved_from_buffer_frees_nothing();
  open_fails(1, 0, 0, 0);   // the stream
  open_fails(0, 2, 1, 1);   // the second event
  open_and_the_device_probe();
  timed_section();
  the_shared_helpers();
  store_check_dispatch();
  obstacle_rows_are_packed();
  obstacle_list_checks_refuse_in_the_callers_words();
  create_object_refuses_and_creates();
  destroy_object_releases_in_order();
  guarded_entry_points();
  fetch_copies_device_memory();
  CHECK(fake_hip.live_allocs == 0 && fake_hip.live_streams == 0 && fake_hip.live_events == 0);
  CHECK(fake_hip.mallocs == fake_hip.frees);
  if (!failures) printf("ok\n");
  return failures ? 1 : 0;
}

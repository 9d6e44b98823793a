// A fake of exactly the HIP calls csrc/rrtx_host.h uses, for tests/native/host_core_check.cpp: device memory is malloc,
// copies are memcpy, streams and events are dummies.  Every call is logged, live objects are counted, and the n-th
// hipMalloc / stream creation / event creation can be told to fail.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorNoDevice = 100, hipErrorLaunchFailure = 719 };
typedef struct fake_stream* hipStream_t;
typedef struct fake_event* hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
enum { hipStreamNonBlocking = 1 };
struct hipDeviceProp_t {
  char gcnArchName[256];
  int multiProcessorCount;
};

struct FakeHip {
  std::vector<std::string> log;   // the name of every call, in order
  int live_allocs = 0, live_streams = 0, live_events = 0;
  int mallocs = 0, frees = 0;
  // 1 = the next call of that kind fails, 2 = the one after it, ...; 0 = none
  int fail_malloc = 0, fail_stream = 0, fail_event = 0;
  hipError_t last_error = hipSuccess;   // what the next hipGetLastError reports (and clears)
  int devices = 1;
  const char* arch = "gfx950:sramecc+:xnack-";
};
inline FakeHip fake_hip;

inline bool fake_hip_trips(int& countdown) { return countdown > 0 && --countdown == 0; }

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "fake error"; }

inline hipError_t hipGetDeviceCount(int* n) {
  fake_hip.log.push_back("hipGetDeviceCount");
  *n = fake_hip.devices;
  return fake_hip.devices > 0 ? hipSuccess : hipErrorNoDevice;
}
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {
  fake_hip.log.push_back("hipGetDeviceProperties");
  memset(p, 0, sizeof(*p));
  strncpy(p->gcnArchName, fake_hip.arch, sizeof(p->gcnArchName) - 1);
  p->multiProcessorCount = 256;
  return hipSuccess;
}
inline hipError_t hipSetDevice(int) {
  fake_hip.log.push_back("hipSetDevice");
  return hipSuccess;
}
inline hipError_t hipMalloc(void** p, size_t bytes) {
  fake_hip.log.push_back("hipMalloc");
  if (fake_hip_trips(fake_hip.fail_malloc)) return hipErrorOutOfMemory;
  *p = malloc(bytes ? bytes : 1);
  fake_hip.live_allocs++;
  fake_hip.mallocs++;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  fake_hip.log.push_back("hipFree");
  if (p) {
    free(p);
    fake_hip.live_allocs--;
    fake_hip.frees++;
  }
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  fake_hip.log.push_back("hipMemcpyAsync");
  memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  fake_hip.log.push_back("hipMemcpy");
  memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  fake_hip.log.push_back("hipStreamCreateWithFlags");
  if (fake_hip_trips(fake_hip.fail_stream)) return hipErrorOutOfMemory;
  *s = (hipStream_t)malloc(1);
  fake_hip.live_streams++;
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  fake_hip.log.push_back("hipStreamDestroy");
  free(s);
  fake_hip.live_streams--;
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  fake_hip.log.push_back("hipStreamSynchronize");
  return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t* e) {
  fake_hip.log.push_back("hipEventCreate");
  if (fake_hip_trips(fake_hip.fail_event)) return hipErrorOutOfMemory;
  *e = (hipEvent_t)malloc(1);
  fake_hip.live_events++;
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  fake_hip.log.push_back("hipEventDestroy");
  free(e);
  fake_hip.live_events--;
  return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) {
  fake_hip.log.push_back("hipEventRecord");
  return hipSuccess;
}
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  fake_hip.log.push_back("hipEventElapsedTime");
  *ms = 1.5f;
  return hipSuccess;
}
inline hipError_t hipGetLastError() {
  fake_hip.log.push_back("hipGetLastError");
  const hipError_t e = fake_hip.last_error;
  fake_hip.last_error = hipSuccess;
  return e;
}

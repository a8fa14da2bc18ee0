// Host helpers every unit with C entry points shares: the thread's error text, HIP error codes, the device guard, the
// alignment and workspace checks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/wekws_hip.h"

// a host function that crosses units of the library and is no part of what it exports
#define WEKWS_LOCAL __attribute__((visibility("hidden")))

namespace wekws {
// sets the thread's last-error message (wekws_hip_last_error) and returns `code`; the string lives in model.hip
int set_last_error(int code, const char* msg);
}  // namespace wekws

static int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), unused));
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return wekws::set_last_error(code, buf);
}

// the WEKWS_HIP_* code of a failed HIP call
static inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? WEKWS_HIP_ENOMEM : WEKWS_HIP_EDEVICE; }
static inline __attribute__((unused)) int hip_fail(hipError_t e, const char* what) {
  return fail(hip_code(e), "%s: %s", what, hipGetErrorString(e));
}

#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);  \
  } while (0)

// Makes `device` current for the scope and restores the caller's device afterwards: the library never changes the
// calling thread's current device behind its back (a Python __del__ may run at any time).
struct WEKWS_LOCAL DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) ok = hipSetDevice(device) == hipSuccess;
    else prev = -1;                       // already current: nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// does `p` (NULL included) start on a 16-byte boundary, as the kernels' 16-byte accesses and double workspaces need?
static inline __attribute__((unused)) bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The caller's workspace for the call `what`: present, 16-byte aligned and of at least `need` bytes, the figure `sizer_name`
// (the exported wekws_hip_*_workspace_bytes) gives for the shape.
static inline __attribute__((unused)) int check_workspace(const char* what, const void* workspace, size_t workspace_bytes, size_t need,
                                                          const char* sizer_name) {
  if (!workspace) return fail(WEKWS_HIP_EINVAL, "%s: this call needs a workspace", what);
  if (!aligned16(workspace)) return fail(WEKWS_HIP_EINVAL, "%s: the workspace must be 16-byte aligned", what);
  if (workspace_bytes < need)
    return fail(WEKWS_HIP_EINVAL, "%s: workspace of %zu bytes, need %zu (%s)", what, workspace_bytes, need, sizer_name);
  return WEKWS_HIP_OK;
}

// is `stream` being captured into a HIP graph?  (a capture admits no synchronisation and no allocation)
static inline __attribute__((unused)) bool stream_is_capturing(hipStream_t stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// does the head give one output row per frame (LINEAR, IDENTITY) and not one per utterance (GLOBAL, LAST)?
static inline __attribute__((unused)) bool per_frame_head(const wekws_hip_desc& d) {
  return d.head == WEKWS_HIP_HEAD_LINEAR || d.head == WEKWS_HIP_HEAD_IDENTITY;
}

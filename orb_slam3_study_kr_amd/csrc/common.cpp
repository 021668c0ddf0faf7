// common.cpp -- osh_last_error / osh_version / osh_device_count and the host plumbing of common.h.
#include "common.h"
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

namespace osh {
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

int launch_check(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("kernel launch %s failed: %s", what, hipGetErrorString(e)); return OSH_ERR_DEVICE; }
  return OSH_OK;
}

int allow_dynamic_lds(int device, int bytes, std::initializer_list<const void*> kernels) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> done;
  std::lock_guard<std::mutex> lock(mu);
  for (const void* k : kernels) {
    if (std::find(done.begin(), done.end(), std::make_pair(k, device)) != done.end()) continue;
    OSH_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.emplace_back(k, device);
  }
  return OSH_OK;
}

int StagedCall::reserve(const Layout& in, const Layout& out, size_t work_bytes, size_t min_arena_bytes) {
  in_bytes = in.bytes; out_bytes = out.bytes;
  if (!h_in.reserve(in_bytes) || !h_out.reserve(out_bytes)) {
    set_error("pinned staging allocation of %zu + %zu bytes failed", in_bytes, out_bytes);
    return OSH_ERR_DEVICE;
  }
  return arena.reserve(std::max(in_bytes + out_bytes + work_bytes, min_arena_bytes));
}

int StagedCall::upload(hipStream_t s) {
  OSH_HIP(hipMemcpyAsync(dev_in(), host_in(), in_bytes, hipMemcpyHostToDevice, s));
  return OSH_OK;
}

int StagedCall::download(hipStream_t s) {
  OSH_HIP(hipMemcpyAsync(host_out(), dev_out(), out_bytes, hipMemcpyDeviceToHost, s));
  OSH_HIP(hipStreamSynchronize(s));
  return OSH_OK;
}
}  // namespace osh

extern "C" {
const char* osh_last_error(void) { return osh::get_error(); }
const char* osh_version(void) { return "orbslam3_hip 0.1 gfx950"; }
int osh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
}

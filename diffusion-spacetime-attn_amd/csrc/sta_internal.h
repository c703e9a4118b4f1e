// Internal to libsta_xattn.so: the thread-local error text behind sta_last_error(), the per-device
// "dynamic LDS size raised" bookkeeping, the tuning hook, and the host-side launch helpers every entry point goes through.
#ifndef STA_INTERNAL_H
#define STA_INTERNAL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
extern thread_local char g_sta_err[256];
int sta_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// after a launch: STA_OK, or STA_E_LAUNCH with "<what>: <HIP's text>" (both defined in sta_xattn.hip)
int sta_launched(const char* what);

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: one flag per (kernel
// instantiation, device), so a process that drives several GPUs raises the limit on each of them.
// (Benign race: the call is idempotent.)
constexpr int STA_MAX_DEVICES = 64;
struct StaLdsAttr {
  bool done[STA_MAX_DEVICES] = {};
  bool ensure(const void* kernel, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (dev >= 0 && dev < STA_MAX_DEVICES && done[dev]) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    if (dev >= 0 && dev < STA_MAX_DEVICES) done[dev] = true;
    return true;
  }
};

// kernel-selection overrides set through sta_set_option (include/sta_xattn.h); 0 = automatic. Relaxed atomics: a test or tool
// thread may flip one while another thread launches (each launch reads every key it needs exactly once per decision).
#include <atomic>
struct StaOpt {
  std::atomic<int> v{0};
  operator int() const { return v.load(std::memory_order_relaxed); }
  void operator=(int x) { v.store(x, std::memory_order_relaxed); }
};
extern StaOpt g_sta_opt[STA_OPT_COUNT];

// Forced inline: a launch site compiles to what it would be written out by hand (tracked epochs are bound by eager launches).
#define STA_INLINE __attribute__((always_inline)) inline

// One launch and its check. Kernel is a template argument so that sta_launch_lds can own the StaLdsAttr of exactly that
// instantiation; the arguments convert to the kernel's parameter types as in a direct launch.
template <auto Kernel, typename... A>
STA_INLINE int sta_launch(const char* what, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... a) {
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, a...);
  return sta_launched(what);
}

// For a kernel that needs more than the default dynamic LDS: raises its limit to lds_limit once per device ...
template <auto Kernel>
STA_INLINE int sta_raise_lds(const char* what, int lds_limit) {
  static StaLdsAttr attr;
  return attr.ensure((const void*)Kernel, lds_limit) ? STA_OK : sta_fail(STA_E_LAUNCH, "hipFuncSetAttribute(%s) failed", what);
}

// ... and launches it with lds <= lds_limit bytes.
template <auto Kernel, typename... A>
STA_INLINE int sta_launch_lds(const char* what, int lds_limit, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... a) {
  if (const int rc = sta_raise_lds<Kernel>(what, lds_limit)) return rc;
  return sta_launch<Kernel>(what, grid, block, lds, st, a...);
}

// f(T{}) with T = the element type of `dtype`: one launch written against T instead of a bf16 / f16 pair
template <typename F>
STA_INLINE int sta_by_dtype(int dtype, F&& f) {
  if (dtype == STA_BF16) return f(__bf16{});
  if (dtype == STA_F16) return f(_Float16{});
  return sta_fail(STA_E_UNSUP, "dtype %d", dtype);
}

// the elementwise kernels: a lane's 16 bytes of T; null or 16-byte aligned; 256-lane blocks over nvec vectors, grid-stride from 8192 blocks up
template <typename T> struct V8T { typedef T type __attribute__((ext_vector_type(8))); };
inline bool sta_aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }
inline unsigned sta_grid_for(long nvec) {
  long blocks = (nvec + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  return (unsigned)blocks;
}
#endif

// hip_runtime_emul.h — TEST HARNESS ONLY (included by rg_api.hip under -DRG_EMUL, never by the product build).  The slice of the HIP
// runtime API that the host side of the C ABI uses, for the CPU emulation build: "device memory" is host memory, streams and devices
// do not exist, and a launch runs the kernel on the fibers of tests/emul/hip_emul.h.  It sits beside rg_api.hip because it mirrors that
// file's hip* calls one for one: whatever harness compiles rg_api.hip for the host finds it with it.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "hip_emul.h"

typedef void* hipStream_t;
typedef int hipError_t;
#define hipSuccess 0
enum { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
static hipError_t hipMalloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? 0 : 1; }
static hipError_t hipFree(void* p) { free(p); return 0; }
static hipError_t hipMemcpy(void* d, const void* s, size_t n, int) { memcpy(d, s, n); return 0; }
static hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); return 0; }
static hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return 0; }
static hipError_t hipMemset2D(void* d, size_t pitch, int v, size_t w, size_t h) { for (size_t r = 0; r < h; r++) memset((char*)d + r * pitch, v, w); return 0; }
static hipError_t hipGetDevice(int* dev) { *dev = 0; return 0; }
static hipError_t hipSetDevice(int) { return 0; }
static hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
static hipError_t hipDeviceSynchronize() { return 0; }
static hipError_t hipGetLastError() { return 0; }
static const char* hipGetErrorString(hipError_t) { return "emul"; }
struct DeviceGuard { explicit DeviceGuard(int) {} };

// launch of a closure: `f()` is the kernel call with its arguments bound.  It is invoked once per fiber start and has to
// stay alive only until this returns (emul_launch_n returns after the last workgroup has finished).
template <class F> static void emul_launch_closure(int nblocks, int nthreads, size_t lds_bytes, F&& f) {
  emul_launch_n(nblocks, nthreads, lds_bytes, [](void* p) { (*static_cast<std::remove_reference_t<F>*>(p))(); }, (void*)&f);
}

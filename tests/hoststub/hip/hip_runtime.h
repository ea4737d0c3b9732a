// HOST-ONLY STAND-IN for <hip/hip_runtime.h> - TEST INFRASTRUCTURE (tests/test_host_asan.py), never part of the product.
//
// SURVEY section 5 asks for sanitizer coverage of the host code; GPU AddressSanitizer is not available on this pool.  The host
// half of libkarios_hip.so (every api*.hip: argument validation, workspace slots, upload tickets, the frame ring, the host algebra
// and list protocols of the align step; staging.hip: the page-locked staging ring and landing arena) is compiled a second time with
// g++ -fsanitize=address,undefined against THIS header: "device" memory is host memory, streams execute at once, events are always
// complete, kernels (stub_kernels.cpp, stub_kernels_align.cpp) fill their outputs deterministically - those of RANSAC and SIFT with
// the arithmetic of ransac_math.hpp / sift_math.hpp.  What is exercised is the host code and every memcpy of the staging paths.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "../stub_order.hpp"      // the happens-before checker (off by default: every hook below then returns at once)

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorNotReady = 600 };
typedef struct stub_stream *hipStream_t;
typedef struct stub_event *hipEvent_t;
struct stub_stream { int priority; };
struct stub_event { int recorded; };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipHostMallocDefault = 0, hipHostRegisterDefault = 0 };
enum hipMemoryType { hipMemoryTypeHost = 1, hipMemoryTypeDevice = 2, hipMemoryTypeUnregistered = 0 };
enum hipDeviceAttribute_t { hipDeviceAttributeMultiprocessorCount = 16 };
struct hipPointerAttribute_t { hipMemoryType type; int device; void *devicePointer, *hostPointer; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct alignas(16) float4 { float x, y, z, w; };      // (k_align.hpp: the {image, gx, gy, pre-mask} plane of the ECC input)

// registry of the page-locked ranges (hipHostMalloc): hipPointerGetAttributes tells them from pageable memory
struct stub_state {
    std::mutex m;
    std::map<const char *, size_t> pinned;
    long device_allocs = 0, host_allocs = 0, pageable_async_copies = 0;
    long streams = 0, events = 0;    // alive (like the two allocation counts: up where the stand-in creates one, down where it destroys one)
    int fail_malloc_after = -1;      // test knob: the n-th hipMalloc from now fails
    int fail_host_malloc_after = -1; //   ... the n-th hipHostMalloc
    int fail_create_after = -1;      //   ... the n-th creation of a stream or an event
    bool lk_jobs_unsupported = false;   // kl_jobs_launch answers KM_E_UNSUPPORTED: the kernel-size search with batched corners, trackers one by one
    bool corners_like_exact = false;    // kf_rank_select_units finds the corners the stand-ins of the exact path find
};
stub_state &stub();
// true: this call is the one a knob condemned (the knob then disarms itself)
static inline bool stub_fails_now(int &knob)
{
    if (knob == 0) { knob = -1; return true; }
    if (knob > 0) knob--;
    return false;
}
template <typename T>
static inline hipError_t stub_create(T **out, long &alive, int arg)
{
    *out = nullptr;
    if (stub_fails_now(stub().fail_create_after)) return hipErrorOutOfMemory;
    *out = new T{arg};
    alive++;
    return hipSuccess;
}

static inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "hipSuccess" : e == hipErrorOutOfMemory ? "hipErrorOutOfMemory" : "hipError(stub)"; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipGetDeviceCount(int *n) { *n = getenv("KARIOS_STUB_NO_DEVICE") ? 0 : 1; return hipSuccess; }
static inline hipError_t hipSetDevice(int) { return hipSuccess; }
static inline hipError_t hipDeviceSynchronize() { stub_order::host_join_all(); return hipSuccess; }
static inline hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = 256; return hipSuccess; }
static inline hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) { *lo = 0; *hi = -1; return hipSuccess; }

hipError_t hipMalloc(void **p, size_t n);
hipError_t hipFree(void *p);
hipError_t hipHostMalloc(void **p, size_t n, unsigned flags);
hipError_t hipHostFree(void *p);
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *at, const void *p);
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s);
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t s);
// (blocking: an operation on the null stream, then the host knows it is through - it does not order behind non-blocking streams)
static inline hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind k)
{
    const hipError_t e = hipMemcpyAsync(dst, src, n, k, nullptr);
    stub_order::host_join_stream(nullptr);
    return e;
}
static inline hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t s) { stub_order::op(s, "hipMemsetAsync").write(dst, n); memset(dst, v, n); return hipSuccess; }
static inline hipError_t hipHostRegister(void *, size_t, unsigned) { return hipSuccess; }

static inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return stub_create(s, stub().streams, 0); }
static inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int p) { return stub_create(s, stub().streams, p); }
static inline hipError_t hipStreamDestroy(hipStream_t s) { if (s) stub().streams--; stub_order::on_stream_destroy(s); delete s; return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t s) { stub_order::host_join_stream(s); return hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { if (!e) return hipErrorInvalidValue; stub_order::on_wait(s, e); return hipSuccess; }
static inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return stub_create(e, stub().events, 0); }
static inline hipError_t hipEventCreate(hipEvent_t *e) { return stub_create(e, stub().events, 0); }
static inline hipError_t hipEventDestroy(hipEvent_t e) { if (e) { stub().events--; stub_order::on_event_destroy(e); } delete e; return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { if (!e) return hipErrorInvalidValue; e->recorded++; stub_order::on_record(e, s); return hipSuccess; }
static inline hipError_t hipEventSynchronize(hipEvent_t e) { if (!e) return hipErrorInvalidValue; stub_order::host_join_event(e); return hipSuccess; }
static inline hipError_t hipEventQuery(hipEvent_t e) { if (!e) return hipErrorInvalidValue; stub_order::host_join_event(e); return hipSuccess; }   // (the stand-in executes everything at once: always complete)
static inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) { *ms = 0.f; return a && b ? hipSuccess : hipErrorInvalidValue; }

// Host stand-in for <hip/hip_runtime.h>, for csrc/avsim_io.h, avsim_stage.h, avsim_devbuf.h and avsim_dev.h alone (tests/hostshim_io/io_main.cpp and dev_main.cpp,
// tests/test_io_host.py and test_dev_host.py): the runtime calls those headers make, over malloc and memcpy.  Copies execute at once, every call is
// counted, and the n-th hipMalloc / hipHostMalloc / copy / event creation / elapsed-time read can be told to fail.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1, hipErrorLaunchFailure = 719 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef struct fake_stream* hipStream_t;
typedef struct fake_event* hipEvent_t;
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2;

struct FakeHip {
    // calls made so far
    int mallocs = 0, frees = 0, host_mallocs = 0, host_frees = 0, copies = 0, h2d = 0, d2h = 0, events = 0, event_destroys = 0, records = 0, event_syncs = 0, stream_syncs = 0, memsets = 0, elapsed = 0;
    size_t d2h_bytes = 0, last_d2h_bytes = 0, last_malloc_bytes = 0;
    const void* last_d2h_dst = nullptr;
    // the k-th call from now fails (1: the next one); 0: none
    int fail_malloc = 0, fail_host_malloc = 0, fail_copy = 0, fail_sync = 0, fail_event = 0, fail_elapsed = 0;
    int total() const { return mallocs + frees + host_mallocs + host_frees + copies + events + event_destroys + records + event_syncs + stream_syncs + memsets + elapsed; }
};
inline FakeHip g_hip;
inline bool fake_hits(int& countdown) { return countdown > 0 && --countdown == 0; }

inline const char* hipGetErrorString(hipError_t e) {
    return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorLaunchFailure ? "unspecified launch failure" : "invalid argument";
}
inline hipError_t hipMalloc(void** p, size_t bytes) {
    g_hip.mallocs++;
    g_hip.last_malloc_bytes = bytes;
    if (fake_hits(g_hip.fail_malloc)) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes ? bytes : 1);          // (exactly `bytes`: AddressSanitizer sees a copy that runs past a buffer)
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipFree(void* p) { g_hip.frees++; std::free(p); return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    g_hip.host_mallocs++;
    if (fake_hits(g_hip.fail_host_malloc)) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes ? bytes : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipHostFree(void* p) { g_hip.host_frees++; std::free(p); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    g_hip.copies++;
    if (fake_hits(g_hip.fail_copy)) return hipErrorLaunchFailure;
    if (kind == hipMemcpyHostToDevice) g_hip.h2d++;
    else { g_hip.d2h++; g_hip.d2h_bytes += bytes; g_hip.last_d2h_bytes = bytes; g_hip.last_d2h_dst = dst; }
    if (bytes) std::memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { return hipMemcpyAsync(dst, src, bytes, kind, nullptr); }
inline hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) { g_hip.memsets++; std::memset(p, v, bytes); return hipSuccess; }
inline hipError_t hipEventCreate(hipEvent_t* e) {
    g_hip.events++;
    if (fake_hits(g_hip.fail_event)) { *e = nullptr; return hipErrorOutOfMemory; }
    *e = (hipEvent_t)std::malloc(1);
    return hipSuccess;
}
// every pair took a quarter of a millisecond: sums of them are exact in binary
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
    g_hip.elapsed++;
    if (fake_hits(g_hip.fail_elapsed)) return hipErrorInvalidValue;
    *ms = 0.25f;
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { g_hip.events++; *e = (hipEvent_t)std::malloc(1); return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { g_hip.event_destroys++; std::free(e); return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { g_hip.records++; return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t) { g_hip.event_syncs++; return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) {
    g_hip.stream_syncs++;
    return fake_hits(g_hip.fail_sync) ? hipErrorLaunchFailure : hipSuccess;
}

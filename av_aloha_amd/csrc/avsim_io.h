// avsim_io.h -- how an entry point of avsim_api.hip gets a call's arrays onto the device and its results back: a pool of device buffers the handle
// owns (IoPool) and one object per call, built on the stack at the top of an entry point (IoCall).  Host code only, like avsim_stage.h.
//
// Device I/O mode: the caller's pointers ARE device pointers; every operation hands them back and makes no HIP call (scratch apart).
// Host I/O mode: the k-th array a call stages lives in pool buffer k, inputs are copied up where they are named, outputs are remembered and copied
// back by finish(), which then synchronises the stream -- so the next call may take the same buffers again.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "avsim_devbuf.h"

namespace avs {

struct IoPool {
    // the most arrays one call stages: avsim_obs_history_push with 8 cameras (ids, elapsed, state, its history, a batch and a history per camera)
    static constexpr int NBUF = 20;
    // Large results to pageable host memory (the images of avsim_render_*: 0.9 MB per 480 x 640 colour view).  hipMemcpy into pageable memory
    // runs at ~5 GB/s here (measured: 354 MB of pixels in 66 of the 73 ms of a 64-env gym step).  From 16 MB the copy is pipelined instead: the
    // device buffer goes in 32 MB chunks by DMA into two pinned staging buffers while the previous chunk is copied on into the caller's memory by
    // four threads.
    static constexpr size_t PIPELINE_FROM = (size_t)16 << 20, PIN_CHUNK = (size_t)32 << 20;
    static constexpr int COPY_THREADS = 4;

    DevBuf own[NBUF];          // grow-only, each as large as the largest array it has served
    void* buf[NBUF] = {};      // own[k]'s pointer and capacity as grow() and destroy() left them: what the calls (and tests/hostshim_io) read
    size_t cap[NBUF] = {};
    void* pin[2] = {};
    hipEvent_t pin_ev[2] = {};

    void destroy() {
        for (int k = 0; k < NBUF; k++) {
            own[k].free();
            buf[k] = nullptr;
            cap[k] = 0;
        }
        for (int k = 0; k < 2; k++) {
            if (pin[k]) (void)hipHostFree(pin[k]);
            if (pin_ev[k]) (void)hipEventDestroy(pin_ev[k]);
            pin[k] = nullptr;
            pin_ev[k] = nullptr;
        }
    }

    // buffer k, at least `bytes` large; empty after a failure
    hipError_t grow(int k, size_t bytes) {
        const hipError_t e = own[k].reserve(bytes);
        buf[k] = own[k].ptr();
        cap[k] = own[k].cap();
        return e;
    }

    // the two pinned chunks and their events, made at the first large result; false: there is no pinned memory to have (the plain copy serves)
    bool pinned() {
        for (int k = 0; k < 2; k++) {
            if (!pin[k] && hipHostMalloc(&pin[k], PIN_CHUNK, hipHostMallocDefault) != hipSuccess) { pin[k] = nullptr; return false; }
            if (!pin_ev[k] && hipEventCreateWithFlags(&pin_ev[k], hipEventDisableTiming) != hipSuccess) { pin_ev[k] = nullptr; return false; }
        }
        return true;
    }

    // `bytes` at device address `src` into pageable `dst` through the pinned chunks; synchronous.  Call pinned() first
    hipError_t copy_out_pipelined(const char* src, char* dst, size_t bytes, hipStream_t stream) {
        const size_t nchunk = (bytes + PIN_CHUNK - 1) / PIN_CHUNK;
        auto issue = [&](size_t c) -> hipError_t {
            const size_t off = c * PIN_CHUNK, n = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
            hipError_t e = hipMemcpyAsync(pin[c & 1], src + off, n, hipMemcpyDeviceToHost, stream);
            return e != hipSuccess ? e : hipEventRecord(pin_ev[c & 1], stream);
        };
        hipError_t e = issue(0);
        for (size_t c = 0; c < nchunk && e == hipSuccess; c++) {
            if ((e = hipEventSynchronize(pin_ev[c & 1])) != hipSuccess) break;
            if (c + 1 < nchunk && (e = issue(c + 1)) != hipSuccess) break;          // (the other buffer: its previous contents were copied out in the last round)
            const size_t off = c * PIN_CHUNK, n = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
            const char* from = (const char*)pin[c & 1];
            const size_t part = ((n + COPY_THREADS - 1) / COPY_THREADS + 4095) & ~(size_t)4095;
            std::thread th[COPY_THREADS - 1];
            int started = 0;
            for (int t = 1; t < COPY_THREADS; t++) {
                const size_t a = (size_t)t * part;
                if (a >= n) break;
                const size_t m = n - a < part ? n - a : part;
                th[started++] = std::thread([=] { std::memcpy(dst + off + a, from + a, m); });
            }
            std::memcpy(dst + off, from, n < part ? n : part);
            for (int t = 0; t < started; t++) th[t].join();
        }
        return e;
    }
};

// One call's arrays.  An error is sticky: after a HIP call has failed, every operation returns nullptr and enqueues nothing, `err` says which call
// failed and why, and finish() returns the code.  An entry point asks failed() once before it launches and returns what finish() gives.
class IoCall {
public:
    IoCall(IoPool& pool, hipStream_t stream, bool device_mode, std::string& err) : pool_(pool), stream_(stream), device_(device_mode), err_(err) {}
    IoCall(const IoCall&) = delete;
    IoCall& operator=(const IoCall&) = delete;

    hipError_t failed() const { return e_; }

    // an input: the device pointer that holds `bytes` of `p`.  A null `p` (an optional input) gives nullptr and no copy
    template <typename T>
    const T* in(const T* p, size_t bytes) {
        if (!p || e_ != hipSuccess) return nullptr;
        if (device_) return p;
        return static_cast<const T*>(upload(take(bytes), p, bytes));
    }
    // an output: the device pointer the kernels write `bytes` to; a host caller's `p` gets them in finish().  A null `p` (an output nobody asked
    // for) gives `own`, a buffer of the handle's or nullptr, and no copy
    template <typename T>
    T* out(T* p, size_t bytes, T* own = nullptr) {
        if (e_ != hipSuccess) return nullptr;
        if (!p) return own;
        if (device_) return p;
        void* d = take(bytes);
        if (e_ == hipSuccess) outs_[nout_++] = Out{p, d, bytes};          // (take() has counted it: nout_ <= used_ <= NBUF)
        return static_cast<T*>(d);
    }
    // an array the kernels update in place: an output whose present contents go up first
    template <typename T>
    T* inout(T* p, size_t bytes) {
        T* d = out(p, bytes);
        if (d && !device_) upload(d, p, bytes);
        return e_ == hipSuccess ? d : nullptr;
    }
    // device memory of the call's own, in either mode (stream-ordered in device mode: the call before has the same stream)
    void* scratch(size_t bytes) { return e_ == hipSuccess ? take(bytes) : nullptr; }

    // host mode: the outputs back, in the order they were named, and the stream synchronised; device mode: nothing.  The first error of the call
    hipError_t finish() {
        if (e_ != hipSuccess || device_) return e_;
        for (int i = 0; i < nout_ && e_ == hipSuccess; i++) {
            const Out& o = outs_[i];
            if (o.bytes >= IoPool::PIPELINE_FROM && pool_.pinned())
                check(pool_.copy_out_pipelined((const char*)o.dev, (char*)o.host, o.bytes, stream_), "D2H copy");
            else
                check(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, stream_), "D2H copy");
        }
        nout_ = 0;
        if (e_ == hipSuccess) check(hipStreamSynchronize(stream_), "stream sync");
        return e_;
    }

private:
    struct Out {
        void* host;
        const void* dev;
        size_t bytes;
    };
    IoPool& pool_;
    hipStream_t stream_;
    const bool device_;
    std::string& err_;
    hipError_t e_ = hipSuccess;
    int used_ = 0, nout_ = 0;
    Out outs_[IoPool::NBUF];

    void check(hipError_t e, const char* what, size_t bytes = 0) {
        if (e == hipSuccess || e_ != hipSuccess) return;
        e_ = e;
        char msg[256];
        if (bytes) snprintf(msg, sizeof msg, "%s(%zu) failed: %s", what, bytes, hipGetErrorString(e));
        else snprintf(msg, sizeof msg, "%s failed: %s", what, hipGetErrorString(e));
        err_ = msg;
    }
    // the call's next pool buffer, at least `bytes` large
    void* take(size_t bytes) {
        if (used_ == IoPool::NBUF) {
            e_ = hipErrorOutOfMemory;
            err_ = "a call stages more arrays than the pool has buffers";
            return nullptr;
        }
        const int k = used_++;
        if (pool_.cap[k] < bytes) check(pool_.grow(k, bytes), "hipMalloc", bytes);
        return e_ == hipSuccess ? pool_.buf[k] : nullptr;
    }
    void* upload(void* d, const void* p, size_t bytes) {
        if (e_ != hipSuccess) return nullptr;
        check(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, stream_), "H2D copy");
        return e_ == hipSuccess ? d : nullptr;
    }
};

}  // namespace avs

// avsim_dev.h -- who owns device memory and timing events in libavsim's host code: one allocation that grows on demand (DevBuf, avsim_devbuf.h), the
// allocations of one set-up, freed together (DevArena), and the event pairs around a launch (EventTimer).  Each is movable, not copyable, and releases
// what it holds in its destructor; none makes a message -- the caller knows what the memory was for.  Host code only, like avsim_io.h and avsim_stage.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

#include "avsim_devbuf.h"

namespace avs {

constexpr size_t EV_RING = 1024;      // HIP event pairs an EventTimer keeps before it folds them into its running sum

// The allocations of one set-up.  The error is sticky: after the first failure every call returns nullptr and makes no runtime call, error() says
// which code it was; a set-up asks once at its end.  clear() frees everything and forgets the error
class DevArena {
public:
    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    DevArena(DevArena&& o) noexcept : blocks_(std::move(o.blocks_)), e_(std::exchange(o.e_, hipSuccess)) { o.blocks_.clear(); }
    DevArena& operator=(DevArena&& o) noexcept {
        if (this != &o) { clear(); blocks_ = std::move(o.blocks_); o.blocks_.clear(); e_ = std::exchange(o.e_, hipSuccess); }
        return *this;
    }
    ~DevArena() { clear(); }

    hipError_t error() const { return e_; }
    bool empty() const { return blocks_.empty(); }

    void* get(size_t bytes) {
        if (e_ != hipSuccess) return nullptr;
        void* p = nullptr;
        if ((e_ = hipMalloc(&p, bytes ? bytes : 1)) != hipSuccess) return nullptr;
        blocks_.push_back(p);
        return p;
    }
    void* zeroed(size_t bytes, hipStream_t stream) {
        void* p = get(bytes);
        if (p && (e_ = hipMemsetAsync(p, 0, bytes ? bytes : 1, stream)) != hipSuccess) return nullptr;
        return p;
    }
    // synchronous: `v` may go out of scope behind the call
    template <typename T>
    T* upload(const std::vector<T>& v) {
        void* p = get(v.size() * sizeof(T));
        if (p && !v.empty() && (e_ = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess) return nullptr;
        return static_cast<T*>(p);
    }
    void clear() {
        for (void* p : blocks_) (void)hipFree(p);
        blocks_.clear();
        e_ = hipSuccess;
    }

private:
    std::vector<void*> blocks_;
    hipError_t e_ = hipSuccess;
};

// Pairs of events recorded around a launch on its stream, and their elapsed times summed when somebody asks: read() waits for the pairs, begin()
// and end() never do -- except once per EV_RING pairs, when the pairs held are folded into the running sum so that a long run does not grow the list
class EventTimer {
public:
    EventTimer() = default;
    EventTimer(const EventTimer&) = delete;
    EventTimer& operator=(const EventTimer&) = delete;
    EventTimer(EventTimer&& o) noexcept : ev_(std::move(o.ev_)), used_(o.used_), open_(o.open_), ms_(o.ms_), n_(o.n_) { o.ev_.clear(); o.forget(); }
    EventTimer& operator=(EventTimer&& o) noexcept {
        if (this != &o) { destroy(); ev_ = std::move(o.ev_); used_ = o.used_; open_ = o.open_; ms_ = o.ms_; n_ = o.n_; o.ev_.clear(); o.forget(); }
        return *this;
    }
    ~EventTimer() { destroy(); }

    // the first event of a pair.  The pair counts once end() has recorded the second: a begin() whose launch failed leaves nothing behind
    hipError_t begin(hipStream_t stream) {
        open_ = false;
        hipError_t e = hipSuccess;
        if (used_ >= 2 * EV_RING && (e = fold()) != hipSuccess) return e;
        while (ev_.size() < used_ + 2) {
            hipEvent_t ev;
            if ((e = hipEventCreate(&ev)) != hipSuccess) return e;
            ev_.push_back(ev);
        }
        if ((e = hipEventRecord(ev_[used_], stream)) == hipSuccess) open_ = true;
        return e;
    }
    hipError_t end(hipStream_t stream) {
        if (!open_) return hipSuccess;
        open_ = false;
        const hipError_t e = hipEventRecord(ev_[used_ + 1], stream);
        if (e == hipSuccess) used_ += 2;
        return e;
    }
    // the sum over every complete pair since the last reset, in milliseconds, and their number (either may be null); waits for the pairs held
    hipError_t read(bool reset, double* total_ms, long long* launches) {
        double tot = 0;
        const hipError_t e = sum(tot);
        if (e != hipSuccess) return e;
        if (total_ms) *total_ms = tot + ms_;
        if (launches) *launches = (long long)(used_ / 2) + n_;
        if (reset) forget();
        return hipSuccess;
    }

private:
    std::vector<hipEvent_t> ev_;
    size_t used_ = 0;      // events of complete pairs
    bool open_ = false;    // ev_[used_] is recorded and waits for its partner
    double ms_ = 0;        // folded out of the list
    long long n_ = 0;

    hipError_t sum(double& tot) {
        for (size_t i = 0; i + 1 < used_; i += 2) {
            float ms = 0;
            hipError_t e = hipEventSynchronize(ev_[i + 1]);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev_[i], ev_[i + 1]);
            if (e != hipSuccess) return e;
            tot += ms;
        }
        return hipSuccess;
    }
    hipError_t fold() {
        double tot = 0;
        const hipError_t e = sum(tot);
        if (e != hipSuccess) return e;
        ms_ += tot;
        n_ += (long long)(used_ / 2);
        used_ = 0;
        return hipSuccess;
    }
    void forget() { used_ = 0; open_ = false; ms_ = 0; n_ = 0; }
    void destroy() {
        for (hipEvent_t ev : ev_) (void)hipEventDestroy(ev);
        ev_.clear();
        forget();
    }
};

}  // namespace avs

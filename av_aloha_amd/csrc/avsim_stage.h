// avsim_stage.h -- pinned staging of the per-call host arrays of avsim_image_prep, avsim_image_jitter, avsim_image_augment and avsim_image_resize: four slots of pinned and of device
// memory, reused behind events.  Host code only (avsim_imgaug.hip.h, which a unit of other flags reads too, includes it).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "avsim_devbuf.h"

namespace avs {

struct StageRing {
    static constexpr int NSLOT = 4;
    struct Slot {
        void* pin = nullptr;
        DevBuf dev;
        size_t cap = 0;      // of either
        hipEvent_t done = nullptr;
        bool busy = false;
    };
    Slot slot[NSLOT];
    int next = 0;

    void destroy() {
        for (auto& s : slot) {
            if (s.busy) (void)hipEventSynchronize(s.done);
            if (s.pin) (void)hipHostFree(s.pin);
            if (s.done) (void)hipEventDestroy(s.done);
            s = Slot{};
        }
    }

    // the next slot, idle (its last call's event waited for) and holding at least `bytes` of pinned and of device memory; nullptr: HIP, err says what
    Slot* acquire(size_t bytes, std::string& err) {
        Slot& s = slot[next];
        next = (next + 1) % NSLOT;
        hipError_t e = hipSuccess;
        if (s.busy) e = hipEventSynchronize(s.done);      // (the call four calls back: long done in a training loop)
        s.busy = false;
        if (e == hipSuccess && s.cap < bytes) {
            if (s.pin) (void)hipHostFree(s.pin);
            s.pin = nullptr;
            s.cap = 0;
            const size_t cap = (bytes + 4095) & ~(size_t)4095;
            e = hipHostMalloc(&s.pin, cap, hipHostMallocDefault);
            if (e == hipSuccess) e = s.dev.reserve(cap);
            if (e == hipSuccess) s.cap = cap;
        }
        if (e == hipSuccess && !s.done) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        if (e != hipSuccess) { err = std::string("image staging ring: ") + hipGetErrorString(e); return nullptr; }
        return &s;
    }

    // the slot's pinned bytes to its device copy, on `stream`.  -3: HIP (nothing is in flight, the slot stays idle)
    int upload(Slot& s, size_t bytes, hipStream_t stream, std::string& err) {
        const hipError_t e = hipMemcpyAsync(s.dev.ptr(), s.pin, bytes, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) err = std::string("image staging ring: ") + hipGetErrorString(e);
        return e == hipSuccess ? 0 : -3;
    }

    // after upload and the kernels that read the slot were put on `stream`: the slot is busy until they have run.  Also after a launch that
    // failed -- the copy may be in flight.  -3: HIP
    int release(Slot& s, hipStream_t stream, std::string& err) {
        const hipError_t e = hipEventRecord(s.done, stream);
        s.busy = e == hipSuccess;
        if (e != hipSuccess) err = std::string("image staging ring: ") + hipGetErrorString(e);
        return e == hipSuccess ? 0 : -3;
    }
};

}  // namespace avs

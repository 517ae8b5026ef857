// avsim_devbuf.h -- DevBuf, the first of the three owners of avsim_dev.h, in a header of its own: avsim_io.h and avsim_stage.h need it alone, and with it
// no runtime call beyond hipMalloc and hipFree (the stand-in runtime of tests/hostshim_io serves them as it always has).  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace avs {

class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { free(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
        return *this;
    }
    ~DevBuf() { free(); }

    // at least `bytes`: nothing when the block is large enough, else the old block freed (hipFree waits for the kernels that still use it) and
    // exactly `bytes` allocated (0: one byte).  After a failure the buffer is empty
    hipError_t reserve(size_t bytes) { return p_ && cap_ >= bytes ? hipSuccess : alloc(bytes); }
    // exactly `bytes`, whatever was held
    hipError_t alloc(size_t bytes) {
        free();
        if (!bytes) bytes = 1;
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = bytes;
        return e;
    }
    void free() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }

    void* ptr() const { return p_; }
    size_t cap() const { return cap_; }
    template <typename T>
    T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void* p_ = nullptr;
    size_t cap_ = 0;      // bytes
};

}  // namespace avs

// csrc/avsim_io.h against the counting runtime of tests/hostshim_io/hip/hip_runtime.h: a program of its own (tests/test_io_host.py builds it with
// AddressSanitizer, LeakSanitizer and UBSan and runs it).  A "kernel" here is host code that reads and writes the "device" pointers a call hands out.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "avsim_io.h"

using avs::IoCall;
using avs::IoPool;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static std::vector<uint8_t> pattern(size_t n, unsigned seed) {
    std::vector<uint8_t> v(n);
    uint32_t x = seed * 2654435761u + 1;
    for (size_t i = 0; i < n; i++) { x = x * 1664525u + 1013904223u; v[i] = (uint8_t)(x >> 24); }
    return v;
}

static void device_mode() {
    g_hip = FakeHip{};
    IoPool pool;
    std::string err;
    uint8_t a[16], o[16], x[16], own[16];
    {
        IoCall io(pool, nullptr, true, err);
        CHECK(io.in(a, sizeof a) == a);
        CHECK(io.in((const uint8_t*)nullptr, 16) == nullptr);
        CHECK(io.out(o, sizeof o) == o);
        CHECK(io.out((uint8_t*)nullptr, 16) == nullptr);
        CHECK(io.out((uint8_t*)nullptr, 16, own) == own);
        CHECK(io.out(o, sizeof o, own) == o);
        CHECK(io.inout(x, sizeof x) == x);
        CHECK(io.failed() == hipSuccess);
        CHECK(io.finish() == hipSuccess);
        CHECK(g_hip.total() == 0);          // the speed invariant: device mode makes no HIP call
    }
    for (size_t bytes : {(size_t)100, (size_t)100, (size_t)40}) {          // scratch: allocated once, then served from the pool
        IoCall io(pool, nullptr, true, err);
        CHECK(io.scratch(bytes) == pool.buf[0] && pool.buf[0]);
        CHECK(io.finish() == hipSuccess);
        CHECK(g_hip.mallocs == 1 && g_hip.total() == 1);
    }
    pool.destroy();
    CHECK(g_hip.frees == 1);
}

static void host_mode() {
    g_hip = FakeHip{};
    IoPool pool;
    std::string err;
    const auto a = pattern(300, 1), x0 = pattern(77, 2);
    std::vector<uint8_t> o(300, 0xee), x = x0, own(8, 0x11);
    IoCall io(pool, nullptr, false, err);
    const uint8_t* da = io.in(a.data(), a.size());
    CHECK(da && da != a.data() && !std::memcmp(da, a.data(), a.size()));          // the input has arrived
    CHECK(g_hip.h2d == 1);
    CHECK(io.in((const uint8_t*)nullptr, 300) == nullptr && g_hip.total() == 2);          // (one hipMalloc, one copy: a null optional adds nothing)
    uint8_t* dout = io.out(o.data(), o.size());
    CHECK(dout && dout != o.data() && dout != da);
    CHECK(io.out((uint8_t*)nullptr, 8, own.data()) == own.data());
    CHECK(io.out((uint8_t*)nullptr, 8) == nullptr);
    uint8_t* dx = io.inout(x.data(), x.size());
    CHECK(dx && dx != x.data() && !std::memcmp(dx, x0.data(), x0.size()));          // in-out: the present contents went up
    CHECK(g_hip.h2d == 2 && g_hip.mallocs == 3);
    for (size_t i = 0; i < o.size(); i++) dout[i] = da[i] ^ 0x5a;
    for (size_t i = 0; i < x.size(); i++) dx[i] = (uint8_t)(dx[i] + 1);
    CHECK(g_hip.d2h == 0 && g_hip.stream_syncs == 0 && o[0] == 0xee && x == x0);          // nothing comes back before finish()
    CHECK(io.finish() == hipSuccess);
    CHECK(g_hip.d2h == 2 && g_hip.d2h_bytes == o.size() + x.size() && g_hip.stream_syncs == 1);          // each output once, with its byte count
    for (size_t i = 0; i < o.size(); i++) CHECK(o[i] == (a[i] ^ 0x5a));
    for (size_t i = 0; i < x.size(); i++) CHECK(x[i] == (uint8_t)(x0[i] + 1));
    CHECK(own == std::vector<uint8_t>(8, 0x11));
    CHECK(g_hip.copies == 4 && err.empty());
    pool.destroy();
    CHECK(g_hip.frees == 3);
}

// three calls whose k-th arrays are small, larger, small: the pool reallocates for the larger one only
static void reuse_and_growth() {
    g_hip = FakeHip{};
    IoPool pool;
    std::string err;
    const size_t sizes[3][2] = {{100, 260}, {5000, 7001}, {90, 33}};
    const int mallocs_after[3] = {2, 4, 4}, frees_after[3] = {0, 2, 2};
    for (int r = 0; r < 3; r++) {
        const auto a = pattern(sizes[r][0], 10 + r);
        std::vector<uint8_t> o(sizes[r][1]);
        IoCall io(pool, nullptr, false, err);
        const uint8_t* da = io.in(a.data(), a.size());
        uint8_t* dout = io.out(o.data(), o.size());
        CHECK(io.failed() == hipSuccess && da == pool.buf[0] && dout == pool.buf[1]);          // the k-th array of a call: pool buffer k
        for (size_t i = 0; i < o.size(); i++) dout[i] = (uint8_t)(da[i % a.size()] + i);
        CHECK(io.finish() == hipSuccess);
        for (size_t i = 0; i < o.size(); i++) CHECK(o[i] == (uint8_t)(a[i % a.size()] + i));
        CHECK(g_hip.mallocs == mallocs_after[r] && g_hip.frees == frees_after[r]);
        CHECK(g_hip.last_d2h_bytes == o.size());
    }
    CHECK(pool.cap[0] == 5000 && pool.cap[1] == 7001);
    pool.destroy();
}

// results from 16 MB: two pinned 32 MB chunks; 33 MB + 5 bytes span both and end ragged
static void large_outputs() {
    const size_t big = ((size_t)33 << 20) + 5;
    const auto want = pattern(big, 99);
    for (int pinned = 1; pinned >= 0; pinned--) {
        g_hip = FakeHip{};
        g_hip.fail_host_malloc = pinned ? 0 : 2;          // (the second chunk cannot be had: the plain copy serves)
        IoPool pool;
        std::string err;
        std::vector<uint8_t> o(big, 0);
        IoCall io(pool, nullptr, false, err);
        uint8_t* d = io.out(o.data(), big);
        CHECK(d);
        std::memcpy(d, want.data(), big);
        CHECK(io.finish() == hipSuccess && err.empty());
        CHECK(o == want);
        if (pinned) CHECK(g_hip.host_mallocs == 2 && g_hip.events == 2 && g_hip.d2h == 2 && g_hip.records == 2 && g_hip.event_syncs == 2 && g_hip.d2h_bytes == big);
        else CHECK(g_hip.host_mallocs == 2 && g_hip.d2h == 1 && g_hip.d2h_bytes == big && g_hip.last_d2h_dst == o.data());
        CHECK(g_hip.stream_syncs == 1);
        pool.destroy();
        CHECK(g_hip.host_frees == (pinned ? 2 : 1) && g_hip.event_destroys == g_hip.events && g_hip.frees == 1);
    }
    // the threshold itself: 16 MB takes the pinned path (one chunk), a byte less the plain copy
    for (int below = 0; below < 2; below++) {
        g_hip = FakeHip{};
        const size_t n = ((size_t)16 << 20) - below;
        IoPool pool;
        std::string err;
        std::vector<uint8_t> o(n, 0);
        IoCall io(pool, nullptr, false, err);
        uint8_t* d = io.out(o.data(), n);
        CHECK(d);
        std::memcpy(d, want.data(), n);
        CHECK(io.finish() == hipSuccess);
        CHECK(!std::memcmp(o.data(), want.data(), n));
        CHECK(g_hip.host_mallocs == (below ? 0 : 2) && g_hip.d2h == 1 && g_hip.last_d2h_dst == (below ? (void*)o.data() : pool.pin[0]));
        pool.destroy();
    }
    // a copy that fails in the middle of the pinned path is the call's error
    {
        g_hip = FakeHip{};
        g_hip.fail_copy = 2;
        IoPool pool;
        std::string err;
        std::vector<uint8_t> o(big, 0);
        IoCall io(pool, nullptr, false, err);
        CHECK(io.out(o.data(), big));
        CHECK(io.finish() == hipErrorLaunchFailure);
        CHECK(err.find("D2H copy") != std::string::npos && err.find(hipGetErrorString(hipErrorLaunchFailure)) != std::string::npos);
        CHECK(g_hip.stream_syncs == 0);
        pool.destroy();
    }
}

// One call that uses every operation -- 5 hipMalloc, 3 copies up, 2 back, 1 synchronisation -- with a failure injected at each of them in turn: the
// call returns the HIP code, the message names the operation, nothing is enqueued after the failure, destroy() leaves nothing behind (LeakSanitizer)
static void injected_failures() {
    enum { MALLOC, COPY, SYNC };
    struct Case { int what, nth; hipError_t code; const char* names; };
    const Case cases[] = {
        {MALLOC, 1, hipErrorOutOfMemory, "hipMalloc(64)"}, {MALLOC, 2, hipErrorOutOfMemory, "hipMalloc(32)"}, {MALLOC, 3, hipErrorOutOfMemory, "hipMalloc(48)"},
        {MALLOC, 4, hipErrorOutOfMemory, "hipMalloc(16)"}, {MALLOC, 5, hipErrorOutOfMemory, "hipMalloc(128)"},
        {COPY, 1, hipErrorLaunchFailure, "H2D copy"}, {COPY, 2, hipErrorLaunchFailure, "H2D copy"}, {COPY, 3, hipErrorLaunchFailure, "H2D copy"},
        {COPY, 4, hipErrorLaunchFailure, "D2H copy"}, {COPY, 5, hipErrorLaunchFailure, "D2H copy"}, {SYNC, 1, hipErrorLaunchFailure, "stream sync"},
    };
    for (int warm = 0; warm < 2; warm++)          // a fresh pool, and one whose buffers are too small (growth: hipFree, then the hipMalloc that fails)
        for (const Case& c : cases) {
            g_hip = FakeHip{};
            IoPool pool;
            std::string err;
            if (warm) {
                IoCall io(pool, nullptr, false, err);
                for (int k = 0; k < 5; k++) CHECK(io.scratch(8));
                CHECK(io.finish() == hipSuccess);
                g_hip = FakeHip{};
            }
            (c.what == MALLOC ? g_hip.fail_malloc : c.what == COPY ? g_hip.fail_copy : g_hip.fail_sync) = c.nth;
            uint8_t a[64] = {1}, b[32] = {2}, o[48] = {3}, x[16] = {4};
            int at_failure = -1;
            bool failed_before = false;
            IoCall io(pool, nullptr, false, err);
            auto step = [&](const void* got) {
                if (failed_before) CHECK(got == nullptr && g_hip.total() == at_failure);          // sticky: nullptr, and nothing more is enqueued
                else if (io.failed() != hipSuccess) { CHECK(got == nullptr); failed_before = true; at_failure = g_hip.total(); }
                else CHECK(got != nullptr);
            };
            step(io.in(a, sizeof a));
            step(io.in(b, sizeof b));
            step(io.out(o, sizeof o));
            step(io.inout(x, sizeof x));
            step(io.scratch(128));
            const bool in_finish = !failed_before;
            CHECK(io.finish() == c.code);
            CHECK(io.finish() == c.code && io.failed() == c.code);
            if (!in_finish) CHECK(g_hip.total() == at_failure);
            else CHECK(g_hip.d2h == (c.what == SYNC ? 2 : c.nth - 4) && g_hip.stream_syncs == (c.what == SYNC ? 1 : 0));
            CHECK(err.find(c.names) != std::string::npos && err.find("failed: ") != std::string::npos);
            CHECK(err.find(hipGetErrorString(c.code)) != std::string::npos);
            if (!in_finish) CHECK(o[0] == 3 && x[0] == 4);          // (no output comes back from a call that failed before its copies)
            pool.destroy();
            for (int k = 0; k < IoPool::NBUF; k++) CHECK(!pool.buf[k] && !pool.cap[k]);
        }
    // more arrays than the pool has buffers: an error, not a write past the tables
    {
        g_hip = FakeHip{};
        IoPool pool;
        std::string err;
        IoCall io(pool, nullptr, false, err);
        for (int k = 0; k < IoPool::NBUF; k++) CHECK(io.scratch(4));
        CHECK(io.scratch(4) == nullptr && io.failed() != hipSuccess && !err.empty());
        CHECK(io.finish() != hipSuccess);
        pool.destroy();
    }
}

int main() {
    device_mode();
    host_mode();
    reuse_and_growth();
    large_outputs();
    injected_failures();
    std::puts("io ok");
    return 0;
}

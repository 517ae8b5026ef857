// csrc/avsim_dev.h (DevBuf, DevArena, EventTimer) and the staging ring of csrc/avsim_stage.h against the counting runtime of
// tests/hostshim_io/hip/hip_runtime.h: a program of its own (tests/test_dev_host.py builds it with AddressSanitizer, LeakSanitizer and UBSan and runs
// it).  "Device" memory is malloc's, allocated exactly: a write one byte past a buffer is AddressSanitizer's to catch, a lost block LeakSanitizer's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "avsim_dev.h"
#include "avsim_stage.h"

using avs::DevArena;
using avs::DevBuf;
using avs::EV_RING;
using avs::EventTimer;
using avs::StageRing;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static void fill(const DevBuf& b) { std::memset(b.ptr(), 0xa5, b.cap()); }          // every byte the buffer says it has

static void devbuf() {
    g_hip = FakeHip{};
    {
        DevBuf b;
        CHECK(!b && b.ptr() == nullptr && b.cap() == 0);
        CHECK(b.reserve(100) == hipSuccess && b && b.cap() == 100);
        CHECK(g_hip.mallocs == 1 && g_hip.frees == 0 && g_hip.last_malloc_bytes == 100);
        fill(b);
        void* const p = b.ptr();
        for (size_t bytes : {(size_t)100, (size_t)40, (size_t)0}) {          // smaller or equal: no runtime call
            CHECK(b.reserve(bytes) == hipSuccess && b.ptr() == p && b.cap() == 100);
            CHECK(g_hip.total() == 1);
        }
        CHECK(b.reserve(101) == hipSuccess && b.cap() == 101);          // larger: one free, one malloc of exactly that size
        CHECK(g_hip.mallocs == 2 && g_hip.frees == 1 && g_hip.total() == 3 && g_hip.last_malloc_bytes == 101);
        fill(b);
        CHECK(b.as<uint8_t>()[100] == 0xa5);
        CHECK(b.alloc(101) == hipSuccess && b.cap() == 101);          // alloc: always, also the same size and a smaller one
        CHECK(g_hip.mallocs == 3 && g_hip.frees == 2);
        CHECK(b.alloc(7) == hipSuccess && b.cap() == 7 && g_hip.last_malloc_bytes == 7);
        CHECK(g_hip.mallocs == 4 && g_hip.frees == 3);
        fill(b);
        b.free();
        CHECK(!b && b.cap() == 0 && g_hip.frees == 4);
        b.free();
        CHECK(g_hip.frees == 4);
        CHECK(b.reserve(0) == hipSuccess && b && b.cap() == 1 && g_hip.last_malloc_bytes == 1);          // zero bytes: one
        fill(b);
    }
    CHECK(g_hip.mallocs == 5 && g_hip.frees == 5);          // destruction frees once

    // an injected failure, on a fresh buffer and on a held one: empty afterwards, nothing leaks, the next reserve works
    for (int held = 0; held < 2; held++)
        for (int use_alloc = 0; use_alloc < 2; use_alloc++) {
            g_hip = FakeHip{};
            {
                DevBuf b;
                if (held) { CHECK(b.reserve(64) == hipSuccess); fill(b); }
                g_hip.fail_malloc = 1;
                CHECK((use_alloc ? b.alloc(256) : b.reserve(256)) == hipErrorOutOfMemory);
                CHECK(!b && b.ptr() == nullptr && b.cap() == 0);
                CHECK(g_hip.frees == held);          // (the held block went before the allocation that failed)
                CHECK(b.reserve(32) == hipSuccess && b && b.cap() == 32);          // not "32 <= a capacity that is no longer there"
                fill(b);
                CHECK(b.reserve(256) == hipSuccess && b.cap() == 256);
                fill(b);
            }
            CHECK(g_hip.mallocs == g_hip.frees + 1);          // (the failed call is counted, and it allocated nothing)
        }

    // moves: the source is empty and frees nothing; a buffer moved onto frees what it held
    g_hip = FakeHip{};
    {
        DevBuf a;
        CHECK(a.reserve(48) == hipSuccess);
        void* const p = a.ptr();
        DevBuf b(std::move(a));
        CHECK(!a && a.cap() == 0 && b.ptr() == p && b.cap() == 48 && g_hip.total() == 1);
        DevBuf c;
        CHECK(c.reserve(16) == hipSuccess);
        c = std::move(b);
        CHECK(!b && c.ptr() == p && c.cap() == 48 && g_hip.frees == 1);
        fill(c);
        std::vector<DevBuf> v;          // what JpegHost::cache and ComposeHost::tables do: entries that own a table, in a vector that reallocates
        for (int i = 0; i < 9; i++) { DevBuf e; CHECK(e.reserve(8 + i) == hipSuccess); v.push_back(std::move(e)); }
        for (int i = 0; i < 9; i++) { CHECK(v[i].cap() == (size_t)(8 + i)); fill(v[i]); }
        CHECK(g_hip.mallocs == 11 && g_hip.frees == 1);
    }
    CHECK(g_hip.mallocs == 11 && g_hip.frees == 11);
}

// a set-up of ten allocations, as ChunkHost::setup makes: nine zeroed, then the table that is copied
static int setup10(DevArena& a, void* got[10]) {
    int n = 0;
    for (int k = 0; k < 9; k++) n += (got[k] = a.zeroed(16 + 8 * k, nullptr)) != nullptr;
    n += (got[9] = a.upload(std::vector<float>(12, 1.5f))) != nullptr;
    return n;
}

static void devarena() {
    g_hip = FakeHip{};
    {
        DevArena a;
        void* got[10];
        CHECK(setup10(a, got) == 10 && a.error() == hipSuccess);
        CHECK(g_hip.mallocs == 10 && g_hip.memsets == 9 && g_hip.h2d == 1);
        for (int k = 0; k < 9; k++)
            for (int i = 0; i < 16 + 8 * k; i++) CHECK(((uint8_t*)got[k])[i] == 0);
        for (int i = 0; i < 12; i++) CHECK(((float*)got[9])[i] == 1.5f);
        const int before = g_hip.total();
        int* e = a.upload(std::vector<int>());          // empty: one byte, nothing copied
        CHECK(e && g_hip.last_malloc_bytes == 1 && g_hip.total() == before + 1 && g_hip.copies == 1);
        CHECK(a.get(0) && g_hip.last_malloc_bytes == 1);
        a.clear();
        CHECK(g_hip.frees == 12 && a.error() == hipSuccess);
        CHECK(a.get(5));          // reusable after clear(), as the set-ups that run twice on a handle need
    }
    CHECK(g_hip.mallocs == 13 && g_hip.frees == 13);

    for (int nth = 1; nth <= 10; nth++) {          // the nth allocation fails
        g_hip = FakeHip{};
        DevArena a;
        g_hip.fail_malloc = nth;
        void* got[10];
        CHECK(setup10(a, got) == nth - 1);
        for (int k = 0; k < 10; k++) CHECK((got[k] != nullptr) == (k < nth - 1));
        CHECK(a.error() == hipErrorOutOfMemory);
        CHECK(g_hip.mallocs == nth);          // sticky: nothing after the failure reached the runtime
        const int at = g_hip.total();
        CHECK(a.get(8) == nullptr && a.zeroed(8, nullptr) == nullptr && a.upload(std::vector<int>(3, 1)) == nullptr && g_hip.total() == at);
        a.clear();
        CHECK(g_hip.frees == nth - 1 && a.error() == hipSuccess);          // exactly what was allocated
        CHECK(setup10(a, got) == 10);
    }
    {          // a copy that fails is the arena's error too, and its block is the arena's to free
        g_hip = FakeHip{};
        DevArena a;
        g_hip.fail_copy = 1;
        CHECK(a.upload(std::vector<int>(4, 7)) == nullptr && a.error() == hipErrorLaunchFailure);
        CHECK(a.get(4) == nullptr && g_hip.mallocs == 1);
        DevArena b(std::move(a));          // a moved-from arena frees nothing
        a.clear();
        CHECK(g_hip.frees == 0 && b.error() == hipErrorLaunchFailure);
    }
    CHECK(g_hip.frees == 1);
}

static void eventtimer() {
    const long long n = 2 * (long long)EV_RING + 3;
    g_hip = FakeHip{};
    {
        EventTimer t;
        double ms = -1;
        long long cnt = -1;
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && ms == 0 && cnt == 0 && g_hip.total() == 0);
        for (long long i = 0; i < n; i++) {
            CHECK(t.begin(nullptr) == hipSuccess && t.end(nullptr) == hipSuccess);
            // the fold: at the begin() that finds EV_RING pairs held, and it waits for those pairs only
            const int folds = (int)(i / (long long)EV_RING);
            CHECK(g_hip.event_syncs == folds * (int)EV_RING && g_hip.elapsed == folds * (int)EV_RING);
        }
        CHECK(g_hip.events == 2 * (int)EV_RING && g_hip.records == 2 * n);          // the list does not grow with the run
        CHECK(g_hip.event_syncs == 2 * (int)EV_RING);
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == n && ms == 0.25 * (double)n);
        CHECK(g_hip.event_syncs == 2 * (int)EV_RING + 3);          // (the three pairs held)
        CHECK(t.read(false, nullptr, nullptr) == hipSuccess);          // either output may be left out
        CHECK(t.read(true, &ms, &cnt) == hipSuccess && cnt == n && ms == 0.25 * (double)n);
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == 0 && ms == 0);

        // a begin() without end() -- the launch between them failed -- adds nothing
        CHECK(t.begin(nullptr) == hipSuccess);
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == 0 && ms == 0);
        CHECK(t.begin(nullptr) == hipSuccess && t.end(nullptr) == hipSuccess);
        CHECK(t.end(nullptr) == hipSuccess);          // (an end() with nothing open records nothing)
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == 1 && ms == 0.25);

        // a failed elapsed-time read is read()'s error and changes nothing
        g_hip.fail_elapsed = 1;
        ms = -1; cnt = -1;
        CHECK(t.read(true, &ms, &cnt) == hipErrorInvalidValue && ms == -1 && cnt == -1);
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == 1 && ms == 0.25);
        EventTimer u(std::move(t));          // a moved-from timer destroys nothing and reads empty
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == 0 && g_hip.event_destroys == 0);
        CHECK(u.read(false, &ms, &cnt) == hipSuccess && cnt == 1);
    }
    CHECK(g_hip.events == g_hip.event_destroys);

    // a failed event creation, of the pair's first and of its second event: begin()'s error, the timer stays usable and loses no event
    for (int nth = 1; nth <= 2; nth++) {
        g_hip = FakeHip{};
        {
            EventTimer t;
            double ms = -1;
            long long cnt = -1;
            g_hip.fail_event = nth;
            CHECK(t.begin(nullptr) == hipErrorOutOfMemory);
            CHECK(t.end(nullptr) == hipSuccess && g_hip.records == 0);
            CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == 0 && ms == 0);
            CHECK(t.begin(nullptr) == hipSuccess && t.end(nullptr) == hipSuccess);
            CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == 1 && ms == 0.25);
            CHECK(g_hip.events == 2 + 1);          // (the failed call is counted)
        }
        CHECK(g_hip.event_destroys == 2);
    }
    // a failed elapsed-time read inside the fold: begin()'s error; the pairs are still held and are folded by the next begin()
    {
        g_hip = FakeHip{};
        EventTimer t;
        for (size_t i = 0; i < EV_RING; i++) CHECK(t.begin(nullptr) == hipSuccess && t.end(nullptr) == hipSuccess);
        g_hip.fail_elapsed = 5;
        CHECK(t.begin(nullptr) == hipErrorInvalidValue);
        double ms = -1;
        long long cnt = -1;
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == (long long)EV_RING && ms == 0.25 * (double)EV_RING);
        CHECK(t.begin(nullptr) == hipSuccess && t.end(nullptr) == hipSuccess);
        CHECK(t.read(false, &ms, &cnt) == hipSuccess && cnt == (long long)EV_RING + 1 && ms == 0.25 * (double)(EV_RING + 1));
        CHECK(g_hip.events == 2 * (int)EV_RING);
    }
}

// StageRing::acquire: four slots in turn, each grown for a larger call only (to a multiple of 4096, pinned and device alike), a failure of
// either allocation named and leaking nothing, and the slot usable by the call after
static void stagering() {
    g_hip = FakeHip{};
    {
        StageRing ring;
        std::string err;
        StageRing::Slot* first[StageRing::NSLOT];
        for (int k = 0; k < StageRing::NSLOT; k++) {
            StageRing::Slot* s = first[k] = ring.acquire(100, err);
            CHECK(s && s == &ring.slot[k] && s->cap == 4096 && s->dev.cap() == 4096 && s->pin && s->dev && s->done && !s->busy);
            std::memset(s->pin, 1, s->cap);
            CHECK(ring.upload(*s, 100, nullptr, err) == 0 && ((uint8_t*)s->dev.ptr())[99] == 1);
            CHECK(ring.release(*s, nullptr, err) == 0 && s->busy);
        }
        CHECK(g_hip.mallocs == 4 && g_hip.host_mallocs == 4 && g_hip.events == 4 && g_hip.frees == 0 && g_hip.event_syncs == 0);
        // round two, smaller and equal: the slots come back in turn, waited for, nothing allocated
        for (int k = 0; k < StageRing::NSLOT; k++) {
            StageRing::Slot* s = ring.acquire(k ? 4096 : 8, err);
            CHECK(s == first[k] && !s->busy && s->cap == 4096);
        }
        CHECK(g_hip.mallocs == 4 && g_hip.host_mallocs == 4 && g_hip.events == 4 && g_hip.event_syncs == 4);
        // larger: that slot alone is reallocated
        StageRing::Slot* s = ring.acquire(4097, err);
        CHECK(s == first[0] && s->cap == 8192 && s->dev.cap() == 8192);
        CHECK(g_hip.mallocs == 5 && g_hip.frees == 1 && g_hip.host_mallocs == 5 && g_hip.host_frees == 1 && g_hip.events == 4);
        std::memset(s->pin, 2, s->cap);
        CHECK(ring.upload(*s, 8192, nullptr, err) == 0 && ((uint8_t*)s->dev.ptr())[8191] == 2);
        CHECK(err.empty());
        // the pinned, then the device allocation of slot 1's regrow fails: nullptr and a message, and the slot serves the next call that reaches it
        for (int what = 0; what < 2; what++) {
            (what ? g_hip.fail_malloc : g_hip.fail_host_malloc) = 1;
            err.clear();
            StageRing::Slot* bad = ring.acquire(20000, err);
            CHECK(bad == nullptr && err.find("image staging ring: ") == 0 && err.find(hipGetErrorString(hipErrorOutOfMemory)) != std::string::npos);
            CHECK(ring.slot[1 + what].cap == 0);
            ring.next = 1 + what;          // (the same slot again)
            StageRing::Slot* again = ring.acquire(20000, err);
            CHECK(again == &ring.slot[1 + what] && again->cap == 20480 && again->dev.cap() == 20480);
            std::memset(again->pin, 3, again->cap);
            CHECK(ring.upload(*again, 20000, nullptr, err) == 0 && ((uint8_t*)again->dev.ptr())[19999] == 3);
            CHECK(ring.release(*again, nullptr, err) == 0);
        }
        ring.destroy();
        CHECK(g_hip.mallocs == g_hip.frees + 1 && g_hip.host_mallocs == g_hip.host_frees + 1);          // (one failed call of each is counted)
        CHECK(g_hip.events == g_hip.event_destroys);
        for (auto& sl : ring.slot) CHECK(!sl.pin && !sl.dev && !sl.cap && !sl.done && !sl.busy);
    }
}

int main() {
    devbuf();
    devarena();
    eventtimer();
    stagering();
    std::puts("dev ok");
    return 0;
}

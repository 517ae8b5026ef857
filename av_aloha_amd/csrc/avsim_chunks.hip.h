// avsim_chunks.hip.h -- per-env execution of action chunks on the device (avsim_chunk_*): what avsim_api.hip needs of the
// unit csrc/avsim_chunks.hip -- the arguments of the kernels, the checks of the set-up, the state a handle owns and the launchers.
//
// av_aloha_amd/chunks.py is the specification, and the device equals it bit for bit: every float32 *, + and / rounded on its own and
// correctly, denormals kept.  avsim_api.hip's flags do not give that (build.py, F32_FLAGS), so the kernels live in a unit built as
// avsim_imgaug.hip is and are reached through chunk_launch_* (the build is -fno-gpu-rdc).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "avsim_dev.h"

namespace avs {

constexpr int CHK_MAX_C = 1024, CHK_MAX_A = 64;
constexpr int CHK_ENSEMBLE = 0, CHK_QUEUE = 1;
constexpr int CHK_BOOK_THREADS = 1024;      // k_chunk_book is one workgroup: its envs' flags meet in LDS
constexpr int CHK_THREADS = 256;
// what k_chunk_book tells k_chunk_queue about an env in cur_b
constexpr int CHK_POP = 0, CHK_TAKE = 1, CHK_REPEAT = 2, CHK_ZERO = 3;

// The kernels' view of a handle's chunk state.  sa / sb: ensemble -- the ring's head u mod C and the count min(u, C-1); queue -- the next row
// of the queue and the rows left.  cur_a / cur_b: what k_chunk_book found for THIS call (ensemble: head and count before the update; queue:
// the row to pop and CHK_*), the only per-env state the pass over the floats reads -- k_chunk_book advances sa / sb in front of it, after every
// reader of the previous call and before every reader of the next (calls on one stream are ordered).
struct ChunkArgs {
    int N, C, A, CA, mode, k, first, has_ms;
    unsigned magic;              // floor(2^32 / A) + 1 for A >= 2: (i * magic) >> 32 == i / A for i < 2^16
    int64_t* last_id;
    int *stepped, *sa, *sb, *cur_a, *cur_b;
    float* buf;                  // ensemble: the rings [N][C][A]; queue: the queues [N][k][A]
    float* prev;                 // [N][A], the last action (queue mode's starved envs repeat it)
    unsigned long long* starved;
    const float* tab;            // w[C], cum[C]
    const float* ms;             // mean[A], std[A]
};

// the refusals of avsim_chunk_setup; -1 and err says which
inline int chunk_validate(int C, int A, int mode, int k, int first, const float* tables, const float* mean_std, std::string& err) {
    char buf[200];
    if (C < 1 || C > CHK_MAX_C) { snprintf(buf, sizeof buf, "avsim_chunk_setup: chunk_size %d outside 1..%d", C, CHK_MAX_C); err = buf; return -1; }
    if (A < 1 || A > CHK_MAX_A) { snprintf(buf, sizeof buf, "avsim_chunk_setup: action_dim %d outside 1..%d", A, CHK_MAX_A); err = buf; return -1; }
    if (mode != CHK_ENSEMBLE && mode != CHK_QUEUE) { snprintf(buf, sizeof buf, "avsim_chunk_setup: mode %d is 0 (ensemble) or 1 (queue)", mode); err = buf; return -1; }
    if (mode == CHK_QUEUE && (k < 1 || first < 0 || (long long)first + k > C)) {
        snprintf(buf, sizeof buf, "avsim_chunk_setup: a queue of %d rows from row %d of a chunk of %d (n_action_steps >= 1, first >= 0, first + n_action_steps <= chunk_size)", k, first, C);
        err = buf;
        return -1;
    }
    if (mode == CHK_ENSEMBLE) {
        if (!tables) { err = "avsim_chunk_setup: ensemble mode needs the tables w[C], cum[C]"; return -1; }
        for (int i = 0; i < 2 * C; i++)
            if (!std::isfinite(tables[i])) { snprintf(buf, sizeof buf, "avsim_chunk_setup: table entry %d is not finite", i); err = buf; return -1; }
        for (int i = 0; i < C; i++)
            if (!(tables[C + i] > 0.0f)) { snprintf(buf, sizeof buf, "avsim_chunk_setup: cum[%d] = %g is not positive", i, (double)tables[C + i]); err = buf; return -1; }
    }
    if (mean_std)
        for (int i = 0; i < 2 * A; i++)
            if (!std::isfinite(mean_std[i])) { err = "avsim_chunk_setup: a mean or std that is not finite"; return -1; }
    return 0;
}

// csrc/avsim_chunks.hip.  All pointers are device pointers.
// k_chunk_book alone: need u8 [N] and any int32 [1] (either may be NULL) of the envs' flags; commit = 0 changes nothing
void chunk_launch_book(hipStream_t stream, const ChunkArgs& P, int commit, int have_chunks, const int64_t* episode_id, const int* elapsed, uint8_t* need, int* any);
// k_chunk_book (commit) and the pass over the floats: chunks float [N][C][A] or NULL (queue mode), action float [N][A]
void chunk_launch_step(hipStream_t stream, const ChunkArgs& P, const float* chunks, const int64_t* episode_id, const int* elapsed, float* action);

// The state a handle owns (avsim_chunk_setup), sized to its num_envs
struct ChunkHost {
    bool ready = false;
    ChunkArgs P{};
    DevArena arena;
    std::vector<float> host_tab;      // what the set-up uploads: w, cum, mean, std (kept until the next set-up)

    void destroy() {
        arena.clear();
        ready = false;
        P = ChunkArgs{};
    }

    // validated arguments; the stream is idle (the caller synchronised it).  -3: HIP
    int setup(hipStream_t stream, int N, int C, int A, int mode, int k, int first, const float* tables, const float* mean_std, std::string& err) {
        destroy();
        ChunkArgs a{};
        a.N = N; a.C = C; a.A = A; a.CA = C * A; a.mode = mode; a.k = mode == CHK_QUEUE ? k : 0; a.first = mode == CHK_QUEUE ? first : 0;
        a.has_ms = mean_std != nullptr;
        a.magic = A >= 2 ? (unsigned)(0x100000000ull / (unsigned)A) + 1u : 0u;
        const size_t n = (size_t)N, rows = mode == CHK_QUEUE ? (size_t)k : (size_t)C;
        auto get = [&](size_t bytes) { return arena.zeroed(bytes, stream); };
        a.last_id = (int64_t*)get(sizeof(int64_t) * n);
        a.stepped = (int*)get(sizeof(int) * n); a.sa = (int*)get(sizeof(int) * n); a.sb = (int*)get(sizeof(int) * n);
        a.cur_a = (int*)get(sizeof(int) * n); a.cur_b = (int*)get(sizeof(int) * n);
        a.buf = (float*)get(sizeof(float) * n * rows * A);
        a.prev = (float*)get(sizeof(float) * n * A);
        a.starved = (unsigned long long*)get(sizeof(unsigned long long));
        float* tab = (float*)get(sizeof(float) * (2 * (size_t)C + 2 * (size_t)A));
        hipError_t e = arena.error();
        if (e == hipSuccess) {
            host_tab.assign(2 * (size_t)C + 2 * (size_t)A, 0.0f);
            if (tables) std::copy(tables, tables + 2 * C, host_tab.begin());
            if (mean_std) std::copy(mean_std, mean_std + 2 * A, host_tab.begin() + 2 * C);
            e = hipMemcpyAsync(tab, host_tab.data(), sizeof(float) * host_tab.size(), hipMemcpyHostToDevice, stream);
        }
        if (e != hipSuccess) {
            err = std::string("avsim_chunk_setup: ") + hipGetErrorString(e);
            destroy();
            return -3;
        }
        a.tab = tab;
        a.ms = tab + 2 * (size_t)C;
        P = a;
        ready = true;
        return 0;
    }
};

}  // namespace avs

// avsim_chunks.hip -- the kernels of avsim_chunk_need / avsim_chunk_step: per-env execution of a policy's action chunks, with
// LeRobot's temporal ensembling or an n-step queue.  av_aloha_amd/chunks.py is the specification; every float32 operation here is the one it
// names, rounded on its own.  The unit is built like avsim_imgaug.hip (av_aloha_amd/build.py): -ffp-contract=off, so that
// ens * cum[c-1] + y * w[c] is two v_mul and a v_add, IEEE division, denormals kept.  Kernels:
//   k_chunk_book      ONE workgroup, a lane per env (strided).  Reads the env's id and elapsed steps and the state of the previous call, decides
//                     fresh / need, and -- when it commits -- writes what THIS call's pass needs into cur_a / cur_b and advances the state.
//                     It is the only writer and the only reader of the state proper, and it runs in front of the pass on the same stream: no
//                     workgroup of the pass can see a head that another has already advanced.  need[N] and the any flag come out of the
//                     same launch (the flags meet through __syncthreads_or, the starved count through one LDS counter); commit = 0 is
//                     avsim_chunk_need and stores nothing else.
//   k_chunk_ensemble  grid = (envs, slabs).  Per env the chunk and the ring are the same flat array of C A floats, rotated against each other
//                     by head A elements.  Lanes run over the RING's flat index, V = 4 floats each when C A is a multiple of four (the rings
//                     are the library's own allocation: every env's ring then starts on a 16-byte boundary, a group never straddles the
//                     wrap, and the ring -- two thirds of the traffic -- goes through 16-byte loads and stores); the chunk, whose rotation
//                     falls off that alignment on most calls, is read one float at a time.  k = i / A once per lane through a multiply-high
//                     (exact for i < 2^16), then carried along.  V = 1 otherwise.  The lanes that hold row k = 0 also store the action.
//   k_chunk_queue     grid = envs.  By cur_b: take rows [first, first + k) of the chunk into the queue (un-normalised) and return the first,
//                     pop row cur_a, repeat the previous action, or zeros.
#include "avsim_chunks.hip.h"

namespace avs {

__global__ void __launch_bounds__(CHK_BOOK_THREADS) k_chunk_book(ChunkArgs P, int commit, int have_chunks, const int64_t* __restrict__ episode_id,
                                                                 const int* __restrict__ elapsed, uint8_t* __restrict__ need, int* __restrict__ any) {
    __shared__ int s_starved;
    if (threadIdx.x == 0) s_starved = 0;
    __syncthreads();
    int any_l = 0, starved_l = 0;
    for (int e = threadIdx.x; e < P.N; e += CHK_BOOK_THREADS) {
        const int64_t id = episode_id[e];
        const bool fresh = !P.stepped[e] || elapsed[e] == 0 || id != P.last_id[e];
        int nd = 1;
        if (P.mode == CHK_ENSEMBLE) {
            if (commit) {
                const int head = fresh ? 0 : P.sa[e], cnt = fresh ? 0 : P.sb[e];
                P.cur_a[e] = head;
                P.cur_b[e] = cnt;
                P.sa[e] = head + 1 == P.C ? 0 : head + 1;
                P.sb[e] = cnt + 1 < P.C - 1 ? cnt + 1 : P.C - 1;
            }
        } else {
            const int left = fresh ? 0 : P.sb[e];
            nd = left == 0;
            if (commit) {
                if (!nd) {
                    const int row = P.sa[e];
                    P.cur_a[e] = row;
                    P.cur_b[e] = CHK_POP;
                    P.sa[e] = row + 1;
                    P.sb[e] = left - 1;
                } else if (have_chunks) {
                    P.cur_a[e] = 0;
                    P.cur_b[e] = CHK_TAKE;
                    P.sa[e] = 1;
                    P.sb[e] = P.k - 1;
                } else {
                    P.cur_a[e] = 0;
                    P.cur_b[e] = fresh ? CHK_ZERO : CHK_REPEAT;
                    P.sa[e] = 0;
                    P.sb[e] = 0;
                    starved_l++;
                }
            }
        }
        if (commit) {
            P.stepped[e] = 1;
            P.last_id[e] = id;
        }
        if (need) need[e] = (uint8_t)nd;
        any_l |= nd;
    }
    if (starved_l) atomicAdd(&s_starved, starved_l);
    const int any_b = __syncthreads_or(any_l);
    if (threadIdx.x == 0) {
        if (any) *any = any_b ? 1 : 0;
        if (commit && s_starved) *P.starved = *P.starved + (unsigned long long)s_starved;
    }
}

template <int V>
__global__ void __launch_bounds__(CHK_THREADS) k_chunk_ensemble(ChunkArgs P, int groups, const float* __restrict__ chunks, float* __restrict__ action) {
    const int e = blockIdx.x;
    const int g = blockIdx.y * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    const int C = P.C, A = P.A, CA = P.CA;
    const int head = P.cur_a[e], cnt = P.cur_b[e];
    const int r0 = g * V;                                  // the ring's flat index of this lane's first float
    int i = r0 - head * A;                                 // ... and the chunk's
    if (i < 0) i += CA;
    int k = A == 1 ? i : (int)__umulhi((unsigned)i, P.magic);
    int a = i - k * A;
    const float* __restrict__ x = chunks + (size_t)e * CA;
    float* ring = P.buf + (size_t)e * CA + r0;
    const float* __restrict__ w = P.tab;
    const float* __restrict__ cum = P.tab + C;
    float o[V], v[V];
#pragma unroll
    for (int t = 0; t < V; t++) o[t] = 0.0f;
    if (cnt > 0) {                                         // (a fresh env's ring is never read)
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(ring);
            o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
        } else {
            o[0] = ring[0];
        }
    }
#pragma unroll
    for (int t = 0; t < V; t++) {
        float y = x[k * A + a];
        if (P.has_ms) {
            y = y * P.ms[A + a];
            y = y + P.ms[a];
        }
        const int c = min(cnt, C - 1 - k);                 // the predictions this time step already holds
        float r = y;
        if (c > 0) {
            const float p = o[t] * cum[c - 1];
            const float q = y * w[c];
            r = (p + q) / cum[c];
        }
        v[t] = r;
        if (k == 0) action[(size_t)e * A + a] = r;
        if (++a == A) {
            a = 0;
            if (++k == C) k = 0;
        }
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(ring) = make_float4(v[0], v[1], v[2], v[3]);
    else ring[0] = v[0];
}

__global__ void __launch_bounds__(CHK_THREADS) k_chunk_queue(ChunkArgs P, const float* __restrict__ chunks, float* __restrict__ action) {
    const int e = blockIdx.x;
    const int A = P.A, kA = P.k * A;
    const int row = P.cur_a[e], what = P.cur_b[e];
    float* q = P.buf + (size_t)e * kA;
    float* prev = P.prev + (size_t)e * A;
    float* act = action + (size_t)e * A;
    if (what == CHK_TAKE) {
        const float* __restrict__ x = chunks + (size_t)e * P.CA + (size_t)P.first * A;
        for (int i = threadIdx.x; i < kA; i += CHK_THREADS) {
            float y = x[i];
            if (P.has_ms) {
                const int kk = A == 1 ? i : (int)__umulhi((unsigned)i, P.magic);
                const int a = i - kk * A;
                y = y * P.ms[A + a];
                y = y + P.ms[a];
            }
            q[i] = y;
            if (i < A) {
                act[i] = y;
                prev[i] = y;
            }
        }
    } else {
        for (int a = threadIdx.x; a < A; a += CHK_THREADS) {
            const float y = what == CHK_POP ? q[row * A + a] : (what == CHK_REPEAT ? prev[a] : 0.0f);
            act[a] = y;
            prev[a] = y;
        }
    }
}

void chunk_launch_book(hipStream_t stream, const ChunkArgs& P, int commit, int have_chunks, const int64_t* episode_id, const int* elapsed, uint8_t* need, int* any) {
    hipLaunchKernelGGL(k_chunk_book, dim3(1), dim3(CHK_BOOK_THREADS), 0, stream, P, commit, have_chunks, episode_id, elapsed, need, any);
}

void chunk_launch_step(hipStream_t stream, const ChunkArgs& P, const float* chunks, const int64_t* episode_id, const int* elapsed, float* action) {
    chunk_launch_book(stream, P, 1, chunks != nullptr, episode_id, elapsed, nullptr, nullptr);
    if (P.mode == CHK_QUEUE) {
        hipLaunchKernelGGL(k_chunk_queue, dim3(P.N), dim3(CHK_THREADS), 0, stream, P, chunks, action);
        return;
    }
    // the slabs of an env: as few as hold its groups, each as many whole waves as its share needs (C A = 2100: 525 groups, 3 slabs of 192 lanes)
    const int V = P.CA % 4 == 0 ? 4 : 1;
    const int groups = P.CA / V;
    const int slabs = (groups + CHK_THREADS - 1) / CHK_THREADS;
    const int threads = (((groups + slabs - 1) / slabs) + 63) / 64 * 64;
    if (V == 4) hipLaunchKernelGGL(k_chunk_ensemble<4>, dim3(P.N, slabs), dim3(threads), 0, stream, P, groups, chunks, action);
    else hipLaunchKernelGGL(k_chunk_ensemble<1>, dim3(P.N, slabs), dim3(threads), 0, stream, P, groups, chunks, action);
}

}  // namespace avs

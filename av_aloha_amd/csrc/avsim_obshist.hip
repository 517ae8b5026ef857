// avsim_obshist.hip -- the kernels of avsim_obs_history_push: per-env histories [N][K][...] of a policy's observations, slot K-1 the
// newest, restarted per env when its episode is.  av_aloha_amd/obshist.py is the specification.  The unit is built like avsim_imgaug.hip
// (av_aloha_amd/build.py): -ffp-contract=off, IEEE division, denormals kept, so that (x - mean) / std rounds as numpy's does.  Kernels:
//   k_obs_book    ONE workgroup, envs strided over its lanes.  The only reader and writer of pushed / last_id: decides fresh per env (not pushed
//                 since the set-up or reset, elapsed 0, or another episode id than the previous call's), writes cur_fresh and advances the state.
//                 It runs in front of the passes on the same stream; they read cur_fresh only.  No atomics on global memory anywhere.
//   k_obs_image   grid = (envs, slabs, cameras): one launch for all cameras, their pointers a kernel argument, their boxes and tables a device
//                 table of the set-up; the camera's [3][256] table is staged in LDS as k_image_prep does.  A lane owns V consecutive pixels of the
//                 flat plane index (V = 4: a group may straddle an image row) in the three planes of an env's slot, and carries each through all K
//                 slots: it reads slot[k+1] and writes slot[k] at the SAME position, up to four slots in flight, so the in-place shift has no reader
//                 other than its writer; the newest slot comes from the source through the table.  A fresh env's lanes read no history and write
//                 the new value K times.  V = 4 (16-byte history loads and stores) when oh ow is a multiple of four -- 3 oh ow is then one too --
//                 and every history pointer is 16-byte aligned; V = 1 otherwise.
//   k_obs_state   [N][K][D], a lane per (env, dimension), the same rule; new = (x - mean[d]) / std[d], two operations.
#include "avsim_obshist.hip.h"

namespace avs {

__global__ void __launch_bounds__(OBH_BOOK_THREADS) k_obs_book(ObsArgs P, const int64_t* __restrict__ episode_id, const int* __restrict__ elapsed) {
    for (int e = threadIdx.x; e < P.N; e += OBH_BOOK_THREADS) {
        const int64_t id = episode_id[e];
        P.cur_fresh[e] = (!P.pushed[e] || elapsed[e] == 0 || id != P.last_id[e]) ? 1 : 0;
        P.pushed[e] = 1;
        P.last_id[e] = id;
    }
}

__device__ __forceinline__ int obh_u8(float v) {      // (int)(v * 255 + 0.5f), each operation rounded on its own, clamped to a byte (imgprep.to_u8)
    const float x = v * 255.0f;
    const float y = x + 0.5f;
    return (int)fminf(fmaxf(y, 0.0f), 255.0f);
}

template <int V> struct ObhVec;
template <> struct ObhVec<1> { typedef float type; };
template <> struct ObhVec<4> { typedef float4 type; };

// One position (V floats at h) through the K slots, `stride` floats apart: the loads of up to four slots, then their stores one slot down
template <int V>
__device__ __forceinline__ void obh_shift(float* h, size_t stride, int K, bool fresh, typename ObhVec<V>::type nv) {
    typedef typename ObhVec<V>::type T;
    if (fresh) {                                           // (the old contents are not read: they may be anything)
        for (int k = 0; k < K; k++) *reinterpret_cast<T*>(h + (size_t)k * stride) = nv;
        return;
    }
    for (int k = 0; k < K - 1; k += 4) {
        const int n = K - 1 - k;
        T* p = reinterpret_cast<T*>(h + (size_t)k * stride);      // (named values, not an array: an array here is promoted to LDS)
        T t0 = nv, t1 = nv, t2 = nv, t3 = nv;
        t0 = *reinterpret_cast<const T*>(h + (size_t)(k + 1) * stride);
        if (n > 1) t1 = *reinterpret_cast<const T*>(h + (size_t)(k + 2) * stride);
        if (n > 2) t2 = *reinterpret_cast<const T*>(h + (size_t)(k + 3) * stride);
        if (n > 3) t3 = *reinterpret_cast<const T*>(h + (size_t)(k + 4) * stride);
        *p = t0;
        if (n > 1) *reinterpret_cast<T*>(h + (size_t)(k + 1) * stride) = t1;
        if (n > 2) *reinterpret_cast<T*>(h + (size_t)(k + 2) * stride) = t2;
        if (n > 3) *reinterpret_cast<T*>(h + (size_t)(k + 3) * stride) = t3;
    }
    *reinterpret_cast<T*>(h + (size_t)(K - 1) * stride) = nv;
}

// SF: the source's format (0: u8 [N][SH][SW][3], 1: float32 [N][3][SH][SW]); V: pixels per lane
template <int SF, int V>
__global__ void __launch_bounds__(OBH_THREADS) k_obs_image(ObsArgs P, ObsPtrs Q) {
    __shared__ float s_lut[3 * 256];
    const int e = blockIdx.x, cam = blockIdx.z, tid = threadIdx.x;
    const float* __restrict__ tab = P.lut + (size_t)cam * 768;
    for (int t = tid; t < 768; t += OBH_THREADS) s_lut[t] = tab[t];
    __syncthreads();
    const int x0 = P.box[3 * cam], y0 = P.box[3 * cam + 1], flip = P.box[3 * cam + 2];
    const unsigned ow = (unsigned)P.ow;
    const size_t plane = (size_t)P.oh * P.ow, S = 3 * plane;      // (plane <= 65535^2 < 2^32)
    const size_t groups = plane / V;
    const bool fresh = P.cur_fresh[e] != 0;
    float* hist = Q.hist[cam] + (size_t)e * P.K * S;
    const void* __restrict__ src = Q.img[cam];
    const size_t SH = (size_t)P.SH, SW = (size_t)P.SW;
    for (size_t g = (size_t)blockIdx.y * OBH_THREADS + tid; g < groups; g += (size_t)gridDim.y * OBH_THREADS) {
        const unsigned q0 = (unsigned)(g * V);
        unsigned y = q0 / ow, x = q0 - y * ow;
        float nv[3][V];
#pragma unroll
        for (int j = 0; j < V; j++) {
            const size_t sy = (size_t)y0 + y, sx = (size_t)x0 + (flip ? ow - 1 - x : x);
            if (SF == 0) {
                const uint8_t* s = (const uint8_t*)src + (((size_t)e * SH + sy) * SW + sx) * 3;
#pragma unroll
                for (int c = 0; c < 3; c++) nv[c][j] = s_lut[c * 256 + s[c]];
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) nv[c][j] = s_lut[c * 256 + obh_u8(((const float*)src)[(((size_t)e * 3 + c) * SH + sy) * SW + sx])];
            }
            if (++x == ow) { x = 0; ++y; }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float* h = hist + c * plane + q0;
            if constexpr (V == 4) obh_shift<4>(h, S, P.K, fresh, make_float4(nv[c][0], nv[c][1], nv[c][2], nv[c][3]));
            else obh_shift<1>(h, S, P.K, fresh, nv[c][0]);
        }
    }
}

__global__ void __launch_bounds__(OBH_THREADS) k_obs_state(ObsArgs P, const float* __restrict__ state, float* hist) {
    const size_t i = (size_t)blockIdx.x * OBH_THREADS + threadIdx.x;
    if (i >= (size_t)P.N * P.D) return;
    const size_t e = i / (unsigned)P.D;
    const int d = (int)(i - e * P.D);
    float v = state[i];
    if (P.has_ms) {
        v = v - P.ms[d];
        v = v / P.ms[P.D + d];
    }
    obh_shift<1>(hist + e * P.K * P.D + d, (size_t)P.D, P.K, P.cur_fresh[e] != 0, v);
}

void obs_launch_push(hipStream_t stream, const ObsArgs& P, const ObsPtrs& Q, const int64_t* episode_id, const int* elapsed, const float* state, float* state_hist) {
    hipLaunchKernelGGL(k_obs_book, dim3(1), dim3(OBH_BOOK_THREADS), 0, stream, P, episode_id, elapsed);
    if (P.D > 0) {
        const size_t n = (size_t)P.N * P.D;
        hipLaunchKernelGGL(k_obs_state, dim3((unsigned)((n + OBH_THREADS - 1) / OBH_THREADS)), dim3(OBH_THREADS), 0, stream, P, state, state_hist);
    }
    if (P.ncam > 0) {
        const size_t plane = (size_t)P.oh * P.ow;
        bool wide = plane % 4 == 0;
        for (int c = 0; c < P.ncam; c++) wide = wide && ((uintptr_t)Q.hist[c] & 15) == 0;
        const size_t groups = plane / (wide ? 4 : 1);
        const unsigned slabs = (unsigned)std::min<size_t>(OBH_MAX_SLABS, (groups + OBH_THREADS - 1) / OBH_THREADS);
        const dim3 grid(P.N, slabs, P.ncam), block(OBH_THREADS);
        if (P.fmt == 0) {
            if (wide) hipLaunchKernelGGL((k_obs_image<0, 4>), grid, block, 0, stream, P, Q);
            else hipLaunchKernelGGL((k_obs_image<0, 1>), grid, block, 0, stream, P, Q);
        } else {
            if (wide) hipLaunchKernelGGL((k_obs_image<1, 4>), grid, block, 0, stream, P, Q);
            else hipLaunchKernelGGL((k_obs_image<1, 1>), grid, block, 0, stream, P, Q);
        }
    }
}

}  // namespace avs

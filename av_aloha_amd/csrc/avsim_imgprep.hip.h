// avsim_imgprep.hip.h -- training batches on the device (avsim_image_stats, avsim_image_prep): the per-image sums a data set's
// statistics are made of, and the crop + flip + table look-up that turns a decoded frame into a policy's input.
//
// av_aloha_amd/imgprep.py is the specification (stats_reference, prep_reference).  The statistics are integers and the prepared images are
// table entries copied, so both are equal to it bit for bit and the same on every run.  Kernels:
//   k_image_stats_init  out[i][c] = (0, 0, 255, 0): the neutral element of (sum, sum of squares, min, max)
//   k_image_stats<0>    u8 HWC: an image is a byte stream whose byte o holds channel o % 3.  From the first 16-byte boundary on it is read in
//                       units of 48 bytes per lane (three 16-byte loads), in which a byte's position fixes its channel: sums and sums of
//                       squares by v_dot4_u32_u8 against masks, min / max on 16-bit pairs.  A lane sums in 32 bits for at most 2048 units
//                       (2048 x 16 x 255^2 < 2^32) and widens to 64.  The bytes in front of the boundary and behind the last unit go one
//                       per lane.  Wave shuffle, LDS across the waves, then twelve 64-bit integer atomics per workgroup.
//   k_image_stats<1>    float32 CHW: the three planes, each value through (int)(v * 255 + 0.5f).
//   k_image_prep        a workgroup per output image and band of rows, the image's [3][256] table in LDS; a lane makes four consecutive
//                       pixels of a row: 12 source bytes (the dwords that hold them, shifted into place) or 3 x 4 floats in, one 16-byte
//                       store per plane out where the address allows, single floats where it does not.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>

#include "avsim_jpeg.hip.h"
#include "avsim_stage.h"

namespace avs {

constexpr int IST_THREADS = 256;
constexpr int IST_UNIT = 48;          // bytes a lane reads per step: the smallest multiple of 16 (a load) and of 3 (a pixel)
constexpr int IST_FLUSH = 2048;       // units a lane sums in 32 bits
constexpr int IST_MAX_SLABS = 1024;   // workgroups per image
constexpr int IPR_THREADS = 256;

typedef unsigned short ist_us2 __attribute__((ext_vector_type(2)));

// the 0x01 bytes of dword type t (= its index in the unit mod 3) that hold class r: byte b of such a dword has class (t + b) % 3
__host__ __device__ constexpr uint32_t ist_mask(int t, int r) {
    uint32_t m = 0;
    for (int b = 0; b < 4; b++)
        if ((t + b) % 3 == r) m |= 1u << (8 * b);
    return m;
}

__device__ __forceinline__ uint32_t ist_sel3(int k, uint32_t a, uint32_t b, uint32_t c) { return k == 0 ? a : k == 1 ? b : c; }
__device__ __forceinline__ unsigned long long ist_sel3(int k, unsigned long long a, unsigned long long b, unsigned long long c) { return k == 0 ? a : k == 1 ? b : c; }

__global__ void __launch_bounds__(256) k_image_stats_init(unsigned long long* __restrict__ out, int n3) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    unsigned long long* o = out + 4 * (size_t)i;
    o[0] = 0; o[1] = 0; o[2] = 255; o[3] = 0;
}

// FMT 0: u8 [n][H][W][3], FMT 1: float32 [n][3][H][W].  grid = (slabs, images of this launch); out: [nimg][3][4], initialised
template <int FMT>
__global__ void __launch_bounds__(IST_THREADS) k_image_stats(const void* __restrict__ img, const int* __restrict__ index, int img0, size_t HW,
                                                             unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_red[IST_THREADS / 64][12];
    const int i = img0 + blockIdx.y, tid = threadIdx.x;
    const size_t src = index ? (size_t)index[i] : (size_t)i;
    unsigned long long S[3] = {0, 0, 0}, Q[3] = {0, 0, 0};      // per channel
    uint32_t MN[3] = {255, 255, 255}, MX[3] = {0, 0, 0};
    if (FMT == 0) {
        const size_t L = 3 * HW;
        const uint8_t* p = (const uint8_t*)img + src * L;
        const size_t to16 = (size_t)((0 - (uintptr_t)p) & 15);
        const size_t head = to16 < L ? to16 : L;
        const size_t nu = (L - head) / IST_UNIT;
        const size_t tail0 = head + nu * IST_UNIT;                // the bytes [tail0, L) follow the last unit
        unsigned long long s64[3] = {0, 0, 0}, q64[3] = {0, 0, 0};      // per class: (byte offset in the unit) % 3
        uint32_t lo_mn[3], hi_mn[3], lo_mx[3], hi_mx[3];                // per dword type: bytes 0 | 2 and 1 | 3 as 16-bit pairs
#pragma unroll
        for (int t = 0; t < 3; t++) { lo_mn[t] = hi_mn[t] = 0x00FF00FFu; lo_mx[t] = hi_mx[t] = 0; }
        const uint4* base = (const uint4*)(p + head);
        const size_t stride = (size_t)gridDim.x * IST_THREADS;
        size_t u = (size_t)blockIdx.x * IST_THREADS + tid;
        while (u < nu) {
            uint32_t s32[3] = {0, 0, 0}, q32[3] = {0, 0, 0};
            for (int n = 0; n < IST_FLUSH && u < nu; n++, u += stride) {
                const uint4* q = base + 3 * u;
                const uint4 a = q[0], b = q[1], c = q[2];
                const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
                for (int d = 0; d < 12; d++) {
                    const int t = d % 3;
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const uint32_t m = ist_mask(t, r);
                        s32[r] = __builtin_amdgcn_udot4(w[d], m, s32[r], false);
                        q32[r] = __builtin_amdgcn_udot4(w[d] & (m * 255u), w[d], q32[r], false);
                    }
                    const uint32_t lo = w[d] & 0x00FF00FFu, hi = (w[d] >> 8) & 0x00FF00FFu;
                    lo_mn[t] = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(ist_us2, lo_mn[t]), __builtin_bit_cast(ist_us2, lo)));
                    hi_mn[t] = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(ist_us2, hi_mn[t]), __builtin_bit_cast(ist_us2, hi)));
                    lo_mx[t] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(ist_us2, lo_mx[t]), __builtin_bit_cast(ist_us2, lo)));
                    hi_mx[t] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(ist_us2, hi_mx[t]), __builtin_bit_cast(ist_us2, hi)));
                }
            }
#pragma unroll
            for (int r = 0; r < 3; r++) { s64[r] += s32[r]; q64[r] += q32[r]; }
        }
        // min / max per class out of the pairs: byte b of type t is lo's half b / 2 (b even) or hi's (b odd)
        uint32_t cmn[3] = {255, 255, 255}, cmx[3] = {0, 0, 0};
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int r = (t + b) % 3;
                const uint32_t vmn = ((b & 1 ? hi_mn[t] : lo_mn[t]) >> (8 * (b & 2))) & 0xFFFFu;
                const uint32_t vmx = ((b & 1 ? hi_mx[t] : lo_mx[t]) >> (8 * (b & 2))) & 0xFFFFu;
                cmn[r] = min(cmn[r], vmn);
                cmx[r] = max(cmx[r], vmx);
            }
        // class r of the units is channel (head + r) % 3
        const int hp = (int)(head % 3);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int r = (c + 3 - hp) % 3;
            S[c] = ist_sel3(r, s64[0], s64[1], s64[2]);
            Q[c] = ist_sel3(r, q64[0], q64[1], q64[2]);
            MN[c] = ist_sel3(r, cmn[0], cmn[1], cmn[2]);
            MX[c] = ist_sel3(r, cmx[0], cmx[1], cmx[2]);
        }
        // the bytes in front of the first unit and behind the last one: at most 15 + 47, a lane each, in the image's first workgroup
        if (blockIdx.x == 0) {
            const size_t ntail = L - tail0;
            if ((size_t)tid < head + ntail) {
                const size_t o = (size_t)tid < head ? (size_t)tid : tail0 + ((size_t)tid - head);
                const uint32_t v = p[o];
                const int c = (int)(o % 3);
#pragma unroll
                for (int k = 0; k < 3; k++)
                    if (c == k) { S[k] += v; Q[k] += v * v; MN[k] = min(MN[k], v); MX[k] = max(MX[k], v); }
            }
        }
    } else {
        const size_t stride = (size_t)gridDim.x * IST_THREADS;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float* p = (const float*)img + (src * 3 + c) * HW;
            for (size_t k = (size_t)blockIdx.x * IST_THREADS + tid; k < HW; k += stride) {
                const uint32_t v = (uint32_t)jpg_u8(p[k]);
                S[c] += v; Q[c] += v * v; MN[c] = min(MN[c], v); MX[c] = max(MX[c], v);
            }
        }
    }
    // across the wave, across the waves, then one atomic per value and workgroup
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            S[c] += __shfl_xor(S[c], off);
            Q[c] += __shfl_xor(Q[c], off);
            MN[c] = min(MN[c], (uint32_t)__shfl_xor((int)MN[c], off));
            MX[c] = max(MX[c], (uint32_t)__shfl_xor((int)MX[c], off));
        }
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s_red[wave][4 * c] = S[c]; s_red[wave][4 * c + 1] = Q[c]; s_red[wave][4 * c + 2] = MN[c]; s_red[wave][4 * c + 3] = MX[c];
        }
    }
    __syncthreads();
    if (tid < 12) {
        const int k = tid & 3;
        unsigned long long v = s_red[0][tid];
        for (int w = 1; w < IST_THREADS / 64; w++) {
            const unsigned long long x = s_red[w][tid];
            v = k < 2 ? v + x : k == 2 ? (x < v ? x : v) : (x > v ? x : v);
        }
        unsigned long long* o = out + 12 * (size_t)i + tid;
        if (k < 2) atomicAdd(o, v);
        else if (k == 2) atomicMin(o, v);
        else atomicMax(o, v);
    }
}

// One output image as k_image_prep reads it: the source image, the box's corner, flip | table << 1 (validated by the host)
struct PrepItem { int src, x0, y0, fl; };

__device__ __forceinline__ float ipr_pick(int k, float a, float b, float c, float d) { return k == 0 ? a : k == 1 ? b : k == 2 ? c : d; }

// SF: the source's format.  grid = (bands of `rb` output rows, images of this launch); out: float32 [nout][3][oh][ow]
template <int SF>
__global__ void __launch_bounds__(IPR_THREADS) k_image_prep(const void* __restrict__ src, int SH, int SW, const float* __restrict__ lut,
                                                            const PrepItem* __restrict__ items, int item0, int oh, int ow, int rb, float* __restrict__ out) {
    __shared__ float s_lut[3 * 256];
    const int i = item0 + blockIdx.y, tid = threadIdx.x;
    const PrepItem P = items[i];
    const float* tab = lut + (size_t)(P.fl >> 1) * 768;
    for (int t = tid; t < 768; t += IPR_THREADS) s_lut[t] = tab[t];
    __syncthreads();
    const int flip = P.fl & 1;
    const int G = (ow + 3) >> 2;
    const int r0 = blockIdx.x * rb, nr = min(rb, oh - r0);
    const size_t plane = (size_t)oh * ow;
    float* o = out + (size_t)i * 3 * plane;
    for (int it = tid; it < nr * G; it += IPR_THREADS) {
        const int y = r0 + it / G, x = (it % G) * 4, npx = min(4, ow - x);
        const size_t sy = (size_t)(P.y0 + y), sx = (size_t)(P.x0 + (flip ? ow - x - npx : x));      // the npx source pixels, left to right
        uint32_t u[3][4];
        if (SF == 0) {
            // the aligned dwords that hold the 3 npx bytes (none of them lies wholly outside the image), shifted so that byte 0 is the first
            const uintptr_t a = (uintptr_t)((const uint8_t*)src + (((size_t)P.src * SH + sy) * SW + sx) * 3);
            const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
            const int sh = (int)(a & 3), nd = (sh + 3 * npx + 3) >> 2;
            const uint32_t w0 = q[0], w1 = nd > 1 ? q[1] : 0u, w2 = nd > 2 ? q[2] : 0u, w3 = nd > 3 ? q[3] : 0u;
            const uint32_t d[3] = {(uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * sh)), (uint32_t)((((uint64_t)w2 << 32) | w1) >> (8 * sh)),
                                   (uint32_t)((((uint64_t)w3 << 32) | w2) >> (8 * sh))};
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) u[c][k] = (d[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255u;
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* q = (const float*)src + (((size_t)P.src * 3 + c) * SH + sy) * SW + sx;
#pragma unroll
                for (int k = 0; k < 4; k++) u[c][k] = k < npx ? (uint32_t)jpg_u8(q[k]) : 0u;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v0 = s_lut[c * 256 + u[c][0]], v1 = s_lut[c * 256 + u[c][1]], v2 = s_lut[c * 256 + u[c][2]], v3 = s_lut[c * 256 + u[c][3]];
            float* dst = o + c * plane + (size_t)y * ow + x;
            if (npx == 4 && ((uintptr_t)dst & 15) == 0) {
                *(float4*)dst = flip ? make_float4(v3, v2, v1, v0) : make_float4(v0, v1, v2, v3);
            } else {
                for (int j = 0; j < npx; j++) dst[j] = ipr_pick(flip ? npx - 1 - j : j, v0, v1, v2, v3);
            }
        }
    }
}

// The host side: the per-call arrays (box, lut_index, src_index) go through the library's pinned staging (avsim_stage.h)
struct ImgPrepHost {
    // the conditions of the header on the host arrays; -1 and err says which
    static int validate(int nsrc, int SH, int SW, int nlut, const int32_t* lut_index, const int32_t* box, int nout, const int32_t* src_index, int oh,
                        int ow, std::string& err) {
        char buf[200];
        for (int i = 0; i < nout; i++) {
            const long long x0 = box[3 * (size_t)i], y0 = box[3 * (size_t)i + 1], fl = box[3 * (size_t)i + 2];
            const long long s = src_index ? src_index[i] : i, l = lut_index ? lut_index[i] : 0;
            const char* what = nullptr;
            if (s < 0 || s >= nsrc) what = "source image out of range";
            else if (l < 0 || l >= nlut) what = "table out of range";
            else if (fl != 0 && fl != 1) what = "flip is 0 or 1";
            else if (x0 < 0 || y0 < 0 || x0 + ow > SW || y0 + oh > SH) what = "the crop does not lie inside the source";
            if (what) {
                snprintf(buf, sizeof buf, "avsim_image_prep: output %d (source %lld, table %lld, box %lld %lld %lld): %s", i, s, l, x0, y0, fl, what);
                err = buf;
                return -1;
            }
        }
        return 0;
    }

    // src, lut, out: device pointers; the three arrays: host, validated.  -3: HIP
    static int launch(StageRing& ring, hipStream_t stream, const void* src, int sf, int SH, int SW, const float* lut, const int32_t* lut_index, const int32_t* box,
                      int nout, const int32_t* src_index, int oh, int ow, float* out, std::string& err) {
        const size_t bytes = (size_t)nout * sizeof(PrepItem);
        StageRing::Slot* sp = ring.acquire(bytes, err);
        if (!sp) return -3;
        StageRing::Slot& s = *sp;
        PrepItem* it = (PrepItem*)s.pin;
        for (int i = 0; i < nout; i++)
            it[i] = PrepItem{src_index ? src_index[i] : i, box[3 * (size_t)i], box[3 * (size_t)i + 1], box[3 * (size_t)i + 2] | ((lut_index ? lut_index[i] : 0) << 1)};
        if (ring.upload(s, bytes, stream, err)) return -3;
        const int G = (ow + 3) / 4;
        const int rb = std::min(oh, std::max(1, (4 * IPR_THREADS + G - 1) / G));      // some four items per lane
        const int bands = (oh + rb - 1) / rb;
        for (int i0 = 0; i0 < nout; i0 += 65535) {
            const dim3 grid(bands, std::min(65535, nout - i0));
            if (sf == 0) hipLaunchKernelGGL(k_image_prep<0>, grid, dim3(IPR_THREADS), 0, stream, src, SH, SW, lut, s.dev.as<const PrepItem>(), i0, oh, ow, rb, out);
            else hipLaunchKernelGGL(k_image_prep<1>, grid, dim3(IPR_THREADS), 0, stream, src, SH, SW, lut, s.dev.as<const PrepItem>(), i0, oh, ow, rb, out);
        }
        const hipError_t e = hipGetLastError();
        const int rc = ring.release(s, stream, err);
        if (e != hipSuccess) { err = std::string("image prep kernel: ") + hipGetErrorString(e); return -3; }
        return rc;
    }

    // img, index, out: device pointers
    static int stats(hipStream_t stream, const void* img, int fmt, const int* index, int nimg, int H, int W, unsigned long long* out, std::string& err) {
        const size_t HW = (size_t)H * W;
        hipLaunchKernelGGL(k_image_stats_init, dim3((3 * (unsigned)nimg + 255) / 256), dim3(256), 0, stream, out, 3 * nimg);
        // a slab: some eight steps per lane (units of 48 bytes, or pixels of a plane)
        const size_t steps = fmt == 0 ? 3 * HW / IST_UNIT : HW;
        const int slabs = (int)std::min<size_t>(IST_MAX_SLABS, std::max<size_t>(1, (steps + 8 * IST_THREADS - 1) / (8 * IST_THREADS)));
        for (int i0 = 0; i0 < nimg; i0 += 65535) {
            const dim3 grid(slabs, std::min(65535, nimg - i0));
            if (fmt == 0) hipLaunchKernelGGL(k_image_stats<0>, grid, dim3(IST_THREADS), 0, stream, img, index, i0, HW, out);
            else hipLaunchKernelGGL(k_image_stats<1>, grid, dim3(IST_THREADS), 0, stream, img, index, i0, HW, out);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = std::string("image stats kernels: ") + hipGetErrorString(e); return -3; }
        return 0;
    }
};

}  // namespace avs

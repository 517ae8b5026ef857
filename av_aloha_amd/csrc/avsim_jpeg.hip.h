// avsim_jpeg.hip.h -- baseline JPEG encoding of rendered frames on the device (avsim_jpeg_encode) and decoding of those streams
// (avsim_jpeg_decode; DESIGN 8.z: the section further down).
//
// The stream is the one av_aloha_amd/jpeg.py encode_reference writes, byte for byte: SOF0, 8 bit, JFIF, Y Cb Cr 4:2:0, the Annex K Huffman
// tables, one restart interval per MCU row.  All arithmetic is integer.  Two kernels:
//   k_jpeg_interval  one wave per restart interval (an MCU row of one image).  It walks the row in chunks of JPG_CHUNK MCUs (60 blocks): pixels ->
//                    level-shifted Y / subsampled Cb Cr planes in LDS; the two DCT passes with 8 lanes per block; quantiser + zigzag; then one
//                    block per lane for the entropy coder: code lengths, a wave prefix sum of bit offsets, the bits OR-ed into an LDS bit
//                    buffer, and a ballot pass that stuffs 0xFF bytes on the way to the interval's slot of the staging area.  DC predictors,
//                    the unfinished byte and the output position carry from chunk to chunk, so the row may be of any width.
//   k_jpeg_pack      per image: scans the interval lengths and copies header, intervals, RST markers and EOI to the caller's buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "avsim_dev.h"

namespace avs {

constexpr int JPG_HDR = 629;                 // SOI APP0 DQT DQT SOF0 DHT x 4 DRI SOS
constexpr int JPG_BLOCK_BITS = 63 * 26 + 22; // 63 AC coefficients of 16 + 10 bits, a DC difference of 11 + 11
constexpr int JPG_BLOCK_BYTES = (JPG_BLOCK_BITS + 7) / 8;
constexpr int JPG_CHUNK = 10;                // MCUs coded at a time
constexpr int JPG_NB = 6 * JPG_CHUNK;        // their blocks: one per lane in the entropy passes
constexpr int JPG_BSTRIDE = 33;              // dwords between the blocks of a coefficient array (64 int16 + 1 dword: no bank is hit twice)
constexpr int JPG_YW = 16 * JPG_CHUNK, JPG_CW = 8 * JPG_CHUNK;
constexpr int JPG_PLANE_WORDS = (16 * JPG_YW + 2 * 8 * JPG_CW) / 4;
constexpr int JPG_BIT_WORDS = (JPG_NB * JPG_BLOCK_BITS + 7 + 31) / 32 + 2;
static_assert(JPG_NB <= 64, "one block per lane");
static_assert(JPG_PLANE_WORDS + JPG_NB * JPG_BSTRIDE <= JPG_BIT_WORDS, "the planes and the row-pass result live in the bit buffer's space");

// what the kernels read, built on the host once per (height, width, quality)
struct JpegTables {
    uint32_t ac[2][256];  // code << 8 | length of symbol (run << 4 | size); luma, chroma
    uint32_t dc[2][16];
    int32_t q[2][64];     // quantiser steps, natural order
    float rq[2][64];      // 1 / (q << 15): the first guess of the quantiser's division
    uint8_t zz_inv[64];   // natural index -> zigzag position
    uint8_t hdr[JPG_HDR + 3];
};
constexpr int JPG_LDS_TABLE_WORDS = 2 * 256 + 2 * 16 + 2 * 64 + 2 * 64 + 16;       // everything up to and including zz_inv

__device__ constexpr int JPG_DCT[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                                          {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                                          {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                                          {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

__device__ __forceinline__ int jpg_u8(float v) {      // (int)(v * 255 + 0.5f), each operation rounded on its own, clamped to a byte
#pragma clang fp contract(off)
    const float x = v * 255.0f;
    const float y = x + 0.5f;
    return (int)fminf(fmaxf(y, 0.0f), 255.0f);
}
__device__ __forceinline__ int jpg_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// `len` bits (1 .. 26, most significant first) at bit `pos` of a big-endian bit buffer of dwords
__device__ __forceinline__ void jpg_put(uint32_t* bits, int pos, uint32_t v, int len) {
    const int w = pos >> 5, end = (pos & 31) + len;
    if (end <= 32) {
        atomicOr(&bits[w], v << (32 - end));
    } else {
        atomicOr(&bits[w], v >> (end - 32));
        atomicOr(&bits[w + 1], v << (64 - end));
    }
}

// the symbols of one block (Huffman code and amplitude bits together); EMIT false: only their total length
template <bool EMIT>
__device__ __forceinline__ int jpg_block(const uint32_t* ac, const uint32_t* dc, const int16_t* z, unsigned long long acmask, int pred, uint32_t* bits, int pos) {
    const int pos0 = pos;
    auto sym = [&](uint32_t e, int v, int n) {
        const int len = (int)(e & 255u) + n;
        if (EMIT) jpg_put(bits, pos, ((e >> 8) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), len);
        pos += len;
    };
    const int diff = (int)z[0] - pred;
    int n = 32 - __clz(diff < 0 ? -diff : diff);
    sym(dc[n], diff, n);
    int last = 0;
    while (acmask) {
        const int k = __ffsll((long long)acmask) - 1;
        acmask &= acmask - 1;
        int run = k - last - 1;
        last = k;
        while (run > 15) { sym(ac[0xF0], 0, 0); run -= 16; }
        const int v = z[k];
        n = 32 - __clz(v < 0 ? -v : v);
        sym(ac[(run << 4) | n], v, n);
    }
    if (last != 63) sym(ac[0], 0, 0);
    return pos - pos0;
}

// FMT 0: u8 [.][H][W][3]; 1: float32 [.][3][H][W] in [0, 1]
template <int FMT>
__global__ void __launch_bounds__(64) k_jpeg_interval(const JpegTables* __restrict__ T, const void* __restrict__ img, const int* __restrict__ index, int img0,
                                                      int H, int W, int mw, int mh, uint8_t* __restrict__ stage, int cap, int* __restrict__ ivlen) {
    __shared__ uint32_t s_tab[JPG_LDS_TABLE_WORDS];
    __shared__ uint32_t s_coef[JPG_NB * JPG_BSTRIDE];       // quantised coefficients, int16, zigzag order
    __shared__ uint32_t s_work[JPG_BIT_WORDS];              // the planes and the row pass's result, then the chunk's bits
    const int lane = threadIdx.x;
    const int iv = blockIdx.x, iml = iv / mh, row = iv - iml * mh;
    const size_t src = index ? (size_t)index[img0 + iml] : (size_t)(img0 + iml);
    for (int i = lane; i < JPG_LDS_TABLE_WORDS; i += 64) s_tab[i] = ((const uint32_t*)T)[i];
    const uint32_t* t_ac = s_tab;
    const uint32_t* t_dc = s_tab + 512;
    const int* t_q = (const int*)(s_tab + 544);
    const float* t_rq = (const float*)(s_tab + 672);
    const uint8_t* t_zz = (const uint8_t*)(s_tab + 800);
    int8_t* pY = (int8_t*)s_work;
    int8_t* pC = pY + 16 * JPG_YW;                          // Cb, then Cr
    uint32_t* tmp = s_work + JPG_PLANE_WORDS;
    uint8_t* dst = stage + (size_t)iv * cap;
    int pred_y = 0, pred_cb = 0, pred_cr = 0;               // DC predictors, the unfinished byte and the bytes written so far: wave-uniform
    int carry_n = 0, outpos = 0;
    uint32_t carry_v = 0;

    for (int mx0 = 0; mx0 < mw; mx0 += JPG_CHUNK) {
        const int nm = mw - mx0 < JPG_CHUNK ? mw - mx0 : JPG_CHUNK, nb = 6 * nm;
        __syncthreads();                                    // the tables; the previous chunk's bytes are out of s_work
        // 1. pixels -> planes: a lane takes a 2 x 2 group (4 Y, 1 Cb, 1 Cr); past the image's edge the last column / row repeats
        for (int g = lane; g < 8 * JPG_CW; g += 64) {
            const int gy = g / JPG_CW, gx = g - gy * JPG_CW;
            if (gx >= 8 * nm) continue;
            const int px = mx0 * 16 + 2 * gx, py = row * 16 + 2 * gy;
            int cb = 0, cr = 0;
#pragma unroll
            for (int dy = 0; dy < 2; dy++) {
                const size_t y = py + dy < H ? py + dy : H - 1;
                int yy[2];
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const size_t x = px + dx < W ? px + dx : W - 1;
                    int r, g8, b;
                    if (FMT == 0) {
                        const uint8_t* p = (const uint8_t*)img + ((src * H + y) * W + x) * 3;
                        r = p[0]; g8 = p[1]; b = p[2];
                    } else {
                        const float* p = (const float*)img + (src * 3 * H + y) * W + x;
                        const size_t plane = (size_t)H * W;
                        r = jpg_u8(p[0]); g8 = jpg_u8(p[plane]); b = jpg_u8(p[2 * plane]);
                    }
                    yy[dx] = jpg_clamp8((19595 * r + 38470 * g8 + 7471 * b + 32768) >> 16) - 128;
                    cb += jpg_clamp8(((-11059 * r - 21709 * g8 + 32768 * b + 32768) >> 16) + 128);
                    cr += jpg_clamp8(((32768 * r - 27439 * g8 - 5329 * b + 32768) >> 16) + 128);
                }
                *(uint16_t*)(pY + (2 * gy + dy) * JPG_YW + 2 * gx) = (uint16_t)((yy[0] & 255) | ((yy[1] & 255) << 8));
            }
            pC[gy * JPG_CW + gx] = (int8_t)(((cb + 2) >> 2) - 128);
            pC[8 * JPG_CW + gy * JPG_CW + gx] = (int8_t)(((cr + 2) >> 2) - 128);
        }
        __syncthreads();
        // 2. rows: lane (block, row) -> (sum + 1024) >> 11 as int16
        for (int t = lane; t < nb * 8; t += 64) {
            const int b = t >> 3, r = t & 7, m = b / 6, j = b - 6 * m;
            const int8_t* p = j < 4 ? pY + ((j >> 1) * 8 + r) * JPG_YW + m * 16 + (j & 1) * 8 : pC + (j - 4) * 8 * JPG_CW + r * JPG_CW + m * 8;
            const uint32_t lo = ((const uint32_t*)p)[0], hi = ((const uint32_t*)p)[1];
            int x[8];
#pragma unroll
            for (int n = 0; n < 4; n++) {
                x[n] = (int)(int8_t)(lo >> (8 * n));
                x[4 + n] = (int)(int8_t)(hi >> (8 * n));
            }
            int o[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int s = 1024;
#pragma unroll
                for (int n = 0; n < 8; n++) s += JPG_DCT[k][n] * x[n];
                o[k] = s >> 11;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) tmp[b * JPG_BSTRIDE + r * 4 + k] = (uint32_t)(o[2 * k] & 0xffff) | ((uint32_t)o[2 * k + 1] << 16);
        }
        __syncthreads();
        // 3. columns, quantiser (round half away from zero), zigzag: lane (block, column)
        for (int t = lane; t < nb * 8; t += 64) {
            const int b = t >> 3, c = t & 7, comp = (b % 6) < 4 ? 0 : 1;
            const int16_t* p = (const int16_t*)(tmp + b * JPG_BSTRIDE) + c;
            int x[8];
#pragma unroll
            for (int r = 0; r < 8; r++) x[r] = p[r * 8];
            int16_t* zc = (int16_t*)(s_coef + b * JPG_BSTRIDE);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int s = 0;
#pragma unroll
                for (int r = 0; r < 8; r++) s += JPG_DCT[k][r] * x[r];
                const int nat = k * 8 + c;
                const uint32_t den = (uint32_t)t_q[comp * 64 + nat] << 15, num = (uint32_t)(s < 0 ? -s : s) + (den >> 1);
                // num / den: num < 2^27 and the quotient < 2^12, so the float product is within 1 of it; two steps make it exact
                uint32_t v = (uint32_t)((float)num * t_rq[comp * 64 + nat]);
                if (v * den > num) v--;
                if ((v + 1) * den <= num) v++;
                zc[t_zz[nat]] = (int16_t)(s < 0 ? -(int)v : (int)v);
            }
        }
        __syncthreads();
        // 4. entropy coder: lane = block.  Lengths, prefix sum, bits.
        const bool live = lane < nb;
        const int b = live ? lane : 0, m = b / 6, j = b - 6 * m, comp = j < 4 ? 0 : 1;
        const int16_t* z = (const int16_t*)(s_coef + b * JPG_BSTRIDE);
        unsigned long long acmask = 0;
#pragma unroll 8
        for (int w = 0; w < 32; w++) {
            const uint32_t d = s_coef[b * JPG_BSTRIDE + w];
            acmask |= (unsigned long long)((d & 0xffffu) != 0) << (2 * w) | (unsigned long long)((d >> 16) != 0) << (2 * w + 1);
        }
        acmask &= ~1ull;
        int pred;
        if (j >= 4) pred = m > 0 ? ((const int16_t*)(s_coef + (b - 6) * JPG_BSTRIDE))[0] : (j == 4 ? pred_cb : pred_cr);
        else if (j > 0) pred = ((const int16_t*)(s_coef + (b - 1) * JPG_BSTRIDE))[0];
        else pred = m > 0 ? ((const int16_t*)(s_coef + (b - 3) * JPG_BSTRIDE))[0] : pred_y;
        const uint32_t* ac = t_ac + comp * 256;
        const uint32_t* dc = t_dc + comp * 16;
        const int nbits = live ? jpg_block<false>(ac, dc, z, acmask, pred, nullptr, 0) : 0;
        int incl = nbits;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        int total = carry_n + __shfl(incl, 63);
        const bool last_chunk = mx0 + JPG_CHUNK >= mw;
        const int pad = last_chunk ? (-total) & 7 : 0;
        for (int i = lane; i < ((total + pad + 31) >> 5) + 1; i += 64) s_work[i] = 0;      // (the planes are dead since step 3's barrier)
        __syncthreads();
        if (lane == 0) {
            if (carry_n) jpg_put(s_work, 0, carry_v, carry_n);
            if (pad) jpg_put(s_work, total, (1u << pad) - 1u, pad);                          // the interval ends on a byte, filled with ones
        }
        if (live) jpg_block<true>(ac, dc, z, acmask, pred, s_work, carry_n + incl - nbits);
        total += pad;
        pred_y = ((const int16_t*)(s_coef + ((nm - 1) * 6 + 3) * JPG_BSTRIDE))[0];
        pred_cb = ((const int16_t*)(s_coef + ((nm - 1) * 6 + 4) * JPG_BSTRIDE))[0];
        pred_cr = ((const int16_t*)(s_coef + ((nm - 1) * 6 + 5) * JPG_BSTRIDE))[0];
        __syncthreads();
        // 5. whole bytes -> staging, a zero after every 0xFF; the rest of the bits waits for the next chunk
        const int nbytes = total >> 3;
        for (int base = 0; base < nbytes; base += 64) {
            const int i = base + lane;
            const bool valid = i < nbytes;
            const uint32_t byte = valid ? (s_work[i >> 2] >> (24 - 8 * (i & 3))) & 255u : 0u;
            const bool ff = byte == 255u;
            const unsigned long long ffs = __ballot(ff);
            const int pos = outpos + lane + __popcll(ffs & ((1ull << lane) - 1ull));
            if (valid && pos < cap) dst[pos] = (uint8_t)byte;
            if (ff && pos + 1 < cap) dst[pos + 1] = 0;
            outpos += (nbytes - base < 64 ? nbytes - base : 64) + __popcll(ffs);
        }
        carry_n = total & 7;
        carry_v = carry_n ? ((s_work[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u) >> (8 - carry_n) : 0u;
    }
    if (lane == 0) ivlen[iv] = outpos;
}

// header, intervals with their RST markers, EOI -> out; blockIdx.x: image of the batch, blockIdx.y: the intervals y, y + gridDim.y, ...
__global__ void __launch_bounds__(256) k_jpeg_pack(const JpegTables* __restrict__ T, const uint8_t* __restrict__ stage, int cap, const int* __restrict__ ivlen,
                                                   int mh, int img0, uint8_t* __restrict__ out, long long stride, int* __restrict__ out_len) {
    __shared__ long long s_off[4096 + 1];
    const int iml = blockIdx.x, tid = threadIdx.x;
    if (tid < 64) {
        long long run = 0;
        for (int base = 0; base < mh; base += 64) {
            const int r = base + tid;
            const int v = r < mh ? ivlen[(size_t)iml * mh + r] : 0;
            int incl = v;                                   // (64 intervals of at most 4096 x 2496 bytes: the sum fits)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (tid >= d) incl += o;
            }
            if (r < mh) s_off[r] = run + (incl - v);
            run += __shfl(incl, 63);
        }
        if (tid == 0) s_off[mh] = run;
    }
    __syncthreads();
    uint8_t* o = out + (size_t)(img0 + iml) * stride;
    if (blockIdx.y == 0) {
        for (int i = tid; i < JPG_HDR; i += 256)
            if (i < stride) o[i] = T->hdr[i];
        const long long end = JPG_HDR + s_off[mh] + 2 * (long long)(mh - 1);
        if (tid < 2 && end + tid < stride) o[end + tid] = tid ? 0xD9 : 0xFF;
        if (tid == 0) out_len[img0 + iml] = end + 2 > 0x7fffffffLL ? 0x7fffffff : (int)(end + 2);
    }
    for (int r = blockIdx.y; r < mh; r += gridDim.y) {
        const long long d0 = JPG_HDR + s_off[r] + 2 * (long long)r;
        if (r > 0 && tid < 2 && d0 - 2 + tid < stride) o[d0 - 2 + tid] = tid ? (uint8_t)(0xD0 + ((r - 1) & 7)) : 0xFF;
        const long long len = s_off[r + 1] - s_off[r];
        const int n = (int)(len < cap ? len : cap);
        const uint8_t* s = stage + ((size_t)iml * mh + r) * cap;
        for (int i = tid; i < n; i += 256)
            if (d0 + i < stride) o[d0 + i] = s[i];
    }
}

// The views of an env side by side (avsim_render_jpeg, tile 1: the Cartesian env's zed_cam = left | right): src [n][ntile][H][rw] -> dst
// [n][H][ntile][rw] in units of U, rw = W * 3 / sizeof(U).  A bijection of [0, total): every index on either side is below total.
template <typename U>
__global__ void __launch_bounds__(256) k_jpeg_tile(const U* __restrict__ src, U* __restrict__ dst, int ntile, int H, int rw, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t x = i % rw, r = i / rw;            // r = (env * H + y) * ntile + view
        const size_t c = r % ntile, ny = r / ntile, y = ny % H, n = ny / H;
        dst[i] = src[((n * ntile + c) * H + y) * rw + x];
    }
}
inline int jpeg_tile(hipStream_t stream, const void* src, void* dst, int n, int ntile, int H, int W, std::string& err) {
    const size_t row = (size_t)W * 3;
    const bool words = row % 4 == 0;                    // (both buffers come from hipMalloc: a view then starts on a dword)
    const size_t total = (size_t)n * ntile * H * (words ? row / 4 : row);
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    if (words) hipLaunchKernelGGL(k_jpeg_tile<uint32_t>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, ntile, H, (int)(row / 4), total);
    else hipLaunchKernelGGL(k_jpeg_tile<uint8_t>, dim3(blocks), dim3(256), 0, stream, (const uint8_t*)src, (uint8_t*)dst, ntile, H, (int)row, total);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("jpeg tile kernel: ") + hipGetErrorString(e); return -3; }
    return 0;
}

// ---- decoding (avsim_jpeg_decode) ----------------------------------------------------------------------------------------------
// The streams of the encoder above and nothing else, as av_aloha_amd/jpeg.py decode_reference reads them, byte for byte.  Three kernels:
//   k_jpeg_index        per image: the header against the expected one for (H, W) outside the DQT payloads, the image's two quantiser tables,
//                       a block-wide scan for the RST markers (stuffing leaves FF 00 as the only FF pair inside entropy data), the intervals'
//                       byte ranges and the image's status.
//   k_jpeg_entropy      one restart interval per lane: Huffman decoding through two-level tables in LDS (8 + 8 bits) from a 64-bit window
//                       that drops the stuffed zeros on refill; the non-zero coefficients go to a zeroed int16 staging area
//                       [image][MCU row][MCU][block][64] in natural order.  Every read is bounded by the interval's end, every coefficient
//                       index by 63, the block count by the MCU row's: an error sets status bit 2 and ends that interval.
//   k_jpeg_reconstruct  a workgroup per JPD_K MCUs of an MCU row, 8 lanes per block: dequantiser, the two IDCT passes through LDS, the planes
//                       in LDS, then chroma upsampling and colour conversion per pixel.  The triangle filter needs one chroma row / column
//                       of the neighbouring blocks: those blocks are transformed again here (no second staging area).
constexpr int JPD_NSUB = 13;                 // second-level tables: the distinct 8-bit prefixes of the Annex K codes longer than 8 bits (1 + 5 + 1 + 6)
constexpr int JPD_K = 10;                    // MCUs per workgroup of k_jpeg_reconstruct
constexpr int JPD_BSTRIDE = 33;              // dwords between blocks in LDS (as JPG_BSTRIDE)
constexpr int JPD_DQT0 = 25, JPD_DQT1 = 94;  // the quantiser payloads inside the header
constexpr int JPD_SOF_SIZE = 163, JPD_DRI_MW = 613;

struct JpegDecTables {
    uint16_t l1[4][256];          // DC luma, AC luma, DC chroma, AC chroma by the next 8 bits: symbol << 5 | length, or table << 5 | 31; 0: no code
    uint16_t l2[JPD_NSUB][256];   // by the 8 bits after those: symbol << 5 | length (9 .. 16)
    uint8_t zz[64];               // zigzag position -> natural index
    float unit[256];              // (float)k / 255, divided on the host (see vis_u8_unit)
    uint8_t hdr[JPG_HDR + 3];     // the header of a 1 x 1 image: size and restart interval are patched in by the reader
};
constexpr int JPD_LDS_TABLE_WORDS = (4 * 256 + JPD_NSUB * 256) / 2 + 16;       // l1, l2, zz

__global__ void __launch_bounds__(256) k_jpeg_index(const JpegDecTables* __restrict__ T, const uint8_t* __restrict__ in, long long stride, const int* __restrict__ in_len,
                                                    const int* __restrict__ index, int img0, int H, int W, int mh, int* __restrict__ ivoff,
                                                    uint8_t* __restrict__ qtab, int* __restrict__ status) {
    __shared__ int s_wave[4];
    __shared__ int s_bad;
    const int iml = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, img = img0 + iml;
    const size_t src = index ? (size_t)index[img] : (size_t)img;
    const uint8_t* s = in + src * (size_t)stride;
    const long long len = in_len[src];
    int* off = ivoff + (size_t)iml * (mh + 1);          // off[r] + 2 .. off[r + 1]: the bytes of interval r
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (len < JPG_HDR + 2 || len > stride) {            // (uniform)
        if (tid == 0) status[img] = 2;
        return;
    }
    const int mw = (W + 15) >> 4;
    for (int i = tid; i < JPG_HDR; i += 256) {
        const int b = s[i];
        if (i >= JPD_DQT0 && i < JPD_DQT0 + 64) qtab[(size_t)iml * 128 + T->zz[i - JPD_DQT0]] = (uint8_t)b;
        else if (i >= JPD_DQT1 && i < JPD_DQT1 + 64) qtab[(size_t)iml * 128 + 64 + T->zz[i - JPD_DQT1]] = (uint8_t)b;
        else {
            int e = T->hdr[i];
            if (i == JPD_SOF_SIZE) e = H >> 8;
            else if (i == JPD_SOF_SIZE + 1) e = H & 255;
            else if (i == JPD_SOF_SIZE + 2) e = W >> 8;
            else if (i == JPD_SOF_SIZE + 3) e = W & 255;
            else if (i == JPD_DRI_MW) e = mw >> 8;
            else if (i == JPD_DRI_MW + 1) e = mw & 255;
            if (b != e) atomicOr(&s_bad, 1);
        }
    }
    __syncthreads();
    if (s_bad & 1) {
        if (tid == 0) status[img] = 1;
        return;
    }
    // the pairs (i, i + 1), JPG_HDR <= i < n: FF 00 is a stuffed byte, FF D0..D7 a restart marker, any other FF pair does not belong here
    const long long n = len - 2;
    int run = 0, bad = 0;
    for (long long base = JPG_HDR; base < n; base += 1024) {
        const long long p = base + 4 * tid;
        int b[5];
#pragma unroll
        for (int j = 0; j < 5; j++) b[j] = p + j <= n ? s[p + j] : 0;
        int c = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (p + j < n && b[j] == 0xFF) {
                if ((b[j + 1] & 0xF8) == 0xD0) c++;
                else if (b[j + 1] != 0) bad = 1;
            }
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        int ord = run + incl - c;
        for (int w = 0; w < wv; w++) ord += s_wave[w];
        run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (p + j < n && b[j] == 0xFF && (b[j + 1] & 0xF8) == 0xD0) {
                if (ord < mh - 1) {
                    off[ord + 1] = (int)(p + j);
                    if ((b[j + 1] & 7) != (ord & 7)) bad = 1;
                }
                ord++;
            }
        __syncthreads();
    }
    if (tid == 0) {
        off[0] = JPG_HDR - 2;
        off[mh] = (int)n;
        if (s[n] != 0xFF || s[n + 1] != 0xD9) bad = 1;
    }
    if (run != mh - 1) bad = 1;
    if (bad) atomicOr(&s_bad, 2);
    __syncthreads();
    if (tid == 0) status[img] = s_bad & 2;
}

__global__ void __launch_bounds__(64) k_jpeg_entropy(const JpegDecTables* __restrict__ T, const uint8_t* __restrict__ in, long long stride, const int* __restrict__ index,
                                                     int img0, int nimg, int mw, int mh, const int* __restrict__ ivoff, int16_t* __restrict__ coef, int* status) {
    __shared__ uint32_t s_tab[JPD_LDS_TABLE_WORDS];
    const int lane = threadIdx.x;
    for (int i = lane; i < JPD_LDS_TABLE_WORDS; i += 64) s_tab[i] = ((const uint32_t*)T)[i];
    __syncthreads();
    const uint16_t* l1 = (const uint16_t*)s_tab;
    const uint16_t* l2 = l1 + 4 * 256;
    const uint8_t* zz = (const uint8_t*)(l2 + JPD_NSUB * 256);
    const long long iv = (long long)blockIdx.x * 64 + lane;
    if (iv >= (long long)nimg * mh) return;
    const int iml = (int)(iv / mh), row = (int)(iv - (long long)iml * mh), img = img0 + iml;
    if (status[img] & 3) return;
    const uint8_t* s = in + (index ? (size_t)index[img] : (size_t)img) * (size_t)stride;
    long long pos = ivoff[(size_t)iml * (mh + 1) + row] + 2;
    const long long end = ivoff[(size_t)iml * (mh + 1) + row + 1];
    int16_t* c = coef + (size_t)iv * mw * 384;
    unsigned long long acc = 0;             // the next nb bits of the interval, from bit 63 down
    int nb = 0;
    auto refill = [&]() {
        while (nb <= 56 && pos < end) {
            const unsigned v = s[pos++];
            if (v == 0xFFu) pos++;          // (its stuffed zero: k_jpeg_index found no other pair in here)
            acc |= (unsigned long long)v << (56 - nb);
            nb += 8;
        }
    };
    auto symbol = [&](int tab) -> int {     // -1: no such code, or the bytes ran out
        refill();
        const unsigned pk = (unsigned)(acc >> 48);
        unsigned e = l1[tab * 256 + (pk >> 8)];
        if ((e & 31u) == 31u) e = l2[(e >> 5) * 256 + (pk & 255u)];
        const int len = (int)(e & 31u);
        if (len == 0 || len > nb) return -1;
        acc <<= len;
        nb -= len;
        return (int)(e >> 5);
    };
    auto amplitude = [&](int n, int& v) -> bool {      // 1 <= n <= 11; symbol() left 41 bits or all there are
        if (n > nb) return false;
        const int u = (int)(acc >> (64 - n));
        acc <<= n;
        nb -= n;
        v = u < (1 << (n - 1)) ? u - (1 << n) + 1 : u;
        return true;
    };
    int pred_y = 0, pred_cb = 0, pred_cr = 0;
    bool ok = true;
    for (int m = 0; m < mw && ok; m++) {
        for (int j = 0; j < 6 && ok; j++, c += 64) {
            const int comp = j < 4 ? 0 : 1;
            int n = symbol(2 * comp), d = 0;
            if (n < 0 || n > 11 || (n && !amplitude(n, d))) { ok = false; break; }
            const int pred = d + (j < 4 ? pred_y : j == 4 ? pred_cb : pred_cr);
            if (j < 4) pred_y = pred;
            else if (j == 4) pred_cb = pred;
            else pred_cr = pred;
            if (pred) c[0] = (int16_t)(pred < -32768 ? -32768 : pred > 32767 ? 32767 : pred);
            int k = 1;
            while (k < 64) {
                const int rs = symbol(2 * comp + 1);
                if (rs < 0) { ok = false; break; }
                if (rs == 0) break;
                n = rs & 15;
                k += rs >> 4;
                if (n > 10 || k + (n == 0) > 63) { ok = false; break; }
                if (n == 0) { k++; continue; }              // ZRL
                int v;
                if (!amplitude(n, v)) { ok = false; break; }
                c[zz[k]] = (int16_t)v;
                k++;
            }
        }
    }
    if (ok) {                               // fewer than 8 bits are left and all of them are 1
        refill();
        ok = pos >= end && nb < 8 && (nb == 0 || (acc >> (64 - nb)) == (1ull << nb) - 1ull);
    }
    if (!ok) atomicOr(&status[img], 4);
}

// FMT 0: u8 [.][H][W][3]; 1: float32 [.][3][H][W], (float)u8 / 255.  TRI: libjpeg's h2v2 triangle filter on the cropped chroma plane; else replication
template <int FMT, bool TRI>
__global__ void __launch_bounds__(256) k_jpeg_reconstruct(const JpegDecTables* __restrict__ T, const int16_t* __restrict__ coef, const uint8_t* __restrict__ qtab,
                                                          const int* __restrict__ status, int img0, int H, int W, int mw, int mh, void* __restrict__ out) {
    constexpr int YW = 16 * JPD_K;                          // the luma plane: 16 rows
    constexpr int CW = TRI ? 8 * (JPD_K + 2) : 8 * JPD_K;   // a chroma plane: with the filter, the blocks around the tile too
    constexpr int CR = TRI ? 24 : 8;
    constexpr int NCJ = TRI ? 3 * (JPD_K + 2) : JPD_K;      // chroma blocks per component
    constexpr int NJ = 4 * JPD_K + 2 * NCJ;
    __shared__ uint32_t s_f[NJ * JPD_BSTRIDE];              // dequantised coefficients, int16 [k][l]
    __shared__ uint32_t s_t[NJ * JPD_BSTRIDE];              // after the column pass, int16 [r][l]
    __shared__ uint32_t s_pl[(16 * YW + 2 * CR * CW) / 4];  // Y, Cb, Cr samples, u8
    __shared__ long long s_src[NJ];                         // a job's block in `coef`, -1: outside the image
    __shared__ int s_dst[NJ], s_dw[NJ];                     // its place in s_pl: byte offset, row stride
    __shared__ int16_t s_q[128];
    __shared__ float s_unit[256];
    const int tid = threadIdx.x, row = blockIdx.y, iml = blockIdx.z, m0 = blockIdx.x * JPD_K, img = img0 + iml;
    if (status[img]) return;                                // (uniform)
    if (tid < 128) s_q[tid] = qtab[(size_t)iml * 128 + tid];
    if (FMT == 1) s_unit[tid] = T->unit[tid];
    if (tid < NJ) {
        int r = row, m, jb, dst, dw;
        if (tid < 4 * JPD_K) {
            m = tid >> 2; jb = tid & 3;
            dst = (jb >> 1) * 8 * YW + m * 16 + (jb & 1) * 8; dw = YW;
            m += m0;
        } else {
            const int t = tid - 4 * JPD_K, comp = t / NCJ, u = t - comp * NCJ;
            const int dr = TRI ? u / (JPD_K + 2) : 0, mc = TRI ? u - dr * (JPD_K + 2) : u;
            jb = 4 + comp;
            dst = 16 * YW + comp * CR * CW + dr * 8 * CW + mc * 8; dw = CW;
            r = TRI ? row + dr - 1 : row;
            m = TRI ? m0 + mc - 1 : m0 + mc;
        }
        s_src[tid] = r >= 0 && r < mh && m >= 0 && m < mw ? (long long)(((((size_t)iml * mh + r) * mw + m) * 6 + jb) * 64) : -1;
        s_dst[tid] = dst; s_dw[tid] = dw;
    }
    __syncthreads();
    // 1. dequantiser: lane (block, k) takes the 8 coefficients F[k][.], clamps the products to [-2048, 2047]
    for (int t = tid; t < NJ * 8; t += 256) {
        const int b = t >> 3, k = t & 7;
        if (s_src[b] < 0) continue;
        const uint4 v = *(const uint4*)(coef + s_src[b] + k * 8);
        const int16_t* q = s_q + (b < 4 * JPD_K ? 0 : 64) + k * 8;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int lo = (int)(int16_t)(w[i] & 0xffffu) * q[2 * i], hi = (int)(int16_t)(w[i] >> 16) * q[2 * i + 1];
            lo = lo < -2048 ? -2048 : lo > 2047 ? 2047 : lo;
            hi = hi < -2048 ? -2048 : hi > 2047 ? 2047 : hi;
            s_f[b * JPD_BSTRIDE + k * 4 + i] = (uint32_t)(lo & 0xffff) | ((uint32_t)hi << 16);
        }
    }
    __syncthreads();
    // 2. columns: lane (block, l) -> t[r][l] = (sum_k M[k][r] F[k][l] + 1024) >> 11, |t| <= 32137
    for (int t = tid; t < NJ * 8; t += 256) {
        const int b = t >> 3, l = t & 7;
        if (s_src[b] < 0) continue;
        const int16_t* p = (const int16_t*)(s_f + b * JPD_BSTRIDE) + l;
        int x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = p[k * 8];
        int16_t* o = (int16_t*)(s_t + b * JPD_BSTRIDE) + l;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            int s = 1024;
#pragma unroll
            for (int k = 0; k < 8; k++) s += JPG_DCT[k][r] * x[k];
            o[r * 8] = (int16_t)(s >> 11);
        }
    }
    __syncthreads();
    // 3. rows: lane (block, r) -> p[r][c] = (sum_l M[l][c] t[r][l] + 16384) >> 15, + 128, a byte
    for (int t = tid; t < NJ * 8; t += 256) {
        const int b = t >> 3, r = t & 7;
        if (s_src[b] < 0) continue;
        int x[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t w = s_t[b * JPD_BSTRIDE + r * 4 + i];
            x[2 * i] = (int)(int16_t)(w & 0xffffu);
            x[2 * i + 1] = (int)(int16_t)(w >> 16);
        }
        uint32_t o[2] = {0, 0};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            int s = 16384;
#pragma unroll
            for (int l = 0; l < 8; l++) s += JPG_DCT[l][c] * x[l];
            o[c >> 2] |= (uint32_t)jpg_clamp8((s >> 15) + 128) << (8 * (c & 3));
        }
        uint32_t* d = s_pl + ((s_dst[b] + r * s_dw[b]) >> 2);
        d[0] = o[0]; d[1] = o[1];
    }
    __syncthreads();
    // 4. pixels of the tile that lie inside the image
    const uint8_t* pY = (const uint8_t*)s_pl;
    const uint8_t* pC = pY + 16 * YW;
    const int x0 = m0 * 16, y0 = row * 16, ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int cy0 = TRI ? row * 8 - 8 : row * 8, cx0 = TRI ? m0 * 8 - 8 : m0 * 8;
    auto pixel = [&](int y, int x, int& R, int& G, int& B) {
        const int Y = pY[(y - y0) * YW + (x - x0)];
        int cb, cr;
        const int cy = y >> 1, cx = x >> 1;
        if (TRI) {
            int ny = (y & 1) ? cy + 1 : cy - 1, nx = (x & 1) ? cx + 1 : cx - 1;
            ny = ny < 0 ? 0 : ny > ch - 1 ? ch - 1 : ny;
            nx = nx < 0 ? 0 : nx > cw - 1 ? cw - 1 : nx;
            const int a = (cy - cy0) * CW - cx0, n = (ny - cy0) * CW - cx0, rnd = (x & 1) ? 7 : 8;
            cb = (3 * (3 * pC[a + cx] + pC[n + cx]) + 3 * pC[a + nx] + pC[n + nx] + rnd) >> 4;
            cr = (3 * (3 * pC[CR * CW + a + cx] + pC[CR * CW + n + cx]) + 3 * pC[CR * CW + a + nx] + pC[CR * CW + n + nx] + rnd) >> 4;
        } else {
            cb = pC[(cy - cy0) * CW + cx - cx0];
            cr = pC[CR * CW + (cy - cy0) * CW + cx - cx0];
        }
        cb -= 128; cr -= 128;
        R = jpg_clamp8(Y + ((91881 * cr + 32768) >> 16));
        G = jpg_clamp8(Y - ((22554 * cb + 46802 * cr + 32768) >> 16));
        B = jpg_clamp8(Y + ((116130 * cb + 32768) >> 16));
    };
    if (FMT == 1) {
        float* o = (float*)out + (size_t)img * 3 * H * W;
        const size_t plane = (size_t)H * W;
        for (int p = tid; p < 16 * YW; p += 256) {
            const int yl = p / YW, y = y0 + yl, x = x0 + p - yl * YW;
            if (y >= H || x >= W) continue;
            int R, G, B;
            pixel(y, x, R, G, B);
            float* d = o + (size_t)y * W + x;
            d[0] = s_unit[R]; d[plane] = s_unit[G]; d[2 * plane] = s_unit[B];
        }
    } else {
        uint8_t* o = (uint8_t*)out + (size_t)img * H * W * 3;
        for (int p = tid; p < 16 * (YW / 4); p += 256) {          // four pixels, twelve bytes: three dwords where they are aligned
            const int yl = p / (YW / 4), y = y0 + yl, x = x0 + 4 * (p - yl * (YW / 4));
            if (y >= H || x >= W) continue;
            uint8_t* d = o + ((size_t)y * W + x) * 3;
            uint32_t w[3] = {0, 0, 0};
            const int np = W - x < 4 ? W - x : 4;
            for (int i = 0; i < np; i++) {
                int R, G, B;
                pixel(y, x + i, R, G, B);
                const int v[3] = {R, G, B};
#pragma unroll
                for (int k = 0; k < 3; k++) w[(3 * i + k) >> 2] |= (uint32_t)v[k] << (8 * ((3 * i + k) & 3));
            }
            if (np == 4 && ((uintptr_t)d & 3) == 0) {
                ((uint32_t*)d)[0] = w[0]; ((uint32_t*)d)[1] = w[1]; ((uint32_t*)d)[2] = w[2];
            } else {
                for (int i = 0; i < 3 * np; i++) d[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// T.81 Annex K: quantiser tables K.1 / K.2 (natural order), Huffman tables K.3 - K.6 (codes per length, symbols in code order)
static const uint8_t JPG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const uint8_t JPG_QUANT[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
static const uint8_t JPG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t JPG_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t JPG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t JPG_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

inline long long jpeg_bound(int H, int W) {
    const long long mh = (H + 15) / 16, mw = (W + 15) / 16;
    return JPG_HDR + mh * mw * 6 * 2 * JPG_BLOCK_BYTES + 2 * (mh - 1) + 2;
}

inline void jpeg_build_tables(int H, int W, int quality, JpegTables& t) {
    std::memset(&t, 0, sizeof t);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;        // libjpeg's quality rule
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < 64; i++) {
            int q = (JPG_QUANT[c][i] * scale + 50) / 100;
            q = q < 1 ? 1 : q > 255 ? 255 : q;
            t.q[c][i] = q;
            t.rq[c][i] = 1.0f / (float)((uint32_t)q << 15);
        }
    for (int i = 0; i < 64; i++) t.zz_inv[JPG_ZIGZAG[i]] = (uint8_t)i;
    auto codes = [](const uint8_t* bits, const uint8_t* vals, uint32_t* out) {   // T.81 Annex C
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
        return k;
    };
    uint8_t* p = t.hdr;
    auto put = [&](std::initializer_list<int> b) { for (int v : b) *p++ = (uint8_t)v; };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; c++) {
        put({0xFF, 0xDB, 0, 67, c});
        for (int i = 0; i < 64; i++) *p++ = (uint8_t)t.q[c][JPG_ZIGZAG[i]];
    }
    put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; c++) {
        const int ndc = codes(JPG_DC_BITS[c], JPG_DC_VALS, t.dc[c]);
        put({0xFF, 0xC4, 0, 19 + ndc, c});
        for (int i = 0; i < 16; i++) *p++ = JPG_DC_BITS[c][i];
        for (int i = 0; i < ndc; i++) *p++ = JPG_DC_VALS[i];
        const int nac = codes(JPG_AC_BITS[c], JPG_AC_VALS[c], t.ac[c]);
        put({0xFF, 0xC4, 0, 19 + nac, 0x10 | c});
        for (int i = 0; i < 16; i++) *p++ = JPG_AC_BITS[c][i];
        for (int i = 0; i < nac; i++) *p++ = JPG_AC_VALS[c][i];
    }
    const int mw = (W + 15) / 16;
    put({0xFF, 0xDD, 0, 4, mw >> 8, mw & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

struct JpegHost {
    struct Entry {
        int H, W, quality;
        DevBuf dev;                              // a JpegTables
        std::unique_ptr<JpegTables> host;        // the upload's source: never written again
    };
    std::vector<Entry> cache;                    // tables of the shapes / qualities seen
    DevBuf stage;                                // [images of a launch][interval][cap]: the intervals' bytes before they are packed
    DevBuf ivlen;
    size_t stage_budget = (size_t)512 << 20;     // a call whose staging would be larger goes through the kernels in groups of images

    int tables(hipStream_t stream, int H, int W, int quality, const JpegTables** out, std::string& err) {
        for (auto& e : cache)
            if (e.H == H && e.W == W && e.quality == quality) { *out = e.dev.as<JpegTables>(); return 0; }
        if (cache.size() >= 64) {                // (a caller that walks through shapes: start over once nothing reads the old ones)
            (void)hipStreamSynchronize(stream);
            cache.clear();
        }
        Entry e{H, W, quality, DevBuf{}, std::make_unique<JpegTables>()};
        jpeg_build_tables(H, W, quality, *e.host);
        hipError_t rc = e.dev.reserve(sizeof(JpegTables));
        if (rc == hipSuccess) rc = hipMemcpyAsync(e.dev.ptr(), e.host.get(), sizeof(JpegTables), hipMemcpyHostToDevice, stream);
        if (rc != hipSuccess) { err = std::string("jpeg tables: ") + hipGetErrorString(rc); return -3; }
        *out = e.dev.as<JpegTables>();
        cache.push_back(std::move(e));
        return 0;
    }
    // img, index, out, out_len: device pointers
    int launch(hipStream_t stream, const void* img, int fmt, const int* index, int nimg, int H, int W, int quality, uint8_t* out, long long stride,
               int* out_len, std::string& err) {
        const JpegTables* T = nullptr;
        int rc = tables(stream, H, W, quality, &T, err);
        if (rc) return rc;
        const int mh = (H + 15) / 16, mw = (W + 15) / 16;
        // an interval longer than the caller's stride belongs to a stream that does not fit: its tail is counted, not kept
        long long cap = (long long)mw * 6 * 2 * JPG_BLOCK_BYTES;
        if (cap > stride) cap = stride;
        cap = cap < 16 ? 16 : (cap + 15) & ~15LL;
        const size_t per_img = (size_t)mh * cap;
        size_t group = stage_budget / per_img;
        group = group < 1 ? 1 : group > (size_t)nimg ? (size_t)nimg : group;
        if (group * mh > 0x3fffffffULL) group = 0x3fffffffULL / mh;
        if (stage.reserve(group * per_img) != hipSuccess || ivlen.reserve(group * mh * sizeof(int)) != hipSuccess) { err = "jpeg staging: hipMalloc failed"; return -3; }
        uint8_t* const d_stage = stage.as<uint8_t>();
        int* const d_ivlen = ivlen.as<int>();
        for (int i0 = 0; i0 < nimg; i0 += (int)group) {
            const int n = nimg - i0 < (int)group ? nimg - i0 : (int)group;
            if (fmt == 0) hipLaunchKernelGGL(k_jpeg_interval<0>, dim3(n * mh), dim3(64), 0, stream, T, img, index, i0, H, W, mw, mh, d_stage, (int)cap, d_ivlen);
            else hipLaunchKernelGGL(k_jpeg_interval<1>, dim3(n * mh), dim3(64), 0, stream, T, img, index, i0, H, W, mw, mh, d_stage, (int)cap, d_ivlen);
            hipLaunchKernelGGL(k_jpeg_pack, dim3(n, mh < 8 ? mh : 8), dim3(256), 0, stream, T, d_stage, (int)cap, d_ivlen, mh, i0, out, stride, out_len);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = std::string("jpeg kernels: ") + hipGetErrorString(e); return -3; }
        return 0;
    }
};

inline int jpeg_build_dec_tables(JpegDecTables& t) {
    std::memset(&t, 0, sizeof t);
    const uint8_t* bits[4] = {JPG_DC_BITS[0], JPG_AC_BITS[0], JPG_DC_BITS[1], JPG_AC_BITS[1]};
    const uint8_t* vals[4] = {JPG_DC_VALS, JPG_AC_VALS[0], JPG_DC_VALS, JPG_AC_VALS[1]};
    int nsub = 0;
    for (int tab = 0; tab < 4; tab++) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < bits[tab][len - 1]; i++, code++) {
                const uint16_t e = (uint16_t)((vals[tab][k++] << 5) | len);
                if (len <= 8) {
                    for (uint32_t x = code << (8 - len); x < (code + 1) << (8 - len); x++) t.l1[tab][x] = e;
                } else {
                    const uint32_t pre = code >> (len - 8), low = code & ((1u << (len - 8)) - 1u);
                    if (!t.l1[tab][pre]) {
                        if (nsub == JPD_NSUB) return -1;
                        t.l1[tab][pre] = (uint16_t)((nsub++ << 5) | 31);
                    }
                    uint16_t* sub = t.l2[t.l1[tab][pre] >> 5];
                    for (uint32_t x = low << (16 - len); x < (low + 1) << (16 - len); x++) sub[x] = e;
                }
            }
            code <<= 1;
        }
    }
    for (int i = 0; i < 64; i++) t.zz[i] = JPG_ZIGZAG[i];
    for (int k = 0; k < 256; k++) t.unit[k] = (float)k / 255.0f;
    JpegTables enc;
    jpeg_build_tables(1, 1, 50, enc);
    std::memcpy(t.hdr, enc.hdr, sizeof t.hdr);
    return 0;
}

struct JpegDecHost {
    DevBuf tab;                                  // a JpegDecTables
    std::unique_ptr<JpegDecTables> host;         // the upload's source: never written again
    DevBuf coef;                                 // int16 [images of a launch][MCU row][MCU][6][64]: zeroed, then the entropy decoder's coefficients
    DevBuf ivoff;                                // int [image][mh + 1]
    DevBuf qtab;                                 // u8 [image][2][64], natural order
    size_t coef_budget = (size_t)512 << 20;      // a call whose staging would be larger goes through the kernels in groups of images

    // in, in_len, index, out, status: device pointers
    int launch(hipStream_t stream, const uint8_t* in, long long stride, const int* in_len, const int* index, int nimg, int H, int W, int fmt, int upsample,
               void* out, int* status, std::string& err, hipEvent_t* ev = nullptr) {          // ev: four events recorded around the three kernels (of the last group)
        if (!tab) {
            host = std::make_unique<JpegDecTables>();
            if (jpeg_build_dec_tables(*host)) { err = "jpeg decode tables: more long-code prefixes than JPD_NSUB"; host.reset(); return -3; }
            hipError_t rc = tab.reserve(sizeof(JpegDecTables));
            if (rc == hipSuccess) rc = hipMemcpyAsync(tab.ptr(), host.get(), sizeof(JpegDecTables), hipMemcpyHostToDevice, stream);
            if (rc != hipSuccess) { tab.free(); err = std::string("jpeg decode tables: ") + hipGetErrorString(rc); return -3; }
        }
        const int mh = (H + 15) / 16, mw = (W + 15) / 16;
        const size_t per_img = (size_t)mh * mw * 384;                 // coefficients
        size_t group = coef_budget / (per_img * sizeof(int16_t));
        group = group < 1 ? 1 : group > (size_t)nimg ? (size_t)nimg : group;
        if (group > 65535) group = 65535;                             // (gridDim.z)
        if (coef.reserve(group * per_img * sizeof(int16_t)) != hipSuccess || ivoff.reserve(group * (mh + 1) * sizeof(int)) != hipSuccess || qtab.reserve(group * 128) != hipSuccess) {
            err = "jpeg decode staging: hipMalloc failed";
            return -3;
        }
        const JpegDecTables* const d_tab = tab.as<JpegDecTables>();
        int16_t* const d_coef = coef.as<int16_t>();
        int* const d_ivoff = ivoff.as<int>();
        uint8_t* const d_qtab = qtab.as<uint8_t>();
        const int nchunk = (mw + JPD_K - 1) / JPD_K;
        for (int i0 = 0; i0 < nimg; i0 += (int)group) {
            const int n = nimg - i0 < (int)group ? nimg - i0 : (int)group;
            if (hipMemsetAsync(d_coef, 0, (size_t)n * per_img * sizeof(int16_t), stream) != hipSuccess) { err = "jpeg decode staging: hipMemsetAsync failed"; return -3; }
            if (ev) (void)hipEventRecord(ev[0], stream);
            hipLaunchKernelGGL(k_jpeg_index, dim3(n), dim3(256), 0, stream, d_tab, in, stride, in_len, index, i0, H, W, mh, d_ivoff, d_qtab, status);
            if (ev) (void)hipEventRecord(ev[1], stream);
            hipLaunchKernelGGL(k_jpeg_entropy, dim3((unsigned)(((size_t)n * mh + 63) / 64)), dim3(64), 0, stream, d_tab, in, stride, index, i0, n, mw, mh, d_ivoff, d_coef, status);
            if (ev) (void)hipEventRecord(ev[2], stream);
            const dim3 grid(nchunk, mh, n);
#define JPD_RECON(F, T) hipLaunchKernelGGL((k_jpeg_reconstruct<F, T>), grid, dim3(256), 0, stream, d_tab, d_coef, d_qtab, status, i0, H, W, mw, mh, out)
            if (fmt == 0 && !upsample) JPD_RECON(0, false);
            else if (fmt == 0) JPD_RECON(0, true);
            else if (!upsample) JPD_RECON(1, false);
            else JPD_RECON(1, true);
#undef JPD_RECON
            if (ev) (void)hipEventRecord(ev[3], stream);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = std::string("jpeg decode kernels: ") + hipGetErrorString(e); return -3; }
        return 0;
    }
};

}  // namespace avs

// avsim_compose.hip.h -- camera views composed on the device (avsim_compose, avsim_compose_label): an image is resampled and
// written into a rectangle of a larger canvas, and a line of text is painted over it.
//
// The pixels are those of av_aloha_amd/compose.py compose_reference / label_reference, byte for byte: a separable triangle filter whose
// support grows with the shrink factor, in Pillow's fixed-point scheme (22 fractional bits).  The coefficients are computed on the host, in
// double, once per (input size, output size) pair; the device does integer arithmetic only.  Three kernels:
//   k_compose        one workgroup per placement and 8 x 64 tile of its rectangle: the horizontal pass over the source rows the tile needs goes
//                    into LDS as bytes, the vertical pass reads them there and stores to the canvas.  Rows that two tiles share are computed
//                    by both (as k_jpeg_reconstruct computes its neighbour blocks twice); the horizontal result never reaches global memory.
//   k_compose_fill   the whole canvas in one colour (clear = 1), in front of k_compose on the same stream.
//   k_compose_label  one workgroup per label: prefix + the decimal digits of an int64 read on the device, 5 x 7 glyphs in 6 x 8 cells.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "avsim_jpeg.hip.h"

namespace avs {

constexpr int CMP_TW = 64, CMP_TH = 8;       // an output tile: 64 pixels of 8 rows
constexpr int CMP_THREADS = 3 * CMP_TW;      // a thread per byte of a tile row
constexpr int CMP_MAX_RATIO = 16;            // n_in / n_out per axis (enlarging is unbounded)
// source rows under an output tile: lo(first row) > (i0 + 0.5) s - s - 0.5 and hi(last row) <= (i0 + TH - 0.5) s + s + 0.5, so at most
// (TH + 1) s + 1 rows, 145 at s = 16; the host checks every tile of a table against this before anything is launched
constexpr int CMP_ROWS = (CMP_TH + 1) * CMP_MAX_RATIO + 4;
constexpr int CMP_LDS_BYTES = CMP_ROWS * CMP_THREADS;      // 28 416 B: five workgroups (15 waves) on a CU's 160 KiB
constexpr int CMP_PREC = 22;                 // fractional bits of a coefficient (Pillow's 32 - 8 - 2)
constexpr int CMP_PREFIX = 15, CMP_TEXT = CMP_PREFIX + 20;      // a label: the prefix, then at most 19 digits and a sign
constexpr int CMP_MAX_SCALE = 64;
constexpr int CMP_NGLYPH = 41;

// The font: 5 x 7 glyphs, a byte per row, bit 4 = the left pixel.  Digits, A-Z, then : . - = /   (this project's own drawing)
#define CMP_FONT_ROWS                                                                                                                       \
    {{0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110}, {0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110},      \
     {0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111}, {0b11110, 0b00001, 0b00001, 0b01110, 0b00001, 0b00001, 0b11110},      \
     {0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010}, {0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110},      \
     {0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110}, {0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000},      \
     {0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110}, {0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100},      \
     {0b01110, 0b10001, 0b10001, 0b11111, 0b10001, 0b10001, 0b10001}, {0b11110, 0b10001, 0b10001, 0b11110, 0b10001, 0b10001, 0b11110},      \
     {0b01110, 0b10001, 0b10000, 0b10000, 0b10000, 0b10001, 0b01110}, {0b11100, 0b10010, 0b10001, 0b10001, 0b10001, 0b10010, 0b11100},      \
     {0b11111, 0b10000, 0b10000, 0b11110, 0b10000, 0b10000, 0b11111}, {0b11111, 0b10000, 0b10000, 0b11110, 0b10000, 0b10000, 0b10000},      \
     {0b01110, 0b10001, 0b10000, 0b10111, 0b10001, 0b10001, 0b01111}, {0b10001, 0b10001, 0b10001, 0b11111, 0b10001, 0b10001, 0b10001},      \
     {0b01110, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110}, {0b00111, 0b00010, 0b00010, 0b00010, 0b00010, 0b10010, 0b01100},      \
     {0b10001, 0b10010, 0b10100, 0b11000, 0b10100, 0b10010, 0b10001}, {0b10000, 0b10000, 0b10000, 0b10000, 0b10000, 0b10000, 0b11111},      \
     {0b10001, 0b11011, 0b10101, 0b10101, 0b10001, 0b10001, 0b10001}, {0b10001, 0b11001, 0b10101, 0b10011, 0b10001, 0b10001, 0b10001},      \
     {0b01110, 0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b01110}, {0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000, 0b10000},      \
     {0b01110, 0b10001, 0b10001, 0b10001, 0b10101, 0b10010, 0b01101}, {0b11110, 0b10001, 0b10001, 0b11110, 0b10100, 0b10010, 0b10001},      \
     {0b01111, 0b10000, 0b10000, 0b01110, 0b00001, 0b00001, 0b11110}, {0b11111, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100},      \
     {0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b01110}, {0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b01010, 0b00100},      \
     {0b10001, 0b10001, 0b10001, 0b10101, 0b10101, 0b11011, 0b10001}, {0b10001, 0b10001, 0b01010, 0b00100, 0b01010, 0b10001, 0b10001},      \
     {0b10001, 0b10001, 0b01010, 0b00100, 0b00100, 0b00100, 0b00100}, {0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b10000, 0b11111},      \
     {0b00000, 0b00100, 0b00100, 0b00000, 0b00100, 0b00100, 0b00000}, {0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00110, 0b00110},      \
     {0b00000, 0b00000, 0b00000, 0b11111, 0b00000, 0b00000, 0b00000}, {0b00000, 0b00000, 0b11111, 0b00000, 0b11111, 0b00000, 0b00000},      \
     {0b00001, 0b00001, 0b00010, 0b00100, 0b01000, 0b10000, 0b10000}}
__device__ constexpr uint8_t CMP_FONT[CMP_NGLYPH][7] = CMP_FONT_ROWS;
static constexpr uint8_t CMP_FONT_HOST[CMP_NGLYPH][7] = CMP_FONT_ROWS;

// the glyph of a character, -1: none (draws as a space)
__host__ __device__ inline int cmp_glyph(int ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'A' && ch <= 'Z') return 10 + ch - 'A';
    return ch == ':' ? 36 : ch == '.' ? 37 : ch == '-' ? 38 : ch == '=' ? 39 : ch == '/' ? 40 : -1;
}

// One placement as the kernel reads it.  A table (h: along a row, v: along a column) holds, for the n_out output coordinates of its axis,
// [lo: n_out][count: n_out][k: n_out x ks]; nullptr = the sizes are equal and the pass copies.
struct ComposePlace {
    int out, src, x0, y0, w, h, hks, vks;
    const int* htab;
    const int* vtab;
};
struct ComposeText { char c[CMP_PREFIX + 1]; };

template <int SF>
__device__ __forceinline__ int cmp_load(const void* __restrict__ src, size_t img, int SH, int SW, int row, int col, int c) {
    if (SF == 0) return ((const uint8_t*)src)[((img * SH + row) * SW + col) * 3 + c];
    return jpg_u8(((const float*)src)[((img * 3 + c) * SH + row) * SW + col]);
}

// SF / DF: the format of the source / the canvas, 0 = u8 [n][H][W][3], 1 = float32 [n][3][H][W] (read as (int)(v * 255 + 0.5f), written as unit[u8])
template <int SF, int DF>
__global__ void __launch_bounds__(CMP_THREADS) k_compose(const ComposePlace* __restrict__ places, int place0, const void* __restrict__ src, int SH, int SW,
                                                         void* __restrict__ canvas, int CH, int CW, const float* __restrict__ unit) {
    __shared__ uint8_t s_h[CMP_LDS_BYTES];       // [source row of the tile][64 pixels][3]: the horizontal pass's result
    const ComposePlace P = places[place0 + blockIdx.z];
    const int tx0 = blockIdx.x * CMP_TW, ty0 = blockIdx.y * CMP_TH;
    if (tx0 >= P.w || ty0 >= P.h) return;         // (the grid is sized for the call's largest rectangle)
    const int tw = min(CMP_TW, P.w - tx0), th = min(CMP_TH, P.h - ty0);
    int row0 = ty0, nrows = th;
    if (P.vtab) {                                 // lo and lo + count do not decrease along the axis
        row0 = P.vtab[ty0];
        nrows = P.vtab[ty0 + th - 1] + P.vtab[P.h + ty0 + th - 1] - row0;
        nrows = min(nrows, min(CMP_ROWS, SH - row0));
    }
    const int t = threadIdx.x;
    {   // horizontal pass: a thread keeps one byte column of the tile; with planes as the source the lanes of a wave read along a row of one plane
        const int x = SF == 0 ? t / 3 : t & (CMP_TW - 1), c = SF == 0 ? t % 3 : t >> 6;
        if (x < tw) {
            const int ox = tx0 + x;
            const size_t img = (size_t)P.src;
            uint8_t* dst = s_h + x * 3 + c;
            if (P.htab) {
                const int lo = P.htab[ox], cnt = P.htab[P.w + ox];
                const int* __restrict__ k = P.htab + 2 * (size_t)P.w + (size_t)ox * P.hks;
                for (int r = 0; r < nrows; r++) {
                    int acc = 1 << (CMP_PREC - 1);
                    for (int j = 0; j < cnt; j++) acc += k[j] * cmp_load<SF>(src, img, SH, SW, row0 + r, lo + j, c);
                    dst[r * CMP_THREADS] = (uint8_t)jpg_clamp8(acc >> CMP_PREC);
                }
            } else {
                for (int r = 0; r < nrows; r++) dst[r * CMP_THREADS] = (uint8_t)cmp_load<SF>(src, img, SH, SW, row0 + r, ox, c);
            }
        }
    }
    __syncthreads();
    {   // vertical pass out of LDS; the lanes of a wave store along a canvas row (of one plane when the canvas is planes)
        const int x = DF == 0 ? t / 3 : t & (CMP_TW - 1), c = DF == 0 ? t % 3 : t >> 6;
        if (x < tw) {
            const uint8_t* col = s_h + x * 3 + c;
            const size_t cx = (size_t)(P.x0 + tx0 + x);
            for (int y = 0; y < th; y++) {
                const int oy = ty0 + y;
                int v;
                if (P.vtab) {
                    const int lo = P.vtab[oy] - row0, cnt = P.vtab[P.h + oy];
                    const int* __restrict__ k = P.vtab + 2 * (size_t)P.h + (size_t)oy * P.vks;
                    int acc = 1 << (CMP_PREC - 1);
                    for (int j = 0; j < cnt; j++) {
                        const int r = min(lo + j, nrows - 1);
                        acc += k[j] * col[r * CMP_THREADS];
                    }
                    v = jpg_clamp8(acc >> CMP_PREC);
                } else {
                    v = col[y * CMP_THREADS];
                }
                const size_t cy = (size_t)(P.y0 + oy);
                if (DF == 0) ((uint8_t*)canvas)[(((size_t)P.out * CH + cy) * CW + cx) * 3 + c] = (uint8_t)v;
                else ((float*)canvas)[(((size_t)P.out * 3 + c) * CH + cy) * CW + cx] = unit[v];
            }
        }
    }
}

// the canvas in one colour: u8 as dwords where the buffer starts on one (a period of three dwords), else as bytes; float32 per element
template <int DF>
__global__ void __launch_bounds__(256) k_compose_fill(void* __restrict__ canvas, size_t total, size_t plane, uint32_t rgb, const float* __restrict__ unit) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t ch[3] = {(rgb >> 16) & 255u, (rgb >> 8) & 255u, rgb & 255u};
    if (DF == 1) {
        const float f0 = unit[ch[0]], f1 = unit[ch[1]], f2 = unit[ch[2]];
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const int c = (int)((i / plane) % 3);
            ((float*)canvas)[i] = c == 0 ? f0 : c == 1 ? f1 : f2;
        }
        return;
    }
    // byte i holds channel i % 3: the three dwords of a period
    const uint32_t w0 = ch[0] | ch[1] << 8 | ch[2] << 16 | ch[0] << 24, w1 = ch[1] | ch[2] << 8 | ch[0] << 16 | ch[1] << 24,
                   w2 = ch[2] | ch[0] << 8 | ch[1] << 16 | ch[2] << 24;
    uint8_t* p = (uint8_t*)canvas;
    if (((uintptr_t)p & 3) == 0) {
        const size_t words = total / 4;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
            const int m = (int)(i % 3);
            ((uint32_t*)p)[i] = m == 0 ? w0 : m == 1 ? w1 : w2;
        }
        for (size_t i = words * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const int m = (int)(i % 3);
            p[i] = (uint8_t)(m == 0 ? ch[0] : m == 1 ? ch[1] : ch[2]);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const int m = (int)(i % 3);
            p[i] = (uint8_t)(m == 0 ? ch[0] : m == 1 ? ch[1] : ch[2]);
        }
    }
}

// where: int32 [nlabel][4] = out image, x, y, scale (validated by the host); value: int64 [nlabel] or nullptr.  Pixels outside the canvas are skipped.
template <int DF>
__global__ void __launch_bounds__(256) k_compose_label(const int* __restrict__ where, ComposeText prefix, int nprefix, const long long* __restrict__ value,
                                                       void* __restrict__ canvas, int CH, int CW, uint32_t rgb, const float* __restrict__ unit) {
    __shared__ int s_glyph[CMP_TEXT];
    __shared__ int s_n;
    const int lab = blockIdx.x;
    const int out = where[4 * lab], x0 = where[4 * lab + 1], y0 = where[4 * lab + 2], scale = where[4 * lab + 3];
    if (threadIdx.x == 0) {
        int n = 0;
        for (; n < nprefix; n++) s_glyph[n] = cmp_glyph(prefix.c[n]);
        if (value) {
            const long long v = value[lab];
            unsigned long long m = v < 0 ? 0ULL - (unsigned long long)v : (unsigned long long)v;
            if (v < 0) s_glyph[n++] = cmp_glyph('-');
            int nd = 1;
            for (unsigned long long q = m; q >= 10; q /= 10) nd++;
            for (int d = nd - 1; d >= 0; d--, m /= 10) s_glyph[n + d] = (int)(m % 10);
            n += nd;
        }
        s_n = n;
    }
    __syncthreads();
    const int cw = 6 * scale, chh = 8 * scale, n = s_n;
    const int total = n * cw * chh;
    const uint32_t ch[3] = {(rgb >> 16) & 255u, (rgb >> 8) & 255u, rgb & 255u};
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int py = i / (n * cw), px = i % (n * cw);
        const int g = s_glyph[px / cw], gx = (px % cw) / scale, gy = py / scale;
        if (g < 0 || gx >= 5 || gy >= 7 || !((CMP_FONT[g][gy] >> (4 - gx)) & 1)) continue;
        const long long x = (long long)x0 + px, y = (long long)y0 + py;
        if (x < 0 || y < 0 || x >= CW || y >= CH) continue;
        if (DF == 0) {
            uint8_t* p = (uint8_t*)canvas + (((size_t)out * CH + (size_t)y) * CW + (size_t)x) * 3;
            p[0] = (uint8_t)ch[0]; p[1] = (uint8_t)ch[1]; p[2] = (uint8_t)ch[2];
        } else {
            float* p = (float*)canvas + ((size_t)out * 3 * CH + (size_t)y) * CW + (size_t)x;
            const size_t plane = (size_t)CH * CW;
            p[0] = unit[ch[0]]; p[plane] = unit[ch[1]]; p[2 * plane] = unit[ch[2]];
        }
    }
}

// The coefficients of one axis, in double (compose.py axis_table, Pillow's precompute_coeffs + normalize_coeffs_8bpc): -> [lo][count][k], ks taps per row
inline void compose_axis_table(int n_in, int n_out, std::vector<int>& tab, int& ks) {
#pragma clang fp contract(off)
    const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale, support = fs;
    ks = 2 * (int)std::ceil(support) + 1;
    tab.assign((size_t)n_out * (2 + ks), 0);
    std::vector<double> w((size_t)ks);
    for (int i = 0; i < n_out; i++) {
        const double center = (i + 0.5) * scale;
        int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_in ? n_in : hi;
        const int cnt = hi - lo;
        double sum = 0.0;
        for (int j = 0; j < cnt; j++) {
            const double a = std::fabs(((double)(j + lo) - center + 0.5) / fs);
            w[j] = a < 1.0 ? 1.0 - a : 0.0;
            sum += w[j];
        }
        tab[i] = lo;
        tab[(size_t)n_out + i] = cnt;
        for (int j = 0; j < cnt; j++) {
            const double v = sum != 0.0 ? w[j] / sum : w[j];
            tab[2 * (size_t)n_out + (size_t)i * ks + j] = (int)(0.5 + v * (double)(1 << CMP_PREC));
        }
    }
}

struct ComposeHost {
    struct Table {
        int n_in, n_out, ks;
        DevBuf dev;
        std::unique_ptr<std::vector<int>> host;      // the upload's source: never written again
    };
    struct Call {                                    // the validated host arrays of a call and their device form
        std::vector<int32_t> key;
        DevBuf dev;
        std::unique_ptr<std::vector<uint8_t>> host;
        int gx, gy;
    };
    std::vector<Table> tables;
    std::vector<Call> calls;
    DevBuf d_unit;
    std::unique_ptr<std::vector<float>> unit_host;

    void drop(hipStream_t stream) {
        (void)hipStreamSynchronize(stream);
        tables.clear();
        calls.clear();
    }
    int upload(hipStream_t stream, const void* host, size_t bytes, DevBuf& dev, std::string& err) {
        hipError_t rc = dev.alloc(bytes ? bytes : 4);
        if (rc == hipSuccess && bytes) rc = hipMemcpyAsync(dev.ptr(), host, bytes, hipMemcpyHostToDevice, stream);
        if (rc != hipSuccess) {
            dev.free();
            err = std::string("compose tables: ") + hipGetErrorString(rc);
            return -3;
        }
        return 0;
    }
    int unit(hipStream_t stream, std::string& err) {
        if (d_unit) return 0;
        unit_host = std::make_unique<std::vector<float>>(256);
        for (int k = 0; k < 256; k++) (*unit_host)[k] = (float)k / 255.0f;      // divided on the host, as the renderer's and the decoder's table
        return upload(stream, unit_host->data(), 256 * sizeof(float), d_unit, err);
    }
    // the table of an axis (nullptr for equal sizes); -1: some tile would need more rows than the kernel's LDS holds
    int table(hipStream_t stream, int n_in, int n_out, bool vertical, const int** dev, int* ks, std::string& err) {
        *dev = nullptr;
        *ks = 0;
        if (n_in == n_out) return 0;
        for (auto& t : tables)
            if (t.n_in == n_in && t.n_out == n_out) { *dev = t.dev.as<int>(); *ks = t.ks; return vertical ? rows_fit(*t.host, n_out, err) : 0; }
        Table t{n_in, n_out, 0, DevBuf{}, std::make_unique<std::vector<int>>()};
        compose_axis_table(n_in, n_out, *t.host, t.ks);
        if (vertical && rows_fit(*t.host, n_out, err)) return -1;
        int rc = upload(stream, t.host->data(), t.host->size() * sizeof(int), t.dev, err);
        if (rc) return rc;
        *dev = t.dev.as<int>();
        *ks = t.ks;
        tables.push_back(std::move(t));
        return 0;
    }
    static int rows_fit(const std::vector<int>& tab, int n_out, std::string& err) {
        for (int i0 = 0; i0 < n_out; i0 += CMP_TH) {
            const int i1 = std::min(n_out, i0 + CMP_TH) - 1;
            if (tab[i1] + tab[(size_t)n_out + i1] - tab[i0] > CMP_ROWS) { err = "avsim_compose: a tile needs more source rows than the kernel holds"; return -1; }
        }
        return 0;
    }
    Call* find(const std::vector<int32_t>& key) {
        for (auto& c : calls)
            if (c.key == key) return &c;
        return nullptr;
    }

    // src, canvas: device pointers; places: host.  -1: an argument the header rules out (err says which), -3: HIP
    int launch(hipStream_t stream, const void* src, int sf, int nsrc, int SH, int SW, void* canvas, int df, int nout, int CH, int CW, const int32_t* places,
               int nplace, int clear, uint32_t clear_rgb, std::string& err) {
        std::vector<int32_t> key{0, sf, nsrc, SH, SW, df, nout, CH, CW, nplace};
        key.insert(key.end(), places, places + (size_t)6 * nplace);
        int rc;
        if ((rc = unit(stream, err))) return rc;
        Call* call = find(key);
        if (!call) {
            if ((rc = validate(nsrc, SH, SW, nout, CH, CW, places, nplace, err))) return rc;
            if (calls.size() >= 64 || tables.size() >= 256) drop(stream);       // (a caller that walks through layouts: start over once nothing reads the old ones)
            auto host = std::make_unique<std::vector<uint8_t>>((size_t)nplace * sizeof(ComposePlace));
            ComposePlace* P = (ComposePlace*)host->data();
            int gx = 1, gy = 1;
            for (int i = 0; i < nplace; i++) {
                const int32_t* p = places + 6 * (size_t)i;
                ComposePlace& q = P[i];
                q.out = p[0]; q.src = p[1]; q.x0 = p[2]; q.y0 = p[3]; q.w = p[4]; q.h = p[5];
                if ((rc = table(stream, SW, q.w, false, &q.htab, &q.hks, err))) return rc;
                if ((rc = table(stream, SH, q.h, true, &q.vtab, &q.vks, err))) return rc;
                gx = std::max(gx, (q.w + CMP_TW - 1) / CMP_TW);
                gy = std::max(gy, (q.h + CMP_TH - 1) / CMP_TH);
            }
            Call c{std::move(key), DevBuf{}, std::move(host), gx, gy};
            if ((rc = upload(stream, c.host->data(), c.host->size(), c.dev, err))) return rc;
            calls.push_back(std::move(c));
            call = &calls.back();
        }
        if (clear) {
            const size_t plane = (size_t)CH * CW, total = (size_t)nout * plane * 3;
            const unsigned blocks = (unsigned)std::min<size_t>((total / (df ? 1 : 4) + 255) / 256 + 1, 16384);
            if (df == 0) hipLaunchKernelGGL(k_compose_fill<0>, dim3(blocks), dim3(256), 0, stream, canvas, total, plane, clear_rgb, d_unit.as<float>());
            else hipLaunchKernelGGL(k_compose_fill<1>, dim3(blocks), dim3(256), 0, stream, canvas, total, plane, clear_rgb, d_unit.as<float>());
        }
        const ComposePlace* dp = call->dev.as<const ComposePlace>();
        for (int p0 = 0; p0 < nplace; p0 += 65535) {
            const dim3 grid(call->gx, call->gy, std::min(65535, nplace - p0));
#define CMP_LAUNCH(S, D) hipLaunchKernelGGL((k_compose<S, D>), grid, dim3(CMP_THREADS), 0, stream, dp, p0, src, SH, SW, canvas, CH, CW, d_unit.as<float>())
            if (sf == 0 && df == 0) CMP_LAUNCH(0, 0);
            else if (sf == 0) CMP_LAUNCH(0, 1);
            else if (df == 0) CMP_LAUNCH(1, 0);
            else CMP_LAUNCH(1, 1);
#undef CMP_LAUNCH
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = std::string("compose kernels: ") + hipGetErrorString(e); return -3; }
        return 0;
    }

    static int validate(int nsrc, int SH, int SW, int nout, int CH, int CW, const int32_t* places, int nplace, std::string& err) {
        char buf[256];
        for (int i = 0; i < nplace; i++) {
            const int32_t* p = places + 6 * (size_t)i;
            const long long o = p[0], s = p[1], x0 = p[2], y0 = p[3], w = p[4], h = p[5];
            const char* what = nullptr;
            if (o < 0 || o >= nout) what = "output image out of range";
            else if (s < 0 || s >= nsrc) what = "source image out of range";
            else if (w < 1 || h < 1 || w > 65535 || h > 65535) what = "rectangle size outside 1..65535";
            else if (x0 < 0 || y0 < 0 || x0 + w > CW || y0 + h > CH) what = "rectangle outside the canvas";
            else if (SW > CMP_MAX_RATIO * w || SH > CMP_MAX_RATIO * h) what = "shrinks by more than 16";
            if (what) {
                snprintf(buf, sizeof buf, "avsim_compose: place %d (%lld %lld %lld %lld %lld %lld): %s", i, o, s, x0, y0, w, h, what);
                err = buf;
                return -1;
            }
        }
        // rectangles of one output image must not overlap (a parallel kernel gives overlaps no order)
        std::vector<int> order((size_t)nplace);
        for (int i = 0; i < nplace; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            const int32_t *p = places + 6 * (size_t)a, *q = places + 6 * (size_t)b;
            return p[0] != q[0] ? p[0] < q[0] : p[3] != q[3] ? p[3] < q[3] : a < b;
        });
        for (int a = 0; a < nplace; a++) {
            const int32_t* p = places + 6 * (size_t)order[a];
            for (int b = a + 1; b < nplace; b++) {
                const int32_t* q = places + 6 * (size_t)order[b];
                if (q[0] != p[0] || q[3] >= p[3] + p[5]) break;          // (sorted by y0 inside an image: nothing further down starts above p's end)
                if (q[2] < p[2] + p[4] && p[2] < q[2] + q[4]) {
                    snprintf(buf, sizeof buf, "avsim_compose: places %d and %d overlap on output image %d", order[a], order[b], (int)p[0]);
                    err = buf;
                    return -1;
                }
            }
        }
        return 0;
    }

    // canvas, value: device pointers; where, prefix: host
    int label(hipStream_t stream, void* canvas, int df, int nout, int CH, int CW, const int32_t* where, int nlabel, const char* prefix, const long long* value,
              uint32_t rgb, std::string& err) {
        const size_t np = prefix ? strnlen(prefix, CMP_PREFIX + 1) : 0;
        if (np > CMP_PREFIX) { err = "avsim_compose_label: the prefix has more than 15 characters"; return -1; }
        std::vector<int32_t> key{1, nout, nlabel};
        key.insert(key.end(), where, where + (size_t)4 * nlabel);
        int rc;
        if ((rc = unit(stream, err))) return rc;
        Call* call = find(key);
        if (!call) {
            for (int i = 0; i < nlabel; i++) {
                const int32_t* w = where + 4 * (size_t)i;
                if (w[0] < 0 || w[0] >= nout || w[3] < 1 || w[3] > CMP_MAX_SCALE || w[1] < -(1 << 20) || w[1] > (1 << 20) || w[2] < -(1 << 20) || w[2] > (1 << 20)) {
                    char buf[200];
                    snprintf(buf, sizeof buf, "avsim_compose_label: label %d (%d %d %d %d): image out of range, scale outside 1..64 or a position beyond 2^20", i, w[0], w[1], w[2], w[3]);
                    err = buf;
                    return -1;
                }
            }
            if (calls.size() >= 64) drop(stream);
            auto host = std::make_unique<std::vector<uint8_t>>((size_t)nlabel * 4 * sizeof(int32_t));
            std::memcpy(host->data(), where, host->size());
            Call c{std::move(key), DevBuf{}, std::move(host), 0, 0};
            if ((rc = upload(stream, c.host->data(), c.host->size(), c.dev, err))) return rc;
            calls.push_back(std::move(c));
            call = &calls.back();
        }
        ComposeText text{};
        if (np) std::memcpy(text.c, prefix, np);
        if (df == 0) hipLaunchKernelGGL(k_compose_label<0>, dim3(nlabel), dim3(256), 0, stream, call->dev.as<const int>(), text, (int)np, value, canvas, CH, CW, rgb, d_unit.as<float>());
        else hipLaunchKernelGGL(k_compose_label<1>, dim3(nlabel), dim3(256), 0, stream, call->dev.as<const int>(), text, (int)np, value, canvas, CH, CW, rgb, d_unit.as<float>());
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = std::string("compose label kernel: ") + hipGetErrorString(e); return -3; }
        return 0;
    }
};

}  // namespace avs

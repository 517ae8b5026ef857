// avsim_imgaug.hip -- the kernels of avsim_image_jitter and avsim_image_augment: brightness, contrast, saturation, hue and sharpness of a decoded u8
// frame, the crop, the mirror and the normalisation in one pass, plus the reduction contrast needs first.  av_aloha_amd/imgaug.py is the
// specification; every float32 operation here is the one it names, rounded on its own.  The unit is built -ffp-contract=off with IEEE
// division and denormals kept (av_aloha_amd/build.py): a * f + b * g is two v_mul and a v_add, x / y the v_div_scale / v_div_fmas /
// v_div_fixup sequence.  u / 255 comes from a 256-entry table that each workgroup fills by that division.  Kernels:
//   k_aug_gray_sum   grid = (slabs, outputs that have the contrast bit).  The source image is a byte stream of 3 H W bytes; its body from the
//                    first address that is both a 16-byte and a pixel boundary is read in units of 48 bytes = 16 pixels per lane (three
//                    16-byte loads); the at most 15 pixels in front of it and the at most 15 behind the last unit go one per lane in the
//                    image's first workgroup.  Per pixel: table, brightness if set, gray, q = (uint32)(gray * 2^20 + 0.5).  q <= 2^20, so a
//                    lane sums 128 units in 32 bits (128 x 16 x 2^20 = 2^31) and widens.  Wave shuffle, LDS across the waves, one 64-bit
//                    integer atomic add per workgroup into the output's slot, which the launcher has zeroed.  Integers: exact, and the same on
//                    every run.
//   k_aug_apply      grid = (tiles across, tiles down, outputs); a workgroup makes a 16 x 64 tile of the output crop, a lane four consecutive
//                    pixels of a row.  m = float(double(S) / double(H W 2^20)) per lane.  Without the sharpness bit a lane reads its 12 source
//                    bytes (the aligned dwords that hold them, none wholly outside the image), runs the pointwise chain and stores.  With it
//                    the workgroup runs the chain once per pixel of the tile's source rectangle grown by one pixel (clipped to the source
//                    image, not to the crop), keeps the three floats per pixel in LDS, and after a barrier every lane sums the eight
//                    neighbours of its pixels in the specification's order.  The mirror, the normalisation and the stores are
//                    k_image_prep's: a 16-byte store per plane where the address allows, single floats where it does not.  The mask is one
//                    per output, so every branch on it is uniform in the workgroup.  Its body is iag_apply_tile, which the two kernels below share.
// The kernels of avsim_image_augment, which adds bit 5, an affine resampling of the whole image between sharpness and the crop:
//   k_aug_apply_list k_aug_apply for a list of outputs: those of a call that have no bit 5, when others have.
//   k_aug_affine<interp, format>  k_aug_apply's grid and tile; a lane makes four consecutive output pixels: the source position of each by
//                    the specification's float32 steps, one tap (nearest) or four (bilinear), each tested against the image in float before an
//                    index exists.  Format 0, outputs without sharpness: a tap is three bytes of the u8 image through the table and the
//                    pointwise chain -- the chain commutes with the gather, and the contrast mean is k_aug_gray_sum's, the pre-affine image's.
//                    Format 1, outputs with sharpness: a tap is three floats of the image k_aug_whole made.  A tap outside is 0.
//   k_aug_whole      iag_apply_tile over the whole source image of an output that has sharpness and bit 5 -- no box, no mirror, no
//                    normalisation -- into one of the float scratch images of ImgAugHost.
#include "avsim_imgaug.hip.h"

#include <algorithm>

namespace avs {

constexpr int IAG_UNIT = 48;           // bytes a lane of k_aug_gray_sum reads per step: 16 pixels, three 16-byte loads
constexpr int IAG_FLUSH = 128;         // units a lane sums in 32 bits
constexpr int IAG_MAX_SLABS = 1024;    // workgroups per image
constexpr int IAG_SROW = IAG_TX + 2;   // floats per row of the LDS tile: the tile and its halo
constexpr int IAG_SPLANE = (IAG_TY + 2) * IAG_SROW;

__device__ __forceinline__ float iag_clamp(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
__device__ __forceinline__ float iag_gray(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }
__device__ __forceinline__ float iag_pick(int k, float a, float b, float c, float d) { return k == 0 ? a : k == 1 ? b : k == 2 ? c : d; }

// what the pointwise ops of an output need: the factors, 1 - factor, and contrast's m * (1 - fc)
struct AugPoint {
    int mask;
    float fb, fc, mterm, fs, gs, fh;
};

__device__ __forceinline__ void iag_hue(float fh, float& r, float& g, float& b) {
    // torchvision's _rgb_to_hsv
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const float cr = maxc - minc;
    const float s = cr / (maxc == minc ? 1.0f : maxc);
    const float crd = cr == 0.0f ? 1.0f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    float h = maxc == r ? bc - gc : (maxc == g ? (2.0f + rc) - bc : (4.0f + gc) - rc);
    h = h / 6.0f + 1.0f;
    h = h - floorf(h);
    h = h + fh;
    h = h - floorf(h);
    // _hsv_to_rgb
    const float v = maxc, h6 = h * 6.0f, fl = floorf(h6), f = h6 - fl;
    int i = (int)fl;                    // 0 <= h <= 1: 0..6
    i = i >= 6 ? i - 6 : i;
    const float p = iag_clamp(v * (1.0f - s)), q = iag_clamp(v * (1.0f - s * f)), t = iag_clamp(v * (1.0f - s * (1.0f - f)));
    r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
    g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// brightness, contrast, saturation and hue of one pixel
__device__ __forceinline__ void iag_point(const AugPoint& P, float& r, float& g, float& b) {
    if (P.mask & IAG_BRIGHTNESS) { r = iag_clamp(r * P.fb); g = iag_clamp(g * P.fb); b = iag_clamp(b * P.fb); }      // (+ 0 * (1 - fb): nothing)
    if (P.mask & IAG_CONTRAST) { r = iag_clamp(r * P.fc + P.mterm); g = iag_clamp(g * P.fc + P.mterm); b = iag_clamp(b * P.fc + P.mterm); }
    if (P.mask & IAG_SATURATION) {
        const float t = iag_gray(r, g, b) * P.gs;
        r = iag_clamp(r * P.fs + t); g = iag_clamp(g * P.fs + t); b = iag_clamp(b * P.fs + t);
    }
    if (P.mask & IAG_HUE) iag_hue(P.fh, r, g, b);
}

// the u8 values of npx (1..4) consecutive pixels from pixel `pix` of the image at `img`: the aligned dwords that hold the 3 npx bytes (each
// holds at least one of them, so none lies wholly outside the image), shifted so that byte 0 is the first
__device__ __forceinline__ void iag_load4(const uint8_t* img, size_t pix, int npx, uint32_t u[3][4]) {
    const uintptr_t a = (uintptr_t)(img + pix * 3);
    const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
    const int sh = (int)(a & 3), nd = (sh + 3 * npx + 3) >> 2;
    const uint32_t w0 = q[0], w1 = nd > 1 ? q[1] : 0u, w2 = nd > 2 ? q[2] : 0u, w3 = nd > 3 ? q[3] : 0u;
    const uint32_t d[3] = {(uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * sh)), (uint32_t)((((uint64_t)w2 << 32) | w1) >> (8 * sh)),
                           (uint32_t)((((uint64_t)w3 << 32) | w2) >> (8 * sh))};
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) u[c][k] = (d[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255u;
}

// grid = (slabs, contrast outputs of this launch); gsum: one slot per output, zeroed
__global__ void __launch_bounds__(IAG_THREADS) k_aug_gray_sum(const uint8_t* __restrict__ src, size_t HW, const AugItem* __restrict__ items,
                                                              const int* __restrict__ cidx, int c0, unsigned long long* __restrict__ gsum) {
    __shared__ float s_tab[256];
    __shared__ unsigned long long s_red[IAG_THREADS / 64];
    const int tid = threadIdx.x;
    const int i = cidx[c0 + blockIdx.y];
    const AugItem P = items[i];
    const bool bright = (P.fm >> 1) & IAG_BRIGHTNESS;
    const float fb = P.f[0];
    s_tab[tid] = (float)tid / 255.0f;
    __syncthreads();
    const size_t L = 3 * HW;
    const uint8_t* p = src + (size_t)P.src * L;
    // head: the bytes in front of the first address that is a 16-byte boundary and a pixel's first byte (to16 + 16 k with k = -to16 mod 3)
    const size_t to16 = (size_t)((0 - (uintptr_t)p) & 15);
    const size_t h48 = to16 + 16 * ((3 - to16 % 3) % 3);
    const size_t head = h48 < L ? h48 : L;
    const size_t nu = (L - head) / IAG_UNIT;
    const size_t tail0 = head + nu * IAG_UNIT;
    unsigned long long s64 = 0;
    auto pixel = [&](uint32_t ur, uint32_t ug, uint32_t ub) -> uint32_t {
        float r = s_tab[ur], g = s_tab[ug], b = s_tab[ub];
        if (bright) { r = iag_clamp(r * fb); g = iag_clamp(g * fb); b = iag_clamp(b * fb); }
        return (uint32_t)(iag_gray(r, g, b) * 1048576.0f + 0.5f);
    };
    const uint4* base = (const uint4*)(p + head);
    const size_t stride = (size_t)gridDim.x * IAG_THREADS;
    size_t u = (size_t)blockIdx.x * IAG_THREADS + tid;
    while (u < nu) {
        uint32_t s32 = 0;
        for (int n = 0; n < IAG_FLUSH && u < nu; n++, u += stride) {
            const uint4* q = base + 3 * u;
            const uint4 a = q[0], b = q[1], c = q[2];
            const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int j = 3 * k;
                s32 += pixel((w[j >> 2] >> (8 * (j & 3))) & 255u, (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u, (w[(j + 2) >> 2] >> (8 * ((j + 2) & 3))) & 255u);
            }
        }
        s64 += s32;
    }
    if (blockIdx.x == 0) {
        const size_t nh = head / 3, nt = (L - tail0) / 3;      // at most 15 each
        if ((size_t)tid < nh + nt) {
            const size_t o = (size_t)tid < nh ? 3 * (size_t)tid : tail0 + 3 * ((size_t)tid - nh);
            s64 += pixel(p[o], p[o + 1], p[o + 2]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s64 += __shfl_xor(s64, off);
    if ((tid & 63) == 0) s_red[tid >> 6] = s64;
    __syncthreads();
    if (tid == 0) {
        unsigned long long v = s_red[0];
        for (int w = 1; w < IAG_THREADS / 64; w++) v += s_red[w];
        atomicAdd(gsum + i, v);
    }
}

// k_aug_apply's workgroup: the tile (blockIdx.x, blockIdx.y) of the output P, whose gray sum is *gs, into the image at oimg (three planes
// of oh x ow).  ms: mean[3], std[3]
__device__ __forceinline__ void iag_apply_tile(const uint8_t* __restrict__ src, int SH, int SW, const AugItem& P, const unsigned long long* __restrict__ gs,
                                               const float* __restrict__ ms, int normalise, int oh, int ow, float* __restrict__ oimg) {
    __shared__ float s_tab[256];
    __shared__ float s_x[3 * IAG_SPLANE];
    const int tid = threadIdx.x;
    const int flip = P.fm & 1;
    AugPoint A;
    A.mask = P.fm >> 1;
    A.fb = P.f[0]; A.fc = P.f[1]; A.fs = P.f[2]; A.fh = P.f[3];
    A.gs = 1.0f - A.fs;
    A.mterm = 0.0f;
    if (A.mask & IAG_CONTRAST) {
        const float m = (float)((double)*gs / (double)((unsigned long long)SH * (unsigned long long)SW * 1048576ull));
        A.mterm = m * (1.0f - A.fc);
    }
    const float fsh = P.f[4], gsh = 1.0f - fsh;
    s_tab[tid] = (float)tid / 255.0f;
    __syncthreads();
    const uint8_t* img = src + (size_t)P.src * SH * SW * 3;
    // the tile in output coordinates and its source rectangle [cx, cx + tw) x [cy, cy + th)
    const int tx0 = blockIdx.x * IAG_TX, ty0 = blockIdx.y * IAG_TY;
    const int tw = min(IAG_TX, ow - tx0), th = min(IAG_TY, oh - ty0);
    const int cx = P.x0 + (flip ? ow - tx0 - tw : tx0), cy = P.y0 + ty0;
    const int ly = tid >> 4, lx = (tid & 15) * 4;
    const bool mine = ly < th && lx < tw;
    const int npx = mine ? min(4, tw - lx) : 0;
    const int sy = cy + ly, sx = cx + (flip ? tw - lx - npx : lx);      // the lane's npx source pixels, left to right
    float v[3][4];
    if (A.mask & IAG_SHARPNESS) {
        // the chain once per pixel of the rectangle grown by one, inside the source image
        const int rx0 = cx - 1, ry0 = cy - 1;
        const int c_lo = max(rx0, 0), c_hi = min(cx + tw + 1, SW), r_lo = max(ry0, 0), r_hi = min(cy + th + 1, SH);
        const int G = (c_hi - c_lo + 3) >> 2;
        for (int it = tid; it < (r_hi - r_lo) * G; it += IAG_THREADS) {
            const int ry = r_lo + it / G, gx = c_lo + (it % G) * 4, n = min(4, c_hi - gx);
            uint32_t u[3][4];
            iag_load4(img, (size_t)ry * SW + gx, n, u);
            float* row = s_x + (ry - ry0) * IAG_SROW + (gx - rx0);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float r = s_tab[u[0][k]], g = s_tab[u[1][k]], b = s_tab[u[2][k]];
                iag_point(A, r, g, b);
                if (k < n) { row[k] = r; row[IAG_SPLANE + k] = g; row[2 * IAG_SPLANE + k] = b; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k >= npx) continue;
            const int X = sx + k;
            const float* q = s_x + (sy - ry0) * IAG_SROW + (X - rx0);
            const bool inner = sy > 0 && sy < SH - 1 && X > 0 && X < SW - 1;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* e = q + c * IAG_SPLANE;
                const float x = e[0];
                float y = x;
                if (inner) {
                    float t = e[-IAG_SROW - 1] + e[-IAG_SROW];
                    t = t + e[-IAG_SROW + 1];
                    t = t + e[-1];
                    t = t + e[1];
                    t = t + e[IAG_SROW - 1];
                    t = t + e[IAG_SROW];
                    t = t + e[IAG_SROW + 1];
                    const float blur = (t + 5.0f * x) / 13.0f;
                    y = iag_clamp(x * fsh + blur * gsh);
                }
                v[c][k] = y;
            }
        }
    } else if (mine) {
        uint32_t u[3][4];
        iag_load4(img, (size_t)sy * SW + sx, npx, u);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float r = s_tab[u[0][k]], g = s_tab[u[1][k]], b = s_tab[u[2][k]];
            iag_point(A, r, g, b);
            v[0][k] = r; v[1][k] = g; v[2][k] = b;
        }
    }
    if (!mine) return;
    const size_t plane = (size_t)oh * ow;
    float* o = oimg + (size_t)(ty0 + ly) * ow + (tx0 + lx);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v0 = v[c][0], v1 = v[c][1], v2 = v[c][2], v3 = v[c][3];
        if (normalise) {
            const float mean = ms[c], sd = ms[3 + c];
            v0 = (v0 - mean) / sd; v1 = (v1 - mean) / sd; v2 = (v2 - mean) / sd; v3 = (v3 - mean) / sd;
        }
        float* dst = o + c * plane;
        if (npx == 4 && ((uintptr_t)dst & 15) == 0) {
            *(float4*)dst = flip ? make_float4(v3, v2, v1, v0) : make_float4(v0, v1, v2, v3);
        } else {
            for (int j = 0; j < npx; j++) dst[j] = iag_pick(flip ? npx - 1 - j : j, v0, v1, v2, v3);
        }
    }
}

// grid = (tiles across, tiles down, outputs of this launch); ms: mean[3], std[3]; out: float32 [nout][3][oh][ow]
__global__ void __launch_bounds__(IAG_THREADS) k_aug_apply(const uint8_t* __restrict__ src, int SH, int SW, const AugItem* __restrict__ items, int item0,
                                                           const float* __restrict__ ms, int normalise, int oh, int ow,
                                                           const unsigned long long* __restrict__ gsum, float* __restrict__ out) {
    const int i = item0 + blockIdx.z;
    const AugItem P = items[i];
    iag_apply_tile(src, SH, SW, P, gsum + i, ms, normalise, oh, ow, out + (size_t)i * 3 * ((size_t)oh * ow));
}

// k_aug_apply for the outputs list[l0 + blockIdx.z]: those of an avsim_image_augment call that have no bit 5, when others have
__global__ void __launch_bounds__(IAG_THREADS) k_aug_apply_list(const uint8_t* __restrict__ src, int SH, int SW, const AugItem* __restrict__ items,
                                                                const int* __restrict__ list, int l0, const float* __restrict__ ms, int normalise, int oh, int ow,
                                                                const unsigned long long* __restrict__ gsum, float* __restrict__ out) {
    const int i = list[l0 + blockIdx.z];
    const AugItem P = items[i];
    iag_apply_tile(src, SH, SW, P, gsum + i, ms, normalise, oh, ow, out + (size_t)i * 3 * ((size_t)oh * ow));
}

// The colour ops and sharpness of the outputs list[l0 + blockIdx.z] over their WHOLE source images -- no box, no mirror, no normalisation --
// into scratch: float32 [gridDim.z][3][SH][SW], which k_aug_affine<., 1> then gathers from.  grid = (tiles of the source, ., outputs of the group)
__global__ void __launch_bounds__(IAG_THREADS) k_aug_whole(const uint8_t* __restrict__ src, int SH, int SW, const AugItem* __restrict__ items,
                                                           const int* __restrict__ list, int l0, const unsigned long long* __restrict__ gsum,
                                                           float* __restrict__ scratch) {
    const int i = list[l0 + blockIdx.z];
    AugItem P = items[i];
    P.x0 = 0; P.y0 = 0; P.fm &= ~1;
    iag_apply_tile(src, SH, SW, P, gsum + i, nullptr, 0, SH, SW, scratch + (size_t)blockIdx.z * 3 * ((size_t)SH * SW));
}

// One tap of the gather.  FMT 0: the u8 source pixel through the table and the pointwise chain; FMT 1: the three planes of a float image
template <int FMT>
__device__ __forceinline__ void iag_tap(const void* __restrict__ img, size_t HW, int SW, const float* s_tab, const AugPoint& A, float xi, float yi, float wlim, float hlim,
                                        float& r, float& g, float& b) {
    r = g = b = 0.0f;
    if (xi >= 0.0f && xi <= wlim && yi >= 0.0f && yi <= hlim) {      // on the floats: no address is formed for a tap outside (or a NaN)
        const size_t pix = (size_t)(int)yi * SW + (size_t)(int)xi;
        if (FMT == 0) {
            const uint8_t* q = (const uint8_t*)img + pix * 3;
            r = s_tab[q[0]]; g = s_tab[q[1]]; b = s_tab[q[2]];
            iag_point(A, r, g, b);
        } else {
            const float* q = (const float*)img + pix;
            r = q[0]; g = q[HW]; b = q[2 * HW];
        }
    }
}

// grid = (tiles across, tiles down, outputs of this launch), k_aug_apply's tiles: the outputs list[l0 + blockIdx.z], which have bit 5.
// FMT 0: src = the u8 images, the pointwise chain runs per tap (it commutes with the gather; the contrast mean is the pre-affine image's);
// FMT 1: src = k_aug_whole's scratch, image blockIdx.z.  mats: float32 [nout][6]
template <int INTERP, int FMT>
__global__ void __launch_bounds__(IAG_THREADS) k_aug_affine(const void* __restrict__ src, int SH, int SW, const AugItem* __restrict__ items, const float* __restrict__ mats,
                                                            const int* __restrict__ list, int l0, const float* __restrict__ ms, int normalise, int oh, int ow,
                                                            const unsigned long long* __restrict__ gsum, float* __restrict__ out) {
    __shared__ float s_tab[256];
    const int tid = threadIdx.x;
    const int i = list[l0 + blockIdx.z];
    const AugItem P = items[i];
    const int flip = P.fm & 1;
    const size_t HW = (size_t)SH * SW;
    AugPoint A;
    A.mask = 0;
    const void* img;
    if (FMT == 0) {
        A.mask = P.fm >> 1;
        A.fb = P.f[0]; A.fc = P.f[1]; A.fs = P.f[2]; A.fh = P.f[3];
        A.gs = 1.0f - A.fs;
        A.mterm = 0.0f;
        if (A.mask & IAG_CONTRAST) {
            const float m = (float)((double)gsum[i] / (double)((unsigned long long)SH * (unsigned long long)SW * 1048576ull));
            A.mterm = m * (1.0f - A.fc);
        }
        s_tab[tid] = (float)tid / 255.0f;
        __syncthreads();
        img = (const uint8_t*)src + (size_t)P.src * HW * 3;
    } else {
        img = (const float*)src + (size_t)blockIdx.z * 3 * HW;
    }
    const float* M = mats + 6 * (size_t)i;
    const float m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5];
    const int tx0 = blockIdx.x * IAG_TX, ty0 = blockIdx.y * IAG_TY;
    const int ly = tid >> 4, lx = (tid & 15) * 4;
    const int oy = ty0 + ly, ox = tx0 + lx;
    if (oy >= oh || ox >= ow) return;
    const int npx = min(4, ow - ox);
    const float halfw = (float)SW / 2.0f, halfh = (float)SH / 2.0f;
    const float backx = halfw - 0.5f, backy = halfh - 0.5f;
    const float wlim = (float)(SW - 1), hlim = (float)(SH - 1);
    const float yf = ((float)(P.y0 + oy) + 0.5f) - halfh;
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[0][k] = v[1][k] = v[2][k] = 0.0f;
        if (k >= npx) continue;
        const int X = P.x0 + (flip ? ow - 1 - (ox + k) : ox + k);      // the pixel of the whole image behind output column ox + k
        const float xf = ((float)X + 0.5f) - halfw;
        const float sx = (((m0 * xf) + (m1 * yf)) + m2) + backx;
        const float sy = (((m3 * xf) + (m4 * yf)) + m5) + backy;
        if (INTERP == 0) {
            iag_tap<FMT>(img, HW, SW, s_tab, A, rintf(sx), rintf(sy), wlim, hlim, v[0][k], v[1][k], v[2][k]);
        } else {
            const float x0 = floorf(sx), y0 = floorf(sy);
            const float wx = sx - x0, wy = sy - y0, ux = 1.0f - wx, uy = 1.0f - wy;
            const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
            float a[3], b[3], c[3], d[3];
            iag_tap<FMT>(img, HW, SW, s_tab, A, x0, y0, wlim, hlim, a[0], a[1], a[2]);
            iag_tap<FMT>(img, HW, SW, s_tab, A, x1, y0, wlim, hlim, b[0], b[1], b[2]);
            iag_tap<FMT>(img, HW, SW, s_tab, A, x0, y1, wlim, hlim, c[0], c[1], c[2]);
            iag_tap<FMT>(img, HW, SW, s_tab, A, x1, y1, wlim, hlim, d[0], d[1], d[2]);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const float top = a[ch] * ux + b[ch] * wx, bot = c[ch] * ux + d[ch] * wx;
                v[ch][k] = top * uy + bot * wy;
            }
        }
    }
    const size_t plane = (size_t)oh * ow;
    float* o = out + (size_t)i * 3 * plane + (size_t)oy * ow + ox;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v0 = v[c][0], v1 = v[c][1], v2 = v[c][2], v3 = v[c][3];
        if (normalise) {
            const float mean = ms[c], sd = ms[3 + c];
            v0 = (v0 - mean) / sd; v1 = (v1 - mean) / sd; v2 = (v2 - mean) / sd; v3 = (v3 - mean) / sd;
        }
        float* dst = o + c * plane;
        if (npx == 4 && ((uintptr_t)dst & 15) == 0) {
            *(float4*)dst = make_float4(v0, v1, v2, v3);
        } else {
            for (int j = 0; j < npx; j++) dst[j] = iag_pick(j, v0, v1, v2, v3);
        }
    }
}

// zeroes gsum and runs k_aug_gray_sum for the ncon outputs of cidx
static void iag_sums(hipStream_t stream, const void* src, size_t HW, const AugItem* items, const int* cidx, int nout, int ncon, unsigned long long* gsum, hipError_t& e) {
    e = hipMemsetAsync(gsum, 0, sizeof(unsigned long long) * (size_t)nout, stream);
    if (e != hipSuccess) return;
    // a slab: some eight units of 16 pixels per lane
    const size_t units = 3 * HW / IAG_UNIT;
    const int slabs = (int)std::min<size_t>(IAG_MAX_SLABS, std::max<size_t>(1, (units + 8 * IAG_THREADS - 1) / (8 * IAG_THREADS)));
    for (int c0 = 0; c0 < ncon; c0 += 65535)
        hipLaunchKernelGGL(k_aug_gray_sum, dim3(slabs, std::min(65535, ncon - c0)), dim3(IAG_THREADS), 0, stream, (const uint8_t*)src, HW, items, cidx, c0, gsum);
}

template <int FMT>
static void iag_launch_affine(hipStream_t stream, int interp, dim3 grid, const void* src, int SH, int SW, const AugItem* items, const float* mats, const int* list, int l0,
                              const float* ms, int normalise, int oh, int ow, const unsigned long long* gsum, float* out) {
    if (interp == 0)
        hipLaunchKernelGGL((k_aug_affine<0, FMT>), grid, dim3(IAG_THREADS), 0, stream, src, SH, SW, items, mats, list, l0, ms, normalise, oh, ow, gsum, out);
    else
        hipLaunchKernelGGL((k_aug_affine<1, FMT>), grid, dim3(IAG_THREADS), 0, stream, src, SH, SW, items, mats, list, l0, ms, normalise, oh, ow, gsum, out);
}

int imgaug_launch_affine(hipStream_t stream, const void* src, int SH, int SW, const void* stage, int nout, int ncon, const int count[3], int interp, bool normalise,
                         int oh, int ow, unsigned long long* gsum, float* scratch, int group, float* out, std::string& err) {
    const AugItem* items = (const AugItem*)stage;
    const int* cidx = (const int*)(items + nout);
    const float* ms = (const float*)(cidx + nout);
    const float* mats = ms + 8;
    const int* plain = (const int*)(mats + 6 * (size_t)nout);
    const int *gather = plain + nout, *sharp = gather + nout;
    const size_t HW = (size_t)SH * SW;
    const int norm = normalise ? 1 : 0;
    hipError_t e = hipSuccess;
    if (ncon > 0) {
        iag_sums(stream, src, HW, items, cidx, nout, ncon, gsum, e);
        if (e != hipSuccess) { err = std::string("image augment sums: ") + hipGetErrorString(e); return -3; }
    }
    const dim3 tiles((ow + IAG_TX - 1) / IAG_TX, (oh + IAG_TY - 1) / IAG_TY), whole((SW + IAG_TX - 1) / IAG_TX, (SH + IAG_TY - 1) / IAG_TY);
    for (int l0 = 0; l0 < count[0]; l0 += 65535)
        hipLaunchKernelGGL(k_aug_apply_list, dim3(tiles.x, tiles.y, std::min(65535, count[0] - l0)), dim3(IAG_THREADS), 0, stream, (const uint8_t*)src, SH, SW, items, plain, l0,
                           ms, norm, oh, ow, gsum, out);
    for (int l0 = 0; l0 < count[1]; l0 += 65535)
        iag_launch_affine<0>(stream, interp, dim3(tiles.x, tiles.y, std::min(65535, count[1] - l0)), src, SH, SW, items, mats, gather, l0, ms, norm, oh, ow, gsum, out);
    // the outputs with sharpness and bit 5, `group` at a time through the scratch images: the stream orders a group's gather before the next group's fill
    for (int l0 = 0; l0 < count[2]; l0 += group) {
        const int n = std::min(group, count[2] - l0);
        hipLaunchKernelGGL(k_aug_whole, dim3(whole.x, whole.y, n), dim3(IAG_THREADS), 0, stream, (const uint8_t*)src, SH, SW, items, sharp, l0, gsum, scratch);
        iag_launch_affine<1>(stream, interp, dim3(tiles.x, tiles.y, n), scratch, SH, SW, items, mats, sharp, l0, ms, norm, oh, ow, gsum, out);
    }
    e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("image augment kernels: ") + hipGetErrorString(e); return -3; }
    return 0;
}

int imgaug_launch(hipStream_t stream, const void* src, int SH, int SW, const void* stage, int nout, int ncon, bool normalise, int oh, int ow,
                  unsigned long long* gsum, float* out, std::string& err) {
    const AugItem* items = (const AugItem*)stage;
    const int* cidx = (const int*)(items + nout);
    const float* ms = (const float*)(cidx + nout);
    const size_t HW = (size_t)SH * SW;
    hipError_t e = hipSuccess;
    if (ncon > 0) {
        iag_sums(stream, src, HW, items, cidx, nout, ncon, gsum, e);
        if (e != hipSuccess) { err = std::string("image jitter sums: ") + hipGetErrorString(e); return -3; }
    }
    const dim3 tiles((ow + IAG_TX - 1) / IAG_TX, (oh + IAG_TY - 1) / IAG_TY);
    for (int i0 = 0; i0 < nout; i0 += 65535)
        hipLaunchKernelGGL(k_aug_apply, dim3(tiles.x, tiles.y, std::min(65535, nout - i0)), dim3(IAG_THREADS), 0, stream, (const uint8_t*)src, SH, SW, items, i0, ms,
                           normalise ? 1 : 0, oh, ow, gsum, out);
    e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("image jitter kernels: ") + hipGetErrorString(e); return -3; }
    return 0;
}

}  // namespace avs

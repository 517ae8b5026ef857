// avsim_imgresize.hip -- the kernels of avsim_image_resize: a region of a decoded u8 frame (or of a float image) resized by the
// separable triangle filter of interpolate(mode="bilinear", antialias=...) into a rectangle of a padded output, mirrored and normalised, in
// one launch and without an intermediate image in global memory.  av_aloha_amd/imgresize.py is the specification; every float32 operation
// here is the one it names, rounded on its own.  The unit is built -ffp-contract=off with IEEE division and denormals kept
// (av_aloha_amd/build.py): v * w + acc is a v_mul and a v_add, x / y the v_div_scale / v_div_fmas / v_div_fixup sequence.
//
//   k_resize<class, format>   grid = (tiles across, tiles down, outputs of the class); a workgroup of 256 makes a TY x TX tile of the WHOLE
//       output, fill included.
//       1. Taps.  Lane t < TX computes the taps of tile column t (of the resized column rw - 1 - x when the output is mirrored), lane
//          64 + r those of tile row r, by the specification's float32 steps, into LDS: first input, count, `count` weights.  Columns and
//          rows outside the dst rectangle have count 0.  LDS integer min / max give the tile's source footprint.
//       2. The footprint's rows that some tile row reads are listed (without antialias and a ratio above 2 most are not read at all).
//       3. Horizontal pass, a band of BAND listed rows at a time for the u8 format: the band's bytes [xmin, xmax) are read -- the
//          aligned dwords that lie wholly inside that range by 4-byte loads, the at most 3 bytes in front and behind them by byte loads --
//          and staged into LDS as floats through the workgroup's table of u / 255, once per source value; then an item (row, channel) of a
//          lane's column sums its taps, one LDS read each, into the float array s_h[row][channel][column].  A lane keeps its column for
//          the whole pass (256 is a multiple of TX), so with up to 11 taps its weights are read from LDS once, into registers.  The float
//          format reads its taps from global memory as they lie.
//       4. Vertical pass: an item (row, channel, column) of the tile sums its taps down s_h (consecutive lanes, consecutive columns: no
//          bank conflict), or takes the fill value, normalises and stores -- consecutive lanes, consecutive floats of an output row.
//       Tile shape and LDS per class (IrsShape): the rows s_h can hold, HR = (TY + 1) S + 2, bound the footprint of TY rows at ratio
//       S: hi(last) - lo(first) <= (TY - 1) S + 2 S + 1, and one more for the roundings; FC, the staged columns, likewise.
#include "avsim_imgresize.hip.h"

#include <algorithm>
#include <climits>

namespace avs {

template <int CLS> struct IrsShape;
// S: the class's largest ratio, K: its taps, TX x TY: the tile, BAND: footprint rows staged at a time (u8 format)
template <> struct IrsShape<0> { static constexpr int S = 2, K = 5, TX = 64, TY = 16, BAND = 4; };       // ratio <= 2 (and every upscale)
template <> struct IrsShape<1> { static constexpr int S = 5, K = 11, TX = 32, TY = 8, BAND = 8; };       // ratio <= 5
template <> struct IrsShape<2> { static constexpr int S = 16, K = 33, TX = 32, TY = 4, BAND = 2; };      // ratio <= 16
constexpr int IRS_KREG = 11;           // up to this many taps a lane keeps its column's weights in registers

// the taps of output index i of an n_in -> n_out resize (imgresize.py, resize_taps): first input, count (<= kmax), weights into w
__device__ __forceinline__ void irs_taps(int i, int n_in, int n_out, int antialias, int kmax, int& lo, int& cnt, float* w) {
    const float scale = (float)n_in / (float)n_out;
    float support = 1.0f, inv = 1.0f;
    if (antialias && scale >= 1.0f) { support = scale; inv = 1.0f / scale; }
    const float center = scale * ((float)i + 0.5f);
    lo = max(0, (int)((center - support) + 0.5f));
    const int hi = min(n_in, (int)((center + support) + 0.5f));
    cnt = min(max(hi - lo, 0), kmax);
    float tot = 0.0f;
    for (int k = 0; k < cnt; k++) {
        const float r = fmaxf(0.0f, 1.0f - fabsf((((float)(lo + k) - center) + 0.5f) * inv));
        w[k] = r;
        tot = tot + r;
    }
    for (int k = 0; k < cnt; k++) w[k] = w[k] / tot;
}

template <int CLS, int FMT>
__global__ void __launch_bounds__(IRS_THREADS) k_resize(const void* __restrict__ src, int SH, int SW, const ResizeItem* __restrict__ items, const int* __restrict__ list,
                                                        int l0, const float* __restrict__ par, int antialias, int normalise, int oh, int ow, float* __restrict__ out) {
    using P = IrsShape<CLS>;
    constexpr int K = P::K, TX = P::TX, TY = P::TY, IRS_BAND = P::BAND;
    constexpr int HR = (TY + 1) * P::S + 2, FC = (TX + 1) * P::S + 2;
    constexpr int ROWF = FC * 3, ROWD = (ROWF + 3 + 3) / 4;          // floats of a staged row; the aligned dwords that can hold its bytes
    static_assert(TX <= 64 && TY <= 64 && HR <= IRS_THREADS && IRS_THREADS % TX == 0, "the set-up lanes; a lane keeps its column");
    __shared__ float s_tab[FMT == 0 ? 256 : 1];
    __shared__ float s_wx[TX * K], s_wy[TY * K];
    __shared__ int s_lox[TX], s_cntx[TX], s_loy[TY], s_cnty[TY];
    __shared__ int s_pos[HR], s_row[HR];
    __shared__ int s_rng[4], s_nrow;
    __shared__ float s_h[HR * 3 * TX];
    __shared__ float s_stage[FMT == 0 ? IRS_BAND * ROWF : 1];
    const int tid = threadIdx.x;
    const int i = list[l0 + blockIdx.z];
    const ResizeItem it = items[i];
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    if (FMT == 0) s_tab[tid] = (float)tid / 255.0f;
    if (tid < 4) s_rng[tid] = (tid & 1) ? -1 : INT_MAX;          // xmin, xmax, ymin, ymax
    if (tid < HR) s_pos[tid] = -1;
    __syncthreads();
    if (tid < TX) {
        const int xr = tx0 + tid - it.ox;
        int lo = 0, cnt = 0;
        if (xr >= 0 && xr < it.rw) {
            irs_taps(it.flip ? it.rw - 1 - xr : xr, it.w, it.rw, antialias, K, lo, cnt, s_wx + tid * K);
            atomicMin(&s_rng[0], lo);
            atomicMax(&s_rng[1], lo + cnt);
        }
        s_lox[tid] = lo;
        s_cntx[tid] = cnt;
    } else if (tid >= 64 && tid < 64 + TY) {
        const int r = tid - 64, yr = ty0 + r - it.oy;
        int lo = 0, cnt = 0;
        if (yr >= 0 && yr < it.rh) {
            irs_taps(yr, it.h, it.rh, antialias, K, lo, cnt, s_wy + r * K);
            atomicMin(&s_rng[2], lo);
            atomicMax(&s_rng[3], lo + cnt);
        }
        s_loy[r] = lo;
        s_cnty[r] = cnt;
    }
    __syncthreads();
    const int xmin = s_rng[0], xmax = s_rng[1], ymin = s_rng[2], ymax = s_rng[3];
    const bool any = xmax > xmin && ymax > ymin;          // the tile meets the dst rectangle (the same for every lane)
    if (any) {
        if (tid < TY)
            for (int k = 0; k < s_cnty[tid]; k++) {
                const int r = s_loy[tid] + k - ymin;
                if (r < HR) s_pos[r] = 0;
            }
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            const int nr = min(ymax - ymin, HR);
            for (int r = 0; r < nr; r++)
                if (s_pos[r] == 0) { s_row[n] = r; s_pos[r] = n++; }
            s_nrow = n;
        }
        __syncthreads();
        const int nrow = s_nrow;
        // a lane's column is the same in every item of the horizontal pass: its taps live in registers
        const int j = tid % TX, cnt = s_cntx[j], lox = s_lox[j];
        const float* wl = s_wx + j * K;
        float w[K <= IRS_KREG ? K : 1];
        if constexpr (K <= IRS_KREG) {
#pragma unroll
            for (int k = 0; k < K; k++) w[k] = k < cnt ? wl[k] : 0.0f;
        }
        if (FMT == 0) {
            const uint8_t* img = (const uint8_t*)src + (size_t)it.src * SH * SW * 3;
            const int nbytes = min(xmax - xmin, FC) * 3;
            for (int b0 = 0; b0 < nrow; b0 += IRS_BAND) {
                const int nb = min(IRS_BAND, nrow - b0);
                for (int idx = tid; idx < nb * ROWD; idx += IRS_THREADS) {
                    const int r = idx / ROWD, d = idx - r * ROWD;
                    const uint8_t* p = img + ((size_t)(it.y0 + ymin + s_row[b0 + r]) * SW + (size_t)(it.x0 + xmin)) * 3;          // the row's first byte
                    const int sh = (int)((uintptr_t)p & 3);
                    // byte b of the row's aligned dwords is the byte p - sh + b; bytes [sh, sh + nbytes) are wanted
                    const int b = 4 * d;
                    if (b >= sh + nbytes || b + 4 <= sh) continue;
                    const uint8_t* q = p - sh + b;
                    uint32_t v = 0;
                    if (b >= sh && b + 4 <= sh + nbytes) {
                        v = *(const uint32_t*)q;
                    } else {
                        for (int t = 0; t < 4; t++)
                            if (b + t >= sh && b + t < sh + nbytes) v |= (uint32_t)q[t] << (8 * t);
                    }
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int f = b + t - sh;          // the value's place in the row: 3 (x - xmin) + channel
                        if (f >= 0 && f < nbytes) s_stage[r * ROWF + f] = s_tab[(v >> (8 * t)) & 255u];
                    }
                }
                __syncthreads();
                if (cnt > 0)
                    for (int rc = tid / TX; rc < nb * 3; rc += IRS_THREADS / TX) {
                        const int r = rc / 3, c = rc - 3 * r;
                        const float* sf = s_stage + r * ROWF + (lox - xmin) * 3 + c;
                        float acc = 0.0f;
                        if constexpr (K <= IRS_KREG) {
#pragma unroll
                            for (int k = 0; k < K; k++) {
                                if (k >= cnt) break;
                                acc = acc + sf[3 * k] * w[k];
                            }
                        } else {
                            for (int k = 0; k < cnt; k++) acc = acc + sf[3 * k] * wl[k];
                        }
                        s_h[((b0 + r) * 3 + c) * TX + j] = acc;
                    }
                __syncthreads();
            }
        } else {
            const float* img = (const float*)src + (size_t)it.src * 3 * SH * SW;
            if (cnt > 0)
                for (int rc = tid / TX; rc < nrow * 3; rc += IRS_THREADS / TX) {
                    const int r = rc / 3, c = rc - 3 * r;
                    const float* p = img + ((size_t)c * SH + (size_t)(it.y0 + ymin + s_row[r])) * SW + (size_t)(it.x0 + lox);
                    float acc = 0.0f;
                    if constexpr (K <= IRS_KREG) {
#pragma unroll
                        for (int k = 0; k < K; k++) {
                            if (k >= cnt) break;
                            acc = acc + p[k] * w[k];
                        }
                    } else {
                        for (int k = 0; k < cnt; k++) acc = acc + p[k] * wl[k];
                    }
                    s_h[(r * 3 + c) * TX + j] = acc;
                }
            __syncthreads();
        }
    }
    for (int idx = tid; idx < TY * 3 * TX; idx += IRS_THREADS) {
        const int j = idx % TX, c = (idx / TX) % 3, r = idx / (3 * TX);
        const int X = tx0 + j, Y = ty0 + r;
        if (X >= ow || Y >= oh) continue;
        float v = par[c];
        const int cnt = s_cnty[r];
        if (any && cnt > 0 && s_cntx[j] > 0) {
            const int p0 = s_pos[min(s_loy[r] - ymin, HR - 1)];
            const float* w = s_wy + r * K;
            float acc = 0.0f;
            for (int k = 0; k < cnt; k++) acc = acc + s_h[(min(p0 + k, HR - 1) * 3 + c) * TX + j] * w[k];
            v = acc;
        }
        if (normalise) v = (v - par[3 + c]) / par[6 + c];
        out[(((size_t)i * 3 + c) * oh + Y) * ow + X] = v;
    }
}

template <int CLS>
static void irs_launch(hipStream_t stream, int fmt, int n, const void* src, int SH, int SW, const ResizeItem* items, const int* list, int l0, const float* par, int antialias,
                       int normalise, int oh, int ow, float* out) {
    using P = IrsShape<CLS>;
    const dim3 grid((ow + P::TX - 1) / P::TX, (oh + P::TY - 1) / P::TY, n);
    if (fmt == 0)
        hipLaunchKernelGGL((k_resize<CLS, 0>), grid, dim3(IRS_THREADS), 0, stream, src, SH, SW, items, list, l0, par, antialias, normalise, oh, ow, out);
    else
        hipLaunchKernelGGL((k_resize<CLS, 1>), grid, dim3(IRS_THREADS), 0, stream, src, SH, SW, items, list, l0, par, antialias, normalise, oh, ow, out);
}

int imgresize_launch(hipStream_t stream, const void* src, int fmt, int SH, int SW, const void* stage, int nout, const int count[IRS_CLASSES], int antialias, bool normalise,
                     int oh, int ow, float* out, std::string& err) {
    const ResizeItem* items = (const ResizeItem*)stage;
    const int* list = (const int*)(items + nout);
    const float* par = (const float*)(list + nout);
    const int norm = normalise ? 1 : 0;
    int first = 0;
    for (int cls = 0; cls < IRS_CLASSES; first += count[cls], cls++)
        for (int l0 = first; l0 < first + count[cls]; l0 += 65535) {
            const int n = std::min(65535, first + count[cls] - l0);
            if (cls == 0) irs_launch<0>(stream, fmt, n, src, SH, SW, items, list, l0, par, antialias, norm, oh, ow, out);
            else if (cls == 1) irs_launch<1>(stream, fmt, n, src, SH, SW, items, list, l0, par, antialias, norm, oh, ow, out);
            else irs_launch<2>(stream, fmt, n, src, SH, SW, items, list, l0, par, antialias, norm, oh, ow, out);
        }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("image resize kernels: ") + hipGetErrorString(e); return -3; }
    return 0;
}

}  // namespace avs

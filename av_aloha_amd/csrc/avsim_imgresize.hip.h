// avsim_imgresize.hip.h -- resizing images on the device, antialiased, into a rectangle of a padded output (avsim_image_resize):
// what avsim_api.hip needs of the unit csrc/avsim_imgresize.hip -- the record of an output, the checks on the caller's host arrays, the
// packing into the pinned staging and the launcher.
//
// av_aloha_amd/imgresize.py is the specification, and the device equals it bit for bit.  Like the image augmentation that needs every float32
// operation rounded on its own and correctly, so the kernels live in a unit built with avsim_imgaug.hip's flags (av_aloha_amd/build.py) and
// are reached through imgresize_launch (the build is -fno-gpu-rdc).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "avsim_stage.h"

namespace avs {

constexpr int IRS_THREADS = 256;
constexpr int IRS_MAX_RATIO = 16;      // source pixels per output pixel, per axis, at most: a filter of at most 33 taps
constexpr int IRS_CLASSES = 3;         // a kernel per class of ratio: <= 2 (5 taps), <= 5 (11 taps), <= 16 (33 taps)

// One output image as the kernels read it (validated by the host)
struct ResizeItem {
    int src, x0, y0, w, h, flip, ox, oy, rw, rh;
    int pad[2];
};
static_assert(sizeof(ResizeItem) == 48, "ResizeItem is twelve words");

// the class of an output: by the larger of its two ratios, computed as the kernels compute their scale
inline int imgresize_class(int w, int rw, int h, int rh) {
    const float sx = (float)w / (float)rw, sy = (float)h / (float)rh;
    const float s = sx > sy ? sx : sy;
    return s <= 2.0f ? 0 : (s <= 5.0f ? 1 : 2);
}

// the bytes of a call's staging: the items, the outputs ordered by class, then fill, mean and std (12 floats)
inline size_t imgresize_stage_bytes(int nout) { return (size_t)nout * (sizeof(ResizeItem) + sizeof(int)) + 12 * sizeof(float); }

// the conditions of the header on the host arrays; -1 and err says which
inline int imgresize_validate(int nsrc, int SH, int SW, const int32_t* src_box, const int32_t* dst, const int32_t* src_index, int nout, int antialias, const float* fill,
                              const float* mean_std, int oh, int ow, std::string& err) {
    char buf[240];
    if (antialias != 0 && antialias != 1) { err = "avsim_image_resize: antialias is 0 or 1"; return -1; }
    if (fill)
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(fill[c])) { err = "avsim_image_resize: a fill that is not finite"; return -1; }
    if (mean_std)
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(mean_std[3 + c]) || mean_std[3 + c] == 0.0f) { err = "avsim_image_resize: a std that is 0 or not finite"; return -1; }
    for (int i = 0; i < nout; i++) {
        const int32_t *b = src_box + 5 * (size_t)i, *d = dst + 4 * (size_t)i;
        const long long x0 = b[0], y0 = b[1], w = b[2], h = b[3], fl = b[4], ox = d[0], oy = d[1], rw = d[2], rh = d[3], s = src_index ? src_index[i] : i;
        const char* what = nullptr;
        if (s < 0 || s >= nsrc) what = "source image out of range";
        else if (w < 1 || h < 1 || rw < 1 || rh < 1) what = "an empty source box or dst rectangle";
        else if (x0 < 0 || y0 < 0 || x0 + w > SW || y0 + h > SH) what = "the source box does not lie inside the image";
        else if (ox < 0 || oy < 0 || ox + rw > ow || oy + rh > oh) what = "the dst rectangle does not lie inside the output";
        else if (w > IRS_MAX_RATIO * rw || h > IRS_MAX_RATIO * rh) what = "a ratio above 16";
        else if (fl != 0 && fl != 1) what = "flip is 0 or 1";
        if (what) {
            snprintf(buf, sizeof buf, "avsim_image_resize: output %d (source %lld, box %lld %lld %lld %lld %lld, dst %lld %lld %lld %lld): %s", i, s, x0, y0, w, h, fl, ox, oy,
                     rw, rh, what);
            err = buf;
            return -1;
        }
    }
    return 0;
}

// packs a validated call into `pin` (imgresize_stage_bytes(nout) bytes); count: the outputs of each class, which follow one another in the list
inline void imgresize_pack(void* pin, const int32_t* src_box, const int32_t* dst, const int32_t* src_index, int nout, const float* fill, const float* mean_std,
                           int count[IRS_CLASSES]) {
    ResizeItem* it = (ResizeItem*)pin;
    int* list = (int*)(it + nout);
    float* par = (float*)(list + nout);
    for (int k = 0; k < IRS_CLASSES; k++) count[k] = 0;
    for (int i = 0; i < nout; i++) {
        const int32_t *b = src_box + 5 * (size_t)i, *d = dst + 4 * (size_t)i;
        ResizeItem a{};
        a.src = src_index ? src_index[i] : i;
        a.x0 = b[0]; a.y0 = b[1]; a.w = b[2]; a.h = b[3]; a.flip = b[4];
        a.ox = d[0]; a.oy = d[1]; a.rw = d[2]; a.rh = d[3];
        a.pad[0] = imgresize_class(a.w, a.rw, a.h, a.rh);
        it[i] = a;
        count[a.pad[0]]++;
    }
    int at[IRS_CLASSES] = {0, count[0], count[0] + count[1]};
    for (int i = 0; i < nout; i++) list[at[it[i].pad[0]]++] = i;
    for (int c = 0; c < 3; c++) {
        par[c] = fill ? fill[c] : 0.0f;
        par[3 + c] = mean_std ? mean_std[c] : 0.0f;
        par[6 + c] = mean_std ? mean_std[3 + c] : 1.0f;
        par[9 + c] = 0.0f;
    }
}

// csrc/avsim_imgresize.hip.  stage: the device copy of what imgresize_pack wrote, count: its classes' lengths; src, out: device pointers.
// One launch of k_resize<class, fmt> per class that has outputs (and per 65535 of them).  -3: HIP
int imgresize_launch(hipStream_t stream, const void* src, int fmt, int SH, int SW, const void* stage, int nout, const int count[IRS_CLASSES], int antialias, bool normalise,
                     int oh, int ow, float* out, std::string& err);

// The host side of avsim_image_resize.  src, out: device pointers; the host arrays: validated.  -3: HIP
inline int imgresize_run(StageRing& ring, hipStream_t stream, const void* src, int fmt, int SH, int SW, const int32_t* src_box, const int32_t* dst, const int32_t* src_index,
                         int n, int antialias, const float* fill, const float* mean_std, int oh, int ow, float* out, std::string& err) {
    const size_t bytes = imgresize_stage_bytes(n);
    StageRing::Slot* s = ring.acquire(bytes, err);
    if (!s) return -3;
    int count[IRS_CLASSES];
    imgresize_pack(s->pin, src_box, dst, src_index, n, fill, mean_std, count);
    if (ring.upload(*s, bytes, stream, err)) return -3;
    std::string lerr;
    const int lrc = imgresize_launch(stream, src, fmt, SH, SW, s->dev.ptr(), n, count, antialias, mean_std != nullptr, oh, ow, out, lerr);
    const int rc = ring.release(*s, stream, err);
    if (lrc) { err = lerr; return lrc; }
    return rc;
}

}  // namespace avs

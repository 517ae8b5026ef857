// avsim_imgaug.hip.h -- colour, sharpness and affine augmentation of training images on the device (avsim_image_jitter, avsim_image_augment;
// DESIGN 8.ac, 8.af): what
// avsim_api.hip needs of the unit csrc/avsim_imgaug.hip -- the record of an output, the checks on the caller's host arrays and the launcher.
//
// av_aloha_amd/imgaug.py is the specification, and the device equals it bit for bit.  That needs every float32 operation rounded on its own
// and correctly -- no fused multiply-add, IEEE division, denormals kept --, which avsim_api.hip's flags do not give (build.py, F32_FLAGS):
// the kernels live in a unit of their own, built as avsim_phys_f64.hip is, and are reached through imgaug_launch (the build is -fno-gpu-rdc).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "avsim_stage.h"

namespace avs {

constexpr int IAG_THREADS = 256;
constexpr int IAG_TX = 64, IAG_TY = 16;      // k_aug_apply's tile of the output crop: 16 lanes of four pixels across, 16 rows
constexpr int IAG_BRIGHTNESS = 1, IAG_CONTRAST = 2, IAG_SATURATION = 4, IAG_HUE = 8, IAG_SHARPNESS = 16;
constexpr int IAG_AFFINE = 32;               // avsim_image_augment's geometric op
constexpr float IAG_MATRIX_LIMIT = 1048576.0f;                   // the largest magnitude of a matrix entry: source coordinates stay finite
constexpr size_t IAG_SCRATCH_BYTES = (size_t)128 << 20;          // the cap of the float scratch images of sharpness + affine

// One output image as the kernels read it (validated by the host): the source image, the box's corner, flip | mask << 1, the five factors
struct AugItem {
    int src, x0, y0, fm;
    float f[5];
    int pad[3];
};
static_assert(sizeof(AugItem) == 48, "AugItem is twelve words");

// the bytes of a call's staging: the items, the outputs that have the contrast bit, mean and std
inline size_t imgaug_stage_bytes(int nout) { return (size_t)nout * (sizeof(AugItem) + sizeof(int)) + 8 * sizeof(float); }

// the conditions of the header on the host arrays; -1 and err says which
inline int imgaug_validate(int nsrc, int SH, int SW, const int32_t* box_mask, const float* factor, const int32_t* src_index, int nout,
                           const float* mean_std, int oh, int ow, std::string& err, const char* fn = "avsim_image_jitter", int max_mask = 31) {
    static const char* const opname[5] = {"brightness", "contrast", "saturation", "hue", "sharpness"};
    char buf[240];
    if (mean_std)
        for (int c = 0; c < 3; c++) {
            if (!std::isfinite(mean_std[3 + c]) || mean_std[3 + c] == 0.0f) { err = std::string(fn) + ": a std that is 0 or not finite"; return -1; }
        }
    for (int i = 0; i < nout; i++) {
        const int32_t* b = box_mask + 4 * (size_t)i;
        const long long x0 = b[0], y0 = b[1], fl = b[2], mask = b[3], s = src_index ? src_index[i] : i;
        const char* what = nullptr;
        if (s < 0 || s >= nsrc) what = "source image out of range";
        else if (fl != 0 && fl != 1) what = "flip is 0 or 1";
        else if (mask < 0 || mask > max_mask) what = max_mask == 31 ? "mask outside 0..31" : "mask outside 0..63";
        else if (x0 < 0 || y0 < 0 || x0 + ow > SW || y0 + oh > SH) what = "the crop does not lie inside the source";
        if (what) {
            snprintf(buf, sizeof buf, "%s: output %d (source %lld, box %lld %lld %lld, mask %lld): %s", fn, i, s, x0, y0, fl, mask, what);
            err = buf;
            return -1;
        }
        for (int k = 0; k < 5; k++) {
            if (!((mask >> k) & 1)) continue;      // factors of unset bits are not looked at
            const float f = factor[5 * (size_t)i + k];
            const float lo = k == 3 ? -0.5f : 0.0f, hi = k == 3 ? 0.5f : 16.0f;
            if (!std::isfinite(f) || f < lo || f > hi) {
                snprintf(buf, sizeof buf, "%s: output %d: the %s factor %g is not a finite value in [%g, %g]", fn, i, opname[k], (double)f, (double)lo, (double)hi);
                err = buf;
                return -1;
            }
        }
    }
    return 0;
}

// packs a validated call into `pin` (imgaug_stage_bytes(nout) bytes) -> the number of outputs that have the contrast bit
inline int imgaug_pack(void* pin, const int32_t* box_mask, const float* factor, const int32_t* src_index, int nout, const float* mean_std) {
    AugItem* it = (AugItem*)pin;
    int* cidx = (int*)(it + nout);
    float* ms = (float*)(cidx + nout);
    int ncon = 0;
    for (int i = 0; i < nout; i++) {
        const int32_t* b = box_mask + 4 * (size_t)i;
        AugItem a{};
        a.src = src_index ? src_index[i] : i;
        a.x0 = b[0]; a.y0 = b[1]; a.fm = b[2] | (b[3] << 1);
        for (int k = 0; k < 5; k++) a.f[k] = ((b[3] >> k) & 1) ? factor[5 * (size_t)i + k] : 0.0f;
        it[i] = a;
        if (b[3] & IAG_CONTRAST) cidx[ncon++] = i;
    }
    for (int k = 0; k < 6; k++) ms[k] = mean_std ? mean_std[k] : (k < 3 ? 0.0f : 1.0f);
    ms[6] = ms[7] = 0.0f;
    return ncon;
}

// avsim_image_augment's conditions: imgaug_validate's with masks 0..63, interp 0 / 1 and, for an output that has bit 5, six finite matrix
// entries of magnitude at most 2^20 (affine may be NULL when no output has the bit; entries of outputs without it are not read)
inline int imgaug_validate_affine(int nsrc, int SH, int SW, const int32_t* box_mask, const float* factor, const float* affine, int interp, const int32_t* src_index,
                                  int nout, const float* mean_std, int oh, int ow, std::string& err) {
    char buf[200];
    if (interp != 0 && interp != 1) { err = "avsim_image_augment: interp is 0 (nearest) or 1 (bilinear)"; return -1; }
    if (imgaug_validate(nsrc, SH, SW, box_mask, factor, src_index, nout, mean_std, oh, ow, err, "avsim_image_augment", 63)) return -1;
    for (int i = 0; i < nout; i++) {
        if (!(box_mask[4 * (size_t)i + 3] & IAG_AFFINE)) continue;
        if (!affine) { snprintf(buf, sizeof buf, "avsim_image_augment: output %d has bit 5 and affine is NULL", i); err = buf; return -1; }
        for (int k = 0; k < 6; k++) {
            const float m = affine[6 * (size_t)i + k];
            if (!std::isfinite(m) || std::fabs(m) > IAG_MATRIX_LIMIT) {
                snprintf(buf, sizeof buf, "avsim_image_augment: output %d: matrix entry %d (%g) is not a finite value of magnitude <= 2^20", i, k, (double)m);
                err = buf;
                return -1;
            }
        }
    }
    return 0;
}

// the bytes of an avsim_image_augment call's staging: imgaug_pack's, then the matrices and three lists of outputs -- without bit 5, with it
// and without sharpness, with both
inline size_t imgaug_stage_bytes_affine(int nout) { return imgaug_stage_bytes(nout) + (size_t)nout * (6 * sizeof(float) + 3 * sizeof(int)); }

// packs a validated call into `pin` (imgaug_stage_bytes_affine(nout) bytes) -> the number of outputs that have the contrast bit; count: the lists' lengths
inline int imgaug_pack_affine(void* pin, const int32_t* box_mask, const float* factor, const float* affine, const int32_t* src_index, int nout, const float* mean_std,
                              int count[3]) {
    const int ncon = imgaug_pack(pin, box_mask, factor, src_index, nout, mean_std);
    float* mats = (float*)((char*)pin + imgaug_stage_bytes(nout));
    int* list[3] = {(int*)(mats + 6 * (size_t)nout), nullptr, nullptr};
    list[1] = list[0] + nout;
    list[2] = list[1] + nout;
    count[0] = count[1] = count[2] = 0;
    for (int i = 0; i < nout; i++) {
        const int mask = box_mask[4 * (size_t)i + 3];
        const bool aff = mask & IAG_AFFINE;
        for (int k = 0; k < 6; k++) mats[6 * (size_t)i + k] = aff ? affine[6 * (size_t)i + k] : (k == 0 || k == 4 ? 1.0f : 0.0f);
        const int which = !aff ? 0 : (mask & IAG_SHARPNESS) ? 2 : 1;
        list[which][count[which]++] = i;
    }
    return ncon;
}

// csrc/avsim_imgaug.hip.  stage: the device copy of what imgaug_pack wrote; gsum: nout 64-bit slots of the library's; src, out: device
// pointers.  Zeroes gsum, runs k_aug_gray_sum for the ncon outputs that have the contrast bit and k_aug_apply for all.  -3: HIP
int imgaug_launch(hipStream_t stream, const void* src, int SH, int SW, const void* stage, int nout, int ncon, bool normalise, int oh, int ow,
                  unsigned long long* gsum, float* out, std::string& err);

// csrc/avsim_imgaug.hip.  stage: the device copy of what imgaug_pack_affine wrote, count: its lists' lengths.  The gray sums as above;
// k_aug_apply_list for the outputs without bit 5, k_aug_affine<interp, 0> for those with it and without sharpness, and for those with both,
// `group` (>= 1) at a time, k_aug_whole into scratch (group x 3 x SH x SW floats) and k_aug_affine<interp, 1> out of it.  -3: HIP
int imgaug_launch_affine(hipStream_t stream, const void* src, int SH, int SW, const void* stage, int nout, int ncon, const int count[3], int interp, bool normalise,
                         int oh, int ow, unsigned long long* gsum, float* scratch, int group, float* out, std::string& err);

// The host side of avsim_image_jitter: the gray sums behind contrast, one 64-bit slot per output, grown on demand and kept for
// avsim_image_jitter_sums; the per-call arrays go through the library's pinned staging like avsim_image_prep's
struct ImgAugHost {
    DevBuf gsum;       // unsigned long long [outputs, rounded up to 512]
    int nout = 0;      // the outputs of the last call
    // avsim_image_augment: the float images of the outputs that have sharpness and bit 5, a group at a time; grown on demand, at most
    // scratch_limit bytes (option "augment_scratch_bytes") unless one image alone is larger
    DevBuf scratch;
    size_t scratch_limit = IAG_SCRATCH_BYTES;

    int grow_sums(int n, std::string& err) {
        const hipError_t e = gsum.reserve(sizeof(unsigned long long) * (((size_t)n + 511) & ~(size_t)511));
        if (e != hipSuccess) { err = std::string("image jitter sums: ") + hipGetErrorString(e); return -3; }
        return 0;
    }

    // avsim_image_augment with at least one bit 5.  -3: HIP
    int launch_affine(StageRing& ring, hipStream_t stream, const void* src, int SH, int SW, const int32_t* box_mask, const float* factor, const float* affine, int interp,
                      const int32_t* src_index, int n, const float* mean_std, int oh, int ow, float* out, std::string& err) {
        if (grow_sums(n, err)) return -3;
        const size_t bytes = imgaug_stage_bytes_affine(n);
        StageRing::Slot* s = ring.acquire(bytes, err);
        if (!s) return -3;
        int count[3];
        const int ncon = imgaug_pack_affine(s->pin, box_mask, factor, affine, src_index, n, mean_std, count);
        int group = 1;
        if (count[2] > 0) {
            const size_t one = sizeof(float) * 3 * (size_t)SH * SW;
            group = (int)std::min<size_t>(std::min<size_t>((size_t)count[2], 65535), std::max<size_t>(1, scratch_limit / one));
            const hipError_t e = scratch.reserve(one * group);      // (growing frees the old one, which waits for the kernels that still read it)
            if (e != hipSuccess) { err = std::string("image augment scratch: ") + hipGetErrorString(e); return -3; }
        }
        if (ring.upload(*s, bytes, stream, err)) return -3;
        std::string lerr;
        const int lrc = imgaug_launch_affine(stream, src, SH, SW, s->dev.ptr(), n, ncon, count, interp, mean_std != nullptr, oh, ow, gsum.as<unsigned long long>(), scratch.as<float>(), group, out, lerr);
        const int rc = ring.release(*s, stream, err);
        if (lrc) { err = lerr; return lrc; }
        if (rc == 0) nout = n;
        return rc;
    }

    // src, out: device pointers; the four arrays: host, validated.  -3: HIP
    int launch(StageRing& ring, hipStream_t stream, const void* src, int SH, int SW, const int32_t* box_mask, const float* factor, const int32_t* src_index,
               int n, const float* mean_std, int oh, int ow, float* out, std::string& err) {
        if (grow_sums(n, err)) return -3;
        const size_t bytes = imgaug_stage_bytes(n);
        StageRing::Slot* s = ring.acquire(bytes, err);
        if (!s) return -3;
        const int ncon = imgaug_pack(s->pin, box_mask, factor, src_index, n, mean_std);
        if (ring.upload(*s, bytes, stream, err)) return -3;
        std::string lerr;
        const int lrc = imgaug_launch(stream, src, SH, SW, s->dev.ptr(), n, ncon, mean_std != nullptr, oh, ow, gsum.as<unsigned long long>(), out, lerr);
        const int rc = ring.release(*s, stream, err);
        if (lrc) { err = lerr; return lrc; }
        if (rc == 0) nout = n;
        return rc;
    }
};

}  // namespace avs

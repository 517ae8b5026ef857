// avsim_obshist.hip.h -- per-env observation histories on the device (avsim_obs_history_*): what avsim_api.hip needs of the unit
// csrc/avsim_obshist.hip -- the arguments of the kernels, the checks of the set-up, the state a handle owns and the launcher.
//
// av_aloha_amd/obshist.py is the specification, and the device equals it bit for bit: the images are table entries copied (imgprep.py's
// prep_reference), the state is (x - mean) / std in two float32 operations, the division the IEEE one, denormals kept.  avsim_api.hip's flags
// do not give that (build.py, F32_FLAGS), so the kernels live in a unit built as avsim_imgaug.hip is and are reached through obs_launch_push
// (the build is -fno-gpu-rdc).
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

constexpr int OBH_MAX_K = 16, OBH_MAX_D = 256, OBH_MAX_CAMS = 8;
constexpr int OBH_BOOK_THREADS = 1024;      // k_obs_book is one workgroup
constexpr int OBH_THREADS = 256;
constexpr int OBH_MAX_SLABS = 4096;         // workgroups per env and camera; the lanes stride over what is left

// The kernels' view of a handle's history state.  pushed / last_id: k_obs_book's alone.  cur_fresh: what it found for THIS call, the only
// per-env state the passes read -- it runs in front of them on the same stream, after every reader of the previous call.
struct ObsArgs {
    int N, K, D, has_ms, ncam, fmt, SH, SW, oh, ow;
    int64_t* last_id;
    int *pushed, *cur_fresh;
    const float* ms;             // mean[D], std[D]
    const float* lut;            // [ncam][3][256]
    const int* box;              // [ncam][3]: x0, y0, flip
};

// The pointers of one push, a kernel argument: the cameras' source batches and histories (device pointers)
struct ObsPtrs {
    const void* img[OBH_MAX_CAMS];
    float* hist[OBH_MAX_CAMS];
};

// the refusals of avsim_obs_history_setup; -1 and err says which
inline int obs_validate(int K, int D, const float* mean_std, int ncam, int fmt, int SH, int SW, const float* lut, const int32_t* box, int oh, int ow,
                        std::string& err) {
    char buf[200];
    const char* F = "avsim_obs_history_setup";
    if (K < 1 || K > OBH_MAX_K) { snprintf(buf, sizeof buf, "%s: n_obs_steps %d outside 1..%d", F, K, OBH_MAX_K); err = buf; return -1; }
    if (D < 0 || D > OBH_MAX_D) { snprintf(buf, sizeof buf, "%s: state_dim %d outside 0..%d", F, D, OBH_MAX_D); err = buf; return -1; }
    if (ncam < 0 || ncam > OBH_MAX_CAMS) { snprintf(buf, sizeof buf, "%s: %d cameras, outside 0..%d", F, ncam, OBH_MAX_CAMS); err = buf; return -1; }
    if (D == 0 && ncam == 0) { snprintf(buf, sizeof buf, "%s: neither a state nor a camera", F); err = buf; return -1; }
    if (mean_std)
        for (int i = 0; i < 2 * D; i++) {
            if (!std::isfinite(mean_std[i])) { snprintf(buf, sizeof buf, "%s: a state mean or std that is not finite", F); err = buf; return -1; }
            if (i >= D && mean_std[i] == 0.0f) { snprintf(buf, sizeof buf, "%s: std[%d] is 0", F, i - D); err = buf; return -1; }
        }
    if (ncam > 0) {
        if (fmt != 0 && fmt != 1) { snprintf(buf, sizeof buf, "%s: image format %d is 0 (u8 HWC) or 1 (float32 CHW)", F, fmt); err = buf; return -1; }
        if (SH < 1 || SH > 65535 || SW < 1 || SW > 65535 || oh < 1 || oh > 65535 || ow < 1 || ow > 65535) {
            snprintf(buf, sizeof buf, "%s: a size of %d x %d -> %d x %d outside 1..65535", F, SH, SW, oh, ow);
            err = buf;
            return -1;
        }
        if (!lut || !box) { snprintf(buf, sizeof buf, "%s: cameras need their tables and boxes", F); err = buf; return -1; }
        for (int c = 0; c < ncam; c++) {
            const long long x0 = box[3 * c], y0 = box[3 * c + 1], fl = box[3 * c + 2];
            if (fl != 0 && fl != 1) { snprintf(buf, sizeof buf, "%s: camera %d: flip is 0 or 1", F, c); err = buf; return -1; }
            if (x0 < 0 || y0 < 0 || x0 + ow > SW || y0 + oh > SH) {
                snprintf(buf, sizeof buf, "%s: camera %d: the crop (%lld, %lld) + %d x %d does not lie inside the %d x %d source", F, c, x0, y0, oh, ow, SH, SW);
                err = buf;
                return -1;
            }
        }
    }
    return 0;
}

// csrc/avsim_obshist.hip.  All pointers are device pointers: k_obs_book, then the state pass (D > 0) and the image pass (ncam > 0)
void obs_launch_push(hipStream_t stream, const ObsArgs& P, const ObsPtrs& Q, const int64_t* episode_id, const int* elapsed, const float* state, float* state_hist);

// The state a handle owns (avsim_obs_history_setup), sized to its num_envs
struct ObsHistHost {
    bool ready = false;
    ObsArgs P{};
    DevArena arena;
    std::vector<float> host_f;        // what the set-up uploads (kept until the next set-up): mean, std, the tables
    std::vector<int> host_box;

    void destroy() {
        arena.clear();
        ready = false;
        P = ObsArgs{};
    }

    // validated arguments; the stream is idle (the caller synchronised it).  -3: HIP
    int setup(hipStream_t stream, int N, int K, int D, const float* mean_std, int ncam, int fmt, int SH, int SW, const float* lut, const int32_t* box, int oh,
              int ow, std::string& err) {
        destroy();
        ObsArgs a{};
        a.N = N; a.K = K; a.D = D; a.has_ms = mean_std != nullptr && D > 0; a.ncam = ncam;
        if (ncam > 0) { a.fmt = fmt; a.SH = SH; a.SW = SW; a.oh = oh; a.ow = ow; }
        const size_t n = (size_t)N;
        auto get = [&](size_t bytes) { return arena.zeroed(bytes, stream); };
        a.last_id = (int64_t*)get(sizeof(int64_t) * n);
        a.pushed = (int*)get(sizeof(int) * n);
        a.cur_fresh = (int*)get(sizeof(int) * n);
        const size_t nf = 2 * (size_t)D + 768 * (size_t)ncam;
        float* f = (float*)get(sizeof(float) * nf);
        int* b = (int*)get(sizeof(int) * 3 * (size_t)(ncam ? ncam : 1));
        hipError_t e = arena.error();
        if (e == hipSuccess) {
            host_f.assign(nf ? nf : 1, 0.0f);
            if (a.has_ms) std::copy(mean_std, mean_std + 2 * D, host_f.begin());
            if (ncam > 0) std::copy(lut, lut + 768 * (size_t)ncam, host_f.begin() + 2 * D);
            host_box.assign(3 * (size_t)(ncam ? ncam : 1), 0);
            if (ncam > 0) std::copy(box, box + 3 * ncam, host_box.begin());
            if (nf) e = hipMemcpyAsync(f, host_f.data(), sizeof(float) * nf, hipMemcpyHostToDevice, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(b, host_box.data(), sizeof(int) * host_box.size(), hipMemcpyHostToDevice, stream);
        }
        if (e != hipSuccess) {
            err = std::string("avsim_obs_history_setup: ") + hipGetErrorString(e);
            destroy();
            return -3;
        }
        a.ms = f;
        a.lut = f + 2 * (size_t)D;
        a.box = b;
        P = a;
        ready = true;
        return 0;
    }
};

}  // namespace avs

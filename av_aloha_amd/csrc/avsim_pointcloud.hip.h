// avsim_pointcloud.hip.h -- point clouds, voxel grids and virtual views on the device (avsim_camera_poses, avsim_point_cloud; avsim_voxel_grid; 8.ai;
// avsim_virtual_views; 8.al): what avsim_api.hip needs of the
// unit csrc/avsim_pointcloud.hip -- the limits, the checks on the caller's host arrays, the scratch of a chunk of envs and the launchers.
//
// av_aloha_amd/pointcloud.py is the specification, and the device equals it bit for bit given the camera poses.  Like the image calls that
// needs every float32 operation rounded on its own and correctly, so the kernels live in a unit built with avsim_imgaug.hip's flags
// (av_aloha_amd/build.py) and are reached through pointcloud_poses_launch / pointcloud_launch (the build is -fno-gpu-rdc).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "avsim_dev.h"

namespace avs {

constexpr int PC_THREADS = 1024;             // one workgroup per env: 16 waves
constexpr int PC_MAX_CANDIDATES = 16384;     // AVSIM_PC_MAX_CANDIDATES: 16 per lane, xyz and the running distance in registers
constexpr int PC_MAX_POINTS = 4096;
constexpr int PC_MAX_CAMS = 16;              // the renderer's limit
constexpr int PC_MAX_PIXELS = 1 << 24;       // ncam * H * W of one env
constexpr int PC_POSE_W = 16;                // floats of a pose record: pc[3], Rc[9], tan(fovy / 2), 0, 0, 0
constexpr int PC_ENV_CHUNK = 1024;           // envs per pass: bounds the scratch

// the camera tables of the render model and the body poses, as the pose kernel reads them (device pointers)
struct PcModel {
    const float* xpose;       // [N][nbody][12]
    const int* cam_body;
    const float *cam_pos, *cam_mat, *cam_tan;
    int nbody;
};

// what a call passes by value: nothing of the caller's host arrays is read after the call returns, and nothing is staged
struct PcCall {
    int cam[PC_MAX_CAMS];
    int ncam, H, W, P;
    float lo[3], hi[3], max_depth;
};

// the conditions of the header; -1 and err says which
inline int pointcloud_validate(int ncam_model, const int32_t* cam_ids, int ncam, int H, int W, const float* bounds, float max_depth, int npoints, std::string& err) {
    char buf[200];
    const char* what = nullptr;
    if (ncam < 1 || ncam > PC_MAX_CAMS) what = "1..16 cameras";
    else if (npoints < 1 || npoints > PC_MAX_POINTS) what = "npoints outside 1..4096";
    else if (H < 1 || H > 65535 || W < 1 || W > 65535) what = "an image size outside 1..65535";
    else if ((long long)ncam * H * W > PC_MAX_PIXELS) what = "more than 2^24 pixels per env";
    else if (!std::isfinite(max_depth) || !(max_depth > 0.0f)) what = "max_depth is finite and > 0";
    if (!what)
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(bounds[k])) what = "a bound that is not finite";
    if (!what)
        for (int k = 0; k < 3; k++)
            if (bounds[k] > bounds[3 + k]) what = "a lower bound above its upper bound";
    if (!what)
        for (int c = 0; c < ncam; c++)
            if (cam_ids[c] < 0 || cam_ids[c] >= ncam_model) what = "camera index out of range";
    if (what) {
        snprintf(buf, sizeof buf, "avsim_point_cloud: %s (%d cameras, %d x %d, %d points)", what, ncam, H, W, npoints);
        err = buf;
        return -1;
    }
    return 0;
}

// csrc/avsim_pointcloud.hip.  out: device float [n][ncam][16], the records of envs e0 .. e0 + n - 1.  -3: HIP
int pointcloud_poses_launch(hipStream_t stream, const PcModel& m, const PcCall& c, int e0, int n, float* out, std::string& err);
// one workgroup per env of the chunk: depth [n][ncam][H][W], pose [n][ncam][16], list: the chunk's scratch, [n][min(ncam H W, 16384)]
// int32; xyz [n][P][3], index [n][P], count [n][2] -- all device pointers of the chunk's first env.  -3: HIP
int pointcloud_launch(hipStream_t stream, const PcCall& c, int n, const float* depth, const float* pose, int* list, float* xyz, int* index, int* count, std::string& err);

// The scratch of a chunk of envs: pose records and candidate lists.  Grows, never shrinks; allocating synchronises (the first use of a size)
struct PcHost {
    DevBuf pose, list;

    static size_t list_len(const PcCall& c) {
        const size_t q = (size_t)c.ncam * c.H * c.W;
        return q < (size_t)PC_MAX_CANDIDATES ? q : (size_t)PC_MAX_CANDIDATES;
    }
    int reserve(int chunk, const PcCall& c, std::string& err) {
        const size_t nl = (size_t)chunk * list_len(c);
        if (const int rc = reserve_poses(chunk, c.ncam, err)) return rc;
        if (list.reserve(nl * sizeof(int)) != hipSuccess) { err = "hipMalloc(point cloud candidates) failed"; return -3; }
        return 0;
    }
    // the pose records alone (avsim_voxel_grid: its accumulator is the caller's output, no other scratch)
    int reserve_poses(int chunk, int ncam, std::string& err) {
        const size_t np = (size_t)chunk * ncam * PC_POSE_W;
        if (pose.reserve(np * sizeof(float)) != hipSuccess) { err = "hipMalloc(point cloud poses) failed"; return -3; }
        return 0;
    }
    // poses of the current body poses, then the cloud, a chunk of envs at a time.  All pointers: device, of env 0
    int run(hipStream_t stream, const PcModel& m, const PcCall& c, int N, const float* depth, float* xyz, int* index, int* count, std::string& err) {
        const int chunk = N < PC_ENV_CHUNK ? N : PC_ENV_CHUNK;
        int rc;
        if ((rc = reserve(chunk, c, err))) return rc;
        const size_t q = (size_t)c.ncam * c.H * c.W;
        for (int e0 = 0; e0 < N; e0 += chunk) {
            const int n = N - e0 < chunk ? N - e0 : chunk;
            if ((rc = pointcloud_poses_launch(stream, m, c, e0, n, pose.as<float>(), err))) return rc;
            if ((rc = pointcloud_launch(stream, c, n, depth + (size_t)e0 * q, pose.as<float>(), list.as<int>(), xyz + (size_t)e0 * c.P * 3, index + (size_t)e0 * c.P, count + (size_t)e0 * 2, err))) return rc;
        }
        return 0;
    }
};

// ---- voxel grids (avsim_voxel_grid; av_aloha_amd/voxel.py is the specification): the same points and candidates scattered into a
// dense grid of seven u32 sums per cell, in the caller's output buffer, and finished in place into eight float32 channels
constexpr int VOX_MAX_DIM = 256;             // AVSIM_VOXEL_MAX_DIM
constexpr int VOX_MAX_CELLS = 1 << 21;       // AVSIM_VOXEL_MAX_CELLS
constexpr int VOX_CHANNELS = 8;
// the accumulate form the library ships: 1 = runs of consecutive lanes in one cell are summed in the wave and the run's first lane adds,
// 0 = every candidate lane adds.  Both are compiled; option "voxel_other_form" runs the one not picked here, for a measurement (tools/bench_voxel.py)
#ifndef AVSIM_VOXEL_MERGE
#define AVSIM_VOXEL_MERGE 1
#endif

struct VoxCall {
    PcCall pc;                // cameras, image size, box, max_depth (P unused)
    int g[3];
};

inline int voxel_validate(int ncam_model, const int32_t* cam_ids, int ncam, int H, int W, const float* bounds, float max_depth, const int32_t* grid, std::string& err) {
    char buf[240];
    const char* what = nullptr;
    if (ncam < 1 || ncam > PC_MAX_CAMS) what = "1..16 cameras";
    else if (H < 1 || H > 65535 || W < 1 || W > 65535) what = "an image size outside 1..65535";
    else if ((long long)ncam * H * W > PC_MAX_PIXELS) what = "more than 2^24 pixels per env";
    else if (grid[0] < 1 || grid[0] > VOX_MAX_DIM || grid[1] < 1 || grid[1] > VOX_MAX_DIM || grid[2] < 1 || grid[2] > VOX_MAX_DIM) what = "a grid dim outside 1..256";
    else if ((long long)grid[0] * grid[1] * grid[2] > VOX_MAX_CELLS) what = "more than 2^21 cells";
    else if (!std::isfinite(max_depth) || !(max_depth > 0.0f)) what = "max_depth is finite and > 0";
    if (!what)
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(bounds[k])) what = "a bound that is not finite";
    if (!what)
        for (int k = 0; k < 3; k++) {
            if (!(bounds[k] < bounds[3 + k])) { what = "a lower bound that is not below its upper bound"; break; }
            const volatile float ext = bounds[3 + k] - bounds[k];          // (volatile: rounded to float32 here, whatever the host's flags)
            const volatile float inv = (float)grid[k] / ext, size = ext / (float)grid[k];
            if (!std::isfinite(inv) || !std::isfinite(size)) what = "an extent whose cell size or its reciprocal is not a finite float32";
        }
    if (!what)
        for (int c = 0; c < ncam; c++)
            if (cam_ids[c] < 0 || cam_ids[c] >= ncam_model) what = "camera index out of range";
    if (what) {
        snprintf(buf, sizeof buf, "avsim_voxel_grid: %s (%d cameras, %d x %d, grid %d x %d x %d)", what, ncam, H, W, grid[0], grid[1], grid[2]);
        err = buf;
        return -1;
    }
    return 0;
}

// csrc/avsim_pointcloud.hip.  The three passes over a chunk of n envs: depth [n][ncam][H][W], rgb u8 [n][ncam][H][W][3] or null, pose
// [n][ncam][16], out [n][gx][gy][gz][8] -- device pointers of the chunk's first env.  merge: the accumulate form.  -3: HIP
int voxel_launch(hipStream_t stream, const VoxCall& c, int n, const float* depth, const uint8_t* rgb, const float* pose, float* out, bool merge, std::string& err);

// ---- virtual orthographic views (avsim_virtual_views; av_aloha_amd/virtviews.py is the specification): the same points and candidates
// scattered into up to six axis-aligned images of the box by a z-buffer whose entry is ONE unsigned 64-bit key -- the bits of the distance to the
// view's face above the source pixel's flat slot -- and whose update is an atomic minimum: the nearest point wins and, among equals, the lowest
// slot, whatever the order of arrival.  The caller's output is the buffer: a virtual pixel's first 8 of its 32 bytes hold the key until
// k_vv_finish turns the pixel into its eight float32 channels in place.
constexpr int VV_MAX_VIEWS = 6;              // AVSIM_VV_MAX_VIEWS
constexpr int VV_MAX_SIZE = 1024;            // AVSIM_VV_MAX_SIZE
constexpr int VV_MAX_RADIUS = 4;             // AVSIM_VV_MAX_RADIUS
constexpr int VV_CHANNELS = 8;
// the scatter form the library ships.  Two bits name a form outright: 1 = a lane first LOADS the virtual pixel's key and skips the atomic when its
// own is not smaller (keys only decrease: a stale read costs an atomic that loses, never a wrong result), 2 = runs of consecutive lanes on the
// same virtual pixel take their minimum in the wave and the run's first lane alone issues.  4 = the merge always, and the load where the
// measurement has it pay (vv_form below).  All four forms are compiled and give the same bits; option "virtviews_form" f + 1 runs form f (0: the
// one picked here), for a measurement (tools/bench_virtviews.py).  4 ships (DESIGN 8.al has the table)
#ifndef AVSIM_VV_FORM
#define AVSIM_VV_FORM 4
#endif

struct VvCall {
    PcCall pc;                // cameras, image size, box, max_depth (P unused)
    int view[VV_MAX_VIEWS];
    int nviews, VH, VW, radius;
};

inline int virtviews_validate(int ncam_model, const int32_t* cam_ids, int ncam, int H, int W, const float* bounds, float max_depth, const int32_t* views, int nviews,
                              const int32_t* size, int radius, std::string& err) {
    char buf[260];
    const char* what = nullptr;
    if (ncam < 1 || ncam > PC_MAX_CAMS) what = "1..16 cameras";
    else if (H < 1 || H > 65535 || W < 1 || W > 65535) what = "an image size outside 1..65535";
    else if ((long long)ncam * H * W > PC_MAX_PIXELS) what = "more than 2^24 pixels per env";
    else if (nviews < 1 || nviews > VV_MAX_VIEWS) what = "1..6 views";
    else if (size[0] < 1 || size[0] > VV_MAX_SIZE || size[1] < 1 || size[1] > VV_MAX_SIZE) what = "a view size outside 1..1024";
    else if (radius < 0 || radius > VV_MAX_RADIUS) what = "a radius outside 0..4";
    else if (!std::isfinite(max_depth) || !(max_depth > 0.0f)) what = "max_depth is finite and > 0";
    if (!what)
        for (int v = 0; v < nviews; v++)
            if (views[v] < 0 || views[v] > 5) what = "a view code outside 0..5";
    if (!what)
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(bounds[k])) what = "a bound that is not finite";
    if (!what)
        for (int k = 0; k < 3 && !what; k++) {
            if (!(bounds[k] < bounds[3 + k])) { what = "a lower bound that is not below its upper bound"; break; }
            const volatile float ext = bounds[3 + k] - bounds[k];          // (volatile: rounded to float32 here, whatever the host's flags)
            for (int a = 0; a < 2; a++) {          // every axis against both image sides, whichever views the call names
                const volatile float inv = (float)size[a] / ext, px = ext / (float)size[a];
                if (!std::isfinite(inv) || !std::isfinite(px)) what = "an extent whose pixel size or its reciprocal is not a finite float32";
            }
        }
    if (!what)
        for (int c = 0; c < ncam; c++)
            if (cam_ids[c] < 0 || cam_ids[c] >= ncam_model) what = "camera index out of range";
    if (what) {
        snprintf(buf, sizeof buf, "avsim_virtual_views: %s (%d cameras, %d x %d, %d views of %d x %d, radius %d)", what, ncam, H, W, nviews, nviews >= 1 ? size[0] : 0,
                 nviews >= 1 ? size[1] : 0, radius);
        err = buf;
        return -1;
    }
    return 0;
}

// the two bits of form 4 for a call.  The merge always: it is never slower than the form without it beyond the spread of the rounds.  The load with
// a footprint of more than one pixel -- the footprints of neighbouring lanes overlap, an atomic instruction then carries several lanes on one
// address, which the atomic unit takes one after the other, where a load of them is one access: 1.5 to 1.6 times faster than the merge alone --
// and with radius 0 where a view has more pixels than the env has source pixels (there it was 1.0 to 1.5 % faster; with fewer pixels between
// 1.4 % faster and 2.7 % slower: the merge has left one lane per address, and the load is a second access for every lane whose atomic is
// still needed).  profiles/virtviews_r20.json
inline int vv_form(int form, const VvCall& c) {
    if (form != 4) return form & 3;
    return 2 | ((c.radius > 0 || (long long)c.VH * c.VW > (long long)c.pc.ncam * c.pc.H * c.pc.W) ? 1 : 0);
}

// csrc/avsim_pointcloud.hip.  The three passes over a chunk of n envs: depth [n][ncam][H][W], rgb u8 [n][ncam][H][W][3] or null, pose
// [n][ncam][16], out [n][nviews][VH][VW][8], index [n][nviews][VH][VW] -- device pointers of the chunk's first env.  form: the scatter's two bits.  -3: HIP
int virtviews_launch(hipStream_t stream, const VvCall& c, int n, const float* depth, const uint8_t* rgb, const float* pose, float* out, int32_t* index, int form, std::string& err);

}  // namespace avs

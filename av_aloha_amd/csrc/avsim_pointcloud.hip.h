// avsim_pointcloud.hip.h -- point clouds and voxel grids on the device (avsim_camera_poses, avsim_point_cloud; avsim_voxel_grid; 8.ai): what avsim_api.hip needs of the
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

}  // namespace avs

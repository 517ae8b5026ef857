// avsim_pointcloud.hip -- the kernels of avsim_camera_poses and avsim_point_cloud: depth images deprojected into one world
// frame, cropped to a box, capped and thinned by farthest point sampling.  av_aloha_amd/pointcloud.py is the specification; every float32
// operation here is the one it names, rounded on its own.  The unit is built -ffp-contract=off with IEEE division and denormals kept
// (av_aloha_amd/build.py): a * b + c is a v_mul and a v_add.
//
//   k_pc_poses   a lane per (env, camera slot): the camera's world pose from the body pose and the model's camera tables, a record of 16
//       floats.  avsim_camera_poses returns these records; k_pc_cloud reads them.
//   k_pc_cloud   a workgroup of 1024 per env, three phases.
//       1. Ordered compaction.  Wave w owns the contiguous pixels [w per, (w + 1) per) of the env's ncam H W, per a multiple of 64.  It
//          counts its candidates (a ballot per 64 pixels), the 16 counts are summed in LDS (M, and the wave's first position), and a second
//          walk over the same pixels writes candidate `pos` to the env's list -- at pos, or with M > 16384 at i where (i M) / 16384 == pos,
//          if there is such an i (at most one: M > 16384).  The order is the pixels': nothing is appended atomically.
//       2. Farthest point sampling.  Candidate k = 1024 j + tid lives in lane tid's registers, trip j: xyz recomputed from the depth (the
//          same function, the same bits) and the running squared distance, 64 registers for 16 trips.  An iteration updates the distances
//          against the last selection and finds the arg-max as the maximum of a 64-bit key -- the distance's bits above the complement of
//          the position, so that the larger distance wins and, among equals, the LOWER position: two DPP reductions per wave, the
//          wave's winner and its coordinates into LDS, ONE barrier, then every lane takes the maximum of the 16 keys and reads the winner's
//          coordinates (the winner's wave is a field of its position).  The LDS records alternate between two sets, which is what makes one
//          barrier enough.  When the winning distance is 0 every distance is, and by the rule all further selections are candidate 0.
//       3. The selected positions (LDS) become points and pixel indices, 1024 at a time.
//   k_vox_clear, k_vox_accum, k_vox_finish   avsim_voxel_grid, below the cloud's: they call pc_world and read k_pc_poses's records.
//   k_vv_clear, k_vv_scatter, k_vv_finish   avsim_virtual_views, below the grid's: likewise.
#include "avsim_pointcloud.hip.h"

namespace avs {

__global__ void __launch_bounds__(256) k_pc_poses(PcModel m, PcCall c, int e0, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * c.ncam) return;
    const int e = i / c.ncam, s = i - e * c.ncam, cam = c.cam[s];
    const float *pb = m.xpose + ((size_t)(e0 + e) * m.nbody + m.cam_body[cam]) * 12, *Rb = pb + 3, *cp = m.cam_pos + 3 * cam, *Rm = m.cam_mat + 9 * cam;
    float* o = out + (size_t)i * PC_POSE_W;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        o[r] = ((pb[r] + Rb[3 * r] * cp[0]) + Rb[3 * r + 1] * cp[1]) + Rb[3 * r + 2] * cp[2];
#pragma unroll
        for (int j = 0; j < 3; j++) o[3 + 3 * r + j] = (Rb[3 * r] * Rm[j] + Rb[3 * r + 1] * Rm[3 + j]) + Rb[3 * r + 2] * Rm[6 + j];
    }
    o[12] = m.cam_tan[cam];
    o[13] = o[14] = o[15] = 0.0f;
}

// the crop box and what locates a pixel, in registers
struct PcView {
    int HW, W;
    float hh, hw, lo[3], hi[3], max_depth;
};

// pixel `pix` of the env (slot H W + r W + c) as a world point; true when it is a candidate.  s_pose: the env's records, s_scale: 2 t / H per slot
__device__ __forceinline__ bool pc_world(const PcView& v, const float* s_pose, const float* s_scale, const float* __restrict__ depth, int pix, float& wx, float& wy, float& wz) {
    const int slot = pix / v.HW, rem = pix - slot * v.HW, r = rem / v.W, c = rem - r * v.W;
    const float* P = s_pose + slot * PC_POSE_W;
    const float sc = s_scale[slot], d = depth[pix];
    const float x = (((float)c + 0.5f) - v.hw) * sc;
    const float y = -((((float)r + 0.5f) - v.hh) * sc);
    const float X = x * d, Y = y * d, Z = -d;
    wx = ((P[0] + P[3] * X) + P[4] * Y) + P[5] * Z;
    wy = ((P[1] + P[6] * X) + P[7] * Y) + P[8] * Z;
    wz = ((P[2] + P[9] * X) + P[10] * Y) + P[11] * Z;
    return d < v.max_depth && wx >= v.lo[0] && wx <= v.hi[0] && wy >= v.lo[1] && wy <= v.hi[1] && wz >= v.lo[2] && wz <= v.hi[2];
}

constexpr int PC_WAVES = PC_THREADS / 64, PC_TRIPS = PC_MAX_CANDIDATES / PC_THREADS;

// the maximum over the 64 lanes of the wave, the same in every lane (through an SGPR): DPP moves, no LDS (avsim_phys.hip.h's wave_sum with max)
__device__ __forceinline__ unsigned wave_umax(unsigned x) {
    x = max(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x128, 0xf, 0xf, true));          // row_ror:8
    x = max(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x124, 0xf, 0xf, true));          // row_ror:4
    x = max(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x122, 0xf, 0xf, true));          // row_ror:2
    x = max(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x121, 0xf, 0xf, true));          // row_ror:1: every lane of a row of 16 holds the row's
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1, 3
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)x, 63);
}

__global__ void __launch_bounds__(PC_THREADS) k_pc_cloud(PcCall c, const float* __restrict__ depth, const float* __restrict__ pose, int* list, int L, float* __restrict__ xyz,
                                                         int* __restrict__ index, int* __restrict__ count) {
    __shared__ float s_pose[PC_MAX_CAMS * PC_POSE_W];
    __shared__ float s_scale[PC_MAX_CAMS];
    __shared__ int s_cnt[PC_WAVES];
    __shared__ unsigned long long s_key[2][PC_WAVES];
    __shared__ float s_win[2][PC_WAVES][4];
    __shared__ int s_sel[PC_MAX_POINTS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, env = blockIdx.x;
    const int P = c.P, Q = c.ncam * c.H * c.W;
    depth += (size_t)env * Q;
    pose += (size_t)env * c.ncam * PC_POSE_W;
    list += (size_t)env * L;
    xyz += (size_t)env * P * 3;
    index += (size_t)env * P;
    count += (size_t)env * 2;
    PcView v;
    v.HW = c.H * c.W; v.W = c.W; v.hh = 0.5f * (float)c.H; v.hw = 0.5f * (float)c.W; v.max_depth = c.max_depth;
#pragma unroll
    for (int k = 0; k < 3; k++) { v.lo[k] = c.lo[k]; v.hi[k] = c.hi[k]; }
    if (tid < c.ncam * PC_POSE_W) s_pose[tid] = pose[tid];
    __syncthreads();
    if (tid < c.ncam) s_scale[tid] = (2.0f * s_pose[tid * PC_POSE_W + 12]) / (float)c.H;
    __syncthreads();

    // ---- 1. ordered compaction: counts, a scan, a scatter
    const int per = ((Q + PC_THREADS - 1) / PC_THREADS) * 64;
    const int p0 = wv * per, p1 = p0 + per < Q ? p0 + per : Q;
    int cnt = 0;
    for (int b = p0; b < p1; b += 64) {
        float wx, wy, wz;
        const int pix = b + lane;
        const bool ok = pix < p1 && pc_world(v, s_pose, s_scale, depth, pix, wx, wy, wz);
        cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    int base = 0, M = 0;
#pragma unroll
    for (int w = 0; w < PC_WAVES; w++) {
        const int n = s_cnt[w];
        if (w < wv) base += n;
        M += n;
    }
    const int Mp = M < PC_MAX_CANDIDATES ? M : PC_MAX_CANDIDATES;
    if (tid == 0) { count[0] = M; count[1] = Mp < P ? Mp : P; }
    if (M == 0) {          // (the same for every lane)
        for (int p = tid; p < P; p += PC_THREADS) { xyz[3 * p] = 0.0f; xyz[3 * p + 1] = 0.0f; xyz[3 * p + 2] = 0.0f; index[p] = -1; }
        return;
    }
    for (int b = p0; b < p1; b += 64) {
        float wx, wy, wz;
        const int pix = b + lane;
        const bool ok = pix < p1 && pc_world(v, s_pose, s_scale, depth, pix, wx, wy, wz);
        const unsigned long long mask = __ballot(ok);
        if (ok) {
            const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (M > PC_MAX_CANDIDATES) {
                const long long i = ((long long)pos * PC_MAX_CANDIDATES + M - 1) / M;
                if (i < PC_MAX_CANDIDATES && (i * M) / PC_MAX_CANDIDATES == pos) list[i] = pix;
            } else {
                list[pos] = pix;
            }
        }
        base += __popcll(mask);
    }
    __threadfence_block();
    __syncthreads();

    // ---- 2. farthest point sampling over the Mp listed candidates
    // (the trips are loaded by a ROLLED loop that shifts the four arrays down by one and puts the new trip last: trip t ends at index t, the
    // arrays are only ever indexed by constants, and the body -- two integer divisions -- exists once.  Unrolled it spilled 3.9 K registers.)
    float x[PC_TRIPS], y[PC_TRIPS], z[PC_TRIPS], md[PC_TRIPS];
#pragma unroll
    for (int j = 0; j < PC_TRIPS; j++) { x[j] = y[j] = z[j] = 0.0f; md[j] = -1.0f; }
#pragma nounroll
    for (int t = 0; t < PC_TRIPS; t++) {
        const int k = t * PC_THREADS + tid;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, nm = -1.0f;          // no candidate: never the arg-max
        if (k < Mp) {
            pc_world(v, s_pose, s_scale, depth, list[k], nx, ny, nz);
            nm = __builtin_inff();
        }
#pragma unroll
        for (int j = 0; j + 1 < PC_TRIPS; j++) { x[j] = x[j + 1]; y[j] = y[j + 1]; z[j] = z[j + 1]; md[j] = md[j + 1]; }
        x[PC_TRIPS - 1] = nx; y[PC_TRIPS - 1] = ny; z[PC_TRIPS - 1] = nz; md[PC_TRIPS - 1] = nm;
    }
    if (tid == 0) { s_win[0][0][0] = x[0]; s_win[0][0][1] = y[0]; s_win[0][0][2] = z[0]; s_sel[0] = 0; }
    __syncthreads();
    float sx = s_win[0][0][0], sy = s_win[0][0][1], sz = s_win[0][0][2];
    for (int p = 1; p < P; p++) {
        const int buf = p & 1;
        float bv = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
        int bp = 0;
#pragma unroll
        for (int j = 0; j < PC_TRIPS; j++) {
            if (j * PC_THREADS < Mp) {          // (the same for the whole workgroup)
                const float dx = x[j] - sx, dy = y[j] - sy, dz = z[j] - sz;
                const float m = fminf(md[j], (dx * dx + dy * dy) + dz * dz);
                md[j] = m;
                if (m > bv) { bv = m; bp = j * PC_THREADS + tid; bx = x[j]; by = y[j]; bz = z[j]; }          // ascending positions: the first of equals stays
            }
        }
        // the wave's arg-max in two reductions: the largest distance (its bits + 1; 0: the lane holds no candidate), then among the lanes that
        // hold it the lowest position (the largest complement)
        const unsigned hi_mine = bv < 0.0f ? 0u : __float_as_uint(bv) + 1u;
        const unsigned hi = wave_umax(hi_mine);
        const unsigned lo_mine = (hi_mine == hi && hi != 0u) ? ~(unsigned)bp : 0u;
        const unsigned lo = wave_umax(lo_mine);
        if (hi != 0u ? (hi_mine == hi && lo_mine == lo) : lane == 0) {          // the wave's winner (positions are distinct), or lane 0 of a wave without candidates
            s_key[buf][wv] = ((unsigned long long)hi << 32) | lo;
            s_win[buf][wv][0] = bx; s_win[buf][wv][1] = by; s_win[buf][wv][2] = bz;
        }
        __syncthreads();
        unsigned long long best = 0ull;
#pragma unroll
        for (int w = 0; w < PC_WAVES; w++) {
            const unsigned long long o = s_key[buf][w];
            best = o > best ? o : best;
        }
        unsigned pos = ~(unsigned)best;
        pos = pos < (unsigned)Mp ? pos : 0u;
        const int ww = (pos & (PC_THREADS - 1)) >> 6;
        sx = s_win[buf][ww][0]; sy = s_win[buf][ww][1]; sz = s_win[buf][ww][2];
        if (tid == 0) s_sel[p] = (int)pos;
        if ((unsigned)(best >> 32) <= 1u) {          // the largest distance is +0: every distance is, and candidate 0 wins from here on
            for (int q = p + 1 + tid; q < P; q += PC_THREADS) s_sel[q] = 0;
            break;
        }
    }
    __syncthreads();

    // ---- 3. the selections as points and pixels
    for (int p = tid; p < P; p += PC_THREADS) {
        const int pix = list[s_sel[p]];
        float wx, wy, wz;
        pc_world(v, s_pose, s_scale, depth, pix, wx, wy, wz);
        xyz[3 * p] = wx; xyz[3 * p + 1] = wy; xyz[3 * p + 2] = wz;
        index[p] = pix;
    }
}

int pointcloud_poses_launch(hipStream_t stream, const PcModel& m, const PcCall& c, int e0, int n, float* out, std::string& err) {
    hipLaunchKernelGGL(k_pc_poses, dim3((n * c.ncam + 255) / 256), dim3(256), 0, stream, m, c, e0, n, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("camera pose kernel: ") + hipGetErrorString(e); return -3; }
    return 0;
}

int pointcloud_launch(hipStream_t stream, const PcCall& c, int n, const float* depth, const float* pose, int* list, float* xyz, int* index, int* count, std::string& err) {
    hipLaunchKernelGGL(k_pc_cloud, dim3(n), dim3(PC_THREADS), 0, stream, c, depth, pose, list, (int)PcHost::list_len(c), xyz, index, count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("point cloud kernel: ") + hipGetErrorString(e); return -3; }
    return 0;
}

// ---- voxel grids (avsim_voxel_grid).  The caller's output [n][gx][gy][gz][8] is the accumulator: a cell's 32 bytes hold the u32
// words count, sum qx, sum qy, sum qz, sum r, sum g, sum b and a zero until k_vox_finish turns them into the eight float32 channels in place.
//   k_vox_clear    16-byte stores of zeros over the chunk's cells
//   k_vox_accum    a lane per pixel (a workgroup of 256 pixels of one env): pc_world, the cell and the position inside it in 1/256 per axis,
//       then no-return relaxed agent-scope integer adds into the cell's words -- 4 without a colour image, 7 with one.  MERGE: consecutive
//       lanes of the wave that hit the same cell form a run (neighbouring pixels of a row mostly see one surface); the run's values are summed
//       towards its first lane by a segmented shuffle scan -- three registers, two 16-bit sums each (a run's sum is at most 64 x 255), and
//       only as many steps as the wave's longest run needs -- and the first lane alone adds.  Integer sums: the result does not depend on
//       the form, nor on the order in which the adds arrive.
//   k_vox_finish   a lane per cell: reads its 32 bytes and, where count > 0, writes the eight floats (an empty cell's zeros are +0.0 already)
constexpr int VOX_THREADS = 256;

__global__ void __launch_bounds__(256) k_vox_clear(float4* __restrict__ out, size_t n4) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) out[i] = z;
}

__device__ __forceinline__ void vox_add(unsigned* p, unsigned v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool MERGE>
__global__ void __launch_bounds__(VOX_THREADS) k_vox_accum(VoxCall vc, const float* __restrict__ depth, const uint8_t* __restrict__ rgb, const float* __restrict__ pose,
                                                           unsigned* out) {
    __shared__ float s_pose[PC_MAX_CAMS * PC_POSE_W];
    __shared__ float s_scale[PC_MAX_CAMS];
    const PcCall& c = vc.pc;
    const int tid = threadIdx.x, lane = tid & 63, env = blockIdx.y;
    const int Q = c.ncam * c.H * c.W, gx = vc.g[0], gy = vc.g[1], gz = vc.g[2];
    depth += (size_t)env * Q;
    pose += (size_t)env * c.ncam * PC_POSE_W;
    out += (size_t)env * gx * gy * gz * VOX_CHANNELS;
    PcView v;
    v.HW = c.H * c.W; v.W = c.W; v.hh = 0.5f * (float)c.H; v.hw = 0.5f * (float)c.W; v.max_depth = c.max_depth;
#pragma unroll
    for (int k = 0; k < 3; k++) { v.lo[k] = c.lo[k]; v.hi[k] = c.hi[k]; }
    if (tid < c.ncam * PC_POSE_W) s_pose[tid] = pose[tid];
    __syncthreads();
    if (tid < c.ncam) s_scale[tid] = (2.0f * s_pose[tid * PC_POSE_W + 12]) / (float)c.H;
    __syncthreads();

    const int pix = blockIdx.x * VOX_THREADS + tid;
    float w[3];
    const bool ok = pix < Q && pc_world(v, s_pose, s_scale, depth, pix, w[0], w[1], w[2]);
    int cell = -1;
    unsigned q[3] = {0u, 0u, 0u}, col[3] = {0u, 0u, 0u};
    if (ok) {
        int ci[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float g = (float)vc.g[k], inv = g / (c.hi[k] - c.lo[k]);
            const float u = (w[k] - c.lo[k]) * inv;
            const float fi = fminf(floorf(u), g - 1.0f);
            const int qi = (int)((u - fi) * 256.0f);
            const int i = (int)fi;
            ci[k] = i < 0 ? 0 : i > vc.g[k] - 1 ? vc.g[k] - 1 : i;          // (0 <= fi <= g - 1 by the box; the clamp keeps the address inside whatever the floats)
            q[k] = (unsigned)(qi < 0 ? 0 : qi > 255 ? 255 : qi);
        }
        cell = (ci[0] * gy + ci[1]) * gz + ci[2];
        if (rgb) {
            const uint8_t* p = rgb + ((size_t)env * Q + pix) * 3;
            col[0] = p[0]; col[1] = p[1]; col[2] = p[2];
        }
    }
    unsigned cnt = 1u;
    bool add = ok;
    if (MERGE) {
        const int prev = __shfl_up(cell, 1);
        const bool head = lane == 0 || prev != cell;
        const unsigned long long heads = __ballot(head), rest = (heads >> lane) >> 1;
        const int after = rest ? __builtin_ctzll(rest) : 63 - lane;          // the lanes after this one in its run
        unsigned a = q[0] | (q[1] << 16), b = q[2] | (col[0] << 16), d = col[1] | (col[2] << 16);
        for (int s = 1; s < 64; s <<= 1) {
            if (__ballot(after >= s) == 0ull) break;          // (the same for the wave) no run reaches further
            const unsigned ta = __shfl_down(a, s), tb = __shfl_down(b, s), td = __shfl_down(d, s);
            if (after >= s) { a += ta; b += tb; d += td; }          // after step s a lane holds the sum of itself and the next 2 s - 1 lanes of its run
        }
        q[0] = a & 0xffffu; q[1] = a >> 16; q[2] = b & 0xffffu; col[0] = b >> 16; col[1] = d & 0xffffu; col[2] = d >> 16;
        cnt = (unsigned)after + 1u;
        add = ok && head;
    }
    if (add) {
        unsigned* o = out + (size_t)cell * VOX_CHANNELS;
        vox_add(o, cnt);
        vox_add(o + 1, q[0]); vox_add(o + 2, q[1]); vox_add(o + 3, q[2]);
        if (rgb) { vox_add(o + 4, col[0]); vox_add(o + 5, col[1]); vox_add(o + 6, col[2]); }
    }
}

__global__ void __launch_bounds__(256) k_vox_finish(VoxCall vc, size_t total, float* out) {
    const PcCall& c = vc.pc;
    const int gy = vc.g[1], gz = vc.g[2], cells = vc.g[0] * gy * gz;
    float size[3];
#pragma unroll
    for (int k = 0; k < 3; k++) size[k] = (c.hi[k] - c.lo[k]) / (float)vc.g[k];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const uint4 a = ((const uint4*)out)[2 * i], b = ((const uint4*)out)[2 * i + 1];
        if (a.x == 0u) continue;
        const int cell = (int)(i % (size_t)cells), iz = cell % gz, t = cell / gz, iy = t % gy, ix = t / gy;
        const float n = (float)a.x;
        float4 p, s;
        p.x = c.lo[0] + ((float)ix + ((float)a.y / n + 0.5f) * 0.00390625f) * size[0];
        p.y = c.lo[1] + ((float)iy + ((float)a.z / n + 0.5f) * 0.00390625f) * size[1];
        p.z = c.lo[2] + ((float)iz + ((float)a.w / n + 0.5f) * 0.00390625f) * size[2];
        p.w = ((float)b.x / n) * (1.0f / 255.0f);
        s.x = ((float)b.y / n) * (1.0f / 255.0f);
        s.y = ((float)b.z / n) * (1.0f / 255.0f);
        s.z = n;
        s.w = 1.0f;
        ((float4*)out)[2 * i] = p;
        ((float4*)out)[2 * i + 1] = s;
    }
}

int voxel_launch(hipStream_t stream, const VoxCall& c, int n, const float* depth, const uint8_t* rgb, const float* pose, float* out, bool merge, std::string& err) {
    const size_t total = (size_t)n * c.g[0] * c.g[1] * c.g[2], blocks = (total + 255) / 256;
    const int Q = c.pc.ncam * c.pc.H * c.pc.W;
    const dim3 sweep((unsigned)(blocks < 65536 ? blocks : 65536)), pixels((Q + VOX_THREADS - 1) / VOX_THREADS, n);
    hipLaunchKernelGGL(k_vox_clear, sweep, dim3(256), 0, stream, (float4*)out, total * 2);
    if (merge) hipLaunchKernelGGL(k_vox_accum<true>, pixels, dim3(VOX_THREADS), 0, stream, c, depth, rgb, pose, (unsigned*)out);
    else hipLaunchKernelGGL(k_vox_accum<false>, pixels, dim3(VOX_THREADS), 0, stream, c, depth, rgb, pose, (unsigned*)out);
    hipLaunchKernelGGL(k_vox_finish, sweep, dim3(256), 0, stream, c, total, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("voxel grid kernels: ") + hipGetErrorString(e); return -3; }
    return 0;
}

// ---- virtual orthographic views (avsim_virtual_views).  The caller's output [n][V][VH][VW][8] is the z-buffer: the first 8 of a
// virtual pixel's 32 bytes hold its key, (bits of dist << 32) | source slot, until k_vv_finish turns the pixel into its eight float32 channels.
//   k_vv_clear     one 16-byte store of ones per virtual pixel: the key of a pixel nothing covers (no candidate has it: a dist is no NaN)
//   k_vv_scatter   a lane per source pixel (a workgroup of 256 pixels of one env): pc_world once, the four pixel coordinates the six views choose
//       from (x and y along VW, y and z along VH), then per view the key and a relaxed agent-scope 64-bit atomic MINIMUM into every pixel of the
//       footprint that lies inside the image -- one global_atomic_umin_x2 without return each, no compare-and-swap loop.  CHECK: a relaxed load
//       of the pixel's key first, and no atomic when the lane's own is not smaller; keys only decrease, so a stale read is safe.  The loads go
//       out in batches -- with radius 0 those of all views, BEFORE the runs merge, otherwise three pixels of a footprint row -- so that a lane waits once per batch.  MERGE:
//       consecutive lanes of the wave on the same virtual pixel form a run, a segmented shuffle scan takes the run's minimum towards its first
//       lane, and that lane alone issues the footprint.  A minimum depends neither on the form nor on the order of arrival.
//   k_vv_finish    a lane per virtual pixel (a workgroup of 256 of one env): reads the key, recomputes the winner's world point from its slot
//       with pc_world (the same function, the same bits), reads its colour and writes the eight floats and the index
constexpr int VV_THREADS = 256;

__global__ void __launch_bounds__(256) k_vv_clear(uint4* __restrict__ out, size_t npix) {
    const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) out[2 * i] = ones;
}

// the pixel of coordinate w on an image axis of n pixels over [lo, hi]: the voxel grid's cell formula (the clamp keeps the address inside whatever the floats)
__device__ __forceinline__ int vv_pixel(float w, float lo, float hi, int n) {
    const float g = (float)n, inv = g / (hi - lo);
    const float u = (w - lo) * inv;
    const int i = (int)fminf(floorf(u), g - 1.0f);
    return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}

// what a lane brings to every view
struct VvLane {
    float w[3];
    int cx, cy, ry, rz;          // x, y as columns (of VW), y, z as rows (of VH), ascending
    int pix, lane;
    bool ok;
};

// the lane's key and virtual pixel in view iv, whether it is a candidate or not
__device__ __forceinline__ void vv_place(const VvCall& vc, const VvLane& l, int iv, unsigned long long& key, int& pr, int& pc) {
    const PcCall& c = vc.pc;
    const int VH = vc.VH, VW = vc.VW;
    float dist;
    switch (vc.view[iv]) {          // (the same for the whole grid)
        case 0: dist = c.hi[0] - l.w[0]; pc = l.cy; pr = VH - 1 - l.rz; break;
        case 1: dist = l.w[0] - c.lo[0]; pc = VW - 1 - l.cy; pr = VH - 1 - l.rz; break;
        case 2: dist = c.hi[1] - l.w[1]; pc = VW - 1 - l.cx; pr = VH - 1 - l.rz; break;
        case 3: dist = l.w[1] - c.lo[1]; pc = l.cx; pr = VH - 1 - l.rz; break;
        case 4: dist = c.hi[2] - l.w[2]; pc = l.cx; pr = VH - 1 - l.ry; break;
        default: dist = l.w[2] - c.lo[2]; pc = l.cx; pr = l.ry; break;
    }
    key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)l.pix;
}

// whether the lane issues.  MERGE: the run of consecutive lanes on the lane's virtual pixel takes its minimum towards its first lane, which alone issues
template <bool MERGE>
__device__ __forceinline__ bool vv_issues(const VvCall& vc, const VvLane& l, unsigned long long& key, int pr, int pc) {
    if (!MERGE) return l.ok;
    const int target = l.ok ? pr * vc.VW + pc : -1;
    const int prev = __shfl_up(target, 1);
    const bool head = l.lane == 0 || prev != target;
    const unsigned long long heads = __ballot(head), rest = (heads >> l.lane) >> 1;
    const int after = rest ? __builtin_ctzll(rest) : 63 - l.lane;          // the lanes after this one in its run
    for (int s = 1; s < 64; s <<= 1) {
        if (__ballot(after >= s) == 0ull) break;          // (the same for the wave) no run reaches further
        const unsigned long long t = __shfl_down(key, s);
        if (after >= s && t < key) key = t;          // after step s a lane holds the minimum of itself and the next 2 s - 1 lanes of its run
    }
    return l.ok && head;
}

__device__ __forceinline__ unsigned long long vv_load(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vv_min(unsigned long long* p, unsigned long long key) { (void)__hip_atomic_fetch_min(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool CHECK, bool MERGE>
__global__ void __launch_bounds__(VV_THREADS) k_vv_scatter(VvCall vc, const float* __restrict__ depth, const float* __restrict__ pose, unsigned long long* out) {
    __shared__ float s_pose[PC_MAX_CAMS * PC_POSE_W];
    __shared__ float s_scale[PC_MAX_CAMS];
    const PcCall& c = vc.pc;
    const int tid = threadIdx.x, env = blockIdx.y;
    const int Q = c.ncam * c.H * c.W, VH = vc.VH, VW = vc.VW, R = vc.radius;
    depth += (size_t)env * Q;
    pose += (size_t)env * c.ncam * PC_POSE_W;
    out += (size_t)env * vc.nviews * VH * VW * 4;
    PcView v;
    v.HW = c.H * c.W; v.W = c.W; v.hh = 0.5f * (float)c.H; v.hw = 0.5f * (float)c.W; v.max_depth = c.max_depth;
#pragma unroll
    for (int k = 0; k < 3; k++) { v.lo[k] = c.lo[k]; v.hi[k] = c.hi[k]; }
    if (tid < c.ncam * PC_POSE_W) s_pose[tid] = pose[tid];
    __syncthreads();
    if (tid < c.ncam) s_scale[tid] = (2.0f * s_pose[tid * PC_POSE_W + 12]) / (float)c.H;
    __syncthreads();

    VvLane l;
    l.pix = blockIdx.x * VV_THREADS + tid;
    l.lane = tid & 63;
    l.w[0] = l.w[1] = l.w[2] = 0.0f;
    l.ok = l.pix < Q && pc_world(v, s_pose, s_scale, depth, l.pix, l.w[0], l.w[1], l.w[2]);
    if (!MERGE && !l.ok) return;
    l.cx = l.cy = l.ry = l.rz = 0;
    if (l.ok) {
        l.cx = vv_pixel(l.w[0], c.lo[0], c.hi[0], VW);
        l.cy = vv_pixel(l.w[1], c.lo[1], c.hi[1], VW);
        l.ry = vv_pixel(l.w[1], c.lo[1], c.hi[1], VH);
        l.rz = vv_pixel(l.w[2], c.lo[2], c.hi[2], VH);
    }
    const size_t view_words = (size_t)VH * VW * 4;
    if (CHECK && R == 0) {          // one pixel per view: the loads of all views go out together and travel while the runs merge; then the atomics that are left
        unsigned long long key[VV_MAX_VIEWS], cur[VV_MAX_VIEWS];
        size_t at[VV_MAX_VIEWS];          // (offsets, not pointers: the accesses stay global ones)
        int pr[VV_MAX_VIEWS], pc[VV_MAX_VIEWS];
#pragma unroll
        for (int iv = 0; iv < VV_MAX_VIEWS; iv++) {
            key[iv] = 0ull;
            at[iv] = 0;          // (a lane that is no candidate loads a word of the buffer all the same: no branch round the load)
            pr[iv] = pc[iv] = 0;
            if (iv < vc.nviews) {
                vv_place(vc, l, iv, key[iv], pr[iv], pc[iv]);
                if (l.ok) at[iv] = iv * view_words + (size_t)(pr[iv] * VW + pc[iv]) * 4;
            }
        }
#pragma unroll
        for (int iv = 0; iv < VV_MAX_VIEWS; iv++) cur[iv] = iv < vc.nviews ? vv_load(out + at[iv]) : 0ull;
#pragma unroll
        for (int iv = 0; iv < VV_MAX_VIEWS; iv++)
            if (iv < vc.nviews) {
                const bool go = vv_issues<MERGE>(vc, l, key[iv], pr[iv], pc[iv]);
                if (go && key[iv] < cur[iv]) vv_min(out + at[iv], key[iv]);
            }
        return;
    }
    for (int iv = 0; iv < vc.nviews; iv++, out += view_words) {
        unsigned long long key;
        int pr, pc;
        vv_place(vc, l, iv, key, pr, pc);
        if (!vv_issues<MERGE>(vc, l, key, pr, pc)) continue;
        const int r0 = pr - R < 0 ? 0 : pr - R, r1 = pr + R > VH - 1 ? VH - 1 : pr + R;
        const int c0 = pc - R < 0 ? 0 : pc - R, c1 = pc + R > VW - 1 ? VW - 1 : pc + R;
        for (int r = r0; r <= r1; r++) {
            unsigned long long* row = out + (size_t)r * VW * 4;
            if (CHECK) {          // three pixels of the row at a time: their loads together, then the atomics that are left
                for (int q = c0; q <= c1; q += 3) {
                    const int q1 = q + 1 <= c1 ? q + 1 : q, q2 = q + 2 <= c1 ? q + 2 : q;
                    const unsigned long long a0 = vv_load(row + (size_t)q * 4), a1 = vv_load(row + (size_t)q1 * 4), a2 = vv_load(row + (size_t)q2 * 4);
                    if (key < a0) vv_min(row + (size_t)q * 4, key);
                    if (q1 != q && key < a1) vv_min(row + (size_t)q1 * 4, key);
                    if (q2 != q && key < a2) vv_min(row + (size_t)q2 * 4, key);
                }
            } else {
                for (int q = c0; q <= c1; q++) vv_min(row + (size_t)q * 4, key);
            }
        }
    }
}

__global__ void __launch_bounds__(VV_THREADS) k_vv_finish(VvCall vc, const float* __restrict__ depth, const uint8_t* __restrict__ rgb, const float* __restrict__ pose, float* out,
                                                          int32_t* __restrict__ index) {
    __shared__ float s_pose[PC_MAX_CAMS * PC_POSE_W];
    __shared__ float s_scale[PC_MAX_CAMS];
    const PcCall& c = vc.pc;
    const int tid = threadIdx.x, env = blockIdx.y;
    const int Q = c.ncam * c.H * c.W, VP = vc.nviews * vc.VH * vc.VW;
    depth += (size_t)env * Q;
    pose += (size_t)env * c.ncam * PC_POSE_W;
    PcView v;
    v.HW = c.H * c.W; v.W = c.W; v.hh = 0.5f * (float)c.H; v.hw = 0.5f * (float)c.W; v.max_depth = c.max_depth;
#pragma unroll
    for (int k = 0; k < 3; k++) { v.lo[k] = c.lo[k]; v.hi[k] = c.hi[k]; }
    if (tid < c.ncam * PC_POSE_W) s_pose[tid] = pose[tid];
    __syncthreads();
    if (tid < c.ncam) s_scale[tid] = (2.0f * s_pose[tid * PC_POSE_W + 12]) / (float)c.H;
    __syncthreads();

    const int i = blockIdx.x * VV_THREADS + tid;
    if (i >= VP) return;
    const size_t at = (size_t)env * VP + i;
    const uint2 key = ((const uint2*)out)[4 * at];          // x: the slot, y: the bits of dist
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    int slot = -1;
    if (key.x < (unsigned)Q && key.y != ~0u) {          // (a written key's slot is below Q: the test keeps the reads inside whatever the buffer held)
        slot = (int)key.x;
        pc_world(v, s_pose, s_scale, depth, slot, b.x, b.y, b.z);
        if (rgb) {
            const uint8_t* p = rgb + ((size_t)env * Q + slot) * 3;
            a.x = (float)p[0] * (1.0f / 255.0f); a.y = (float)p[1] * (1.0f / 255.0f); a.z = (float)p[2] * (1.0f / 255.0f);
        }
        a.w = __uint_as_float(key.y);
        b.w = 1.0f;
    }
    ((float4*)out)[2 * at] = a;
    ((float4*)out)[2 * at + 1] = b;
    index[at] = slot;
}

int virtviews_launch(hipStream_t stream, const VvCall& c, int n, const float* depth, const uint8_t* rgb, const float* pose, float* out, int32_t* index, int form, std::string& err) {
    const int VP = c.nviews * c.VH * c.VW, Q = c.pc.ncam * c.pc.H * c.pc.W;
    const size_t total = (size_t)n * VP, blocks = (total + 255) / 256;
    const dim3 sweep((unsigned)(blocks < 65536 ? blocks : 65536)), pixels((Q + VV_THREADS - 1) / VV_THREADS, n), vpixels((VP + VV_THREADS - 1) / VV_THREADS, n);
    unsigned long long* keys = (unsigned long long*)out;
    hipLaunchKernelGGL(k_vv_clear, sweep, dim3(256), 0, stream, (uint4*)out, total);
    switch (vv_form(form, c)) {
        case 0: hipLaunchKernelGGL((k_vv_scatter<false, false>), pixels, dim3(VV_THREADS), 0, stream, c, depth, pose, keys); break;
        case 1: hipLaunchKernelGGL((k_vv_scatter<true, false>), pixels, dim3(VV_THREADS), 0, stream, c, depth, pose, keys); break;
        case 2: hipLaunchKernelGGL((k_vv_scatter<false, true>), pixels, dim3(VV_THREADS), 0, stream, c, depth, pose, keys); break;
        default: hipLaunchKernelGGL((k_vv_scatter<true, true>), pixels, dim3(VV_THREADS), 0, stream, c, depth, pose, keys); break;
    }
    hipLaunchKernelGGL(k_vv_finish, vpixels, dim3(VV_THREADS), 0, stream, c, depth, rgb, pose, out, index);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("virtual view kernels: ") + hipGetErrorString(e); return -3; }
    return 0;
}

}  // namespace avs

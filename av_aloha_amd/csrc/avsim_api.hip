// avsim_api.hip -- the C-ABI of libavsim.so (include/avsim.h) and the kernel launches behind it.
// gfx950 only; there is no CPU path in this library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/avsim.h"
#include "avsim_chunks.hip.h"
#include "avsim_compose.hip.h"
#include "avsim_imgprep.hip.h"
#include "avsim_obshist.hip.h"
#include "avsim_imgaug.hip.h"
#include "avsim_imgresize.hip.h"
#include "avsim_pointcloud.hip.h"
#include "avsim_episode.hip.h"
#include "avsim_ik.hip.h"
#include "avsim_io.h"
#include "avsim_jpeg.hip.h"
#include "avsim_model.h"
#include "avsim_phys.hip.h"
#include "avsim_render.hip.h"
#include "avsim_vis.hip.h"

using namespace avs;

static thread_local std::string g_create_error;

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (h)->set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return AVSIM_EHIP;                                                                       \
        }                                                                                            \
    } while (0)

// Every entry point runs on the handle's device and puts the caller's current device back on return (a torch process keeps
// its own current device; one process per GPU is the intended deployment, several handles per process still work).
struct DevGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;      // a failed switch is an error of the entry point (AVS_ON_DEVICE), never a silent run on the caller's device
    explicit DevGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DevGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define AVS_ON_DEVICE(h)                                                                                          \
    DevGuard dev_guard_((h)->device);                                                                       \
    if (dev_guard_.err != hipSuccess) {                                                                     \
        (h)->set_error("hipSetDevice(%d) failed: %s", (h)->device, hipGetErrorString(dev_guard_.err));      \
        return AVSIM_EHIP;                                                                                  \
    }

// Device memory belongs to members that release it themselves (avsim_dev.h).  avsim_destroy synchronises the stream, deletes the handle -- which
// frees all of it -- and destroys the stream last
struct avsim {
    int device = 0;
    uint32_t flags = 0;
    int N = 0;
    bool io_device = false, f64 = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[16] = {};
    std::string err;
    // model
    int nq = 0, nv = 0, nu = 0, nj = 0, nobj = 0, task_id = 0, num_arms = 3, max_reward = 0;
    IkParams ik;
    std::vector<int> obj_qadr, obs_qadr;
    std::vector<double> qpos_home, ctrl_home;
    PhysHost phys;  // device model image + launch configuration (avsim_phys.hip.h)
    RenderHost render;   // depth renderer (avsim_render.hip.h)
    VisHost vis;         // colour images of the visual meshes (avsim_vis.hip.h), once avsim_load_visual has run
    JpegHost jpeg;       // JPEG streams of such images (avsim_jpeg.hip.h): tables per shape, the intervals' staging area
    JpegDecHost jpegdec; // and those streams back into images: Huffman lookup tables, the coefficients' staging area
    ComposeHost compose; // views resampled into a canvas, labels (avsim_compose.hip.h): coefficient tables per size pair, the validated placements
    StageRing stage;     // the pinned staging of a call's host arrays (avsim_stage.h): avsim_image_prep's, avsim_image_jitter's, avsim_image_augment's and avsim_image_resize's
    ImgAugHost imgaug;   // colour, sharpness and affine augmentation (avsim_imgaug.hip.h): the gray sums behind contrast, the scratch images of sharpness + affine
    ChunkHost chunks;    // per-env execution of action chunks (avsim_chunks.hip.h), once avsim_chunk_setup has run
    ObsHistHost obshist; // per-env observation histories (avsim_obshist.hip.h), once avsim_obs_history_setup has run
    PcHost pointcloud;   // point clouds from depth images (avsim_pointcloud.hip.h): a chunk of envs' pose records and candidate lists
    int virtviews_form = 0;          // option "virtviews_form": 0 = avsim_virtual_views runs the scatter form AVSIM_VV_FORM, f + 1 = form f (the same bits; there to be measured)
    bool labels_unpacked = false;    // option "render_labels_form": avsim_render_labels keeps a lane's eight winners in eight registers (1) instead of two (0, the default); the same images, there to be measured
    bool voxel_other_form = false;   // option "voxel_other_form": avsim_voxel_grid runs the accumulate form that AVSIM_VOXEL_MERGE did NOT pick (the same bits; there to be measured)
    bool jpegdec_events = false;   // option "jpeg_decode_events": avsim_jpeg_decode records ev[12..15] around its three kernels
    // the state's version: bumped by everything that writes qpos (reset, the steps, set_state); the image calls skip their pose pass and the shadow
    // map when they already hold this version's (a facade that fetches its cameras one call at a time repeats neither)
    unsigned long long state_ver = 1, xpose_ver = 0;
    bool render_proxies = false;   // option "render_proxies": avsim_render_rgb draws the collision proxies even with a visual scene loaded
    // device state (real = float, or double with AVSIM_F64_PHYSICS)
    DevArena state;
    void *d_qpos = nullptr, *d_qvel = nullptr, *d_ctrl = nullptr, *d_warm = nullptr;
    int* d_latch = nullptr;
    IoPool io;           // device copies of the arrays of a host caller, a call's scratch (avsim_io.h)
    // per-env episodes (avsim_episode_setup; avsim_episode.hip.h): parameters, per-env bookkeeping, records, outputs nobody asked for
    bool ep_ready = false;
    EpArgs ep{};
    DevArena ep_arena;
    double* ep_ap = nullptr;
    int *ep_rw = nullptr, *ep_el = nullptr;
    uint8_t *ep_su = nullptr, *ep_te = nullptr, *ep_tr = nullptr;
    int64_t* ep_id = nullptr;
    // kernel timing: pairs of HIP events recorded around every physics launch on the launch stream, read
    // back (and only then synchronised) by avsim_kernel_time
    bool ktiming = false;
    EventTimer ktimer;

    void set_error(const char* fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
    }
    size_t rsz() const { return f64 ? 8 : 4; }
};

// The arrays of one entry point (avsim_io.h), with the library's return codes: built after AVS_ON_DEVICE, asked once before the launch
// (`if (io.failed()) return AVSIM_EHIP;`), and `return io.done();` last -- in host I/O mode that copies the outputs back and synchronises
static_assert(IoPool::NBUF >= 4 + 2 * OBH_MAX_CAMS, "avsim_obs_history_push stages four arrays and two per camera");
struct Call : IoCall {
    explicit Call(avsim* h) : Call(h, h->io_device) {}
    Call(avsim* h, bool device_mode) : IoCall(h->io, h->stream, device_mode, h->err) {}
    int done() { return finish() == hipSuccess ? AVSIM_OK : AVSIM_EHIP; }
};

// ------------------------------------------------------------------------------------------------
// IK kernels: one problem per lane; blockIdx.y selects the arm so a wave never mixes 6- and 7-DoF code
// ------------------------------------------------------------------------------------------------
template <int NJ>
__global__ void __launch_bounds__(64) k_fk_jac(IkParams P, int arm, int n, const double* __restrict__ q, double* __restrict__ Tout,
                                               double* __restrict__ Jout) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double th[NJ];
#pragma unroll
    for (int k = 0; k < NJ; k++) th[k] = q[(size_t)i * NJ + k];
    if (Tout) {
        double R[9], p[3];
        fk<double, NJ>(P.arm[arm], th, R, p);
        double* T = Tout + (size_t)i * 16;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) T[4 * r + c] = R[3 * r + c];
            T[4 * r + 3] = p[r];
        }
        T[12] = T[13] = T[14] = 0;
        T[15] = 1;
    }
    if (Jout) {
        double J[6][NJ];
        jac<double, NJ>(P.arm[arm], th, J);
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int k = 0; k < NJ; k++) Jout[((size_t)i * 6 + r) * NJ + k] = J[r][k];
    }
}

// avsim_ik's GradIK: one problem per 16-lane row (gradik spreads its cost evaluations over the row), four per block.  (Its DiffIK: k_cart_ctrl.)
__global__ void __launch_bounds__(64) k_ik(IkParams P, int arm, int iters, int n, const double* __restrict__ q,
                                           const double* __restrict__ pos, const double* __restrict__ quat,
                                           double* __restrict__ qout) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool live = i < n;
    const int ii = live ? i : n - 1;          // idle rows of the last block shadow the last problem (wave-wide shuffles inside gradik)
    double th[6], out[6], tp[3], qx[4], Rt[9];
#pragma unroll
    for (int k = 0; k < 6; k++) th[k] = q[(size_t)ii * 6 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) tp[k] = pos[(size_t)ii * 3 + k];
    qx[0] = quat[(size_t)ii * 4 + 1]; qx[1] = quat[(size_t)ii * 4 + 2]; qx[2] = quat[(size_t)ii * 4 + 3];
    qx[3] = quat[(size_t)ii * 4 + 0];  // wxyz_to_xyzw (diff_ik.py:59)
    quat2mat_xyzw(qx, Rt);
    gradik<double>(P, arm, th, tp, Rt, iters, out);
    if (!live || (threadIdx.x & 15) != 0) return;
#pragma unroll
    for (int k = 0; k < 6; k++) qout[(size_t)i * 6 + k] = out[k];
}

// sim_env.py:277-301: Cartesian action -> ctrl, IK seeded with the MEASURED qpos
// The GradIK arms of the reference mode in a kernel of their own, one env per 16-lane row, gradik inlined: as an out-of-line function
// next to the DiffIK code it spilled 3.3 KB per lane at 512 registers.  (Capped at 256 registers for two waves per SIMD it is no
// faster: 50 iterations x 3 rounds of f64 forward kinematics are VALU-bound, not latency-bound.)
template <typename real>
__global__ void __launch_bounds__(64) k_gradik_ctrl(IkParams P, int N, int nq, int nu, const double* __restrict__ act,
                                                                                          const real* __restrict__ qpos, real* __restrict__ ctrl) {
    const int arm = blockIdx.y;
    const int i0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool live = i0 < N;
    const int i = live ? i0 : N - 1;
    const double* a = act + (size_t)i * 23 + (arm == 0 ? 0 : 8);
    double tp[3] = {a[0], a[1], a[2]}, qx[4] = {a[4], a[5], a[6], a[3]}, Rt[9];
    quat2mat_xyzw(qx, Rt);
    const real* qp = qpos + (size_t)i * nq;
    real* c = ctrl + (size_t)i * nu + (arm == 0 ? 0 : 7);
    const IkArm& A = P.arm[arm];
    double th[6], out[6];
#pragma unroll
    for (int k = 0; k < 6; k++) th[k] = (double)qp[A.qadr[k]];
    gradik<double>(P, arm, th, tp, Rt, P.grad_iters, out);
    if (!live || (threadIdx.x & 15) != 0) return;
#pragma unroll
    for (int k = 0; k < 6; k++) c[k] = (real)out[k];
    const double trig = a[7];  // sim_env.py:300-301: unnorm(1 - trigger)
    c[6] = (real)((1.0 - trig) * (P.grip_hi - P.grip_lo) + P.grip_lo);
}

// DiffIK, one problem per lane, blockIdx.y + arm0 = arm: THE kernel behind avsim_step_cartesian (the DLS mode's three arms, the reference
// mode's camera arm) and behind avsim_ik's DiffIK.  One compiled body, so that the control path and the stand-alone call answer a problem
// with the same bits: this unit fuses multiply-adds where the compiler sees fit, and it chose differently in two kernels' inlined copies of
// diffik<double, 7> (tests/test_gpu_ik_batch.py measured up to 4.5e-11 between ctrl and avsim_ik).  So the addressing and the two real
// types are arguments here, not template parameters.
struct DiffIkIo {
    const void* q;            // joints: a row per problem, float (q_f32) or double, q_stride entries long; q_adr: the arm's joints
    int q_f32, q_stride, q_adr;          // stand at IkArm::qadr in it (a qpos row), else the row is the joint vector
    const double *pos, *quat, *trig;     // targets: pos[3], quat wxyz[4], trigger (null: no gripper) of problem i, arm y at
    int pos_stride, quat_stride, arm_stride;        // i * stride + y * arm_stride (y = blockIdx.y)
    void* out;                // answers: float (out_f32) or double, problem i, arm y at i * out_stride + y * out_arm_stride
    int out_f32, out_stride, out_arm_stride;
};
__global__ void __launch_bounds__(64) k_cart_ctrl(IkParams P, int arm0, int iters, int N, DiffIkIo io) {
    const int arm = blockIdx.y + arm0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const size_t ay = (size_t)blockIdx.y * io.arm_stride;
    const double* ap = io.pos + (size_t)i * io.pos_stride + ay;
    const double* aq = io.quat + (size_t)i * io.quat_stride + ay;
    double tp[3] = {ap[0], ap[1], ap[2]}, qx[4] = {aq[1], aq[2], aq[3], aq[0]}, Rt[9];      // wxyz_to_xyzw (diff_ik.py:59)
    quat2mat_xyzw(qx, Rt);
    const IkArm& A = P.arm[arm];
    const size_t qo = (size_t)i * io.q_stride, oo = (size_t)i * io.out_stride + (size_t)blockIdx.y * io.out_arm_stride;
    auto load = [&](int k) -> double {
        const size_t j = qo + (io.q_adr ? A.qadr[k] : k);
        return io.q_f32 ? (double)((const float*)io.q)[j] : ((const double*)io.q)[j];
    };
    auto store = [&](int k, double v) {
        if (io.out_f32) ((float*)io.out)[oo + k] = (float)v;
        else ((double*)io.out)[oo + k] = v;
    };
    if (arm == 2) {
        double th[7], out[7];
#pragma unroll
        for (int k = 0; k < 7; k++) th[k] = load(k);
        diffik<double, 7>(P, 2, th, tp, Rt, iters, out);
#pragma unroll
        for (int k = 0; k < 7; k++) store(k, out[k]);
    } else {
        double th[6], out[6];
#pragma unroll
        for (int k = 0; k < 6; k++) th[k] = load(k);
        diffik<double, 6>(P, arm, th, tp, Rt, iters, out);       // (the GradIK arms of the reference mode: k_gradik_ctrl)
#pragma unroll
        for (int k = 0; k < 6; k++) store(k, out[k]);
        if (io.trig) {
            const double trig = io.trig[(size_t)i * io.pos_stride + ay];  // sim_env.py:300-301: unnorm(1 - trigger)
            store(6, (1.0 - trig) * (P.grip_hi - P.grip_lo) + P.grip_lo);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// small state kernels
// ------------------------------------------------------------------------------------------------
template <typename real>
__global__ void k_reset(int N, int nq, int nv, int nu, int nobj, const unsigned char* __restrict__ mask,
                        const double* __restrict__ obj, const double* __restrict__ qhome, const double* __restrict__ chome,
                        const int* __restrict__ objadr, real* qpos, real* qvel, real* ctrl, real* warm, int* latch, double* obj_keep) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (mask && !mask[i]) return;
    reset_env<real>(i, nq, nv, nu, nobj, obj + (size_t)i * nobj * 7, qhome, chome, objadr, qpos, qvel, ctrl, warm, latch, obj_keep);      // (avsim_episode.hip.h)
}

template <typename A, typename B>
__global__ void k_convert(size_t n, const A* __restrict__ a, B* __restrict__ b) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = (B)a[i];
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
static int reset_from(avsim_t* h, bool device_mode, const uint8_t* mask, const double* obj_qpos);

extern "C" {

const char* avsim_last_error(const avsim_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static void fill_ik(const Blob& b, IkParams& P) {
    std::memset(&P, 0, sizeof P);
    auto n = b.i("ik_n");
    auto w0 = b.f("ik_w0"), p0 = b.f("ik_p0"), s0 = b.f("ik_site0"), rg = b.f("ik_range");
    auto qa = b.i("ik_qadr");
    auto home = b.f("qpos_home");
    for (int a = 0; a < 3; a++) {
        IkArm& A = P.arm[a];
        A.n = n[a];
        for (int i = 0; i < 7; i++) {
            const double* w = &w0[(a * 7 + i) * 3];
            const double* p = &p0[(a * 7 + i) * 3];
            for (int k = 0; k < 3; k++) A.w[i][k] = w[k];
            // kinematics.py:12  v0 = -cross(w0, p0)
            A.v[i][0] = -(w[1] * p[2] - w[2] * p[1]);
            A.v[i][1] = -(w[2] * p[0] - w[0] * p[2]);
            A.v[i][2] = -(w[0] * p[1] - w[1] * p[0]);
            A.lo[i] = rg[(a * 7 + i) * 2];
            A.hi[i] = rg[(a * 7 + i) * 2 + 1];
            A.qadr[i] = qa[a * 7 + i];
        }
        for (int k = 0; k < 12; k++) A.site0[k] = s0[a * 16 + k];
    }
    // DiffIK parameters: sim_env.py:125-138 (middle arm); manipulators reuse the gains with q0 = home pose
    P.k_pos = 0.9; P.k_ori = 0.9; P.damping = 1.0e-4; P.max_angvel = 3.14; P.dt = 0.04; P.diff_iters = 10;
    const double kn[7] = {10.0, 10.0, 10.0, 10.0, 5.0, 5.0, 5.0};
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < P.arm[a].n; i++) {
            P.k_null[a][i] = kn[i];
            P.q0[a][i] = home[P.arm[a].qadr[i]];
        }
    // GradIK parameters: sim_env.py:89-122
    P.g_step = 1e-4; P.g_min_delta = 1e-12; P.grad_iters = 50; P.g_pw = 500.0; P.g_rw = 100.0;
    P.g_pthr = 1e-3; P.g_rthr = 1e-3; P.g_maxp = 0.1; P.g_maxr = 0.3; P.g_joint_p = 0.9;
    const double jc[6] = {10.0, 10.0, 1.0, 50.0, 1.0, 1.0};
    for (int i = 0; i < 6; i++) { P.g_jcw[i] = jc[i]; P.g_jdw[i] = 50.0; }
    auto gr = b.f("grip_range");
    P.grip_lo = gr[0];
    P.grip_hi = gr[1];
}

int avsim_create(const void* blob, size_t nbytes, int num_envs, int device, uint32_t flags, avsim_t** out) {
    if (!out) return AVSIM_EINVAL;
    *out = nullptr;
    if (!blob || num_envs <= 0) { g_create_error = "avsim_create: bad arguments"; return AVSIM_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_create_error = "avsim_create: no usable HIP device (this library has no CPU path)";
        return AVSIM_ENODEV;
    }
    std::unique_ptr<avsim> h(new avsim);
    h->device = device;
    h->flags = flags;
    h->N = num_envs;
    h->io_device = flags & AVSIM_IO_DEVICE;
    h->f64 = flags & AVSIM_F64_PHYSICS;
    DevGuard dev_guard_(device);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return AVSIM_EHIP; }
    try {
        Blob b(blob, nbytes);
        h->nq = b.scalar("nq"); h->nv = b.scalar("nv"); h->nu = b.scalar("nu");
        h->task_id = b.scalar("task_id"); h->num_arms = b.scalar("num_arms");
        h->nj = h->num_arms == 3 ? 21 : 14;
        static const int mx[5] = {4, 4, 5, 3, 4};  // env.py:423, 509, 598, 699, 788
        h->max_reward = mx[h->task_id];
        h->obj_qadr = b.i("objects_qposadr");
        h->nobj = (int)h->obj_qadr.size();
        h->obs_qadr = b.i("obs_qposadr");
        h->qpos_home = b.f("qpos_home");
        h->ctrl_home = b.f("ctrl_home");
        fill_ik(b, h->ik);
        std::string perr;
        if (!h->phys.init(b, num_envs, h->f64, perr)) { g_create_error = perr; return AVSIM_EMODEL; }
        h->render.build(b, num_envs);
        h->vis.keep_instances(b);
    } catch (const std::exception& ex) {
        g_create_error = std::string("avsim_create: ") + ex.what();
        return AVSIM_EMODEL;
    }
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); return AVSIM_EHIP; }
    h->own_stream = true;
    for (auto& ev : h->ev) (void)hipEventCreate(&ev);
    size_t N = num_envs, r = h->rsz();
    h->d_qpos = h->state.get(N * h->nq * r); h->d_qvel = h->state.get(N * h->nv * r);
    h->d_ctrl = h->state.get(N * h->nu * r); h->d_warm = h->state.get(N * h->nv * r);
    h->d_latch = (int*)h->state.get(N * sizeof(int));
    if (h->state.error() != hipSuccess) {
        g_create_error = "avsim_create: hipMalloc of the state arrays failed";
        avsim_destroy(h.release());
        return AVSIM_EHIP;
    }
    *out = h.release();
    // bring every env to the home pose with objects at their model default pose
    std::vector<double> obj((size_t)num_envs * (*out)->nobj * 7);
    for (int i = 0; i < num_envs; i++)
        for (int o = 0; o < (*out)->nobj; o++)
            for (int k = 0; k < 7; k++) obj[((size_t)i * (*out)->nobj + o) * 7 + k] = (*out)->qpos_home[(*out)->obj_qadr[o] + k];
    int rc = reset_from(*out, /*device_mode=*/false, nullptr, obj.data());          // (a host array, whatever the handle's I/O mode)
    if (rc) {
        g_create_error = (*out)->err;
        avsim_destroy(*out);
        *out = nullptr;
        return rc;
    }
    return AVSIM_OK;
}

void avsim_destroy(avsim_t* h) {
    if (!h) return;
    DevGuard dev_guard_(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->stage.destroy();          // (pinned memory and events next to the device buffers: these two keep a destroy())
    h->io.destroy();
    for (auto& ev : h->ev)
        if (ev) (void)hipEventDestroy(ev);
    const hipStream_t own = h->own_stream ? h->stream : nullptr;
    delete h;                    // every member's device memory and timing events
    if (own) (void)hipStreamDestroy(own);
}

int avsim_dims(const avsim_t* h, int32_t d[AVSIM_NDIMS]) {
    if (!h || !d) return AVSIM_EINVAL;
    d[0] = h->nq; d[1] = h->nv; d[2] = h->nu; d[3] = h->nj; d[4] = h->nobj; d[5] = h->max_reward; d[6] = h->N;
    d[7] = h->task_id; d[8] = h->phys.maxcon; d[9] = h->phys.maxefc;
    d[10] = (int32_t)h->phys.lds_bytes();
    d[11] = (int32_t)(160 * 1024 / (h->phys.lds_bytes() ? h->phys.lds_bytes() : 1));
    return AVSIM_OK;
}

int avsim_set_option(avsim_t* h, const char* name, double value) {
    if (!h || !name) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);               // "maxefc" / "maxcon" / "profile_phases" allocate on the handle's device
    if (!std::strcmp(name, "kernel_timing")) { h->ktiming = value != 0; h->render.timing = value != 0; return AVSIM_OK; }
    if (!std::strcmp(name, "render_proxies")) { h->render_proxies = value != 0; return AVSIM_OK; }
    if (!std::strcmp(name, "render_samples")) { if (value != 1 && value != 4) { h->set_error("render_samples is 1 or 4"); return AVSIM_EINVAL; } h->vis.samples = (int)value; return AVSIM_OK; }
    if (!std::strcmp(name, "render_shadows")) { h->vis.shadows = value != 0; return AVSIM_OK; }
    if (!std::strcmp(name, "render_smooth")) { h->vis.smooth_opt = value != 0; h->vis.S.smooth = value != 0 ? 1 : 0; return AVSIM_OK; }
    if (!std::strcmp(name, "render_shadow_size")) { if (value != 512 && value != 1024 && value != 2048) { h->set_error("render_shadow_size is 512, 1024 or 2048"); return AVSIM_EINVAL; } h->vis.shadow_size = (int)value; return AVSIM_OK; }
    if (!std::strcmp(name, "render_cam_major")) { h->vis.cam_major = value != 0; return AVSIM_OK; }
    if (!std::strcmp(name, "render_chunk")) { if (value < 1) { h->set_error("render_chunk is a number of envs >= 1"); return AVSIM_EINVAL; } h->render.env_chunk = (int)value; return AVSIM_OK; }
    if (!std::strcmp(name, "render_labels_form")) { h->labels_unpacked = value != 0; return AVSIM_OK; }
    if (!std::strcmp(name, "voxel_other_form")) { h->voxel_other_form = value != 0; return AVSIM_OK; }
    if (!std::strcmp(name, "virtviews_form")) { if (!(value >= 0 && value <= 5 && value == (int)value)) { h->set_error("virtviews_form is 0 (the form the build ships) or 1 + a form 0..4"); return AVSIM_EINVAL; } h->virtviews_form = (int)value; return AVSIM_OK; }
    if (!std::strcmp(name, "jpeg_decode_events")) { h->jpegdec_events = value != 0; return AVSIM_OK; }
    if (!std::strcmp(name, "jpeg_decode_budget")) { if (value < 1) { h->set_error("jpeg_decode_budget is a number of bytes >= 1"); return AVSIM_EINVAL; } h->jpegdec.coef_budget = (size_t)value; return AVSIM_OK; }
    if (!std::strcmp(name, "augment_scratch_bytes")) { if (!(value >= 1)) { h->set_error("augment_scratch_bytes is a number of bytes >= 1"); return AVSIM_EINVAL; } h->imgaug.scratch_limit = (size_t)value; return AVSIM_OK; }
    if (!std::strcmp(name, "diffik_iters")) { h->ik.diff_iters = (int)value; return AVSIM_OK; }
    if (!std::strcmp(name, "gradik_iters")) { h->ik.grad_iters = (int)value; return AVSIM_OK; }
    try {
        if (h->phys.set_option(name, value)) {
            if (!std::strcmp(name, "num_joints")) h->nj = (int)value;
            return AVSIM_OK;
        }
    } catch (const std::exception& ex) {
        h->set_error("avsim_set_option(%s): %s", name, ex.what());
        return AVSIM_EHIP;
    }
    h->set_error("avsim_set_option: unknown option '%s'", name);
    return AVSIM_EINVAL;
}

int avsim_sync(avsim_t* h) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return AVSIM_OK;
}

int avsim_set_stream(avsim_t* h, void* s) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)s;
    h->own_stream = false;
    return AVSIM_OK;
}

int avsim_event_record(avsim_t* h, int slot) {
    if (!h || slot < 0 || slot >= 16) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipEventRecord(h->ev[slot], h->stream));
    return AVSIM_OK;
}

int avsim_event_elapsed_ms(avsim_t* h, int a, int b, float* ms) {
    if (!h || !ms || a < 0 || a >= 16 || b < 0 || b >= 16) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipEventSynchronize(h->ev[b]));
    HIPCHK(h, hipEventElapsedTime(ms, h->ev[a], h->ev[b]));
    return AVSIM_OK;
}

int avsim_kernel_time(avsim_t* h, int reset, double* total_ms, int64_t* launches) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    long long n = 0;
    HIPCHK(h, h->ktimer.read(reset != 0, total_ms, &n));
    if (launches) *launches = n;
    return AVSIM_OK;
}

int avsim_render_kernel_time(avsim_t* h, int reset, double* total_ms, int64_t* launches) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    long long n = 0;
    HIPCHK(h, h->render.timer.read(reset != 0, total_ms, &n));
    if (launches) *launches = n;
    return AVSIM_OK;
}

// option "phys_specialised" = 2: a call whose physics launch would take the generic kernel fails HERE, before the call's first enqueue
// (the reset kernel, the state conversion and the Cartesian step's IK all write state ahead of the physics launch)
#define AVS_PHYS_GATE(h) do { if ((h)->phys.refuses((h)->err)) return AVSIM_EINVAL; } while (0)

int avsim_observe(avsim_t* h, double* agent_pos, int32_t* reward, uint8_t* success) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    AVS_PHYS_GATE(h);
    Call io(h);
    const size_t N = h->N;
    double* dap = io.out(agent_pos, sizeof(double) * N * h->nj);
    int32_t* drw = io.out(reward, sizeof(int32_t) * N);
    uint8_t* dsu = io.out(success, N);
    if (io.failed()) return AVSIM_EHIP;
    h->phys.force_reward = 1;
    const int rc = h->phys.launch(h->stream, 0, nullptr, h->d_qpos, h->d_qvel, h->d_ctrl, h->d_warm, h->d_latch, dap, drw, dsu, h->err);
    h->phys.force_reward = 0;
    if (rc) return rc;
    return io.done();
}

int avsim_fk_jac(avsim_t* h, int arm, int n, const double* q, double* T, double* J) {
    if (!h || arm < 0 || arm > 2 || n <= 0 || !q) { if (h) h->set_error("avsim_fk_jac: bad arguments"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const int nj = h->ik.arm[arm].n;
    Call io(h);
    const double* dq = io.in(q, sizeof(double) * n * nj);
    double* dT = io.out(T, sizeof(double) * n * 16);
    double* dJ = io.out(J, sizeof(double) * n * 6 * nj);
    if (io.failed()) return AVSIM_EHIP;
    dim3 grid((n + 63) / 64);
    if (nj == 6) hipLaunchKernelGGL(k_fk_jac<6>, grid, dim3(64), 0, h->stream, h->ik, arm, n, dq, dT, dJ);
    else hipLaunchKernelGGL(k_fk_jac<7>, grid, dim3(64), 0, h->stream, h->ik, arm, n, dq, dT, dJ);
    HIPCHK(h, hipGetLastError());
    return io.done();
}

int avsim_ik(avsim_t* h, int arm, int controller, int max_iters, int n, const double* q, const double* pos,
             const double* quat, double* qout) {
    if (!h || arm < 0 || arm > 2 || n <= 0 || !q || !pos || !quat || !qout || controller < 0 || controller > 1) {
        if (h) h->set_error("avsim_ik: bad arguments");
        return AVSIM_EINVAL;
    }
    if (controller == 1 && arm == 2) { h->set_error("avsim_ik: GradIK is defined for the 6-DoF manipulators only"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const int nj = h->ik.arm[arm].n;
    int iters = max_iters > 0 ? max_iters : (controller == 0 ? h->ik.diff_iters : h->ik.grad_iters);
    Call io(h);
    const double* dq = io.in(q, sizeof(double) * n * nj);
    const double* dp = io.in(pos, sizeof(double) * n * 3);
    const double* dqt = io.in(quat, sizeof(double) * n * 4);
    double* dout = io.out(qout, sizeof(double) * n * nj);
    if (io.failed()) return AVSIM_EHIP;
    if (controller == 1) hipLaunchKernelGGL(k_ik, dim3((n + 3) / 4), dim3(64), 0, h->stream, h->ik, arm, iters, n, dq, dp, dqt, dout);
    else {
        const DiffIkIo dio = {dq, 0, nj, 0, dp, dqt, nullptr, 3, 4, 0, dout, 0, nj, 0};
        hipLaunchKernelGGL(k_cart_ctrl, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->ik, arm, iters, n, dio);
    }
    HIPCHK(h, hipGetLastError());
    return io.done();
}

}  // extern "C"

template <typename real>
static int reset_impl(avsim_t* h, Call& io, const uint8_t* mask, const double* obj) {
    const uint8_t* dm = io.in(mask, h->N);
    const double* dobj = io.in(obj, sizeof(double) * h->N * h->nobj * 7);
    if (io.failed()) return AVSIM_EHIP;
    hipLaunchKernelGGL(k_reset<real>, dim3((h->N + 63) / 64), dim3(64), 0, h->stream, h->N, h->nq, h->nv, h->nu, h->nobj, dm, dobj, h->phys.d_qpos_home,
                       h->phys.d_ctrl_home, h->phys.d_obj_qadr, (real*)h->d_qpos, (real*)h->d_qvel, (real*)h->d_ctrl, (real*)h->d_warm, h->d_latch,
                       h->phys.d_obj_reset);
    HIPCHK(h, hipGetLastError());
    // mj_forward (env.py:244, 538): refresh kinematics + contacts of the new state, no time stepping
    if (int rc = h->phys.launch(h->stream, 0, nullptr, h->d_qpos, h->d_qvel, h->d_ctrl, h->d_warm, h->d_latch, nullptr, nullptr, nullptr, h->err))
        return rc;
    return io.done();
}

// avsim_reset; avsim_create brings the envs to the model's default pose through it, from a host array whatever the handle's I/O mode
static int reset_from(avsim_t* h, bool device_mode, const uint8_t* mask, const double* obj_qpos) {
    AVS_ON_DEVICE(h);
    AVS_PHYS_GATE(h);
    h->state_ver++;
    Call io(h, device_mode);
    return h->f64 ? reset_impl<double>(h, io, mask, obj_qpos) : reset_impl<float>(h, io, mask, obj_qpos);
}

extern "C" {

int avsim_reset(avsim_t* h, const uint8_t* mask, const double* obj_qpos) {
    if (!h || !obj_qpos) { if (h) h->set_error("avsim_reset: obj_qpos is required"); return AVSIM_EINVAL; }
    return reset_from(h, h->io_device, mask, obj_qpos);
}

// the physics launch of the steps, between its pair of timing events.  Device pointers all: the callers stage, and finish, round it
static int step_common(avsim_t* h, const float* d_action, int nsub, double* dap, int32_t* drw, uint8_t* dsu) {
    if (h->ktiming) HIPCHK(h, h->ktimer.begin(h->stream));      // (once per EV_RING launches this waits for the pairs held and folds them into the sum)
    if (int rc = h->phys.launch(h->stream, nsub, d_action, h->d_qpos, h->d_qvel, h->d_ctrl, h->d_warm, h->d_latch, dap, drw, dsu, h->err)) return rc;
    if (h->ktiming) HIPCHK(h, h->ktimer.end(h->stream));
    return AVSIM_OK;
}
// ... with the three outputs every step has staged in front of it and brought back behind it
static int step_staged(avsim_t* h, Call& io, const float* d_action, int nsub, double* agent_pos, int32_t* reward, uint8_t* success) {
    h->state_ver++;
    const size_t N = h->N;
    double* dap = io.out(agent_pos, sizeof(double) * N * h->nj);
    int32_t* drw = io.out(reward, sizeof(int32_t) * N);
    uint8_t* dsu = io.out(success, N);
    if (io.failed()) return AVSIM_EHIP;
    if (int rc = step_common(h, d_action, nsub, dap, drw, dsu)) return rc;
    return io.done();
}

int avsim_step(avsim_t* h, const float* action, int nsub, double* agent_pos, int32_t* reward, uint8_t* success) {
    if (!h || !action || nsub < 0) { if (h) h->set_error("avsim_step: bad arguments"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    AVS_PHYS_GATE(h);
    Call io(h);
    const float* da = io.in(action, sizeof(float) * h->N * h->nj);
    if (io.failed()) return AVSIM_EHIP;
    return step_staged(h, io, da, nsub, agent_pos, reward, success);
}

int avsim_step_ctrl(avsim_t* h, int nsub, double* agent_pos, int32_t* reward, uint8_t* success) {
    if (!h || nsub < 0) { if (h) h->set_error("avsim_step_ctrl: bad arguments"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    AVS_PHYS_GATE(h);
    Call io(h);
    return step_staged(h, io, nullptr, nsub, agent_pos, reward, success);
}

int avsim_step_cartesian(avsim_t* h, const double* action23, int ik_mode, int nsub, double* agent_pos, int32_t* reward,
                         uint8_t* success) {
    if (!h || !action23 || nsub < 0 || (ik_mode != AVSIM_IK_REFERENCE && ik_mode != AVSIM_IK_DLS)) {
        if (h) h->set_error("avsim_step_cartesian: bad arguments");
        return AVSIM_EINVAL;
    }
    if (h->num_arms != 3) { h->set_error("avsim_step_cartesian: the 23-D Cartesian action drives three arms (sim_env.py:277-282)"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    AVS_PHYS_GATE(h);
    Call io(h);
    const double* da = io.in(action23, sizeof(double) * h->N * 23);
    if (io.failed()) return AVSIM_EHIP;
    auto launch = [&](dim3 grid, int arm0) {      // arms arm0 .. arm0 + grid.y - 1: their slices of the action (8 entries an arm) and of ctrl (7)
        const size_t real = h->f64 ? sizeof(double) : sizeof(float);
        const DiffIkIo dio = {h->d_qpos, !h->f64, h->nq, 1, da + 8 * arm0, da + 8 * arm0 + 3, da + 8 * arm0 + 7, 23, 23, 8,
                              (char*)h->d_ctrl + real * 7 * arm0, !h->f64, h->nu, 7};
        hipLaunchKernelGGL(k_cart_ctrl, grid, dim3(64), 0, h->stream, h->ik, arm0, h->ik.diff_iters, h->N, dio);
    };
    if (ik_mode == AVSIM_IK_DLS) launch(dim3((h->N + 63) / 64, 3), 0);
    else {
        // GradIK on the two manipulators: 16 lanes per env
        if (h->f64) hipLaunchKernelGGL(k_gradik_ctrl<double>, dim3((h->N + 3) / 4, 2), dim3(64), 0, h->stream, h->ik, h->N, h->nq, h->nu, da, (const double*)h->d_qpos, (double*)h->d_ctrl);
        else hipLaunchKernelGGL(k_gradik_ctrl<float>, dim3((h->N + 3) / 4, 2), dim3(64), 0, h->stream, h->ik, h->N, h->nq, h->nu, da, (const float*)h->d_qpos, (float*)h->d_ctrl);
        launch(dim3((h->N + 63) / 64, 1), 2);     // DiffIK on the camera arm: one env per lane
    }
    HIPCHK(h, hipGetLastError());
    return step_staged(h, io, nullptr, nsub, agent_pos, reward, success);
}

// ---- state access --------------------------------------------------------------------------------
// one state array in / out, converted to / from the handle's real.  A null array is left out; so is everything after a failure, which the caller's
// io.done() reports
static void put(avsim_t* h, Call& io, const double* src, void* dst, size_t n) {
    const double* d = io.in(src, sizeof(double) * n);
    if (!d) return;
    unsigned g = (unsigned)((n + 255) / 256);
    if (h->f64) hipLaunchKernelGGL((k_convert<double, double>), dim3(g), dim3(256), 0, h->stream, n, d, (double*)dst);
    else hipLaunchKernelGGL((k_convert<double, float>), dim3(g), dim3(256), 0, h->stream, n, d, (float*)dst);
}
static void get(avsim_t* h, Call& io, double* dst, const void* src, size_t n) {
    double* d = io.out(dst, sizeof(double) * n);
    if (!d) return;
    unsigned g = (unsigned)((n + 255) / 256);
    if (h->f64) hipLaunchKernelGGL((k_convert<double, double>), dim3(g), dim3(256), 0, h->stream, n, (const double*)src, d);
    else hipLaunchKernelGGL((k_convert<float, double>), dim3(g), dim3(256), 0, h->stream, n, (const float*)src, d);
}

int avsim_get_state(avsim_t* h, double* qpos, double* qvel, double* ctrl, double* warm) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    size_t N = h->N;
    Call io(h);
    get(h, io, qpos, h->d_qpos, N * h->nq);
    get(h, io, qvel, h->d_qvel, N * h->nv);
    get(h, io, ctrl, h->d_ctrl, N * h->nu);
    get(h, io, warm, h->d_warm, N * h->nv);
    if (io.failed()) return AVSIM_EHIP;
    HIPCHK(h, hipGetLastError());
    return io.done();
}

int avsim_set_state(avsim_t* h, const double* qpos, const double* qvel, const double* ctrl, const double* warm) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    AVS_PHYS_GATE(h);
    h->state_ver++;
    size_t N = h->N;
    Call io(h);
    put(h, io, qpos, h->d_qpos, N * h->nq);
    put(h, io, qvel, h->d_qvel, N * h->nv);
    put(h, io, ctrl, h->d_ctrl, N * h->nu);
    put(h, io, warm, h->d_warm, N * h->nv);
    if (io.failed()) return AVSIM_EHIP;
    HIPCHK(h, hipGetLastError());
    if (int rc = h->phys.launch(h->stream, 0, nullptr, h->d_qpos, h->d_qvel, h->d_ctrl, h->d_warm, h->d_latch, nullptr, nullptr, nullptr, h->err))
        return rc;
    return io.done();
}

int avsim_get_latch(avsim_t* h, int32_t* latch) {
    if (!h || !latch) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(latch, h->d_latch, sizeof(int32_t) * (size_t)h->N, h->io_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return Call(h).done();
}

int avsim_set_latch(avsim_t* h, const int32_t* latch) {
    if (!h || !latch) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(h->d_latch, latch, sizeof(int32_t) * (size_t)h->N, h->io_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return Call(h).done();
}

// The object poses a diverged env falls back to (mj_checkPos-style reset): written by avsim_reset; state next to the
// latch for a handle that continues another one's episode (hide / show_middle_arm, checkpoints): double[N][nobj][7]
int avsim_get_reset_poses(avsim_t* h, double* obj_qpos) {
    if (!h || !obj_qpos) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(obj_qpos, h->phys.d_obj_reset, sizeof(double) * (size_t)h->N * h->nobj * 7, h->io_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return Call(h).done();
}

int avsim_set_reset_poses(avsim_t* h, const double* obj_qpos) {
    if (!h || !obj_qpos) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(h->phys.d_obj_reset, obj_qpos, sizeof(double) * (size_t)h->N * h->nobj * 7, h->io_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return Call(h).done();
}

int avsim_set_qpos(avsim_t* h, const double* qpos) {
    if (!h || !qpos) return AVSIM_EINVAL;
    return avsim_set_state(h, qpos, nullptr, nullptr, nullptr);
}

int avsim_get_contacts(avsim_t* h, int32_t* ncon, int32_t* pairs, double* dist) {
    if (!h) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    size_t N = h->N, cap = h->phys.maxcon;
    if (h->io_device) {
        if (ncon) HIPCHK(h, hipMemcpyAsync(ncon, h->phys.d_ncon, N * 4, hipMemcpyDeviceToDevice, h->stream));
        if (pairs) HIPCHK(h, hipMemcpyAsync(pairs, h->phys.cpairs.ptr(), N * cap * 8, hipMemcpyDeviceToDevice, h->stream));
        if (dist) HIPCHK(h, hipMemcpyAsync(dist, h->phys.cdist.ptr(), N * cap * 8, hipMemcpyDeviceToDevice, h->stream));
        return AVSIM_OK;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (ncon) HIPCHK(h, hipMemcpy(ncon, h->phys.d_ncon, N * 4, hipMemcpyDeviceToHost));
    if (pairs) HIPCHK(h, hipMemcpy(pairs, h->phys.cpairs.ptr(), N * cap * 8, hipMemcpyDeviceToHost));
    if (dist) HIPCHK(h, hipMemcpy(dist, h->phys.cdist.ptr(), N * cap * 8, hipMemcpyDeviceToHost));
    return AVSIM_OK;
}

/* debug: per-env cycle counters of the 8 physics phases of the last launch (option "profile_phases"); int64[N][10] */
int avsim_get_phase_cycles(avsim_t* h, int64_t* out) {
    if (!h || !out || !h->phys.d_prof) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->phys.d_prof, (size_t)h->N * avs::PROF_W * 8, h->io_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return AVSIM_OK;
}

int avsim_get_diag(avsim_t* h, int32_t* diag) {
    if (!h || !diag) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    size_t N = h->N;
    if (h->io_device) {
        HIPCHK(h, hipMemcpyAsync(diag, h->phys.d_diag, N * 16, hipMemcpyDeviceToDevice, h->stream));
        return AVSIM_OK;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(diag, h->phys.d_diag, N * 16, hipMemcpyDeviceToHost));
    return AVSIM_OK;
}

}  // extern "C"

extern "C" {

// E6 (env.py:180-188 get_obs pixels / :195-200 render) as depth images: forward pass of the physics kernel (nsub = 0) exports
// the body poses, then the two render kernels run on the same stream.  render_to: into device memory, with the handle's device current.
// body poses of the current state into render.d_xpose, when those it holds are another state's (a forward pass of the physics kernel, no substep)
static int refresh_xpose(avsim_t* h) {
    if (h->xpose_ver != h->state_ver) {
        h->phys.d_xpose = h->render.d_xpose;
        const int rc = h->phys.launch(h->stream, 0, nullptr, h->d_qpos, h->d_qvel, h->d_ctrl, h->d_warm, h->d_latch, nullptr, nullptr, nullptr, h->err);
        h->phys.d_xpose = nullptr;
        if (rc) return rc;
        h->xpose_ver = h->state_ver;
    }
    return 0;
}
static int render_to(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, void* dout, bool rgb, bool f32) {
    int rc;
    if ((rc = refresh_xpose(h))) return rc;
    if (rgb && h->vis.cam_major && !(h->vis.loaded && !h->render_proxies)) { h->set_error("option render_cam_major applies to the visual scene's images only (avsim_load_visual, render_proxies 0)"); return AVSIM_EINVAL; }
    if (rgb && h->vis.loaded && !h->render_proxies)
        rc = h->vis.launch(h->stream, h->N, h->render.d_xpose, (const int*)cam_ids, ncam, h->render.m.ncam, height, width, dout, h->err, h->state_ver, f32);
    else
        rc = h->render.launch(h->stream, (const int*)cam_ids, ncam, height, width, dout, rgb, h->err);
    return rc ? (rc < -1 ? AVSIM_EHIP : AVSIM_EINVAL) : AVSIM_OK;
}
static int render_images(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, void* out, bool rgb, bool f32 = false) {
    const char* who = f32 ? "avsim_render_rgb_f32" : rgb ? "avsim_render_rgb" : "avsim_render_depth";
    if (!h || !cam_ids || !out) { if (h) h->set_error("%s: bad arguments", who); return AVSIM_EINVAL; }
    if (f32 && !(h->vis.loaded && !h->render_proxies)) { h->set_error("avsim_render_rgb_f32 draws the visual scene only (avsim_load_visual, render_proxies 0)"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    Call io(h);
    void* dout = io.out(out, (f32 ? 3 * sizeof(float) : rgb ? 3 : sizeof(float)) * (size_t)h->N * ncam * height * width);
    if (io.failed()) return AVSIM_EHIP;
    if (int rc = render_to(h, cam_ids, ncam, height, width, dout, rgb, f32)) return rc;
    return io.done();
}
int avsim_render_depth(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, float* out) {
    return render_images(h, cam_ids, ncam, height, width, out, false);
}
// E6 as colour images of the same proxies (env.py:180-188 "pixels" u8[H][W][3], :195-200 render)
int avsim_render_rgb(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, uint8_t* out) {
    return render_images(h, cam_ids, ncam, height, width, out, true);
}
// the visual scene's colour images as a policy reads them (eval.py preprocess_observation): float32 planar CHW, (float)u8 / 255
int avsim_render_rgb_f32(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, float* out) {
    return render_images(h, cam_ids, ncam, height, width, out, true, true);
}

// ---- what every pixel shows (av_aloha_amd/segment.py is the specification): k_render_depth's labels mode, the depth mode's cast with the winning
// record kept.  table and drop are folded into one entry per geom here -- label | LUT_DROP where drop[label] -- and go through the pinned staging.
int avsim_render_labels(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, const uint8_t* table, const uint8_t* drop, float* depth, uint8_t* labels) {
    if (!h) return AVSIM_EINVAL;
    if (!cam_ids) { h->set_error("avsim_render_labels: cam_ids is null"); return AVSIM_EINVAL; }
    if (!depth && !labels) { h->set_error("avsim_render_labels: depth and labels are both null"); return AVSIM_EINVAL; }
    if (drop && !depth) { h->set_error("avsim_render_labels: drop changes the depth image, and depth is null"); return AVSIM_EINVAL; }
    if (ncam < 1 || ncam > 16 || height < 1 || width < 1 || height > 4096 || width > 4096) { h->set_error("avsim_render_labels: bad camera count or image size"); return AVSIM_EINVAL; }
    for (int c = 0; c < ncam; c++)
        if (cam_ids[c] < 0 || cam_ids[c] >= h->render.m.ncam) { h->set_error("avsim_render_labels: camera index out of range"); return AVSIM_EINVAL; }
    const int ngeom = h->render.m.ngeom;
    if (ngeom > BL_MAX) { h->set_error("avsim_render_labels: the model has more geoms than a bin's list holds (BL_MAX)"); return AVSIM_EINVAL; }
    if (h->io_device && (width & 3) == 0 && ((depth && ((uintptr_t)depth & 15)) || (labels && ((uintptr_t)labels & 3)))) {
        h->set_error("avsim_render_labels: with a width that is a multiple of 4, depth is 16-byte and labels 4-byte aligned (a row's four pixels leave in one store)");
        return AVSIM_EINVAL;
    }
    AVS_ON_DEVICE(h);
    Call io(h);
    const size_t npx = (size_t)h->N * ncam * height * width;
    float* ddepth = io.out(depth, sizeof(float) * npx);
    uint8_t* dlabels = io.out(labels, npx);
    if (io.failed()) return AVSIM_EHIP;
    if (int rc = refresh_xpose(h)) return rc;
    const size_t bytes = sizeof(uint16_t) * (size_t)(ngeom + 1);
    StageRing::Slot* s = h->stage.acquire(bytes, h->err);
    if (!s) return AVSIM_EHIP;
    uint16_t* lut = (uint16_t*)s->pin;
    for (int g = 0; g <= ngeom; g++) {
        const unsigned l = table ? table[g] : (g < ngeom ? (unsigned)g : 255u);
        lut[g] = (uint16_t)(l | (drop && drop[l] ? LUT_DROP : 0));
    }
    if (h->stage.upload(*s, bytes, h->stream, h->err)) return AVSIM_EHIP;
    const int lrc = h->render.launch_mode(h->stream, (const int*)cam_ids, ncam, height, width, h->labels_unpacked ? RM_LABELS : RM_LABELS_PK, ddepth, dlabels, (const unsigned short*)s->dev.ptr(), h->err);
    const std::string lerr = h->err;
    const int rrc = h->stage.release(*s, h->stream, h->err);
    if (lrc) { h->err = lerr; return lrc < -1 ? AVSIM_EHIP : AVSIM_EINVAL; }
    if (rrc) return AVSIM_EHIP;
    return io.done();
}

// ---- point clouds from depth images (av_aloha_amd/pointcloud.py is the specification; the kernels: csrc/avsim_pointcloud.hip, a unit of its own flags)
static PcModel pc_model(const avsim_t* h) {
    const RenderModel& m = h->render.m;
    return PcModel{h->render.d_xpose, m.cam_body, m.cam_pos, m.cam_mat, m.cam_fovy, m.nbody};
}
int avsim_camera_poses(avsim_t* h, const int32_t* cam_ids, int ncam, float* out) {
    if (!h) return AVSIM_EINVAL;
    if (!cam_ids || !out || ncam < 1 || ncam > PC_MAX_CAMS) { h->set_error("avsim_camera_poses: bad arguments (1..%d cameras)", PC_MAX_CAMS); return AVSIM_EINVAL; }
    PcCall c{};
    for (int k = 0; k < ncam; k++) {
        if (cam_ids[k] < 0 || cam_ids[k] >= h->render.m.ncam) { h->set_error("avsim_camera_poses: camera index out of range"); return AVSIM_EINVAL; }
        c.cam[k] = cam_ids[k];
    }
    c.ncam = ncam;
    AVS_ON_DEVICE(h);
    Call io(h);
    float* dout = io.out(out, sizeof(float) * PC_POSE_W * (size_t)h->N * ncam);
    if (io.failed()) return AVSIM_EHIP;
    if (int rc = refresh_xpose(h)) return rc;
    if (pointcloud_poses_launch(h->stream, pc_model(h), c, 0, h->N, dout, h->err)) return AVSIM_EHIP;
    return io.done();
}

int avsim_point_cloud(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, const float* depth, const float* bounds, float max_depth, int npoints, float* xyz,
                      int32_t* index, int32_t* count) {
    if (!h) return AVSIM_EINVAL;
    if (!cam_ids || !depth || !bounds || !xyz || !index || !count) { h->set_error("avsim_point_cloud: a null pointer"); return AVSIM_EINVAL; }
    {   // the host arrays are checked before anything moves or is launched
        std::string why;
        if (pointcloud_validate(h->render.m.ncam, cam_ids, ncam, height, width, bounds, max_depth, npoints, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    PcCall c{};
    for (int k = 0; k < ncam; k++) c.cam[k] = cam_ids[k];
    c.ncam = ncam; c.H = height; c.W = width; c.P = npoints; c.max_depth = max_depth;
    for (int k = 0; k < 3; k++) { c.lo[k] = bounds[k]; c.hi[k] = bounds[3 + k]; }
    AVS_ON_DEVICE(h);
    Call io(h);
    const size_t N = (size_t)h->N;
    const float* ddepth = io.in(depth, sizeof(float) * N * ncam * height * width);
    float* dxyz = io.out(xyz, sizeof(float) * 3 * N * npoints);
    int32_t* dindex = io.out(index, sizeof(int32_t) * N * npoints);
    int32_t* dcount = io.out(count, sizeof(int32_t) * 2 * N);
    if (io.failed()) return AVSIM_EHIP;
    if (int rc = refresh_xpose(h)) return rc;
    if (h->pointcloud.run(h->stream, pc_model(h), c, h->N, ddepth, dxyz, dindex, dcount, h->err)) return AVSIM_EHIP;
    return io.done();
}

// ---- voxel grids from depth (and colour) images (av_aloha_amd/voxel.py is the specification; the kernels: csrc/avsim_pointcloud.hip, below the cloud's)
int avsim_voxel_grid(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, const float* depth, const uint8_t* rgb, const float* bounds, float max_depth,
                     const int32_t* grid, float* out) {
    if (!h) return AVSIM_EINVAL;
    if (!cam_ids || !depth || !bounds || !grid || !out) { h->set_error("avsim_voxel_grid: a null pointer"); return AVSIM_EINVAL; }
    {   // the host arrays are checked before anything moves or is launched
        std::string why;
        if (voxel_validate(h->render.m.ncam, cam_ids, ncam, height, width, bounds, max_depth, grid, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    if (h->io_device && ((uintptr_t)out & 15)) { h->set_error("avsim_voxel_grid: out is 16-byte aligned (the cells are cleared and finished with 16-byte accesses)"); return AVSIM_EINVAL; }
    VoxCall c{};
    for (int k = 0; k < ncam; k++) c.pc.cam[k] = cam_ids[k];
    c.pc.ncam = ncam; c.pc.H = height; c.pc.W = width; c.pc.P = 0; c.pc.max_depth = max_depth;
    for (int k = 0; k < 3; k++) { c.pc.lo[k] = bounds[k]; c.pc.hi[k] = bounds[3 + k]; c.g[k] = grid[k]; }
    AVS_ON_DEVICE(h);
    Call io(h);
    const size_t N = (size_t)h->N, q = (size_t)ncam * height * width, cell_floats = (size_t)grid[0] * grid[1] * grid[2] * VOX_CHANNELS;
    const float* ddepth = io.in(depth, sizeof(float) * N * q);
    const uint8_t* drgb = io.in(rgb, 3 * N * q);
    float* dout = io.out(out, sizeof(float) * N * cell_floats);
    if (io.failed()) return AVSIM_EHIP;
    if (int rc = refresh_xpose(h)) return rc;
    const int chunk = h->N < PC_ENV_CHUNK ? h->N : PC_ENV_CHUNK;
    if (h->pointcloud.reserve_poses(chunk, ncam, h->err)) return AVSIM_EHIP;
    for (int e0 = 0; e0 < h->N; e0 += chunk) {          // envs in chunks, as PcHost::run: the pose scratch is a chunk's
        const int n = h->N - e0 < chunk ? h->N - e0 : chunk;
        if (pointcloud_poses_launch(h->stream, pc_model(h), c.pc, e0, n, h->pointcloud.pose.as<float>(), h->err)) return AVSIM_EHIP;
        if (voxel_launch(h->stream, c, n, ddepth + (size_t)e0 * q, drgb ? drgb + (size_t)e0 * q * 3 : nullptr, h->pointcloud.pose.as<float>(), dout + (size_t)e0 * cell_floats,
                         (AVSIM_VOXEL_MERGE != 0) != h->voxel_other_form, h->err))
            return AVSIM_EHIP;
    }
    return io.done();
}

// ---- virtual orthographic views from depth (and colour) images (av_aloha_amd/virtviews.py is the specification; the kernels: csrc/avsim_pointcloud.hip, below the grid's)
int avsim_virtual_views(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, const float* depth, const uint8_t* rgb, const float* bounds, float max_depth,
                        const int32_t* views, int nviews, const int32_t* size, int radius, float* out, int32_t* index) {
    if (!h) return AVSIM_EINVAL;
    if (!cam_ids || !depth || !bounds || !views || !size || !out || !index) { h->set_error("avsim_virtual_views: a null pointer"); return AVSIM_EINVAL; }
    {   // the host arrays are checked before anything moves or is launched
        std::string why;
        if (virtviews_validate(h->render.m.ncam, cam_ids, ncam, height, width, bounds, max_depth, views, nviews, size, radius, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    if (h->io_device && ((uintptr_t)out & 15)) { h->set_error("avsim_virtual_views: out is 16-byte aligned (the pixels are cleared and finished with 16-byte accesses)"); return AVSIM_EINVAL; }
    VvCall c{};
    for (int k = 0; k < ncam; k++) c.pc.cam[k] = cam_ids[k];
    c.pc.ncam = ncam; c.pc.H = height; c.pc.W = width; c.pc.P = 0; c.pc.max_depth = max_depth;
    for (int k = 0; k < 3; k++) { c.pc.lo[k] = bounds[k]; c.pc.hi[k] = bounds[3 + k]; }
    for (int k = 0; k < nviews; k++) c.view[k] = views[k];
    c.nviews = nviews; c.VH = size[0]; c.VW = size[1]; c.radius = radius;
    AVS_ON_DEVICE(h);
    Call io(h);
    const size_t N = (size_t)h->N, q = (size_t)ncam * height * width, vp = (size_t)nviews * size[0] * size[1];
    const float* ddepth = io.in(depth, sizeof(float) * N * q);
    const uint8_t* drgb = io.in(rgb, 3 * N * q);
    float* dout = io.out(out, sizeof(float) * N * vp * VV_CHANNELS);
    int32_t* dindex = io.out(index, sizeof(int32_t) * N * vp);
    if (io.failed()) return AVSIM_EHIP;
    if (int rc = refresh_xpose(h)) return rc;
    const int chunk = h->N < PC_ENV_CHUNK ? h->N : PC_ENV_CHUNK;
    if (h->pointcloud.reserve_poses(chunk, ncam, h->err)) return AVSIM_EHIP;
    const int form = h->virtviews_form ? h->virtviews_form - 1 : AVSIM_VV_FORM;
    for (int e0 = 0; e0 < h->N; e0 += chunk) {          // envs in chunks, as avsim_voxel_grid: the pose scratch is a chunk's
        const int n = h->N - e0 < chunk ? h->N - e0 : chunk;
        if (pointcloud_poses_launch(h->stream, pc_model(h), c.pc, e0, n, h->pointcloud.pose.as<float>(), h->err)) return AVSIM_EHIP;
        if (virtviews_launch(h->stream, c, n, ddepth + (size_t)e0 * q, drgb ? drgb + (size_t)e0 * q * 3 : nullptr, h->pointcloud.pose.as<float>(), dout + (size_t)e0 * vp * VV_CHANNELS,
                             dindex + (size_t)e0 * vp, form, h->err))
            return AVSIM_EHIP;
    }
    return io.done();
}

// ---- the image calls: what they share
// bytes per pixel of format 0 (u8 HWC) / 1 (float32 CHW)
static size_t img_bpp(int fmt) { return fmt ? 12 : 3; }
// refuses a format other than 0 / 1 and a size outside 1..65535, of the call's image and of its second one where it has two (a call whose
// image has one format only passes that format)
static int img_args(avsim_t* h, const char* who, int fmt, int64_t ht, int64_t wd, int fmt2 = 0, int64_t ht2 = 1, int64_t wd2 = 1) {
    if ((fmt != 0 && fmt != 1) || (fmt2 != 0 && fmt2 != 1)) { h->set_error("%s: a format is 0 (u8 HWC) or 1 (float32 CHW)", who); return AVSIM_EINVAL; }
    const bool first = ht < 1 || wd < 1 || ht > 65535 || wd > 65535;
    if (first || ht2 < 1 || wd2 < 1 || ht2 > 65535 || wd2 > 65535) {
        h->set_error("%s: image size %lld x %lld outside 1..65535", who, (long long)(first ? ht : ht2), (long long)(first ? wd : wd2));
        return AVSIM_EINVAL;
    }
    return AVSIM_OK;
}
// rows: the images (streams) the input holds -- nimg, but a host caller's index says how many
static int index_rows(avsim_t* h, const char* who, const int32_t* index, int nimg, size_t* rows) {
    *rows = (size_t)nimg;
    if (h->io_device || !index) return AVSIM_OK;
    int top = 0;
    for (int i = 0; i < nimg; i++) {
        if (index[i] < 0) { h->set_error("%s: negative index", who); return AVSIM_EINVAL; }
        top = index[i] > top ? index[i] : top;
    }
    *rows = (size_t)top + 1;
    return AVSIM_OK;
}

// JPEG streams of a batch of images (av_aloha_amd/jpeg.py is the specification; csrc/avsim_jpeg.hip.h)
int64_t avsim_jpeg_bound(int height, int width) {
    if (height < 1 || width < 1 || height > 65535 || width > 65535) return AVSIM_EINVAL;
    return jpeg_bound(height, width);
}
int avsim_jpeg_encode(avsim_t* h, const void* img, int fmt, const int32_t* index, int nimg, int height, int width, int quality, uint8_t* out,
                      int64_t stride, int32_t* out_len) {
    if (!h) return AVSIM_EINVAL;
    if (!img || !out || !out_len || nimg < 0 || stride < 0) { h->set_error("avsim_jpeg_encode: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_jpeg_encode", fmt, height, width))) return rc;
    if (quality < 1 || quality > 100) { h->set_error("avsim_jpeg_encode: quality %d outside 1..100", quality); return AVSIM_EINVAL; }
    if (nimg == 0) return AVSIM_OK;
    size_t rows;
    if ((rc = index_rows(h, "avsim_jpeg_encode", index, nimg, &rows))) return rc;
    AVS_ON_DEVICE(h);
    Call io(h);
    const void* dimg = io.in(img, rows * (size_t)height * width * img_bpp(fmt));
    const int32_t* dindex = io.in(index, sizeof(int32_t) * (size_t)nimg);
    uint8_t* dout = io.out(out, (size_t)nimg * stride);
    int32_t* dlen = io.out(out_len, sizeof(int32_t) * (size_t)nimg);
    if (io.failed()) return AVSIM_EHIP;
    if (h->jpeg.launch(h->stream, dimg, fmt, dindex, nimg, height, width, quality, dout, stride, dlen, h->err)) return AVSIM_EHIP;
    return io.done();
}

// avsim_render_rgb's visual-scene images as JPEG streams: rendered into a buffer of the library's and encoded from there, so that no pixel
// leaves the device; a host caller gets the lengths and, of every stream, as many bytes as the longest one has.
int avsim_render_jpeg(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, int tile, int quality, uint8_t* out, int64_t stride,
                      int32_t* out_len) {
    if (!h) return AVSIM_EINVAL;
    if (!cam_ids || !out || !out_len || ncam < 1 || stride < 0) { h->set_error("avsim_render_jpeg: bad arguments"); return AVSIM_EINVAL; }
    if (quality < 1 || quality > 100) { h->set_error("avsim_render_jpeg: quality %d outside 1..100", quality); return AVSIM_EINVAL; }
    const int64_t iw = tile ? (int64_t)width * ncam : width;      // (below 1 where width is: ncam >= 1)
    int rc;
    if ((rc = img_args(h, "avsim_render_jpeg", 0, height, iw))) return rc;
    if (!(h->vis.loaded && !h->render_proxies)) { h->set_error("avsim_render_jpeg draws the visual scene only (avsim_load_visual, render_proxies 0)"); return AVSIM_EINVAL; }
    if (tile && h->vis.cam_major) { h->set_error("avsim_render_jpeg: tile puts the views of an env side by side (render_cam_major 0)"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const int nstream = tile ? h->N : h->N * ncam;
    const size_t bytes = (size_t)3 * h->N * ncam * height * width;
    Call io(h);
    void* dimg = io.scratch(bytes);
    if (io.failed()) return AVSIM_EHIP;
    if ((rc = render_to(h, cam_ids, ncam, height, width, dimg, true, false))) return rc;
    if (tile && ncam > 1) {
        void* dtile = io.scratch(bytes);
        if (io.failed()) return AVSIM_EHIP;
        if (jpeg_tile(h->stream, dimg, dtile, h->N, ncam, height, width, h->err)) return AVSIM_EHIP;
        dimg = dtile;
    }
    // a host caller's streams and lengths come back below, not through io.done(): device copies of the call's own
    uint8_t* dout = h->io_device ? out : (uint8_t*)io.scratch((size_t)nstream * stride);
    int32_t* dlen = h->io_device ? out_len : (int32_t*)io.scratch(sizeof(int32_t) * (size_t)nstream);
    if (io.failed()) return AVSIM_EHIP;
    if (h->jpeg.launch(h->stream, dimg, 0, nullptr, nstream, height, (int)iw, quality, dout, stride, dlen, h->err)) return AVSIM_EHIP;
    if (h->io_device) return AVSIM_OK;
    HIPCHK(h, hipMemcpyAsync(out_len, dlen, sizeof(int32_t) * (size_t)nstream, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int64_t w = 0;
    for (int i = 0; i < nstream; i++) w = out_len[i] > w ? out_len[i] : w;
    w = w < stride ? w : stride;
    if (w > 0) HIPCHK(h, hipMemcpy2DAsync(out, (size_t)stride, dout, (size_t)stride, (size_t)w, (size_t)nstream, hipMemcpyDeviceToHost, h->stream));
    return io.done();
}

// ... and back: the streams of avsim_jpeg_encode -> images (av_aloha_amd/jpeg.py decode_reference is the specification)
int avsim_jpeg_decode(avsim_t* h, const uint8_t* in, int64_t stride, const int32_t* in_len, const int32_t* index, int nimg, int height, int width,
                      int fmt, int upsample, void* out, int32_t* status) {
    if (!h) return AVSIM_EINVAL;
    if (!in || !in_len || !out || !status || nimg < 0 || stride < 1) { h->set_error("avsim_jpeg_decode: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_jpeg_decode", fmt, height, width))) return rc;
    if (upsample != 0 && upsample != 1) { h->set_error("avsim_jpeg_decode: upsample is 0 (replicate) or 1 (triangle)"); return AVSIM_EINVAL; }
    if (nimg == 0) return AVSIM_OK;
    size_t rows;
    if ((rc = index_rows(h, "avsim_jpeg_decode", index, nimg, &rows))) return rc;
    AVS_ON_DEVICE(h);
    Call io(h);
    const uint8_t* din = io.in(in, rows * (size_t)stride);
    const int32_t* dlen = io.in(in_len, sizeof(int32_t) * rows);
    const int32_t* dindex = io.in(index, sizeof(int32_t) * (size_t)nimg);
    void* dout = io.out(out, (size_t)nimg * height * width * img_bpp(fmt));
    int32_t* dstatus = io.out(status, sizeof(int32_t) * (size_t)nimg);
    if (io.failed()) return AVSIM_EHIP;
    if (h->jpegdec.launch(h->stream, din, stride, dlen, dindex, nimg, height, width, fmt, upsample, dout, dstatus, h->err, h->jpegdec_events ? h->ev + 12 : nullptr)) return AVSIM_EHIP;
    return io.done();
}

// Camera views resampled into rectangles of a canvas and labelled there (av_aloha_amd/compose.py is the specification; csrc/avsim_compose.hip.h)
int avsim_compose(avsim_t* h, const void* src, int src_fmt, int nsrc, int src_h, int src_w, void* canvas, int canvas_fmt, int nout, int canvas_h, int canvas_w,
                  const int32_t* places, int nplace, int clear, uint32_t clear_rgb) {
    if (!h) return AVSIM_EINVAL;
    if (!src || !canvas || nplace < 0 || (nplace > 0 && !places) || nsrc < 1 || nout < 1) { h->set_error("avsim_compose: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_compose", src_fmt, src_h, src_w, canvas_fmt, canvas_h, canvas_w))) return rc;
    if (!h->io_device) {          // (the arguments are checked before a host caller's pixels move)
        std::string why;
        if (ComposeHost::validate(nsrc, src_h, src_w, nout, canvas_h, canvas_w, places, nplace, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    AVS_ON_DEVICE(h);
    Call io(h);
    const size_t cbytes = (size_t)nout * canvas_h * canvas_w * img_bpp(canvas_fmt);
    const void* dsrc = io.in(src, (size_t)nsrc * src_h * src_w * img_bpp(src_fmt));
    void* dcanvas = clear ? io.out(canvas, cbytes) : io.inout(canvas, cbytes);          // (a canvas that is cleared first need not go up)
    if (io.failed()) return AVSIM_EHIP;
    if ((rc = h->compose.launch(h->stream, dsrc, src_fmt, nsrc, src_h, src_w, dcanvas, canvas_fmt, nout, canvas_h, canvas_w, places, nplace, clear, clear_rgb, h->err)))
        return rc == -1 ? AVSIM_EINVAL : AVSIM_EHIP;
    return io.done();
}

int avsim_compose_label(avsim_t* h, void* canvas, int canvas_fmt, int nout, int canvas_h, int canvas_w, const int32_t* where, int nlabel, const char* prefix,
                        const int64_t* value, uint32_t rgb) {
    if (!h) return AVSIM_EINVAL;
    if (!canvas || nlabel < 0 || (nlabel > 0 && !where) || nout < 1) { h->set_error("avsim_compose_label: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_compose_label", canvas_fmt, canvas_h, canvas_w))) return rc;
    if (nlabel == 0) return AVSIM_OK;
    AVS_ON_DEVICE(h);
    Call io(h);
    void* dcanvas = io.inout(canvas, (size_t)nout * canvas_h * canvas_w * img_bpp(canvas_fmt));
    const int64_t* dvalue = io.in(value, sizeof(int64_t) * (size_t)nlabel);
    if (io.failed()) return AVSIM_EHIP;
    if ((rc = h->compose.label(h->stream, dcanvas, canvas_fmt, nout, canvas_h, canvas_w, where, nlabel, prefix, (const long long*)dvalue, rgb, h->err)))
        return rc == -1 ? AVSIM_EINVAL : AVSIM_EHIP;
    return io.done();
}

void avsim_compose_font(uint8_t rows[128][7]) {
    std::memset(rows, 0, 128 * 7);
    for (int ch = 0; ch < 128; ch++) {
        const int g = cmp_glyph(ch);
        if (g >= 0) std::memcpy(rows[ch], CMP_FONT_HOST[g], 7);
    }
}

// Per-image sums for data-set statistics, and crops through look-up tables (av_aloha_amd/imgprep.py is the specification; csrc/avsim_imgprep.hip.h)
int avsim_image_stats(avsim_t* h, const void* img, int fmt, const int32_t* index, int nimg, int height, int width, uint64_t* out) {
    if (!h) return AVSIM_EINVAL;
    if (!img || !out || nimg < 1) { h->set_error("avsim_image_stats: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_image_stats", fmt, height, width))) return rc;
    size_t rows;
    if ((rc = index_rows(h, "avsim_image_stats", index, nimg, &rows))) return rc;
    AVS_ON_DEVICE(h);
    Call io(h);
    const void* dimg = io.in(img, rows * (size_t)height * width * img_bpp(fmt));
    const int32_t* dindex = io.in(index, sizeof(int32_t) * (size_t)nimg);
    uint64_t* dout = io.out(out, sizeof(uint64_t) * 12 * (size_t)nimg);
    if (io.failed()) return AVSIM_EHIP;
    if (ImgPrepHost::stats(h->stream, dimg, fmt, dindex, nimg, height, width, (unsigned long long*)dout, h->err)) return AVSIM_EHIP;
    return io.done();
}

int avsim_image_prep(avsim_t* h, const void* img, int fmt, int nsrc, int height, int width, const float* lut, int nlut, const int32_t* lut_index,
                     const int32_t* box, int nout, const int32_t* src_index, int out_h, int out_w, float* out) {
    if (!h) return AVSIM_EINVAL;
    if (!img || !lut || !box || !out || nsrc < 1 || nout < 1 || nlut < 1 || nlut > (1 << 20)) { h->set_error("avsim_image_prep: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_image_prep", fmt, height, width, 1, out_h, out_w))) return rc;
    {   // the host arrays are checked before anything moves or is launched
        std::string why;
        if (ImgPrepHost::validate(nsrc, height, width, nlut, lut_index, box, nout, src_index, out_h, out_w, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    AVS_ON_DEVICE(h);
    Call io(h);
    const void* dimg = io.in(img, (size_t)nsrc * height * width * img_bpp(fmt));
    const float* dlut = io.in(lut, sizeof(float) * 768 * (size_t)nlut);
    float* dout = io.out(out, sizeof(float) * 3 * (size_t)nout * out_h * out_w);
    if (io.failed()) return AVSIM_EHIP;
    if (ImgPrepHost::launch(h->stage, h->stream, dimg, fmt, height, width, dlut, lut_index, box, nout, src_index, out_h, out_w, dout, h->err)) return AVSIM_EHIP;
    return io.done();
}

// Colour and sharpness augmentation (av_aloha_amd/imgaug.py is the specification; the kernels: csrc/avsim_imgaug.hip, a unit of its own flags)
int avsim_image_jitter(avsim_t* h, const void* img, int nsrc, int height, int width, const int32_t* box_mask, const float* factor,
                       const int32_t* src_index, int nout, const float* mean_std, int out_h, int out_w, float* out) {
    if (!h) return AVSIM_EINVAL;
    if (!img || !box_mask || !factor || !out || nsrc < 1 || nout < 1) { h->set_error("avsim_image_jitter: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_image_jitter", 0, height, width, 1, out_h, out_w))) return rc;
    {   // the host arrays are checked before anything moves or is launched
        std::string why;
        if (imgaug_validate(nsrc, height, width, box_mask, factor, src_index, nout, mean_std, out_h, out_w, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    AVS_ON_DEVICE(h);
    Call io(h);
    const void* dimg = io.in(img, (size_t)nsrc * height * width * img_bpp(0));
    float* dout = io.out(out, sizeof(float) * 3 * (size_t)nout * out_h * out_w);
    if (io.failed()) return AVSIM_EHIP;
    if (h->imgaug.launch(h->stage, h->stream, dimg, height, width, box_mask, factor, src_index, nout, mean_std, out_h, out_w, dout, h->err)) return AVSIM_EHIP;
    return io.done();
}

// avsim_image_jitter with the geometric op, bit 5.  Without the bit anywhere: avsim_image_jitter's launches
int avsim_image_augment(avsim_t* h, const void* img, int nsrc, int height, int width, const int32_t* box_mask, const float* factor, const float* affine, int interp,
                        const int32_t* src_index, int nout, const float* mean_std, int out_h, int out_w, float* out) {
    if (!h) return AVSIM_EINVAL;
    if (!img || !box_mask || !factor || !out || nsrc < 1 || nout < 1) { h->set_error("avsim_image_augment: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_image_augment", 0, height, width, 1, out_h, out_w))) return rc;
    {   // the host arrays are checked before anything moves or is launched
        std::string why;
        if (imgaug_validate_affine(nsrc, height, width, box_mask, factor, affine, interp, src_index, nout, mean_std, out_h, out_w, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    bool any = false;
    for (int i = 0; i < nout && !any; i++) any = box_mask[4 * (size_t)i + 3] & IAG_AFFINE;
    AVS_ON_DEVICE(h);
    Call io(h);
    const void* dimg = io.in(img, (size_t)nsrc * height * width * img_bpp(0));
    float* dout = io.out(out, sizeof(float) * 3 * (size_t)nout * out_h * out_w);
    if (io.failed()) return AVSIM_EHIP;
    if (any ? h->imgaug.launch_affine(h->stage, h->stream, dimg, height, width, box_mask, factor, affine, interp, src_index, nout, mean_std, out_h, out_w, dout, h->err)
            : h->imgaug.launch(h->stage, h->stream, dimg, height, width, box_mask, factor, src_index, nout, mean_std, out_h, out_w, dout, h->err))
        return AVSIM_EHIP;
    return io.done();
}

// Resizing into a rectangle of a padded output (av_aloha_amd/imgresize.py is the specification; the kernels: csrc/avsim_imgresize.hip, a unit of its own flags)
int avsim_image_resize(avsim_t* h, const void* img, int fmt, int nsrc, int height, int width, const int32_t* src_box, const int32_t* dst, const int32_t* src_index, int nout,
                       int antialias, const float* fill, const float* mean_std, int out_h, int out_w, float* out) {
    if (!h) return AVSIM_EINVAL;
    if (!img || !src_box || !dst || !out || nsrc < 1 || nout < 1) { h->set_error("avsim_image_resize: bad arguments"); return AVSIM_EINVAL; }
    int rc;
    if ((rc = img_args(h, "avsim_image_resize", fmt, height, width, 1, out_h, out_w))) return rc;
    {   // the host arrays are checked before anything moves or is launched
        std::string why;
        if (imgresize_validate(nsrc, height, width, src_box, dst, src_index, nout, antialias, fill, mean_std, out_h, out_w, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    AVS_ON_DEVICE(h);
    Call io(h);
    const void* dimg = io.in(img, (size_t)nsrc * height * width * img_bpp(fmt));
    float* dout = io.out(out, sizeof(float) * 3 * (size_t)nout * out_h * out_w);
    if (io.failed()) return AVSIM_EHIP;
    if (imgresize_run(h->stage, h->stream, dimg, fmt, height, width, src_box, dst, src_index, nout, antialias, fill, mean_std, out_h, out_w, dout, h->err)) return AVSIM_EHIP;
    return io.done();
}

int avsim_image_jitter_sums(avsim_t* h, uint64_t* sums, int nout) {
    if (!h) return AVSIM_EINVAL;
    if (!sums || nout < 1 || nout > h->imgaug.nout) { h->set_error("avsim_image_jitter_sums: %d sums asked for, the last avsim_image_jitter made %d outputs", nout, h->imgaug.nout); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(sums, h->imgaug.gsum.ptr(), sizeof(uint64_t) * (size_t)nout, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return AVSIM_OK;
}

// The visual scene of avsim_render_rgb: the mesh library (models/visual_meshes.avv, compiler/vismesh.py) against the instances the
// model blob carries.  From then on avsim_render_rgb draws the visual meshes (option "render_proxies" 1: the collision proxies again).
int avsim_load_visual(avsim_t* h, const void* library_blob, size_t nbytes) {
    if (!h || !library_blob) { if (h) h->set_error("avsim_load_visual: bad arguments"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    try {
        Blob lib(library_blob, nbytes);
        h->vis.load(lib, h->render.m.nbody, h->render.m.cam_pos, h->render.m.cam_mat, h->render.m.cam_fovy, h->render.m.cam_body, h->render.m.light, h->render.m.znear);
    } catch (const std::exception& e) {
        h->set_error("avsim_load_visual: %s", e.what());
        return AVSIM_EMODEL;
    }
    return AVSIM_OK;
}
// triangles / vertices of the loaded visual scene (0 when none is loaded); overflow flags of the last visual render: bit 0 a view ran
// out of triangle records, bit 1 out of tile-list entries (the image then lacks triangles); synchronises the stream
int avsim_visual_info(avsim_t* h, int32_t info[4]) {
    if (!h || !info) return AVSIM_EINVAL;
    AVS_ON_DEVICE(h);
    info[0] = h->vis.loaded ? h->vis.S.ntri : 0; info[1] = h->vis.loaded ? h->vis.S.nvert : 0; info[2] = 0; info[3] = h->vis.have_inst ? (int)h->vis.inst_mesh.size() : 0;
    if (h->vis.loaded && h->vis.X.flags && h->vis.last_nviews > 0) {      // the views of the LAST launch only: rows beyond them hold an earlier, larger call's flags
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<int> f((size_t)h->vis.last_nviews * 8);
        HIPCHK(h, hipMemcpy(f.data(), h->vis.X.flags, f.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t v = 0; v < f.size(); v += 8) info[2] |= f[v];
    }
    return AVSIM_OK;
}

// debug: per-view records of the last visual render, int32[nviews][8] = {overflow bits, cycles / 1024 of the stages transform, set-up,
// count, fill, tiles, triangle records, tile-list entries}; nviews = num_envs x cameras of that call
int avsim_visual_profile(avsim_t* h, int32_t* out, int nviews) {
    if (!h || !out || nviews < 0 || nviews > h->vis.nviews_cap || !h->vis.X.flags) { if (h) h->set_error("avsim_visual_profile: no visual render of that size yet"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->vis.X.flags, (size_t)nviews * 8 * sizeof(int), hipMemcpyDeviceToHost));
    return AVSIM_OK;
}

int avsim_camera_count(const avsim_t* h) { return h ? h->render.m.ncam : 0; }

// R1 (env.py:425-863, get_reward x5) on caller-supplied contact lists: the class-bit predicate the step kernel applies
// to its own contacts (reward_pair_flags / reward_from_flags), one thread per list; host pointers
int avsim_reward_from_pairs(avsim_t* h, const int32_t* geom_pairs, int nsets, int cap, int32_t* latch, int32_t* reward) {
    if (!h || (!geom_pairs && cap > 0) || !reward || nsets < 0 || cap < 0) { if (h) h->set_error("avsim_reward_from_pairs: bad arguments"); return AVSIM_EINVAL; }
    if (nsets == 0) return AVSIM_OK;
    AVS_ON_DEVICE(h);
    DevBuf buf;
    const size_t pb = sizeof(int) * (size_t)nsets * (cap ? cap : 1) * 2, nb = sizeof(int) * (size_t)nsets;
    HIPCHK(h, buf.alloc(pb + 2 * nb));
    int *const dp = buf.as<int>(), *const dl = dp + (pb / sizeof(int)), *const dr = dl + nsets;
    hipError_t e = hipSuccess;
    if (cap) e = hipMemcpyAsync(dp, geom_pairs, sizeof(int) * (size_t)nsets * cap * 2, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = latch ? hipMemcpyAsync(dl, latch, nb, hipMemcpyHostToDevice, h->stream) : hipMemsetAsync(dl, 0, nb, h->stream);
    if (e == hipSuccess) {
        GLB_PTR(const int) gc = h->phys.f64 ? h->phys.md.geom_class : h->phys.mf.geom_class;
        const int ng = h->phys.f64 ? h->phys.md.ngeom : h->phys.mf.ngeom, task = h->phys.f64 ? h->phys.md.task_id : h->phys.mf.task_id;
        hipLaunchKernelGGL(k_reward_pairs, dim3((nsets + 255) / 256), dim3(256), 0, h->stream, gc, ng, task, dp, nsets, cap, dl, dr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(reward, dr, nb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && latch) e = hipMemcpyAsync(latch, dl, nb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->set_error("avsim_reward_from_pairs: %s", hipGetErrorString(e)); return AVSIM_EHIP; }
    return AVSIM_OK;
}

}  // extern "C"

// ---- per-env episodes (avsim_episode.hip.h) ----------------------------------------------------------------------------------------
template <typename real>
static void ep_launch(avsim_t* h, int mode, const uint8_t* mask, double* ap, int* rw, uint8_t* su, uint8_t* te, uint8_t* tr, int64_t* id, int* el) {
    EpArgs A = h->ep;
    A.obs_off = h->f64 ? (const void*)(const double*)h->phys.md.obs_offset : (const void*)(const float*)h->phys.mf.obs_offset;
    A.obs_scale = h->f64 ? (const void*)(const double*)h->phys.md.obs_scale : (const void*)(const float*)h->phys.mf.obs_scale;
    A.obs_qposadr = h->f64 ? (const int*)h->phys.md.obs_qposadr : (const int*)h->phys.mf.obs_qposadr;
    hipLaunchKernelGGL(k_episode<real>, dim3(1), dim3(EP_THREADS), 0, h->stream, A, mode, mask, (const int*)h->phys.d_diag, (real*)h->d_qpos, (real*)h->d_qvel,
                       (real*)h->d_ctrl, (real*)h->d_warm, h->d_latch, ap, rw, su, te, tr, id, el);
}

extern "C" {

int avsim_episode_setup(avsim_t* h, const double* box, const int32_t* share, uint64_t seed, int max_episode_steps, int terminate_on_success,
                        int64_t log_capacity) {
    if (!h || !box || !share || max_episode_steps < 1 || log_capacity < 0) { if (h) h->set_error("avsim_episode_setup: bad arguments"); return AVSIM_EINVAL; }
    if (h->nobj > EP_MAXOBJ) { h->set_error("avsim_episode_setup: at most %d free objects", EP_MAXOBJ); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (buffers of an earlier set-up may still be in use)
    h->ep_arena.clear();
    h->ep_ready = false;
    const size_t N = h->N, no = h->nobj, L = (size_t)log_capacity;
    EpArgs& A = h->ep;
    A = EpArgs{};
    A.N = h->N; A.nq = h->nq; A.nv = h->nv; A.nu = h->nu; A.nj = h->nj; A.nobj = h->nobj;
    A.max_steps = max_episode_steps; A.term_on_success = terminate_on_success != 0; A.seed = seed; A.log_cap = log_capacity;
    A.qhome = h->phys.d_qpos_home; A.chome = h->phys.d_ctrl_home; A.objadr = h->phys.d_obj_qadr; A.obj_reset = h->phys.d_obj_reset;
#define EPA(field, T, n) do { if (!(field = (T*)h->ep_arena.get(sizeof(T) * (n)))) { h->set_error("avsim_episode_setup: hipMalloc(%zu) failed", sizeof(T) * (n)); return AVSIM_EHIP; } } while (0)
    EPA(A.id, int64_t, N); EPA(A.elapsed, int, N); EPA(A.maxr, int, N); EPA(A.ret, double, N); EPA(A.succ, uint8_t, N); EPA(A.pending, uint8_t, N);
    EPA(A.log_ret, double, L); EPA(A.log_obj, double, L * no * 7); EPA(A.log_len, int, L); EPA(A.log_maxr, int, L); EPA(A.log_succ, uint8_t, L);
    EPA(A.count, int64_t, 2);
    EPA(h->ep_ap, double, N * h->nj); EPA(h->ep_rw, int, N); EPA(h->ep_el, int, N); EPA(h->ep_su, uint8_t, N); EPA(h->ep_te, uint8_t, N);
    EPA(h->ep_tr, uint8_t, N); EPA(h->ep_id, int64_t, N);
#undef EPA
    for (size_t o = 0; o < no; o++) {
        for (int k = 0; k < 6; k++) A.box[6 * o + k] = box[6 * o + k];
        A.share[o] = share[o];
    }
    // no episode yet: every env starts one at its first avsim_episode_step (or avsim_episode_reset); id -1 until then
    HIPCHK(h, hipMemsetAsync(A.id, 0xff, sizeof(int64_t) * N, h->stream));
    HIPCHK(h, hipMemsetAsync(A.pending, 1, N, h->stream));
    for (auto q : {(void*)A.elapsed, (void*)A.maxr}) HIPCHK(h, hipMemsetAsync(q, 0, sizeof(int) * N, h->stream));
    HIPCHK(h, hipMemsetAsync(A.ret, 0, sizeof(double) * N, h->stream));
    HIPCHK(h, hipMemsetAsync(A.succ, 0, N, h->stream));
    HIPCHK(h, hipMemsetAsync(A.count, 0, 2 * sizeof(int64_t), h->stream));
    if (L) {
        HIPCHK(h, hipMemsetAsync(A.log_len, 0, sizeof(int) * L, h->stream));
        HIPCHK(h, hipMemsetAsync(A.log_maxr, 0, sizeof(int) * L, h->stream));
        HIPCHK(h, hipMemsetAsync(A.log_succ, 0, L, h->stream));
        HIPCHK(h, hipMemsetAsync(A.log_ret, 0, sizeof(double) * L, h->stream));
        HIPCHK(h, hipMemsetAsync(A.log_obj, 0, sizeof(double) * L * no * 7, h->stream));
    }
    h->ep_ready = true;
    return Call(h).done();
}

int avsim_sample_poses(avsim_t* h, uint64_t seed, int n, const int64_t* episode_id, double* obj_qpos) {
    if (!h || n < 0 || (n && (!episode_id || !obj_qpos))) { if (h) h->set_error("avsim_sample_poses: bad arguments"); return AVSIM_EINVAL; }
    if (!h->ep_ready) { h->set_error("avsim_sample_poses: call avsim_episode_setup first"); return AVSIM_EINVAL; }
    if (n == 0) return AVSIM_OK;
    AVS_ON_DEVICE(h);
    Call io(h);
    const int64_t* did = io.in(episode_id, sizeof(int64_t) * (size_t)n);
    double* dout = io.out(obj_qpos, sizeof(double) * (size_t)n * h->nobj * 7);
    if (io.failed()) return AVSIM_EHIP;
    hipLaunchKernelGGL(k_sample_poses, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->ep, seed, n, did, dout);
    HIPCHK(h, hipGetLastError());
    return io.done();
}

int avsim_episode_reset(avsim_t* h, const uint8_t* mask, double* agent_pos, int64_t* episode_id) {
    if (!h) return AVSIM_EINVAL;
    if (!h->ep_ready) { h->set_error("avsim_episode_reset: call avsim_episode_setup first"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    h->state_ver++;
    const size_t N = h->N;
    Call io(h);
    const uint8_t* dm = io.in(mask, N);
    // (an output nobody asked for goes to the handle's own buffer: the kernel writes them all)
    double* dap = io.out(agent_pos, sizeof(double) * N * h->nj, h->ep_ap);
    int64_t* did = io.out(episode_id, sizeof(int64_t) * N, h->ep_id);
    if (io.failed()) return AVSIM_EHIP;
    if (h->f64) ep_launch<double>(h, 0, dm, dap, nullptr, nullptr, nullptr, nullptr, did, nullptr);
    else ep_launch<float>(h, 0, dm, dap, nullptr, nullptr, nullptr, nullptr, did, nullptr);
    HIPCHK(h, hipGetLastError());
    return io.done();
}

int avsim_episode_step(avsim_t* h, const float* action, int nsub, double* agent_pos, int32_t* reward, uint8_t* success, uint8_t* terminated,
                       uint8_t* truncated, int64_t* episode_id, int32_t* elapsed) {
    if (!h || !action || nsub < 0) { if (h) h->set_error("avsim_episode_step: bad arguments"); return AVSIM_EINVAL; }
    if (!h->ep_ready) { h->set_error("avsim_episode_step: call avsim_episode_setup first"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const size_t N = h->N;
    Call io(h);
    const float* da = io.in(action, sizeof(float) * N * h->nj);
    double* dap = io.out(agent_pos, sizeof(double) * N * h->nj, h->ep_ap);
    int32_t* drw = io.out(reward, sizeof(int32_t) * N, h->ep_rw);
    uint8_t* dsu = io.out(success, N, h->ep_su);
    uint8_t* dte = io.out(terminated, N, h->ep_te);
    uint8_t* dtr = io.out(truncated, N, h->ep_tr);
    int64_t* did = io.out(episode_id, sizeof(int64_t) * N, h->ep_id);
    int32_t* del = io.out(elapsed, sizeof(int32_t) * N, h->ep_el);
    if (io.failed()) return AVSIM_EHIP;
    // the physics launch of avsim_step (it also steps the envs that start an episode below; k_episode overwrites them)
    h->state_ver++;
    if (int rc = step_common(h, da, nsub, dap, drw, dsu)) return rc;
    if (h->f64) ep_launch<double>(h, 1, nullptr, dap, drw, dsu, dte, dtr, did, del);
    else ep_launch<float>(h, 1, nullptr, dap, drw, dsu, dte, dtr, did, del);
    HIPCHK(h, hipGetLastError());
    return io.done();
}

// Records and counters out: device pointers in device mode, or host pointers in either mode (a poll from the host); only a copy to host
// memory synchronises the stream
static bool ep_host_ptr(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return true; }      // (memory HIP does not know: pageable host memory)
    return a.type != hipMemoryTypeDevice;
}
static int ep_copy(avsim_t* h, void* dst, const void* src, size_t bytes, bool* to_host) {
    if (!dst || !bytes) return 0;
    const bool host = !h->io_device || ep_host_ptr(dst);
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    *to_host = *to_host || host;
    return 0;
}

int avsim_episode_log(avsim_t* h, int64_t n, double* ret, int32_t* length, int32_t* max_reward, uint8_t* success, double* obj_qpos0) {
    if (!h || n < 0) { if (h) h->set_error("avsim_episode_log: bad arguments"); return AVSIM_EINVAL; }
    if (!h->ep_ready || n > h->ep.log_cap) { h->set_error("avsim_episode_log: %lld records asked, %lld kept (avsim_episode_setup)", (long long)n, (long long)h->ep.log_cap); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const size_t m = (size_t)n;
    int rc;
    bool host = false;
    if ((rc = ep_copy(h, ret, h->ep.log_ret, sizeof(double) * m, &host))) return rc;
    if ((rc = ep_copy(h, length, h->ep.log_len, sizeof(int32_t) * m, &host))) return rc;
    if ((rc = ep_copy(h, max_reward, h->ep.log_maxr, sizeof(int32_t) * m, &host))) return rc;
    if ((rc = ep_copy(h, success, h->ep.log_succ, m, &host))) return rc;
    if ((rc = ep_copy(h, obj_qpos0, h->ep.log_obj, sizeof(double) * m * h->nobj * 7, &host))) return rc;
    if (host) HIPCHK(h, hipStreamSynchronize(h->stream));
    return AVSIM_OK;
}

int avsim_episode_count(avsim_t* h, int64_t count[2]) {
    if (!h || !count) return AVSIM_EINVAL;
    if (!h->ep_ready) { h->set_error("avsim_episode_count: call avsim_episode_setup first"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    int rc;
    bool host = false;
    if ((rc = ep_copy(h, count, h->ep.count, 2 * sizeof(int64_t), &host))) return rc;
    if (host) HIPCHK(h, hipStreamSynchronize(h->stream));
    return AVSIM_OK;
}

}  // extern "C"

// ---- per-env execution of action chunks (av_aloha_amd/chunks.py is the specification; the kernels: csrc/avsim_chunks.hip, a unit of its own flags) ----
extern "C" {

int avsim_chunk_setup(avsim_t* h, int chunk_size, int action_dim, int mode, int n_action_steps, int first, const float* tables, const float* mean_std) {
    if (!h) return AVSIM_EINVAL;
    {
        std::string why;
        if (chunk_validate(chunk_size, action_dim, mode, n_action_steps, first, tables, mean_std, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (buffers of an earlier set-up may still be in use)
    if (h->chunks.setup(h->stream, h->N, chunk_size, action_dim, mode, n_action_steps, first, tables, mean_std, h->err)) return AVSIM_EHIP;
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (the tables are on the device: the caller's arrays are free)
    return AVSIM_OK;
}

int avsim_chunk_reset(avsim_t* h) {
    if (!h) return AVSIM_EINVAL;
    if (!h->chunks.ready) { h->set_error("avsim_chunk_reset: call avsim_chunk_setup first"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemsetAsync(h->chunks.P.stepped, 0, sizeof(int) * (size_t)h->N, h->stream));
    return Call(h).done();
}

int avsim_chunk_need(avsim_t* h, const int64_t* episode_id, const int32_t* elapsed, uint8_t* need, int32_t* any) {
    if (!h) return AVSIM_EINVAL;
    if (!h->chunks.ready) { h->set_error("avsim_chunk_need: call avsim_chunk_setup first"); return AVSIM_EINVAL; }
    if (!episode_id || !elapsed) { h->set_error("avsim_chunk_need: episode_id and elapsed are required"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const size_t N = h->N;
    Call io(h);
    const int64_t* did = io.in(episode_id, sizeof(int64_t) * N);
    const int32_t* del = io.in(elapsed, sizeof(int32_t) * N);
    uint8_t* dn = io.out(need, N);
    int32_t* da = io.out(any, sizeof(int32_t));
    if (io.failed()) return AVSIM_EHIP;
    chunk_launch_book(h->stream, h->chunks.P, 0, 0, did, del, dn, da);
    HIPCHK(h, hipGetLastError());
    return io.done();
}

int avsim_chunk_step(avsim_t* h, const float* chunks, const int64_t* episode_id, const int32_t* elapsed, float* action) {
    if (!h) return AVSIM_EINVAL;
    if (!h->chunks.ready) { h->set_error("avsim_chunk_step: call avsim_chunk_setup first"); return AVSIM_EINVAL; }
    if (!episode_id || !elapsed || !action) { h->set_error("avsim_chunk_step: episode_id, elapsed and action are required"); return AVSIM_EINVAL; }
    const ChunkArgs& P = h->chunks.P;
    if (!chunks && P.mode == CHK_ENSEMBLE) { h->set_error("avsim_chunk_step: ensemble mode needs a chunk in every call"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const size_t N = h->N;
    Call io(h);
    const float* dc = io.in(chunks, sizeof(float) * N * P.CA);
    const int64_t* did = io.in(episode_id, sizeof(int64_t) * N);
    const int32_t* del = io.in(elapsed, sizeof(int32_t) * N);
    float* dact = io.out(action, sizeof(float) * N * P.A);
    if (io.failed()) return AVSIM_EHIP;
    chunk_launch_step(h->stream, P, dc, did, del, dact);
    HIPCHK(h, hipGetLastError());
    return io.done();
}

int avsim_chunk_starved(avsim_t* h, uint64_t* count) {
    if (!h || !count) return AVSIM_EINVAL;
    if (!h->chunks.ready) { h->set_error("avsim_chunk_starved: call avsim_chunk_setup first"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(count, h->chunks.P.starved, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return AVSIM_OK;
}

}  // extern "C"

// ---- per-env observation histories (av_aloha_amd/obshist.py is the specification; the kernels: csrc/avsim_obshist.hip, a unit of its own flags) ----
extern "C" {

int avsim_obs_history_setup(avsim_t* h, int n_obs_steps, int state_dim, const float* state_mean_std, int ncam, int fmt, int height, int width, const float* lut,
                            const int32_t* box, int out_h, int out_w) {
    if (!h) return AVSIM_EINVAL;
    {
        std::string why;
        if (obs_validate(n_obs_steps, state_dim, state_mean_std, ncam, fmt, height, width, lut, box, out_h, out_w, why)) { h->set_error("%s", why.c_str()); return AVSIM_EINVAL; }
    }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (buffers of an earlier set-up may still be in use)
    if (h->obshist.setup(h->stream, h->N, n_obs_steps, state_dim, state_mean_std, ncam, fmt, height, width, lut, box, out_h, out_w, h->err)) return AVSIM_EHIP;
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (the tables are on the device: the caller's arrays are free)
    return AVSIM_OK;
}

int avsim_obs_history_reset(avsim_t* h) {
    if (!h) return AVSIM_EINVAL;
    if (!h->obshist.ready) { h->set_error("avsim_obs_history_reset: call avsim_obs_history_setup first"); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    HIPCHK(h, hipMemsetAsync(h->obshist.P.pushed, 0, sizeof(int) * (size_t)h->N, h->stream));
    return Call(h).done();
}

int avsim_obs_history_push(avsim_t* h, const int64_t* episode_id, const int32_t* elapsed, const float* state, float* state_hist, const void* const* img,
                           float* const* img_hist) {
    if (!h) return AVSIM_EINVAL;
    ObsHistHost& O = h->obshist;
    if (!O.ready) { h->set_error("avsim_obs_history_push: call avsim_obs_history_setup first"); return AVSIM_EINVAL; }
    const ObsArgs& P = O.P;
    if (!episode_id || !elapsed) { h->set_error("avsim_obs_history_push: episode_id and elapsed are required"); return AVSIM_EINVAL; }
    if (P.D > 0 && (!state || !state_hist)) { h->set_error("avsim_obs_history_push: state and state_hist are required (state_dim %d)", P.D); return AVSIM_EINVAL; }
    if (P.ncam > 0 && (!img || !img_hist)) { h->set_error("avsim_obs_history_push: img and img_hist are required (%d cameras)", P.ncam); return AVSIM_EINVAL; }
    for (int c = 0; c < P.ncam; c++)
        if (!img[c] || !img_hist[c]) { h->set_error("avsim_obs_history_push: camera %d: a NULL pointer", c); return AVSIM_EINVAL; }
    AVS_ON_DEVICE(h);
    const size_t N = h->N, K = P.K;
    // a host caller's histories cross twice per call (for tests and numpy callers)
    Call io(h);
    const int64_t* did = io.in(episode_id, sizeof(int64_t) * N);
    const int32_t* del = io.in(elapsed, sizeof(int32_t) * N);
    const float* dstate = P.D > 0 ? io.in(state, sizeof(float) * N * P.D) : nullptr;
    float* dshist = P.D > 0 ? io.inout(state_hist, sizeof(float) * N * K * P.D) : nullptr;
    ObsPtrs Q{};
    for (int c = 0; c < P.ncam; c++) {
        Q.img[c] = io.in(img[c], N * P.SH * P.SW * img_bpp(P.fmt));
        Q.hist[c] = io.inout(img_hist[c], sizeof(float) * N * K * 3 * P.oh * P.ow);
    }
    if (io.failed()) return AVSIM_EHIP;
    obs_launch_push(h->stream, P, Q, did, del, dstate, dshist);
    HIPCHK(h, hipGetLastError());
    return io.done();
}

}  // extern "C"

// avsim_episode.hip.h -- per-env episodes on the device (avsim_episode_*): initial object poses from a counter-based RNG, episode ids,
// gymnasium's NEXT_STEP autoreset and one record per finished episode, so that a vector env never leaves the device between steps.
//
// Initial poses: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), key = the seed, counter =
// (episode id, object index, 0).  They depend on (seed, episode id) only -- not on the batch size, the env slot or when other envs
// reset.  Every kernel here is templated on the physics precision (float, or double with AVSIM_F64_PHYSICS).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace avs {

struct Philox4 { uint32_t v[4]; };

// Random123's philox4x32 with 10 rounds (tests/test_vec_env_host.py restates it in numpy and checks the published answers)
__host__ __device__ inline Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.v[0], p1 = (uint64_t)0xCD9E8D57u * c.v[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c = Philox4{{hi1 ^ c.v[1] ^ k0, lo1, hi0 ^ c.v[3] ^ k1, lo0}};
    }
    return c;
}

constexpr int EP_MAXOBJ = 4;

struct EpArgs {
    int N, nq, nv, nu, nj, nobj, max_steps, term_on_success;
    uint64_t seed;
    int64_t log_cap;
    double box[EP_MAXOBJ * 6];    // [nobj][6] = lo xyz, hi xyz (kernel arguments: the set-up copies nothing to the device)
    int share[EP_MAXOBJ];         // [nobj]: -1, or an earlier object whose position this one takes
    const double *qhome, *chome;
    const int *objadr, *obs_qposadr;
    const void *obs_off, *obs_scale;       // real[nj] (the physics model's own copies: agent_pos rounds as k_phys's does)
    double* obj_reset;        // PhysHost::d_obj_reset [N][nobj][7]
    // per env
    int64_t* id;
    int *elapsed, *maxr;
    double* ret;
    uint8_t *succ, *pending;
    // records, indexed by episode id < log_cap
    double *log_ret, *log_obj;
    int *log_len, *log_maxr;
    uint8_t* log_succ;
    int64_t* count;           // [2] started, finished
};

// [x y z qw qx qy qz] of every free object for episode `id`: u = (x + 0.5) 2^-32, pos = lo + (hi - lo) u, each operation rounded on its own.
// avsim_api is compiled with FP contraction on, which fuses even __dmul_rn / __dadd_rn once they are inlined (measured: 1 ulp off the numpy
// restatement in a third of the draws): contraction is off in this function
__host__ __device__ inline void ep_sample(const double* box, const int* share, int nobj, uint64_t seed, int64_t id, double* out) {
#pragma clang fp contract(off)
    for (int o = 0; o < nobj; o++) {
        double* p = out + 7 * o;
        const int sh = share[o];
        if (sh >= 0 && sh < o) {
            for (int k = 0; k < 3; k++) p[k] = out[7 * sh + k];
        } else {
            const Philox4 x = philox4x32_10(Philox4{{(uint32_t)(uint64_t)id, (uint32_t)((uint64_t)id >> 32), (uint32_t)o, 0u}}, (uint32_t)seed, (uint32_t)(seed >> 32));
            for (int k = 0; k < 3; k++) {
                const double u = ((double)x.v[k] + 0.5) * 0x1p-32;
                const double lo = box[6 * o + k], hi = box[6 * o + 3 + k];
                p[k] = lo + (hi - lo) * u;
            }
        }
        p[3] = 1.0; p[4] = 0.0; p[5] = 0.0; p[6] = 0.0;
    }
}

// the state of a fresh episode, as avsim_reset writes it (k_reset): home qpos with the objects at obj[nobj][7], zero qvel / warmstart,
// home ctrl, latch 0; obj_keep = the poses a diverged env of this episode is put back to
template <typename real>
__device__ inline void reset_env(int i, int nq, int nv, int nu, int nobj, const double* __restrict__ obj, const double* __restrict__ qhome,
                                 const double* __restrict__ chome, const int* __restrict__ objadr, real* qpos, real* qvel, real* ctrl, real* warm,
                                 int* latch, double* obj_keep) {
    for (int k = 0; k < nq; k++) qpos[(size_t)i * nq + k] = (real)qhome[k];
    for (int o = 0; o < nobj; o++)
        for (int k = 0; k < 7; k++) {
            const double v = obj[o * 7 + k];
            qpos[(size_t)i * nq + objadr[o] + k] = (real)v;
            obj_keep[((size_t)i * nobj + o) * 7 + k] = v;      // where a diverged env of this episode is put back (check_divergence)
        }
    for (int k = 0; k < nv; k++) { qvel[(size_t)i * nv + k] = 0; warm[(size_t)i * nv + k] = 0; }
    for (int k = 0; k < nu; k++) ctrl[(size_t)i * nu + k] = (real)chome[k];
    latch[i] = 0;
}

// agent_pos of env i from its qpos: the gather of k_phys (obs_qposadr, with the right_right_finger quirk; grippers normalised)
template <typename real>
__device__ inline void ep_agent_pos(const EpArgs& A, int i, const real* qpos, double* ap) {
    const real* off = (const real*)A.obs_off;
    const real* sc = (const real*)A.obs_scale;
    for (int k = 0; k < A.nj; k++) ap[(size_t)i * A.nj + k] = ((double)qpos[(size_t)i * A.nq + A.obs_qposadr[k]] - (double)off[k]) * (double)sc[k];
}

__global__ void k_sample_poses(EpArgs A, uint64_t seed, int n, const int64_t* __restrict__ ids, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ep_sample(A.box, A.share, A.nobj, seed, ids[i], out + (size_t)i * A.nobj * 7);
}

constexpr int EP_THREADS = 1024;

// One workgroup walks the batch in chunks of 1024 envs, so that the envs that start an episode in this call take consecutive ids in
// env-index order (an exclusive scan of the start flags over the chunk, carried from chunk to chunk): no two starts race for an id.
//   mode 0 (avsim_episode_reset): envs with mask[i] (NULL: all) start an episode now; the others only report agent_pos and their id.
//   mode 1 (avsim_episode_step, after the physics launch, whose agent_pos / reward / success are in o_ap / o_rw / o_su):
//     an env whose previous episode ended (pending) starts its new one -- the step the launch just took is overwritten, the action of
//     this call never reaches the new episode -- and reports reward 0, flags 0, elapsed 0, its new id and the new state's agent_pos;
//     the others book the step: elapsed, return, max reward, success seen; truncated = elapsed reached max_steps or the launch put the
//     env back after a divergence (diag bit 0), terminated = term_on_success && success; an env that ends is pending for the next call
//     and writes its record when its id < log_cap.
template <typename real>
__global__ void __launch_bounds__(EP_THREADS) k_episode(EpArgs A, int mode, const uint8_t* __restrict__ mask, const int* __restrict__ diag,
                                                        real* qpos, real* qvel, real* ctrl, real* warm, int* latch, double* o_ap, int* o_rw,
                                                        uint8_t* o_su, uint8_t* o_term, uint8_t* o_trunc, int64_t* o_id, int* o_elapsed) {
    __shared__ int wsum[EP_THREADS / 64];
    __shared__ long long base_s, fin_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { base_s = A.count[0]; fin_s = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < A.N; c0 += EP_THREADS) {
        const int i = c0 + tid;
        const bool live = i < A.N;
        const bool start = live && (mode == 0 ? (!mask || mask[i]) : A.pending[i] != 0);
        const unsigned long long b = __ballot(start);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        long long id = base_s;
        int total = 0;
        for (int w = 0; w < EP_THREADS / 64; w++) { if (w < wave) id += wsum[w]; total += wsum[w]; }
        id += before;
        if (start) {
            double obj[EP_MAXOBJ * 7];
            ep_sample(A.box, A.share, A.nobj, A.seed, id, obj);
            reset_env<real>(i, A.nq, A.nv, A.nu, A.nobj, obj, A.qhome, A.chome, A.objadr, qpos, qvel, ctrl, warm, latch, A.obj_reset);
            A.id[i] = id; A.elapsed[i] = 0; A.maxr[i] = 0; A.ret[i] = 0.0; A.succ[i] = 0; A.pending[i] = 0;
            if (o_ap) ep_agent_pos<real>(A, i, qpos, o_ap);
            if (o_rw) o_rw[i] = 0;
            if (o_su) o_su[i] = 0;
            if (o_term) o_term[i] = 0;
            if (o_trunc) o_trunc[i] = 0;
            if (o_elapsed) o_elapsed[i] = 0;
            if (o_id) o_id[i] = id;
        } else if (live && mode == 0) {
            if (o_ap) ep_agent_pos<real>(A, i, qpos, o_ap);
            if (o_id) o_id[i] = A.id[i];
        } else if (live) {
            const int rw = o_rw[i];
            const bool su = o_su[i] != 0;
            const int el = A.elapsed[i] + 1;
            const double ret = A.ret[i] + (double)rw;
            const int mr = rw > A.maxr[i] ? rw : A.maxr[i];
            const bool seen = A.succ[i] || su;
            const bool trunc = el >= A.max_steps || (diag[4 * i + 3] & 1);
            const bool term = A.term_on_success && su;
            A.elapsed[i] = el; A.ret[i] = ret; A.maxr[i] = mr; A.succ[i] = seen ? 1 : 0;
            if (o_term) o_term[i] = term ? 1 : 0;
            if (o_trunc) o_trunc[i] = trunc ? 1 : 0;
            if (o_elapsed) o_elapsed[i] = el;
            const int64_t eid = A.id[i];
            if (o_id) o_id[i] = eid;
            if (term || trunc) {
                A.pending[i] = 1;
                atomicAdd((unsigned long long*)&fin_s, 1ull);
                if (eid >= 0 && eid < A.log_cap) {
                    A.log_ret[eid] = ret; A.log_len[eid] = el; A.log_maxr[eid] = mr; A.log_succ[eid] = seen ? 1 : 0;
                    for (int k = 0; k < A.nobj * 7; k++) A.log_obj[(size_t)eid * A.nobj * 7 + k] = A.obj_reset[(size_t)i * A.nobj * 7 + k];
                }
            }
        }
        __syncthreads();          // (every lane has read wsum and base_s)
        if (tid == 0) base_s += total;
        __syncthreads();
    }
    if (tid == 0) { A.count[0] = base_s; A.count[1] += fin_s; }
}

}  // namespace avs

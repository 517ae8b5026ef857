// avsim_phys_layout.h -- where the physics kernel keeps things in LDS: the per-env record (Layout) and the offsets of the model
// tables inside the block's table image (MOff).  Plain C++ (no HIP): the host computes a handle's layout with make_layout_of at run
// time, and a kernel specialised for one model (avsim_phys_specs.h, avsim_phys_spec.hip) evaluates the SAME function at compile
// time, so the two cannot drift.
#pragma once

namespace avs {

constexpr int RS_S = 9;            // solver record: 8 words used
constexpr int ANC_MAX = 64;        // LDS ints of the kinematics' pointer-jumping table (one per body)
constexpr int NARROW_SCR_W = 64 * 24 + 4 * 56;   // narrow phase: 64 result slots (SLOT_W words each) + 4 box work areas

// The table image: the hot model tables that every block copies into LDS, ints and reals apart.  These two lists ARE the image, in image
// order: MOff, Env's accessors X_() (avsim_phys.hip.h) and PhysHost::build's check that every table was filled come from them.  A new
// table is one entry here and one fill line in PhysHost::build (plus its pointer in DevModelT).
#define AVSIM_IMG_INT_TABLES(X) \
    X(body_parent) X(body_jntadr) X(body_jntnum) X(body_dofadr) X(body_dofnum) X(body_tree) X(body_dofmask) X(body_last) \
    X(tree_bodyadr) X(tree_bodylist) X(tree_dofadr) X(tree_dofnum) X(tree_madr) X(jnt_type) X(jnt_qposadr) X(jnt_dofadr) \
    X(jnt_actfrclimited) X(limited_jnt) X(dof_body) X(dof_parent) X(dof_tree) X(dof_jnt) X(floss_dof) X(ment_i) X(ment_j) \
    X(act_dof) X(act_qposadr) X(act_ctrllimited) X(geom_type) X(geom_body) X(geom_static)
#define AVSIM_IMG_REAL_TABLES(X) \
    X(body_pos) X(body_quat) X(body_mass) X(body_ipos) X(body_inertia) X(body_invweight0) X(jnt_pos) X(jnt_axis) X(jnt_range) \
    X(jnt_actfrcrange) X(jnt_margin) X(dof_armature) X(dof_damping) X(dof_frictionloss) X(dof_invweight0) X(act_kp) X(act_kv) \
    X(act_gear) X(act_ctrlrange) X(geom_cpos) X(geom_rbound)

// where each table starts in its half of the image (in words of that half; -1: not filled -- PhysHost::build refuses to leave one so);
// nreal / nint: the halves' sizes, multiples of four
struct MOff {
    int nreal = 0, nint = 0;
#define AVSIM_MOFF_MEMBER(x) int x = -1;
    AVSIM_IMG_INT_TABLES(AVSIM_MOFF_MEMBER)
    AVSIM_IMG_REAL_TABLES(AVSIM_MOFF_MEMBER)
#undef AVSIM_MOFF_MEMBER
};
constexpr int MOFF_WORDS = sizeof(MOff) / sizeof(int);

// per-env LDS layout (offsets in reals / ints)
struct Layout {
    int qpos, qvel, ctrl, warm, xpos, xmat, xipos, cdof, gcen, M, L, Minv, bias, fsm, asm_, qacc, fcon, nH, ng, ndl, njv, U, nreal;
    // scratch union U, phase A
    int cinert, cvel, cacc, cfrc, binert;   // binert: the bodies' own spatial inertias (cinert becomes the composites)
    // phase B
    int cdist, cpos, cnrm, rowS, scr;   // scr: narrow-phase scratch (overlays rowS: NARROW_SCR_W words = 64 result slots of SLOT_W words + 4 box work areas)
    // ints
    int cand, cpair, cefc, rmeta, rowI, gI, misc, nprof, nint;
    int maxgrp;
    int maxcon, maxefc;
    int expcon;                   // stride of the contact export arrays (the full capacity, whatever this layout's own)
    int gefc, ggrp;               // rows / groups per env in the global scratch (the full capacities)
    int bytes_per_env;
};
constexpr int LAYOUT_WORDS = sizeof(Layout) / sizeof(int);

// The layout of an env's record for the capacities (maxcon, maxefc) of one tier; full_maxcon / full_maxefc are the handle's full
// capacities (the strides of the contact export and of the global row scratch, the same in both tiers).  Pure arithmetic.
constexpr Layout make_layout_of(int maxcon, int maxefc, int full_maxcon, int full_maxefc, int nq, int nv, int nu, int nb, int ng, int msize,
                                int ntree, int real_bytes) {
    Layout L{};
    int o = 0;
    L.qpos = o; o += nq; L.qvel = o; o += nv; L.ctrl = o; o += nu; L.warm = o; o += nv;
    L.xpos = o; o += 3 * nb; L.xmat = o; o += 9 * nb; L.xipos = o; o += 3 * nb; L.cdof = o; o += 6 * nv; L.gcen = o; o += 3 * ng;
    L.M = o; o += msize; L.L = o; o += msize; o = (o + 3) & ~3; L.Minv = o; o += 64 * ntree;
    L.bias = o; o += nv; L.fsm = o; o += nv; L.asm_ = o; o += nv; L.qacc = o; o += nv; L.fcon = o; o += nv;
    // Newton scratch (packed Hessian, gradient, direction, per-row J.dl) lives over xpos..gcen where it fits: every
    // position-derived quantity is dead between make_constraints and the next substep's kinematics
    {
        const int nvh = nv * (nv + 1) / 2, need1 = nvh + 2 * nv, need2 = need1 + maxefc, avail = 15 * nb + 6 * nv + 3 * ng;
        int base = L.xpos;
        if (!(need1 <= avail)) { base = o; o += need1; }
        L.nH = base; L.ng = base + nvh; L.ndl = L.ng + nv;
        if (need2 <= avail) L.njv = L.ndl + nv;
        else { L.njv = o; o += maxefc; }
    }
    L.U = o;
    int a = o;
    L.cinert = a; a += 10 * nb; L.binert = a; a += 10 * nb; L.cvel = a; a += 6 * nb; L.cacc = a; a += 6 * nb; L.cfrc = a; a += 6 * nb;
    int bq = o;
    L.cdist = bq; bq += maxcon; L.cpos = bq; bq += 3 * maxcon; L.cnrm = bq; bq += 3 * maxcon;
    bq = (bq + 3) & ~3; L.rowS = bq; L.scr = bq; bq += RS_S * maxefc;
    L.maxgrp = maxefc / 3 + 8;
    if (bq < L.scr + NARROW_SCR_W) bq = L.scr + NARROW_SCR_W;
    o = a > bq ? a : bq;
    L.nreal = (o + 3) & ~3;
    int io = 0;
    L.cand = io; io += ANC_MAX; L.cpair = io; io += maxcon; L.cefc = io; io += maxcon; L.rmeta = io; io += maxefc; L.rowI = io; io += maxefc;
    L.gI = io; io += maxefc / 3 + 8; L.misc = io; io += 12; L.nprof = io; io += 16;
    L.nint = (io + 3) & ~3;
    L.maxcon = maxcon;
    L.maxefc = maxefc;
    L.expcon = full_maxcon;
    L.gefc = full_maxefc;
    L.ggrp = full_maxefc / 3 + 8;
    L.bytes_per_env = (int)(((unsigned long long)L.nreal * (unsigned)real_bytes + (unsigned long long)L.nint * 4 + 15) & ~15ull);
    return L;
}

// row / contact capacities per task (index: the blob's task_id): every box of a compound object resting on the condim-6 table
// contributes 4 contacts x 6 rows (SewNeedle 24 contacts / 128 rows, TubeTransfer 40 / 248 at rest)
// Two tiers where the smaller first one lets more envs share a CU (SewNeedle: 7 instead of 6 -- the scripted grasp of
// BASELINE config 3 reaches 194 rows / 35 contacts in most envs at once, so the first tier must hold that: with 176 rows,
// 8 per CU, nearly every env needed the full record during the grasp; TubeTransfer): the second pass costs a launch and,
// when its list is not empty, the latency of one env-step, so the other tasks keep one tier.
constexpr int CAP_EFC[5] = {176, 176, 336, 480, 176}, CAP_CON[5] = {48, 48, 72, 96, 48};
constexpr int CAP_EFC1[5] = {176, 176, 224, 288, 176}, CAP_CON1[5] = {48, 48, 56, 64, 48};

// ---- contact rows two per lane (Env::make_constraints_i; tests/test_rows_paired_host.py runs these on the host) ----
// A contact of dim rows (1, 3, 4 or 6) has up to three axes: axis s carries the contact's sub-row s and, where the contact has it,
// sub-row s + 3 -- the translational and the rotational row along one direction of the contact frame.  Item 3 c + s of a substep is
// axis s of contact c; the items are dealt to the wave's lanes 64 at a time like the rows are.
constexpr int row_trips(int n, int lanes) { return (n + lanes - 1) / lanes; }
// two rows per lane only where that takes FEWER trips than one row per lane: never more trips than the rows themselves need
constexpr bool rows_pair_pays(int ncon, int ncontact_rows, int lanes) { return row_trips(3 * ncon, lanes) < row_trips(ncontact_rows, lanes); }
// The rows of axis s of a contact whose row word is ce (first row | rows << 16; negative: the contact has no rows -- inactive, or cut
// off by the row cap): false = nothing to fill, else row0 = the table row of sub-row s and live1 = row0 + 3 (sub-row s + 3) exists too.
constexpr bool axis_rows(int ce, int s, int& row0, bool& live1) {
    const int first = ce & 0xffff, dim = ce >> 16;
    if (ce < 0 || s >= dim) return false;
    row0 = first + s;
    live1 = s + 3 < dim;
    return true;
}

}  // namespace avs

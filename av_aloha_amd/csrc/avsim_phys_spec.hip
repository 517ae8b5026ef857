// avsim_phys_spec.hip -- the one-pass f32 physics kernel compiled once more for each model of avsim_phys_specs.h, with that model's LDS
// layout, table offsets, dims and solver configuration as compile-time constants (KFixed in avsim_phys.hip.h): what the generic kernel
// fetches through `ka` in every phase of every substep -- where qpos lives, where the row records start, where body_parent sits in the
// table image -- is an immediate offset of the LDS instruction here, the trip counts of the loops over dofs, bodies and trees are
// numbers, and the solver paths a default handle does not take (PGS, the other QCQP and noslip variants) are not compiled in.  Its own translation unit, compiled next to avsim_api.hip with the same flags
// (av_aloha_amd/build.py); the build is -fno-gpu-rdc, so the kernels are reached through this unit's host stubs (phys_spec_kernel).
// Two-tier models (SewNeedle, TubeTransfer) and the f64 parity kernel stay generic.
#define AVSIM_NO_F32_LAUNCH 1      // the generic kernels are avsim_api.hip's
#include "avsim_phys.hip.h"
#include "avsim_phys_specs.h"

namespace avs {

const void* phys_spec_kernel(const PhysHost& ph, const char** name) {
    if (ph.f64 || ph.two_pass()) return nullptr;
#define AVSIM_SPEC_TRY(SPEC) \
    if (spec_matches<SPEC>(ph)) { if (name) *name = SPEC::name; return (const void*)k_phys<float, 64, AVSIM_PHYS_MAXW, false, SPEC>; }
    AVSIM_PHYS_SPECS(AVSIM_SPEC_TRY)
#undef AVSIM_SPEC_TRY
    return nullptr;
}

}  // namespace avs

// avsim_phys_spec.hip -- the one-pass f32 physics kernel compiled once more for each model of avsim_phys_specs.h, with that model's LDS
// layout and table offsets as compile-time constants (KFixed in avsim_phys.hip.h): what the generic kernel fetches through `ka` in
// every phase of every substep -- where qpos lives, where the row records start, where body_parent sits in the table image -- is an
// immediate offset of the LDS instruction here.  Its own translation unit, compiled next to avsim_api.hip with the same flags
// (av_aloha_amd/build.py); the build is -fno-gpu-rdc, so the kernels are reached through this unit's host stubs (phys_spec_kernel).
// Two-tier models (SewNeedle, TubeTransfer) and the f64 parity kernel stay generic.
#define AVSIM_NO_F32_LAUNCH 1      // the generic kernels are avsim_api.hip's
#include "avsim_phys.hip.h"
#include "avsim_phys_specs.h"

namespace avs {

template <typename SPEC>
static bool spec_matches(const PhysHost& ph) {
    static_assert(sizeof(Layout) == LAYOUT_WORDS * sizeof(int) && sizeof(MOff) == MOFF_WORDS * sizeof(int), "structs of ints, no padding");
    static constexpr Layout lay = SPEC::lay;
    static constexpr MOff mo = SPEC::mo;
    return std::memcmp(&ph.lay, &lay, sizeof(Layout)) == 0 && std::memcmp(&ph.lay2, &lay, sizeof(Layout)) == 0 &&
           std::memcmp(&ph.moff, &mo, sizeof(MOff)) == 0 && std::memcmp(ph.dims, SPEC::dims, sizeof(ph.dims)) == 0;
}

const void* phys_spec_kernel(const PhysHost& ph, const char** name) {
    if (ph.f64 || ph.two_pass()) return nullptr;
#define AVSIM_SPEC_TRY(SPEC) \
    if (spec_matches<SPEC>(ph)) { if (name) *name = SPEC::name; return (const void*)k_phys<float, 64, AVSIM_PHYS_MAXW, false, SPEC>; }
    AVSIM_PHYS_SPECS(AVSIM_SPEC_TRY)
#undef AVSIM_SPEC_TRY
    return nullptr;
}

}  // namespace avs

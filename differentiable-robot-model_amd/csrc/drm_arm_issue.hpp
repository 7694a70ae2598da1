// drm_arm_issue.hpp — the lock-step trig of the arm FK / Jacobian kernel's PRE form (drm_arm_kernels.hip), which exists to cut
// ISSUE SLOTS.
//
// At the metric's shape (Panda, 65 536 rows) every SIMD runs one lone wavefront, so an instruction that does no work is not hidden
// behind another wavefront's.  gfx950 wants a wait state between dependent packed-fp32 operations, and chain_trig's four sincos_pair
// evaluations, one after another, are each one dependent chain: the compiler fills them with s_nop (50 in the kernel).
// chain_trig_lockstep advances the (NJ + 1) / 2 evaluations one step at a time TOGETHER, so the independent chains fill each
// other's wait states (3 s_nop left).  Every element sees the same operations in the same order as in sincos_pair: the results are
// bit-identical (tests/test_arm_issue.py holds them to that on the host).  Measurements: profiles/metric_issue_slots.md.
// Compiles for the host as well (DRM_HD), like drm_sample.hpp.
#pragma once

#include "drm_sample.hpp"

namespace drm {

// cos / sin of the NJ joint angles of a chain: chain_trig (drm_sample.hpp) with its pair evaluations in lock step.
// Same escape to sincos_f for |x| > 1e5 or non-finite x, entered wave-uniformly and taken lane by lane; marked unlikely so that
// the fp64 reduction is laid out behind the straight-line code instead of in the middle of it.
template <int NJ>
DRM_HD void chain_trig_lockstep(const float (&q)[NJ], float (&cs)[NJ], float (&sn)[NJ]) {
    constexpr int NP = (NJ + 1) / 2;
    bool big = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) big = big || !(fabsf(q[d]) <= SINCOS_PAIR_MAX_ARG);
    if (__builtin_expect(DRM_WAVE_ANY(big), 0)) {
        // entered by the whole wavefront, but only the lanes that hold such an angle take sincos_f's values: the others keep the
        // packed evaluation's, bit for bit (as in chain_trig), so that a row never depends on the rows it shares a wavefront with
        // (Plain DRM_WAVE_ANY, not chain_trig's DRM_WAVE_ANY_RARE / DRM_RARE_COPY: their opaque asm on the common path cost this lone
        // wavefront 1.5 % of the 65 536-row launch, 3.81 against 3.75 us; as written here it measures the same as without the selection.)
        if (big) {
#pragma unroll
            for (int d = 0; d < NJ; ++d) sincos_f(q[d], sn[d], cs[d]);
        } else {
            chain_trig_packed<NJ>(q, cs, sn);
        }
        return;
    }
    // sincos_pair (drm_sample.hpp), statement by statement, over all NP pairs.  The constants and the operation order are a COPY:
    // an edit to sincos_pair must be mirrored here, and tests/test_arm_issue.py fails (bit patterns) until it is.
    const f2 magic = f2_bcast(12582912.0f);
    f2 x[NP], kb[NP], kf[NP], r[NP], z[NP], ps[NP], pc[NP], sr[NP], cr[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) x[p] = f2_make(q[2 * p], q[2 * p + 1 < NJ ? 2 * p + 1 : 2 * p]);
#pragma unroll
    for (int p = 0; p < NP; ++p) kb[p] = f2_fma(x[p], f2_bcast(0.318309886f), magic);
#pragma unroll
    for (int p = 0; p < NP; ++p) kf[p] = kb[p] - magic;
#pragma unroll
    for (int p = 0; p < NP; ++p) r[p] = f2_fma(kf[p], f2_bcast(-3.14159202e+00f), x[p]);
#pragma unroll
    for (int p = 0; p < NP; ++p) r[p] = f2_fma(kf[p], f2_bcast(-6.27832947e-07f), r[p]);
#pragma unroll
    for (int p = 0; p < NP; ++p) r[p] = f2_fma(kf[p], f2_bcast(-1.07806051e-14f), r[p]);
#pragma unroll
    for (int p = 0; p < NP; ++p) z[p] = r[p] * r[p];
#pragma unroll
    for (int p = 0; p < NP; ++p) ps[p] = z[p] * f2_bcast(-2.3776610902e-08f) + f2_bcast(2.7522166874e-06f);
#pragma unroll
    for (int p = 0; p < NP; ++p) ps[p] = z[p] * ps[p] + f2_bcast(-1.9840880122e-04f);
#pragma unroll
    for (int p = 0; p < NP; ++p) ps[p] = z[p] * ps[p] + f2_bcast(8.3333319053e-03f);
#pragma unroll
    for (int p = 0; p < NP; ++p) ps[p] = z[p] * ps[p] + f2_bcast(-1.6666667163e-01f);
#pragma unroll
    for (int p = 0; p < NP; ++p) sr[p] = (r[p] * z[p]) * ps[p] + r[p];
#pragma unroll
    for (int p = 0; p < NP; ++p) pc[p] = z[p] * f2_bcast(1.6759177379e-09f) + f2_bcast(-2.7332046670e-07f);
#pragma unroll
    for (int p = 0; p < NP; ++p) pc[p] = z[p] * pc[p] + f2_bcast(2.4796934667e-05f);
#pragma unroll
    for (int p = 0; p < NP; ++p) pc[p] = z[p] * pc[p] + f2_bcast(-1.3888848480e-03f);
#pragma unroll
    for (int p = 0; p < NP; ++p) pc[p] = z[p] * pc[p] + f2_bcast(4.1666664183e-02f);
#pragma unroll
    for (int p = 0; p < NP; ++p) pc[p] = z[p] * pc[p] + f2_bcast(-0.5f);
#pragma unroll
    for (int p = 0; p < NP; ++p) cr[p] = z[p] * pc[p] + f2_bcast(1.0f);
#pragma unroll
    for (int d = 0; d < NJ; ++d) {
        // (elements copied into scalars before the bit casts: see sincos_pair)
        const float kbi = kb[d / 2][d & 1], sri = sr[d / 2][d & 1], cri = cr[d / 2][d & 1];
        const uint32_t flip = __builtin_bit_cast(uint32_t, kbi) << 31;
        sn[d] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, sri) ^ flip);
        cs[d] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, cri) ^ flip);
    }
}

} // namespace drm

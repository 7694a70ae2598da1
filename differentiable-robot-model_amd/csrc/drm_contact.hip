// drm_contact.hip — plane contact of spheres on the links and joint-limit springs (csrc/drm_contact.hpp), as the joint torques of one
// state (drm_contact_torques) and inside a rollout (drm_contact_rollout): T steps of
//     qdd_t = FD(q_t, qd_t, tau[t] + tau_ext(q_t, qd_t) + tau_lim(q_t, qd_t))
// and an Euler integrator per launch (include/drm_hip.h).  drm_forward_dynamics_rollout cannot do this: its torques are fixed before
// the launch, and a contact force depends on the state of the step.
//
//   contact_torques_arm_kernel   serial 7-DoF arm chains of 8 ops, every op a contact link in walk order, full 64-row tiles, 16-byte
//                                aligned pointers: one wavefront per tile, one row per lane, the constant table staged in LDS once, ONE
//                                chain_trig, ONE sweep outwards with velocities that keeps the origins and axes, the law per link, one
//                                sweep inwards, the springs (drm_contact.hpp contact_chain_torques).  The [64, 7] tile of torques and,
//                                when asked for, the two [64, 8, 3] wrench tiles leave through LDS in 16-byte stores.
//   contact_torques_vjp_arm_kernel   drm_contact_torques_vjp under contact_torques_arm_kernel's condition: the cotangent of the
//                                torques beside q and qd (84 B in per row), ONE chain_trig, ONE sweep outwards that carries the
//                                velocities at rates qd and at rates grad_tau together with the law and its backward per link, ONE
//                                sweep inwards with three wrench sets and two free vectors, the springs (drm_contact.hpp
//                                contact_chain_torques_vjp); the two [64, 7] tiles leave through LDS in 16-byte stores (56 B out).
//   contact_rollout_arm_kernel   the same walks with a dynamics walk drm_rollout.hip's arm kernel takes, B n % 4 == 0: that kernel's
//                                body with the contact and spring torques added to the right-hand side before the solve.  BOTH
//                                constant tables staged in LDS once for all T steps; plane, radii, springs and bounds are wave-uniform
//                                values; tau_{t+1} in flight while step t computes; the tiles staged over the parking area and stored
//                                with 16-byte stores.  The contact phase lies before the RNEA and 7 floats of it outlive it.
//   every other case             (other robots, hands, trees, a subset of links, ragged tails, misaligned pointers, B n % 4 != 0
//                                slabs, DRM_LINKS_COMPOSED) is composed on the caller's stream out of the one scratch:
//                                drm_link_motion -> contact_law_kernel (element-wise over the links) -> drm_external_torques ->
//                                contact_add_kernel (the springs, and tau[t] in a rollout); per rollout step then
//                                drm_forward_dynamics and contact_rollout_integrate_kernel.  This is the second of the two forms
//                                the general drm_contact_torques may take: it adds no tree walk of its own to the ones drm_links.hip
//                                already holds to fp64.  The VJP composes likewise: drm_link_motion at (q, qd) and at (q, grad_tau)
//                                -> contact_law_vjp_kernel -> drm_link_power_dq twice and drm_external_torques once ->
//                                contact_vjp_add_kernel (the sums, the springs' share, NaN rows).
//
// Compiler's kernel-resource-usage remarks (gfx950, the flags of this unit; profiles/contact_resource_usage.txt):
//   contact_torques_arm_kernel<8, 7, 8>      VGPRs 126  spills 0  LDS 15 616 B  occupancy 3 waves / SIMD
//   contact_torques_vjp_arm_kernel<8, 7, 8>  VGPRs 256 + 21 AGPRs  spills 0  scratch 0  LDS 4 608 B  occupancy 1 wave / SIMD
//   contact_rollout_arm_kernel<8, 7, 7>      VGPRs 224  spills 0  LDS 51 200 B  occupancy 2 waves / SIMD
//   contact_rollout_arm_kernel<8, 7, 8>      VGPRs 240  spills 0  LDS 57 344 B  occupancy 2 waves / SIMD
// (forward_dynamics_rollout_arm_kernel: 200 / 206 VGPRs, 2 waves per SIMD: the contact phase costs 24 / 34 registers and no wave.)
// The VJP kernel keeps the per-link records of its sweep inwards (origins, axes, two velocity sets, f, gv and the depth cotangent; m, gw
// and gp are formed again on the way in) in registers at one wavefront per SIMD.  Parking the two velocity sets in LDS (72 floats per
// row, 19 456 B per wavefront) and asking for two wavefronts per SIMD (amdgpu_waves_per_eu) was compiled and NOT kept: the register
// allocator still spilled 21 - 25 VGPRs to scratch at 256, with or without the parking — the pressure peaks inside the unrolled sweep
// outwards, not in the records — and scratch is what the kernel must not have.
//
// Per row and step, fused rollout: in tau [n], out q, qd [n] (84 B; 112 B with qdd_traj), as the plain rollout.  Torques, fused:
// 56 B in, 28 B out (220 B with both wrench tiles); their VJP, fused: 84 B in, 56 B out.
#include <math.h>

#include "drm_common.hpp"
#include "drm_contact.hpp"
#include "drm_dispatch.hpp"
#include "drm_rollout.hpp"
#include "drm_rows.hpp"
#include "drm_sample.hpp"
#include "drm_args.hpp"

namespace drm {

constexpr uint32_t contact_tile_magic(int S) { return (uint32_t)((((uint64_t)1 << 32) + (uint64_t)S - 1) / (uint64_t)S); }

// joint-limit springs as kernel arguments (on = 0: none, lower / upper are not read)
struct SpringArgs {
    float k, c;
    const float *lower, *upper;
    int on;
};

__device__ __forceinline__ const float *contact_slab_ptr(const float *base, int64_t off) {
    const uint64_t u = (uint64_t)(uintptr_t)(base + off);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return reinterpret_cast<const float *>((uintptr_t)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ float *contact_slab_ptr(float *base, int64_t off) {
    return const_cast<float *>(contact_slab_ptr(const_cast<const float *>(base), off));
}

template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE)
    contact_torques_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd, int n_tiles,
                               ContactPlane pl, const float *__restrict__ radius, SpringArgs sp, float *__restrict__ tau,
                               float *__restrict__ force, float *__restrict__ moment) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int S = 3 * LINKS, SP = S | 1;
    static_assert(!(S & 1) && !((WAVE * S) & 3), "even row widths (padded LDS image), whole 16-byte stores");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * SP), Q_FLOATS = round4(WAVE * NJ);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 2 * T_FLOATS + Q_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lf = smem + C_FLOATS, *lm = lf + T_FLOATS, *lt = lm + T_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], qdv[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qdv[d] = qd[r0 + d];
    }
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    // a row that cannot be used walks the chain at rest at q = 0 and gets NaN outputs (drm_links.hip)
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || lag_bad_input(qv[d], qdv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; }
    const float nan = __builtin_nanf("");

    float ext[NJ], cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    contact_chain_torques<LINKS, NJ>(
        row, pl, cs, sn, qdv, [&](int k) { return radius ? radius[k] : 0.0f; },
        [&](int k, const float *f, const float *m) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                lf[lane * SP + 3 * k + i] = bad ? nan : f[i];
                lm[lane * SP + 3 * k + i] = bad ? nan : m[i];
            }
        },
        [&](int j, float v) { ext[j] = v; });
    if (sp.on) {
#pragma unroll
        for (int d = 0; d < NJ; ++d) ext[d] += joint_spring_torque(sp.k, sp.c, sp.lower[d], sp.upper[d], qv[d], qdv[d]);
    }
#pragma unroll
    for (int d = 0; d < NJ; ++d) lt[lane * NJ + d] = bad ? nan : ext[d];
    wave_lds_sync();
    tile_store<NJ>(tau + b0 * NJ, WAVE, NJ, 0u, lt, lane, true);
    if (force) tile_store<S>(force + b0 * S, WAVE, S, contact_tile_magic(S), lf, lane, false, true);
    if (moment) tile_store<S>(moment + b0 * S, WAVE, S, contact_tile_magic(S), lm, lane, false, true);
}

// drm_contact_torques_vjp, fused: contact_torques_arm_kernel's tiles and LDS image with the cotangent lam of the torques beside q and qd
// (84 B in per row), drm_contact.hpp contact_chain_torques_vjp per lane, the springs' share, and the two [64, 7] tiles of grad_q and
// grad_qd out through LDS in 16-byte stores (56 B out per row).  The per-link records of the sweep inwards stay in registers, at one
// wavefront per SIMD (the file header says what else was compiled).
template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE)
    contact_torques_vjp_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd,
                                   const float *__restrict__ lam, int n_tiles, ContactPlane pl, const float *__restrict__ radius,
                                   SpringArgs sp, float *__restrict__ grad_q, float *__restrict__ grad_qd) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, Q_FLOATS = round4(WAVE * NJ);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 2 * Q_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lgq = smem + C_FLOATS, *lgqd = lgq + Q_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], qdv[NJ], lv[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qdv[d] = qd[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) lv[d] = lam[r0 + d];
    }
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || lag_bad_input(qv[d], qdv[d]) || !(fabsf(lv[d]) <= 3.0e38f);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; lv[d] = bad ? 0.0f : lv[d]; }
    const float nan = __builtin_nanf("");

    float gq[NJ], gqd[NJ], cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    contact_chain_torques_vjp<LINKS, NJ>(
        row, pl, cs, sn, qdv, lv, [&](int k) { return radius ? radius[k] : 0.0f; }, [&](int j, float a, float b) { gq[j] = a; gqd[j] = b; });
    if (sp.on) {
#pragma unroll
        for (int d = 0; d < NJ; ++d) joint_spring_vjp(sp.k, sp.c, sp.lower[d], sp.upper[d], qv[d], lv[d], gq[d], gqd[d]);
    }
#pragma unroll
    for (int d = 0; d < NJ; ++d) { lgq[lane * NJ + d] = bad ? nan : gq[d]; lgqd[lane * NJ + d] = bad ? nan : gqd[d]; }
    wave_lds_sync();
    if (grad_q) tile_store<NJ>(grad_q + b0 * NJ, WAVE, NJ, 0u, lgq, lane, true);
    if (grad_qd) tile_store<NJ>(grad_qd + b0 * NJ, WAVE, NJ, 0u, lgqd, lane, true);
}

// forward_dynamics_rollout_arm_kernel (drm_rollout.hip) with the contact and spring torques of the step's state added to the
// right-hand side.  LINKS: the links of the dynamics walk (7 or 8); the links walk has CAP = 8 ops, all of them contact links.
// LDS per wavefront: [ dynamics table : CAP x 32 ][ links table : CAP x 32 ][ parked body forces : (LINKS - KEEP) x 6 x 64 ]; the q,
// qd, qdd tiles of a step are staged side by side over the parking area once the step's RNEA is done with it.  Every slab start is
// 16-byte aligned (the launcher's condition).
template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE *MAX_WAVES_PER_BLOCK)
    contact_rollout_arm_kernel(const float *__restrict__ dyn_f, const float *__restrict__ links_f, const float *__restrict__ q0,
                               const float *__restrict__ qd0, const float *__restrict__ tau, int64_t B, int T, float dt, int n_tiles,
                               int flags, ContactPlane pl, int has_plane, const float *__restrict__ radius, SpringArgs sp,
                               float *__restrict__ q_traj, float *__restrict__ qd_traj, float *__restrict__ qdd_traj) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies a constant table");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, Q_FLOATS = round4(WAVE * NJ), F_FLOATS = (LINKS - DRM_RNEA_KEEP) * 6 * WAVE;
    static_assert(3 * Q_FLOATS <= F_FLOATS, "the q, qd and qdd tiles fit under the parking area");
    constexpr int PER_WAVE = 2 * C_FLOATS + F_FLOATS;
    __shared__ __attribute__((aligned(16))) float smem[MAX_WAVES_PER_BLOCK * PER_WAVE];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tile = (int)blockIdx.x * MAX_WAVES_PER_BLOCK + wave;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem + wave * PER_WAVE, *ll = lc + C_FLOATS;
    float *lq = ll + C_FLOATS, *lqd = lq + Q_FLOATS, *lqdd = lqd + Q_FLOATS;
    float *park = lq + lane;
    const int64_t b0 = (int64_t)tile * WAVE, slab = B * NJ, r0 = (b0 + lane) * NJ;
    const bool explicit_euler = (flags & DRM_ROLLOUT_EXPLICIT_EULER) != 0, want_qdd = qdd_traj != nullptr;

    float4 cv = reinterpret_cast<const float4 *>(dyn_f)[lane], lv = reinterpret_cast<const float4 *>(links_f)[lane];
    float qv[NJ], qdv[NJ], fv[NJ], zero[NJ];
#pragma unroll
    for (int d = 0; d < NJ; ++d) qv[d] = q0[r0 + d];
#pragma unroll
    for (int d = 0; d < NJ; ++d) qdv[d] = qd0[r0 + d];
#pragma unroll
    for (int d = 0; d < NJ; ++d) { fv[d] = tau[r0 + d]; zero[d] = 0.0f; }
    pin(cv);
    pin(lv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    reinterpret_cast<float4 *>(ll)[lane] = lv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };
    auto lrow = [&](int k) -> const float * { return ll + k * DRM_OPF_STRIDE; };

    // wave-uniform: read once, held in scalar registers across the steps
    float rad[CAP], lo[NJ], hi[NJ];
#pragma unroll
    for (int k = 0; k < CAP; ++k) rad[k] = (has_plane && radius) ? radius[k] : 0.0f;
#pragma unroll
    for (int d = 0; d < NJ; ++d) { lo[d] = sp.on ? sp.lower[d] : -INFINITY; hi[d] = sp.on ? sp.upper[d] : INFINITY; }

#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        float rhs[NJ], nle[NJ];
#pragma unroll
        for (int d = 0; d < NJ; ++d) rhs[d] = fv[d];
        if (t + 1 < T) { // the next step's torques, in flight while this step computes
            const float *nx = contact_slab_ptr(tau, (int64_t)(t + 1) * slab + b0 * NJ) + lane * NJ;
#pragma unroll
            for (int d = 0; d < NJ; ++d) fv[d] = nx[d];
        }
        float cs[NJ], sn[NJ];
        chain_trig<NJ>(qv, cs, sn);
        {
            float ext[NJ];
#pragma unroll
            for (int d = 0; d < NJ; ++d) ext[d] = 0.0f;
            if (has_plane)
                contact_chain_torques<CAP, NJ>(
                    lrow, pl, cs, sn, qdv, [&](int k) { return rad[k]; }, [&](int, const float *, const float *) {},
                    [&](int j, float v) { ext[j] = v; });
            if (sp.on) {
#pragma unroll
                for (int d = 0; d < NJ; ++d) ext[d] += joint_spring_torque(sp.k, sp.c, lo[d], hi[d], qv[d], qdv[d]);
            }
#pragma unroll
            for (int d = 0; d < NJ; ++d) rhs[d] += ext[d];
        }
        rnea_chain_trig<LINKS, NJ>(row, flags & DRM_RNEA_GRAVITY, flags & DRM_RNEA_DAMPING, cs, sn, qdv, zero, nle,
                                   [&](int k, const Force &F) {
#pragma unroll
                                       for (int i = 0; i < 3; ++i) {
                                           park[(k * 6 + i) * WAVE] = F.la[i][0];
                                           park[(k * 6 + 3 + i) * WAVE] = F.la[i][1];
                                       }
                                   },
                                   [&](int k, Force &F) {
#pragma unroll
                                       for (int i = 0; i < 3; ++i) F.la[i] = f2_make(park[(k * 6 + i) * WAVE], park[(k * 6 + 3 + i) * WAVE]);
                                   });
        float Ht[NJ * (NJ + 1) / 2];
        crba_chain_trig<LINKS, NJ>(row, cs, sn, [&](int i, int j, float v) {
            if (i >= j) Ht[tri_index(i, j)] = v;
        });
#pragma unroll
        for (int d = 0; d < NJ; ++d) rhs[d] -= nle[d];
        ltdl_solve_unrolled<NJ>(Ht, rhs);
#pragma unroll
        for (int d = 0; d < NJ; ++d) rollout_step(qv[d], qdv[d], rhs[d], dt, explicit_euler);
        wave_lds_sync(); // every lane is done with the parking area before the tiles are staged over it
#pragma unroll
        for (int d = 0; d < NJ; ++d) { lq[lane * NJ + d] = qv[d]; lqd[lane * NJ + d] = qdv[d]; }
        if (want_qdd) {
#pragma unroll
            for (int d = 0; d < NJ; ++d) lqdd[lane * NJ + d] = rhs[d];
        }
        wave_lds_sync();
        const int64_t out = (int64_t)t * slab + b0 * NJ;
        tile_store<NJ>(contact_slab_ptr(q_traj, out), WAVE, NJ, 0u, lq, lane, true);
        tile_store<NJ>(contact_slab_ptr(qd_traj, out), WAVE, NJ, 0u, lqd, lane, true);
        if (want_qdd) tile_store<NJ>(contact_slab_ptr(qdd_traj, out), WAVE, NJ, 0u, lqdd, lane, true);
        wave_lds_sync(); // the stores have read the tiles before the next step parks its body forces over them
    }
}

// The composed path's law: one thread per (row, link).  A link of a row drm_link_motion refused (NaN position) gets a NaN wrench.
__global__ void __launch_bounds__(256)
    contact_law_kernel(const float *__restrict__ pos, const float *__restrict__ lin_vel, const float *__restrict__ ang_vel, int64_t count,
                       int T, ContactPlane pl, const float *__restrict__ radius, float *__restrict__ force, float *__restrict__ moment) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        const float p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
        const float v[3] = {lin_vel[3 * i], lin_vel[3 * i + 1], lin_vel[3 * i + 2]};
        const float w[3] = {ang_vel[3 * i], ang_vel[3 * i + 1], ang_vel[3 * i + 2]};
        float f[3], m[3];
        contact_wrench(pl, radius ? radius[t] : 0.0f, p, v, w, f, m);
        const bool bad = p[0] != p[0];
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < 3; ++k) { force[3 * i + k] = bad ? nan : f[k]; moment[3 * i + k] = bad ? nan : m[k]; }
    }
}

// out = tau_in + (tau_ext + tau_lim), element-wise over count = rows * n coordinates; tau_in / tau_ext NULL: zero.  check_rows: a
// coordinate of a row with a q or qd that cannot be used is NaN (drm_contact_torques; a rollout's forward dynamics sees to that).
__global__ void __launch_bounds__(256)
    contact_add_kernel(const float *__restrict__ tau_in, const float *__restrict__ tau_ext, const float *__restrict__ q,
                       const float *__restrict__ qd, int64_t count, int n, SpringArgs sp, int check_rows, float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % n);
        float e = tau_ext ? tau_ext[i] : 0.0f;
        if (sp.on) e += joint_spring_torque(sp.k, sp.c, sp.lower[d], sp.upper[d], q[i], qd[i]);
        if (check_rows) {
            const int64_t r0 = i - d;
            bool bad = false;
            for (int j = 0; j < n; ++j) bad = bad || lag_bad_input(q[r0 + j], qd[r0 + j]);
            if (bad) e = __builtin_nanf("");
        }
        out[i] = tau_in ? tau_in[i] + e : e;
    }
}

// The composed path's law and its backward: one thread per (row, link).  (a, b): the links' velocities at rates lam, the cotangents of
// the wrenches.  Rows that cannot be used are seen to by contact_vjp_add_kernel.
__global__ void __launch_bounds__(256)
    contact_law_vjp_kernel(const float *__restrict__ pos, const float *__restrict__ lin_vel, const float *__restrict__ ang_vel,
                           const float *__restrict__ lin_cot, const float *__restrict__ ang_cot, int64_t count, int T, ContactPlane pl,
                           const float *__restrict__ radius, float *__restrict__ force, float *__restrict__ moment, float *__restrict__ gpos,
                           float *__restrict__ glin, float *__restrict__ gang) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        float p[3], v[3], w[3], a[3], b[3], f[3], m[3], gp[3], gv[3], gw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = pos[3 * i + k]; v[k] = lin_vel[3 * i + k]; w[k] = ang_vel[3 * i + k]; a[k] = lin_cot[3 * i + k]; b[k] = ang_cot[3 * i + k];
        }
        contact_wrench_vjp(pl, radius ? radius[t] : 0.0f, p, v, w, a, b, f, m, gp, gv, gw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            force[3 * i + k] = f[k]; moment[3 * i + k] = m[k]; gpos[3 * i + k] = gp[k]; glin[3 * i + k] = gv[k]; gang[3 * i + k] = gw[k];
        }
    }
}

// grad_q = (dq1 + t2) + dq3 + the springs' share, grad_qd = tau3 + the springs' share, element-wise over count = rows * n coordinates
// (the four inputs NULL: no plane).  A coordinate of a row with a q, qd or lam that cannot be used is NaN.
__global__ void __launch_bounds__(256)
    contact_vjp_add_kernel(const float *__restrict__ dq1, const float *__restrict__ t2, const float *__restrict__ dq3,
                           const float *__restrict__ tau3, const float *__restrict__ q, const float *__restrict__ qd,
                           const float *__restrict__ lam, int64_t count, int n, SpringArgs sp, float *__restrict__ grad_q,
                           float *__restrict__ grad_qd) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % n);
        float gq = dq1 ? (dq1[i] + t2[i]) + dq3[i] : 0.0f, gqd = dq1 ? tau3[i] : 0.0f;
        if (sp.on) joint_spring_vjp(sp.k, sp.c, sp.lower[d], sp.upper[d], q[i], lam[i], gq, gqd);
        const int64_t r0 = i - d;
        bool bad = false;
        for (int j = 0; j < n; ++j) bad = bad || lag_bad_input(q[r0 + j], qd[r0 + j]) || !(fabsf(lam[r0 + j]) <= 3.0e38f);
        if (bad) gq = gqd = __builtin_nanf("");
        if (grad_q) grad_q[i] = gq;
        if (grad_qd) grad_qd[i] = gqd;
    }
}

// the composed path's integrator (drm_rollout.hip's, which a launch from this unit cannot reach): one step of count coordinates.
// qdd_out (NULL: not wanted) gets a copy of the accelerations: drm_forward_dynamics always writes them to the scratch, so that the
// kernel it picks by the alignment of its pointers, and with it every bit of q and qd, does not depend on whether qdd_traj is asked for
__global__ void __launch_bounds__(256)
    contact_rollout_integrate_kernel(const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ qdd, int64_t count,
                                     float dt, int explicit_euler, float *__restrict__ q_out, float *__restrict__ qd_out,
                                     float *__restrict__ qdd_out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        float x = q[i], v = qd[i];
        const float a = qdd[i];
        rollout_step(x, v, a, dt, explicit_euler != 0);
        q_out[i] = x;
        qd_out[i] = v;
        if (qdd_out) qdd_out[i] = a;
    }
}

static inline unsigned contact_blocks(int64_t count) {
    const int64_t b = (count + 255) / 256;
    return (unsigned)(b < 8192 ? (b < 1 ? 1 : b) : 8192);
}
static inline int64_t r4(int64_t x) { return (x + 3) & ~(int64_t)3; }

// an arm7_walk of 8 ops whose every op is a target, slots in walk order (drm_links.hip links_fused)
static inline bool contact_links_fused(const drm_walk *w, int T, int64_t B, int flags, bool aligned) {
    return !(flags & DRM_LINKS_COMPOSED) && (w->shape & DRM_WALK_TARGETS_ORDERED) && w->n_ops == 8 && T == 8 && rows_fused(w, B, aligned);
}

// the checked contact arguments (drm_args.hpp ContactPlan) as the kernels take them
struct ContactArgs {
    ContactPlane pl;
    int has_plane;
    const float *radius;
    SpringArgs sp;
};
static ContactArgs contact_args(const ContactPlan &p) {
    return ContactArgs{p.pl, p.has_plane, p.radius, SpringArgs{p.k, p.c, p.lower, p.upper, p.lower != nullptr}};
}

// The composed contact torques of `rows` rows: out = tau_in + (tau_ext + tau_lim).  `buf`: 5 x r4(rows T 3) + r4(rows n) floats (the
// links' motion, the wrenches unless the caller gave arrays for them, tau_ext), `sub`: the scratch of the two link calls.
static int64_t contact_buf_floats(int64_t rows, int T, int n) { return 5 * r4(rows * T * 3) + r4(rows * n); }
static int contact_composed(const drm_walk *lw, const ContactArgs &a, const float *q, const float *qd, const float *tau_in, int64_t rows,
                            int T, int n, int flags, int check_rows, float *out, float *force, float *moment, float *buf, float *sub,
                            hipStream_t s) {
    const int64_t count = rows * n;
    const float *ext = nullptr;
    if (a.has_plane) {
        if (!buf) return fail(DRM_ERR_INVALID, "pass the matching _scratch_floats() query's floats of scratch");
        const int64_t L = r4(rows * T * 3);
        float *pos = buf, *lv = pos + L, *av = lv + L, *f = force ? force : av + L, *m = moment ? moment : av + 2 * L, *te = av + 3 * L;
        const int lf = flags & DRM_LINKS_COMPOSED;
        int rc = drm_link_motion(lw, q, qd, nullptr, rows, T, lf, pos, lv, av, nullptr, nullptr, sub, s);
        if (rc) return rc;
        hipLaunchKernelGGL(contact_law_kernel, dim3(contact_blocks(rows * T)), dim3(256), 0, s, (const float *)pos, (const float *)lv,
                           (const float *)av, rows * T, T, a.pl, a.radius, f, m);
        rc = launched();
        if (rc) return rc;
        rc = drm_external_torques(lw, q, f, m, rows, T, lf, te, sub, s);
        if (rc) return rc;
        ext = te;
    }
    hipLaunchKernelGGL(contact_add_kernel, dim3(contact_blocks(count)), dim3(256), 0, s, tau_in, ext, q, qd, count, n, a.sp, check_rows, out);
    return launched();
}

static int64_t contact_links_sub(const drm_walk *lw, int64_t B) {
    const int64_t a = drm_link_motion_scratch_floats(lw, B), b = drm_external_torques_scratch_floats(lw, B);
    return r4(a > b ? a : b);
}

} // namespace drm

using namespace drm;

// The composed form over ALL B rows, whatever the alignment: whether a call is fused depends on n_targets, which the query does not
// see (drm_links.hip links_scratch).
extern "C" int64_t drm_contact_torques_scratch_floats(const drm_walk *lw, int64_t B) {
    if (check_sweep_walk(lw) || B <= 0) return 0;
    return contact_buf_floats(B, lw->n_ops, lw->n_dofs) + contact_links_sub(lw, B);
}
extern "C" int64_t drm_contact_torques_scratch_floats_aligned(const drm_walk *lw, int64_t B) { return drm_contact_torques_scratch_floats(lw, B); }

extern "C" int drm_contact_torques(const drm_walk *lw, const float *q, const float *qd, int64_t B, int32_t n_targets,
                                   const drm_contact_plane *plane, const float *radius, const drm_joint_springs *springs,
                                   const float *lower, const float *upper, int32_t flags, float *tau, float *force, float *moment,
                                   float *scratch, void *stream) {
    ContactPlan plan;
    int rc = args_contact_torques(lw, q, qd, B, n_targets, plane, radius, springs, lower, upper, tau, plan);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    const ContactArgs a = contact_args(plan);
    hipStream_t s = (hipStream_t)stream;
    const int n = lw->n_dofs, T = n_targets;
    int64_t lo = 0;
    if (contact_links_fused(lw, T, B, flags, aligned16(q, qd, tau, force, moment))) {
        const int n_tiles = (int)(B / WAVE);
        hipLaunchKernelGGL((contact_torques_arm_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, lw->ops_f, q, qd, n_tiles, a.pl,
                           a.radius, a.sp, tau, force, moment);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    const int64_t rows = B - lo;
    float *sub = scratch ? scratch + contact_buf_floats(rows, T, n) : nullptr;
    return contact_composed(lw, a, q + lo * n, qd + lo * n, nullptr, rows, T, n, flags, 1, tau + lo * n, force ? force + lo * T * 3 : nullptr,
                            moment ? moment + lo * T * 3 : nullptr, scratch, sub, s);
}

// The composed vector-Jacobian product of `rows` rows.  `buf`: 10 x r4(rows T 3) (the links' motion at rates qd, their velocities at
// rates lam, the wrenches and the three cotangents of the law) + 4 x r4(rows n) floats; `sub`: the scratch of the link calls.
static int64_t contact_vjp_buf_floats(int64_t rows, int T, int n) { return 10 * r4(rows * T * 3) + 4 * r4(rows * n); }
static int64_t contact_vjp_links_sub(const drm_walk *lw, int64_t B) {
    const int64_t a = contact_links_sub(lw, B), b = drm_link_power_dq_scratch_floats(lw, B);
    return r4(a > b ? a : b);
}
static int contact_vjp_composed(const drm_walk *lw, const ContactArgs &a, const float *q, const float *qd, const float *lam, int64_t rows,
                                int T, int n, int flags, float *grad_q, float *grad_qd, float *buf, float *sub, hipStream_t s) {
    const int64_t count = rows * n;
    const float *dq1 = nullptr, *t2 = nullptr, *dq3 = nullptr, *tau3 = nullptr;
    if (a.has_plane) {
        if (!buf) return fail(DRM_ERR_INVALID, "pass the matching _scratch_floats() query's floats of scratch");
        const int64_t L = r4(rows * T * 3), N = r4(count);
        float *pos = buf, *lv = pos + L, *av = lv + L, *la = av + L, *lb = la + L, *f = lb + L, *m = f + L, *gp = m + L, *gv = gp + L;
        float *gw = gv + L, *o1 = gw + L, *o2 = o1 + N, *o3 = o2 + N, *o4 = o3 + N;
        const int lf = flags & DRM_LINKS_COMPOSED;
        int rc = drm_link_motion(lw, q, qd, nullptr, rows, T, lf, pos, lv, av, nullptr, nullptr, sub, s);
        if (rc) return rc;
        rc = drm_link_motion(lw, q, lam, nullptr, rows, T, lf, nullptr, la, lb, nullptr, nullptr, sub, s);
        if (rc) return rc;
        hipLaunchKernelGGL(contact_law_vjp_kernel, dim3(contact_blocks(rows * T)), dim3(256), 0, s, (const float *)pos, (const float *)lv,
                           (const float *)av, (const float *)la, (const float *)lb, rows * T, T, a.pl, a.radius, f, m, gp, gv, gw);
        rc = launched();
        if (rc) return rc;
        rc = drm_link_power_dq(lw, q, lam, f, m, rows, T, lf, o1, nullptr, sub, s);
        if (rc) return rc;
        rc = drm_external_torques(lw, q, gp, nullptr, rows, T, lf, o2, sub, s);
        if (rc) return rc;
        rc = drm_link_power_dq(lw, q, qd, gv, gw, rows, T, lf, o3, o4, sub, s);
        if (rc) return rc;
        dq1 = o1; t2 = o2; dq3 = o3; tau3 = o4;
    }
    hipLaunchKernelGGL(contact_vjp_add_kernel, dim3(contact_blocks(count)), dim3(256), 0, s, dq1, t2, dq3, tau3, q, qd, lam, count, n, a.sp,
                       grad_q, grad_qd);
    return launched();
}

// The composed form over ALL B rows, as drm_contact_torques_scratch_floats.
extern "C" int64_t drm_contact_torques_vjp_scratch_floats(const drm_walk *lw, int64_t B) {
    if (check_sweep_walk(lw) || B <= 0) return 0;
    return contact_vjp_buf_floats(B, lw->n_ops, lw->n_dofs) + contact_vjp_links_sub(lw, B);
}
extern "C" int64_t drm_contact_torques_vjp_scratch_floats_aligned(const drm_walk *lw, int64_t B) {
    return drm_contact_torques_vjp_scratch_floats(lw, B);
}

extern "C" int drm_contact_torques_vjp(const drm_walk *lw, const float *q, const float *qd, const float *grad_tau, int64_t B,
                                       int32_t n_targets, const drm_contact_plane *plane, const float *radius,
                                       const drm_joint_springs *springs, const float *lower, const float *upper, int32_t flags,
                                       float *grad_q, float *grad_qd, float *scratch, void *stream) {
    ContactPlan plan;
    int rc = args_contact_torques_vjp(lw, q, qd, grad_tau, B, n_targets, plane, radius, springs, lower, upper, grad_q, grad_qd, plan);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    const ContactArgs a = contact_args(plan);
    hipStream_t s = (hipStream_t)stream;
    const int n = lw->n_dofs, T = n_targets;
    int64_t lo = 0;
    if (plane && contact_links_fused(lw, T, B, flags, aligned16(q, qd, grad_tau, grad_q, grad_qd))) {
        const int n_tiles = (int)(B / WAVE);
        hipLaunchKernelGGL((contact_torques_vjp_arm_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, lw->ops_f, q, qd, grad_tau,
                           n_tiles, a.pl, a.radius, a.sp, grad_q, grad_qd);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    const int64_t rows = B - lo;
    float *sub = scratch ? scratch + contact_vjp_buf_floats(rows, T, n) : nullptr;
    return contact_vjp_composed(lw, a, q + lo * n, qd + lo * n, grad_tau + lo * n, rows, T, n, flags, grad_q ? grad_q + lo * n : nullptr,
                                grad_qd ? grad_qd + lo * n : nullptr, scratch, sub, s);
}

// both walks, the batch and every pointer qualify for contact_rollout_arm_kernel
static bool contact_rollout_fused(const drm_walk *dw, const drm_walk *lw, int T_links, int64_t B, int flags, bool has_plane, bool aligned) {
    if (!(arm7_walk(dw) && table_aligned(dw) && aligned && full_tiles_fit(B) && (B * dw->n_dofs) % 4 == 0)) return false;
    if (flags & DRM_LINKS_COMPOSED) return false;
    return !has_plane || contact_links_fused(lw, T_links, B, flags, aligned);
}

// scratch of the composed steps of `rows` rows: [ tau of the step : r4(rows n) ][ qdd : r4(rows n) ][ contact_buf_floats ][ sub ]
static int64_t contact_rollout_scratch_impl(const drm_walk *dw, const drm_walk *lw, int64_t B, bool aligned) {
    if (check_walk(dw) || B <= 0) return 0;
    const int n = dw->n_dofs;
    const int64_t fd = aligned && (B * n) % 4 == 0 ? drm_forward_dynamics_scratch_floats_aligned(dw, B) : drm_forward_dynamics_scratch_floats(dw, B);
    int64_t links = 0, buf = 0;
    if (lw && !check_sweep_walk(lw)) {
        links = contact_links_sub(lw, B);
        buf = contact_buf_floats(B, lw->n_ops, n);
    }
    return 2 * r4(B * n) + buf + (links > fd ? links : r4(fd));
}
extern "C" int64_t drm_contact_rollout_scratch_floats(const drm_walk *dw, const drm_walk *lw, int64_t B) {
    return contact_rollout_scratch_impl(dw, lw, B, false);
}
extern "C" int64_t drm_contact_rollout_scratch_floats_aligned(const drm_walk *dw, const drm_walk *lw, int64_t B) {
    return contact_rollout_scratch_impl(dw, lw, B, true);
}

extern "C" int drm_contact_rollout(const drm_walk *dw, const drm_walk *lw, const float *q0, const float *qd0, const float *tau, int64_t B,
                                   int32_t T, float dt, int32_t flags, int32_t n_targets, const drm_contact_plane *plane,
                                   const float *radius, const drm_joint_springs *springs, const float *lower, const float *upper,
                                   float *q_traj, float *qd_traj, float *qdd_traj, float *scratch, void *stream) {
    ContactPlan plan;
    int rc = args_contact_rollout(dw, lw, q0, qd0, tau, B, T, dt, n_targets, plane, radius, springs, lower, upper, q_traj, qd_traj, plan);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    const ContactArgs a = contact_args(plan);
    hipStream_t s = (hipStream_t)stream;
    const int n = dw->n_dofs, TL = n_targets;
    const bool aligned = aligned16(q0, qd0, tau, q_traj, qd_traj, qdd_traj) && (!plane || table_aligned(lw));
    int64_t lo = 0;
    if (contact_rollout_fused(dw, lw, TL, B, flags, plane != nullptr, aligned)) {
        const int n_tiles = (int)(B / WAVE);
        const dim3 grid((unsigned)((n_tiles + MAX_WAVES_PER_BLOCK - 1) / MAX_WAVES_PER_BLOCK)), block(WAVE * MAX_WAVES_PER_BLOCK);
        const float *links_f = plane ? lw->ops_f : dw->ops_f; // (never walked without a plane)
        if (arm_links(dw) == 7)
            hipLaunchKernelGGL((contact_rollout_arm_kernel<8, 7, 7>), grid, block, 0, s, dw->ops_f, links_f, q0, qd0, tau, B, (int)T, dt,
                               n_tiles, (int)flags, a.pl, a.has_plane, a.radius, a.sp, q_traj, qd_traj, qdd_traj);
        else
            hipLaunchKernelGGL((contact_rollout_arm_kernel<8, 7, 8>), grid, block, 0, s, dw->ops_f, links_f, q0, qd0, tau, B, (int)T, dt,
                               n_tiles, (int)flags, a.pl, a.has_plane, a.radius, a.sp, q_traj, qd_traj, qdd_traj);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the composed steps of rows [lo, B)
    if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_contact_rollout_scratch_floats() floats of scratch");
    const int64_t rows = B - lo, count = rows * n, slab = B * n;
    float *total = scratch, *qdd_buf = total + r4(count), *buf = qdd_buf + r4(count);
    float *sub = buf + (plane ? contact_buf_floats(rows, TL, n) : 0);
    const int fd_flags = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING), expl = (flags & DRM_ROLLOUT_EXPLICIT_EULER) != 0;
    for (int t = 0; t < T; ++t) {
        const int64_t off = (int64_t)t * slab + lo * n;
        const float *qi = t ? q_traj + off - slab : q0 + lo * n, *qdi = t ? qd_traj + off - slab : qd0 + lo * n;
        rc = contact_composed(lw, a, qi, qdi, tau + off, rows, TL, n, flags, 0, total, nullptr, nullptr, buf, sub, s);
        if (rc) return rc;
        rc = drm_forward_dynamics(dw, qi, qdi, total, rows, fd_flags, qdd_buf, sub, s);
        if (rc) return rc;
        hipLaunchKernelGGL(contact_rollout_integrate_kernel, dim3(contact_blocks(count)), dim3(256), 0, s, qi, qdi, (const float *)qdd_buf,
                           count, dt, expl, q_traj + off, qd_traj + off, qdd_traj ? qdd_traj + off : (float *)nullptr);
        rc = launched();
        if (rc) return rc;
    }
    return DRM_OK;
}

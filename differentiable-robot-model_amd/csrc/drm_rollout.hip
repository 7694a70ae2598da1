// drm_rollout.hip — ABI 14: T steps of forward dynamics and an Euler integrator per launch (include/drm_hip.h
// drm_forward_dynamics_rollout).  What a Python loop over compute_forward_dynamics does for sampling-based MPC, for fitting dynamics
// parameters to recorded trajectories and for trajectory optimisation through the dynamics, without a launch per step and without
// sending the state through HBM between the steps.
//
// Two fused kernels, each the body of its single-step counterpart (drm_forward_dynamics.hip) inside a loop over the steps:
//   forward_dynamics_rollout_arm_kernel      7-DoF arm chains, full 64-row tiles: the constant table staged in LDS ONCE for all T
//                                            steps, q and qd in registers across the steps, tau_{t+1} loaded before step t is
//                                            computed; q_{t+1}, qd_{t+1} (and qdd_t) staged through the parking area and written
//                                            with 16-byte stores
//   forward_dynamics_rollout_fingers_kernel  hands (K fingers of L joints off the root): H is block diagonal, so every finger's
//                                            wavefront integrates its own L columns and never needs another finger's results
// Every other robot, the ragged tail of a launch and misaligned pointers: drm_forward_dynamics on each step's [B, n] slab followed by
// forward_dynamics_rollout_integrate_kernel, all enqueued on the caller's stream without a host synchronisation.
//
// Per row and step, fused: in tau [n], out q, qd [n] (12 n bytes; 16 n with qdd_traj).   n = 7: 84 B (112 B)
// Composed: drm_forward_dynamics (16 n) + the integrator (20 n: q, qd, qdd in, q, qd out).  n = 7: 252 B
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_rollout.hpp"
#include "drm_sample.hpp"
#include "drm_args.hpp"

namespace drm {
// 7-DoF arms with their own two-samples-per-lane forward-dynamics kernel attached take the composed steps from this many 128-row
// pairs of tiles on (Panda, 16 steps: fused 195 / 1 320 us against composed 347 / 1 061 us at 2^17 / 2^20 rows)
#ifndef DRM_ROLLOUT_COMPOSED_MIN_PAIRS
#define DRM_ROLLOUT_COMPOSED_MIN_PAIRS 4096 /* 524 288 rows */
#endif

// base + offset as a wave-uniform pointer the compiler cannot see through: the per-step slab pointers are then formed in SGPRs inside
// each step instead of being strength-reduced into per-lane 64-bit induction variables that stay live across the whole loop
__device__ __forceinline__ float *slab_ptr(float *base, int64_t off) {
    const uint64_t u = (uint64_t)(uintptr_t)(base + off);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return reinterpret_cast<float *>((uintptr_t)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ const float *slab_ptr(const float *base, int64_t off) { return slab_ptr(const_cast<float *>(base), off); }

// Serial 7-DoF arm chains (DRM_WALK_ARM_CHAIN, capacity 8), full tiles: forward_dynamics_arm_kernel's three steps (bias torques by
// rnea_chain_trig with qdd = 0, H by crba_chain_trig on the same cos / sin, the unrolled L^T D L solve) once per time step.
// LDS per wavefront as there: [ table : CAP x 32 ][ parked body forces : (LINKS - KEEP) x 6 x 64 ]; the q, qd, qdd tiles of a step
// are staged side by side over the parking area once the step's RNEA is done with it.
// vec: every slab start is 16-byte aligned (B * n % 4 == 0 and aligned pointers): 16-byte stores, else 4-byte ones.
// -DDRM_ROLLOUT_NO_PREFETCH (variant builds): tau_t loaded at the top of step t instead of one step ahead.
template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE *MAX_WAVES_PER_BLOCK)
    forward_dynamics_rollout_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q0, const float *__restrict__ qd0,
                                        const float *__restrict__ tau, int64_t B, int T, float dt, int n_tiles, int flags,
                                        float *__restrict__ q_traj, float *__restrict__ qd_traj, float *__restrict__ qdd_traj, int vec) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, Q_FLOATS = round4(WAVE * NJ), F_FLOATS = (LINKS - DRM_RNEA_KEEP) * 6 * WAVE;
    static_assert(3 * Q_FLOATS <= F_FLOATS, "the q, qd and qdd tiles fit under the parking area");
    constexpr int PER_WAVE = C_FLOATS + F_FLOATS;
    __shared__ __attribute__((aligned(16))) float smem[MAX_WAVES_PER_BLOCK * PER_WAVE];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tile = (int)blockIdx.x * MAX_WAVES_PER_BLOCK + wave;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem + wave * PER_WAVE;
    float *lq = lc + C_FLOATS, *lqd = lq + Q_FLOATS, *lqdd = lqd + Q_FLOATS;
    float *park = lq + lane;
    const int64_t b0 = (int64_t)tile * WAVE, slab = B * NJ, r0 = (b0 + lane) * NJ;
    const bool explicit_euler = (flags & DRM_ROLLOUT_EXPLICIT_EULER) != 0, want_qdd = qdd_traj != nullptr;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], qdv[NJ], fv[NJ], zero[NJ];
#pragma unroll
    for (int d = 0; d < NJ; ++d) qv[d] = q0[r0 + d];
#pragma unroll
    for (int d = 0; d < NJ; ++d) qdv[d] = qd0[r0 + d];
#pragma unroll
    for (int d = 0; d < NJ; ++d) { fv[d] = tau[r0 + d]; zero[d] = 0.0f; }
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        float rhs[NJ], nle[NJ];
#ifndef DRM_ROLLOUT_NO_PREFETCH
#pragma unroll
        for (int d = 0; d < NJ; ++d) rhs[d] = fv[d];
        if (t + 1 < T) { // the next step's torques, in flight while this step computes
            const float *nx = slab_ptr(tau, (int64_t)(t + 1) * slab + b0 * NJ) + lane * NJ;
#pragma unroll
            for (int d = 0; d < NJ; ++d) fv[d] = nx[d];
        }
#else
        if (t) {
            const float *nx = slab_ptr(tau, (int64_t)t * slab + b0 * NJ) + lane * NJ;
#pragma unroll
            for (int d = 0; d < NJ; ++d) fv[d] = nx[d];
        }
#pragma unroll
        for (int d = 0; d < NJ; ++d) rhs[d] = fv[d];
#endif
        float cs[NJ], sn[NJ];
        chain_trig<NJ>(qv, cs, sn);
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
        tile_store<NJ>(slab_ptr(q_traj, out), WAVE, NJ, 0u, lq, lane, vec != 0);
        tile_store<NJ>(slab_ptr(qd_traj, out), WAVE, NJ, 0u, lqd, lane, vec != 0);
        if (want_qdd) tile_store<NJ>(slab_ptr(qdd_traj, out), WAVE, NJ, 0u, lqdd, lane, vec != 0);
        wave_lds_sync(); // the stores have read the tiles before the next step parks its body forces over them
    }
}

// A HAND (DRM_WALK_FINGERS: K serial chains of L revolute ops off the root), full tiles: forward_dynamics_fingers_kernel's body once
// per time step, one wavefront per finger integrating the finger's own L columns.  Every lane reads and writes only its own rows
// and its own parking column, so the steps need no synchronisation between the lanes.
// LDS (static), per wavefront: [ table : L x 32 ][ parked body forces : L x 6 x 64 ]
template <int L>
__global__ void __launch_bounds__(WAVE * 4)
    forward_dynamics_rollout_fingers_kernel(const float *__restrict__ ops_f, const float *__restrict__ q0, const float *__restrict__ qd0,
                                            const float *__restrict__ tau, int64_t B, int T, float dt, int n, int flags,
                                            float *__restrict__ q_traj, float *__restrict__ qd_traj, float *__restrict__ qdd_traj, int vec) {
    constexpr int C_FLOATS = L * DRM_OPF_STRIDE, P_FLOATS = L * 6 * WAVE;
    __shared__ __attribute__((aligned(16))) float smem[4 * (C_FLOATS + P_FLOATS)];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem + wave * (C_FLOATS + P_FLOATS);
    float *park = lc + C_FLOATS + lane;
    if (lane < (unsigned)(L * (DRM_OPF_STRIDE / 4)))
        reinterpret_cast<float4 *>(lc)[lane] = reinterpret_cast<const float4 *>(ops_f + (size_t)wave * C_FLOATS)[lane];
    const int64_t r0 = ((int64_t)blockIdx.x * WAVE + lane) * n + wave * L, slab = B * n;
    const bool explicit_euler = (flags & DRM_ROLLOUT_EXPLICIT_EULER) != 0;
    float qv[L], qdv[L], fv[L], zero[L];
    auto load = [&](const float *src, float (&dst)[L]) {
        if (L == 4 && vec) {
            const float4 a = *reinterpret_cast<const float4 *>(src);
            dst[0] = a.x; dst[1] = a.y; dst[2 % L] = a.z; dst[3 % L] = a.w;
        } else {
#pragma unroll
            for (int d = 0; d < L; ++d) dst[d] = src[d];
        }
    };
    auto store = [&](float *dst, const float (&src)[L]) {
        if (L == 4 && vec) *reinterpret_cast<float4 *>(dst) = make_float4(src[0], src[1], src[2 % L], src[3 % L]);
        else {
#pragma unroll
            for (int d = 0; d < L; ++d) dst[d] = src[d];
        }
    };
    load(q0 + r0, qv); load(qd0 + r0, qdv); load(tau + r0, fv);
#pragma unroll
    for (int d = 0; d < L; ++d) zero[d] = 0.0f;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        float rhs[L], nle[L];
#pragma unroll
        for (int d = 0; d < L; ++d) rhs[d] = fv[d];
        if (t + 1 < T) load(tau + (int64_t)(t + 1) * slab + r0, fv);
        float cs[L], sn[L];
        chain_trig<L>(qv, cs, sn);
        rnea_chain_trig<L, L>(row, flags & DRM_RNEA_GRAVITY, flags & DRM_RNEA_DAMPING, cs, sn, qdv, zero, nle,
                              [&](int k, const Force &F) {
#pragma unroll
                                  for (int i = 0; i < 3; ++i) { park[(k * 6 + i) * WAVE] = F.la[i][0]; park[(k * 6 + 3 + i) * WAVE] = F.la[i][1]; }
                              },
                              [&](int k, Force &F) {
#pragma unroll
                                  for (int i = 0; i < 3; ++i) F.la[i] = f2_make(park[(k * 6 + i) * WAVE], park[(k * 6 + 3 + i) * WAVE]);
                              });
        float Ht[L * (L + 1) / 2];
        crba_chain_trig<L, L>(row, cs, sn, [&](int i, int j, float v) {
            if (i >= j) Ht[tri_index(i, j)] = v;
        });
#pragma unroll
        for (int d = 0; d < L; ++d) rhs[d] -= nle[d];
        ltdl_solve_unrolled<L>(Ht, rhs);
#pragma unroll
        for (int d = 0; d < L; ++d) rollout_step(qv[d], qdv[d], rhs[d], dt, explicit_euler);
        const int64_t out = (int64_t)t * slab + r0;
        store(q_traj + out, qv);
        store(qd_traj + out, qdv);
        if (qdd_traj) store(qdd_traj + out, rhs);
    }
}

// The composed path's integrator: count = rows * n coordinates of one step, element-wise.
__global__ void __launch_bounds__(256)
    forward_dynamics_rollout_integrate_kernel(const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ qdd,
                                              int64_t count, float dt, int explicit_euler, float *__restrict__ q_out,
                                              float *__restrict__ qd_out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        float x = q[i], v = qd[i];
        rollout_step(x, v, qdd[i], dt, explicit_euler != 0);
        q_out[i] = x;
        qd_out[i] = v;
    }
}

enum RolloutKind { ROLLOUT_COMPOSED = 0, ROLLOUT_ARM = 1, ROLLOUT_FINGERS = 2 };

// which fused kernel takes the full tiles of this walk (ROLLOUT_COMPOSED: none); `aligned`: every pointer is 16-byte aligned
static RolloutKind rollout_kind(const drm_walk *w, int64_t B, bool aligned) {
    if (!full_tiles_fit(B) || !table_aligned(w)) return ROLLOUT_COMPOSED;
    if ((w->shape & DRM_WALK_FINGERS)) {
        int K, L;
        if (fingers_shape(w, K, L)) return ROLLOUT_FINGERS;
    }
    if (arm7_walk(w) && aligned) {
        // an arm whose own two-samples-per-lane kernel drm_forward_dynamics runs at this size (DRM_SPECIAL_FD_ARM2): from
        // DRM_ROLLOUT_COMPOSED_MIN_PAIRS pairs of tiles on, the composed steps are faster than the fused kernel
        if (w->special[DRM_SPECIAL_FD_ARM2] && w->special[DRM_SPECIAL_FD_ARM] && (B / WAVE) / 2 >= DRM_ROLLOUT_COMPOSED_MIN_PAIRS)
            return ROLLOUT_COMPOSED;
        return ROLLOUT_ARM;
    }
    return ROLLOUT_COMPOSED;
}

static int launch_rollout_fused(RolloutKind kind, const drm_walk *w, const float *q0, const float *qd0, const float *tau, int64_t B,
                                int T, float dt, int flags, float *q_traj, float *qd_traj, float *qdd_traj, bool aligned, hipStream_t s) {
    const int n = w->n_dofs, n_tiles = (int)(B / WAVE);
    if (kind == ROLLOUT_ARM) {
        const int vec = aligned && (B * n) % 4 == 0;
        const dim3 grid((unsigned)((n_tiles + MAX_WAVES_PER_BLOCK - 1) / MAX_WAVES_PER_BLOCK)), block(WAVE * MAX_WAVES_PER_BLOCK);
        if (arm_links(w) == 7)
            hipLaunchKernelGGL((forward_dynamics_rollout_arm_kernel<8, 7, 7>), grid, block, 0, s, w->ops_f, q0, qd0, tau, B, T, dt, n_tiles,
                               flags, q_traj, qd_traj, qdd_traj, vec);
        else
            hipLaunchKernelGGL((forward_dynamics_rollout_arm_kernel<8, 7, 8>), grid, block, 0, s, w->ops_f, q0, qd0, tau, B, T, dt, n_tiles,
                               flags, q_traj, qd_traj, qdd_traj, vec);
    } else {
        const int K = DRM_WALK_AH_K(w->shape), L = DRM_WALK_AH_L(w->shape);
        const int vec = aligned && n % 4 == 0;
#define X(l)                                                                                                                      \
    if (L == l)                                                                                                                   \
        hipLaunchKernelGGL((forward_dynamics_rollout_fingers_kernel<l>), dim3((unsigned)n_tiles), dim3(WAVE * K), 0, s, w->ops_f, q0, qd0, \
                           tau, B, T, dt, n, flags, q_traj, qd_traj, qdd_traj, vec);
        X(2) X(3) X(4)
#undef X
    }
    return launched();
}

// Steps of rows [lo, B) of every slab: drm_forward_dynamics on the slab, then the integrator.  qdd goes to qdd_traj or to the front
// of the scratch; drm_forward_dynamics's own scratch follows it.
static int rollout_composed(const drm_walk *w, const float *q0, const float *qd0, const float *tau, int64_t B, int64_t lo, int T,
                            float dt, int flags, float *q_traj, float *qd_traj, float *qdd_traj, float *scratch, hipStream_t s) {
    const int n = w->n_dofs;
    const int64_t rows = B - lo, count = rows * n, slab = B * n;
    float *qdd_buf = nullptr, *fd_scratch = scratch;
    if (!qdd_traj) {
        if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_forward_dynamics_rollout_scratch_floats() floats of scratch (or qdd_traj)");
        qdd_buf = scratch;
        fd_scratch = scratch + ((count + 3) & ~(int64_t)3);
    }
    const int fd_flags = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING), expl = (flags & DRM_ROLLOUT_EXPLICIT_EULER) != 0;
    const int64_t blocks64 = (count + 255) / 256;
    const unsigned blocks = (unsigned)(blocks64 < 8192 ? blocks64 : 8192);
    for (int t = 0; t < T; ++t) {
        const int64_t off = (int64_t)t * slab + lo * n;
        const float *qi = t ? q_traj + off - slab : q0 + lo * n, *qdi = t ? qd_traj + off - slab : qd0 + lo * n;
        float *acc = qdd_traj ? qdd_traj + off : qdd_buf;
        int rc = drm_forward_dynamics(w, qi, qdi, tau + off, rows, fd_flags, acc, fd_scratch, s);
        if (rc) return rc;
        hipLaunchKernelGGL(forward_dynamics_rollout_integrate_kernel, dim3(blocks), dim3(256), 0, s, qi, qdi, (const float *)acc, count, dt,
                           expl, q_traj + off, qd_traj + off);
        rc = launched();
        if (rc) return rc;
    }
    return DRM_OK;
}

} // namespace drm

using namespace drm;

static int64_t drm_forward_dynamics_rollout_scratch_floats_impl(const drm_walk *w, int64_t B, bool aligned) {
    if (check_walk(w) || B <= 0) return 0;
    const int n = w->n_dofs;
    const int64_t lo = rollout_kind(w, B, aligned) != ROLLOUT_COMPOSED ? B / WAVE * WAVE : 0;
    if (lo == B) return 0;
    // (a slab start is 16-byte aligned only when B * n is a multiple of 4: otherwise drm_forward_dynamics sees misaligned pointers)
    const int64_t fd = aligned && (B * n) % 4 == 0 ? drm_forward_dynamics_scratch_floats_aligned(w, B) : drm_forward_dynamics_scratch_floats(w, B);
    return (((B - lo) * n + 3) & ~(int64_t)3) + fd;
}
extern "C" int64_t drm_forward_dynamics_rollout_scratch_floats(const drm_walk *w, int64_t B) {
    return drm_forward_dynamics_rollout_scratch_floats_impl(w, B, false);
}
extern "C" int64_t drm_forward_dynamics_rollout_scratch_floats_aligned(const drm_walk *w, int64_t B) {
    return drm_forward_dynamics_rollout_scratch_floats_impl(w, B, true);
}

extern "C" int drm_forward_dynamics_rollout(const drm_walk *w, const float *q0, const float *qd0, const float *tau, int64_t B, int32_t T,
                                            float dt, int32_t flags, float *q_traj, float *qd_traj, float *qdd_traj, float *scratch,
                                            void *stream) {
    int rc = args_forward_dynamics_rollout(w, q0, qd0, tau, B, T, dt, q_traj, qd_traj);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool aligned = aligned16(q0, qd0, tau, q_traj, qd_traj, qdd_traj);
    const RolloutKind kind = rollout_kind(w, B, aligned);
    int64_t lo = 0;
    if (kind != ROLLOUT_COMPOSED) {
        rc = launch_rollout_fused(kind, w, q0, qd0, tau, B, T, dt, (int)flags, q_traj, qd_traj, qdd_traj, aligned, s);
        if (rc) return rc;
        lo = B / WAVE * WAVE;
        if (lo == B) return DRM_OK;
    }
    return rollout_composed(w, q0, qd0, tau, B, lo, T, dt, (int)flags, q_traj, qd_traj, qdd_traj, scratch, s);
}

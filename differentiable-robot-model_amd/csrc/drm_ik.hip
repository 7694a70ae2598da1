// drm_ik.hip — ABI 15: batched inverse kinematics of one link by damped least squares, every iteration of a solve in one call
// (include/drm_hip.h drm_inverse_kinematics).  What a Python loop of compute_fk_and_jacobian, a batched 6 x 6 solve and the clamps
// does, without ~15 launches per iteration and without sending the [B, 6, n] Jacobians through HBM.
//
//   inverse_kinematics_arm_kernel      7-DoF arm chains, full 64-row tiles: the constant table staged in LDS ONCE for all
//                                      iterations, q, the target and the Jacobian in registers, the bounds in LDS; the wavefront
//                                      leaves the loop when none of its rows is still live (a converged row never changes again,
//                                      so the early exit changes no result)
//   inverse_kinematics_update_kernel   the composed path: max_iters + 1 rounds of drm_fk_jacobian into the scratch followed by this
//                                      kernel, one lane per row; every other robot, the ragged tail of a launch, misaligned
//                                      pointers and DRM_IK_COMPOSED.  All on the caller's stream, no host synchronisation, no
//                                      early exit.
// The per-row arithmetic (error, Cholesky solve, J^T y and the clamp) is drm_ik.hpp's, shared with the host build.
//
// Per row, fused: in q0 [n], target 7 floats; out q [n], err 2, iters 1 — 56 B in, 40 B out for n = 7, whatever the iteration count.
// Composed, per row and round: drm_fk_jacobian (4 n in, 4 (7 + 6 n) out), the update (4 (8 + 7 n) in, 8 n out).
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_ik.hpp"
#include "drm_sample.hpp"
#include "drm_args.hpp"

namespace drm {

template <int MAXN, class QA>
__device__ __forceinline__ bool ik_finite(const QA &q, int n) {
    bool ok = true;
#pragma unroll
    for (int d = 0; d < MAXN; ++d)
        if (d < n) ok = ok && isfinite(q[d]);
    return ok;
}

// Serial 7-DoF arm chains (DRM_WALK_ARM_CHAIN, capacity 8, target_perm 2), full tiles: fk_jacobian_arm_kernel's chain in its
// op-by-op form (table rows read from LDS inside the walk) once per iteration, then drm_ik.hpp's update.
// LDS per wavefront: [ table : CAP x 32 ][ lower : 8 ][ upper : 8 ][ q tile : 64 x NJ ][ err tile : 64 x 2 ]; the q and err
// tiles are written once, at the end, and leave with 16-byte stores.
template <int CAP, int NJ>
__global__ void __launch_bounds__(WAVE)
    inverse_kinematics_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q0, const float *__restrict__ tpos,
                                  const float *__restrict__ tquat, int n_tiles, int max_iters, IkOpts o, const float *__restrict__ lower,
                                  const float *__restrict__ upper, int pos_only, float *__restrict__ q, float *__restrict__ err,
                                  int32_t *__restrict__ iters) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(NJ <= 8, "the bounds rows hold 8 DoFs");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, Q_FLOATS = round4(WAVE * NJ);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 16 + Q_FLOATS + 2 * WAVE];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *llo = lc + C_FLOATS, *lhi = llo + 8, *lq = lhi + 8, *le = lq + Q_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE, b = b0 + lane;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], tp[3], tq[4] = {0.0f, 0.0f, 0.0f, 1.0f};
#pragma unroll
    for (int d = 0; d < NJ; ++d) qv[d] = q0[b * NJ + d];
#pragma unroll
    for (int i = 0; i < 3; ++i) tp[i] = tpos[b * 3 + i];
    if (!pos_only) {
        const float4 t4 = reinterpret_cast<const float4 *>(tquat)[b];
        tq[0] = t4.x; tq[1] = t4.y; tq[2] = t4.z; tq[3] = t4.w;
        ik_normalize_quat(tq);
    }
    const bool clamp = lower != nullptr;
    if (clamp && lane < (unsigned)NJ) { llo[lane] = lower[lane]; lhi[lane] = upper[lane]; }
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    bool live = true;
    float pos_err = 0.0f, rot_err = 0.0f;
    int it = 0;
#pragma unroll 1
    for (int i = 0;; ++i) {
        // the table rows are re-read from LDS in every iteration: hoisted out of the loop they would hold 96 VGPRs for its whole
        // length (the register-resident PRE form of fk_jacobian_arm_kernel), which halves the occupancy
        asm volatile("" ::: "memory");
        // a row whose q is not finite walks the chain at q = 0 and gets a NaN error (it never converges and stays NaN): a NaN angle
        // in any lane would send the whole wavefront's sines and cosines down chain_trig's slow path and change other rows' bits
        float qk[NJ];
        const bool bad = !ik_finite<NJ>(qv, NJ);
#pragma unroll
        for (int d = 0; d < NJ; ++d) qk[d] = bad ? 0.0f : qv[d];
        PoseP ee;
        f2 Bk[NJ][3];
        fk_chain_pairs<CAP, NJ>(row, qk, ee, Bk, [] {});
        const float pe[3] = {bad ? __builtin_nanf("") : ee.B[0][1], ee.B[1][1], ee.B[2][1]};
        float Jp[3][NJ], Jw[3][NJ];
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const float z[3] = {Bk[k][0][0], Bk[k][1][0], Bk[k][2][0]};
            const float dp[3] = {pe[0] - Bk[k][0][1], pe[1] - Bk[k][1][1], pe[2] - Bk[k][2][1]};
            float c[3];
            cross3(z, dp, c); // robot_model.py:661
#pragma unroll
            for (int r = 0; r < 3; ++r) { Jp[r][k] = c[r]; Jw[r][k] = z[r]; }
        }
        float cq[4] = {0.0f, 0.0f, 0.0f, 1.0f};
        if (!pos_only) { // (wave-uniform)
            Pose E;
            pose_from_pairs(ee, E);
            quat_xyzw(E.R, cq);
        }
        if (live) {
            auto J = [&](int r, int k) -> float { return r < 3 ? Jp[r][k] : Jw[r - 3][k]; };
            auto qf = [&](int k) -> float & { return qv[k]; };
            float pe_, re_;
            if (ik_iteration(J, NJ, pe, cq, tp, tq, pos_only != 0, o, i == max_iters, qf, clamp ? llo : nullptr, clamp ? lhi : nullptr,
                             pe_, re_)) {
                live = false;
                pos_err = pe_;
                rot_err = re_;
                it = i;
            }
        }
        if (!DRM_WAVE_ANY(live)) break;
    }
#pragma unroll
    for (int d = 0; d < NJ; ++d) lq[lane * NJ + d] = qv[d];
    le[lane * 2] = pos_err;
    le[lane * 2 + 1] = rot_err;
    wave_lds_sync();
    tile_store<NJ>(q + b0 * NJ, WAVE, NJ, 0u, lq, lane, true);
    tile_store<2>(err + b0 * 2, WAVE, 2, 0u, le, lane, true);
    if (iters) iters[b] = it;
}

// q of a row as drm_fk_jacobian reads it in the composed path: q, or 0 where the row's q is not finite (as in the fused kernel: a NaN
// angle would send the sines and cosines of its whole tile down chain_trig's slow path and change other rows' bits)
__device__ __forceinline__ void ik_fk_input(const float *q, int n, float *qfk) {
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && isfinite(q[k]);
    for (int k = 0; k < n; ++k) qfk[k] = ok ? q[k] : 0.0f;
}

// The composed path's start, one lane per row: q = q0, and the FK input of round 0
__global__ void __launch_bounds__(64)
    inverse_kinematics_start_kernel(const float *__restrict__ q0, int64_t rows, int n, float *__restrict__ q, float *__restrict__ qfk) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    for (int k = 0; k < n; ++k) q[b * n + k] = q0[b * n + k];
    ik_fk_input(q0 + b * n, n, qfk + b * n);
}

// The composed path's update, one lane per row of [0, rows): the row's FK + Jacobian of round i (pos, quat, lin, ang, as
// drm_fk_jacobian wrote them from qfk) and drm_ik.hpp's update of q in place, then the FK input of the next round.  Round 0 sets
// the row's done flag; later rounds skip a row that is done.  64-lane blocks: the rows of a small batch spread over as many CUs as
// possible.
__global__ void __launch_bounds__(64)
    inverse_kinematics_update_kernel(const float *__restrict__ pos, const float *__restrict__ quat, const float *__restrict__ lin,
                                     const float *__restrict__ ang, const float *__restrict__ tpos, const float *__restrict__ tquat,
                                     int64_t rows, int n, int i, int max_iters, IkOpts o, const float *__restrict__ lower,
                                     const float *__restrict__ upper, int pos_only, int32_t *done, float *__restrict__ q,
                                     float *__restrict__ qfk, float *__restrict__ err, int32_t *__restrict__ iters) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    if (i > 0 && done[b]) return;
    float *qo = q + b * n;
    const float *lr = lin + b * 3 * n, *ar = ang + b * 3 * n;
    float tp[3] = {tpos[b * 3], tpos[b * 3 + 1], tpos[b * 3 + 2]}, tq[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    float p[3] = {pos[b * 3], pos[b * 3 + 1], pos[b * 3 + 2]}, c[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    if (!pos_only) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { tq[k] = tquat[b * 4 + k]; c[k] = quat[b * 4 + k]; }
        ik_normalize_quat(tq);
    }
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && isfinite(qo[k]);
    if (!ok) p[0] = __builtin_nanf(""); // (FK ran at q = 0: the row's error is NaN)
    auto J = [&](int r, int k) -> float { return r < 3 ? lr[r * n + k] : ar[(r - 3) * n + k]; };
    auto qf = [&](int k) -> float & { return qo[k]; };
    float pos_err, rot_err;
    const bool stop = ik_iteration(J, n, p, c, tp, tq, pos_only != 0, o, i == max_iters, qf, lower, upper, pos_err, rot_err);
    done[b] = stop;
    if (stop) {
        err[b * 2] = pos_err;
        err[b * 2 + 1] = rot_err;
        if (iters) iters[b] = i;
    } else {
        ik_fk_input(qo, n, qfk + b * n);
    }
}

// the fused kernel takes the full tiles of this walk (the rows where drm_fk_jacobian itself launches the arm kernel)
static bool ik_fused(const drm_walk *w, int64_t B, bool aligned) {
    return arm7_walk(w) && w->target_perm == 2 && aligned && table_aligned(w) && full_tiles_fit(B);
}

// scratch of the composed path over `rows` rows: pos, quat, lin, ang of drm_fk_jacobian, its input qfk and the done flags, each
// 16-byte aligned
struct IkScratch {
    int64_t pos, quat, lin, ang, qfk, done, total;
};
static IkScratch ik_scratch_layout(int64_t rows, int n) {
    auto r4 = [](int64_t x) { return (x + 3) & ~(int64_t)3; };
    IkScratch s;
    s.pos = 0;
    s.quat = s.pos + r4(rows * 3);
    s.lin = s.quat + r4(rows * 4);
    s.ang = s.lin + r4(rows * 3 * n);
    s.qfk = s.ang + r4(rows * 3 * n);
    s.done = s.qfk + r4(rows * n);
    s.total = s.done + r4(rows);
    return s;
}

} // namespace drm

using namespace drm;

static int64_t drm_inverse_kinematics_scratch_floats_impl(const drm_walk *w, int64_t B, bool aligned) {
    if (check_walk(w) || B <= 0) return 0;
    const int64_t lo = ik_fused(w, B, aligned) ? B / WAVE * WAVE : 0;
    if (lo == B) return 0;
    return ik_scratch_layout(B - lo, w->n_dofs).total;
}
extern "C" int64_t drm_inverse_kinematics_scratch_floats(const drm_walk *w, int64_t B) {
    return drm_inverse_kinematics_scratch_floats_impl(w, B, false);
}
extern "C" int64_t drm_inverse_kinematics_scratch_floats_aligned(const drm_walk *w, int64_t B) {
    return drm_inverse_kinematics_scratch_floats_impl(w, B, true);
}

extern "C" int drm_inverse_kinematics(const drm_walk *w, const float *q0, const float *target_pos, const float *target_quat, int64_t B,
                                      int32_t max_iters, float damping, float step, float tol_pos, float tol_rot, const float *lower,
                                      const float *upper, int32_t flags, float *q, float *err, int32_t *iters, float *scratch,
                                      void *stream) {
    int rc = args_inverse_kinematics(w, q0, target_pos, target_quat, B, max_iters, damping, step, tol_pos, tol_rot, lower, upper, flags, q, err);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    const bool pos_only = (flags & DRM_IK_POSITION_ONLY) != 0;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs;
    const IkOpts o = {damping * damping, step, tol_pos, tol_rot};
    const bool aligned = aligned16(q0, target_pos, target_quat, q, err, iters);
    int64_t lo = 0;
    if (!(flags & DRM_IK_COMPOSED) && ik_fused(w, B, aligned)) {
        const int n_tiles = (int)(B / WAVE);
        hipLaunchKernelGGL((inverse_kinematics_arm_kernel<8, 7>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q0, target_pos,
                           target_quat, n_tiles, (int)max_iters, o, lower, upper, (int)pos_only, q, err, iters);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the composed path over rows [lo, B)
    if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_inverse_kinematics_scratch_floats() floats of scratch");
    const int64_t rows = B - lo;
    if (rows / 64 >= GRID_MAX) return fail(DRM_ERR_UNSUPPORTED, "batch too large");
    const IkScratch L = ik_scratch_layout(rows, n);
    float *pos = scratch + L.pos, *quat = scratch + L.quat, *lin = scratch + L.lin, *ang = scratch + L.ang;
    float *qfk = scratch + L.qfk;
    int32_t *done = reinterpret_cast<int32_t *>(scratch + L.done);
    const float *q0r = q0 + lo * n, *tpr = target_pos + lo * 3, *tqr = target_quat ? target_quat + lo * 4 : nullptr;
    float *qr = q + lo * n, *er = err + lo * 2;
    int32_t *itr = iters ? iters + lo : nullptr;
    const unsigned blocks = (unsigned)((rows + 63) / 64);
    hipLaunchKernelGGL(inverse_kinematics_start_kernel, dim3(blocks), dim3(64), 0, s, q0r, rows, n, qr, qfk);
    rc = launched();
    if (rc) return rc;
    for (int i = 0; i <= max_iters; ++i) {
        rc = drm_fk_jacobian(w, qfk, rows, pos, quat, lin, ang, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(inverse_kinematics_update_kernel, dim3(blocks), dim3(64), 0, s, (const float *)pos, (const float *)quat,
                           (const float *)lin, (const float *)ang, tpr, tqr, rows, n, i, (int)max_iters, o, lower, upper, (int)pos_only,
                           done, qr, qfk, er, itr);
        rc = launched();
        if (rc) return rc;
    }
    return DRM_OK;
}

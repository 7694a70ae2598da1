// drm_idd.hip — tau = ID(q, qd, qdd) and its first-order derivatives dtau/dq, dtau/dqd and dtau/dqdd = H(q) in one call
// (include/drm_hip.h drm_rnea_derivatives).  What a caller otherwise gets from n backward passes through inverse dynamics with one-hot
// cotangents plus an inertia-matrix call, or from -H dqdd/dq out of the forward-dynamics derivatives at the cost of cond(H).
//
//   rnea_derivatives_arm_kernel    serial 7-DoF arm chains, full 64-row tiles, 16-byte aligned pointers: one wavefront per tile, one row
//                                  per lane, the constant table staged in LDS once, ONE chain_trig; the links' velocities and
//                                  accelerations, the composite of the chain below a joint and the four wrenches that climb its ancestors
//                                  stay in registers (drm_idd.hpp idd_chain_trig).  dtau/dq and dtau/dqd land in the lane's stretches of
//                                  TWO 64 x 49 tiles in LDS (odd pitch) as they are formed and leave in 16-byte stores; the triangle of H
//                                  and tau wait in registers and leave through the first tile after them.  A tile of each output is
//                                  contiguous and 16-byte aligned.  26 KB of LDS per wavefront.
//   rnea_derivatives_rows_kernel   every other walk (trees, hands, prismatic joints, two-op skew-axis links, fixed ops kept for learnable
//                                  links), the ragged tail of an arm launch, misaligned pointers, DRM_IDD_COMPOSED: one lane per row,
//                                  loops over the ops (drm_idd.hpp idd_tree_walk), ALL segments of the walk on the one wavefront.
//                                  Between the sweeps a row keeps 15 floats per op and 28 per branch point, placed by drm_rows.hpp
//                                  (LDS up to IDD_LDS_BYTES).  Its rows of the three matrices are zeroed by hipMemsetAsync ahead
//                                  of it and the kernel stores the entries between a joint and its ancestors only: entries between
//                                  branches are exact zeros.
//
// Per row, fused, n = 7: in q, qd, qdd (84 B); out 4 (3 * 49 + 7) B = 616 B.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_idd.hpp"
#include "drm_rows.hpp"
#include "drm_args.hpp"

namespace drm {

constexpr int IDD_LDS_BYTES = 32 * 1024; // per-row state of the general kernel in LDS up to here (five blocks per CU)

static inline int idd_state_floats(const drm_walk *w) { return IDD_REC_FLOATS * w->n_ops + IDD_SLOT_FLOATS * w->n_slots; }

template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE)
    rnea_derivatives_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd,
                                const float *__restrict__ qdd, int n_tiles, int flags, float *__restrict__ tau, float *__restrict__ dq,
                                float *__restrict__ dqd, float *__restrict__ H) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int NN = NJ * NJ;
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * NN);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 2 * T_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lt0 = smem + C_FLOATS, *lt1 = lt0 + T_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;
    const bool gravity = flags & DRM_RNEA_GRAVITY, damping = flags & DRM_RNEA_DAMPING;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], qdv[NJ], qddv[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qdv[d] = qd[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qddv[d] = qdd[r0 + d];
    }
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    // a row that cannot be used walks the chain at rest at q = 0 and gets NaN outputs: its angles would send the whole wavefront's
    // sines and cosines down chain_trig's slow path and change other rows' bits
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || idd_bad_input(qv[d], qdv[d], qddv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; qddv[d] = bad ? 0.0f : qddv[d]; }
    const float nan = __builtin_nanf("");

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    // dtau/dq and dtau/dqd go into the lane's stretches of the two tiles as they are formed; the triangle of H and tau wait in registers
    float *mine0 = lt0 + lane * NN, *mine1 = lt1 + lane * NN;
    float Ht[NJ * (NJ + 1) / 2], tv[NJ];
    idd_chain_trig<LINKS, NJ>(
        row, gravity ? 9.81f : 0.0f, damping, cs, sn, qdv, qddv, [](int) { return true; },
        [&](int which, int i, int j, float v) {
            if (which == IDD_DQ) mine0[i * NJ + j] = bad ? nan : v;
            else if (which == IDD_DQD) mine1[i * NJ + j] = bad ? nan : v;
            else if (i >= j) Ht[tri_index(i, j)] = v;
        },
        [&](int j, float v) { tv[j] = v; });
    wave_lds_sync();
    if (dq) tile_store<NN>(dq + b0 * NN, WAVE, NN, 0u, lt0, lane, true);
    if (H) {
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < NJ; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const float v = bad ? nan : Ht[tri_index(i, j)];
                mine0[i * NJ + j] = v;
                mine0[j * NJ + i] = v;
            }
    }
    if (dqd) tile_store<NN>(dqd + b0 * NN, WAVE, NN, 0u, lt1, lane, true);
    if (H) {
        wave_lds_sync();
        tile_store<NN>(H + b0 * NN, WAVE, NN, 0u, lt0, lane, true);
    }
    if (tau) {
        wave_lds_sync();
#pragma unroll
        for (int d = 0; d < NJ; ++d) lt1[lane * NJ + d] = bad ? nan : tv[d];
        wave_lds_sync();
        tile_store<NJ>(tau + b0 * NJ, WAVE, NJ, 0u, lt1, lane, true);
    }
}

// The general kernel.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles.  The lanes' records and parked
// composites: drm_rows.hpp rows_state.  The matrices arrive zeroed.
template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
    rnea_derivatives_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int p_end,
                                 int n_slots, int n, const float *__restrict__ q, const float *__restrict__ qd,
                                 const float *__restrict__ qdd, int64_t B, int64_t n_tiles, int flags, float *__restrict__ tau,
                                 float *__restrict__ dq, float *__restrict__ dqd, float *__restrict__ H, float *__restrict__ scratch,
                                 int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<IDD_REC_FLOATS, WAVE> recs = {state};
    const Records<IDD_SLOT_FLOATS, WAVE> slots = {state + IDD_REC_FLOATS * n_ops * WAVE};
    const RowsCtl ctl(ops_i, cap);
    const float nan = __builtin_nanf("");
    const bool gravity = flags & DRM_RNEA_GRAVITY, damping = flags & DRM_RNEA_DAMPING;
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue; // (a lane shares nothing with its neighbours: no barrier below)
        const float *qr = q + r * n, *qdr = qd + r * n, *qddr = qdd + r * n;
        float *tr = tau ? tau + r * n : nullptr;
        float *Mr[3] = {dq ? dq + r * n * n : nullptr, dqd ? dqd + r * n * n : nullptr, H ? H + r * n * n : nullptr};
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || idd_bad_input(qr[d], qdr[d], qddr[d]);
        idd_tree_walk(
            n_ops, p_end, n_slots, gravity ? 9.81f : 0.0f, damping, ctl, row,
            [&](int d, float &a, float &v, float &acc) { a = bad ? 0.0f : qr[d]; v = bad ? 0.0f : qdr[d]; acc = bad ? 0.0f : qddr[d]; },
            [&](int k, const float *x) { recs.put(k, x); }, [&](int k, float *x) { recs.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int which, int i, int j, float v) {
                float *M = which == IDD_DQ ? Mr[0] : which == IDD_DQD ? Mr[1] : Mr[2];
                if (M && i >= 0 && j >= 0 && i < n && j < n) M[i * n + j] = bad ? nan : v;
            },
            [&](int j, float v) {
                if (tr && j >= 0 && j < n) tr[j] = bad ? nan : v;
            });
    }
}

} // namespace drm

using namespace drm;

static int64_t idd_scratch(const drm_walk *w, int64_t B, bool aligned) {
    return check_sweep_walk(w) ? 0 : rows_scratch_floats(w, B, aligned, idd_state_floats(w), IDD_LDS_BYTES);
}
extern "C" int64_t drm_rnea_derivatives_scratch_floats(const drm_walk *w, int64_t B) { return idd_scratch(w, B, false); }
extern "C" int64_t drm_rnea_derivatives_scratch_floats_aligned(const drm_walk *w, int64_t B) { return idd_scratch(w, B, true); }

extern "C" int drm_rnea_derivatives(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                                    float *tau, float *dq, float *dqd, float *H, float *scratch, void *stream) {
    int rc = args_rnea_derivatives(w, q, qd, qdd, B, tau, dq, dqd, H);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs;
    const int fl = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    int64_t lo = 0;
    if (!(flags & DRM_IDD_COMPOSED) && rows_fused(w, B, aligned16(q, qd, qdd, tau, dq, dqd, H))) {
        const int n_tiles = (int)(B / WAVE);
        if (arm_links(w) == 7)
            hipLaunchKernelGGL((rnea_derivatives_arm_kernel<8, 7, 7>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, qdd, n_tiles,
                               fl, tau, dq, dqd, H);
        else
            hipLaunchKernelGGL((rnea_derivatives_arm_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, qdd, n_tiles,
                               fl, tau, dq, dqd, H);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general kernel over rows [lo, B)
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, idd_state_floats(w), IDD_LDS_BYTES);
    const int p_end = w->n_segments > 1 ? w->prefix_end : 0;
    const float *qs = q + lo * n, *qds = qd + lo * n, *qdds = qdd + lo * n;
    float *ts = tau ? tau + lo * n : nullptr, *dqs = dq ? dq + lo * n * n : nullptr, *dqds = dqd ? dqd + lo * n * n : nullptr,
          *Hs = H ? H + lo * n * n : nullptr;
    rc = rows_zero({dqs, dqds, Hs}, (size_t)rows * n * n, s);
    if (rc) return rc;
    return rows_launch(rnea_derivatives_rows_kernel<true>, rnea_derivatives_rows_kernel<false>, plan, scratch,
                       "drm_rnea_derivatives_scratch_floats", s, w->ops_f, w->ops_i, (int)w->capacity, (int)w->n_ops, p_end, (int)w->n_slots, n, qs,
                       qds, qdds, rows, plan.tiles, fl, ts, dqs, dqds, Hs);
}

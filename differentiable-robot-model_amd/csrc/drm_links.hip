// drm_links.hip — the links' positions, velocities and classical accelerations (drm_link_motion) and the joint torques of external
// wrenches on the links (drm_external_torques), each in one call over a many-target FK walk (include/drm_hip.h).  What a caller
// otherwise composes from one drm_fk_jacobian launch (168 B per row, thrown away after one product) and two small products PER LINK.
// The two are adjoint to each other — sum_l f_l . v_l + m_l . w_l == tau . qd — and serve as each other's backward pass.
//
//   link_motion_arm_kernel    serial 7-DoF arm chains of 8 ops, every op a target in walk order, full 64-row tiles, 16-byte aligned
//                             pointers: one wavefront per tile, one row per lane, the constant table staged in LDS once, ONE
//                             chain_trig; the chain's state and the T x 3 floats of every requested output stay in registers
//                             (drm_links.hpp link_chain_motion).  Each requested [64, T, 3] tile is assembled in ONE LDS buffer
//                             (row stride 3 T + 1 words: no bank conflicts) and leaves whole in 16-byte stores, one output after
//                             the other.  Three instantiations: positions alone, + velocities, + accelerations.
//   link_torques_arm_kernel   the same tiles: the two [64, T, 3] wrench tiles come in through LDS in 16-byte loads, the origins of
//                             the 8 links and the axes of the 7 joints stay in registers from the sweep out, the [64, 7] tile of
//                             torques leaves through LDS as drm_energy's p does.
//   link_motion_rows_kernel, link_torques_rows_kernel
//                             every other walk (trees, hands, prismatic joints, two-op skew-axis links, target subsets), the ragged
//                             tail of an arm launch, misaligned pointers, DRM_LINKS_COMPOSED: one lane per row, loops over the ops
//                             (drm_links.hpp link_motion_walk / link_torques_walk).  A row keeps 24 floats per branch point
//                             (motion) or 12 floats per op and 24 per branch point (torques), placed by drm_rows.hpp.
//   link_power_dq_arm_kernel, link_power_dq_rows_kernel
//                             drm_link_power_dq, the q-gradient of both sweeps as dS/dq of the power S = sum_l f_l . v_l + m_l . w_l:
//                             the torques kernels with the velocities carried outwards and one more free vector inwards
//                             (drm_links.hpp link_chain_power_dq / link_power_dq_walk); tau, when asked for, is drm_external_torques'
//                             to the bit.  Same dispatch, same tiles; the general kernel keeps 21 floats per op.
//
// Per row, fused, T = 8: motion 84 B in (q, qd, qdd), up to 5 x 96 = 480 B out; torques 28 + 2 x 96 = 220 B in, 28 B out; power
// gradient 56 + 2 x 96 = 248 B in, 28 B (dq) or 56 B (dq and tau) out.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_links.hpp"
#include "drm_rows.hpp"
#include "drm_args.hpp"

namespace drm {

constexpr int LINKS_LDS_BYTES = 32 * 1024; // per-row state of the general kernels in LDS up to here (five blocks per CU)

// (a walk without branch points still gets one slot's worth: a plan of zero floats would read as "the state lives in the scratch")
static inline int motion_state_floats(const drm_walk *w) { return LINKS_SLOT_FLOATS * (w->n_slots > 0 ? w->n_slots : 1); }
static inline int torques_state_floats(const drm_walk *w) { return LINKS_REC_FLOATS * w->n_ops + LINKS_SLOT_FLOATS * w->n_slots; }
static inline int power_dq_state_floats(const drm_walk *w) { return LINKS_DQ_REC_FLOATS * w->n_ops + LINKS_SLOT_FLOATS * w->n_slots; }

// floor(w / S) == umulhi(w, tile_magic(S)) for w S < 2^32 (drm_common.hpp div_magic, as a constant)
constexpr uint32_t tile_magic(int S) { return (uint32_t)((((uint64_t)1 << 32) + (uint64_t)S - 1) / (uint64_t)S); }

// MODE 0: positions alone; 1: + velocities; 2: + accelerations.  Outputs whose pointer is NULL are not stored (wave-uniform).
template <int CAP, int NJ, int LINKS, int MODE>
__global__ void __launch_bounds__(WAVE)
    link_motion_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd,
                           const float *__restrict__ qdd, int n_tiles, float *__restrict__ pos, float *__restrict__ lin_vel,
                           float *__restrict__ ang_vel, float *__restrict__ lin_acc, float *__restrict__ ang_acc) {
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int S = 3 * LINKS, SP = S | 1, NOUT = MODE == 0 ? 1 : MODE == 1 ? 3 : 5;
    static_assert(!(S & 1) && !((WAVE * S) & 3), "even row widths (padded LDS image), whole 16-byte stores");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * SP);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + T_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lt = smem + C_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], qdv[NJ], qddv[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qdv[d] = (MODE >= 1 && qd) ? qd[r0 + d] : 0.0f;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qddv[d] = (MODE >= 2 && qdd) ? qdd[r0 + d] : 0.0f;
    }
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    // a row that cannot be used walks the chain at rest at q = 0 and gets NaN outputs: its angles would send the whole wavefront's
    // sines and cosines down chain_trig's slow path and change other rows' bits
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || links_bad_input(qv[d], qdv[d], qddv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; qddv[d] = bad ? 0.0f : qddv[d]; }
    const float nan = __builtin_nanf("");

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    float o[NOUT][S];
    link_chain_motion<LINKS, NJ, (MODE >= 1), (MODE >= 2)>(row, cs, sn, qdv, qddv, [&](int k, const LinkState &st) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            o[0][3 * k + i] = st.p[i];
            if constexpr (MODE >= 1) { o[1][3 * k + i] = st.v[i]; o[2][3 * k + i] = st.w[i]; }
            if constexpr (MODE >= 2) { o[3][3 * k + i] = st.a[i]; o[4][3 * k + i] = st.al[i]; }
        }
    });
    float *const outs[5] = {pos, lin_vel, ang_vel, lin_acc, ang_acc};
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        if (!outs[j]) continue;
#pragma unroll
        for (int i = 0; i < S; ++i) lt[lane * SP + i] = bad ? nan : o[j][i];
        wave_lds_sync();
        tile_store<S>(outs[j] + b0 * S, WAVE, S, tile_magic(S), lt, lane, false, true);
        wave_lds_sync();
    }
}

template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE)
    link_torques_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ force,
                            const float *__restrict__ torque, int n_tiles, float *__restrict__ tau) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int S = 3 * LINKS, SP = S | 1;
    static_assert(!(S & 1) && !((WAVE * S) & 3), "even row widths (padded LDS image), whole 16-byte loads");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * SP);
    static_assert(WAVE * NJ <= T_FLOATS, "the torque tile reuses a wrench tile's buffer");
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 2 * T_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lf = smem + C_FLOATS, *lm = lf + T_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
    }
    if (force) tile_load<S>(force + b0 * S, WAVE, S, tile_magic(S), lf, lane, false, true);
    if (torque) tile_load<S>(torque + b0 * S, WAVE, S, tile_magic(S), lm, lane, false, true);
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || lag_bad_input(qv[d], 0.0f);
#pragma unroll
    for (int d = 0; d < NJ; ++d) qv[d] = bad ? 0.0f : qv[d];
    const float nan = __builtin_nanf("");

    float fw[S], tw[S];
#pragma unroll
    for (int i = 0; i < S; ++i) fw[i] = force ? lf[lane * SP + i] : 0.0f;
#pragma unroll
    for (int i = 0; i < S; ++i) tw[i] = torque ? lm[lane * SP + i] : 0.0f;
    wave_lds_sync(); // (the torque tile below reuses lf)

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    float *lp = lf + lane * NJ;
    link_chain_torques<LINKS, NJ>(
        row, cs, sn,
        [&](int k, float *f, float *m) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { f[i] = fw[3 * k + i]; m[i] = tw[3 * k + i]; }
        },
        [&](int j, float v) { lp[j] = bad ? nan : v; });
    wave_lds_sync();
    tile_store<NJ>(tau + b0 * NJ, WAVE, NJ, 0u, lf, lane, true);
}

// The general kernels.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles.  The lanes' records and parked
// states: drm_rows.hpp rows_state.
template <bool IN_LDS, int MODE>
__global__ void __launch_bounds__(WAVE)
    link_motion_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int n_slots, int n, int T,
                            const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ qdd, int64_t B,
                            int64_t n_tiles, float *__restrict__ pos, float *__restrict__ lin_vel, float *__restrict__ ang_vel,
                            float *__restrict__ lin_acc, float *__restrict__ ang_acc, float *__restrict__ scratch, int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<LINKS_SLOT_FLOATS, WAVE> slots = {state};
    const RowsCtl ctl(ops_i, cap);
    const float nan = __builtin_nanf("");
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue; // (a lane shares nothing with its neighbours: no barrier below)
        const float *qr = q + r * n, *qdr = (MODE >= 1 && qd) ? qd + r * n : nullptr, *qddr = (MODE >= 2 && qdd) ? qdd + r * n : nullptr;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || links_bad_input(qr[d], qdr ? qdr[d] : 0.0f, qddr ? qddr[d] : 0.0f);
        const int64_t o0 = r * T * 3;
        link_motion_walk<(MODE >= 1), (MODE >= 2)>(
            n_ops, n_slots, ctl, row,
            [&](int d, float &a, float &v, float &acc) {
                a = bad ? 0.0f : qr[d];
                v = (bad || !qdr) ? 0.0f : qdr[d];
                acc = (bad || !qddr) ? 0.0f : qddr[d];
            },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int t, const LinkState &st) {
                if (t >= T) return;
                const int64_t at = o0 + 3 * t;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (pos) pos[at + i] = bad ? nan : st.p[i];
                    if constexpr (MODE >= 1) {
                        if (lin_vel) lin_vel[at + i] = bad ? nan : st.v[i];
                        if (ang_vel) ang_vel[at + i] = bad ? nan : st.w[i];
                    }
                    if constexpr (MODE >= 2) {
                        if (lin_acc) lin_acc[at + i] = bad ? nan : st.a[i];
                        if (ang_acc) ang_acc[at + i] = bad ? nan : st.al[i];
                    }
                }
            });
    }
}

template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
    link_torques_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int n_slots, int n, int T,
                             const float *__restrict__ q, const float *__restrict__ force, const float *__restrict__ torque, int64_t B,
                             int64_t n_tiles, float *__restrict__ tau, float *__restrict__ scratch, int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<LINKS_REC_FLOATS, WAVE> recs = {state};
    const Records<LINKS_SLOT_FLOATS, WAVE> slots = {state + LINKS_REC_FLOATS * n_ops * WAVE};
    const RowsCtl ctl(ops_i, cap);
    const float nan = __builtin_nanf("");
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue;
        const float *qr = q + r * n;
        const float *fr = force ? force + r * T * 3 : nullptr, *mr = torque ? torque + r * T * 3 : nullptr;
        float *tr = tau + r * n;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || lag_bad_input(qr[d], 0.0f);
        // (columns of DoFs that no target's chain crosses stay zero)
#pragma unroll 1
        for (int d = 0; d < n; ++d) tr[d] = bad ? nan : 0.0f;
        link_torques_walk(
            n_ops, n_slots, ctl, row, [&](int d) { return bad ? 0.0f : qr[d]; },
            [&](int k, const float *x) { recs.put(k, x); }, [&](int k, float *x) { recs.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int t, float *f, float *m) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    f[i] = (fr && t < T) ? fr[3 * t + i] : 0.0f;
                    m[i] = (mr && t < T) ? mr[3 * t + i] : 0.0f;
                }
            },
            [&](int j, float v) {
                if (j < n) tr[j] = bad ? nan : v;
            });
    }
}

// drm_link_power_dq, fused: link_torques_arm_kernel's tiles and LDS image, with the [64, 7] tiles of q and qd coming in through LDS in
// 16-byte loads as well.  The origins, velocities and angular velocities of the 8 links and the axes of the 7 joints stay in registers
// from the sweep out; the wrenches are read out of their LDS tiles on the way in (nothing else writes those), and the [64, 7] tiles of
// the gradient and of the torques leave through the buffers q and qd came in by.  tau NULL (wave-uniform): not stored.
template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE)
    link_power_dq_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd,
                             const float *__restrict__ force, const float *__restrict__ torque, int n_tiles, float *__restrict__ dq,
                             float *__restrict__ tau) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int S = 3 * LINKS, SP = S | 1;
    static_assert(!(S & 1) && !((WAVE * S) & 3), "even row widths (padded LDS image), whole 16-byte loads");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * SP), Q_FLOATS = round4(WAVE * NJ);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 2 * T_FLOATS + 2 * Q_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lf = smem + C_FLOATS, *lm = lf + T_FLOATS, *lq = lm + T_FLOATS, *lqd = lq + Q_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    tile_load<NJ>(q + b0 * NJ, WAVE, NJ, 0u, lq, lane, true);
    tile_load<NJ>(qd + b0 * NJ, WAVE, NJ, 0u, lqd, lane, true);
    if (force) tile_load<S>(force + b0 * S, WAVE, S, tile_magic(S), lf, lane, false, true);
    if (torque) tile_load<S>(torque + b0 * S, WAVE, S, tile_magic(S), lm, lane, false, true);
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    float qv[NJ], qdv[NJ];
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = lq[lane * NJ + d]; qdv[d] = lqd[lane * NJ + d]; }
    wave_lds_sync(); // (the gradient and torque tiles below reuse lq and lqd)

    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || lag_bad_input(qv[d], qdv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; }
    const float nan = __builtin_nanf("");

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    float *ldq = lq + lane * NJ, *ltau = lqd + lane * NJ;
    const float *lfr = lf + lane * SP, *lmr = lm + lane * SP;
    link_chain_power_dq<LINKS, NJ>(
        row, cs, sn, qdv,
        [&](int k, float *f, float *m) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { f[i] = force ? lfr[3 * k + i] : 0.0f; m[i] = torque ? lmr[3 * k + i] : 0.0f; }
        },
        [&](int j, float g, float t) {
            ldq[j] = bad ? nan : g;
            ltau[j] = bad ? nan : t;
        });
    wave_lds_sync();
    tile_store<NJ>(dq + b0 * NJ, WAVE, NJ, 0u, lq, lane, true);
    if (tau) tile_store<NJ>(tau + b0 * NJ, WAVE, NJ, 0u, lqd, lane, true);
}

template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
    link_power_dq_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int n_slots, int n, int T,
                              const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ force,
                              const float *__restrict__ torque, int64_t B, int64_t n_tiles, float *__restrict__ dq, float *__restrict__ tau,
                              float *__restrict__ scratch, int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<LINKS_DQ_REC_FLOATS, WAVE> recs = {state};
    const Records<LINKS_SLOT_FLOATS, WAVE> slots = {state + LINKS_DQ_REC_FLOATS * n_ops * WAVE};
    const RowsCtl ctl(ops_i, cap);
    const float nan = __builtin_nanf("");
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue;
        const float *qr = q + r * n, *qdr = qd + r * n;
        const float *fr = force ? force + r * T * 3 : nullptr, *mr = torque ? torque + r * T * 3 : nullptr;
        float *gr = dq + r * n, *tr = tau ? tau + r * n : nullptr;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || lag_bad_input(qr[d], qdr[d]);
        // (columns of DoFs that no target's chain crosses stay zero)
#pragma unroll 1
        for (int d = 0; d < n; ++d) {
            gr[d] = bad ? nan : 0.0f;
            if (tr) tr[d] = bad ? nan : 0.0f;
        }
        link_power_dq_walk(
            n_ops, n_slots, ctl, row,
            [&](int d, float &a, float &v) {
                a = bad ? 0.0f : qr[d];
                v = bad ? 0.0f : qdr[d];
            },
            [&](int k, const float *x) { recs.put(k, x); }, [&](int k, float *x) { recs.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int t, float *f, float *m) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    f[i] = (fr && t < T) ? fr[3 * t + i] : 0.0f;
                    m[i] = (mr && t < T) ? mr[3 * t + i] : 0.0f;
                }
            },
            [&](int j, float g, float t) {
                if (j >= n) return;
                gr[j] = bad ? nan : g;
                if (tr) tr[j] = bad ? nan : t;
            });
    }
}

// an arm7_walk of 8 ops whose every op is a target, slots in walk order: what the fused kernels are compiled for
static inline bool links_fused(const drm_walk *w, int T, int64_t B, int flags, bool aligned) {
    return !(flags & DRM_LINKS_COMPOSED) && (w->shape & DRM_WALK_TARGETS_ORDERED) && w->n_ops == 8 && T == 8 && rows_fused(w, B, aligned);
}

} // namespace drm

using namespace drm;

// The scratch of the general kernel over ALL B rows, whatever the alignment: whether a call is fused depends on n_targets, which the
// query does not see, and the plan's scratch grows with the rows, so this covers the tail of a fused call too.  (The walks the fused
// kernels take keep their state in LDS: 0 either way.)
static int64_t links_scratch(const drm_walk *w, int64_t B, int state_floats) {
    return (check_sweep_walk(w) || B <= 0) ? 0 : rows_plan(B, state_floats, LINKS_LDS_BYTES).scratch_floats;
}
extern "C" int64_t drm_link_motion_scratch_floats(const drm_walk *w, int64_t B) { return links_scratch(w, B, w ? motion_state_floats(w) : 0); }
extern "C" int64_t drm_link_motion_scratch_floats_aligned(const drm_walk *w, int64_t B) { return drm_link_motion_scratch_floats(w, B); }
extern "C" int64_t drm_external_torques_scratch_floats(const drm_walk *w, int64_t B) {
    return links_scratch(w, B, w ? torques_state_floats(w) : 0);
}
extern "C" int64_t drm_external_torques_scratch_floats_aligned(const drm_walk *w, int64_t B) { return drm_external_torques_scratch_floats(w, B); }
extern "C" int64_t drm_link_power_dq_scratch_floats(const drm_walk *w, int64_t B) { return links_scratch(w, B, w ? power_dq_state_floats(w) : 0); }
extern "C" int64_t drm_link_power_dq_scratch_floats_aligned(const drm_walk *w, int64_t B) { return drm_link_power_dq_scratch_floats(w, B); }

extern "C" int drm_link_motion(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t n_targets,
                               int32_t flags, float *pos, float *lin_vel, float *ang_vel, float *lin_acc, float *ang_acc, float *scratch,
                               void *stream) {
    int rc = args_link_motion(w, q, B, n_targets, pos, lin_vel, ang_vel, lin_acc, ang_acc);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs, T = n_targets;
    const int mode = (lin_acc || ang_acc) ? 2 : (lin_vel || ang_vel) ? 1 : 0;
    int64_t lo = 0;
    if (links_fused(w, T, B, flags, aligned16(q, qd, qdd, pos, lin_vel, ang_vel, lin_acc, ang_acc))) {
        const int n_tiles = (int)(B / WAVE);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, qdd, n_tiles, pos, lin_vel, ang_vel, lin_acc,
                               ang_acc);
        };
        if (mode == 2) go(link_motion_arm_kernel<8, 7, 8, 2>);
        else if (mode == 1) go(link_motion_arm_kernel<8, 7, 8, 1>);
        else go(link_motion_arm_kernel<8, 7, 8, 0>);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general kernel over rows [lo, B)
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, motion_state_floats(w), LINKS_LDS_BYTES);
    auto off = [&](float *p) { return p ? p + lo * T * 3 : nullptr; };
    auto in = [&](const float *p) { return p ? p + lo * n : nullptr; };
    auto go = [&](auto in_lds, auto in_scratch) {
        return rows_launch(in_lds, in_scratch, plan, scratch, "drm_link_motion_scratch_floats", s, w->ops_f, w->ops_i, (int)w->capacity,
                           (int)w->n_ops, (int)w->n_slots, n, T, in(q), in(qd), in(qdd), rows, plan.tiles, off(pos), off(lin_vel),
                           off(ang_vel), off(lin_acc), off(ang_acc));
    };
    if (mode == 2) return go(link_motion_rows_kernel<true, 2>, link_motion_rows_kernel<false, 2>);
    if (mode == 1) return go(link_motion_rows_kernel<true, 1>, link_motion_rows_kernel<false, 1>);
    return go(link_motion_rows_kernel<true, 0>, link_motion_rows_kernel<false, 0>);
}

extern "C" int drm_external_torques(const drm_walk *w, const float *q, const float *force, const float *torque, int64_t B,
                                    int32_t n_targets, int32_t flags, float *tau, float *scratch, void *stream) {
    int rc = args_external_torques(w, q, force, torque, B, n_targets, tau);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs, T = n_targets;
    int64_t lo = 0;
    if (links_fused(w, T, B, flags, aligned16(q, force, torque, tau))) {
        const int n_tiles = (int)(B / WAVE);
        hipLaunchKernelGGL((link_torques_arm_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, force, torque, n_tiles,
                           tau);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, torques_state_floats(w), LINKS_LDS_BYTES);
    return rows_launch(link_torques_rows_kernel<true>, link_torques_rows_kernel<false>, plan, scratch, "drm_external_torques_scratch_floats",
                       s, w->ops_f, w->ops_i, (int)w->capacity, (int)w->n_ops, (int)w->n_slots, n, T, q + lo * n,
                       force ? force + lo * T * 3 : nullptr, torque ? torque + lo * T * 3 : nullptr, rows, plan.tiles, tau + lo * n);
}

extern "C" int drm_link_power_dq(const drm_walk *w, const float *q, const float *qd, const float *force, const float *torque, int64_t B,
                                 int32_t n_targets, int32_t flags, float *dq, float *tau, float *scratch, void *stream) {
    int rc = args_link_power_dq(w, q, qd, force, torque, B, n_targets, dq);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs, T = n_targets;
    int64_t lo = 0;
    if (links_fused(w, T, B, flags, aligned16(q, qd, force, torque, dq, tau))) {
        const int n_tiles = (int)(B / WAVE);
        hipLaunchKernelGGL((link_power_dq_arm_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, force, torque,
                           n_tiles, dq, tau);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, power_dq_state_floats(w), LINKS_LDS_BYTES);
    return rows_launch(link_power_dq_rows_kernel<true>, link_power_dq_rows_kernel<false>, plan, scratch, "drm_link_power_dq_scratch_floats", s,
                       w->ops_f, w->ops_i, (int)w->capacity, (int)w->n_ops, (int)w->n_slots, n, T, q + lo * n, qd + lo * n,
                       force ? force + lo * T * 3 : nullptr, torque ? torque + lo * T * 3 : nullptr, rows, plan.tiles, dq + lo * n,
                       tau ? tau + lo * n : nullptr);
}

// drm_whole_body.hip — the centre of mass, its velocity, acceleration and Jacobian, the angular momentum about the base origin and the
// wrench the mount applies to the base link, in one call (include/drm_hip_whole_body.h drm_whole_body).  What a caller otherwise
// composes from all-links motion, a loop over the link masses and inertias and one Jacobian launch PER LINK.
//
//   whole_body_arm_kernel    serial 7-DoF arm chains, full 64-row tiles, 16-byte aligned pointers: one wavefront per tile, one row per
//                            lane, the constant table staged in LDS once, the q / qd / qdd tiles in through LDS in 16-byte loads, ONE
//                            chain_trig; the bodies' momenta and their rates and the one composite of the sweep back (16 floats) stay
//                            in registers (drm_whole_body.hpp whole_body_chain_trig).  Every output tile is assembled in LDS ([64, 3]
//                            is 768 contiguous bytes, com_jac [64, 21]) and leaves whole in 16-byte stores.  Instantiated per level
//                            (positions; + velocities; + accelerations) and with / without the Jacobian.  11 KB of LDS per wavefront.
//   whole_body_rows_kernel   every other walk (trees, hands, prismatic joints, two-op skew-axis links), the ragged tail of an arm
//                            launch, misaligned pointers, DRM_WHOLE_BODY_COMPOSED: one lane per row, loops over the ops
//                            (drm_whole_body.hpp whole_body_tree_walk).  Between the sweeps a row keeps 16 / 22 / 28 floats per op and
//                            4 / 10 / 16 per branch point (by level), placed by drm_rows.hpp (LDS up to WB_LDS_BYTES).
//
// Per row, fused, n = 7: in q, qd, qdd (28 - 84 B); out up to 6 x 12 + 84 = 156 B.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_whole_body.hpp"
#include "drm_rows.hpp"
#include "drm_args_whole_body.hpp"

namespace drm {

constexpr int WB_LDS_BYTES = 32 * 1024; // per-row state of the general kernel in LDS up to here (five blocks per CU)

static inline int wb_state_floats(const drm_walk *w, int level) {
    return wb_rec_floats(level) * w->n_ops + wb_slot_floats(level) * w->n_slots;
}

struct WbBaseArg {
    float v[4];
};

// LEVEL: drm_whole_body.hpp's; JAC: the Jacobian's columns are formed.  Outputs whose pointer is NULL are not stored (wave-uniform).
template <int CAP, int NJ, int LINKS, int LEVEL, bool JAC>
__global__ void __launch_bounds__(WAVE)
    whole_body_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd,
                          const float *__restrict__ qdd, int n_tiles, int gravity, WbBaseArg base, float *__restrict__ com,
                          float *__restrict__ com_vel, float *__restrict__ com_acc, float *__restrict__ com_jac, float *__restrict__ ang_mom,
                          float *__restrict__ force, float *__restrict__ moment) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, Q_FLOATS = round4(WAVE * NJ), J_FLOATS = round4(WAVE * 3 * NJ), V_FLOATS = round4(WAVE * 3);
    static_assert(3 * Q_FLOATS <= J_FLOATS, "the Jacobian's tile reuses the input tiles' buffer");
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + J_FLOATS + 6 * V_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lj = smem + C_FLOATS, *lv = lj + J_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    tile_load<NJ>(q + b0 * NJ, WAVE, NJ, 0u, lj, lane, true);
    if (LEVEL >= 1 && qd) tile_load<NJ>(qd + b0 * NJ, WAVE, NJ, 0u, lj + Q_FLOATS, lane, true);
    if (LEVEL >= 2 && qdd) tile_load<NJ>(qdd + b0 * NJ, WAVE, NJ, 0u, lj + 2 * Q_FLOATS, lane, true);
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    float qv[NJ], qdv[NJ], qddv[NJ];
#pragma unroll
    for (int d = 0; d < NJ; ++d) {
        qv[d] = lj[lane * NJ + d];
        qdv[d] = (LEVEL >= 1 && qd) ? lj[Q_FLOATS + lane * NJ + d] : 0.0f;
        qddv[d] = (LEVEL >= 2 && qdd) ? lj[2 * Q_FLOATS + lane * NJ + d] : 0.0f;
    }
    wave_lds_sync(); // (the Jacobian's tile below reuses lj)

    // a row that cannot be used walks the chain at rest at q = 0 and gets NaN outputs
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || wb_bad_input(qv[d], qdv[d], qddv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; qddv[d] = bad ? 0.0f : qddv[d]; }
    const float nan = __builtin_nanf("");

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    float jac[JAC ? 3 * NJ : 1];
    WbRoot root;
    whole_body_chain_trig<LINKS, NJ, LEVEL, JAC>(row, cs, sn, qdv, qddv, jac, base.v[0], root);
    WbOut o;
    wb_finish<LEVEL>(root, base.v, gravity != 0, o);

    float *const outs[6] = {com, LEVEL >= 1 ? com_vel : nullptr, LEVEL >= 2 ? com_acc : nullptr, LEVEL >= 1 ? ang_mom : nullptr, force, moment};
    const float *const vals[6] = {o.com, o.com_vel, o.com_acc, o.ang_mom, o.force, o.moment};
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        if (!outs[j]) continue;
#pragma unroll
        for (int i = 0; i < 3; ++i) lv[j * V_FLOATS + lane * 3 + i] = bad ? nan : vals[j][i];
    }
    if constexpr (JAC) {
        if (com_jac) {
#pragma unroll
            for (int i = 0; i < 3 * NJ; ++i) lj[lane * 3 * NJ + i] = bad ? nan : jac[i];
        }
    }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if (outs[j]) tile_store<3>(outs[j] + b0 * 3, WAVE, 3, 0u, lv + j * V_FLOATS, lane, true);
    if constexpr (JAC) {
        if (com_jac) tile_store<3 * NJ>(com_jac + b0 * 3 * NJ, WAVE, 3 * NJ, 0u, lj, lane, true);
    }
}

// The general kernel.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles.  The lanes' records and parked
// composites: drm_rows.hpp rows_state.
template <bool IN_LDS, int LEVEL>
__global__ void __launch_bounds__(WAVE)
    whole_body_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int p_end, int n_slots, int n,
                           const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ qdd, int64_t B, int64_t n_tiles,
                           int gravity, WbBaseArg base, float *__restrict__ com, float *__restrict__ com_vel, float *__restrict__ com_acc,
                           float *__restrict__ com_jac, float *__restrict__ ang_mom, float *__restrict__ force, float *__restrict__ moment,
                           float *__restrict__ scratch, int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<wb_rec_floats(LEVEL), WAVE> recs = {state};
    const Records<wb_slot_floats(LEVEL), WAVE> slots = {state + wb_rec_floats(LEVEL) * n_ops * WAVE};
    const RowsCtl ctl(ops_i, cap);
    const float nan = __builtin_nanf("");
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue; // (a lane shares nothing with its neighbours: no barrier below)
        const float *qr = q + r * n, *qdr = (LEVEL >= 1 && qd) ? qd + r * n : nullptr, *qddr = (LEVEL >= 2 && qdd) ? qdd + r * n : nullptr;
        float *jr = com_jac ? com_jac + r * 3 * n : nullptr;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || wb_bad_input(qr[d], qdr ? qdr[d] : 0.0f, qddr ? qddr[d] : 0.0f);
        WbRoot root;
        whole_body_tree_walk<LEVEL>(
            n_ops, p_end, n_slots, ctl, row,
            [&](int d, float &a, float &v, float &acc) {
                a = bad ? 0.0f : qr[d];
                v = (bad || !qdr) ? 0.0f : qdr[d];
                acc = (bad || !qddr) ? 0.0f : qddr[d];
            },
            [&](int k, const float *x) { recs.put(k, x); }, [&](int k, float *x) { recs.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int j, const float *col) {
                if (j >= n || !jr) return;
#pragma unroll
                for (int i = 0; i < 3; ++i) jr[i * n + j] = bad ? nan : col[i];
            },
            base.v[0], root);
        WbOut o;
        wb_finish<LEVEL>(root, base.v, gravity != 0, o);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (com) com[r * 3 + i] = bad ? nan : o.com[i];
            if (LEVEL >= 1 && com_vel) com_vel[r * 3 + i] = bad ? nan : o.com_vel[i];
            if (LEVEL >= 2 && com_acc) com_acc[r * 3 + i] = bad ? nan : o.com_acc[i];
            if (LEVEL >= 1 && ang_mom) ang_mom[r * 3 + i] = bad ? nan : o.ang_mom[i];
            if (force) force[r * 3 + i] = bad ? nan : o.force[i];
            if (moment) moment[r * 3 + i] = bad ? nan : o.moment[i];
        }
    }
}

template <int LINKS, int LEVEL, class... A>
static void launch_whole_body_arm(bool jac, int n_tiles, hipStream_t s, A... args) {
    if (jac) hipLaunchKernelGGL((whole_body_arm_kernel<8, 7, LINKS, LEVEL, true>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, args...);
    else hipLaunchKernelGGL((whole_body_arm_kernel<8, 7, LINKS, LEVEL, false>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, args...);
}
template <int LINKS, class... A>
static void launch_whole_body_arm_level(int level, bool jac, int n_tiles, hipStream_t s, A... args) {
    if (level == 2) launch_whole_body_arm<LINKS, 2>(jac, n_tiles, s, args...);
    else if (level == 1) launch_whole_body_arm<LINKS, 1>(jac, n_tiles, s, args...);
    else launch_whole_body_arm<LINKS, 0>(jac, n_tiles, s, args...);
}

} // namespace drm

using namespace drm;

// (the query does not know the call's level: it sizes the scratch for the largest records)
static int64_t whole_body_scratch(const drm_walk *w, int64_t B, bool aligned) {
    return check_sweep_walk(w) ? 0 : rows_scratch_floats(w, B, aligned, wb_state_floats(w, 2), WB_LDS_BYTES);
}
extern "C" int64_t drm_whole_body_scratch_floats(const drm_walk *w, int64_t B) { return whole_body_scratch(w, B, false); }
extern "C" int64_t drm_whole_body_scratch_floats_aligned(const drm_walk *w, int64_t B) { return whole_body_scratch(w, B, true); }

extern "C" int drm_whole_body(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                              const drm_base_share *base, float *com, float *com_vel, float *com_acc, float *com_jac, float *ang_mom,
                              float *force, float *moment, float *scratch, void *stream) {
    WholeBodyBase hb;
    int rc = args_whole_body(w, q, qd, B, base, com, com_vel, com_acc, com_jac, ang_mom, force, moment, hb);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs;
    const int level = whole_body_level(qd, qdd, com_vel, com_acc, ang_mom, force, moment);
    const int gravity = (flags & DRM_RNEA_GRAVITY) ? 1 : 0;
    WbBaseArg ba;
    for (int i = 0; i < 4; ++i) ba.v[i] = hb.v[i];
    int64_t lo = 0;
    const bool al = aligned16(q, qd, qdd, com, com_vel, com_acc) && aligned16(com_jac, ang_mom, force, moment);
    if (!(flags & DRM_WHOLE_BODY_COMPOSED) && rows_fused(w, B, al)) {
        const int n_tiles = (int)(B / WAVE);
        if (arm_links(w) == 7)
            launch_whole_body_arm_level<7>(level, com_jac != nullptr, n_tiles, s, w->ops_f, q, qd, qdd, n_tiles, gravity, ba, com, com_vel, com_acc,
                                           com_jac, ang_mom, force, moment);
        else
            launch_whole_body_arm_level<8>(level, com_jac != nullptr, n_tiles, s, w->ops_f, q, qd, qdd, n_tiles, gravity, ba, com, com_vel, com_acc,
                                           com_jac, ang_mom, force, moment);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general kernel over rows [lo, B)
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, wb_state_floats(w, level), WB_LDS_BYTES);
    const int p_end = w->n_segments > 1 ? w->prefix_end : 0;
    auto at = [&](const float *x, int64_t width) -> const float * { return x ? x + lo * width : nullptr; };
    auto out = [&](float *x, int64_t width) -> float * { return x ? x + lo * width : nullptr; };
    const char *query = "drm_whole_body_scratch_floats";
#define DRM_WB_ROWS(L)                                                                                                                      \
    rows_launch(whole_body_rows_kernel<true, L>, whole_body_rows_kernel<false, L>, plan, scratch, query, s, w->ops_f, w->ops_i,             \
                (int)w->capacity, (int)w->n_ops, p_end, (int)w->n_slots, n, at(q, n), at(qd, n), at(qdd, n), rows, plan.tiles, gravity, ba, \
                out(com, 3), out(com_vel, 3), out(com_acc, 3), out(com_jac, 3 * (int64_t)n), out(ang_mom, 3), out(force, 3), out(moment, 3))
    if (level == 2) return DRM_WB_ROWS(2);
    if (level == 1) return DRM_WB_ROWS(1);
    return DRM_WB_ROWS(0);
#undef DRM_WB_ROWS
}

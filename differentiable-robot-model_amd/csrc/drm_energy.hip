// drm_energy.hip — the kinetic energy T(q, qd), the potential energy V(q), the generalised momentum p = H qd and the gradients dT/dq
// and dV/dq = g(q) in one call (include/drm_hip.h drm_energy).  What a caller otherwise composes from drm_lagrangian_dynamics (420 B
// per row, to throw H and C away again after two small products), all-links forward kinematics and a loop over the link masses.
//
//   energy_arm_kernel    serial 7-DoF arm chains, full 64-row tiles, 16-byte aligned pointers: one wavefront per tile, one row per lane,
//                        the constant table staged in LDS once, ONE chain_trig; the links' velocities and momenta and the one composite of the
//                        sweep back (momentum, mass, first moment: ten floats) stay in registers (drm_energy.hpp energy_chain_trig).
//                        T and V leave as one float per lane; the [64, 7] tiles of p, dT/dq and g are assembled side by side in LDS
//                        (28 B per row is not 16-byte aligned on its own) and leave whole in 16-byte stores.  With p, dT/dq and g all
//                        NULL (the energies alone) another instantiation makes no sweep back.  6.3 KB of LDS per wavefront.
//   energy_rows_kernel   every other walk (trees, hands, prismatic joints, two-op skew-axis links, fixed ops kept for learnable links),
//                        the ragged tail of an arm launch, misaligned pointers, DRM_ENERGY_COMPOSED: one lane per row, loops over the
//                        ops (drm_energy.hpp energy_tree_walk), ALL segments of the walk on the one wavefront.  Between the sweeps a
//                        row keeps 14 floats per op and 10 per branch point, placed by drm_rows.hpp (LDS up to ENERGY_LDS_BYTES).
//
// Per row, fused, n = 7: in q, qd (56 B); out 4 (1 + 1 + 7 + 7 + 7) B = 92 B.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_energy.hpp"
#include "drm_rows.hpp"
#include "drm_args.hpp"

namespace drm {

constexpr int ENERGY_LDS_BYTES = 32 * 1024; // per-row state of the general kernel in LDS up to here (five blocks per CU)

static inline int energy_state_floats(const drm_walk *w) { return ENERGY_REC_FLOATS * w->n_ops + ENERGY_SLOT_FLOATS * w->n_slots; }

// BACK: the sweep back is made and p, dT/dq, g are staged (stored where their pointer is not NULL: wave-uniform); otherwise T, V alone
template <int CAP, int NJ, int LINKS, bool BACK>
__global__ void __launch_bounds__(WAVE)
    energy_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd, int n_tiles,
                      float *__restrict__ T, float *__restrict__ V, float *__restrict__ p, float *__restrict__ dT, float *__restrict__ g) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * NJ);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + (BACK ? 3 * T_FLOATS : 0)];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem;
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

    // a row that cannot be used walks the chain at rest at q = 0 and gets NaN outputs: its angles would send the whole wavefront's
    // sines and cosines down chain_trig's slow path and change other rows' bits
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || lag_bad_input(qv[d], qdv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; }
    const float nan = __builtin_nanf("");

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    float Tv, Vv;
    if constexpr (BACK) {
        float *lp = smem + C_FLOATS + lane * NJ, *ld = lp + T_FLOATS, *lg = ld + T_FLOATS;
        energy_chain_trig<LINKS, NJ, true>(row, cs, sn, qdv, Tv, Vv, [&](int j, float pj, float dj, float gj) {
            lp[j] = bad ? nan : pj;
            ld[j] = bad ? nan : dj;
            lg[j] = bad ? nan : gj;
        });
    } else {
        energy_chain_trig<LINKS, NJ, false>(row, cs, sn, qdv, Tv, Vv, [](int, float, float, float) {});
    }
    if (T) T[b0 + lane] = bad ? nan : Tv;
    if (V) V[b0 + lane] = bad ? nan : Vv;
    if constexpr (BACK) {
        const float *lt = smem + C_FLOATS;
        wave_lds_sync();
        if (p) tile_store<NJ>(p + b0 * NJ, WAVE, NJ, 0u, lt, lane, true);
        if (dT) tile_store<NJ>(dT + b0 * NJ, WAVE, NJ, 0u, lt + T_FLOATS, lane, true);
        if (g) tile_store<NJ>(g + b0 * NJ, WAVE, NJ, 0u, lt + 2 * T_FLOATS, lane, true);
    }
}

// The general kernel.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles.  The lanes' records and parked
// composites: drm_rows.hpp rows_state.
template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
    energy_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int p_end, int n_slots, int n,
                       const float *__restrict__ q, const float *__restrict__ qd, int64_t B, int64_t n_tiles, float *__restrict__ T,
                       float *__restrict__ V, float *__restrict__ p, float *__restrict__ dT, float *__restrict__ g,
                       float *__restrict__ scratch, int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<ENERGY_REC_FLOATS, WAVE> recs = {state};
    const Records<ENERGY_SLOT_FLOATS, WAVE> slots = {state + ENERGY_REC_FLOATS * n_ops * WAVE};
    const RowsCtl ctl(ops_i, cap);
    const float nan = __builtin_nanf("");
    const bool back = p || dT || g;
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue; // (a lane shares nothing with its neighbours: no barrier below)
        const float *qr = q + r * n, *qdr = qd + r * n;
        float *pr = p ? p + r * n : nullptr, *dr = dT ? dT + r * n : nullptr, *gr = g ? g + r * n : nullptr;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || lag_bad_input(qr[d], qdr[d]);
        energy_tree_walk(
            n_ops, p_end, n_slots, back, ctl, row,
            [&](int d, float &a, float &v) { a = bad ? 0.0f : qr[d]; v = bad ? 0.0f : qdr[d]; },
            [&](int k, const float *x) { recs.put(k, x); }, [&](int k, float *x) { recs.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](float Tv, float Vv) {
                if (T) T[r] = bad ? nan : Tv;
                if (V) V[r] = bad ? nan : Vv;
            },
            [&](int j, float pj, float dj, float gj) {
                if (j >= n) return;
                if (pr) pr[j] = bad ? nan : pj;
                if (dr) dr[j] = bad ? nan : dj;
                if (gr) gr[j] = bad ? nan : gj;
            });
    }
}

template <int LINKS>
static void launch_energy_arm(const drm_walk *w, const float *q, const float *qd, int n_tiles, float *T, float *V, float *p, float *dT,
                              float *g, hipStream_t s) {
    if (p || dT || g)
        hipLaunchKernelGGL((energy_arm_kernel<8, 7, LINKS, true>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, n_tiles, T, V, p,
                           dT, g);
    else
        hipLaunchKernelGGL((energy_arm_kernel<8, 7, LINKS, false>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, n_tiles, T, V,
                           p, dT, g);
}

} // namespace drm

using namespace drm;

static int64_t energy_scratch(const drm_walk *w, int64_t B, bool aligned) {
    return check_sweep_walk(w) ? 0 : rows_scratch_floats(w, B, aligned, energy_state_floats(w), ENERGY_LDS_BYTES);
}
extern "C" int64_t drm_energy_scratch_floats(const drm_walk *w, int64_t B) { return energy_scratch(w, B, false); }
extern "C" int64_t drm_energy_scratch_floats_aligned(const drm_walk *w, int64_t B) { return energy_scratch(w, B, true); }

extern "C" int drm_energy(const drm_walk *w, const float *q, const float *qd, int64_t B, int32_t flags, float *T, float *V, float *p,
                          float *dT, float *g, float *scratch, void *stream) {
    int rc = args_sweep_q_qd(w, q, qd, B, T || V || p || dT || g);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs;
    int64_t lo = 0;
    // (T and V are stored one float per lane: any alignment serves them)
    if (!(flags & DRM_ENERGY_COMPOSED) && rows_fused(w, B, aligned16(q, qd, p, dT, g))) {
        const int n_tiles = (int)(B / WAVE);
        if (arm_links(w) == 7) launch_energy_arm<7>(w, q, qd, n_tiles, T, V, p, dT, g, s);
        else launch_energy_arm<8>(w, q, qd, n_tiles, T, V, p, dT, g, s);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general kernel over rows [lo, B)
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, energy_state_floats(w), ENERGY_LDS_BYTES);
    const int p_end = w->n_segments > 1 ? w->prefix_end : 0;
    const float *qs = q + lo * n, *qds = qd + lo * n;
    float *Ts = T ? T + lo : nullptr, *Vs = V ? V + lo : nullptr;
    float *ps = p ? p + lo * n : nullptr, *ds = dT ? dT + lo * n : nullptr, *gs = g ? g + lo * n : nullptr;
    return rows_launch(energy_rows_kernel<true>, energy_rows_kernel<false>, plan, scratch, "drm_energy_scratch_floats", s, w->ops_f, w->ops_i,
                       (int)w->capacity, (int)w->n_ops, p_end, (int)w->n_slots, n, qs, qds, rows, plan.tiles, Ts, Vs, ps, ds, gs);
}

// drm_lagrangian.hip — H(q), the Christoffel-consistent Coriolis matrix C(q, qd) and g(q) of  H qdd + C qd + g = tau  in one call
// (include/drm_hip.h drm_lagrangian_dynamics).  What a caller otherwise gets from dH/dq by autograd — one backward pass through the
// inertia matrix per entry of its upper triangle, each n launches of the RNEA backward kernel — an einsum and one inverse-dynamics call.
//
//   lagrangian_arm_kernel    serial 7-DoF arm chains, full 64-row tiles, 16-byte aligned pointers: one wavefront per tile, one row per
//                            lane, the constant table staged in LDS once, ONE chain_trig; the links' velocities, the composite of the
//                            chain below a joint and the three wrenches that climb its ancestors stay in registers
//                            (drm_lagrangian.hpp lagrangian_chain_trig).  C lands in the lane's stretch of ONE 64 x 49 tile in LDS
//                            (odd pitch) as it is formed and leaves in 16-byte stores; the triangle of H and g wait in registers
//                            and leave through the same tile after it.  A tile of each output is contiguous and 16-byte aligned.
//                            13.5 KB of LDS per wavefront (three tiles side by side were 27.9 KB: five wavefronts per CU).  With H
//                            and g both NULL (the Coriolis matrix alone) another instantiation forms neither.
//   lagrangian_rows_kernel   every other walk (trees, hands, prismatic joints, two-op skew-axis links, fixed ops kept for learnable
//                            links), the ragged tail of an arm launch, misaligned pointers, DRM_LAGRANGIAN_COMPOSED: one lane per row,
//                            loops over the ops (drm_lagrangian.hpp lagrangian_tree_walk), ALL segments of the walk on the one
//                            wavefront.  Between the sweeps a row keeps twelve floats per op and 22 per branch point, placed by
//                            drm_rows.hpp (LDS up to LAG_LDS_BYTES).  Its rows of H and C are zeroed by hipMemsetAsync
//                            ahead of it and the kernel stores the entries between a joint and its ancestors only: entries between
//                            branches are exact zeros (the regressor measured the memset against in-kernel zeros: up to 2x faster).
//
// Per row, fused, n = 7: in q, qd (56 B); out 4 (49 + 49 + 7) B = 420 B.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_lagrangian.hpp"
#include "drm_rows.hpp"
#include "drm_args.hpp"

namespace drm {

constexpr int LAG_LDS_BYTES = 32 * 1024; // per-row state of the general kernel in LDS up to here (five blocks per CU)

static inline int lagrangian_state_floats(const drm_walk *w) { return LAG_REC_FLOATS * w->n_ops + LAG_SLOT_FLOATS * w->n_slots; }

// ALL: H and g are formed and staged too (stored where their pointer is not NULL: wave-uniform); otherwise C alone
template <int CAP, int NJ, int LINKS, bool ALL>
__global__ void __launch_bounds__(WAVE)
    lagrangian_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd, int n_tiles,
                          float *__restrict__ H, float *__restrict__ C, float *__restrict__ g) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int NN = NJ * NJ;
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * NN);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + T_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lt = smem + C_FLOATS;
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
    // C goes into the lane's stretch of the tile as it is formed; the triangle of H and g wait in registers for the tile to be free
    float *mine = lt + lane * NN;
    float Ht[ALL ? NJ * (NJ + 1) / 2 : 1], gv[ALL ? NJ : 1];
    lagrangian_chain_trig<LINKS, NJ, ALL, ALL>(
        row, cs, sn, qdv,
        [&](int i, int j, float v) {
            if (i >= j) Ht[tri_index(i, j)] = v;
        },
        [&](int i, int j, float v) { mine[i * NJ + j] = bad ? nan : v; }, [&](int j, float v) { gv[j] = v; });
    wave_lds_sync();
    if (C) tile_store<NN>(C + b0 * NN, WAVE, NN, 0u, lt, lane, true);
    if constexpr (ALL) {
        if (H) {
            wave_lds_sync();
#pragma unroll
            for (int i = 0; i < NJ; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    const float v = bad ? nan : Ht[tri_index(i, j)];
                    mine[i * NJ + j] = v;
                    mine[j * NJ + i] = v;
                }
            wave_lds_sync();
            tile_store<NN>(H + b0 * NN, WAVE, NN, 0u, lt, lane, true);
        }
        if (g) {
            wave_lds_sync();
#pragma unroll
            for (int d = 0; d < NJ; ++d) lt[lane * NJ + d] = bad ? nan : gv[d];
            wave_lds_sync();
            tile_store<NJ>(g + b0 * NJ, WAVE, NJ, 0u, lt, lane, true);
        }
    }
}

// The general kernel.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles.  The lanes' records and parked
// composites: drm_rows.hpp rows_state.  H and C arrive zeroed.
template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
    lagrangian_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int p_end, int n_slots,
                           int n, const float *__restrict__ q, const float *__restrict__ qd, int64_t B, int64_t n_tiles,
                           float *__restrict__ H, float *__restrict__ C, float *__restrict__ g, float *__restrict__ scratch,
                           int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<LAG_REC_FLOATS, WAVE> recs = {state};
    const Records<LAG_SLOT_FLOATS, WAVE> slots = {state + LAG_REC_FLOATS * n_ops * WAVE};
    const RowsCtl ctl(ops_i, cap);
    const float nan = __builtin_nanf("");
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue; // (a lane shares nothing with its neighbours: no barrier below)
        const float *qr = q + r * n, *qdr = qd + r * n;
        float *Hr = H ? H + r * n * n : nullptr, *Cr = C ? C + r * n * n : nullptr, *gr = g ? g + r * n : nullptr;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || lag_bad_input(qr[d], qdr[d]);
        lagrangian_tree_walk(
            n_ops, p_end, n_slots, ctl, row,
            [&](int d, float &a, float &v) { a = bad ? 0.0f : qr[d]; v = bad ? 0.0f : qdr[d]; },
            [&](int k, const float *x) { recs.put(k, x); }, [&](int k, float *x) { recs.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int i, int j, float v) {
                if (Hr && i < n && j < n) Hr[i * n + j] = bad ? nan : v;
            },
            [&](int i, int j, float v) {
                if (Cr && i < n && j < n) Cr[i * n + j] = bad ? nan : v;
            },
            [&](int j, float v) {
                if (gr && j < n) gr[j] = bad ? nan : v;
            });
    }
}

template <int LINKS>
static void launch_lagrangian_arm(const drm_walk *w, const float *q, const float *qd, int n_tiles, float *H, float *C, float *g,
                                  hipStream_t s) {
    if (H || g)
        hipLaunchKernelGGL((lagrangian_arm_kernel<8, 7, LINKS, true>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, n_tiles, H,
                           C, g);
    else
        hipLaunchKernelGGL((lagrangian_arm_kernel<8, 7, LINKS, false>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, n_tiles, H,
                           C, g);
}

} // namespace drm

using namespace drm;

static int64_t lagrangian_scratch(const drm_walk *w, int64_t B, bool aligned) {
    return check_sweep_walk(w) ? 0 : rows_scratch_floats(w, B, aligned, lagrangian_state_floats(w), LAG_LDS_BYTES);
}
extern "C" int64_t drm_lagrangian_dynamics_scratch_floats(const drm_walk *w, int64_t B) { return lagrangian_scratch(w, B, false); }
extern "C" int64_t drm_lagrangian_dynamics_scratch_floats_aligned(const drm_walk *w, int64_t B) { return lagrangian_scratch(w, B, true); }

extern "C" int drm_lagrangian_dynamics(const drm_walk *w, const float *q, const float *qd, int64_t B, int32_t flags, float *H, float *C,
                                       float *g, float *scratch, void *stream) {
    int rc = args_sweep_q_qd(w, q, qd, B, H || C || g);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs;
    int64_t lo = 0;
    if (!(flags & DRM_LAGRANGIAN_COMPOSED) && rows_fused(w, B, aligned16(q, qd, H, C, g))) {
        const int n_tiles = (int)(B / WAVE);
        if (arm_links(w) == 7) launch_lagrangian_arm<7>(w, q, qd, n_tiles, H, C, g, s);
        else launch_lagrangian_arm<8>(w, q, qd, n_tiles, H, C, g, s);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general kernel over rows [lo, B)
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, lagrangian_state_floats(w), LAG_LDS_BYTES);
    const int p_end = w->n_segments > 1 ? w->prefix_end : 0;
    const float *qs = q + lo * n, *qds = qd + lo * n;
    float *Hs = H ? H + lo * n * n : nullptr, *Cs = C ? C + lo * n * n : nullptr, *gs = g ? g + lo * n : nullptr;
    rc = rows_zero({Hs, Cs}, (size_t)rows * n * n, s);
    if (rc) return rc;
    return rows_launch(lagrangian_rows_kernel<true>, lagrangian_rows_kernel<false>, plan, scratch, "drm_lagrangian_dynamics_scratch_floats", s,
                       w->ops_f, w->ops_i, (int)w->capacity, (int)w->n_ops, p_end, (int)w->n_slots, n, qs, qds, rows, plan.tiles, Hs, Cs, gs);
}

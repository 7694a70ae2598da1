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
//                                  Between the sweeps a row keeps 15 floats per op and 28 per branch point, in LDS where 64 rows of them
//                                  fit IDD_LDS_BYTES, else in the caller's scratch (a persistent grid of at most IDD_SCRATCH_BLOCKS
//                                  blocks, each with its own slice).  Its rows of the three matrices are zeroed by hipMemsetAsync ahead
//                                  of it and the kernel stores the entries between a joint and its ancestors only: entries between
//                                  branches are exact zeros.
//
// Per row, fused, n = 7: in q, qd, qdd (84 B); out 4 (3 * 49 + 7) B = 616 B.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_idd.hpp"

namespace drm {

constexpr int IDD_LDS_BYTES = 32 * 1024;   // per-row state of the general kernel in LDS up to here (five blocks per CU)
constexpr int IDD_SCRATCH_BLOCKS = 2048;   // ... beyond: blocks of the persistent grid, each with a slice of the scratch

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

#if DRM_IDD_BLOCK
// The variant that was measured against the kernel above and left out of the shipped library (make EXTRA=-DDRM_IDD_BLOCK=1;
// profiles/id_derivatives_bench.txt): a BLOCK of four wavefronts per tile, every wavefront one row per lane of the SAME 64 rows.  Each
// repeats the motions and the chain of composites and forms the wrenches and the climbs of its own joints only ({6}, {5, 0}, {4, 1},
// {3, 2}: seven wrench moves each); the four outputs are assembled in four tiles of LDS (40.4 KB per block) and stored by all 256 threads.
template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(4 * WAVE)
    rnea_derivatives_arm_block_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd,
                                      const float *__restrict__ qdd, int n_tiles, int flags, float *__restrict__ tau,
                                      float *__restrict__ dq, float *__restrict__ dqd, float *__restrict__ H) {
    static_assert(NJ == 7, "the joints are shared out by hand");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int NN = NJ * NJ;
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, T_FLOATS = round4(WAVE * NN), V_FLOATS = round4(WAVE * NJ);
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 3 * T_FLOATS + V_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return; // (the whole block)
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *lc = smem, *t0 = smem + C_FLOATS, *t1 = t0 + T_FLOATS, *t2 = t1 + T_FLOATS, *tt = t2 + T_FLOATS;
    const int64_t b0 = (int64_t)tile * WAVE;
    const bool gravity = flags & DRM_RNEA_GRAVITY, damping = flags & DRM_RNEA_DAMPING;
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
    if (wave == 0) reinterpret_cast<float4 *>(lc)[lane] = reinterpret_cast<const float4 *>(ops_f)[lane];
    __syncthreads();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || idd_bad_input(qv[d], qdv[d], qddv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; qddv[d] = bad ? 0.0f : qddv[d]; }
    const float nan = __builtin_nanf("");
    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    float *m0 = t0 + lane * NN, *m1 = t1 + lane * NN, *m2 = t2 + lane * NN, *mt = tt + lane * NJ;
    idd_chain_trig<LINKS, NJ>(
        row, gravity ? 9.81f : 0.0f, damping, cs, sn, qdv, qddv,
        [&](int k) { return k == 6 ? wave == 0 : (k == 5 || k == 0) ? wave == 1 : (k == 4 || k == 1) ? wave == 2 : wave == 3; },
        [&](int which, int i, int j, float v) { (which == IDD_DQ ? m0 : which == IDD_DQD ? m1 : m2)[i * NJ + j] = bad ? nan : v; },
        [&](int j, float v) { mt[j] = bad ? nan : v; });
    __syncthreads();
    if (dq) block_tile_store(dq + b0 * NN, WAVE, NN, 0u, t0, true);
    if (dqd) block_tile_store(dqd + b0 * NN, WAVE, NN, 0u, t1, true);
    if (H) block_tile_store(H + b0 * NN, WAVE, NN, 0u, t2, true);
    if (tau) block_tile_store(tau + b0 * NJ, WAVE, NJ, 0u, tt, true);
}
#endif

// The general kernel.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles.  state: the lanes' records and
// parked composites, [float][64 lanes] — LDS (IN_LDS) or the block's slice of the scratch.  The matrices arrive zeroed.
struct IddCtl {
    const int32_t *w0, *w1;
    __device__ void raw(int k, int &a, int &b) const { a = w0[k]; b = w1[k]; }
    __device__ int uniform(int r) const { return __builtin_amdgcn_readfirstlane(r); }
};

template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
    rnea_derivatives_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int p_end,
                                 int n_slots, int n, const float *__restrict__ q, const float *__restrict__ qd,
                                 const float *__restrict__ qdd, int64_t B, int64_t n_tiles, int flags, float *__restrict__ tau,
                                 float *__restrict__ dq, float *__restrict__ dqd, float *__restrict__ H, float *__restrict__ scratch,
                                 int state_floats) {
    extern __shared__ __attribute__((aligned(16))) float idd_rows_lds[];
    const unsigned lane = threadIdx.x & 63u;
    float *state = (IN_LDS ? idd_rows_lds : scratch + (int64_t)blockIdx.x * state_floats * WAVE) + lane;
    float *recs = state, *slots = state + IDD_REC_FLOATS * n_ops * WAVE;
    const IddCtl ctl = {ops_i + DRM_OPI_W0 * cap, ops_i + DRM_OPI_W1 * cap};
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
            [&](int k, const float *x) {
#pragma unroll
                for (int i = 0; i < IDD_REC_FLOATS; ++i) recs[(IDD_REC_FLOATS * k + i) * WAVE] = x[i];
            },
            [&](int k, float *x) {
#pragma unroll
                for (int i = 0; i < IDD_REC_FLOATS; ++i) x[i] = recs[(IDD_REC_FLOATS * k + i) * WAVE];
            },
            [&](int s, const float *x) {
#pragma unroll
                for (int i = 0; i < IDD_SLOT_FLOATS; ++i) slots[(IDD_SLOT_FLOATS * s + i) * WAVE] = x[i];
            },
            [&](int s, float *x) {
#pragma unroll
                for (int i = 0; i < IDD_SLOT_FLOATS; ++i) x[i] = slots[(IDD_SLOT_FLOATS * s + i) * WAVE];
            },
            [&](int which, int i, int j, float v) {
                float *M = which == IDD_DQ ? Mr[0] : which == IDD_DQD ? Mr[1] : Mr[2];
                if (M && i >= 0 && j >= 0 && i < n && j < n) M[i * n + j] = bad ? nan : v;
            },
            [&](int j, float v) {
                if (tr && j >= 0 && j < n) tr[j] = bad ? nan : v;
            });
    }
}

// the fused kernel takes the full tiles of what drm_lagrangian_dynamics' fused kernel takes
static bool idd_fused(const drm_walk *w, int64_t B, bool aligned) {
    return arm7_walk(w) && aligned && table_aligned(w) && full_tiles_fit(B);
}

static int idd_check_walk(const drm_walk *w) {
    int rc = check_walk(w);
    if (rc) return rc;
    if (w->n_ops < 1) return fail(DRM_ERR_INVALID, "the walk has no ops");
    return DRM_OK;
}

// scratch of the general kernel over `rows` rows
static int64_t idd_rows_scratch(const drm_walk *w, int64_t rows) {
    const int64_t state = idd_state_floats(w);
    if (rows <= 0 || state * WAVE * (int64_t)sizeof(float) <= IDD_LDS_BYTES) return 0;
    const int64_t tiles = (rows + WAVE - 1) / WAVE;
    return (tiles < IDD_SCRATCH_BLOCKS ? tiles : IDD_SCRATCH_BLOCKS) * state * WAVE;
}

} // namespace drm

using namespace drm;

static int64_t idd_scratch_floats_impl(const drm_walk *w, int64_t B, bool aligned) {
    if (idd_check_walk(w) || B <= 0) return 0;
    const int64_t lo = idd_fused(w, B, aligned) ? B / WAVE * WAVE : 0;
    return idd_rows_scratch(w, B - lo);
}
extern "C" int64_t drm_rnea_derivatives_scratch_floats(const drm_walk *w, int64_t B) { return idd_scratch_floats_impl(w, B, false); }
extern "C" int64_t drm_rnea_derivatives_scratch_floats_aligned(const drm_walk *w, int64_t B) { return idd_scratch_floats_impl(w, B, true); }

extern "C" int drm_rnea_derivatives(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                                    float *tau, float *dq, float *dqd, float *H, float *scratch, void *stream) {
    int rc = idd_check_walk(w);
    if (rc) return rc;
    if (!q || !qd || !qdd) return fail(DRM_ERR_INVALID, "q / qd / qdd must not be NULL");
    if (!tau && !dq && !dqd && !H) return fail(DRM_ERR_INVALID, "every output is NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs;
    const int fl = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    int64_t lo = 0;
    if (!(flags & DRM_IDD_COMPOSED) && idd_fused(w, B, aligned16(q, qd, qdd, tau, dq, dqd, H))) {
        const int n_tiles = (int)(B / WAVE);
#if DRM_IDD_BLOCK
        if (arm_links(w) == 7)
            hipLaunchKernelGGL((rnea_derivatives_arm_block_kernel<8, 7, 7>), dim3((unsigned)n_tiles), dim3(4 * WAVE), 0, s, w->ops_f, q, qd, qdd,
                               n_tiles, fl, tau, dq, dqd, H);
        else
            hipLaunchKernelGGL((rnea_derivatives_arm_block_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(4 * WAVE), 0, s, w->ops_f, q, qd, qdd,
                               n_tiles, fl, tau, dq, dqd, H);
#else
        if (arm_links(w) == 7)
            hipLaunchKernelGGL((rnea_derivatives_arm_kernel<8, 7, 7>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, qdd, n_tiles,
                               fl, tau, dq, dqd, H);
        else
            hipLaunchKernelGGL((rnea_derivatives_arm_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, qdd, n_tiles,
                               fl, tau, dq, dqd, H);
#endif
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general kernel over rows [lo, B)
    const int64_t rows = B - lo, tiles = (rows + WAVE - 1) / WAVE;
    const int state = idd_state_floats(w);
    const size_t lds = sizeof(float) * (size_t)state * WAVE;
    const int p_end = w->n_segments > 1 ? w->prefix_end : 0;
    const float *qs = q + lo * n, *qds = qd + lo * n, *qdds = qdd + lo * n;
    float *ts = tau ? tau + lo * n : nullptr, *dqs = dq ? dq + lo * n * n : nullptr, *dqds = dqd ? dqd + lo * n * n : nullptr,
          *Hs = H ? H + lo * n * n : nullptr;
    for (float *M : {dqs, dqds, Hs}) {
        if (!M) continue;
        const hipError_t e = hipMemsetAsync(M, 0, sizeof(float) * (size_t)rows * n * n, s);
        if (e != hipSuccess) return fail(DRM_ERR_LAUNCH, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (lds <= (size_t)IDD_LDS_BYTES) {
        if (!grid_fits(tiles)) return fail(DRM_ERR_UNSUPPORTED, "batch too large");
        hipLaunchKernelGGL((rnea_derivatives_rows_kernel<true>), dim3((unsigned)tiles), dim3(WAVE), lds, s, w->ops_f, w->ops_i,
                           (int)w->capacity, (int)w->n_ops, p_end, (int)w->n_slots, n, qs, qds, qdds, rows, tiles, fl, ts, dqs, dqds, Hs,
                           (float *)nullptr, state);
    } else {
        if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_rnea_derivatives_scratch_floats() floats of scratch");
        const int64_t blocks = tiles < IDD_SCRATCH_BLOCKS ? tiles : IDD_SCRATCH_BLOCKS;
        hipLaunchKernelGGL((rnea_derivatives_rows_kernel<false>), dim3((unsigned)blocks), dim3(WAVE), 0, s, w->ops_f, w->ops_i,
                           (int)w->capacity, (int)w->n_ops, p_end, (int)w->n_slots, n, qs, qds, qdds, rows, tiles, fl, ts, dqs, dqds, Hs,
                           scratch, state);
    }
    return launched();
}

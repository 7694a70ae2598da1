// drm_regressor.hip — the inverse-dynamics regressor in one call (include/drm_hip.h drm_rnea_regressor): Y [B, n, P] with
// tau = Y phi, phi the stacked per-op (m, m c, I_o) of the walk (+ the joint dampings), P = 10 n_ops (+ n).  What a caller otherwise
// gets from 10 n_ops inverse-dynamics calls on unit-parameter copies of the robot.
//
//   regressor_arm_kernel    serial 7-DoF arm chains, full 64-row tiles, 16-byte aligned pointers: one BLOCK of four wavefronts per tile,
//                           one row per lane in each of them, the constant table staged in LDS once.  Every wavefront evaluates
//                           chain_trig and walks the motions of the whole chain (cheap), then forms the blocks of ITS bodies in
//                           registers (drm_regressor.hpp regressor_chain_trig: the body's 6 x 10 matrix carried up the chain) — the
//                           bodies are dealt so that each wavefront carries its matrices over seven joints (nine with a fixed tail
//                           op) — and writes them, with the zeros above a body's own joint, into the tile's image of Y in LDS: 64
//                           rows x n P floats, 123 KB (152 KB with a tail op and the damping columns), one block per CU.  The tile
//                           is contiguous in Y and leaves in 16-byte stores by all 256 lanes, every cache line written whole, once.
//                           (A first version staged one body's 7 x 10 floats per row at a time on a lone wavefront, eight to a CU:
//                           its runs of 40 bytes reached HBM as partial lines from a quarter of a gigabyte of tiles in flight, 1.47 ms
//                           for 2^20 rows; profiles/regressor_bench.txt.)
//   regressor_rows_kernel   every other walk (trees, hands, prismatic joints, fixed ops kept for learnable links), the ragged tail of
//                           an arm launch, misaligned pointers, DRM_REGRESSOR_COMPOSED: one lane per row, a loop over the ops
//                           (drm_regressor.hpp regressor_tree_walk), ALL segments of the walk on the one wavefront.  Between ops a
//                           row keeps cos / sin / value of every joint and the motions of the open branch points: 3 n_ops +
//                           12 n_slots floats, placed by drm_rows.hpp (LDS up to REG_LDS_BYTES).  Its rows of Y are
//                           zeroed by ONE hipMemsetAsync ahead of it and the kernel stores the rows of a body's ancestors only: on a
//                           tree most of Y is structural zeros (Allegro: 4 of 16 joints above a body), and lanes writing them ten
//                           floats at a time took twice as long (573 against 287 us, 65 536 Allegro rows; Fetch 432 against 283).
//
// Per row, fused, n = 7: in q, qd, qdd (84 B); out 4 x 7 x 70 B = 1 960 B.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_regressor.hpp"
#include "drm_rows.hpp"
#include "drm_args.hpp"

namespace drm {

constexpr int REG_LDS_BYTES = 20 * 1024; // per-row state of the general kernel in LDS up to here (eight blocks per CU)
constexpr int REG_ARM_WAVES = 4;         // wavefronts of the fused kernel's block: they share the bodies of a tile

static inline int regressor_state_floats(const drm_walk *w) { return 3 * w->n_ops + 12 * w->n_slots; }

// the wavefront that forms body k's block: pairs (k, LINKS - 1 - k) cost the same number of joint transforms
template <int LINKS>
__host__ __device__ constexpr int regressor_owner(int k) {
    if (LINKS & 1) return k == LINKS - 1 ? 0 : (k < LINKS - 2 - k ? k : LINKS - 2 - k) + 1;
    return k < LINKS - 1 - k ? k : LINKS - 1 - k;
}

template <int NJ, int LINKS>
__global__ void __launch_bounds__(REG_ARM_WAVES *WAVE)
    regressor_arm_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, const float *__restrict__ q,
                         const float *__restrict__ qd, const float *__restrict__ qdd, int n_tiles, int flags, float *__restrict__ Y) {
    constexpr int CAP = 8;
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    static_assert(regressor_owner<LINKS>(0) < REG_ARM_WAVES && regressor_owner<LINKS>(LINKS / 2) < REG_ARM_WAVES &&
                      regressor_owner<LINKS>(LINKS - 1) < REG_ARM_WAVES, "every body has a wavefront");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE;
    extern __shared__ __attribute__((aligned(16))) float reg_arm_lds[]; // [ table ][ the tile of Y: 64 x NJ x P ]
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool gravity = flags & DRM_RNEA_GRAVITY, damping = flags & DRM_RNEA_DAMPING;
    const int P = REG_COLS * LINKS + (damping ? NJ : 0), RP = NJ * P;
    float *lc = reg_arm_lds, *image = reg_arm_lds + C_FLOATS, *mine = image + lane * RP;
    const int64_t b0 = (int64_t)tile * WAVE;

    if (wave == 0) reinterpret_cast<float4 *>(lc)[lane] = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], qdv[NJ], qddv[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qdv[d] = qd[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qddv[d] = qdd ? qdd[r0 + d] : 0.0f;
    }
    __syncthreads();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };
    const int32_t *w0 = ops_i + DRM_OPI_W0 * CAP;
    auto perm = [&](int k) -> int { return (w0[k] >> 27) & 7; };

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    regressor_chain_trig<LINKS, NJ>(
        row, perm, gravity, cs, sn, qdv, qddv,
        [&](int k) {
            if (regressor_owner<LINKS>(k) != wave) return false;
#pragma unroll 1
            for (int j = k + 1; j < NJ; ++j) { // the joints below body k do not carry it
#pragma unroll
                for (int c = 0; c < REG_COLS; ++c) mine[j * P + REG_COLS * k + c] = 0.0f;
            }
            return true;
        },
        [&](int j, int k, int col, float v) { mine[j * P + REG_COLS * k + col] = v; });
    if (damping && wave == 0) { // Y[j, 10 LINKS + d] = qd_j where d == j
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int d = 0; d < NJ; ++d) mine[j * P + REG_COLS * LINKS + d] = d == j ? qdv[j] : 0.0f;
    }
    __syncthreads();
    // the tile's rows are contiguous in Y: 64 RP floats = 16 RP vectors, by the whole block
    float4 *g4 = reinterpret_cast<float4 *>(Y + b0 * RP);
    const float4 *l4 = reinterpret_cast<const float4 *>(image);
    for (int i = (int)threadIdx.x; i < 16 * RP; i += REG_ARM_WAVES * WAVE) g4[i] = l4[i];
}

// The general kernel.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles.  The lanes' records, [record
// float][64 lanes]: drm_rows.hpp rows_state.  Y arrives zeroed: only the ancestors' rows are stored.
template <bool IN_LDS>
__global__ void __launch_bounds__(WAVE)
    regressor_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int p_end, int n,
                          const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ qdd, int64_t B,
                          int64_t n_tiles, int flags, float *__restrict__ Y, float *__restrict__ scratch, int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    float *trig = state, *slots = state + 3 * n_ops * WAVE;
    const int n_slots = (state_floats - 3 * n_ops) / 12;
    const bool damping = flags & DRM_RNEA_DAMPING;
    const float g = (flags & DRM_RNEA_GRAVITY) ? 9.81f : 0.0f;
    const int P = REG_COLS * n_ops + (damping ? n : 0);
    const RowsCtl ctl(ops_i, cap);
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue; // (a lane shares nothing with its neighbours: no barrier below)
        const float *qr = q + r * n, *qdr = qd + r * n, *qddr = qdd ? qdd + r * n : nullptr;
        float *Yr = Y + r * n * P;
        regressor_tree_walk(
            n_ops, p_end, ctl, row, g, [&](int d, float &a, float &v, float &acc) { a = qr[d]; v = qdr[d]; acc = qddr ? qddr[d] : 0.0f; },
            [&](int k, float c, float s, float x) { trig[(3 * k) * WAVE] = c; trig[(3 * k + 1) * WAVE] = s; trig[(3 * k + 2) * WAVE] = x; },
            [&](int k, float &c, float &s, float &x) { c = trig[(3 * k) * WAVE]; s = trig[(3 * k + 1) * WAVE]; x = trig[(3 * k + 2) * WAVE]; },
            [&](int sl, const Motion &M) {
                if (sl >= n_slots) return; // (a malformed table must not write past the records)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    slots[(12 * sl + 4 * i) * WAVE] = M.wa[i][0]; slots[(12 * sl + 4 * i + 1) * WAVE] = M.wa[i][1];
                    slots[(12 * sl + 4 * i + 2) * WAVE] = M.va[i][0]; slots[(12 * sl + 4 * i + 3) * WAVE] = M.va[i][1];
                }
            },
            [&](int sl, Motion &M) {
                if (sl >= n_slots) return;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    M.wa[i] = f2_make(slots[(12 * sl + 4 * i) * WAVE], slots[(12 * sl + 4 * i + 1) * WAVE]);
                    M.va[i] = f2_make(slots[(12 * sl + 4 * i + 2) * WAVE], slots[(12 * sl + 4 * i + 3) * WAVE]);
                }
            },
            [&](int dof, int op, int col, float v) {
                if (dof < n) Yr[dof * P + REG_COLS * op + col] = v;
            });
        if (damping) {
#pragma unroll 1
            for (int j = 0; j < n; ++j) Yr[j * P + REG_COLS * n_ops + j] = qdr[j];
        }
    }
}

} // namespace drm

using namespace drm;

// (DRM_REGRESSOR_COMPOSED sends an arm's rows through the general kernel: its state fits LDS, no scratch either way)
static int64_t regressor_scratch(const drm_walk *w, int64_t B, bool aligned) {
    return check_regressor_walk(w) ? 0 : rows_scratch_floats(w, B, aligned, regressor_state_floats(w), REG_LDS_BYTES);
}
extern "C" int64_t drm_rnea_regressor_scratch_floats(const drm_walk *w, int64_t B) { return regressor_scratch(w, B, false); }
extern "C" int64_t drm_rnea_regressor_scratch_floats_aligned(const drm_walk *w, int64_t B) { return regressor_scratch(w, B, true); }

extern "C" int drm_rnea_regressor(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *Y,
                                  float *scratch, void *stream) {
    int rc = args_rnea_regressor(w, q, qd, B, Y);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs;
    const int kflags = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    const int64_t P = (int64_t)REG_COLS * w->n_ops + ((flags & DRM_RNEA_DAMPING) ? n : 0);
    int64_t lo = 0;
    if (!(flags & DRM_REGRESSOR_COMPOSED) && rows_fused(w, B, aligned16(q, qd, qdd, Y))) {
        const int n_tiles = (int)(B / WAVE);
        const size_t lds = sizeof(float) * (size_t)(8 * DRM_OPF_STRIDE + WAVE * n * P);
        if (arm_links(w) == 7) {
            rc = ensure_lds(regressor_arm_kernel<7, 7>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL((regressor_arm_kernel<7, 7>), dim3((unsigned)n_tiles), dim3(REG_ARM_WAVES * WAVE), lds, s, w->ops_f, w->ops_i, q,
                               qd, qdd, n_tiles, kflags, Y);
        } else {
            rc = ensure_lds(regressor_arm_kernel<7, 8>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL((regressor_arm_kernel<7, 8>), dim3((unsigned)n_tiles), dim3(REG_ARM_WAVES * WAVE), lds, s, w->ops_f, w->ops_i, q,
                               qd, qdd, n_tiles, kflags, Y);
        }
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general kernel over rows [lo, B)
    const int64_t rows = B - lo;
    const RowsPlan plan = rows_plan(rows, regressor_state_floats(w), REG_LDS_BYTES);
    const int p_end = w->n_segments > 1 ? w->prefix_end : 0;
    const float *qs = q + lo * n, *qds = qd + lo * n, *qdds = qdd ? qdd + lo * n : nullptr;
    float *Ys = Y + lo * n * P;
    rc = rows_zero({Ys}, (size_t)rows * n * P, s);
    if (rc) return rc;
    return rows_launch(regressor_rows_kernel<true>, regressor_rows_kernel<false>, plan, scratch, "drm_rnea_regressor_scratch_floats", s, w->ops_f,
                       w->ops_i, (int)w->capacity, (int)w->n_ops, p_end, n, qs, qds, qdds, rows, plan.tiles, kflags, Ys);
}

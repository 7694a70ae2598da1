// drm_fdd.hip — forward dynamics and its linearisation about a state in one call (include/drm_hip.h
// drm_forward_dynamics_derivatives): qdd = H^-1 (f - nle), dqdd_dq = -H^-1 dID/dq at (q, qd, qdd), dqdd_dqd = -H^-1 dID/dqd and
// minv = H^-1.  What a caller otherwise gets from n backward passes through drm_forward_dynamics with one-hot cotangents (each an
// implicit solve through H plus a launch of the RNEA backward) and an n x n transpose.
//
//   forward_dynamics_derivatives_arm_kernel   serial 7-DoF arm chains, full 64-row tiles: one wavefront per tile, one row per lane, the
//                                     constant table staged in LDS once, ONE chain_trig shared by rnea_chain_trig (qdd = 0),
//                                     crba_chain_trig and the reverse sweeps; H factorised once in registers (L^T D L): qdd, the lower
//                                     triangle of H^-1, then one reverse sweep of RNEA per row of dID/dq and dID/dqd (a rolled loop: the
//                                     rows land in the lane's stretch of two LDS tiles) and 2 n solves in place there; the three
//                                     matrices leave LDS in 16-byte stores
//   forward_dynamics_derivatives_finish_*_kernel   the composed path: drm_forward_dynamics, drm_crba and n calls of drm_rnea_backward
//                                     (grad_tau = e_k) write into the scratch, the finish kernel inverts and solves with one lane per
//                                     row — n <= 16: H in registers, every array through an LDS tile; beyond: H factorised in the
//                                     lane's stretch of LDS, or in place in the scratch where 64 rows do not fit (n > 24).
//                                     Every other robot, the ragged tail, misaligned pointers, DRM_FDD_COMPOSED.
// The per-row arithmetic is drm_fdd.hpp's, shared with the host build.
//
// Per row, fused, n = 7: in q, qd, f (84 B); out 4 (7 + 3 x 49) B = 616 B.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_fdd.hpp"
#include "drm_sample.hpp"
#include "drm_args.hpp"

namespace drm {

// Serial 7-DoF arm chains, full tiles.  LINKS as in forward_dynamics_arm_kernel: the ops the sweeps visit (NJ when the host folded the
// fixed tail into the last moving link, else CAP).
// LDS per wavefront: [ table : CAP x 32 ][ RNEA's parked body forces : (LINKS - KEEP) x 6 x 64; then two tiles of 64 x 49: qdd and
// minv leave through the first before the sweeps fill the two with dID/dq | dID/dqd ]: 25.5 KB, six wavefronts per CU
// (a lane's rows of the tiles lie 49 floats apart: an odd pitch, no bank conflicts)
template <int CAP, int NJ, int LINKS>
__global__ void __launch_bounds__(WAVE)
    forward_dynamics_derivatives_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, const float *__restrict__ qd,
                                            const float *__restrict__ f, int n_tiles, int flags, float *__restrict__ qdd,
                                            float *__restrict__ dq, float *__restrict__ dqd, float *__restrict__ minv) {
    static_assert(NJ & 1, "odd row widths only (linear LDS image)");
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    constexpr int NN = NJ * NJ;
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, F_FLOATS = (LINKS - DRM_RNEA_KEEP) * 6 * WAVE, T_FLOATS = round4(WAVE * NN);
    static_assert(F_FLOATS <= 2 * T_FLOATS && round4(WAVE * NJ) <= T_FLOATS, "the parking area and the qdd tile fit under the two tiles");
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + 2 * T_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *lq = smem + C_FLOATS, *lv = lq + T_FLOATS;
    float *park = lq + lane;
    const int64_t b0 = (int64_t)tile * WAVE;

    float4 cv = reinterpret_cast<const float4 *>(ops_f)[lane];
    float qv[NJ], qdv[NJ], acc[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) qdv[d] = qd[r0 + d];
#pragma unroll
        for (int d = 0; d < NJ; ++d) acc[d] = f[r0 + d];
    }
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    // a row whose q, qd or f is not finite walks the chain at rest at q = 0 and gets NaN outputs: a NaN angle in any lane would send
    // the whole wavefront's sines and cosines down chain_trig's slow path and change other rows' bits
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || !isfinite(qv[d]) || !isfinite(qdv[d]) || !isfinite(acc[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; acc[d] = bad ? 0.0f : acc[d]; }
    const bool gravity = flags & DRM_RNEA_GRAVITY, damping = flags & DRM_RNEA_DAMPING;
    const float nan = __builtin_nanf("");

    // forward dynamics as forward_dynamics_arm_kernel: bias torques first, H afterwards (the triangle is not live across RNEA)
    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    {
        float zero[NJ], nle[NJ];
#pragma unroll
        for (int d = 0; d < NJ; ++d) zero[d] = 0.0f;
        rnea_chain_trig<LINKS, NJ>(row, gravity, damping, cs, sn, qdv, zero, nle,
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
#pragma unroll
        for (int d = 0; d < NJ; ++d) acc[d] -= nle[d];
    }
    float Ht[NJ * (NJ + 1) / 2], bw[NJ];
    crba_chain_trig<LINKS, NJ>(row, cs, sn, [&](int i, int j, float v) {
        if (i >= j) Ht[tri_index(i, j)] = v;
    });
    auto H = [&](int i, int j) -> float & { return Ht[tri_index(i, j)]; };
    auto b = [&](int i) -> float & { return bw[i]; };
    fdd_ltdl_factor<float>(NJ, H);
    fdd_ltdl_apply<float>(NJ, H, [&](int i) -> float & { return acc[i]; });   // acc = qdd

    wave_lds_sync(); // every lane is done with the parking area before the tiles are staged over it
    float *mine_q = lq + lane * NN, *mine_v = lv + lane * NN;
    // qdd (unless the entry point leaves it to drm_forward_dynamics: wave-uniform), then minv leave through the dID/dq tile before
    // the sweeps fill it
    if (qdd) {
#pragma unroll
        for (int d = 0; d < NJ; ++d) lq[lane * NJ + d] = bad ? nan : acc[d];
        wave_lds_sync();
        tile_store<NJ>(qdd + b0 * NJ, WAVE, NJ, 0u, lq, lane, true);
        wave_lds_sync();
    }
    fdd_inverse<float>(NJ, H, b, [&](int i, int c, float v) {
        mine_q[i * NJ + c] = bad ? nan : v;
        mine_q[c * NJ + i] = bad ? nan : v;
    });
    wave_lds_sync();
    tile_store<NN>(minv + b0 * NN, WAVE, NN, 0u, lq, lane, true);
    wave_lds_sync();

    // row k of dID/dq and dID/dqd: the reverse sweep seeded with e_k
    Motion tip;
    fdd_chain_tip_motion<LINKS, NJ>(row, gravity, cs, sn, qdv, acc, tip);
#pragma unroll 1
    for (int k = 0; k < NJ; ++k) {
        // the table is read again in every trip, from an offset the compiler cannot see through: hoisted out of the loop, the eight rows
        // and the joint transforms made from them stay live across it and the kernel spills (204 VGPRs to scratch)
        int off = 0;
        asm volatile("" : "+v"(off));
        auto rowk = [&](int j) -> const float * { return lc + off + j * DRM_OPF_STRIDE; };
        float seed[NJ];
#pragma unroll
        for (int d = 0; d < NJ; ++d) seed[d] = d == k ? 1.0f : 0.0f;
        fdd_chain_adjoint<LINKS, NJ>(rowk, gravity, damping, cs, sn, qdv, acc, tip, seed, [&](int d, float gq, float gqd) {
            mine_q[k * NJ + d] = gq;
            mine_v[k * NJ + d] = gqd;
        });
    }
    // the 2 n columns of [dID/dq | dID/dqd] solved in place, one per trip of a rolled loop (unrolled, the loads of all the columns
    // are hoisted and the kernel spills)
#pragma unroll 1
    for (int c = 0; c < 2 * NJ; ++c) {
        float *g = c < NJ ? mine_q + c : mine_v + (c - NJ);
        fdd_solve_column<float>(NJ, H, b, [&](int i, int) { return g[i * NJ]; }, [&](int i, int, float v) { g[i * NJ] = bad ? nan : v; }, 0);
    }
    wave_lds_sync();
    tile_store<NN>(dq + b0 * NN, WAVE, NN, 0u, lq, lane, true);
    __builtin_amdgcn_sched_barrier(0);
    tile_store<NN>(dqd + b0 * NN, WAVE, NN, 0u, lv, lane, true);
}

// The composed path's start, one thread per element of [rows, n] (coalesced): the q, qd and f the walks read — the row's own, or zeros
// where any entry of the row is not finite (as in the fused kernel; the finish kernel writes that row's outputs as NaN) — the row's
// flag, and the one-hot seeds of the n reverse sweeps, seeds[k][row][d] = (d == k)
__global__ void __launch_bounds__(256)
    forward_dynamics_derivatives_start_kernel(const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ f,
                                              int64_t rows, int n, float *__restrict__ qs, float *__restrict__ qds, float *__restrict__ fs,
                                              float *__restrict__ okf, float *__restrict__ seeds, int64_t slab) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * n) return;
    const int64_t r = e / n;
    const int d = (int)(e - r * n);
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && isfinite(q[r * n + k]) && isfinite(qd[r * n + k]) && isfinite(f[r * n + k]);
    qs[e] = ok ? q[e] : 0.0f;
    qds[e] = ok ? qd[e] : 0.0f;
    fs[e] = ok ? f[e] : 0.0f;
    if (d == 0) okf[r] = ok ? 1.0f : 0.0f;
    for (int k = 0; k < n; ++k) seeds[k * slab + e] = d == k ? 1.0f : 0.0f;
}

// The composed path's finish, one lane per row of [0, rows): H [n, n] as drm_crba wrote it, qdds [n] as drm_forward_dynamics did, and
// gq / gqd [k][row][n] = row k of dID/dq / dID/dqd as the n calls of drm_rnea_backward did.  64-lane blocks.
// IN_LDS: the row's H and the n-vector the solves work in live in the lane's own stretch of LDS (n^2 + n floats, odd pitch: no bank
// conflicts); otherwise H is factorised in place in the scratch and the vector lies in `work` (n > 24).
template <bool IN_LDS>
__global__ void __launch_bounds__(64)
    forward_dynamics_derivatives_finish_kernel(const float *__restrict__ okf, const float *__restrict__ qdds, float *__restrict__ Hs,
                                               const float *__restrict__ gq, const float *__restrict__ gqd, float *__restrict__ work,
                                               int64_t slab, int64_t rows, int n, float *__restrict__ qdd, float *__restrict__ dq,
                                               float *__restrict__ dqd, float *__restrict__ minv) {
    extern __shared__ __attribute__((aligned(16))) float fdd_rows_lds[];
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const bool ok = okf[r] != 0.0f;
    const float nan = __builtin_nanf("");
    float *Hr, *wr;
    if constexpr (IN_LDS) {
        Hr = fdd_rows_lds + threadIdx.x * ((n * n + n) | 1);
        wr = Hr + n * n;
        const float *Hg = Hs + r * n * n;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) Hr[i * n + j] = Hg[i * n + j];
    } else {
        Hr = Hs + r * n * n;
        wr = work + r * n;
    }
    auto H = [&](int i, int j) -> float & { return Hr[i * n + j]; };
    auto b = [&](int i) -> float & { return wr[i]; };
    const int64_t o = r * n * n;
    for (int k = 0; k < n; ++k) qdd[r * n + k] = ok ? qdds[r * n + k] : nan;
    fdd_ltdl_factor<float>(n, H);
    fdd_inverse<float>(n, H, b, [&](int i, int c, float v) {
        minv[o + i * n + c] = ok ? v : nan;
        minv[o + c * n + i] = ok ? v : nan;
    });
    fdd_solve_columns<float>(n, H, b, [&](int i, int j) { return gq[i * slab + r * n + j]; },
                             [&](int i, int j, float v) { dq[o + i * n + j] = ok ? v : nan; });
    fdd_solve_columns<float>(n, H, b, [&](int i, int j) { return gqd[i * slab + r * n + j]; },
                             [&](int i, int j, float v) { dqd[o + i * n + j] = ok ? v : nan; });
}

// The finish for a compile-time n <= FDD_FIXED_MAX, one wavefront per 64 rows: the row's H (packed triangle) and the solve vector in
// REGISTERS, every loop of drm_fdd.hpp unrolled (with a run-time n the same arithmetic walks LDS with computed addresses: 1.46 ms
// of the 2.56 ms of 2^20 composed Panda rows, 2.1 ms of 3.2 ms for 65 536 Fetch rows).  One n x n tile per row in LDS carries every
// array between HBM and the lanes with coalesced accesses by the whole wavefront: the block's H comes in through it, minv is staged
// in it and stored, then the rows of dID/dq (dID/dqd) are gathered into it, solved in place column by column and stored.
constexpr int FDD_FIXED_MAX = 16;
template <int N>
__global__ void __launch_bounds__(64, 1)
    forward_dynamics_derivatives_finish_fixed_kernel(const float *__restrict__ okf, const float *__restrict__ qdds,
                                                     const float *__restrict__ Hs, const float *__restrict__ gq,
                                                     const float *__restrict__ gqd, int64_t slab, int64_t rows, float *__restrict__ qdd,
                                                     float *__restrict__ dq, float *__restrict__ dqd, float *__restrict__ minv) {
    constexpr int NN = N * N, P = NN | 1;
    __shared__ __attribute__((aligned(16))) float tiles[64 * P];
    const int lane = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64, r = r0 + lane;
    const int cnt = rows - r0 < 64 ? (int)(rows - r0) : 64;
    const bool live = lane < cnt, ok = live && okf[r] != 0.0f;
    const float nan = __builtin_nanf("");
    float *tl = tiles + lane * P;
    auto store = [&](float *g) { // the block's cnt x n^2 tile, contiguous in g
        wave_lds_sync();
        for (int rr = 0; rr < cnt; ++rr)
            for (int c = lane; c < NN; c += 64) g[(r0 + rr) * NN + c] = tiles[rr * P + c];
        wave_lds_sync();
    };
    auto gather = [&](const float *g) { // tile[row][k][j] = g[k][row][j]: per k the block's cnt x n floats are contiguous
        for (int k = 0; k < N; ++k)
            for (int e = lane; e < cnt * N; e += 64) {
                const int rr = e / N;
                tiles[rr * P + k * N + (e - rr * N)] = g[k * slab + r0 * N + e];
            }
        wave_lds_sync();
    };
    for (int rr = 0; rr < cnt; ++rr)
        for (int c = lane; c < NN; c += 64) tiles[rr * P + c] = Hs[(r0 + rr) * NN + c];
    wave_lds_sync();
    float Ht[N * (N + 1) / 2], bw[N];
    auto H = [&](int i, int j) -> float & { return Ht[tri_index(i, j)]; };
    auto b = [&](int i) -> float & { return bw[i]; };
    if (live) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) H(i, j) = tl[i * N + j];
        for (int k = 0; k < N; ++k) qdd[r * N + k] = ok ? qdds[r * N + k] : nan;
        __builtin_amdgcn_sched_barrier(0);
        fdd_ltdl_factor<float>(N, H);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
        for (int i = 0; i < N; ++i)
#pragma unroll 4
            for (int j = 0; j < N; ++j) tl[i * N + j] = i == j ? -1.0f : 0.0f;
    }
    // the N columns of the tile solved in place, one per trip of a rolled loop (H and the vector keep compile-time indices); a row
    // that is not finite leaves as NaN
    auto solve = [&](bool mirror) {
        if (!live) return;
#pragma unroll 1
        for (int j = 0; j < N; ++j)
            fdd_solve_column<float>(N, H, b, [&](int i, int) { return tl[i * N + j]; }, [&](int i, int, float v) { tl[i * N + j] = v; }, 0);
        if (mirror) {
#pragma unroll 1
            for (int i = 1; i < N; ++i)
#pragma unroll 4
                for (int c = 0; c < i; ++c) tl[c * N + i] = tl[i * N + c];
        }
        if (!ok) {
#pragma unroll 4
            for (int i = 0; i < NN; ++i) tl[i] = nan;
        }
    };
    // minv = -H^-1 (-I), column by column as drm_fdd.hpp fdd_inverse (the zeros of e_c multiplied, not skipped: the same bits), the
    // lower triangle mirrored
    solve(true);
    store(minv);
    gather(gq);
    solve(false);
    store(dq);
    gather(gqd);
    solve(false);
    store(dqd);
}

template <int N>
static void launch_fdd_finish_fixed(unsigned blocks, hipStream_t s, const float *okf, const float *qdds, const float *H, const float *gq,
                                    const float *gqd, int64_t slab, int64_t rows, float *qdd, float *dq, float *dqd, float *minv) {
    hipLaunchKernelGGL((forward_dynamics_derivatives_finish_fixed_kernel<N>), dim3(blocks), dim3(64), 0, s, okf, qdds, H, gq, gqd, slab, rows,
                       qdd, dq, dqd, minv);
}

// the fused kernel takes the full tiles of what forward_dynamics_arm_kernel takes
static bool fdd_fused(const drm_walk *w, int64_t B, bool aligned) { return arm7_walk(w) && aligned && table_aligned(w) && full_tiles_fit(B); }

// scratch of the composed path over `rows` rows, every array 16-byte aligned: the walks' inputs qs / qds / fs, qdd of
// drm_forward_dynamics, the rows' flags, H of drm_crba, the n one-hot seeds, gq / gqd of the n reverse sweeps (slabs of rows x n
// floats), their grad_qdd (not used), the finish kernel's vectors, then what the three entry points ask for themselves (one after
// the other on the stream: they share it)
struct FddScratch {
    int64_t qs, qds, fs, qdd, ok, H, seeds, gq, gqd, gqdd, work, sub, slab, total;
};
static FddScratch fdd_scratch_layout(const drm_walk *w, int64_t rows) {
    auto r4 = [](int64_t x) { return (x + 3) & ~(int64_t)3; };
    const int64_t n = w->n_dofs;
    FddScratch s;
    s.slab = r4(rows * n);
    s.qs = 0;
    s.qds = s.qs + s.slab;
    s.fs = s.qds + s.slab;
    s.qdd = s.fs + s.slab;
    s.ok = s.qdd + s.slab;
    s.H = s.ok + r4(rows);
    s.seeds = s.H + r4(rows * n * n);
    s.gq = s.seeds + n * s.slab;
    s.gqd = s.gq + n * s.slab;
    s.gqdd = s.gqd + n * s.slab;
    s.work = s.gqdd + s.slab;
    s.sub = s.work + s.slab;
    const int64_t a = drm_crba_scratch_floats(w, rows), c = drm_forward_dynamics_scratch_floats(w, rows);
    const int64_t d = drm_rnea_backward_scratch_floats(rows, w->capacity, w->n_dofs, w->n_slots);
    const int64_t m = a > c ? (a > d ? a : d) : (c > d ? c : d);
    s.total = s.sub + r4(m > 1 ? m : 1);
    return s;
}

} // namespace drm

using namespace drm;

static int64_t fdd_scratch_floats_impl(const drm_walk *w, int64_t B, bool aligned) {
    if (check_backward_walk(w) || B <= 0) return 0;
    const int64_t lo = fdd_fused(w, B, aligned) ? B / WAVE * WAVE : 0;
    if (lo == B) return 0;
    return fdd_scratch_layout(w, B - lo).total;
}
extern "C" int64_t drm_forward_dynamics_derivatives_scratch_floats(const drm_walk *w, int64_t B) { return fdd_scratch_floats_impl(w, B, false); }
extern "C" int64_t drm_forward_dynamics_derivatives_scratch_floats_aligned(const drm_walk *w, int64_t B) {
    return fdd_scratch_floats_impl(w, B, true);
}

extern "C" int drm_forward_dynamics_derivatives(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, int32_t flags,
                                                float *qdd, float *dq, float *dqd, float *minv, float *scratch, void *stream) {
    int rc = args_forward_dynamics_derivatives(w, q, qd, f, B, qdd, dq, dqd, minv);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs, dyn_flags = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    const bool aligned = aligned16(q, qd, f, qdd, dq, dqd, minv, scratch);
    int64_t lo = 0;
    if (!(flags & DRM_FDD_COMPOSED) && fdd_fused(w, B, aligned)) {
        const int n_tiles = (int)(B / WAVE);
        // qdd is what drm_forward_dynamics returns, to the value: a walk that carries its robot's own forward-dynamics kernel (constants
        // folded into the instruction stream: another rounding, 5e-5 apart on an iiwa) gets its qdd from that kernel, in a launch of
        // its own; the derivatives are taken at the fused kernel's qdd either way
        const bool own_fd = w->special[DRM_SPECIAL_FD] || w->special[DRM_SPECIAL_FD_ARM] || w->special[DRM_SPECIAL_FD_ARM2];
        float *qdd_fused = own_fd ? nullptr : qdd;
        if (arm_links(w) == 7)
            hipLaunchKernelGGL((forward_dynamics_derivatives_arm_kernel<8, 7, 7>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, f,
                               n_tiles, dyn_flags, qdd_fused, dq, dqd, minv);
        else
            hipLaunchKernelGGL((forward_dynamics_derivatives_arm_kernel<8, 7, 8>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, w->ops_f, q, qd, f,
                               n_tiles, dyn_flags, qdd_fused, dq, dqd, minv);
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (own_fd) { // (full aligned tiles of an arm: no scratch)
            rc = drm_forward_dynamics(w, q, qd, f, lo, dyn_flags, qdd, nullptr, stream);
            if (rc) return rc;
        }
        if (lo == B) return DRM_OK;
    }
    // the composed path over rows [lo, B)
    if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_forward_dynamics_derivatives_scratch_floats() floats of scratch");
    const int64_t rows = B - lo;
    if (rows * n / 256 >= GRID_MAX) return fail(DRM_ERR_UNSUPPORTED, "batch too large");
    const FddScratch L = fdd_scratch_layout(w, rows);
    float *qs = scratch + L.qs, *qds = scratch + L.qds, *fs = scratch + L.fs, *qdds = scratch + L.qdd, *okf = scratch + L.ok;
    float *H = scratch + L.H, *seeds = scratch + L.seeds, *gq = scratch + L.gq, *gqd = scratch + L.gqd, *gqdd = scratch + L.gqdd;
    float *work = scratch + L.work, *sub = scratch + L.sub;
    const unsigned blocks = (unsigned)((rows + 63) / 64);
    hipLaunchKernelGGL(forward_dynamics_derivatives_start_kernel, dim3((unsigned)((rows * n + 255) / 256)), dim3(256), 0, s, q + lo * n, qd + lo * n, f + lo * n, rows, n, qs,
                       qds, fs, okf, seeds, L.slab);
    rc = launched();
    if (rc) return rc;
    rc = drm_forward_dynamics(w, qs, qds, fs, rows, dyn_flags, qdds, sub, stream);
    if (rc) return rc;
    rc = drm_crba(w, qs, rows, H, sub, stream);
    if (rc) return rc;
    for (int k = 0; k < n; ++k) {
        rc = drm_rnea_backward(w, qs, qds, qdds, rows, dyn_flags, seeds + k * L.slab, 0, gq + k * L.slab, gqd + k * L.slab, gqdd, nullptr, sub,
                               stream);
        if (rc) return rc;
    }
    float *oq = qdd + lo * n, *odq = dq + lo * n * n, *odqd = dqd + lo * n * n, *om = minv + lo * n * n;
    if (n <= FDD_FIXED_MAX) {
#define FDD_FIXED(N) case N: launch_fdd_finish_fixed<N>(blocks, s, okf, qdds, H, gq, gqd, L.slab, rows, oq, odq, odqd, om); break
        switch (n) {
            FDD_FIXED(1); FDD_FIXED(2); FDD_FIXED(3); FDD_FIXED(4); FDD_FIXED(5); FDD_FIXED(6); FDD_FIXED(7); FDD_FIXED(8);
            FDD_FIXED(9); FDD_FIXED(10); FDD_FIXED(11); FDD_FIXED(12); FDD_FIXED(13); FDD_FIXED(14); FDD_FIXED(15); FDD_FIXED(16);
        }
#undef FDD_FIXED
        return launched();
    }
    // any larger n: the rows' H and solve vector in LDS where 64 of them fit, else in the scratch
    const size_t lds = sizeof(float) * 64 * (size_t)((n * n + n) | 1);
    const bool in_lds = lds <= (size_t)MAX_LDS_BYTES;
    if (in_lds) {
        rc = ensure_lds(forward_dynamics_derivatives_finish_kernel<true>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL((forward_dynamics_derivatives_finish_kernel<true>), dim3(blocks), dim3(64), lds, s, (const float *)okf,
                           (const float *)qdds, H, (const float *)gq, (const float *)gqd, work, L.slab, rows, n, oq, odq, odqd, om);
    } else {
        hipLaunchKernelGGL((forward_dynamics_derivatives_finish_kernel<false>), dim3(blocks), dim3(64), 0, s, (const float *)okf,
                           (const float *)qdds, H, (const float *)gq, (const float *)gqd, work, L.slab, rows, n, oq, odq, odqd, om);
    }
    return launched();
}

// drm_osc.hip — operational-space dynamics of one link in one call (include/drm_hip.h drm_operational_space): the task-space
// inertia (J H^-1 J^T + reg^2 I)^-1, the dynamically consistent inverse of J, Jdot qd and the task-space bias force.  What a caller
// otherwise composes from drm_fk_jacobian, drm_crba, drm_rnea (three passes over the same q, three sin / cos evaluations, the
// [B, 6, n] and [B, n, n] intermediates through HBM) and a chain of small batched solves, and cannot get at all for Jdot qd.
//
//   operational_space_arm_kernel      serial 7-DoF arm chains whose target is the chain's last link, full 64-row tiles: one wavefront
//                                     per tile, the constant table staged in LDS once, ONE chain_trig shared by rnea_chain_trig
//                                     (qdd = 0), crba_chain_trig and the FK chain; H factorised once in registers (L^T D L), solved
//                                     against the M rows of J; A inverted by Cholesky; the four outputs staged through LDS one
//                                     after the other (over RNEA's parking area) and stored 16 bytes at a time
//   operational_space_finish_kernel   the composed path: drm_fk_jacobian, drm_crba and drm_rnea (qdd = NULL) write into the scratch,
//                                     this kernel finishes with one lane per row — H factorised in the lane's stretch of LDS, or in
//                                     place in the scratch where 64 rows do not fit (any n <= DRM_MAX_DOFS), Jdot qd from a walk of
//                                     the chain's control words over the Jacobian's columns.
//                                     Every other robot, a mid-chain target, the ragged tail, misaligned pointers, DRM_OSC_COMPOSED.
// The per-row arithmetic is drm_osc.hpp's, shared with the host build.
//
// Per row, fused, n = 7: in q, qd (56 B); out 4 (M^2 + 7 M + 2 M) B = 360 B for M = 6, 144 B for M = 3.
#include <math.h>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#include "drm_osc.hpp"
#include "drm_sample.hpp"
#include "drm_args.hpp"

namespace drm {

// ceil(2^32 / S), drm_common.hpp div_magic at compile time
constexpr uint32_t osc_magic(int S) { return (uint32_t)((((uint64_t)1 << 32) + (uint64_t)S - 1) / (uint64_t)S); }

// One output tile of the fused kernel: lane `lane` hands its S values over through val(i), the tile leaves with 16-byte stores.
// LDS image as tile_store reads it: linear for odd S, row stride S + 1 for even S (no bank conflicts either way).  `bad`: NaN row.
template <int S, class VAL>
__device__ __forceinline__ void osc_store_tile(float *__restrict__ g, float *lds, unsigned lane, bool bad, VAL val) {
    constexpr int SP = S | 1;
#pragma unroll
    for (int i = 0; i < S; ++i) lds[lane * SP + i] = bad ? __builtin_nanf("") : val(i);
    wave_lds_sync();
    if (S & 1) tile_store<S>(g, WAVE, S, 0u, lds, lane, true);
    else tile_store<S>(g, WAVE, S, osc_magic(S), lds, lane, false, true);
    wave_lds_sync(); // the next tile is staged over this one
}

// Serial 7-DoF arm chains, full tiles.  LINKS as in fk_rnea_arm_kernel: the ops the dynamics sweeps visit (NJ when the host folded
// the fixed tail into the last moving link, rows from the TREE walk's table), the FK chain walks all CAP ops (rows LINKS .. CAP-1
// from the CHAIN walk's table).  M = 6, or 3 in position-only mode.
// Order of the walks: bias torques, then H and its factorisation, then the FK chain — RNEA's peak is not shared with the 28-entry
// triangle, and the Jacobian (6 NJ floats) comes to life only once the walks' own temporaries are gone.
// LDS per wavefront: [ table : CAP x 32 ][ RNEA's parked body forces : (LINKS - KEEP) x 6 x 64, then the output tiles ]
template <int CAP, int NJ, int LINKS, int M>
__global__ void __launch_bounds__(WAVE)
    operational_space_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ ops_tail, const float *__restrict__ q,
                                 const float *__restrict__ qd, int n_tiles, int flags, float reg2, float *__restrict__ inertia,
                                 float *__restrict__ jbar, float *__restrict__ bias_acc, float *__restrict__ bias_force) {
    static_assert(CAP * DRM_OPF_STRIDE == 4 * WAVE, "one float4 per lane copies the constant table");
    static_assert(M == 3 || M == 6, "lin_jac alone, or [lin_jac; ang_jac]");
    constexpr int C_FLOATS = CAP * DRM_OPF_STRIDE, F_FLOATS = (LINKS - DRM_RNEA_KEEP) * 6 * WAVE;
    constexpr int WIDEST = NJ * M > M * M ? NJ * M : M * M, T_FLOATS = round4(WAVE * (WIDEST | 1));
    constexpr int S_FLOATS = F_FLOATS > T_FLOATS ? F_FLOATS : T_FLOATS;
    __shared__ __attribute__((aligned(16))) float smem[C_FLOATS + S_FLOATS];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const unsigned lane = threadIdx.x & 63u;
    float *lc = smem, *ls = smem + C_FLOATS;
    float *park = ls + lane;
    const int64_t b0 = (int64_t)tile * WAVE, b = b0 + lane;

    float4 cv = reinterpret_cast<const float4 *>(lane < LINKS * (DRM_OPF_STRIDE / 4) ? ops_f : ops_tail)[lane];
    float qv[NJ], qdv[NJ];
#pragma unroll
    for (int d = 0; d < NJ; ++d) qv[d] = q[b * NJ + d];
#pragma unroll
    for (int d = 0; d < NJ; ++d) qdv[d] = qd ? qd[b * NJ + d] : 0.0f;
    pin(cv);
    reinterpret_cast<float4 *>(lc)[lane] = cv;
    wave_lds_sync();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };

    // a row whose q or qd is not finite walks the chain at rest at q = 0 and gets NaN outputs: a NaN angle in any lane would send the
    // whole wavefront's sines and cosines down chain_trig's slow path and change other rows' bits
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || !isfinite(qv[d]) || !isfinite(qdv[d]);
#pragma unroll
    for (int d = 0; d < NJ; ++d) { qv[d] = bad ? 0.0f : qv[d]; qdv[d] = bad ? 0.0f : qdv[d]; }

    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);
    float nle[NJ];
    if (bias_force) { // (wave-uniform)
        float zero[NJ];
#pragma unroll
        for (int d = 0; d < NJ; ++d) zero[d] = 0.0f;
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
    } else {
#pragma unroll
        for (int d = 0; d < NJ; ++d) nle[d] = 0.0f;
    }
    float Ht[NJ * (NJ + 1) / 2];
    crba_chain_trig<LINKS, NJ>(row, cs, sn, [&](int i, int j, float v) {
        if (i >= j) Ht[tri_index(i, j)] = v;
    });
    auto H = [&](int i, int j) -> float & { return Ht[tri_index(i, j)]; };
    osc_ltdl_factor(NJ, H);

    // the Jacobian of the last link from the axes and origins of the chain (robot_model.py:626-667), Jdot qd from the same registers
    float Jv[M][NJ], acc[M];
    {
        PoseP ee;
        f2 Bk[NJ][3];
        fk_chain_pairs_trig<CAP, NJ>(row, cs, sn, ee, Bk, [] {});
        const float pe[3] = {ee.B[0][1], ee.B[1][1], ee.B[2][1]};
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const float z[3] = {Bk[k][0][0], Bk[k][1][0], Bk[k][2][0]};
            const float dp[3] = {pe[0] - Bk[k][0][1], pe[1] - Bk[k][1][1], pe[2] - Bk[k][2][1]};
            float c[3];
            cross3(z, dp, c);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                Jv[r][k] = c[r];
                if (M == 6) Jv[M - 3 + r][k] = z[r];
            }
        }
        osc_bias_acc<M>(NJ, [&](int k, float *z, float *r, bool &pris, float &v) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { z[i] = Bk[k][i][0]; r[i] = pe[i] - Bk[k][i][1]; }
            pris = false;
            v = qdv[k];
            return true;
        }, acc);
    }
    auto J = [&](int r, int k) -> float { return Jv[r][k]; };
    float Xv[M][NJ], Lam[M][M], eta[M];
    auto X = [&](int r, int k) -> float & { return Xv[r][k]; };
    osc_solve_columns<M>(NJ, H, J, X);
    osc_inertia<M>(NJ, J, X, reg2, Lam);
    osc_bias_force<M>(NJ, X, [&](int k) { return nle[k]; }, acc, Lam, eta);

    wave_lds_sync(); // every lane is done with the parking area before the output tiles are staged over it
    if (inertia) osc_store_tile<M * M>(inertia + b0 * (M * M), ls, lane, bad, [&](int i) { return Lam[i / M][i % M]; });
    if (jbar) osc_store_tile<NJ * M>(jbar + b0 * (NJ * M), ls, lane, bad, [&](int i) { return osc_jbar<M>(X, Lam, i / M, i % M); });
    if (bias_acc) osc_store_tile<M>(bias_acc + b0 * M, ls, lane, bad, [&](int i) { return acc[i]; });
    if (bias_force) osc_store_tile<M>(bias_force + b0 * M, ls, lane, bad, [&](int i) { return eta[i]; });
}

// The composed path's start, one lane per row: the q and qd the three walks read — the row's own, or zeros where either is not finite
// (as in the fused kernel; the finish kernel writes that row's outputs as NaN)
__global__ void __launch_bounds__(64)
    operational_space_start_kernel(const float *__restrict__ q, const float *__restrict__ qd, int64_t rows, int n, float *__restrict__ qs,
                                   float *__restrict__ qds) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && isfinite(q[b * n + k]) && (!qd || isfinite(qd[b * n + k]));
    for (int k = 0; k < n; ++k) {
        qs[b * n + k] = ok ? q[b * n + k] : 0.0f;
        qds[b * n + k] = ok && qd ? qd[b * n + k] : 0.0f;
    }
}

// The composed path's finish, one lane per row of [0, rows): lin / ang [3, n] as drm_fk_jacobian wrote them, H [n, n] as drm_crba did,
// nle [n] as drm_rnea did (bias_force wanted).  w0: the W0 control words of the chain walk (DoF column and joint kind of every op, in
// chain order).  64-lane blocks, as the IK update kernel.
// IN_LDS: the row's H and X = J H^-1 live in the lane's own stretch of LDS (n^2 + M n floats, odd pitch: no bank conflicts) — H is
// read from the scratch once and factorised there.  Factorising in place in the scratch costs O(n^3) strided 4-byte accesses per
// row, which fall out of the caches beyond some 10^5 rows (measured: 20.5 ms instead of 0.37 ms x 16 for 2^20 Panda rows); that
// form remains for robots whose rows do not fit (n > 21 at M = 6).
template <int M, bool IN_LDS>
__global__ void __launch_bounds__(64)
    operational_space_finish_kernel(const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ qds,
                                    const float *__restrict__ lin, const float *__restrict__ ang, float *__restrict__ Hs,
                                    const float *__restrict__ nles, float *__restrict__ Xs, const int32_t *__restrict__ w0, int chain_ops,
                                    int64_t rows, int n, float reg2, float *__restrict__ inertia, float *__restrict__ jbar,
                                    float *__restrict__ bias_acc, float *__restrict__ bias_force) {
    extern __shared__ __attribute__((aligned(16))) float osc_rows_lds[];
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && isfinite(q[b * n + k]) && (!qd || isfinite(qd[b * n + k]));
    const float *lr = lin + b * 3 * n, *ar = ang + b * 3 * n, *vr = qds + b * n;
    auto J = [&](int r, int k) -> float { return r < 3 ? lr[r * n + k] : ar[(r - 3) * n + k]; };
    float Lam[M][M], acc[M], eta[M];
    auto solve = [&](float *Hr, float *Xr) {
        auto H = [&](int i, int j) -> float & { return Hr[i * n + j]; };
        auto X = [&](int r, int k) -> float & { return Xr[r * n + k]; };
        osc_ltdl_factor(n, H);
        osc_solve_columns<M>(n, H, J, X);
        osc_inertia<M>(n, J, X, reg2, Lam);
    };
    float *Xr;
    if constexpr (IN_LDS) {
        float *Hl = osc_rows_lds + threadIdx.x * ((n * n + M * n) | 1);
        const float *Hg = Hs + b * n * n;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) Hl[i * n + j] = Hg[i * n + j];
        Xr = Hl + n * n;
        solve(Hl, Xr);
    } else {
        Xr = Xs + b * M * n;
        solve(Hs + b * n * n, Xr);
    }
    auto X = [&](int r, int k) -> float & { return Xr[r * n + k]; };
    osc_bias_acc<M>(chain_ops, [&](int k, float *z, float *r, bool &pris, float &v) {
        const int d = (w0[k] & 0xff) - 1;
        if (d < 0) return false;
        pris = (w0[k] >> 26) & 1;
        const float jp[3] = {lr[d], lr[n + d], lr[2 * n + d]};
        for (int i = 0; i < 3; ++i) z[i] = pris ? jp[i] : ar[i * n + d];
        cross3(jp, z, r); // the point of the axis nearest to the target: r = (z x (p - p_k)) x z
        v = vr[d];
        return true;
    }, acc);
    const float nan = __builtin_nanf("");
    if (bias_force) {
        const float *nr = nles + b * n;
        osc_bias_force<M>(n, X, [&](int k) { return nr[k]; }, acc, Lam, eta);
        for (int i = 0; i < M; ++i) bias_force[b * M + i] = ok ? eta[i] : nan;
    }
    if (bias_acc)
        for (int i = 0; i < M; ++i) bias_acc[b * M + i] = ok ? acc[i] : nan;
    if (inertia)
        for (int i = 0; i < M * M; ++i) inertia[b * (M * M) + i] = ok ? Lam[i / M][i % M] : nan;
    if (jbar)
        for (int k = 0; k < n; ++k)
            for (int c = 0; c < M; ++c) jbar[(b * n + k) * M + c] = ok ? osc_jbar<M>(X, Lam, k, c) : nan;
}

// The fused kernel takes the full tiles of this pair of walks: where drm_fk_rnea fuses (drm_rnea.hip fk_rnea_arm_applies) — the tree
// walk IS the chain (`same`), or holds the moving joints only and the chain still walks the fixed tail.  The target's axis code plays
// no part: no orientation is emitted.
static bool osc_fused(const drm_walk *tree, const drm_walk *chain, int64_t B, bool aligned, bool &same) {
    const int n = tree->n_dofs;
    const bool chain_arm = (chain->shape & DRM_WALK_ARM_CHAIN) && chain->capacity == 8 && chain->n_dofs == n;
    same = tree->n_ops == chain->n_ops;
    const bool folded = tree->n_ops == n && chain->n_ops > n;
    return arm7_walk(tree) && chain_arm && (same || folded) && aligned && table_aligned(tree) && table_aligned(chain) && full_tiles_fit(B);
}

// scratch of the composed path over `rows` rows, every array 16-byte aligned: the walks' inputs qs / qds, lin / ang of
// drm_fk_jacobian, H of drm_crba, nle of drm_rnea, X of the finish kernel, then what drm_crba / drm_rnea ask for themselves (one
// after the other on the stream: they share it)
struct OscScratch {
    int64_t qs, qds, lin, ang, H, nle, X, sub, total;
};
static OscScratch osc_scratch_layout(const drm_walk *tree, int64_t rows) {
    auto r4 = [](int64_t x) { return (x + 3) & ~(int64_t)3; };
    const int64_t n = tree->n_dofs;
    OscScratch s;
    s.qs = 0;
    s.qds = s.qs + r4(rows * n);
    s.lin = s.qds + r4(rows * n);
    s.ang = s.lin + r4(rows * 3 * n);
    s.H = s.ang + r4(rows * 3 * n);
    s.nle = s.H + r4(rows * n * n);
    s.X = s.nle + r4(rows * n);
    s.sub = s.X + r4(rows * 6 * n);
    const int64_t a = drm_crba_scratch_floats(tree, rows), c = drm_rnea_scratch_floats(tree, rows);
    s.total = s.sub + r4(a > c ? a : c);
    return s;
}

} // namespace drm

using namespace drm;

static int64_t drm_operational_space_scratch_floats_impl(const drm_walk *tree, const drm_walk *chain, int64_t B, bool aligned) {
    if (check_walk(tree) || check_walk(chain) || B <= 0 || tree->n_dofs != chain->n_dofs) return 0;
    bool same;
    const int64_t lo = osc_fused(tree, chain, B, aligned, same) ? B / WAVE * WAVE : 0;
    if (lo == B) return 0;
    return osc_scratch_layout(tree, B - lo).total;
}
extern "C" int64_t drm_operational_space_scratch_floats(const drm_walk *tree, const drm_walk *chain, int64_t B) {
    return drm_operational_space_scratch_floats_impl(tree, chain, B, false);
}
extern "C" int64_t drm_operational_space_scratch_floats_aligned(const drm_walk *tree, const drm_walk *chain, int64_t B) {
    return drm_operational_space_scratch_floats_impl(tree, chain, B, true);
}

template <int LINKS, int M>
static void launch_osc_arm(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int n_tiles, int flags, float reg2,
                           float *inertia, float *jbar, float *bias_acc, float *bias_force, hipStream_t s) {
    hipLaunchKernelGGL((operational_space_arm_kernel<8, 7, LINKS, M>), dim3((unsigned)n_tiles), dim3(WAVE), 0, s, tree->ops_f, chain->ops_f, q, qd,
                       n_tiles, flags, reg2, inertia, jbar, bias_acc, bias_force);
}

extern "C" int drm_operational_space(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int64_t B, int32_t flags,
                                     float reg, float *inertia, float *jbar, float *bias_acc, float *bias_force, float *scratch,
                                     void *stream) {
    int rc = args_operational_space(tree, chain, q, qd, B, reg, inertia, jbar, bias_acc, bias_force);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n = tree->n_dofs, m = (flags & DRM_OSC_POSITION_ONLY) ? 3 : 6;
    const int dyn_flags = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    const float reg2 = reg * reg;
    if (!bias_acc && !bias_force) qd = nullptr;
    const bool aligned = aligned16(q, qd, inertia, jbar, bias_acc, bias_force, scratch);
    int64_t lo = 0;
    bool same;
    if (!(flags & DRM_OSC_COMPOSED) && osc_fused(tree, chain, B, aligned, same)) {
        const int n_tiles = (int)(B / WAVE);
        const bool links7 = !same || arm_links(tree) == 7;
#define OSC_ARM(L, M) launch_osc_arm<L, M>(tree, chain, q, qd, n_tiles, dyn_flags, reg2, inertia, jbar, bias_acc, bias_force, s)
        if (links7) { if (m == 6) OSC_ARM(7, 6); else OSC_ARM(7, 3); }
        else { if (m == 6) OSC_ARM(8, 6); else OSC_ARM(8, 3); }
#undef OSC_ARM
        rc = launched();
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the composed path over rows [lo, B)
    if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_operational_space_scratch_floats() floats of scratch");
    const int64_t rows = B - lo;
    if (rows / 64 >= GRID_MAX) return fail(DRM_ERR_UNSUPPORTED, "batch too large");
    const OscScratch L = osc_scratch_layout(tree, rows);
    float *qs = scratch + L.qs, *qds = scratch + L.qds, *lin = scratch + L.lin, *ang = scratch + L.ang, *H = scratch + L.H;
    float *nle = scratch + L.nle, *X = scratch + L.X, *sub = scratch + L.sub;
    const float *qr = q + lo * n, *qdr = qd ? qd + lo * n : nullptr;
    const unsigned blocks = (unsigned)((rows + 63) / 64);
    hipLaunchKernelGGL(operational_space_start_kernel, dim3(blocks), dim3(64), 0, s, qr, qdr, rows, n, qs, qds);
    rc = launched();
    if (rc) return rc;
    rc = drm_fk_jacobian(chain, qs, rows, nullptr, nullptr, lin, ang, stream);
    if (rc) return rc;
    rc = drm_crba(tree, qs, rows, H, sub, stream);
    if (rc) return rc;
    if (bias_force) {
        rc = drm_rnea(tree, qs, qds, nullptr, rows, dyn_flags, nle, sub, stream);
        if (rc) return rc;
    }
    const int32_t *w0 = chain->ops_i + DRM_OPI_W0 * chain->capacity;
    auto out = [&](float *p, int64_t width) { return p ? p + lo * width : nullptr; };
    // the rows' H and X in LDS where 64 of them fit, else in the scratch
    const size_t lds = sizeof(float) * 64 * (size_t)((n * n + m * n) | 1);
    const bool in_lds = lds <= (size_t)MAX_LDS_BYTES;
#define OSC_FINISH(M, IN_LDS)                                                                                                            \
    do {                                                                                                                                 \
        if (IN_LDS) rc = ensure_lds(operational_space_finish_kernel<M, IN_LDS>, lds);                                                    \
        if (rc) return rc;                                                                                                               \
        hipLaunchKernelGGL((operational_space_finish_kernel<M, IN_LDS>), dim3(blocks), dim3(64), IN_LDS ? lds : 0, s, qr, qdr,           \
                           (const float *)qds, (const float *)lin, (const float *)ang, H, (const float *)nle, X, w0, (int)chain->n_ops,  \
                           rows, n, reg2, out(inertia, M * M), out(jbar, (int64_t)n * M), out(bias_acc, M), out(bias_force, M));         \
    } while (0)
    if (m == 6) { if (in_lds) OSC_FINISH(6, true); else OSC_FINISH(6, false); }
    else { if (in_lds) OSC_FINISH(3, true); else OSC_FINISH(3, false); }
#undef OSC_FINISH
    return launched();
}

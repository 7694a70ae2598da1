// drm_collision.hip — collision of spheres fixed to the links with a world of spheres and oriented boxes and with each other
// (csrc/drm_collision.hpp): the cost and its q-gradient (drm_collision_cost), the centres and their clearances (drm_sphere_distances),
// each in one call over a many-target FK walk (include/drm_hip.h).  What a caller otherwise composes from the link frames, broadcast
// signed distances with [B, S, M] intermediates in HBM and an autograd pass back through the FK backward kernel, for 28 B in and 32 B
// out per row.  The package's first compute-bound kernel: at S = 48 spheres and 16 obstacles about 800 signed distances per row plus
// the pair list.
//
//   collision_arm_kernel<NW, MODE>   serial 7-DoF arm chains of 8 ops, every op a target in walk order, full 64-row tiles, 16-byte
//                                    aligned pointers, S <= COLL_FUSED_SPHERES, obstacles <= COLL_FUSED_OBSTACLES, pairs <=
//                                    COLL_FUSED_PAIRS.  One row per lane, a BLOCK of NW wavefronts per 64-row tile: every wavefront
//                                    stages nothing of its own but runs the one chain_trig and the one sweep outwards (300 VALU, against
//                                    tens of thousands in the loops), forms the centres of ITS spheres (those whose index within their
//                                    link's group is wave mod NW, so the split does not depend on the groups before) and leaves them in
//                                    LDS for the pair phase, row-major with an odd row stride.  The sphere, obstacle and pair tables are
//                                    read through wave-uniform addresses (scalar loads).  MODE 0, cost: every wavefront adds its world
//                                    terms and its share of the pairs (pair index mod NW) into its OWN (F_l, M_l) accumulators in LDS —
//                                    the gradient of a run of pairs with the same first sphere stays in registers until the run ends —
//                                    wavefront 0 adds the NW partial wrenches and costs in wave order and runs the one sweep inwards with
//                                    p_l, z_l still in its registers; the [64, 7] and [64] tiles leave through LDS in 16-byte stores.
//                                    With dq NULL neither accumulators nor sweep exist.  MODE 1, distances: the least clearances in
//                                    [64, S] LDS tiles (one self-distance tile per wavefront, merged by min, which is exact), and the
//                                    [64, 3 S] and [64, S] tiles leave in 16-byte stores by the whole block.
//   collision_walk_rows_kernel, collision_pairs_rows_kernel
//                                    every other walk (trees, hands, prismatic and skew joints, link subsets), ragged tails, misaligned
//                                    pointers, anything over the caps, DRM_LINKS_COMPOSED: one lane per row.  Kernel 1 walks outwards
//                                    (drm_links.hpp link_motion_walk, positions only), evaluates each target's spheres against the
//                                    world and writes centres, link origins, the per-link (F, M) and the cost of its row to the scratch;
//                                    kernel 2 loops over the pairs and adds to them (and gives unusable rows their NaN);
//                                    drm_external_torques then produces dq.  No new inward tree walk.
//
// Order of every sum: spheres in grouped order against the obstacles in table order, spheres before boxes, then the pairs in list
// order.  The fused kernel splits that order over its wavefronts and adds the partial sums in wave order: the two paths agree to
// rounding, and each is the same from launch to launch.
//
// LDS of a fused block (floats): table 256 + link ids S + centres 64 (3 S | 1); cost mode + origins 1 536 + NW 64 + 448 + 64 and, with
// dq, NW 3 072 accumulators; distances mode + (1 + NW) 64 (S | 1).  At S = 48, NW = 4: 94 KiB with dq (one block of four wavefronts
// per CU), 46 KiB for the cost alone.  One wavefront per tile (a build with -DDRM_COLL_WAVES=1) needs 58 KiB: two blocks, two
// wavefronts per CU.
//
// Compiler's kernel-resource-usage remarks (gfx950, the flags of this unit; profiles/collision_resource_usage.txt); LDS is dynamic:
//   collision_arm_kernel<4, 0>            VGPRs 128  spills 0  scratch 0  occupancy by registers 4 waves / SIMD
//   collision_arm_kernel<4, 1>            VGPRs 65   spills 0  scratch 0
//   (one wavefront per tile, -DDRM_COLL_WAVES=1: <1, 0> VGPRs 129, occupancy 3; <1, 1> VGPRs 64; no spills, no scratch)
//   collision_walk_rows_kernel            VGPRs 83 - 97  spills 0  scratch 0;   collision_pairs_rows_kernel  VGPRs 40 / 32
// Measured on an MI355X (profiles/collision_bench.txt), Panda, 48 spheres, 16 obstacles, 720 pairs, 65 536 rows, kernel time: cost and
// gradient 692 us with four wavefronts per tile against 1 059 us with one (cost alone 256 / 781, distances 390 / 594): four are kept.
// 26 363 VALU instructions per wavefront: an issue floor of 88 us; one block per CU with the gradient, so occupancy binds.
#include <math.h>

#include "drm_common.hpp"
#include "drm_collision.hpp"
#include "drm_dispatch.hpp"
#include "drm_links.hpp"
#include "drm_rows.hpp"
#include "drm_args.hpp"

namespace drm {

// wavefronts per 64-row tile of the fused kernel (its caps: drm_collision.hpp).  A power of two; a build with -DDRM_COLL_WAVES=1 is
// the one wavefront per tile that the header comment's measurement compares against.
#ifndef DRM_COLL_WAVES
#define DRM_COLL_WAVES 4
#endif
constexpr int COLL_WAVES = DRM_COLL_WAVES;
constexpr int COLL_LDS_BYTES = 32 * 1024; // the parked states of the general walk in LDS up to here (drm_links.hip)

// the tables of a call, as kernel arguments
struct CollArgs {
    const float *sph;
    const int32_t *start;
    int S;
    const float *ws, *wb;
    int n_ws, n_wb;
    const int32_t *pairs;
    int P;
    CollLaw world, self;
};

constexpr int COLL_ARM_LINKS = 8, COLL_ARM_NJ = 7;
constexpr int COLL_ORG_FLOATS = COLL_ARM_LINKS * 3 * WAVE, COLL_ACC_FLOATS = COLL_ARM_LINKS * 6 * WAVE;
constexpr int COLL_TQ_FLOATS = round4(WAVE * COLL_ARM_NJ);
static inline size_t coll_arm_lds_floats(int nw, int mode, int S, bool want_dq) {
    size_t f = (size_t)COLL_ARM_LINKS * DRM_OPF_STRIDE + round4(S) + round4(WAVE * ((3 * S) | 1));
    if (mode == 0) f += COLL_ORG_FLOATS + nw * WAVE + COLL_TQ_FLOATS + WAVE + (want_dq ? (size_t)nw * COLL_ACC_FLOATS : 0);
    else f += (size_t)(1 + nw) * round4(WAVE * (S | 1));
    return f;
}

// MODE 0: o0 = cost [B], o1 = dq [B, 7] (either NULL, wave-uniform).  MODE 1: o0 = center [B, S, 3], o1 = world_distance [B, S],
// o2 = self_distance [B, S].  magic3 / magic1: div_magic(3 S) / div_magic(S) of the tile stores.
template <int NW, int MODE>
__global__ void __launch_bounds__(WAVE *NW)
    collision_arm_kernel(const float *__restrict__ ops_f, const float *__restrict__ q, int n_tiles, CollArgs a, uint32_t magic3,
                         uint32_t magic1, float *__restrict__ o0, float *__restrict__ o1, float *__restrict__ o2) {
    constexpr int NJ = COLL_ARM_NJ, LINKS = COLL_ARM_LINKS, C_FLOATS = LINKS * DRM_OPF_STRIDE;
    static_assert(C_FLOATS == 4 * WAVE, "one float4 per lane copies the constant table");
    static_assert((NW & (NW - 1)) == 0, "a power of two");
    extern __shared__ __attribute__((aligned(16))) float coll_lds[];
    const int tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned lane = threadIdx.x & 63u;
    const int S = a.S, CP = (3 * S) | 1, SP = S | 1;
    float *lc = coll_lds;
    int *llink = reinterpret_cast<int *>(lc + C_FLOATS);
    float *cen = lc + C_FLOATS + round4(S), *rest = cen + round4(WAVE * CP);
    const int64_t b0 = (int64_t)tile * WAVE;
    const float nan = __builtin_nanf("");

    if (wave == 0) reinterpret_cast<float4 *>(lc)[lane] = reinterpret_cast<const float4 *>(ops_f)[lane];
    for (int s = (int)threadIdx.x; s < S; s += WAVE * NW) llink[s] = coll_group_of(a.start, LINKS + 1, s);
    float qv[NJ];
    {
        const int64_t r0 = (b0 + lane) * NJ;
#pragma unroll
        for (int d = 0; d < NJ; ++d) qv[d] = q[r0 + d];
    }
    int st[LINKS + 2];
#pragma unroll
    for (int i = 0; i < LINKS + 2; ++i) st[i] = a.start[i];
    __syncthreads();
    auto row = [&](int k) -> const float * { return lc + k * DRM_OPF_STRIDE; };
    auto link_of = [&](int s) { return __builtin_amdgcn_readfirstlane(llink[s]); };

    // a row that cannot be used walks the chain at q = 0 and gets NaN outputs (drm_links.hip)
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NJ; ++d) bad = bad || lag_bad_input(qv[d], 0.0f);
#pragma unroll
    for (int d = 0; d < NJ; ++d) qv[d] = bad ? 0.0f : qv[d];
    float cs[NJ], sn[NJ];
    chain_trig<NJ>(qv, cs, sn);

    // the sweep outwards: the centres of this wavefront's spheres to LDS; origins and axes stay in registers for the sweep inwards
    float *org = rest; // MODE 0: [LINKS][3][64]
    float p[LINKS][3], z[NJ][3];
    float *crow = cen + lane * CP;
    for (int s = st[0] + wave; s < st[1]; s += NW) {
        const float *c = a.sph + COLL_SPHERE_FLOATS * s;
        crow[3 * s] = c[0]; crow[3 * s + 1] = c[1]; crow[3 * s + 2] = c[2];
    }
    {
        LinkState cur;
        link_state_root(cur);
#pragma unroll
        for (int k = 0; k < LINKS; ++k) {
            const OpFT o = load_ft(row(k));
            float J[9], t[3];
            link_joint_transform(o, k < NJ, false, 0.0f, k < NJ ? cs[k] : 1.0f, k < NJ ? sn[k] : 0.0f, J, t);
            link_step<false, false>(J, t, k < NJ, false, 0.0f, 0.0f, cur);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                p[k][i] = cur.p[i];
                if (k < NJ) z[k < NJ ? k : 0][i] = cur.R[3 * i + 2];
                if (MODE == 0 && wave == 0) org[(k * 3 + i) * WAVE + lane] = cur.p[i];
            }
#pragma unroll 1
            for (int s = st[k + 1] + wave; s < st[k + 2]; s += NW) {
                const float *c = a.sph + COLL_SPHERE_FLOATS * s;
                float x[3];
                coll_centre(cur.R, cur.p, c[0], c[1], c[2], x);
                crow[3 * s] = x[0]; crow[3 * s + 1] = x[1]; crow[3 * s + 2] = x[2];
            }
        }
    }
    __syncthreads(); // the origins (wavefront 0 wrote them) before the accumulators use them

    if constexpr (MODE == 0) {
        float *costp = org + COLL_ORG_FLOATS, *tq = costp + NW * WAVE, *tc = tq + COLL_TQ_FLOATS, *acc = tc + WAVE;
        const bool want_dq = o1 != nullptr;
        float *mine = acc + wave * COLL_ACC_FLOATS + lane;
        // (F, M) of link l (0 .. LINKS - 1) += the wrench of g on a sphere at x
        auto acc_add = [&](int l, const float *x, const float *g) {
            float *f = mine + l * 6 * WAVE;
            const float *pl = org + l * 3 * WAVE + lane;
            const float po[3] = {pl[0], pl[WAVE], pl[2 * WAVE]};
            float F[3] = {f[0], f[WAVE], f[2 * WAVE]}, M[3] = {f[3 * WAVE], f[4 * WAVE], f[5 * WAVE]};
            coll_wrench_add(x, po, g, F, M);
#pragma unroll
            for (int i = 0; i < 3; ++i) { f[i * WAVE] = F[i]; f[(3 + i) * WAVE] = M[i]; }
        };
        if (want_dq) {
#pragma unroll 1
            for (int i = 0; i < LINKS * 6; ++i) mine[i * WAVE] = 0.0f;
        }
        float cost = 0.0f;
        if (a.n_ws + a.n_wb > 0) {
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                const int l = link_of(s);
                if ((s - a.start[l] - wave) & (NW - 1)) continue; // (not this wavefront's)
                const float x[3] = {crow[3 * s], crow[3 * s + 1], crow[3 * s + 2]};
                float g[3] = {0.0f, 0.0f, 0.0f};
                coll_world_sphere<true>(x, a.sph[COLL_SPHERE_FLOATS * s + 3], a.ws, a.n_ws, a.wb, a.n_wb, a.world, cost, g);
                if (want_dq && l > 0) acc_add(l - 1, x, g);
            }
        }
        if (a.P > 0) {
            __syncthreads(); // every wavefront's centres
            int ci = -1, li = 0;
            float xi[3] = {0.0f, 0.0f, 0.0f}, gi[3] = {0.0f, 0.0f, 0.0f}, ri = 0.0f;
#pragma unroll 1
            for (int k = wave; k < a.P; k += NW) {
                const int i = a.pairs[2 * k], j = a.pairs[2 * k + 1];
                if (i != ci) {
                    if (want_dq && ci >= 0 && li > 0) acc_add(li - 1, xi, gi);
                    ci = i;
                    li = link_of(i);
                    ri = a.sph[COLL_SPHERE_FLOATS * i + 3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { xi[c] = crow[3 * i + c]; gi[c] = 0.0f; }
                }
                const float xj[3] = {crow[3 * j], crow[3 * j + 1], crow[3 * j + 2]};
                float n[3], phi, dphi;
                const float d = coll_pair_distance(xi, xj, ri, a.sph[COLL_SPHERE_FLOATS * j + 3], n);
                coll_phi(a.self, d, phi, dphi);
                cost = __builtin_fmaf(a.self.w, phi, cost);
                if (want_dq) {
                    const float s = a.self.w * dphi;
                    const float gj[3] = {s * n[0], s * n[1], s * n[2]};
#pragma unroll
                    for (int c = 0; c < 3; ++c) gi[c] -= gj[c];
                    const int lj = link_of(j);
                    if (lj > 0) acc_add(lj - 1, xj, gj);
                }
            }
            if (want_dq && ci >= 0 && li > 0) acc_add(li - 1, xi, gi);
        }
        costp[wave * WAVE + lane] = cost;
        __syncthreads();
        if (wave != 0) return;
        if (o0) {
            float c = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) c += costp[w * WAVE + lane];
            tc[lane] = bad ? nan : c;
        }
        if (want_dq) {
            float Fc[3] = {0.0f, 0.0f, 0.0f}, Mc[3] = {0.0f, 0.0f, 0.0f}; // what op k + 1 hands up, about op k's origin
#pragma unroll
            for (int k = LINKS - 1; k >= 0; --k) {
                float F[3] = {0.0f, 0.0f, 0.0f}, M[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const float *f = acc + w * COLL_ACC_FLOATS + k * 6 * WAVE + lane;
#pragma unroll
                    for (int i = 0; i < 3; ++i) { F[i] += f[i * WAVE]; M[i] += f[(3 + i) * WAVE]; }
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) { F[i] += Fc[i]; M[i] += Mc[i]; }
                if (k < NJ) tq[lane * NJ + (k < NJ ? k : 0)] = bad ? nan : link_joint_torque(z[k < NJ ? k : 0], F, M, false);
                if (k > 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) { Fc[i] = 0.0f; Mc[i] = 0.0f; }
                    link_wrench_up(p[k], p[k > 0 ? k - 1 : 0], F, M, Fc, Mc);
                }
            }
        }
        wave_lds_sync();
        if (want_dq) tile_store<NJ>(o1 + b0 * NJ, WAVE, NJ, 0u, tq, lane, true);
        if (o0 && lane < 16u) store16_wt(o0 + b0 + 4 * lane, reinterpret_cast<const float4 *>(tc)[lane]);
    } else {
        const int SD_FLOATS = round4(WAVE * SP);
        float *wd = rest, *sd = wd + SD_FLOATS;
        const float inf = INFINITY;
        if (o1) {
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                const int l = link_of(s);
                if ((s - a.start[l] - wave) & (NW - 1)) continue; // (not this wavefront's)
                const float x[3] = {crow[3 * s], crow[3 * s + 1], crow[3 * s + 2]};
                float unused = 0.0f, g[3];
                wd[lane * SP + s] = coll_world_sphere<false>(x, a.sph[COLL_SPHERE_FLOATS * s + 3], a.ws, a.n_ws, a.wb, a.n_wb, a.world, unused, g);
            }
        }
        if (o2) {
            float *mine = sd + wave * SD_FLOATS + lane * SP;
#pragma unroll 1
            for (int s = 0; s < S; ++s) mine[s] = inf;
            __syncthreads(); // every wavefront's centres
            int ci = -1;
            float xi[3] = {0.0f, 0.0f, 0.0f}, ri = 0.0f, di = inf;
#pragma unroll 1
            for (int k = wave; k < a.P; k += NW) {
                const int i = a.pairs[2 * k], j = a.pairs[2 * k + 1];
                if (i != ci) {
                    if (ci >= 0) mine[ci] = fminf(mine[ci], di);
                    ci = i;
                    ri = a.sph[COLL_SPHERE_FLOATS * i + 3];
                    di = inf;
#pragma unroll
                    for (int c = 0; c < 3; ++c) xi[c] = crow[3 * i + c];
                }
                const float xj[3] = {crow[3 * j], crow[3 * j + 1], crow[3 * j + 2]};
                float n[3];
                const float d = coll_pair_distance(xi, xj, ri, a.sph[COLL_SPHERE_FLOATS * j + 3], n);
                di = fminf(di, d);
                mine[j] = fminf(mine[j], d);
            }
            if (ci >= 0) mine[ci] = fminf(mine[ci], di);
            if (NW > 1) {
                __syncthreads();
                for (int i = (int)threadIdx.x; i < WAVE * SP; i += WAVE * NW) {
                    float m = sd[i];
#pragma unroll
                    for (int w = 1; w < NW; ++w) m = fminf(m, sd[w * SD_FLOATS + i]);
                    sd[i] = m;
                }
            }
        }
        __syncthreads();
        if (wave == 0 && bad) {
#pragma unroll 1
            for (int c = 0; c < 3 * S; ++c) crow[c] = nan;
#pragma unroll 1
            for (int s = 0; s < S; ++s) { wd[lane * SP + s] = nan; sd[lane * SP + s] = nan; }
        }
        __syncthreads();
        if (o0) block_tile_store(o0 + b0 * 3 * S, WAVE, 3 * S, magic3, cen, true);
        if (o1) block_tile_store(o1 + b0 * S, WAVE, S, magic1, wd, true);
        if (o2) block_tile_store(o2 + b0 * S, WAVE, S, magic1, sd, true);
    }
}

// The general kernels.  Rows [0, B) in tiles of 64, one lane per row; blocks stride over the tiles; the parked states of the walk:
// drm_rows.hpp rows_state.  Kernel 1: the walk outwards with the world terms.  MODE 0: cen [B, S, 3], org / F / M [B, T, 3] (NULL
// when no gradient is wanted) and cost [B] get the row's centres, link origins, wrenches and world cost.  MODE 1: cen and, unless
// NULL, wd [B, S] the least world clearances.
template <bool IN_LDS, int MODE>
__global__ void __launch_bounds__(WAVE)
    collision_walk_rows_kernel(const float *__restrict__ ops_f, const int32_t *__restrict__ ops_i, int cap, int n_ops, int n_slots, int n, int T,
                               const float *__restrict__ q, int64_t B, int64_t n_tiles, CollArgs a, float *__restrict__ cen,
                               float *__restrict__ org, float *__restrict__ F, float *__restrict__ M, float *__restrict__ cost,
                               float *__restrict__ wd, float *__restrict__ scratch, int state_floats) {
    const unsigned lane = threadIdx.x & 63u;
    float *state = rows_state<IN_LDS>(scratch, state_floats);
    const Records<LINKS_SLOT_FLOATS, WAVE> slots = {state};
    const RowsCtl ctl(ops_i, cap);
    const int S = a.S;
    auto row = [&](int k) -> const float * { return ops_f + k * DRM_OPF_STRIDE; };
#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * WAVE + lane;
        if (r >= B) continue; // (a lane shares nothing with its neighbours: no barrier below)
        const float *qr = q + r * n;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || lag_bad_input(qr[d], 0.0f);
        float *cr = cen + r * S * 3;
        float c = 0.0f;
        // one sphere of a group whose frame is (R, p): its centre, its world terms; returns the least clearance
        auto sphere = [&](int s, const float *R, const float *p, float *g, float *x) {
            const float *t = a.sph + COLL_SPHERE_FLOATS * s;
            coll_centre(R, p, t[0], t[1], t[2], x);
            cr[3 * s] = x[0]; cr[3 * s + 1] = x[1]; cr[3 * s + 2] = x[2];
            const float least = coll_world_sphere<MODE == 0>(x, t[3], a.ws, a.n_ws, a.wb, a.n_wb, a.world, c, g);
            if (MODE == 1 && wd) wd[r * S + s] = least;
            return least;
        };
        {
            const float I[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, o[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
            for (int s = a.start[0]; s < a.start[1]; ++s) {
                float g[3] = {0.0f, 0.0f, 0.0f}, x[3];
                sphere(s, I, o, g, x);
            }
        }
        link_motion_walk<false, false>(
            n_ops, n_slots, ctl, row,
            [&](int d, float &x, float &v, float &acc) {
                x = bad ? 0.0f : qr[d];
                v = 0.0f;
                acc = 0.0f;
            },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int t, const LinkState &st) {
                if (t >= T) return;
                float Fl[3] = {0.0f, 0.0f, 0.0f}, Ml[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (int s = a.start[t + 1]; s < a.start[t + 2]; ++s) {
                    float g[3] = {0.0f, 0.0f, 0.0f}, x[3];
                    sphere(s, st.R, st.p, g, x);
                    if (MODE == 0) coll_wrench_add(x, st.p, g, Fl, Ml);
                }
                if (MODE == 0 && F) {
                    const int64_t at = (r * T + t) * 3;
#pragma unroll
                    for (int i = 0; i < 3; ++i) { org[at + i] = st.p[i]; F[at + i] = Fl[i]; M[at + i] = Ml[i]; }
                }
            });
        if (MODE == 0) cost[r] = c;
    }
}

// Kernel 2, one thread per row: the pairs in list order on kernel 1's centres, added to its cost and wrenches (MODE 0) or taken as
// the least self clearances sd [B, S] (MODE 1, NULL: not wanted); then NaN in every output of a row whose q cannot be used
// (nan_cen: the centres are an output too).
template <int MODE>
__global__ void __launch_bounds__(WAVE)
    collision_pairs_rows_kernel(const float *__restrict__ q, int n, int64_t B, int T, CollArgs a, float *__restrict__ cen,
                                const float *__restrict__ org, float *__restrict__ F, float *__restrict__ M, float *__restrict__ cost,
                                float *__restrict__ wd, float *__restrict__ sd, int nan_cen) {
    const float nan = __builtin_nanf("");
    const int S = a.S;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < B; r += (int64_t)gridDim.x * blockDim.x) {
        const float *qr = q + r * n;
        bool bad = false;
#pragma unroll 1
        for (int d = 0; d < n; ++d) bad = bad || lag_bad_input(qr[d], 0.0f);
        float *cr = cen + r * S * 3;
        float c = MODE == 0 ? cost[r] : 0.0f;
        if (MODE == 1 && sd) {
#pragma unroll 1
            for (int s = 0; s < S; ++s) sd[r * S + s] = INFINITY;
        }
        if (MODE == 0 || sd) {
#pragma unroll 1
            for (int k = 0; k < a.P; ++k) {
                const int i = a.pairs[2 * k], j = a.pairs[2 * k + 1];
                const float xi[3] = {cr[3 * i], cr[3 * i + 1], cr[3 * i + 2]}, xj[3] = {cr[3 * j], cr[3 * j + 1], cr[3 * j + 2]};
                float nrm[3], phi, dphi;
                const float d = coll_pair_distance(xi, xj, a.sph[COLL_SPHERE_FLOATS * i + 3], a.sph[COLL_SPHERE_FLOATS * j + 3], nrm);
                if (MODE == 1) {
                    sd[r * S + i] = fminf(sd[r * S + i], d);
                    sd[r * S + j] = fminf(sd[r * S + j], d);
                    continue;
                }
                coll_phi(a.self, d, phi, dphi);
                c = __builtin_fmaf(a.self.w, phi, c);
                if (F) {
                    const float s = a.self.w * dphi;
                    const float gi[3] = {-(s * nrm[0]), -(s * nrm[1]), -(s * nrm[2])}, gj[3] = {s * nrm[0], s * nrm[1], s * nrm[2]};
                    const int li = coll_group_of(a.start, T + 1, i), lj = coll_group_of(a.start, T + 1, j);
                    auto add = [&](int l, const float *x, const float *g) {
                        const int64_t at = (r * T + l) * 3;
                        const float po[3] = {org[at], org[at + 1], org[at + 2]};
                        float Fl[3] = {F[at], F[at + 1], F[at + 2]}, Ml[3] = {M[at], M[at + 1], M[at + 2]};
                        coll_wrench_add(x, po, g, Fl, Ml);
#pragma unroll
                        for (int u = 0; u < 3; ++u) { F[at + u] = Fl[u]; M[at + u] = Ml[u]; }
                    };
                    if (li) add(li - 1, xi, gi);
                    if (lj) add(lj - 1, xj, gj);
                }
            }
        }
        if (MODE == 0) cost[r] = bad ? nan : c;
        if (MODE == 1 && bad) {
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                if (wd) wd[r * S + s] = nan;
                if (sd) sd[r * S + s] = nan;
                if (nan_cen) { cr[3 * s] = nan; cr[3 * s + 1] = nan; cr[3 * s + 2] = nan; }
            }
        }
    }
}

static inline int64_t coll_r4(int64_t x) { return (x + 3) & ~(int64_t)3; }
static inline int coll_state_floats(const drm_walk *w) { return LINKS_SLOT_FLOATS * (w->n_slots > 0 ? w->n_slots : 1); }

// the scratch of the general path over `rows` rows of T targets: [ centres ][ origins ][ F ][ M ][ cost ][ walk state / torques ]
struct CollScratch {
    int64_t cen, link, cost, sub, total;
};
static CollScratch coll_scratch_plan(const drm_walk *w, int64_t rows, int T, int S) {
    CollScratch p;
    p.cen = coll_r4(rows * S * 3);
    p.link = coll_r4(rows * T * 3);
    p.cost = coll_r4(rows);
    const int64_t walk = rows_plan(rows, coll_state_floats(w), COLL_LDS_BYTES).scratch_floats;
    const int64_t torques = drm_external_torques_scratch_floats(w, rows);
    p.sub = coll_r4(walk > torques ? walk : torques);
    p.total = p.cen + 3 * p.link + p.cost + p.sub;
    return p;
}

// the checked tables of a call (drm_args.hpp args_collision) as the kernels take them
static CollArgs coll_args(const CollTables &t) { return CollArgs{t.spheres, t.start, t.S, t.ws, t.wb, t.n_ws, t.n_wb, t.pairs, t.P, t.world, t.self}; }

// an arm7_walk of 8 ops whose every op is a target, slots in walk order (drm_links.hip links_fused), and tables within the caps
static inline bool coll_fused(const drm_walk *w, int T, int64_t B, int flags, bool aligned, const CollArgs &a) {
    return !(flags & DRM_LINKS_COMPOSED) && (w->shape & DRM_WALK_TARGETS_ORDERED) && w->n_ops == 8 && T == 8 && rows_fused(w, B, aligned) &&
           coll_within_caps(a.S, a.n_ws + a.n_wb, a.P);
}

template <int MODE>
static int coll_launch_fused(const drm_walk *w, const float *q, int n_tiles, const CollArgs &a, float *o0, float *o1, float *o2, hipStream_t s) {
    const size_t lds = sizeof(float) * coll_arm_lds_floats(COLL_WAVES, MODE, a.S, MODE == 0 && o1 != nullptr);
    if (lds > (size_t)MAX_LDS_BYTES) return fail(DRM_ERR_UNSUPPORTED, "the fused collision kernel's LDS");
    int rc = ensure_lds(collision_arm_kernel<COLL_WAVES, MODE>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((collision_arm_kernel<COLL_WAVES, MODE>), dim3((unsigned)n_tiles), dim3(WAVE * COLL_WAVES), lds, s, w->ops_f, q, n_tiles, a,
                       div_magic(3 * a.S), div_magic(a.S), o0, o1, o2);
    return launched();
}

static inline unsigned coll_row_blocks(int64_t rows) {
    const int64_t b = (rows + WAVE - 1) / WAVE;
    return (unsigned)(b < 8192 ? (b < 1 ? 1 : b) : 8192);
}

// kernel 1 over `rows` rows (all pointers at the first of them)
template <int MODE>
static int coll_launch_walk(const drm_walk *w, const float *q, int64_t rows, int T, const CollArgs &a, float *cen, float *org, float *F, float *M,
                            float *cost, float *wd, float *sub, const char *query, hipStream_t s) {
    const RowsPlan plan = rows_plan(rows, coll_state_floats(w), COLL_LDS_BYTES);
    return rows_launch(collision_walk_rows_kernel<true, MODE>, collision_walk_rows_kernel<false, MODE>, plan, sub, query, s, w->ops_f, w->ops_i,
                       (int)w->capacity, (int)w->n_ops, (int)w->n_slots, (int)w->n_dofs, T, q, rows, plan.tiles, a, cen, org, F, M, cost, wd);
}

} // namespace drm

using namespace drm;

// The general path over ALL B rows, whatever the alignment, the targets and the caps (drm_links.hip links_scratch).
static int64_t coll_query(const drm_walk *w, int64_t B, int32_t S) {
    if (check_sweep_walk(w) || B <= 0 || S < 1) return 0;
    return coll_scratch_plan(w, B, w->n_ops, S).total;
}
// The same for a call without DRM_LINKS_COMPOSED whose pointers are all 16-byte aligned, of which the query is told what else
// decides whether the fused kernel takes the full tiles (coll_fused): then only the tail of B % 64 rows is left to the general path.
static int64_t coll_query_aligned(const drm_walk *w, int64_t B, int32_t T, int32_t S, int32_t n_obstacles, int32_t n_pairs) {
    if (check_sweep_walk(w) || B <= 0 || S < 1) return 0;
    if (T < 1 || T > w->n_ops || n_obstacles < 0 || n_pairs < 0) return coll_query(w, B, S);
    CollArgs a{};
    a.S = S;
    a.n_ws = n_obstacles;
    a.P = n_pairs;
    if (!coll_fused(w, T, B, 0, true, a)) return coll_scratch_plan(w, B, T, S).total;
    const int64_t rows = B % WAVE;
    return rows ? coll_scratch_plan(w, rows, T, S).total : 0;
}
extern "C" int64_t drm_collision_cost_scratch_floats(const drm_walk *w, int64_t B, int32_t S) { return coll_query(w, B, S); }
extern "C" int64_t drm_collision_cost_scratch_floats_aligned(const drm_walk *w, int64_t B, int32_t T, int32_t S, int32_t n_obstacles,
                                                             int32_t n_pairs) {
    return coll_query_aligned(w, B, T, S, n_obstacles, n_pairs);
}
extern "C" int64_t drm_sphere_distances_scratch_floats(const drm_walk *w, int64_t B, int32_t S) { return coll_query(w, B, S); }
extern "C" int64_t drm_sphere_distances_scratch_floats_aligned(const drm_walk *w, int64_t B, int32_t T, int32_t S, int32_t n_obstacles,
                                                               int32_t n_pairs) {
    return coll_query_aligned(w, B, T, S, n_obstacles, n_pairs);
}

extern "C" int drm_collision_cost(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const drm_collision_spheres *spheres,
                                  const drm_collision_world *world, const drm_collision_pairs *pairs, const drm_collision_params *params,
                                  int32_t flags, float *cost, float *dq, float *scratch, void *stream) {
    CollTables tables;
    int rc = args_collision_cost(w, q, B, n_targets, spheres, world, pairs, params, cost, dq, tables);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    const CollArgs a = coll_args(tables);
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs, T = n_targets;
    int64_t lo = 0;
    if (coll_fused(w, T, B, flags, aligned16(q, cost, dq), a)) {
        const int n_tiles = (int)(B / WAVE);
        rc = coll_launch_fused<0>(w, q, n_tiles, a, cost, dq, nullptr, s);
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    // the general path over rows [lo, B)
    if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_collision_cost_scratch_floats() floats of scratch");
    const int64_t rows = B - lo;
    const CollScratch plan = coll_scratch_plan(w, rows, T, a.S);
    float *cen = scratch, *org = cen + plan.cen, *F = org + plan.link, *M = F + plan.link, *cbuf = M + plan.link, *sub = cbuf + plan.cost;
    float *co = cost ? cost + lo : cbuf;
    if (!dq) org = F = M = nullptr;
    rc = coll_launch_walk<0>(w, q + lo * n, rows, T, a, cen, org, F, M, co, nullptr, sub, "drm_collision_cost_scratch_floats", s);
    if (rc) return rc;
    hipLaunchKernelGGL(collision_pairs_rows_kernel<0>, dim3(coll_row_blocks(rows)), dim3(WAVE), 0, s, q + lo * n, n, rows, T, a, cen,
                       (const float *)org, F, M, co, (float *)nullptr, (float *)nullptr, 0);
    rc = launched();
    if (rc || !dq) return rc;
    return drm_external_torques(w, q + lo * n, F, M, rows, T, flags & DRM_LINKS_COMPOSED, dq + lo * n, sub, s);
}

extern "C" int drm_sphere_distances(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const drm_collision_spheres *spheres,
                                    const drm_collision_world *world, const drm_collision_pairs *pairs, int32_t flags, float *center,
                                    float *world_distance, float *self_distance, float *scratch, void *stream) {
    CollTables tables;
    int rc = args_sphere_distances(w, q, B, n_targets, spheres, world, pairs, center, world_distance, self_distance, tables);
    if (rc) return rc;
    if (B == 0) return DRM_OK;
    const CollArgs a = coll_args(tables);
    hipStream_t s = (hipStream_t)stream;
    const int n = w->n_dofs, T = n_targets, S = a.S;
    int64_t lo = 0;
    if (coll_fused(w, T, B, flags, aligned16(q, center, world_distance, self_distance), a)) {
        const int n_tiles = (int)(B / WAVE);
        rc = coll_launch_fused<1>(w, q, n_tiles, a, center, world_distance, self_distance, s);
        if (rc) return rc;
        lo = (int64_t)n_tiles * WAVE;
        if (lo == B) return DRM_OK;
    }
    if (!scratch) return fail(DRM_ERR_INVALID, "pass drm_sphere_distances_scratch_floats() floats of scratch");
    const int64_t rows = B - lo;
    const CollScratch plan = coll_scratch_plan(w, rows, T, S);
    float *cen = center ? center + lo * S * 3 : scratch, *sub = scratch + plan.cen + 3 * plan.link + plan.cost;
    float *wd = world_distance ? world_distance + lo * S : nullptr, *sd = self_distance ? self_distance + lo * S : nullptr;
    rc = coll_launch_walk<1>(w, q + lo * n, rows, T, a, cen, nullptr, nullptr, nullptr, nullptr, wd, sub, "drm_sphere_distances_scratch_floats", s);
    if (rc) return rc;
    hipLaunchKernelGGL(collision_pairs_rows_kernel<1>, dim3(coll_row_blocks(rows)), dim3(WAVE), 0, s, q + lo * n, n, rows, T, a, cen,
                       (const float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, wd, sd, center ? 1 : 0);
    return launched();
}

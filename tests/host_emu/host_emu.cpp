// TEST INFRASTRUCTURE ONLY — never loaded by the product package (the generic per-sample loops it shares with the host build of
// the C ABI, csrc/drm_cpu.cpp, live in csrc/drm_host_loops.hpp; the shape-specialised variants below exist only here).
//
// Compiles the per-sample arithmetic of the HIP kernels (csrc/drm_sample.hpp)
// with g++ and runs it one sample at a time over HOST arrays, so that the
// kernel arithmetic and the walk encoding can be checked against the oracle
// in the GPU-less build container.  The tile I/O and launch code of
// drm_kernels.hip are NOT covered here; the `-m gpu` tests cover the real thing.
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../differentiable-robot-model_amd/csrc/drm_host_loops.hpp"   // the generic walks (shared with the host build of the C ABI)

using namespace drm;
using namespace drm_host;

namespace {
// packed-FP32 chain arithmetic of the arm kernel (fk_jacobian_arm_kernel<8, 7>)
void jac_arm_8_7(const drm_walk *w, const float *q, int64_t B, float *pos, float *quat, float *lin, float *ang) {
    constexpr int CAP = 8, NJ = 7;
    for (int64_t b = 0; b < B; ++b) {
        float qv[NJ];
        for (int d = 0; d < NJ; ++d) qv[d] = q[b * NJ + d];
        PoseP ee;
        f2 Bk[NJ][3];
        fk_chain_pairs<CAP, NJ>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, qv, ee, Bk, [] {});
        Pose E;
        pose_from_pairs(ee, E);
        for (int i = 0; i < 3; ++i) pos[b * 3 + i] = E.p[i];
        unpermute(w->target_perm, E.R);
        quat_xyzw(E.R, quat + b * 4);
        for (int k = 0; k < NJ; ++k) {
            const float z[3] = {Bk[k][0][0], Bk[k][1][0], Bk[k][2][0]};
            const float dp[3] = {E.p[0] - Bk[k][0][1], E.p[1] - Bk[k][1][1], E.p[2] - Bk[k][2][1]};
            float c[3];
            cross3(z, dp, c);
            for (int r = 0; r < 3; ++r) { lin[(b * 3 + r) * NJ + k] = c[r]; ang[(b * 3 + r) * NJ + k] = z[r]; }
        }
    }
}

// the arithmetic of rnea_arm_kernel<8, 7, LINKS>: LINKS = 8 (whole table) or 7 (tail folded: the sweeps stop at the last joint)
template <int LINKS>
void rnea_arm_8_7(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int flags, float *tau) {
    constexpr int NJ = 7;
    for (int64_t b = 0; b < B; ++b) {
        float qv[NJ], qdv[NJ], qddv[NJ], tv[NJ];
        for (int d = 0; d < NJ; ++d) { qv[d] = q[b * NJ + d]; qdv[d] = qd[b * NJ + d]; qddv[d] = qdd ? qdd[b * NJ + d] : 0.f; }
        Force park[LINKS];
        rnea_chain<LINKS, NJ>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, flags & DRM_RNEA_GRAVITY,
                              flags & DRM_RNEA_DAMPING, qv, qdv, qddv, tv, [&](int k, const Force &F) { park[k] = F; },
                              [&](int k, Force &F) { F = park[k]; });
        for (int d = 0; d < NJ; ++d) tau[b * NJ + d] = tv[d];
    }
}

// the arithmetic of fk_rnea_arm_kernel<8, 7, LINKS>: one sin / cos evaluation; the pose chain walks all 8 rows — rows 0 .. LINKS-1 of
// the TREE walk's table, the fixed tail behind them from the CHAIN walk's — then the sweeps of rnea_arm_kernel on the first LINKS
template <int LINKS>
void fk_rnea_arm_8_7(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, const float *qdd, int64_t B, int flags,
                     float *tau, float *pos, float *quat) {
    constexpr int CAP = 8, NJ = 7;
    auto row = [&](int k) { return (k < LINKS ? tree->ops_f : chain->ops_f) + k * DRM_OPF_STRIDE; };
    for (int64_t b = 0; b < B; ++b) {
        float qv[NJ], qdv[NJ], qddv[NJ], tv[NJ], cs[NJ], sn[NJ];
        for (int d = 0; d < NJ; ++d) { qv[d] = q[b * NJ + d]; qdv[d] = qd[b * NJ + d]; qddv[d] = qdd ? qdd[b * NJ + d] : 0.f; }
        chain_trig<NJ>(qv, cs, sn);
        PoseP ee;
        f2 Bk[NJ][3];
        fk_chain_pairs_trig<CAP, NJ>(row, cs, sn, ee, Bk, [] {});
        for (int i = 0; i < 3; ++i) pos[b * 3 + i] = ee.B[i][1];
        Pose E;
        pose_from_pairs(ee, E);
        quat_xyzw(E.R, quat + b * 4);
        Force park[LINKS];
        rnea_chain_trig<LINKS, NJ>(row, flags & DRM_RNEA_GRAVITY, flags & DRM_RNEA_DAMPING, cs, sn, qdv, qddv, tv,
                                   [&](int k, const Force &F) { park[k] = F; }, [&](int k, Force &F) { F = park[k]; });
        for (int d = 0; d < NJ; ++d) tau[b * NJ + d] = tv[d];
    }
}

// the arithmetic of rnea_arm2_kernel: samples (b, b + 1) share a lane as (A, B); LINKS = 8 (whole table) or 7 (tail folded)
template <int LINKS>
void rnea_arm2_8_7(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int flags, float *tau) {
    constexpr int NJ = 7;
    for (int64_t b = 0; b < B; b += 2) {
        const int64_t b1 = b + 1 < B ? b + 1 : b;
        f2 qv[NJ], qdv[NJ], qddv[NJ], tv[NJ], cs[NJ], sn[NJ];
        for (int d = 0; d < NJ; ++d) {
            qv[d] = f2_make(q[b * NJ + d], q[b1 * NJ + d]);
            qdv[d] = f2_make(qd[b * NJ + d], qd[b1 * NJ + d]);
            qddv[d] = qdd ? f2_make(qdd[b * NJ + d], qdd[b1 * NJ + d]) : f2_bcast(0.f);
        }
        chain_trig2<NJ>(qv, cs, sn);
        Force2 park[LINKS];
        rnea_chain2_trig<LINKS, NJ>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, flags & DRM_RNEA_GRAVITY,
                                    flags & DRM_RNEA_DAMPING, cs, sn, qdv, qddv, tv, [&](int k, const Force2 &F) { park[k] = F; },
                                    [&](int k, Force2 &F) { F = park[k]; });
        for (int d = 0; d < NJ; ++d) { tau[b * NJ + d] = tv[d][0]; tau[b1 * NJ + d] = tv[d][1]; }
    }
}

// the arithmetic of rnea_fingers2_kernel<L>: finger w = ops w L .. w L + L - 1 = DoF columns of the same numbers; two samples share
// a lane; all body forces kept (nothing parked)
template <int L>
void rnea_fingers2_emu(const drm_walk *w, int K, const float *q, const float *qd, const float *qdd, int64_t B, int flags, float *tau) {
    const int n = w->n_dofs;
    for (int64_t b = 0; b < B; b += 2) {
        const int64_t b1 = b + 1 < B ? b + 1 : b;
        for (int f = 0; f < K; ++f) {
            f2 qv[L], qdv[L], qddv[L], tv[L], cs[L], sn[L];
            for (int d = 0; d < L; ++d) {
                const int c = f * L + d;
                qv[d] = f2_make(q[b * n + c], q[b1 * n + c]);
                qdv[d] = f2_make(qd[b * n + c], qd[b1 * n + c]);
                qddv[d] = qdd ? f2_make(qdd[b * n + c], qdd[b1 * n + c]) : f2_bcast(0.f);
            }
            chain_trig2<L>(qv, cs, sn);
            rnea_chain2_trig<L, L, L - 1>([&](int k) { return w->ops_f + (f * L + k) * DRM_OPF_STRIDE; }, flags & DRM_RNEA_GRAVITY,
                                          flags & DRM_RNEA_DAMPING, cs, sn, qdv, qddv, tv, [](int, const Force2 &) {}, [](int, Force2 &) {});
            for (int d = 0; d < L; ++d) { tau[b * n + f * L + d] = tv[d][0]; tau[b1 * n + f * L + d] = tv[d][1]; }
        }
    }
}

// the arithmetic of rnea_arm_hand_kernel<P, L> (one sample per lane; K sub-chains of L ops behind a prefix of P ops)
template <int P, int L>
void rnea_arm_hand_emu(const drm_walk *w, int K, const float *q, const float *qd, const float *qdd, int64_t B, int flags, float *tau) {
    const int n = w->n_dofs;
    const int32_t *w0 = w->ops_i + DRM_OPI_W0 * w->capacity;
    auto dof_of = [&](int k) { return (w0[k] & 0xff) - 1; };
    for (int64_t b = 0; b < B; ++b) {
        auto state = [&](int d, float &a, float &v, float &acc) {
            a = d < 0 ? 0.f : q[b * n + d]; v = d < 0 ? 0.f : qd[b * n + d]; acc = (d < 0 || !qdd) ? 0.f : qdd[b * n + d];
        };
        float qv[P], qdv[P], qddv[P], cs[P], sn[P], tp[P];
        for (int k = 0; k < P; ++k) state(dof_of(k), qv[k], qdv[k], qddv[k]);
        chain_trig<P>(qv, cs, sn);
        Force park[P];
        auto kind = [&](int op) { const int x = w0[op]; return ((x & 0xff) ? 1 : 0) | (((x >> 26) & 1) << 1); };
        rnea_arm_hand<P, L>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, kind, K, flags & DRM_RNEA_GRAVITY, flags & DRM_RNEA_DAMPING,
                            qv, cs, sn, qdv, qddv, [&](int j, int i, float &a, float &v, float &acc) { state(dof_of(P + j * L + i), a, v, acc); },
                            tp, [&](int j, int i, float t) { const int d = dof_of(P + j * L + i); if (d >= 0) tau[b * n + d] = t; },
                            [&](int k, const Force &F) { park[k] = F; }, [&](int k, Force &F) { F = park[k]; });
        for (int k = 0; k < P; ++k) if (dof_of(k) >= 0) tau[b * n + dof_of(k)] = tp[k];
    }
}

// the arithmetic of forward_dynamics_arm_hand_kernel<P, L>
template <int P, int L>
void fd_arm_hand_emu(const drm_walk *w, int K, const float *q, const float *qd, const float *f, int64_t B, int flags, float *qdd) {
    const int n = w->n_dofs;
    const int32_t *w0 = w->ops_i + DRM_OPI_W0 * w->capacity;
    auto dof_of = [&](int k) { return (w0[k] & 0xff) - 1; };
    auto kind = [&](int op) { const int x = w0[op]; return ((x & 0xff) ? 1 : 0) | (((x >> 26) & 1) << 1); };
    for (int64_t b = 0; b < B; ++b) {
        auto state = [&](int d, float &a, float &v, float &t) {
            a = d < 0 ? 0.f : q[b * n + d]; v = d < 0 ? 0.f : qd[b * n + d]; t = d < 0 ? 0.f : f[b * n + d];
        };
        float qv[P], qdv[P], fv[P], cs[P], sn[P], out[P], slot[P][8];
        for (int k = 0; k < P; ++k) state(dof_of(k), qv[k], qdv[k], fv[k]);
        chain_trig<P>(qv, cs, sn);
        aba_arm_hand<P, L>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, kind, K, flags & DRM_RNEA_GRAVITY, flags & DRM_RNEA_DAMPING,
                           qv, cs, sn, qdv, fv, [&](int j, int i, float &a, float &v, float &t) { state(dof_of(P + j * L + i), a, v, t); }, out,
                           [&](int j, int i, float a) { const int d = dof_of(P + j * L + i); if (d >= 0) qdd[b * n + d] = a; },
                           [&](int k, const float *s8) { for (int c = 0; c < 8; ++c) slot[k][c] = s8[c]; },
                           [&](int k, float *s8) { for (int c = 0; c < 8; ++c) s8[c] = slot[k][c]; });
        for (int k = 0; k < P; ++k) if (dof_of(k) >= 0) qdd[b * n + dof_of(k)] = out[k];
    }
}

// the arithmetic of crba_arm_hand_kernel<P, L>
template <int P, int L>
void crba_arm_hand_emu(const drm_walk *w, int K, const float *q, int64_t B, float *H) {
    const int n = w->n_dofs;
    const int32_t *w0 = w->ops_i + DRM_OPI_W0 * w->capacity;
    auto dof_of = [&](int k) { return (w0[k] & 0xff) - 1; };
    auto kind = [&](int op) { const int x = w0[op]; return ((x & 0xff) ? 1 : 0) | (((x >> 26) & 1) << 1); };
    for (int64_t b = 0; b < B; ++b) {
        for (int i = 0; i < n * n; ++i) H[b * n * n + i] = 0.f;
        float qv[P], cs[P], sn[P];
        for (int k = 0; k < P; ++k) qv[k] = dof_of(k) < 0 ? 0.f : q[b * n + dof_of(k)];
        chain_trig<P>(qv, cs, sn);
        auto row = [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; };
        auto hq = [&](int j, int i) { const int d = dof_of(P + j * L + i); return d < 0 ? 0.f : q[b * n + d]; };
        auto hout = [&](int oa, int ob, float v) {
            const int di = dof_of(oa), dj = dof_of(ob);
            H[(b * n + di) * n + dj] = v; H[(b * n + dj) * n + di] = v;
        };
        // as the kernel runs it: a wavefront per sub-chain, the palm's composites summed in sub-chain order, every wavefront
        // sweeps the prefix with its sub-chain's forces and its share of the prefix's columns
        Inertia palm, part[4];
        Force Fp[4][L];
        inertia_zero(palm);
        for (int j = 0; j < K; ++j) {
            crba_arm_hand_sub<P, L>(row, kind, j, [&](int i) { return hq(j, i); }, hout, Fp[j], part[j]);
            inertia_add(palm, part[j]);
        }
        for (int j = 0; j < K; ++j) crba_arm_hand_prefix<P, L>(row, kind, j, qv, cs, sn, palm, Fp[j], j, K, hout);
    }
}

// the arithmetic of rnea_backward_arm_hand_kernel<P, L>
template <int P, int L>
void rneab_arm_hand_emu(const drm_walk *w, int K, const float *q, const float *qd, const float *qdd, int64_t B, int flags,
                        const float *gtau, uint64_t mask, float *gq, float *gqd, float *gqdd, float *gops) {
    const int n = w->n_dofs, CAP = w->capacity;
    const int32_t *w0 = w->ops_i + DRM_OPI_W0 * w->capacity;
    auto dof_of = [&](int k) { return (w0[k] & 0xff) - 1; };
    auto kind = [&](int op) { const int x = w0[op]; return ((x & 0xff) ? 1 : 0) | (((x >> 26) & 1) << 1); };
    std::vector<double> sum((size_t)CAP * DRM_OPF_STRIDE, 0.0);
    for (int64_t b = 0; b < B; ++b) {
        auto at = [&](const float *a, int d) { return (d < 0 || !a) ? 0.f : a[b * n + d]; };
        float palm[36];
        rnea_backward_arm_hand<P, L>(
            [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, kind, K, flags & DRM_RNEA_GRAVITY, flags & DRM_RNEA_DAMPING, mask,
            gq != nullptr,
            [&](int k, float &a, float &v, float &acc, float &g) {
                const int d = dof_of(k);
                a = at(q, d); v = at(qd, d); acc = at(qdd, d); g = at(gtau, d);
            },
            [&](int j, int i, float &a, float &v, float &acc, float &g) {
                const int d = dof_of(P + j * L + i);
                a = at(q, d); v = at(qd, d); acc = at(qdd, d); g = at(gtau, d);
            },
            [&](int op, float a, float v, float acc) { const int d = dof_of(op); gq[b * n + d] = a; gqd[b * n + d] = v; gqdd[b * n + d] = acc; },
            [&](int k, const float *g) { for (int j = 0; j < DRM_OPF_STRIDE; ++j) sum[k * DRM_OPF_STRIDE + j] += g[j]; },
            [&](int i, float x) { palm[i] = x; }, [&](int i) { return palm[i]; });
    }
    if (gops) for (int i = 0; i < CAP * DRM_OPF_STRIDE; ++i) gops[i] = (float)sum[i];
}


// the arithmetic of forward_dynamics_arm_kernel<8, 7, LINKS>: bias torques by rnea_chain_trig with qdd = 0, H's lower triangle by
// crba_chain_trig on the same cos / sin, the unrolled L^T D L solve; LINKS = 7 (fixed tail folded) or 8 (the whole table)
template <int LINKS>
void fd_arm_8_7(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, int flags, float *qdd) {
    constexpr int NJ = 7;
    auto row = [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; };
    for (int64_t b = 0; b < B; ++b) {
        float qv[NJ], qdv[NJ], rhs[NJ], zero[NJ], nle[NJ], cs[NJ], sn[NJ];
        for (int d = 0; d < NJ; ++d) { qv[d] = q[b * NJ + d]; qdv[d] = qd[b * NJ + d]; rhs[d] = f[b * NJ + d]; zero[d] = 0.f; }
        chain_trig<NJ>(qv, cs, sn);
        Force park[8];
        rnea_chain_trig<LINKS, NJ>(row, flags & DRM_RNEA_GRAVITY, flags & DRM_RNEA_DAMPING, cs, sn, qdv, zero, nle,
                                   [&](int k, const Force &F) { park[k] = F; }, [&](int k, Force &F) { F = park[k]; });
        float Ht[NJ * (NJ + 1) / 2];
        crba_chain_trig<LINKS, NJ>(row, cs, sn, [&](int i, int j, float v) { if (i >= j) Ht[tri_index(i, j)] = v; });
        for (int d = 0; d < NJ; ++d) rhs[d] -= nle[d];
        ltdl_solve_unrolled<NJ>(Ht, rhs);
        for (int d = 0; d < NJ; ++d) qdd[b * NJ + d] = rhs[d];
    }
}

} // namespace

extern "C" {
int emu_fk(const drm_walk *w, const float *q, int64_t B, int32_t T, float *pos, float *quat) {
    fk_loop(w, q, B, T, pos, quat);
    return 0;
}
int emu_fk_jacobian(const drm_walk *w, const float *q, int64_t B, float *pos, float *quat, float *lin, float *ang) {
    jac_loop(w, q, B, pos, quat, lin, ang);
    return 0;
}
int emu_fk_jacobian_arm(const drm_walk *w, const float *q, int64_t B, float *pos, float *quat, float *lin, float *ang) {
    if (!(w->shape & DRM_WALK_ARM_CHAIN) || w->capacity != 8 || w->n_dofs != 7) return -2;
    jac_arm_8_7(w, q, B, pos, quat, lin, ang);
    return 0;
}
int emu_rnea_arm(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau) {
    if (!(w->shape & DRM_WALK_ARM_CHAIN) || w->capacity != 8 || w->n_dofs != 7) return -2;
    if (w->n_ops == 7) rnea_arm_8_7<7>(w, q, qd, qdd, B, flags, tau);
    else rnea_arm_8_7<8>(w, q, qd, qdd, B, flags, tau);
    return 0;
}
// drm_fk_rnea's fused arm rung (fk_rnea_arm_applies): the tree walk IS the chain (8 ops on both), or the tree walk holds the 7 moving
// joints and the chain walk the fixed tail behind them
int emu_fk_rnea_arm(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                    float *tau, float *pos, float *quat) {
    if (!(tree->shape & DRM_WALK_ARM_CHAIN) || tree->capacity != 8 || tree->n_dofs != 7) return -2;
    if (!(chain->shape & DRM_WALK_ARM_CHAIN) || chain->capacity != 8 || chain->n_ops != 8 || chain->target_perm != 2) return -2;
    if (tree->n_ops == 7) fk_rnea_arm_8_7<7>(tree, chain, q, qd, qdd, B, flags, tau, pos, quat);
    else if (tree->n_ops == 8) fk_rnea_arm_8_7<8>(tree, chain, q, qd, qdd, B, flags, tau, pos, quat);
    else return -2;
    return 0;
}
int emu_rnea_arm_hand(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau) {
    if (!(w->shape & DRM_WALK_ARM_HAND)) return -2;
    const int P = DRM_WALK_AH_P(w->shape), K = DRM_WALK_AH_K(w->shape), L = DRM_WALK_AH_L(w->shape);
    if (P + K * L != w->n_ops) return -1;
    if (P == 7 && L == 1) { rnea_arm_hand_emu<7, 1>(w, K, q, qd, qdd, B, flags, tau); return 0; }
    if (P == 6 && L == 2) { rnea_arm_hand_emu<6, 2>(w, K, q, qd, qdd, B, flags, tau); return 0; }
    if (P == 7 && L == 4) { rnea_arm_hand_emu<7, 4>(w, K, q, qd, qdd, B, flags, tau); return 0; }
    if (P == 9 && L == 1) rnea_arm_hand_emu<9, 1>(w, K, q, qd, qdd, B, flags, tau);
    else if (P == 7 && L == 2) rnea_arm_hand_emu<7, 2>(w, K, q, qd, qdd, B, flags, tau);
    else if (P == 8 && L == 4) rnea_arm_hand_emu<8, 4>(w, K, q, qd, qdd, B, flags, tau);
    else return -2;
    return 0;
}
int emu_forward_dynamics_arm_hand(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, int32_t flags, float *qdd) {
    if (!(w->shape & DRM_WALK_ARM_HAND)) return -2;
    const int P = DRM_WALK_AH_P(w->shape), K = DRM_WALK_AH_K(w->shape), L = DRM_WALK_AH_L(w->shape);
    if (P + K * L != w->n_ops) return -1;
    if (P == 7 && L == 1) { fd_arm_hand_emu<7, 1>(w, K, q, qd, f, B, flags, qdd); return 0; }
    if (P == 6 && L == 2) { fd_arm_hand_emu<6, 2>(w, K, q, qd, f, B, flags, qdd); return 0; }
    if (P == 7 && L == 4) { fd_arm_hand_emu<7, 4>(w, K, q, qd, f, B, flags, qdd); return 0; }
    if (P == 9 && L == 1) fd_arm_hand_emu<9, 1>(w, K, q, qd, f, B, flags, qdd);
    else if (P == 7 && L == 2) fd_arm_hand_emu<7, 2>(w, K, q, qd, f, B, flags, qdd);
    else if (P == 8 && L == 4) fd_arm_hand_emu<8, 4>(w, K, q, qd, f, B, flags, qdd);
    else return -2;
    return 0;
}
int emu_crba_arm_hand(const drm_walk *w, const float *q, int64_t B, float *H) {
    if (!(w->shape & DRM_WALK_ARM_HAND)) return -2;
    const int P = DRM_WALK_AH_P(w->shape), K = DRM_WALK_AH_K(w->shape), L = DRM_WALK_AH_L(w->shape);
    if (P + K * L != w->n_ops || K < 2 || K > 4) return -1;
    if (P == 7 && L == 1) { crba_arm_hand_emu<7, 1>(w, K, q, B, H); return 0; }
    if (P == 6 && L == 2) { crba_arm_hand_emu<6, 2>(w, K, q, B, H); return 0; }
    if (P == 7 && L == 4) { crba_arm_hand_emu<7, 4>(w, K, q, B, H); return 0; }
    if (P == 9 && L == 1) crba_arm_hand_emu<9, 1>(w, K, q, B, H);
    else if (P == 7 && L == 2) crba_arm_hand_emu<7, 2>(w, K, q, B, H);
    else if (P == 8 && L == 4) crba_arm_hand_emu<8, 4>(w, K, q, B, H);
    else return -2;
    return 0;
}
int emu_rnea_fingers(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau) {
    if (!(w->shape & DRM_WALK_FINGERS)) return -2;
    const int K = DRM_WALK_AH_K(w->shape), L = DRM_WALK_AH_L(w->shape);
    if (K * L != w->n_ops || w->n_ops != w->n_dofs) return -1;
    if (L == 2) rnea_fingers2_emu<2>(w, K, q, qd, qdd, B, flags, tau);
    else if (L == 3) rnea_fingers2_emu<3>(w, K, q, qd, qdd, B, flags, tau);
    else if (L == 4) rnea_fingers2_emu<4>(w, K, q, qd, qdd, B, flags, tau);
    else return -2;
    return 0;
}
int emu_rnea_arm2(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau) {
    if (!(w->shape & DRM_WALK_ARM_CHAIN) || w->capacity != 8 || w->n_dofs != 7) return -2;
    if (w->n_ops == 7) rnea_arm2_8_7<7>(w, q, qd, qdd, B, flags, tau);
    else rnea_arm2_8_7<8>(w, q, qd, qdd, B, flags, tau);
    return 0;
}
int emu_rnea_backward(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                      const float *gtau, uint64_t mask, float *gq, float *gqd, float *gqdd, float *gops) {
    rneab_t(w, q, qd, qdd, B, flags, gtau, mask, gq, gqd, gqdd, gops);
    return 0;
}
int emu_forward_dynamics(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, int32_t flags,
                         float *qdd) {
    fd_loop(w, q, qd, f, B, flags, qdd);
    return 0;
}
int emu_forward_dynamics_arm(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, int32_t flags, float *qdd) {
    if (!(w->shape & DRM_WALK_ARM_CHAIN) || w->capacity != 8 || w->n_dofs != 7) return -2;
    if (w->n_ops == 7) fd_arm_8_7<7>(w, q, qd, f, B, flags, qdd);
    else fd_arm_8_7<8>(w, q, qd, f, B, flags, qdd);
    return 0;
}
int emu_link_rows(const float *params, int32_t n, float *rows) {
    for (int i = 0; i < n; ++i) link_row(params + i * LINK_PARAM_FLOATS, rows + i * DRM_OPF_STRIDE);
    return 0;
}
int emu_link_rows_backward(const float *params, const float *grad_rows, int32_t n, float *grad_params) {
    for (int i = 0; i < n; ++i)
        link_row_backward(params + i * LINK_PARAM_FLOATS, grad_rows + i * DRM_OPF_STRIDE, grad_params + i * LINK_PARAM_FLOATS);
    return 0;
}
int emu_rnea_backward_arm_hand(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                               const float *gtau, uint64_t mask, float *gq, float *gqd, float *gqdd, float *gops) {
    if (!(w->shape & DRM_WALK_ARM_HAND)) return -2;
    const int P = DRM_WALK_AH_P(w->shape), K = DRM_WALK_AH_K(w->shape), L = DRM_WALK_AH_L(w->shape);
    if (P + K * L != w->n_ops) return -1;
#define X(p, l) if (P == p && L == l) { rneab_arm_hand_emu<p, l>(w, K, q, qd, qdd, B, flags, gtau, mask, gq, gqd, gqdd, gops); return 0; }
    X(7, 1) X(6, 2) X(7, 4) X(9, 1) X(7, 2) X(8, 4)
#undef X
    return -2;
}
int emu_rnea_backward_arm(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                          const float *gtau, uint64_t mask, float *gq, float *gqd, float *gqdd, float *gops) {
    if (!(w->shape & DRM_WALK_ARM_CHAIN) || w->capacity != 8 || w->n_dofs != 7) return -2;
    constexpr int CAP = 8, NJ = 7;
    static thread_local double sum[CAP * DRM_OPF_STRIDE];
    for (int i = 0; i < CAP * DRM_OPF_STRIDE; ++i) sum[i] = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        float qv[NJ], qdv[NJ], qddv[NJ], gt[NJ];
        for (int d = 0; d < NJ; ++d) {
            qv[d] = q[b * NJ + d]; qdv[d] = qd[b * NJ + d]; qddv[d] = qdd ? qdd[b * NJ + d] : 0.f; gt[d] = gtau[b * NJ + d];
        }
        rnea_backward_chain<CAP, NJ>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, flags & DRM_RNEA_GRAVITY,
                                     flags & DRM_RNEA_DAMPING, mask, gq != nullptr, qv, qdv, qddv, gt,
                                     [&](int d, float a, float v, float c) { gq[b * NJ + d] = a; gqd[b * NJ + d] = v; gqdd[b * NJ + d] = c; },
                                     [&](int k, const float *g) { for (int j = 0; j < DRM_OPF_STRIDE; ++j) sum[k * DRM_OPF_STRIDE + j] += g[j]; });
    }
    if (gops) for (int i = 0; i < CAP * DRM_OPF_STRIDE; ++i) gops[i] = (float)sum[i];
    return 0;
}
int emu_fk_backward_arm(const drm_walk *w, const float *q, int64_t B, const float *gpos, uint64_t mask, float *gq, float *gops) {
    if (!(w->shape & DRM_WALK_ARM_CHAIN) || w->capacity != 8 || w->n_dofs != 7) return -2;
    constexpr int CAP = 8, NJ = 7;
    static thread_local double sum[CAP * 12];
    for (int i = 0; i < CAP * 12; ++i) sum[i] = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        float qv[NJ], gv[3], out[NJ];
        for (int d = 0; d < NJ; ++d) qv[d] = q[b * NJ + d];
        for (int i = 0; i < 3; ++i) gv[i] = gpos[b * 3 + i];
        fk_backward_chain<CAP, NJ>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, qv, gv, mask, out,
                                   [&](int d) { return qv[d]; },
                                   [&](int k, const float *dF, const float *dt) {
                                       for (int j = 0; j < 9; ++j) sum[k * 12 + j] += dF[j];
                                       for (int j = 0; j < 3; ++j) sum[k * 12 + 9 + j] += dt[j];
                                   });
        if (gq) for (int d = 0; d < NJ; ++d) gq[b * NJ + d] = out[d];
    }
    if (gops)
        for (int k = 0; k < CAP; ++k) {
            for (int j = 0; j < DRM_OPF_STRIDE; ++j) gops[k * DRM_OPF_STRIDE + j] = 0.f;
            for (int j = 0; j < 12; ++j)
                gops[k * DRM_OPF_STRIDE + (j < 9 ? DRM_OPF_FIJ(j / 3, j % 3) : DRM_OPF_TI(j - 9))] = (float)sum[k * 12 + j];
        }
    return 0;
}
int emu_crba_arm(const drm_walk *w, const float *q, int64_t B, float *H) {
    if (!(w->shape & DRM_WALK_ARM_CHAIN) || w->capacity != 8 || w->n_dofs != 7) return -2;
    for (int64_t b = 0; b < B; ++b) {
        float qv[7];
        for (int d = 0; d < 7; ++d) qv[d] = q[b * 7 + d];
        crba_chain<8, 7>([&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, qv,
                         [&](int i, int j, float v) { H[(b * 7 + i) * 7 + j] = v; });
    }
    return 0;
}
int emu_crba(const drm_walk *w, const float *q, int64_t B, float *H) {
    crba_loop(w, q, B, H);
    return 0;
}
int emu_fk_backward(const drm_walk *w, const float *q, int64_t B, int32_t T, const float *gpos, uint64_t mask, float *gq,
                    float *gops) {
    fkb_t(w, q, B, T, gpos, nullptr, nullptr, mask, gq, gops);
    return 0;
}
int emu_fk_backward_rot(const drm_walk *w, const float *q, int64_t B, int32_t T, const float *gpos, const float *grot,
                        uint64_t mask, float *gq, float *gops) {
    fkb_t(w, q, B, T, gpos, nullptr, nullptr, mask, gq, gops, grot);
    return 0;
}
int emu_fk_jacobian_backward(const drm_walk *w, const float *q, int64_t B, const float *gpos, const float *glin,
                             const float *gang, uint64_t mask, float *gq, float *gops) {
    fkb_t(w, q, B, 1, gpos, glin, gang, mask, gq, gops);
    return 0;
}
int emu_rnea_short(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau) {
    // the register-parked form of short segments (drm_tree.hpp rnea_tree_walk_short<6>)
    const int n = w->n_dofs;
    const Ctl ctl(w);
    for (int s = 0; s < w->n_segments; ++s)
        if (w->seg_begin[s + 1] - w->seg_begin[s] > 6) return -2;
    for (int64_t b = 0; b < B; ++b)
        for (int seg = 0; seg < w->n_segments; ++seg) {
            Motion ms[DRM_MAX_SLOTS];
            Force fs[DRM_MAX_SLOTS];
            for (auto &F : fs) for (int i = 0; i < 3; ++i) F.la[i] = f2_bcast(0.f);
            rnea_tree_walk_short<6>(
                w->prefix_end, w->seg_begin[seg], w->seg_begin[seg + 1], ctl, [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; }, flags,
                [&](int d, float &a, float &v, float &acc) { a = q[b * n + d]; v = qd[b * n + d]; acc = qdd ? qdd[b * n + d] : 0.f; },
                [&](int d, float v) { tau[b * n + d] = v; }, [&](int sl, const Motion &M) { ms[sl] = M; },
                [&](int sl, Motion &M) { M = ms[sl]; },
                [&](int sl, const Force &F) { for (int i = 0; i < 3; ++i) fs[sl].la[i] += F.la[i]; },
                [&](int sl, Force &F) { for (int i = 0; i < 3; ++i) { F.la[i] += fs[sl].la[i]; fs[sl].la[i] = f2_bcast(0.f); } });
        }
    return 0;
}
int emu_rnea(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau) {
    rnea_loop(w, q, qd, qdd, B, flags, tau);
    return 0;
}
}

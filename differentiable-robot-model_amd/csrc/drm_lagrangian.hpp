// drm_lagrangian.hpp — include/drm_hip.h drm_lagrangian_dynamics: the per-row arithmetic of H(q), the Christoffel-consistent Coriolis
// matrix C(q, qd) and the gravity torques g(q) of  H qdd + C qd + g = tau  in ONE sweep over the tree (Echeandia and Wensing, "Numerical
// methods to compute the Coriolis matrix and Christoffel symbols for rigid-body systems", 2021).  Shared by the kernels
// (drm_lagrangian.hip) and by the host build (drm_cpu.cpp) so that both round the same way.  Kept out of drm_sample.hpp on purpose, as
// drm_fdd.hpp and drm_regressor.hpp are: that header is part of the source key of every robot's own kernels (specialize._HEADERS).
//
// Frames: every quantity of link i in link i's OWN stored frame (joint about / along +z, child -> parent x_p = J x_c + t), as the RNEA
// and CRBA walks; spatial vectors as (angular, linear) at the link origin.  The joint axes are then component picks, and nothing is
// formed about a distant origin: a base-frame version sums inertias about the robot's base, whose parallel-axis terms cancel in
// float32 when the entries of C are read off (DESIGN_KERNELS.md).
//
//   forward   v_i = X v_parent + S_i qd_i          velocity (w, u);  gd_i = J^T gd_parent, the base acceleration (0, 0, +9.81) that stands
//                                                  for gravity (drm_sample.hpp motion_root)
//   per body  IC_i = I_i                           (m, h = m c, I_o): drm_sample.hpp Inertia
//             BC_i = (crf(v) I - I crm(v) + bar(I v)) / 2
//   backward  F1 = IC_j Sd_j + BC_j S_j,  F2 = IC_j S_j,  F3 = BC_j^T S_j   with Sd_j = crm(v_j) S_j;   g_j = F2 . (0, gd_j)
//             up the ancestors i = j, parent(j), ... (the three wrenches moved by each joint transform on the way):
//                 H[i, j] = H[j, i] = S_i . F2      C[i, j] = S_i . F1      C[j, i] = Sd_i . F2 + S_i . F3   (i != j)
//             IC_parent += IC_j,  BC_parent += BC_j   (moved into the parent's frame)
//
// BC is not a general 6 x 6 matrix.  Written out for one body with momentum (N, P) = I v:  BC = [[A, 0], [-[P]x, 0]] with
//   A = ([w]x I_o - I_o [w]x - [u]x [h]x - [h]x [u]x - [N]x) / 2,       P = m u - h x w
// and the form survives the move into the parent's frame (P' = J P, A' = J A J^T - [t]x [P']x) and the sum over a sub-tree: twelve
// floats, P the linear momentum of the sub-tree.  So  BC S = (A e_z, e_z x P)  and  BC^T S = (A^T e_z, 0)  for a revolute joint,
// BC S = 0  and  BC^T S = (P x e_z, 0)  for a prismatic one.
#pragma once
#include "drm_sample.hpp"
#include "drm_tree.hpp"

namespace drm {

constexpr float LAG_MAX_ARG = SINCOS_PAIR_MAX_ARG; // a joint value beyond this (or not finite) makes the row's outputs NaN
constexpr int LAG_REC_FLOATS = 12;                 // per op between the sweeps: cos, sin, value of the joint, w, u, gd
constexpr int LAG_SLOT_FLOATS = 22;                // per open branch point on the way back: the composite (IC: 10, BC: 12)

struct LagVel {
    float w[3], u[3]; // angular, linear velocity
    float gd[3];      // the base acceleration in this frame
};
struct LagWrench {
    float n[3], f[3]; // moment, force
};
struct LagBias {
    float A[9], P[3];
};
struct LagComposite {
    Inertia I;
    LagBias B;
};

DRM_HD void lag_vel_root(LagVel &v) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { v.w[i] = 0.0f; v.u[i] = 0.0f; v.gd[i] = 0.0f; }
    v.gd[2] = 9.81f;
}
// w = J^T w_p (+ e_z qd) ;  u = J^T (u_p + w_p x t) (+ e_z qd for a prismatic joint) ;  gd = J^T gd_p
DRM_HD void lag_vel_step(const float *J, const float *t, float qd, bool moving, bool prismatic, const LagVel &par, LagVel &out) {
    float x[3], y[3];
    LagVel N;
    matT_vec(J, par.w, N.w);
    cross3(par.w, t, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = par.u[i] + x[i];
    matT_vec(J, y, N.u);
    matT_vec(J, par.gd, N.gd);
    if (moving) {
        if (prismatic) N.u[2] += qd;
        else N.w[2] += qd;
    }
    out = N;
}

DRM_HD void lag_composite_zero(LagComposite &c) {
    inertia_zero(c.I);
#pragma unroll
    for (int i = 0; i < 9; ++i) c.B.A[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.B.P[i] = 0.0f;
}
DRM_HD void lag_composite_add(LagComposite &a, const LagComposite &b) {
    inertia_add(a.I, b.I);
#pragma unroll
    for (int i = 0; i < 9; ++i) a.B.A[i] += b.B.A[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) a.B.P[i] += b.B.P[i];
}
DRM_HD void lag_composite_to_floats(const LagComposite &c, float *v) {
    v[0] = c.I.m;
#pragma unroll
    for (int i = 0; i < 3; ++i) v[1 + i] = c.I.h[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[4 + i] = c.I.I[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) v[10 + i] = c.B.A[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[19 + i] = c.B.P[i];
}
DRM_HD void lag_composite_from_floats(const float *v, LagComposite &c) {
    c.I.m = v[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.I.h[i] = v[1 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) c.I.I[i] = v[4 + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) c.B.A[i] = v[10 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.B.P[i] = v[19 + i];
}

// I_o x for the packed symmetric I_o
DRM_HD void lag_sym_vec(const float *I, const float *x, float *y) {
    y[0] = I[0] * x[0] + I[1] * x[1] + I[2] * x[2];
    y[1] = I[1] * x[0] + I[3] * x[1] + I[4] * x[2];
    y[2] = I[2] * x[0] + I[4] * x[1] + I[5] * x[2];
}

// BC of one body from its own inertia and velocity
DRM_HD void lag_body_bias(const Inertia &I, const LagVel &v, LagBias &B) {
    float Iw[3], hu[3], hw[3], N[3];
    lag_sym_vec(I.I, v.w, Iw);
    cross3(I.h, v.u, hu);
    cross3(I.h, v.w, hw);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        N[i] = Iw[i] + hu[i];
        B.P[i] = I.m * v.u[i] - hw[i];
    }
    // M = [w]x I_o: column c of M is w x (column c of I_o);  [w]x I_o - I_o [w]x = M + M^T
    const float If[9] = {I.I[0], I.I[1], I.I[2], I.I[1], I.I[3], I.I[4], I.I[2], I.I[4], I.I[5]};
    float M[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float col[3] = {If[c], If[3 + c], If[6 + c]};
        float x[3];
        cross3(v.w, col, x);
        M[c] = x[0]; M[3 + c] = x[1]; M[6 + c] = x[2];
    }
    // -([u]x [h]x + [h]x [u]x) = 2 (u . h) 1 - u h^T - h u^T
    const float uh2 = 2.0f * (v.u[0] * I.h[0] + v.u[1] * I.h[1] + v.u[2] * I.h[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            B.A[r * 3 + c] = 0.5f * (M[r * 3 + c] + M[c * 3 + r] + (r == c ? uh2 : 0.0f) - (v.u[r] * I.h[c] + I.h[r] * v.u[c]));
    // - [N]x / 2
    B.A[1] += 0.5f * N[2]; B.A[2] -= 0.5f * N[1];
    B.A[3] -= 0.5f * N[2]; B.A[5] += 0.5f * N[0];
    B.A[6] += 0.5f * N[1]; B.A[7] -= 0.5f * N[0];
}

// BC into the parent's frame: P' = J P, A' = J A J^T - [t]x [P']x,   - [t]x [P']x = (t . P') 1 - P' t^T
DRM_HD void lag_bias_to_parent(const float *J, const float *t, const LagBias &c, LagBias &out) {
    float M[9], P[3];
    mat_vec(J, c.P, P);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[r * 3 + k] = J[r * 3 + 0] * c.A[0 * 3 + k] + J[r * 3 + 1] * c.A[1 * 3 + k] + J[r * 3 + 2] * c.A[2 * 3 + k];
    const float tp = t[0] * P[0] + t[1] * P[1] + t[2] * P[2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            out.A[r * 3 + k] = (M[r * 3 + 0] * J[k * 3 + 0] + M[r * 3 + 1] * J[k * 3 + 1] + M[r * 3 + 2] * J[k * 3 + 2]) +
                               ((r == k ? tp : 0.0f) - P[r] * t[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i) out.P[i] = P[i];
}
DRM_HD void lag_composite_to_parent(const float *J, const float *t, const LagComposite &c, LagComposite &out) {
    inertia_to_parent(J, t, c.I, out.I);
    lag_bias_to_parent(J, t, c.B, out.B);
}

// the three wrenches of joint j (about / along +z of its frame) from the composites of its sub-tree and its link's velocity
DRM_HD void lag_joint_wrenches(const LagComposite &c, const LagVel &v, bool prismatic, LagWrench &F1, LagWrench &F2, LagWrench &F3) {
    const Inertia &I = c.I;
    const LagBias &B = c.B;
    if (!prismatic) {
        // S = (e_z, 0);  Sd = (w x e_z, u x e_z) = ((w_y, -w_x, 0), (u_y, -u_x, 0))
        const float a[3] = {v.w[1], -v.w[0], 0.0f}, b[3] = {v.u[1], -v.u[0], 0.0f};
        float Ia[3], hb[3], ha[3];
        lag_sym_vec(I.I, a, Ia);
        cross3(I.h, b, hb);
        cross3(I.h, a, ha);
        F1.n[0] = Ia[0] + hb[0] + B.A[2]; F1.n[1] = Ia[1] + hb[1] + B.A[5]; F1.n[2] = Ia[2] + hb[2] + B.A[8];
        F1.f[0] = I.m * b[0] - ha[0] - B.P[1]; F1.f[1] = I.m * b[1] - ha[1] + B.P[0]; F1.f[2] = I.m * b[2] - ha[2];
        F2.n[0] = I.I[2]; F2.n[1] = I.I[4]; F2.n[2] = I.I[5];
        F2.f[0] = -I.h[1]; F2.f[1] = I.h[0]; F2.f[2] = 0.0f;
        F3.n[0] = B.A[6]; F3.n[1] = B.A[7]; F3.n[2] = B.A[8];
    } else {
        // S = (0, e_z);  Sd = (0, w x e_z)
        const float b[3] = {v.w[1], -v.w[0], 0.0f};
        cross3(I.h, b, F1.n);
#pragma unroll
        for (int i = 0; i < 3; ++i) F1.f[i] = I.m * b[i];
        F2.n[0] = I.h[1]; F2.n[1] = -I.h[0]; F2.n[2] = 0.0f;
        F2.f[0] = 0.0f; F2.f[1] = 0.0f; F2.f[2] = I.m;
        F3.n[0] = B.P[1]; F3.n[1] = -B.P[0]; F3.n[2] = 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) F3.f[i] = 0.0f;
}
// f' = J f ;  n' = J n + t x f'
DRM_HD void lag_wrench_up(const float *J, const float *t, LagWrench &F) {
    float f[3], n[3], x[3];
    mat_vec(J, F.f, f);
    mat_vec(J, F.n, n);
    cross3(t, f, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) { F.f[i] = f[i]; F.n[i] = n[i] + x[i]; }
}
DRM_HD float lag_axis_dot(const LagWrench &F, bool prismatic) { return prismatic ? F.f[2] : F.n[2]; }
// Sd_i . F for the joint of a link with velocity v
DRM_HD float lag_axis_rate_dot(const LagVel &v, bool prismatic, const LagWrench &F) {
    const float lin = v.w[1] * F.f[0] - v.w[0] * F.f[1];
    if (prismatic) return lin;
    return (v.w[1] * F.n[0] - v.w[0] * F.n[1]) + (v.u[1] * F.f[0] - v.u[0] * F.f[1]);
}
DRM_HD float lag_gravity(const LagWrench &F2, const LagVel &v) { return F2.f[0] * v.gd[0] + F2.f[1] * v.gd[1] + F2.f[2] * v.gd[2]; }

// a row whose joint values or rates cannot be used: the caller walks it at rest at q = 0 and hands out NaN
DRM_HD bool lag_bad_input(float q, float qd) { return !(fabsf(q) <= LAG_MAX_ARG) || !(fabsf(qd) <= 3.0e38f); }

DRM_HD void lag_record_pack(float c, float s, float q, const LagVel &v, float *r) {
    r[0] = c; r[1] = s; r[2] = q;
#pragma unroll
    for (int i = 0; i < 3; ++i) { r[3 + i] = v.w[i]; r[6 + i] = v.u[i]; r[9 + i] = v.gd[i]; }
}
DRM_HD void lag_record_unpack(const float *r, float &c, float &s, float &q, LagVel &v) {
    c = r[0]; s = r[1]; q = r[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) { v.w[i] = r[3 + i]; v.u[i] = r[6 + i]; v.gd[i] = r[9 + i]; }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ANY walk, one row: the ops [0, n_ops) in walk order, all segments by the one caller.  The forward sweep leaves one record per op
// (LAG_REC_FLOATS: a link finds its parent's velocity there, by the parent's op index, DRM_OPI_W1); the sweep back carries the
// composite of a chain in registers and parks it at open branch points (LAG_SLOT_FLOATS per slot), as crba_tree_walk does.
//   qf(d, q, qd)                      joint value and rate of DoF d (zeros for a row that is not to be used)
//   rput(k, const float *) / rget(k, float *)       the record of op k
//   sput(s, const float *) / sget(s, float *)       the composite parked in slot s
//   hout(i, j, v)  cout(i, j, v)  gout(j, v)        entries of H (both triangles are handed over), C and g by DoF
// Only entries between a joint and its ancestors are handed over: every other entry of H and C is zero, and the caller's to write.
template <class CTL, class ROW, class QF, class RPUT, class RGET, class SPUT, class SGET, class HOUT, class COUT, class GOUT>
DRM_HD void lagrangian_tree_walk(int n_ops, int p_end, int n_slots, CTL ctl, ROW row, QF qf, RPUT rput, RGET rget, SPUT sput, SGET sget,
                                 HOUT hout, COUT cout, GOUT gout) {
    float rec[LAG_REC_FLOATS], sl[LAG_SLOT_FLOATS];
    // ---- forward: velocities ------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int k = 0; k < n_ops; ++k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        float q = 0.0f, qd = 0.0f, c = 1.0f, s = 0.0f;
        if (ct.dof >= 0) {
            qf(ct.dof, q, qd);
            if (!ct.prismatic) sincos_one(q, s, c);
        }
        LagVel par;
        if (ct.src == DRM_SRC_ROOT || ct.parent < 0 || ct.parent >= k) {
            lag_vel_root(par);
        } else {
            float pc, ps, pq;
            rget(ct.parent, rec);
            lag_record_unpack(rec, pc, ps, pq, par);
        }
        const OpFT o = load_ft(row(k));
        float J[9], t[3];
        joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
        LagVel v;
        lag_vel_step(J, t, qd, ct.dof >= 0, ct.prismatic, par, v);
        lag_record_pack(c, s, q, v, rec);
        rput(k, rec);
    }
    // ---- back: composites, and every joint's wrenches up its ancestors ------------------------------------------------------
    LagComposite carry;
    lag_composite_zero(carry);
    lag_composite_to_floats(carry, sl);
#pragma unroll 1
    for (int s = 0; s < n_slots; ++s) sput(s, sl);
#pragma unroll 1
    for (int k = n_ops - 1; k >= p_end; --k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        const float *of = row(k);
        LagVel v;
        float c, s, q;
        rget(k, rec);
        lag_record_unpack(rec, c, s, q, v);
        LagComposite tot;
        inertia_from_row(of, tot.I);
        lag_body_bias(tot.I, v, tot.B);
        if (ct.child_next) lag_composite_add(tot, carry);
        if (ct.save >= 0 && ct.save < n_slots) { // take: add and reset
            LagComposite parked;
            sget(ct.save, sl);
            lag_composite_from_floats(sl, parked);
            lag_composite_add(tot, parked);
            LagComposite z;
            lag_composite_zero(z);
            lag_composite_to_floats(z, sl);
            sput(ct.save, sl);
        }
        const OpFT o = load_ft(of);
        float J[9], t[3];
        joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
        if (ct.dof >= 0) {
            LagWrench F1, F2, F3;
            lag_joint_wrenches(tot, v, ct.prismatic, F1, F2, F3);
            gout(ct.dof, lag_gravity(F2, v));
            hout(ct.dof, ct.dof, lag_axis_dot(F2, ct.prismatic));
            cout(ct.dof, ct.dof, lag_axis_dot(F1, ct.prismatic));
            lag_wrench_up(J, t, F1);
            lag_wrench_up(J, t, F2);
            lag_wrench_up(J, t, F3);
            int anc = ct.parent;
#pragma unroll 1
            while (anc >= p_end && anc < k) {
                int v0, v1;
                ctl_words(ctl, anc, v0, v1);
                const OpCtl ca = decode_ctl(v0, v1);
                LagVel va;
                float ac, as, aq;
                rget(anc, rec);
                lag_record_unpack(rec, ac, as, aq, va);
                if (ca.dof >= 0) {
                    const float h = lag_axis_dot(F2, ca.prismatic);
                    hout(ca.dof, ct.dof, h);
                    hout(ct.dof, ca.dof, h);
                    cout(ca.dof, ct.dof, lag_axis_dot(F1, ca.prismatic));
                    cout(ct.dof, ca.dof, lag_axis_rate_dot(va, ca.prismatic, F2) + lag_axis_dot(F3, ca.prismatic));
                }
                if (ca.src == DRM_SRC_ROOT || ca.parent < p_end) break;
                const OpFT oa = load_ft(row(anc));
                float Ja[9], ta[3];
                joint_transform(oa, ca.dof >= 0, ca.prismatic, aq, ac, as, Ja, ta);
                lag_wrench_up(Ja, ta, F1);
                lag_wrench_up(Ja, ta, F2);
                lag_wrench_up(Ja, ta, F3);
                anc = ca.parent;
            }
        }
        if (ct.src != DRM_SRC_ROOT && ct.parent >= p_end) {
            LagComposite up;
            lag_composite_to_parent(J, t, tot, up);
            if (ct.src >= 0) {
                if (ct.src < n_slots) {
                    LagComposite parked;
                    sget(ct.src, sl);
                    lag_composite_from_floats(sl, parked);
                    lag_composite_add(parked, up);
                    lag_composite_to_floats(parked, sl);
                    sput(ct.src, sl);
                }
            } else {
                carry = up;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same on a serial chain whose first NJ ops are revolute joints driving DoF columns 0 .. NJ-1 (DRM_WALK_ARM_CHAIN), straight
// line, on cos / sin the caller already has; ops NJ .. LINKS-1 are fixed.  Everything stays in registers: the velocities of the
// links on the way out, one composite and three wrenches on the way back; the joint transforms are rebuilt from cos / sin and the
// table where they are used.  WANT_H / WANT_G: outputs nobody reads are not formed (H and g fall out of F2, which C needs anyway).
template <int LINKS, int NJ, bool WANT_H, bool WANT_G, class ROW, class HOUT, class COUT, class GOUT>
DRM_HD void lagrangian_chain_trig(ROW row, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ], HOUT hout, COUT cout,
                                  GOUT gout) {
    LagVel v[LINKS];
    {
        LagVel cur;
        lag_vel_root(cur);
#pragma unroll
        for (int k = 0; k < LINKS; ++k) {
            const OpFT o = load_ft(row(k));
            float J[9];
            if (k < NJ) {
                joint_rot_z(o.F, cs[k], sn[k], J);
            } else {
#pragma unroll
                for (int i = 0; i < 9; ++i) J[i] = o.F[i];
            }
            lag_vel_step(J, o.t, k < NJ ? qd[k] : 0.0f, k < NJ, false, cur, cur);
            v[k] = cur;
        }
    }
    LagComposite carry;
#pragma unroll
    for (int k = LINKS - 1; k >= 0; --k) {
        DRM_RNEA_LINK_FENCE();
        LagComposite tot;
        inertia_from_row(row(k), tot.I);
        lag_body_bias(tot.I, v[k], tot.B);
        if (k < LINKS - 1) lag_composite_add(tot, carry);
        if (k < NJ) {
            LagWrench F1, F2, F3;
            lag_joint_wrenches(tot, v[k], false, F1, F2, F3);
            if (WANT_G) gout(k, lag_gravity(F2, v[k]));
            if (WANT_H) hout(k, k, F2.n[2]);
            cout(k, k, F1.n[2]);
#pragma unroll
            for (int a = k - 1; a >= 0; --a) {
                const OpFT o = load_ft(row(a + 1));
                float J[9];
                if (a + 1 < NJ) {
                    joint_rot_z(o.F, cs[a + 1], sn[a + 1], J);
                } else {
#pragma unroll
                    for (int i = 0; i < 9; ++i) J[i] = o.F[i];
                }
                lag_wrench_up(J, o.t, F1);
                lag_wrench_up(J, o.t, F2);
                lag_wrench_up(J, o.t, F3);
                if (WANT_H) { hout(a, k, F2.n[2]); hout(k, a, F2.n[2]); }
                cout(a, k, F1.n[2]);
                cout(k, a, lag_axis_rate_dot(v[a], false, F2) + F3.n[2]);
            }
        }
        if (k > 0) {
            const OpFT o = load_ft(row(k));
            float J[9];
            if (k < NJ) {
                joint_rot_z(o.F, cs[k], sn[k], J);
            } else {
#pragma unroll
                for (int i = 0; i < 9; ++i) J[i] = o.F[i];
            }
            lag_composite_to_parent(J, o.t, tot, carry);
        }
    }
}
} // namespace drm

// drm_idd.hpp — include/drm_hip.h drm_rnea_derivatives: the per-row arithmetic of tau = ID(q, qd, qdd) and its first-order derivatives
// dtau/dq, dtau/dqd and dtau/dqdd = H(q) in ONE sweep out and one back over the tree (Carpentier and Mansard, "Analytical derivatives
// of rigid body dynamics algorithms", 2018; Singh, Russell and Wensing, "Efficient analytical derivatives of rigid-body dynamics using
// spatial vector algebra", 2022).  Shared by the kernels (drm_idd.hip) and by the host build (drm_cpu.cpp) so that both round the same
// way.  Kept out of drm_sample.hpp on purpose, as drm_lagrangian.hpp is: that header is part of the source key of every robot's own
// kernels (specialize._HEADERS).
//
// Frames and composites are those of drm_lagrangian.hpp: every quantity of link i in link i's OWN stored frame (joint about / along +z,
// child -> parent x_p = J x_c + t), spatial vectors as (angular, linear) at the link origin, IC the sub-tree's inertia (10 floats) and
// BC its bias matrix (12 floats).  On top of them travels fC, the sub-tree's wrench (6 floats).
//
//   forward   v_i = X v_parent + S_i qd_i,   a_i = X a_parent + S_i qdd_i + v_i x S_i qd_i     (a_base = (0, 0, +9.81) stands for gravity)
//   per body  IC_i = I_i,   BC_i = (crf(v) I - I crm(v) + bar(I v)) / 2,   fC_i = I a + v x* I v
//   backward  Pd_j = v_j x S_j,   Pdd_j = a_j x S_j + v_j x Pd_j      (d v_k / d q_j and the k-independent part of d a_k / d q_j for every
//                                                                      k below j, in coordinates that move with link j; the link's OWN
//                                                                      velocity and acceleration serve, since S_j x S_j = 0)
//             F1 = IC_j Pdd_j + 2 BC_j Pd_j + S_j x* fC_j     F2 = 2 (IC_j Pd_j + BC_j S_j)     F3 = BC_j^T S_j     F4 = IC_j S_j
//             tau_j = S_j . fC_j (+ damping_j qd_j)
//             up the ancestors i = j, parent(j), ... (the four wrenches moved by each joint transform on the way):
//                 dq[i, j] = S_i . F1       dqd[i, j] = S_i . F2 (+ damping_j where i = j)       H[i, j] = H[j, i] = S_i . F4
//                 dq[j, i] = 2 Pd_i . F3 + Pdd_i . F4       dqd[j, i] = 2 (S_i . F3 + Pd_i . F4)                              (i != j)
//             IC_parent += IC_j,  BC_parent += BC_j,  fC_parent += fC_j   (moved into the parent's frame)
// The part of d a_k / d q_j that depends on k (Pd_j x v_k) is what turns BC into 2 BC above.  F3 has no force part (BC^T S = (A^T e_z, 0)
// or (P x e_z, 0), drm_lagrangian.hpp), and a moment alone moves up by n' = J n.  Entries between joints on different branches are
// never formed: they are exact zeros, and the caller's to write.
#pragma once
#include "drm_lagrangian.hpp"

namespace drm {

constexpr int IDD_REC_FLOATS = 15;  // per op between the sweeps: cos, sin, value of the joint, w, u, al, a
constexpr int IDD_SLOT_FLOATS = 28; // per open branch point on the way back: the composite (IC: 10, BC: 12, fC: 6)

struct IddMotion {
    float w[3], u[3];  // angular, linear velocity
    float al[3], a[3]; // angular, linear acceleration
};
struct IddComposite {
    LagComposite c;
    LagWrench f;
};

DRM_HD void idd_motion_root(IddMotion &m, float g) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { m.w[i] = 0.0f; m.u[i] = 0.0f; m.al[i] = 0.0f; m.a[i] = 0.0f; }
    m.a[2] = g;
}
// velocity as lag_vel_step; al = J^T al_p (+ e_z qdd + w x e_z qd);  a = J^T (a_p + al_p x t) + u x e_z qd   (revolute)
//                                                                   a = J^T (a_p + al_p x t) + e_z qdd + w x e_z qd   (prismatic)
DRM_HD void idd_motion_step(const float *J, const float *t, float qd, float qdd, bool moving, bool prismatic, const IddMotion &par,
                            IddMotion &out) {
    float x[3], y[3];
    IddMotion N;
    matT_vec(J, par.w, N.w);
    cross3(par.w, t, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = par.u[i] + x[i];
    matT_vec(J, y, N.u);
    matT_vec(J, par.al, N.al);
    cross3(par.al, t, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = par.a[i] + x[i];
    matT_vec(J, y, N.a);
    if (moving) {
        if (prismatic) {
            N.u[2] += qd;
            N.a[2] += qdd;
            N.a[0] += N.w[1] * qd; N.a[1] -= N.w[0] * qd;
        } else {
            N.w[2] += qd;
            N.al[2] += qdd;
            N.al[0] += N.w[1] * qd; N.al[1] -= N.w[0] * qd;
            N.a[0] += N.u[1] * qd; N.a[1] -= N.u[0] * qd;
        }
    }
    out = N;
}

// I x for a motion x = (xa, xl):  n = I_o xa + h x xl,  f = m xl - h x xa
DRM_HD void idd_inertia_apply(const Inertia &I, const float *xa, const float *xl, LagWrench &F) {
    float Ia[3], hl[3], ha[3];
    lag_sym_vec(I.I, xa, Ia);
    cross3(I.h, xl, hl);
    cross3(I.h, xa, ha);
#pragma unroll
    for (int i = 0; i < 3; ++i) { F.n[i] = Ia[i] + hl[i]; F.f[i] = I.m * xl[i] - ha[i]; }
}

// one body: IC = I, BC from its velocity, fC = I a + v x* (I v)
DRM_HD void idd_body(const float *of, const IddMotion &m, IddComposite &c) {
    inertia_from_row(of, c.c.I);
    LagVel v;
#pragma unroll
    for (int i = 0; i < 3; ++i) { v.w[i] = m.w[i]; v.u[i] = m.u[i]; v.gd[i] = 0.0f; }
    lag_body_bias(c.c.I, v, c.c.B);
    LagWrench h, g;
    idd_inertia_apply(c.c.I, m.w, m.u, h);
    idd_inertia_apply(c.c.I, m.al, m.a, g);
    float wn[3], uf[3], wf[3];
    cross3(m.w, h.n, wn);
    cross3(m.u, h.f, uf);
    cross3(m.w, h.f, wf);
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.f.n[i] = g.n[i] + (wn[i] + uf[i]); c.f.f[i] = g.f[i] + wf[i]; }
}
DRM_HD void idd_composite_zero(IddComposite &c) {
    lag_composite_zero(c.c);
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.f.n[i] = 0.0f; c.f.f[i] = 0.0f; }
}
DRM_HD void idd_composite_add(IddComposite &a, const IddComposite &b) {
    lag_composite_add(a.c, b.c);
#pragma unroll
    for (int i = 0; i < 3; ++i) { a.f.n[i] += b.f.n[i]; a.f.f[i] += b.f.f[i]; }
}
DRM_HD void idd_composite_to_parent(const float *J, const float *t, const IddComposite &c, IddComposite &out) {
    lag_composite_to_parent(J, t, c.c, out.c);
    out.f = c.f;
    lag_wrench_up(J, t, out.f);
}
DRM_HD void idd_composite_to_floats(const IddComposite &c, float *v) {
    lag_composite_to_floats(c.c, v);
#pragma unroll
    for (int i = 0; i < 3; ++i) { v[22 + i] = c.f.n[i]; v[25 + i] = c.f.f[i]; }
}
DRM_HD void idd_composite_from_floats(const float *v, IddComposite &c) {
    lag_composite_from_floats(v, c.c);
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.f.n[i] = v[22 + i]; c.f.f[i] = v[25 + i]; }
}

// Pd = v x S and Pdd = a x S + v x Pd of the joint (about / along +z) of a link with motion m, as (angular, linear) halves
struct IddAxisRates {
    float da[3], dl[3], dda[3], ddl[3];
};
DRM_HD void idd_axis_rates(const IddMotion &m, bool prismatic, IddAxisRates &r) {
    float x[3], y[3];
    if (!prismatic) {
        r.da[0] = m.w[1]; r.da[1] = -m.w[0]; r.da[2] = 0.0f;
        r.dl[0] = m.u[1]; r.dl[1] = -m.u[0]; r.dl[2] = 0.0f;
        cross3(m.w, r.da, r.dda);
        r.dda[0] += m.al[1]; r.dda[1] -= m.al[0];
        cross3(m.w, r.dl, x);
        cross3(m.u, r.da, y);
        r.ddl[0] = (x[0] + y[0]) + m.a[1]; r.ddl[1] = (x[1] + y[1]) - m.a[0]; r.ddl[2] = x[2] + y[2];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) { r.da[i] = 0.0f; r.dda[i] = 0.0f; }
        r.dl[0] = m.w[1]; r.dl[1] = -m.w[0]; r.dl[2] = 0.0f;
        cross3(m.w, r.dl, r.ddl);
        r.ddl[0] += m.al[1]; r.ddl[1] -= m.al[0];
    }
}

// the four wrenches of joint j from the composites of its sub-tree and its link's motion; F3 is a moment alone
DRM_HD void idd_joint_wrenches(const IddComposite &c, const IddAxisRates &r, bool prismatic, LagWrench &F1, LagWrench &F2, float *F3,
                               LagWrench &F4) {
    const Inertia &I = c.c.I;
    const LagBias &B = c.c.B;
    LagWrench X;
    // IC Pdd + 2 BC Pd:  BC (x, y) = (A x, x x P)
    idd_inertia_apply(I, r.dda, r.ddl, F1);
    idd_inertia_apply(I, r.da, r.dl, X);
    if (!prismatic) {
        float Ax[3], xP[3];
        mat_vec(B.A, r.da, Ax);
        cross3(r.da, B.P, xP);
#pragma unroll
        for (int i = 0; i < 3; ++i) { F1.n[i] += 2.0f * Ax[i]; F1.f[i] += 2.0f * xP[i]; }
        // S x* fC = (e_z x n, e_z x f)
        F1.n[0] -= c.f.n[1]; F1.n[1] += c.f.n[0];
        F1.f[0] -= c.f.f[1]; F1.f[1] += c.f.f[0];
        // BC S = (A e_z, e_z x P)
        F2.n[0] = 2.0f * (X.n[0] + B.A[2]); F2.n[1] = 2.0f * (X.n[1] + B.A[5]); F2.n[2] = 2.0f * (X.n[2] + B.A[8]);
        F2.f[0] = 2.0f * (X.f[0] - B.P[1]); F2.f[1] = 2.0f * (X.f[1] + B.P[0]); F2.f[2] = 2.0f * X.f[2];
        F3[0] = B.A[6]; F3[1] = B.A[7]; F3[2] = B.A[8];
        F4.n[0] = I.I[2]; F4.n[1] = I.I[4]; F4.n[2] = I.I[5];
        F4.f[0] = -I.h[1]; F4.f[1] = I.h[0]; F4.f[2] = 0.0f;
    } else {
        // Pd has no angular part: BC Pd = 0;  S x* fC = (e_z x f, 0);  BC S = 0
        F1.n[0] -= c.f.f[1]; F1.n[1] += c.f.f[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) { F2.n[i] = 2.0f * X.n[i]; F2.f[i] = 2.0f * X.f[i]; }
        F3[0] = B.P[1]; F3[1] = -B.P[0]; F3[2] = 0.0f;
        F4.n[0] = I.h[1]; F4.n[1] = -I.h[0]; F4.n[2] = 0.0f;
        F4.f[0] = 0.0f; F4.f[1] = 0.0f; F4.f[2] = I.m;
    }
}
DRM_HD void idd_moment_up(const float *J, float *n) {
    float x[3];
    mat_vec(J, n, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = x[i];
}
DRM_HD float idd_dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// the entries of row j (the joint the wrenches belong to) in the column of ancestor i, whose axis rates are r
DRM_HD float idd_dq_below(const IddAxisRates &r, const float *F3, const LagWrench &F4) {
    return 2.0f * idd_dot3(r.da, F3) + (idd_dot3(r.dda, F4.n) + idd_dot3(r.ddl, F4.f));
}
DRM_HD float idd_dqd_below(const IddAxisRates &r, bool prismatic, const float *F3, const LagWrench &F4) {
    return 2.0f * ((prismatic ? 0.0f : F3[2]) + (idd_dot3(r.da, F4.n) + idd_dot3(r.dl, F4.f)));
}

// a row whose joint values, rates or accelerations cannot be used: the caller walks it at rest at q = 0 and hands out NaN
DRM_HD bool idd_bad_input(float q, float qd, float qdd) { return lag_bad_input(q, qd) || !(fabsf(qdd) <= 3.0e38f); }

DRM_HD void idd_record_pack(float c, float s, float q, const IddMotion &m, float *r) {
    r[0] = c; r[1] = s; r[2] = q;
#pragma unroll
    for (int i = 0; i < 3; ++i) { r[3 + i] = m.w[i]; r[6 + i] = m.u[i]; r[9 + i] = m.al[i]; r[12 + i] = m.a[i]; }
}
DRM_HD void idd_record_unpack(const float *r, float &c, float &s, float &q, IddMotion &m) {
    c = r[0]; s = r[1]; q = r[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) { m.w[i] = r[3 + i]; m.u[i] = r[6 + i]; m.al[i] = r[9 + i]; m.a[i] = r[12 + i]; }
}

constexpr int IDD_DQ = 0, IDD_DQD = 1, IDD_H = 2; // which matrix an entry belongs to

// ---------------------------------------------------------------------------------------------------------------------------
// ANY walk, one row: the ops [0, n_ops) in walk order, all segments by the one caller, in the structure of lagrangian_tree_walk.
//   g                                 9.81 with gravity, else 0;   damping: the joint dampings enter tau and the diagonal of dtau/dqd
//   qf(d, q, qd, qdd)                 joint value, rate and acceleration of DoF d (zeros for a row that is not to be used)
//   rput(k, const float *) / rget(k, float *)       the record of op k (IDD_REC_FLOATS)
//   sput(s, const float *) / sget(s, float *)       the composite parked in slot s (IDD_SLOT_FLOATS)
//   mout(which, i, j, v)              entry [i, j] of dtau/dq (IDD_DQ), dtau/dqd (IDD_DQD) or H (IDD_H, both triangles are handed over)
//   tout(j, v)                        tau by DoF
template <class CTL, class ROW, class QF, class RPUT, class RGET, class SPUT, class SGET, class MOUT, class TOUT>
DRM_HD void idd_tree_walk(int n_ops, int p_end, int n_slots, float g, bool damping, CTL ctl, ROW row, QF qf, RPUT rput, RGET rget,
                          SPUT sput, SGET sget, MOUT mout, TOUT tout) {
    float rec[IDD_REC_FLOATS], sl[IDD_SLOT_FLOATS];
    // ---- forward: velocities and accelerations --------------------------------------------------------------------------------
#pragma unroll 1
    for (int k = 0; k < n_ops; ++k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        float q = 0.0f, qd = 0.0f, qdd = 0.0f, c = 1.0f, s = 0.0f;
        if (ct.dof >= 0) {
            qf(ct.dof, q, qd, qdd);
            if (!ct.prismatic) sincos_one(q, s, c);
        }
        IddMotion par;
        if (ct.src == DRM_SRC_ROOT || ct.parent < 0 || ct.parent >= k) {
            idd_motion_root(par, g);
        } else {
            float pc, ps, pq;
            rget(ct.parent, rec);
            idd_record_unpack(rec, pc, ps, pq, par);
        }
        const OpFT o = load_ft(row(k));
        float J[9], t[3];
        joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
        IddMotion m;
        idd_motion_step(J, t, qd, qdd, ct.dof >= 0, ct.prismatic, par, m);
        idd_record_pack(c, s, q, m, rec);
        rput(k, rec);
    }
    // ---- back: composites, and every joint's wrenches up its ancestors ------------------------------------------------------
    IddComposite carry;
    idd_composite_zero(carry);
    idd_composite_to_floats(carry, sl);
#pragma unroll 1
    for (int s = 0; s < n_slots; ++s) sput(s, sl);
#pragma unroll 1
    for (int k = n_ops - 1; k >= p_end; --k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        const float *of = row(k);
        IddMotion m;
        float c, s, q;
        rget(k, rec);
        idd_record_unpack(rec, c, s, q, m);
        IddComposite tot;
        idd_body(of, m, tot);
        if (ct.child_next) idd_composite_add(tot, carry);
        if (ct.save >= 0 && ct.save < n_slots) { // take: add and reset
            IddComposite parked;
            sget(ct.save, sl);
            idd_composite_from_floats(sl, parked);
            idd_composite_add(tot, parked);
            IddComposite z;
            idd_composite_zero(z);
            idd_composite_to_floats(z, sl);
            sput(ct.save, sl);
        }
        const OpFT o = load_ft(of);
        float J[9], t[3];
        joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
        if (ct.dof >= 0) {
            IddAxisRates r;
            idd_axis_rates(m, ct.prismatic, r);
            LagWrench F1, F2, F4;
            float F3[3];
            idd_joint_wrenches(tot, r, ct.prismatic, F1, F2, F3, F4);
            float dmp = 0.0f;
            {
                float jq, jqd, jqdd;
                qf(ct.dof, jq, jqd, jqdd);
                const float t0 = lag_axis_dot(tot.f, ct.prismatic);
                if (damping) dmp = of[DRM_OPF_DAMP];
                tout(ct.dof, damping ? t0 + dmp * jqd : t0);
            }
            mout(IDD_DQ, ct.dof, ct.dof, lag_axis_dot(F1, ct.prismatic));
            mout(IDD_DQD, ct.dof, ct.dof, lag_axis_dot(F2, ct.prismatic) + dmp);
            mout(IDD_H, ct.dof, ct.dof, lag_axis_dot(F4, ct.prismatic));
            lag_wrench_up(J, t, F1);
            lag_wrench_up(J, t, F2);
            idd_moment_up(J, F3);
            lag_wrench_up(J, t, F4);
            int anc = ct.parent;
#pragma unroll 1
            while (anc >= p_end && anc < k) {
                int v0, v1;
                ctl_words(ctl, anc, v0, v1);
                const OpCtl ca = decode_ctl(v0, v1);
                IddMotion ma;
                float ac, as, aq;
                rget(anc, rec);
                idd_record_unpack(rec, ac, as, aq, ma);
                if (ca.dof >= 0) {
                    IddAxisRates ra;
                    idd_axis_rates(ma, ca.prismatic, ra);
                    const float h = lag_axis_dot(F4, ca.prismatic);
                    mout(IDD_H, ca.dof, ct.dof, h);
                    mout(IDD_H, ct.dof, ca.dof, h);
                    mout(IDD_DQ, ca.dof, ct.dof, lag_axis_dot(F1, ca.prismatic));
                    mout(IDD_DQD, ca.dof, ct.dof, lag_axis_dot(F2, ca.prismatic));
                    mout(IDD_DQ, ct.dof, ca.dof, idd_dq_below(ra, F3, F4));
                    mout(IDD_DQD, ct.dof, ca.dof, idd_dqd_below(ra, ca.prismatic, F3, F4));
                }
                if (ca.src == DRM_SRC_ROOT || ca.parent < p_end) break;
                const OpFT oa = load_ft(row(anc));
                float Ja[9], ta[3];
                joint_transform(oa, ca.dof >= 0, ca.prismatic, aq, ac, as, Ja, ta);
                lag_wrench_up(Ja, ta, F1);
                lag_wrench_up(Ja, ta, F2);
                idd_moment_up(Ja, F3);
                lag_wrench_up(Ja, ta, F4);
                anc = ca.parent;
            }
        }
        if (ct.src != DRM_SRC_ROOT && ct.parent >= p_end) {
            IddComposite up;
            idd_composite_to_parent(J, t, tot, up);
            if (ct.src >= 0) {
                if (ct.src < n_slots) {
                    IddComposite parked;
                    sget(ct.src, sl);
                    idd_composite_from_floats(sl, parked);
                    idd_composite_add(parked, up);
                    idd_composite_to_floats(parked, sl);
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
// line, on cos / sin the caller already has; ops NJ .. LINKS-1 are fixed.  Everything stays in registers: the motions of the links
// on the way out, one composite and four wrenches on the way back; the joint transforms are rebuilt from cos / sin and the table
// where they are used.  own(k): this caller forms the entries of joint k's row and column below the diagonal block it closes
// (always true for a lone wavefront; a block of wavefronts sharing a tile shares the joints out, every one repeating the rest).
template <int LINKS, int NJ, class ROW, class OWN, class MOUT, class TOUT>
DRM_HD void idd_chain_trig(ROW row, float g, bool damping, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ],
                           const float (&qdd)[NJ], OWN own, MOUT mout, TOUT tout) {
    IddMotion m[LINKS];
    {
        IddMotion cur;
        idd_motion_root(cur, g);
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
            idd_motion_step(J, o.t, k < NJ ? qd[k] : 0.0f, k < NJ ? qdd[k] : 0.0f, k < NJ, false, cur, cur);
            m[k] = cur;
        }
    }
    IddComposite carry;
#pragma unroll
    for (int k = LINKS - 1; k >= 0; --k) {
        DRM_RNEA_LINK_FENCE();
        IddComposite tot;
        idd_body(row(k), m[k], tot);
        if (k < LINKS - 1) idd_composite_add(tot, carry);
        if (k < NJ && own(k)) {
            IddAxisRates r;
            idd_axis_rates(m[k], false, r);
            LagWrench F1, F2, F4;
            float F3[3];
            idd_joint_wrenches(tot, r, false, F1, F2, F3, F4);
            const float dmp = damping ? row(k)[DRM_OPF_DAMP] : 0.0f;
            tout(k, damping ? tot.f.n[2] + dmp * qd[k] : tot.f.n[2]);
            mout(IDD_DQ, k, k, F1.n[2]);
            mout(IDD_DQD, k, k, F2.n[2] + dmp);
            mout(IDD_H, k, k, F4.n[2]);
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
                idd_moment_up(J, F3);
                lag_wrench_up(J, o.t, F4);
                IddAxisRates ra;
                idd_axis_rates(m[a], false, ra);
                mout(IDD_H, a, k, F4.n[2]);
                mout(IDD_H, k, a, F4.n[2]);
                mout(IDD_DQ, a, k, F1.n[2]);
                mout(IDD_DQD, a, k, F2.n[2]);
                mout(IDD_DQ, k, a, idd_dq_below(ra, F3, F4));
                mout(IDD_DQD, k, a, idd_dqd_below(ra, false, F3, F4));
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
            idd_composite_to_parent(J, o.t, tot, carry);
        }
    }
}
} // namespace drm

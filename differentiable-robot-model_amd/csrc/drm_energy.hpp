// drm_energy.hpp — include/drm_hip.h drm_energy: the per-row arithmetic of the kinetic energy T(q, qd), the potential energy V(q), the
// generalised momentum p = dT/dqd = H qd and the gradients dT/dq and dV/dq = g(q), in ONE sweep out and one back over the tree.  Shared
// by the kernels (drm_energy.hip) and by the host build (drm_cpu.cpp) so that both round the same way.  Kept out of drm_sample.hpp on
// purpose, as drm_lagrangian.hpp is: that header is part of the source key of every robot's own kernels (specialize._HEADERS).
//
// Frames and body forms are drm_lagrangian.hpp's: every quantity of link i in link i's OWN stored frame, spatial vectors as (angular,
// linear) at the link origin, the joint axes component picks.  No 6 x 6 composite and no acceleration sweep:
//
//   forward   v_i = X v_parent + S_i qd_i,  gd_i = J^T gd_parent                      lag_vel_step
//             z_i = z_parent + (gd_parent . t_i) / 9.81                               height of the link origin above the base's z = 0
//             h_i = I_i v_i = (I_o w + mc x u,  m u - mc x w)                          the body's momentum
//             T  += (w . h_i.n + u . h_i.f) / 2
//             V  += 9.81 m_i z_i + gd_i . mc_i                                        only where a joint moves the link (below)
//   backward  hC_j = h_j + sum over children (moved into j's frame)                   the momentum of joint j's sub-tree, 6 floats
//             (m, mc)C_j likewise                                                     mass and first moment of the sub-tree, 4 floats
//             p_j     = S_j . hC_j
//             dT/dq_j = Sd_j . hC_j = -S_j . (v_j x* hC_j)        with Sd_j = crm(v_j) S_j, lag_axis_rate_dot
//             g_j     = (IC_j S_j).f . gd_j                        lag_gravity of the force part (e_z x mc, or m e_z for a prismatic joint)
//
// dT/dq: pdot_j = S_j . (fC_j - v_j x* hC_j) and Lagrange's pdot_j = tau_j + dT/dq_j with tau_j = S_j . fC_j.
// V leaves out the links that no joint moves (the base and whatever is fixed to it, the static prefix of a split walk): they add a
// constant to V and nothing to the other four.
#pragma once
#include "drm_lagrangian.hpp"

namespace drm {

constexpr int ENERGY_REC_FLOATS = 14;  // per op between the sweeps: cos, sin, value of the joint, w, u, gd, z, moved (0 / 1)
constexpr int ENERGY_SLOT_FLOATS = 10; // per open branch point on the way back: the momentum (6), mass and first moment (4)
constexpr float ENERGY_INV_G = 1.0f / 9.81f;

struct EnergyComposite {
    LagWrench h;  // momentum (angular about the link origin, linear)
    float m;      // mass
    float mc[3];  // first moment
};

DRM_HD void energy_composite_zero(EnergyComposite &c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.h.n[i] = 0.0f; c.h.f[i] = 0.0f; c.mc[i] = 0.0f; }
    c.m = 0.0f;
}
DRM_HD void energy_composite_add(EnergyComposite &a, const EnergyComposite &b) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { a.h.n[i] += b.h.n[i]; a.h.f[i] += b.h.f[i]; a.mc[i] += b.mc[i]; }
    a.m += b.m;
}
DRM_HD void energy_composite_to_floats(const EnergyComposite &c, float *v) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { v[i] = c.h.n[i]; v[3 + i] = c.h.f[i]; v[7 + i] = c.mc[i]; }
    v[6] = c.m;
}
DRM_HD void energy_composite_from_floats(const float *v, EnergyComposite &c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.h.n[i] = v[i]; c.h.f[i] = v[3 + i]; c.mc[i] = v[7 + i]; }
    c.m = v[6];
}
// one body: its momentum I v, mass and first moment
DRM_HD void energy_body(const Inertia &I, const LagVel &v, EnergyComposite &c) {
    float Iw[3], hu[3], hw[3];
    lag_sym_vec(I.I, v.w, Iw);
    cross3(I.h, v.u, hu);
    cross3(I.h, v.w, hw);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c.h.n[i] = Iw[i] + hu[i];
        c.h.f[i] = I.m * v.u[i] - hw[i];
        c.mc[i] = I.h[i];
    }
    c.m = I.m;
}
// into the parent's frame, x_p = J x_c + t: the momentum as a wrench, mc' = J mc + m t (inertia_to_parent's first moment)
DRM_HD void energy_composite_to_parent(const float *J, const float *t, const EnergyComposite &c, EnergyComposite &out) {
    float g[3];
    EnergyComposite N = c;
    lag_wrench_up(J, t, N.h);
    mat_vec(J, c.mc, g);
#pragma unroll
    for (int i = 0; i < 3; ++i) N.mc[i] = g[i] + c.m * t[i];
    out = N;
}
DRM_HD float energy_height_step(const LagVel &par, const float *t, float z_par) {
    return z_par + (par.gd[0] * t[0] + par.gd[1] * t[1] + par.gd[2] * t[2]) * ENERGY_INV_G;
}
DRM_HD float energy_body_kinetic(const LagVel &v, const LagWrench &h) {
    return 0.5f * ((v.w[0] * h.n[0] + v.w[1] * h.n[1] + v.w[2] * h.n[2]) + (v.u[0] * h.f[0] + v.u[1] * h.f[1] + v.u[2] * h.f[2]));
}
DRM_HD float energy_body_potential(const Inertia &I, const LagVel &v, float z) {
    return 9.81f * I.m * z + (v.gd[0] * I.h[0] + v.gd[1] * I.h[1] + v.gd[2] * I.h[2]);
}
// T and V of one body from its row of the table
DRM_HD void energy_body_scalars(const float *of, const LagVel &v, float z, bool moved, float &T, float &V) {
    Inertia I;
    EnergyComposite c;
    inertia_from_row(of, I);
    energy_body(I, v, c);
    T += energy_body_kinetic(v, c.h);
    if (moved) V += energy_body_potential(I, v, z);
}
// the three entries of joint j (about / along +z of its frame) from the composite of its sub-tree and its link's velocity
DRM_HD void energy_joint(const EnergyComposite &c, const LagVel &v, bool prismatic, float &p, float &dT, float &g) {
    p = lag_axis_dot(c.h, prismatic);
    dT = lag_axis_rate_dot(v, prismatic, c.h);
    LagWrench F2; // the force part of IC S, as lag_joint_wrenches forms it
    if (!prismatic) { F2.f[0] = -c.mc[1]; F2.f[1] = c.mc[0]; F2.f[2] = 0.0f; }
    else { F2.f[0] = 0.0f; F2.f[1] = 0.0f; F2.f[2] = c.m; }
    g = lag_gravity(F2, v);
}

DRM_HD void energy_record_pack(float c, float s, float q, const LagVel &v, float z, bool moved, float *r) {
    lag_record_pack(c, s, q, v, r);
    r[12] = z;
    r[13] = moved ? 1.0f : 0.0f;
}
DRM_HD void energy_record_unpack(const float *r, float &c, float &s, float &q, LagVel &v, float &z, bool &moved) {
    lag_record_unpack(r, c, s, q, v);
    z = r[12];
    moved = r[13] != 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// ANY walk, one row: the ops [0, n_ops) in walk order, all segments by the one caller (lagrangian_tree_walk's structure).  The forward
// sweep leaves one record per op (ENERGY_REC_FLOATS) and hands out T and V; with `back` the sweep back carries the composite of a
// chain in registers and parks it at open branch points (ENERGY_SLOT_FLOATS per slot).
//   qf(d, q, qd)                      joint value and rate of DoF d (zeros for a row that is not to be used)
//   rput(k, const float *) / rget(k, float *)       the record of op k
//   sput(s, const float *) / sget(s, float *)       the composite parked in slot s
//   sout(T, V)      jout(dof, p, dT_dq, g)
template <class CTL, class ROW, class QF, class RPUT, class RGET, class SPUT, class SGET, class SOUT, class JOUT>
DRM_HD void energy_tree_walk(int n_ops, int p_end, int n_slots, bool back, CTL ctl, ROW row, QF qf, RPUT rput, RGET rget, SPUT sput, SGET sget,
                             SOUT sout, JOUT jout) {
    float rec[ENERGY_REC_FLOATS], sl[ENERGY_SLOT_FLOATS];
    // ---- forward: velocities, heights, T and V ----------------------------------------------------------------------------------
    float T = 0.0f, V = 0.0f;
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
        float z_par = 0.0f;
        bool moved = false;
        if (ct.src == DRM_SRC_ROOT || ct.parent < 0 || ct.parent >= k) {
            lag_vel_root(par);
        } else {
            float pc, ps, pq;
            rget(ct.parent, rec);
            energy_record_unpack(rec, pc, ps, pq, par, z_par, moved);
        }
        moved = moved || ct.dof >= 0;
        const float *of = row(k);
        const OpFT o = load_ft(of);
        float J[9], t[3];
        joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
        LagVel v;
        lag_vel_step(J, t, qd, ct.dof >= 0, ct.prismatic, par, v);
        const float z = energy_height_step(par, t, z_par);
        energy_body_scalars(of, v, z, moved, T, V);
        energy_record_pack(c, s, q, v, z, moved, rec);
        rput(k, rec);
    }
    sout(T, V);
    if (!back) return;
    // ---- back: the momentum, mass and first moment of every joint's sub-tree ---------------------------------------------------
    EnergyComposite carry;
    energy_composite_zero(carry);
    energy_composite_to_floats(carry, sl);
#pragma unroll 1
    for (int s = 0; s < n_slots; ++s) sput(s, sl);
#pragma unroll 1
    for (int k = n_ops - 1; k >= p_end; --k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        const float *of = row(k);
        LagVel v;
        float c, s, q, z;
        bool moved;
        rget(k, rec);
        energy_record_unpack(rec, c, s, q, v, z, moved);
        Inertia I;
        EnergyComposite tot;
        inertia_from_row(of, I);
        energy_body(I, v, tot);
        if (ct.child_next) energy_composite_add(tot, carry);
        if (ct.save >= 0 && ct.save < n_slots) { // take: add and reset
            EnergyComposite parked;
            sget(ct.save, sl);
            energy_composite_from_floats(sl, parked);
            energy_composite_add(tot, parked);
            EnergyComposite zero;
            energy_composite_zero(zero);
            energy_composite_to_floats(zero, sl);
            sput(ct.save, sl);
        }
        if (ct.dof >= 0) {
            float p, dT, g;
            energy_joint(tot, v, ct.prismatic, p, dT, g);
            jout(ct.dof, p, dT, g);
        }
        if (ct.src != DRM_SRC_ROOT && ct.parent >= p_end) {
            const OpFT o = load_ft(of);
            float J[9], t[3];
            joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
            EnergyComposite up;
            energy_composite_to_parent(J, t, tot, up);
            if (ct.src >= 0) {
                if (ct.src < n_slots) {
                    EnergyComposite parked;
                    sget(ct.src, sl);
                    energy_composite_from_floats(sl, parked);
                    energy_composite_add(parked, up);
                    energy_composite_to_floats(parked, sl);
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
// line, on cos / sin the caller already has; ops NJ .. LINKS-1 are fixed.  Everything stays in registers: the velocities and momenta of
// the links on the way out (the momenta are formed there for T and only summed on the way back), one composite on the way back; the joint transforms are rebuilt from cos / sin and the table where they are
// used.  BACK: without it the sweep back is not made (T and V alone).  Every link of such a chain is moved by joint 0.
template <int LINKS, int NJ, bool BACK, class ROW, class JOUT>
DRM_HD void energy_chain_trig(ROW row, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ], float &T_out, float &V_out,
                              JOUT jout) {
    LagVel v[BACK ? LINKS : 1];
    LagWrench hb[BACK ? LINKS : 1]; // the bodies' momenta: formed on the way out for T, summed on the way back
    float T = 0.0f, V = 0.0f;
    {
        LagVel cur;
        float z = 0.0f;
        lag_vel_root(cur);
#pragma unroll
        for (int k = 0; k < LINKS; ++k) {
            const float *of = row(k);
            const OpFT o = load_ft(of);
            float J[9];
            if (k < NJ) {
                joint_rot_z(o.F, cs[k], sn[k], J);
            } else {
#pragma unroll
                for (int i = 0; i < 9; ++i) J[i] = o.F[i];
            }
            z = energy_height_step(cur, o.t, z);
            lag_vel_step(J, o.t, k < NJ ? qd[k] : 0.0f, k < NJ, false, cur, cur);
            {
                Inertia I;
                EnergyComposite c;
                inertia_from_row(of, I);
                energy_body(I, cur, c);
                T += energy_body_kinetic(cur, c.h);
                V += energy_body_potential(I, cur, z);
                if constexpr (BACK) { v[k] = cur; hb[k] = c.h; }
            }
        }
    }
    T_out = T;
    V_out = V;
    if constexpr (BACK) {
        EnergyComposite carry;
#pragma unroll
        for (int k = LINKS - 1; k >= 0; --k) {
            DRM_RNEA_LINK_FENCE();
            const float *of = row(k);
            EnergyComposite tot;
            tot.h = hb[k];
            tot.m = of[DRM_OPF_MASS];
#pragma unroll
            for (int i = 0; i < 3; ++i) tot.mc[i] = of[DRM_OPF_MCOM + i];
            if (k < LINKS - 1) energy_composite_add(tot, carry);
            if (k < NJ) {
                float p, dT, g;
                energy_joint(tot, v[k], false, p, dT, g);
                jout(k, p, dT, g);
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
                energy_composite_to_parent(J, o.t, tot, carry);
            }
        }
    }
}
} // namespace drm

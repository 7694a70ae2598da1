// drm_links.hpp — include/drm_hip.h drm_link_motion and drm_external_torques: the per-row arithmetic of the links' positions, velocities
// and classical accelerations (one sweep outwards over a many-target FK walk) and of the joint torques of external wrenches on the
// links (the same sweep outwards for the poses, one inwards for the wrenches).  Shared by the kernels (drm_links.hip) and by the host
// build (drm_cpu.cpp) so that both round the same way.  Kept out of drm_sample.hpp on purpose, as drm_energy.hpp is: that header is
// part of the source key of every robot's own kernels (specialize._HEADERS).
//
// Frame: compute_endeffector_jacobian's — WORLD axes, at the link frame's origin.  A world-frame recursion needs no axis
// canonicalisation code: the joint axis is z = R e_z of the stored frame whatever DRM_OPI_PERM says.  With r = p - p_parent:
//
//   outwards   R = R_p J,  p = p_p + R_p t                                               (t includes a prismatic joint's slide)
//              revolute    w = w_p + z qd          v = v_p + w_p x r
//                          al = al_p + z qdd + w_p x z qd
//                          a = a_p + al_p x r + w_p x (w_p x r)
//              prismatic   w = w_p                 v = v_p + w_p x r + z qd
//                          al = al_p               a = a_p + al_p x r + w_p x (w_p x r) + z qdd + 2 w_p x z qd
//              fixed       transport only
//   inwards    F_k = f_k + sum over children F_c
//              M_k = m_k + sum over children (M_c + (p_c - p_k) x F_c)
//              tau_j = z_j . M_j   (z_j . F_j for a prismatic joint)
//
// v = lin_jac qd, w = ang_jac qd, a = d/dt v (gravity not included), al = d/dt w; tau = sum_l lin_jac_l^T f_l + ang_jac_l^T m_l.  The
// two sweeps are adjoint: sum_l f_l . v_l + m_l . w_l == tau . qd for every qd, so each serves as the other's exact backward pass.
// The q-gradient of that scalar (drm_link_power_dq) is the q-gradient of both: see link_joint_power_dq below.
#pragma once
#include "drm_lagrangian.hpp"

namespace drm {

constexpr int LINKS_SLOT_FLOATS = 24; // motion: the state of a branch point (R, p, w, v, al, a) parked for its later children
constexpr int LINKS_REC_FLOATS = 12;  // torques, per op: origin p, axis z, and the wrench (F, M) its children have handed up so far
constexpr int LINKS_DQ_REC_FLOATS = 21; // power gradient, per op: p, z, v, w, and (F, M, A) its children have handed up so far

struct LinkState {
    float R[9], p[3]; // world pose of the stored frame
    float w[3], v[3]; // angular velocity, velocity of the origin
    float al[3], a[3]; // their time derivatives
};
DRM_HD void link_state_root(LinkState &s) {
#pragma unroll
    for (int i = 0; i < 9; ++i) s.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) s.p[i] = s.w[i] = s.v[i] = s.al[i] = s.a[i] = 0.0f;
}
DRM_HD void link_state_to_floats(const LinkState &s, float *x) {
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] = s.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { x[9 + i] = s.p[i]; x[12 + i] = s.w[i]; x[15 + i] = s.v[i]; x[18 + i] = s.al[i]; x[21 + i] = s.a[i]; }
}
DRM_HD void link_state_from_floats(const float *x, LinkState &s) {
#pragma unroll
    for (int i = 0; i < 9; ++i) s.R[i] = x[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { s.p[i] = x[9 + i]; s.w[i] = x[12 + i]; s.v[i] = x[15 + i]; s.al[i] = x[18 + i]; s.a[i] = x[21 + i]; }
}

// a row that cannot be used (lag_bad_input's convention, with the acceleration)
DRM_HD bool links_bad_input(float q, float qd, float qdd) { return lag_bad_input(q, qd) || !(fabsf(qdd) <= 3.0e38f); }

// Every product-sum below is written with explicit fused multiply-adds.  Left to the compiler's contraction (-ffp-contract=fast), WHICH
// product of a sum is fused depends on the code around it, and the instantiations of one walk (positions alone, with velocities, with
// accelerations; fused and general) rounded positions differently in the last bit — outputs requested alone must equal those
// requested together to the bit.
DRM_HD float lk_dot(float a0, float a1, float a2, float b0, float b1, float b2) {
    return __builtin_fmaf(a2, b2, __builtin_fmaf(a1, b1, a0 * b0));
}
DRM_HD void lk_cross(const float *a, const float *b, float *out) {
    out[0] = __builtin_fmaf(a[1], b[2], -(a[2] * b[1]));
    out[1] = __builtin_fmaf(a[2], b[0], -(a[0] * b[2]));
    out[2] = __builtin_fmaf(a[0], b[1], -(a[1] * b[0]));
}
// joint transform of one op (drm_sample.hpp joint_transform: child -> parent, x_p = J x_c + t), on explicit fused multiply-adds
DRM_HD void link_joint_transform(const OpFT &o, bool moving, bool prismatic, float q, float c, float s, float *J, float *t) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float f0 = o.F[r * 3 + 0], f1 = o.F[r * 3 + 1];
        J[r * 3 + 0] = (moving && !prismatic) ? __builtin_fmaf(f0, c, f1 * s) : f0;
        J[r * 3 + 1] = (moving && !prismatic) ? __builtin_fmaf(f1, c, -(f0 * s)) : f1;
        J[r * 3 + 2] = o.F[r * 3 + 2];
    }
    const float d = (moving && prismatic) ? q : 0.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = __builtin_fmaf(o.F[r * 3 + 2], d, o.t[r]);
}

// One op outwards: `s` is the parent's state on entry and the op's on return.  (J, t) is the op's joint transform (a prismatic
// joint's slide in t).  VEL / ACC: whether the velocity / acceleration terms are formed at all.
template <bool VEL, bool ACC>
DRM_HD void link_step(const float *J, const float *t, bool moving, bool prismatic, float qd, float qdd, LinkState &s) {
    float r[3], R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r[i] = lk_dot(s.R[i * 3 + 0], s.R[i * 3 + 1], s.R[i * 3 + 2], t[0], t[1], t[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) R[i * 3 + c] = lk_dot(s.R[i * 3 + 0], s.R[i * 3 + 1], s.R[i * 3 + 2], J[c], J[3 + c], J[6 + c]);
    }
    const float z[3] = {R[2], R[5], R[8]};
    if constexpr (VEL) {
        float wr[3], wz[3];
        lk_cross(s.w, r, wr);
        lk_cross(s.w, z, wz);
        if constexpr (ACC) {
            float ar[3], wwr[3];
            lk_cross(s.al, r, ar);
            lk_cross(s.w, wr, wwr);
#pragma unroll
            for (int i = 0; i < 3; ++i) s.a[i] = (s.a[i] + ar[i]) + wwr[i];
            if (moving && prismatic) {
#pragma unroll
                for (int i = 0; i < 3; ++i) s.a[i] += __builtin_fmaf(z[i], qdd, 2.0f * (wz[i] * qd));
            } else if (moving) {
#pragma unroll
                for (int i = 0; i < 3; ++i) s.al[i] += __builtin_fmaf(z[i], qdd, wz[i] * qd);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) s.v[i] += wr[i];
        if (moving && prismatic) {
#pragma unroll
            for (int i = 0; i < 3; ++i) s.v[i] = __builtin_fmaf(z[i], qd, s.v[i]);
        } else if (moving) {
#pragma unroll
            for (int i = 0; i < 3; ++i) s.w[i] = __builtin_fmaf(z[i], qd, s.w[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) s.R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) s.p[i] += r[i];
}

// the wrench (F, M) of a child at origin pc, handed to its parent at origin pp:  Fp += F,  Mp += M + (pc - pp) x F
DRM_HD void link_wrench_up(const float *pc, const float *pp, const float *F, const float *M, float *Fp, float *Mp) {
    const float d[3] = {pc[0] - pp[0], pc[1] - pp[1], pc[2] - pp[2]};
    float dF[3];
    lk_cross(d, F, dF);
#pragma unroll
    for (int i = 0; i < 3; ++i) { Fp[i] += F[i]; Mp[i] += M[i] + dF[i]; }
}
DRM_HD float link_joint_torque(const float *z, const float *F, const float *M, bool prismatic) {
    return prismatic ? lk_dot(z[0], z[1], z[2], F[0], F[1], F[2]) : lk_dot(z[0], z[1], z[2], M[0], M[1], M[2]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// ANY many-target FK walk, one row, outwards: the ops [0, n_ops) in walk order; the state of a chain is carried, parked at branch
// points (DRM_OPI_SAVE) and taken up again by their later children (DRM_OPI_SRC).
//   qf(d, q, qd, qdd)                 joint value, rate and acceleration of DoF d (zeros for a row that is not to be used)
//   sput(s, const float *) / sget(s, float *)       the state parked in slot s (LINKS_SLOT_FLOATS)
//   emit(t, const LinkState &)        the state of the op whose output slot is t
template <bool VEL, bool ACC, class CTL, class ROW, class QF, class SPUT, class SGET, class EMIT>
DRM_HD void link_motion_walk(int n_ops, int n_slots, CTL ctl, ROW row, QF qf, SPUT sput, SGET sget, EMIT emit) {
    float sl[LINKS_SLOT_FLOATS];
    LinkState cur;
    link_state_root(cur);
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
        if (ct.src == DRM_SRC_ROOT) {
            link_state_root(cur);
        } else if (ct.src >= 0 && ct.src < n_slots) {
            sget(ct.src, sl);
            link_state_from_floats(sl, cur);
        }
        const OpFT o = load_ft(row(k));
        float J[9], t[3];
        link_joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
        link_step<VEL, ACC>(J, t, ct.dof >= 0, ct.prismatic, qd, qdd, cur);
        if (ct.save >= 0 && ct.save < n_slots) {
            link_state_to_floats(cur, sl);
            sput(ct.save, sl);
        }
        if (ct.out >= 0) emit(ct.out, cur);
    }
}

// The same walk for the torques of external wrenches, one row.  Outwards it leaves (p, z) and a zero (F, M) accumulator per op
// (LINKS_REC_FLOATS); inwards op k adds its own wrench, hands the joint's torque out and the total to its parent's accumulator
// (the parent is DRM_OPI_W1's op index: no slots on the way back).  The pose is carried and parked as in link_motion_walk.
//   qf(d)                              joint value of DoF d
//   rput(k, const float *) / rget(k, float *)       the record of op k
//   wrench(t, f[3], m[3])              the wrench on the link of output slot t
//   jout(dof, tau)
template <class CTL, class ROW, class QF, class RPUT, class RGET, class SPUT, class SGET, class WRENCH, class JOUT>
DRM_HD void link_torques_walk(int n_ops, int n_slots, CTL ctl, ROW row, QF qf, RPUT rput, RGET rget, SPUT sput, SGET sget, WRENCH wrench,
                              JOUT jout) {
    float sl[LINKS_SLOT_FLOATS], rec[LINKS_REC_FLOATS];
    {
        LinkState cur;
        link_state_root(cur);
#pragma unroll 1
        for (int k = 0; k < n_ops; ++k) {
            int w0, w1;
            ctl_words(ctl, k, w0, w1);
            const OpCtl ct = decode_ctl(w0, w1);
            float q = 0.0f, c = 1.0f, s = 0.0f;
            if (ct.dof >= 0) {
                q = qf(ct.dof);
                if (!ct.prismatic) sincos_one(q, s, c);
            }
            if (ct.src == DRM_SRC_ROOT) {
                link_state_root(cur);
            } else if (ct.src >= 0 && ct.src < n_slots) {
                sget(ct.src, sl);
                link_state_from_floats(sl, cur);
            }
            const OpFT o = load_ft(row(k));
            float J[9], t[3];
            link_joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
            link_step<false, false>(J, t, ct.dof >= 0, ct.prismatic, 0.0f, 0.0f, cur);
            if (ct.save >= 0 && ct.save < n_slots) {
                link_state_to_floats(cur, sl);
                sput(ct.save, sl);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) { rec[i] = cur.p[i]; rec[3 + i] = cur.R[3 * i + 2]; rec[6 + i] = 0.0f; rec[9 + i] = 0.0f; }
            rput(k, rec);
        }
    }
#pragma unroll 1
    for (int k = n_ops - 1; k >= 0; --k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        rget(k, rec);
        float F[3] = {rec[6], rec[7], rec[8]}, M[3] = {rec[9], rec[10], rec[11]};
        if (ct.out >= 0) {
            float f[3], m[3];
            wrench(ct.out, f, m);
#pragma unroll
            for (int i = 0; i < 3; ++i) { F[i] += f[i]; M[i] += m[i]; }
        }
        if (ct.dof >= 0) jout(ct.dof, link_joint_torque(rec + 3, F, M, ct.prismatic));
        if (ct.parent >= 0 && ct.parent < k) {
            float par[LINKS_REC_FLOATS];
            rget(ct.parent, par);
            link_wrench_up(rec, par, F, M, par + 6, par + 9);
            rput(ct.parent, par);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same on a serial chain whose first NJ ops are revolute joints driving DoF columns 0 .. NJ-1 (DRM_WALK_ARM_CHAIN) and whose ops
// NJ .. LINKS-1 are fixed, every op a target (slot k = op k), straight line on cos / sin the caller already has.  Everything stays in
// registers.
template <int LINKS, int NJ, bool VEL, bool ACC, class ROW, class EMIT>
DRM_HD void link_chain_motion(ROW row, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ], const float (&qdd)[NJ], EMIT emit) {
    LinkState cur;
    link_state_root(cur);
#pragma unroll
    for (int k = 0; k < LINKS; ++k) {
        const OpFT o = load_ft(row(k));
        float J[9], t[3];
        link_joint_transform(o, k < NJ, false, 0.0f, k < NJ ? cs[k] : 1.0f, k < NJ ? sn[k] : 0.0f, J, t);
        link_step<VEL, ACC>(J, t, k < NJ, false, k < NJ ? qd[k] : 0.0f, k < NJ ? qdd[k] : 0.0f, cur);
        emit(k, cur);
    }
}

//   wrench(k, f[3], m[3])   the wrench on op k's link        jout(dof, tau)
template <int LINKS, int NJ, class ROW, class WRENCH, class JOUT>
DRM_HD void link_chain_torques(ROW row, const float (&cs)[NJ], const float (&sn)[NJ], WRENCH wrench, JOUT jout) {
    float p[LINKS][3], z[NJ][3];
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
            }
        }
    }
    float Fc[3] = {0.0f, 0.0f, 0.0f}, Mc[3] = {0.0f, 0.0f, 0.0f}; // what op k + 1 hands up, about op k's origin
#pragma unroll
    for (int k = LINKS - 1; k >= 0; --k) {
        float F[3], M[3];
        wrench(k, F, M);
#pragma unroll
        for (int i = 0; i < 3; ++i) { F[i] += Fc[i]; M[i] += Mc[i]; }
        if (k < NJ) jout(k, link_joint_torque(z[k < NJ ? k : 0], F, M, false));
        if (k > 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { Fc[i] = 0.0f; Mc[i] = 0.0f; }
            link_wrench_up(p[k], p[k > 0 ? k - 1 : 0], F, M, Fc, Mc);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// include/drm_hip.h drm_link_power_dq: the q-gradient of the power of the wrenches,
//   S(q; qd, F, M) = sum_l F_l . v_l + M_l . w_l = tau_ext(q; F, M) . qd,
// with the rates and the wrenches held fixed.  It is the q-gradient of BOTH sweeps above: of the velocities with (F, M) := their
// cotangents, of the torques with qd := theirs.  Turning joint j turns its sub-tree rigidly about (p_j, z_j): what the sub-tree's own
// joints add to a velocity turns with it, what the joints before j add is the parent's velocity field read at a moved point.  With
// F^S_j, M^S_j the sub-tree's wrench about p_j (the inward sweep of the torques) and one more FREE vector carried inwards,
//   A_k = v_k x F_k + w_k x M_k + sum over children A_c                                 (no transport)
//   revolute    dS/dq_j = z_j . (A_j - v_j x F^S_j) + (w_j x z_j) . M^S_j               (w_j x z_j == w_parent x z_j)
//   prismatic   dS/dq_j = (w_j x z_j) . F^S_j
//   fixed       transport only
// so no kinematic Hessian is formed.  The inward sweep forms F^S, M^S by link_torques_walk's own operations in its own order: the
// torques it hands out next to the gradient are drm_external_torques' to the bit.
DRM_HD float link_joint_power_dq(const float *z, const float *v, const float *w, const float *F, const float *M, const float *A,
                                 bool prismatic) {
    float wz[3], vF[3];
    lk_cross(w, z, wz);
    lk_cross(v, F, vF);
    const float t0 = A[0] - vF[0], t1 = A[1] - vF[1], t2 = A[2] - vF[2];
    const float slide = lk_dot(wz[0], wz[1], wz[2], F[0], F[1], F[2]);
    const float turn = __builtin_fmaf(z[2], t2, __builtin_fmaf(z[1], t1, __builtin_fmaf(z[0], t0, lk_dot(wz[0], wz[1], wz[2], M[0], M[1], M[2]))));
    return prismatic ? slide : turn;
}
// A += v x f + w x m: the link's own term of the free vector
DRM_HD void link_power_own(const float *v, const float *w, const float *f, const float *m, float *A) {
    float vf[3], wm[3];
    lk_cross(v, f, vf);
    lk_cross(w, m, wm);
#pragma unroll
    for (int i = 0; i < 3; ++i) A[i] += vf[i] + wm[i];
}

// ANY many-target FK walk, one row.  Outwards link_motion_walk's sweep with the velocities, leaving (p, z, v, w) and zero (F, M, A)
// accumulators per op (LINKS_DQ_REC_FLOATS); inwards link_torques_walk's sweep with A beside the wrench.
//   qf(d, q, qd)                       joint value and rate of DoF d
//   rput / rget, sput / sget, wrench   as link_torques_walk's (records of LINKS_DQ_REC_FLOATS)
//   jout(dof, dS/dq, tau)
template <class CTL, class ROW, class QF, class RPUT, class RGET, class SPUT, class SGET, class WRENCH, class JOUT>
DRM_HD void link_power_dq_walk(int n_ops, int n_slots, CTL ctl, ROW row, QF qf, RPUT rput, RGET rget, SPUT sput, SGET sget, WRENCH wrench,
                               JOUT jout) {
    float sl[LINKS_SLOT_FLOATS], rec[LINKS_DQ_REC_FLOATS];
    {
        LinkState cur;
        link_state_root(cur);
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
            if (ct.src == DRM_SRC_ROOT) {
                link_state_root(cur);
            } else if (ct.src >= 0 && ct.src < n_slots) {
                sget(ct.src, sl);
                link_state_from_floats(sl, cur);
            }
            const OpFT o = load_ft(row(k));
            float J[9], t[3];
            link_joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
            link_step<true, false>(J, t, ct.dof >= 0, ct.prismatic, qd, 0.0f, cur);
            if (ct.save >= 0 && ct.save < n_slots) {
                link_state_to_floats(cur, sl);
                sput(ct.save, sl);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                rec[i] = cur.p[i]; rec[3 + i] = cur.R[3 * i + 2]; rec[6 + i] = cur.v[i]; rec[9 + i] = cur.w[i];
                rec[12 + i] = 0.0f; rec[15 + i] = 0.0f; rec[18 + i] = 0.0f;
            }
            rput(k, rec);
        }
    }
#pragma unroll 1
    for (int k = n_ops - 1; k >= 0; --k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        rget(k, rec);
        float F[3] = {rec[12], rec[13], rec[14]}, M[3] = {rec[15], rec[16], rec[17]}, A[3] = {rec[18], rec[19], rec[20]};
        if (ct.out >= 0) {
            float f[3], m[3];
            wrench(ct.out, f, m);
            link_power_own(rec + 6, rec + 9, f, m, A);
#pragma unroll
            for (int i = 0; i < 3; ++i) { F[i] += f[i]; M[i] += m[i]; }
        }
        if (ct.dof >= 0)
            jout(ct.dof, link_joint_power_dq(rec + 3, rec + 6, rec + 9, F, M, A, ct.prismatic), link_joint_torque(rec + 3, F, M, ct.prismatic));
        if (ct.parent >= 0 && ct.parent < k) {
            float par[LINKS_DQ_REC_FLOATS];
            rget(ct.parent, par);
            link_wrench_up(rec, par, F, M, par + 12, par + 15);
#pragma unroll
            for (int i = 0; i < 3; ++i) par[18 + i] += A[i];
            rput(ct.parent, par);
        }
    }
}

// The same on the serial chain of link_chain_torques, everything in registers.
//   wrench(k, f[3], m[3])   the wrench on op k's link        jout(dof, dS/dq, tau)
template <int LINKS, int NJ, class ROW, class WRENCH, class JOUT>
DRM_HD void link_chain_power_dq(ROW row, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ], WRENCH wrench, JOUT jout) {
    float p[LINKS][3], v[LINKS][3], w[LINKS][3], z[NJ][3];
    {
        LinkState cur;
        link_state_root(cur);
#pragma unroll
        for (int k = 0; k < LINKS; ++k) {
            const OpFT o = load_ft(row(k));
            float J[9], t[3];
            link_joint_transform(o, k < NJ, false, 0.0f, k < NJ ? cs[k] : 1.0f, k < NJ ? sn[k] : 0.0f, J, t);
            link_step<true, false>(J, t, k < NJ, false, k < NJ ? qd[k] : 0.0f, 0.0f, cur);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                p[k][i] = cur.p[i]; v[k][i] = cur.v[i]; w[k][i] = cur.w[i];
                if (k < NJ) z[k < NJ ? k : 0][i] = cur.R[3 * i + 2];
            }
        }
    }
    float Fc[3] = {0.0f, 0.0f, 0.0f}, Mc[3] = {0.0f, 0.0f, 0.0f}, A[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = LINKS - 1; k >= 0; --k) {
        float F[3], M[3];
        wrench(k, F, M);
        link_power_own(v[k], w[k], F, M, A);
#pragma unroll
        for (int i = 0; i < 3; ++i) { F[i] += Fc[i]; M[i] += Mc[i]; }
        if (k < NJ) jout(k, link_joint_power_dq(z[k < NJ ? k : 0], v[k], w[k], F, M, A, false), link_joint_torque(z[k < NJ ? k : 0], F, M, false));
        if (k > 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { Fc[i] = 0.0f; Mc[i] = 0.0f; }
            link_wrench_up(p[k], p[k > 0 ? k - 1 : 0], F, M, Fc, Mc);
        }
    }
}
} // namespace drm

// drm_whole_body.hpp — include/drm_hip_whole_body.h drm_whole_body: the per-row arithmetic of what the robot does AS A WHOLE — its
// centre of mass, the CoM's velocity, acceleration and Jacobian, the angular momentum about the base origin and the wrench the mount
// applies to the base link — in ONE sweep out and one back over the tree.  Shared by the kernels (drm_whole_body.hip) and by the host
// build (drm_cpu.cpp) so that both round the same way.  Kept out of drm_sample.hpp on purpose, as drm_energy.hpp is: that header is
// part of the source key of every robot's own kernels (specialize._HEADERS).
//
// Frames and body forms are drm_energy.hpp's: every quantity of link i in link i's OWN stored frame, spatial vectors as (angular,
// linear) at the link origin, the joint axes component picks.  Gravity is NOT folded into the base acceleration here (com_acc wants none):
// its weight terms are added from the total mass and first moment at the root.
//
//   outwards  v_i = X v_p + S_i qd_i                                                    (w, u)
//             a_i = X a_p + S_i qdd_i + v_i x S_i qd_i                                  spatial acceleration (al, a)
//             R_i = R_p J,  p_i = p_p + R_p t                                           world pose of the stored frame (general walk)
//   per body  h_i = I_i v_i = (I_o w + mc x u,  m u - mc x w)                           momentum
//             f_i = I_i a_i + v_i x* h_i                                                its rate of change
//   back      (h, f, m, mc)C_j = own + sum over children (moved into j's frame)         16 floats; only bodies that a joint moves
//             com_jac[:, j] = R_j (e_z x mcC_j) / M   (R_j e_z mC_j / M for a prismatic joint)
//             The general walk, which carries every link's world pose, keeps (m, mc) in BASE axes about the base origin instead
//             (own: m p_i + R_i mc_i, no transport) and forms z_j x (mcC_j - mC_j p_j) / M.  A first moment in a link's frame is
//             rounded at the size of its largest component, which for a tall robot is the height; in base axes the horizontal
//             components, which are what the static moment and the ZMP read and which nearly cancel against the base share on a
//             mobile manipulator, keep their own (tests/test_whole_body.py has Fetch's figures).
//   root      the composites moved into the base frame: sum m c, the momentum (angular about the base origin), its rate
//             com = (sum m c + base share) / M      com_vel = h.f / M      ang_mom = h.n      com_acc = f.f / M
//             force = f.f + [gravity] M g e_z       moment = f.n + [gravity] (sum m c) x g e_z
//
// The base and whatever is fixed to it (the static prefix of a split walk, fixed ops before the first joint) move with nothing: the
// caller hands their mass and first moment in as the base share.
//
// Every product-sum is written with explicit fused multiply-adds, as drm_links.hpp's are and for its reason: the three levels of one
// walk (positions alone, with velocities, with accelerations) must round what they share the same way — outputs requested alone equal
// those requested together to the bit.
#pragma once
#include "drm_energy.hpp"
#include "drm_links.hpp"

namespace drm {

// LEVEL 0: positions (com, com_jac, the static wrench); 1: + velocities (com_vel, ang_mom); 2: + accelerations (com_acc, the wrench)
constexpr int wb_rec_floats(int level) { return 16 + 6 * level; }  // cos, sin, value of the joint, R, p, moved; + (w, u); + (al, a)
constexpr int wb_slot_floats(int level) { return 4 + 6 * level; }  // m, mc; + momentum; + its rate

// An anchor for the straight-line sweeps (device code only).  The arithmetic of a link has no place of its own between the link
// fences: instruction selection orders only what touches memory, and without stores the constant reads of ALL links gather ahead of
// the first link's arithmetic (300 - 490 live registers).  An empty asm statement that takes a link's results holds them, and what they
// depend on, in that link's slot.
#if defined(__HIP_DEVICE_COMPILE__)
#define DRM_WB_ANCHOR(x) asm volatile("" : "+v"(x))
#else
#define DRM_WB_ANCHOR(x) ((void)0)
#endif

struct WbMotion {
    float w[3], u[3];  // spatial velocity
    float al[3], a[3]; // spatial acceleration
};
struct WbComposite {
    float m, mc[3];
    LagWrench h; // momentum
    LagWrench f; // its rate of change
};
struct WbRoot {
    float M, inv_M; // the total mass: the moved bodies' (summed on the way out) and the base share's
    WbComposite c; // in the base frame
};
// what a row hands out, all in base axes
struct WbOut {
    float com[3], com_vel[3], com_acc[3], ang_mom[3], force[3], moment[3];
};

DRM_HD void wb_mat_vec(const float *M, const float *x, float *y) {
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = lk_dot(M[r * 3 + 0], M[r * 3 + 1], M[r * 3 + 2], x[0], x[1], x[2]);
}
DRM_HD void wb_matT_vec(const float *M, const float *x, float *y) {
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = lk_dot(M[c], M[3 + c], M[6 + c], x[0], x[1], x[2]);
}
DRM_HD void wb_sym_vec(const float *I, const float *x, float *y) {
    y[0] = lk_dot(I[0], I[1], I[2], x[0], x[1], x[2]);
    y[1] = lk_dot(I[1], I[3], I[4], x[0], x[1], x[2]);
    y[2] = lk_dot(I[2], I[4], I[5], x[0], x[1], x[2]);
}
DRM_HD void wb_motion_zero(WbMotion &v) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { v.w[i] = 0.0f; v.u[i] = 0.0f; v.al[i] = 0.0f; v.a[i] = 0.0f; }
}
DRM_HD void wb_wrench_zero(LagWrench &F) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { F.n[i] = 0.0f; F.f[i] = 0.0f; }
}
DRM_HD void wb_composite_zero(WbComposite &c) {
    c.m = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.mc[i] = 0.0f;
    wb_wrench_zero(c.h);
    wb_wrench_zero(c.f);
}
template <int LEVEL>
DRM_HD void wb_composite_add(WbComposite &a, const WbComposite &b) {
    a.m += b.m;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a.mc[i] += b.mc[i];
        if constexpr (LEVEL >= 1) { a.h.n[i] += b.h.n[i]; a.h.f[i] += b.h.f[i]; }
        if constexpr (LEVEL >= 2) { a.f.n[i] += b.f.n[i]; a.f.f[i] += b.f.f[i]; }
    }
}
template <int LEVEL>
DRM_HD void wb_composite_to_floats(const WbComposite &c, float *v) {
    v[0] = c.m;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[1 + i] = c.mc[i];
        if constexpr (LEVEL >= 1) { v[4 + i] = c.h.n[i]; v[7 + i] = c.h.f[i]; }
        if constexpr (LEVEL >= 2) { v[10 + i] = c.f.n[i]; v[13 + i] = c.f.f[i]; }
    }
}
template <int LEVEL>
DRM_HD void wb_composite_from_floats(const float *v, WbComposite &c) {
    wb_composite_zero(c);
    c.m = v[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c.mc[i] = v[1 + i];
        if constexpr (LEVEL >= 1) { c.h.n[i] = v[4 + i]; c.h.f[i] = v[7 + i]; }
        if constexpr (LEVEL >= 2) { c.f.n[i] = v[10 + i]; c.f.f[i] = v[13 + i]; }
    }
}

// One op outwards in link-local frames (lag_vel_step with the acceleration): `v` is the parent's motion on entry, the op's on return.
template <int LEVEL>
DRM_HD void wb_motion_step(const float *J, const float *t, bool moving, bool prismatic, float qd, float qdd, WbMotion &v) {
    if constexpr (LEVEL >= 1) {
        float x[3], y[3], w[3], u[3];
        wb_matT_vec(J, v.w, w);
        lk_cross(v.w, t, x);
#pragma unroll
        for (int i = 0; i < 3; ++i) y[i] = v.u[i] + x[i];
        wb_matT_vec(J, y, u);
        if constexpr (LEVEL >= 2) {
            float al[3], a[3];
            wb_matT_vec(J, v.al, al);
            lk_cross(v.al, t, x);
#pragma unroll
            for (int i = 0; i < 3; ++i) y[i] = v.a[i] + x[i];
            wb_matT_vec(J, y, a);
            // + S qdd + v x S qd:  revolute ((w_y, -w_x, qdd'), (u_y, -u_x, 0)) qd;  prismatic (0, (w_y, -w_x, qdd'))
            if (moving && prismatic) {
                a[0] = __builtin_fmaf(w[1], qd, a[0]);
                a[1] = __builtin_fmaf(-w[0], qd, a[1]);
                a[2] += qdd;
            } else if (moving) {
                al[0] = __builtin_fmaf(w[1], qd, al[0]);
                al[1] = __builtin_fmaf(-w[0], qd, al[1]);
                al[2] += qdd;
                a[0] = __builtin_fmaf(u[1], qd, a[0]);
                a[1] = __builtin_fmaf(-u[0], qd, a[1]);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) { v.al[i] = al[i]; v.a[i] = a[i]; }
        }
        if (moving && prismatic) u[2] += qd;
        else if (moving) w[2] += qd;
#pragma unroll
        for (int i = 0; i < 3; ++i) { v.w[i] = w[i]; v.u[i] = u[i]; }
    }
}

// one body: mass, first moment, momentum I v and its rate I a + v x* (I v)
template <int LEVEL>
DRM_HD void wb_body(const float *of, const WbMotion &v, WbComposite &c) {
    wb_composite_zero(c);
    Inertia I;
    inertia_from_row(of, I);
    c.m = I.m;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.mc[i] = I.h[i];
    if constexpr (LEVEL >= 1) {
        float Iw[3], hu[3], hw[3];
        wb_sym_vec(I.I, v.w, Iw);
        lk_cross(I.h, v.u, hu);
        lk_cross(I.h, v.w, hw);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            c.h.n[i] = Iw[i] + hu[i];
            c.h.f[i] = __builtin_fmaf(I.m, v.u[i], -hw[i]);
        }
        if constexpr (LEVEL >= 2) {
            float Ia[3], ha[3], hal[3], wn[3], up[3], wp[3];
            wb_sym_vec(I.I, v.al, Ia);
            lk_cross(I.h, v.a, ha);
            lk_cross(I.h, v.al, hal);
            lk_cross(v.w, c.h.n, wn);
            lk_cross(v.u, c.h.f, up);
            lk_cross(v.w, c.h.f, wp);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                c.f.n[i] = (Ia[i] + ha[i]) + (wn[i] + up[i]);
                c.f.f[i] = __builtin_fmaf(I.m, v.a[i], -hal[i]) + wp[i];
            }
        }
    }
}
// a wrench through x_p = J x_c + t:  f' = J f,  n' = J n + t x f'
DRM_HD void wb_wrench_up(const float *J, const float *t, LagWrench &F) {
    float f[3], n[3], x[3];
    wb_mat_vec(J, F.f, f);
    wb_mat_vec(J, F.n, n);
    lk_cross(t, f, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) { F.f[i] = f[i]; F.n[i] = n[i] + x[i]; }
}
// the composite through x_p = J x_c + t (into the parent's frame; with the link's world pose, into the base frame).  MC_MOVES: the
// first moment goes with it; otherwise it is kept as it is (the general walk's, which is in base axes about the base origin already)
template <int LEVEL, bool MC_MOVES = true>
DRM_HD void wb_composite_up(const float *J, const float *t, const WbComposite &c, WbComposite &out) {
    WbComposite N = c;
    if constexpr (MC_MOVES) {
        float g[3];
        wb_mat_vec(J, c.mc, g);
#pragma unroll
        for (int i = 0; i < 3; ++i) N.mc[i] = __builtin_fmaf(c.m, t[i], g[i]);
    }
    if constexpr (LEVEL >= 1) wb_wrench_up(J, t, N.h);
    if constexpr (LEVEL >= 2) wb_wrench_up(J, t, N.f);
    out = N;
}
// the CoM Jacobian's column of a joint about / along +z of its frame, in that frame and not yet divided by M
DRM_HD void wb_column(const WbComposite &c, bool prismatic, float *col) {
    col[0] = prismatic ? 0.0f : -c.mc[1];
    col[1] = prismatic ? 0.0f : c.mc[0];
    col[2] = prismatic ? c.m : 0.0f;
}
// the sums in the base frame -> the row's outputs.  `base`: mass and first moment of the bodies no joint moves (zeros: left out)
template <int LEVEL>
DRM_HD void wb_finish(const WbRoot &r, const float *base, bool gravity, WbOut &o) {
    const float M = r.M, inv_M = r.inv_M;
    const float mc[3] = {r.c.mc[0] + base[1], r.c.mc[1] + base[2], r.c.mc[2] + base[3]};
    const float g = gravity ? 9.81f : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.com[i] = mc[i] * inv_M;
        o.com_vel[i] = LEVEL >= 1 ? r.c.h.f[i] * inv_M : 0.0f;
        o.ang_mom[i] = LEVEL >= 1 ? r.c.h.n[i] : 0.0f;
        o.com_acc[i] = LEVEL >= 2 ? r.c.f.f[i] * inv_M : 0.0f;
        o.force[i] = LEVEL >= 2 ? r.c.f.f[i] : 0.0f;
        o.moment[i] = LEVEL >= 2 ? r.c.f.n[i] : 0.0f;
    }
    o.force[2] = __builtin_fmaf(M, g, o.force[2]);
    o.moment[0] = __builtin_fmaf(mc[1], g, o.moment[0]);
    o.moment[1] = __builtin_fmaf(-mc[0], g, o.moment[1]);
}
// a row that cannot be used (links_bad_input's convention)
DRM_HD bool wb_bad_input(float q, float qd, float qdd) { return links_bad_input(q, qd, qdd); }

template <int LEVEL>
DRM_HD void wb_record_pack(float c, float s, float q, const float *R, const float *p, bool moved, const WbMotion &v, float *r) {
    r[0] = c; r[1] = s; r[2] = q;
#pragma unroll
    for (int i = 0; i < 9; ++i) r[3 + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r[12 + i] = p[i];
        if constexpr (LEVEL >= 1) { r[16 + i] = v.w[i]; r[19 + i] = v.u[i]; }
        if constexpr (LEVEL >= 2) { r[22 + i] = v.al[i]; r[25 + i] = v.a[i]; }
    }
    r[15] = moved ? 1.0f : 0.0f;
}
template <int LEVEL>
DRM_HD void wb_record_unpack(const float *r, float &c, float &s, float &q, float *R, float *p, bool &moved, WbMotion &v) {
    c = r[0]; s = r[1]; q = r[2];
    wb_motion_zero(v);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = r[3 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p[i] = r[12 + i];
        if constexpr (LEVEL >= 1) { v.w[i] = r[16 + i]; v.u[i] = r[19 + i]; }
        if constexpr (LEVEL >= 2) { v.al[i] = r[22 + i]; v.a[i] = r[25 + i]; }
    }
    moved = r[15] != 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// ANY walk, one row: the ops [0, n_ops) in walk order, all segments by the one caller (energy_tree_walk's structure).  The forward
// sweep leaves one record per op (wb_rec_floats(LEVEL)); the sweep back carries the composite of a chain in registers, parks it at
// open branch points (wb_slot_floats(LEVEL) per slot) and moves it into the base frame where a link hangs off the root or the static
// prefix.
//   qf(d, q, qd, qdd)                 joint value, rate and acceleration of DoF d (zeros for a row that is not to be used)
//   rput(k, const float *) / rget(k, float *)       the record of op k
//   sput(s, const float *) / sget(s, float *)       the composite parked in slot s
//   jout(dof, col[3])                 the CoM Jacobian's column in base axes
// `base_mass`: the base share's; `root` returns the total mass and the sums in the base frame.
template <int LEVEL, class CTL, class ROW, class QF, class RPUT, class RGET, class SPUT, class SGET, class JOUT>
DRM_HD void whole_body_tree_walk(int n_ops, int p_end, int n_slots, CTL ctl, ROW row, QF qf, RPUT rput, RGET rget, SPUT sput, SGET sget,
                                 JOUT jout, float base_mass, WbRoot &root) {
    constexpr int RF = wb_rec_floats(LEVEL), SF = wb_slot_floats(LEVEL);
    float rec[RF], sl[SF];
    float M = 0.0f;
    // ---- outwards: world poses, velocities, accelerations ---------------------------------------------------------------------
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
        LinkState st;
        link_state_root(st);
        WbMotion v;
        wb_motion_zero(v);
        bool moved = false;
        if (!(ct.src == DRM_SRC_ROOT || ct.parent < 0 || ct.parent >= k)) {
            float pc, ps, pq;
            rget(ct.parent, rec);
            wb_record_unpack<LEVEL>(rec, pc, ps, pq, st.R, st.p, moved, v);
        }
        moved = moved || ct.dof >= 0;
        const float *of = row(k);
        const OpFT o = load_ft(of);
        float J[9], t[3];
        link_joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
        wb_motion_step<LEVEL>(J, t, ct.dof >= 0, ct.prismatic, qd, qdd, v);
        link_step<false, false>(J, t, false, false, 0.0f, 0.0f, st);
        if (moved && k >= p_end) M += of[DRM_OPF_MASS];
        wb_record_pack<LEVEL>(c, s, q, st.R, st.p, moved, v, rec);
        rput(k, rec);
    }
    root.M = M + base_mass;
    root.inv_M = 1.0f / root.M;
    // ---- back: the mass, first moment, momentum and its rate of every joint's sub-tree ----------------------------------------
    WbComposite carry, total;
    wb_composite_zero(carry);
    wb_composite_zero(total);
    wb_composite_to_floats<LEVEL>(carry, sl);
#pragma unroll 1
    for (int s = 0; s < n_slots; ++s) sput(s, sl);
#pragma unroll 1
    for (int k = n_ops - 1; k >= p_end; --k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        const float *of = row(k);
        WbMotion v;
        float c, s, q, R[9], p[3];
        bool moved;
        rget(k, rec);
        wb_record_unpack<LEVEL>(rec, c, s, q, R, p, moved, v);
        WbComposite tot;
        wb_composite_zero(tot);
        if (moved) {
            wb_body<LEVEL>(of, v, tot);
            wb_composite_up<0>(R, p, tot, tot); // (the first moment alone: m p + R mc)
        }
        if (ct.child_next) wb_composite_add<LEVEL>(tot, carry);
        if (ct.save >= 0 && ct.save < n_slots) { // take: add and reset
            WbComposite parked;
            sget(ct.save, sl);
            wb_composite_from_floats<LEVEL>(sl, parked);
            wb_composite_add<LEVEL>(tot, parked);
            WbComposite zero;
            wb_composite_zero(zero);
            wb_composite_to_floats<LEVEL>(zero, sl);
            sput(ct.save, sl);
        }
        if (ct.dof >= 0) {
            // z x (mcC - mC p): the sub-tree's first moment about the joint's own origin
            const float z[3] = {R[2], R[5], R[8]};
            float d[3], wc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) d[i] = __builtin_fmaf(-tot.m, p[i], tot.mc[i]);
            lk_cross(z, d, wc);
#pragma unroll
            for (int i = 0; i < 3; ++i) wc[i] = (ct.prismatic ? z[i] * tot.m : wc[i]) * root.inv_M;
            jout(ct.dof, wc);
        }
        if (ct.src != DRM_SRC_ROOT && ct.parent >= p_end && ct.parent < k) {
            const OpFT o = load_ft(of);
            float J[9], t[3];
            link_joint_transform(o, ct.dof >= 0, ct.prismatic, q, c, s, J, t);
            WbComposite up;
            wb_composite_up<LEVEL, false>(J, t, tot, up);
            if (ct.src >= 0) {
                if (ct.src < n_slots) {
                    WbComposite parked;
                    sget(ct.src, sl);
                    wb_composite_from_floats<LEVEL>(sl, parked);
                    wb_composite_add<LEVEL>(parked, up);
                    wb_composite_to_floats<LEVEL>(parked, sl);
                    sput(ct.src, sl);
                }
            } else {
                carry = up;
            }
        } else { // off the root or the static prefix: into the base frame by the link's own world pose
            WbComposite up;
            wb_composite_up<LEVEL, false>(R, p, tot, up);
            wb_composite_add<LEVEL>(total, up);
        }
    }
    root.c = total;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same on a serial chain whose first NJ ops are revolute joints driving DoF columns 0 .. NJ-1 (DRM_WALK_ARM_CHAIN), straight
// line, on cos / sin the caller already has; ops NJ .. LINKS-1 are fixed.  Everything stays in registers: the bodies' momenta and
// their rates are formed on the way out and only summed on the way back; no world pose is carried — the composite reaches the base
// frame through op 0's own transform, and the Jacobian's columns ride back with it, turned by every joint transform they pass.
// JAC: without it no column is formed.  Every link of such a chain is moved by joint 0.
//   jac[3 NJ]   [3, NJ] row-major, in base axes
template <int LINKS, int NJ, int LEVEL, bool JAC, class ROW>
DRM_HD void whole_body_chain_trig(ROW row, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ], const float (&qdd)[NJ],
                                  float *jac, float base_mass, WbRoot &root) {
    LagWrench hb[LEVEL >= 1 ? LINKS : 1], fb[LEVEL >= 2 ? LINKS : 1];
    float M = 0.0f;
    {
        WbMotion cur;
        wb_motion_zero(cur);
#pragma unroll
        for (int k = 0; k < LINKS; ++k) {
            DRM_RNEA_LINK_FENCE();
            const float *of = row(k);
            M += of[DRM_OPF_MASS];
            if constexpr (LEVEL >= 1) {
                const OpFT o = load_ft(of);
                float J[9], t[3];
                link_joint_transform(o, k < NJ, false, 0.0f, k < NJ ? cs[k] : 1.0f, k < NJ ? sn[k] : 0.0f, J, t);
                wb_motion_step<LEVEL>(J, t, k < NJ, false, k < NJ ? qd[k] : 0.0f, k < NJ ? qdd[k] : 0.0f, cur);
                WbComposite c;
                wb_body<LEVEL>(of, cur, c);
                hb[k] = c.h;
                if constexpr (LEVEL >= 2) fb[k] = c.f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    DRM_WB_ANCHOR(cur.w[i]); DRM_WB_ANCHOR(cur.u[i]); DRM_WB_ANCHOR(hb[k].n[i]); DRM_WB_ANCHOR(hb[k].f[i]);
                    if constexpr (LEVEL >= 2) {
                        DRM_WB_ANCHOR(cur.al[i]); DRM_WB_ANCHOR(cur.a[i]); DRM_WB_ANCHOR(fb[k].n[i]); DRM_WB_ANCHOR(fb[k].f[i]);
                    }
                }
            }
        }
    }
    root.M = M + base_mass;
    root.inv_M = 1.0f / root.M;
    float col[NJ][3];
    WbComposite carry;
    wb_composite_zero(carry);
#pragma unroll
    for (int k = LINKS - 1; k >= 0; --k) {
        DRM_RNEA_LINK_FENCE();
        const float *of = row(k);
        WbComposite tot;
        wb_composite_zero(tot);
        tot.m = of[DRM_OPF_MASS];
#pragma unroll
        for (int i = 0; i < 3; ++i) tot.mc[i] = of[DRM_OPF_MCOM + i];
        if constexpr (LEVEL >= 1) tot.h = hb[k];
        if constexpr (LEVEL >= 2) tot.f = fb[k];
        if (k < LINKS - 1) wb_composite_add<LEVEL>(tot, carry);
        if constexpr (JAC) {
            if (k < NJ) wb_column(tot, false, col[k < NJ ? k : 0]);
        }
        const OpFT o = load_ft(of);
        float J[9], t[3];
        link_joint_transform(o, k < NJ, false, 0.0f, k < NJ ? cs[k] : 1.0f, k < NJ ? sn[k] : 0.0f, J, t);
        wb_composite_up<LEVEL>(J, t, tot, carry);
        if constexpr (JAC) {
#pragma unroll
            for (int j = k; j < NJ; ++j) {
                float x[3];
                wb_mat_vec(J, col[j], x);
#pragma unroll
                for (int i = 0; i < 3; ++i) { col[j][i] = x[i]; DRM_WB_ANCHOR(col[j][i]); }
            }
        }
        DRM_WB_ANCHOR(carry.m);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            DRM_WB_ANCHOR(carry.mc[i]);
            if constexpr (LEVEL >= 1) { DRM_WB_ANCHOR(carry.h.n[i]); DRM_WB_ANCHOR(carry.h.f[i]); }
            if constexpr (LEVEL >= 2) { DRM_WB_ANCHOR(carry.f.n[i]); DRM_WB_ANCHOR(carry.f.f[i]); }
        }
    }
    if constexpr (JAC) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) jac[i * NJ + j] = col[j][i] * root.inv_M;
    }
    root.c = carry;
}
} // namespace drm

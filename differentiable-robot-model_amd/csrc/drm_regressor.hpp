// drm_regressor.hpp — include/drm_hip.h drm_rnea_regressor: the per-row arithmetic of the inverse-dynamics regressor Y(q, qd, qdd),
// tau = Y phi with phi the stacked per-body (m, m c, I_o) — what the walk table stores as DRM_OPF_MASS / DRM_OPF_MCOM / DRM_OPF_IO.
// Shared by the kernels (drm_regressor.hip) and by the host build (drm_cpu.cpp) so that both round the same way.  Kept out of
// drm_sample.hpp on purpose, as drm_fdd.hpp and drm_osc.hpp are: that header is part of the source key of every robot's own kernels
// (specialize._HEADERS).
//
// The body force of RNEA, f = I a + v x* (I v) (drm_sample.hpp rnea_body_force_hg), is linear in (m, m c, I_o).  With w, wd the
// angular velocity / acceleration of the body and ac = a + w x v its classical linear acceleration (all in the body's own frame):
//   m        lin = ac                               ang = 0
//   m c_k    lin = wd x e_k + w x (w x e_k)         ang = e_k x ac
//   I_ab     lin = 0                                ang = E_ab wd + w x (E_ab w),   E_ab = e_a e_b^T (+ e_b e_a^T for a != b)
// which is the 6 x 10 matrix A_i of body i.  A_i is carried up the chain of parents one joint transform at a time (lin' = J lin,
// ang' = J ang + t x lin': drm_sample.hpp rnea_link_force_up) and leaves the row S_j^T (X A_i) at every moving ancestor j and at i
// itself: the torque about +z of the stored frame for a revolute joint, the force along +z for a prismatic one.  Only ONE such
// matrix is live at a time, and its six inertia columns never have a linear part (42 floats).
//
// Columns are computed in the stored, axis-canonicalised frame of the body (DRM_OPI_PERM) and handed over in the link's own URDF
// frame: undoing the signed permutation is a signed permutation of the block's ten columns (regressor_column), applied when a row
// is handed to the caller.
#pragma once
#include "drm_sample.hpp"
#include "drm_tree.hpp"

namespace drm {

constexpr int REG_COLS = 10; // m, m c_x, m c_y, m c_z, Ixx, Ixy, Ixz, Iyy, Iyz, Izz

struct RegBlock {
    Force mc[4];     // columns m, m c_x, m c_y, m c_z as (linear, angular) pairs
    float io[6][3];  // columns Ixx, Ixy, Ixz, Iyy, Iyz, Izz: angular part (the linear part is identically zero)
};

// column `col` of a block computed in the stored frame of an op with DRM_OPI_PERM code `code`: its column in the URDF frame and its
// sign.  Stored frame: c~_r = d_r c_pi(r), I~_rc = d_r d_c I_pi(r)pi(c) (flatten._gather_row), pi = (1, 2, 0) for a joint about x,
// (2, 0, 1) about y, the identity about z; d = (1, -1, -1) for a negative axis.
DRM_HD int regressor_column(int code, int col, float &sign) {
    const int a = code >= 3 ? code - 3 : code;
    const float s = code >= 3 ? -1.0f : 1.0f;
    sign = 1.0f;
    if (col == 0 || a > 2) return col;
    const int p0 = a == 0 ? 1 : (a == 1 ? 2 : 0), p1 = a == 0 ? 2 : (a == 1 ? 0 : 1), p2 = a == 0 ? 0 : (a == 1 ? 1 : 2);
    auto pi = [&](int r) { return r == 0 ? p0 : (r == 1 ? p1 : p2); };
    auto d = [&](int r) { return r == 0 ? 1.0f : s; };
    if (col < 4) {
        sign = d(col - 1);
        return 1 + pi(col - 1);
    }
    const int e = col - 4;                       // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    const int r = e < 3 ? 0 : (e < 5 ? 1 : 2), c = e < 3 ? e : (e < 5 ? e - 2 : 2);
    int R = pi(r), C = pi(c);
    if (R > C) { const int t = R; R = C; C = t; }
    sign = d(r) * d(c);
    return 4 + (R == 0 ? C : (R == 1 ? 2 + C : 5));
}

// A_i of a body from its motion (own frame)
DRM_HD void regressor_body(const Motion &M, RegBlock &A) {
    const float w[3] = {M.wa[0][0], M.wa[1][0], M.wa[2][0]}, wd[3] = {M.wa[0][1], M.wa[1][1], M.wa[2][1]};
    const float v[3] = {M.va[0][0], M.va[1][0], M.va[2][0]};
    float ac[3], x[3];
    cross3(w, v, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) ac[i] = M.va[i][1] + x[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) A.mc[0].la[i] = f2_make(ac[i], 0.0f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float e[3] = {k == 0 ? 1.0f : 0.0f, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f};
        float we[3], wwe[3], wde[3], eac[3];
        cross3(w, e, we);
        cross3(w, we, wwe);
        cross3(wd, e, wde);
        cross3(e, ac, eac);
#pragma unroll
        for (int i = 0; i < 3; ++i) A.mc[1 + k].la[i] = f2_make(wde[i] + wwe[i], eac[i]);
    }
    int col = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b, ++col) {
            // E w and E wd for E = e_a e_b^T (+ e_b e_a^T)
            float Ew[3] = {0.0f, 0.0f, 0.0f}, Ewd[3] = {0.0f, 0.0f, 0.0f};
            Ew[a] = w[b]; Ewd[a] = wd[b];
            if (a != b) { Ew[b] = w[a]; Ewd[b] = wd[a]; }
            cross3(w, Ew, x);
#pragma unroll
            for (int i = 0; i < 3; ++i) A.io[col][i] = Ewd[i] + x[i];
        }
}

// A into the parent's frame through the joint transform (x_p = J x_c + t)
DRM_HD void regressor_block_up(const float *J, const float *t, RegBlock &A) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        Force up;
        rnea_link_force_up(J, t, A.mc[c], up);
        A.mc[c] = up;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        float y[3];
        mat_vec(J, A.io[c], y);
#pragma unroll
        for (int i = 0; i < 3; ++i) A.io[c][i] = y[i];
    }
}

// S^T A: the ten entries of the row of a joint whose frame A is expressed in; out(col, value), col in the stored frame of the BODY
template <class OUT>
DRM_HD void regressor_joint_row(const RegBlock &A, bool prismatic, OUT out) {
#pragma unroll
    for (int c = 0; c < 4; ++c) out(c, prismatic ? A.mc[c].la[2][0] : A.mc[c].la[2][1]);
#pragma unroll
    for (int c = 0; c < 6; ++c) out(4 + c, prismatic ? 0.0f : A.io[c][2]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The regressor of ANY walk, one row: the ops [0, n_ops) in walk order, all segments by the one caller (the sub-trees off the root
// share nothing but the static prefix).  Per op the forward step of RNEA (drm_tree.hpp rnea_forward_step: the body's motion from
// its parent's, gravity as base acceleration g), then, the motion still live, the body's block is walked up its ancestors (parent op
// indices, DRM_OPI_W1).  What outlives an op is cos / sin / value of its joint (three floats, the transform is rebuilt from them and
// the table as RNEA's way back does) and the motions of the open branch points.
//   ctl / row / qf / motion_save / motion_load   as rnea_tree_walk
//   tput(k, c, s, q) / tget(k, c, s, q)          the record of op k
//   yout(dof, op, col, value)                    Y[dof, 10 op + col], col in the URDF frame of op's link
// Only the rows of a body's moving ancestors are handed over: every other entry of Y is zero, and the caller's to write.  The ops
// of the static prefix [0, p_end) have no moving ancestor: nothing is handed over for them.
template <class CTL, class ROW, class QF, class TPUT, class TGET, class MSAVE, class MLOAD, class YOUT>
DRM_HD void regressor_tree_walk(int n_ops, int p_end, CTL ctl, ROW row, float g, QF qf, TPUT tput, TGET tget, MSAVE motion_save,
                                MLOAD motion_load, YOUT yout) {
    Motion cur;
    motion_root(cur, g);
#pragma unroll 1
    for (int k = 0; k < n_ops; ++k) {
        int w0, w1;
        ctl_words(ctl, k, w0, w1);
        const OpCtl ct = decode_ctl(w0, w1);
        Force unused;
        float c, s, q;
        rnea_forward_step(k, ct, row, g, qf, motion_save, motion_load, cur, false, unused, c, s, q);
        tput(k, c, s, q);
        if (k >= p_end) {
            RegBlock A;
            regressor_body(cur, A);
            OpCtl cj = ct;
            int j = k;
#pragma unroll 1
            for (;;) {
                if (cj.dof >= 0) {
                    const int dof = cj.dof;
                    regressor_joint_row(A, cj.prismatic, [&](int col, float v) {
                        float sign;
                        const int dst = regressor_column(ct.perm, col, sign);
                        yout(dof, k, dst, sign * v);
                    });
                }
                if (cj.src == DRM_SRC_ROOT || cj.parent < p_end || cj.parent < 0 || cj.parent >= j) break; // (parents precede their children)
                const OpFT o = load_ft(row(j));
                float J[9], t[3];
                joint_transform(o, cj.dof >= 0, cj.prismatic, q, c, s, J, t);
                regressor_block_up(J, t, A);
                j = cj.parent;
                ctl_words(ctl, j, w0, w1);
                cj = decode_ctl(w0, w1);
                tget(j, c, s, q);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same on a serial chain whose first NJ ops are revolute joints driving DoF columns 0 .. NJ-1 (DRM_WALK_ARM_CHAIN), straight
// line, on cos / sin the caller already has; ops NJ .. LINKS-1 are fixed.  perm(k): DRM_OPI_PERM code of op k.
//   yout(dof, op, col, value) as above (dof and op compile-time constants after unrolling)
//   own(op)    whether this caller forms op's block: the kernel shares the bodies of a tile out over the wavefronts of a block, every
//              one of which walks the motions of the whole chain
template <int LINKS, int NJ, class ROW, class PERM, class OWN, class YOUT>
DRM_HD void regressor_chain_trig(ROW row, PERM perm, bool gravity, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ],
                                 const float (&qdd)[NJ], OWN own, YOUT yout) {
    Motion cur;
    motion_root(cur, gravity ? 9.81f : 0.0f);
#pragma unroll
    for (int k = 0; k < LINKS; ++k) {
        DRM_RNEA_LINK_FENCE();
        {
            const OpFT o = load_ft(row(k));
            float J[9];
            if (k < NJ) {
                joint_rot_z(o.F, cs[k], sn[k], J);
            } else {
#pragma unroll
                for (int i = 0; i < 9; ++i) J[i] = o.F[i];
            }
            rnea_link_motion(J, o.t, k < NJ ? qd[k] : 0.0f, k < NJ ? qdd[k] : 0.0f, cur, cur);
        }
        if (!own(k)) continue;
        RegBlock A;
        regressor_body(cur, A);
        const int code = perm(k);
#pragma unroll
        for (int j = k; j >= 0; --j) {
            if (j < NJ) {
                regressor_joint_row(A, false, [&](int col, float v) {
                    float sign;
                    const int dst = regressor_column(code, col, sign);
                    yout(j, k, dst, sign * v);
                });
            }
            if (j > 0) {
                DRM_RNEA_LINK_FENCE();
                const OpFT o = load_ft(row(j));
                float J[9];
                if (j < NJ) {
                    joint_rot_z(o.F, cs[j], sn[j], J);
                } else {
#pragma unroll
                    for (int i = 0; i < 9; ++i) J[i] = o.F[i];
                }
                regressor_block_up(J, o.t, A);
            }
        }
    }
}
} // namespace drm

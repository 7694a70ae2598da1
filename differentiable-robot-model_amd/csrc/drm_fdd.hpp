// drm_fdd.hpp — include/drm_hip.h drm_forward_dynamics_derivatives: the per-row arithmetic of the linearisation of forward dynamics
// about a state, shared by the fused arm kernel and the composed path's kernels (drm_fdd.hip) and by the host build (drm_cpu.cpp) so
// that all three round the same way.  Kept out of drm_sample.hpp on purpose, as drm_osc.hpp is: that header is part of the source key
// of every robot's own kernels (specialize._HEADERS).
//
// With ID(q, qd, qdd) = H(q) qdd + nle(q, qd) the inverse dynamics (damping inside when the flag is set) and qdd = H^-1 (f - nle):
//   minv = H^-1 = d qdd / d f          dqdd_dq = -H^-1 dID/dq at (q, qd, qdd)          dqdd_dqd = -H^-1 dID/dqd
// Row k of dID/dq and of dID/dqd is the reverse sweep of RNEA seeded with grad_tau = e_k: n sweeps give both matrices, and 3 n
// solves with the one factorisation of H the outputs.  (Seeding the sweeps with the rows of H^-1 instead — H is symmetric — saves the
// 2 n solves but sums kilogram-scale and gram-scale adjoints in one sweep: on an arm that carries a hand, float32 loses 3e-3 of
// dqdd_dqd that way against 4e-4 for the solves.)  The linear algebra is templated on the scalar type — a double instantiation on the
// host separates a wrong formula from float32 rounding; the sweeps are drm_sample.hpp's and float only.
#pragma once
#include "drm_sample.hpp"

namespace drm {

template <class T> DRM_HD T fdd_recip(T x) { return T(1) / x; }
template <> DRM_HD float fdd_recip<float>(float x) { return recip_f(x); }

// H = L^T D L in place, from the last DoF to the first (drm_sample.hpp ltdl_factor_acc, the elimination order of the
// articulated-body recursion) on a two-index accessor H(i, j), i >= j.  The diagonal keeps 1 / D.
template <class T, class HA>
DRM_HD void fdd_ltdl_factor(int n, HA H) {
#pragma unroll
    for (int k = n - 1; k >= 0; --k) {
        const T inv = fdd_recip<T>(H(k, k));
        H(k, k) = inv;
#pragma unroll
        for (int i = 0; i < k; ++i) {
            const T hki = H(k, i);
            const T a = hki * inv;
#pragma unroll
            for (int j = 0; j < i; ++j) H(i, j) -= hki * H(k, j);
            H(i, i) -= hki * a;
            H(k, i) = a;
        }
    }
}

// H^-1 from those factors, column by column: column c is the solve of e_c (whose zeros above c are skipped, not multiplied), kept for
// the rows i >= c and handed over once as out(i, c, value) — the caller mirrors it, so the inverse is symmetric to the bit.
// b(i): a reference to entry i of an n-vector of working storage.
template <class T, class HA, class BF, class MO>
DRM_HD void fdd_inverse(int n, HA H, BF b, MO out) {
#pragma unroll
    for (int c = 0; c < n; ++c) {
        b(c) = T(1);
#pragma unroll
        for (int j = 0; j < c; ++j) b(j) = -H(c, j);
#pragma unroll
        for (int i = c - 1; i >= 0; --i) {       // y = L^-T e_c
            const T bi = b(i);
#pragma unroll
            for (int j = 0; j < i; ++j) b(j) -= H(i, j) * bi;
        }
#pragma unroll
        for (int i = 0; i < n; ++i) {            // z = D^-1 y,  x = L^-1 z
            T t = i <= c ? b(i) * H(i, i) : T(0);
#pragma unroll
            for (int j = 0; j < i; ++j) t -= H(i, j) * b(j);
            b(i) = t;
            if (i >= c) out(i, c, t);
        }
    }
}

// b <- H^-1 b with those factors (drm_sample.hpp ltdl_apply_acc); b(i) is a reference to entry i
template <class T, class HA, class BF>
DRM_HD void fdd_ltdl_apply(int n, HA H, BF b) {
#pragma unroll
    for (int i = n - 1; i >= 0; --i) {
        const T bi = b(i);
#pragma unroll
        for (int j = 0; j < i; ++j) b(j) -= H(i, j) * bi;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) {
        T t = b(i) * H(i, i);
#pragma unroll
        for (int j = 0; j < i; ++j) t -= H(i, j) * b(j);
        b(i) = t;
    }
}

// Column j of -H^-1 G: G(i, j) = d ID_i / d x_j is read, out(i, j, d qdd_i / d x_j) takes the result (in place where the caller's
// two accessors name the same storage: the column is read whole before any of it is written)
template <class T, class HA, class BF, class GF, class OF>
DRM_HD void fdd_solve_column(int n, HA H, BF b, GF G, OF out, int j) {
#pragma unroll
    for (int i = 0; i < n; ++i) b(i) = G(i, j);
    fdd_ltdl_apply<T>(n, H, b);
#pragma unroll
    for (int i = 0; i < n; ++i) out(i, j, -b(i));
}
template <class T, class HA, class BF, class GF, class OF>
DRM_HD void fdd_solve_columns(int n, HA H, BF b, GF G, OF out) {
    for (int j = 0; j < n; ++j) fdd_solve_column<T>(n, H, b, G, out, j);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The reverse sweep of RNEA on a serial chain for the derivatives (drm_sample.hpp rnea_backward_chain without the gradients of
// the constants and of qdd, on cos / sin the caller already has, and with what does not depend on the seed taken out of it): the
// motion of the chain's last link at (q, qd, qdd) once, then per seed the force adjoints up the chain and the walk back to the
// root.  row(k) -> op k's constant row.
template <int CAP, int NJ, class ROW>
DRM_HD void fdd_chain_joint(ROW &row, const float (&cs)[NJ], const float (&sn)[NJ], int k, float *J, float *t) {
    const OpFT o = load_ft(row(k));
    if (k < NJ) {
        joint_rot_z(o.F, cs[k], sn[k], J);
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) J[i] = o.F[i];
    }
    t[0] = o.t[0]; t[1] = o.t[1]; t[2] = o.t[2];
}

template <int CAP, int NJ, class ROW>
DRM_HD void fdd_chain_tip_motion(ROW row, bool gravity, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ],
                                 const float (&qdd)[NJ], Motion &M) {
    motion_root(M, gravity ? 9.81f : 0.0f);
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
        float J[9], t[3];
        fdd_chain_joint<CAP, NJ>(row, cs, sn, k, J, t);
        rnea_link_motion(J, t, k < NJ ? qd[k] : 0.0f, k < NJ ? qdd[k] : 0.0f, M, M);
    }
}

// gout(d, gq, gqd): entry d of grad_tau^T dID/dq and of grad_tau^T dID/dqd
template <int CAP, int NJ, class ROW, class GOUT>
DRM_HD void fdd_chain_adjoint(ROW row, bool gravity, bool damping, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ],
                              const float (&qdd)[NJ], const Motion &tip, const float (&gtau)[NJ], GOUT gout) {
    const float g = gravity ? 9.81f : 0.0f;
    // adjoints of the total forces up the chain: T[i] = (tbar.lin_i, tbar.ang_i)
    f2 T[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) T[i] = f2_bcast(0.0f);
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
        float J[9], t[3];
        fdd_chain_joint<CAP, NJ>(row, cs, sn, k, J, t);
        if (k > 0) {
            const float ua[3] = {T[0][1], T[1][1], T[2][1]};
            f2 x[3] = {T[0], T[1], T[2]}, y[3];
            x[0][0] += ua[1] * t[2] - ua[2] * t[1];
            x[1][0] += ua[2] * t[0] - ua[0] * t[2];
            x[2][0] += ua[0] * t[1] - ua[1] * t[0];
            matT_vec_p(J, x, y);
#pragma unroll
            for (int i = 0; i < 3; ++i) T[i] = y[i];
        }
        if (k < NJ) T[2][1] += gtau[k];
    }
    // back to the root: the parent's motion and force adjoint recovered from the link's, the body force recomputed from the motion
    Motion M = tip, B;
    Force carry;
#pragma unroll
    for (int i = 0; i < 3; ++i) { B.wa[i] = f2_bcast(0.0f); B.va[i] = f2_bcast(0.0f); carry.la[i] = f2_bcast(0.0f); }
#pragma unroll
    for (int k = CAP - 1; k >= 0; --k) {
        const float *of = row(k);
        float J[9], t[3];
        fdd_chain_joint<CAP, NJ>(row, cs, sn, k, J, t);
        const float wj = k < NJ ? qd[k] : 0.0f, aj = k < NJ ? qdd[k] : 0.0f;
        Motion Pm;
        f2 U[3];
        if (k == 0) {
            motion_root(Pm, g);
#pragma unroll
            for (int i = 0; i < 3; ++i) U[i] = f2_bcast(0.0f);
        } else {
            const float w0 = M.wa[0][0], w1 = M.wa[1][0], v0 = M.va[0][0], v1 = M.va[1][0];
            f2 x[3] = {M.wa[0], M.wa[1], M.wa[2]}, y[3], c[3];
            x[0][1] -= w1 * wj; x[1][1] += w0 * wj; x[2] -= f2_make(wj, aj);
            mat_vec_p(J, x, Pm.wa);
            x[0] = M.va[0]; x[1] = M.va[1]; x[2] = M.va[2];
            x[0][1] -= v1 * wj; x[1][1] += v0 * wj;
            mat_vec_p(J, x, y);
            cross3_ps(Pm.wa, t, c);
#pragma unroll
            for (int i = 0; i < 3; ++i) Pm.va[i] = y[i] - c[i];
            x[0] = T[0]; x[1] = T[1]; x[2] = T[2];
            if (k < NJ) x[2][1] -= gtau[k];
            mat_vec_p(J, x, U);
            const float ua[3] = {U[0][1], U[1][1], U[2][1]};
            U[0][0] -= ua[1] * t[2] - ua[2] * t[1];
            U[1][0] -= ua[2] * t[0] - ua[0] * t[2];
            U[2][0] -= ua[0] * t[1] - ua[1] * t[0];
        }
        Force tot;
        f2 hgl[3], hga[3];
        rnea_body_force_hg(of[DRM_OPF_MASS], of + DRM_OPF_MCOM, of + DRM_OPF_IO, M, tot, hgl, hga);
#pragma unroll
        for (int i = 0; i < 3; ++i) tot.la[i] += carry.la[i];
        LinkAdjointP A;
        rnea_link_adjoint_packed(of[DRM_OPF_MASS], of + DRM_OPF_MCOM, of + DRM_OPF_IO, J, t, wj, M, hgl, hga, T, tot, k > 0, B, A);
        if (k < NJ) gout(k, A.gq, A.wjb + (damping ? of[DRM_OPF_DAMP] * gtau[k] : 0.0f));
        if (k > 0) rnea_link_force_up(J, t, tot, carry);
        DRM_RNEA_LINK_FENCE();
        B = A.pb;
        M = Pm;
#pragma unroll
        for (int i = 0; i < 3; ++i) T[i] = U[i];
    }
}
} // namespace drm

// drm_osc.hpp — include/drm_hip.h drm_operational_space: the per-row arithmetic of the operational-space dynamics of one link,
// shared by the fused arm kernel and the composed path's finish kernel (drm_osc.hip) and by the host build (drm_cpu.cpp) so that
// all three round the same way.  Kept out of drm_sample.hpp on purpose, as drm_ik.hpp is: that header is part of the source key of
// every robot's own kernels (specialize._HEADERS).
//
// With J = [lin_jac; ang_jac] (M = 6 rows, or M = 3: lin_jac alone), H the joint-space inertia matrix and nle the bias torques:
//   X = J H^-1 (M x n, one L^T D L factorisation of H and M solves)      A = J X^T + reg^2 I (M x M)      inertia = A^-1
//   jacobian_pinv = X^T inertia (n x M)       bias_acc = Jdot qd       bias_force = inertia (X nle - bias_acc)
// (J H^-1 nle = X nle because H is symmetric: no solve of its own.)
// Everything is read and written through accessors: the fused kernel passes its registers, the finish kernel and the host build
// their rows of the scratch / of the caller's arrays.  With n a compile-time constant at the call site every loop unrolls.
#pragma once
#include "drm_sample.hpp"

namespace drm {

// Jdot qd of a chain of revolute / prismatic joints, world frame: the classical acceleration of the target's origin p (out[0..2])
// and, for M = 6, the angular acceleration of the target (out[3..5]) at zero joint accelerations.  The ops are visited in chain
// order; joint(k, z, r, prismatic, v) returns false for an op that does not move and otherwise fills the joint's axis z, the offset
// r = p - (ANY point on the axis; unused for a prismatic joint) and the joint velocity v.  With w the angular velocity of the link
// before joint k, u the velocity it would give the point p, and V the velocity of p itself:
//   revolute:   alpha += (w x z) v      a += ((w x z) x r + z x (V - (u - w x r))) v      w += z v      u += (z x r) v
//   prismatic:  a += (w x z) v          u += z v
template <int M, class JOINT>
DRM_HD void osc_bias_acc(int n_ops, JOINT joint, float (&out)[M]) {
    float V[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < n_ops; ++k) {
        float z[3], r[3], v, c[3];
        bool pris;
        if (!joint(k, z, r, pris, v)) continue;
        cross3(z, r, c);
#pragma unroll
        for (int i = 0; i < 3; ++i) V[i] = fmaf(pris ? z[i] : c[i], v, V[i]);
    }
    float w[3] = {0.0f, 0.0f, 0.0f}, u[3] = {0.0f, 0.0f, 0.0f}, a[3] = {0.0f, 0.0f, 0.0f}, al[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < n_ops; ++k) {
        float z[3], r[3], v, wz[3];
        bool pris;
        if (!joint(k, z, r, pris, v)) continue;
        cross3(w, z, wz);
        if (pris) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { a[i] = fmaf(wz[i], v, a[i]); u[i] = fmaf(z[i], v, u[i]); }
        } else {
            float wr[3], d[3], t1[3], t2[3], c[3];
            cross3(w, r, wr);
#pragma unroll
            for (int i = 0; i < 3; ++i) d[i] = V[i] - u[i] + wr[i];
            cross3(wz, r, t1);
            cross3(z, d, t2);
            cross3(z, r, c);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a[i] = fmaf(t1[i] + t2[i], v, a[i]);
                al[i] = fmaf(wz[i], v, al[i]);
                w[i] = fmaf(z[i], v, w[i]);
                u[i] = fmaf(c[i], v, u[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = a[i];
    if (M == 6) {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[M - 3 + i] = al[i];
    }
}

// H = L^T D L in place, from the last DoF to the first — drm_sample.hpp ltdl_factor_acc (the elimination order of the
// articulated-body recursion) on a two-index accessor H(i, j), i >= j: the lower triangle of a dense n x n array (composed path, host
// build) or a packed triangle in registers (fused kernel).  The diagonal keeps 1 / D.
template <class HA>
DRM_HD void osc_ltdl_factor(int n, HA H) {
#pragma unroll
    for (int k = n - 1; k >= 0; --k) {
        const float inv = recip_f(H(k, k));
        H(k, k) = inv;
#pragma unroll
        for (int i = 0; i < k; ++i) {
            const float hki = H(k, i);
            const float a = hki * inv;
#pragma unroll
            for (int j = 0; j < i; ++j) H(i, j) -= hki * H(k, j);
            H(i, i) -= hki * a;
            H(k, i) = a;
        }
    }
}
// b <- H^-1 b with those factors (ltdl_apply_acc); b(i) is a reference to entry i
template <class HA, class BF>
DRM_HD void osc_ltdl_apply(int n, HA H, BF b) {
#pragma unroll
    for (int i = n - 1; i >= 0; --i) {
        const float bi = b(i);
#pragma unroll
        for (int j = 0; j < i; ++j) b(j) -= H(i, j) * bi;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) {
        float t = b(i) * H(i, i);
#pragma unroll
        for (int j = 0; j < i; ++j) t -= H(i, j) * b(j);
        b(i) = t;
    }
}

// X = J H^-1, row by row: X(r, .) = H^-1 J(r, .)^T
template <int M, class HA, class JF, class XF>
DRM_HD void osc_solve_columns(int n, HA H, JF J, XF X) {
#pragma unroll
    for (int r = 0; r < M; ++r) {
#pragma unroll
        for (int k = 0; k < n; ++k) X(r, k) = J(r, k);
        osc_ltdl_apply(n, H, [&](int k) -> float & { return X(r, k); });
    }
}

// inertia = (J X^T + reg2 I)^-1: the lower triangle of A, its Cholesky factor L (reciprocals of the diagonal, as drm_ik.hpp
// ik_solve), W = L^-1 and inertia = W^T W, computed for i >= j and mirrored: symmetric to the bit.  A matrix that is not positive
// definite in fp32 (a singular configuration with reg = 0) gives Inf / NaN entries, nothing else.
template <int M, class JF, class XF>
DRM_HD void osc_inertia(int n, JF J, XF X, float reg2, float (&Lam)[M][M]) {
    float L[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float a = i == j ? reg2 : 0.0f;
#pragma unroll
            for (int k = 0; k < n; ++k) a = fmaf(J(i, k), X(j, k), a);
            L[i][j] = a;
        }
    float inv[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        float d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = fmaf(-L[j][k], L[j][k], d);
        inv[j] = 1.0f / sqrtf(d);
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            float a = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) a = fmaf(-L[i][k], L[j][k], a);
            L[i][j] = a * inv[j];
        }
    }
    float W[M][M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        W[j][j] = inv[j];
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            float a = 0.0f;
#pragma unroll
            for (int k = j; k < i; ++k) a = fmaf(L[i][k], W[k][j], a);
            W[i][j] = -a * inv[i];
        }
    }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float a = 0.0f;
#pragma unroll
            for (int k = i; k < M; ++k) a = fmaf(W[k][i], W[k][j], a);
            Lam[i][j] = a;
            Lam[j][i] = a;
        }
}

// entry (k, c) of jacobian_pinv = X^T inertia
template <int M, class XF>
DRM_HD float osc_jbar(XF X, const float (&Lam)[M][M], int k, int c) {
    float a = 0.0f;
#pragma unroll
    for (int r = 0; r < M; ++r) a = fmaf(X(r, k), Lam[r][c], a);
    return a;
}

// bias_force = inertia (X nle - bias_acc)
template <int M, class XF, class NF>
DRM_HD void osc_bias_force(int n, XF X, NF nle, const float (&bias_acc)[M], const float (&Lam)[M][M], float (&eta)[M]) {
    float t[M];
#pragma unroll
    for (int r = 0; r < M; ++r) {
        float a = -bias_acc[r];
#pragma unroll
        for (int k = 0; k < n; ++k) a = fmaf(X(r, k), nle(k), a);
        t[r] = a;
    }
#pragma unroll
    for (int c = 0; c < M; ++c) {
        float a = 0.0f;
#pragma unroll
        for (int r = 0; r < M; ++r) a = fmaf(Lam[c][r], t[r], a);
        eta[c] = a;
    }
}
} // namespace drm

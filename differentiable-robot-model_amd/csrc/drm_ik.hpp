// drm_ik.hpp — ABI 15 (include/drm_hip.h drm_inverse_kinematics): the per-row arithmetic of one damped-least-squares iteration,
// shared by the device kernels (drm_ik.hip) and the host build (drm_cpu.cpp) so that both round the same way.  Kept out of
// drm_sample.hpp on purpose: that header is part of the source key of every robot's own kernels (specialize._HEADERS).
//
// The Jacobian is read through an accessor J(r, k), r < M (rows 0-2 linear, 3-5 angular), k < n: the fused kernel passes its
// registers, the composed kernel and the host build their [3, n] lin / ang arrays.
#pragma once
#include "drm_sample.hpp"

namespace drm {

struct IkOpts {
    float lam2;     // damping^2
    float step;     // alpha
    float tol_pos, tol_rot;
};

// the target quaternion, normalised once per row
DRM_HD void ik_normalize_quat(float t[4]) {
    const float s = sqrtf(fmaf(t[0], t[0], fmaf(t[1], t[1], fmaf(t[2], t[2], t[3] * t[3]))));
    const float inv = 1.0f / s;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] *= inv;
}

// step 2: e = [e_p; e_R] of the pose (p, c) against the target (tp, tq normalised), pos_err = |e_p|, rot_err = theta (0 when
// pos_only, which leaves e[3..5] untouched)
DRM_HD void ik_error(const float p[3], const float c[4], const float tp[3], const float tq[4], bool pos_only, float e[6],
                     float &pos_err, float &rot_err) {
    e[0] = tp[0] - p[0];
    e[1] = tp[1] - p[1];
    e[2] = tp[2] - p[2];
    pos_err = sqrtf(fmaf(e[0], e[0], fmaf(e[1], e[1], e[2] * e[2])));
    rot_err = 0.0f;
    if (pos_only) return;
    // t (x) conj(c), xyzw: conj(c) = (-cx, -cy, -cz, cw)
    const float ax = tq[0], ay = tq[1], az = tq[2], aw = tq[3], bx = -c[0], by = -c[1], bz = -c[2], bw = c[3];
    float w = fmaf(aw, bw, -fmaf(ax, bx, fmaf(ay, by, az * bz)));
    float x = fmaf(aw, bx, fmaf(ax, bw, fmaf(ay, bz, -(az * by))));
    float y = fmaf(aw, by, fmaf(-ax, bz, fmaf(ay, bw, az * bx)));
    float z = fmaf(aw, bz, fmaf(ax, by, fmaf(-ay, bx, az * bw)));
    if (w < 0.0f) { w = -w; x = -x; y = -y; z = -z; }
    const float s = sqrtf(fmaf(x, x, fmaf(y, y, z * z)));
    const float th = 2.0f * atan2f(s, w);
    const float k = s > 0.0f ? th / s : 2.0f;
    e[3] = k * x;
    e[4] = k * y;
    e[5] = k * z;
    rot_err = th;
}

DRM_HD bool ik_converged(float pos_err, float rot_err, const IkOpts &o) { return pos_err <= o.tol_pos && rot_err <= o.tol_rot; }

// step 4, the solve: y = (J J^T + lam2 I)^-1 e for M = 3 or 6, by Cholesky L L^T of the lower triangle (kept as reciprocals of the
// diagonal), forward and back substitution
template <int M, class JF>
DRM_HD void ik_solve(JF J, int n, float lam2, const float (&e)[6], float (&y)[M]) {
    float L[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float a = i == j ? lam2 : 0.0f;
#pragma unroll
            for (int k = 0; k < n; ++k) a = fmaf(J(i, k), J(j, k), a);
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
    float z[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        float a = e[i];
#pragma unroll
        for (int k = 0; k < i; ++k) a = fmaf(-L[i][k], z[k], a);
        z[i] = a * inv[i];
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
        float a = z[i];
#pragma unroll
        for (int k = i + 1; k < M; ++k) a = fmaf(-L[k][i], y[k], a);
        y[i] = a * inv[i];
    }
}

// x clamped to [lo, hi]; a NaN x stays NaN (min(max(x, lo), hi) with NaN-propagating min / max)
DRM_HD float ik_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// step 4, the update: q_k <- clamp(q_k + step * (J^T y)_k, lower_k, upper_k) for every DoF (lower / upper NULL: no clamp)
template <int M, class JF, class QF>
DRM_HD void ik_update(JF J, int n, const float (&y)[M], float step, QF q, const float *lower, const float *upper) {
#pragma unroll
    for (int k = 0; k < n; ++k) {
        float dq = 0.0f;
#pragma unroll
        for (int i = 0; i < M; ++i) dq = fmaf(J(i, k), y[i], dq);
        const float x = fmaf(step, dq, q(k));
        q(k) = lower ? ik_clamp(x, lower[k], upper[k]) : x;
    }
}

// steps 2 - 4 of one row at iteration i: returns true when the row stops at q (converged, or last == true), with its errors in
// pos_err / rot_err; otherwise q(k) has been updated in place.
template <class JF, class QF>
DRM_HD bool ik_iteration(JF J, int n, const float p[3], const float c[4], const float tp[3], const float tq[4], bool pos_only,
                         const IkOpts &o, bool last, QF q, const float *lower, const float *upper, float &pos_err, float &rot_err) {
    float e[6];
    ik_error(p, c, tp, tq, pos_only, e, pos_err, rot_err);
    if (ik_converged(pos_err, rot_err, o) || last) return true;
    if (pos_only) {
        float y[3];
        ik_solve<3>(J, n, o.lam2, e, y);
        ik_update<3>(J, n, y, o.step, q, lower, upper);
    } else {
        float y[6];
        ik_solve<6>(J, n, o.lam2, e, y);
        ik_update<6>(J, n, y, o.step, q, lower, upper);
    }
    return false;
}
} // namespace drm

// drm_collision.hpp — include/drm_hip.h drm_collision_cost and drm_sphere_distances: the collision law of spheres fixed to the links
// against a world of spheres and oriented boxes and against each other.  Shared by the kernels (drm_collision.hip) and by the host
// build (drm_cpu.cpp) so that both round the same way.  Kept out of drm_sample.hpp on purpose, as drm_links.hpp is: that header is
// part of the source key of every robot's own kernels (specialize._HEADERS).
//
// Sphere s sits on link l(s) with centre c~_s in the STORED frame of the link's op (R~ = R P, DRM_OPI_PERM; the host converts the
// URDF-frame centre once, c~ = P^T c, exactly) and radius r_s >= 0:  x_s = p_l + R~_l c~_s.  Root spheres have R = I, p = 0.
//
//   sphere obstacle (c, r)        sd = |x - c| - r,   direction (x - c) / |x - c|   (0 when the norm is 0)
//   box (c, Rb box -> world, h)   y = Rb^T (x - c),  a = |y| - h
//                                 outside (max a > 0):  sd = |max(a, 0)|,  direction Rb (sign(y) max(a, 0) / sd)
//                                 inside:               sd = max a,        direction Rb (sign(y_i) e_i), i the first largest a_i
//   world clearance   d_sm = sd_m(x_s) - r_s            self clearance   d_ij = |x_i - x_j| - r_i - r_j, direction as a sphere's
//   phi(u) = 0 (u <= 0),  u^2 / (2 eta) (0 < u <= eta),  u - eta / 2 (above);    phi'(u) = clamp(u / eta, 0, 1);    u = eta - d
//   cost = w_world sum_{s, m} phi(eta_world - d_sm) + w_self sum_{pairs} phi(eta_self - d_ij)        (a sum, not a minimum)
//   g_s = dcost/dx_s = -w phi' direction from every world term, -/+ from every pair (i, j)
//   F_l = sum_{s on l} g_s,   M_l = sum_{s on l} (x_s - p_l) x g_s,   dcost/dq = sum_l lin_jac_l^T F_l + ang_jac_l^T M_l
// which is drm_external_torques' sweep inwards (drm_links.hpp link_wrench_up, link_joint_torque) of the wrenches (F_l, M_l).
// Every product-sum is an explicit fused multiply-add, as in drm_links.hpp.
#pragma once
#include <math.h>

#include "drm_links.hpp"

namespace drm {

constexpr int COLL_SPHERE_FLOATS = 4; // centre 3, radius
constexpr int COLL_BOX_FLOATS = 16;   // centre 3, half extents 3, rotation 9 (row-major, box -> world), one pad

// the caps of the fused kernel (drm_collision.hip; the host build takes its chain form within the same): the centres of 64 rows in
// LDS (48 KiB at the cap), obstacle and pair tables that stay in the scalar cache (2 KiB and 8 KiB)
constexpr int COLL_FUSED_SPHERES = 64, COLL_FUSED_OBSTACLES = 32, COLL_FUSED_PAIRS = 1024;
inline bool coll_within_caps(int n_spheres, int n_obstacles, int n_pairs) {
    return n_spheres <= COLL_FUSED_SPHERES && n_obstacles <= COLL_FUSED_OBSTACLES && n_pairs <= COLL_FUSED_PAIRS;
}

// one term of the cost: weight, activation distance and the two constants phi needs (formed once, on the host, in both builds)
struct CollLaw {
    float w, eta, inv_eta, half_inv, half_eta; // 1 / eta, 1 / (2 eta), eta / 2
};
inline CollLaw coll_law_make(float w, float eta) { return CollLaw{w, eta, 1.0f / eta, 0.5f / eta, 0.5f * eta}; }
// what drm_collision_cost asks of a term that is present
inline bool coll_law_ok(float w, float eta) { return w >= 0.0f && w <= 3.0e38f && eta > 0.0f && eta <= 3.0e38f; }

// phi and phi' at the clearance d
DRM_HD void coll_phi(const CollLaw &L, float d, float &phi, float &dphi) {
    const float u = L.eta - d;
    const float quad = (u * u) * L.half_inv, lin = u - L.half_eta;
    phi = u > 0.0f ? (u <= L.eta ? quad : lin) : 0.0f;
    dphi = u > 0.0f ? fminf(u * L.inv_eta, 1.0f) : 0.0f;
}

// x = p + R c: the world centre of a sphere at c in the frame (R, p)
DRM_HD void coll_centre(const float *R, const float *p, float c0, float c1, float c2, float *x) {
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = __builtin_fmaf(R[3 * i + 2], c2, __builtin_fmaf(R[3 * i + 1], c1, __builtin_fmaf(R[3 * i], c0, p[i])));
}

// |x - c| and the unit direction from c to x (0 when they coincide)
DRM_HD float coll_point_distance(const float *x, float c0, float c1, float c2, float *n) {
    const float e0 = x[0] - c0, e1 = x[1] - c1, e2 = x[2] - c2;
    const float len = sqrtf(lk_dot(e0, e1, e2, e0, e1, e2));
    const float inv = len > 0.0f ? 1.0f / len : 0.0f;
    n[0] = e0 * inv; n[1] = e1 * inv; n[2] = e2 * inv;
    return len;
}

// signed distance of the point x to the box b[COLL_BOX_FLOATS] and its direction in world axes
DRM_HD float coll_box_distance(const float *x, const float *b, float *n) {
    const float e[3] = {x[0] - b[0], x[1] - b[1], x[2] - b[2]};
    const float *Rb = b + 6;
    float y[3], a[3], m[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        y[i] = lk_dot(Rb[i], Rb[3 + i], Rb[6 + i], e[0], e[1], e[2]);
        a[i] = fabsf(y[i]) - b[3 + i];
        m[i] = fmaxf(a[i], 0.0f);
    }
    const float amax = fmaxf(a[0], fmaxf(a[1], a[2]));
    const bool outside = amax > 0.0f;
    const float out = sqrtf(lk_dot(m[0], m[1], m[2], m[0], m[1], m[2]));
    const float inv = outside ? 1.0f / out : 0.0f;
    const int first = a[0] >= amax ? 0 : (a[1] >= amax ? 1 : 2);
    float dl[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) dl[i] = copysignf(outside ? m[i] * inv : (i == first ? 1.0f : 0.0f), y[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = lk_dot(Rb[3 * i], Rb[3 * i + 1], Rb[3 * i + 2], dl[0], dl[1], dl[2]);
    return outside ? out : amax;
}

// One robot sphere (centre x, radius r) against the world, spheres before boxes, in table order.  COST: its terms are added to `cost`
// and their gradient with respect to x to g[3].  Returns the least clearance (+inf with an empty world).
template <bool COST>
DRM_HD float coll_world_sphere(const float *x, float r, const float *ws, int n_ws, const float *wb, int n_wb, const CollLaw &L, float &cost,
                               float *g) {
    float least = INFINITY;
#pragma unroll 1
    for (int m = 0; m < n_ws; ++m) {
        const float *o = ws + COLL_SPHERE_FLOATS * m;
        float n[3];
        const float d = (coll_point_distance(x, o[0], o[1], o[2], n) - o[3]) - r;
        least = fminf(least, d);
        if constexpr (COST) {
            float phi, dphi;
            coll_phi(L, d, phi, dphi);
            cost = __builtin_fmaf(L.w, phi, cost);
            const float s = L.w * dphi;
#pragma unroll
            for (int i = 0; i < 3; ++i) g[i] = __builtin_fmaf(-s, n[i], g[i]);
        }
    }
#pragma unroll 1
    for (int m = 0; m < n_wb; ++m) {
        float n[3];
        const float d = coll_box_distance(x, wb + COLL_BOX_FLOATS * m, n) - r;
        least = fminf(least, d);
        if constexpr (COST) {
            float phi, dphi;
            coll_phi(L, d, phi, dphi);
            cost = __builtin_fmaf(L.w, phi, cost);
            const float s = L.w * dphi;
#pragma unroll
            for (int i = 0; i < 3; ++i) g[i] = __builtin_fmaf(-s, n[i], g[i]);
        }
    }
    return least;
}

// the clearance of the pair (i, j) and the direction from x_j to x_i
DRM_HD float coll_pair_distance(const float *xi, const float *xj, float ri, float rj, float *n) {
    return (coll_point_distance(xi, xj[0], xj[1], xj[2], n) - ri) - rj;
}

// (F, M) += the wrench of the gradient g on a sphere at x, about the link origin p
DRM_HD void coll_wrench_add(const float *x, const float *p, const float *g, float *F, float *M) {
    const float d[3] = {x[0] - p[0], x[1] - p[1], x[2] - p[2]};
    float dg[3];
    lk_cross(d, g, dg);
#pragma unroll
    for (int i = 0; i < 3; ++i) { F[i] += g[i]; M[i] += dg[i]; }
}

// the group (0: the root, t + 1: target t) of sphere s in the CSR offsets start[0 .. n_groups]
DRM_HD int coll_group_of(const int32_t *start, int n_groups, int s) {
    int l = 0;
    while (l + 1 < n_groups && start[l + 1] <= s) ++l;
    return l;
}

// ---------------------------------------------------------------------------------------------------------------------------
// One row on the host, and the order of summation every path keeps up to the split of a sum over wavefronts: spheres in grouped
// order against the obstacles in table order, then the pairs in list order.
//   R [T][9], p [T][3]     stored frames and origins of the targets (group t + 1)
//   cen [S][3]             out: the centres
//   F, M [T][3]            out (NULL: not formed): the wrenches about the link origins
//   wd, sd [S]             out (NULL: not formed): least world / self clearance
// Returns the cost.
struct CollTables {
    const float *spheres;   // [S][4]
    const int32_t *start;   // [T + 2]
    int S, T;
    const float *ws, *wb;   // world spheres [n_ws][4], boxes [n_wb][16]
    int n_ws, n_wb;
    const int32_t *pairs;   // [P][2]
    int P;
    CollLaw world, self;
};
inline float coll_row(const CollTables &t, const float *R, const float *p, float *cen, float *F, float *M, float *wd, float *sd) {
    const float I[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, o[3] = {0.0f, 0.0f, 0.0f};
    float cost = 0.0f;
    if (F)
        for (int i = 0; i < 3 * t.T; ++i) F[i] = M[i] = 0.0f;
    for (int l = 0; l < t.T + 1; ++l) {
        const float *Rl = l ? R + 9 * (l - 1) : I, *pl = l ? p + 3 * (l - 1) : o;
        for (int s = t.start[l]; s < t.start[l + 1]; ++s) {
            const float *c = t.spheres + COLL_SPHERE_FLOATS * s;
            float *x = cen + 3 * s, g[3] = {0.0f, 0.0f, 0.0f};
            coll_centre(Rl, pl, c[0], c[1], c[2], x);
            const float least = coll_world_sphere<true>(x, c[3], t.ws, t.n_ws, t.wb, t.n_wb, t.world, cost, g);
            if (wd) wd[s] = least;
            if (F && l) coll_wrench_add(x, pl, g, F + 3 * (l - 1), M + 3 * (l - 1));
        }
    }
    if (sd)
        for (int s = 0; s < t.S; ++s) sd[s] = INFINITY;
    for (int k = 0; k < t.P; ++k) {
        const int i = t.pairs[2 * k], j = t.pairs[2 * k + 1];
        float n[3], phi, dphi;
        const float d = coll_pair_distance(cen + 3 * i, cen + 3 * j, t.spheres[4 * i + 3], t.spheres[4 * j + 3], n);
        if (sd) { sd[i] = fminf(sd[i], d); sd[j] = fminf(sd[j], d); }
        coll_phi(t.self, d, phi, dphi);
        cost = __builtin_fmaf(t.self.w, phi, cost);
        if (F) {
            const float s = t.self.w * dphi;
            const float gi[3] = {-(s * n[0]), -(s * n[1]), -(s * n[2])}, gj[3] = {s * n[0], s * n[1], s * n[2]};
            const int li = coll_group_of(t.start, t.T + 1, i), lj = coll_group_of(t.start, t.T + 1, j);
            if (li) coll_wrench_add(cen + 3 * i, p + 3 * (li - 1), gi, F + 3 * (li - 1), M + 3 * (li - 1));
            if (lj) coll_wrench_add(cen + 3 * j, p + 3 * (lj - 1), gj, F + 3 * (lj - 1), M + 3 * (lj - 1));
        }
    }
    return cost;
}
} // namespace drm

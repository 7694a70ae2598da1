// drm_contact.hpp — include/drm_hip.h drm_contact_torques, drm_contact_torques_vjp and drm_contact_rollout: the contact law of spheres
// on a plane and its backward, the joint-limit springs, and their straight-line forms on a 7-DoF arm chain.  Shared by the kernels (drm_contact.hip) and by the host
// build (drm_cpu.cpp) so that both round the same way.  Kept out of drm_sample.hpp on purpose, as drm_links.hpp is: that header is
// part of the source key of every robot's own kernels (specialize._HEADERS).
//
// Plane {x : n.x = d}, unit normal n.  A contact link has, in drm_link_motion's frame (world axes, at the link origin), origin p,
// linear velocity v, angular velocity w and a sphere of radius rl >= 0 about the origin:
//
//   r     = -rl n                      contact point relative to the origin
//   depth = rl - (n.p - d)
//   v_c   = v + w x r,   v_n = n.v_c,   v_t = v_c - v_n n
//   f_n   = max(0, k depth - c v_n)  if depth > 0,  else 0          (never pulls)
//   f_t   = -min(c_t, mu f_n / |v_t|) v_t                           (0 when mu, c_t, f_n or |v_t| is 0)
//   f     = f_n n + f_t,   m = r x f
//
// f_t is regularised Coulomb friction: viscous with slope c_t, capped at mu f_n.  Joint-limit springs of a DoF with lo < hi:
//
//   q < lo :  tau =  k_l (lo - q) - c_l qd          q > hi :  tau = -k_l (q - hi) - c_l qd          otherwise 0
//
// (a DoF with -inf / +inf bounds is free).  Every product-sum is an explicit fused multiply-add, as in drm_links.hpp.
#pragma once
#include <math.h>

#include "drm_links.hpp"

namespace drm {

struct ContactPlane {
    float n[3], d, k, c, mu, ct; // unit normal, offset, stiffness, damping, friction coefficient, friction slope
};

// checks a drm_contact_plane and normalises its normal in double: 0, or the number of the first thing that is wrong
// (1: a parameter is not finite or negative, 2: the normal is zero or not finite)
inline int contact_plane_make(const drm_contact_plane *in, ContactPlane &out) {
    const float par[4] = {in->stiffness, in->damping, in->friction, in->friction_slope};
    for (int i = 0; i < 4; ++i)
        if (!(par[i] >= 0.0f) || !(par[i] <= 3.0e38f)) return 1;
    if (!(fabsf(in->offset) <= 3.0e38f)) return 1;
    const double x = in->normal[0], y = in->normal[1], z = in->normal[2];
    const double len = sqrt(x * x + y * y + z * z);
    if (!(len > 0.0) || !(len <= 3.0e38)) return 2;
    out.n[0] = (float)(x / len); out.n[1] = (float)(y / len); out.n[2] = (float)(z / len);
    out.d = in->offset; out.k = in->stiffness; out.c = in->damping; out.mu = in->friction; out.ct = in->friction_slope;
    return 0;
}
inline bool joint_springs_ok(const drm_joint_springs *s) {
    return s->stiffness >= 0.0f && s->stiffness <= 3.0e38f && s->damping >= 0.0f && s->damping <= 3.0e38f;
}

// the wrench (f, m) of the plane on one link, about the link origin
DRM_HD void contact_wrench(const ContactPlane &pl, float rl, const float *p, const float *v, const float *w, float *f, float *m) {
    const float r[3] = {-(rl * pl.n[0]), -(rl * pl.n[1]), -(rl * pl.n[2])};
    const float depth = rl - (lk_dot(pl.n[0], pl.n[1], pl.n[2], p[0], p[1], p[2]) - pl.d);
    float wr[3];
    lk_cross(w, r, wr);
    const float vc[3] = {v[0] + wr[0], v[1] + wr[1], v[2] + wr[2]};
    const float vn = lk_dot(pl.n[0], pl.n[1], pl.n[2], vc[0], vc[1], vc[2]);
    const float fn = depth > 0.0f ? fmaxf(0.0f, __builtin_fmaf(pl.k, depth, -(pl.c * vn))) : 0.0f;
    float vt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) vt[i] = __builtin_fmaf(-vn, pl.n[i], vc[i]);
    const float speed = sqrtf(lk_dot(vt[0], vt[1], vt[2], vt[0], vt[1], vt[2]));
    const float cap = pl.mu * fn;
    const bool slides = cap > 0.0f && pl.ct > 0.0f && speed > 0.0f;
    const float g = slides ? fminf(pl.ct, cap / speed) : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = __builtin_fmaf(fn, pl.n[i], -(g * vt[i]));
    lk_cross(r, f, m);
}

DRM_HD float joint_spring_torque(float k, float c, float lo, float hi, float q, float qd) {
    if (q < lo) return __builtin_fmaf(k, lo - q, -(c * qd));
    if (q > hi) return -__builtin_fmaf(k, q - hi, c * qd);
    return 0.0f;
}

// The law and its backward on one link (include/drm_hip.h drm_contact_torques_vjp).  (f, m) are contact_wrench's, to the bit; (a, b)
// are the cotangents of (f, m) and (gp, gv, gw) those of (p, v, w) they give, going back through the definitions above:
//   m = r x f               gf  = a + b x r
//   f = f_n n - g v_t       gfn = gf.n,  gg = -(gf.v_t),  gvt = -g gf
//   g = mu f_n / |v_t|      (saturated only; viscous g = c_t is a constant)  gfn += gg mu / |v_t|,  gvt += -(gg g / |v_t|) v_t / |v_t|
//   v_t = v_c - v_n n       gvc = gvt,  gvn = -(gvt.n)
//   f_n = k depth - c v_n   (depth > 0 and f_n > 0 only)  gdepth = k gfn,  gvn -= c gfn
//   v_n = n.v_c             gvc += gvn n
//   v_c = v + w x r         gv = gvc,  gw = r x gvc
//   depth = rl - (n.p - d)  gp = -gdepth n
// At a switch the derivative is that of the branch the forward took; an exact tie in fminf goes to the viscous branch.
DRM_HD void contact_wrench_vjp(const ContactPlane &pl, float rl, const float *p, const float *v, const float *w, const float *a,
                               const float *b, float *f, float *m, float *gp, float *gv, float *gw, float *gdepth_out = nullptr) {
    const float r[3] = {-(rl * pl.n[0]), -(rl * pl.n[1]), -(rl * pl.n[2])};
    const float depth = rl - (lk_dot(pl.n[0], pl.n[1], pl.n[2], p[0], p[1], p[2]) - pl.d);
    float wr[3];
    lk_cross(w, r, wr);
    const float vc[3] = {v[0] + wr[0], v[1] + wr[1], v[2] + wr[2]};
    const float vn = lk_dot(pl.n[0], pl.n[1], pl.n[2], vc[0], vc[1], vc[2]);
    const float fn = depth > 0.0f ? fmaxf(0.0f, __builtin_fmaf(pl.k, depth, -(pl.c * vn))) : 0.0f;
    float vt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) vt[i] = __builtin_fmaf(-vn, pl.n[i], vc[i]);
    const float speed = sqrtf(lk_dot(vt[0], vt[1], vt[2], vt[0], vt[1], vt[2]));
    const float cap = pl.mu * fn;
    const bool slides = cap > 0.0f && pl.ct > 0.0f && speed > 0.0f;
    const float g = slides ? fminf(pl.ct, cap / speed) : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = __builtin_fmaf(fn, pl.n[i], -(g * vt[i]));
    lk_cross(r, f, m);

    const bool pushes = fn > 0.0f, saturated = slides && (cap / speed < pl.ct);
    float br[3];
    lk_cross(b, r, br);
    const float gf[3] = {a[0] + br[0], a[1] + br[1], a[2] + br[2]};
    float gfn = lk_dot(gf[0], gf[1], gf[2], pl.n[0], pl.n[1], pl.n[2]);
    float gvt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) gvt[i] = -(g * gf[i]);
    if (saturated) {
        const float gg = -lk_dot(gf[0], gf[1], gf[2], vt[0], vt[1], vt[2]), inv = 1.0f / speed;
        gfn = __builtin_fmaf(gg, pl.mu * inv, gfn);
        const float along = -((gg * g) * inv) * inv; // gspeed / |v_t|
#pragma unroll
        for (int i = 0; i < 3; ++i) gvt[i] = __builtin_fmaf(along, vt[i], gvt[i]);
    }
    const float gpre = pushes ? gfn : 0.0f;
    const float gvn = __builtin_fmaf(-pl.c, gpre, -lk_dot(gvt[0], gvt[1], gvt[2], pl.n[0], pl.n[1], pl.n[2]));
    const float gdepth = pl.k * gpre;
    float gvc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gvc[i] = pushes ? __builtin_fmaf(gvn, pl.n[i], gvt[i]) : 0.0f;
        gv[i] = gvc[i];
        gp[i] = -(gdepth * pl.n[i]);
    }
    lk_cross(r, gvc, gw);
    if (gdepth_out) *gdepth_out = gdepth; // gp = -gdepth n
}

// the backward of joint_spring_torque under the cotangent lam of the torque: what it adds to grad_q and grad_qd of the DoF
DRM_HD void joint_spring_vjp(float k, float c, float lo, float hi, float q, float lam, float &gq, float &gqd) {
    if (q < lo || q > hi) {
        gq = __builtin_fmaf(-k, lam, gq);
        gqd = __builtin_fmaf(-c, lam, gqd);
    }
}

// The contact torques of a serial chain whose first NJ ops are revolute joints driving DoF columns 0 .. NJ-1 and whose ops
// NJ .. LINKS-1 are fixed, every op a contact link (drm_links.hpp link_chain_*), on cos / sin the caller already has.  ONE sweep
// outwards with velocities keeps the origins and the joint axes; the law per link; one sweep inwards (link_chain_torques', without
// its second sweep outwards).
//   radius(k)                   the sphere of op k's link
//   emit(k, f[3], m[3])         the wrench on op k's link
//   jout(dof, tau)
template <int LINKS, int NJ, class ROW, class RADIUS, class EMIT, class JOUT>
DRM_HD void contact_chain_torques(ROW row, const ContactPlane &pl, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ],
                                  RADIUS radius, EMIT emit, JOUT jout) {
    float p[LINKS][3], z[NJ][3], f[LINKS][3], m[LINKS][3];
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
                p[k][i] = cur.p[i];
                if (k < NJ) z[k < NJ ? k : 0][i] = cur.R[3 * i + 2];
            }
            contact_wrench(pl, radius(k), cur.p, cur.v, cur.w, f[k], m[k]);
            emit(k, f[k], m[k]);
        }
    }
    float Fc[3] = {0.0f, 0.0f, 0.0f}, Mc[3] = {0.0f, 0.0f, 0.0f}; // what op k + 1 hands up, about op k's origin
#pragma unroll
    for (int k = LINKS - 1; k >= 0; --k) {
        float F[3], M[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { F[i] = f[k][i] + Fc[i]; M[i] = m[k][i] + Mc[i]; }
        if (k < NJ) jout(k, link_joint_torque(z[k < NJ ? k : 0], F, M, false));
        if (k > 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { Fc[i] = 0.0f; Mc[i] = 0.0f; }
            link_wrench_up(p[k], p[k > 0 ? k - 1 : 0], F, M, Fc, Mc);
        }
    }
}

// The vector-Jacobian product of contact_chain_torques under the cotangent lam of its torques, on the same chain (springs not
// included).  ONE sweep outwards carries the velocities at rates qd, (v, w), and at rates lam, (a, b) — the cotangents of the wrenches
// — together; the law and its backward run per link on the spot.  ONE sweep inwards carries three wrench sets and two free vectors:
//   1  (f, m) with the velocities (a, b)        drm_link_power_dq(q, lam, f, m): dS/dq with the wrenches held fixed
//   2  (gp, 0)                                  drm_external_torques(q, gp, 0): the positions' share of grad_q
//   3  (gv, gw) with the velocities (v, w)      drm_link_power_dq(q, qd, gv, gw): the velocities' share of grad_q; its torques are grad_qd
// each by link_chain_power_dq's / link_chain_torques' own operations in their own order.
//   jout(dof, grad_q, grad_qd)
template <int LINKS, int NJ, class ROW, class RADIUS, class JOUT>
DRM_HD void contact_chain_torques_vjp(ROW row, const ContactPlane &pl, const float (&cs)[NJ], const float (&sn)[NJ], const float (&qd)[NJ],
                                      const float (&lam)[NJ], RADIUS radius, JOUT jout) {
    float p[LINKS][3], z[NJ][3], v[LINKS][3], w[LINKS][3], a[LINKS][3], b[LINKS][3];
    float f[LINKS][3], gd[LINKS], gv[LINKS][3]; // (gp = -gd n, m = r x f and gw = r x gv are formed again on the way in)
    {
        LinkState cur;
        link_state_root(cur);
        float av[3] = {0.0f, 0.0f, 0.0f}, bv[3] = {0.0f, 0.0f, 0.0f}; // the velocity of the origin and the angular velocity at rates lam
#pragma unroll
        for (int k = 0; k < LINKS; ++k) {
            const OpFT o = load_ft(row(k));
            float J[9], t[3], r[3], br[3];
            link_joint_transform(o, k < NJ, false, 0.0f, k < NJ ? cs[k] : 1.0f, k < NJ ? sn[k] : 0.0f, J, t);
#pragma unroll
            for (int i = 0; i < 3; ++i) r[i] = lk_dot(cur.R[i * 3 + 0], cur.R[i * 3 + 1], cur.R[i * 3 + 2], t[0], t[1], t[2]); // link_step's
            link_step<true, false>(J, t, k < NJ, false, k < NJ ? qd[k] : 0.0f, 0.0f, cur);
            lk_cross(bv, r, br);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                av[i] += br[i];
                if (k < NJ) bv[i] = __builtin_fmaf(cur.R[3 * i + 2], lam[k < NJ ? k : 0], bv[i]);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                p[k][i] = cur.p[i]; v[k][i] = cur.v[i]; w[k][i] = cur.w[i]; a[k][i] = av[i]; b[k][i] = bv[i];
                if (k < NJ) z[k < NJ ? k : 0][i] = cur.R[3 * i + 2];
            }
            float mk[3], gwk[3], gpk[3];
            contact_wrench_vjp(pl, radius(k), cur.p, cur.v, cur.w, av, bv, f[k], mk, gpk, gv[k], gwk, &gd[k]);
        }
    }
    float F1[3] = {0.0f, 0.0f, 0.0f}, M1[3] = {0.0f, 0.0f, 0.0f}, A1[3] = {0.0f, 0.0f, 0.0f};
    float F2[3] = {0.0f, 0.0f, 0.0f}, M2[3] = {0.0f, 0.0f, 0.0f};
    float F3[3] = {0.0f, 0.0f, 0.0f}, M3[3] = {0.0f, 0.0f, 0.0f}, A3[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = LINKS - 1; k >= 0; --k) {
        float Fa[3], Ma[3], Fb[3], Mb[3], Fc[3], Mc[3], mk[3], gwk[3];
        const float rl = radius(k), r[3] = {-(rl * pl.n[0]), -(rl * pl.n[1]), -(rl * pl.n[2])};
        const float *ak = a[k], *bk = b[k], *wk = w[k];
        const float gpk[3] = {-(gd[k] * pl.n[0]), -(gd[k] * pl.n[1]), -(gd[k] * pl.n[2])};
        lk_cross(r, f[k], mk);   // contact_wrench_vjp's m and gw, to the bit
        lk_cross(r, gv[k], gwk);
        link_power_own(ak, bk, f[k], mk, A1);
        link_power_own(v[k], wk, gv[k], gwk, A3);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Fa[i] = f[k][i] + F1[i]; Ma[i] = mk[i] + M1[i];
            Fb[i] = gpk[i] + F2[i]; Mb[i] = 0.0f + M2[i];
            Fc[i] = gv[k][i] + F3[i]; Mc[i] = gwk[i] + M3[i];
        }
        if (k < NJ) {
            const float *zk = z[k < NJ ? k : 0];
            const float d1 = link_joint_power_dq(zk, ak, bk, Fa, Ma, A1, false);
            const float t2 = link_joint_torque(zk, Fb, Mb, false);
            const float d3 = link_joint_power_dq(zk, v[k], wk, Fc, Mc, A3, false);
            jout(k, (d1 + t2) + d3, link_joint_torque(zk, Fc, Mc, false));
        }
        if (k > 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { F1[i] = M1[i] = F2[i] = M2[i] = F3[i] = M3[i] = 0.0f; }
            link_wrench_up(p[k], p[k > 0 ? k - 1 : 0], Fa, Ma, F1, M1);
            link_wrench_up(p[k], p[k > 0 ? k - 1 : 0], Fb, Mb, F2, M2);
            link_wrench_up(p[k], p[k > 0 ? k - 1 : 0], Fc, Mc, F3, M3);
        }
    }
}
} // namespace drm

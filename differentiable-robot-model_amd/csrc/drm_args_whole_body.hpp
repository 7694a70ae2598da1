// drm_args_whole_body.hpp — what include/drm_hip_whole_body.h drm_whole_body asks of its ARGUMENTS, written once for both builds of the
// C ABI, as drm_args.hpp does for the entry points of include/drm_hip.h: libdrm_hip.so (drm_whole_body.hip) and libdrm_cpu.so
// (drm_cpu.cpp) start the call with args_whole_body() and so refuse the same calls with the same code and the same drm_last_error().
// tests/test_whole_body_abi.py holds the table of them.  The walk is asked what drm_args.hpp's tree sweeps ask of theirs.
//
// The total mass is not looked at here: the masses live in the walk's table, which is the device's in libdrm_hip.so, and the call
// never synchronises the host.  A robot without mass gets NaN rows; the Python layer, which knows the masses, refuses it.
#pragma once
#include <cmath>

#include "../../include/drm_hip_whole_body.h"
#include "drm_args.hpp"

namespace drm {

// the base share as both builds compute with it: mass, first moment (zeros: left out)
struct WholeBodyBase {
    float v[4];
};
static inline int args_whole_body(const drm_walk *w, const float *q, const float *qd, int64_t B, const drm_base_share *base, const float *com,
                                  const float *com_vel, const float *com_acc, const float *com_jac, const float *ang_mom, const float *force,
                                  const float *moment, WholeBodyBase &b) {
    b = WholeBodyBase{};
    if (int rc = check_sweep_walk(w)) return rc;
    if (!q) return fail(DRM_ERR_INVALID, "q must not be NULL");
    if (!com && !com_vel && !com_acc && !com_jac && !ang_mom && !force && !moment) return fail(DRM_ERR_INVALID, "every output is NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    if (!qd && (com_vel || com_acc || ang_mom)) return fail(DRM_ERR_INVALID, "com_vel / com_acc / ang_mom need qd");
    if (base) {
        const bool finite = std::isfinite(base->mass) && std::isfinite(base->mc[0]) && std::isfinite(base->mc[1]) && std::isfinite(base->mc[2]);
        if (!finite || base->mass < 0.0f) return fail(DRM_ERR_INVALID, "the base share must be finite and its mass >= 0");
        b.v[0] = base->mass; b.v[1] = base->mc[0]; b.v[2] = base->mc[1]; b.v[3] = base->mc[2];
    }
    return DRM_OK;
}
// 0: positions; 1: + velocities; 2: + accelerations.  The wrench of a call without qd and qdd is the static one: positions do.
static inline int whole_body_level(const float *qd, const float *qdd, const float *com_vel, const float *com_acc, const float *ang_mom,
                                   const float *force, const float *moment) {
    if (com_acc || ((force || moment) && (qd || qdd))) return 2;
    return (com_vel || ang_mom) ? 1 : 0;
}

} // namespace drm

// drm_rollout.hpp — ABI 14 (include/drm_hip.h drm_forward_dynamics_rollout): the integrator of a rollout step, shared by the device
// kernels (drm_rollout.hip) and the host build (drm_cpu.cpp) so that both round the same way.  Kept out of drm_sample.hpp on purpose:
// that header is part of the source key of every robot's own kernels (specialize._HEADERS).
#pragma once
#include "drm_sample.hpp"

namespace drm {
// One Euler step of one coordinate, each update a single fused multiply-add:
//   semi-implicit (default)   qd' = qd + dt * qdd,  q' = q + dt * qd'
//   explicit                  q'  = q + dt * qd,    qd' = qd + dt * qdd
DRM_HD void rollout_step(float &q, float &qd, float qdd, float dt, bool explicit_euler) {
    const float v1 = fmaf(dt, qdd, qd);
    q = fmaf(dt, explicit_euler ? qd : v1, q);
    qd = v1;
}
} // namespace drm

/*
 * drm_hip_whole_body.h — what the robot does AS A WHOLE, in ONE call: its centre of mass, the CoM's velocity, acceleration and
 * Jacobian, its angular momentum, and the wrench its mount has to supply.  An addition to drm_hip.h (which it includes for drm_walk
 * and the error codes); DRM_ABI_VERSION stays as it is.  Both builds of the C ABI (libdrm_hip.so, libdrm_cpu.so) export these names.
 *
 * World is the base frame, z up, g = 9.81, as drm_energy and drm_link_motion use them.  Body i: mass m_i, centre of mass c_i, angular
 * velocity / acceleration w_i / al_i, classical velocity / acceleration v_ci / a_ci of c_i, inertia I_i about c_i in base axes.
 * "Moved" bodies have at least one joint on their path to the root; the base and whatever is fixed to it are the BASE SHARE, a
 * constant (mass, first moment) in the base frame that the caller hands in.  M = sum m_i over all of them.
 *
 *   com      [B, 3]      sum m_i c_i / M
 *   com_vel  [B, 3]      sum_moved m_i v_ci / M.  The linear momentum is M com_vel.
 *   com_acc  [B, 3]      sum_moved m_i a_ci / M
 *   com_jac  [B, 3, n]   column j: z_j x (mc_sub,j - m_sub,j p_j) / M for a revolute joint, z_j m_sub,j / M for a prismatic one (z_j the
 *                        world joint axis, p_j the joint origin, (m, mc)_sub,j mass and world first moment of joint j's sub-tree).
 *                        com_jac qd = com_vel, and com_jac^T (0, 0, M g) = drm_energy's g.  The base share enters M only.
 *   ang_mom  [B, 3]      sum_moved (c_i x m_i v_ci + I_i w_i): the angular momentum about the base ORIGIN.  About the centre of mass it
 *                        is ang_mom - com x M com_vel.
 *   force, moment [B, 3] the wrench the mount applies to the base link, at the base origin in base axes, that keeps the base at rest:
 *                        force  = sum_moved m_i a_ci + [gravity] M g e_z
 *                        moment = sum_moved (c_i x m_i a_ci + I_i al_i + w_i x I_i w_i) + [gravity] (sum m_i c_i) x g e_z
 *                        — the root wrench that drm_rnea drops.  Joint damping does not enter.  The wrench the robot applies to its
 *                        mount is the negative; the ZMP on the plane z = 0 is (-moment_y / force_z, moment_x / force_z).
 *
 * walk     the whole-tree dynamics walk, the one drm_energy takes
 * qd, qdd  [B, n], NULL: zero.  com_vel, ang_mom and com_acc need qd.  force / moment are always allowed; with qd and qdd NULL they
 *          are the static wrench.
 * flags    DRM_RNEA_GRAVITY (the wrench only) | DRM_WHOLE_BODY_COMPOSED
 * base     HOST struct, read during the call; NULL leaves the base share out
 * Any output may be NULL, not all of them.  Only the levels the requested outputs need are computed (positions; + velocities;
 * + accelerations), drm_link_motion's rule.
 *
 * One sweep out and one back over the tree (csrc/drm_whole_body.hpp), every quantity in its link's own frame.  Serial 7-DoF arm chains
 * (DRM_WALK_ARM_CHAIN, capacity 8), full 64-row tiles, every pointer and the table 16-byte aligned: ONE kernel, one wavefront per tile,
 * one row per lane, everything in registers, the tiles in and out through LDS in 16-byte accesses (28 - 84 B in, up to 156 B out per
 * row).  Every other walk, the ragged tail, misaligned pointers and DRM_WHOLE_BODY_COMPOSED: one lane per row and two loops over the ops.
 * A row with a q / qd / qdd that is not finite, or with a |q| beyond 1e5, gets NaN in every output that is written and changes no bit
 * of any other row.  A robot whose total mass is zero gets NaN everywhere: the masses live in the device's table, which the call does
 * not read on the host.
 *   scratch   drm_whole_body_scratch_floats_aligned floats when every pointer is 16-byte aligned, drm_whole_body_scratch_floats floats
 *             otherwise and with DRM_WHOLE_BODY_COMPOSED: the rows' records between the sweeps where 64 rows of them do not fit the
 *             general kernel's LDS budget (up to 28 n_ops + 16 n_slots floats per row and at most 2 048 tiles of 64 rows at a time;
 *             0 where nothing is needed: scratch may then be NULL)
 * DRM_ERR_INVALID for a NULL q, all seven outputs NULL, a negative B, a velocity-level output without qd, or a base share that is not
 * finite or has a negative mass; B == 0 returns DRM_OK.  Asynchronous on `stream`, never a host synchronisation, no allocation.
 */
#ifndef DRM_HIP_WHOLE_BODY_H
#define DRM_HIP_WHOLE_BODY_H

#include "drm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRM_WHOLE_BODY_COMPOSED 2048 /* force the general kernel on every row (tests, A/B) */

typedef struct drm_base_share {
    float mass, mc[3]; /* of the bodies no joint moves: mass and first moment sum m_i c_i in the base frame */
} drm_base_share;

int64_t drm_whole_body_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_whole_body_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_whole_body(const drm_walk *walk, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                   const drm_base_share *base, float *com, float *com_vel, float *com_acc, float *com_jac, float *ang_mom, float *force,
                   float *moment, float *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif

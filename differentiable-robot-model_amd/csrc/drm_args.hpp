// drm_args.hpp — what every work entry point of include/drm_hip.h asks of its ARGUMENTS, written once for both builds of the C ABI:
// libdrm_hip.so (the .hip unit of each entry point) and libdrm_cpu.so (drm_cpu.cpp) start every call with the same args_<entry>() and
// so refuse the same calls with the same code and the same drm_last_error().  tests/test_abi_refusals.py holds the table of them.
//
// Plain host C++17, no HIP types; never included by the device headers.  Each function takes the entry point's arguments without
// scratch and stream, refuses through fail() and returns its code, DRM_OK for a call whose arguments stand.  B == 0 is the caller's to
// answer afterwards.  What only one build's way of computing needs stays in that build: 16-byte alignment, grid and LDS limits,
// segments_ok, the "pass ..._scratch_floats() floats of scratch" refusals and every hipError_t in the .hip units; the rows the host
// loops cannot read in drm_cpu.cpp.
//
// fail() is the including unit's: declared as drm_common.hpp declares it (the .hip units include that first; drm_cpu.cpp repeats the
// declaration) and defined once per library next to its error string.  Its first variadic slot is a string, so a message with numbers
// alone carries a "%s" for the empty one.
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../include/drm_hip.h"
#include "drm_collision.hpp"
#include "drm_contact.hpp"
#include "drm_regressor.hpp"

namespace drm {

// ---- walks ---------------------------------------------------------------------------------------------------------------------
inline int check_walk(const drm_walk *w) {
    if (!w) return fail(DRM_ERR_INVALID, "walk is NULL");
    if (!w->ops_f || !w->ops_i) return fail(DRM_ERR_INVALID, "walk tables are NULL");
    const int c = w->capacity;
    if (c < 4 || (c & 3) || c > 0xffff) return fail(DRM_ERR_INVALID, "walk capacity %s%ld is not a multiple of 4 in [4, 65535]", "", c);
    if (w->n_ops < 0 || w->n_ops > c) return fail(DRM_ERR_INVALID, "walk has %s%ld ops but capacity %ld", "", w->n_ops, c);
    if (w->n_dofs < 1 || w->n_dofs > DRM_MAX_DOFS) return fail(DRM_ERR_UNSUPPORTED, "n_dofs %s%ld outside [1, %ld]", "", w->n_dofs, DRM_MAX_DOFS);
    if (w->n_slots < 0 || w->n_slots > DRM_MAX_SLOTS)
        return fail(DRM_ERR_UNSUPPORTED, "walk needs %s%ld save slots, kernels have %ld", "", w->n_slots, DRM_MAX_SLOTS);
    // (seg_begin has DRM_MAX_SEGMENTS + 1 entries; whether the segments are consistent is asked where they are walked)
    if (w->n_segments < 1 || w->n_segments > DRM_MAX_SEGMENTS) return fail(DRM_ERR_INVALID, "walk has %s%ld segments", "", w->n_segments);
    return DRM_OK;
}
// what the tree-sweep entry points ask of a walk: check_walk, and the walk has something to sweep
static inline int check_sweep_walk(const drm_walk *w) {
    if (int rc = check_walk(w)) return rc;
    return w->n_ops < 1 ? fail(DRM_ERR_INVALID, "the walk has no ops") : DRM_OK;
}
// the size of the walks the reverse sweeps take, of a CHECKED walk
static inline int backward_walk_fits(const drm_walk *w) {
    if (w->capacity > DRM_MAX_OPS)
        return fail(DRM_ERR_UNSUPPORTED, "backward walks take at most %s%ld ops (capacity %ld)", "", DRM_MAX_OPS, w->capacity);
    if (w->n_slots > DRM_MAX_SLOTS_BACKWARD)
        return fail(DRM_ERR_UNSUPPORTED, "backward walks take at most %s%ld save slots (%ld)", "", DRM_MAX_SLOTS_BACKWARD, w->n_slots);
    return DRM_OK;
}
static inline int check_backward_walk(const drm_walk *w) {
    if (int rc = check_walk(w)) return rc;
    return backward_walk_fits(w);
}
// the largest table of drm_rnea_regressor: a row of Y is addressed with 32-bit offsets inside the kernels
static inline int check_regressor_walk(const drm_walk *w) {
    if (int rc = check_sweep_walk(w)) return rc;
    if ((int64_t)w->n_dofs * (REG_COLS * (int64_t)w->n_ops + w->n_dofs) >= (1 << 24))
        return fail(DRM_ERR_UNSUPPORTED, "a row of the regressor of this walk has 2^24 entries or more (%s%ld ops, %ld DoFs)", "", w->n_ops, w->n_dofs);
    return DRM_OK;
}

// ---- forward kinematics and the Jacobian ------------------------------------------------------------------------------------------
// drm_fk, drm_fk_links
static inline int args_fk(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const float *pos, const float *quat) {
    if (int rc = check_walk(w)) return rc;
    if (!q || !pos || !quat) return fail(DRM_ERR_INVALID, "q / pos / quat must not be NULL");
    if (B < 0 || n_targets < 1) return fail(DRM_ERR_INVALID, "negative batch or no targets");
    if (n_targets > w->n_ops) return fail(DRM_ERR_INVALID, "more targets than ops in the walk");
    return DRM_OK;
}
// drm_fk_fanout, drm_fk_fanout_links
static inline int args_fk_fanout(const drm_walk *chains, int32_t n_chains, const float *q, int64_t B, const float *pos, const float *quat) {
    if (!chains || n_chains < 2 || n_chains > 4) return fail(DRM_ERR_INVALID, "fan-out FK takes 2 to 4 chains");
    if (!q || !pos || !quat) return fail(DRM_ERR_INVALID, "q / pos / quat must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    for (int t = 0; t < n_chains; ++t) {
        if (int rc = check_walk(chains + t)) return rc;
        if (chains[t].capacity != chains[0].capacity || chains[t].n_dofs != chains[0].n_dofs || chains[t].n_slots != 0)
            return fail(DRM_ERR_INVALID, "fan-out chains must share capacity and n_dofs and have no branch points");
    }
    return DRM_OK;
}
static inline int args_fk_jacobian(const drm_walk *w, const float *q, int64_t B, const float *lin_jac, const float *ang_jac) {
    if (int rc = check_walk(w)) return rc;
    if (!q || !lin_jac || !ang_jac) return fail(DRM_ERR_INVALID, "q / lin_jac / ang_jac must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    if (w->target_perm < 0 || w->target_perm > 5) return fail(DRM_ERR_INVALID, "target_perm must be in 0..5");
    return DRM_OK;
}

// ---- dynamics ----------------------------------------------------------------------------------------------------------------------
static inline int args_rnea(const drm_walk *w, const float *q, const float *qd, int64_t B, const float *tau) {
    if (int rc = check_walk(w)) return rc;
    if (!q || !qd || !tau) return fail(DRM_ERR_INVALID, "q / qd / tau must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
static inline int args_fk_rnea(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int64_t B, const float *tau,
                               const float *pos, const float *quat) {
    if (int rc = check_walk(tree)) return rc;
    if (int rc = check_walk(chain)) return rc;
    if (!q || !qd || !tau || !pos || !quat) return fail(DRM_ERR_INVALID, "q / qd / tau / pos / quat must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    if (tree->n_dofs != chain->n_dofs) return fail(DRM_ERR_INVALID, "the two walks belong to different robots");
    return DRM_OK;
}
// (a gather without destinations is drm_fk_rnea: the rest of such a drm_put is not looked at)
static inline int args_fk_rnea_put(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int64_t B, const float *tau,
                                   const float *pos, const float *quat, const drm_put *put) {
    if (put && put->n_peers != 0 && (put->n_peers < 0 || put->n_peers > DRM_MAX_PEERS || put->row_offset < 0))
        return fail(DRM_ERR_INVALID, "drm_put: n_peers must be 0 .. DRM_MAX_PEERS and row_offset >= 0");
    return args_fk_rnea(tree, chain, q, qd, B, tau, pos, quat);
}
static inline int args_crba(const drm_walk *w, const float *q, int64_t B, const float *H) {
    if (int rc = check_walk(w)) return rc;
    if (!q || !H) return fail(DRM_ERR_INVALID, "q / H must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
static inline int args_forward_dynamics(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, const float *qdd) {
    if (int rc = check_walk(w)) return rc;
    if (!q || !qd || !f || !qdd) return fail(DRM_ERR_INVALID, "q / qd / f / qdd must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
// the trajectory arguments of drm_forward_dynamics_rollout and drm_contact_rollout, of a CHECKED dynamics walk
static inline int args_trajectory(const float *q0, const float *qd0, const float *tau, int32_t T, float dt, const float *q_traj, const float *qd_traj) {
    if (!q0 || !qd0 || !tau || !q_traj || !qd_traj) return fail(DRM_ERR_INVALID, "q0 / qd0 / tau / q_traj / qd_traj must not be NULL");
    if (T < 1) return fail(DRM_ERR_INVALID, "a rollout takes at least one step (T = %s%ld)", "", T);
    if (!(dt > 0.0f) || !std::isfinite(dt)) return fail(DRM_ERR_INVALID, "dt must be finite and positive");
    return DRM_OK;
}
static inline int args_forward_dynamics_rollout(const drm_walk *w, const float *q0, const float *qd0, const float *tau, int64_t B, int32_t T, float dt,
                                                const float *q_traj, const float *qd_traj) {
    if (int rc = check_walk(w)) return rc;
    if (int rc = args_trajectory(q0, qd0, tau, T, dt, q_traj, qd_traj)) return rc;
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
static inline int args_inverse_kinematics(const drm_walk *w, const float *q0, const float *target_pos, const float *target_quat, int64_t B,
                                          int32_t max_iters, float damping, float step, float tol_pos, float tol_rot, const float *lower,
                                          const float *upper, int32_t flags, const float *q, const float *err) {
    if (int rc = check_walk(w)) return rc;
    if (!q0 || !target_pos || !q || !err) return fail(DRM_ERR_INVALID, "q0 / target_pos / q / err must not be NULL");
    if ((target_quat == nullptr) != ((flags & DRM_IK_POSITION_ONLY) != 0))
        return fail(DRM_ERR_INVALID, "target_quat must be NULL iff DRM_IK_POSITION_ONLY");
    if ((lower == nullptr) != (upper == nullptr)) return fail(DRM_ERR_INVALID, "lower and upper must be given together");
    if (max_iters < 0) return fail(DRM_ERR_INVALID, "max_iters must be >= 0");
    if (!(damping > 0.0f) || !std::isfinite(damping) || !(step > 0.0f) || !std::isfinite(step))
        return fail(DRM_ERR_INVALID, "damping and step must be finite and positive");
    if (!(tol_pos >= 0.0f) || !std::isfinite(tol_pos) || !(tol_rot >= 0.0f) || !std::isfinite(tol_rot))
        return fail(DRM_ERR_INVALID, "tolerances must be finite and >= 0");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
static inline int args_operational_space(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int64_t B, float reg,
                                         const float *inertia, const float *jbar, const float *bias_acc, const float *bias_force) {
    if (int rc = check_walk(tree)) return rc;
    if (int rc = check_walk(chain)) return rc;
    if (tree->n_dofs != chain->n_dofs) return fail(DRM_ERR_INVALID, "the two walks belong to different robots");
    if (!inertia && !jbar && !bias_acc && !bias_force) return fail(DRM_ERR_INVALID, "every output is NULL");
    if (!q || (!qd && (bias_acc || bias_force)))
        return fail(DRM_ERR_INVALID, "q must not be NULL, nor qd when bias_acc / bias_force are asked for");
    if (!(reg >= 0.0f) || !std::isfinite(reg)) return fail(DRM_ERR_INVALID, "reg must be finite and >= 0");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
static inline int args_forward_dynamics_derivatives(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, const float *qdd,
                                                    const float *dq, const float *dqd, const float *minv) {
    if (int rc = check_backward_walk(w)) return rc;
    if (!q || !qd || !f) return fail(DRM_ERR_INVALID, "q / qd / f must not be NULL");
    if (!qdd || !dq || !dqd || !minv) return fail(DRM_ERR_INVALID, "qdd / dqdd_dq / dqdd_dqd / minv must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}

// ---- the tree sweeps -----------------------------------------------------------------------------------------------------------------
static inline int args_rnea_regressor(const drm_walk *w, const float *q, const float *qd, int64_t B, const float *Y) {
    if (int rc = check_regressor_walk(w)) return rc;
    if (!q || !qd || !Y) return fail(DRM_ERR_INVALID, "q / qd / Y must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
// drm_lagrangian_dynamics (any_output = H || C || g) and drm_energy (any_output = T || V || p || dT_dq || g)
static inline int args_sweep_q_qd(const drm_walk *w, const float *q, const float *qd, int64_t B, bool any_output) {
    if (int rc = check_sweep_walk(w)) return rc;
    if (!q || !qd) return fail(DRM_ERR_INVALID, "q / qd must not be NULL");
    if (!any_output) return fail(DRM_ERR_INVALID, "every output is NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}
static inline int args_rnea_derivatives(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, const float *tau,
                                        const float *dq, const float *dqd, const float *H) {
    if (int rc = check_sweep_walk(w)) return rc;
    if (!q || !qd || !qdd) return fail(DRM_ERR_INVALID, "q / qd / qdd must not be NULL");
    if (!tau && !dq && !dqd && !H) return fail(DRM_ERR_INVALID, "every output is NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    return DRM_OK;
}

// ---- links ---------------------------------------------------------------------------------------------------------------------------
// what every entry point over the targets of a link walk asks first
static inline int args_links(const drm_walk *w, const float *q, int64_t B, int32_t n_targets) {
    if (int rc = check_sweep_walk(w)) return rc;
    if (!q) return fail(DRM_ERR_INVALID, "q must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    if (n_targets < 1 || n_targets > w->n_ops) return fail(DRM_ERR_INVALID, "n_targets is not the walk's number of output slots");
    return DRM_OK;
}
static inline int args_link_motion(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const float *pos, const float *lin_vel,
                                   const float *ang_vel, const float *lin_acc, const float *ang_acc) {
    if (int rc = args_links(w, q, B, n_targets)) return rc;
    if (!pos && !lin_vel && !ang_vel && !lin_acc && !ang_acc) return fail(DRM_ERR_INVALID, "every output is NULL");
    return DRM_OK;
}
static inline int args_external_torques(const drm_walk *w, const float *q, const float *force, const float *torque, int64_t B, int32_t n_targets,
                                        const float *tau) {
    if (int rc = args_links(w, q, B, n_targets)) return rc;
    if (!force && !torque) return fail(DRM_ERR_INVALID, "force and torque are both NULL");
    if (!tau) return fail(DRM_ERR_INVALID, "tau must not be NULL");
    return DRM_OK;
}
static inline int args_link_power_dq(const drm_walk *w, const float *q, const float *qd, const float *force, const float *torque, int64_t B,
                                     int32_t n_targets, const float *dq) {
    if (int rc = args_links(w, q, B, n_targets)) return rc;
    if (!qd) return fail(DRM_ERR_INVALID, "qd must not be NULL");
    if (!force && !torque) return fail(DRM_ERR_INVALID, "force and torque are both NULL");
    if (!dq) return fail(DRM_ERR_INVALID, "dq must not be NULL");
    return DRM_OK;
}

// ---- contact -------------------------------------------------------------------------------------------------------------------------
// the contact arguments as both builds compute with them
struct ContactPlan {
    ContactPlane pl;
    bool has_plane;
    const float *radius;
    float k, c;                 // of the joint-limit springs
    const float *lower, *upper; // NULL: no joint-limit springs
};
// what the three contact entry points ask of their contact arguments
static inline int args_contact(const drm_walk *lw, int64_t B, int32_t n_targets, const drm_contact_plane *plane, const float *radius,
                               const drm_joint_springs *springs, const float *lower, const float *upper, ContactPlan &a) {
    a = ContactPlan{};
    if (!plane && !springs) return fail(DRM_ERR_INVALID, "neither a contact plane nor joint-limit springs");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    if (plane) {
        if (int rc = check_sweep_walk(lw)) return rc;
        if (n_targets < 1 || n_targets > lw->n_ops) return fail(DRM_ERR_INVALID, "n_targets is not the walk's number of output slots");
        const int bad = contact_plane_make(plane, a.pl);
        if (bad == 1) return fail(DRM_ERR_INVALID, "the plane's offset must be finite, its stiffness, damping, friction and slope finite and >= 0");
        if (bad) return fail(DRM_ERR_INVALID, "the plane's normal must be finite and not zero");
        a.has_plane = true;
        a.radius = radius;
    }
    if (springs) {
        if (!joint_springs_ok(springs)) return fail(DRM_ERR_INVALID, "the joint springs' stiffness and damping must be finite and >= 0");
        if (!lower || !upper) return fail(DRM_ERR_INVALID, "joint springs need lower and upper");
        a.k = springs->stiffness; a.c = springs->damping; a.lower = lower; a.upper = upper;
    }
    return DRM_OK;
}
static inline int args_contact_torques(const drm_walk *lw, const float *q, const float *qd, int64_t B, int32_t n_targets,
                                       const drm_contact_plane *plane, const float *radius, const drm_joint_springs *springs, const float *lower,
                                       const float *upper, const float *tau, ContactPlan &a) {
    if (int rc = check_sweep_walk(lw)) return rc;
    if (!q || !qd || !tau) return fail(DRM_ERR_INVALID, "q / qd / tau must not be NULL");
    if (!plane) return fail(DRM_ERR_INVALID, "drm_contact_torques needs a plane");
    return args_contact(lw, B, n_targets, plane, radius, springs, lower, upper, a);
}
static inline int args_contact_torques_vjp(const drm_walk *lw, const float *q, const float *qd, const float *grad_tau, int64_t B, int32_t n_targets,
                                           const drm_contact_plane *plane, const float *radius, const drm_joint_springs *springs, const float *lower,
                                           const float *upper, const float *grad_q, const float *grad_qd, ContactPlan &a) {
    if (int rc = check_sweep_walk(lw)) return rc;
    if (!q || !qd || !grad_tau) return fail(DRM_ERR_INVALID, "q / qd / grad_tau must not be NULL");
    if (!grad_q && !grad_qd) return fail(DRM_ERR_INVALID, "grad_q and grad_qd are both NULL");
    return args_contact(lw, B, n_targets, plane, radius, springs, lower, upper, a);
}
static inline int args_contact_rollout(const drm_walk *dw, const drm_walk *lw, const float *q0, const float *qd0, const float *tau, int64_t B,
                                       int32_t T, float dt, int32_t n_targets, const drm_contact_plane *plane, const float *radius,
                                       const drm_joint_springs *springs, const float *lower, const float *upper, const float *q_traj,
                                       const float *qd_traj, ContactPlan &a) {
    if (int rc = check_walk(dw)) return rc;
    if (int rc = args_trajectory(q0, qd0, tau, T, dt, q_traj, qd_traj)) return rc;
    if (int rc = args_contact(lw, B, n_targets, plane, radius, springs, lower, upper, a)) return rc;
    if (plane && lw->n_dofs != dw->n_dofs) return fail(DRM_ERR_INVALID, "the two walks are not of one robot");
    return DRM_OK;
}

// ---- collision -----------------------------------------------------------------------------------------------------------------------
// what drm_collision_cost and drm_sphere_distances ask of the arguments they share; the tables of the call in `t`, its laws the
// neutral one
static inline int args_collision(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const drm_collision_spheres *spheres,
                                 const drm_collision_world *world, const drm_collision_pairs *pairs, CollTables &t) {
    t = CollTables{};
    if (int rc = args_links(w, q, B, n_targets)) return rc;
    if (!spheres || !spheres->spheres || !spheres->start) return fail(DRM_ERR_INVALID, "spheres, their table and their offsets must not be NULL");
    if (spheres->n_spheres < 1) return fail(DRM_ERR_INVALID, "at least one sphere");
    t.spheres = spheres->spheres; t.start = spheres->start; t.S = spheres->n_spheres; t.T = n_targets;
    if (world) {
        if (world->n_spheres < 0 || world->n_boxes < 0) return fail(DRM_ERR_INVALID, "negative obstacle count");
        if ((world->n_spheres > 0 && !world->spheres) || (world->n_boxes > 0 && !world->boxes)) return fail(DRM_ERR_INVALID, "a world table is NULL");
        t.ws = world->spheres; t.n_ws = world->n_spheres; t.wb = world->boxes; t.n_wb = world->n_boxes;
    }
    if (pairs) {
        if (pairs->n_pairs < 0) return fail(DRM_ERR_INVALID, "negative pair count");
        if (pairs->n_pairs > 0 && !pairs->pairs) return fail(DRM_ERR_INVALID, "the pair list is NULL");
        t.pairs = pairs->pairs; t.P = pairs->n_pairs;
    }
    t.world = t.self = coll_law_make(0.0f, 1.0f);
    return DRM_OK;
}
static inline int args_collision_cost(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const drm_collision_spheres *spheres,
                                      const drm_collision_world *world, const drm_collision_pairs *pairs, const drm_collision_params *params,
                                      const float *cost, const float *dq, CollTables &t) {
    if (int rc = args_collision(w, q, B, n_targets, spheres, world, pairs, t)) return rc;
    if (!world && !pairs) return fail(DRM_ERR_INVALID, "neither a world nor pairs");
    if (!params) return fail(DRM_ERR_INVALID, "params must not be NULL");
    if (!cost && !dq) return fail(DRM_ERR_INVALID, "cost and dq are both NULL");
    if (world && !coll_law_ok(params->world_weight, params->world_activation))
        return fail(DRM_ERR_INVALID, "the world weight must be finite and >= 0, its activation distance finite and > 0");
    if (pairs && !coll_law_ok(params->self_weight, params->self_activation))
        return fail(DRM_ERR_INVALID, "the self weight must be finite and >= 0, its activation distance finite and > 0");
    if (world) t.world = coll_law_make(params->world_weight, params->world_activation);
    if (pairs) t.self = coll_law_make(params->self_weight, params->self_activation);
    return DRM_OK;
}
static inline int args_sphere_distances(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const drm_collision_spheres *spheres,
                                        const drm_collision_world *world, const drm_collision_pairs *pairs, const float *center,
                                        const float *world_distance, const float *self_distance, CollTables &t) {
    if (int rc = args_collision(w, q, B, n_targets, spheres, world, pairs, t)) return rc;
    if (!center && !world_distance && !self_distance) return fail(DRM_ERR_INVALID, "every output is NULL");
    return DRM_OK;
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
// which constants a reverse sweep differentiates: grad_ops_f goes with param_mask, and the mask stays inside the walk
static inline int args_param_mask(const drm_walk *w, uint64_t param_mask, const float *grad_ops_f) {
    if ((param_mask != 0) != (grad_ops_f != nullptr)) return fail(DRM_ERR_INVALID, "grad_ops_f must be given exactly when param_mask selects ops");
    if (w->capacity < 64 && (param_mask >> w->capacity)) return fail(DRM_ERR_INVALID, "param_mask selects ops beyond the walk's capacity");
    return DRM_OK;
}
// drm_fk_backward and drm_fk_jacobian_backward (one target) behind their own rules
static inline int args_fk_backward_common(const drm_walk *w, int64_t B, int32_t n_targets, uint64_t param_mask, const float *grad_q,
                                          const float *grad_ops_f) {
    if (int rc = backward_walk_fits(w)) return rc;
    if (B < 0 || n_targets < 1) return fail(DRM_ERR_INVALID, "negative batch or no targets");
    if (n_targets > w->n_ops) return fail(DRM_ERR_INVALID, "more targets than ops in the walk");
    if (int rc = args_param_mask(w, param_mask, grad_ops_f)) return rc;
    if (!grad_q && !grad_ops_f) return fail(DRM_ERR_INVALID, "nothing to compute: grad_q and grad_ops_f are both NULL");
    return DRM_OK;
}
static inline int args_fk_backward(const drm_walk *w, const float *q, int64_t B, int32_t n_targets, const float *grad_pos, uint64_t param_mask,
                                   const float *grad_q, const float *grad_ops_f) {
    if (int rc = check_walk(w)) return rc;
    if (!q || !grad_pos) return fail(DRM_ERR_INVALID, "q / grad_pos must not be NULL");
    return args_fk_backward_common(w, B, n_targets, param_mask, grad_q, grad_ops_f);
}
static inline int args_fk_jacobian_backward(const drm_walk *w, const float *q, int64_t B, const float *grad_lin_jac, const float *grad_ang_jac,
                                            uint64_t param_mask, const float *grad_q, const float *grad_ops_f) {
    if (int rc = check_walk(w)) return rc;
    if (!q || !grad_lin_jac || !grad_ang_jac) return fail(DRM_ERR_INVALID, "q / grad_lin_jac / grad_ang_jac must not be NULL");
    if (w->n_slots != 0) return fail(DRM_ERR_INVALID, "the walk must be the root->link chain of the Jacobian's target (no branch points)");
    return args_fk_backward_common(w, B, 1, param_mask, grad_q, grad_ops_f);
}
// (both builds keep the loss's partial sums in the scratch: it is an argument like the others here)
static inline int args_fk_mse(const drm_walk *w, const float *q, const float *target, uint64_t param_mask, const float *loss, const float *grad_ops_f,
                              const float *scratch) {
    if (int rc = check_backward_walk(w)) return rc;
    if (!q || !target || !loss || !scratch) return fail(DRM_ERR_INVALID, "q / target / loss / scratch must not be NULL");
    return args_param_mask(w, param_mask, grad_ops_f);
}
static inline int args_fk_mse_links(const drm_walk *w, const int32_t *sel, const float *gsign, const drm_link_pieces *links, int32_t n_links,
                                    const float *q, const float *target, uint64_t param_mask, const float *loss, const float *grad_params,
                                    const float *scratch) {
    if (int rc = check_backward_walk(w)) return rc;
    if (!sel || !gsign || !links || !q || !target || !loss || !grad_params || !scratch)
        return fail(DRM_ERR_INVALID, "drm_fk_mse_links: sel / gsign / links / q / target / loss / grad_params / scratch must not be NULL");
    if (n_links < 1 || n_links > DRM_FK_MSE_MAX_LINKS)
        return fail(DRM_ERR_UNSUPPORTED, "drm_fk_mse_links takes 1 .. %s%ld learnable links (%ld): compose drm_walk_table, drm_fk_mse, "
                                         "drm_walk_table_backward otherwise", "", DRM_FK_MSE_MAX_LINKS, n_links);
    if (!param_mask || (w->capacity < 64 && (param_mask >> w->capacity)))
        return fail(DRM_ERR_INVALID, "param_mask must select ops of the walk (those of the learnable links)");
    for (int l = 0; l < n_links; ++l)
        if (!links[l].rot_angles || !links[l].trans) return fail(DRM_ERR_INVALID, "drm_fk_mse_links: rot_angles / trans of a link are NULL");
    return DRM_OK;
}
static inline int args_rnea_backward(const drm_walk *w, const float *q, const float *qd, int64_t B, const float *grad_tau, uint64_t param_mask,
                                     const float *grad_q, const float *grad_qd, const float *grad_qdd, const float *grad_ops_f) {
    if (int rc = check_backward_walk(w)) return rc;
    if (!q || !qd || !grad_tau) return fail(DRM_ERR_INVALID, "q / qd / grad_tau must not be NULL");
    if (B < 0) return fail(DRM_ERR_INVALID, "negative batch");
    if (int rc = args_param_mask(w, param_mask, grad_ops_f)) return rc;
    const bool want_q = grad_q != nullptr;
    if (want_q != (grad_qd != nullptr) || want_q != (grad_qdd != nullptr))
        return fail(DRM_ERR_INVALID, "grad_q, grad_qd and grad_qdd are produced together: give all three or none");
    if (!want_q && !grad_ops_f) return fail(DRM_ERR_INVALID, "nothing to compute");
    return DRM_OK;
}

// ---- the walk table from the links' parameters ---------------------------------------------------------------------------------------
static inline int args_link_rows(const float *params, int32_t n_links, const float *rows) {
    if (!params || !rows || n_links < 0) return fail(DRM_ERR_INVALID, "params / rows must not be NULL, n_links >= 0");
    return DRM_OK;
}
static inline int args_link_rows_backward(const float *params, const float *grad_rows, int32_t n_links, const float *grad_params) {
    if (!params || !grad_rows || !grad_params || n_links < 0)
        return fail(DRM_ERR_INVALID, "params / grad_rows / grad_params must not be NULL, n_links >= 0");
    return DRM_OK;
}
static inline int args_table_counts(const char *who, int32_t n_links, int32_t n_entries) {
    if (n_links < 1 || n_links > 32 || n_entries < 1 || n_entries > DRM_MAX_OPS * DRM_OPF_STRIDE)
        return fail(DRM_ERR_INVALID, "%s: 1..32 learnable links and at most 32 x 32 walk entries", who);
    return DRM_OK;
}
// drm_walk_table (table = base, out = ops_f) and drm_walk_table_backward (table = grad_ops_f, out = grad_params), named by `who`
static inline int args_walk_table(const char *who, const float *params, int32_t n_links, const float *table, const int32_t *sel, const float *gsign,
                                  int32_t n_entries, const float *out) {
    if (!params || !table || !sel || !gsign || !out) return fail(DRM_ERR_INVALID, "%s: NULL argument", who);
    return args_table_counts(who, n_links, n_entries);
}
// drm_walk_table_links and drm_walk_table_links_backward, the same way
static inline int args_walk_table_links(const char *who, const drm_link_pieces *links, const drm_link_forms *forms, int32_t n_links, const float *table,
                                        const int32_t *sel, const float *gsign, int32_t n_entries, const float *out) {
    if (!table || !sel || !gsign || !out) return fail(DRM_ERR_INVALID, "%s: NULL argument", who);
    if (!links) return fail(DRM_ERR_INVALID, "%s: links must not be NULL", who);
    if (int rc = args_table_counts(who, n_links, n_entries)) return rc;
    for (int l = 0; l < n_links; ++l) {
        if (!links[l].rot_angles || !links[l].trans || !links[l].mass || !links[l].com || !links[l].inertia_mat || !links[l].damping)
            return fail(DRM_ERR_INVALID, "%s: a piece of a link is NULL", who);
        const drm_link_forms f = forms ? forms[l] : drm_link_forms{};
        const bool ok = (f.mass == DRM_FORM_PLAIN || f.mass == DRM_FORM_SQUARE_PLUS) &&
                        (f.damping == DRM_FORM_PLAIN || f.damping == DRM_FORM_SQUARE_PLUS) &&
                        (f.inertia_mat == DRM_FORM_PLAIN || (f.inertia_mat >= DRM_FORM_SYMM && f.inertia_mat <= DRM_FORM_COV));
        if (!ok) return fail(DRM_ERR_INVALID, "%s: unknown form of a piece", who);
    }
    return DRM_OK;
}

} // namespace drm

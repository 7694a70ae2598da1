"""The refusals of the C ABI (include/drm_hip.h), entry point by entry point: the table below is their written specification.

Both builds of the ABI, libdrm_cpu.so and libdrm_hip.so, begin every work entry point with the same function of csrc/drm_args.hpp, so
each row of the table, one fault in an otherwise valid call of B = 0 rows, must be refused by both with the same code and the same
drm_last_error().  A row goes to the host library first and reaches the HIP library only once the host library has refused it as the
table says: nothing here can launch a kernel.  No device is needed: libdrm_hip.so refuses bad arguments before it touches one."""
import ctypes
import os
import re

import numpy as np
import pytest

from differentiable_robot_model_amd import backend
from differentiable_robot_model_amd.flatten import build_walk
from helpers import load_model
from test_host_emu import host_walk

INVALID, UNSUPPORTED = -1, -2
NAN, INF = float("nan"), float("inf")
HEADER = os.path.join(os.path.dirname(os.path.abspath(backend.__file__)), "csrc", "drm_args.hpp")

# the exports without arguments to refuse (queries answer 0 for what they cannot size; drm_special_load belongs to one build)
EXCLUDED = tuple(n for n in backend.EXPORTS if "_scratch_floats" in n) + ("drm_abi_version", "drm_walk_sizeof", "drm_last_error", "drm_special_load")
# a valid call of these writes or launches, whatever its sizes: their baseline goes to the host library alone
NO_EMPTY_CALL = ("drm_walk_table", "drm_walk_table_backward", "drm_walk_table_links", "drm_walk_table_links_backward")
# the loss of these is a mean over B >= 1 rows and their kernels take arm chains only: the baseline of B = 0 rows of the 2-link robot is
# refused by each build's own rule (behind the shared ones, so the rows below still compare)
NO_EMPTY_BATCH = {"drm_fk_mse": "at least one row", "drm_fk_mse_links": "at least one row"}


class Walk:
    """A walk argument: the tree or the chain walk of the 2-link robot with some fields changed."""
    def __init__(self, kind, **fields):
        self.kind, self.fields = kind, fields

    def __call__(self, **fields):
        return Walk(self.kind, **dict(self.fields, **fields))


class Struct:
    """A struct argument passed by pointer: `cls` with the baseline `fields`, some changed."""
    def __init__(self, cls, **fields):
        self.cls, self.fields = cls, fields

    def __call__(self, **fields):
        return Struct(self.cls, **dict(self.fields, **fields))


class Chains:
    """The chains of a fan-out call: the chain walk twice, the second with some fields changed."""
    def __init__(self, **fields):
        self.fields = fields


TREE, CHAIN, BUF = Walk("tree"), Walk("chain"), "a one-row buffer"
PLANE = Struct(backend.DrmContactPlane, normal=(0.0, 0.0, 1.0), offset=0.0, stiffness=100.0, damping=1.0, friction=0.5, friction_slope=10.0)
SPRINGS = Struct(backend.DrmJointSprings, stiffness=10.0, damping=0.1)
SPHERES = Struct(backend.DrmCollisionSpheres, spheres=BUF, start=BUF, n_spheres=1)
WORLD = Struct(backend.DrmCollisionWorld, spheres=BUF, boxes=BUF, n_spheres=1, n_boxes=1)
PAIRS = Struct(backend.DrmCollisionPairs, pairs=BUF, n_pairs=1)
PARAMS = Struct(backend.DrmCollisionParams, world_weight=1.0, world_activation=0.1, self_weight=1.0, self_activation=0.1)
PUT = Struct(backend.DrmPut, n_peers=1, row_offset=0)
LINKS = Struct(backend.DrmLinkPieces, rot_angles=BUF, trans=BUF, mass=BUF, com=BUF, inertia_mat=BUF, damping=BUF)
FORMS = Struct(backend.DrmLinkForms)

# what every walk argument is asked (csrc/drm_args.hpp check_walk), as changes to the walk
WALK_FAULTS = [
    (dict(ops_f=None), INVALID, "walk tables are NULL"),
    (dict(ops_i=None), INVALID, "walk tables are NULL"),
    (dict(capacity=10), INVALID, "walk capacity 10 is not a multiple of 4 in [4, 65535]"),
    (dict(capacity=0), INVALID, "walk capacity 0 is not a multiple of 4"),
    (dict(n_ops=9, capacity=8), INVALID, "walk has 9 ops but capacity 8"),
    (dict(n_ops=-1), INVALID, "walk has -1 ops"),
    (dict(n_dofs=0), UNSUPPORTED, "n_dofs 0 outside [1, 64]"),
    (dict(n_dofs=65), UNSUPPORTED, "n_dofs 65 outside [1, 64]"),
    (dict(n_slots=17), UNSUPPORTED, "walk needs 17 save slots, kernels have 16"),
    (dict(n_segments=0), INVALID, "walk has 0 segments"),
    (dict(n_segments=9), INVALID, "walk has 9 segments"),
]
NO_OPS = (dict(n_ops=0), INVALID, "the walk has no ops")
TOO_LONG = (dict(capacity=68), UNSUPPORTED, "backward walks take at most 64 ops (capacity 68)")
TOO_BRANCHED = (dict(n_slots=7), UNSUPPORTED, "backward walks take at most 6 save slots (7)")


def nulls(names, message):
    return [({n: None}, INVALID, message) for n in names.split()]


def on(walk_arg, base, *faults):
    """walk faults as rows: the walk argument `walk_arg` with each change"""
    return [({walk_arg: base(**change)}, code, message) for change, code, message in faults]


BATCH = [(dict(B=-1), INVALID, "negative batch")]
TARGETS = [(dict(T=0), INVALID, "n_targets is not the walk's number of output slots"),
           (dict(T=4), INVALID, "n_targets is not the walk's number of output slots")]
TRAJECTORY = nulls("q0 qd0 tau q_traj qd_traj", "q0 / qd0 / tau / q_traj / qd_traj must not be NULL") + [
    (dict(T=0), INVALID, "a rollout takes at least one step (T = 0)"),
    (dict(dt=0.0), INVALID, "dt must be finite and positive"), (dict(dt=NAN), INVALID, "dt must be finite and positive"),
    (dict(dt=INF), INVALID, "dt must be finite and positive"), (dict(dt=-0.01), INVALID, "dt must be finite and positive")]
CONTACT = [
    (dict(plane=PLANE(stiffness=-1.0)), INVALID, "the plane's offset must be finite, its stiffness"),
    (dict(plane=PLANE(friction=INF)), INVALID, "the plane's offset must be finite, its stiffness"),
    (dict(plane=PLANE(offset=NAN)), INVALID, "the plane's offset must be finite, its stiffness"),
    (dict(plane=PLANE(normal=(0.0, 0.0, 0.0))), INVALID, "the plane's normal must be finite and not zero"),
    (dict(plane=PLANE(normal=(0.0, NAN, 1.0))), INVALID, "the plane's normal must be finite and not zero"),
    (dict(springs=SPRINGS(stiffness=-1.0)), INVALID, "the joint springs' stiffness and damping must be finite and >= 0"),
    (dict(springs=SPRINGS(damping=NAN)), INVALID, "the joint springs' stiffness and damping must be finite and >= 0"),
    (dict(lower=None), INVALID, "joint springs need lower and upper"), (dict(upper=None), INVALID, "joint springs need lower and upper")]
NO_CONTACT = [(dict(plane=None, springs=None), INVALID, "neither a contact plane nor joint-limit springs")]
LINK_CALL = on("w", TREE, NO_OPS) + nulls("q", "q must not be NULL") + BATCH + TARGETS
COLLISION = LINK_CALL + [
    (dict(spheres=None), INVALID, "spheres, their table and their offsets must not be NULL"),
    (dict(spheres=SPHERES(spheres=None)), INVALID, "spheres, their table and their offsets must not be NULL"),
    (dict(spheres=SPHERES(start=None)), INVALID, "spheres, their table and their offsets must not be NULL"),
    (dict(spheres=SPHERES(n_spheres=0)), INVALID, "at least one sphere"),
    (dict(world=WORLD(n_spheres=-1)), INVALID, "negative obstacle count"), (dict(world=WORLD(n_boxes=-1)), INVALID, "negative obstacle count"),
    (dict(world=WORLD(spheres=None)), INVALID, "a world table is NULL"), (dict(world=WORLD(boxes=None)), INVALID, "a world table is NULL"),
    (dict(pairs=PAIRS(n_pairs=-1)), INVALID, "negative pair count"), (dict(pairs=PAIRS(pairs=None)), INVALID, "the pair list is NULL")]
GRAD_OPS = [(dict(mask=1), INVALID, "grad_ops_f must be given exactly when param_mask selects ops"),
            (dict(gops=BUF), INVALID, "grad_ops_f must be given exactly when param_mask selects ops"),
            (dict(mask=1 << 4, gops=BUF), INVALID, "param_mask selects ops beyond the walk's capacity")]      # (the walks' capacity is 4)


def table_rows(who, table, out):
    return nulls("params %s sel gsign %s" % (table, out), who + ": NULL argument") + [
        (dict(n_links=n), INVALID, who + ": 1..32 learnable links and at most 32 x 32 walk entries") for n in (0, 33)] + [
        (dict(n_entries=n), INVALID, who + ": 1..32 learnable links and at most 32 x 32 walk entries") for n in (0, 2049)]


def table_links_rows(who, table, out):
    return nulls("%s sel gsign %s" % (table, out), who + ": NULL argument") + [
        (dict(links=None), INVALID, who + ": links must not be NULL"),
        (dict(n_links=0), INVALID, who + ": 1..32 learnable links and at most 32 x 32 walk entries"),
        (dict(n_links=33), INVALID, who + ": 1..32 learnable links and at most 32 x 32 walk entries"),
        (dict(n_entries=0), INVALID, who + ": 1..32 learnable links and at most 32 x 32 walk entries"),
        (dict(n_entries=2049), INVALID, who + ": 1..32 learnable links and at most 32 x 32 walk entries"),
        (dict(links=LINKS(mass=None)), INVALID, who + ": a piece of a link is NULL"),
        (dict(links=LINKS(rot_angles=None)), INVALID, who + ": a piece of a link is NULL"),
        (dict(forms=FORMS(mass=7)), INVALID, who + ": unknown form of a piece"),
        (dict(forms=FORMS(inertia_mat=1)), INVALID, who + ": unknown form of a piece"),
        (dict(forms=FORMS(damping=-1)), INVALID, who + ": unknown form of a piece")]


FK = (dict(w=TREE, q=BUF, B=0, T=1, pos=BUF, quat=BUF, stream=None),
      nulls("q pos quat", "q / pos / quat must not be NULL") + [
          (dict(B=-1), INVALID, "negative batch or no targets"), (dict(T=0), INVALID, "negative batch or no targets"),
          (dict(T=4), INVALID, "more targets than ops in the walk")])
FANOUT = (dict(chains=Chains(), n=2, q=BUF, B=0, pos=BUF, quat=BUF, stream=None),
          [(dict(chains=None), INVALID, "fan-out FK takes 2 to 4 chains"), (dict(n=1), INVALID, "fan-out FK takes 2 to 4 chains"),
           (dict(n=5), INVALID, "fan-out FK takes 2 to 4 chains")] + nulls("q pos quat", "q / pos / quat must not be NULL") + BATCH + [
              (dict(chains=Chains(capacity=8)), INVALID, "fan-out chains must share capacity and n_dofs and have no branch points"),
              (dict(chains=Chains(n_dofs=3)), INVALID, "fan-out chains must share capacity and n_dofs and have no branch points"),
              (dict(chains=Chains(n_slots=1)), INVALID, "fan-out chains must share capacity and n_dofs and have no branch points")])
FK_RNEA = nulls("q qd tau pos quat", "q / qd / tau / pos / quat must not be NULL") + BATCH + [
    (dict(chain=CHAIN(n_dofs=1)), INVALID, "the two walks belong to different robots")]
CONTACT_ARGS = dict(plane=PLANE, radius=BUF, springs=SPRINGS, lower=BUF, upper=BUF)

# entry point -> (the baseline call: its arguments in order, the rows: (changes, code, text of the message))
TABLE = {
    "drm_fk": FK,
    "drm_fk_links": FK,
    "drm_fk_fanout": FANOUT,
    "drm_fk_fanout_links": FANOUT,
    "drm_fk_jacobian": (dict(w=CHAIN, q=BUF, B=0, pos=BUF, quat=BUF, lin=BUF, ang=BUF, stream=None),
                        nulls("q lin ang", "q / lin_jac / ang_jac must not be NULL") + BATCH + [
                            (dict(w=CHAIN(target_perm=6)), INVALID, "target_perm must be in 0..5"),
                            (dict(w=CHAIN(target_perm=-1)), INVALID, "target_perm must be in 0..5")]),
    "drm_rnea": (dict(w=TREE, q=BUF, qd=BUF, qdd=BUF, B=0, flags=3, tau=BUF, scratch=BUF, stream=None),
                 nulls("q qd tau", "q / qd / tau must not be NULL") + BATCH),
    "drm_fk_rnea": (dict(tree=TREE, chain=CHAIN, target_op=0, q=BUF, qd=BUF, qdd=BUF, B=0, flags=3, tau=BUF, pos=BUF, quat=BUF, scratch=BUF,
                         stream=None), FK_RNEA),
    "drm_fk_rnea_put": (dict(tree=TREE, chain=CHAIN, target_op=0, q=BUF, qd=BUF, qdd=BUF, B=0, flags=3, tau=BUF, pos=BUF, quat=BUF, scratch=BUF,
                             put=PUT, stream=None),
                        FK_RNEA + [(dict(put=PUT(n_peers=n)), INVALID, "drm_put: n_peers must be 0 .. DRM_MAX_PEERS and row_offset >= 0") for n in (-1, 9)]
                        + [(dict(put=PUT(row_offset=-1)), INVALID, "drm_put: n_peers must be 0 .. DRM_MAX_PEERS and row_offset >= 0")]),
    "drm_crba": (dict(w=TREE, q=BUF, B=0, H=BUF, scratch=BUF, stream=None), nulls("q H", "q / H must not be NULL") + BATCH),
    "drm_forward_dynamics": (dict(w=TREE, q=BUF, qd=BUF, f=BUF, B=0, flags=3, qdd=BUF, scratch=BUF, stream=None),
                             nulls("q qd f qdd", "q / qd / f / qdd must not be NULL") + BATCH),
    "drm_forward_dynamics_rollout": (dict(w=TREE, q0=BUF, qd0=BUF, tau=BUF, B=0, T=1, dt=0.01, flags=3, q_traj=BUF, qd_traj=BUF, qdd_traj=BUF,
                                          scratch=BUF, stream=None), TRAJECTORY + BATCH),
    "drm_inverse_kinematics": (
        dict(w=CHAIN, q0=BUF, target_pos=BUF, target_quat=BUF, B=0, max_iters=10, damping=0.1, step=1.0, tol_pos=1e-4, tol_rot=1e-4, lower=None,
             upper=None, flags=0, q=BUF, err=BUF, iters=BUF, scratch=BUF, stream=None),
        nulls("q0 target_pos q err", "q0 / target_pos / q / err must not be NULL") + [
            (dict(target_quat=None), INVALID, "target_quat must be NULL iff DRM_IK_POSITION_ONLY"),
            (dict(flags=1), INVALID, "target_quat must be NULL iff DRM_IK_POSITION_ONLY"),
            (dict(lower=BUF), INVALID, "lower and upper must be given together"), (dict(upper=BUF), INVALID, "lower and upper must be given together"),
            (dict(max_iters=-1), INVALID, "max_iters must be >= 0"),
            (dict(damping=0.0), INVALID, "damping and step must be finite and positive"), (dict(damping=NAN), INVALID, "damping and step must be finite and positive"),
            (dict(step=0.0), INVALID, "damping and step must be finite and positive"), (dict(step=INF), INVALID, "damping and step must be finite and positive"),
            (dict(tol_pos=-1.0), INVALID, "tolerances must be finite and >= 0"), (dict(tol_rot=NAN), INVALID, "tolerances must be finite and >= 0")] + BATCH),
    "drm_operational_space": (
        dict(tree=TREE, chain=CHAIN, q=BUF, qd=BUF, B=0, flags=3, reg=0.0, inertia=BUF, jbar=BUF, bias_acc=BUF, bias_force=BUF, scratch=BUF, stream=None),
        [(dict(chain=CHAIN(n_dofs=1)), INVALID, "the two walks belong to different robots"),
         (dict(inertia=None, jbar=None, bias_acc=None, bias_force=None), INVALID, "every output is NULL"),
         (dict(q=None), INVALID, "q must not be NULL, nor qd when bias_acc / bias_force are asked for"),
         (dict(qd=None), INVALID, "q must not be NULL, nor qd when bias_acc / bias_force are asked for"),
         (dict(reg=-1.0), INVALID, "reg must be finite and >= 0"), (dict(reg=NAN), INVALID, "reg must be finite and >= 0")] + BATCH),
    "drm_forward_dynamics_derivatives": (
        dict(w=TREE, q=BUF, qd=BUF, f=BUF, B=0, flags=3, qdd=BUF, dq=BUF, dqd=BUF, minv=BUF, scratch=BUF, stream=None),
        on("w", TREE, TOO_LONG, TOO_BRANCHED) + nulls("q qd f", "q / qd / f must not be NULL")
        + nulls("qdd dq dqd minv", "qdd / dqdd_dq / dqdd_dqd / minv must not be NULL") + BATCH),
    "drm_rnea_regressor": (
        dict(w=TREE, q=BUF, qd=BUF, qdd=BUF, B=0, flags=3, Y=BUF, scratch=BUF, stream=None),
        on("w", TREE, NO_OPS, (dict(capacity=65532, n_ops=65532, n_dofs=64), UNSUPPORTED,
                               "a row of the regressor of this walk has 2^24 entries or more (65532 ops, 64 DoFs)"))
        + nulls("q qd Y", "q / qd / Y must not be NULL") + BATCH),
    "drm_lagrangian_dynamics": (
        dict(w=TREE, q=BUF, qd=BUF, B=0, flags=0, H=BUF, C=BUF, g=BUF, scratch=BUF, stream=None),
        on("w", TREE, NO_OPS) + nulls("q qd", "q / qd must not be NULL") + [(dict(H=None, C=None, g=None), INVALID, "every output is NULL")] + BATCH),
    "drm_rnea_derivatives": (
        dict(w=TREE, q=BUF, qd=BUF, qdd=BUF, B=0, flags=3, tau=BUF, dq=BUF, dqd=BUF, H=BUF, scratch=BUF, stream=None),
        on("w", TREE, NO_OPS) + nulls("q qd qdd", "q / qd / qdd must not be NULL")
        + [(dict(tau=None, dq=None, dqd=None, H=None), INVALID, "every output is NULL")] + BATCH),
    "drm_energy": (
        dict(w=TREE, q=BUF, qd=BUF, B=0, flags=0, T=BUF, V=BUF, p=BUF, dT=BUF, g=BUF, scratch=BUF, stream=None),
        on("w", TREE, NO_OPS) + nulls("q qd", "q / qd must not be NULL")
        + [(dict(T=None, V=None, p=None, dT=None, g=None), INVALID, "every output is NULL")] + BATCH),
    "drm_link_motion": (
        dict(w=TREE, q=BUF, qd=BUF, qdd=BUF, B=0, T=1, flags=0, pos=BUF, lv=BUF, av=BUF, la=BUF, aa=BUF, scratch=BUF, stream=None),
        LINK_CALL + [(dict(pos=None, lv=None, av=None, la=None, aa=None), INVALID, "every output is NULL")]),
    "drm_external_torques": (
        dict(w=TREE, q=BUF, force=BUF, torque=BUF, B=0, T=1, flags=0, tau=BUF, scratch=BUF, stream=None),
        LINK_CALL + [(dict(force=None, torque=None), INVALID, "force and torque are both NULL"), (dict(tau=None), INVALID, "tau must not be NULL")]),
    "drm_link_power_dq": (
        dict(w=TREE, q=BUF, qd=BUF, force=BUF, torque=BUF, B=0, T=1, flags=0, dq=BUF, tau=BUF, scratch=BUF, stream=None),
        LINK_CALL + [(dict(qd=None), INVALID, "qd must not be NULL"), (dict(force=None, torque=None), INVALID, "force and torque are both NULL"),
                     (dict(dq=None), INVALID, "dq must not be NULL")]),
    "drm_contact_torques": (
        dict(w=TREE, q=BUF, qd=BUF, B=0, T=1, **CONTACT_ARGS, flags=0, tau=BUF, force=BUF, moment=BUF, scratch=BUF, stream=None),
        on("w", TREE, NO_OPS) + nulls("q qd tau", "q / qd / tau must not be NULL") + [(dict(plane=None), INVALID, "drm_contact_torques needs a plane")]
        + BATCH + TARGETS + CONTACT),
    "drm_contact_torques_vjp": (
        dict(w=TREE, q=BUF, qd=BUF, grad_tau=BUF, B=0, T=1, **CONTACT_ARGS, flags=0, grad_q=BUF, grad_qd=BUF, scratch=BUF, stream=None),
        on("w", TREE, NO_OPS) + nulls("q qd grad_tau", "q / qd / grad_tau must not be NULL")
        + [(dict(grad_q=None, grad_qd=None), INVALID, "grad_q and grad_qd are both NULL")] + NO_CONTACT + BATCH + TARGETS + CONTACT),
    "drm_contact_rollout": (
        dict(dw=TREE, w=TREE, q0=BUF, qd0=BUF, tau=BUF, B=0, T=1, dt=0.01, flags=3, TL=1, **CONTACT_ARGS, q_traj=BUF, qd_traj=BUF, qdd_traj=BUF,
             scratch=BUF, stream=None),
        TRAJECTORY + NO_CONTACT + BATCH + on("w", TREE, NO_OPS) + CONTACT + [
            (dict(TL=0), INVALID, "n_targets is not the walk's number of output slots"),
            (dict(TL=4), INVALID, "n_targets is not the walk's number of output slots"),
            (dict(w=TREE(n_dofs=1)), INVALID, "the two walks are not of one robot")]),
    "drm_collision_cost": (
        dict(w=TREE, q=BUF, B=0, T=1, spheres=SPHERES, world=WORLD, pairs=PAIRS, params=PARAMS, flags=0, cost=BUF, dq=BUF, scratch=BUF, stream=None),
        COLLISION + [
            (dict(world=None, pairs=None), INVALID, "neither a world nor pairs"), (dict(params=None), INVALID, "params must not be NULL"),
            (dict(cost=None, dq=None), INVALID, "cost and dq are both NULL"),
            (dict(params=PARAMS(world_weight=-1.0)), INVALID, "the world weight must be finite and >= 0, its activation distance finite and > 0"),
            (dict(params=PARAMS(world_activation=0.0)), INVALID, "the world weight must be finite and >= 0, its activation distance finite and > 0"),
            (dict(params=PARAMS(self_weight=NAN)), INVALID, "the self weight must be finite and >= 0, its activation distance finite and > 0"),
            (dict(params=PARAMS(self_activation=INF)), INVALID, "the self weight must be finite and >= 0, its activation distance finite and > 0")]),
    "drm_sphere_distances": (
        dict(w=TREE, q=BUF, B=0, T=1, spheres=SPHERES, world=WORLD, pairs=PAIRS, flags=0, center=BUF, wd=BUF, sd=BUF, scratch=BUF, stream=None),
        COLLISION + [(dict(center=None, wd=None, sd=None), INVALID, "every output is NULL")]),
    "drm_fk_backward": (
        dict(w=TREE, q=BUF, B=0, T=1, gpos=BUF, grot=BUF, mask=0, gq=BUF, gops=None, scratch=BUF, stream=None),
        nulls("q gpos", "q / grad_pos must not be NULL") + on("w", TREE, TOO_LONG, TOO_BRANCHED) + [
            (dict(B=-1), INVALID, "negative batch or no targets"), (dict(T=0), INVALID, "negative batch or no targets"),
            (dict(T=4), INVALID, "more targets than ops in the walk"),
            (dict(gq=None), INVALID, "nothing to compute: grad_q and grad_ops_f are both NULL")] + GRAD_OPS),
    "drm_fk_jacobian_backward": (
        dict(w=CHAIN, q=BUF, B=0, gpos=BUF, grot=BUF, glin=BUF, gang=BUF, mask=0, gq=BUF, gops=None, scratch=BUF, stream=None),
        nulls("q glin gang", "q / grad_lin_jac / grad_ang_jac must not be NULL") + on("w", CHAIN, TOO_LONG) + [
            (dict(w=CHAIN(n_slots=1)), INVALID, "the walk must be the root->link chain of the Jacobian's target (no branch points)"),
            (dict(B=-1), INVALID, "negative batch or no targets"), (dict(w=CHAIN(n_ops=0)), INVALID, "more targets than ops in the walk"),
            (dict(gq=None), INVALID, "nothing to compute: grad_q and grad_ops_f are both NULL")] + GRAD_OPS),
    "drm_fk_mse": (
        dict(w=CHAIN, q=BUF, target=BUF, B=0, mask=0, loss=BUF, gq=BUF, gops=None, scratch=BUF, stream=None),
        on("w", CHAIN, TOO_LONG, TOO_BRANCHED) + nulls("q target loss scratch", "q / target / loss / scratch must not be NULL") + GRAD_OPS),
    "drm_fk_mse_links": (
        dict(w=CHAIN, sel=BUF, gsign=BUF, links=LINKS, n_links=1, q=BUF, target=BUF, B=0, mask=1, loss=BUF, gq=BUF, grad_params=BUF, scratch=BUF,
             stream=None),
        on("w", CHAIN, TOO_LONG, TOO_BRANCHED)
        + nulls("sel gsign links q target loss grad_params scratch",
                "drm_fk_mse_links: sel / gsign / links / q / target / loss / grad_params / scratch must not be NULL") + [
            (dict(n_links=0), UNSUPPORTED, "drm_fk_mse_links takes 1 .. 8 learnable links (0): compose drm_walk_table, drm_fk_mse, drm_walk_table_backward otherwise"),
            (dict(n_links=9), UNSUPPORTED, "drm_fk_mse_links takes 1 .. 8 learnable links (9)"),
            (dict(mask=0), INVALID, "param_mask must select ops of the walk (those of the learnable links)"),
            (dict(mask=1 << 4), INVALID, "param_mask must select ops of the walk (those of the learnable links)"),
            (dict(links=LINKS(rot_angles=None)), INVALID, "drm_fk_mse_links: rot_angles / trans of a link are NULL"),
            (dict(links=LINKS(trans=None)), INVALID, "drm_fk_mse_links: rot_angles / trans of a link are NULL")]),
    "drm_rnea_backward": (
        dict(w=TREE, q=BUF, qd=BUF, qdd=BUF, B=0, flags=3, gtau=BUF, mask=0, gq=BUF, gqd=BUF, gqdd=BUF, gops=None, scratch=BUF, stream=None),
        on("w", TREE, TOO_LONG, TOO_BRANCHED) + nulls("q qd gtau", "q / qd / grad_tau must not be NULL") + BATCH + GRAD_OPS + [
            (dict(gqd=None), INVALID, "grad_q, grad_qd and grad_qdd are produced together: give all three or none"),
            (dict(gq=None), INVALID, "grad_q, grad_qd and grad_qdd are produced together: give all three or none"),
            (dict(gq=None, gqd=None, gqdd=None), INVALID, "nothing to compute")]),
    "drm_link_rows": (dict(params=BUF, n_links=0, rows=BUF, stream=None),
                      nulls("params rows", "params / rows must not be NULL, n_links >= 0") + [
                          (dict(n_links=-1), INVALID, "params / rows must not be NULL, n_links >= 0")]),
    "drm_link_rows_backward": (dict(params=BUF, grad_rows=BUF, n_links=0, grad_params=BUF, stream=None),
                               nulls("params grad_rows grad_params", "params / grad_rows / grad_params must not be NULL, n_links >= 0") + [
                                   (dict(n_links=-1), INVALID, "params / grad_rows / grad_params must not be NULL, n_links >= 0")]),
    "drm_walk_table": (dict(params=BUF, n_links=1, base=BUF, sel=BUF, gsign=BUF, n_entries=1, ops_f=BUF, stream=None),
                       table_rows("drm_walk_table", "base", "ops_f")),
    "drm_walk_table_backward": (dict(params=BUF, n_links=1, grad_ops_f=BUF, sel=BUF, gsign=BUF, n_entries=1, grad_params=BUF, stream=None),
                                table_rows("drm_walk_table_backward", "grad_ops_f", "grad_params")),
    "drm_walk_table_links": (dict(links=LINKS, forms=FORMS, n_links=1, base=BUF, sel=BUF, gsign=BUF, n_entries=1, ops_f=BUF, stream=None),
                             table_links_rows("drm_walk_table_links", "base", "ops_f")),
    "drm_walk_table_links_backward": (
        dict(links=LINKS, forms=FORMS, n_links=1, grad_ops_f=BUF, sel=BUF, gsign=BUF, n_entries=1, grad_params=BUF, stream=None),
        table_links_rows("drm_walk_table_links_backward", "grad_ops_f", "grad_params")),
}


def rows_of(name):
    """the rows of an entry point: its own, and check_walk's of every walk argument"""
    baseline, rows = TABLE[name]
    rows = list(rows)
    for arg, value in baseline.items():
        if isinstance(value, Walk):
            rows += [({arg: None}, INVALID, "walk is NULL")] + on(arg, value, *WALK_FAULTS)
        elif isinstance(value, Chains):
            rows += [({arg: Chains(**change)}, code, message) for change, code, message in WALK_FAULTS]
    return rows


@pytest.fixture(scope="module")
def walks():
    model = load_model("2link_robot", device="cpu")
    tree = host_walk(model, build_walk(model._spec, whole_tree=True))
    chain = host_walk(model, build_walk(model._spec, targets=[model._name_to_idx_map["endEffector"]]))
    assert tree[0].n_ops == chain[0].n_ops == 3 and tree[0].capacity == chain[0].capacity == 4 and tree[0].n_dofs == 2, "the rows assume this"
    return {"tree": tree, "chain": chain}


class Call:
    """The ctypes arguments of one call; holds what they point to."""
    def __init__(self, walks, arguments):
        self.keep = []
        self.args = [self.value(walks, v) for v in arguments.values()]

    def changed(self, walks, kind, fields):
        w = backend.DrmWalk.from_buffer_copy(walks[kind][0])
        for k, v in fields.items():
            setattr(w, k, v)
        return w

    def value(self, walks, v):
        if v is BUF:
            self.keep.append(np.zeros(4096, np.float32))      # (a row of the 2-link robot has at most 2 x 2 floats)
            return self.keep[-1].ctypes.data
        if isinstance(v, Walk):
            self.keep.append(self.changed(walks, v.kind, v.fields))
            return ctypes.byref(self.keep[-1])
        if isinstance(v, Chains):
            self.keep.append((backend.DrmWalk * 2)(self.changed(walks, "chain", {}), self.changed(walks, "chain", v.fields)))
            return ctypes.cast(self.keep[-1], ctypes.POINTER(backend.DrmWalk))
        if isinstance(v, Struct):
            s = v.cls()
            for k, f in v.fields.items():
                setattr(s, k, f if isinstance(f, tuple) else self.value(walks, f))
            self.keep.append(s)
            return ctypes.byref(s)
        return v


def refused(lib, name, call):
    rc = getattr(lib, name)(*call.args)
    return rc, lib.drm_last_error()


@pytest.mark.parametrize("name", sorted(TABLE))
def test_both_libraries_refuse_the_same_calls_with_the_same_words(name, walks):
    host, hip = backend.load_library(kind="cpu"), backend.load_library()
    baseline, _ = TABLE[name]
    assert len(baseline) == len(getattr(host, name).argtypes), "the baseline names every argument"
    call = Call(walks, baseline)
    if name in NO_EMPTY_BATCH:
        rc, said = refused(host, name, call)
        assert rc == INVALID and NO_EMPTY_BATCH[name].encode() in said, (rc, said)
        rc, said = refused(hip, name, call)
        assert rc == UNSUPPORTED and b"7-DoF arm chains" in said, (rc, said)
    else:
        assert refused(host, name, call)[0] == 0, host.drm_last_error()
        if name not in NO_EMPTY_CALL:
            assert refused(hip, name, call)[0] == 0, hip.drm_last_error()
    for changes, code, message in rows_of(name):
        assert set(changes) <= set(baseline), changes
        call = Call(walks, dict(baseline, **changes))
        rc, said = refused(host, name, call)
        assert rc == code and message.encode() in said, (changes, rc, said)
        assert refused(hip, name, call) == (rc, said), (changes, rc, said)      # (only a call the host library refused gets here)


def test_the_table_names_every_entry_point():
    assert set(TABLE) | set(EXCLUDED) == set(backend.EXPORTS) and not set(TABLE) & set(EXCLUDED)


def test_the_table_hits_every_refusal_of_the_shared_header(walks):
    """Every message of csrc/drm_args.hpp, its conversions filled in, is the whole drm_last_error() of at least one row."""
    source = re.sub(r"//[^\n]*", "", open(HEADER).read())
    literals = {"".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)))
                for m in re.finditer(r'\bfail\(\s*DRM_ERR_\w+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', source)}
    assert len(literals) > 80, len(literals)      # (the pattern still finds them)
    host = backend.load_library(kind="cpu")
    said = {refused(host, name, Call(walks, dict(TABLE[name][0], **changes)))[1].decode() for name in TABLE for changes, _, _ in rows_of(name)}
    for literal in literals:
        # ("%s%ld": the empty string in front of a message's numbers; a "%s" alone names the entry point)
        pattern = re.escape(literal).replace("%s%ld", r"-?\d+").replace("%ld", r"-?\d+").replace("%s", r"\w+")
        assert any(re.fullmatch(pattern, text) for text in said), literal

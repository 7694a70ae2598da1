"""Drop-in ``DifferentiableRobotModel`` for the FK / Jacobian / RNEA path on MI355X.

Keeps the reference's Python method surface (reference
``differentiable_robot_model/robot_model.py:87-790``): same constructor, same
method names / argument meaning / return shapes, the ``tensor_check`` batching
rules (robot_model.py:25-84), ``AssertionError`` / ``AttributeError`` /
``KeyError`` behaviour, and the learnable-parameter mechanism
(robot_model.py:669-713).  Underneath, the reference's per-link Python loops
over tiny torch ops are replaced by:

  host (this file + flatten.py)   URDF -> RobotSpec -> depth-first walk tables, once;
  device (csrc/*.hip)             one fused hand-written HIP kernel per API call,
                                  reached through the C ABI of include/drm_hip.h.

There is NO CPU compute path: the compute methods raise if the model does not
live on a HIP device or if the native library is missing.
"""
import math
import os
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import backend
from .flatten import (OPF_DAMP, OPF_IO, OPF_MASS, OPF_MCOM, OPF_STRIDE, OPI_OUT, OPI_PERM, _PERM, RobotSpec, WalkProgram, build_robot_spec,
                      build_walk, fold_link_table, foldable_links, identity_table_row, virtual_row_constants)
from .autograd import (_FkJacobian, _FkMse, _FkMseLinks, _FkPositions, _ForwardDynamics, _InverseDynamics, _MassMatrix,  # noqa: F401
                       _ForwardDynamicsRollout, _Energy, _LinkAdjoint, _CollisionCost, _CenterOfMass, _ContactTorques, _ContactRollout,
                       _quat_grad_to_rot)
from .rigid_body import DifferentiableRigidBody, LinkPose, LinkVelocity
from .urdf_utils import URDFRobotModel

robot_description_folder = os.path.join(os.path.dirname(os.path.abspath(__file__)), "robot_data")
_WARNED_URDFS = set()      # URDF files whose "joints modelled as the URDF says" warning has been given in this process


def tensor_check(function):
    """Input normalisation shared by all public compute methods.

    Behaviour of the reference decorator of the same name (robot_model.py:25-84):
    every ``torch.Tensor`` argument must be on the model's device type, have
    ndim 1 or 2 and share one batch shape; 1-D inputs are promoted to ``[1, n]``
    and Tensor / tuple results are stripped back (dict results pass through).
    """

    @dataclass
    class BatchInfo:
        shape: torch.Size = torch.Size([])
        init: bool = False

    def preprocess(arg, obj, info):
        if type(arg) is torch.Tensor:
            assert arg.device.type == obj._device.type, f"Input argument of different device as module: {arg}"
            assert arg.ndim in [1, 2], "Input tensors must have ndim of 1 or 2."
            if info.init:
                assert info.shape == arg.shape[:-1], "Batch size mismatch between input tensors."
            else:
                info.init = True
                info.shape = arg.shape[:-1]
            if len(info.shape) == 0:
                return arg.unsqueeze(0)
        return arg

    def postprocess(arg, info):
        if type(arg) is torch.Tensor and info.init and len(info.shape) == 0:
            return arg[0, ...]
        return arg

    def wrapper(self, *args, **kwargs):
        info = BatchInfo()
        p_args = [preprocess(a, self, info) for a in args]
        if kwargs:
            kwargs = {k: preprocess(v, self, info) for k, v in kwargs.items()}
        ret = function(self, *p_args, **kwargs)
        if not (info.init and len(info.shape) == 0):     # batched inputs: results pass through as they are
            return ret
        if type(ret) is torch.Tensor:
            return postprocess(ret, info)
        if type(ret) is tuple:
            return tuple(postprocess(r, info) for r in ret)
        return ret

    wrapper.__name__ = getattr(function, "__name__", "wrapper")
    wrapper.__doc__ = function.__doc__
    return wrapper


@dataclass
class _DeviceWalk:
    program: WalkProgram
    ops_i: torch.Tensor                 # int32 [8, cap] (field-major) on the model device
    gather: torch.Tensor                # int64 [cap * 32] flat indices into the [L+1, 32] link table
    gsign: torch.Tensor                 # float32 [cap * 32] +-1 factors of the gathered entries
    static_ops_f: Optional[torch.Tensor] = None
    folded: bool = False                # a dynamics walk without the foldable links, on the folded link table
    fold_key: Optional[tuple] = None    # ... folded for this set of kept (learnable) links (robot_model._fold_mask)
    learnable_plan: Optional[tuple] = None   # (learnable links, constant walk table, row selector) of _ops_f_learnable


@dataclass
class InverseKinematicsResult:
    """What DifferentiableRobotModel.compute_inverse_kinematics returns (no autograd history on any field)."""
    q: torch.Tensor                     # [B, n] the joint angles where each row stopped
    pos_err: torch.Tensor               # [B] |target_pos - p| at q
    rot_err: Optional[torch.Tensor]     # [B] rotation angle between the target and the link's orientation at q; None: position only
    iterations: torch.Tensor            # [B] int32: the updates applied
    converged: torch.Tensor             # [B] bool: the errors are within the tolerances


class OperationalSpaceDynamics(NamedTuple):
    """What DifferentiableRobotModel.compute_operational_space_dynamics returns (no autograd history on any field); m = 6, or 3 in
    position-only mode."""
    inertia: torch.Tensor               # [B, m, m] (J H^-1 J^T + regularization^2 I)^-1
    jacobian_pinv: torch.Tensor         # [B, n, m] H^-1 J^T inertia
    bias_acc: torch.Tensor              # [B, m] Jdot qd
    bias_force: torch.Tensor            # [B, m] inertia (J H^-1 nle - Jdot qd)


class ForwardDynamicsDerivatives(NamedTuple):
    """What DifferentiableRobotModel.compute_forward_dynamics_derivatives returns (no autograd history on any field)."""
    qdd: torch.Tensor                   # [B, n] = compute_forward_dynamics(q, qd, f, ...)
    dqdd_dq: torch.Tensor               # [B, n, n] [b, i, j] = d qdd_i / d q_j
    dqdd_dqd: torch.Tensor              # [B, n, n] [b, i, j] = d qdd_i / d qd_j (with use_damping it includes -H^-1 diag(damping))
    minv: torch.Tensor                  # [B, n, n] H(q)^-1 = d qdd / d f, symmetric


class LagrangianDynamics(NamedTuple):
    """What DifferentiableRobotModel.compute_lagrangian_dynamics returns (no autograd history on any field): the terms of
    H(q) qdd + C(q, qd) qd + g(q) = tau."""
    inertia: torch.Tensor               # [B, n, n] H(q) = compute_lagrangian_inertia_matrix(q)
    coriolis: torch.Tensor              # [B, n, n] the Christoffel matrix C(q, qd): dH/dt = C + C^T
    gravity: torch.Tensor               # [B, n] g(q) = compute_inverse_dynamics(q, 0, 0, include_gravity=True, use_damping=False)


class InverseDynamicsDerivatives(NamedTuple):
    """What DifferentiableRobotModel.compute_inverse_dynamics_derivatives returns (no autograd history on any field);
    [b, i, j] = d tau_i / d x_j."""
    tau: torch.Tensor                   # [B, n] = compute_inverse_dynamics(q, qd, qdd, ...)
    dtau_dq: torch.Tensor               # [B, n, n] (damping never enters it)
    dtau_dqd: torch.Tensor              # [B, n, n] (with use_damping it includes diag(damping); gravity never enters it)
    dtau_dqdd: torch.Tensor             # [B, n, n] H(q), symmetric to the bit


class EnergyDerivatives(NamedTuple):
    """What DifferentiableRobotModel.compute_energy_derivatives returns (no autograd history on any field)."""
    kinetic: torch.Tensor               # [B] T = 1/2 qd^T H(q) qd
    potential: torch.Tensor             # [B] V = 9.81 sum_i m_i z_i over the bodies a joint moves
    momentum: torch.Tensor              # [B, n] p = dT/dqd = H(q) qd
    dkinetic_dq: torch.Tensor           # [B, n] dT/dq = C(q, qd)^T qd
    gravity: torch.Tensor               # [B, n] dV/dq = g(q)


class Energy(NamedTuple):
    """What DifferentiableRobotModel.compute_energy returns: differentiable once with respect to q and qd."""
    kinetic: torch.Tensor               # [B]
    potential: torch.Tensor             # [B]


class CenterOfMass(NamedTuple):
    """What DifferentiableRobotModel.compute_center_of_mass returns: base axes; ``position`` is differentiable once in q and
    ``velocity`` once in qd, every other field carries no autograd history."""
    mass: object                                # M: a Python float; a detached 0-dim tensor for a model with learnable links
    position: torch.Tensor                      # [B, 3] sum m_i c_i / M
    velocity: Optional[torch.Tensor]            # [B, 3] jacobian qd; None when qd is None
    acceleration: Optional[torch.Tensor]        # [B, 3] d/dt velocity (gravity not included); None when qdd is None
    jacobian: Optional[torch.Tensor]            # [B, 3, n]; None unless asked for
    angular_momentum: Optional[torch.Tensor]    # [B, 3] about the base ORIGIN; None when qd is None


class BaseWrench(NamedTuple):
    """What DifferentiableRobotModel.compute_base_wrench returns (no autograd history on either field): the wrench the mount applies to
    the base link, at the base origin in base axes."""
    force: torch.Tensor                         # [B, 3]
    moment: torch.Tensor                        # [B, 3]


class LinkMotion(NamedTuple):
    """What DifferentiableRobotModel.compute_link_motion returns (no autograd history on any field): world axes, at the link origins."""
    position: torch.Tensor                          # [B, L, 3] the link origins
    linear_velocity: torch.Tensor                   # [B, L, 3] lin_jac_l qd
    angular_velocity: torch.Tensor                  # [B, L, 3] ang_jac_l qd
    linear_acceleration: Optional[torch.Tensor]     # [B, L, 3] d/dt linear_velocity (gravity not included); None when qdd is None
    angular_acceleration: Optional[torch.Tensor]    # [B, L, 3] d/dt angular_velocity; None when qdd is None


class PlaneContact:
    """Penalty contact of spheres on the links with the plane {x : normal . x = offset} (csrc/drm_contact.hpp): a spring-damper along
    the normal that never pulls, f_n = max(0, stiffness depth - damping v_n) while depth > 0, and regularised Coulomb friction
    f_t = -min(friction_slope, friction f_n / |v_t|) v_t (viscous with slope ``friction_slope``, capped at ``friction`` f_n).
    ``normal`` is normalised in float64.  ``radius``: one float for every link, or one value per entry of the call's ``link_names``;
    the sphere is centred at the link origin and its lowest point is the contact point."""

    def __init__(self, normal=(0.0, 0.0, 1.0), offset=0.0, *, stiffness, damping, friction=0.0, friction_slope=0.0, radius=0.0):
        n = [float(x) for x in normal]
        if len(n) != 3 or not all(math.isfinite(x) for x in n):
            raise ValueError("normal must be three finite numbers (got %r)" % (normal,))
        length = math.sqrt(sum(x * x for x in n))
        if not length > 0.0:
            raise ValueError("normal must not be zero")
        self.normal = tuple(x / length for x in n)
        self.offset = float(offset)
        if not math.isfinite(self.offset):
            raise ValueError("offset must be finite (got %r)" % (offset,))
        for name, v in (("stiffness", stiffness), ("damping", damping), ("friction", friction), ("friction_slope", friction_slope)):
            v = float(v)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError("%s must be finite and >= 0 (got %r)" % (name, v))
            setattr(self, name, v)
        radii = [float(radius)] if isinstance(radius, (int, float)) else [float(r) for r in radius]
        if not all(math.isfinite(r) and r >= 0.0 for r in radii):
            raise ValueError("radius must be finite and >= 0 (got %r)" % (radius,))
        self.radius = radii[0] if isinstance(radius, (int, float)) else tuple(radii)

    def _plane(self):
        return (self.normal, self.offset, self.stiffness, self.damping, self.friction, self.friction_slope)


class JointLimitSprings:
    """Spring-dampers at the joint limits (get_joint_limits(); a continuous joint is free): below the lower bound
    tau = stiffness (lower - q) - damping qd, above the upper bound tau = -stiffness (q - upper) - damping qd, zero in between."""

    def __init__(self, stiffness, damping=0.0):
        self.stiffness, self.damping = float(stiffness), float(damping)
        for name in ("stiffness", "damping"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError("%s must be finite and >= 0 (got %r)" % (name, v))


class ContactTorques(NamedTuple):
    """What DifferentiableRobotModel.compute_contact_torques returns (no autograd history): world axes, at the link origins."""
    tau: torch.Tensor                   # [B, n] sum_l lin_jac_l^T force_l + ang_jac_l^T moment_l, plus the joint-limit springs
    force: torch.Tensor                 # [B, L, 3] the plane's force on each named link
    moment: torch.Tensor                # [B, L, 3] its moment about the link origin


class ContactRollout(NamedTuple):
    """What DifferentiableRobotModel.compute_contact_rollout returns (no autograd history)."""
    q: torch.Tensor                     # [T, B, n] the positions after steps 1 .. T
    qd: torch.Tensor                    # [T, B, n] the velocities after steps 1 .. T
    qdd: Optional[torch.Tensor]         # [T, B, n] the acceleration OF step t (at the state before it); None unless asked for


def _float_array(x, shape, name):
    """``x`` as a float32 numpy array of ``shape`` (-1: any length), finite"""
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    if a.ndim != len(shape) or any(want >= 0 and got != want for got, want in zip(a.shape, shape)):
        raise ValueError("%s must have shape %s (got %s)" % (name, list(shape), list(a.shape)))
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % name)
    return a


class CollisionSpheres:
    """The robot as spheres fixed to its links: sphere s sits on link ``link_names[s]`` with centre ``centers[s]`` in that link's own
    URDF frame (the frame whose pose compute_forward_kinematics returns) and radius ``radii[s]`` >= 0.  Any order, any number per link;
    spheres on the root are allowed (they never move: a constant of the cost, but they take part in self pairs)."""

    def __init__(self, link_names, centers, radii):
        self.link_names = [str(n) for n in link_names]
        self.centers = _float_array(centers, (len(self.link_names), 3), "centers")
        self.radii = _float_array(radii, (len(self.link_names),), "radii")
        if not self.link_names:
            raise ValueError("at least one sphere")
        if (self.radii < 0).any():
            raise ValueError("radii must be >= 0")


class CollisionWorld:
    """The obstacles, shared by every row of a batch: ``spheres`` [Ms, 4] = centre and radius; boxes with centres ``box_centers``
    [Mb, 3], half extents ``box_half_extents`` [Mb, 3] >= 0 and rotations ``box_rotations`` [Mb, 3, 3] from box to world axes
    (None: axis-aligned).  Either kind may be absent."""

    def __init__(self, spheres=None, box_centers=None, box_half_extents=None, box_rotations=None):
        self.spheres = _float_array(spheres, (-1, 4), "spheres") if spheres is not None else np.zeros((0, 4), np.float32)
        if (self.spheres[:, 3] < 0).any():
            raise ValueError("sphere radii must be >= 0")
        if (box_centers is None) != (box_half_extents is None):
            raise ValueError("boxes need box_centers and box_half_extents")
        if box_centers is None:
            if box_rotations is not None:
                raise ValueError("box_rotations without boxes")
            self.boxes = np.zeros((0, 16), np.float32)
        else:
            c = _float_array(box_centers, (-1, 3), "box_centers")
            h = _float_array(box_half_extents, (len(c), 3), "box_half_extents")
            if (h < 0).any():
                raise ValueError("box_half_extents must be >= 0")
            R = np.tile(np.eye(3, dtype=np.float32), (len(c), 1, 1)) if box_rotations is None else \
                _float_array(box_rotations, (len(c), 3, 3), "box_rotations")
            self.boxes = np.concatenate([c, h, R.reshape(len(c), 9), np.zeros((len(c), 1), np.float32)], axis=1).astype(np.float32)

    @property
    def n_obstacles(self):
        return len(self.spheres) + len(self.boxes)


class CollisionGeometry:
    """What DifferentiableRobotModel.make_collision_geometry returns: the device tables of one sphere set, its self pairs and one
    world (csrc/drm_collision.hpp), built once.  ``with_world`` swaps the obstacles and shares everything else."""

    def __init__(self, model, walk_names, spheres, start, order, pairs, world_spheres, world_boxes):
        self._model = model
        self._walk_names = walk_names          # what _links_plan takes: the links of the walk
        self.spheres, self.start = spheres, start      # [S, 4] float32 grouped by link, [T + 2] int32
        self.order = order                     # [S] int64: grouped position of the caller's sphere s; None: the caller's order is grouped
        self.pairs = pairs                     # [P, 2] int32 in grouped indices, or None
        self.world_spheres, self.world_boxes = world_spheres, world_boxes      # [Ms, 4], [Mb, 16] or None

    @property
    def n_spheres(self):
        return int(self.spheres.shape[0])

    @property
    def n_pairs(self):
        return 0 if self.pairs is None else int(self.pairs.shape[0])

    @property
    def has_world(self):
        return self.world_spheres is not None or self.world_boxes is not None

    def tables(self):
        return (self.spheres, self.start, self.world_spheres, self.world_boxes, self.pairs)

    def with_world(self, world):
        """The same spheres and pairs against another CollisionWorld (None: no obstacles)."""
        ws, wb = self._model._collision_world_tables(world)
        return CollisionGeometry(self._model, self._walk_names, self.spheres, self.start, self.order, self.pairs, ws, wb)


class CollisionCost(NamedTuple):
    """What DifferentiableRobotModel.compute_collision_cost returns."""
    cost: torch.Tensor                  # [B] differentiable once with respect to q
    dcost_dq: torch.Tensor              # [B, n] its gradient, from the same launch (no autograd history)


class SphereDistances(NamedTuple):
    """What DifferentiableRobotModel.compute_sphere_distances returns (no autograd history), in the caller's sphere order."""
    center: torch.Tensor                # [B, S, 3] world centres
    world_distance: torch.Tensor        # [B, S] least clearance to an obstacle (+inf without a world); < 0: penetration
    self_distance: torch.Tensor         # [B, S] least clearance over the pairs the sphere is in (+inf without one)


class DifferentiableRobotModel(torch.nn.Module):
    """Batched FK / geometric Jacobian / RNEA on MI355X behind the reference API."""

    def __init__(self, urdf_path: str, name="", device=None, reference_compat: bool = True):
        """Same signature and defaults as the reference's constructor (robot_model.py:94-104): ``device=None`` is the CPU, and
        every non-fixed joint is an axis-aligned revolute joint (robot_model.py:122-126, rigid_body.py:149-154), so a model
        built the reference's way returns the reference's numbers for every URDF the reference accepts.
        ``reference_compat=False`` opts into what the URDF says instead: prismatic joints slide and joints turn about their
        true (possibly skew) axis."""
        super().__init__()
        self.name = name
        self._reference_compat = bool(reference_compat)
        if device is None:
            device = "cpu"      # robot_model.py:100-104 (pass device="cuda" for the HIP kernels; nothing falls back either way)
        self._device = torch.device(device)
        if self._device.type == "cuda" and self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())

        self._urdf_model = URDFRobotModel(urdf_path=urdf_path, device=self._device)
        self._bodies = torch.nn.ModuleList()
        self._n_dofs = 0
        self._controlled_joints = []
        self._name_to_idx_map = dict()

        body_params, parent_names = [], []
        # the joint is folded into its child link, as in the reference (robot_model.py:107-131)
        for i, link in enumerate(self._urdf_model.robot.links):
            params = self._urdf_model.get_body_parameters_from_urdf(i, link)
            body = DifferentiableRigidBody(rigid_body_params=params, device=self._device)
            if params["joint_type"] != "fixed":
                body.joint_idx = self._n_dofs
                self._n_dofs += 1
                self._controlled_joints.append(i)
            self._bodies.append(body)
            self._name_to_idx_map[body.name] = i
            body_params.append(params)
            parent_names.append(None if i == 0 else self._urdf_model.get_name_of_parent_body(link.name))
        for i, body in enumerate(self._bodies):
            body._attach(self, i)
            if i == 0:
                continue
            parent = self._bodies[self._name_to_idx_map[parent_names[i]]]
            body.set_parent(parent)
            parent.add_child(body)
        self._zero1 = torch.zeros(1, device=self._device)
        self._table_links = os.environ.get("DRM_TABLE_LINKS", "1") != "0"        # (0: the table of a learnable model through a cat of the modules' outputs + drm_walk_table; A/B switch)
        self._source_plan = None
        self._learnable_version = 0                 # counts make_link_param_learnable: what is cached per set of learnable parameters looks at it
        self._fk_mse_links = os.environ.get("DRM_FK_MSE_LINKS", "1") != "0"      # (0: fk_mse_loss composes WalkTable + drm_fk_mse; A/B switch)
        self._kin_state = None   # (q, qd) of the last update_kinematic_state
        self._kin_cache = {}

        self._spec: RobotSpec = build_robot_spec(body_params, parent_names, reference_compat=self._reference_compat)
        if self._reference_compat:
            # the reference's joint model is the default; tell a user whose URDF has a sliding joint what that means (once per
            # URDF file and process: models are built in loops and on every rank), pointing at the USER's call
            sliding = [b.name for i, b in enumerate(self._bodies) if body_params[i]["joint_type"] == "prismatic"]
            if sliding and os.path.abspath(urdf_path) not in _WARNED_URDFS:
                _WARNED_URDFS.add(os.path.abspath(urdf_path))
                import warnings
                warnings.warn(
                    "%s: prismatic joint(s) of %s modelled as REVOLUTE joints, as the reference does (robot_model.py:122-126) "
                    "— upstream's numbers, not the mechanism's.  Pass reference_compat=False for joints that slide (and for "
                    "joint axes that are not +-x / y / z)." % (os.path.basename(urdf_path), ", ".join(sliding)),
                    stacklevel=2 if type(self) is DifferentiableRobotModel else 3)
        self._learnable = set()          # {(link_idx, parameter_name)}
        self._walks: Dict[tuple, _DeviceWalk] = {}
        self._chain_walks: Dict[int, _DeviceWalk] = {}          # link index -> _chain_walk's answer while nothing is learnable
        self._dyn_walk: Optional[_DeviceWalk] = None            # _dynamics_walk's answer while nothing is learnable
        self._fanout_plans: Dict[tuple, Optional[list]] = {}
        self._fan_handles: Dict[tuple, int] = {}               # fan-out plan key -> the constant-folded kernel of THAT ordered set
        # prepared eager calls of a constant model (csrc/drm_hostcall.cpp FastCall): link name -> (call, walk program, its struct cache)
        self._fast_fk: Dict[str, tuple] = {}
        self._fast_jac: Dict[str, tuple] = {}
        self._fast_id: Optional[tuple] = None
        self._fast_crba: Optional[tuple] = None
        self._fast_fd: Optional[tuple] = None
        self._fast_fkid: Dict[str, tuple] = {}                  # link name -> (call, dynamics walk program, its cache, chain program, its cache)
        self._stream_arg = (lambda: 0) if self._device.type != "cuda" or backend._raw_stream is None else \
            (lambda raw=backend._raw_stream, i=self._device.index: raw(i))
        self._own_kernels: Optional[str] = None                 # None: DRM_SPECIALIZE decides (default "auto"); "off" / "auto" / "build"
        self._static_table: Optional[torch.Tensor] = None      # snapshot of all rows (constants)
        self._static_folded: Dict[tuple, torch.Tensor] = {}    # ... with the links of a fold mask folded into their parents
        self._fold_masks: Dict[tuple, np.ndarray] = {}          # kept (learnable) links -> foldable_links(spec, keep)
        self._root_pose = None                                  # the root link's identity (pos [1,3], quat [1,4]), made on first use
        self._learnable_links: Optional[torch.Tensor] = None   # link indices whose rows are rebuilt per call

    # ------------------------------------------------------------------ copies
    # copy.deepcopy(model) works as it does for the reference's plain nn.Module (a ground-truth copy, a target network): parameters,
    # constants and the set of learnable parameters are copied; everything DERIVED — walks with their launch structs and kernel handles,
    # prepared calls, the source plan of the learnable links — is left behind and rebuilt by the copy on first use.
    _DERIVED = {"_walks": dict, "_chain_walks": dict, "_dyn_walk": lambda: None, "_fanout_plans": dict, "_fan_handles": dict,
                "_fast_fk": dict, "_fast_jac": dict, "_fast_id": lambda: None, "_fast_crba": lambda: None, "_fast_fd": lambda: None,
                "_fast_fkid": dict, "_source_plan": lambda: None, "_kin_cache": dict, "_kin_state": lambda: None,
                "_stream_arg": lambda: None, "_arm_specialized": lambda: False}
    _DERIVED_LAZY = ("_learnable_sorted", "_skew_any", "_dyn_walk_learnable", "_body_names", "_all_link_idxs", "_fast_links", "_fk_links_plans",
                     "_ik_bounds")

    def __getstate__(self):
        state = self.__dict__.copy()
        for name, make in self._DERIVED.items():
            if name in state:
                state[name] = make()
        for name in self._DERIVED_LAZY:
            state.pop(name, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._stream_arg = (lambda: 0) if self._device.type != "cuda" or backend._raw_stream is None else \
            (lambda raw=backend._raw_stream, i=self._device.index: raw(i))
        self._learnable_version = self.__dict__.get("_learnable_version", 0) + 1
        for i, body in enumerate(self._bodies):
            body._attach(self, i)       # (a body's pose / vel ask ITS model)

    # ------------------------------------------------------------------ constants
    def _link_rows(self, link_idxs, device=None) -> torch.Tensor:
        """[len(link_idxs), OPF_STRIDE] float32 rows of per-link constants on the model device.

        Built with torch ops from the bodies' parameter callables, so gradients reach learnable
        parametrisations.  The arithmetic mirrors the reference:
        R_fixed = (Rz(yaw) @ Ry(pitch)) @ Rx(roll)  (rigid_body.py:138-143, spatial_vector_algebra.py:14-53),
        mcom = com * mass, I_o = I_c + mass * S(com) S(com)^T  (spatial_vector_algebra.py:321-327).
        """
        dev = self._device if device is None else device
        rows = backend.link_rows_torch(self._link_params(link_idxs, device=dev).to(torch.float32))
        if OPF_STRIDE != rows.shape[1]:
            rows = torch.cat([rows, torch.zeros(rows.shape[0], OPF_STRIDE - rows.shape[1], device=dev)], dim=1)
        return rows.to(torch.float32)

    def _link_table(self, fold_key: Optional[tuple] = None) -> torch.Tensor:
        """[L + 1, OPF_STRIDE] table of per-link constants (row L = the identity op used to pad walks); ``fold_key``: with
        the links of that fold mask folded into their parents (_dynamics_walk).

        With learnable parameters only the rows of the links that carry them are rebuilt (differentiably) on
        top of a cached snapshot of the constant rows: the per-step host work is O(#learnable links), not O(L).
        """
        if self._static_table is None:
            with torch.no_grad():
                # the constant snapshot is computed on the HOST whatever the model's device (round 5): R_fixed = Rz Ry Rx through the
                # host's cos / sin is the reference's own CPU result bit for bit (a device's differ in the last bit for general
                # angles), the table — and with it the key of a robot's own kernels, specialize.build — is the same on every machine
                ident = torch.from_numpy(identity_table_row()).reshape(1, OPF_STRIDE)
                base = torch.cat([self._link_rows(range(len(self._bodies)), device=torch.device("cpu")), ident], dim=0)
                self._static_table = self._with_virtual_rows(base).to(self._device)
        if not self._learnable:
            return self._static_table if fold_key is None else self._with_virtual_rows(self._static_rows(fold_key))
        links = sorted({link for link, _ in self._learnable})
        if self._learnable_links is None or self._learnable_links.numel() != len(links):
            self._learnable_links = torch.tensor(links, dtype=torch.int64, device=self._device)
        if self._device.type == "cuda":
            # the rows of the learnable links through the fused parameter kernels (backend.LinkRows)
            rows = backend.LinkRows.apply(self._link_params(links))
        else:
            rows = self._link_rows(links)   # host-side tests of the table construction
        return self._with_virtual_rows(self._static_rows(fold_key).index_copy(0, self._learnable_links, rows))

    def _with_virtual_rows(self, base: torch.Tensor) -> torch.Tensor:
        """Append the two virtual rows of every link whose joint axis is not +-x / y / z (flatten.build_walk):
        A = (F R_a, t, massless, damping) — the joint itself, turning about +z — and B = (R_a^T, 0, mass, mcom, I_o, 0),
        the fixed step back into the link's own frame.  Differentiable in the link's row (torch ops)."""
        links, Ra = virtual_row_constants(self._spec)
        if not links:
            return base
        Ra_t = torch.from_numpy(np.ascontiguousarray(Ra)).to(base.device)
        rows = base[torch.tensor(links, device=base.device)]
        S = len(links)
        zeros = lambda k: torch.zeros(S, k, device=base.device)
        FA = (rows[:, 0:9].reshape(S, 3, 3) @ Ra_t).reshape(S, 9)
        row_a = torch.cat([FA, rows[:, 9:12], zeros(13), rows[:, 25:26], zeros(OPF_STRIDE - 26)], dim=1)
        row_b = torch.cat([Ra_t.transpose(1, 2).reshape(S, 9), zeros(3), rows[:, 12:25], zeros(OPF_STRIDE - 25)], dim=1)
        return torch.cat([base, torch.stack([row_a, row_b], dim=1).reshape(2 * S, OPF_STRIDE)], dim=0)

    def _link_params(self, link_idxs, device=None) -> torch.Tensor:
        """[len(link_idxs), 20] rpy, trans, mass, com, inertia_mat, damping of the given links (include/drm_hip.h
        drm_link_rows), read from the bodies' parameter callables so that gradients reach learnable modules."""
        dev = self._device if device is None else device
        zero1 = torch.zeros(1, device=dev)
        rows = []
        for i in link_idxs:
            b = self._bodies[i]
            damping = b.joint_damping()
            rows.append(torch.cat([t.reshape(-1).to(dev) for t in (
                b.rot_angles(), b.trans(), b.inertia.mass(), b.inertia.com(), b.inertia.inertia_mat(),
                damping if damping is not None else zero1)]))
        return torch.stack(rows)

    def _get_walk(self, key, targets=None, whole_tree=False, folded=False, fold_key=None) -> _DeviceWalk:
        dw = self._walks.get(key)
        if dw is None:
            prog = build_walk(self._spec, targets=targets, whole_tree=whole_tree, drop_folded=folded and whole_tree,
                              fold=self._fold_masks[fold_key] if folded else None)
            dw = _DeviceWalk(
                program=prog,
                ops_i=torch.from_numpy(prog.ops_i_dev).to(self._device).contiguous(),
                gather=torch.from_numpy(prog.gather.reshape(-1)).to(self._device),
                gsign=torch.from_numpy(prog.gsign.reshape(-1)).to(self._device),
                folded=folded, fold_key=fold_key if folded else None,
            )
            self._walks[key] = dw
        return dw

    def _own_kernel_mode(self) -> str:
        """How this model comes by its OWN kernels (its constants / its tree folded into the instruction stream, specialize.py):

          "auto"   (default, round 6) a code object that is ALREADY built — shipped next to the library (csrc/special_cache/, the
                   robots of the package), or in the run-time cache of an earlier `specialize()` — is attached on first use; nothing
                   is ever compiled on a call path, and a miss keeps the library's kernels (logged once per robot at INFO);
          "build"  compile what is missing with hipcc (2-7 s per kernel, cached): `model.specialize()`, `model.own_kernels = "build"`,
                   DRM_SPECIALIZE=1 (or =tune) in the environment;
          "off"    the library's kernels only: `model.own_kernels = "off"` or DRM_SPECIALIZE=0.
        Either way the results are the same to a few ulp (tests/test_specialize.py runs both)."""
        if self._own_kernels is not None:
            return self._own_kernels
        env = os.environ.get("DRM_SPECIALIZE")
        if env == "0":
            return "off"
        if env in ("1", "tune") or getattr(self, "_arm_specialized", False):
            return "build"
        return "auto"

    @property
    def own_kernels(self) -> Optional[str]:
        """None (DRM_SPECIALIZE decides; "auto" when unset), "off", "auto" or "build" — see _own_kernel_mode."""
        return self._own_kernels

    @own_kernels.setter
    def own_kernels(self, mode: Optional[str]) -> None:
        if mode not in (None, "off", "auto", "build"):
            raise ValueError('own_kernels must be None, "off", "auto" or "build"')
        self._own_kernels = mode
        # whatever was attached under the previous setting goes: the next call looks again under the new one
        for dw in list(self._walks.values()) + [w for plan in self._fanout_plans.values() if plan for w in plan]:
            prog = dw.program
            prog._special, prog._special_const, prog._special_tried, prog._ws_cache = {}, False, False, None
            prog._arm_special_failed = False
            prog.__dict__.pop("_fan_cache", None)
        self._fan_handles.clear()
        self._dyn_walk = None
        self.__dict__.pop("_own_kernel_missed", None)
        if mode in (None, "auto", "build"):
            for key, plan in self._fanout_plans.items():
                if plan:
                    self._fan_special(key, plan)

    def _own_kernel_miss(self, what: str, err: Exception) -> None:
        """One INFO line per model and kind of kernel when the default (`auto`) finds nothing built."""
        seen = self.__dict__.setdefault("_own_kernel_missed", set())
        if what not in seen:
            seen.add(what)
            import logging
            logging.getLogger("differentiable_robot_model_amd").info(
                "%s: no pre-built own kernel for %s (%s); the library's kernels serve it — model.specialize() builds one",
                self.name or "robot", what, str(err)[:160])

    def specialize(self, force: bool = False, tune: bool = False):
        """Build (hipcc, 3-7 s, cached) and attach this robot's OWN straight-line dynamics kernels — inverse dynamics and its
        reverse mode, the inertia matrix, forward dynamics (specialize.py, csrc/drm_static.hpp): for robots whose tree is none of the
        shapes the library ships straight-line kernels for (a mobile manipulator such as Fetch) the loop-structured kernels stop being
        the only choice (Fetch at 2^20 rows: 233 -> 70 us, 982 -> 206 us, 655 -> 170 us, 615 -> 150 us — round 5: a CONSTANT model's
        kernels also carry its walk table as compile-time constants, so products with the robot's zeros and ones are gone).  DRM_SPECIALIZE=1 in the environment does it on first use.  Returns True when a kernel was
        attached, False when the robot already runs a compiled straight-line kernel (7-DoF arms, arm + hand, hands).  Models with
        learnable link parameters specialise their full walk as well (the kernel reads the same table).  `force`: build the
        robot's own kernels even when the library has a straight-line kernel for its shape (measurements, tools/probe_special.py).
        `tune`: build them for ANY robot that is not a plain 7-DoF arm, time every entry point both ways on this device and keep the
        faster of the two per entry point (specialize.tune; returns its report): the library's kernels for "an arm that carries a
        hand" are generic in (P, K, L), a small robot's own walk can beat them (Panda with gripper: inertia matrix 133 -> 86 us,
        forward dynamics 167 -> 125, inverse dynamics 70 -> 58, its reverse mode 197 -> 149 at 2^20 rows)."""
        from . import specialize as sp
        if self._device.type != "cuda":
            raise RuntimeError("per-robot kernels are HIP code objects: the model must live on a HIP device (it is on %s)" % self._device)
        dw = self._dynamics_walk()
        from .flatten import SHAPE_ARM_CHAIN, SHAPE_ARM_HAND, SHAPE_FINGERS
        if not self._learnable:
            # constant models: the kernels that bake the robot's CONSTANTS (round 5) are built where they are first needed — the fused
            # FK + RNEA kernel of an arm's target link, the fan-out FK kernel of a set of fingertips (compute_forward_kinematics_links)
            self._arm_specialized = True
            for key, plan in self._fanout_plans.items():
                if plan:
                    self._fan_special(key, plan)
        if tune:
            if dw.program.shape & SHAPE_ARM_CHAIN or dw.program.n_ops > sp.MAX_STATIC_OPS:
                return {}
            dw.program._special = {k: h for k, h in (getattr(dw.program, "_special", None) or {}).items() if k not in sp.KERNELS}
            sp.attach(dw.program, self._spec, self._n_dofs, self._const_table(dw), ignore_tuned=True)
            return sp.tune(dw.program, self._ops_f(dw).detach(), dw.ops_i, self._n_dofs)      # (remembered: specialize.tuned_kinds)
        if not force and sp.arm_qualifies(dw.program, self._n_dofs):
            # a serial 7-DoF arm (Panda, iiwa): its OWN kernels too, of a different kind — the library's streaming walk with this
            # robot's constants folded into the instruction stream (specialize.attach_arm, csrc/drm_arm_stream.hpp).  Inverse
            # dynamics now; the fused FK + RNEA kernel of a target link when plan_fk_and_inverse_dynamics /
            # compute_fk_and_inverse_dynamics first meets it.  Constant models only (the kernels do not read the table).
            if self._learnable:      # the reverse-mode kernel of this set of learnable blocks (the constant blocks folded in)
                kin, dyn = self._learnable_block_masks(dw)
                sp.attach_arm_param(dw.program, self._ops_f(dw).detach().cpu().numpy(), self._n_dofs, kin, dyn)
                return True
            self._arm_specialized = True
            sp.attach_arm(dw.program, self._ops_f(dw).detach().cpu().numpy(), self._n_dofs)
            return True
        if not force and dw.program.shape & (SHAPE_ARM_CHAIN | SHAPE_ARM_HAND | SHAPE_FINGERS):
            return False
        sp.attach(dw.program, self._spec, self._n_dofs, self._const_table(dw))
        return True

    def _const_table(self, dw: "_DeviceWalk"):
        """The walk's table as a host array for kernels that carry it as compile-time constants (round 5) — None for a model with
        learnable parameters (its kernels keep reading the table: it changes every step)."""
        if self._learnable:
            return None
        return self._ops_f(dw).detach().cpu().numpy()

    def _arm_fused_special(self, tree: "_DeviceWalk", chain: "_DeviceWalk") -> None:
        """After specialize() (or under DRM_SPECIALIZE=1) on a serial 7-DoF arm: build and attach, once per target chain, the
        constant-folded fused FK + RNEA kernel of this (dynamics walk, chain walk) pair."""
        if self._learnable or self._device.type != "cuda":
            return
        mode = self._own_kernel_mode()
        if mode == "off":
            return
        from . import specialize as sp
        have = (getattr(tree.program, "_special", None) or {}).get(sp.SPECIAL_FK_RNEA_ARM)
        if have is not None and have == (getattr(chain.program, "_special", None) or {}).get(sp.SPECIAL_FK_RNEA_ARM):
            return
        if getattr(chain.program, "_arm_special_failed", False):
            return
        if not (sp.arm_qualifies(tree.program, self._n_dofs) and sp.arm_qualifies(chain.program, self._n_dofs) and chain.program.n_ops == 8):
            return
        try:
            sp.attach_arm(tree.program, self._ops_f(tree).detach().cpu().numpy(), self._n_dofs,
                          chain.program, self._ops_f(chain).detach().cpu().numpy(), cached_only=mode == "auto")
            if (tree.program._special or {}).get(sp.SPECIAL_FK_RNEA_ARM) is None:      # (auto: not built yet)
                chain.program._arm_special_failed = True
                self._own_kernel_miss("the fused FK + inverse-dynamics launch", sp.CacheMiss("; ".join(tree.program._special_missed)))
        except sp.SpecializeError:
            if getattr(self, "_arm_specialized", False):
                raise
            chain.program._arm_special_failed = True      # (environment opt-in on a machine without hipcc: the library's kernels)

    def _fold_key(self) -> tuple:
        """The links that must stay ops of their own (those with learnable parameters), as the key of a fold mask."""
        key = tuple(sorted({link for link, _ in self._learnable}))
        if key not in self._fold_masks:
            self._fold_masks[key] = foldable_links(self._spec, keep=key)
        return key

    def _dynamics_walk(self) -> _DeviceWalk:
        """The whole-tree walk of the dynamics kernels, forward and backward.  Links behind fixed joints (end-effector frames,
        fingertips, and the flanges / palms / plates between moving joints) are folded away: their inertia is added to the
        nearest moving ancestor's row and their transform composed into the rows of the links below them, once on the host
        (flatten.fold_link_table), and the walk leaves them out — the same torques / inertia matrix / accelerations and the
        same gradients from one op per DoF (Panda 8 -> 7, Panda with gripper 12 -> 9, Allegro 20 -> 16, Fetch 24 -> 14).  Links
        with learnable parameters stay ops of their own, and so does whatever would have been folded into them or would have
        had to carry a transform for them (flatten.foldable_links)."""
        if not self._learnable and self._dyn_walk is not None:      # (constant model: the walk never changes)
            return self._dyn_walk
        mode = self._own_kernel_mode()
        have = self.__dict__.get("_dyn_walk_learnable")     # (a model with learnable links asks on every call)
        if have is not None and have[0] == (self._learnable_version, mode) and (
                mode == "off" or self._device.type != "cuda" or getattr(have[1].program, "_special_tried", False)):
            return have[1]
        key = self._fold_key()
        if not self._fold_masks[key].any():
            dw = self._get_walk(("tree",), whole_tree=True)
        else:
            dw = self._get_walk(("tree", "folded", key), whole_tree=True, folded=True, fold_key=key)
        if mode != "off" and self._device.type == "cuda" and not getattr(dw.program, "_special_tried", False):
            # the robot's OWN kernels on first use.  "auto" (the default, round 6): whatever is already built — the code objects
            # shipped next to the library, the run-time cache of an earlier specialize() — is attached, nothing is compiled; "build"
            # (DRM_SPECIALIZE=1, model.own_kernels = "build"): every robot without a compiled straight-line shape builds its kernels
            # (specialize.py; ~2 s once per robot and machine; a machine without hipcc keeps the loop kernels).  DRM_SPECIALIZE=tune:
            # robots WITH a compiled shape (other than plain 7-DoF arms) build theirs too and keep, per entry point, the faster
            dw.program._special_tried = True
            from . import specialize as sp
            from .flatten import SHAPE_ARM_CHAIN, SHAPE_ARM_HAND, SHAPE_FINGERS
            auto = mode == "auto"
            try:
                if sp.arm_qualifies(dw.program, self._n_dofs):
                    if not self._learnable:
                        sp.attach_arm(dw.program, self._ops_f(dw).detach().cpu().numpy(), self._n_dofs, cached_only=auto)   # (constants folded in)
                        for what in dw.program._special_missed:
                            self._own_kernel_miss(what, sp.CacheMiss("not in the cache"))
                    else:
                        # learnable link parameters: the reverse-mode kernel of THIS set of learnable blocks — every other block of
                        # the table is still a constant of the robot and folds into the instruction stream (round 6)
                        kin, dyn = self._learnable_block_masks(dw)
                        sp.attach_arm_param(dw.program, self._ops_f(dw).detach().cpu().numpy(), self._n_dofs, kin, dyn, cached_only=auto)
                elif not dw.program.shape & (SHAPE_ARM_CHAIN | SHAPE_ARM_HAND | SHAPE_FINGERS):
                    if dw.program.n_ops <= sp.MAX_STATIC_OPS:
                        sp.attach(dw.program, self._spec, self._n_dofs, self._const_table(dw), cached_only=auto)
                elif (os.environ.get("DRM_SPECIALIZE") == "tune" and not dw.program.shape & SHAPE_ARM_CHAIN
                      and dw.program.n_ops <= sp.MAX_STATIC_OPS):
                    sp.attach(dw.program, self._spec, self._n_dofs, self._const_table(dw), ignore_tuned=True)
                    sp.tune(dw.program, self._ops_f(dw).detach(), dw.ops_i, self._n_dofs)
                elif auto and not dw.program.shape & SHAPE_ARM_CHAIN and dw.program.n_ops <= sp.MAX_STATIC_OPS and not self._learnable:
                    # a robot WITH a compiled shape in the library (an arm that carries a hand, a hand): its own kernels where a
                    # tuning record — this machine's `specialize(tune=True)`, or the one shipped with the package — says they are
                    # the faster ones, and only those entry points; silently none without a record
                    try:
                        sp.attach(dw.program, self._spec, self._n_dofs, self._const_table(dw), cached_only=True, tuned_only=True)
                    except sp.CacheMiss:
                        pass
            except sp.CacheMiss as err:
                self._own_kernel_miss("the dynamics walk", err)
            except sp.SpecializeError:
                pass
        if not self._learnable:
            self._dyn_walk = dw
        else:
            self.__dict__["_dyn_walk_learnable"] = ((self._learnable_version, mode), dw)
        return dw

    def _static_rows(self, fold_key: Optional[tuple]) -> torch.Tensor:
        """[L + 1, OPF_STRIDE] snapshot of the constant rows, with the links of a fold mask folded into their parents."""
        if self._static_table is None:
            self._link_table()
        L1 = len(self._bodies) + 1
        if fold_key is None:
            return self._static_table[:L1]
        if fold_key not in self._static_folded:
            with torch.no_grad():
                rows = fold_link_table(self._spec, self._static_table[:L1].cpu().numpy(), self._fold_masks[fold_key])
                self._static_folded[fold_key] = torch.from_numpy(rows.astype(np.float32)).to(self._device)
        return self._static_folded[fold_key]

    def _ops_f(self, dw: _DeviceWalk) -> torch.Tensor:
        """[cap, OPF_STRIDE] constants gathered (and axis-canonicalised) in walk order; ONE differentiable
        gather (+ exact sign flips) from the link table, cached while nothing is learnable."""
        if not self._learnable and dw.static_ops_f is not None:
            return dw.static_ops_f
        if self._learnable and len(self._learnable_link_list()) <= 32 and not self._has_skew():
            return self._ops_f_learnable(dw)      # (more learnable links than the fused kernel takes: the torch path below)
        table = self._link_table(dw.fold_key)
        ops_f = (table.reshape(-1).index_select(0, dw.gather) * dw.gsign).reshape(dw.program.capacity, OPF_STRIDE)
        if not self._learnable:
            dw.static_ops_f = ops_f
        return ops_f

    def _learnable_link_list(self) -> list:
        """The links with a learnable parameter, ascending (cached per set of learnable parameters)."""
        have = self.__dict__.get("_learnable_sorted")
        if have is None or have[0] != self._learnable_version:
            have = self.__dict__["_learnable_sorted"] = (self._learnable_version, sorted({link for link, _ in self._learnable}))
        return have[1]

    def _has_skew(self) -> bool:
        have = self.__dict__.get("_skew_any")
        if have is None:
            have = self.__dict__["_skew_any"] = bool(self._spec.skew.any())
        return have

    def _ops_f_learnable(self, dw: _DeviceWalk) -> torch.Tensor:
        """The walk table with learnable links through ONE fused kernel (backend.WalkTable): the constant entries come
        from a cached gather of the constant link table, the entries of the learnable links are rebuilt from their
        parameter callables inside the kernel, and the autograd graph holds a single node."""
        links, base, sel = self._learnable_plan(dw)
        if self._table_links:
            # ABI 13: from the parameter tensors where they lie, the known modules' arithmetic inside the kernel (backend.WalkTableLinks)
            plan, sources = self._learnable_sources(links)
            ops_f = backend.WalkTableLinks.apply(base, sel, dw.gsign, plan, *sources)
        else:
            ops_f = backend.WalkTable.apply(base, sel, dw.gsign, len(links), *self._learnable_pieces(links))
        return ops_f.reshape(dw.program.capacity, OPF_STRIDE)

    def _learnable_sources(self, links):
        """(backend.LinkSourcePlan, live tensors) of the given learnable links.  A piece that is a constant of the model is part of
        the plan; a piece supplied by a parameter module is LIVE: the module's RAW parameter and its form where the kernels know the
        module (exactly PositiveScalar for mass / damping, exactly one of the l[6] inertia-matrix modules for inertia_mat; exactly
        UnconstrainedTensor / UnconstrainedScalar: the parameter itself), the output of the module's call otherwise.  Cached per set
        of links and modules."""
        from . import rigid_body_params as rbp
        key = tuple(links)
        cached = self._source_plan
        if cached is None or cached[0] != key:
            entries, fixed, getters, refs = [], [], [], []      # refs: (module._parameters, name) of a live piece, None for a module's call
            for i in links:
                b = self._bodies[i]
                link = []
                for name, fn in (("rot_angles", b.rot_angles), ("trans", b.trans), ("mass", b.inertia.mass), ("com", b.inertia.com),
                                 ("inertia_mat", b.inertia.inertia_mat), ("damping", b.joint_damping)):
                    form, const = backend.FORM_PLAIN, 0.0
                    if not isinstance(fn, torch.nn.Module):
                        value = fn()
                        value = self._zero1 if value is None else value
                        fixed.append(value.detach().to(device=self._device, dtype=torch.float32).reshape(-1).contiguous())
                        link.append((form, const, None))
                        continue
                    fixed.append(None)
                    kind = type(fn)
                    if name in ("mass", "damping") and kind is rbp.PositiveScalar:
                        form, const = backend.FORM_SQUARE_PLUS, fn._min_val
                    elif name == "inertia_mat" and kind is rbp.Symm3DInertiaMatrixNet:
                        form = backend.FORM_SYMM
                    elif name == "inertia_mat" and kind is rbp.SymmPosDef3DInertiaMatrixNet:
                        form, const = backend.FORM_SPD, fn.spd_3d_inertia_mat_diag_bias
                    elif name == "inertia_mat" and kind is rbp.CovParameterized3DInertiaMatrixNet:
                        form, const = backend.FORM_COV, fn.spd_3d_cov_inertia_mat_diag_bias
                    link.append((form, const, fn if form != backend.FORM_PLAIN else None))
                    if form != backend.FORM_PLAIN:           # (the module's own dictionary: nn.Module.__getattr__ is three times slower)
                        getters.append(lambda d=fn._parameters: d["l"])
                        refs.append((fn._parameters, "l"))
                    elif kind in (rbp.UnconstrainedTensor, rbp.UnconstrainedScalar):
                        getters.append(lambda d=fn._parameters: d["param"])
                        refs.append((fn._parameters, "param"))
                    else:
                        getters.append(fn)
                        refs.append(None)
                entries.append(link)
            cached = self._source_plan = (key, backend.LinkSourcePlan(entries, fixed), getters, refs)
        return cached[1], [g() for g in cached[2]]

    def _learnable_plan(self, dw: _DeviceWalk):
        """(learnable links, base, sel) of a walk: the table of the CONSTANT links gathered into walk order, and for every entry of
        the table the element of a learnable link's row it comes from (slot * 32 + column; -1: constant).  Cached per set of links."""
        links = self._learnable_link_list()
        key = tuple(links)
        plan = dw.learnable_plan
        if plan is None or plan[0] != key:
            with torch.no_grad():
                static = self._with_virtual_rows(self._static_rows(dw.fold_key))
                base = (static.reshape(-1).index_select(0, dw.gather) * dw.gsign).contiguous()
            gather = dw.program.gather.reshape(-1)
            row_of = {link: i for i, link in enumerate(links)}
            sel = np.full(gather.shape, -1, np.int32)
            for e, flat in enumerate(gather):
                link, col = divmod(int(flat), OPF_STRIDE)
                if link in row_of:
                    sel[e] = row_of[link] * OPF_STRIDE + col
            plan = dw.learnable_plan = (key, base, torch.from_numpy(sel).to(self._device))
        return links, plan[1], plan[2]

    def _learnable_pieces(self, links) -> list:
        """The outputs of the parameter callables of the given links, six per link (backend.WalkTable's ``pieces``)."""
        zero1 = self._zero1
        pieces = []
        for i in links:
            b = self._bodies[i]
            damping = b.joint_damping()
            pieces += [b.rot_angles(), b.trans(), b.inertia.mass(), b.inertia.com(), b.inertia.inertia_mat(),
                       damping if damping is not None else zero1]
        return pieces

    def _chain_walk(self, idx: int) -> _DeviceWalk:
        """The root -> link chain walk of the kinematics calls that do NOT run under autograd.  Without learnable parameters the
        fixed links between the chain's moving joints are stepped over (their transforms composed into the next link's row of
        the folded table, flatten.fold_link_table; a fixed TARGET keeps its op, with the fixed links right before it composed into
        its row): the same pose and Jacobian from fewer ops (Panda with gripper: 10 -> 8 to a finger or to the tool frame, a
        capacity-8 walk; TriFinger fingertip: 6 -> 4).  With learnable parameters, and under autograd, the plain walk."""
        if idx == 0:
            return self._get_walk(("chain", idx), targets=[])
        if self._learnable:
            return self._get_walk(("chain", idx), targets=[idx])
        hit = self._chain_walks.get(idx)      # (constant model: the walk of a link never changes; cleared when a link turns learnable)
        if hit is not None:
            return hit
        dw = self._chain_walks[idx] = self._chain_walk_build(idx)
        return dw

    def _chain_walk_build(self, idx: int) -> _DeviceWalk:
        key = self._fold_key()
        fold = self._fold_masks[key]
        chain = self._spec.chain_to(idx)
        if fold[idx] and len(chain) > 1 and fold[chain[-2]]:
            # the target sits behind several fixed joints in a row (flange -> hand -> tool frame): it alone keeps an op, whose row
            # carries the others' transforms — a fold mask of its own, the target un-folded
            tkey = ("target", idx) + tuple(key)
            if tkey not in self._fold_masks:
                mask = fold.copy()
                mask[idx] = False
                self._fold_masks[tkey] = mask
            key, fold = tkey, self._fold_masks[tkey]
        if not any(fold[c] and not all(fold[d] for d in chain[n + 1:]) for n, c in enumerate(chain)):
            return self._get_walk(("chain", idx), targets=[idx])      # nothing to step over
        return self._get_walk(("chain", idx, "folded", key), targets=[idx], folded=True, fold_key=key)

    def _fanout_chains(self, targets, merged: _DeviceWalk):
        """Per-target chain walks for the fan-out FK kernel, or None when the merged walk is the better plan: 2..4
        targets whose chains overlap so little that walking them separately costs < 1.25x the ops of the merged
        walk (the fingertips of a hand: every finger hangs off the palm)."""
        key = ("fanout", tuple(targets))
        if key not in self._fanout_plans:
            plan = None
            if 2 <= len(targets) <= 4:
                lengths = [len(self._spec.chain_to(t)) for t in targets]
                if sum(lengths) <= 1.25 * merged.program.n_ops and merged.program.n_ops > 8:
                    if not self._learnable:     # the folded chain walks (fixed links stepped over), when they share a capacity
                        walks = [self._chain_walk(t) for t in targets]
                        if len({w.program.capacity for w in walks}) == 1:
                            self._fanout_plans[key] = walks
                            self._fan_special(key, walks)
                            return walks
                    cap = max(build_walk(self._spec, targets=[t]).capacity for t in targets)
                    plan = []
                    for t in targets:
                        prog = build_walk(self._spec, targets=[t], min_capacity=cap)
                        plan.append(_DeviceWalk(
                            program=prog,
                            ops_i=torch.from_numpy(prog.ops_i_dev).to(self._device).contiguous(),
                            gather=torch.from_numpy(prog.gather.reshape(-1)).to(self._device),
                            gsign=torch.from_numpy(prog.gsign.reshape(-1)).to(self._device)))
            self._fanout_plans[key] = plan
        return self._fanout_plans[key]

    def _fan_special(self, key, walks) -> None:
        """The fan-out FK call's own kernel — every chain's constants folded into the instruction stream (specialize.attach_fan) —
        for THIS ordered set of targets (`key` of _fanout_plans): built already (the default) or compiled now (specialize(),
        DRM_SPECIALIZE=1).  The handle stays with the plan (`_fan_handles`), never on the chain walks, which other sets share."""
        if self._learnable or self._device.type != "cuda" or key in self._fan_handles:
            return
        mode = self._own_kernel_mode()
        if mode == "off":
            return
        from . import specialize as sp
        try:
            handle = sp.attach_fan([w.program for w in walks], [self._ops_f(w).detach().cpu().numpy() for w in walks], self._n_dofs,
                                   cached_only=mode == "auto")
            if handle:
                self._fan_handles[key] = handle
        except sp.CacheMiss as err:
            self._own_kernel_miss("forward kinematics of links %s" % (list(key[1]),), err)
        except sp.SpecializeError:
            if getattr(self, "_arm_specialized", False):
                raise      # (the environment opt-in on a machine without hipcc keeps the library's kernels)

    def _fan_own(self, targets) -> Optional[int]:
        """The handle of the own fan-out kernel of this ordered set of targets, or None."""
        return self._fan_handles.get(("fanout", tuple(targets))) if self._own_kernel_mode() != "off" else None

    def _kinematic_param_mask(self, dw: _DeviceWalk) -> int:
        """bit k set <=> op k's R_fixed / trans come from a learnable parametrisation (needs a constant gradient)."""
        have = dw.__dict__.get("_kin_mask")
        if have is not None and have[0] == self._learnable_version:
            return have[1]
        links = {link for link, pname in self._learnable if pname in ("trans", "rot_angles")}
        mask = 0
        for k, link in enumerate(dw.program.links):
            if int(link) in links:
                mask |= 1 << k
        dw.__dict__["_kin_mask"] = (self._learnable_version, mask)
        return mask

    def _differentiable(self, dw: _DeviceWalk) -> None:
        """The backward kernels take walks of up to 64 links and 6 branch points (any joint model)."""
        if not dw.program.backward_ok:
            raise NotImplementedError("gradients need a walk of <= 64 links with <= 6 branch points (this one: %d links, "
                                      "%d slots)" % (dw.program.n_ops, dw.program.n_slots))

    def _require_device(self):
        """The library that computes on the model's device must be there: libdrm_hip.so for a HIP device, libdrm_cpu.so (the host
        build of the same C ABI) for the CPU, the reference's default device (robot_model.py:100-104).  One never stands in for
        the other (backend.library_for raises NativeLibraryError)."""
        backend.library_for(self._device)

    # ------------------------------------------------------------------ kinematic state (reference API)
    @tensor_check
    def update_kinematic_state(self, q: torch.Tensor, qd: torch.Tensor) -> None:
        """Record the joint state; ``body.pose`` / ``body.vel`` of every link then reflect it (robot_model.py:139-195).

        The reference walks the tree here and stores a pose and a velocity on every body; the kernels are
        stateless, so this only remembers (q, qd) and the per-link quantities are evaluated when read:
        poses by one all-links FK launch, a link's body-frame velocity from its Jacobian (R^T J qd).
        """
        assert q.ndim == 2
        assert qd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        self._kin_state = (q.detach(), qd.detach())
        self._kin_cache = {}

    def _all_poses(self):
        """pos [B, L', 3], quat [B, L', 4], rot [B, L', 3, 3] of every link of the recorded state, indexed by link (the kernel's
        outputs as they stand when the links are in walk order, else gathered once)."""
        if "poses" not in self._kin_cache:
            q = self._kin_state[0]
            with torch.no_grad():
                cols = self._fk_links(q, list(range(len(self._bodies))))
                pos = torch.stack([cols[i][0] for i in range(len(self._bodies))], dim=1)
                quat = torch.stack([cols[i][1] for i in range(len(self._bodies))], dim=1)
            x, y, z, w = quat.unbind(-1)
            rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                               2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                               2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1)
            self._kin_cache["poses"] = (pos, quat, rot.reshape(*quat.shape[:-1], 3, 3))
        return self._kin_cache["poses"]

    def _link_pose(self, idx: int) -> LinkPose:
        if self._kin_state is None:   # a fresh body sits at the identity (rigid_body.py:64-76)
            return LinkPose(torch.eye(3, device=self._device).unsqueeze(0), torch.zeros(1, 3, device=self._device),
                            torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=self._device))
        pos, quat, rot = self._all_poses()
        return LinkPose(rot[:, idx], pos[:, idx], quat[:, idx])

    def _link_velocity(self, idx: int) -> LinkVelocity:
        if self._kin_state is None:
            return LinkVelocity(torch.zeros(1, 3, device=self._device), torch.zeros(1, 3, device=self._device))
        key = ("vel", idx)
        if key not in self._kin_cache:
            q, qd = self._kin_state
            rot = self._all_poses()[2][:, idx]
            with torch.no_grad():
                lin, ang = self.compute_endeffector_jacobian(q, self._bodies[idx].name)
            to_body = lambda jac: torch.einsum("bji,bj->bi", rot, torch.einsum("bij,bj->bi", jac, qd))
            self._kin_cache[key] = LinkVelocity(to_body(lin), to_body(ang))
        return self._kin_cache[key]

    # ------------------------------------------------------------------ FK
    def _fk_links(self, q: torch.Tensor, link_idxs: List[int]) -> Dict[int, Tuple[torch.Tensor, torch.Tensor]]:
        """{link index: (pos [B,3], quat [B,4])} — column views of ONE launch whose targets are taken in WALK order (the many-target
        kernel then writes its outputs a group of consecutive slots at a time, DRM_WALK_TARGETS_ORDERED); the root's identity
        pose is two small tensors of its own."""
        out = {}
        B = q.shape[0]
        # (the walk order of a set of links is found once per set: the per-call Python work of a 13-link dictionary was ~10x the
        # kernel's time at 65 536 rows)
        plans = self.__dict__.setdefault("_fk_links_plans", {})
        key = tuple(link_idxs)
        plan = plans.get(key)
        if plan is None:
            wanted = set(int(i) for i in link_idxs if i != 0)
            ordered = [i for i in self._spec.preorder() if i in wanted]
            plan = plans[key] = (0 in link_idxs, ordered)
        has_root, ordered = plan
        if has_root:            # (read-only views of two constants: no kernel, no memory)
            if self._root_pose is None:
                self._root_pose = (torch.zeros(1, 3, device=self._device), torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=self._device))
            out[0] = (self._root_pose[0].expand(B, 3), self._root_pose[1].expand(B, 4))
        if ordered:
            dw = self._get_walk(("fk", tuple(ordered)), targets=ordered) if len(ordered) > 1 else None
            if dw is not None and not (torch.is_grad_enabled() and (q.requires_grad or self._ops_f(dw).requires_grad)):
                # no graph to build: link-major outputs — every link's poses a contiguous array.  A few links at the ends of
                # (nearly) disjoint chains, the fingertips of a hand: a wavefront per chain (drm_fk_fanout_links); else one walk
                # over all of them (drm_fk_links)
                self._require_device()
                fan = self._fanout_chains(ordered, dw)
                if fan is not None:
                    pos, quat = backend.fk_fanout([(c.program, self._ops_f(c), c.ops_i) for c in fan], q, self._n_dofs, link_major=True,
                                                  own=self._fan_own(ordered))
                else:
                    pos, quat = backend.fk_links(dw.program, self._ops_f(dw), dw.ops_i, q, len(ordered), self._n_dofs)
                out.update(zip(ordered, zip(pos.unbind(0), quat.unbind(0))))      # (one unbind per array instead of an index op per link)
                return out
            pos, quat = self._fk_targets(q, ordered)
            out.update(zip(ordered, zip(pos.unbind(1), quat.unbind(1))))
        return out

    def _fast_entry_learnable(self, fast, entry: str, scratch: Optional[str], dw: "_DeviceWalk", chain, target_op: int) -> Optional[tuple]:
        """The prepared call of a model WITH learnable link parameters (round 6): the C++ side rebuilds the walk table from the parameter
        tensors in front of every call (drm_walk_table_links, looked up in the modules' own parameter dictionaries each time) whenever
        the call builds no autograd graph — torch.no_grad(), or every parameter frozen: a learned model in a control loop costs what a
        constant one does plus one small launch.  None where the table does not come from the links path, a live piece is the output of
        a module the kernels do not know, or the call needs two walks."""
        import ctypes
        if (chain is not None or not hasattr(fast.FastCall, "set_table") or not self._table_links or self._has_skew()
                or len(self._learnable_link_list()) > 32):
            return None
        links, base, sel = self._learnable_plan(dw)
        plan, sources = self._learnable_sources(links)
        refs = self._source_plan[3]
        if any(r is None for r in refs) or any(t.device != self._device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n
                                              for t, n in zip(sources, plan.sizes)):
            return None
        lib = backend.library_for(self._device)
        with torch.no_grad():
            ops_f = self._ops_f(dw)
        shared = backend._walk_struct(dw.program, ops_f.detach(), dw.ops_i, self._n_dofs)
        walk = backend.DrmWalk.from_buffer_copy(shared)      # (this call's own struct: the C++ side rewrites its table pointer per call)
        pieces = plan.pieces(sources)
        keep = [walk, dw.ops_i, lib, plan, base, sel, dw.gsign]
        call = fast.FastCall(backend._fn_addr(lib, entry), backend._fn_addr(lib, scratch) if scratch else 0, ctypes.addressof(walk), 0,
                             self._n_dofs, target_op, self._device.type == "cuda",
                             self._device.index if self._device.index is not None else -1, tuple(keep))
        call.set_table(backend._fn_addr(lib, "drm_walk_table_links"), ctypes.addressof(pieces), ctypes.addressof(plan.forms), plan.n_links,
                       base, sel.data_ptr(), dw.gsign.data_ptr(), list(plan.live), list(plan.sizes), [r[0] for r in refs], [r[1] for r in refs])
        return (call, dw.program, dw.program._ws_cache)

    def _fk_targets(self, q: torch.Tensor, link_idxs: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        """pos [B,T,3], quat [B,T,4] of the given links (root targets filled with the identity pose)."""
        self._require_device()
        B = q.shape[0]
        non_root = [i for i in link_idxs if i != 0]
        pos = quat = None
        if len(non_root) != len(link_idxs):    # the root link's pose is the identity: no kernel needed for it
            pos = torch.zeros(B, len(link_idxs), 3, device=self._device)
            quat = torch.zeros(B, len(link_idxs), 4, device=self._device)
            quat[..., 3] = 1.0
        if non_root:
            dw = self._get_walk(("fk", tuple(non_root)), targets=non_root)
            ops_f = self._ops_f(dw)
            needs_grad = torch.is_grad_enabled() and (q.requires_grad or ops_f.requires_grad)
            fan = None if needs_grad else self._fanout_chains(non_root, dw)
            if fan is not None:
                p, r = backend.fk_fanout([(c.program, self._ops_f(c), c.ops_i) for c in fan], q, self._n_dofs)
            elif needs_grad and len(non_root) > 1 and not dw.program.backward_ok:
                # a many-target walk the backward kernels do not take (more than 6 branch points open at once, > 64 ops): the targets'
                # root -> link chains one by one — a chain has no branch point — as the reference's per-link autograd graph would
                parts = [self._fk_targets(q, [i]) for i in non_root]
                p, r = torch.cat([a for a, _ in parts], dim=1), torch.cat([b for _, b in parts], dim=1)
            elif needs_grad:
                self._differentiable(dw)
                p, r = _FkPositions.apply(q, ops_f, dw, len(non_root), self._n_dofs, self._kinematic_param_mask(dw))
            else:
                p, r = backend.fk(dw.program, ops_f, dw.ops_i, q, len(non_root), self._n_dofs)
            if len(non_root) == len(link_idxs):
                return p, r
            cols = [k for k, i in enumerate(link_idxs) if i != 0]
            if cols == list(range(cols[0], cols[0] + len(cols))):     # (a slice: no index tensor, capturable into a hipGraph)
                pos[:, cols[0]:cols[0] + len(cols)] = p
                quat[:, cols[0]:cols[0] + len(cols)] = r
            else:
                pos[:, cols] = p
                quat[:, cols] = r
        return pos, quat

    def compute_forward_kinematics_all_links(self, q: torch.Tensor) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """{link_name: (pos [B,3], quat_xyzw [B,4])} for every link (robot_model.py:197-221).  (Repeat calls of a constant model with a
        batched q: one C++ call over drm_fk_links' link-major outputs, see compute_forward_kinematics.)"""
        ent = self.__dict__.get("_fast_links")
        if ent is not None and ent[1]._ws_cache is ent[2]:
            pairs = ent[0].links(q, len(ent[3]), self._stream_arg())
            if pairs.__class__ is list:
                names, B = self.__dict__["_body_names"], q.shape[0]
                out = dict.fromkeys(names)
                out[names[0]] = (self._root_pose[0].expand(B, 3), self._root_pose[1].expand(B, 4))
                for i, pair in zip(ent[3], pairs):
                    out[names[i]] = pair
                return out
            if pairs is not None:
                backend._check(pairs, backend.library_for(self._device))
        return self._compute_forward_kinematics_all_links(q)

    @tensor_check
    def _compute_forward_kinematics_all_links(self, q: torch.Tensor) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        assert q.ndim == 2
        assert q.shape[1] == self._n_dofs
        names = self.__dict__.get("_body_names")
        if names is None:       # (ModuleList indexing costs ~3 us per link and call)
            names = self.__dict__["_body_names"] = [b.name for b in self._bodies]
            self.__dict__["_all_link_idxs"] = list(range(len(names)))
        ent = self.__dict__.get("_fast_links")
        cols = self._fk_links(q, self.__dict__["_all_link_idxs"])
        if ent is None or ent[1]._ws_cache is not ent[2]:
            self.__dict__["_fast_links"] = self._fast_links_entry()
        return {name: cols[i] for i, name in enumerate(names)}

    def _fast_links_entry(self) -> Optional[tuple]:
        """(FastCall of drm_fk_links over every non-root link, its walk program, the program's struct cache, the links in the walk's
        target order) — None for models the prepared call does not serve (learnable parameters, a robot of one link, no C++ host path)."""
        plan = self.__dict__.get("_fk_links_plans", {}).get(tuple(self.__dict__["_all_link_idxs"]))
        if plan is None or not plan[0] or len(plan[1]) < 2 or self._root_pose is None:
            return None
        ordered = plan[1]
        dw = self._get_walk(("fk", tuple(ordered)), targets=ordered)
        if self._fanout_chains(ordered, dw) is not None:
            return None
        ent = self._fast_entry("drm_fk_links", None, dw)
        return None if ent is None else ent + (list(ordered),)

    @tensor_check
    def compute_forward_kinematics_links(self, q: torch.Tensor, link_names: List[str]) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """{link name: (pos [B, 3], quat xyzw [B, 4])} of the NAMED links in one launch — what calling
        compute_forward_kinematics (robot_model.py:223-248) once per link returns, e.g. for the fingertips of a hand (BASELINE
        configuration 4).  Not in the reference (which recomputes every link per call, robot_model.py:139-195).  Without a graph to
        build every tensor is a contiguous array of its own (link-major launch); under autograd they are columns of one
        [B, T, .] result, differentiable like compute_forward_kinematics."""
        idxs = [self._name_to_idx_map[name] for name in link_names]
        cols = self._fk_links(q, idxs)
        return {name: cols[i] for name, i in zip(link_names, idxs)}

    def _fast_entry(self, entry: str, scratch: Optional[str], dw: "_DeviceWalk", chain: Optional["_DeviceWalk"] = None,
                    target_op: int = -1) -> Optional[tuple]:
        """(FastCall, walk program, the program's struct cache) of one prepared eager call of this walk through the C ABI's `entry`
        — None when the C++ host path is not built, the model has learnable parameters (its table changes every call) or lives on
        a device kind the path does not serve.  The call stays valid while the program's struct cache does (the identity is checked
        per call): attaching own kernels or rebuilding the table retires it and the next call through the Python path renews it."""
        fast = backend.hostcall()
        if fast is None or not hasattr(fast, "FastCall") or self._device.type not in ("cuda", "cpu"):
            return None
        if self._learnable:
            return self._fast_entry_learnable(fast, entry, scratch, dw, chain, target_op)
        import ctypes
        lib = backend.library_for(self._device)
        ops_f = self._ops_f(dw)
        walk = backend._walk_struct(dw.program, ops_f, dw.ops_i, self._n_dofs)
        keep, walk2 = [walk, ops_f, dw.ops_i, lib], 0
        if chain is not None:      # (drm_fk_rnea: the dynamics walk and the target's chain walk)
            cf = self._ops_f(chain)
            w2 = backend._walk_struct(chain.program, cf, chain.ops_i, self._n_dofs)
            keep += [w2, cf, chain.ops_i]
            walk2 = ctypes.addressof(w2)
        call = fast.FastCall(backend._fn_addr(lib, entry), backend._fn_addr(lib, scratch) if scratch else 0, ctypes.addressof(walk), walk2,
                             self._n_dofs, target_op, self._device.type == "cuda",
                             self._device.index if self._device.index is not None else -1, tuple(keep))
        if chain is not None:
            return (call, dw.program, dw.program._ws_cache, chain.program, chain.program._ws_cache)
        return (call, dw.program, dw.program._ws_cache)

    def compute_forward_kinematics(self, q: torch.Tensor, link_name: str, recursive: bool = False
                                   ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(pos [B,3], quat_xyzw [B,4]) of ``link_name`` (robot_model.py:223-248).

        ``recursive`` selects between two implementations in the reference that return the same
        pose on a fresh model; both map to the same kernel here.
        A constant model's repeat calls go through ONE C++ call (csrc/drm_hostcall.cpp FastCall: tensor_check, the asserts below,
        the allocation and the launch); whatever that does not take as it is — and every first call — comes here.
        """
        ent = self._fast_fk.get(link_name)
        if ent is not None and ent[1]._ws_cache is ent[2]:
            out = ent[0].kinematics(q, 0, self._stream_arg())
            if out.__class__ is tuple:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_forward_kinematics(q, link_name, recursive)

    @tensor_check
    def _compute_forward_kinematics(self, q: torch.Tensor, link_name: str, recursive: bool = False):
        assert q.ndim == 2
        assert q.shape[1] == self._n_dofs
        idx = self._name_to_idx_map[link_name]
        if idx != 0 and not (torch.is_grad_enabled() and (q.requires_grad or self._learnable)):
            # the common call: one kernel, outputs allocated in their final shape (no slicing ops on the way out)
            self._require_device()
            dw = self._chain_walk(idx)
            out = backend.fk(dw.program, self._ops_f(dw), dw.ops_i, q, 1, self._n_dofs, squeeze=True)
            if link_name not in self._fast_fk or self._fast_fk[link_name][1]._ws_cache is not self._fast_fk[link_name][2]:
                ent = self._fast_entry("drm_fk", None, dw)
                if ent is not None:
                    self._fast_fk[link_name] = ent
            return out
        pos, quat = self._fk_targets(q, [idx])
        return pos[:, 0], quat[:, 0]

    def fk_mse_loss(self, q: torch.Tensor, link_name: str, target: torch.Tensor) -> torch.Tensor:
        """``torch.nn.functional.mse_loss(self.compute_forward_kinematics(q, link_name)[0], target)`` — the loss of the reference's
        kinematics-learning loop (examples/learn_kinematics_of_iiwa.py:47-55) — as ONE differentiable node: for a serial 7-DoF arm
        (the iiwa of BASELINE configuration 5, the Panda) and a batch that is a multiple of 64 rows, forward kinematics, the loss
        and its gradients with respect to q and the learnable ``trans`` / ``rot_angles`` come from one pass over q (drm_fk_mse)
        instead of an FK launch, the loss kernels and a backward launch; every other robot / batch takes exactly the composition
        above.  Not in the reference."""
        assert q.ndim == 2 and q.shape[1] == self._n_dofs and target.shape == (q.shape[0], 3)
        self._require_device()
        idx = self._name_to_idx_map[link_name]
        if idx != 0 and q.shape[0] % 64 == 0 and q.shape[0] > 0:
            dw = self._get_walk(("fk", (idx,)), targets=[idx])
            if dw.program.shape & 1 and dw.program.capacity == 8 and self._n_dofs == 7:    # DRM_WALK_ARM_CHAIN
                if (self._learnable and torch.is_grad_enabled() and not self._spec.skew.any()
                        and len({link for link, _ in self._learnable}) <= backend.FK_MSE_MAX_LINKS and self._fk_mse_links):
                    # learnable links: from their parameter tensors to the gradients with respect to them in TWO launches and one
                    # autograd node (drm_fk_mse_links, ABI 12) — no table pass before, no table backward pass after
                    links, base, sel = self._learnable_plan(dw)
                    pieces = self._learnable_pieces(links)
                    mask = self._kinematic_param_mask(dw)
                    if mask and all(p.device == self._device for p in pieces):
                        try:
                            self._differentiable(dw)
                            return _FkMseLinks.apply(q, target, base, sel, dw.gsign, dw, self._n_dofs, mask, *pieces)
                        except backend.KernelUnsupported:
                            pass
                ops_f = self._ops_f(dw)
                try:
                    if torch.is_grad_enabled() and (q.requires_grad or ops_f.requires_grad):
                        self._differentiable(dw)
                        return _FkMse.apply(q, target, ops_f, dw, self._n_dofs, self._kinematic_param_mask(dw))
                    return backend.fk_mse(dw.program, ops_f, dw.ops_i, q, target, self._n_dofs, 0, False)[0]
                except backend.KernelUnsupported:
                    pass
        pos, _ = self.compute_forward_kinematics(q, link_name)
        return torch.nn.functional.mse_loss(pos, target)

    # ------------------------------------------------------------------ Jacobian
    def compute_endeffector_jacobian(self, q: torch.Tensor, link_name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lin_jac [B,3,n], ang_jac [B,3,n]) at the link origin, world frame (robot_model.py:626-667).  (Repeat calls of a constant
        model: one C++ call, see compute_forward_kinematics.)"""
        ent = self._fast_jac.get(link_name)
        if ent is not None and ent[1]._ws_cache is ent[2]:
            out = ent[0].kinematics(q, 1, self._stream_arg())
            if out.__class__ is tuple:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_endeffector_jacobian(q, link_name)

    @tensor_check
    def _compute_endeffector_jacobian(self, q: torch.Tensor, link_name: str):
        assert len(q.shape) == 2
        assert q.shape[1] == self._n_dofs
        _, _, lin, ang = self._fk_and_jacobian(q, link_name)
        return lin, ang

    def compute_fk_and_jacobian(self, q: torch.Tensor, link_name: str
                                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(pos, quat, lin_jac, ang_jac) from ONE fused kernel launch.

        The reference's ``compute_endeffector_jacobian`` runs the full FK first and throws the pose
        away (robot_model.py:641); this returns it instead.
        """
        ent = self._fast_jac.get(link_name)
        if ent is not None and ent[1]._ws_cache is ent[2]:
            out = ent[0].kinematics(q, 2, self._stream_arg())
            if out.__class__ is tuple:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_fk_and_jacobian(q, link_name)

    @tensor_check
    def _compute_fk_and_jacobian(self, q: torch.Tensor, link_name: str):
        assert q.ndim == 2
        assert q.shape[1] == self._n_dofs
        return self._fk_and_jacobian(q, link_name)

    def _fk_and_jacobian(self, q: torch.Tensor, link_name: str):
        self._require_device()
        idx = self._name_to_idx_map[link_name]
        if idx != 0 and torch.is_grad_enabled() and (q.requires_grad or self._learnable):
            dw = self._get_walk(("chain", idx), targets=[idx])
            ops_f = self._ops_f(dw)
            if q.requires_grad or ops_f.requires_grad:
                self._differentiable(dw)
                return _FkJacobian.apply(q, ops_f, dw, self._n_dofs, self._kinematic_param_mask(dw))
            return backend.fk_jacobian(dw.program, ops_f, dw.ops_i, q, self._n_dofs)
        dw = self._chain_walk(idx)
        out = backend.fk_jacobian(dw.program, self._ops_f(dw), dw.ops_i, q, self._n_dofs)
        have = self._fast_jac.get(link_name)
        if idx != 0 and (have is None or have[1]._ws_cache is not have[2]):
            ent = self._fast_entry("drm_fk_jacobian", None, dw)
            if ent is not None:
                self._fast_jac[link_name] = ent
        return out

    def plan_fk_and_jacobian(self, q: torch.Tensor, link_name: str, want_pose: bool = True
                             ) -> "backend.FkJacobianPlan":
        """Prepared (allocation-free, graph-capturable) FK+Jacobian launch on fixed buffers."""
        self._require_device()
        assert q.ndim == 2 and q.shape[1] == self._n_dofs
        assert not self._learnable, "plans snapshot the constants; not available with learnable parameters"
        idx = self._name_to_idx_map[link_name]
        dw = self._chain_walk(idx)
        return backend.FkJacobianPlan(dw.program, self._ops_f(dw), dw.ops_i, q, self._n_dofs, want_pose)

    def plan_inverse_dynamics(self, q: torch.Tensor, qd: torch.Tensor, qdd_des: Optional[torch.Tensor],
                              include_gravity: bool = True, use_damping: bool = True) -> "backend.InverseDynamicsPlan":
        """Prepared (allocation-free, graph-capturable) inverse-dynamics launch on fixed buffers; ``qdd_des=None``
        gives the non-linear effects."""
        self._require_device()
        assert q.ndim == 2 and q.shape[1] == self._n_dofs
        assert not self._learnable, "plans snapshot the constants; not available with learnable parameters"
        dw = self._dynamics_walk()
        return backend.InverseDynamicsPlan(dw.program, self._ops_f(dw), dw.ops_i, q, qd, qdd_des, bool(include_gravity),
                                           bool(use_damping), self._n_dofs)

    def plan_fk_and_inverse_dynamics(self, q: torch.Tensor, qd: torch.Tensor, qdd_des: Optional[torch.Tensor],
                                     link_name: str, include_gravity: bool = True, use_damping: bool = True,
                                     outputs=None, put=None) -> "backend.FkInverseDynamicsPlan":
        """Prepared launch of inverse dynamics + the pose of ``link_name`` on fixed buffers (drm_fk_rnea): what the
        reference computes with compute_inverse_dynamics (robot_model.py:305-375) followed by
        compute_forward_kinematics (robot_model.py:223-248) on the same q.  One fused kernel for a serial 7-DoF arm
        whose last link is the target, the two walks back to back otherwise.  ``outputs``: caller-owned (tau [B,n], pos [B,3],
        quat [B,4]) buffers to write into.  ``put``: the destinations of a one-sided gather (distributed.PeerGather.put(): every
        launch also writes its rows into the other ranks' gathered arrays, drm_fk_rnea_put)."""
        self._require_device()
        assert q.ndim == 2 and q.shape[1] == self._n_dofs
        assert not self._learnable, "plans snapshot the constants; not available with learnable parameters"
        idx = self._name_to_idx_map[link_name]
        if idx == 0:
            raise ValueError("the root link has the identity pose; use plan_inverse_dynamics")
        tree = self._dynamics_walk()
        chain = self._get_walk(("chain", idx) + (("folded", tree.fold_key) if tree.folded else ()), targets=[idx],
                               folded=tree.folded, fold_key=tree.fold_key)
        self._arm_fused_special(tree, chain)
        return backend.FkInverseDynamicsPlan((tree.program, self._ops_f(tree), tree.ops_i),
                                             (chain.program, self._ops_f(chain), chain.ops_i),
                                             int(tree.program.op_of_link.get(idx, -1)),
                                             q, qd, qdd_des, bool(include_gravity), bool(use_damping), self._n_dofs,
                                             outputs=outputs, put=put)

    def compute_fk_and_inverse_dynamics(self, q: torch.Tensor, qd: torch.Tensor, qdd_des: torch.Tensor, link_name: str,
                                        include_gravity: Optional[bool] = True, use_damping: Optional[bool] = True
                                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(tau [B,n], pos [B,3], quat [B,4]) from one pass over q — see _compute_fk_and_inverse_dynamics; repeat calls of a constant
        model go through one prepared C++ call (csrc/drm_hostcall.cpp FastCall)."""
        ent = self._fast_fkid.get(link_name)
        if ent is not None and ent[1]._ws_cache is ent[2] and ent[3]._ws_cache is ent[4]:
            out = ent[0].fk_inverse_dynamics(q, qd, qdd_des, (1 if include_gravity else 0) | (2 if use_damping else 0), self._stream_arg())
            if out.__class__ is tuple:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_fk_and_inverse_dynamics(q, qd, qdd_des, link_name, include_gravity, use_damping)

    @tensor_check
    def _compute_fk_and_inverse_dynamics(self, q: torch.Tensor, qd: torch.Tensor, qdd_des: torch.Tensor, link_name: str,
                                         include_gravity: Optional[bool] = True, use_damping: Optional[bool] = True
                                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(tau [B,n], pos [B,3], quat [B,4]): compute_inverse_dynamics and compute_forward_kinematics of one link from
        a single pass over q (not differentiable; use the two separate methods under autograd)."""
        assert q.ndim == 2 and qd.ndim == 2 and qdd_des.ndim == 2
        assert q.shape[1] == self._n_dofs and qd.shape[1] == self._n_dofs and qdd_des.shape[1] == self._n_dofs
        idx = self._name_to_idx_map[link_name]
        if idx != 0 and not self._learnable:      # one eager call through the C++ host path (no plan object per call)
            self._require_device()
            tree = self._dynamics_walk()
            chain = self._get_walk(("chain", idx) + (("folded", tree.fold_key) if tree.folded else ()), targets=[idx],
                                   folded=tree.folded, fold_key=tree.fold_key)
            self._arm_fused_special(tree, chain)
            out = backend.fk_rnea((tree.program, self._ops_f(tree), tree.ops_i), (chain.program, self._ops_f(chain), chain.ops_i),
                                  int(tree.program.op_of_link.get(idx, -1)), q.detach(), qd.detach(), qdd_des.detach(),
                                  bool(include_gravity), bool(use_damping), self._n_dofs)
            if out is not None:
                have = self._fast_fkid.get(link_name)
                if have is None or have[1]._ws_cache is not have[2] or have[3]._ws_cache is not have[4]:
                    ent = self._fast_entry("drm_fk_rnea", "drm_rnea_scratch_floats_aligned", tree, chain,
                                           int(tree.program.op_of_link.get(idx, -1)))
                    if ent is not None:
                        self._fast_fkid[link_name] = ent
                return out
        # (this plan lives for one launch: a row or column slice of a larger tensor is copied, as compute_inverse_dynamics does)
        q, qd, qdd_des = (backend._dev_f32(t.detach(), name, self._n_dofs) for t, name in ((q, "q"), (qd, "qd"), (qdd_des, "qdd_des")))
        plan = self.plan_fk_and_inverse_dynamics(q, qd, qdd_des, link_name, bool(include_gravity), bool(use_damping))
        with backend._on_device(self._device):
            plan.launch()
        return plan.tau, plan.pos, plan.quat

    # ------------------------------------------------------------------ inverse dynamics
    def compute_inverse_dynamics(self, q: torch.Tensor, qd: torch.Tensor, qdd_des: torch.Tensor,
                                 include_gravity: Optional[bool] = True, use_damping: Optional[bool] = True
                                 ) -> torch.Tensor:
        """tau [B,n] achieving ``qdd_des`` (RNEA, robot_model.py:305-375).  (Repeat calls of a constant model: one C++ call, see
        compute_forward_kinematics.)"""
        ent = self._fast_id
        if ent is not None and ent[1]._ws_cache is ent[2]:
            out = ent[0].inverse_dynamics(q, qd, qdd_des, (1 if include_gravity else 0) | (2 if use_damping else 0), self._stream_arg())
            if out.__class__ is torch.Tensor:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_inverse_dynamics(q, qd, qdd_des, include_gravity, use_damping)

    @tensor_check
    def _compute_inverse_dynamics(self, q: torch.Tensor, qd: torch.Tensor, qdd_des: torch.Tensor,
                                  include_gravity: Optional[bool] = True, use_damping: Optional[bool] = True):
        assert q.ndim == 2
        assert qd.ndim == 2
        assert qdd_des.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        assert qdd_des.shape[1] == self._n_dofs
        self._require_device()
        return self._inverse_dynamics(q, qd, qdd_des, bool(include_gravity), bool(use_damping))

    def compute_non_linear_effects(self, q: torch.Tensor, qd: torch.Tensor, include_gravity: Optional[bool] = True,
                                   use_damping: Optional[bool] = True) -> torch.Tensor:
        """Coriolis + centrifugal + gravity + damping torques = RNEA with qdd = 0 (robot_model.py:377-400)."""
        ent = self._fast_id
        if ent is not None and ent[1]._ws_cache is ent[2]:
            out = ent[0].inverse_dynamics(q, qd, None, (1 if include_gravity else 0) | (2 if use_damping else 0), self._stream_arg())
            if out.__class__ is torch.Tensor:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_non_linear_effects(q, qd, include_gravity, use_damping)

    @tensor_check
    def _compute_non_linear_effects(self, q: torch.Tensor, qd: torch.Tensor, include_gravity: Optional[bool] = True,
                                    use_damping: Optional[bool] = True):
        assert q.ndim == 2 and qd.ndim == 2
        assert q.shape[1] == self._n_dofs and qd.shape[1] == self._n_dofs
        self._require_device()
        return self._inverse_dynamics(q, qd, None, bool(include_gravity), bool(use_damping))

    def iterative_newton_euler(self, base_lin_acc: torch.Tensor, base_ang_acc: torch.Tensor) -> None:
        """The reference's RNEA sweeps over per-body state written by ``update_kinematic_state`` (robot_model.py:250-303):
        an internal step of its Python recursion.  Here both sweeps are one kernel behind ``compute_inverse_dynamics``."""
        raise NotImplementedError("iterative_newton_euler is an internal step of the reference's per-link recursion; "
                                  "call compute_inverse_dynamics / compute_non_linear_effects")

    def _learnable_block_masks(self, dw) -> Tuple[int, int]:
        """(kinematic, dynamic): bit k set <=> op k's F / t block (`trans`, `rot_angles`) / its mass - mcom - I_o - damping block
        (`mass`, `com`, `inertia_mat`, `joint_damping`) comes from a learnable parametrisation."""
        kin_links = {link for link, pname in self._learnable if pname in ("trans", "rot_angles")}
        dyn_links = {link for link, pname in self._learnable if pname not in ("trans", "rot_angles")}
        kin = dyn = 0
        for k, link in enumerate(dw.program.links):
            if int(link) in kin_links:
                kin |= 1 << k
            if int(link) in dyn_links:
                dyn |= 1 << k
        return kin, dyn

    def _learnable_op_mask(self, dw) -> int:
        """Bit k set <=> op k of the walk belongs to a link with a learnable parameter (param_mask of the backward kernels)."""
        have = dw.__dict__.get("_op_mask")
        if have is not None and have[0] == self._learnable_version:
            return have[1]
        links = {link for link, _ in self._learnable}
        mask = 0
        for k, link in enumerate(dw.program.links):
            if int(link) in links:
                mask |= 1 << k
        dw.__dict__["_op_mask"] = (self._learnable_version, mask)
        return mask

    def _inverse_dynamics(self, q, qd, qdd, gravity: bool, damping: bool) -> torch.Tensor:
        dw = self._dynamics_walk()    # (the full walk whenever a link parameter is learnable)
        ops_f = self._ops_f(dw)
        needs_grad = torch.is_grad_enabled() and (ops_f.requires_grad or any(
            t is not None and t.requires_grad for t in (q, qd, qdd)))
        if needs_grad:
            self._differentiable(dw)
            return _InverseDynamics.apply(q, qd, qdd, ops_f, dw, gravity, damping, self._n_dofs,
                                          self._learnable_op_mask(dw))
        out = backend.rnea(dw.program, ops_f, dw.ops_i, q, qd, qdd, gravity, damping, self._n_dofs)
        have = self._fast_id
        if have is None or have[1]._ws_cache is not have[2]:
            self._fast_id = self._fast_entry("drm_rnea", "drm_rnea_scratch_floats_aligned", dw)
        return out

    def compute_lagrangian_inertia_matrix(self, q: torch.Tensor, include_gravity: Optional[bool] = True,
                                          use_damping: Optional[bool] = True) -> torch.Tensor:
        """H(q) [B, n, n] (robot_model.py:402-450) — see _compute_lagrangian_inertia_matrix; repeat calls of a constant model go
        through one prepared C++ call (csrc/drm_hostcall.cpp FastCall)."""
        ent = self._fast_crba
        if ent is not None and ent[1]._ws_cache is ent[2]:
            out = ent[0].inertia_matrix(q, self._stream_arg())
            if out.__class__ is torch.Tensor:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_lagrangian_inertia_matrix(q, include_gravity, use_damping)

    @tensor_check
    def _compute_lagrangian_inertia_matrix(self, q: torch.Tensor, include_gravity: Optional[bool] = True,
                                           use_damping: Optional[bool] = True) -> torch.Tensor:
        """Joint-space inertia matrix H(q) [B, n, n] (robot_model.py:402-450).

        The reference assembles H from n + 1 inverse-dynamics passes, column j = ID(q, 0, e_j) - ID(q, 0, 0);
        ``include_gravity`` / ``use_damping`` cancel out of that difference (gravity is subtracted, damping
        multiplies qd = 0) and are accepted for signature compatibility only.  One fused
        composite-rigid-body kernel here; differentiable with respect to q and the learnable link parameters
        (n passes of the RNEA backward kernel, one per column).
        """
        assert q.ndim == 2
        assert q.shape[1] == self._n_dofs
        self._require_device()
        dw = self._dynamics_walk()
        ops_f = self._ops_f(dw)
        if torch.is_grad_enabled() and (ops_f.requires_grad or q.requires_grad):
            self._differentiable(dw)
            return _MassMatrix.apply(q, ops_f, dw, self._n_dofs, self._learnable_op_mask(dw))
        out = backend.crba(dw.program, ops_f, dw.ops_i, q, self._n_dofs)
        have = self._fast_crba
        if have is None or have[1]._ws_cache is not have[2]:
            self._fast_crba = self._fast_entry("drm_crba", "drm_crba_scratch_floats_aligned", dw)
        return out

    def compute_forward_dynamics(self, q: torch.Tensor, qd: torch.Tensor, f: torch.Tensor,
                                 include_gravity: Optional[bool] = True, use_damping: Optional[bool] = False
                                 ) -> torch.Tensor:
        """qdd [B, n] (robot_model.py:487-624) — see _compute_forward_dynamics; repeat calls of a constant model go through one
        prepared C++ call (csrc/drm_hostcall.cpp FastCall)."""
        ent = self._fast_fd
        if ent is not None and ent[1]._ws_cache is ent[2]:
            out = ent[0].forward_dynamics(q, qd, f, (1 if include_gravity else 0) | (2 if use_damping else 0), self._stream_arg())
            if out.__class__ is torch.Tensor:
                return out
            if out is not None:
                backend._check(out, backend.library_for(self._device))
        return self._compute_forward_dynamics(q, qd, f, include_gravity, use_damping)

    @tensor_check
    def _compute_forward_dynamics(self, q: torch.Tensor, qd: torch.Tensor, f: torch.Tensor,
                                  include_gravity: Optional[bool] = True, use_damping: Optional[bool] = False
                                  ) -> torch.Tensor:
        """qdd [B,n] that the joint torques ``f`` produce in state (q, qd) (robot_model.py:487-624).

        One kernel launch: Featherstone's articulated-body recursion, as in the reference, for robots with a long
        segment (an arm carrying a gripper or a hand); for 7-DoF arms and for hands (short independent fingers) the same
        linear system H(q) qdd = f - nle(q, qd) formed and solved in registers (composite-rigid-body H, RNEA bias torques,
        leaf-to-root L^T D L elimination).
        With ``use_damping`` the reference subtracts damping * qd from its ``f`` argument IN PLACE
        (robot_model.py:515-521); here ``f`` is left untouched.  Differentiable with respect to q, qd, f and the
        learnable link parameters (implicit differentiation: one more solve + the RNEA backward kernel).
        """
        assert q.ndim == 2
        assert qd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        self._require_device()
        dw = self._dynamics_walk()
        ops_f = self._ops_f(dw)
        if torch.is_grad_enabled() and (ops_f.requires_grad or any(t.requires_grad for t in (q, qd, f))):
            self._differentiable(dw)
            return _ForwardDynamics.apply(q, qd, f, ops_f, dw, bool(include_gravity), bool(use_damping), self._n_dofs,
                                          self._learnable_op_mask(dw))
        out = backend.forward_dynamics(dw.program, ops_f, dw.ops_i, q, qd, f, bool(include_gravity),
                                       bool(use_damping), self._n_dofs)
        have = self._fast_fd
        if have is None or have[1]._ws_cache is not have[2]:
            self._fast_fd = self._fast_entry("drm_forward_dynamics", "drm_forward_dynamics_scratch_floats_aligned", dw)
        return out

    ROLLOUT_INTEGRATORS = ("semi_implicit_euler", "euler")

    def compute_forward_dynamics_rollout(self, q0: torch.Tensor, qd0: torch.Tensor, tau: torch.Tensor, dt: float,
                                         integrator: str = "semi_implicit_euler", include_gravity: Optional[bool] = True,
                                         use_damping: Optional[bool] = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(q_traj, qd_traj) [T, B, n]: the states after steps 1 .. T of a simulation from (q0, qd0) [B, n] under the joint torques
        tau [T, B, n] (TIME-MAJOR: step t's torques are the contiguous slab tau[t]).  Step t computes
        qdd_t = compute_forward_dynamics(q_t, qd_t, tau[t], include_gravity, use_damping), then
            "semi_implicit_euler" (default):   qd_{t+1} = qd_t + dt * qdd_t,  q_{t+1} = q_t + dt * qd_{t+1}
            "euler" (explicit):                q_{t+1} = q_t + dt * qd_t,     qd_{t+1} = qd_t + dt * qdd_t
        One launch for 7-DoF arms and hands (the state stays in registers across the steps, csrc/drm_rollout.hip), two per step for
        every other robot; ``tau`` is never modified.  Unbatched q0, qd0 [n] with tau [T, n] give [T, n].  Differentiable with respect
        to q0, qd0, tau and the learnable link parameters (one autograd node whose backward sweeps the steps in reverse); first order
        only: for second derivatives compose compute_forward_dynamics step by step."""
        if integrator not in self.ROLLOUT_INTEGRATORS:
            raise ValueError("integrator must be one of %s (got %r)" % (self.ROLLOUT_INTEGRATORS, integrator))
        for name, t in (("q0", q0), ("qd0", qd0), ("tau", tau)):
            assert type(t) is torch.Tensor, "%s must be a tensor" % name
            assert t.device.type == self._device.type, f"Input argument of different device as module: {t}"
        assert q0.ndim in [1, 2], "Input tensors must have ndim of 1 or 2."
        assert qd0.shape == q0.shape, "Batch size mismatch between input tensors."
        assert tau.ndim == q0.ndim + 1, "tau must be [T, B, n] ([T, n] for unbatched q0 / qd0)"
        assert tau.shape[1:-1] == q0.shape[:-1], "Batch size mismatch between input tensors."
        assert q0.shape[-1] == self._n_dofs and tau.shape[-1] == self._n_dofs
        dt = float(dt)
        if tau.shape[0] < 1:
            raise ValueError("a rollout takes at least one step (tau has T = 0)")
        if not (math.isfinite(dt) and dt > 0):
            raise ValueError("dt must be finite and positive (got %r)" % (dt,))
        single = q0.ndim == 1
        if single:
            q0, qd0, tau = q0.unsqueeze(0), qd0.unsqueeze(0), tau.unsqueeze(1)
        self._require_device()
        dw = self._dynamics_walk()
        ops_f = self._ops_f(dw)
        explicit = integrator == "euler"
        if torch.is_grad_enabled() and (ops_f.requires_grad or any(t.requires_grad for t in (q0, qd0, tau))):
            self._differentiable(dw)
            q_traj, qd_traj = _ForwardDynamicsRollout.apply(q0, qd0, tau, ops_f, dw, dt, bool(include_gravity), bool(use_damping),
                                                            explicit, self._n_dofs, self._learnable_op_mask(dw))
        else:
            q_traj, qd_traj, _ = backend.forward_dynamics_rollout(dw.program, ops_f, dw.ops_i, q0, qd0, tau, dt, bool(include_gravity),
                                                                  bool(use_damping), explicit, self._n_dofs)
        if single:
            return q_traj[:, 0], qd_traj[:, 0]
        return q_traj, qd_traj

    def _joint_bounds(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lower, upper) [n] float32 on the model device from get_joint_limits(): a DoF whose parsed limits have lower >= upper
        (a continuous joint, whose <limit> carries no lower / upper) is free, -inf / +inf.  Made once (no copy inside a captured
        graph)."""
        have = self.__dict__.get("_ik_bounds")
        if have is None:
            lo, hi = [], []
            for lim in self.get_joint_limits():
                a, b = float(lim["lower"]), float(lim["upper"])
                free = not a < b
                lo.append(-math.inf if free else a)
                hi.append(math.inf if free else b)
            have = self._ik_bounds = (torch.tensor(lo, dtype=torch.float32, device=self._device),
                                      torch.tensor(hi, dtype=torch.float32, device=self._device))
        return have

    def compute_inverse_kinematics(self, q0: torch.Tensor, link_name: str, target_pos: torch.Tensor,
                                   target_quat: Optional[torch.Tensor] = None, *, max_iterations: int = 32, damping: float = 0.01,
                                   step_size: float = 1.0, tol_pos: float = 1e-4, tol_rot: float = 1e-3,
                                   respect_joint_limits: bool = True, _composed: bool = False) -> InverseKinematicsResult:
        """Joint angles that put ``link_name`` at target_pos [B, 3] (and at target_quat [B, 4], xyzw as compute_forward_kinematics
        returns it; None: position only), by damped least squares from q0 [B, n].  Iteration i = 0 .. max_iterations evaluates
        (p, c, J) = compute_fk_and_jacobian(q_i, link_name) and the errors e_p = target_pos - p and e_R, the rotation vector of
        target (x) conj(c).  A row stops at q_i when |e_p| <= tol_pos and its rotation angle <= tol_rot, or at i = max_iterations;
        otherwise q_{i+1} = clamp(q_i + step_size * J^T (J J^T + damping^2 I)^-1 e) (J = [lin_jac; ang_jac], 6 x n; lin_jac alone,
        3 x n, in position-only mode) between the joint limits of get_joint_limits() (respect_joint_limits; a continuous joint
        is free).  One kernel launch per solve for 7-DoF arms (csrc/drm_ik.hip), two per iteration for every other robot, never a
        host synchronisation.  Unbatched q0 [n] with target_pos [3] give unbatched results.  A row whose q0 (in any DoF, one the
        link does not depend on included), target_pos or target_quat is not finite never reports convergence and changes no other row.

        The results carry NO autograd history, even when the inputs or the learnable link parameters require grad: the solve is
        not differentiable here.  A model with learnable links solves against their current values.  (``_composed``: every row takes
        the composed path, DRM_IK_COMPOSED; for tests and A/B measurements.)"""
        for name, t in (("q0", q0), ("target_pos", target_pos), ("target_quat", target_quat)):
            if t is None and name == "target_quat":
                continue
            if type(t) is not torch.Tensor:
                raise TypeError("%s must be a tensor" % name)
            if t.device.type != self._device.type:
                raise ValueError("%s is on %s, the model on %s" % (name, t.device, self._device))
            if not t.is_floating_point():
                raise TypeError("%s must be a floating-point tensor (got %s)" % (name, t.dtype))
        if q0.ndim not in (1, 2) or q0.shape[-1] != self._n_dofs:
            raise ValueError("q0 must be [B, %d] or [%d], got %s" % (self._n_dofs, self._n_dofs, tuple(q0.shape)))
        batch = q0.shape[:-1]
        if target_pos.shape != batch + (3,):
            raise ValueError("target_pos must be %s, got %s" % (tuple(batch + (3,)), tuple(target_pos.shape)))
        if target_quat is not None and target_quat.shape != batch + (4,):
            raise ValueError("target_quat must be %s, got %s" % (tuple(batch + (4,)), tuple(target_quat.shape)))
        if link_name not in self._name_to_idx_map:
            raise ValueError("unknown link %r" % (link_name,))
        idx = self._name_to_idx_map[link_name]
        if idx == 0:
            raise ValueError("%r is the root link: it does not move" % (link_name,))
        max_iterations = int(max_iterations)
        if max_iterations < 0:
            raise ValueError("max_iterations must be >= 0 (got %d)" % max_iterations)
        damping, step_size, tol_pos, tol_rot = float(damping), float(step_size), float(tol_pos), float(tol_rot)
        for name, v in (("damping", damping), ("step_size", step_size)):
            if not (math.isfinite(v) and v > 0):
                raise ValueError("%s must be finite and positive (got %r)" % (name, v))
        for name, v in (("tol_pos", tol_pos), ("tol_rot", tol_rot)):
            if not (math.isfinite(v) and v >= 0):
                raise ValueError("%s must be finite and >= 0 (got %r)" % (name, v))
        single = q0.ndim == 1
        if single:
            q0, target_pos = q0.unsqueeze(0), target_pos.unsqueeze(0)
            target_quat = target_quat.unsqueeze(0) if target_quat is not None else None
        self._require_device()
        with torch.no_grad():
            dw = self._get_walk(("chain", idx), targets=[idx]) if self._learnable else self._chain_walk(idx)
            ops_f = self._ops_f(dw).detach()
            lower, upper = self._joint_bounds() if respect_joint_limits else (None, None)
            q, err, iters = backend.inverse_kinematics(dw.program, ops_f, dw.ops_i, q0.detach(), target_pos.detach(),
                                                       target_quat.detach() if target_quat is not None else None, max_iterations,
                                                       damping, step_size, tol_pos, tol_rot, lower, upper, self._n_dofs,
                                                       composed=bool(_composed))
        pos_err = err[:, 0]
        rot_err = err[:, 1] if target_quat is not None else None
        # (the tolerances as the float32 values the kernel compared with)
        converged = pos_err <= float(np.float32(tol_pos))
        if rot_err is not None:
            converged = converged & (rot_err <= float(np.float32(tol_rot)))
        if single:
            q, pos_err, iters, converged = q[0], pos_err[0], iters[0], converged[0]
            rot_err = rot_err[0] if rot_err is not None else None
        return InverseKinematicsResult(q=q, pos_err=pos_err, rot_err=rot_err, iterations=iters, converged=converged)

    def compute_operational_space_dynamics(self, q: torch.Tensor, qd: torch.Tensor, link_name: str, *, include_gravity: bool = True,
                                           use_damping: bool = False, position_only: bool = False, regularization: float = 0.0,
                                           _composed: bool = False) -> OperationalSpaceDynamics:
        """The operational-space (task-space) dynamics of ``link_name`` at q, qd [B, n]: what a task-space controller needs every
        tick.  With H(q) qdd + nle(q, qd) = tau (nle = compute_non_linear_effects(q, qd, include_gravity, use_damping)),
        J = [lin_jac; ang_jac] of compute_endeffector_jacobian(q, link_name) (m = 6 rows; lin_jac alone, m = 3, with
        ``position_only``) and A = J H^-1 J^T + regularization^2 I:
            inertia        [B, m, m]  A^-1, symmetric
            jacobian_pinv  [B, n, m]  H^-1 J^T inertia, the dynamically consistent inverse of J
            bias_acc       [B, m]     Jdot qd = d/dt J(q + t qd)|t=0 qd: the world-frame classical acceleration of the link origin
                                      (rows 0-2) and its angular acceleration (rows 3-5) at qdd = 0, gravity absent
            bias_force     [B, m]     inertia (J H^-1 nle - Jdot qd)
        so that tau = J^T (inertia a + bias_force) produces the link acceleration a when regularization = 0.  One kernel launch for
        a 7-DoF arm whose last link is the target (csrc/drm_osc.hip: one pass over q, no intermediate in HBM); the Jacobian, inertia
        matrix and bias-torque kernels followed by a one-lane-per-row finish kernel for every other robot or link.  Unbatched q, qd
        [n] give unbatched results.

        At a SINGULAR configuration (J without full row rank: a stretched arm, or more task rows than the chain has joints) with
        ``regularization=0`` A has no inverse: inertia — and with it jacobian_pinv and bias_force — is huge or non-finite on that
        row only; no other row changes and nothing faults.  A positive ``regularization`` bounds |inertia| by 1 / regularization^2.
        A row whose q or qd is not finite returns non-finite values and changes no other row.

        The results carry NO autograd history, even when the inputs or the learnable link parameters require grad.  A model with
        learnable links uses their current values.  (``_composed``: every row takes the composed path, DRM_OSC_COMPOSED; for tests
        and A/B measurements.)"""
        for name, t in (("q", q), ("qd", qd)):
            if type(t) is not torch.Tensor:
                raise TypeError("%s must be a tensor" % name)
            if t.device.type != self._device.type:
                raise ValueError("%s is on %s, the model on %s" % (name, t.device, self._device))
            if not t.is_floating_point():
                raise TypeError("%s must be a floating-point tensor (got %s)" % (name, t.dtype))
        if q.ndim not in (1, 2) or q.shape[-1] != self._n_dofs:
            raise ValueError("q must be [B, %d] or [%d], got %s" % (self._n_dofs, self._n_dofs, tuple(q.shape)))
        if qd.shape != q.shape:
            raise ValueError("qd must be %s like q, got %s" % (tuple(q.shape), tuple(qd.shape)))
        if link_name not in self._name_to_idx_map:
            raise ValueError("unknown link %r" % (link_name,))
        idx = self._name_to_idx_map[link_name]
        if idx == 0:
            raise ValueError("%r is the root link: it does not move" % (link_name,))
        regularization = float(regularization)
        if not (math.isfinite(regularization) and regularization >= 0):
            raise ValueError("regularization must be finite and >= 0 (got %r)" % (regularization,))
        single = q.ndim == 1
        if single:
            q, qd = q.unsqueeze(0), qd.unsqueeze(0)
        self._require_device()
        with torch.no_grad():
            tree = self._dynamics_walk()
            chain = self._get_walk(("chain", idx) + (("folded", tree.fold_key) if tree.folded else ()), targets=[idx],
                                   folded=tree.folded, fold_key=tree.fold_key)
            out = backend.operational_space((tree.program, self._ops_f(tree).detach(), tree.ops_i),
                                            (chain.program, self._ops_f(chain).detach(), chain.ops_i), q.detach(), qd.detach(),
                                            bool(include_gravity), bool(use_damping), bool(position_only), regularization,
                                            self._n_dofs, composed=bool(_composed))
        if single:
            out = tuple(t[0] for t in out)
        return OperationalSpaceDynamics(*out)

    def compute_forward_dynamics_derivatives(self, q: torch.Tensor, qd: torch.Tensor, f: torch.Tensor,
                                             include_gravity: Optional[bool] = True, use_damping: Optional[bool] = False, *,
                                             _composed: bool = False) -> ForwardDynamicsDerivatives:
        """Forward dynamics and its linearisation about the state (q, qd) and the torques f [B, n]: what iLQR / DDP, LQR, linearised
        MPC and an EKF need at every knot.  With ID(q, qd, qdd) = H(q) qdd + nle(q, qd) the inverse dynamics (the damping torques
        inside when ``use_damping``):
            qdd       [B, n]     compute_forward_dynamics(q, qd, f, include_gravity, use_damping)
            dqdd_dq   [B, n, n]  [b, i, j] = d qdd_i / d q_j  = -(H^-1 dID/dq)[i, j] at (q, qd, qdd)
            dqdd_dqd  [B, n, n]  [b, i, j] = d qdd_i / d qd_j = -(H^-1 dID/dqd)[i, j]
            minv      [B, n, n]  H(q)^-1 = d qdd / d f, symmetric
        so that A = [dqdd_dq, dqdd_dqd] and B = minv linearise the continuous dynamics.  One kernel launch for a 7-DoF arm
        (csrc/drm_fdd.hip: one pass over q, one factorisation of H, n reverse sweeps of RNEA for the rows of dID/dq and dID/dqd, 3 n
        solves, no intermediate in HBM; qdd from the forward-dynamics kernel itself when the robot's own kernels are attached); for every
        other robot the forward-dynamics and inertia-matrix kernels, n launches of the RNEA
        backward kernel and a one-lane-per-row kernel that inverts and solves, all out of one scratch allocation.  Argument handling is that of
        compute_forward_dynamics (unbatched inputs give unbatched results); ``f`` is never modified.  A row whose q, qd or f is not
        finite returns non-finite values and changes no other row.  Robots whose trees the backward kernels do not take (more than
        64 links or 6 open branch points) are refused as a gradient of compute_forward_dynamics would be.

        The results carry NO autograd history, even when the inputs or the learnable link parameters require grad.  A model with
        learnable links uses their current values.  (``_composed``, or DRM_FDD_COMPOSED=1 in the environment: every row takes the
        composed path, DRM_FDD_COMPOSED; for tests and A/B measurements.)"""
        return ForwardDynamicsDerivatives(*self._compute_forward_dynamics_derivatives(q, qd, f, include_gravity, use_damping,
                                                                                      bool(_composed)))

    @tensor_check
    def _compute_forward_dynamics_derivatives(self, q, qd, f, include_gravity, use_damping, composed):
        assert q.ndim == 2
        assert qd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            self._differentiable(dw)
            return backend.forward_dynamics_derivatives(dw.program, self._ops_f(dw).detach(), dw.ops_i, q.detach(), qd.detach(),
                                                        f.detach(), bool(include_gravity), bool(use_damping), self._n_dofs,
                                                        composed=composed)

    def compute_inverse_dynamics_regressor(self, q: torch.Tensor, qd: torch.Tensor, qdd: torch.Tensor,
                                           include_gravity: Optional[bool] = True, use_damping: Optional[bool] = False, *,
                                           _composed: bool = False) -> torch.Tensor:
        """The inverse-dynamics regressor Y [B, n, P] at q, qd, qdd [B, n]: inverse dynamics is linear in the inertial parameters,
            compute_inverse_dynamics(q, qd, qdd, include_gravity, use_damping) = Y @ inertial_parameters(use_damping)
        up to float32 rounding.  P = 10 per body of regressor_links(), in that order, each block multiplying
            [m, m c_x, m c_y, m c_z, Ixx, Ixy, Ixz, Iyy, Iyz, Izz]
        of the body: c and I in the link's own URDF frame, I about the frame's origin, an off-diagonal column the coefficient of the
        tied pair Ixy = Iyx.  With ``use_damping`` n more columns follow, Y[b, j, 10 Nb + j] = qd_j: the joint dampings in DoF order.
        Y[b, j, block i] is zero where body i is not in the sub-tree of joint j.  What closed-form and recursive least-squares
        identification, adaptive control and excitation-trajectory design need per sample.

        One kernel launch (csrc/drm_regressor.hip): a 7-DoF arm's full 64-row tiles in a kernel that keeps the blocks in registers
        and stores every tile of Y whole; every other robot a memset of Y and one lane per row with a loop over the bodies.  Argument handling is that of compute_inverse_dynamics
        (unbatched inputs give an unbatched [n, P]); works for models on the CPU and on a HIP device, and for models with learnable
        links: their current values are used — Y depends on the kinematic ones — and the links kept for them are bodies of their own.
        A row whose q, qd or qdd is not finite has non-finite entries and changes no other row.

        The result is computed WITHOUT building an autograd graph and is returned detached, whatever requires grad.  (``_composed``:
        every row takes the general kernel, DRM_REGRESSOR_COMPOSED; for tests and A/B.)"""
        return self._compute_inverse_dynamics_regressor(q, qd, qdd, include_gravity, use_damping, bool(_composed))

    @tensor_check
    def _compute_inverse_dynamics_regressor(self, q, qd, qdd, include_gravity, use_damping, composed):
        assert q.ndim == 2
        assert qd.ndim == 2
        assert qdd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        assert qdd.shape[1] == self._n_dofs
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            return backend.rnea_regressor(dw.program, self._ops_f(dw).detach(), dw.ops_i, q.detach(), qd.detach(), qdd.detach(),
                                          bool(include_gravity), bool(use_damping), self._n_dofs, composed=composed)

    def compute_lagrangian_dynamics(self, q: torch.Tensor, qd: torch.Tensor, *, _composed: bool = False) -> LagrangianDynamics:
        """The terms of the equations of motion  H(q) qdd + C(q, qd) qd + g(q) = tau  at q, qd [B, n], separately:
            inertia   [B, n, n]  compute_lagrangian_inertia_matrix(q), up to float32 rounding; symmetric to the bit
            coriolis  [B, n, n]  the Christoffel matrix, C[i, j] = sum_k Gamma_ijk qd_k with
                                 Gamma_ijk = (dH_ij/dq_k + dH_ik/dq_j - dH_jk/dq_i) / 2
            gravity   [B, n]     compute_inverse_dynamics(q, 0, 0, include_gravity=True, use_damping=False)
        so that C qd + g = compute_non_linear_effects(q, qd, True, False) and dH/dt = C + C^T: dH/dt - 2 C is skew-symmetric, which
        passivity-based and adaptive controllers (tau = H a + C v + g - K s with v != qd) rely on, as generalised-momentum observers
        do on pdot = tau + C^T qd - g + tau_ext with p = H qd.  The product C qd does not determine C; this is the one choice with
        those properties.  Joint damping is NOT part of C:  tau = H qdd + C qd + g + damping * qd.  H[i, j] and C[i, j] are exactly
        zero where joints i and j lie on different branches.

        One kernel launch (csrc/drm_lagrangian.hip): one sweep out and one back over the tree instead of dH/dq by n (n + 1) / 2
        backward passes through the inertia matrix.  A 7-DoF arm's full 64-row tiles run a kernel that keeps everything in registers and stores
        the tiles of H, C and g whole; every other robot one lane per row over the ops of its walk.  With the robot's own
        constant-folded kernels attached this entry point still runs the library kernels.  Argument handling is that of
        compute_forward_dynamics_derivatives (unbatched inputs give unbatched results); works for models on the CPU and on a HIP
        device, with either joint model (reference_compat) and for models with learnable links: their current values are used.
        A row whose q or qd is not finite — or whose |q| is beyond 1e5, where float32 no longer resolves an angle — returns NaN
        and changes no bit of any other row.

        The results carry NO autograd history, whatever requires grad.  (``_composed``, or DRM_LAGRANGIAN_COMPOSED=1 in the
        environment: every row takes the general kernel, DRM_LAGRANGIAN_COMPOSED; for tests and A/B measurements.)"""
        return LagrangianDynamics(*self._compute_lagrangian_dynamics(q, qd, False, bool(_composed)))

    def compute_coriolis_matrix(self, q: torch.Tensor, qd: torch.Tensor) -> torch.Tensor:
        """compute_lagrangian_dynamics(q, qd).coriolis [B, n, n] alone, to the bit: the same launch with the other two outputs
        neither formed (7-DoF arms) nor written."""
        return self._compute_lagrangian_dynamics(q, qd, True, False)[1]

    @tensor_check
    def _compute_lagrangian_dynamics(self, q, qd, coriolis_only, composed):
        assert q.ndim == 2
        assert qd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        assert q.shape[0] == qd.shape[0]
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            return backend.lagrangian_dynamics(dw.program, self._ops_f(dw).detach(), dw.ops_i, q.detach(), qd.detach(), self._n_dofs,
                                               coriolis_only=coriolis_only, composed=composed)

    def compute_energy_derivatives(self, q: torch.Tensor, qd: torch.Tensor, *, _composed: bool = False) -> EnergyDerivatives:
        """The Lagrangian L = T - V and the Hamiltonian T + V of the robot at q, qd [B, n], with their first derivatives:
            kinetic      [B]     T = 1/2 qd^T H(q) qd, summed over the bodies as 1/2 v_i . (I_i v_i) in each link's own frame (H is
                                 never formed); >= 0, and exactly 0 where qd = 0
            potential    [B]     V = 9.81 sum_i m_i z_i, z_i the height of body i's centre of mass above the base frame's z = 0
                                 plane, over the bodies of regressor_links().  Links that no joint moves — the base and whatever is
                                 fixed to it — are LEFT OUT: they add a constant to V and nothing to the other four.
            momentum     [B, n]  p = dT/dqd = H(q) qd, the generalised momentum
            dkinetic_dq  [B, n]  dT/dq_j = 1/2 qd^T (dH/dq_j) qd = (C^T qd)_j with compute_coriolis_matrix's C
            gravity      [B, n]  dV/dq = compute_lagrangian_dynamics(q, qd).gravity, up to float32 rounding
        so that Lagrange's equations read pdot = tau + dkinetic_dq - gravity and Hamilton's qdot = dHam/dp, pdot = -dHam/dq + tau
        with dHam/dq = gravity - dkinetic_dq at fixed p.  Joint damping enters none of them.  What energy-shaping and swing-up
        controllers, symplectic integrators, Lagrangian / Hamiltonian network losses and an energy-drift check of a rollout need.

        One kernel launch (csrc/drm_energy.hip): one sweep out and one back over the tree, lighter than inverse dynamics — 56 B in
        and 92 B out per row of a 7-DoF arm instead of the 420 B of compute_lagrangian_dynamics, two products, all-links forward
        kinematics and a loop over the masses.  A 7-DoF arm's full 64-row tiles run a kernel that keeps everything in registers;
        every other robot one lane per row over the ops of its walk.  With the robot's own constant-folded kernels attached this
        entry point still runs the library kernels.  Argument handling is that of compute_lagrangian_dynamics (unbatched inputs give
        unbatched results); works for models on the CPU and on a HIP device, with either joint model (reference_compat) and for
        models with learnable links: their current values are used.  A row whose q or qd is not finite — or whose |q| is beyond
        1e5, where float32 no longer resolves an angle — returns NaN in all five and changes no bit of any other row.

        The results carry NO autograd history, whatever requires grad (compute_energy is the differentiable form).  (``_composed``,
        or DRM_ENERGY_COMPOSED=1 in the environment: every row takes the general kernel, DRM_ENERGY_COMPOSED; for tests and A/B
        measurements.)"""
        return EnergyDerivatives(*self._compute_energy(q, qd, backend.ENERGY_OUTPUTS, bool(_composed)))

    def compute_generalized_momentum(self, q: torch.Tensor, qd: torch.Tensor) -> torch.Tensor:
        """compute_energy_derivatives(q, qd).momentum [B, n] alone, to the bit: the same launch with only p requested."""
        return self._compute_energy(q, qd, ("momentum",), False)[2]

    def compute_energy(self, q: torch.Tensor, qd: torch.Tensor) -> Energy:
        """(kinetic [B], potential [B]) of compute_energy_derivatives, to the bit, from the same launch — and DIFFERENTIABLE with
        respect to q and qd: one autograd node (autograd._Energy) whose forward asks the launch for all five outputs and keeps the
        three vectors, and whose backward is
            grad_q = gT[:, None] * dkinetic_dq + gV[:, None] * gravity,      grad_qd = gT[:, None] * momentum.
        FIRST order only: the node is once_differentiable, a second backward through it raises.  When neither q nor qd requires
        grad (or grad mode is off) only T and V are requested and the sweep back is not made.  No history flows to learnable link
        parameters: their current values are used, as by compute_energy_derivatives."""
        return Energy(*self._compute_energy_differentiable(q, qd))

    @tensor_check
    def _compute_energy(self, q, qd, want, composed):
        assert q.ndim == 2
        assert qd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        assert q.shape[0] == qd.shape[0]
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            return backend.energy(dw.program, self._ops_f(dw).detach(), dw.ops_i, q.detach(), qd.detach(), self._n_dofs, want=want,
                                  composed=composed)

    @tensor_check
    def _compute_energy_differentiable(self, q, qd):
        assert q.ndim == 2
        assert qd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        assert q.shape[0] == qd.shape[0]
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            ops_f = self._ops_f(dw).detach()
        if torch.is_grad_enabled() and (q.requires_grad or qd.requires_grad):
            return _Energy.apply(q, qd, dw.program, ops_f, dw.ops_i, self._n_dofs)
        with torch.no_grad():
            return backend.energy(dw.program, ops_f, dw.ops_i, q.detach(), qd.detach(), self._n_dofs, want=("kinetic", "potential"))[:2]

    # ------------------------------------------------------------------ the robot as a whole
    def _moved_links(self) -> np.ndarray:
        """bool [L]: at least one moving joint on the way from the root to the link."""
        have = self.__dict__.get("_moved_mask")
        if have is None:
            spec = self._spec
            have = self.__dict__["_moved_mask"] = np.array([any(spec.dof[j] >= 0 for j in spec.chain_to(i)) for i in range(spec.n_links)])
        return have

    def _base_share(self):
        """(mass, (mc_x, mc_y, mc_z)) of the links no joint moves — the base and whatever is fixed to it — in the base frame: fp64 on
        the host from the constant link table, the fixed transforms composed as flatten.fold_link_table composes them.  Once per set
        of learnable parameters; a learnable mass, com, trans or rot_angles on one of these links is refused."""
        have = self.__dict__.get("_base_share_cache")
        if have is not None and have[0] == self._learnable_version:
            return have[1]
        spec, moved = self._spec, self._moved_links()
        for link, name in self._learnable:
            if not moved[link] and name in ("mass", "com", "trans", "rot_angles"):
                raise NotImplementedError("%s of %s is learnable and the link belongs to the base share (no joint moves it): "
                                          "pass include_base=False" % (name, spec.link_names[link]))
        if self._static_table is None:
            self._link_table()
        rows = self._static_table[:spec.n_links].detach().cpu().numpy().astype(np.float64)
        F, t = rows[:, 0:9].reshape(-1, 3, 3), rows[:, 9:12]      # (the link table's rows: F row-major, then t; flatten.OPF_F / OPF_T)
        R, p = [None] * spec.n_links, [None] * spec.n_links
        mass, mc = 0.0, np.zeros(3)
        for i in range(spec.n_links):      # children come after their parents in URDF <link> order
            if moved[i]:
                continue
            par = int(spec.parent[i])
            Rp, pp = (np.eye(3), np.zeros(3)) if par < 0 else (R[par], p[par])
            R[i], p[i] = Rp @ F[i], Rp @ t[i] + pp
            mass += rows[i, OPF_MASS]
            mc += R[i] @ rows[i, OPF_MCOM:OPF_MCOM + 3] + rows[i, OPF_MASS] * p[i]
        share = (float(mass), tuple(float(x) for x in mc))
        self.__dict__["_base_share_cache"] = (self._learnable_version, share)
        return share

    def total_mass(self, include_base: bool = True):
        """M = sum of the link masses: over every link, or with ``include_base=False`` over the links that a joint moves.  A Python
        float for a constant model; for a model with learnable links a detached 0-dim tensor of their current values."""
        moved = self._moved_links()
        base = self._base_share()[0] if include_base else 0.0
        if not self._learnable:
            have = self.__dict__.setdefault("_total_mass_cache", {})      # (a constant model: once, not a device read per call)
            if bool(include_base) not in have:
                if self._static_table is None:
                    self._link_table()
                m = self._static_table[:self._spec.n_links, OPF_MASS].detach().cpu().numpy().astype(np.float64)
                have[bool(include_base)] = float((m * moved).sum() + base)
            return have[bool(include_base)]
        with torch.no_grad():
            m = self._link_table()[:self._spec.n_links, OPF_MASS].detach().to(torch.float64)
            return ((m * torch.from_numpy(moved).to(m.device)).sum() + base).to(torch.float32)

    def _whole_body_mass(self, include_base: bool):
        """total_mass, refused where it is zero (a constant model; a learnable model's lives on the device and is not read back: its
        rows come out NaN)"""
        mass = self.total_mass(include_base)
        if not self._learnable and not mass > 0.0:
            raise ValueError("the robot's total mass is zero: it has no centre of mass")
        return mass

    def compute_center_of_mass(self, q: torch.Tensor, qd: Optional[torch.Tensor] = None, qdd: Optional[torch.Tensor] = None, *,
                               jacobian: bool = False, include_base: bool = True, _composed: bool = False) -> CenterOfMass:
        """Where the robot's centre of mass is and how it moves, at q [B, n] (qd, qdd [B, n] optional), in base axes (z up):
            mass              M = total_mass(include_base)
            position          [B, 3]     sum m_i c_i / M over the links (c_i the world position of link i's centre of mass)
            velocity          [B, 3]     jacobian qd; the linear momentum is M velocity.  None without qd.
            acceleration      [B, 3]     d/dt velocity, gravity not included; needs qd.  None without qdd.
            jacobian          [B, 3, n]  d position / d q.  jacobian^T (0, 0, M g) = compute_energy_derivatives(q, qd).gravity.
                                         None unless ``jacobian=True``.
            angular_momentum  [B, 3]     sum (c_i x m_i v_ci + I_i w_i): about the base ORIGIN.  About the centre of mass it is
                                         angular_momentum - position x M velocity.  None without qd.
        The links that no joint moves — the base and whatever is fixed to it — enter ``mass`` and ``position`` as a constant (the
        base share); ``include_base=False`` leaves them out of both.

        One kernel launch (csrc/drm_whole_body.hip; two with a ragged tail): one sweep out and one back over the tree that keeps what
        inverse dynamics and compute_energy_derivatives carry to the root and drop there.  Only the levels the requested outputs need
        are computed.  A 7-DoF arm's full 64-row tiles run a kernel that keeps everything in registers; every other robot one lane
        per row over the ops of its walk.  Argument handling is that of compute_energy_derivatives (unbatched inputs give unbatched
        results); works for models on the CPU and on a HIP device, with either joint model and for models with learnable links:
        their current values are used, ``mass`` is then a detached 0-dim tensor, and a learnable mass, com, trans or rot_angles on a
        link of the base share raises NotImplementedError with ``include_base=True``.  A row whose q / qd / qdd is not finite — or
        whose |q| is beyond 1e5 — returns NaN in every field and changes no bit of any other row.

        ``position`` is differentiable with respect to q and ``velocity`` with respect to qd, FIRST order only, through one autograd
        node whose backward launches the same call for the Jacobian and contracts it with the cotangent; a second backward raises.
        The q-gradient of ``velocity`` is not formed.  ``acceleration``, ``jacobian`` and ``angular_momentum`` carry NO autograd
        history, whatever requires grad, and no history flows to learnable link parameters.  (``_composed``, or
        DRM_WHOLE_BODY_COMPOSED=1 in the environment: every row takes the general kernel; for tests and A/B measurements.)"""
        if qdd is not None and qd is None:
            raise ValueError("the acceleration of the centre of mass needs qd")
        mass = self._whole_body_mass(include_base)
        want = ["com"] + (["com_vel", "ang_mom"] if qd is not None else []) + (["com_acc"] if qdd is not None else []) + \
            (["com_jac"] if jacobian else [])
        base = self._base_share() if include_base else None
        com, vel, acc, jac, ang, _, _ = self._compute_whole_body(q, qd, qdd, tuple(want), base, True, bool(_composed), True)
        return CenterOfMass(mass, com, vel, acc, jac, ang)

    def compute_base_wrench(self, q: torch.Tensor, qd: Optional[torch.Tensor] = None, qdd: Optional[torch.Tensor] = None, *,
                            include_gravity: bool = True, include_base: bool = True, _composed: bool = False) -> BaseWrench:
        """The wrench the mount applies to the base link — at the base origin, in base axes — that keeps the base at rest while the
        robot moves through (q, qd, qdd) [B, n]: the root wrench that inverse dynamics carries down the tree and drops.
            force   [B, 3]  sum m_i a_ci + M g e_z
            moment  [B, 3]  sum (c_i x m_i a_ci + I_i al_i + w_i x I_i w_i) + (sum m_i c_i) x g e_z
        qd / qdd None: zero; with both None it is the static wrench.  ``include_gravity=False`` drops the two weight terms;
        ``include_base=False`` leaves the weight of the links that no joint moves out of them.  Joint damping does not enter.  The
        wrench the robot applies to its mount is the negative; the zero-moment point on the plane z = 0 is
        (-moment_y / force_z, moment_x / force_z) — what a force plate or a base force/torque sensor reads, and what tip-over
        margins of a mobile manipulator are computed from.

        One launch, batching, devices, learnable links and non-finite rows as for compute_center_of_mass.  The results carry NO
        autograd history, whatever requires grad."""
        self._whole_body_mass(include_base)
        base = self._base_share() if include_base else None
        outs = self._compute_whole_body(q, qd, qdd, ("force", "moment"), base, bool(include_gravity), bool(_composed), False)
        return BaseWrench(outs[5], outs[6])

    @tensor_check
    def _compute_whole_body(self, q, qd, qdd, want, base, gravity, composed, differentiable):
        assert q.ndim == 2
        assert q.shape[1] == self._n_dofs
        for t in (qd, qdd):
            assert t is None or (t.ndim == 2 and t.shape == q.shape)
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            ops_f = self._ops_f(dw).detach()
        if differentiable and torch.is_grad_enabled() and (q.requires_grad or (qd is not None and qd.requires_grad)):
            return _CenterOfMass.apply(q, qd, qdd, dw.program, ops_f, dw.ops_i, self._n_dofs, want, base, composed)
        with torch.no_grad():
            return backend.whole_body(dw.program, ops_f, dw.ops_i, q.detach(), qd.detach() if qd is not None else None,
                                      qdd.detach() if qdd is not None else None, self._n_dofs, want, base_share=base,
                                      include_gravity=gravity, composed=composed)

    # ------------------------------------------------------------------ link motion and external wrenches
    def _links_plan(self, link_names):
        """(walk of the distinct non-root links in pre-order, T, sel, identity) for a list of link names (None: every link, root
        included): ``sel`` [L] maps the caller's position to the walk's output slot, T for the root (a column of zeros that the
        gather appends, a wrench that the scatter drops); ``identity``: the caller's order IS the walk's, nothing to move."""
        key = None if link_names is None else tuple(link_names)
        plans = self.__dict__.setdefault("_links_plans", {})
        plan = plans.get(key)
        if plan is None:
            names = self.get_link_names() if link_names is None else list(link_names)
            idxs = [self._name_to_idx_map[name] for name in names]
            wanted = set(i for i in idxs if i != 0)
            ordered = [i for i in self._spec.preorder() if i in wanted]
            if not ordered:
                raise ValueError("link_names must name at least one link besides the root")
            slot = {i: t for t, i in enumerate(ordered)}
            sel = [slot.get(i, len(ordered)) for i in idxs]
            plan = plans[key] = (tuple(ordered), len(ordered), torch.tensor(sel, dtype=torch.int64, device=self._device),
                                 sel == list(range(len(ordered))))
        ordered, T, sel, identity = plan
        return self._get_walk(("fk", ordered), targets=list(ordered)), T, sel, identity

    @staticmethod
    def _links_gather(x, sel, identity):
        """[B, T, 3] in walk order -> [B, L, 3] in the caller's order (zeros for the root)"""
        if x is None or identity:
            return x
        return torch.cat([x, x.new_zeros(x.shape[0], 1, 3)], dim=1).index_select(1, sel)

    @staticmethod
    def _links_scatter(x, sel, T, identity):
        """[B, L, 3] in the caller's order -> [B, T, 3] in walk order (repeats add up, the root's entry is dropped)"""
        if x is None or identity:
            return x
        return x.new_zeros(x.shape[0], T + 1, 3).index_add_(1, sel, x)[:, :T]

    def _links_args(self, q, others, trailing):
        """The argument handling of tensor_check for tensors whose trailing shape is not [n]: ``others`` are (tensor or None, name)
        with trailing shape ``trailing`` after q's batch shape.  Returns (unbatched, q [B, n], others batched)."""
        tensors = [(q, "q")] + [(t, name) for t, name in others if t is not None]
        for t, name in tensors:
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a tensor" % name)
            assert t.device.type == self._device.type, f"Input argument of different device as module: {name}"
        assert q.ndim in [1, 2], "Input tensors must have ndim of 1 or 2."
        unbatched = q.ndim == 1
        batch = tuple(q.shape[:-1])
        assert q.shape[-1] == self._n_dofs
        out = []
        for t, name in others:
            if t is not None:
                assert tuple(t.shape) == batch + tuple(trailing), "%s must be %s, got %s" % (name, batch + tuple(trailing), tuple(t.shape))
                t = t.unsqueeze(0) if unbatched else t
            out.append(t)
        return unbatched, (q.unsqueeze(0) if unbatched else q), out

    def _refuse_grad_q(self, q, what):
        if torch.is_grad_enabled() and q.requires_grad:
            raise ValueError("%s has no gradient with respect to q (it needs the kinematic Hessian, which is out of scope): "
                             "pass q.detach()" % what)

    def compute_link_motion(self, q: torch.Tensor, qd: torch.Tensor, qdd: Optional[torch.Tensor] = None,
                            link_names: Optional[List[str]] = None, *, _composed: bool = False) -> LinkMotion:
        """Position, velocity and classical acceleration of the named links (None: every link in get_link_names() order, the root
        included) at q, qd, qdd [B, n], in the frame of compute_endeffector_jacobian — WORLD axes, at the link frame's origin.  With
        lin_jac_l, ang_jac_l that method's outputs for link l:
            position              [B, L, 3]  the link origin (compute_forward_kinematics' position up to float32 rounding)
            linear_velocity       [B, L, 3]  lin_jac_l qd
            angular_velocity      [B, L, 3]  ang_jac_l qd
            linear_acceleration   [B, L, 3]  d/dt linear_velocity = lin_jac_l qdd + d(lin_jac_l)/dt qd: the classical acceleration of
                                             the origin, what an accelerometer there reads once gravity is added (it is NOT included)
                                             and the bias term of a contact constraint; None when qdd is None
            angular_acceleration  [B, L, 3]  d/dt angular_velocity; None when qdd is None
        ``link_names`` may be any list: any order, repeats, the root (which gets zeros).  Link orientation is
        compute_forward_kinematics_links'; body-frame outputs are out of scope.

        ONE kernel launch (csrc/drm_links.hip drm_link_motion): a world-frame sweep outwards over the many-target walk of the distinct
        non-root links, instead of one compute_endeffector_jacobian launch and two einsums per link.  All 8 links of a 7-DoF arm: a
        kernel that keeps everything in registers on full 64-row tiles; every other robot and link set one lane per row over the ops.
        Together with compute_external_torques it enters the existing entry points exactly, by linearity:
            tau = compute_inverse_dynamics(q, qd, qdd) - tau_ext          qdd = compute_forward_dynamics(q, qd, f + tau_ext).
        Argument handling is that of the neighbours (unbatched inputs give unbatched results); works on the CPU and on a HIP device,
        with either joint model and for models with learnable links (their current values are used).  A row whose q, qd or qdd is
        not finite, or whose |q| is beyond 1e5, returns NaN in every output and changes no bit of any other row.  The results carry
        NO autograd history (compute_link_velocities is differentiable in qd).  (``_composed``, or DRM_LINKS_COMPOSED=1 in the
        environment: every row takes the general kernel; for tests and A/B measurements.)"""
        unbatched, q, (qd, qdd) = self._links_args(q, [(qd, "qd"), (qdd, "qdd")], (self._n_dofs,))
        assert qd is not None, "qd must be given"
        self._require_device()
        with torch.no_grad():
            dw, T, sel, identity = self._links_plan(link_names)
            want = backend.LINK_MOTION_OUTPUTS[:3 if qdd is None else 5]
            outs = backend.link_motion(dw.program, self._ops_f(dw).detach(), dw.ops_i, q.detach(), qd.detach(),
                                       None if qdd is None else qdd.detach(), T, self._n_dofs, want=want, composed=bool(_composed))
            outs = [self._links_gather(x, sel, identity) for x in outs]
        return LinkMotion(*[x[0] if (unbatched and x is not None) else x for x in outs])

    def compute_link_velocities(self, q: torch.Tensor, qd: torch.Tensor, link_names: Optional[List[str]] = None, *,
                                differentiable_q: bool = False, _composed: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(linear_velocity, angular_velocity) [B, L, 3] of compute_link_motion(q, qd, link_names=link_names), to the bit, from the same
        launch with the two velocity arrays alone requested — and DIFFERENTIABLE once with respect to qd: the backward is the
        compute_external_torques launch with (forces, torques) := (grad_linear, grad_angular) (autograd._LinkAdjoint; a second backward
        raises).  By default there is NO gradient with respect to q: with grad mode on a q that requires grad raises ValueError; pass
        q.detach().  ``differentiable_q=True`` opts in: q may require grad, the forward values are the same bits, and the backward is ONE
        drm_link_power_dq launch — grad_q = d/dq [sum_l g_lin_l . v_l + g_ang_l . w_l] at fixed qd, and grad_qd from the same launch
        when qd needs one too (compute_link_power_gradient is that launch without autograd).  Still first order only."""
        unbatched, q, (qd,) = self._links_args(q, [(qd, "qd")], (self._n_dofs,))
        assert qd is not None, "qd must be given"
        if not differentiable_q:
            self._refuse_grad_q(q, "compute_link_velocities")
        self._require_device()
        with torch.no_grad():
            dw, T, sel, identity = self._links_plan(link_names)
            ops_f = self._ops_f(dw).detach()
        if torch.is_grad_enabled() and (qd.requires_grad or (differentiable_q and q.requires_grad)):
            lin, ang = _LinkAdjoint.apply(False, q if differentiable_q else q.detach(), qd, None, dw.program, ops_f, dw.ops_i, T,
                                          self._n_dofs, bool(_composed), bool(differentiable_q))
        else:
            with torch.no_grad():
                out = backend.link_motion(dw.program, ops_f, dw.ops_i, q.detach(), qd.detach(), None, T, self._n_dofs,
                                          want=("linear_velocity", "angular_velocity"), composed=bool(_composed))
            lin, ang = out[1], out[2]
        lin, ang = self._links_gather(lin, sel, identity), self._links_gather(ang, sel, identity)
        return (lin[0], ang[0]) if unbatched else (lin, ang)

    def compute_external_torques(self, q: torch.Tensor, forces: Optional[torch.Tensor], torques: Optional[torch.Tensor] = None,
                                 link_names: Optional[List[str]] = None, *, differentiable_q: bool = False,
                                 _composed: bool = False) -> torch.Tensor:
        """tau_ext [B, n] = sum_l lin_jac_l^T forces[:, l] + ang_jac_l^T torques[:, l]: the joint torques of external wrenches on the
        named links (None: every link in get_link_names() order) — contact forces, a payload, a wrist force/torque reading — with
        lin_jac_l, ang_jac_l compute_endeffector_jacobian's outputs for link l.  ``forces`` / ``torques`` [B, L, 3] are in WORLD axes
        and a force acts at the link frame's ORIGIN; a force at another point is the caller's torques += r x f.  Either may be None
        (zero), not both.  ``link_names`` may be any list: repeats add up, a wrench on the root is ignored.  Columns of joints that no
        named link's chain crosses are zero.  External wrenches enter the existing entry points exactly, by linearity:
            tau = compute_inverse_dynamics(q, qd, qdd) - tau_ext          qdd = compute_forward_dynamics(q, qd, f + tau_ext).

        ONE kernel launch (csrc/drm_links.hip drm_external_torques): a sweep outwards for the poses and one inwards for the wrenches,
        instead of one Jacobian launch and two einsums per loaded link.  It is the adjoint of compute_link_velocities:
        sum_l f_l . v_l + m_l . w_l == tau_ext . qd for every qd.  DIFFERENTIABLE once with respect to forces and torques: the backward
        is the link-motion launch with qd := grad_tau (autograd._LinkAdjoint; a second backward raises).  By default there is NO
        gradient with respect to q: with grad mode on a q that requires grad raises ValueError; pass q.detach().
        ``differentiable_q=True`` opts in: q may require grad, the forward values are the same bits, and grad_q = d/dq [tau_ext .
        g_tau] comes from ONE drm_link_power_dq launch with qd := grad_tau (compute_link_power_gradient is that launch without
        autograd).  Still first order only.  A row whose q is not finite (or beyond 1e5) returns NaN and changes no other row; a wrench
        component that is not finite makes the torques of that link's ancestor joints non-finite and changes nothing else.  Devices,
        joint models, learnable links and ``_composed``: as for compute_link_motion."""
        if forces is None and torques is None:
            raise ValueError("forces and torques are both None")
        with torch.no_grad():
            dw, T, sel, identity = self._links_plan(link_names)
        unbatched, q, (forces, torques) = self._links_args(q, [(forces, "forces"), (torques, "torques")], (int(sel.numel()), 3))
        if not differentiable_q:
            self._refuse_grad_q(q, "compute_external_torques")
        self._require_device()
        with torch.no_grad():
            ops_f = self._ops_f(dw).detach()
        wrench_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (forces, torques))
        needs_grad = wrench_grad or (torch.is_grad_enabled() and bool(differentiable_q) and q.requires_grad)
        with torch.set_grad_enabled(wrench_grad):
            f, m = self._links_scatter(forces, sel, T, identity), self._links_scatter(torques, sel, T, identity)
        if needs_grad:
            tau = _LinkAdjoint.apply(True, q if differentiable_q else q.detach(), f, m, dw.program, ops_f, dw.ops_i, T, self._n_dofs,
                                     bool(_composed), bool(differentiable_q))
        else:
            with torch.no_grad():
                tau = backend.external_torques(dw.program, ops_f, dw.ops_i, q.detach(), f.detach() if f is not None else None,
                                               m.detach() if m is not None else None, T, self._n_dofs, composed=bool(_composed))
        return tau[0] if unbatched else tau

    def compute_link_power_gradient(self, q: torch.Tensor, qd: torch.Tensor, forces: Optional[torch.Tensor],
                                    torques: Optional[torch.Tensor] = None, link_names: Optional[List[str]] = None, *,
                                    _composed: bool = False) -> torch.Tensor:
        """dpower_dq [B, n] = dS/dq of the power of external wrenches on the named links,
            S(q; qd, forces, torques) = sum_l forces_l . v_l + torques_l . w_l = compute_external_torques(q, forces, torques) . qd,
        with qd and the wrenches held fixed and (v_l, w_l) = compute_link_velocities(q, qd).  It is the vector-Jacobian product in q
        of BOTH methods: of the velocities under the cotangents (forces, torques), of the torques under the cotangent qd — what their
        ``differentiable_q=True`` backward launches, here for callers who want it without autograd.  ONE kernel launch
        (csrc/drm_links.hip drm_link_power_dq): the two sweeps of compute_external_torques with the velocities carried outwards and one
        more 3-vector inwards; no kinematic Hessian, no per-link Jacobian.  Argument handling, ``link_names``, non-finite rows and
        wrenches, devices and ``_composed``: compute_external_torques'.  No autograd history."""
        if forces is None and torques is None:
            raise ValueError("forces and torques are both None")
        with torch.no_grad():
            dw, T, sel, identity = self._links_plan(link_names)
        unbatched, q, (forces, torques) = self._links_args(q, [(forces, "forces"), (torques, "torques")], (int(sel.numel()), 3))
        assert isinstance(qd, torch.Tensor) and tuple(qd.shape) == ((self._n_dofs,) if unbatched else tuple(q.shape)), "qd must be like q"
        qd = qd.unsqueeze(0) if unbatched else qd
        self._require_device()
        with torch.no_grad():
            f, m = self._links_scatter(forces, sel, T, identity), self._links_scatter(torques, sel, T, identity)
            dq, _ = backend.link_power_dq(dw.program, self._ops_f(dw).detach(), dw.ops_i, q.detach(), qd.detach(),
                                          f.detach() if f is not None else None, m.detach() if m is not None else None, T, self._n_dofs,
                                          composed=bool(_composed))
        return dq[0] if unbatched else dq

    # ------------------------------------------------------------------ collision of spheres with a world and with each other
    def _collision_world_tables(self, world):
        """(spheres [Ms, 4] or None, boxes [Mb, 16] or None) on the device; both None without obstacles"""
        if world is None:
            return None, None
        if not isinstance(world, CollisionWorld):
            raise TypeError("world must be a CollisionWorld (or None)")
        if world.n_obstacles == 0:
            return None, None
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self._device)
        return dev(world.spheres), dev(world.boxes)

    def _collision_rep(self, link):
        """the link a fixed-joint chain hangs on: a chain of fixed joints counts as one link"""
        i = int(link)
        while i > 0 and self._spec.dof[i] < 0:
            i = int(self._spec.parent[i])
        return i

    def make_collision_geometry(self, spheres: CollisionSpheres, world: Optional[CollisionWorld] = None, self_pairs="auto", *,
                                _subset_walk: bool = False) -> CollisionGeometry:
        """The device tables of compute_collision_cost / compute_sphere_distances, built once: the spheres sorted by link (a stable
        sort; results come back in the caller's order), their centres converted into the frames the kernels walk, the obstacles, and
        the self-collision pairs.  ``self_pairs``: "auto" — every pair of spheres whose links are neither the same nor parent and
        child, a chain of fixed joints counting as one link; None; or an explicit [P, 2] list in the caller's sphere indices
        (i != j).  The walk is the one of compute_link_motion over every link, so links without a sphere cost nothing but an empty
        group (``_subset_walk``: the walk over the links that carry spheres alone; for tests)."""
        if not isinstance(spheres, CollisionSpheres):
            raise TypeError("spheres must be a CollisionSpheres")
        for name in spheres.link_names:
            if name not in self._name_to_idx_map:
                raise KeyError("unknown link %r" % name)
        link_idx = [self._name_to_idx_map[name] for name in spheres.link_names]
        walk_names = None
        if _subset_walk:
            walk_names = tuple(dict.fromkeys(spheres.link_names))
        with torch.no_grad():
            dw, T, sel, _ = self._links_plan(None if walk_names is None else list(walk_names))
        names = self.get_link_names() if walk_names is None else list(walk_names)
        slot = {self._name_to_idx_map[name]: int(t) for name, t in zip(names, sel.tolist())}      # T for the root
        group = np.asarray([0 if slot[i] == T else slot[i] + 1 for i in link_idx], np.int64)
        # the stored frame of target t is R~ = R P with (M P)[:, c] = d[c] M[:, pi[c]]: c~ = P^T c, c~[c] = d[c] c[pi[c]], exactly
        ops = np.asarray(dw.program.ops_i)
        code = {}
        for k in range(dw.program.n_ops):
            if ops[k, OPI_OUT] >= 0:
                code[int(ops[k, OPI_OUT])] = int(ops[k, OPI_PERM])        # (a link of two ops: the frame of its last op)
        centers = spheres.centers.copy()
        for s_i, g in enumerate(group):
            c = code[int(g) - 1] if g else 2
            pi, sign = _PERM[c % 3], (-1.0 if c >= 3 else 1.0)
            d = (1.0, sign, sign)
            centers[s_i] = [d[k] * spheres.centers[s_i, pi[k]] for k in range(3)]
        order = np.argsort(group, kind="stable")             # grouped position g holds the caller's sphere order[g]
        inverse = np.empty_like(order)
        inverse[order] = np.arange(len(order))
        table = np.concatenate([centers, spheres.radii[:, None]], axis=1)[order].astype(np.float32)
        start = np.searchsorted(group[order], np.arange(T + 2), side="left").astype(np.int32)
        if isinstance(self_pairs, str):
            if self_pairs != "auto":
                raise ValueError("self_pairs must be 'auto', None or a [P, 2] list of sphere indices")
            rep = [self._collision_rep(i) for i in link_idx]
            up = [self._collision_rep(self._spec.parent[r]) if r > 0 else -1 for r in rep]
            pairs = [(i, j) for i in range(len(rep)) for j in range(i + 1, len(rep))
                     if rep[i] != rep[j] and up[i] != rep[j] and up[j] != rep[i]]
            # (in grouped order, first sphere by first sphere: the kernels keep a run's gradient in registers)
            pairs = sorted((min(inverse[i], inverse[j]), max(inverse[i], inverse[j])) for i, j in pairs)
            pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        elif self_pairs is not None:
            pairs = np.asarray(self_pairs.detach().cpu() if isinstance(self_pairs, torch.Tensor) else self_pairs, dtype=np.int64)
            if pairs.ndim != 2 or pairs.shape[1] != 2:
                raise ValueError("self_pairs must be [P, 2] (got %s)" % (list(pairs.shape),))
            if pairs.size and (pairs.min() < 0 or pairs.max() >= len(group) or (pairs[:, 0] == pairs[:, 1]).any()):
                raise ValueError("self_pairs must index the spheres, i != j")
            pairs = inverse[pairs].astype(np.int32)
        else:
            pairs = None
        if pairs is not None and len(pairs) == 0:
            pairs = None
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self._device)
        ws, wb = self._collision_world_tables(world)
        identity = bool((order == np.arange(len(order))).all())
        return CollisionGeometry(self, walk_names, dev(table), dev(start), None if identity else dev(inverse), None if pairs is None else dev(pairs),
                                 ws, wb)

    def _collision_args(self, q, geometry):
        if not isinstance(geometry, CollisionGeometry) or geometry._model is not self:
            raise TypeError("geometry must come from this model's make_collision_geometry")
        if not isinstance(q, torch.Tensor):
            raise TypeError("q must be a tensor")
        assert q.device.type == self._device.type, "Input argument of different device as module: q"
        assert q.ndim in [1, 2], "Input tensors must have ndim of 1 or 2."
        assert q.shape[-1] == self._n_dofs
        self._require_device()
        with torch.no_grad():
            dw, T, _, _ = self._links_plan(None if geometry._walk_names is None else list(geometry._walk_names))
            ops_f = self._ops_f(dw).detach()
        return q.ndim == 1, (q.unsqueeze(0) if q.ndim == 1 else q), dw, T, ops_f

    def compute_collision_cost(self, q: torch.Tensor, geometry: CollisionGeometry, *, world_activation: float = 0.05,
                               self_activation: float = 0.02, world_weight: float = 1.0, self_weight: float = 1.0,
                               _composed: bool = False) -> CollisionCost:
        """The collision cost of the geometry's spheres at q [B, n] and its gradient, from ONE launch (csrc/drm_collision.hip):
            cost      [B]     world_weight sum_{s, m} phi(world_activation - d_sm) + self_weight sum_pairs phi(self_activation - d_ij)
            dcost_dq  [B, n]  its gradient with respect to q
        with d_sm the clearance of sphere s to obstacle m (signed distance of its centre minus its radius), d_ij = |x_i - x_j| - r_i -
        r_j, and phi(u) = 0 for u <= 0, u^2 / (2 eta) up to eta, u - eta / 2 above: a sum over obstacles, not a minimum, zero beyond the
        activation distance and C1 where it switches on.  All 8 links of a 7-DoF arm with at most 64 spheres, 32 obstacles and 1 024
        pairs on full 64-row tiles: one kernel, a block of four wavefronts per tile; every other robot, size and tail one lane per row
        (a walk outwards, the pairs, compute_external_torques' sweep inwards).  ``cost`` is DIFFERENTIABLE once with respect to q: its
        backward is g[:, None] * dcost_dq and launches nothing; a second backward raises.  ``dcost_dq`` carries no history.  A row whose q
        is not finite (or beyond 1e5) returns NaN and changes no bit of any other row.  A geometry with neither a world nor pairs raises
        ValueError.  Argument handling: unbatched q gives unbatched results; CPU or HIP device; the current values of learnable links."""
        unbatched, q, dw, T, ops_f = self._collision_args(q, geometry)
        if not geometry.has_world and geometry.pairs is None:
            raise ValueError("the geometry has neither a world nor self pairs: there is no cost")
        params = (float(world_weight), float(world_activation), float(self_weight), float(self_activation))
        for name, w, eta, on in (("world", params[0], params[1], geometry.has_world), ("self", params[2], params[3], geometry.pairs is not None)):
            if on and not (math.isfinite(w) and w >= 0.0 and math.isfinite(eta) and eta > 0.0):
                raise ValueError("%s_weight must be finite and >= 0 and %s_activation finite and > 0" % (name, name))
        args = (dw.program, ops_f, dw.ops_i, T, self._n_dofs, geometry.tables(), params, bool(_composed))
        if torch.is_grad_enabled() and q.requires_grad:
            cost, dq = _CollisionCost.apply(q, *args)
        else:
            with torch.no_grad():
                cost, dq = backend.collision_cost(args[0], args[1], args[2], q.detach(), *args[3:7], composed=args[7])
        return CollisionCost(cost[0], dq[0]) if unbatched else CollisionCost(cost, dq)

    def compute_sphere_distances(self, q: torch.Tensor, geometry: CollisionGeometry, *, _composed: bool = False) -> SphereDistances:
        """The world centres of the geometry's spheres at q [B, n] and their clearances, in the CALLER's sphere order, from one launch
        (csrc/drm_collision.hip drm_sphere_distances):
            center          [B, S, 3]
            world_distance  [B, S]  min over the obstacles of (signed distance of the centre - radius); +inf without a world
            self_distance   [B, S]  min over the pairs the sphere is in of |x_i - x_j| - r_i - r_j; +inf when it is in none
        A negative clearance is a penetration.  Forward only: a q that requires grad raises ValueError (compute_collision_cost is
        the differentiable quantity; gradients of the clearances are out of scope).  Rows, devices, paths: compute_collision_cost's."""
        unbatched, q, dw, T, ops_f = self._collision_args(q, geometry)
        if torch.is_grad_enabled() and q.requires_grad:
            raise ValueError("compute_sphere_distances is forward only: use compute_collision_cost for a differentiable quantity "
                             "(or pass q.detach())")
        with torch.no_grad():
            outs = backend.sphere_distances(dw.program, ops_f, dw.ops_i, q.detach(), T, self._n_dofs, geometry.tables(),
                                            composed=bool(_composed))
            if geometry.order is not None:
                outs = [x.index_select(1, geometry.order) for x in outs]
        return SphereDistances(*[x[0] if unbatched else x for x in outs])

    # ------------------------------------------------------------------ plane contact and joint-limit springs
    def _contact_plan(self, contact, link_names, joint_limits):
        """(links walk or None, T, sel, identity, plane tuple or None, radius [T] on the device or None, springs tuple or None)"""
        if contact is not None and not isinstance(contact, PlaneContact):
            raise TypeError("contact must be a PlaneContact (or None)")
        if joint_limits is not None and not isinstance(joint_limits, JointLimitSprings):
            raise TypeError("joint_limits must be a JointLimitSprings (or None)")
        lw = sel = plane = radius = springs = None
        T, identity = 0, True
        if contact is not None:
            lw, T, sel, identity = self._links_plan(link_names)
            plane = contact._plane()
            per_entry = contact.radius
            if isinstance(per_entry, tuple):
                if len(per_entry) != int(sel.numel()):
                    raise ValueError("radius has %d values for %d link names" % (len(per_entry), int(sel.numel())))
            if per_entry != 0.0:
                key = (None if link_names is None else tuple(link_names), per_entry)
                cache = self.__dict__.setdefault("_contact_radii", {})
                radius = cache.get(key)
                if radius is None:
                    slots = [None] * T
                    for pos, s in enumerate(sel.tolist()):
                        r = per_entry[pos] if isinstance(per_entry, tuple) else per_entry
                        if s < T:           # (the root never touches)
                            if slots[s] is not None and slots[s] != r:
                                raise ValueError("a link named twice has two different radii")
                            slots[s] = r
                    radius = cache[key] = torch.tensor(slots, dtype=torch.float32, device=self._device)
        if joint_limits is not None:
            lower, upper = self._joint_bounds()
            springs = (joint_limits.stiffness, joint_limits.damping, lower, upper)
        return lw, T, sel, identity, plane, radius, springs

    def _refuse_grad(self, what, **tensors):
        if torch.is_grad_enabled():
            for name, t in tensors.items():
                if t is not None and t.requires_grad:
                    raise ValueError("%s is forward only: it has no gradient with respect to %s (pass %s.detach())" % (what, name, name))

    def compute_contact_torques(self, q: torch.Tensor, qd: torch.Tensor, contact: PlaneContact, link_names: Optional[List[str]] = None,
                                joint_limits: Optional[JointLimitSprings] = None, *, differentiable: bool = False,
                                _composed: bool = False) -> ContactTorques:
        """The joint torques of a plane's penalty contact with spheres on the named links (None: every link in get_link_names()
        order) at q, qd [B, n], plus those of joint-limit springs when ``joint_limits`` is given, and the wrenches themselves:
            tau     [B, n]     sum_l lin_jac_l^T force_l + ang_jac_l^T moment_l (+ tau_lim)
            force   [B, L, 3]  the plane's force on link l, world axes       moment  [B, L, 3]  its moment about the link origin
        The law is PlaneContact's; ``link_names`` is handled as in compute_link_motion (any order, repeats, the root — which never
        touches and gets zeros).  ONE kernel launch for all 8 links of a 7-DoF arm on full 64-row tiles (csrc/drm_contact.hip: one
        sweep outwards with velocities, the law per link, one sweep inwards, all in registers); every other robot and link set
        composes the link-motion launch, one element-wise law kernel, the external-torques launch and one add.  By default forward
        only: a q or qd that requires grad raises ValueError, and the results carry no autograd history (the current values of
        learnable links are used).  ``differentiable=True`` opts in: the forward values are the same bits from the same launch, and
        ``tau`` is DIFFERENTIABLE once with respect to q and qd — its backward is ONE compute_contact_torques_vjp call
        (autograd._ContactTorques; a second backward raises NotImplementedError).  The law is piecewise smooth: at a switch the
        gradient is that of the branch the forward took.  ``force`` and ``moment`` come back detached, and no gradient reaches
        learnable link parameters or the contact parameters: the walk's table is a constant of the node.  A row whose q or qd is not
        finite returns NaN and changes no bit of any other row."""
        if contact is None:
            raise ValueError("compute_contact_torques needs a PlaneContact")
        unbatched, q, (qd,) = self._links_args(q, [(qd, "qd")], (self._n_dofs,))
        assert qd is not None, "qd must be given"
        if not differentiable:
            self._refuse_grad("compute_contact_torques", q=q, qd=qd)
        self._require_device()
        with torch.no_grad():
            lw, T, sel, identity, plane, radius, springs = self._contact_plan(contact, link_names, joint_limits)
            ops_f = self._ops_f(lw).detach()
        if differentiable and torch.is_grad_enabled() and (q.requires_grad or qd.requires_grad):
            tau, force, moment = _ContactTorques.apply(q, qd, lw.program, ops_f, lw.ops_i, T, self._n_dofs, plane, radius, springs,
                                                       bool(_composed))
        else:
            with torch.no_grad():
                tau, force, moment = backend.contact_torques(lw.program, ops_f, lw.ops_i, q.detach(), qd.detach(), T, self._n_dofs, plane,
                                                             radius, springs, composed=bool(_composed))
        with torch.no_grad():
            force, moment = self._links_gather(force, sel, identity), self._links_gather(moment, sel, identity)
        return ContactTorques(*[x[0] if unbatched else x for x in (tau, force, moment)])

    def compute_contact_torques_vjp(self, q: torch.Tensor, qd: torch.Tensor, grad_tau: torch.Tensor, contact: Optional[PlaneContact],
                                    link_names: Optional[List[str]] = None, joint_limits: Optional[JointLimitSprings] = None, *,
                                    _composed: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(grad_q, grad_qd) [B, n]: the vector-Jacobian product of compute_contact_torques' ``tau`` at q, qd under the cotangent
        ``grad_tau`` [B, n], i.e. the gradients of grad_tau . tau with respect to q and qd — what the ``differentiable=True`` backward
        launches, here for callers who want it without autograd.  ONE launch for all 8 links of a 7-DoF arm on full 64-row tiles
        (csrc/drm_contact.hip: one sweep outwards that carries the link velocities at rates qd and at rates grad_tau together with the
        law and its backward per link, one sweep inwards with three wrench sets); every other robot and link set composes the
        link-motion launch twice, one element-wise kernel, the link-power-gradient launch twice, the external-torques launch and one
        add.  No Jacobian and no kinematic Hessian is formed.  At a switch of the law the gradient is that of the branch
        compute_contact_torques takes.  ``contact`` may be None when ``joint_limits`` is given (the springs' share alone).  Argument
        handling and ``link_names``: compute_contact_torques'.  A row whose q, qd or grad_tau is not finite returns NaN and changes no
        bit of any other row.  No autograd history."""
        if contact is None and joint_limits is None:
            raise ValueError("neither contact nor joint_limits")
        unbatched, q, (qd, grad_tau) = self._links_args(q, [(qd, "qd"), (grad_tau, "grad_tau")], (self._n_dofs,))
        assert qd is not None and grad_tau is not None, "qd and grad_tau must be given"
        self._require_device()
        with torch.no_grad():
            lw, T, _, _, plane, radius, springs = self._contact_plan(contact, link_names, joint_limits)
            if lw is None:          # (springs alone: any links walk, it is not walked)
                lw, T, _, _ = self._links_plan(None)
            gq, gqd = backend.contact_torques_vjp(lw.program, self._ops_f(lw).detach(), lw.ops_i, q.detach(), qd.detach(), grad_tau.detach(),
                                                  T, self._n_dofs, plane, radius, springs, composed=bool(_composed))
        return (gq[0], gqd[0]) if unbatched else (gq, gqd)

    def compute_contact_rollout(self, q0: torch.Tensor, qd0: torch.Tensor, tau: torch.Tensor, dt: float,
                                contact: Optional[PlaneContact], link_names: Optional[List[str]] = None,
                                joint_limits: Optional[JointLimitSprings] = None, integrator: str = "semi_implicit_euler",
                                include_gravity: Optional[bool] = True, use_damping: Optional[bool] = False,
                                return_acceleration: bool = False, *, differentiable: bool = False,
                                _composed: bool = False) -> ContactRollout:
        """compute_forward_dynamics_rollout with contact: step t computes
            qdd_t = compute_forward_dynamics(q_t, qd_t, tau[t] + tau_ext(q_t, qd_t) + tau_lim(q_t, qd_t), include_gravity, use_damping)
        with tau_ext, tau_lim compute_contact_torques' at the state of the step, then the integrator's update.  Shapes, the
        time-major tau [T, B, n], the integrators and the unbatched form are compute_forward_dynamics_rollout's; ``qdd`` [T, B, n]
        (the acceleration of each step) comes back with ``return_acceleration``.  ONE launch for a 7-DoF arm with all of its 8
        links in contact, on full 64-row tiles with B n a multiple of 4 (csrc/drm_contact.hip: the state stays in registers across
        the steps); every other case composes, per step, the contact torques, one add, the forward dynamics and the integrator on
        the caller's stream.  ``contact=None`` needs ``joint_limits`` (the plain rollout exists for neither).  By default forward
        only: a q0, qd0 or tau that requires grad raises ValueError; the results carry no autograd history.
        ``differentiable=True`` opts in: the forward values are the same bits, and ``q`` and ``qd`` are DIFFERENTIABLE once with
        respect to q0, qd0 and tau through ONE autograd node (autograd._ContactRollout) whose backward is a reverse sweep over the
        steps — per step the two launches of compute_forward_dynamics' backward and one compute_contact_torques_vjp call, at the
        states the forward returned.  At a switch of the law the gradient is that of the branch the forward took.  ``qdd`` comes
        back detached; a second backward raises NotImplementedError; no gradient reaches learnable link parameters (their current
        values are used) or the contact parameters: both walks' tables are constants of the node.  A row with a non-finite q0, qd0
        or tau gets non-finite results from that step on and changes no bit of any other row."""
        if integrator not in self.ROLLOUT_INTEGRATORS:
            raise ValueError("integrator must be one of %s (got %r)" % (self.ROLLOUT_INTEGRATORS, integrator))
        if contact is None and joint_limits is None:
            raise ValueError("neither contact nor joint_limits: compute_forward_dynamics_rollout is the plain rollout")
        for name, t in (("q0", q0), ("qd0", qd0), ("tau", tau)):
            assert type(t) is torch.Tensor, "%s must be a tensor" % name
            assert t.device.type == self._device.type, f"Input argument of different device as module: {t}"
        assert q0.ndim in [1, 2], "Input tensors must have ndim of 1 or 2."
        assert qd0.shape == q0.shape, "Batch size mismatch between input tensors."
        assert tau.ndim == q0.ndim + 1, "tau must be [T, B, n] ([T, n] for unbatched q0 / qd0)"
        assert tau.shape[1:-1] == q0.shape[:-1], "Batch size mismatch between input tensors."
        assert q0.shape[-1] == self._n_dofs and tau.shape[-1] == self._n_dofs
        dt = float(dt)
        if tau.shape[0] < 1:
            raise ValueError("a rollout takes at least one step (tau has T = 0)")
        if not (math.isfinite(dt) and dt > 0):
            raise ValueError("dt must be finite and positive (got %r)" % (dt,))
        if not differentiable:
            self._refuse_grad("compute_contact_rollout", q0=q0, qd0=qd0, tau=tau)
        single = q0.ndim == 1
        if single:
            q0, qd0, tau = q0.unsqueeze(0), qd0.unsqueeze(0), tau.unsqueeze(1)
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            lw, T, _, _, plane, radius, springs = self._contact_plan(contact, link_names, joint_limits)
            links = (lw.program, self._ops_f(lw).detach(), lw.ops_i) if lw is not None else None
            dyn = (dw.program, self._ops_f(dw).detach(), dw.ops_i)
        if differentiable and torch.is_grad_enabled() and (q0.requires_grad or qd0.requires_grad or tau.requires_grad):
            vjp_links = links
            if vjp_links is None:          # (springs alone: any links walk, the backward does not walk it)
                with torch.no_grad():
                    aw = self._links_plan(None)[0]
                    vjp_links = (aw.program, self._ops_f(aw).detach(), aw.ops_i)
            out = _ContactRollout.apply(q0, qd0, tau, dyn, links, vjp_links, dt, bool(include_gravity), bool(use_damping),
                                        integrator == "euler", T, self._n_dofs, plane, radius, springs, bool(return_acceleration),
                                        bool(_composed))
        else:
            with torch.no_grad():
                out = backend.contact_rollout(dyn, links, q0.detach(), qd0.detach(), tau.detach(), dt, bool(include_gravity),
                                              bool(use_damping), integrator == "euler", T, self._n_dofs, plane, radius, springs,
                                              want_qdd=bool(return_acceleration), composed=bool(_composed))
        return ContactRollout(*[x[:, 0] if (single and x is not None) else x for x in out])

    def compute_inverse_dynamics_derivatives(self, q: torch.Tensor, qd: torch.Tensor, qdd: torch.Tensor,
                                             include_gravity: Optional[bool] = True, use_damping: Optional[bool] = False, *,
                                             _composed: bool = False) -> InverseDynamicsDerivatives:
        """Inverse dynamics tau = ID(q, qd, qdd) and its first-order derivatives at q, qd, qdd [B, n]: what inverse-dynamics
        trajectory optimisation (direct transcription with torque limits) needs at every knot, and gain design for computed-torque
        control, an EKF with a torque measurement and Gauss-Newton identification in the state:
            tau        [B, n]     compute_inverse_dynamics(q, qd, qdd, include_gravity, use_damping)
            dtau_dq    [B, n, n]  [b, i, j] = d tau_i / d q_j    (damping never enters it)
            dtau_dqd   [B, n, n]  [b, i, j] = d tau_i / d qd_j   (with ``use_damping`` it includes diag(damping); gravity never enters it)
            dtau_dqdd  [B, n, n]  H(q) = compute_lagrangian_inertia_matrix(q), up to float32 rounding; symmetric to the bit
        Entries of the three matrices are exactly zero where joints i and j lie on different branches.

        One kernel launch (csrc/drm_idd.hip): one sweep out and one back over the tree (Carpentier and Mansard 2018; Singh, Russell
        and Wensing 2022), O(n depth) work, instead of n backward passes through compute_inverse_dynamics and an inertia-matrix call.
        A 7-DoF arm's full 64-row tiles run a kernel that keeps everything in registers and stores the tiles of the outputs whole; every
        other robot one lane per row over the ops of its walk.  With the robot's own constant-folded kernels attached this entry point
        still runs the library kernels.  Argument handling is that of compute_forward_dynamics_derivatives (unbatched inputs give
        unbatched results); works for models on the CPU and on a HIP device, with either joint model (reference_compat) and for
        models with learnable links: their current values are used.  A row whose q, qd or qdd is not finite — or whose |q| is
        beyond 1e5, where float32 no longer resolves an angle — returns NaN and changes no bit of any other row.

        The results carry NO autograd history, whatever requires grad.  (``_composed``, or DRM_IDD_COMPOSED=1 in the environment:
        every row takes the general kernel, DRM_IDD_COMPOSED; for tests and A/B measurements.)"""
        return InverseDynamicsDerivatives(*self._compute_inverse_dynamics_derivatives(q, qd, qdd, include_gravity, use_damping,
                                                                                      bool(_composed)))

    @tensor_check
    def _compute_inverse_dynamics_derivatives(self, q, qd, qdd, include_gravity, use_damping, composed):
        assert q.ndim == 2
        assert qd.ndim == 2
        assert qdd.ndim == 2
        assert q.shape[1] == self._n_dofs
        assert qd.shape[1] == self._n_dofs
        assert qdd.shape[1] == self._n_dofs
        assert q.shape[0] == qd.shape[0] == qdd.shape[0]
        self._require_device()
        with torch.no_grad():
            dw = self._dynamics_walk()
            return backend.rnea_derivatives(dw.program, self._ops_f(dw).detach(), dw.ops_i, q.detach(), qd.detach(), qdd.detach(),
                                            bool(include_gravity), bool(use_damping), self._n_dofs, composed=composed)

    def regressor_links(self) -> List[str]:
        """The bodies of compute_inverse_dynamics_regressor, in block order: the link of every op of the dynamics walk — the moving
        links, plus any link kept as an op of its own because it (or a neighbour) is learnable.  Links folded away behind fixed
        joints are part of their fold target's body (flatten.fold_link_table).  (A link whose joint axis is not +-x / y / z is two
        ops, and appears twice: the first block, of the massless joint op, multiplies zeros.)"""
        prog = self._dynamics_walk().program
        return [self._spec.link_names[int(i)] for i in prog.links[:prog.n_ops]]

    def inertial_parameters(self, use_damping: Optional[bool] = False) -> torch.Tensor:
        """phi [P]: the parameters compute_inverse_dynamics_regressor's columns multiply, read from the same (folded, current) link
        table the kernels read — 10 per body of regressor_links(), [m, m c, Ixx, Ixy, Ixz, Iyy, Iyz, Izz] in the link's URDF frame
        with I about the frame's origin, then with ``use_damping`` the n joint dampings in DoF order.  float32 on the model's
        device, detached."""
        with torch.no_grad():
            dw = self._dynamics_walk()
            prog = dw.program
            table = self._link_table(dw.fold_key).detach().reshape(-1)
            rows = prog.gather[:prog.n_ops, OPF_MASS] - OPF_MASS          # flat index of every op's row in the link table
            take = [OPF_MASS, OPF_MCOM, OPF_MCOM + 1, OPF_MCOM + 2, OPF_IO, OPF_IO + 1, OPF_IO + 2, OPF_IO + 4, OPF_IO + 5, OPF_IO + 8]
            idx = (rows[:, None] + np.asarray(take, np.int64)[None, :]).reshape(-1)
            if use_damping:
                op_of_dof = {int(prog.ops_i[k, 0]): k for k in range(prog.n_ops) if prog.ops_i[k, 0] >= 0}
                idx = np.concatenate([idx, np.asarray([prog.gather[op_of_dof[d], OPF_DAMP] for d in range(self._n_dofs)], np.int64)])
            return table.index_select(0, torch.from_numpy(idx).to(table.device)).to(torch.float32)

    def compute_forward_dynamics_old(self, q: torch.Tensor, qd: torch.Tensor, f: torch.Tensor,
                                     include_gravity: Optional[bool] = True, use_damping: Optional[bool] = True
                                     ) -> torch.Tensor:
        """qdd = H^-1 (f - nle) (robot_model.py:452-485; upstream it calls ``torch.solve``, which current torch no longer
        has).  The same linear system as ``compute_forward_dynamics`` — note the different default of ``use_damping``."""
        return self.compute_forward_dynamics(q, qd, f, include_gravity=include_gravity, use_damping=use_damping)

    # ------------------------------------------------------------------ learnable parameters
    def _get_parent_object_of_param(self, link_name: str, parameter_name: str):
        body_idx = self._name_to_idx_map[link_name]
        if parameter_name in ["trans", "rot_angles", "joint_damping"]:
            return self._bodies[body_idx]
        if parameter_name in ["mass", "inertia_mat", "com"]:
            return self._bodies[body_idx].inertia
        raise AttributeError(
            "Invalid parameter name. Accepted parameter names are: "
            "trans, rot_angles, joint_damping, mass, inertia_mat, com")

    def make_link_param_learnable(self, link_name: str, parameter_name: str, parametrization: torch.nn.Module):
        """Replace a URDF constant by a learnable module under the same attribute (robot_model.py:682-689)."""
        parent_object = self._get_parent_object_of_param(link_name, parameter_name)
        parent_object.__delattr__(parameter_name)
        parent_object.add_module(parameter_name, parametrization.to(self._device))
        self._learnable.add((self._name_to_idx_map[link_name], parameter_name))
        self._learnable_links = None
        self._source_plan = None
        self._learnable_version += 1
        for dw in self._walks.values():
            dw.static_ops_f = None
            special = getattr(dw.program, "_special", None) or {}
            # kernels that carry the walk table as compile-time constants (specialize.attach_arm / attach_fan / attach_arm_param;
            # attach(table=...)) bake the OLD constants or the OLD set of learnable blocks: dropped — the next call looks again
            baked = getattr(dw.program, "_special_const", False)
            dw.program._special = {} if baked else {k: v for k, v in special.items() if k < 4}
            dw.program._special_const = False
            dw.program._special_tried = False
            dw.program._special_mask = 0
            dw.program._ws_cache = None
        self._arm_specialized = False
        self._fast_fk.clear(); self._fast_jac.clear(); self._fast_fkid.clear()    # (prepared calls snapshot the constants)
        self.__dict__.pop("_fast_links", None)
        self._fast_id = self._fast_crba = self._fast_fd = None
        self._fanout_plans.clear()      # (they may hold folded chain walks, which are for models without learnable parameters)
        self._fan_handles.clear()       # (kernels that bake the OLD constants)
        self._chain_walks.clear()
        self._dyn_walk = None

    def _learnable_module(self, link_name: str, parameter_name: str):
        parent_object = self._get_parent_object_of_param(link_name, parameter_name)
        module = getattr(parent_object, parameter_name)
        assert isinstance(module, torch.nn.Module), f"{parameter_name} of {link_name} is not a learnable module."
        return module

    def freeze_learnable_link_param(self, link_name: str, parameter_name: str):
        for param in self._learnable_module(link_name, parameter_name).parameters():
            param.requires_grad = False

    def unfreeze_learnable_link_param(self, link_name: str, parameter_name: str):
        for param in self._learnable_module(link_name, parameter_name).parameters():
            param.requires_grad = True

    # ------------------------------------------------------------------ introspection
    def get_joint_limits(self) -> List[Dict[str, float]]:
        return [self._bodies[idx].get_joint_limits() for idx in self._controlled_joints]

    def get_link_names(self) -> List[str]:
        return [body.name for body in self._bodies]

    def print_link_names(self) -> None:
        for body in self._bodies:
            print(body.name)

    def print_learnable_params(self) -> None:
        for name, param in self.named_parameters():
            print(f"{name}: {param}")


def _robot_path(rel):
    return os.path.join(robot_description_folder, rel)


class DifferentiableKUKAiiwa(DifferentiableRobotModel):
    def __init__(self, device=None):
        self.urdf_path = _robot_path("iiwa7.urdf")
        self.learnable_rigid_body_config = None
        self.name = "differentiable_kuka_iiwa"
        super().__init__(self.urdf_path, self.name, device=device)


class DifferentiableFrankaPanda(DifferentiableRobotModel):
    def __init__(self, device=None):
        self.urdf_path = _robot_path("panda_no_gripper.urdf")
        self.learnable_rigid_body_config = None
        self.name = "differentiable_franka_panda"
        super().__init__(self.urdf_path, self.name, device=device)


class DifferentiableTwoLinkRobot(DifferentiableRobotModel):
    def __init__(self, device=None):
        self.urdf_path = _robot_path("2link_robot.urdf")
        self.learnable_rigid_body_config = None
        self.name = "diff_2d_robot"
        super().__init__(self.urdf_path, self.name, device=device)


class DifferentiableTrifingerEdu(DifferentiableRobotModel):
    def __init__(self, device=None):
        self.urdf_path = _robot_path("trifinger_edu.urdf")
        self.learnable_rigid_body_config = None
        self.name = "trifinger_edu"
        super().__init__(self.urdf_path, self.name, device=device)

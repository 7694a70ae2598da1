"""Inverse dynamics and the fused forward kinematics + inverse dynamics on every rung of their dispatch (csrc/drm_rnea.hip drm_rnea,
drm_fk_rnea; DifferentiableRobotModel.compute_inverse_dynamics / compute_non_linear_effects / compute_fk_and_inverse_dynamics), row by
row against fp64.  Written in the manner of tests/test_fd_crba_rungs.py, whose helpers it shares.

INPUTS: for every robot of helpers.ALL_ROBOTS 256 rows of sample_states(m, 256, seed=61) and a second set with seed=7.  Case "id": the
drawn qdd under all four (include_gravity, use_damping); case "nle": qdd = None (compute_non_linear_effects: drm_rnea with qdd = NULL)
under (1, 1) and (0, 0).  The fused call takes the "id" cases and the link FUSED_LINK[robot] (an arm's last link).

TRUTH, from the fp64 oracle only: tau64 = Oracle.rnea(q, qd, qdd or 0) and, for the fused call, Oracle.fk(q, [link]).  Before anything
under test is compared: no row of tau64 is identically zero, and no joint column is — except ZERO_COLUMNS, listed literally below and
asserted against the truth: Fetch's two wheels under "nle" (both seeds, both flag pairs: a wheel turns about an axis through its own
centre of mass, is a leaf, and the base does not move; its torque is I_zz qdd and nothing else, and its damping is 0).  Those 2 of
Fetch's 14 columns are left out of `joint` in the "nle" cases only; they stay in `row`.

METRICS, in fp64, the worst over the batch:
    row    per row    max_i |dtau_i| / max_i |tau64_i|
    joint  per joint  max_b |dtau_bi| / max_b |tau64_bi|   (the gram-scale fingers and the last wrist joints at their own scale: the
           smallest joint scale under flags (0, 0) is 1.5e-4 N m on allegro_left, 4.9e-4 on fetch_arm_no_gripper, 4.7e-4 on jaco)
    pos    max_b |dpos| / max_b |pos64| of the target link (fused call)
    quat   max |dquat| after the sign rule of helpers.quat_close: a row within its branch margin (1e-5) may flip sign, a flip
           outside the margin counts with its full size (2) and fails
YARDSTICKS, not code under test: the same metrics of Oracle.rnea(float32) and Oracle.fk(float32) on the same rows.
REQUIREMENT: err(path) <= 8 max(err(yardstick), 2^-23) for each metric (8: the project's margin for a different summation order, as in
test_fd_crba_rungs.py, test_energy.py, test_links.py, test_lagrangian.py).  No path needed a further yardstick.
Every comparison prints one "RNEARUNG" line (robot, path, flags, case, seed, metric, error, yardstick, ratio) before it asserts;
profiles/rnea_rungs_tests.txt holds the worst of them per path and metric.

PATHS without a GPU: the device="cpu" model through the three public calls; the host emulation of the kernel arithmetic under g++ and
the ROCm clang — emu_rnea on the whole-tree and on the folded walk, emu_rnea_short where every segment has at most 6 ops, emu_rnea_arm
and emu_rnea_arm2 on the 8-link and on the folded 7-link table, emu_rnea_fingers, emu_rnea_arm_hand on all seven ARM_HAND_CASES,
emu_fk_rnea_arm (the fused arm kernel: pose chain over all 8 rows, the sweeps over the first LINKS) in both shapes of
fk_rnea_arm_applies — and Fetch's generated straight-line source (static_rnea) compiled for the host with both compilers.  Each of
them also takes the zero input and the |q| = 4.0e5 rows.

PATHS on the GPU (-m gpu).  A launch of B rows is repeated over consecutive slices of the 256 rows, so the statistic is over the same
rows whatever B is: B = 64 and 256 full tiles, 65 and 131 a fast rung plus a ragged tail in the loop kernel, 1 and 63 the loop kernel
alone, 128 and 129 (the two hands) one full 128-row tile of rnea_fingers2_kernel without and with a tail.  What sends a launch to a
rung (read off drm_rnea and drm_fk_rnea):
    own        special[DRM_SPECIAL_RNEA] set (model.specialize(); Fetch): full tiles at any pointer alignment, also as a [1:] view
    arm-own    special[DRM_SPECIAL_RNEA_ARM] / [DRM_SPECIAL_FK_RNEA_ARM] (specialize() on a 7-DoF arm) AND at least
               DRM_ARM_STATIC_MIN_PAIRS (1 024) pairs of tiles: below that size a specialized arm runs the library's arm rung
    arm        DRM_WALK_ARM_CHAIN, 16-byte aligned pointers: rnea_arm_kernel<8, 7, 7> on the API's folded walk, <8, 7, 8> on the
               unfolded 8-op walk through the C ABI; more than DRM_TWO_SAMPLE_MIN_TILES (1 024) tiles: rnea_arm2_kernel on the pairs,
               its latency form up to DRM_LAT2_MAX_TILES (1 024) pairs, its throughput form beyond
    fingers    DRM_WALK_FINGERS, full 128-row tiles (allegro_left L = 4, trifinger_edu L = 3)
    arm-hand   DRM_WALK_ARM_HAND, full tiles, own_kernels = "off" (panda, jaco, iiwa7_allegro)
    loop       what is left: rnea_tree_kernel where rnea_short_plan applies (segments of <= 6 ops: the hands, 2link_robot), the
               persistent rnea_records_kernel elsewhere; reached by B < 64, by a ragged tail, by the walk with its shape bit cleared
               through the C ABI, and by a [1:] view
    fused      compute_fk_and_inverse_dynamics: fk_rnea_arm_kernel / fk_rnea_arm2_kernel / drm_fk_rnea_arm_static on panda_no_gripper,
               iiwa7 and fetch_arm_no_gripper (the API's folded walk; `same`, tree walk == chain walk, through the host emulation and
               through the C ABI); tau bit-equal to compute_inverse_dynamics of the same rows, pos and quat bit-equal to
               compute_forward_kinematics where the two launches share a tile width (a wave of the two-samples-per-lane forms owns 128
               rows: the tiles of the |q| = 4.0e5 rows are held to the requirement only); every other robot: drm_fk then drm_rnea
RUNGS that need size (the 256 rows tiled cyclically, every row of the launch compared with its truth row in one numpy expression):
1 027 * 64 + 17 rows (513 pairs through rnea_arm2_kernel / fk_rnea_arm2_kernel, the odd tile through the one-sample kernel, the tail
through the loop kernel; API walk and the unfolded walk); 2 * 64 * 1 024 + 64 + 3 rows on a specialized arm (drm_rnea_arm_static,
drm_fk_rnea_arm_static), and 2 * 64 * 1 025 + 64 + 3 with own_kernels = "off" (n2 = 1 025 > DRM_LAT2_MAX_TILES: the throughput form);
a [1:] view of 65 * 64 + 1 rows of panda_no_gripper and panda (more than MISALIGNED_TILES = 64 tiles on the capped grid of
rnea_records_kernel, scratch sized by drm_rnea_scratch_floats, not the _aligned query); 2 049 * 64 + 3 rows of Fetch with
own_kernels = "off" — the one robot family whose walk (14 ops, a segment of more than 6: rnea_short_plan says no) takes
rnea_records_kernel with no straight-line rung in front; its resident count (256 CUs x at most 8 blocks of 192 threads, LDS-bound
lower) is below 2 049, so blocks walk a second tile.  arm2_stream_kernel is off by default (DRM_PIPE_MIN_TILES) and not covered.

RUNG IDENTITY: two launches of one kernel on the same rows are bit-equal; rows of full tiles are bit-equal with and without a tail
behind them; two rungs that compute the same rows with different arithmetic must NOT agree bit for bit over the 256 rows — arm-own
against arm (at the size arm-own needs), fingers against loop, arm-hand against loop, own against loop, and arm against loop where
the two are not bit-identical by construction (MUST_DIFFER_FROM_LOOP below and FOUND: fetch_arm_no_gripper with damping on).

EXACT, on the host build and on every GPU rung: qd = 0, qdd = 0, gravity off gives tau == 0; q, qd, qdd unchanged by the call; an
output pre-filled with NaN has no NaN in its B rows and the row behind them keeps its sentinel; a row with one |q| = 4.0e5 (the fp64
sincos fallback, wave-uniform) meets the requirement like every other; an all-NaN q row and an all-Inf qdd row come back non-finite in
every entry (but see FOUND for Fetch's two wheels, whose torque does not see q) and change no bit of the other rows, once in full tiles (128 rows, rows 5 and 70) and once in a ragged tail (127 rows,
rows 70 and 100); 1-D arguments and a column-slice q give the bits of the contiguous batched call; compute_non_linear_effects(q, qd)
equals compute_inverse_dynamics with a zero qdd tensor to the bit on the same rung.

FOUND by this module:
  * compute_fk_and_inverse_dynamics raised ValueError ("q of a plan must be a contiguous, 16-byte aligned fp32 tensor") on a row slice
    4 n bytes off a 16-byte boundary (q[65:130] of a 7-DoF arm) and on a column slice — tensors that compute_inverse_dynamics copies and
    serves.  FIXED in robot_model._compute_fk_and_inverse_dynamics: its one-launch plan now copies such a slice (backend._dev_f32).
  * drm_rnea_static of Fetch (model.specialize(): the walk table folded into the instruction stream under -ffinite-math-only) returns, on
    the row of an all-NaN q, the clean bits in the two wheel columns (-0.0078, 0.0072 N m) and NaN in the other twelve; every other rung
    returns NaN in all fourteen.  Those torques do not depend on q (Q_INDEPENDENT, asserted against the truth), so the finite value is
    the right one and the kernel stays as it is; the exact condition on a NaN row is therefore "non-finite, or a Q_INDEPENDENT entry
    with the bits of the clean row" — for Fetch's two columns only, every other robot and column is held to "non-finite".
  * rnea_arm_kernel (both instantiations) and rnea_arm2_kernel carry the bits of the loop kernel on panda_no_gripper and iiwa7 in every
    case, and on fetch_arm_no_gripper with damping off (MUST_DIFFER_FROM_LOOP above says why): bit-identical by construction, so `arm`
    against `loop` is asserted on fetch_arm_no_gripper ("id", 1, 1) alone (225 of 1 792 entries differ) and reported for the rest.
    For the same reason "two samples per lane vs one" is reported, not asserted.
  * drm_fk_rnea_arm_static and drm_rnea_arm_static are two code objects and do not agree to the bit: on panda_no_gripper tau differs in
    69 120 of 917 973 entries (largest 7.7e-07 of 47.2 N m; iiwa7: bit-equal), the pose differs from compute_forward_kinematics by one
    ulp in a quarter of the entries.  The fused call's bit-equality with the separate calls is asserted at every B of the table above
    and on the library's two-samples-per-lane kernels; at the size of `arm-own` both calls are held to the requirement and the
    comparison is printed.

MEASURED (profiles/rnea_rungs_tests.txt), worst err / yardstick over both seeds, all cases and flags, per metric:
                                                   row    joint  pos    quat
    host build (API), fused call                   4.72   2.27   1.33   1.82     (row: fetch, "nle", (0, 0), seed 7)
    host emulation g++ / clang, static source      4.91   2.29   1.25   1.82     (emu_rnea on the folded walk and static_rnea: fetch)
      emu_rnea tree / folded / short               4.91   2.29   -      -
      emu_rnea_arm, emu_rnea_arm2 <8,7,7>, <8,7,8> 1.93   2.29   -      -
      emu_rnea_fingers                             2.01   1.30   -      -
      emu_rnea_arm_hand (seven cases)              3.88   1.89   -      -        (row: panda with sliding fingers)
      emu_fk_rnea_arm <8,7,7>, <8,7,8>             1.93   2.29   1.25   1.82
    MI355X, all rungs                              4.72   2.27   1.33   1.82
      own, own+tail, own on a [1:] view (Fetch)    4.27   1.62   1.04   1.06
      arm-own + odd tile + tail (131 139 rows)     2.17   0.92   1.09   1.27
      arm<8,7,7>, +tail; fused                     1.56   1.95   1.25   1.82
      arm<8,7,8>, +tail; fused `same`              1.56   1.95   1.25   1.82
      arm2 latency form + odd tile + tail          1.45   1.15   1.09   1.09     (65 745 rows; <8,7,8>: joint 1.02)
      arm2 throughput form + odd tile + tail       1.45   0.99   1.09   1.09     (131 267 rows)
      fingers, +tail                               1.90   1.30   0.89   1.11
      arm-hand, +tail                              2.30   1.54   1.33   1.39
      loop (B < 64, shape bit cleared)             4.72   2.27   1.33   1.82
      loop, misaligned beyond the capped grid      1.72   1.00   -      -
      loop, persistent beyond resident blocks      0.92   0.75   -      -        (1 792 resident blocks, 2 050 tiles)
      the other five robots, B = 65 and 256        2.10   1.95   1.27   1.21
      |q| = 4.0e5 rows (every rung)                2.17   1.15   1.33   1.39
MUTATIONS on a scratch copy of the host emulation (figures in profiles/rnea_rungs_tests.txt):
  * the mass of link 2 of allegro_left's folded table scaled by 1 + 1e-3: TOL_TAU passes (1.9e-05 N m), CAUGHT (row 5.9e-04 against
    4.5e-07, joint 4.0e-04 against 1.5e-06);
  * the velocity-product force of link 6 left out of the distal joint's torque, fetch_arm_no_gripper, (0, 0): CAUGHT (joint 0.27 against
    4.8e-05) — at 1.3e-04 N m it is beyond TOL_TAU's 2e-05 as well, so this one the old tolerance did not let through;
  * the z offset of the fixed tail of panda_no_gripper's fused pose chain + 1e-6 m: pos 8.9e-07 against 1.19e-07, 7.5x — inside the
    margin, NOT caught (eight fp32 ulps of a 1.17 m reach are 1.1e-06 m); + 2e-6 m is (1.75e-06, 14.7x).
NO HOST EMULATION: fk_rnea_arm2_kernel's pose chain (fk_chain2_trig) and the constant-folded code objects (drm_rnea_static on the device,
drm_rnea_arm_static, drm_fk_rnea_arm_static); the GPU tests hold every row of their launches.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from differentiable_robot_model_amd import specialize as sp
from differentiable_robot_model_amd.flatten import SHAPE_ARM_CHAIN, SHAPE_ARM_HAND, SHAPE_FINGERS, build_walk, foldable_links
from helpers import ALL_ROBOTS, GOLDEN_ROBOTS, quat_branch_margin, sample_states
from oracle import Oracle
from test_fd_crba_rungs import (ARM_HAND_ROBOTS, ARM_ROBOTS, ARM_STATIC_MIN_PAIRS, BIG_ANGLE, FINGER_ROBOTS, FLAGS, FLOOR, MARGIN, ROWS,
                                RUNG_ROBOTS, RUNGS, SEEDS, dev, gpu_model, library_and_stream, model_on, needs_hipcc, specialized, walk_of)
from test_host_emu import ARM_HAND_CASES, COMPILERS, ROCM_CLANG, _ptr, arm_hand_case, emu, folded_host_walk, host_walk  # noqa: F401  (emu is a fixture)

CASES = tuple(("id", g, d) for g, d in FLAGS) + (("nle", 1, 1), ("nle", 0, 0))
ID_CASES = CASES[:4]
LARGE_ANGLE_CASES = (("id", 1, 1), ("id", 0, 0), ("nle", 1, 1))
TWO_SAMPLE_MIN_TILES = 1024             # DRM_TWO_SAMPLE_MIN_TILES (csrc/drm_arm_dynamics.hip)
LAT2_MAX_TILES = 1024                   # DRM_LAT2_MAX_TILES (csrc/drm_arm_dynamics.hip), pairs of tiles
MISALIGNED_TILES = 64                   # csrc/drm_common.hpp
# joint columns whose truth is identically zero, by (robot, case kind): left out of `joint`, asserted against the truth
ZERO_COLUMNS = {("fetch", "nle"): (0, 1)}
# ... and the joints whose torque does not depend on q at all (the same two wheels: tau = I_zz qdd + d qd), asserted against the truth:
# on the row of an all-NaN q such an entry is non-finite OR carries the bits of the clean row (see FOUND)
Q_INDEPENDENT = {"fetch": (0, 1)}
FUSED_LINK = dict({r: links[0] for r, links in GOLDEN_ROBOTS}, fetch="gripper_link")
FUSED_ARMS = ARM_ROBOTS
# The cases in which a fast rung must NOT carry the loop kernel's bits.  rnea_arm_kernel and the loop kernels take the same steps link
# by link (rnea_chain_trig, rnea_tree_walk: rnea_link_motion, rnea_body_force, rnea_link_force_up); what differs is the damping term —
# a separately rounded product behind a select in the arm rung, one FMA in the loop form — so the two are bit-identical by construction
# where damping is off, zero (panda_no_gripper) or a power of two (iiwa7: 0.5) and must differ on fetch_arm_no_gripper (1 and 5 N m s)
# with damping on.  trifinger_edu (no damping) differs from the loop form only where gravity or qdd enter.  The other cases are printed.
BOTH = (("id", 1, 1), ("nle", 0, 0))
MUST_DIFFER_FROM_LOOP = dict(panda_no_gripper=(), iiwa7=(), fetch_arm_no_gripper=BOTH[:1], allegro_left=BOTH, trifinger_edu=BOTH[:1],
                             panda=BOTH, jaco=BOTH, iiwa7_allegro=BOTH)


# ------------------------------------------------------------------------------------------------------------------- truth
def quat_error(a, b):
    """max |a - b| with the sign of a row taken from b where b is within 1e-5 of a case boundary (helpers.quat_close)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    near = (quat_branch_margin(b) <= 1e-5)[..., None]
    sgn = np.sign((a * b).sum(-1, keepdims=True))
    sgn[sgn == 0] = 1.0
    return float(np.abs(a * np.where(near, sgn, 1.0) - b).max())


def tau_errors(X, case, idx=None):
    """(row, joint) of the torques X [N, n] against the truth rows idx [N] (None: the 256 rows in order) — one vectorised expression"""
    X = np.asarray(X, np.float64)
    T = case["tau64"]
    idx = np.arange(X.shape[0]) % ROWS if idx is None else idx
    assert X.shape == (len(idx), T.shape[1])
    d = np.abs(X - T[idx])
    row = float((d.max(axis=1) / np.abs(T).max(axis=1)[idx]).max())
    keep = case["columns"]
    return dict(row=row, joint=float((d.max(axis=0)[keep] / np.abs(T).max(axis=0)[keep]).max()))


def pose_errors(pos, quat, t, idx=None):
    pos = np.asarray(pos, np.float64)
    idx = np.arange(pos.shape[0]) % ROWS if idx is None else idx
    assert pos.shape == (len(idx), 3) and np.shape(quat) == (len(idx), 4)
    return dict(pos=float(np.abs(pos - t["pos64"][idx]).max() / np.abs(t["pos64"]).max()), quat=quat_error(quat, t["quat64"][idx]))


def build_truth(spec, robot, q, qd, qdd, link):
    orc = Oracle(spec)
    q64, qd64, qdd64, z = q.astype(np.float64), qd.astype(np.float64), qdd.astype(np.float64), np.zeros(q.shape)
    t = dict(q=q, qd=qd, qdd=qdd, cases={})
    for kind, g, d in CASES:
        tau64 = orc.rnea(q64, qd64, qdd64 if kind == "id" else z, g, d, np.float64)
        # the truth itself, before anything under test
        assert tau64.dtype == np.float64 and (np.abs(tau64).max(axis=1) > 0).all(), (robot, kind, g, d)
        zero = tuple(int(c) for c in np.nonzero(np.abs(tau64).max(axis=0) == 0)[0])
        assert zero == ZERO_COLUMNS.get((robot, kind), ()), (robot, kind, g, d, zero)
        case = dict(tau64=tau64, columns=np.array([c for c in range(q.shape[1]) if c not in zero]))
        tau32 = orc.rnea(q, qd, qdd if kind == "id" else z.astype(np.float32), g, d, np.float32)
        assert tau32.dtype == np.float32
        case["yard"] = tau_errors(tau32, case)
        t["cases"][(kind, g, d)] = case
    pos64, quat64 = orc.fk(q64, [link], np.float64)
    pos32, quat32 = orc.fk(q, [link], np.float32)
    assert pos32.dtype == np.float32 and np.abs(pos64).max() > 0
    t.update(pos64=pos64[:, 0], quat64=quat64[:, 0])
    t["yard_pose"] = pose_errors(pos32[:, 0], quat32[:, 0], t)
    return t


def link_index(m, robot):
    return m._name_to_idx_map[FUSED_LINK[robot]]


@functools.lru_cache(maxsize=None)
def truth(robot, seed):
    m = model_on(robot)
    t = build_truth(m._spec, robot, *sample_states(m, ROWS, seed=seed), link_index(m, robot))
    t["seed"] = seed
    return t


@functools.lru_cache(maxsize=None)
def truth_large_angle(robot):
    """seed 61 with one joint of rows 2 and 77 at +-4.0e5 (the float32 value is what the truth sees)"""
    m = model_on(robot)
    q, qd, qdd = sample_states(m, ROWS, seed=61)
    q = q.copy()
    q[2, min(5, q.shape[1] - 1)] = BIG_ANGLE
    q[77, 0] = -BIG_ANGLE
    t = build_truth(m._spec, robot, q, qd, qdd, link_index(m, robot))
    t["seed"] = 61
    return t


# ------------------------------------------------------------------------------------------------------------------- checks
def line(robot, path, flags, kind, seed, metric, e, ey):
    print("RNEARUNG %-34s %-30s %s %-3s %2d %-5s %.3e %.3e %.2f" % (robot, path, flags, kind, seed, metric, e, ey, e / ey))


def host(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)


def check_tau(robot, path, t, case, X, idx=None):
    kind, g, d = case
    c = t["cases"][case]
    X = host(X)
    assert X.dtype == np.float32 and np.isfinite(X).all()
    e, failures = tau_errors(X, c, idx), []
    for metric in ("row", "joint"):
        ey = max(c["yard"][metric], FLOOR)
        line(robot, path, "g%dd%d" % (g, d), kind, t["seed"], metric, e[metric], ey)
        if not e[metric] <= MARGIN * ey:
            failures.append((metric, e[metric], ey))
    assert not failures, (robot, path, case, failures)


def check_pose(robot, path, t, pos, quat, idx=None):
    pos, quat = host(pos), host(quat)
    assert pos.dtype == np.float32 and quat.dtype == np.float32 and np.isfinite(pos).all() and np.isfinite(quat).all()
    e, failures = pose_errors(pos, quat, t, idx), []
    for metric in ("pos", "quat"):
        ey = max(t["yard_pose"][metric], FLOOR)
        line(robot, path, "----", "fk", t["seed"], metric, e[metric], ey)
        if not e[metric] <= MARGIN * ey:
            failures.append((metric, e[metric], ey))
    assert not failures, (robot, path, failures)


def same_bits(a, b, expect, what):
    """Two rungs with different arithmetic must differ somewhere, two launches of one kernel must not."""
    equal = bool(torch.equal(a, b)) if isinstance(a, torch.Tensor) else bool(np.array_equal(a, b))
    note = ""
    if not equal and isinstance(a, torch.Tensor) and a.shape == b.shape:
        d = (a.double() - b.double()).abs()
        note = "  (%d of %d entries, largest %.3e of %.3e)" % (int((a != b).sum()), a.numel(), float(d.max()), float(b.abs().max()))
    print("RNEARUNG-BITS %-76s %s%s" % (what, "equal" if equal else "differ", note))
    assert expect is None or equal == expect, what      # (None: reported only — a pair that is bit-identical by construction)


# ------------------------------------------------------------------------------------------------------------------- runners
def inputs(t, case, device, rows=slice(None)):
    q, qd = dev(t["q"][rows], device), dev(t["qd"][rows], device)
    return q, qd, (dev(t["qdd"][rows], device) if case[0] == "id" else None)


def call_id(model, q, qd, qdd, g, d):
    if qdd is None:
        return model.compute_non_linear_effects(q, qd, include_gravity=bool(g), use_damping=bool(d))
    return model.compute_inverse_dynamics(q, qd, qdd, include_gravity=bool(g), use_damping=bool(d))


def api_tau(model, t, case, B=None):
    """the public call over the 256 rows in consecutive launches of B rows (None: one launch); q, qd, qdd stay as they were"""
    _, g, d = case
    q, qd, qdd = inputs(t, case, model._device)
    keep = [x.clone() for x in (q, qd, qdd) if x is not None]
    B = B or ROWS
    out = torch.cat([call_id(model, q[i:i + B], qd[i:i + B], None if qdd is None else qdd[i:i + B], g, d) for i in range(0, ROWS, B)])
    assert all(torch.equal(a, b) for a, b in zip(keep, (x for x in (q, qd, qdd) if x is not None))), "the caller's tensors are not modified"
    assert out.shape == q.shape and out.dtype == torch.float32 and out.grad_fn is None
    return out


def api_fused(model, robot, t, case, B=None):
    _, g, d = case
    q, qd, qdd = inputs(t, case, model._device)
    keep = [x.clone() for x in (q, qd, qdd)]
    B = B or ROWS
    outs = [model.compute_fk_and_inverse_dynamics(q[i:i + B], qd[i:i + B], qdd[i:i + B], FUSED_LINK[robot], bool(g), bool(d)) for i in range(0, ROWS, B)]
    assert all(torch.equal(a, b) for a, b in zip(keep, (q, qd, qdd)))
    return tuple(torch.cat([o[k] for o in outs]) for k in range(3))


def api_everything(model, robot, path, seed, B=None, t=None, cases=CASES, fused=True):
    """all six cases of one seed through the public API, and the fused call on the "id" cases; the outputs by case (the poses under "pose")"""
    t, outs = t or truth(robot, seed), {}
    for case in cases:
        outs[case] = api_tau(model, t, case, B)
        check_tau(robot, path, t, case, outs[case])
        if fused and case[0] == "id":
            tau, pos, quat = api_fused(model, robot, t, case, B)
            check_tau(robot, "fused:" + path, t, case, tau)
            check_pose(robot, "fused:" + path, t, pos, quat)
            same_bits(tau, outs[case], True, "%s %s B=%s %s fused tau vs compute_inverse_dynamics" % (robot, path, B, case))
            if "pose" in outs:
                assert torch.equal(pos, outs["pose"][0]) and torch.equal(quat, outs["pose"][1]), "the pose does not see the flags"
            outs["pose"] = (pos, quat)
    if fused and robot in FUSED_ARMS and "pose" in outs:
        q = dev(t["q"], model._device)
        BB = B or ROWS
        fk = [model.compute_forward_kinematics(q[i:i + BB], FUSED_LINK[robot]) for i in range(0, ROWS, BB)]
        same_bits(outs["pose"][0], torch.cat([f[0] for f in fk]), True, "%s %s B=%s fused pos vs compute_forward_kinematics" % (robot, path, B))
        same_bits(outs["pose"][1], torch.cat([f[1] for f in fk]), True, "%s %s B=%s fused quat vs compute_forward_kinematics" % (robot, path, B))
    return outs


def abi_rnea(walk, q, qd, qdd, flags, out=None, aligned_query=False):
    """drm_rnea on the tensors as they are (views included); the scratch sized by drm_rnea_scratch_floats (any pointers)"""
    from differentiable_robot_model_amd import backend
    lib, stream = library_and_stream(q.device)
    B, n = q.shape
    query = lib.drm_rnea_scratch_floats_aligned if aligned_query else lib.drm_rnea_scratch_floats
    query.restype = ctypes.c_int64
    need = int(query(ctypes.byref(walk), ctypes.c_int64(B)))
    scratch = torch.empty(max(need, 4), device=q.device)
    out = torch.full((B, n), float("nan"), device=q.device) if out is None else out
    backend._check(lib.drm_rnea(ctypes.byref(walk), ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(qd.data_ptr()),
                                ctypes.c_void_p(qdd.data_ptr()) if qdd is not None else None, ctypes.c_int64(B), flags,
                                ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), stream), lib)
    return out


def abi_everything(walk, device, robot, path, seed, B=None, t=None, cases=CASES):
    """the same through the C ABI, in consecutive launches of B rows (None: one launch) on 16-byte aligned copies of the slices"""
    t, outs = t or truth(robot, seed), {}
    B = B or ROWS
    for case in cases:
        q, qd, qdd = inputs(t, case, device)
        outs[case] = torch.cat([abi_rnea(walk, q[i:i + B].clone(), qd[i:i + B].clone(), None if qdd is None else qdd[i:i + B].clone(),
                                         case[1] | (case[2] << 1)) for i in range(0, ROWS, B)])
        check_tau(robot, path, t, case, outs[case])
    return outs


def abi_edges(walk, device, robot, path, B):
    """zero input and the |q| = 4.0e5 rows through the C ABI"""
    q = dev(truth(robot, 61)["q"][:B], device)
    z = torch.zeros_like(q)
    for flags in (0, 2):
        assert (abi_rnea(walk, q, z, z.clone(), flags) == 0).all() and (abi_rnea(walk, q, z, None, flags) == 0).all(), "at rest, no gravity: no torque"
    abi_everything(walk, device, robot, path + "-4e5", 61, B, t=truth_large_angle(robot), cases=LARGE_ANGLE_CASES)


def emu_everything(emu, walk, robot, path, seed, fn="emu_rnea", t=None, cases=CASES):
    t, outs = t or truth(robot, seed), {}
    q, qd, qdd = (np.ascontiguousarray(t[k]) for k in ("q", "qd", "qdd"))
    B, n = q.shape
    for case in cases:
        out = np.full((B, n), np.nan, np.float32)
        assert getattr(emu, fn)(ctypes.byref(walk), _ptr(q), _ptr(qd), _ptr(qdd) if case[0] == "id" else None, ctypes.c_int64(B),
                                case[1] | (case[2] << 1), _ptr(out)) == 0
        check_tau(robot, path, t, case, out)
        outs[case] = out
    return outs


def emu_edges(emu, walk, robot, path, fn="emu_rnea"):
    """zero input and the |q| = 4.0e5 rows on an emulated path"""
    q = np.ascontiguousarray(truth(robot, 61)["q"])
    z = np.zeros_like(q)
    for flags in (0, 2):
        for acc in (_ptr(z), None):
            out = np.full(q.shape, np.nan, np.float32)
            assert getattr(emu, fn)(ctypes.byref(walk), _ptr(q), _ptr(z), acc, ctypes.c_int64(len(q)), flags, _ptr(out)) == 0
            assert (out == 0).all(), "at rest, no gravity: no torque"
    emu_everything(emu, walk, robot, path + "-4e5", 61, fn, t=truth_large_angle(robot), cases=LARGE_ANGLE_CASES)


# ------------------------------------------------------------------------------------------------------------------- edges (any device)
def zero_input_check(model, robot, B):
    n, device = model._n_dofs, model._device
    q = dev(sample_states(model, B, seed=61)[0], device)
    z = torch.zeros(B, n, device=device)
    for damp in (False, True):
        assert (model.compute_inverse_dynamics(q, z, z.clone(), include_gravity=False, use_damping=damp) == 0).all(), "at rest, no gravity: no torque"
        assert (model.compute_non_linear_effects(q, z, include_gravity=False, use_damping=damp) == 0).all()
        assert (model.compute_fk_and_inverse_dynamics(q, z, z.clone(), FUSED_LINK[robot], False, damp)[0] == 0).all()


def outputs_where_given_check(model, robot, B):
    """through the C ABI: tau pre-filled with NaN in an allocation one row longer than the launch"""
    t = truth(robot, 61)
    device, n = model._device, model._n_dofs
    walk = walk_of(model)
    q, qd, qdd = (dev(t[k][:B], device) for k in ("q", "qd", "qdd"))
    keep = [x.clone() for x in (q, qd, qdd)]
    for acc in (qdd, None):
        tau = torch.full((B + 1, n), float("nan"), device=device)
        tau[B] = -7.25
        abi_rnea(walk, q, qd, acc, 3, out=tau[:B])
        assert not torch.isnan(tau[:B]).any() and (tau[B] == -7.25).all()
        assert all(torch.equal(a, b) for a, b in zip(keep, (q, qd, qdd)))
        # ... and they are what the public API returns
        assert torch.equal(tau[:B], call_id(model, q, qd, acc, 1, 1))


def large_angle_check(model, robot, path, B=None):
    api_everything(model, robot, path, 61, B, t=truth_large_angle(robot), cases=LARGE_ANGLE_CASES, fused=robot not in FUSED_ARMS or (B or ROWS) <= ROWS)


@functools.lru_cache(maxsize=None)
def q_independent_columns(robot):
    """the joints whose torque does not see q at all, from the truth: tau64 of seed 61 with the q of seed 7 in its place"""
    m = model_on(robot)
    (q, qd, qdd), q7 = sample_states(m, ROWS, seed=61), sample_states(m, ROWS, seed=7)[0]
    orc = Oracle(m._spec)
    a, b = (orc.rnea(x.astype(np.float64), qd.astype(np.float64), qdd.astype(np.float64), True, True, np.float64) for x in (q, q7))
    cols = tuple(int(c) for c in np.nonzero(np.abs(a - b).max(axis=0) <= 1e-12 * np.abs(a).max(axis=0))[0])
    assert cols == Q_INDEPENDENT.get(robot, ()), (robot, cols)
    return cols


def nan_row_check(robot, got, clean):
    """the row of an all-NaN q: non-finite in every entry; a Q_INDEPENDENT entry may instead carry the bits of the clean row"""
    free = q_independent_columns(robot)
    for c in range(got.shape[0]):
        assert not torch.isfinite(got[c]) or (c in free and torch.equal(got[c], clean[c])), (robot, c, float(got[c]), float(clean[c]))


def non_finite_rows_check(model, robot):
    """an all-NaN q row and an all-Inf qdd row: non-finite in every entry, no bit of another row changes; both in full tiles (128 rows)
    and both in the ragged tail (127 rows: its second tile has 63)"""
    t = truth(robot, 61)
    device = model._device
    for B, (r_nan, r_inf) in ((128, (5, 70)), (127, (70, 100))):
        q, qd, qdd = (dev(t[k][:B], device) for k in ("q", "qd", "qdd"))
        run = lambda: (model.compute_inverse_dynamics(q, qd, qdd, include_gravity=True, use_damping=True),
                       model.compute_fk_and_inverse_dynamics(q, qd, qdd, FUSED_LINK[robot], True, True)[0])
        clean = run()
        q[r_nan] = float("nan")
        qdd[r_inf] = float("inf")
        got = run()
        others = torch.ones(B, dtype=torch.bool, device=device)
        others[[r_nan, r_inf]] = False
        for a, b in zip(got, clean):
            assert torch.equal(a[others], b[others]) and torch.isfinite(a[others]).all(), (robot, B)
            assert not torch.isfinite(a[r_inf]).any(), (robot, B)
            nan_row_check(robot, a[r_nan], b[r_nan])


def interface_check(model, robot, B):
    """compute_non_linear_effects == compute_inverse_dynamics with a zero qdd tensor; 1-D arguments; a column-slice q"""
    t = truth(robot, 61)
    device, n = model._device, model._n_dofs
    q, qd, qdd = (dev(t[k][:B], device) for k in ("q", "qd", "qdd"))
    z = torch.zeros_like(q)
    tau = {(g, d): model.compute_inverse_dynamics(q, qd, qdd, include_gravity=bool(g), use_damping=bool(d)) for g, d in FLAGS}
    for g, d in FLAGS:
        nle = model.compute_non_linear_effects(q, qd, include_gravity=bool(g), use_damping=bool(d))
        assert torch.equal(nle, model.compute_inverse_dynamics(q, qd, z, include_gravity=bool(g), use_damping=bool(d))), (robot, g, d)
    assert torch.equal(model.compute_inverse_dynamics(q, qd, qdd), tau[(1, 1)]), "both flags default to True"
    # unbatched: the rows of one-row launches (the loop kernel); the batched call of the same single row gives the same bits
    for r in (0, B - 1):
        one = model.compute_inverse_dynamics(q[r], qd[r], qdd[r], include_gravity=True, use_damping=True)
        assert one.shape == (n,) and torch.equal(one, model.compute_inverse_dynamics(q[r:r + 1].clone(), qd[r:r + 1].clone(), qdd[r:r + 1].clone(), True, True)[0])
        one = model.compute_non_linear_effects(q[r], qd[r])
        assert one.shape == (n,) and torch.equal(one, model.compute_non_linear_effects(q[r:r + 1].clone(), qd[r:r + 1].clone())[0])
    # a column slice of a wider tensor
    wide = torch.full((B, n + 3), 9.5, device=device)
    wide[:, 2:2 + n] = q
    qs = wide[:, 2:2 + n]
    assert not qs.is_contiguous()
    assert torch.equal(model.compute_inverse_dynamics(qs, qd, qdd, include_gravity=True, use_damping=True), tau[(1, 1)])
    assert torch.equal(model.compute_non_linear_effects(qs, qd), model.compute_non_linear_effects(q, qd))
    fused = model.compute_fk_and_inverse_dynamics(q, qd, qdd, FUSED_LINK[robot], True, True)
    sliced = model.compute_fk_and_inverse_dynamics(qs, qd, qdd, FUSED_LINK[robot], True, True)
    assert all(torch.equal(a, b) for a, b in zip(fused, sliced)) and torch.equal(fused[0], tau[(1, 1)])
    # a row slice 4 n bytes off a 16-byte boundary (n odd): the rows of the aligned copy
    if n % 4:
        off = [x[1:] for x in (q, qd, qdd)]
        assert any(x.data_ptr() % 16 for x in off)
        for a, b in zip(model.compute_fk_and_inverse_dynamics(*off, FUSED_LINK[robot], True, True),
                        model.compute_fk_and_inverse_dynamics(*(x.clone() for x in off), FUSED_LINK[robot], True, True)):
            assert torch.equal(a, b)
    assert (wide[:, :2] == 9.5).all() and (wide[:, 2 + n:] == 9.5).all() and torch.equal(wide[:, 2:2 + n], q)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_host_build_against_truth(cpu_library, robot, seed):
    api_everything(model_on(robot), robot, "host", seed)


@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_host_build_edges(cpu_library, robot):
    m = model_on(robot)
    zero_input_check(m, robot, 65)
    outputs_where_given_check(m, robot, 65)
    interface_check(m, robot, 65)
    non_finite_rows_check(m, robot)
    large_angle_check(m, robot, "host-4e5")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_emu_loop_walks_against_truth(emu, robot, seed):
    """emu_rnea (csrc/drm_host_loops.hpp: the arithmetic of rnea_records_kernel) on the whole-tree walk and on the folded walk the API
    launches; emu_rnea_short (rnea_tree_walk_short<6>: the arithmetic of rnea_tree_kernel) where every segment has at most 6 ops"""
    m = model_on(robot)
    prog, fprog = build_walk(m._spec, whole_tree=True), build_walk(m._spec, whole_tree=True, drop_folded=True)   # (own the tables)
    walk, keep = host_walk(m, prog)
    fwalk, fkeep = folded_host_walk(m, fprog)
    paths = [(walk, prog, "emu-tree"), (fwalk, fprog, "emu-folded")]
    for w, p, name in paths:
        emu_everything(emu, w, robot, name, seed)
        short = max(b - a for a, b in zip(p.seg_begin, p.seg_begin[1:])) <= 6
        if short:
            emu_everything(emu, w, robot, name + "-short", seed, fn="emu_rnea_short")
        if seed == SEEDS[0]:
            emu_edges(emu, w, robot, name)
            if short:
                emu_edges(emu, w, robot, name + "-short", fn="emu_rnea_short")
    if robot in FINGER_ROBOTS + ("2link_robot",):
        assert max(b - a for a, b in zip(fprog.seg_begin, fprog.seg_begin[1:])) <= 6, "the robots of rnea_tree_kernel are emulated in its form"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ARM_ROBOTS)
def test_emu_arm_kernels_against_truth(emu, robot, seed):
    """rnea_arm_8_7<LINKS> / rnea_arm2_8_7<LINKS> (tests/host_emu/host_emu.cpp): the arithmetic of rnea_arm_kernel<8, 7, LINKS> and of
    rnea_arm2_kernel<8, 7, LINKS> on the folded walk (LINKS = 7, what the API launches) and on the whole table (LINKS = 8)"""
    m = model_on(robot)
    fprog, prog = build_walk(m._spec, whole_tree=True, drop_folded=True), build_walk(m._spec, whole_tree=True)      # (own the tables)
    assert (fprog.n_ops, prog.n_ops) == (7, 8)
    fwalk, fkeep = folded_host_walk(m, fprog)
    walk, keep = host_walk(m, prog)
    for fn, name in (("emu_rnea_arm", "emu-arm"), ("emu_rnea_arm2", "emu-arm2")):
        for w, links in ((fwalk, 7), (walk, 8)):
            emu_everything(emu, w, robot, "%s<8,7,%d>" % (name, links), seed, fn=fn)
            if seed == SEEDS[0]:
                emu_edges(emu, w, robot, "%s<8,7,%d>" % (name, links), fn=fn)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", FINGER_ROBOTS)
def test_emu_fingers_against_truth(emu, robot, seed):
    """rnea_fingers2_emu<L>: the arithmetic of rnea_fingers2_kernel"""
    m = model_on(robot)
    prog = build_walk(m._spec, whole_tree=True, drop_folded=True)
    assert prog.shape & SHAPE_FINGERS
    walk, keep = folded_host_walk(m, prog)
    emu_everything(emu, walk, robot, "emu-fingers", seed, fn="emu_rnea_fingers")
    if seed == SEEDS[0]:
        emu_edges(emu, walk, robot, "emu-fingers", fn="emu_rnea_fingers")


@functools.lru_cache(maxsize=None)
def arm_hand_truth(case, seed):
    """the truth of an ARM_HAND_CASES entry: "robot:sliding-fingers" is another model (prismatic fingers) of the same URDF"""
    m, prog, walk, keep = arm_hand_case(case)
    robot = case.split(":")[0].split("+")[0]
    q, qd, qdd = sample_states(m, ROWS, seed=61 if seed == "4e5" else seed)
    if seed == "4e5":
        q = q.copy()
        q[2, 5], q[77, 0] = BIG_ANGLE, -BIG_ANGLE
    t = build_truth(m._spec, robot, q, qd, qdd, link_index(m, robot))
    t["seed"] = 61 if seed == "4e5" else seed
    return t


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", ARM_HAND_CASES)
def test_emu_arm_hand_against_truth(emu, case, seed):
    """rnea_arm_hand_emu<P, L>: the arithmetic of rnea_arm_hand_kernel, on the three robots as the API folds them, on the Panda with
    sliding fingers and with a link kept as an op of its own"""
    m, prog, walk, keep = arm_hand_case(case)
    assert prog.shape & SHAPE_ARM_HAND
    emu_everything(emu, walk, case, "emu-arm-hand", seed, fn="emu_rnea_arm_hand", t=arm_hand_truth(case, seed))
    if seed == SEEDS[0]:
        q = np.ascontiguousarray(arm_hand_truth(case, seed)["q"])
        z = np.zeros_like(q)
        for flags in (0, 2):
            out = np.full(q.shape, np.nan, np.float32)
            assert emu.emu_rnea_arm_hand(ctypes.byref(walk), _ptr(q), _ptr(z), None, ctypes.c_int64(len(q)), flags, _ptr(out)) == 0 and (out == 0).all()
        emu_everything(emu, walk, case, "emu-arm-hand-4e5", seed, fn="emu_rnea_arm_hand", t=arm_hand_truth(case, "4e5"), cases=LARGE_ANGLE_CASES)


def fused_host_walks(m, robot, same):
    """(tree walk, chain walk) of drm_fk_rnea's arm rung: `same` — both the 8-op chain; else the folded 7-op tree walk and the chain walk
    on the folded table, as robot_model._compute_fk_and_inverse_dynamics builds them.  The tables stay alive in the returned list."""
    ee = link_index(m, robot)
    if same:
        prog, chain = build_walk(m._spec, whole_tree=True), build_walk(m._spec, targets=[ee])
        (tw, k0), (cw, k1) = host_walk(m, prog), host_walk(m, chain)
    else:
        fold = foldable_links(m._spec)
        prog, chain = build_walk(m._spec, whole_tree=True, drop_folded=True), build_walk(m._spec, targets=[ee], fold=fold)
        (tw, k0), (cw, k1) = folded_host_walk(m, prog), folded_host_walk(m, chain, fold)
    assert chain.n_ops == 8 and chain.shape & SHAPE_ARM_CHAIN and prog.n_ops == (8 if same else 7)
    return tw, cw, [prog, chain, k0, k1]


def emu_fused(emu, tw, cw, t, case):
    q, qd, qdd = (np.ascontiguousarray(t[k]) for k in ("q", "qd", "qdd"))
    tau, pos, quat = np.full((ROWS, 7), np.nan, np.float32), np.full((ROWS, 3), np.nan, np.float32), np.full((ROWS, 4), np.nan, np.float32)
    assert emu.emu_fk_rnea_arm(ctypes.byref(tw), ctypes.byref(cw), _ptr(q), _ptr(qd), _ptr(qdd) if case[0] == "id" else None, ctypes.c_int64(ROWS),
                               case[1] | (case[2] << 1), _ptr(tau), _ptr(pos), _ptr(quat)) == 0
    return tau, pos, quat


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", FUSED_ARMS)
def test_emu_fused_arm_against_truth(emu, robot, seed):
    """fk_rnea_arm_8_7<LINKS>: the arithmetic of fk_rnea_arm_kernel<8, 7, LINKS> — the pose chain over the tree walk's rows and the chain
    walk's fixed tail, then the sweeps — in both shapes of fk_rnea_arm_applies.  Its torques are those of emu_rnea_arm to the bit."""
    m = model_on(robot)
    for same in (True, False):
        tw, cw, keep = fused_host_walks(m, robot, same)
        path = "emu-fused<8,7,%d>" % (8 if same else 7)
        for t, cases, p in ((truth(robot, seed), CASES, path),) + (((truth_large_angle(robot), LARGE_ANGLE_CASES, path + "-4e5"),) if seed == SEEDS[0] else ()):
            for case in cases:
                tau, pos, quat = emu_fused(emu, tw, cw, t, case)
                check_tau(robot, p, t, case, tau)
                check_pose(robot, p, t, pos, quat)
                alone = np.full((ROWS, 7), np.nan, np.float32)
                q, qd, qdd = (np.ascontiguousarray(t[k]) for k in ("q", "qd", "qdd"))
                assert emu.emu_rnea_arm(ctypes.byref(tw), _ptr(q), _ptr(qd), _ptr(qdd) if case[0] == "id" else None, ctypes.c_int64(ROWS),
                                        case[1] | (case[2] << 1), _ptr(alone)) == 0
                assert np.array_equal(alone, tau)


@pytest.mark.parametrize("cxx", COMPILERS)
def test_static_source_of_fetch_against_truth(cpu_library, tmp_path, cxx):
    """static_rnea: Fetch's generated straight-line source (csrc/drm_static.hpp rnea_static_walk) compiled for the host"""
    from test_specialize import host_harness
    robot = "fetch"
    m = model_on(robot)
    dw = m._dynamics_walk()
    prog, n = dw.program, m._n_dofs
    st = host_harness(tmp_path, sp.walk_tree(prog), n, "g++" if cxx == "g++" else ROCM_CLANG)
    assert st.static_n_ops() == prog.n_ops
    ops_f = m._ops_f(dw).detach().contiguous()
    of, cb = ctypes.c_void_p(ops_f.data_ptr()), ctypes.c_int64(ROWS)

    def run(t, case, zero_state=False):
        q, qd, qdd = (np.ascontiguousarray(t[k]) for k in ("q", "qd", "qdd"))
        if zero_state:
            qd, qdd = np.zeros_like(qd), np.zeros_like(qdd)
        out = np.full((ROWS, n), np.nan, np.float32)
        assert st.static_rnea(of, _ptr(q), _ptr(qd), _ptr(qdd) if case[0] == "id" else None, cb, case[1] | (case[2] << 1), _ptr(out)) == 0
        return out
    for seed in SEEDS:
        for case in CASES:
            check_tau(robot, "static-source", truth(robot, seed), case, run(truth(robot, seed), case))
    tl = truth_large_angle(robot)
    for case in (("id", 0, 0), ("id", 0, 1), ("nle", 0, 0)):
        assert (run(tl, case, zero_state=True) == 0).all(), "at rest, no gravity: no torque"
    for case in LARGE_ANGLE_CASES:
        check_tau(robot, "static-source-4e5", tl, case, run(tl, case))


# ------------------------------------------------------------------------------------------------------------------- GPU
def rung_name(model, robot, B):
    """the rung(s) a launch of B aligned rows takes with the library's kernels (module docstring)"""
    fast = RUNGS.get(robot)
    tile = 128 if fast == "fingers" else 64
    if fast == "arm":
        fast = "arm<8,7,%d>" % model._dynamics_walk().program.n_ops
    if fast is None or B < tile:
        return "loop-B%d" % B
    return ("%s-B%d" % (fast, B)) if B % tile == 0 else ("%s+tail-B%d" % (fast, B))


def no_own_kernels(walk):
    return not any(walk.special[k] for k in (sp.SPECIAL_RNEA, sp.SPECIAL_RNEA_ARM, sp.SPECIAL_FK_RNEA_ARM))


@pytest.mark.gpu
@pytest.mark.parametrize("robot,B", [(r, B) for r in RUNG_ROBOTS for B in (1, 63, 64, 65, 131, 256) + ((128, 129) if r in FINGER_ROBOTS else ())])
def test_gpu_library_rungs_against_truth(robot, B):
    """own_kernels = "off": full tiles through the shape's kernel (the shape bit of the walk; every pointer of the public API is 16-byte
    aligned), the rest of the launch through the loop kernels; the fused call beside it.  (B = 128 and 129 are the hands': one 128-row
    tile of rnea_fingers2_kernel without and with a tail.)"""
    m = gpu_model(robot)
    prog = m._dynamics_walk().program
    assert no_own_kernels(walk_of(m)), "library kernels only"
    assert bool(prog.shape & SHAPE_ARM_CHAIN and m._n_dofs == 7) == (robot in ARM_ROBOTS) and bool(prog.shape & SHAPE_FINGERS) == (robot in FINGER_ROBOTS)
    assert bool(prog.shape & SHAPE_ARM_HAND) == (robot in ARM_HAND_ROBOTS)
    tile = 128 if robot in FINGER_ROBOTS else 64
    for seed in SEEDS:
        outs = api_everything(m, robot, rung_name(m, robot, B), seed, B)
        full = B // tile * tile
        if seed == 61 and full and B % tile:
            # rows of full tiles: the same bits with and without a tail behind them
            t = truth(robot, seed)
            for case in (("id", 1, 1), ("nle", 0, 0)):
                q, qd, qdd = inputs(t, case, "cuda:0", slice(0, full))
                same_bits(outs[case][:full], call_id(m, q, qd, qdd, case[1], case[2]), True, "%s %s full tiles of B=%d alone" % (robot, case, B))
        if seed == 61:
            again = api_tau(m, truth(robot, seed), ("id", 1, 1), B)
            same_bits(outs[("id", 1, 1)], again, True, "%s B=%d launched twice" % (robot, B))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARM_ROBOTS + FINGER_ROBOTS + ARM_HAND_ROBOTS)
def test_gpu_loop_kernels_on_the_walks_of_the_fast_rungs(robot):
    """The walk with its shape bit cleared through the C ABI: every row through rnea_tree_kernel (hands) or rnea_records_kernel (arms, arms
    with hands).  Different arithmetic from the fast rung: not its bits; the kernel of the fast rung's ragged tail: its bits."""
    m = gpu_model(robot)
    walk = walk_of(m, clear_shape=SHAPE_ARM_CHAIN | SHAPE_FINGERS | SHAPE_ARM_HAND)
    loop = abi_everything(walk, "cuda:0", robot, "loop-abi-B256", 61)
    abi_everything(walk, "cuda:0", robot, "loop-abi-B256", 7)
    abi_edges(walk, "cuda:0", robot, "loop-abi", 256)
    fast = api_everything(m, robot, rung_name(m, robot, 256), 61, fused=False)
    tile = 128 if robot in FINGER_ROBOTS else 64
    for case in BOTH:
        same_bits(loop[case], fast[case], False if case in MUST_DIFFER_FROM_LOOP[robot] else None, "%s %s loop kernel vs %s" % (robot, case, RUNGS[robot]))
        # the ragged tail of a launch of one tile + 1 row is that row through the loop kernel
        q, qd, qdd = inputs(truth(robot, 61), case, "cuda:0", slice(0, tile + 1))
        same_bits(call_id(m, q, qd, qdd, case[1], case[2])[tile:], loop[case][tile:tile + 1], True, "%s %s tail row of B=%d vs loop kernel" % (robot, case, tile + 1))
    torch.cuda.synchronize()


def unfolded_walks(m):
    from differentiable_robot_model_amd import backend
    dt = m._get_walk(("tree",), whole_tree=True)
    assert dt.program.n_ops == 8 and dt.program.shape & SHAPE_ARM_CHAIN and m._dynamics_walk().program.n_ops == 7
    build = lambda: backend._walk_struct_build(dt.program, m._ops_f(dt).detach(), dt.ops_i, m._n_dofs)
    walk, loop_walk = build(), build()
    assert no_own_kernels(walk)
    loop_walk.shape = loop_walk.shape & ~SHAPE_ARM_CHAIN & 0xffffff
    return walk, loop_walk


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARM_ROBOTS)
def test_gpu_arm_kernel_on_the_unfolded_walk(robot):
    """rnea_arm_kernel<8, 7, 8>: the arm's whole-tree walk with all 8 links as ops through the C ABI (DRM_WALK_ARM_CHAIN, arm_links(w) ==
    8, full tiles, aligned pointers).  Full tiles alone and with a ragged tail; not the bits of the loop kernel on the same walk (its shape
    bit cleared), whose bits the tail row has."""
    m = gpu_model(robot)
    walk, loop_walk = unfolded_walks(m)
    outs = {}
    for B in (64, 256, 65, 131):
        for seed in SEEDS:
            outs[B, seed] = abi_everything(walk, "cuda:0", robot, "arm<8,7,8>%s-B%d" % ("+tail" if B % 64 else "", B), seed, B)
    abi_edges(walk, "cuda:0", robot, "arm<8,7,8>", 256)
    abi_edges(walk, "cuda:0", robot, "arm<8,7,8>+tail", 65)
    loop = abi_everything(loop_walk, "cuda:0", robot, "loop-abi-unfolded-B256", 61)
    for case in BOTH:
        same_bits(outs[256, 61][case], loop[case], False if case in MUST_DIFFER_FROM_LOOP[robot] else None,
                  "%s %s arm<8,7,8> vs loop kernel on the unfolded walk" % (robot, case))
        same_bits(outs[65, 61][case][:64], outs[256, 61][case][:64], True, "%s %s arm<8,7,8> full tile of B=65 alone" % (robot, case))
        same_bits(outs[65, 61][case][64:65], loop[case][64:65], True, "%s %s arm<8,7,8> tail row of B=65 vs loop kernel" % (robot, case))
    torch.cuda.synchronize()


@pytest.mark.gpu
@needs_hipcc
def test_gpu_own_kernel_rung_against_truth():
    """model.specialize() on Fetch: drm_rnea_static (special[DRM_SPECIAL_RNEA]) takes the full tiles at any pointer alignment, the library's
    loop kernel the tail.  Constants folded into the instruction stream: not the bits of the loop kernel."""
    robot = "fetch"
    m, special = specialized(robot)
    assert special.get(sp.SPECIAL_RNEA), "the walk carries its own kernel"
    lib_model = gpu_model(robot)
    for B in (64, 65, 256):
        for seed in SEEDS:
            outs = api_everything(m, robot, "own%s-B%d" % ("+tail" if B % 64 else "", B), seed, B)
        if B == 256:
            other = api_everything(lib_model, robot, "loop-B256", SEEDS[-1], B, fused=False)
            for case in (("id", 1, 1), ("nle", 0, 0)):
                same_bits(outs[case], other[case], False, "fetch %s own kernel vs loop kernel" % (case,))
    # a [1:] view through the C ABI: still the own kernel on the full tiles (its bits), the row in front untouched
    t, n = truth(robot, 61), m._n_dofs
    walk = walk_of(m)
    assert walk.special[sp.SPECIAL_RNEA]
    for case in (("id", 1, 1), ("nle", 0, 0)):
        q, qd, qdd = inputs(t, case, "cuda:0")
        out = torch.full((ROWS, n), float("nan"), device="cuda:0")
        views = [None if x is None else x[1:] for x in (q, qd, qdd, out)]
        assert all(v is None or v.data_ptr() % 16 for v in views)
        abi_rnea(walk, views[0], views[1], views[2], case[1] | (case[2] << 1), out=views[3])
        assert torch.isnan(out[0]).all(), "the row in front of the view is not written"
        check_tau(robot, "own-misaligned+tail-B255", t, case, out[1:], np.arange(1, ROWS))
        aligned = call_id(m, q[1:193].clone(), qd[1:193].clone(), None if qdd is None else qdd[1:193].clone(), case[1], case[2])
        same_bits(out[1:193], aligned, True, "fetch %s own kernel on a [1:] view vs aligned rows" % (case,))
    for B in (128, 65):
        zero_input_check(m, robot, B)
        outputs_where_given_check(m, robot, B)
        interface_check(m, robot, B)
    non_finite_rows_check(m, robot)
    large_angle_check(m, robot, "own-4e5")
    torch.cuda.synchronize()


def tiled(t, case, N, device="cuda:0"):
    """the 256 rows repeated cyclically to N rows"""
    idx = np.arange(N) % ROWS
    return idx, tuple(None if (k == "qdd" and case[0] != "id") else dev(t[k][idx], device) for k in ("q", "qd", "qdd"))


def repeats(out, N, period=ROWS):
    """rows share nothing: every repetition of the 256 rows carries the bits of the first"""
    reps = N // period
    return torch.equal(out[:reps * period].view(reps, period, -1), out[:period].expand(reps, -1, -1)) and torch.equal(out[reps * period:], out[:N - reps * period])


def sized_launch(model, robot, path, N, cases=(("id", 1, 1), ("id", 0, 0), ("nle", 1, 1)), fused=True, fused_bits=True):
    """every row of a launch of N tiled rows against its truth row: the three calls, the exact conditions, the |q| = 4.0e5 rows.
    `fused_bits`: whether the fused call must carry the bits of the separate calls (None: reported only)"""
    t, outs = truth(robot, 61), {}
    for case in cases:
        idx, (q, qd, qdd) = tiled(t, case, N)
        keep = [x.clone() for x in (q, qd, qdd) if x is not None]
        outs[case] = call_id(model, q, qd, qdd, case[1], case[2])
        assert all(torch.equal(a, b) for a, b in zip(keep, (x for x in (q, qd, qdd) if x is not None)))
        check_tau(robot, path, t, case, outs[case], idx)
        if fused and case[0] == "id":
            tau, pos, quat = model.compute_fk_and_inverse_dynamics(q, qd, qdd, FUSED_LINK[robot], bool(case[1]), bool(case[2]))
            check_tau(robot, "fused:" + path, t, case, tau, idx)
            check_pose(robot, "fused:" + path, t, pos, quat, idx)
            outs["fused", case] = tau
            same_bits(tau, outs[case], fused_bits, "%s %s %s fused tau vs compute_inverse_dynamics" % (robot, path, case))
            p2, r2 = model.compute_forward_kinematics(q, FUSED_LINK[robot])
            same_bits(torch.cat([pos, quat], 1), torch.cat([p2, r2], 1), fused_bits, "%s %s %s fused pose vs compute_forward_kinematics" % (robot, path, case))
    # exact conditions and the |q| = 4.0e5 rows
    tl, case = truth_large_angle(robot), ("id", 1, 1)
    idx, (q, qd, qdd) = tiled(tl, case, N)
    run = lambda: model.compute_inverse_dynamics(q, qd, qdd, include_gravity=True, use_damping=True)
    clean = run()
    check_tau(robot, path + "-4e5", tl, case, clean, idx)
    if fused:
        tau, pos, quat = model.compute_fk_and_inverse_dynamics(q, qd, qdd, FUSED_LINK[robot], True, True)
        check_tau(robot, "fused:" + path + "-4e5", tl, case, tau, idx)
        check_pose(robot, "fused:" + path + "-4e5", tl, pos, quat, idx)
        same_bits(tau, clean, fused_bits, "%s %s-4e5 fused tau vs compute_inverse_dynamics" % (robot, path))
        # (the sincos fallback is wave-uniform: the pose is the separate call's to the bit outside the waves of rows 2 and 77)
        p2, r2 = model.compute_forward_kinematics(q, FUSED_LINK[robot])
        plain = torch.ones(N, dtype=torch.bool, device=q.device)
        for r in (2, 77):
            plain &= torch.arange(N, device=q.device) % ROWS // 128 != r // 128
        same_bits(torch.cat([pos, quat], 1)[plain], torch.cat([p2, r2], 1)[plain], fused_bits, "%s %s-4e5 fused pose vs compute_forward_kinematics" % (robot, path))
    z = torch.zeros_like(q)
    assert (model.compute_inverse_dynamics(q, z, z.clone(), include_gravity=False, use_damping=False) == 0).all()
    assert (model.compute_non_linear_effects(q, z, include_gravity=False, use_damping=True) == 0).all()
    r_nan, r_inf = 5, N - 2
    q[r_nan] = float("nan")
    qdd[r_inf] = float("inf")
    got = run()
    others = torch.ones(N, dtype=torch.bool, device=q.device)
    others[[r_nan, r_inf]] = False
    assert torch.equal(got[others], clean[others]) and torch.isfinite(got[others]).all()
    assert not torch.isfinite(got[r_inf]).any()
    nan_row_check(robot, got[r_nan], clean[r_nan])
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARM_ROBOTS)
def test_gpu_two_samples_per_lane_rung(robot):
    """1 027 tiles + 17 rows with own_kernels = "off": more than DRM_TWO_SAMPLE_MIN_TILES tiles, so 513 pairs go through rnea_arm2_kernel /
    fk_rnea_arm2_kernel (latency form), the odd tile through the one-sample kernel, the tail through the loop kernel — on the API's folded
    walk and, through the C ABI, on the unfolded 8-op walk.  Every row against its truth row."""
    m = gpu_model(robot)
    assert no_own_kernels(walk_of(m))
    N = (TWO_SAMPLE_MIN_TILES + 3) * 64 + 17
    pairs = N // 128 * 128
    outs = sized_launch(m, robot, "arm2<8,7,7>+odd+tail", N)
    t = truth(robot, 61)
    for case, out in outs.items():
        if case[0] == "fused":
            continue
        q, qd, qdd = inputs(t, case, "cuda:0")
        one = call_id(m, q, qd, qdd, case[1], case[2])
        # (rnea_chain2_trig keeps the association order of the one-sample form: the same bits by construction — reported, not asserted)
        same_bits(out[:256], one, None, "%s %s two samples per lane vs one" % (robot, case))
        same_bits(out[pairs:pairs + 64], one[pairs % ROWS:pairs % ROWS + 64], True, "%s %s the odd tile is the one-sample kernel's" % (robot, case))
        assert repeats(out[:pairs], pairs)
    walk, loop_walk = unfolded_walks(m)
    for case in (("id", 1, 1), ("nle", 0, 0)):
        idx, (q, qd, qdd) = tiled(t, case, N)
        out = abi_rnea(walk, q, qd, qdd, case[1] | (case[2] << 1))
        check_tau(robot, "arm2<8,7,8>+odd+tail", t, case, out, idx)
        one = abi_rnea(walk, q[:256].clone(), qd[:256].clone(), None if qdd is None else qdd[:256].clone(), case[1] | (case[2] << 1))
        same_bits(out[:256], one, None, "%s %s two samples per lane vs one, unfolded walk" % (robot, case))
    torch.cuda.synchronize()


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7"])
def test_gpu_arm_own_kernels_and_the_throughput_form(robot):
    """specialize() on a 7-DoF arm: drm_rnea_arm_static and drm_fk_rnea_arm_static take launches of at least DRM_ARM_STATIC_MIN_PAIRS (1 024)
    pairs of tiles — 1 024 pairs + one odd tile (the library's one-sample kernel) + 3 rows (the loop kernel).  Below that size the
    specialized model runs the library's arm rung: its bits.  With own_kernels = "off" the same size is rnea_arm2_kernel's latency form
    (n2 = 1 024 = DRM_LAT2_MAX_TILES) and one more pair its throughput form: constants folded in or not, forces parked or not — not each
    other's bits."""
    m, special = specialized(robot)
    assert special.get(sp.SPECIAL_RNEA_ARM)
    lib_model = gpu_model(robot)
    assert no_own_kernels(walk_of(lib_model))
    t = truth(robot, 61)
    N = 2 * 64 * ARM_STATIC_MIN_PAIRS + 64 + 3
    own = sized_launch(m, robot, "arm-own+odd+tail", N, fused_bits=None)
    assert (getattr(m._dynamics_walk().program, "_special", None) or {}).get(sp.SPECIAL_FK_RNEA_ARM), "the fused call built its own kernel"
    lat = sized_launch(lib_model, robot, "arm2-lat<8,7,7>+odd+tail", N, fused=False)
    assert LAT2_MAX_TILES == ARM_STATIC_MIN_PAIRS
    thr = sized_launch(lib_model, robot, "arm2-thr<8,7,7>+odd+tail", N + 128)
    for case in lat:
        same_bits(own[case][:ROWS], lat[case][:ROWS], False, "%s %s arm-own vs arm (two samples per lane, latency form)" % (robot, case))
        same_bits(own[case][N - 67:], lat[case][N - 67:], True, "%s %s odd tile and tail behind arm-own are the library's" % (robot, case))
        q, qd, qdd = inputs(t, case, "cuda:0")
        same_bits(call_id(m, q, qd, qdd, case[1], case[2]), call_id(lib_model, q, qd, qdd, case[1], case[2]), True,
                  "%s %s a small launch of the specialized model is the library's arm rung" % (robot, case))
        assert repeats(thr[case][:N + 128 - 67], N + 128 - 67) and repeats(own[case][:N - 67], N - 67)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_persistent_grid_with_more_tiles_than_blocks():
    """Fetch with own_kernels = "off" (no shape bit, 14 ops, a segment of more than 6): rnea_records_kernel on 2 049 full tiles + 3 rows, more
    tiles than the device holds blocks (rnea_records_plan's resident count, asserted below through the scratch query: it sizes the records
    for min(tiles, resident) blocks), so blocks walk a second tile.  Every row against its truth row."""
    robot = "fetch"
    m = gpu_model(robot)
    walk = walk_of(m)
    assert no_own_kernels(walk) and not walk.shape & (SHAPE_ARM_CHAIN | SHAPE_FINGERS | SHAPE_ARM_HAND)
    N = 2049 * 64 + 3
    lib, _ = library_and_stream(torch.device("cuda:0"))
    lib.drm_rnea_scratch_floats.restype = ctypes.c_int64
    per_block = int(lib.drm_rnea_scratch_floats(ctypes.byref(walk), ctypes.c_int64(1)))
    resident = int(lib.drm_rnea_scratch_floats(ctypes.byref(walk), ctypes.c_int64(N))) // per_block
    print("RNEARUNG-RESIDENT fetch rnea_records_kernel %d blocks, %d tiles" % (resident, 2050))
    assert per_block > 0 and 0 < resident < 2050, "more tiles than resident blocks"
    outs = sized_launch(m, robot, "loop-persistent", N, fused=False)
    for out in outs.values():
        assert repeats(out, N)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "panda"])
def test_gpu_misaligned_call_beyond_the_capped_grid(robot):
    """A [1:] view of 65 * 64 + 1 rows through the C ABI: q, qd, qdd and tau start 4 n bytes off a 16-byte boundary (n = 7, 9), so the
    straight-line kernels of these walks do not apply and rnea_records_kernel runs all 65 tiles on a grid capped at MISALIGNED_TILES = 64
    blocks, its scratch sized by drm_rnea_scratch_floats: block 0 walks a second tile.  The bits of the loop kernel on the aligned rows."""
    m = gpu_model(robot)
    n = m._n_dofs
    N = (MISALIGNED_TILES + 1) * 64 + 1
    t = truth(robot, 61)
    walk = walk_of(m)
    assert walk.shape & (SHAPE_ARM_CHAIN | SHAPE_ARM_HAND)
    loop_walk = walk_of(m, clear_shape=SHAPE_ARM_CHAIN | SHAPE_ARM_HAND)
    idx = (np.arange(N) % ROWS)[1:]
    for case in (("id", 1, 1), ("id", 0, 0), ("nle", 1, 1)):
        _, (q, qd, qdd) = tiled(t, case, N)
        out = torch.full((N, n), float("nan"), device="cuda:0")
        views = [None if x is None else x[1:] for x in (q, qd, qdd, out)]
        assert all(v is None or v.data_ptr() % 16 for v in views)
        abi_rnea(walk, views[0], views[1], views[2], case[1] | (case[2] << 1), out=views[3])
        assert torch.isnan(out[0]).all(), "the row in front of the view is not written"
        check_tau(robot, "loop-misaligned", t, case, out[1:], idx)
        aligned = abi_rnea(loop_walk, q[1:257].clone(), qd[1:257].clone(), None if qdd is None else qdd[1:257].clone(), case[1] | (case[2] << 1))
        same_bits(out[1:257], aligned, True, "%s %s misaligned call vs the loop kernel on aligned rows" % (robot, case))
        assert repeats(out[1:], N - 1)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", FUSED_ARMS)
def test_gpu_fused_kernel_where_the_tree_walk_is_the_chain(robot):
    """drm_fk_rnea through the C ABI with the unfolded 8-op walk as tree AND chain (`same` of fk_rnea_arm_applies: fk_rnea_arm_kernel<8, 7,
    8>), full tiles and a ragged tail (drm_fk + drm_rnea on the rest).  tau: the bits of drm_rnea on that walk."""
    from differentiable_robot_model_amd import backend
    m = gpu_model(robot)
    walk, _ = unfolded_walks(m)
    ee = link_index(m, robot)
    assert m._get_walk(("tree",), whole_tree=True).program.op_of_link.get(ee, -1) == 7, "the target is the walk's last op"
    dc = m._get_walk(("chain", ee), targets=[ee])
    assert dc.program.n_ops == 8 and dc.program.shape & SHAPE_ARM_CHAIN
    chain = backend._walk_struct_build(dc.program, m._ops_f(dc).detach(), dc.ops_i, m._n_dofs)
    assert chain.target_perm == 2
    lib, stream = library_and_stream(torch.device("cuda:0"))
    for seed in SEEDS:
        t = truth(robot, seed)
        for B in (256, 65):
            for case in ID_CASES:
                q, qd, qdd = inputs(t, case, "cuda:0", slice(0, B))
                tau, pos, quat = (torch.full((B, k), float("nan"), device="cuda:0") for k in (7, 3, 4))
                lib.drm_rnea_scratch_floats.restype = ctypes.c_int64
                scratch = torch.empty(max(4, int(lib.drm_rnea_scratch_floats(ctypes.byref(walk), ctypes.c_int64(B)))), device="cuda:0")
                backend._check(lib.drm_fk_rnea(ctypes.byref(walk), ctypes.byref(chain), 7, ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(qd.data_ptr()),
                                               ctypes.c_void_p(qdd.data_ptr()), ctypes.c_int64(B), case[1] | (case[2] << 1), ctypes.c_void_p(tau.data_ptr()),
                                               ctypes.c_void_p(pos.data_ptr()), ctypes.c_void_p(quat.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), stream), lib)
                path = "fused-same<8,7,8>%s-B%d" % ("+tail" if B % 64 else "", B)
                idx = np.arange(B)
                check_tau(robot, path, t, case, tau, idx)
                check_pose(robot, path, t, pos, quat, idx)
                same_bits(tau, abi_rnea(walk, q, qd, qdd, case[1] | (case[2] << 1)), True, "%s %s %s tau vs drm_rnea" % (robot, path, case))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_gpu_edges(robot):
    """the exact conditions on the library's rungs: 128 rows (full tiles) and 65 / 127 rows (a ragged tail)"""
    m = gpu_model(robot)
    for B in (128, 65):
        zero_input_check(m, robot, B)
        outputs_where_given_check(m, robot, B)
        interface_check(m, robot, B)
    non_finite_rows_check(m, robot)
    large_angle_check(m, robot, "gpu-4e5-B256")
    if robot in ("panda_no_gripper", "allegro_left", "panda", "fetch"):
        large_angle_check(m, robot, "gpu-4e5-B3", B=3)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", [r for r in ALL_ROBOTS if r not in RUNG_ROBOTS])
def test_gpu_remaining_robots_against_truth(robot):
    """the robots that share a rung with one of RUNG_ROBOTS (the small-damping variants, jaco_clean): full tiles and a fast rung + tail"""
    m = gpu_model(robot)
    for B in (65, 256):
        for seed in SEEDS:
            api_everything(m, robot, "library-B%d" % B, seed, B)
    torch.cuda.synchronize()

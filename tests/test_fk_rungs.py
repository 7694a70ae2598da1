"""Forward kinematics and the geometric Jacobian on every rung of their dispatch (csrc/drm_fk_jacobian.hip drm_fk_jacobian, csrc/drm_fk.hip
drm_fk and drm_fk_fanout; DifferentiableRobotModel.compute_fk_and_jacobian / compute_endeffector_jacobian / plan_fk_and_jacobian /
compute_forward_kinematics / compute_forward_kinematics_all_links / _fk_targets), column by column against fp64.  Written in the manner of
tests/test_rnea_rungs.py and tests/test_fd_crba_rungs.py, whose helpers it shares.  The link-major calls (drm_fk_links,
drm_fk_fanout_links: compute_forward_kinematics_links, and compute_forward_kinematics_all_links on a device) stay with their own tests
(tests/test_gpu_parity.py, tests/test_links.py) and are out of scope; compute_forward_kinematics_all_links is still held to the
requirement here, on the host build and on the GPU, because that costs one call.

INPUTS: for every robot of helpers.ALL_ROBOTS 256 rows of sample_states(m, 256, seed=61) and a second set with seed=7; a third set "4e5":
seed 61 with one joint of rows 2 and 77 at +-4.0e5 (the fp64 argument reduction of the sine and cosine).  Two models whose joints
slide (reference_compat=False, loaded and judged as tests/test_joint_models.py does: the oracle on the model's own spec): "fetch:sliding"
to r_gripper_finger_link (the chain passes the prismatic torso joint and ends in a sliding finger) and "panda:sliding" to
panda_rightfinger (the last joint slides).  Host paths: every non-root link.  GPU: the links of GPU_LINKS, listed literally with the
kernel instantiation each is there for (asserted against the walk on the host as well) — every instantiation a shipped link reaches, the
last and the last-but-one link of the 7-DoF arms, one interior link per robot.  No shipped link has a walk that is NOT a serial chain of
at most 16 ops, so no link stands for "no fast path": the loop kernels are reached by size, alignment and through the C ABI instead.

TRUTH, from the fp64 oracle only: Oracle.fk(q64, all links) and Oracle.fk_jacobian(q64, link).  Asserted on the truth itself before
anything under test is compared (truth, jac_truth, test_truth_column_classes_and_lever_threshold): quat64 is unit to 1e-12; the pose
of fk_jacobian is the pose of fk to 1e-12; every DoF column of every (robot, link) is classified from the truth and the spec,
    off          the DoF is not on the chain: ang64 and lin64 identically zero
    prismatic    on the chain, ang64 == 0 and |lin64| == 1 to 1e-12 (and the spec says the joint slides) — looked at BEFORE zero-lever:
                 a sliding joint's own link has no lever and a unit column
    zero-lever   on the chain and lever_k == 0 (a link's own joint, a link fixed to it without an offset): lin64 identically zero
    revolute     everything else: |ang64| == 1 to 1e-12 and the lever identity lin64[:, :, k] == z_k x (p_e - p_k) to 1e-12 lever_k,
                 z_k from ang64, p_k the origin of the link that DoF k moves, lever_k = max_b |p_e - p_k| (Euclidean);
the per-robot counts of off and zero-lever columns, summed over the links, are kept literally (COLUMN_COUNTS: between 2 and 23 zero-lever
columns per robot) and asserted, as is the number of (row, column) pairs `rowlin` leaves out (ROWLIN_SKIPPED: none, on any robot and
seed, of between 768 and 53 248 pairs; the cap is 1 %).  The smallest non-zero lever is 0.0140 m (trifinger_edu), 0.0164 m on the hands.

METRICS, in fp64, the worst over the batch (errors: the largest of x, y, z):
    pos     per link    max_b |dpos| / max_b |pos64|; a link that never leaves the origin must be exactly there
    quat    per link    quat_error of tests/test_rnea_rungs.py: a row within its branch margin (1e-5) may flip sign, elsewhere a flip counts 2
    ang     per revolute or zero-lever column   max_b |dang|  (unit vectors: the scale is 1); the worst column
    lin     per revolute column max_b |dlin_k| / lever_k, per prismatic column max_b |dlin_k|; the worst column
    rowlin  per row     max_k |dlin_bk| / |p_e - p_k|_b over the revolute columns whose lever in that row exceeds 1e-3 lever_k
    exact   off columns of ang and lin, zero-lever columns of lin and prismatic columns of ang are == 0.0 — but see FOUND for the
            zero-lever columns of chain_fk_kernel, which are held to 2^-23 of the link's reach instead (CHAIN_ZERO_LEVER)
YARDSTICKS, not code under test: the same metrics of Oracle.fk_jacobian(float32) and Oracle.fk(float32) on the same rows.
REQUIREMENT: err(path) <= 8 max(err(yardstick), 2^-23) for each metric (8: the project's margin for a different summation order, as in
the two model modules).  No path needed a further yardstick.  Every comparison prints one "FKRUNG" line (robot, link, path, seed,
metric, error, yardstick, ratio) before it asserts; profiles/fk_rungs_tests.txt holds the worst of them per path and metric.

PATHS without a GPU: the device="cpu" model through the public calls (every non-root link, all links, the fingertips); the host emulation
under g++ and the ROCm clang — emu_fk and emu_fk_jacobian (csrc/drm_host_loops.hpp fk_loop, jac_loop: the loop kernels' arithmetic) on
the single-target walk of every non-root link, plain and as the API launches it (fixed links folded), emu_fk on the all-links walk and
on the all-links walk in walk order (fanned out behind a hub), emu_fk_jacobian_arm (fk_chain_pairs: the arm kernel's packed chain) on the
three 7-DoF arms.  Each of them also takes the |q| = 4.0e5 rows.

PATHS on the GPU (-m gpu), own_kernels = "off".  A launch of B rows is repeated over consecutive slices of the 256 rows (aligned copies),
so the statistic is over the same rows whatever B is: 64 and 256 full tiles, 65 and 131 a fast rung plus a ragged tail in the loop
kernel, 1 and 63 the loop kernel alone.
RUNGS (read off drm_fk_jacobian, drm_fk, drm_fk_fanout and their launchers):
    arm      DRM_WALK_ARM_CHAIN on a capacity-8 walk of a 7-DoF robot, target_perm == 2, every pointer (pos and quat included) 16-byte
             aligned, full tiles: fk_jacobian_arm_kernel<8, 7, JAC = true> — the register-resident form up to DRM_PRE_MAX_TILES (2 048)
             tiles, the plain form beyond, the streamed multi-wave form once the outputs pass 256 MiB (stream_past_llc); through drm_fk
             the FK-only instantiation (launch_fk_arm: the plain form at every size).  fetch_arm_no_gripper's wrist_roll_link carries
             the shape bit but a permuted target frame (target_perm != 2): chain<8,8>.
    chain    any other serial chain: chain_fk_kernel<CAP, USED, JAC, NT>.  Reached by shipped links, with and without JAC: <4,4> (1 - 4
             ops), <8,6> (5, 6), <8,8> (7, 8), <12,10> (9, 10), <12,12> (11, 12); NOT reachable: <16,14> and <16,16> (the longest shipped
             chain, an iiwa7_allegro fingertip, has 12 ops) — test_every_reachable_instantiation_is_in_gpu_links.  NT: outputs past 256 MiB.
    fan      drm_fk_fanout on the fingertips of allegro_left (4 chains, <8,5>) and trifinger_edu (3 chains, <4,4>): fk_fan_chain_kernel in
             the form without trigonometry on the last op (every chain of both hands ends in a fixed frame; the other form has no shipped
             robot); fk_fanout_kernel on a ragged tail and below 64 rows; fk_fan_chain2_kernel from DRM_FAN2_MIN_TILES (2 048) PAIRS of
             tiles on.
    all-links  drm_fk with every link as a target in walk order: fk_tree_fan_kernel (a hub and at most 80 KiB of LDS: both hands,
             iiwa7_allegro), fk_tree_groups_kernel (T > 8 otherwise: fetch, jaco, jaco_clean, panda), fk_tree_kernel (T <= 8: the arms,
             2link_robot) — ALL_LINKS_KERNEL, asserted against the walk; the same kernel for full tiles, tails, fewer than 64 rows and
             misaligned pointers.  NOT reached by any test: the streamed instantiations fk_tree_fan_kernel<true> and
             fk_tree_groups_kernel<true> (outputs past 256 MiB: 2^19 rows of a 28-link robot); the one launch of that size the suite
             has goes through drm_fk_links, and the issue rules out a second.
             compute_forward_kinematics_all_links itself launches drm_fk_links on a device (out of scope, see above).
    loop     fk_jacobian_tree_kernel / fk_tree_kernel: B < 64; a ragged tail; a [1:] view (pos is always 12 bytes off a 16-byte boundary,
             q and the Jacobians 4 n and 12 n), also as 65 * 64 + 1 rows; the walk with its shape bits cleared through the C ABI; and
    plan     plan_fk_and_jacobian(want_pose=False): pos = quat = NULL — al16(NULL) is 0 and launch_chain_fk_jacobian wants both, so
             NEITHER straight-line rung takes the launch: the loop kernel, its bits.  With a pose: the rung and the bits of the direct call.
             Eager and replayed from a captured graph.
    repeat   the first call of compute_fk_and_jacobian / compute_forward_kinematics goes through Python, later ones through the prepared
             entry (_fast_jac / _fast_fk): first, second and third call bit-equal, again after own_kernels is set to None and back.
RUNGS that need size (the 256 rows tiled cyclically; every row against its truth row, subtraction and maxima in fp64 ON THE DEVICE):
2 049 * 64 + 3 rows of panda_no_gripper (plain arm form + tail); the smallest count of full tiles whose outputs pass 256 MiB, from
stream_past_llc's bound, + 3 rows: 1 369 603 rows of panda_no_gripper at 196 B (streamed arm form) and 462 851 rows of an iiwa7_allegro
fingertip at 580 B (chain_fk_kernel<12, 12, JAC, NT>); (2 * 2 048 + 1) * 64 + 5 rows on both hands (fk_fan_chain2_kernel + the odd tile +
a tail).  All-links FK past the Infinity Cache: test_all_links_fk_beyond_the_infinity_cache (tests/test_gpu_parity.py) now also
holds every link of its sampled rows to this module's pos and quat metrics.

RUNG IDENTITY (what proves a rung was reached): two launches of one kernel are bit-equal; rows of full tiles are bit-equal with and
without a tail behind them; the tail row of B = 65 and every row of a [1:] view carry the bits of the loop kernel; every repetition of
the 256 rows in a sized launch carries the bits of the first.  Must NOT agree over the 256 rows: arm against loop (lin_jac: packed
two-joint sincos and pose pairs against one joint at a time), chain against loop on lin_jac of a link behind at least three moving
joints (z x p_e - z x p_k against z x (p_e - p_k); with one or two joints axes and origins can be exact in float32 — 2link_robot,
iiwa_link_2 — and the two agree: reported), two samples per lane against one (fk_chain2_trig composes in another order).  Bit-identical
BY CONSTRUCTION and asserted so: the fan-out against the single-target chain kernels (one chain_walk; the fixed last op taken as J = F
is a joint at angle 0, whose cos = 1 and sin = 0 make J == F exactly), the plain and the streamed arm form against the
register-resident form on the same rows (the same operations, in lock step), the NT form of the chain kernel against the cached one,
compute_endeffector_jacobian against compute_fk_and_jacobian, the C ABI against the public call, and the pose of
compute_fk_and_jacobian against compute_forward_kinematics on the chain and loop rungs (one kernel template with and without the
Jacobian; every kernel here owns 64 rows per wavefront).  On the arm rung that last pair is reported only: see FOUND.

EXACT, on the host build and on every GPU rung: q is unchanged by the call; outputs pre-filled with NaN have no NaN in their B rows and
the row behind them keeps its sentinel in each of the four arrays — at 128, 65, 131 and 63 rows and behind every sized launch (the tail of
a fast rung starts at an offset pointer); a row with one |q| = 4.0e5 meets the requirement like any other; two all-NaN q rows, in full
tiles (128 rows: rows 5 and 70) and in a ragged tail (127 rows: rows 70 and 100), come back non-finite in every entry that depends on q
(an entry that does not — Q-independent from the truth: off columns, the first joint's axis, a link fixed to the base — is non-finite or
carries the bits of the clean row) and change no bit of the other rows; the same two rows with |q| = 4.0e5 in every joint stay finite
and change no bit of the other rows — these conditions (sentinel, q unchanged, NaN rows, 4.0e5 rows, their neighbours) are run on the
single-link calls of every link of GPU_LINKS, through plans with and without a pose, on drm_fk with every link in walk order (each
of the three many-target kernels) and on drm_fk_fanout (full tiles, a 65-row launch, 63 rows, and the pair-tile launch with rows set
in one pair of tiles, in the odd tile and in the tail), on the host build as well; 1-D q, a column-slice q and both values of
`recursive` give the bits of the contiguous batched call.

FOUND by this module:
  * A row depended on the rows of its wavefront.  chain_trig_all (csrc/drm_chain_kernels.hip: chain_fk_kernel, fk_fan_chain_kernel) and
    chain_trig_lockstep (csrc/drm_arm_issue.hpp: the register-resident arm form) sent ALL 64 lanes through the fp64 argument
    reduction (sincos_f) as soon as one lane held a NaN, an Inf or an angle beyond 1e5 — against the rule drm_sample.hpp states for
    sincos_one and chain_trig ("a row never depends on the rows it shares a wavefront with").  Before: with rows 5 and 70 of 128 set to
    NaN the other 126 rows changed bits in all four outputs on every chain and arm link (e.g. allegro_left link_11.0_tip, fetch
    gripper_link, fetch_arm_no_gripper virtual_ee_link), within rounding.  FIXED: the escape is still entered by the whole wavefront
    (one scalar branch on the common path) but only the lanes that need it take sincos_f's values, the others keep the packed
    evaluation's, bit for bit.  After: no bit of another row changes, on every rung; occupancy of every kernel unchanged
    (register-resident arm form 140 -> 146 VGPRs at 3 waves per SIMD, chain kernels -1 .. +5 VGPRs); the benchmark's launch at parity
    (3.73 us against 3.72 us, medians of 12 alternating runs whose own spread is 3.70 .. 3.87 us).
  * chain_fk_kernel writes lin_jac as z_k x p_e - z_k x p_k (it parks z_k x p_k, three registers per op).  In a zero-lever column
    p_e == p_k bit for bit, so that is the difference of two evaluations of ONE cross product, which the compiler contracts
    differently: trifinger_edu finger_upper_link_0 comes back with 256 entries of up to 5.5e-17 instead of 0.0 (one per row; the arm rung,
    the loop kernels and the host build give 0.0).  Right to within rounding — each evaluation is within half an ulp of a sum of
    products |z_i p_j| <= max |p_e| — and left as it is: taking p_e - p_k first costs chain_fk_kernel<4,4>, <8,6> and <12,10> one
    wave per SIMD (73, 81, 98 VGPRs).  The exact condition is therefore: on the links of CHAIN_ZERO_LEVER_LINKS (that one link today; listed so
    that a change shows either way) a launch through the chain rung gives 0 < max |entry| <= 2^-23 max_b |pos64| of the link
    (CHAIN_ZERO_LEVER) in the zero-lever columns of lin; every other link on that rung, off columns, prismatic columns of ang, and
    every other rung: == 0.0.
    The same formula is why `lin` of the chain rung is the largest ratio of the module (MEASURED) — inside the requirement.
  * The pose of compute_fk_and_jacobian (register-resident arm form) and compute_forward_kinematics (plain FK-only arm form) differ by
    one ulp in 82 .. 117 of 1 792 entries on panda_no_gripper's panda_link7 (equal on the other arm links and robots, and equal between
    the three FK + Jacobian forms): two instantiations, contracted differently.  Both meet the requirement; reported, not asserted.

MEASURED (profiles/fk_rungs_tests.txt), worst err / yardstick over all seeds, links and batch sizes, per metric:
                                                          pos    quat   ang    lin    rowlin
    host build (API): every link, all links, fingertips   1.62   2.33   1.58   1.48   1.48     (quat: panda panda_leftfinger, seed 7)
    host emulation g++ / clang: emu_fk, emu_fk_jacobian    1.62   2.33   1.96   1.67   2.13     (plain, API, all-links, fanned walks)
      emu_fk_jacobian_arm                                 1.25   1.82   1.47   1.13   1.13
    MI355X, all rungs                                     1.62   1.95   1.51   3.32   2.93
      arm, register-resident form, +tail                  1.25   1.82   1.47   1.31   1.31
      arm, plain form + tail (131 139 rows)               1.09   1.09   1.24   0.87   0.87
      arm, streamed form + tail (1 369 603 rows)          1.09   1.09   1.24   0.87   0.87
      chain<4,4>, +tail                                   1.09   1.47   1.17   2.76   2.76
      chain<8,6>, +tail                                   1.06   1.53   1.48   2.11   2.05
      chain<8,8>, +tail                                   1.62   1.46   1.39   2.93   2.93
      chain<12,10>, +tail                                 1.30   1.32   1.51   3.32   2.73     (lin: fetch gripper_link)
      chain<12,12>, +tail; streamed (462 851 rows)        1.00   0.95   1.37   2.61   2.32
      fan, fan + tail, fan2 + odd tile + tail             1.09   1.95   -      -      -        (262 213 rows)
      fk_tree_fan / fk_tree_groups / fk_tree_kernel       1.62   1.95   -      -      -
      loop (B < 64, tails, shape bits cleared, [1:] view) 1.62   1.82   1.51   1.48   1.48
      plans with a pose / without (loop kernel)           1.30   1.21   1.47   2.61   2.32
      |q| = 4.0e5 rows (every rung)                       1.62   1.95   1.51   3.32   2.93
      all-links FK past the Infinity Cache (test_gpu_parity) 1.33 1.41  -      -      -
    Wall time of the module: 37 s without a GPU (212 tests), 8.6 s on the MI355X (144 tests; slowest case 1.1 s).
MUTATIONS on a scratch copy of the host emulation (figures in profiles/fk_rungs_tests.txt; seed 61):
  * the fixed offset of allegro_left's last finger link to its tip (link_15.0_tip, 0.0423 m) + 1e-6 m: TOL_POS and TOL_JAC pass (1.0e-06 m,
    1.0e-06); CAUGHT: pos 6.2e-06 against 1.27e-07 (49x), lin 2.4e-05 against 2.1e-07 (113x), rowlin 125x;
  * the lever of column 21 of iiwa7_allegro's link_15.0_tip taken to the origin of joint 22: CAUGHT, lin 0.55 against 1.1e-06 — at
    5.1e-02 it is beyond TOL_JAC as well, so this one the old tolerance did not let through;
  * the z offset (0.105 m) of the folded fixed tail of panda_no_gripper's arm chain + 1e-6 (emu_fk_jacobian_arm): TOL_POS and TOL_JAC pass
    (1.05e-06 m, 1.1e-06); pos 8.9e-07 against 1.19e-07 is 7.5x, inside the margin, but CAUGHT by lin and rowlin: 7.5e-06 against
    5.5e-07, 13.6x (the levers of the wrist joints are 0.09 .. 0.11 m).
NO HOST EMULATION: chain_fk_kernel, fk_fan_chain_kernel (chain_trig_all and chain_walk live in csrc/drm_chain_kernels.hip, not in a header
that compiles for the host), fk_fan_chain2_kernel (its chain, fk_chain2_trig, is in drm_sample.hpp, but the host form of pin2 inside it does not compile under
the ROCm clang — "couldn't allocate output register for constraint 'x'" — and the emulation is built with both compilers), fk_fanout_kernel, fk_tree_fan_kernel and fk_tree_groups_kernel (fk_loop emulates their walk, not their staging), the three forms of
fk_jacobian_arm_kernel beyond their shared arithmetic.  The GPU tests hold every row of their launches.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from differentiable_robot_model_amd.flatten import SHAPE_ARM_CHAIN, SHAPE_FK_FAN, SHAPE_SERIAL_CHAIN, build_walk
from helpers import ALL_ROBOTS, load_model, quat_branch_margin, sample_states
from oracle import Oracle
from test_fd_crba_rungs import ARM_ROBOTS, BIG_ANGLE, FLOOR, MARGIN, ROWS, SEEDS, dev, gpu_model, library_and_stream, model_on
from test_host_emu import _ptr, emu, host_walk  # noqa: F401  (emu is a fixture)
from test_rnea_rungs import quat_error

OFF, ZERO_LEVER, PRISMATIC, REVOLUTE = 0, 1, 2, 3
# chain_fk_kernel alone writes lin_jac as z_k x p_e - z_k x p_k: in a zero-lever column (p_e == p_k bit for bit) that is the difference of
# two evaluations of ONE cross product, which the compiler is free to contract differently; each is within half an ulp of a sum of
# products |z_i p_j| <= max |p_e|, so the entry is 0.0 or at most one ulp of the link's reach.  Every other path: exactly 0.0.
CHAIN_ZERO_LEVER = 2.0 ** -23
# ... and the links on which it is not 0.0 today, listed so that a change shows: on every other link of GPU_LINKS the chain rung, too, is
# held to exactly 0.0, and on these a launch through the chain rung that DOES come back all zero fails as well
CHAIN_ZERO_LEVER_LINKS = {("trifinger_edu", "finger_upper_link_0")}
ROWLIN_THRESHOLD = 1e-3                 # a (row, column) pair enters `rowlin` when its lever exceeds this share of the column's largest
ROWLIN_CAP = 0.01                       # ... and no robot may lose more than this share of its pairs to the threshold
PRE_MAX_TILES = 2048                    # DRM_PRE_MAX_TILES (csrc/drm_arm_kernels.hip)
FAN2_MIN_TILES = 2048                   # DRM_FAN2_MIN_TILES (csrc/drm_chain_kernels.hip), pairs of tiles
MISALIGNED_TILES = 64                   # csrc/drm_common.hpp
LLC_BYTES = 256 * 1024 * 1024           # stream_past_llc (csrc/drm_common.hpp): outputs of MORE bytes are streamed past the Infinity Cache
# the two models whose joints slide (reference_compat=False, built as tests/test_joint_models.py builds them): robot key -> the link
SLIDING = {"fetch:sliding": "r_gripper_finger_link", "panda:sliding": "panda_rightfinger"}
FINGERTIPS = {"allegro_left": ("link_11.0_tip", "link_7.0_tip", "link_3.0_tip", "link_15.0_tip"),
              "trifinger_edu": ("finger_tip_link_0", "finger_tip_link_120", "finger_tip_link_240")}
# columns by class, summed over the non-root links of a robot: (off, zero-lever).  From the truth and the spec alone; asserted
# against the truth of both seeds, so that a change of the classification shows up here.
COLUMN_COUNTS = {"2link_robot": (1, 2), "allegro_left": (264, 16), "allegro_left_small_damping": (264, 16), "fetch": (251, 15),
                 "fetch_arm_no_gripper": (21, 7), "fetch_arm_no_gripper_small_damping": (21, 7), "iiwa7": (21, 7), "iiwa7_allegro": (413, 23),
                 "jaco": (96, 12), "jaco_clean": (102, 12), "panda": (43, 11), "panda_no_gripper": (21, 9), "trifinger_edu": (117, 9),
                 "fetch:sliding": (251, 11), "panda:sliding": (43, 9)}
# (row, revolute column) pairs below ROWLIN_THRESHOLD, summed over the non-root links: (seed 61, seed 7) of the pairs in all
ROWLIN_SKIPPED = {"2link_robot": (0, 0, 768), "allegro_left": (0, 0, 10240), "allegro_left_small_damping": (0, 0, 10240), "fetch": (0, 0, 17920),
                  "fetch_arm_no_gripper": (0, 0, 7168), "fetch_arm_no_gripper_small_damping": (0, 0, 7168), "iiwa7": (0, 0, 7168),
                  "iiwa7_allegro": (0, 0, 53248), "jaco": (0, 0, 15360), "jaco_clean": (0, 0, 16896), "panda": (0, 0, 13824),
                  "panda_no_gripper": (0, 0, 6656), "trifinger_edu": (0, 0, 4608), "fetch:sliding": (0, 0, 13568), "panda:sliding": (0, 0, 13824)}


# ------------------------------------------------------------------------------------------------------------------- truth
@functools.lru_cache(maxsize=None)
def sliding_model(robot, device):
    m = load_model(robot, device, reference_compat=False)
    if device != "cpu":
        m.own_kernels = "off"
    return m


def model_for(key, device="cpu"):
    robot, _, sliding = key.partition(":")
    if sliding:
        return sliding_model(robot, device)
    return model_on(robot) if device == "cpu" else gpu_model(robot)


def with_root(pos, quat):
    """[B, L-1, .] of the non-root links -> [B, L, .] with the root's identity pose in front"""
    B = pos.shape[0]
    root = np.zeros((B, 1, 4), quat.dtype)
    root[..., 3] = 1
    return np.concatenate([np.zeros((B, 1, 3), pos.dtype), pos], 1), np.concatenate([root, quat], 1)


def quat_err_rows(a, b, near):
    """quat_error of tests/test_rnea_rungs.py on torch tensors (any device): a [N, ..., 4] against b, the sign free where `near`"""
    sgn = torch.sign((a * b).sum(-1, keepdim=True))
    sgn = torch.where(sgn == 0, torch.ones_like(sgn), sgn)
    return (a * torch.where(near[..., None], sgn, torch.ones_like(sgn)) - b).abs()


@functools.lru_cache(maxsize=None)
def truth(key, seed):
    """the fp64 oracle's all-links FK of 256 rows (seed 61, 7, or "4e5": seed 61 with one joint of rows 2 and 77 at +-4.0e5 — the float32
    value is what the truth sees), checked; the Jacobian truths of single links are added by jac_truth"""
    m = model_for(key)
    n, L = m._n_dofs, len(m._bodies)
    q = sample_states(m, ROWS, seed=61 if seed == "4e5" else seed)[0]
    if seed == "4e5":
        q = q.copy()
        q[2, min(5, n - 1)] = BIG_ANGLE
        q[77, 0] = -BIG_ANGLE
    orc, links = Oracle(m._spec), list(range(1, L))
    P64, Q64 = with_root(*orc.fk(q.astype(np.float64), links, np.float64))
    P32, Q32 = with_root(*orc.fk(q, links, np.float32))
    assert P64.dtype == np.float64 and P32.dtype == np.float32
    assert np.abs(np.linalg.norm(Q64, axis=-1) - 1).max() <= 1e-12, "the truth's quaternions are unit"
    t = dict(key=key, seed=61 if seed == "4e5" else seed, q=q, P64=P64, Q64=Q64, reach=np.abs(P64).max(axis=(0, 2)),
             near=quat_branch_margin(Q64) <= 1e-5, names=[b.name for b in m._bodies], orc=orc, spec=m._spec, jac={}, dev={})
    yp, yq = pose_errors(t, torch.from_numpy(P32), torch.from_numpy(Q32), list(range(L)))
    assert all(yp[i] == 0 for i in range(L) if t["reach"][i] == 0), "a link at the origin is there in float32 too"
    # (the torch restatement of quat_error is that function)
    assert abs(max(yq) - quat_error(Q32, Q64)) <= 1e-15
    t.update(yard_pos=yp, yard_quat=yq)
    return t


def on_device(t, device, name, make):
    """a truth array as a float64 / bool / int64 tensor on `device`, uploaded once"""
    k = (str(device), name)
    if k not in t["dev"]:
        t["dev"][k] = torch.from_numpy(np.ascontiguousarray(make())).to(device)
    return t["dev"][k]


def rows_of(N, idx, device):
    idx = np.arange(N) % ROWS if idx is None else np.asarray(idx)
    assert len(idx) == N
    return torch.from_numpy(idx.astype(np.int64)).to(device)


def pose_errors(t, P, Q, links, idx=None):
    """(pos, quat) per link of `links` of the poses P [N, T, 3], Q [N, T, 4] against the truth rows idx; on the device of P, in fp64.
    pos: max_b |dpos| / max_b |pos64| of that link, exactly 0 required (inf otherwise) where the link never leaves the origin"""
    assert P.shape[1:] == (len(links), 3) and Q.shape[1:] == (len(links), 4) and P.shape[0] == Q.shape[0], (P.shape, Q.shape)
    d = P.device
    P64 = on_device(t, d, "P64", lambda: t["P64"])
    Q64 = on_device(t, d, "Q64", lambda: t["Q64"])
    near = on_device(t, d, "near", lambda: t["near"])
    k, cols = rows_of(P.shape[0], idx, d), torch.tensor(links, device=d)
    dp = torch.zeros(len(links), dtype=torch.float64, device=d)
    dq = torch.zeros(len(links), dtype=torch.float64, device=d)
    for lo in range(0, len(k), 32768):
        kk = k[lo:lo + 32768]
        dp = torch.maximum(dp, (P[lo:lo + 32768].double() - P64[kk][:, cols]).abs().amax(dim=(0, 2)))
        dq = torch.maximum(dq, quat_err_rows(Q[lo:lo + 32768].double(), Q64[kk][:, cols], near[kk][:, cols]).amax(dim=(0, 2)))
        bad = ~(torch.isfinite(P[lo:lo + 32768]).all() & torch.isfinite(Q[lo:lo + 32768]).all())
        if bool(bad):
            dp += float("nan")
    dp, dq, reach = dp.cpu().numpy(), dq.cpu().numpy(), t["reach"][links]
    pos = [float(e / r) if r > 0 else (0.0 if e == 0 else float("inf")) for e, r in zip(dp, reach)]
    return pos, [float(x) for x in dq]


def jac_truth(t, link):
    """The fp64 Jacobian of one link with its own checks: every DoF column classified from the truth and the spec (never from an output
    under test), the lever identity, the yardstick (the float32 oracle on the same rows)."""
    if link in t["jac"]:
        return t["jac"][link]
    spec, orc, q, P64 = t["spec"], t["orc"], t["q"], t["P64"]
    n = q.shape[1]
    pos64, quat64, lin64, ang64 = orc.fk_jacobian(q.astype(np.float64), link, np.float64)
    assert lin64.dtype == np.float64 and np.abs(pos64 - P64[:, link]).max() <= 1e-12 and np.abs(quat64 - t["Q64"][:, link]).max() <= 1e-12
    chain = [int(c) for c in spec.chain_to(link)]
    link_of = {int(spec.dof[c]): c for c in chain if spec.dof[c] >= 0}
    cls, lever_b = np.full(n, OFF), np.zeros((ROWS, n))
    for k, c in link_of.items():
        d = pos64 - P64[:, c]                                    # p_e - p_k: the origin of the link that DoF k moves
        lever_b[:, k] = np.linalg.norm(d, axis=1)
        a, l = ang64[:, :, k], lin64[:, :, k]
        if not a.any() and np.abs(np.linalg.norm(l, axis=1) - 1).max() <= 1e-12:
            cls[k] = PRISMATIC
            continue
        cls[k] = REVOLUTE if lever_b[:, k].max() > 0 else ZERO_LEVER
        assert np.abs(np.linalg.norm(a, axis=1) - 1).max() <= 1e-12, "a revolute column of ang64 is a unit axis"
        assert np.abs(l - np.cross(a, d)).max() <= 1e-12 * lever_b[:, k].max(), "lin64 = z_k x (p_e - p_k)"
    kind = getattr(spec, "kind", None)
    if ":" in t["key"]:
        assert kind is not None and all((int(kind[c]) == 2) == (cls[k] == PRISMATIC) for k, c in link_of.items()), "the spec's sliding joints"
    off = cls == OFF
    assert not ang64[:, :, off].any() and not lin64[:, :, off].any(), "columns of DoFs off the chain are identically zero"
    assert not lin64[:, :, cls == ZERO_LEVER].any()
    lever = lever_b.max(axis=0)
    rowmask = (cls == REVOLUTE)[None, :] & (lever_b > ROWLIN_THRESHOLD * lever[None, :])
    J = dict(link=link, name=t["names"][link], lin64=lin64, ang64=ang64, cls=cls, lever=lever, lever_b=lever_b, rowmask=rowmask,
             skipped=int(((cls == REVOLUTE)[None, :] & ~rowmask).sum()), pairs=int((cls == REVOLUTE).sum()) * ROWS, dev={})
    t["jac"][link] = J
    pos32, quat32, lin32, ang32 = orc.fk_jacobian(q, link, np.float32)
    assert lin32.dtype == np.float32
    J["yard"] = jac_errors(t, J, tuple(torch.from_numpy(x) for x in (pos32, quat32, lin32, ang32)))[0]
    return J


def jac_errors(t, J, outs, idx=None):
    """({metric: error}, number of entries of off columns and of prismatic columns of ang that are not 0.0, largest |entry| of the zero-lever
    columns of lin) of (pos, quat, lin, ang) — pos and quat may be None —
    against the truth rows idx; computed on the device of the outputs, in fp64, in chunks"""
    pos, quat, lin, ang = outs
    d, link, cls = lin.device, J["link"], J["cls"]
    N, n = lin.shape[0], len(cls)
    assert lin.shape == (N, 3, n) and ang.shape == (N, 3, n)
    up = lambda name: on_device(J, d, name, lambda: J[name])
    lin64, ang64, lever_b, rowmask = up("lin64"), up("ang64"), up("lever_b"), up("rowmask")
    k = rows_of(N, idx, d)
    zero_lin, own = torch.from_numpy(cls == OFF).to(d), torch.from_numpy(cls == ZERO_LEVER).to(d)
    zero_ang = torch.from_numpy((cls == OFF) | (cls == PRISMATIC)).to(d)
    lin_col = torch.zeros(n, dtype=torch.float64, device=d)
    ang_col = torch.zeros(n, dtype=torch.float64, device=d)
    rowlin = torch.zeros((), dtype=torch.float64, device=d)
    exact = torch.zeros((), dtype=torch.int64, device=d)
    zero_lever = torch.zeros((), dtype=torch.float64, device=d)
    finite = torch.ones((), dtype=torch.bool, device=d)
    for lo in range(0, N, 32768):
        kk, l, a = k[lo:lo + 32768], lin[lo:lo + 32768], ang[lo:lo + 32768]
        dl, da = (l.double() - lin64[kk]).abs().amax(dim=1), (a.double() - ang64[kk]).abs().amax(dim=1)      # [rows, n]: the worst of x, y, z
        lin_col, ang_col = torch.maximum(lin_col, dl.amax(dim=0)), torch.maximum(ang_col, da.amax(dim=0))
        m = rowmask[kk]
        if bool(m.any()):
            rowlin = torch.maximum(rowlin, (dl[m] / lever_b[kk][m]).max())
        exact += (l[:, :, zero_lin] != 0).sum() + (a[:, :, zero_ang] != 0).sum()
        if bool(own.any()):
            zero_lever = torch.maximum(zero_lever, l[:, :, own].double().abs().max())
        finite &= torch.isfinite(l).all() & torch.isfinite(a).all()
    lin_col, ang_col = lin_col.cpu().numpy(), ang_col.cpu().numpy()
    e = {}
    if pos is not None:
        p, r = pose_errors(t, pos[:, None], quat[:, None], [link], idx)
        e.update(pos=p[0], quat=r[0])
    turning = (cls == REVOLUTE) | (cls == ZERO_LEVER)
    if turning.any():
        e["ang"] = float(ang_col[turning].max())
    rev, pris = cls == REVOLUTE, cls == PRISMATIC
    if rev.any() or pris.any():
        e["lin"] = float(max(list(lin_col[rev] / J["lever"][rev]) + list(lin_col[pris])))
    if rev.any():
        e["rowlin"] = float(rowlin)
    if not bool(finite):
        e = {m: float("nan") for m in e}
    return e, int(exact), float(zero_lever)


# ------------------------------------------------------------------------------------------------------------------- checks
def line(key, link, path, seed, metric, e, ey):
    print("FKRUNG %-28s %-32s %-34s %2d %-6s %.3e %.3e %.2f" % (key, link, path, seed, metric, e, ey, e / ey))


def as_tensor(x):
    return None if x is None else (x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x)))


def check_jac(path, t, link, outs, idx=None, chain_rung=False):
    """(pos, quat, lin, ang) of one link against the requirement: every metric printed, then asserted; the exact zeros.  `chain_rung`: full
    tiles went through chain_fk_kernel, whose zero-lever columns on the links of CHAIN_ZERO_LEVER_LINKS are non-zero and held to
    CHAIN_ZERO_LEVER of the link's reach (FOUND); everywhere else they are 0.0"""
    J = jac_truth(t, link)
    outs = tuple(as_tensor(x) for x in outs)
    assert all(x is None or x.dtype == torch.float32 for x in outs)
    e, exact, zero_lever = jac_errors(t, J, outs, idx)
    failures = []
    for metric, err in e.items():
        ey = max(J["yard"][metric], FLOOR)
        line(t["key"], J["name"], path, t["seed"], metric, err, ey)
        if not err <= MARGIN * ey:
            failures.append((metric, err, ey))
    assert not failures, (t["key"], J["name"], path, failures)
    assert exact == 0, (t["key"], J["name"], path, "%d entries of off / prismatic columns are not 0.0" % exact)
    noisy = chain_rung and (t["key"], J["name"]) in CHAIN_ZERO_LEVER_LINKS
    if zero_lever or noisy:
        print("FKRUNG-ZERO-LEVER %-28s %-32s %-34s largest |entry| %.3e, reach %.3e" % (t["key"], J["name"], path, zero_lever, t["reach"][link]))
    if noisy:
        assert 0.0 < zero_lever <= CHAIN_ZERO_LEVER * t["reach"][link], (t["key"], J["name"], path, zero_lever)
    else:
        assert zero_lever == 0.0, (t["key"], J["name"], path, zero_lever)


def check_poses(path, t, links, P, Q, idx=None):
    """the poses P [N, T, 3], Q [N, T, 4] of `links` against the requirement, link by link"""
    P, Q = as_tensor(P), as_tensor(Q)
    assert P.dtype == torch.float32 and Q.dtype == torch.float32
    pos, quat = pose_errors(t, P, Q, list(links), idx)
    failures = []
    for j, link in enumerate(links):
        for metric, err, yard in (("pos", pos[j], t["yard_pos"][link]), ("quat", quat[j], t["yard_quat"][link])):
            ey = max(yard, FLOOR)
            line(t["key"], t["names"][link], path, t["seed"], metric, err, ey)
            if not err <= MARGIN * ey:
                failures.append((t["names"][link], metric, err, ey))
    assert not failures, (t["key"], path, failures)


def same_bits(a, b, expect, what):
    """Two rungs with different arithmetic must differ somewhere, two launches of one kernel must not (None: reported only)."""
    a, b = (torch.cat([x.reshape(x.shape[0], -1) for x in v], 1) if isinstance(v, (tuple, list)) else v for v in (a, b))
    equal = bool(torch.equal(a, b)) if isinstance(a, torch.Tensor) else bool(np.array_equal(a, b))
    note = ""
    if not equal and isinstance(a, torch.Tensor) and a.shape == b.shape:
        note = "  (%d of %d entries, largest %.3e)" % (int((a != b).sum()), a.numel(), float((a.double() - b.double()).abs().max()))
    print("FKRUNG-BITS %-90s %s%s" % (what, "equal" if equal else "differ", note))
    assert expect is None or equal == expect, what


def link_index(m, name):
    return m._name_to_idx_map[name]


def non_root(m):
    return list(range(1, len(m._bodies)))


# ------------------------------------------------------------------------------------------------------------------- the truth itself
@pytest.mark.parametrize("key", ALL_ROBOTS + sorted(SLIDING))
def test_truth_column_classes_and_lever_threshold(key):
    """Before anything under test: the lever identity, unit quaternions and the column classes of every non-root link (jac_truth asserts
    them), the literal counts of off and zero-lever columns, and the share of (row, column) pairs `rowlin` leaves out."""
    m = model_for(key)
    counts, skipped, pairs = None, [], 0
    for seed in SEEDS:
        t = truth(key, seed)
        Js = [jac_truth(t, link) for link in non_root(m)]
        c = (sum(int((J["cls"] == OFF).sum()) for J in Js), sum(int((J["cls"] == ZERO_LEVER).sum()) for J in Js))
        assert counts in (None, c), "the classes do not depend on the rows"
        counts, pairs = c, sum(J["pairs"] for J in Js)
        skipped.append(sum(J["skipped"] for J in Js))
        smallest = min([J["lever"][J["cls"] == REVOLUTE].min() for J in Js if (J["cls"] == REVOLUTE).any()])
        print("FKRUNG-TRUTH %-34s seed %2d off %3d zero-lever %2d prismatic %d smallest lever %.4f m, rowlin skips %d of %d pairs (%.3f %%)" % (
            key, seed, c[0], c[1], sum(int((J["cls"] == PRISMATIC).sum()) for J in Js), smallest, skipped[-1], pairs, 100.0 * skipped[-1] / pairs))
        assert skipped[-1] <= ROWLIN_CAP * pairs
        if ":" in key:
            J = jac_truth(t, link_index(m, SLIDING[key]))
            assert (J["cls"] == PRISMATIC).sum() == (2 if key.startswith("fetch") else 1), "the chain passes the sliding joints"
    assert (counts, tuple(skipped), pairs) == (COLUMN_COUNTS[key], ROWLIN_SKIPPED[key][:2], ROWLIN_SKIPPED[key][2]), (key, counts, skipped, pairs)


# ------------------------------------------------------------------------------------------------------------------- runners
# The links of the GPU tests, with the kernel instantiation the full aligned tiles of each take (asserted against the walk the API
# launches, instantiation_of): every (CAP, USED) a shipped link reaches, the arm kernel, one interior link.  No shipped link has a walk
# that is not a serial chain of at most 16 ops (the longest, an iiwa7_allegro fingertip, has 12), so none stands for "no fast path".
GPU_LINKS = {
    "2link_robot": (("endEffector", "chain<4,4>"), ("arm1", "chain<4,4>")),
    "allegro_left": (("link_11.0_tip", "chain<8,6>"), ("link_15.0", "chain<4,4>"), ("link_9.0", "chain<4,4>")),
    "allegro_left_small_damping": (("link_3.0_tip", "chain<8,6>"), ("link_6.0", "chain<4,4>")),
    "fetch": (("gripper_link", "chain<12,10>"), ("wrist_roll_link", "chain<8,8>"), ("forearm_roll_link", "chain<8,6>"),
              ("head_camera_rgb_optical_frame", "chain<4,4>"), ("shoulder_lift_link", "chain<4,4>")),
    "fetch_arm_no_gripper": (("virtual_ee_link", "arm"), ("wrist_roll_link", "chain<8,8>"), ("forearm_roll_link", "chain<8,6>"), ("elbow_flex_link", "chain<4,4>")),
    "fetch_arm_no_gripper_small_damping": (("virtual_ee_link", "arm"), ("upperarm_roll_link", "chain<4,4>")),
    "iiwa7": (("iiwa_link_ee", "arm"), ("iiwa_link_7", "arm"), ("iiwa_link_5", "chain<8,6>"), ("iiwa_link_2", "chain<4,4>")),
    "iiwa7_allegro": (("link_15.0_tip", "chain<12,12>"), ("link_13.0", "chain<12,10>"), ("palm_link", "chain<8,8>"), ("iiwa_link_6", "chain<8,6>"),
                      ("iiwa_link_3", "chain<4,4>")),
    "jaco": (("j2n6s300_link_finger_tip_3", "chain<8,8>"), ("j2n6s300_end_effector", "chain<8,8>"), ("j2n6s300_link_5", "chain<8,6>"),
             ("j2n6s300_link_3", "chain<4,4>")),
    "jaco_clean": (("j2n6s300_link_ee", "chain<8,8>"), ("j2n6s300_link_finger_tip_1", "chain<8,8>"), ("j2n6s300_link_2", "chain<4,4>")),
    "panda": (("panda_rightfinger", "chain<8,8>"), ("panda_hand", "chain<8,8>"), ("panda_link6", "chain<8,6>"), ("panda_link3", "chain<4,4>")),
    "panda_no_gripper": (("panda_virtual_ee_link", "arm"), ("panda_link7", "arm"), ("panda_link5", "chain<8,6>"), ("panda_link4", "chain<4,4>")),
    "trifinger_edu": (("finger_tip_link_240", "chain<4,4>"), ("finger_middle_link_120", "chain<4,4>"), ("finger_upper_link_0", "chain<4,4>")),
    "fetch:sliding": (("r_gripper_finger_link", "chain<12,10>"),),
    "panda:sliding": (("panda_rightfinger", "chain<8,8>"),),
}


def chain_struct(model, name, clear_shape=0):
    """A private copy of the struct of the walk the kinematics calls launch for this link (robot_model._chain_walk: fixed links folded),
    shape bits switched off on request"""
    from differentiable_robot_model_amd import backend
    dw = model._chain_walk(link_index(model, name))
    walk = backend._walk_struct_build(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs)
    if clear_shape:
        walk.shape = walk.shape & ~clear_shape
    return walk


def instantiation_of(walk):
    """the kernel the full aligned tiles of a launch of this walk take (csrc/drm_fk_jacobian.hip drm_fk_jacobian, csrc/drm_fk.hip drm_fk,
    csrc/drm_chain_kernels.hip launch_chain)"""
    if walk.shape & SHAPE_ARM_CHAIN and walk.capacity == 8 and walk.n_dofs == 7 and walk.target_perm == 2:
        return "arm"
    if walk.shape & SHAPE_SERIAL_CHAIN and walk.capacity in (4, 8, 12, 16) and walk.n_ops >= 1 and walk.n_slots == 0 and walk.n_dofs <= 32:
        cap = walk.capacity
        return "chain<%d,%d>" % (cap, cap - 2 if cap > 4 and walk.n_ops <= cap - 2 else cap)
    return "loop"


def path_name(inst, B):
    if B < 64:
        return "loop-B%d" % B
    return "%s%s-B%d" % (inst, "+tail" if B % 64 else "", B)


def sliced(call, q, B):
    """a call over the 256 rows in consecutive launches of B rows, each on a 16-byte aligned copy of its slice"""
    outs = [call(q[i:i + B].clone()) for i in range(0, q.shape[0], B)]
    return tuple(torch.cat([o[k] for o in outs]) for k in range(len(outs[0])))


def api_link(model, path, t, name, B=None, fk_bits=True, chain_rung=False):
    """compute_fk_and_jacobian of one link over the 256 rows against the requirement; compute_endeffector_jacobian gives its bits;
    compute_forward_kinematics meets the requirement and (fk_bits; None: reported) gives the bits of its pose.  q stays as it was."""
    link, B = link_index(model, name), B or ROWS
    q = dev(t["q"], model._device)
    keep = q.clone()
    outs = sliced(lambda x: model.compute_fk_and_jacobian(x, name), q, B)
    assert all(o.dtype == torch.float32 and o.grad_fn is None for o in outs)
    check_jac(path, t, link, outs, chain_rung=chain_rung)
    same_bits(sliced(lambda x: model.compute_endeffector_jacobian(x, name), q, B), outs[2:], True,
              "%s %s %s compute_endeffector_jacobian vs compute_fk_and_jacobian" % (t["key"], name, path))
    fk = sliced(lambda x: model.compute_forward_kinematics(x, name), q, B)
    check_poses("fk:" + path, t, [link], fk[0][:, None], fk[1][:, None])
    same_bits(fk, outs[:2], fk_bits, "%s %s %s compute_forward_kinematics vs the pose of compute_fk_and_jacobian" % (t["key"], name, path))
    assert torch.equal(keep, q), "the caller's q is not modified"
    return outs


def all_links_order(model):
    return [i for i in model._spec.preorder() if i != 0]


def api_all_links(model, path, t, B=None):
    """compute_forward_kinematics_all_links (root included), _fk_targets over every link in walk order (drm_fk with ordered targets) and,
    for the two hands, _fk_targets over the fingertips (drm_fk_fanout)"""
    B = B or ROWS
    q = dev(t["q"], model._device)
    keep = q.clone()
    names = t["names"]
    poses = [model.compute_forward_kinematics_all_links(q[i:i + B].clone()) for i in range(0, ROWS, B)]
    assert all(list(p) == names for p in poses)
    P = torch.stack([torch.cat([p[nm][0] for p in poses]) for nm in names], 1)
    Q = torch.stack([torch.cat([p[nm][1] for p in poses]) for nm in names], 1)
    check_poses("all-links:" + path, t, list(range(len(names))), P, Q)
    order = all_links_order(model)
    P2, Q2 = sliced(lambda x: model._fk_targets(x, order), q, B)
    check_poses("ordered-targets:" + path, t, order, P2, Q2)
    key = t["key"].split(":")[0]
    if key in FINGERTIPS:
        tips = [link_index(model, nm) for nm in FINGERTIPS[key]]
        check_poses("fingertips:" + path, t, tips, *sliced(lambda x: model._fk_targets(x, tips), q, B))
    assert torch.equal(keep, q)
    return P2, Q2


def abi_jac(walk, q, outs=None, pose=True):
    """drm_fk_jacobian on the tensors as they are (views included); (pos, quat, lin, ang) pre-filled with NaN unless given"""
    from differentiable_robot_model_amd import backend
    lib, stream = library_and_stream(q.device)
    B, n = q.shape
    if outs is None:
        outs = tuple(torch.full((B,) + s, float("nan"), device=q.device) for s in ((3,), (4,), (3, n), (3, n)))
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    backend._check(lib.drm_fk_jacobian(ctypes.byref(walk), ptr(q), ctypes.c_int64(B), ptr(outs[0]) if pose else None, ptr(outs[1]) if pose else None,
                                       ptr(outs[2]), ptr(outs[3]), stream), lib)
    return outs


def abi_fk(walk, q, T=1, outs=None):
    """drm_fk: pos [B, T, 3], quat [B, T, 4]"""
    from differentiable_robot_model_amd import backend
    lib, stream = library_and_stream(q.device)
    B = q.shape[0]
    if outs is None:
        outs = tuple(torch.full((B, T, k), float("nan"), device=q.device) for k in (3, 4))
    backend._check(lib.drm_fk(ctypes.byref(walk), ctypes.c_void_p(q.data_ptr()), ctypes.c_int64(B), T, ctypes.c_void_p(outs[0].data_ptr()),
                              ctypes.c_void_p(outs[1].data_ptr()), stream), lib)
    return outs


# ------------------------------------------------------------------------------------------------------------------- edges (any device)
def sentinel_check(model, t, name, B):
    """through the C ABI: the four outputs pre-filled with NaN in allocations one row longer than the launch — no NaN in the B rows, the
    row behind them keeps its sentinel, q is unchanged, and the rows are the public call's"""
    device, n = model._device, model._n_dofs
    walk = chain_struct(model, name)
    q = dev(t["q"][:B], device)
    keep = q.clone()
    bufs = [torch.full((B + 1,) + s, float("nan"), device=device) for s in ((3,), (4,), (3, n), (3, n))]
    for b in bufs:
        b[B] = -7.25
    abi_jac(walk, q, tuple(b[:B] for b in bufs))
    for b in bufs:
        assert not torch.isnan(b[:B]).any() and (b[B] == -7.25).all(), (t["key"], name, B)
    assert torch.equal(keep, q)
    same_bits(tuple(b[:B] for b in bufs), model.compute_fk_and_jacobian(q, name), True, "%s %s B=%d C ABI vs compute_fk_and_jacobian" % (t["key"], name, B))
    pose = [torch.full((B + 1, 1, k), float("nan"), device=device) for k in (3, 4)]
    for b in pose:
        b[B] = -7.25
    abi_fk(walk, q, 1, tuple(b[:B] for b in pose))
    for b in pose:
        assert not torch.isnan(b[:B]).any() and (b[B] == -7.25).all(), (t["key"], name, B)
    same_bits(tuple(b[:B, 0] for b in pose), model.compute_forward_kinematics(q, name), True, "%s %s B=%d C ABI vs compute_forward_kinematics" % (t["key"], name, B))


@functools.lru_cache(maxsize=None)
def q_independent(key, name):
    """the entries of (pos, quat, lin, ang) of a link that do not see q at all, from the truth: those that are one value over all rows of
    both seeds (off columns, the first joint's axis, a link fixed to the base)"""
    m = model_for(key)
    link = link_index(m, name)
    both = [truth(key, seed) for seed in SEEDS]
    Js = [jac_truth(t, link) for t in both]
    arrays = [np.concatenate([t["P64"][:, link] for t in both]), np.concatenate([t["Q64"][:, link] for t in both]),
              np.concatenate([J["lin64"] for J in Js]), np.concatenate([J["ang64"] for J in Js])]
    return tuple(np.ptp(a, axis=0) <= 1e-12 for a in arrays)


FULL_AND_RAGGED = ((128, (5, 70)), (127, (70, 100)))


def same_words(a, b):
    """bit equality that also holds for NaN"""
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def neighbour_rows_check(what, t, run, free, device, sizes=FULL_AND_RAGGED):
    """run(q) -> tensors [B, ...].  Rows of q set to NaN in every joint — sizes: (rows of the launch, the rows set), by default in full
    tiles (128 rows: rows 5 and 70) and in a ragged tail (127 rows: rows 70 and 100) — come back non-finite in every entry that depends
    on q (`free`, per output: the entries that do not, from the truth — there: non-finite or the bits of the clean row) and change no
    bit of the other rows.  The same with |q| = 4.0e5 in every joint of those rows (the fp64 argument reduction, entered by the whole
    wavefront): finite, and no bit of another row changes.  q is unchanged by every call."""
    free = [torch.from_numpy(np.ascontiguousarray(f)).to(device) for f in free]
    for value in (float("nan"), BIG_ANGLE):
        for B, rows in sizes:
            q = on_device(t, device, "q", lambda: t["q"])[rows_of(B, None, device)].float().clone() if B > ROWS else dev(t["q"][:B], device)
            keep = q.clone()
            clean = run(q)
            assert same_words(q, keep), "q is unchanged by the call"
            q[list(rows)] = value
            keep = q.clone()
            got = run(q)
            assert same_words(q, keep), "q is unchanged by the call"
            others = torch.ones(B, dtype=torch.bool, device=device)
            others[list(rows)] = False
            assert len(got) == len(clean) == len(free)
            for a, b, f in zip(got, clean, free):
                changed = int((a[others] != b[others]).sum())
                assert changed == 0 and torch.isfinite(a[others]).all(), (what, B, value, "%d entries of other rows changed" % changed)
                for r in rows:
                    ok = torch.isfinite(a[r]) if value == BIG_ANGLE else ~torch.isfinite(a[r]) | (f & (a[r] == b[r]))
                    assert bool(ok.all()), (what, B, r, value, a[r], b[r])


def nan_rows_check(model, t, name):
    """neighbour_rows_check on compute_fk_and_jacobian and compute_forward_kinematics of one link"""
    free = q_independent(t["key"], name)
    neighbour_rows_check("%s %s" % (t["key"], name), t, lambda q: model.compute_fk_and_jacobian(q, name) + model.compute_forward_kinematics(q, name),
                         free + free[:2], model._device)


@functools.lru_cache(maxsize=None)
def q_independent_poses(key):
    """the entries of pos [L, 3] and quat [L, 4] of every link that do not see q at all, from the all-links truth of both seeds"""
    both = [truth(key, seed) for seed in SEEDS]
    return tuple(np.ptp(np.concatenate([t[k] for t in both]), axis=0) <= 1e-12 for k in ("P64", "Q64"))


def with_sentinel(call, T, device):
    """run(q) for neighbour_rows_check around a C ABI pose call(q, (pos, quat)): outputs pre-filled with NaN in allocations one row longer
    than the launch — no NaN may be left by a clean q (checked by the caller's finiteness conditions), the row behind keeps its sentinel"""
    def run(q):
        B = q.shape[0]
        bufs = [torch.full((B + 1, T, k), float("nan"), device=device) for k in (3, 4)]
        for b in bufs:
            b[B] = -7.25
        call(q, tuple(b[:B] for b in bufs))
        assert all((b[B] == -7.25).all() for b in bufs), "the row behind the launch keeps its sentinel"
        return tuple(b[:B] for b in bufs)
    return run


def pose_rows_check(what, t, links, call, device, sizes=FULL_AND_RAGGED):
    """the exact conditions of a many-pose C ABI call(q, (pos [B, T, 3], quat [B, T, 4])) over `links`: sentinel, q unchanged, NaN and
    |q| = 4.0e5 rows and their neighbours"""
    fp, fq = q_independent_poses(t["key"])
    neighbour_rows_check(what, t, with_sentinel(call, len(links), device), (fp[links], fq[links]), device, sizes)


def interface_check(model, t, name, B):
    """1-D q, a column-slice q and both values of `recursive` give the bits of the contiguous batched call (misaligned row slices: the
    [1:] views of the GPU tests, through the C ABI)"""
    device, n = model._device, model._n_dofs
    q = dev(t["q"][:B], device)
    ref = model.compute_fk_and_jacobian(q, name)
    fk = model.compute_forward_kinematics(q, name)
    same_bits(model.compute_forward_kinematics(q, name, recursive=True), fk, True, "%s %s recursive=True vs False" % (t["key"], name))
    same_bits(model.compute_forward_kinematics(q, name, recursive=False), fk, True, "%s %s recursive=False vs the default" % (t["key"], name))
    for r in (0, B - 1):
        one = model.compute_fk_and_jacobian(q[r], name)
        assert [tuple(o.shape) for o in one] == [(3,), (4,), (3, n), (3, n)]
        for a, b in zip(one, model.compute_fk_and_jacobian(q[r:r + 1].clone(), name)):
            assert torch.equal(a, b[0])
        for a, b in zip(model.compute_forward_kinematics(q[r], name), model.compute_forward_kinematics(q[r:r + 1].clone(), name)):
            assert a.ndim == 1 and torch.equal(a, b[0])
    wide = torch.full((B, n + 3), 9.5, device=device)
    wide[:, 2:2 + n] = q
    qs = wide[:, 2:2 + n]
    assert not qs.is_contiguous()
    same_bits(model.compute_fk_and_jacobian(qs, name), ref, True, "%s %s B=%d column-slice q vs contiguous" % (t["key"], name, B))
    same_bits(model.compute_forward_kinematics(qs, name), fk, True, "%s %s B=%d column-slice q vs contiguous, FK" % (t["key"], name, B))
    same_bits(model.compute_endeffector_jacobian(qs, name), ref[2:], True, "%s %s B=%d column-slice q vs contiguous, Jacobian" % (t["key"], name, B))
    assert (wide[:, :2] == 9.5).all() and (wide[:, 2 + n:] == 9.5).all() and torch.equal(wide[:, 2:2 + n], q)


def edges(model, key, name, Bs=(128, 65)):
    t = truth(key, 61)
    for B in Bs:
        sentinel_check(model, t, name, B)
        interface_check(model, t, name, B)
    nan_rows_check(model, t, name)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("seed", SEEDS + ("4e5",))
@pytest.mark.parametrize("key", ALL_ROBOTS + sorted(SLIDING))
def test_host_build_against_truth(cpu_library, key, seed):
    """the device="cpu" model through the public calls: every non-root link (the sliding models: the link of SLIDING)"""
    m, t = model_for(key), truth(key, seed)
    path = "host" if seed != "4e5" else "host-4e5"
    for link in (non_root(m) if ":" not in key else [link_index(m, SLIDING[key])]):
        api_link(m, path, t, t["names"][link])
    api_all_links(m, path, t)


@pytest.mark.parametrize("key", ALL_ROBOTS + sorted(SLIDING))
def test_host_build_edges(cpu_library, key):
    m = model_for(key)
    for name, _ in GPU_LINKS[key]:
        edges(m, key, name)
    if ":" not in key:
        many_pose_edges(m, key, "cpu")


def many_pose_edges(m, key, device):
    """the exact conditions of drm_fk with every link in walk order and, on the two hands, of drm_fk_fanout on the fingertips"""
    t = truth(key, 61)
    kernel, walk, order, keep = all_links_kernel(m, key)
    pose_rows_check("%s %s" % (key, kernel), t, order, lambda q, outs: abi_fk(walk, q, len(order), outs), device)
    if key in FINGERTIPS:
        tips, walks, keep = fan_structs(m, FINGERTIPS[key])
        pose_rows_check("%s drm_fk_fanout" % key, t, tips, lambda q, outs: abi_fanout(walks, len(tips), q, outs), device)


def emu_jac(emu, walk, t, fn="emu_fk_jacobian"):
    q = np.ascontiguousarray(t["q"])
    B, n = q.shape
    keep = q.copy()
    pos, quat = np.full((B, 3), np.nan, np.float32), np.full((B, 4), np.nan, np.float32)
    lin, ang = np.full((B, 3, n), np.nan, np.float32), np.full((B, 3, n), np.nan, np.float32)
    assert getattr(emu, fn)(ctypes.byref(walk), _ptr(q), ctypes.c_int64(B), _ptr(pos), _ptr(quat), _ptr(lin), _ptr(ang)) == 0
    assert np.array_equal(keep, q)
    return pos, quat, lin, ang


def emu_fk(emu, walk, t, T):
    q = np.ascontiguousarray(t["q"])
    B = q.shape[0]
    pos, quat = np.full((B, T, 3), np.nan, np.float32), np.full((B, T, 4), np.nan, np.float32)
    assert emu.emu_fk(ctypes.byref(walk), _ptr(q), ctypes.c_int64(B), T, _ptr(pos), _ptr(quat)) == 0
    return pos, quat


def cpu_struct(model, dw):
    from differentiable_robot_model_amd import backend
    return backend._walk_struct_build(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs)


@pytest.mark.parametrize("seed", SEEDS + ("4e5",))
@pytest.mark.parametrize("key", ALL_ROBOTS + sorted(SLIDING))
def test_emu_against_truth(emu, key, seed):
    """the host emulation of the loop kernels' arithmetic (csrc/drm_host_loops.hpp fk_loop, jac_loop) under g++ and the ROCm clang:
    emu_fk and emu_fk_jacobian on the single-target walk of every non-root link — the plain walk and the walk the API launches (fixed
    links folded) —, emu_fk on the all-links walk and on the all-links walk in walk order (fanned out behind a hub where the tree has one)"""
    m, t = model_for(key), truth(key, seed)
    tag = "" if seed != "4e5" else "-4e5"
    for link in (non_root(m) if ":" not in key else [link_index(m, SLIDING[key])]):
        prog = build_walk(m._spec, targets=[link])
        plain, keep = host_walk(m, prog)
        for walk, path in ((plain, "emu-plain-walk"), (cpu_struct(m, m._chain_walk(link)), "emu-api-walk")):
            check_jac("emu_fk_jacobian:" + path + tag, t, link, emu_jac(emu, walk, t))
            check_poses("emu_fk:" + path + tag, t, [link], *emu_fk(emu, walk, t, 1))
    if ":" in key:
        return
    for targets, path in ((non_root(m), "emu-all-links"), (all_links_order(m), "emu-all-links-fanned")):
        prog = build_walk(m._spec, targets=targets)
        if path.endswith("fanned") and key in ("allegro_left", "iiwa7_allegro", "trifinger_edu"):
            assert prog.shape & SHAPE_FK_FAN and len(prog.seg_begin) >= 3
        walk, keep = host_walk(m, prog)
        check_poses("emu_fk:" + path + tag, t, targets, *emu_fk(emu, walk, t, len(targets)))


@pytest.mark.parametrize("seed", SEEDS + ("4e5",))
@pytest.mark.parametrize("robot", ARM_ROBOTS)
def test_emu_arm_kernel_against_truth(emu, robot, seed):
    """emu_fk_jacobian_arm: the packed chain arithmetic of fk_jacobian_arm_kernel<8, 7> (fk_chain_pairs) on the last link of the three
    7-DoF arms, on the plain walk and on the walk the API launches"""
    m, t = model_for(robot), truth(robot, seed)
    link = len(m._bodies) - 1
    plain, keep = host_walk(m, build_walk(m._spec, targets=[link]))
    for walk, path in ((plain, "emu-plain-walk"), (cpu_struct(m, m._chain_walk(link)), "emu-api-walk")):
        assert instantiation_of(walk) == "arm"
        check_jac("emu_fk_jacobian_arm:" + path + ("" if seed != "4e5" else "-4e5"), t, link, emu_jac(emu, walk, t, "emu_fk_jacobian_arm"))


# ------------------------------------------------------------------------------------------------------------------- GPU
GPU = "cuda:0"
KEYS = ALL_ROBOTS + sorted(SLIDING)
LOOP_BITS = SHAPE_ARM_CHAIN | SHAPE_SERIAL_CHAIN
# What two rungs must show on the same 256 rows (RUNG IDENTITY in the module docstring) — True: the same bits, False: not the same bits
ARM_VS_LOOP = False             # lin_jac: packed two-joint sincos and pose pairs against the loop kernel's one joint at a time
CHAIN_LIN_VS_LOOP = False       # lin_jac of a link behind at least CHAIN_MOVING moving joints: z x p_e - z x p_k against z x (p_e - p_k)
CHAIN_MOVING = 3                # (with one or two, axes and origins can be exact in float32 — 2link_robot, iiwa_link_2 — and both forms agree)
FAN_VS_CHAINS = True            # the fan-out's walk is chain_fk_kernel's (chain_walk); its fixed last op taken as J = F is a joint at angle 0, exactly
FAN2_VS_FAN = False             # two samples per lane: fk_chain2_trig, another composition order
ARM_FORMS = True                # plain and streamed form: fk_chain_pairs on chain_trig; the register-resident form: the same operations in lock step


def fk_vs_jacobian_pose(inst):
    """compute_forward_kinematics against the pose of compute_fk_and_jacobian: one kernel template with and without the Jacobian on the
    chain and loop rungs (the same bits); on the arm rung the register-resident form against the plain FK-only form (reported: FOUND)"""
    return None if inst == "arm" else True


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 131, 256])
@pytest.mark.parametrize("key", KEYS)
def test_gpu_rungs_against_truth(key, B):
    """own_kernels = "off": every link of GPU_LINKS through the three public calls in launches of B rows — full tiles through the link's
    instantiation, the rest of the launch through the loop kernel; then all links in walk order, the all-links call and the fingertips"""
    m = model_for(key, GPU)
    for name, inst in GPU_LINKS[key]:
        assert instantiation_of(chain_struct(m, name)) == inst, (key, name)
        for seed in SEEDS:
            t = truth(key, seed)
            outs = api_link(m, path_name(inst, B), t, name, B, fk_bits=fk_vs_jacobian_pose(inst if B >= 64 else "loop"), chain_rung=inst.startswith("chain") and B >= 64)
            full = B // 64 * 64
            if seed == 61 and full and B % 64:
                q = dev(t["q"][:full], GPU)
                same_bits(tuple(o[:full] for o in outs), m.compute_fk_and_jacobian(q, name), True, "%s %s full tiles of B=%d alone" % (key, name, B))
            if seed == 61:
                again = sliced(lambda x: m.compute_fk_and_jacobian(x, name), dev(t["q"], GPU), B)
                same_bits(outs, again, True, "%s %s B=%d launched twice" % (key, name, B))
    if ":" not in key:
        for seed in SEEDS:
            api_all_links(m, "B%d" % B, truth(key, seed), B)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_gpu_loop_kernels_on_the_walks_of_the_fast_rungs(key):
    """The walk with its shape bits cleared through the C ABI: every row through fk_jacobian_tree_kernel / fk_tree_kernel.  Held to the
    requirement; compared bit for bit with the fast rung on the same rows; the kernel of a fast rung's ragged tail (its bits); the
    kernel of a [1:] view, whose pointers are 4 n (12, 16, 12 n) bytes off a 16-byte boundary (its bits; the row in front stays)."""
    m = model_for(key, GPU)
    n = m._n_dofs
    for name, inst in GPU_LINKS[key]:
        link = link_index(m, name)
        walk, loop_walk = chain_struct(m, name), chain_struct(m, name, clear_shape=LOOP_BITS)
        assert instantiation_of(loop_walk) == "loop"
        for seed in SEEDS:
            t = truth(key, seed)
            q = dev(t["q"], GPU)
            loop = abi_jac(loop_walk, q)
            check_jac("loop-abi-B256", t, link, loop)
            loop_fk = abi_fk(loop_walk, q)
            check_poses("fk:loop-abi-B256", t, [link], *loop_fk)
            lin_only = abi_jac(loop_walk, q, pose=False)
            assert torch.isnan(lin_only[0]).all() and torch.isnan(lin_only[1]).all()
            same_bits(lin_only[2:], loop[2:], True, "%s %s loop kernel without a pose vs with" % (key, name))
            fast, fast_fk = abi_jac(walk, q), abi_fk(walk, q)
            moving = int((jac_truth(t, link)["cls"] >= PRISMATIC).sum())
            expect = ARM_VS_LOOP if inst == "arm" else (CHAIN_LIN_VS_LOOP if moving >= CHAIN_MOVING else None)
            same_bits(fast[2], loop[2], expect, "%s %s %s vs loop kernel, lin_jac" % (key, name, inst))
            same_bits((fast[0], fast[1], fast[3]), (loop[0], loop[1], loop[3]), None, "%s %s %s vs loop kernel, pos quat ang_jac" % (key, name, inst))
            same_bits(fast_fk, loop_fk, None, "%s %s %s vs loop kernel, FK alone" % (key, name, inst))
            same_bits(fast, m.compute_fk_and_jacobian(q, name), True, "%s %s C ABI vs the public call" % (key, name))
            # the ragged tail of a launch of one tile + 1 row is that row through the loop kernel
            tail = m.compute_fk_and_jacobian(dev(t["q"][:65], GPU), name)
            same_bits(tuple(o[64:] for o in tail), tuple(o[64:65] for o in loop), True, "%s %s tail row of B=65 vs loop kernel" % (key, name))
            tail = m.compute_forward_kinematics(dev(t["q"][:65], GPU), name)
            same_bits(tuple(o[64:] for o in tail), tuple(o[64:65, 0] for o in loop_fk), True, "%s %s tail row of B=65 vs loop kernel, FK alone" % (key, name))
            # a [1:] view of q and of every output
            outs = tuple(torch.full((ROWS,) + s, float("nan"), device=GPU) for s in ((3,), (4,), (3, n), (3, n)))
            views = [x[1:] for x in (q,) + outs]
            assert views[1].data_ptr() % 16 == 12, "pos, at least, is off a 16-byte boundary"
            abi_jac(walk, views[0], tuple(views[1:]))
            assert all(torch.isnan(o[0]).all() for o in outs), "the row in front of the view is not written"
            same_bits(tuple(o[1:] for o in outs), tuple(o[1:] for o in loop), True, "%s %s [1:] view vs loop kernel on aligned rows" % (key, name))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "panda"])
def test_gpu_misaligned_call_beyond_one_grid_of_tiles(robot):
    """A [1:] view of 65 * 64 + 1 rows through the C ABI (q and the outputs 4 n, 12 and 12 n bytes off a 16-byte boundary; n = 7, 9): the
    loop kernel on all 65 tiles and the ragged row.  Every row against its truth row; the bits of the loop kernel on aligned rows."""
    m = model_for(robot, GPU)
    n, name = m._n_dofs, GPU_LINKS[robot][0][0]
    link, t = link_index(m, name), truth(robot, 61)
    N = (MISALIGNED_TILES + 1) * 64 + 1
    idx = np.arange(N) % ROWS
    q = dev(t["q"][idx], GPU)
    outs = tuple(torch.full((N,) + s, float("nan"), device=GPU) for s in ((3,), (4,), (3, n), (3, n)))
    views = [x[1:] for x in (q,) + outs]
    assert views[1].data_ptr() % 16 == 12, "pos, at least, is off a 16-byte boundary"
    abi_jac(chain_struct(m, name), views[0], tuple(views[1:]))
    assert all(torch.isnan(o[0]).all() for o in outs), "the row in front of the view is not written"
    check_jac("loop-misaligned", t, link, tuple(o[1:] for o in outs), idx[1:])
    loop = abi_jac(chain_struct(m, name, clear_shape=LOOP_BITS), q[1:257].clone())
    same_bits(tuple(o[1:257] for o in outs), loop, True, "%s %s misaligned call vs the loop kernel on aligned rows" % (robot, name))
    assert all(repeats(o[1:], N - 1) for o in outs)
    torch.cuda.synchronize()


def repeats(out, N, period=ROWS):
    """rows share nothing: every repetition of the 256 rows carries the bits of the first"""
    reps = N // period
    out = out.reshape(out.shape[0], -1)
    return torch.equal(out[:reps * period].view(reps, period, -1), out[:period].expand(reps, -1, -1)) and torch.equal(out[reps * period:N], out[:N - reps * period])


def sized_jac(m, key, name, path, N, small=None, forms=None):
    """every row of ONE launch of N tiled rows against its truth row, on the device; its first 256 rows against `small` (the same rows
    through the form a small launch takes: expectation `forms`); the |q| = 4.0e5 rows; the sentinel behind the launch"""
    link = link_index(m, name)
    n = m._n_dofs
    for seed in (61, "4e5"):
        t = truth(key, seed)
        idx = np.arange(N) % ROWS
        q = on_device(t, GPU, "q", lambda: t["q"])[rows_of(N, None, GPU)]
        keep = q.clone()
        bufs = [torch.full((N + 1,) + s, float("nan"), device=GPU) for s in ((3,), (4,), (3, n), (3, n))]
        for b in bufs:
            b[N] = -7.25
        outs = abi_jac(chain_struct(m, name), q, tuple(b[:N] for b in bufs))
        check_jac(path + ("" if seed == 61 else "-4e5"), t, link, outs, idx, chain_rung=path.startswith("chain"))
        assert all((b[N] == -7.25).all() for b in bufs) and torch.equal(keep, q)
        full = N // 64 * 64
        assert all(repeats(o, full) for o in outs)
        if seed == 61:
            same_bits(outs, m.compute_fk_and_jacobian(q, name), True, "%s %s %s C ABI vs the public call" % (key, name, path))
            if small is not None:
                same_bits(tuple(o[:ROWS] for o in outs), small, forms, "%s %s %s first 256 rows vs the small launch" % (key, name, path))
            loop = abi_jac(chain_struct(m, name, clear_shape=LOOP_BITS), q[full:].clone())
            same_bits(tuple(o[full:] for o in outs), loop, True, "%s %s %s tail rows vs loop kernel" % (key, name, path))
    return outs


def rows_past_llc(bytes_per_row):
    """the smallest count of full tiles whose outputs pass stream_past_llc, in rows"""
    tiles = LLC_BYTES // (64 * bytes_per_row) + 1
    assert tiles * 64 * bytes_per_row > LLC_BYTES >= (tiles - 1) * 64 * bytes_per_row
    return tiles * 64


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "streamed"])
def test_gpu_arm_forms_that_need_size(form):
    """fk_jacobian_arm_kernel<8, 7> on panda_no_gripper beyond DRM_PRE_MAX_TILES tiles (the plain form, 2 049 tiles + 3 rows) and with
    outputs beyond 256 MiB (the streamed multi-wave form, + 3 rows), every row of the launch; the first 256 rows against the
    register-resident form of a 256-row launch"""
    key, (name, inst) = "panda_no_gripper", GPU_LINKS["panda_no_gripper"][0]
    m = model_for(key, GPU)
    assert inst == "arm" and instantiation_of(chain_struct(m, name)) == "arm"
    N = ((PRE_MAX_TILES + 1) * 64 if form == "plain" else rows_past_llc(4 * (7 + 6 * 7))) + 3
    small = m.compute_fk_and_jacobian(dev(truth(key, 61)["q"], GPU), name)
    sized_jac(m, key, name, "arm-%s+tail" % form, N, small, ARM_FORMS)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_chain_kernel_streamed_past_the_infinity_cache():
    """chain_fk_kernel<12, 12, JAC, NT = true>: an iiwa7_allegro fingertip (23 columns, 580 B of outputs per row — the fewest rows of any
    shipped chain) with outputs beyond 256 MiB, + 3 rows; the first 256 rows carry the bits of the cached-store form"""
    key, (name, inst) = "iiwa7_allegro", GPU_LINKS["iiwa7_allegro"][0]
    m = model_for(key, GPU)
    assert m._n_dofs == 23 and inst == "chain<12,12>"
    N = rows_past_llc(4 * (7 + 6 * 23)) + 3
    small = m.compute_fk_and_jacobian(dev(truth(key, 61)["q"], GPU), name)
    sized_jac(m, key, name, "chain<12,12>-streamed+tail", N, small, True)
    torch.cuda.synchronize()


def fan_structs(m, tips):
    from differentiable_robot_model_amd import backend
    order = [link_index(m, nm) for nm in tips]
    dw = m._get_walk(("fk", tuple(order)), targets=order)
    fan = m._fanout_chains(order, dw)
    assert fan is not None, "the fingertips of a hand take drm_fk_fanout"
    walks = (backend.DrmWalk * len(fan))()
    keep = []
    for k, c in enumerate(fan):
        ops_f = m._ops_f(c).detach()
        keep.append(ops_f)
        walks[k] = backend._walk_struct_build(c.program, ops_f, c.ops_i, m._n_dofs)
    return order, walks, keep


def abi_fanout(walks, T, q, outs=None):
    from differentiable_robot_model_amd import backend
    lib, stream = library_and_stream(q.device)
    B = q.shape[0]
    if outs is None:
        outs = tuple(torch.full((B, T, k), float("nan"), device=q.device) for k in (3, 4))
    backend._check(lib.drm_fk_fanout(walks, T, ctypes.c_void_p(q.data_ptr()), ctypes.c_int64(B), ctypes.c_void_p(outs[0].data_ptr()),
                                     ctypes.c_void_p(outs[1].data_ptr()), stream), lib)
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("robot", sorted(FINGERTIPS))
def test_gpu_fan_out_rungs(robot):
    """drm_fk_fanout on the fingertips: fk_fan_chain_kernel (the form without trigonometry on the fixed fingertip frame: every chain of
    both hands ends in one) on full tiles, fk_fanout_kernel on a ragged tail and below 64 rows, fk_fan_chain2_kernel from
    DRM_FAN2_MIN_TILES pairs of tiles on — 2 048 pairs + one odd tile + 5 rows, every row.  Against the single-target chains."""
    m = model_for(robot, GPU)
    tips = FINGERTIPS[robot]
    order, walks, keep = fan_structs(m, tips)
    T = len(tips)
    assert all(instantiation_of(w).startswith("chain") and not w.chain_dof1[w.n_ops - 1] for w in walks), "every chain ends in a fixed frame"
    for seed in SEEDS:
        t = truth(robot, seed)
        q = dev(t["q"], GPU)
        outs = {}
        for B in (256, 65, 63):
            outs[B] = sliced(lambda x: abi_fanout(walks, T, x), q, B)
            check_poses("fan%s-B%d" % ("" if B == 256 else "+tail" if B == 65 else "out-loop", B), t, order, *outs[B])
            same_bits(outs[B], sliced(lambda x: m._fk_targets(x, order), q, B), True, "%s B=%d drm_fk_fanout vs _fk_targets" % (robot, B))
        single = tuple(torch.stack([m.compute_forward_kinematics(q, nm)[k] for nm in tips], 1) for k in (0, 1))
        same_bits(outs[256], single, FAN_VS_CHAINS, "%s fan-out vs the single-target chain kernels" % robot)
        same_bits(outs[63], outs[256], None, "%s fk_fanout_kernel vs fk_fan_chain_kernel" % robot)
        same_bits(tuple(o[:64] for o in outs[65]), tuple(o[:64] for o in outs[256]), True, "%s full tile of B=65 alone" % robot)
        same_bits(tuple(o[64:65] for o in outs[65]), tuple(o[64:65] for o in outs[63]), True, "%s tail row of B=65 vs fk_fanout_kernel of B=63" % robot)
    # two samples per lane
    N = (2 * FAN2_MIN_TILES + 1) * 64 + 5
    for seed in (61, "4e5"):
        t = truth(robot, seed)
        q = on_device(t, GPU, "q", lambda: t["q"])[rows_of(N, None, GPU)]
        bufs = [torch.full((N + 1, T, k), float("nan"), device=GPU) for k in (3, 4)]
        for b in bufs:
            b[N] = -7.25
        big = abi_fanout(walks, T, q, tuple(b[:N] for b in bufs))
        check_poses("fan2+odd+tail" + ("" if seed == 61 else "-4e5"), t, order, *big, idx=np.arange(N) % ROWS)
        assert all((b[N] == -7.25).all() for b in bufs)
        pairs = 2 * FAN2_MIN_TILES * 64
        assert all(repeats(o[:pairs], pairs) and repeats(o[pairs:], 64, 64) for o in big)
        if seed == 61:
            one = abi_fanout(walks, T, q[:ROWS].clone())
            same_bits(tuple(o[:ROWS] for o in big), one, FAN2_VS_FAN, "%s two samples per lane vs one" % robot)
            same_bits(tuple(o[pairs:pairs + 64] for o in big), tuple(o[:64] for o in one), True, "%s the odd tile is the one-sample kernel's" % robot)
            same_bits(big, m._fk_targets(q, order), True, "%s fan2 C ABI vs _fk_targets" % robot)
    # the exact conditions: full tiles and a ragged tail (65 rows: the tail starts at an offset pointer), fewer than 64 rows, and the
    # pair-tile launch with rows set in one pair of tiles (rows 5 and 70: lane partners 69 and 6), in the odd tile and in the tail
    t = truth(robot, 61)
    call = lambda q, outs: abi_fanout(walks, T, q, outs)
    pose_rows_check("%s drm_fk_fanout" % robot, t, order, call, GPU, FULL_AND_RAGGED + ((65, (3, 64)), (63, (0, 62))))
    pose_rows_check("%s drm_fk_fanout, pairs of tiles" % robot, t, order, call, GPU, ((N, (5, 70, pairs + 9, N - 2)),))
    torch.cuda.synchronize()


def all_links_kernel(m, key):
    """(the kernel drm_fk launches for every link in walk order — read off csrc/drm_fk.hip —, the walk's struct, the links, what to keep)"""
    from differentiable_robot_model_amd import backend
    from differentiable_robot_model_amd.flatten import SHAPE_TARGETS_ORDERED
    order = all_links_order(m)
    T, n = len(order), m._n_dofs
    dw = m._get_walk(("fk", tuple(order)), targets=order)
    ops_f = m._ops_f(dw).detach()
    walk = backend._walk_struct_build(dw.program, ops_f, dw.ops_i, n)
    assert walk.shape & SHAPE_TARGETS_ORDERED
    pad_odd = lambda x: x | 1
    round4 = lambda x: (x + 3) // 4 * 4
    lds_fan = 4 * (round4(walk.n_ops * 32) + round4(2 * walk.n_ops) + round4(64 * pad_odd(n)) + walk.n_slots * 12 * 64 + round4(64 * pad_odd(3 * T)) +
                   round4(64 * pad_odd(4 * T)))
    fanned = bool(walk.shape & SHAPE_FK_FAN) and 2 <= walk.n_segments <= 8 and lds_fan <= 80 * 1024
    kernel = "fk_tree_kernel" if T <= 8 else ("fk_tree_fan_kernel" if fanned else "fk_tree_groups_kernel")
    print("FKRUNG-ALL-LINKS %-34s T %2d ops %2d segments %d hub prefix %d slots %d: %s (%d B of LDS fanned out)" % (
        key, T, walk.n_ops, walk.n_segments, walk.prefix_end, walk.n_slots, kernel, lds_fan))
    return kernel, walk, order, (dw, ops_f)


@pytest.mark.parametrize("key", ALL_ROBOTS)
def test_all_links_kernel_table(cpu_library, key):
    """ALL_LINKS_KERNEL against the walk (the host build has the same walks)"""
    assert all_links_kernel(model_for(key), key)[0] == ALL_LINKS_KERNEL[key]


@pytest.mark.gpu
@pytest.mark.parametrize("key", ALL_ROBOTS)
def test_gpu_all_links_rungs(key):
    """drm_fk with every link as a target in walk order: fk_tree_fan_kernel (a hub and the LDS bound), fk_tree_groups_kernel (T > 8
    otherwise), fk_tree_kernel (T <= 8) — which one is read off the walk and asserted; full tiles, a ragged tail, fewer than 64 rows
    and a [1:] view give the same bits (one kernel at every size and alignment)"""
    from differentiable_robot_model_amd import backend
    from differentiable_robot_model_amd.flatten import SHAPE_TARGETS_ORDERED
    m = model_for(key, GPU)
    kernel, walk, order, keep = all_links_kernel(m, key)
    assert kernel == ALL_LINKS_KERNEL[key]
    T = len(order)
    for seed in SEEDS + ("4e5",):
        t = truth(key, seed)
        q = dev(t["q"], GPU)
        tag = "" if seed != "4e5" else "-4e5"
        outs = abi_fk(walk, q, T)
        check_poses("%s-B256%s" % (kernel, tag), t, order, *outs)
        for B in (65, 63, 1):
            part = sliced(lambda x: abi_fk(walk, x, T), q, B)
            same_bits(part, outs, True, "%s %s B=%d vs B=256" % (key, kernel, B))
        same_bits(outs, m._fk_targets(q, order), True, "%s %s C ABI vs _fk_targets" % (key, kernel))
        bufs = tuple(torch.full((ROWS + 1, T, k), float("nan"), device=GPU) for k in (3, 4))
        for b in bufs:
            b[ROWS] = -7.25
        abi_fk(walk, q[1:], T, tuple(b[1:ROWS] for b in bufs))
        assert all(torch.isnan(b[0]).all() and (b[ROWS] == -7.25).all() for b in bufs)
        same_bits(tuple(b[1:ROWS] for b in bufs), tuple(o[1:] for o in outs), True, "%s %s [1:] view vs aligned rows" % (key, kernel))
    pose_rows_check("%s %s" % (key, kernel), truth(key, 61), order, lambda q, o: abi_fk(walk, q, T, o), GPU, FULL_AND_RAGGED + ((63, (0, 62)),))
    torch.cuda.synchronize()


# the many-target kernel of every robot's all-links walk in walk order (drm_fk; asserted against the walk in test_gpu_all_links_rungs)
ALL_LINKS_KERNEL = dict({r: "fk_tree_kernel" for r in ("2link_robot", "fetch_arm_no_gripper", "fetch_arm_no_gripper_small_damping", "iiwa7", "panda_no_gripper")},
                        **{r: "fk_tree_fan_kernel" for r in ("allegro_left", "allegro_left_small_damping", "iiwa7_allegro", "trifinger_edu")},
                        **{r: "fk_tree_groups_kernel" for r in ("fetch", "jaco", "jaco_clean", "panda")})


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["panda_no_gripper", "iiwa7_allegro", "allegro_left", "fetch:sliding"])
def test_gpu_plans_and_repeat_calls(key):
    """plan_fk_and_jacobian with and without a pose, eager and replayed from a captured graph: with a pose the rung and the bits of the
    direct call; without one (pos = quat = NULL: neither straight-line rung takes the launch, see drm_fk_jacobian and
    launch_chain_fk_jacobian) the loop kernel — its bits, and the requirement.  The first, second and third call of
    compute_fk_and_jacobian (the Python path, then the prepared C++ call) are bit-equal, again after own_kernels is toggled."""
    m = model_for(key, GPU)
    name, inst = GPU_LINKS[key][0]
    link = link_index(m, name)
    for B in (256, 65):
        for seed in SEEDS:
            t = truth(key, seed)
            q = dev(t["q"][:B], GPU)
            direct = m.compute_fk_and_jacobian(q, name)
            loop = abi_jac(chain_struct(m, name, clear_shape=LOOP_BITS), q)
            for want_pose in (True, False):
                plan = m.plan_fk_and_jacobian(q, name, want_pose=want_pose)
                plan.launch()
                eager = tuple(None if o is None else o.clone() for o in plan.outputs())
                for o in plan.outputs():
                    if o is not None:
                        o.fill_(float("nan"))
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    plan.launch()
                for o in plan.outputs():
                    if o is not None:
                        o.fill_(float("nan"))
                g.replay()
                torch.cuda.synchronize()
                replayed = plan.outputs()
                path = "plan%s-B%d" % ("" if want_pose else "-no-pose", B)
                check_jac(path, t, link, replayed, np.arange(B), chain_rung=want_pose and inst.startswith("chain"))
                if want_pose:
                    same_bits(eager, direct, True, "%s %s %s eager vs the direct call" % (key, name, path))
                    same_bits(replayed, direct, True, "%s %s %s replayed vs the direct call" % (key, name, path))
                else:
                    assert eager[0] is None and eager[1] is None
                    same_bits(eager[2:], loop[2:], True, "%s %s %s eager vs the loop kernel" % (key, name, path))
                    same_bits(replayed[2:], loop[2:], True, "%s %s %s replayed vs the loop kernel" % (key, name, path))
    t = truth(key, 61)
    free = q_independent(key, name)
    for want_pose in (True, False):
        def through_plan(q):
            plan = m.plan_fk_and_jacobian(q, name, want_pose=want_pose)
            for o in plan.outputs():
                if o is not None:
                    o.fill_(float("nan"))
            plan.launch()
            return tuple(o for o in plan.outputs() if o is not None)
        neighbour_rows_check("%s %s plan, want_pose=%s" % (key, name, want_pose), t, through_plan, free if want_pose else free[2:], GPU)
    q = dev(t["q"], GPU)
    for mode in ("off", None, "off"):
        m.own_kernels = mode
        m._fast_jac.clear(); m._fast_fk.clear()
        calls = [m.compute_fk_and_jacobian(q, name) for _ in range(3)]
        assert name in m._fast_jac or m._learnable, "the second call went through the prepared entry"
        fks = [m.compute_forward_kinematics(q, name) for _ in range(3)]
        for k in (1, 2):
            same_bits(calls[k], calls[0], True, "%s %s own_kernels=%s call %d vs the first" % (key, name, mode, k + 1))
            same_bits(fks[k], fks[0], True, "%s %s own_kernels=%s FK call %d vs the first" % (key, name, mode, k + 1))
        check_jac("repeat-%s" % mode, t, link, calls[2], chain_rung=inst.startswith("chain"))
    m.own_kernels = "off"
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_gpu_edges(key):
    """the exact conditions on the library's rungs — 128 rows (full tiles), 65 and 131 rows (a fast rung + a tail that starts at an offset
    pointer), 63 rows (the loop kernel) — and the |q| = 4.0e5 rows on every link of GPU_LINKS"""
    m = model_for(key, GPU)
    t4 = truth(key, "4e5")
    for name, inst in GPU_LINKS[key]:
        edges(m, key, name, Bs=(128, 65, 131, 63))
        for B in (256, 65, 3):
            api_link(m, path_name(inst, B) + "-4e5", t4, name, B, fk_bits=None, chain_rung=inst.startswith("chain") and B >= 64)
    if ":" not in key:
        api_all_links(m, "B256-4e5", t4)
    torch.cuda.synchronize()


@pytest.mark.parametrize("key", KEYS)
def test_gpu_links_table(cpu_library, key):
    """GPU_LINKS against the walks (the host build has the same walks): the instantiation named for each link is the one its walk takes"""
    m = model_for(key)
    for name, inst in GPU_LINKS[key]:
        assert instantiation_of(chain_struct(m, name)) == inst, (key, name)


def test_every_reachable_instantiation_is_in_gpu_links(cpu_library):
    """every kernel instantiation a non-root link of a shipped robot reaches has a link in GPU_LINKS; CAP = 16 is reached by none"""
    reached = set()
    for key in ALL_ROBOTS:
        m = model_for(key)
        reached |= {instantiation_of(chain_struct(m, m._bodies[i].name)) for i in non_root(m)}
    listed = {inst for links in GPU_LINKS.values() for _, inst in links}
    assert reached == listed == {"arm", "chain<4,4>", "chain<8,6>", "chain<8,8>", "chain<12,10>", "chain<12,12>"}, (reached, listed)

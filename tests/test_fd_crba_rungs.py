"""Forward dynamics and the joint-space inertia matrix on every rung of their dispatch (csrc/drm_forward_dynamics.hip drm_forward_dynamics,
csrc/drm_crba.hip drm_crba; DifferentiableRobotModel.compute_forward_dynamics / compute_lagrangian_inertia_matrix), row by row against fp64.

INPUTS: for every robot of helpers.ALL_ROBOTS 256 rows of sample_states(m, 256, seed=61) and a second set with seed=7.  Torques "rand":
default_rng(3).uniform(-1, 1, (256, n)) as float32, under all four (include_gravity, use_damping); torques "id": float32 of the fp64
Oracle.rnea(q, qd, qdd) of the drawn qdd (forward dynamics undoing inverse dynamics), under (1, 1) and (0, 0).  H on the same q.

TRUTH, from the fp64 oracle only: qdd64 = Oracle.forward_dynamics, H64 = Oracle.mass_matrix(q, False, False), nle64 = Oracle.rnea(q, qd, 0).
Before anything under test is compared, np.linalg.solve(H64, f - nle64) must equal qdd64 to 1e-10 of each row's largest entry, and no
row and no joint column of qdd64 may be identically zero (so no metric needs a floor).

METRICS, in fp64, the worst over the batch:
    row    per row    max_i |dqdd_i| / max_i |qdd64_i|
    joint  per joint  max_b |dqdd_bi| / max_b |qdd64_bi|   (a joint whose accelerations are small beside the fingers' at its own scale)
    resid  per row    max_i |H64 qdd + nle64 - f|_i / (max_i (|H64| |qdd|)_i + max_i |f_i| + max_i |nle64_i|)   (the backward error: it
           stays near 1e-7 where cond(H) makes `row` vacuous — allegro_left, "id", (1, 1): kernel and yardstick are both 5e-2 .. 9e-2 off)
    H      max_bij |dH_ij| / sqrt(H64_ii H64_jj)
YARDSTICKS, not code under test: for H Oracle.mass_matrix(float32); for forward dynamics the largest error of three float32 solutions:
Oracle.forward_dynamics(float32) (the articulated-body recursion), np.linalg.solve in float32 of Oracle.mass_matrix(float32) against
f - Oracle.rnea(q, qd, 0, float32) (LU with partial pivoting), and ltdl_solve_numpy below of the same float32 system: the elimination
H = L^T D L from the last joint towards the first restated in numpy, which must equal qdd64 to 1e-8 when it runs in fp64.
    Why the third: against the first two alone forward_dynamics_arm_kernel and drm_fd_arm_static miss the requirement on the MI355X for
    iiwa7, seed 61, "rand", (0, 0): `joint` 6.3e-6 (6.5e-6) against 7.8e-7, 8.13x (8.33x).  tests/host_emu fd_arm_8_7 under clang gives
    the arm kernel's bits: 8.13x there, 8.40x under (0, 1).  The kernel's float32 H and bias torques solved exactly meet the yardstick
    at 0.9x .. 1.8x and the residual is 0.7x, so the loss is in the solve: row 78 has q1 = 0.05, joints 0 and 2 nearly parallel, the last pivot D_0 = 0.055 is what six
    eliminations leave of H_00 = 1.44, and it carries 5.5e-6.  LU and the articulated-body recursion meet this cancellation first, on
    exact inputs; the distal-first order (chosen for gram-scale fingers, drm_sample.hpp) meets it last.  The numpy elimination of the
    ORACLE's float32 H in that order loses the same: 2.7e-6 .. 5.4e-6 for iiwa7.  Rounding order, not a defect of the kernel.
    Asserted, not only told: test_emu_arm_forward_dynamics_against_truth solves the emulated float32 H and bias torques in fp64 and holds
    the result to the first two yardsticks alone (worst 3.27x), so what the arm kernel loses beyond them it loses in the elimination.
REQUIREMENT: err(path) <= 8 max(err(yardstick), 2^-23) for each metric (8: the project's margin for a different summation order, as in
test_energy.py, test_links.py, test_lagrangian.py); H bit-symmetric and positive definite (eigvalsh of the fp64 cast > 0).
Every comparison prints one "FDCRBA" line (robot, path, flags, torque set, metric, error, yardstick, ratio) before it asserts;
profiles/fd_crba_tests.txt holds, for the host build and the MI355X, the worst of them per path and metric (all of them are 0.6 MB).

PATHS without a GPU: the device="cpu" model through the public API; the host emulation of the kernel arithmetic under g++ and clang —
emu_forward_dynamics and emu_crba on the whole-tree and on the folded walk, emu_forward_dynamics_arm (LINKS = 7 and 8),
emu_forward_dynamics_arm_hand, emu_crba_arm, emu_crba_arm_hand — and the generated straight-line source of Fetch (static_fd,
static_crba) compiled for the host.  Each of them also takes the zero input and the |q| = 4.0e5 rows.

PATHS on the GPU (-m gpu).  A launch of B rows is repeated over consecutive slices of the 256 rows, so the statistic is over the same
rows whatever B is: B = 64 and 256 full tiles, 65 and 131 a fast rung plus a ragged tail in the loop kernel, 1 and 63 the loop kernel
alone; rows of full tiles are bit-equal with and without a tail behind them.  What sends a launch to a rung (RUNGS below):
    own        special[DRM_SPECIAL_FD] / special[DRM_SPECIAL_CRBA] set (model.specialize(); Fetch), full tiles
    fingers    DRM_WALK_FINGERS in the shape word, full tiles (allegro_left L = 4, trifinger_edu L = 3); H: crba_tree_kernel at every B
    arm-own    DRM_WALK_ARM_CHAIN, full tiles, 16-byte aligned pointers, special[DRM_SPECIAL_FD_ARM] / [CRBA_ARM] set (specialize())
    arm        the same with own_kernels = "off": forward_dynamics_arm_kernel / crba_arm_kernel <8, 7, 7> (the API's walk: fixed tail
               folded) and <8, 7, 8> (the unfolded 8-op walk through the C ABI: arm_links(w) == 8)
    arm-hand   DRM_WALK_ARM_HAND, full tiles, own_kernels = "off" (panda, jaco, iiwa7_allegro)
    loop       what is left: forward_dynamics_tree_kernel / crba_tree_kernel (segments of <= 6 ops) or the persistent
               forward_dynamics_aba_kernel / crba_rows_kernel; reached by B < 64, by a ragged tail, by the walk with its shape bit
               cleared through the C ABI, and by a [1:] view (pointers 4 n bytes off a 16-byte boundary)
Two rungs that compute the same rows with different arithmetic must NOT agree bit for bit, two launches of one kernel must: a dispatch
change that silently drops a rung fails a test.
RUNGS that need size (the 256 rows tiled cyclically, every row of the launch compared): drm_fd_arm2_static at 2 * 64 *
DRM_ARM_STATIC_MIN_PAIRS rows + one odd tile + 3; the persistent grids of Fetch at 2049 * 64 + 3 rows (more tiles than resident blocks);
a [1:] view of 65 * 64 + 1 rows of panda_no_gripper and panda (more than MISALIGNED_TILES tiles on a capped grid);
launch_crba_fingers_tree on trifinger_edu at 2048 * 64 + 70 rows.  The first two also take zero input, a NaN row in the first tile
and an Inf row in the ragged tail; all of them the |q| = 4.0e5 rows.

EXACT, on the host build and on the GPU: f = 0, qd = 0, gravity off gives qdd == 0; q, qd, f unchanged by the call; an output pre-filled
with NaN has no NaN in its B rows and the row behind them keeps its sentinel; a row with one |q| = 4.0e5 (fp64 sincos fallback) meets
the requirement like every other; an all-NaN q row and an all-Inf f row come back non-finite in every entry of qdd (H of the NaN
row: non-finite somewhere; its structural zeros stay) and change no bit of the other rows, once in full tiles (128 rows, rows 5 and
70) and once in a ragged tail (127 rows, rows 70 and 100); H ignores its flags to
the bit; 1-D arguments and a column-slice q give the bits of the contiguous batched call; compute_forward_dynamics_old ==
compute_forward_dynamics(..., True, True) to the bit on every robot.

FOUND by this module: inertia_to_parent (drm_sample.hpp) formed the diagonal of 2 (w . t) E - w t^T - t w^T as the full dot product
minus 2 w_i t_i, which cancels where a link's offset lies along the next joint's axis: H_22 = 0.0163 of fetch_arm_no_gripper came out
3.7e-8 off under clang, 9.3x .. 9.7x the yardstick (1.9x under g++).  The diagonal is now summed entry by entry: 1.3x .. 1.7x.

MEASURED (profiles/fd_crba_tests.txt), worst err / yardstick over both seeds, both torque sets and all flags, per metric:
                                              row    joint  resid  H
    host build, host emulation, static source 2.49   2.34   1.58   1.93     (iiwa7: emu loop walks and fd_arm; H: emu_crba_arm)
    MI355X, all rungs                         2.48   2.38   1.25   1.93
      own / own+tail (Fetch)                  0.96   0.82   1.04   1.42
      arm-own, arm-own+tail                   2.48   2.38   1.25   1.93
      arm2-own + odd tile + tail              1.16   1.41   0.98   -
      arm<8,7,7>, +tail                       2.43   2.34   1.21   1.42
      arm<8,7,8>, +tail                       2.37   2.34   1.21   1.42
      arm-hand, +tail                         1.12   1.05   0.99   1.37
      fingers, +tail; fingers-tree (H)        1.67   1.75   1.07   1.16
      loop (B < 64, shape bit cleared, hands' H) 1.76 1.87  1.13   1.52
      loop, misaligned beyond the capped grid 0.79   0.85   1.07   1.11
      loop, persistent beyond resident blocks 0.94   0.30   0.65   1.17
      the other five robots, B = 65 and 256   1.41   2.32   1.25   1.40
      |q| = 4.0e5 rows (every rung)           1.40   1.46   1.25   1.93
MUTATIONS on a scratch copy of the host emulation, both caught: the last diagonal entry of allegro_left's H set to zero (H: 1.0 against
2.7e-7; TOL_TAU's atol 2e-5 passes it); one pivot of the unrolled L^T D L solve scaled by 1 + 1e-4 (row and joint 1e-4 against 2e-6,
resid 9e-6 against 2e-7).
NO HOST EMULATION: the two-samples-per-lane solve of drm_fd_arm2_static; the GPU test holds every one of its 131 139 rows.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from differentiable_robot_model_amd import specialize as sp
from differentiable_robot_model_amd.flatten import SHAPE_ARM_CHAIN, SHAPE_ARM_HAND, SHAPE_FINGERS, build_walk
from helpers import ALL_ROBOTS, load_model, sample_states
from oracle import Oracle
from test_host_emu import _ptr, arm_hand_case, emu, folded_host_walk, host_walk  # noqa: F401  (emu is a fixture)

needs_hipcc = pytest.mark.skipif(sp.hipcc() is None, reason="hipcc not on this machine")

ROWS, FLOOR, MARGIN = 256, 2.0 ** -23, 8.0
SEEDS = (61, 7)
FLAGS = ((1, 0), (1, 1), (0, 0), (0, 1))
CASES = tuple(("rand", g, d) for g, d in FLAGS) + (("id", 1, 1), ("id", 0, 0))
BIG_ANGLE = 4.0e5
LARGE_ANGLE_CASES = (("rand", 1, 1), ("id", 0, 0))
ARM_STATIC_MIN_PAIRS = 1024             # DRM_ARM_STATIC_MIN_PAIRS (csrc/drm_common.hpp)

ARM_ROBOTS = ("panda_no_gripper", "iiwa7", "fetch_arm_no_gripper")
FINGER_ROBOTS = ("allegro_left", "trifinger_edu")
ARM_HAND_ROBOTS = ("panda", "jaco", "iiwa7_allegro")
# robot -> the fast rung its full aligned tiles take with own_kernels = "off" (None: the loop kernels at every size)
RUNGS = dict({r: "arm" for r in ARM_ROBOTS}, **{r: "fingers" for r in FINGER_ROBOTS}, **{r: "arm-hand" for r in ARM_HAND_ROBOTS})
RUNG_ROBOTS = ARM_ROBOTS + FINGER_ROBOTS + ARM_HAND_ROBOTS + ("fetch", "2link_robot")


# ------------------------------------------------------------------------------------------------------------------- truth
@functools.lru_cache(maxsize=None)
def model_on(robot, device="cpu", own="default"):
    m = load_model(robot, device)
    if own != "default":
        m.own_kernels = own
    return m


def fd_errors(X, case, idx=None):
    """(row, joint, resid) of the accelerations X [N, n] against the truth rows idx [N] (None: the 256 rows in order)."""
    X = np.asarray(X, np.float64)
    T, H, nle, f = case["qdd64"], case["H64"], case["nle64"], case["f64"]
    idx = np.arange(X.shape[0]) % ROWS if idx is None else idx
    assert X.shape == (len(idx), T.shape[1])
    row = resid = 0.0
    joint_num = np.zeros(T.shape[1])
    row_scale = np.abs(T).max(axis=1)
    for lo in range(0, len(idx), 16384):
        k, x = idx[lo:lo + 16384], X[lo:lo + 16384]
        d = np.abs(x - T[k])
        row = max(row, float((d.max(axis=1) / row_scale[k]).max()))
        joint_num = np.maximum(joint_num, d.max(axis=0))
        r = np.abs(np.einsum("bij,bj->bi", H[k], x) + nle[k] - f[k]).max(axis=1)
        scale = np.einsum("bij,bj->bi", np.abs(H[k]), np.abs(x)).max(axis=1) + np.abs(f[k]).max(axis=1) + np.abs(nle[k]).max(axis=1)
        resid = max(resid, float((r / scale).max()))
    return dict(row=row, joint=float((joint_num / np.abs(T).max(axis=0)).max()), resid=resid)


def h_error(Hx, H64, idx=None):
    """max_bij |dH_ij| / sqrt(H64_ii H64_jj)"""
    idx = np.arange(Hx.shape[0]) % ROWS if idx is None else idx
    dg = np.sqrt(np.einsum("bii->bi", H64))
    scale = dg[:, :, None] * dg[:, None, :]
    worst = 0.0
    for lo in range(0, len(idx), 16384):
        k = idx[lo:lo + 16384]
        worst = max(worst, float((np.abs(np.asarray(Hx[lo:lo + 16384], np.float64) - H64[k]) / scale[k]).max()))
    return worst


def ltdl_solve_numpy(H, b):
    """x [B, n] with H x = b in the dtype of H: the elimination H = L^T D L from the LAST joint towards the first and the three solves
    (the order of csrc/drm_sample.hpp ltdl_solve and of the reference's leaf-to-root recursion), restated in numpy.  The third yardstick
    of forward dynamics, see the module docstring."""
    H, b = H.copy(), b.copy()
    n = b.shape[1]
    for k in range(n - 1, -1, -1):
        for i in range(k):
            a = H[:, k, i] / H[:, k, k]
            H[:, i, :i + 1] -= H[:, k, i, None] * np.concatenate([H[:, k, :i] / H[:, k, k, None], a[:, None]], axis=1)
        H[:, k, :k] /= H[:, k, k, None]                    # row k now holds L[k][:k], its diagonal D_k
    for i in range(n - 1, -1, -1):                         # y = L^-T b
        b[:, :i] -= H[:, i, :i] * b[:, i, None]
    for i in range(n):                                     # z = D^-1 y, x = L^-1 z
        b[:, i] = b[:, i] / H[:, i, i] - (H[:, i, :i] * b[:, :i]).sum(axis=1)
    return b


def build_truth(spec, q, qd, qdd):
    orc = Oracle(spec)
    n = q.shape[1]
    q64, qd64, qdd64s, z = q.astype(np.float64), qd.astype(np.float64), qdd.astype(np.float64), np.zeros(q.shape)
    z32 = z.astype(np.float32)
    H64 = orc.mass_matrix(q64, False, False, np.float64)
    assert (np.einsum("bii->bi", H64) > 0).all()
    H32 = orc.mass_matrix(q, False, False, np.float32)
    assert H32.dtype == np.float32
    t = dict(q=q, qd=qd, H64=H64, yard_H=h_error(H32, H64), cases={})
    rand = np.random.default_rng(3).uniform(-1, 1, (q.shape[0], n)).astype(np.float32)
    for tset, g, d in CASES:
        f = rand if tset == "rand" else orc.rnea(q64, qd64, qdd64s, g, d, np.float64).astype(np.float32)
        f64 = f.astype(np.float64)
        want = orc.forward_dynamics(q64, qd64, f64, g, d, np.float64)
        nle64 = orc.rnea(q64, qd64, z, g, d, np.float64)
        # the truth itself, before anything under test
        pin = np.abs(np.linalg.solve(H64, (f64 - nle64)[:, :, None])[:, :, 0] - want).max(axis=1) / np.abs(want).max(axis=1)
        assert pin.max() <= 1e-10, (tset, g, d, pin.max())
        assert (np.abs(want).max(axis=1) > 0).all() and (np.abs(want).max(axis=0) > 0).all()
        case = dict(f=f, f64=f64, qdd64=want, nle64=nle64, H64=H64)
        aba32 = orc.forward_dynamics(q, qd, f, g, d, np.float32)
        rhs32 = f - orc.rnea(q, qd, z32, g, d, np.float32)
        solve32 = np.linalg.solve(H32, rhs32[:, :, None])[:, :, 0]
        ltdl32 = ltdl_solve_numpy(H32, rhs32)
        assert aba32.dtype == np.float32 and solve32.dtype == np.float32 and ltdl32.dtype == np.float32
        # the restated elimination is the truth when it runs in fp64
        pin = fd_errors(ltdl_solve_numpy(H64, f64 - nle64), case)
        assert max(pin["row"], pin["joint"]) <= 1e-8, (tset, g, d, pin)
        each = [fd_errors(x, case) for x in (aba32, solve32, ltdl32)]
        case["yard"] = {k: max(e[k] for e in each) for k in each[0]}
        case["yard_aba_lu"] = {k: max(e[k] for e in each[:2]) for k in each[0]}     # (what the inputs of a solve are held to)
        t["cases"][(tset, g, d)] = case
    return t


@functools.lru_cache(maxsize=None)
def truth(robot, seed):
    m = model_on(robot)
    return build_truth(m._spec, *sample_states(m, ROWS, seed=seed))


@functools.lru_cache(maxsize=None)
def truth_large_angle(robot):
    """seed 61 with one joint of rows 2 and 77 at +-4.0e5 (the float32 value is what the truth sees)"""
    m = model_on(robot)
    q, qd, qdd = sample_states(m, ROWS, seed=61)
    q = q.copy()
    q[2, min(5, q.shape[1] - 1)] = BIG_ANGLE
    q[77, 0] = -BIG_ANGLE
    return build_truth(m._spec, q, qd, qdd)


# ------------------------------------------------------------------------------------------------------------------- checks
def line(robot, path, flags, tset, metric, e, ey):
    print("FDCRBA %-20s %-24s %s %-4s %-5s %.3e %.3e %.2f" % (robot, path, flags, tset, metric, e, ey, e / ey))


def check_fd(robot, path, t, case, X, idx=None, yard="yard"):
    tset, g, d = case
    c = t["cases"][case]
    X = np.asarray(X.detach().cpu() if isinstance(X, torch.Tensor) else X)
    assert X.dtype in (np.float32, np.float64) and np.isfinite(X).all()
    e, failures = fd_errors(X, c, idx), []
    for metric in ("row", "joint", "resid"):
        ey = max(c[yard][metric], FLOOR)
        line(robot, path, "g%dd%d" % (g, d), tset, metric, e[metric], ey)
        if not e[metric] <= MARGIN * ey:
            failures.append((metric, e[metric], ey))
    assert not failures, (robot, path, case, failures)


def check_H(robot, path, t, H, idx=None, spectrum=None):
    """`spectrum`: the rows whose eigenvalues are taken (None: all) — a launch of the 256 rows repeated names the first repetition here
    and asserts itself that the others carry its bits."""
    if isinstance(H, torch.Tensor):
        assert torch.equal(H, H.transpose(1, 2)), "both triangles carry the same bits"
        H = H.detach().cpu().numpy()
    else:
        assert np.array_equal(H, H.transpose(0, 2, 1))
    assert H.dtype == np.float32 and np.isfinite(H).all()
    e, ey = h_error(H, t["H64"], idx), max(t["yard_H"], FLOOR)
    line(robot, path, "----", "-", "H", e, ey)
    assert e <= MARGIN * ey, (robot, path, e, ey)
    low = float(np.linalg.eigvalsh((H if spectrum is None else H[spectrum]).astype(np.float64)).min())
    assert low > 0, (robot, path, low)


def same_bits(a, b, expect, what):
    """Two rungs with different arithmetic must differ somewhere, two launches of one kernel must not."""
    equal = bool(torch.equal(a, b)) if isinstance(a, torch.Tensor) else bool(np.array_equal(a, b))
    print("FDCRBA-BITS %-60s %s" % (what, "equal" if equal else "differ"))
    assert equal == expect, what


# ------------------------------------------------------------------------------------------------------------------- runners
def dev(x, device):
    return torch.from_numpy(np.array(x, copy=True)).to(device)       # (a copy: the truth is shared and stays as it is)


def api_fd(model, t, case, B=None):
    """compute_forward_dynamics over the 256 rows in consecutive launches of B rows (None: one launch); q, qd, f stay as they were"""
    _, g, d = case
    q, qd, f = (dev(x, model._device) for x in (t["q"], t["qd"], t["cases"][case]["f"]))
    keep = [x.clone() for x in (q, qd, f)]
    B = B or ROWS
    out = torch.cat([model.compute_forward_dynamics(q[i:i + B], qd[i:i + B], f[i:i + B], include_gravity=bool(g), use_damping=bool(d))
                     for i in range(0, ROWS, B)])
    assert all(torch.equal(a, b) for a, b in zip(keep, (q, qd, f))), "the caller's tensors are not modified"
    assert out.shape == q.shape and out.dtype == torch.float32 and out.grad_fn is None
    return out


def api_H(model, t, B=None):
    q = dev(t["q"], model._device)
    keep = q.clone()
    B = B or ROWS
    out = torch.cat([model.compute_lagrangian_inertia_matrix(q[i:i + B]) for i in range(0, ROWS, B)])
    assert torch.equal(keep, q)
    return out


def api_everything(model, robot, path, seed, B=None, path_H=None):
    """all six forward-dynamics cases and H of one seed through the public API; the outputs by case (H under "H")"""
    t, outs = truth(robot, seed), {}
    for case in CASES:
        outs[case] = api_fd(model, t, case, B)
        check_fd(robot, path, t, case, outs[case])
    outs["H"] = api_H(model, t, B)
    check_H(robot, path_H or path, t, outs["H"])
    return outs


def walk_of(model, clear_shape=0):
    """A private copy of the dynamics walk's struct, shape bits switched off on request (the cached struct stays)."""
    from differentiable_robot_model_amd import backend
    dw = model._dynamics_walk()
    walk = backend._walk_struct_build(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs)
    if clear_shape:
        walk.shape = walk.shape & ~clear_shape & 0xffffff           # (the top byte carries the (P, K, L) of the bit that goes)
    return walk


def library_and_stream(device):
    from differentiable_robot_model_amd import backend
    d = torch.device(device)
    return backend.library_for(d), backend._stream(d)


def abi_fd(walk, q, qd, f, flags, out=None):
    """drm_forward_dynamics on the tensors as they are (views included); the scratch sized for any pointers"""
    from differentiable_robot_model_amd import backend
    lib, stream = library_and_stream(q.device)
    B, n = q.shape
    need = int(lib.drm_forward_dynamics_scratch_floats(ctypes.byref(walk), B))
    scratch = torch.empty(max(need, 4), device=q.device)
    out = torch.full((B, n), float("nan"), device=q.device) if out is None else out
    backend._check(lib.drm_forward_dynamics(ctypes.byref(walk), q.data_ptr(), qd.data_ptr(), f.data_ptr(), B, flags, out.data_ptr(),
                                            scratch.data_ptr(), stream), lib)
    return out


def abi_H(walk, q, out=None):
    from differentiable_robot_model_amd import backend
    lib, stream = library_and_stream(q.device)
    B, n = q.shape
    need = int(lib.drm_crba_scratch_floats(ctypes.byref(walk), B))
    scratch = torch.empty(max(need, 4), device=q.device)
    out = torch.full((B, n, n), float("nan"), device=q.device) if out is None else out
    backend._check(lib.drm_crba(ctypes.byref(walk), q.data_ptr(), B, out.data_ptr(), scratch.data_ptr(), stream), lib)
    return out


def abi_everything(walk, device, robot, path, seed, B=None, t=None, cases=CASES):
    """the same through the C ABI, in consecutive launches of B rows (None: one launch) on 16-byte aligned copies of the slices"""
    t, outs = t or truth(robot, seed), {}
    q, qd = dev(t["q"], device), dev(t["qd"], device)
    B = B or ROWS
    for case in cases:
        f = dev(t["cases"][case]["f"], device)
        outs[case] = torch.cat([abi_fd(walk, q[i:i + B].clone(), qd[i:i + B].clone(), f[i:i + B].clone(), case[1] | (case[2] << 1))
                                for i in range(0, ROWS, B)])
        check_fd(robot, path, t, case, outs[case])
    outs["H"] = torch.cat([abi_H(walk, q[i:i + B].clone()) for i in range(0, ROWS, B)])
    check_H(robot, path, t, outs["H"])
    return outs


def abi_edges(walk, device, robot, path, B):
    """zero input and the |q| = 4.0e5 rows through the C ABI"""
    q = dev(truth(robot, 61)["q"][:B], device)
    z = torch.zeros_like(q)
    for flags in (0, 2):
        assert (abi_fd(walk, q, z, z.clone(), flags) == 0).all(), "f = 0, qd = 0, no gravity: nothing accelerates"
    abi_everything(walk, device, robot, path + "-4e5", 61, B, t=truth_large_angle(robot), cases=LARGE_ANGLE_CASES)


def emu_everything(emu, walk, robot, path, seed, fd="emu_forward_dynamics", crba="emu_crba", t=None, cases=CASES):
    t = t or truth(robot, seed)
    q, qd = np.ascontiguousarray(t["q"]), np.ascontiguousarray(t["qd"])
    B, n = q.shape
    if fd:
        for case in cases:
            f, out = np.ascontiguousarray(t["cases"][case]["f"]), np.full((B, n), np.nan, np.float32)
            assert getattr(emu, fd)(ctypes.byref(walk), _ptr(q), _ptr(qd), _ptr(f), ctypes.c_int64(B), case[1] | (case[2] << 1), _ptr(out)) == 0
            check_fd(robot, path, t, case, out)
    if crba:
        H = np.full((B, n, n), np.nan, np.float32)
        assert getattr(emu, crba)(ctypes.byref(walk), _ptr(q), ctypes.c_int64(B), _ptr(H)) == 0
        check_H(robot, path, t, H)


def emu_edges(emu, walk, robot, path, fd="emu_forward_dynamics", crba="emu_crba"):
    """zero input and the |q| = 4.0e5 rows on an emulated path"""
    if fd:
        q = np.ascontiguousarray(truth(robot, 61)["q"])
        z = np.zeros_like(q)
        for flags in (0, 2):
            out = np.full(q.shape, np.nan, np.float32)
            assert getattr(emu, fd)(ctypes.byref(walk), _ptr(q), _ptr(z), _ptr(z), ctypes.c_int64(len(q)), flags, _ptr(out)) == 0
            assert (out == 0).all(), "f = 0, qd = 0, no gravity: nothing accelerates"
    emu_everything(emu, walk, robot, path + "-4e5", 61, fd, crba, t=truth_large_angle(robot), cases=LARGE_ANGLE_CASES)


# ------------------------------------------------------------------------------------------------------------------- edges (any device)
def zero_input_check(model, B):
    n, device = model._n_dofs, model._device
    q = dev(sample_states(model, B, seed=61)[0], device)
    z = torch.zeros(B, n, device=device)
    for damp in (False, True):
        out = model.compute_forward_dynamics(q, z, z.clone(), include_gravity=False, use_damping=damp)
        assert (out == 0).all(), "f = 0, qd = 0, no gravity: nothing accelerates"


def outputs_where_given_check(model, robot, B):
    """through the C ABI: outputs pre-filled with NaN in an allocation one row longer than the launch"""
    t = truth(robot, 61)
    device, n = model._device, model._n_dofs
    walk = walk_of(model)
    q, qd, f = (dev(x[:B], device) for x in (t["q"], t["qd"], t["cases"][("rand", 1, 1)]["f"]))
    keep = [x.clone() for x in (q, qd, f)]
    qdd = torch.full((B + 1, n), float("nan"), device=device)
    qdd[B] = -7.25
    abi_fd(walk, q, qd, f, 3, out=qdd[:B])
    H = torch.full((B + 1, n, n), float("nan"), device=device)
    H[B] = -7.25
    abi_H(walk, q, out=H[:B])
    assert not torch.isnan(qdd[:B]).any() and (qdd[B] == -7.25).all()
    assert not torch.isnan(H[:B]).any() and (H[B] == -7.25).all()
    assert all(torch.equal(a, b) for a, b in zip(keep, (q, qd, f)))
    # ... and they are what the public API returns
    assert torch.equal(qdd[:B], model.compute_forward_dynamics(q, qd, f, include_gravity=True, use_damping=True))
    assert torch.equal(H[:B], model.compute_lagrangian_inertia_matrix(q))


def large_angle_check(model, robot, path, B=None):
    t = truth_large_angle(robot)
    for case in LARGE_ANGLE_CASES:
        check_fd(robot, path, t, case, api_fd(model, t, case, B))
    check_H(robot, path, t, api_H(model, t, B))


def non_finite_rows_check(model, robot):
    """an all-NaN q row and an all-Inf f row: non-finite in every entry, no bit of another row changes; both in full tiles (128 rows)
    and both in the ragged tail (127 rows: its second tile has 63)"""
    t = truth(robot, 61)
    device = model._device
    for B, (r_nan, r_inf) in ((128, (5, 70)), (127, (70, 100))):
        q, qd, f = (dev(x[:B], device) for x in (t["q"], t["qd"], t["cases"][("rand", 1, 1)]["f"]))
        run = lambda: (model.compute_forward_dynamics(q, qd, f, include_gravity=True, use_damping=True), model.compute_lagrangian_inertia_matrix(q))
        clean = run()
        q[r_nan] = float("nan")
        f[r_inf] = float("inf")
        got = run()
        others = torch.ones(B, dtype=torch.bool, device=device)
        others[[r_nan, r_inf]] = False
        for a, b in zip(got, clean):
            assert torch.equal(a[others], b[others]) and torch.isfinite(a[others]).all(), (robot, B)
        assert not torch.isfinite(got[0][r_nan]).any() and not torch.isfinite(got[0][r_inf]).any(), (robot, B)
        # (H of joints on different branches is a structural zero, and a leaf's own diagonal entry does not see its angle)
        assert not torch.isfinite(got[1][r_nan]).all() and torch.equal(got[1][r_inf], clean[1][r_inf]), (robot, B)


def interface_check(model, robot, B):
    """H ignores its flags; 1-D arguments; a column-slice q; compute_forward_dynamics_old"""
    t = truth(robot, 61)
    device, n = model._device, model._n_dofs
    q, qd, f = (dev(x[:B], device) for x in (t["q"], t["qd"], t["cases"][("rand", 1, 1)]["f"]))
    H = model.compute_lagrangian_inertia_matrix(q)
    for g, d in FLAGS:
        assert torch.equal(H, model.compute_lagrangian_inertia_matrix(q, include_gravity=bool(g), use_damping=bool(d))), (g, d)
    acc = {(g, d): model.compute_forward_dynamics(q, qd, f, include_gravity=bool(g), use_damping=bool(d)) for g, d in FLAGS}
    assert torch.equal(model.compute_forward_dynamics_old(q, qd, f), acc[(1, 1)])
    assert torch.equal(model.compute_forward_dynamics(q, qd, f), acc[(1, 0)]), "use_damping defaults to False"
    # unbatched: the rows of one-row launches (the loop kernel); the batched call of the same single row gives the same bits
    for r in (0, B - 1):
        one = model.compute_forward_dynamics(q[r], qd[r], f[r], include_gravity=True, use_damping=True)
        assert one.shape == (n,) and torch.equal(one, model.compute_forward_dynamics(q[r:r + 1].clone(), qd[r:r + 1].clone(), f[r:r + 1].clone(), True, True)[0])
        H1 = model.compute_lagrangian_inertia_matrix(q[r])
        assert H1.shape == (n, n) and torch.equal(H1, model.compute_lagrangian_inertia_matrix(q[r:r + 1].clone())[0])
    # a column slice of a wider tensor
    wide = torch.full((B, n + 3), 9.5, device=device)
    wide[:, 2:2 + n] = q
    qs = wide[:, 2:2 + n]
    assert not qs.is_contiguous()
    assert torch.equal(model.compute_forward_dynamics(qs, qd, f, include_gravity=True, use_damping=True), acc[(1, 1)])
    assert torch.equal(model.compute_lagrangian_inertia_matrix(qs), H)
    assert (wide[:, :2] == 9.5).all() and (wide[:, 2 + n:] == 9.5).all() and torch.equal(wide[:, 2:2 + n], q)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_host_build_against_truth(cpu_library, robot, seed):
    api_everything(model_on(robot), robot, "host", seed)


@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_host_build_edges(cpu_library, robot):
    m = model_on(robot)
    zero_input_check(m, 65)
    outputs_where_given_check(m, robot, 65)
    interface_check(m, robot, 65)
    non_finite_rows_check(m, robot)
    large_angle_check(m, robot, "host-4e5")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_emu_loop_walks_against_truth(emu, robot, seed):
    """emu_forward_dynamics / emu_crba (csrc/drm_host_loops.hpp: the arithmetic of the loop kernels) on the whole-tree walk and on the
    folded walk the API launches"""
    m = model_on(robot)
    prog, fprog = build_walk(m._spec, whole_tree=True), build_walk(m._spec, whole_tree=True, drop_folded=True)   # (own the tables)
    walk, keep = host_walk(m, prog)
    emu_everything(emu, walk, robot, "emu-tree", seed)
    fwalk, fkeep = folded_host_walk(m, fprog)
    emu_everything(emu, fwalk, robot, "emu-folded", seed)
    if seed == SEEDS[0]:
        emu_edges(emu, walk, robot, "emu-tree")
        emu_edges(emu, fwalk, robot, "emu-folded")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ARM_HAND_ROBOTS)
def test_emu_arm_hand_against_truth(emu, robot, seed):
    """aba_arm_hand / crba_arm_hand: the arithmetic of the arm-with-hand straight-line kernels"""
    m, prog, walk, keep = arm_hand_case(robot)
    assert prog.shape & SHAPE_ARM_HAND
    emu_everything(emu, walk, robot, "emu-arm-hand", seed, fd="emu_forward_dynamics_arm_hand", crba="emu_crba_arm_hand")
    if seed == SEEDS[0]:
        emu_edges(emu, walk, robot, "emu-arm-hand", fd="emu_forward_dynamics_arm_hand", crba="emu_crba_arm_hand")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ARM_ROBOTS)
def test_emu_crba_arm_against_truth(emu, robot, seed):
    """crba_chain<8, 7>: the arithmetic of crba_arm_kernel"""
    m = model_on(robot)
    prog = build_walk(m._spec, whole_tree=True)                      # (owns the tables)
    walk, keep = host_walk(m, prog)
    emu_everything(emu, walk, robot, "emu-crba-arm", seed, fd=None, crba="emu_crba_arm")
    if seed == SEEDS[0]:
        emu_edges(emu, walk, robot, "emu-crba-arm", fd=None, crba="emu_crba_arm")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("robot", ARM_ROBOTS)
def test_emu_arm_forward_dynamics_against_truth(emu, robot, seed):
    """fd_arm_8_7 (tests/host_emu/host_emu.cpp): the arithmetic of forward_dynamics_arm_kernel<8, 7, LINKS> — rnea_chain_trig, crba_chain_trig
    and the unrolled L^T D L solve — on the folded walk (LINKS = 7, what the API launches) and on the whole table (LINKS = 8)"""
    m = model_on(robot)
    fprog, prog = build_walk(m._spec, whole_tree=True, drop_folded=True), build_walk(m._spec, whole_tree=True)      # (own the tables)
    assert (fprog.n_ops, prog.n_ops) == (7, 8)
    fwalk, fkeep = folded_host_walk(m, fprog)
    emu_everything(emu, fwalk, robot, "emu-fd-arm<8,7,7>", seed, fd="emu_forward_dynamics_arm", crba=None)
    walk, keep = host_walk(m, prog)
    emu_everything(emu, walk, robot, "emu-fd-arm<8,7,8>", seed, fd="emu_forward_dynamics_arm", crba=None)
    if seed == SEEDS[0]:
        emu_edges(emu, fwalk, robot, "emu-fd-arm<8,7,7>", fd="emu_forward_dynamics_arm", crba=None)
        emu_edges(emu, walk, robot, "emu-fd-arm<8,7,8>", fd="emu_forward_dynamics_arm", crba=None)
    # what the third yardstick rests on: the INPUTS of the kernel's solve — the emulated float32 H (crba_chain) and bias torques
    # (rnea_chain, qdd = NULL) — solved in fp64 meet the requirement against the first two yardsticks alone, so whatever the arm
    # kernel loses beyond them it loses in the elimination, and a solve that lost more than the restated elimination would still fail
    t = truth(robot, seed)
    q, qd = np.ascontiguousarray(t["q"]), np.ascontiguousarray(t["qd"])
    H = np.full((ROWS, 7, 7), np.nan, np.float32)
    assert emu.emu_crba_arm(ctypes.byref(walk), _ptr(q), ctypes.c_int64(ROWS), _ptr(H)) == 0
    for case in CASES:
        nle = np.full((ROWS, 7), np.nan, np.float32)
        assert emu.emu_rnea_arm(ctypes.byref(walk), _ptr(q), _ptr(qd), None, ctypes.c_int64(ROWS), case[1] | (case[2] << 1), _ptr(nle)) == 0
        x = np.linalg.solve(H.astype(np.float64), (t["cases"][case]["f64"] - nle.astype(np.float64))[:, :, None])[:, :, 0]
        check_fd(robot, "emu-arm-inputs-fp64-solve", t, case, x, yard="yard_aba_lu")


def test_static_source_of_fetch_against_truth(cpu_library, tmp_path):
    """static_fd / static_crba: Fetch's generated straight-line source (csrc/drm_static.hpp) compiled for the host"""
    from differentiable_robot_model_amd import backend
    from test_specialize import host_harness
    robot = "fetch"
    m = model_on(robot)
    dw = m._dynamics_walk()
    prog, n = dw.program, m._n_dofs
    st = host_harness(tmp_path, sp.walk_tree(prog), n)
    assert st.static_n_ops() == prog.n_ops
    ops_f = m._ops_f(dw).detach().contiguous()
    of = ctypes.c_void_p(ops_f.data_ptr())
    for seed in SEEDS:
        t = truth(robot, seed)
        q, qd = np.ascontiguousarray(t["q"]), np.ascontiguousarray(t["qd"])
        cb = ctypes.c_int64(ROWS)
        for case in CASES:
            f, out = np.ascontiguousarray(t["cases"][case]["f"]), np.full((ROWS, n), np.nan, np.float32)
            assert st.static_fd(of, _ptr(q), _ptr(qd), _ptr(f), cb, case[1] | (case[2] << 1), _ptr(out)) == 0
            check_fd(robot, "static-source", t, case, out)
        H = np.full((ROWS, n, n), np.nan, np.float32)
        assert st.static_crba(of, _ptr(q), cb, _ptr(H)) == 0
        check_H(robot, "static-source", t, H)
    tl = truth_large_angle(robot)
    q, qd, z = np.ascontiguousarray(tl["q"]), np.ascontiguousarray(tl["qd"]), np.zeros((ROWS, n), np.float32)
    for flags in (0, 2):
        out = np.full((ROWS, n), np.nan, np.float32)
        assert st.static_fd(of, _ptr(q), _ptr(z), _ptr(z), cb, flags, _ptr(out)) == 0 and (out == 0).all()
    for case in LARGE_ANGLE_CASES:
        f, out = np.ascontiguousarray(tl["cases"][case]["f"]), np.full((ROWS, n), np.nan, np.float32)
        assert st.static_fd(of, _ptr(q), _ptr(qd), _ptr(f), cb, case[1] | (case[2] << 1), _ptr(out)) == 0
        check_fd(robot, "static-source-4e5", tl, case, out)
    H = np.full((ROWS, n, n), np.nan, np.float32)
    assert st.static_crba(of, _ptr(q), cb, _ptr(H)) == 0
    check_H(robot, "static-source-4e5", tl, H)


# ------------------------------------------------------------------------------------------------------------------- GPU
def gpu_model(robot, own="off"):
    return model_on(robot, "cuda:0", own)


def specialized(robot):
    """the model with its own kernels attached (built with hipcc where they are not shipped)"""
    m = model_on(robot, "cuda:0", "default")
    m.specialize()
    return m, (getattr(m._dynamics_walk().program, "_special", None) or {})


def rung_name(model, robot, B, what):
    """the rung(s) a launch of B aligned rows takes with the library's kernels (module docstring)"""
    fast = RUNGS.get(robot)
    if fast == "arm":
        fast = "arm<8,7,%d>" % model._dynamics_walk().program.n_ops
    if what == "H" and fast == "fingers":
        fast = None                                  # (below DRM_CRBA_TREE_MIN_TILES tiles a hand's H is the tree kernel's)
    if fast is None or B < 64:
        return "loop-B%d" % B
    return ("%s-B%d" % (fast, B)) if B % 64 == 0 else ("%s+tail-B%d" % (fast, B))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 131, 256])
@pytest.mark.parametrize("robot", RUNG_ROBOTS)
def test_gpu_library_rungs_against_truth(robot, B):
    """own_kernels = "off": full tiles through the shape's kernel (the shape bit of the walk; every pointer of the public API is 16-byte
    aligned), the rest of the launch through the loop kernels"""
    m = gpu_model(robot)
    prog = m._dynamics_walk().program
    own = walk_of(m).special
    assert not any(own[k] for k in (sp.SPECIAL_FD, sp.SPECIAL_CRBA, sp.SPECIAL_FD_ARM, sp.SPECIAL_CRBA_ARM, sp.SPECIAL_FD_ARM2)), "library kernels only"
    # (the two-link robot is a serial chain too, but arm7_walk wants 7 DoF in a table of 8 rows: it stays with the loop kernels)
    assert bool(prog.shape & SHAPE_ARM_CHAIN and m._n_dofs == 7) == (robot in ARM_ROBOTS) and bool(prog.shape & SHAPE_FINGERS) == (robot in FINGER_ROBOTS)
    assert bool(prog.shape & SHAPE_ARM_HAND) == (robot in ARM_HAND_ROBOTS)
    for seed in SEEDS:
        outs = api_everything(m, robot, rung_name(m, robot, B, "fd"), seed, B, path_H=rung_name(m, robot, B, "H"))
        full = B // 64 * 64
        if seed == 61 and full and B % 64:
            # rows of full tiles: the same bits with and without a tail behind them
            t = truth(robot, seed)
            q, qd, f = (dev(x[:full], "cuda:0") for x in (t["q"], t["qd"], t["cases"][("rand", 1, 1)]["f"]))
            same_bits(outs[("rand", 1, 1)][:full], m.compute_forward_dynamics(q, qd, f, True, True), True, "%s fd full tiles of B=%d alone" % (robot, B))
            same_bits(outs["H"][:full], m.compute_lagrangian_inertia_matrix(q), True, "%s H full tiles of B=%d alone" % (robot, B))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARM_ROBOTS + FINGER_ROBOTS + ARM_HAND_ROBOTS)
def test_gpu_loop_kernels_on_the_walks_of_the_fast_rungs(robot):
    """The walk with its shape bit cleared through the C ABI: every row through forward_dynamics_tree_kernel / crba_tree_kernel (hands) or
    the persistent kernels (arms, arms with hands).  Different arithmetic from the fast rung: not its bits; the kernel of the fast rung's
    ragged tail: its bits."""
    m = gpu_model(robot)
    walk = walk_of(m, clear_shape=SHAPE_ARM_CHAIN | SHAPE_FINGERS | SHAPE_ARM_HAND)
    loop = abi_everything(walk, "cuda:0", robot, "loop-abi-B256", 61)
    abi_edges(walk, "cuda:0", robot, "loop-abi", 256)
    fast = api_everything(m, robot, rung_name(m, robot, 256, "fd"), 61, path_H=rung_name(m, robot, 256, "H"))
    case = ("rand", 1, 1)
    same_bits(loop[case], fast[case], False, "%s fd loop kernel vs %s" % (robot, RUNGS[robot]))
    same_bits(loop["H"], fast["H"], robot in FINGER_ROBOTS, "%s H loop kernel vs %s" % (robot, RUNGS[robot]))
    # the ragged tail of a 65-row launch is row 64 through the loop kernel
    t = truth(robot, 61)
    q, qd, f = (dev(x[:65], "cuda:0") for x in (t["q"], t["qd"], t["cases"][case]["f"]))
    same_bits(m.compute_forward_dynamics(q, qd, f, True, True)[64:], loop[case][64:65], True, "%s fd tail row of B=65 vs loop kernel" % robot)
    same_bits(m.compute_lagrangian_inertia_matrix(q)[64:], loop["H"][64:65], True, "%s H tail row of B=65 vs loop kernel" % robot)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARM_ROBOTS)
def test_gpu_arm_kernels_on_the_unfolded_walk(robot):
    """forward_dynamics_arm_kernel<8, 7, 8> and crba_arm_kernel<8, 7, 8>: the arm's whole-tree walk with all 8 links as ops (the API launches
    the 7-op walk with the fixed tail folded) through the C ABI, as tests/test_gpu_parity.py sends it to drm_rnea — DRM_WALK_ARM_CHAIN,
    arm_links(w) == 8, full tiles, aligned pointers.  Full tiles alone and with a ragged tail; not the bits of the loop kernel on the
    same walk (its shape bit cleared), whose bits the tail row has.  (Against <8, 7, 7> nothing is asserted: where the fixed tail link has
    no mass the two instantiations give the same bits — panda_no_gripper's H, fetch_arm_no_gripper's accelerations.)"""
    from differentiable_robot_model_amd import backend
    m = gpu_model(robot)
    dt = m._get_walk(("tree",), whole_tree=True)
    assert dt.program.n_ops == 8 and dt.program.shape & SHAPE_ARM_CHAIN and m._dynamics_walk().program.n_ops == 7
    build = lambda: backend._walk_struct_build(dt.program, m._ops_f(dt).detach(), dt.ops_i, m._n_dofs)
    walk, loop_walk = build(), build()
    assert not any(walk.special[k] for k in (sp.SPECIAL_FD, sp.SPECIAL_CRBA, sp.SPECIAL_FD_ARM, sp.SPECIAL_CRBA_ARM, sp.SPECIAL_FD_ARM2))
    loop_walk.shape = loop_walk.shape & ~SHAPE_ARM_CHAIN & 0xffffff
    outs = {}
    for B in (64, 256, 65, 131):
        for seed in SEEDS:
            outs[B, seed] = abi_everything(walk, "cuda:0", robot, "arm<8,7,8>%s-B%d" % ("+tail" if B % 64 else "", B), seed, B)
    abi_edges(walk, "cuda:0", robot, "arm<8,7,8>", 256)
    abi_edges(walk, "cuda:0", robot, "arm<8,7,8>+tail", 65)
    loop = abi_everything(loop_walk, "cuda:0", robot, "loop-abi-unfolded-B256", 61)
    case = ("rand", 1, 1)
    for what, key in (("fd", case), ("H", "H")):
        same_bits(outs[256, 61][key], loop[key], False, "%s %s arm<8,7,8> vs loop kernel on the unfolded walk" % (robot, what))
        same_bits(outs[65, 61][key][:64], outs[256, 61][key][:64], True, "%s %s arm<8,7,8> full tile of B=65 alone" % (robot, what))
        same_bits(outs[65, 61][key][64:65], loop[key][64:65], True, "%s %s arm<8,7,8> tail row of B=65 vs loop kernel" % (robot, what))
    torch.cuda.synchronize()


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("robot", ["fetch", "panda_no_gripper", "iiwa7"])
def test_gpu_own_kernel_rungs_against_truth(robot):
    """model.specialize(): Fetch's drm_fd_static / drm_crba_static (special[DRM_SPECIAL_FD] / [DRM_SPECIAL_CRBA]) and the arms'
    drm_fd_arm_static / drm_crba_arm_static (special[DRM_SPECIAL_FD_ARM] / [DRM_SPECIAL_CRBA_ARM]) take the full tiles, the library's
    loop kernels the tail.  Constants folded into the instruction stream: not the bits of the library's rung."""
    m, special = specialized(robot)
    kinds = (sp.SPECIAL_FD, sp.SPECIAL_CRBA) if robot == "fetch" else (sp.SPECIAL_FD_ARM, sp.SPECIAL_CRBA_ARM)
    assert all(special.get(k) for k in kinds), "the walk carries its own kernels"
    name = "own" if robot == "fetch" else "arm-own"
    lib_model = gpu_model(robot)
    for B in (64, 65, 256):
        for seed in SEEDS:
            outs = api_everything(m, robot, "%s%s-B%d" % (name, "+tail" if B % 64 else "", B), seed, B)
        if B == 256:
            other = api_everything(lib_model, robot, rung_name(lib_model, robot, B, "fd"), SEEDS[-1], B, path_H=rung_name(lib_model, robot, B, "H"))
            same_bits(outs[("rand", 1, 1)], other[("rand", 1, 1)], False, "%s fd own kernel vs library" % robot)
            same_bits(outs["H"], other["H"], False, "%s H own kernel vs library" % robot)
    zero_input_check(m, 128)
    non_finite_rows_check(m, robot)
    large_angle_check(m, robot, name + "-4e5")
    torch.cuda.synchronize()


def tiled(t, case, N, device="cuda:0"):
    """the 256 rows repeated cyclically to N rows"""
    idx = np.arange(N) % ROWS
    return idx, tuple(dev(x[idx], device) for x in (t["q"], t["qd"], t["cases"][case]["f"]))


def tiled_edges(model, robot, path, N):
    """the exact conditions on a launch of N tiled rows: the |q| = 4.0e5 rows, zero input, a NaN row in the first tile and an Inf row in
    the ragged tail"""
    tl, case = truth_large_angle(robot), ("rand", 1, 1)
    idx, (q, qd, f) = tiled(tl, case, N)
    run = lambda: model.compute_forward_dynamics(q, qd, f, include_gravity=True, use_damping=True)
    clean = run()
    check_fd(robot, path + "-4e5", tl, case, clean, idx)
    z = torch.zeros_like(q)
    assert (model.compute_forward_dynamics(q, z, z.clone(), include_gravity=False, use_damping=False) == 0).all()
    r_nan, r_inf = 5, N - 2
    q[r_nan] = float("nan")
    f[r_inf] = float("inf")
    got = run()
    others = torch.ones(N, dtype=torch.bool, device=q.device)
    others[[r_nan, r_inf]] = False
    assert torch.equal(got[others], clean[others]) and torch.isfinite(got[others]).all()
    assert not torch.isfinite(got[r_nan]).any() and not torch.isfinite(got[r_inf]).any()


@pytest.mark.gpu
@needs_hipcc
def test_gpu_arm_two_samples_per_lane_rung():
    """drm_fd_arm2_static: special[DRM_SPECIAL_FD_ARM2] and at least DRM_ARM_STATIC_MIN_PAIRS (1 024) pairs of full tiles.  1 024 pairs + one odd
    tile (drm_fd_arm_static) + 3 rows (the loop kernel), every row against its truth row."""
    robot = "panda_no_gripper"
    m, special = specialized(robot)
    assert special.get(sp.SPECIAL_FD_ARM2) and special.get(sp.SPECIAL_FD_ARM)
    pairs = 2 * 64 * ARM_STATIC_MIN_PAIRS
    N = pairs + 64 + 3
    t = truth(robot, 61)
    for case in (("rand", 1, 1), ("rand", 0, 1), ("id", 0, 0)):
        idx, (q, qd, f) = tiled(t, case, N)
        out = m.compute_forward_dynamics(q, qd, f, include_gravity=bool(case[1]), use_damping=bool(case[2]))
        check_fd(robot, "arm2-own+odd+tail", t, case, out, idx)
        one = m.compute_forward_dynamics(q[:256], qd[:256], f[:256], include_gravity=bool(case[1]), use_damping=bool(case[2]))
        # the same truth rows through the two-samples-per-lane form and through the one-sample form of a small launch
        same_bits(out[:256], one, False, "panda_no_gripper fd %s two samples per lane vs one" % (case,))
        same_bits(out[pairs:pairs + 64], one[:64], True, "panda_no_gripper fd %s the odd tile is the one-sample kernel's" % (case,))
        same_bits(out[256:512], out[:256], True, "panda_no_gripper fd %s the same rows in another pair of tiles" % (case,))
    tiled_edges(m, robot, "arm2-own+odd+tail", N)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_persistent_grids_with_more_tiles_than_blocks():
    """Fetch with own_kernels = "off" (no shape bit, a 14-op walk): forward_dynamics_aba_kernel and crba_rows_kernel on 2 049 full tiles
    + 3 rows, more tiles than the device holds blocks, so blocks walk a second tile.  Every row against its truth row; rows share nothing,
    so every repetition of the 256 rows carries the bits of the first."""
    robot = "fetch"
    m = gpu_model(robot)
    N = 2049 * 64 + 3
    t = truth(robot, 61)
    for case in (("rand", 1, 1), ("id", 0, 0)):
        idx, (q, qd, f) = tiled(t, case, N)
        out = m.compute_forward_dynamics(q, qd, f, include_gravity=bool(case[1]), use_damping=bool(case[2]))
        check_fd(robot, "loop-persistent", t, case, out, idx)
        reps = N // ROWS
        assert torch.equal(out[:reps * ROWS].view(reps, ROWS, -1), out[:ROWS].expand(reps, -1, -1)) and torch.equal(out[reps * ROWS:], out[:N - reps * ROWS])
    idx, (q, _, _) = tiled(t, ("rand", 1, 1), N)
    H = m.compute_lagrangian_inertia_matrix(q)
    reps = N // ROWS
    n = m._n_dofs
    assert torch.equal(H[:reps * ROWS].view(reps, ROWS, n, n), H[:ROWS].expand(reps, -1, -1, -1)) and torch.equal(H[reps * ROWS:], H[:N - reps * ROWS])
    check_H(robot, "loop-persistent", t, H, idx, spectrum=slice(0, ROWS))
    tiled_edges(m, robot, "loop-persistent", N)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "panda"])
def test_gpu_misaligned_call_beyond_the_capped_grid(robot):
    """A [1:] view of 65 * 64 + 1 rows through the C ABI: q, qd, f and the outputs start 4 n bytes off a 16-byte boundary (n = 7, 9), so
    the straight-line kernels of these walks do not apply and the persistent loop kernels run all 65 tiles on a grid capped at
    MISALIGNED_TILES = 64 blocks: block 0 walks a second tile.  The bits of the loop kernel on the aligned rows."""
    m = gpu_model(robot)
    n = m._n_dofs
    N = 65 * 64 + 1
    t = truth(robot, 61)
    walk = walk_of(m)
    assert walk.shape & (SHAPE_ARM_CHAIN | SHAPE_ARM_HAND)
    loop_walk = walk_of(m, clear_shape=SHAPE_ARM_CHAIN | SHAPE_ARM_HAND)
    idx = (np.arange(N) % ROWS)[1:]
    for case in (("rand", 1, 1), ("id", 0, 0)):
        _, (q, qd, f) = tiled(t, case, N)
        out = torch.full((N, n), float("nan"), device="cuda:0")
        views = [x[1:] for x in (q, qd, f, out)]
        assert all(v.data_ptr() % 16 for v in views)
        abi_fd(walk, views[0], views[1], views[2], case[1] | (case[2] << 1), out=views[3])
        assert torch.isnan(out[0]).all(), "the row in front of the view is not written"
        check_fd(robot, "loop-misaligned", t, case, out[1:], idx)
        aligned = abi_fd(loop_walk, q[1:257].clone(), qd[1:257].clone(), f[1:257].clone(), case[1] | (case[2] << 1))
        same_bits(out[1:257], aligned, True, "%s fd %s misaligned call vs the loop kernel on aligned rows" % (robot, case))
    _, (q, _, _) = tiled(t, ("rand", 1, 1), N)
    H = torch.full((N, n, n), float("nan"), device="cuda:0")
    assert H[1:].data_ptr() % 16
    abi_H(walk, q[1:], out=H[1:])
    assert torch.isnan(H[0]).all()
    reps = (N - 1) // ROWS
    assert torch.equal(H[1:1 + reps * ROWS].view(reps, ROWS, n, n), H[1:1 + ROWS].expand(reps, -1, -1, -1))
    check_H(robot, "loop-misaligned", t, H[1:], idx, spectrum=slice(0, ROWS))
    same_bits(H[1:257], abi_H(loop_walk, q[1:257].clone()), True, "%s H misaligned call vs the loop kernel on aligned rows" % robot)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_crba_fingers_tree_rung():
    """launch_crba_fingers_tree: DRM_WALK_FINGERS, K L <= 12 ops and at least DRM_CRBA_TREE_MIN_TILES (2 048) full tiles — trifinger_edu at
    2 048 * 64 + 70 rows: 2 049 tiles through the one-wavefront-per-tile walk, 6 rows through crba_tree_kernel.  Every row against its
    truth row; the other arithmetic than the small launch's (tests/test_mass_matrix.py holds the two to 2e-5 of each other)."""
    robot = "trifinger_edu"
    m = gpu_model(robot)
    N = 2048 * 64 + 70
    for seed in SEEDS:
        t = truth(robot, seed)
        idx, (q, _, _) = tiled(t, ("rand", 1, 1), N)
        H = m.compute_lagrangian_inertia_matrix(q)
        reps, n = (N - 6) // ROWS, m._n_dofs
        assert torch.equal(H[:reps * ROWS].view(reps, ROWS, n, n), H[:ROWS].expand(reps, -1, -1, -1))
        check_H(robot, "fingers-tree+tail", t, H, idx, spectrum=np.r_[0:ROWS, N - 6:N])
        small = m.compute_lagrangian_inertia_matrix(q[:ROWS])
        same_bits(H[N - 6:], small[(N - 6) % ROWS:(N - 6) % ROWS + 6], True, "trifinger_edu H seed %d tail rows are the tree kernel's" % seed)
    tl = truth_large_angle(robot)
    idx, (q, _, _) = tiled(tl, ("rand", 1, 1), N)
    check_H(robot, "fingers-tree+tail-4e5", tl, m.compute_lagrangian_inertia_matrix(q), idx, spectrum=np.r_[0:ROWS, N - 6:N])
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_gpu_edges(robot):
    """the exact conditions on the library's rungs: 128 rows (full tiles) and 65 / 127 rows (a ragged tail)"""
    m = gpu_model(robot)
    for B in (128, 65):
        zero_input_check(m, B)
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

"""Forward-dynamics derivatives in one call (csrc/drm_fdd.hip, include/drm_hip.h drm_forward_dynamics_derivatives;
DifferentiableRobotModel.compute_forward_dynamics_derivatives): qdd = H^-1 (f - nle), dqdd_dq = -H^-1 dID/dq at (q, qd, qdd),
dqdd_dqd = -H^-1 dID/dqd, minv = H^-1.

INPUTS: tests/golden/golden_fd_derivatives.npz (make_golden_fd_derivatives.py), 128 rows per robot: q within the joint limits,
qd ~ U(-1, 1), f = the reference's inverse dynamics of qdd ~ U(-2, 2).

TRUTH, computed here: the fp64 central difference, h = 1e-5, of Oracle.forward_dynamics(dtype=np.float64) in q and in qd;
np.linalg.inv of Oracle.mass_matrix in fp64 for minv.  (Measured on the host: the difference agrees with -H^-1 dID/d(q, qd) from
differenced fp64 RNEA to <= 6e-8 on all six robots, differencing in f with inv(H) to <= 3e-13.)

YARDSTICKS, neither of them code under test, in err(X) = max over rows of max|X - X64| / max|X64|:
  (a) the same formulas in float32 LAPACK: the fp64-differenced dID/dq and dID/dqd rounded to float32 and the oracle's float32 H,
      -np.linalg.solve(H32, .) and np.linalg.inv(H32);
  (b) the reference's own float32 Jacobians of its compute_forward_dynamics from the fixture, over the rows it holds (flags
      gravity = damping = True only).
REQUIREMENT, for each of dqdd_dq, dqdd_dqd, minv and each path: err(path) <= 8 max(err(a), err(b), 2^-23); 8 is the project's margin
for unpivoted elimination and a different summation order (tests/test_operational_space.py).  qdd must equal
compute_forward_dynamics to atol = rtol = 2e-5.  Every comparison prints one "FDD" line (check, robot, flags, path, array, error,
yardstick) before it asserts; profiles/fd_derivatives_tests.txt holds them for the host build and the MI355X.

GPU (-m gpu): a launch of B rows is repeated over consecutive slices of the 128 rows, so the statistic is taken over the same rows
as on the CPU whatever B is.  A 30-joint serial chain (test_max_sizes.chain_model, 65 rows of sample_states, yardstick (a) alone) adds
the one size at which the GPU's finish kernel inverts H in the scratch instead of LDS.

Measured (profiles/fd_derivatives_tests.txt): the worst err(path) / yardstick is 6.2 on the host build (Fetch, dqdd_dq, no gravity, no
damping) and 1.3 on the MI355X (Allegro, dqdd_dq).
"""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, load_model
from oracle import Oracle

ROWS, FD_H, FLOOR, MARGIN = 128, 1e-5, 2.0 ** -23, 8.0
ROBOTS = ("panda_no_gripper", "iiwa7", "fetch", "allegro_left", "2link_robot", "iiwa7_allegro")
ALL_FLAGS = [(g, d) for g in (True, False) for d in (True, False)]
REF_FLAGS = (True, True)          # the flags of the reference's Jacobians in the fixture
ARRAYS = ("dqdd_dq", "dqdd_dqd", "minv")


@functools.lru_cache(maxsize=None)
def model_on(robot, device="cpu", compat=True):
    return load_model(robot, device, reference_compat=compat)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN_DIR, "golden_fd_derivatives.npz"), allow_pickle=False)


def states(robot):
    g = fixture()
    return tuple(g["%s/%s" % (robot, k)] for k in ("q", "qd", "f"))


def reference_jacobians(robot):
    """(dq, dqd, df) [rows, n, n] float32 of the unmodified reference, or None where the fixture holds none."""
    g = fixture()
    if robot + "/ref_dq" not in g.files:
        return None
    return tuple(g["%s/%s" % (robot, k)] for k in ("ref_dq", "ref_dqd", "ref_df"))


def central(fun, x):
    """[B, n_out, n] fp64: d fun / d x by central differences, one column of x at a time."""
    cols = []
    for j in range(x.shape[1]):
        d = np.zeros_like(x)
        d[:, j] = FD_H
        cols.append((fun(x + d) - fun(x - d)) / (2 * FD_H))
    return np.stack(cols, 2)


@functools.lru_cache(maxsize=None)
def problem(robot, gravity, damping, compat=True):
    """dict: truth (fp64) and yardstick (a) (float32 LAPACK) of the three arrays, H64, and qdd64 at the fixture's states."""
    return build_problem(Oracle(model_on(robot, "cpu", compat)._spec), states(robot), gravity, damping)


def build_problem(orc, inputs, gravity, damping):
    q, qd, f = (x.astype(np.float64) for x in inputs)
    fd = lambda a, b: orc.forward_dynamics(a, b, f, gravity, damping, np.float64)
    qdd = fd(q, qd)
    H64 = orc.mass_matrix(q, True, True, np.float64)             # (H depends on neither flag; called as the OSC test calls it)
    truth = (central(lambda x: fd(x, qd), q), central(lambda x: fd(q, x), qd), np.linalg.inv(H64))
    idq = central(lambda x: orc.rnea(x, qd, qdd, gravity, damping, np.float64), q).astype(np.float32)
    idqd = central(lambda x: orc.rnea(q, x, qdd, gravity, damping, np.float64), qd).astype(np.float32)
    H32 = orc.mass_matrix(q.astype(np.float32), True, True, np.float32)
    yard = (-np.linalg.solve(H32, idq), -np.linalg.solve(H32, idqd), np.linalg.inv(H32))
    assert all(y.dtype == np.float32 for y in yard)
    return dict(truth=truth, yard=yard, H64=H64, qdd=qdd)


def err(X, X64):
    X, X64 = np.asarray(X, np.float64).reshape(len(X64), -1), np.asarray(X64).reshape(len(X64), -1)
    return float((np.abs(X - X64).max(1) / np.abs(X64).max(1)).max())


def report(check, robot, flags, path, array, value, other):
    print("FDD %-9s %-17s g%d d%d %-14s %-9s %.3e  %.3e" % (check, robot, flags[0], flags[1], path, array, value, other))


def yardstick(robot, flags, k, rows, compat=True):
    """max(err(a), err(b), floor) of array k over `rows` (b: the rows of `rows` the fixture holds, flags (True, True) only)."""
    p = problem(robot, flags[0], flags[1], compat)
    ey = err(p["yard"][k][rows], p["truth"][k][rows])
    ref = reference_jacobians(robot) if compat and tuple(flags) == REF_FLAGS else None
    if ref is not None:
        held = np.arange(ROWS)[rows]
        held = held[held < len(ref[k])]
        if held.size:
            ey = max(ey, err(ref[k][held], p["truth"][k][held]))
    return max(ey, FLOOR)


def check_against_truth(robot, flags, path, out, rows=slice(None), compat=True):
    """The 8 x rule for the three matrices and TOL_TAU-style closeness of qdd to the fp64 forward dynamics, over `rows`."""
    p = problem(robot, flags[0], flags[1], compat)
    got = [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in out]
    n = states(robot)[0].shape[1]
    count = len(p["qdd"][rows])
    assert got[0].shape == (count, n) and all(g.shape == (count, n, n) for g in got[1:])
    bad = []
    for k, name in enumerate(ARRAYS):
        e, ey = err(got[1 + k], p["truth"][k][rows]), yardstick(robot, flags, k, rows, compat)
        report("truth", robot, flags, path, name, e, ey)
        if not e <= MARGIN * ey:
            bad.append((name, e, ey))
    assert not bad, bad
    return got


def run_model(model, robot, flags, B=None, composed=False):
    """compute_forward_dynamics_derivatives over the 128 rows in consecutive launches of B rows (None: one launch)."""
    q, qd, f = (torch.from_numpy(x).to(model._device) for x in states(robot))
    B = B or ROWS
    outs = [model.compute_forward_dynamics_derivatives(q[i:i + B], qd[i:i + B], f[i:i + B], flags[0], flags[1], _composed=composed)
            for i in range(0, ROWS, B)]
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))


def check_qdd(model, robot, flags, out, B=None):
    """qdd against compute_forward_dynamics of the same launches (a launch of another size may run another forward-dynamics kernel)."""
    q, qd, f = (torch.from_numpy(x).to(model._device) for x in states(robot))
    B = B or ROWS
    want = torch.cat([model.compute_forward_dynamics(q[i:i + B], qd[i:i + B], f[i:i + B], include_gravity=flags[0], use_damping=flags[1])
                      for i in range(0, ROWS, B)])
    torch.testing.assert_close(out[0], want, atol=2e-5, rtol=2e-5)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("flags", ALL_FLAGS, ids=lambda f: "g%d-d%d" % f)
@pytest.mark.parametrize("robot", ROBOTS)
def test_host_build_against_truth(cpu_library, robot, flags):
    model = model_on(robot)
    out = run_model(model, robot, flags)
    assert type(out) is tuple
    check_against_truth(robot, flags, "host", out)
    check_qdd(model, robot, flags, out)


@pytest.mark.parametrize("robot", [r for r in ROBOTS if r != "iiwa7_allegro"])
def test_reference_yardstick_agrees_with_the_formulas(robot):
    """Yardstick (b) lies within 8 x of yardstick (a) over the rows it holds: the semantics are the reference's."""
    p = problem(robot, *REF_FLAGS)
    ref = reference_jacobians(robot)
    bad = []
    for k, name in enumerate(ARRAYS):
        held = slice(0, len(ref[k]))
        eb, ea = err(ref[k], p["truth"][k][held]), err(p["yard"][k][held], p["truth"][k][held])
        report("reference", robot, REF_FLAGS, "reference", name, eb, ea)
        if not eb <= MARGIN * max(ea, FLOOR):
            bad.append((name, eb, ea))
    assert not bad, bad


def test_fetch_with_sliding_joints(cpu_library):
    """Fetch with its torso lift and fingers modelled as the prismatic joints they are (reference_compat=False)."""
    model = model_on("fetch", "cpu", False)
    out = run_model(model, "fetch", (True, True))
    check_against_truth("fetch", (True, True), "host-prismatic", out, compat=False)
    check_qdd(model, "fetch", (True, True), out)


@pytest.mark.parametrize("robot", ["panda_no_gripper", "fetch", "allegro_left"])
def test_identities(cpu_library, robot):
    """minv symmetric and minv H = I by the 8 x rule; dqdd_dqd with damping minus without = -minv diag(damping) by the same rule."""
    model = model_on(robot)
    flags = (True, True)
    p = problem(robot, *flags)
    out = [t.numpy() for t in run_model(model, robot, flags)]
    minv = out[3]
    bound = MARGIN * yardstick(robot, flags, 2, slice(None))
    e = err(minv.transpose(0, 2, 1), minv.astype(np.float64))
    report("symmetry", robot, flags, "host", "minv", e, bound / MARGIN)
    assert e <= bound
    n = minv.shape[1]
    eye = np.broadcast_to(np.eye(n), minv.shape)
    e = err(minv.astype(np.float64) @ p["H64"], eye)
    ey = max(err(p["yard"][2].astype(np.float64) @ p["H64"], eye), FLOOR)
    report("inverse", robot, flags, "host", "minv H", e, ey)
    assert e <= MARGIN * ey
    plain = [t.numpy() for t in run_model(model, robot, (True, False))]
    damping = _damping(model)
    want = -p["truth"][2] * damping[None, None, :]
    diff = out[2].astype(np.float64) - plain[2].astype(np.float64)
    scale = np.abs(p["truth"][1]).reshape(ROWS, -1).max(1)          # the difference of two arrays of this size
    e = float((np.abs(diff - want).reshape(ROWS, -1).max(1) / scale).max())
    ey = yardstick(robot, flags, 1, slice(None)) + yardstick(robot, (True, False), 1, slice(None))
    report("damping", robot, flags, "host", "dqdd_dqd", e, ey)
    assert e <= MARGIN * ey


def _damping(model):
    """[n] joint damping by DoF, read back through inverse dynamics: tau(qd = e_j) - tau(qd = 0) without gravity at q = 0."""
    n = model._n_dofs
    z = torch.zeros(n, n)
    with_d = model.compute_inverse_dynamics(z, torch.eye(n), z, include_gravity=False, use_damping=True)
    without = model.compute_inverse_dynamics(z, torch.eye(n), z, include_gravity=False, use_damping=False)
    return torch.diagonal(with_d - without).double().numpy()


def test_f_is_left_alone_and_no_autograd_history(cpu_library):
    from differentiable_robot_model_amd import ForwardDynamicsDerivatives
    model = model_on("panda_no_gripper")
    q, qd, f = (torch.from_numpy(x[:16].copy()) for x in states("panda_no_gripper"))
    keep = f.clone()
    out = model.compute_forward_dynamics_derivatives(q.requires_grad_(True), qd, f.requires_grad_(True), True, True)
    assert torch.equal(f, keep)
    assert type(out) is ForwardDynamicsDerivatives and out._fields == ("qdd", "dqdd_dq", "dqdd_dqd", "minv")
    assert all(t.grad_fn is None and not t.requires_grad and t.dtype == torch.float32 for t in out)


@pytest.mark.parametrize("shape", [(), (1,), (3,)], ids=str)
def test_batch_shapes(cpu_library, shape):
    model = model_on("iiwa7")
    q, qd, f = (torch.from_numpy(x[:3].copy()) for x in states("iiwa7"))
    many = model.compute_forward_dynamics_derivatives(q, qd, f)
    pick = (lambda t: t[1]) if shape == () else (lambda t: t[:shape[0]])
    got = model.compute_forward_dynamics_derivatives(pick(q), pick(qd), pick(f))
    assert got.qdd.shape == shape + (7,) and all(t.shape == shape + (7, 7) for t in got[1:])
    assert all(torch.equal(a, pick(b)) for a, b in zip(got, many))


def test_empty_batch(cpu_library):
    model = model_on("iiwa7")
    e = torch.empty(0, 7)
    out = model.compute_forward_dynamics_derivatives(e, e, e)
    assert out.qdd.shape == (0, 7) and all(t.shape == (0, 7, 7) for t in out[1:])


def nan_row_check(model, device, composed=False, B=64):
    q, qd, f = (torch.from_numpy(x[:B].copy()).to(device) for x in states("panda_no_gripper"))
    clean = model.compute_forward_dynamics_derivatives(q, qd, f, True, True, _composed=composed)
    q[37, 2] = float("nan")
    got = model.compute_forward_dynamics_derivatives(q, qd, f, True, True, _composed=composed)
    others = torch.arange(B, device=device) != 37
    for a, b in zip(got, clean):
        assert not torch.isfinite(a[37]).any()
        assert torch.equal(a[others], b[others])


def test_non_finite_row(cpu_library):
    nan_row_check(model_on("panda_no_gripper"), "cpu")


def test_refuses_the_trees_the_backward_kernels_refuse(cpu_library, tmp_path):
    """A tree with nine branch points open at once: gradients of compute_forward_dynamics are refused (the backward kernels address six
    save slots), and so is this call, with the same message."""
    import contextlib
    import io
    from differentiable_robot_model_amd import DifferentiableRobotModel
    from test_max_sizes import comb_urdf
    path = os.path.join(str(tmp_path), "comb.urdf")
    with open(path, "w") as fh:
        fh.write(comb_urdf(9))
    with contextlib.redirect_stdout(io.StringIO()):
        model = DifferentiableRobotModel(path)
    q = torch.zeros(2, model._n_dofs)
    with pytest.raises(NotImplementedError) as want:
        model.compute_forward_dynamics(q.clone().requires_grad_(True), q, q)
    with pytest.raises(NotImplementedError) as got:
        model.compute_forward_dynamics_derivatives(q, q, q)
    assert str(got.value) == str(want.value) and "<= 6 branch points" in str(got.value)


def long_chain_check(tmp_path, device, path):
    """A serial chain of 30 joints, 65 rows: on the GPU the rows' H no longer fits in LDS and is inverted in the scratch."""
    from helpers import sample_states
    from test_max_sizes import chain_model
    model, flags = chain_model(tmp_path, 30, device), (True, True)
    q, qd, qdd0 = (torch.from_numpy(x).to(device) for x in sample_states(model, 65, seed=0))
    f = model.compute_inverse_dynamics(q, qd, qdd0, include_gravity=True, use_damping=True)
    p = build_problem(Oracle(model._spec), [t.cpu().numpy() for t in (q, qd, f)], *flags)
    out = model.compute_forward_dynamics_derivatives(q, qd, f, *flags)
    if device != "cpu":
        torch.cuda.synchronize()
    bad = []
    for k, name in enumerate(ARRAYS):
        e, ey = err(out[1 + k].cpu().numpy(), p["truth"][k]), max(err(p["yard"][k], p["truth"][k]), FLOOR)
        report("truth", "chain30", flags, path, name, e, ey)
        if not e <= MARGIN * ey:
            bad.append((name, e, ey))
    assert not bad, bad
    torch.testing.assert_close(out[0], model.compute_forward_dynamics(q, qd, f, include_gravity=True, use_damping=True), atol=2e-5, rtol=2e-5)


def test_long_chain(cpu_library, tmp_path):
    long_chain_check(tmp_path, "cpu", "host")


# ------------------------------------------------------------------------------------------------------------------- GPU
GPU_FLAGS = (True, True)


@pytest.mark.gpu
def test_gpu_long_chain_inverts_in_the_scratch(tmp_path):
    long_chain_check(tmp_path, "cuda", "composed-B65")


def gpu_run_and_check(robot, B, composed=False, path=None):
    model = model_on(robot, "cuda:0")
    out = run_model(model, robot, GPU_FLAGS, B=B, composed=composed)
    torch.cuda.synchronize()
    got = check_against_truth(robot, GPU_FLAGS, path or ("composed" if composed else "fused") + "-B%d" % B, out)
    check_qdd(model, robot, GPU_FLAGS, out, B)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 128])
@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7"])
def test_gpu_arm_against_truth(robot, B):
    """Tiles are 64 rows: 64 and 128 are fused, 65 is one fused tile plus a composed tail, 1 and 63 are composed only."""
    gpu_run_and_check(robot, B)


@pytest.mark.gpu
def test_gpu_arm_composed_against_truth_and_fused():
    """Panda, 128 rows, every row through the composed path: held to the truth, and to the fused kernel on the same rows within the
    sum of both bounds."""
    robot = "panda_no_gripper"
    composed = gpu_run_and_check(robot, 128, composed=True)
    fused = gpu_run_and_check(robot, 128)
    for k, name in enumerate(ARRAYS):
        e = err(fused[1 + k], composed[1 + k].astype(np.float64))
        bound = 2 * MARGIN * yardstick(robot, GPU_FLAGS, k, slice(None))
        report("paths", robot, GPU_FLAGS, "fused-composed", name, e, bound)
        assert e <= bound


@pytest.mark.gpu
def test_gpu_misaligned_q():
    """q as a view one float into a larger buffer (4 bytes off a 16-byte boundary), straight through the C ABI (the Python binding would
    copy it to an aligned tensor): every row takes the composed path, the same bits as the aligned call with _composed, held to the
    truth."""
    import ctypes
    from differentiable_robot_model_amd import backend
    robot = "panda_no_gripper"
    model = model_on(robot, "cuda:0")
    lib = backend.load_library()
    dw = model._dynamics_walk()
    walk = backend._walk_struct(dw.program, model._ops_f(dw).detach(), dw.ops_i, 7)
    q, qd, f = (torch.from_numpy(x).cuda() for x in states(robot))
    buf = torch.zeros(ROWS * 7 + 1, device="cuda")
    buf[1:] = q.reshape(-1)
    vq = buf[1:].view(ROWS, 7)
    assert vq.data_ptr() % 16 != 0 and vq.is_contiguous()
    assert int(lib.drm_forward_dynamics_derivatives_scratch_floats_aligned(ctypes.byref(walk), ROWS)) == 0      # (all fused)
    need = int(lib.drm_forward_dynamics_derivatives_scratch_floats(ctypes.byref(walk), ROWS))
    assert need > 0
    scratch = torch.empty(need, device="cuda")
    out = [torch.empty(ROWS, 7, device="cuda")] + [torch.empty(ROWS, 7, 7, device="cuda") for _ in range(3)]
    flags = backend.RNEA_GRAVITY | backend.RNEA_DAMPING
    assert lib.drm_forward_dynamics_derivatives(ctypes.byref(walk), vq.data_ptr(), qd.data_ptr(), f.data_ptr(), ROWS, flags,
                                                *(t.data_ptr() for t in out), scratch.data_ptr(), backend._stream(vq.device)) == 0
    want = model.compute_forward_dynamics_derivatives(q, qd, f, *GPU_FLAGS, _composed=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    check_against_truth(robot, GPU_FLAGS, "misaligned", out)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 65])
@pytest.mark.parametrize("robot", ["fetch", "allegro_left", "2link_robot", "iiwa7_allegro"])
def test_gpu_composed_robots_against_truth(robot, B):
    """Fetch (articulated-body forward dynamics), the Allegro hand (finger kernels), the 2-link robot and an arm that carries a hand
    (23 DoFs: 64 rows of H take 138 KB of LDS)."""
    gpu_run_and_check(robot, B, path="composed-B%d" % B)


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "composed"])
def test_gpu_non_finite_row(composed):
    nan_row_check(model_on("panda_no_gripper", "cuda:0"), "cuda", composed=composed)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_second_stream():
    robot = "panda_no_gripper"
    model = model_on(robot, "cuda:0")
    q, qd, f = (torch.from_numpy(x[:65]).cuda() for x in states(robot))
    want = model.compute_forward_dynamics_derivatives(q, qd, f, *GPU_FLAGS)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = model.compute_forward_dynamics_derivatives(q, qd, f, *GPU_FLAGS)
    s.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))

"""The inverse-dynamics regressor in one call (csrc/drm_regressor.hip, include/drm_hip.h drm_rnea_regressor;
DifferentiableRobotModel.compute_inverse_dynamics_regressor / regressor_links / inertial_parameters): tau = Y(q, qd, qdd) phi.

INPUTS: the first 128 rows of q and qd per robot of tests/golden/golden_fd_derivatives.npz, qdd ~ U(-2, 2) from default_rng(0).

TRUTH, computed here: Y64, column by column, from Oracle.rnea(dtype=np.float64, use_damping=False) on copies of the robot's spec whose
links are all massless but one body, which carries unit parameters:
    m      m = 1, c = 0, I_c = 0                        tau of that model
    m c_a  m = 1, c = e_a, I_c = -(I - e_a e_a^T)       tau of that model minus the m column   (I_o = 0, all constants exact in float32)
    I_ab   m = 0, I_c[a, b] = I_c[b, a] = 1             tau of that model
so a block of the truth is in its link's URDF frame by construction.  The damping columns are qd itself.  Before anything under test is
compared, Y64 @ phi64 must reproduce the oracle's fp64 torque of the real robot to 1e-12 max|tau|, with phi64 built HERE from the spec:
every link behind a fixed joint composed into the nearest body above it in fp64.

YARDSTICK, not code under test: the same construction with dtype=np.float32 (the oracle's float32 RNEA on the unit-parameter robots).
METRIC: err(X) = max over rows and bodies of max|X - Y64| / max|Y64| over that row's block [n, 10]; a block whose truth is identically
zero must be exactly zero.  REQUIREMENT: err(path) <= 8 max(err(float32 oracle), 2^-23); 8 is the project's margin for a different
summation order (tests/test_operational_space.py, tests/test_fd_derivatives.py).  Torques: Y @ inertial_parameters() in fp64 against the
fp64 oracle torque of the real robot, max|.| / max|tau| <= 8 max(the float32 oracle's torque error, 2^-23).
Every comparison prints one "REG" line (robot, flags, path, error, yardstick, ratio) before it asserts; profiles/regressor_tests.txt
holds them for the host build and the MI355X.

GPU (-m gpu): a launch of B rows is repeated over consecutive slices of the 128 rows, so the statistic is over the same rows whatever
B is.  64-row tiles: B = 64 and 128 are the fused arm kernel, 65 and 131 a fused part plus a ragged tail in the general kernel, 1 the
general kernel alone.  test_max_sizes.chain_model's 30-joint chain at 65 rows is the size at which the general kernel's per-row records
(3 floats per op) leave LDS for the scratch.

Measured (profiles/regressor_tests.txt): the worst err(Y) / yardstick is 1.17 on the host build and 1.17 on the MI355X (Fetch with
sliding joints; the general kernel runs the host build's arithmetic), the worst torque ratio 2.11 on both (the 30-joint chain).
"""
import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, load_model
from oracle import Oracle

ROWS, FLOOR, MARGIN = 128, 2.0 ** -23, 8.0
ARMS = ("panda_no_gripper", "iiwa7")
OTHERS = ("fetch", "allegro_left", "2link_robot", "iiwa7_allegro")
ALL_FLAGS = [(g, d) for g in (True, False) for d in (True, False)]
TWO_FLAGS = [(True, False), (False, True)]
CASES = [(r, f) for r in ("panda_no_gripper", "fetch") for f in ALL_FLAGS] + \
        [(r, f) for r in ("iiwa7", "allegro_left", "2link_robot", "iiwa7_allegro") for f in TWO_FLAGS]
SYM = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


@functools.lru_cache(maxsize=None)
def model_on(robot, device="cpu", compat=True):
    return load_model(robot, device, reference_compat=compat)


@functools.lru_cache(maxsize=None)
def states(robot):
    g = np.load(os.path.join(GOLDEN_DIR, "golden_fd_derivatives.npz"), allow_pickle=False)
    q, qd = g[robot + "/q"][:ROWS], g[robot + "/qd"][:ROWS]
    qdd = np.random.default_rng(0).uniform(-2.0, 2.0, q.shape).astype(np.float32)
    return q, qd, qdd


def unit_spec(spec, body, mass, com, inertia):
    L = spec.n_links
    m, c, I = np.zeros(L, np.float32), np.zeros((L, 3), np.float32), np.zeros((L, 9), np.float32)
    m[body], c[body], I[body] = mass, com, np.asarray(inertia, np.float32).reshape(9)
    return dataclasses.replace(spec, mass=m, com=c, inertia=I)


def regressor_from_oracle(spec, bodies, inputs, gravity, dtype):
    """[B, n, 10 len(bodies)] in dtype: the unit-parameter construction of the module docstring."""
    q, qd, qdd = (x.astype(dtype) for x in inputs)
    tau = lambda s: Oracle(s).rnea(q, qd, qdd, gravity, False, dtype)
    eye, cols = np.eye(3), []
    for b in bodies:
        m_col = tau(unit_spec(spec, b, 1.0, np.zeros(3), np.zeros(9)))
        cols.append(m_col)
        for a in range(3):
            cols.append(tau(unit_spec(spec, b, 1.0, eye[a], -(eye - np.outer(eye[a], eye[a])))) - m_col)
        for a, c in SYM:
            I = np.zeros((3, 3))
            I[a, c] = I[c, a] = 1.0
            cols.append(tau(unit_spec(spec, b, 0.0, np.zeros(3), I)))
    return np.stack(cols, 2)


def rpy_matrix(rpy):
    r, p, y = (float(v) for v in rpy)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def phi_from_spec(spec, bodies):
    """[10 len(bodies)] fp64: (m, m c, I_o) of every body in its own URDF frame, every other link composed into the nearest body
    above it through its fixed joints (links with no body above them rest on the root and drop out)."""
    slot = {int(b): i for i, b in enumerate(bodies)}
    phi = np.zeros((len(bodies), 10))
    for link in range(1, spec.n_links):
        R, p, at = np.eye(3), np.zeros(3), link
        while at > 0 and at not in slot:
            assert spec.dof[at] < 0, "a moving link is always a body"
            Rj, tj = rpy_matrix(spec.rpy[at].astype(np.float64)), spec.trans[at].astype(np.float64)
            R, p = Rj @ R, Rj @ p + tj
            at = int(spec.parent[at])
        if at <= 0:
            continue
        m = float(spec.mass[link])
        c = R @ spec.com[link].astype(np.float64) + p
        Io = R @ spec.inertia[link].astype(np.float64).reshape(3, 3) @ R.T + m * ((c @ c) * np.eye(3) - np.outer(c, c))
        phi[slot[at]] += np.concatenate([[m], m * c, [Io[a, b] for a, b in SYM]])
    return phi.reshape(-1)


def bodies_of(model):
    return [model._name_to_idx_map[name] for name in model.regressor_links()]


def build_problem(spec, bodies, inputs, gravity):
    orc = Oracle(spec)
    q, qd, qdd = inputs
    Y64 = regressor_from_oracle(spec, bodies, inputs, gravity, np.float64)
    Y32 = regressor_from_oracle(spec, bodies, inputs, gravity, np.float32)
    assert Y32.dtype == np.float32
    phi64 = phi_from_spec(spec, bodies)
    f64 = lambda x: x.astype(np.float64)
    tau64 = orc.rnea(f64(q), f64(qd), f64(qdd), gravity, False, np.float64)
    pin = np.abs(Y64 @ phi64 - tau64).max()
    assert pin <= 1e-12 * np.abs(tau64).max(), pin       # the truth and the folding convention, before anything under test
    return dict(Y64=Y64, Y32=Y32, phi64=phi64, orc=orc)


@functools.lru_cache(maxsize=None)
def problem(robot, gravity, compat=True):
    model = model_on(robot, "cpu", compat)
    return build_problem(model._spec, tuple(bodies_of(model)), states(robot), gravity)


def block_err(X, Y64):
    """err of the module docstring over [B, n, 10 Nb] arrays; asserts exact zeros where a block of the truth is identically zero."""
    B, n, P = Y64.shape
    X = np.asarray(X, np.float64).reshape(B, n, P // 10, 10)
    T = Y64.reshape(B, n, P // 10, 10)
    scale = np.abs(T).max(axis=(1, 3))                    # [B, Nb]
    dead = scale == 0
    assert (np.abs(X).max(axis=(1, 3))[dead] == 0).all(), "a block whose truth is identically zero must be exactly zero"
    diff = np.abs(X - T).max(axis=(1, 3))
    return float((diff[~dead] / scale[~dead]).max()) if (~dead).any() else 0.0


def report(robot, flags, path, e, ey):
    print("REG %-17s g%d d%d %-16s %.3e  %.3e  %.2f" % (robot, flags[0], flags[1], path, e, ey, e / ey))


def check_against_truth(robot, flags, path, Y, inputs=None, prob=None, rows=slice(None)):
    """Check 1: shape, the damping columns (qd itself, to the bit), the 8 x rule over the body blocks."""
    p = prob or problem(robot, flags[0])
    q, qd, qdd = inputs or states(robot)
    Y = np.asarray(Y.cpu() if isinstance(Y, torch.Tensor) else Y)
    Y64, Y32 = p["Y64"][rows], p["Y32"][rows]
    B, n, P10 = Y64.shape
    assert Y.dtype == np.float32 and Y.shape == (B, n, P10 + (n if flags[1] else 0))
    if flags[1]:
        want = np.zeros((B, n, n), np.float32)
        want[:, np.arange(n), np.arange(n)] = qd[rows]
        assert np.array_equal(Y[:, :, P10:], want)
    e, ey = block_err(Y[:, :, :P10], Y64), max(block_err(Y32, Y64), FLOOR)
    report(robot, flags, path, e, ey)
    assert e <= MARGIN * ey, (e, ey)
    return Y


def check_torques(model, robot, flags, path, Y, inputs=None, prob=None):
    """Check 2: Y @ inertial_parameters() and compute_inverse_dynamics, each held to the fp64 oracle torque of the real robot."""
    p = prob or problem(robot, flags[0])
    q, qd, qdd = inputs or states(robot)
    f64 = lambda x: x.astype(np.float64)
    tau64 = p["orc"].rnea(f64(q), f64(qd), f64(qdd), flags[0], flags[1], np.float64)
    tau32 = p["orc"].rnea(q, qd, qdd, flags[0], flags[1], np.float32)
    scale = np.abs(tau64).max()
    ey = max(np.abs(tau32 - tau64).max() / scale, FLOOR)
    phi = model.inertial_parameters(use_damping=flags[1])
    assert phi.dtype == torch.float32 and phi.shape == (Y.shape[2],) and not phi.requires_grad and phi.device.type == model._device.type
    nb = len(model.regressor_links())
    assert Y.shape[2] == 10 * nb + (len(q[0]) if flags[1] else 0)
    assert np.abs(phi.cpu().numpy()[:10 * nb] - p["phi64"]).max() <= 1e-6 * max(np.abs(p["phi64"]).max(), 1.0)
    e = np.abs(np.asarray(Y, np.float64) @ phi.cpu().numpy().astype(np.float64) - tau64).max() / scale
    to = lambda x: torch.from_numpy(x).to(model._device)
    tau = model.compute_inverse_dynamics(to(q), to(qd), to(qdd), include_gravity=flags[0], use_damping=flags[1]).detach().cpu().numpy()
    e_id = np.abs(tau - tau64).max() / scale
    report(robot, flags, path + ":Y@phi", e, ey)
    report(robot, flags, path + ":ID", e_id, ey)
    assert e <= MARGIN * ey and e_id <= MARGIN * ey, (e, e_id, ey)


def run_model(model, robot, flags, B=None, composed=False):
    """compute_inverse_dynamics_regressor over the 128 rows in consecutive launches of B rows (None: one launch)."""
    q, qd, qdd = (torch.from_numpy(x).to(model._device) for x in states(robot))
    B = B or ROWS
    return torch.cat([model.compute_inverse_dynamics_regressor(q[i:i + B], qd[i:i + B], qdd[i:i + B], flags[0], flags[1],
                                                               _composed=composed) for i in range(0, ROWS, B)])


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("robot,flags", CASES, ids=lambda v: v if isinstance(v, str) else "g%d-d%d" % v)
def test_host_build_against_truth(cpu_library, robot, flags):
    model = model_on(robot)
    Y = run_model(model, robot, flags)
    assert type(Y) is torch.Tensor and Y.grad_fn is None and not Y.requires_grad
    Y = check_against_truth(robot, flags, "host", Y)
    check_torques(model, robot, flags, "host", Y)


def test_fetch_with_sliding_joints(cpu_library):
    """Fetch with its torso lift and fingers modelled as the prismatic joints they are (reference_compat=False)."""
    model, flags = model_on("fetch", "cpu", False), (True, True)
    assert (model._spec.kind == 2).any()
    p = problem("fetch", True, False)
    Y = check_against_truth("fetch", flags, "host-prismatic", run_model(model, "fetch", flags), prob=p)
    check_torques(model, "fetch", flags, "host-prismatic", Y, prob=p)


def test_bodies_and_zero_pattern(cpu_library):
    """regressor_links() names the moving links of the folded walk; Y[j, block i] is exactly zero where body i is not below joint j."""
    model = model_on("allegro_left")
    spec, names = model._spec, model.regressor_links()
    assert [n for n in names if spec.dof[model._name_to_idx_map[n]] >= 0] == [spec.link_names[i] for i in spec.preorder() if spec.dof[i] >= 0]
    Y = run_model(model, "allegro_left", (True, False)).numpy()
    for i, name in enumerate(names):
        chain = set(spec.chain_to(model._name_to_idx_map[name]))
        for j, link in enumerate(spec.controlled):
            if link not in chain:
                assert not Y[:, j, 10 * i:10 * i + 10].any()


def test_detached_and_argument_handling(cpu_library):
    model = model_on("iiwa7")
    q, qd, qdd = (torch.from_numpy(x[:3].copy()) for x in states("iiwa7"))
    many = model.compute_inverse_dynamics_regressor(q.requires_grad_(True), qd, qdd.requires_grad_(True))
    assert many.shape == (3, 7, 70) and many.grad_fn is None and not many.requires_grad and many.dtype == torch.float32
    one = model.compute_inverse_dynamics_regressor(q[1].detach(), qd[1], qdd[1].detach())
    assert one.shape == (7, 70) and torch.equal(one, many[1])
    assert model.compute_inverse_dynamics_regressor(q[:1].detach(), qd[:1], qdd[:1].detach(), True, True).shape == (1, 7, 77)
    e = torch.empty(0, 7)
    assert model.compute_inverse_dynamics_regressor(e, e, e).shape == (0, 7, 70)
    with pytest.raises(AssertionError):
        model.compute_inverse_dynamics_regressor(q.detach(), qd[:2], qdd.detach())


def walk_of(model):
    from differentiable_robot_model_amd import backend
    dw = model._dynamics_walk()
    return backend._walk_struct(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs)


def test_c_abi_codes_on_the_host_build(cpu_library):
    """NULL arguments and B = 0 straight through the C ABI of the host build; the guard words behind Y stay."""
    from differentiable_robot_model_amd import backend
    lib = backend.load_library(kind="cpu")
    model = model_on("panda_no_gripper")
    walk = walk_of(model)
    q, qd, qdd = (torch.from_numpy(x[:5].copy()) for x in states("panda_no_gripper"))
    assert lib.drm_rnea_regressor_scratch_floats(ctypes.byref(walk), 5) == 0
    assert lib.drm_rnea_regressor_scratch_floats_aligned(ctypes.byref(walk), 5) == 0
    Y = torch.full((5 * 7 * 70 + 8,), 7.5)
    call = lambda a, b, c, B, y: lib.drm_rnea_regressor(ctypes.byref(walk), a, b, c, B, backend.RNEA_GRAVITY, y, None, None)
    assert call(None, qd.data_ptr(), qdd.data_ptr(), 5, Y.data_ptr()) == -1
    assert call(q.data_ptr(), None, qdd.data_ptr(), 5, Y.data_ptr()) == -1
    assert call(q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), 5, None) == -1
    assert call(q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), -1, Y.data_ptr()) == -1
    assert call(q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), 0, Y.data_ptr()) == 0
    assert (Y == 7.5).all()
    assert call(q.data_ptr(), qd.data_ptr(), None, 5, Y.data_ptr()) == 0          # qdd = NULL: zeros
    want = model.compute_inverse_dynamics_regressor(q, qd, torch.zeros_like(qdd))
    assert torch.equal(Y[:5 * 7 * 70].view(5, 7, 70), want) and (Y[5 * 7 * 70:] == 7.5).all()


def bad_rows_check(model, device, composed=False, B=128):
    """One row with NaN in q, one with Inf in qdd: every other row keeps its bits; the bad rows are non-finite wherever the truth
    depends on the bad input (measured on the fp64 truth: the entries that move when that input does)."""
    robot, flags = "panda_no_gripper", (True, False)
    q, qd, qdd = (torch.from_numpy(x[:B].copy()).to(device) for x in states(robot))
    run = lambda: model.compute_inverse_dynamics_regressor(q, qd, qdd, *flags, _composed=composed)
    clean = run()
    q[37, 2] = float("nan")
    qdd[70, 4] = float("inf")
    got = run()
    others = torch.ones(B, dtype=torch.bool, device=device)
    others[[37, 70]] = False
    assert torch.equal(got[others], clean[others])
    spec, bodies = model._spec, bodies_of(model)
    for row, arr, col in ((37, 0, 2), (70, 2, 4)):
        base = [x[row:row + 1].copy() for x in states(robot)]
        moved = [x.copy() for x in base]
        moved[arr][0, col] += 0.37
        T0 = regressor_from_oracle(spec, bodies, base, flags[0], np.float64)[0]
        T1 = regressor_from_oracle(spec, bodies, moved, flags[0], np.float64)[0]
        depends = np.abs(T1 - T0) > 1e-9 * np.abs(T0).max()
        assert depends.any()
        assert not np.isfinite(got[row].cpu().numpy()[depends]).any()


def test_non_finite_rows(cpu_library):
    bad_rows_check(model_on("panda_no_gripper"), "cpu")


def learnable_check(device, path):
    """A model with one learnable link whose parameter has moved: Y against the oracle on the changed spec; the kept link is a body."""
    from differentiable_robot_model_amd.rigid_body_params import UnconstrainedTensor
    robot, flags, link = "panda_no_gripper", (True, False), "panda_virtual_ee_link"
    model = load_model(robot, device)
    idx = model._name_to_idx_map[link]
    assert model._spec.dof[idx] < 0 and link not in model.regressor_links()      # (folded away while nothing is learnable)
    trans = model._spec.trans[idx] + np.asarray([0.03, -0.02, 0.05], np.float32)
    model.make_link_param_learnable(link, "trans", UnconstrainedTensor(dim1=1, dim2=3, init_tensor=torch.from_numpy(trans)))
    assert link in model.regressor_links()
    new_trans = model._spec.trans.copy()
    new_trans[idx] = trans
    spec = dataclasses.replace(model._spec, trans=new_trans)
    p = build_problem(spec, tuple(bodies_of(model)), states(robot), flags[0])
    Y = run_model(model, robot, flags)
    assert Y.grad_fn is None and not Y.requires_grad
    Y = check_against_truth(robot, flags, path, Y, prob=p)
    check_torques(model, robot, flags, path, Y, prob=p)


def test_learnable_link(cpu_library):
    learnable_check("cpu", "host-learnable")


def long_chain_check(tmp_path, device, path):
    """test_max_sizes.chain_model's 30-joint chain (joints about +-x / +-y / +-z), 65 rows."""
    from helpers import sample_states
    from test_max_sizes import chain_model
    model, flags = chain_model(tmp_path, 30, device), (True, True)
    inputs = sample_states(model, 65, seed=0)
    p = build_problem(model._spec, tuple(bodies_of(model)), inputs, flags[0])
    Y = model.compute_inverse_dynamics_regressor(*(torch.from_numpy(x).to(device) for x in inputs), *flags)
    Y = check_against_truth("chain30", flags, path, Y, inputs=inputs, prob=p)
    check_torques(model, "chain30", flags, path, Y, inputs=inputs, prob=p)


def test_long_chain(cpu_library, tmp_path):
    long_chain_check(tmp_path, "cpu", "host")


# ------------------------------------------------------------------------------------------------------------------- GPU
def gpu_run_and_check(robot, flags, B, composed=False, compat=True, path=None):
    model = model_on(robot, "cuda:0", compat)
    Y = run_model(model, robot, flags, B=B, composed=composed)
    torch.cuda.synchronize()
    p = problem(robot, flags[0], compat)
    name = path or ("general" if composed or robot not in ARMS else "fused") + "-B%d" % B
    Y = check_against_truth(robot, flags, name, Y, prob=p)
    check_torques(model, robot, flags, name, Y, prob=p)
    return Y


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 131])
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_against_truth(robot, B):
    for flags in (ALL_FLAGS if robot == "panda_no_gripper" else TWO_FLAGS):
        gpu_run_and_check(robot, flags, B)


@pytest.mark.gpu
def test_gpu_arm_general_kernel():
    """DRM_REGRESSOR_COMPOSED on the Panda: the general kernel on every row meets the same bound (it need not agree with the fused
    kernel to the bit)."""
    for flags in TWO_FLAGS:
        gpu_run_and_check("panda_no_gripper", flags, 128, composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 65])
@pytest.mark.parametrize("robot", OTHERS)
def test_gpu_other_robots_against_truth(robot, B):
    for flags in (ALL_FLAGS if robot == "fetch" else TWO_FLAGS):
        gpu_run_and_check(robot, flags, B)


@pytest.mark.gpu
def test_gpu_fetch_with_sliding_joints():
    gpu_run_and_check("fetch", (True, True), 65, compat=False, path="general-prismatic")


@pytest.mark.gpu
def test_gpu_long_chain_keeps_its_records_in_the_scratch(tmp_path):
    from differentiable_robot_model_amd import backend
    from test_max_sizes import chain_model
    walk = walk_of(chain_model(tmp_path, 30, "cuda"))
    assert backend.load_library().drm_rnea_regressor_scratch_floats(ctypes.byref(walk), 65) > 0
    long_chain_check(tmp_path, "cuda", "general-B65")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7_allegro"])
def test_gpu_c_abi_misaligned_and_guards(robot):
    """Straight through the C ABI: q, qd, qdd and Y 4 bytes off a 16-byte boundary (the general kernel), a scratch of exactly
    drm_rnea_regressor_scratch_floats floats, guard words behind the scratch and on both sides of Y."""
    from differentiable_robot_model_amd import backend
    flags = (True, True)
    model = model_on(robot, "cuda:0")
    lib, walk, n = backend.load_library(), walk_of(model), model._n_dofs
    P = 10 * len(model.regressor_links()) + n

    def off_by_4(x):
        buf = torch.zeros(x.numel() + 1, device="cuda")
        buf[1:] = x.reshape(-1)
        view = buf[1:].view(x.shape)
        assert view.data_ptr() % 16 == 4
        return view
    q, qd, qdd = (off_by_4(torch.from_numpy(x).cuda()) for x in states(robot))
    need = int(lib.drm_rnea_regressor_scratch_floats(ctypes.byref(walk), ROWS))
    assert (need > 0) == (robot == "iiwa7_allegro")
    GUARD = 64
    scratch = torch.full((need + GUARD,), 3.25, device="cuda")
    out = torch.full((1 + ROWS * n * P + GUARD,), -1.5, device="cuda")
    Y = out[1:1 + ROWS * n * P].view(ROWS, n, P)
    assert Y.data_ptr() % 16 == 4
    rc = lib.drm_rnea_regressor(ctypes.byref(walk), q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), ROWS,
                                backend.RNEA_GRAVITY | backend.RNEA_DAMPING, Y.data_ptr(), scratch.data_ptr(), backend._stream(q.device))
    torch.cuda.synchronize()
    assert rc == 0
    assert (scratch[need:] == 3.25).all() and (out[1 + ROWS * n * P:] == -1.5).all() and out[0] == -1.5
    Y = check_against_truth(robot, flags, "misaligned", Y)
    check_torques(model, robot, flags, "misaligned", Y)


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_non_finite_rows(composed):
    bad_rows_check(model_on("panda_no_gripper", "cuda:0"), "cuda", composed=composed)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_learnable_link():
    learnable_check("cuda:0", "learnable")

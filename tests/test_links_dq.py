"""The q-gradient of the link sweeps (csrc/drm_links.hip, include/drm_hip.h drm_link_power_dq; DifferentiableRobotModel.
compute_link_power_gradient and differentiable_q=True on compute_link_velocities / compute_external_torques): dS/dq of the power of
the wrenches, S(q; qd, F, M) = sum_l F_l . v_l + M_l . w_l = tau_ext(q; F, M) . qd, with qd and the wrenches held fixed.

INPUTS: tests/test_links.py's — the first 128 rows of q and qd per robot of tests/golden/golden_fd_derivatives.npz, seeded unit-scale
force and torque [128, L, 3] on every link (the root included).

TRUTH, from the fp64 oracle only: S64(q) = sum_l W64_l . (Oracle.fk_jacobian(q, l, float64) @ qd64); dS/dq_j a central difference at
h = 1e-4 and 3e-4, Richardson-combined as test_lagrangian.richardson does.

YARDSTICK, not code under test: the recursion of the entry point restated HERE in numpy (power_dq_world, over test_links._frames'
kinematics).  Run in fp64 it must first match the truth to PIN = 1e-8 relative (printed as a "yardstick64" line).  In float32 it is the
yardstick; for the shipped robots the existing differentiable path — autograd through compute_endeffector_jacobian per link on the CPU
build — gives the same gradient, so its error counts too and the larger is taken.  REQUIREMENT: row_err(path) <= 8 max(row_err(
yardstick), 2^-23), row_err test_lagrangian's per-row max|X - X64| / max|X64|, worst over rows.  Joints that no named link's chain
crosses are tested for exact zeros.  Every comparison prints one "LINKSDQ" line (robot, path, quantity, error, yardstick, ratio) before
it asserts; profiles/links_dq_tests.txt holds them.

BITS, on every run: tau of the drm_link_power_dq launch equals compute_external_torques; the forward values with differentiable_q=True
equal those without; autograd.grad((lin, ang), (q, qd), (f, m)) == (compute_link_power_gradient(q, qd, f, m), compute_external_torques(
q, f, m)); the q-gradient of compute_external_torques(q, f, m) under g equals compute_link_power_gradient(q, g, f, m).

GPU (-m gpu): as tests/test_links.py — a launch of B rows is repeated over consecutive slices of the 128 rows.  B = 64 and 128 are the
fused kernel, 65 and 131 a fused part plus a ragged tail, 1 / _composed=True / every other robot the general kernel; the 30-joint chain
at 65 rows keeps its records in the scratch.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import Oracle
from test_lagrangian import ARMS, OTHERS, model_on, richardson, row_err, states
from test_links import _cross, _frames, inputs, random_inputs, walk_of

ROWS, FLOOR, MARGIN = 128, 2.0 ** -23, 8.0
PIN = 1e-8           # the fp64 yardstick against the truth (tests/test_links.py's pin)


# ------------------------------------------------------------------------------------------- the yardstick: numpy, world frame
def power_dq_world(spec, q, qd, force, torque, dt):
    """dS/dq [B, n] in dtype dt: outwards the velocities, inwards the sub-tree wrench (F, M about the joint's origin) and the free
    vector A_k = v_k x F_k + w_k x M_k + sum over children A_c;
        revolute  j   dS/dq_j = z_j . (A_j - v_j x F^S_j) + (w_j x z_j) . M^S_j        prismatic j   dS/dq_j = (w_j x z_j) . F^S_j"""
    dt = np.dtype(dt).type
    qd = qd.astype(dt)
    B, n = q.shape
    L, frames = _frames(spec, q, dt)
    P, V, W = (np.zeros((B, L, 3), dt) for _ in range(3))
    for i, par, d, pris, z, r, _, p in frames:
        P[:, i] = p
        W[:, i], V[:, i] = W[:, par], V[:, par] + _cross(W[:, par], r)
        if d >= 0:
            if pris:
                V[:, i] = V[:, i] + z * qd[:, d:d + 1]
            else:
                W[:, i] = W[:, i] + z * qd[:, d:d + 1]
    F, M = force.astype(dt).copy(), torque.astype(dt).copy()
    A = (_cross(V, F) + _cross(W, M)).astype(dt)
    dot = lambda a, b: np.einsum("bi,bi->b", a, b)
    out = np.zeros((B, n), dt)
    for i, par, d, pris, z, r, _, p in reversed(frames):
        if d >= 0:
            wz = _cross(W[:, i], z)
            out[:, d] = dot(wz, F[:, i]) if pris else dot(z, A[:, i] - _cross(V[:, i], F[:, i])) + dot(wz, M[:, i])
        F[:, par] = F[:, par] + F[:, i]
        M[:, par] = M[:, par] + M[:, i] + _cross(P[:, i] - P[:, par], F[:, i])
        A[:, par] = A[:, par] + A[:, i]
    return out


# ------------------------------------------------------------------------------------------------------------------- truth
def report(robot, path, what, e, ey):
    print("LINKSDQ %-17s %-22s %-8s %.3e  %.3e  %.2f" % (robot, path, what, e, ey, e / ey))


def crossed(spec, links):
    """the DoFs that the chain of at least one of ``links`` crosses"""
    return sorted(set(int(spec.dof[i]) for l in links for i in spec.chain_to(l) if spec.dof[i] >= 0))


def jacobian_path(model, q, qd, force, torque):
    """dS/dq [B, n] float32 from the existing differentiable path: autograd through compute_endeffector_jacobian per loaded link"""
    names, spec = model.get_link_names(), model._spec
    qr = torch.from_numpy(q).requires_grad_(True)
    tqd = torch.from_numpy(qd)
    S = qr.sum() * 0.0
    for l in range(1, len(names)):
        if not crossed(spec, [l]) or not (force[:, l].any() or torque[:, l].any()):
            continue
        lin, ang = model.compute_endeffector_jacobian(qr, names[l])
        S = S + (torch.einsum("bij,bj->bi", lin, tqd) * torch.from_numpy(force[:, l])).sum() \
            + (torch.einsum("bij,bj->bi", ang, tqd) * torch.from_numpy(torque[:, l])).sum()
    (g,) = torch.autograd.grad(S, qr)
    return g.numpy()


def build_truth(spec, q, qd, force, torque, name="?", model=None):
    """``force`` / ``torque`` [B, L, 3] by link index.  ``model``: a CPU model whose Jacobian path counts as a yardstick too."""
    orc = Oracle(spec)
    B, n = q.shape
    L = len(spec.parent)
    q64, qd64, F64, M64 = (x.astype(np.float64) for x in (q, qd, force, torque))
    loaded = [l for l in range(1, L) if force[:, l].any() or torque[:, l].any()]

    def power(x):
        S = np.zeros(B)
        for l in loaded:
            _, _, lin, ang = orc.fk_jacobian(x, l, np.float64)
            S += np.einsum("bi,bij,bj->b", F64[:, l], lin, qd64) + np.einsum("bi,bij,bj->b", M64[:, l], ang, qd64)
        return S

    def column(j):
        e = np.zeros(n)
        e[j] = 1.0
        return richardson(lambda h: (power(q64 + h * e) - power(q64 - h * e)) / (2 * h))
    t64 = np.stack([column(j) for j in range(n)], axis=1)
    y64 = power_dq_world(spec, q, qd, force, torque, np.float64)
    e = row_err(y64, t64)
    report(name, "yardstick64", "dq", e, PIN)
    assert e <= PIN, e                                     # the yardstick in fp64 must be the truth
    y32 = power_dq_world(spec, q, qd, force, torque, np.float32)
    assert y32.dtype == np.float32
    j32 = jacobian_path(model, q, qd, force, torque) if model is not None else None
    live = crossed(spec, loaded)
    assert (t64[:, [d for d in range(n) if d not in live]] == 0).all()
    return dict(t64=t64, y32=y32, j32=j32, live=live)


@functools.lru_cache(maxsize=None)
def truth(robot, compat=True):
    q, qd, _, f, m = inputs(robot, compat)
    model = model_on(robot, "cpu", compat)
    return build_truth(model._spec, q, qd, f, m, name=robot, model=model if compat else None)


def check(robot, path, dq, t, rows=slice(None), what="dq"):
    x = np.asarray(dq.detach().cpu() if isinstance(dq, torch.Tensor) else dq)
    assert x.dtype == np.float32
    t64 = t["t64"][rows]
    assert x.shape == t64.shape, (x.shape, t64.shape)
    e = row_err(x, t64)
    ey = max(row_err(t["y32"][rows], t64), FLOOR)
    if t["j32"] is not None:
        ey = max(ey, row_err(t["j32"][rows], t64))
    report(robot, path, what, e, ey)
    dead = [d for d in range(x.shape[1]) if d not in t["live"]]
    assert (x[:, dead] == 0).all(), "joints that no named link's chain crosses: exact zeros"
    assert e <= MARGIN * ey, (e, ey)


def bits(model, q, qd, f, m, composed=False, link_names=None):
    """The bit identities of the module docstring on one launch's rows; returns compute_link_power_gradient's result."""
    from differentiable_robot_model_amd import backend
    kw = dict(link_names=link_names, _composed=composed)
    dq = model.compute_link_power_gradient(q, qd, f, m, **kw)
    assert dq.grad_fn is None and not dq.requires_grad and dq.shape == q.shape and dq.dtype == torch.float32
    tau = model.compute_external_torques(q, f, m, **kw)
    lin, ang = model.compute_link_velocities(q, qd, **kw)
    # tau of the same launch
    dw, T, sel, identity = model._links_plan(link_names)
    fs, ms = model._links_scatter(f, sel, T, identity), model._links_scatter(m, sel, T, identity)
    dq2, tau2 = backend.link_power_dq(dw.program, model._ops_f(dw).detach(), dw.ops_i, q, qd, fs, ms, T, model._n_dofs, want_tau=True,
                                      composed=composed)
    assert torch.equal(dq2, dq) and torch.equal(tau2, tau)
    # the velocities: same forward bits, (grad_q, grad_qd) from one launch
    qr, qdr = q.clone().requires_grad_(True), qd.clone().requires_grad_(True)
    lin_d, ang_d = model.compute_link_velocities(qr, qdr, differentiable_q=True, **kw)
    assert lin_d.requires_grad and torch.equal(lin_d.detach(), lin) and torch.equal(ang_d.detach(), ang)
    gq, gqd = torch.autograd.grad((lin_d, ang_d), (qr, qdr), (f, m))
    assert torch.equal(gq, dq) and torch.equal(gqd, tau)
    lin_q, ang_q = model.compute_link_velocities(qr, qd, differentiable_q=True, **kw)          # q alone
    assert torch.equal(torch.autograd.grad((lin_q, ang_q), qr, (f, m))[0], dq)
    # the torques: same forward bits, grad_q under the cotangent g is the primitive at qd := g
    tau_d = model.compute_external_torques(qr, f, m, differentiable_q=True, **kw)
    assert tau_d.requires_grad and torch.equal(tau_d.detach(), tau)
    assert torch.equal(torch.autograd.grad(tau_d, qr, qd)[0], dq)
    return dq


def run_model(model, data, B=None, composed=False):
    """compute_link_power_gradient over the rows in consecutive launches of B rows (None: one launch), with the bit identities."""
    q, qd, _, f, m = (torch.from_numpy(x).to(model._device) for x in data)
    N = q.shape[0]
    B = B or N
    return torch.cat([bits(model, q[i:i + B], qd[i:i + B], f[i:i + B], m[i:i + B], composed) for i in range(0, N, B)])


def more_checks(model, data, composed=False, B=None):
    """Forces alone / torques alone work and equal the call with zeros for the other; zero rates or zero wrenches give zeros; both
    wrenches None, a second backward and a q that requires grad with the keyword off raise."""
    q, qd, _, f, m = (torch.from_numpy(x[:B or ROWS]).to(model._device) for x in data)
    kw = dict(_composed=composed)
    both = model.compute_link_power_gradient(q, qd, f, m, **kw)
    only_f = model.compute_link_power_gradient(q, qd, f, **kw)
    only_m = model.compute_link_power_gradient(q, qd, None, m, **kw)
    assert torch.equal(only_f, model.compute_link_power_gradient(q, qd, f, torch.zeros_like(m), **kw))
    assert torch.equal(only_m, model.compute_link_power_gradient(q, qd, torch.zeros_like(f), m, **kw))
    assert torch.allclose(only_f + only_m, both, atol=1e-3)
    assert (model.compute_link_power_gradient(q, torch.zeros_like(qd), f, m, **kw) == 0).all()
    assert (model.compute_link_power_gradient(q, qd, torch.zeros_like(f), torch.zeros_like(m), **kw) == 0).all()
    qr = q.clone().requires_grad_(True)
    (gf,) = torch.autograd.grad(model.compute_external_torques(qr, f, differentiable_q=True, **kw), qr, qd)
    assert torch.equal(gf, only_f)
    with pytest.raises(ValueError):
        model.compute_link_power_gradient(q, qd, None, None)
    # first order only
    lin, ang = model.compute_link_velocities(qr, qd, differentiable_q=True, **kw)
    (g1,) = torch.autograd.grad((lin, ang), qr, (f.clone().requires_grad_(True), m), create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    # the keyword off: refused, not a silent zero
    for call in (lambda: model.compute_external_torques(qr, f, m, **kw), lambda: model.compute_link_velocities(qr, qd, **kw)):
        with pytest.raises(ValueError, match=r"q\.detach\(\)"):
            call()
    # q that does not require grad, or no grad mode: no node
    assert model.compute_external_torques(q, f, m, differentiable_q=True, **kw).grad_fn is None
    with torch.no_grad():
        assert model.compute_link_velocities(qr, qd, differentiable_q=True, **kw)[0].grad_fn is None
    one = model.compute_link_power_gradient(q[0], qd[0], f[0], m[0], **kw)
    assert one.shape == (model._n_dofs,) and torch.equal(one, both[0])
    assert model.compute_link_power_gradient(q[:0], qd[:0], f[:0], m[:0], **kw).shape == (0, model._n_dofs)
    with pytest.raises(AssertionError):
        model.compute_link_power_gradient(q, qd[:, :-1], f, m, **kw)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("robot", ARMS + OTHERS)
def test_host_build_against_truth(cpu_library, robot):
    model = model_on(robot)
    check(robot, "host", run_model(model, inputs(robot)), truth(robot))
    more_checks(model, inputs(robot))


@pytest.mark.parametrize("robot", ARMS)
def test_host_general_walk_on_the_arms(cpu_library, robot):
    check(robot, "host-general", run_model(model_on(robot), inputs(robot), composed=True), truth(robot))
    more_checks(model_on(robot), inputs(robot), composed=True)


def test_fetch_with_sliding_joints(cpu_library):
    model = model_on("fetch", "cpu", False)
    assert (model._spec.kind == 2).any()
    check("fetch", "host-prismatic", run_model(model, inputs("fetch", False)), truth("fetch", False))


def skew_check(tmp_path_factory, device, path):
    """tests/test_joint_models.py's toy robot: prismatic about z, revolute and prismatic about skew axes (two ops per skew link)."""
    from helpers import sample_states
    from test_joint_models import toy_model, toy_urdf
    urdf = tmp_path_factory.mktemp("toy_links_dq") / "toy.urdf"
    urdf.write_text(toy_urdf())
    model = toy_model(str(urdf), device)
    assert model._spec.skew.any()
    q, qd, _ = sample_states(model, 65, seed=1)
    data = (q, qd) + random_inputs(q.shape[1], len(model._spec.parent), rows=65)
    t = build_truth(model._spec, data[0], data[1], data[3], data[4], name="toy_skew")
    check("toy_skew", path, run_model(model, data), t)


def test_skew_axis_model(cpu_library, tmp_path_factory):
    skew_check(tmp_path_factory, "cpu", "host-prismatic")


def subset_check(robot, device, path, composed=False):
    """A subset of links in non-walk order, with a repeat and the root: repeated wrenches add up, the root's is dropped, and the
    joints that none of the named links' chains crosses get exact zeros."""
    model = model_on(robot, device)
    names = model.get_link_names()
    L = len(names)
    pick = [L - 1, 0, 2, L - 1, 1] if L > 3 else [L - 1, 0, L - 1, 1]
    sub = [names[i] for i in pick]
    data = inputs(robot)
    q, qd, _, f, m = (torch.from_numpy(x).to(device) for x in data)
    dq = bits(model, q, qd, f[:, pick].contiguous(), m[:, pick].contiguous(), composed, link_names=sub)
    F, M = np.zeros_like(data[3]), np.zeros_like(data[4])
    for l in pick:
        if l:
            F[:, l] += data[3][:, l]
            M[:, l] += data[4][:, l]
    t = subset_truth(robot, tuple(pick))
    assert np.array_equal(F, t["F"]) and np.array_equal(M, t["M"])
    if robot == "allegro_left":
        assert len(t["live"]) < model._n_dofs             # (the other fingers' joints: exact zeros, checked below)
    check(robot, path, dq, t)


@functools.lru_cache(maxsize=None)
def subset_truth(robot, pick):
    model = model_on(robot, "cpu")
    data = inputs(robot)
    F, M = np.zeros_like(data[3]), np.zeros_like(data[4])
    for l in pick:
        if l:
            F[:, l] += data[3][:, l]
            M[:, l] += data[4][:, l]
    return dict(build_truth(model._spec, data[0], data[1], F, M, name=robot, model=model), F=F, M=M)


@pytest.mark.parametrize("robot", ["panda_no_gripper", "allegro_left", "fetch"])
def test_subset_of_links_in_the_callers_order(cpu_library, robot):
    subset_check(robot, "cpu", "host-subset")


def long_chain_check(tmp_path, device, path):
    """test_max_sizes.chain_model's 30-joint chain (joints about +-x / +-y / +-z), 65 rows."""
    from helpers import sample_states
    from test_max_sizes import chain_model
    model = chain_model(tmp_path, 30, device)
    q, qd, _ = sample_states(model, 65, seed=0)
    data = (q, qd) + random_inputs(q.shape[1], len(model._spec.parent), rows=65)
    t = build_truth(model._spec, data[0], data[1], data[3], data[4], name="chain30")
    check("chain30", path, run_model(model, data), t)
    return model


def test_long_chain(cpu_library, tmp_path):
    long_chain_check(tmp_path, "cpu", "host")


def launch(model, q, qd, f, m, composed=False):
    """(dq, tau) of ONE drm_link_power_dq launch over every link of the model"""
    from differentiable_robot_model_amd import backend
    dw, T, sel, identity = model._links_plan(None)
    return backend.link_power_dq(dw.program, model._ops_f(dw).detach(), dw.ops_i, q, qd, model._links_scatter(f, sel, T, identity),
                                 model._links_scatter(m, sel, T, identity), T, model._n_dofs, want_tau=True, composed=composed)


def bad_rows_check(model, device, composed=False, B=128):
    """q[5] NaN, qd[70] Inf, q[3] = 4e5 planted in 128 rows: those rows are NaN in dq and tau, no other row changes a bit."""
    q, qd, _, f, m = (torch.from_numpy(x[:B].copy()).to(device) for x in inputs("panda_no_gripper"))
    clean = launch(model, q, qd, f, m, composed)
    q[5, 2] = float("nan")
    qd[70, 4] = float("inf")
    q[3, 1] = 4e5
    got = launch(model, q, qd, f, m, composed)
    others = torch.ones(B, dtype=torch.bool, device=device)
    others[[3, 5, 70]] = False
    for a, b in zip(got, clean):
        assert torch.isfinite(b).all()
        assert torch.equal(a[others], b[others]) and torch.isnan(a[[3, 5, 70]]).all()
    assert torch.isnan(model.compute_link_power_gradient(q, qd, f, m, _composed=composed)[[3, 5, 70]]).all()
    qd[9, 0] = float("-inf")
    q[11, 6] = float("inf")
    again = launch(model, q, qd, f, m, composed)
    assert all(torch.isnan(x[[9, 11]]).all() for x in again)


def test_non_finite_rows(cpu_library):
    bad_rows_check(model_on("panda_no_gripper"), "cpu")
    bad_rows_check(model_on("panda_no_gripper"), "cpu", composed=True)


def nan_wrench_check(device):
    """A NaN force on one fingertip of the Allegro: that finger's joints are non-finite in dq and tau, every other joint keeps its bits."""
    model = model_on("allegro_left", device)
    spec, names = model._spec, model.get_link_names()
    q, qd, _, f, m = (torch.from_numpy(x.copy()).to(device) for x in inputs("allegro_left"))
    clean = launch(model, q, qd, f, m)
    leaves = [i for i in range(len(names)) if i not in set(int(p) for p in spec.parent)]
    tip = leaves[0]
    on_chain = crossed(spec, [tip])
    assert 0 < len(on_chain) < model._n_dofs
    f[:, tip, 1] = float("nan")
    got = launch(model, q, qd, f, m)
    off = [d for d in range(model._n_dofs) if d not in on_chain]
    for a, b in zip(got, clean):
        assert torch.equal(a[:, off], b[:, off]) and not torch.isfinite(a[:, on_chain]).any()


def test_nan_force_on_one_fingertip(cpu_library):
    nan_wrench_check("cpu")


# ------------------------------------------------------------------------------------------------------------------- C ABI
def c_abi_check(lib, model, device, stream, B=5, flags=0):
    """The NULL-pointer combinations, the DRM_ERR_INVALID cases, B == 0, and the scratch query honoured with guard words behind it."""
    (walk, T), n = walk_of(model), model._n_dofs
    q, qd, _, f, m = (torch.from_numpy(x[:B].copy()).to(device) for x in inputs("panda_no_gripper"))
    f, m = f[:, 1:].contiguous(), m[:, 1:].contiguous()          # (the walk's links: every link but the root)
    sync = (lambda: None) if device == "cpu" else torch.cuda.synchronize
    GUARD = 64
    need = int(lib.drm_link_power_dq_scratch_floats(ctypes.byref(walk), B))
    assert need == int(lib.drm_link_power_dq_scratch_floats_aligned(ctypes.byref(walk), B)) and need >= 0
    scratch = torch.full((need + GUARD,), 3.25, device=device)
    ptr = lambda x: x.data_ptr() if x is not None else None

    def call(a=q, b=qd, ff=f, mm=m, rows=B, targets=T, out=True, want_tau=True):
        dq, tau = (torch.full((B * n + 8,), 7.5, device=device) for _ in range(2))
        rc = lib.drm_link_power_dq(ctypes.byref(walk), ptr(a), ptr(b), ptr(ff), ptr(mm), rows, targets, flags, dq.data_ptr() if out else None,
                                   tau.data_ptr() if want_tau else None, scratch.data_ptr(), stream)
        sync()
        return rc, dq, tau
    rc, dq, tau = call()
    assert rc == 0 and (scratch[need:] == 3.25).all()
    for o in (dq, tau):
        assert (o[B * n:] == 7.5).all() and torch.isfinite(o[:B * n]).all()
    ref = torch.full((B * n + 8,), 7.5, device=device)
    assert lib.drm_external_torques(ctypes.byref(walk), q.data_ptr(), f.data_ptr(), m.data_ptr(), B, T, flags, ref.data_ptr(),
                                    scratch.data_ptr(), stream) == 0
    sync()
    assert torch.equal(tau, ref)
    rc, dq1, tau1 = call(want_tau=False)                           # tau NULL: not stored, dq the same bits
    assert rc == 0 and torch.equal(dq1, dq) and (tau1 == 7.5).all()
    rc, df, _ = call(mm=None)
    rc2, df0, _ = call(mm=torch.zeros_like(m))
    assert rc == rc2 == 0 and torch.equal(df, df0)
    rc, dm, _ = call(ff=None)
    rc2, dm0, _ = call(ff=torch.zeros_like(f))
    assert rc == rc2 == 0 and torch.equal(dm, dm0)
    assert call(a=None)[0] == -1 and call(b=None)[0] == -1 and call(out=False)[0] == -1 and call(ff=None, mm=None)[0] == -1
    assert call(targets=0)[0] == -1 and call(targets=T + 1)[0] == -1 and call(rows=-1)[0] == -1
    rc, d0, t0 = call(rows=0)
    assert rc == 0 and (d0 == 7.5).all() and (t0 == 7.5).all()
    assert (scratch[need:] == 3.25).all()


def test_c_abi_on_the_host_build(cpu_library):
    from differentiable_robot_model_amd import backend
    lib = backend.load_library(kind="cpu")
    assert lib.drm_abi_version() == 15
    assert {"drm_link_power_dq", "drm_link_power_dq_scratch_floats", "drm_link_power_dq_scratch_floats_aligned"} <= set(backend.EXPORTS)
    c_abi_check(lib, model_on("panda_no_gripper"), "cpu", None)
    c_abi_check(lib, model_on("panda_no_gripper"), "cpu", None, flags=1024)


# ------------------------------------------------------------------------------------------------------------------- GPU
def gpu_run_and_check(robot, B, composed=False, compat=True, path=None):
    model = model_on(robot, "cuda:0", compat)
    out = run_model(model, inputs(robot, compat), B=B, composed=composed)
    torch.cuda.synchronize()
    name = path or ("general" if composed or robot not in ARMS or B < 64 else "fused") + "-B%d" % B
    check(robot, name, out, truth(robot, compat))
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 128, 131])
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_against_truth(robot, B):
    model = gpu_run_and_check(robot, B)
    more_checks(model, inputs(robot), B=B)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_general_kernel(robot):
    model = gpu_run_and_check(robot, 128, composed=True)
    more_checks(model, inputs(robot), composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", OTHERS)
def test_gpu_other_robots_against_truth(robot):
    model = gpu_run_and_check(robot, 65)
    more_checks(model, inputs(robot), B=65)


@pytest.mark.gpu
def test_gpu_fetch_with_sliding_joints():
    gpu_run_and_check("fetch", 65, compat=False, path="general-prismatic")


@pytest.mark.gpu
def test_gpu_skew_axis_model(tmp_path_factory):
    skew_check(tmp_path_factory, "cuda:0", "general-B65-prismatic")


@pytest.mark.gpu
def test_gpu_long_chain_keeps_its_records_in_the_scratch(tmp_path):
    from differentiable_robot_model_amd import backend
    model = long_chain_check(tmp_path, "cuda", "general-B65")
    assert backend.load_library().drm_link_power_dq_scratch_floats(ctypes.byref(walk_of(model)[0]), 65) > 0


@pytest.mark.gpu
def test_gpu_subset_of_links_in_the_callers_order():
    subset_check("allegro_left", "cuda:0", "subset")


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_non_finite_rows(composed):
    bad_rows_check(model_on("panda_no_gripper", "cuda:0"), "cuda", composed=composed)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_nan_force_on_one_fingertip():
    nan_wrench_check("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_two_launches_agree_to_the_bit(composed):
    model = model_on("panda_no_gripper", "cuda:0")
    q, qd, _, f, m = (torch.from_numpy(x).cuda() for x in inputs("panda_no_gripper"))
    a, b = launch(model, q, qd, f, m, composed), launch(model, q, qd, f, m, composed)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_gpu_c_abi():
    from differentiable_robot_model_amd import backend
    model = model_on("panda_no_gripper", "cuda:0")
    lib = backend.load_library()
    assert lib.drm_abi_version() == 15
    stream = backend._stream(torch.device("cuda:0"))
    c_abi_check(lib, model, "cuda", stream, B=5)
    c_abi_check(lib, model, "cuda", stream, B=128)
    c_abi_check(lib, model, "cuda", stream, B=128, flags=1024)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7_allegro"])
def test_gpu_c_abi_misaligned_and_guards(robot):
    """Straight through the C ABI: every input and output 4 bytes off a 16-byte boundary (the general kernel), a scratch of exactly the
    queried size with guard words behind it, guard words on both sides of both outputs; the truth within the same bound."""
    from differentiable_robot_model_amd import backend
    model = model_on(robot, "cuda:0")
    lib, (walk, T), n = backend.load_library(), walk_of(model), model._n_dofs
    stream = backend._stream(torch.device("cuda:0"))

    def off_by_4(x):
        buf = torch.zeros(x.numel() + 1, device="cuda")
        buf[1:] = x.reshape(-1)
        view = buf[1:].view(x.shape)
        assert view.data_ptr() % 16 == 4
        return view
    data = inputs(robot)
    q, qd = (off_by_4(torch.from_numpy(x).cuda()) for x in data[:2])
    _, _, sel, identity = model._links_plan(None)
    f, m = (off_by_4(model._links_scatter(torch.from_numpy(x).cuda(), sel, T, identity).contiguous()) for x in data[3:])
    GUARD = 64
    need = int(lib.drm_link_power_dq_scratch_floats(ctypes.byref(walk), ROWS))
    assert need > 0                                     # (8 ops of 21 floats are past the general kernel's LDS budget already)
    sc = torch.full((need + GUARD,), 3.25, device="cuda")
    bufs = [torch.full((1 + ROWS * n + GUARD,), -1.5, device="cuda") for _ in range(2)]
    outs = [b[1:1 + ROWS * n] for b in bufs]
    assert all(o.data_ptr() % 16 == 4 for o in outs)
    rc = lib.drm_link_power_dq(ctypes.byref(walk), q.data_ptr(), qd.data_ptr(), f.data_ptr(), m.data_ptr(), ROWS, T, 0, outs[0].data_ptr(),
                               outs[1].data_ptr(), sc.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0 and (sc[need:] == 3.25).all()
    for b, o in zip(bufs, outs):
        assert (b[1 + o.numel():] == -1.5).all() and b[0] == -1.5
    check(robot, "misaligned", outs[0].view(ROWS, n).clone(), truth(robot))
    ref = model.compute_external_torques(*(torch.from_numpy(x).cuda() for x in (data[0], data[3], data[4])), _composed=True)
    assert torch.equal(outs[1].view(ROWS, n), ref)

"""Batched forward-dynamics rollouts (ABI 14, csrc/drm_rollout.hip: T integration steps per launch;
DifferentiableRobotModel.compute_forward_dynamics_rollout).

CPU (not gpu): the host build (libdrm_cpu.so) against one compute_forward_dynamics call plus the integrator (T = 1), against a
rollout composed from the fp64 oracle (T = 50), against rollouts and gradients of the UNMODIFIED reference for both integrators
(tests/golden/golden_rollout.npz, made by tests/golden/make_golden_rollout.py), gradients against torch autograd through this
package's own per-step loop, and the API.  GPU (-m gpu): the fused arm and finger kernels, the composed path and ragged tails
against the host build and the oracle at the defaults (semi-implicit Euler, gravity, no damping), a full-size Panda launch, the
Panda's gradients and graph capture.

What is NOT here is in test_rollout_edges.py: explicit Euler and the flags on the GPU, qdd_traj, pointers that really are misaligned
and the scratch contract (through the C ABI: the views of check_normalised_views_and_ragged are copied to aligned tensors by the
binding), gradients against fp64 on every path (worst error 2.3 x the float32 yardstick's on the host build, 1.5 x on the MI355X,
8 x allowed), and non-finite rows.
"""
import ctypes

import numpy as np
import pytest
import torch

from differentiable_robot_model_amd import backend
from helpers import ALL_ROBOTS, GOLDEN_DIR, load_model, sample_states
from oracle import Oracle
from test_forward_dynamics import FLAGS, tol_of

import os

INTEGRATORS = ("semi_implicit_euler", "euler")
GOLDEN_ROBOTS = ("panda_no_gripper", "iiwa7", "allegro_left", "fetch_arm_no_gripper")


def composed(model, q0, qd0, tau, dt, integrator="semi_implicit_euler", gravity=True, damping=False):
    """The Python loop the rollout replaces: compute_forward_dynamics per step, then the integrator."""
    q, qd, qs, qds = q0, qd0, [], []
    for t in range(tau.shape[0]):
        qdd = model.compute_forward_dynamics(q, qd, tau[t], include_gravity=gravity, use_damping=damping)
        if integrator == "euler":
            q, qd = q + dt * qd, qd + dt * qdd
        else:
            qd = qd + dt * qdd
            q = q + dt * qd
        qs.append(q)
        qds.append(qd)
    return torch.stack(qs), torch.stack(qds)


def oracle_rollout(model, q0, qd0, tau, dt, integrator, gravity=True, damping=False):
    """fp64 oracle accelerations, fp64 integrator."""
    orc = Oracle(model._spec)
    x, v, qs, qds = np.asarray(q0, np.float64), np.asarray(qd0, np.float64), [], []
    for t in range(tau.shape[0]):
        a = orc.forward_dynamics(x, v, np.asarray(tau[t], np.float64), gravity, damping, np.float64)
        if integrator == "euler":
            x, v = x + dt * v, v + dt * a
        else:
            v = v + dt * a
            x = x + dt * v
        qs.append(x)
        qds.append(v)
    return np.stack(qs), np.stack(qds)


def rel(a, ref):
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    return float((np.abs(a - ref) / (1.0 + np.abs(ref))).max())


def rollout_tol(robot, T, dt):
    """|d| <= tol * (1 + |x|) against the fp64 rollout.  Each step's qdd is within tol_of(robot) * (1 + |qdd|) of fp64
    (test_forward_dynamics); qd integrates T of those errors times dt and q integrates qd's, so the states carry
    T * dt * tol_of(robot) to first order, doubled for the feedback of the state error into later steps.  Calibrated on the
    host build, T = 50, dt = 1e-3, torques of +-0.01 Nm plus gravity: measured at most 1.8e-5 (jaco's qd; its bound 1e-4) and
    4.6e-7 for the arms (bound 1e-5)."""
    return 2.0 * T * dt * tol_of(robot)


def torques(model, T, B, seed=5, scale=0.01):
    rng = np.random.default_rng(seed)
    return rng.uniform(-scale, scale, size=(T, B, model._n_dofs)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_one_step_is_forward_dynamics_plus_integrator(robot):
    m = load_model(robot)
    q, qd, _ = sample_states(m, 9, seed=1)
    q, qd = torch.from_numpy(q), torch.from_numpy(qd)
    tau = torch.from_numpy(torques(m, 1, 9, scale=0.5))
    dt = 1e-3
    for grav, damp in FLAGS:
        qdd = m.compute_forward_dynamics(q, qd, tau[0], include_gravity=bool(grav), use_damping=bool(damp)).double()
        for integ in INTEGRATORS:
            qt, qdt = m.compute_forward_dynamics_rollout(q, qd, tau, dt, integrator=integ, include_gravity=bool(grav),
                                                         use_damping=bool(damp))
            assert qt.shape == (1, 9, m._n_dofs) and qdt.shape == (1, 9, m._n_dofs)
            v1 = qd.double() + dt * qdd
            x1 = q.double() + dt * (qd.double() if integ == "euler" else v1)
            assert rel(qdt[0], v1) < 1e-6, (robot, grav, damp, integ, rel(qdt[0], v1))
            assert rel(qt[0], x1) < 1e-6, (robot, grav, damp, integ, rel(qt[0], x1))


@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_fifty_steps_against_fp64_oracle(robot):
    m = load_model(robot)
    T, dt, B = 50, 1e-3, 16
    q, qd, _ = sample_states(m, B, seed=3)
    tau = torques(m, T, B)
    tol = rollout_tol(robot, T, dt)
    for integ in INTEGRATORS:
        qt, qdt = m.compute_forward_dynamics_rollout(torch.from_numpy(q), torch.from_numpy(qd), torch.from_numpy(tau), dt, integrator=integ)
        xq, xv = oracle_rollout(m, q, qd, tau, dt, integ)
        assert rel(qt.numpy(), xq) <= tol, (robot, integ, rel(qt.numpy(), xq), tol)
        assert rel(qdt.numpy(), xv) <= tol, (robot, integ, rel(qdt.numpy(), xv), tol)


def load_golden_rollout():
    return np.load(os.path.join(GOLDEN_DIR, "golden_rollout.npz"), allow_pickle=False)


@pytest.mark.parametrize("robot", GOLDEN_ROBOTS)
def test_against_reference_rollout(robot):
    g = load_golden_rollout()
    m = load_model(robot)
    dt = float(g["dt"])
    q0, qd0, tau = (torch.from_numpy(g["%s/%s" % (robot, k)].copy()) for k in ("q0", "qd0", "tau"))
    T = tau.shape[0]
    for key, integ, grav in (("semi_g1_d0", "semi_implicit_euler", True), ("euler_g0_d0", "euler", False)):
        qt, qdt = m.compute_forward_dynamics_rollout(q0, qd0, tau, dt, integrator=integ, include_gravity=grav)
        tol = rollout_tol(robot, T, dt)
        assert rel(qt.numpy(), g["%s/%s/q_traj" % (robot, key)]) <= tol, (robot, key)
        assert rel(qdt.numpy(), g["%s/%s/qd_traj" % (robot, key)]) <= tol, (robot, key)


def loss_of(q_traj, qd_traj):
    return (q_traj[-1] ** 2).sum() + 0.1 * (qd_traj ** 2).mean()


def grad_close(a, b, rtol):
    a = np.asarray(a, np.float64).reshape(-1); b = np.asarray(b, np.float64).reshape(-1)
    return np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-12)


def learnable_mass_model(robot, link, l_value, device="cpu"):
    from differentiable_robot_model_amd.rigid_body_params import PositiveScalar
    m = load_model(robot, device)
    mod = PositiveScalar()
    m.make_link_param_learnable(link, "mass", mod)
    with torch.no_grad():
        mod.l.copy_(torch.as_tensor(np.asarray(l_value, np.float32)).reshape(mod.l.shape))
    return m, mod.l


@pytest.mark.parametrize("robot", GOLDEN_ROBOTS)
def test_gradients_against_reference_autograd(robot):
    g = load_golden_rollout()
    dt = float(g["dt"])
    for pre, integ, grav in (("/grad/", "semi_implicit_euler", True), ("/grad_euler_g0_d0/", "euler", False)):
        pre = robot + pre
        m, l = learnable_mass_model(robot, str(g[robot + "/grad/link"]), g[robot + "/grad/l"])
        q0, qd0, tau = (torch.tensor(g["%s/%s" % (robot, k)], requires_grad=True) for k in ("q0", "qd0", "tau"))
        qt, qdt = m.compute_forward_dynamics_rollout(q0, qd0, tau, dt, integrator=integ, include_gravity=grav)
        loss = loss_of(qt, qdt)
        assert abs(loss.item() - float(g[pre + "loss"])) <= 1e-4 * abs(float(g[pre + "loss"]))
        loss.backward()
        rtol = 1e-3 if robot in ("panda_no_gripper", "iiwa7") else 1e-2
        assert grad_close(q0.grad, g[pre + "q0"], rtol), (robot, integ)
        assert grad_close(qd0.grad, g[pre + "qd0"], rtol), (robot, integ)
        assert grad_close(tau.grad, g[pre + "tau"], rtol), (robot, integ)
        ref = g[pre + "l_grad"]
        assert abs(float(l.grad) - float(ref)) <= rtol * max(abs(float(ref)), 1e-3 * np.abs(g[pre + "tau"]).max()), (integ, float(l.grad), float(ref))


def _grads_through(m, fn, q0, qd0, tau, params):
    leaves = [t.clone().requires_grad_(True) for t in (q0, qd0, tau)]
    qt, qdt = fn(m, *leaves)
    loss = loss_of(qt, qdt)
    got = torch.autograd.grad(loss, leaves + list(params))
    return [x.detach().cpu().numpy() for x in got]


@pytest.mark.parametrize("robot,learn", [("panda_no_gripper", None), ("iiwa7", "iiwa_link_3"), ("allegro_left", None),
                                         ("fetch_arm_no_gripper", "shoulder_lift_link")])
def test_gradients_against_own_per_step_loop(robot, learn):
    if learn:
        m, l = learnable_mass_model(robot, learn, 1.1)
        params = [l]
    else:
        m, params = load_model(robot), []
    T, B, dt = 12, 5, 2e-3
    q, qd, _ = sample_states(m, B, seed=4)
    tau = torch.from_numpy(torques(m, T, B, scale=0.05))
    damp = robot in ("panda_no_gripper", "iiwa7")     # (the shipped hand's and Fetch's joint damping is too stiff for an Euler step)
    for integ in INTEGRATORS:
        got = _grads_through(m, lambda mm, a, b, c: mm.compute_forward_dynamics_rollout(a, b, c, dt, integrator=integ, use_damping=damp),
                             torch.from_numpy(q), torch.from_numpy(qd), tau, params)
        want = _grads_through(m, lambda mm, a, b, c: composed(mm, a, b, c, dt, integ, damping=damp), torch.from_numpy(q),
                              torch.from_numpy(qd), tau, params)
        assert all(np.isfinite(y).all() for y in want)
        for x, y in zip(got, want):
            assert grad_close(x, y, 1e-3), (robot, integ, np.abs(x - y).max(), np.abs(y).max())


def test_unbatched_shapes_and_tau_untouched():
    m = load_model("panda_no_gripper")
    q, qd, _ = sample_states(m, 1)
    tau = torch.from_numpy(torques(m, 6, 1, scale=1.0)[:, 0])
    keep = tau.clone()
    qt, qdt = m.compute_forward_dynamics_rollout(torch.from_numpy(q[0]), torch.from_numpy(qd[0]), tau, 1e-3, use_damping=True)
    assert qt.shape == (6, 7) and qdt.shape == (6, 7)
    assert torch.equal(tau, keep)
    qb, qdb = m.compute_forward_dynamics_rollout(torch.from_numpy(q), torch.from_numpy(qd), tau[:, None], 1e-3, use_damping=True)
    assert torch.equal(qb[:, 0], qt) and torch.equal(qdb[:, 0], qdt)


def test_refusals():
    m = load_model("iiwa7")
    q, qd, _ = sample_states(m, 4)
    q, qd = torch.from_numpy(q), torch.from_numpy(qd)
    tau = torch.from_numpy(torques(m, 3, 4))
    with pytest.raises(ValueError):
        m.compute_forward_dynamics_rollout(q, qd, tau, 1e-3, integrator="rk4")
    with pytest.raises(ValueError):
        m.compute_forward_dynamics_rollout(q, qd, tau[:0], 1e-3)
    for dt in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            m.compute_forward_dynamics_rollout(q, qd, tau, dt)
    with pytest.raises(AssertionError):
        m.compute_forward_dynamics_rollout(q, qd, tau[:, :3], 1e-3)          # batch mismatch
    with pytest.raises(AssertionError):
        m.compute_forward_dynamics_rollout(q, qd, tau[0], 1e-3)              # tau must carry the time axis
    with pytest.raises(AssertionError):
        m.compute_forward_dynamics_rollout(q[:, :6], qd[:, :6], tau[..., :6], 1e-3)
    if torch.cuda.is_available():
        with pytest.raises(AssertionError):
            m.compute_forward_dynamics_rollout(q.cuda(), qd, tau, 1e-3)
    else:
        with pytest.raises(AssertionError):
            m.compute_forward_dynamics_rollout(q.to("meta"), qd, tau, 1e-3)


def test_c_abi_refusals(cpu_library):
    lib = cpu_library
    m = load_model("iiwa7")
    dw = m._dynamics_walk()
    ops_f = m._ops_f(dw)
    walk = backend._walk_struct(dw.program, ops_f, dw.ops_i, 7)
    x = torch.zeros(4, 7)
    out = torch.zeros(2, 4, 7)
    p = lambda t: t.data_ptr()
    for T, dt in ((0, 1e-3), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        rc = lib.drm_forward_dynamics_rollout(ctypes.byref(walk), p(x), p(x), p(out), 4, T, dt, 1, p(out), p(out), None, None, None)
        assert rc == -1, (T, dt)
    assert lib.drm_forward_dynamics_rollout(ctypes.byref(walk), p(x), p(x), p(out), 0, 2, 1e-3, 1, p(out), p(out), None, None, None) == 0


def test_double_backward_raises():
    m = load_model("panda_no_gripper")
    q, qd, _ = sample_states(m, 3)
    q = torch.from_numpy(q).requires_grad_(True)
    tau = torch.from_numpy(torques(m, 4, 3))
    qt, qdt = m.compute_forward_dynamics_rollout(q, torch.from_numpy(qd), tau, 1e-3)
    (gq,) = torch.autograd.grad(loss_of(qt, qdt), q, create_graph=True)
    want = _grads_through(m, lambda mm, a, b, c: composed(mm, a, b, c, 1e-3), q.detach(), torch.from_numpy(qd), tau, [])[0]
    assert grad_close(gq.detach().numpy(), want, 1e-3)          # a correct first-order gradient
    with pytest.raises(NotImplementedError, match="compute_forward_dynamics"):
        gq.sum().backward()


def _backend_rollout(m, q0, qd0, tau, dt, explicit=False, want_qdd=True):
    dw = m._dynamics_walk()
    return backend.forward_dynamics_rollout(dw.program, m._ops_f(dw), dw.ops_i, q0, qd0, tau, dt, True, False, explicit, m._n_dofs,
                                            want_qdd=want_qdd)


def check_normalised_views_and_ragged(device):
    """Row slices that backend._dev_f32 copies to aligned tensors, and B % 64 != 0, against the aligned, full-tile call at the backend
    level (rows are independent).  The C side never sees a misaligned pointer here: test_rollout_edges.py hands it some."""
    for robot in ("panda_no_gripper", "allegro_left", "fetch_arm_no_gripper", "iiwa7_allegro"):
        m = load_model(robot, device)
        n, T, B = m._n_dofs, 5, 128
        q, qd, _ = sample_states(m, B + 1, seed=8)
        tau = torques(m, T, B + 1, scale=0.05)
        full = _backend_rollout(m, torch.from_numpy(q[:B]).to(device), torch.from_numpy(qd[:B]).to(device),
                                torch.from_numpy(np.ascontiguousarray(tau[:, :B])).to(device), 1e-3)
        # rows 1 .. B of a [B + 1, n] tensor: a slice whose data pointer is off a 16-byte boundary (n = 7), and a non-contiguous
        # slice of tau: the binding clones the first and .reshape copies the second
        qs, qds = torch.from_numpy(np.concatenate([q[-1:], q[:B]])).to(device)[1:], torch.from_numpy(np.concatenate([qd[-1:], qd[:B]])).to(device)[1:]
        ts = torch.from_numpy(np.concatenate([tau[:, -1:], tau[:, :B]], axis=1)).to(device)[:, 1:]
        mis = _backend_rollout(m, qs, qds, ts, 1e-3)
        # (on the GPU a ragged tail runs other kernels than the full aligned tiles: their rows agree to the rounding of the two
        # kernels, within twice the rollout tolerance; the host build computes every row the same way)
        tol = 2 * rollout_tol(robot, 8, 1e-3) if device != "cpu" else 0.0
        for a, b in zip(full[:2], mis[:2]):
            assert rel(b.cpu(), a.cpu()) <= tol, (robot, rel(b.cpu(), a.cpu()))
        for rows in (1, 63, 65, 100):
            part = _backend_rollout(m, torch.from_numpy(q[:rows]).to(device), torch.from_numpy(qd[:rows]).to(device),
                                    torch.from_numpy(np.ascontiguousarray(tau[:, :rows])).to(device), 1e-3)
            for a, b in zip(full[:2], part[:2]):
                assert rel(b.cpu(), a[:, :rows].cpu()) <= tol, (robot, rows, rel(b.cpu(), a[:, :rows].cpu()))


def test_normalised_views_and_ragged_cpu():
    check_normalised_views_and_ragged("cpu")


# ---------------------------------------------------------------------------------------------------------------------- GPU

def _gpu_model(robot, own=None):
    m = load_model(robot, "cuda:0")
    if own is not None:
        m.own_kernels = own
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ALL_ROBOTS)
@pytest.mark.parametrize("own", [None, "off"])
def test_gpu_against_host_and_oracle(robot, own):
    cpu = load_model(robot)
    gpu = _gpu_model(robot, own)
    dt = 1e-3
    for B in (1, 63, 64, 65, 257, 4096):
        q, qd, _ = sample_states(cpu, B, seed=B)
        for T in (1, 7, 64):
            tau = torques(cpu, T, B, seed=T)
            want_q, want_qd = cpu.compute_forward_dynamics_rollout(torch.from_numpy(q), torch.from_numpy(qd), torch.from_numpy(tau), dt)
            got_q, got_qd = gpu.compute_forward_dynamics_rollout(torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda(),
                                                                 torch.from_numpy(tau).cuda(), dt)
            got_q, got_qd = got_q.cpu().numpy(), got_qd.cpu().numpy()
            tol = rollout_tol(robot, max(T, 8), dt)
            assert np.isfinite(got_q).all() and np.isfinite(got_qd).all()
            # (each build is within tol of the fp64 rollout: the two are within twice that of each other)
            assert rel(got_q, want_q.numpy()) <= 2 * tol and rel(got_qd, want_qd.numpy()) <= 2 * tol, (robot, own, B, T)
            if B in (65, 4096) and T == 64:
                k = min(B, 64)
                xq, xv = oracle_rollout(cpu, q[:k], qd[:k], tau[:, :k], dt, "semi_implicit_euler")
                assert rel(got_q[:, :k], xq) <= tol and rel(got_qd[:, :k], xv) <= tol, (robot, own, B, T)


@pytest.mark.gpu
def test_gpu_full_size_panda():
    gpu = load_model("panda_no_gripper", "cuda:0")
    B, T, dt = 65536, 32, 1e-3
    q, qd, _ = sample_states(gpu, B, seed=2)
    tau = torch.from_numpy(torques(gpu, T, B, scale=1.0)).cuda()
    q, qd = torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()
    got_q, got_qd = gpu.compute_forward_dynamics_rollout(q, qd, tau, dt)
    with torch.no_grad():
        want_q, want_qd = composed(gpu, q, qd, tau, dt)
    assert torch.isfinite(got_q).all() and torch.isfinite(got_qd).all()
    tol = rollout_tol("panda_no_gripper", T, dt)
    assert rel(got_q.cpu(), want_q.cpu()) <= tol and rel(got_qd.cpu(), want_qd.cpu()) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("learn", [None, "panda_link3"])
def test_gpu_gradients_against_cpu(learn):
    T, B, dt = 10, 70, 2e-3
    grads = []
    for device in ("cpu", "cuda:0"):
        if learn:
            from differentiable_robot_model_amd.rigid_body_params import UnconstrainedTensor
            m, l = learnable_mass_model("panda_no_gripper", learn, 1.1, device)
            com = UnconstrainedTensor(dim1=1, dim2=3)
            m.make_link_param_learnable(learn, "com", com)
            with torch.no_grad():
                com.param.copy_(torch.tensor([[0.01, -0.02, 0.03]]).reshape(com.param.shape))
            params = [l, com.param]
        else:
            m, params = load_model("panda_no_gripper", device), []
        q, qd, _ = sample_states(m, B, seed=6)
        tau = torch.from_numpy(torques(m, T, B, scale=1.0)).to(device)
        grads.append(_grads_through(m, lambda mm, a, b, c: mm.compute_forward_dynamics_rollout(a, b, c, dt, use_damping=True),
                                    torch.from_numpy(q).to(device), torch.from_numpy(qd).to(device), tau, params))
    for x, y in zip(grads[1], grads[0]):
        assert grad_close(x, y, 2e-3), (learn, np.abs(x - y).max(), np.abs(y).max())


@pytest.mark.gpu
def test_gpu_graph_capture_bit_equal():
    m = load_model("panda_no_gripper", "cuda:0")
    B, T, dt = 256, 8, 1e-3
    q, qd, _ = sample_states(m, B, seed=9)
    q, qd = torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()
    tau = torch.from_numpy(torques(m, T, B, scale=1.0)).cuda()
    eager = m.compute_forward_dynamics_rollout(q, qd, tau, dt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.compute_forward_dynamics_rollout(q, qd, tau, dt)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = m.compute_forward_dynamics_rollout(q, qd, tau, dt)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])


@pytest.mark.gpu
def test_gpu_normalised_views_and_ragged():
    check_normalised_views_and_ragged("cuda:0")

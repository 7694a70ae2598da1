"""Forward-dynamics rollouts (ABI 14, csrc/drm_rollout.hip, autograd._ForwardDynamicsRollout) held to fp64 on every path, integrator,
flag and gradient.

test_rollout.py pins the rollout at its defaults; this file pins what a subtly wrong kernel, scratch size or reverse sweep could still
get away with there.  Every check is one function of the device: it runs un-marked on the host build and under -m gpu on cuda:0, where
the three forward paths are the fused arm kernel (Panda, iiwa7), the fused fingers kernel (Allegro) and the composed per-step path
(every other robot, ragged tails, misaligned pointers).

  A  forward, GPU: path x integrator x (gravity, damping) x B in {64, 65, 129} x T in {1, 2, 9} against the host build
     (2 rollout_tol) and, at T = 9, against the fp64 oracle's rollout (rollout_tol): the rule of test_rollout.py
  B  qdd_traj[t] = the fp64 oracle's forward dynamics at the call's own previous state, within tol_of(robot) (1 + |qdd|); asking for
     qdd_traj changes no bit of q_traj, qd_traj
  C  pointers that are NOT 16-byte aligned (asserted), straight through the C ABI: the binding would copy them to aligned tensors.
     Every C call gets a scratch of exactly the queried size plus 64 guard words, which must survive
  D  gradients of L = sum Wq q_traj + sum Wv qd_traj against fp64 central differences (h = 1e-5) of the oracle's fp64 rollout.
     The integrator's identity dominates dL/dq0 and dL/dqd0, so the metric removes it:
         err(g) = max|g - g64| / max|g64 - g_kin|,   g_kin: the closed-form fp64 gradient of the same loss with qdd = 0.
     Yardstick (not code under test): the reverse sweep of _ForwardDynamicsRollout's docstring in float32 numpy, its per-step Jacobians
     yardstick (a) of test_fd_derivatives.build_problem (float32 LAPACK on fp64-differenced dID/dq, dID/dqd and the oracle's float32 H)
     at the fp64 trajectory's states.  REQUIREMENT for dL/dq0, dL/dqd0, dL/dtau:
         err(path) <= 8 max(err(yardstick), 2^-23 max|g64| / max|g64 - g_kin|)
     8 is test_fd_derivatives.MARGIN; the floor is float32's resolution of g itself in the metric's unit.
  E  a NaN in q0 of row 5 and an Inf in tau[3] of row 70 change no bit of any other row (nor of another finger of row 5)

Torques are U(+-0.01) Nm (test_rollout.torques).  use_damping is exercised only where an Euler step of the case's dt is stable
(damping_ok): the shipped Allegro's and Fetch's joint damping is too stiff for any dt used here, and the fp64 rollout itself
overflows.  Measured with the fp64 oracle, max|qd| from 1 rad/s: allegro_left_small_damping grows 17-fold PER STEP at dt = 1e-3 (1e39
after 9 steps), so it takes damping in rollouts of at most 3 steps only; fetch_arm_no_gripper_small_damping is stable at dt <= 2e-3
and reaches 4e4 rad/s after 8 steps of 5e-3; iiwa7 and 2link_robot are stable throughout.  The Panda has no joint damping.

Every comparison of C and D prints one "ROLLEDGE" line (check, robot, integrator, flags, path, array, error, yardstick or bound) before
it asserts; profiles/rollout_edge_tests.txt holds them for the host build and the MI355X.  Measured there: the worst
err(path) / yardstick of D is 2.3 on the host build (Fetch arm, dL/dqd0, semi-implicit, g0 d0) and 1.5 on the MI355X (Fetch arm,
composed tail, dL/dq0, semi-implicit, g1 d1).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from differentiable_robot_model_amd import backend
from helpers import load_model, sample_states
from oracle import Oracle
from test_fd_derivatives import FD_H, FLOOR, MARGIN, build_problem
from test_forward_dynamics import tol_of
from test_rollout import (INTEGRATORS, _grads_through, grad_close, learnable_mass_model, oracle_rollout, rel, rollout_tol,
                          torques)

GPU = "cuda:0"
ALL_FLAGS = ((1, 0), (1, 1), (0, 0), (0, 1))
GRAD_FLAGS = ((1, 0), (0, 0), (1, 1))
ARMS7 = ("panda_no_gripper", "iiwa7")
# (robot, own_kernels) of the forward checks on the GPU
FORWARD_GPU = [("panda_no_gripper", None), ("panda_no_gripper", "off"), ("iiwa7", None), ("allegro_left_small_damping", None),
               ("fetch_arm_no_gripper_small_damping", None), ("iiwa7_allegro", None)]
C_ABI_ROBOTS = ("panda_no_gripper", "allegro_left", "fetch_arm_no_gripper")
FILL, SENTINEL, GUARD = -7.0, 12345.0, 64


@functools.lru_cache(maxsize=None)
def model(robot, dev="cpu", own=None):
    m = load_model(robot, dev)
    if own is not None:
        m.own_kernels = own
    return m


def damping_ok(robot, T, dt, panda=False):
    """Is an Euler rollout of T steps of dt with use_damping=True stable for this robot (module docstring)?  panda: count the Panda,
    whose URDF has no joint damping, so that the flag must change nothing"""
    if robot in ("iiwa7", "2link_robot"):
        return True
    if robot == "fetch_arm_no_gripper_small_damping":
        return dt <= 2e-3
    if robot == "allegro_left_small_damping":
        return dt <= 1e-3 and T <= 3
    return panda and robot == "panda_no_gripper"


def flags_of(robot, sets, T, dt, panda=False):
    return [f for f in sets if not f[1] or damping_ok(robot, T, dt, panda)]


def path_name(robot, dev, misaligned=False, own=None):
    if dev == "cpu":
        return "host"
    tag = "" if own is None else "-own-" + own
    if robot in ARMS7:
        return ("gpu-composed" if misaligned else "gpu-arm") + tag
    return ("gpu-fingers" if robot.startswith("allegro") else "gpu-composed") + tag


def report(check, robot, integ, flags, path, array, value, other):
    print("ROLLEDGE %-10s %-34s %-5s g%d d%d %-21s %-8s %.3e  %.3e" % (check, robot, "euler" if integ == "euler" else "semi",
                                                                     flags[0], flags[1], path, array, value, other))


def to(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


# ------------------------------------------------------------------------------------------------------------------- section A


@pytest.mark.gpu
@pytest.mark.parametrize("robot,own", FORWARD_GPU, ids=lambda v: str(v))
def test_gpu_forward_every_path_integrator_flag(robot, own):
    """B = 64: a full tile; 65: a tile and one tail row; 129: two tiles and a tail.  T = 1 never prefetches, T = 2 is the first reuse
    of the parking area and of the prefetched torques; at T = 9 with B = 65 or 129 the slabs of t >= 1 start off a 16-byte boundary
    for n = 7 (B n % 4 != 0)."""
    cpu, gpu = model(robot), model(robot, GPU, own)
    dt, worst = 1e-3, 0.0
    for B in (64, 65, 129):
        q, qd, _ = sample_states(cpu, B, seed=B)
        for T in (1, 2, 9):
            tau = torques(cpu, T, B, seed=T)
            host_in, gpu_in = to("cpu", q, qd, tau), to(GPU, q, qd, tau)
            tol = rollout_tol(robot, max(T, 8), dt)
            for integ in INTEGRATORS:
                for g, d in flags_of(robot, ALL_FLAGS, T, dt, panda=True):
                    kw = dict(integrator=integ, include_gravity=bool(g), use_damping=bool(d))
                    want = [x.numpy() for x in cpu.compute_forward_dynamics_rollout(*host_in, dt, **kw)]
                    got = [x.cpu().numpy() for x in gpu.compute_forward_dynamics_rollout(*gpu_in, dt, **kw)]
                    assert all(x.shape == (T, B, cpu._n_dofs) and np.isfinite(x).all() for x in got)
                    e = max(rel(got[0], want[0]), rel(got[1], want[1]))
                    worst = max(worst, e / (2 * tol))
                    assert e <= 2 * tol, (robot, own, B, T, integ, g, d, e, 2 * tol)
                    if T == 9:
                        xq, xv = oracle_rollout(cpu, q, qd, tau, dt, integ, bool(g), bool(d))
                        e = max(rel(got[0], xq), rel(got[1], xv))
                        worst = max(worst, e / tol)
                        assert e <= tol, (robot, own, B, T, integ, g, d, e, tol)
    print("ROLLEDGE forward    %-34s own=%s worst error / bound %.3f" % (robot, own, worst))


# ------------------------------------------------------------------------------------------------------------------- section B


def backend_rollout(m, q0, qd0, tau, dt, gravity, damping, explicit, want_qdd):
    dw = m._dynamics_walk()
    return backend.forward_dynamics_rollout(dw.program, m._ops_f(dw), dw.ops_i, q0, qd0, tau, dt, bool(gravity), bool(damping),
                                            bool(explicit), m._n_dofs, want_qdd=want_qdd)


def check_qdd_traj(robot, dev, own=None):
    """B = 129: two tiles and a tail row (n = 7: 4-byte stores of the staged tile); B = 64: one tile, 16-byte stores."""
    cpu, m = model(robot), model(robot, dev, own)
    orc = Oracle(cpu._spec)
    dt, T, f64 = 1e-3, 3, np.float64
    for B in (129, 64):
        q, qd, _ = sample_states(cpu, B, seed=12)
        tau = torques(cpu, T, B, seed=13)
        dev_in = to(dev, q, qd, tau)
        for integ in INTEGRATORS:
            for g, d in flags_of(robot, ((1, 0), (1, 1)), T, dt, panda=True):
                plain = backend_rollout(m, *dev_in, dt, g, d, integ == "euler", False)
                full = backend_rollout(m, *dev_in, dt, g, d, integ == "euler", True)
                assert plain[2] is None and full[2].shape == (T, B, cpu._n_dofs)
                assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1]), (robot, B, integ, g, d)
                qt, qdt, qddt = (x.cpu().numpy() for x in full)
                worst = 0.0
                for t in range(T):
                    x, v = (q, qd) if t == 0 else (qt[t - 1], qdt[t - 1])
                    want = orc.forward_dynamics(x.astype(f64), v.astype(f64), tau[t].astype(f64), bool(g), bool(d), f64)
                    worst = max(worst, float((np.abs(qddt[t] - want) / (1.0 + np.abs(want))).max()))
                report("qdd_traj", robot, integ, (g, d), path_name(robot, dev, own=own) + "-B%d" % B, "qdd", worst, tol_of(robot))
                assert worst <= tol_of(robot), (robot, B, integ, g, d, worst)


QDD_ROBOTS = [r for r, own in FORWARD_GPU if own is None]


@pytest.mark.parametrize("robot", QDD_ROBOTS)
def test_qdd_traj_against_fp64(cpu_library, robot):
    check_qdd_traj(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot,own", FORWARD_GPU, ids=lambda v: str(v))
def test_gpu_qdd_traj_against_fp64(robot, own):
    check_qdd_traj(robot, GPU, own)


# ------------------------------------------------------------------------------------------------------------------- section C


def place(values, dev, misaligned):
    """(flat, view): a contiguous copy of `values` inside a flat buffer of FILL one float longer, at the buffer's 16-byte aligned start
    or ([1:]) four bytes past it"""
    flat = torch.full((values.numel() + 1,), FILL, device=dev, dtype=values.dtype)
    view = (flat[1:] if misaligned else flat[:-1]).view(values.shape)
    view.copy_(values)
    assert flat.data_ptr() % 16 == 0 and view.is_contiguous()
    return flat, view


def c_rollout(robot, dev, q0, qd0, tau, dt, integ, flags, misaligned):
    """drm_forward_dynamics_rollout straight through the C ABI, every tensor aligned or every tensor misaligned (asserted), the scratch
    sized by the query that goes with that and followed by GUARD sentinel words.  -> (q_traj, qd_traj) on the CPU"""
    m = model(robot, dev)
    device = torch.device(dev)
    lib = backend.library_for(device)
    dw = m._dynamics_walk()
    ops_f = m._ops_f(dw).detach()
    walk = backend._walk_struct(dw.program, ops_f, dw.ops_i, m._n_dofs)
    T, B, n = tau.shape
    ins = [place(t, dev, misaligned) for t in to("cpu", q0, qd0, tau)]
    outs = [place(torch.full((T, B, n), FILL), dev, misaligned) for _ in range(2)]
    for _, v in ins + outs:
        assert (v.data_ptr() % 16 != 0) == misaligned
    need = int(lib.drm_forward_dynamics_rollout_scratch_floats(ctypes.byref(walk), B))
    need_aligned = int(lib.drm_forward_dynamics_rollout_scratch_floats_aligned(ctypes.byref(walk), B))
    assert 0 <= need_aligned <= need, (need_aligned, need)
    size = need if misaligned else need_aligned
    scratch = None
    if device.type == "cuda":
        fused = path_name(robot, dev, misaligned) in ("gpu-arm", "gpu-fingers")
        if B % 64 or not fused:         # (rollout_composed runs, and qdd_traj is NULL: the accelerations go to the scratch)
            assert size > 0, (robot, B, misaligned)
        scratch = torch.full((size + GUARD,), SENTINEL, device=dev)
    else:
        assert need == 0 and need_aligned == 0
    fl = ((backend.RNEA_GRAVITY if flags[0] else 0) | (backend.RNEA_DAMPING if flags[1] else 0) |
          (backend.ROLLOUT_EXPLICIT_EULER if integ == "euler" else 0))
    rc = lib.drm_forward_dynamics_rollout(ctypes.byref(walk), ins[0][1].data_ptr(), ins[1][1].data_ptr(), ins[2][1].data_ptr(), B, T,
                                          float(dt), fl, outs[0][1].data_ptr(), outs[1][1].data_ptr(), None,
                                          scratch.data_ptr() if scratch is not None else None, backend._stream(device))
    assert rc == 0, lib.drm_last_error()
    if scratch is not None:
        torch.cuda.synchronize()
        assert bool((scratch[size:] == SENTINEL).all()), (robot, B, misaligned, "the call wrote past its scratch")
    for (flat, view), src in zip(ins, (q0, qd0, tau)):          # (the inputs are read only)
        assert np.array_equal(view.cpu().numpy(), src)
    for flat, _ in outs:                                        # (the float in front of / behind the output keeps its fill value)
        assert float(flat[0 if misaligned else -1]) == FILL
    return [v.cpu().numpy().copy() for _, v in outs]


def check_misaligned(robot, dev):
    cpu, m = model(robot), model(robot, dev)
    B, T, dt, flags = 129, 5, 1e-3, (1, 0)
    q, qd, _ = sample_states(cpu, B, seed=8)
    tau = torques(cpu, T, B, seed=9)
    tol = 2 * rollout_tol(robot, 8, dt) if dev != "cpu" else 0.0
    for integ in INTEGRATORS:
        aligned = c_rollout(robot, dev, q, qd, tau, dt, integ, flags, False)
        mis = c_rollout(robot, dev, q, qd, tau, dt, integ, flags, True)
        api = [x.cpu().numpy() for x in m.compute_forward_dynamics_rollout(*to(dev, q, qd, tau), dt, integrator=integ)]
        for name, a, b, c in zip(("q_traj", "qd_traj"), aligned, mis, api):
            assert np.array_equal(a, c), (robot, integ, name)       # (the aligned C call is the binding's call)
            e = rel(b, a)
            report("misaligned", robot, integ, flags, path_name(robot, dev, True), name, e, tol)
            assert np.isfinite(b).all() and e <= tol, (robot, integ, name, e, tol)
            if dev != "cpu" and robot in ARMS7:
                # an arm at misaligned pointers takes the composed path on every row, as the tail row (128) of the aligned call
                # does: the same kernels on the same values
                assert np.array_equal(b[:, 128], a[:, 128]), (robot, integ, name)


def check_scratch_small(robot, dev):
    """B = 1 and 63: no full tile, every row on the composed path whatever the alignment"""
    cpu, m = model(robot), model(robot, dev)
    T, dt, flags, integ = 2, 1e-3, (1, 0), "semi_implicit_euler"
    tol = 2 * rollout_tol(robot, 8, dt) if dev != "cpu" else 0.0
    for B in (1, 63):
        q, qd, _ = sample_states(cpu, B, seed=10)
        tau = torques(cpu, T, B, seed=11)
        api = [x.cpu().numpy() for x in m.compute_forward_dynamics_rollout(*to(dev, q, qd, tau), dt)]
        for misaligned in (False, True):
            got = c_rollout(robot, dev, q, qd, tau, dt, integ, flags, misaligned)
            for name, a, b in zip(("q_traj", "qd_traj"), api, got):
                e = rel(b, a)
                report("scratch-B%d" % B, robot, integ, flags, "misaligned" if misaligned else "aligned", name, e, tol)
                assert e <= tol, (robot, B, misaligned, name, e, tol)


@pytest.mark.parametrize("robot", C_ABI_ROBOTS)
def test_misaligned_pointers_through_the_c_abi(cpu_library, robot):
    check_misaligned(robot, "cpu")
    check_scratch_small(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", C_ABI_ROBOTS)
def test_gpu_misaligned_pointers_through_the_c_abi(robot):
    """Panda: aligned16 false sends every row to the composed path; Allegro: the fingers kernel with vec = 0 and a composed tail row;
    Fetch arm: the composed path at misaligned slabs."""
    check_misaligned(robot, GPU)
    check_scratch_small(robot, GPU)


# ------------------------------------------------------------------------------------------------------------------- section D

ARRAYS = ("dL/dq0", "dL/dqd0", "dL/dtau")


def fp64_gradients(cpu, q0, qd0, tau, Wq, Wv, dt, integ, g, d):
    """Central differences (h = FD_H) of the per-row loss of the fp64 rollout.  Rows are independent: entry j of all B rows is perturbed
    at once, and all 2 n (2 + T) perturbed batches are rows of ONE fp64 rollout.  -> (dL/dq0 [B, n], dL/dqd0 [B, n], dL/dtau [T, B, n])"""
    T, B, n = tau.shape
    z = np.concatenate([q0, qd0, tau.transpose(1, 0, 2).reshape(B, T * n)], 1).astype(np.float64)
    P = z.shape[1]
    zz = np.broadcast_to(z, (2, P, B, P)).copy()
    idx = np.arange(P)
    zz[0, idx, :, idx] += FD_H
    zz[1, idx, :, idx] -= FD_H
    zz = zz.reshape(2 * P * B, P)
    tt = np.ascontiguousarray(zz[:, 2 * n:].reshape(-1, T, n).transpose(1, 0, 2))
    qs, qds = oracle_rollout(cpu, zz[:, :n], zz[:, n:2 * n], tt, dt, integ, bool(g), bool(d))
    assert np.isfinite(qs).all() and np.isfinite(qds).all()
    rows = lambda W: np.tile(W.astype(np.float64), (1, 2 * P, 1))             # (row r of the rollout is row r % B of the problem)
    loss = ((rows(Wq) * qs).sum((0, 2)) + (rows(Wv) * qds).sum((0, 2))).reshape(2, P, B)
    grad = ((loss[0] - loss[1]) / (2 * FD_H)).T
    return grad[:, :n], grad[:, n:2 * n], grad[:, 2 * n:].reshape(B, T, n).transpose(1, 0, 2)


def kinematic_gradients(Wq, Wv, dt):
    """The closed-form fp64 gradient of the loss with qdd = 0 (either integrator: q_T = q0 + T dt qd0, qd_T = qd0)"""
    Q = np.zeros(Wq.shape[1:], np.float64)
    V = np.zeros_like(Q)
    for t in range(Wq.shape[0] - 1, -1, -1):
        Q = Q + Wq[t]
        V = V + Wv[t]
        V = V + dt * Q
    return Q, V, np.zeros(Wq.shape, np.float64)


def yardstick_gradients(cpu, q0, qd0, tau, Wq, Wv, dt, integ, g, d):
    """The reverse sweep of _ForwardDynamicsRollout's docstring in float32 numpy; per-step Jacobians: yardstick (a) of
    test_fd_derivatives.build_problem at the states of the fp64 trajectory"""
    T, B, n = tau.shape
    qs, qds = oracle_rollout(cpu, q0, qd0, tau, dt, integ, bool(g), bool(d))
    xq = np.concatenate([q0[None].astype(np.float64), qs[:-1]]).reshape(T * B, n)
    xv = np.concatenate([qd0[None].astype(np.float64), qds[:-1]]).reshape(T * B, n)
    p = build_problem(Oracle(cpu._spec), (xq, xv, tau.reshape(T * B, n)), bool(g), bool(d))
    Jq, Jv, Mi = (y.reshape(T, B, n, n) for y in p["yard"])
    f32 = np.float32
    h = f32(dt)
    Q = np.zeros((B, n), f32)
    V = np.zeros((B, n), f32)
    gtau = np.empty((T, B, n), f32)
    vjp = lambda A, J: np.einsum("bi,bij->bj", A, J)
    for t in range(T - 1, -1, -1):
        Q = Q + Wq[t]
        V = V + Wv[t]
        if integ == "euler":
            A = h * V
            V = V + h * Q
        else:
            V = V + h * Q
            A = h * V
        Q = Q + vjp(A, Jq[t])
        V = V + vjp(A, Jv[t])
        gtau[t] = vjp(A, Mi[t])
    assert Q.dtype == f32 and V.dtype == f32
    return Q, V, gtau


def path_gradients(m, dev, q0, qd0, tau, Wq, Wv, dt, integ, g, d):
    leaves = [t.requires_grad_(True) for t in to(dev, q0, qd0, tau)]
    qt, qdt = m.compute_forward_dynamics_rollout(*leaves, dt, integrator=integ, include_gravity=bool(g), use_damping=bool(d))
    wq, wv = to(dev, Wq, Wv)
    loss = (wq * qt).sum() + (wv * qdt).sum()
    return [x.detach().cpu().numpy() for x in torch.autograd.grad(loss, leaves)]


def check_gradients(robot, dev, integ, flags, B, T, dt, rows, paths):
    """One launch of B rows; truth and yardstick over `rows` (a list of index arrays, reported separately under `paths`).
    -> the worst err(path) / max(err(yardstick), floor)"""
    cpu, m = model(robot), model(robot, dev)
    n = cpu._n_dofs
    q0, qd0, _ = sample_states(cpu, B, seed=21)
    tau = torques(cpu, T, B, seed=22)
    rng = np.random.default_rng(23)
    Wq, Wv = (rng.uniform(-1.0, 1.0, size=(T, B, n)).astype(np.float32) for _ in range(2))
    g, d = flags
    got = path_gradients(m, dev, q0, qd0, tau, Wq, Wv, dt, integ, g, d)
    bad, worst = [], 0.0
    for sel, path in zip(rows, paths):
        args = (cpu, q0[sel], qd0[sel], tau[:, sel], Wq[:, sel], Wv[:, sel], dt, integ, g, d)
        truth, yard = fp64_gradients(*args), yardstick_gradients(*args)
        kin = kinematic_gradients(Wq[:, sel].astype(np.float64), Wv[:, sel].astype(np.float64), dt)
        for k, name in enumerate(ARRAYS):
            g64 = truth[k]
            mine = got[k][sel] if k < 2 else got[k][:, sel]
            scale = np.abs(g64 - kin[k]).max()
            assert scale > 0 and np.isfinite(mine).all()
            e = float(np.abs(mine - g64).max() / scale)
            ey = max(float(np.abs(yard[k] - g64).max() / scale), float(FLOOR * np.abs(g64).max() / scale))
            report("gradient", robot, integ, flags, path, name, e, ey)
            worst = max(worst, e / ey)
            if not e <= MARGIN * ey:
                bad.append((path, name, e, ey))
    assert not bad, bad
    return worst


GRAD_CPU_ROBOTS = ("panda_no_gripper", "iiwa7", "2link_robot", "allegro_left", "fetch_arm_no_gripper_small_damping")
# use_damping on the fingers and the composed path, at horizons where damping_ok: (robot, T, dt)
GRAD_DAMPED = [("allegro_left_small_damping", 3, 1e-3), ("fetch_arm_no_gripper_small_damping", 8, 2e-3)]


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("robot", GRAD_CPU_ROBOTS)
def test_gradients_against_fp64(cpu_library, robot, integ):
    """T = 32, dt = 5e-3: the dynamics' share of every gradient is 22 - 100 % at this horizon"""
    worst = max(check_gradients(robot, "cpu", integ, flags, 4, 32, 5e-3, [np.arange(4)], ["host"])
                for flags in flags_of(robot, GRAD_FLAGS, 32, 5e-3))
    print("ROLLEDGE gradient   %-34s %s worst err / yardstick %.2f" % (robot, integ, worst))


# (damping on the iiwa: neither the hand nor the Fetch arm takes it at dt = 5e-3)
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("robot,T,dt", GRAD_DAMPED, ids=[r for r, _, _ in GRAD_DAMPED])
def test_damped_gradients_against_fp64(cpu_library, robot, T, dt, integ):
    assert damping_ok(robot, T, dt)
    check_gradients(robot, "cpu", integ, (1, 1), 4, T, dt, [np.arange(4)], ["host"])


GRAD_GPU = [("panda_no_gripper", ((1, 0),)), ("iiwa7", ((1, 1),)), ("allegro_left", ((1, 0),)),
            ("fetch_arm_no_gripper_small_damping", ((1, 0),))]


@pytest.mark.gpu
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("robot,flag_sets", GRAD_GPU, ids=[r for r, _ in GRAD_GPU])
def test_gpu_gradients_against_fp64(robot, flag_sets, integ):
    """One launch of 70 rows: rows 0 - 3 lie in the full tile (the fused kernels' qdd_traj feeds the sweep), rows 64 - 67 in the tail
    (the composed path's)."""
    tile, tail = np.arange(4), np.arange(64, 68)
    name = path_name(robot, GPU)
    worst = max(check_gradients(robot, GPU, integ, flags, 70, 8, 5e-3, [tile, tail], [name, "gpu-tail"]) for flags in flag_sets)
    print("ROLLEDGE gradient   %-34s %s worst err / yardstick %.2f" % (robot, integ, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("robot,T,dt", GRAD_DAMPED, ids=[r for r, _, _ in GRAD_DAMPED])
def test_gpu_damped_gradients_against_fp64(robot, T, dt, integ):
    check_gradients(robot, GPU, integ, (1, 1), 70, T, dt, [np.arange(4), np.arange(64, 68)], [path_name(robot, GPU), "gpu-tail"])


@pytest.mark.gpu
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("robot,link,l_value", [("allegro_left", "link_2.0", 0.25), ("fetch_arm_no_gripper", "elbow_flex_link", 1.6)])
def test_gpu_mass_gradients_against_host(robot, link, l_value, integ):
    """Gradients with respect to q0, qd0, tau and a learnable PositiveScalar mass through the fingers kernel and the composed path,
    against the host build at the bound of test_rollout.test_gpu_gradients_against_cpu (the parameter gradient itself is pinned to the
    reference's autograd by test_rollout.test_gradients_against_reference_autograd).  (The Allegro's link_2.0: the rollout does not
    depend on the mass of link_1.0, whose gradient is rounding noise.)"""
    T, B, dt = 10, 70, 2e-3
    grads = []
    for device in ("cpu", GPU):
        m, l = learnable_mass_model(robot, link, l_value, device)
        q, qd, _ = sample_states(m, B, seed=6)
        tau = torch.from_numpy(torques(m, T, B)).to(device)
        grads.append(_grads_through(m, lambda mm, a, b, c: mm.compute_forward_dynamics_rollout(a, b, c, dt, integrator=integ),
                                    torch.from_numpy(q).to(device), torch.from_numpy(qd).to(device), tau, [l]))
    for name, x, y in zip(ARRAYS + ("dL/dmass",), grads[1], grads[0]):
        e = float(np.abs(np.asarray(x, np.float64) - y).max() / max(np.abs(y).max(), 1e-12))
        report("mass-grad", robot, integ, (1, 0), path_name(robot, GPU), name, e, 2e-3)
    for x, y in zip(grads[1], grads[0]):
        assert grad_close(x, y, 2e-3), (robot, integ, np.abs(x - y).max(), np.abs(y).max())


# ------------------------------------------------------------------------------------------------------------------- section E


def check_non_finite_rows(robot, dev, B=128):
    cpu, m = model(robot), model(robot, dev)
    T, dt, n = 6, 1e-3, cpu._n_dofs
    NAN_ROW, NAN_DOF, INF_ROW, INF_STEP, INF_DOF = 5, 2, 70, 3, 1
    q, qd, _ = sample_states(cpu, B, seed=14)
    tau = torques(cpu, T, B, seed=15)
    bad_q, bad_tau = q.copy(), tau.copy()
    bad_q[NAN_ROW, NAN_DOF] = np.nan
    bad_tau[INF_STEP, INF_ROW, INF_DOF] = np.inf
    # the coordinates of a row that depend on its DoF NAN_DOF: H of a hand is block diagonal, a finger never sees another finger
    hand = robot.startswith("allegro")
    dep = np.zeros(n, bool)
    if hand:
        dep[NAN_DOF // 4 * 4:NAN_DOF // 4 * 4 + 4] = True
    else:
        dep[:] = True
    others = np.ones(B, bool)
    others[[NAN_ROW, INF_ROW]] = False
    for integ in INTEGRATORS:
        clean = [x.cpu().numpy() for x in m.compute_forward_dynamics_rollout(*to(dev, q, qd, tau), dt, integrator=integ)]
        got = [x.cpu().numpy() for x in m.compute_forward_dynamics_rollout(*to(dev, bad_q, qd, bad_tau), dt, integrator=integ)]
        assert all(np.isfinite(x).all() for x in clean)
        for a, b in zip(got, clean):
            assert np.array_equal(a[:, others], b[:, others]), (robot, integ)
            assert np.array_equal(a[:, NAN_ROW][:, ~dep], b[:, NAN_ROW][:, ~dep]), (robot, integ)
            assert np.array_equal(a[:INF_STEP, INF_ROW], b[:INF_STEP, INF_ROW]), (robot, integ)
        gq, gqd = got
        # row NAN_ROW: qd is non-finite from the first step on; q too, except that explicit Euler's first q = q0 + dt qd0 does not
        # see the acceleration yet (its NaN DoF aside)
        assert not np.isfinite(gqd[:, NAN_ROW][:, dep]).any(), (robot, integ)
        assert not np.isfinite(gq[:, NAN_ROW, NAN_DOF]).any(), (robot, integ)
        assert not np.isfinite(gq[(1 if integ == "euler" else 0):, NAN_ROW][:, dep]).any(), (robot, integ)
        # row INF_ROW: the torque of step INF_STEP reaches qd at that step
        assert not np.isfinite(gqd[INF_STEP:, INF_ROW, INF_DOF]).any(), (robot, integ)
        assert all(not np.isfinite(gqd[t, INF_ROW]).all() for t in range(INF_STEP, T))


@pytest.mark.parametrize("robot", C_ABI_ROBOTS)
def test_non_finite_rows_are_isolated(cpu_library, robot):
    check_non_finite_rows(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", C_ABI_ROBOTS)
def test_gpu_non_finite_rows_are_isolated(robot):
    """128 rows: the Panda's and the Allegro's rows all lie in full tiles of the fused kernels, the Fetch arm's on the composed path."""
    check_non_finite_rows(robot, GPU)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", C_ABI_ROBOTS)
def test_gpu_non_finite_rows_stay_in_their_tile(robot):
    """192 rows: a third tile that holds no non-finite row, next to the two that do"""
    check_non_finite_rows(robot, GPU, B=192)

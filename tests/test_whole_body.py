"""The centre of mass, its velocity, acceleration and Jacobian, the angular momentum about the base origin and the base reaction wrench in
one call (csrc/drm_whole_body.hip, include/drm_hip_whole_body.h drm_whole_body; DifferentiableRobotModel.compute_center_of_mass /
compute_base_wrench / total_mass).

INPUTS: the first 128 rows of q and qd per robot of tests/golden/golden_fd_derivatives.npz (test_lagrangian.states), qdd [128, n] from a
seeded numpy generator at unit scale; the robots of tests/test_lagrangian.py, Fetch also with its sliding joints, and the skew-axis toy
of tests/test_joint_models.py.

TRUTH, fp64, from the oracle only: c_i = p_i + R_i com_i from Oracle.fk_all_poses, the per-link Jacobians from Oracle.fk_jacobian,
J_ci = lin_jac_i - [R_i com_i]x ang_jac_i; velocities are J qd, accelerations J qdd plus the Richardson-combined directional difference
of test_links' truth (h = 1e-4 and 3e-4); I_i = R_i I_com,i R_i^T with I_com,i = spec.inertia[i]; then the sums of the header's
definitions, over the links with at least one moving joint on spec.chain_to(i) (test_energy.moved_links) where it says "moved".
PINS, before any code under test is compared: central differences of com (Richardson) equal the truth's com_jac to 1e-9, and
com_jac^T (0, 0, M g) equals Oracle.rnea(q, 0, 0, gravity) to 1e-9 of the m g l scale of test_energy.potential_from_oracle.

YARDSTICK, not code under test: the world-frame recursion restated HERE in numpy on top of test_links._frames / links_world, with a
sweep back of every sub-tree's force and moment (about the base origin), mass and first moment.  In fp64 it must match every truth to
PIN = 1e-8, and its by-product joint torques z_j . (n_sub,j - p_j x f_sub,j) (z_j . f_sub,j for a prismatic joint) must match
Oracle.rnea(q, qd, qdd, gravity, no damping) in fp64 to 1e-8 on every robot: that ties the inertia convention and the wrench's signs to
the oracle.  In float32 it is the yardstick.
REQUIREMENT on the host build, the fused kernel and the general kernel: err <= 8 max(err(yardstick), 2^-23), the error the per-row
max|X - X64| / max|X64| over the row's vector or [3, n] array, worst over rows.  Where a truth is identically zero over the WHOLE batch the
error is normalised by a physical scale instead: lengths (com, com_jac) by mgl / (9.81 M), velocities, accelerations and momenta by
the same length, wrench components by mgl.  On these inputs no quantity of any robot is: the two-link robot turns about the vertical,
which zeroes the z component of its CoM velocity, the z row of its Jacobian and the x, y components of its angular momentum, but not
the vectors the error is taken over.
Every comparison prints one "WHOLEBODY" line (robot, path, quantity, error, yardstick, ratio) before it asserts;
profiles/whole_body_tests.txt holds them.

EXACT: see exact_check, bad_rows_check, autograd_check and c_abi_check.

GPU (-m gpu): a launch of B rows is repeated over consecutive slices of the 128 rows, so the statistic is over the same rows whatever B
is.  B = 64 and 128 are the fused arm kernel, 65 and 131 a fused part plus a ragged tail in the general kernel, 1 and every other robot
the general kernel alone, _composed=True the general kernel on the arms.  test_max_sizes.chain_model's 30-joint chain at 65 rows is a
size at which the general kernel's per-row records leave LDS for the scratch.

Measured (profiles/whole_body_tests.txt): the worst err / yardstick is 2.48 on the host build and 2.48 on the MI355X (com_acc of Fetch with
its sliding joints, 4.6e-7 against 1.8e-7); per quantity 2.04 for com_jac, 1.79 for ang_mom, 1.73 for force, 1.51 for com_vel, 1.28 for
moment and 1.22 for com.  With the sub-trees' first moment kept in link frames by the general walk, Fetch's moment stood at 8.29: its
horizontal first moment nearly cancels against the base share in some rows and was rounded at the size of the robot's height.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import load_model, sample_states
from oracle import Oracle
from test_energy import moved_links, potential_from_oracle
from test_lagrangian import ARMS, OTHERS, ROWS, model_on, richardson, row_err, states
from test_links import _cross, _frames, links_world

FLOOR, MARGIN, GRAVITY, PIN = 2.0 ** -23, 8.0, 9.81, 1e-8
NAMES = ("com", "com_vel", "com_acc", "com_jac", "ang_mom", "force", "moment")


def report(robot, path, what, e, ey):
    print("WHOLEBODY %-17s %-22s %-8s %.3e  %.3e  %.2f" % (robot, path, what, e, ey, e / ey))


# ------------------------------------------------------------------------------------------- the yardstick: numpy, world frame
def whole_body_world(spec, q, qd, qdd, dt, gravity=True):
    """({name: array in dtype dt}, tau [B, n]): the issue's sums from the world-frame recursion outwards and a sweep back of the
    sub-trees' force, moment about the base origin, mass and first moment"""
    dt = np.dtype(dt).type
    B, n = q.shape
    L, frames = _frames(spec, q, dt)
    P, V, W, A, AL = links_world(spec, q, qd, qdd, dt)
    moved = moved_links(spec)
    mass, com = spec.mass.astype(dt), spec.com.astype(dt)
    g = dt(GRAVITY if gravity else 0.0)
    ez = np.array([0, 0, 1], dt)
    R = {0: np.broadcast_to(np.eye(3, dtype=dt), (B, 3, 3))}
    for i, *_, Ri, _p in frames:
        R[i] = Ri
    f, no, mc, h, ho = (np.zeros((B, L, 3), dt) for _ in range(5))      # (f, no: without gravity; the weight comes from m, mc)
    m = np.zeros((B, L), dt)
    c_all = np.zeros((B, L, 3), dt)
    for i in range(L):
        rc = np.einsum("bij,j->bi", R[i], com[i]).astype(dt)
        c = (P[:, i] + rc).astype(dt)
        c_all[:, i] = c
        if not moved[i]:
            continue
        I = (R[i] @ spec.inertia[i].reshape(3, 3).astype(dt) @ np.swapaxes(R[i], 1, 2)).astype(dt)
        vc = V[:, i] + _cross(W[:, i], rc)
        ac = A[:, i] + _cross(AL[:, i], rc) + _cross(W[:, i], _cross(W[:, i], rc))
        Iw = np.einsum("bij,bj->bi", I, W[:, i]).astype(dt)
        m[:, i], mc[:, i] = mass[i], mass[i] * c
        h[:, i], ho[:, i] = mass[i] * vc, _cross(c, mass[i] * vc) + Iw
        f[:, i] = mass[i] * ac
        no[:, i] = _cross(c, f[:, i]) + np.einsum("bij,bj->bi", I, AL[:, i]).astype(dt) + _cross(W[:, i], Iw)
    tau, cols = np.zeros((B, n), dt), np.zeros((B, 3, n), dt)
    for i, par, d, pris, z, r, _, p in reversed(frames):
        if d >= 0:
            fg = f[:, i] + m[:, i, None] * g * ez
            ng = no[:, i] + _cross(mc[:, i], g * ez[None, :])
            tau[:, d] = np.einsum("bi,bi->b", z, fg if pris else ng - _cross(p, fg))
            cols[:, :, d] = z * m[:, i, None] if pris else _cross(z, mc[:, i] - m[:, i, None] * p)
        for x in (f, no, m, mc, h, ho):
            x[:, par] = x[:, par] + x[:, i]
    still = ~moved
    M = dt(m[0, 0] + mass[still].sum())
    mc_all = mc[:, 0] + (c_all[:, still] * mass[still][None, :, None]).sum(axis=1)
    out = dict(com=mc_all / M, com_vel=h[:, 0] / M, com_acc=f[:, 0] / M, com_jac=cols / M, ang_mom=ho[:, 0],
               force=f[:, 0] + M * g * ez, moment=no[:, 0] + _cross(mc_all, g * ez[None, :]))
    return {k: v.astype(dt) for k, v in out.items()}, tau


# ------------------------------------------------------------------------------------------------------------------- truth
def build_truth(spec, q, qd, qdd, name="?"):
    orc = Oracle(spec)
    B, n = q.shape
    L = len(spec.parent)
    q64, qd64, qdd64 = (x.astype(np.float64) for x in (q, qd, qdd))
    mass, com, moved = spec.mass.astype(np.float64), spec.com.astype(np.float64), moved_links(spec)
    mm = mass * moved
    M = mass.sum()

    def centres(x):
        R, p = orc.fk_all_poses(x, np.float64)
        rc = np.einsum("blij,lj->bli", R, com)
        return R, rc, p + rc

    def jac(x):
        """[B, L, 6, n]: the Jacobians of the links' centres of mass (linear) and frames (angular)"""
        _, rc, _ = centres(x)
        J = np.zeros((x.shape[0], L, 6, n))
        for l in range(1, L):
            _, _, lin, ang = orc.fk_jacobian(x, l, np.float64)
            J[:, l, :3], J[:, l, 3:] = lin - np.einsum("bij,bjn->bin", _skew_b(rc[:, l]), ang), ang
        return J

    R, rc, c = centres(q64)
    J64 = jac(q64)
    V64 = np.einsum("blij,bj->bli", J64, qd64)
    Jd = lambda s: np.einsum("blij,bj->bli", jac(q64 + s * qd64), qd64)
    A64 = np.einsum("blij,bj->bli", J64, qdd64) + richardson(lambda h: (Jd(h) - Jd(-h)) / (2 * h))
    I = np.einsum("blij,ljk,blmk->blim", R, spec.inertia.reshape(L, 3, 3).astype(np.float64), R)
    vc, w, ac, al = V64[..., :3], V64[..., 3:], A64[..., :3], A64[..., 3:]
    Iw = np.einsum("blij,blj->bli", I, w)
    ez = np.array([0.0, 0.0, 1.0])
    mc_all = (c * mass[None, :, None]).sum(1)
    t64 = dict(
        com=mc_all / M,
        com_vel=(vc * mm[None, :, None]).sum(1) / M,
        com_acc=(ac * mm[None, :, None]).sum(1) / M,
        com_jac=(J64[:, :, :3] * mm[None, :, None, None]).sum(1) / M,
        ang_mom=((np.cross(c, vc) * mass[None, :, None] + Iw) * moved[None, :, None]).sum(1),
        force=(ac * mm[None, :, None]).sum(1) + M * GRAVITY * ez,
        moment=((np.cross(c, ac) * mass[None, :, None] + np.einsum("blij,blj->bli", I, al) + np.cross(w, Iw)) * moved[None, :, None]).sum(1)
        + np.cross(mc_all, GRAVITY * ez[None, :]))
    # pins
    _, mgl = potential_from_oracle(orc, spec, q64)
    fd = np.zeros((B, 3, n))
    for d in range(n):
        e = np.zeros(n)
        e[d] = 1.0
        com_at = lambda s: (centres(q64 + s * e)[2] * mass[None, :, None]).sum(1) / M
        fd[:, :, d] = richardson(lambda h: (com_at(h) - com_at(-h)) / (2 * h))
    assert np.abs(fd - t64["com_jac"]).max() <= 1e-9, np.abs(fd - t64["com_jac"]).max()
    g64 = orc.rnea(q64, np.zeros_like(q64), np.zeros_like(q64), True, False, np.float64)
    assert np.abs(t64["com_jac"][:, 2, :] * M * GRAVITY - g64).max() <= 1e-9 * mgl
    # the yardstick in fp64 must be the truth, and its torques the oracle's
    y64, tau64 = whole_body_world(spec, q, qd, qdd, np.float64)
    scale = scales(mgl, M)
    for k in NAMES:
        e = err_of(y64[k], t64[k], scale[k])
        if k in ("com_acc", "force", "moment"):
            report(name, "yardstick64", k, e, PIN)
        assert e <= PIN, (k, e)
    e = row_err(tau64, orc.rnea(q64, qd64, qdd64, True, False, np.float64))
    report(name, "yardstick64", "tau", e, PIN)
    assert e <= PIN, e
    y32, _ = whole_body_world(spec, q, qd, qdd, np.float32)
    assert all(v.dtype == np.float32 for v in y32.values())
    return dict(t64=t64, y32=y32, scale=scale, M=M, base_mass=float(mass[~moved].sum()), mgl=mgl)


def _skew_b(v):
    K = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -v[..., 2], v[..., 1], v[..., 2], -v[..., 0], -v[..., 1], v[..., 0]
    return K


def scales(mgl, M):
    """the physical scale a quantity's error is normalised by where its truth is identically zero over the batch"""
    length = mgl / (GRAVITY * M)
    return dict(com=length, com_vel=length, com_acc=length, com_jac=length, ang_mom=mgl / GRAVITY * length, force=mgl, moment=mgl)


def err_of(X, T, scale):
    T = np.asarray(T, np.float64)
    if np.abs(T).max() == 0:
        return float(np.abs(np.asarray(X, np.float64)).max() / scale)
    return row_err(X, T)


def qdd_of(n, rows=ROWS, seed=20261):
    return np.random.default_rng(seed).standard_normal((rows, n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(robot, compat=True):
    q, qd = states(robot)
    return q, qd, qdd_of(q.shape[1])


@functools.lru_cache(maxsize=None)
def truth(robot, compat=True):
    return build_truth(model_on(robot, "cpu", compat)._spec, *inputs(robot, compat), name=robot)


def check(robot, path, got, t, rows=slice(None)):
    failures = []
    for k in NAMES:
        x = got[k]
        x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
        assert x.dtype == np.float32 and x.shape == t["t64"][k][rows].shape, (k, x.shape)
        e = err_of(x, t["t64"][k][rows], t["scale"][k])
        ey = max(err_of(t["y32"][k][rows], t["t64"][k][rows], t["scale"][k]), FLOOR)
        report(robot, path, k, e, ey)
        if not e <= MARGIN * ey:
            failures.append((k, e, ey))
    assert not failures, failures


def run_model(model, data, B=None, composed=False):
    """Both methods over the rows in consecutive launches of B rows (None: one launch) -> {quantity: tensor}"""
    q, qd, qdd = (torch.from_numpy(x).to(model._device) for x in data)
    N = q.shape[0]
    B = B or N
    parts = []
    for i in range(0, N, B):
        s = slice(i, i + B)
        c = model.compute_center_of_mass(q[s], qd[s], qdd[s], jacobian=True, _composed=composed)
        w = model.compute_base_wrench(q[s], qd[s], qdd[s], _composed=composed)
        assert type(c).__name__ == "CenterOfMass" and c._fields == ("mass", "position", "velocity", "acceleration", "jacobian", "angular_momentum")
        assert type(w).__name__ == "BaseWrench" and w._fields == ("force", "moment")
        assert all(x.grad_fn is None and not x.requires_grad for x in tuple(c[1:]) + tuple(w))
        parts.append((c.position, c.velocity, c.acceleration, c.jacobian, c.angular_momentum, w.force, w.moment))
    return dict(zip(NAMES, (torch.cat([p[i] for p in parts]) for i in range(7))))


def call_all(model, q, qd, qdd, want=NAMES, composed=False, base=True, gravity=True):
    """backend.whole_body — the ctypes call itself — on the model's dynamics walk"""
    from differentiable_robot_model_amd import backend
    dw = model._dynamics_walk()
    return dict(zip(NAMES, backend.whole_body(dw.program, model._ops_f(dw).detach(), dw.ops_i, q, qd, qdd, model._n_dofs, want,
                                              base_share=model._base_share() if base else None, include_gravity=gravity, composed=composed)))


def exact_check(model, data, t, composed=False, B=None):
    """qd = 0 -> velocity, angular momentum == 0; at rest force == (0, 0, M g) up to the rounding of one product with force_x, force_y
    == 0 exactly, and without gravity exact zeros; outputs requested alone equal the same outputs requested together, and the two
    methods the call for all seven, to the bit; include_base=False against True."""
    q, qd, qdd = (torch.from_numpy(x[:B or ROWS]).to(model._device) for x in data)
    z = torch.zeros_like(qd)
    still = model.compute_center_of_mass(q, z, qdd, _composed=composed)
    assert (still.velocity == 0).all() and (still.angular_momentum == 0).all() and still.acceleration.abs().max() > 0
    rest = model.compute_base_wrench(q, z, z, _composed=composed)
    static = model.compute_base_wrench(q, _composed=composed)
    M = model.total_mass()
    assert isinstance(M, float) and abs(M - t["M"]) <= 1e-6 * t["M"]
    for w in (rest, static):
        assert (w.force[:, :2] == 0).all()
        assert (w.force[:, 2] - M * GRAVITY).abs().max() <= 2.0 ** -22 * M * GRAVITY
    assert torch.equal(rest.moment, static.moment)
    for w in (model.compute_base_wrench(q, z, z, include_gravity=False, _composed=composed),
              model.compute_base_wrench(q, include_gravity=False, _composed=composed)):
        assert (w.force == 0).all() and (w.moment == 0).all()
    # alone == together, and the methods == the call for all seven
    all7 = call_all(model, q, qd, qdd, composed=composed)
    for k in NAMES:
        qd_k, qdd_k = (qd if k not in ("com", "com_jac") else None), (qdd if k in ("com_acc", "force", "moment") else None)
        alone = call_all(model, q, qd_k, qdd_k, want=(k,), composed=composed)
        assert torch.equal(alone[k], all7[k]), k
        assert all(alone[o] is None for o in NAMES if o != k)
    c = model.compute_center_of_mass(q, qd, qdd, jacobian=True, _composed=composed)
    w = model.compute_base_wrench(q, qd, qdd, _composed=composed)
    for k, x in zip(NAMES, (c.position, c.velocity, c.acceleration, c.jacobian, c.angular_momentum, w.force, w.moment)):
        assert torch.equal(x, all7[k]), k
    only = model.compute_center_of_mass(q, _composed=composed)
    assert torch.equal(only.position, all7["com"]) and only.velocity is None and only.acceleration is None and only.jacobian is None
    # without the base share
    Mm = model.total_mass(include_base=False)
    assert abs((M - Mm) - t["base_mass"]) <= 1e-6 * max(t["base_mass"], 1.0)
    cm = model.compute_center_of_mass(q, qd, jacobian=True, include_base=False, _composed=composed)
    assert cm.mass == Mm
    for a, b, k in ((cm.velocity * Mm, c.velocity * M, "com_vel"), (cm.jacobian * Mm, c.jacobian * M, "com_jac")):
        ey = max(err_of(t["y32"][k][:len(q)], t["t64"][k][:len(q)], t["scale"][k]), FLOOR)
        assert row_err(a.cpu().numpy(), b.cpu().numpy()) <= MARGIN * ey, k
    wm = model.compute_base_wrench(q, _composed=composed, include_base=False)
    assert (wm.force[:, :2] == 0).all()
    assert ((static.force[:, 2] - wm.force[:, 2]) - t["base_mass"] * GRAVITY).abs().max() <= 2.0 ** -21 * M * GRAVITY


def bad_rows_check(model, data, composed=False, B=ROWS):
    """a NaN, an Inf and a |q| = 1e6 row planted in a launch make that row's outputs NaN and change no bit of the others"""
    q, qd, qdd = (torch.from_numpy(x[:B].copy()).to(model._device) for x in data)
    clean = call_all(model, q, qd, qdd, composed=composed)
    bad = {3: (0, float("nan")), 70 % B: (1, float("inf")), B - 1: (0, 1e6), 17: (2, float("-inf"))}
    x = [q.clone(), qd.clone(), qdd.clone()]
    for r, (which, v) in bad.items():
        x[which][r, r % q.shape[1]] = v
    dirty = call_all(model, *x, composed=composed)
    good = torch.ones(B, dtype=torch.bool, device=q.device)
    good[list(bad)] = False
    for k in NAMES:
        assert torch.isnan(dirty[k][~good]).all(), k
        assert torch.equal(dirty[k][good], clean[k][good]), k


def autograd_check(device):
    model = model_on("panda_no_gripper", device)
    q0, qd0, qdd0 = (torch.from_numpy(x[:67]).to(device) for x in inputs("panda_no_gripper"))
    J = model.compute_center_of_mass(q0, jacobian=True).jacobian
    q, qd = q0.clone().requires_grad_(True), qd0.clone().requires_grad_(True)
    c = model.compute_center_of_mass(q, qd, qdd0, jacobian=True)
    assert c.position.requires_grad and c.velocity.requires_grad
    assert not any(x.requires_grad for x in (c.acceleration, c.jacobian, c.angular_momentum))
    c.position.sum().backward(retain_graph=True)
    ones = torch.ones_like(c.position)
    assert torch.equal(q.grad, torch.einsum("bi,bin->bn", ones, J)) and qd.grad is None
    q.grad = None
    c.velocity.sum().backward()
    assert torch.equal(qd.grad, torch.einsum("bi,bin->bn", ones, J)) and (q.grad is None or (q.grad == 0).all())
    # the backward launches for the Jacobian where the forward did not
    q2 = q0.clone().requires_grad_(True)
    cot = torch.from_numpy(np.random.default_rng(5).standard_normal((67, 3)).astype(np.float32)).to(device)
    (model.compute_center_of_mass(q2).position * cot).sum().backward()
    assert torch.equal(q2.grad, torch.einsum("bi,bin->bn", cot, J))
    # first order only
    q3 = q0.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(model.compute_center_of_mass(q3).position.sum(), (q3,), create_graph=True)
    with pytest.raises(NotImplementedError):
        g1.sum().backward()
    # the wrench and a call under no_grad carry no graph
    w = model.compute_base_wrench(q, qd, qdd0)
    with torch.no_grad():
        c4 = model.compute_center_of_mass(q, qd)
    assert not any(x.requires_grad for x in tuple(w) + (c4.position, c4.velocity))
    # unbatched inputs give unbatched results
    c1 = model.compute_center_of_mass(q0[0], qd0[0], jacobian=True)
    assert c1.position.shape == (3,) and c1.jacobian.shape == (3, 7) and torch.equal(c1.position, model.compute_center_of_mass(q0[:1]).position[0])


def walk_of(model):
    from differentiable_robot_model_amd import backend
    dw = model._dynamics_walk()
    return backend._walk_struct(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs)


def c_abi_check(lib, robot, device, stream, t, B=ROWS):
    """Straight through ctypes: every pointer 4 bytes off a 16-byte boundary (the general kernel on the device) gives the aligned call's
    values within the bound; a scratch of exactly the queried size; guard words behind the scratch and on both sides of every output."""
    from differentiable_robot_model_amd import backend
    model = model_on(robot, device)
    walk, n = walk_of(model), model._n_dofs
    sync = (lambda: None) if device == "cpu" else torch.cuda.synchronize
    GUARD = 64
    mass, mc = model._base_share()
    base = backend.DrmBaseShare(mass, (ctypes.c_float * 3)(*mc))

    def shifted(x, off):
        buf = torch.zeros(x.numel() + 4, device=device)
        lead = (off - buf.data_ptr() // 4) % 4
        buf[lead:lead + x.numel()] = x.reshape(-1)
        view = buf[lead:lead + x.numel()].view(x.shape)
        assert view.data_ptr() % 16 == 4 * off
        return view

    def call(off, flags=1, rows=B):
        q, qd, qdd = (shifted(torch.from_numpy(x[:B].copy()).to(device), off) for x in inputs(robot))
        query = lib.drm_whole_body_scratch_floats if off else lib.drm_whole_body_scratch_floats_aligned
        need = int(query(ctypes.byref(walk), max(rows, 0)))
        scratch = torch.full((need + GUARD,), 3.25, device=device)
        sizes = (B * 3, B * 3, B * 3, B * 3 * n, B * 3, B * 3, B * 3)
        bufs, outs = [], []
        for s in sizes:
            buf = torch.full((s + 2 * GUARD + 4,), -1.5, device=device)
            lead = GUARD + (off - (buf.data_ptr() // 4 + GUARD)) % 4
            bufs.append((buf, lead, s))
            outs.append(buf[lead:lead + s])
            assert outs[-1].data_ptr() % 16 == 4 * off
        rc = lib.drm_whole_body(ctypes.byref(walk), q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), rows, flags, ctypes.byref(base),
                                *[o.data_ptr() for o in outs], scratch.data_ptr(), stream)
        sync()
        assert (scratch[need:] == 3.25).all()
        for buf, lead, s in bufs:
            assert (buf[:lead] == -1.5).all() and (buf[lead + s:] == -1.5).all()
            if rc != 0 or rows <= 0:
                assert (buf == -1.5).all()
        shapes = [(B, 3)] * 3 + [(B, 3, n)] + [(B, 3)] * 3
        return rc, dict(zip(NAMES, (o.clone().view(sh) for o, sh in zip(outs, shapes)))), need

    assert lib.drm_abi_version() == 15
    rc, aligned, _ = call(0)
    assert rc == 0
    rc, off4, _ = call(1)
    assert rc == 0
    check(robot, "abi-aligned", aligned, t, rows=slice(0, B))
    check(robot, "abi-misaligned", off4, t, rows=slice(0, B))
    assert call(0, rows=0)[0] == 0 and call(0, rows=-1)[0] == -1
    return aligned, off4


def long_chain_check(tmp_path, device, path):
    """test_max_sizes.chain_model's 30-joint chain (joints about +-x / +-y / +-z), 65 rows."""
    from test_max_sizes import chain_model
    model = chain_model(tmp_path, 30, device)
    q, qd, _ = sample_states(model, 65, seed=0)
    data = (q, qd, qdd_of(q.shape[1], 65))
    check("chain30", path, run_model(model, data), build_truth(model._spec, *data, name="chain30"))
    return model


def skew_check(tmp_path_factory, device, path):
    """tests/test_joint_models.py's toy robot: prismatic about z, revolute and prismatic about skew axes (two ops per skew link)."""
    from test_joint_models import toy_model, toy_urdf
    urdf = tmp_path_factory.mktemp("toy_whole_body") / "toy.urdf"
    urdf.write_text(toy_urdf())
    model = toy_model(str(urdf), device)
    assert model._spec.skew.any()
    q, qd, _ = sample_states(model, 65, seed=1)
    data = (q, qd, qdd_of(q.shape[1], 65))
    t = build_truth(model._spec, *data, name="toy_skew")
    check("toy_skew", path, run_model(model, data), t)
    exact_check(model, data, t, B=65)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("robot", ARMS + OTHERS)
def test_host_build_against_truth(cpu_library, robot):
    model = model_on(robot)
    check(robot, "host", run_model(model, inputs(robot)), truth(robot))
    exact_check(model, inputs(robot), truth(robot))


@pytest.mark.parametrize("robot", ARMS)
def test_host_general_walk_on_the_arms(cpu_library, robot):
    """the host build runs the chain form on an arm and the general walk with _composed: both against the truth, and not the same bits"""
    model = model_on(robot)
    out = run_model(model, inputs(robot), composed=True)
    check(robot, "host-general", out, truth(robot))
    exact_check(model, inputs(robot), truth(robot), composed=True)
    chain = run_model(model, inputs(robot))
    assert any(not torch.equal(out[k], chain[k]) for k in NAMES)


def test_fetch_with_sliding_joints(cpu_library):
    model = model_on("fetch", "cpu", False)
    assert (model._spec.kind == 2).any()
    check("fetch", "host-prismatic", run_model(model, inputs("fetch", False)), truth("fetch", False))


def test_skew_axis_model(cpu_library, tmp_path_factory):
    skew_check(tmp_path_factory, "cpu", "host-prismatic")


def test_long_chain(cpu_library, tmp_path):
    long_chain_check(tmp_path, "cpu", "host")


@pytest.mark.parametrize("composed", [False, True], ids=["chain", "general"])
def test_non_finite_rows(cpu_library, composed):
    bad_rows_check(model_on("panda_no_gripper"), inputs("panda_no_gripper"), composed=composed)


def test_non_finite_rows_of_a_tree(cpu_library):
    bad_rows_check(model_on("iiwa7_allegro"), inputs("iiwa7_allegro"))


def test_autograd(cpu_library):
    autograd_check("cpu")


@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7_allegro"])
def test_c_abi_on_the_host_build(cpu_library, robot):
    c_abi_check(cpu_library, robot, "cpu", None, truth(robot))


def test_exports_and_refusals(cpu_library):
    import differentiable_robot_model_amd as drm
    from differentiable_robot_model_amd import backend
    assert drm.CenterOfMass._fields[0] == "mass" and drm.BaseWrench._fields == ("force", "moment")
    assert backend.WHOLE_BODY_COMPOSED == 2048
    model = model_on("panda_no_gripper")
    q, qd, qdd = (torch.from_numpy(x[:5]) for x in inputs("panda_no_gripper"))
    with pytest.raises(ValueError):
        model.compute_center_of_mass(q, None, qdd)
    with pytest.raises(RuntimeError, match="need qd"):
        call_all(model, q, None, None, want=("com_vel",))


def test_learnable_links(cpu_library):
    """a moved learnable link enters with its current value and ``mass`` becomes a detached 0-dim tensor; a learnable mass on a link of the
    base share is refused with include_base=True and served without"""
    import dataclasses
    from differentiable_robot_model_amd.rigid_body_params import PositiveScalar, UnconstrainedTensor
    robot = "fetch"
    model = load_model(robot, "cpu")
    spec = model._spec
    moving = max(i for i in range(len(spec.parent)) if spec.dof[i] >= 0)
    new_com = spec.com.copy()
    new_com[moving] = spec.com[moving] + np.asarray([0.03, -0.02, 0.05], np.float32)
    model.make_link_param_learnable(spec.link_names[moving], "com", UnconstrainedTensor(dim1=1, dim2=3, init_tensor=torch.from_numpy(new_com[moving])))
    data = inputs(robot)
    t = build_truth(dataclasses.replace(spec, com=new_com), *data, name="fetch-learnable")
    assert row_err(t["t64"]["com"], truth(robot)["t64"]["com"]) > 1e-4
    check(robot, "host-learnable", run_model(model, data), t)
    mass = model.compute_center_of_mass(torch.from_numpy(data[0][:3])).mass
    assert isinstance(mass, torch.Tensor) and mass.ndim == 0 and not mass.requires_grad and abs(float(mass) - t["M"]) <= 1e-5 * t["M"]
    still = [i for i in range(len(spec.parent)) if not moved_links(spec)[i] and spec.mass[i] > 0]
    model.make_link_param_learnable(spec.link_names[still[0]], "mass", PositiveScalar())
    q = torch.from_numpy(data[0][:3])
    with pytest.raises(NotImplementedError):
        model.compute_center_of_mass(q)
    with pytest.raises(NotImplementedError):
        model.compute_base_wrench(q)
    assert torch.isfinite(model.compute_center_of_mass(q, include_base=False).position).all()


# ------------------------------------------------------------------------------------------------------------------- GPU
def gpu_run_and_check(robot, B, composed=False, compat=True, path=None):
    model = model_on(robot, "cuda:0", compat)
    out = run_model(model, inputs(robot, compat), B=B, composed=composed)
    torch.cuda.synchronize()
    name = path or ("general" if composed or robot not in ARMS or B < 64 else "fused") + "-B%d" % B
    check(robot, name, out, truth(robot, compat))
    return model, out


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 128, 131])
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_against_truth(robot, B):
    model, _ = gpu_run_and_check(robot, B)
    if B >= 64:
        exact_check(model, inputs(robot), truth(robot), B=B if B <= ROWS else ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_general_kernel(robot):
    model, general = gpu_run_and_check(robot, 128, composed=True)
    exact_check(model, inputs(robot), truth(robot), composed=True)
    fused = run_model(model, inputs(robot))
    again = run_model(model, inputs(robot))
    twice = run_model(model, inputs(robot), composed=True)
    torch.cuda.synchronize()
    assert any(not torch.equal(general[k], fused[k]) for k in NAMES), "a dispatch that drops a rung"
    assert all(torch.equal(fused[k], again[k]) and torch.equal(general[k], twice[k]) for k in NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", OTHERS)
def test_gpu_other_robots_against_truth(robot):
    model, _ = gpu_run_and_check(robot, 65)
    exact_check(model, inputs(robot), truth(robot), B=65)


@pytest.mark.gpu
def test_gpu_fetch_with_sliding_joints():
    gpu_run_and_check("fetch", 65, compat=False, path="general-prismatic")


@pytest.mark.gpu
def test_gpu_skew_axis_model(tmp_path_factory):
    skew_check(tmp_path_factory, "cuda:0", "general-B65")


@pytest.mark.gpu
def test_gpu_long_chain_keeps_its_records_in_the_scratch(tmp_path):
    from differentiable_robot_model_amd import backend
    model = long_chain_check(tmp_path, "cuda", "general-B65")
    assert backend.load_library().drm_whole_body_scratch_floats(ctypes.byref(walk_of(model)), 65) > 0


@pytest.mark.gpu
def test_gpu_persistent_grid_beyond_2048_tiles(tmp_path):
    from test_lagrangian import persistent_grid_check
    persistent_grid_check(tmp_path, "drm_whole_body_scratch_floats_aligned", lambda m, q, qd: m.compute_base_wrench(q, qd, qd))


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7_allegro"])
def test_gpu_c_abi_misaligned_and_guards(robot):
    from differentiable_robot_model_amd import backend
    aligned, off4 = c_abi_check(backend.load_library(), robot, "cuda", backend._stream(torch.device("cuda:0")), truth(robot))
    if robot in ARMS:
        assert any(not torch.equal(aligned[k], off4[k]) for k in NAMES)       # (the fused kernel and the general one)


@pytest.mark.gpu
def test_gpu_c_abi_ragged_batch():
    from differentiable_robot_model_amd import backend
    c_abi_check(backend.load_library(), "panda_no_gripper", "cuda", backend._stream(torch.device("cuda:0")), truth("panda_no_gripper"), B=67)


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_non_finite_rows(composed):
    bad_rows_check(model_on("panda_no_gripper", "cuda:0"), inputs("panda_no_gripper"), composed=composed)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_autograd():
    autograd_check("cuda:0")

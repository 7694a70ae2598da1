"""Kinetic and potential energy, generalised momentum and their gradients in one call (csrc/drm_energy.hip, include/drm_hip.h drm_energy;
DifferentiableRobotModel.compute_energy_derivatives / compute_energy / compute_generalized_momentum).

INPUTS: the first 128 rows of q and qd per robot of tests/golden/golden_fd_derivatives.npz; the robots of tests/test_lagrangian.py.

TRUTH, from the fp64 oracle only: H64 = Oracle.mass_matrix, T64 = 1/2 qd^T H64 qd, p64 = H64 qd, g64 = Oracle.rnea(q, 0, 0, gravity),
V64 = 9.81 sum_i m_i (p_i + R_i c_i)_z from Oracle.fk_all_poses(float64) and spec.mass / spec.com over the links with at least one
moving joint on spec.chain_to(i), dTdq64 = central differences of T64 at h = 1e-4 and 3e-4, Richardson-combined as (9 f_h - f_3h) / 8.
Before anything under test is compared the same differences of V64 must equal g64 to 1e-9 max(|g64|, floor).

YARDSTICK, not code under test: the recursion of csrc/drm_energy.hpp restated HERE in numpy in link-local frames (Featherstone's
convention, spatial vectors [angular; linear] at each link's origin, general joint axes).  Run in fp64 it must first match all five
truths to 1e-8 relative: that settles the formula and its signs.  Run in float32 it is the yardstick; for g and p the oracle's own
float32 rnea / mass_matrix @ qd are taken too, and the larger error of the two counts.
REQUIREMENT throughout: err(path) <= 8 max(err(yardstick), 2^-23); 8 is the project's margin for a different summation order.
    p, dT/dq, g   per-row max|X - X64| / max|X64|, worst over rows
    T, V          max_b |X - X64| / max_b |X64|
FLOOR: where a truth is identically zero (the two-link robot turns about the vertical: g64 = 0 in every row, V64 is a constant that may
be 0) the error is normalised by 9.81 sum_i m_i max_b |p_i + R_i c_i|, the gravity torque the robot would feel with gravity in its
plane, instead of by max|X64|.  Nowhere else.
Every comparison prints one "ENERGY" line (robot, path, quantity, error, yardstick, ratio) before it asserts; profiles/energy_tests.txt
holds them for the host build and the MI355X.

EXACT: rows with qd = 0 give kinetic == 0, momentum == 0, dkinetic_dq == 0; kinetic >= 0 everywhere; compute_energy and
compute_generalized_momentum equal compute_energy_derivatives to the bit; outputs requested alone equal the same outputs requested
together to the bit; a NaN, an Inf and a |q| = 1e6 row planted in a 128-row launch make that row's five outputs NaN and change no bit
of the other 127.

GPU (-m gpu): a launch of B rows is repeated over consecutive slices of the 128 rows, so the statistic is over the same rows whatever
B is.  B = 64 and 128 are the fused arm kernel, 65 and 131 a fused part plus a ragged tail in the general kernel, 1 the general kernel
alone.  test_max_sizes.chain_model's 30-joint chain at 65 rows is a size at which the general kernel's per-row records leave LDS for
the scratch.

Measured (profiles/energy_tests.txt): the worst err / yardstick is 1.54 on the host build and 1.54 on the MI355X, on both kernels
(V of the Panda, 2.1e-7 against 1.4e-7); per quantity 1.34 for T (the skew-axis toy), 1.44 for dT/dq (the two-link robot), 0.95 for g and
0.55 for p, whose yardstick is the oracle's float32 H @ qd at 1e-5.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from helpers import load_model
from oracle import Oracle
from test_lagrangian import ARMS, OTHERS, ROWS, _crm, _rpy, _skew, model_on, richardson, states, walk_of

FLOOR, MARGIN, GRAVITY = 2.0 ** -23, 8.0, 9.81
NAMES = ("kinetic", "potential", "momentum", "dkinetic_dq", "gravity")
SHORT = dict(kinetic="T", potential="V", momentum="p", dkinetic_dq="dT/dq", gravity="g")


# ------------------------------------------------------------------------------------------------------------------- truth
def moved_links(spec):
    """[L] bool: at least one moving joint on the way from the root to the link"""
    return np.array([any(spec.dof[j] >= 0 for j in spec.chain_to(i)) for i in range(len(spec.parent))])


def potential_from_oracle(orc, spec, q64):
    """(V64 [B], the m g L scale of the robot) from the oracle's fp64 poses of every link"""
    R, p = orc.fk_all_poses(q64, np.float64)
    com = p + np.einsum("blij,lj->bli", R, spec.com.astype(np.float64))
    m = spec.mass.astype(np.float64) * moved_links(spec)
    return GRAVITY * (com[:, :, 2] * m[None, :]).sum(axis=1), GRAVITY * float((np.linalg.norm(com, axis=2).max(axis=0) * m).sum())


def central(f, q64, h):
    """[B, n]: central differences of the scalar field f [B] at step h"""
    out = np.empty(q64.shape)
    for k in range(q64.shape[1]):
        e = np.zeros(q64.shape[1])
        e[k] = h
        out[:, k] = (f(q64 + e) - f(q64 - e)) / (2 * h)
    return out


def vec_err(X, T, floor=0.0):
    """per-row max|X - T| / max(max|T|, floor) over the row's entries, worst over rows (rows without a scale are skipped)"""
    X, T = np.asarray(X, np.float64), np.asarray(T, np.float64)
    scale = np.maximum(np.abs(T).max(axis=1), floor)
    live = scale > 0
    return float((np.abs(X - T).max(axis=1)[live] / scale[live]).max()) if live.any() else 0.0


def scalar_err(X, T, floor=0.0):
    """max_b |X - T| / max(max_b |T|, floor)"""
    X, T = np.asarray(X, np.float64), np.asarray(T, np.float64)
    return float(np.abs(X - T).max() / max(np.abs(T).max(), floor))


def errors(got, t, rows=slice(None)):
    """the five errors of (T, V, p, dT/dq, g) against the truth t over its rows `rows`"""
    T, V, p, dT, g = got
    return dict(kinetic=scalar_err(T, t["T64"][rows], t["floors"]["kinetic"]), potential=scalar_err(V, t["V64"][rows], t["floors"]["potential"]),
                momentum=vec_err(p, t["p64"][rows]), dkinetic_dq=vec_err(dT, t["dT64"][rows]), gravity=vec_err(g, t["g64"][rows], t["floors"]["gravity"]))


def build_truth(spec, q, qd):
    orc = Oracle(spec)
    q64, qd64, z = q.astype(np.float64), qd.astype(np.float64), np.zeros(q.shape)
    H = lambda x: orc.mass_matrix(x, True, False, np.float64)
    kinetic = lambda x: 0.5 * np.einsum("bi,bij,bj->b", qd64, H(x), qd64)
    H64 = H(q64)
    g64 = orc.rnea(q64, z, z, True, False, np.float64)
    V64, mgl = potential_from_oracle(orc, spec, q64)
    assert mgl > 0
    # a truth that is identically zero is normalised by the robot's m g L instead (module docstring, FLOOR)
    floors = dict(kinetic=0.0, potential=mgl if np.abs(V64).max() <= 1e-12 * mgl else 0.0, gravity=mgl if np.abs(g64).max() <= 1e-12 * mgl else 0.0)
    # the truth itself, before anything under test: dV64/dq = g64
    dV64 = richardson(lambda h: central(lambda x: potential_from_oracle(orc, spec, x)[0], q64, h))
    pin = np.abs(dV64 - g64).max()
    assert pin <= 1e-9 * max(np.abs(g64).max(), mgl if floors["gravity"] else 0.0), pin
    t = dict(T64=kinetic(q64), V64=V64, p64=np.einsum("bij,bj->bi", H64, qd64), dT64=richardson(lambda h: central(kinetic, q64, h)), g64=g64,
             floors=floors)
    # the yardstick: in fp64 it must be the truth
    e64 = errors(energy_local(spec, q, qd, np.float64), t)
    assert all(e <= 1e-8 for e in e64.values()), e64
    y32 = energy_local(spec, q, qd, np.float32)
    assert all(x.dtype == np.float32 for x in y32)
    z32 = z.astype(np.float32)
    g32 = orc.rnea(q, z32, z32, True, False, np.float32)
    p32 = np.einsum("bij,bj->bi", orc.mass_matrix(q, True, False, np.float32), qd)
    assert g32.dtype == np.float32 and p32.dtype == np.float32
    ey = errors(y32, t)
    ey["gravity"] = max(ey["gravity"], vec_err(g32, g64, floors["gravity"]))
    ey["momentum"] = max(ey["momentum"], vec_err(p32, t["p64"]))
    t.update(yard=ey, y32=y32)
    return t


@functools.lru_cache(maxsize=None)
def truth(robot, compat=True):
    return build_truth(model_on(robot, "cpu", compat)._spec, *states(robot))


# --------------------------------------------------------------------------------------------- the yardstick: numpy, link-local frames
def energy_local(spec, q, qd, dt):
    """(T [B], V [B], p [B, n], dT/dq [B, n], g [B, n]) in dtype dt: the recursion of csrc/drm_energy.hpp in link-local frames.  X_i
    maps a motion of the parent's frame into link i's (w_c = E^T w_p, u_c = E^T (u_p - r x w_p)); momenta go up through X_i^T, the
    first moment as mc_p = E mc_c + m r."""
    dt = np.dtype(dt).type
    q, qd = q.astype(dt), qd.astype(dt)
    B, n = q.shape
    L = int(len(spec.parent))
    kind = getattr(spec, "kind", None)
    eye3 = np.eye(3, dtype=dt)
    moved = moved_links(spec)
    X, E_, r_, S, v, gd, zc, hC, mC, mcC = ([None] * L for _ in range(10))
    zero6, up = np.zeros((B, 6), dt), np.zeros((B, 3), dt)
    up[:, 2] = dt(GRAVITY)                                 # gravity enters as a base acceleration (0, 0, +9.81)
    order = [i for i in range(L) if spec.parent[i] >= 0]
    assert all(spec.parent[i] < i for i in order), "parents precede their children"
    dot = lambda a, b: np.einsum("bi,bi->b", a, b)
    T, V = np.zeros(B, dt), np.zeros(B, dt)
    for i in order:
        p, d = int(spec.parent[i]), int(spec.dof[i])
        E = np.broadcast_to(_rpy(spec.rpy[i], dt), (B, 3, 3))
        r = np.broadcast_to(spec.trans[i].astype(dt), (B, 3))
        if d >= 0:
            a = spec.axis[i].astype(np.float64)
            a = (a / (np.linalg.norm(a) or 1.0)).astype(dt)
            if kind is not None and int(kind[i]) == 2:
                r = r + (E @ a)[:, :] * q[:, d:d + 1]
                S[i] = np.concatenate([np.zeros(3, dt), a])
            else:
                K = _skew(a)
                sn, cs = np.sin(q[:, d])[:, None, None], np.cos(q[:, d])[:, None, None]
                E = E @ (eye3 + sn * K + (dt(1) - cs) * (K @ K))
                S[i] = np.concatenate([a, np.zeros(3, dt)])
        Et = np.swapaxes(E, -1, -2)
        Xi = np.zeros((B, 6, 6), dt)
        Xi[:, :3, :3] = Xi[:, 3:, 3:] = Et
        Xi[:, 3:, :3] = -Et @ _skew(r)
        X[i], E_[i], r_[i] = Xi, E, r
        root = v[p] is None
        vp, gp, zp = (zero6, up, np.zeros(B, dt)) if root else (v[p], gd[p], zc[p])
        v[i] = np.einsum("bij,bj->bi", Xi, vp)
        if d >= 0:
            v[i] = v[i] + S[i][None, :] * qd[:, d:d + 1]
        gd[i] = np.einsum("bij,bj->bi", Et, gp)
        zc[i] = zp + dot(gp, r) / dt(GRAVITY)
        m, c = dt(spec.mass[i]), spec.com[i].astype(dt)
        Ic = spec.inertia[i].astype(dt).reshape(3, 3)
        I = np.zeros((6, 6), dt)
        I[:3, :3] = Ic + m * ((c @ c) * eye3 - np.outer(c, c))
        I[:3, 3:] = m * _skew(c)
        I[3:, :3] = -m * _skew(c)
        I[3:, 3:] = m * eye3
        hC[i] = np.einsum("ij,bj->bi", I, v[i])
        mC[i], mcC[i] = m, np.broadcast_to(m * c, (B, 3)).copy()
        T = T + dt(0.5) * dot(v[i], hC[i])
        if moved[i]:
            V = V + (dt(GRAVITY) * m * zc[i] + dot(gd[i], mcC[i]))
    P, D, G = np.zeros((B, n), dt), np.zeros((B, n), dt), np.zeros((B, n), dt)
    for j in reversed(order):
        dj, p = int(spec.dof[j]), int(spec.parent[j])
        if dj >= 0:
            Sj = np.broadcast_to(S[j], (B, 6))
            P[:, dj] = dot(Sj, hC[j])
            D[:, dj] = dot(np.einsum("bij,bj->bi", _crm(v[j]), Sj), hC[j])
            f = np.cross(Sj[:, :3], mcC[j]) + mC[j] * Sj[:, 3:]      # the force part of IC S
            G[:, dj] = dot(f.astype(dt), gd[j])
        if X[p] is not None:
            hC[p] = hC[p] + np.einsum("bji,bj->bi", X[j], hC[j])
            mcC[p] = mcC[p] + np.einsum("bij,bj->bi", E_[j], mcC[j]) + mC[j] * r_[j]
            mC[p] = mC[p] + mC[j]
    return T, V, P, D, G


# ------------------------------------------------------------------------------------------------------------------- checks
def as_numpy(outs):
    return tuple(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x) for x in outs)


def check_all(robot, path, outs, t=None, rows=slice(None)):
    """The requirement of the module docstring on the five float32 outputs (tensors or arrays), and the sign of T."""
    t = t or truth(robot)
    outs = as_numpy(outs)
    B, n = t["p64"][rows].shape
    assert all(x.dtype == np.float32 for x in outs)
    assert outs[0].shape == outs[1].shape == (B,) and outs[2].shape == outs[3].shape == outs[4].shape == (B, n)
    e, failures = errors(outs, t, rows), []
    for name in NAMES:
        ey = max(t["yard"][name], FLOOR)
        print("ENERGY %-17s %-20s %-6s %.3e  %.3e  %.2f" % (robot, path, SHORT[name], e[name], ey, e[name] / ey))
        if not e[name] <= MARGIN * ey:
            failures.append((name, e[name], ey))
    assert not failures, failures
    assert (outs[0] >= 0).all(), "the kinetic energy is a sum of squares"


def run_model(model, robot, B=None, composed=False, inputs=None):
    """compute_energy_derivatives over the rows in consecutive launches of B rows (None: one launch)."""
    q, qd = (torch.from_numpy(x).to(model._device) for x in (inputs or states(robot)))
    N = q.shape[0]
    B = B or N
    outs = [model.compute_energy_derivatives(q[i:i + B], qd[i:i + B], _composed=composed) for i in range(0, N, B)]
    for o in outs:
        assert type(o).__name__ == "EnergyDerivatives" and o._fields == NAMES
        assert all(x.grad_fn is None and not x.requires_grad for x in o)
    return tuple(torch.cat([o[i] for o in outs]) for i in range(5))


def exact_check(model, robot, B=None, composed=False, inputs=None):
    """The exact conditions: rows at rest, the entry points that share the launch, outputs alone against outputs together."""
    from differentiable_robot_model_amd import backend
    q, qd = (torch.from_numpy(x[:B or ROWS].copy()).to(model._device) for x in (inputs or states(robot)))
    rest = torch.arange(q.shape[0], device=q.device) % 3 == 1
    qd[rest] = 0
    if composed:
        os.environ["DRM_ENERGY_COMPOSED"] = "1"
    try:
        both = model.compute_energy_derivatives(q, qd, _composed=composed)
        assert (both.kinetic[rest] == 0).all() and (both.momentum[rest] == 0).all() and (both.dkinetic_dq[rest] == 0).all()
        assert (both.kinetic >= 0).all() and (both.kinetic[~rest] > 0).all()
        energy = model.compute_energy(q, qd)
        assert type(energy).__name__ == "Energy" and energy._fields == NAMES[:2]
        assert torch.equal(energy.kinetic, both.kinetic) and torch.equal(energy.potential, both.potential)
        assert energy.kinetic.grad_fn is None and energy.potential.grad_fn is None
        assert torch.equal(model.compute_generalized_momentum(q, qd), both.momentum)
        dw = model._dynamics_walk()
        for want in [(name,) for name in NAMES] + [("kinetic", "gravity"), ("potential", "momentum", "dkinetic_dq")]:
            part = backend.energy(dw.program, model._ops_f(dw).detach(), dw.ops_i, q, qd, model._n_dofs, want=want)
            for name, x, y in zip(NAMES, part, both):
                assert (x is None) if name not in want else torch.equal(x, y), (want, name)
    finally:
        os.environ.pop("DRM_ENERGY_COMPOSED", None)


def bad_rows_check(model, device, composed=False, B=128):
    """q[5] NaN, qd[70] Inf, q[3] = 1e6: every other row keeps its bits, those three are NaN in all five outputs."""
    q, qd = (torch.from_numpy(x[:B].copy()).to(device) for x in states("panda_no_gripper"))
    run = lambda: model.compute_energy_derivatives(q, qd, _composed=composed)
    clean = run()
    q[5, 2] = float("nan")
    qd[70, 4] = float("inf")
    q[3, 1] = 1e6
    got = run()
    bad = [3, 5, 70]
    others = torch.ones(B, dtype=torch.bool, device=device)
    others[bad] = False
    for a, b in zip(got, clean):
        assert torch.equal(a[others], b[others]) and torch.isfinite(a[others]).all()
        assert torch.isnan(a[bad]).all()


def interface_check(device):
    """Unbatched inputs, B == 0, mismatched batches; results detached whatever requires grad; the definitions of p, dT/dq and g."""
    model = model_on("iiwa7", device)
    q, qd = (torch.from_numpy(x[:3].copy()).to(device) for x in states("iiwa7"))
    many = model.compute_energy_derivatives(q.clone().requires_grad_(True), qd.clone().requires_grad_(True))
    assert many.kinetic.shape == many.potential.shape == (3,) and many.momentum.shape == many.dkinetic_dq.shape == many.gravity.shape == (3, 7)
    assert all(x.grad_fn is None and not x.requires_grad and x.dtype == torch.float32 for x in many)
    one = model.compute_energy_derivatives(q[1], qd[1])
    assert one.kinetic.shape == one.potential.shape == () and one.momentum.shape == one.dkinetic_dq.shape == one.gravity.shape == (7,)
    assert all(torch.equal(a, b[1]) for a, b in zip(one, many))
    assert model.compute_generalized_momentum(q[1], qd[1]).shape == (7,)
    e1 = model.compute_energy(q[1], qd[1])
    assert e1.kinetic.shape == e1.potential.shape == () and torch.equal(e1.kinetic, many.kinetic[1])
    e = torch.empty(0, 7, device=device)
    out = model.compute_energy_derivatives(e, e)
    assert out.kinetic.shape == out.potential.shape == (0,) and out.momentum.shape == out.dkinetic_dq.shape == out.gravity.shape == (0, 7)
    assert model.compute_generalized_momentum(e, e).shape == (0, 7) and model.compute_energy(e, e).kinetic.shape == (0,)
    with pytest.raises(AssertionError):
        model.compute_energy_derivatives(q, qd[:2])
    # the definitions, to float32 rounding: p = H qd, dT/dq = C^T qd, g = the Lagrangian launch's
    lag = model.compute_lagrangian_dynamics(q, qd)
    assert torch.allclose(many.momentum, torch.einsum("bij,bj->bi", lag.inertia, qd), atol=2e-5)
    assert torch.allclose(many.dkinetic_dq, torch.einsum("bji,bj->bi", lag.coriolis, qd), atol=5e-5)
    assert torch.allclose(many.gravity, lag.gravity, atol=2e-5)
    assert torch.allclose(many.kinetic, 0.5 * torch.einsum("bi,bi->b", many.momentum, qd), atol=2e-5)


def autograd_check(device, path, robot="panda_no_gripper"):
    """compute_energy under autograd: the gradients are a dT/dq + b g and a p to the bit, meet the truth, and are first order only."""
    model, t = model_on(robot, device), truth(robot)
    q0, qd0 = (torch.from_numpy(x).to(device) for x in states(robot))
    gen = torch.Generator().manual_seed(7)
    a, b = (torch.rand(ROWS, generator=gen).add_(0.5).to(device) for _ in range(2))
    q, qd = q0.clone().requires_grad_(True), qd0.clone().requires_grad_(True)
    energy = model.compute_energy(q, qd)
    assert energy.kinetic.grad_fn is not None and energy.potential.grad_fn is not None
    gq, gqd = torch.autograd.grad((a * energy.kinetic + b * energy.potential).sum(), (q, qd))
    d = model.compute_energy_derivatives(q0, qd0)
    assert torch.equal(energy.kinetic.detach(), d.kinetic) and torch.equal(energy.potential.detach(), d.potential)
    assert torch.equal(gq, a[:, None] * d.dkinetic_dq + b[:, None] * d.gravity) and torch.equal(gqd, a[:, None] * d.momentum)
    a64, b64 = (x.cpu().numpy().astype(np.float64)[:, None] for x in (a, b))
    a32, b32 = (x.cpu().numpy()[:, None] for x in (a, b))
    _, _, p32, dT32, g32 = t["y32"]
    for what, got, want, yard in (("grad_q", gq, a64 * t["dT64"] + b64 * t["g64"], a32 * dT32 + b32 * g32), ("grad_qd", gqd, a64 * t["p64"], a32 * p32)):
        e, ey = vec_err(got.cpu().numpy(), want), max(vec_err(yard, want), FLOOR)
        print("ENERGY %-17s %-20s %-6s %.3e  %.3e  %.2f" % (robot, path, what, e, ey, e / ey))
        assert e <= MARGIN * ey
    # one of the two inputs alone
    e2 = model.compute_energy(q0, qd)
    (only,) = torch.autograd.grad(e2.kinetic.sum(), (qd,))
    assert torch.equal(only, d.momentum)
    # first order only
    e3 = model.compute_energy(q, qd)
    (g1,) = torch.autograd.grad(e3.kinetic.sum(), (q,), create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    # nothing requires grad: no graph
    with torch.no_grad():
        e4 = model.compute_energy(q, qd)
    e5 = model.compute_energy(q0, qd0)
    assert all(x.grad_fn is None and not x.requires_grad for x in tuple(e4) + tuple(e5))
    assert torch.equal(e4.kinetic, d.kinetic) and torch.equal(e5.potential, d.potential)


def c_abi_check(lib, robot, device, stream, B=ROWS):
    """Straight through the C ABI: q, qd and the five outputs 4 bytes off a 16-byte boundary (the general kernel on the device)
    against the aligned call, a scratch of exactly drm_energy_scratch_floats floats, guard words behind the scratch and on both sides
    of every output; the error codes."""
    model = model_on(robot, device)
    walk, n = walk_of(model), model._n_dofs
    sync = (lambda: None) if device == "cpu" else torch.cuda.synchronize
    GUARD = 64

    def shifted(x, off):
        """a copy of x whose first element lies `off` floats past a 16-byte boundary"""
        buf = torch.zeros(x.numel() + 4, device=device)
        lead = (off - buf.data_ptr() // 4) % 4
        buf[lead:lead + x.numel()] = x.reshape(-1)
        view = buf[lead:lead + x.numel()].view(x.shape)
        assert view.data_ptr() % 16 == 4 * off
        return view

    def call(off, flags=0, rows=B, which=(True,) * 5, q_null=False, qd_null=False):
        q, qd = (shifted(torch.from_numpy(x[:B].copy()).to(device), off) for x in states(robot))
        query = lib.drm_energy_scratch_floats if off else lib.drm_energy_scratch_floats_aligned
        need = int(query(ctypes.byref(walk), max(rows, 0)))
        scratch = torch.full((need + GUARD,), 3.25, device=device)
        sizes = (B, B, B * n, B * n, B * n)
        bufs, outs = [], []
        for s in sizes:
            buf = torch.full((s + 2 * GUARD + 4,), -1.5, device=device)
            lead = GUARD + (off - (buf.data_ptr() // 4 + GUARD)) % 4
            bufs.append((buf, lead, s))
            outs.append(buf[lead:lead + s])
            assert outs[-1].data_ptr() % 16 == 4 * off
        rc = lib.drm_energy(ctypes.byref(walk), None if q_null else q.data_ptr(), None if qd_null else qd.data_ptr(), rows, flags,
                            *[o.data_ptr() if w else None for o, w in zip(outs, which)], scratch.data_ptr(), stream)
        sync()
        assert (scratch[need:] == 3.25).all()
        for (buf, lead, s), w in zip(bufs, which):
            assert (buf[:lead] == -1.5).all() and (buf[lead + s:] == -1.5).all()
            if not w or rc != 0 or rows <= 0:
                assert (buf == -1.5).all()
        shapes = ((B,), (B,), (B, n), (B, n), (B, n))
        return rc, tuple(o.clone().view(sh) for o, sh in zip(outs, shapes)), need

    assert lib.drm_abi_version() == 15
    rc, aligned, _ = call(0)
    assert rc == 0
    rc, off4, need = call(1)
    assert rc == 0 and all(torch.isfinite(x).all() for x in off4)
    if B == ROWS:
        check_all(robot, "abi-aligned", aligned)
        check_all(robot, "abi-misaligned", off4)
    if device != "cpu":
        assert (need > 0) == (robot == "iiwa7_allegro")
    # each output alone, to the bit; none at all is an error
    for i in range(5):
        rc, part, _ = call(0, which=tuple(j == i for j in range(5)))
        assert rc == 0 and torch.equal(part[i], aligned[i])
    assert call(0, which=(False,) * 5)[0] == -1
    assert call(0, rows=0)[0] == 0
    assert call(0, rows=-1)[0] == -1
    assert call(0, q_null=True)[0] == -1 and call(0, qd_null=True)[0] == -1


def long_chain_check(tmp_path, device, path):
    """test_max_sizes.chain_model's 30-joint chain (joints about +-x / +-y / +-z), 65 rows."""
    from helpers import sample_states
    from test_max_sizes import chain_model
    model = chain_model(tmp_path, 30, device)
    q, qd, _ = sample_states(model, 65, seed=0)
    check_all("chain30", path, run_model(model, "chain30", inputs=(q, qd)), t=build_truth(model._spec, q, qd))
    exact_check(model, "chain30", inputs=(q, qd))
    return model


def skew_check(tmp_path_factory, device, path):
    """tests/test_joint_models.py's toy robot: prismatic about z, revolute and prismatic about skew axes (two ops per skew link)."""
    from helpers import sample_states
    from test_joint_models import toy_model, toy_urdf
    urdf = tmp_path_factory.mktemp("toy_energy") / "toy.urdf"
    urdf.write_text(toy_urdf())
    model = toy_model(str(urdf), device)
    assert model._spec.skew.any()
    q, qd, _ = sample_states(model, 65, seed=1)
    check_all("toy_skew", path, run_model(model, "toy_skew", inputs=(q, qd)), t=build_truth(model._spec, q, qd))


def fixed_learnable_check(device, path):
    """A link that no joint moves, kept as an op of its own because it is learnable: V leaves it out, as the truth does; and a moved
    learnable link enters with its current value."""
    import dataclasses
    from differentiable_robot_model_amd.rigid_body_params import UnconstrainedTensor
    robot = "fetch"
    model = load_model(robot, device)
    spec = model._spec
    still = [i for i in range(1, len(spec.parent)) if not moved_links(spec)[i] and spec.mass[i] > 0]
    assert still, "fetch carries fixed links with mass on its base"
    moving = max(i for i in range(len(spec.parent)) if spec.dof[i] >= 0)
    new_trans = spec.trans.copy()
    for idx in (still[0], moving):
        new_trans[idx] = spec.trans[idx] + np.asarray([0.03, -0.02, 0.05], np.float32)
        model.make_link_param_learnable(spec.link_names[idx], "trans", UnconstrainedTensor(dim1=1, dim2=3, init_tensor=torch.from_numpy(new_trans[idx])))
    assert spec.link_names[still[0]] in model.regressor_links()
    t = build_truth(dataclasses.replace(spec, trans=new_trans), *states(robot))
    assert vec_err(t["g64"], truth(robot)["g64"]) > 1e-3           # (the moved link changes the answer)
    check_all(robot, path, run_model(model, robot), t=t)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("robot", ARMS + OTHERS)
def test_host_build_against_truth(cpu_library, robot):
    model = model_on(robot)
    check_all(robot, "host", run_model(model, robot))
    exact_check(model, robot)


def test_host_composed_flag_is_accepted(cpu_library):
    model = model_on("panda_no_gripper")
    a, b = run_model(model, "panda_no_gripper"), run_model(model, "panda_no_gripper", composed=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))      # (the host build has one path)
    exact_check(model, "panda_no_gripper", composed=True)


def test_fetch_with_sliding_joints(cpu_library):
    model = model_on("fetch", "cpu", False)
    assert (model._spec.kind == 2).any()
    check_all("fetch", "host-prismatic", run_model(model, "fetch"), t=truth("fetch", False))


def test_skew_axis_model(cpu_library, tmp_path_factory):
    skew_check(tmp_path_factory, "cpu", "host")


def test_interface(cpu_library):
    interface_check("cpu")


def test_exports():
    import differentiable_robot_model_amd as drm
    from differentiable_robot_model_amd import backend
    assert drm.EnergyDerivatives._fields == NAMES and drm.Energy._fields == NAMES[:2]
    assert {"drm_energy", "drm_energy_scratch_floats", "drm_energy_scratch_floats_aligned"} <= set(backend.EXPORTS)
    assert backend.ENERGY_COMPOSED == 512


@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7_allegro"])
def test_c_abi_on_the_host_build(cpu_library, robot):
    c_abi_check(cpu_library, robot, "cpu", None)


def test_non_finite_rows(cpu_library):
    bad_rows_check(model_on("panda_no_gripper"), "cpu")


def test_autograd(cpu_library):
    autograd_check("cpu", "host-autograd")


def test_fixed_and_moved_learnable_links(cpu_library):
    fixed_learnable_check("cpu", "host-learnable")


def test_long_chain(cpu_library, tmp_path):
    long_chain_check(tmp_path, "cpu", "host")


# ------------------------------------------------------------------------------------------------------------------- GPU
def gpu_run_and_check(robot, B, composed=False, compat=True, path=None):
    model = model_on(robot, "cuda:0", compat)
    out = run_model(model, robot, B=B, composed=composed)
    torch.cuda.synchronize()
    name = path or ("general" if composed or robot not in ARMS or B < 64 else "fused") + "-B%d" % B
    check_all(robot, name, out, t=truth(robot, compat))
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 128, 131])
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_against_truth(robot, B):
    model = gpu_run_and_check(robot, B)
    exact_check(model, robot, B=B)


@pytest.mark.gpu
def test_gpu_arm_general_kernel():
    model = gpu_run_and_check("panda_no_gripper", 128, composed=True)
    exact_check(model, "panda_no_gripper", composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", OTHERS)
def test_gpu_other_robots_against_truth(robot):
    model = gpu_run_and_check(robot, 65)
    exact_check(model, robot, B=65)


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
    assert backend.load_library().drm_energy_scratch_floats(ctypes.byref(walk_of(model)), 65) > 0


@pytest.mark.gpu
def test_gpu_persistent_grid_beyond_2048_tiles(tmp_path):
    from test_lagrangian import persistent_grid_check
    persistent_grid_check(tmp_path, "drm_energy_scratch_floats_aligned", lambda m, q, qd: m.compute_energy_derivatives(q, qd))


@pytest.mark.gpu
def test_gpu_interface():
    interface_check("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7_allegro"])
def test_gpu_c_abi(robot):
    from differentiable_robot_model_amd import backend
    c_abi_check(backend.load_library(), robot, "cuda", backend._stream(torch.device("cuda:0")))


@pytest.mark.gpu
def test_gpu_c_abi_ragged_batch():
    from differentiable_robot_model_amd import backend
    c_abi_check(backend.load_library(), "panda_no_gripper", "cuda", backend._stream(torch.device("cuda:0")), B=67)


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_non_finite_rows(composed):
    bad_rows_check(model_on("panda_no_gripper", "cuda:0"), "cuda", composed=composed)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_autograd():
    autograd_check("cuda:0", "fused-autograd")


@pytest.mark.gpu
def test_gpu_fixed_and_moved_learnable_links():
    fixed_learnable_check("cuda:0", "learnable")

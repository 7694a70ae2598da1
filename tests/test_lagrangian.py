"""H(q), the Coriolis matrix C(q, qd) and g(q) in one call (csrc/drm_lagrangian.hip, include/drm_hip.h drm_lagrangian_dynamics;
DifferentiableRobotModel.compute_lagrangian_dynamics / compute_coriolis_matrix):  H qdd + C qd + g = tau, C the Christoffel matrix.

INPUTS: the first 128 rows of q and qd per robot of tests/golden/golden_fd_derivatives.npz.

TRUTH, from the fp64 oracle only: H64 = Oracle.mass_matrix, g64 = Oracle.rnea(q, 0, 0, gravity), C64[i, j] = sum_k Gamma_ijk qd_k with
Gamma_ijk = (dH_ij/dq_k + dH_ik/dq_j - dH_jk/dq_i) / 2 from central differences of H64 at h = 1e-4 and 3e-4, Richardson-combined as
(9 C_h - C_3h) / 8.  Before anything under test is compared the truth must satisfy max|C64 qd + g64 - rnea64(q, qd, 0)| <= 1e-9 max|tau|.

YARDSTICK for C, not code under test: the recursion of Echeandia and Wensing (2021) restated HERE in numpy in link-local frames
(Featherstone's convention, spatial vectors [angular; linear] at each link's origin), run in float32.  Run in fp64 it must first match
C64 to 1e-8 relative: that proves the yardstick is the right formula.  Yardsticks for H, g and C qd + g: the oracle's own float32
mass_matrix / rnea.  REQUIREMENT throughout: err(path) <= 8 max(err(yardstick), 2^-23); 8 is the project's margin for a different
summation order (tests/test_regressor.py, tests/test_fd_derivatives.py, tests/test_operational_space.py).
    C           per-row max|C - C64| / max|C64| over the row's matrix, worst over rows
    C qd + g    summed in fp64 from the float32 outputs, max|. - rnea64(q, qd, 0)| / max|tau|
    H, g        per-row max|X - X64| / max|X64|, worst over rows
    C + C^T     against (H64(q + h qd) - H64(q - h qd)) / 2h, Richardson as above; the yardstick of C, doubled
Entries of H64 that are zero in every row must be exactly 0.0 in H, and in C where C64 is zero in every row too; that set must hold
every pair of joints on different branches (H64 also vanishes between crossing perpendicular axes of one finger, where C64 does not).
Every comparison prints one "LAG" line (robot, path, quantity, error, yardstick, ratio) before it asserts; profiles/lagrangian_tests.txt
holds them for the host build and the MI355X.

GPU (-m gpu): a launch of B rows is repeated over consecutive slices of the 128 rows, so the statistic is over the same rows whatever
B is.  64-row tiles: B = 64 and 128 are the fused arm kernel, 65 and 131 a fused part plus a ragged tail in the general kernel, 1 the
general kernel alone.  test_max_sizes.chain_model's 30-joint chain at 65 rows is a size at which the general kernel's per-row records
leave LDS for the scratch.

Measured (profiles/lagrangian_tests.txt): the worst err / yardstick is 1.35 on the host build and 1.39 on the MI355X for C (iiwa + Allegro,
Fetch), 0.96 on both for C qd + g (iiwa7), 4.4 and 6.2 for C + C^T (the two-link robot, whose yardstick sits at the 2^-23 floor).
"""
import ctypes
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
GRAVITY = 9.81


@functools.lru_cache(maxsize=None)
def model_on(robot, device="cpu", compat=True):
    return load_model(robot, device, reference_compat=compat)


@functools.lru_cache(maxsize=None)
def states(robot):
    g = np.load(os.path.join(GOLDEN_DIR, "golden_fd_derivatives.npz"), allow_pickle=False)
    return g[robot + "/q"][:ROWS], g[robot + "/qd"][:ROWS]


# ------------------------------------------------------------------------------------------------------------------- truth
def christoffel_from_oracle(orc, q, qd, h):
    """C [B, n, n] fp64 from central differences of the oracle's fp64 H at step h."""
    B, n = q.shape
    D = np.empty((B, n, n, n))                             # D[b, i, j, k] = dH_ij / dq_k
    for k in range(n):
        e = np.zeros(n)
        e[k] = h
        D[:, :, :, k] = (orc.mass_matrix(q + e, True, False, np.float64) - orc.mass_matrix(q - e, True, False, np.float64)) / (2 * h)
    G = 0.5 * (D + D.transpose(0, 1, 3, 2) - D.transpose(0, 3, 1, 2))      # G[i, j, k]: D[i,j,k] + D[i,k,j] - D[j,k,i]
    return np.einsum("bijk,bk->bij", G, qd)


def hdot_from_oracle(orc, q, qd, h):
    return (orc.mass_matrix(q + h * qd, True, False, np.float64) - orc.mass_matrix(q - h * qd, True, False, np.float64)) / (2 * h)


def richardson(f, h=1e-4):
    return (9.0 * f(h) - f(3.0 * h)) / 8.0


def build_truth(spec, q, qd):
    orc = Oracle(spec)
    q64, qd64, z = q.astype(np.float64), qd.astype(np.float64), np.zeros(q.shape)
    H64 = orc.mass_matrix(q64, True, False, np.float64)
    g64 = orc.rnea(q64, z, z, True, False, np.float64)
    C64 = richardson(lambda h: christoffel_from_oracle(orc, q64, qd64, h))
    Hd64 = richardson(lambda h: hdot_from_oracle(orc, q64, qd64, h))
    tau64 = orc.rnea(q64, qd64, z, True, False, np.float64)
    pin = np.abs(np.einsum("bij,bj->bi", C64, qd64) + g64 - tau64).max()
    assert pin <= 1e-9 * np.abs(tau64).max(), pin          # the truth itself, before anything under test
    H32 = orc.mass_matrix(q, True, False, np.float32)
    g32 = orc.rnea(q, z.astype(np.float32), z.astype(np.float32), True, False, np.float32)
    tau32 = orc.rnea(q, qd, z.astype(np.float32), True, False, np.float32)
    assert H32.dtype == np.float32 and tau32.dtype == np.float32
    # the yardstick of C: the recursion in link-local frames; in fp64 it must be the truth
    _, Cl64, _ = lagrangian_local(spec, q, qd, np.float64)
    assert row_err(Cl64, C64) <= 1e-8, row_err(Cl64, C64)
    _, C32, _ = lagrangian_local(spec, q, qd, np.float32)
    assert C32.dtype == np.float32
    return dict(H64=H64, g64=g64, C64=C64, Hd64=Hd64, tau64=tau64, H32=H32, g32=g32, C32=C32, tau32=tau32,
                dead=np.abs(H64).max(axis=0) == 0, deadC=(np.abs(H64).max(axis=0) == 0) & (np.abs(C64).max(axis=0) == 0),
                apart=different_branches(spec))


def different_branches(spec):
    """[n, n] bool: joints i and j lie on different branches (neither link is on the other's path to the root)."""
    n = int(max(spec.dof)) + 1
    link = {int(d): i for i, d in enumerate(spec.dof) if d >= 0}
    path = lambda i: set(spec.chain_to(i))
    return np.array([[link[i] not in path(link[j]) and link[j] not in path(link[i]) for j in range(n)] for i in range(n)])


@functools.lru_cache(maxsize=None)
def truth(robot, compat=True):
    return build_truth(model_on(robot, "cpu", compat)._spec, *states(robot))


# --------------------------------------------------------------------------------------------- the yardstick: numpy, link-local frames
def _skew(v):
    S = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    S[..., 0, 1], S[..., 0, 2], S[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    S[..., 1, 2], S[..., 2, 0], S[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    return S


def _crm(v):
    """motion cross product matrix of v = [w; u] [B, 6]"""
    M = np.zeros(v.shape[:-1] + (6, 6), v.dtype)
    M[..., :3, :3] = M[..., 3:, 3:] = _skew(v[..., :3])
    M[..., 3:, :3] = _skew(v[..., 3:])
    return M


def _crf(v):
    return -np.swapaxes(_crm(v), -1, -2)


def _bar(f):
    """bar(f) v = crf(v) f for f = [n; l]"""
    M = np.zeros(f.shape[:-1] + (6, 6), f.dtype)
    M[..., :3, :3] = -_skew(f[..., :3])
    M[..., :3, 3:] = M[..., 3:, :3] = -_skew(f[..., 3:])
    return M


def _rpy(rpy, dt):
    r, p, y = (dt(v) for v in rpy)
    c, s = np.cos, np.sin
    Rx = np.array([[1, 0, 0], [0, c(r), -s(r)], [0, s(r), c(r)]], dt)
    Ry = np.array([[c(p), 0, s(p)], [0, 1, 0], [-s(p), 0, c(p)]], dt)
    Rz = np.array([[c(y), -s(y), 0], [s(y), c(y), 0], [0, 0, 1]], dt)
    return Rz @ Ry @ Rx


def lagrangian_local(spec, q, qd, dt):
    """(H [B, n, n], C [B, n, n], g [B, n]) in dtype dt: the recursion of the issue in link-local frames.  X_i maps a motion of the
    parent's frame into link i's (w_c = E^T w_p, u_c = E^T (u_p - r x w_p)); forces and the composites go up through X_i^T."""
    dt = np.dtype(dt).type
    q, qd = q.astype(dt), qd.astype(dt)
    B, n = q.shape
    L = int(len(spec.parent))
    kind = getattr(spec, "kind", None)
    eye3 = np.eye(3, dtype=dt)
    X, S, v, a0, IC, BC = [None] * L, [None] * L, [None] * L, [None] * L, [None] * L, [None] * L
    zero6 = np.zeros((B, 6), dt)
    grav = np.zeros((B, 6), dt)
    grav[:, 5] = dt(GRAVITY)                               # gravity enters as a base acceleration (0, 0, +9.81)
    order = [i for i in range(L) if spec.parent[i] >= 0]
    assert all(spec.parent[i] < i for i in order), "parents precede their children"
    for i in order:
        p, d = int(spec.parent[i]), int(spec.dof[i])
        E = np.broadcast_to(_rpy(spec.rpy[i], dt), (B, 3, 3))
        r = np.broadcast_to(spec.trans[i].astype(dt), (B, 3))
        S[i] = None
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
        X[i] = Xi
        vp, ap = (v[p], a0[p]) if p > 0 or v[p] is not None else (zero6, grav)
        v[i] = np.einsum("bij,bj->bi", Xi, vp)
        if d >= 0:
            v[i] = v[i] + S[i][None, :] * qd[:, d:d + 1]
        a0[i] = np.einsum("bij,bj->bi", Xi, ap)
        m, c = dt(spec.mass[i]), spec.com[i].astype(dt)
        Ic = spec.inertia[i].astype(dt).reshape(3, 3)
        I = np.zeros((6, 6), dt)
        I[:3, :3] = Ic + m * ((c @ c) * eye3 - np.outer(c, c))
        I[:3, 3:] = m * _skew(c)
        I[3:, :3] = -m * _skew(c)
        I[3:, 3:] = m * eye3
        IC[i] = np.broadcast_to(I, (B, 6, 6)).copy()
        Iv = np.einsum("ij,bj->bi", I, v[i])
        BC[i] = dt(0.5) * (_crf(v[i]) @ I - I @ _crm(v[i]) + _bar(Iv))
    H, C, g = np.zeros((B, n, n), dt), np.zeros((B, n, n), dt), np.zeros((B, n), dt)
    dot = lambda a, b: np.einsum("bi,bi->b", a, b)
    for j in reversed(order):
        dj, p = int(spec.dof[j]), int(spec.parent[j])
        if dj >= 0:
            Sj = np.broadcast_to(S[j], (B, 6))
            Sdj = np.einsum("bij,bj->bi", _crm(v[j]), Sj)
            F1 = np.einsum("bij,bj->bi", IC[j], Sdj) + np.einsum("bij,bj->bi", BC[j], Sj)
            F2 = np.einsum("bij,bj->bi", IC[j], Sj)
            F3 = np.einsum("bji,bj->bi", BC[j], Sj)
            g[:, dj] = dot(F2, a0[j])
            i = j
            while i > 0 and X[i] is not None:
                di = int(spec.dof[i])
                if di >= 0:
                    Si = np.broadcast_to(S[i], (B, 6))
                    H[:, di, dj] = H[:, dj, di] = dot(Si, F2)
                    C[:, di, dj] = dot(Si, F1)
                    if i != j:
                        Sdi = np.einsum("bij,bj->bi", _crm(v[i]), Si)
                        C[:, dj, di] = dot(Sdi, F2) + dot(Si, F3)
                F1, F2, F3 = (np.einsum("bji,bj->bi", X[i], F) for F in (F1, F2, F3))
                i = int(spec.parent[i])
        if p > 0 or X[p] is not None:
            Xt = np.swapaxes(X[j], -1, -2)
            IC[p] = IC[p] + Xt @ IC[j] @ X[j]
            BC[p] = BC[p] + Xt @ BC[j] @ X[j]
    return H, C, g


# ------------------------------------------------------------------------------------------------------------------- metrics
def row_err(X, T):
    """per-row max|X - T| / max|T| over the row's entries, worst over rows"""
    X, T = np.asarray(X, np.float64), np.asarray(T, np.float64)
    ax = tuple(range(1, T.ndim))
    scale = np.abs(T).max(axis=ax)
    live = scale > 0
    return float((np.abs(X - T).max(axis=ax)[live] / scale[live]).max()) if live.any() else 0.0


def report(robot, path, what, e, ey):
    print("LAG %-17s %-20s %-8s %.3e  %.3e  %.2f" % (robot, path, what, e, ey, e / ey))


def check_all(robot, path, H, C, g, t=None, inputs=None, rows=slice(None)):
    """Requirements 1 - 5 of the module docstring on float32 outputs (tensors or arrays)."""
    t = t or truth(robot)
    q, qd = inputs or states(robot)
    H, C, g = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (H, C, g))
    B, n = q[rows].shape
    assert H.dtype == C.dtype == g.dtype == np.float32 and H.shape == C.shape == (B, n, n) and g.shape == (B, n)
    qd64 = qd[rows].astype(np.float64)
    failures = []

    def rule(what, e, ey):
        ey = max(ey, FLOOR)
        report(robot, path, what, e, ey)
        if not e <= MARGIN * ey:
            failures.append((what, e, ey))
    eyC = row_err(t["C32"][rows], t["C64"][rows])
    rule("C", row_err(C, t["C64"][rows]), eyC)
    scale = np.abs(t["tau64"][rows]).max()
    nle = np.einsum("bij,bj->bi", C.astype(np.float64), qd64) + g.astype(np.float64)
    rule("Cqd+g", np.abs(nle - t["tau64"][rows]).max() / scale, np.abs(t["tau32"][rows] - t["tau64"][rows]).max() / scale)
    rule("H", row_err(H, t["H64"][rows]), row_err(t["H32"][rows], t["H64"][rows]))
    rule("g", row_err(g, t["g64"][rows]), row_err(t["g32"][rows], t["g64"][rows]))
    C64f = C.astype(np.float64)
    rule("C+C^T", row_err(C64f + C64f.transpose(0, 2, 1), t["Hd64"][rows]), 2.0 * max(eyC, FLOOR))
    assert not failures, failures
    # H64 is also identically zero between some joints of ONE branch (crossing perpendicular axes of a finger) where C64 is not: C must be
    # exactly zero where H64 AND C64 are identically zero, which must cover every pair of joints on different branches
    assert (t["apart"] <= t["deadC"]).all() and (t["deadC"] <= t["dead"]).all()
    assert (H[:, t["dead"]] == 0).all() and (C[:, t["deadC"]] == 0).all(), "entries between different branches must be exactly zero"
    assert np.array_equal(H, H.transpose(0, 2, 1))


def run_model(model, robot, B=None, composed=False, inputs=None):
    """compute_lagrangian_dynamics over the rows in consecutive launches of B rows (None: one launch)."""
    q, qd = (torch.from_numpy(x).to(model._device) for x in (inputs or states(robot)))
    N = q.shape[0]
    B = B or N
    outs = [model.compute_lagrangian_dynamics(q[i:i + B], qd[i:i + B], _composed=composed) for i in range(0, N, B)]
    for o in outs:
        assert type(o).__name__ == "LagrangianDynamics" and o._fields == ("inertia", "coriolis", "gravity")
        assert all(x.grad_fn is None and not x.requires_grad for x in o)
    return tuple(torch.cat([o[i] for o in outs]) for i in range(3))


def coriolis_alone_check(model, robot, B=None, composed=False):
    """Requirement 6: compute_coriolis_matrix is bit-equal to .coriolis of the same path."""
    q, qd = (torch.from_numpy(x[:B or ROWS]).to(model._device) for x in states(robot))
    both = model.compute_lagrangian_dynamics(q, qd, _composed=composed).coriolis
    if composed:
        os.environ["DRM_LAGRANGIAN_COMPOSED"] = "1"
    try:
        alone = model.compute_coriolis_matrix(q, qd)
    finally:
        os.environ.pop("DRM_LAGRANGIAN_COMPOSED", None)
    assert torch.equal(alone, both) and alone.grad_fn is None


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("robot", ARMS + OTHERS)
def test_host_build_against_truth(cpu_library, robot):
    model = model_on(robot)
    check_all(robot, "host", *run_model(model, robot))
    coriolis_alone_check(model, robot)


def test_host_composed_flag_is_accepted(cpu_library):
    model = model_on("panda_no_gripper")
    a, b = run_model(model, "panda_no_gripper"), run_model(model, "panda_no_gripper", composed=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))      # (the host build has one path)


def test_fetch_with_sliding_joints(cpu_library):
    model = model_on("fetch", "cpu", False)
    assert (model._spec.kind == 2).any()
    check_all("fetch", "host-prismatic", *run_model(model, "fetch"), t=truth("fetch", False))


def skew_check(tmp_path_factory, device, path):
    """tests/test_joint_models.py's toy robot: prismatic about z, revolute and prismatic about skew axes (two ops per skew link)."""
    from helpers import sample_states
    from test_joint_models import toy_model, toy_urdf
    urdf = tmp_path_factory.mktemp("toy_lag") / "toy.urdf"
    urdf.write_text(toy_urdf())
    model = toy_model(str(urdf), device)
    assert model._spec.skew.any()
    q, qd, _ = sample_states(model, 65, seed=1)
    t = build_truth(model._spec, q, qd)
    check_all("toy_skew", path, *run_model(model, "toy_skew", inputs=(q, qd)), t=t, inputs=(q, qd))


def test_skew_axis_model(cpu_library, tmp_path_factory):
    skew_check(tmp_path_factory, "cpu", "host")


def interface_check(device):
    """Requirement 9: unbatched inputs, B == 0, mismatched batches; results detached whatever requires grad."""
    model = model_on("iiwa7", device)
    q, qd = (torch.from_numpy(x[:3].copy()).to(device) for x in states("iiwa7"))
    many = model.compute_lagrangian_dynamics(q.clone().requires_grad_(True), qd.clone().requires_grad_(True))
    assert many.inertia.shape == many.coriolis.shape == (3, 7, 7) and many.gravity.shape == (3, 7)
    assert all(x.grad_fn is None and not x.requires_grad and x.dtype == torch.float32 for x in many)
    one = model.compute_lagrangian_dynamics(q[1], qd[1])
    assert one.inertia.shape == one.coriolis.shape == (7, 7) and one.gravity.shape == (7,)
    assert all(torch.equal(a, b[1]) for a, b in zip(one, many))
    assert model.compute_coriolis_matrix(q[1], qd[1]).shape == (7, 7)
    e = torch.empty(0, 7, device=device)
    out = model.compute_lagrangian_dynamics(e, e)
    assert out.inertia.shape == out.coriolis.shape == (0, 7, 7) and out.gravity.shape == (0, 7)
    assert model.compute_coriolis_matrix(e, e).shape == (0, 7, 7)
    with pytest.raises(AssertionError):
        model.compute_lagrangian_dynamics(q, qd[:2])
    # the definitions: inertia is compute_lagrangian_inertia_matrix, gravity the inverse dynamics at rest, to float32 rounding
    H = model.compute_lagrangian_inertia_matrix(q)
    g = model.compute_inverse_dynamics(q, torch.zeros_like(q), torch.zeros_like(q), include_gravity=True, use_damping=False)
    nle = model.compute_non_linear_effects(q, qd, True, False)
    assert torch.allclose(many.inertia, H, atol=1e-5) and torch.allclose(many.gravity, g, atol=2e-5)
    assert torch.allclose(torch.einsum("bij,bj->bi", many.coriolis, qd) + many.gravity, nle, atol=5e-5)


def test_interface(cpu_library):
    interface_check("cpu")


def walk_of(model):
    from differentiable_robot_model_amd import backend
    dw = model._dynamics_walk()
    return backend._walk_struct(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs)


def c_abi_null_check(lib, model, device, stream, B=5):
    """Requirement 8: each of H, C, g NULL in turn gives the other two to the bit; all three NULL is DRM_ERR_INVALID; B == 0 is DRM_OK."""
    walk, n = walk_of(model), model._n_dofs
    q, qd = (torch.from_numpy(x[:B].copy()).to(device) for x in states("panda_no_gripper"))
    need = int(lib.drm_lagrangian_dynamics_scratch_floats(ctypes.byref(walk), B))
    scratch = torch.empty(max(need, 1), device=device)
    sizes = (B * n * n, B * n * n, B * n)

    def call(which, a=None, b=None, rows=B):
        outs = [torch.full((s + 8,), 7.5, device=device) for s in sizes]
        ptr = [o.data_ptr() if w else None for o, w in zip(outs, which)]
        rc = lib.drm_lagrangian_dynamics(ctypes.byref(walk), q.data_ptr() if a is None else a, qd.data_ptr() if b is None else b, rows, 0,
                                         ptr[0], ptr[1], ptr[2], scratch.data_ptr(), stream)
        if device != "cpu":
            torch.cuda.synchronize()
        return rc, outs
    rc, full = call((True, True, True))
    assert rc == 0
    for o, s in zip(full, sizes):
        assert (o[s:] == 7.5).all() and torch.isfinite(o[:s]).all()
    for drop in range(3):
        which = tuple(i != drop for i in range(3))
        rc, part = call(which)
        assert rc == 0
        for i in range(3):
            assert torch.equal(part[i], full[i]) if which[i] else (part[i] == 7.5).all()
    assert call((False, False, False))[0] == -1
    rc, outs = call((True, True, True), rows=0)
    assert rc == 0 and all((o == 7.5).all() for o in outs)
    assert call((True, True, True), rows=-1)[0] == -1
    assert lib.drm_lagrangian_dynamics(ctypes.byref(walk), None, qd.data_ptr(), B, 0, full[0].data_ptr(), None, None, None, stream) == -1
    assert lib.drm_lagrangian_dynamics(ctypes.byref(walk), q.data_ptr(), None, B, 0, full[0].data_ptr(), None, None, None, stream) == -1


def test_c_abi_codes_on_the_host_build(cpu_library):
    from differentiable_robot_model_amd import backend
    lib = backend.load_library(kind="cpu")
    assert lib.drm_abi_version() == 15
    c_abi_null_check(lib, model_on("panda_no_gripper"), "cpu", None)


def bad_rows_check(model, device, composed=False, B=128):
    """Requirement 7: q[5] NaN, qd[70] Inf, q[3] = 2e9: every other row keeps its bits, those three are non-finite."""
    q, qd = (torch.from_numpy(x[:B].copy()).to(device) for x in states("panda_no_gripper"))
    run = lambda: model.compute_lagrangian_dynamics(q, qd, _composed=composed)
    clean = run()
    q[5, 2] = float("nan")
    qd[70, 4] = float("inf")
    q[3, 1] = 2e9
    got = run()
    bad = [3, 5, 70]
    others = torch.ones(B, dtype=torch.bool, device=device)
    others[bad] = False
    for a, b in zip(got, clean):
        assert torch.equal(a[others], b[others])
    for r in bad:
        assert not any(torch.isfinite(x[r]).any() for x in got)


def test_non_finite_rows(cpu_library):
    bad_rows_check(model_on("panda_no_gripper"), "cpu")


def learnable_check(device, path):
    """A model with one learnable link whose parameter has moved: the current values, detached results, no graph."""
    import dataclasses
    from differentiable_robot_model_amd.rigid_body_params import UnconstrainedTensor
    robot, link = "panda_no_gripper", "panda_link5"
    model = load_model(robot, device)
    idx = model._name_to_idx_map[link]
    trans = model._spec.trans[idx] + np.asarray([0.03, -0.02, 0.05], np.float32)
    model.make_link_param_learnable(link, "trans", UnconstrainedTensor(dim1=1, dim2=3, init_tensor=torch.from_numpy(trans)))
    new_trans = model._spec.trans.copy()
    new_trans[idx] = trans
    spec = dataclasses.replace(model._spec, trans=new_trans)
    t = build_truth(spec, *states(robot))
    assert row_err(t["C64"], truth(robot)["C64"]) > 1e-3       # (the moved link changes the answer)
    check_all(robot, path, *run_model(model, robot), t=t)


def test_learnable_link(cpu_library):
    learnable_check("cpu", "host-learnable")


def long_chain_check(tmp_path, device, path):
    """test_max_sizes.chain_model's 30-joint chain (joints about +-x / +-y / +-z), 65 rows."""
    from helpers import sample_states
    from test_max_sizes import chain_model
    model = chain_model(tmp_path, 30, device)
    q, qd, _ = sample_states(model, 65, seed=0)
    t = build_truth(model._spec, q, qd)
    check_all("chain30", path, *run_model(model, "chain30", inputs=(q, qd)), t=t, inputs=(q, qd))
    return model


def test_long_chain(cpu_library, tmp_path):
    long_chain_check(tmp_path, "cpu", "host")


# ------------------------------------------------------------------------------------------------------------------- GPU
def gpu_run_and_check(robot, B, composed=False, compat=True, path=None):
    model = model_on(robot, "cuda:0", compat)
    out = run_model(model, robot, B=B, composed=composed)
    torch.cuda.synchronize()
    name = path or ("general" if composed or robot not in ARMS or B < 64 else "fused") + "-B%d" % B
    check_all(robot, name, *out, t=truth(robot, compat))
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 128, 131])
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_against_truth(robot, B):
    model = gpu_run_and_check(robot, B)
    coriolis_alone_check(model, robot, B=B)


@pytest.mark.gpu
def test_gpu_arm_general_kernel():
    model = gpu_run_and_check("panda_no_gripper", 128, composed=True)
    coriolis_alone_check(model, "panda_no_gripper", composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", OTHERS)
def test_gpu_other_robots_against_truth(robot):
    model = gpu_run_and_check(robot, 65)
    coriolis_alone_check(model, robot, B=65)


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
    assert backend.load_library().drm_lagrangian_dynamics_scratch_floats(ctypes.byref(walk_of(model)), 65) > 0


def persistent_grid_check(tmp_path, query, compute):
    """test_max_sizes.chain_model's 11-joint chain is the shortest whose 64 rows of records leave a 32 KB LDS limit for the scratch,
    and 64 * 2048 + 65 rows are more tiles than the persistent grid has blocks: blocks 0 and 1 walk a second tile through the slice of
    the scratch they used for their first, and the last tile is ragged.  The scratch does not grow past 2048 tiles.  Rows share
    nothing, so the rows of the one big call equal the same rows computed 65 at a time to the bit: the first 65, the 65 from row
    64 * 2048 on, and the last 65 (which here are the same rows).  Truth at 65 rows: the long-chain tests."""
    from differentiable_robot_model_amd import backend
    from helpers import sample_states
    from test_max_sizes import chain_model
    model = chain_model(tmp_path, 11, "cuda")
    full, B = 64 * 2048, 64 * 2048 + 65
    fn, walk = getattr(backend.load_library(), query), walk_of(model)
    need = int(fn(ctypes.byref(walk), B))
    assert need > 0 and need == int(fn(ctypes.byref(walk), full))
    q, qd, _ = (torch.from_numpy(x).cuda() for x in sample_states(model, B, seed=0))
    big = compute(model, q, qd)
    for lo in (0, full, B - 65):
        part = compute(model, q[lo:lo + 65].clone(), qd[lo:lo + 65].clone())
        for name, whole, rows in zip(big._fields, big, part):
            assert rows.shape[0] == 65 and torch.equal(whole[lo:lo + 65], rows), (name, lo)


@pytest.mark.gpu
def test_gpu_persistent_grid_beyond_2048_tiles(tmp_path):
    persistent_grid_check(tmp_path, "drm_lagrangian_dynamics_scratch_floats_aligned", lambda m, q, qd: m.compute_lagrangian_dynamics(q, qd))


@pytest.mark.gpu
def test_gpu_interface():
    interface_check("cuda:0")


@pytest.mark.gpu
def test_gpu_c_abi_null_outputs():
    from differentiable_robot_model_amd import backend
    model = model_on("panda_no_gripper", "cuda:0")
    lib = backend.load_library()
    assert lib.drm_abi_version() == 15
    c_abi_null_check(lib, model, "cuda", backend._stream(torch.device("cuda:0")), B=5)
    c_abi_null_check(lib, model, "cuda", backend._stream(torch.device("cuda:0")), B=128)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["panda_no_gripper", "iiwa7_allegro"])
def test_gpu_c_abi_misaligned_and_guards(robot):
    """Straight through the C ABI: q, qd, H, C and g 4 bytes off a 16-byte boundary (the general kernel), a scratch of exactly
    drm_lagrangian_dynamics_scratch_floats floats, guard words behind the scratch and on both sides of every output."""
    from differentiable_robot_model_amd import backend
    model = model_on(robot, "cuda:0")
    lib, walk, n = backend.load_library(), walk_of(model), model._n_dofs

    def off_by_4(x):
        buf = torch.zeros(x.numel() + 1, device="cuda")
        buf[1:] = x.reshape(-1)
        view = buf[1:].view(x.shape)
        assert view.data_ptr() % 16 == 4
        return view
    q, qd = (off_by_4(torch.from_numpy(x).cuda()) for x in states(robot))
    need = int(lib.drm_lagrangian_dynamics_scratch_floats(ctypes.byref(walk), ROWS))
    assert (need > 0) == (robot == "iiwa7_allegro")
    GUARD = 64
    scratch = torch.full((need + GUARD,), 3.25, device="cuda")
    sizes = (ROWS * n * n, ROWS * n * n, ROWS * n)
    bufs = [torch.full((1 + s + GUARD,), -1.5, device="cuda") for s in sizes]
    outs = [b[1:1 + s] for b, s in zip(bufs, sizes)]
    assert all(o.data_ptr() % 16 == 4 for o in outs)
    rc = lib.drm_lagrangian_dynamics(ctypes.byref(walk), q.data_ptr(), qd.data_ptr(), ROWS, 0, outs[0].data_ptr(), outs[1].data_ptr(),
                                     outs[2].data_ptr(), scratch.data_ptr(), backend._stream(q.device))
    torch.cuda.synchronize()
    assert rc == 0
    assert (scratch[need:] == 3.25).all()
    for b, s in zip(bufs, sizes):
        assert (b[1 + s:] == -1.5).all() and b[0] == -1.5
    check_all(robot, "misaligned", outs[0].view(ROWS, n, n), outs[1].view(ROWS, n, n), outs[2].view(ROWS, n))


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_non_finite_rows(composed):
    bad_rows_check(model_on("panda_no_gripper", "cuda:0"), "cuda", composed=composed)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_learnable_link():
    learnable_check("cuda:0", "learnable")

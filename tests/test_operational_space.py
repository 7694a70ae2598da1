"""Operational-space dynamics of one link in one call (csrc/drm_osc.hip, include/drm_hip.h drm_operational_space;
DifferentiableRobotModel.compute_operational_space_dynamics): inertia = (J H^-1 J^T + rho^2 I)^-1, jacobian_pinv = H^-1 J^T inertia,
bias_acc = Jdot qd, bias_force = inertia (J H^-1 nle - Jdot qd).

TRUTH, computed here: inertia, jacobian_pinv and bias_force in NumPy fp64 from Oracle.fk_jacobian, Oracle.mass_matrix and
Oracle.rnea(qdd = 0) called with dtype=np.float64; Jdot qd the fp64 central difference (J(q + h qd) - J(q - h qd)) / 2h . qd, h = 1e-5
(truncation and rounding both about 1e-10).

bias_acc: Jdot qd is a sum of at most n^2 products of quantities held to TOL_JAC, so atol = n^2 TOL_JAC["atol"] vel^2, rtol = 2e-5.

inertia, jacobian_pinv, bias_force: the error depends on the conditioning, so the YARDSTICK is the error of the same formulas in
float32 NumPy (np.linalg, LAPACK) from the oracle's float32 outputs (the fp64 Jdot qd rounded to float32 stands in for the one
quantity float32 differences cannot produce) — no code under test.  With err(X) = max over rows of max|X - X64| / max|X64| the
requirement is err(path) <= 8 max(err(yardstick), 2^-23) for each array and each path; 8 covers unpivoted elimination and a
different summation order.  Every comparison prints one "OSC" line (check, robot, link, m, rho, flags, path, array, error, yardstick
or bound) before it asserts; profiles/osc_tests.txt holds them for the host build and the MI355X.

Inputs: sample_states(model, 512, seed=0, vel=1.0).  rho = 0.1 bounds |inertia| by 100.  With rho = 0 only rows whose truth has
cond_2(A) <= 1e4 are kept, and at least half must remain.  Measured on the host build with exactly this sampling, rows kept at
m = 6: Panda 0.900, iiwa 0.674, Fetch (gripper_link) 0.953; at m = 3: 1.000 for the three arms, 0.998 for the Allegro fingertip.
rho = 0 is NOT a case where J cannot have full row rank (m = 6 on the 4-joint chains of a finger and of panda_link4, whose origin
lies on its own joint's axis and leaves three joints for three rows with a rank of two; the planar 2-link robot at either m): A is
then singular on every row and no truth exists.

GPU (-m gpu): a launch of B rows is repeated over consecutive slices of the 512 rows, so the statistic is taken over the same rows
as on the CPU whatever B is.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from differentiable_robot_model_amd import backend
from helpers import TOL_JAC, load_model, sample_states
from oracle import Oracle

ROWS, VEL, FD_H, FLOOR, MARGIN = 512, 1.0, 1e-5, 2.0 ** -23, 8.0
PANDA = ("panda_no_gripper", "panda_virtual_ee_link")
IIWA = ("iiwa7", "iiwa_link_ee")
FETCH = ("fetch", "gripper_link")                    # the whole tree (wheels, head, gripper) with the arm in its middle
ALLEGRO = ("allegro_left", "link_3.0_tip")
TWO_LINK = ("2link_robot", "endEffector")
ARM_HAND = ("iiwa7_allegro", "link_3.0_tip")         # 23 DoFs: on the GPU the finish kernel's rows no longer fit in LDS
ALL_FLAGS = [(g, d) for g in (True, False) for d in (True, False)]
# (robot, link, m, rho): see the module docstring for the cases rho = 0 leaves out
CASES = ([(r, m, rho) for r in (PANDA, IIWA, FETCH) for m in (6, 3) for rho in (0.1, 0.0)] +
         [(ALLEGRO, 6, 0.1), (ALLEGRO, 3, 0.1), (ALLEGRO, 3, 0.0), (TWO_LINK, 3, 0.1), (ARM_HAND, 6, 0.1)])


def case_id(c):
    return "%s-m%d-rho%g" % (c[0][0], c[1], c[2])


@functools.lru_cache(maxsize=None)
def model_on(robot, device="cpu"):
    return load_model(robot, device)


@functools.lru_cache(maxsize=None)
def states(robot):
    q, qd, _ = sample_states(model_on(robot), ROWS, seed=0, vel=VEL)
    return q, qd


@functools.lru_cache(maxsize=None)
def kinematics(robot, link):
    """(J64 [B, 6, n], H64, Jdot qd [B, 6] fp64, J32, H32): what does not depend on m, rho or the flags."""
    model = model_on(robot)
    orc, idx = Oracle(model._spec), model._name_to_idx_map[link]
    q, qd = states(robot)
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)

    def jac(x, dt):
        _, _, lin, ang = orc.fk_jacobian(x.astype(dt), idx, dt)
        return np.concatenate([lin, ang], 1)
    acc = np.einsum("bmn,bn->bm", (jac(q64 + FD_H * qd64, np.float64) - jac(q64 - FD_H * qd64, np.float64)) / (2 * FD_H), qd64)
    return (jac(q64, np.float64), orc.mass_matrix(q64, True, True, np.float64), acc,
            jac(q, np.float32), orc.mass_matrix(q, True, True, np.float32))


@functools.lru_cache(maxsize=None)
def bias_torques(robot, gravity, damping, dt):
    q, qd = states(robot)
    return Oracle(model_on(robot)._spec).rnea(q.astype(dt), qd.astype(dt), np.zeros_like(q, dtype=dt), gravity, damping, dt)


def compose(J, H, nle, acc, rho, dt):
    """The formulas of the module docstring in NumPy at dtype dt -> (inertia, jacobian_pinv, bias_force, A)."""
    J, H, nle, acc = J.astype(dt), H.astype(dt), nle.astype(dt), acc.astype(dt)
    X = np.linalg.solve(H, J.transpose(0, 2, 1))                  # H^-1 J^T, [B, n, m]
    A = J @ X + dt(rho) ** 2 * np.eye(J.shape[1], dtype=dt)
    lam = np.linalg.inv(A)
    eta = np.einsum("bij,bj->bi", lam, np.einsum("bnm,bn->bm", X, nle) - acc)
    assert lam.dtype == dt and eta.dtype == dt
    return lam, X @ lam, eta, A


@functools.lru_cache(maxsize=None)
def problem(robot, link, m, rho, gravity=True, damping=False):
    """dict: truth (fp64), yardstick (float32 NumPy), the rows kept, for one case."""
    J64, H64, acc, J32, H32 = kinematics(robot, link)
    lam, jbar, eta, A = compose(J64[:, :m], H64, bias_torques(robot, gravity, damping, np.float64), acc[:, :m], rho, np.float64)
    ylam, yjbar, yeta, _ = compose(J32[:, :m], H32, bias_torques(robot, gravity, damping, np.float32), acc[:, :m], rho, np.float32)
    keep = np.ones(ROWS, bool)
    if rho == 0.0:
        keep = np.linalg.cond(A) <= 1e4
        assert keep.mean() >= 0.5, "the conditioning bound thinned the test to %.3f of its rows" % keep.mean()
    return dict(truth=(lam, jbar, eta), yard=(ylam, yjbar, yeta), acc=acc[:, :m], keep=keep, J64=J64[:, :m], J32=J32[:, :m], H32=H32)


def err(X, X64, keep):
    X, X64 = np.asarray(X, np.float64).reshape(len(X64), -1), X64.reshape(len(X64), -1)
    return float((np.abs(X - X64).max(1) / np.abs(X64).max(1))[keep].max())


def report(check, case, flags, path, array, value, other):
    (robot, link), m, rho = case
    print("OSC %-9s %-17s %-22s m=%d rho=%-3g g%d d%d %-9s %-13s %.3e  %.3e" % (check, robot, link, m, rho, flags[0], flags[1], path, array,
                                                                            value, other))


def check_against_truth(case, flags, path, out, rows=slice(None)):
    """The 8 x rule for inertia, jacobian_pinv, bias_force and the derived bound for bias_acc, over the kept rows of `rows`."""
    (robot, link), m, rho = case
    p = problem(robot, link, m, rho, *flags)
    keep = p["keep"][rows]
    n = states(robot)[0].shape[1]
    got = [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in out]
    assert got[0].shape == (keep.size, m, m) and got[1].shape == (keep.size, n, m) and got[2].shape == got[3].shape == (keep.size, m)
    bad = []
    for name, g, t, y in zip(("inertia", "jacobian_pinv", "bias_force"), (got[0], got[1], got[3]), p["truth"], p["yard"]):
        e, ey = err(g, t[rows], keep), err(y[rows], t[rows], keep)
        report("truth", case, flags, path, name, e, ey)
        if not e <= MARGIN * max(ey, FLOOR):
            bad.append((name, e, ey))
    acc = p["acc"][rows]
    atol, rtol = n * n * TOL_JAC["atol"] * VEL ** 2, 2e-5
    excess = float((np.abs(got[2] - acc) - rtol * np.abs(acc))[keep].max())
    report("truth", case, flags, path, "bias_acc", excess, atol)
    if not excess <= atol:
        bad.append(("bias_acc", excess, atol))
    assert not bad, bad
    return got


def run_model(model, case, flags, B=None, composed=False):
    """compute_operational_space_dynamics over the 512 rows in consecutive launches of B rows (None: one launch)."""
    (robot, link), m, rho = case
    q, qd = (torch.from_numpy(x).to(model._device) for x in states(robot))
    B = B or ROWS
    outs = [model.compute_operational_space_dynamics(q[i:i + B], qd[i:i + B], link, include_gravity=flags[0], use_damping=flags[1],
                                                     position_only=m == 3, regularization=rho, _composed=composed)
            for i in range(0, ROWS, B)]
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("flags", ALL_FLAGS, ids=lambda f: "g%d-d%d" % f)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_build_against_truth(cpu_library, case, flags):
    out = run_model(model_on(case[0][0]), case, flags)
    check_against_truth(case, flags, "host", out)


def yardstick_identity(p, nle32, a, m):
    """The control identity through the float32 yardstick: J qdd + Jdot qd with qdd = H^-1 (J^T (inertia a + bias_force) - nle)."""
    J, H = p["J32"], p["H32"]
    lam, _, eta = p["yard"]
    tau = np.einsum("bmn,bm->bn", J, np.einsum("bij,bj->bi", lam, a) + eta)
    qdd = np.linalg.solve(H, (tau - nle32)[..., None])[..., 0]
    out = np.einsum("bmn,bn->bm", J, qdd) + p["acc"].astype(np.float32)
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("flags", [(True, False), (False, True)], ids=lambda f: "g%d-d%d" % f)
@pytest.mark.parametrize("case", [(PANDA, 6, 0.0), (IIWA, 6, 0.0), (FETCH, 3, 0.0)], ids=case_id)
def test_control_identity(cpu_library, case, flags):
    """tau = J^T (inertia a + bias_force) through compute_forward_dynamics gives the link the acceleration a (rho = 0, kept rows)."""
    (robot, link), m, rho = case
    model, p = model_on(robot), problem(robot, link, m, rho, *flags)
    q, qd = (torch.from_numpy(x) for x in states(robot))
    a = np.random.default_rng(1).uniform(-1, 1, (ROWS, m)).astype(np.float32)
    o = model.compute_operational_space_dynamics(q, qd, link, include_gravity=flags[0], use_damping=flags[1], position_only=m == 3)
    lin, ang = model.compute_endeffector_jacobian(q, link)
    J = torch.cat([lin, ang], 1)[:, :m]
    tau = (J.transpose(1, 2) @ (o.inertia @ torch.from_numpy(a)[..., None] + o.bias_force[..., None]))[..., 0]
    qdd = model.compute_forward_dynamics(q, qd, tau, include_gravity=flags[0], use_damping=flags[1])
    got = ((J @ qdd[..., None])[..., 0] + o.bias_acc).numpy()
    a64 = a.astype(np.float64)
    e = err(got, a64, p["keep"])
    ey = err(yardstick_identity(p, bias_torques(robot, flags[0], flags[1], np.float32), a, m), a64, p["keep"])
    report("identity", case, flags, "host", "J qdd + bias", e, ey)
    assert e <= MARGIN * max(ey, FLOOR), (e, ey)


@pytest.mark.parametrize("case", [(PANDA, 6, 0.1), (PANDA, 6, 0.0), (IIWA, 3, 0.1), (FETCH, 6, 0.1), (ALLEGRO, 6, 0.1)], ids=case_id)
def test_symmetry_and_pinv(cpu_library, case):
    """inertia is symmetric to 4 ulp of its largest entry; J jacobian_pinv = I - rho^2 inertia by the 8 x rule."""
    (robot, link), m, rho = case
    flags = (True, False)
    p = problem(robot, link, m, rho, *flags)
    lam, jbar, _, _ = (t.numpy() for t in run_model(model_on(robot), case, flags))
    asym = np.abs(lam - lam.transpose(0, 2, 1)).reshape(ROWS, -1).max(1)
    ulp = np.spacing(np.abs(lam).reshape(ROWS, -1).max(1).astype(np.float32))
    report("symmetry", case, flags, "host", "inertia", float((asym / ulp).max()), 4.0)
    assert (asym <= 4 * ulp).all()
    want = np.eye(m) - rho ** 2 * p["truth"][0]
    e = err(p["J64"] @ jbar.astype(np.float64), want, p["keep"])
    ey = err(p["J32"] @ p["yard"][1], want, p["keep"])
    report("pinv", case, flags, "host", "J jbar", e, ey)
    assert e <= MARGIN * max(ey, FLOOR), (e, ey)


def test_bias_acc_with_sliding_joints(cpu_library):
    """Fetch with its torso lift modelled as the prismatic joint it is (reference_compat=False): Jdot qd of a chain that slides and
    turns, against the fp64 central difference of that model's Jacobian, by the bound of the module docstring."""
    robot, link = FETCH
    model = load_model(robot, reference_compat=False)
    orc, idx = Oracle(model._spec), model._name_to_idx_map[link]
    q, qd, _ = sample_states(model, 256, seed=0, vel=VEL)
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)

    def jac(x):
        _, _, lin, ang = orc.fk_jacobian(x, idx, np.float64)
        return np.concatenate([lin, ang], 1)
    acc = np.einsum("bmn,bn->bm", (jac(q64 + FD_H * qd64) - jac(q64 - FD_H * qd64)) / (2 * FD_H), qd64)
    got = model.compute_operational_space_dynamics(torch.from_numpy(q), torch.from_numpy(qd), link, regularization=0.1).bias_acc.numpy()
    n = q.shape[1]
    atol, rtol = n * n * TOL_JAC["atol"] * VEL ** 2, 2e-5
    excess = float((np.abs(got - acc) - rtol * np.abs(acc)).max())
    report("sliding", ((robot, link), 6, 0.1), (True, False), "host", "bias_acc", excess, atol)
    assert excess <= atol


def walks_of(model, link):
    """(tree, chain) drm_walk structs as compute_operational_space_dynamics passes them, and their owners."""
    idx = model._name_to_idx_map[link]
    tree = model._dynamics_walk()
    chain = model._get_walk(("chain", idx) + (("folded", tree.fold_key) if tree.folded else ()), targets=[idx], folded=tree.folded,
                            fold_key=tree.fold_key)
    n = model._n_dofs
    return (backend._walk_struct(tree.program, model._ops_f(tree).detach(), tree.ops_i, n),
            backend._walk_struct(chain.program, model._ops_f(chain).detach(), chain.ops_i, n), (tree, chain))


def c_call(lib, wt, wc, q, qd, B, flags, reg, outs, scratch=None):
    ptr = lambda t: t.data_ptr() if t is not None else None
    return lib.drm_operational_space(ctypes.byref(wt), ctypes.byref(wc), ptr(q), ptr(qd), B, flags, reg, *(ptr(t) for t in outs),
                                     ptr(scratch), None)


def test_abi_entry_points_and_null_outputs(cpu_library):
    lib = backend.load_library(kind="cpu")
    assert lib.drm_abi_version() == 15
    robot, link = PANDA
    model = model_on(robot)
    wt, wc, _owners = walks_of(model, link)
    assert lib.drm_operational_space_scratch_floats(ctypes.byref(wt), ctypes.byref(wc), 100) == 0
    assert lib.drm_operational_space_scratch_floats_aligned(ctypes.byref(wt), ctypes.byref(wc), 100) == 0
    q, qd = (torch.from_numpy(x[:8].copy()) for x in states(robot))
    full = [torch.empty(8, 6, 6), torch.empty(8, 7, 6), torch.empty(8, 6), torch.empty(8, 6)]
    assert c_call(lib, wt, wc, q, qd, 8, backend.RNEA_GRAVITY, 0.1, full) == 0
    want = model.compute_operational_space_dynamics(q, qd, link, regularization=0.1)
    assert all(torch.equal(a, b) for a, b in zip(full, want))
    assert c_call(lib, wt, wc, q, qd, 8, backend.RNEA_GRAVITY, -0.5, full) == -1                      # reg < 0
    assert c_call(lib, wt, wc, q, qd, 8, backend.RNEA_GRAVITY, float("nan"), full) == -1
    assert c_call(lib, wt, wc, q, qd, 8, backend.RNEA_GRAVITY, float("inf"), full) == -1
    assert c_call(lib, wt, wc, q, qd, 0, backend.RNEA_GRAVITY, 0.1, full) == 0                       # B == 0
    assert c_call(lib, wt, wc, q, qd, 8, backend.RNEA_GRAVITY, 0.1, [None] * 4) == -1                # every output NULL
    assert c_call(lib, wt, wc, None, qd, 8, backend.RNEA_GRAVITY, 0.1, full) == -1                   # a required pointer
    assert c_call(lib, wt, wc, q, None, 8, backend.RNEA_GRAVITY, 0.1, full) == -1                    # (bias_acc needs qd)
    # any output may be NULL: the others are written with the same values; qd is not needed for inertia / jacobian_pinv alone
    for k in range(4):
        outs = [torch.full_like(t, 7.0) if i == k else None for i, t in enumerate(full)]
        assert c_call(lib, wt, wc, q, qd if k >= 2 else None, 8, backend.RNEA_GRAVITY, 0.1, outs) == 0
        assert torch.equal(outs[k], full[k]), k
    pos = [torch.empty(8, 3, 3), torch.empty(8, 7, 3), torch.empty(8, 3), torch.empty(8, 3)]
    assert c_call(lib, wt, wc, q, qd, 8, backend.RNEA_GRAVITY | backend.OSC_POSITION_ONLY, 0.1, pos) == 0
    want = model.compute_operational_space_dynamics(q, qd, link, regularization=0.1, position_only=True)
    assert all(torch.equal(a, b) for a, b in zip(pos, want))


def test_unbatched_and_types(cpu_library):
    robot, link = PANDA
    model = model_on(robot)
    q, qd = (torch.from_numpy(x[:3].copy()) for x in states(robot))
    many = model.compute_operational_space_dynamics(q, qd, link, regularization=0.1)
    assert type(many).__name__ == "OperationalSpaceDynamics" and many._fields == ("inertia", "jacobian_pinv", "bias_acc", "bias_force")
    one = model.compute_operational_space_dynamics(q[1], qd[1], link, regularization=0.1)
    assert one.inertia.shape == (6, 6) and one.jacobian_pinv.shape == (7, 6) and one.bias_acc.shape == (6,) and one.bias_force.shape == (6,)
    assert all(torch.equal(a, b[1]) for a, b in zip(one, many))
    one3 = model.compute_operational_space_dynamics(q[1], qd[1], link, position_only=True)
    assert one3.inertia.shape == (3, 3) and one3.jacobian_pinv.shape == (7, 3) and one3.bias_acc.shape == (3,)
    f64 = model.compute_operational_space_dynamics(q.double(), qd.double(), link, regularization=0.1)     # (computed in fp32)
    assert all(t.dtype == torch.float32 for t in f64) and all(torch.equal(a, b) for a, b in zip(f64, many))
    empty = model.compute_operational_space_dynamics(q[:0], qd[:0], link)
    assert empty.inertia.shape == (0, 6, 6) and empty.jacobian_pinv.shape == (0, 7, 6)


def test_validation(cpu_library):
    robot, link = PANDA
    model = model_on(robot)
    q, qd = (torch.from_numpy(x[:3].copy()) for x in states(robot))
    f = model.compute_operational_space_dynamics
    with pytest.raises(TypeError):
        f(q.numpy(), qd, link)
    with pytest.raises(TypeError):
        f(q, None, link)
    with pytest.raises(TypeError):
        f(q.long(), qd, link)
    with pytest.raises(ValueError):
        f(q.to("meta"), qd, link)
    with pytest.raises(ValueError):
        f(q[:, :6], qd[:, :6], link)
    with pytest.raises(ValueError):
        f(q[None], qd[None], link)
    with pytest.raises(ValueError):
        f(q, qd[:2], link)
    with pytest.raises(ValueError, match="unknown link"):
        f(q, qd, "no_such_link")
    with pytest.raises(ValueError, match="root link"):
        f(q, qd, model.get_link_names()[0])
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="regularization"):
            f(q, qd, link, regularization=bad)
    with pytest.raises(TypeError):
        f(q, qd, link, True)                                      # the options are keyword-only


def test_learnable_link_uses_current_values(cpu_library):
    """No autograd history, and a changed parameter changes the result: held, by the 8 x rule, to the composition of the SAME model's
    Jacobian, inertia matrix and bias torques (fp64 NumPy from its float32 outputs; yardstick: float32 NumPy from the same)."""
    from differentiable_robot_model_amd.rigid_body_params import UnconstrainedTensor
    robot, link = PANDA
    model = load_model(robot)
    model.make_link_param_learnable("panda_link3", "trans", UnconstrainedTensor(dim1=1, dim2=3))
    model.make_link_param_learnable("panda_link5", "mass", UnconstrainedTensor(dim1=1, dim2=1))
    q, qd = (torch.from_numpy(x[:64].copy()).requires_grad_(True) for x in states(robot))
    before = model.compute_operational_space_dynamics(q, qd, link, regularization=0.1)
    assert all(t.grad_fn is None and not t.requires_grad for t in before)
    with torch.no_grad():
        for prm in model.parameters():
            prm.add_(0.05)
    after = model.compute_operational_space_dynamics(q, qd, link, regularization=0.1)
    assert all(t.grad_fn is None and not t.requires_grad for t in after)
    assert float((after.inertia - before.inertia).abs().max()) > 1e-3
    with torch.no_grad():
        lin, ang = model.compute_endeffector_jacobian(q, link)
        J = torch.cat([lin, ang], 1).numpy()
        H = model.compute_lagrangian_inertia_matrix(q).numpy()
        nle = model.compute_non_linear_effects(q, qd, include_gravity=True, use_damping=False).numpy()
    acc = after.bias_acc.numpy()
    keep = np.ones(64, bool)
    case = ((robot, link), 6, 0.1)
    for name, g, t, y in zip(("inertia", "jacobian_pinv", "bias_force"), (after.inertia, after.jacobian_pinv, after.bias_force),
                             compose(J, H, nle, acc, 0.1, np.float64), compose(J, H, nle, acc, 0.1, np.float32)):
        e, ey = err(g.numpy(), t, keep), err(y, t, keep)
        report("learnable", case, (True, False), "host", name, e, ey)
        assert e <= MARGIN * max(ey, FLOOR), (name, e, ey)


# ------------------------------------------------------------------------------------------------------------------- GPU
GPU_FLAGS = (True, True)


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "composed"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("arm", [PANDA, IIWA], ids=lambda a: a[0])
def test_gpu_arm_against_truth(arm, B, composed):
    """Tiles start at 64 rows: 65 and 257 are fused rows plus a ragged tail in one call, 1 and 63 are all tail."""
    model = model_on(arm[0], "cuda:0")
    for m, rho in ((6, 0.1), (3, 0.1)) + (((6, 0.0),) if B in (64, 257) else ()):
        case = (arm, m, rho)
        out = run_model(model, case, GPU_FLAGS, B=B, composed=composed)
        torch.cuda.synchronize()
        check_against_truth(case, GPU_FLAGS, ("composed" if composed else "fused") + "-B%d" % B, out)


@pytest.mark.gpu
def test_gpu_fused_and_composed_agree_on_the_tail():
    """Rows behind the last full tile take the composed path either way: the same bits."""
    model = model_on(PANDA[0], "cuda:0")
    q, qd = (torch.from_numpy(x[:65]).cuda() for x in states(PANDA[0]))
    a = model.compute_operational_space_dynamics(q, qd, PANDA[1], regularization=0.1)
    b = model.compute_operational_space_dynamics(q, qd, PANDA[1], regularization=0.1, _composed=True)
    assert all(torch.equal(x[64:], y[64:]) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(FETCH, 6, 0.1), (FETCH, 3, 0.0), (ALLEGRO, 6, 0.1), (ALLEGRO, 3, 0.0), ((PANDA[0], "panda_link4"), 3, 0.1),
                                  (ARM_HAND, 6, 0.1)], ids=case_id)
def test_gpu_composed_robots_against_truth(case):
    """Fetch, an Allegro fingertip, a mid-chain Panda target (position only) and a fingertip of an arm that carries a hand (23 DoFs:
    the finish kernel factorises in the scratch, not in LDS): the composed path, launches of 65 rows."""
    out = run_model(model_on(case[0][0], "cuda:0"), case, GPU_FLAGS, B=65)
    torch.cuda.synchronize()
    check_against_truth(case, GPU_FLAGS, "composed-B65", out)


@pytest.mark.gpu
def test_gpu_misaligned_q():
    """q and qd as [1:] views of [B + 1, n] buffers (28 bytes off a 16-byte boundary), straight through the C ABI: the composed path,
    the same values as the aligned call, held to the truth."""
    robot, link = PANDA
    B, case = 130, (PANDA, 6, 0.1)
    model = model_on(robot, "cuda:0")
    lib = backend.load_library()
    wt, wc, _owners = walks_of(model, link)
    q, qd = (torch.from_numpy(x[:B]).cuda() for x in states(robot))
    bufs = [torch.zeros(B + 1, 7, device="cuda") for _ in range(2)]
    bufs[0][1:] = q
    bufs[1][1:] = qd
    vq, vqd = bufs[0][1:], bufs[1][1:]
    assert vq.data_ptr() % 16 != 0 and vqd.data_ptr() % 16 != 0 and vq.is_contiguous()
    need = int(lib.drm_operational_space_scratch_floats(ctypes.byref(wt), ctypes.byref(wc), B))
    assert need > 0
    scratch = torch.empty(need, device="cuda")
    outs = [torch.empty(B, 6, 6, device="cuda"), torch.empty(B, 7, 6, device="cuda"), torch.empty(B, 6, device="cuda"),
            torch.empty(B, 6, device="cuda")]
    flags = backend.RNEA_GRAVITY | backend.RNEA_DAMPING
    assert lib.drm_operational_space(ctypes.byref(wt), ctypes.byref(wc), vq.data_ptr(), vqd.data_ptr(), B, flags, 0.1,
                                     *(t.data_ptr() for t in outs), scratch.data_ptr(), backend._stream(vq.device)) == 0
    torch.cuda.synchronize()
    want = model.compute_operational_space_dynamics(q, qd, link, include_gravity=True, use_damping=True, regularization=0.1, _composed=True)
    assert all(torch.equal(a, b) for a, b in zip(outs, want))
    check_against_truth(case, GPU_FLAGS, "misaligned", outs, rows=slice(0, B))


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "composed"])
def test_gpu_non_finite_row(composed):
    """One non-finite row among 128: its outputs are non-finite, every other row has the bits of a run with that row finite."""
    robot, link = PANDA
    model = model_on(robot, "cuda:0")
    q, qd = (torch.from_numpy(x[:128].copy()).cuda() for x in states(robot))
    kw = dict(regularization=0.1, _composed=composed)
    clean = model.compute_operational_space_dynamics(q, qd, link, **kw)
    for where, value in ((q, float("nan")), (qd, float("inf"))):
        spoiled = [q.clone(), qd.clone()]
        spoiled[0 if where is q else 1][37, 2] = value
        got = model.compute_operational_space_dynamics(*spoiled, link, **kw)
        torch.cuda.synchronize()
        others = torch.arange(128, device="cuda") != 37
        for a, b in zip(got, clean):
            assert not torch.isfinite(a[37]).any()
            assert torch.equal(a[others], b[others])


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "composed"])
def test_gpu_singular_row(composed):
    """Panda at q = 0 is singular for m = 6: with rho = 0 the call returns, the device synchronises, and the other rows keep the bits
    of a run without that row (what the singular row itself holds is huge or non-finite, and not looked at)."""
    robot, link = PANDA
    model = model_on(robot, "cuda:0")
    q, qd = (torch.from_numpy(x[:128].copy()).cuda() for x in states(robot))
    clean = model.compute_operational_space_dynamics(q, qd, link, _composed=composed)
    q[70] = 0.0
    got = model.compute_operational_space_dynamics(q, qd, link, _composed=composed)
    torch.cuda.synchronize()
    others = torch.arange(128, device="cuda") != 70
    assert all(torch.equal(a[others], b[others]) for a, b in zip(got, clean))
    assert bool(torch.isfinite(got.bias_acc[70]).all())               # (Jdot qd does not go through the inverse)


@pytest.mark.gpu
def test_gpu_graph_capture_bit_equal():
    robot, link = PANDA
    model = model_on(robot, "cuda:0")
    q, qd = (torch.from_numpy(x[:256]).cuda() for x in states(robot))
    eager = model.compute_operational_space_dynamics(q, qd, link, regularization=0.1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.compute_operational_space_dynamics(q, qd, link, regularization=0.1)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = model.compute_operational_space_dynamics(q, qd, link, regularization=0.1)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))

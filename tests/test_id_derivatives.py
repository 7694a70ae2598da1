"""Inverse-dynamics derivatives in one call (csrc/drm_idd.hip, include/drm_hip.h drm_rnea_derivatives;
DifferentiableRobotModel.compute_inverse_dynamics_derivatives): tau = ID(q, qd, qdd), dtau_dq, dtau_dqd and dtau_dqdd = H(q),
[b, i, j] = d tau_i / d x_j.

INPUTS: per robot the 128 rows of q and qd of tests/golden/golden_fd_derivatives.npz and qdd ~ U(-2, 2) of
tests/golden/golden_id_derivatives.npz (make_golden_id_derivatives.py).

TRUTH, from the fp64 oracle only: dtau_dq and dtau_dqd are central differences of Oracle.rnea(..., np.float64) at h = 1e-4 and 3e-4,
Richardson-combined as (9 D_h - D_3h) / 8; H64 = Oracle.mass_matrix, tau64 = Oracle.rnea.  Before anything under test is compared
the truth at h = 1e-4 must agree with the same at h = 2e-4 to 1e-8 relative.

The one-sweep recursion (Carpentier and Mansard 2018; Singh, Russell and Wensing 2022) is restated HERE in numpy in link-local
frames (id_derivatives_local); run in fp64 it must match the truth to 1e-8 relative.

METRIC: err(X) = max over rows of max|X - X64| / max|X64| over the row's matrix.  YARDSTICKS, none of them code under test:
    dtau_dq    the unmodified reference's float32 autograd Jacobian from the fixture at the setting with the same gravity flag
    dtau_dqd   ... at the setting with the same damping flag
               (each over the rows of the launch the fixture holds: 128 for n <= 7, 32 for Fetch and Allegro, 16 for iiwa7_allegro)
    H          the oracle's own float32 mass_matrix
Models the reference does not describe (sliding joints and skew axes under reference_compat=False, the 30-joint chain, a moved
learnable link) have no reference Jacobian: there the yardstick of dtau_dq and dtau_dqd is the numpy restatement run in float32,
the reasoning of tests/test_lagrangian.py: the same formula in the same precision in another summation order.
REQUIREMENT on every path, all four flag combinations: err(path) <= 8 max(err(yardstick), 2^-23); 8 is the project's margin for a
different summation order.  tau must match compute_inverse_dynamics of the same launches to atol = rtol = 2e-5.
Every comparison prints one "IDD" line (robot, flags, path, array, error, yardstick, ratio) before it asserts;
profiles/id_derivatives_tests.txt holds them for the host build and the MI355X.

STRUCTURE: dtau_dqdd is symmetric to the bit; the entries of all three matrices between joints on different branches (the set read
off the kinematic tree) are exactly 0.0, vanish in the truth in every row, and the set is not empty for Fetch, Allegro and iiwa7_allegro.

GPU (-m gpu): a launch of B rows is repeated over consecutive slices of the 128 rows, so the statistic is over the same rows whatever
B is.  64-row tiles: B = 64 and 128 are the fused arm kernel, 65 and 131 a fused part plus a ragged tail in the general kernel, 1 the
general kernel alone.  test_max_sizes.chain_model's 30-joint chain at 65 rows is the size at which the general kernel's per-row records
leave LDS for the scratch.

Measured (profiles/id_derivatives_tests.txt), worst err / yardstick: 6.80 on the host build and 6.90 on the MI355X, both for dtau_dqd of
iiwa7_allegro without damping: the statistic runs over all 128 rows, the reference's Jacobians over the 16 the fixture holds, and the
worst row (31; this recursion 2.3e-6, the same recursion in float32 numpy 1.7e-6, the reference itself 4.9e-7 when run there by hand)
is not among them; over the 16 held rows the ratio is 0.97.  Next: 2.64 (dtau_dq, iiwa7_allegro, MI355X), 2.33 (dtau_dqd with damping);
the arms' fused kernel stays below 2.4, dtau_dqdd below 0.1 everywhere.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, load_model
from oracle import Oracle
from test_lagrangian import _bar, _crf, _crm, _rpy, _skew, different_branches, walk_of

ROWS, FLOOR, MARGIN = 128, 2.0 ** -23, 8.0
ARMS = ("panda_no_gripper", "iiwa7")
OTHERS = ("fetch", "allegro_left", "2link_robot", "iiwa7_allegro")
ALL_FLAGS = [(g, d) for g in (True, False) for d in (True, False)]
ARRAYS = ("dtau_dq", "dtau_dqd", "dtau_dqdd")
GRAVITY = 9.81


@functools.lru_cache(maxsize=None)
def model_on(robot, device="cpu", compat=True):
    return load_model(robot, device, reference_compat=compat)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN_DIR, "golden_id_derivatives.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def states(robot):
    g = np.load(os.path.join(GOLDEN_DIR, "golden_fd_derivatives.npz"), allow_pickle=False)
    return g[robot + "/q"][:ROWS], g[robot + "/qd"][:ROWS], fixture()[robot + "/qdd"][:ROWS]


# ------------------------------------------------------------------------------------------------------------------- metric
def err(X, X64):
    X, X64 = np.asarray(X, np.float64).reshape(len(X64), -1), np.asarray(X64, np.float64).reshape(len(X64), -1)
    scale = np.abs(X64).max(1)
    live = scale > 0
    return float((np.abs(X - X64).max(1)[live] / scale[live]).max()) if live.any() else 0.0


def report(robot, flags, path, array, e, ey):
    print("IDD %-17s g%d d%d %-18s %-9s %.3e  %.3e  %.2f" % (robot, flags[0], flags[1], path, array, e, ey, e / ey))


# ------------------------------------------------------------------------------------------------------------------- truth
def central(fun, x, h):
    """[B, n, n] fp64: d fun_i / d x_j by central differences at step h, one column of x at a time."""
    cols = []
    for j in range(x.shape[1]):
        d = np.zeros_like(x)
        d[:, j] = h
        cols.append((fun(x + d) - fun(x - d)) / (2 * h))
    return np.stack(cols, 2)


def richardson(f, h):
    return (9.0 * f(h) - f(3.0 * h)) / 8.0


def build_truth(spec, q, qd, qdd):
    """dict: dq[gravity], dqd[damping], tau[(gravity, damping)], H64, H32, apart; the truth checked against itself first."""
    orc = Oracle(spec)
    q32, (q, qd, qdd) = q, (x.astype(np.float64) for x in (q, qd, qdd))
    t = dict(dq={}, dqd={}, tau={})
    for flag in (True, False):
        dq = lambda h: central(lambda x: orc.rnea(x, qd, qdd, flag, False, np.float64), q, h)
        dqd = lambda h: central(lambda x: orc.rnea(q, x, qdd, True, flag, np.float64), qd, h)
        t["dq"][flag], t["dqd"][flag] = richardson(dq, 1e-4), richardson(dqd, 1e-4)
        for name, f in (("dq", dq), ("dqd", dqd)):
            pin = err(richardson(f, 2e-4), t[name][flag])
            assert pin <= 1e-8, (name, flag, pin)            # the truth itself, before anything under test
    for flags in ALL_FLAGS:
        t["tau"][flags] = orc.rnea(q, qd, qdd, flags[0], flags[1], np.float64)
    t["H64"] = orc.mass_matrix(q, True, False, np.float64)
    t["H32"] = orc.mass_matrix(q32.astype(np.float32), True, False, np.float32)
    assert t["H32"].dtype == np.float32
    t["apart"] = different_branches(spec)
    for M in (t["dq"][True], t["dq"][False], t["dqd"][True], t["dqd"][False], t["H64"]):
        assert (M[:, t["apart"]] == 0).all(), "the truth itself must vanish between different branches in every row"
    return t


@functools.lru_cache(maxsize=None)
def truth(robot, compat=True):
    return build_truth(model_on(robot, "cpu", compat)._spec, *states(robot))


def truth_of(t, flags):
    return t["dq"][flags[0]], t["dqd"][flags[1]], t["H64"]


# --------------------------------------------------------------------------------------- the recursion in numpy, link-local frames
def id_derivatives_local(spec, q, qd, qdd, gravity, damping, dt):
    """(tau [B, n], dtau_dq, dtau_dqd, H [B, n, n]) in dtype dt: ONE sweep out and one back, every quantity in its link's own frame
    (Featherstone's convention, spatial vectors [angular; linear] at the link's origin).  X_i maps a motion of the parent's frame
    into link i's; forces and the composites go up through X_i^T.
        out    v_i = X v_p + S_i qd_i,  a_i = X a_p + S_i qdd_i + v_i x S_i qd_i  (a_base = (0, 0, +9.81) stands for gravity)
               IC_i = I_i,  BC_i = (crf(v) I - I crm(v) + bar(I v)) / 2,  fC_i = I a + v x* I v
        back   Pd_j = v_j x S_j,  Pdd_j = a_j x S_j + v_j x Pd_j        (the link's OWN velocity and acceleration serve: S_j x S_j = 0)
               F1 = IC Pdd_j + 2 BC Pd_j + S_j x* fC,  F2 = 2 (IC Pd_j + BC S_j),  F3 = BC^T S_j,  F4 = IC S_j,  tau_j = S_j . fC
               up the ancestors i of j (i = j included; the four wrenches moved by each joint transform on the way):
                   dq[i, j] = S_i . F1      dqd[i, j] = S_i . F2      H[i, j] = H[j, i] = S_i . F4
                   dq[j, i] = 2 Pd_i . F3 + Pdd_i . F4      dqd[j, i] = 2 (S_i . F3 + Pd_i . F4)        (i != j)
               IC, BC, fC of the parent += the link's (moved into the parent's frame)."""
    dt = np.dtype(dt).type
    q, qd, qdd = q.astype(dt), qd.astype(dt), qdd.astype(dt)
    B, n = q.shape
    L = int(len(spec.parent))
    kind = getattr(spec, "kind", None)
    eye3 = np.eye(3, dtype=dt)
    X, S, v, a, IC, BC, fC = ([None] * L for _ in range(7))
    zero6 = np.zeros((B, 6), dt)
    grav = np.zeros((B, 6), dt)
    if gravity:
        grav[:, 5] = dt(GRAVITY)
    mv = lambda M, x: np.einsum("bij,bj->bi", M, x)
    mtv = lambda M, x: np.einsum("bji,bj->bi", M, x)
    dot = lambda x, y: np.einsum("bi,bi->b", x, y)
    order = [i for i in range(L) if spec.parent[i] >= 0]
    assert all(spec.parent[i] < i for i in order), "parents precede their children"
    for i in order:
        p, d = int(spec.parent[i]), int(spec.dof[i])
        E = np.broadcast_to(_rpy(spec.rpy[i], dt), (B, 3, 3))
        r = np.broadcast_to(spec.trans[i].astype(dt), (B, 3))
        if d >= 0:
            ax = spec.axis[i].astype(np.float64)
            ax = (ax / (np.linalg.norm(ax) or 1.0)).astype(dt)
            if kind is not None and int(kind[i]) == 2:
                r = r + (E @ ax)[:, :] * q[:, d:d + 1]
                S[i] = np.broadcast_to(np.concatenate([np.zeros(3, dt), ax]), (B, 6))
            else:
                K = _skew(ax)
                sn, cs = np.sin(q[:, d])[:, None, None], np.cos(q[:, d])[:, None, None]
                E = E @ (eye3 + sn * K + (dt(1) - cs) * (K @ K))
                S[i] = np.broadcast_to(np.concatenate([ax, np.zeros(3, dt)]), (B, 6))
        Et = np.swapaxes(E, -1, -2)
        Xi = np.zeros((B, 6, 6), dt)
        Xi[:, :3, :3] = Xi[:, 3:, 3:] = Et
        Xi[:, 3:, :3] = -Et @ _skew(r)
        X[i] = Xi
        vp, ap = (v[p], a[p]) if v[p] is not None else (zero6, grav)
        v[i], a[i] = mv(Xi, vp), mv(Xi, ap)
        if d >= 0:
            v[i] = v[i] + S[i] * qd[:, d:d + 1]
            a[i] = a[i] + S[i] * qdd[:, d:d + 1] + mv(_crm(v[i]), S[i]) * qd[:, d:d + 1]
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
        fC[i] = np.einsum("ij,bj->bi", I, a[i]) + mv(_crf(v[i]), Iv)
    tau, dq, dqd, H = np.zeros((B, n), dt), np.zeros((B, n, n), dt), np.zeros((B, n, n), dt), np.zeros((B, n, n), dt)
    two = dt(2)
    for j in reversed(order):
        dj, p = int(spec.dof[j]), int(spec.parent[j])
        if dj >= 0:
            Pd = mv(_crm(v[j]), S[j])
            Pdd = mv(_crm(a[j]), S[j]) + mv(_crm(v[j]), Pd)
            F1 = mv(IC[j], Pdd) + two * mv(BC[j], Pd) + mv(_crf(S[j]), fC[j])
            F2 = two * (mv(IC[j], Pd) + mv(BC[j], S[j]))
            F3 = mtv(BC[j], S[j])
            F4 = mv(IC[j], S[j])
            tau[:, dj] = dot(S[j], fC[j])
            if damping:
                tau[:, dj] += dt(spec.damping[j]) * qd[:, dj]
                dqd[:, dj, dj] = dt(spec.damping[j])
            i = j
            while i > 0 and X[i] is not None:
                di = int(spec.dof[i])
                if di >= 0:
                    dq[:, di, dj] = dot(S[i], F1)
                    H[:, di, dj] = H[:, dj, di] = dot(S[i], F4)
                    if i == j:
                        dqd[:, di, dj] += dot(S[i], F2)
                    else:
                        dqd[:, di, dj] = dot(S[i], F2)
                        Pdi = mv(_crm(v[i]), S[i])
                        Pddi = mv(_crm(a[i]), S[i]) + mv(_crm(v[i]), Pdi)
                        dq[:, dj, di] = two * dot(Pdi, F3) + dot(Pddi, F4)
                        dqd[:, dj, di] = two * (dot(S[i], F3) + dot(Pdi, F4))
                F1, F2, F3, F4 = (mtv(X[i], F) for F in (F1, F2, F3, F4))
                i = int(spec.parent[i])
        if v[p] is not None:
            Xt = np.swapaxes(X[j], -1, -2)
            IC[p] = IC[p] + Xt @ IC[j] @ X[j]
            BC[p] = BC[p] + Xt @ BC[j] @ X[j]
            fC[p] = fC[p] + mtv(X[j], fC[j])
    return tau, dq, dqd, H


def restatement_check(robot, spec, t, inputs):
    """The numpy recursion in fp64 against the truth: 1e-8 relative, every flag combination."""
    for flags in ALL_FLAGS:
        tau, dq, dqd, H = id_derivatives_local(spec, *inputs, flags[0], flags[1], np.float64)
        for name, X, T in zip(("tau",) + ARRAYS, (tau, dq, dqd, H), (t["tau"][flags],) + truth_of(t, flags)):
            e = err(X, T)
            report(robot, flags, "numpy-fp64", name, e, 1e-8)
            assert e <= 1e-8, (name, flags, e)
        assert (dq[:, t["apart"]] == 0).all() and (dqd[:, t["apart"]] == 0).all() and (H[:, t["apart"]] == 0).all()


# ------------------------------------------------------------------------------------------------------------------- yardsticks
def reference_yardsticks(robot):
    """(fun(flags, held) -> (ref_dq, ref_dqd), rows the fixture holds) from the unmodified reference's Jacobians."""
    g = fixture()
    tag = lambda on: "on" if on else "off"
    held = len(g[robot + "/ref_dq_on"])
    return (lambda flags: (g["%s/ref_dq_%s" % (robot, tag(flags[0]))], g["%s/ref_dqd_%s" % (robot, tag(flags[1]))])), held


def local32_yardsticks(spec, inputs):
    """The same from the numpy recursion in float32, for models the reference does not describe."""
    @functools.lru_cache(maxsize=None)
    def fun(flags):
        out = id_derivatives_local(spec, *inputs, flags[0], flags[1], np.float32)
        assert out[1].dtype == np.float32
        return out[1], out[2]
    return fun, len(inputs[0])


def check_all(robot, flags, path, out, t=None, yard=None, first=0):
    """The 8 x rule for the three matrices over rows [first, first + len(out)), and the structure.  Returns the worst ratio."""
    t = t or truth(robot)
    fun, held = yard or reference_yardsticks(robot)
    got = [np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in out]
    B, n = got[0].shape
    rows = slice(first, first + B)
    assert all(g.dtype == np.float32 for g in got) and all(g.shape == (B, n, n) for g in got[1:])
    want = [T[rows] for T in truth_of(t, flags)]
    ref = fun(flags)
    hr = slice(first, max(first, min(first + B, held)))           # the rows of this launch the yardstick holds
    yards = [err(ref[0][hr], truth_of(t, flags)[0][hr]) if hr.stop > hr.start else 0.0,
             err(ref[1][hr], truth_of(t, flags)[1][hr]) if hr.stop > hr.start else 0.0,
             err(t["H32"][rows], want[2])]
    bad, worst = [], 0.0
    for k, name in enumerate(ARRAYS):
        e, ey = err(got[1 + k], want[k]), max(yards[k], FLOOR)
        report(robot, flags, path, name, e, ey)
        worst = max(worst, e / ey)
        if not e <= MARGIN * ey:
            bad.append((name, e, ey))
    assert not bad, bad
    assert np.array_equal(got[3], got[3].transpose(0, 2, 1)), "dtau_dqdd must be symmetric to the bit"
    for g in got[1:]:
        assert (g[:, t["apart"]] == 0).all(), "entries between different branches must be exactly zero"
    return worst


def run_model(model, inputs, flags, B=None, composed=False):
    """compute_inverse_dynamics_derivatives over the rows in consecutive launches of B rows (None: one launch); tau is compared
    with compute_inverse_dynamics of the same launches on the way."""
    q, qd, qdd = (torch.from_numpy(np.ascontiguousarray(x)).to(model._device) for x in inputs)
    N = q.shape[0]
    B = B or N
    outs = []
    for i in range(0, N, B):
        o = model.compute_inverse_dynamics_derivatives(q[i:i + B], qd[i:i + B], qdd[i:i + B], flags[0], flags[1], _composed=composed)
        assert type(o).__name__ == "InverseDynamicsDerivatives" and o._fields == ("tau", "dtau_dq", "dtau_dqd", "dtau_dqdd")
        assert all(x.grad_fn is None and not x.requires_grad and x.dtype == torch.float32 for x in o)
        tau = model.compute_inverse_dynamics(q[i:i + B], qd[i:i + B], qdd[i:i + B], include_gravity=flags[0], use_damping=flags[1])
        torch.testing.assert_close(o.tau, tau, atol=2e-5, rtol=2e-5)
        outs.append(o)
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))


def run_and_check(robot, device, flags, path, B=None, composed=False, compat=True):
    model = model_on(robot, device, compat)
    out = run_model(model, states(robot), flags, B=B, composed=composed)
    if device != "cpu":
        torch.cuda.synchronize()
    t = truth(robot, compat)
    yard = None if compat else local32_yardsticks(model_on(robot, "cpu", compat)._spec, states(robot))
    scale = np.abs(t["tau"][flags]).max()
    e = np.abs(out[0].cpu().numpy() - t["tau"][flags]).max() / scale
    report(robot, flags, path, "tau", e, FLOOR)
    check_all(robot, flags, path, out, t=t, yard=yard)
    return model


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("robot", ARMS + OTHERS)
def test_numpy_restatement_in_fp64_is_the_truth(robot):
    restatement_check(robot, model_on(robot)._spec, truth(robot), states(robot))


def test_cross_branch_set_is_not_empty():
    for robot in ("fetch", "allegro_left", "iiwa7_allegro"):
        assert truth(robot)["apart"].any()
    assert int(truth("allegro_left")["apart"].sum()) == 192        # four fingers of four joints: 256 - 4 * 16
    for robot in ARMS + ("2link_robot",):
        assert not truth(robot)["apart"].any()


@pytest.mark.parametrize("flags", ALL_FLAGS, ids=lambda f: "g%d-d%d" % f)
@pytest.mark.parametrize("robot", ARMS + OTHERS)
def test_host_build_against_truth(cpu_library, robot, flags):
    run_and_check(robot, "cpu", flags, "host")


def test_fetch_with_sliding_joints(cpu_library):
    model = model_on("fetch", "cpu", False)
    assert (model._spec.kind == 2).any()
    restatement_check("fetch-prismatic", model._spec, truth("fetch", False), states("fetch"))
    for flags in ((True, True), (False, False)):
        run_and_check("fetch", "cpu", flags, "host-prismatic", compat=False)


def skew_check(tmp_path_factory, device, path):
    """tests/test_joint_models.py's toy robot: prismatic about z, revolute and prismatic about skew axes (two ops per skew link)."""
    from helpers import sample_states
    from test_joint_models import toy_model, toy_urdf
    urdf = tmp_path_factory.mktemp("toy_idd") / "toy.urdf"
    urdf.write_text(toy_urdf())
    model = toy_model(str(urdf), device)
    assert model._spec.skew.any()
    inputs = sample_states(model, 65, seed=1)
    t = build_truth(model._spec, *inputs)
    if device == "cpu":
        restatement_check("toy_skew", model._spec, t, inputs)
    yard = local32_yardsticks(model._spec, inputs)
    for flags in ((True, True), (False, False)):
        check_all("toy_skew", flags, path, run_model(model, inputs, flags), t=t, yard=yard)


def test_skew_axis_model(cpu_library, tmp_path_factory):
    skew_check(tmp_path_factory, "cpu", "host")


def interface_check(device):
    """Unbatched inputs, shapes, the namedtuple, B == 0, mismatched batches, no grad_fn, _composed and the environment switch."""
    from differentiable_robot_model_amd import InverseDynamicsDerivatives
    model = model_on("iiwa7", device)
    q, qd, qdd = (torch.from_numpy(x[:3].copy()).to(device) for x in states("iiwa7"))
    many = model.compute_inverse_dynamics_derivatives(q.clone().requires_grad_(True), qd.clone().requires_grad_(True), qdd)
    assert type(many) is InverseDynamicsDerivatives and many._fields == ("tau", "dtau_dq", "dtau_dqd", "dtau_dqdd")
    assert many.tau.shape == (3, 7) and all(x.shape == (3, 7, 7) for x in many[1:])
    assert all(x.grad_fn is None and not x.requires_grad and x.dtype == torch.float32 for x in many)
    one = model.compute_inverse_dynamics_derivatives(q[1], qd[1], qdd[1])
    assert one.tau.shape == (7,) and all(x.shape == (7, 7) for x in one[1:])
    assert all(torch.equal(a, b[1]) for a, b in zip(one, many))
    e = torch.empty(0, 7, device=device)
    out = model.compute_inverse_dynamics_derivatives(e, e, e)
    assert out.tau.shape == (0, 7) and all(x.shape == (0, 7, 7) for x in out[1:])
    with pytest.raises(AssertionError):
        model.compute_inverse_dynamics_derivatives(q, qd[:2], qdd)
    # the definitions: dtau_dqdd is compute_lagrangian_inertia_matrix; the defaults are gravity on, damping off
    H = model.compute_lagrangian_inertia_matrix(q)
    assert torch.allclose(many.dtau_dqdd, H, atol=1e-5)
    same = model.compute_inverse_dynamics_derivatives(q, qd, qdd, True, False)
    assert all(torch.equal(a, b) for a, b in zip(same, many))
    # damping enters dtau_dqd as diag(damping) and tau, never dtau_dq; gravity never enters dtau_dqd
    damped = model.compute_inverse_dynamics_derivatives(q, qd, qdd, True, True)
    nograv = model.compute_inverse_dynamics_derivatives(q, qd, qdd, False, False)
    assert torch.equal(damped.dtau_dq, many.dtau_dq) and torch.equal(nograv.dtau_dqd, many.dtau_dqd)
    off = damped.dtau_dqd - many.dtau_dqd
    assert (off.diagonal(dim1=1, dim2=2) > 0).all() and (off - torch.diag_embed(off.diagonal(dim1=1, dim2=2)) == 0).all()
    # _composed and DRM_IDD_COMPOSED=1 take the general kernel on every row
    a = model.compute_inverse_dynamics_derivatives(q, qd, qdd, _composed=True)
    os.environ["DRM_IDD_COMPOSED"] = "1"
    try:
        b = model.compute_inverse_dynamics_derivatives(q, qd, qdd)
    finally:
        os.environ.pop("DRM_IDD_COMPOSED", None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.allclose(x, y, atol=1e-4) for x, y in zip(a, many))


def test_interface(cpu_library):
    interface_check("cpu")


def test_host_composed_flag_is_accepted(cpu_library):
    model = model_on("panda_no_gripper")
    a = run_model(model, states("panda_no_gripper"), (True, True))
    b = run_model(model, states("panda_no_gripper"), (True, True), composed=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))      # (the host build has one path)


def c_abi_null_check(lib, model, device, stream, B=5):
    """Each of tau, dtau_dq, dtau_dqd, H NULL in turn gives the other three to the bit; all NULL is DRM_ERR_INVALID; B == 0 is
    DRM_OK and writes nothing; NULL inputs and a negative batch are DRM_ERR_INVALID."""
    walk, n = walk_of(model), model._n_dofs
    q, qd, qdd = (torch.from_numpy(x[:B].copy()).to(device) for x in states("panda_no_gripper"))
    need = int(lib.drm_rnea_derivatives_scratch_floats(ctypes.byref(walk), B))
    scratch = torch.empty(max(need, 1), device=device)
    sizes = (B * n, B * n * n, B * n * n, B * n * n)
    flags = 3

    def call(which, ins=None, rows=B):
        outs = [torch.full((s + 8,), 7.5, device=device) for s in sizes]
        ptr = [o.data_ptr() if w else None for o, w in zip(outs, which)]
        a = ins or (q.data_ptr(), qd.data_ptr(), qdd.data_ptr())
        rc = lib.drm_rnea_derivatives(ctypes.byref(walk), a[0], a[1], a[2], rows, flags, ptr[0], ptr[1], ptr[2], ptr[3],
                                      scratch.data_ptr(), stream)
        if device != "cpu":
            torch.cuda.synchronize()
        return rc, outs
    rc, full = call((True,) * 4)
    assert rc == 0
    for o, s in zip(full, sizes):
        assert (o[s:] == 7.5).all() and torch.isfinite(o[:s]).all()
    for drop in range(4):
        which = tuple(i != drop for i in range(4))
        rc, part = call(which)
        assert rc == 0
        for i in range(4):
            assert torch.equal(part[i], full[i]) if which[i] else (part[i] == 7.5).all()
    assert call((False,) * 4)[0] == -1
    rc, outs = call((True,) * 4, rows=0)
    assert rc == 0 and all((o == 7.5).all() for o in outs)
    assert call((True,) * 4, rows=-1)[0] == -1
    for drop in range(3):
        ins = [q.data_ptr(), qd.data_ptr(), qdd.data_ptr()]
        ins[drop] = None
        assert call((True,) * 4, ins=tuple(ins))[0] == -1


def test_c_abi_codes_on_the_host_build(cpu_library):
    from differentiable_robot_model_amd import backend
    lib = backend.load_library(kind="cpu")
    assert lib.drm_abi_version() == 15
    model = model_on("panda_no_gripper")
    c_abi_null_check(lib, model, "cpu", None)
    walk = walk_of(model)
    assert lib.drm_rnea_derivatives_scratch_floats(ctypes.byref(walk), 128) == 0
    assert lib.drm_rnea_derivatives_scratch_floats_aligned(ctypes.byref(walk), 128) == 0


def bad_rows_check(model, device, composed=False, B=128):
    """q[5] NaN, qd[70] Inf, q[3] = 2e9, qdd[90] NaN: every other row keeps its bits, those four are NaN in every output."""
    q, qd, qdd = (torch.from_numpy(x[:B].copy()).to(device) for x in states("panda_no_gripper"))
    run = lambda: model.compute_inverse_dynamics_derivatives(q, qd, qdd, True, True, _composed=composed)
    clean = run()
    q[5, 2] = float("nan")
    qd[70, 4] = float("inf")
    q[3, 1] = 2e9
    qdd[90, 6] = float("nan")
    got = run()
    bad = [3, 5, 70, 90]
    others = torch.ones(B, dtype=torch.bool, device=device)
    others[bad] = False
    for a, b in zip(got, clean):
        assert torch.equal(a[others], b[others])
        assert torch.isfinite(b).all()
    for r in bad:
        assert all(torch.isnan(x[r]).all() for x in got)


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
    inputs, flags = states(robot), (True, True)
    t = build_truth(spec, *inputs)
    assert err(t["dq"][True], truth(robot)["dq"][True]) > 1e-3       # (the moved link changes the answer)
    check_all(robot, flags, path, run_model(model, inputs, flags), t=t, yard=local32_yardsticks(spec, inputs))


def test_learnable_link(cpu_library):
    learnable_check("cpu", "host-learnable")


def long_chain_check(tmp_path, device, path):
    """test_max_sizes.chain_model's 30-joint chain (joints about +-x / +-y / +-z), 65 rows."""
    from helpers import sample_states
    from test_max_sizes import chain_model
    model = chain_model(tmp_path, 30, device)
    inputs, flags = sample_states(model, 65, seed=0), (True, True)
    t = build_truth(model._spec, *inputs)
    check_all("chain30", flags, path, run_model(model, inputs, flags), t=t, yard=local32_yardsticks(model._spec, inputs))
    return model


def test_long_chain(cpu_library, tmp_path):
    long_chain_check(tmp_path, "cpu", "host")


# ------------------------------------------------------------------------------------------------------------------- GPU
def gpu_run_and_check(robot, B, flags=(True, True), composed=False, compat=True, path=None):
    name = path or ("general" if composed or robot not in ARMS or B < 64 else "fused") + "-B%d" % B
    return run_and_check(robot, "cuda:0", flags, name, B=B, composed=composed, compat=compat)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 128, 131])
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_against_truth(robot, B):
    for flags in ALL_FLAGS if B in (64, 65) else ((True, True), (False, False)):
        gpu_run_and_check(robot, B, flags)


@pytest.mark.gpu
def test_gpu_arm_general_kernel():
    for flags in ALL_FLAGS:
        gpu_run_and_check("panda_no_gripper", 128, flags, composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", OTHERS)
def test_gpu_other_robots_against_truth(robot):
    for flags in ALL_FLAGS:
        gpu_run_and_check(robot, 65, flags)


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
    assert backend.load_library().drm_rnea_derivatives_scratch_floats(ctypes.byref(walk_of(model)), 65) > 0


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
    """Straight through the C ABI: the inputs and all four outputs 4 bytes off a 16-byte boundary (the general kernel), a scratch
    of exactly drm_rnea_derivatives_scratch_floats floats, guard words behind the scratch and on both sides of every output."""
    from differentiable_robot_model_amd import backend
    model = model_on(robot, "cuda:0")
    lib, walk, n = backend.load_library(), walk_of(model), model._n_dofs

    def off_by_4(x):
        buf = torch.zeros(x.numel() + 1, device="cuda")
        buf[1:] = x.reshape(-1)
        view = buf[1:].view(x.shape)
        assert view.data_ptr() % 16 == 4
        return view
    q, qd, qdd = (off_by_4(torch.from_numpy(x).cuda()) for x in states(robot))
    need = int(lib.drm_rnea_derivatives_scratch_floats(ctypes.byref(walk), ROWS))
    assert (need > 0) == (robot == "iiwa7_allegro")
    GUARD = 64
    scratch = torch.full((need + GUARD,), 3.25, device="cuda")
    sizes = (ROWS * n, ROWS * n * n, ROWS * n * n, ROWS * n * n)
    bufs = [torch.full((1 + s + GUARD,), -1.5, device="cuda") for s in sizes]
    outs = [b[1:1 + s] for b, s in zip(bufs, sizes)]
    assert all(o.data_ptr() % 16 == 4 for o in outs)
    rc = lib.drm_rnea_derivatives(ctypes.byref(walk), q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), ROWS, 3, outs[0].data_ptr(),
                                  outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), scratch.data_ptr(), backend._stream(q.device))
    torch.cuda.synchronize()
    assert rc == 0
    assert (scratch[need:] == 3.25).all()
    for b, s in zip(bufs, sizes):
        assert (b[1 + s:] == -1.5).all() and b[0] == -1.5
    check_all(robot, (True, True), "misaligned", [outs[0].view(ROWS, n)] + [o.view(ROWS, n, n) for o in outs[1:]])


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_non_finite_rows(composed):
    bad_rows_check(model_on("panda_no_gripper", "cuda:0"), "cuda", composed=composed)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_learnable_link():
    learnable_check("cuda:0", "learnable")

"""Gradients of contact torques and contact rollouts (csrc/drm_contact.hpp contact_wrench_vjp, drm_contact_torques_vjp;
compute_contact_torques_vjp, compute_contact_torques / compute_contact_rollout with differentiable=True) held to fp64.

Every check is one function of the device: it runs un-marked on the host build and under -m gpu on cuda:0, where the paths are the
fused arm kernel (Panda with and without its own kernels, iiwa7, the Fetch arm at full 64-row tiles), the composed path (_composed, the
B % 64 tail, B = 1, every other robot, a link subset, misaligned pointers) and, for the rollout, the reverse sweep over the states of
the fused (B = 64) and the composed (row 64 of B = 65) forward.

TRUTH (fp64, not code under test): S = lam . tau of test_contact_rollout.reference(..., np.float64) (restated here as reference_m for a
model that is not that file's cached one — the Fetch with its sliding joint — and asserted equal to it); for the rollout the fp64
step-by-step rollout built from the same reference and the oracle's fp64 forward dynamics, with test_rollout_edges' loss
L = sum Wq . q + Wv . qd.  Central differences at h = 1e-4 and 5e-5, Richardson-combined ((4 D(h/2) - D(h)) / 3).

YARDSTICK (float32, not code under test): the composition of the issue in numpy float32 — test_links_dq.power_dq_world twice, the
oracle's float32 Jacobians for the two J^T products, the law's backward written out in numpy (law_vjp).  Run in float64 it must first
match the truth to 1e-8 of max|truth| on the rows kept (printed as "pin").  For the rollout: the float32 reverse sweep of
test_rollout_edges.yardstick_gradients (per-step Jacobians of test_fd_derivatives.build_problem at the fp64 trajectory's states and
total torques) with that contact VJP added per step.

REQUIREMENT, the project's standing rule:   err(path) <= 8 max(err(yardstick), 2^-23 scale)
torques: err = max |x - truth| over the rows kept, scale = max |truth|; rollout: test_rollout_edges.check_gradients' metric, the error
relative to the dynamics' share max|g64 - g_kin| with the integrator's identity left out.  One CONTACTGRAD line per comparison is
printed before it asserts; profiles/contact_grad_tests.txt holds them for the host build and the MI355X.

SWITCHES.  The law is not differentiable where depth, k depth - c v_n, c_t |v_t| - mu f_n, q - lower or upper - q changes sign.  A row
is left out of a gradient comparison when the sign pattern (depth > 0, f_n > 0, saturated, below, above) at any stencil point — for a
rollout at any step of any stencil trajectory — differs from the base point's: exact detection, no margin.  Asserted: at most 5 % of
the rows per torque case, at most 10 % per rollout case; test_contact_rollout.activity's floors (25 % of the contact points active,
both friction regimes, 5 % of the coordinates on their springs) wherever the robot can meet them (the 2-link robot has two contact
links and continuous joints: its floors are the active share alone).

Rollout cases: T = 4, dt = 1e-3, seed ROLLOUT_SEEDS (101 for both robots), the first tried; with the fp64 reference alone it leaves no
compared row out: 0 of 4 on the host shapes (B = 4), 0 of 10 on the GPU shapes (B = 64: rows 0 - 9; B = 65: rows 0 - 8 and the tail
row 64), for both integrators with and without gravity.  The torque cases leave out 0 to 0.8 % of their rows.

Measured (profiles/contact_grad_tests.txt): the worst err(path) / bound is 2.98 on the host build (Panda, the link subset, grad_qd) and
2.62 on the MI355X (Panda, misaligned pointers at B = 128, grad_q; 2.33 on the fused kernel); the rollouts' worst is 1.11.  The fp64
yardstick lies within 8e-11 of max|truth| of the truth.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_contact_rollout as tcr
from differentiable_robot_model_amd import JointLimitSprings, backend
from helpers import load_model
from oracle import Oracle
from test_contact_rollout import (SOFT, SOFT_HAND, SPRINGS_ARM, SPRINGS_HAND, SUBSET, TILTED, bounds_of, law, median_offset,  # noqa: F401
                                  plane_of, reference, rollout_case, soft, springs_of, springs_par, states, unit)
from test_fd_derivatives import FLOOR, MARGIN, build_problem
from test_links_dq import power_dq_world
from test_rollout import INTEGRATORS
from test_rollout_edges import ARRAYS, FILL, GUARD, SENTINEL, kinematic_gradients, place, to

GPU = "cuda:0"
DT = 1e-3
H = 1e-4
PIN = 1e-8
Z = (0.0, 0.0, 1.0)
PRISMATIC = "fetch"          # loaded with its sliding joint (reference_compat=False)
HOST_ROBOTS = ("panda_no_gripper", "iiwa7", "fetch_arm_no_gripper", "allegro_left", "2link_robot", PRISMATIC)
PANDA = "panda_no_gripper"
PANDA_SUBSET = tuple(SUBSET[PANDA]) + ("panda_link0", "panda_link2")      # the caller's order, the root, a repeat


@functools.lru_cache(maxsize=None)
def model(robot, dev="cpu", own=None):
    if robot != PRISMATIC:
        return tcr.model(robot, dev, own)
    return load_model(robot, dev, reference_compat=False)


@functools.lru_cache(maxsize=None)
def oracle(robot):
    return tcr.oracle(robot) if robot != PRISMATIC else Oracle(model(robot)._spec)


def names_of(robot, names):
    return list(model(robot).get_link_names()) if names is None else list(names)


def line(check, robot, path, array, err, yard, scale):
    bound = max(yard, FLOOR * scale)
    print("CONTACTGRAD %-14s %-22s %-22s %-8s %.3e  %.3e  %.2f" % (check, robot, path, array, err, bound, err / bound if bound > 0 else 0.0))
    return err <= MARGIN * bound


# ------------------------------------------------------------------------------------------------------------------- the truth


def reference_m(robot, names, q, qd, normal, offset, par, radii, springs, dt):
    """test_contact_rollout.reference for this file's models (the same recursion), plus the sign pattern of every switch:
    tau [B, n], depth / saturated [B, L], lim_active [B, n], pattern [B, K] bool"""
    m, orc = model(robot), oracle(robot)
    q, qd = np.asarray(q, dt), np.asarray(qd, dt)
    B, n = q.shape
    tau = np.zeros((B, n), dt)
    D, S, P = [], [], []
    seen = set()
    if normal is not None:
        nn = unit(normal)
        radii = np.broadcast_to(np.asarray(radii, np.float64), (len(names),))
        for name, rl in zip(names, radii):
            idx = m._name_to_idx_map[name]
            if idx == 0 or idx in seen:
                continue
            seen.add(idx)
            pos, _, lin, ang = orc.fk_jacobian(q, idx, dt)
            v, w = np.einsum("bij,bj->bi", lin, qd), np.einsum("bij,bj->bi", ang, qd)
            f, mo, depth, sat = law(pos, v, w, nn, offset, par, np.full(B, rl), dt)
            tau += np.einsum("bij,bi->bj", lin, f) + np.einsum("bij,bi->bj", ang, mo)
            D.append(depth); S.append(sat); P.append((f * nn.astype(dt)).sum(-1) > 0)
    out = dict(depth=np.stack(D, 1) if D else np.zeros((B, 0)), saturated=np.stack(S, 1) if S else np.zeros((B, 0), bool))
    pattern = [out["depth"] > 0, np.stack(P, 1) if P else np.zeros((B, 0), bool), out["saturated"]]
    out["lim_active"] = np.zeros((B, n), bool)
    if springs is not None:
        lo, hi = bounds_of(m)
        t, act, _ = springs_of(q, qd, lo, hi, springs[0], springs[1], dt)
        tau = tau + t
        out["lim_active"] = act
        pattern += [q < lo.astype(dt), q > hi.astype(dt)]
    out["tau"] = tau.astype(dt)
    out["pattern"] = np.concatenate(pattern, 1)
    return out


def law_vjp(p, v, w, a, b, n, d, par, radius, dt):
    """test_contact_rollout.law and its backward in dtype dt: the cotangents (a, b) of (force, moment) -> (force, moment, gp, gv, gw),
    the branches of the forward taken"""
    n = n.astype(dt)
    k, c, mu, ct = (dt(par[x]) for x in ("stiffness", "damping", "friction", "friction_slope"))
    rl = np.asarray(radius, dt)[..., None]
    r = -rl * n
    depth = rl[..., 0] - ((p * n).sum(-1) - dt(d))
    vc = v + np.cross(w, r)
    vn = (vc * n).sum(-1)
    vt = vc - vn[..., None] * n
    pre = k * depth - c * vn
    push = (depth > 0) & (pre > 0)
    fn = np.where(push, pre, dt(0)).astype(dt)
    speed = np.sqrt((vt * vt).sum(-1))
    sp = np.where(speed > 0, speed, dt(1)).astype(dt)
    cap = mu * fn
    slides = (cap > 0) & (ct > 0) & (speed > 0)
    sat = slides & (cap / sp < ct)
    g = np.where(slides, np.where(sat, cap / sp, ct), dt(0)).astype(dt)
    f = fn[..., None] * n - g[..., None] * vt
    gf = a + np.cross(b, r)
    gfn = (gf * n).sum(-1)
    gg = -(gf * vt).sum(-1)
    gvt = -g[..., None] * gf
    gfn = gfn + np.where(sat, gg * mu / sp, dt(0))
    gvt = gvt + np.where(sat, -gg * g / sp / sp, dt(0))[..., None] * vt
    gpre = np.where(push, gfn, dt(0))
    gvn = -c * gpre - (gvt * n).sum(-1)
    gvc = np.where(push[..., None], gvt + gvn[..., None] * n, dt(0))
    gp = -(k * gpre)[..., None] * n
    return [x.astype(dt) for x in (f, np.cross(r, f), gp, gvc, np.cross(r, gvc))]


def yard_vjp(robot, names, q, qd, lam, normal, offset, par, radii, springs, dt):
    """(grad_q, grad_qd) [B, n] in dtype dt: the composition of the issue in numpy"""
    m, orc = model(robot), oracle(robot)
    spec = m._spec
    q, qd, lam = (np.asarray(x, dt) for x in (q, qd, lam))
    B, n = q.shape
    L = len(spec.parent)
    gq, gqd = np.zeros((B, n), dt), np.zeros((B, n), dt)
    if normal is not None:
        F, M, GV, GW = (np.zeros((B, L, 3), dt) for _ in range(4))
        seen = set()
        radii = np.broadcast_to(np.asarray(radii, np.float64), (len(names),))
        for name, rl in zip(names, radii):
            idx = m._name_to_idx_map[name]
            if idx == 0 or idx in seen:
                continue
            seen.add(idx)
            pos, _, lin, ang = orc.fk_jacobian(q, idx, dt)
            mul = lambda J, x: np.einsum("bij,bj->bi", J, x)
            f, mo, gp, gv, gw = law_vjp(pos, mul(lin, qd), mul(ang, qd), mul(lin, lam), mul(ang, lam), unit(normal), offset, par,
                                        np.full(B, rl), dt)
            F[:, idx], M[:, idx], GV[:, idx], GW[:, idx] = f, mo, gv, gw
            gqd = gqd + np.einsum("bij,bi->bj", lin, gv) + np.einsum("bij,bi->bj", ang, gw)
            gq = gq + np.einsum("bij,bi->bj", lin, gp)
        gq = gq + power_dq_world(spec, q, lam, F, M, dt) + power_dq_world(spec, q, qd, GV, GW, dt)
    if springs is not None:
        lo, hi = bounds_of(m)
        act = (q < lo.astype(dt)) | (q > hi.astype(dt))
        gq = gq + np.where(act, -dt(springs[0]) * lam, dt(0))
        gqd = gqd + np.where(act, -dt(springs[1]) * lam, dt(0))
    return gq.astype(dt), gqd.astype(dt)


def stencil(z, h):
    """[2 P B, P]: column j of all B rows moved by +h (first half) and -h at once; rows are independent"""
    B, P = z.shape
    zz = np.broadcast_to(z, (2, P, B, P)).copy()
    idx = np.arange(P)
    zz[0, idx, :, idx] += h
    zz[1, idx, :, idx] -= h
    return zz.reshape(2 * P * B, P)


def differences(per_row, z, base_pattern):
    """Richardson-combined central differences of the per-row scalar per_row(zz) -> (values [rows], pattern [rows, ...]) with respect
    to every column of z [B, P], and the rows whose sign pattern changes at some stencil point -> (grad [B, P], exclude [B])"""
    B, P = z.shape
    grads, exclude = [], np.zeros(B, bool)
    for h in (H, H / 2):
        val, pat = per_row(stencil(z, h))
        val = val.reshape(2, P, B)
        grads.append(((val[0] - val[1]) / (2 * h)).T)
        pat = pat.reshape((2 * P, B) + pat.shape[1:])
        exclude |= (pat != base_pattern[None]).reshape(2 * P, B, -1).any(2).any(0)
    return (4.0 * grads[1] - grads[0]) / 3.0, exclude


@functools.lru_cache(maxsize=None)
def torque_case(robot, B, mode, normal, radius, names, seed):
    """inputs, truth and yardstick of one torques-VJP case (shared by every path that runs it)"""
    m = model(robot)
    n = m._n_dofs
    q, qd = states(robot, B, seed, push=mode != "contact") if robot != PRISMATIC else prismatic_states(B, seed, mode != "contact")
    lam = np.random.default_rng(seed + 7).standard_normal((B, n)).astype(np.float32)
    link_names = names_of(robot, names)
    par = dict(soft(robot), radius=radius)
    springs = None if mode == "contact" else springs_par(robot)
    nrm = None if mode == "springs" else normal
    offset = None if nrm is None else offset_of(robot, q, nrm, radius)
    args = (nrm, offset, par, radius, springs)
    base = reference_m(robot, link_names, q, qd, *args, np.float64)
    lam64 = lam.astype(np.float64)

    def per_row(zz):
        r = reference_m(robot, link_names, zz[:, :n], zz[:, n:], *args, np.float64)
        return (np.tile(lam64, (len(zz) // B, 1)) * r["tau"]).sum(-1), r["pattern"]
    grad, exclude = differences(per_row, np.concatenate([q, qd], 1).astype(np.float64), base["pattern"])
    truth = (grad[:, :n], grad[:, n:])
    y64 = yard_vjp(robot, link_names, q, qd, lam, *args, np.float64)
    y32 = yard_vjp(robot, link_names, q, qd, lam, *args, np.float32)
    assert all(y.dtype == np.float32 for y in y32)
    keep = ~exclude
    tag = (robot, B, mode, normal, radius, seed)
    assert exclude.mean() <= 0.05, (tag, exclude.mean())
    for name, t, y in zip(("grad_q", "grad_qd"), truth, y64):
        scale = float(np.abs(t[keep]).max())
        pin = float(np.abs(y[keep] - t[keep]).max())
        print("CONTACTGRAD %-14s %-22s %-22s %-8s %.3e  (fp64 yardstick against the truth, max|truth| %.3e)" % ("pin", robot, mode, name, pin, scale))
        assert pin <= PIN * max(scale, 1e-300), (tag, name, pin, scale)
    # the case exercises the law (test_contact_rollout.activity's floors)
    active = base["depth"] > 0
    rich = robot != "2link_robot"
    if nrm is not None:
        assert active.mean() >= 0.25, (tag, active.mean())
        if rich:
            assert base["saturated"].any() and (active & ~base["saturated"]).any(), tag
    if springs is not None and rich:
        assert base["lim_active"].mean() >= 0.05, (tag, base["lim_active"].mean())
    return dict(q=q, qd=qd, lam=lam, names=link_names, contact=None if nrm is None else plane_of(nrm, offset, par), springs=springs,
                truth=truth, y32=y32, keep=keep, excluded=float(exclude.mean()))


def prismatic_states(B, seed, push):
    """test_contact_rollout.states for this file's model of the Fetch"""
    from helpers import sample_states
    m = model(PRISMATIC)
    q, qd, _ = sample_states(m, B, seed)
    if push:
        lo, hi = bounds_of(m)
        rng = np.random.default_rng(seed + 1000)
        u, amount = rng.random(q.shape), rng.uniform(0.0, 0.1, q.shape)
        fin = np.isfinite(lo) & np.isfinite(hi)
        q = np.where((u < 0.1) & fin, lo - amount, np.where((u > 0.9) & fin, hi + amount, q)).astype(np.float32)
    return q, qd


def offset_of(robot, q, normal, radius):
    if robot != PRISMATIC:
        return median_offset(robot, q, normal, radius)
    _, p = oracle(robot).fk_all_poses(q.astype(np.float64), np.float64)
    return float(np.median((p[:, 1:] * unit(normal)).sum(-1))) + (tcr.POINT_SHIFT if radius == 0.0 else 0.0)


def test_reference_m_is_the_contact_file_reference(cpu_library):
    q, qd = states(PANDA, 9, 3, push=True)
    names = names_of(PANDA, None)
    args = (Z, median_offset(PANDA, q, Z), soft(PANDA), soft(PANDA)["radius"], springs_par(PANDA))
    for dt in (np.float64, np.float32):
        assert np.array_equal(reference_m(PANDA, names, q, qd, *args, dt)["tau"], reference(PANDA, names, q, qd, *args, dt)["tau"])


# ------------------------------------------------------------------------------------------------------------------- 1  torques VJP


def call_vjp(m, dev, case, rows=slice(None), composed=False):
    jl = JointLimitSprings(*case["springs"]) if case["springs"] is not None else None
    q, qd, lam = to(dev, case["q"][rows], case["qd"][rows], case["lam"][rows])
    out = m.compute_contact_torques_vjp(q, qd, lam, case["contact"], link_names=case["names"], joint_limits=jl, _composed=composed)
    assert len(out) == 2 and not any(x.requires_grad for x in out)
    return [x.cpu().numpy() for x in out]


def compare_vjp(check, robot, path, got, case, rows=slice(None)):
    keep = case["keep"][rows]
    ok = True
    for name, x, t, y in zip(("grad_q", "grad_qd"), got, case["truth"], case["y32"]):
        t, y = t[rows][keep], y[rows][keep]
        assert x.shape == case["q"][rows].shape and np.isfinite(x).all(), (check, robot, path, name)
        if not keep.any():
            continue
        ok = line(check, robot, path, name, float(np.abs(x[keep] - t).max()), float(np.abs(y - t).max()), float(np.abs(t).max())) and ok
    assert ok, (check, robot, path)


TORQUE_CASES = (("both", Z, None), ("contact", TILTED, 0.0), ("springs", Z, None))


def radius_of(robot, radius):
    return soft(robot)["radius"] if radius is None else radius


def check_torques_vjp(robot, dev, B=65, own=None, composed=False, cases=TORQUE_CASES, names=None, path=None):
    m = model(robot, dev, own)
    path = path or ("host" if dev == "cpu" else "gpu")
    for mode, normal, radius in cases:
        case = torque_case(robot, B, mode, normal, radius_of(robot, radius), names, 11)
        got = call_vjp(m, dev, case, composed=composed)
        again = call_vjp(m, dev, case, composed=composed)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two launches agree to the bit"
        compare_vjp("vjp-B%d" % B, robot, "%s-%s%s" % (path, mode, "-subset" if names else ""), got, case)


@pytest.mark.parametrize("robot", HOST_ROBOTS)
def test_torques_vjp_against_fp64(cpu_library, robot):
    check_torques_vjp(robot, "cpu")


def test_torques_vjp_radii_planes_and_subset(cpu_library):
    check_torques_vjp(PANDA, "cpu", cases=(("contact", Z, 0.03), ("both", TILTED, 0.0), ("contact", Z, 0.0), ("both", TILTED, 0.03)))
    check_torques_vjp(PANDA, "cpu", cases=(("both", Z, None), ("contact", TILTED, None)), names=PANDA_SUBSET)
    # the host build's general walk on the arm (DRM_LINKS_COMPOSED) against the same truth
    check_torques_vjp(PANDA, "cpu", composed=True, path="host-composed")


@pytest.mark.gpu
@pytest.mark.parametrize("B,own,composed", [(64, None, False), (64, "off", False), (128, None, False), (128, "off", False), (65, None, False),
                                            (128, None, True)], ids=lambda v: str(v))
def test_gpu_torques_vjp_panda(B, own, composed):
    path = "gpu-" + ("composed" if composed else "arm" if B % 64 == 0 else "arm+tail") + ("" if own is None else "-own-" + own)
    check_torques_vjp(PANDA, GPU, B=B, own=own, composed=composed, path=path)
    if B == 65:
        check_torques_vjp(PANDA, GPU, B=65, cases=(("both", Z, None),), names=PANDA_SUBSET, path="gpu-composed")
        # B = 1: the first row of the case alone
        case = torque_case(PANDA, 65, "both", Z, radius_of(PANDA, None), None, 11)
        row = slice(int(np.argmax(case["keep"])), int(np.argmax(case["keep"])) + 1)
        compare_vjp("vjp-B1", PANDA, "gpu-composed", call_vjp(model(PANDA, GPU), GPU, case, rows=row), case, rows=row)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", HOST_ROBOTS[1:])
def test_gpu_torques_vjp_other_robots(robot):
    check_torques_vjp(robot, GPU, path="gpu-arm+tail" if robot in tcr.ARMS else "gpu-composed")


# ------------------------------------------------------------------------------------------------------------------- 2  rollout

ROLLOUT_T = 4
ROLLOUT_SEEDS = {"panda_no_gripper": 101, "allegro_left": 101}
ROLLOUT_ROBOTS = ("panda_no_gripper", "allegro_left")
ROLLOUT_FLAGS = ((1, 0), (0, 0))


def rollout64(robot, names, q0, qd0, tau, normal, offset, par, springs, integ, g, d):
    """The fp64 step-by-step contact rollout -> (qs, qds, tau_c, pattern, refs), each with a leading T"""
    orc = oracle(robot)
    x, v = np.asarray(q0, np.float64), np.asarray(qd0, np.float64)
    qs, qds, tcs, pats, refs = [], [], [], [], []
    for t in range(tau.shape[0]):
        e = reference_m(robot, names, x, v, normal, offset, par, par["radius"], springs, np.float64)
        a = orc.forward_dynamics(x, v, np.asarray(tau[t], np.float64) + e["tau"], bool(g), bool(d), np.float64)
        if integ == "euler":
            x, v = x + DT * v, v + DT * a
        else:
            v = v + DT * a
            x = x + DT * v
        qs.append(x); qds.append(v); tcs.append(e["tau"]); pats.append(e["pattern"]); refs.append(e)
    return np.stack(qs), np.stack(qds), np.stack(tcs), np.stack(pats, 1), refs


@functools.lru_cache(maxsize=None)
def rollout_case_of(robot, B, integ, g, d, sel):
    """inputs of one rollout case of B rows, and truth, yardstick and kinematic share over the rows `sel`"""
    m = model(robot)
    n, T = m._n_dofs, ROLLOUT_T
    q0, qd0, tau = rollout_case(robot, B, T, ROLLOUT_SEEDS[robot], push=True)
    rng = np.random.default_rng(23)
    Wq, Wv = (rng.uniform(-1.0, 1.0, size=(T, B, n)).astype(np.float32) for _ in range(2))
    names, par, springs = names_of(robot, None), soft(robot), springs_par(robot)
    offset = median_offset(robot, q0, Z)
    fixed = (Z, offset, par, springs, integ, g, d)
    rows = np.asarray(sel)
    S = len(rows)
    wq, wv = Wq[:, rows].astype(np.float64), Wv[:, rows].astype(np.float64)
    qs, qds, tcs, base_pattern, _ = rollout64(robot, names, q0[rows], qd0[rows], tau[:, rows], *fixed)

    def per_row(zz):
        tt = np.ascontiguousarray(zz[:, 2 * n:].reshape(-1, T, n).transpose(1, 0, 2))
        a, b, _, pat, _ = rollout64(robot, names, zz[:, :n], zz[:, n:2 * n], tt, *fixed)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        tile = lambda W: np.tile(W, (1, len(zz) // S, 1))
        return (tile(wq) * a).sum((0, 2)) + (tile(wv) * b).sum((0, 2)), pat
    z = np.concatenate([q0[rows], qd0[rows], tau[:, rows].transpose(1, 0, 2).reshape(S, T * n)], 1).astype(np.float64)
    grad, exclude = differences(per_row, z, base_pattern)
    truth = (grad[:, :n], grad[:, n:2 * n], grad[:, 2 * n:].reshape(S, T, n).transpose(1, 0, 2))
    # the yardstick: test_rollout_edges.yardstick_gradients' sweep at the fp64 trajectory, the contact VJP added per step
    xq = np.concatenate([q0[rows][None].astype(np.float64), qs[:-1]])
    xv = np.concatenate([qd0[rows][None].astype(np.float64), qds[:-1]])
    total = tau[:, rows].astype(np.float64) + tcs
    p = build_problem(oracle(robot), (xq.reshape(T * S, n), xv.reshape(T * S, n), total.reshape(T * S, n)), bool(g), bool(d))
    Jq, Jv, Mi = (y.reshape(T, S, n, n) for y in p["yard"])
    f32 = np.float32
    h = f32(DT)
    Q, V, gtau = np.zeros((S, n), f32), np.zeros((S, n), f32), np.empty((T, S, n), f32)
    vjp = lambda A, J: np.einsum("bi,bij->bj", A, J)
    for t in range(T - 1, -1, -1):
        Q = Q + Wq[t][rows]
        V = V + Wv[t][rows]
        if integ == "euler":
            A = h * V
            V = V + h * Q
        else:
            V = V + h * Q
            A = h * V
        gtau[t] = vjp(A, Mi[t])
        cq, cqd = yard_vjp(robot, names, xq[t].astype(f32), xv[t].astype(f32), gtau[t], Z, offset, par, par["radius"], springs, f32)
        Q = Q + vjp(A, Jq[t]) + cq
        V = V + vjp(A, Jv[t]) + cqd
    assert Q.dtype == f32 and V.dtype == f32
    kin = kinematic_gradients(wq, wv, DT)
    # activity over all B rows and steps of the base trajectory
    _, _, _, _, refs = rollout64(robot, names, q0, qd0, tau, *fixed)
    active = np.concatenate([r["depth"] > 0 for r in refs])
    sat = np.concatenate([r["saturated"] for r in refs])
    tag = (robot, B, integ, g, d)
    assert active.mean() >= 0.25 and sat.any() and (active & ~sat).any(), tag
    assert np.concatenate([r["lim_active"] for r in refs]).mean() >= 0.05, tag
    assert exclude.mean() <= 0.10, (tag, exclude.mean())
    print("CONTACTGRAD %-14s %-22s %-22s excluded %d of %d rows" % ("rollout-rows", robot, "B%d-%s-g%dd%d" % (B, integ[:4], g, d),
                                                                    int(exclude.sum()), S))
    return dict(q0=q0, qd0=qd0, tau=tau, Wq=Wq, Wv=Wv, names=names, contact=plane_of(Z, offset, par), springs=springs, rows=rows,
                truth=truth, yard=(Q, V, gtau), kin=kin, keep=~exclude)


def rollout_path_gradients(m, dev, case, integ, g, d, composed=False, differentiable=True):
    leaves = [t.requires_grad_(True) for t in to(dev, case["q0"], case["qd0"], case["tau"])]
    out = m.compute_contact_rollout(*leaves, DT, case["contact"], link_names=case["names"], joint_limits=JointLimitSprings(*case["springs"]),
                                    integrator=integ, include_gravity=bool(g), use_damping=bool(d), differentiable=True, _composed=composed)
    assert out.q.requires_grad and out.qd.requires_grad and out.qdd is None
    wq, wv = to(dev, case["Wq"], case["Wv"])
    loss = (wq * out.q).sum() + (wv * out.qd).sum()
    return [x.detach().cpu().numpy() for x in torch.autograd.grad(loss, leaves)], out


def check_rollout_gradients(robot, dev, B, sel, path, own=None):
    m = model(robot, dev, own)
    worst = 0.0
    for integ in INTEGRATORS:
        for g, d in ROLLOUT_FLAGS:
            case = rollout_case_of(robot, B, integ, g, d, tuple(sel))
            got, _ = rollout_path_gradients(m, dev, case, integ, g, d)
            rows, keep, bad = case["rows"], case["keep"], []
            for k, name in enumerate(ARRAYS):
                pick = (lambda x: x[keep]) if k < 2 else (lambda x: x[:, keep])
                g64, yard, kin = pick(case["truth"][k]), pick(case["yard"][k]), pick(case["kin"][k])
                mine = pick(got[k][rows] if k < 2 else got[k][:, rows])
                scale = np.abs(g64 - kin).max()
                assert scale > 0 and np.isfinite(got[k]).all()
                e = float(np.abs(mine - g64).max() / scale)
                ey = max(float(np.abs(yard - g64).max() / scale), float(FLOOR * np.abs(g64).max() / scale))
                print("CONTACTGRAD %-14s %-22s %-22s %-8s %.3e  %.3e  %.2f" % ("rollout", robot, "%s-B%d-%s-g%dd%d" % (path, B, integ[:4], g, d),
                                                                               name, e, ey, e / ey))
                worst = max(worst, e / ey)
                if not e <= MARGIN * ey:
                    bad.append((integ, g, d, name, e, ey))
            assert not bad, bad
    return worst


@pytest.mark.parametrize("robot", ROLLOUT_ROBOTS)
def test_rollout_gradients_against_fp64(cpu_library, robot):
    check_rollout_gradients(robot, "cpu", 4, range(4), "host")


@pytest.mark.gpu
@pytest.mark.parametrize("robot,B", [(r, B) for r in ROLLOUT_ROBOTS for B in (64, 65)], ids=lambda v: str(v))
def test_gpu_rollout_gradients_against_fp64(robot, B):
    """B = 64: the fused forward's states (Panda); B = 65: rows 0 - 8 of the tile and the composed tail row 64"""
    sel = list(range(10)) if B == 64 else list(range(9)) + [64]
    check_rollout_gradients(robot, GPU, B, sel, "gpu-arm" if robot == PANDA else "gpu-composed")


# ------------------------------------------------------------------------------------------------------------------- 3  bits


def check_bits(robot, dev, B, composed=False):
    m = model(robot, dev)
    case = torque_case(robot, B, "both", Z, radius_of(robot, None), None, 11)
    jl = JointLimitSprings(*case["springs"])
    kw = dict(link_names=case["names"], joint_limits=jl, _composed=composed)
    q, qd, lam = to(dev, case["q"], case["qd"], case["lam"])
    plain = m.compute_contact_torques(q, qd, case["contact"], **kw)
    ql, qdl = q.clone().requires_grad_(True), qd.clone().requires_grad_(True)
    diff = m.compute_contact_torques(ql, qdl, case["contact"], differentiable=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, diff)), "differentiable=True changes no bit of the forward"
    assert diff.tau.requires_grad and not diff.force.requires_grad and not diff.moment.requires_grad
    gq, gqd = torch.autograd.grad(diff.tau, (ql, qdl), lam)
    vq, vqd = m.compute_contact_torques_vjp(q, qd, lam, case["contact"], **kw)
    assert torch.equal(gq, vq) and torch.equal(gqd, vqd), "autograd.grad is the VJP call"
    # one input alone: the other output is NULL in the C call and changes no bit
    diff = m.compute_contact_torques(ql, qd, case["contact"], differentiable=True, **kw)
    assert torch.equal(torch.autograd.grad(diff.tau, ql, lam)[0], vq)
    diff = m.compute_contact_torques(q, qdl, case["contact"], differentiable=True, **kw)
    assert torch.equal(torch.autograd.grad(diff.tau, qdl, lam)[0], vqd)
    # a plane far below the robot, no springs: zero contact gradients
    far = plane_of(Z, -100.0, soft(robot))
    zq, zqd = m.compute_contact_torques_vjp(q, qd, lam, far, link_names=case["names"], _composed=composed)
    assert not zq.any() and not zqd.any()
    # ... and the rollout's gradients are the plain rollout's, to the bit — wherever the two FORWARD calls take the same path and so
    # return the same states (test_contact_rollout.check_zero_contact): full tiles, or a batch that both compose on every row.  (At
    # B n % 4 != 0 the contact rollout composes every row while the plain one runs its fused kernel on the full tile.)
    T = 3
    if dev != "cpu" and (B % 64 or composed):
        B, composed = 63, True
    q0, qd0, tau = rollout_case(robot, B, T, seed=50, push=False)
    rng = np.random.default_rng(5)
    wq, wv = to(dev, *(rng.uniform(-1.0, 1.0, size=tau.shape).astype(np.float32) for _ in range(2)))
    for integ in INTEGRATORS:
        grads = []
        for contact in (far, None):
            leaves = [t.requires_grad_(True) for t in to(dev, q0, qd0, tau)]
            if contact is None:
                out = m.compute_forward_dynamics_rollout(*leaves, DT, integrator=integ)
            else:
                out = m.compute_contact_rollout(*leaves, DT, contact, integrator=integ, differentiable=True, _composed=composed)
                off = m.compute_contact_rollout(*[t.detach() for t in leaves], DT, contact, integrator=integ, _composed=composed)
                assert torch.equal(out.q, off.q) and torch.equal(out.qd, off.qd), "differentiable=True changes no bit of the rollout"
            grads.append(torch.autograd.grad((wq * out[0]).sum() + (wv * out[1]).sum(), leaves))
        for name, a, b in zip(ARRAYS, *grads):
            assert torch.equal(a, b), (robot, integ, name, "zero contact: the plain rollout's gradients")
    # the rollout with contact: differentiable=True changes no bit, two backward passes agree
    rc = rollout_case_of(robot, 4, "semi_implicit_euler", 1, 0, tuple(range(4))) if robot in ROLLOUT_ROBOTS and dev == "cpu" else None
    if rc is not None:
        a, out = rollout_path_gradients(m, dev, rc, "semi_implicit_euler", 1, 0)
        b, _ = rollout_path_gradients(m, dev, rc, "semi_implicit_euler", 1, 0)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        off = m.compute_contact_rollout(*to(dev, rc["q0"], rc["qd0"], rc["tau"]), DT, rc["contact"], link_names=rc["names"],
                                        joint_limits=JointLimitSprings(*rc["springs"]))
        assert torch.equal(out.q.detach(), off.q) and torch.equal(out.qd.detach(), off.qd)


@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left"))
def test_bits(cpu_library, robot):
    check_bits(robot, "cpu", 65)
    check_bits(robot, "cpu", 65, composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("robot,B,composed", [(PANDA, 128, False), (PANDA, 65, False), (PANDA, 128, True), ("allegro_left", 65, False)],
                         ids=lambda v: str(v))
def test_gpu_bits(robot, B, composed):
    check_bits(robot, GPU, B, composed)


# ------------------------------------------------------------------------------------------------------------------- 4  edges


def check_non_finite_rows(robot, dev, B=128):
    m = model(robot, dev)
    case = torque_case(robot, B, "both", Z, radius_of(robot, None), None, 12)
    for composed in (False, True):
        clean = call_vjp(m, dev, case, composed=composed)
        assert all(np.isfinite(x).all() for x in clean)
        for key, row, value in (("q", 5, np.nan), ("q", 70, 4e5), ("qd", 9, np.inf), ("lam", 127, np.nan), ("lam", 64, -np.inf)):
            bad = dict(case)
            bad[key] = case[key].copy()
            bad[key][row, 2] = value
            got = call_vjp_unchecked(m, dev, bad, composed)
            others = np.arange(B) != row
            for a, b in zip(got, clean):
                assert np.array_equal(a[others], b[others]), (robot, composed, key, row)
                assert np.isnan(a[row]).all(), (robot, composed, key, row)


def call_vjp_unchecked(m, dev, case, composed):
    jl = JointLimitSprings(*case["springs"])
    out = m.compute_contact_torques_vjp(*to(dev, case["q"], case["qd"], case["lam"]), case["contact"], link_names=case["names"],
                                        joint_limits=jl, _composed=composed)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left"))
def test_non_finite_rows_are_isolated(cpu_library, robot):
    check_non_finite_rows(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left"))
def test_gpu_non_finite_rows_are_isolated(robot):
    check_non_finite_rows(robot, GPU)


def c_vjp(robot, dev, case, misaligned, want=(True, True), flags=0):
    """drm_contact_torques_vjp straight through the C ABI: every tensor aligned or every tensor 4 bytes off a 16-byte boundary, the
    scratch of exactly the queried size followed by GUARD sentinel words -> [grad_q, grad_qd] (None where not asked for)"""
    m = model(robot, dev)
    device = torch.device(dev)
    lib = backend.library_for(device)
    lw, TL, _, _ = m._links_plan(case["names"])
    n = m._n_dofs
    walk = backend._walk_struct(lw.program, m._ops_f(lw).detach(), lw.ops_i, n)
    B = case["q"].shape[0]
    ins = [place(t, dev, misaligned) for t in to("cpu", case["q"], case["qd"], case["lam"])]
    outs = [place(torch.full((B, n), FILL), dev, misaligned) if w else None for w in want]
    for _, v in ins + [o for o in outs if o is not None]:
        assert (v.data_ptr() % 16 != 0) == misaligned
    need = int(lib.drm_contact_torques_vjp_scratch_floats(ctypes.byref(walk), B))
    need_aligned = int(lib.drm_contact_torques_vjp_scratch_floats_aligned(ctypes.byref(walk), B))
    assert 0 <= need_aligned <= need
    size = need if misaligned else need_aligned
    scratch = torch.full((size + GUARD,), SENTINEL, device=dev) if device.type == "cuda" else None
    if scratch is None:
        assert need == 0
    else:
        assert size > 0
    c = case["contact"]
    pl = backend.DrmContactPlane((ctypes.c_float * 3)(*c.normal), c.offset, c.stiffness, c.damping, c.friction, c.friction_slope)
    sp = backend.DrmJointSprings(*case["springs"])
    lo, hi = m._joint_bounds()
    rad = torch.full((TL,), float(c.radius), device=dev)
    ptr = lambda o: o[1].data_ptr() if o is not None else None
    rc = lib.drm_contact_torques_vjp(ctypes.byref(walk), ins[0][1].data_ptr(), ins[1][1].data_ptr(), ins[2][1].data_ptr(), B, TL,
                                     ctypes.byref(pl), rad.data_ptr(), ctypes.byref(sp), lo.data_ptr(), hi.data_ptr(), flags, ptr(outs[0]),
                                     ptr(outs[1]), scratch.data_ptr() if scratch is not None else None, backend._stream(device))
    assert rc == 0, lib.drm_last_error()
    if scratch is not None:
        torch.cuda.synchronize()
        assert bool((scratch[size:] == SENTINEL).all()), (robot, B, misaligned, "the call wrote past its scratch")
    for (flat, view), src in zip(ins, (case["q"], case["qd"], case["lam"])):
        assert np.array_equal(view.cpu().numpy(), src)
    for o in outs:
        if o is not None:
            assert float(o[0][0 if misaligned else -1]) == FILL
    return [None if o is None else o[1].cpu().numpy().copy() for o in outs]


def check_c_abi(robot, dev):
    m = model(robot, dev)
    n = m._n_dofs
    for B in (128, 65):
        case = torque_case(robot, B, "both", Z, radius_of(robot, None), None, 11 if B == 65 else 12)
        api = call_vjp(m, dev, case)
        aligned = c_vjp(robot, dev, case, False)
        mis = c_vjp(robot, dev, case, True)
        assert all(np.array_equal(a, b) for a, b in zip(aligned, api)), "the aligned C call is the binding's call"
        compare_vjp("misaligned-B%d" % B, robot, "host" if dev == "cpu" else "gpu-composed", mis, case)
        # grad_q NULL or grad_qd NULL changes no bit of the other
        for misaligned, full in ((False, aligned), (True, mis)):
            only_q = c_vjp(robot, dev, case, misaligned, want=(True, False))
            only_qd = c_vjp(robot, dev, case, misaligned, want=(False, True))
            assert only_q[1] is None and only_qd[0] is None
            assert np.array_equal(only_q[0], full[0]) and np.array_equal(only_qd[1], full[1]), (robot, B, misaligned)
    # every refusal returns an error with drm_last_error() set
    lib = backend.library_for(torch.device(dev))
    lw, TL, _, _ = m._links_plan(None)
    walk = backend._walk_struct(lw.program, m._ops_f(lw).detach(), lw.ops_i, n)
    q, qd, lam = to(dev, case["q"][:3], case["qd"][:3], case["lam"][:3])
    out = torch.zeros(3, n, device=dev)
    lo, hi = m._joint_bounds()
    good = backend.DrmContactPlane((ctypes.c_float * 3)(0.0, 0.0, 1.0), 0.0, 1.0, 1.0, 0.0, 0.0)
    sp = backend.DrmJointSprings(1.0, 1.0)
    scratch = torch.zeros(max(1, int(lib.drm_contact_torques_vjp_scratch_floats(ctypes.byref(walk), 3))), device=dev)
    stream = backend._stream(torch.device(dev))

    def call(qp=q.data_ptr(), qdp=qd.data_ptr(), lp=lam.data_ptr(), B=3, T=TL, plane=good, springs=None, lower=None, upper=None,
             gq=out.data_ptr(), gqd=None):
        return lib.drm_contact_torques_vjp(ctypes.byref(walk), qp, qdp, lp, B, T, ctypes.byref(plane) if plane is not None else None, None,
                                           ctypes.byref(springs) if springs is not None else None, lower, upper, 0, gq, gqd,
                                           scratch.data_ptr(), stream)
    assert call() == 0, lib.drm_last_error()
    assert call(B=0) == 0
    assert call(plane=None, springs=sp, lower=lo.data_ptr(), upper=hi.data_ptr()) == 0, "the springs' share alone"
    refusals = [dict(qp=None), dict(qdp=None), dict(lp=None), dict(gq=None, gqd=None), dict(B=-1), dict(plane=None), dict(T=0),
                dict(T=TL + 100), dict(springs=sp), dict(springs=backend.DrmJointSprings(-1.0, 1.0), lower=lo.data_ptr(), upper=hi.data_ptr())]
    for normal, k in (((0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, 1.0), -1.0), ((0.0, float("nan"), 1.0), 1.0), ((0.0, 0.0, 1.0), float("inf"))):
        refusals.append(dict(plane=backend.DrmContactPlane((ctypes.c_float * 3)(*normal), 0.0, k, 1.0, 0.0, 0.0)))
    for kw in refusals:
        assert call(**kw) != 0 and lib.drm_last_error(), kw
    assert {"drm_contact_torques_vjp", "drm_contact_torques_vjp_scratch_floats", "drm_contact_torques_vjp_scratch_floats_aligned"} <= \
        set(backend.EXPORTS)
    assert lib.drm_abi_version() == 15


@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left"))
def test_c_abi(cpu_library, robot):
    check_c_abi(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left"))
def test_gpu_c_abi(robot):
    check_c_abi(robot, GPU)


def check_python(dev):
    robot = PANDA
    m = model(robot, dev)
    n = m._n_dofs
    q, qd, tau = (torch.from_numpy(x).to(dev) for x in rollout_case(robot, 3, 2, seed=70, push=True))
    lam = torch.from_numpy(np.random.default_rng(1).standard_normal((3, n)).astype(np.float32)).to(dev)
    good = plane_of(Z, 0.4, soft(robot))
    jl = JointLimitSprings(*springs_par(robot))
    # without the keyword the old refusals still raise
    for k in range(3):
        leaves = [q.clone(), qd.clone(), tau.clone()]
        leaves[k].requires_grad_(True)
        with pytest.raises(ValueError, match="forward only"):
            m.compute_contact_rollout(*leaves, DT, good)
        if k < 2:
            with pytest.raises(ValueError, match="forward only"):
                m.compute_contact_torques(leaves[0], leaves[1], good)
    with pytest.raises(ValueError):
        m.compute_contact_torques_vjp(q, qd, lam, None)
    # a second backward raises
    ql = q.clone().requires_grad_(True)
    out = m.compute_contact_torques(ql, qd, good, joint_limits=jl, differentiable=True)
    (g,) = torch.autograd.grad(out.tau, ql, lam, create_graph=True)
    assert g.requires_grad
    with pytest.raises(NotImplementedError, match="first-order"):
        g.sum().backward()
    leaves = [t.clone().requires_grad_(True) for t in (q, qd, tau)]
    roll = m.compute_contact_rollout(*leaves, DT, good, joint_limits=jl, differentiable=True, return_acceleration=True)
    assert roll.q.requires_grad and roll.qd.requires_grad and not roll.qdd.requires_grad
    grads = torch.autograd.grad(roll.q.sum() + roll.qd.sum(), leaves, create_graph=True)
    with pytest.raises(NotImplementedError, match="first-order"):
        (grads[0].sum() + grads[2].sum()).backward()
    # springs alone (contact=None) differentiate too
    leaves = [t.clone().requires_grad_(True) for t in (q, qd, tau)]
    roll = m.compute_contact_rollout(*leaves, DT, None, joint_limits=jl, differentiable=True)
    assert all(torch.isfinite(x).all() for x in torch.autograd.grad(roll.q.sum() + roll.qd.sum(), leaves))
    # unbatched inputs give unbatched gradients
    g1 = m.compute_contact_torques_vjp(q[0], qd[0], lam[0], good, joint_limits=jl)
    gb = m.compute_contact_torques_vjp(q, qd, lam, good, joint_limits=jl)
    assert all(a.shape == (n,) and torch.equal(a, b[0]) for a, b in zip(g1, gb))
    q1 = q[0].clone().requires_grad_(True)
    t1 = m.compute_contact_torques(q1, qd[0], good, joint_limits=jl, differentiable=True)
    (a,) = torch.autograd.grad(t1.tau, q1, lam[0])
    assert a.shape == (n,) and torch.equal(a, gb[0][0])
    l1 = [q[0].clone().requires_grad_(True), qd[0].clone().requires_grad_(True), tau[:, 0].clone().requires_grad_(True)]
    r1 = m.compute_contact_rollout(*l1, DT, good, joint_limits=jl, differentiable=True)
    lb = [t.clone().requires_grad_(True) for t in (q, qd, tau)]
    rb = m.compute_contact_rollout(*lb, DT, good, joint_limits=jl, differentiable=True)
    ga, gbb = torch.autograd.grad(r1.q.sum(), l1), torch.autograd.grad(rb.q[:, 0].sum(), lb)
    assert ga[0].shape == (n,) and ga[2].shape == (2, n)
    assert torch.equal(ga[0], gbb[0][0]) and torch.equal(ga[1], gbb[1][0]) and torch.equal(ga[2], gbb[2][:, 0])


def check_learnable(dev):
    """a model with a learnable link: no parameter gradient, no error"""
    from test_rollout import learnable_mass_model
    m, param = learnable_mass_model(PANDA, "panda_link4", 1.2, dev)
    params = [param]
    n = m._n_dofs
    q, qd, tau = (torch.from_numpy(x).to(dev) for x in rollout_case(PANDA, 3, 2, seed=71, push=True))
    good = plane_of(Z, 0.4, soft(PANDA))
    leaves = [t.clone().requires_grad_(True) for t in (q, qd, tau)]
    roll = m.compute_contact_rollout(*leaves, DT, good, differentiable=True)
    loss = roll.q.sum() + roll.qd.sum()
    loss.backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in leaves)
    assert all(p.grad is None for p in params)
    out = m.compute_contact_torques(leaves[0], leaves[1], good, differentiable=True)
    got = torch.autograd.grad(out.tau.sum(), list(params) + leaves[:2], allow_unused=True)
    assert all(g is None for g in got[:len(params)]) and got[-1] is not None and got[-1].shape == (3, n)


def test_python_interface(cpu_library):
    check_python("cpu")
    check_learnable("cpu")


@pytest.mark.gpu
def test_gpu_python_interface():
    check_python(GPU)
    check_learnable(GPU)

"""Inverse kinematics (ABI 15, csrc/drm_ik.hip + csrc/drm_ik.hpp) held to fp64 at every iteration, option and edge.

test_inverse_kinematics.py pins the solve at its defaults; this file pins what a subtly wrong kernel could still get away with there.
Every check is one function of (device, _composed): it runs un-marked on the host build and under -m gpu on cuda:0, where the 7-DoF
arms run it twice (the fused kernel and the composed path).  The reference is numpy / torch fp64 on the fp64 oracle's FK + Jacobian,
except where a check is a bit-for-bit invariant of the kernel with itself (a row does not depend on its tile mates, on the sign or a
power-of-two scale of its target quaternion, on the strides or the dtype of the inputs).

  1  every iteration k = 1 .. 6 against the fp64 update from the kernel's own previous iterate (teacher-forced), all options
  2  rows that stop without converging, next to rows that stop at iteration 0 and rows that converge, in one tile and tile by tile
  3  the rotation error from 0 to pi, -target_quat, scaled target_quat, one update from a large rotation error
  4  clamps that bite: a third of the bounded DoFs on a bound, pushed outwards
  5  non-finite rows (q0, target_pos, target_quat) leave every other row's bits alone
  6  call forms (unbatched, float64, strided), a model with learnable links, targets in the middle of the chain

Bounds, relative to 1 + |q| per row: damping 0.01 and 0.1: check_close_rows(4 tol_of(robot)), the rule of test_inverse_kinematics.py;
damping 1.0: J J^T + I is well conditioned, the update is as accurate as FK and the Jacobian themselves: 2e-6 (helpers.TOL_POS /
TOL_JAC) on every row.  Reported errors: pos_err within 2e-6, rot_err within 1e-5 (the quaternion is good to TOL_QUAT = 2e-6 per
component and theta = 2 atan2(s, w) moves by at most twice the change of (s, w)).  Each check prints one "IKEDGE" line (check, robot,
path, worst value, bound) before it asserts; profiles/ik_edge_tests.txt holds them for the host build and the MI355X.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from helpers import ALL_ROBOTS, load_model
from oracle import Oracle
from test_forward_dynamics import tol_of
from test_inverse_kinematics import (FUSED, LINKS, bounds, check_close_rows, errors, fp64_step, learnable_iiwa, quat_mul,
                                     seeded_problem)

GPU = "cuda:0"
TIGHT = 2e-6                                                      # helpers.TOL_POS / TOL_JAC
TOL_POS_ERR, TOL_ROT_ERR = 2e-6, 1e-5
OPTION_SETS = ((0.01, 1.0, 0.1), (0.1, 0.5, 0.5), (1.0, 1.0, 0.3))      # (damping, step_size, noise of q0)
# (robot, link, _composed) of the GPU runs: the fused arms on both paths, then robots that only have the composed path
ARM_PATHS = [(r, l, c) for r, l in FUSED for c in (False, True)]
GPU_PATHS = ARM_PATHS + [(r, LINKS[r], False) for r in ("fetch", "jaco", "allegro_left", "iiwa7_allegro", "panda", "trifinger_edu",
                                                        "2link_robot")]
PANDA = ("panda_no_gripper", "panda_virtual_ee_link")


@functools.lru_cache(maxsize=None)
def model(robot, dev="cpu"):
    return load_model(robot, dev)


def path_name(robot, dev, composed):
    if dev == "cpu":
        return "host"
    return "gpu-fused" if (robot in [r for r, _ in FUSED] and not composed) else "gpu-composed"


def report(check, robot, path, worst, bound):
    print("IKEDGE %-22s %-28s %-12s worst %.3e bound %.3e" % (check, robot, path, worst, bound))


def run(m, link, q0, tp, tq, dev="cpu", composed=False, **kw):
    """compute_inverse_kinematics on `dev`, every field of the result back on the CPU"""
    mv = lambda t: None if t is None else t.to(dev)
    r = m.compute_inverse_kinematics(mv(q0), link, mv(tp), mv(tq), _composed=composed, **kw)
    return dataclasses.replace(r, **{f.name: (None if getattr(r, f.name) is None else getattr(r, f.name).cpu())
                                     for f in dataclasses.fields(r)})


def rows_equal(a, b, ia=slice(None), ib=slice(None)):
    """q, the errors and the iteration counts of rows ia of a = rows ib of b, bit for bit"""
    assert torch.equal(a.q[ia], b.q[ib])
    assert torch.equal(a.iterations[ia], b.iterations[ib])
    assert torch.equal(a.pos_err[ia], b.pos_err[ib])
    assert (a.rot_err is None) == (b.rot_err is None)
    if a.rot_err is not None:
        assert torch.equal(a.rot_err[ia], b.rot_err[ib])


def row_rel(a, ref):
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    return (np.abs(a - ref) / (1.0 + np.abs(ref))).max(axis=-1)


def step_bound(robot, damping):
    return TIGHT if damping >= 1.0 else 4 * tol_of(robot)


def check_step(got, want, robot, damping):
    """one update against fp64 by the tier of `damping`; -> the worst row"""
    r = row_rel(got, want)
    if r.size == 0:
        return 0.0
    if damping >= 1.0:
        assert r.max() <= TIGHT, r.max()
    else:
        check_close_rows(got, want, 4 * tol_of(robot))
    return float(r.max())


def teacher_forced(m, robot, link, dev, composed, q0, tp, tq, K, damping=0.01, step=1.0, limits=True, spec=None):
    """Section 1.  r_k = the solve with max_iterations = k and tolerances 0, k = 0 .. K.  A row of r_k with iterations == k: its q
    against the fp64 update of ITS OWN q in r_{k-1} (rounding does not compound, no row is left out); a row that stopped earlier
    (tolerance 0 still stops a row whose error is exactly 0.0f): bit-equal to r_{k-1}.  With the limits on, a DoF whose fp64 update
    lies beyond its bound by more than the tier's bound must equal the float32 bound bit for bit; every other DoF is held to the tier.
    -> (worst row against fp64, number of DoFs held to a bound bit for bit, r_K)"""
    cpu = model(robot)
    lower, upper = bounds(cpu) if limits else (None, None)
    kw = dict(tol_pos=0.0, tol_rot=0.0, damping=damping, step_size=step, respect_joint_limits=limits)
    prev = run(m, link, q0, tp, tq, dev, composed, max_iterations=0, **kw)
    assert torch.equal(prev.q, q0) and (prev.iterations == 0).all()
    worst, held = 0.0, 0
    for k in range(1, K + 1):
        r = run(m, link, q0, tp, tq, dev, composed, max_iterations=k, **kw)
        assert (r.iterations <= k).all() and (r.iterations >= 0).all()
        took = r.iterations == k
        rows_equal(r, prev, ~took, ~took)
        want, u = fp64_step(cpu, link, prev.q[took], tp[took], None if tq is None else tq[took], damping, lower, upper, step, spec,
                            unclamped=True)
        got = r.q[took].numpy()
        if limits:
            lo, hi = lower.numpy(), upper.numpy()
            margin = step_bound(robot, damping) * (1.0 + np.abs(u))
            over, under = u > hi.astype(np.float64) + margin, u < lo.astype(np.float64) - margin
            assert (got[over] == np.broadcast_to(hi, got.shape)[over]).all()
            assert (got[under] == np.broadcast_to(lo, got.shape)[under]).all()
            assert ((r.q >= lower) & (r.q <= upper)).all()
            held += int(over.sum() + under.sum())
            got = np.where(over | under, want, got.astype(np.float64))
        worst = max(worst, check_step(got, want, robot, damping))
        prev = r
    return worst, held, prev


def check_every_iteration(robot, link, dev, composed, B, K=6, path=None):
    m, cpu = model(robot, dev), model(robot)
    worst = {}
    try:
        for pos_only in (False, True):
            for limits in (True, False):
                for damping, step, noise in OPTION_SETS:
                    q0, tp, tq, _ = seeded_problem(cpu, link, B, seed=31, noise=noise, pos_only=pos_only)
                    w, _, last = teacher_forced(m, robot, link, dev, composed, q0, tp, tq, K, damping, step, limits)
                    assert (last.iterations == K).any()         # (the problem does not die out before K)
                    worst[damping] = max(worst.get(damping, 0.0), w)
    finally:
        for damping, w in sorted(worst.items()):
            report("1-step-damping-%g" % damping, robot, path or path_name(robot, dev, composed), w, step_bound(robot, damping))


# ------------------------------------------------------------------------------------------------------------------- section 2


def mixed_problem(cpu, link, B, seed=41):
    """seeded_problem with odd rows unreachable (kind 1), every 8th row on target at q0 (kind 2), the rest reachable (kind 0)"""
    q0, tp, tq, _ = seeded_problem(cpu, link, B, seed=seed)
    idx = torch.arange(B)
    kind = torch.zeros(B, dtype=torch.long)
    kind[idx % 2 == 1] = 1
    kind[idx % 8 == 0] = 2
    tp[kind == 1] = tp[kind == 1] * 3 + 2
    with torch.no_grad():
        p, r = cpu.compute_forward_kinematics(q0[kind == 2], link)
    tp[kind == 2] = p
    tq[kind == 2] = r
    return q0, tp, tq, kind


def reported_errors(cpu, link, res, tp, tq):
    """(|pos_err - fp64|, |rot_err - fp64|) maxima over EVERY row, the fp64 errors from the oracle's FK of the returned q"""
    p, c, _, _ = Oracle(cpu._spec).fk_jacobian(res.q.double().numpy(), cpu._name_to_idx_map[link], np.float64)
    t64 = None if tq is None else tq.double() / tq.double().norm(dim=-1, keepdim=True)
    _, pe, re = errors(torch.from_numpy(p), torch.from_numpy(c), tp.double(), t64)
    dp = float((res.pos_err.double() - pe).abs().max())
    dr = 0.0 if tq is None else float((res.rot_err.double() - re).abs().max())
    return dp, dr


def check_mixed_tiles(robot, link, dev, composed, B=512, K=12, homogeneous=True):
    m, cpu = model(robot, dev), model(robot)
    q0, tp, tq, kind = mixed_problem(cpu, link, B)
    lower, upper = bounds(cpu)
    a = run(m, link, q0, tp, tq, dev, composed, max_iterations=K)
    dp, dr = reported_errors(cpu, link, a, tp, tq)
    path = path_name(robot, dev, composed)
    report("2-pos_err-K%d" % K, robot, path, dp, TOL_POS_ERR)
    report("2-rot_err-K%d" % K, robot, path, dr, TOL_ROT_ERR)
    un, on, re = kind == 1, kind == 2, kind == 0
    assert not a.converged[un].any() and (a.iterations[un] == K).all()
    assert torch.isfinite(a.q).all() and ((a.q >= lower) & (a.q <= upper)).all()
    assert (a.iterations[on] == 0).all() and torch.equal(a.q[on], q0[on]) and a.converged[on].all()
    assert a.converged[re].any() and (a.iterations[re] >= 1).all()          # (the tiles do mix all three kinds)
    assert dp <= TOL_POS_ERR and dr <= TOL_ROT_ERR, (dp, dr)
    # a row does not depend on its tile mates: sorted by kind (whole tiles of one kind), and each kind alone
    perm = torch.argsort(kind, stable=True)
    b = run(m, link, q0[perm], tp[perm], tq[perm], dev, composed, max_iterations=K)
    rows_equal(a, b, perm)
    if homogeneous:
        for sel in (un, on, re):
            assert int(sel.sum()) % 64 == 0
            h = run(m, link, q0[sel], tp[sel], tq[sel], dev, composed, max_iterations=K)
            rows_equal(a, h, sel)


# ------------------------------------------------------------------------------------------------------------------- section 3

THETAS = (0.0, 1e-7, 1e-5, 1e-3, 0.5, math.pi / 2, math.pi - 1e-3, math.pi - 1e-5, math.pi)


def rotated_targets(cpu, link, q0, thetas, seed):
    """target_pos = the oracle's fp64 position of q0, target_quat = d (x) c64 rounded: c64 the oracle's quaternion of q0, d a rotation
    by thetas[b % len] about a seeded random axis"""
    p, c, _, _ = Oracle(cpu._spec).fk_jacobian(q0.double().numpy(), cpu._name_to_idx_map[link], np.float64)
    B = q0.shape[0]
    g = torch.Generator().manual_seed(seed)
    ax = torch.randn(B, 3, generator=g, dtype=torch.float64)
    ax = ax / ax.norm(dim=-1, keepdim=True)
    th = torch.tensor(thetas, dtype=torch.float64)[torch.arange(B) % len(thetas)]
    d = torch.cat([ax * torch.sin(th / 2)[:, None], torch.cos(th / 2)[:, None]], -1)
    tq = quat_mul(d, torch.from_numpy(c))
    return torch.from_numpy(p).float(), tq.float(), th, torch.from_numpy(p), torch.from_numpy(c)


def check_error_measure(robot, link, dev, composed, B=576):
    m, cpu = model(robot, dev), model(robot)
    q0, _, _, _ = seeded_problem(cpu, link, B, seed=42)
    tp, tq, th, p64, c64 = rotated_targets(cpu, link, q0, THETAS, seed=43)
    _, pe, re = errors(p64, c64, tp.double(), tq.double() / tq.double().norm(dim=-1, keepdim=True))
    assert float((re - th).abs().max()) <= 1e-6           # (the rounded inputs still carry theta)
    r = run(m, link, q0, tp, tq, dev, composed, max_iterations=0)
    dp, dr = float((r.pos_err.double() - pe).abs().max()), float((r.rot_err.double() - re).abs().max())
    path = path_name(robot, dev, composed)
    report("3-rot_err-0..pi", robot, path, dr, TOL_ROT_ERR)
    assert (r.iterations == 0).all() and torch.equal(r.q, q0)
    assert dp <= TOL_POS_ERR and dr <= TOL_ROT_ERR, (dp, dr)
    # the sign and a power-of-two scale of target_quat change no bit (4 tq and tq / 4 normalise exactly)
    plain = run(m, link, q0, tp, tq, dev, composed, max_iterations=3)
    assert (plain.iterations > 0).any() and (plain.iterations == 0).any()
    for scale in (-1.0, 4.0, 0.25, -4.0):
        rows_equal(plain, run(m, link, q0, tp, tq * scale, dev, composed, max_iterations=3))


def check_large_rotation_step(robot, link, dev, composed, B=192):
    """One update from a rotation error of 1.0, 2.5 and 3.0 rad (no row within 0.14 rad of pi, where the sign of the axis is
    ill-defined, so no row is excluded), damping 1.0 (2e-6) and 0.1 (4 tol_of), limits on and off.  damping 0.01 is left out: the
    error of the solve scales with |e|, and from 2.5 rad the host build itself is 5.2e-4 from fp64 on the Panda, above 4 tol_of.
    A target quaternion scaled by 3 (normalisation rounds) stays within check_close_rows of the plain one."""
    m, cpu = model(robot, dev), model(robot)
    q0, _, _, _ = seeded_problem(cpu, link, B, seed=44)
    tp, tq, _, _, _ = rotated_targets(cpu, link, q0, (1.0, 2.5, 3.0), seed=45)
    worst = {}
    try:
        for damping in (1.0, 0.1):
            for limits in (True, False):
                w, _, r = teacher_forced(m, robot, link, dev, composed, q0, tp, tq, 1, damping, 1.0, limits)
                assert (r.iterations == 1).all()
                worst[damping] = max(worst.get(damping, 0.0), w)
                if damping == 0.1:
                    r3 = run(m, link, q0, tp, tq * 3.0, dev, composed, max_iterations=1, tol_pos=0.0, tol_rot=0.0, damping=damping,
                             respect_joint_limits=limits)
                    check_close_rows(r3.q, r.q, 4 * tol_of(robot))
    finally:
        for damping, w in sorted(worst.items()):
            report("3-large-angle-damp-%g" % damping, robot, path_name(robot, dev, composed), w, step_bound(robot, damping))


# ------------------------------------------------------------------------------------------------------------------- section 4


def clamp_problem(cpu, link, B, seed=46):
    """q0 with a seeded third of its bounded DoFs exactly on a bound; the target is FK (limits ignored) of a configuration whose
    DoFs of that third lie 0.3 rad beyond their bound (the others at the q* of seeded_problem)"""
    q0, _, _, qs = seeded_problem(cpu, link, B, seed=seed)
    lower, upper = bounds(cpu)
    bounded = torch.isfinite(lower) & torch.isfinite(upper)
    g = torch.Generator().manual_seed(seed + 1000)
    on = (torch.rand(q0.shape, generator=g) < 1.0 / 3.0) & bounded
    up = torch.rand(q0.shape, generator=g) < 0.5
    edge = torch.where(up, upper.expand_as(q0), lower.expand_as(q0))
    q0 = torch.where(on, edge, q0)
    qt = torch.where(on, edge + torch.where(up, torch.tensor(0.3), torch.tensor(-0.3)), qs)
    with torch.no_grad():
        tp, tq = cpu.compute_forward_kinematics(qt, link)
    return q0, tp.clone(), tq.clone(), bounded


def check_clamps(robot, link, dev, composed, B=256):
    m, cpu = model(robot, dev), model(robot)
    q0, tp, tq, bounded = clamp_problem(cpu, link, B)
    lower, upper = bounds(cpu)
    lo, hi = lower.double().numpy(), upper.double().numpy()
    path = path_name(robot, dev, composed)
    _, _, lin, ang = Oracle(cpu._spec).fk_jacobian(q0.double().numpy(), cpu._name_to_idx_map[link], np.float64)
    depends = (np.abs(lin).max(axis=(0, 1)) + np.abs(ang).max(axis=(0, 1))) > 0
    chain = depends & bounded.numpy()
    worst = {}
    try:
        for damping in (0.1, 1.0):
            # the inputs make the fp64 reference clamp (by more than 1e-3 rad) at least 20 % of the bounded DoFs of the link's chain
            _, u = fp64_step(cpu, link, q0, tp, tq, damping, lower, upper, unclamped=True)
            beyond = ((u > hi + 1e-3) | (u < lo - 1e-3))[:, chain]
            assert beyond.mean() >= 0.2, beyond.mean()
            for K in (1, 4):
                w, held, _ = teacher_forced(m, robot, link, dev, composed, q0, tp, tq, K, damping, 1.0, True)
                assert held >= 0.2 * B * int(chain.sum()) - B           # (the bit-for-bit branch did the work)
                worst[damping] = max(worst.get(damping, 0.0), w)
            # limits off: the same rows leave the bounds (wherever fp64 is beyond a bound by more than five times the tier's bound)
            w, _, free = teacher_forced(m, robot, link, dev, composed, q0, tp, tq, 1, damping, 1.0, False)
            worst[damping] = max(worst.get(damping, 0.0), w)
            margin = 5 * step_bound(robot, damping) * (1.0 + np.abs(u))
            over, under = u > hi + margin, u < lo - margin
            assert over.sum() + under.sum() >= 0.05 * B * int(chain.sum())
            got = free.q.double().numpy()
            assert (got[over] > np.broadcast_to(hi, got.shape)[over]).all() and (got[under] < np.broadcast_to(lo, got.shape)[under]).all()
    finally:
        for damping, w in sorted(worst.items()):
            report("4-clamp-damping-%g" % damping, robot, path, w, step_bound(robot, damping))


# ------------------------------------------------------------------------------------------------------------------- section 5

POISONS = ("q0_nan", "q0_inf", "target_pos_inf", "target_quat_nan", "target_quat_zero")


def check_poisoned_rows(robot, link, dev, composed, what, pos_only, B, rows, K=8):
    """The poisoned rows: not converged, pos_err not finite, iterations == max_iterations; every other row bit-equal to the clean
    solve."""
    m, cpu = model(robot, dev), model(robot)
    q0, tp, tq, _ = seeded_problem(cpu, link, B, seed=47, pos_only=pos_only)
    clean = run(m, link, q0, tp, tq, dev, composed, max_iterations=K)
    assert torch.isfinite(clean.q).all() and torch.isfinite(clean.pos_err).all()
    q0, tp, tq = q0.clone(), tp.clone(), None if tq is None else tq.clone()
    for r in rows:
        if what == "q0_nan":
            q0[r, 1] = float("nan")
        elif what == "q0_inf":
            q0[r, 0] = float("inf")
        elif what == "target_pos_inf":
            tp[r, 2] = float("inf")
        elif what == "target_quat_nan":
            tq[r, 1] = float("nan")
        else:
            tq[r] = 0.0
    res = run(m, link, q0, tp, tq, dev, composed, max_iterations=K)
    bad = torch.zeros(B, dtype=torch.bool)
    bad[list(rows)] = True
    assert not res.converged[bad].any() and not torch.isfinite(res.pos_err[bad]).any() and (res.iterations[bad] == K).all()
    rows_equal(res, clean, ~bad, ~bad)
    assert torch.equal(res.converged[~bad], clean.converged[~bad])


def poison_cases():
    return [(w, po) for w in POISONS for po in (False, True) if not (po and w.startswith("target_quat"))]


# ------------------------------------------------------------------------------------------------------------------- section 6


def check_call_forms(robot, link, dev, composed, B=128):
    """float64 inputs and strided views give the bits of their contiguous float32 copies; an unbatched call takes one fp64-exact
    update and returns unbatched fields"""
    m, cpu = model(robot, dev), model(robot)
    q0, tp, tq, _ = seeded_problem(cpu, link, B, seed=48, noise=0.3)
    n = q0.shape[1]
    base = run(m, link, q0, tp, tq, dev, composed, max_iterations=6)
    assert (base.iterations > 0).any()
    rows_equal(base, run(m, link, q0.double(), tp.double(), tq.double(), dev, composed, max_iterations=6))
    Q0, TP, TQ = q0.to(dev), tp.to(dev), tq.to(dev)
    wide = torch.full((B, n + 3), 7.0, device=dev)
    wide[:, :n] = Q0
    tqT = TQ.t().contiguous().t()
    tpw = torch.full((B, 5), 7.0, device=dev)
    tpw[:, 1:4] = TP
    assert not wide[:, :n].is_contiguous() and not tqT.is_contiguous() and not tpw[:, 1:4].is_contiguous()
    s = m.compute_inverse_kinematics(wide[:, :n], link, tpw[:, 1:4], tqT, max_iterations=6, _composed=composed)
    assert torch.equal(s.q.cpu(), base.q) and torch.equal(s.iterations.cpu(), base.iterations)
    assert torch.equal(s.pos_err.cpu(), base.pos_err) and torch.equal(s.rot_err.cpu(), base.rot_err)
    assert (wide[:, n:] == 7.0).all()
    lower, upper = bounds(cpu)
    worst = 0.0
    for b in (0, 77):
        one = m.compute_inverse_kinematics(Q0[b], link, TP[b], TQ[b], max_iterations=1, tol_pos=0.0, tol_rot=0.0, damping=1.0,
                                           _composed=composed)
        assert one.q.shape == (n,) and one.pos_err.shape == () and one.rot_err.shape == () and one.iterations.shape == ()
        assert int(one.iterations) == 1 and one.iterations.dtype == torch.int32 and one.converged.dtype == torch.bool
        want = fp64_step(cpu, link, q0[b:b + 1], tp[b:b + 1], tq[b:b + 1], 1.0, lower, upper)
        worst = max(worst, check_step(one.q.cpu()[None], want, robot, 1.0))
    report("6-unbatched-step", robot, path_name(robot, dev, True), worst, TIGHT)       # (one row: never the fused kernel)


def perturbed_iiwa_spec(m):
    """the robot description of learnable_iiwa() with its learnable parameters' current values, for the oracle"""
    i = m._name_to_idx_map["iiwa_link_3"]
    trans, rpy = np.array(m._spec.trans, copy=True), np.array(m._spec.rpy, copy=True)
    trans[i] = (0.01, -0.02, 0.03)
    rpy[i] = (0.05, 0.0, -0.04)
    return dataclasses.replace(m._spec, trans=trans, rpy=rpy)


def check_learnable(dev, composed, B=256):
    """A model with learnable links: every update against fp64 on the PERTURBED robot description (2e-6 at damping 1.0: the
    constant model's Jacobian would miss it by orders of magnitude), and not the constant model's result"""
    link = "iiwa_link_ee"
    m = learnable_iiwa(dev)
    host = m if dev == "cpu" else learnable_iiwa()
    spec = perturbed_iiwa_spec(host)
    q0, tp, tq, _ = seeded_problem(host, link, B, seed=49)
    for damping in (1.0, 0.01):
        w, _, r = teacher_forced(m, "iiwa7", link, dev, composed, q0, tp, tq, 3, damping, 1.0, True, spec=spec)
        report("6-learnable-damping-%g" % damping, "iiwa7-learnable", path_name("iiwa7", dev, composed), w, step_bound("iiwa7", damping))
        const = run(model("iiwa7", dev), link, q0, tp, tq, dev, composed, max_iterations=3, tol_pos=0.0, tol_rot=0.0, damping=damping)
        assert not torch.equal(const.q, r.q)
        if damping == 1.0:          # (the perturbation is far above what the bound lets through)
            assert row_rel(const.q, r.q).max() > 100 * TIGHT


def check_mid_chain(link, dev, composed, B=256):
    """A target in the middle of the chain (the Jacobian columns of the distal DoFs are identically zero; the walk is not an arm
    chain, so a 7-DoF arm takes the composed path too): every update against fp64, and the distal DoFs never move"""
    robot = "panda_no_gripper"
    m, cpu = model(robot, dev), model(robot)
    for pos_only in (False, True):
        q0, tp, tq, _ = seeded_problem(cpu, link, B, seed=50, pos_only=pos_only)
        _, _, lin, ang = Oracle(cpu._spec).fk_jacobian(q0.double().numpy(), cpu._name_to_idx_map[link], np.float64)
        distal = (np.abs(lin).max(axis=(0, 1)) + np.abs(ang).max(axis=(0, 1))) == 0
        assert 0 < distal.sum() < q0.shape[1]
        for damping in (1.0, 0.01):
            w, _, _ = teacher_forced(m, robot, link, dev, composed, q0, tp, tq, 2, damping, 1.0, True)
            report("6-%s-damping-%g" % (link, damping), robot, path_name(robot, dev, True), w, step_bound(robot, damping))
        full = run(m, link, q0, tp, tq, dev, composed)
        assert torch.equal(full.q[:, distal], q0[:, distal]) and not torch.equal(full.q[:, ~distal], q0[:, ~distal])
        assert full.converged.float().mean() >= 0.9


# ----------------------------------------------------------------------------------------------------------------------- CPU

MIXED_CPU = [PANDA, ("iiwa7", "iiwa_link_ee"), ("fetch_arm_no_gripper", "virtual_ee_link"), ("fetch", "gripper_link"),
             ("allegro_left", "link_3.0_tip")]


@pytest.mark.parametrize("robot", ALL_ROBOTS)
def test_every_iteration_against_fp64(robot):
    check_every_iteration(robot, LINKS[robot], "cpu", False, 256)


@pytest.mark.parametrize("robot,link", MIXED_CPU)
def test_mixed_tiles(robot, link):
    check_mixed_tiles(robot, link, "cpu", False)


def test_mixed_tiles_many_iterations():
    check_mixed_tiles(*PANDA, "cpu", False, B=128, K=200, homogeneous=False)


@pytest.mark.parametrize("robot,link", list(FUSED) + [("fetch", "gripper_link"), ("jaco", "j2n6s300_end_effector"),
                                                       ("allegro_left", "link_3.0_tip")])
def test_error_measure_edges(robot, link):
    check_error_measure(robot, link, "cpu", False)
    check_large_rotation_step(robot, link, "cpu", False)


@pytest.mark.parametrize("robot,link", list(FUSED) + [("fetch", "gripper_link"), ("allegro_left", "link_3.0_tip")])
def test_clamps_that_bite(robot, link):
    check_clamps(robot, link, "cpu", False)


@pytest.mark.parametrize("what,pos_only", poison_cases())
@pytest.mark.parametrize("robot,link", [PANDA, ("fetch", "gripper_link")])
def test_non_finite_rows_are_isolated(robot, link, what, pos_only):
    check_poisoned_rows(robot, link, "cpu", False, what, pos_only, 130, (5,))


def test_call_forms():
    check_call_forms(*PANDA, "cpu", False)


def test_learnable_model_against_fp64():
    check_learnable("cpu", False)


@pytest.mark.parametrize("link", ["panda_link4", "panda_link6"])
def test_mid_chain_target(link):
    check_mid_chain(link, "cpu", False)


# ----------------------------------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("robot,link,composed", GPU_PATHS)
def test_gpu_every_iteration_against_fp64(robot, link, composed):
    check_every_iteration(robot, link, GPU, composed, 4096 if (robot, link) in FUSED else 257)


@pytest.mark.gpu
def test_gpu_every_iteration_ragged():
    """three tiles of the fused kernel and a tail of 37 rows on the composed path in one call"""
    check_every_iteration(*PANDA, GPU, False, 3 * 64 + 37, path="gpu-fused+tail")


@pytest.mark.gpu
@pytest.mark.parametrize("robot,link,composed", ARM_PATHS + [("fetch", "gripper_link", False), ("allegro_left", "link_3.0_tip", False)])
def test_gpu_mixed_tiles(robot, link, composed):
    check_mixed_tiles(robot, link, GPU, composed)


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True])
def test_gpu_mixed_tiles_many_iterations(composed):
    check_mixed_tiles(*PANDA, GPU, composed, B=128, K=200, homogeneous=False)


@pytest.mark.gpu
@pytest.mark.parametrize("robot,link,composed", ARM_PATHS + [("fetch", "gripper_link", False), ("jaco", "j2n6s300_end_effector", False)])
def test_gpu_error_measure_edges(robot, link, composed):
    check_error_measure(robot, link, GPU, composed)
    check_large_rotation_step(robot, link, GPU, composed)


@pytest.mark.gpu
@pytest.mark.parametrize("robot,link,composed", ARM_PATHS + [("fetch", "gripper_link", False), ("allegro_left", "link_3.0_tip", False)])
def test_gpu_clamps_that_bite(robot, link, composed):
    check_clamps(robot, link, GPU, composed)


@pytest.mark.gpu
@pytest.mark.parametrize("what,pos_only", poison_cases())
@pytest.mark.parametrize("robot,link,composed", [PANDA + (False,), PANDA + (True,), ("iiwa7", "iiwa_link_ee", False),
                                                 ("fetch", "gripper_link", False)])
def test_gpu_non_finite_rows_are_isolated(robot, link, composed, what, pos_only):
    check_poisoned_rows(robot, link, GPU, composed, what, pos_only, 256, (5, 70))


@pytest.mark.gpu
@pytest.mark.parametrize("robot,link,composed", [PANDA + (False,), PANDA + (True,), ("fetch", "gripper_link", False)])
def test_gpu_call_forms(robot, link, composed):
    check_call_forms(robot, link, GPU, composed)


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True])
def test_gpu_learnable_model_against_fp64(composed):
    check_learnable(GPU, composed)


@pytest.mark.gpu
@pytest.mark.parametrize("link", ["panda_link4", "panda_link6"])
def test_gpu_mid_chain_target(link):
    check_mid_chain(link, GPU, False)

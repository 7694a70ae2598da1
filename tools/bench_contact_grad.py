#!/usr/bin/env python3
"""Gradients through contact (compute_contact_torques_vjp, compute_contact_rollout(differentiable=True); csrc/drm_contact.hip) against
what they replace, on the same seeded inputs in one run:

  vjp        compute_contact_torques_vjp of B rows — fused (a 7-DoF arm's full tiles: ONE launch) and composed (_composed=True: two
             link-motion launches, the law's backward, two link-power-gradient launches, one external-torques launch, one add) —
             beside the forward compute_contact_torques (tau alone) of the same rows, and the byte floor of the VJP (84 B in, 56 B out
             per row) at the HBM peak (8.0 TB/s)
  rollout    forward + backward of L = sum q_T^2 + qd_T^2 through compute_contact_rollout(differentiable=True); the same through
             compute_forward_dynamics_rollout (no contact: what contact costs per step in the reverse sweep); the same through the
             per-step Python composition (compute_forward_kinematics per link, compute_link_velocities and compute_external_torques
             with differentiable_q=True, the law in torch, compute_forward_dynamics, the integrator); and the forward-only
             compute_contact_rollout call

CALL time: HIP events around back-to-back calls after warm-up, divided by their number, median of `--reps` windows — host work of a
call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o grad -- python tools/bench_contact_grad.py --trace B

whose statistics name contact_torques_vjp_arm_kernel and contact_torques_arm_kernel.

    python tools/bench_contact_grad.py [--vjp B,...] [--general robot:B,...] [--cases robot:B:T,...] [--reps 5] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_contact_rollout import DT, HBM_PEAK, setup, timed  # noqa: E402
from differentiable_robot_model_amd import JointLimitSprings, backend  # noqa: E402

VJP_ROWS = (4096, 65536, 1 << 20)
GENERAL = (("fetch", 65536), ("allegro_left", 65536))
CASES = (("panda_no_gripper", 4096, 64), ("panda_no_gripper", 65536, 32), ("allegro_left", 4096, 64))
VJP_BYTES = 84 + 56


def emit(out, text):
    print(text, flush=True)
    if out is not None:
        out.write(text + "\n")
        out.flush()


def vjp_setup(robot, B):
    m, links, par, springs, q, qd, _, offset, contact = setup(robot, B, 1)
    lam = torch.randn(B, m._n_dofs, generator=torch.Generator().manual_seed(B + 1)).to(q.device)
    return m, links, JointLimitSprings(*springs), q, qd, lam, contact


def bench_vjp(robot, B, reps, out, fused_expected):
    m, links, jl, q, qd, lam, contact = vjp_setup(robot, B)
    lw, TL, _, _ = m._links_plan(links)
    plane, radius, spr = m._contact_plan(contact, links, jl)[4:]
    launches = 20 if B <= 65536 else 5
    with torch.no_grad():
        call = lambda **kw: m.compute_contact_torques_vjp(q, qd, lam, contact, link_names=links, joint_limits=jl, **kw)
        t_vjp = timed(call, reps, launches)
        t_comp = timed(lambda: call(_composed=True), reps, max(2, launches // 4))
        t_fwd = timed(lambda: backend.contact_torques(lw.program, m._ops_f(lw).detach(), lw.ops_i, q, qd, TL, m._n_dofs, plane, radius, spr,
                                                      want_wrenches=False), reps, launches)
        a, b = call(), call(_composed=True)
        rel = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(a, b))
    floor = B * VJP_BYTES / HBM_PEAK * 1e6
    emit(out, "%-22s %8d | %9.1f %10.1f %9.1f | %6.2f %7.2f | %8.2f %6.1f %% | %8.1e" % (
        robot + ("" if fused_expected else " (general)"), B, t_vjp, t_comp, t_fwd, t_vjp / t_fwd, t_comp / t_vjp, floor, 100 * floor / t_vjp,
        rel))


def python_composition(m, links, q, qd, tau, par, springs, offset):
    """the per-step loop with autograd: the differentiable route without the fused node"""
    k, c, mu, ct, r = (par[x] for x in ("stiffness", "damping", "friction", "friction_slope", "radius"))
    kl, cl = springs
    lo, hi = m._joint_bounds()
    nz = torch.tensor([0.0, 0.0, 1.0], device=q.device)
    arm = -r * nz
    for t in range(tau.shape[0]):
        height = torch.stack([m.compute_forward_kinematics(q, name)[0][:, 2] for name in links], dim=1)
        lin, ang = m.compute_link_velocities(q, qd, link_names=links, differentiable_q=True)
        depth = r - (height - offset)
        vc = lin + torch.cross(ang, arm.expand_as(ang), dim=-1)
        vn = vc[..., 2]
        vt = vc - vn[..., None] * nz
        fn = ((k * depth - c * vn).clamp_min(0.0)) * (depth > 0)
        speed = (vt * vt).sum(-1).clamp_min(1e-30).sqrt()
        g = torch.where(fn > 0, torch.minimum(torch.full_like(fn, ct), mu * fn / speed), torch.zeros_like(fn))
        force = fn[..., None] * nz - g[..., None] * vt
        moment = torch.cross(arm.expand_as(force), force, dim=-1)
        tau_ext = m.compute_external_torques(q, force, moment, link_names=links, differentiable_q=True)
        tau_lim = torch.where(q < lo, kl * (lo - q) - cl * qd, torch.where(q > hi, -kl * (q - hi) - cl * qd, torch.zeros_like(q)))
        qdd = m.compute_forward_dynamics(q, qd, tau[t] + (tau_ext + tau_lim), include_gravity=True, use_damping=False)
        qd = qd + DT * qdd
        q = q + DT * qd
    return q, qd


def bench_rollout(robot, B, T, reps, out):
    m, links, par, springs, q, qd, tau, offset, contact = setup(robot, B, T)
    jl = JointLimitSprings(*springs)

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in (q, qd, tau)]

    def through(fn):
        def run():
            x = leaves()
            a, b = fn(*x)
            (a.square().sum() + b.square().sum()).backward()
            return [t.grad for t in x]
        return run
    contact_fb = through(lambda a, b, c: [x[-1] for x in m.compute_contact_rollout(a, b, c, DT, contact, link_names=links, joint_limits=jl,
                                                                                   differentiable=True)[:2]])
    plain_fb = through(lambda a, b, c: [x[-1] for x in m.compute_forward_dynamics_rollout(a, b, c, DT)])
    loop_fb = through(lambda a, b, c: python_composition(m, links, a, b, c, par, springs, offset))
    t_contact = timed(contact_fb, reps, 2)
    t_plain = timed(plain_fb, reps, 2)
    t_loop = timed(loop_fb, max(2, reps // 2), 1)
    with torch.no_grad():
        t_forward = timed(lambda: m.compute_contact_rollout(q, qd, tau, DT, contact, link_names=links, joint_limits=jl), reps, 5)
    # the two gradients row by row: d_loop is the worst row's max|d| / max|.|, `off` the rows beyond 1e-4 (a row whose two float32
    # forwards take a switch of the law differently after T steps has another gradient in each)
    ga, gl = contact_fb(), loop_fb()
    worst = torch.zeros(B, device=q.device)
    for x, y in zip(ga, gl):
        d = (x - y).abs() / y.abs().max().clamp_min(1e-30)
        worst = torch.maximum(worst, d.amax(dim=-1) if d.ndim == 2 else d.amax(dim=(0, 2)))
    emit(out, "%-22s %7d %3d | %10.1f %10.1f %11.1f %10.1f | %7.1f | %11.2f | %8.1e %5d" % (
        robot, B, T, t_contact, t_plain, t_loop, t_forward, t_loop / t_contact, (t_contact - t_plain) / T, float(worst.max()),
        int((worst > 1e-4).sum())))
    del q, qd, tau
    torch.cuda.empty_cache()


def trace(B, launches=10):
    m, links, jl, q, qd, lam, contact = vjp_setup("panda_no_gripper", B)
    with torch.no_grad():
        for fn in (lambda: m.compute_contact_torques_vjp(q, qd, lam, contact, link_names=links, joint_limits=jl),
                   lambda: m.compute_contact_torques(q, qd, contact, link_names=links, joint_limits=jl)):
            for _ in range(2 + launches):
                fn()
            torch.cuda.synchronize()
    print("traced B = %d: 2 + %d calls of the contact torques VJP and of the contact torques" % (B, launches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vjp", default="", help="B,... rows of the VJP measurement on the Panda")
    ap.add_argument("--general", default="", help="robot:B,... of the general path")
    ap.add_argument("--cases", default="", help="robot:B:T,... of the rollout measurement")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--trace", type=int, default=None, help="B: the profiled pass of the VJP and the forward on the Panda")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_contact_grad.py measures on a HIP device"
    if args.trace:
        return trace(args.trace)
    out = open(args.out, "a") if args.out else None
    rows = [int(x) for x in args.vjp.split(",")] if args.vjp else VJP_ROWS
    general = [(g.split(":")[0], int(g.split(":")[1])) for g in args.general.split(",")] if args.general else GENERAL
    cases = [(c.split(":")[0], int(c.split(":")[1]), int(c.split(":")[2])) for c in args.cases.split(",")] if args.cases else CASES
    emit(out, "call times in us (HIP events, median of %d windows); byte floor of the VJP: %d B per row at %.1f TB/s" % (
        args.reps, VJP_BYTES, HBM_PEAK / 1e12))
    emit(out, "%-22s %8s | %9s %10s %9s | %6s %7s | %8s %8s | %8s" % ("compute_contact_torques_vjp", "B", "vjp", "composed", "forward",
                                                                   "x_fwd", "x_comp", "floor us", "share", "d_comp"))
    for B in rows:
        bench_vjp("panda_no_gripper", B, args.reps, out, True)
    for robot, B in general:
        bench_vjp(robot, B, args.reps, out, False)
    emit(out, "%-22s %7s %3s | %10s %10s %11s %10s | %7s | %11s | %8s %5s" % ("rollout forward+backward", "B", "T", "contact", "plain", "python",
                                                                            "fwd only", "x_loop", "+us/step", "d_loop", "off"))
    for robot, B, T in cases:
        bench_rollout(robot, B, T, args.reps, out)


if __name__ == "__main__":
    main()

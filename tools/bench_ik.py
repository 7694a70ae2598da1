#!/usr/bin/env python3
"""Batched inverse kinematics (compute_inverse_kinematics, csrc/drm_ik.hip) three ways on the same seeded inputs, HIP events after
warm-up: the fused call (one launch per solve for 7-DoF arms), the composed call (DRM_IK_COMPOSED: drm_fk_jacobian + an update kernel
per iteration) and the Python loop it replaces (compute_fk_and_jacobian, a batched Cholesky solve with torch.linalg.cholesky_ex /
cholesky_solve, J^T y and the clamps: no host synchronisation either).

The inputs are the tests' calibration setup: q* uniform in the middle 80 % of each joint's range, target = FK(q*),
q0 = clamp(q* + 0.1 N(0, 1)); defaults damping 0.01, tolerances 1e-4 m / 1e-3 rad.

    python tools/bench_ik.py [--cases panda_no_gripper:panda_virtual_ee_link,...] [--reps 5]

Prints one line per (robot, B, K): the three times, the fused call's speed-up over the loop and over the composed call, the converged
fraction, the mean number of iterations and rows x iterations per second of the fused call.
"""
import argparse
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from differentiable_robot_model_amd.robot_model import DifferentiableRobotModel, robot_description_folder  # noqa: E402

# (robot, link, position only, sizes, iteration counts)
FUSED_SIZES, COMPOSED_SIZES, KS = (4096, 65536, 1 << 20), (4096, 65536), (8, 32)
CASES = (("panda_no_gripper", "panda_virtual_ee_link", False, FUSED_SIZES), ("iiwa7", "iiwa_link_ee", False, FUSED_SIZES),
         ("fetch_arm_no_gripper", "virtual_ee_link", False, FUSED_SIZES), ("fetch", "gripper_link", False, COMPOSED_SIZES),
         ("jaco", "j2n6s300_end_effector", False, COMPOSED_SIZES), ("allegro_left", "link_3.0_tip", True, COMPOSED_SIZES))


def python_loop(model, link, q0, tp, tq, K, lower, upper, damping=0.01, tol_pos=1e-4, tol_rot=1e-3):
    """The per-iteration loop of the issue: ~15 launches per iteration, no host synchronisation (cholesky_ex, not solve)."""
    B = q0.shape[0]
    q = q0
    done = torch.zeros(B, dtype=torch.bool, device=q0.device)
    eye = torch.eye(3 if tq is None else 6, device=q0.device) * damping ** 2
    conj = torch.tensor([-1.0, -1.0, -1.0, 1.0], device=q0.device)
    for i in range(K + 1):
        p, c, lin, ang = model.compute_fk_and_jacobian(q, link)
        e = tp - p
        conv = e.norm(dim=1) <= tol_pos
        if tq is not None:
            a, b = tq, c * conj
            eq = torch.stack([a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                              a[:, 3] * b[:, 1] - a[:, 0] * b[:, 2] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0],
                              a[:, 3] * b[:, 2] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3],
                              a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]], 1)
            eq = torch.where(eq[:, 3:] < 0, -eq, eq)
            s = eq[:, :3].norm(dim=1)
            th = 2 * torch.atan2(s, eq[:, 3])
            e = torch.cat([e, eq[:, :3] * torch.where(s > 0, th / s.clamp_min(1e-30), 2.0)[:, None]], 1)
            conv = conv & (th <= tol_rot)
        done = done | conv
        if i == K:
            break
        J = lin if tq is None else torch.cat([lin, ang], 1)
        L, _ = torch.linalg.cholesky_ex(J @ J.transpose(1, 2) + eye)
        qn = q + (J.transpose(1, 2) @ torch.cholesky_solve(e[..., None], L))[..., 0]
        q = torch.where(done[:, None], q, torch.minimum(torch.maximum(qn, lower), upper))
    return q, done


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def problem(m, link, B, pos_only, seed):
    lim = m.get_joint_limits()
    lo = torch.tensor([j["lower"] for j in lim]); hi = torch.tensor([j["upper"] for j in lim])
    free = lo >= hi
    lo, hi = torch.where(free, -np.pi, lo), torch.where(free, np.pi, hi)
    g = torch.Generator().manual_seed(seed)
    qs = (lo + (hi - lo) * (0.1 + 0.8 * torch.rand(B, lo.shape[0], generator=g))).cuda()
    noise = (0.1 * torch.randn(qs.shape, generator=g)).cuda()
    with torch.no_grad():
        p, r = m.compute_forward_kinematics(qs, link)
    lower, upper = m._joint_bounds()
    q0 = torch.minimum(torch.maximum(qs + noise, lower), upper)
    return q0, p.clone(), None if pos_only else r.clone(), lower, upper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:link[:pos],... (default: every case of the issue)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="")
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--no-loop", action="store_true", help="skip the Python loop")
    args = ap.parse_args()
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], c.split(":")[1], c.endswith(":pos"), COMPOSED_SIZES) for c in args.cases.split(",")]
    if args.sizes:
        cases = [c[:3] + (tuple(int(x) for x in args.sizes.split(",")),) for c in cases]
    ks = [int(k) for k in args.ks.split(",")]
    print("%-20s %-22s %8s %3s %11s %11s %11s %8s %8s %7s %6s %10s" % (
        "robot", "link", "B", "K", "fused_us", "composed_us", "loop_us", "x_loop", "x_comp", "conv%", "iters", "row_it/s"))
    for robot, link, pos_only, sizes in cases:
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = DifferentiableRobotModel(os.path.join(robot_description_folder, robot + ".urdf"), device="cuda:0")
        for B in sizes:
            q0, tp, tq, lower, upper = problem(m, link, B, pos_only, seed=B)
            for K in ks:
                with torch.no_grad():
                    fused = lambda: m.compute_inverse_kinematics(q0, link, tp, tq, max_iterations=K)  # noqa: E731
                    t_f = timed(fused, args.reps)
                    t_c = timed(lambda: m.compute_inverse_kinematics(q0, link, tp, tq, max_iterations=K, _composed=True), args.reps)
                    t_l = float("nan")
                    if not args.no_loop:
                        tqn = tq / tq.norm(dim=1, keepdim=True) if tq is not None else None
                        t_l = timed(lambda: python_loop(m, link, q0, tp, tqn, K, lower, upper), args.reps, warmup=1)
                    res = fused()
                    conv = res.converged.float().mean().item()
                    iters = res.iterations.float().mean().item()
                print("%-20s %-22s %8d %3d %11.1f %11.1f %11.1f %8.2f %8.2f %7.2f %6.2f %10.3e" % (
                    robot, link, B, K, t_f, t_c, t_l, t_l / t_f, t_c / t_f, 100 * conv, iters, B * iters / (t_f * 1e-6)), flush=True)
            del q0, tp, tq
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Batched inverse kinematics with many seeds per target: every target pose of a Franka Panda's end effector is solved from S random
joint configurations at once (compute_inverse_kinematics: damped least squares, one kernel launch per solve on the GPU), and the best
seed of each target is kept — the converged seed with the smallest error, else the seed with the smallest error.

    python examples/inverse_kinematics_panda.py [--targets 1024] [--seeds 16] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda

EE = "panda_virtual_ee_link"


def run(targets=1024, seeds=16, max_iterations=32, device="cuda", verbose=True):
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    lim = model.get_joint_limits()
    lower = torch.tensor([j["lower"] for j in lim], device=device)
    upper = torch.tensor([j["upper"] for j in lim], device=device)
    n = model._n_dofs
    # reachable targets: the poses of random configurations in the middle 80 % of each joint's range
    u = torch.rand(targets, n, device=device)
    q_true = lower + (upper - lower) * (0.1 + 0.8 * u)
    with torch.no_grad():
        tp, tq = model.compute_forward_kinematics(q_true, EE)
    # S seeds per target, uniform over the joint ranges: rows t * S .. t * S + S - 1 belong to target t
    q0 = lower + (upper - lower) * torch.rand(targets * seeds, n, device=device)
    res = model.compute_inverse_kinematics(q0, EE, tp.repeat_interleave(seeds, 0), tq.repeat_interleave(seeds, 0),
                                           max_iterations=max_iterations)
    score = (res.pos_err + 0.1 * res.rot_err).reshape(targets, seeds)
    score = score + (~res.converged).reshape(targets, seeds).float() * 1e3     # converged seeds first
    score = torch.nan_to_num(score, nan=float("inf"))
    best = score.argmin(1)
    rows = torch.arange(targets, device=device) * seeds + best
    q_best, solved = res.q[rows], res.converged[rows]
    with torch.no_grad():
        p, _ = model.compute_forward_kinematics(q_best, EE)
    pos_err = (p - tp).norm(dim=1)
    stats = dict(solved=solved.float().mean().item(), seeds_converged=res.converged.float().mean().item(),
                 mean_iterations=res.iterations.float().mean().item(), max_pos_err_solved=pos_err[solved].max().item() if solved.any() else 0.0)
    if verbose:
        print("%d targets x %d seeds: %.1f %% of the targets solved (%.1f %% of the seeds converged, %.2f iterations on average); "
              "worst position error of a solved target %.2e m" % (targets, seeds, 100 * stats["solved"], 100 * stats["seeds_converged"],
                                                                 stats["mean_iterations"], stats["max_pos_err_solved"]))
    return q_best, solved, stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.targets, a.seeds, a.iterations, a.device)

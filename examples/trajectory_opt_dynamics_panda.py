#!/usr/bin/env python3
"""Trajectory optimisation THROUGH THE DYNAMICS of a Franka Panda: the dynamic counterpart of the reference's kinematic example
(examples/run_kinematic_trajectory_opt.py optimises joint positions directly).  Here the decision variables are a torque sequence
tau [T, 7] on top of gravity compensation; the state follows from compute_forward_dynamics_rollout (T steps of forward dynamics and
semi-implicit Euler in one launch), and Adam brings the end effector to a goal position at rest.  Gradients come from the rollout's
reverse sweep (one autograd node for the whole trajectory).

    python examples/trajectory_opt_dynamics_panda.py [--steps 100] [--iters 200] [--particles 1]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda

EE = "panda_virtual_ee_link"


def run(steps=100, iters=200, particles=1, dt=1e-2, lr=0.5, device="cuda", verbose=True):
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    n = model._n_dofs
    q0 = torch.tensor([0.0, -0.3, 0.0, -2.2, 0.0, 2.0, 0.8], device=device).repeat(particles, 1)
    qd0 = torch.zeros_like(q0)
    goal = torch.tensor([0.45, 0.25, 0.45], device=device)
    with torch.no_grad():   # gravity compensation at the start state: a zero correction keeps the arm roughly where it is
        hold = model.compute_inverse_dynamics(q0, qd0, torch.zeros_like(q0))
    correction = torch.zeros(steps, particles, n, device=device, requires_grad=True)
    opt = torch.optim.Adam([correction], lr=lr)
    history = []
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        q_traj, qd_traj = model.compute_forward_dynamics_rollout(q0, qd0, hold + correction, dt)
        pos = model.compute_forward_kinematics(q_traj[-1], EE)[0]
        loss = ((pos - goal) ** 2).sum(-1).mean() + 1e-2 * (qd_traj[-1] ** 2).sum(-1).mean() + 1e-6 * (correction ** 2).mean()
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
        if verbose and (it % max(1, iters // 10) == 0 or it == iters - 1):
            print("iter %4d  loss %.4e  |ee - goal| %.4f m" % (it, history[-1], float((pos - goal).norm(dim=-1).mean())))
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--particles", type=int, default=1)
    a = ap.parse_args()
    run(a.steps, a.iters, a.particles)

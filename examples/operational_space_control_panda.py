#!/usr/bin/env python3
"""Operational-space control of a batch of Franka Pandas: a task-space PD law drives every robot's end effector to its own target
position.  Every control tick asks compute_operational_space_dynamics (one kernel launch on the GPU) for the task-space inertia,
the dynamically consistent inverse of the Jacobian, Jdot qd and the task-space bias force, commands

    tau = J^T (inertia a_des + bias_force) + (I - J^T jacobian_pinv^T) tau_0,    a_des = kp (p* - p) - kd J qd,   tau_0 = nle - kn qd

(the second term holds the arm against gravity and damps the motion the task leaves free, without disturbing the task) and integrates the robot with
compute_forward_dynamics and a semi-implicit Euler step.

    python examples/operational_space_control_panda.py [--batch 1024] [--steps 400] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda

EE = "panda_virtual_ee_link"


def run(batch=1024, steps=400, dt=2e-3, kp=100.0, kd=20.0, kn=10.0, regularization=0.05, device="cuda", verbose=True):
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    lim = model.get_joint_limits()
    lower = torch.tensor([j["lower"] for j in lim], device=device)
    upper = torch.tensor([j["upper"] for j in lim], device=device)
    n = model._n_dofs
    # start in the middle half of every joint's range, at rest; the target is the end effector's position a short way off
    q = lower + (upper - lower) * (0.25 + 0.5 * torch.rand(batch, n, device=device))
    qd = torch.zeros(batch, n, device=device)
    eye = torch.eye(n, device=device)
    with torch.no_grad():
        goal = model.compute_forward_kinematics((q + 0.3 * torch.randn(batch, n, device=device)).clamp(lower, upper), EE)[0]
        start_err = (goal - model.compute_forward_kinematics(q, EE)[0]).norm(dim=1)
        for _ in range(steps):
            p, _, lin, _ = model.compute_fk_and_jacobian(q, EE)
            osd = model.compute_operational_space_dynamics(q, qd, EE, position_only=True, regularization=regularization)
            a_des = kp * (goal - p) - kd * (lin @ qd[..., None])[..., 0]
            force = (osd.inertia @ a_des[..., None])[..., 0] + osd.bias_force
            null = eye - lin.transpose(1, 2) @ osd.jacobian_pinv.transpose(1, 2)
            tau_0 = model.compute_non_linear_effects(q, qd, include_gravity=True, use_damping=False) - kn * qd
            tau = (lin.transpose(1, 2) @ force[..., None] + null @ tau_0[..., None])[..., 0]
            qdd = model.compute_forward_dynamics(q, qd, tau)
            qd = qd + dt * qdd
            q = q + dt * qd
        end_err = (goal - model.compute_forward_kinematics(q, EE)[0]).norm(dim=1)
    stats = dict(start_err=start_err.mean().item(), end_err=end_err.mean().item(), worst_ratio=(end_err / start_err).max().item(),
                 joint_speed=qd.abs().max().item())
    if verbose:
        print("%d Pandas, %d ticks of %.1f ms: mean position error %.3f m -> %.2e m (worst robot: %.3f of its initial error), "
              "largest joint speed at the end %.2e rad/s" % (batch, steps, 1e3 * dt, stats["start_err"], stats["end_err"],
                                                             stats["worst_ratio"], stats["joint_speed"]))
    return q, stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.steps, device=a.device)

#!/usr/bin/env python3
"""Trajectory optimisation THROUGH contact: a batch of Franka Pandas, each with its own torque sequence, optimised so that after T
steps the hand rests on a horizontal plane at a target point.  The simulator is ONE differentiable call,

    out = model.compute_contact_rollout(q0, qd0, tau, dt, contact, joint_limits=..., differentiable=True)

(csrc/drm_contact.hip: on a HIP device the forward is one kernel launch for a batch that is a multiple of 64), and the gradient of the
loss with respect to tau [T, B, n] comes from its reverse sweep: per step the two launches of the forward-dynamics backward and one
drm_contact_torques_vjp call — no per-step Python composition of Jacobians, a torch law and forward dynamics.

The arms start at rest a few centimetres above the plane, held by gravity compensation (the initial guess).  The loss is the squared
distance of the hand's origin from the target on the plane at the last step, plus a little of the final joint velocity and of the
torques' departure from the initial guess.  The hand has to go down INTO contact: the last part of the motion is shaped by the
plane's force, and so is the gradient.

    python examples/contact_trajopt_panda.py [--batch 64] [--steps 60] [--dt 5e-3] [--iters 60] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda, JointLimitSprings, PlaneContact

HAND = "panda_virtual_ee_link"
RADIUS = 0.03          # the contact sphere on every link
CLEARANCE = 0.05       # how far above the plane the hand's sphere starts
STIFFNESS = 2.0e3      # N / m
DAMPING = 40.0         # N s / m


def run(batch=64, steps=60, dt=5e-3, iters=60, lr=0.3, device="cuda", verbose=True):
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    n = model._n_dofs
    nominal = torch.tensor([0.0, 0.9, 0.0, -0.5, 0.0, 1.2, 0.0, 0.02, 0.02][:n], device=device)
    q0 = nominal[None] + 0.05 * (2 * torch.rand(batch, n, device=device) - 1)
    qd0 = torch.zeros_like(q0)
    with torch.no_grad():
        hand0, _ = model.compute_forward_kinematics(q0, HAND)
        plane_z = float(hand0[:, 2].min()) - RADIUS - CLEARANCE
        hold = model.compute_inverse_dynamics(q0, qd0, torch.zeros_like(q0), include_gravity=True)
    contact = PlaneContact(normal=(0.0, 0.0, 1.0), offset=plane_z, stiffness=STIFFNESS, damping=DAMPING, friction=0.5,
                           friction_slope=50.0, radius=RADIUS)
    limits = JointLimitSprings(50.0, 0.5)
    # the target: 5 cm further out than the hand starts, resting on the plane
    target = hand0.clone()
    target[:, 0] += 0.05
    target[:, 2] = plane_z + RADIUS
    guess = hold[None].expand(steps, batch, n).contiguous()
    tau = guess.clone().requires_grad_(True)
    opt = torch.optim.Adam([tau], lr=lr)
    history = []
    for it in range(iters):
        opt.zero_grad()
        out = model.compute_contact_rollout(q0, qd0, tau, dt, contact, joint_limits=limits, differentiable=True)
        hand, _ = model.compute_forward_kinematics(out.q[-1], HAND)
        miss = ((hand - target) ** 2).sum(-1)
        loss = (miss + 1e-3 * (out.qd[-1] ** 2).sum(-1)).mean() + 1e-5 * ((tau - guess) ** 2).mean()
        loss.backward()
        opt.step()
        history.append((loss.item(), miss.detach().mean().sqrt().item()))
        if verbose and (it % 10 == 0 or it == iters - 1):
            print("iteration %3d   loss %.6f   rms distance of the hand from its target %.4f m" % (it, history[-1][0], history[-1][1]))
    with torch.no_grad():
        out = model.compute_contact_rollout(q0, qd0, tau.detach(), dt, contact, joint_limits=limits)
        wrench = model.compute_contact_torques(out.q[-1], out.qd[-1], contact, joint_limits=limits)
        touching = float((wrench.force[..., 2].max(dim=1).values > 0).float().mean())
        height = float((model.compute_forward_kinematics(out.q[-1], HAND)[0][:, 2] - plane_z).mean())
    if verbose:
        print("%d Pandas, %d steps of %.1e s: loss %.6f -> %.6f; at the end %.0f %% of the arms touch the plane, the hand's origin %.3f m "
              "above it (sphere radius %.3f m)" % (batch, steps, dt, history[0][0], history[-1][0], 100 * touching, height, RADIUS))
    return dict(first=history[0][0], last=history[-1][0], distance_first=history[0][1], distance_last=history[-1][1], touching=touching,
                height=height, history=history)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--dt", type=float, default=5e-3)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--lr", type=float, default=0.3)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.steps, a.dt, a.iters, a.lr, device=a.device)

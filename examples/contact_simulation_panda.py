#!/usr/bin/env python3
"""Penalty contact for a batch of Franka Pandas: the arms are released torque-free above the horizontal plane their base stands on and
fall onto it; a spring-damper at every link origin, written in torch, pushes back.

Each step makes ONE compute_link_motion launch (the origins' heights and velocities), ONE compute_external_torques launch (the contact
forces as joint torques) and one compute_forward_dynamics call, qdd = FD(q, qd, tau_ext), followed by a semi-implicit Euler update.
The same arms are simulated once more without the plane: there the lowest link origin ends far below it.

The two launches are adjoint to each other, sum_l f_l . v_l == tau_ext . qd, so the work of the contact forces can be accumulated on
either side: sum f . v dt at the links and sum tau_ext . qd dt at the joints.  Both are printed.

    python examples/contact_simulation_panda.py [--batch 256] [--steps 1200] [--dt 5e-4] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda

PLANE_Z = 0.0          # the plane the base stands on
STIFFNESS = 2.0e4      # N / m
DAMPING = 2.0e2        # N s / m


def contact_forces(height, vertical_velocity):
    """[B, L, 3] spring-damper forces of the plane on the link origins: along +z, never pulling"""
    depth = (PLANE_Z - height).clamp_min(0.0)
    fz = (STIFFNESS * depth - DAMPING * vertical_velocity * (depth > 0)).clamp_min(0.0)
    return torch.stack([torch.zeros_like(fz), torch.zeros_like(fz), fz], dim=-1)


def simulate(model, links, q, qd, steps, dt, contact):
    """-> (lowest origin height over the batch at the end, lowest over the run, contact work at the links [B], at the joints [B], the
    sum of the absolute work terms [B]); works in float64"""
    q, qd = q.clone(), qd.clone()
    B = q.shape[0]
    work_links = torch.zeros(B, dtype=torch.float64, device=q.device)
    work_joints, terms = torch.zeros_like(work_links), torch.zeros_like(work_links)
    lowest_ever = float("inf")
    for _ in range(steps):
        tau_ext = torch.zeros_like(q)
        if contact:
            motion = model.compute_link_motion(q, qd, link_names=links)
            force = contact_forces(motion.position[..., 2], motion.linear_velocity[..., 2])
            tau_ext = model.compute_external_torques(q, force, link_names=links)
            at_links = (force.double() * motion.linear_velocity.double()).flatten(1)
            at_joints = tau_ext.double() * qd.double()
            work_links += dt * at_links.sum(1)
            work_joints += dt * at_joints.sum(1)
            terms += dt * (at_links.abs().sum(1) + at_joints.abs().sum(1))
            lowest_ever = min(lowest_ever, motion.position[..., 2].min().item())
        qdd = model.compute_forward_dynamics(q, qd, tau_ext, include_gravity=True, use_damping=False)
        qd = qd + dt * qdd
        q = q + dt * qd
    height = model.compute_link_motion(q, qd, link_names=links).position[..., 2]
    return height.min().item(), min(lowest_ever, height.min().item()), work_links, work_joints, terms


def run(batch=256, steps=1200, dt=5e-4, device="cuda", verbose=True):
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    spec = model._spec
    names = model.get_link_names()
    links = [names[i] for i in range(1, len(names)) if any(spec.dof[j] >= 0 for j in spec.chain_to(i))]   # the links a joint moves
    # leaning forward, so that gravity swings the arm down onto the plane
    q0 = torch.tensor([0.0, 0.9, 0.0, -0.5, 0.0, 1.2, 0.0, 0.02, 0.02][:model._n_dofs], device=device)
    q0 = q0[None] + 0.1 * (2 * torch.rand(batch, model._n_dofs, device=device) - 1)
    qd0 = torch.zeros_like(q0)
    with torch.no_grad():
        start = model.compute_link_motion(q0, qd0, link_names=links).position[..., 2].min().item()
        end_c, low_c, w_links, w_joints, terms = simulate(model, links, q0, qd0, steps, dt, contact=True)
        end_f, low_f, _, _, _ = simulate(model, links, q0, qd0, steps, dt, contact=False)
    stats = dict(start=start, lowest_with_contact=end_c, lowest_without_contact=end_f, lowest_ever_with_contact=low_c,
                 work_links=w_links, work_joints=w_joints, work_terms=terms)
    if verbose:
        print("%d Pandas, %d steps of %.1e s, %d contact points each; lowest link origin at release %.3f m above the plane" % (
            batch, steps, dt, len(links), start - PLANE_Z))
        print("lowest link origin at the end:  with contact %+.4f m   without %+.4f m   (deepest penetration during the run %.4f m)" % (
            end_c - PLANE_Z, end_f - PLANE_Z, max(0.0, PLANE_Z - low_c)))
        print("contact work, summed over the batch:  sum f.v dt = %+.6e J   sum tau_ext.qd dt = %+.6e J   (worst robot: |difference| "
              "%.2e J of %.2e J of terms)" % (w_links.sum().item(), w_joints.sum().item(), (w_links - w_joints).abs().max().item(),
                                                 terms.max().item()))
    return stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--dt", type=float, default=5e-4)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.steps, a.dt, device=a.device)

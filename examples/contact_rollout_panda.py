#!/usr/bin/env python3
"""The scenario of contact_simulation_panda.py — a batch of Franka Pandas released torque-free above the horizontal plane their base
stands on, a spring-damper at every link origin pushing back — with the contact law inside the rollout: ONE
compute_contact_rollout call per chunk of steps instead of a link-motion launch, a handful of torch kernels, an external-torques launch,
a forward-dynamics call and a torch integrator per step.  On a HIP device a chunk is one kernel launch (csrc/drm_contact.hip: the
state stays in registers across the steps) when the batch is a multiple of 64.

The same arms are simulated once more without the plane (compute_forward_dynamics_rollout): there the lowest link origin ends far
below it.  With --friction the plane also resists sliding (regularised Coulomb friction), which the per-step example has no law for.

    python examples/contact_rollout_panda.py [--batch 256] [--steps 1200] [--chunk 100] [--dt 5e-4] [--friction 0.0] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda, PlaneContact

PLANE_Z = 0.0          # the plane the base stands on
STIFFNESS = 2.0e4      # N / m
DAMPING = 2.0e2        # N s / m
FRICTION_SLOPE = 50.0  # N s / m: the viscous slope of the regularised friction law


def simulate(model, links, q, qd, steps, chunk, dt, contact):
    """-> (lowest origin height over the batch at the end, lowest over the states at the ends of the chunks)"""
    lowest_ever = float("inf")
    done = 0
    while done < steps:
        T = min(chunk, steps - done)
        tau = torch.zeros(T, *q.shape, device=q.device)
        if contact is not None:
            out = model.compute_contact_rollout(q, qd, tau, dt, contact, link_names=links)
            q, qd = out.q[-1], out.qd[-1]
        else:
            qs, qds = model.compute_forward_dynamics_rollout(q, qd, tau, dt)
            q, qd = qs[-1], qds[-1]
        done += T
        height = model.compute_link_motion(q, qd, link_names=links).position[..., 2]
        lowest_ever = min(lowest_ever, height.min().item())
    return height.min().item(), lowest_ever


def run(batch=256, steps=1200, chunk=100, dt=5e-4, friction=0.0, device="cuda", verbose=True):
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    spec = model._spec
    names = model.get_link_names()
    links = [names[i] for i in range(1, len(names)) if any(spec.dof[j] >= 0 for j in spec.chain_to(i))]   # the links a joint moves
    contact = PlaneContact(normal=(0.0, 0.0, 1.0), offset=PLANE_Z, stiffness=STIFFNESS, damping=DAMPING, friction=friction,
                           friction_slope=FRICTION_SLOPE if friction > 0 else 0.0)
    # leaning forward, so that gravity swings the arm down onto the plane
    q0 = torch.tensor([0.0, 0.9, 0.0, -0.5, 0.0, 1.2, 0.0, 0.02, 0.02][:model._n_dofs], device=device)
    q0 = q0[None] + 0.1 * (2 * torch.rand(batch, model._n_dofs, device=device) - 1)
    qd0 = torch.zeros_like(q0)
    with torch.no_grad():
        start = model.compute_link_motion(q0, qd0, link_names=links).position[..., 2].min().item()
        end_c, low_c = simulate(model, links, q0, qd0, steps, chunk, dt, contact)
        end_f, low_f = simulate(model, links, q0, qd0, steps, chunk, dt, None)
    stats = dict(start=start, lowest_with_contact=end_c, lowest_without_contact=end_f, lowest_ever_with_contact=low_c,
                 calls=2 * ((steps + chunk - 1) // chunk))
    if verbose:
        print("%d Pandas, %d steps of %.1e s in chunks of %d, %d contact points each; lowest link origin at release %.3f m above the "
              "plane" % (batch, steps, dt, chunk, len(links), start - PLANE_Z))
        print("lowest link origin at the end:  with contact %+.4f m   without %+.4f m   (deepest penetration at the end of a chunk "
              "%.4f m)" % (end_c - PLANE_Z, end_f - PLANE_Z, max(0.0, PLANE_Z - low_c)))
    return stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--dt", type=float, default=5e-4)
    ap.add_argument("--friction", type=float, default=0.0)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.steps, a.chunk, a.dt, a.friction, device=a.device)

#!/usr/bin/env python3
"""Posture optimisation with obstacles: a batch of Franka Pandas starts at random postures and descends on

    collision cost(q) + 1/2 k |p_ee(q) - p_goal|^2,

the cost of compute_collision_cost — spheres on the links against a world of spheres and boxes and against each other — plus a soft
end-effector position penalty.  ONE launch per step gives the collision cost and its gradient for the whole batch (csrc/
drm_collision.hip; on a HIP device a block of four wavefronts per 64 postures), autograd multiplies it through; the penalty goes through
compute_forward_kinematics.  compute_sphere_distances says, before and after, which postures are in collision (a clearance < 0).

    python examples/collision_avoidance_panda.py [--batch 1024] [--steps 200] [--lr 0.02] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import CollisionSpheres, CollisionWorld, DifferentiableFrankaPanda

EE = "panda_virtual_ee_link"
GOAL_WEIGHT = 20.0         # k of the end-effector penalty, per m^2
ACTIVATION = dict(world_activation=0.05, self_activation=0.02, world_weight=10.0, self_weight=10.0)


def geometry_of(model):
    """two spheres per moving link — at the link origin and 8 cm down its z axis — two obstacle spheres and a table-like box"""
    names = model.get_link_names()[1:]
    links = [n for n in names for _ in range(2)]
    centers = [c for _ in names for c in ((0.0, 0.0, 0.0), (0.0, 0.0, -0.08))]
    spheres = CollisionSpheres(links, centers, [0.04] * len(links))
    world = CollisionWorld(spheres=[[0.45, 0.25, 0.45, 0.12], [0.35, -0.35, 0.7, 0.10]],
                           box_centers=[[0.55, 0.0, 0.1]], box_half_extents=[[0.25, 0.4, 0.1]])
    return model.make_collision_geometry(spheres, world, self_pairs="auto")


def in_collision(model, q, geometry):
    d = model.compute_sphere_distances(q, geometry)
    return (torch.minimum(d.world_distance, d.self_distance) < 0).any(dim=1)


def run(batch=1024, steps=200, lr=0.02, device="cuda", verbose=True):
    model = DifferentiableFrankaPanda(device=device)
    geometry = geometry_of(model)
    q0 = _common.sample_states(model, batch, seed=0)[0]
    with torch.no_grad():
        goal = model.compute_forward_kinematics(_common.sample_states(model, batch, seed=1)[0], EE)[0]
        before = in_collision(model, q0, geometry)
    q = q0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        cost = model.compute_collision_cost(q, geometry, **ACTIVATION).cost
        err = model.compute_forward_kinematics(q, EE)[0] - goal
        (cost + 0.5 * GOAL_WEIGHT * (err * err).sum(dim=1)).sum().backward()
        opt.step()
    with torch.no_grad():
        qf = q.detach()
        after = in_collision(model, qf, geometry)
        cost = model.compute_collision_cost(qf, geometry, **ACTIVATION).cost
        miss = (model.compute_forward_kinematics(qf, EE)[0] - goal).norm(dim=1)
    stats = dict(before=before.float().mean().item(), after=after.float().mean().item(), cost=cost.mean().item(),
                 miss=miss.median().item(), spheres=geometry.n_spheres, pairs=geometry.n_pairs)
    if verbose:
        print("%d Pandas, %d spheres each, %d self pairs, 3 obstacles; %d Adam steps" % (batch, stats["spheres"], stats["pairs"], steps))
        print("postures in collision: %.1f %% before, %.1f %% after; mean collision cost %.4f; median end-effector miss %.3f m"
              % (100 * stats["before"], 100 * stats["after"], stats["cost"], stats["miss"]))
    return stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.steps, a.lr, device=a.device)

#!/usr/bin/env python3
"""Tip-over margin of a Fetch mobile manipulator swinging its arm: the zero-moment point from ONE compute_base_wrench call (one kernel
launch on the GPU) per batch of trajectory knots.

The wrench the floor has to apply to the base to keep it at rest is (force, moment) at the base origin; the point of the floor plane
z = 0 about which that wrench has no horizontal moment, the ZMP, is (-moment_y / force_z, moment_x / force_z).  The base stays flat on
the floor as long as the ZMP lies inside the support polygon of its wheels and casters, here a rectangle about the base origin; the
margin is the distance of the ZMP to the rectangle's nearest edge, negative once it has left it.  A seeded trajectory drives the torso
and the arm through sums of sines inside the joint limits, `--speed` scaling its rates; the same margin of the STATIC wrench (qd = qdd
= 0, where the ZMP is the ground projection of the centre of mass) shows how much of the loss is the motion's.

    python examples/zmp_margin_fetch.py [--knots 4096] [--batch 1024] [--speed 1.0] [--device cuda]
"""
import argparse
import contextlib
import io
import math
import os
import warnings

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableRobotModel
from differentiable_robot_model_amd.robot_model import robot_description_folder

SUPPORT = (0.20, 0.18)      # half extents of the support rectangle about the base origin along x and y [m]
HORIZON = 4.0               # seconds


def trajectory(model, knots, speed, seed=0):
    """(q, qd, qdd) [knots, n] of a sum of three sines per joint about the middle of its range, analytic rates"""
    lim = model.get_joint_limits()
    dev = model._device
    lo = torch.tensor([j["lower"] for j in lim], device=dev)
    hi = torch.tensor([j["upper"] for j in lim], device=dev)
    free = lo >= hi
    lo, hi = torch.where(free, torch.full_like(lo, -math.pi), lo), torch.where(free, torch.full_like(hi, math.pi), hi)
    gen = torch.Generator().manual_seed(seed)
    n = len(lim)
    amp = (torch.rand(3, n, generator=gen) / 3).to(dev) * 0.45 * (hi - lo)
    freq = (speed * 2 * math.pi * (0.2 + 0.8 * torch.rand(3, n, generator=gen))).to(dev)
    phase = (2 * math.pi * torch.rand(3, n, generator=gen)).to(dev)
    t = torch.linspace(0.0, HORIZON, knots, device=dev)[:, None, None]
    arg = freq * t + phase
    q = 0.5 * (lo + hi) + (amp * torch.sin(arg)).sum(1)
    qd = (amp * freq * torch.cos(arg)).sum(1)
    qdd = -(amp * freq * freq * torch.sin(arg)).sum(1)
    return q, qd, qdd


def zmp(wrench):
    """[B, 2]: the zero-moment point on z = 0 of a BaseWrench"""
    return torch.stack([-wrench.moment[:, 1], wrench.moment[:, 0]], dim=1) / wrench.force[:, 2:3]


def margin(point):
    """[B]: distance of a point [B, 2] to the nearest edge of the support rectangle, negative outside"""
    half = torch.tensor(SUPPORT, device=point.device)
    return (half - point.abs()).min(dim=1).values


def run(knots=4096, batch=1024, speed=1.0, device="cuda", verbose=True):
    """-> stats: the worst margin of the moving and of the static ZMP over the trajectory [m], and how far the static ZMP lies from the
    ground projection of the centre of mass (float32 rounding)."""
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = DifferentiableRobotModel(os.path.join(robot_description_folder, "fetch.urdf"), device=device)
    q, qd, qdd = trajectory(model, knots, speed)
    worst, worst_static, gap = math.inf, math.inf, 0.0
    with torch.no_grad():
        for i in range(0, knots, batch):
            s = slice(i, i + batch)
            moving = zmp(model.compute_base_wrench(q[s], qd[s], qdd[s]))
            static = zmp(model.compute_base_wrench(q[s]))
            com = model.compute_center_of_mass(q[s]).position
            worst = min(worst, margin(moving).min().item())
            worst_static = min(worst_static, margin(static).min().item())
            gap = max(gap, (static - com[:, :2]).abs().max().item())
    _common.sync(device)
    stats = dict(margin=worst, static_margin=worst_static, static_zmp_to_com=gap, mass=model.total_mass())
    if verbose:
        print("Fetch, %.1f kg, %d knots over %.1f s at speed %.2f, support rectangle +-%.2f m x +-%.2f m" % (
            stats["mass"], knots, HORIZON, speed, SUPPORT[0], SUPPORT[1]))
        print("worst ZMP margin %+.4f m; of the static wrench %+.4f m (the static ZMP is the CoM's ground projection to %.1e m)" % (
            worst, worst_static, gap))
    return stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--knots", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--speed", type=float, default=1.0)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.knots, a.batch, a.speed, a.device)

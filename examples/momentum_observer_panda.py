#!/usr/bin/env python3
"""A generalised-momentum observer on a batch of Franka Pandas: external joint torques (a collision, a payload) estimated without
acceleration measurements and without inverting H, from ONE call of compute_lagrangian_dynamics per tick (one kernel launch on the GPU).

With p = H(q) qd and dH/dt = C + C^T, the equations of motion H qdd + C qd + g = tau + tau_ext give

    pdot = tau + C^T qd - g + tau_ext,

so the residual  r <- K (p - int (tau + C^T qd - g + r) dt - p0)  follows tau_ext like a first-order filter, rdot = K (tau_ext - r).
That needs the Christoffel-consistent C itself: the product C qd, which compute_non_linear_effects returns, does not give C^T qd.

Every robot holds a posture under a PD law with gravity compensation, tau = Kp (q_ref - q) - Kd qd + g(q); a known torque step is
applied to one joint of every robot from `t_step` on, and the simulation (semi-implicit Euler through compute_forward_dynamics, the
non-linear model) is observed tick by tick.

    python examples/momentum_observer_panda.py [--batch 256] [--steps 600] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda


def run(batch=256, steps=600, dt=1e-3, gain=100.0, joint=3, torque=2.0, t_step=100, device="cuda", terms=None, verbose=True):
    """-> (r [batch, n] the residual after the last tick, stats).  ``terms(q, qd) -> (H, C, g)``: what the observer is fed; the
    default is model.compute_lagrangian_dynamics."""
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    lim = model.get_joint_limits()
    lower = torch.tensor([j["lower"] for j in lim], device=device)
    upper = torch.tensor([j["upper"] for j in lim], device=device)
    n = model._n_dofs
    terms = terms or model.compute_lagrangian_dynamics
    q_ref = lower + (upper - lower) * (0.25 + 0.5 * torch.rand(batch, n, device=device))
    q = q_ref + 0.05 * (2 * torch.rand(batch, n, device=device) - 1)
    qd = torch.zeros(batch, n, device=device)
    kp, kd = 100.0, 20.0
    tau_ext = torch.zeros(batch, n, device=device)
    # the observer's state in float64: an integral over many ticks
    integral = torch.zeros(batch, n, dtype=torch.float64, device=device)
    r = torch.zeros(batch, n, dtype=torch.float64, device=device)
    p0 = None
    with torch.no_grad():
        for k in range(steps):
            H, C, g = terms(q, qd)                                  # the tick's one call
            p = (H.double() @ qd.double()[..., None])[..., 0]
            if p0 is None:
                p0 = p
            r = gain * (p - integral - p0)
            tau = kp * (q_ref - q) - kd * qd + g.to(q.dtype)
            pdot_model = tau.double() + (C.double().transpose(1, 2) @ qd.double()[..., None])[..., 0] - g.double()
            integral = integral + dt * (pdot_model + r)
            if k == t_step:
                tau_ext[:, joint] = torque
            qdd = model.compute_forward_dynamics(q, qd, tau + tau_ext, include_gravity=True, use_damping=False)
            qd = qd + dt * qdd
            q = q + dt * qd
    want = tau_ext.double()
    err = (r - want).abs()
    stats = dict(worst=err.max().item(), on_joint=err[:, joint].max().item(), estimate=r[:, joint].mean().item(), torque=torque,
                 speed=qd.abs().max().item())
    if verbose:
        print("%d Pandas, %d ticks of %.1f ms, observer gain %.0f /s: %.2f N m on joint %d from tick %d -> estimated %.4f N m "
              "(worst error over all joints and robots %.2e N m)" % (batch, steps, 1e3 * dt, gain, torque, joint, t_step, stats["estimate"],
                                                                     stats["worst"]))
    return r, stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.steps, device=a.device)

#!/usr/bin/env python3
"""The energy budget of simulated Franka Pandas: how well compute_forward_dynamics_rollout conserves T + V, checked with ONE
compute_energy call (one kernel launch on the GPU) over all the states of a trajectory.

Without joint torques and without damping the total energy T(q, qd) + V(q) of a robot is constant, so its drift along a rollout is the
integrator's error and nothing else.  A batch of robots is released from random postures with random joint rates and simulated over
the same horizon at dt, dt / 2 and dt / 4 with both integrators; the states [T, B, n] are flattened to [T * B, n] and handed to
compute_energy at once.  Both integrators are first order: halving dt halves the drift.

The run closes with a torque-driven rollout and the power balance d(T + V)/dt = qd . tau: the energy gained over the horizon against
the work sum_t dt qd_{t+1} . tau_t the torques did on the joints.

    python examples/energy_budget_panda.py [--batch 256] [--horizon 0.2] [--dt 2e-3] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda

INTEGRATORS = ("semi_implicit_euler", "euler")


def total_energy(model, q_traj, qd_traj):
    """[T, B] float64: T + V of every state of a trajectory [T, B, n], from one compute_energy call on the flattened states"""
    steps, batch, n = q_traj.shape
    energy = model.compute_energy(q_traj.reshape(steps * batch, n), qd_traj.reshape(steps * batch, n))
    return (energy.kinetic.double() + energy.potential.double()).reshape(steps, batch)


def run(batch=256, horizon=0.2, dt=2e-3, device="cuda", verbose=True):
    """-> stats: drift[integrator] = [worst |E_t - E_0| over the robots and the horizon at dt, dt / 2, dt / 4] in joules, the scale of
    the energy, and the power balance of the torque-driven run."""
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    lim = model.get_joint_limits()
    lower = torch.tensor([j["lower"] for j in lim], device=device)
    upper = torch.tensor([j["upper"] for j in lim], device=device)
    n = model._n_dofs
    q0 = lower + (upper - lower) * (0.25 + 0.5 * torch.rand(batch, n, device=device))
    qd0 = 0.5 * (2 * torch.rand(batch, n, device=device) - 1)
    stats = dict(drift={}, dts=[dt, dt / 2, dt / 4])
    with torch.no_grad():
        e0 = total_energy(model, q0[None], qd0[None])[0]
        stats["kinetic"] = model.compute_energy(q0, qd0).kinetic.max().item()
        for integrator in INTEGRATORS:
            drifts = []
            for h in stats["dts"]:
                steps = int(round(horizon / h))
                tau = torch.zeros(steps, batch, n, device=device)
                q_traj, qd_traj = model.compute_forward_dynamics_rollout(q0, qd0, tau, h, integrator=integrator, include_gravity=True,
                                                                         use_damping=False)
                drifts.append((total_energy(model, q_traj, qd_traj) - e0[None]).abs().max().item())
            stats["drift"][integrator] = drifts
            if verbose:
                print("%-20s drift of T + V over %.2f s, worst of %d robots: %s J  (largest kinetic energy at release %.3f J)" % (
                    integrator, horizon, batch, "  ".join("dt=%.2g: %.3e" % (h, d) for h, d in zip(stats["dts"], drifts)), stats["kinetic"]))
        # power balance: slowly varying torques, dt / 4
        h = dt / 4
        steps = int(round(horizon / h))
        t = torch.arange(steps, device=device)[:, None, None] * h
        amp = 2.0 * (2 * torch.rand(batch, n, device=device) - 1)
        tau = amp[None] * torch.sin(2 * torch.pi * t / horizon)
        q_traj, qd_traj = model.compute_forward_dynamics_rollout(q0, qd0, tau, h, include_gravity=True, use_damping=False)
        gained = total_energy(model, q_traj[-1:], qd_traj[-1:])[0] - e0
        work = h * (qd_traj.double() * tau.double()).sum(dim=(0, 2))
        stats["work"] = work.abs().max().item()
        stats["balance"] = (gained - work).abs().max().item()
        if verbose:
            print("torque-driven run at dt=%.2g: E_end - E_0 against the work of the torques, worst of %d robots: %.3e J of up to %.3f J (the drift at this dt included)" % (
                h, batch, stats["balance"], stats["work"]))
    return stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=float, default=0.2)
    ap.add_argument("--dt", type=float, default=2e-3)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.horizon, a.dt, device=a.device)

#!/usr/bin/env python3
"""Inverse-dynamics trajectory optimisation on a batch of Franka Pandas: point-to-point motions of least squared torque, descended with
the ANALYTIC gradient from ONE call of compute_inverse_dynamics_derivatives per iteration (one kernel launch on the GPU for all knots
of all motions) instead of a backward pass through inverse dynamics.

Every motion goes from q_start to q_goal in `duration` seconds through K free knots Q_1 .. Q_K (Q_0 = q_start, Q_K+1 = q_goal fixed),
dt = duration / (K + 1) apart.  At the free knots

    qd_k = (Q_k+1 - Q_k-1) / (2 dt),     qdd_k = (Q_k+1 - 2 Q_k + Q_k-1) / dt^2,     tau_k = ID(Q_k, qd_k, qdd_k)

and the cost is J = sum_k |tau_k|^2.  With g_k = 2 tau_k the chain rule through the three matrices of the call gives

    dJ/dQ_k  =  dtau_dq_k^T g_k  -  2 H_k g_k / dt^2
              + (dtau_dqd_k-1^T g_k-1) / (2 dt) + H_k-1 g_k-1 / dt^2              (knot k is the "next" of knot k - 1)
              - (dtau_dqd_k+1^T g_k+1) / (2 dt) + H_k+1 g_k+1 / dt^2              (knot k is the "previous" of knot k + 1)

    python examples/inverse_dynamics_trajopt_panda.py [--batch 256] [--knots 8] [--iters 50] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda


def finite_differences(Q, dt):
    """Q [B, K + 2, n] -> (q, qd, qdd) [B, K, n] at the free knots."""
    return Q[:, 1:-1], (Q[:, 2:] - Q[:, :-2]) / (2 * dt), (Q[:, 2:] - 2 * Q[:, 1:-1] + Q[:, :-2]) / (dt * dt)


def cost_and_gradient(model, Q, dt):
    """-> (J [B], dJ/dQ_1..K [B, K, n]) from one compute_inverse_dynamics_derivatives call over all B K knots."""
    B, K2, n = Q.shape
    K = K2 - 2
    q, qd, qdd = (x.reshape(B * K, n) for x in finite_differences(Q, dt))
    out = model.compute_inverse_dynamics_derivatives(q, qd, qdd, include_gravity=True, use_damping=False)
    tau = out.tau.reshape(B, K, n)
    g = (2 * out.tau)[:, None, :]                                   # [B K, 1, n] row vectors: g^T M = (M^T g)^T
    gq = (g @ out.dtau_dq)[:, 0].reshape(B, K, n)
    gqd = (g @ out.dtau_dqd)[:, 0].reshape(B, K, n)
    gqdd = (g @ out.dtau_dqdd)[:, 0].reshape(B, K, n)
    grad = torch.zeros(B, K + 2, n, device=Q.device, dtype=Q.dtype)
    grad[:, 1:-1] += gq - 2 * gqdd / (dt * dt)
    grad[:, 2:] += gqd / (2 * dt) + gqdd / (dt * dt)
    grad[:, :-2] += -gqd / (2 * dt) + gqdd / (dt * dt)
    return (tau * tau).sum((1, 2)), grad[:, 1:-1]


def cost_and_gradient_by_autograd(model, Q, dt):
    """The same by a backward pass through compute_inverse_dynamics."""
    B, K2, n = Q.shape
    free = Q[:, 1:-1].detach().clone().requires_grad_(True)
    full = torch.cat([Q[:, :1], free, Q[:, -1:]], 1)
    q, qd, qdd = (x.reshape(-1, n) for x in finite_differences(full, dt))
    tau = model.compute_inverse_dynamics(q, qd, qdd, include_gravity=True, use_damping=False)
    J = (tau * tau).reshape(B, -1).sum(1)
    (grad,) = torch.autograd.grad(J.sum(), free)
    return J.detach(), grad


def run(batch=256, knots=8, iters=50, duration=2.0, device="cuda", verbose=True):
    """-> (costs [iters + 1, batch], Q [batch, knots + 2, n]): backtracking gradient descent on the free knots of every motion."""
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    lim = model.get_joint_limits()
    lower = torch.tensor([j["lower"] for j in lim], device=device)
    upper = torch.tensor([j["upper"] for j in lim], device=device)
    n = model._n_dofs
    span = upper - lower
    q_start = lower + span * (0.2 + 0.6 * torch.rand(batch, n, device=device))
    q_goal = lower + span * (0.2 + 0.6 * torch.rand(batch, n, device=device))
    dt = duration / (knots + 1)
    s = torch.linspace(0, 1, knots + 2, device=device)[None, :, None]
    Q = q_start[:, None] + s * (q_goal - q_start)[:, None]           # the straight line in joint space, sampled at the knots
    # ... bent, so that the start is not already smooth
    Q[:, 1:-1] += 0.1 * (2 * torch.rand(batch, knots, n, device=device) - 1)
    step = torch.full((batch, 1, 1), 1e-4, device=device)
    with torch.no_grad():
        J, grad = cost_and_gradient(model, Q, dt)
        costs = [J]
        for _ in range(iters):
            trial = Q.clone()
            trial[:, 1:-1] -= step * grad
            Jt, gt = cost_and_gradient(model, trial, dt)
            better = Jt < J                                          # per motion: take the step and lengthen it, or halve it
            Q = torch.where(better[:, None, None], trial, Q)
            grad = torch.where(better[:, None, None], gt, grad)
            J = torch.where(better, Jt, J)
            step = torch.where(better[:, None, None], step * 1.5, step * 0.5)
            costs.append(J)
    costs = torch.stack(costs)
    if verbose:
        print("%d motions of %d free knots, %d iterations: summed squared torque %.1f -> %.1f (N m)^2 on average, every motion's fell: %s"
              % (batch, knots, iters, costs[0].mean().item(), costs[-1].mean().item(), bool((costs[-1] < costs[0]).all())))
    return costs, Q


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--knots", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.knots, a.iters, device=a.device)

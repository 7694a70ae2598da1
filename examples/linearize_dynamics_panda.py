#!/usr/bin/env python3
"""LQR stabilisation of a batch of Franka Pandas about gravity-compensated postures, from ONE call of
compute_forward_dynamics_derivatives (one kernel launch on the GPU).  At the posture q*, at rest, under the torques f* = nle(q*, 0)
the call returns dqdd_dq, dqdd_dqd and minv = dqdd/df; with x = (q - q*, qd) and u = f - f* the semi-implicit Euler step

    qd+ = qd + dt qdd,   q+ = q + dt qd+      linearises to      x+ = A x + B u,

    A = [[I + dt^2 dqdd_dq,  dt (I + dt dqdd_dqd)],        B = [[dt^2 minv],
         [dt dqdd_dq,        I + dt dqdd_dqd     ]]             [dt minv  ]]

The Riccati recursion P <- Q + A^T P (A - B K), K = (R + B^T P B)^-1 B^T P A is iterated in torch (batched, float64) to the
stationary gain, and the loop u = -K x is closed step by step through compute_forward_dynamics, the non-linear model.

    python examples/linearize_dynamics_panda.py [--batch 256] [--steps 300] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import torch

from differentiable_robot_model_amd import DifferentiableFrankaPanda


def discrete_model(lin, dt):
    """(A [B, 2n, 2n], B [B, 2n, n]) of the semi-implicit Euler step from a ForwardDynamicsDerivatives, in float64."""
    aq, aqd, minv = lin.dqdd_dq.double(), lin.dqdd_dqd.double(), lin.minv.double()
    eye = torch.eye(aq.shape[-1], dtype=torch.float64, device=aq.device).expand_as(aq)
    top = torch.cat([eye + dt * dt * aq, dt * (eye + dt * aqd)], 2)
    bottom = torch.cat([dt * aq, eye + dt * aqd], 2)
    return torch.cat([top, bottom], 1), torch.cat([dt * dt * minv, dt * minv], 1)


def lqr_gain(A, B, Q, R, iterations):
    """The stationary gain K [B, n, 2n] of the discrete Riccati recursion."""
    P = Q.clone()
    for _ in range(iterations):
        BtP = B.transpose(1, 2) @ P
        K = torch.linalg.solve(R + BtP @ B, BtP @ A)
        P = Q + A.transpose(1, 2) @ P @ (A - B @ K)
        P = 0.5 * (P + P.transpose(1, 2))
    return K


def run(batch=256, steps=300, dt=5e-3, perturbation=0.05, riccati_iterations=400, use_gain=True, device="cuda", verbose=True):
    torch.manual_seed(0)
    model = DifferentiableFrankaPanda(device=device)
    lim = model.get_joint_limits()
    lower = torch.tensor([j["lower"] for j in lim], device=device)
    upper = torch.tensor([j["upper"] for j in lim], device=device)
    n = model._n_dofs
    # postures in the middle half of every joint's range, held against gravity
    q_ref = lower + (upper - lower) * (0.25 + 0.5 * torch.rand(batch, n, device=device))
    rest = torch.zeros(batch, n, device=device)
    with torch.no_grad():
        f_ref = model.compute_non_linear_effects(q_ref, rest, include_gravity=True, use_damping=True)
        lin = model.compute_forward_dynamics_derivatives(q_ref, rest, f_ref, include_gravity=True, use_damping=True)
        A, B = discrete_model(lin, dt)
        Q = torch.diag(torch.cat([torch.full((n,), 100.0), torch.ones(n)])).to(device=device, dtype=torch.float64).expand(batch, -1, -1)
        R = (0.01 * torch.eye(n, dtype=torch.float64, device=device)).expand(batch, -1, -1)
        K = lqr_gain(A, B, Q, R, riccati_iterations).float() if use_gain else torch.zeros(batch, n, 2 * n, device=device)
        q = q_ref + perturbation * (2 * torch.rand(batch, n, device=device) - 1)
        qd = rest.clone()
        start = torch.cat([q - q_ref, qd], 1).norm(dim=1)
        for _ in range(steps):
            x = torch.cat([q - q_ref, qd], 1)
            f = f_ref - (K @ x[..., None])[..., 0]
            qdd = model.compute_forward_dynamics(q, qd, f, include_gravity=True, use_damping=True)
            qd = qd + dt * qdd
            q = q + dt * qd
        end = torch.cat([q - q_ref, qd], 1).norm(dim=1)
    stats = dict(start=start.mean().item(), end=end.mean().item(), worst_ratio=(end / start).max().item(), best_ratio=(end / start).min().item(),
                 residual_acc=lin.qdd.abs().max().item())
    if verbose:
        print("%d Pandas, %d steps of %.1f ms, %s: mean state error %.3f -> %.2e (worst robot: %.3g of its initial error)"
              % (batch, steps, 1e3 * dt, "LQR from one linearisation" if use_gain else "no feedback", stats["start"], stats["end"],
                 stats["worst_ratio"]))
    return q, stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.batch, a.steps, device=a.device)
    run(a.batch, a.steps, use_gain=False, device=a.device)

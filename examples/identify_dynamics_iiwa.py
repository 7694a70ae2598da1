#!/usr/bin/env python3
"""Closed-form identification of the inertial parameters of a KUKA iiwa from sampled states and torques, from ONE call of
compute_inverse_dynamics_regressor per data set (one kernel launch on the GPU) — no training loop.  Inverse dynamics is linear in the
stacked per-body parameters phi = (m, m c, I_o): tau = Y(q, qd, qdd) phi.  The example

  * samples states (q uniform over the joint ranges, qd in +-1 rad/s, qdd in +-2 rad/s^2) and takes tau from compute_inverse_dynamics;
  * stacks the float32 Y of the training states into [B n, P] and solves the minimum-norm least squares for phi in float64 on the
    host (numpy.linalg.lstsq: the data determine only the base-parameter combinations, rank(Y) < P);
  * reports the torque error of the identified phi on held-out states and rank(Y) next to P = 10 Nb.

`regressor(model, q, qd, qdd)` -> [B, n, P] may be replaced (tests feed an fp64 truth rounded to float32 through the same solve).

    python examples/identify_dynamics_iiwa.py [--samples 4096] [--device cuda]
"""
import argparse

import _common  # noqa: F401
import numpy as np
import torch

from differentiable_robot_model_amd import DifferentiableKUKAiiwa


def sample(model, count, generator):
    lim = model.get_joint_limits()
    lower = torch.tensor([j["lower"] for j in lim])
    upper = torch.tensor([j["upper"] for j in lim])
    n = model._n_dofs
    q = lower + (upper - lower) * torch.rand(count, n, generator=generator)
    qd = 2 * torch.rand(count, n, generator=generator) - 1
    qdd = 4 * torch.rand(count, n, generator=generator) - 2
    return tuple(t.to(model._device) for t in (q, qd, qdd))


def default_regressor(model, q, qd, qdd):
    return model.compute_inverse_dynamics_regressor(q, qd, qdd, include_gravity=True, use_damping=False)


def run(samples=4096, held_out=None, device="cuda", regressor=default_regressor, verbose=True):
    model = DifferentiableKUKAiiwa(device=device)
    g = torch.Generator().manual_seed(0)
    held_out = held_out or max(samples // 4, 1)
    train, test = sample(model, samples, g), sample(model, held_out, g)
    with torch.no_grad():
        tau_train = model.compute_inverse_dynamics(*train, include_gravity=True, use_damping=False)
        tau_test = model.compute_inverse_dynamics(*test, include_gravity=True, use_damping=False)
    stack = lambda Y: np.asarray(Y.cpu() if isinstance(Y, torch.Tensor) else Y, np.float64).reshape(-1, Y.shape[-1])
    Y = stack(regressor(model, *train))
    # singular values below the rounding of the float32 Y (numpy.linalg.matrix_rank's rule at ITS precision) are null directions
    rcond = np.finfo(np.float32).eps * max(Y.shape)
    phi, _, rank, _ = np.linalg.lstsq(Y, tau_train.cpu().numpy().astype(np.float64).reshape(-1), rcond=rcond)
    want = tau_test.cpu().numpy().astype(np.float64)
    got = (stack(regressor(model, *test)) @ phi).reshape(want.shape)
    stats = dict(rank=int(rank), columns=Y.shape[1], bodies=len(model.regressor_links()),
                 held_out_error=float(np.abs(got - want).max() / np.abs(want).max()),
                 parameter_error=float(np.abs(phi - model.inertial_parameters().cpu().numpy()).max()))
    if verbose:
        print("iiwa, %d training and %d held-out states: rank(Y) = %d of P = 10 x %d = %d columns; held-out torque error %.2e of max|tau|"
              % (samples, held_out, stats["rank"], stats["bodies"], stats["columns"], stats["held_out_error"]))
        print("(the minimum-norm phi differs from the model's own by up to %.3g: only the %d base-parameter combinations are determined)"
              % (stats["parameter_error"], stats["rank"]))
    return (train, test), stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    run(a.samples, device=a.device)

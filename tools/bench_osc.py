#!/usr/bin/env python3
"""Operational-space dynamics (compute_operational_space_dynamics, csrc/drm_osc.hip) against the Python composition it replaces, on the
same seeded inputs (q uniform over the joint ranges, qd uniform in +-1 rad/s, regularization 0.1):

  call      compute_operational_space_dynamics as a user calls it: the fused kernel for 7-DoF arms whose last link is the target,
            the composed path (Jacobian, inertia-matrix and bias-torque kernels + a finish kernel) for every other robot
  composed  the same call with every row on the composed path (DRM_OSC_COMPOSED)
  python    compute_endeffector_jacobian, compute_lagrangian_inertia_matrix, compute_non_linear_effects, torch.linalg solves for
            H^-1 J^T, the m x m inverse, the products, and Jdot qd by a central difference of two more Jacobian calls — what a
            user writes today (the difference is the only way to Jdot qd there; in float32 it is good to about three digits)

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows —
host work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o osc -- python tools/bench_osc.py --trace robot:link:B[:composed]
    python tools/bench_osc.py --read DIR/.../osc_results.db --trace robot:link:B[:composed]

which adds up the dispatches of one call.  Bytes per row are what the algorithm needs (q and qd in, the four results out:
4 (2 n + m^2 + n m + 2 m)); the fraction of the HBM peak (8.0 TB/s) is those bytes over kernel time.

    python tools/bench_osc.py [--cases robot:link,...] [--sizes 4096,65536,1048576] [--reps 5] [--launches 20] [--no-python]
"""
import argparse
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from differentiable_robot_model_amd.robot_model import DifferentiableRobotModel, robot_description_folder  # noqa: E402

HBM_PEAK = 8.0e12
SIZES = (4096, 65536, 1 << 20)
# (robot, link, position only)
CASES = (("panda_no_gripper", "panda_virtual_ee_link", False), ("iiwa7", "iiwa_link_ee", False), ("fetch", "gripper_link", False),
         ("allegro_left", "link_3.0_tip", True))
RHO, WARMUP = 0.1, 3


def load(robot, device="cuda:0"):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DifferentiableRobotModel(os.path.join(robot_description_folder, robot + ".urdf"), device=device)


def inputs(m, B, seed):
    lim = m.get_joint_limits()
    lo = torch.tensor([j["lower"] for j in lim]); hi = torch.tensor([j["upper"] for j in lim])
    free = lo >= hi
    lo, hi = torch.where(free, -np.pi, lo), torch.where(free, np.pi, hi)
    g = torch.Generator().manual_seed(seed)
    q = lo + (hi - lo) * torch.rand(B, lo.shape[0], generator=g)
    qd = torch.rand(B, lo.shape[0], generator=g) * 2 - 1
    return q.to(m._device), qd.to(m._device)


def python_composition(m, link, q, qd, pos_only, rho=RHO, h=1e-3):
    """What the call replaces: three model calls, batched torch.linalg solves and a finite-difference Jdot qd (float32, so h = 1e-3)."""
    k = 3 if pos_only else 6
    lin, ang = m.compute_endeffector_jacobian(q, link)
    J = lin if pos_only else torch.cat([lin, ang], 1)
    H = m.compute_lagrangian_inertia_matrix(q)
    nle = m.compute_non_linear_effects(q, qd, include_gravity=True, use_damping=False)
    X = torch.linalg.solve_ex(H, J.transpose(1, 2))[0]          # (the _ex forms: no status check on the host, no synchronisation)
    lam = torch.linalg.inv_ex(J @ X + rho ** 2 * torch.eye(k, device=q.device))[0]
    jbar = X @ lam
    jp, jm = m.compute_endeffector_jacobian(q + h * qd, link), m.compute_endeffector_jacobian(q - h * qd, link)
    Jp, Jm = (jp[0], jm[0]) if pos_only else (torch.cat(jp, 1), torch.cat(jm, 1))
    acc = (((Jp - Jm) / (2 * h)) @ qd[..., None])[..., 0]
    eta = (lam @ ((X.transpose(1, 2) @ nle[..., None])[..., 0] - acc)[..., None])[..., 0]
    return lam, jbar, acc, eta


def timed(fn, reps, launches):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / launches)
    return float(np.median(times))


def row_bytes(n, k):
    return 4 * (2 * n + k * k + n * k + 2 * k)


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of one case and nothing else on the device."""
    parts = spec.split(":")
    robot, link, B, composed = parts[0], parts[1], int(parts[2]), parts[3:] == ["composed"]
    pos_only = dict((c[0], c[2]) for c in CASES).get(robot, False)
    m = load(robot)
    q, qd = inputs(m, B, B)
    for _ in range(WARMUP + launches):
        m.compute_operational_space_dynamics(q, qd, link, position_only=pos_only, regularization=RHO, _composed=composed)
    torch.cuda.synchronize()
    print("traced %s: %d + %d calls" % (spec, WARMUP, launches))


def read(db, spec, launches):
    """Kernel time of one call from the trace's rocpd database: every kernel name's dispatches per call, the mean of its timed
    dispatches (the warm-up calls' are left out), and their sum."""
    import re
    import sqlite3
    parts = spec.split(":")
    robot, B = parts[0], int(parts[2])
    pos_only = dict((c[0], c[2]) for c in CASES).get(robot, False)
    n = load(robot, None)._n_dofs
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    calls = WARMUP + launches
    by = {}
    for name, d in rows:
        by.setdefault(re.sub(r"\(.*", "", name), []).append(d)
    total = 0.0
    lines = []
    for name, ds in by.items():
        if len(ds) % calls or "drm" not in name:
            continue                                   # (not part of the calls: set-up work and copies of torch)
        per = len(ds) // calls
        mean = float(np.mean(ds[WARMUP * per:])) / 1e3
        total += per * mean
        lines.append("  %3d x %10.2f us  %s" % (per, mean, name))
    print("%s: %.2f us of kernel time per call" % (spec, total))
    by_row = row_bytes(n, 3 if pos_only else 6)
    print("  %d B per row -> %.3f TB/s, %.1f %% of the HBM peak" % (by_row, B * by_row / total / 1e6, 100 * B * by_row / (total * 1e-6) / HBM_PEAK))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:link[:pos],... (default: Panda, iiwa, Fetch, an Allegro fingertip)")
    ap.add_argument("--sizes", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-python", action="store_true", help="skip the Python composition")
    ap.add_argument("--trace", default=None, help="robot:link:B[:composed]: the profiled pass of one case")
    ap.add_argument("--read", default=None, help="the rocpd database of a --trace run")
    args = ap.parse_args()
    if args.read:
        return read(args.read, args.trace, args.launches)
    assert torch.cuda.is_available(), "bench_osc.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], c.split(":")[1], c.endswith(":pos")) for c in args.cases.split(",")]
    sizes = tuple(int(x) for x in args.sizes.split(",")) if args.sizes else SIZES
    print("%-17s %-22s %2s %8s %10s %12s %11s %8s %8s %6s %12s" % (
        "robot", "link", "m", "B", "call_us", "composed_us", "python_us", "x_python", "x_comp", "B/row", "call_rows/s"))
    for robot, link, pos_only in cases:
        m = load(robot)
        k = 3 if pos_only else 6
        for B in sizes:
            q, qd = inputs(m, B, B)
            with torch.no_grad():
                call = lambda: m.compute_operational_space_dynamics(q, qd, link, position_only=pos_only, regularization=RHO)  # noqa: E731
                t_call = timed(call, args.reps, args.launches)
                t_comp = timed(lambda: m.compute_operational_space_dynamics(q, qd, link, position_only=pos_only, regularization=RHO,
                                                                            _composed=True), args.reps, args.launches)
                t_py = float("nan")
                if not args.no_python:
                    t_py = timed(lambda: python_composition(m, link, q, qd, pos_only), args.reps, max(1, args.launches // 4))
            print("%-17s %-22s %2d %8d %10.1f %12.1f %11.1f %8.2f %8.2f %6d %12.3e" % (
                robot, link, k, B, t_call, t_comp, t_py, t_py / t_call, t_comp / t_call, row_bytes(m._n_dofs, k), B / (t_call * 1e-6)),
                flush=True)
            del q, qd
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

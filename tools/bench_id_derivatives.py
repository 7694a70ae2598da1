#!/usr/bin/env python3
"""tau, dtau/dq, dtau/dqd and H in one call (compute_inverse_dynamics_derivatives, csrc/drm_idd.hip) against the composition it
replaces, on the same seeded inputs (q uniform over the joint ranges, qd uniform in +-1 rad/s, qdd uniform in +-2 rad/s^2):

  call         compute_inverse_dynamics_derivatives as a user calls it: the fused kernel for 7-DoF arms, the general kernel otherwise
  general      the same with every row in the general kernel (DRM_IDD_COMPOSED: memsets of the three matrices + the kernel)
  composition  what a user writes today: n backward passes through compute_inverse_dynamics with one-hot cotangents (rows of dtau/dq
               and dtau/dqd) plus compute_lagrangian_inertia_matrix.  Its matrices are also compared with the call's
               (max|d| / max|.|: the two agree).
  fdd          compute_forward_dynamics_derivatives at f = the call's tau, in the same run: it moves the same bytes and does n reverse
               sweeps, a factorisation and 3 n solves on top

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows —
host work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o idd -- python tools/bench_id_derivatives.py --trace robot:B[:general][:fdd]
    python tools/bench_id_derivatives.py --read DIR/.../idd_results.db --trace robot:B[:general][:fdd]

which adds up the dispatches of one call; with `:fdd` the forward-dynamics-derivatives call runs in the same process, alternating with
the call, and its kernels are listed beside it.  Bytes per row are what the algorithm needs (q, qd and qdd in, tau and three matrices
out: 12 n + 4 (3 n^2 + n), 700 B for a 7-DoF arm); the share of the byte floor is those bytes at the HBM peak (8.0 TB/s) over the time.

    python tools/bench_id_derivatives.py [--cases robot:B,...] [--reps 5] [--launches 20] [--no-composition]
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
CASES = (("panda_no_gripper", 4096), ("panda_no_gripper", 65536), ("panda_no_gripper", 1 << 20), ("fetch", 65536), ("allegro_left", 65536))
WARMUP = 3


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
    n = lo.shape[0]
    q = (lo + (hi - lo) * torch.rand(B, n, generator=g)).to(m._device)
    qd = (torch.rand(B, n, generator=g) * 2 - 1).to(m._device)
    qdd = (torch.rand(B, n, generator=g) * 4 - 2).to(m._device)
    return q, qd, qdd


def composition(m, q, qd, qdd):
    """(tau, dtau_dq, dtau_dqd, H) the way it is written without the call."""
    q, qd = q.detach().requires_grad_(True), qd.detach().requires_grad_(True)
    tau = m.compute_inverse_dynamics(q, qd, qdd, include_gravity=True, use_damping=False)
    n = q.shape[1]
    rows = [torch.autograd.grad(tau[:, i].sum(), (q, qd), retain_graph=i + 1 < n) for i in range(n)]
    H = m.compute_lagrangian_inertia_matrix(q.detach())
    return tau.detach(), torch.stack([r[0] for r in rows], 1), torch.stack([r[1] for r in rows], 1), H


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


def row_bytes(n):
    return 12 * n + 4 * (3 * n * n + n)


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of one case (and, with :fdd, as many forward-dynamics-derivatives calls,
    alternating) and nothing else on the device."""
    parts = spec.split(":")
    robot, B = parts[0], int(parts[1])
    m = load(robot)
    q, qd, qdd = inputs(m, B, B)
    general, fdd = "general" in parts[2:], "fdd" in parts[2:]
    f = m.compute_inverse_dynamics(q, qd, qdd, include_gravity=True, use_damping=False) if fdd else None
    torch.cuda.synchronize()
    for _ in range(WARMUP + launches):
        m.compute_inverse_dynamics_derivatives(q, qd, qdd, _composed=general)
        if fdd:
            m.compute_forward_dynamics_derivatives(q, qd, f)
    torch.cuda.synchronize()
    print("traced %s: %d + %d calls" % (spec, WARMUP, launches))


def read(db, spec, launches):
    """Kernel time of one call from the trace's rocpd database: every kernel name's dispatches per call, the mean of its timed
    dispatches (the warm-up calls' are left out), and their sum; the forward-dynamics-derivatives kernels of a :fdd run apart."""
    import re
    import sqlite3
    parts = spec.split(":")
    robot, B = parts[0], int(parts[1])
    n = load(robot, None)._n_dofs
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    calls = WARMUP + launches
    by = {}
    for name, d in rows:
        by.setdefault(re.sub(r"\(.*", "", name), []).append(d)
    total, other = 0.0, 0.0
    lines, others = [], []
    for name, ds in by.items():
        if len(ds) % calls or not ("drm" in name or "fill" in name.lower() or "memset" in name.lower()):
            continue                                   # (not part of the calls: set-up work and copies of torch)
        per = len(ds) // calls
        mean = float(np.mean(ds[WARMUP * per:])) / 1e3
        line = "  %3d x %10.2f us  %s" % (per, mean, name)
        if "drm" in name and "rnea_derivatives" not in name:     # (a :fdd run: the other call's kernels, its forward-dynamics launch included)
            other += per * mean
            others.append(line)
        else:
            total += per * mean
            lines.append(line)
    print("%s: %.2f us of kernel time per call" % (spec, total))
    by_row = row_bytes(n)
    floor = B * by_row / HBM_PEAK * 1e6
    print("  %d B per row: byte floor %.1f us at 8 TB/s -> %.3f TB/s, %.1f %% of the HBM peak" % (by_row, floor, B * by_row / total / 1e6,
                                                                                                    100 * floor / total))
    print("\n".join(lines))
    if others:
        print("  compute_forward_dynamics_derivatives in the same run: %.2f us of kernel time per call (%.2fx)" % (other, other / total))
        print("\n".join(others))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:B,... (default: Panda at 4 096, 65 536 and 2^20 rows, Fetch and Allegro at 65 536)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-composition", action="store_true", help="skip the n backward passes")
    ap.add_argument("--trace", default=None, help="robot:B[:general][:fdd]: the profiled pass of one case")
    ap.add_argument("--read", default=None, help="the rocpd database of a --trace run")
    args = ap.parse_args()
    if args.read:
        return read(args.read, args.trace, args.launches)
    assert torch.cuda.is_available(), "bench_id_derivatives.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    print("%-17s %2s %8s %9s %10s %9s %14s %8s %9s %9s %6s %7s" % (
        "robot", "n", "B", "call_us", "general_us", "fdd_us", "composition_us", "x_compn", "d(dq)", "d(dqd)", "B/row", "floor%"))
    models = {}
    for robot, B in cases:
        m = models.get(robot) or models.setdefault(robot, load(robot))
        q, qd, qdd = inputs(m, B, B)
        n = m._n_dofs
        f = m.compute_inverse_dynamics(q, qd, qdd, include_gravity=True, use_damping=False)
        t = {general: timed(lambda: m.compute_inverse_dynamics_derivatives(q, qd, qdd, _composed=general), args.reps, args.launches)
             for general in (False, True)}                # (the two paths alternate per case, not per run of the script)
        t_fdd = timed(lambda: m.compute_forward_dynamics_derivatives(q, qd, f), args.reps, args.launches)
        t_py, d_dq, d_dqd = float("nan"), float("nan"), float("nan")
        if not args.no_composition:
            comp = composition(m, q, qd, qdd)
            out = m.compute_inverse_dynamics_derivatives(q, qd, qdd)
            d_dq = float((comp[1] - out.dtau_dq).abs().max() / out.dtau_dq.abs().max())
            d_dqd = float((comp[2] - out.dtau_dqd).abs().max() / out.dtau_dqd.abs().max())
            del comp, out
            t_py = timed(lambda: composition(m, q, qd, qdd), min(args.reps, 3), 1)
        floor = B * row_bytes(n) / HBM_PEAK * 1e6
        print("%-17s %2d %8d %9.1f %10.1f %9.1f %14.1f %8.2f %9.1e %9.1e %6d %7.1f" % (
            robot, n, B, t[False], t[True], t_fdd, t_py, t_py / t[False], d_dq, d_dqd, row_bytes(n), 100 * floor / t[False]), flush=True)
        del q, qd, qdd, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

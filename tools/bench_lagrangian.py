#!/usr/bin/env python3
"""H, C and g in one call (compute_lagrangian_dynamics / compute_coriolis_matrix, csrc/drm_lagrangian.hip) against the composition it
replaces, on the same seeded inputs (q uniform over the joint ranges, qd uniform in +-1 rad/s):

  call         compute_lagrangian_dynamics as a user calls it: the fused kernel for 7-DoF arms, the general kernel otherwise
  c_only       compute_coriolis_matrix: the same launch, H and g neither formed (arms) nor written
  general      compute_lagrangian_dynamics with every row in the general kernel (DRM_LAGRANGIAN_COMPOSED: memsets of H and C + the kernel)
  gen_c_only   compute_coriolis_matrix that way
  composition  what a user writes today: dH/dq by autograd with one-hot cotangents over the upper triangle of
               compute_lagrangian_inertia_matrix (n (n + 1) / 2 backward passes), the einsum to the Christoffel matrix and one
               compute_inverse_dynamics(q, 0, 0).  Its C is also compared with the call's (max|dC| / max|C|: the two agree).

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows —
host work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o lag -- python tools/bench_lagrangian.py --trace robot:B[:general][:conly]
    python tools/bench_lagrangian.py --read DIR/.../lag_results.db --trace robot:B[:general][:conly]

which adds up the dispatches of one call.  Bytes per row are what the algorithm needs (q and qd in, H, C and g out: 8 n + 4 (2 n^2 + n),
476 B for a 7-DoF arm; C alone 8 n + 4 n^2); the share of the byte floor is those bytes at the HBM peak (8.0 TB/s) over the time.

    python tools/bench_lagrangian.py [--cases robot:B,...] [--reps 5] [--launches 20] [--no-composition]
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
    return q, qd


def composition(m, q, qd):
    """(H, C, g) the way it is written without the call."""
    q = q.detach().requires_grad_(True)
    H = m.compute_lagrangian_inertia_matrix(q)
    B, n = q.shape
    D = torch.empty(B, n, n, n, device=q.device)                   # D[b, i, j, k] = dH_ij / dq_k
    for i in range(n):
        for j in range(i, n):
            (gq,) = torch.autograd.grad(H[:, i, j].sum(), q, retain_graph=True)
            D[:, i, j] = gq
            D[:, j, i] = gq
    G = 0.5 * (D + D.transpose(2, 3) - D.permute(0, 3, 1, 2))      # D[i, j, k] + D[i, k, j] - D[j, k, i]
    C = torch.einsum("bijk,bk->bij", G, qd)
    z = torch.zeros_like(qd)
    g = m.compute_inverse_dynamics(q.detach(), z, z, include_gravity=True, use_damping=False)
    return H.detach(), C, g


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


def row_bytes(n, c_only=False):
    return 8 * n + 4 * (n * n if c_only else 2 * n * n + n)


def call_of(m, q, qd, general, c_only):
    if not c_only:
        return lambda: m.compute_lagrangian_dynamics(q, qd, _composed=general)
    return lambda: m.compute_coriolis_matrix(q, qd)        # (the general kernel through DRM_LAGRANGIAN_COMPOSED=1: set by the caller)


@contextlib.contextmanager
def general_env(on):
    if on:
        os.environ["DRM_LAGRANGIAN_COMPOSED"] = "1"
    try:
        yield
    finally:
        os.environ.pop("DRM_LAGRANGIAN_COMPOSED", None)


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of one case and nothing else on the device."""
    parts = spec.split(":")
    robot, B = parts[0], int(parts[1])
    m = load(robot)
    q, qd = inputs(m, B, B)
    torch.cuda.synchronize()
    general = "general" in parts[2:]
    with general_env(general):
        fn = call_of(m, q, qd, general, "conly" in parts[2:])
        for _ in range(WARMUP + launches):
            fn()
        torch.cuda.synchronize()
    print("traced %s: %d + %d calls" % (spec, WARMUP, launches))


def read(db, spec, launches):
    """Kernel time of one call from the trace's rocpd database: every kernel name's dispatches per call, the mean of its timed
    dispatches (the warm-up calls' are left out), and their sum."""
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
    total = 0.0
    lines = []
    for name, ds in by.items():
        if len(ds) % calls or not ("drm" in name or "fill" in name.lower() or "memset" in name.lower()):
            continue                                   # (not part of the calls: set-up work and copies of torch)
        per = len(ds) // calls
        mean = float(np.mean(ds[WARMUP * per:])) / 1e3
        total += per * mean
        lines.append("  %3d x %10.2f us  %s" % (per, mean, name))
    print("%s: %.2f us of kernel time per call" % (spec, total))
    by_row = row_bytes(n, "conly" in parts[2:])
    floor = B * by_row / HBM_PEAK * 1e6
    print("  %d B per row: byte floor %.1f us at 8 TB/s -> %.3f TB/s, %.1f %% of the HBM peak" % (by_row, floor, B * by_row / total / 1e6,
                                                                                                    100 * floor / total))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:B,... (default: Panda at 4 096, 65 536 and 2^20 rows, Fetch and Allegro at 65 536)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-composition", action="store_true", help="skip the n (n + 1) / 2 backward passes")
    ap.add_argument("--trace", default=None, help="robot:B[:general][:conly]: the profiled pass of one case")
    ap.add_argument("--read", default=None, help="the rocpd database of a --trace run")
    args = ap.parse_args()
    if args.read:
        return read(args.read, args.trace, args.launches)
    assert torch.cuda.is_available(), "bench_lagrangian.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    print("%-17s %2s %8s %9s %9s %10s %10s %14s %8s %9s %6s %7s" % (
        "robot", "n", "B", "call_us", "c_only_us", "general_us", "gen_c_only", "composition_us", "x_compn", "dC/C", "B/row", "floor%"))
    models = {}
    for robot, B in cases:
        m = models.get(robot) or models.setdefault(robot, load(robot))
        q, qd = inputs(m, B, B)
        n = m._n_dofs
        t = {}
        for general in (False, True):                 # (the two paths alternate per case, not per run of the script)
            with general_env(general):
                for c_only in (False, True):
                    t[general, c_only] = timed(call_of(m, q, qd, general, c_only), args.reps, args.launches)
        t_py, dC = float("nan"), float("nan")
        if not args.no_composition:
            _, Cc, _ = composition(m, q, qd)
            C = m.compute_coriolis_matrix(q, qd)
            dC = float((Cc - C).abs().max() / C.abs().max())
            del Cc, C
            t_py = timed(lambda: composition(m, q, qd), min(args.reps, 3), 1)
        floor = B * row_bytes(n) / HBM_PEAK * 1e6
        print("%-17s %2d %8d %9.1f %9.1f %10.1f %10.1f %14.1f %8.2f %9.1e %6d %7.1f" % (
            robot, n, B, t[False, False], t[False, True], t[True, False], t[True, True], t_py, t_py / t[False, False], dC, row_bytes(n),
            100 * floor / t[False, False]), flush=True)
        del q, qd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

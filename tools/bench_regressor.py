#!/usr/bin/env python3
"""The inverse-dynamics regressor (compute_inverse_dynamics_regressor, csrc/drm_regressor.hip) against the composition it replaces, on
the same seeded inputs (q uniform over the joint ranges, qd uniform in +-1 rad/s, qdd uniform in +-2 rad/s^2, gravity on, no damping
columns):

  call         compute_inverse_dynamics_regressor as a user calls it: the fused kernel for 7-DoF arms, the general kernel otherwise
  general      the same call with every row in the general kernel (DRM_REGRESSOR_COMPOSED: one memset of Y, then the kernel)
  composition  what a user writes today: 10 Nb inverse-dynamics launches on unit-parameter copies of the walk table (what
               compute_inverse_dynamics of 10 Nb unit-parameter models launches) and one torch.stack into [B, n, 10 Nb]

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows —
host work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o reg -- python tools/bench_regressor.py --trace robot:B[:general]
    python tools/bench_regressor.py --read DIR/.../reg_results.db --trace robot:B[:general]

which adds up the dispatches of one call.  Bytes per row are what the algorithm needs (q, qd and qdd in, Y out: 12 n + 4 n P, 2 044 B
for a 7-DoF arm); the share of the byte floor is those bytes at the HBM peak (8.0 TB/s) over the time.

    python tools/bench_regressor.py [--cases robot:B,...] [--reps 5] [--launches 20] [--no-composition]
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
from differentiable_robot_model_amd import backend  # noqa: E402
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


def unit_tables(m):
    """The 10 Nb walk tables of the unit-parameter robots: every op massless but one, which carries one unit parameter."""
    dw = m._dynamics_walk()
    base = m._ops_f(dw).detach().clone()
    base[:, 12:25] = 0.0
    at = [12, 13, 14, 15, (16,), (17, 19), (18, 22), (20,), (21, 23), (24,)]
    tables = []
    for k in range(dw.program.n_ops):
        for e in at:
            t = base.clone()
            t[k, list(e) if isinstance(e, tuple) else e] = 1.0
            tables.append(t)
    return dw, tables


def composition(m, dw, tables, q, qd, qdd):
    cols = [backend.rnea(dw.program, t, dw.ops_i, q, qd, qdd, True, False, m._n_dofs) for t in tables]
    return torch.stack(cols, 2)


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


def row_bytes(n, P):
    return 12 * n + 4 * n * P


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of one case and nothing else on the device."""
    parts = spec.split(":")
    robot, B = parts[0], int(parts[1])
    m = load(robot)
    q, qd, qdd = inputs(m, B, B)
    torch.cuda.synchronize()
    for _ in range(WARMUP + launches):
        m.compute_inverse_dynamics_regressor(q, qd, qdd, True, False, _composed="general" in parts[2:])
    torch.cuda.synchronize()
    print("traced %s: %d + %d calls" % (spec, WARMUP, launches))


def read(db, spec, launches):
    """Kernel time of one call from the trace's rocpd database: every kernel name's dispatches per call, the mean of its timed
    dispatches (the warm-up calls' are left out), and their sum."""
    import re
    import sqlite3
    parts = spec.split(":")
    robot, B = parts[0], int(parts[1])
    m = load(robot, None)
    n, P = m._n_dofs, 10 * len(m.regressor_links())
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
    by_row = row_bytes(n, P)
    floor = B * by_row / HBM_PEAK * 1e6
    print("  %d B per row: byte floor %.1f us at 8 TB/s -> %.3f TB/s, %.1f %% of the HBM peak" % (by_row, floor, B * by_row / total / 1e6,
                                                                                                    100 * floor / total))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:B,... (default: Panda at 4 096, 65 536 and 2^20 rows, Fetch and Allegro at 65 536)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-composition", action="store_true", help="skip the 10 Nb inverse-dynamics launches")
    ap.add_argument("--trace", default=None, help="robot:B[:general]: the profiled pass of one case")
    ap.add_argument("--read", default=None, help="the rocpd database of a --trace run")
    args = ap.parse_args()
    if args.read:
        return read(args.read, args.trace, args.launches)
    assert torch.cuda.is_available(), "bench_regressor.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    print("%-17s %2s %4s %8s %10s %10s %15s %8s %7s %7s" % (
        "robot", "n", "P", "B", "call_us", "general_us", "composition_us", "x_compn", "B/row", "floor%"))
    models = {}
    for robot, B in cases:
        m = models.get(robot) or models.setdefault(robot, load(robot))
        q, qd, qdd = inputs(m, B, B)
        n, P = m._n_dofs, 10 * len(m.regressor_links())
        run = lambda **kw: timed(lambda: m.compute_inverse_dynamics_regressor(q, qd, qdd, True, False, **kw), args.reps, args.launches)
        t_call, t_gen = run(), run(_composed=True)
        t_py = float("nan")
        if not args.no_composition:
            dw, tables = unit_tables(m)
            t_py = timed(lambda: composition(m, dw, tables, q, qd, qdd), args.reps, max(1, args.launches // 10))
            del tables
        floor = B * row_bytes(n, P) / HBM_PEAK * 1e6
        print("%-17s %2d %4d %8d %10.1f %10.1f %15.1f %8.2f %7d %7.1f" % (
            robot, n, P, B, t_call, t_gen, t_py, t_py / t_call, row_bytes(n, P), 100 * floor / t_call), flush=True)
        del q, qd, qdd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

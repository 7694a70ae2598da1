#!/usr/bin/env python3
"""T, V, p = H qd, dT/dq and g in one call (compute_energy_derivatives / compute_energy / compute_generalized_momentum,
csrc/drm_energy.hip) against its neighbours and the composition it replaces, on the same seeded inputs (q uniform over the joint
ranges, qd uniform in +-1 rad/s):

  call         compute_energy_derivatives as a user calls it: the fused kernel for 7-DoF arms, the general kernel otherwise
  tv_only      compute_energy without grad: the same launch, T and V alone (arms: no sweep back)
  general      compute_energy_derivatives with every row in the general kernel (DRM_ENERGY_COMPOSED)
  lagrangian   compute_lagrangian_dynamics (H, C, g: 420 B out per row of a 7-DoF arm)
  inv_dyn      compute_inverse_dynamics(q, qd, 0) with the LIBRARY kernels (own_kernels = "off")
  composition  what a user writes today: compute_lagrangian_dynamics, p = H qd, dT/dq = C^T qd, T = qd . p / 2, and V from
               compute_forward_kinematics_all_links with the mass-weighted sum of the centre-of-mass heights over the links a joint
               moves.  Its outputs are also compared with the call's (the worst max|d| / max|.| of the five: the two agree).

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows —
host work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o energy -- python tools/bench_energy.py --trace robot:B
    python tools/bench_energy.py --read DIR/.../energy_results.db --trace robot:B

in which ONE process makes the energy calls, the T-and-V-only calls, the Lagrangian calls and the library inverse-dynamics calls of
the case, so the kernels are compared within one run; --read adds up the dispatches of one call of each.  Bytes per row are what the
algorithm needs (q and qd in, T, V, p, dT/dq and g out: 8 n + 4 (2 + 3 n), 148 B for a 7-DoF arm); the share of the byte floor is
those bytes at the HBM peak (8.0 TB/s) over the time.

    python tools/bench_energy.py [--cases robot:B,...] [--reps 5] [--launches 20]
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
from differentiable_robot_model_amd.autograd import _rot_from_quat  # noqa: E402
from differentiable_robot_model_amd.robot_model import DifferentiableRobotModel, robot_description_folder  # noqa: E402

HBM_PEAK = 8.0e12
CASES = (("panda_no_gripper", 4096), ("panda_no_gripper", 65536), ("panda_no_gripper", 1 << 20), ("fetch", 65536), ("allegro_left", 65536))
WARMUP = 3
GROUPS = (("lagrangian", "lagrangian_"), ("inverse dynamics", "rnea"))   # (the energy kernels are told apart by their order)


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


def moved_masses(m):
    """[(link name, mass, com)] of the links that at least one joint moves"""
    spec = m._spec
    return [(spec.link_names[i], float(spec.mass[i]), torch.from_numpy(spec.com[i].copy()).to(m._device))
            for i in range(1, len(spec.parent)) if spec.mass[i] > 0 and any(spec.dof[j] >= 0 for j in spec.chain_to(i))]


def composition(m, q, qd, bodies):
    """(T, V, p, dT/dq, g) the way it is written without the call."""
    lag = m.compute_lagrangian_dynamics(q, qd)
    p = torch.einsum("bij,bj->bi", lag.inertia, qd)
    dT = torch.einsum("bji,bj->bi", lag.coriolis, qd)
    T = 0.5 * (p * qd).sum(-1)
    poses = m.compute_forward_kinematics_all_links(q)
    V = torch.zeros_like(T)
    for name, mass, com in bodies:
        pos, quat = poses[name]
        Rz = _rot_from_quat(quat)[:, 6:9]                          # the third row of R: z of R c
        V = V + (9.81 * mass) * (pos[:, 2] + (Rz * com).sum(-1))
    return T, V, p, dT, lag.gravity


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
    return 8 * n + 4 * (2 + 3 * n)


def library_inverse_dynamics(m, q, qd):
    """compute_inverse_dynamics(q, qd, 0) on the library kernels, whatever kernels of its own the robot carries"""
    z = torch.zeros_like(q)

    def fn():
        keep = m.own_kernels
        m.own_kernels = "off"
        try:
            return m.compute_inverse_dynamics(q, qd, z, include_gravity=True, use_damping=False)
        finally:
            m.own_kernels = keep
    return fn


def calls_of(m, q, qd):
    return (("energy", lambda: m.compute_energy_derivatives(q, qd)), ("tv_only", lambda: m.compute_energy(q, qd)),
            ("lagrangian", lambda: m.compute_lagrangian_dynamics(q, qd)), ("inv_dyn", library_inverse_dynamics(m, q, qd)))


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of each entry point of one case, one after the other, and nothing else."""
    robot, B = spec.split(":")[0], int(spec.split(":")[1])
    m = load(robot)
    q, qd = inputs(m, B, B)
    torch.cuda.synchronize()
    with torch.no_grad():
        for _, fn in calls_of(m, q, qd):
            for _ in range(WARMUP + launches):
                fn()
            torch.cuda.synchronize()
    print("traced %s: %d + %d calls of each entry point" % (spec, WARMUP, launches))


def read(db, spec, launches):
    """Kernel time of one call of each entry point from the trace's rocpd database: every kernel name's dispatches per call, the mean
    of its timed dispatches (the warm-up calls' are left out), and their sum per group."""
    import re
    import sqlite3
    robot, B = spec.split(":")[0], int(spec.split(":")[1])
    n = load(robot, None)._n_dofs
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    calls = WARMUP + launches
    by = {}
    for name, d in rows:
        by.setdefault(re.sub(r"\(.*", "", name), []).append(d)

    def mean_us(ds, per):
        return float(np.mean(ds[WARMUP * per:])) / 1e3

    # the energy kernels: the first `calls` dispatches are the calls for all five outputs, the next `calls` those for T and V alone
    # (one kernel per call at the batch sizes of a multiple of 64 this tool takes; the general kernel serves both under one name)
    en = [(re.sub(r"\(.*", "", name), d) for name, d in rows if "drm" in name and "energy_" in name]
    assert len(en) == 2 * calls, "expected one energy kernel per call (%d dispatches, %d calls)" % (len(en), 2 * calls)
    t_all, t_tv = mean_us([d for _, d in en[:calls]], 1), mean_us([d for _, d in en[calls:]], 1)
    print("%s: energy" % spec)
    print("    1 x %10.2f us  %s   (T, V, p, dT/dq, g)" % (t_all, en[0][0]))
    print("    1 x %10.2f us  %s   (T and V alone)" % (t_tv, en[calls][0]))
    t_other = {}
    for group, key in GROUPS:
        print("%s: %s" % (spec, group))
        total = 0.0
        for name, ds in by.items():
            if key not in name or "drm" not in name or len(ds) % calls:
                continue
            per = len(ds) // calls
            total += per * mean_us(ds, per)
            print("  %3d x %10.2f us  %s" % (per, mean_us(ds, per), name))
        t_other[group] = total
    floor = B * row_bytes(n) / HBM_PEAK * 1e6
    lag = t_other["lagrangian"]
    print("  energy %.2f us against lagrangian %.2f us (%.2fx) and inverse dynamics %.2f us;  %d B per row: byte floor %.2f us at 8 TB/s -> "
          "%.3f TB/s, %.1f %% of the HBM peak" % (t_all, lag, lag / t_all, t_other["inverse dynamics"], row_bytes(n), floor,
                                                   B * row_bytes(n) / t_all / 1e6, 100 * floor / t_all))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:B,... (default: Panda at 4 096, 65 536 and 2^20 rows, Fetch and Allegro at 65 536)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--trace", default=None, help="robot:B: the profiled pass of one case")
    ap.add_argument("--read", default=None, help="the rocpd database of a --trace run")
    args = ap.parse_args()
    if args.read:
        return read(args.read, args.trace, args.launches)
    assert torch.cuda.is_available(), "bench_energy.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    print("%-17s %2s %8s %9s %10s %10s %13s %10s %14s %8s %9s %6s %7s" % (
        "robot", "n", "B", "call_us", "tv_only_us", "general_us", "lagrangian_us", "inv_dyn_us", "composition_us", "x_compn", "d/max", "B/row",
        "floor%"))
    models = {}
    for robot, B in cases:
        m = models.get(robot) or models.setdefault(robot, load(robot))
        bodies = moved_masses(m)
        q, qd = inputs(m, B, B)
        n = m._n_dofs
        with torch.no_grad():
            t = {name: timed(fn, args.reps, args.launches) for name, fn in calls_of(m, q, qd)}
            t["general"] = timed(lambda: m.compute_energy_derivatives(q, qd, _composed=True), args.reps, args.launches)
            got, ref = m.compute_energy_derivatives(q, qd), composition(m, q, qd, bodies)
            diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(got, ref))
            del got, ref
            t_py = timed(lambda: composition(m, q, qd, bodies), args.reps, args.launches)
        floor = B * row_bytes(n) / HBM_PEAK * 1e6
        print("%-17s %2d %8d %9.1f %10.1f %10.1f %13.1f %10.1f %14.1f %8.2f %9.1e %6d %7.1f" % (
            robot, n, B, t["energy"], t["tv_only"], t["general"], t["lagrangian"], t["inv_dyn"], t_py, t_py / t["energy"], diff,
            row_bytes(n), 100 * floor / t["energy"]), flush=True)
        del q, qd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

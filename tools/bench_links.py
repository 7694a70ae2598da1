#!/usr/bin/env python3
"""Link motion and external-wrench torques in one call each (compute_link_motion / compute_link_velocities /
compute_external_torques, csrc/drm_links.hip) against the general kernels on the same rows and the composition they replace, on the
same seeded inputs (q uniform over the joint ranges, qd and qdd uniform in +-1, unit-normal wrenches), on every link of the robot but
the root, named in the walk's own (pre-)order so that the results are the kernels' outputs as they stand (with link_names=None the
root's column of zeros is put in front by one more copy of every output):

  motion        compute_link_motion(q, qd, qdd): all five outputs; the fused kernel for a 7-DoF arm's full tiles, the general one otherwise
  velocities    compute_link_velocities(q, qd): the same launch, the two velocity arrays alone
  torques       compute_external_torques(q, forces, torques)
  *_general     the same calls with every row in the general kernel (DRM_LINKS_COMPOSED)
  vel_compn     what a user writes today for the velocities: per link one compute_endeffector_jacobian launch and two einsums
  tau_compn     ... and for the torques: per link one compute_endeffector_jacobian launch and two einsums, summed
The compositions' outputs are also compared with the calls' (max|d| / max|.|: they agree).  (The accelerations have no composition in
the library: compute_operational_space_dynamics' bias_acc is one link at a time behind a factorisation of H.)

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows —
host work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o links -- python tools/bench_links.py --trace robot:B
    python tools/bench_links.py --read DIR/.../links_results.db --trace robot:B

in which ONE process makes the six kinds of calls of the case one after the other, and the energy call beside them, so the kernels
are compared within one run; --read takes the mean of the timed dispatches of each.  Bytes per row are what the algorithm needs — motion
12 n in, 60 T out; velocities 8 n in, 24 T out; torques 4 n + 24 T in, 4 n out (T links) — and the share of the byte floor is those
bytes at the HBM peak (8.0 TB/s) over the time.

    python tools/bench_links.py [--cases robot:B,...] [--reps 5] [--launches 20]
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
KINDS = ("motion", "velocities", "torques", "motion_general", "velocities_general", "torques_general")


def load(robot, device="cuda:0"):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DifferentiableRobotModel(os.path.join(robot_description_folder, robot + ".urdf"), device=device)


def links_of(m):
    names = m.get_link_names()
    return [names[i] for i in m._spec.preorder() if i != 0]


def inputs(m, B, seed):
    lim = m.get_joint_limits()
    lo = torch.tensor([j["lower"] for j in lim]); hi = torch.tensor([j["upper"] for j in lim])
    free = lo >= hi
    lo, hi = torch.where(free, -np.pi, lo), torch.where(free, np.pi, hi)
    g = torch.Generator().manual_seed(seed)
    n, L = lo.shape[0], len(links_of(m))
    q = (lo + (hi - lo) * torch.rand(B, n, generator=g)).to(m._device)
    qd = (torch.rand(B, n, generator=g) * 2 - 1).to(m._device)
    qdd = (torch.rand(B, n, generator=g) * 2 - 1).to(m._device)
    f = torch.randn(B, L, 3, generator=g).to(m._device)
    t = torch.randn(B, L, 3, generator=g).to(m._device)
    return q, qd, qdd, f, t


def velocities_composition(m, q, qd):
    lin, ang = [], []
    for name in links_of(m):
        jl, ja = m.compute_endeffector_jacobian(q, name)
        lin.append(torch.einsum("bij,bj->bi", jl, qd))
        ang.append(torch.einsum("bij,bj->bi", ja, qd))
    return torch.stack(lin, dim=1), torch.stack(ang, dim=1)


def torques_composition(m, q, f, t):
    tau = torch.zeros_like(q)
    for l, name in enumerate(links_of(m)):
        jl, ja = m.compute_endeffector_jacobian(q, name)
        tau = tau + torch.einsum("bij,bi->bj", jl, f[:, l]) + torch.einsum("bij,bi->bj", ja, t[:, l])
    return tau


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


def row_bytes(n, T):
    return dict(motion=12 * n + 60 * T, velocities=8 * n + 24 * T, torques=4 * n + 24 * T + 4 * n)


def calls_of(m, q, qd, qdd, f, t):
    ln = links_of(m)
    return (("motion", lambda: m.compute_link_motion(q, qd, qdd, link_names=ln)),
            ("velocities", lambda: m.compute_link_velocities(q, qd, link_names=ln)),
            ("torques", lambda: m.compute_external_torques(q, f, t, link_names=ln)),
            ("motion_general", lambda: m.compute_link_motion(q, qd, qdd, link_names=ln, _composed=True)),
            ("velocities_general", lambda: m.compute_link_velocities(q, qd, link_names=ln, _composed=True)),
            ("torques_general", lambda: m.compute_external_torques(q, f, t, link_names=ln, _composed=True)))


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of each kind of one case, one after the other, then as many energy calls."""
    robot, B = spec.split(":")[0], int(spec.split(":")[1])
    m = load(robot)
    q, qd, qdd, f, t = inputs(m, B, B)
    torch.cuda.synchronize()
    with torch.no_grad():
        for _, fn in calls_of(m, q, qd, qdd, f, t) + (("energy", lambda: m.compute_energy_derivatives(q, qd)),):
            for _ in range(WARMUP + launches):
                fn()
            torch.cuda.synchronize()
    print("traced %s: %d + %d calls of each kind" % (spec, WARMUP, launches))


def read(db, spec, launches):
    """Kernel time of one call of each kind from the trace's rocpd database.  The link kernels are told apart by their order: the
    dispatches whose name holds "link_" come in six blocks of WARMUP + launches calls (a batch that is a multiple of 64 makes one
    dispatch per call)."""
    import re
    import sqlite3
    robot, B = spec.split(":")[0], int(spec.split(":")[1])
    m = load(robot, None)
    n, T = m._n_dofs, len(m.get_link_names()) - 1
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    calls = WARMUP + launches
    ln = [(re.sub(r"\(.*", "", name), d) for name, d in rows if "drm" in name and "link_" in name]
    assert len(ln) == len(KINDS) * calls, "expected one link kernel per call (%d dispatches, %d calls)" % (len(ln), len(KINDS) * calls)
    en = [d for name, d in rows if "drm" in name and "energy_" in name]
    assert len(en) == calls, "expected one energy kernel per call"
    t_en = float(np.mean(en[WARMUP:])) / 1e3
    by = row_bytes(n, T)
    en_bytes = 8 * n + 4 * (2 + 3 * n)
    en_share = B * en_bytes / HBM_PEAK * 1e6 / t_en
    print("%s: kernel time of one call (mean of %d dispatches), T = %d links, n = %d" % (spec, launches, T, n))
    for i, kind in enumerate(KINDS):
        block = ln[i * calls:(i + 1) * calls]
        t_us = float(np.mean([d for _, d in block[WARMUP:]])) / 1e3
        b = by[kind.split("_")[0]]
        floor = B * b / HBM_PEAK * 1e6
        print("  %-19s %10.2f us  %4d B per row: byte floor %7.2f us -> %5.1f %% of the HBM peak   %s" % (
            kind, t_us, b, floor, 100 * floor / t_us, block[0][0]))
    print("  %-19s %10.2f us  %4d B per row: %5.1f %% of the HBM peak (the energy kernel of the same run)" % (
        "energy", t_en, en_bytes, 100 * en_share))


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
    assert torch.cuda.is_available(), "bench_links.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    print("%-17s %2s %2s %8s | %9s %9s %9s | %9s %9s %9s | %10s %10s | %7s %7s | %8s %8s" % (
        "robot", "n", "T", "B", "motion", "velocity", "torques", "motion_g", "velocity_g", "torques_g", "vel_compn", "tau_compn", "x_vel",
        "x_tau", "d_vel", "d_tau"))
    models = {}
    for robot, B in cases:
        m = models.get(robot) or models.setdefault(robot, load(robot))
        q, qd, qdd, f, t = inputs(m, B, B)
        n, T = m._n_dofs, len(m.get_link_names()) - 1
        with torch.no_grad():
            tm = {name: timed(fn, args.reps, args.launches) for name, fn in calls_of(m, q, qd, qdd, f, t)}
            rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            d_vel = max(rel(a, b) for a, b in zip(m.compute_link_velocities(q, qd, link_names=links_of(m)), velocities_composition(m, q, qd)))
            d_tau = rel(m.compute_external_torques(q, f, t, link_names=links_of(m)), torques_composition(m, q, f, t))
            t_vel = timed(lambda: velocities_composition(m, q, qd), args.reps, max(2, args.launches // 4))
            t_tau = timed(lambda: torques_composition(m, q, f, t), args.reps, max(2, args.launches // 4))
        print("%-17s %2d %2d %8d | %9.1f %9.1f %9.1f | %9.1f %9.1f %9.1f | %10.1f %10.1f | %7.1f %7.1f | %8.1e %8.1e" % (
            robot, n, T, B, tm["motion"], tm["velocities"], tm["torques"], tm["motion_general"], tm["velocities_general"],
            tm["torques_general"], t_vel, t_tau, t_vel / tm["velocities"], t_tau / tm["torques"], d_vel, d_tau), flush=True)
        del q, qd, qdd, f, t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The q-gradient of the link sweeps in one call (compute_link_power_gradient, csrc/drm_links.hip drm_link_power_dq) against
drm_external_torques in the same run, the general kernel on the same rows, the composition it replaces and the byte floor, on seeded
inputs (tools/bench_links.py's: q uniform over the joint ranges, qd uniform in +-1, unit-normal wrenches on every link but the root,
named in the walk's own order).  Appends its lines to profiles/links_dq_bench.txt (--out).

  dq            compute_link_power_gradient(q, qd, forces, torques): dS/dq alone; the fused kernel on a 7-DoF arm's full tiles
  dq_tau        the same launch with tau stored too (backend.link_power_dq(want_tau=True)): what the backward of the velocities runs
  torques       compute_external_torques(q, forces, torques): the forward sweep pair the gradient extends
  dq_general    dq with every row in the general kernel (DRM_LINKS_COMPOSED)
  compn         what a user writes today: per link one compute_endeffector_jacobian launch on a q that requires grad, two einsums,
                and autograd back to q
The composition's gradient is also compared with the call's (max|d| / max|.|).

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows —
host work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o linksdq -- python tools/bench_links_dq.py --trace robot:B
    python tools/bench_links_dq.py --read DIR/.../linksdq_results.db --trace robot:B

in which ONE process makes the four kinds of calls one after the other; --read takes the mean of the timed dispatches of each.  Bytes per
row are what the algorithm needs — 8 n + 24 T in (q, qd, two wrench arrays of T links), 4 n (dq) or 8 n (dq and tau) out: 276 / 304 B
for the Panda's 8 links — and the byte floor is those bytes at the HBM peak (8.0 TB/s).

    python tools/bench_links_dq.py [--cases robot:B,...] [--reps 5] [--launches 20] [--out profiles/links_dq_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_links import CASES, HBM_PEAK, WARMUP, inputs, links_of, load, timed  # noqa: E402

KINDS = ("dq", "dq_tau", "torques", "dq_general")
OUT = [None]


def say(line):
    print(line, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as fh:
            fh.write(line + "\n")


def row_bytes(n, T):
    return dict(dq=8 * n + 24 * T + 4 * n, dq_tau=8 * n + 24 * T + 8 * n, torques=4 * n + 24 * T + 4 * n, dq_general=8 * n + 24 * T + 4 * n)


def composition(m, q, qd, f, t):
    """dS/dq through the existing differentiable path: per link a Jacobian launch, two einsums, autograd"""
    qr = q.detach().requires_grad_(True)
    S = 0.0
    for l, name in enumerate(links_of(m)):
        jl, ja = m.compute_endeffector_jacobian(qr, name)
        S = S + (torch.einsum("bij,bj->bi", jl, qd) * f[:, l]).sum() + (torch.einsum("bij,bj->bi", ja, qd) * t[:, l]).sum()
    return torch.autograd.grad(S, qr)[0]


def calls_of(m, q, qd, f, t):
    from differentiable_robot_model_amd import backend
    ln = links_of(m)
    dw, T, _, _ = m._links_plan(ln)
    ops_f = m._ops_f(dw).detach()
    return (("dq", lambda: m.compute_link_power_gradient(q, qd, f, t, link_names=ln)),
            ("dq_tau", lambda: backend.link_power_dq(dw.program, ops_f, dw.ops_i, q, qd, f, t, T, m._n_dofs, want_tau=True)),
            ("torques", lambda: m.compute_external_torques(q, f, t, link_names=ln)),
            ("dq_general", lambda: m.compute_link_power_gradient(q, qd, f, t, link_names=ln, _composed=True)))


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of each kind of one case, one after the other."""
    robot, B = spec.split(":")[0], int(spec.split(":")[1])
    m = load(robot)
    q, qd, _, f, t = inputs(m, B, B)
    torch.cuda.synchronize()
    with torch.no_grad():
        for _, fn in calls_of(m, q, qd, f, t):
            for _ in range(WARMUP + launches):
                fn()
            torch.cuda.synchronize()
    print("traced %s: %d + %d calls of each kind" % (spec, WARMUP, launches))


def read(db, spec, launches):
    """Kernel time of one call of each kind from the trace's rocpd database: the dispatches whose name holds "link_" come in four blocks
    of WARMUP + launches calls (a batch that is a multiple of 64 makes one dispatch per call)."""
    import re
    import sqlite3
    robot, B = spec.split(":")[0], int(spec.split(":")[1])
    m = load(robot, None)
    n, T = m._n_dofs, len(m.get_link_names()) - 1
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    calls = WARMUP + launches
    ln = [(re.sub(r"\(.*", "", name), d) for name, d in rows if "drm" in name and "link_" in name]
    assert len(ln) == len(KINDS) * calls, "expected one link kernel per call (%d dispatches, %d calls)" % (len(ln), len(KINDS) * calls)
    by = row_bytes(n, T)
    say("%s: kernel time of one call (mean of %d dispatches), T = %d links, n = %d" % (spec, launches, T, n))
    t_of = {}
    for i, kind in enumerate(KINDS):
        block = ln[i * calls:(i + 1) * calls]
        t_of[kind] = float(np.mean([d for _, d in block[WARMUP:]])) / 1e3
        floor = B * by[kind] / HBM_PEAK * 1e6
        say("  %-11s %10.2f us  %4d B per row: byte floor %7.2f us -> %5.1f %% of the HBM peak   %s" % (
            kind, t_of[kind], by[kind], floor, 100 * floor / t_of[kind], block[0][0]))
    say("  dq / torques %.2f   dq_tau / torques %.2f   dq_general / dq %.2f" % (
        t_of["dq"] / t_of["torques"], t_of["dq_tau"] / t_of["torques"], t_of["dq_general"] / t_of["dq"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:B,... (default: Panda at 4 096, 65 536 and 2^20 rows, Fetch and Allegro at 65 536)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--trace", default=None, help="robot:B: the profiled pass of one case")
    ap.add_argument("--read", default=None, help="the rocpd database of a --trace run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links_dq_bench.txt"), help="the file the lines are appended to")
    args = ap.parse_args()
    OUT[0] = args.out
    if args.read:
        return read(args.read, args.trace, args.launches)
    assert torch.cuda.is_available(), "bench_links_dq.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    say("call time, us: %-15s %2s %2s %8s | %8s %8s %8s %10s | %10s %8s | %9s %9s | %8s" % (
        "robot", "n", "T", "B", "dq", "dq_tau", "torques", "dq_general", "compn", "x_compn", "floor_dq", "floor_tau", "d_compn"))
    models = {}
    for robot, B in cases:
        m = models.get(robot) or models.setdefault(robot, load(robot))
        q, qd, _, f, t = inputs(m, B, B)
        n, T = m._n_dofs, len(m.get_link_names()) - 1
        with torch.no_grad():
            tm = {name: timed(fn, args.reps, args.launches) for name, fn in calls_of(m, q, qd, f, t)}
            got = m.compute_link_power_gradient(q, qd, f, t, link_names=links_of(m))
        want = composition(m, q, qd, f, t)
        d = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
        t_c = timed(lambda: composition(m, q, qd, f, t), args.reps, max(2, args.launches // 4))
        by = row_bytes(n, T)
        say("               %-15s %2d %2d %8d | %8.1f %8.1f %8.1f %10.1f | %10.1f %8.1f | %9.2f %9.2f | %8.1e" % (
            robot, n, T, B, tm["dq"], tm["dq_tau"], tm["torques"], tm["dq_general"], t_c, t_c / tm["dq"],
            B * by["dq"] / HBM_PEAK * 1e6, B * by["dq_tau"] / HBM_PEAK * 1e6, d))
        del q, qd, f, t, got, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

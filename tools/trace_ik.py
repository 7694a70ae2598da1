#!/usr/bin/env python3
"""One Panda solve (fused: one dispatch) and one full-Fetch solve (composed: drm_fk_jacobian + the update kernel per round), for
`rocprofv3 --kernel-trace --stats -d DIR -o ik -- python tools/trace_ik.py` (profiles/ik_trace.txt).  The inputs are made on the
CPU and copied; the model and the targets' FK launch kernels of their own before each solve.

    python tools/trace_ik.py [--B 65536] [--K 32]
    python tools/trace_ik.py --read DIR/ik_results.db      the dispatches of each solve: kernel, count, total and mean time
"""
import argparse
import contextlib
import io
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from differentiable_robot_model_amd.robot_model import DifferentiableRobotModel, robot_description_folder  # noqa: E402


def solve(robot, link, B, K, seed):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cpu = DifferentiableRobotModel(os.path.join(robot_description_folder, robot + ".urdf"))
        gpu = DifferentiableRobotModel(os.path.join(robot_description_folder, robot + ".urdf"), device="cuda:0")
    lower, upper = cpu._joint_bounds()
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.where(torch.isinf(lower), -3.0, lower), torch.where(torch.isinf(upper), 3.0, upper)
    qs = lo + (hi - lo) * (0.1 + 0.8 * torch.rand(B, lo.shape[0], generator=g))
    with torch.no_grad():
        tp, tq = cpu.compute_forward_kinematics(qs, link)
    q0 = torch.minimum(torch.maximum(qs + 0.1 * torch.randn(qs.shape, generator=g), lower), upper)
    q0, tp, tq = q0.cuda(), tp.cuda(), tq.cuda()
    gpu._joint_bounds()
    torch.cuda.synchronize()
    res = gpu.compute_inverse_kinematics(q0, link, tp, tq, max_iterations=K)
    torch.cuda.synchronize()
    print("%s %s B=%d K=%d: converged %.2f %%, mean iterations %.2f" % (robot, link, B, K, 100 * res.converged.float().mean().item(),
                                                                        res.iterations.float().mean().item()))


def read(db):
    """Group the dispatches of the trace's rocpd database by solve: a solve starts at its first IK kernel or drm_fk_jacobian kernel
    after the targets were made, and ends at the last inverse_kinematics kernel."""
    import re
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    ik = [i for i, (n, _) in enumerate(rows) if "inverse_kinematics" in n]
    if not ik:
        print("no inverse_kinematics dispatch in", db)
        return
    # the two solves: split where the gap between IK dispatches contains a non-IK, non-jacobian kernel of torch
    groups, cur = [], [ik[0]]
    for i in ik[1:]:
        between = [rows[j][0] for j in range(cur[-1] + 1, i)]
        if any(not ("jacobian" in n or "chain" in n or "tree" in n) for n in between):
            groups.append(cur); cur = [i]
        else:
            cur.append(i)
    groups.append(cur)
    for g in groups:
        first = g[0]
        while first > 0 and ("jacobian" in rows[first - 1][0] or "chain_fk" in rows[first - 1][0]):
            first -= 1
        stats = {}
        for n, d in rows[first:g[-1] + 1]:
            short = re.sub(r"\(.*", "", n)
            c, t = stats.get(short, (0, 0))
            stats[short] = (c + 1, t + d)
        total = sum(t for _, t in stats.values())
        print("solve: %d dispatches, %.1f us of kernel time" % (g[-1] + 1 - first, total / 1e3))
        for n, (c, t) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
            print("  %5d x %10.1f us total %9.2f us mean  %s" % (c, t / 1e3, t / 1e3 / c, n))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--read", default=None)
    a = ap.parse_args()
    if a.read:
        read(a.read)
        sys.exit(0)
    solve("panda_no_gripper", "panda_virtual_ee_link", a.B, a.K, 1)
    solve("fetch", "gripper_link", 4096, a.K, 2)

#!/usr/bin/env python3
"""Sphere collision cost, its q-gradient and clearances in one launch (compute_collision_cost / compute_sphere_distances,
csrc/drm_collision.hip) against the general kernels on the same rows and against the composition available without them, on the same
seeded inputs (q uniform over the joint ranges; `per_link` spheres on every link but the root, centres uniform in +-6 cm, radii 3 to 8
cm; 8 spheres and 8 oriented boxes around the workspace; "auto" self pairs; the hand in centimetres):

  cost_grad     compute_collision_cost(q, geometry): cost and gradient; the fused kernel (a block of four wavefronts per 64-row tile) for
                a 7-DoF arm's full tiles, the general kernels otherwise
  cost          the same launch asked for the cost alone (no accumulators, no sweep inwards)
  distances     compute_sphere_distances(q, geometry)
  *_general     every row in the general kernels (DRM_LINKS_COMPOSED)
  compn         what a user writes without them: compute_forward_kinematics_links, quaternions to rotations, broadcast signed distances
                with [B, S, M] intermediates, and autograd back through the FK backward kernel (not run above --compn-max rows: its
                intermediates are 12 S M bytes per row and tensor)
The composition's cost and gradient are also compared with the call's (max|d| / max|.|), and both gradients with central differences
of the call's own cost at steps of FD_H (float32, and the cost is only C1: at entries next to a switch of phi the quotient itself is
off by a few hundredths of the largest entry; the figure says which of two gradients that differ by more than a tenth of it is the
cost's, no more).  One wavefront per tile instead of four is a build of csrc/drm_collision.hip with
-DDRM_COLL_WAVES=1, measured by this same script.

CALL time: HIP events around `--launches` back-to-back calls after warm-up, divided by their number, median of `--reps` windows — host
work of a call included.  KERNEL time: a separate run under the profiler,

    rocprofv3 --kernel-trace --stats -d DIR -o collision -- python tools/bench_collision.py --trace robot:B

in which ONE process makes the calls of the case one after the other and drm_link_motion / drm_external_torques beside them.

    python tools/bench_collision.py [--cases robot:B,...] [--reps 5] [--launches 10]
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
import differentiable_robot_model_amd as drm  # noqa: E402
from differentiable_robot_model_amd.robot_model import DifferentiableRobotModel, robot_description_folder  # noqa: E402

CASES = (("panda_no_gripper", 4096), ("panda_no_gripper", 65536), ("panda_no_gripper", 1 << 20), ("fetch", 65536), ("allegro_left", 65536))
WARMUP = 3
FD_H = 1e-3
# per_link, centre spread, radii, world half range, world offset, obstacle radii, half extents, activations
SETUPS = {"panda_no_gripper": (6, 0.06, (0.03, 0.08), (0.6, 0.6, 0.5), (0.0, 0.0, 0.5), (0.08, 0.18), (0.05, 0.2), 0.1, 0.05),
          "fetch": (2, 0.06, (0.03, 0.08), (0.7, 0.7, 0.7), (0.2, 0.0, 0.7), (0.1, 0.22), (0.08, 0.25), 0.1, 0.05),
          "allegro_left": (2, 0.008, (0.009, 0.017), (0.06, 0.06, 0.06), (0.0, 0.0, 0.08), (0.012, 0.03), (0.008, 0.03), 0.02, 0.015)}


def load(robot, device="cuda:0"):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DifferentiableRobotModel(os.path.join(robot_description_folder, robot + ".urdf"), device=device)


def setup(m, robot, seed=11):
    """(geometry, numpy tables of the composition, activations)"""
    per_link, spread, (r0, r1), half, off, (o0, o1), (h0, h1), ew, es = SETUPS[robot]
    rng = np.random.default_rng(seed)
    names = m.get_link_names()
    link = np.repeat(np.arange(1, len(names)), per_link)
    S = len(link)
    centers, radii = rng.uniform(-spread, spread, (S, 3)).astype(np.float32), rng.uniform(r0, r1, S).astype(np.float32)
    place = lambda k: rng.uniform(-1, 1, (k, 3)) * np.asarray(half) + np.asarray(off)
    ws = np.concatenate([place(8), rng.uniform(o0, o1, (8, 1))], 1).astype(np.float32)
    Q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(8)])
    Q[np.linalg.det(Q) < 0, :, 0] *= -1
    bc, bh = place(8).astype(np.float32), rng.uniform(h0, h1, (8, 3)).astype(np.float32)
    world = drm.CollisionWorld(spheres=ws, box_centers=bc, box_half_extents=bh, box_rotations=Q)
    geometry = m.make_collision_geometry(drm.CollisionSpheres([names[l] for l in link], centers, radii), world, "auto")
    # the pairs in the caller's indices, for the composition
    inv = np.arange(S) if geometry.order is None else geometry.order.cpu().numpy()
    back = np.argsort(inv)
    pairs = back[geometry.pairs.cpu().numpy()] if geometry.pairs is not None else np.zeros((0, 2), np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(m._device)
    tables = dict(link=link, names=[names[l] for l in sorted(set(link.tolist()))], c=dev(centers), r=dev(radii), ws=dev(ws), bc=dev(bc), bh=dev(bh),
                  Q=dev(Q.astype(np.float32)), pi=dev(pairs[:, 0]), pj=dev(pairs[:, 1]))
    tables["slot"] = dev(np.searchsorted(sorted(set(link.tolist())), link))
    return geometry, tables, (ew, es)


def inputs(m, B, seed):
    lim = m.get_joint_limits()
    lo = torch.tensor([j["lower"] for j in lim]); hi = torch.tensor([j["upper"] for j in lim])
    free = lo >= hi
    lo, hi = torch.where(free, -np.pi, lo), torch.where(free, np.pi, hi)
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(B, lo.shape[0], generator=g)).to(m._device)


def quat_to_rot(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def phi(d, eta):
    u = eta - d
    return torch.where(u <= 0, torch.zeros_like(u), torch.where(u <= eta, u * u / (2 * eta), u - eta / 2))


def composition(m, q, t, ew, es):
    """(cost [B], gradient [B, n]) from the link frames, broadcast torch ops and autograd"""
    q = q.detach().requires_grad_(True)
    fk = m.compute_forward_kinematics_links(q, t["names"])
    P = torch.stack([fk[name][0] for name in t["names"]], 1)
    R = quat_to_rot(torch.stack([fk[name][1] for name in t["names"]], 1))
    x = P[:, t["slot"]] + torch.einsum("bsij,sj->bsi", R[:, t["slot"]], t["c"])
    e = x[:, :, None, :] - t["ws"][None, None, :, :3]
    d_s = e.norm(dim=-1) - t["ws"][None, None, :, 3] - t["r"][None, :, None]
    y = torch.einsum("mji,bsmj->bsmi", t["Q"], x[:, :, None, :] - t["bc"][None, None])
    a = y.abs() - t["bh"][None, None]
    d_b = torch.where(a.amax(-1) > 0, a.clamp_min(0).norm(dim=-1), a.amax(-1)) - t["r"][None, :, None]
    cost = phi(d_s, ew).sum((1, 2)) + phi(d_b, ew).sum((1, 2))
    d_p = (x[:, t["pi"]] - x[:, t["pj"]]).norm(dim=-1) - t["r"][t["pi"]] - t["r"][t["pj"]]
    cost = cost + phi(d_p, es).sum(1)
    (g,) = torch.autograd.grad(cost.sum(), q)
    return cost.detach(), g


def central_differences(m, q, geometry, ew, es):
    """[B, n]: (cost(q + h e_j) - cost(q - h e_j)) / 2 h of compute_collision_cost's cost, row by row"""
    cost = lambda x: m.compute_collision_cost(x, geometry, world_activation=ew, self_activation=es).cost.double()
    cols = []
    for j in range(q.shape[1]):
        e = torch.zeros_like(q[0])
        e[j] = FD_H
        cols.append((cost(q + e) - cost(q - e)) / (2 * FD_H))
    return torch.stack(cols, 1)


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


def calls_of(m, q, geometry, ew, es, fused):
    from differentiable_robot_model_amd import backend
    dw, T, _, _ = m._links_plan(None)
    args = (dw.program, m._ops_f(dw).detach(), dw.ops_i, q, T, m._n_dofs, geometry.tables(), (1.0, ew, 1.0, es))
    kinds = [("", {})] + [("_general", dict(composed=True))]
    out = []
    for tag, kw in kinds:
        out.append(("cost_grad" + tag, lambda kw=kw: backend.collision_cost(*args, **kw)))
        out.append(("cost" + tag, lambda kw=kw: backend.collision_cost(*args, want=("cost",), **kw)))
        out.append(("distances" + tag, lambda kw=kw: backend.sphere_distances(*args[:7], **kw)))
    return out


def trace(spec, launches):
    """The profiled pass: WARMUP + `launches` calls of each kind of one case, then as many link-motion and external-torque calls."""
    robot, B = spec.split(":")[0], int(spec.split(":")[1])
    m = load(robot)
    geometry, _, (ew, es) = setup(m, robot)
    q = inputs(m, B, B)
    T = len(m.get_link_names())
    f = torch.randn(B, T, 3, device=q.device)
    torch.cuda.synchronize()
    with torch.no_grad():
        extra = [("link_motion", lambda: m.compute_link_motion(q, q, q)), ("external_torques", lambda: m.compute_external_torques(q, f, f))]
        for _, fn in calls_of(m, q, geometry, ew, es, m._n_dofs == 7 and T == 9) + extra:
            for _ in range(WARMUP + launches):
                fn()
            torch.cuda.synchronize()
    print("traced %s: %d + %d calls of each kind; S = %d spheres, %d pairs" % (spec, WARMUP, launches, geometry.n_spheres, geometry.n_pairs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="robot:B,... (default: Panda at 4 096, 65 536 and 2^20 rows, Fetch and Allegro at 65 536)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--compn-max", type=int, default=65536, help="the composition is not run above this many rows")
    ap.add_argument("--trace", default=None, help="robot:B: the profiled pass of one case")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_collision.py measures on a HIP device"
    if args.trace:
        return trace(args.trace, args.launches)
    cases = CASES
    if args.cases:
        cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    models = {}
    for robot, B in cases:
        m = models.get(robot) or models.setdefault(robot, load(robot))
        geometry, tables, (ew, es) = setup(m, robot)
        q = inputs(m, B, B)
        fused = m._n_dofs == 7 and len(m.get_link_names()) == 9
        print("%s B = %d: n = %d, S = %d spheres, 8 + 8 obstacles, %d pairs%s" % (
            robot, B, m._n_dofs, geometry.n_spheres, geometry.n_pairs, "" if fused else " (general kernels only)"), flush=True)
        with torch.no_grad():
            tm = {name: timed(fn, args.reps, args.launches) for name, fn in calls_of(m, q, geometry, ew, es, fused)}
        for name, us in tm.items():
            print("  %-20s %12.1f us   %8.2f ns per row" % (name, us, us * 1e3 / B), flush=True)
        if B <= args.compn_max:
            out = m.compute_collision_cost(q, geometry, world_activation=ew, self_activation=es)
            cost, g = composition(m, q, tables, ew, es)
            rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            t_c = timed(lambda: composition(m, q, tables, ew, es), args.reps, max(2, args.launches // 4))
            print("  %-20s %12.1f us   %8.2f ns per row   x %.1f of cost_grad; max|d| / max|.|: cost %.1e, gradient %.1e" % (
                "compn", t_c, t_c * 1e3 / B, t_c / tm["cost_grad"], rel(out.cost, cost), rel(out.dcost_dq, g)), flush=True)
            with torch.no_grad():
                fd = central_differences(m, q, geometry, ew, es)
            print("  central differences of the cost (h = %g), max|d| / max|.|: the call's gradient %.1e, the composition's %.1e" % (
                FD_H, rel(out.dcost_dq.double(), fd), rel(g.double(), fd)), flush=True)
            del fd
            del cost, g
        del q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

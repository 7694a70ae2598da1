"""Sphere collision cost, its q-gradient and clearances (csrc/drm_collision.hip, include/drm_hip.h drm_collision_cost and
drm_sphere_distances; DifferentiableRobotModel.make_collision_geometry, compute_collision_cost, compute_sphere_distances).

TRUTH, not code under test: the law of csrc/drm_collision.hpp restated HERE in numpy (`law`) on the fp64 oracle's Oracle.fk_all_poses and
fk_jacobian.  Its gradient is first pinned to Richardson-combined central differences of its own fp64 cost, to PIN = 1e-8 (a
"yardstick64" line).  The cost is C1 and piecewise smooth — phi changes branch at u = 0 and u = eta, a box's distance at its faces —
so a difference quotient is an estimate of that order only where no term changes its branch between the stencil's points: the pin is
taken at steps FD_H = 1e-5 and 3e-5 over the entries (row, joint) on whose stencil every term keeps the branch it has at q (`state`),
which must be at least PIN_SHARE = 96 % of them (a "pinned" line gives the share: 96.9 % on the toy, 98.0 % and more on every other
case); the analytic gradient of the other entries, those next to a switch of phi or a box's face, is the same code.  YARDSTICK: the
same numpy in float32 on the oracle's float32 poses and Jacobians.  REQUIREMENT per array — cost, dcost_dq, center, world_distance
and the finite entries of self_distance —
    err <= MARGIN max(err(yardstick), FLOOR max|truth|),     err = max|X - truth|,
MARGIN = 8 and FLOOR = 2^-23 imported from test_fd_derivatives.  Every comparison prints one "COLLISION" line (check, robot, path, array,
error, bound, ratio) before it asserts; profiles/collision_tests.txt holds them for the host build and the MI355X.

RECIPE (`recipe`): states helpers.sample_states(model, B, 3); default_rng(11); 3 spheres per link on every link, the root included
(Panda: S = 27), centres uniform in +-spread in the link frame; a world of 4 spheres and 4 boxes with QR-random rotations; self pairs
between spheres whose link indices differ by at least 2 (Panda: 252; thinned to at most 400 on the trees); activation distances per
robot.  The Panda's numbers are the issue's; the other robots' scales (SCALES) are chosen so that the ACTIVITY asserts hold on the
fp64 truth alone, in EVERY case (each robot, each variant, the skew-axis toy): at least 5 % of world terms active and 1 %
penetrating, at least 2 % of pair terms active and 0.5 % penetrating.
EXCLUSION: rows within 1e-5 of a non-smooth point (a centre inside a box whose two largest a components lie within 1e-5; coincident
centres) are left out of the gradient comparison; their share is asserted <= 2 %.

Every check is a function of the device: un-marked on the host build (cpu_library), test_gpu_* under -m gpu on cuda:0.  On the GPU
B = 64 is one tile of the fused kernel, 65 a tile plus a one-row tail on the general kernels, 192 three tiles.  The variants (world
only, pairs only, spheres only, boxes only, a link subset in scrambled order with a repeated link and links without a sphere, S at the
fused cap and at cap + 1) run on all three arms.  Which path a call takes is observed, not only named: test_gpu_which_path_runs.

Measured (profiles/collision_tests.txt): the worst error / bound is 0.28 on the host build and 0.30 on the MI355X (Panda, boxes only,
dcost_dq); the pin's worst is 9.9e-10 (Fetch arm, S at the cap).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import load_model, sample_states
from oracle import Oracle
from test_fd_derivatives import FLOOR, MARGIN

PIN = 1e-8
FD_H = 1e-5          # the pin's step: see the module docstring
PIN_SHARE = 0.96     # the least share of the entries (row, joint) that the pin covers: see the module docstring
ROWS = 192
ARMS = ("panda_no_gripper", "iiwa7", "fetch_arm_no_gripper")
TREES = ("allegro_left", "fetch")
# per robot: centre spread, radii, world centre half range and offset, obstacle radii, box half extents, eta_world, eta_self
SCALES = {
    "panda_no_gripper": (0.06, (0.03, 0.08), (0.5, 0.5, 0.4), (0.0, 0.0, 0.5), (0.08, 0.18), (0.05, 0.20), 0.1, 0.05),
    "iiwa7": (0.08, (0.05, 0.11), (0.45, 0.45, 0.4), (0.0, 0.0, 0.5), (0.08, 0.18), (0.05, 0.20), 0.1, 0.05),
    "fetch_arm_no_gripper": (0.06, (0.04, 0.09), (0.45, 0.45, 0.4), (0.3, 0.0, 0.6), (0.08, 0.18), (0.05, 0.20), 0.1, 0.05),
    "fetch": (0.06, (0.03, 0.08), (0.6, 0.6, 0.6), (0.2, 0.0, 0.7), (0.10, 0.22), (0.08, 0.25), 0.1, 0.05),
    "allegro_left": (0.008, (0.009, 0.017), (0.06, 0.06, 0.06), (0.0, 0.0, 0.08), (0.012, 0.03), (0.008, 0.03), 0.02, 0.015),
    # (the toy's links lie 0.3 to 1 m apart: spheres of 12 to 20 cm reach the links two further on, obstacles around the links' mean)
    "toy_skew": (0.05, (0.12, 0.20), (0.3, 0.4, 0.5), (0.12, -0.07, 0.65), (0.08, 0.18), (0.05, 0.2), 0.1, 0.05),
}


@functools.lru_cache(maxsize=None)
def model_on(robot, device="cpu", compat=True):
    return load_model(robot, device, reference_compat=compat)


# ------------------------------------------------------------------------------------------------- the law, in numpy
def _phi(d, eta):
    u = eta - d
    return np.where(u <= 0, 0 * u, np.where(u <= eta, u * u / (2 * eta), u - eta / 2)), np.clip(u / eta, 0, 1)


def _unit(e):
    nrm = np.sqrt((e * e).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(nrm[..., None] > 0, e / nrm[..., None], 0 * e)
    return nrm, n


def law(R, P, jac, geo, dt):
    """dict(cost [B], dq [B, n] (None without jac), center [B, S, 3], wd, sd [B, S], and the statistics of the module docstring) of the
    geometry `geo` at link poses R [B, L, 3, 3], P [B, L, 3]; jac: link -> (lin [B, 3, n], ang [B, 3, n]).  Everything in dtype dt."""
    f = np.dtype(dt).type
    li, c, r = geo["link"], geo["centers"].astype(dt), geo["radii"].astype(dt)
    B, S = R.shape[0], len(li)
    x = (P[:, li] + np.einsum("bsij,sj->bsi", R[:, li], c)).astype(dt)
    cost, g = np.zeros(B, dt), np.zeros((B, S, 3), dt)
    wd, sd = np.full((B, S), np.inf, dt), np.full((B, S), np.inf, dt)
    stats, rough, state = {}, np.zeros(B, bool), [np.zeros((B, 0), np.int64)]
    ww, ew, ws, es = (f(v) for v in geo["params"])
    terms = []
    if geo["ws"] is not None and len(geo["ws"]):
        o = geo["ws"].astype(dt)
        nrm, n = _unit(x[:, :, None, :] - o[None, None, :, :3])
        terms.append((nrm - o[None, None, :, 3] - r[None, :, None], n))
        rough |= (nrm < 1e-5).any((1, 2))
        state.append((nrm > 0).reshape(B, -1).astype(np.int64))
    if geo["wb"] is not None and len(geo["wb"]):
        b = geo["wb"].astype(dt)
        Rb = b[:, 6:15].reshape(-1, 3, 3)
        y = np.einsum("mji,bsmj->bsmi", Rb, x[:, :, None, :] - b[None, None, :, :3])
        a = np.abs(y) - b[None, None, :, 3:6]
        amax, m = a.max(-1), np.maximum(a, 0)
        outside, out = amax > 0, np.sqrt((m * m).sum(-1))
        sgn = np.where(y >= 0, f(1), f(-1))
        with np.errstate(invalid="ignore", divide="ignore"):
            dl = np.where(outside[..., None], sgn * m / out[..., None], sgn * (np.arange(3) == a.argmax(-1)[..., None]))
        terms.append((np.where(outside, out, amax) - r[None, :, None], np.einsum("mij,bsmj->bsmi", Rb, dl.astype(dt))))
        srt = np.sort(a, -1)
        rough |= (~outside & (srt[..., 2] - srt[..., 1] < 1e-5)).any((1, 2))
        state.append((outside * 4 + np.where(outside, (a > 0) @ np.asarray([8, 16, 32]), a.argmax(-1))).reshape(B, -1))
    if terms:
        d, n = np.concatenate([t[0] for t in terms], 2), np.concatenate([t[1] for t in terms], 2)
        ph, dp = _phi(d, ew)
        cost = cost + ww * ph.sum((1, 2))
        g = g - ww * (dp[..., None] * n).sum(2)
        wd = d.min(2)
        state.append(((ew - d > 0) * 1 + (ew - d > ew)).reshape(B, -1))
        stats["world_active"], stats["world_pen"] = float((d < ew).mean()), float((d < 0).mean())
        stats["rows_active"] = float((d < ew).any((1, 2)).mean())
    if geo["pairs"] is not None and len(geo["pairs"]):
        pi, pj = geo["pairs"][:, 0], geo["pairs"][:, 1]
        nrm, n = _unit(x[:, pi] - x[:, pj])
        d = nrm - r[pi] - r[pj]
        ph, dp = _phi(d, es)
        cost = cost + ws * ph.sum(1)
        gi = -ws * dp[..., None] * n
        np.add.at(g, (slice(None), pi), gi)
        np.add.at(g, (slice(None), pj), -gi)
        np.minimum.at(sd, (slice(None), pi), d)
        np.minimum.at(sd, (slice(None), pj), d)
        rough |= (nrm < 1e-5).any(1)
        state.append((es - d > 0) * 1 + (es - d > es) + 4 * (nrm > 0))
        stats["pair_active"], stats["pair_pen"] = float((d < es).mean()), float((d < 0).mean())
    dq = None
    if jac is not None:
        dq = np.zeros((B, next(iter(jac.values()))[0].shape[2]), dt)
        for l, (lin, ang) in jac.items():
            on = np.nonzero(li == l)[0]
            F = g[:, on].sum(1)
            M = np.cross(x[:, on] - P[:, l:l + 1], g[:, on]).sum(1)
            dq = dq + np.einsum("bij,bi->bj", lin, F) + np.einsum("bij,bi->bj", ang, M)
    out = dict(cost=cost, dq=dq, center=x, wd=wd, sd=sd, stats=stats, rough=rough)
    assert all(v.dtype == dt for k, v in out.items() if isinstance(v, np.ndarray) and k != "rough"), "the yardstick left its dtype"
    out["state"] = np.concatenate(state, 1)      # the branch of every term: the cost is smooth wherever none of them changes
    return out


def on_oracle(spec, q, geo, dt, grad=True):
    orc = Oracle(spec)
    R, P = orc.fk_all_poses(q.astype(dt), dt)
    jac = None
    if grad:
        jac = {int(l): orc.fk_jacobian(q.astype(dt), int(l), dt)[2:] for l in sorted(set(geo["link"].tolist())) if l > 0}
    return law(R, P, jac, geo, dt)


# ------------------------------------------------------------------------------------------------- the recipe
def random_rotations(rng, k):
    Q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(k)])
    Q[np.linalg.det(Q) < 0, :, 0] *= -1
    return Q


def recipe(spec, scale, per_link=3, links=None, n_ws=4, n_wb=4, max_pairs=400, pairs=True, seed=11):
    """The geometry of the module docstring as numpy arrays in the caller's sphere order: link [S], centers, radii, ws [Ms, 4],
    wb [Mb, 16], pairs [P, 2], params (w_world, eta_world, w_self, eta_self)."""
    spread, (r0, r1), half, off, (o0, o1), (h0, h1), ew, es = scale
    rng = np.random.default_rng(seed)
    links = list(range(len(spec.parent))) if links is None else list(links)
    link = np.repeat(np.asarray(links, np.int64), per_link)
    S = len(link)
    centers = rng.uniform(-spread, spread, (S, 3))
    radii = rng.uniform(r0, r1, S)
    place = lambda k: rng.uniform(-1, 1, (k, 3)) * np.asarray(half) + np.asarray(off)
    ws = np.concatenate([place(n_ws), rng.uniform(o0, o1, (n_ws, 1))], 1) if n_ws else None
    wb = None
    if n_wb:
        c, h, Q = place(n_wb), rng.uniform(h0, h1, (n_wb, 3)), random_rotations(rng, n_wb)
        wb = np.concatenate([c, h, Q.reshape(n_wb, 9), np.zeros((n_wb, 1))], 1)
    pr = None
    if pairs:
        pr = np.asarray([(i, j) for i in range(S) for j in range(i + 1, S) if abs(int(link[i]) - int(link[j])) >= 2], np.int64).reshape(-1, 2)
        if len(pr) > max_pairs:
            pr = pr[np.sort(rng.choice(len(pr), max_pairs, replace=False))]
    return dict(link=link, centers=centers.astype(np.float32), radii=radii.astype(np.float32),
                ws=None if ws is None else ws.astype(np.float32), wb=None if wb is None else wb.astype(np.float32), pairs=pr,
                params=(1.0, ew, 1.0, es))


def geometry_of(model, geo, **kw):
    import differentiable_robot_model_amd as drm
    names = model.get_link_names()
    spheres = drm.CollisionSpheres([names[l] for l in geo["link"]], geo["centers"], geo["radii"])
    world = None
    if geo["ws"] is not None or geo["wb"] is not None:
        wb = geo["wb"]
        world = drm.CollisionWorld(spheres=geo["ws"], box_centers=None if wb is None else wb[:, :3],
                                   box_half_extents=None if wb is None else wb[:, 3:6],
                                   box_rotations=None if wb is None else wb[:, 6:15].reshape(-1, 3, 3))
    return model.make_collision_geometry(spheres, world, self_pairs=geo["pairs"], **kw)


def report(check, robot, path, array, e, bound):
    print("COLLISION %-11s %-20s %-18s %-14s %.3e  %.3e  %.2f" % (check, robot, path, array, e, bound, e / bound if bound else 0.0))


def build_truth(spec, q, geo, name):
    """truth (fp64) and yardstick (float32) of every array on the rows q, with the pin, the activity asserts and the exclusions"""
    t = on_oracle(spec, q.astype(np.float64), geo, np.float64)
    q64, n = q.astype(np.float64), q.shape[1]

    def column(j):
        e = np.zeros(n)
        e[j] = 1.0
        at = {k: on_oracle(spec, q64 + k * FD_H * e, geo, np.float64, grad=False) for k in (-3, -1, 1, 3)}
        smooth = np.all([(v["state"] == t["state"]).all(1) for v in at.values()], 0)
        return (9.0 * (at[1]["cost"] - at[-1]["cost"]) / (2 * FD_H) - (at[3]["cost"] - at[-3]["cost"]) / (6 * FD_H)) / 8.0, smooth
    cols = [column(j) for j in range(n)]
    fd, smooth = np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1)
    keep = ~t["rough"]
    pinned = smooth & keep[:, None]
    e = float(np.abs(t["dq"] - fd)[pinned].max())
    report("yardstick64", name, "-", "dcost_dq", e, PIN)
    print("COLLISION pinned      %-20s %-18s %-14s %.4f of the entries, at least %.2f" % (name, "-", "dcost_dq", pinned.mean(), PIN_SHARE))
    assert e <= PIN, e
    assert pinned.mean() >= PIN_SHARE, "the pin must cover the bulk of the entries"
    assert (~keep).mean() <= 0.02, "more than 2 % of the rows lie at a non-smooth point"
    s = t["stats"]
    if "world_active" in s:
        assert s["world_active"] >= 0.05 and s["world_pen"] >= 0.01, s
    if "pair_active" in s:
        assert s["pair_active"] >= 0.02 and s["pair_pen"] >= 0.005, s
    y = on_oracle(spec, q, geo, np.float32)
    return dict(t=t, y=y, keep=keep)


def compare(check, robot, path, array, x, truth, rows=slice(None)):
    x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
    assert x.dtype == np.float32
    key = {"cost": "cost", "dcost_dq": "dq", "center": "center", "world_distance": "wd", "self_distance": "sd"}[array]
    t, y = truth["t"][key][rows], truth["y"][key][rows]
    assert x.shape == t.shape, (x.shape, t.shape)
    if array == "dcost_dq":
        k = truth["keep"][rows]
        x, t, y = x[k], t[k], y[k]
    finite = np.isfinite(t)
    assert (x[~finite] == t[~finite]).all(), "+inf where the truth has no term"
    if not finite.any():
        return
    e = float(np.abs(x[finite] - t[finite]).max())
    bound = MARGIN * max(float(np.abs(y[finite] - t[finite]).max()), FLOOR * float(np.abs(t[finite]).max()))
    report(check, robot, path, array, e, bound)
    assert e <= bound, (array, e, bound)


@functools.lru_cache(maxsize=None)
def case(robot, variant="full"):
    """(geo, q [ROWS, n], truth) of a robot and a variant of the recipe"""
    model = model_on(robot)
    spec = model._spec
    L = len(spec.parent)
    kw = {}
    if variant == "world_only":
        kw = dict(pairs=False)
    elif variant == "pairs_only":
        kw = dict(n_ws=0, n_wb=0)
    elif variant == "spheres_only":
        kw = dict(n_wb=0, n_ws=8, seed=13)
    elif variant == "boxes_only":
        kw = dict(n_ws=0, n_wb=8)
    elif variant == "subset":       # a link subset in scrambled order with a repeated link; links without a sphere
        kw = dict(links=[L - 2, 2, 5, 2, 0, L - 1], seed=15)
    elif variant == "cap":          # S at the fused cap
        kw = dict(per_link=8, links=list(range(1, 9)), max_pairs=1024)
    elif variant == "cap_plus_one":
        kw = dict(per_link=5, links=list(range(1, L)) + [1, 2, 3, 4, 5], max_pairs=1024)
    geo = recipe(spec, SCALES[robot], **kw)
    if variant == "cap":
        assert len(geo["link"]) == 64
    if variant == "cap_plus_one":
        assert len(geo["link"]) == 65
    q = sample_states(model, ROWS, 3)[0]
    return geo, q, build_truth(spec, q, geo, "%s/%s" % (robot, variant))


def run_and_check(robot, device, path, B=ROWS, variant="full", composed=False, compat=True, subset_walk=False):
    geo, q, truth = case(robot, variant)
    model = model_on(robot, device, compat)
    g = geometry_of(model, geo, _subset_walk=subset_walk)
    tq = torch.from_numpy(q[:B]).to(device)
    out = model.compute_collision_cost(tq, g, world_activation=geo["params"][1], self_activation=geo["params"][3], _composed=composed)
    dist = model.compute_sphere_distances(tq, g, _composed=composed)
    assert out.cost.shape == (B,) and out.dcost_dq.shape == (B, q.shape[1]) and out.cost.grad_fn is None
    rows = slice(0, B)
    name = "%s/%s" % (robot, variant) if variant != "full" else robot
    compare("truth", name, path, "cost", out.cost, truth, rows)
    compare("truth", name, path, "dcost_dq", out.dcost_dq, truth, rows)
    for array, x in zip(("center", "world_distance", "self_distance"), dist):
        compare("truth", name, path, array, x, truth, rows)
    return model, g, tq, out, dist


# ------------------------------------------------------------------------------------------------- host build
@pytest.mark.parametrize("robot", ARMS + TREES)
def test_host_build_against_truth(cpu_library, robot):
    run_and_check(robot, "cpu", "host")


@pytest.mark.parametrize("robot", ARMS)
def test_host_general_walk_on_the_arms(cpu_library, robot):
    run_and_check(robot, "cpu", "host-general", composed=True, B=65)


VARIANTS = ("world_only", "pairs_only", "spheres_only", "boxes_only", "subset", "cap", "cap_plus_one")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("robot", ARMS)
def test_host_variants(cpu_library, robot, variant):
    run_and_check(robot, "cpu", "host", variant=variant, B=65)
    if variant == "subset":
        run_and_check(robot, "cpu", "host-subset-walk", variant=variant, B=65, subset_walk=True)


def skew_check(tmp_path_factory, device, path):
    """tests/test_joint_models.py's toy robot with reference_compat=False: prismatic and skew-axis joints, links of two ops — a wrong
    frame conversion of the centres shows here."""
    from test_joint_models import toy_model, toy_urdf
    urdf = tmp_path_factory.mktemp("toy_collision") / "toy.urdf"
    urdf.write_text(toy_urdf())
    model = toy_model(str(urdf), device)
    spec = model._spec
    assert spec.skew.any()
    geo = recipe(spec, SCALES["toy_skew"])
    q = sample_states(model, 65, 3)[0]
    truth = build_truth(spec, q, geo, "toy_skew")
    g = geometry_of(model, geo)
    tq = torch.from_numpy(q).to(device)
    out = model.compute_collision_cost(tq, g, world_activation=geo["params"][1], self_activation=geo["params"][3])
    dist = model.compute_sphere_distances(tq, g)
    compare("truth", "toy_skew", path, "cost", out.cost, truth)
    compare("truth", "toy_skew", path, "dcost_dq", out.dcost_dq, truth)
    for array, x in zip(("center", "world_distance", "self_distance"), dist):
        compare("truth", "toy_skew", path, array, x, truth)


def test_skew_axis_model(cpu_library, tmp_path_factory):
    skew_check(tmp_path_factory, "cpu", "host")


# ------------------------------------------------------------------------------------------------- exact checks
def exact_checks(device, composed=False, B=128):
    import differentiable_robot_model_amd as drm
    robot = "panda_no_gripper"
    geo, q, _ = case(robot)
    model = model_on(robot, device)
    names = model.get_link_names()
    tq = torch.from_numpy(q[:B]).to(device)
    kw = dict(world_activation=0.1, self_activation=0.05, _composed=composed)
    g = geometry_of(model, geo)
    out = model.compute_collision_cost(tq, g, **kw)
    dist = model.compute_sphere_distances(tq, g, _composed=composed)
    # two launches give the same bits
    again = model.compute_collision_cost(tq, g, **kw)
    assert torch.equal(out.cost, again.cost) and torch.equal(out.dcost_dq, again.dcost_dq)
    assert all(torch.equal(a, b) for a, b in zip(dist, model.compute_sphere_distances(tq, g, _composed=composed)))
    # an output requested alone equals the same output requested together, to the bit
    from differentiable_robot_model_amd import backend
    dw, T, _, _ = model._links_plan(None)
    args = (dw.program, model._ops_f(dw).detach(), dw.ops_i, tq, T, model._n_dofs, g.tables())
    par = (1.0, 0.1, 1.0, 0.05)
    assert torch.equal(backend.collision_cost(*args, par, want=("cost",), composed=composed)[0], out.cost)
    assert torch.equal(backend.collision_cost(*args, par, want=("dq",), composed=composed)[1], out.dcost_dq)
    together = backend.sphere_distances(*args, composed=composed)
    for k, name in enumerate(backend.SPHERE_DISTANCE_OUTPUTS):
        assert torch.equal(backend.sphere_distances(*args, want=(name,), composed=composed)[k], together[k])
    # a world 100 m away and no pair within reach: exact zeros
    far = dict(geo, ws=geo["ws"] + np.float32([100, 0, 0, 0]), wb=geo["wb"] + np.float32([100] + [0] * 15), pairs=geo["pairs"][:1])
    far["radii"] = np.zeros_like(geo["radii"])
    far["centers"] = np.zeros_like(geo["centers"])
    far["pairs"] = np.asarray([(0, 26)])                  # the root's origin and the last link's: further apart than eta
    o = model.compute_collision_cost(tq, geometry_of(model, far), **kw)
    assert (o.cost == 0).all() and (o.dcost_dq == 0).all()
    # r = 0 spheres are points, and a centre exactly on an obstacle's centre gives finite outputs
    on = dict(geo, radii=np.zeros_like(geo["radii"]), ws=geo["ws"].copy(), wb=geo["wb"].copy())
    on["ws"][0, :3] = geo["centers"][0]                    # sphere 0 sits on the root: its world centre is its link-frame centre
    on["wb"][0, :3] = geo["centers"][1]
    og = geometry_of(model, on)
    o = model.compute_collision_cost(tq, og, **kw)
    d = model.compute_sphere_distances(tq, og, _composed=composed)
    assert torch.isfinite(o.cost).all() and torch.isfinite(o.dcost_dq).all() and torch.isfinite(d.world_distance).all()
    assert (d.world_distance[:, 0] <= -on["ws"][0, 3]).all()         # (|x - c| = 0 exactly)
    # root spheres change dcost_dq by no bit when pairs are off
    keep = geo["link"] > 0
    no_pairs = dict(geo, pairs=None)
    without = dict(no_pairs, link=geo["link"][keep], centers=geo["centers"][keep], radii=geo["radii"][keep])
    a = model.compute_collision_cost(tq, geometry_of(model, no_pairs), **kw)
    b = model.compute_collision_cost(tq, geometry_of(model, without), **kw)
    assert torch.equal(a.dcost_dq, b.dcost_dq)
    # per-sphere outputs come back in the caller's order under a shuffled sphere list
    perm = np.random.default_rng(5).permutation(len(geo["link"]))
    inv = np.argsort(perm)
    shuffled = dict(geo, link=geo["link"][perm], centers=geo["centers"][perm], radii=geo["radii"][perm], pairs=inv[geo["pairs"]])
    sg = geometry_of(model, shuffled)
    assert sg.order is not None
    sdist = model.compute_sphere_distances(tq, sg, _composed=composed)
    assert torch.equal(sdist.center, dist.center[:, perm])
    _, _, truth = case(robot)
    pt = dict(truth, t={k: (v[:, perm] if k in ("center", "wd", "sd") else v) for k, v in truth["t"].items()},
              y={k: (v[:, perm] if k in ("center", "wd", "sd") else v) for k, v in truth["y"].items()})
    path = "shuffled" + ("-general" if composed else "")
    compare("order", robot, path, "world_distance", sdist.world_distance, pt, slice(0, B))
    compare("order", robot, path, "self_distance", sdist.self_distance, pt, slice(0, B))
    so = model.compute_collision_cost(tq, sg, **kw)
    compare("order", robot, path, "cost", so.cost, truth, slice(0, B))
    compare("order", robot, path, "dcost_dq", so.dcost_dq, truth, slice(0, B))
    # with_world swaps the obstacles only
    ww = g.with_world(drm.CollisionWorld(spheres=far["ws"]))
    assert ww.spheres is g.spheres and ww.pairs is g.pairs
    assert torch.equal(model.compute_sphere_distances(tq, ww, _composed=composed).self_distance, dist.self_distance)


def test_exact_checks(cpu_library):
    exact_checks("cpu")
    exact_checks("cpu", composed=True, B=65)


def bad_rows_check(device, composed=False, B=128):
    """NaN, Inf and |q| = 4e5 planted in a full tile and in the tail: those rows are NaN, no other row changes a bit."""
    robot = "panda_no_gripper"
    geo, q, _ = case(robot)
    model = model_on(robot, device)
    g = geometry_of(model, geo)
    kw = dict(world_activation=0.1, self_activation=0.05, _composed=composed)
    tq = torch.from_numpy(q[:B].copy()).to(device)
    clean = tuple(model.compute_collision_cost(tq, g, **kw)) + tuple(model.compute_sphere_distances(tq, g, _composed=composed))
    bad = [5, 40, B - 1] if B % 64 else [5, 40, 70]
    tq[bad[0], 2] = float("nan")
    tq[bad[1], 4] = float("inf")
    tq[bad[2], 1] = 4e5
    got = tuple(model.compute_collision_cost(tq, g, **kw)) + tuple(model.compute_sphere_distances(tq, g, _composed=composed))
    others = torch.ones(B, dtype=torch.bool, device=device)
    others[bad] = False
    for a, b in zip(got, clean):
        assert torch.equal(a[others], b[others]) and torch.isnan(a[bad]).all()


def test_non_finite_rows(cpu_library):
    bad_rows_check("cpu")
    bad_rows_check("cpu", composed=True, B=65)


# ------------------------------------------------------------------------------------------------- autograd, errors, shapes
def autograd_check(device):
    robot = "panda_no_gripper"
    geo, q, _ = case(robot)
    model = model_on(robot, device)
    g = geometry_of(model, geo)
    kw = dict(world_activation=0.1, self_activation=0.05)
    tq = torch.from_numpy(q[:64]).to(device).requires_grad_(True)
    w = torch.linspace(0.5, 2.0, 64, device=device)
    out = model.compute_collision_cost(tq, g, **kw)
    assert out.cost.requires_grad and not out.dcost_dq.requires_grad
    (out.cost * w).sum().backward(create_graph=False)
    assert torch.equal(tq.grad, w[:, None] * out.dcost_dq)
    with torch.no_grad():
        o = model.compute_collision_cost(tq, g, **kw)
    assert o.cost.grad_fn is None and not o.cost.requires_grad and torch.equal(o.cost, out.cost.detach())
    out = model.compute_collision_cost(tq, g, **kw)
    (gq,) = torch.autograd.grad(out.cost.sum(), tq, create_graph=True)
    with pytest.raises(RuntimeError):
        gq.sum().backward()
    with pytest.raises(ValueError, match="compute_collision_cost"):
        model.compute_sphere_distances(tq, g)
    # unbatched q gives unbatched results
    one = model.compute_collision_cost(tq[3].detach(), g, **kw)
    assert one.cost.shape == () and one.dcost_dq.shape == (q.shape[1],)
    assert model.compute_sphere_distances(tq[3].detach(), g).center.shape == (len(geo["link"]), 3)
    empty = model.compute_collision_cost(tq[:0].detach(), g, **kw)
    assert empty.cost.shape == (0,) and empty.dcost_dq.shape == (0, q.shape[1])


def test_autograd_and_shapes(cpu_library):
    autograd_check("cpu")


def test_errors_and_auto_pairs(cpu_library):
    import differentiable_robot_model_amd as drm
    model = model_on("panda_no_gripper")
    geo, q, _ = case("panda_no_gripper")
    names = model.get_link_names()
    tq = torch.from_numpy(q[:4])
    nothing = dict(geo, ws=None, wb=None, pairs=None)
    with pytest.raises(ValueError):
        model.compute_collision_cost(tq, geometry_of(model, nothing))
    assert torch.isinf(model.compute_sphere_distances(tq, geometry_of(model, nothing)).world_distance).all()
    with pytest.raises(KeyError):
        model.make_collision_geometry(drm.CollisionSpheres(["no_such_link"], [[0, 0, 0]], [0.1]))
    with pytest.raises(ValueError):
        drm.CollisionSpheres(names[:2], [[0, 0, 0]] * 2, [0.1, -0.1])
    with pytest.raises(ValueError):
        model.make_collision_geometry(drm.CollisionSpheres(names[:2], [[0, 0, 0]] * 2, [0.1, 0.1]), self_pairs=[(0, 0)])
    g = geometry_of(model, geo)
    for bad in (dict(world_activation=0.0), dict(self_activation=float("nan")), dict(world_weight=-1.0), dict(self_weight=float("inf"))):
        with pytest.raises(ValueError):
            model.compute_collision_cost(tq, g, **bad)
    # "auto": spheres whose links are neither the same nor parent and child, a chain of fixed joints counting as one link
    spec = model._spec
    spheres = drm.CollisionSpheres([names[l] for l in geo["link"]], geo["centers"], geo["radii"])
    auto = model.make_collision_geometry(spheres, None, "auto")
    rep = lambda l: rep(int(spec.parent[l])) if l > 0 and spec.dof[l] < 0 else l
    up = lambda l: rep(int(spec.parent[rep(l)])) if rep(l) > 0 else -1
    want = sum(1 for i in range(len(geo["link"])) for j in range(i + 1, len(geo["link"]))
               if rep(geo["link"][i]) != rep(geo["link"][j]) and up(geo["link"][i]) != rep(geo["link"][j]) and up(geo["link"][j]) != rep(geo["link"][i]))
    assert auto.n_pairs == want > 0


# ------------------------------------------------------------------------------------------------- C ABI
def c_abi_check(lib, device, stream, B=5, flags=0, misalign=False):
    """Every DRM_ERR_INVALID case, B == 0, the scratch query honoured with guard words behind the scratch and every output; with
    `misalign` every pointer 4 bytes off a 16-byte boundary and the result within the rule."""
    from differentiable_robot_model_amd import backend
    robot = "panda_no_gripper"
    geo, q, truth = case(robot)
    model = model_on(robot, device)
    g = geometry_of(model, geo)
    dw, T, _, _ = model._links_plan(None)
    walk, n, S = backend._walk_struct(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs), model._n_dofs, g.n_spheres
    sync = (lambda: None) if device == "cpu" else torch.cuda.synchronize
    off = 1 if misalign else 0
    qb = torch.zeros(B * n + 4, device=device)
    qb[off:off + B * n] = torch.from_numpy(q[:B]).to(device).reshape(-1)
    tq = qb[off:]
    sp, world, pr, _ = backend._collision_structs(g.tables(), tq.device)
    GUARD = 64
    full = int(lib.drm_collision_cost_scratch_floats(ctypes.byref(walk), B, S))
    counts = (T, S, len(geo["ws"]) + len(geo["wb"]), len(geo["pairs"]))
    tail = int(lib.drm_collision_cost_scratch_floats_aligned(ctypes.byref(walk), B, *counts))
    assert full == int(lib.drm_sphere_distances_scratch_floats(ctypes.byref(walk), B, S)) >= 0
    assert tail == int(lib.drm_sphere_distances_scratch_floats_aligned(ctypes.byref(walk), B, *counts))
    if device == "cpu":
        assert full == tail == 0
    else:       # the aligned query leaves the full tiles to the fused kernel: the B % 64 tail rows alone
        assert tail == int(lib.drm_collision_cost_scratch_floats(ctypes.byref(walk), B % 64 if B >= 64 else B, S)) > 0 and tail <= full
    need = full if (misalign or flags) else tail
    scratch = torch.full((need + GUARD + 4,), 3.25, device=device)
    ref = lambda s: ctypes.byref(s) if s is not None else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    good = backend.DrmCollisionParams(1.0, 0.1, 1.0, 0.05)

    def cost_call(a=tq, rows=B, targets=T, spheres=sp, w=world, p=pr, par=good, want_cost=True, want_dq=True):
        cost, dq = torch.full((B + 12,), 7.5, device=device), torch.full((B * n + 12,), 7.5, device=device)
        rc = lib.drm_collision_cost(ctypes.byref(walk), ptr(a), rows, targets, ref(spheres), ref(w), ref(p), ref(par), flags,
                                    cost[off:].data_ptr() if want_cost else None, dq[off:].data_ptr() if want_dq else None,
                                    scratch[off:].data_ptr(), stream)
        sync()
        return rc, cost, dq

    def dist_call(a=tq, rows=B, targets=T, spheres=sp, w=world, p=pr, want=(True, True, True)):
        outs = [torch.full((B * S * k + 12,), 7.5, device=device) for k in (3, 1, 1)]
        rc = lib.drm_sphere_distances(ctypes.byref(walk), ptr(a), rows, targets, ref(spheres), ref(w), ref(p), flags,
                                      *[o[off:].data_ptr() if on else None for o, on in zip(outs, want)], scratch[off:].data_ptr(), stream)
        sync()
        return rc, outs
    rc, cost, dq = cost_call()
    assert rc == 0 and (scratch[off + need:] == 3.25).all() and (scratch[:off] == 3.25).all()
    assert (cost[off + B:] == 7.5).all() and (dq[off + B * n:] == 7.5).all() and (cost[:off] == 7.5).all() and (dq[:off] == 7.5).all()
    path = ("misaligned" if misalign else "c-abi") + ("-general" if flags else "")
    compare("abi", robot, path, "cost", cost[off:off + B], truth, slice(0, B))
    compare("abi", robot, path, "dcost_dq", dq[off:off + B * n].reshape(B, n), truth, slice(0, B))
    rc, outs = dist_call()
    assert rc == 0 and (scratch[off + need:] == 3.25).all()
    inv = g.order.cpu().numpy() if g.order is not None else np.arange(S)
    for o, k, name in zip(outs, (3, 1, 1), ("center", "world_distance", "self_distance")):
        assert (o[off + B * S * k:] == 7.5).all() and (o[:off] == 7.5).all()
        x = o[off:off + B * S * k].reshape((B, S, 3) if k == 3 else (B, S))[:, inv]
        compare("abi", robot, path, name, x, truth, slice(0, B))
    if misalign:
        return
    # cost or dq may be NULL, not both; the one that is written keeps its bits
    rc, c1, d1 = cost_call(want_dq=False)
    assert rc == 0 and torch.equal(c1, cost) and (d1 == 7.5).all()
    rc, c1, d1 = cost_call(want_cost=False)
    assert rc == 0 and torch.equal(d1, dq) and (c1 == 7.5).all()
    assert cost_call(want_cost=False, want_dq=False)[0] == -1
    # world or pairs may be NULL, not both
    assert cost_call(w=None)[0] == 0 and cost_call(p=None)[0] == 0 and cost_call(w=None, p=None)[0] == -1
    rc, outs = dist_call(w=None, p=None)                  # an output whose input is NULL is +inf
    assert rc == 0 and torch.isinf(outs[1][:B * S]).all() and torch.isinf(outs[2][:B * S]).all()
    assert dist_call(want=(False, False, False))[0] == -1
    assert dist_call(want=(True, False, False))[0] == 0 and dist_call(want=(False, False, True))[0] == 0
    # NULL required pointers, B < 0, n_targets outside [1, n_ops], S < 1
    assert cost_call(a=None)[0] == -1 and dist_call(a=None)[0] == -1
    assert cost_call(spheres=None)[0] == -1 and dist_call(spheres=None)[0] == -1 and cost_call(par=None)[0] == -1
    assert cost_call(rows=-1)[0] == -1 and dist_call(rows=-1)[0] == -1
    for t in (0, walk.n_ops + 1):
        assert cost_call(targets=t)[0] == -1 and dist_call(targets=t)[0] == -1
    none = backend.DrmCollisionSpheres(sp.spheres, sp.start, 0)
    assert cost_call(spheres=none)[0] == -1 and dist_call(spheres=none)[0] == -1
    assert cost_call(spheres=backend.DrmCollisionSpheres(None, sp.start, S))[0] == -1
    assert cost_call(spheres=backend.DrmCollisionSpheres(sp.spheres, None, S))[0] == -1
    # an activation that is not finite and positive where its term is present; a weight that is negative or not finite
    P = backend.DrmCollisionParams
    for par in (P(1.0, 0.0, 1.0, 0.05), P(1.0, float("nan"), 1.0, 0.05), P(1.0, float("inf"), 1.0, 0.05), P(1.0, 0.1, 1.0, -0.05),
                P(-1.0, 0.1, 1.0, 0.05), P(1.0, 0.1, float("inf"), 0.05), P(float("nan"), 0.1, 1.0, 0.05)):
        assert cost_call(par=par)[0] == -1
    assert cost_call(par=P(1.0, 0.1, -1.0, 0.0), p=None)[0] == 0        # (the self term is absent: its parameters are not read)
    # B == 0
    rc, c0, d0 = cost_call(rows=0)
    assert rc == 0 and (c0 == 7.5).all() and (d0 == 7.5).all()
    rc, outs = dist_call(rows=0)
    assert rc == 0 and all((o == 7.5).all() for o in outs)
    assert (scratch[off + need:] == 3.25).all()


def test_c_abi_on_the_host_build(cpu_library):
    from differentiable_robot_model_amd import backend
    lib = backend.load_library(kind="cpu")
    assert lib.drm_abi_version() == 15
    assert {"drm_collision_cost", "drm_sphere_distances", "drm_collision_cost_scratch_floats", "drm_sphere_distances_scratch_floats",
            "drm_collision_cost_scratch_floats_aligned", "drm_sphere_distances_scratch_floats_aligned"} <= set(backend.EXPORTS)
    c_abi_check(lib, "cpu", None)
    c_abi_check(lib, "cpu", None, flags=1024)
    c_abi_check(lib, "cpu", None, misalign=True)


# ------------------------------------------------------------------------------------------------- GPU
def gpu_path(robot, B, composed):
    return ("general" if composed or robot not in ARMS else "fused") + "-B%d" % B


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 65, 192])
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_against_truth(robot, B):
    run_and_check(robot, "cuda:0", gpu_path(robot, B, False), B=B)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_arm_general_kernel(robot):
    run_and_check(robot, "cuda:0", gpu_path(robot, 65, True), B=65, composed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 65, 192])
@pytest.mark.parametrize("robot", TREES)
def test_gpu_trees_against_truth(robot, B):
    run_and_check(robot, "cuda:0", gpu_path(robot, B, False), B=B)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_variants(robot, variant):
    path = "general-B65" if variant == "cap_plus_one" else "fused-B65"
    run_and_check(robot, "cuda:0", path, variant=variant, B=65)
    if variant == "subset":
        run_and_check(robot, "cuda:0", "general-subset-walk", variant=variant, B=65, subset_walk=True)


def null_scratch(lib, robot, variant, B, flags=0, off=0):
    """(return code of drm_collision_cost, of drm_sphere_distances) with scratch = NULL: only the fused kernel needs none, so DRM_OK
    says that it took every row and DRM_ERR_INVALID that the general path was asked for some (which then launches nothing)."""
    from differentiable_robot_model_amd import backend
    geo, q, _ = case(robot, variant)
    model = model_on(robot, "cuda:0")
    g = geometry_of(model, geo)
    dw, T, _, _ = model._links_plan(None)
    walk, n, S = backend._walk_struct(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs), model._n_dofs, g.n_spheres
    tq = torch.zeros(B * n + 4, device="cuda:0")
    tq[off:off + B * n] = torch.from_numpy(q[:B]).to("cuda:0").reshape(-1)
    sp, world, pr, _ = backend._collision_structs(g.tables(), tq.device)
    par = backend.DrmCollisionParams(1.0, geo["params"][1], 1.0, geo["params"][3])
    cost, dq = torch.empty(B + 4, device="cuda:0"), torch.empty(B * n + 4, device="cuda:0")
    outs = [torch.empty(B * S * k + 4, device="cuda:0") for k in (3, 1, 1)]
    stream = torch.cuda.current_stream().cuda_stream
    rc = (lib.drm_collision_cost(ctypes.byref(walk), tq[off:].data_ptr(), B, T, ctypes.byref(sp), ctypes.byref(world), ctypes.byref(pr),
                                 ctypes.byref(par), flags, cost[off:].data_ptr(), dq[off:].data_ptr(), None, stream),
          lib.drm_sphere_distances(ctypes.byref(walk), tq[off:].data_ptr(), B, T, ctypes.byref(sp), ctypes.byref(world), ctypes.byref(pr),
                                   flags, *[o[off:].data_ptr() for o in outs], None, stream))
    torch.cuda.synchronize()
    counts = (T, S, len(geo["ws"]) + len(geo["wb"]), len(geo["pairs"]))
    tail = int(lib.drm_collision_cost_scratch_floats_aligned(ctypes.byref(walk), B, *counts))
    return rc, tail


@pytest.mark.gpu
def test_gpu_which_path_runs():
    """The labels 'fused' and 'general' of the other tests, observed: with scratch = NULL a call succeeds exactly when the fused
    kernel takes every row, and the aligned scratch query is 0 exactly then."""
    from differentiable_robot_model_amd import backend
    lib = backend.load_library()
    OK, INVALID = (0, 0), (-1, -1)
    for robot in ARMS:
        for B in (64, 192):
            assert null_scratch(lib, robot, "full", B) == (OK, 0)
        rc, tail = null_scratch(lib, robot, "full", 65)                   # a one-row tail
        assert rc == INVALID and tail > 0
    robot = "panda_no_gripper"
    assert null_scratch(lib, robot, "cap", 64) == (OK, 0)                 # S at the fused cap
    rc, tail = null_scratch(lib, robot, "cap_plus_one", 64)               # cap + 1 takes the general path
    assert rc == INVALID and tail > 0
    assert null_scratch(lib, robot, "full", 64, flags=1024)[0] == INVALID     # DRM_LINKS_COMPOSED
    assert null_scratch(lib, robot, "full", 64, off=1)[0] == INVALID          # pointers 4 bytes off a 16-byte boundary
    # the wrapper allocates no scratch for a call that is fused throughout
    geo, q, _ = case(robot)
    model = model_on(robot, "cuda:0")
    dw, T, _, _ = model._links_plan(None)
    walk = backend._walk_struct(dw.program, model._ops_f(dw).detach(), dw.ops_i, model._n_dofs)
    tables = geometry_of(model, geo).tables()
    assert backend._collision_scratch(lib, "drm_collision_cost", walk, 128, T, tables, False, "cuda:0") is None
    assert backend._collision_scratch(lib, "drm_collision_cost", walk, 128, T, tables, True, "cuda:0") is not None


@pytest.mark.gpu
def test_gpu_skew_axis_model(tmp_path_factory):
    skew_check(tmp_path_factory, "cuda:0", "general")


@pytest.mark.gpu
@pytest.mark.parametrize("composed", [False, True], ids=["fused", "general"])
def test_gpu_exact_checks(composed):
    exact_checks("cuda:0", composed=composed, B=128 if not composed else 65)


@pytest.mark.gpu
@pytest.mark.parametrize("B,composed", [(128, False), (65, False), (65, True)], ids=["tiles", "tail", "general"])
def test_gpu_non_finite_rows(B, composed):
    bad_rows_check("cuda:0", composed=composed, B=B)


@pytest.mark.gpu
def test_gpu_autograd_and_shapes():
    autograd_check("cuda:0")


@pytest.mark.gpu
def test_gpu_c_abi():
    from differentiable_robot_model_amd import backend
    lib = backend.load_library()
    assert lib.drm_abi_version() == 15
    stream = torch.cuda.current_stream().cuda_stream
    c_abi_check(lib, "cuda:0", stream)
    c_abi_check(lib, "cuda:0", stream, B=70)
    c_abi_check(lib, "cuda:0", stream, flags=1024)
    c_abi_check(lib, "cuda:0", stream, B=70, misalign=True)

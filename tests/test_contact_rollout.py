"""Plane contact and joint-limit springs (csrc/drm_contact.hpp, drm_contact.hip; compute_contact_torques, compute_contact_rollout)
held to fp64.

Every check is one function of the device: it runs un-marked on the host build and under -m gpu on cuda:0, where the paths are the
fused arm kernels (Panda with and without its own kernels, iiwa7, the Fetch arm: all 8 links, full tiles, B n % 4 == 0) and the
composed per-step path (a link subset, hands, ragged tails, B n % 4 != 0 slabs, misaligned pointers).

Truth (not code under test): oracle.Oracle's fp64 fk_jacobian per link and forward_dynamics, and the law of drm_contact.hpp written
in float64 numpy.  Yardstick: the same recursion in float32 numpy on the oracle's float32 Jacobians, followed by the oracle's float32
forward dynamics at the same states.  REQUIREMENT, per array, the project's standing rule (test_fd_derivatives.MARGIN, FLOOR):

    err(path) <= 8 max(err(yardstick), 2^-23 max|truth|)              err = max |x - truth| over the compared rows

Inputs: helpers.sample_states(model, B, seed), tau ~ U(+-0.01), dt = 1e-3, T <= 9; the plane's offset is the median of n.p over rows
and non-root links at q0; "soft" parameters k = 200, c = 2, mu = 0.5, c_t = 20, radius = 0.03 (Allegro's masses: k = 2, c = 0.02,
c_t = 0.2, radius = 0.005); springs k_l = 50, c_l = 0.5 with about 10 % of the coordinates pushed up to 0.1 rad below `lower` and
about 10 % up to 0.1 rad above `upper`.  The Allegro's springs are k_l = 0.5, c_l = 0.005, the plane's factor of 100: with k_l = 50 an
Euler step of 1e-3 s is unstable for its finger inertias and the fp64 truth itself overflows (max|qd| 827 rad/s after one step, 4e153
after nine; with k_l = 0.5 it stays below 13 rad/s with 21 % of the coordinates active).

The law is discontinuous only where a contact switches on with v_n != 0 and where a limit is crossed: a (row, step) is left out of a
comparison when a contact point has fp64 |depth| < 1e-5 m or a coordinate lies within 1e-5 rad of one of its bounds.  The
excluded share must stay at or below 2 % per case (asserted).  Each case also asserts that at least 25 % of the contact points are
active, that both friction regimes occur and, with springs, that at least 5 % of the coordinates are active: a kernel that never
touches anything cannot pass.

Every comparison prints one "CONTACT" line (check, robot, path, array, error, yardstick, ratio) before it asserts;
profiles/contact_rollout_tests.txt holds them for the host build and the MI355X.  Measured there: the worst ratio is 3.79 on the host
build (Allegro, qdd, B = 65, T = 2, both) and 5.25 on the MI355X (Panda, qdd, B = 64, T = 9, springs only; the fused kernel with and
without the robot's own kernels and the composed subset path alike).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from differentiable_robot_model_amd import JointLimitSprings, PlaneContact, backend
from helpers import load_model, sample_states
from oracle import Oracle
from test_fd_derivatives import FLOOR, MARGIN
from test_rollout import INTEGRATORS, rel, rollout_tol, torques
from test_rollout_edges import ALL_FLAGS, FILL, GUARD, SENTINEL, flags_of, place, to

GPU = "cuda:0"
DT = 1e-3
SWITCH = 1e-5
TILTED = (0.3, -0.2, 0.933)
SOFT = dict(stiffness=200.0, damping=2.0, friction=0.5, friction_slope=20.0, radius=0.03)
SOFT_HAND = dict(stiffness=2.0, damping=0.02, friction=0.5, friction_slope=0.2, radius=0.005)
SPRINGS_ARM, SPRINGS_HAND = (50.0, 0.5), (0.5, 0.005)
ARMS = ("panda_no_gripper", "iiwa7", "fetch_arm_no_gripper")
ROBOTS = ARMS + ("allegro_left",)
SUBSET = {"panda_no_gripper": ["panda_link7", "panda_link2", "panda_link5"]}


def soft(robot):
    return dict(SOFT_HAND if "allegro" in robot else SOFT)


def springs_par(robot):
    return SPRINGS_HAND if "allegro" in robot else SPRINGS_ARM


@functools.lru_cache(maxsize=None)
def model(robot, dev="cpu", own=None):
    m = load_model(robot, dev)
    if own is not None:
        m.own_kernels = own
    return m


@functools.lru_cache(maxsize=None)
def oracle(robot):
    return Oracle(model(robot)._spec)


def report(check, robot, path, array, err, yard, scale):
    bound = max(yard, FLOOR * scale)
    print("CONTACT %-12s %-22s %-16s %-7s %.3e  %.3e  %.2f" % (check, robot, path, array, err, bound, err / bound if bound > 0 else 0.0))
    return err <= MARGIN * bound


# ---------------------------------------------------------------------------------------------------------------- the truth


def unit(normal):
    n = np.asarray(normal, np.float64)
    return n / np.linalg.norm(n)


def law(p, v, w, n, d, par, radius, dt):
    """The law of drm_contact.hpp on [..., 3] arrays in dtype dt -> (force, moment, depth, saturated)"""
    n = n.astype(dt)
    k, c, mu, ct = (dt(par[x]) for x in ("stiffness", "damping", "friction", "friction_slope"))
    rl = np.asarray(radius, dt)[..., None]
    r = -rl * n
    depth = rl[..., 0] - ((p * n).sum(-1) - dt(d))
    vc = v + np.cross(w, r)
    vn = (vc * n).sum(-1)
    vt = vc - vn[..., None] * n
    fn = np.where(depth > 0, np.maximum(dt(0), k * depth - c * vn), dt(0)).astype(dt)
    speed = np.sqrt((vt * vt).sum(-1))
    cap = mu * fn
    slides = (cap > 0) & (ct > 0) & (speed > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(slides, np.minimum(ct, cap / np.where(speed > 0, speed, dt(1))), dt(0)).astype(dt)
    f = fn[..., None] * n - g[..., None] * vt
    return f.astype(dt), np.cross(r, f).astype(dt), depth, slides & (g < ct)


def springs_of(q, qd, lo, hi, k, c, dt):
    q, qd, lo, hi = (np.asarray(x, dt) for x in (q, qd, lo, hi))
    below, above = q < lo, q > hi
    with np.errstate(invalid="ignore"):
        t = np.where(below, dt(k) * (lo - q) - dt(c) * qd, np.where(above, -dt(k) * (q - hi) - dt(c) * qd, dt(0)))
    near = (np.abs(q - lo) < SWITCH) | (np.abs(q - hi) < SWITCH)
    return t.astype(dt), below | above, near


def bounds_of(m):
    lo, hi = m._joint_bounds()
    return lo.cpu().numpy(), hi.cpu().numpy()


def reference(robot, names, q, qd, normal, offset, par, radii, springs, dt):
    """tau [B, n], force, moment [B, L, 3] of the named links in dtype dt, and what the exclusion and the activity checks need"""
    m, orc = model(robot), oracle(robot)
    q, qd = np.asarray(q, dt), np.asarray(qd, dt)
    B, n = q.shape
    tau = np.zeros((B, n), dt)
    F, M, D, S = [], [], [], []
    seen = set()
    radii = np.broadcast_to(np.asarray(radii, np.float64), (len(names),))
    for name, rl in zip(names, radii):
        idx = m._name_to_idx_map[name]
        if idx == 0:                                                     # (the root never touches)
            F.append(np.zeros((B, 3), dt)); M.append(np.zeros((B, 3), dt)); D.append(np.full(B, -1.0)); S.append(np.zeros(B, bool))
            continue
        pos, _, lin, ang = orc.fk_jacobian(q, idx, dt)
        v, w = np.einsum("bij,bj->bi", lin, qd), np.einsum("bij,bj->bi", ang, qd)
        f, mo, depth, sat = law(pos, v, w, unit(normal), offset, par, np.full(B, rl), dt)
        if idx not in seen:                                              # (a link named twice loads the robot once)
            tau += np.einsum("bij,bi->bj", lin, f) + np.einsum("bij,bi->bj", ang, mo)
            seen.add(idx)
        F.append(f); M.append(mo); D.append(depth); S.append(sat)
    out = dict(force=np.stack(F, 1), moment=np.stack(M, 1), depth=np.stack(D, 1), saturated=np.stack(S, 1))
    out["exclude"] = (np.abs(out["depth"]) < SWITCH).any(1)
    out["lim_active"] = np.zeros((B, n), bool)
    if springs is not None:
        lo, hi = bounds_of(m)
        t, act, near = springs_of(q, qd, lo, hi, springs[0], springs[1], dt)
        tau = tau + t
        out["lim_active"] = act
        out["exclude"] = out["exclude"] | near.any(1)
    out["tau"] = tau.astype(dt)
    return out


def states(robot, B, seed, push=False):
    m = model(robot)
    q, qd, _ = sample_states(m, B, seed)
    if push:
        lo, hi = bounds_of(m)
        rng = np.random.default_rng(seed + 1000)
        u, amount = rng.random(q.shape), rng.uniform(0.0, 0.1, q.shape)
        fin = np.isfinite(lo) & np.isfinite(hi)
        q = np.where((u < 0.1) & fin, lo - amount, np.where((u > 0.9) & fin, hi + amount, q)).astype(np.float32)
    return q, qd


POINT_SHIFT = 0.01


def median_offset(robot, q, normal, radius=None):
    """The median of n.p over rows and non-root links.  With radius = 0 it is raised by POINT_SHIFT: the first two links of the arms
    sit at one fixed height, a quarter of all values, which for the z plane IS the median — with spheres their depth is the radius,
    with points it would be a rounding error around zero on every row, the switching case that every comparison leaves out."""
    orc = oracle(robot)
    _, p = orc.fk_all_poses(q.astype(np.float64), np.float64)
    return float(np.median((p[:, 1:] * unit(normal)).sum(-1))) + (POINT_SHIFT if radius == 0.0 else 0.0)


def activity(ref, par, with_springs, tag):
    """the case exercises the law: enough contact points, both friction regimes, enough coordinates on their springs"""
    active = ref["depth"] > 0
    assert active.mean() >= 0.25, (tag, active.mean())
    if par["friction"] > 0 and par["friction_slope"] > 0:
        assert ref["saturated"].any() and (active & ~ref["saturated"]).any(), tag
    if with_springs:
        assert ref["lim_active"].mean() >= 0.05, (tag, ref["lim_active"].mean())
    assert ref["exclude"].mean() <= 0.02, (tag, ref["exclude"].mean())


def plane_of(normal, offset, par):
    return PlaneContact(normal=normal, offset=offset, **par)


# ---------------------------------------------------------------------------------------------------------------- 1  torques


def call_torques(m, dev, q, qd, contact, names, springs=None, composed=False):
    jl = JointLimitSprings(*springs) if springs is not None else None
    out = m.compute_contact_torques(*to(dev, q, qd), contact, link_names=names, joint_limits=jl, _composed=composed)
    assert type(out).__name__ == "ContactTorques" and out._fields == ("tau", "force", "moment")
    assert not any(x.requires_grad for x in out)
    return [x.cpu().numpy() for x in out]


def compare_torques(check, robot, path, got, names, q, qd, normal, offset, par, radii, springs):
    r64 = reference(robot, names, q, qd, normal, offset, par, radii, springs, np.float64)
    r32 = reference(robot, names, q, qd, normal, offset, par, radii, springs, np.float32)
    keep = ~r64["exclude"]
    ok = True
    for name, x in zip(("tau", "force", "moment"), got):
        assert x.shape == r64[name].shape and np.isfinite(x).all(), (check, robot, name)
        err = float(np.abs(x[keep] - r64[name][keep]).max())
        yard = float(np.abs(r32[name][keep] - r64[name][keep]).max())
        ok = report(check, robot, path, name, err, yard, float(np.abs(r64[name][keep]).max())) and ok
    assert ok, (check, robot, path)
    return r64


def check_torques(robot, dev, own=None):
    SPRINGS = springs_par(robot)
    cpu, m = model(robot), model(robot, dev, own)
    names = cpu.get_link_names()
    par = soft(robot)
    path = "host" if dev == "cpu" else ("gpu-arm" if robot in ARMS else "gpu-composed") + ("" if own is None else "-own-" + own)
    rng = np.random.default_rng(3)
    for B in (64, 65, 129):
        q, qd = states(robot, B, seed=B, push=True)
        for normal in ((0.0, 0.0, 1.0), TILTED):
            for radii in (tuple(rng.uniform(0.2, 1.5, len(names)) * par["radius"]), 0.0):
                offset = median_offset(robot, q, normal, radii)
                p = dict(par, radius=radii)
                got = call_torques(m, dev, q, qd, plane_of(normal, offset, p), names, SPRINGS)
                ref = compare_torques("torques-B%d" % B, robot, path, got, names, q, qd, normal, offset, p, radii, SPRINGS)
                activity(ref, p, True, (robot, B, normal))
    # exact identities at B = 129 on the z plane
    z = (0.0, 0.0, 1.0)
    offset = median_offset(robot, q, z)
    no_mu, no_ct = dict(par, friction=0.0), dict(par, friction_slope=0.0)
    a = call_torques(m, dev, q, qd, plane_of(z, offset, no_mu), names)
    b = call_torques(m, dev, q, qd, plane_of(z, offset, no_ct), names)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "mu = 0 and c_t = 0 are the same frictionless law"
    assert np.array_equal(a[1][..., :2], np.zeros_like(a[1][..., :2])) and (a[1][..., 2] > 0).any()
    # r = 0, mu = 0: the shipped example's law through compute_external_torques
    point = dict(no_mu, radius=0.0)
    full_offset, offset = offset, median_offset(robot, q, z, 0.0)
    got = call_torques(m, dev, q, qd, plane_of(z, offset, point), names)
    dq, dqd = to(dev, q, qd)
    motion = m.compute_link_motion(dq, dqd, link_names=names)
    depth = (offset - motion.position[..., 2]).clamp_min(0.0)
    fz = (point["stiffness"] * depth - point["damping"] * motion.linear_velocity[..., 2] * (depth > 0)).clamp_min(0.0)
    force = torch.stack([torch.zeros_like(fz), torch.zeros_like(fz), fz], dim=-1)
    force[:, names.index(cpu.get_link_names()[0])] = 0.0            # (the example leaves the root out of its links: it never touches)
    example = m.compute_external_torques(dq, force, link_names=names).cpu().numpy()
    compare_torques("example-law", robot, path, [example, force.cpu().numpy(), np.zeros_like(got[2])], names, q, qd, z, offset, point,
                    0.0, None)
    compare_torques("point-law", robot, path, got, names, q, qd, z, offset, point, 0.0, None)
    # a plane far below every link
    offset = full_offset
    far = call_torques(m, dev, q, qd, plane_of(z, -100.0, par), names)
    assert all(np.array_equal(x, np.zeros_like(x)) for x in far)
    # a subset, a permuted order and a repeated link agree with the all-links call on the links they share
    full = call_torques(m, dev, q, qd, plane_of(z, offset, par), names)
    pick = [names[-1], names[2], names[0], names[4], names[2]]
    sub = call_torques(m, dev, q, qd, plane_of(z, offset, par), pick)
    for j, name in enumerate(pick):
        i = names.index(name)
        scale = FLOOR * MARGIN * max(float(np.abs(full[1]).max()), float(np.abs(full[2]).max()))
        assert np.abs(sub[1][:, j] - full[1][:, i]).max() <= scale and np.abs(sub[2][:, j] - full[2][:, i]).max() <= scale, name
    ref = compare_torques("subset", robot, path, sub, pick, q, qd, z, offset, par, par["radius"], None)


@pytest.mark.parametrize("robot", ROBOTS)
def test_contact_torques_against_fp64(cpu_library, robot):
    check_torques(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot,own", [("panda_no_gripper", None), ("panda_no_gripper", "off"), ("iiwa7", None),
                                       ("fetch_arm_no_gripper", None), ("allegro_left", None)], ids=lambda v: str(v))
def test_gpu_contact_torques_against_fp64(robot, own):
    check_torques(robot, GPU, own)


# ---------------------------------------------------------------------------------------------------------------- 2  rollout


def fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def call_rollout(m, dev, q, qd, tau, contact, names, springs, integ, g, d, qdd=True, composed=False):
    jl = JointLimitSprings(*springs) if springs is not None else None
    out = m.compute_contact_rollout(*to(dev, q, qd, tau), DT, contact, link_names=names, joint_limits=jl, integrator=integ,
                                    include_gravity=bool(g), use_damping=bool(d), return_acceleration=qdd, _composed=composed)
    assert type(out).__name__ == "ContactRollout" and out._fields == ("q", "qd", "qdd")
    assert (out.qdd is None) == (not qdd) and not out.q.requires_grad
    return [None if x is None else x.cpu().numpy() for x in out]


def check_steps(check, robot, path, names, q, qd, tau, got, normal, offset, par, springs, integ, g, d, rows=None):
    """every step from the call's own previous state: qdd against fp64, the integrator's identity to the bit.  -> the worst ratio"""
    orc = oracle(robot)
    qt, qdt, qddt = got
    T, B, n = tau.shape
    rows = np.arange(B) if rows is None else rows
    h = np.float32(DT)
    errs, yards, scales, excluded, refs = [], [], [], 0, []
    for t in range(T):
        x, v = (q, qd) if t == 0 else (qt[t - 1], qdt[t - 1])
        x, v = x[rows], v[rows]
        # the integrator, exactly
        v1 = fma32(h, qddt[t][rows], v)
        x1 = fma32(h, v if integ == "euler" else v1, x)
        assert np.array_equal(v1, qdt[t][rows]) and np.array_equal(x1, qt[t][rows]), (check, robot, path, t, "integrator identity")
        if normal is None:
            e64 = dict(tau=np.zeros((len(rows), n)), exclude=np.zeros(len(rows), bool), lim_active=np.zeros((len(rows), n), bool))
            e32 = dict(tau=np.zeros((len(rows), n), np.float32))
            if springs is not None:
                lo, hi = bounds_of(model(robot))
                for e, dt in ((e64, np.float64), (e32, np.float32)):
                    e["tau"], act, near = springs_of(x, v, lo, hi, springs[0], springs[1], dt)
                    if dt is np.float64:
                        e["lim_active"], e["exclude"] = act, near.any(1)
        else:
            e64 = reference(robot, names, x, v, normal, offset, par, par["radius"], springs, np.float64)
            e32 = reference(robot, names, x, v, normal, offset, par, par["radius"], springs, np.float32)
        want = orc.forward_dynamics(x.astype(np.float64), v.astype(np.float64), tau[t][rows].astype(np.float64) + e64["tau"], bool(g),
                                    bool(d), np.float64)
        yard = orc.forward_dynamics(x, v, (tau[t][rows] + e32["tau"]).astype(np.float32), bool(g), bool(d), np.float32)
        keep = ~e64["exclude"]
        excluded += int(e64["exclude"].sum())
        assert np.isfinite(qddt[t][rows]).all()
        errs.append(float(np.abs(qddt[t][rows][keep] - want[keep]).max()))
        yards.append(float(np.abs(yard[keep] - want[keep]).max()))
        scales.append(float(np.abs(want[keep]).max()))
        refs.append(e64)
    assert excluded <= 0.02 * T * len(rows), (check, robot, path, excluded)
    ok = report(check, robot, path, "qdd", max(errs), max(yards), max(scales))
    assert ok, (check, robot, path, integ, g, d)
    return refs


def rollout_case(robot, B, T, seed, push):
    q, qd = states(robot, B, seed, push)
    return q, qd, torques(model(robot), T, B, seed=seed + 1)


MODES = ("both", "contact", "springs")


def check_rollout(robot, dev, own=None, names=None, path=None):
    SPRINGS = springs_par(robot)
    cpu, m = model(robot), model(robot, dev, own)
    names = cpu.get_link_names() if names is None else names
    par = soft(robot)
    z = (0.0, 0.0, 1.0)
    path = path or ("host" if dev == "cpu" else "gpu")
    # every B x T once, the integrators, flag pairs and modes rotating through them; then what the rotation left out at one shape
    flag_sets = flags_of(robot, ALL_FLAGS, 9, DT, panda=True)
    combos = [(B, T, INTEGRATORS[i % 2], flag_sets[i % len(flag_sets)], MODES[i % 3])
              for i, (B, T) in enumerate((B, T) for B in (64, 65, 129) for T in (1, 2, 9))]
    combos += [(129, 9, integ, (1, 0), mode) for integ in INTEGRATORS for mode in MODES]
    combos += [(65, 2, "semi_implicit_euler", f, "both") for f in flag_sets]
    for B, T, integ, (g, d), mode in combos:
        q, qd, tau = rollout_case(robot, B, T, seed=7 * B + T, push=mode != "contact")
        normal = None if mode == "springs" else z
        offset = median_offset(robot, q, z)
        contact = None if mode == "springs" else plane_of(z, offset, par)
        springs = None if mode == "contact" else SPRINGS
        got = call_rollout(m, dev, q, qd, tau, contact, names, springs, integ, g, d)
        plain = call_rollout(m, dev, q, qd, tau, contact, names, springs, integ, g, d, qdd=False)
        assert plain[2] is None and np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]), "asking for qdd changes q, qd"
        assert all(x.shape == (T, B, cpu._n_dofs) for x in got)
        tag = "%s-B%d-T%d-%s-g%dd%d-%s" % (path, B, T, "eul" if integ == "euler" else "semi", g, d, mode)
        refs = check_steps("rollout", robot, tag, names, q, qd, tau, got, normal, offset, par, springs, integ, g, d)
        if mode != "springs" and T == 9:
            activity(dict(depth=np.concatenate([r["depth"] for r in refs]), saturated=np.concatenate([r["saturated"] for r in refs]),
                          lim_active=np.concatenate([r["lim_active"] for r in refs]),
                          exclude=np.concatenate([r["exclude"] for r in refs])), par, mode == "both", tag)


@pytest.mark.parametrize("robot", ROBOTS + ("iiwa7_allegro",))
def test_contact_rollout_steps_against_fp64(cpu_library, robot):
    check_rollout(robot, "cpu")


GPU_PATHS = [("panda_no_gripper", None, None, "gpu-arm"), ("panda_no_gripper", "off", None, "gpu-arm-own-off"),
             ("iiwa7", None, None, "gpu-arm"), ("fetch_arm_no_gripper", None, None, "gpu-arm"),
             ("panda_no_gripper", None, "subset", "gpu-composed-subset"), ("allegro_left", None, None, "gpu-composed"),
             ("iiwa7_allegro", None, None, "gpu-composed")]


@pytest.mark.gpu
@pytest.mark.parametrize("robot,own,names,path", GPU_PATHS, ids=lambda v: str(v))
def test_gpu_contact_rollout_steps_against_fp64(robot, own, names, path):
    check_rollout(robot, GPU, own, SUBSET[robot] if names == "subset" else None, path)


def test_subset_rollout_against_fp64(cpu_library):
    check_rollout("panda_no_gripper", "cpu", None, SUBSET["panda_no_gripper"], "host-subset")


# ---------------------------------------------------------------------------------------------------------------- 3  paths


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ARMS)
def test_gpu_fused_composed_and_host_agree(robot):
    """B = 128: two full tiles (fused); the same rows composed (_composed) differ in some bit, two launches of one path in none; both
    lie within twice the bound of the host build.  B = 65: the tail row and the B n % 4 != 0 slabs are composed rows."""
    cpu, gpu = model(robot), model(robot, GPU)
    names, par, z = cpu.get_link_names(), soft(robot), (0.0, 0.0, 1.0)
    T, SPRINGS = 9, springs_par(robot)
    q, qd, tau = rollout_case(robot, 128, T, seed=31, push=True)
    contact = plane_of(z, median_offset(robot, q, z), par)
    args = (q, qd, tau, contact, names, SPRINGS, "semi_implicit_euler", 1, 0)
    fused, again = call_rollout(gpu, GPU, *args), call_rollout(gpu, GPU, *args)
    comp, comp2 = call_rollout(gpu, GPU, *args, composed=True), call_rollout(gpu, GPU, *args, composed=True)
    host = call_rollout(cpu, "cpu", *args)
    tol = 2 * rollout_tol(robot, 8, DT)
    for k, name in enumerate(("q", "qd")):
        assert np.array_equal(fused[k], again[k]) and np.array_equal(comp[k], comp2[k]), (robot, name, "one path, two launches")
        for path, x in (("gpu-arm", fused), ("gpu-composed", comp)):
            e = rel(x[k], host[k])
            print("CONTACT %-12s %-22s %-16s %-7s %.3e  %.3e  %.2f" % ("vs-host", robot, path, name, e, tol, e / tol))
            assert e <= tol, (robot, path, name, e, tol)
    assert any(not np.array_equal(fused[k], comp[k]) for k in range(3)), "the fused and the composed path are different code"
    tq, tf, tm = call_torques(gpu, GPU, q, qd, contact, names, SPRINGS)
    cq, cf, cm = call_torques(gpu, GPU, q, qd, contact, names, SPRINGS, composed=True)
    hq, hf, hm = call_torques(cpu, "cpu", q, qd, contact, names, SPRINGS)
    for name, a, b, c in (("tau", tq, cq, hq), ("force", tf, cf, hf), ("moment", tm, cm, hm)):
        scale = float(np.abs(c).max())
        assert np.abs(a - c).max() <= 2 * MARGIN * 64 * FLOOR * scale and np.abs(b - c).max() <= 2 * MARGIN * 64 * FLOOR * scale, (robot, name)
    # the tail row of B = 65 takes the composed path: the composed call's values on the same row
    q, qd, tau = rollout_case(robot, 65, T, seed=32, push=True)
    args = (q, qd, tau, contact, names, SPRINGS, "semi_implicit_euler", 1, 0)
    a, b = call_rollout(gpu, GPU, *args), call_rollout(gpu, GPU, *args, composed=True)
    assert all(np.array_equal(x[:, 64], y[:, 64]) for x, y in zip(a, b))


def c_rollout(robot, dev, names, q0, qd0, tau, contact, radius, springs, misaligned):
    """drm_contact_rollout straight through the C ABI (test_rollout_edges.c_rollout): every tensor aligned or every tensor
    misaligned, the scratch of exactly the queried size followed by GUARD sentinel words.  -> (q_traj, qd_traj) on the CPU"""
    m = model(robot, dev)
    device = torch.device(dev)
    lib = backend.library_for(device)
    dw = m._dynamics_walk()
    lw, TL, _, _ = m._links_plan(names)
    dwalk = backend._walk_struct(dw.program, m._ops_f(dw).detach(), dw.ops_i, m._n_dofs)
    lwalk = backend._walk_struct(lw.program, m._ops_f(lw).detach(), lw.ops_i, m._n_dofs)
    T, B, n = tau.shape
    ins = [place(t, dev, misaligned) for t in to("cpu", q0, qd0, tau)]
    outs = [place(torch.full((T, B, n), FILL), dev, misaligned) for _ in range(2)]
    need = int(lib.drm_contact_rollout_scratch_floats(ctypes.byref(dwalk), ctypes.byref(lwalk), B))
    need_aligned = int(lib.drm_contact_rollout_scratch_floats_aligned(ctypes.byref(dwalk), ctypes.byref(lwalk), B))
    assert 0 <= need_aligned <= need
    size = need if misaligned else need_aligned
    scratch = torch.full((size + GUARD,), SENTINEL, device=dev) if device.type == "cuda" else None
    if scratch is None:
        assert need == 0
    pl = backend.DrmContactPlane((ctypes.c_float * 3)(*contact.normal), contact.offset, contact.stiffness, contact.damping,
                                 contact.friction, contact.friction_slope)
    sp = backend.DrmJointSprings(*springs)
    lo, hi = m._joint_bounds()
    rad = torch.full((TL,), float(radius), device=dev)
    rc = lib.drm_contact_rollout(ctypes.byref(dwalk), ctypes.byref(lwalk), ins[0][1].data_ptr(), ins[1][1].data_ptr(),
                                 ins[2][1].data_ptr(), B, T, float(DT), backend.RNEA_GRAVITY, TL, ctypes.byref(pl), rad.data_ptr(),
                                 ctypes.byref(sp), lo.data_ptr(), hi.data_ptr(), outs[0][1].data_ptr(), outs[1][1].data_ptr(), None,
                                 scratch.data_ptr() if scratch is not None else None, backend._stream(device))
    assert rc == 0, lib.drm_last_error()
    if scratch is not None:
        torch.cuda.synchronize()
        assert bool((scratch[size:] == SENTINEL).all()), (robot, B, misaligned, "the call wrote past its scratch")
    for flat, _ in outs:
        assert float(flat[0 if misaligned else -1]) == FILL
    return [v.cpu().numpy().copy() for _, v in outs]


def check_c_abi(robot, dev):
    SPRINGS = springs_par(robot)
    cpu, m = model(robot), model(robot, dev)
    names, par, z = cpu.get_link_names(), soft(robot), (0.0, 0.0, 1.0)
    for B in (128, 129):
        q, qd, tau = rollout_case(robot, B, 5, seed=40 + B, push=True)
        contact = plane_of(z, median_offset(robot, q, z), par)
        api = call_rollout(m, dev, q, qd, tau, contact, names, SPRINGS, "semi_implicit_euler", 1, 0, qdd=False)
        aligned = c_rollout(robot, dev, names, q, qd, tau, contact, par["radius"], SPRINGS, False)
        mis = c_rollout(robot, dev, names, q, qd, tau, contact, par["radius"], SPRINGS, True)
        tol = 2 * rollout_tol(robot, 8, DT) if dev != "cpu" else 0.0
        for k, name in enumerate(("q", "qd")):
            assert np.array_equal(aligned[k], api[k]), (robot, B, name)
            e = rel(mis[k], aligned[k])
            print("CONTACT %-12s %-22s %-16s %-7s %.3e  %.3e" % ("misaligned", robot, "B%d" % B, name, e, tol))
            assert np.isfinite(mis[k]).all() and e <= tol, (robot, B, name, e, tol)


@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left"))
def test_misaligned_pointers_through_the_c_abi(cpu_library, robot):
    check_c_abi(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left", "fetch_arm_no_gripper"))
def test_gpu_misaligned_pointers_through_the_c_abi(robot):
    check_c_abi(robot, GPU)


# ---------------------------------------------------------------------------------------------------------------- 4  zero contact


def check_zero_contact(robot, dev, B, composed):
    """a plane far below every link and no springs: the plain rollout — to the bit on the composed path (the same forward-dynamics
    and integrator arithmetic on tau + 0), within rollout_tol on the fused path (bit-equality reported)"""
    cpu, m = model(robot), model(robot, dev)
    q, qd, tau = rollout_case(robot, B, 9, seed=50, push=False)
    contact = plane_of((0.0, 0.0, 1.0), -100.0, soft(robot))
    for integ in INTEGRATORS:
        got = call_rollout(m, dev, q, qd, tau, contact, None, None, integ, 1, 0, qdd=False, composed=composed)
        want = [x.cpu().numpy() for x in m.compute_forward_dynamics_rollout(*to(dev, q, qd, tau), DT, integrator=integ)]
        same = all(np.array_equal(a, b) for a, b in zip(got[:2], want))
        print("CONTACT %-12s %-22s %-16s bit-equal to the plain rollout: %s" % ("zero", robot, "composed" if composed else "fused", same))
        if composed:
            assert same, (robot, integ)
        else:
            tol = rollout_tol(robot, 9, DT)
            assert max(rel(got[0], want[0]), rel(got[1], want[1])) <= tol, (robot, integ)


@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left", "fetch_arm_no_gripper"))
def test_zero_contact_is_the_plain_rollout(cpu_library, robot):
    check_zero_contact(robot, "cpu", 65, True)


@pytest.mark.gpu
@pytest.mark.parametrize("robot,B,composed", [("panda_no_gripper", 128, False), ("iiwa7", 128, False), ("fetch_arm_no_gripper", 63, True),
                                              ("panda_no_gripper", 63, True), ("iiwa7_allegro", 64, True)], ids=lambda v: str(v))
def test_gpu_zero_contact_is_the_plain_rollout(robot, B, composed):
    """composed: batches whose PLAIN rollout is composed on every row too (an arm below one full tile, a robot without a fused rollout
    kernel), so that both calls run drm_forward_dynamics and the integrator on the same rows"""
    check_zero_contact(robot, GPU, B, composed)


# ---------------------------------------------------------------------------------------------------------------- 5  edges


def check_non_finite_rows(robot, dev, B=128):
    SPRINGS = springs_par(robot)
    cpu, m = model(robot), model(robot, dev)
    names, par, z = cpu.get_link_names(), soft(robot), (0.0, 0.0, 1.0)
    T = 6
    q, qd, tau = rollout_case(robot, B, T, seed=60, push=True)
    contact = plane_of(z, median_offset(robot, q, z), par)
    bad_q, bad_tau = q.copy(), tau.copy()
    bad_q[5, 2] = np.nan
    bad_tau[3, 70, 1] = np.inf
    others = np.ones(B, bool)
    others[[5, 70]] = False
    for integ in INTEGRATORS:
        clean = call_rollout(m, dev, q, qd, tau, contact, names, SPRINGS, integ, 1, 0)
        got = call_rollout(m, dev, bad_q, qd, bad_tau, contact, names, SPRINGS, integ, 1, 0)
        assert all(np.isfinite(x).all() for x in clean)
        for a, b in zip(got, clean):
            assert np.array_equal(a[:, others], b[:, others]), (robot, integ)
            assert np.array_equal(a[:3, 70], b[:3, 70]), (robot, integ)
        assert not np.isfinite(got[1][:, 5]).all(1).any() and not np.isfinite(got[1][3:, 70, 1]).any(), (robot, integ)
    ct = call_torques(m, dev, bad_q, qd, contact, names, SPRINGS)
    cc = call_torques(m, dev, q, qd, contact, names, SPRINGS)
    keep = np.arange(B) != 5
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(ct, cc))
    assert np.isnan(ct[0][5]).all() and np.isnan(ct[1][5, 1:]).all() and np.isnan(ct[2][5, 1:]).all()      # (entry 0 is the root)


@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left"))
def test_non_finite_rows_are_isolated(cpu_library, robot):
    check_non_finite_rows(robot, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ("panda_no_gripper", "allegro_left", "fetch_arm_no_gripper"))
def test_gpu_non_finite_rows_are_isolated(robot):
    check_non_finite_rows(robot, GPU)


def check_refusals(dev):
    robot = "panda_no_gripper"
    m = model(robot, dev)
    n = m._n_dofs
    q, qd, tau = (torch.from_numpy(x).to(dev) for x in rollout_case(robot, 3, 2, seed=70, push=False))
    good = PlaneContact(stiffness=100.0, damping=1.0)
    for kw in (dict(stiffness=float("nan"), damping=1.0), dict(stiffness=-1.0, damping=1.0), dict(stiffness=1.0, damping=float("inf")),
               dict(stiffness=1.0, damping=1.0, friction=-0.1), dict(stiffness=1.0, damping=1.0, friction_slope=float("nan")),
               dict(stiffness=1.0, damping=1.0, normal=(0.0, 0.0, 0.0)), dict(stiffness=1.0, damping=1.0, radius=-0.1),
               dict(stiffness=1.0, damping=1.0, offset=float("inf"))):
        with pytest.raises(ValueError):
            PlaneContact(**kw)
    for args in ((-1.0,), (1.0, float("nan"))):
        with pytest.raises(ValueError):
            JointLimitSprings(*args)
    with pytest.raises(ValueError, match="at least one step"):
        m.compute_contact_rollout(q, qd, tau[:0], DT, good)
    for dt in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dt"):
            m.compute_contact_rollout(q, qd, tau, dt, good)
    with pytest.raises(ValueError, match="plain rollout"):
        m.compute_contact_rollout(q, qd, tau, DT, None)
    with pytest.raises(ValueError, match="integrator"):
        m.compute_contact_rollout(q, qd, tau, DT, good, integrator="rk4")
    with pytest.raises(ValueError, match="radius"):
        m.compute_contact_torques(q, qd, PlaneContact(stiffness=1.0, damping=1.0, radius=(0.1, 0.2)))
    for k in range(3):
        leaves = [q.clone(), qd.clone(), tau.clone()]
        leaves[k].requires_grad_(True)
        with pytest.raises(ValueError, match="forward only"):
            m.compute_contact_rollout(*leaves, DT, good)
        if k < 2:
            with pytest.raises(ValueError, match="forward only"):
                m.compute_contact_torques(leaves[0], leaves[1], good)
    with pytest.raises(AssertionError):
        m.compute_contact_rollout(q, qd[:2], tau, DT, good)
    with pytest.raises(AssertionError):
        m.compute_contact_rollout(q, qd, tau[:, :2], DT, good)
    with pytest.raises(AssertionError):
        m.compute_contact_torques(q, qd[:, :n - 1], good)
    # the C ABI refuses what the binding lets through: a plane built around the constructor
    lib = backend.library_for(torch.device(dev))
    lw, TL, _, _ = m._links_plan(None)
    walk = backend._walk_struct(lw.program, m._ops_f(lw).detach(), lw.ops_i, n)
    out = torch.zeros(3, n, device=dev)
    for normal, k in (((0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, 1.0), -1.0), ((0.0, float("nan"), 1.0), 1.0), ((0.0, 0.0, 1.0), float("inf"))):
        pl = backend.DrmContactPlane((ctypes.c_float * 3)(*normal), 0.0, k, 1.0, 0.0, 0.0)
        rc = lib.drm_contact_torques(ctypes.byref(walk), q.data_ptr(), qd.data_ptr(), 3, TL, ctypes.byref(pl), None, None, None, None, 0,
                                     out.data_ptr(), None, None, None, backend._stream(torch.device(dev)))
        assert rc != 0 and lib.drm_last_error(), (normal, k)
    # unbatched inputs give unbatched results
    one = m.compute_contact_rollout(q[0], qd[0], tau[:, 0], DT, good, return_acceleration=True)
    full = m.compute_contact_rollout(q, qd, tau, DT, good, return_acceleration=True)
    assert all(a.shape == (2, n) and torch.equal(a, b[:, 0]) for a, b in zip(one, full))
    t1, tb = m.compute_contact_torques(q[0], qd[0], good), m.compute_contact_torques(q, qd, good)
    assert t1.tau.shape == (n,) and t1.force.shape == (9, 3) and all(torch.equal(a, b[0]) for a, b in zip(t1, tb))
    assert not full.q.requires_grad and full.q.grad_fn is None


def test_refusals_shapes_and_unbatched_inputs(cpu_library):
    check_refusals("cpu")


@pytest.mark.gpu
def test_gpu_refusals_shapes_and_unbatched_inputs():
    check_refusals(GPU)

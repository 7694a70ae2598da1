#!/usr/bin/env python3
"""Generate tests/golden/golden_rollout.npz: rollouts of the UNMODIFIED reference (its `compute_forward_dynamics`,
robot_model.py:487-624, called in a Python loop with the Euler integrators of compute_forward_dynamics_rollout) and the
reference autograd's gradients of a fixed scalar loss on the trajectory with respect to q0, qd0, tau and one learnable link
mass (PositiveScalar, rigid_body_params.py:26-43, started at 1.2 times the URDF's mass), for both rollouts of RUNS: under
"<robot>/grad/..." for the first (semi-implicit Euler, gravity) and "<robot>/grad_<key>/..." for every further one.

Every step passes a CLONE of tau[t]: the reference subtracts the damping torques from its `f` argument in place.

Run in the build container only (needs /root/reference):   python tests/golden/make_golden_rollout.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

B, T, DT = 8, 20, 1e-3
# (robot, reference urdf, the link whose mass is learnable, TAU_SCALE)
ROBOTS = [
    ("panda_no_gripper", "panda_description/urdf/panda_no_gripper.urdf", "panda_link3", 5.0),
    ("iiwa7", "kuka_iiwa/urdf/iiwa7.urdf", "iiwa_link_4", 5.0),
    ("allegro_left", "allegro/urdf/allegro_hand_description_left.urdf", "link_1.0", 0.01),
    ("fetch_arm_no_gripper", "fetch_description/urdf/fetch_arm_no_gripper.urdf", "elbow_flex_link", 1.0),
]
# (key, integrator, include_gravity, use_damping)
RUNS = [("semi_g1_d0", "semi_implicit_euler", True, False), ("euler_g0_d0", "euler", False, False)]
# (no damping: the joint damping of the shipped hand against its gram-scale links is far too stiff for an Euler step of 1 ms)


def rollout(model, q0, qd0, tau, integrator, gravity, damping):
    q, qd, qs, qds = q0, qd0, [], []
    for t in range(tau.shape[0]):
        qdd = model.compute_forward_dynamics(q, qd, tau[t].clone(), include_gravity=gravity, use_damping=damping)
        if integrator == "euler":
            q, qd = q + DT * qd, qd + DT * qdd
        else:
            qd = qd + DT * qdd
            q = q + DT * qd
        qs.append(q)
        qds.append(qd)
    return torch.stack(qs), torch.stack(qds)


def loss_of(q_traj, qd_traj):
    """The fixed scalar loss of the gradient fixtures (tests/test_rollout.py uses the same)."""
    return (q_traj[-1] ** 2).sum() + 0.1 * (qd_traj ** 2).mean()


def main():
    rm = ref_import.import_reference()
    import differentiable_robot_model.rigid_body_params as rbp
    torch.set_num_threads(1)
    out = {"B": np.asarray(B), "T": np.asarray(T), "dt": np.asarray(DT)}
    for name, rel, link, scale in ROBOTS:
        path = os.path.join(ref_import.reference_data_dir(), rel)
        with contextlib.redirect_stdout(io.StringIO()):
            model = rm.DifferentiableRobotModel(path)
            learn = rm.DifferentiableRobotModel(path)
        lim = model.get_joint_limits()
        lo = np.asarray([j["lower"] for j in lim]); hi = np.asarray([j["upper"] for j in lim])
        n = len(lim)
        rng = np.random.default_rng(11)
        q0 = rng.uniform(lo, hi, size=(B, n)).astype(np.float32)
        qd0 = rng.uniform(-1.0, 1.0, size=(B, n)).astype(np.float32)
        # torques of the scale the robot takes: +-TAU_SCALE Nm per step (a 10 g fingertip link reaches 1e5 rad/s^2 under 1 Nm)
        tau = rng.uniform(-scale, scale, size=(T, B, n)).astype(np.float32)
        out[name + "/q0"], out[name + "/qd0"], out[name + "/tau"] = q0, qd0, tau
        for key, integ, grav, damp in RUNS:
            with torch.no_grad():
                qt, qdt = rollout(model, torch.from_numpy(q0), torch.from_numpy(qd0), torch.from_numpy(tau), integ, grav, damp)
            assert torch.isfinite(qt).all() and torch.isfinite(qdt).all(), (name, key)
            out["%s/%s/q_traj" % (name, key)], out["%s/%s/qd_traj" % (name, key)] = qt.numpy(), qdt.numpy()
        body = learn._bodies[learn._name_to_idx_map[link]]
        mass = float(body.inertia.mass.detach().reshape(-1)[0]) if isinstance(body.inertia.mass, torch.Tensor) else float(body.inertia.mass())
        learn.make_link_param_learnable(link, "mass", rbp.PositiveScalar(init_param=torch.tensor(1.2 * mass)))
        mod = learn._bodies[learn._name_to_idx_map[link]].inertia.mass
        mk = lambda a: torch.tensor(a, requires_grad=True)
        out[name + "/grad/link"] = np.asarray(link)
        out[name + "/grad/l"] = mod.l.detach().numpy().copy()
        for i, (key, integ, grav, damp) in enumerate(RUNS):
            pre = name + ("/grad/" if i == 0 else "/grad_%s/" % key)
            q0t, qd0t, taut = mk(q0), mk(qd0), mk(tau)
            mod.l.grad = None
            qt, qdt = rollout(learn, q0t, qd0t, taut, integ, grav, damp)
            loss = loss_of(qt, qdt)
            assert torch.isfinite(loss), (name, key)
            loss.backward()
            out[pre + "loss"] = np.asarray(loss.item(), np.float64)
            out[pre + "q0"], out[pre + "qd0"], out[pre + "tau"] = q0t.grad.numpy(), qd0t.grad.numpy(), taut.grad.numpy()
            out[pre + "l_grad"] = mod.l.grad.numpy().copy()
            print("%-22s %-11s n=%2d |q_T - q0| max %.3g  loss %.5f  dL/dl %.4g" % (name, key, n, np.abs(qt[-1].detach().numpy() - q0).max(),
                                                                                 loss.item(), float(mod.l.grad)))
    np.savez_compressed(os.path.join(HERE, "golden_rollout.npz"), **out)


if __name__ == "__main__":
    main()

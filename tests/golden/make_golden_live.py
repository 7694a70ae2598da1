#!/usr/bin/env python3
"""Generate tests/golden/golden_live.npz and tests/golden/golden_live_loader.json: what the UNMODIFIED reference returns on its
CPU path for the comparisons of test_live_reference.py, test_oracle_golden.py::test_oracle_vs_live_reference,
test_reference_binding.py::test_binding_takes_the_references_own_loader_output and
test_rigid_body_params.py::test_same_parameters_same_matrix_as_the_reference, so that those tests run from the fixtures alone.

  golden_live.npz          every/<robot>/...  joint states (9 rows), FK and Jacobian of every link, inverse dynamics (4 flag
                                              combinations), non-linear effects, inertia matrix, forward dynamics
                           grad/<case>/...    one learn-kinematics and one learn-dynamics step with learnable link parameters:
                                              initial parameter values, losses, input and parameter gradients
                           oracle/<robot>/... 16 joint states and the reference's FK, Jacobian and inverse dynamics
                           rbp/<name>/...     the inertia parametrisations: parameters, matrices, initialisation from a matrix
  golden_live_loader.json  the per-link dicts the reference's URDF loader returns for panda_no_gripper, and the parent names

Needs the upstream source tree (ref_import.py: DRM_REFERENCE_ROOT) and a built libdrm_cpu.so:
    python tests/golden/make_golden_live.py
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
import ref_import  # noqa: E402

# (robot of this package, URDF under the reference's diff_robot_data)
EVERY = {"2link_robot": "2link_robot.urdf", "panda_no_gripper": "panda_description/urdf/panda_no_gripper.urdf",
         "iiwa7": "kuka_iiwa/urdf/iiwa7.urdf", "panda": "panda_description/urdf/panda.urdf",
         "jaco": "kinova_description/urdf/jaco.urdf", "allegro_left": "allegro/urdf/allegro_hand_description_left.urdf",
         "trifinger_edu": "trifinger_edu_description/trifinger_edu.urdf",
         "fetch_arm_no_gripper": "fetch_description/urdf/fetch_arm_no_gripper.urdf", "fetch": "fetch_description/urdf/fetch.urdf"}
EVERY_SEED, EVERY_ROWS = 20260927, 9
GRAD_CASES = [("iiwa7", "iiwa_link_2", "iiwa_link_ee"), ("panda", "panda_link3", "panda_virtual_ee_link"),
              ("allegro_left", "link_5.0", "link_7.0_tip")]
GRAD_SEED, GRAD_ROWS = 5, 12
ORACLE_CASES = [("panda_no_gripper", "panda_virtual_ee_link"), ("trifinger_edu", "finger_tip_link_120")]
ORACLE_SEED, ORACLE_ROWS = 11, 16
RBP_NAMES = ["Symm3DInertiaMatrixNet", "SymmPosDef3DInertiaMatrixNet", "CovParameterized3DInertiaMatrixNet"]
RBP_TARGET = [[0.031, 0.002, -0.004], [0.002, 0.045, 0.003], [-0.004, 0.003, 0.052]]
LOADER_ROBOT = "panda_no_gripper"


def reference_model(rm, robot):
    with contextlib.redirect_stdout(io.StringIO()):
        return rm.DifferentiableRobotModel(os.path.join(ref_import.reference_data_dir(), EVERY[robot]))


def states(model, B, seed):
    """q ~ U(joint limits), qd ~ U(+-1), qdd ~ U(+-2), f ~ U(+-1) from one torch generator (the live tests' sampling)."""
    lim = model.get_joint_limits()
    lo = torch.tensor([j["lower"] for j in lim]); hi = torch.tensor([j["upper"] for j in lim])
    g = torch.Generator().manual_seed(seed)
    n = len(lim)
    q = lo + (hi - lo) * torch.rand(B, n, generator=g)
    return q, torch.rand(B, n, generator=g) * 2 - 1, torch.rand(B, n, generator=g) * 4 - 2, torch.rand(B, n, generator=g) * 2 - 1


def every_public_method(rm, out):
    for robot in EVERY:
        ref = reference_model(rm, robot)
        q, qd, qdd, f = states(ref, EVERY_ROWS, EVERY_SEED)
        key = "every/%s/" % robot
        links = [b.name for b in ref._bodies][1:]
        out[key + "bodies"] = np.array([b.name for b in ref._bodies])
        out[key + "n_dofs"] = np.int64(ref._n_dofs)
        for name, t in (("q", q), ("qd", qd), ("qdd", qdd), ("f", f)):
            out[key + name] = t.numpy().copy()
        with torch.no_grad():
            for link in links:        # (per link: the reference returns some links' poses unbatched)
                rp, rq = ref.compute_forward_kinematics(q, link)
                rl, ra = ref.compute_endeffector_jacobian(q, link)
                for name, t in (("pos", rp), ("quat", rq), ("lin", rl), ("ang", ra)):
                    out["%s%s/%s" % (key, name, link)] = t.numpy().copy()
            for grav in (True, False):
                for damp in (True, False):
                    out[key + "tau_g%d_d%d" % (grav, damp)] = ref.compute_inverse_dynamics(
                        q, qd, qdd, include_gravity=grav, use_damping=damp).numpy()
            out[key + "nle"] = ref.compute_non_linear_effects(q, qd).numpy()
            out[key + "H"] = ref.compute_lagrangian_inertia_matrix(q).numpy()
            out[key + "qdd_fd"] = ref.compute_forward_dynamics(q, qd, f.clone(), include_gravity=True, use_damping=True).numpy()
        print("every   %-22s %2d links" % (robot, len(links)))


def learnable(rm, robot, link, names):
    """The reference model with learnable `names` on `link`, each module built right after torch.manual_seed(7)."""
    import differentiable_robot_model.rigid_body_params as ref_params
    ref = reference_model(rm, robot)
    mods = []
    for pname in names:
        torch.manual_seed(7)
        mod = {"trans": lambda: ref_params.UnconstrainedTensor(dim1=1, dim2=3),
               "rot_angles": lambda: ref_params.UnconstrainedTensor(dim1=1, dim2=3),
               "mass": lambda: ref_params.PositiveScalar(),
               "com": lambda: ref_params.UnconstrainedTensor(dim1=1, dim2=3)}[pname]()
        ref.make_link_param_learnable(link, pname, mod)
        mods.append((pname, mod))
    return ref, mods


def save_params(out, key, mods, what):
    for pname, mod in mods:
        for pn, p in mod.named_parameters():
            out["%s%s/%s/%s" % (key, what, pname, pn)] = (p.grad if what == "grad" else p.detach()).numpy().copy()


def gradients(rm, out):
    for robot, link, ee in GRAD_CASES:
        key = "grad/%s/" % robot
        ref, mods = learnable(rm, robot, link, ["trans", "rot_angles"])
        q, qd, qdd, _ = states(ref, GRAD_ROWS, GRAD_SEED)
        target = torch.rand(GRAD_ROWS, 3, generator=torch.Generator().manual_seed(1))
        for name, t in (("q", q), ("qd", qd), ("qdd", qdd), ("target", target)):
            out[key + name] = t.numpy().copy()
        save_params(out, key + "kin_", mods, "init")
        x = q.clone().requires_grad_(True)
        loss = torch.nn.functional.mse_loss(ref.compute_forward_kinematics(x, ee)[0], target)
        loss.backward()
        out[key + "kin_loss"] = np.float64(loss.item())
        out[key + "kin_dq"] = x.grad.numpy().copy()
        save_params(out, key + "kin_", mods, "grad")
        ref, mods = learnable(rm, robot, link, ["mass", "com"])
        want = torch.rand(GRAD_ROWS, ref._n_dofs, generator=torch.Generator().manual_seed(2))
        out[key + "want"] = want.numpy().copy()
        save_params(out, key + "dyn_", mods, "init")
        xs = [t.clone().requires_grad_(True) for t in (q, qd, qdd)]
        loss = torch.nn.functional.mse_loss(ref.compute_inverse_dynamics(*xs), want)
        loss.backward()
        out[key + "dyn_loss"] = np.float64(loss.item())
        for name, x in zip(("q", "qd", "qdd"), xs):
            out[key + "dyn_d" + name] = x.grad.numpy().copy()
        save_params(out, key + "dyn_", mods, "grad")
        print("grad    %-22s %s" % (robot, link))


def oracle_states(rm, out):
    from helpers import load_model, sample_states
    for robot, link in ORACLE_CASES:
        ref = reference_model(rm, robot)
        q, qd, qdd = sample_states(load_model(robot), ORACLE_ROWS, seed=ORACLE_SEED)
        key = "oracle/%s/" % robot
        out[key + "q"], out[key + "qd"], out[key + "qdd"] = q, qd, qdd
        with torch.no_grad():
            rp, rq = ref.compute_forward_kinematics(torch.from_numpy(q), link)
            rl, ra = ref.compute_endeffector_jacobian(torch.from_numpy(q), link)
            rt = ref.compute_inverse_dynamics(torch.from_numpy(q), torch.from_numpy(qd), torch.from_numpy(qdd))
        out[key + "pos"], out[key + "quat"], out[key + "lin"], out[key + "ang"] = rp.numpy(), rq.numpy(), rl.numpy(), ra.numpy()
        out[key + "tau"] = rt.numpy()
        print("oracle  %-22s %s" % (robot, link))


def inertia_parametrisations(out):
    import differentiable_robot_model.rigid_body_params as ref_rbp
    target = torch.tensor(RBP_TARGET)
    for name in RBP_NAMES:
        torch.manual_seed(1)
        kw = {} if name == "Symm3DInertiaMatrixNet" else {"bias": 1e-6}
        ref = getattr(ref_rbp, name)(init_param_std=0.2, **kw)
        ref2 = getattr(ref_rbp, name)(init_param=target.reshape(1, 3, 3), **kw)
        with torch.no_grad():
            out["rbp/%s/l" % name] = ref.l.numpy().copy()
            out["rbp/%s/matrix" % name] = ref().numpy().copy()
            out["rbp/%s/l_from_target" % name] = ref2.l.numpy().copy()


def _plain(v):
    if isinstance(v, torch.Tensor):
        return {"tensor": v.tolist(), "dtype": str(v.dtype).replace("torch.", "")}
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v


def loader_dicts():
    rm = ref_import.import_reference()
    um = reference_model(rm, LOADER_ROBOT)._urdf_model
    params = [um.get_body_parameters_from_urdf(i, link) for i, link in enumerate(um.robot.links)]
    parents = [None] + [um.get_name_of_parent_body(link.name) for link in um.robot.links[1:]]
    return {"robot": LOADER_ROBOT, "body_params": [_plain(p) for p in params], "parents": parents}


def main():
    rm = ref_import.import_reference()
    torch.set_num_threads(1)
    out = {}
    every_public_method(rm, out)
    gradients(rm, out)
    oracle_states(rm, out)
    inertia_parametrisations(out)
    np.savez_compressed(os.path.join(HERE, "golden_live.npz"), **out)
    with open(os.path.join(HERE, "golden_live_loader.json"), "w") as f:
        json.dump(loader_dicts(), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

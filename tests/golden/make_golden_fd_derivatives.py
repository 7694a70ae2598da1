#!/usr/bin/env python3
"""Generate tests/golden/golden_fd_derivatives.npz: the states the forward-dynamics derivatives are tested at
(tests/test_fd_derivatives.py) and, as a second yardstick, the UNMODIFIED reference's own float32 Jacobians of its
compute_forward_dynamics (robot_model.py:487-624) with respect to q, qd and f at those states.

Per robot, 128 rows: q uniform within the joint limits, qd ~ U(-1, 1) and f = the reference's compute_inverse_dynamics of
qdd ~ U(-2, 2) with gravity and damping on — torques that produce accelerations of order one (random torques throw a 10 g
fingertip to 1e5 rad/s^2 and make every float32 derivative rounding noise, see make_golden_grad_fd.py).

Jacobians: n backward passes of the batch sum of qdd[:, i] (rows do not interact, so the gradient of the sum holds every
row's own), include_gravity=True, use_damping=True, `f` cloned because the reference subtracts the damping torques from its
argument in place (robot_model.py:515-521).  All 128 rows for the robots with n <= 7, the first 32 rows of fetch and
allegro_left, none for iiwa7_allegro (23 DoFs).
    <robot>/q, qd, f [128, n]      <robot>/ref_dq, ref_dqd, ref_df [rows, n, n]   ([b, i, j] = d qdd_i / d x_j)

Run in the build container only (needs /root/reference):   python tests/golden/make_golden_fd_derivatives.py
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

ROWS = 128
# (robot, reference urdf, rows with reference Jacobians)
CASES = [
    ("panda_no_gripper", "panda_description/urdf/panda_no_gripper.urdf", 128),
    ("iiwa7", "kuka_iiwa/urdf/iiwa7.urdf", 128),
    ("fetch", "fetch_description/urdf/fetch.urdf", 32),
    ("allegro_left", "allegro/urdf/allegro_hand_description_left.urdf", 32),
    ("2link_robot", "2link_robot.urdf", 128),
    ("iiwa7_allegro", "kuka_iiwa/urdf/iiwa7_allegro.urdf", 0),
]


def generate(cases):
    rm = ref_import.import_reference()
    torch.set_num_threads(1)
    out = {}
    for name, rel, ref_rows in cases:
        torch.manual_seed(0)
        np.random.seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            model = rm.DifferentiableRobotModel(os.path.join(ref_import.reference_data_dir(), rel))
        lim = model.get_joint_limits()
        lo = np.asarray([j["lower"] for j in lim]); hi = np.asarray([j["upper"] for j in lim])
        n = len(lim)
        q = torch.tensor(np.random.uniform(lo, hi, size=(ROWS, n)), dtype=torch.float32)
        qd = torch.tensor(np.random.uniform(-1.0, 1.0, size=(ROWS, n)), dtype=torch.float32)
        qdd0 = torch.tensor(np.random.uniform(-2.0, 2.0, size=(ROWS, n)), dtype=torch.float32)
        with torch.no_grad():
            f = model.compute_inverse_dynamics(q, qd, qdd0, include_gravity=True, use_damping=True)
        out[name + "/q"], out[name + "/qd"], out[name + "/f"] = q.numpy(), qd.numpy(), f.numpy().copy()
        if ref_rows:
            qg, qdg, fg = (t[:ref_rows].clone().requires_grad_(True) for t in (q, qd, f))
            qdd = model.compute_forward_dynamics(qg, qdg, fg.clone(), include_gravity=True, use_damping=True)
            rows = [torch.autograd.grad(qdd[:, i].sum(), (qg, qdg, fg), retain_graph=i + 1 < n) for i in range(n)]
            for k, key in enumerate(("ref_dq", "ref_dqd", "ref_df")):
                out["%s/%s" % (name, key)] = torch.stack([r[k] for r in rows], 1).numpy()
        print("%-18s n=%2d rows=%d reference Jacobians on %d rows" % (name, n, ROWS, ref_rows))
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "golden_fd_derivatives.npz"), **generate(CASES))


if __name__ == "__main__":
    main()

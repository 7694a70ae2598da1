#!/usr/bin/env python3
"""Generate tests/golden/golden_id_derivatives.npz: the accelerations the inverse-dynamics derivatives are tested at
(tests/test_id_derivatives.py; q and qd are those of golden_fd_derivatives.npz) and, as the yardstick, the UNMODIFIED
reference's own float32 autograd Jacobians of its compute_inverse_dynamics with respect to q and qd at those states.

Per robot, 128 rows: qdd ~ U(-2, 2), seeded.

Jacobians: n backward passes of the batch sum of tau[:, i] (rows do not interact, so the gradient of the sum holds every
row's own), at two flag settings: include_gravity = use_damping = True ("on") and both False ("off").  All 128 rows for the
robots with n <= 7, the first 32 rows of fetch and allegro_left, the first 16 of iiwa7_allegro (23 DoFs).
    <robot>/qdd [128, n]     <robot>/ref_dq_on, ref_dqd_on, ref_dq_off, ref_dqd_off [rows, n, n]   ([b, i, j] = d tau_i / d x_j)

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_id_derivatives.py
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
    ("iiwa7_allegro", "kuka_iiwa/urdf/iiwa7_allegro.urdf", 16),
]


def generate(cases):
    rm = ref_import.import_reference()
    torch.set_num_threads(1)
    states = np.load(os.path.join(HERE, "golden_fd_derivatives.npz"), allow_pickle=False)
    out = {}
    for k, (name, rel, ref_rows) in enumerate(cases):
        with contextlib.redirect_stdout(io.StringIO()):
            model = rm.DifferentiableRobotModel(os.path.join(ref_import.reference_data_dir(), rel))
        q, qd = torch.from_numpy(states[name + "/q"][:ROWS]), torch.from_numpy(states[name + "/qd"][:ROWS])
        n = q.shape[1]
        qdd = torch.tensor(np.random.RandomState(1000 + k).uniform(-2.0, 2.0, size=(ROWS, n)), dtype=torch.float32)
        out[name + "/qdd"] = qdd.numpy()
        for tag, flag in (("on", True), ("off", False)):
            qg, qdg = (t[:ref_rows].clone().requires_grad_(True) for t in (q, qd))
            tau = model.compute_inverse_dynamics(qg, qdg, qdd[:ref_rows].clone(), include_gravity=flag, use_damping=flag)
            rows = [torch.autograd.grad(tau[:, i].sum(), (qg, qdg), retain_graph=i + 1 < n) for i in range(n)]
            out["%s/ref_dq_%s" % (name, tag)] = torch.stack([r[0] for r in rows], 1).numpy()
            out["%s/ref_dqd_%s" % (name, tag)] = torch.stack([r[1] for r in rows], 1).numpy()
        print("%-18s n=%2d rows=%d reference Jacobians on %d rows" % (name, n, ROWS, ref_rows))
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "golden_id_derivatives.npz"), **generate(CASES))


if __name__ == "__main__":
    main()

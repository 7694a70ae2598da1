"""examples/identify_dynamics_iiwa.py (closed-form identification from one call of compute_inverse_dynamics_regressor) runs on the CPU
device, small: the rank it reports is numpy.linalg.matrix_rank of the fp64 truth's stack at the same states (tests/test_regressor.py's
unit-parameter construction from the oracle), and its held-out torque error is within 8 x of the same solve fed that truth rounded to
float32 (floor 1e-6).  Both numbers are printed."""
import importlib
import os
import sys

import numpy as np

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_identification_on_the_cpu(cpu_library):
    from test_regressor import bodies_of, regressor_from_oracle
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("identify_dynamics_iiwa")
    (train, _), stats = mod.run(samples=384, held_out=128, device="cpu", verbose=False)

    def truth(model, q, qd, qdd, dtype=np.float32):
        inputs = [t.cpu().numpy() for t in (q, qd, qdd)]
        return regressor_from_oracle(model._spec, bodies_of(model), inputs, True, np.float64).astype(dtype)
    _, yard = mod.run(samples=384, held_out=128, device="cpu", regressor=truth, verbose=False)
    model = mod.DifferentiableKUKAiiwa(device="cpu")
    Y64 = truth(model, *train, dtype=np.float64)
    rank64 = int(np.linalg.matrix_rank(Y64.reshape(-1, Y64.shape[-1])))
    print("IDENT rank %d (fp64 truth %d) of %d columns; held-out error %.3e, with the rounded truth %.3e"
          % (stats["rank"], rank64, stats["columns"], stats["held_out_error"], yard["held_out_error"]))
    assert stats["columns"] == 10 * stats["bodies"] == 70
    assert stats["rank"] == rank64 < stats["columns"]
    assert stats["held_out_error"] <= 8 * max(yard["held_out_error"], 1e-6)

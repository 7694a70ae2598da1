"""examples/linearize_dynamics_panda.py (LQR about gravity-compensated postures from one call of
compute_forward_dynamics_derivatives) runs on the CPU device: with the gain every robot's state error shrinks below its start, without
it none does."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_lqr_from_one_linearisation_stabilises_on_the_cpu(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("linearize_dynamics_panda")
    q, stats = mod.run(batch=8, steps=300, device="cpu", verbose=False)
    assert q.shape == (8, 7)
    assert stats["residual_acc"] < 1e-3, stats               # the postures are equilibria under f*
    assert stats["worst_ratio"] < 0.1, stats
    _, free = mod.run(batch=8, steps=300, use_gain=False, device="cpu", verbose=False)
    assert free["end"] > free["start"] and free["best_ratio"] >= 1.0, free

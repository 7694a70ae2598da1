"""examples/inverse_kinematics_panda.py (many seeds per target, the best seed kept) runs on the CPU device and solves its targets."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_ik_example_solves_on_the_cpu(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("inverse_kinematics_panda")
    q, solved, stats = mod.run(targets=32, seeds=8, device="cpu", verbose=False)
    assert q.shape == (32, 7)
    assert stats["solved"] >= 0.9, stats
    assert stats["max_pos_err_solved"] <= 2e-4, stats

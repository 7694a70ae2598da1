"""examples/operational_space_control_panda.py (task-space PD control through compute_operational_space_dynamics) runs on the CPU
device and brings every end effector to its target."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_osc_example_reaches_its_targets_on_the_cpu(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("operational_space_control_panda")
    q, stats = mod.run(batch=8, steps=400, device="cpu", verbose=False)
    assert q.shape == (8, 7)
    assert stats["worst_ratio"] < 0.1, stats
    assert stats["end_err"] < 0.1 * stats["start_err"], stats

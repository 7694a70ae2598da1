"""examples/trajectory_opt_dynamics_panda.py (Adam on a torque sequence through compute_forward_dynamics_rollout) runs on the CPU
device and its cost decreases."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_trajectory_opt_example_learns_on_the_cpu(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("trajectory_opt_dynamics_panda")
    hist = mod.run(steps=20, iters=30, device="cpu", verbose=False)
    assert all(h == h for h in hist)
    assert hist[-1] < 0.8 * hist[0], hist

"""examples/payload_posture_panda.py (descent on the squared holding torque of a payload plus a soft penalty on the hand's position,
through compute_external_torques(..., differentiable_q=True) and the differentiable forward kinematics) runs on the CPU device: the
loss falls, and so does the holding torque."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_the_loss_falls_on_the_cpu(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("payload_posture_panda")
    stats = mod.run(batch=8, steps=40, device="cpu", verbose=False)
    assert stats["end"]["loss"] < 0.8 * stats["start"]["loss"], stats
    assert stats["end"]["effort"] < stats["start"]["effort"], stats
    assert stats["start"]["moved"] == 0.0 and stats["end"]["moved"] < 0.15, stats

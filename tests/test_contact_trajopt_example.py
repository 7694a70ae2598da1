"""examples/contact_trajopt_panda.py (a torque sequence per arm optimised through compute_contact_rollout(differentiable=True) towards a
hand pose resting on the plane) runs small on the CPU device: the loss falls and the hands end on the plane near their targets."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_the_loss_falls_and_the_hands_come_to_rest_on_the_plane(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("contact_trajopt_panda")
    stats = mod.run(batch=4, steps=60, dt=5e-3, iters=30, device="cpu", verbose=False)
    assert stats["last"] < 0.1 * stats["first"], stats
    assert stats["distance_last"] < 0.25 * stats["distance_first"], stats
    assert stats["touching"] == 1.0                                      # (every arm's gradient went through the plane's force)
    assert 0.0 < stats["height"] < mod.RADIUS + 0.01

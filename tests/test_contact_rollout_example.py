"""examples/contact_rollout_panda.py (the scenario of contact_simulation_panda.py with the contact law inside the rollout: one
compute_contact_rollout call per chunk of steps) runs small on the CPU device: the plane holds the arms up while the torque-free arms
without it fall through, and the rollout ends where the per-step example's loop ends."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_the_plane_holds_the_arms_while_the_free_arms_fall_through(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("contact_rollout_panda")
    stats = mod.run(batch=4, steps=600, chunk=150, dt=1e-3, device="cpu", verbose=False)      # (0.6 s, as the per-step example's test)
    assert stats["calls"] == 8
    assert stats["start"] > mod.PLANE_Z
    assert stats["lowest_without_contact"] < mod.PLANE_Z - 0.05          # (without the plane the arms swing through it)
    assert stats["lowest_with_contact"] > stats["lowest_without_contact"]
    assert stats["lowest_with_contact"] > mod.PLANE_Z - 0.05             # (the springs give a few centimetres under the impact)
    assert stats["lowest_ever_with_contact"] > mod.PLANE_Z - 0.05

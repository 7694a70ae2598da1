"""examples/collision_avoidance_panda.py (descent on the collision cost plus a soft end-effector penalty over a batch of postures) runs
small on the CPU device: fewer postures are in collision afterwards, and the end effectors have moved towards their goals."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_descent_leaves_fewer_postures_in_collision(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("collision_avoidance_panda")
    stats = mod.run(batch=64, steps=60, lr=0.03, device="cpu", verbose=False)
    assert stats["spheres"] == 16 and stats["pairs"] > 0
    assert stats["before"] > 0.1                       # (random postures: a fair share start in collision)
    assert stats["after"] < 0.5 * stats["before"]
    assert stats["miss"] < 0.25 and stats["cost"] == stats["cost"]

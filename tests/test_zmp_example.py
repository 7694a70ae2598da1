"""examples/zmp_margin_fetch.py (the tip-over margin of a Fetch swinging its arm, from one compute_base_wrench call per batch of knots)
runs on the CPU device at a small batch and prints finite margins; the static ZMP is the ground projection of the centre of mass, and a
trajectory at speed 0 has the static margin."""
import importlib
import math
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_margins_on_the_cpu(cpu_library, capsys):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("zmp_margin_fetch")
    stats = mod.run(knots=48, batch=20, speed=1.0, device="cpu", verbose=True)
    assert "worst ZMP margin" in capsys.readouterr().out
    assert all(math.isfinite(stats[k]) for k in ("margin", "static_margin", "static_zmp_to_com"))
    assert stats["margin"] <= max(mod.SUPPORT) and stats["static_margin"] <= max(mod.SUPPORT)
    # static: ZMP = (mc_x, mc_y) / M, the centre of mass over the floor, up to float32 rounding of lengths of the robot's size
    assert stats["static_zmp_to_com"] <= 1e-5
    still = mod.run(knots=48, batch=48, speed=0.0, device="cpu", verbose=False)
    assert abs(still["margin"] - still["static_margin"]) <= 1e-6

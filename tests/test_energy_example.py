"""examples/energy_budget_panda.py (the drift of T + V along torque-free, undamped rollouts, from one compute_energy call per
trajectory) runs on the CPU device: both integrators are first order, so the drift at dt / 4 lies below the drift at dt."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_drift_shrinks_with_the_step_on_the_cpu(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("energy_budget_panda")
    stats = mod.run(batch=4, horizon=0.04, dt=2e-3, device="cpu", verbose=False)
    assert set(stats["drift"]) == {"semi_implicit_euler", "euler"}
    for integrator, drift in stats["drift"].items():
        assert len(drift) == 3 and drift[2] < drift[0], (integrator, drift)

"""examples/momentum_observer_panda.py (a generalised-momentum observer fed by one compute_lagrangian_dynamics call per tick) runs on the
CPU device: the residual settles on the torque step injected into one joint and on zero on every other joint.

The tolerance.  After 300 ticks of 1 ms (the step at tick 100, observer gain 100 /s: two time constants of 10 ms would leave 13 %, twenty
leave e^-20) what remains is the observer's own discretisation: with the fp64 truth in place of the call — H and g from the oracle in
float64, C from Christoffel symbols of Richardson-combined central differences of the oracle's H, as tests/test_lagrangian.py builds
them — the same run ends 5.9e-5 N m from the injected torque (worst joint, worst robot).  With the call it ends 6.0e-5 N m away, 2e-6 from
the truth's run.  The bound is twice the truth's figure, 1.2e-4 N m: 6e-5 of the 2 N m step."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")
TRUTH_RUN_ERROR = 5.9e-5        # N m: the run with the fp64 truth in place of the call (module docstring)


def test_residual_settles_on_the_injected_torque_on_the_cpu(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("momentum_observer_panda")
    r, stats = mod.run(batch=4, steps=300, device="cpu", verbose=False)
    assert r.shape == (4, 7)
    assert stats["torque"] == 2.0 and abs(stats["estimate"] - 2.0) <= 2 * TRUTH_RUN_ERROR, stats
    assert stats["worst"] <= 2 * TRUTH_RUN_ERROR, stats           # every joint of every robot, the six without a torque included

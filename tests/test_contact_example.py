"""examples/contact_simulation_panda.py (Pandas falling onto a plane under a spring-damper contact law: one compute_link_motion launch,
one compute_external_torques launch and one forward-dynamics call per step) runs small on the CPU device: the plane holds the arms
up, and the contact work accumulated at the links, sum f . v dt, equals the one accumulated at the joints, sum tau_ext . qd dt."""
import importlib
import os
import sys

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")


def test_the_plane_holds_the_arms_and_the_two_works_agree(cpu_library):
    if EX not in sys.path:
        sys.path.insert(0, EX)
    mod = importlib.import_module("contact_simulation_panda")
    stats = mod.run(batch=4, steps=1200, dt=5e-4, device="cpu", verbose=False)
    assert stats["start"] > mod.PLANE_Z
    assert stats["lowest_without_contact"] < mod.PLANE_Z - 0.05          # (without the plane the arms swing through it)
    assert stats["lowest_with_contact"] > stats["lowest_without_contact"]
    assert stats["lowest_with_contact"] > mod.PLANE_Z - 0.05             # (the springs give a few centimetres under the impact)
    # the two launches are adjoint: per step f . v == tau_ext . qd to float32 rounding of the terms, and so are the sums (8: the
    # project's margin on a float32 rounding bound; the terms are sum |f . v| dt + sum |tau_ext . qd| dt)
    terms = stats["work_terms"]
    assert (terms > 0).all(), "every arm touched the plane"
    assert ((stats["work_links"] - stats["work_joints"]).abs() <= 8 * 2.0 ** -23 * terms).all()

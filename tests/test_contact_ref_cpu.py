"""The fp64 reference decode of the contact-force read-out (tests/contact_ref.py) against the oracle itself, on the CPU.

The decode turns constraint-row forces into per-contact forces and per-body wrenches.  The oracle has no such read-out, but it has
J and efc_force: on the six dofs of a free root, J' efc_force IS the total contact force on the root's tree (world axes) and the total
torque about the root body's origin (root axes).  Three identities pin the decode's row order, signs, friction factors, frame
orientation and reference points:
  (1) sum of the bodies' forces (world excluded)                       == (J' efc_force)[0:3]
  (2) their torques, moved to the root body's origin, in its frame     == (J' efc_force)[3:6]
  (3) all bodies including the world sum to zero, force and torque about a common point (every contact acts on two bodies)
each to 1e-12 relative to max(1, max |efc_force|): fp64 sums of at most a few hundred terms of that size (measured: 1.2e-15).
"""
import os

import numpy as np
import pytest

import contact_ref
from kernel_models import rollout_states
from oracle_lib import ASSETS, HUMANOID_HBM, TEAM_HBM, Oracle, golden_states, load_state, MODELS_DIR as MODELS

TOL = 1e-12


def worst_identity(o, states, ctrls):
    """(largest deviation of the three identities, states with contact rows, per-state (f, contacts)) over the states"""
    worst, with_rows, outs = 0.0, 0, []
    for s, c in zip(states, ctrls):
        load_state(o, s, np.asarray(c, dtype=np.float64))
        o.forward()
        f, w, con = contact_ref.oracle_readout(o)
        worst = max(worst, contact_ref.root_checks(o, w))
        with_rows += any(k["efc_address"] >= 0 for k in con)
        outs.append((f, con))
    return worst, with_rows, outs


@pytest.mark.parametrize("solver,iterations", [(0, 50), (2, 100)], ids=["pgs50", "newton100"])
def test_decode_reproduces_root_forces_on_golden_states(solver, iterations):
    st, ctrl, ncon = golden_states()
    o = Oracle(HUMANOID_HBM)
    o.set_opt(solver=solver, iterations=iterations)
    idx = np.flatnonzero(ncon > 0)
    assert len(idx) == 102
    worst, with_rows, outs = worst_identity(o, st[idx], ctrl[idx])
    dims = {int(k["dim"]) for _, con in outs for k in con}
    print("\ngolden states, solver %d: worst identity deviation %.2e over %d states with contact rows, condims %s" % (solver, worst, with_rows, sorted(dims)))
    assert with_rows >= 90 and dims == {1, 3}
    assert worst <= TOL, worst


def test_decode_reproduces_root_forces_on_the_team_robot():
    """condim 6: torsional and rolling rows, mesh hulls on a height field"""
    o = Oracle(TEAM_HBM)
    states, ctrls = contact_ref.team_states(o)
    worst, with_rows, outs = worst_identity(o, states, ctrls)
    six = sum(any(k["dim"] == 6 and k["efc_address"] >= 0 for k in con) for _, con in outs)
    spin = max((float(np.abs(f[:, 3:6]).max(initial=0.0)) for f, _ in outs), default=0.0)
    print("\nteam robot: worst %.2e, %d of %d states with a condim-6 contact, largest torsional / rolling entry %.3e" % (worst, six, len(states), spin))
    assert six >= 8 and spin > 0.0
    assert worst <= TOL, worst


@pytest.mark.parametrize("asset", ["team_robot_plane.hbm", "humanoid27_hfield.hbm"])
def test_decode_reproduces_root_forces_on_the_other_assets(asset):
    o = Oracle(os.path.join(ASSETS, asset))
    states, ctrls = rollout_states(o, steps=400, every=25, seed=5, keyframe=0 if asset.startswith("team") else -1)
    worst, with_rows, _ = worst_identity(o, states, ctrls)
    print("\n%s: worst %.2e, %d of %d states with contact rows" % (asset, worst, with_rows, len(states)))
    assert with_rows >= 4
    assert worst <= TOL, worst


def test_resting_ball_carries_its_weight(hbmod, tmp_path):
    """A ball at rest on the plane: the decoded normal force is m g.  Newton's second law holds exactly in the oracle,
    m qacc_z = f_n - m g, so what separates f_n from m g is the acceleration the settling ball still has at that step: the test asserts
    the identity to fp64 rounding and that the ball has settled (|qacc_z| <= 1e-6 g), which together put f_n within 1e-6 of m g."""
    m = hbmod.Model.load(os.path.join(MODELS, "ball_plane.xml"))
    m.set_opt(solver=2, iterations=100)
    p = str(tmp_path / "ball.hbm")
    m.save(p)
    o = Oracle(p)
    o.reset()
    o.step(2000)
    o.forward()
    f, w, con = contact_ref.oracle_readout(o)
    mass, g = float(o.marr("body_mass")[1]), -float(o.marr("gravity")[2])
    az = float(o.qacc[2])
    assert len(con) == 1 and con[0]["dim"] == 3
    print("\nresting ball: f_n %.12g, m g %.12g, qacc_z %.3e, tangential %.3e" % (f[0, 0], mass * g, az, np.abs(f[0, 1:3]).max()))
    assert abs(f[0, 0] - mass * (g + az)) <= 1e-10 * mass * g
    assert abs(az) <= 1e-6 * g
    assert abs(f[0, 0] - mass * g) <= 1.1e-6 * mass * g
    assert np.allclose(w[1, 0:3], [0.0, 0.0, f[0, 0]], atol=1e-9 * mass * g) and np.allclose(w[0, 0:3], -w[1, 0:3], atol=0)

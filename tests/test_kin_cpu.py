"""The whole-body kinematics read-out without a GPU: the reference's velocity formula (tests/kin_ref.py) against central differences of
the oracle's own poses, and the presence of the C-ABI and Python entry points (tests/test_cabi.py checks that every declared symbol is
exported and that the header compiles as C)."""
import os
import re

import numpy as np
import pytest

import kin_ref
import rk4_ref
from kernel_models import oracle_for, rollout_states
from oracle_lib import HUMANOID_HBM, ROOT, Oracle, load_state

EPS = 1e-7
FD_BOUND = 1e-6  # (central differences at eps 1e-7 in fp64: truncation ~ eps^2 |x'''|, rounding ~ 1e-16 |x| / eps = 1e-9 |x|)


def _poses(o, qpos):
    s = np.concatenate([[0.0], qpos, np.zeros(2 * o.nv)])
    load_state(o, s, np.zeros(o.nu))
    o.forward()
    return o.xipos.reshape(-1, 3).copy(), o.ximat.reshape(-1, 3, 3).copy()


def _fd_errors(o, states):
    nq, nv = o.nq, o.nv
    lin, ang = [], []
    for s in states:
        qpos, qvel = s[1:1 + nq], s[1 + nq:1 + nq + nv]
        load_state(o, s, np.zeros(o.nu))
        o.forward()
        vel = kin_ref.reference(o)["vel"]
        xp, mp = _poses(o, rk4_ref.integrate_pos(o, qpos, qvel, EPS))
        xm, mm = _poses(o, rk4_ref.integrate_pos(o, qpos, qvel, -EPS))
        x0, m0 = _poses(o, rk4_ref.integrate_pos(o, qpos, qvel, 0.0))
        v_fd = (xp - xm) / (2 * EPS)
        W = np.einsum("bij,bkj->bik", (mp - mm) / (2 * EPS), m0)  # dR/dt R' = [omega]x
        w_fd = np.stack([W[:, 2, 1] - W[:, 1, 2], W[:, 0, 2] - W[:, 2, 0], W[:, 1, 0] - W[:, 0, 1]], axis=1) / 2
        lin.append(np.abs(vel[:, 3:6] - v_fd).max() / max(1.0, np.abs(v_fd).max()))
        ang.append(np.abs(vel[:, 0:3] - w_fd).max() / max(1.0, np.abs(w_fd).max()))
    return max(lin), max(ang)


def test_reference_velocity_humanoid():
    o = Oracle(HUMANOID_HBM)
    states, _ = rollout_states(o, steps=200, every=20)
    lin, ang = _fd_errors(o, states)
    print("humanoid27: linear %.3g angular %.3g" % (lin, ang))
    assert lin <= FD_BOUND and ang <= FD_BOUND


def test_reference_velocity_bush(hbmod, tmp_path):
    m, _, o = oracle_for(hbmod, kin_ref.bush_xml((11, 11, 11, 11), 2), tmp_path)
    assert (m.nbody, m.nv) == (46, 32)
    states, _ = rollout_states(o, steps=120, every=20)
    assert np.abs(states[:, 1 + o.nq:1 + o.nq + o.nv]).max() > 0.1
    lin, ang = _fd_errors(o, states)
    print("bush: linear %.3g angular %.3g" % (lin, ang))
    assert lin <= FD_BOUND and ang <= FD_BOUND


def test_header_declares_the_readout():
    h = open(os.path.join(ROOT, "include", "hb.h")).read()
    for fn in ("hb_kinematics", "hb_kinematics_dev", "hb_kinematics_states", "hb_kinematics_states_dev"):
        assert re.search(r"\bint %s\(hb_batch\* b," % fn, h), fn
    assert re.search(r"HB_TUNE_FOLD, HB_TUNE_KIN_PACK, HB_TUNE_COUNT", h)


def test_python_entry_points(hbmod):
    hb = hbmod
    for name in ("kinematics", "kinematics_dev", "kinematics_states", "kinematics_states_dev"):
        assert callable(getattr(hb.Batch, name)), name
    for name in ("body_poses", "body_velocities", "geom_poses"):
        assert callable(getattr(hb.VecEnv, name)), name
    assert hb.Batch.TUNE["kin_pack"] == 10
    q = np.array([[1.0, 0, 0, 0], [np.sqrt(0.5), 0, 0, np.sqrt(0.5)]])
    np.testing.assert_allclose(hb.quat_to_mat(q), kin_ref.quat_to_mat(q), atol=1e-15)

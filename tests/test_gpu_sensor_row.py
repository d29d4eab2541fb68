"""Every part of a sensor row is where Batch.sensor_layout says (hb_device.hpp: sensor_row(); hb_step.hip: the three write sites) on the GPU.

One spec with every part and uneven counts against nine specs holding one of its parts alone, on the same states and controls, T = 3 steps
in one hb_rollout_sensors call: the slice sensor_layout names for a part is the whole row of that part's own spec, bit for bit
(np.array_equal).  A part written at a shifted offset, with a neighbour's count or a neighbour's table misses this by the values
themselves.  The kernels differ between the runs - the full spec takes the kernel with the body-acceleration read-out, a spec without
such parts its twin without - and compute a part's entries with the same arithmetic (test_gpu_body_acc.py: test_nothing_else_moves).
  humanoid27, PGS: one launch covers the T steps (the kernel strides through the rows by row.stride)
  team robot:      a staged step, one launch chain per step: launch_step advances sensor.out by row.stride per step.  It has kernels
                   with the body-acceleration read-out (step_lib.ACC_KERNELS, the names select_step gives), so the spec keeps those parts.
"""
import numpy as np
import pytest

import contact_ref
from step_lib import ACC_KERNELS

pytestmark = pytest.mark.gpu
N, T = 4, 3
OFF = (0.05, 0.02, -0.03)
# (bodies of humanoid27.hbm: torso 1, foot_right 7, foot_left 10; states 6..9 of the golden steps: a few steps into a fall, both feet down)
HUMANOID = dict(case="humanoid27_pgs", states=slice(6, 10), feet=(7, 10),
                full=dict(framepos_bodies=(1, 7, 10), offsets=[None, OFF, None], subtree_body=1, axes=((2, 0), (10, 2)), linvel_bodies=(7,), subtreelinvel_bodies=(3, 10),
                          touch_bodies=(7, 10), contactforce_bodies=(10,), imu=((1, (0.0, 0.0, 0.0)), (7, OFF)), frameacc_bodies=(10,)))
# (the team robot: body 1 the trunk, four limbs 3-4-5, 6-7-8, 9-10-11, 12-13-14; states 1..4 of contact_ref.team_states: lying on the floor)
TEAM = dict(case="team_robot", states=slice(1, 5), feet=(14, 5),
            full=dict(framepos_bodies=(1, 14, 5), offsets=[None, OFF, None], subtree_body=1, axes=((2, 0), (8, 2)), linvel_bodies=(14,), subtreelinvel_bodies=(3, 12),
                      touch_bodies=(14, 5), contactforce_bodies=(14,), imu=((1, (0.0, 0.0, 0.0)), (14, OFF)), frameacc_bodies=(11,)))
# the arguments of Batch.sensor_spec that make up each part
PART_ARGS = dict(framepos=("framepos_bodies", "offsets"), subtree=("subtree_body",), axis=("axes",), linvel=("linvel_bodies",), sub=("subtreelinvel_bodies",),
                 touch=("touch_bodies",), cfrc=("contactforce_bodies",), imu=("imu",), facc=("frameacc_bodies",))


def _rows(hbmod, gpu, m, st, ctrl, spec):
    b = hbmod.Batch(m, len(st), gpu)
    b.set_state(hbmod.STATE_INTEGRATION, st)
    rows, _ = b.rollout_sensors(ctrl, spec)
    out = rows, b.get_state(hbmod.STATE_INTEGRATION), b.last_kernel()
    b.close()
    return out


@pytest.mark.parametrize("cfg", [HUMANOID, TEAM], ids=["humanoid27_pgs", "team_robot"])
def test_each_part_is_where_the_layout_says(hbmod, gpu, cfg):
    m, _, st, _, _ = contact_ref.make_case(hbmod, cfg["case"], None)
    st = st[cfg["states"]]
    assert len(st) == N
    ctrl = np.random.default_rng(11).uniform(-0.5, 0.5, (T, N, m.nu)).astype(np.float32)
    full = hbmod.Batch.sensor_spec(**cfg["full"])
    lay = hbmod.Batch.sensor_layout(full)
    assert [lay[p][1] for p in hbmod.engine.SENSOR_PARTS] == [9, 6, 6, 3, 6, 2, 3, 12, 6] and lay["width"] == 53  # uneven counts, every part
    rows, end, kernel = _rows(hbmod, gpu, m, st, ctrl, full)
    assert rows.shape == (T, N, 53) and np.isfinite(rows).all() and kernel in ACC_KERNELS[cfg["case"]], kernel
    o, c = lay["touch"]
    assert (rows[:, :, o:o + c] > 0).any(axis=(0, 1)).all()  # both touch bodies are in contact in some env-step
    seen = 0
    for part in hbmod.engine.SENSOR_PARTS:
        alone = hbmod.Batch.sensor_spec(**{k: cfg["full"][k] for k in PART_ARGS[part]})
        one, end1, _ = _rows(hbmod, gpu, m, st, ctrl, alone)
        o, c = lay[part]
        assert hbmod.Batch.sensor_layout(alone)[part] == (0, c) and one.shape == (T, N, c), part
        assert np.array_equal(rows[:, :, o:o + c], one), (part, float(np.abs(rows[:, :, o:o + c] - one).max()))
        assert np.abs(one).max() > 0 and np.array_equal(end, end1), part  # (the same three steps)
        seen += c
    assert seen == lay["width"]

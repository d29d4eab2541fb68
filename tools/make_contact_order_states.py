#!/usr/bin/env python3
"""Generate tests/golden/contact_order_states.npz — the steady-regime states of
tests/test_gpu_timed_kernels.py::test_one_step_parity_in_both_contact_orders.

PROVENANCE: produced by THIS repository's fp64 oracle (oracle/mjstep_oracle.c), not by MuJoCo.  For each contact order (0: geom-major,
1: body-pair-major, hb_model_pair_order) the oracle rolls envs 1, 4 and 6 of the benchmark workload (Halton controls, Halton-perturbed
reset) through 700 steps on the model in that order and records every 8th state from step 300 on: fallen humanoids, self collisions,
several bodies on the floor.  A rollout that long amplifies the last bit of every operation, so the states it reaches depend on the
instruction set the oracle was compiled for (oracle/Makefile builds it for the host CPU); stored, the test steps the same states on
every host.

Keys, for order k in (0, 1): state<k> [150, 1 + nq + nv + nv] float32 (time | qpos | qvel | qacc_warmstart, rounded to float32 as
hb_set_state leaves them on the device), ctrl<k> [150, nu] float32.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle_lib import GOLDEN, HUMANOID_HBM, Oracle  # noqa: E402

ENVS = (1, 4, 6)
STEPS = 700
FIRST, EVERY = 300, 8


def states_for_order(hb, order, tmp):
    m = hb.Model.load(HUMANOID_HBM)
    assert m.pair_order(order) == order
    p = os.path.join(tmp, "order%d.hbm" % order)
    m.save(p)
    o = Oracle(p)
    states, ctrls = [], []
    for e in ENVS:
        o.init_env(e)
        for t in range(STEPS):
            c = o.ctrl_env(t, e)
            o.ctrl[:] = c
            if t >= FIRST and t % EVERY == 0:
                states.append(np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart])); ctrls.append(c.copy())
            o.step()
    return np.array(states).astype(np.float32), np.array(ctrls, dtype=np.float32)


def main():
    import humanoid_mujoco_amd as hb
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for order in (0, 1):
            out["state%d" % order], out["ctrl%d" % order] = states_for_order(hb, order, tmp)
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, "contact_order_states.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

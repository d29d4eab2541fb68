"""The sampling actor without a GPU: the fp64 reference's heads against closed forms, the statistics of the reference draws the GPU
tests compare the device with, and the layout of the two C structs against their ctypes mirrors."""
import ctypes
import os
import subprocess

import numpy as np

import actor_ref as ar
from conftest import ROOT

# the collection of tests/test_gpu_collect.py: seed, env offset, envs, steps, actuators
SEED, OFFSET, N_ENV, T, NU = 2024, 0, 64, 8, 21


def test_zero_weights_give_the_bias():
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(5, 48))
    sizes = [48, 40, 24, 21]
    ws = [np.zeros((a, c), np.float32) for a, c in zip(sizes[:-1], sizes[1:])]
    bs = [np.zeros(c, np.float32) for c in sizes[1:]]
    bs[-1] = rng.uniform(-1, 1, 21).astype(np.float32)
    out = ar.actor(obs, ws, bs, ar.GAUSSIAN, log_std=np.full(21, -1.0), eps=np.ones((5, 21)))
    assert np.array_equal(out["mean"], np.broadcast_to(bs[-1].astype(np.float64), (5, 21)))
    assert np.allclose(out["action"], out["mean"] + np.exp(-1.0), rtol=0, atol=1e-15)
    out0 = ar.actor(obs, ws, bs, ar.DETERMINISTIC)
    assert np.array_equal(out0["action"], np.tanh(bs[-1].astype(np.float64)) * np.ones((5, 1))) and np.array_equal(out0["mean"], out0["action"])
    assert not out0["eps"].any()


def test_squashed_head_clamps_log_std_and_squashes():
    obs = np.zeros((3, 48))
    ws = [np.zeros((48, 42), np.float32)]
    b = np.zeros(42, np.float32)
    b[:21] = 0.25
    b[21:28], b[28:35], b[35:] = -50.0, 7.0, -0.5  # below the clamp, above it, inside
    eps = np.full((3, 21), 0.5)
    out = ar.actor(obs, ws, [b], ar.SQUASHED, eps=eps)
    assert np.array_equal(out["log_std"][0], np.r_[np.full(7, -20.0), np.full(7, 2.0), np.full(7, -0.5)])
    assert np.array_equal(out["mean"], np.full((3, 21), 0.25))
    want = np.tanh(0.25 + np.exp(np.r_[np.full(7, -20.0), np.full(7, 2.0), np.full(7, -0.5)]) * 0.5)
    assert np.allclose(out["action"][1], want, rtol=0, atol=1e-15) and np.abs(out["action"]).max() < 1.0


def test_deterministic_gives_zero_eps_for_every_head():
    rng = np.random.default_rng(1)
    obs = rng.normal(size=(4, 48))
    for head, last in ((ar.DETERMINISTIC, 21), (ar.GAUSSIAN, 21), (ar.SQUASHED, 42)):
        ws, bs = ar.make_actor([48, 40, 24, last], seed=3)
        out = ar.actor(obs, ws, bs, head, log_std=np.zeros(21), eps=rng.normal(size=(4, 21)), deterministic=True)
        assert not out["eps"].any()
        y = ar.network(obs, ws, bs, head)
        assert np.array_equal(out["action"], np.tanh(y[:, :21]) if head == ar.SQUASHED else y)


def test_reference_draw_statistics():
    """The 8 x 64 x 21 draws of the GPU test's collection (same seed, offset, counters): a standard normal sample, no repeated row."""
    eps = ar.draws(SEED, OFFSET, N_ENV, NU, 0, T)
    n = eps.size
    assert n == 10752
    mean, var = eps.mean(), eps.var()
    print("actor draws: mean %.4f (bound %.4f), var - 1 %.4f (bound %.4f), max |eps| %.3f" % (mean, 5 / np.sqrt(n), var - 1, 5 * np.sqrt(2 / n), np.abs(eps).max()))
    assert abs(mean) <= 5 / np.sqrt(n) and 5 / np.sqrt(n) < 0.0483
    assert abs(var - 1) <= 5 * np.sqrt(2 / n) and 5 * np.sqrt(2 / n) < 0.0682
    rows = eps.reshape(T * N_ENV, NU)
    assert len({r.tobytes() for r in rows}) == len(rows)
    assert np.abs(eps).max() < 5.9  # (Box-Muller on a 24-bit uniform: sqrt(-2 ln 2^-25))
    # a second call continues the counter: other numbers; another env offset: the rows of the envs it covers
    again = ar.draws(SEED, OFFSET, 4, NU, T, 1)
    assert not np.array_equal(again[0], eps[0, :4])
    assert np.array_equal(ar.draws(SEED, 27, 3, NU, 0, 1)[0], eps[0, 27:30])


def test_ctypes_structs_match_the_header(hbmod, tmp_path):
    """hb_actor_config and hb_collect_out have the size and the field offsets include/hb.h gives them (as tests/test_cabi.py checks the
    older structs, whose list is fixed)."""
    import humanoid_mujoco_amd.engine as eng
    pairs = [("hb_actor_config", eng.HbActorConfig), ("hb_collect_out", eng.HbCollectOut)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hb.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['printf("heads %d %d %d\\n", HB_ACTOR_DETERMINISTIC, HB_ACTOR_GAUSSIAN, HB_ACTOR_SQUASHED);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    rows = [l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    out = {r[0]: r[1:] for r in rows}
    for cname, cls in pairs:
        assert int(out[cname][0]) == ctypes.sizeof(cls), (cname, out[cname], ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            assert int(out["%s.%s" % (cname, fname)][0]) == getattr(cls, fname).offset, (cname, fname)
    assert [int(x) for x in out["heads"]] == [eng.ACTOR_DETERMINISTIC, eng.ACTOR_GAUSSIAN, eng.ACTOR_SQUASHED] == [ar.DETERMINISTIC, ar.GAUSSIAN, ar.SQUASHED]
    assert eng.RS_ACTOR == ar.RS_ACTOR == 32
    header = open(os.path.join(ROOT, "include", "hb.h")).read()
    assert "RS_ACTOR = 32" in header

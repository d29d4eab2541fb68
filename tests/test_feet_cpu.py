"""Foot-contact terms without a GPU (include/hb.h: hb_env_feet): tests/feet_ref.py on hand-built wrenches and records, every refusal
that needs no device with its message, the documented defaults, and the ctypes mirror against the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import feet_ref
from oracle_lib import ROOT

FOOT_R, FOOT_L, TORSO = 7, 10, 1


def _cfg(hbmod, model, **kw):
    import humanoid_mujoco_amd.engine as eng
    c = eng.HbEnvFeet()
    assert hbmod.lib().hb_env_default_feet(model._h, ctypes.byref(c)) == 0
    c.set_bodies(bodies=kw.pop("bodies", (FOOT_R, FOOT_L)), penalised=kw.pop("penalised", ()), terminal=kw.pop("terminal", ()))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _error(hbmod):
    return hbmod.lib().hb_error().decode()


def _wrench(**forces):
    w = np.zeros((28, 6), dtype=np.float32)
    for body, f in forces.items():
        w[int(body[1:])][:3] = f
    return w


@pytest.fixture
def C(hbmod, humanoid_model):
    # weights that make every term readable: air 2 per second, 0.5 per N over 100 N, stumble -3 at a ratio of 2, collision -7
    return _cfg(hbmod, humanoid_model, w_air_time=2.0, air_time_target=0.25, w_force=0.5, force_max=100.0, w_stumble=-3.0, stumble_ratio=2.0, w_collision=-7.0,
                air_gate=0, penalised=(4, 5), terminal=(TORSO,))


def test_library_exports_the_entry_points(hbmod):
    L = ctypes.CDLL(hbmod.LIB_PATH)
    for name in ("hb_env_default_feet", "hb_env_feet_check", "hb_env_feet_configure", "hb_env_get_feet"):
        assert hasattr(L, name), name


def test_touchdown_pays_once(C):
    t_last, mask = feet_ref.start_record(C, 0.0)
    assert mask == 3 and np.array_equal(t_last, np.zeros(2, np.float32))
    # in the air: both bits clear, t_last stays
    r = feet_ref.evaluate(C, _wrench(), np.float32(0.5), t_last, mask, (0, 0))
    assert r["mask"] == 0 and r["reward"] == 0.0 and np.array_equal(r["t_last"], t_last)
    # the right foot lands at t = 1: air = 1 - 0 = 1 s, pays 2 * (1 - 0.25)
    w = _wrench(b7=(0, 0, 50.0))
    r1 = feet_ref.evaluate(C, w, np.float32(1.0), r["t_last"], r["mask"], (0, 0))
    assert r1["touchdown"] == [True, False] and r1["air"] == pytest.approx(1.5) and r1["mask"] == 1 and r1["t_last"][0] == np.float32(1.0) and r1["t_last"][1] == 0
    # the next step: still down, nothing paid, t_last follows the time
    r2 = feet_ref.evaluate(C, w, np.float32(1.005), r1["t_last"], r1["mask"], (0, 0))
    assert r2["touchdown"] == [False, False] and r2["air"] == 0.0 and r2["reward"] == 0.0 and r2["t_last"][0] == np.float32(1.005)
    # a standing start pays nothing for the first step
    r3 = feet_ref.evaluate(C, _wrench(b7=(0, 0, 50.0), b10=(0, 0, 50.0)), np.float32(0.005), t_last, mask, (0, 0))
    assert r3["reward"] == 0.0 and r3["mask"] == 3
    # air is one float32 subtraction
    r4 = feet_ref.evaluate(C, w, np.float32(0.7), np.array([0.1, 0.0], np.float32), 0, (0, 0))
    assert r4["air"] == 2.0 * (float(np.float32(np.float32(0.7) - np.float32(0.1))) - 0.25)


def test_gate(hbmod, humanoid_model, C):
    C.air_gate, C.air_cmd_min = 1, 0.5
    w = _wrench(b7=(0, 0, 50.0))
    args = (np.float32(1.0), np.zeros(2, np.float32), 0)
    assert feet_ref.evaluate(C, w, *args, (0.0, 0.5))["air"] == 0.0       # |cmd| = 0.5 exactly: closed
    assert not feet_ref.gate(C, (np.float32(0.5), 0.0))                   # exactly at the bound: closed
    assert feet_ref.evaluate(C, w, *args, (0.5, 0.1))["air"] == pytest.approx(1.5)
    closed = feet_ref.evaluate(C, w, *args, (0.0, 0.0))
    assert closed["air"] == 0.0 and closed["mask"] == 1 and closed["touchdown"] == [True, False]  # (the record moves all the same)
    C.air_gate = 0
    assert feet_ref.evaluate(C, w, *args, (0.0, 0.0))["air"] == pytest.approx(1.5)


def test_threshold_is_exclusive(C):
    C.contact_threshold = 5.0
    assert not feet_ref.in_contact(C, (3.0, 4.0, 0.0))          # n2 = 25 = thr^2: not in contact
    assert feet_ref.in_contact(C, (3.0, 4.0, np.float32(2e-3)))  # 25 + 4e-6 rounds above 25
    assert not feet_ref.in_contact(C, (3.0, 4.0, np.float32(1e-5)))  # 25 + 1e-10 rounds to 25 in float32
    r = feet_ref.evaluate(C, _wrench(b7=(3.0, 4.0, 0.0), b4=(0, 5.0, 0), b1=(5.0, 0, 0)), np.float32(1.0), np.zeros(2, np.float32), 0, (0, 0))
    assert r["mask"] == 0 and r["collisions"] == 0 and not r["terminated"]


def test_stumble_at_the_ratio(C):
    rec = (np.float32(1.0), np.full(2, 1.0, np.float32), 3)
    assert not feet_ref.evaluate(C, _wrench(b7=(20.0, 0, 10.0)), *rec, (0, 0))["stumble"]      # planar^2 = 400 = 4 * 100: exactly at the ratio
    at = feet_ref.evaluate(C, _wrench(b7=(20.0, 0, 10.0)), *rec, (0, 0))
    assert at["stumble_term"] == 0.0
    over = feet_ref.evaluate(C, _wrench(b7=(20.5, 0, 10.0), b10=(0, 21.0, 10.0)), *rec, (0, 0))
    assert over["stumble"] and over["stumble_term"] == -3.0 and over["reward"] == -3.0          # once, though both feet stumble
    assert not feet_ref.evaluate(C, _wrench(b7=(0.5, 0, 0.1)), *rec, (0, 0))["stumble"]        # below the contact threshold: no stumble


def test_excess_force_collisions_termination(C):
    rec = (np.float32(1.0), np.full(2, 1.0, np.float32), 3)
    r = feet_ref.evaluate(C, _wrench(b7=(0, 0, 130.0), b10=(0, 0, 90.0)), *rec, (0, 0))
    assert r["force"] == pytest.approx(0.5 * 30.0) and r["reward"] == r["force"]
    r = feet_ref.evaluate(C, _wrench(b4=(0, 2.0, 0), b5=(0, 0, 0.5)), *rec, (0, 0))
    assert r["collisions"] == 1 and r["collision"] == -7.0 and not r["terminated"]
    r = feet_ref.evaluate(C, _wrench(b4=(0, 2.0, 0), b5=(0, 0, 3.0), b1=(0, 0, 2.0)), *rec, (0, 0))
    assert r["collisions"] == 2 and r["collision"] == -14.0 and r["terminated"]


def test_record_and_layout(C):
    R = feet_ref.Record(C, 3, np.array([0.0, 0.5, 1.0], np.float32))
    assert np.array_equal(R.contact(), np.ones((3, 2), np.uint8)) and np.array_equal(R.t_last[:, 0], [0.0, 0.5, 1.0])
    w = np.stack([_wrench(), _wrench(b7=(0, 0, 9.0)), _wrench(b10=(0, 0, 9.0))])
    R.look(w, np.array([1, 1, 1], np.float32), np.zeros((3, 2)))
    assert np.array_equal(R.contact(), np.ones((3, 2), np.uint8))  # looking writes nothing
    R.step(w, np.array([1, 1, 2], np.float32), np.zeros((3, 2)))
    assert np.array_equal(R.contact(), [[0, 0], [1, 0], [0, 1]]) and np.array_equal(R.t_last, np.array([[0, 0], [1, 0.5], [1, 2]], np.float32))
    R.start(np.array([0, 0, 0], np.float32), which=[2])
    assert np.array_equal(R.contact()[2], [1, 1]) and np.array_equal(R.t_last[2], [0, 0])
    L, n = feet_ref.layout(46, 21, 9, True, True, 2, True)
    assert n == 81 and L["foot_contact"] == slice(76, 78) and L["command"] == slice(78, 81) and L["height_scan"] == slice(67, 76)
    L, n = feet_ref.layout(46, 21, 0, False, False, 4, False)
    assert n == 50 and L["foot_contact"] == slice(46, 50) and "command" not in L


def test_ctypes_struct_matches_the_header(hbmod, humanoid_model, tmp_path):
    import humanoid_mujoco_amd.engine as eng
    cls = eng.HbEnvFeet
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hb.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(hb_env_feet));',
             'printf("maxfeet %d\\n", HB_ENV_MAX_FEET);', 'printf("maxbodies %d\\n", HB_ENV_MAX_CONTACT_BODIES);']
    lines += ['printf("%s %%zu\\n", offsetof(hb_env_feet, %s));' % (f, f) for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 4 * (3 + 4 + 8 + 8 + 11)
    assert int(out["maxfeet"]) == 4 and int(out["maxbodies"]) == 8
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_defaults(hbmod, humanoid_model):
    import humanoid_mujoco_amd.engine as eng
    c = eng.HbEnvFeet()
    assert hbmod.lib().hb_env_default_feet(humanoid_model._h, ctypes.byref(c)) == 0 and _error(hbmod) == ""
    assert (c.n_feet, c.n_penalised, c.n_terminal, c.observe) == (0, 0, 0, 0)
    assert c.contact_threshold == 1.0 and c.air_time_target == 0.5 and (c.air_gate, c.air_cmd_min) == (1, np.float32(0.1)) and c.stumble_ratio == 5.0
    assert (c.w_air_time, c.w_force, c.w_stumble, c.w_collision) == (1.0, np.float32(-0.01), -1.0, -1.0)
    # twice the model's weight, computed here from the model's own arrays: the sum of the body masses times |gravity|
    g = humanoid_model.opt.gravity
    weight = float(np.sum(humanoid_model.array("body_mass"), dtype=np.float64)) * float(np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2))
    assert weight > 100.0 and c.force_max == pytest.approx(2.0 * weight, rel=1e-6)
    import feet_lib  # (what the GPU tests and profiles/feet_parity.txt call a quarter of the model's weight)
    assert feet_lib.feet_options(hbmod, humanoid_model)["force_max"] == pytest.approx(0.25 * weight, rel=1e-6)
    assert hbmod.lib().hb_env_default_feet(None, ctypes.byref(c)) == -1 and "NULL" in _error(hbmod)
    # the defaults name no feet: they do not pass the check until the caller does
    assert hbmod.lib().hb_env_feet_check(humanoid_model._h, ctypes.byref(c)) == -1 and "n_feet" in _error(hbmod)
    c.set_bodies(bodies=(FOOT_R, FOOT_L))
    assert hbmod.lib().hb_env_feet_check(humanoid_model._h, ctypes.byref(c)) == 0 and _error(hbmod) == ""


def test_refusals_without_a_device(hbmod, humanoid_model):
    L, m = hbmod.lib(), humanoid_model
    c = _cfg(hbmod, m)
    assert L.hb_env_feet_configure(None, ctypes.byref(c)) == -1 and "NULL batch" in _error(hbmod)
    assert L.hb_env_get_feet(None, None, None) == -1 and "NULL batch" in _error(hbmod)
    assert L.hb_env_feet_check(m._h, None) == -1 and "NULL" in _error(hbmod)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(n_feet=0), "n_feet"), (dict(n_feet=5), "n_feet"), (dict(n_penalised=-1), "n_penalised"), (dict(n_penalised=9), "n_penalised"),
             (dict(n_terminal=-1), "n_terminal"), (dict(n_terminal=9), "n_terminal"),
             (dict(bodies=(0, FOOT_L)), "foot body id"), (dict(bodies=(FOOT_R, m.nbody)), "foot body id"), (dict(bodies=(FOOT_R, -3)), "foot body id"),
             (dict(penalised=(m.nbody,)), "penalised body id"), (dict(terminal=(0,)), "terminal body id"),
             (dict(bodies=(FOOT_R, FOOT_L, FOOT_R)), "named twice"),
             (dict(contact_threshold=nan), "not finite"), (dict(w_air_time=inf), "not finite"), (dict(air_time_target=nan), "not finite"),
             (dict(air_cmd_min=nan), "not finite"), (dict(w_force=-inf), "not finite"), (dict(force_max=nan), "not finite"),
             (dict(w_stumble=nan), "not finite"), (dict(stumble_ratio=inf), "not finite"), (dict(w_collision=nan), "not finite"),
             (dict(contact_threshold=0.0), "contact_threshold"), (dict(contact_threshold=-1.0), "contact_threshold"),
             (dict(air_cmd_min=-0.1), "air_cmd_min"), (dict(stumble_ratio=-1.0), "stumble_ratio"),
             (dict(air_gate=2), "air_gate"), (dict(air_gate=-1), "air_gate"), (dict(observe=2), "observe")]
    for kw, word in cases:
        c = _cfg(hbmod, m, **kw)
        assert L.hb_env_feet_check(m._h, ctypes.byref(c)) == -1, kw
        assert word in _error(hbmod), (kw, _error(hbmod))
    # what is allowed: zero weights, a ratio and a speed bound of zero, the same body as a foot and as a penalised body, full lists
    c = _cfg(hbmod, m, w_air_time=0.0, w_force=0.0, w_stumble=0.0, w_collision=0.0, stumble_ratio=0.0, air_cmd_min=0.0, bodies=(7, 10, 6, 9),
             penalised=(7, 2, 3, 4, 5, 6, 8, 9), terminal=(1, 2, 3, 4, 5, 6, 7, 8))
    assert L.hb_env_feet_check(m._h, ctypes.byref(c)) == 0 and _error(hbmod) == ""

"""The observation extension's contract without a GPU (include/hb.h: hb_env_obs_extend, hb_env_nobs): the exports, the ctypes mirror
of hb_obs_ext, and tests/obs_ext_ref.py - the numpy composition of tests/ray_ref.py's cast into the extension row - on hand-made cases."""
import ctypes
import os
import subprocess

import numpy as np

import obs_ext_ref
import ray_cases
from oracle_lib import ROOT, Oracle


def test_library_exports_the_entry_points(hbmod):
    L = ctypes.CDLL(hbmod.LIB_PATH)
    assert hasattr(L, "hb_env_obs_extend") and hasattr(L, "hb_env_nobs")
    assert hbmod.lib().hb_env_nobs(None) == -1 and hbmod.lib().hb_env_obs_extend(None, None) == -1


def test_ctypes_struct_matches_the_header(hbmod, tmp_path):
    import humanoid_mujoco_amd.engine as eng
    cls = eng.HbObsExt
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hb.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(hb_obs_ext));']
    lines += ['printf("%s %%zu\\n", offsetof(hb_obs_ext, %s));' % (f, f) for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 24
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_env_row_export_and_mirror(hbmod, tmp_path):
    """hb_env_row is exported and refuses NULL; engine.HbEnvRow has the size and the field offsets of the header's struct hb_env_row"""
    import humanoid_mujoco_amd.engine as eng
    assert hasattr(ctypes.CDLL(hbmod.LIB_PATH), "hb_env_row") and hbmod.lib().hb_env_row(None, None) == -1
    cls = eng.HbEnvRow
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hb.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(struct hb_env_row));']
    lines += ['printf("%s %%zu\\n", offsetof(struct hb_env_row, %s));' % (f, f) for f, _ in cls._fields_]
    src = tmp_path / "row.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = tmp_path / "row"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 40
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def _terrain_case(points, cutoff):
    """world-frame downward rays from `points` at the terrain model's static geoms"""
    c = ray_cases.case("terrain")
    p = np.asarray(points, dtype=np.float32)
    c.update(pnt=p, vec=np.tile(np.float32([0, 0, -1]), (len(p), 1)), frame="world", frame_body=0, cutoff=cutoff)
    return c


def _rest_state(o):
    return np.concatenate([[0.0], np.asarray(o.info["qpos0"], dtype=np.float64), np.zeros(2 * o.nv)])


def test_flat_field_no_hit_and_clamp():
    o = Oracle(ray_cases.HFIELD_HBM)
    info = o.info
    assert int(info["geom_type"][0]) == 1 and int(info["geom_bodyid"][0]) == 0
    zf, half = float(info["geom_pos"][2]), float(info["hfield_size"][0])
    flat = np.zeros(int(info["nhfielddata"]))
    z0, cutoff = 1.0, 2.5
    pts = [[x, y, zf + z0] for x in (-3.3, 0.4, 2.9) for y in (-1.7, 0.6)] + [[half + 20.0, 0.0, zf + z0]]  # (the last one: off the field)
    c = _terrain_case(pts, cutoff)
    hs = dict(offset=0.25, scale=3.0)
    scan, res = obs_ext_ref.reference_scan(o, c, _rest_state(o), hs, hfield_data=flat)
    assert scan.dtype == np.float32 and scan.shape == (7,)
    assert (res["geomid"][:6] == 0).all() and res["geomid"][6] == -1
    # a flat field: scale * (offset - z0) everywhere; nothing hit: the cutoff takes the distance's place
    assert np.array_equal(scan[:6], np.full(6, np.float32(3.0) * (np.float32(0.25) - np.float32(z0)), dtype=np.float32))
    assert scan[6] == np.float32(3.0) * (np.float32(0.25) - np.float32(cutoff))
    # the clamp binds on both sides: the hits at -2.25 from below, the miss at -6.75 from below, and with the sign turned from above
    lo = obs_ext_ref.reference_scan(o, c, _rest_state(o), dict(hs, clip=(-1.0, 5.0)), hfield_data=flat)[0]
    assert np.array_equal(lo, np.full(7, -1.0, dtype=np.float32))
    hi = obs_ext_ref.reference_scan(o, c, _rest_state(o), dict(offset=0.25, scale=-3.0, clip=(-1.0, 2.0)), hfield_data=flat)[0]
    assert np.array_equal(hi, np.full(7, 2.0, dtype=np.float32))
    both = obs_ext_ref.scan_entries(np.float64([0.5, 1.0, 1.5]), np.int32([0, 0, 0]), cutoff, offset=1.0, scale=2.0, clip=(-0.5, 0.5))
    assert np.array_equal(both, np.float32([0.5, 0.0, -0.5]))
    # over the model's own elevations the same rays see the bumps: the terrain height relative to the rays' origin less offset
    own = obs_ext_ref.reference_scan(o, c, _rest_state(o), dict(offset=z0, scale=1.0))[0]
    assert own[:6].min() >= -1e-6 and own[:6].max() <= 0.0985 and own[:6].max() > 0.0


def test_extension_row_layout():
    latest = np.arange(6, dtype=np.float32).reshape(2, 3)
    dist, gid = np.float32([[0.5, -1.0], [2.0, 0.25]]), np.int32([[0, -1], [3, 0]])
    hs = dict(offset=1.0, scale=2.0, clip=(-1.5, 1.2))
    row = obs_ext_ref.extension(latest, dist, gid, 1.5, prev_action=True, height_scan=hs)
    assert row.dtype == np.float32 and np.array_equal(row, np.float32([[0, 1, 2, 1.0, -1.0], [3, 4, 5, -1.5, 1.2]]))
    assert np.array_equal(obs_ext_ref.extension(latest, dist, gid, 1.5, prev_action=False, height_scan=hs), row[:, 3:])
    assert np.array_equal(obs_ext_ref.extension(latest, dist, gid, 1.5, prev_action=True, height_scan=None), latest)

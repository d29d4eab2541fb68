"""The build/hb_tables tool for the tests that read the device model tables without a GPU (tests/test_device_tables_cpu.py,
tests/test_box_cpu.py): its runner, the readers of its output and of its --dump file, and the refusal texts that more than one file pins.

TEST INFRASTRUCTURE: the product package never imports this module.
"""
import os
import struct
import subprocess

import numpy as np

from oracle_lib import HB_TABLES, ROOT

STAGED = "only models that step in one kernel (plane / sphere / capsule geoms, condim 1 / 3) are implemented; this model steps in stages (mesh hulls, height fields or condim 4 / 6): "
GENERAL_28 = "models with mesh geoms, height fields or condim 4 / 6 support at most 28 degrees of freedom in this build"


def run(model, *options):
    """(exit code, stdout) of build/hb_tables on a model file; the tool is built first if it is not there"""
    if not os.path.exists(HB_TABLES):
        subprocess.check_call(["make", "-C", ROOT, "-s", "build/hb_tables"])
    p = subprocess.run([HB_TABLES, str(model)] + [str(o) for o in options], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.stderr == "", p.stderr
    return p.returncode, p.stdout


def fields(out):
    """the tool's lines: scalars and flags by name; "array" -> {name: length}; "table" -> {name: (array, offset, count, hash)}"""
    f = {"array": {}, "table": {}}
    for ln in out.strip().split("\n"):
        t = ln.split()
        if t[0] == "array":
            f["array"][t[1]] = int(t[2])
        elif t[0] == "table":
            f["table"][t[1]] = (t[2], int(t[3]), int(t[4]), t[5])
        elif t[0] == "qpos_src":
            f["qpos_src"] = int(t[1])
        else:
            f[t[0]] = float(t[1]) if "." in t[1] or "e" in t[1] else int(t[1])
    return f


def read_dump(path):
    """the int array and the fix-ups [(field offset, array, element offset)] of a --dump file (tools/hb_tables.cpp)"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"HBTABLE1"
    pos = 8

    def u64():
        nonlocal pos
        pos += 8
        return struct.unpack_from("<Q", raw, pos - 8)[0]

    n = u64(); pos += n  # the DevModel
    n = u64(); iv = np.frombuffer(raw, "<i4", n, pos); pos += 4 * n
    n = u64(); pos += 4 * n
    n = u64(); pos += 8 * n
    fix = [(u64(), u64(), u64()) for _ in range(u64())]
    return iv, fix

"""The learners' shared host arithmetic (csrc/hb_learn_host.hpp) and the refresh of the packed operands (hb_device.hpp: learn_refresh)
through the build/hb_learn_check tool, which runs them on the host over buffers of the device's sizes: no GPU.  The tool itself checks
the layout against the loops the learners had before they shared one, that the segments of every Adam / Polyak launch tile the record,
that every packed index stays inside its operand and that rows below k0 reach no place in a transpose (tools/hb_learn_check.cpp)."""
import os
import subprocess

from oracle_lib import HB_LEARN_CHECK as TOOL, ROOT


def test_layout_segments_refresh_and_carve():
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", ROOT, "-s", "build/hb_learn_check"])
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    assert p.stdout.splitlines() == ["ok ppo [48,20,33,21] [48,20,33,1]: P 4115", "ok ppo [48,42] [48,1]: P 2149",
                                     "ok sac [48,20,33,42] [69,20,33,1]: P 7356, targets 4254", "ok sac [48,42] [69,1]: P 2199, targets 140"]

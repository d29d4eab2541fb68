"""Generated models at the sizes where the step kernels' dispatch and their dense, padded code change (tests/test_gpu_kernel_matrix.py;
the chain specs themselves are step_lib.CHAINS).

chain_xml writes a capsule chain in MJCF: a free or a fixed base, two joints per link (hinges on alternating axes, one slide joint), a motor
on every joint, ranges on every third joint, a plane or a height-field floor.  Only the base and every third link collide, and only with
the floor, so that a state's contacts and limit rows stay inside the classic kernels' capacity (24 contacts, 63 rows).

perturbed_hbm writes a copy of a compiled .hbm with other masses, inertias, joint axes, ranges, damping, geom sizes and gears but the same
sizes: a model that still takes the size-specialised kernels (hb_tables.cpp: sized_h27 / sized_team).

kernel_table reads the step kernels' table (hb_step.hip: HB_KERNELS) for the CPU tests that hold its rows to what they must be.
"""
import os
import re

import numpy as np

from oracle_lib import CSRC, Oracle, load_state

# the columns of a row of HB_KERNELS behind the name: step_body's template arguments (the configuration the dispatch looks a kernel up
# by), then the launch attributes
CONFIG_COLUMNS = ("SOLVER", "NDENSE", "COLL", "NG", "DEFER", "LEAN", "SIZED", "INV", "INTEG", "ACC", "FRIC")
KERNEL_COLUMNS = CONFIG_COLUMNS + ("WAVES", "VGPRS", "RERUN")


def kernel_table():
    """hb_step.hip's kernel table in row order: [(name, {column: the cell's text})]"""
    lines = open(os.path.join(CSRC, "hb_step.hip")).read().split("\n")
    first = lines.index(next(ln for ln in lines if ln.startswith("#define HB_KERNELS(K)")))
    last = next(k for k in range(first, len(lines)) if not lines[k].rstrip().endswith("\\"))  # the macro's last line has no continuation
    rows = []
    for ln in lines[first + 1:last + 1]:
        m = re.match(r"\s*K\((\w+),([^)]*)\)", ln)
        if m:
            cells = [c.strip() for c in m.group(2).split(",")]
            assert len(cells) == len(KERNEL_COLUMNS), ln
            rows.append((m.group(1), dict(zip(KERNEL_COLUMNS, cells))))
        else:
            assert ln.strip().startswith("/*"), ln  # (only rows and comments)
    return rows

CNSTR_LIMIT_JOINT, CNSTR_CONTACT_FRICTIONLESS, CNSTR_CONTACT_PYRAMIDAL = 3, 5, 6  # (oracle/mjstep_oracle.c: mjmodel.h:256-265)
HFIELD_ELEV = np.array([[0.0, 0.3, 0.1, 0.6, 0.2],
                        [0.5, 0.9, 0.4, 0.0, 0.7],
                        [0.2, 0.0, 1.0, 0.5, 0.3],
                        [0.8, 0.4, 0.6, 0.1, 0.9],
                        [0.1, 0.7, 0.2, 0.8, 0.0]])
AXES = ("0 1 0", "0 0 1", "1 0 0")


def chain_xml(nv, free=True, floor="plane", condim=3, solver="PGS", timestep=0.004, forcerange=None):
    """A capsule chain of nv degrees of freedom (6 of them the free base's).  floor: "plane" or "hfield" (the height field of
    convex_models.hfield_xml with condim and friction of its own).  PGS runs its 50 sweeps with tolerance 0, as the terrain
    config does: whenever there are rows the sweep counts of device and oracle are the same number.  forcerange: None (no force limits, the XML of
    every caller that does not pass it) or r: every motor forcelimited to [-r, r]."""
    nj = nv - (6 if free else 0)
    assert nj >= 2
    nlink = (nj + 1) // 2
    z0 = 0.16 if floor == "plane" else 0.3
    parts = ['<body name="base" pos="0 0 %g">' % z0]
    if free:
        parts.append('<freejoint name="root"/><geom name="base" type="sphere" size="0.07" mass="1.5" contype="1"/>')
    else:  # (a fixed base: the chain is held at one end and falls onto the floor around it)
        parts.append('<geom name="base" type="sphere" size="0.05" mass="1" contype="0"/>')
    joints, j = [], 0
    for k in range(nlink):
        parts.append('<body name="l%d" pos="%g 0 0">' % (k, 0.0 if k == 0 else 0.1))
        for _ in range(2 if j + 1 < nj else 1):
            name = "j%d" % j
            lim = ' limited="true" range="-%d %d"' % (20 + 3 * (j % 5), 20 + 3 * (j % 5)) if j % 3 == 1 else ""
            if j == 2:  # the one slide joint: a telescoping link
                parts.append('<joint name="%s" type="slide" axis="1 0 0" limited="true" range="-0.02 0.02"/>' % name)
            else:
                parts.append('<joint name="%s" type="hinge" axis="%s"%s/>' % (name, AXES[j % 2 if j % 7 else 2], lim))
            joints.append(name)
            j += 1
        hit = k % 3 == 2
        parts.append('<geom name="g%d" type="capsule" fromto="0 0 0 0.1 0 0" size="0.025" mass="%g" contype="%d"/>' % (k, 0.2 + 0.01 * k, 1 if hit else 0))
    parts.append("</body>" * nlink)
    parts.append("</body>")
    body = "".join(parts)
    if floor == "plane":
        ground = '<geom name="floor" type="plane" size="0 0 1" condim="%d" friction="1 0.01 0.001" contype="1" conaffinity="1"/>' % condim
        asset = ""
    else:
        e = HFIELD_ELEV
        asset = '<asset><hfield name="h" nrow="%d" ncol="%d" size="3 3 0.08 0.5" elevation="%s"/></asset>' % (e.shape[0], e.shape[1], " ".join("%.17g" % v for v in e.reshape(-1)))
        ground = '<geom name="floor" type="hfield" hfield="h" condim="%d" friction="1 0.01 0.001" contype="1" conaffinity="1"/>' % condim
    frc = "" if forcerange is None else ' forcelimited="true" forcerange="-%g %g"' % (forcerange, forcerange)
    motors = "".join('<motor name="m_%s" joint="%s" gear="%g" ctrlrange="-1 1" ctrllimited="true"%s/>' % (n, n, 2.0 if i != 2 else 20.0, frc) for i, n in enumerate(joints))
    return ('<mujoco model="chain%d"><compiler angle="degree"/><option timestep="%g" iterations="%d" tolerance="%s" solver="%s"/>'
            '<default><joint damping="0.05" armature="0.01"/><geom conaffinity="0" condim="%d"/></default>%s'
            '<worldbody>%s%s</worldbody><actuator>%s</actuator></mujoco>'
            % (nv, timestep, 50 if solver == "PGS" else 100, 0 if solver == "PGS" else 1e-8, solver, condim, asset, ground, body, motors))


def oracle_for(hbmod, xml, tmp_path, name="m.hbm"):
    """the model compiled from the MJCF text, the .hbm file it was saved to in the directory tmp_path (a path or its text), and the
    fp64 oracle on that file"""
    m = hbmod.Model.from_xml_string(xml)
    p = os.path.join(str(tmp_path), name)
    m.save(p)
    return m, p, Oracle(p)


def rollout_states(o, steps=300, every=10, seed=0, keyframe=-1):
    """States every `every` steps along an oracle rollout under piecewise-constant random controls: [time, qpos, qvel, qacc_warmstart]
    records rounded to fp32 (what hb_set_state leaves on the device), and the controls of the step that follows each."""
    rng = np.random.default_rng(seed)
    o.reset(keyframe)
    states, ctrls = [], []
    c = np.zeros(o.nu)
    for t in range(steps):
        if t % 25 == 0:
            c = rng.uniform(-1, 1, o.nu)
        o.ctrl[:] = c
        if t % every == every - 1:
            states.append(np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart]))
            ctrls.append(c.copy())
        o.step()
    return np.array(states).astype(np.float32).astype(np.float64), np.array(ctrls, dtype=np.float32)


def oracle_steps(o, states, ctrls):
    """one oracle step from each state: a dict of per-state arrays (qpos, qvel after the step; qacc, efc_force, contacts, counts, row
    types of the step)"""
    out = dict(qpos=[], qvel=[], qacc=[], force=[], ncon=[], nefc=[], con=[], types=[])
    for s, c in zip(states, ctrls):
        load_state(o, s, c.astype(np.float64))
        o.forward()
        out["ncon"].append(o.ncon); out["nefc"].append(o.nefc)
        out["qacc"].append(o.qacc.copy()); out["force"].append(o.efc_force[:o.nefc].copy())
        out["con"].append(o.contacts()); out["types"].append(o.efc_types()[0])
        o.step()
        out["qpos"].append(o.qpos.copy()); out["qvel"].append(o.qvel.copy())
    return out


def row_kinds(ref):
    """(states with a contact row, states with a joint-limit row) of oracle_steps' output"""
    con = sum(bool(np.isin(t, (CNSTR_CONTACT_FRICTIONLESS, CNSTR_CONTACT_PYRAMIDAL)).any()) for t in ref["types"])
    lim = sum(bool((t == CNSTR_LIMIT_JOINT).any()) for t in ref["types"])
    return con, lim


def perturbed_hbm(src, dst, seed=0, scale=0.08):
    """A copy of the .hbm `src` with perturbed physical parameters and unchanged sizes: body masses and inertias (one factor per body,
    so the principal moments stay a valid inertia), hinge axes (renormalised), joint ranges and damping, geom sizes (shrunk only: the
    stored bounding radii stay conservative) and actuator gears."""
    rng = np.random.default_rng(seed)
    lines = open(src).read().splitlines()
    rec = {ln.split()[1]: i for i, ln in enumerate(lines) if ln[:2] in ("I ", "D ", "i ", "d ")}

    def vals(name):
        return np.array([float(x) for x in lines[rec[name]].split()[3:]])

    def put(name, v):
        tok = lines[rec[name]].split()[:3]
        lines[rec[name]] = " ".join(tok + ["%.17g" % x for x in v])

    jtype = vals("jnt_type").astype(int)
    body_f = 1 + scale * rng.uniform(-1, 1, len(vals("body_mass")))
    put("body_mass", vals("body_mass") * body_f)
    put("body_inertia", vals("body_inertia") * np.repeat(body_f, 3))
    ax = vals("jnt_axis").reshape(-1, 3)
    for j in range(len(ax)):
        if jtype[j] == 3:  # (hinge; the free joint's axis is not read)
            a = ax[j] + 0.15 * rng.uniform(-1, 1, 3)
            ax[j] = a / np.linalg.norm(a)
    put("jnt_axis", ax.reshape(-1))
    put("jnt_range", vals("jnt_range") * (1 + scale * rng.uniform(-1, 1, len(vals("jnt_range")))))
    put("dof_damping", vals("dof_damping") * (1 + scale * rng.uniform(-1, 1, len(vals("dof_damping")))))
    put("geom_size", vals("geom_size") * (1 - 0.5 * scale * rng.uniform(0, 1, len(vals("geom_size")))))
    put("actuator_gear", vals("actuator_gear") * (1 + scale * rng.uniform(-1, 1, len(vals("actuator_gear")))))
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    return dst

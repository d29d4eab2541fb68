"""The ray sets of tests/test_gpu_ray.py, tests/test_ray_cpu.py and tools/gpu_ray_report.py: models, states, specs and rays, and the
fp64 reference (ray_ref) of each, computed once per process.

TEST INFRASTRUCTURE: the product package never imports this module.

A case is a dict: xml or hbm (the model), states ([time, qpos, qvel, warm] records, one per env), pnt / vec [n_ray, 3], frame, frame_body,
bodyexclude, static, moving, cutoff, and planted: the indices of the rays placed ON grid lines, vertices and cell diagonals of a height
field - fragile on purpose.  Every other ray of every case is robust (tests/test_ray_cpu.py holds that from the reference alone).
"""
import functools
import os

import numpy as np

import ray_ref
from kernel_models import chain_xml, rollout_states
from oracle_lib import HFIELD_HBM, HUMANOID_HBM, TEAM_HBM, Oracle, load_state  # noqa: F401  (HFIELD_HBM: tests take it from here)

FRAMES = {"world": ray_ref.FRAME_WORLD, "body": ray_ref.FRAME_BODY, "yaw": ray_ref.FRAME_YAW}
BASE = 1  # the chain's base body
PHASE = {"world": 0.1, "body": 0.32, "yaw": 0.0}
PICK = (4, 14, 26)  # the states of rollout_states the three envs stand in: early in the fall, on the floor, tumbled


def sphere_dirs(n, phase=0.0, zmin=0.12):
    """n directions spread over the sphere (a Fibonacci spiral), none within zmin of the horizontal: a ray that grazes the infinite floor
    plane is fragile"""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    z = np.sign(z) * (zmin + (1 - zmin) * np.abs(z))
    phi = i * np.pi * (3 - np.sqrt(5)) + phase
    s = np.sqrt(1 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def primitive_rays(frame):
    """70 rays (one full wave and a remainder of 6) from around the base body: all over the sphere from points within 3 cm of the frame's
    origin - in the world frame, of a point 25 cm above where the chain lies.  The spiral's phase is chosen per frame so that no ray grazes
    a surface or passes within 1e-4 m of a second one at the three states (computed from ray_ref alone; tests/test_ray_cpu.py holds it)"""
    d = sphere_dirs(70, PHASE[frame])
    k = np.arange(70)
    p = 0.03 * np.stack([np.sin(1.3 * k), np.cos(2.1 * k), np.sin(0.7 * k + 1)], axis=1)
    if frame == "world":
        p = p + np.array([0.1, 0.0, 0.3])
    return p.astype(np.float32), d.astype(np.float32)


def _downward(points):
    p = np.asarray(points, dtype=np.float64)
    return p, np.tile([0.0, 0.0, -1.0], (len(p), 1))


def hfield_misc_rays():
    """World-frame rays at the 5 x 5 field of chain_xml(floor="hfield") (x, y in [-3, 3], grid lines every 1.5 m, elevations up to 8 cm) and
    the chain above it.  Returns (pnt, vec, planted)."""
    P, V = [], []
    rng = np.random.default_rng(12)
    for _ in range(66):  # oblique, from above, towards points of the field
        a, t = rng.uniform(-2.8, 2.8, 2), rng.uniform(-2.8, 2.8, 2)
        o = np.array([a[0], a[1], rng.uniform(0.4, 1.5)])
        P.append(o); V.append(np.array([t[0], t[1], 0.02]) - o)
    for k in range(16):  # from outside the field's extent, entering it across each side
        ang = 2 * np.pi * (k + 0.3) / 16
        o = np.array([4.5 * np.cos(ang), 4.5 * np.sin(ang), 0.9])
        P.append(o); V.append(np.array([0.7 * np.cos(ang + 2.5), 0.7 * np.sin(ang + 2.5), 0.03]) - o)
    for k in range(12):  # leaving the extent without a hit: flat or rising, over the field and out
        ang = 2 * np.pi * (k + 0.6) / 12
        P.append(np.array([0.4 * np.cos(ang), 0.4 * np.sin(ang), 0.5 + 0.05 * k])); V.append(np.array([np.cos(ang + 0.4), np.sin(ang + 0.4), 0.03 * k]))
    for k in range(6):  # parallel to the field's x axis (no y component: one component of the grid walk is zero), descending across cells
        P.append(np.array([-2.9 + 0.2 * k, -2.6 + 0.97 * k, 0.5])); V.append(np.array([1.0 if k % 2 == 0 else -0.2, 0.0, -0.12 - 0.03 * k]))
    for k in range(6):  # ... and to its y axis
        P.append(np.array([-2.3 + 0.93 * k, 2.8 - 0.1 * k, 0.45])); V.append(np.array([0.0, -1.0 if k % 2 == 0 else -0.3, -0.11 - 0.02 * k]))
    for k in range(8):  # from below the surface upward: the underside is hit (no base, no walls)
        P.append(np.array([-2.4 + 0.65 * k, 1.9 - 0.55 * k, -0.3])); V.append(np.array([0.15 * (k - 2), 0.1, 1.0]))
    planted = list(range(len(P), len(P) + 6))
    # ON a grid line, ON vertices, ON the cut of a cell (x - y constant: the (r, c) - (r + 1, c + 1) diagonal), straight down and oblique
    P += [np.array([-1.5, 0.4, 1.0]), np.array([0.6, 1.5, 1.0]), np.array([-1.5, 1.5, 1.0]), np.array([-2.25, -0.75, 1.0]),
          np.array([-1.5, -2.0, 1.0]), np.array([2.0, 0.0, 1.0])]
    V += [np.array([0, 0, -1.0])] * 4 + [np.array([0.0, 1.0, -1.0]), np.array([-1.0, 0.0, -0.8])]
    return np.array(P, dtype=np.float32), np.array(V, dtype=np.float32), planted


@functools.lru_cache(maxsize=None)
def _chain_states(floor):
    """(xml, the three states) of the 12-dof chain on `floor`"""
    import tempfile

    import humanoid_mujoco_amd as hb
    xml = chain_xml(12, floor=floor)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.hbm")
        hb.Model.from_xml_string(xml).save(p)
        hbm = open(p).read()
        o = Oracle(p)
        states, _ = rollout_states(o, steps=300, every=10, seed=0)
    return xml, hbm, states[list(PICK)]


def case(name):
    """the case's dict (module docstring)"""
    c = dict(frame="world", frame_body=0, bodyexclude=-1, static=True, moving=True, cutoff=0.0, planted=[])
    if name.startswith("prim_"):
        xml, hbm, states = _chain_states("plane")
        p, v = primitive_rays(name[5:])
        c.update(xml=xml, hbm_text=hbm, states=states, pnt=p, vec=v, frame=name[5:], frame_body=BASE, bodyexclude=BASE)
    elif name.startswith("hf_"):
        xml, hbm, states = _chain_states("hfield")
        c.update(xml=xml, hbm_text=hbm, states=states)
        if name == "hf_scan":  # the height scan: a yaw-frame grid of downward rays under the base, terrain only
            import humanoid_mujoco_amd as hb
            p, v = hb.height_scan_rays(np.linspace(-0.8, 0.8, 9) + 0.013, np.linspace(-0.6, 0.6, 7) - 0.007, 1.0)
            c.update(pnt=p, vec=v, frame="yaw", frame_body=BASE, moving=False)
        elif name == "hf_misc":
            p, v, planted = hfield_misc_rays()
            c.update(pnt=p, vec=v, planted=planted)
        elif name == "hf_cutoff":  # straight down from 1 m onto elevations of 0 .. 8 cm: a cutoff of 0.96 m turns the low half into misses
            g = np.stack(np.meshgrid(np.linspace(-2.6, 2.6, 8) + 0.031, np.linspace(-2.7, 2.5, 7) - 0.017), axis=-1).reshape(-1, 2)
            p, v = _downward(np.concatenate([g, np.ones((len(g), 1))], axis=1))
            c.update(pnt=p.astype(np.float32), vec=v.astype(np.float32), moving=False, cutoff=0.96)
        else:
            raise KeyError(name)
    elif name in ("terrain", "team"):  # yaw-frame scans of the assets' 8 x 8 fields under the torso (states: the tests' own)
        import humanoid_mujoco_amd as hb
        p, v = hb.height_scan_rays(np.linspace(-1.0, 1.0, 11) + 0.017, np.linspace(-0.6, 0.6, 7) + 0.011, 1.0)
        c.update(hbm=HFIELD_HBM if name == "terrain" else TEAM_HBM, pnt=p, vec=v, frame="yaw", frame_body=1, moving=False, cutoff=3.0)
    else:
        raise KeyError(name)
    return c


CHAIN_CASES = ("prim_world", "prim_body", "prim_yaw", "hf_scan", "hf_misc", "hf_cutoff")


def flags_of(c):
    return (ray_ref.STATIC if c["static"] else 0) | (ray_ref.MOVING if c["moving"] else 0)


def reference_at(o, c, state, hfield_data=None):
    """ray_ref.reference of the case's rays with the oracle at one [time, qpos, qvel, warm] record"""
    load_state(o, state, np.zeros(o.nu))
    o.forward()
    return ray_ref.reference(o, c["pnt"], c["vec"], FRAMES[c["frame"]], c["frame_body"], flags_of(c), c["bodyexclude"], c["cutoff"], hfield_data)


@functools.lru_cache(maxsize=None)
def chain_reference(name):
    """[ray_ref result per env] of one of CHAIN_CASES at its three states"""
    import tempfile
    c = case(name)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.hbm")
        with open(p, "w") as f:
            f.write(c["hbm_text"])
        o = Oracle(p)
        return [reference_at(o, c, s) for s in c["states"]]


def team_states(n=4):
    """[time, qpos, qvel, warm] records along an oracle rollout of the reference's robot from its standup reset, rounded to fp32"""
    o = Oracle(TEAM_HBM)
    o.reset(0)
    out = []
    for t in range(n * 15):
        o.ctrl[:] = 0.2 * np.sin(0.05 * t + np.arange(o.nu))
        o.step()
        if t % 15 == 14:
            out.append(np.concatenate([[o.time], o.qpos, o.qvel, o.qacc_warmstart]))
    return np.array(out).astype(np.float32).astype(np.float64)


def compare(res, dist, geomid):
    """One env's device rows against its reference: (worst deviation of dist over the robust rays relative to max(1, dist_ref), number of
    robust rays, number of fragile rays).  Asserts what holds without a bound: a robust ray has the reference's geom (and is a miss where
    the reference misses), a fragile ray has one of the reference's two candidates (geom; distance within 1e-3 of either, or the miss a
    cutoff or a clearance below FRAGILE_DIST allows)."""
    fr = ray_ref.fragile(res)
    worst = 0.0
    for i in range(len(dist)):
        g, t = int(geomid[i]), float(dist[i])
        if not fr[i]:
            assert g == int(res["geomid"][i]), (i, g, t, {k: v[i] for k, v in res.items()})
            if g >= 0:
                worst = max(worst, abs(t - res["dist"][i]) / max(1.0, res["dist"][i]))
            else:
                assert t == -1.0, (i, t)
        else:
            first = g == int(res["geomid"][i]) and (g < 0 or abs(t - res["dist"][i]) < 1e-3)
            second = g == int(res["second_geom"][i]) and (g < 0 or abs(t - res["second"][i]) < 1e-3)
            assert first or second or g < 0 and res["geomid"][i] < 0, (i, g, t, {k: v[i] for k, v in res.items()})
    return worst, int((~fr).sum()), int(fr.sum())

"""The rows of tests/test_gpu_domain_params.py and what it shares with tests/test_dr_ref_cpu.py: which model reaches which step kernels,
the families each row is held on, the models, oracles and teacher-forced states (computed once per session), the reference step of each
row's kind and the deviations in the normalisation of their bounds.  Needs no GPU.  Test infrastructure only."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

import dr_ref
import eq_ref
import fric_ref
import rk4_ref
from bounds import BOUNDS  # noqa: F401  (the golden bounds: tests/test_gpu_domain_params.py takes them from here)
from eq_models import add_equality
from fric_models import add_friction
from kernel_models import chain_xml, rollout_states
from oracle_lib import HUMANOID_HBM, TEAM_HBM, Oracle, load_state
from step_lib import CHAINS

_TMP = None
N, ROUNDS, T = 8, 4, 5
FORCERANGE = 0.6   # of the chains' motors (gain 1, ctrl in [-1, 1]): the clamp bites whenever |ctrl| > 0.6 -+ the drawn change
ALL5 = dr_ref.FAMILIES
NO_FRICTION = tuple(f for f in ALL5 if f != "friction")
H27_KP = (1.0, 0.3)  # humanoid27 has no force-limited actuator: its family "actuator" is the gain, drawn around the model's own 1

# row -> dict(model, kind (the reference), runs [(knobs, "diag" | "state", kernel)], families, kp, bump; focus: a row that is there for one
# family only - its kernel runs the others on row a)
ROWS = {
    "a_humanoid27_pgs": dict(model=("asset", HUMANOID_HBM, None, -1), kind="plain", kp=H27_KP, runs=[({}, "diag", "hb_step_kernel")], families=ALL5),
    "b_humanoid27_newton": dict(model=("asset", HUMANOID_HBM, 2, -1), kind="plain", kp=H27_KP, runs=[({}, "diag", "hb_step_newton28_kernel")], families=ALL5),
    "c_chain32_cd3_pgs": dict(model=("chain", "chain32_cd3_pgs"), kind="plain", runs=[({}, "diag", "hb_step32_kernel")], families=ALL5),
    "c_chain32_cd1_newton": dict(model=("chain", "chain32_cd1_newton"), kind="plain", runs=[({}, "diag", "hb_step_newton32_kernel")], families=NO_FRICTION),
    "d_chain21_hfield_pgs": dict(model=("chain", "chain21_hfield_pgs"), kind="plain", bump=1.0, families=NO_FRICTION, own_states=("all",),
                                 runs=[({}, "diag", "hb_step_gen_fast_kernel"), ({"staged": 0}, "diag", "hb_step_gen_kernel")]),
    "e_chain21_cd6_pgs": dict(model=("chain", "chain21_cd6_pgs"), kind="plain", families=ALL5,
                              runs=[({}, "diag", "hb_step_gen_big_kernel"), ({"lean": 0}, "state", "hb_step_gen_fast1_kernel")]),
    "e_chain20_cd6_newton": dict(model=("chain", "chain20_cd6_newton"), kind="plain", families=ALL5,
                                 runs=[({}, "diag", "hb_step_newton_big20_kernel"), ({"lean": 0}, "state", "hb_step_newton_gen20_kernel")]),
    "f_team_robot": dict(model=("asset", TEAM_HBM, None, 0), kind="plain", kp=(2.0, 0.5), families=NO_FRICTION,
                         runs=[({}, "diag", "hb_step_newton_big20_kernel"), ({"lean": 0}, "state", "hb_step_newton_gen20_kernel")]),
    "f_chain21_position_pgs": dict(model=("chain", "chain21_cd3_pgs", "position"), kind="plain", kp=(2.0, 0.5), families=("actuator",), focus=True,
                                   runs=[({}, "diag", "hb_step_kernel")]),
    "g_fric28_cd1_newton": dict(model=("fric", 28, 1, "Newton"), kind="fric", runs=[({}, "diag", "hb_fric_newton28_kernel")], families=NO_FRICTION),
    "g_eq28_cd3_pgs": dict(model=("eq", 28, 3, "PGS"), kind="eq", runs=[({}, "diag", "hb_eq_kernel")], families=ALL5),
    "h_humanoid27_rk4": dict(model=("asset", HUMANOID_HBM, None, -1, "rk4"), kind="rk4", kp=H27_KP, runs=[({}, "diag", "hb_rk4_kernel")], families=ALL5),
}
CASES = [(row, cfg) for row, r in ROWS.items() for cfg in r["families"] + ("all",)]


@functools.lru_cache(maxsize=None)
def _setup_cached(row, tmp):
    import humanoid_mujoco_amd as hb
    spec = ROWS[row]
    mk = spec["model"]
    rk4 = mk[-1] == "rk4"
    if mk[0] == "asset":
        path, solver, key = mk[1:4]
        m, o = hb.Model.load(path), Oracle(path)
        if solver is not None:
            m.set_opt(solver=solver, iterations=100)
            o.set_opt(solver=solver, iterations=100)
        if rk4:
            m.set_opt(integrator=hb.INT_RK4)
        st, ct = rollout_states(o, keyframe=key)
        fences_ok = path.endswith(("hfield.hbm", "team_robot.hbm"))
    else:
        if mk[0] == "chain":
            cs = CHAINS[mk[1]]
            xml = chain_xml(*cs, forcerange=FORCERANGE)
            if mk[-1] == "position":  # position servos: biasprm[1] = -kp, the affine bias that follows a drawn gain
                assert xml.count("<motor name=") == cs[0] - 6
                xml = xml.replace("<motor name=", '<position kp="2" name=')
            fences_ok = cs[2] == "hfield"
        else:
            xml = add_friction(chain_xml(mk[1], condim=mk[2], solver=mk[3], forcerange=FORCERANGE))
            if mk[0] == "eq":
                xml = add_equality(xml)
            fences_ok = False
        m = hb.Model.from_xml_string(xml)
        path = os.path.join(tmp, row + ".hbm")
        m.save(path)
        o = Oracle(path)
        st, ct = {"chain": rollout_states, "fric": fric_ref.rollout_states, "eq": eq_ref.rollout_states}[mk[0]](o)
    return dict(row=row, m=m, path=path, o=o, st=st, ct=ct, fences_ok=fences_ok, kind=spec["kind"], base=dr_ref.snapshot(o), A=dr_ref.model_arrays(m),
                kp=spec.get("kp"), bump=spec.get("bump", 0.0))


def setup_row(row):
    """the row's model, oracle, nominal teacher-forced states and controls: computed once per session and shared.  The oracle's model
    arrays are changed by dr_ref.apply during a case and put back (dr_ref.restore) at its end."""
    global _TMP
    if _TMP is None:
        _TMP = tempfile.mkdtemp(prefix="dr_rows_")
        atexit.register(shutil.rmtree, _TMP, ignore_errors=True)
    return _setup_cached(row, _TMP)


def config(S, name):
    return dr_ref.family(name, kp=S["kp"], bump=S["bump"])


def blocks(S, D, n=N):
    """the blocks the device draws for envs 0 .. n - 1 at episode 0 (dr_ref.draw)"""
    return np.array([dr_ref.draw(S["A"], D, e, 0) for e in range(n)])


@functools.lru_cache(maxsize=None)
def _own_states(row):
    """row d, config "all": every env's own rollout ON ITS OWN BLOCK (its drawn height map included), so that its teacher-forced states
    touch its own terrain - the states of the nominal rollout float above or sink into another map.  [(states, ctrls)] per env."""
    S = setup_row(row)
    o, base = S["o"], S["base"]
    L = dr_ref.layout(S["m"], dr_ref.stride_of(S["m"]))
    P = blocks(S, config(S, "all"))
    out = []
    try:
        for e in range(N):
            dr_ref.apply(o, P[e], L, base)
            out.append(rollout_states(o, seed=e))
    finally:
        dr_ref.restore(o, base)
    return out


def round_states(S, r, cfg=None):
    """states and controls of round r, one per env: state (8 r + e) mod 30 of the nominal rollout, or - ROWS[row]["own_states"] names
    the configs - of env e's own rollout on its own block"""
    idx = [(N * r + e) % len(S["st"]) for e in range(N)]
    if cfg in ROWS[S["row"]].get("own_states", ()):
        own = _own_states(S["row"])
        return np.array([own[e][0][i] for e, i in enumerate(idx)]), np.array([own[e][1][i] for e, i in enumerate(idx)])
    return S["st"][idx], S["ct"][idx]


def ref_step(S, s, c):
    """one reference step of the row's kind from the record s under c, with whatever model arrays the oracle carries now: dict of ncon,
    nefc, niter (None: not compared), con, qacc, force (of the step), qpos, qvel (after it)"""
    o, kind = S["o"], S["kind"]
    c = np.asarray(c, dtype=np.float64)
    if kind == "plain":
        load_state(o, s, c)
        o.forward()
        r = dict(ncon=o.ncon, nefc=o.nefc, niter=o.dint("solver_niter") if o.opt("solver") != 2 else None, con=o.contacts(), qacc=o.qacc.copy(),
                 force=o.efc_force[:o.nefc].copy())
        o.step()
        r.update(qpos=o.qpos.copy(), qvel=o.qvel.copy())
        return r
    if kind == "rk4":
        x = rk4_ref.rk4_step(o, s, c)
        return dict(ncon=x["counts"][3][0], nefc=x["counts"][3][1], niter=None, con=x["contacts"], qacc=x["qacc"], force=x["efc_force"], qpos=x["qpos"], qvel=x["qvel"])
    ref = (fric_ref if kind == "fric" else eq_ref).steps_ref(o, [s], [c])
    return dict(ncon=ref["ncon"][0], nefc=ref["nefc"][0], niter=ref["niter"][0] if o.opt("solver") != 2 else None, con=ref["con"][0], qacc=ref["qacc"][0],
                force=ref["force"][0], qpos=ref["qpos"][0], qvel=ref["qvel"][0])


COMPARED = {"diag": ("qpos", "qvel", "qacc", "force"), "state": ("qpos", "qvel")}  # what a run of each mode holds to its bound, besides the counts


def deviation(x, r):
    """the compared quantities of x against the reference step r, each in the normalisation of its bound (bounds.BOUNDS)"""
    d = dict(qpos=(np.abs(x["qpos"] - r["qpos"]) / np.maximum(1.0, np.abs(r["qpos"]))).max(), qvel=np.abs(x["qvel"] - r["qvel"]).max() / max(1.0, np.abs(r["qvel"]).max()),
             qacc=np.abs(x["qacc"] - r["qacc"]).max() / max(1.0, np.abs(r["qacc"]).max()))
    if r["nefc"]:
        d["force"] = np.abs(x["force"][:r["nefc"]] - r["force"]).max() / max(1.0, np.abs(r["force"]).max())
    return d

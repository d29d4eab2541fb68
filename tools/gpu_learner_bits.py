#!/usr/bin/env python3
"""The bits the device learners leave behind, as SHA-256 digests: run on two builds of the library (a checkout each, this file copied
into the other one's tools/), every line has to be equal for the two to compute the same thing.  Both learners have a fixed reduction
order and fixed roundings, so equal within a tolerance is not the bar.
  ppo: hb_ppo_grad_dev + hb_ppo_adam_dev on the seeded problems of tests/ppo_ref.py
  sac: hb_sac_step_dev with given draws on the seeded problems of tests/sac_ref.py
for the tests' networks small, one_layer, mixed and wide (SAC's wide: the wide actor and Q network of its tests), each with
  mb100:  three optimiser steps on 100 rows of 200 (two chunks, the last with a partial 16-row tile): rows 0 .. 99, an index, rows 100 .. 199
  mb4112: one step on 4112 rows (chunks of 80 rows, 52 of them)
Printed per case: a digest each of the parameters, the gradients, m, v, (SAC) the targets, and the 16 statistics of every step.
Every case runs in a child process of its own under its own time limit, and the first one that fails ends the run.
usage: gpu_learner_bits.py [--out FILE]     (results: profiles/learn_core_bits.txt)"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NU = 21
WIDE_A, WIDE_V, WIDE_Q = [48, 256, 256, 256], [48, 256, 256, 256, 1], [69, 256, 256, 256, 1]
PPO_NETS = {"small": ([48, 20, 33, 21], [48, 20, 33, 1]), "one_layer": ([48, 21], [48, 1]), "mixed": ([48, 64, 21], [48, 16, 1]), "wide": (WIDE_A + [21], WIDE_V)}
SAC_NETS = {"small": ([48, 20, 33, 42], [69, 20, 33, 1]), "one_layer": ([48, 42], [69, 1]), "mixed": ([48, 64, 42], [69, 16, 1]), "wide": (WIDE_A + [42], WIDE_Q)}
CASES = [(learner, net, mb) for learner in ("ppo", "sac") for net in ("small", "one_layer", "mixed", "wide") for mb in (100, 4112)]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--child", nargs=3, default=None, metavar=("LEARNER", "NET", "MB"))
args = ap.parse_args()

if args.child is None:
    lines = []
    for learner, net, mb in CASES:
        limit = 180
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", learner, net, str(mb)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit("gpu_learner_bits: %s %s mb%d ran into its time limit of %d s - nothing more is started" % (learner, net, mb, limit))
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit("gpu_learner_bits: %s %s mb%d failed with status %d - nothing more is started" % (learner, net, mb, r.returncode))
        lines += r.stdout.splitlines()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402

import humanoid_mujoco_amd as hb  # noqa: E402

learner, net, MB = args.child[0], args.child[1], int(args.child[2])
model = hb.Model.load(os.path.join(ROOT, "humanoid_mujoco_amd", "assets", "humanoid27.hbm"))
b = hb.Batch(model, 16, 0)
N_ROWS = 200 if MB == 100 else MB
rng = np.random.default_rng(5)
SELS = [(np.arange(0, 100), 0), (rng.permutation(200)[:100], None), (np.arange(100, 200), 100)] if MB == 100 else [(np.arange(MB), 0)]


def to_dev(a):
    p = b.dev_alloc(max(a.nbytes, 4))
    b.to_dev(p, np.ascontiguousarray(a))
    return p


def layers(t, tag, sizes):
    n = len(sizes) - 1
    return [t["%s.w%d" % (tag, l)] for l in range(n)], [t["%s.b%d" % (tag, l)] for l in range(n)]


stats_dev = to_dev(np.full(16, np.nan, np.float32))
stats = []
if learner == "ppo":
    import ppo_ref as pr
    asz, csz = PPO_NETS[net]
    flat, rows = pr.random_problem(asz, csz, N_ROWS, seed=1)
    t = pr.split(flat.astype(np.float32), asz, csz, NU)
    b.actor_set(asz, *layers(t, "actor", asz), head="gaussian", log_std=t["log_std"], seed=3)
    b.critic_set(csz, *layers(t, "critic", csz))
    b.learner_create(lr=1e-3, ent_coef=0.01)
    tapes = [to_dev(rows[k].astype(np.float32)) for k in ("obs", "action", "old_log_prob", "advantage", "returns")]
    for sel, first in SELS:
        index = None if first is not None else to_dev(sel.astype(np.int32))
        b.ppo_grad_dev(*tapes, N_ROWS, MB, index=index, first=first or 0, stats=stats_dev)
        b.ppo_adam_dev(stats=stats_dev)
        stats.append(b.from_dev(stats_dev, (16,)))
    st, grads = b.learner_state(), b.learner_grads()
else:
    import sac_ref as sr
    asz, qsz = SAC_NETS[net]
    pb = sr.random_problem(asz, qsz, N_ROWS, seed=1)
    t = sr.split(pb["flat"].astype(np.float32), asz, qsz)
    b.actor_set(asz, *layers(t, "actor", asz), head="squashed", seed=3)
    b.q_set(0, qsz, *layers(t, "q1", qsz))
    b.q_set(1, qsz, *layers(t, "q2", qsz))
    b.sac_create(lr_actor=1e-3, lr_critic=1e-3, lr_ent=1e-3, ent_coef_init=0.3, tau=0.05)
    st = b.sac_state()
    st["params"], st["targets"] = pb["flat"].astype(np.float32), pb["targets"].astype(np.float32)
    b.sac_set_state(st)
    tapes = [to_dev(pb["rows"][k].astype(np.uint8 if k == "done" else np.float32)) for k in ("obs", "action", "reward", "next_obs", "done")]
    for sel, first in SELS:
        index = None if first is not None else to_dev(sel.astype(np.int32))
        eps = [to_dev(pb[k][sel].astype(np.float32)) for k in ("eps_pi", "eps_next")]
        b.sac_step_dev(*tapes, N_ROWS, MB, index=index, first=first or 0, eps_pi=eps[0], eps_next=eps[1], eps_given=True, stats=stats_dev)
        stats.append(b.from_dev(stats_dev, (16,)))
    st, grads = b.sac_state(), b.sac_grads()

assert int(st["t"]) == len(SELS), st["t"]
what = [("params", st["params"]), ("grads", grads), ("m", st["m"]), ("v", st["v"])] + ([("targets", st["targets"])] if learner == "sac" else []) + [("stats", np.concatenate(stats))]
for name, a in what:
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.size and np.isfinite(a).all(), name
    print("%s %-9s mb%-4d %-7s %6d floats  sha256 %s" % (learner, net, MB, name, a.size, hashlib.sha256(a.tobytes()).hexdigest()))
b.close()

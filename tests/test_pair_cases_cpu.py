"""(CPU) The pair case table (tests/pair_cases.py) proven against the oracle alone, before any device sees it:

  - the labelled restatement tests/pair_ref.py equals Oracle.contacts() to 1e-12 on every case (count, geoms, dist, pos, normal),
    from the fp32-rounded state loaded with load_state;
  - every case takes the branches it was built for, and every branch label is taken by at least two cases (histogram printed);
  - no case sits on an activation boundary: every activation test the reference makes is more than GUARD = 1e-4 m off its threshold;
  - exactly one pair is in range per case, and it is the pair under test; the parked bodies are at least 5 m from everything;
  - the CONDITIONING ENVELOPE of every case, from the reference alone: the oracle at NPERT = 32 states whose qpos is perturbed by one
    fp32 rounding, 2^-24 max(1, |qpos|) N(0, 1), and the spread of dist, pos and normal over them.  A case whose perturbed evaluations
    disagree on the contact COUNT is ill-conditioned; at most 5 % of the table may be.  The exact cases (bitwise equal operands) get
    neither an envelope nor a count allowance: reference() gives them a zero envelope and only the unperturbed evaluation.

pair_cases.reference() computes all of this once; it is what tests/test_gpu_narrow_pairs.py holds the device to.
"""
import collections

import numpy as np
import pytest

import pair_cases
import pair_ref
from oracle_lib import Oracle
from pair_cases import GUARD, compiled, envelope, evaluate, reference


@pytest.fixture(scope="module")
def ref(hbmod, tmp_path_factory):
    return reference(hbmod, "pgs", tmp_path_factory.mktemp("pairs"))


def _labelled(ref):
    return [pair_ref.collide(ref["info"], c["qpos"]) for c in ref["cases"]]


def test_pair_ref_equals_the_oracle(ref):
    assert len(ref["cases"]) >= 150
    for c, ev, (con, _, _) in zip(ref["cases"], ref["evals"], _labelled(ref)):
        want = ev[0]["con"]
        assert len(con) == len(want), (c["name"], len(con), len(want))
        for a, b in zip(con, want):
            assert (a["geom1"], a["geom2"]) == (b["geom1"], b["geom2"]), c["name"]
            assert {a["geom1"], a["geom2"]} == set(c["geoms"]), c["name"]
            assert np.abs(b["frame"] @ b["frame"].T - np.eye(3)).max() <= 1e-9, (c["name"], "the oracle's own frame is degenerate")
            assert abs(a["dist"] - b["dist"]) <= 1e-12 and np.abs(a["pos"] - b["pos"]).max() <= 1e-12 and np.abs(a["normal"] - b["frame"][0]).max() <= 1e-12, c["name"]


def test_every_branch_is_taken_at_least_twice(ref):
    hist = collections.Counter()
    for c, (_, labels, _) in zip(ref["cases"], _labelled(ref)):
        assert set(c["expect"]) <= set(labels), (c["name"], c["expect"], labels)
        hist.update(set(labels))
    print("\nbranch histogram over %d cases:" % len(ref["cases"]))
    for k in sorted(hist):
        print("  %-28s %d" % (k, hist[k]))
    need = ["plane-sphere", "sphere-sphere", "normal:dif", "normal:fallback", "cc:general", "cc:parallel", "clamp:double", "parallel:0", "parallel:2",
            "sphere-capsule:g1<g2", "sphere-capsule:g1>g2"]
    need += ["plane-capsule:" + s for s in ("00", "01", "10", "11")] + ["sphere-capsule:" + s for s in ("interior", "x>len", "x<-len")]
    need += ["clamp1:" + s for s in ("none", "x1>len1", "x1<-len1")] + ["clamp2:" + s for s in ("none", "x2>len2", "x2<-len2")] + ["hit:h%d" % k for k in range(4)]
    assert all(hist[k] >= 2 for k in need), {k: hist[k] for k in need if hist[k] < 2}
    assert min(hist.values()) >= 2, hist
    # the parallel branch's "first two hits in order" rule: every pair of candidates that two parallel capsules can hit together
    pairs = collections.Counter(tuple(sorted(x for x in set(labels) if x.startswith("hit:"))) for _, labels, _ in _labelled(ref) if "cc:parallel" in labels)
    for want in (("hit:h0", "hit:h1"), ("hit:h0", "hit:h2"), ("hit:h0", "hit:h3"), ("hit:h1", "hit:h2"), ("hit:h2", "hit:h3")):
        assert pairs[want] >= 2, (want, pairs)


def test_guard_band_and_one_pair_in_range(ref):
    info = ref["info"]
    worst = np.inf
    floor = list(info["geom_name"]).index("floor")
    for c, (_, _, tests) in zip(ref["cases"], _labelled(ref)):
        near = set()
        for kind, cdist, thresh, g1, g2 in tests:
            if {g1, g2} == set(c["geoms"]):
                assert abs(cdist - thresh) > GUARD, (c["name"], kind, cdist, thresh)
                worst = min(worst, abs(cdist - thresh))
                near.add((g1, g2))
                assert cdist < thresh + 0.5, (c["name"], "the pair under test is not in range")
            else:  # (a parked body: 4 m beyond any range; the pair under test against the plane: clear of its range by 0.3 m)
                clear = 0.3 if {g1, g2} <= set(c["geoms"]) | {floor} else 4.0
                assert kind == "bound" and cdist > thresh + clear, (c["name"], g1, g2, cdist, thresh)
        assert len(near) == 1, (c["name"], near)
        gpos, _ = pair_ref.geom_poses(info, c["qpos"])
        nrm = pair_ref.quat2mat(info["geom_quat"][4 * floor:4 * floor + 4])[:, 2]
        parked = [g for g in range(len(gpos)) if g != floor and g not in c["geoms"]]
        for g in parked:
            assert (gpos[g] - gpos[floor]) @ nrm >= 5.0, c["name"]
            assert all(np.linalg.norm(gpos[g] - gpos[h]) >= 5.0 for h in range(len(gpos)) if h not in (g, floor)), c["name"]
    print("\nguard band: the closest activation test of the table is %.3e m off its threshold (required > %.0e)" % (worst, GUARD))


def test_conditioning_envelopes(ref):
    cases, ill = ref["cases"], ref["ill"]
    exact = np.array([c["exact"] for c in cases])
    assert exact.sum() >= 25 and not ill[exact].any()
    for i in np.flatnonzero(exact):
        assert len(ref["evals"][i]) == 1 and envelope(ref, i, ref["evals"][i][0]["ncon"])[1].sum() == 0.0
    share = ill.mean()
    print("\nill-conditioned cases (the perturbed oracle evaluations disagree on the contact count): %d of %d = %.1f %%" % (ill.sum(), len(cases), 100 * share))
    for i in np.flatnonzero(ill):
        print("  %-60s counts %s" % (cases[i]["name"], sorted({e["ncon"] for e in ref["evals"][i]})))
    assert share <= 0.05
    by_type = collections.defaultdict(lambda: np.zeros(3))
    for i, c in enumerate(cases):
        e = envelope(ref, i, ref["evals"][i][0]["ncon"])[1]
        if len(e):
            k = "-".join(n[0] if n == "floor" else n for n in c["pair"])
            by_type[k] = np.maximum(by_type[k], e.max(axis=0))
    for k, e in sorted(by_type.items()):
        print("  largest envelope %-4s dist %.2e pos %.2e normal %.2e" % (k, e[0], e[1], e[2]))


def test_scene_variants_share_the_table(hbmod, tmp_path):
    """the four variants compile to 24 dofs and the same poses: same contacts from the same cases (geom ids aside)"""
    base = None
    for v in pair_cases.VARIANTS:
        m, p, info = compiled(hbmod, v, tmp_path)
        assert (m.nq, m.nv, m.nu) == (28, 24, 0), v
        o = Oracle(p)
        got = []
        for c in pair_cases.build_cases(info)[::7]:
            ev = evaluate(o, c["qpos"])
            got.append((ev["ncon"], [x["dist"] for x in ev["con"]]))
        base = base or got
        assert got == base, v

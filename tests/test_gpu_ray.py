"""The ray read-out (include/hb.h: hb_ray_configure, hb_rays*; csrc/hb_ray.hip) on the GPU against the fp64 reference tests/ray_ref.py.

The ray sets are tests/ray_cases.py's; tests/test_ray_cpu.py holds, from the reference alone, that apart from the rays planted on grid
lines, vertices and cuts none of them is fragile.  For every robust ray the device must name the reference's geom and give its distance
within BOUND; for a planted ray one of the reference's two candidates.

BOUND (bounds.RAY_BOUND) is the project's contact-geometry bound, bounds.BOUNDS["pos"] = 1e-5 relative to max(1, dist_ref).  Measured on MI355X
by tools/gpu_ray_report.py (profiles/ray_parity.txt; these sets at 30 states of the chain's rollout, 8 of the robot's, 8 envs' own terrain):
worst 2.141e-06 (a floor-plane hit 5 m away from a tumbled base frame), medians below 7e-08 - under the target, so the target is the bound
(it would have become four times the measured worst case otherwise).
"""
import ctypes

import numpy as np
import pytest

import ray_cases
import ray_ref
from bounds import RAY_BOUND as BOUND
from oracle_lib import Oracle
from step_lib import snapshot

pytestmark = pytest.mark.gpu

KERNELS = ("hb_ray_kernel", "hb_ray_lds_kernel")


def _spec(c):
    return dict(frame=c["frame"], frame_body=c["frame_body"], bodyexclude=c["bodyexclude"], static=c["static"], moving=c["moving"], cutoff=c["cutoff"])


def _chain_model(hbmod, c):
    return hbmod.Model.from_xml_string(c["xml"])


def _cast(hbmod, m, c, states, gpu):
    b = hbmod.Batch(m, len(states), gpu)
    b.set_state(hbmod.STATE_INTEGRATION, np.asarray(states))
    b.ray_configure(c["pnt"], c["vec"], **_spec(c))
    dist, gid = b.rays()
    kernel = b.last_kernel()
    b.close()
    return dist, gid, kernel


def _hold(name, refs, dist, gid, planted):
    worst, robust, fragile = 0.0, 0, 0
    for e, res in enumerate(refs):
        w, r, f = ray_cases.compare(res, dist[e], gid[e])
        worst, robust, fragile = max(worst, w), robust + r, fragile + f
    print("%s: %d robust rays, worst |dist - ref| / max(1, ref) %.3g; %d fragile" % (name, robust, worst, fragile))
    assert fragile == len(planted) * len(refs)
    assert worst <= BOUND, (name, worst)
    return worst


@pytest.mark.parametrize("frame", ["world", "body", "yaw"])
def test_primitives(hbmod, gpu, frame):
    """plane, spheres and capsules of the 12-dof chain from its base body, the base's own geom excluded: 70 rays = a full wave and six"""
    c = ray_cases.case("prim_" + frame)
    dist, gid, kernel = _cast(hbmod, _chain_model(hbmod, c), c, c["states"], gpu)
    assert kernel == "hb_ray_kernel" and dist.shape == gid.shape == (3, 70) and dist.dtype == np.float32 and gid.dtype == np.int32
    _hold("prim_" + frame, ray_cases.chain_reference("prim_" + frame), dist, gid, c["planted"])
    assert (gid == -1).any() and (gid == 0).any() and (gid >= 2).any() and not (gid == 1).any()
    assert np.array_equal(dist[gid < 0], np.full((gid < 0).sum(), -1, dtype=np.float32))


@pytest.mark.parametrize("name", ["hf_scan", "hf_misc", "hf_cutoff"])
def test_height_field(hbmod, gpu, name):
    """the 5 x 5 field: a yaw-frame scan; oblique rays, rays that enter from outside, leave without a hit, run along either axis, come
    from below, and the planted ones; a cutoff through the middle of the set"""
    c = ray_cases.case(name)
    dist, gid, kernel = _cast(hbmod, _chain_model(hbmod, c), c, c["states"], gpu)
    assert kernel == "hb_ray_lds_kernel"
    _hold(name, ray_cases.chain_reference(name), dist, gid, c["planted"])
    if name == "hf_cutoff":
        assert (gid < 0).sum() >= 30 and (gid == 0).sum() >= 30 and dist.max() <= c["cutoff"]


def test_per_env_terrain(hbmod, gpu):
    """an env-adapter batch with per-env elevations: every env's scan is that of ITS terrain"""
    import dr_ref
    c = ray_cases.case("terrain")
    m = hbmod.Model.load(c["hbm"])
    n = 4
    b = hbmod.Batch(m, n, gpu)
    b.env_configure(b.env_default_config())
    D = b.env_default_domain_randomization()
    D.seed, D.factor, D.floor_bump_min, D.floor_bump_max = 5, 1.0, 0.0, 0.1
    b.env_domain_randomize(D)
    b.env_reset()
    b.ray_configure(c["pnt"], c["vec"], **_spec(c))
    dist, gid = b.rays()
    assert b.last_kernel() == "hb_ray_lds_kernel"
    P = b.env_domain_params()
    elev = dr_ref.table(P, dr_ref.layout(m, P.shape[1]), "hfield")
    states = b.get_state(hbmod.STATE_INTEGRATION, dtype=np.float64)
    b.close()
    assert np.abs(elev[0] - elev[1]).max() > 0.02
    o = Oracle(c["hbm"])
    refs = [ray_cases.reference_at(o, c, states[e], hfield_data=elev[e]) for e in range(n)]
    nfrag = sum(int(ray_ref.fragile(r).sum()) for r in refs)
    assert nfrag <= 0.05 * n * len(c["pnt"])
    worst = max(ray_cases.compare(refs[e], dist[e], gid[e])[0] for e in range(n))
    print("terrain: worst %.3g, %d fragile" % (worst, nfrag))
    assert worst <= BOUND
    assert (gid == 0).all() and np.abs(dist[0] - dist[1]).max() > 0.01  # (the same pose over different terrain)
    # against the model's own elevations the same rows would be off by centimetres: the env's own block was read
    own = ray_cases.reference_at(o, c, states[0])
    assert np.abs(own["dist"] - dist[0]).max() > 0.01


def test_team_robot(hbmod, gpu):
    """the reference's robot: its static-only scan sees the height-field floor (the world's axis cylinders are markers); a spec with its
    mesh hulls in it is refused by name, and the batch goes on as before"""
    c = ray_cases.case("team")
    m = hbmod.Model.load(c["hbm"])
    states = ray_cases.team_states(4)
    b = hbmod.Batch(m, len(states), gpu)
    b.set_state(hbmod.STATE_INTEGRATION, states)
    b.ray_configure(c["pnt"], c["vec"], **_spec(c))
    dist, gid = b.rays()
    o = Oracle(c["hbm"])
    refs = [ray_cases.reference_at(o, c, s) for s in states]
    _hold("team", refs, dist, gid, [])
    assert (gid == 3).all()
    with pytest.raises(hbmod.HbError, match=r"code -4.*geom 4 .*mesh"):
        b.ray_configure(c["pnt"][:5], c["vec"][:5], frame="yaw", frame_body=1, static=True, moving=True)
    again = b.rays()
    assert np.array_equal(again[0], dist) and np.array_equal(again[1], gid)
    b.step(np.zeros((len(states), m.nu), dtype=np.float32))
    assert not b.status().any() and not np.array_equal(b.get_state(hbmod.STATE_QPOS), states[:, 1:1 + m.nq].astype(np.float32))
    assert b.rays()[0].shape == dist.shape
    b.close()


def test_nothing_is_written(hbmod, gpu):
    """state, status, counts, launch count and the next step are those of a twin that never cast a ray; the device form is the host form"""
    c = ray_cases.case("prim_body")
    m = _chain_model(hbmod, c)
    states = np.tile(c["states"], (2, 1))[:5]
    ctrl = np.random.default_rng(2).uniform(-1, 1, (5, m.nu)).astype(np.float32)
    a, twin = hbmod.Batch(m, 5, gpu), hbmod.Batch(m, 5, gpu)
    for b in (a, twin):
        b.set_state(hbmod.STATE_INTEGRATION, states)
        b.step(ctrl)
    a.ray_configure(c["pnt"], c["vec"], **_spec(c))
    before = snapshot(hbmod, a)
    dist, gid = a.rays()
    assert a.last_kernel() in KERNELS
    for x, y in zip(before, snapshot(hbmod, a)):
        assert np.array_equal(x, y)
    dd, dg = a.dev_alloc(dist.nbytes), a.dev_alloc(gid.nbytes)
    a.rays_dev(dd, dg)
    a.sync()
    assert np.array_equal(a.from_dev(dd, dist.shape), dist) and np.array_equal(a.from_dev(dg, gid.shape, np.int32), gid)
    a.rays_dev(dd, None)  # either output alone
    a.rays_dev(None, dg)
    a.sync()
    assert np.array_equal(a.from_dev(dd, dist.shape), dist) and np.array_equal(a.from_dev(dg, gid.shape, np.int32), gid)
    for x, y in zip(before, snapshot(hbmod, a)):
        assert np.array_equal(x, y)
    a.dev_free(dd); a.dev_free(dg)
    for b in (a, twin):
        b.step(ctrl)
    assert np.array_equal(a.get_state(hbmod.STATE_INTEGRATION), twin.get_state(hbmod.STATE_INTEGRATION))
    assert np.array_equal(a.status(), twin.status()) and all(np.array_equal(x, y) for x, y in zip(a.counts(), twin.counts()))
    a.close(); twin.close()


def test_held_step_calls_come_first(hbmod, gpu, humanoid_model):
    """folded hb_step_dev calls held back on a pipelined batch are launched before the rays: the same rows as after an explicit sync"""
    m = humanoid_model
    n = 256
    p, v = hbmod.height_scan_rays(np.linspace(-0.5, 0.5, 5), np.linspace(-0.3, 0.3, 3), 1.0)
    ctrl = np.random.default_rng(3).uniform(-1, 1, (n, m.nu)).astype(np.float32)
    outs = []
    for sync_first in (False, True):
        b = hbmod.Batch(m, n, gpu)
        b.pipeline(True)
        b.reset(perturb=True)
        b.ray_configure(p, v, frame="yaw", frame_body=1, bodyexclude=1)
        first = b.rays()
        d = b.dev_alloc(ctrl.nbytes)
        b.to_dev(d, ctrl)
        n0 = b.step_launches()
        for _ in range(3):
            b.step_dev(d)
        if sync_first:
            b.sync()
        outs.append(b.rays())
        assert b.step_launches() - n0 in (1, 3)
        b.sync()
        assert not np.array_equal(first[0], outs[-1][0])  # (the state moved)
        b.dev_free(d)
        b.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("name", ["prim_body", "hf_misc"])
def test_same_bits_per_ray(hbmod, gpu, name):
    """a ray's row in a 1-env and in a 5-env batch, and wherever the ray stands in the array"""
    c = ray_cases.case(name)
    m = _chain_model(hbmod, c)
    five = np.tile(c["states"], (2, 1))[:5]
    dist, gid, _ = _cast(hbmod, m, c, five, gpu)
    for e in (0, 4):
        d1, g1, _ = _cast(hbmod, m, c, five[e:e + 1], gpu)
        assert np.array_equal(d1[0], dist[e]) and np.array_equal(g1[0], gid[e])
    perm = np.random.default_rng(1).permutation(len(c["pnt"]))
    cp = dict(c, pnt=c["pnt"][perm], vec=c["vec"][perm])
    dp, gp, _ = _cast(hbmod, m, cp, five, gpu)
    assert np.array_equal(dp, dist[:, perm]) and np.array_equal(gp, gid[:, perm])
    few = dict(c, pnt=c["pnt"][60:63], vec=c["vec"][60:63])  # three rays of the second wave, alone in a launch
    df, gf, _ = _cast(hbmod, m, few, five, gpu)
    assert np.array_equal(df, dist[:, 60:63]) and np.array_equal(gf, gid[:, 60:63])


def test_argument_errors(hbmod, gpu, humanoid_model):
    """every HB_EINVAL case of include/hb.h; a refused call leaves the configuration as it was; the batch steps afterwards"""
    m = humanoid_model
    L = hbmod.lib()
    b = hbmod.Batch(m, 3, gpu)
    b.reset()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p, v = hbmod.height_scan_rays([0.0, 0.2], [0.0], 1.0)
    dist, gid = np.zeros((3, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.int32)
    spec = hbmod.engine.HbRaySpec(2, 1, -1, 3, 0.0)
    EINVAL = L.hb_rays(None, P(dist), P(gid))
    assert EINVAL == -1 and L.hb_rays_dev(None, P(dist), P(gid)) == EINVAL and L.hb_ray_configure(None, ctypes.byref(spec), P(p), P(v), 2) == EINVAL
    # nothing configured
    assert L.hb_rays(b._h, P(dist), P(gid)) == EINVAL and L.hb_rays_dev(b._h, P(dist), P(gid)) == EINVAL
    with pytest.raises(hbmod.HbError):
        b.rays()
    b.ray_configure(p, v, frame="yaw", frame_body=1)
    # both outputs NULL
    assert L.hb_rays(b._h, None, None) == EINVAL and L.hb_rays_dev(b._h, None, None) == EINVAL
    good = b.rays()
    bad_vec = v.copy(); bad_vec[1] = 0
    nan_vec = v.copy(); nan_vec[0, 2] = np.nan
    for fields, pp, vv, n in (((2, m.nbody, -1, 3, 0.0), p, v, 2), ((2, -1, -1, 3, 0.0), p, v, 2),       # frame_body out of range
                              ((2, 1, m.nbody, 3, 0.0), p, v, 2), ((2, 1, -2, 3, 0.0), p, v, 2),       # bodyexclude out of range
                              ((2, 1, -1, 0, 0.0), p, v, 2), ((2, 1, -1, 4, 0.0), p, v, 2),            # flags without an eligibility bit
                              ((3, 1, -1, 3, 0.0), p, v, 2),                                           # an unknown frame
                              ((2, 1, -1, 3, 0.0), p, bad_vec, 2), ((2, 1, -1, 3, 0.0), p, nan_vec, 2),  # a zero / non-finite vector
                              ((2, 1, -1, 3, 0.0), p, v, -1), ((2, 1, -1, 3, 0.0), p, v, 4097)):         # n_ray out of range
        s = hbmod.engine.HbRaySpec(*fields)
        assert L.hb_ray_configure(b._h, ctypes.byref(s), P(pp), P(vv), n) == EINVAL, fields
    assert L.hb_ray_configure(b._h, ctypes.byref(spec), None, P(v), 2) == EINVAL and L.hb_ray_configure(b._h, ctypes.byref(spec), P(p), None, 2) == EINVAL
    after = b.rays()
    assert np.array_equal(after[0], good[0]) and np.array_equal(after[1], good[1])
    big = np.tile(p, (2048, 1))  # 4096 rays: the most
    b.ray_configure(big, np.tile(v, (2048, 1)), frame="yaw", frame_body=1)
    d4, g4 = b.rays()
    assert d4.shape == (3, 4096) and np.array_equal(d4[:, :2], good[0]) and np.array_equal(d4[:, 4094:], good[0]) and np.array_equal(g4[:, 4094:], good[1])
    b.ray_configure(None, None)  # remove
    assert L.hb_rays(b._h, P(dist), P(gid)) == EINVAL
    b.step(np.zeros((3, m.nu), dtype=np.float32))
    assert not b.status().any()
    b.close()


def test_vecenv(hbmod, gpu):
    """height_scan() and height_scan_torch() agree, have the documented shape and fill, and their presence changes no step output"""
    import torch
    m = hbmod.Model.load(ray_cases.HFIELD_HBM)
    xs, ys = np.linspace(-1.0, 1.0, 6) + 0.017, np.linspace(-0.6, 0.6, 4) + 0.011
    cutoff = 2.29  # (the torso stands 1.28 m over elevations of up to 4 cm: through the middle of the scan's distances)
    env = hbmod.VecEnv(m, 4, device=gpu, randomization_factor=0.0, height_scan=dict(body="torso", xs=xs, ys=ys, z0=1.0, cutoff=cutoff))
    twin = hbmod.VecEnv(m, 4, device=gpu, randomization_factor=0.0)
    with pytest.raises(RuntimeError):
        twin.height_scan()
    assert np.array_equal(env.reset(), twin.reset())
    scan = env.height_scan()
    assert scan.shape == (4, 4, 6) and scan.dtype == np.float32
    assert (scan == np.float32(cutoff)).any() and (scan < cutoff).any() and scan.max() <= np.float32(cutoff) and scan.min() > 2.2
    dist, gid = env.batch.rays()
    assert np.array_equal(scan.reshape(4, -1), np.where(gid >= 0, dist, np.float32(cutoff)))
    rng = np.random.default_rng(4)
    for k in range(4):
        act = rng.uniform(-1, 1, (4, m.nu)).astype(np.float32)
        a, t = env.step_arrays(act), twin.step_arrays(act)
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], t[:4]))
        if k == 1:
            env.height_scan()
    act = torch.from_numpy(rng.uniform(-1, 1, (4, m.nu)).astype(np.float32)).cuda(gpu)
    o1 = [x.cpu().numpy() for x in env.step_torch(act)]
    ts = env.height_scan_torch()  # (ordered behind the step just enqueued)
    o2 = [x.cpu().numpy() for x in twin.step_torch(act)]
    assert all(np.array_equal(x, y) for x, y in zip(o1, o2))
    assert ts.is_cuda and tuple(ts.shape) == (4, 4, 6) and ts.dtype == torch.float32
    assert np.array_equal(ts.cpu().numpy(), env.height_scan())
    del act, ts  # (tensors the batches' streams still have a claim on go before the streams do)
    torch.cuda.synchronize()
    env.close(); twin.close()

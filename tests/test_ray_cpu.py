"""The fp64 ray reference (tests/ray_ref.py) against known answers, the collider's triangulation against the oracle's, the shapes of
height_scan_rays, and - from the reference alone - the fragility of every ray set tests/test_gpu_ray.py casts on the GPU.  No GPU."""
import numpy as np
import pytest

import ray_cases
import ray_ref
from kernel_models import oracle_for

EYE = np.eye(3)[None]


def _one(gtype, size, pnt, vec, **kw):
    info = dict(ngeom=1, geom_bodyid=[0], geom_type=[gtype], geom_contype=[1], geom_conaffinity=[1], geom_size=list(size), geom_dataid=[0])
    info.update(kw.pop("info", {}))
    r = ray_ref.cast(info, np.zeros((1, 3)), EYE, np.atleast_2d(pnt), np.atleast_2d(vec), **kw)
    return {k: v[0] for k, v in r.items()}


def test_sphere():
    out = _one(ray_ref.SPHERE, (0.5, 0, 0), [3, 0, 0], [-2, 0, 0])  # (the direction is normalised)
    assert out["geomid"] == 0 and abs(out["dist"] - 2.5) < 1e-14 and abs(out["second"] - 3.5) < 1e-14 and abs(out["cosine"] - 1) < 1e-14
    inside = _one(ray_ref.SPHERE, (0.5, 0, 0), [0.1, 0, 0], [1, 0, 0])  # from inside: the exit point
    assert inside["geomid"] == 0 and abs(inside["dist"] - 0.4) < 1e-14
    tangent = _one(ray_ref.SPHERE, (0.5, 0, 0), [3, 0.5 + 1e-6, 0], [-1, 0, 0])  # a miss by a micrometre: fragile
    assert tangent["geomid"] == -1 and tangent["dist"] == -1 and abs(tangent["clearance"] - 1e-6) < 1e-12
    assert ray_ref.fragile({k: np.array([v]) for k, v in tangent.items()})[0]
    away = _one(ray_ref.SPHERE, (0.5, 0, 0), [3, 0, 0], [1, 0, 0])
    assert away["geomid"] == -1 and abs(away["clearance"] - 2.5) < 1e-14


def test_capsule():
    wall = _one(ray_ref.CAPSULE, (0.2, 0.5, 0), [2, 0, 0.3], [-1, 0, 0])
    assert wall["geomid"] == 0 and abs(wall["dist"] - 1.8) < 1e-14
    cap = _one(ray_ref.CAPSULE, (0.2, 0.5, 0), [0, 0, 3], [0, 0, -1])
    assert abs(cap["dist"] - 2.3) < 1e-14
    skew = _one(ray_ref.CAPSULE, (0.2, 0.5, 0), [0.1, 0, 3], [0, 0, -1])  # on the cap, off the axis
    assert abs(skew["dist"] - (2.5 - np.sqrt(0.04 - 0.01))) < 1e-14
    inside = _one(ray_ref.CAPSULE, (0.2, 0.5, 0), [0, 0, -0.6], [0, 0, 1])  # inside the lower cap: out through the upper one, not the
    assert abs(inside["dist"] - 1.3) < 1e-14                              # lower sphere's inner half
    assert _one(ray_ref.CAPSULE, (0.2, 0.5, 0), [2, 0, 0.71], [-1, 0, 0])["geomid"] == -1  # over the cap


def test_plane():
    hit = _one(ray_ref.PLANE, (1.0, 0.5, 1), [0.5, 0.2, 2], [0, 0, -1])
    assert hit["geomid"] == 0 and abs(hit["dist"] - 2) < 1e-14
    assert _one(ray_ref.PLANE, (1.0, 0.5, 1), [0.5, 0.2, -2], [0, 0, 1])["dist"] == 2  # from below as well
    out = _one(ray_ref.PLANE, (1.0, 0.5, 1), [0.5, 0.6, 2], [0, 0, -1])
    assert out["geomid"] == -1 and abs(out["clearance"] - 0.1) < 1e-14
    assert abs(_one(ray_ref.PLANE, (0, 0, 1), [50, 60, 2], [0, 0, -1])["dist"] - 2) < 1e-14  # size 0: infinite
    assert _one(ray_ref.PLANE, (0, 0, 1), [0, 0, 2], [1, 0, 0])["geomid"] == -1
    assert abs(_one(ray_ref.PLANE, (0, 0, 1), [0, 0, 2], [1, 0, 0], cutoff=5.0)["clearance"] - 2) < 1e-14
    cut = _one(ray_ref.PLANE, (0, 0, 1), [0, 0, 2], [0, 0, -1], cutoff=1.5)
    assert cut["geomid"] == -1 and abs(cut["clearance"] - 0.5) < 1e-14


def _field(elev, size=(2.0, 1.0, 0.5, 0.1)):
    e = np.asarray(elev, dtype=np.float64)
    return dict(hfield_nrow=[e.shape[0]], hfield_ncol=[e.shape[1]], hfield_adr=[0], hfield_size=list(size), hfield_data=e.reshape(-1))


def test_height_field():
    flat = _field(np.full((3, 4), 0.6))
    for x, y in ((0.3, -0.2), (-1.9, 0.9), (0.0, 0.0)):  # (the last on a vertex... of a flat field: the same height from every triangle)
        out = _one(ray_ref.HFIELD, (0, 0, 0), [x, y, 2], [0, 0, -1], info=flat)
        assert out["geomid"] == 0 and abs(out["dist"] - 1.7) < 1e-14
    assert _one(ray_ref.HFIELD, (0, 0, 0), [2.1, 0, 2], [0, 0, -1], info=flat)["geomid"] == -1  # beside the extent: no walls, no base
    assert abs(_one(ray_ref.HFIELD, (0, 0, 0), [0.3, 0.2, -1], [0, 0, 1], info=flat)["dist"] - 1.3) < 1e-14  # the underside
    rng = np.random.default_rng(0)
    e = rng.uniform(0, 1, (4, 5))
    f = _field(e)
    for r in range(3):
        for c in range(4):  # a cell's centre lies on its cut: the mean of the (r, c) and (r + 1, c + 1) corners
            x, y = -2 + 4 * (c + 0.5) / 4, -1 + 2 * (r + 0.5) / 3
            out = _one(ray_ref.HFIELD, (0, 0, 0), [x, y, 3], [0, 0, -1], info=f)
            assert abs(3 - out["dist"] - 0.5 * 0.5 * (e[r, c] + e[r + 1, c + 1])) < 1e-13
            assert abs(out["second"] - out["dist"]) < 1e-12  # (both halves of the cell are hit there: fragile)
            # a quarter of the way along the OTHER diagonal from (r, c + 1): inside the half with that corner, a plane through it
            xq, yq = -2 + 4 * (c + 0.75) / 4, -1 + 2 * (r + 0.25) / 3
            want = 0.5 * e[r, c + 1] + 0.25 * (e[r, c] + e[r + 1, c + 1])
            assert abs(3 - _one(ray_ref.HFIELD, (0, 0, 0), [xq, yq, 3], [0, 0, -1], info=f)["dist"] - 0.5 * want) < 1e-13


SADDLE = ('<mujoco model="saddle"><option timestep="0.002"/><asset><hfield name="h" nrow="2" ncol="2" size="1 1 0.5 0.1" elevation="%s"/></asset>'
          '<worldbody><geom name="floor" type="hfield" hfield="h"/><body name="ball" pos="0 0 %g"><freejoint/><geom type="sphere" size="0.05"/></body>'
          '</worldbody></mujoco>')


@pytest.mark.parametrize("elev", ["1 0 0 1", "0 1 1 0"])
def test_the_cut_is_the_oracles(hbmod, tmp_path, elev):
    """A one-cell saddle: cut along (0, 0) - (1, 1) the centre is a ridge at full height when those two corners are the high ones and the
    bottom of a valley when they are the low ones; cut the other way it would be the opposite.  The oracle's collider (convex_hfield's
    strip order), with a ball 1 cm into where the ridge would be, and the reference's surface must tell the same story."""
    m, path, o = oracle_for(hbmod, SADDLE % (elev, 0.5 + 0.05 - 0.01), tmp_path)
    data = np.asarray(o.info["hfield_data"]).reshape(2, 2)  # (the compiler stores the rows of the elevation attribute bottom row first)
    ridge = bool(data[0, 0] == 1 and data[1, 1] == 1)
    assert sorted(data.reshape(-1).tolist()) == [0, 0, 1, 1] and data[0, 0] == data[1, 1] != data[0, 1] == data[1, 0]
    o.reset()
    o.forward()
    assert (o.ncon > 0) == ridge
    if ridge:
        assert abs(o.contacts()[0]["dist"] + 0.01) < 5e-3
    res = ray_ref.reference(o, [[0, 0, 2.0]], [[0, 0, -1]], flags=ray_ref.STATIC)  # through the ball, which a static spec does not see
    assert res["geomid"][0] == 0 and abs(2.0 - res["dist"][0] - (0.5 if ridge else 0.0)) < 1e-14


def test_frames():
    q = np.array([np.cos(0.35), 0.3 * np.sin(0.35), -0.2 * np.sin(0.35), np.sqrt(1 - 0.13) * np.sin(0.35)])
    pos = np.array([0.3, -0.2, 1.1])
    R = ray_ref.quat_to_mat(q)
    p, v = ray_ref.world_rays(ray_ref.FRAME_BODY, pos, q, [[0.1, 0.2, 0.3]], [[0, 0, -2]])
    assert np.allclose(p[0], pos + R @ [0.1, 0.2, 0.3], atol=1e-15) and np.allclose(v[0], -R[:, 2], atol=1e-15)
    p, v = ray_ref.world_rays(ray_ref.FRAME_YAW, pos, q, [[1, 0, 0.5], [0, 1, 0.5]], [[0, 0, -1], [1, 0, 0]])
    hx = R[:2, 0] / np.linalg.norm(R[:2, 0])
    assert np.allclose(p[0], pos + [hx[0], hx[1], 0.5], atol=1e-15) and np.allclose(p[1], pos + [-hx[1], hx[0], 0.5], atol=1e-15)
    assert np.allclose(v[0], [0, 0, -1], atol=1e-15) and np.allclose(v[1], [hx[0], hx[1], 0], atol=1e-15)
    up = np.array([np.sqrt(0.5), 0, -np.sqrt(0.5), 0])  # the body's x axis points straight up: the world x axis takes over
    p, _ = ray_ref.world_rays(ray_ref.FRAME_YAW, pos, up, [[1, 0, 0]], [[0, 0, -1]])
    assert np.allclose(p[0], pos + [1, 0, 0], atol=1e-15)


def test_markers_and_refusals():
    info = dict(ngeom=3, geom_bodyid=[0, 0, 1], geom_type=[5, 0, 7], geom_contype=[0, 1, 1], geom_conaffinity=[0, 1, 1])
    assert ray_ref.eligible_geoms(info, ray_ref.STATIC) == [1]  # (a cylinder that collides with nothing is a marker: skipped)
    with pytest.raises(ValueError, match="geom 2"):
        ray_ref.eligible_geoms(info, ray_ref.STATIC | ray_ref.MOVING)
    assert ray_ref.eligible_geoms(info, ray_ref.STATIC | ray_ref.MOVING, bodyexclude=1) == [1]


def test_height_scan_rays(hbmod):
    xs, ys = np.linspace(-1, 1, 17), np.linspace(-0.5, 0.5, 11)
    p, v = hbmod.height_scan_rays(xs, ys, 0.8)
    assert p.shape == v.shape == (17 * 11, 3) and p.dtype == v.dtype == np.float32
    grid = p.reshape(11, 17, 3)
    assert np.array_equal(grid[:, :, 0], np.tile(xs.astype(np.float32), (11, 1))) and np.array_equal(grid[:, :, 1], np.tile(ys.astype(np.float32)[:, None], (1, 17)))
    assert np.all(grid[:, :, 2] == np.float32(0.8)) and np.array_equal(v, np.tile(np.array([0, 0, -1], dtype=np.float32), (187, 1)))
    assert hbmod.height_scan_rays([0.5], [0.25])[0].tolist() == [[0.5, 0.25, 1.0]]


@pytest.mark.parametrize("name", ray_cases.CHAIN_CASES)
def test_the_gpu_ray_sets_are_robust(name):
    """at most 5 % of a set is fragile, and only the rays planted on grid lines, vertices and cuts are - all of those"""
    c = ray_cases.case(name)
    n = len(c["pnt"])
    assert n <= 150 and len(c["states"]) == 3
    for res in ray_cases.chain_reference(name):
        fr = np.flatnonzero(ray_ref.fragile(res)).tolist()
        assert fr == c["planted"], (name, fr)
        assert len(fr) <= 0.05 * n
    if name.startswith("prim_"):
        assert n == 70
        hit = set(np.concatenate([r["geomid"] for r in ray_cases.chain_reference(name)]).tolist())
        assert {-1, 0} <= hit and len(hit - {-1, 0}) >= 1  # misses, the floor, capsules
    if name == "hf_cutoff":
        for res in ray_cases.chain_reference(name):
            assert 10 <= (res["geomid"] >= 0).sum() <= n - 10  # (the cutoff cuts through the set)


@pytest.mark.parametrize("name", ["team", "terrain"])
def test_the_asset_scans_are_robust(name):
    """the yaw-frame scans of the two assets' fields at the model's own elevations (the per-env ones exist on the device only: the GPU
    test holds the same share there)"""
    from oracle_lib import Oracle
    c = ray_cases.case(name)
    o = Oracle(c["hbm"])
    if name == "team":
        states = ray_cases.team_states(4)
    else:
        o.reset()
        states = [np.concatenate([[0.0], o.qpos, o.qvel, o.qacc_warmstart])]
    for s in states:
        res = ray_cases.reference_at(o, c, s)
        assert (res["geomid"] >= 0).all() and not ray_ref.fragile(res).any()

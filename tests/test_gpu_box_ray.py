"""Rays against box geoms (csrc/hb_ray.hip: ray_box) on the GPU: the fp64 reference is tests/box_ref.py's ray_box for the boxes and
tests/ray_ref.py for every other surface of the scene, the nearest hit winning (ties to the lowest geom id, as the kernel walks them).

The scene is tests/box_cases.py's: a tilted plane, a height field, the static box W and the moving boxes P and Q beside a sphere and a
capsule.  64 rays x 8 envs, in the world frame (half of them aimed at W and what lies on it, half at the height field and what hovers over
it), in the sphere S's body frame and in its yaw frame (S itself excluded, half of the rays aimed at the box P beside it).  BOUND is tests/test_gpu_ray.py's, bounds.RAY_BOUND (profiles/ray_parity.txt): 1e-5 relative to max(1, dist).
A ray is FRAGILE as in ray_ref (second candidate within 1e-4, grazing below |cos| 0.05, a miss that clears a surface by less than 1e-4
- for a box: a miss that hits the box grown by 1e-4) and then may give either candidate.

The stairs model (tests/models/box_stairs.xml): VecEnv(height_scan=...) returns the step heights, and with obs_extend the scan columns of
the observation are height_scan_torch() through the configured affine map and clamp, bit for bit.
"""
import numpy as np
import pytest

import box_cases
import box_ref
import obs_ext_ref
import pair_ref
import ray_ref
from oracle_lib import parse_hbm
from bounds import RAY_BOUND as BOUND

pytestmark = pytest.mark.gpu
N_ENV, N_RAY = 8, 64


def _scene(hbmod, tmp_path):
    m = hbmod.Model.from_xml_string(box_cases.scene_xml("pgs"))
    p = str(tmp_path / "boxes.hbm")
    m.save(p)
    return m, parse_hbm(p)


P_OFFSET = np.array([0.4, 0.05, -0.05])  # where the box P stands in the frame the rays of S are given in


def _states(info, frame):
    """8 states: P and S hover over the height field, Q and X lie on and beside the static box W, all in generic orientations.  For the
    rays of S's body and yaw frames P stands at P_OFFSET in that frame of S, so that rays aimed there find it in every env."""
    rng = np.random.default_rng(11)
    out = []
    for e in range(N_ENV):
        q = np.zeros(28)
        for k, (anchor, lift) in enumerate(((box_cases.FIELD_POS, 0.35), (box_cases.FIELD_POS, 0.6), (box_cases.W_POS, 0.3), (box_cases.W_POS, 0.5))):
            q[7 * k:7 * k + 3] = anchor + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), lift + rng.uniform(0, 0.1)])
            q[7 * k + 3:7 * k + 7] = box_cases._qrand(rng)
        if frame != "world":
            q[0:3] = ray_ref.world_rays({"body": 1, "yaw": 2}[frame], q[7:10], q[10:14], P_OFFSET, [1.0, 0, 0])[0][0]
        out.append(np.concatenate([[0.0], q.astype(np.float32).astype(np.float64), np.zeros(48)]))
    return np.array(out)


def _rays(frame):
    rng = np.random.default_rng(5)
    if frame == "world":
        anchors = [box_cases.FIELD_POS] * (N_RAY // 2) + [box_cases.W_POS] * (N_RAY // 2)
        pnt = np.array([a + np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(0.9, 1.4)]) for a in anchors])
        tgt = np.array([a + np.array([rng.uniform(-0.45, 0.45), rng.uniform(-0.45, 0.45), rng.uniform(0.0, 0.5)]) for a in anchors])
        return pnt, tgt - pnt
    # in S's frame (S's own sphere excluded): from a shell around it, half of them towards the box P, half anywhere - the field and the
    # plane below are in sight too
    pnt = rng.standard_normal((N_RAY, 3))
    pnt = pnt / np.linalg.norm(pnt, axis=1, keepdims=True) * rng.uniform(0.08, 0.2, (N_RAY, 1))
    vec = rng.standard_normal((N_RAY, 3))
    vec[::2] = P_OFFSET + rng.uniform(-0.12, 0.12, (N_RAY // 2, 3)) - pnt[::2]
    return pnt, vec


def _reference(info, state, pnt, vec, frame, frame_body, bodyexclude, cutoff):
    gpos, gmat = pair_ref.geom_poses(info, state[1:29])
    gpos, gmat = np.array(gpos), np.array(gmat)
    q = state[1:29]
    b = frame_body
    xpos = np.zeros(3) if b == 0 else q[7 * (b - 1):7 * (b - 1) + 3]
    xquat = np.array([1.0, 0, 0, 0]) if b == 0 else q[7 * (b - 1) + 3:7 * (b - 1) + 7]
    pw, vw = ray_ref.world_rays({"world": ray_ref.FRAME_WORLD, "body": ray_ref.FRAME_BODY, "yaw": ray_ref.FRAME_YAW}[frame], xpos, xquat, pnt, vec)
    # every surface but the boxes through ray_ref (the boxes marked as markers, which it passes over) ...
    rest = dict(info)
    box = info["geom_type"] == box_ref.GEOM_BOX
    rest["geom_contype"], rest["geom_conaffinity"] = np.where(box, 0, info["geom_contype"]), np.where(box, 0, info["geom_conaffinity"])
    res = ray_ref.cast(rest, gpos, gmat, pw, vw, bodyexclude=bodyexclude, cutoff=cutoff)
    frag = ray_ref.fragile(res)
    dist, gid, second = res["dist"].copy(), res["geomid"].copy(), res["second"].copy()
    size = info["geom_size"].reshape(-1, 3)
    limit = cutoff if cutoff > 0 else np.inf
    for i in range(len(pw)):
        cands = [] if gid[i] < 0 else [(dist[i], int(gid[i]), 1.0)]
        if np.isfinite(second[i]):
            cands.append((second[i], int(res["second_geom"][i]), 1.0))
        for g in np.flatnonzero(box):
            if info["geom_bodyid"][g] == bodyexclude:
                continue
            o, d = gmat[g].T @ (pw[i] - gpos[g]), gmat[g].T @ vw[i]
            hits = box_ref.ray_box(o, d, size[g])[1]
            cands += [(t, int(g), c) for t, c in hits if t <= limit]
            if not hits and box_ref.ray_box(o, d, size[g] + ray_ref.FRAGILE_DIST)[1]:
                frag[i] = True
        cands.sort()
        if cands:
            dist[i], gid[i] = cands[0][0], cands[0][1]
            frag[i] |= cands[0][2] < ray_ref.FRAGILE_COS or (len(cands) > 1 and cands[1][0] - cands[0][0] < ray_ref.FRAGILE_DIST and cands[1][1] != cands[0][1])
            frag[i] |= len(cands) > 1 and cands[1][0] - cands[0][0] < ray_ref.FRAGILE_DIST
    return dist, gid, frag


@pytest.mark.parametrize("frame", ["world", "body", "yaw"])
def test_rays_against_boxes(hbmod, gpu, tmp_path, frame):
    m, info = _scene(hbmod, tmp_path)
    states = _states(info, frame)
    pnt, vec = _rays(frame)
    pnt, vec = pnt.astype(np.float32), vec.astype(np.float32)
    body = 0 if frame == "world" else 2  # S
    cutoff = 0.0 if frame == "world" else 12.0
    b = hbmod.Batch(m, N_ENV, gpu)
    b.set_state(hbmod.STATE_INTEGRATION, states)
    b.ray_configure(pnt, vec, frame=frame, frame_body=body, bodyexclude=body if body else -1, cutoff=cutoff)
    dist, gid = b.rays()
    assert b.last_kernel() == "hb_ray_lds_kernel"
    b.close()
    worst, robust, seen = 0.0, 0, set()
    for e in range(N_ENV):
        want_d, want_g, frag = _reference(info, states[e], pnt.astype(np.float64), vec.astype(np.float64), frame, body, body if body else -1, cutoff)
        for i in np.flatnonzero(~frag):
            assert int(gid[e, i]) == int(want_g[i]), (frame, e, i, gid[e, i], dist[e, i], want_g[i], want_d[i])
            if want_g[i] >= 0:
                worst = max(worst, abs(float(dist[e, i]) - want_d[i]) / max(1.0, want_d[i]))
                seen.add(int(info["geom_type"][want_g[i]]))
            else:
                assert dist[e, i] == -1.0
        robust += int((~frag).sum())
        boxes_hit = int((info["geom_type"][want_g[want_g >= 0]] == box_ref.GEOM_BOX).sum())
        assert boxes_hit >= 3, (frame, e, boxes_hit)
    print("\nrays, %s frame: %d robust of %d, worst |dist - ref| / max(1, ref) %.3g (bound %.0e), surfaces hit %s" % (frame, robust, N_ENV * N_RAY, worst, BOUND, sorted(seen)))
    assert robust >= 0.9 * N_ENV * N_RAY and worst <= BOUND
    assert box_ref.GEOM_BOX in seen and len(seen) >= 3
    if frame == "world":
        assert {box_ref.GEOM_HFIELD, box_ref.GEOM_SPHERE, box_ref.GEOM_CAPSULE} <= seen


def test_a_mesh_geom_is_still_refused_by_name(hbmod, gpu):
    m = hbmod.Model.from_xml_string(box_cases.scene_xml("mesh"))
    b = hbmod.Batch(m, 2, gpu)
    p, v = np.array([[0, 0, 1.0]], dtype=np.float32), np.array([[0, 0, -1.0]], dtype=np.float32)
    with pytest.raises(hbmod.HbError, match=r"code -4.*geom 6 \(X, a mesh geom.*boxes only"):
        b.ray_configure(p, v)
    b.ray_configure(p, v, moving=False)  # the static box W, the plane and the field alone: accepted
    assert b.rays()[1].shape == (2, 1)
    b.close()


# ---- the height scan over the stairs ----------------------------------------------------------------------------------------------------
XS = [box_cases.STEP_X0 + box_cases.STEP_RUN * k for k in range(box_cases.NSTEPS)] + [0.15, 1.7]  # the four treads, the floor before and behind
YS = [-0.3, 0.0, 0.25]
Z0, CUTOFF = 1.0, 4.0
HS = dict(offset=1.0, scale=2.0, clip=(-4.0, 5.0))


def test_height_scan_sees_the_stairs(hbmod, gpu):
    m = hbmod.Model.from_xml_string(box_cases.stairs_xml())
    torso = m.name2id("body", "torso")
    env = hbmod.VecEnv(m, 4, gpu, seed=3, target_z=10.0, height_scan=dict(body=torso, xs=XS, ys=YS, z0=Z0, cutoff=CUTOFF), obs_extend=dict(prev_action=True, height_scan=HS))
    obs = env.reset()  # (float32 [n_envs, nobs] on the host)
    scan = env.height_scan()
    assert scan.shape == (4, len(YS), len(XS))
    q = env.batch.qpos.astype(np.float64)
    # the reset keeps the torso upright and heading along x within the env's reset noise: the grid points stay on their treads (0.3 m deep,
    # the points at their middles), so every column has the height of its tread
    heights = np.array([box_cases.STEP_RISE * (k + 1) for k in range(box_cases.NSTEPS)] + [0.0, 0.0])
    for e in range(4):
        want = q[e, 2] + Z0 - heights
        assert np.abs(scan[e] - want[None, :]).max() <= BOUND * max(1.0, want.max()), (e, scan[e], want)
    # the observation's scan columns: height_scan_torch() through the affine map and the clamp, the same bits
    cols = env.obs_layout()["height_scan"]
    t = env.height_scan_torch().cpu().numpy().reshape(4, -1)
    want = obs_ext_ref.scan_entries(t, np.where(t < CUTOFF, 0, -1), CUTOFF, **HS)
    assert np.array_equal(obs[:, cols], want)
    env.close()

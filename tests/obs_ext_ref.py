"""Reference of the env adapter's observation extension (include/hb.h: hb_env_obs_extend): the row [prev_action | scan] composed in numpy
from the last action and a ray result - tests/ray_ref.py's fp64 cast (through tests/ray_cases.py) or the device's own hb_rays arrays.

TEST INFRASTRUCTURE: the product package never imports this module.

The transform is the header's, in float32 and in its order - a subtract, a multiply, a clamp, each rounded once:
    entry = clamp(scale * (offset - d), lo, hi),   d = the ray's distance, or the cutoff where nothing is hit
so that the bits of `scan_entries` on the device's distances are the bits the device must give.
"""
import numpy as np

import ray_cases


def scan_entries(dist, geomid, cutoff, offset=0.0, scale=1.0, clip=(-3.0e38, 3.0e38)):
    """float32 [...]: the scan columns of rays with distances `dist` (any float type; rounded to float32 first) and hit geoms `geomid`
    (< 0: nothing hit)"""
    f = np.float32
    d = np.where(np.asarray(geomid) >= 0, np.asarray(dist).astype(f), f(cutoff)).astype(f)
    v = (f(scale) * (f(offset) - d).astype(f)).astype(f)
    return np.minimum(np.maximum(v, f(clip[0])), f(clip[1])).astype(f)


def extension(latest, dist, geomid, cutoff, prev_action=True, height_scan=None):
    """float32 [n, n_ext]: prev_action (the rows of `latest` [n, nu]) | scan (height_scan: the dict of Batch.obs_extend, or None)"""
    parts = []
    if prev_action:
        parts.append(np.asarray(latest, dtype=np.float32))
    if height_scan is not None:
        parts.append(scan_entries(dist, geomid, cutoff, height_scan.get("offset", 0.0), height_scan.get("scale", 1.0), height_scan.get("clip", (-3.0e38, 3.0e38))))
    return np.concatenate(parts, axis=-1)


def reference_scan(o, c, state, height_scan, hfield_data=None):
    """(scan float32 [n_ray], ray_ref result) of case c's rays (ray_cases.case) with the oracle at one state record, in fp64 up to the
    transform's input"""
    res = ray_cases.reference_at(o, c, state, hfield_data=hfield_data)
    return scan_entries(res["dist"], res["geomid"], c["cutoff"], height_scan.get("offset", 0.0), height_scan.get("scale", 1.0),
                        height_scan.get("clip", (-3.0e38, 3.0e38))), res

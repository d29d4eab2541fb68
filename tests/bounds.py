"""The GPU-side tolerances that more than one test file holds the device to: each defined once, here, with the reasoning and the
measurement it came from.  A test file imports the bound it needs and never restates it; a bound that one file alone uses stays in
that file.

TEST INFRASTRUCTURE: the product package never imports this module.  It imports nothing, so that every module under tests/ can.
"""

# ---- one step of a step kernel against the fp64 oracle (tests/test_gpu_kernel_matrix.py, and every test of a step kernel since) - the
# golden bounds of tests/test_gpu_parity.py: qacc and efc_force within 4e-4 * max(1, max|.|), qpos within 4e-5 relative, qvel within
# 4e-4 * max(1, max|qvel|), contact dist / pos within 1e-5 and frame within 1e-3
BOUNDS = dict(qpos=4e-5, qvel=4e-4, qacc=4e-4, force=4e-4, dist=1e-5, pos=1e-5, frame=1e-3)

# ---- a free-running, contact-free window against the oracle (tests/test_gpu_parity.py): relative qpos drift, the north-star bar
FREE_RUNNING_BOUND = 1e-4

# ---- one step of an RK4 kernel against tests/rk4_ref.py (tests/test_gpu_rk4.py)
# Measured on MI355X against the fp64 reference, maximum over the six models (median of the worst model in brackets):
#   qpos 2.27e-6 (4.96e-8)   qvel 5.07e-5 (5.24e-7)   qacc = qacc_warmstart' 8.09e-5 (4.39e-6)   efc_force 9.63e-5 (3.48e-6)   time 1.14e-7
# - every one below the Euler step's bound itself (4e-5 / 4e-4), none near twice it.  Each bound is at most 3 x its measured maximum.
RK4_BOUNDS = dict(qpos=6e-6, qvel=1.5e-4, qacc=2.4e-4, warm=2.4e-4, force=2.8e-4, time=3e-7)

# ---- the general collision path against the oracle (tests/test_gpu_convex.py): at most 3x the maxima measured on the MI355X - contact
# distance 5e-7 m, position 3e-6 m, normal 3e-5; qacc 2e-4 and forces 3e-4 relative to their scale, qvel 1.5e-5, qpos 1e-6.  The pair
# and box case tables (tests/test_gpu_narrow_pairs.py, tests/test_gpu_box.py) take their BASE from dist, pos and nrm.
CONVEX_TOL = dict(qpos=1e-6, qvel=1.5e-5, qacc=2e-4, force=3e-4, dist=5e-7, pos=3e-6, nrm=3e-5)

# ---- a ray's distance against tests/ray_ref.py, relative to max(1, dist_ref) (tests/test_gpu_ray.py): the project's contact-geometry
# bound; profiles/ray_parity.txt: worst measured 2.141e-06, below it
RAY_BOUND = BOUNDS["pos"]

# ---- the read-outs, each against its fp64 reference and relative to max(1, max |.|) of the state: at most 3 x the maximum measured on
# MI355X.  The docstring of the test file named holds the measurement and the two tiers (decode: the device's own inputs; parity: the oracle's).
CONTACT_DECODE_BOUND, CONTACT_PARITY_BOUND = 1.5e-6, 5e-4  # tests/test_gpu_contact_force.py; of max |efc_force|
ACC_DECODE_BOUND, ACC_PARITY_BOUND = 1.8e-6, 2.7e-4        # tests/test_gpu_body_acc.py
POSE_BOUND, VEL_BOUND = 1.54e-6, 1.8e-6                    # tests/test_gpu_kinematics.py; capped at ACC_DECODE_BOUND (the same kinematics plus a longer sum)
assert POSE_BOUND <= ACC_DECODE_BOUND and VEL_BOUND <= ACC_DECODE_BOUND
DYN_BOUND = {"M": 8.44e-7, "bias": 5.02e-6, "passive": 2.04e-7, "jac": 1.66e-6}  # tests/test_gpu_dynamics.py
assert max(DYN_BOUND.values()) < BOUNDS["qacc"]

# ---- an MLP's output against the fp64 MLP, times max(1, |ref|): tests/test_gpu_policy.py's bound for this arithmetic (f32 MFMA chains,
# tanhf), which the actor's mean and log_std (tests/test_gpu_collect.py) and the critic's values (tests/test_gpu_gae.py) are held to
MEAN_TOL = 5e-5
VALUE_TOL = MEAN_TOL

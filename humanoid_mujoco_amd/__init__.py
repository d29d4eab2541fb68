"""humanoid_mujoco_amd — MI355X-native batched humanoid physics-step / rollout engine.

The package holds only what the hot path needs: ``csrc/`` (HIP kernels + the C-ABI of
``libhb.so``, declared in ``include/hb.h``) and the ctypes host binding in ``engine.py``
plus the VecEnv-shaped adapter in ``vecenv.py``.
"""
from .engine import (Batch, HbError, Model, lib, LIB_PATH, INT_EULER, INT_RK4, STATE_INTEGRATION, STATE_PHYSICS, STATE_QPOS, STATE_QVEL,  # noqa: F401
                     STATE_TIME, STATE_WARMSTART, STATE_XFRC_APPLIED, WARN_BADQACC, WARN_BADQPOS, WARN_BADQVEL,
                     WARN_CNSTRFULL, WARN_CONTACTFULL, quat_to_mat, height_scan_rays, RAY_STATIC, RAY_MOVING, HbJacSpec, MAX_JAC, JAC_POINT, JAC_SUBTREE_COM,
                     ACTOR_DETERMINISTIC, ACTOR_GAUSSIAN, ACTOR_SQUASHED, ACT_TANH, ACT_RELU, ACT_ELU, NET_POLICY, NET_ACTOR, NET_CRITIC, NET_Q1, NET_Q2, RS_ACTOR, HbActorConfig, HbCollectOut, HbGaeConfig, HbGaeOut, HbNormConfig, HbNormIo, HbNormTapes, HbSacConfig, HbSacRows, SAC_STATS, sac_flat_shapes, sac_split, sac_join)

from .vecenv import VecEnv  # noqa: E402,F401
from .replay import ReplayBuffer  # noqa: E402,F401

__all__ = ["Batch", "Model", "VecEnv", "ReplayBuffer", "HbError", "lib", "LIB_PATH", "quat_to_mat", "height_scan_rays"]

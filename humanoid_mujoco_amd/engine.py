"""ctypes host binding of libhb.so (include/hb.h) — the Python side of the drop-in boundary.

Mirrors how the reference's Python reaches its physics step: ``mujoco.MjModel.from_xml_path`` /
``mujoco.MjData`` / ``mujoco.mj_step`` in simulation/cpu_env.py:86,397,684 become
``Model.load`` / ``Batch`` / ``Batch.step``.  All compute happens in the HIP kernels behind the
C-ABI; this module only moves pointers.  There is no CPU fallback: creating a Batch without a
GPU raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (HB_LIB: another build of the same library, e.g. build/libhb_stamps.so with the per-stage cycle stamps; there is no other backend)
LIB_PATH = os.environ.get("HB_LIB") or os.path.join(_HERE, "libhb.so")

HB_OK = 0
WARN_CONTACTFULL, WARN_CNSTRFULL, WARN_BADQPOS, WARN_BADQVEL, WARN_BADQACC = 1 << 1, 1 << 2, 1 << 4, 1 << 5, 1 << 6
STATE_TIME, STATE_QPOS, STATE_QVEL, STATE_WARMSTART, STATE_XFRC_APPLIED = 1 << 0, 1 << 1, 1 << 2, 1 << 4, 1 << 7
STATE_PHYSICS = STATE_QPOS | STATE_QVEL
STATE_INTEGRATION = STATE_TIME | STATE_QPOS | STATE_QVEL | STATE_WARMSTART
HB_INV_DISCRETE = 1  # hb_inverse flags: mjENBL_INVDISCRETE
INT_EULER, INT_RK4 = 0, 1  # hb_options.integrator (mjtIntegrator): Model.set_opt(integrator=...)

# mjtDisableBit (simulation/mujoco/include/mujoco/mjmodel.h:50-68)
DSBL_CONSTRAINT, DSBL_LIMIT, DSBL_CONTACT, DSBL_PASSIVE, DSBL_GRAVITY = 1 << 0, 1 << 3, 1 << 4, 1 << 5, 1 << 6
DSBL_CLAMPCTRL, DSBL_WARMSTART, DSBL_FILTERPARENT, DSBL_ACTUATION, DSBL_REFSAFE, DSBL_EULERDAMP = 1 << 7, 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 14
DSBL_EQUALITY, DSBL_FRICTIONLOSS = 1 << 1, 1 << 2
EQ_CONNECT, EQ_JOINT = 0, 2  # mjtEq values of Model.array("eq_type")


class HbOptions(ctypes.Structure):
    _fields_ = [("timestep", ctypes.c_double), ("gravity", ctypes.c_double * 3), ("impratio", ctypes.c_double),
                ("tolerance", ctypes.c_double), ("iterations", ctypes.c_int), ("solver", ctypes.c_int),
                ("cone", ctypes.c_int), ("integrator", ctypes.c_int), ("disableflags", ctypes.c_int),
                ("ls_iterations", ctypes.c_int), ("ls_tolerance", ctypes.c_double)]


class HbSizes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "ntendon", "nM", "nkey",
                                            "npair", "nobs", "ncon_max", "nefc_max")]


class HbObsExt(ctypes.Structure):
    """hb_obs_ext (include/hb.h): what the env adapter appends to the model's observation."""
    _fields_ = [("prev_action", ctypes.c_int), ("height_scan", ctypes.c_int), ("scan_offset", ctypes.c_float), ("scan_scale", ctypes.c_float),
                ("scan_lo", ctypes.c_float), ("scan_hi", ctypes.c_float)]


class HbEnvRow(ctypes.Structure):
    """struct hb_env_row (include/hb.h): offset and count of every part of an observation row of the env adapter, and its width."""
    _fields_ = [(n, ctypes.c_int) for n in ("base", "prev_action", "n_prev_action", "scan", "n_scan", "foot_contact", "n_foot_contact", "command", "n_command", "width")]


class HbEnvCommands(ctypes.Structure):
    """hb_env_commands (include/hb.h): per-env velocity commands - ranges, schedule, reward weight, frame, observation."""
    _fields_ = [("seed", ctypes.c_uint)] + [(n, ctypes.c_float) for n in ("vx_min", "vx_max", "vy_min", "vy_max", "yaw_min", "yaw_max", "resample_time",
                                                                           "zero_fraction", "w_yaw")] + [("frame", ctypes.c_int), ("observe", ctypes.c_int)]


class HbEnvFeet(ctypes.Structure):
    """hb_env_feet (include/hb.h): foot-contact terms of the env adapter - the bodies, the contact threshold, the weights, observation."""
    _fields_ = [("n_feet", ctypes.c_int), ("foot_body", ctypes.c_int * 4), ("n_penalised", ctypes.c_int), ("penalised_body", ctypes.c_int * 8),
                ("n_terminal", ctypes.c_int), ("terminal_body", ctypes.c_int * 8), ("contact_threshold", ctypes.c_float),
                ("w_air_time", ctypes.c_float), ("air_time_target", ctypes.c_float), ("air_gate", ctypes.c_int), ("air_cmd_min", ctypes.c_float),
                ("w_force", ctypes.c_float), ("force_max", ctypes.c_float), ("w_stumble", ctypes.c_float), ("stumble_ratio", ctypes.c_float),
                ("w_collision", ctypes.c_float), ("observe", ctypes.c_int)]

    def set_bodies(self, bodies=None, penalised=None, terminal=None):
        """fills the three body lists (ids; None leaves a list as it is) and their counts"""
        for ids, count, field, cap in ((bodies, "n_feet", "foot_body", 4), (penalised, "n_penalised", "penalised_body", 8), (terminal, "n_terminal", "terminal_body", 8)):
            if ids is None:
                continue
            ids = [int(i) for i in ids]
            if len(ids) > cap:
                raise ValueError("feet: %s holds at most %d bodies" % (field, cap))
            setattr(self, count, len(ids))
            arr = getattr(self, field)
            for i in range(cap):
                arr[i] = ids[i] if i < len(ids) else 0
        return self


class HbRaySpec(ctypes.Structure):
    """hb_ray_spec (include/hb.h): frame, eligible geoms and cutoff of the installed rays."""
    _fields_ = [("frame", ctypes.c_int), ("frame_body", ctypes.c_int), ("bodyexclude", ctypes.c_int), ("flags", ctypes.c_int), ("cutoff", ctypes.c_float)]


class HbJacSpec(ctypes.Structure):
    """hb_jac_spec (include/hb.h): the points whose Jacobians hb_dynamics* returns."""
    _fields_ = [("n", ctypes.c_int), ("kind", ctypes.c_int * 16), ("body", ctypes.c_int * 16), ("offset", (ctypes.c_float * 3) * 16)]


MAX_JAC, JAC_POINT, JAC_SUBTREE_COM = 16, 0, 1
RAY_STATIC, RAY_MOVING = 1, 2
RAY_FRAMES = {"world": 0, "body": 1, "yaw": 2}
RAY_SURFACES = (0, 1, 2, 3, 6)  # geom types a ray intersects: plane, height field, sphere, capsule, box


def height_scan_rays(xs, ys, z0=1.0):
    """The downward grid of a terrain height scan: (pnt, vec) float32 [len(ys) * len(xs), 3], row-major over (y, x), pnt = (x, y, z0) and
    vec = (0, 0, -1) - for Batch.ray_configure(..., frame="yaw")."""
    xs, ys = np.asarray(xs, dtype=np.float32).reshape(-1), np.asarray(ys, dtype=np.float32).reshape(-1)
    pnt = np.empty((len(ys), len(xs), 3), dtype=np.float32)
    pnt[..., 0] = xs[None, :]; pnt[..., 1] = ys[:, None]; pnt[..., 2] = z0
    vec = np.zeros_like(pnt)
    vec[..., 2] = -1.0
    return pnt.reshape(-1, 3), vec.reshape(-1, 3)


class HbEnvConfig(ctypes.Structure):
    """hb_env_config (include/hb.h): reward / termination parameters of the env adapter."""
    _fields_ = [("target_velocity", ctypes.c_float * 2), ("target_z", ctypes.c_float), ("min_z", ctypes.c_float),
                ("max_time", ctypes.c_float), ("safe_torque", ctypes.c_float), ("control_frequency", ctypes.c_float),
                ("action_scale", ctypes.c_float), ("w_hvel", ctypes.c_float), ("w_upright", ctypes.c_float),
                ("w_height", ctypes.c_float), ("w_torque", ctypes.c_float), ("w_ctrl_change", ctypes.c_float),
                ("w_ctrl_reg", ctypes.c_float), ("w_symmetry", ctypes.c_float), ("self_collision_penalty", ctypes.c_float),
                ("terminal_reward", ctypes.c_float), ("upright_tol", ctypes.c_float), ("n_equal", ctypes.c_int),
                ("n_opposite", ctypes.c_int), ("equal_pairs", (ctypes.c_int * 2) * 16), ("opposite_pairs", (ctypes.c_int * 2) * 16),
                ("auto_reset", ctypes.c_int), ("reset_keyframe", ctypes.c_int), ("reset_perturb", ctypes.c_float),
                ("reward_kind", ctypes.c_int), ("w_vvel", ctypes.c_float), ("min_z_grounded", ctypes.c_float),
                ("reset_collision_mode", ctypes.c_int), ("reset_quat_perturb", ctypes.c_float), ("obs_actuator_order", ctypes.c_int)]


class HbEnvRandomization(ctypes.Structure):
    """hb_env_randomization (include/hb.h): sensor/action noise, delay FIFOs and pushes of CPUEnv, per env on the device."""
    _fields_ = [("factor", ctypes.c_float), ("seed", ctypes.c_uint), ("control_timestep", ctypes.c_float),
                ("joint_angle_noise", ctypes.c_float), ("joint_velocity_noise", ctypes.c_float), ("gyro_noise", ctypes.c_float),
                ("imu_noise", ctypes.c_float), ("action_noise", ctypes.c_float), ("min_delay", ctypes.c_float),
                ("max_delay", ctypes.c_float), ("frozen_noise", ctypes.c_int), ("push_enabled", ctypes.c_int),
                ("push_min_interval", ctypes.c_float), ("push_max_interval", ctypes.c_float), ("push_min_duration", ctypes.c_float),
                ("push_max_duration", ctypes.c_float), ("push_min_force", ctypes.c_float), ("push_max_force", ctypes.c_float)]


class HbTaskStand(ctypes.Structure):
    _fields_ = [("head_body", ctypes.c_int), ("n_feet", ctypes.c_int), ("foot_body", ctypes.c_int * 4), ("foot_offset", (ctypes.c_float * 3) * 4),
                ("subtree_body", ctypes.c_int), ("height_goal", ctypes.c_float), ("norm", ctypes.c_int * 5), ("weight", ctypes.c_float * 5),
                ("norm_p", (ctypes.c_float * 2) * 5), ("risk", ctypes.c_float)]


class HbTaskWalk(ctypes.Structure):
    _fields_ = [("torso_body", ctypes.c_int), ("pelvis_body", ctypes.c_int), ("foot_right_body", ctypes.c_int), ("foot_left_body", ctypes.c_int),
                ("waist_lower_body", ctypes.c_int), ("height_goal", ctypes.c_float), ("speed_goal", ctypes.c_float), ("n_term", ctypes.c_int),
                ("dim", ctypes.c_int * 8), ("norm", ctypes.c_int * 8), ("weight", ctypes.c_float * 8), ("norm_p", (ctypes.c_float * 2) * 8),
                ("risk", ctypes.c_float)]


class HbCostSpec(ctypes.Structure):
    """hb_cost_spec (include/hb.h): cost terms over consecutive slices of a residual vector (mjpc task.cc:71-110)."""
    _fields_ = [("n_term", ctypes.c_int), ("dim", ctypes.c_int * 8), ("norm", ctypes.c_int * 8), ("weight", ctypes.c_float * 8),
                ("norm_p", (ctypes.c_float * 2) * 8), ("risk", ctypes.c_float)]


class HbSensorSpec(ctypes.Structure):
    """hb_sensor_spec (include/hb.h): the entries of every part of a sensor row - framepos, one tree's subtreecom / subtreelinvel, frame axes,
    framelinvel, subtreelinvel, touch, contact force, accelerometer / gyro, frame acceleration (Batch.sensor_spec fills it)."""
    _fields_ = [("n_framepos", ctypes.c_int), ("framepos_body", ctypes.c_int * 16), ("subtree_body", ctypes.c_int),
                ("framepos_offset", (ctypes.c_float * 3) * 16),
                ("n_frameaxis", ctypes.c_int), ("frameaxis_body", ctypes.c_int * 8), ("frameaxis_which", ctypes.c_int * 8),
                ("n_framelinvel", ctypes.c_int), ("framelinvel_body", ctypes.c_int * 8),
                ("n_subtreelinvel", ctypes.c_int), ("subtreelinvel_body", ctypes.c_int * 4),
                ("n_touch", ctypes.c_int), ("touch_body", ctypes.c_int * 8),
                ("n_contactforce", ctypes.c_int), ("contactforce_body", ctypes.c_int * 4),
                ("n_imu", ctypes.c_int), ("imu_body", ctypes.c_int * 4), ("imu_offset", (ctypes.c_float * 3) * 4),
                ("n_frameacc", ctypes.c_int), ("frameacc_body", ctypes.c_int * 4)]


SENSOR_PARTS = ("framepos", "subtree", "axis", "linvel", "sub", "touch", "cfrc", "imu", "facc")  # the parts of a sensor row, in its order


class HbSensorRow(ctypes.Structure):
    """struct hb_sensor_row (include/hb.h): offset (floats) and count (entries) of every part of a sensor row, and its width."""
    _fields_ = [(f, ctypes.c_int) for n in SENSOR_PARTS for f in (n, "n_" + n)] + [("width", ctypes.c_int)]


class HbDomainRandomization(ctypes.Structure):
    """hb_domain_randomization (include/hb.h): per-env model parameters drawn at reset."""
    _fields_ = [("factor", ctypes.c_float), ("seed", ctypes.c_uint), ("friction_min_mult", ctypes.c_float), ("friction_max_mult", ctypes.c_float),
                ("max_mass_change", ctypes.c_float), ("max_external_mass", ctypes.c_float), ("armature_max_change", ctypes.c_float),
                ("stiffness_max_change", ctypes.c_float), ("margin_max_change", ctypes.c_float), ("range_max_change", ctypes.c_float),
                ("kp_nominal", ctypes.c_float), ("kp_max_change", ctypes.c_float), ("force_limit_max_change", ctypes.c_float),
                ("floor_bump_min", ctypes.c_float), ("floor_bump_max", ctypes.c_float)]


ACTOR_DETERMINISTIC, ACTOR_GAUSSIAN, ACTOR_SQUASHED = 0, 1, 2  # hb_actor_config.head (HB_ACTOR_*)
ACTOR_HEADS = {"deterministic": ACTOR_DETERMINISTIC, "gaussian": ACTOR_GAUSSIAN, "squashed": ACTOR_SQUASHED}
ACT_TANH, ACT_RELU, ACT_ELU = 0, 1, 2  # the hidden activation of an installed MLP (HB_ACT_*)
ACTIVATIONS = {"tanh": ACT_TANH, "relu": ACT_RELU, "elu": ACT_ELU}
NET_POLICY, NET_ACTOR, NET_CRITIC, NET_Q1, NET_Q2 = 0, 1, 2, 3, 4  # which installed MLP (HB_NET_*)
NETS = {"policy": NET_POLICY, "actor": NET_ACTOR, "critic": NET_CRITIC, "q1": NET_Q1, "q2": NET_Q2}
RS_ACTOR = 32  # random-number stream of the actor's draws (include/hb.h: hb_env_collect_dev)


class HbActorConfig(ctypes.Structure):
    """hb_actor_config (include/hb.h): the sampling head of the actor."""
    _fields_ = [("head", ctypes.c_int), ("seed", ctypes.c_uint), ("log_std", ctypes.c_float * 32), ("deterministic", ctypes.c_int)]


class HbCollectOut(ctypes.Structure):
    """hb_collect_out (include/hb.h): device pointers of the tapes hb_env_collect_dev reads (obs row 0) and writes."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("obs", "action", "mean", "log_std", "eps", "reward", "terminated", "truncated", "terminal_obs")]


class HbGaeConfig(ctypes.Structure):
    """hb_gae_config (include/hb.h): discount, GAE lambda, and whether envs cut by truncation alone are bootstrapped."""
    _fields_ = [("gamma", ctypes.c_float), ("lam", ctypes.c_float), ("bootstrap_truncated", ctypes.c_int)]


class HbGaeOut(ctypes.Structure):
    """hb_gae_out (include/hb.h): device pointers of what hb_collect_gae_dev writes, each nullable."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("value", "terminal_value", "log_prob", "advantage", "returns")]


class HbNormConfig(ctypes.Structure):
    """hb_norm_config (include/hb.h): VecNormalize's switches and constants."""
    _fields_ = [("norm_obs", ctypes.c_int), ("norm_reward", ctypes.c_int), ("training", ctypes.c_int), ("clip_obs", ctypes.c_float),
                ("clip_reward", ctypes.c_float), ("gamma", ctypes.c_float), ("epsilon", ctypes.c_float)]


class HbNormIo(ctypes.Structure):
    """hb_norm_io (include/hb.h): device pointers of one normaliser step."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("obs_in", "obs_out", "reward_in", "reward_out", "terminated", "truncated", "terminal_obs_in",
                                               "terminal_obs_out", "ep_return_out", "ep_length_out")]


class HbNormTapes(ctypes.Structure):
    """hb_norm_tapes (include/hb.h): the normaliser's own tapes of a collection, each nullable."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("raw_obs", "raw_reward", "ep_return", "ep_length")]


class HbPpoConfig(ctypes.Structure):
    """hb_ppo_config (include/hb.h): the hyper-parameters of the PPO learner, stable-baselines3's defaults."""
    _fields_ = [("clip_range", ctypes.c_float), ("ent_coef", ctypes.c_float), ("vf_coef", ctypes.c_float), ("max_grad_norm", ctypes.c_float),
                ("normalize_advantage", ctypes.c_int), ("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("eps", ctypes.c_float)]


class HbPpoRows(ctypes.Structure):
    """hb_ppo_rows (include/hb.h): device pointers of the flattened tapes, and the minibatch (index, or first .. first + mb - 1)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("obs", "action", "old_log_prob", "advantage", "returns", "index")] + \
               [("n_rows", ctypes.c_longlong), ("first", ctypes.c_longlong), ("mb", ctypes.c_int)]


# the statistics hb_ppo_grad_dev / hb_ppo_adam_dev leave in their float[16] (include/hb.h), in order
PPO_STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm", "adv_mean", "adv_std", "ratio_max",
             "skipped")


def _flat_shapes(nets, tail):
    """(name, shape) of a flat record's tensors in order: for every (tag, sizes) of nets the layers W [K, N] | b [N], and behind the
    network it names the one tensor of tail = (tag, name, shape)."""
    out = []
    for tag, sizes in nets:
        for l in range(len(sizes) - 1):
            out += [("%s.w%d" % (tag, l), (int(sizes[l]), int(sizes[l + 1]))), ("%s.b%d" % (tag, l), (int(sizes[l + 1]),))]
        if tag == tail[0]:
            out.append(tail[1:])
    return out


def _split(what, flat, shapes):
    flat = np.asarray(flat)
    total = sum(int(np.prod(sh)) for _, sh in shapes)
    if flat.shape != (total,):
        raise ValueError("%s: the record of these networks holds %d values" % (what, total))
    out, o = {}, 0
    for name, sh in shapes:
        n = int(np.prod(sh))
        out[name] = flat[o:o + n].reshape(sh).copy()
        o += n
    return out


def _join(what, tensors, shapes, dtype):
    parts = []
    for name, sh in shapes:
        a = np.asarray(tensors[name], dtype=dtype)
        if a.shape != sh:
            raise ValueError("%s: %s must be %s" % (what, name, sh))
        parts.append(a.ravel())
    return np.concatenate(parts)


def ppo_flat_shapes(actor_sizes, critic_sizes, nu):
    """The tensors of the learner's flat record in order, as (name, shape): the actor's layers W [K, N] | b [N], log_std [nu], the critic's
    layers (include/hb.h: hb_learner_get_params)."""
    return _flat_shapes((("actor", actor_sizes), ("critic", critic_sizes)), ("actor", "log_std", (int(nu),)))


def ppo_split(flat, actor_sizes, critic_sizes, nu):
    """The flat record as a dict of per-tensor arrays (copies): actor.w0, actor.b0, ..., log_std, critic.w0, ..."""
    return _split("ppo_split", flat, ppo_flat_shapes(actor_sizes, critic_sizes, nu))


def ppo_join(tensors, actor_sizes, critic_sizes, nu, dtype=np.float32):
    """The inverse of ppo_split."""
    return _join("ppo_join", tensors, ppo_flat_shapes(actor_sizes, critic_sizes, nu), dtype)


def ppo_row_chunk(mb):
    """Rows per chunk of the learner's row reductions for a minibatch of mb rows (hb_ppo_row_chunk)."""
    return int(lib().hb_ppo_row_chunk(int(mb)))


class HbSacConfig(ctypes.Structure):
    """hb_sac_config (include/hb.h): the hyper-parameters of the SAC learner, stable-baselines3's defaults."""
    _fields_ = [(n, ctypes.c_float) for n in ("gamma", "tau", "lr_actor", "lr_critic", "lr_ent", "beta1", "beta2", "eps", "ent_coef_init")] + \
               [("auto_ent", ctypes.c_int), ("target_entropy_auto", ctypes.c_int), ("target_entropy", ctypes.c_float),
                ("target_update_interval", ctypes.c_int), ("seed", ctypes.c_uint)]


class HbSacRows(ctypes.Structure):
    """hb_sac_rows (include/hb.h): device pointers of the replay rows, the minibatch (index, or first .. first + mb - 1) and the draws."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("obs", "action", "reward", "next_obs", "done", "index")] + \
               [("n_rows", ctypes.c_longlong), ("first", ctypes.c_longlong), ("mb", ctypes.c_int), ("eps_pi", ctypes.c_void_p),
                ("eps_next", ctypes.c_void_p), ("eps_given", ctypes.c_int)]


# the statistics hb_sac_step_dev leaves in its float[16] (include/hb.h), in order
SAC_STATS = ("actor_loss", "critic_loss", "ent_coef_loss", "ent_coef", "lp_pi", "q1", "q2", "y", "min_q_pi")


def sac_flat_shapes(actor_sizes, q_sizes):
    """The tensors of the SAC learner's flat record in order, as (name, shape): the actor's layers W [K, N] | b [N], Q1's, Q2's,
    log_ent_coef [1] (include/hb.h: hb_sac_get_params).  The targets' record mirrors the q1.*, q2.* stretch."""
    return _flat_shapes((("actor", actor_sizes), ("q1", q_sizes), ("q2", q_sizes)), ("q2", "log_ent_coef", (1,)))


def sac_split(flat, actor_sizes, q_sizes):
    """The flat record as a dict of per-tensor arrays (copies): actor.w0, actor.b0, ..., q1.w0, ..., q2.w0, ..., log_ent_coef."""
    return _split("sac_split", flat, sac_flat_shapes(actor_sizes, q_sizes))


def sac_join(tensors, actor_sizes, q_sizes, dtype=np.float32):
    """The inverse of sac_split."""
    return _join("sac_join", tensors, sac_flat_shapes(actor_sizes, q_sizes), dtype)


class HbError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libhb.so; fails loudly when the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HbError("libhb.so is missing (%s): build it with `make` or __graft_entry__.build(); "
                      "this package has no fallback path" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, cp, ci, cu = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    L.hb_version.restype = cp
    L.hb_model_load.restype = vp; L.hb_model_load.argtypes = [cp, cp, ci]
    L.hb_model_load_xml_string.restype = vp; L.hb_model_load_xml_string.argtypes = [cp, cp, ci]
    L.hb_model_save.argtypes = [vp, cp, cp, ci]
    L.hb_model_free.argtypes = [vp]; L.hb_model_free.restype = None
    L.hb_model_sizes.argtypes = [vp, ctypes.POINTER(HbSizes)]
    L.hb_options_get.argtypes = [vp, ctypes.POINTER(HbOptions)]
    L.hb_options_set.argtypes = [vp, ctypes.POINTER(HbOptions)]
    L.hb_model_name2id.argtypes = [vp, cp, cp]
    L.hb_model_id2name.argtypes = [vp, cp, ctypes.c_int, cp, ctypes.c_int]
    L.hb_model_get_array.argtypes = [vp, cp, vp, ci]
    L.hb_batch_create.restype = vp; L.hb_batch_create.argtypes = [vp, ci, ci, cp, ci]
    L.hb_batch_free.argtypes = [vp]; L.hb_batch_free.restype = None
    L.hb_batch_n_env.argtypes = [vp]
    L.hb_batch_stream.restype = vp; L.hb_batch_stream.argtypes = [vp]
    L.hb_batch_sync.argtypes = [vp]
    L.hb_batch_pipeline.argtypes = [vp, ci]
    L.hb_batch_join.argtypes = [vp]
    L.hb_reset.argtypes = [vp, vp, ci, ci, ci]
    L.hb_step.argtypes = [vp, vp, ci]
    L.hb_step_dev.argtypes = [vp, vp, ci]
    L.hb_rollout.argtypes = [vp, vp, ci, vp]
    L.hb_rollout_dev.argtypes = [vp, vp, ci, vp]
    L.hb_rollout_halton.argtypes = [vp, ci, ci, ci, vp]
    L.hb_forward.argtypes = [vp, vp]
    L.hb_inverse.argtypes = [vp, vp, ci, vp, vp]
    L.hb_inverse_dev.argtypes = [vp, vp, ci, vp, vp]
    L.hb_kinematics.argtypes = [vp, vp, vp, vp]; L.hb_kinematics_dev.argtypes = [vp, vp, vp, vp]
    L.hb_kinematics_states.argtypes = [vp, vp, vp, ci, vp, vp, vp]; L.hb_kinematics_states_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp]
    jp = ctypes.POINTER(HbJacSpec)
    L.hb_dynamics.argtypes = [vp, vp, vp, vp, jp, vp]; L.hb_dynamics_dev.argtypes = [vp, vp, vp, vp, jp, vp]
    L.hb_dynamics_states.argtypes = [vp, vp, vp, ci, vp, vp, vp, jp, vp]; L.hb_dynamics_states_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp, jp, vp]
    L.hb_ray_configure.argtypes = [vp, ctypes.POINTER(HbRaySpec), vp, vp, ci]
    L.hb_rays.argtypes = [vp, vp, vp]; L.hb_rays_dev.argtypes = [vp, vp, vp]
    L.hb_state_size.argtypes = [vp, cu]
    L.hb_get_state.argtypes = [vp, cu, vp]; L.hb_set_state.argtypes = [vp, cu, vp]
    L.hb_get_state_f64.argtypes = [vp, cu, vp]; L.hb_set_state_f64.argtypes = [vp, cu, vp]
    L.hb_get_obs.argtypes = [vp, vp, vp, vp, vp]
    L.hb_get_status.argtypes = [vp, vp]
    L.hb_get_counts.argtypes = [vp, vp, vp, vp]
    L.hb_last_kernel.argtypes = [vp]; L.hb_last_kernel.restype = ctypes.c_char_p
    L.hb_batch_step_launches.argtypes = [vp]; L.hb_batch_step_launches.restype = ctypes.c_longlong
    L.hb_batch_tune.argtypes = [vp, ci, ci]
    L.hb_model_pair_order.argtypes = [vp, ci]
    L.hb_model_box_manifold.argtypes = [vp, ci]
    L.hb_env_terminal_obs.argtypes = [vp, vp]
    L.hb_env_warnings.argtypes = [vp, vp]
    L.hb_env_joint_torques.argtypes = [vp, vp]
    L.hb_batch_device_name.argtypes = [vp, cp, ci]
    L.hb_get_collision_counts.argtypes = [vp, vp, vp, vp]
    L.hb_batch_segments.argtypes = [vp]
    L.hb_diag_enable.argtypes = [vp, ci]
    L.hb_get_qacc.argtypes = [vp, vp]; L.hb_get_efc_force.argtypes = [vp, vp]; L.hb_get_contacts.argtypes = [vp, vp]
    L.hb_contact_readout.argtypes = [vp, ci]
    L.hb_get_contact_force.argtypes = [vp, vp]; L.hb_get_body_contact.argtypes = [vp, vp]
    L.hb_contact_readout_dev.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.hb_body_acc_readout.argtypes = [vp, ci]
    L.hb_get_body_acc.argtypes = [vp, vp]
    L.hb_body_acc_readout_dev.argtypes = [vp, ctypes.POINTER(vp)]
    L.hb_env_default_config.argtypes = [vp, ctypes.POINTER(HbEnvConfig)]
    L.hb_env_team_config.argtypes = [vp, ctypes.POINTER(HbEnvConfig)]
    L.hb_env_configure.argtypes = [vp, ctypes.POINTER(HbEnvConfig)]
    L.hb_env_default_randomization.argtypes = [vp, ctypes.POINTER(HbEnvRandomization)]
    L.hb_env_randomize.argtypes = [vp, ctypes.POINTER(HbEnvRandomization)]
    L.hb_env_default_domain_randomization.argtypes = [vp, ctypes.POINTER(HbDomainRandomization)]
    L.hb_env_domain_randomize.argtypes = [vp, ctypes.POINTER(HbDomainRandomization)]
    L.hb_env_get_domain_params.argtypes = [vp, vp]
    L.hb_state_to_proto.argtypes = [vp, ci, vp, ci]
    L.hb_state_from_proto.argtypes = [vp, ci, cp, ci]
    L.hb_sensor_size.argtypes = [ctypes.POINTER(HbSensorSpec)]
    L.hb_sensor_row.argtypes = [ctypes.POINTER(HbSensorSpec), ctypes.POINTER(HbSensorRow)]
    L.hb_set_state_broadcast.argtypes = [vp, cu, vp]
    L.hb_set_state_broadcast_f64.argtypes = [vp, cu, vp]
    L.hb_rollout_sensors.argtypes = [vp, vp, ci, ctypes.POINTER(HbSensorSpec), vp, vp]
    L.hb_rollout_trajectory.argtypes = [vp, vp, ci, vp, vp, vp]
    L.hb_rollout_noise.argtypes = [vp, ctypes.c_float, ctypes.c_float, ctypes.c_uint]
    L.hb_ctrl_tape_splines.argtypes = [vp, vp, vp, ci, ci, ctypes.c_double, ci]
    L.hb_ctrl_tape_read.argtypes = [vp, ci, vp]
    L.hb_task_cost.argtypes = [vp, vp, ci, ci, ctypes.POINTER(HbCostSpec), vp, vp]
    L.hb_transition_fd.argtypes = [vp, vp, vp, vp, ci, ctypes.c_double, ci, vp, vp]
    L.hb_transition_fd_sensors.argtypes = [vp, vp, vp, vp, ci, ctypes.c_double, ci, ctypes.POINTER(HbSensorSpec), vp, vp, vp, vp]
    L.hb_task_stand_default.argtypes = [vp, ctypes.POINTER(HbTaskStand)]
    L.hb_rollout_task_stand.argtypes = [vp, vp, ci, ctypes.POINTER(HbTaskStand), vp, vp]
    L.hb_task_walk_default.argtypes = [vp, ctypes.POINTER(HbTaskWalk)]
    L.hb_rollout_task_walk.argtypes = [vp, vp, ci, ctypes.POINTER(HbTaskWalk), vp, vp]
    L.hb_sensors.argtypes = [vp, vp, ctypes.POINTER(HbSensorSpec), vp]
    L.hb_env_reset.argtypes = [vp, vp]
    L.hb_env_step.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    L.hb_env_step_async.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    L.hb_env_step_dev.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    L.hb_env_obs_extend.argtypes = [vp, ctypes.POINTER(HbObsExt)]
    L.hb_env_nobs.argtypes = [vp]
    L.hb_env_row.argtypes = [vp, ctypes.POINTER(HbEnvRow)]
    L.hb_env_default_commands.argtypes = [vp, ctypes.POINTER(HbEnvCommands)]
    L.hb_env_commands_check.argtypes = [vp, ctypes.POINTER(HbEnvCommands)]
    L.hb_env_commands_configure.argtypes = [vp, ctypes.POINTER(HbEnvCommands)]
    L.hb_env_get_commands.argtypes = [vp, vp]
    L.hb_env_set_commands.argtypes = [vp, vp, vp]
    L.hb_env_default_feet.argtypes = [vp, ctypes.POINTER(HbEnvFeet)]
    L.hb_env_feet_check.argtypes = [vp, ctypes.POINTER(HbEnvFeet)]
    L.hb_env_feet_configure.argtypes = [vp, ctypes.POINTER(HbEnvFeet)]
    L.hb_env_get_feet.argtypes = [vp, vp, vp]
    L.hb_env_feet_count.argtypes = [vp]
    L.hb_error.argtypes = []
    L.hb_error.restype = ctypes.c_char_p
    L.hb_policy_set_mlp.argtypes = [vp, ci, vp, vp, vp]
    L.hb_policy_eval.argtypes = [vp, vp]
    L.hb_rollout_policy.argtypes = [vp, ci, vp]
    L.hb_actor_set_mlp.argtypes = [vp, ci, vp, vp, vp, ctypes.POINTER(HbActorConfig)]
    L.hb_env_collect_dev.argtypes = [vp, ci, ci, ctypes.POINTER(HbCollectOut)]
    L.hb_critic_set_mlp.argtypes = [vp, ci, vp, vp, vp]
    L.hb_collect_gae_dev.argtypes = [vp, ci, ctypes.POINTER(HbCollectOut), ctypes.POINTER(HbGaeConfig), ctypes.POINTER(HbGaeOut)]
    L.hb_norm_default_config.argtypes = [ctypes.POINTER(HbNormConfig)]
    L.hb_norm_configure.argtypes = [vp, ctypes.POINTER(HbNormConfig)]
    L.hb_norm_get_stats.argtypes = [vp, vp]
    L.hb_norm_set_stats.argtypes = [vp, vp]
    L.hb_norm_get_env.argtypes = [vp, vp, vp, vp]
    L.hb_norm_episode_totals.argtypes = [vp, vp]
    L.hb_norm_step_dev.argtypes = [vp, ctypes.POINTER(HbNormIo)]
    L.hb_norm_reset_dev.argtypes = [vp, vp, vp]
    L.hb_norm_obs_dev.argtypes = [vp, vp, vp, ctypes.c_longlong]
    L.hb_env_collect_norm_dev.argtypes = [vp, ci, ci, ctypes.POINTER(HbCollectOut), ctypes.POINTER(HbNormTapes)]
    L.hb_ppo_default_config.argtypes = [ctypes.POINTER(HbPpoConfig)]
    L.hb_ppo_row_chunk.argtypes = [ci]
    L.hb_learner_create.argtypes = [vp, ctypes.POINTER(HbPpoConfig)]
    L.hb_learner_configure.argtypes = [vp, ctypes.POINTER(HbPpoConfig)]
    L.hb_learner_destroy.argtypes = [vp]
    L.hb_learner_param_count.argtypes = [vp]; L.hb_learner_param_count.restype = ctypes.c_longlong
    L.hb_learner_get_params.argtypes = [vp, vp, ctypes.c_longlong]; L.hb_learner_set_params.argtypes = [vp, vp, ctypes.c_longlong]
    L.hb_learner_get_grads.argtypes = [vp, vp, ctypes.c_longlong]
    L.hb_learner_get_state.argtypes = [vp, vp, vp, vp, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    L.hb_learner_set_state.argtypes = [vp, vp, vp, vp, ctypes.c_longlong, ctypes.c_longlong]
    L.hb_learner_grad_dev.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_longlong)]
    L.hb_ppo_grad_dev.argtypes = [vp, ctypes.POINTER(HbPpoRows), vp]
    L.hb_ppo_adam_dev.argtypes = [vp, vp]
    L.hb_ppo_minibatch_dev.argtypes = [vp, ctypes.POINTER(HbPpoRows), vp]
    ll = ctypes.c_longlong
    L.hb_q_set_mlp.argtypes = [vp, ci, ci, vp, vp, vp]
    L.hb_q_values_dev.argtypes = [vp, vp, vp, ll, vp, vp]
    L.hb_mlp_set_activation.argtypes = [vp, ci, ci]
    L.hb_mlp_get_activation.argtypes = [vp, ci]
    L.hb_sac_default_config.argtypes = [ctypes.POINTER(HbSacConfig)]
    L.hb_sac_create.argtypes = [vp, ctypes.POINTER(HbSacConfig)]
    L.hb_sac_configure.argtypes = [vp, ctypes.POINTER(HbSacConfig)]
    L.hb_sac_destroy.argtypes = [vp]
    L.hb_sac_param_count.argtypes = [vp]; L.hb_sac_param_count.restype = ll
    L.hb_sac_target_count.argtypes = [vp]; L.hb_sac_target_count.restype = ll
    L.hb_sac_get_params.argtypes = [vp, vp, ll]; L.hb_sac_set_params.argtypes = [vp, vp, ll]; L.hb_sac_get_grads.argtypes = [vp, vp, ll]
    L.hb_sac_get_state.argtypes = [vp, vp, vp, vp, ll, vp, ll, ctypes.POINTER(ll)]
    L.hb_sac_set_state.argtypes = [vp, vp, vp, vp, ll, vp, ll, ll]
    L.hb_sac_step_dev.argtypes = [vp, ctypes.POINTER(HbSacRows), vp]
    L.hb_dev_alloc.restype = vp; L.hb_dev_alloc.argtypes = [vp, ctypes.c_uint64]
    L.hb_dev_free.restype = None; L.hb_dev_free.argtypes = [vp, vp]
    L.hb_host_alloc.restype = vp; L.hb_host_alloc.argtypes = [ctypes.c_uint64]
    L.hb_host_free.restype = None; L.hb_host_free.argtypes = [vp]
    L.hb_memcpy_h2d.argtypes = [vp, vp, vp, ctypes.c_uint64]; L.hb_memcpy_d2h.argtypes = [vp, vp, vp, ctypes.c_uint64]
    L.hb_halton_ctrl_dev.argtypes = [vp, ci, ci, ci, vp]
    L.hb_timer_start.argtypes = [vp]; L.hb_timer_stop.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.hb_step_timing.argtypes = [vp, ci]; L.hb_step_timing_read.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ci)]
    _lib = L
    return L


def quat_to_mat(q):
    """rotation matrices [..., 3, 3] of unit quaternions [..., 4] (w x y z): xmat / geom_xmat of the quaternions Batch.kinematics returns
    (mju_quat2Mat)"""
    q = np.asarray(q)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    m = np.empty(q.shape[:-1] + (3, 3), dtype=q.dtype)
    m[..., 0, 0] = w * w + x * x - y * y - z * z; m[..., 0, 1] = 2 * (x * y - w * z); m[..., 0, 2] = 2 * (x * z + w * y)
    m[..., 1, 0] = 2 * (x * y + w * z); m[..., 1, 1] = w * w - x * x + y * y - z * z; m[..., 1, 2] = 2 * (y * z - w * x)
    m[..., 2, 0] = 2 * (x * z - w * y); m[..., 2, 1] = 2 * (y * z + w * x); m[..., 2, 2] = w * w - x * x - y * y + z * z
    return m


def _activation(a):
    if isinstance(a, str):
        if a not in ACTIVATIONS:
            raise ValueError("activation must be one of %s, not %r" % (sorted(ACTIVATIONS), a))
        return ACTIVATIONS[a]
    return int(a)


def _net(n):
    if isinstance(n, str):
        if n not in NETS:
            raise ValueError("net must be one of %s, not %r" % (sorted(NETS), n))
        return NETS[n]
    return int(n)


def _check(rc, what, why=None):
    if rc != HB_OK:
        raise HbError("%s failed with code %d%s" % (what, rc, ": " + why if why else ""))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _mlp_args(what, weights, biases, sizes=None):
    """The arguments of hb_policy_set_mlp / hb_actor_set_mlp / hb_critic_set_mlp: (ws, bs, csizes, wp, bp) - the contiguous float32 arrays
    (keep them alive across the call) and the ctypes arrays of the widths and of the weight and bias pointers.  sizes None: the widths
    are the first weight's rows and every weight's columns.  Every layer's shape is checked, so the library never reads past an array."""
    ws = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
    bs = [np.ascontiguousarray(x, dtype=np.float32) for x in biases]
    if sizes is None:  # (a weight that is no matrix leaves the list short, and fails the check below)
        sizes = [w.shape[0] for w in ws[:1] if w.ndim == 2] + [w.shape[1] for w in ws if w.ndim == 2]
    sizes = [int(s) for s in sizes]
    if len(ws) != len(sizes) - 1 or len(bs) != len(ws) or any(w.shape != (a, c) for w, a, c in zip(ws, sizes[:-1], sizes[1:])) or \
            any(x.shape != (c,) for x, c in zip(bs, sizes[1:])):
        raise ValueError("%s: weights[l] must be [sizes[l], sizes[l+1]] and biases[l] [sizes[l+1]]" % what)
    csz = (ctypes.c_int * len(sizes))(*sizes)
    wp = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
    bp = (ctypes.c_void_p * len(bs))(*[x.ctypes.data for x in bs])
    return ws, bs, csz, wp, bp


class _Pinned:
    """numpy array over page-locked host memory (hb_host_alloc): copies to and from it are DMA transfers."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib().hb_host_alloc(max(1, self.nbytes))
        if not self.ptr:
            raise HbError("hb_host_alloc(%d) failed" % self.nbytes)
        buf = (ctypes.c_char * max(1, self.nbytes)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().hb_host_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


class Model:
    """Compiled model (replaces mujoco.MjModel for this path)."""

    def __init__(self, handle):
        self._h = handle
        self._read_sizes()

    def _read_sizes(self):
        s = HbSizes()
        _check(lib().hb_model_sizes(self._h, ctypes.byref(s)), "hb_model_sizes")
        for name, _ in HbSizes._fields_:
            setattr(self, name, getattr(s, name))

    @classmethod
    def load(cls, path):
        err = ctypes.create_string_buffer(1024)
        h = lib().hb_model_load(os.fsencode(path), err, len(err))
        if not h:
            raise HbError("hb_model_load(%s): %s" % (path, err.value.decode()))
        return cls(h)

    @classmethod
    def from_xml_string(cls, xml):
        err = ctypes.create_string_buffer(1024)
        h = lib().hb_model_load_xml_string(xml.encode(), err, len(err))
        if not h:
            raise HbError("hb_model_load_xml_string: %s" % err.value.decode())
        return cls(h)

    def save(self, path):
        err = ctypes.create_string_buffer(1024)
        if lib().hb_model_save(self._h, os.fsencode(path), err, len(err)) != HB_OK:
            raise HbError("hb_model_save: %s" % err.value.decode())

    def __del__(self):
        try:
            if self._h:
                lib().hb_model_free(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def opt(self):
        o = HbOptions()
        _check(lib().hb_options_get(self._h, ctypes.byref(o)), "hb_options_get")
        return o

    def set_opt(self, **kw):
        o = self.opt
        for k, v in kw.items():
            if k == "gravity":
                for i in range(3):
                    o.gravity[i] = v[i]
            else:
                setattr(o, k, v)
        _check(lib().hb_options_set(self._h, ctypes.byref(o)), "hb_options_set")
        self._read_sizes()  # (the solver selects the instantiation: contact and row capacities follow it)

    def pair_order(self, order=-1):
        """contact order of mj_collision (include/hb.h: hb_model_pair_order): 1 body pairs first (the compiler's default), 0 geom pairs
        ascending; -1: query.  Returns the order in force."""
        rc = lib().hb_model_pair_order(self._h, int(order))
        if rc < 0:
            _check(rc, "hb_model_pair_order")
        return rc

    def box_manifold(self, mode=-1):
        """the box - box manifold (include/hb.h: hb_model_box_manifold): 1 every box - box pair is collided by the analytic clipping
        routine, up to eight contacts; 0 (the default) one contact through the portal search; -1: query.  Returns the mode in force.
        Call before a Batch is made of the model."""
        rc = lib().hb_model_box_manifold(self._h, int(mode))
        if rc < 0:
            _check(rc, "hb_model_box_manifold", lib().hb_error().decode() if rc == -1 else None)
        return rc

    def name2id(self, kind, name):
        return lib().hb_model_name2id(self._h, kind.encode(), name.encode())

    def id2name(self, kind, i):
        buf = ctypes.create_string_buffer(256)
        _check(min(0, lib().hb_model_id2name(self._h, kind.encode(), int(i), buf, len(buf))), "hb_model_id2name")
        return buf.value.decode()

    def array(self, field):
        n = lib().hb_model_get_array(self._h, field.encode(), None, 0)
        if n < 0:
            raise KeyError(field)
        out = np.zeros(n, dtype=np.float64)
        lib().hb_model_get_array(self._h, field.encode(), _ptr(out), n)
        return out

    def jac_spec(self, bodies=(), sites=(), body_coms=(), subtree_coms=()):
        """The points of a Jacobian read-out (HbJacSpec, at most 16), in this order: the frame origins of `bodies` (mj_jacBody), the
        `sites` as (body, offset in the body's frame) pairs (mj_jacSite), the centres of mass of `body_coms` (mj_jacBodyCom) and of the
        subtrees rooted at `subtree_coms` (mj_jacSubtreeCom).  Bodies are names or ids."""
        m = self

        def bid(b):
            i = m.name2id("body", b) if isinstance(b, str) else int(b)
            if not 0 <= i < m.nbody:
                raise ValueError("jac_spec: no body %r" % (b,))
            return i
        ipos = m.array("body_ipos").reshape(-1, 3)
        pts = [(JAC_POINT, bid(b), (0.0, 0.0, 0.0)) for b in bodies] + [(JAC_POINT, bid(b), tuple(float(x) for x in off)) for b, off in sites]
        pts += [(JAC_POINT, bid(b), tuple(ipos[bid(b)])) for b in body_coms] + [(JAC_SUBTREE_COM, bid(b), (0.0, 0.0, 0.0)) for b in subtree_coms]
        if not 1 <= len(pts) <= MAX_JAC:
            raise ValueError("jac_spec: %d points, 1 to %d are supported" % (len(pts), MAX_JAC))
        spec = HbJacSpec()
        spec.n = len(pts)
        for k, (kind, body, off) in enumerate(pts):
            spec.kind[k], spec.body[k] = kind, body
            for i in range(3):
                spec.offset[k][i] = off[i]
        return spec

    # ---- equality constraints (include/hb.h: hb_batch_create)
    @property
    def neq(self):
        """number of elements of the model's <equality> section, active or not"""
        return len(self.array("eq_type"))

    def equalities(self):
        """One dict per equality: name, type ("joint" / "connect"), obj1, obj2 (joint ids, -1 for no joint2; body ids, 0 for the world),
        active, data (a joint's polycoef[5]; a connect's anchor in body1's frame [3] | in body2's frame [3]), solref, solimp."""
        t, o1, o2, act = (self.array(f).astype(int) for f in ("eq_type", "eq_obj1id", "eq_obj2id", "eq_active0"))
        data, sr, si = self.array("eq_data").reshape(-1, 11), self.array("eq_solref").reshape(-1, 2), self.array("eq_solimp").reshape(-1, 5)
        return [dict(name=self.id2name("equality", e), type={EQ_CONNECT: "connect", EQ_JOINT: "joint"}[int(t[e])], obj1=int(o1[e]), obj2=int(o2[e]),
                     active=bool(act[e]), data=data[e, :5 if t[e] == EQ_JOINT else 6].copy(), solref=sr[e].copy(), solimp=si[e].copy()) for e in range(len(t))]

    def equality_rows(self):
        """ne: the equality rows a batch of this model has with the options as they are now (one per active joint coupling, three per
        active connect; none under mjDSBL_EQUALITY or mjDSBL_CONSTRAINT)"""
        if self.opt.disableflags & (DSBL_CONSTRAINT | DSBL_EQUALITY):
            return 0
        return int(sum((1 if e["type"] == "joint" else 3) for e in self.equalities() if e["active"]))


class Batch:
    """n_env environments resident on one GPU (replaces n_env mujoco.MjData blocks)."""

    def __init__(self, model, n_env, device=0):
        self.model = model
        self.n_env = int(n_env)
        err = ctypes.create_string_buffer(1024)
        self._h = lib().hb_batch_create(model._h, self.n_env, int(device), err, len(err))
        if not self._h:
            raise HbError("hb_batch_create: %s" % err.value.decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().hb_batch_free(self._h)
            self._h = None
        for pb in (getattr(self, "_env_pin", None) or {}).values():
            if isinstance(pb, _Pinned):
                pb.free()
        self._env_pin = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().hb_batch_stream(self._h)

    def sync(self):
        _check(lib().hb_batch_sync(self._h), "hb_batch_sync")

    def pipeline(self, on=True):
        """Pipelined stepping (hb_batch_pipeline): env segments (three by default, two when the process' streams cannot have a hardware queue each) on their own streams, so the slow tail of
        one step overlaps the next step.  Results are identical; see include/hb.h for the stream contract."""
        _check(lib().hb_batch_pipeline(self._h, int(on)), "hb_batch_pipeline")  # True: the default; 2..8: that many

    @property
    def segments(self):
        """env segments a step call is cut into at the moment (1: unpipelined)"""
        return lib().hb_batch_segments(self._h)

    def join(self):
        _check(lib().hb_batch_join(self._h), "hb_batch_join")

    def reset(self, mask=None, keyframe=-1, perturb=False, env_offset=0):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        _check(lib().hb_reset(self._h, _ptr(m), int(keyframe), int(bool(perturb)), int(env_offset)), "hb_reset")

    def step(self, ctrl, n_substeps=1):
        c = np.ascontiguousarray(ctrl, dtype=np.float32)
        assert c.shape == (self.n_env, self.model.nu), c.shape
        _check(lib().hb_step(self._h, _ptr(c), int(n_substeps)), "hb_step")

    def step_dev(self, ctrl_ptr, n_substeps=1):
        """ctrl_ptr: device address (int) of a float32 [n_env, nu] array; asynchronous."""
        _check(lib().hb_step_dev(self._h, ctypes.c_void_p(ctrl_ptr), int(n_substeps)), "hb_step_dev")

    def forward(self, ctrl=None):
        c = None if ctrl is None else np.ascontiguousarray(ctrl, dtype=np.float32)
        _check(lib().hb_forward(self._h, _ptr(c)), "hb_forward")

    def inverse(self, qacc, discrete=False, want_warnings=False):
        """mj_inverse of every env at its current state (include/hb.h: hb_inverse): qacc float32 [n_env, nv] -> qfrc_inverse float32
        [n_env, nv]; with want_warnings also the per-env HB_WARN_CONTACTFULL / HB_WARN_CNSTRFULL bits of rows this call dropped.
        discrete: qacc is (qvel' - qvel) / h of one step (mjENBL_INVDISCRETE).  The batch's state is left as it is."""
        a = np.ascontiguousarray(qacc, dtype=np.float32)
        assert a.shape == (self.n_env, self.model.nv), a.shape
        out = np.empty((self.n_env, self.model.nv), dtype=np.float32)
        warn = np.zeros(self.n_env, dtype=np.int32) if want_warnings else None
        _check(lib().hb_inverse(self._h, _ptr(a), HB_INV_DISCRETE if discrete else 0, _ptr(out), _ptr(warn)), "hb_inverse")
        return (out, warn) if want_warnings else out

    def inverse_dev(self, qacc_ptr, out_ptr, discrete=False, warnings_ptr=None):
        """qacc_ptr / out_ptr: device addresses (int) of float32 [n_env, nv] arrays, warnings_ptr (nullable) of int32 [n_env];
        asynchronous (hb_inverse_dev)."""
        _check(lib().hb_inverse_dev(self._h, ctypes.c_void_p(qacc_ptr), HB_INV_DISCRETE if discrete else 0, ctypes.c_void_p(out_ptr),
                                    ctypes.c_void_p(warnings_ptr) if warnings_ptr else None), "hb_inverse_dev")

    def _kin_out(self, lead, pose, vel, geoms):
        m = self.model
        return (np.empty(lead + (m.nbody, 10), dtype=np.float32) if pose else None, np.empty(lead + (m.nbody, 6), dtype=np.float32) if vel else None,
                np.empty(lead + (m.ngeom, 7), dtype=np.float32) if geoms else None)

    def kinematics(self, pose=True, vel=True, geoms=False):
        """mj_kinematics + mj_objectVelocity of every env at its state as it is now (include/hb.h: hb_kinematics): a dict of float32
        arrays, "pose" [n_env, nbody, 10] = xpos | xquat (w x y z) | xipos, "vel" [n_env, nbody, 6] = omega | velocity of the body's
        xipos (world axes), "geoms" [n_env, ngeom, 7] = geom_xpos | quaternion - those asked for.  The batch is left as it is."""
        p, v, g = self._kin_out((self.n_env,), pose, vel, geoms)
        _check(lib().hb_kinematics(self._h, _ptr(p), _ptr(v), _ptr(g)), "hb_kinematics")
        return {k: a for k, a in (("pose", p), ("vel", v), ("geoms", g)) if a is not None}

    def kinematics_dev(self, pose_ptr=None, vel_ptr=None, geom_ptr=None):
        """the same into device arrays (addresses as int, None: not wanted); asynchronous (hb_kinematics_dev)"""
        _check(lib().hb_kinematics_dev(self._h, ctypes.c_void_p(pose_ptr or 0), ctypes.c_void_p(vel_ptr or 0), ctypes.c_void_p(geom_ptr or 0)), "hb_kinematics_dev")

    def kinematics_states(self, qpos, qvel=None, pose=True, vel=True, geoms=False):
        """the same of given states (hb_kinematics_states): qpos [n, nq] or [T, n_env, nq] (e.g. rollout_trajectory's), qvel likewise
        (may be None with vel=False); any n.  The arrays of the returned dict have qpos' leading shape."""
        q = np.ascontiguousarray(qpos, dtype=np.float32)
        assert q.ndim >= 2 and q.shape[-1] == self.model.nq, q.shape
        lead = q.shape[:-1]
        n = int(np.prod(lead))
        assert n < 2 ** 31, "hb_kinematics_states takes the number of states as an int: %d states, split the call" % n
        qv = None
        if qvel is not None:
            qv = np.ascontiguousarray(qvel, dtype=np.float32)
            assert qv.shape == lead + (self.model.nv,), qv.shape
        p, v, g = self._kin_out(lead, pose, vel, geoms)
        _check(lib().hb_kinematics_states(self._h, _ptr(q), _ptr(qv), n, _ptr(p), _ptr(v), _ptr(g)), "hb_kinematics_states")
        return {k: a for k, a in (("pose", p), ("vel", v), ("geoms", g)) if a is not None}

    def kinematics_states_dev(self, qpos_ptr, qvel_ptr, n, pose_ptr=None, vel_ptr=None, geom_ptr=None):
        """device arrays: qpos [n, nq], qvel [n, nv] (None without vel_ptr) in, the outputs asked for out; asynchronous"""
        assert int(n) < 2 ** 31, n
        _check(lib().hb_kinematics_states_dev(self._h, ctypes.c_void_p(qpos_ptr or 0), ctypes.c_void_p(qvel_ptr or 0), int(n), ctypes.c_void_p(pose_ptr or 0),
                                              ctypes.c_void_p(vel_ptr or 0), ctypes.c_void_p(geom_ptr or 0)), "hb_kinematics_states_dev")

    # ---- dynamics read-out (mj_fullM, qfrc_bias, qfrc_passive, mj_jac*; include/hb.h: hb_dynamics)
    def jac_spec(self, bodies=(), sites=(), body_coms=(), subtree_coms=()):
        """the points of a Jacobian read-out, for dynamics(jac=...): Model.jac_spec"""
        return self.model.jac_spec(bodies=bodies, sites=sites, body_coms=body_coms, subtree_coms=subtree_coms)

    def _dyn_out(self, lead, M, bias, passive, jac):
        nv = self.model.nv
        return (np.empty(lead + (nv, nv), dtype=np.float32) if M else None, np.empty(lead + (nv,), dtype=np.float32) if bias else None,
                np.empty(lead + (nv,), dtype=np.float32) if passive else None, np.empty(lead + (jac.n, 6, nv), dtype=np.float32) if jac is not None else None)

    @staticmethod
    def _dyn_dict(M, b, p, j):
        return {k: a for k, a in (("M", M), ("bias", b), ("passive", p), ("jac", j)) if a is not None}

    def dynamics(self, M=True, bias=True, passive=True, jac=None):
        """The terms of the equations of motion of every env at its state as it is now (include/hb.h: hb_dynamics): a dict of float32
        arrays, "M" [n_env, nv, nv] the dense mass matrix (mj_fullM), "bias" [n_env, nv] qfrc_bias, "passive" [n_env, nv] qfrc_passive,
        "jac" [n_env, jac.n, 6, nv] = jacp | jacr of the points of `jac` (a jac_spec) - those asked for.  With domain randomisation
        installed every env's own masses, armature and stiffness enter.  The batch is left as it is."""
        Mo, b, p, j = self._dyn_out((self.n_env,), M, bias, passive, jac)
        _check(lib().hb_dynamics(self._h, _ptr(Mo), _ptr(b), _ptr(p), ctypes.byref(jac) if jac is not None else None, _ptr(j)), "hb_dynamics")
        return self._dyn_dict(Mo, b, p, j)

    def dynamics_dev(self, M_ptr=None, bias_ptr=None, passive_ptr=None, jac=None, jac_ptr=None):
        """the same into device arrays (addresses as int, None: not wanted); asynchronous (hb_dynamics_dev)"""
        _check(lib().hb_dynamics_dev(self._h, ctypes.c_void_p(M_ptr or 0), ctypes.c_void_p(bias_ptr or 0), ctypes.c_void_p(passive_ptr or 0),
                                     ctypes.byref(jac) if jac is not None else None, ctypes.c_void_p(jac_ptr or 0)), "hb_dynamics_dev")

    def dynamics_states(self, qpos, qvel=None, M=True, bias=True, passive=True, jac=None):
        """the same of given states with the model's nominal parameters (hb_dynamics_states): qpos [n, nq] or [T, n_env, nq], qvel
        likewise (may be None with bias=False, passive=False); any n.  The arrays of the returned dict have qpos' leading shape."""
        q = np.ascontiguousarray(qpos, dtype=np.float32)
        assert q.ndim >= 2 and q.shape[-1] == self.model.nq, q.shape
        lead = q.shape[:-1]
        n = int(np.prod(lead))
        assert n < 2 ** 31, "hb_dynamics_states takes the number of states as an int: %d states, split the call" % n
        qv = None
        if qvel is not None:
            qv = np.ascontiguousarray(qvel, dtype=np.float32)
            assert qv.shape == lead + (self.model.nv,), qv.shape
        Mo, b, p, j = self._dyn_out(lead, M, bias, passive, jac)
        _check(lib().hb_dynamics_states(self._h, _ptr(q), _ptr(qv), n, _ptr(Mo), _ptr(b), _ptr(p), ctypes.byref(jac) if jac is not None else None, _ptr(j)),
               "hb_dynamics_states")
        return self._dyn_dict(Mo, b, p, j)

    def dynamics_states_dev(self, qpos_ptr, qvel_ptr, n, M_ptr=None, bias_ptr=None, passive_ptr=None, jac=None, jac_ptr=None):
        """device arrays: qpos [n, nq], qvel [n, nv] (None without bias_ptr and passive_ptr) in, the outputs asked for out; asynchronous"""
        assert int(n) < 2 ** 31, n
        _check(lib().hb_dynamics_states_dev(self._h, ctypes.c_void_p(qpos_ptr or 0), ctypes.c_void_p(qvel_ptr or 0), int(n), ctypes.c_void_p(M_ptr or 0),
                                            ctypes.c_void_p(bias_ptr or 0), ctypes.c_void_p(passive_ptr or 0), ctypes.byref(jac) if jac is not None else None,
                                            ctypes.c_void_p(jac_ptr or 0)), "hb_dynamics_states_dev")

    # ---- ray casting (mj_ray of a fixed set of rays in every env; include/hb.h)
    def _no_rays_why(self, rc, flags, bodyexclude):
        """HB_EUNSUPPORTED (-4) from hb_ray_configure: name the first eligible geom that has no ray surface (include/hb.h)"""
        if rc != -4:
            return None
        m = self.model
        gtype, gbody = m.array("geom_type").astype(int), m.array("geom_bodyid").astype(int)
        marker = (m.array("geom_contype") == 0) & (m.array("geom_conaffinity") == 0)
        names = {5: "cylinder", 7: "mesh", 4: "ellipsoid"}
        for g in range(m.ngeom):
            if gbody[g] != bodyexclude and (flags & (RAY_STATIC if gbody[g] == 0 else RAY_MOVING)) and gtype[g] not in RAY_SURFACES and not marker[g]:
                return ("geom %d (%s, a %s geom of body %r) would be eligible and rays intersect planes, height fields, spheres, capsules and boxes only"
                        % (g, m.id2name("geom", g) or "unnamed", names.get(int(gtype[g]), "type %d" % gtype[g]), m.id2name("body", int(gbody[g]))))
        return None

    def ray_configure(self, pnt, vec, frame="world", frame_body=0, bodyexclude=-1, static=True, moving=True, cutoff=0.0):
        """Installs rays (hb_ray_configure): pnt, vec [n_ray, 3] in the world frame, in frame_body's frame ("body": a rangefinder site) or in
        its heading frame ("yaw": the height-scan frame); static / moving: geoms of the world body / of the other bodies are eligible,
        less those of body bodyexclude; hits beyond cutoff (> 0) count as none.  pnt=None removes the rays.  A configuration that is
        refused (HbError) leaves the previous one installed."""
        if pnt is None:
            _check(lib().hb_ray_configure(self._h, None, None, None, 0), "hb_ray_configure")
            self._n_ray = 0
            return
        p, v = np.ascontiguousarray(pnt, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(vec, dtype=np.float32).reshape(-1, 3)
        assert p.shape == v.shape, (p.shape, v.shape)
        flags = (RAY_STATIC if static else 0) | (RAY_MOVING if moving else 0)
        spec = HbRaySpec(RAY_FRAMES[frame] if isinstance(frame, str) else int(frame), int(frame_body), int(bodyexclude), flags, float(cutoff))
        rc = lib().hb_ray_configure(self._h, ctypes.byref(spec), _ptr(p), _ptr(v), len(p))
        _check(rc, "hb_ray_configure", self._no_rays_why(rc, flags, int(bodyexclude)))
        self._n_ray = len(p)

    def rays(self):
        """(dist float32 [n_env, n_ray], geomid int32 [n_env, n_ray]) of the installed rays at the batch's state as it is now (hb_rays):
        metres to the nearest eligible surface and the geom hit, -1 / -1 where nothing is.  The batch is left as it is."""
        n = getattr(self, "_n_ray", 0)
        dist, gid = np.empty((self.n_env, n), dtype=np.float32), np.empty((self.n_env, n), dtype=np.int32)
        _check(lib().hb_rays(self._h, _ptr(dist) if n else None, _ptr(gid) if n else None), "hb_rays")
        return dist, gid

    def rays_dev(self, dist_ptr=None, geomid_ptr=None):
        """the same into device arrays (addresses as int, None: not wanted); asynchronous (hb_rays_dev)"""
        _check(lib().hb_rays_dev(self._h, ctypes.c_void_p(dist_ptr or 0), ctypes.c_void_p(geomid_ptr or 0)), "hb_rays_dev")

    def rollout(self, ctrl, want_qpos=False):
        c = np.ascontiguousarray(ctrl, dtype=np.float32)
        T = c.shape[0]
        assert c.shape == (T, self.n_env, self.model.nu), c.shape
        q = np.zeros((T, self.n_env, self.model.nq), dtype=np.float32) if want_qpos else None
        _check(lib().hb_rollout(self._h, _ptr(c), T, _ptr(q)), "hb_rollout")
        return q

    def rollout_dev(self, ctrl_ptr, T, qpos_out_ptr=None):
        _check(lib().hb_rollout_dev(self._h, ctypes.c_void_p(ctrl_ptr), int(T), ctypes.c_void_p(qpos_out_ptr or 0)), "hb_rollout_dev")

    def rollout_halton(self, T, t0=0, env_offset=0, qpos_out_ptr=None):
        _check(lib().hb_rollout_halton(self._h, int(T), int(t0), int(env_offset), ctypes.c_void_p(qpos_out_ptr or 0)), "hb_rollout_halton")

    def state_size(self, spec):
        return lib().hb_state_size(self._h, spec)

    def get_state(self, spec=STATE_INTEGRATION, dtype=np.float32):
        w = self.state_size(spec)
        out = np.zeros((self.n_env, w), dtype=dtype)
        fn = lib().hb_get_state if dtype == np.float32 else lib().hb_get_state_f64
        _check(fn(self._h, spec, _ptr(out)), "hb_get_state")
        return out

    def set_state(self, spec, values):
        dt = np.float64 if np.asarray(values).dtype == np.float64 else np.float32
        v = np.ascontiguousarray(values, dtype=dt)
        assert v.shape == (self.n_env, self.state_size(spec)), v.shape
        fn = lib().hb_set_state if dt == np.float32 else lib().hb_set_state_f64
        _check(fn(self._h, spec, _ptr(v)), "hb_set_state")

    @property
    def qpos(self):
        return self.get_state(STATE_QPOS)

    @property
    def qvel(self):
        return self.get_state(STATE_QVEL)

    @property
    def time(self):
        return self.get_state(STATE_TIME)[:, 0]

    def obs(self, want_reward=True):
        o = np.zeros((self.n_env, self.env_nobs), dtype=np.float32)
        r = np.zeros(self.n_env, dtype=np.float32) if want_reward else None
        te = np.zeros(self.n_env, dtype=np.uint8)
        tr = np.zeros(self.n_env, dtype=np.uint8)
        _check(lib().hb_get_obs(self._h, _ptr(o), _ptr(r), _ptr(te), _ptr(tr)), "hb_get_obs")
        return o, r, te.astype(bool), tr.astype(bool)

    def status(self):
        s = np.zeros(self.n_env, dtype=np.int32)
        _check(lib().hb_get_status(self._h, _ptr(s)), "hb_get_status")
        return s

    def counts(self):
        a, b, c = (np.zeros(self.n_env, dtype=np.int32) for _ in range(3))
        _check(lib().hb_get_counts(self._h, _ptr(a), _ptr(b), _ptr(c)), "hb_get_counts")
        return a, b, c

    TUNE = {"duo": 0, "lean": 1, "sized": 2, "staged": 3, "fastpass": 4, "narrow_prim": 5, "schedule": 6, "reorder_period": 7, "policy_lean": 8, "fold": 9,
            "kin_pack": 10}

    def tune(self, **knobs):
        """run-time choices between kernels / schedules that give the same results (include/hb.h: hb_batch_tune, HB_TUNE_*), e.g.
        tune(duo=2, staged=0)"""
        for k, v in knobs.items():
            _check(lib().hb_batch_tune(self._h, self.TUNE[k], int(v)), "hb_batch_tune")

    def duo(self, mode=1):
        """two envs per wave for the lean launches of the 27-dof humanoid's PGS kernel: 0 never, 1 where it pays (default), 2 always"""
        self.tune(duo=mode)

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        _check(lib().hb_batch_device_name(self._h, buf, 256), "hb_batch_device_name")
        return buf.value.decode()

    def step_launches(self):
        """number of step launches so far (include/hb.h: hb_batch_step_launches)"""
        return int(lib().hb_batch_step_launches(self._h))

    def last_kernel(self):
        """name of the step kernel the batch's last step / rollout / forward launch ran (include/hb.h: hb_last_kernel)"""
        return lib().hb_last_kernel(self._h).decode()

    def collision_counts(self, want_cycles=False):
        """(work items, portal searches[, narrowphase wave time in 1024-cycle units]) of every env's last step (general collision
        models; zeros otherwise)."""
        a, b, c = (np.zeros(self.n_env, dtype=np.int32) for _ in range(3))
        _check(lib().hb_get_collision_counts(self._h, _ptr(a), _ptr(b), _ptr(c)), "hb_get_collision_counts")
        return (a, b, c) if want_cycles else (a, b)

    def diag_enable(self, on=True):
        _check(lib().hb_diag_enable(self._h, int(on)), "hb_diag_enable")

    def qacc(self):
        out = np.zeros((self.n_env, self.model.nv), dtype=np.float32)
        _check(lib().hb_get_qacc(self._h, _ptr(out)), "hb_get_qacc")
        return out

    def efc_force(self):
        out = np.zeros((self.n_env, self.model.nefc_max), dtype=np.float32)
        _check(lib().hb_get_efc_force(self._h, _ptr(out)), "hb_get_efc_force")
        return out

    def contacts(self):
        out = np.zeros((self.n_env, self.model.ncon_max, 16), dtype=np.float32)
        _check(lib().hb_get_contacts(self._h, _ptr(out)), "hb_get_contacts")
        return out

    # ---- contact forces (mj_contactForce, cfrc_ext without xfrc_applied; include/hb.h)
    def contact_readout(self, on=True):
        """From the next launch on, steps write every contact's force and every body's contact wrench (full step kernels only)."""
        rc = lib().hb_contact_readout(self._h, int(on))
        _check(rc, "hb_contact_readout", lib().hb_error().decode() if rc == -1 else None)

    def contact_force(self):
        """[n_env, ncon_max, 6]: contact-frame force and torque of contact k of contacts(); zeros beyond the env's ncon."""
        out = np.zeros((self.n_env, self.model.ncon_max, 6), dtype=np.float32)
        _check(lib().hb_get_contact_force(self._h, _ptr(out)), "hb_get_contact_force")
        return out

    def body_contact(self):
        """[n_env, nbody, 6]: force | torque about the body's xipos, world axes, of the contacts on every body (row 0: the world)."""
        out = np.zeros((self.n_env, self.model.nbody, 6), dtype=np.float32)
        _check(lib().hb_get_body_contact(self._h, _ptr(out)), "hb_get_body_contact")
        return out

    def contact_readout_dev(self):
        """Device addresses (contact_force, body_contact) of the read-out buffers, ordered behind the step calls made so far."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().hb_contact_readout_dev(self._h, ctypes.byref(a), ctypes.byref(b)), "hb_contact_readout_dev")
        return a.value, b.value

    # ---- body accelerations (mj_objectAcceleration of every body, gravity pseudo-acceleration included; include/hb.h)
    def _no_body_acc_why(self, rc):
        """HB_EUNSUPPORTED (-4) from a body-acceleration read-out on a model with equality rows or joint frictionloss: say so (include/hb.h)"""
        if rc == -4 and self.model.equality_rows():
            return "a model with equality constraints has no body-acceleration read-out (accelerometer, gyro and frame-acceleration sensors included)"
        if rc == -4 and self.model.array("dof_frictionloss").any():
            return "a model with joint friction loss has no body-acceleration read-out (accelerometer, gyro and frame-acceleration sensors included)"
        return None

    def body_acc_readout(self, on=True):
        """From the next launch on, steps write every body's acceleration (full step kernels only)."""
        rc = lib().hb_body_acc_readout(self._h, int(on))
        _check(rc, "hb_body_acc_readout", self._no_body_acc_why(rc))

    def body_acc(self):
        """[n_env, nbody, 6]: angular | linear acceleration of the body's xipos, world axes (row 0, the world: (0, -gravity))."""
        out = np.zeros((self.n_env, self.model.nbody, 6), dtype=np.float32)
        _check(lib().hb_get_body_acc(self._h, _ptr(out)), "hb_get_body_acc")
        return out

    def body_acc_readout_dev(self):
        """Device address of the read-out buffer, ordered behind the step calls made so far."""
        a = ctypes.c_void_p()
        _check(lib().hb_body_acc_readout_dev(self._h, ctypes.byref(a)), "hb_body_acc_readout_dev")
        return a.value

    # ---- wire format: agent.proto State of one env
    def state_to_proto(self, env):
        n = lib().hb_state_to_proto(self._h, int(env), None, 0)
        if n < 0:
            _check(n, "hb_state_to_proto")
        buf = ctypes.create_string_buffer(n)
        _check(min(0, lib().hb_state_to_proto(self._h, int(env), buf, n)), "hb_state_to_proto")
        return buf.raw

    def state_from_proto(self, env, data):
        _check(lib().hb_state_from_proto(self._h, int(env), bytes(data), len(data)), "hb_state_from_proto")

    # ---- planner rollouts (MJPC Trajectory::Rollout analogue)
    @staticmethod
    def sensor_spec(framepos_bodies=(), subtree_body=-1, offsets=None, axes=(), linvel_bodies=(), subtreelinvel_bodies=(), touch_bodies=(),
                    contactforce_bodies=(), imu=(), frameacc_bodies=()):
        """offsets: per frame, the site's position in its body frame (None / missing: the body frame itself);
        axes: (body, which) pairs, which = 0 (framexaxis) or 2 (framezaxis); linvel_bodies: framelinvel (objtype body);
        subtreelinvel_bodies: subtreelinvel of further bodies; touch_bodies: summed normal contact force of a body (one float);
        contactforce_bodies: contact force on a body, world axes (three floats); imu: (body, (x, y, z)) pairs, accelerometer | gyro
        of a site at that offset in the body frame, in the body's axes (six floats); frameacc_bodies: frameangacc | framelinacc of a
        body, world axes (six floats: its row of body_acc())."""
        sp = HbSensorSpec()
        sp.n_framepos = len(framepos_bodies)
        for k, bd in enumerate(framepos_bodies):
            sp.framepos_body[k] = int(bd)
            if offsets is not None and offsets[k] is not None:
                for i in range(3):
                    sp.framepos_offset[k][i] = float(offsets[k][i])
        sp.subtree_body = int(subtree_body)
        sp.n_frameaxis = len(axes)
        for k, (bd, which) in enumerate(axes):
            sp.frameaxis_body[k] = int(bd); sp.frameaxis_which[k] = int(which)
        sp.n_framelinvel = len(linvel_bodies)
        for k, bd in enumerate(linvel_bodies):
            sp.framelinvel_body[k] = int(bd)
        sp.n_subtreelinvel = len(subtreelinvel_bodies)
        for k, bd in enumerate(subtreelinvel_bodies):
            sp.subtreelinvel_body[k] = int(bd)
        sp.n_touch = len(touch_bodies)
        for k, bd in enumerate(touch_bodies):
            sp.touch_body[k] = int(bd)
        sp.n_contactforce = len(contactforce_bodies)
        for k, bd in enumerate(contactforce_bodies):
            sp.contactforce_body[k] = int(bd)
        sp.n_imu = len(imu)
        for k, (bd, off) in enumerate(imu):
            sp.imu_body[k] = int(bd)
            for i in range(3):
                sp.imu_offset[k][i] = float(off[i])
        sp.n_frameacc = len(frameacc_bodies)
        for k, bd in enumerate(frameacc_bodies):
            sp.frameacc_body[k] = int(bd)
        return sp

    @staticmethod
    def _sensor_size(spec):
        ns = lib().hb_sensor_size(ctypes.byref(spec))
        if ns <= 0:
            raise HbError("hb_sensor_size: invalid sensor spec")
        return ns

    @staticmethod
    def sensor_layout(spec):
        """where each part of a row of `spec` is: {part: (offset, floats)} for SENSOR_PARTS (a part that is off: 0 floats), and "width"
        (hb_sensor_row; the floats of a part end where the next part begins)"""
        r = HbSensorRow()
        _check(lib().hb_sensor_row(ctypes.byref(spec), ctypes.byref(r)), "hb_sensor_row")
        ends = [getattr(r, n) for n in SENSOR_PARTS[1:]] + [r.width]
        out = {n: (getattr(r, n), end - getattr(r, n)) for n, end in zip(SENSOR_PARTS, ends)}
        out["width"] = r.width
        return out

    def set_state_broadcast(self, spec, state):
        """One state record on every env (the common start of a sampling planner's candidates)."""
        s = np.ascontiguousarray(state)
        if s.dtype == np.float64:
            _check(lib().hb_set_state_broadcast_f64(self._h, spec, _ptr(s)), "hb_set_state_broadcast_f64")
        else:
            s = s.astype(np.float32)
            _check(lib().hb_set_state_broadcast(self._h, spec, _ptr(s)), "hb_set_state_broadcast")

    def rollout_sensors(self, ctrl, spec, want_qpos=False):
        """ctrl [T, n_env, nu] -> sensors [T, n_env, ns] (evaluated before each step's integration), qpos [T, n_env, nq] or None."""
        c = np.ascontiguousarray(ctrl, dtype=np.float32)
        T = c.shape[0]
        assert c.shape == (T, self.n_env, self.model.nu), c.shape
        ns = self._sensor_size(spec)
        out = np.zeros((T, self.n_env, ns), dtype=np.float32)
        q = np.zeros((T, self.n_env, self.model.nq), dtype=np.float32) if want_qpos else None
        _check(lib().hb_rollout_sensors(self._h, _ptr(c), T, ctypes.byref(spec), _ptr(out), _ptr(q)), "hb_rollout_sensors")
        return out, q

    def transition_fd(self, x, u, warmstart=None, eps=1e-3, centered=True, sensor_spec=None):
        """mjd_transitionFD for T points at once: x [T, nq + nv], u [T, nu] -> A [T, 2nv, 2nv], B [T, 2nv, nu] (float64)."""
        xs = np.ascontiguousarray(x, dtype=np.float64)
        us = np.ascontiguousarray(u, dtype=np.float64)
        T, nv, nu = xs.shape[0], self.model.nv, self.model.nu
        assert xs.shape == (T, self.model.nq + nv) and us.shape == (T, nu)
        w = None if warmstart is None else np.ascontiguousarray(warmstart, dtype=np.float64)
        A = np.zeros((T, 2 * nv, 2 * nv)); B = np.zeros((T, 2 * nv, nu))
        if sensor_spec is None:
            _check(lib().hb_transition_fd(self._h, _ptr(xs), _ptr(us), _ptr(w), T, float(eps), int(bool(centered)), _ptr(A), _ptr(B)), "hb_transition_fd")
            return A, B
        ns = lib().hb_sensor_size(ctypes.byref(sensor_spec))  # (not _sensor_size: a spec it refuses has always ended in np.zeros' ValueError here)
        C = np.zeros((T, ns, 2 * nv)); D = np.zeros((T, ns, nu))
        _check(lib().hb_transition_fd_sensors(self._h, _ptr(xs), _ptr(us), _ptr(w), T, float(eps), int(bool(centered)), ctypes.byref(sensor_spec),
                                              _ptr(A), _ptr(B), _ptr(C), _ptr(D)), "hb_transition_fd_sensors")
        return A, B, C, D

    def ctrl_tape_splines(self, knots, times, interpolation, time0, T):
        """knots [n_env, P, nu], times [P] -> the action tape of T steps on the device (SamplingPolicy::Action per candidate);
        pass ("tape", T) as `ctrl` to rollout_task_stand / rollout_task_walk."""
        k = np.ascontiguousarray(knots, dtype=np.float32)
        tm = np.ascontiguousarray(times, dtype=np.float32)
        assert k.shape == (self.n_env, len(tm), self.model.nu), k.shape
        _check(lib().hb_ctrl_tape_splines(self._h, _ptr(k) if len(tm) else None, _ptr(tm) if len(tm) else None, len(tm), int(interpolation), float(time0), int(T)),
               "hb_ctrl_tape_splines")

    def ctrl_tape_read(self, T):
        """The tape ctrl_tape_splines left on the device: [T, n_env, nu] (TimeSpline::Sample per candidate and step time)."""
        out = np.zeros((int(T), self.n_env, self.model.nu), dtype=np.float32)
        _check(lib().hb_ctrl_tape_read(self._h, int(T), _ptr(out)), "hb_ctrl_tape_read")
        return out

    def task_cost(self, residual, dims, norms, weights, norm_p=None, risk=0.0):
        """BaseResidualFn::CostTerms / CostValue on the device for residual [n, n_residual] -> (terms [n, n_term], cost [n])."""
        r = np.ascontiguousarray(residual, dtype=np.float32)
        n, nres = r.shape
        sp = HbCostSpec()
        sp.n_term = len(dims)
        for k in range(len(dims)):
            sp.dim[k] = int(dims[k]); sp.norm[k] = int(norms[k]); sp.weight[k] = float(weights[k])
            if norm_p is not None:
                sp.norm_p[k][0] = float(norm_p[k][0]); sp.norm_p[k][1] = float(norm_p[k][1])
        sp.risk = float(risk)
        terms = np.zeros((n, len(dims)), dtype=np.float32)
        cost = np.zeros(n, dtype=np.float32)
        _check(lib().hb_task_cost(self._h, _ptr(r), n, nres, ctypes.byref(sp), _ptr(terms), _ptr(cost)), "hb_task_cost")
        return terms, cost

    def _tape_or_ctrl(self, ctrl):
        if isinstance(ctrl, tuple) and ctrl[0] == "tape":
            return int(ctrl[1]) + 1, ctypes.c_void_p(1)  # HB_CTRL_TAPE
        c = np.ascontiguousarray(ctrl, dtype=np.float32)
        H = c.shape[0] + 1
        assert c.shape == (H - 1, self.n_env, self.model.nu), c.shape
        self._keep = c
        return H, (_ptr(c) if H > 1 else None)

    def task_stand_default(self):
        t = HbTaskStand()
        _check(lib().hb_task_stand_default(self.model._h, ctypes.byref(t)), "hb_task_stand_default")
        return t

    def rollout_task_stand(self, ctrl, task, want_costs=False):
        """ctrl [horizon - 1, n_env, nu] -> (total_return [n_env], stage costs [horizon, n_env] or None) of MJPC's Humanoid Stand task."""
        H, cp = self._tape_or_ctrl(ctrl)
        total = np.zeros(self.n_env, dtype=np.float32)
        costs = np.zeros((H, self.n_env), dtype=np.float32) if want_costs else None
        _check(lib().hb_rollout_task_stand(self._h, cp, H, ctypes.byref(task), _ptr(total), _ptr(costs)), "hb_rollout_task_stand")
        return total, costs

    def task_walk_default(self):
        t = HbTaskWalk()
        _check(lib().hb_task_walk_default(self.model._h, ctypes.byref(t)), "hb_task_walk_default")
        return t

    def rollout_task_walk(self, ctrl, task, want_costs=False):
        """ctrl [horizon - 1, n_env, nu] -> (total_return [n_env], stage costs [horizon, n_env] or None) of MJPC's Humanoid Walk task."""
        H, cp = self._tape_or_ctrl(ctrl)
        total = np.zeros(self.n_env, dtype=np.float32)
        costs = np.zeros((H, self.n_env), dtype=np.float32) if want_costs else None
        _check(lib().hb_rollout_task_walk(self._h, cp, H, ctypes.byref(task), _ptr(total), _ptr(costs)), "hb_rollout_task_walk")
        return total, costs

    def rollout_noise(self, xfrc_std, xfrc_rate, seed=0):
        """Ornstein-Uhlenbeck noise on xfrc_applied for the rollouts that follow (Trajectory::NoisyRollout); std 0: off."""
        _check(lib().hb_rollout_noise(self._h, float(xfrc_std), float(xfrc_rate), int(seed)), "hb_rollout_noise")

    def rollout_trajectory(self, ctrl):
        """ctrl [T, n_env, nu] -> (qpos [T, n_env, nq], qvel [T, n_env, nv], failed [n_env]): the states after every step."""
        c = np.ascontiguousarray(ctrl, dtype=np.float32)
        T = c.shape[0]
        assert c.shape == (T, self.n_env, self.model.nu), c.shape
        q = np.zeros((T, self.n_env, self.model.nq), dtype=np.float32)
        v = np.zeros((T, self.n_env, self.model.nv), dtype=np.float32)
        f = np.zeros(self.n_env, dtype=np.int32)
        _check(lib().hb_rollout_trajectory(self._h, _ptr(c), T, _ptr(q), _ptr(v), _ptr(f)), "hb_rollout_trajectory")
        return q, v, f.astype(bool)

    def sensors(self, spec, ctrl=None):
        ns = self._sensor_size(spec)
        out = np.zeros((self.n_env, ns), dtype=np.float32)
        c = None if ctrl is None else np.ascontiguousarray(ctrl, dtype=np.float32)
        rc = lib().hb_sensors(self._h, _ptr(c), ctypes.byref(spec), _ptr(out))
        _check(rc, "hb_sensors", self._no_body_acc_why(rc) if spec.n_imu + spec.n_frameacc else None)
        return out

    # ---- env adapter (CPUEnv.step/reset analogue)
    def env_default_config(self):
        c = HbEnvConfig()
        _check(lib().hb_env_default_config(self.model._h, ctypes.byref(c)), "hb_env_default_config")
        return c

    def env_team_config(self):
        """The reference's own values for its own robot (hb_env_team_config)."""
        c = HbEnvConfig()
        _check(lib().hb_env_team_config(self.model._h, ctypes.byref(c)), "hb_env_team_config")
        return c

    def env_configure(self, cfg):
        _check(lib().hb_env_configure(self._h, ctypes.byref(cfg)), "hb_env_configure")

    def env_default_randomization(self):
        r = HbEnvRandomization()
        _check(lib().hb_env_default_randomization(self.model._h, ctypes.byref(r)), "hb_env_default_randomization")
        return r

    def env_randomize(self, cfg):
        """Install (cfg.factor > 0) or remove (None) the realism layer; call before env_reset."""
        _check(lib().hb_env_randomize(self._h, ctypes.byref(cfg) if cfg is not None else None), "hb_env_randomize")

    def env_default_domain_randomization(self):
        d = HbDomainRandomization()
        _check(lib().hb_env_default_domain_randomization(self.model._h, ctypes.byref(d)), "hb_env_default_domain_randomization")
        return d

    def env_domain_randomize(self, cfg):
        """Install (cfg.factor > 0) or remove (None) per-env model parameters; call before env_reset."""
        _check(lib().hb_env_domain_randomize(self._h, ctypes.byref(cfg) if cfg is not None else None), "hb_env_domain_randomize")

    def env_domain_params(self):
        """[n_env, stride] float32 (layout in include/hb.h), or None when domain randomisation is off."""
        stride = lib().hb_env_get_domain_params(self._h, None)
        if stride < 0:
            _check(stride, "hb_env_get_domain_params")
        if stride == 0:
            return None
        out = np.zeros((self.n_env, stride), dtype=np.float32)
        _check(min(0, lib().hb_env_get_domain_params(self._h, _ptr(out))), "hb_env_get_domain_params")
        return out

    @property
    def env_nobs(self):
        """the width of every observation row the env adapter produces: the model's nobs and what obs_extend appended (hb_env_nobs)"""
        return int(lib().hb_env_nobs(self._h))

    def env_row(self):
        """the layout of those rows, [base | prev_action | scan | foot_contact | command]: an HbEnvRow with the offset and the count of
        every part (count 0: the part is off) and the width (hb_env_row)"""
        r = HbEnvRow()
        _check(lib().hb_env_row(self._h, ctypes.byref(r)), "hb_env_row")
        return r

    def obs_extend(self, prev_action=False, height_scan=None):
        """Appends to every observation of the env adapter, on the device (hb_env_obs_extend): prev_action - the nu entries of the action
        the env last applied (zero after a reset); height_scan=dict(offset=0.0, scale=1.0, clip=(lo, hi)) - one entry per installed ray
        (ray_configure, with a cutoff > 0), clamp(scale * (offset - d), lo, hi) with d the ray's distance, or the cutoff where nothing is
        hit.  Row layout [model nobs | prev_action | scan]; env_nobs is the new width.  Call it before anything sized by the observation
        is installed (actor, critic, Q networks, normaliser, learners); obs_extend() with nothing on removes the extension.  A call that
        is refused (HbError) changes nothing."""
        x = HbObsExt(1 if prev_action else 0, 0, 0.0, 1.0, 0.0, 0.0)
        if height_scan is not None:
            hs = dict(height_scan)
            lo, hi = hs.pop("clip", (-3.0e38, 3.0e38))
            x.height_scan, x.scan_offset, x.scan_scale, x.scan_lo, x.scan_hi = 1, float(hs.pop("offset", 0.0)), float(hs.pop("scale", 1.0)), float(lo), float(hi)
            if hs:
                raise TypeError("obs_extend: unknown height_scan option(s) %s" % sorted(hs))
        rc = lib().hb_env_obs_extend(self._h, ctypes.byref(x))
        _check(rc, "hb_env_obs_extend", "call it before an actor, critic, Q network, normaliser or learner is installed; height_scan needs rays "
               "installed with a cutoff > 0, finite parameters and clip lo <= hi" if rc == -1 else None)
        self._env_pin = None  # (the transfer record of env_step has rows of the old width)

    def default_commands(self):
        """hb_env_default_commands: an HbEnvCommands to edit and hand to commands_configure"""
        c = HbEnvCommands()
        _check(lib().hb_env_default_commands(self.model._h, ctypes.byref(c)), "hb_env_default_commands")
        return c

    def commands_configure(self, cfg=None, **kw):
        """Per-env velocity commands on the device (hb_env_commands_configure): commands_configure(vx_min=..., resample_time=..., frame=1,
        observe=1, ...) installs the defaults of hb_env_default_commands with the given fields replaced (or an HbEnvCommands as it is);
        commands_configure(None) with no fields removes them.  Every env then follows its own (vx, vy, yaw rate), drawn at every episode
        start and every resample_time seconds, rewarded by the linear and the yaw term (target_velocity is ignored), and - with observe -
        seen as the last three entries of every observation row (env_nobs grows by 3: call it before anything sized by the observation
        is installed).  A call that is refused (HbError, with the library's reason) changes nothing."""
        if cfg is None and kw:
            cfg = self.default_commands()
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("commands_configure: unknown field %r" % k)
            setattr(cfg, k, v)
        rc = lib().hb_env_commands_configure(self._h, ctypes.byref(cfg) if cfg is not None else None)
        _check(rc, "hb_env_commands_configure", lib().hb_error().decode() if rc == -1 else None)
        self._env_pin = None  # (the transfer record of env_step has rows of the old width)

    def commands(self):
        """[n_env, 3] float32: every env's current (vx, vy, yaw rate) command, behind the enqueued work (hb_env_get_commands)"""
        out = np.zeros((self.n_env, 3), dtype=np.float32)
        rc = lib().hb_env_get_commands(self._h, _ptr(out))
        _check(rc, "hb_env_get_commands", lib().hb_error().decode() if rc == -1 else None)
        return out

    def set_commands(self, cmd, mask=None):
        """Overwrites the current command of the envs of `mask` ([n_env] bool; None: all) with cmd [n_env, 3] (or [3] for all of them) -
        evaluation and teleoperation (hb_env_set_commands).  The draw counters do not move: the next scheduled draw replaces it."""
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(cmd, dtype=np.float32), (self.n_env, 3)))
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        if m is not None and m.shape != (self.n_env,):
            raise ValueError("set_commands: mask must be [n_env]")
        rc = lib().hb_env_set_commands(self._h, _ptr(c), _ptr(m))
        _check(rc, "hb_env_set_commands", lib().hb_error().decode() if rc == -1 else None)

    def default_feet(self):
        """hb_env_default_feet: an HbEnvFeet to edit (set_bodies names the bodies) and hand to feet_configure"""
        c = HbEnvFeet()
        _check(lib().hb_env_default_feet(self.model._h, ctypes.byref(c)), "hb_env_default_feet")
        return c

    def feet_configure(self, cfg=None, **kw):
        """Foot-contact terms in the env kernel (hb_env_feet_configure): feet_configure(bodies=(7, 10), penalised=(...), terminal=(...),
        w_air_time=..., observe=1, ...) installs the defaults of hb_env_default_feet with the given fields replaced (or an HbEnvFeet as
        it is); feet_configure(None) with no fields removes them.  Bodies are ids.  Every env then earns the air-time term at a touchdown,
        pays for impacts, stumbles and contacts of the penalised bodies, and its episode ends when a terminal body touches anything; with
        observe the n_feet contact flags sit in front of the command in every row (env_nobs grows by n_feet: call it before anything
        sized by the observation is installed).  The contact read-out is switched on.  A call that is refused (HbError, with the
        library's reason) changes nothing."""
        if cfg is None and kw:
            cfg = self.default_feet()
        lists = {k: kw.pop(k) for k in ("bodies", "penalised", "terminal") if k in kw}
        if lists:
            cfg.set_bodies(**lists)
        for k, v in kw.items():
            if not hasattr(cfg, k) or k.endswith("_body"):
                raise TypeError("feet_configure: unknown field %r" % k)
            setattr(cfg, k, v)
        rc = lib().hb_env_feet_configure(self._h, ctypes.byref(cfg) if cfg is not None else None)
        _check(rc, "hb_env_feet_configure", lib().hb_error().decode() if rc == -1 else None)
        self._env_pin = None  # (the transfer record of env_step has rows of the old width)

    def feet(self):
        """(t_last [n_env, n_feet] float32, contact [n_env, n_feet] uint8): the env time each foot was last evaluated in contact and the
        contact bits of the last step evaluation, behind the enqueued work (hb_env_get_feet)"""
        nf = int(lib().hb_env_feet_count(self._h))  # (the library's own count: the arrays below are never smaller than what it writes)
        t = np.zeros((self.n_env, nf), dtype=np.float32)
        c = np.zeros((self.n_env, nf), dtype=np.uint8)
        rc = lib().hb_env_get_feet(self._h, _ptr(t), _ptr(c))
        _check(rc, "hb_env_get_feet", lib().hb_error().decode() if rc == -1 else None)
        return t, c

    def env_reset(self):
        o = np.zeros((self.n_env, self.env_nobs), dtype=np.float32)
        _check(lib().hb_env_reset(self._h, _ptr(o)), "hb_env_reset")
        return o

    def env_step(self, action, n_substeps=1, copy=True, wait=True):
        """action [n_env, nu] -> (obs, reward, terminated, truncated).  The transfer buffers are page-locked and reused; the four
        outputs are one record in device and host memory, so they come back in one transfer.  copy=True (default): the returned
        arrays are fresh copies, the caller may keep them; copy=False: views of the transfer buffer, valid until the next call.
        wait=False: enqueue only (hb_env_step_async) and return None; sync(), then env_step_result()."""
        pin = getattr(self, "_env_pin", None)
        if pin is None:
            n, nobs = self.n_env, self.env_nobs
            ob, rb = n * nobs * 4, n * 4
            out = _Pinned((ob + rb + 2 * n,), np.uint8)
            pin = self._env_pin = dict(a=_Pinned((n, self.model.nu), np.float32), out=out,
                                       o=out.array[:ob].view(np.float32).reshape(n, nobs), r=out.array[ob:ob + rb].view(np.float32),
                                       te=out.array[ob + rb:ob + rb + n], tr=out.array[ob + rb + n:], off=(0, ob, ob + rb, ob + rb + n))
        a = np.asarray(action, dtype=np.float32)
        assert a.shape == (self.n_env, self.model.nu), a.shape
        if getattr(self, "_env_pending", False):  # a step enqueued with wait=False may still be reading the action buffer / writing the outputs
            self.sync()
            self._env_pending = False
        pin["a"].array[...] = a
        base, off = pin["out"].ptr, pin["off"]
        fn = lib().hb_env_step_async if wait is False else lib().hb_env_step
        _check(fn(self._h, ctypes.c_void_p(pin["a"].ptr), int(n_substeps), ctypes.c_void_p(base + off[0]), ctypes.c_void_p(base + off[1]),
                  ctypes.c_void_p(base + off[2]), ctypes.c_void_p(base + off[3])), "hb_env_step")
        if wait is False:
            self._env_pending = True
            return None
        return self.env_step_result(copy)

    def env_step_result(self, copy=True):
        """the outputs of the last env_step (after env_step(..., wait=False): call sync() first)"""
        pin = getattr(self, "_env_pin", None)
        if pin is None:
            raise HbError("env_step_result before any env_step")
        if not copy:
            return pin["o"], pin["r"], pin["te"].view(bool), pin["tr"].view(bool)
        return pin["o"].copy(), pin["r"].copy(), pin["te"].astype(bool), pin["tr"].astype(bool)

    def env_warnings(self):
        """HB_WARN_* bits every env has raised since the previous call, across in-place resets (include/hb.h: hb_env_warnings)"""
        w = np.zeros(self.n_env, dtype=np.int32)
        _check(lib().hb_env_warnings(self._h, _ptr(w)), "hb_env_warnings")
        return w

    def env_joint_torques(self):
        """[n_env, nv] qfrc_smooth + qfrc_constraint of the last physics step of the last env step (include/hb.h: hb_env_joint_torques)"""
        out = np.zeros((self.n_env, self.model.nv), dtype=np.float32)
        _check(lib().hb_env_joint_torques(self._h, _ptr(out)), "hb_env_joint_torques")
        return out

    def env_terminal_obs(self, fetch=True):
        """[n_env, nobs] observations of the states episodes ended in (include/hb.h: hb_env_terminal_obs); fetch=False only switches the
        recording on"""
        if not fetch:
            _check(lib().hb_env_terminal_obs(self._h, None), "hb_env_terminal_obs")
            return None
        out = np.zeros((self.n_env, self.env_nobs), dtype=np.float32)
        _check(lib().hb_env_terminal_obs(self._h, _ptr(out)), "hb_env_terminal_obs")
        return out

    def env_step_dev(self, action_ptr, obs_ptr, reward_ptr, terminated_ptr, truncated_ptr, n_substeps=1):
        """hb_env_step_dev: device pointers (e.g. torch tensors' data_ptr()), asynchronous on the batch's stream: a policy on
        the same GPU never sees the host.  Work the caller enqueued on other streams must be finished (or ordered before
        this call through hb_batch_stream); call sync() before reading the outputs from another stream."""
        _check(lib().hb_env_step_dev(self._h, ctypes.c_void_p(action_ptr), int(n_substeps), ctypes.c_void_p(obs_ptr), ctypes.c_void_p(reward_ptr),
                                     ctypes.c_void_p(terminated_ptr), ctypes.c_void_p(truncated_ptr)), "hb_env_step_dev")

    # ---- policy in the loop (BASELINE config 4)
    def set_policy_mlp(self, weights, biases, activation="tanh"):
        """weights[l]: [in, out] float32 (transpose of torch.nn.Linear.weight); `activation` ("tanh", "relu", "elu") after every hidden
        layer, tanh after the last."""
        act = _activation(activation)
        ws, bs, csz, wp, bp = _mlp_args("set_policy_mlp", weights, biases)
        _check(lib().hb_policy_set_mlp(self._h, len(ws), csz, wp, bp), "hb_policy_set_mlp")
        if act != ACT_TANH:  # (what hb_policy_set_mlp installs)
            self.mlp_set_activation(NET_POLICY, act)

    def mlp_set_activation(self, net, activation):
        """hb_mlp_set_activation: the activation behind the hidden layers of the installed network `net` ("policy", "actor", "critic",
        "q1", "q2" or the NET_* value): "tanh", "relu", "elu" or the ACT_* value.  Every installation starts with tanh; a change destroys
        a learner that trains the network, as installing it again does."""
        rc = lib().hb_mlp_set_activation(self._h, _net(net), _activation(activation))
        _check(rc, "hb_mlp_set_activation", "needs an installed network of that kind")

    def mlp_activation(self, net):
        """The activation behind the hidden layers of the installed network `net` ("policy", "actor", "critic", "q1", "q2" or NET_*):
        "tanh", "relu" or "elu"."""
        rc = lib().hb_mlp_get_activation(self._h, _net(net))
        _check(min(rc, 0), "hb_mlp_get_activation", "needs an installed network of that kind")
        return {v: k for k, v in ACTIVATIONS.items()}[rc]

    def policy_eval(self):
        out = np.zeros((self.n_env, self.model.nu), dtype=np.float32)
        _check(lib().hb_policy_eval(self._h, _ptr(out)), "hb_policy_eval")
        return out

    def rollout_policy(self, T, qpos_out_ptr=None):
        _check(lib().hb_rollout_policy(self._h, int(T), ctypes.c_void_p(qpos_out_ptr or 0)), "hb_rollout_policy")

    # ---- actor and rollout collection (include/hb.h: hb_actor_set_mlp, hb_env_collect_dev)
    def actor_set(self, sizes, weights, biases, head="gaussian", log_std=None, seed=0, deterministic=False, activation="tanh"):
        """Installs the sampling actor.  sizes: [nobs, hidden..., nu] (head "squashed": ..., 2 nu); weights[l]: [sizes[l], sizes[l+1]]
        float32 - the TRANSPOSE of torch.nn.Linear.weight -, biases[l]: [sizes[l+1]]; `activation` ("tanh", "relu", "elu") after every hidden layer.  head: "deterministic"
        (tanh output, no sampling), "gaussian" (linear mean, state-independent log_std [nu]: SB3 PPO / A2C) or "squashed" (linear
        mean | log_std, clamped to [-20, 2], tanh of the sample: SB3 SAC), or the ACTOR_* value.  At most four layers of width <= 256."""
        head = ACTOR_HEADS[head] if isinstance(head, str) else int(head)
        act = _activation(activation)
        ws, bs, csz, wp, bp = _mlp_args("actor_set", weights, biases, sizes)
        cfg = HbActorConfig()
        cfg.head, cfg.seed, cfg.deterministic = head, int(seed) & 0xFFFFFFFF, int(bool(deterministic))
        if log_std is not None:
            ls = np.broadcast_to(np.asarray(log_std, dtype=np.float32), (self.model.nu,))
            if len(ls) > 32:
                raise ValueError("actor_set: log_std holds at most 32 actuators")
            cfg.log_std[:len(ls)] = [float(x) for x in ls]
        rc = lib().hb_actor_set_mlp(self._h, len(ws), csz, wp, bp, ctypes.byref(cfg))
        _check(rc, "hb_actor_set_mlp", "a layer wider than 256: the actor is one fused kernel, there is no layer-by-layer path" if rc == -4 else
               "sizes must run from nobs to nu (squashed: 2 nu) over 1..4 layers, nu <= 32, log_std finite" if rc == -1 else None)
        self.actor_head = head
        if act != ACT_TANH:  # (what hb_actor_set_mlp installs)
            self.mlp_set_activation(NET_ACTOR, act)

    def env_collect_dev(self, T, n_substeps=1, obs=None, action=None, mean=None, log_std=None, eps=None, reward=None, terminated=None,
                        truncated=None, terminal_obs=None):
        """hb_env_collect_dev: T env steps with the installed actor in the loop, enqueued on the batch's stream.  Device pointers (ints, e.g.
        torch tensors' data_ptr()) of the tapes; obs [T + 1, n_env, nobs] (row 0 is the input) and action [T, n_env, nu] are required."""
        out = HbCollectOut(obs, action, mean, log_std, eps, reward, terminated, truncated, terminal_obs)
        rc = lib().hb_env_collect_dev(self._h, int(T), int(n_substeps), ctypes.byref(out))
        _check(rc, "hb_env_collect_dev", "needs T >= 1, n_substeps >= 1, obs and action tapes, an installed actor (actor_set), and a log_std "
               "tape only with the squashed head" if rc == -1 else None)

    # ---- critic and the PPO buffer over a collection's tapes (include/hb.h: hb_critic_set_mlp, hb_collect_gae_dev)
    def critic_set(self, sizes, weights, biases, activation="tanh"):
        """Installs the critic.  sizes: [nobs, hidden..., 1]; weights[l]: [sizes[l], sizes[l+1]] float32 - the TRANSPOSE of
        torch.nn.Linear.weight -, biases[l]: [sizes[l+1]]; `activation` ("tanh", "relu", "elu") after every hidden layer, the last layer linear.  At most
        four layers of width <= 256.  Independent of the actor and of the policy MLP."""
        act = _activation(activation)
        ws, bs, csz, wp, bp = _mlp_args("critic_set", weights, biases, sizes)
        rc = lib().hb_critic_set_mlp(self._h, len(ws), csz, wp, bp)
        _check(rc, "hb_critic_set_mlp", "a layer wider than 256: the critic is one fused kernel, there is no layer-by-layer path" if rc == -4 else
               "sizes must run from nobs to 1 over 1..4 layers" if rc == -1 else None)
        if act != ACT_TANH:  # (what hb_critic_set_mlp installs)
            self.mlp_set_activation(NET_CRITIC, act)

    def collect_gae_dev(self, T, gamma, lam, bootstrap_truncated=True, *, obs=None, action=None, mean=None, log_std=None, eps=None, reward=None,
                        terminated=None, truncated=None, terminal_obs=None, value=None, terminal_value=None, log_prob=None, advantage=None, returns=None):
        """hb_collect_gae_dev: critic values, log-probabilities and GAE(gamma, lam) advantages / returns over the T-step tapes of a collection,
        enqueued on the batch's stream.  Device pointers (ints, e.g. torch tensors' data_ptr()): the tapes as env_collect_dev takes them, and
        the outputs value [T + 1, n_env], terminal_value, log_prob, advantage, returns [T, n_env], each optional (at least one)."""
        tapes = HbCollectOut(obs, action, mean, log_std, eps, reward, terminated, truncated, terminal_obs)
        cfg = HbGaeConfig(float(gamma), float(lam), int(bool(bootstrap_truncated)))
        out = HbGaeOut(value, terminal_value, log_prob, advantage, returns)
        rc = lib().hb_collect_gae_dev(self._h, int(T), ctypes.byref(tapes), ctypes.byref(cfg), ctypes.byref(out))
        _check(rc, "hb_collect_gae_dev", "needs T >= 1, gamma and lam in [0, 1], at least one output, the tapes each output reads, a critic "
               "(critic_set) for the value outputs and a sampling actor (actor_set, not the deterministic head) for log_prob" if rc == -1 else None)

    # ---- the PPO learner (include/hb.h: hb_learner_*, hb_ppo_*)
    _PPO_WHY = "needs a learner (learner_create), the five tapes, 1 <= mb, and first + mb <= n_rows without an index"

    @staticmethod
    def _learn_config(struct, default_fn, what, cfg, base, convert):
        """A learner's config struct: base's values, or the library's defaults (default_fn: the C function's name), and on top of them
        cfg's, each set by convert(c, k, v)."""
        c = struct()
        if base is not None:
            ctypes.memmove(ctypes.byref(c), ctypes.byref(base), ctypes.sizeof(c))
        else:
            _check(getattr(lib(), default_fn)(ctypes.byref(c)), default_fn)
        names = dict(struct._fields_)
        for k, v in cfg.items():
            if k not in names:
                raise ValueError("%s: unknown hyper-parameter %r (one of %s)" % (what, k, ", ".join(names)))
            convert(c, k, v)
        return c

    # a learner's records (both keep them in LearnerCore): fn is the C function, name what _check calls it, why its refusal's text
    def _learn_count(self, fn, name, why):
        n = fn(self._h)
        _check(0 if n >= 0 else int(n), name, why)
        return int(n)

    def _learn_download(self, n, fn, name):
        out = np.zeros(n, dtype=np.float32)
        _check(fn(self._h, _ptr(out), out.size), name)
        return out

    def _learn_upload(self, flat, fn, name, why):
        a = np.ascontiguousarray(flat, dtype=np.float32)
        _check(fn(self._h, _ptr(a), a.size if a.ndim == 1 else -1), name, why)

    def _learn_get_state(self, n, fn, name, *more):
        """(params, m, v, t); more: the arrays the C function fills behind the three records, each passed with its size"""
        p, m, v = (np.zeros(n, dtype=np.float32) for _ in range(3))
        t = ctypes.c_longlong()
        _check(fn(self._h, _ptr(p), _ptr(m), _ptr(v), n, *[x for a in more for x in (_ptr(a), a.size)], ctypes.byref(t)), name)
        return p, m, v, int(t.value)

    def _learn_set_state(self, state, fn, name, why, *more):
        """more: the keys of state the C function reads behind the three records"""
        p, m, v, *rest = (np.ascontiguousarray(state[k], dtype=np.float32) for k in ("params", "m", "v") + more)
        n = p.size if p.ndim == 1 and p.shape == m.shape == v.shape else -1
        _check(fn(self._h, _ptr(p), _ptr(m), _ptr(v), n, *[x for a in rest for x in (_ptr(a), a.size if a.ndim == 1 else -1)], int(state["t"])),
               name, why)

    def _ppo_config(self, what, cfg, base=None):
        def convert(c, k, v):
            setattr(c, k, int(bool(v)) if k == "normalize_advantage" else float(v))
        return self._learn_config(HbPpoConfig, "hb_ppo_default_config", what, cfg, base, convert)

    def learner_create(self, **cfg):
        """Creates the PPO learner over the installed actor (Gaussian head) and critic: they become the trainable parameters, with Adam
        moments of zero and t = 0.  cfg: clip_range, ent_coef, vf_coef, max_grad_norm, normalize_advantage, lr, beta1, beta2, eps
        (stable-baselines3's defaults where not given)."""
        c = self._ppo_config("learner_create", cfg)
        rc = lib().hb_learner_create(self._h, ctypes.byref(c))
        _check(rc, "hb_learner_create", "the learner trains the Gaussian head only: the deterministic head has no density, and the squashed head "
               "(SAC's actor) belongs to an off-policy learner" if rc == -4 else
               "needs an actor and a critic, clip_range > 0, betas in [0, 1), lr >= 0, eps > 0, all finite" if rc == -1 else None)
        self._ppo_cfg = c

    def learner_configure(self, **cfg):
        """Changes hyper-parameters (schedules of lr or clip_range) and keeps parameters, moments and t; those not named stay."""
        c = self._ppo_config("learner_configure", cfg, getattr(self, "_ppo_cfg", None))
        _check(lib().hb_learner_configure(self._h, ctypes.byref(c)), "hb_learner_configure",
               "needs a learner, clip_range > 0, betas in [0, 1), lr >= 0, eps > 0, all finite")
        self._ppo_cfg = c

    def learner_destroy(self):
        _check(lib().hb_learner_destroy(self._h), "hb_learner_destroy", "no learner")

    def learner_param_count(self):
        return self._learn_count(lib().hb_learner_param_count, "hb_learner_param_count", "no learner")

    def learner_params(self):
        """the parameters as the flat float32 record (ppo_split gives the per-layer arrays)"""
        return self._learn_download(self.learner_param_count(), lib().hb_learner_get_params, "hb_learner_get_params")

    def learner_set_params(self, flat):
        self._learn_upload(flat, lib().hb_learner_set_params, "hb_learner_set_params", "needs a learner and a flat record of learner_param_count() values")

    def learner_grads(self):
        return self._learn_download(self.learner_param_count(), lib().hb_learner_get_grads, "hb_learner_get_grads")

    def learner_state(self):
        """{"params", "m", "v": flat float32 records, "t": Adam's step count}: checkpoint of the learner"""
        p, m, v, t = self._learn_get_state(self.learner_param_count(), lib().hb_learner_get_state, "hb_learner_get_state")
        return {"params": p, "m": m, "v": v, "t": t}

    def learner_set_state(self, state):
        self._learn_set_state(state, lib().hb_learner_set_state, "hb_learner_set_state",
                              "needs a learner, three flat records of learner_param_count() values and t >= 0")

    def learner_grad_dev(self):
        """(device pointer, count) of the gradient buffer, flat layout: what a multi-GPU caller all-reduces between ppo_grad_dev and ppo_adam_dev"""
        p, n = ctypes.c_void_p(), ctypes.c_longlong()
        _check(lib().hb_learner_grad_dev(self._h, ctypes.byref(p), ctypes.byref(n)), "hb_learner_grad_dev", "no learner")
        return p.value, int(n.value)

    def ppo_grad_dev(self, obs, action, old_log_prob, advantage, returns, n_rows, mb, index=None, first=0, stats=None):
        """hb_ppo_grad_dev: loss, statistics and gradients of one minibatch, enqueued on the batch's stream.  Device pointers of the
        flattened tapes ([n_rows, ...]); index: device int32 [mb], or None for rows first .. first + mb - 1; stats: device float32 [16]."""
        rows = HbPpoRows(obs, action, old_log_prob, advantage, returns, index, int(n_rows), int(first), int(mb))
        _check(lib().hb_ppo_grad_dev(self._h, ctypes.byref(rows), ctypes.c_void_p(stats or 0)), "hb_ppo_grad_dev", self._PPO_WHY)

    def ppo_adam_dev(self, stats=None):
        """hb_ppo_adam_dev: global-norm clipping and the Adam step on the gradient buffer; the next collection runs the new parameters."""
        _check(lib().hb_ppo_adam_dev(self._h, ctypes.c_void_p(stats or 0)), "hb_ppo_adam_dev", "no learner")

    def ppo_minibatch_dev(self, obs, action, old_log_prob, advantage, returns, n_rows, mb, index=None, first=0, stats=None):
        """hb_ppo_minibatch_dev: ppo_grad_dev, then ppo_adam_dev."""
        rows = HbPpoRows(obs, action, old_log_prob, advantage, returns, index, int(n_rows), int(first), int(mb))
        _check(lib().hb_ppo_minibatch_dev(self._h, ctypes.byref(rows), ctypes.c_void_p(stats or 0)), "hb_ppo_minibatch_dev", self._PPO_WHY)

    # ---- the Q networks and the SAC learner (include/hb.h: hb_q_*, hb_sac_*)
    def q_set(self, k, sizes, weights, biases, activation="tanh"):
        """Installs Q network k (0 or 1).  sizes: [nobs + nu, hidden..., 1] - the input row is obs | action; weights[l]: [sizes[l],
        sizes[l+1]] float32 - the TRANSPOSE of torch.nn.Linear.weight -, biases[l]: [sizes[l+1]]; `activation` ("tanh", "relu", "elu") after every hidden layer,
        the last layer linear; Q1 and Q2 of a SAC learner share it.  At most four layers of width <= 256.  Destroys a SAC learner of this
        batch."""
        act = _activation(activation)
        ws, bs, csz, wp, bp = _mlp_args("q_set", weights, biases, sizes)
        rc = lib().hb_q_set_mlp(self._h, int(k), len(ws), csz, wp, bp)
        _check(rc, "hb_q_set_mlp", "a layer wider than 256: the Q network is one fused kernel, there is no layer-by-layer path" if rc == -4 else
               "k is 0 or 1, sizes must run from nobs + nu to 1 over 1..4 layers" if rc == -1 else None)
        if act != ACT_TANH:  # (what hb_q_set_mlp installs)
            self.mlp_set_activation(NET_Q1 + int(k), act)

    def q_values_dev(self, obs, action, n_rows, q1=None, q2=None):
        """hb_q_values_dev: Q1 and Q2 over n_rows rows obs [n_rows, nobs] | action [n_rows, nu] into q1, q2 [n_rows] (device pointers,
        at least one), one launch on the batch's stream."""
        rc = lib().hb_q_values_dev(self._h, ctypes.c_void_p(obs or 0), ctypes.c_void_p(action or 0), int(n_rows), ctypes.c_void_p(q1 or 0), ctypes.c_void_p(q2 or 0))
        _check(rc, "hb_q_values_dev", "needs obs, action, n_rows >= 1 and an output whose Q network is installed (q_set)")

    _SAC_WHY = "needs a SAC learner (sac_create), the five tapes, 1 <= mb, first + mb <= n_rows without an index, and both eps with eps_given"
    _SAC_CFG_WHY = ("gamma and tau in [0, 1], learning rates >= 0, betas in [0, 1), eps > 0, ent_coef_init > 0, "
                    "target_update_interval >= 1, all finite")

    def _sac_config(self, what, cfg, base=None):
        names = dict(HbSacConfig._fields_)

        def convert(c, k, v):
            if k == "target_entropy" and "target_entropy_auto" not in cfg:
                c.target_entropy_auto = 0
            setattr(c, k, int(v) if names[k] in (ctypes.c_int, ctypes.c_uint) else float(v))
        return self._learn_config(HbSacConfig, "hb_sac_default_config", what, cfg, base, convert)

    def sac_create(self, **cfg):
        """Creates the SAC learner over the installed actor (squashed head) and Q networks: they become the trainable parameters, the
        targets are made as copies of Q1 and Q2, log_ent_coef = log(ent_coef_init), Adam moments of zero and t = 0.  cfg: the fields of
        hb_sac_config (stable-baselines3's defaults where not given; a target_entropy switches target_entropy_auto off)."""
        c = self._sac_config("sac_create", cfg)
        rc = lib().hb_sac_create(self._h, ctypes.byref(c))
        _check(rc, "hb_sac_create", "the SAC learner trains the squashed head only (actor_set(head=\"squashed\")); the Gaussian head is the "
               "PPO learner's" if rc == -4 else "needs an actor and two Q networks of equal sizes (q_set); " + self._SAC_CFG_WHY if rc == -1 else None)
        self._sac_cfg = c

    def sac_configure(self, **cfg):
        """Changes hyper-parameters and keeps parameters, moments, targets and t; those not named stay."""
        c = self._sac_config("sac_configure", cfg, getattr(self, "_sac_cfg", None))
        _check(lib().hb_sac_configure(self._h, ctypes.byref(c)), "hb_sac_configure", "needs a SAC learner; " + self._SAC_CFG_WHY)
        self._sac_cfg = c

    def sac_destroy(self):
        _check(lib().hb_sac_destroy(self._h), "hb_sac_destroy", "no SAC learner")

    def sac_param_count(self):
        return self._learn_count(lib().hb_sac_param_count, "hb_sac_param_count", "no SAC learner")

    def sac_target_count(self):
        return self._learn_count(lib().hb_sac_target_count, "hb_sac_target_count", "no SAC learner")

    def sac_params(self):
        """the parameters as the flat float32 record (sac_split gives the per-layer arrays)"""
        return self._learn_download(self.sac_param_count(), lib().hb_sac_get_params, "hb_sac_get_params")

    def sac_set_params(self, flat):
        self._learn_upload(flat, lib().hb_sac_set_params, "hb_sac_set_params", "needs a SAC learner and a flat record of sac_param_count() values")

    def sac_grads(self):
        """the gradients the last step used, flat layout"""
        return self._learn_download(self.sac_param_count(), lib().hb_sac_get_grads, "hb_sac_get_grads")

    def sac_state(self):
        """{"params", "m", "v": flat float32 records, "targets": the targets' record (Q1' then Q2'), "t": the step count}: checkpoint"""
        tg = np.zeros(self.sac_target_count(), dtype=np.float32)
        p, m, v, t = self._learn_get_state(self.sac_param_count(), lib().hb_sac_get_state, "hb_sac_get_state", tg)
        return {"params": p, "m": m, "v": v, "targets": tg, "t": t}

    def sac_set_state(self, state):
        self._learn_set_state(state, lib().hb_sac_set_state, "hb_sac_set_state",
                              "needs a SAC learner, three flat records of sac_param_count() values, sac_target_count() targets and t >= 0", "targets")

    def sac_step_dev(self, obs, action, reward, next_obs, done, n_rows, mb, index=None, first=0, eps_pi=None, eps_next=None, eps_given=False,
                     stats=None):
        """hb_sac_step_dev: one SAC gradient step on a minibatch, enqueued on the batch's stream.  Device pointers of the replay rows
        ([n_rows, ...]; done uint8); index: device int32 [mb], or None for rows first .. first + mb - 1; eps_pi, eps_next: device float32
        [mb, nu], written with the draws (eps_given False) or read (True); stats: device float32 [16] (SAC_STATS)."""
        rows = HbSacRows(obs, action, reward, next_obs, done, index, int(n_rows), int(first), int(mb), eps_pi, eps_next, int(bool(eps_given)))
        _check(lib().hb_sac_step_dev(self._h, ctypes.byref(rows), ctypes.c_void_p(stats or 0)), "hb_sac_step_dev", self._SAC_WHY)

    # ---- running observation / reward normalisation and episode statistics (include/hb.h: hb_norm_*)
    _NORM_WHY = "needs a normaliser (norm_configure) and the required device pointers"

    def norm_configure(self, norm_obs=True, norm_reward=True, training=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        """Installs the normaliser (VecNormalize over a VecMonitor, stable-baselines3's defaults); a later call changes the switches and
        constants and keeps the statistics (training=False: evaluation).  norm_configure(None) removes it."""
        if norm_obs is None:
            _check(lib().hb_norm_configure(self._h, None), "hb_norm_configure")
            return
        cfg = HbNormConfig(int(bool(norm_obs)), int(bool(norm_reward)), int(bool(training)), float(clip_obs), float(clip_reward), float(gamma), float(epsilon))
        rc = lib().hb_norm_configure(self._h, ctypes.byref(cfg))
        _check(rc, "hb_norm_configure", "clip_obs, clip_reward and epsilon must be finite and positive, gamma in [0, 1]" if rc == -1 else
               "more than 240 observations" if rc == -4 else None)

    def norm_stats(self):
        """the flat fp64 record obs_mean[nobs] | obs_var[nobs] | obs_count | ret_mean | ret_var | ret_count (hb_norm_get_stats)"""
        out = np.zeros(2 * self.env_nobs + 4, dtype=np.float64)
        _check(lib().hb_norm_get_stats(self._h, _ptr(out)), "hb_norm_get_stats", "no normaliser configured")
        return out

    def norm_set_stats(self, record):
        a = np.ascontiguousarray(record, dtype=np.float64)
        if a.shape != (2 * self.env_nobs + 4,):
            raise ValueError("norm_set_stats: the record holds 2 nobs + 4 values")
        _check(lib().hb_norm_set_stats(self._h, _ptr(a)), "hb_norm_set_stats", "needs a normaliser, finite values, and no negative var or count")

    def norm_env(self):
        """(disc_return [n_env] f64, ep_return [n_env] f64, ep_length [n_env] i32): the per-env accumulators (hb_norm_get_env)"""
        ret, er, el = np.zeros(self.n_env), np.zeros(self.n_env), np.zeros(self.n_env, dtype=np.int32)
        _check(lib().hb_norm_get_env(self._h, _ptr(ret), _ptr(er), _ptr(el)), "hb_norm_get_env", "no normaliser configured")
        return ret, er, el

    def norm_episode_totals(self):
        """[episodes finished, sum of returns, sum of squared returns, sum of lengths] since the normaliser was installed"""
        out = np.zeros(4, dtype=np.float64)
        _check(lib().hb_norm_episode_totals(self._h, _ptr(out)), "hb_norm_episode_totals", "no normaliser configured")
        return out

    def norm_step_dev(self, obs_in, obs_out, reward_in, terminated, truncated, reward_out=None, terminal_obs_in=None, terminal_obs_out=None,
                      ep_return_out=None, ep_length_out=None):
        """hb_norm_step_dev: one VecNormalize / VecMonitor step over the batch's rows on its stream; device pointers, in place allowed."""
        io = HbNormIo(obs_in, obs_out, reward_in, reward_out, terminated, truncated, terminal_obs_in, terminal_obs_out, ep_return_out, ep_length_out)
        _check(lib().hb_norm_step_dev(self._h, ctypes.byref(io)), "hb_norm_step_dev", self._NORM_WHY)

    def norm_reset_dev(self, obs_in, obs_out):
        """hb_norm_reset_dev: VecNormalize.reset on the observations hb_env_reset returned (device pointers)."""
        _check(lib().hb_norm_reset_dev(self._h, ctypes.c_void_p(obs_in), ctypes.c_void_p(obs_out)), "hb_norm_reset_dev", self._NORM_WHY)

    def norm_obs_dev(self, in_ptr, out_ptr, n_rows):
        """hb_norm_obs_dev: normalize_obs on n_rows rows with the current statistics, no update."""
        _check(lib().hb_norm_obs_dev(self._h, ctypes.c_void_p(in_ptr), ctypes.c_void_p(out_ptr), int(n_rows)), "hb_norm_obs_dev", self._NORM_WHY)

    def env_collect_norm_dev(self, T, n_substeps=1, obs=None, action=None, mean=None, log_std=None, eps=None, reward=None, terminated=None,
                             truncated=None, terminal_obs=None, raw_obs=None, raw_reward=None, ep_return=None, ep_length=None):
        """hb_env_collect_norm_dev: env_collect_dev with the normaliser behind every env step; row 0 of obs is given normalised.  The aux
        tapes raw_obs [T, n_env, nobs], raw_reward, ep_return (float32) and ep_length (int32) [T, n_env] are optional."""
        out = HbCollectOut(obs, action, mean, log_std, eps, reward, terminated, truncated, terminal_obs)
        aux = HbNormTapes(raw_obs, raw_reward, ep_return, ep_length)
        rc = lib().hb_env_collect_norm_dev(self._h, int(T), int(n_substeps), ctypes.byref(out), ctypes.byref(aux))
        _check(rc, "hb_env_collect_norm_dev", "needs what env_collect_dev needs and a normaliser (norm_configure)" if rc == -1 else None)

    # ---- device buffers / timing helpers (no HIP headers or torch needed on the caller's side)
    def dev_alloc(self, nbytes):
        p = lib().hb_dev_alloc(self._h, int(nbytes))
        if not p:
            raise HbError("hb_dev_alloc(%d) failed" % nbytes)
        return p

    def dev_free(self, p):
        lib().hb_dev_free(self._h, ctypes.c_void_p(p))

    def to_dev(self, p, arr):
        a = np.ascontiguousarray(arr)
        _check(lib().hb_memcpy_h2d(self._h, ctypes.c_void_p(p), _ptr(a), a.nbytes), "hb_memcpy_h2d")

    def from_dev(self, p, shape, dtype=np.float32):
        out = np.zeros(shape, dtype=dtype)
        _check(lib().hb_memcpy_d2h(self._h, _ptr(out), ctypes.c_void_p(p), out.nbytes), "hb_memcpy_d2h")
        return out

    def halton_ctrl_dev(self, T, t0, env_offset, out_ptr):
        _check(lib().hb_halton_ctrl_dev(self._h, int(T), int(t0), int(env_offset), ctypes.c_void_p(out_ptr)), "hb_halton_ctrl_dev")

    def timer_start(self):
        _check(lib().hb_timer_start(self._h), "hb_timer_start")

    def timer_stop(self):
        ms = ctypes.c_float()
        _check(lib().hb_timer_stop(self._h, ctypes.byref(ms)), "hb_timer_stop")
        return ms.value

    def step_timing(self, enable=True):
        _check(lib().hb_step_timing(self._h, int(enable)), "hb_step_timing")

    def step_timing_read(self):
        us, n = ctypes.c_float(), ctypes.c_int()
        _check(lib().hb_step_timing_read(self._h, ctypes.byref(us), ctypes.byref(n)), "hb_step_timing_read")
        return us.value, n.value

/* hb.h — C-ABI of the MI355X batched humanoid physics-step / rollout engine (libhb.so).
 *
 * Drop-in boundary for the reference's physics-step path.  Every entry point
 * cites the reference interface it replaces; paths are relative to the reference repository
 * (mcgill-robotics/Humanoid-MuJoCo), MuJoCo C API = simulation/mujoco/include/mujoco/mujoco.h.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in any signature.
 *   - every function returns an int status (HB_OK == 0, negative = error) or a handle
 *     (NULL on failure, message in the caller's err buffer).  Nothing aborts the process
 *     (the reference's mju_error would, mujoco.h:810).
 *   - "env-major" arrays are [n_env][width], row e belonging to environment e.
 *   - *_dev variants take DEVICE pointers (hipMalloc / torch tensor data_ptr) on the batch's
 *     device and enqueue on the batch's stream without synchronising; the plain variants take
 *     HOST pointers, copy, and synchronise before returning.
 *   - there is no CPU backend: hb_batch_create fails (HB_ENODEVICE) without a HIP device.
 */
#ifndef HB_H_
#define HB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_OK 0
#define HB_EINVAL (-1)    /* bad argument */
#define HB_ENODEVICE (-2) /* no usable HIP device / HIP call failed */
#define HB_ENOMEM (-3)
#define HB_EUNSUPPORTED (-4)

/* hb_options.integrator (mjtIntegrator, mjmodel.h:138-143) */
#define HB_INT_EULER 0 /* mjINT_EULER */
#define HB_INT_RK4 1   /* mjINT_RK4 */
#define HB_EIO (-5)

/* per-env status bits, the batched counterpart of mjData.warning[] (mjdata.h:54-65,185) */
#define HB_WARN_CONTACTFULL (1 << 1) /* mjWARN_CONTACTFULL: contact buffer overflow, extras dropped */
#define HB_WARN_CNSTRFULL (1 << 2)   /* mjWARN_CNSTRFULL: constraint rows overflow, extras dropped */
#define HB_WARN_BADQPOS (1 << 4)     /* mjWARN_BADQPOS: NaN/huge qpos, env was reset (mujoco.h:301) */
#define HB_WARN_BADQVEL (1 << 5)     /* mjWARN_BADQVEL (mujoco.h:304) */
#define HB_WARN_BADQACC (1 << 6)     /* mjWARN_BADQACC (mujoco.h:307) */

/* state specification bits — identical to mjtState (mjdata.h:27-50); hb_get_state/hb_set_state
 * concatenate the selected components per env in ascending bit order, as mj_getState does. */
#define HB_STATE_TIME (1 << 0)
#define HB_STATE_QPOS (1 << 1)
#define HB_STATE_QVEL (1 << 2)
#define HB_STATE_WARMSTART (1 << 4)
#define HB_STATE_CTRL (1 << 5)
#define HB_STATE_XFRC_APPLIED (1 << 7)
#define HB_STATE_PHYSICS (HB_STATE_QPOS | HB_STATE_QVEL)
#define HB_STATE_INTEGRATION (HB_STATE_TIME | HB_STATE_QPOS | HB_STATE_QVEL | HB_STATE_WARMSTART)

typedef struct hb_model hb_model; /* immutable compiled model; shareable across batches/devices */
typedef struct hb_batch hb_batch; /* n_env independent simulations resident on one GPU */

/* The fields of mjOption this engine honours (mjmodel.h:403-445). */
typedef struct hb_options {
  double timestep;
  double gravity[3];
  double impratio;
  double tolerance;  /* solver early-exit threshold on the scaled cost improvement (Newton: also on the scaled gradient) */
  int iterations;    /* PGS sweep cap / Newton iteration cap */
  int solver;        /* 0 = PGS (mjSOL_PGS), 2 = Newton (mjSOL_NEWTON, the reference's default); CG is not implemented */
  int cone;          /* 0 = pyramidal; the only cone implemented */
  int integrator;    /* HB_INT_EULER (semi-implicit, implicit joint damping) or HB_INT_RK4 (models that step in one kernel: see hb_step);
                      * implicit (2) and implicitfast (3) are not implemented */
  int disableflags;  /* mjtDisableBit (mjmodel.h:50-68).  Bit 2 (mjDSBL_FRICTIONLOSS, <flag frictionloss="disable"/>): the joints'
                      * frictionloss has no rows, and the model steps in the kernels of a model without friction loss.  Bit 1
                      * (mjDSBL_EQUALITY, <flag equality="disable"/>): likewise for the model's equality constraints */
  int ls_iterations;   /* Newton: cap on line-search evaluations per iteration (mjOption.ls_iterations, mjmodel.h:434) */
  double ls_tolerance; /* Newton: line-search slope tolerance relative to `tolerance` (mjmodel.h:411) */
} hb_options;

/* sizes a caller needs to allocate buffers (mjModel.nq/nv/nu/..., mjmodel.h:560-620) */
typedef struct hb_sizes {
  int nq, nv, nu, nbody, njnt, ngeom, ntendon, nM, nkey, npair;
  int nobs;     /* width of the env observation (hb_get_obs) */
  int ncon_max; /* contact capacity per env */
  int nefc_max; /* constraint-row capacity per env */
} hb_sizes;

/* ---- model --------------------------------------------------------------------------------- */

/* Replaces mj_loadXML (mujoco.h:103) / mj_loadModel (mujoco.h:163).  `path` ends in ".xml"
 * (MJCF subset, compiled on the host) or ".hbm" (this engine's compiled text model).
 * Geoms that collide: plane, sphere, capsule, box (mjGEOM_BOX, size = three half extents), mesh (through its convex hull) and height
 * field; a cylinder only as a non-colliding marker.  A model with a colliding box steps in the kernels of the general collision path
 * (hb_last_kernel: hb_box_* / the staged step's fast pass), as a mesh model does: at most 28 dofs, Euler, no friction loss or equality
 * rows.  plane - box (up to four corner contacts) and sphere - box are MuJoCo's analytic routines; capsule - box, box - box, box - mesh
 * and height field - box go through the portal search, and so does box - box unless hb_model_box_manifold(m, 1) selects this engine's
 * clipped manifold of up to eight contacts.  DEVIATION from MuJoCo: capsule - box gives ONE contact per pair where mjc_CapsuleBox gives
 * up to 2, and so does box - box in mode 0 where mjc_BoxBox gives up to 8. */
hb_model* hb_model_load(const char* path, char* err, int err_sz);
/* Replaces mj_loadXML with an in-memory string (mjVFS use in the reference). */
hb_model* hb_model_load_xml_string(const char* xml, char* err, int err_sz);
/* Replaces mj_saveModel (mujoco.h:159). */
int hb_model_save(const hb_model* m, const char* path, char* err, int err_sz);
/* Replaces mj_deleteModel (mujoco.h:166). */
void hb_model_free(hb_model* m);
int hb_model_sizes(const hb_model* m, hb_sizes* out);
/* mjOption get/set (model->opt in the reference, e.g. simulation/cpu_env.py:87 sets
 * opt.timestep).  Options are copied into a batch at hb_batch_create. */
int hb_options_get(const hb_model* m, hb_options* out);
int hb_options_set(hb_model* m, const hb_options* in);
/* The order in which mj_collision emits contacts = the order of the model's candidate geom pairs.  Physically irrelevant, but PGS cut at a
 * finite sweep count depends on it (up to 4e-2 in qacc on the benchmark workload at 50 sweeps, 3e-14 for converged Newton:
 * profiles/r03_contact_order.txt).  order 1 (what the MJCF compiler writes): body pairs ascending, then the geoms of the first and of the
 * second body - MuJoCo's collision driver enumerates body pairs, then the geoms inside a pair (the documented structure of
 * engine_collision_driver; the pinned MuJoCo 3.1.4 is not in the reference tree to check the details against); order 0: geom pairs
 * ascending (this engine's rounds 1-3, and .hbm files written then).  -1: query.  Returns the order in force.  Call before
 * hb_batch_create. */
int hb_model_pair_order(hb_model* m, int order);
/* The box - box manifold.  mode 1: every box - box candidate pair is collided by an analytic routine of THIS ENGINE'S OWN DEFINITION (not a
 * restatement of mjc_BoxBox; DESIGN.md 3.6a gives it in full): fifteen separating axes, then either one edge - edge contact or the
 * incident face clipped against the reference face - 0 to 8 contacts per pair in a fixed order (incident corners inside the reference
 * face, reference corners inside the incident face, edge crossings), normal from geom 1 to geom 2, each an ordinary contact of the pair;
 * no portal search.  mode 0 (the default, and every .hbm without the optional record box_manifold): one contact through the portal
 * search, bit for bit what the engine did before the mode existed.  -1: query.  Returns the mode in force; any other mode is
 * HB_EINVAL with its reason in hb_error().  The mode is saved in the .hbm only when it is 1.  A model without a box - box candidate pair
 * accepts the mode and steps exactly as without it.  Capsule - box stays one contact.  Call before hb_batch_create. */
int hb_model_box_manifold(hb_model* m, int mode);
/* mj_name2id (mujoco.h:516) for kind in {"body","joint","geom","actuator","tendon","key","equality"}; -1 if absent. */
int hb_model_name2id(const hb_model* m, const char* kind, const char* name);
/* mj_id2name for the same kinds: copies the name (empty for an unnamed element) into out[cap], zero-terminated; returns its length,
 * HB_EINVAL for an unknown kind, an id out of range or a buffer that is too small. */
int hb_model_id2name(const hb_model* m, const char* kind, int id, char* out, int cap);
/* Copies a named fp64 model array (mjModel field name, e.g. "body_mass", "qpos0") into out[cap];
 * returns its length, or HB_EINVAL. */
int hb_model_get_array(const hb_model* m, const char* field, double* out, int cap);

/* ---- batch --------------------------------------------------------------------------------- */

/* Replaces n_env calls of mj_makeData (mujoco.h:173).  device = HIP ordinal (>= 0).
 * Joint friction loss (dof_frictionloss > 0 on a hinge or slide joint's dof, not disabled by the options): one constraint row per such
 * dof, always active, with the force bounded by -frictionloss <= f <= frictionloss (mj_instantiateFriction).  The rows' constants are
 * worked out here from the options as they are now.  Implemented for models that step in one kernel with the Euler integrator: a model
 * with friction loss that steps in stages (mesh hulls, height fields, condim 4 / 6), or whose integrator is HB_INT_RK4, is refused here
 * with a message that says so.
 * Equality constraints (the model's <equality> section: scalar-joint couplings, mjEQ_JOINT, and connect anchors, mjEQ_CONNECT; get_array
 * fields eq_type, eq_obj1id, eq_obj2id, eq_active0, eq_data [neq][11], eq_solref, eq_solimp - neq is the length of eq_type): one row per
 * active joint coupling and three per active connect, always active, in front of the friction-loss rows, with an unbounded force
 * (mj_instantiateEquality), unless the options carry mjDSBL_EQUALITY or mjDSBL_CONSTRAINT.  The same rules as for friction loss: a model
 * with equality rows that steps in stages, or whose integrator is HB_INT_RK4, is refused here, and so is a model whose equality and
 * friction-loss rows together number more than 32; each message names equality constraints. */
hb_batch* hb_batch_create(const hb_model* m, int n_env, int device, char* err, int err_sz);
/* Replaces mj_deleteData (mujoco.h:206). */
void hb_batch_free(hb_batch* b);
int hb_batch_n_env(const hb_batch* b);
/* The HIP stream (hipStream_t as void*) that orders all work of this batch.  Work the caller enqueues on
 * it before a step call (e.g. a policy writing the controls) is seen by that step; every hb_* call is
 * ordered after the steps enqueued before it.  The call itself performs hb_batch_join. */
void* hb_batch_stream(hb_batch* b);
int hb_batch_sync(hb_batch* b);
/* Pipelined stepping (off by default; on = 1: the default count, on = 2..8: that many segments).  The default is three segments -
 * the first on the batch's own stream - when their streams are seen to run kernels side by side, two when the process' other streams
 * leave them no hardware queue each (ROCm shares GPU_MAX_HW_QUEUES = 4 queues among all streams of a process; the call probes
 * with three idle waves of 60 us, once).  More than four concurrently active queues are slower whatever the setting.  When on, hb_step_dev /
 * hb_rollout*_dev cut the batch into fixed env segments and step each with its own launch on an internal stream: segment c of step t+1
 * follows only segment c of step t, so the slowest envs of one step overlap the start of the next
 * (envs are independent: results are identical to the unpipelined launch).  The internal streams fork
 * from the batch's stream at every step call and are joined back by the next hb_* call of any other
 * kind.  A caller that enqueues its OWN work on hb_batch_stream() after step calls must call
 * hb_batch_join first (or fetch the stream again); callers that only use hb_* functions need nothing.
 * A pipelined batch also folds hb_step_dev calls made back to back into one launch (see hb_step_dev): the same rule covers it. */
int hb_batch_pipeline(hb_batch* b, int on);
/* Number of env segments step calls are cut into at the moment (1: unpipelined). */
int hb_batch_segments(const hb_batch* b);
int hb_batch_join(hb_batch* b);

/* Replaces mj_resetData (keyframe < 0) / mj_resetDataKeyframe (mujoco.h:180,186) for the envs
 * whose mask byte is non-zero (mask == NULL: all).  perturb != 0 adds the deterministic
 * Halton perturbation of SURVEY.md §8(d) (hinges +-0.2 rad, root z +0.1 m) indexed by
 * env_offset + e, mirroring CPUEnv.reset's joint/height randomisation (cpu_env.py:282-328). */
int hb_reset(hb_batch* b, const uint8_t* mask, int keyframe, int perturb, int env_offset);

/* Replaces `for e: mju_copy(d->ctrl, ...); mj_step(m, d)` (mujoco.h:120; call sites
 * simulation/cpu_env.py:683-684, simulation/mujoco/sample/testspeed.cc:93-96).
 * ctrl: env-major [n_env][nu] float32, applied for n_substeps consecutive steps.
 * With integrator HB_INT_RK4 a step is mj_RungeKutta(4): four forward passes (collision, constraint rows and solver in each) at the
 * stage states, combined by the classic tableau, so it costs about four Euler steps; no implicit joint damping (mjDSBL_EULERDAMP has
 * no effect).  ctrl, xfrc_applied (rollout noise: one draw per step) and qacc_warmstart are held for all four stages; the warm start is
 * replaced once, by the last stage's qacc.  The position / velocity checks run at the start of the step and the acceleration check
 * after the first stage only.  What is read after the step is what mjData holds after mj_step: sensors (hb_rollout_sensors, the task
 * residuals, hb_sensors) are those of the FIRST stage; everything else - hb_get_qacc, hb_get_efc_force, hb_get_contacts, hb_get_counts,
 * hb_get_contact_force, hb_get_body_contact, hb_get_body_acc, the env adapter's joint torques - is that of the LAST stage.  HB_WARN_CONTACTFULL / HB_WARN_CNSTRFULL accumulate over all stages.
 * RK4 exists for models that step in one kernel (plane / sphere / capsule geoms, condim 1 / 3): for a model that steps in stages (mesh
 * hulls, height fields, condim 4 / 6) hb_batch_create fails and says so.
 * A model with joint friction loss (hb_batch_create) steps in the friction kernels, hb_fric_* in hb_last_kernel, whatever the launch
 * looks like: they are full kernels - no lean, size-specialised, two-envs-per-wave or folded launch applies to such a model - and run
 * every read-out but the body accelerations.  Row overflow still drops limit and contact rows from the end (HB_WARN_CNSTRFULL): the
 * friction rows, at most nv <= 32, always fit.
 * A model with equality rows (hb_batch_create) steps in the equality kernels, hb_eq_* in hb_last_kernel, under the same rules; they hold
 * the friction rows as well, and the two kinds together, at most 32 rows, always fit.  hb_inverse runs hb_eq_inverse*_kernel: an
 * equality row's force is -D (J qacc - aref) whatever its sign. */
int hb_step(hb_batch* b, const float* ctrl, int n_substeps);
/* The same with the controls already in device memory, asynchronous: the call returns at once, its results are there after hb_batch_sync
 * or behind anything enqueued on hb_batch_stream later, and ctrl_dev must stay allocated and untouched until then.  On a PIPELINED batch
 * (hb_batch_pipeline) of a primitive-geometry model whose waves all fit on the chip at once (8 per CU: up to 2048 envs on MI355X, 4096
 * for the models with the two-envs-per-wave kernel, HB_TUNE_DUO), calls made back to back - nothing else of the batch's API in between -
 * are executed as ONE kernel launch of up to HB_TUNE_FOLD steps, step t reading the controls of call t: no env waits for the batch's
 * slowest one between steps (MI355X: 2048 envs 42 us per step against 64, 4096 envs 62 against 78).  The states are bit-identical to one
 * launch per call; the work starts when HB_TUNE_FOLD steps are held or when any other hb_* call of the batch (hb_batch_sync,
 * hb_batch_stream, hb_batch_join, a read) arrives. */
int hb_step_dev(hb_batch* b, const float* ctrl_dev, int n_substeps);

/* Replaces the open-loop rollout loops (mujoco_mpc/mjpc/trajectory.cc:141-179,
 * simulation/mujoco/sample/testspeed.cc:84-103): T steps in ONE launch with state resident
 * on chip; ctrl is [T][n_env][nu]; qpos_out (nullable) receives [T][n_env][nq] after each step. */
int hb_rollout(hb_batch* b, const float* ctrl, int T, float* qpos_out);
int hb_rollout_dev(hb_batch* b, const float* ctrl_dev, int T, float* qpos_out_dev);
/* Same rollout with controls generated on device from the Halton sequence of
 * testspeed.cc:64-80 (ctrl[t,e,i] = 2*H(1+t0+t+1000*(env_offset+e), i+2)-1): the benchmark
 * workload of SURVEY.md §8(d), no control tensor in HBM. */
int hb_rollout_halton(hb_batch* b, int T, int t0, int env_offset, float* qpos_out_dev);

/* Replaces mj_forward (mujoco.h:129): recompute everything up to qacc without integrating. */
int hb_forward(hb_batch* b, const float* ctrl);

/* Replaces mj_inverse (mujoco.h, declared beside mj_forward) [recall]: the generalized forces that produce the given accelerations in every env,
 *   qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - J' f,   f_i = -D_i (J_i qacc - aref_i) where that is negative, else 0,
 * with M (armature included), the bias and passive forces, the collisions, the constraint rows and their aref computed from the
 * batch's qpos / qvel exactly as hb_forward computes them (per-env model parameters included).  ctrl and xfrc_applied do not enter:
 * for the qacc of hb_forward, qfrc_inverse is qfrc_actuator + J' xfrc_applied.  qacc and qfrc_inverse are env-major [n_env][nv].
 * flags HB_INV_DISCRETE (mjENBL_INVDISCRETE): qacc is (qvel' - qvel) / h of this engine's Euler step with implicit damping, and is
 * turned into the continuous acceleration M^-1 (M + h diag(damping)) qacc first (defined for the Euler step only: HB_EUNSUPPORTED on a
 * model whose integrator is HB_INT_RK4).  warnings (nullable) receives per env the
 * HB_WARN_CONTACTFULL / HB_WARN_CNSTRFULL bits of rows this call dropped.  The call is a pure function of the batch: state, controls,
 * xfrc_applied, status and warning words, env adapter and heavy-first orders are left as they are.  Step calls held back (hb_step_dev)
 * are launched first and the pipes joined, as for every other call.  hb_last_kernel names the inverse kernel.
 * hb_inverse is synchronous with host arrays; hb_inverse_dev takes device arrays and is asynchronous like hb_step_dev. */
#define HB_INV_DISCRETE 1 /* mjENBL_INVDISCRETE */
int hb_inverse(hb_batch* b, const float* qacc, int flags, float* qfrc_inverse, int* warnings);
int hb_inverse_dev(hb_batch* b, const float* qacc_dev, int flags, float* qfrc_inverse_dev, int* warnings_dev);

/* ---- whole-body kinematics read-out ---------------------------------------------------------------------------- */

/* Replaces a direct mj_kinematics + mj_comVel call and the mjData fields it fills (mjData.xpos, xquat, xipos, geom_xpos, geom_xmat),
 * and mj_objectVelocity(objtype body, flg_local = 0) of every body: the poses and velocities of all bodies and the poses of all geoms,
 * as a pure function of (qpos, qvel) and the model.
 *   body_pose [n][nbody][10] = xpos[3] | xquat[4] (w x y z) | xipos[3]
 *   body_vel  [n][nbody][6]  = omega[3] | v[3]: angular velocity and the velocity of the body's own xipos, world axes - the point and
 *                              axes hb_get_body_acc, hb_get_body_contact and the framelinvel sensor entries refer to
 *   geom_pose [n][ngeom][7]  = geom_xpos[3] | quaternion[4] (w x y z) of the geom's world orientation (geom_xmat is its matrix)
 * Row 0 of the body arrays is the world: zero position and velocity, identity quaternion.  Each output may be NULL, not all three.
 * hb_kinematics / hb_kinematics_dev evaluate the batch's qpos / qvel AS THEY ARE NOW (n = n_env): what mj_kinematics + mj_comVel would
 * give if called now.  After a step that is the NEW state, the one the returned observation describes - the mjData.xpos that mj_step
 * leaves behind belongs to the state before the step and is one step stale.  Step calls held back (hb_step_dev) are launched first and
 * the pipes joined, as for hb_inverse.  hb_kinematics_states / _states_dev evaluate n >= 1 given states, qpos [n][nq] and qvel [n][nv]
 * row-major (e.g. the [T][n_env] tapes of hb_rollout_trajectory with n = T * n_env): n is not tied to n_env, qvel may be NULL when
 * body_vel is NULL, and the batch is used for its model, device and stream only.
 * The calls read and compute: state, status and warning words, counts, warm start and orders of the batch stay as they are, and a free
 * joint's quaternion is normalised for the computation only, not written back.  A non-finite or huge input makes the rows of that state
 * unspecified and nothing else.  No model is refused, whatever kernels it steps in: the read-out is a kernel of its own
 * (csrc/hb_kin.hip), hb_last_kernel names it ("hb_kin16_kernel" / "hb_kin32_kernel" / "hb_kin64_kernel": HB_TUNE_KIN_PACK), and
 * hb_batch_step_launches does not count it.  HB_EINVAL: NULL batch, all outputs NULL, n <= 0, NULL qpos, body_vel without qvel.
 * The host forms are synchronous; the _dev forms take device arrays and are asynchronous like hb_inverse_dev. */
int hb_kinematics(hb_batch* b, float* body_pose, float* body_vel, float* geom_pose);
int hb_kinematics_dev(hb_batch* b, float* body_pose_dev, float* body_vel_dev, float* geom_pose_dev);
int hb_kinematics_states(hb_batch* b, const float* qpos, const float* qvel, int n, float* body_pose, float* body_vel, float* geom_pose);
int hb_kinematics_states_dev(hb_batch* b, const float* qpos_dev, const float* qvel_dev, int n, float* body_pose_dev, float* body_vel_dev, float* geom_pose_dev);

/* ---- dynamics read-out ----------------------------------------------------------------------------------------------- */

/* Replaces mj_fullM of mjData.qM, reads of mjData.qfrc_bias and mjData.qfrc_passive, and mj_jacBody / mj_jacSite / mj_jacBodyCom /
 * mj_jacSubtreeCom: the terms of the equations of motion  M qacc + qfrc_bias = qfrc_passive + qfrc_actuator + J' f  of every state, as a
 * pure function of (qpos, qvel) and the model.
 *   M            [n][nv][nv]         the dense symmetric joint-space inertia, armature included; both triangles are written from one
 *                                    computed value: M[i][j] and M[j][i] have the same bits
 *   qfrc_bias    [n][nv]             mj_rne with zero acceleration: Coriolis, centrifugal and gravity terms (none of the last under mjDSBL_GRAVITY)
 *   qfrc_passive [n][nv]             what hb_forward forms: joint springs and dampers (zero under mjDSBL_PASSIVE)
 *   jac          [n][spec.n][6][nv]  per point of the spec: rows 0..2 jacp, rows 3..5 jacr, world axes
 * The dofs of a free joint follow MuJoCo's convention: translations along the world axes, rotations about the body's own axes.
 * A point of the spec is HB_JAC_POINT: fixed in `body`'s frame at `offset` (body coordinates) - offset 0 is mj_jacBody, a site's pos
 * mj_jacSite, the body's ipos mj_jacBodyCom; or HB_JAC_SUBTREE_COM: the centre of mass of the subtree rooted at `body` (mj_jacSubtreeCom;
 * translational rows only, the rotational rows are zero, offset is ignored).  The spec is the same for every state.
 * Any output may be NULL, not all of them; jac and spec go together.
 * hb_dynamics / hb_dynamics_dev evaluate the batch's state AS IT IS NOW (n = n_env; after a step the NEW state, as hb_kinematics does):
 * step calls held back (hb_step_dev) are launched first and the pipes joined.  With per-env model parameters installed
 * (hb_env_domain_randomize) they use each env's own masses, armature and stiffness, as the step kernels do.
 * hb_dynamics_states / _states_dev evaluate n >= 1 given states, qpos [n][nq] and qvel [n][nv] row-major, with the model's nominal
 * parameters: n is not tied to n_env, qvel may be NULL when only M and jac are asked for, and the batch is used for its model, device and
 * stream only.
 * The calls read and compute: state, warm start, status and warning words, counts and orders of the batch stay as they are, and a free
 * joint's quaternion is normalised for the computation only.  A non-finite state makes the rows of that state unspecified and nothing
 * else.  No model is refused, whatever kernels it steps in: the read-out is a kernel of its own (csrc/hb_dyn.hip, no atomics: every sum
 * runs in a fixed order, so a state's result has the same bits whatever n is and wherever the state stands), hb_last_kernel names it
 * ("hb_dyn16_kernel" / "hb_dyn32_kernel" / "hb_dyn64_kernel": HB_TUNE_KIN_PACK chooses as for hb_kinematics), and
 * hb_batch_step_launches does not count it.  HB_EINVAL: NULL batch, all outputs NULL, exactly one of jac and spec, spec.n outside
 * 1..HB_MAX_JAC, a body or kind out of range, n <= 0, NULL qpos, qfrc_bias or qfrc_passive without qvel.
 * The host forms are synchronous; the _dev forms take device arrays (the spec stays a host struct) and are asynchronous like
 * hb_kinematics_dev. */
#define HB_MAX_JAC 16
#define HB_JAC_POINT 0       /* a point fixed in body's frame at `offset` (body frame) */
#define HB_JAC_SUBTREE_COM 1 /* mj_jacSubtreeCom of the subtree rooted at `body`: translational rows only, rotational rows zero */
typedef struct hb_jac_spec {
  int n;
  int kind[HB_MAX_JAC];
  int body[HB_MAX_JAC];
  float offset[HB_MAX_JAC][3];
} hb_jac_spec;
int hb_dynamics(hb_batch* b, float* M, float* qfrc_bias, float* qfrc_passive, const hb_jac_spec* spec, float* jac);
int hb_dynamics_dev(hb_batch* b, float* M_dev, float* qfrc_bias_dev, float* qfrc_passive_dev, const hb_jac_spec* spec, float* jac_dev);
int hb_dynamics_states(hb_batch* b, const float* qpos, const float* qvel, int n, float* M, float* qfrc_bias, float* qfrc_passive, const hb_jac_spec* spec, float* jac);
int hb_dynamics_states_dev(hb_batch* b, const float* qpos_dev, const float* qvel_dev, int n, float* M_dev, float* qfrc_bias_dev, float* qfrc_passive_dev,
                           const hb_jac_spec* spec, float* jac_dev);

/* ---- ray casting ------------------------------------------------------------------------------------------------------ */

/* Replaces mj_ray / mj_multiRay (mujoco.h) [recall] for a fixed set of rays cast in every env: what a rangefinder, or the grid of downward
 * rays of a terrain height scan, sees from the batch's state.
 * hb_ray_configure installs n_ray rays, 1 <= n_ray <= 4096: pnt / vec are host arrays [n_ray][3], origin and direction in the frame the
 * spec names.  They are copied to the device, into a buffer the batch owns, and stay installed until replaced or removed (n_ray 0 or a
 * NULL spec).  vec is normalised here; a zero or non-finite vector (or a non-finite pnt) gives HB_EINVAL.
 *   HB_RAY_FRAME_WORLD  world coordinates
 *   HB_RAY_FRAME_BODY   coordinates of frame_body's frame (xpos, xquat): a rangefinder site
 *   HB_RAY_FRAME_YAW    the heading frame of frame_body, the height-scan frame: origin = xpos[frame_body]; x = the body's x axis projected
 *                       onto the world xy plane and normalised, or the world x axis when that projection is shorter than 1e-6; z = world
 *                       z; y = z x x
 * Eligible geoms: those of the world body with HB_RAY_STATIC, those of every other body with HB_RAY_MOVING, less the geoms of body
 * bodyexclude (-1: none).  The surfaces are mj_rayGeom's [recall]:
 *   plane        the z = 0 plane of the geom frame, hit from either side, inside size[0..1] where those are > 0
 *   sphere       the smallest non-negative root; from inside that is the exit point
 *   capsule      likewise, on the cylinder wall between the caps and the outer halves of the two end spheres
 *   box          the six faces in the geom's frame (the slab test): the nearest non-negative crossing of a face's plane inside the
 *                other two half extents - from outside the face the ray enters by, from inside the one it leaves by
 *   height field the elevation surface, triangulated exactly as the collider triangulates it: cell (r, c) is cut along the diagonal
 *                (r, c) - (r + 1, c + 1).  Both faces are hit.  With per-env elevations installed (hb_env_domain_randomize with
 *                floor_bump_max > 0) the env's OWN elevations are used.  The field's side walls and base are NOT intersected - a
 *                departure from MuJoCo, which also tests the field's bounding box: a ray that passes under the surface from the side
 *                sees the surface from below, or nothing.
 * Mesh and cylinder geoms (and ellipsoid ones) are not intersected: a configuration under which a geom of such a type would be
 * eligible is refused with HB_EUNSUPPORTED (Batch.ray_configure names the geom), e.g. HB_RAY_MOVING on the reference's robot, whose
 * HB_RAY_STATIC configurations see its height-field floor.  The one exception: a geom of such a type that collides with nothing (contype
 * and conaffinity both 0 - a visual marker, like the axis cylinders of the reference's world) is skipped, not refused.  A refused configuration (HB_EUNSUPPORTED or HB_EINVAL) leaves the previous
 * one installed and the batch stepping.  HB_EINVAL: NULL batch or arrays, n_ray out of range, an unknown frame, frame_body or
 * bodyexclude out of range, flags without HB_RAY_STATIC or HB_RAY_MOVING.
 * hb_rays / hb_rays_dev cast the installed rays at the batch's qpos AS IT IS NOW (after a step: the new state, as for hb_kinematics):
 *   dist   [n_env][n_ray]  metres along the unit direction to the nearest eligible surface; a hit farther than cutoff (> 0) counts as none
 *   geomid [n_env][n_ray]  the geom that was hit; ties go to the lowest geom id
 * Both are -1 where nothing is hit: mj_ray's return convention.  Either may be NULL, not both.  Step calls held back (hb_step_dev) are
 * launched first and the pipes joined.  Nothing of the batch is written: state, warm start, status and warning words, counts and orders
 * stay as they are.  The arithmetic is fp32, one lane per ray, without atomics: a ray's result has the same bits whatever n_env is and
 * wherever the ray stands in the array.  A non-finite state makes that env's rows unspecified and nothing else.  The rays are a kernel
 * of their own (csrc/hb_ray.hip; "hb_ray_kernel" / "hb_ray_lds_kernel" in hb_last_kernel - the latter stages the env's elevations in LDS),
 * behind the kinematics read-out's launch for the poses it needs (none for world-frame rays at static geoms); hb_batch_step_launches
 * counts neither.  HB_EINVAL: nothing configured, or both outputs NULL.  hb_rays is synchronous with host arrays; hb_rays_dev takes
 * device arrays and is asynchronous like hb_kinematics_dev. */
#define HB_RAY_STATIC 1      /* geoms of the world body are eligible (terrain, floor) */
#define HB_RAY_MOVING 2      /* geoms of moving bodies are eligible */
#define HB_RAY_FRAME_WORLD 0 /* pnt / vec are world coordinates */
#define HB_RAY_FRAME_BODY 1  /* ... coordinates of frame_body's frame (xpos, xquat): a rangefinder site */
#define HB_RAY_FRAME_YAW 2   /* ... of the heading frame of frame_body: the height-scan frame */
typedef struct hb_ray_spec {
  int frame, frame_body, bodyexclude /* -1: none */, flags;
  float cutoff; /* > 0: hits farther than this count as no hit; <= 0: no limit */
} hb_ray_spec;
int hb_ray_configure(hb_batch* b, const hb_ray_spec* spec, const float* pnt, const float* vec, int n_ray);
int hb_rays(hb_batch* b, float* dist, int* geomid);
int hb_rays_dev(hb_batch* b, float* dist_dev, int* geomid_dev);

/* ---- wire format of a state ------------------------------------------------------------ */

/* One env's state as the `State` message of the reference's gRPC agent service (mujoco_mpc/mjpc/grpc/agent.proto:75-83:
 * time = 1, qpos = 2, qvel = 3, act = 4, mocap_pos = 5, mocap_quat = 6, userdata = 7; doubles, repeated fields packed),
 * in protobuf wire encoding, so that existing clients' GetState / SetState payloads can be produced and consumed
 * without a protobuf dependency.  This engine has no activations, mocap bodies or user data: those fields are not
 * written, and a message that carries any of them is refused (HB_EUNSUPPORTED).
 * hb_state_to_proto returns the number of bytes the message takes (also when buf is NULL or cap is too small: call
 * twice), hb_state_from_proto sets the fields present (absent ones keep their values; qacc_warmstart is reset to 0 as
 * mj_setState leaves it for a new state). */
int hb_state_to_proto(hb_batch* b, int env, unsigned char* buf, int cap);
int hb_state_from_proto(hb_batch* b, int env, const unsigned char* buf, int len);

/* ---- planner rollouts (MJPC's Trajectory::Rollout, mujoco_mpc/mjpc/trajectory.cc:100-210) -------------------- */

/* The sensors MJPC's humanoid tasks build their residuals from (tasks/humanoid_cap/stand/task.xml:22-40), and the contact and
 * acceleration sensors of a legged robot.  Per env and step the read-out is a row of hb_sensor_size() floats, its parts in the order of
 * the fields below (hb_sensor_row names where each begins):
 *   [ framepos (3 each) | subtreecom (3), subtreelinvel (3) | frame axes (3 each) | framelinvel (3 each) | subtreelinvel (3 each)
 *     | touch (1 each) | contact force (3 each) | accelerometer, gyro (6 each) | frameangacc, framelinacc (6 each) ]
 * framepos: up to 16 bodies or sites (a site is a body plus an offset in the body frame); subtreecom / subtreelinvel (mj_subtreeVel,
 * mujoco.h:346): of one kinematic tree, named by its root body (a direct child of the world; < 0: none). */
#define HB_MAX_FRAMEPOS 16
typedef struct hb_sensor_spec {
  int n_framepos;
  int framepos_body[HB_MAX_FRAMEPOS];
  int subtree_body;
  float framepos_offset[HB_MAX_FRAMEPOS][3]; /* position in the body's frame: zeros = objtype "xbody" (the body frame); a site's pos = objtype
                                               "site"; the body's ipos (hb_model_get_array "body_ipos") = objtype "body" (inertial frame) */
  /* further read-outs, appended behind the above in this order (3 floats each): */
  int n_frameaxis;            /* framexaxis / framezaxis of a body frame (objtype "xbody") */
  int frameaxis_body[8];
  int frameaxis_which[8];     /* 0: x axis, 2: z axis */
  int n_framelinvel;          /* framelinvel, objtype "body": linear velocity of the body's inertial frame origin, world axes */
  int framelinvel_body[8];
  int n_subtreelinvel;        /* subtreelinvel of further bodies (any body of the model, not only a tree root) */
  int subtreelinvel_body[4];
  /* contact sensors, appended behind all of the above.  They belong to the acceleration stage of the step's forward pass: row t of
   * hb_rollout_sensors holds the forces of step t's constraint solve (RK4: of its first stage, like every sensor).  A spec that has
   * any of them makes its launches carry the contact-force read-out (see hb_contact_readout; the getters there stay off). */
  int n_touch;                /* one float each: the sum of the normal forces f[0] of the contacts that involve the body - MuJoCo's touch */
  int touch_body[8];          /*   sensor taken over the WHOLE BODY instead of a site volume */
  int n_contactforce;         /* three floats each: the force part of the body's contact wrench (hb_get_body_contact), world axes */
  int contactforce_body[4];
  /* acceleration sensors, appended behind the contact sensors.  They too belong to the acceleration stage: row t holds step t's forward
   * pass (RK4: its first stage).  A spec that has any of them makes its launches carry the body-acceleration read-out (see
   * hb_body_acc_readout; the getter there stays off).  Both include the gravity pseudo-acceleration, as MuJoCo's do: at rest on the
   * floor they read +|g| upward, in free fall 0. */
  int n_imu;                  /* six floats each: accelerometer[3] | gyro[3] of a site at body frame + offset with the body's orientation: */
  int imu_body[4];            /*   R' (linear acceleration of that point, omega x v included) | R' omega, R = the body's xmat */
  float imu_offset[4][3];
  int n_frameacc;             /* six floats each: frameangacc[3] | framelinacc[3], objtype body: row b of hb_get_body_acc */
  int frameacc_body[4];
} hb_sensor_spec;
int hb_sensor_size(const hb_sensor_spec* spec);  /* the width of a row; HB_EINVAL for NULL or a count outside [0, its array's length] */
/* The layout of that row: the offset (floats) and the count (entries, as in the spec; subtree: 1 or 0) of each part, and the width.  A
 * part that is off has count 0 and the offset at which it would begin.  Needs no batch; HB_EINVAL for NULL, for a spec hb_sensor_size
 * refuses and for an empty one.  (The struct has no typedef: the function bears the name.) */
struct hb_sensor_row {
  int framepos, n_framepos;
  int subtree, n_subtree;
  int axis, n_axis;
  int linvel, n_linvel;
  int sub, n_sub;
  int touch, n_touch;
  int cfrc, n_cfrc;
  int imu, n_imu;
  int facc, n_facc;
  int width;
};
int hb_sensor_row(const hb_sensor_spec* spec, struct hb_sensor_row* out);
/* mj_setState of ONE state on every env: the N candidate action sequences of a sampling planner all start from the
 * current state (sampling/planner.cc:342-380).  `state` is one record of hb_state_size(b, spec) floats. */
int hb_set_state_broadcast(hb_batch* b, unsigned spec, const float* state);
int hb_set_state_broadcast_f64(hb_batch* b, unsigned spec, const double* state);
/* hb_rollout plus the sensor read-out of every step: sensor_out[t][e][:] holds the sensors mj_step evaluates at the
 * state BEFORE step t's integration (what mjData.sensordata holds after the t-th mj_step call).  Host pointers;
 * qpos_out nullable. */
int hb_rollout_sensors(hb_batch* b, const float* ctrl, int T, const hb_sensor_spec* spec, float* sensor_out, float* qpos_out);
/* SamplingPolicy::Action for every candidate on the device (mujoco_mpc/mjpc/planners/sampling/policy.cc:50-58 over
 * mjpc/spline/spline.cc:103-156,240-277): knots[e][k][nu] are the spline nodes of candidate e (host, [n_env][n_points][nu]),
 * times[n_points] the node times shared by the candidates, interpolation 0 = zero-order, 1 = linear, 2 = cubic Hermite
 * with finite-difference slopes.  The splines are sampled at time0 + t * timestep for t = 0..T-1, clamped to ctrlrange
 * and left on the device as the action tape of the rollouts that follow: pass HB_CTRL_TAPE as their `ctrl` (the
 * hb_rollout_task_* functions accept it; horizon - 1 <= T).  n_points * nu floats per candidate cross PCIe instead of
 * T * nu. */
#define HB_CTRL_TAPE ((const float*)(uintptr_t)1)
int hb_ctrl_tape_splines(hb_batch* b, const float* knots, const float* times, int n_points, int interpolation, double time0, int T);
/* The tape hb_ctrl_tape_splines left on the device, copied back: out[T][n_env][nu] (host), T <= the tape's length; HB_EINVAL when
 * there is no tape (any call that writes the batch's controls discards it).  This is TimeSpline::Sample for every candidate at
 * every step time, which is how the reference's own expectations for the spline (mujoco_mpc/mjpc/test/spline/spline_test.cc:52-157)
 * are checked against the device code (tests/test_gpu_mjpc_expectations.py). */
int hb_ctrl_tape_read(hb_batch* b, int T, float* out);
/* BaseResidualFn::CostTerms and CostValue (mujoco_mpc/mjpc/task.cc:71-110) for n residual vectors at once, on the device, with the
 * code the hb_rollout_task_* kernels use: term k = weight[k] * Norm(norm[k]; norm_p[k]) over the next dim[k] entries of the
 * residual (mjpc/norm.h:24-36), cost = the sum through the risk transformation (exp(risk c) - 1) / risk, or the sum itself when
 * |risk| < 1e-6.  residual[n][n_residual], terms[n][n_term] (nullable), cost[n]: host pointers.  sum(dim) must equal n_residual. */
typedef struct hb_cost_spec {
  int n_term;
  int dim[8];
  int norm[8];          /* mjpc::NormType */
  float weight[8];
  float norm_p[8][2];
  float risk;
} hb_cost_spec;
int hb_task_cost(hb_batch* b, const float* residual, int n, int n_residual, const hb_cost_spec* spec, float* terms, float* cost);
/* Trajectory::NoisyRollout's perturbation (mujoco_mpc/mjpc/trajectory.cc:147-156): before every step of the calls that
 * follow, every xfrc_applied entry of every env becomes rate * xfrc + scale * N(0, 1), rate = exp(-timestep / xfrc_rate),
 * scale = xfrc_std * sqrt(1 - rate^2) (an Ornstein-Uhlenbeck process with stationary deviation xfrc_std); xfrc_std = 0
 * switches it off (the xfrc_applied values stay as they are).  The draws are counter-based (seed, global env, call, step,
 * entry): reproducible, unlike the reference's absl::BitGen, and independent across envs. */
int hb_rollout_noise(hb_batch* b, float xfrc_std, float xfrc_rate, unsigned seed);
/* Open-loop rollout that records the trajectory the way MJPC's Trajectory::Rollout does (mujoco_mpc/mjpc/trajectory.cc:
 * 141-190): states after every step, qpos_out[t][e][nq] and qvel_out[t][e][nv] (host pointers, each nullable; times are
 * t0 + (t + 1) * timestep and the actions are the caller's own tape), and failed[e] = 1 when the env raised a bad-state
 * warning on the way (CheckWarnings, utilities.cc:787-799; nullable). */
int hb_rollout_trajectory(hb_batch* b, const float* ctrl, int T, float* qpos_out, float* qvel_out, int* failed);
/* ---- transition derivatives for the gradient-based planners ------------------------------------------------------
 * mjd_transitionFD (mujoco.h:1242-1251) for T (state, control) points at once, the way ModelDerivatives::Compute fans it
 * over its thread pool (mujoco_mpc/mjpc/planners/model_derivatives.cc:44-105): finite differences of the discrete
 * dynamics x' = step(x, u) in tangent-space coordinates, x = (qpos, qvel), dx = (dqpos in R^nv, dqvel),
 *     A[t] = d x'/d x   [2nv][2nv],     B[t] = d x'/d u   [2nv][nu]      (row-major doubles; either may be NULL).
 * Every perturbed copy of every point is one env of the batch: T * (1 + k * (2nv + nu)) envs are needed, k = 2 when
 * `centered`, else 1 (HB_EINVAL if the batch is smaller); all of them advance in ONE step launch.  x[t] = qpos[nq] |
 * qvel[nv]; warmstart[t][nv] (nullable: zeros) is used by the nominal and by every perturbed copy, as mjd_transitionFD
 * does.  Position perturbations and differences go through mj_integratePos / mj_differentiatePos (quaternion dofs in
 * the tangent space); a control is nudged inside its ctrlrange.  The arithmetic is fp32 on the device: eps should be
 * about 1e-3 (rounding in x' divided by eps is the noise floor), not the 1e-6 an fp64 caller would use.
 * The batch's states are overwritten. */
int hb_transition_fd(hb_batch* b, const double* x, const double* u, const double* warmstart, int T, double eps, int centered, double* A, double* B);
/* The same with the sensor derivatives of mjd_transitionFD: d(sensor) = C dx + D du, for the read-out row of `spec`
 * (hb_sensor_size(spec) values, evaluated in the step's forward pass, i.e. at (x, u) itself: the residual Jacobians a
 * gradient-based planner builds its cost derivatives from).  C[t][ns][2nv], D[t][ns][nu], either nullable. */
int hb_transition_fd_sensors(hb_batch* b, const double* x, const double* u, const double* warmstart, int T, double eps, int centered,
                             const hb_sensor_spec* spec, double* A, double* B, double* C, double* D);

/* ---- a planner iteration's cost evaluation on the device: MJPC's "Humanoid Stand" task ------------------------------
 * (mujoco_mpc/mjpc/tasks/humanoid/stand/{stand.cc:41-104, task.xml:14-36}; the two-foot variant of
 * tasks/humanoid_cap/stand is the same residual with n_feet = 2).  Residual, in order: Height (head z minus mean foot z
 * minus height_goal), Balance (distance in xy of the mean foot position from the capture point com + 0.2 s * com
 * velocity), CoM Vel. (xy), Joint Vel. (qvel[6:]), Control (ctrl); cost = sum_k weight[k] * Norm(norm[k]; norm_p[k])
 * (mjpc/norm.h:24-36, task.cc:71-110), risk transformation as in task.cc:104-109. */
typedef struct hb_task_stand {
  int head_body;
  int n_feet;              /* 1..4 foot frames (the reference's sites sp0..sp3): body + offset in the body frame */
  int foot_body[4];
  float foot_offset[4][3];
  int subtree_body;        /* root body of the tree whose subtreecom / subtreelinvel enter (torso) */
  float height_goal;       /* task parameter "Height Goal" */
  int norm[5];             /* mjpc::NormType per term */
  float weight[5];
  float norm_p[5][2];      /* norm parameters p, q */
  float risk;              /* task_risk (0: risk neutral) */
} hb_task_stand;
/* The values of the reference's task.xml for this model: bodies "head", "foot_left", "foot_right", "torso" by name, feet
 * offsets of sites sp0..sp3 (humanoid.xml.patch:170-171,217-218); HB_EINVAL if the model has no such bodies. */
int hb_task_stand_default(const hb_model* m, hb_task_stand* out);
/* Trajectory::Rollout + UpdateReturn (trajectory.cc:100-210,312-326) for N candidates at once: from the batch's current
 * state, horizon - 1 steps with ctrl[t][e][nu] (host, [horizon-1][n_env][nu]; the last action is repeated for the final
 * mj_forward, zero when horizon = 1), the residual of every one of the `horizon` states, its cost, and
 * total_return[e] = mean cost (1e6 for a candidate that raised a bad-state warning: kMaxReturnValue).  costs
 * ([horizon][n_env], nullable) receives the stage costs.  Nothing but these floats crosses PCIe on the way back.  The
 * per-env status words are cleared first: failure is a property of this rollout. */
int hb_rollout_task_stand(hb_batch* b, const float* ctrl, int horizon, const hb_task_stand* task, float* total_return, float* costs);

/* MJPC's "Humanoid Walk" task the same way (mujoco_mpc/mjpc/tasks/humanoid/walk/{walk.cc:44-163, task.xml:14-86}).
 * Residual, in order: torso height (1), pelvis/feet (1), balance (2: capture point against its projection onto the
 * segment between the feet), upright (8), posture (qpos[7:]), walk (1), move feet (2), control (nu).  The cost terms are
 * the task's user sensors IN THEIR ORDER with THEIR dimensions (Height 1, Pelvis/Feet 1, Balance 2, Upright 8, Posture
 * nq-7, Velocity 2, Walk 1, Control nu), applied to consecutive slices of that vector as BaseResidualFn::CostTerms does. */
typedef struct hb_task_walk {
  int torso_body, pelvis_body, foot_right_body, foot_left_body, waist_lower_body;
  float height_goal;  /* residual_Torso */
  float speed_goal;   /* residual_Speed */
  int n_term;
  int dim[8];
  int norm[8];
  float weight[8];
  float norm_p[8][2];
  float risk;
} hb_task_walk;
int hb_task_walk_default(const hb_model* m, hb_task_walk* out);
int hb_rollout_task_walk(hb_batch* b, const float* ctrl, int horizon, const hb_task_walk* task, float* total_return, float* costs);

/* The same read-out at the current state (mj_forward, no integration): the terminal residual of a trajectory. */
int hb_sensors(hb_batch* b, const float* ctrl, const hb_sensor_spec* spec, float* sensor_out);

/* Replaces mj_stateSize / mj_getState / mj_setState (mujoco.h:378-384). */
int hb_state_size(const hb_batch* b, unsigned spec);
int hb_get_state(hb_batch* b, unsigned spec, float* out);
int hb_set_state(hb_batch* b, unsigned spec, const float* in);
/* fp64 variants for bit-exact hand-over of oracle/CPU states */
int hb_get_state_f64(hb_batch* b, unsigned spec, double* out);
int hb_set_state_f64(hb_batch* b, unsigned spec, const double* in);

/* Env adapter outputs, the 27-DoF analogue of CPUEnv._get_obs/_get_reward (cpu_env.py:465-616):
 * obs[n_env][nobs] = [hinge qpos (nv-6), hinge qvel (nv-6), root angular velocity (3),
 * gravity direction in the torso frame (3)]; reward/terminated/truncated may be NULL; when requested they are
 * evaluated with the current hb_env_config without resetting anything (pure query). */
int hb_get_obs(hb_batch* b, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated);

/* Per-env status bits (HB_WARN_*), accumulated since the last hb_reset; replaces polling
 * mjData.warning (mujoco_mpc/mjpc/utilities.cc:787-799 CheckWarnings). */
int hb_get_status(hb_batch* b, int* status);
/* The same for a training loop that resets finished envs in place (hb_env_step with auto_reset): hb_get_status is cleared by an env's reset,
 * so a warning of an episode that ended before the next poll would be lost.  warnings[e] = the bits env e has raised since the previous
 * call of this function, in whatever episodes; the call clears what finished episodes left behind. */
int hb_env_warnings(hb_batch* b, int* warnings);
/* The joint torques the env adapter's reward reads: qfrc[n_env][nv] = qfrc_smooth + qfrc_constraint (= M qacc) of the last physics step of
 * the last hb_env_step; zeros before the first one. */
int hb_env_joint_torques(hb_batch* b, float* qfrc);
/* Per-env counters of the last step: ncon, nefc, solver iterations (mjData.ncon/nefc/
 * solver_niter, mjdata.h:196-201) — what testspeed.cc:97-98 accumulates.  nefc counts the friction-loss rows of the model as well
 * (one per dof with dof_frictionloss > 0: they are always active) and its equality rows (one per active joint coupling, three per
 * active connect). */
int hb_get_counts(hb_batch* b, int* ncon, int* nefc, int* niter);
/* Name of the step kernel the batch's last step / rollout / forward launch ran ("hb_step_duo_kernel", "hb_step_h27_q_kernel", ...; ""
 * before the first).  Which instantiation a launch takes depends on the model's solver and sizes and on the optional inputs / outputs
 * the call asked for: the parity tests assert that the kernel they checked is the kernel the benchmark times, and
 * bench.py names the kernel of its roofline object by this string.  The pointer stays valid for the life of the library. */
const char* hb_last_kernel(hb_batch* b);
/* How many times the batch has launched its step kernel(s) so far - the launches of one call's env segments (hb_batch_pipeline) count as
 * one, a staged step's kernels as one, hb_step_dev calls folded into one launch as one: bench.py divides its timed region by the
 * difference to get the launch duration its roofline object quotes.  Step calls still held back are launched first. */
long long hb_batch_step_launches(hb_batch* b);
/* "<device name> (<gfx arch>, <n> CUs) #<index>" of the GPU the batch lives on: what every rank of a multi-GPU bench.py run reports about
 * itself (the reference's testspeed.cc prints its thread count: sample/testspeed.cc:203-210). */
int hb_batch_device_name(const hb_batch* b, char* out, int cap);
/* Run-time choices between kernels and schedules: for the tests that compare them and for measurements.  Takes effect from the next
 * launch on.  Nothing of the reference corresponds: mj_step (mujoco.h:120) has one code path.  DUO, LEAN, SIZED, NARROW_PRIM, SCHEDULE,
 * FOLD and KIN_PACK give the SAME results: a test holds each bit-identical to its alternative (tests/test_gpu_kernel_matrix.py, test_gpu_duo.py,
 * test_gpu_fold.py).  STAGED, FASTPASS and POLICY_LEAN choose kernels that sum in other orders (one register group against two or four,
 * the policy kernel's own arithmetic): their results differ by rounding, and tests hold them to the fp64 oracle or to each other within
 * bounds instead (tests/test_gpu_kernel_matrix.py, test_gpu_staged.py, test_gpu_policy.py).
 *   HB_TUNE_DUO            two envs per wavefront for the lean launches of the 27-dof humanoid's PGS kernel (csrc/hb_step_duo.hip; DESIGN.md
 *                          3.8): 1 (default) where it pays - pipelined step calls of batches from 2.5 x the chip's wave slots on (5120 envs on
 *                          MI355X), unpipelined ones from 1.5 x (3072), launches of several steps from more than 1 x (2049); 0 never; 2 always
 *   HB_TUNE_LEAN           1 (default): launches without optional inputs / outputs take the lean instantiations of step_body; 0: the full ones
 *   HB_TUNE_SIZED          1 (default): models with the size signature of the 27-dof humanoid / the reference's robot take the kernels that
 *                          have those sizes as constants; 0: the generic ones
 *   HB_TUNE_STAGED         1 (default): models with mesh hulls / height fields step in stages (pose, narrowphase, step kernels: DESIGN.md
 *                          3.6); 0: everything inside one step kernel
 *   HB_TUNE_FASTPASS       1 (default): the staged step runs the one-group fast kernel first and the full one for what that defers; 0: full only
 *   HB_TUNE_NARROW_PRIM    1 (default): a model without mesh geoms takes the narrowphase kernel that has no hull climb in it
 *   HB_TUNE_SCHEDULE       1 (default): blocks are dispatched heavy-first (hb_order_kernel); 0: in env order
 *   HB_TUNE_REORDER_PERIOD the heavy-first order is re-sorted every n-th step call (default 4), and after every launch of eight steps or more
 *                          (the multi-step two-envs-per-wave kernel pairs its envs by that order: DESIGN.md 3.9)
 *   HB_TUNE_POLICY_LEAN    hb_rollout_policy: 1 (default) the LDS-free policy kernel beside the other segments' step kernels when
 *                          pipelined; 0 never; 2 always
 *   HB_TUNE_FOLD           hb_step_dev calls enqueued back to back run as ONE launch of up to this many steps (default and maximum 256; 1:
 *                          every call its own launch).  See hb_step_dev.
 *   HB_TUNE_KIN_PACK       hb_kinematics* and hb_dynamics*: 1 (default) as many states per wavefront as fit (16 or 32 lanes per state for models of up to 16 /
 *                          32 moving bodies); 0: one state per wavefront.  The same bits (tests/test_gpu_kinematics.py)
 * Environment variables the library reads (all others of earlier rounds are gone): HB_DEBUG (name failing HIP calls on stderr), HB_DUO
 * (HB_TUNE_DUO's value for new batches), HB_BOX_CULL=0 (model tables without the oriented-box cull of portal-search pairs: a test),
 * and in the diagnostic build (-DHB_STAMPS) HB_STOP_PHASE and HB_MPR_LIMIT (tools/gpu_narrow_limits.sh). */
enum { HB_TUNE_DUO = 0, HB_TUNE_LEAN, HB_TUNE_SIZED, HB_TUNE_STAGED, HB_TUNE_FASTPASS, HB_TUNE_NARROW_PRIM, HB_TUNE_SCHEDULE, HB_TUNE_REORDER_PERIOD,
       HB_TUNE_POLICY_LEAN, HB_TUNE_FOLD, HB_TUNE_KIN_PACK, HB_TUNE_COUNT };
int hb_batch_tune(hb_batch* b, int knob, int value);
/* Narrowphase work of the last step of each env, for models that collide through mesh hulls or height fields (the staged step:
 * DESIGN.md 3.6): nwork = work items (a candidate pair that passed the broadphase, or one prism of a height-field pair's sub-grid),
 * nsearch = those of them that needed a portal search (mjc_Convex / mjc_ConvexHField: libccd MPR), kcycles = shader clock cycles / 1024
 * the env's narrowphase wave took (saturating at 255; the cost the heavy-first dispatch of that launch sorts by).  Zeros for other
 * models.  Any pointer may be NULL. */
int hb_get_collision_counts(hb_batch* b, int* nwork, int* nsearch, int* kcycles);

/* Diagnostics of the last step for parity tests (mjData.qacc, efc_force, contact[]; mjdata.h:
 * 362,376,427): enable once, then read after a step.  efc_force is [n_env][nefc_max];
 * contact is [n_env][ncon_max][16] = dist, pos[3], frame[9], dim, geom1, geom2.
 * Row order (mj_makeConstraint's; a model without equality rows): the friction-loss rows in dof order, then joint limits, tendon limits and
 * contacts.  A friction row's entry is the joint-space friction force on its dof, in [-frictionloss, frictionloss]; every other row's is
 * >= 0.  A model with nf friction rows has its limit rows start at row nf, and every contact's first row moves up by nf as well.
 * With equality rows the order is mj_makeConstraint's in full: the ne equality rows first, in the order of the <equality> section (a
 * connect: world x, y, z), then friction loss, limits, contacts.  An equality row's entry is signed and unbounded; limit rows start
 * at row ne + nf. */
int hb_diag_enable(hb_batch* b, int on);
int hb_get_qacc(hb_batch* b, float* qacc);
int hb_get_efc_force(hb_batch* b, float* efc_force);
int hb_get_contacts(hb_batch* b, float* contact);

/* ---- contact forces (mj_contactForce, mjData.cfrc_ext; mujoco.h, mjdata.h) ---------------------------------------------------
 * What each contact pushed with in the last constraint solve, decoded on the device from the solver's own rows.
 * For contact c with first row a, dimension d, friction coefficients mu[0..d-2] (sliding, sliding, torsional, rolling, rolling) and
 * frame rows n, t1, t2 (hb_get_contacts):
 *   contact-frame force f[6]:  d == 1: f[0] = efc_force[a];  otherwise, with r = efc_force[a .. a + 2 (d - 1)) the pyramid rows:
 *                              f[0] = sum r, f[i + 1] = mu[i] (r[2 i] - r[2 i + 1]);  entries at and beyond d are 0.
 *                              A contact without rows - in the gap (dist >= margin - gap), or dropped with HB_WARN_CNSTRFULL - has f = 0.
 *   world force  F = frame' f[0:3], world torque T = frame' f[3:6]: acting with + on the body of geom2, with - on the body of geom1,
 *                              at the contact position.
 *   body contact wrench        w[b] = (sum +-F, sum +-((pos - xipos[b]) x F + T)) over the contacts of body b, for every body, the
 *                              world (row 0) included: mjData.cfrc_ext WITHOUT xfrc_applied, and with the torque taken about the
 *                              body's OWN inertial-frame origin xipos[b], world axes (the reference's cfrc_ext refers to the subtree
 *                              centre of mass of the body's tree).  The sums run in contact order in one lane per body, without
 *                              atomics: the same bits for the same state, however the batch is launched.
 * hb_contact_readout(b, 1) allocates the two buffers; from the next launch on every step, forward and env-step launch writes them (such
 * a launch runs the full step kernel: the lean and two-envs-per-wave kernels have no read-out).  off: launches stop writing them.
 * hb_get_contact_force: [n_env][ncon_max][6], zeros beyond the env's ncon; row k belongs to contact k of hb_get_contacts.
 * hb_get_body_contact:  [n_env][nbody][6] = force[3] | torque[3].
 * Both launch step calls held back and join the pipes like every other read, and return HB_EINVAL while the read-out is off.  They
 * hold the LAST forward pass (RK4: the last stage; the sensor entries of hb_sensor_spec hold the first - the rule at hb_step).  Envs a
 * launch skips (an env mask) keep their rows.
 * hb_contact_readout_dev hands out the device buffers (same layouts; either pointer may be NULL) for a policy or reward on the same
 * GPU: it joins like hb_batch_stream, so work enqueued on the batch's stream afterwards sees the step calls made so far. */
int hb_contact_readout(hb_batch* b, int on);
int hb_get_contact_force(hb_batch* b, float* out);
int hb_get_body_contact(hb_batch* b, float* out);
int hb_contact_readout_dev(hb_batch* b, const float** contact_force_dev, const float** body_contact_dev);

/* ---- body accelerations (mj_rnePostConstraint's cacc, mj_objectAcceleration; mujoco.h) -------------------------------------------
 * What every body does in the last forward pass, from the qacc the solver ended with (exactly the vector hb_get_qacc reports):
 *   cacc[0] = (0, -gravity)   (the world; zero with mjDSBL_GRAVITY)
 *   cacc[b] = cacc[parent(b)] + sum over the dofs i of b: cdof_dot[i] qvel[i] + cdof[i] qacc[i]
 * The convention INCLUDES the gravity pseudo-acceleration: a body at rest on the floor reads +|g| upward, a body in free fall reads 0 -
 * what MuJoCo's accelerometer, framelinacc and cacc all do, and what a real IMU's specific force is.
 * hb_get_body_acc: [n_env][nbody][6] = angular acceleration[3] | linear acceleration[3] of the body's OWN inertial-frame origin
 * xipos[b], world axes: mj_objectAcceleration(objtype body, flg_local = 0).  The reference's raw cacc refers to the subtree centre of
 * mass of the body's tree and lacks the omega x v term; here it is transported to xipos and omega x v(xipos) is added - the same "own
 * origin, world axes" choice as hb_get_body_contact.  Row 0 (the world) is (0, -gravity).  One lane per body sums its dofs in
 * ascending order, without atomics: the same bits for the same state, however the batch is launched.
 * hb_body_acc_readout(b, 1) allocates the buffer (and a scratch of 24 floats per body); from the next launch on every step, forward
 * and env-step launch writes it (such a launch runs the full step kernel's instantiation with the read-out, hb_acc_* in hb_last_kernel:
 * the lean and two-envs-per-wave kernels have none, and the full kernels themselves are compiled without it).
 * off: launches stop writing it.  hb_get_body_acc launches step calls held back and joins the pipes like every other read, and returns
 * HB_EINVAL while the read-out is off.  hb_body_acc_readout(b, 1) on a model with friction-loss or equality rows returns HB_EUNSUPPORTED (no step
 * kernel has both), and so does a sensor spec with n_imu or n_frameacc entries; the batch goes on stepping.  It holds the LAST forward pass (RK4: the last stage; the sensor entries of hb_sensor_spec hold
 * the first - the rule at hb_step).  Envs a launch skips (an env mask) keep their rows.
 * hb_body_acc_readout_dev hands out the device buffer (same layout) for a policy or reward on the same GPU: it joins like
 * hb_batch_stream, so work enqueued on the batch's stream afterwards sees the step calls made so far. */
int hb_body_acc_readout(hb_batch* b, int on);
int hb_get_body_acc(hb_batch* b, float* out);
int hb_body_acc_readout_dev(hb_batch* b, const float** body_acc_dev);

/* ---- env adapter: the 27-DoF analogue of CPUEnv.step/reset (simulation/cpu_env.py:374-416,656-693) --------- */

#define HB_ENV_MAX_PAIRS 16
/* Reward / termination parameters of standupReward (simulation/reward_functions.py:247-374), made explicit.
 * hb_env_default_config fills the reference's weights and model-derived heights. */
typedef struct hb_env_config {
  float target_velocity[2];     /* control_input_velocity (cpu_env.py:593) */
  float target_z, min_z;        /* TARGET_Z_POS / MIN_Z_POS_FOR_REWARD (reward_functions.py:303-305) */
  float max_time;               /* MAX_SIM_TIME_STANDUP; <= 0 disables the time limit */
  float safe_torque;            /* MAX__SAFE_JOINT_TORQUE */
  float control_frequency;      /* CONTROL_FREQUENCY (simulation_parameters.py:51) */
  float action_scale;           /* previous/latest action are divided by this (pi/2 at cpu_env.py:601-602) */
  float w_hvel, w_upright, w_height, w_torque, w_ctrl_change, w_ctrl_reg, w_symmetry;
  float self_collision_penalty; /* SELF_COLLISION_PENALTY */
  float terminal_reward;        /* TERMINAL_REWARD (overrides the step reward at the time limit) */
  float upright_tol;            /* success needs max|g_local[0:2]| below this (0.7) */
  int n_equal, n_opposite;      /* actuator index pairs of symmetry_reward (reward_functions.py:98-113) */
  int equal_pairs[HB_ENV_MAX_PAIRS][2];
  int opposite_pairs[HB_ENV_MAX_PAIRS][2];
  int auto_reset;               /* 1: envs that terminate/truncate are reset inside hb_env_step (VecEnv semantics) */
  int reset_keyframe;           /* -1 = qpos0 */
  float reset_perturb;          /* 0..1 scale of the Halton joint/height perturbation (randomization_factor) */
  /* 0: standupReward semantics (terminated = time limit, with terminal_reward; truncated = success),
   * 1: controlInputReward semantics (reward_functions.py:116-245: terminated = fallen over or torso below
   *    min_z_grounded, with terminal_reward; truncated = time limit) */
  int reward_kind;
  float w_vvel;                 /* VERTICAL_VELOCITY_PENALTY_WEIGHT (0 for standupReward) */
  float min_z_grounded;         /* MIN_Z_BEFORE_GROUNDED */
  /* reset-until-collision-free (cpu_env.py:411-414: reset steps once and starts over while anything collides):
   * 0 off, 1 any contact (the reference's test), 2 self-collision only; hb_env_reset only, at most 8 draws */
  int reset_collision_mode;
  /* CPUEnv._randomize_starting_position also perturbs the root quaternion, +-QUAT_INITIAL_OFFSET_MAX (0.1) per component, scaled by
   * reset_perturb like the rest (cpu_env.py:300-328; the result is not renormalised there either: mj_kinematics does that) */
  float reset_quat_perturb;
  /* 0: the joint entries of the observation are in joint order; 1: in ACTUATOR order, the reference's JOINT_NAMES order
   * (simulation_parameters.py:84-103 = the <motor> order of assets/humanoid.xml:97-110): needs one actuator per scalar joint */
  int obs_actuator_order;
} hb_env_config;

int hb_env_default_config(const hb_model* m, hb_env_config* out);
/* The reference's own values for its own robot (simulation/assets/world.xml + humanoid.xml; reward_functions.py:289-372,
 * simulation_parameters.py:51-103): TARGET_Z_POS -0.375, MIN_Z_POS_FOR_REWARD -0.6, safe torque 1 N m, 500 Hz, the symmetry pairs
 * by joint name (equal: elbows; opposite: hip roll, hip pitch, knee, shoulder pitch, shoulder roll), observation in JOINT_NAMES
 * order, reset = keyframe "standup_reset" if the model has it (lying on the floor: INITIAL_QUAT_STANDUP, Z_INITIAL_POS_STANDUP) with
 * the joint / height / quaternion perturbations of CPUEnv.reset.  HB_EINVAL if the model lacks the reference's joint names. */
int hb_env_team_config(const hb_model* m, hb_env_config* out);
int hb_env_configure(hb_batch* b, const hb_env_config* cfg);

/* Sensor / actuation realism of CPUEnv (cpu_env.py:135-186,465-545,612-674; values of simulation_parameters.py:5-48),
 * all on the device and per env.  `factor` is the reference's randomization_factor and scales every magnitude.
 *  - action noise, then an integer-step action delay FIFO (filled with zeros at reset);
 *  - observation noise on joint angles / velocities, gyro, and the torso quaternion before the gravity vector is
 *    taken, then one delay FIFO per channel group (joints, gyro, gravity; fillers 0 / 0 / (0,0,-1));
 *  - delays are drawn per env and episode: round(U(min_delay, max_delay) * factor / control_timestep) steps;
 *  - pushes: a horizontal force of U(min,max)*factor N on a random body for U(duration) s every U(interval) s,
 *    through xfrc_applied (cpu_env.py:612-654).
 * Random numbers are a counter-based hash of (seed, global env index, episode, step, stream, element), so a run
 * is reproducible and independent of the batch split across GPUs.  frozen_noise = 1 reproduces a quirk of the
 * reference (its PRNG key is never split, so every step of an episode adds the same noise vector). */
typedef struct hb_env_randomization {
  float factor;
  unsigned int seed;
  float control_timestep;      /* seconds per hb_env_step call; <= 0: the model's timestep */
  float joint_angle_noise;     /* rad   (JOINT_ANGLE_NOISE_STDDEV, degrees in the reference) */
  float joint_velocity_noise;  /* rad/s (JOINT_VELOCITY_NOISE_STDDEV) */
  float gyro_noise;            /* rad/s (GYRO_NOISE_STDDEV) */
  float imu_noise;             /* added to each torso quaternion component (IMU_NOISE_STDDEV in rad) */
  float action_noise;          /* rad   (JOINT_ACTION_NOISE_STDDEV) */
  float min_delay, max_delay;  /* s */
  int frozen_noise;
  int push_enabled;
  float push_min_interval, push_max_interval, push_min_duration, push_max_duration, push_min_force, push_max_force;
} hb_env_randomization;

/* The reference's values (factor = 1, pushes on, fresh noise every step). */
int hb_env_default_randomization(const hb_model* m, hb_env_randomization* out);
/* Installs (cfg != NULL and cfg->factor > 0) or removes the above; takes effect at the next hb_env_reset
 * (call it before resetting).  Delays beyond 63 control steps are refused. */
int hb_env_randomize(hb_batch* b, const hb_env_randomization* cfg);
/* Domain randomisation of the model per env and episode (cpu_env.py:188-264, values of simulation_parameters.py:5-37),
 * drawn on the device at hb_env_reset and at every auto-reset, all scaled by `factor` as in the reference:
 *  - body masses += U(-max_mass_change, +max_mass_change) (floor 1e-5 kg) and one random body += U(0, max_external_mass);
 *    like the reference, derived constants (inverse weights, subtree masses) are NOT recomputed;
 *  - floor sliding friction *= (1 - factor) + U(friction_min_mult, friction_max_mult) * factor   (first plane geom);
 *  - per hinge/slide joint: armature += U(0, armature_max_change), stiffness += U(0, stiffness_max_change),
 *    limit margin += U(0, margin_max_change), each limit bound += U(-range_max_change, +range_max_change);
 *  - per actuator: force range bounds += U(-force_limit_max_change, +...); if kp_nominal > 0 the gain becomes
 *    kp_nominal + U(-kp_max_change, +kp_max_change) and, for actuators with an affine bias, biasprm[1] = -gain.
 * Random numbers come from the same counter-based generator as hb_env_randomization (seed, global env, episode). */
typedef struct hb_domain_randomization {
  float factor;
  unsigned int seed;
  float friction_min_mult, friction_max_mult;
  float max_mass_change, max_external_mass;
  float armature_max_change, stiffness_max_change, margin_max_change, range_max_change;
  float kp_nominal, kp_max_change, force_limit_max_change;
  float floor_bump_min, floor_bump_max;  /* height fields: per-env elevations, smooth noise scaled to [0, min + factor (max - min)]
                                            (CPUEnv._randomize_floor_heightmap, cpu_env.py:267-280); max = 0: the model's own data */
} hb_domain_randomization;
/* The reference's values (factor = 1, kp_nominal = 0: gains stay the model's — JOINT_P_GAIN = 2 is the team robot's). */
int hb_env_default_domain_randomization(const hb_model* m, hb_domain_randomization* out);
/* Installs (cfg != NULL and cfg->factor > 0) or removes per-env model parameters; call before hb_env_reset. */
int hb_env_domain_randomize(hb_batch* b, const hb_domain_randomization* cfg);
/* Current per-env parameters, for inspection: out[n_env][stride] with per env
 * mass[nbody] | armature[nv] | stiffness[nv] | limit margin[nlim] | limit bound[nlim] | gain[nu] | biasprm1[nu] |
 * forcerange[2 nu] | floor friction scale | hfield_data[nhfielddata]; returns stride (also when out == NULL), 0 when off. nlim = 2 per limited
 * joint / tendon in constraint order (lower, upper). */
int hb_env_get_domain_params(hb_batch* b, float* out);

/* CPUEnv.reset for every env: returns obs[n_env][nobs]. */
int hb_env_reset(hb_batch* b, float* obs);
/* CPUEnv.step: action[n_env][nu] -> ctrl (unscaled; the physics clamps to ctrlrange), n_substeps x mj_step,
 * reward, termination, observation; finished envs are reset when auto_reset is set and then report the
 * observation of their new episode. Host pointers.  The four outputs are one record on the device ([obs | reward | terminated |
 * truncated]); a caller whose four buffers lie back to back in that order (reward == obs + n_env * nobs, terminated ==
 * (uint8_t*)(reward + n_env), truncated == terminated + n_env; page-locked for a DMA transfer: hb_host_alloc) gets them in ONE
 * device-to-host transfer, anyone else in four. */
int hb_env_step(hb_batch* b, const float* action, int n_substeps, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated);
/* The observations of the states episodes ENDED in.  hb_env_step resets a finished env in place and reports the first observation of its
 * new episode; stable-baselines3's vectorised envs (the reference trains through DummyVecEnv: rl/train.py:134-136) keep the last
 * observation of the old one as infos[i]["terminal_observation"], and its off-policy learners bootstrap from it when the episode was
 * truncated - which in the reference's standupReward is the SUCCESS case (reward_functions.py:371-372, cpu_env.py:686-693).  The first call
 * (terminal_obs may be NULL) switches the recording on; from the next hb_env_step on, row e of the [n_env][nobs] table is rewritten
 * whenever env e finishes an episode (same sensor model, noise and delays as that episode's other observations) and keeps its value
 * otherwise.  With a non-NULL pointer the table is copied to the host (after the steps enqueued so far). */
int hb_env_terminal_obs(hb_batch* b, float* terminal_obs);
/* The same, enqueued only: VecEnv.step_async of the reference's training loop (stable-baselines3 VecEnv: step_async() then
 * step_wait(); rl/train.py:134-136 builds a DummyVecEnv whose step() is that pair).  The action buffer must stay untouched and the
 * output buffers unread until hb_batch_sync(b) returns (= step_wait); page-locked buffers (hb_host_alloc) make the copies truly
 * asynchronous.  The host is free in between - e.g. to run the learner's update. */
int hb_env_step_async(hb_batch* b, const float* action, int n_substeps, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated);
/* Same with device pointers, asynchronous on the batch's stream (policy on the same GPU). */
int hb_env_step_dev(hb_batch* b, const float* action_dev, int n_substeps, float* obs_dev, float* reward_dev, uint8_t* terminated_dev, uint8_t* truncated_dev);

/* ---- observation extension: the last action and the height scan in every observation the adapter produces ------------------------ */

/* Appends to the model's observation, on the device, what a perceptive policy needs beside it.  Every row the env adapter writes is then
 *   [ base (the model's nobs) | prev_action (nu) | scan (n_ray) ]        hb_env_nobs floats; a part that is off is absent
 *                                                                        (observed velocity commands add three entries behind these:
 *                                                                        hb_env_commands, below)
 *   prev_action  the action the env last applied - the adapter's `latest`, which the reward's control-change term reads: behind the
 *                realism layer's action noise and delay where that is on; zero after a reset
 *   scan         one entry per installed ray (hb_ray_configure), in ray order: clamp(scan_scale * (scan_offset - d), scan_lo, scan_hi),
 *                d the ray's distance at the env's state, or the configuration's cutoff where nothing is hit.  With scan_offset = the
 *                height the rays start above the body this is the terrain height relative to the body origin.  fp32: a subtract, a
 *                multiply, a clamp, each rounded once (no fused multiply-add); d has the bits hb_rays gives at that state.
 * The model's nobs does not change: hb_model queries, hb_policy_set_mlp, hb_policy_eval and hb_rollout_policy never go through the
 * adapter and keep the base observation.  The base part keeps its realism layer (noise, delay lines) exactly; extension entries get
 * NO noise and NO delay.
 * Producers - all write rows of hb_env_nobs floats: hb_env_reset, hb_env_step, hb_env_step_async, hb_env_step_dev, hb_get_obs,
 * hb_env_terminal_obs, hb_env_collect_dev and hb_env_collect_norm_dev with their obs, terminal_obs and raw_obs tapes.
 * Consumers - all sized by hb_env_nobs: hb_actor_set_mlp and hb_critic_set_mlp (sizes[0]), hb_q_set_mlp (sizes[0] - nu), the
 * normaliser's record with hb_norm_* (their existing limit applies: nobs <= 240), hb_collect_gae_dev, the PPO and SAC learners.
 * An episode that ends with auto_reset on: the terminal observation carries the extension of the state the episode ended in - the
 * action just applied and the scan at the pre-reset state, with terrain randomisation over the OLD elevations; the observation of the
 * new episode carries a zero last action and the scan at the reset state over the NEW elevations.
 * With a scan an evaluation of the envs is: the poses the rays need and the ray kernel at the post-step state, the env kernel, and - where
 * envs may reset - the same two launches masked to the envs that did, writing straight into their observation rows.  Without an extension the
 * adapter makes exactly the launches it made before and gives the same bits.  No atomics: a scan entry is a function of the env's
 * state, its elevations and the ray alone.  hb_last_kernel goes on naming the step kernel.
 * Order of calls: before anything sized by the observation is installed.  HB_EINVAL: an actor, critic, Q network, normaliser or learner
 * exists; height_scan with no rays installed or with a ray configuration whose cutoff <= 0; scan_lo > scan_hi; a non-finite parameter.
 * While the scan is part of the observation, hb_ray_configure with another n_ray, a cutoff <= 0 or a removal is refused with HB_EINVAL;
 * the same n_ray with new rays is allowed.  A refused call changes nothing.  NULL or an all-zero struct removes the extension. */
typedef struct hb_obs_ext {
  int prev_action;        /* 1: append the nu entries of the action the env last applied (the adapter's `latest`; 0 after a reset) */
  int height_scan;        /* 1: append one entry per installed ray (hb_ray_configure), in ray order */
  float scan_offset, scan_scale, scan_lo, scan_hi;
} hb_obs_ext;
int hb_env_obs_extend(hb_batch* b, const hb_obs_ext* ext);   /* NULL or all-zero: remove */
int hb_env_nobs(hb_batch* b);                                /* the width of a row: hb_env_row's `width` */
/* The layout of every row the adapter writes, [ base | prev_action | scan | foot_contact | command ]: the offset and the count of each
 * part (a part that is off has count 0; base begins at 0) and the width.  Read-only; HB_EINVAL for a NULL argument.  (The struct has
 * no typedef: the function bears the name, so the type is written `struct hb_env_row`.) */
struct hb_env_row {
  int base;
  int prev_action, n_prev_action;
  int scan, n_scan;
  int foot_contact, n_foot_contact;
  int command, n_command;
  int width;
};
int hb_env_row(hb_batch* b, struct hb_env_row* out);

/* ---- velocity commands: every env follows its own commanded planar velocity and yaw rate, drawn, tracked and observed on the device -- */

/* With a configuration installed every env owns a current command (cx, cy, cyaw) - m/s, m/s, rad/s - and the number k of draws made
 * so far in its episode, in a device buffer of the batch (16 bytes per env).
 *   draw     Draw k of episode ep of global env g (the batch's env offset + e) comes from the counter-based generator of
 *            hb_env_randomization: u_i = uniform(seed, g, ep, k, stream 40, i), i = 0..3.  u_0 < zero_fraction: the command is (0, 0, 0).
 *            Otherwise component c is lo_c + u_{c+1} * (hi_c - lo_c) in fp32: a subtract, a multiply, an add, each rounded once (no fused
 *            multiply-add).  A draw depends on (seed, g, ep, k) alone: the same bits on any split of a batch and in any order of envs.
 *   when     Draw 0 at every episode start: in hb_env_reset (with the episode number the env ends up with after the collision
 *            re-draws of reset_collision_mode) and at an auto-reset inside the env kernel.  Inside an episode, with resample_time > 0,
 *            the env kernel of hb_env_step* / hb_env_collect* redraws after the step's reward and termination are formed: an env that did
 *            not reset and whose state time (fp32) >= (float)k * resample_time (an fp32 product) makes draw k and sets k += 1.  At most
 *            one draw per env step.  hb_get_obs and the settle step of hb_env_reset never draw.
 *   reward   A step is rewarded against the command that was in force during it - the one the policy saw in obs[t]; the terminal
 *            observation of an episode carries that command, obs[t+1] the new one (or draw 0 of the new episode).
 *            The linear term of hb_env_config becomes w_hvel * scaled_exp(|v - (cx, cy)|^2): frame 0, v = the root's world-frame
 *            (vx, vy) as before; frame 1, the same vector in the root body's heading frame - the definition of HB_RAY_FRAME_YAW: the
 *            root's x axis flattened onto the world xy plane, unit (c, s), (1, 0) below a flattened length of 1e-6; v = (c vx + s vy,
 *            -s vx + c vy).  A term w_yaw * scaled_exp((wz - cyaw)^2) is added, wz = the world z component of the root's angular
 *            velocity (the free joint's angular velocity is in the body frame: wz = R[2][0] w0 + R[2][1] w1 + R[2][2] w2).  Every other
 *            term, termination, truncation, terminal_reward and auto-reset stay as they are.  hb_env_config.target_velocity is IGNORED
 *            while commands are installed.
 *   observe  1: every row the adapter writes becomes [ base | prev_action | scan | command(3) ] - the command last, so the offsets of
 *            hb_env_obs_extend do not move - and hb_env_nobs grows by 3.  Command entries get NO noise and NO delay.  Producers and
 *            consumers are those hb_env_obs_extend lists (hb_get_obs, the terminal-observation table and the collection tapes among the
 *            producers; the normaliser's limit of 240 entries still applies).  hb_policy_set_mlp, hb_policy_eval and hb_rollout_policy
 *            keep the base observation.
 * Without a configuration the adapter makes exactly the launches it made before and gives the same bits; with one it makes the same
 * number of launches per step, and hb_env_reset one small launch more (the draws).  No atomics.
 * Refusals, all HB_EINVAL, each leaving everything as it was and its reason in hb_error(): a NULL batch; a non-finite field; a min above
 * its max; zero_fraction outside [0, 1]; frame or observe other than 0 or 1; a model whose observation has no free root; a call that
 * would change the observation width (observe 0 -> 1, 1 -> 0, or a removal with observe on) while an actor, critic, Q network,
 * normaliser or learner exists - the rule of hb_env_obs_extend; hb_env_get_commands / hb_env_set_commands with nothing installed (or a
 * NULL array).  Changing ranges, weights, frame or resample_time of an installed configuration is always allowed: the current commands
 * and counters stay, ranges and resample_time act from the next draw, weights and frame from the next step.  Installing draws draw 0
 * of every env's current episode at once. */
typedef struct hb_env_commands {
  unsigned seed;
  float vx_min, vx_max, vy_min, vy_max;   /* m/s   */
  float yaw_min, yaw_max;                 /* rad/s */
  float resample_time;    /* s of env time between draws inside an episode; <= 0: one draw per episode */
  float zero_fraction;    /* in [0,1]: probability that a draw is the zero command (stand still) */
  float w_yaw;            /* weight of the yaw-rate term; w_hvel of hb_env_config keeps weighting the linear term */
  int   frame;            /* 0: world axes (the frame the reward uses without commands); 1: the root body's heading frame */
  int   observe;          /* 1: append (vx, vy, yaw) to every observation row the adapter writes */
} hb_env_commands;
/* seed 0, vx in [-1, 1], vy in [-0.5, 0.5], yaw in [-1, 1], a draw every 5 s, a tenth of the draws zero, w_yaw = half of the default
 * w_hvel, heading frame, observed.  HB_EINVAL: NULL argument. */
int hb_env_default_commands(const hb_model* m, hb_env_commands* out);
/* The checks of hb_env_commands_configure that need no batch: the fields, and the model's free root.  HB_OK or HB_EINVAL with hb_error(). */
int hb_env_commands_check(const hb_model* m, const hb_env_commands* cfg);
int hb_env_commands_configure(hb_batch* b, const hb_env_commands* cfg);   /* NULL: remove */
int hb_env_get_commands(hb_batch* b, float* out);                         /* host [n_env][3], behind the enqueued work */
/* For evaluation and teleoperation: overwrites the current command of the chosen envs (mask NULL: all; else [n_env], non-zero = chosen).
 * The draw counters do not move, so the next scheduled draw replaces the command as usual. */
int hb_env_set_commands(hb_batch* b, const float* cmd, const uint8_t* mask); /* host [n_env][3]; mask NULL = all */
/* Why the calling thread's last hb_env_*commands* call was refused ("" when it was not): a static string, valid until that thread's
 * next such call. */
const char* hb_error(void);

/* ---- foot-contact terms: air time, impacts, stumbles, collisions and contact resets, computed in the env kernel ------------------ */

/* With a configuration installed the env kernel reads the per-body contact read-out (hb_contact_readout, which the configure call
 * switches on; hb_contact_readout(b, 0) is then refused with HB_EINVAL and a reason in hb_error()) and every env owns one 32-byte
 * record in a device buffer of the batch: t_last[4] (fp32, the env time at which foot f was last evaluated in contact), a mask word
 * (bit f: foot f was in contact at the last step evaluation) and padding.
 * Below, "one rounding" means a single fp32 multiply, add or subtract with no fused multiply-add, so that every discrete decision is
 * reproducible bit for bit in numpy float32 (tests/feet_ref.py restates all of this).  F = the first three entries of the body's
 * hb_get_body_contact row, the read-out of the last physics substep; t = the env's fp32 state time at the evaluation, before any reset.
 *   in contact   n2 = (Fx*Fx + Fy*Fy) + Fz*Fz, each operation one rounding, in that order; c = n2 > thr*thr (thr = contact_threshold, the
 *                product one rounding).  The same test serves feet, penalised bodies and terminal bodies.
 *   air time     air_f = t - t_last[f] (one rounding); touchdown_f = c_f && !(mask bit f).  The term is
 *                w_air_time * gate * sum_f (touchdown_f ? air_f - air_time_target : 0).  gate = 1 when air_gate == 0; otherwise
 *                gate = (cx*cx + cy*cy > air_cmd_min*air_cmd_min), each operation one rounding, on the command in force during the step
 *                (hb_env_commands), or on hb_env_config.target_velocity when no commands are installed.
 *   impact       w_force * sum_f max(sqrt(n2_f) - force_max, 0), over all feet.
 *   stumble      s_f = c_f && (Fx*Fx + Fy*Fy) > (ratio*ratio) * (Fz*Fz), each product and sum one rounding (ratio = stumble_ratio).
 *                The term is w_stumble, once, if any s_f.
 *   collision    w_collision * the number of penalised bodies in contact.
 *   termination  any terminal body in contact: terminated = 1 under both reward_kinds.  It is OR-ed into the termination of
 *                hb_env_config before the terminal reward replaces the step's reward, so terminal_reward and auto_reset act as for
 *                any other termination.
 *   The four terms are ADDED to the reward: penalties carry negative weights.
 *   update       Step evaluations only - the env kernel of hb_env_step* / hb_env_collect*, the evaluations that may reset and that may
 *                redraw a command: t_last[f] = c_f ? t : t_last[f]; the mask becomes the c_f bits.  hb_get_obs, the settle steps and
 *                the final observation of hb_env_reset compute the terms but never write the record.  They do compute them: with
 *                reset_collision_mode != 0 a settle step that ends with a terminal body in contact counts as ending in a terminal
 *                state, and hb_env_reset draws that env again - with a foot among the terminal bodies every standing start is
 *                redrawn for all eight attempts, so keep the feet out of terminal_body when that mode is on.  The final observation
 *                of hb_env_reset evaluates the terms on the read-out of whatever physics step ran last (a settle step, or the last
 *                step before the reset when there is none); its reward and flags are not returned.
 *   episode      At an episode start t_last[f] = the new state's time and all n_feet mask bits are set, so a standing start pays
 *   start        nothing for the first touchdown: at an auto-reset inside the env kernel; in hb_env_reset by one small launch after the
 *                last settle step, with the time each env has then; in hb_env_feet_configure for every env at once.
 *   observe      1: every row the adapter writes becomes [ base | prev_action | scan | foot_contact(n_feet) | command(3) ] - the
 *                command stays last - and hb_env_nobs grows by n_feet.  The entries are the record's mask after the evaluation's update
 *                (a looking evaluation: the record's mask as it is), as 0.f / 1.f, with NO noise and NO delay.  The terminal observation
 *                carries the flags of the state the episode ended in, the first row of the new episode carries ones.  Producers and
 *                consumers are those hb_env_obs_extend lists, and its rule holds: a call that would change the width (observe 0 <-> 1,
 *                another n_feet while observed, a removal with observe on) while an actor, critic, Q network, normaliser or learner
 *                exists is refused.
 * Envs outside a launch's mask keep record, reward and rows.  Without a configuration the adapter makes exactly the launches it made
 * before and gives the same bits; with one a step makes the same number of launches, and hb_env_reset one small launch more.  No atomics.
 * A batch with feet steps in the full step kernel, as any batch with the contact read-out does (profiles/contact_readout_bench.txt).
 * Not provided: foot slip (it needs body velocities: a kinematics launch per step), contact filtering over several steps, per-foot
 * weights.
 * Refusals, all HB_EINVAL, each leaving everything as it was and its reason in hb_error(): a NULL batch; n_feet outside 1..4,
 * n_penalised or n_terminal outside 0..8; a body id outside 1..nbody-1; a body named twice in foot_body; a non-finite field;
 * contact_threshold <= 0; air_cmd_min < 0; stumble_ratio < 0; air_gate or observe other than 0 or 1; the width rule above;
 * hb_env_get_feet with nothing installed.  If the read-out cannot be had for the batch, that error is passed on and nothing changes. */
#define HB_ENV_MAX_FEET 4
#define HB_ENV_MAX_CONTACT_BODIES 8
typedef struct hb_env_feet {
  int   n_feet;       int foot_body[HB_ENV_MAX_FEET];                      /* body ids, 1 <= n_feet <= 4 */
  int   n_penalised;  int penalised_body[HB_ENV_MAX_CONTACT_BODIES];       /* a contact costs w_collision each */
  int   n_terminal;   int terminal_body[HB_ENV_MAX_CONTACT_BODIES];        /* a contact ends the episode */
  float contact_threshold;   /* N: a body is "in contact" when |F| of its hb_get_body_contact row exceeds it (> 0) */
  float w_air_time, air_time_target;  /* s */
  int   air_gate;  float air_cmd_min;   /* 1: the air-time term counts only while the commanded planar speed > air_cmd_min (>= 0) */
  float w_force, force_max;  /* N */
  float w_stumble, stumble_ratio;
  float w_collision;
  int   observe;             /* 1: append n_feet contact flags (0.f / 1.f) to every row the adapter writes */
} hb_env_feet;
/* n_feet 0 and empty lists - the caller names the bodies -, threshold 1 N, w_air_time 1 with a target of 0.5 s, the gate on at 0.1 m/s,
 * w_force -0.01 per N above force_max = 2 x the model's weight (total mass x |gravity|), w_stumble -1 at a ratio of 5, w_collision -1,
 * observe 0.  HB_EINVAL: NULL argument. */
int hb_env_default_feet(const hb_model* m, hb_env_feet* out);
/* The checks of hb_env_feet_configure that need no batch: counts, body ids and fields.  HB_OK or HB_EINVAL with hb_error(). */
int hb_env_feet_check(const hb_model* m, const hb_env_feet* cfg);
int hb_env_feet_configure(hb_batch* b, const hb_env_feet* cfg);    /* NULL: remove (the read-out stays on) */
int hb_env_feet_count(hb_batch* b);                                /* n_feet of the installed configuration; 0: none (or a NULL batch) */
/* host [n_env][n_feet] each (n_feet: hb_env_feet_count), either nullable, behind the enqueued work: the records' t_last and contact bits (0 / 1) */
int hb_env_get_feet(hb_batch* b, float* t_last, uint8_t* contact);

/* ---- policy in the loop (BASELINE.json configs[3]: MLP policy inference fused into the rollout loop) ---------- */

/* Installs an MLP policy obs[nobs] -> sizes[1] -> ... -> sizes[n_layers] == nu with tanh after every layer (hidden
 * layers: or what hb_mlp_set_activation chooses)
 * (sizes and activation of simulation/hyperparam_config.py:21-27, rl/train.py:163-167).  weights[l] is row-major
 * [sizes[l]][sizes[l+1]] float32 (the transpose of torch.nn.Linear.weight), biases[l] is [sizes[l+1]].  Host pointers;
 * copied to the device.  n_layers <= 4, every size <= 512. */
int hb_policy_set_mlp(hb_batch* b, int n_layers, const int* sizes, const float* const* weights, const float* const* biases);
/* One policy evaluation on the current states: ctrl_out[n_env][nu] (host, nullable) and the batch's control buffer. */
int hb_policy_eval(hb_batch* b, float* ctrl_out);
/* T closed-loop steps on the device: observation -> MLP (f32 MFMA GEMMs) -> mj_step, no host round trip.
 * qpos_out_dev (nullable, device) receives [T][n_env][nq]. */
int hb_rollout_policy(hb_batch* b, int T, float* qpos_out_dev);

/* ---- actor and rollout collection: a sampling policy in the env loop, with tapes of what happened ------------------------------ */

#define HB_ACTOR_DETERMINISTIC 0  /* action = tanh(last layer): hb_policy_eval's network, no sampling */
#define HB_ACTOR_GAUSSIAN 1       /* action = mean + exp(log_std[i]) * eps; the last layer is linear; log_std is state independent (SB3 PPO / A2C) */
#define HB_ACTOR_SQUASHED 2       /* the last layer is linear and 2 nu wide: mean | log_std; log_std is clamped to [-20, 2];
                                     action = tanh(mean + exp(log_std) * eps)  (SB3 SAC's actor - what the reference trains) */
typedef struct hb_actor_config {
  int head;              /* HB_ACTOR_* */
  unsigned seed;
  float log_std[32];     /* HB_ACTOR_GAUSSIAN: one per actuator (nu <= 32) */
  int deterministic;     /* 1: eps = 0 for every head (evaluation rollouts) */
} hb_actor_config;

/* Installs the actor of hb_env_collect_dev: an MLP obs[nobs] -> sizes[1] -> ... -> sizes[n_layers] with tanh (or what hb_mlp_set_activation chooses) after every hidden layer; the
 * last layer has tanh for head 0 and is linear for heads 1 and 2.  sizes[0] == nobs; sizes[n_layers] == nu for heads 0 and 1 and 2 nu for
 * head 2.  weights[l] is row-major [sizes[l]][sizes[l+1]] float32 (the transpose of torch.nn.Linear.weight), biases[l] is [sizes[l+1]];
 * host pointers, copied to the device.  The actor is separate from the MLP of hb_policy_set_mlp: either may be installed or replaced
 * without touching the other.  Installing an actor sets the batch's draw counter (below) back to 0.
 * Refusals: HB_EINVAL - NULL argument, n_layers outside 1..4, a size < 1, sizes[0] or sizes[n_layers] not as above, a head that is none
 * of HB_ACTOR_*, nu > 32, a non-finite log_std[i] (i < nu, head 1); HB_EUNSUPPORTED - a width above 256: the actor is one fused kernel
 * whose activation tiles live in LDS, and there is no layer-by-layer fallback.  A refused call leaves the installed actor as it was. */
int hb_actor_set_mlp(hb_batch* b, int n_layers, const int* sizes, const float* const* weights, const float* const* biases, const hb_actor_config* cfg);

typedef struct hb_collect_out {   /* device pointers; every field but obs and action may be NULL */
  float* obs;           /* [T + 1][n_env][nobs]  row 0 is INPUT, written by the caller (see below) */
  float* action;        /* [T][n_env][nu]        what was handed to the env adapter */
  float* mean;          /* [T][n_env][nu]        the head's mean (head 0: equal to action) */
  float* log_std;       /* [T][n_env][nu]        HB_ACTOR_SQUASHED: the clamped log_std */
  float* eps;           /* [T][n_env][nu]        the N(0, 1) draws (zeros when deterministic) */
  float* reward;        /* [T][n_env] */
  uint8_t* terminated;  /* [T][n_env] */
  uint8_t* truncated;   /* [T][n_env] */
  float* terminal_obs;  /* [T][n_env][nobs]      row (t, e) is meaningful where env e finished at step t */
} hb_collect_out;

/* T env steps with the actor in the loop, all enqueued on the batch's stream: no host synchronisation, no host transfer.  For
 * t = 0 .. T-1: the actor kernel reads obs[t] and writes mean[t], log_std[t], eps[t] (those given) and action[t]; then exactly
 * hb_env_step_dev(b, action[t], n_substeps, obs[t+1], reward[t], terminated[t], truncated[t]) - action noise and delay, pushes, physics,
 * reward, termination, auto-reset (an env that finishes at step t is reset in place and obs[t+1] holds the first observation of its new
 * episode), the realism layer on the observation.  With terminal_obs the recording of hb_env_terminal_obs is switched on if it is not
 * yet, and after step t the batch's terminal-observation table is copied (device to device) into terminal_obs[t]: rows of envs that did
 * NOT finish at t hold older values (the table's row of an env changes only when that env finishes; zeros before its first end).
 * obs[0] is supplied by the caller: the observation the env last returned - from hb_env_reset, the last hb_env_step*, or row T of the
 * previous collection.  The library keeps no hidden current observation, so the call is a pure function of the batch, the actor and
 * obs[0].  eps[t][e][i] is the existing counter-based normal draw (seed = cfg.seed, env = the batch's env offset + e, episode 0,
 * step = draw0 + t, stream RS_ACTOR = 32 - the realism layer uses 1..8, domain randomisation 16..25 -, element i), where draw0 counts the
 * steps collected since hb_actor_set_mlp: reproducible, the same on any split of a batch across GPUs, independent of the env adapter's
 * noise.  hb_last_kernel names the step kernel; hb_batch_step_launches counts as for hb_env_step_dev.
 * HB_EINVAL: NULL b or out, T < 1, n_substeps < 1, NULL obs or action, no actor installed, a log_std tape with a head other than 2. */
int hb_env_collect_dev(hb_batch* b, int T, int n_substeps, const hb_collect_out* out);

/* ---- PPO buffer over the tapes of a collection: critic values, log-probabilities, GAE(gamma, lambda) advantages and returns ---- */

/* Installs the critic of hb_collect_gae_dev: an MLP obs[nobs] -> sizes[1] -> ... -> sizes[n_layers] == 1 with tanh (or what hb_mlp_set_activation chooses) after every hidden layer
 * and a linear last layer.  The weight conventions are hb_actor_set_mlp's: weights[l] is row-major [sizes[l]][sizes[l+1]] float32 (the
 * transpose of torch.nn.Linear.weight), biases[l] is [sizes[l+1]]; host pointers, copied to the device and packed.  The critic is
 * independent of the actor and of the MLP of hb_policy_set_mlp: any of them may be installed or replaced without touching the others.
 * Refusals: HB_EINVAL - NULL argument, n_layers outside 1..4, a size < 1, sizes[0] != nobs, sizes[n_layers] != 1; HB_EUNSUPPORTED - a
 * width above 256 (the critic is the actor's fused kernel design: activation tiles in LDS, no layer-by-layer fallback).  A refused call
 * leaves the installed critic as it was. */
int hb_critic_set_mlp(hb_batch* b, int n_layers, const int* sizes, const float* const* weights, const float* const* biases);

typedef struct hb_gae_config {
  float gamma, lam;          /* discount and GAE lambda, each in [0, 1] */
  int bootstrap_truncated;   /* 1: an env cut by truncation alone gets gamma V(terminal_obs) added to its reward (VecEnv's TimeLimit.truncated) */
} hb_gae_config;
typedef struct hb_gae_out {  /* device pointers, each nullable, not all NULL */
  float* value;           /* [T + 1][n_env]  V(obs[t]) */
  float* terminal_value;  /* [T][n_env]      V(terminal_obs[t][e]) where the env is bootstrapped at (t, e), 0 elsewhere */
  float* log_prob;        /* [T][n_env] */
  float* advantage;       /* [T][n_env] */
  float* returns;         /* [T][n_env]      advantage + value[t] */
} hb_gae_out;

/* What a PPO update needs from the T-step tapes of hb_env_collect_dev (`tapes`: the struct that collection was given, or any tapes of
 * the same shapes), computed on the device in at most four launches on the batch's stream: no host synchronisation, no host transfer,
 * no allocation beyond a scratch the batch owns and grows on demand.  A pure function of the tapes, the installed critic and the
 * installed actor's head (cfg.head, and for HB_ACTOR_GAUSSIAN its log_std[]): nothing of the batch is written - state, draw counter,
 * status words, counts, hb_last_kernel and hb_batch_step_launches stay as they are (held hb_step_dev calls are launched first and the
 * pipes joined, as for every other call).  With done = terminated | truncated, boot = bootstrap_truncated && truncated && !terminated:
 *   value[t][e]          = V(obs[t][e])                                   t = 0..T
 *   terminal_value[t][e] = boot ? V(terminal_obs[t][e]) : 0
 *   r'                   = reward[t][e] + gamma * terminal_value[t][e]
 *   nt                   = done ? 0 : 1
 *   delta                = r' + gamma * nt * value[t+1][e] - value[t][e]
 *   advantage[t][e]      = delta + gamma * lam * nt * advantage[t+1][e],      advantage[T] = 0
 *   returns[t][e]        = advantage[t][e] + value[t][e]
 * - stable-baselines3's on-policy semantics (collect_rollouts' bootstrap of truncated envs, RolloutBuffer.compute_returns_and_advantage).
 * obs[t+1] of an env that finished at t is the first observation of its NEW episode (the auto-reset): value[t+1] is masked by nt there.
 * What terminated and truncated mean depends on hb_env_config.reward_kind; where both are set the env is not bootstrapped.
 * terminal_obs rows where boot is not set are NOT READ (they hold older values or whatever the caller left there).
 * log_prob[t][e], with ls_i the actor's log_std[i] (head 1) or the log_std tape (head 2):
 *   head 1: sum_i (-eps_i^2 / 2 - ls_i - log(2 pi) / 2)          - the normal log-density of action, (action - mean) / sigma being eps;
 *   head 2: the same sum minus sum_i 2 (log 2 - x_i - softplus(-2 x_i)), x_i = mean_i + exp(ls_i) eps_i - the change of variables of
 *           tanh, log(1 - tanh(x)^2), written so that it does not cancel near |action| = 1.  SB3 writes log(1 - a^2 + 1e-6) on the
 *           squashed action instead: the two differ only where 1 - a^2 is of the order of 1e-6 (|x| above about 7);
 *   head 0 has no density: a non-NULL log_prob is refused.
 * Each env's column is computed by one lane from that env's rows alone, and a row's value does not depend on its neighbours: env e's
 * results are the same bits whatever n_env is and wherever e stands in the batch.
 * Tapes read per output (others may be NULL): value - obs; advantage, returns - obs, reward, terminated, truncated, and terminal_obs
 * when bootstrap_truncated; terminal_value - terminal_obs, terminated, truncated (all zeros without bootstrap_truncated); log_prob -
 * eps, and mean and log_std for head 2.
 * HB_EINVAL: NULL b, tapes, cfg or out; T < 1; all outputs NULL; gamma or lam not finite or outside [0, 1]; a tape missing for a
 * requested output; value, terminal_value, advantage or returns without a critic; log_prob without an actor or with head 0.  A refused
 * call writes nothing. */
int hb_collect_gae_dev(hb_batch* b, int T, const hb_collect_out* tapes, const hb_gae_config* cfg, const hb_gae_out* out);

/* ---- running observation / reward normalisation and episode statistics on the device (VecNormalize over a VecMonitor) ---- */

/* The semantics are those of stable-baselines3's VecNormalize wrapped around a VecMonitor, restated here [recall: neither package is a
 * dependency of this library; tests/norm_ref.py is the fp64 restatement the kernels are held to].
 * Statistics are fp64: obs_rms = mean[nobs], var[nobs], count; ret_rms = mean, var, count (scalars); all start at mean 0, var 1,
 * count 1e-4.  An UPDATE with n rows of mean mb and biased variance vb does, with d = mb - mean, tot = count + n:
 *   mean += d n / tot;   var = (var count + vb n + d d count n / tot) / tot;   count = tot.
 * One STEP, given the raw obs[n_env][nobs], the raw reward[n_env] and done = terminated | truncated, in this order:
 *   1. training && norm_obs: update obs_rms with the n_env rows of obs (terminal observations never enter an update);
 *   2. obs_out = clip((obs - mean) / sqrt(var + epsilon), -clip_obs, clip_obs) with the statistics after 1 (norm_obs 0: obs_out = obs);
 *   3. training: ret[e] = ret[e] gamma + reward[e] for every env, then update ret_rms with the n_env values of ret (whether or not
 *      norm_reward is set, as SB3 does);
 *   4. norm_reward: reward_out = clip(reward / sqrt(ret_var + epsilon), -clip_reward, clip_reward) with the statistics after 3, else
 *      reward_out = reward;
 *   5. where done, the terminal-observation row is normalised as in 2 with the statistics after 1;
 *   6. the monitor: ep_ret[e] += reward[e] (raw), ep_len[e] += 1; where done, ep_return_out[e] = ep_ret[e], ep_length_out[e] = ep_len[e],
 *      the episode totals advance and ep_ret[e] = ep_len[e] = 0; where not done both outputs are 0;
 *   7. ret[e] = 0 where done.
 * A RESET (VecNormalize.reset) sets ret, ep_ret and ep_len to 0, updates obs_rms with the reset observations when training && norm_obs,
 * and normalises them.
 * Arithmetic: sums, statistics and (x - mean) / sqrt(var + epsilon) in fp64, rounded to fp32 once and clipped in fp32.  The n_env rows
 * are reduced in fixed chunks of 64 consecutive envs, merged in chunk order with the update formula: the same bits run after run, but
 * statistics are PER BATCH - unlike the actor's draws, normalised values are not the same bits on any split of a batch.  Several ranks
 * share statistics through hb_norm_get_stats / hb_norm_set_stats: each rank reads its record, the ranks merge the records with the
 * update formula (n = the other record's count, mb its mean, vb its var), and each rank writes the result back.
 * Non-finite inputs are not special-cased, as in SB3: a NaN or infinity in an observation or reward enters the statistics. */
typedef struct hb_norm_config {
  int norm_obs, norm_reward, training;            /* SB3's defaults: 1, 1, 1 */
  float clip_obs, clip_reward, gamma, epsilon;    /* 10, 10, 0.99, 1e-8 */
} hb_norm_config;
int hb_norm_default_config(hb_norm_config* cfg);
/* Installs the normaliser.  The first installation allocates and initialises the statistics and the per-env accumulators; a later call
 * changes the flags and constants and keeps statistics and accumulators (training = 0: evaluation with frozen statistics).  cfg NULL
 * removes the normaliser with its statistics.  HB_EINVAL: NULL b; clip_obs, clip_reward or epsilon not finite or not positive; gamma
 * not finite or outside [0, 1].  HB_EUNSUPPORTED: nobs above 240 (a chunk of rows is held in LDS).  A refused call changes nothing. */
int hb_norm_configure(hb_batch* b, const hb_norm_config* cfg);
/* VecNormalize.save / load, and the multi-GPU merge above.  The record is 2 nobs + 4 doubles: obs_mean[nobs] | obs_var[nobs] |
 * obs_count | ret_mean | ret_var | ret_count.  Host pointers; both calls run behind the work enqueued so far and end synchronised.
 * HB_EINVAL: NULL argument, no normaliser; set: a non-finite value, a negative var or count (nothing is written then). */
int hb_norm_get_stats(hb_batch* b, double* out);
int hb_norm_set_stats(hb_batch* b, const double* in);
/* The per-env accumulators, each [n_env], each pointer nullable: the discounted return ret, the running episode return and length. */
int hb_norm_get_env(hb_batch* b, double* disc_return, double* ep_return, int32_t* ep_length);
/* out[0..3]: episodes finished, the sum of their (raw) returns, the sum of the squared returns, the sum of their lengths - counted
 * since the first hb_norm_configure (ep_rew_mean = out[1] / out[0], ep_len_mean = out[3] / out[0]). */
int hb_norm_episode_totals(hb_batch* b, double out[4]);

typedef struct hb_norm_io {   /* device pointers; an output may be its input (in place) */
  const float* obs_in;           /* [n_env][nobs] raw */
  float* obs_out;                /* [n_env][nobs] */
  const float* reward_in;        /* [n_env] raw */
  float* reward_out;             /* [n_env], nullable */
  const uint8_t* terminated;     /* [n_env] */
  const uint8_t* truncated;      /* [n_env] */
  const float* terminal_obs_in;  /* [n_env][nobs], nullable (then terminal_obs_out too): only the rows of done envs are read */
  float* terminal_obs_out;       /* [n_env][nobs]: only the rows of done envs are written */
  float* ep_return_out;          /* [n_env], nullable */
  int32_t* ep_length_out;        /* [n_env], nullable */
} hb_norm_io;
/* One step (1 - 7 above) for the batch's n_env rows in two launches on the batch's stream: no host synchronisation, no transfer.
 * HB_EINVAL: NULL b or io, no normaliser, NULL obs_in, obs_out, reward_in, terminated or truncated, only one of terminal_obs_in /
 * terminal_obs_out.  A refused call writes nothing and leaves the statistics as they were. */
int hb_norm_step_dev(hb_batch* b, const hb_norm_io* io);
/* The reset form, for the observations hb_env_reset returned (device pointers, [n_env][nobs], in place allowed). */
int hb_norm_reset_dev(hb_batch* b, const float* obs_in, float* obs_out);
/* VecNormalize.normalize_obs: point 2 with the current statistics on any number of rows, no update (evaluation data, a learner's own
 * buffers).  HB_EINVAL: NULL argument, no normaliser, n_rows < 1. */
int hb_norm_obs_dev(hb_batch* b, const float* in, float* out, long long n_rows);

typedef struct hb_norm_tapes {   /* device pointers, each nullable */
  float* raw_obs;       /* [T][n_env][nobs]  row t is the raw form of obs[t + 1] */
  float* raw_reward;    /* [T][n_env] */
  float* ep_return;     /* [T][n_env]        the return of the episode env e finished at step t, 0 elsewhere */
  int32_t* ep_length;   /* [T][n_env] */
} hb_norm_tapes;
/* hb_env_collect_dev's loop with one hb_norm_step_dev behind every env step, all on the batch's stream (the pipes of a pipelined batch
 * are joined where the actor's launch already joins them).  The actor reads obs[t]; the caller supplies row 0 ALREADY NORMALISED - what
 * hb_norm_reset_dev, hb_norm_step_dev or row T of the previous collection gave.  The env step writes raw values; the normaliser writes
 * obs[t + 1], reward[t] and the rows of terminal_obs[t] whose env finished at t in normalised form (the other rows of terminal_obs[t]
 * keep what the table copy put there: they were never meaningful), and fills the tapes of aux that are given (aux may be NULL).  With
 * norm_obs = norm_reward = 0 the tapes of out equal hb_env_collect_dev's bit for bit.
 * HB_EINVAL: as hb_env_collect_dev, and no normaliser. */
int hb_env_collect_norm_dev(hb_batch* b, int T, int n_substeps, const hb_collect_out* out, const hb_norm_tapes* aux);

/* ---- the PPO learner on the device: clipped surrogate, backward pass, global-norm clipping, Adam ------------------------------ */

/* The update rule is stable-baselines3's PPO.train with separate actor and critic networks and a state-independent log_std
 * (HB_ACTOR_GAUSSIAN), clip_range_vf = None, restated here [neither package is a dependency; tests/ppo_ref.py is the fp64 restatement
 * the kernels are held to].  The data are flattened tapes of n_rows rows (hb_ppo_rows); a minibatch is mb of those rows.  With the
 * current parameters, c = clip_range, s_i = exp(log_std_i):
 *   mu_r = actor(obs_r)   v_r = critic(obs_r)             (tanh after every hidden layer, linear at the top)
 *   lp_r = sum_i ( -(a_ri - mu_ri)^2 / (2 s_i^2) - log_std_i - log(2 pi) / 2 )
 *   A_r  = normalize_advantage && mb > 1 ? (adv_r - mean(adv)) / (std(adv) + 1e-8) : adv_r      (std unbiased, over the minibatch)
 *   d_r  = lp_r - old_log_prob_r,  ratio_r = exp(d_r)
 *   policy_loss  = -mean_r min(A_r ratio_r, A_r clamp(ratio_r, 1 - c, 1 + c))
 *   value_loss   = mean_r (returns_r - v_r)^2
 *   entropy_loss = -sum_i (1/2 + log(2 pi) / 2 + log_std_i)
 *   loss         = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 *   approx_kl    = mean_r ((ratio_r - 1) - d_r),  clip_fraction = mean_r [ |ratio_r - 1| > c ]
 * Gradients are autograd's: dloss/dlp_r = -A_r ratio_r / mb where 1 - c <= ratio_r <= 1 + c (bounds included) or where
 * A_r ratio_r < A_r clamp(ratio_r), else 0; dlp/dmu_ri = (a_ri - mu_ri) / s_i^2; dlp/dlog_std_i = (a_ri - mu_ri)^2 / s_i^2 - 1;
 * dloss/dlog_std_i gains -ent_coef; dloss/dv_r = 2 vf_coef (v_r - returns_r) / mb; back-propagation through the tanh layers.
 * The step (torch.nn.utils.clip_grad_norm_, then torch.optim.Adam without weight decay or amsgrad): g = the 2-norm of ALL gradient
 * entries; max_grad_norm > 0: every entry is scaled by min(1, max_grad_norm / (g + 1e-6)); t += 1; m = b1 m + (1 - b1) grad;
 * v = b2 v + (1 - b2) grad^2; p -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps).  A non-finite g leaves parameters, moments and
 * t untouched and sets the `skipped` statistic.
 * Arithmetic: every matrix product is v_mfma_f32_16x16x4_f32 (exact f32); A_r, the advantage moments, the statistics, the norm and
 * the Adam step are formed in fp64 and rounded to fp32 once.  Every reduction over rows goes over chunks of hb_ppo_row_chunk(mb)
 * consecutive minibatch rows merged in chunk order, the norm over chunks of 4096 entries: no atomics, the same bits run after run. */
typedef struct hb_ppo_config {
  float clip_range;          /* 0.2    > 0 */
  float ent_coef;            /* 0 */
  float vf_coef;             /* 0.5 */
  float max_grad_norm;       /* 0.5    <= 0: no clipping */
  int normalize_advantage;   /* 1 */
  float lr;                  /* 3e-4   >= 0 */
  float beta1, beta2;        /* 0.9, 0.999   in [0, 1) */
  float eps;                 /* 1e-5   > 0 */
} hb_ppo_config;
int hb_ppo_default_config(hb_ppo_config* cfg);

/* Creates the batch's learner: the installed actor (its head must be HB_ACTOR_GAUSSIAN) and critic become the trainable parameters -
 * the networks hb_env_collect_dev and hb_collect_gae_dev run ARE the learner's, there is no second copy to keep in step.  Allocates
 * the gradient, the Adam moments (zero) and the packed transposes; t = 0.  A learner that exists is replaced: moments and t start over,
 * the parameters - log_std included - are the trained ones.
 * hb_learner_configure changes the hyper-parameters (learning-rate and clip-range schedules) and touches no state.
 * hb_actor_set_mlp / hb_critic_set_mlp on a batch with a learner: the new network becomes the trainable one; when its sizes (and the
 * Gaussian head) are unchanged the learner stays, that network's moments (the actor's: log_std's too) are zeroed, t and the other
 * network's moments stay; when they changed the learner is destroyed and has to be created again.  Either way the actor goes on with the
 * trained log_std behind hb_critic_set_mlp, and with the log_std of its new config behind hb_actor_set_mlp.
 * HB_EINVAL: NULL argument; no actor or no critic; a hyper-parameter that is not finite or out of range (clip_range <= 0, a beta
 * outside [0, 1), lr < 0, eps <= 0); configure / destroy without a learner.  HB_EUNSUPPORTED: the deterministic head, and the squashed
 * head (HB_ACTOR_SQUASHED, SAC's actor: its learner is hb_sac_create, below).  A refused call changes nothing. */
int hb_learner_create(hb_batch* b, const hb_ppo_config* cfg);
int hb_learner_configure(hb_batch* b, const hb_ppo_config* cfg);
int hb_learner_destroy(hb_batch* b);

/* The flat record, P = hb_learner_param_count(b) floats: the actor's layers in order, each W[sizes[l]][sizes[l+1]] row-major
 * (hb_actor_set_mlp's convention: the transpose of torch.nn.Linear.weight) followed by b[sizes[l+1]]; then log_std[nu]; then the
 * critic's layers the same way.  Parameters, gradients and both moments use it; how the device holds the operands of its kernels
 * (packed B operands, a second packing of the transposes) is internal.  Host pointers; every call runs behind the work enqueued so
 * far and ends synchronised.  get_state / set_state: params[P] | m[P] | v[P] and the step count t - checkpoint and resume; set_params
 * and set_state also refresh what the forward kernels read and the actor's log_std.  count must equal P.
 * HB_EINVAL: NULL argument, no learner, a wrong count, t < 0.  (hb_learner_param_count: the count, or HB_EINVAL.) */
long long hb_learner_param_count(hb_batch* b);
int hb_learner_get_params(hb_batch* b, float* out, long long count);
int hb_learner_set_params(hb_batch* b, const float* in, long long count);
int hb_learner_get_grads(hb_batch* b, float* out, long long count);
int hb_learner_get_state(hb_batch* b, float* params, float* m, float* v, long long count, long long* t);
int hb_learner_set_state(hb_batch* b, const float* params, const float* m, const float* v, long long count, long long t);
/* The device gradient buffer and its length P, in the flat layout above: a multi-GPU caller all-reduces it (and divides by the number
 * of ranks) between hb_ppo_grad_dev and hb_ppo_adam_dev.  The pointer stays valid until the learner is destroyed. */
int hb_learner_grad_dev(hb_batch* b, float** ptr, long long* count);
/* Rows per chunk of the row reductions of a minibatch of mb rows (64 up to 4096 rows; beyond that mb / 64 rounded up to a multiple of
 * 16, so that there are never more than 64 chunks); 0 for mb < 1. */
int hb_ppo_row_chunk(int mb);

typedef struct hb_ppo_rows {     /* device pointers */
  const float* obs;              /* [n_rows][nobs] */
  const float* action;           /* [n_rows][nu] */
  const float* old_log_prob;     /* [n_rows] */
  const float* advantage;        /* [n_rows] */
  const float* returns;          /* [n_rows] */
  const int32_t* index;          /* [mb] row numbers in any order, repeats allowed; NULL: rows first .. first + mb - 1 */
  long long n_rows, first;
  int mb;
} hb_ppo_rows;

/* Loss, statistics and all gradients of one minibatch, into the learner's gradient buffer: FIVE launches on the batch's stream whatever
 * mb is (forward with kept activations; the head by row; back-propagation of dZ; the chunk partials of dW, db, dlog_std and the
 * statistics; their merge).  Asynchronous: no host synchronisation, no host transfer, no allocation beyond the learner's scratch, which
 * grows on demand (every layer's activations and dZ as [mb][width], and [chunks][P] partial gradients; a call that has to grow it waits
 * for the stream first).  A pure function of the rows, the parameters and the config: nothing else of the batch is written - state, draw
 * counter, status words, hb_last_kernel and hb_batch_step_launches stay (held hb_step_dev calls are launched first and the pipes joined,
 * as for every other call).  Rows outside the minibatch are not read.  The values of index[] are the caller's responsibility, like
 * every device pointer of this API: they are not checked.
 * stats_dev: NULL or a device float[16]: policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction, grad_norm (before
 * clipping), adv_mean, adv_std (the minibatch's moments, whether or not they are applied), ratio_max, skipped, then zeros.
 * hb_ppo_grad_dev writes all sixteen, grad_norm and skipped as 0; hb_ppo_adam_dev, given the same pointer, writes those two alone.
 * HB_EINVAL: NULL b or rows, no learner, a NULL tape, mb < 1, n_rows < 1, first < 0 or first + mb > n_rows (index NULL). */
int hb_ppo_grad_dev(hb_batch* b, const hb_ppo_rows* rows, float* stats_dev);
/* Clipping and the Adam step on the gradient buffer, in TWO launches (the norm's chunk sums; the step), asynchronous like the above.
 * The step kernel also rewrites every updated weight in the packed operands the forward kernels read, so the next
 * hb_env_collect_dev / hb_collect_gae_dev / hb_ppo_grad_dev runs the new parameters with no host transfer; pad entries of the packed
 * operands are never written and stay zero.  log_std reaches hb_actor_kernel and hb_log_prob_kernel by value in their descriptors:
 * the call marks the learner dirty, and the first later hb_env_collect*_dev / hb_collect_gae_dev copies the nu floats back into the
 * actor's config - ONE device-to-host copy of at most 128 bytes and one synchronisation per iteration, not per minibatch.
 * HB_EINVAL: NULL b, no learner. */
int hb_ppo_adam_dev(hb_batch* b, float* stats_dev);
/* hb_ppo_grad_dev, then hb_ppo_adam_dev: seven launches. */
int hb_ppo_minibatch_dev(hb_batch* b, const hb_ppo_rows* rows, float* stats_dev);

/* ---- the SAC learner on the device: twin Q critics, squashed Gaussian actor, entropy coefficient, Polyak targets, Adam -------- */

/* The update rule is stable-baselines3's SAC.train, restated here [neither package is a dependency; tests/sac_ref.py is the fp64
 * restatement the kernels are held to].  Networks (tanh after every hidden layer, linear at the top, at most four layers of width
 * <= 256; SB3's SAC default is ReLU - a stated difference): the ACTOR, the installed HB_ACTOR_SQUASHED network obs[nobs] -> 2 nu
 * (mean | raw log_std); Q1 and Q2, two networks of equal sizes [nobs + nu] -> 1 whose input row is obs | action; the TARGETS Q1', Q2',
 * created as copies.  One gradient step on mb rows (obs, action, reward, next_obs, done), with alpha = exp(log_ent_coef) at the START of
 * the step, ls = clamp(raw_ls, -20, 2), s = exp(ls):
 *   pi:     x = mean(obs) + s(obs) eps_pi,  a_pi = tanh(x),
 *           lp_pi = sum_i (-eps_i^2 / 2 - ls_i - log(2 pi) / 2) - sum_i 2 (log 2 - x_i - softplus(-2 x_i))   (hb_collect_gae_dev's head 2)
 *   next:   the same on next_obs with eps_next: a', lp'
 *   ent:    ent_coef_loss = -mean_r (log_ent_coef (lp_pi_r + target_entropy)), lp_pi a constant; auto_ent: Adam on log_ent_coef
 *   target: y_r = reward_r + (1 - done_r) gamma (min(Q1'(next_obs, a'), Q2'(next_obs, a')) - alpha lp'_r), a constant
 *   critic: critic_loss = (mean_r (Q1(obs, action) - y)^2 + mean_r (Q2(obs, action) - y)^2) / 2; dloss/dQk_r = (Qk_r - y_r) / mb; Adam on
 *           Q1, Q2
 *   actor:  with the UPDATED Q1, Q2: actor_loss = mean_r (alpha lp_pi_r - min(Q1(obs, a_pi), Q2(obs, a_pi))), the gradient through a_pi
 *           and lp_pi into the actor only; Adam on the actor
 *   polyak: when the step count t, this step included, is a multiple of target_update_interval: Q' = tau Q + (1 - tau) Q'.  (SB3 counts
 *           the gradient steps of one train() call from 0; here the count is the learner's t, which a checkpoint carries.)
 * Gradients are autograd's: torch.clamp passes the gradient where -20 <= raw_ls <= 2 (bounds included) and nothing outside; torch.min
 * sends it to the smaller Q, and on an exact tie half to each; with g_i = d min Q / da_i:  dlp/dmean_i = 2 a_i,
 * dlp/dls_i = -1 + 2 a_i s_i eps_i, da_i/dx_i = 1 - a_i^2, mb dL/dmean_i = 2 alpha a_i - g_i (1 - a_i^2),
 * mb dL/dls_i = alpha (-1 + 2 a_i s_i eps_i) - g_i (1 - a_i^2) s_i eps_i.  [tests/test_sac_cpu.py holds all of it to torch autograd in
 * float64: no disagreement was found.]  The log-probability is not SB3's log(1 - a^2 + 1e-6): the same stated difference as in
 * hb_collect_gae_dev.
 * Adam is torch.optim.Adam per group (actor, critics, log_ent_coef), each with its own learning rate; no gradient clipping and no skip
 * logic, as SB3's SAC has none; ONE step count t serves all groups; with auto_ent = 0 log_ent_coef is never stepped.
 * Arithmetic follows the PPO learner: matrix products are v_mfma_f32_16x16x4_f32 (exact f32); row reductions go over chunks of
 * hb_ppo_row_chunk(mb) rows in row order, merged in chunk order; the statistics, alpha, the Adam and the Polyak step are formed in fp64
 * and rounded to fp32 once.  No atomics: the same call gives the same bits.
 * Draws: eps_pi[r][i] = rng_normal(seed, minibatch row r, 0, t, stream 33, element i), eps_next on stream 34 (RS_ACTOR is 32, the realism
 * layer uses 1..8, domain randomisation 16..25), t being the step count BEFORE the step.
 * NOT provided: a multi-GPU gradient all-reduce (the step would have to be split at two points), gSDE / use_sde, more than two critics. */

/* Installs Q network k (0 or 1): an MLP [nobs + nu] -> sizes[1] -> ... -> 1 over the row obs | action, hb_critic_set_mlp's conventions
 * and checks (HB_EINVAL: NULL argument, k outside 0..1, n_layers outside 1..4, a size < 1, sizes[0] != nobs + nu, sizes[n_layers] != 1;
 * HB_EUNSUPPORTED: a width above 256).  Independent of the actor, the PPO critic and the MLP of hb_policy_set_mlp.  On a batch with a
 * SAC learner the call destroys that learner (so does hb_actor_set_mlp): create it again.  A refused call changes nothing. */
int hb_q_set_mlp(hb_batch* b, int k, int n_layers, const int* sizes, const float* const* weights, const float* const* biases);
/* Q1 and Q2 over n_rows rows: obs [n_rows][nobs], action [n_rows][nu] -> q1_out, q2_out [n_rows] (device pointers, either output nullable,
 * not both), ONE launch on the batch's stream, nothing kept.  HB_EINVAL: NULL b, obs or action, both outputs NULL, n_rows < 1 or above
 * 2^31 - 1, an output whose network is not installed. */
int hb_q_values_dev(hb_batch* b, const float* obs, const float* action, long long n_rows, float* q1_out, float* q2_out);

/* ---- the hidden activation of an installed network ----------------------------------------------------------------------------- */

#define HB_ACT_TANH 0
#define HB_ACT_RELU 1   /* v < 0 ? 0 : v; derivative 0 at v <= 0, as torch */
#define HB_ACT_ELU  2   /* v > 0 ? v : expm1(v)  (alpha = 1) */
#define HB_NET_POLICY 0 /* hb_policy_set_mlp */
#define HB_NET_ACTOR  1 /* hb_actor_set_mlp */
#define HB_NET_CRITIC 2 /* hb_critic_set_mlp */
#define HB_NET_Q1     3 /* hb_q_set_mlp, k = 0 */
#define HB_NET_Q2     4 /* hb_q_set_mlp, k = 1 */
/* The activation behind every HIDDEN layer of the installed network `net`, in every kernel that runs it - hb_policy_eval and
 * hb_rollout_policy, the collection, hb_collect_gae_dev, hb_q_values_dev, both learners' forward and backward passes (which form the
 * derivative from the kept output a: 1 - a^2; a > 0 ? 1 : 0; a > 0 ? 1 : a + 1).  The last layer stays what its installation made it:
 * tanh for hb_policy_set_mlp and actor head 0, linear for the other heads, the critic and Q; the squashing tanh of HB_ACTOR_SQUASHED is
 * part of the head.  A non-finite pre-activation stays non-finite behind all three.  Every hb_*_set_mlp installs its network with
 * HB_ACT_TANH: a caller that never calls this function sees no difference, and one that replaces a network sets the activation again.
 * Setting the value in force is a no-op.  Another value follows the rule of the network's set_mlp: on the actor or the critic it destroys
 * a PPO learner (the actor keeps the log_std it trained), on the actor, Q1 or Q2 a SAC learner; the actor's draw counter is NOT reset.
 * The SAC targets run their Q network's activation, and hb_sac_create refuses Q1 and Q2 with different ones (the actor's may differ).
 * The activation belongs to the installation, not to a learner: the parameter, moment and checkpoint records (hb_learner_get_state,
 * hb_sac_get_state) keep their layout and do not hold it, so a caller that resumes repeats set_mlp AND this call before it creates the
 * learner and restores the state.
 * HB_EINVAL: NULL batch, a net that is none of HB_NET_*, an activation that is none of HB_ACT_*, no network of that kind installed.  A
 * refused call changes nothing. */
int hb_mlp_set_activation(hb_batch* b, int net, int activation);
int hb_mlp_get_activation(hb_batch* b, int net);   /* HB_ACT_*, or HB_EINVAL */

typedef struct hb_sac_config {
  float gamma;                  /* 0.99    in [0, 1] */
  float tau;                    /* 0.005   in [0, 1] */
  float lr_actor, lr_critic, lr_ent;  /* 3e-4 each   >= 0 */
  float beta1, beta2;           /* 0.9, 0.999   in [0, 1) */
  float eps;                    /* 1e-8    > 0 */
  float ent_coef_init;          /* 1.0     > 0; read by hb_sac_create alone: log_ent_coef = log(ent_coef_init) */
  int auto_ent;                 /* 1       0: log_ent_coef stays what it is */
  int target_entropy_auto;      /* 1       target_entropy = -nu */
  float target_entropy;         /* 0       read when target_entropy_auto is 0 */
  int target_update_interval;   /* 1       >= 1 */
  unsigned seed;                /* 0       of the draws */
} hb_sac_config;
int hb_sac_default_config(hb_sac_config* cfg);

/* Creates the batch's SAC learner: the installed actor (its head must be HB_ACTOR_SQUASHED) and both Q networks become the trainable
 * parameters - the actor hb_env_collect_dev runs IS the learner's.  Makes the targets as copies of Q1 and Q2, sets
 * log_ent_coef = log(ent_coef_init), zeroes the moments, t = 0.  A SAC learner that exists is replaced.  hb_sac_configure changes the
 * hyper-parameters and touches no state.  hb_actor_set_mlp or hb_q_set_mlp on a batch with a SAC learner destroys it.  A PPO learner
 * (hb_learner_create) needs the Gaussian head, this one the squashed head: a batch never holds both.
 * HB_EINVAL: NULL argument; no actor, a Q network missing, Q1 and Q2 of unequal sizes or with different activations; a hyper-parameter that is not finite or out of
 * range (above); configure / destroy without a learner.  HB_EUNSUPPORTED: any other actor head.  A refused call changes nothing. */
int hb_sac_create(hb_batch* b, const hb_sac_config* cfg);
int hb_sac_configure(hb_batch* b, const hb_sac_config* cfg);
int hb_sac_destroy(hb_batch* b);

/* The flat record, P = hb_sac_param_count(b) floats: the actor's layers in order, each W[sizes[l]][sizes[l+1]] row-major followed by
 * b[sizes[l+1]]; then Q1's layers, then Q2's, then log_ent_coef.  Parameters, gradients and both moments use it.  The targets' record,
 * PT = hb_sac_target_count(b) floats: Q1' then Q2' in the same layer layout.  Host pointers; every call runs behind the work enqueued so
 * far and ends synchronised.  get_grads after a step returns the gradients that step USED: the critic and log_ent_coef entries come from
 * its critic phase (the log_ent_coef entry is formed whether or not auto_ent steps it), the actor entries from its actor phase, which
 * forms no dW of the Q networks.  set_params / set_state also refresh every operand the kernels read; set_params leaves the targets.
 * HB_EINVAL: NULL argument, no learner, a wrong count, t < 0. */
long long hb_sac_param_count(hb_batch* b);
long long hb_sac_target_count(hb_batch* b);
int hb_sac_get_params(hb_batch* b, float* out, long long count);
int hb_sac_set_params(hb_batch* b, const float* in, long long count);
int hb_sac_get_grads(hb_batch* b, float* out, long long count);
int hb_sac_get_state(hb_batch* b, float* params, float* m, float* v, long long count, float* targets, long long target_count, long long* t);
int hb_sac_set_state(hb_batch* b, const float* params, const float* m, const float* v, long long count, const float* targets, long long target_count, long long t);

typedef struct hb_sac_rows {     /* device pointers */
  const float* obs;              /* [n_rows][nobs] */
  const float* action;           /* [n_rows][nu] */
  const float* reward;           /* [n_rows] */
  const float* next_obs;         /* [n_rows][nobs] */
  const uint8_t* done;           /* [n_rows]  terminated (an env cut by truncation alone bootstraps) */
  const int32_t* index;          /* [mb] row numbers in any order, repeats allowed; NULL: rows first .. first + mb - 1 */
  long long n_rows, first;
  int mb;
  float* eps_pi;                 /* [mb][nu], nullable unless eps_given */
  float* eps_next;               /* [mb][nu], nullable unless eps_given */
  int eps_given;                 /* 0: the draws are made on the device and written to the pointers that are given; 1: they are read */
} hb_sac_rows;

/* One gradient step as above, asynchronous on the batch's stream: SIXTEEN launches whatever mb is (fifteen on a step whose count is no
 * multiple of target_update_interval) - forward of the actor on obs and next_obs and of Q1, Q2; the samples by row; forward of the
 * targets; the critic head by row; back-propagation, dW partials, their merge and Adam for Q1, Q2 (and log_ent_coef); forward of the
 * updated Q1, Q2 at a_pi; their back-propagation into the action inputs; the actor head by row; back-propagation, dW partials, merge and
 * Adam for the actor; the Polyak step.  No host synchronisation, no host transfer, no allocation beyond the learner's scratch, which
 * grows with mb (a call that has to grow it waits for the stream first).  The Adam and Polyak kernels rewrite every updated weight in
 * the packed operands the forward kernels read and in the packed transposes, so the next hb_env_collect_dev runs the new actor; pad
 * entries are never written.  A pure function of the rows, the draws and the learner's state: nothing else of the batch is written -
 * state, the collection's draw counter, status words, hb_last_kernel and hb_batch_step_launches stay.  Rows outside the minibatch are
 * not read; the values of index[] are not checked.
 * stats_dev: NULL or a device float[16]: actor_loss, critic_loss, ent_coef_loss, ent_coef (the alpha used), the means of lp_pi,
 * Q1(obs, action), Q2(obs, action), y and min Q(obs, a_pi), then zeros.
 * HB_EINVAL: NULL b or rows, no learner, a NULL tape, mb < 1, n_rows < 1, first < 0 or first + mb > n_rows (index NULL), eps_given with a
 * NULL eps_pi or eps_next.  A refused call writes nothing. */
int hb_sac_step_dev(hb_batch* b, const hb_sac_rows* rows, float* stats_dev);

/* ---- host-side helpers so a C/C++/ctypes caller needs no HIP headers ---------------------------- */

/* Device buffer on the batch's GPU (hipMalloc / hipFree). */
void* hb_dev_alloc(hb_batch* b, uint64_t bytes);
void hb_dev_free(hb_batch* b, void* p);
/* Page-locked host memory (hipHostMalloc / hipHostFree).  Host pointers handed to hb_step, hb_env_step, hb_get_obs ...
 * may be any memory; when they are page-locked the copies are DMA transfers that overlap instead of staged ones
 * (VecEnv keeps its action and observation arrays in such buffers). */
void* hb_host_alloc(uint64_t bytes);
void hb_host_free(void* p);
int hb_memcpy_h2d(hb_batch* b, void* dst_dev, const void* src, uint64_t bytes);
int hb_memcpy_d2h(hb_batch* b, void* dst, const void* src_dev, uint64_t bytes);
/* Fills out_dev[T][n_env][nu] with the benchmark's deterministic controls, the generator of
 * simulation/mujoco/sample/testspeed.cc:64-80 (CtrlNoise) with ctrlnoise = 1:
 * ctrl[t,e,i] = 2*Halton(1 + t0 + t + 1000*(env_offset+e), i+2) - 1. */
int hb_halton_ctrl_dev(hb_batch* b, int T, int t0, int env_offset, float* out_dev);
/* HIP-event stopwatch on the batch's stream (hipEventRecord on that stream; hipEventElapsedTime). */
int hb_timer_start(hb_batch* b);
int hb_timer_stop(hb_batch* b, float* elapsed_ms);
/* Per-kernel timing of the step kernel alone: when enabled, every 8th step launch is bracketed by its own pair
 * of HIP events on the launch stream (up to 256 samples); hb_step_timing_read synchronises and returns their mean. */
int hb_step_timing(hb_batch* b, int enable);
int hb_step_timing_read(hb_batch* b, float* mean_us, int* samples);
/* Diagnostic builds only (libhb_stamps.so, -DHB_STAMPS): per-env s_memtime stamps at the 16 phase
 * boundaries of the last step; the first call arms the buffer.  HB_EUNSUPPORTED in the product build. */
int hb_get_stamps(hb_batch* b, unsigned long long* out);

const char* hb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HB_H_ */

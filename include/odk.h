/* odk.h -- C-ABI of the MI355X-native Open Duck env engine (libodk.so).
 *
 * Drop-in boundary for the physics + Joystick-task hot path of apirrone/Open_Duck_Playground
 * (SURVEY.md section 8b).  The reference has no FFI: its boundary is the Python/JAX API
 *     mjx.put_model(mj_model)                                  playground/open_duck_mini_v2/base.py:61
 *     Joystick.reset(rng) -> State                              playground/open_duck_mini_v2/joystick.py:206
 *     Joystick.step(State, action) -> State                     playground/open_duck_mini_v2/joystick.py:323
 *     Standing.reset / Standing.step (env_kind = ODK_ENV_STANDING) playground/open_duck_mini_v2/standing.py:200,316
 *       (which calls mjx_env.init :258 and mjx_env.step(model, data, motor_targets, n_substeps) :420)
 *     randomize.domain_randomize(model, rng) -> batched fields  playground/common/randomize.py:26-146
 *     wrapper.wrap_for_brax_training (Vmap/Episode/AutoReset)   playground/common/runner.py:117
 * Each entry point below names the call it replaces.  Plain pointers and sizes only; all
 * `*_dev` pointers are device (HIP) addresses owned by the caller; calls are ordered on the caller's
 * stream (`hipStream_t` passed as void*), never synchronise the host, and never allocate in step.
 *
 * Every function returns 0 on success or a negative odk_status; odk_last_error() gives the
 * thread-local message.  Numerical failure inside an env is NOT an error: it yields NaN ->
 * done = 1 for that env (reference joystick.py:483-485).
 */
#ifndef ODK_H
#define ODK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct odk_model odk_model;
typedef struct odk_batch odk_batch;

enum odk_status {
  ODK_OK = 0,
  ODK_ERR_INVALID = -1,      /* bad argument / malformed blob */
  ODK_ERR_UNSUPPORTED = -2,  /* model shape or option the kernels were not built for */
  ODK_ERR_HIP = -3,          /* HIP runtime failure */
  ODK_ERR_NOMEM = -4
};

/* Observation row strides of the duck (nu = 14 actuators).  For a robot with nu actuators (odk_model_obs_sizes): joystick.py:570-615
 * state 17 + 6 nu, privileged_state = state + 69 + 3 nu; standing.py:524-565 state 15 + 5 nu, privileged_state = state + 26 + 3 nu. */
#define ODK_NOBS 101     /* obs["state"]            joystick.py:570-589 */
#define ODK_NPRIV 212    /* obs["privileged_state"] joystick.py:596-615 */
#define ODK_NOBS_STANDING 85    /* standing.py:524-540 */
#define ODK_NPRIV_STANDING 153  /* standing.py:548-565 */
#define ODK_ENV_JOYSTICK 0
#define ODK_ENV_STANDING 1
#define ODK_NMETRIC 8    /* reward/cost terms (7) + swing_peak, joystick.py:304-311 */
#define ODK_NU 14        /* the duck's actuators; odk_model_dims reports a model's own count */

/* Environment configuration == default_config() of the reference (joystick.py:49-102). */
typedef struct {
  float ctrl_dt, action_scale, dof_vel_scale, max_motor_velocity;
  float noise_level, noise_gyro, noise_accelerometer, noise_gravity, noise_joint_vel;
  float qpos_noise_scale[16];
  float reward_scales[7];  /* tracking_lin_vel, tracking_ang_vel, torques, action_rate, stand_still, alive, imitation;
                              Standing: orientation, head_pos, torques, action_rate, stand_still, alive, (unused) */
  float tracking_sigma;
  float push_enable, push_interval_range[2], push_magnitude_range[2];
  float cmd_range[7][2];   /* lin_vel_x, lin_vel_y, ang_vel_yaw, neck_pitch, head_pitch, head_yaw, head_roll */
  int32_t use_imitation, use_motor_speed_limits;
  int32_t autoreset;       /* BraxAutoResetWrapper on/off */
  int32_t episode_length;  /* EpisodeWrapper */
  int32_t n_substeps;      /* ctrl_dt / sim_dt */
  int32_t lanes_per_env;   /* kernel geometry hint: 32 or 64 (0 = default); see odk_batch_lanes */
  int32_t env_kind;        /* ODK_ENV_JOYSTICK (joystick.py) or ODK_ENV_STANDING (standing.py): selects the obs layout
                              (101/212 vs 85/153 floats per env -- the output row strides) and the reward table */
  float reset_base_qvel;   /* half-range of the base velocity noise at reset: joystick.py:253 0.05, standing.py:247 0.5 */
  int32_t hfield_up_normals_only; /* BUILD-DEFINED opt-in, default 0 = the prism algorithm as recalled from MJX.  1: on a height-field
                              floor a prism pair's contacts count only when their normal points up (n_z > 0.5 in the field's frame): drops the
                              sideways contacts of prism side faces.  The reading under which the reference's rough-terrain task trains
                              (profiles/r4/hfield_variants.json); parity against the oracle's hfield_mode 3 */
} odk_env_config;

/* Caller-owned device outputs of reset/step (any pointer may be NULL to skip it). */
typedef struct {
  float* obs_dev;         /* [nenv, nobs]   (the duck: 101; odk_model_obs_sizes) */
  float* priv_dev;        /* [nenv, npriv]  (the duck: 212) */
  float* reward_dev;      /* [nenv] */
  float* done_dev;        /* [nenv] */
  float* truncation_dev;  /* [nenv] */
  float* metrics_dev;     /* [nenv, 8] */
} odk_outputs;

/* Per-env randomised model fields == the 8 fields of randomize.py:119-144 (geom_friction is a
 * visual geom in the reference and therefore has no physical effect; it is not taken). */
enum odk_param {
  ODK_PARAM_BODY_MASS = 0,        /* [nenv, nbody] */
  ODK_PARAM_BODY_IPOS_TORSO = 1,  /* [nenv, 3]   body_ipos[TORSO_BODY_ID=1] */
  ODK_PARAM_DOF_FRICTIONLOSS = 2, /* [nenv, nu]  actuated dofs */
  ODK_PARAM_DOF_ARMATURE = 3,     /* [nenv, nu] */
  ODK_PARAM_QPOS0 = 4,            /* [nenv, nu]  actuated joints */
  ODK_PARAM_KP = 5                /* [nenv, nu]  gainprm[:,0]; biasprm[:,1] = -kp */
};

const char* odk_last_error(void);
void odk_default_config(odk_env_config* cfg);
/* default_config() of reference standing.py:44-100 (incl. USE_IMITATION_REWARD = False, no motor speed limit) */
void odk_default_config_standing(odk_env_config* cfg);
/* row strides of the obs / privileged_state outputs for an env kind -- of the duck (14 actuators) */
void odk_obs_sizes(int env_kind, int* nobs, int* npriv);

/* mjx.put_model: parse a ModelBlob (open_duck_playground_amd/model.py; written by the MJCF compiler mjcf.py).
 * Colliders the kernels take: two feet -- convex meshes or boxes (cgeom_type 7: hull vertices + outward triangles), or spheres /
 * capsules (cgeom_type 2 / 3 with the optional record cgeom_size[ncgeom][3]: radius, half length) -- and one floor, a plane (0) or a
 * height field (1: hfield_data + hfield_size).  ODK_ERR_UNSUPPORTED for anything else (other foot types, a hull foot beside a
 * primitive one on a height field, feet wider than two height-field cells, hulls with more than 17 vertices / 30 faces / 48 edges
 * or faces of more than four vertices).
 * Solver options read from the blob: opt_iterations / opt_ls_iterations, opt_impratio, and the optional opt_cone (0 pyramidal, 1 elliptic:
 * the elliptic-cone instantiations of the kernels -- hull feet, 32 lanes per env; sphere / capsule feet refuse it).  The optional eq_*
 * records (<equality>): joint couplings between two hinges of one serial chain, and connect / weld constraints whose two bodies lie on one
 * root-to-leaf path of the tree (or body2 = the world) or on the two foot chains (a closed loop) -- at most two with nine rows --, are
 * taken for the third and fourth model shapes; every other
 * ACTIVE equality is refused by name. */
int odk_model_load(const void* blob, uint64_t len, odk_model** out);
void odk_model_free(odk_model* m);
int odk_model_dims(const odk_model* m, int* nq, int* nv, int* nu, int* nbody);
/* row strides of the obs / privileged_state outputs of THIS model's env kernels (what `observation_size` of the reference's env reports,
 * base.py:277-291 / joystick.py:570-615, for a robot with the model's actuator count): the duck 101 / 212 (Standing 85 / 153), a robot
 * with 12 actuators 89 / 194.  The per-env layout is the reference's with nu in place of 14. */
int odk_model_obs_sizes(const odk_model* m, int env_kind, int* nobs, int* npriv);

/* Twin dofs (backlash joints: a hinge declared right after another hinge on the same body, same anchor and axis) share
 * their motion column, so the kernels keep the inertia / Newton Hessian on the REDUCED tree with the twins merged
 * (csrc/odk_model.h DevModel::paired).  Reports that reduction: paired (0 / 1), reduced dof count, entries of the reduced
 * tree layout and of its virtual (Hessian) tree, and per reduced dof the main dof and the twin dof (-1: none); arrays of
 * >= 32 ints, any pointer may be NULL.  Host-only (no GPU needed). */
int odk_model_reduced(const odk_model* m, int* paired, int* nvr, int* nMr, int* nHr, int* red_main, int* red_twin);
/* Body-to-lane layout of the kinematics / inertia sweeps at `lanes_per_env` (32 or 64) lanes per env: out[lane] = the body id
 * that lane computes, -1 for a lane without a body, for the first min(n, lanes_per_env) lanes.  Every serial body chain sits
 * in consecutive lanes of one 16-lane row, in chain order (its scans are DPP row shifts); a model without such a layout is
 * refused by odk_model_load.  Host-only (no GPU needed). */
int odk_model_body_lanes(const odk_model* m, int lanes_per_env, int* out, int n);
/* floats of LDS one env occupies in the fused step kernel (8 single-wave workgroups of two envs per CU need <= 2560) */
int odk_model_env_lds_floats(const odk_model* m);
/* The launch-invariant small integers of the substep as the plane-floor step kernel reads them (csrc/odk_model.h DevModel::hot_pk: three
 * packed words, written at load; a value that does not fit its field is refused there by name) and, next to them, the twelve values they
 * were packed from: foot_body[2], foot_nvert[2], foot_rchain_first[2], foot_rchain_len[2], ls_iterations, max_nonpath_level, np_count,
 * foot_prim.  Layout: word 0 = foot_body * 4 in bytes 0 / 1, foot_nvert in bytes 2 / 3; word 1 = foot_rchain_first * 4 in bytes 0 / 1,
 * foot_rchain_len in bits 16-19 / 20-23, ls_iterations in byte 3; word 2 = max_nonpath_level + 1, np_count, foot_prim in bytes 0 / 1 / 2.
 * Host-only (no GPU needed). */
int odk_model_hot_words(const odk_model* m, int* packed, int* fields);

/* One batch of `nenv` environments resident on HIP device `device`.  `prm_table` is the host
 * [nx,ny,nth,40,16] float32 reference-motion table (poly_reference_motion.py), grids in float64. */
int odk_batch_create(const odk_model* m, const odk_env_config* cfg, int nenv, int device, const float* prm_table,
                     const double* dxs, int nx, const double* dys, int ny, const double* dths, int nth, const double* ranges6,
                     int nsteps_in_period, odk_batch** out);
void odk_batch_destroy(odk_batch* b);
/* Replaces the configuration of a live batch; the next odk_reset / odk_step uses it.  The config travels BY VALUE in the kernel arguments of
 * every launch, so a captured graph keeps the config it was captured with: call this before capturing, or capture again.  `env_kind` is fixed
 * at creation (it sets the output strides: ODK_ERR_INVALID for another kind) and so is the lane count (`lanes_per_env` is ignored here:
 * odk_batch_lanes).  `push_interval_steps` is drawn at reset from `push_interval_range` / `ctrl_dt`: an env keeps the interval it drew under
 * the old config, through auto-resets too, until the next odk_reset. */
int odk_batch_set_config(odk_batch* b, const odk_env_config* cfg);

/* domain_randomize: per-env model fields, host pointer, copied synchronously */
int odk_batch_set_param(odk_batch* b, int param, const float* host_values, int count_per_env);

/* Joystick.reset (vmapped) + wrapper resets.  Env e uses key(seed, env_id_offset + e). */
int odk_reset(odk_batch* b, uint32_t seed, uint32_t env_id_offset, const odk_outputs* outs, void* stream);

/* AutoReset.step -> Episode.step -> Joystick.step for all envs; action_dev is [nenv, nu]. */
int odk_step(odk_batch* b, const float* action_dev, const odk_outputs* outs, void* stream);

/* Caller-given commands (replaces mujoco_infer.py's keyboard `self.commands`).  cmd_dev: [nenv, row_stride] device floats on the
 * batch's device, row e = env e's lin_vel_x, lin_vel_y, ang_vel_yaw, neck_pitch, head_pitch, head_yaw, head_roll (the order of
 * cmd_range); row_stride >= 7.  NULL unbinds (sampled commands again).  While bound:
 *   - every odk_step reads env e's row at the start of its step (before the reference motion, the reward and the observation), so a
 *     stream-ordered write to the buffer between two steps is what the next step follows;
 *   - odk_reset, the auto-reset inside odk_step and the resample after step 500 store the row where sample_command's value went;
 *   - every random draw is still made, in the same order: noise, push and reset streams are those of an unbound run.
 * The buffer stays the caller's and must outlive the binding.  The pointer is a kernel argument: a captured graph keeps the pointer it
 * was captured with (and reads that buffer's current contents at every replay); bind before capturing. */
int odk_batch_bind_commands(odk_batch* b, const float* cmd_dev, int row_stride);

/* Reward-library terms (reference playground/common/rewards.py) computed by the step kernel on top of the seven native slots of
 * odk_env_config.reward_scales.  A term is on when its scale is non-zero (the reference's reward_config.scales decide it the same
 * way, joystick.py:304-311); the scaled term is added to the step's total before clip(total * dt, 0, 10000), and its metric is
 * stored like the native ones: scale > 0 ? scaled : -scaled.  Inputs (the robot's own sensors, sites, actuators and limits):
 *   LIN_VEL_Z        cost_lin_vel_z(global_linvel sensor of the imu site)       -- needs a `global_linvel` sensor (ODK_ERR_UNSUPPORTED otherwise)
 *   ANG_VEL_XY       cost_ang_vel_xy(global_angvel sensor)
 *   ORIENTATION      cost_orientation(upvector sensor)                          -- joystick.py:645 (commented there); Standing has it as a native slot
 *   BASE_HEIGHT      cost_base_height(qpos[2], base_height_target)
 *   ENERGY           cost_energy(|qvel| |qfrc_actuator|) over the actuated dofs (qfrc_actuator of a dof = its actuator's force)
 *   JOINT_POS_LIMITS cost_joint_pos_limits(actuated qpos, soft limits c -+ 0.5 r soft_joint_pos_limit_factor of jnt_range, joystick.py:135-139)
 *   TERMINATION      cost_termination(the step's termination: not the EpisodeWrapper's truncation)
 *   POSE             cost_pose(actuated qpos, home keyframe ctrl, pose_weight[0 .. nu))
 *   FEET_SLIP        cost_feet_slip(contact[2], feet *_global_linvel sensors [2][3])
 *   FEET_CLEARANCE   cost_feet_clearance(feet linvel sensors, feet site z, max_foot_height)
 *   FEET_HEIGHT      cost_feet_height(swing_peak after this step's max, first_contact, max_foot_height)
 *   FEET_AIR_TIME    reward_feet_air_time(feet_air_time after += dt, first_contact, command, air_time_range)
 * with first_contact = (feet_air_time before the increment > 0) * (contact | last_contact), joystick.py:430-431. */
#define ODK_NXTERM 12
enum odk_xterm {
  ODK_XTERM_LIN_VEL_Z = 0, ODK_XTERM_ANG_VEL_XY = 1, ODK_XTERM_ORIENTATION = 2, ODK_XTERM_BASE_HEIGHT = 3, ODK_XTERM_ENERGY = 4,
  ODK_XTERM_JOINT_POS_LIMITS = 5, ODK_XTERM_TERMINATION = 6, ODK_XTERM_POSE = 7, ODK_XTERM_FEET_SLIP = 8, ODK_XTERM_FEET_CLEARANCE = 9,
  ODK_XTERM_FEET_HEIGHT = 10, ODK_XTERM_FEET_AIR_TIME = 11
};
typedef struct {
  float scale[ODK_NXTERM];          /* by enum odk_xterm; 0 = off */
  float base_height_target;         /* BASE_HEIGHT */
  float max_foot_height;            /* FEET_CLEARANCE, FEET_HEIGHT */
  float air_time_range[2];          /* FEET_AIR_TIME: threshold_min, threshold_max */
  float soft_joint_pos_limit_factor;/* JOINT_POS_LIMITS */
  float pose_weight[16];            /* POSE: one per actuator */
} odk_reward_terms;
/* Sets the terms (copied synchronously into a device buffer the batch owns).  NULL or all scales 0: off -- the step then computes
 * exactly what it computes without this call.  A parameter of an enabled term that is not finite is ODK_ERR_INVALID.  The kernels
 * receive the buffer's pointer while some term is on: a graph captured then reads the buffer's contents at every replay, so later
 * calls that change scales or parameters (or set every scale to 0) are followed; a graph captured while all terms were off stays off. */
int odk_batch_set_reward_terms(odk_batch* b, const odk_reward_terms* terms);
/* Where every step writes the library metrics while some term is on: dev [nenv, ODK_NXTERM] (column = enum odk_xterm; 0 for a term
 * that is off), or NULL (not written).  odk_reset writes zeros there.  Caller-owned, like odk_batch_bind_commands' buffer. */
int odk_batch_bind_reward_metrics(odk_batch* b, float* dev);

/* Joint map of the imitation reward (custom_rewards.py:80-88): frame_joint[u] is the joint of the reference-motion frame (rows u and
 * 16 + u of the canonical [.., 40, 16] table) that actuator u's position and velocity are compared with, or -1 for an actuator the
 * reward does not compare.  nu must be the model's actuator count, every entry in [-1, 15], no frame joint used twice; otherwise
 * ODK_ERR_INVALID.  The duck's model shapes start with the duck's map (joints[:5] ++ joints[9:] vs frame[:5] ++ frame[11:16]); other
 * robots start without one, and their odk_reset / odk_step refuse use_imitation until it is set.  Synchronous; the map lives in a
 * buffer of the batch, so a graph captured earlier follows later calls. */
int odk_batch_set_imitation_joints(odk_batch* b, const int32_t* frame_joint, int nu);

/* Head joints of the Standing task (standing.py:590-597, rewards.py:105-147): actuator[k] is the actuator that posture command k tracks,
 * in cmd_range order 3..6 (neck_pitch, head_pitch, head_yaw, head_roll), or -1 for a slot with no joint.  cost_head_pos sums over the
 * mapped slots; cost_stand_still(ignore_head=True) leaves the mapped actuators out (an all -1 map: a robot without a head, every actuator
 * counted, head_pos 0).  n must be 4, every entry in [-1, nu - 1], no actuator used twice; otherwise ODK_ERR_INVALID.  The duck's model
 * shapes start with {5, 6, 7, 8}; other robots start without a map, and their odk_reset / odk_step refuse env_kind = ODK_ENV_STANDING until
 * it is set.  Synchronous; the map lives in a buffer of the batch, so a graph captured earlier follows later calls. */
int odk_batch_set_head_joints(odk_batch* b, const int32_t* actuator, int n);

/* Velocity-tracking accumulator: one launch per evaluation step, after odk_step, graph-capturable.  For every env whose
 * acc[e][ODK_TRACK_ENDED] is 0 (its first episode: the Evaluator's `active`) it adds 1 to STEPS and the step's reward to REWARD; on
 * a done step it adds 1 to FALLS when truncation is 0 and sets ENDED; otherwise (a velocity sample: the observation of a done step is
 * the auto-reset's first one) it adds 1 to SAMPLES, the achieved local linear velocity x, y and yaw rate to SUM + 0..2 and their
 * squared errors against the bound command's first three entries to SQERR + 0..2.  The achieved values come from the noise-free
 * privileged observation (priv_dev [nenv, npriv] of this step): gyro at row offset nobs, local linear velocity at nobs + 9
 * (odk_model_obs_sizes).  reward_dev / done_dev / truncation_dev: [nenv]; acc_dev: [nenv, ODK_TRACK_NACC], zeroed by the caller
 * before the first step.  Needs bound commands. */
#define ODK_TRACK_NACC 12
enum { ODK_TRACK_ENDED = 0, ODK_TRACK_STEPS = 1, ODK_TRACK_SAMPLES = 2, ODK_TRACK_FALLS = 3, ODK_TRACK_REWARD = 4, ODK_TRACK_SUM = 5,
       ODK_TRACK_SQERR = 8 };
int odk_tracking_accumulate(const odk_batch* b, const float* priv_dev, const float* reward_dev, const float* done_dev,
                            const float* truncation_dev, float* acc_dev, void* stream);

/* Caller-given pushes (replaces the mouse of mujoco_infer.py's viewer: shove the robot, see whether the policy stays up).  push_dev:
 * [nenv, row_stride] device floats on the batch's device, row e = the world-frame velocity kick (dvx, dvy) in m/s that env e's NEXT
 * odk_step adds to qvel[0:2]; row_stride >= 2.  NULL unbinds (the sampled push of push_config again).  While bound:
 *   - every odk_step reads env e's row where the sampled push * push_magnitude entered (joystick.py:381-398): before the motor targets
 *     and the substeps, on the state the step starts from -- after a done step that is the auto-reset's state; a stream-ordered write to
 *     the buffer between two steps is what the next step applies, and a row left non-zero is applied again by every step;
 *   - the sampled push is not applied: push_enable and the interval gate do not matter;
 *   - every random draw is still made, in the same order (theta and magnitude are drawn and dropped): push_step, push_interval_steps,
 *     the rng counter and the noise, command and reset streams are those of an unbound run;
 *   - info["push"] (record field `push`) holds the kick's unit direction, 0 0 for a zero row (the reference keeps a direction there, not
 *     a velocity);
 *   - odk_reset is untouched (push starts at 0).
 * Only the floating base's planar velocity is touched, so this works for every robot the engine steps.  The buffer stays the caller's
 * and must outlive the binding.  The pointer is a kernel argument: a captured graph keeps the pointer it was captured with (and reads
 * that buffer's current contents at every replay); bind before capturing.  row_stride < 2, or memory that is not device memory of the
 * batch's device: ODK_ERR_INVALID, and the binding stays as it was. */
int odk_batch_bind_pushes(odk_batch* b, const float* push_dev, int row_stride);

/* Caller-given action delays (control latency as a controlled axis: the reference draws a 0..2-step delay per step, joystick.py:357-376, and
 * a trained policy claims to tolerate every one of them).  delay_dev: [nenv, row_stride] device int32 on the batch's device, row e's first
 * entry = the row of env e's action-history ring that its NEXT odk_step turns into motor targets: 0 the action just given, 1 the one before,
 * 2 the one before that; row_stride >= 1.  NULL unbinds (the sampled delay again).  While bound:
 *   - every odk_step reads env e's row where the sampled index entered (joystick.py:372-376), clamped in the kernel: a value above 2 is 2;
 *   - a NEGATIVE row (-1, and any other negative value alike) means "sample, as unbound": one buffer can mix fixed and sampled envs;
 *   - the delay's random draw is still made and dropped: the rng key and counter, the push, noise, command and reset streams are those of an
 *     unbound run, and the ring keeps rolling as ever (a step with delay 2 applies the action given two steps earlier);
 *   - odk_reset and the auto-reset do not read the delay (they clear the ring).
 * The buffer stays the caller's and must outlive the binding.  The pointer is a kernel argument: a captured graph keeps the pointer it was
 * captured with (and reads that buffer's current contents at every replay); bind before capturing.  row_stride < 1, or memory that is not
 * device memory of the batch's device: ODK_ERR_INVALID, and the binding stays as it was. */
int odk_batch_bind_action_delays(odk_batch* b, const int32_t* delay_dev, int row_stride);

/* Push-recovery accumulator: one launch per evaluation step, graph-capturable, issued after odk_step and BEFORE odk_tracking_accumulate
 * (track_acc_dev [nenv, ODK_TRACK_NACC] is that function's accumulator: its ENDED slot then still says whether env e's first episode was
 * running when this step began, and its STEPS slot counts the first-episode steps before this one).  Env e's row of acc_dev
 * [nenv, ODK_PUSH_NACC], zeroed by the caller before the first step, is updated only during e's first episode:
 *   PUSHED          becomes 1 at the first step whose bound push row was non-zero (the pushed step; the row is read as the step left it)
 *   PUSH_AT         number of first-episode steps before that step
 *   FELL            1 when the first episode ends with done and no truncation, at or after the pushed step
 *   STEPS_TO_FALL   steps from the pushed step to that done step, counting both (1: it fell in the pushed step)
 *   LAST_OFF        steps from the pushed step, counting both, to the latest velocity sample at or after it whose planar velocity error
 *                   hypot(vx - cmd_x, vy - cmd_y) exceeded lin_tol or whose yaw-rate error |wz - cmd_wz| exceeded ang_tol; 0 if none.
 *                   The recovery time, causal: a running "last seen", final once the episode is over
 *   PEAK_LIN_ERR, PEAK_ANG_ERR   the maxima of those two errors over the velocity samples at or after the pushed step
 *   PRE_LIN_ERR_SUM, PRE_SAMPLES sum of the planar error over, and count of, the velocity samples before the pushed step: the policy's own
 *                   tracking error, against which the tolerances can be judged.  The sum is compensated (Kahan), so that SUM stays within an ulp of
 *                   the true sum over any number of samples; PRE_LIN_ERR_LOW holds the part SUM dropped (SUM + LOW in float64 is closer still)
 * A velocity sample is odk_tracking_accumulate's (a step that is not done), the achieved velocities are the ones it reads (priv_dev
 * [nenv, npriv] of this step: gyro at row offset nobs, local linear velocity at nobs + 9).  done_dev / truncation_dev: [nenv].  Needs bound
 * commands and bound pushes: ODK_ERR_INVALID otherwise, and nothing is launched. */
#define ODK_PUSH_NACC 10
enum { ODK_PUSH_PUSHED = 0, ODK_PUSH_PUSH_AT = 1, ODK_PUSH_FELL = 2, ODK_PUSH_STEPS_TO_FALL = 3, ODK_PUSH_LAST_OFF = 4, ODK_PUSH_PEAK_LIN_ERR = 5,
       ODK_PUSH_PEAK_ANG_ERR = 6, ODK_PUSH_PRE_LIN_ERR_SUM = 7, ODK_PUSH_PRE_SAMPLES = 8, ODK_PUSH_PRE_LIN_ERR_LOW = 9 };
int odk_push_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                        const float* track_acc_dev, float lin_tol, float ang_tol, float* acc_dev, void* stream);

/* Gait and actuator-load accumulator (how does the policy walk, and what does that cost the motors): one launch per evaluation step,
 * graph-capturable, issued after odk_step and BEFORE odk_tracking_accumulate (track_acc_dev [nenv, ODK_TRACK_NACC] is that function's
 * accumulator: its ENDED slot then still says whether env e's first episode was running when this step began).  Independent of
 * odk_push_accumulate; needs neither bound commands nor bound pushes.  Env e's row of acc_dev [nenv, ODK_GAIT_NACC], zeroed by the caller
 * before the first step, is updated only on a gait sample: a step of e's first episode that is not done (odk_tracking_accumulate's
 * velocity sample; a done step's observation is the auto-reset's first one).  Every other row keeps its bits.  All inputs are the
 * noise-free privileged observation of this step (priv_dev [nenv, npriv]; nu, nobs, npriv: odk_model_obs_sizes), the same layout in
 * both tasks, offsets from the start of the env's row:
 *   last_act 13 + 2 nu (nu) | last_last_act 13 + 3 nu (nu) | gyro nobs (3) | local linvel nobs + 9 (3) | joint angles minus the default
 *   pose nobs + 15 (nu) | joint_vel nobs + 15 + nu (nu) | root_height nobs + 15 + 2 nu (1) | actuator_force nobs + 16 + 2 nu (nu) |
 *   contact nobs + 16 + 3 nu (2: left, right) | feet_vel nobs + 18 + 3 nu (2 x 3)
 * Scalar slots ([2]: left foot, right foot):
 *   SAMPLES               gait samples
 *   SPEED_SUM             sum of hypot(vx, vy) of the local linear velocity
 *   ABS_POWER_SUM         sum over samples and actuators of |actuator_force * joint_vel|
 *   CONTACT[2], DOUBLE, FLIGHT   samples with that foot, both feet, no foot in contact
 *   TOUCHDOWNS[2]         samples in contact whose previous sample was not; the env's first sample counts none
 *   SWING_STEPS_SUM[2]    at a touchdown, the length in samples of the non-contact run that ended (counted from the env's first sample)
 *   SLIP_SUM[2]           over the samples in contact, hypot of that foot's planar feet_vel
 *   HEIGHT_SUM, HEIGHT_SQ_SUM    of root_height
 *   ROLLPITCH_RATE_SQ_SUM gyro_x^2 + gyro_y^2
 *   ACTION_RATE_SUM       sum over actuators of (last_act - last_last_act)^2
 *   PREV_CONTACT[2], AIR_RUN[2]  bookkeeping: the last sample's contact, the length of the running non-contact run
 * Per-actuator arrays, entry u at SLOT + u, ODK_GAIT_STRIDE = 16 apart (entries nu .. 15 stay 0):
 *   TORQUE_SQ             sum of actuator_force^2
 *   TORQUE_PEAK, VEL_PEAK max |actuator_force|, max |joint_vel|
 *   SAT                   samples with |actuator_force| >= 0.99f * torque_limit[u] (float32); never counted when torque_limit_dev is NULL
 *                         or torque_limit[u] <= 0
 *   ABS_POWER             sum of |actuator_force * joint_vel|
 *   RANGE_MIN, RANGE_MAX  of the joint angle minus the default pose; the env's first sample initialises both
 * Every summed term is non-negative and added in float32 in step order.  done_dev / truncation_dev: [nenv] (a gait sample does not depend
 * on the truncation flag; the argument keeps the three accumulators' call shape); torque_limit_dev: [nu] device floats or NULL.  A null
 * pointer other than torque_limit_dev, or a model with more than ODK_GAIT_STRIDE actuators: ODK_ERR_INVALID, odk_last_error names the
 * argument, nothing is launched. */
#define ODK_GAIT_NACC 144
#define ODK_GAIT_STRIDE 16
enum { ODK_GAIT_SAMPLES = 0, ODK_GAIT_SPEED_SUM = 1, ODK_GAIT_ABS_POWER_SUM = 2, ODK_GAIT_CONTACT = 3, ODK_GAIT_DOUBLE = 5, ODK_GAIT_FLIGHT = 6,
       ODK_GAIT_TOUCHDOWNS = 7, ODK_GAIT_SWING_STEPS_SUM = 9, ODK_GAIT_SLIP_SUM = 11, ODK_GAIT_HEIGHT_SUM = 13, ODK_GAIT_HEIGHT_SQ_SUM = 14,
       ODK_GAIT_ROLLPITCH_RATE_SQ_SUM = 15, ODK_GAIT_ACTION_RATE_SUM = 16, ODK_GAIT_PREV_CONTACT = 17, ODK_GAIT_AIR_RUN = 19,
       ODK_GAIT_TORQUE_SQ = 32, ODK_GAIT_TORQUE_PEAK = 48, ODK_GAIT_VEL_PEAK = 64, ODK_GAIT_SAT = 80, ODK_GAIT_ABS_POWER = 96,
       ODK_GAIT_RANGE_MIN = 112, ODK_GAIT_RANGE_MAX = 128 };
int odk_gait_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                        const float* track_acc_dev, const float* torque_limit_dev /* [nu] or NULL */, float* acc_dev /* [nenv, ODK_GAIT_NACC] */,
                        void* stream);

/* Posture and stillness accumulator (does the head go where the posture commands send it, how fast does it settle, and does the rest of the
 * robot keep still meanwhile): one launch per evaluation step, graph-capturable, issued after odk_step and BEFORE odk_tracking_accumulate
 * (track_acc_dev [nenv, ODK_TRACK_NACC] is that function's accumulator: its ENDED slot then still says whether env e's first episode was
 * running when this step began).  Independent of odk_push_accumulate and odk_gait_accumulate.  Env e's row of acc_dev
 * [nenv, ODK_POSTURE_NACC], zeroed by the caller before the first step, is updated only on a sample: a step of e's first episode that is
 * not done (odk_gait_accumulate's gait sample).  Every other row keeps its bits.  The measured values are the noise-free privileged
 * observation of this step (priv_dev [nenv, npriv]; nu, nobs, npriv: odk_model_obs_sizes), the same layout in both tasks, offsets from the
 * start of the env's row:
 *   gyro nobs (3) | gravity nobs + 6 (3) | local linvel nobs + 9 (3) | joint angles minus the default pose nobs + 15 (nu) |
 *   joint_vel nobs + 15 + nu (nu) | root_height nobs + 15 + 2 nu (1)
 * The posture commands are entries 3 + k (k = 0..3: neck_pitch, head_pitch, head_yaw, head_roll) of the env's bound command row, the
 * default pose is the home keyframe's ctrl, and the actuator of slot k is the batch's head-joint map (odk_batch_set_head_joints; the duck's
 * shapes start with 5..8).  The head error of slot k, mapped to actuator u, in float32 and in this order:
 *   angle = P[nobs + 15 + u] + key_ctrl[u];   err = angle - cmd[3 + k]          (the step kernel's jq - cmd, up to the re-added default)
 * Scalar slots:
 *   SAMPLES               samples
 *   DRIFT_SPEED_SUM       sum of hypot(vx, vy) of the local linear velocity
 *   YAW_RATE_SQ_SUM       sum of gyro_z^2
 *   ROLLPITCH_RATE_SQ_SUM sum of gyro_x^2 + gyro_y^2
 *   TILT_SUM, TILT_PEAK   sum and maximum of hypot(g_x, g_y) of the gravity vector: the sine of the lean
 *   HEIGHT_SUM            sum of root_height
 *   LEG_POSE_SUM          sum over samples and over the actuators no slot maps to of |joint angle - default|
 *   LEG_VEL_SUM           likewise of |joint_vel|: the two parts of cost_stand_still(ignore_head=True)
 *   HEAD_SQERR_SUM        sum over samples and mapped slots of err^2: cost_head_pos without its move-command gate
 * Both hypots go through float64 (exact squares, a correctly rounded root, one rounding to float32), so a host restatement has TILT_PEAK's bits.
 * Per-slot arrays, entry k at SLOT + k (k = 0..3; the entries of a slot without an actuator stay 0):
 *   ANGLE_SUM             signed sum of angle
 *   ERR_SQ_SUM            sum of err^2
 *   ERR_PEAK              max |err|
 *   LAST_OFF              1-based index, among the env's samples, of the latest one with |err| > tol; 0 if none.  The settle time: the
 *                         episode starts at the home pose, so every run is a step response to the commanded posture
 * Every sum is float32, added in step order.  done_dev / truncation_dev: [nenv] (a sample does not depend on the truncation flag; the
 * argument keeps the accumulators' call shape).  ODK_ERR_INVALID, with the cause in odk_last_error and nothing launched: a null pointer
 * (the message names the argument), no bound commands, a batch without a head-joint map (not a duck shape and odk_batch_set_head_joints
 * never called; an all -1 map is a map: the head part of the row stays 0 and the stillness part is filled), a model with more than 16
 * actuators, a tol that is negative or not finite. */
#define ODK_POSTURE_NACC 32
enum { ODK_POSTURE_SAMPLES = 0, ODK_POSTURE_DRIFT_SPEED_SUM = 1, ODK_POSTURE_YAW_RATE_SQ_SUM = 2, ODK_POSTURE_ROLLPITCH_RATE_SQ_SUM = 3,
       ODK_POSTURE_TILT_SUM = 4, ODK_POSTURE_TILT_PEAK = 5, ODK_POSTURE_HEIGHT_SUM = 6, ODK_POSTURE_LEG_POSE_SUM = 7, ODK_POSTURE_LEG_VEL_SUM = 8,
       ODK_POSTURE_HEAD_SQERR_SUM = 9, ODK_POSTURE_ANGLE_SUM = 16, ODK_POSTURE_ERR_SQ_SUM = 20, ODK_POSTURE_ERR_PEAK = 24,
       ODK_POSTURE_LAST_OFF = 28 };
int odk_posture_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                           const float* track_acc_dev, float tol, float* acc_dev /* [nenv, ODK_POSTURE_NACC] */, void* stream);

/* Imitation-fidelity accumulator (does the policy walk the reference gait: which joints follow the reference motion, are the feet down when
 * the reference's are, does the robot touch down early or late in the cycle): one launch per evaluation step, graph-capturable, issued
 * after odk_step and BEFORE odk_tracking_accumulate (track_acc_dev [nenv, ODK_TRACK_NACC] is that function's accumulator: its ENDED slot then
 * still says whether env e's first episode was running when this step began).  Independent of odk_push_accumulate, odk_gait_accumulate and
 * odk_posture_accumulate; needs neither bound commands nor bound pushes.  Env e's row of acc_dev [nenv, ODK_IMIT_NACC], zeroed by the caller
 * before the first step, is updated only on a sample: a step of e's first episode that is not done (odk_gait_accumulate's gait sample).
 * Every other row keeps its bits.  All inputs are this step's privileged observation of the Joystick task (priv_dev [nenv, npriv]; nu,
 * nobs, npriv: odk_model_obs_sizes), offsets from the start of the env's row:
 *   command 6 (3) | local linvel nobs + 9 (3) | joint angles minus the default pose nobs + 15 (nu) | joint_vel nobs + 15 + nu (nu) |
 *   contact nobs + 16 + 3 nu (2: left, right) | F = current_reference_motion nobs + 26 + 3 nu (40)
 * F is the canonical frame the step's reward read: F[j], F[16 + j] position and velocity of frame joint j, F[32 + f] foot f's reference
 * contact, F[34 .. 36] the linear velocity.  Actuator u is compared with frame joint ri = imap[u], the batch's device copy of
 * odk_batch_set_imitation_joints read when the launch runs (a graph captured earlier follows a later map; -1: not compared), in float32 and
 * in this order, as the step kernel and odk_posture_accumulate do it (key_ctrl: the home keyframe's ctrl):
 *   jq = P[nobs + 15 + u] + key_ctrl[u];   dp = jq - F[ri];   dv = P[nobs + 15 + nu + u] - F[16 + ri]
 * Per foot f: c = contact[f] != 0, r = F[32 + f] > 0.5f.  Scalar slots ([2]: left foot, right foot):
 *   SAMPLES               samples
 *   GATED                 samples with sqrtf(c0 c0 + c1 c1 + c2 c2) > 0.01f of the command: the samples the imitation reward pays
 *   SPEED_ERR_SQ_SUM      sum of (s - sr)^2, s = hypot of the local linvel's x, y and sr = hypot(F[34], F[35]), both through float64
 *   REF_SPEED_SUM         sum of sr
 *   JOINT_POS_SQ_SUM      sum over samples and compared actuators of dp^2: the reward's joint_pos term before its weight 15
 *   JOINT_VEL_SQ_SUM      likewise of dv^2 (weight 1e-3)
 *   BOTH[2]               samples with c && r
 *   ROBOT_ONLY[2]         samples with c && !r
 *   REF_ONLY[2]           samples with !c && r  (the rest, neither, is SAMPLES minus the three)
 *   REF_TOUCHDOWNS[2]     samples with r whose previous sample had !r; the env's first sample counts none (odk_gait_accumulate's rule)
 *   TOUCHDOWNS[2]         robot touchdowns (c, and !c at the previous sample) while REF_AGE[f] > 0: those that have a lag
 *   LAG_SUM[2]            sum of lag over those touchdowns
 *   LAG_ABS_SUM[2]        sum of |lag|
 *   PREV_CONTACT[2], PREV_REF[2], REF_AGE[2]   bookkeeping: c and r of the previous sample; samples since the reference's latest touchdown
 * REF_AGE[f] is 0 until the reference's first counted touchdown, which sets it to 1; every later sample adds 1, and a later reference
 * touchdown sets it to 1 again.  Within a sample the reference is updated first, then lag = REF_AGE[f] - 1, and if period_steps > 0 and
 * 2 lag > period_steps, lag -= period_steps: negative means the robot touched down before the reference's NEXT touchdown.  Lags are small
 * integers in float32: LAG_SUM and LAG_ABS_SUM are exact.
 * Per-actuator arrays, entry u at SLOT + u, ODK_IMIT_STRIDE = 16 apart (entries of actuators with imap[u] < 0 and entries nu .. 15 stay 0):
 *   POS_ERR_SUM           signed sum of dp: the bias
 *   POS_ERR_SQ            sum of dp^2
 *   POS_ERR_PEAK          max |dp|
 *   VEL_ERR_SQ            sum of dv^2
 *   RANGE_MIN, RANGE_MAX  of jq; the env's first sample initialises both
 *   REF_RANGE_MIN, REF_RANGE_MAX   of F[ri]; the env's first sample initialises both
 * Every sum is float32, added in step order.  done_dev / truncation_dev: [nenv] (a sample does not depend on the truncation flag; the
 * argument keeps the accumulators' call shape).  period_steps: the reference motion's nb_steps_in_period, or 0 for lags that are not folded.
 * The reward's four base-velocity terms read world-frame qvel, which the privileged row does not carry: they are not measured here.
 * ODK_ERR_INVALID, with the cause in odk_last_error and nothing launched: a null pointer (the message names the argument), a Standing batch
 * (its privileged row has no frame), cfg.use_imitation == 0 (the frame is all zeros), a batch without an imitation joint map (not a duck
 * shape and odk_batch_set_imitation_joints never called), a model with more than ODK_IMIT_STRIDE actuators, period_steps < 0. */
#define ODK_IMIT_NACC 160
#define ODK_IMIT_STRIDE 16
enum { ODK_IMIT_SAMPLES = 0, ODK_IMIT_GATED = 1, ODK_IMIT_SPEED_ERR_SQ_SUM = 2, ODK_IMIT_REF_SPEED_SUM = 3, ODK_IMIT_JOINT_POS_SQ_SUM = 4,
       ODK_IMIT_JOINT_VEL_SQ_SUM = 5, ODK_IMIT_BOTH = 6, ODK_IMIT_ROBOT_ONLY = 8, ODK_IMIT_REF_ONLY = 10, ODK_IMIT_REF_TOUCHDOWNS = 12,
       ODK_IMIT_TOUCHDOWNS = 14, ODK_IMIT_LAG_SUM = 16, ODK_IMIT_LAG_ABS_SUM = 18, ODK_IMIT_PREV_CONTACT = 20, ODK_IMIT_PREV_REF = 22,
       ODK_IMIT_REF_AGE = 24,
       ODK_IMIT_POS_ERR_SUM = 32, ODK_IMIT_POS_ERR_SQ = 48, ODK_IMIT_POS_ERR_PEAK = 64, ODK_IMIT_VEL_ERR_SQ = 80, ODK_IMIT_RANGE_MIN = 96,
       ODK_IMIT_RANGE_MAX = 112, ODK_IMIT_REF_RANGE_MIN = 128, ODK_IMIT_REF_RANGE_MAX = 144 };
int odk_imitation_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                             const float* track_acc_dev, int period_steps, float* acc_dev /* [nenv, ODK_IMIT_NACC] */, void* stream);

/* Command schedules (replaces the keyboard of mujoco_infer.py: walk, then stop; forward, then turn): the command of an env changes at given
 * steps of its first episode, inside a captured evaluation step.  A schedule is nseg <= ODK_SCHED_MAX_SEGMENTS segments of
 * ODK_SCHED_SEG_FLOATS floats: start_step, then the 7 command entries in cmd_range order.  Segment 0 starts at step 0, the starts are whole
 * numbers and strictly increasing, and unused trailing segments carry ODK_SCHED_NEVER (above every float32 step count) as start_step.
 * sched_dev: [nsched, nseg, ODK_SCHED_SEG_FLOATS] device floats; sched_of_env_dev: [nenv] int32, env e's schedule (clamped into
 * 0 .. nsched - 1 by the kernels, which never read outside the table); track_acc_dev: [nenv, ODK_TRACK_NACC], odk_tracking_accumulate's.
 * The host cannot see device tables: their contents are the caller's to validate.
 *
 * odk_command_schedule_apply: one launch, graph-capturable, issued BEFORE odk_step.  The tracking accumulator is the clock: STEPS of env e
 * is then the index t of e's first-episode step that is about to run, the segment in force is the last one with start_step <= t, and its
 * command overwrites entries 0..6 of env e's row in the BOUND command buffer (odk_batch_bind_commands: the batch holds the pointer and the
 * stride; the buffer is the caller's, and binding it says that this launch may write it).  Columns beyond 6 of a wider row are left alone.
 * An env whose ENDED is set has no step about to run in its first episode: it gets the command of the step that ended it (t = STEPS - 1),
 * the segment it ended in; none of the accumulators reads it afterwards.  With a zeroed tracking accumulator the launch writes segment
 * 0's command everywhere, which is what odk_reset must find: issue it once before the reset.  No counter, no per-env state: the launch is
 * a pure function of its inputs.  ODK_ERR_INVALID, with the cause in odk_last_error and nothing launched: a null pointer (the message names
 * the argument), no bound commands, nseg outside 1 .. ODK_SCHED_MAX_SEGMENTS, nsched < 1. */
#define ODK_SCHED_MAX_SEGMENTS 8
#define ODK_SCHED_SEG_FLOATS 8
#define ODK_SCHED_NEVER 1.0e9f
int odk_command_schedule_apply(const odk_batch* b, const float* sched_dev, int nsched, int nseg, const int32_t* sched_of_env_dev,
                               const float* track_acc_dev, void* stream);

/* Step-response accumulator (how fast does the policy follow a new command, how far does it overshoot, where does it settle): one launch
 * per evaluation step, graph-capturable, issued after odk_step and BEFORE odk_tracking_accumulate (track_acc_dev's ENDED slot then still
 * says whether env e's first episode was running when this step began, and its STEPS slot is the index t of the step that just ran), with
 * odk_push_accumulate's contract.  Env e's row of acc_dev [nenv, ODK_RESP_NACC], zeroed by the caller before the first step, holds one block
 * of ODK_RESP_STRIDE floats per segment; a launch touches only the block of the segment in force at step t (the last one with start_step
 * <= t, as odk_command_schedule_apply chose it before the step), and only during e's first episode.  Every other float keeps its bits.
 * A sample is odk_tracking_accumulate's velocity sample (a step that is not done), the achieved velocities and the errors are
 * odk_push_accumulate's: local linear velocity at nobs + 9 and yaw rate at nobs + 2 of priv_dev [nenv, npriv]; the planar error
 * hypot(vx - cx, vy - cy) through float64 with one rounding to float32, the yaw error |wz - cwz| in float32; the command c is the
 * segment's, read from the bound row.  k = t - start_step + 1 is the 1-based index of step t among the steps of its segment.  Per segment:
 *   ENTERED         1 once a first-episode step ran in the segment
 *   SAMPLES         velocity samples in the segment
 *   FELL            1 when the first episode ended in this segment with done and no truncation
 *   STEPS_TO_FALL   k of that done step: the steps from the segment's first step to it, counting both
 *   FIRST_IN        k of the first sample with planar error <= lin_tol AND yaw error <= ang_tol; 0 if none.  The response time
 *   LAST_OFF        k of the latest sample beyond either tolerance; 0 if none.  The settle time, a running "last seen" as ODK_PUSH_LAST_OFF
 *   PEAK_LIN_ERR, PEAK_ANG_ERR   maxima of the two errors over the samples at or after FIRST_IN's (0 while FIRST_IN is 0): how far the policy
 *                   leaves the command again once it has reached it
 *   SUM[3], SQERR[3]   of vx, vy, wz and of their squared errors against the segment's command, as ODK_TRACK_SUM / ODK_TRACK_SQERR
 *   OVERSHOOT[3]    per axis the maximum over the samples of (v - c) * sign(c - c_prev), floored at 0; c_prev is the previous segment's
 *                   command on that axis from the table, 0 for segment 0 (the episode starts at rest); an axis whose command did not change
 *                   keeps 0
 *   TAIL_SAMPLES, TAIL_SUM[3]   count of, and sum of the achieved velocities over, the samples with k > tail_after: the steady state after
 *                   the transient
 * Every sum is float32, added in step order, every product is rounded before it is added (no fused multiply-add), one thread owns an env's
 * row and there are no atomics: a host restatement in float32 has the bits, and a replay is deterministic.  ODK_ERR_INVALID, with the
 * cause in odk_last_error and nothing launched: a null pointer (the message names the argument), no bound commands, a tolerance that is
 * negative or not finite, tail_after < 0, nseg outside 1 .. ODK_SCHED_MAX_SEGMENTS, nsched < 1. */
#define ODK_RESP_STRIDE 24
#define ODK_RESP_NACC (ODK_SCHED_MAX_SEGMENTS * ODK_RESP_STRIDE)
enum { ODK_RESP_ENTERED = 0, ODK_RESP_SAMPLES = 1, ODK_RESP_FELL = 2, ODK_RESP_STEPS_TO_FALL = 3, ODK_RESP_FIRST_IN = 4, ODK_RESP_LAST_OFF = 5,
       ODK_RESP_PEAK_LIN_ERR = 6, ODK_RESP_PEAK_ANG_ERR = 7, ODK_RESP_SUM = 8, ODK_RESP_SQERR = 11, ODK_RESP_OVERSHOOT = 14,
       ODK_RESP_TAIL_SAMPLES = 17, ODK_RESP_TAIL_SUM = 18 };
int odk_response_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                            const float* track_acc_dev, const float* sched_dev, int nsched, int nseg, const int32_t* sched_of_env_dev,
                            float lin_tol, float ang_tol, int tail_after, float* acc_dev /* [nenv, ODK_RESP_NACC] */, void* stream);

/* Fall recorder (why, when and which way does the policy fall: the last second before the termination of every env, replayable): one launch
 * per evaluation step, graph-capturable, issued after odk_step and BEFORE odk_tracking_accumulate (track_acc_dev's ENDED slot then still
 * says whether env e's first episode was running when this step began, and its STEPS slot is the index t of the step that just ran), with
 * odk_push_accumulate's contract.  Unlike the accumulators above it keeps samples, not sums: env e's row of acc_dev [nenv, row_stride],
 * zeroed by the caller before the first step, is ODK_FALL_HEAD floats and then a ring of `ring` slots of ODK_FALL_SAMPLE + nq floats
 * (odk_fall_row_floats; nq: odk_model_dims).  The row is touched only during e's first episode; every other float keeps its bits: rows of
 * ended envs, slots not written this step, the floats between odk_fall_row_floats and a wider row_stride, rows past the batch.
 * A sample is odk_gait_accumulate's: a first-episode step that is not done (a done step's observation and state are the auto-reset's), so
 * the latest sample of a fall is the step before the termination.  Sample number s (0-based: SAMPLES before the step) goes to slot
 * s % ring, all float32 copies of this step's outputs -- priv_dev [nenv, npriv] (nu, nobs, npriv: odk_model_obs_sizes; both tasks), the
 * env's bound command row c and the batch's own state record:
 *   S_STEP          t, the index of the step among the steps of the first episode
 *   S_UP[3]         the up vector, priv nobs + 6 (the "gravity" sensor: the imu site's z axis in world coordinates)
 *   S_GYRO[3]       priv nobs
 *   S_LINVEL[3]     local linear velocity, priv nobs + 9
 *   S_HEIGHT        root height, priv nobs + 15 + 2 nu
 *   S_CONTACT[2]    left, right foot, priv nobs + 16 + 3 nu
 *   S_LIN_ERR       hypot(vx - cx, vy - cy) through float64 with one rounding to float32 (odk_push_accumulate's planar error), against the
 *                   bound command row as the step left it: under a command schedule the row odk_command_schedule_apply wrote
 *   S_ANG_ERR       |wz - cwz| in float32, wz = priv nobs + 2
 *   S_SAT           the number of actuators with |actuator_force| >= 0.99f * torque_limit[u] (actuator_force: priv nobs + 16 + 2 nu; float32;
 *                   odk_gait_accumulate's rule: 0 when torque_limit_dev is NULL, an actuator with torque_limit[u] <= 0 never counts)
 *   then qpos[0 .. nq) of the env, at ODK_FALL_SAMPLE
 * Head slots:
 *   SAMPLES         samples so far: a ring holds the last min(SAMPLES, ring) of them, the oldest in slot SAMPLES % ring once SAMPLES >= ring,
 *                   in slot 0 before
 *   FELL            1 when the first episode ended with done and no truncation
 *   FALL_STEP       t of that done step (the first episode's length minus one)
 *   LAST_UPRIGHT    1-based number of the latest sample with tilt <= tilt_tol, tilt = hypot(up_x, up_y) through float64
 *                   (ODK_POSTURE_TILT_PEAK's: the sine of the lean); 0 if none
 *   UPRIGHT_CONTACT[2]   S_CONTACT of that sample: the support the robot left the upright on
 *   TILT_PEAK       maximum of tilt over the samples: how close a survivor came
 * Slots 7 .. 15 stay 0.  A truncated first episode writes nothing at its done step.  No sums: every stored float is a copy, a small whole
 * number or a correctly rounded root, so a host restatement has the row's bits; one 16-lane row owns an env's row and there are no atomics.
 * ODK_ERR_INVALID, with the cause in odk_last_error and nothing launched: a null pointer other than torque_limit_dev (the message names the
 * argument), no bound commands, ring outside 1 .. ODK_FALL_MAX_RING, row_stride < odk_fall_row_floats, a model with more than 16
 * actuators, a tilt_tol that is negative or not finite. */
#define ODK_FALL_HEAD 16        /* floats before the ring */
#define ODK_FALL_SAMPLE 16      /* scalars of a ring slot, before its qpos */
#define ODK_FALL_MAX_RING 64
enum { ODK_FALL_SAMPLES = 0, ODK_FALL_FELL = 1, ODK_FALL_STEP = 2, ODK_FALL_LAST_UPRIGHT = 3, ODK_FALL_UPRIGHT_CONTACT = 4 /* [2] */,
       ODK_FALL_TILT_PEAK = 6 /* 7..15 stay 0 */ };
enum { ODK_FALL_S_STEP = 0, ODK_FALL_S_UP = 1 /* [3] */, ODK_FALL_S_GYRO = 4 /* [3] */, ODK_FALL_S_LINVEL = 7 /* [3] */, ODK_FALL_S_HEIGHT = 10,
       ODK_FALL_S_CONTACT = 11 /* [2] */, ODK_FALL_S_LIN_ERR = 13, ODK_FALL_S_ANG_ERR = 14, ODK_FALL_S_SAT = 15 };
int odk_fall_row_floats(const odk_batch* b, int ring);   /* ODK_FALL_HEAD + ring * (ODK_FALL_SAMPLE + nq); < 0 for a bad ring */
int odk_fall_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                        const float* track_acc_dev, const float* torque_limit_dev /* [nu] or NULL */, float tilt_tol, int ring,
                        float* acc_dev /* [nenv, row_stride] */, int row_stride, void* stream);

/* Paths and waypoints (where did it end up, and can something steer it: the odometry of every env, and a waypoint follower on top of the
 * joystick command).  Three launches, one thread per env, graph-capturable, no LDS; they read the base pose from the batch's own state
 * record (qpos at offset 0 of the env's row, as the fall recorder) and leave the step, reset and physics kernels alone.  Reset draws every
 * env's own xy offset and yaw, so every pose quantity is expressed in the env's START FRAME: the base position and heading right after
 * odk_reset.  Definitions, shared by the three:
 *   pose             p = qpos[0:2] and the heading h of the base quaternion (w, x, y, z) = qpos[3:7]: hx = 1 - 2 (y y + z z),
 *                    hy = 2 (x y + w z), divided by their length n = hypot(hx, hy) (through float64, one rounding to float32); n < 1e-6 (the
 *                    base pitched onto its nose: no heading) gives h = (1, 0)
 *   start-frame position of a pose against a stored start (sx, sy, shx, shy): r = p - s, xs = r . sh, ys = sh x r = shx ry - shy rx
 *   start-frame heading   (c, s) = (sh . h, sh x h)
 * Arithmetic is float32 + - * /, comparisons, fminf / fmaxf and that hypot; every product is rounded before it is added (no fused
 * multiply-add), there is no atan2, sin or cos on the device, one thread owns an env's row and there are no atomics: a float32 host
 * restatement has the bits, and a replay is deterministic.  A model whose first joint is not a free joint has no base pose:
 * ODK_ERR_UNSUPPORTED.  Every other refusal is ODK_ERR_INVALID with the cause in odk_last_error, and nothing is launched.
 *
 * Env e's row of acc_dev [nenv, ODK_PATH_NACC]:
 *   START_X, START_Y, START_HX, START_HY   the start pose (odk_path_begin)
 *   X, Y, HX, HY     the pose at the last sample (odk_path_begin: the start pose)
 *   LENGTH           sum over the samples of hypot(x - X, y - Y): the path length in metres
 *   TURN             sum over the samples of HX hy - HY hx = sin(dpsi), the heading change between two samples.  At 50 Hz and |wz| <= 1 rad/s
 *                    dpsi <= 0.02 rad, so the sum differs from the sum of dpsi (the heading change in radians, turns counted) by less than
 *                    dpsi^2 / 6 < 1e-4 relative
 *   SAMPLES          samples taken
 *   FELL, FELL_LEG   1 when the first episode ended with done and no truncation, and the waypoint index (WP_INDEX) it was heading for
 *   WP_INDEX         the waypoint the env is heading for: the number of waypoints reached so far
 *   XTRACK_SAMPLES, XTRACK_SQ, XTRACK_PEAK   count of, sum of squares of and maximum of the cross-track distance (below)
 *   GOAL_DIST        start-frame distance to the course's last waypoint at the latest sample taken while a waypoint was still ahead
 *   REACHED[8]       per waypoint the 1-based index of the first-episode step at which it was reached; 0: not reached
 * Slots past REACHED + 8 stay 0.
 *
 * odk_path_begin: issued after odk_reset.  Zeroes env e's row and stores the current pose in START_* and in X, Y, HX, HY.
 *
 * odk_path_accumulate: one launch per evaluation step, issued after odk_step and BEFORE odk_tracking_accumulate, with odk_push_accumulate's
 * ENDED / STEPS contract (track_acc_dev [nenv, ODK_TRACK_NACC]).  An env past its first episode is not touched.  A done step takes no
 * sample (the record is the auto-reset's state); with truncation 0 it sets FELL and FELL_LEG.  A sample step adds to LENGTH, TURN and
 * SAMPLES and stores the new pose in X, Y, HX, HY.  With a course (course_dev not NULL) and i = WP_INDEX below the course's count it then
 * takes dist, the start-frame distance to waypoint i, and the cross-track distance xt: from the start-frame position to the segment from
 * waypoint i - 1 (the origin for i = 0) to waypoint i, the projection parameter clamped to 0 .. 1, a zero-length leg the distance to the
 * point; XTRACK_SAMPLES += 1, XTRACK_SQ += xt xt, XTRACK_PEAK = max; GOAL_DIST = the distance to the last waypoint; and when
 * dist <= radius, REACHED[i] = STEPS + 1 and WP_INDEX = i + 1: at most one waypoint per step.  course_dev NULL with ncourse 0 is the plain
 * odometry mode; it needs no bound commands (nor does a course: the accumulator reads no command).  Refused: a null pointer (the message
 * names the argument), course_dev without course_of_env_dev, course_dev NULL with ncourse != 0, ncourse < 1 with a course, a radius that
 * is negative or not finite.
 *
 * Courses: course_dev is [ncourse, ODK_PATH_COURSE_FLOATS] device floats, a row the count and then up to ODK_PATH_MAX_WAYPOINTS points
 * (x, y) in start-frame metres; course_of_env_dev [nenv] int32 is env e's course, clamped into 0 .. ncourse - 1 by the kernels, which also
 * clamp the count into 0 .. ODK_PATH_MAX_WAYPOINTS: they never read outside the table.  The host cannot see device tables: their contents
 * are the caller's to validate.
 *
 * odk_waypoint_command_apply: one launch, issued BEFORE odk_step: a pure-pursuit-like heading controller that writes entries 0..2 (vx, vy,
 * wz) of env e's row of the BOUND command buffer (odk_command_schedule_apply's contract: binding the buffer says this launch may write
 * it).  Entries 3 and beyond keep their bits, and so does any column past 6 of a wider row.  The row of an env whose ENDED is set is not
 * written.  At clock 0 (STEPS == 0, not ENDED) the pose IS the start pose by definition -- position (0, 0), heading (1, 0) -- and neither
 * the records nor START_* are read: the launch before odk_reset gives the reset's observation its command from stale records.  Otherwise
 * the pose comes from the records against START_*.  With i = WP_INDEX: i == count, the course is finished: (0, 0, 0).  Else d = w_i -
 * (xs, ys), dist = hypot(d); dist < 1e-6: f = 1, l = 0, otherwise f = (d . (c, s)) / dist and l = ((c, s) x d) / dist; turn = f >= 0 ? l :
 * (l >= 0 ? 1 : -1) (a target exactly behind turns left); wz = clamp(heading_gain turn, +-turn_rate); vx = v_cruise max(f, 0), on the
 * course's last waypoint times min(1, dist / slow_dist); vy = 0.  Refused: a null pointer (the message names the argument), no bound
 * commands, ncourse < 1, slow_dist or heading_gain not finite and positive, v_cruise or turn_rate not finite and >= 0. */
#define ODK_PATH_NACC 32
#define ODK_PATH_MAX_WAYPOINTS 8
#define ODK_PATH_COURSE_FLOATS (1 + 2 * ODK_PATH_MAX_WAYPOINTS)
enum { ODK_PATH_START_X = 0, ODK_PATH_START_Y = 1, ODK_PATH_START_HX = 2, ODK_PATH_START_HY = 3, ODK_PATH_X = 4, ODK_PATH_Y = 5, ODK_PATH_HX = 6,
       ODK_PATH_HY = 7, ODK_PATH_LENGTH = 8, ODK_PATH_TURN = 9, ODK_PATH_SAMPLES = 10, ODK_PATH_FELL = 11, ODK_PATH_FELL_LEG = 12,
       ODK_PATH_WP_INDEX = 13, ODK_PATH_XTRACK_SAMPLES = 14, ODK_PATH_XTRACK_SQ = 15, ODK_PATH_XTRACK_PEAK = 16, ODK_PATH_GOAL_DIST = 17,
       ODK_PATH_REACHED = 18 /* [8]; 26..31 stay 0 */ };
int odk_path_begin(const odk_batch* b, float* acc_dev /* [nenv, ODK_PATH_NACC] */, void* stream);
int odk_path_accumulate(const odk_batch* b, const float* done_dev, const float* truncation_dev, const float* track_acc_dev,
                        const float* course_dev /* [ncourse, ODK_PATH_COURSE_FLOATS] or NULL */, int ncourse,
                        const int32_t* course_of_env_dev /* [nenv] or NULL without a course */, float radius,
                        float* acc_dev /* [nenv, ODK_PATH_NACC] */, void* stream);
int odk_waypoint_command_apply(const odk_batch* b, const float* course_dev, int ncourse, const int32_t* course_of_env_dev,
                               const float* track_acc_dev, const float* path_acc_dev, float v_cruise, float turn_rate, float heading_gain,
                               float slow_dist, void* stream);

/* Sensor faults: a stage between the observation the env kernels wrote and the policy that reads it, which makes the row look like what
 * a faulty robot's sensors would deliver -- a tilted, biased, mis-scaled or late IMU, late, offset or quantised encoders, a foot switch
 * that sticks.  One launch, a 16-lane row per env (lane = actuator for the joint columns, lanes 0..5 the IMU, lanes 6..7 the foot
 * switches), graph-capturable, no LDS, no scratch.  It is OUT OF PLACE: obs_dev (the step's observation, [nenv, nobs]) is only read and
 * obs_out_dev must not overlap it; the env kernels, the privileged row and with it every report keep their meaning under a fault.  nu,
 * nobs and the env kind are the batch's.  The columns it touches (csrc/odk_obs_layout.h obs_at): gyro [3] at 0, accelerometer [3] at 3,
 * joint positions [nu] at 13, joint velocities [nu] at 13 + nu, contacts [2] at 13 + 6 nu (Joystick) or 13 + 5 nu (Standing).  Every other
 * column -- command, the three action memories, motor targets, phase -- is copied through bit for bit.
 *
 * Env e's row of fault_dev [nenv, ODK_SENSOR_NPRM]:
 *   IMU_ROT[9]       row-major mounting rotation R, applied to gyro and accelerometer (built on the host: no sin / cos runs on the device)
 *   GYRO_SCALE, GYRO_BIAS[3], ACC_SCALE, ACC_BIAS[3]   out = scale (R x) + bias
 *   IMU_DELAY, JOINT_DELAY   whole steps; the kernel clamps them into 0 .. ODK_SENSOR_RING - 1 (NaN: 0) and drops a fraction.  IMU_DELAY
 *                    covers gyro and accelerometer, JOINT_DELAY joint positions and velocities
 *   ENC_QUANT        q > 0: position = q rintf(position / q), after the offset; otherwise off
 *   CONTACT_MODE[2]  0 = pass through, 1 = stuck at 0, 2 = stuck at 1 (any other value passes through); left foot, then right foot
 *   ENC_OFFSET[16]   per-actuator additive zero error on the joint-position columns
 * Slots 22 .. 31 are not read.  The NOMINAL row is R = identity, both scales 1 and 0 elsewhere, and it hands back the input's bits for
 * every value, -0.0, NaN and +-inf included: a stage whose parameters are nominal is skipped by a select, never computed (1 x + 0 would
 * turn -0.0 into +0.0, 0 inf is NaN).  The stages, each with its own select: the rotation when R is not exactly the identity, a scale
 * when it is not 1, a bias or an offset when it is not 0, the quantiser when q > 0.
 *
 * Env e's row of state_dev [nenv, ODK_SENSOR_NSTATE] (zeroed by the caller before an episode's first call): slot ODK_SENSOR_HEAD is the
 * number of samples since the last refill (slots 1 .. 15 are not touched), then a ring of the last ODK_SENSOR_RING RAW samples of
 * ODK_SENSOR_SAMPLE floats each: gyro [3] and accelerometer [3] at ODK_SENSOR_S_IMU (the ten floats behind them are not touched), joint
 * positions [16] at ODK_SENSOR_S_JOINT_POS and joint velocities [16] at ODK_SENSOR_S_JOINT_VEL (0 in the entries past nu).  The ring holds
 * raw values: its contents do not depend on the fault row.  Order per call: when HEAD is 0 or done_dev[e] != 0 (done_dev may be NULL) EVERY
 * slot is filled with the current sample and HEAD becomes 1 -- the observation after a done step is the new episode's first one, and a
 * delayed sensor then shows it, not zeros (BUILD-DEFINED: the reference zero-fills its imu_history, and a zero accelerometer is no
 * plausible reading) -- otherwise the sample goes to slot HEAD mod ODK_SENSOR_RING and HEAD grows by 1 (a float: exact for 2^24 samples);
 * then the sample `delay` slots back is taken; then rotation, scale and bias (IMU), or offset and quantiser (encoders).
 * Arithmetic is float32 + * / and rintf with every product rounded before it is added (no fused multiply-add), R x summed left to right:
 * a numpy restatement has every bit.  Refused (ODK_ERR_INVALID, nothing launched): a null pointer other than done_dev (the message names
 * the argument), obs_out_dev overlapping obs_dev, a model with more than 16 actuators. */
#define ODK_SENSOR_NPRM 48
#define ODK_SENSOR_RING 8
#define ODK_SENSOR_SAMPLE 48
#define ODK_SENSOR_NSTATE (16 + ODK_SENSOR_RING * ODK_SENSOR_SAMPLE)
enum { ODK_SENSOR_IMU_ROT = 0 /* [9] */, ODK_SENSOR_GYRO_SCALE = 9, ODK_SENSOR_GYRO_BIAS = 10 /* [3] */, ODK_SENSOR_ACC_SCALE = 13,
       ODK_SENSOR_ACC_BIAS = 14 /* [3] */, ODK_SENSOR_IMU_DELAY = 17, ODK_SENSOR_JOINT_DELAY = 18, ODK_SENSOR_ENC_QUANT = 19,
       ODK_SENSOR_CONTACT_MODE = 20 /* [2]; 22..31 are not read */, ODK_SENSOR_ENC_OFFSET = 32 /* [16] */ };
enum { ODK_SENSOR_HEAD = 0 /* 1..15 are not touched */, ODK_SENSOR_RING_AT = 16 /* the ring's first slot */, ODK_SENSOR_S_IMU = 0 /* [6] */,
       ODK_SENSOR_S_JOINT_POS = 16 /* [16] */, ODK_SENSOR_S_JOINT_VEL = 32 /* [16] */ };
int odk_sensor_apply(const odk_batch* b, const float* obs_dev /* [nenv, nobs], the step's */, const float* done_dev /* may be NULL */,
                     const float* fault_dev /* [nenv, ODK_SENSOR_NPRM] */, float* state_dev /* [nenv, ODK_SENSOR_NSTATE] */,
                     float* obs_out_dev /* [nenv, nobs], must not alias obs_dev */, void* stream);

/* Actuation faults: a stage between the policy's action and odk_step, which turns the action the policy asked for into the one the servos
 * receive -- a gain error, a mis-indexed horn, command noise, a clamp, the runtime's low-pass filter, the servo's position resolution, a
 * lost packet, a servo that drops off the bus.  One launch, a 16-lane row per env (lane = actuator), graph-capturable, no LDS, no scratch.
 * It is OUT OF PLACE: act_dev (the policy's action, [nenv, nu]) is only read and act_out_dev must not overlap it; the caller hands
 * act_out_dev to odk_step.  nu is the batch's.  Every entry of a fault row is in ACTION UNITS: the env turns an action into a target as
 * default + action * action_scale, so a figure in radians is divided by action_scale on the host.
 *
 * Env e's row of fault_dev [nenv, ODK_ACT_NPRM], in stage order (x < y, x > y and x >= y are false for a NaN, so a NaN parameter leaves
 * its stage off):
 *   GAIN             a = gain a                                   when gain < 1 or gain > 1
 *   OFFSET[16]       a = a + offset[lane]                         when offset < 0 or offset > 0
 *   NOISE            a = a + A ((u + u) - 1), u of stream 1 + lane   when A > 0
 *   LIMIT            a = fminf(fmaxf(a, -L), L)                   when L > 0
 *   ALPHA            y = (alpha y_prev) + ((1 - alpha) a), FILT[lane] = y, a = y   when alpha > 0 (1 - alpha is formed on the device; with
 *                    the filter off FILT keeps its value).  The reference's LowPassActionFilter, alpha = (1 / cutoff) / (dt + 1 / cutoff)
 *   QUANT            a = q rintf(a / q)                           when q > 0
 *   DROP_P, DROP_LEN packet loss, below
 *   FREEZE_AT[16]    the actuator delivers its previous delivered value   when f >= 0 and the episode step >= f
 *   SEED             a whole number in 0 .. 2^24 - 1: fminf(fmaxf(seed, 0), 16777215) (NaN: 0), a fraction dropped
 * Slots 8 .. 15 are not read.  The NOMINAL row is GAIN 1, DROP_LEN 1, every FREEZE_AT -1 and 0 elsewhere, and it hands back the input's
 * bits for every value, -0.0, NaN and +-inf included: every nominal stage is a select, never arithmetic.
 *
 * Env e's row of state_dev [nenv, ODK_ACT_NSTATE] (zeroed by the caller before an episode's first call): HEAD, the calls since the last
 * refill = the episode step of the current call (a float: exact for 2^24 calls); EPISODE, the refill count; HOLD, the loss steps still to
 * come; CALLS and DROPS, the calls and the calls whose packet was lost since the row was zeroed (a refill does not reset them); slots
 * 5 .. 15 are not touched; FILT[16], the filter's state, and PREV[16], the action last delivered (entries past nu are not touched).
 * Order per call:
 *   1. refill, when HEAD is 0 or done_dev[e] != 0 (done_dev may be NULL): FILT and PREV count as 0 (the reference's last_action = 0:
 *      action 0 is the default pose, where the episode starts), HOLD as 0, EPISODE grows by 1 and the step is 0;
 *   2. gain, offset, noise, limit, filter, quantiser (the runtime's side of the bus);
 *   3. packet loss, the same for the row's 16 lanes: HOLD > 0 -- lost, HOLD falls by 1; otherwise u(stream 0) < DROP_P -- lost, and
 *      HOLD = fmaxf(DROP_LEN, 1) - 1.  A lost packet delivers PREV on every actuator.  FILT advances on a lost packet too: the runtime
 *      does not know the bus dropped it;
 *   4. freeze, per lane;
 *   5. PREV = delivered (lanes below nu), HEAD + 1, CALLS + 1, DROPS + 1 if the packet was lost.
 * Random numbers are stateless (a captured graph, an eager run and a host restatement agree), uint32 arithmetic only:
 *   x = seed + 0x9E3779B9 env + 0x85EBCA6B episode + 0xC2B2AE35 step + 0x27D4EB2F stream   (mod 2^32; env = index in the batch, episode =
 *       EPISODE after the refill, step = the episode step)
 *   x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16;  u = float(x >> 8) * 2^-24   (0 <= u < 1, exact)
 * Arithmetic is float32 + - * / and rintf with every product rounded before it is added (no fused multiply-add): a numpy restatement has
 * every bit.  Refused (ODK_ERR_INVALID, nothing launched): a null pointer other than done_dev (the message names the argument),
 * act_out_dev overlapping act_dev, a model with more than 16 actuators. */
#define ODK_ACT_NPRM 48
#define ODK_ACT_NSTATE 48
enum { ODK_ACT_GAIN = 0, ODK_ACT_NOISE = 1, ODK_ACT_LIMIT = 2, ODK_ACT_ALPHA = 3, ODK_ACT_QUANT = 4, ODK_ACT_DROP_P = 5, ODK_ACT_DROP_LEN = 6,
       ODK_ACT_SEED = 7 /* 8..15 are not read */, ODK_ACT_OFFSET = 16 /* [16] */, ODK_ACT_FREEZE_AT = 32 /* [16] */ };
enum { ODK_ACT_HEAD = 0, ODK_ACT_EPISODE = 1, ODK_ACT_HOLD = 2, ODK_ACT_CALLS = 3, ODK_ACT_DROPS = 4 /* 5..15 are not touched */,
       ODK_ACT_FILT = 16 /* [16] */, ODK_ACT_PREV = 32 /* [16] */ };
int odk_action_apply(const odk_batch* b, const float* act_dev /* [nenv, nu], the policy's, only read */, const float* done_dev /* may be NULL */,
                     const float* fault_dev /* [nenv, ODK_ACT_NPRM] */, float* state_dev /* [nenv, ODK_ACT_NSTATE] */,
                     float* act_out_dev /* [nenv, nu], must not overlap act_dev */, void* stream);

/* Fault resampling: training under sensor and actuation faults that are redrawn per episode.  At the start of each episode env e's row of
 * the sensor fault table (odk_sensor_apply's fault_dev) and of the actuation fault table (odk_action_apply's) is rewritten from a small
 * table of ranges, so that a rollout meets a new faulty robot every episode.  Issued BEFORE the two stages of the same step, with the same
 * done_dev.  One launch, a 16-lane row per env with six slots per lane, graph-capturable, no LDS, no scratch.
 *
 * spec_dev [3][ODK_FAULT_NSLOT], only read: row 0 is lo, row 1 hi, row 2 the slot's kind.  Slot s < ODK_SENSOR_NPRM is slot s of the sensor
 * row, slot s >= ODK_SENSOR_NPRM slot s - ODK_SENSOR_NPRM of the actuation row.  The kinds (a float holding 0, 1 or 2; any other value, a
 * NaN included, counts as 0), with u the slot's draw:
 *   ODK_FAULT_FIXED    lo's bits (a select, no arithmetic: NaN and -0.0 are kept)
 *   ODK_FAULT_UNIFORM  lo + ((hi - lo) u)
 *   ODK_FAULT_WHOLE    fminf(lo + floorf(((hi - lo) + 1) u), hi): the whole numbers lo .. hi, each as likely (whole steps, the actuation
 *                      SEED); the clamp because the rounded product can reach the span
 *   u = odk_action_apply's stateless draw with x = seed + 0x9E3779B9 (env_id_offset + e) + 0x85EBCA6B episode + 0x27D4EB2F (32 + s): step
 *       0, episode = EPISODE after the redraw, stream 32 + s (the action stage draws from streams 0 .. 16).  An eager run, a captured
 *       graph, ranks with their own env_id_offset and a host restatement agree.
 *
 * Env e's row of state_dev [nenv, ODK_FAULT_NSTATE] (zeroed by the caller before an episode's first call): HEAD, the calls since the row was
 * zeroed, and EPISODE, the redraw count (floats: exact for 2^24); slots 2 and 3 are not touched.  Order per call: env e redraws when HEAD is
 * 0 or done_dev[e] != 0 (done_dev may be NULL) -- the condition on which both stages refill, so with rows zeroed together a redraw and the
 * stages' refills coincide; on a redraw EPISODE grows by 1 and all ODK_FAULT_NSLOT slots of env e are stored, the slots the stages do not
 * read included; otherwise neither row of env e is touched; HEAD grows by 1 either way.  Both state loads come before the first store.
 * Arithmetic is float32 + - * and floorf with every product rounded before it is added (no fused multiply-add): a numpy restatement has
 * every bit.  Refused (ODK_ERR_INVALID, nothing launched): a null pointer other than done_dev (the message names the argument), the two
 * fault tables overlapping each other or spec_dev. */
#define ODK_FAULT_NSLOT (ODK_SENSOR_NPRM + ODK_ACT_NPRM)
#define ODK_FAULT_NSTATE 4
enum { ODK_FAULT_HEAD = 0, ODK_FAULT_EPISODE = 1 /* 2..3 are not touched */ };
enum { ODK_FAULT_FIXED = 0, ODK_FAULT_UNIFORM = 1, ODK_FAULT_WHOLE = 2 };
int odk_fault_resample(const odk_batch* b, const float* done_dev /* may be NULL */,
                       const float* spec_dev /* [3][ODK_FAULT_NSLOT]: lo, hi, kind */, uint32_t seed, uint32_t env_id_offset,
                       float* state_dev /* [nenv, ODK_FAULT_NSTATE] */, float* sensor_fault_dev /* [nenv, ODK_SENSOR_NPRM] */,
                       float* act_fault_dev /* [nenv, ODK_ACT_NPRM] */, void* stream);

/* Command curriculum: training on commands drawn from a grid over (lin_vel_x, lin_vel_y, ang_vel_yaw) whose bins open as the policy learns
 * to track inside their neighbours.  Two launches: odk_curriculum_step after every odk_step of a rollout (judges the stint that ends, draws
 * the next command into the BOUND command buffer), odk_curriculum_update once per training iteration (promotes bins, rebuilds the cdf).
 * Not reports: they sit next to the fault stages.  The step, reset and physics kernels are not involved.
 *
 * The grid: axis a (0 vx, 1 vy, 2 wz) has n[a] equal bins between lo[a] and hi[a], 1 <= n[a] <= ODK_CURR_MAX_AXIS, and
 * nbins = n[0] n[1] n[2] <= ODK_CURR_MAX_BINS; bin (ix, iy, iz) has index (ix n[1] + iy) n[2] + iz.  width[a] = (hi[a] - lo[a]) / n[a] is
 * computed by the caller (the device does not divide floats).
 *
 * Device arrays (the caller's; int32 so that neither the order of the atomics nor that of the scan can change a bit):
 *   levels  int32 [nbins]      0 .. ODK_CURR_LMAX; a bin is drawn in proportion to its level
 *   cdf     int32 [nbins]      inclusive prefix sums of levels
 *   counts  int32 [nbins][2]   tries and successes since the bin was last judged
 *   stats   int32 [4]          ODK_CURR_STAT_*: updates, bins judged, bins promoted, tries judged (running totals)
 *   state   float [nenv, ODK_CURR_NSTATE]  per env (whole numbers are exact to 2^24): HEAD calls since the row was zeroed, EPISODE, STINT the
 *           draws of this episode, STEP the steps of the stint, BIN the drawn bin (-1: the zero command), SAMPLES, SQLIN, SQYAW
 *   the command buffer  float [nenv, 7]  the one bound with odk_batch_bind_commands, row stride 7
 *
 * odk_curriculum_step, env e (one thread per env, no LDS, no scratch, graph-capturable; every load of env e's state row, command row and
 * velocities comes before its first store; float32 + - * with every product rounded before it is added):
 *   first = HEAD == 0: draw only.  Otherwise, with d = done_dev[e] (0 when done_dev is NULL) and tr = truncation_dev[e] (likewise):
 *   1. a velocity sample when d == 0 and STEP >= skip (a done step's observation is the next episode's): SAMPLES += 1,
 *      SQLIN += (vx - cx)^2 + (vy - cy)^2, SQYAW += (wz - cwz)^2, with (vx, vy) = priv[nobs + 9 .. 10] (the local linear velocity),
 *      wz = priv[nobs + 2] (the gyro) of the noise-free privileged tail and c env e's row of the command buffer: odk_tracking_accumulate's;
 *   2. STEP += 1; the stint ends when d != 0 or STEP == period;
 *   3. an ending stint with BIN >= 0 is judged: a fall (d != 0 and tr == 0) is a try and no success; otherwise, with SAMPLES >= min_samples,
 *      a try, and a success when SQLIN <= (tol_lin tol_lin) SAMPLES and SQYAW <= (tol_yaw tol_yaw) SAMPLES; otherwise it is not counted.
 *      A try is atomicAdd(counts[BIN][0], 1), a success atomicAdd(counts[BIN][1], 1);
 *   4. a draw on a stint end and on the first call: EPISODE += 1 and STINT = 0 on the first call or d != 0; with
 *      u_k = odk_action_apply's stateless draw of (seed, env_id_offset + e, EPISODE, STINT, stream 128 + k), total = cdf[nbins - 1]:
 *        k = 0     the zero command when u < p_zero or total == 0: all seven entries 0, BIN = -1;
 *        k = 1     t = min((int)(u (float)total), total - 1); BIN = the first bin with cdf[bin] > t (binary search);
 *        k = 2..4  entry a = fminf(lo[a] + width[a] ((float)i_a + u), hi[a]);
 *        k = 5..8  entry 3 + j = head_lo[j] + (head_hi[j] - head_lo[j]) u  (the batch config's cmd_range rows 3..6);
 *      then STINT += 1, STEP = SAMPLES = SQLIN = SQYAW = 0;
 *   5. HEAD += 1.  A drawn row is stored into the command buffer and into floats 6..12 of env e's row of obs_dev and of priv_patch_dev
 *      (each may be NULL: not patched) -- what a bound step shows in those slots.  BUILD-DEFINED: the reference's mid-episode resample shows
 *      the old command for one more step; here the policy's first action of a stint sees the command the next step's reward is judged by.
 * Refused (ODK_ERR_INVALID, nothing launched): a null batch, curriculum, priv_dev, cdf_dev, counts_dev, state_dev or cmd_dev (by name);
 * truncation_dev NULL while done_dev is not; a cmd_dev that is not the bound buffer (or a bound stride other than 7); n[a] or nbins out of
 * range; period < 1, min_samples < 0 or skip < 0; any two of counts, state, cmd, obs, priv_patch overlapping, or one of them overlapping cdf.
 *
 * odk_curriculum_update (one workgroup of one wave; lane l walks bins l, 64 + l, ...): a bin is JUDGED when its tries >= min_tries and
 * PROMOTED when also (float)successes >= promote_rate (float)tries.  level' = min(ODK_CURR_LMAX, level + P), P the number of promoted bins
 * among the bin itself and its up to six neighbours one step along an axis (no wrap): gathered, not scattered.  Every new level is parked
 * in cdf before any counter is zeroed or any level stored; then a judged bin's two counters go back to 0 (the others keep theirs), levels
 * takes the new levels, cdf their inclusive prefix sums (a lane scan, no LDS), and stats advances by 1, the judged bins, the promoted bins
 * and the judged bins' tries.  Refused: null pointers (by name), the grid out of range, min_tries < 1, two of the four arrays overlapping. */
#define ODK_CURR_LMAX 5
#define ODK_CURR_MAX_AXIS 16
#define ODK_CURR_MAX_BINS 4096
#define ODK_CURR_NSTATE 8
enum { ODK_CURR_HEAD = 0, ODK_CURR_EPISODE = 1, ODK_CURR_STINT = 2, ODK_CURR_STEP = 3, ODK_CURR_BIN = 4, ODK_CURR_SAMPLES = 5,
       ODK_CURR_SQLIN = 6, ODK_CURR_SQYAW = 7 };
enum { ODK_CURR_STAT_UPDATES = 0, ODK_CURR_STAT_JUDGED = 1, ODK_CURR_STAT_PROMOTED = 2, ODK_CURR_STAT_TRIES = 3 };
typedef struct {
  float lo[3], hi[3];               /* the grid's ends per axis: vx, vy, wz */
  int32_t n[3];                     /* bins per axis, 1 .. ODK_CURR_MAX_AXIS */
  float width[3];                   /* (hi - lo) / n, computed by the caller */
  float head_lo[4], head_hi[4];     /* cmd_range rows 3..6 */
  float p_zero;                     /* share of all-zero commands */
  int32_t period, skip, min_samples;/* steps per stint; steps of a stint before the first sample; samples a judged stint needs */
  float tol_lin, tol_yaw;           /* RMS tolerances of a success: m/s (planar), rad/s */
  int32_t min_tries;                /* tries that make a bin judged */
  float promote_rate;               /* success share that promotes */
  uint32_t seed, env_id_offset;
} odk_curriculum;
int odk_curriculum_step(const odk_batch* b, const odk_curriculum* c, const float* priv_dev /* [nenv, npriv], read */,
                        const float* done_dev /* may be NULL */, const float* truncation_dev /* may be NULL with done_dev */,
                        const int32_t* cdf_dev, int32_t* counts_dev, float* state_dev, float* cmd_dev /* the bound buffer */,
                        float* obs_dev /* [nenv, nobs] or NULL */, float* priv_patch_dev /* [nenv, npriv] or NULL */, void* stream);
int odk_curriculum_update(const odk_batch* b, const odk_curriculum* c, int32_t* levels_dev, int32_t* cdf_dev, int32_t* counts_dev,
                          int32_t* stats_dev, void* stream);

/* Log replay (which plant is the real robot: the actions of a recorded observation log -- mujoco_infer.py's mujoco_saved_obs.pkl, or the
 * robot runtime's -- are replayed through a batch whose envs are candidate plants, and each env's joints are scored against what the log's
 * encoders recorded).  Two launches beside the step kernel, both one 16-lane row per env (lane = actuator, four envs per wave), no LDS, no
 * scratch, graph-capturable, every product rounded before it is added: a float32 host restatement has their bits.  They know one table
 * layout and no task.
 *
 * The table log_dev [nrow, ODK_LOG_ROW(nu)] (the caller's device floats; the host cannot see them, their contents are the caller's to
 * validate).  Row k is what the log shows after control step k, all of it taken from the log's observation row k + 1:
 *   ODK_LOG_COMMAND [7]   the command
 *   ODK_LOG_ACTION [nu]   last_act: the action a_k that step k applies (row k of the log was saved before the policy computed a_k)
 *   log_pos(nu) [nu]      joint position minus default, radians
 *   log_vel(nu) [nu]      joint velocity AS THE OBSERVATION HOLDS IT (rad/s times dof_vel_scale): the logged float32 itself.  BUILD-DEFINED:
 *                         dividing it by dof_vel_scale = 0.05 on the host is not invertible in float32 (x 0.05 maps five neighbouring
 *                         floats onto four), so a plant replayed on its own log would not score 0; the kernel multiplies instead
 *   log_gyro(nu) [3], log_accel(nu) [3], log_contact(nu) [2]
 * with log_pos(nu) = 7 + nu, log_vel = 7 + 2 nu, log_gyro = 7 + 3 nu, log_accel = 10 + 3 nu, log_contact = 13 + 3 nu.
 *
 * odk_log_apply: issued BEFORE odk_step.  The tracking accumulator is the clock, exactly as odk_command_schedule_apply reads it: t = STEPS
 * of env e (STEPS - 1 once ENDED is set), k = min(max(t, 0), nrow - 1).  Lane u < nu stores action_dev[e][u] = row k's action u, lanes
 * 0..6 store entries 0..6 of env e's row of the BOUND command buffer from row k's command.  A pure function of its inputs.
 * ODK_ERR_INVALID, nothing launched: a null pointer (by name), no bound commands, nrow < 1, a model with more than 16 actuators.
 *
 * odk_replay_accumulate: issued after odk_step and BEFORE odk_tracking_accumulate (odk_push_accumulate's ENDED / STEPS contract: STEPS is
 * the index k of the step that just ran).  A sample is odk_gait_accumulate's (first episode, not done) with k < nrow; an env whose first
 * episode has ended or whose clock has passed the end of the table keeps every bit of its row.  acc_dev [nenv, 16, ODK_REPLAY_NSLOT],
 * zeroed by the caller: lane u owns the slots of [e][u].  With Q the noise-free privileged tail of priv_dev (float nobs onwards) and L
 * row k of the table, per sample:
 *   lane u < nu   dp = Q[15 + u] - L[log_pos + u];  POS_ERR_SUM += dp;  POS_ERR_SQ += dp dp;  POS_ERR_PEAK = max(POS_ERR_PEAK, |dp|);
 *                 dv = Q[15 + nu + u] dof_vel_scale - L[log_vel + u]  (the batch config's dof_vel_scale);  VEL_ERR_SQ += dv dv
 *   lane u < 3    GYRO_ERR_SQ += (Q[u] - L[log_gyro + u])^2;  ACCEL_ERR_SQ += (Q[3 + u] - L[log_accel + u])^2
 *   lane u < 2    CONTACT_AGREE += 1 when (Q[16 + 3 nu + u] != 0) == (L[log_contact + u] > 0.5)
 *   lane 0        SAMPLES += 1
 * ODK_ERR_INVALID, nothing launched: a null pointer (by name), nrow < 1, a model with more than 16 actuators. */
#define ODK_LOG_ROW(nu) (15 + 3 * (nu))
#define ODK_REPLAY_NSLOT 8
enum { ODK_LOG_COMMAND = 0, ODK_LOG_ACTION = 7 };
enum { ODK_REPLAY_POS_ERR_SUM = 0, ODK_REPLAY_POS_ERR_SQ = 1, ODK_REPLAY_VEL_ERR_SQ = 2, ODK_REPLAY_POS_ERR_PEAK = 3, ODK_REPLAY_GYRO_ERR_SQ = 4,
       ODK_REPLAY_ACCEL_ERR_SQ = 5, ODK_REPLAY_CONTACT_AGREE = 6, ODK_REPLAY_SAMPLES = 7 };
int odk_log_apply(const odk_batch* b, const float* log_dev, int nrow, const float* track_acc_dev, float* action_dev /* [nenv, nu] out */,
                  void* stream);
int odk_replay_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                          const float* track_acc_dev, const float* log_dev, int nrow, float* acc_dev /* [nenv, 16, ODK_REPLAY_NSLOT] */,
                          void* stream);

/* mjx_env.step alone (physics only, n_substeps, ctrl = ctrl_dev [nenv, nu]); for parity tests */
int odk_physics_step(odk_batch* b, const float* ctrl_dev, int n_substeps, void* stream);

/* state access (host pointers, synchronous): qpos [nenv,nq], qvel [nenv,nv], qacc_warmstart [nenv,nv] */
int odk_batch_get_state(odk_batch* b, float* qpos, float* qvel, float* warm);
int odk_batch_set_state(odk_batch* b, const float* qpos, const float* qvel, const float* warm);
/* debug read-back of the last forward pass of every env: sensordata [nenv,46], actuator_force [nenv,14],
 * contact_dist [nenv,12], qacc [nenv,nv]  (any may be NULL) */
int odk_batch_get_debug(odk_batch* b, float* sensordata, float* actuator_force, float* contact_dist, float* qacc);
/* debug: LDS image (floats) of every env's last forward pass, taken at reset / physics_step and, when
 * odk_set_debug_dump(1), at step; odk_lds_offset names the arrays inside it (csrc/odk_shape.h Shape) */
void odk_set_debug_dump(int on);
int odk_batch_lds_size(const odk_batch* b);
int odk_batch_get_lds(odk_batch* b, float* host_image);
int odk_lds_offset(const odk_batch* b, const char* name);
/* lanes per env the batch's kernels really run (odk_env_config.lanes_per_env is a hint: elliptic cones, height-field floors and robots that are
 * not the duck exist at 32 lanes per env only) */
int odk_batch_lanes(const odk_batch* b);
/* raw per-env info record (floats, layout in csrc/odk_shapes.h) for tests */
int odk_batch_record_size(const odk_batch* b);
int odk_batch_get_records(odk_batch* b, float* host_records);
/* writes the records back (synchronous): restores a saved batch, or presets carried `info` fields -- e.g. info["step"] = 500 so
 * that the next step resamples the command (joystick.py:456-466) */
int odk_batch_set_records(odk_batch* b, const float* host_records);
/* where a field of the carried state lives inside a record: names are the keys of the reference's `info` dict (joystick.py:278-302:
 * "rng", "step", "command", "last_act", "last_last_act", "last_last_last_act", "motor_targets", "feet_air_time", "last_contact",
 * "swing_peak", "push", "push_step", "push_interval_steps", "action_history", "imu_history", "imitation_i"), the wrapper's additions
 * ("steps", "truncation", "episode_done", "episode_metrics/sum_reward", "episode_metrics/length", "episode_metrics/reward_terms")
 * and the physics state ("qpos", "qvel", "qacc_warmstart").  *offset / *count in 4-byte words from the start of the record;
 * *kind = 0 float32, 1 int32 / uint32, 2 bit mask in one int32 (last_contact: bit f = foot f).  `current_reference_motion` and
 * `imitation_phase` are functions of imitation_i and the command and are not carried.  Returns ODK_ERR_INVALID for an unknown name. */
int odk_record_field(const odk_batch* b, const char* name, int* offset, int* count, int* kind);

/* ---- learner-side kernels (csrc/odk_learner.hip): the element-wise halves of one PPO minibatch step.  The
 * reference reaches them through brax ppo.train (common/runner.py:104-118): ppo.losses.compute_gae /
 * compute_ppo_loss and optax.chain(clip_by_global_norm, adam).  All stream-ordered, graph-capturable. ---- */

/* GAE over row-major [B, T] device arrays: vs and advantages out; truncation / termination are flags (0 = clear, any
 * other value = set);
 * bootstrap is [B].  adv_stats (may be NULL) receives {mean, 1/(std+1e-8)} of the advantages (ddof 0). */
int odk_gae(const float* truncation_dev, const float* termination_dev, const float* rewards_dev, const float* values_dev,
            const float* bootstrap_dev, float* vs_dev, float* adv_dev, float* adv_stats_dev, int B, int T, float lambda_,
            float discount, void* stream);

/* PPO loss head, forward and backward in one launch.  logits [n, 2*action_size] = (loc | raw scale) of the
 * tanh-normal policy, noise [n, action_size] ~ N(0,1) for the sampled entropy term, adv_stats from odk_gae (NULL:
 * no advantage normalisation).  Writes grad_scale * dLoss/dlogits and grad_scale * dLoss/dbaseline, and ADDS
 * (total, policy, value, entropy) loss to losses[0..3]: the caller zeroes them, per step or -- for the mean over an
 * epoch of steps -- once per epoch. */
int odk_ppo_head(const float* logits_dev, const float* raw_action_dev, const float* old_log_prob_dev, const float* adv_dev,
                 const float* adv_stats_dev, const float* vs_dev, const float* baseline_dev, const float* noise_dev,
                 float* dlogits_dev, float* dbaseline_dev, float* losses_dev, int n, int action_size, float clipping_epsilon,
                 float entropy_cost, float grad_scale, void* stream);

/* clip_by_global_norm(max_grad_norm; <= 0 disables) + Adam on flat buffers of n floats.  acc_dev[ODK_ADAM_ACC_FLOATS]
 * is scratch owned by the caller: acc[0] = squared gradient norm of this call, acc[1] = step count (zero it once),
 * acc[2..] = per-block partial sums (the norm is reduced in a fixed order: data-parallel replicas stay bit-identical). */
/* Rollout sampling of the tanh-normal policy (brax NormalTanhDistribution, as odk_ppo_head): logits [n, 2A] = (loc | raw_scale),
 * noise [n, A] standard normal (zeros: the mode).  raw_action = loc + (softplus(raw_scale) + 0.001) noise, action = tanh(raw_action),
 * log_prob[n] = log density of the action.  One launch instead of ~15 element-wise ones per rollout step. */
int odk_policy_sample(const float* logits_dev, const float* noise_dev, float* raw_action_dev, float* action_dev, float* log_prob_dev, int n,
                      int action_size, void* stream);

#define ODK_ADAM_MAX_PARTIALS 1024
#define ODK_ADAM_ACC_FLOATS (2 + ODK_ADAM_MAX_PARTIALS)
int odk_adam_clip(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, float* acc_dev, long long n, float lr,
                  float b1, float b2, float eps, float max_grad_norm, void* stream);

/* dz = dh * silu'(z) over row-major [n, w] and colsum[c] = sum_r dz[r, c] (the bias gradient of the layer below), fixed
 * summation order.  partial_dev: scratch of ceil(n / 64) * w floats.  colsum_dev may be NULL: the per-tile partial sums
 * then stay in partial_dev for odk_colsum_finalize. */
int odk_silu_bwd_colsum(const float* dh_dev, const float* z_dev, float* dz_dev, float* colsum_dev, float* partial_dev, int n, int w,
                        void* stream);

/* partial[tile, c] = sum of x[r, c] over the 64 rows of the tile (x row-major [n, w]): the first half of a column sum whose
 * second half is odk_colsum_finalize. */
int odk_colsum_partial(const float* x_dev, float* partial_dev, int n, int w, void* stream);

/* colsum[f][c] = sum over the ceil(n / 64) tile rows of partial[f][tile, c] for up to 8 layers in ONE launch (same fixed
 * order as odk_silu_bwd_colsum's own fold).  partial_dev / colsum_dev / widths are HOST arrays. */
int odk_colsum_finalize(const float* const* partial_dev, float* const* colsum_dev, const int* widths, int count, int n, void* stream);

/* Weight gradients of up to 8 dense layers in one launch on the f32 matrix cores (v_mfma_f32_32x32x2_f32):
 *   out[out_off[l] + i * n_in[l] + j] = sum over the nrows[l] minibatch rows s of dz[l](s, i) * h[l](s, j)      (= dz^T h, torch Linear weight layout)
 * dz[l] / h[l] are in the QUAD-ROW layout the fused network kernels write: [nrows / 4][width][4], element (s, f) at
 * ((s / 4) * width + f) * 4 + s % 4 (16-byte aligned; nrows[l] a multiple of 8 and >= 16 * kslices; rows past the batch hold zeros
 * in at least one of the two operands).  out_dev is the flat gradient buffer.  The rows are split into kslices slices (a
 * multiple of 8); ws_dev is a workspace of kslices * ws_stride floats laid out like out_dev (ws_stride >= every out_off +
 * n_out * n_in, a multiple of 4; every out_off and n_out * n_in a multiple of 4; ws_dev and out_dev 16-byte aligned); the slices
 * are folded in a fixed order, so the result is bit-reproducible.  dz_dev / h_dev / n_out / n_in / out_off / nrows are HOST arrays. */
/* Optional extra work of odk_dw_gemm's slice-fold launch (the launch that finishes the gradient): the bias gradients
 * bias_grad[f][c] = sum over the nblk[f] tile rows of bias_partial[f][tile, c] (what odk_colsum_fold does), and -- when
 * sq_partials_dev is not NULL -- per-block partial sums of the squared norm of everything the launch wrote (all weight and bias
 * gradients), for odk_adam_clip_packed(norm_blocks = nblocks): sq_partials_dev[0 .. nblocks), nblocks <= ODK_ADAM_MAX_PARTIALS is
 * returned in the struct; step_counter_dev (may be NULL) is incremented by 1.  Host struct; the pointers inside are device pointers. */
typedef struct odk_grad_finish {
  const float* bias_partial[8];
  float* bias_grad[8];
  int width[8], nblk[8];
  int nbias;
  float* sq_partials_dev;
  float* step_counter_dev;
  int nblocks;               /* out */
} odk_grad_finish;
int odk_dw_gemm(const float* const* dz_dev, const float* const* h_dev, const int* n_out, const int* n_in, const long long* out_off, int nlayers,
                const int* nrows, int kslices, float* ws_dev, long long ws_stride, float* out_dev, odk_grad_finish* finish /* may be NULL */,
                void* stream);

/* ---- fused policy / value networks (csrc/odk_mlp.hip): a swish MLP  n_in -> 512 -> 256 -> 128 -> n_out  (brax ppo.networks as
 * configured by the reference, common/runner.py:86-118) forward in ONE launch and its backward-data chain in ONE launch, on the
 * f32 matrix cores; a workgroup keeps a tile of 16 samples in LDS for all layers.  One or two networks per launch (policy and
 * value side by side).  Everything row-major float32 on the device.
 * The kernels read the weights from PACKED copies (16-byte pieces of four consecutive reduction indices per column):
 *   forward copy of W [n_out, n_in]:  [pad16(n_in) / 4][n_out][4],  element (o, i) at ((i / 4) * n_out + o) * 4 + i % 4
 *   backward copy:                    [pad16(n_out) / 4][n_in][4],  element (o, i) at ((o / 4) * n_in + i) * 4 + o % 4
 * with pad16(k) = k rounded up to a multiple of 16 and the padding zero (the caller zeroes the buffers once; odk_pack_weights /
 * odk_adam_clip_packed write the weights' elements only). */
#define ODK_MLP_H1 512
#define ODK_MLP_H2 256
#define ODK_MLP_H3 128
#define ODK_MLP_MAX_IN 224
#define ODK_MLP_TILE 16        /* samples per workgroup */
typedef struct odk_mlp_desc {
  const float* x;            /* [n, n_in] network input */
  const float* in_mean;      /* forward, optional (both or none): the input is normalised on load, x <- (x - in_mean) / in_std, per column */
  const float* in_std;
  const float* wf[4];        /* forward-packed weights of the four layers (16-byte aligned) */
  const float* wb[4];        /* backward-packed weights (wb[0] is not read: the input's gradient is never formed) */
  const float* b[4];         /* biases */
  /* training buffers, all in the QUAD-ROW layout [np / 4][width][4] with np = n rounded up to a multiple of ODK_MLP_TILE = 16 (the kernels work on 16-sample tiles and write ceil(n / 16) tile rows of
   * bias_partial; element (s, f) at
   * ((s / 4) * width + f) * 4 + s % 4; the operand layout of odk_dw_gemm); rows n .. np - 1 are written as zeros in h / g / dz / doutp */
  float* xp;                 /* forward out: quad-row copy of x, width n_in (rows past n: copies of row n - 1) */
  float* h[3];               /* forward out: swish(z_l), width H_l; all of xp / h / g NULL: inference only, nothing but `out` is written */
  float* g[3];               /* forward out / backward in: swish'(z_l) */
  float* out;                /* forward out: [n, n_out] row-major */
  const float* dout;         /* backward in: dLoss/dout [n, n_out] row-major */
  float* doutp;              /* backward out: quad-row copy of dout, width n_out */
  float* dz[3];              /* backward out: dLoss/dz_l, width H_l */
  float* bias_partial[4];    /* backward out: per-tile column sums of dz_l (l = 3: of dout), [ceil(n / 16), width_l]; odk_colsum_fold finishes them */
  int n, n_in, n_out;        /* n_in <= ODK_MLP_MAX_IN, n_out <= 32 */
  /* Optional row sources of the forward pass (row_idx NULL: row r of the input is x[r], as above) -- the minibatch gather of brax's
   * sgd_step (jnp.take of the shuffled trajectories; reference common/runner.py:104-118 -> brax ppo.train) folded into the load, so that
   * no gathered copy of the observations is ever written:
   *   rows r <  n_main:  x[row_idx[k B + r / traj_len] * traj_len + r % traj_len]     x = the WHOLE rollout, [n_traj * traj_len, n_in]
   *   rows r >= n_main:  x_tail[row_idx[k B + r - n_main]]                              x_tail = [n_traj, n_in] (the bootstrap observations)
   * with B = n_main / traj_len trajectories per minibatch and k = *cursor (device int: which minibatch of the schedule row_idx holds;
   * NULL: 0).  An index outside [0, n_traj) is never dereferenced: that row reads as NaN and the step's losses say so. */
  const long long* row_idx;
  const int* cursor;
  const float* x_tail;
  int traj_len, n_main, n_traj;
} odk_mlp_desc;
int odk_mlp_forward(const odk_mlp_desc* nets, int count, void* stream);
int odk_mlp_backward(const odk_mlp_desc* nets, int count, void* stream);
/* tools: device buffer of 4 x 1024 int64 receiving, per single-wave workgroup of odk_dw_gemm's matrix launch, its start / end on the
 * 100 MHz wall clock and the HW_ID / XCC_ID registers (where it ran); NULL: off */
void odk_dw_set_profile(long long* dev);
/* tools: device buffer of 32 int64 receiving the forward kernel's phase timestamps (shader clock, workgroup 0); NULL: off */
void odk_mlp_set_profile(long long* stamps_dev);
/* tools: device buffer of 4 x (workgroups of a network launch) int64 receiving every workgroup's start / end on the 100 MHz wall
 * clock, HW_ID | XCC_ID << 32 and its shader-clock cycles (forward and backward launches alike); NULL: off */
void odk_mlp_set_wg_profile(long long* dev);
/* Where up to 8 weight matrices sit in a flat parameter buffer (float offset `off`, torch layout [rows = n_out, cols = n_in]) and
 * in the packed buffers (float offsets, multiples of 4; bwd_off < 0: no backward copy of that weight). */
typedef struct odk_weight_table {
  int count;
  long long off[8];
  int rows[8], cols[8];
  long long fwd_off[8], bwd_off[8];
} odk_weight_table;
/* (re)builds the packed copies from the parameters */
int odk_pack_weights(const float* params_dev, long long n, float* fwd_packed_dev, long long n_fwd, float* bwd_packed_dev, long long n_bwd,
                     const odk_weight_table* table, void* stream);
/* odk_adam_clip that also keeps the packed copies current (every updated weight is written to all of its places).
 * norm_blocks > 0: acc[2 .. 2 + norm_blocks) already hold the partial sums of the squared gradient norm and acc[1] the advanced step
 * count (odk_dw_gemm with an odk_grad_finish whose sq_partials_dev = acc + 2, step_counter_dev = acc + 1): no norm launch of its own. */
int odk_adam_clip_packed(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, float* acc_dev, long long n, float lr, float b1,
                         float b2, float eps, float max_grad_norm, float* fwd_packed_dev, long long n_fwd, float* bwd_packed_dev, long long n_bwd,
                         const odk_weight_table* table, int norm_blocks, void* stream);
/* The same launch with the END-OF-STEP duties of an indexed minibatch step folded in (all optional, NULL / 0 = off), so that a step is
 * six launches and nothing else:
 *   cursor_dev:        *cursor_dev += 1 -- the next step's launches read the next minibatch of the schedule (odk_mlp_desc.cursor,
 *                      odk_ppo_gae_head) without any host-side call between two graph replays;
 *   loss_partials_dev: [n_loss_partials][4] per-workgroup sums of (total, policy, value, entropy) left by odk_ppo_gae_head, folded in
 *                      workgroup order into losses_dev[0..3] += ... (a fixed order; as float atomics the 4 x 320 additions on four
 *                      addresses cost the head launch ~4 us of serialisation). */
typedef struct odk_step_tail {
  int* cursor_dev;
  const float* loss_partials_dev;
  int n_loss_partials;
  float* losses_dev;
} odk_step_tail;
int odk_adam_clip_packed_tail(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, float* acc_dev, long long n, float lr, float b1,
                              float b2, float eps, float max_grad_norm, float* fwd_packed_dev, long long n_fwd, float* bwd_packed_dev, long long n_bwd,
                              const odk_weight_table* table, int norm_blocks, const odk_step_tail* tail /* may be NULL */, void* stream);

/* GAE + advantage statistics + the PPO loss head in ONE launch, reading the rollout through the minibatch's trajectory indices (what
 * odk_gather_rows + odk_gae + odk_ppo_head do as three launches on gathered copies; same arithmetic, same summation orders; brax
 * ppo.losses.compute_gae / compute_ppo_loss).  Every workgroup recomputes the B x T recursion in LDS (B * T <= 5120, B <= 1024) -- the
 * advantage statistics are a global quantity and a launch boundary costs more than 80 redundant copies of a 100 KFLOP scan -- then
 * works its own 64 samples.  Host struct; every pointer inside is a device pointer.
 *   sample s = b T + t of minibatch k = *cursor (NULL: 0) is step t of trajectory j = row_idx[k B + b] of the rollout;
 *   logits [n, 2A], values [n + B] (baselines, then the B bootstrap values), n = B T: the network outputs of THIS minibatch;
 *   raw_action [n_traj, T, A], old_log_prob / reward / termination / truncation [n_traj, T]: the whole rollout;
 *   noise: the entropy sample of minibatch k is noise[k n A ..];  dlogits [n, 2A], dvalues [n] out;
 *   losses: loss_partials != NULL: workgroup w writes its sums of (total, policy, value, entropy) to loss_partials[4 w ..] (ODK_GAE_HEAD_SAMPLES
 *   samples per workgroup: ceil(n / ODK_GAE_HEAD_SAMPLES) entries; odk_adam_clip_packed_tail folds them); otherwise losses[4] += ... by atomics;
 *   adv_out / vs_out [n], stats_out[2] (mean, 1 / (std + 1e-8)): optional outputs (written by workgroup 0), may be NULL. */
#define ODK_GAE_HEAD_SAMPLES 32
typedef struct odk_gae_head_args {
  const float *logits, *values, *raw_action, *old_log_prob, *reward, *termination, *truncation, *noise;
  const long long* row_idx;
  const int* cursor;
  float *dlogits, *dvalues, *losses, *loss_partials, *adv_out, *vs_out, *stats_out;
  int B, T, action_size, n_traj, normalize_advantage;
  float gae_lambda, discount, clipping_epsilon, entropy_cost, grad_scale;
} odk_gae_head_args;
int odk_ppo_gae_head(const odk_gae_head_args* args, void* stream);

/* Column moments of a row-major float32 matrix x [rows, w] in ONE pass, accumulated in float64: partial_dev [slices][2][w] doubles receives, per row
 * slice, the column sums and the column sums of squares (slice s takes rows s, s + slices, ...; fixed order inside a slice); the caller folds the
 * slices (any fixed-order sum: they are few).  The observation normaliser's batch statistics (brax running_statistics.update as reached through
 * reference common/runner.py:104-118: normalize_observations=True) without a float64 copy of the 10^7-element rollout.  slices <= 1024. */
int odk_col_moments(const float* x_dev, long long rows, int w, int slices, double* partial_dev, void* stream);
/* brax running_statistics.update on those moments, one launch: folds the slices of partial_dev (in slice order) into the batch's column sums s
 * and sums of squares s2 over `rows` rows, then, in float64,
 *   count' = count + rows;  mean' = mean + (s / rows - mean) rows / count';  summed_variance' = summed_variance + (s2 - s (mean + mean') + rows mean mean');
 *   std = clamp(sqrt(max(summed_variance' / count', 0)), std_min, std_max)
 * count_dev: one double; mean / summed_variance / std: float32 [w], updated in place. */
int odk_moments_update(const double* partial_dev, int slices, int w, long long rows, double* count_dev, float* mean_dev, float* summed_variance_dev,
                       float* std_dev, float std_min, float std_max, void* stream);

/* colsum[f][c] = sum over the nblk[f] tile rows of partial[f][tile, c] for up to 8 layers in one launch (fixed order);
 * partial_dev / colsum_dev / widths / nblk are HOST arrays */
int odk_colsum_fold(const float* const* partial_dev, float* const* colsum_dev, const int* widths, const int* nblk, int count, void* stream);

/* dst[f][b, :] = src[f][idx[b], :] for up to 10 row-major float fields in one launch (minibatch gather of the rollout).
 * src_dev / dst_dev / row_floats are HOST arrays of device pointers / row lengths; idx_dev is int64 on the device, nrows
 * entries; every indexed source has src_rows rows.  An index outside [0, src_rows) is never dereferenced: its destination
 * rows are filled with NaN.  direct_base (HOST array, may be NULL): direct_base[f] >= 0 makes field f a plain block copy,
 * dst[f][b, :] = src[f][direct_base[f] + b, :] (no index; e.g. this step's slice of a noise pool) -- the caller guarantees
 * the range.  Buffers of fields whose row length is a multiple of 4 must be 16-byte aligned. */
int odk_gather_rows(const float* const* src_dev, float* const* dst_dev, const int* row_floats, const long long* direct_base, int nfields,
                    const long long* idx_dev, int nrows, long long src_rows, void* stream);

/* live timing of odk_step launches with HIP events on the launch stream: returns the average milliseconds per TIMED launch since
 * the last call (and resets the window).  enable: 0 = off, n > 0 = an event pair around every n-th launch from now on (the pair costs
 * the stream ~7 us of serialisation per timed launch: 1.2 % of an 8192-env step when every launch is timed) */
int odk_batch_timing(odk_batch* b, int enable, float* avg_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif

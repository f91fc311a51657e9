// odk_engine.hip -- the batch C-ABI of include/odk.h (libodk.so): create / destroy / configure, the binders and setters that own batch state,
// reset / step / physics step and launch(), the state / record / debug getters and the step timing.  The evaluation reports' kernels and
// entry points (odk_*_accumulate, odk_command_schedule_apply) are odk_reports.hip; both see the batch through odk_batch.h.
//
// Host side: device buffers, launches on the caller's stream (blob -> DevModel, odk_model_load and the model getters: odk_model_load.hip).  Device side:
// the reset / step / physics-only kernels live in odk_env_kernels.h and are compiled one object per kernel set (odk_env_unit.hip); this file
// sees launch_sg's declaration (odk_shapes.h) and chooses the instantiation in launch().  gfx950 only; no CPU fallback of any kind.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/odk.h"
#include "odk_batch.h"
#include "odk_shapes.h"

using namespace odk;

// (the thread's error string, fail() and the whole model side -- blob parsing, table builders, odk_model_load, the odk_model_* getters -- live in
// the host-only odk_model_load.hip)

extern "C" void odk_default_config(odk_env_config* c) {
  memset(c, 0, sizeof(*c));
  c->ctrl_dt = 0.02f; c->action_scale = 0.25f; c->dof_vel_scale = 0.05f; c->max_motor_velocity = 5.24f;
  c->noise_level = 1.0f; c->noise_gyro = 0.1f; c->noise_accelerometer = 0.05f; c->noise_gravity = 0.1f; c->noise_joint_vel = 2.5f;
  const float s10[10] = {0.03f, 0.03f, 0.03f, 0.05f, 0.08f, 0.03f, 0.03f, 0.03f, 0.05f, 0.08f};  // BUG-COMPAT joystick.py:184-200
  for (int i = 0; i < 10; i++) c->qpos_noise_scale[i] = s10[i];
  const float rs[7] = {2.5f, 6.0f, -1.0e-3f, -0.5f, -0.2f, 20.0f, 1.0f};
  memcpy(c->reward_scales, rs, sizeof(rs));
  c->tracking_sigma = 0.01f;
  c->push_enable = 1.0f; c->push_interval_range[0] = 5.0f; c->push_interval_range[1] = 10.0f;
  c->push_magnitude_range[0] = 0.1f; c->push_magnitude_range[1] = 1.0f;
  const float cr[7][2] = {{-0.15f, 0.15f}, {-0.2f, 0.2f}, {-1.0f, 1.0f}, {-0.34f, 1.1f}, {-0.78f, 0.78f}, {-1.5f, 1.5f}, {-0.5f, 0.5f}};
  memcpy(c->cmd_range, cr, sizeof(cr));
  c->use_imitation = 1; c->use_motor_speed_limits = 1; c->autoreset = 1; c->episode_length = 1000; c->n_substeps = 10; c->lanes_per_env = 0;
  c->env_kind = ODK_ENV_JOYSTICK; c->reset_base_qvel = 0.05f; c->hfield_up_normals_only = 0;
}
extern "C" void odk_default_config_standing(odk_env_config* c) {   // reference standing.py:44-100
  odk_default_config(c);
  c->env_kind = ODK_ENV_STANDING; c->reset_base_qvel = 0.5f; c->hfield_up_normals_only = 0;
  c->max_motor_velocity = 0.0f;   // standing.py has no speed limit (and no such config key)
  c->noise_gyro = 0.05f; c->noise_accelerometer = 0.005f;
  const float rs[7] = {-0.5f, -2.0f, -1.0e-3f, -0.375f, -0.3f, 20.0f, 0.0f};   // orientation, head_pos, torques, action_rate, stand_still, alive
  memcpy(c->reward_scales, rs, sizeof(rs));
  for (int k = 0; k < 3; k++) c->cmd_range[k][0] = c->cmd_range[k][1] = 0.0f;   // standing.py:652-654
  c->cmd_range[5][0] = -2.7f; c->cmd_range[5][1] = 2.7f;
  c->use_imitation = 0; c->use_motor_speed_limits = 0;
}
extern "C" void odk_obs_sizes(int env_kind, int* nobs, int* npriv) {
  if (nobs) *nobs = env_kind == ODK_ENV_STANDING ? ODK_NOBS_STANDING : ODK_NOBS;
  if (npriv) *npriv = env_kind == ODK_ENV_STANDING ? ODK_NPRIV_STANDING : ODK_NPRIV;
}

template <class S> static void fill_sizes(odk_batch* b) {
  b->rec_size = Rec<S>::SIZE; b->frec_size = Rec<S>::FSIZE; b->lds_total = S::TOTAL; b->dr_size = DRL<S>::SIZE; b->env_lds = EnvL<S>::TOTAL;
}

static void to_dev_cfg(const odk_env_config& c, EnvCfg& d, int nu) {
  d.ctrl_dt = c.ctrl_dt; d.action_scale = c.action_scale; d.dof_vel_scale = c.dof_vel_scale; d.max_motor_velocity = c.max_motor_velocity;
  d.noise_level = c.noise_level; d.noise_gyro = c.noise_gyro; d.noise_accelerometer = c.noise_accelerometer; d.noise_gravity = c.noise_gravity;
  d.noise_joint_vel = c.noise_joint_vel;
  memcpy(d.qpos_noise_scale, c.qpos_noise_scale, sizeof(d.qpos_noise_scale)); memcpy(d.reward_scales, c.reward_scales, sizeof(d.reward_scales));
  d.tracking_sigma = c.tracking_sigma; d.push_enable = c.push_enable;
  memcpy(d.push_interval_range, c.push_interval_range, 8); memcpy(d.push_magnitude_range, c.push_magnitude_range, 8);
  memcpy(d.cmd_range, c.cmd_range, sizeof(d.cmd_range));
  d.use_imitation = c.use_imitation; d.use_motor_speed_limits = c.use_motor_speed_limits; d.autoreset = c.autoreset;
  d.episode_length = c.episode_length; d.n_substeps = c.n_substeps;
  d.kind = c.env_kind; d.reset_base_qvel = c.reset_base_qvel;
  obs_sizes_nu(nu, c.env_kind, &d.nobs, &d.npriv);
}

extern "C" int odk_batch_create(const odk_model* m, const odk_env_config* cfg, int nenv, int device, const float* prm_table, const double* dxs, int nx,
                                const double* dys, int ny, const double* dths, int nth, const double* ranges6, int nsteps, odk_batch** out) {
  if (!m || !cfg || !out || nenv <= 0 || !prm_table || nx > 16 || ny > 16 || nth > 16) return fail(ODK_ERR_INVALID, "odk_batch_create: bad arguments");
  HIPCHK(hipSetDevice(device));
  odk_batch* b = new odk_batch();
  b->model = *m; b->nenv = nenv; b->device = device; b->cfg = *cfg;
  if (cfg->lanes_per_env != 0 && cfg->lanes_per_env != 32 && cfg->lanes_per_env != 64) { delete b; return fail(ODK_ERR_INVALID, "lanes_per_env must be 0, 32 or 64"); }
  // lanes_per_env is a geometry HINT (one env per wave finishes a small batch's step sooner): the instantiations that exist at 32 lanes per env only
  // -- elliptic cones (whatever set the model's opt_cone: the XML's <option cone> or a config switch), height-field floors, robots that are not the
  // duck -- run there whatever was asked (odk_batch_lanes reports it)
  b->G = (cfg->lanes_per_env == 64 && !m->h.cone && m->h.floor_is_plane && m->shape < 2) ? 64 : 32;
#define X(i, S) if (m->shape == i) fill_sizes<S>(b);
  ODK_SHAPES(X)
#undef X
  DevPRM hp;
  memset(&hp, 0, sizeof(hp));
  hp.nx = nx; hp.ny = ny; hp.nth = nth; hp.nsteps = nsteps;
  for (int i = 0; i < nx; i++) hp.dxs[i] = (float)dxs[i];
  for (int i = 0; i < ny; i++) hp.dys[i] = (float)dys[i];
  for (int i = 0; i < nth; i++) hp.dths[i] = (float)dths[i];
  for (int i = 0; i < 6; i++) hp.ranges[i] = (float)ranges6[i];
  size_t tbytes = (size_t)nx * ny * nth * 640 * sizeof(float);
  HIPCHK(hipMalloc(&b->d_model, sizeof(DevModel)));
  { DevModel hm = m->h; hm.hfield_filter = cfg->hfield_up_normals_only ? 3 : 0;
    HIPCHK(hipMemcpy(b->d_model, &hm, sizeof(DevModel), hipMemcpyHostToDevice)); }   // (the batch's own copy: the filter is a batch setting)
  b->h_prm = hp;
  HIPCHK(hipMalloc(&b->d_table, tbytes)); HIPCHK(hipMemcpy(b->d_table, prm_table, tbytes, hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&b->d_recs, (size_t)nenv * b->rec_size * sizeof(float))); HIPCHK(hipMemset(b->d_recs, 0, (size_t)nenv * b->rec_size * sizeof(float)));
  HIPCHK(hipMalloc(&b->d_first, (size_t)nenv * b->frec_size * sizeof(float))); HIPCHK(hipMemset(b->d_first, 0, (size_t)nenv * b->frec_size * sizeof(float)));
  HIPCHK(hipMalloc(&b->d_dbg, (size_t)nenv * b->lds_total * sizeof(float))); HIPCHK(hipMemset(b->d_dbg, 0, (size_t)nenv * b->lds_total * sizeof(float)));
  HIPCHK(hipMalloc(&b->d_xt, sizeof(XTerms))); HIPCHK(hipMemset(b->d_xt, 0, sizeof(XTerms)));
  {   // imitation joint map: the duck's (custom_rewards.py:80-88) for its two shapes, none (every actuator -1) for another robot
    int h[MAXU];
    for (int u = 0; u < MAXU; u++) h[u] = -1;
    if (m->shape < 2) for (int u = 0; u < m->h.nu; u++) h[u] = u < 5 ? u : (u >= 9 ? u + 2 : -1);
    HIPCHK(hipMalloc(&b->d_imap, sizeof(h))); HIPCHK(hipMemcpy(b->d_imap, h, sizeof(h), hipMemcpyHostToDevice));
    b->imap_set = m->shape < 2;
  }
  {   // Standing's head joints: the duck's actuators 5..8 (neck_pitch, head_pitch, head_yaw, head_roll) for its two shapes, none for another robot
    int h[MAXU];
    for (int u = 0; u < MAXU; u++) h[u] = -1;
    if (m->shape < 2) for (int k = 0; k < 4; k++) h[5 + k] = k;
    HIPCHK(hipMalloc(&b->d_hslot, sizeof(h))); HIPCHK(hipMemcpy(b->d_hslot, h, sizeof(h), hipMemcpyHostToDevice));
    b->hmap_set = m->shape < 2;
  }
  if (!m->hfield.empty()) {   // shared by all envs, L2-resident (256 KB)
    HIPCHK(hipMalloc(&b->d_hfield, m->hfield.size() * sizeof(float)));
    HIPCHK(hipMemcpy(b->d_hfield, m->hfield.data(), m->hfield.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  *out = b;
  return ODK_OK;
}
extern "C" void odk_batch_destroy(odk_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  for (void* p : {(void*)b->d_model, (void*)b->d_table, (void*)b->d_recs, (void*)b->d_first, (void*)b->d_dr, (void*)b->d_dbg, (void*)b->d_hfield, (void*)b->d_xt, (void*)b->d_imap,
                  (void*)b->d_hslot}) (void)hipFree(p);
  for (auto& ev : b->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  delete b;
}
extern "C" int odk_batch_set_config(odk_batch* b, const odk_env_config* cfg) {
  if (!b || !cfg) return fail(ODK_ERR_INVALID, "null");
  if (cfg->env_kind != b->cfg.env_kind) return fail(ODK_ERR_INVALID, "odk_batch_set_config: env_kind is fixed at creation (it sets the output strides)");
  int g = b->cfg.lanes_per_env;
  if ((cfg->hfield_up_normals_only != 0) != (b->cfg.hfield_up_normals_only != 0)) {   // lives in the batch's device model (outside any step)
    const int v = cfg->hfield_up_normals_only ? 3 : 0;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(reinterpret_cast<char*>(b->d_model) + offsetof(DevModel, hfield_filter), &v, sizeof(int), hipMemcpyHostToDevice));
  }
  b->cfg = *cfg;
  b->cfg.lanes_per_env = g;
  return ODK_OK;
}

extern "C" int odk_batch_set_param(odk_batch* b, int param, const float* v, int count) {
  if (!b || !v) return fail(ODK_ERR_INVALID, "null");
  const DevModel& m = b->model.h;
  const int nb = m.nb, nu = m.nu;
  const int MASS = 0, IPOS = nb, FRL = nb + 3, ARM = FRL + nu, Q0 = ARM + nu, KP = Q0 + nu, SIZE = KP + nu;
  if (SIZE != b->dr_size) return fail(ODK_ERR_INVALID, "dr layout");
  if (!b->dr_enabled) {  // start from the nominal model
    b->h_dr.resize((size_t)b->nenv * SIZE);
    for (int e = 0; e < b->nenv; e++) {
      float* d = &b->h_dr[(size_t)e * SIZE];
      for (int i = 0; i < nb; i++) d[MASS + i] = m.body_mass[i];
      for (int k = 0; k < 3; k++) d[IPOS + k] = m.body_ipos[1][k];
      for (int u = 0; u < nu; u++) { d[FRL + u] = m.dof_frictionloss[m.act_dofadr[u]]; d[ARM + u] = m.dof_armature[m.act_dofadr[u]]; d[Q0 + u] = m.qpos0[m.act_qposadr[u]]; d[KP + u] = m.act_kp[u]; }
    }
    b->dr_enabled = true;
  }
  int off, n;
  switch (param) {
    case ODK_PARAM_BODY_MASS: off = MASS; n = nb; break;
    case ODK_PARAM_BODY_IPOS_TORSO: off = IPOS; n = 3; break;
    case ODK_PARAM_DOF_FRICTIONLOSS: off = FRL; n = nu; break;
    case ODK_PARAM_DOF_ARMATURE: off = ARM; n = nu; break;
    case ODK_PARAM_QPOS0: off = Q0; n = nu; break;
    case ODK_PARAM_KP: off = KP; n = nu; break;
    default: return fail(ODK_ERR_INVALID, "unknown param %d", param);
  }
  if (count != n) return fail(ODK_ERR_INVALID, "param %d expects %d values per env, got %d", param, n, count);
  for (int e = 0; e < b->nenv; e++) memcpy(&b->h_dr[(size_t)e * SIZE + off], v + (size_t)e * n, n * sizeof(float));
  HIPCHK(hipSetDevice(b->device));
  if (!b->d_dr) HIPCHK(hipMalloc(&b->d_dr, b->h_dr.size() * sizeof(float)));
  HIPCHK(hipMemcpy(b->d_dr, b->h_dr.data(), b->h_dr.size() * sizeof(float), hipMemcpyHostToDevice));
  return ODK_OK;
}

static hipError_t launch(odk_batch* b, int which, const KArgs& a, hipStream_t st) {
  // height-field floors exist only with the backlash model (scene_rough_terrain_backlash.xml) and run 32 lanes per env; sphere / capsule
  // feet on one are their own instantiation (HF = 2): its out-of-line calls must not enter the duck kernel's register allocation
  if (!b->model.h.floor_is_plane) {
    if (b->model.h.cone) return launch_sg<ShapeBE, 32, 1>(which, a, st);      // (hull feet: checked at load)
    return b->model.h.foot_prim ? launch_sg<ShapeB, 32, 2>(which, a, st) : launch_sg<ShapeB, 32, 1>(which, a, st);
  }
  // robots that are not the duck (reference README.md:74-85): reset / step / physics kernels of their own shape, 32 lanes per env
#define X(i, S) if (i >= 2 && b->model.shape == i) return b->G == 32 ? launch_sg<S, 32, 0>(which, a, st) : hipErrorNotSupported;
  ODK_SHAPES(X)
#undef X
  if (b->model.h.cone) {      // the duck with elliptic cones (plane floor, checked at load): 32 lanes per env
    if (b->G != 32) return hipErrorNotSupported;
    return b->model.shape == 0 ? launch_sg<ShapeAE, 32, 0>(which, a, st) : launch_sg<ShapeBE, 32, 0>(which, a, st);
  }
  if (b->model.shape == 0) return b->G == 64 ? launch_sg<ShapeA, 64, 0>(which, a, st) : launch_sg<ShapeA, 32, 0>(which, a, st);
  return b->G == 64 ? launch_sg<ShapeB, 64, 0>(which, a, st) : launch_sg<ShapeB, 32, 0>(which, a, st);
}

static void base_args(odk_batch* b, KArgs& a, const odk_outputs* o) {
  memset(&a, 0, sizeof(a));
  a.m = b->d_model; a.prm = b->h_prm; a.prm_table = b->d_table; a.recs = b->d_recs; a.first = b->d_first;
  a.hfield = b->d_hfield;
  a.dr = b->dr_enabled ? b->d_dr : nullptr; a.nenv = b->nenv; a.n_substeps = b->cfg.n_substeps;
  a.dbg_lds = nullptr;
  a.cmd = b->d_cmd; a.cmd_stride = b->cmd_stride;
  a.push = b->d_push; a.push_stride = b->push_stride;
  a.delay = b->d_delay; a.delay_stride = b->delay_stride;
  a.xt = b->xt_on ? b->d_xt : nullptr; a.xmet = b->xt_on ? b->d_xmet : nullptr;
  a.imap = b->d_imap;
  a.hslot = b->d_hslot;
  if (o) { a.obs = o->obs_dev; a.priv = o->priv_dev; a.reward = o->reward_dev; a.done = o->done_dev; a.trunc = o->truncation_dev; a.metrics = o->metrics_dev; }
  to_dev_cfg(b->cfg, a.cfg, b->model.h.nu);
}

// The env kernels' task logic is joystick.py's with the robot's own tables (actuators, default pose, feet / imu sites, sensor addresses from the
// ModelBlob).  The imitation reward needs a joint map (custom_rewards.py:80-88) and a reference-motion table of the robot: the duck's shapes start
// with the duck's map, another robot's odk_reset / odk_step refuse use_imitation until odk_batch_set_imitation_joints gave one.  The Standing task
// needs a head-joint map (standing.py:590-597, rewards.py:105-147: the posture commands and the joints that cost_stand_still(ignore_head=True)
// leaves out; the duck's are its actuators 5..8): the duck's shapes start with it, another robot's odk_reset / odk_step refuse Standing until
// odk_batch_set_head_joints gave one (an all -1 map: a robot without a head).  odk_physics_step has no task logic
static int env_logic_ok(const odk_batch* b) {
  if (b->model.shape < 2) return ODK_OK;
  if (b->cfg.use_imitation && !b->imap_set)
    return fail(ODK_ERR_UNSUPPORTED, "use_imitation on a robot that is not the duck without an imitation joint map: the reference-motion table is open_duck_mini_v2's "
                "(give the robot's map with odk_batch_set_imitation_joints, or set use_imitation = 0)");
  if (b->cfg.env_kind != ODK_ENV_JOYSTICK && !b->hmap_set)
    return fail(ODK_ERR_UNSUPPORTED, "the Standing task on a robot that is not the duck without a head-joint map: the head joints are open_duck_mini_v2's "
                "(give the robot's with odk_batch_set_head_joints -- all -1 for none -- or set env_kind = ODK_ENV_JOYSTICK)");
  return ODK_OK;
}

static int g_debug_dump = 0;
extern "C" void odk_set_debug_dump(int on) { g_debug_dump = on; }

extern "C" int odk_reset(odk_batch* b, uint32_t seed, uint32_t env_id_offset, const odk_outputs* outs, void* stream) {
  if (!b) return fail(ODK_ERR_INVALID, "null batch");
  if (int rc = env_logic_ok(b)) return rc;
  HIPCHK(hipSetDevice(b->device));
  KArgs a;
  base_args(b, a, outs);
  a.seed = seed; a.env_offset = env_id_offset;
  a.dbg_lds = b->d_dbg;
  HIPCHK(launch(b, K_RESET, a, (hipStream_t)stream));
  return ODK_OK;
}

extern "C" int odk_step(odk_batch* b, const float* action_dev, const odk_outputs* outs, void* stream) {
  if (!b || !action_dev) return fail(ODK_ERR_INVALID, "null argument");
  if (int rc = env_logic_ok(b)) return rc;
  HIPCHK(hipSetDevice(b->device));
  KArgs a;
  base_args(b, a, outs);
  a.action = action_dev;
  a.dbg_lds = g_debug_dump ? b->d_dbg : nullptr;
  hipStream_t st = (hipStream_t)stream;
  // (event pairs are created by odk_batch_timing, never here: a step allocates nothing; when the pool is used up the
  // remaining launches of the window simply go untimed)
  if (b->timing > 0 && (b->timing_count++ % (size_t)b->timing) == 0 && b->ev_used < b->events.size()) {
    HIPCHK(hipEventRecord(b->events[b->ev_used].first, st));
    HIPCHK(launch(b, K_STEP, a, st));
    HIPCHK(hipEventRecord(b->events[b->ev_used].second, st));
    b->ev_used++;
  } else {
    HIPCHK(launch(b, K_STEP, a, st));
  }
  return ODK_OK;
}

extern "C" int odk_batch_bind_commands(odk_batch* b, const float* cmd_dev, int row_stride) {
  if (!b) return fail(ODK_ERR_INVALID, "null batch");
  if (cmd_dev && row_stride < 7) return fail(ODK_ERR_INVALID, "command rows hold 7 floats: row_stride %d < 7", row_stride);
  b->d_cmd = cmd_dev; b->cmd_stride = cmd_dev ? row_stride : 0;
  return ODK_OK;
}

extern "C" int odk_batch_bind_pushes(odk_batch* b, const float* push_dev, int row_stride) {
  if (!b) return fail(ODK_ERR_INVALID, "null batch");
  if (!push_dev) { b->d_push = nullptr; b->push_stride = 0; return ODK_OK; }
  if (row_stride < 2) return fail(ODK_ERR_INVALID, "odk_batch_bind_pushes: push rows hold 2 floats: row_stride %d < 2", row_stride);
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, push_dev) != hipSuccess) {
    (void)hipGetLastError();   // a pointer the runtime does not know: not this call's error to leave behind
    return fail(ODK_ERR_INVALID, "odk_batch_bind_pushes: push_dev is not device memory");
  }
  if (at.type != hipMemoryTypeDevice || at.device != b->device)
    return fail(ODK_ERR_INVALID, "odk_batch_bind_pushes: push_dev must be device memory of device %d (the batch's), it belongs to device %d", b->device,
                at.device);
  b->d_push = push_dev; b->push_stride = row_stride;
  return ODK_OK;
}

extern "C" int odk_batch_bind_action_delays(odk_batch* b, const int32_t* delay_dev, int row_stride) {
  if (!b) return fail(ODK_ERR_INVALID, "null batch");
  if (!delay_dev) { b->d_delay = nullptr; b->delay_stride = 0; return ODK_OK; }
  if (row_stride < 1) return fail(ODK_ERR_INVALID, "odk_batch_bind_action_delays: a delay row holds 1 int32: row_stride %d < 1", row_stride);
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, delay_dev) != hipSuccess) {
    (void)hipGetLastError();   // a pointer the runtime does not know: not this call's error to leave behind
    return fail(ODK_ERR_INVALID, "odk_batch_bind_action_delays: delay_dev is not device memory");
  }
  if (at.type != hipMemoryTypeDevice || at.device != b->device)
    return fail(ODK_ERR_INVALID, "odk_batch_bind_action_delays: delay_dev must be device memory of device %d (the batch's), it belongs to device %d",
                b->device, at.device);
  b->d_delay = delay_dev; b->delay_stride = row_stride;
  return ODK_OK;
}

extern "C" int odk_batch_set_reward_terms(odk_batch* b, const odk_reward_terms* t) {
  if (!b) return fail(ODK_ERR_INVALID, "null batch");
  static const char* const names[ODK_NXTERM] = {"lin_vel_z", "ang_vel_xy", "orientation", "base_height", "energy", "joint_pos_limits", "termination",
                                                "pose", "feet_slip", "feet_clearance", "feet_height", "feet_air_time"};
  XTerms h;
  memset(&h, 0, sizeof(h));
  bool on = false;
  if (t) for (int k = 0; k < ODK_NXTERM; k++) {
    if (!std::isfinite(t->scale[k])) return fail(ODK_ERR_INVALID, "odk_batch_set_reward_terms: scale of %s is not finite", names[k]);
    on = on || t->scale[k] != 0.0f;
  }
  if (on) {
    const DevModel& m = b->model.h;
    auto is_on = [&](int k) { return t->scale[k] != 0.0f; };
    auto need = [&](int k, const char* what, float v) { return !is_on(k) || std::isfinite(v) ? 0 : fail(ODK_ERR_INVALID, "odk_batch_set_reward_terms: %s needs a finite %s", names[k], what); };
    if (int rc = need(ODK_XTERM_BASE_HEIGHT, "base_height_target", t->base_height_target)) return rc;
    if (int rc = need(ODK_XTERM_FEET_CLEARANCE, "max_foot_height", t->max_foot_height)) return rc;
    if (int rc = need(ODK_XTERM_FEET_HEIGHT, "max_foot_height", t->max_foot_height)) return rc;
    if (int rc = need(ODK_XTERM_FEET_AIR_TIME, "air_time_range[0]", t->air_time_range[0])) return rc;
    if (int rc = need(ODK_XTERM_FEET_AIR_TIME, "air_time_range[1]", t->air_time_range[1])) return rc;
    if (int rc = need(ODK_XTERM_JOINT_POS_LIMITS, "soft_joint_pos_limit_factor", t->soft_joint_pos_limit_factor)) return rc;
    for (int u = 0; u < m.nu; u++) if (int rc = need(ODK_XTERM_POSE, "pose_weight per actuator", t->pose_weight[u])) return rc;
    if (is_on(ODK_XTERM_LIN_VEL_Z) && b->model.adr_global_linvel < 0)
      return fail(ODK_ERR_UNSUPPORTED, "odk_batch_set_reward_terms: lin_vel_z reads the imu's global_linvel sensor, which this model does not have");
    for (int k = 0; k < ODK_NXTERM; k++) h.scale[k] = t->scale[k];
    h.base_height_target = t->base_height_target; h.max_foot_height = t->max_foot_height;
    h.air_lo = t->air_time_range[0]; h.air_hi = t->air_time_range[1];
    h.adr_global_linvel = b->model.adr_global_linvel >= 0 ? b->model.adr_global_linvel : 0;
    for (int u = 0; u < m.nu; u++) {   // soft limits of the actuated joints (joystick.py:135-139), formed in double
      int j = -1;
      for (int k = 0; k < m.nj; k++) if (m.jnt_qposadr[k] == m.act_qposadr[u]) j = k;
      const double lo = j >= 0 ? m.jnt_range[j][0] : 0.0, hi = j >= 0 ? m.jnt_range[j][1] : 0.0;
      const double c = 0.5 * (lo + hi), r = hi - lo, f = t->soft_joint_pos_limit_factor;
      h.soft_lo[u] = (float)(c - 0.5 * r * f); h.soft_hi[u] = (float)(c + 0.5 * r * f);
      h.pose_w[u] = t->pose_weight[u];
    }
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());   // no step in flight reads the buffer while it changes
  HIPCHK(hipMemcpy(b->d_xt, &h, sizeof(h), hipMemcpyHostToDevice));
  b->xt_on = on;
  return ODK_OK;
}

extern "C" int odk_batch_set_imitation_joints(odk_batch* b, const int32_t* frame_joint, int nu) {
  if (!b || !frame_joint) return fail(ODK_ERR_INVALID, "null argument");
  if (nu != b->model.h.nu) return fail(ODK_ERR_INVALID, "odk_batch_set_imitation_joints: %d entries, the model has %d actuators", nu, b->model.h.nu);
  int h[MAXU];
  for (int u = 0; u < MAXU; u++) h[u] = -1;
  unsigned used = 0;
  for (int u = 0; u < nu; u++) {
    const int j = frame_joint[u];
    if (j < -1 || j > 15) return fail(ODK_ERR_INVALID, "odk_batch_set_imitation_joints: actuator %d maps to frame joint %d (valid: -1 .. 15)", u, j);
    if (j >= 0 && (used >> j & 1u)) return fail(ODK_ERR_INVALID, "odk_batch_set_imitation_joints: frame joint %d is used twice", j);
    if (j >= 0) used |= 1u << j;
    h[u] = j;
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());   // no step in flight reads the buffer while it changes
  HIPCHK(hipMemcpy(b->d_imap, h, sizeof(h), hipMemcpyHostToDevice));
  b->imap_set = true;
  return ODK_OK;
}

extern "C" int odk_batch_set_head_joints(odk_batch* b, const int32_t* actuator, int n) {
  if (!b || !actuator) return fail(ODK_ERR_INVALID, "null argument");
  if (n != 4) return fail(ODK_ERR_INVALID, "odk_batch_set_head_joints: %d entries, the map has 4 (neck_pitch, head_pitch, head_yaw, head_roll)", n);
  const int nu = b->model.h.nu;
  int h[MAXU];
  for (int u = 0; u < MAXU; u++) h[u] = -1;
  for (int k = 0; k < 4; k++) {
    const int u = actuator[k];
    if (u < -1 || u >= nu) return fail(ODK_ERR_INVALID, "odk_batch_set_head_joints: slot %d maps to actuator %d (valid: -1 .. %d)", k, u, nu - 1);
    if (u >= 0 && h[u] >= 0) return fail(ODK_ERR_INVALID, "odk_batch_set_head_joints: actuator %d is used twice (slots %d and %d)", u, h[u], k);
    if (u >= 0) h[u] = k;
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());   // no step in flight reads the buffer while it changes
  HIPCHK(hipMemcpy(b->d_hslot, h, sizeof(h), hipMemcpyHostToDevice));
  b->hmap_set = true;
  return ODK_OK;
}

extern "C" int odk_batch_bind_reward_metrics(odk_batch* b, float* dev) {
  if (!b) return fail(ODK_ERR_INVALID, "null batch");
  b->d_xmet = dev;
  return ODK_OK;
}

extern "C" int odk_physics_step(odk_batch* b, const float* ctrl_dev, int n_substeps, void* stream) {
  if (!b || !ctrl_dev) return fail(ODK_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(b->device));
  KArgs a;
  base_args(b, a, nullptr);
  a.action = ctrl_dev; a.n_substeps = n_substeps;
  a.dbg_lds = b->d_dbg;
  HIPCHK(launch(b, K_PHYS, a, (hipStream_t)stream));
  return ODK_OK;
}

extern "C" int odk_batch_timing(odk_batch* b, int enable, float* avg_ms, int* launches) {
  if (!b) return fail(ODK_ERR_INVALID, "null batch");
  HIPCHK(hipSetDevice(b->device));
  double tot = 0;
  for (size_t i = 0; i < b->ev_used; i++) {
    float ms = 0;
    HIPCHK(hipEventSynchronize(b->events[i].second));
    HIPCHK(hipEventElapsedTime(&ms, b->events[i].first, b->events[i].second));
    tot += ms;
  }
  if (avg_ms) *avg_ms = b->ev_used ? (float)(tot / b->ev_used) : 0.0f;
  if (launches) *launches = (int)b->ev_used;
  b->ev_used = 0; b->timing_count = 0;
  b->timing = enable > 0 ? enable : 0;
  while (b->timing > 0 && b->events.size() < odk_batch::ODK_TIMING_EVENT_PAIRS) {
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    b->events.push_back({e0, e1});
  }
  return ODK_OK;
}

extern "C" int odk_batch_lanes(const odk_batch* b) { return b ? b->G : -1; }
extern "C" int odk_batch_record_size(const odk_batch* b) { return b ? b->rec_size : -1; }
extern "C" int odk_batch_lds_size(const odk_batch* b) { return b ? b->lds_total : -1; }
extern "C" int odk_record_field(const odk_batch* b, const char* name, int* offset, int* count, int* kind) {
  if (!b || !name) return fail(ODK_ERR_INVALID, "null argument");
  const int nq = b->model.h.nq, nv = b->model.h.nv, I = nq + 2 * nv, nu = b->model.h.nu;
  const RecLay RL = rec_lay(nu);
  struct F { const char* name; int off, n, kind; };
  const F tab[] = {
    {"qpos", 0, nq, 0}, {"qvel", nq, nv, 0}, {"qacc_warmstart", nq + nv, nv, 0},
    {"command", I + RL.CMD, 7, 0}, {"last_act", I + RL.LAST, nu, 0}, {"last_last_act", I + RL.LAST2, nu, 0},
    {"last_last_last_act", I + RL.LAST3, nu, 0}, {"motor_targets", I + RL.MT, nu, 0}, {"feet_air_time", I + RL.AIR, 2, 0},
    {"swing_peak", I + RL.PEAK, 2, 0}, {"push", I + RL.PUSH, 2, 0}, {"action_history", I + RL.AHIST, 3 * nu, 0},
    {"imu_history", I + RL.IMU, 9, 0}, {"steps", I + RL.EPSTEPS, 1, 0}, {"truncation", I + RL.TRUNC, 1, 0},
    {"episode_done", I + RL.DONE, 1, 0}, {"episode_metrics/sum_reward", I + RL.EPSUM, 1, 0}, {"episode_metrics/length", I + RL.EPLEN, 1, 0},
    {"episode_metrics/reward_terms", I + RL.EPMET, 8, 0}, {"rng", I + RL.KEY0, 3, 1}, {"step", I + RL.STEP, 1, 1},
    {"push_step", I + RL.PSTEP, 1, 1}, {"push_interval_steps", I + RL.PINT, 1, 1}, {"imitation_i", I + RL.IMI, 1, 1},
    {"last_contact", I + RL.LCON, 1, 2},
  };
  for (const F& f : tab)
    if (!strcmp(name, f.name)) {
      if (offset) *offset = f.off;
      if (count) *count = f.n;
      if (kind) *kind = f.kind;
      return ODK_OK;
    }
  return fail(ODK_ERR_INVALID, "unknown record field '%s'", name);
}
extern "C" int odk_batch_get_records(odk_batch* b, float* host) {
  if (!b || !host) return fail(ODK_ERR_INVALID, "null");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, b->d_recs, (size_t)b->nenv * b->rec_size * sizeof(float), hipMemcpyDeviceToHost));
  return ODK_OK;
}
extern "C" int odk_batch_set_records(odk_batch* b, const float* host) {   // checkpoint restore / test presets of the carried info
  if (!b || !host) return fail(ODK_ERR_INVALID, "null");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(b->d_recs, host, (size_t)b->nenv * b->rec_size * sizeof(float), hipMemcpyHostToDevice));
  return ODK_OK;
}
extern "C" int odk_batch_get_lds(odk_batch* b, float* host) {  // debug image of the last forward pass (reset / physics_step / step with dump on)
  if (!b || !host) return fail(ODK_ERR_INVALID, "null");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, b->d_dbg, (size_t)b->nenv * b->lds_total * sizeof(float), hipMemcpyDeviceToHost));
  return ODK_OK;
}
// named offsets into the LDS image for tests
template <class S> static int lds_off(const char* name) {
  if (!strcmp(name, "qpos")) return S::O_QPOS;
  if (!strcmp(name, "qvel")) return S::O_QVEL;
  if (!strcmp(name, "warm")) return S::O_WARM;
  if (!strcmp(name, "ctrl")) return S::O_CTRL;
  if (!strcmp(name, "xpos")) return S::O_XPOS;
  if (!strcmp(name, "xquat")) return S::O_XQUAT;
  if (!strcmp(name, "crb")) return S::O_CRB;
  if (!strcmp(name, "cdof")) return S::O_CDOF;
  if (!strcmp(name, "M")) return S::O_M;
  if (!strcmp(name, "HL")) return S::O_HL;
  if (!strcmp(name, "qfrc_smooth")) return S::O_QFS;
  if (!strcmp(name, "qacc_smooth")) return S::O_QAS;
  if (!strcmp(name, "x")) return S::O_X;
  if (!strcmp(name, "Ma")) return S::O_MA;
  if (!strcmp(name, "search")) return S::O_GRAD;
  if (!strcmp(name, "mv")) return S::O_MV;
  if (!strcmp(name, "efc_D")) return S::O_D;
  if (!strcmp(name, "efc_aref")) return S::O_AREF;
  if (!strcmp(name, "jar")) return S::O_JAR;
  if (!strcmp(name, "jv")) return S::O_JV;
  if (!strcmp(name, "W")) return S::O_W;
  if (!strcmp(name, "contact_dist")) return S::O_CDIST;
  if (!strcmp(name, "contact_r")) return S::O_CR;
  if (!strcmp(name, "scr")) return S::O_SCR;
  if (!strcmp(name, "misc")) return S::O_SCR + S::S_MISC;   // the 16 misc scalars (solver diagnostics of the debug image; feet heights, gravity)
  if (!strcmp(name, "sensordata")) return S::O_SENS;
  if (!strcmp(name, "actuator_force")) return S::O_ACTF;
  if (!strcmp(name, "qacc")) return S::O_QACC;
  return -1;
}
extern "C" int odk_lds_offset(const odk_batch* b, const char* name) {
  if (!b || !name) return -1;
#define X(i, S) if (b->model.shape == i) return lds_off<S>(name);
  ODK_SHAPES(X)
#undef X
  return -1;
}

extern "C" int odk_batch_get_state(odk_batch* b, float* qpos, float* qvel, float* warm) {
  if (!b) return fail(ODK_ERR_INVALID, "null");
  std::vector<float> h((size_t)b->nenv * b->rec_size);
  int rc = odk_batch_get_records(b, h.data());
  if (rc) return rc;
  const int nq = b->model.h.nq, nv = b->model.h.nv;
  for (int e = 0; e < b->nenv; e++) {
    const float* r = &h[(size_t)e * b->rec_size];
    if (qpos) memcpy(qpos + (size_t)e * nq, r, nq * sizeof(float));
    if (qvel) memcpy(qvel + (size_t)e * nv, r + nq, nv * sizeof(float));
    if (warm) memcpy(warm + (size_t)e * nv, r + nq + nv, nv * sizeof(float));
  }
  return ODK_OK;
}
extern "C" int odk_batch_set_state(odk_batch* b, const float* qpos, const float* qvel, const float* warm) {
  if (!b) return fail(ODK_ERR_INVALID, "null");
  std::vector<float> h((size_t)b->nenv * b->rec_size);
  int rc = odk_batch_get_records(b, h.data());
  if (rc) return rc;
  const int nq = b->model.h.nq, nv = b->model.h.nv;
  for (int e = 0; e < b->nenv; e++) {
    float* r = &h[(size_t)e * b->rec_size];
    if (qpos) memcpy(r, qpos + (size_t)e * nq, nq * sizeof(float));
    if (qvel) memcpy(r + nq, qvel + (size_t)e * nv, nv * sizeof(float));
    if (warm) memcpy(r + nq + nv, warm + (size_t)e * nv, nv * sizeof(float));
  }
  HIPCHK(hipMemcpy(b->d_recs, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return ODK_OK;
}
extern "C" int odk_batch_get_debug(odk_batch* b, float* sensordata, float* actuator_force, float* contact_dist, float* qacc) {
  if (!b) return fail(ODK_ERR_INVALID, "null");
  std::vector<float> h((size_t)b->nenv * b->lds_total);
  int rc = odk_batch_get_lds(b, h.data());
  if (rc) return rc;
  const int nv = b->model.h.nv, nu = b->model.h.nu;
  const int o_s = odk_lds_offset(b, "sensordata"), o_a = odk_lds_offset(b, "actuator_force"), o_c = odk_lds_offset(b, "contact_dist"), o_q = odk_lds_offset(b, "qacc");
  for (int e = 0; e < b->nenv; e++) {
    const float* r = &h[(size_t)e * b->lds_total];
    if (sensordata) memcpy(sensordata + (size_t)e * NSENSD, r + o_s, NSENSD * sizeof(float));
    if (actuator_force) memcpy(actuator_force + (size_t)e * nu, r + o_a, nu * sizeof(float));
    if (contact_dist) memcpy(contact_dist + (size_t)e * NCON, r + o_c, NCON * sizeof(float));
    if (qacc) memcpy(qacc + (size_t)e * nv, r + o_q, nv * sizeof(float));
  }
  return ODK_OK;
}

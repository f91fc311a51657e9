// odk_engine.hip -- the batch C-ABI of include/odk.h (libodk.so) + the accumulator kernels of the tracking / push / gait / posture / imitation / response / fall reports
// and the command-schedule kernel.
//
// Host side: device buffers, launches on the caller's stream (blob -> DevModel, odk_model_load and the model getters: odk_model_load.hip).  Device side:
// the reset / step / physics-only kernels live in odk_env_kernels.h and are compiled one object per kernel set (odk_env_unit.hip); this file
// sees launch_sg's declaration (odk_shapes.h) and chooses the instantiation in launch().  gfx950 only; no CPU fallback of any kind.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/odk.h"
#include "odk_host.h"
#include "odk_shapes.h"

using namespace odk;

// the env kernels (reset / step / physics-only) and launch_sg: odk_env_kernels.h, one object per kernel set (odk_env_unit.hip)

// ================================================================================================
// host side
// (the thread's error string, fail() and the whole model side -- blob parsing, table builders, odk_model_load, the odk_model_* getters -- live in
// the host-only odk_model_load.hip; what follows is the batch API)
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(ODK_ERR_HIP, "%s: %s", #x, hipGetErrorString(_e)); } while (0)

struct odk_batch {
  odk_model model;
  int nenv, device, G;
  odk_env_config cfg;
  DevModel* d_model = nullptr; DevPRM h_prm; float* d_table = nullptr;
  float* d_recs = nullptr; float* d_first = nullptr; float* d_dr = nullptr; float* d_dbg = nullptr; float* d_hfield = nullptr;
  std::vector<float> h_dr; bool dr_enabled = false;
  int rec_size, frec_size, lds_total, dr_size, env_lds;
  static constexpr size_t ODK_TIMING_EVENT_PAIRS = 1024;
  int timing = 0; size_t timing_count = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> events; size_t ev_used = 0;   // timing: 0 off, n: every n-th launch
  const float* d_cmd = nullptr; int cmd_stride = 0;   // odk_batch_bind_commands (caller-owned device rows), null: sampled commands
  const float* d_push = nullptr; int push_stride = 0; // odk_batch_bind_pushes (caller-owned device rows), null: the sampled push
  const int32_t* d_delay = nullptr; int delay_stride = 0;   // odk_batch_bind_action_delays (caller-owned device rows), null: the sampled delay
  XTerms* d_xt = nullptr; bool xt_on = false;         // odk_batch_set_reward_terms: the batch's device copy; passed to the kernels while some term is on
  float* d_xmet = nullptr;                             // odk_batch_bind_reward_metrics (caller-owned)
  int* d_imap = nullptr; bool imap_set = false;        // odk_batch_set_imitation_joints: the batch's device copy; set: a map was given (the duck's
                                                       // shapes start with theirs)
  int* d_hslot = nullptr; bool hmap_set = false;       // odk_batch_set_head_joints: per actuator, its posture-command slot (-1: none); set as d_imap
};


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

// Velocity-tracking sums of one evaluation step (one thread per env): the achieved values are the noise-free privileged observation's
// gyro (row offset nobs) and local linear velocity (nobs + 9), joystick.py:596-604 / standing.py:549-556
__global__ void __launch_bounds__(256) tracking_kernel(const float* __restrict__ priv, int npriv, int nobs, const float* __restrict__ reward,
                                                       const float* __restrict__ done, const float* __restrict__ trunc, const float* __restrict__ cmd,
                                                       int cmd_stride, float* __restrict__ acc, int nenv) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  float* A = acc + (size_t)e * ODK_TRACK_NACC;
  if (A[ODK_TRACK_ENDED] != 0.0f) return;       // past its first episode (the Evaluator's `active`)
  const float d = done[e];
  A[ODK_TRACK_STEPS] += 1.0f;
  A[ODK_TRACK_REWARD] += reward[e];
  if (d != 0.0f) {   // the observation of a done step is the auto-reset's first one: no velocity sample
    if (trunc[e] == 0.0f) A[ODK_TRACK_FALLS] += 1.0f;
    A[ODK_TRACK_ENDED] = 1.0f;
    return;
  }
  const float* P = priv + (size_t)e * npriv;
  const float* C = cmd + (size_t)e * cmd_stride;
  const float v[3] = {P[nobs + 9], P[nobs + 10], P[nobs + 2]};
  A[ODK_TRACK_SAMPLES] += 1.0f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float err = v[k] - C[k];
    A[ODK_TRACK_SUM + k] += v[k];
    A[ODK_TRACK_SQERR + k] += err * err;
  }
}

extern "C" int odk_tracking_accumulate(const odk_batch* b, const float* priv_dev, const float* reward_dev, const float* done_dev,
                                       const float* truncation_dev, float* acc_dev, void* stream) {
  if (!b || !priv_dev || !reward_dev || !done_dev || !truncation_dev || !acc_dev) return fail(ODK_ERR_INVALID, "null argument");
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "odk_tracking_accumulate: no commands bound (odk_batch_bind_commands)");
  int nobs, npriv;
  obs_sizes_nu(b->model.h.nu, b->cfg.env_kind, &nobs, &npriv);
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(tracking_kernel, dim3((b->nenv + 255) / 256), dim3(256), 0, (hipStream_t)stream, priv_dev, npriv, nobs, reward_dev, done_dev,
                     truncation_dev, b->d_cmd, b->cmd_stride, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Push-recovery state of one evaluation step (one thread per env), issued between odk_step and odk_tracking_accumulate: the tracking
// accumulator's ENDED slot still tells whether the env's first episode was running when this step began.  Achieved velocities as above.
__global__ void __launch_bounds__(256) push_kernel(const float* __restrict__ priv, int npriv, int nobs, const float* __restrict__ done,
                                                   const float* __restrict__ trunc, const float* __restrict__ cmd, int cmd_stride,
                                                   const float* __restrict__ push, int push_stride, const float* __restrict__ track,
                                                   float lin_tol, float ang_tol, float* __restrict__ acc, int nenv) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  const float* T = track + (size_t)e * ODK_TRACK_NACC;
  if (T[ODK_TRACK_ENDED] != 0.0f) return;       // past its first episode
  float* A = acc + (size_t)e * ODK_PUSH_NACC;
  const float* K = push + (size_t)e * push_stride;
  bool pushed = A[ODK_PUSH_PUSHED] != 0.0f;
  if (!pushed && (K[0] != 0.0f || K[1] != 0.0f)) {   // the step that just ran read this row: the pushed step
    pushed = true;
    A[ODK_PUSH_PUSHED] = 1.0f;
    A[ODK_PUSH_PUSH_AT] = T[ODK_TRACK_STEPS];        // first-episode steps before this one
  }
  const float since = T[ODK_TRACK_STEPS] - A[ODK_PUSH_PUSH_AT] + 1.0f;   // steps from the pushed step to this one, counting both
  if (done[e] != 0.0f) {   // ends the first episode; no velocity sample (the observation is the auto-reset's)
    if (pushed && trunc[e] == 0.0f) { A[ODK_PUSH_FELL] = 1.0f; A[ODK_PUSH_STEPS_TO_FALL] = since; }
    return;
  }
  const float* P = priv + (size_t)e * npriv;
  const float* C = cmd + (size_t)e * cmd_stride;
  const float ex = P[nobs + 9] - C[0], ey = P[nobs + 10] - C[1];
  // the planar error through float64 (the squares are exact there, the root is correctly rounded, then one rounding to float32): a host
  // restatement reproduces it, and with it LAST_OFF and the peaks, bit for bit whatever the compiler fuses
  const float lin = (float)sqrt((double)ex * (double)ex + (double)ey * (double)ey), ang = fabsf(P[nobs + 2] - C[2]);
  if (!pushed) {
    // compensated (Kahan) sum: SUM stays within an ulp of the true sum however many samples come before the push; LOW keeps what SUM dropped
    const float s = A[ODK_PUSH_PRE_LIN_ERR_SUM], y = lin + A[ODK_PUSH_PRE_LIN_ERR_LOW];
    const float t = s + y;
    A[ODK_PUSH_PRE_LIN_ERR_SUM] = t;
    A[ODK_PUSH_PRE_LIN_ERR_LOW] = y - (t - s);
    A[ODK_PUSH_PRE_SAMPLES] += 1.0f;
    return;
  }
  if (lin > lin_tol || ang > ang_tol) A[ODK_PUSH_LAST_OFF] = since;
  A[ODK_PUSH_PEAK_LIN_ERR] = fmaxf(A[ODK_PUSH_PEAK_LIN_ERR], lin);
  A[ODK_PUSH_PEAK_ANG_ERR] = fmaxf(A[ODK_PUSH_PEAK_ANG_ERR], ang);
}

extern "C" int odk_push_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                                   const float* track_acc_dev, float lin_tol, float ang_tol, float* acc_dev, void* stream) {
  if (!b || !priv_dev || !done_dev || !truncation_dev || !track_acc_dev || !acc_dev) return fail(ODK_ERR_INVALID, "null argument");
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "odk_push_accumulate: no commands bound (odk_batch_bind_commands)");
  if (!b->d_push) return fail(ODK_ERR_INVALID, "odk_push_accumulate: no pushes bound (odk_batch_bind_pushes)");
  int nobs, npriv;
  obs_sizes_nu(b->model.h.nu, b->cfg.env_kind, &nobs, &npriv);
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(push_kernel, dim3((b->nenv + 255) / 256), dim3(256), 0, (hipStream_t)stream, priv_dev, npriv, nobs, done_dev, truncation_dev,
                     b->d_cmd, b->cmd_stride, b->d_push, b->push_stride, track_acc_dev, lin_tol, ang_tol, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Gait and actuator-load sums of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED contract of push_kernel).
// One 16-lane DPP row per env, lane = actuator, four envs per wave: the nu-wide reads of the privileged row and the per-actuator arrays of the
// accumulator row (stride ODK_GAIT_STRIDE = 16) are contiguous 64-byte accesses, the per-env scalars are row sums (the four in-row butterfly
// stages of greduce).  The 32 scalar slots are held two per lane (u and 16 + u); every lane computes the row-uniform terms and keeps its own.
// Only a gait sample (first episode, not done) stores anything, so every other row keeps its bits.
__device__ __forceinline__ float row_sum16(float x) {   // uniform control flow only
  x += ODK_DPP(x, 0xB1, 0xF); x += ODK_DPP(x, 0x4E, 0xF); x += ODK_DPP(x, 0x141, 0xF); x += ODK_DPP(x, 0x140, 0xF);
  return x;
}
__global__ void __launch_bounds__(256) gait_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                   const float* __restrict__ track, const float* __restrict__ limit, float* __restrict__ acc, int nenv) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, u = t & 15;
  const bool sample = e < nenv && track[(size_t)(e < nenv ? e : 0) * ODK_TRACK_NACC + ODK_TRACK_ENDED] == 0.0f && done[e < nenv ? e : 0] == 0.0f;
  const bool act = sample && u < nu;
  const float* P = priv + (size_t)(sample ? e : 0) * npriv;   // row 0 for the rows that only take part in the row sums
  float* A = acc + (size_t)(sample ? e : 0) * ODK_GAIT_NACC;
  const float* Q = P + nobs;
  // per actuator (0 in the lanes past nu and in the rows that are no sample)
  const float a1 = act ? P[13 + 2 * nu + u] : 0.0f, a2 = act ? P[13 + 3 * nu + u] : 0.0f;
  const float q = act ? Q[15 + u] : 0.0f, v = act ? Q[15 + nu + u] : 0.0f, f = act ? Q[16 + 2 * nu + u] : 0.0f;
  const float lim = (act && limit) ? limit[u] : 0.0f;
  const float af = fabsf(f), pw = fabsf(f * v), da = a1 - a2;
  const float power = row_sum16(pw), arate = row_sum16(da * da);
  if (!sample) return;
  // per env (the same in the row's 16 lanes)
  const float n0 = A[ODK_GAIT_SAMPLES];
  const bool first = n0 == 0.0f;
  const float h = Q[15 + 2 * nu];
  float c[2], td[2], swing[2], slip[2], run[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float* FV = Q + 18 + 3 * nu + 3 * k;
    const bool con = Q[16 + 3 * nu + k] != 0.0f;
    const float air = A[ODK_GAIT_AIR_RUN + k];
    const bool touch = con && !first && A[ODK_GAIT_PREV_CONTACT + k] == 0.0f;
    c[k] = con ? 1.0f : 0.0f;
    td[k] = touch ? 1.0f : 0.0f;
    swing[k] = touch ? air : 0.0f;               // the non-contact run that this touchdown ends
    slip[k] = con ? hypotf(FV[0], FV[1]) : 0.0f;
    run[k] = con ? 0.0f : air + 1.0f;
  }
  const float speed = hypotf(Q[9], Q[10]), wob = Q[0] * Q[0] + Q[1] * Q[1];
  // scalar slot s: what it gains, or (bookkeeping) what it becomes
  auto next = [&](int s, float old) {
    float inc = 0.0f;
    inc = s == ODK_GAIT_SAMPLES ? 1.0f : inc;
    inc = s == ODK_GAIT_SPEED_SUM ? speed : inc;
    inc = s == ODK_GAIT_ABS_POWER_SUM ? power : inc;
    inc = s == ODK_GAIT_CONTACT ? c[0] : s == ODK_GAIT_CONTACT + 1 ? c[1] : inc;
    inc = s == ODK_GAIT_DOUBLE ? c[0] * c[1] : inc;
    inc = s == ODK_GAIT_FLIGHT ? (1.0f - c[0]) * (1.0f - c[1]) : inc;
    inc = s == ODK_GAIT_TOUCHDOWNS ? td[0] : s == ODK_GAIT_TOUCHDOWNS + 1 ? td[1] : inc;
    inc = s == ODK_GAIT_SWING_STEPS_SUM ? swing[0] : s == ODK_GAIT_SWING_STEPS_SUM + 1 ? swing[1] : inc;
    inc = s == ODK_GAIT_SLIP_SUM ? slip[0] : s == ODK_GAIT_SLIP_SUM + 1 ? slip[1] : inc;
    inc = s == ODK_GAIT_HEIGHT_SUM ? h : inc;
    inc = s == ODK_GAIT_HEIGHT_SQ_SUM ? h * h : inc;
    inc = s == ODK_GAIT_ROLLPITCH_RATE_SQ_SUM ? wob : inc;
    inc = s == ODK_GAIT_ACTION_RATE_SUM ? arate : inc;
    float nv = old + inc;
    nv = s == ODK_GAIT_PREV_CONTACT ? c[0] : s == ODK_GAIT_PREV_CONTACT + 1 ? c[1] : nv;
    nv = s == ODK_GAIT_AIR_RUN ? run[0] : s == ODK_GAIT_AIR_RUN + 1 ? run[1] : nv;
    return nv;
  };
  const float s0 = next(u, A[u]), s1 = next(16 + u, A[16 + u]);
  A[u] = s0;
  A[16 + u] = s1;
  if (u >= nu) return;
  float* B = A + u;
  B[ODK_GAIT_TORQUE_SQ] += f * f;
  B[ODK_GAIT_TORQUE_PEAK] = fmaxf(B[ODK_GAIT_TORQUE_PEAK], af);
  B[ODK_GAIT_VEL_PEAK] = fmaxf(B[ODK_GAIT_VEL_PEAK], fabsf(v));
  B[ODK_GAIT_SAT] += (lim > 0.0f && af >= 0.99f * lim) ? 1.0f : 0.0f;
  B[ODK_GAIT_ABS_POWER] += pw;
  B[ODK_GAIT_RANGE_MIN] = first ? q : fminf(B[ODK_GAIT_RANGE_MIN], q);   // a zeroed row is no minimum: the first sample starts the range
  B[ODK_GAIT_RANGE_MAX] = first ? q : fmaxf(B[ODK_GAIT_RANGE_MAX], q);
}

extern "C" int odk_gait_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                                   const float* track_acc_dev, const float* torque_limit_dev, float* acc_dev, void* stream) {
  if (!b) return fail(ODK_ERR_INVALID, "odk_gait_accumulate: null batch");
  if (!priv_dev) return fail(ODK_ERR_INVALID, "odk_gait_accumulate: null priv_dev");
  if (!done_dev) return fail(ODK_ERR_INVALID, "odk_gait_accumulate: null done_dev");
  if (!truncation_dev) return fail(ODK_ERR_INVALID, "odk_gait_accumulate: null truncation_dev");
  if (!track_acc_dev) return fail(ODK_ERR_INVALID, "odk_gait_accumulate: null track_acc_dev");
  if (!acc_dev) return fail(ODK_ERR_INVALID, "odk_gait_accumulate: null acc_dev");
  const int nu = b->model.h.nu;
  if (nu > ODK_GAIT_STRIDE) return fail(ODK_ERR_INVALID, "odk_gait_accumulate: the model has %d actuators, a row holds %d", nu, ODK_GAIT_STRIDE);
  int nobs, npriv;
  obs_sizes_nu(nu, b->cfg.env_kind, &nobs, &npriv);
  HIPCHK(hipSetDevice(b->device));
  const long long threads = (long long)b->nenv * 16;
  hipLaunchKernelGGL(gait_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, priv_dev, npriv, nobs, nu, done_dev,
                     track_acc_dev, torque_limit_dev, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Posture and stillness sums of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED contract of push_kernel), in
// gait_kernel's layout: one 16-lane DPP row per env, lane = actuator, four envs per wave.  Every actuator lane loads its posture-command slot
// (hslot[u], -1: a leg) and its home pose; the per-env scalars are row sums, held one per lane (lanes 0 .. 9), and the lane whose hslot is
// k >= 0 owns slot k's entries of the four per-slot arrays.  Inputs, offsets into the env's privileged row (both tasks: build_obs_table):
// gyro nobs | gravity nobs + 6 | local linvel nobs + 9 | joint angle minus default nobs + 15 + u | joint_vel nobs + 15 + nu + u | root height
// nobs + 15 + 2 nu.  Only a sample (first episode, not done) stores anything, so every other row keeps its bits.
__device__ __forceinline__ float planar32(float x, float y) {   // hypot through float64: a host restatement has its bits (push_kernel's `lin`)
  return (float)sqrt((double)x * (double)x + (double)y * (double)y);
}
__global__ void __launch_bounds__(256) posture_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                      const float* __restrict__ track, const float* __restrict__ cmd, int cmd_stride,
                                                      const int* __restrict__ hslot, const DevModel* __restrict__ m, float tol,
                                                      float* __restrict__ acc, int nenv) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, u = t & 15;
  const bool sample = e < nenv && track[(size_t)(e < nenv ? e : 0) * ODK_TRACK_NACC + ODK_TRACK_ENDED] == 0.0f && done[e < nenv ? e : 0] == 0.0f;
  const bool act = sample && u < nu;
  const float* P = priv + (size_t)(sample ? e : 0) * npriv;   // row 0 for the rows that only take part in the row sums
  const float* C = cmd + (size_t)(sample ? e : 0) * cmd_stride;
  float* A = acc + (size_t)(sample ? e : 0) * ODK_POSTURE_NACC;
  const float* Q = P + nobs;
  // per actuator (0 in the lanes past nu and in the rows that are no sample)
  const int k = act ? hslot[u] : -1;
  const bool head = k >= 0, leg = act && k < 0;
  const float dq = act ? Q[15 + u] : 0.0f, v = act ? Q[15 + nu + u] : 0.0f;
  const float angle = head ? dq + m->key_ctrl[u] : 0.0f;
  const float err = head ? angle - C[3 + k] : 0.0f, aerr = fabsf(err), sq = err * err;
  const float leg_pose = row_sum16(leg ? fabsf(dq) : 0.0f), leg_vel = row_sum16(leg ? fabsf(v) : 0.0f), head_sq = row_sum16(sq);
  if (!sample) return;
  // per env (the same in the row's 16 lanes)
  const float n0 = A[ODK_POSTURE_SAMPLES];
  const float drift = planar32(Q[9], Q[10]), tilt = planar32(Q[6], Q[7]);
  const float yaw = Q[2] * Q[2], wob = Q[0] * Q[0] + Q[1] * Q[1], h = Q[15 + 2 * nu];
  if (u < 10) {   // scalar slot u: what it gains, or (the peak) what it becomes
    const float old = A[u];
    float inc = 0.0f;
    inc = u == ODK_POSTURE_SAMPLES ? 1.0f : inc;
    inc = u == ODK_POSTURE_DRIFT_SPEED_SUM ? drift : inc;
    inc = u == ODK_POSTURE_YAW_RATE_SQ_SUM ? yaw : inc;
    inc = u == ODK_POSTURE_ROLLPITCH_RATE_SQ_SUM ? wob : inc;
    inc = u == ODK_POSTURE_TILT_SUM ? tilt : inc;
    inc = u == ODK_POSTURE_HEIGHT_SUM ? h : inc;
    inc = u == ODK_POSTURE_LEG_POSE_SUM ? leg_pose : inc;
    inc = u == ODK_POSTURE_LEG_VEL_SUM ? leg_vel : inc;
    inc = u == ODK_POSTURE_HEAD_SQERR_SUM ? head_sq : inc;
    A[u] = u == ODK_POSTURE_TILT_PEAK ? fmaxf(old, tilt) : old + inc;
  }
  if (!head) return;
  float* B = A + k;
  B[ODK_POSTURE_ANGLE_SUM] += angle;
  B[ODK_POSTURE_ERR_SQ_SUM] += sq;
  B[ODK_POSTURE_ERR_PEAK] = fmaxf(B[ODK_POSTURE_ERR_PEAK], aerr);
  if (aerr > tol) B[ODK_POSTURE_LAST_OFF] = n0 + 1.0f;   // this sample's 1-based index
}

extern "C" int odk_posture_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                                      const float* track_acc_dev, float tol, float* acc_dev, void* stream) {
  if (!b) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: null batch");
  if (!priv_dev) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: null priv_dev");
  if (!done_dev) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: null done_dev");
  if (!truncation_dev) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: null truncation_dev");
  if (!track_acc_dev) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: null track_acc_dev");
  if (!acc_dev) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: null acc_dev");
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: no commands bound (odk_batch_bind_commands)");
  if (!b->hmap_set)
    return fail(ODK_ERR_INVALID, "odk_posture_accumulate: the batch has no head-joint map (odk_batch_set_head_joints; an all -1 map is a map)");
  const int nu = b->model.h.nu;
  if (nu > 16) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: the model has %d actuators, a row holds 16", nu);
  if (!std::isfinite(tol) || tol < 0.0f) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: tol = %g (a finite tolerance >= 0, in radians)", (double)tol);
  int nobs, npriv;
  obs_sizes_nu(nu, b->cfg.env_kind, &nobs, &npriv);
  HIPCHK(hipSetDevice(b->device));
  const long long threads = (long long)b->nenv * 16;
  hipLaunchKernelGGL(posture_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, priv_dev, npriv, nobs, nu, done_dev,
                     track_acc_dev, b->d_cmd, b->cmd_stride, b->d_hslot, b->d_model, tol, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Imitation-fidelity sums of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED contract of push_kernel), in
// gait_kernel's layout: one 16-lane DPP row per env, lane = actuator, four envs per wave.  Every actuator lane loads its frame joint through
// the batch's imitation map (imap[u], -1: not compared) and its home pose; the two reward terms are row sums, the 32 scalar slots are held two
// per lane (u and 16 + u) as gait's, and a compared lane owns entry u of the eight per-actuator arrays.  Inputs, offsets into the env's
// privileged Joystick row (build_obs_table): command 6 | local linvel nobs + 9 | joint angle minus default nobs + 15 + u | joint_vel nobs + 15
// + nu + u | contact nobs + 16 + 3 nu | the frame the reward read (O_REF) nobs + 26 + 3 nu.  Only a sample (first episode, not done) stores
// anything, so every other row keeps its bits.
__global__ void __launch_bounds__(256) imitation_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                        const float* __restrict__ track, const int* __restrict__ imap,
                                                        const DevModel* __restrict__ m, int period, float* __restrict__ acc, int nenv) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, u = t & 15;
  const bool sample = e < nenv && track[(size_t)(e < nenv ? e : 0) * ODK_TRACK_NACC + ODK_TRACK_ENDED] == 0.0f && done[e < nenv ? e : 0] == 0.0f;
  const bool act = sample && u < nu;
  const float* P = priv + (size_t)(sample ? e : 0) * npriv;   // row 0 for the rows that only take part in the row sums
  float* A = acc + (size_t)(sample ? e : 0) * ODK_IMIT_NACC;
  const float* Q = P + nobs;
  const float* F = Q + 26 + 3 * nu;
  // per actuator (0 in the lanes past nu, in the lanes the map leaves out and in the rows that are no sample)
  const int ri = act ? imap[u] : -1;
  const bool cmp = ri >= 0;
  const float jq = cmp ? Q[15 + u] + m->key_ctrl[u] : 0.0f, rq = cmp ? F[ri] : 0.0f;
  const float dp = jq - rq, dv = cmp ? Q[15 + nu + u] - F[16 + ri] : 0.0f;
  const float sp = dp * dp, sv = dv * dv;
  const float jpos = row_sum16(sp), jvel = row_sum16(sv);
  if (!sample) return;
  // per env (the same in the row's 16 lanes)
  const bool first = A[ODK_IMIT_SAMPLES] == 0.0f;
  const float gated = sqrtf(P[6] * P[6] + P[7] * P[7] + P[8] * P[8]) > 0.01f ? 1.0f : 0.0f;   // the reward's gate (step_kernel's cn)
  const float sr = planar32(F[34], F[35]), ds = planar32(Q[9], Q[10]) - sr;
  const float per = (float)period;
  float c[2], r[2], both[2], ronly[2], fonly[2], rtd[2], td[2], lag[2], age[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const bool con = Q[16 + 3 * nu + k] != 0.0f, ref = F[32 + k] > 0.5f;
    const bool rtouch = ref && !first && A[ODK_IMIT_PREV_REF + k] == 0.0f;
    const float a0 = A[ODK_IMIT_REF_AGE + k];
    const float a1 = rtouch ? 1.0f : (a0 > 0.0f ? a0 + 1.0f : 0.0f);   // the reference first: a touchdown in the same sample has lag 0
    const bool touch = con && !first && A[ODK_IMIT_PREV_CONTACT + k] == 0.0f && a1 > 0.0f;
    float l = a1 - 1.0f;
    if (period > 0 && 2.0f * l > per) l -= per;                        // past half a period: early for the reference's next touchdown
    c[k] = con ? 1.0f : 0.0f;
    r[k] = ref ? 1.0f : 0.0f;
    both[k] = (con && ref) ? 1.0f : 0.0f;
    ronly[k] = (con && !ref) ? 1.0f : 0.0f;
    fonly[k] = (!con && ref) ? 1.0f : 0.0f;
    rtd[k] = rtouch ? 1.0f : 0.0f;
    td[k] = touch ? 1.0f : 0.0f;
    lag[k] = touch ? l : 0.0f;
    age[k] = a1;
  }
  // scalar slot s: what it gains, or (bookkeeping) what it becomes
  auto next = [&](int s, float old) {
    float inc = 0.0f;
    inc = s == ODK_IMIT_SAMPLES ? 1.0f : inc;
    inc = s == ODK_IMIT_GATED ? gated : inc;
    inc = s == ODK_IMIT_SPEED_ERR_SQ_SUM ? ds * ds : inc;
    inc = s == ODK_IMIT_REF_SPEED_SUM ? sr : inc;
    inc = s == ODK_IMIT_JOINT_POS_SQ_SUM ? jpos : inc;
    inc = s == ODK_IMIT_JOINT_VEL_SQ_SUM ? jvel : inc;
    inc = s == ODK_IMIT_BOTH ? both[0] : s == ODK_IMIT_BOTH + 1 ? both[1] : inc;
    inc = s == ODK_IMIT_ROBOT_ONLY ? ronly[0] : s == ODK_IMIT_ROBOT_ONLY + 1 ? ronly[1] : inc;
    inc = s == ODK_IMIT_REF_ONLY ? fonly[0] : s == ODK_IMIT_REF_ONLY + 1 ? fonly[1] : inc;
    inc = s == ODK_IMIT_REF_TOUCHDOWNS ? rtd[0] : s == ODK_IMIT_REF_TOUCHDOWNS + 1 ? rtd[1] : inc;
    inc = s == ODK_IMIT_TOUCHDOWNS ? td[0] : s == ODK_IMIT_TOUCHDOWNS + 1 ? td[1] : inc;
    inc = s == ODK_IMIT_LAG_SUM ? lag[0] : s == ODK_IMIT_LAG_SUM + 1 ? lag[1] : inc;
    inc = s == ODK_IMIT_LAG_ABS_SUM ? fabsf(lag[0]) : s == ODK_IMIT_LAG_ABS_SUM + 1 ? fabsf(lag[1]) : inc;
    float nv = old + inc;
    nv = s == ODK_IMIT_PREV_CONTACT ? c[0] : s == ODK_IMIT_PREV_CONTACT + 1 ? c[1] : nv;
    nv = s == ODK_IMIT_PREV_REF ? r[0] : s == ODK_IMIT_PREV_REF + 1 ? r[1] : nv;
    nv = s == ODK_IMIT_REF_AGE ? age[0] : s == ODK_IMIT_REF_AGE + 1 ? age[1] : nv;
    return nv;
  };
  const float s0 = next(u, A[u]), s1 = next(16 + u, A[16 + u]);
  A[u] = s0;
  A[16 + u] = s1;
  if (!cmp) return;
  float* B = A + u;
  B[ODK_IMIT_POS_ERR_SUM] += dp;
  B[ODK_IMIT_POS_ERR_SQ] += sp;
  B[ODK_IMIT_POS_ERR_PEAK] = fmaxf(B[ODK_IMIT_POS_ERR_PEAK], fabsf(dp));
  B[ODK_IMIT_VEL_ERR_SQ] += sv;
  B[ODK_IMIT_RANGE_MIN] = first ? jq : fminf(B[ODK_IMIT_RANGE_MIN], jq);   // a zeroed row is no minimum: the first sample starts the ranges
  B[ODK_IMIT_RANGE_MAX] = first ? jq : fmaxf(B[ODK_IMIT_RANGE_MAX], jq);
  B[ODK_IMIT_REF_RANGE_MIN] = first ? rq : fminf(B[ODK_IMIT_REF_RANGE_MIN], rq);
  B[ODK_IMIT_REF_RANGE_MAX] = first ? rq : fmaxf(B[ODK_IMIT_REF_RANGE_MAX], rq);
}

extern "C" int odk_imitation_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                                        const float* track_acc_dev, int period_steps, float* acc_dev, void* stream) {
  if (!b) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: null batch");
  if (!priv_dev) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: null priv_dev");
  if (!done_dev) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: null done_dev");
  if (!truncation_dev) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: null truncation_dev");
  if (!track_acc_dev) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: null track_acc_dev");
  if (!acc_dev) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: null acc_dev");
  if (b->cfg.env_kind != ODK_ENV_JOYSTICK)
    return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: a Standing batch's privileged row has no reference-motion frame (env_kind = ODK_ENV_JOYSTICK only)");
  if (!b->cfg.use_imitation)
    return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: use_imitation = 0: the frame of the privileged row is all zeros, there is nothing to compare with");
  if (!b->imap_set)
    return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: the batch has no imitation joint map (odk_batch_set_imitation_joints)");
  const int nu = b->model.h.nu;
  if (nu > ODK_IMIT_STRIDE) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: the model has %d actuators, a row holds %d", nu, ODK_IMIT_STRIDE);
  if (period_steps < 0) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: period_steps = %d (the reference motion's nb_steps_in_period, or 0 for unfolded lags)", period_steps);
  int nobs, npriv;
  obs_sizes_nu(nu, b->cfg.env_kind, &nobs, &npriv);
  HIPCHK(hipSetDevice(b->device));
  const long long threads = (long long)b->nenv * 16;
  hipLaunchKernelGGL(imitation_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, priv_dev, npriv, nobs, nu, done_dev,
                     track_acc_dev, b->d_imap, b->d_model, period_steps, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Command schedules.  The segment of schedule row S ([nseg, ODK_SCHED_SEG_FLOATS]) in force at first-episode step t: the last one whose
// start_step is <= t (segment 0 when none is: a table whose first start is not 0 is the caller's mistake, not an out-of-range index)
__device__ __forceinline__ int sched_segment(const float* __restrict__ S, int nseg, float t) {
  int k = 0;
  for (int i = 1; i < nseg; i++) k = S[i * ODK_SCHED_SEG_FLOATS] <= t ? i : k;
  return k;
}
__device__ __forceinline__ const float* sched_row(const float* __restrict__ sched, int nsched, int nseg, const int* __restrict__ sched_of_env, int e) {
  const int s = min(max(sched_of_env[e], 0), nsched - 1);   // a map entry outside the table reads a valid row, never past it
  return sched + (size_t)s * nseg * ODK_SCHED_SEG_FLOATS;
}

// The command of the step about to run (one thread per env), issued before odk_step: the tracking accumulator's STEPS slot is the clock.
// An env past its first episode keeps the command of the step that ended it (STEPS - 1; STEPS >= 1 once ENDED is set).
__global__ void __launch_bounds__(256) sched_apply_kernel(const float* __restrict__ sched, int nsched, int nseg, const int* __restrict__ sched_of_env,
                                                          const float* __restrict__ track, float* __restrict__ cmd, int cmd_stride, int nenv) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  const float* T = track + (size_t)e * ODK_TRACK_NACC;
  const float t = T[ODK_TRACK_ENDED] != 0.0f ? T[ODK_TRACK_STEPS] - 1.0f : T[ODK_TRACK_STEPS];
  const float* S = sched_row(sched, nsched, nseg, sched_of_env, e);
  const float* G = S + sched_segment(S, nseg, t) * ODK_SCHED_SEG_FLOATS + 1;
  float* C = cmd + (size_t)e * cmd_stride;
#pragma unroll
  for (int k = 0; k < 7; k++) C[k] = G[k];
}

static int sched_args_ok(const char* fn, const odk_batch* b, const float* sched_dev, int nsched, int nseg, const int32_t* sched_of_env_dev,
                         const float* track_acc_dev) {
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!sched_dev) return fail(ODK_ERR_INVALID, "%s: null sched_dev", fn);
  if (!sched_of_env_dev) return fail(ODK_ERR_INVALID, "%s: null sched_of_env_dev", fn);
  if (!track_acc_dev) return fail(ODK_ERR_INVALID, "%s: null track_acc_dev", fn);
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "%s: no commands bound (odk_batch_bind_commands)", fn);
  if (nseg < 1 || nseg > ODK_SCHED_MAX_SEGMENTS) return fail(ODK_ERR_INVALID, "%s: nseg = %d (a schedule has 1 .. %d segments)", fn, nseg, ODK_SCHED_MAX_SEGMENTS);
  if (nsched < 1) return fail(ODK_ERR_INVALID, "%s: nsched = %d (at least one schedule)", fn, nsched);
  return ODK_OK;
}

extern "C" int odk_command_schedule_apply(const odk_batch* b, const float* sched_dev, int nsched, int nseg, const int32_t* sched_of_env_dev,
                                          const float* track_acc_dev, void* stream) {
  if (int rc = sched_args_ok("odk_command_schedule_apply", b, sched_dev, nsched, nseg, sched_of_env_dev, track_acc_dev)) return rc;
  HIPCHK(hipSetDevice(b->device));
  // the bound buffer is the caller's own device memory, handed over read-only for the step kernels; this launch is the one writer
  hipLaunchKernelGGL(sched_apply_kernel, dim3((b->nenv + 255) / 256), dim3(256), 0, (hipStream_t)stream, sched_dev, nsched, nseg, sched_of_env_dev,
                     track_acc_dev, const_cast<float*>(b->d_cmd), b->cmd_stride, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Step-response state of one evaluation step (one thread per env), issued between odk_step and odk_tracking_accumulate (the ENDED / STEPS
// contract of push_kernel): only the block of the segment in force at the step that just ran is touched.  Velocities and errors as
// push_kernel's.  Contraction is off: every product is rounded before it is added, so a float32 host restatement has the sums' bits.
__global__ void __launch_bounds__(256) response_kernel(const float* __restrict__ priv, int npriv, int nobs, const float* __restrict__ done,
                                                       const float* __restrict__ trunc, const float* __restrict__ cmd, int cmd_stride,
                                                       const float* __restrict__ track, const float* __restrict__ sched, int nsched, int nseg,
                                                       const int* __restrict__ sched_of_env, float lin_tol, float ang_tol, float tail_after,
                                                       float* __restrict__ acc, int nenv) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  const float* T = track + (size_t)e * ODK_TRACK_NACC;
  if (T[ODK_TRACK_ENDED] != 0.0f) return;       // past its first episode
  const float t = T[ODK_TRACK_STEPS];           // first-episode steps before the one that just ran: its index
  const float* S = sched_row(sched, nsched, nseg, sched_of_env, e);
  const int seg = sched_segment(S, nseg, t);
  const float* G = S + seg * ODK_SCHED_SEG_FLOATS;
  float* A = acc + (size_t)e * ODK_RESP_NACC + seg * ODK_RESP_STRIDE;
  const float k = t - G[0] + 1.0f;              // 1-based index of this step among the steps of its segment
  A[ODK_RESP_ENTERED] = 1.0f;
  if (done[e] != 0.0f) {   // ends the first episode; no velocity sample (the observation is the auto-reset's)
    if (trunc[e] == 0.0f) { A[ODK_RESP_FELL] = 1.0f; A[ODK_RESP_STEPS_TO_FALL] = k; }
    return;
  }
  const float* P = priv + (size_t)e * npriv;
  const float* C = cmd + (size_t)e * cmd_stride;
  const float v[3] = {P[nobs + 9], P[nobs + 10], P[nobs + 2]};
  const float ex = v[0] - C[0], ey = v[1] - C[1];
  const float lin = (float)sqrt((double)ex * (double)ex + (double)ey * (double)ey), ang = fabsf(v[2] - C[2]);   // push_kernel's
  A[ODK_RESP_SAMPLES] += 1.0f;
  float first_in = A[ODK_RESP_FIRST_IN];
  if (lin > lin_tol || ang > ang_tol) A[ODK_RESP_LAST_OFF] = k;
  else if (first_in == 0.0f) A[ODK_RESP_FIRST_IN] = first_in = k;
  if (first_in != 0.0f) {
    A[ODK_RESP_PEAK_LIN_ERR] = fmaxf(A[ODK_RESP_PEAK_LIN_ERR], lin);
    A[ODK_RESP_PEAK_ANG_ERR] = fmaxf(A[ODK_RESP_PEAK_ANG_ERR], ang);
  }
  const bool tail = k > tail_after;
  if (tail) A[ODK_RESP_TAIL_SAMPLES] += 1.0f;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float err = v[a] - C[a];
    const float sq = err * err;
    A[ODK_RESP_SUM + a] += v[a];
    A[ODK_RESP_SQERR + a] += sq;
    const float prev = seg > 0 ? S[(seg > 0 ? seg - 1 : 0) * ODK_SCHED_SEG_FLOATS + 1 + a] : 0.0f;   // segment 0: the episode starts at rest
    const float dir = C[a] > prev ? 1.0f : (C[a] < prev ? -1.0f : 0.0f);
    const float over = err * dir;
    if (over > A[ODK_RESP_OVERSHOOT + a]) A[ODK_RESP_OVERSHOOT + a] = over;   // (a strict compare: a -0 product never replaces the zeroed slot's +0)
    if (tail) A[ODK_RESP_TAIL_SUM + a] += v[a];
  }
}

extern "C" int odk_response_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                                       const float* track_acc_dev, const float* sched_dev, int nsched, int nseg, const int32_t* sched_of_env_dev,
                                       float lin_tol, float ang_tol, int tail_after, float* acc_dev, void* stream) {
  const char* fn = "odk_response_accumulate";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!priv_dev) return fail(ODK_ERR_INVALID, "%s: null priv_dev", fn);
  if (!done_dev) return fail(ODK_ERR_INVALID, "%s: null done_dev", fn);
  if (!truncation_dev) return fail(ODK_ERR_INVALID, "%s: null truncation_dev", fn);
  if (!acc_dev) return fail(ODK_ERR_INVALID, "%s: null acc_dev", fn);
  if (int rc = sched_args_ok(fn, b, sched_dev, nsched, nseg, sched_of_env_dev, track_acc_dev)) return rc;
  if (!std::isfinite(lin_tol) || lin_tol < 0.0f) return fail(ODK_ERR_INVALID, "%s: lin_tol = %g (a finite tolerance >= 0, in m/s)", fn, (double)lin_tol);
  if (!std::isfinite(ang_tol) || ang_tol < 0.0f) return fail(ODK_ERR_INVALID, "%s: ang_tol = %g (a finite tolerance >= 0, in rad/s)", fn, (double)ang_tol);
  if (tail_after < 0) return fail(ODK_ERR_INVALID, "%s: tail_after = %d (a number of steps >= 0)", fn, tail_after);
  int nobs, npriv;
  obs_sizes_nu(b->model.h.nu, b->cfg.env_kind, &nobs, &npriv);
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(response_kernel, dim3((b->nenv + 255) / 256), dim3(256), 0, (hipStream_t)stream, priv_dev, npriv, nobs, done_dev, truncation_dev,
                     b->d_cmd, b->cmd_stride, track_acc_dev, sched_dev, nsched, nseg, sched_of_env_dev, lin_tol, ang_tol, (float)tail_after, acc_dev,
                     b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Fall recorder of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED / STEPS contract of push_kernel), in
// gait_kernel's layout: one 16-lane DPP row per env, four envs per wave.  For the saturation count lane = actuator (a row sum of 0 / 1 flags:
// exact); for the stores lane = float: the 16 scalars of the ring slot are one contiguous 64-byte store of the row, the qpos copy from the
// batch's record (offset 0 of the env's row of d_recs) is ceil(nq / 16) passes of consecutive lanes on consecutive floats, and the head's
// slots are written by the lane of their number.  Only the slot of this sample and the head are stored to, and only during the first episode:
// every other float keeps its bits.  Contraction is off and both hypots go through float64, so a host restatement has the row's bits.
__global__ void __launch_bounds__(256) fall_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                   const float* __restrict__ trunc, const float* __restrict__ track, const float* __restrict__ cmd,
                                                   int cmd_stride, const float* __restrict__ limit, const float* __restrict__ recs, int rec_size,
                                                   int nq, float tilt_tol, int ring, float* __restrict__ acc, int row_stride, int nenv) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, u = t & 15;
  const int e0 = e < nenv ? e : 0;
  const float* T = track + (size_t)e0 * ODK_TRACK_NACC;
  const bool live = e < nenv && T[ODK_TRACK_ENDED] == 0.0f;       // the first episode was running when this step began
  const bool sample = live && done[e0] == 0.0f;
  const bool act = sample && u < nu;
  const float* Q = priv + (size_t)(sample ? e : 0) * npriv + nobs;   // row 0 for the rows that only take part in the row sum
  const float f = act ? Q[16 + 2 * nu + u] : 0.0f;
  const float lim = (act && limit) ? limit[u] : 0.0f;
  const float sat = row_sum16((lim > 0.0f && fabsf(f) >= 0.99f * lim) ? 1.0f : 0.0f);
  if (!live) return;
  float* A = acc + (size_t)e * row_stride;
  const float step = T[ODK_TRACK_STEPS];                          // first-episode steps before the one that just ran: its index
  if (!sample) {   // ends the first episode; no sample (the observation and the state are the auto-reset's)
    if (trunc[e] == 0.0f && (u == ODK_FALL_FELL || u == ODK_FALL_STEP)) A[u] = u == ODK_FALL_FELL ? 1.0f : step;
    return;
  }
  // per env (the same in the row's 16 lanes)
  const float n0 = A[ODK_FALL_SAMPLES];
  const float* C = cmd + (size_t)e * cmd_stride;
  const float lin = planar32(Q[9] - C[0], Q[10] - C[1]), ang = fabsf(Q[2] - C[2]);   // push_kernel's
  const float tilt = planar32(Q[6], Q[7]);                                            // posture_kernel's
  const bool upright = tilt <= tilt_tol;
  const float con[2] = {Q[16 + 3 * nu], Q[17 + 3 * nu]};
  // lane u's scalar of the slot: a copy of the privileged row at `off`, or one of the four computed ones
  int off = u + 5;                                                // S_UP: nobs + 6 ..
  off = u >= ODK_FALL_S_GYRO ? u - ODK_FALL_S_GYRO : off;
  off = u >= ODK_FALL_S_LINVEL ? u + 2 : off;                     // nobs + 9 ..
  off = u == ODK_FALL_S_HEIGHT ? 15 + 2 * nu : off;
  off = u >= ODK_FALL_S_CONTACT ? 16 + 3 * nu + (u - ODK_FALL_S_CONTACT) : off;
  off = (u == ODK_FALL_S_STEP || u >= ODK_FALL_S_LIN_ERR) ? 0 : off;
  float v = Q[off];
  v = u == ODK_FALL_S_STEP ? step : v;
  v = u == ODK_FALL_S_LIN_ERR ? lin : v;
  v = u == ODK_FALL_S_ANG_ERR ? ang : v;
  v = u == ODK_FALL_S_SAT ? sat : v;
  const unsigned slot = (unsigned)(int)n0 % (unsigned)ring;       // (unsigned: a row the caller did not zero still lands inside its ring)
  float* S = A + ODK_FALL_HEAD + (size_t)slot * (ODK_FALL_SAMPLE + nq);
  S[u] = v;
  const float* R = recs + (size_t)e * rec_size;
  for (int j = u; j < nq; j += 16) S[ODK_FALL_SAMPLE + j] = R[j];
  // the head: lane = slot
  if (u == ODK_FALL_SAMPLES) A[u] = n0 + 1.0f;
  if (u == ODK_FALL_LAST_UPRIGHT && upright) A[u] = n0 + 1.0f;   // this sample's 1-based number
  if ((u == ODK_FALL_UPRIGHT_CONTACT || u == ODK_FALL_UPRIGHT_CONTACT + 1) && upright) A[u] = con[u - ODK_FALL_UPRIGHT_CONTACT];
  if (u == ODK_FALL_TILT_PEAK) A[u] = fmaxf(A[u], tilt);
}

extern "C" int odk_fall_row_floats(const odk_batch* b, int ring) {
  if (!b || ring < 1 || ring > ODK_FALL_MAX_RING) return -1;
  return ODK_FALL_HEAD + ring * (ODK_FALL_SAMPLE + b->model.h.nq);
}

extern "C" int odk_fall_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                                   const float* track_acc_dev, const float* torque_limit_dev, float tilt_tol, int ring, float* acc_dev,
                                   int row_stride, void* stream) {
  const char* fn = "odk_fall_accumulate";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!priv_dev) return fail(ODK_ERR_INVALID, "%s: null priv_dev", fn);
  if (!done_dev) return fail(ODK_ERR_INVALID, "%s: null done_dev", fn);
  if (!truncation_dev) return fail(ODK_ERR_INVALID, "%s: null truncation_dev", fn);
  if (!track_acc_dev) return fail(ODK_ERR_INVALID, "%s: null track_acc_dev", fn);
  if (!acc_dev) return fail(ODK_ERR_INVALID, "%s: null acc_dev", fn);
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "%s: no commands bound (odk_batch_bind_commands)", fn);
  if (ring < 1 || ring > ODK_FALL_MAX_RING) return fail(ODK_ERR_INVALID, "%s: ring = %d (1 .. %d samples)", fn, ring, ODK_FALL_MAX_RING);
  const int nu = b->model.h.nu, nq = b->model.h.nq, need = odk_fall_row_floats(b, ring);
  if (row_stride < need) return fail(ODK_ERR_INVALID, "%s: row_stride = %d, a row of ring %d holds %d floats (odk_fall_row_floats)", fn, row_stride, ring, need);
  if (nu > 16) return fail(ODK_ERR_INVALID, "%s: the model has %d actuators, a row holds 16", fn, nu);
  if (!std::isfinite(tilt_tol) || tilt_tol < 0.0f)
    return fail(ODK_ERR_INVALID, "%s: tilt_tol = %g (a finite sine of the lean >= 0)", fn, (double)tilt_tol);
  int nobs, npriv;
  obs_sizes_nu(nu, b->cfg.env_kind, &nobs, &npriv);
  HIPCHK(hipSetDevice(b->device));
  const long long threads = (long long)b->nenv * 16;
  hipLaunchKernelGGL(fall_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, priv_dev, npriv, nobs, nu, done_dev,
                     truncation_dev, track_acc_dev, b->d_cmd, b->cmd_stride, torque_limit_dev, b->d_recs, b->rec_size, nq, tilt_tol, ring, acc_dev,
                     row_stride, b->nenv);
  HIPCHK(hipGetLastError());
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

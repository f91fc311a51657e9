// odk_engine.hip -- fused env-step kernels + the batch C-ABI of include/odk.h (libodk.so).
//
// Host side: device buffers, launches on the caller's stream (blob -> DevModel, odk_model_load and the model getters: odk_model_load.hip).  Device side:
// reset / step / physics-only kernels built from odk_kernels.h.  Env logic follows the reference
// playground/open_duck_mini_v2/joystick.py (line map next to each block) and the brax
// Episode/AutoReset wrappers.  gfx950 only; no CPU fallback of any kind.
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

// per-env HBM records, observation strides, random-draw streams, the env logic's LDS floats (EnvL) and the compiled shapes: odk_shapes.h

// the workgroup's copy of the shared tables (call with all 64 lanes; followed by a hand-off barrier at the caller)
template <class S> __device__ __forceinline__ const int* load_shared(float* lds, int envs, const DevModel* m) {
  int* RT = reinterpret_cast<int*>(lds + envs * EnvL<S>::TOTAL);
  {
    constexpr int T = (S::NMR + 63) / 64;
    int v[T];
#pragma unroll
    for (int t = 0; t < T; t++) { const int k = threadIdx.x + 64 * t; v[t] = m->R_ent[k < S::NMR ? k : 0]; }
#pragma unroll
    for (int t = 0; t < T; t++) { const int k = threadIdx.x + 64 * t; if (k < S::NMR) RT[k] = v[t]; }
  }
  float* SH = reinterpret_cast<float*>(RT);
  float* CT = SH + S::SH_CT;
  const int k = threadIdx.x;
  if (k < 3) { CT[k] = m->pair_mu[k]; CT[3 + k] = m->pair_invweight[k]; }
  if (k < 27) CT[6 + k] = m->pair_imp[k / 9][k % 9];
  if (k < 9) CT[33 + k] = m->plane_frame[k];
  return RT;
}

// Device copy of odk_reward_terms, filled by the host: soft joint limits and the robot's global_linvel sensor address resolved there
struct XTerms {
  float scale[ODK_NXTERM];
  float base_height_target, max_foot_height, air_lo, air_hi;
  int adr_global_linvel, pad[3];
  float soft_lo[MAXU], soft_hi[MAXU], pose_w[MAXU];
};

struct KArgs {
  const DevModel* m;
  DevPRM prm;         // by value (232 bytes of kernel arguments): the grid searches read scalar registers, not 20 dependent loads
  const float* prm_table;
  float* recs;        // [nenv][Rec::SIZE]
  float* first;       // [nenv][Rec::FSIZE]
  const float* dr;    // [nenv][NDR] or null
  const float* action;  // [nenv][nu]
  const float* hfield;  // [nrow][ncol] height-field samples in [0, 1], or null (plane floor)
  float* obs; float* priv; float* reward; float* done; float* trunc; float* metrics;
  float* dbg_lds;     // [nenv][TOTAL] or null: LDS image after the last forward
  int nenv;
  uint32_t seed, env_offset;
  int n_substeps;
  EnvCfg cfg;
  const float* cmd;   // [nenv][cmd_stride] bound commands (odk_batch_bind_commands), or null: sampled ones.  (Last, so that the fields
  int cmd_stride;     // above keep their argument offsets.)  A uniform pointer test: the unbound path only gains a scalar branch
  const XTerms* xt;   // reward-library terms (odk_batch_set_reward_terms), null while every term is off: one uniform pointer test
  float* xmet;        // [nenv][ODK_NXTERM] library metrics (odk_batch_bind_reward_metrics), or null
  const int* imap;    // [nu] imitation joint map (odk_batch_set_imitation_joints): frame joint of actuator u, -1 = not compared
  const int* hslot;   // [nu] Standing's head joints (odk_batch_set_head_joints): posture-command slot 0..3 of actuator u, -1 = not a head joint
  const float* push;  // [nenv][push_stride] bound pushes (odk_batch_bind_pushes): world-frame kick (dvx, dvy) of the next step, or null: the
  int push_stride;    // sampled push.  A uniform pointer test like cmd's, placed behind every older field
};

// DR buffer layout per env
template <class S> struct DRL {
  static constexpr int MASS = 0, IPOS = S::NB, FRL = S::NB + 3, ARM = FRL + S::NU, Q0 = ARM + S::NU, KP = Q0 + S::NU, SIZE = KP + S::NU;
};

__device__ __forceinline__ float i2f(int v) { return __int_as_float(v); }
__device__ __forceinline__ int f2i(float v) { return __float_as_int(v); }
__device__ __forceinline__ float nan_to_num(float x) {
  if (isnan(x)) return 0.0f;
  if (isinf(x)) return x > 0 ? 3.4028234663852886e38f : -3.4028234663852886e38f;
  return x;
}

// Debug image of the env's LDS (parity tests).  Out of line and rolled: unrolled in place, its 79 per-lane 64-bit store
// addresses were hoisted above the substep loop and parked in scratch (158 dwords per lane, ~400 MB of HBM per launch).
template <class S, int G>
__device__ __noinline__ void dump_lds(float* dbg, const float* L, int env, int lane) {
  float* o = dbg + (size_t)env * S::TOTAL;
#pragma unroll 1
  for (int k = lane; k < S::TOTAL; k += G) o[k] = L[k];
}

// Global -> LDS copies of the prologue.  Written as "all loads, then all stores" with compile-time trip counts: as
// `for (i = lane; i < N; i += G) dst[i] = src[i]` every trip was its own load -> s_waitcnt vmcnt(0) -> ds_write round trip
// (~25 serialised global round trips per env step: most of the 40 us a zero-substep launch took).
template <int N, int G> struct G2L {
  static constexpr int T = (N + G - 1) / G;
  float v[T];
  __device__ __forceinline__ void load(const float* __restrict__ src, int lane) {
#pragma unroll
    for (int t = 0; t < T; t++) { const int i = lane + t * G; v[t] = src[i < N ? i : 0]; }
  }
  __device__ __forceinline__ void store(float* dst, int lane) const {
#pragma unroll
    for (int t = 0; t < T; t++) { const int i = lane + t * G; if (i < N) dst[i] = v[t]; }
  }
};

// effective per-env model parameters -> LDS: nominal values from the model, domain-randomised ones (dr != null) on top
template <class S, int G>
struct ParamLoad {
  float q0, mass, arm, frl, kp, ipos, dq0, darm, dfrl;
  int qadr, dadr;
  __device__ __forceinline__ void load(const DevModel* __restrict__ m, const float* __restrict__ dr, int lane) {
    static_assert(S::NQ <= G && S::NV <= G && S::NB <= G && S::NU <= G, "one parameter of each kind per lane");
    const int iq = lane < S::NQ ? lane : 0, ib = lane < S::NB ? lane : 0, iv = lane < S::NV ? lane : 0, iu = lane < S::NU ? lane : 0, i3 = lane < 3 ? lane : 0;
    q0 = m->qpos0[iq];
    mass = dr ? dr[DRL<S>::MASS + ib] : m->body_mass[ib];
    arm = m->dof_armature[iv]; frl = m->dof_frictionloss[iv];
    kp = dr ? dr[DRL<S>::KP + iu] : m->act_kp[iu];
    ipos = dr ? dr[DRL<S>::IPOS + i3] : m->body_ipos[1][i3];
    qadr = m->act_qposadr[iu]; dadr = m->act_dofadr[iu];
    dq0 = dr ? dr[DRL<S>::Q0 + iu] : 0.0f; darm = dr ? dr[DRL<S>::ARM + iu] : 0.0f; dfrl = dr ? dr[DRL<S>::FRL + iu] : 0.0f;
  }
  __device__ __forceinline__ void store(float* L, bool has_dr, int lane) const {
    if (lane < S::NQ) L[S::O_Q0 + lane] = q0;
    if (lane < S::NB) L[S::O_MASS + lane] = mass;
    if (lane < S::NV) { L[S::O_ARM + lane] = arm; L[S::O_FRL + lane] = frl; }
    if (lane < S::NU) L[S::O_KP + lane] = kp;
    if (lane < 3) L[S::O_IPOS1 + lane] = ipos;
    ODK_SYNC();   // the actuated joints' randomised values go on top of the nominal ones written by other lanes
    if (has_dr && lane < S::NU) { L[S::O_Q0 + qadr] = dq0; L[S::O_ARM + dadr] = darm; L[S::O_FRL + dadr] = dfrl; }
    ODK_SYNC();
  }
};
template <class S, int G>
__device__ __forceinline__ void load_params(float* L, const DevModel* m, const float* dr, int lane) {
  ParamLoad<S, G> p;
  p.load(m, dr, lane);
  p.store(L, dr != nullptr, lane);
}

// PolyReferenceMotion.get_reference_motion (reference poly_reference_motion.py:148-168): float32 fma Horner
__device__ __forceinline__ int prm_nearest(const float* grid, int n, float v) {   // grid: kernel-argument array, fully unrolled
  int best = 0;
  float bd = fabsf(grid[0] - v);
#pragma unroll
  for (int i = 1; i < 16; i++) { const float d = fabsf(grid[i] - v); if (i < n && d < bd) { bd = d; best = i; } }
  return best;
}
template <int G>
__device__ __forceinline__ void prm_eval(const DevPRM* __restrict__ p, const float* table, float dx, float dy, float dth, int i, float* out, int lane) {
  const float x = fminf(fmaxf(dx, p->ranges[0]), p->ranges[1]);
  const float y = fminf(fmaxf(dy, p->ranges[2]), p->ranges[3]);
  const float t3 = fminf(fmaxf(dth, p->ranges[4]), p->ranges[5]);
  const int ix = prm_nearest(p->dxs, p->nx, x), iy = prm_nearest(p->dys, p->ny, y), it = prm_nearest(p->dths, p->nth, t3);
  float t = (float)(i % p->nsteps) / (float)p->nsteps;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  const float* c = table + ((size_t)((ix * p->ny + iy) * p->nth + it)) * 640;
  for (int k = lane; k < 40; k += G) {
    float yv = c[k * 16];
#pragma unroll
    for (int q = 1; q < 16; q++) yv = fmaf(yv, t, c[k * 16 + q]);
    out[k] = yv;
  }
}
// the same evaluation into two registers per lane (dims lane and lane + 32; G = 32 or 64): the step kernel evaluates the
// reference motion in its prologue, where the table loads overlap the state loads, and parks it in LDS only in the epilogue
template <int G>
__device__ __forceinline__ void prm_eval_regs(const DevPRM* p, const float* table, float dx, float dy, float dth, int i, float& r0, float& r1, int lane) {
  const float x = fminf(fmaxf(dx, p->ranges[0]), p->ranges[1]);
  const float y = fminf(fmaxf(dy, p->ranges[2]), p->ranges[3]);
  const float t3 = fminf(fmaxf(dth, p->ranges[4]), p->ranges[5]);
  const int ix = prm_nearest(p->dxs, p->nx, x), iy = prm_nearest(p->dys, p->ny, y), it = prm_nearest(p->dths, p->nth, t3);
  float t = (float)(i % p->nsteps) / (float)p->nsteps;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  const float* c = table + ((size_t)((ix * p->ny + iy) * p->nth + it)) * 640;
  const int k0 = lane < 40 ? lane : 0, k1 = lane + 32 < 40 ? lane + 32 : 0;
  float a = c[k0 * 16], b = c[k1 * 16];
#pragma unroll
  for (int q = 1; q < 16; q++) { a = fmaf(a, t, c[k0 * 16 + q]); b = fmaf(b, t, c[k1 * 16 + q]); }
  r0 = a; r1 = b;
}

// sample_command (joystick.py:671-725); draws base..base+7 of stream (k0,k1,ctr)
__device__ inline void sample_command(const EnvCfg& c, uint32_t k0, uint32_t k1, uint32_t ctr, uint32_t base, int k, float& out) {
  const float z = rng_uniform(k0, k1, ctr, base + 7);
  const float u = rng_uniform(k0, k1, ctr, base + k);
  out = (z < 0.1f) ? 0.0f : c.cmd_range[k][0] + u * (c.cmd_range[k][1] - c.cmd_range[k][0]);
}

// Draws 4 .. 3 + NDRAW of stream (k0, k1, ctr) in ONE threefry evaluation: lane l < NDRAW / 2 computes block l + 2, whose two words are
// draws 4 + 2 l and 5 + 2 l; NZ[i - 4] = draw i.  (The observation noise and the command resampling used to call the
// generator from inside divergent branches: ~8 serial threefry evaluations per env step.)
template <int NDRAW>
__device__ __forceinline__ void draw_block(uint32_t k0, uint32_t k1, uint32_t ctr, float* NZ, int lane) {
  uint32_t a, b;
  threefry2x32(k0, k1, ctr, (uint32_t)(lane + 2), a, b);
  if (lane < NDRAW / 2) { NZ[2 * lane] = (float)(a >> 8) * (1.0f / 16777216.0f); NZ[2 * lane + 1] = (float)(b >> 8) * (1.0f / 16777216.0f); }
  ODK_SYNC();
}

// _get_obs (joystick.py:487-620 / standing.py:524-565): builds privileged_state (whose first nobs entries are `state`) in LDS by ONE gather
// over DevModel::obs_tab (built at model load by build_obs_table, below: the layouts are written down there).  Element ks of the task's layout is
//   ((L[a] + (b >= 0 ? L[b] : zero)) + noise) - kc) * scale
// with the entry's LDS offsets a, b, its constant kc, its draw and noise scale, `scale` = dof_vel_scale for a joint velocity and 1 elsewhere.  An
// entry without a second offset adds -0, one without a constant subtracts +0, one without noise adds -0 * 1, one without a scale multiplies by 1:
// each leaves every float as it is, so an element goes through the operations its own expression has, in that order.  The values the epilogue
// holds in registers (foot contacts, imitation counter, imitation phase) are parked in the solver-diagnostic slots S_MISC + 1..5, which nobody
// reads after the last forward pass.  NZ: draw_block (read only when `noisy`, i.e. noise_level != 0).
template <class S, int G>
__device__ __forceinline__ void build_obs(float* L, const DevModel* m, const EnvCfg& c, const float* contact, const float* NZ,
                          int imitation_i, const float* phase, bool noisy, int lane) {
  using E = EnvL<S>;
  float* P = L + E::O_PRIV; float* INFO = L + E::O_INFO; float* SCR = L + S::O_SCR;
  const float lvl = c.noise_level;
  constexpr int NU = S::NU;
  constexpr RecLay RL = rec_lay(NU);
  constexpr int NT = (obs_npriv(NU, false) + G - 1) / G;   // passes of the longer layout (Joystick's)
  static_assert(13 + NU <= G, "build_obs: the noisy joint angles (elements 13 .. 12 + nu) must lie in the first pass of G elements: nu <= G - 13 (see MAXU in odk_model.h)");
  const ObsEnt* T = m->obs_tab[c.kind != 0 ? 1 : 0];
  const int np = c.npriv;
  ObsEnt ent[NT];   // every pass' entry up front: the loads are in flight together
#pragma unroll
  for (int it = 0; it < NT; it++) { const int ks = lane + it * G; ent[it] = T[ks < np ? ks : 0]; }
  // imu history ring (noisy gravity, never emitted: joystick.py:522-530)
  float ng = 0;
  if (lane < 3) { ng = SCR[S::S_MISC + 10 + lane]; if (noisy) ng = ng + (2.0f * NZ[10 - 4 + lane] - 1.0f) * lvl * c.noise_gravity; }
  float h0 = 0, h1 = 0;
  if (lane < 3) { h0 = INFO[RL.IMU + lane]; h1 = INFO[RL.IMU + 3 + lane]; }
  if (lane == 0) {
    SCR[S::S_MISC + OBS_PARK_CON] = contact[0]; SCR[S::S_MISC + OBS_PARK_CON + 1] = contact[1]; SCR[S::S_MISC + OBS_PARK_IMI] = (float)imitation_i;
    SCR[S::S_MISC + OBS_PARK_PHASE] = phase[0]; SCR[S::S_MISC + OBS_PARK_PHASE + 1] = phase[1];
  }
  ODK_SYNC();
  if (lane < 3) { INFO[RL.IMU + lane] = ng; INFO[RL.IMU + 3 + lane] = h0; INFO[RL.IMU + 6 + lane] = h1; }
#pragma unroll
  for (int it = 0; it < NT; it++) {
    const int ks = lane + it * G;
    if (ks >= np) continue;
    const ObsEnt e = ent[it];
    const float second = L[e.b >= 0 ? e.b : 0];
    float v = L[e.a] + (e.b >= 0 ? second : ((e.fl & OBS_FL_PLUS0) ? 0.0f : -0.0f));
    if (noisy) {
      const int slot = e.fl & 255, nk = (e.fl >> 8) & 31;
      float nq = 0.0f;   // the joint-angle scale of the element's actuator, picked by compile-time indices (a lane-dependent index into the
                         // kernel arguments would park all of them in scratch); the noisy joint angles are elements 13 .. 12 + nu: the first pass
      if (it == 0) {
#pragma unroll
        for (int u = 0; u < NU; u++) nq = nk - 3 == u ? c.qpos_noise_scale[u] : nq;
      }
      const float ns = nk == 0 ? c.noise_gyro : (nk == 1 ? c.noise_accelerometer : (nk == 2 ? c.noise_joint_vel : nq));
      const float t = (2.0f * NZ[slot ? slot - 1 : 0] - 1.0f) * lvl;
      v = v + (slot ? t : -0.0f) * (slot ? ns : 1.0f);
    }
    v = v - e.kc;
    v = v * ((e.fl & OBS_FL_VEL) ? c.dof_vel_scale : 1.0f);
    P[ks] = v;
  }
  ODK_SYNC();
}

__device__ __forceinline__ void foot_contact_flags(const float* CDIST, float* contact) {
  for (int f = 0; f < 2; f++) {
    float md = 1e4f;
    for (int k = 0; k < 4; k++) md = fminf(md, CDIST[4 * f + k]);
    contact[f] = md < 0 ? 1.0f : 0.0f;
  }
}

template <class S, int G>
__device__ __forceinline__ void write_outputs(const KArgs& a, const float* L, int env, float reward, float done, float trunc, const float* metrics, int lane) {
  using E = EnvL<S>;
  const float* P = L + E::O_PRIV;
  const int nobs = a.cfg.nobs, npriv = a.cfg.npriv;
  if (a.obs) for (int k = lane; k < nobs; k += G) a.obs[(size_t)env * nobs + k] = P[k];
  if (a.priv) for (int k = lane; k < npriv; k += G) a.priv[(size_t)env * npriv + k] = P[k];
  if (lane == 0) {
    if (a.reward) a.reward[env] = reward;
    if (a.done) a.done[env] = done;
    if (a.trunc) a.trunc[env] = trunc;
  }
  if (a.metrics && lane < ODK_NMETRIC) a.metrics[(size_t)env * ODK_NMETRIC + lane] = metrics[lane];
}

// Reward-library terms (reference common/rewards.py; include/odk.h odk_xterm): called under the uniform test of a.xt, in the step's
// epilogue, with every input in LDS (sensors, qpos / qvel, actuator forces, feet site z of the last forward pass) or in registers
// (contact, air time after += dt, swing peak after this step's max, first_contact bits, termination).  Adds the scaled terms to
// `total` in term order, after the native seven, and writes their metrics (lane 0 of a live env).
template <class S, int G>
__device__ __forceinline__ void reward_library(const KArgs& a, const float* L, const DevModel* mp, const float* contact, const float* air,
                                               const float* peak, int fc_bits, bool done_env, float& total, int env, bool live, int lane) {
  using E = EnvL<S>;
  constexpr int NU = S::NU;
  constexpr RecLay RL = rec_lay(NU);
  static_assert(NU <= MAXU, "XTerms holds MAXU actuators");
  const XTerms* xt = a.xt;
  const float* SENS = L + S::O_SENS; const float* QPOS = L + S::O_QPOS; const float* QVEL = L + S::O_QVEL;
  const float* cmd = L + E::O_INFO + RL.CMD;
  // per-actuator sums: energy, joint_pos_limits, pose (lanes 0..NU-1)
  float v[3] = {0.0f, 0.0f, 0.0f};
  if (lane < NU) {
    const int u = lane;
    const float jq = QPOS[mp->act_qposadr[u]], jv = QVEL[mp->act_dofadr[u]], af = L[S::O_ACTF + u];
    v[0] = fabsf(jv) * fabsf(af);
    v[1] = -fminf(jq - xt->soft_lo[u], 0.0f) + fmaxf(jq - xt->soft_hi[u], 0.0f);
    const float dp = jq - mp->key_ctrl[u];
    v[2] = dp * dp * xt->pose_w[u];
  }
  gsum_n<G, 3>(v);
  float r[ODK_NXTERM];
  const float* gl = SENS + xt->adr_global_linvel;
  const float* ga = SENS + mp->adr_global_angvel;
  const float* up = SENS + mp->adr_upvector;
  r[ODK_XTERM_LIN_VEL_Z] = nan_to_num(gl[2] * gl[2]);
  r[ODK_XTERM_ANG_VEL_XY] = nan_to_num(ga[0] * ga[0] + ga[1] * ga[1]);
  r[ODK_XTERM_ORIENTATION] = nan_to_num(up[0] * up[0] + up[1] * up[1]);
  const float dh = QPOS[2] - xt->base_height_target;
  r[ODK_XTERM_BASE_HEIGHT] = nan_to_num(dh * dh);
  r[ODK_XTERM_ENERGY] = nan_to_num(v[0]);
  r[ODK_XTERM_JOINT_POS_LIMITS] = nan_to_num(v[1]);
  r[ODK_XTERM_TERMINATION] = done_env ? 1.0f : 0.0f;
  r[ODK_XTERM_POSE] = nan_to_num(v[2]);
  const float maxh = xt->max_foot_height, tmin = xt->air_lo, tmax = xt->air_hi;
  float slip = 0.0f, clear = 0.0f, height = 0.0f, airt = 0.0f;
#pragma unroll
  for (int f = 0; f < 2; f++) {
    const float* fv = SENS + mp->adr_foot_linvel[f];
    const float fc = ((fc_bits >> f) & 1) ? 1.0f : 0.0f;
    slip += sqrtf(fv[0] * fv[0] + fv[1] * fv[1] + fv[2] * fv[2]) * contact[f];
    clear += fabsf(L[S::O_SCR + S::S_MISC + 8 + f] - maxh) * sqrtf(sqrtf(fv[0] * fv[0] + fv[1] * fv[1]));
    const float he = peak[f] / maxh - 1.0f;
    height += he * he * fc;
    airt += fminf((air[f] - tmin) * fc, tmax - tmin);
  }
  const float cn = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1] + cmd[2] * cmd[2]);
  r[ODK_XTERM_FEET_SLIP] = nan_to_num(slip);
  r[ODK_XTERM_FEET_CLEARANCE] = nan_to_num(clear);
  r[ODK_XTERM_FEET_HEIGHT] = nan_to_num(height);
  r[ODK_XTERM_FEET_AIR_TIME] = nan_to_num(airt * (cn > 0.01f ? 1.0f : 0.0f));
#pragma unroll
  for (int k = 0; k < ODK_NXTERM; k++) {
    const float sc = xt->scale[k], t = r[k] * sc;
    total += t;
    r[k] = sc > 0 ? t : -t;
  }
  if (a.xmet && live && lane == 0) {
    float* o = a.xmet + (size_t)env * ODK_NXTERM;
#pragma unroll
    for (int k = 0; k < ODK_NXTERM; k++) o[k] = r[k];
  }
}

// ================================================================================================
// Joystick.reset (joystick.py:206-321) + Episode/AutoReset wrapper resets
template <class S, int G, int HF>
__global__ void __launch_bounds__(64) reset_kernel(KArgs a) {
  extern __shared__ float lds[];
  using E = EnvL<S>; using R = Rec<S>;
  constexpr int NU = S::NU;
  constexpr RecLay RL = rec_lay(NU);
  const int slot = threadIdx.x / G, lane = threadIdx.x % G;
  const int env = blockIdx.x * (64 / G) + slot;
  const bool live = env < a.nenv;
  const int e = live ? env : a.nenv - 1;
  float* L = lds + slot * E::TOTAL;
  const int* RT = load_shared<S>(lds, 64 / G, a.m);   // ordered before its first use by the ODK_SYNCs below
#ifdef ODK_POISON_LDS   // debug build: every read of LDS that was not written by this launch surfaces as NaN
  for (int k = lane; k < E::TOTAL; k += G) L[k] = __int_as_float(0x7fc00000);
  ODK_SYNC();
#endif
  const DevModel* m = a.m;
  const EnvCfg& c = a.cfg;
  float* INFO = L + E::O_INFO;
  load_params<S, G>(L, m, a.dr ? a.dr + (size_t)e * DRL<S>::SIZE : nullptr, lane);
  Statics<S, G> st;
  load_statics<S, G>(st, m, lane);
  uint32_t k0, k1;
  threefry2x32(a.seed, 0x4F444B31u, a.env_offset + (uint32_t)e, 0u, k0, k1);
  const uint32_t kr = k1 ^ 0x52535421u;
  for (int i = lane; i < S::NQ; i += G) L[S::O_QPOS + i] = m->key_qpos[i];
  for (int i = lane; i < S::NV; i += G) { L[S::O_QVEL + i] = 0; L[S::O_WARM + i] = 0; }
  for (int i = lane; i < S::N_INFO; i += G) INFO[i] = 0;
  ODK_SYNC();
  if (lane < 2) L[S::O_QPOS + lane] += -0.05f + rng_uniform(k0, kr, 0, lane) * 0.1f;
  if (lane == 2) {
    const float yaw = -3.14f + rng_uniform(k0, kr, 0, 2) * 6.28f;
    float s, co;
    sincosf(0.5f * yaw, &s, &co);
    float q0[4] = {L[S::O_QPOS + 3], L[S::O_QPOS + 4], L[S::O_QPOS + 5], L[S::O_QPOS + 6]}, qz[4] = {co, 0, 0, s}, r[4];
    qmul(r, q0, qz);
    for (int k = 0; k < 4; k++) L[S::O_QPOS + 3 + k] = r[k];
  }
  if (lane >= 3 && lane < 9) L[S::O_QVEL + lane - 3] = -c.reset_base_qvel + rng_uniform(k0, kr, 0, 3 + NU + lane - 3) * (2.0f * c.reset_base_qvel);
  for (int u = lane; u < S::NU; u += G) {
    const float v = L[S::O_QPOS + m->act_qposadr[u]] * (0.5f + rng_uniform(k0, kr, 0, 3 + u));
    L[S::O_QPOS + m->act_qposadr[u]] = v;
    L[S::O_CTRL + u] = v;
    INFO[RL.MT + u] = c.kind != 0 ? 0.0f : m->key_ctrl[u];   // standing.py:279 starts from zeros
  }
  if (lane < 7) {   // a bound row replaces the stored value only: the draw is made all the same (the reset stream stays the unbound one)
    float v;
    sample_command(c, k0, kr, 0, 9 + NU, lane, v);
    if (a.cmd) v = a.cmd[(size_t)e * a.cmd_stride + lane];
    INFO[RL.CMD + lane] = v;
  }
  ODK_SYNC();
  forward_env<S, G, HF>(L, RT, m, a.hfield, st, lane, 1);
  if (a.dbg_lds && live) dump_lds<S, G>(a.dbg_lds, L, env, lane);
  const float pint = c.push_interval_range[0] + rng_uniform(k0, kr, 0, 17 + NU) * (c.push_interval_range[1] - c.push_interval_range[0]);
  const int push_interval_steps = (int)rintf(pint / c.ctrl_dt);
  if (c.use_imitation) prm_eval<G>(&a.prm, a.prm_table, INFO[RL.CMD], INFO[RL.CMD + 1], INFO[RL.CMD + 2], 0, L + E::O_REF, lane);
  else for (int k = lane; k < 40; k += G) L[E::O_REF + k] = 0;
  ODK_SYNC();
  float contact[2];
  foot_contact_flags(L + S::O_CDIST, contact);
  const float phase[2] = {0, 0};
  // stash state before the obs overwrites the M|HL region?  (qpos/qvel/warm live elsewhere: safe)
  draw_block<E::NDRAW>(k0, k1, 0u, L + E::O_NZ, lane);   // the motion-column buffers are dead after the forward pass
  build_obs<S, G>(L, m, c, contact, L + E::O_NZ, 0, phase, c.noise_level != 0.0f, lane);
  if (lane == 0) {
    INFO[RL.KEY0] = i2f((int)k0); INFO[RL.KEY1] = i2f((int)k1); INFO[RL.CTR] = i2f(1);
    INFO[RL.STEP] = i2f(0); INFO[RL.PSTEP] = i2f(0); INFO[RL.PINT] = i2f(push_interval_steps);
    INFO[RL.IMI] = i2f(0); INFO[RL.LCON] = i2f(0);
  }
  ODK_SYNC();
  if (live) {
    float* rc = a.recs + (size_t)env * R::SIZE;
    float* fs = a.first + (size_t)env * R::FSIZE;
    for (int i = lane; i < S::NQ; i += G) { rc[i] = L[S::O_QPOS + i]; fs[i] = L[S::O_QPOS + i]; }
    for (int i = lane; i < S::NV; i += G) {
      rc[S::NQ + i] = L[S::O_QVEL + i]; fs[S::NQ + i] = L[S::O_QVEL + i];
      rc[S::NQ + S::NV + i] = L[S::O_WARM + i]; fs[S::NQ + S::NV + i] = L[S::O_WARM + i];
    }
    for (int k = lane; k < R::NPRIV; k += G) {
      if (k < R::NOBS) fs[R::FOBS + k] = L[E::O_PRIV + k];
      fs[R::FOBS + R::NOBS + k] = L[E::O_PRIV + k];
    }
    for (int k = lane; k < RL.NINFO; k += G) rc[R::INFO + k] = INFO[k];
    float metrics[ODK_NMETRIC] = {0, 0, 0, 0, 0, 0, 0, 0};
    write_outputs<S, G>(a, L, env, 0.0f, 0.0f, 0.0f, metrics, lane);
    if (a.xmet && lane < ODK_NXTERM) a.xmet[(size_t)env * ODK_NXTERM + lane] = 0.0f;
  }
}

// ================================================================================================
// AutoReset.step -> Episode.step -> Joystick.step (joystick.py:323-481), all substeps fused
constexpr int STEP_WAVES = 2;     // waves per SIMD the register allocation is held to (3 and 4 spill and run slower: profiles/r5/NOTES.md)
// DBG: the instantiation that fills the debug image (a.dbg_lds: odk_set_debug_dump(1)): forward_env's debug-only stores are compiled in
// and the image is dumped after the last forward pass; the product instantiation (DBG = false) has neither.  The profile build times the
// product instruction stream and reads its counters through the image: its DBG = false kernel keeps the dump.
#ifdef ODK_PROFILE
constexpr bool STEP_DUMPS_ALWAYS = true;
#else
constexpr bool STEP_DUMPS_ALWAYS = false;
#endif
template <class S, int G, int HF, bool DBG>
__device__ __forceinline__ void step_body(const KArgs& a) {
  extern __shared__ float lds[];
  using E = EnvL<S>; using R = Rec<S>;
  constexpr int NU = S::NU;
  constexpr RecLay RL = rec_lay(NU);
  const int slot = threadIdx.x / G, lane = threadIdx.x % G;
  const int env = blockIdx.x * (64 / G) + slot;
  const bool live = env < a.nenv;
  const int e = live ? env : a.nenv - 1;
  float* L = lds + slot * E::TOTAL;
#ifdef ODK_PROFILE
  const long long t_k0 = clock64();   // kernel-level stamps (profile build): prologue / substeps / epilogue pieces -> S_PROF slots 18, 19 + dbg tail
#endif
  const int* RT = load_shared<S>(lds, 64 / G, a.m);   // ordered before its first use by the ODK_SYNCs below
#ifdef ODK_POISON_LDS   // debug build: every read of LDS that was not written by this launch surfaces as NaN
  for (int k = lane; k < E::TOTAL; k += G) L[k] = __int_as_float(0x7fc00000);
  ODK_SYNC();
#endif
  const DevModel* m = a.m;
  const EnvCfg& c = a.cfg;
  float* INFO = L + E::O_INFO; float* ACT = L + E::O_ACT; float* CTRL = L + S::O_CTRL;
  float* rc = a.recs + (size_t)e * R::SIZE;
  // ---- state record, action, parameters, per-lane statics: ONE batch of global loads (coalesced: the group's lanes read
  // consecutive floats), then the LDS stores
  {
    G2L<S::NQ + 2 * S::NV, G> g_state;   // qpos|qvel|warm are contiguous in LDS too
    G2L<RL.NINFO, G> g_info;
    G2L<NU, G> g_act;
    ParamLoad<S, G> g_par;
    const float* drp = a.dr ? a.dr + (size_t)e * DRL<S>::SIZE : nullptr;
    g_state.load(rc, lane); g_info.load(rc + R::INFO, lane); g_act.load(a.action + (size_t)e * NU, lane);
    g_par.load(m, drp, lane);
    g_state.store(L + S::O_QPOS, lane); g_info.store(INFO, lane); g_act.store(ACT, lane);
    g_par.store(L, drp != nullptr, lane);   // syncs
  }
  if (a.cmd) {   // bound commands: env e's row, read before the reference motion, the reward and the observation use info["command"]
    if (lane < 7) INFO[RL.CMD + lane] = a.cmd[(size_t)e * a.cmd_stride + lane];
    ODK_SYNC();
  }
#ifdef ODK_PROFILE
  for (int k = lane; k < 36; k += G) L[S::O_SCR + S::S_PROF + k] = 0;
#endif
  Statics<S, G> st;
  load_statics<S, G>(st, m, lane);
  const uint32_t k0 = (uint32_t)f2i(INFO[RL.KEY0]), k1 = (uint32_t)f2i(INFO[RL.KEY1]), ctr = (uint32_t)f2i(INFO[RL.CTR]);
  int step = f2i(INFO[RL.STEP]), push_step = f2i(INFO[RL.PSTEP]);
  const int push_int = f2i(INFO[RL.PINT]);
  int imi = f2i(INFO[RL.IMI]);
  const int lcon = f2i(INFO[RL.LCON]);
  const float prev_done = INFO[RL.DONE];
  float ep_steps = prev_done != 0.0f ? 0.0f : INFO[RL.EPSTEPS];  // AutoReset.step prologue
  const float dt = c.ctrl_dt;
  // ---- imitation phase + reference motion (:325-355)
  float phase[2] = {0, 0};
  float ref0 = 0.0f, ref1 = 0.0f;   // current_reference_motion[lane], [lane + 32]: two registers across the substeps
  if (c.use_imitation) {
    imi = (imi + 1) % a.prm.nsteps;
    const float ph = ((float)imi / (float)a.prm.nsteps) * 2.0f * PI_F;
    phase[0] = cosf(ph); phase[1] = sinf(ph);
    prm_eval_regs<G>(&a.prm, a.prm_table, INFO[RL.CMD], INFO[RL.CMD + 1], INFO[RL.CMD + 2], imi, ref0, ref1, lane);   // (:347-353)
  } else {
    imi = 0;
  }
  // ---- action delay ring (:362-376): roll by nu, newest first
  float h0 = 0, h1 = 0;
  for (int u = lane; u < NU; u += G) { h0 = INFO[RL.AHIST + u]; h1 = INFO[RL.AHIST + NU + u]; }
  ODK_SYNC();
  for (int u = lane; u < NU; u += G) { INFO[RL.AHIST + u] = ACT[u]; INFO[RL.AHIST + NU + u] = h0; INFO[RL.AHIST + 2 * NU + u] = h1; }
  ODK_SYNC();
  uint32_t w0, w1, w2, w3;   // draws 0 | 1 (unused) and 2 | 3: two generator blocks
  threefry2x32(k0, k1, ctr, 0u, w0, w1);
  threefry2x32(k0, k1, ctr, 1u, w2, w3);
  const int aidx = randint3((float)(w0 >> 8) * (1.0f / 16777216.0f));
  // ---- push (:381-398)
  const float theta = (float)(w2 >> 8) * (1.0f / 16777216.0f) * (2.0f * PI_F);
  const float mag = c.push_magnitude_range[0] + (float)(w3 >> 8) * (1.0f / 16777216.0f) * (c.push_magnitude_range[1] - c.push_magnitude_range[0]);
  const float gate = (((push_step + 1) % push_int) == 0 ? 1.0f : 0.0f) * c.push_enable;
  float push[2] = {cosf(theta) * gate, sinf(theta) * gate};
  if (a.push) {   // bound pushes: env e's row is the kick (theta and mag were drawn and are dropped); info["push"] keeps its unit direction
    if (lane < 2) {
      const float* pr = a.push + (size_t)e * a.push_stride;
      const float kx = pr[0], ky = pr[1];
      L[S::O_QVEL + lane] += lane == 0 ? kx : ky;
      const float n2 = kx * kx + ky * ky;
      const float inv = n2 > 0.0f ? 1.0f / sqrtf(n2) : 0.0f;
      push[0] = kx * inv; push[1] = ky * inv;
    }
  } else if (lane < 2) {
    L[S::O_QVEL + lane] += push[lane] * mag;
  }
  // values only the epilogue needs go back to LDS now instead of riding through the substep loop in scratch:
  // info["push"], the imitation counter, its phase (two spare floats behind the action), the episode step counter
  if (lane == 0) {
    INFO[RL.PUSH] = push[0]; INFO[RL.PUSH + 1] = push[1];
    INFO[RL.IMI] = i2f(imi);
    ACT[NU] = phase[0]; ACT[NU + 1] = phase[1];
    INFO[RL.EPSTEPS] = ep_steps;
  }
  // ---- motor targets with speed limit (:404-417)
  for (int u = lane; u < NU; u += G) {
    float mt = m->key_ctrl[u] + INFO[RL.AHIST + aidx * NU + u] * c.action_scale;
    if (c.use_motor_speed_limits) {
      const float prev = INFO[RL.MT + u], lim = c.max_motor_velocity * dt;
      mt = fminf(fmaxf(mt, prev - lim), prev + lim);
    }
    CTRL[u] = mt;
  }
  ODK_SYNC();
#ifdef ODK_PROFILE
  const long long t_k1 = clock64();
  if (lane == 0) L[S::O_SCR + S::S_PROF + 18] = (float)(t_k1 - t_k0);
#endif
  // ---- mjx_env.step: n_substeps x (forward + Euler)   (:420)
  HotSt hot;
  if constexpr (HF == 0) load_hot<S, G>(hot, m, st, lane);
  for (int s = 0; s < a.n_substeps; s++) {
    const bool last = s == a.n_substeps - 1;
    // The model pointer is made opaque once per substep: the per-lane 64-bit table addresses (and loop-invariant table
    // loads) would otherwise be hoisted out of the loop and, with 256 VGPRs taken, parked in scratch -- ~150 dwords per
    // lane, private per wave, evicted to HBM (hundreds of MB per launch) -- while recomputing an address is one VALU op
    // and the tables themselves are 60 KB shared by every wave (L1 / L2 resident).  (Still a win with ~60 VGPRs free: -6 % without
    // the opaque pointer, -1 % without the opaque lane id -- the hoisted values lengthen live ranges, the loads they save are covered.)
    size_t opaque0 = 0;
    asm volatile("" : "+s"(opaque0));   // an offset, not the pointer itself: the address space (global) stays known
    const DevModel* ms = reinterpret_cast<const DevModel*>(reinterpret_cast<const char*>(m) + opaque0);
    // ... and so is the lane id: every lane-derived LDS address and predicate is a handful of VALU ops to rebuild, while
    // hoisted above the loop they sat in scratch (the range assumption keeps the 24-bit multiply / known-bits folds)
    int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    __builtin_assume(lane_s >= 0 && lane_s < 64);
    if constexpr (HF == 0) forward_env<S, G, HF, true, DBG>(L, RT, ms, a.hfield, st, lane_s, last ? 1 : 0, hot);
    else forward_env<S, G, HF, false, DBG>(L, RT, ms, a.hfield, st, lane_s, last ? 1 : 0);
    if constexpr (DBG || STEP_DUMPS_ALWAYS) {
      if (last && a.dbg_lds && live) dump_lds<S, G>(a.dbg_lds, L, env, lane);
    }
    euler_env<S, G>(L, ms, st, lane_s);
  }
#ifdef ODK_PROFILE
  const long long t_k2 = clock64();
#endif
  // same trick for the epilogue: its table addresses would otherwise be shared (CSE) with the prologue's and carried
  // across the substep loop in scratch
  size_t opaque1 = 0;
  asm volatile("" : "+s"(opaque1));
  const DevModel* mp = reinterpret_cast<const DevModel*>(reinterpret_cast<const char*>(m) + opaque1);
  // ... and for the RNG key / counter: everything derived from them (threefry key schedules of the observation-noise
  // draws) is recomputed here instead of riding through the loop in scratch
  const uint32_t k0e = (uint32_t)f2i(INFO[RL.KEY0]), k1e = (uint32_t)f2i(INFO[RL.KEY1]), ctre = (uint32_t)f2i(INFO[RL.CTR]);
  const int imi_e = f2i(INFO[RL.IMI]);
  const float phase_e[2] = {ACT[NU], ACT[NU + 1]};
  int step_e = f2i(INFO[RL.STEP]), push_step_e = f2i(INFO[RL.PSTEP]);
  float ep_steps_e = INFO[RL.EPSTEPS];
  const float prev_done_e = INFO[RL.DONE];
  for (int u = lane; u < NU; u += G) INFO[RL.MT + u] = CTRL[u];  // info["motor_targets"] (:422)
  // This step's draws 4 .. 3 + NDRAW feed the observation noise (every one scaled by noise_level) and, on a step that resamples a
  // sampled command, the new command.  With noise off and no env of the wave resampling, nobody reads them: the generator block and the
  // noise terms of the observation are skipped (a wave-uniform test; the key and the counter advance below as ever, so a run that turns
  // noise on later draws from the same stream).  An exact-zero observation keeps its sign where the zero noise term made it +0.
  const bool noisy = c.noise_level != 0.0f;
  const bool resamples = !a.cmd && step_e + 1 > 500;
  if (noisy || __builtin_amdgcn_ballot_w64(resamples) != 0)
    draw_block<E::NDRAW>(k0e, k1e, ctre, L + E::O_NZ, lane);   // the motion-column buffers are dead after the last forward pass
  // reference motion of this step: evaluated in the prologue, parked here (reward and privileged obs are its only readers)
  if (lane < 40) L[E::O_REF + lane] = ref0;
  if (lane < 8) L[E::O_REF + 32 + lane] = ref1;
  ODK_SYNC();
  // ---- contacts, air time, swing peak (:424-435)
  float contact[2];
  foot_contact_flags(L + S::O_CDIST, contact);
  float air[2], peak[2];
  for (int f = 0; f < 2; f++) {
    air[f] = INFO[RL.AIR + f] + dt;
    peak[f] = fmaxf(INFO[RL.PEAK + f], L[S::O_SCR + S::S_MISC + 8 + f]);
  }
  int fc_bits = 0;   // first_contact (:430-431) for the reward library, from the air time before its increment is stored below
  if (a.xt) {
    const int lc = f2i(INFO[RL.LCON]);
    for (int f = 0; f < 2; f++) fc_bits |= (INFO[RL.AIR + f] > 0.0f && (contact[f] != 0.0f || ((lc >> f) & 1))) ? 1 << f : 0;
  }
  ODK_SYNC();
  if (lane < 2) INFO[RL.AIR + lane] = air[lane];
  ODK_SYNC();
  // ---- termination (:483-485)
  float nanflag = 0;
  for (int i = lane; i < S::NQ + S::NV; i += G) nanflag += isnan(L[S::O_QPOS + i]) ? 1.0f : 0.0f;
  nanflag = gsum<G>(nanflag);
  const bool done_env = (L[S::O_SENS + mp->adr_upvector + 2] < 0.0f) || nanflag > 0;
  // ---- rewards (:622-669, :440-447); lanes 0..NU-1 hold the per-actuator terms
  float t_tq = 0, t_ar = 0, t_pose = 0, t_vel = 0, t_jp = 0, t_jv = 0;
  const float* REF = L + E::O_REF;
  if (lane < NU) {
    const int u = lane;
    const float jq = L[S::O_QPOS + mp->act_qposadr[u]], jv = L[S::O_QVEL + mp->act_dofadr[u]];
    const float af = L[S::O_ACTF + u];
    t_tq = af * af;
    const float da = ACT[u] - INFO[RL.LAST + u];
    t_ar = da * da;
    int hs = -1;   // Standing: the posture-command slot of this actuator through the batch's head map (the duck's: actuators 5..8 -> slots
                   // 0..3), -1 for a leg.  Loaded under the wave-uniform task test, at the epilogue's opaque offset like the imitation map's
    if (c.kind != 0) hs = reinterpret_cast<const int*>(reinterpret_cast<const char*>(a.hslot) + opaque1)[u];
    const bool counted = hs < 0;   // Standing: cost_stand_still(..., ignore_head=True) (standing.py:590-597); Joystick: every actuator
    t_pose = counted ? fabsf(jq - mp->key_ctrl[u]) : 0.0f;
    t_vel = counted ? fabsf(jv) : 0.0f;
    if (hs >= 0) { const float dh = jq - INFO[RL.CMD + 3 + hs]; t_jp = dh * dh; }   // cost_head_pos (rewards.py:131-147)
    if (c.kind == 0 && c.use_imitation) {   // joints vs the frame's joints through the batch's map (custom_rewards.py:80-88; the duck's:
                                            // joints[:5] ++ joints[9:] vs ref[:5] ++ ref[11:16]).  Its address rides on the epilogue's opaque
                                            // offset: the load stays here instead of being hoisted above the substep loop
      const int ri = reinterpret_cast<const int*>(reinterpret_cast<const char*>(a.imap) + opaque1)[u];
      if (ri >= 0) {
        const float dp = jq - REF[ri], dv = jv - REF[16 + ri];
        t_jp = dp * dp; t_jv = dv * dv;
      }
    }
  }
  t_tq = gsum<G>(t_tq); t_ar = gsum<G>(t_ar); t_pose = gsum<G>(t_pose); t_vel = gsum<G>(t_vel); t_jp = gsum<G>(t_jp); t_jv = gsum<G>(t_jv);
  float rew[7];
  {
    const float* cmd = INFO + RL.CMD;
    const float* lv = L + S::O_SENS + mp->adr_local_linvel;
    const float* gy = L + S::O_SENS + mp->adr_gyro;
    const float ex = (cmd[0] - lv[0]) * (cmd[0] - lv[0]);
    const float ey = fmaxf(fabsf(lv[1] - cmd[1]) - 0.1f, 0.0f);
    rew[0] = nan_to_num(expf(-(ex + ey * ey) / c.tracking_sigma));
    const float ea = (cmd[2] - gy[2]) * (cmd[2] - gy[2]);
    rew[1] = nan_to_num(expf(-ea / c.tracking_sigma));
    rew[2] = nan_to_num(t_tq);
    rew[3] = nan_to_num(t_ar);
    const float cn = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1] + cmd[2] * cmd[2]);
    if (c.kind != 0) {   // standing.py:585-606: cost_orientation(upvector), cost_head_pos (gated by the MOVE command norm)
      const float* up = L + S::O_SENS + mp->adr_upvector;
      rew[0] = nan_to_num(up[0] * up[0] + up[1] * up[1]);
      rew[1] = nan_to_num(t_jp) * (cn > 0.01f ? 1.0f : 0.0f);
    }
    rew[4] = nan_to_num(t_pose + t_vel) * (cn < 0.01f ? 1.0f : 0.0f);
    rew[5] = 1.0f;
    rew[6] = 0.0f;
    if (c.use_imitation) {  // custom_rewards.py:4-148
      const float* bv = L + S::O_QVEL;
      const float lin_xy = expf(-8.0f * ((bv[0] - REF[34]) * (bv[0] - REF[34]) + (bv[1] - REF[35]) * (bv[1] - REF[35])));
      const float lin_z = expf(-8.0f * (bv[2] - REF[36]) * (bv[2] - REF[36]));
      const float ang_xy = expf(-2.0f * ((bv[3] - REF[37]) * (bv[3] - REF[37]) + (bv[4] - REF[38]) * (bv[4] - REF[38]))) * 0.5f;
      const float ang_z = expf(-2.0f * (bv[5] - REF[39]) * (bv[5] - REF[39])) * 0.5f;
      float crew = 0;
      for (int f = 0; f < 2; f++) crew += (contact[f] == (REF[32 + f] > 0.5f ? 1.0f : 0.0f)) ? 1.0f : 0.0f;
      float r = lin_xy + lin_z + ang_xy + ang_z - t_jp * 15.0f - t_jv * 1.0e-3f + crew;
      r *= (cn > 0.01f) ? 1.0f : 0.0f;
      rew[6] = nan_to_num(r);
    }
  }
  float total = 0;
  for (int k = 0; k < 7; k++) { rew[k] *= c.reward_scales[k]; total += rew[k]; }
  if (a.xt) reward_library<S, G>(a, L, mp, contact, air, peak, fc_bits, done_env, total, env, live, lane);
  const float reward = fminf(fmaxf(total * dt, 0.0f), 10000.0f);
  // ---- obs (uses the pre-shift last_act and the post-increment air time; :437)
  const float* NZ = L + E::O_NZ;   // this step's draws 4 .. 49 (drawn above, before the reward block)
  build_obs<S, G>(L, mp, c, contact, NZ, imi_e, phase_e, noisy, lane);
  // ---- info updates (:449-469)
  step_e += 1; push_step_e += 1;
  float la = 0, lla = 0;
  for (int u = lane; u < NU; u += G) { la = INFO[RL.LAST + u]; lla = INFO[RL.LAST2 + u]; }
  ODK_SYNC();
  for (int u = lane; u < NU; u += G) { INFO[RL.LAST3 + u] = lla; INFO[RL.LAST2 + u] = la; INFO[RL.LAST + u] = ACT[u]; }
  if (step_e > 500 && lane < 7 && !a.cmd) {   // sample_command (joystick.py:671-725) on draws 13 + 2 nu .. 20 + 2 nu of this step (the duck: 41 .. 48);
                                              // bound: the row read in the prologue stays (the draws were made by draw_block all the same)
    constexpr int DC = draw_cmd(NU) - 4;
    const float z = NZ[DC + 7], u = NZ[DC + lane];
    INFO[RL.CMD + lane] = (z < 0.1f) ? 0.0f : c.cmd_range[lane][0] + u * (c.cmd_range[lane][1] - c.cmd_range[lane][0]);
  }
  if (done_env || step_e > 500) step_e = 0;
  int lcon_new = 0;
  for (int f = 0; f < 2; f++) {
    if (contact[f] != 0.0f) { air[f] = 0; peak[f] = 0; lcon_new |= (1 << f); }
  }
  (void)lcon;
  float metrics[ODK_NMETRIC];
  for (int k = 0; k < 7; k++) metrics[k] = c.reward_scales[k] > 0 ? rew[k] : -rew[k];
  metrics[7] = 0.5f * (peak[0] + peak[1]);
  // ---- EpisodeWrapper.step
  ep_steps_e += 1.0f;
  float done_f = done_env ? 1.0f : 0.0f, trunc = 0.0f;
  if (ep_steps_e >= (float)c.episode_length) { trunc = 1.0f - done_f; done_f = 1.0f; }
  const float keep = 1.0f - prev_done_e;  // info['episode_done'] of the previous step
  ODK_SYNC();
  if (lane == 0) {
    INFO[RL.AIR] = air[0]; INFO[RL.AIR + 1] = air[1]; INFO[RL.PEAK] = peak[0]; INFO[RL.PEAK + 1] = peak[1];
    INFO[RL.EPSTEPS] = ep_steps_e; INFO[RL.TRUNC] = trunc; INFO[RL.DONE] = done_f;
    INFO[RL.EPSUM] = (INFO[RL.EPSUM] + reward) * keep; INFO[RL.EPLEN] = (INFO[RL.EPLEN] + 1.0f) * keep;
    for (int k = 0; k < ODK_NMETRIC; k++) INFO[RL.EPMET + k] = (INFO[RL.EPMET + k] + metrics[k]) * keep;
    INFO[RL.CTR] = i2f((int)(ctre + 1)); INFO[RL.STEP] = i2f(step_e); INFO[RL.PSTEP] = i2f(push_step_e);
    INFO[RL.LCON] = i2f(lcon_new);
  }
  ODK_SYNC();
  // ---- AutoReset.step epilogue: data, obs <- first_* where done (info is NOT reset)
  if (done_f != 0.0f && c.autoreset) {
    const float* fs = a.first + (size_t)e * R::FSIZE;
    for (int i = lane; i < S::NQ + 2 * S::NV; i += G) L[S::O_QPOS + i] = fs[i];
    for (int k = lane; k < R::NPRIV; k += G) L[E::O_PRIV + k] = fs[R::FOBS + R::NOBS + k];
    // first_obs["state"] == first_priv[:101] by construction; every lane re-reads only what it wrote: no barrier
    if (a.cmd && lane >= 6 && lane < 13) L[E::O_PRIV + lane] = INFO[RL.CMD + lane - 6];   // bound: the command slots (obs 6 .. 12, both tasks) show the row
  }
  if (live) {
    // record store addresses recomputed here (opaque offset) instead of being shared with the prologue's loads and
    // carried across the substep loop: 69 64-bit per-lane pointers = 138 scratch dwords otherwise
    // (the env index is made opaque as well: the 64-bit record offset is then one multiply-add here instead of a value the
    // register allocator carries from the prologue -- in scratch, in the height-field kernel)
    int e_out = e;
    asm volatile("" : "+v"(e_out));
    float* rco = reinterpret_cast<float*>(reinterpret_cast<char*>(a.recs + (size_t)e_out * R::SIZE) + opaque1);
    for (int i = lane; i < S::NQ + 2 * S::NV; i += G) rco[i] = L[S::O_QPOS + i];
    for (int k = lane; k < RL.NINFO; k += G) rco[R::INFO + k] = INFO[k];
    write_outputs<S, G>(a, L, env, reward, done_f, trunc, metrics, lane);
  }
#ifdef ODK_PROFILE
  if (a.dbg_lds && live && lane == 0) a.dbg_lds[(size_t)env * S::TOTAL + S::O_SCR + S::S_PROF + 19] = (float)(clock64() - t_k2);
#endif
}

// the product step and the one that fills the debug image (kernels of their own names: the product kernels keep theirs)
template <class S, int G, int HF>
__global__ void __launch_bounds__(64, STEP_WAVES) step_kernel(KArgs a) { step_body<S, G, HF, false>(a); }
template <class S, int G, int HF>
__global__ void __launch_bounds__(64, STEP_WAVES) step_kernel_dbg(KArgs a) { step_body<S, G, HF, true>(a); }

// mjx_env.step alone: ctrl = action buffer, no env logic (parity tests)
template <class S, int G, int HF>
__global__ void __launch_bounds__(64) physics_kernel(KArgs a) {
  extern __shared__ float lds[];
  using E = EnvL<S>; using R = Rec<S>;
  const int slot = threadIdx.x / G, lane = threadIdx.x % G;
  const int env = blockIdx.x * (64 / G) + slot;
  const bool live = env < a.nenv;
  const int e = live ? env : a.nenv - 1;
  float* L = lds + slot * E::TOTAL;
  const int* RT = load_shared<S>(lds, 64 / G, a.m);   // ordered before its first use by the ODK_SYNCs below
#ifdef ODK_POISON_LDS   // debug build: every read of LDS that was not written by this launch surfaces as NaN
  for (int k = lane; k < E::TOTAL; k += G) L[k] = __int_as_float(0x7fc00000);
  ODK_SYNC();
#endif
  float* rc = a.recs + (size_t)e * R::SIZE;
  for (int i = lane; i < S::NQ + 2 * S::NV; i += G) L[S::O_QPOS + i] = rc[i];
  for (int u = lane; u < S::NU; u += G) L[S::O_CTRL + u] = a.action[(size_t)e * S::NU + u];
  load_params<S, G>(L, a.m, a.dr ? a.dr + (size_t)e * DRL<S>::SIZE : nullptr, lane);
#ifdef ODK_PROFILE
  for (int k = lane; k < 36; k += G) L[S::O_SCR + S::S_PROF + k] = 0;
#endif
  ODK_SYNC();
  Statics<S, G> st;
  load_statics<S, G>(st, a.m, lane);
  for (int s = 0; s < a.n_substeps; s++) {
    const bool last = s == a.n_substeps - 1;
    forward_env<S, G, HF>(L, RT, a.m, a.hfield, st, lane, last ? 1 : 0);
    if (last && a.dbg_lds && live) dump_lds<S, G>(a.dbg_lds, L, env, lane);
    euler_env<S, G>(L, a.m, st, lane);
  }
  if (live) for (int i = lane; i < S::NQ + 2 * S::NV; i += G) rc[i] = L[S::O_QPOS + i];
}

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

enum { K_RESET = 0, K_STEP = 1, K_PHYS = 2 };

template <class S, int G, int HF> static hipError_t launch_sg(int which, const KArgs& a, hipStream_t st) {
  const int per_block = 64 / G;
  const int grid = (a.nenv + per_block - 1) / per_block;
  const size_t lds = (size_t)EnvL<S>::wg_floats(per_block) * sizeof(float);
  if (which == K_RESET) hipLaunchKernelGGL((reset_kernel<S, G, HF>), dim3(grid), dim3(64), lds, st, a);
  else if (which == K_STEP) {   // reset and physics launches always carry the debug image (one instantiation each, debug stores compiled in)
    if constexpr (!STEP_DUMPS_ALWAYS) {   // (the profile build never launches the debug kernels and does not instantiate them)
      if (a.dbg_lds) { hipLaunchKernelGGL((step_kernel_dbg<S, G, HF>), dim3(grid), dim3(64), lds, st, a); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((step_kernel<S, G, HF>), dim3(grid), dim3(64), lds, st, a);
  }
  else hipLaunchKernelGGL((physics_kernel<S, G, HF>), dim3(grid), dim3(64), lds, st, a);
  return hipGetLastError();
}
static hipError_t launch(odk_batch* b, int which, const KArgs& a, hipStream_t st) {
#if defined(ODK_DEV_C32)   // development build: the tail_biped shape alone
  if (b->model.shape == 2 && b->G == 32) return launch_sg<ShapeC, 32, 0>(which, a, st);
  return hipErrorNotSupported;
#elif defined(ODK_DEV_D32)   // development build: the six-dof biped's shape alone
  if (b->model.shape == 3 && b->G == 32) return launch_sg<ShapeD, 32, 0>(which, a, st);
  return hipErrorNotSupported;
#elif defined(ODK_DEV_B32)   // development builds: one instantiation only (make libodk_devB.so / libodk_devA.so: ~25 s instead of 2 min)
  if (b->model.shape == 1 && b->model.h.floor_is_plane && b->G == 32) return launch_sg<ShapeB, 32, 0>(which, a, st);
  return hipErrorNotSupported;
#elif defined(ODK_DEV_A32)
  if (b->model.shape == 0 && b->G == 32) return launch_sg<ShapeA, 32, 0>(which, a, st);
  return hipErrorNotSupported;
#elif defined(ODK_DEV_HF)
  if (!b->model.h.floor_is_plane) return launch_sg<ShapeB, 32, 1>(which, a, st);
  return hipErrorNotSupported;
#endif
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

// odk_env_kernels.h -- the device side of the env engine: reset / step / physics-only kernels built from odk_kernels.h, and launch_sg, which
// launches one (shape, lanes per env, floor) instantiation of them.  Included by odk_env_unit.hip alone, which instantiates one kernel set per
// object (odk_shapes.h: ODK_ENV_SET_...); the batch API in odk_engine.hip sees launch_sg's declaration only.  Env logic follows the reference
// playground/open_duck_mini_v2/joystick.py (line map next to each block) and the brax Episode/AutoReset wrappers.
#pragma once
#include <hip/hip_runtime.h>

#include "odk_shapes.h"
#include "odk_kernels.h"
#include "odk_poison.h"

// per-env HBM records, observation strides, random-draw streams, the env logic's LDS floats (EnvL), the kernels' arguments (KArgs, XTerms, DRL)
// and the compiled shapes: odk_shapes.h


// the workgroup's copy of the shared tables (call with all 64 lanes; followed by a hand-off barrier at the caller)
template <class S, bool HOT = false> __device__ __forceinline__ const int* load_shared(float* lds, int envs, const DevModel* m) {
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
  if constexpr (HOT && S::HOT_LDS) {   // the model's uniform floats of the substep (forward_env: HOTV; HOT: the kernel that reads them), where the shape's workgroup has the room
    if (k < HOT_NF) SH[S::SH_HOT + k] = m->hot_f[k];
  }
  return RT;
}

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
// over DevModel::obs_tab (built at model load by build_obs_table, odk_model_load.hip: the layouts are written down there).  Element ks of the task's layout is
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
#ifdef ODK_POISON_LDS   // debug build: every read of LDS that was not written by this launch surfaces as NaN (the whole allocation:
  odk_poison_fill(lds, E::wg_floats(64 / G));   // env images, padding, shared tables -- which load_shared then writes)
  ODK_SYNC();
#endif
  const int* RT = load_shared<S>(lds, 64 / G, a.m);   // ordered before its first use by the ODK_SYNCs below
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
#ifdef ODK_POISON_LDS   // debug build: every read of LDS that was not written by this launch surfaces as NaN (the whole allocation:
  odk_poison_fill(lds, E::wg_floats(64 / G));   // env images, padding, shared tables -- which load_shared then writes)
  ODK_SYNC();
#endif
  const int* RT = load_shared<S, HF == 0>(lds, 64 / G, a.m);   // (with the hot floats for the plane-floor kernel, which reads them) ordered before its first use by the ODK_SYNCs below
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
  for (int k = lane; k < 40; k += G) L[S::O_SCR + S::S_PROF + k] = 0;
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
  int aidx = randint3((float)(w0 >> 8) * (1.0f / 16777216.0f));
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
  if (a.delay) {   // bound action delays: env e's row names the ring row (draw 0 was taken and is dropped); a negative row keeps the sampled one
    const int d = a.delay[(size_t)e * a.delay_stride];
    if (d >= 0) aidx = d < 2 ? d : 2;
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
#ifdef ODK_POISON_LDS   // debug build: every read of LDS that was not written by this launch surfaces as NaN (the whole allocation:
  odk_poison_fill(lds, E::wg_floats(64 / G));   // env images, padding, shared tables -- which load_shared then writes)
  ODK_SYNC();
#endif
  const int* RT = load_shared<S>(lds, 64 / G, a.m);   // ordered before its first use by the ODK_SYNCs below
  float* rc = a.recs + (size_t)e * R::SIZE;
  for (int i = lane; i < S::NQ + 2 * S::NV; i += G) L[S::O_QPOS + i] = rc[i];
  for (int u = lane; u < S::NU; u += G) L[S::O_CTRL + u] = a.action[(size_t)e * S::NU + u];
  load_params<S, G>(L, a.m, a.dr ? a.dr + (size_t)e * DRL<S>::SIZE : nullptr, lane);
#ifdef ODK_PROFILE
  for (int k = lane; k < 40; k += G) L[S::O_SCR + S::S_PROF + k] = 0;
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

template <class S, int G, int HF> hipError_t launch_sg(int which, const KArgs& a, hipStream_t st) {
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

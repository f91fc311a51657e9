// odk_reports.hip -- the evaluation reports of include/odk.h (libodk.so): the accumulator kernels of the tracking / push / gait / posture /
// imitation / response / fall / path reports, the command-schedule kernel, the waypoint follower, the sensor-fault and actuation-fault stages, the fault resampling, the two command-curriculum kernels and the two log-replay kernels, with their C entry points.  They read
// finished observation rows (odk_obs_layout.h) and the batch (odk_batch.h: read-only here; its state is odk_engine.hip's); no compiled shape.
// gfx950 only, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/odk.h"
#include "odk_batch.h"
#include "odk_lanes.h"   // ODK_DPP
#include "odk_obs_layout.h"

using namespace odk;

// ---- what the kernels share
// hypot through float64 (the squares are exact there, the root is correctly rounded, then one rounding to float32): a host restatement has its bits
__device__ __forceinline__ float planar32(float x, float y) { return (float)sqrt((double)x * (double)x + (double)y * (double)y); }
__device__ __forceinline__ float row_sum16(float x) {   // total of a 16-lane DPP row in each of its lanes; uniform control flow only
  x += ODK_DPP(x, 0xB1, 0xF); x += ODK_DPP(x, 0x4E, 0xF); x += ODK_DPP(x, 0x141, 0xF); x += ODK_DPP(x, 0x140, 0xF);
  return x;
}
// The 16-lane kernels' thread: one DPP row per env, four envs per wave, lane u of its row.  sample: the env's first episode was running when this
// step began (the tracking accumulator's ENDED slot) and the step did not end it (a done step's observation is the auto-reset's); act: a
// sample's lane below nu.  Rows that are no sample only take part in the row sums: row = 0, P / Q = privileged row 0 and its tail.
// (fall_kernel, which also acts on the step that ends the episode, tells `live` from `sample` itself: taken from here its instruction stream changed.)
struct Row16 { int u; bool sample, act; size_t row; const float *P, *Q; };
__device__ __forceinline__ Row16 row16(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                       const float* __restrict__ track, int nenv) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, e = t >> 4;
  Row16 r; r.u = t & 15;
  r.sample = e < nenv && track[(size_t)(e < nenv ? e : 0) * ODK_TRACK_NACC + ODK_TRACK_ENDED] == 0.0f && done[e < nenv ? e : 0] == 0.0f;
  r.act = r.sample && r.u < nu;
  r.row = r.sample ? e : 0;
  r.P = priv + r.row * npriv; r.Q = r.P + nobs;
  return r;
}

// ---- what the entry points share.  Every refusal comes before the launch
static int null_args(const char* fn, const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                     const float* track_acc_dev, const float* acc_dev, bool track_here = true) {   // track_here = false: sched_args_ok names it
  const void* const p[6] = {b, priv_dev, done_dev, truncation_dev, track_acc_dev, acc_dev};
  static const char* const name[6] = {"batch", "priv_dev", "done_dev", "truncation_dev", "track_acc_dev", "acc_dev"};
  for (int i = 0; i < 6; i++) if (!p[i] && (i != 4 || track_here)) return fail(ODK_ERR_INVALID, "%s: null %s", fn, name[i]);
  return ODK_OK;
}
static int finite_nonneg(const char* fn, const char* name, float v, const char* what) {   // what: "tolerance >= 0, in radians"
  return std::isfinite(v) && v >= 0.0f ? ODK_OK : fail(ODK_ERR_INVALID, "%s: %s = %g (a finite %s)", fn, name, (double)v, what);
}
static int fits_row16(const char* fn, int nu) { return nu <= 16 ? ODK_OK : fail(ODK_ERR_INVALID, "%s: the model has %d actuators, a row holds 16", fn, nu); }
// the row strides, the batch's device made current, and a grid of 256-thread blocks with `lanes` threads per env (1, or a 16-lane row)
struct Launch { int nobs, npriv; dim3 grid; };
static int launch_on(const odk_batch* b, int lanes, Launch* g) {
  obs_sizes_nu(b->model.h.nu, b->cfg.env_kind, &g->nobs, &g->npriv);
  HIPCHK(hipSetDevice(b->device));
  g->grid = dim3((unsigned)(((long long)b->nenv * lanes + 255) / 256));
  return ODK_OK;
}

// Velocity-tracking sums of one evaluation step (one thread per env): the achieved values are the noise-free privileged observation's
// gyro and local linear velocity, joystick.py:596-604 / standing.py:549-556
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
  const float v[3] = {P[nobs + priv_at::LOCAL_LINVEL], P[nobs + priv_at::LOCAL_LINVEL + 1], P[nobs + priv_at::GYRO + 2]};
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
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  hipLaunchKernelGGL(tracking_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, reward_dev, done_dev,
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
  const float ex = P[nobs + priv_at::LOCAL_LINVEL] - C[0], ey = P[nobs + priv_at::LOCAL_LINVEL + 1] - C[1];
  const float lin = planar32(ex, ey), ang = fabsf(P[nobs + priv_at::GYRO + 2] - C[2]);   // (a host restatement has LAST_OFF's and the peaks' bits)
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
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  hipLaunchKernelGGL(push_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, done_dev, truncation_dev,
                     b->d_cmd, b->cmd_stride, b->d_push, b->push_stride, track_acc_dev, lin_tol, ang_tol, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Gait and actuator-load sums of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED contract of push_kernel).
// One 16-lane DPP row per env, lane = actuator, four envs per wave: the nu-wide reads of the privileged row and the per-actuator arrays of the
// accumulator row (stride ODK_GAIT_STRIDE = 16) are contiguous 64-byte accesses, the per-env scalars are row sums (the four in-row butterfly
// stages of greduce).  The 32 scalar slots are held two per lane (u and 16 + u); every lane computes the row-uniform terms and keeps its own.
// Only a gait sample (first episode, not done) stores anything, so every other row keeps its bits.
__global__ void __launch_bounds__(256) gait_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                   const float* __restrict__ track, const float* __restrict__ limit, float* __restrict__ acc, int nenv) {
  const Row16 th = row16(priv, npriv, nobs, nu, done, track, nenv);
  const int u = th.u; const bool sample = th.sample, act = th.act;
  const float *P = th.P, *Q = th.Q; float* A = acc + th.row * ODK_GAIT_NACC;
  // per actuator (0 in the lanes past nu and in the rows that are no sample)
  const float a1 = act ? P[obs_at::last_act(nu) + u] : 0.0f, a2 = act ? P[obs_at::last_last_act(nu) + u] : 0.0f;
  const float q = act ? Q[priv_at::JOINT_POS + u] : 0.0f, v = act ? Q[priv_at::joint_vel(nu) + u] : 0.0f;
  const float f = act ? Q[priv_at::actuator_force(nu) + u] : 0.0f;
  const float lim = (act && limit) ? limit[u] : 0.0f;
  const float af = fabsf(f), pw = fabsf(f * v), da = a1 - a2;
  const float power = row_sum16(pw), arate = row_sum16(da * da);
  if (!sample) return;
  // per env (the same in the row's 16 lanes)
  const float n0 = A[ODK_GAIT_SAMPLES];
  const bool first = n0 == 0.0f;
  const float h = Q[priv_at::root_height(nu)];
  float c[2], td[2], swing[2], slip[2], run[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float* FV = Q + priv_at::feet_linvel(nu) + 3 * k;
    const bool con = Q[priv_at::contact(nu) + k] != 0.0f;
    const float air = A[ODK_GAIT_AIR_RUN + k];
    const bool touch = con && !first && A[ODK_GAIT_PREV_CONTACT + k] == 0.0f;
    c[k] = con ? 1.0f : 0.0f;
    td[k] = touch ? 1.0f : 0.0f;
    swing[k] = touch ? air : 0.0f;               // the non-contact run that this touchdown ends
    slip[k] = con ? hypotf(FV[0], FV[1]) : 0.0f;
    run[k] = con ? 0.0f : air + 1.0f;
  }
  const float speed = hypotf(Q[priv_at::LOCAL_LINVEL], Q[priv_at::LOCAL_LINVEL + 1]);
  const float wob = Q[priv_at::GYRO] * Q[priv_at::GYRO] + Q[priv_at::GYRO + 1] * Q[priv_at::GYRO + 1];
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
  const char* fn = "odk_gait_accumulate";
  if (int rc = null_args(fn, b, priv_dev, done_dev, truncation_dev, track_acc_dev, acc_dev)) return rc;
  const int nu = b->model.h.nu;
  static_assert(ODK_GAIT_STRIDE == 16 && ODK_IMIT_STRIDE == 16, "one lane per actuator");
  if (int rc = fits_row16(fn, nu)) return rc;
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  hipLaunchKernelGGL(gait_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, nu, done_dev,
                     track_acc_dev, torque_limit_dev, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Posture and stillness sums of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED contract of push_kernel), in
// gait_kernel's layout: one 16-lane DPP row per env, lane = actuator, four envs per wave.  Every actuator lane loads its posture-command slot
// (hslot[u], -1: a leg) and its home pose; the per-env scalars are row sums, held one per lane (lanes 0 .. 9), and the lane whose hslot is
// k >= 0 owns slot k's entries of the four per-slot arrays.  Only a sample (first episode, not done) stores anything, so every other row keeps its bits.
__global__ void __launch_bounds__(256) posture_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                      const float* __restrict__ track, const float* __restrict__ cmd, int cmd_stride,
                                                      const int* __restrict__ hslot, const DevModel* __restrict__ m, float tol,
                                                      float* __restrict__ acc, int nenv) {
  const Row16 th = row16(priv, npriv, nobs, nu, done, track, nenv);
  const int u = th.u; const bool sample = th.sample, act = th.act;
  const float *Q = th.Q, *C = cmd + th.row * cmd_stride; float* A = acc + th.row * ODK_POSTURE_NACC;
  // per actuator (0 in the lanes past nu and in the rows that are no sample)
  const int k = act ? hslot[u] : -1;
  const bool head = k >= 0, leg = act && k < 0;
  const float dq = act ? Q[priv_at::JOINT_POS + u] : 0.0f, v = act ? Q[priv_at::joint_vel(nu) + u] : 0.0f;
  const float angle = head ? dq + m->key_ctrl[u] : 0.0f;
  const float err = head ? angle - C[3 + k] : 0.0f, aerr = fabsf(err), sq = err * err;
  const float leg_pose = row_sum16(leg ? fabsf(dq) : 0.0f), leg_vel = row_sum16(leg ? fabsf(v) : 0.0f), head_sq = row_sum16(sq);
  if (!sample) return;
  // per env (the same in the row's 16 lanes)
  const float n0 = A[ODK_POSTURE_SAMPLES];
  const float drift = planar32(Q[priv_at::LOCAL_LINVEL], Q[priv_at::LOCAL_LINVEL + 1]), tilt = planar32(Q[priv_at::GRAVITY], Q[priv_at::GRAVITY + 1]);
  const float yaw = Q[priv_at::GYRO + 2] * Q[priv_at::GYRO + 2], wob = Q[priv_at::GYRO] * Q[priv_at::GYRO] + Q[priv_at::GYRO + 1] * Q[priv_at::GYRO + 1];
  const float h = Q[priv_at::root_height(nu)];
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
  const char* fn = "odk_posture_accumulate";
  if (int rc = null_args(fn, b, priv_dev, done_dev, truncation_dev, track_acc_dev, acc_dev)) return rc;
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "odk_posture_accumulate: no commands bound (odk_batch_bind_commands)");
  if (!b->hmap_set)
    return fail(ODK_ERR_INVALID, "odk_posture_accumulate: the batch has no head-joint map (odk_batch_set_head_joints; an all -1 map is a map)");
  const int nu = b->model.h.nu;
  if (int rc = fits_row16(fn, nu)) return rc;
  if (int rc = finite_nonneg(fn, "tol", tol, "tolerance >= 0, in radians")) return rc;
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  hipLaunchKernelGGL(posture_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, nu, done_dev,
                     track_acc_dev, b->d_cmd, b->cmd_stride, b->d_hslot, b->d_model, tol, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Imitation-fidelity sums of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED contract of push_kernel), in
// gait_kernel's layout: one 16-lane DPP row per env, lane = actuator, four envs per wave.  Every actuator lane loads its frame joint through
// the batch's imitation map (imap[u], -1: not compared) and its home pose; the two reward terms are row sums, the 32 scalar slots are held two
// per lane (u and 16 + u) as gait's, and a compared lane owns entry u of the eight per-actuator arrays.  The frame is the one the reward read
// (O_REF).  Only a sample (first episode, not done) stores anything, so every other row keeps its bits.
__global__ void __launch_bounds__(256) imitation_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                        const float* __restrict__ track, const int* __restrict__ imap,
                                                        const DevModel* __restrict__ m, int period, float* __restrict__ acc, int nenv) {
  const Row16 th = row16(priv, npriv, nobs, nu, done, track, nenv);
  const int u = th.u; const bool sample = th.sample, act = th.act;
  const float *P = th.P, *Q = th.Q, *F = Q + priv_at::ref_frame(nu); float* A = acc + th.row * ODK_IMIT_NACC;
  // per actuator (0 in the lanes past nu, in the lanes the map leaves out and in the rows that are no sample)
  const int ri = act ? imap[u] : -1;
  const bool cmp = ri >= 0;
  const float jq = cmp ? Q[priv_at::JOINT_POS + u] + m->key_ctrl[u] : 0.0f, rq = cmp ? F[ref_at::JOINT_POS + ri] : 0.0f;
  const float dp = jq - rq, dv = cmp ? Q[priv_at::joint_vel(nu) + u] - F[ref_at::JOINT_VEL + ri] : 0.0f;
  const float sp = dp * dp, sv = dv * dv;
  const float jpos = row_sum16(sp), jvel = row_sum16(sv);
  if (!sample) return;
  // per env (the same in the row's 16 lanes)
  const bool first = A[ODK_IMIT_SAMPLES] == 0.0f;
  const float* CM = P + obs_at::COMMAND;
  const float gated = sqrtf(CM[0] * CM[0] + CM[1] * CM[1] + CM[2] * CM[2]) > 0.01f ? 1.0f : 0.0f;   // the reward's gate (step_kernel's cn)
  const float sr = planar32(F[ref_at::PLANAR_VEL], F[ref_at::PLANAR_VEL + 1]);
  const float ds = planar32(Q[priv_at::LOCAL_LINVEL], Q[priv_at::LOCAL_LINVEL + 1]) - sr;
  const float per = (float)period;
  float c[2], r[2], both[2], ronly[2], fonly[2], rtd[2], td[2], lag[2], age[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const bool con = Q[priv_at::contact(nu) + k] != 0.0f, ref = F[ref_at::CONTACT + k] > 0.5f;
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
  const char* fn = "odk_imitation_accumulate";
  if (int rc = null_args(fn, b, priv_dev, done_dev, truncation_dev, track_acc_dev, acc_dev)) return rc;
  if (b->cfg.env_kind != ODK_ENV_JOYSTICK)
    return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: a Standing batch's privileged row has no reference-motion frame (env_kind = ODK_ENV_JOYSTICK only)");
  if (!b->cfg.use_imitation)
    return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: use_imitation = 0: the frame of the privileged row is all zeros, there is nothing to compare with");
  if (!b->imap_set)
    return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: the batch has no imitation joint map (odk_batch_set_imitation_joints)");
  const int nu = b->model.h.nu;
  if (int rc = fits_row16(fn, nu)) return rc;
  if (period_steps < 0) return fail(ODK_ERR_INVALID, "odk_imitation_accumulate: period_steps = %d (the reference motion's nb_steps_in_period, or 0 for unfolded lags)", period_steps);
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  hipLaunchKernelGGL(imitation_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, nu, done_dev,
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
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  // the bound buffer is the caller's own device memory, handed over read-only for the step kernels; this launch is the one writer
  hipLaunchKernelGGL(sched_apply_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, sched_dev, nsched, nseg, sched_of_env_dev,
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
  const float v[3] = {P[nobs + priv_at::LOCAL_LINVEL], P[nobs + priv_at::LOCAL_LINVEL + 1], P[nobs + priv_at::GYRO + 2]};
  const float ex = v[0] - C[0], ey = v[1] - C[1];
  // push_kernel's planar32, spelled out: this kernel's contraction is off, the helper's is not, and the instruction stream is kept as it was
  const float lin = (float)sqrt((double)ex * (double)ex + (double)ey * (double)ey), ang = fabsf(v[2] - C[2]);
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
  if (int rc = null_args(fn, b, priv_dev, done_dev, truncation_dev, track_acc_dev, acc_dev, false)) return rc;   // then the schedule's, then track_acc_dev
  if (int rc = sched_args_ok(fn, b, sched_dev, nsched, nseg, sched_of_env_dev, track_acc_dev)) return rc;
  if (int rc = finite_nonneg(fn, "lin_tol", lin_tol, "tolerance >= 0, in m/s")) return rc;
  if (int rc = finite_nonneg(fn, "ang_tol", ang_tol, "tolerance >= 0, in rad/s")) return rc;
  if (tail_after < 0) return fail(ODK_ERR_INVALID, "%s: tail_after = %d (a number of steps >= 0)", fn, tail_after);
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  hipLaunchKernelGGL(response_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, done_dev, truncation_dev,
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
  const float f = act ? Q[priv_at::actuator_force(nu) + u] : 0.0f;
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
  const float lin = planar32(Q[priv_at::LOCAL_LINVEL] - C[0], Q[priv_at::LOCAL_LINVEL + 1] - C[1]), ang = fabsf(Q[priv_at::GYRO + 2] - C[2]);   // push_kernel's
  const float tilt = planar32(Q[priv_at::GRAVITY], Q[priv_at::GRAVITY + 1]);          // posture_kernel's
  const bool upright = tilt <= tilt_tol;
  const float con[2] = {Q[priv_at::contact(nu)], Q[priv_at::contact(nu) + 1]};
  // lane u's scalar of the slot: a copy of the privileged row at `off`, or one of the four computed ones
  int off = priv_at::GRAVITY + u - ODK_FALL_S_UP;
  off = u >= ODK_FALL_S_GYRO ? priv_at::GYRO + u - ODK_FALL_S_GYRO : off;
  off = u >= ODK_FALL_S_LINVEL ? priv_at::LOCAL_LINVEL + u - ODK_FALL_S_LINVEL : off;
  off = u == ODK_FALL_S_HEIGHT ? priv_at::root_height(nu) : off;
  off = u >= ODK_FALL_S_CONTACT ? priv_at::contact(nu) + (u - ODK_FALL_S_CONTACT) : off;
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
  if (int rc = null_args(fn, b, priv_dev, done_dev, truncation_dev, track_acc_dev, acc_dev)) return rc;
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "%s: no commands bound (odk_batch_bind_commands)", fn);
  if (ring < 1 || ring > ODK_FALL_MAX_RING) return fail(ODK_ERR_INVALID, "%s: ring = %d (1 .. %d samples)", fn, ring, ODK_FALL_MAX_RING);
  const int nu = b->model.h.nu, nq = b->model.h.nq, need = odk_fall_row_floats(b, ring);
  if (row_stride < need) return fail(ODK_ERR_INVALID, "%s: row_stride = %d, a row of ring %d holds %d floats (odk_fall_row_floats)", fn, row_stride, ring, need);
  if (int rc = fits_row16(fn, nu)) return rc;
  if (int rc = finite_nonneg(fn, "tilt_tol", tilt_tol, "sine of the lean >= 0")) return rc;
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  hipLaunchKernelGGL(fall_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, nu, done_dev,
                     truncation_dev, track_acc_dev, b->d_cmd, b->cmd_stride, torque_limit_dev, b->d_recs, b->rec_size, nq, tilt_tol, ring, acc_dev,
                     row_stride, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// ---- paths and waypoints (include/odk.h "Paths and waypoints": the definitions these three kernels restate).  One thread per env, no LDS.
// Contraction is off and the hypots go through float64, so a float32 host restatement has the bits.
// The base pose from an env's state record (qpos at offset 0): position, and the heading vector of the base quaternion, normalised;
// (1, 0) when the base is pitched onto its nose
struct Pose { float x, y, hx, hy; };
__device__ __forceinline__ Pose base_pose(const float* __restrict__ R) {
#pragma clang fp contract(off)
  const float w = R[3], x = R[4], y = R[5], z = R[6];
  const float hx = 1.0f - 2.0f * (y * y + z * z), hy = 2.0f * (x * y + w * z);
  const float n = planar32(hx, hy);
  const bool none = n < 1e-6f;
  Pose p; p.x = R[0]; p.y = R[1];
  p.hx = none ? 1.0f : hx / n;
  p.hy = none ? 0.0f : hy / n;
  return p;
}
// a course's row of the table ([ncourse, ODK_PATH_COURSE_FLOATS]: count, then the points) and its count, both clamped as sched_row's map entry
__device__ __forceinline__ const float* course_row(const float* __restrict__ course, int ncourse, const int* __restrict__ course_of_env, int e) {
  const int c = min(max(course_of_env[e], 0), ncourse - 1);
  return course + (size_t)c * ODK_PATH_COURSE_FLOATS;
}
__device__ __forceinline__ int course_count(const float* __restrict__ W) { return min(max((int)W[0], 0), ODK_PATH_MAX_WAYPOINTS); }

// The start pose of every env, issued after odk_reset: the row zeroed, the pose in START_* and in the last-sample slots
__global__ void __launch_bounds__(256) path_begin_kernel(const float* __restrict__ recs, int rec_size, float* __restrict__ acc, int nenv) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  const Pose p = base_pose(recs + (size_t)e * rec_size);
  float* A = acc + (size_t)e * ODK_PATH_NACC;
#pragma unroll
  for (int k = 0; k < ODK_PATH_NACC; k++) A[k] = 0.0f;
  A[ODK_PATH_START_X] = p.x; A[ODK_PATH_START_Y] = p.y; A[ODK_PATH_START_HX] = p.hx; A[ODK_PATH_START_HY] = p.hy;
  A[ODK_PATH_X] = p.x; A[ODK_PATH_Y] = p.y; A[ODK_PATH_HX] = p.hx; A[ODK_PATH_HY] = p.hy;
}

// Odometry and course progress of one evaluation step, issued between odk_step and odk_tracking_accumulate (the ENDED / STEPS contract of
// push_kernel).  course == nullptr: the plain odometry mode
__global__ void __launch_bounds__(256) path_kernel(const float* __restrict__ recs, int rec_size, const float* __restrict__ done,
                                                   const float* __restrict__ trunc, const float* __restrict__ track,
                                                   const float* __restrict__ course, int ncourse, const int* __restrict__ course_of_env,
                                                   float radius, float* __restrict__ acc, int nenv) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  const float* T = track + (size_t)e * ODK_TRACK_NACC;
  if (T[ODK_TRACK_ENDED] != 0.0f) return;       // past its first episode
  float* A = acc + (size_t)e * ODK_PATH_NACC;
  if (done[e] != 0.0f) {   // ends the first episode; no sample (the record is the auto-reset's state)
    if (trunc[e] == 0.0f) { A[ODK_PATH_FELL] = 1.0f; A[ODK_PATH_FELL_LEG] = A[ODK_PATH_WP_INDEX]; }
    return;
  }
  const Pose p = base_pose(recs + (size_t)e * rec_size);
  A[ODK_PATH_LENGTH] += planar32(p.x - A[ODK_PATH_X], p.y - A[ODK_PATH_Y]);
  A[ODK_PATH_TURN] += A[ODK_PATH_HX] * p.hy - A[ODK_PATH_HY] * p.hx;   // sin of the heading change since the last sample
  A[ODK_PATH_SAMPLES] += 1.0f;
  A[ODK_PATH_X] = p.x; A[ODK_PATH_Y] = p.y; A[ODK_PATH_HX] = p.hx; A[ODK_PATH_HY] = p.hy;
  if (!course) return;
  const float* W = course_row(course, ncourse, course_of_env, e);
  const int count = course_count(W), i = max((int)A[ODK_PATH_WP_INDEX], 0);
  if (i >= count) return;                       // the course is finished
  const float shx = A[ODK_PATH_START_HX], shy = A[ODK_PATH_START_HY];
  const float rx = p.x - A[ODK_PATH_START_X], ry = p.y - A[ODK_PATH_START_Y];
  const float xs = rx * shx + ry * shy, ys = shx * ry - shy * rx;      // the start-frame position
  const float wx = W[1 + 2 * i], wy = W[2 + 2 * i];
  const float px = i > 0 ? W[2 * i - 1] : 0.0f, py = i > 0 ? W[2 * i] : 0.0f;   // where the leg starts: the waypoint before, or the origin
  const float dist = planar32(wx - xs, wy - ys);
  const float ax = wx - px, ay = wy - py, qx = xs - px, qy = ys - py;
  const float len2 = ax * ax + ay * ay;
  const float u = len2 > 0.0f ? fminf(fmaxf((qx * ax + qy * ay) / len2, 0.0f), 1.0f) : 0.0f;   // a zero-length leg: the distance to the point
  const float xt = planar32(qx - u * ax, qy - u * ay);
  A[ODK_PATH_XTRACK_SAMPLES] += 1.0f;
  A[ODK_PATH_XTRACK_SQ] += xt * xt;
  A[ODK_PATH_XTRACK_PEAK] = fmaxf(A[ODK_PATH_XTRACK_PEAK], xt);
  A[ODK_PATH_GOAL_DIST] = planar32(W[2 * count - 1] - xs, W[2 * count] - ys);
  if (dist <= radius) {   // at most one waypoint per step
    A[ODK_PATH_REACHED + i] = T[ODK_TRACK_STEPS] + 1.0f;   // this step's 1-based index
    A[ODK_PATH_WP_INDEX] = (float)(i + 1);
  }
}

// The command of the step about to run from the env's course (one thread per env), issued before odk_step: steer towards waypoint WP_INDEX.
// The tracking accumulator's STEPS slot is the clock: at 0 the pose is the start pose by definition, and nothing of the records is read
__global__ void __launch_bounds__(256) waypoint_apply_kernel(const float* __restrict__ recs, int rec_size, const float* __restrict__ track,
                                                             const float* __restrict__ path, const float* __restrict__ course, int ncourse,
                                                             const int* __restrict__ course_of_env, float v_cruise, float turn_rate,
                                                             float heading_gain, float slow_dist, float* __restrict__ cmd, int cmd_stride, int nenv) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  const float* T = track + (size_t)e * ODK_TRACK_NACC;
  if (T[ODK_TRACK_ENDED] != 0.0f) return;       // past its first episode: the row keeps the command of the step that ended it
  const float* A = path + (size_t)e * ODK_PATH_NACC;
  const float* W = course_row(course, ncourse, course_of_env, e);
  const int count = course_count(W);
  float xs = 0.0f, ys = 0.0f, c = 1.0f, s = 0.0f;
  int i = 0;
  if (T[ODK_TRACK_STEPS] != 0.0f) {
    const Pose p = base_pose(recs + (size_t)e * rec_size);
    const float shx = A[ODK_PATH_START_HX], shy = A[ODK_PATH_START_HY];
    const float rx = p.x - A[ODK_PATH_START_X], ry = p.y - A[ODK_PATH_START_Y];
    xs = rx * shx + ry * shy; ys = shx * ry - shy * rx;
    c = shx * p.hx + shy * p.hy; s = shx * p.hy - shy * p.hx;
    i = min(max((int)A[ODK_PATH_WP_INDEX], 0), count);
  }
  float vx = 0.0f, wz = 0.0f;
  if (i < count) {
    const float dx = W[1 + 2 * i] - xs, dy = W[2 + 2 * i] - ys;
    const float dist = planar32(dx, dy);
    const bool on = dist < 1e-6f;
    const float f = on ? 1.0f : (dx * c + dy * s) / dist, l = on ? 0.0f : (c * dy - s * dx) / dist;
    const float turn = f >= 0.0f ? l : (l >= 0.0f ? 1.0f : -1.0f);   // a target exactly behind turns left
    // (the clamps by comparison, not fminf / fmaxf: between +0 and -0 those may return either, a comparison keeps the bits a restatement has)
    wz = heading_gain * turn;
    wz = wz > turn_rate ? turn_rate : wz;
    wz = wz < -turn_rate ? -turn_rate : wz;
    vx = v_cruise * (f > 0.0f ? f : 0.0f);
    if (i == count - 1) vx = vx * fminf(1.0f, dist / slow_dist);
  }
  float* C = cmd + (size_t)e * cmd_stride;
  C[0] = vx; C[1] = 0.0f; C[2] = wz;
}

static int path_model_ok(const char* fn, const odk_batch* b) {
  const DevModel& m = b->model.h;
  bool floating = m.nq >= 7 && m.nv >= 6;
  for (int d = 0; floating && d < 6; d++) floating = m.dof_jnt[d] < 0;   // dofs 0 .. 5 are no hinge's: the free joint's
  return floating ? ODK_OK : fail(ODK_ERR_UNSUPPORTED, "%s: the model's first joint is not a free joint: there is no base pose at qpos[0:7]", fn);
}
static int finite_pos(const char* fn, const char* name, float v, const char* what) {
  return std::isfinite(v) && v > 0.0f ? ODK_OK : fail(ODK_ERR_INVALID, "%s: %s = %g (a finite %s)", fn, name, (double)v, what);
}

extern "C" int odk_path_begin(const odk_batch* b, float* acc_dev, void* stream) {
  const char* fn = "odk_path_begin";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!acc_dev) return fail(ODK_ERR_INVALID, "%s: null acc_dev", fn);
  if (int rc = path_model_ok(fn, b)) return rc;
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  hipLaunchKernelGGL(path_begin_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, b->d_recs, b->rec_size, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

extern "C" int odk_path_accumulate(const odk_batch* b, const float* done_dev, const float* truncation_dev, const float* track_acc_dev,
                                   const float* course_dev, int ncourse, const int32_t* course_of_env_dev, float radius, float* acc_dev,
                                   void* stream) {
  const char* fn = "odk_path_accumulate";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!done_dev) return fail(ODK_ERR_INVALID, "%s: null done_dev", fn);
  if (!truncation_dev) return fail(ODK_ERR_INVALID, "%s: null truncation_dev", fn);
  if (!track_acc_dev) return fail(ODK_ERR_INVALID, "%s: null track_acc_dev", fn);
  if (!acc_dev) return fail(ODK_ERR_INVALID, "%s: null acc_dev", fn);
  if (course_dev && !course_of_env_dev) return fail(ODK_ERR_INVALID, "%s: null course_of_env_dev", fn);
  if (!course_dev && ncourse != 0) return fail(ODK_ERR_INVALID, "%s: null course_dev with ncourse = %d (the odometry mode is NULL with 0)", fn, ncourse);
  if (course_dev && ncourse < 1) return fail(ODK_ERR_INVALID, "%s: ncourse = %d (at least one course)", fn, ncourse);
  if (int rc = finite_nonneg(fn, "radius", radius, "distance >= 0, in metres")) return rc;
  if (int rc = path_model_ok(fn, b)) return rc;
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  hipLaunchKernelGGL(path_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, b->d_recs, b->rec_size, done_dev, truncation_dev, track_acc_dev,
                     course_dev, ncourse, course_of_env_dev, radius, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

extern "C" int odk_waypoint_command_apply(const odk_batch* b, const float* course_dev, int ncourse, const int32_t* course_of_env_dev,
                                          const float* track_acc_dev, const float* path_acc_dev, float v_cruise, float turn_rate,
                                          float heading_gain, float slow_dist, void* stream) {
  const char* fn = "odk_waypoint_command_apply";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!course_dev) return fail(ODK_ERR_INVALID, "%s: null course_dev", fn);
  if (!course_of_env_dev) return fail(ODK_ERR_INVALID, "%s: null course_of_env_dev", fn);
  if (!track_acc_dev) return fail(ODK_ERR_INVALID, "%s: null track_acc_dev", fn);
  if (!path_acc_dev) return fail(ODK_ERR_INVALID, "%s: null path_acc_dev", fn);
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "%s: no commands bound (odk_batch_bind_commands)", fn);
  if (b->cmd_stride < 3) return fail(ODK_ERR_INVALID, "%s: the bound command rows are %d floats apart, the launch writes 3", fn, b->cmd_stride);
  if (ncourse < 1) return fail(ODK_ERR_INVALID, "%s: ncourse = %d (at least one course)", fn, ncourse);
  if (int rc = finite_nonneg(fn, "v_cruise", v_cruise, "speed >= 0, in m/s")) return rc;
  if (int rc = finite_nonneg(fn, "turn_rate", turn_rate, "yaw rate >= 0, in rad/s")) return rc;
  if (int rc = finite_pos(fn, "heading_gain", heading_gain, "gain > 0, in rad/s per unit of the heading error's sine")) return rc;
  if (int rc = finite_pos(fn, "slow_dist", slow_dist, "distance > 0, in metres")) return rc;
  if (int rc = path_model_ok(fn, b)) return rc;
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  // the bound buffer is the caller's own device memory (odk_command_schedule_apply's contract); this launch is the one writer
  hipLaunchKernelGGL(waypoint_apply_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, b->d_recs, b->rec_size, track_acc_dev, path_acc_dev,
                     course_dev, ncourse, course_of_env_dev, v_cruise, turn_rate, heading_gain, slow_dist, const_cast<float*>(b->d_cmd),
                     b->cmd_stride, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// ---- sensor faults (include/odk.h "Sensor faults": the definitions this kernel restates).  Not a report: the stage between the observation
// the step wrote and the policy.  gait_kernel's layout -- a 16-lane row per env, four envs per wave -- without its row sums, so a row past
// nenv leaves at once.  Lane = actuator for the joint columns and their ring entries (contiguous 64-byte accesses), lanes 0..5 carry gyro and
// accelerometer, lanes 6..7 the foot switches, and the columns nothing touches go through in ceil(nobs / 16) passes of consecutive lanes on
// consecutive floats: every float of the output row is stored exactly once.  The delayed sample is loaded before this call's sample is
// stored, and from a slot this call does not store to (delay 0 and a refill take the current values from registers), so no lane reads what
// this launch wrote.  Out of place, no LDS, no scratch; contraction is off and every nominal stage is a select, so a numpy restatement has the bits.
__global__ void __launch_bounds__(256) sensor_kernel(const float* __restrict__ obs, int nobs, int nu, int contact_at, const float* __restrict__ done,
                                                     const float* __restrict__ fault, float* __restrict__ state, float* __restrict__ out, int nenv) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, u = t & 15;
  if (e >= nenv) return;
  const float* X = obs + (size_t)e * nobs;
  const float* F = fault + (size_t)e * ODK_SENSOR_NPRM;
  float* S = state + (size_t)e * ODK_SENSOR_NSTATE;
  float* Y = out + (size_t)e * nobs;
  const int jv_at = obs_at::joint_vel(nu);
  // the columns nothing touches
  for (int j = u; j < nobs; j += 16) {
    const bool touched = j < obs_at::COMMAND || (j >= obs_at::JOINT_POS && j < jv_at + nu) || (j >= contact_at && j < contact_at + 2);
    if (!touched) Y[j] = X[j];
  }
  // the ring (per env: the same in the row's 16 lanes)
  const float n0 = S[ODK_SENSOR_HEAD];
  const bool refill = n0 == 0.0f || (done && done[e] != 0.0f);
  const int cur = refill ? 0 : (int)((unsigned)(int)n0 % (unsigned)ODK_SENSOR_RING);   // (unsigned: a row the caller did not zero still lands inside its ring)
  const int di = (int)fminf(fmaxf(F[ODK_SENSOR_IMU_DELAY], 0.0f), (float)(ODK_SENSOR_RING - 1));
  const int dj = (int)fminf(fmaxf(F[ODK_SENSOR_JOINT_DELAY], 0.0f), (float)(ODK_SENSOR_RING - 1));
  float* R = S + ODK_SENSOR_RING_AT;
  const float* Si = R + ((cur + ODK_SENSOR_RING - di) & (ODK_SENSOR_RING - 1)) * ODK_SENSOR_SAMPLE + ODK_SENSOR_S_IMU;   // the slot di steps back
  const float* Sj = R + ((cur + ODK_SENSOR_RING - dj) & (ODK_SENSOR_RING - 1)) * ODK_SENSOR_SAMPLE;
  const bool imu_now = refill || di == 0, joint_now = refill || dj == 0, imu = u < 6, act = u < nu;
  // this step's raw sample, lane u's part (0 in the joint entries past nu), and the delayed one
  const float raw_i = imu ? X[obs_at::GYRO + u] : 0.0f;
  const float raw_p = act ? X[obs_at::JOINT_POS + u] : 0.0f, raw_v = act ? X[jv_at + u] : 0.0f;
  const int base = u < 3 ? 0 : 3;                  // gyro or accelerometer: the vector lane u's component belongs to
  const float* V = imu_now ? X + obs_at::GYRO + base : Si + base;
  const float v0 = imu ? V[0] : 0.0f, v1 = imu ? V[1] : 0.0f, v2 = imu ? V[2] : 0.0f;
  const float old_p = Sj[ODK_SENSOR_S_JOINT_POS + u], old_v = Sj[ODK_SENSOR_S_JOINT_VEL + u];
  float p = joint_now ? raw_p : old_p;
  const float v = joint_now ? raw_v : old_v;
  for (int s = refill ? 0 : cur; s < (refill ? ODK_SENSOR_RING : cur + 1); s++) {
    float* W = R + s * ODK_SENSOR_SAMPLE;
    if (imu) W[ODK_SENSOR_S_IMU + u] = raw_i;
    W[ODK_SENSOR_S_JOINT_POS + u] = raw_p;
    W[ODK_SENSOR_S_JOINT_VEL + u] = raw_v;
  }
  if (u == ODK_SENSOR_HEAD) S[u] = refill ? 1.0f : n0 + 1.0f;
  // the IMU: out = scale (R x) + bias, component i of its vector in lane u
  if (imu) {
    const int i = u - base;
    bool ident = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ident = ident && F[ODK_SENSOR_IMU_ROT + k] == ((k & 3) == 0 ? 1.0f : 0.0f);
    const float* Ri = F + ODK_SENSOR_IMU_ROT + 3 * i;
    const float rot = (Ri[0] * v0 + Ri[1] * v1) + Ri[2] * v2;
    float r = ident ? (i == 0 ? v0 : (i == 1 ? v1 : v2)) : rot;
    const float scale = F[base ? ODK_SENSOR_ACC_SCALE : ODK_SENSOR_GYRO_SCALE];
    const float bias = F[(base ? ODK_SENSOR_ACC_BIAS : ODK_SENSOR_GYRO_BIAS) + i];
    r = scale != 1.0f ? scale * r : r;
    r = bias != 0.0f ? r + bias : r;
    Y[obs_at::GYRO + u] = r;
  }
  // the encoders: offset, then the quantiser; the velocities are only late
  if (act) {
    const float off = F[ODK_SENSOR_ENC_OFFSET + u], q = F[ODK_SENSOR_ENC_QUANT];
    p = off != 0.0f ? p + off : p;
    p = q > 0.0f ? q * rintf(p / q) : p;
    Y[obs_at::JOINT_POS + u] = p;
    Y[jv_at + u] = v;
  }
  // the foot switches
  if (u == 6 || u == 7) {
    const float mode = F[ODK_SENSOR_CONTACT_MODE + u - 6], c = X[contact_at + u - 6];
    Y[contact_at + u - 6] = mode == 1.0f ? 0.0f : (mode == 2.0f ? 1.0f : c);
  }
}

extern "C" int odk_sensor_apply(const odk_batch* b, const float* obs_dev, const float* done_dev, const float* fault_dev, float* state_dev,
                                float* obs_out_dev, void* stream) {
  const char* fn = "odk_sensor_apply";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!obs_dev) return fail(ODK_ERR_INVALID, "%s: null obs_dev", fn);
  if (!fault_dev) return fail(ODK_ERR_INVALID, "%s: null fault_dev", fn);
  if (!state_dev) return fail(ODK_ERR_INVALID, "%s: null state_dev", fn);
  if (!obs_out_dev) return fail(ODK_ERR_INVALID, "%s: null obs_out_dev", fn);
  static_assert(ODK_SENSOR_S_JOINT_VEL + 16 == ODK_SENSOR_SAMPLE && ODK_SENSOR_ENC_OFFSET + 16 == ODK_SENSOR_NPRM &&
                (ODK_SENSOR_RING & (ODK_SENSOR_RING - 1)) == 0, "one lane per actuator, a ring the mask wraps");
  const int nu = b->model.h.nu;
  if (int rc = fits_row16(fn, nu)) return rc;
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  const size_t n = (size_t)b->nenv * g.nobs;
  if (obs_out_dev < obs_dev + n && obs_dev < obs_out_dev + n)
    return fail(ODK_ERR_INVALID, "%s: obs_out_dev overlaps obs_dev (the stage is out of place: the step's observation is only read)", fn);
  hipLaunchKernelGGL(sensor_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, obs_dev, g.nobs, nu,
                     obs_at::contact(nu, b->cfg.env_kind == ODK_ENV_JOYSTICK), done_dev, fault_dev, state_dev, obs_out_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// ---- actuation faults (include/odk.h "Actuation faults": the definitions this kernel restates).  Not a report: the stage between the
// policy's action and the env step.  sensor_kernel's geometry -- a 16-lane row per env, lane = actuator, four envs per wave, a row past
// nenv leaves at once.  What is uniform over an env's row (the step count, the hold counter, the loss decision) every lane computes from
// the same loads: no cross-lane traffic.  Every load of the state row comes before its first store, and a row sits inside one wave, so
// lane 0's scalar stores follow every lane's loads.  Out of place, no LDS, no scratch; contraction is off and every nominal stage is a
// select, so a numpy restatement has the bits.
__device__ __forceinline__ float act_uniform(unsigned seed, unsigned env, unsigned episode, unsigned step, unsigned stream) {
  unsigned x = seed + 0x9E3779B9u * env + 0x85EBCA6Bu * episode + 0xC2B2AE35u * step + 0x27D4EB2Fu * stream;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return (float)(x >> 8) * 5.9604644775390625e-08f;      // 2^-24: exact, 0 <= u < 1
}

__global__ void __launch_bounds__(256) action_kernel(const float* __restrict__ act, int nu, const float* __restrict__ done,
                                                     const float* __restrict__ fault, float* __restrict__ state, float* __restrict__ out, int nenv) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, u = t & 15;
  if (e >= nenv) return;
  const float* F = fault + (size_t)e * ODK_ACT_NPRM;
  float* S = state + (size_t)e * ODK_ACT_NSTATE;
  const bool lane = u < nu;
  // everything this call reads of the state row, before anything is stored
  const float n0 = S[ODK_ACT_HEAD], ep0 = S[ODK_ACT_EPISODE], hold0 = S[ODK_ACT_HOLD], calls0 = S[ODK_ACT_CALLS], drops0 = S[ODK_ACT_DROPS];
  const float filt0 = S[ODK_ACT_FILT + u], prev0 = S[ODK_ACT_PREV + u];
  float a = lane ? act[(size_t)e * nu + u] : 0.0f;
  // 1. the refill
  const bool refill = n0 == 0.0f || (done && done[e] != 0.0f);
  const float step = refill ? 0.0f : n0, episode = refill ? ep0 + 1.0f : ep0, hold = refill ? 0.0f : hold0;
  const float y_prev = refill ? 0.0f : filt0, prev = refill ? 0.0f : prev0;
  const unsigned seed = (unsigned)fminf(fmaxf(F[ODK_ACT_SEED], 0.0f), 16777215.0f);
  const unsigned ue = (unsigned)e, uep = (unsigned)episode, ust = (unsigned)step;
  // 2. the runtime's side: gain, offset, noise, limit, filter, quantiser
  const float gain = F[ODK_ACT_GAIN], off = F[ODK_ACT_OFFSET + u], amp = F[ODK_ACT_NOISE], lim = F[ODK_ACT_LIMIT];
  const float alpha = F[ODK_ACT_ALPHA], q = F[ODK_ACT_QUANT];
  a = (gain < 1.0f || gain > 1.0f) ? gain * a : a;
  a = (off < 0.0f || off > 0.0f) ? a + off : a;
  const float un = act_uniform(seed, ue, uep, ust, 1u + (unsigned)u);
  a = amp > 0.0f ? a + amp * ((un + un) - 1.0f) : a;
  a = lim > 0.0f ? fminf(fmaxf(a, -lim), lim) : a;
  const float y = (alpha * y_prev) + ((1.0f - alpha) * a);
  const float filt = alpha > 0.0f ? y : y_prev;
  a = alpha > 0.0f ? y : a;
  a = q > 0.0f ? q * rintf(a / q) : a;
  // 3. the bus: a lost packet, the same decision in the row's 16 lanes
  const float u0 = act_uniform(seed, ue, uep, ust, 0u);
  const bool held = hold > 0.0f, drawn = !held && u0 < F[ODK_ACT_DROP_P], lost = held || drawn;
  const float hold1 = held ? hold - 1.0f : (drawn ? fmaxf(F[ODK_ACT_DROP_LEN], 1.0f) - 1.0f : hold);
  a = lost ? prev : a;
  // 4. the servo: off the bus from its step on
  const float f = F[ODK_ACT_FREEZE_AT + u];
  a = (f >= 0.0f && step >= f) ? prev : a;
  // 5. the stores
  if (lane) {
    out[(size_t)e * nu + u] = a;
    S[ODK_ACT_FILT + u] = filt;
    S[ODK_ACT_PREV + u] = a;
  }
  if (u == 0) {
    S[ODK_ACT_HEAD] = step + 1.0f;
    S[ODK_ACT_EPISODE] = episode;
    S[ODK_ACT_HOLD] = hold1;
    S[ODK_ACT_CALLS] = calls0 + 1.0f;
    S[ODK_ACT_DROPS] = lost ? drops0 + 1.0f : drops0;
  }
}

extern "C" int odk_action_apply(const odk_batch* b, const float* act_dev, const float* done_dev, const float* fault_dev, float* state_dev,
                                float* act_out_dev, void* stream) {
  const char* fn = "odk_action_apply";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!act_dev) return fail(ODK_ERR_INVALID, "%s: null act_dev", fn);
  if (!fault_dev) return fail(ODK_ERR_INVALID, "%s: null fault_dev", fn);
  if (!state_dev) return fail(ODK_ERR_INVALID, "%s: null state_dev", fn);
  if (!act_out_dev) return fail(ODK_ERR_INVALID, "%s: null act_out_dev", fn);
  static_assert(ODK_ACT_OFFSET + 16 == ODK_ACT_FREEZE_AT && ODK_ACT_FREEZE_AT + 16 == ODK_ACT_NPRM && ODK_ACT_FILT + 16 == ODK_ACT_PREV &&
                ODK_ACT_PREV + 16 == ODK_ACT_NSTATE, "one lane per actuator in every per-actuator array");
  const int nu = b->model.h.nu;
  if (int rc = fits_row16(fn, nu)) return rc;
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  const size_t n = (size_t)b->nenv * nu;
  if (act_out_dev < act_dev + n && act_dev < act_out_dev + n)
    return fail(ODK_ERR_INVALID, "%s: act_out_dev overlaps act_dev (the stage is out of place: the policy's action is only read)", fn);
  hipLaunchKernelGGL(action_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, act_dev, nu, done_dev, fault_dev, state_dev, act_out_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// ---- fault resampling (include/odk.h "Fault resampling": the definitions this kernel restates).  Not a report: at the start of each episode
// env e's row of the sensor fault table and of the actuation fault table is redrawn from a table of ranges, so that training meets a new
// faulty robot every episode.  The stages' geometry -- a 16-lane row per env, four envs per wave, a row past nenv leaves at once -- with six
// slots per lane (lane u holds slots u, 16 + u, ..: every store of a row's 16 lanes is one contiguous 64 bytes, and a group of 16 slots lies
// wholly in one of the two tables).  The two state loads come before the first store, and a row sits inside one wave, so lane 0's stores
// follow every lane's loads.  No LDS, no scratch; the draws are act_uniform's (streams 32 .. 127), contraction is off and a FIXED slot is a
// select, so a numpy restatement has the bits.
__global__ void __launch_bounds__(256) fault_resample_kernel(const float* __restrict__ done, const float* __restrict__ spec, unsigned seed,
                                                             unsigned env_id_offset, float* __restrict__ state, float* __restrict__ sensor_fault,
                                                             float* __restrict__ act_fault, int nenv) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, u = t & 15;
  if (e >= nenv) return;
  float* S = state + (size_t)e * ODK_FAULT_NSTATE;
  const float n0 = S[ODK_FAULT_HEAD], ep0 = S[ODK_FAULT_EPISODE];
  const bool redraw = n0 == 0.0f || (done && done[e] != 0.0f);
  const float episode = redraw ? ep0 + 1.0f : ep0;
  if (redraw) {
    const unsigned ue = env_id_offset + (unsigned)e, uep = (unsigned)episode;
#pragma unroll
    for (int k = 0; k < ODK_FAULT_NSLOT / 16; k++) {
      const int s = 16 * k + u;
      const float lo = spec[s], hi = spec[ODK_FAULT_NSLOT + s], kind = spec[2 * ODK_FAULT_NSLOT + s];
      const float r = act_uniform(seed, ue, uep, 0u, 32u + (unsigned)s);
      const float uniform = lo + ((hi - lo) * r);
      const float whole = fminf(lo + floorf(((hi - lo) + 1.0f) * r), hi);
      const float v = kind == (float)ODK_FAULT_UNIFORM ? uniform : (kind == (float)ODK_FAULT_WHOLE ? whole : lo);
      if (16 * k < ODK_SENSOR_NPRM) sensor_fault[(size_t)e * ODK_SENSOR_NPRM + s] = v;
      else act_fault[(size_t)e * ODK_ACT_NPRM + (s - ODK_SENSOR_NPRM)] = v;
    }
  }
  if (u == 0) {
    S[ODK_FAULT_HEAD] = n0 + 1.0f;
    S[ODK_FAULT_EPISODE] = episode;
  }
}

extern "C" int odk_fault_resample(const odk_batch* b, const float* done_dev, const float* spec_dev, uint32_t seed, uint32_t env_id_offset,
                                  float* state_dev, float* sensor_fault_dev, float* act_fault_dev, void* stream) {
  const char* fn = "odk_fault_resample";
  if (!b) return fail(ODK_ERR_INVALID, "%s: null batch", fn);
  if (!spec_dev) return fail(ODK_ERR_INVALID, "%s: null spec_dev", fn);
  if (!state_dev) return fail(ODK_ERR_INVALID, "%s: null state_dev", fn);
  if (!sensor_fault_dev) return fail(ODK_ERR_INVALID, "%s: null sensor_fault_dev", fn);
  if (!act_fault_dev) return fail(ODK_ERR_INVALID, "%s: null act_fault_dev", fn);
  static_assert(ODK_FAULT_NSLOT == ODK_SENSOR_NPRM + ODK_ACT_NPRM && ODK_SENSOR_NPRM % 16 == 0 && ODK_ACT_NPRM % 16 == 0,
                "six slots per lane, a group of 16 slots inside one table");
  const float *sf = sensor_fault_dev, *af = act_fault_dev;
  const size_t ns = (size_t)b->nenv * ODK_SENSOR_NPRM, na = (size_t)b->nenv * ODK_ACT_NPRM, nspec = 3 * (size_t)ODK_FAULT_NSLOT;
  if (sf < af + na && af < sf + ns)
    return fail(ODK_ERR_INVALID, "%s: sensor_fault_dev overlaps act_fault_dev (every slot of a row is stored once)", fn);
  if (sf < spec_dev + nspec && spec_dev < sf + ns)
    return fail(ODK_ERR_INVALID, "%s: sensor_fault_dev overlaps spec_dev (the ranges are only read)", fn);
  if (af < spec_dev + nspec && spec_dev < af + na)
    return fail(ODK_ERR_INVALID, "%s: act_fault_dev overlaps spec_dev (the ranges are only read)", fn);
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  hipLaunchKernelGGL(fault_resample_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, done_dev, spec_dev, (unsigned)seed,
                     (unsigned)env_id_offset, state_dev, sensor_fault_dev, act_fault_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// ---- command curriculum (include/odk.h "Command curriculum": the definitions these two kernels restate).  Not reports: the step kernel sits
// behind odk_step in a training rollout, the update kernel runs once per training iteration.
// curriculum_step_kernel: one thread per env, a row past nenv leaves at once.  Everything env e reads -- its state row, its command row, the
// three velocities, done and truncation -- is loaded before its first store, and the patched columns (6 .. 12) are none of the columns
// read, so priv may be the row that is patched.  The only traffic between envs is two integer atomics per judged stint: their order cannot
// change a bit.  No LDS, no scratch (the grid is kernel-argument scalars, every index into it a compile-time constant); the draws are
// act_uniform's streams 128 .. 136; contraction is off, so a numpy restatement has the bits.
__global__ void __launch_bounds__(256) curriculum_step_kernel(const odk_curriculum c, int nbins, const float* priv, int npriv, int nobs,
                                                              const float* __restrict__ done, const float* __restrict__ trunc,
                                                              const int* __restrict__ cdf, int* __restrict__ counts, float* __restrict__ state,
                                                              float* __restrict__ cmd, float* __restrict__ obs, float* priv_patch, int nenv) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nenv) return;
  float* S = state + (size_t)e * ODK_CURR_NSTATE;
  float* C = cmd + (size_t)e * 7;
  const float* P = priv + (size_t)e * npriv + nobs;
  const float head0 = S[ODK_CURR_HEAD], ep0 = S[ODK_CURR_EPISODE], stint0 = S[ODK_CURR_STINT], step0 = S[ODK_CURR_STEP], bin0 = S[ODK_CURR_BIN];
  const float samp0 = S[ODK_CURR_SAMPLES], sql0 = S[ODK_CURR_SQLIN], sqy0 = S[ODK_CURR_SQYAW];
  const float d = done ? done[e] : 0.0f, tr = trunc ? trunc[e] : 0.0f;
  const float ex = P[priv_at::LOCAL_LINVEL] - C[0], ey = P[priv_at::LOCAL_LINVEL + 1] - C[1], ez = P[priv_at::GYRO + 2] - C[2];
  const bool first = head0 == 0.0f, ended = !first && d != 0.0f;
  // 1. the sample, 2. the step count
  const bool sample = !first && d == 0.0f && step0 >= (float)c.skip;
  const float samp = sample ? samp0 + 1.0f : samp0;
  const float sql = sample ? sql0 + (ex * ex + ey * ey) : sql0, sqy = sample ? sqy0 + ez * ez : sqy0;
  const float step = first ? step0 : step0 + 1.0f;
  const bool end = ended || (!first && step == (float)c.period);
  // 3. the judgement
  if (end && bin0 >= 0.0f) {
    const bool fall = ended && tr == 0.0f;
    const bool counted = fall || samp >= (float)c.min_samples;
    const bool success = !fall && counted && sql <= (c.tol_lin * c.tol_lin) * samp && sqy <= (c.tol_yaw * c.tol_yaw) * samp;
    int* K = counts + 2 * (int)bin0;
    if (counted) atomicAdd(K, 1);
    if (success) atomicAdd(K + 1, 1);
  }
  const bool draw = first || end, fresh = first || ended;
  const float episode = fresh ? ep0 + 1.0f : ep0, stint = fresh ? 0.0f : stint0;
  S[ODK_CURR_HEAD] = head0 + 1.0f;
  if (!draw) {
    S[ODK_CURR_STEP] = step; S[ODK_CURR_SAMPLES] = samp; S[ODK_CURR_SQLIN] = sql; S[ODK_CURR_SQYAW] = sqy;
    return;
  }
  // 4. the draw
  const unsigned ue = c.env_id_offset + (unsigned)e, uep = (unsigned)episode, ust = (unsigned)stint;
  const int total = cdf[nbins - 1];
  float row[7];
  float bin = -1.0f;
  const bool zero = act_uniform(c.seed, ue, uep, ust, 128u) < c.p_zero || total <= 0;
#pragma unroll
  for (int k = 0; k < 7; k++) row[k] = 0.0f;
  if (!zero) {
    const int t = min((int)(act_uniform(c.seed, ue, uep, ust, 129u) * (float)total), total - 1);
    int lo = 0, hi = nbins - 1;
    while (lo < hi) {   // the first bin with cdf[bin] > t; cdf[nbins - 1] = total > t, so there is one
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    bin = (float)lo;
    const int i[3] = {lo / (c.n[1] * c.n[2]), (lo / c.n[2]) % c.n[1], lo % c.n[2]};
#pragma unroll
    for (int a = 0; a < 3; a++)
      row[a] = fminf(c.lo[a] + c.width[a] * ((float)i[a] + act_uniform(c.seed, ue, uep, ust, 130u + (unsigned)a)), c.hi[a]);
#pragma unroll
    for (int j = 0; j < 4; j++) row[3 + j] = c.head_lo[j] + (c.head_hi[j] - c.head_lo[j]) * act_uniform(c.seed, ue, uep, ust, 133u + (unsigned)j);
  }
  S[ODK_CURR_EPISODE] = episode; S[ODK_CURR_STINT] = stint + 1.0f; S[ODK_CURR_STEP] = 0.0f; S[ODK_CURR_BIN] = bin;
  S[ODK_CURR_SAMPLES] = 0.0f; S[ODK_CURR_SQLIN] = 0.0f; S[ODK_CURR_SQYAW] = 0.0f;
  float* O = obs ? obs + (size_t)e * nobs + obs_at::COMMAND : nullptr;
  float* Q = priv_patch ? priv_patch + (size_t)e * npriv + obs_at::COMMAND : nullptr;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    C[k] = row[k];
    if (O) O[k] = row[k];
    if (Q) Q[k] = row[k];
  }
}

static int curriculum_grid(const char* fn, const odk_curriculum* c, int* nbins) {
  long long n = 1;
  for (int a = 0; a < 3; a++) {
    if (c->n[a] < 1 || c->n[a] > ODK_CURR_MAX_AXIS)
      return fail(ODK_ERR_INVALID, "%s: n[%d] = %d (1 .. %d bins per axis)", fn, a, (int)c->n[a], ODK_CURR_MAX_AXIS);
    n *= c->n[a];
  }
  if (n > ODK_CURR_MAX_BINS) return fail(ODK_ERR_INVALID, "%s: nbins = %lld (at most %d)", fn, n, ODK_CURR_MAX_BINS);
  *nbins = (int)n;
  return ODK_OK;
}
// the first pair of byte ranges that overlap, by name (a null range takes no part)
struct Span { const char* name; const void* p; size_t bytes; };
static int spans_apart(const char* fn, const Span* s, int n) {
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) {
      if (!s[i].p || !s[j].p) continue;
      const char *a = (const char*)s[i].p, *b = (const char*)s[j].p;
      if (a < b + s[j].bytes && b < a + s[i].bytes) return fail(ODK_ERR_INVALID, "%s: %s overlaps %s", fn, s[i].name, s[j].name);
    }
  return ODK_OK;
}

extern "C" int odk_curriculum_step(const odk_batch* b, const odk_curriculum* c, const float* priv_dev, const float* done_dev,
                                   const float* truncation_dev, const int32_t* cdf_dev, int32_t* counts_dev, float* state_dev, float* cmd_dev,
                                   float* obs_dev, float* priv_patch_dev, void* stream) {
  const char* fn = "odk_curriculum_step";
  const void* const p[7] = {b, c, priv_dev, cdf_dev, counts_dev, state_dev, cmd_dev};
  static const char* const name[7] = {"batch", "curriculum", "priv_dev", "cdf_dev", "counts_dev", "state_dev", "cmd_dev"};
  for (int i = 0; i < 7; i++) if (!p[i]) return fail(ODK_ERR_INVALID, "%s: null %s", fn, name[i]);
  if (done_dev && !truncation_dev) return fail(ODK_ERR_INVALID, "%s: null truncation_dev (with a done_dev: a fall is a done step that is no truncation)", fn);
  if (cmd_dev != b->d_cmd || b->cmd_stride != 7)
    return fail(ODK_ERR_INVALID, "%s: cmd_dev is not the command buffer bound to the batch with row stride 7 (odk_batch_bind_commands)", fn);
  int nbins;
  if (int rc = curriculum_grid(fn, c, &nbins)) return rc;
  if (c->period < 1) return fail(ODK_ERR_INVALID, "%s: period = %d (at least 1 step)", fn, (int)c->period);
  if (c->skip < 0) return fail(ODK_ERR_INVALID, "%s: skip = %d (0 or more steps)", fn, (int)c->skip);
  if (c->min_samples < 0) return fail(ODK_ERR_INVALID, "%s: min_samples = %d (0 or more)", fn, (int)c->min_samples);
  Launch g; if (int rc = launch_on(b, 1, &g)) return rc;
  const size_t n = (size_t)b->nenv;
  // (a priv_dev that is also patched is the same rows: the columns read are none of the columns stored; any other takes part as a range of its own)
  const Span s[7] = {{"counts_dev", counts_dev, 8 * (size_t)nbins}, {"state_dev", state_dev, 4 * n * ODK_CURR_NSTATE}, {"cmd_dev", cmd_dev, 4 * n * 7},
                     {"obs_dev", obs_dev, 4 * n * g.nobs}, {"priv_patch_dev", priv_patch_dev, 4 * n * g.npriv}, {"cdf_dev", cdf_dev, 4 * (size_t)nbins},
                     {"priv_dev", priv_patch_dev == priv_dev ? nullptr : priv_dev, 4 * n * g.npriv}};
  if (int rc = spans_apart(fn, s, 7)) return rc;
  hipLaunchKernelGGL(curriculum_step_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, *c, nbins, priv_dev, g.npriv, g.nobs, done_dev,
                     truncation_dev, (const int*)cdf_dev, (int*)counts_dev, state_dev, cmd_dev, obs_dev, priv_patch_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// curriculum_update_kernel: one wave.  Lane l walks bins l, 64 + l, ...  Pass 1 only reads counts and levels and parks every bin's new level in
// cdf, which nothing reads before pass 2; the barrier between the passes puts every lane's reads of its neighbours' counters in front of the
// first store that zeroes one or rewrites a level.  Pass 2 reads back its own stores only.  The prefix sums are a __shfl_up scan per 64 bins
// with a running carry: no LDS.  All integers.
__device__ __forceinline__ bool curriculum_promoted(const int* __restrict__ counts, int bin, int min_tries, float rate) {
#pragma clang fp contract(off)
  const int tries = counts[2 * bin], wins = counts[2 * bin + 1];
  return tries >= min_tries && (float)wins >= rate * (float)tries;
}
__global__ void __launch_bounds__(64) curriculum_update_kernel(const odk_curriculum c, int nbins, int* levels, int* cdf, int* counts, int* stats) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int n1 = c.n[1], n2 = c.n[2], n0 = c.n[0];
  const int chunks = (nbins + 63) >> 6;
  int judged = 0, promoted = 0, tries_judged = 0;
  for (int k = 0; k < chunks; k++) {
    const int bin = k * 64 + lane;
    if (bin >= nbins) continue;
    const int iz = bin % n2, iy = (bin / n2) % n1, ix = bin / (n1 * n2);
    const bool self = curriculum_promoted(counts, bin, c.min_tries, c.promote_rate);
    int P = self ? 1 : 0;
    if (ix > 0) P += curriculum_promoted(counts, bin - n1 * n2, c.min_tries, c.promote_rate) ? 1 : 0;
    if (ix < n0 - 1) P += curriculum_promoted(counts, bin + n1 * n2, c.min_tries, c.promote_rate) ? 1 : 0;
    if (iy > 0) P += curriculum_promoted(counts, bin - n2, c.min_tries, c.promote_rate) ? 1 : 0;
    if (iy < n1 - 1) P += curriculum_promoted(counts, bin + n2, c.min_tries, c.promote_rate) ? 1 : 0;
    if (iz > 0) P += curriculum_promoted(counts, bin - 1, c.min_tries, c.promote_rate) ? 1 : 0;
    if (iz < n2 - 1) P += curriculum_promoted(counts, bin + 1, c.min_tries, c.promote_rate) ? 1 : 0;
    cdf[bin] = min(ODK_CURR_LMAX, levels[bin] + P);
    const int tries = counts[2 * bin];
    if (tries >= c.min_tries) { judged++; tries_judged += tries; }
    if (self) promoted++;
  }
  __syncthreads();
  int carry = 0;
  for (int k = 0; k < chunks; k++) {   // uniform: every lane takes part in the shuffles
    const int bin = k * 64 + lane;
    const bool in = bin < nbins;
    int x = 0;
    if (in) {
      x = cdf[bin];
      levels[bin] = x;
      if (counts[2 * bin] >= c.min_tries) { counts[2 * bin] = 0; counts[2 * bin + 1] = 0; }
    }
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const int y = __shfl_up(x, dlt, 64);
      if (lane >= dlt) x += y;
    }
    if (in) cdf[bin] = carry + x;
    carry += __shfl(x, 63, 64);
  }
#pragma unroll
  for (int dlt = 32; dlt > 0; dlt >>= 1) {
    judged += __shfl_down(judged, dlt, 64); promoted += __shfl_down(promoted, dlt, 64); tries_judged += __shfl_down(tries_judged, dlt, 64);
  }
  if (lane == 0) {
    stats[ODK_CURR_STAT_UPDATES] += 1; stats[ODK_CURR_STAT_JUDGED] += judged; stats[ODK_CURR_STAT_PROMOTED] += promoted;
    stats[ODK_CURR_STAT_TRIES] += tries_judged;
  }
}

extern "C" int odk_curriculum_update(const odk_batch* b, const odk_curriculum* c, int32_t* levels_dev, int32_t* cdf_dev, int32_t* counts_dev,
                                     int32_t* stats_dev, void* stream) {
  const char* fn = "odk_curriculum_update";
  const void* const p[6] = {b, c, levels_dev, cdf_dev, counts_dev, stats_dev};
  static const char* const name[6] = {"batch", "curriculum", "levels_dev", "cdf_dev", "counts_dev", "stats_dev"};
  for (int i = 0; i < 6; i++) if (!p[i]) return fail(ODK_ERR_INVALID, "%s: null %s", fn, name[i]);
  int nbins;
  if (int rc = curriculum_grid(fn, c, &nbins)) return rc;
  if (c->min_tries < 1) return fail(ODK_ERR_INVALID, "%s: min_tries = %d (at least 1: a bin without a try is not judged)", fn, (int)c->min_tries);
  const Span s[4] = {{"levels_dev", levels_dev, 4 * (size_t)nbins}, {"cdf_dev", cdf_dev, 4 * (size_t)nbins}, {"counts_dev", counts_dev, 8 * (size_t)nbins},
                     {"stats_dev", stats_dev, 16}};
  if (int rc = spans_apart(fn, s, 4)) return rc;
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(curriculum_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *c, nbins, (int*)levels_dev, (int*)cdf_dev,
                     (int*)counts_dev, (int*)stats_dev);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// ---- log replay (include/odk.h "Log replay": the table layout and the definitions these two kernels restate).  One 16-lane row per env,
// lane = actuator, no LDS, no row sums.  Contraction is off, so a float32 host restatement has the bits.
namespace log_at {   // offsets into a row of the table, after ODK_LOG_COMMAND [7] and ODK_LOG_ACTION [nu]
__host__ __device__ constexpr int pos(int nu) { return 7 + nu; }
__host__ __device__ constexpr int vel(int nu) { return 7 + 2 * nu; }
__host__ __device__ constexpr int gyro(int nu) { return 7 + 3 * nu; }
__host__ __device__ constexpr int accel(int nu) { return 10 + 3 * nu; }
__host__ __device__ constexpr int contact(int nu) { return 13 + 3 * nu; }
}  // namespace log_at
static_assert(log_at::contact(ODK_NU) + 2 == ODK_LOG_ROW(ODK_NU), "the contacts end the row");

// The action and the command of the step about to run, issued before odk_step: sched_apply_kernel's clock (STEPS, STEPS - 1 once ENDED is
// set), clamped into the table.  (The clamp is taken on the float: whatever the slot holds, the row read lies inside the table.)
__global__ void __launch_bounds__(256) log_apply_kernel(const float* __restrict__ log, int nrow, int nu, const float* __restrict__ track,
                                                        float* __restrict__ action, float* __restrict__ cmd, int cmd_stride, int nenv) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, e = t >> 4, u = t & 15;
  if (e >= nenv) return;
  const float* T = track + (size_t)e * ODK_TRACK_NACC;
  const float s = T[ODK_TRACK_ENDED] != 0.0f ? T[ODK_TRACK_STEPS] - 1.0f : T[ODK_TRACK_STEPS];
  const int k = (int)fminf(fmaxf(s, 0.0f), (float)(nrow - 1));
  const float* L = log + (size_t)k * ODK_LOG_ROW(nu);
  if (u < nu) action[(size_t)e * nu + u] = L[ODK_LOG_ACTION + u];
  if (u < 7) cmd[(size_t)e * cmd_stride + u] = L[ODK_LOG_COMMAND + u];
}

extern "C" int odk_log_apply(const odk_batch* b, const float* log_dev, int nrow, const float* track_acc_dev, float* action_dev, void* stream) {
  const char* fn = "odk_log_apply";
  const void* const p[4] = {b, log_dev, track_acc_dev, action_dev};
  static const char* const name[4] = {"batch", "log_dev", "track_acc_dev", "action_dev"};
  for (int i = 0; i < 4; i++) if (!p[i]) return fail(ODK_ERR_INVALID, "%s: null %s", fn, name[i]);
  if (!b->d_cmd) return fail(ODK_ERR_INVALID, "%s: no commands bound (odk_batch_bind_commands)", fn);
  if (nrow < 1) return fail(ODK_ERR_INVALID, "%s: nrow = %d (a table has at least one row)", fn, nrow);
  const int nu = b->model.h.nu;
  if (int rc = fits_row16(fn, nu)) return rc;
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  // the bound buffer is the caller's own device memory (odk_command_schedule_apply's note): this launch is the one writer
  hipLaunchKernelGGL(log_apply_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, log_dev, nrow, nu, track_acc_dev, action_dev,
                     const_cast<float*>(b->d_cmd), b->cmd_stride, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

// Residuals of one replayed step against the table's row of that step, issued between odk_step and odk_tracking_accumulate (the ENDED /
// STEPS contract of push_kernel).  Lane u owns the ODK_REPLAY_NSLOT floats of [e][u]; only a sample inside the table stores anything.
__global__ void __launch_bounds__(256) replay_kernel(const float* __restrict__ priv, int npriv, int nobs, int nu, const float* __restrict__ done,
                                                     const float* __restrict__ track, const float* __restrict__ log, int nrow, float vel_scale,
                                                     float* __restrict__ acc, int nenv) {
#pragma clang fp contract(off)
  const Row16 th = row16(priv, npriv, nobs, nu, done, track, nenv);
  const int u = th.u;
  const float s = track[th.row * ODK_TRACK_NACC + ODK_TRACK_STEPS];      // first-episode steps before the one that just ran: its index
  if (!th.sample || !(s >= 0.0f && s < (float)nrow)) return;
  const float *Q = th.Q, *L = log + (size_t)(int)s * ODK_LOG_ROW(nu);
  float* A = acc + (th.row * 16 + u) * ODK_REPLAY_NSLOT;
  if (u < nu) {
    const float dp = Q[priv_at::JOINT_POS + u] - L[log_at::pos(nu) + u];
    const float dv = Q[priv_at::joint_vel(nu) + u] * vel_scale - L[log_at::vel(nu) + u];
    A[ODK_REPLAY_POS_ERR_SUM] += dp;
    A[ODK_REPLAY_POS_ERR_SQ] += dp * dp;
    A[ODK_REPLAY_VEL_ERR_SQ] += dv * dv;
    A[ODK_REPLAY_POS_ERR_PEAK] = fmaxf(A[ODK_REPLAY_POS_ERR_PEAK], fabsf(dp));
  }
  if (u < 3) {
    const float dg = Q[priv_at::GYRO + u] - L[log_at::gyro(nu) + u], da = Q[priv_at::ACCELEROMETER + u] - L[log_at::accel(nu) + u];
    A[ODK_REPLAY_GYRO_ERR_SQ] += dg * dg;
    A[ODK_REPLAY_ACCEL_ERR_SQ] += da * da;
  }
  if (u < 2) A[ODK_REPLAY_CONTACT_AGREE] += ((Q[priv_at::contact(nu) + u] != 0.0f) == (L[log_at::contact(nu) + u] > 0.5f)) ? 1.0f : 0.0f;
  if (u == 0) A[ODK_REPLAY_SAMPLES] += 1.0f;
}

extern "C" int odk_replay_accumulate(const odk_batch* b, const float* priv_dev, const float* done_dev, const float* truncation_dev,
                                     const float* track_acc_dev, const float* log_dev, int nrow, float* acc_dev, void* stream) {
  const char* fn = "odk_replay_accumulate";
  if (int rc = null_args(fn, b, priv_dev, done_dev, truncation_dev, track_acc_dev, acc_dev)) return rc;
  if (!log_dev) return fail(ODK_ERR_INVALID, "%s: null log_dev", fn);
  if (nrow < 1) return fail(ODK_ERR_INVALID, "%s: nrow = %d (a table has at least one row)", fn, nrow);
  const int nu = b->model.h.nu;
  if (int rc = fits_row16(fn, nu)) return rc;
  Launch g; if (int rc = launch_on(b, 16, &g)) return rc;
  hipLaunchKernelGGL(replay_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, priv_dev, g.npriv, g.nobs, nu, done_dev, track_acc_dev,
                     log_dev, nrow, b->cfg.dof_vel_scale, acc_dev, b->nenv);
  HIPCHK(hipGetLastError());
  return ODK_OK;
}

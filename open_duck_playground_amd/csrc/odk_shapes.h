// odk_shapes.h -- the compiled model shapes and the per-env layouts sized by them, shared by the env kernels (odk_env_kernels.h), the batch API
// (odk_engine.hip) and the host-only model loader (odk_model_load.hip): HBM record offsets, observation sizes, the random-draw streams, the env
// logic's LDS floats, the kernels' arguments, the `using Shape...` lines, ODK_SHAPES, the list every per-shape dispatch goes through, and the
// kernel sets (ODK_ENV_SET_...), one object per shape.  A new robot's three lines go in HERE.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/odk.h"
#include "odk_shape.h"

using namespace odk;   // (both includers' own; the generated odk_shapes_user.h names Shape<...> unqualified)

// ================================================================================================
// per-env HBM records (floats; ints stored bit-exact in float slots).  The carried info of joystick.py:278-302 + the wrappers' additions,
// sized by the robot's actuator count nu (the duck: 14 -> the offsets of rounds 1-5: LAST 7, LAST2 21, ..., AHIST 69, IMU 111, NINFO 141)
struct RecLay {
  int CMD, LAST, LAST2, LAST3, MT, AIR, PEAK, PUSH, AHIST, IMU, EPSTEPS, TRUNC, DONE, EPSUM, EPLEN, EPMET, KEY0, KEY1, CTR, STEP, PSTEP, PINT, IMI, LCON, NINFO;
};
constexpr RecLay rec_lay(int nu) {
  RecLay r{};
  r.CMD = 0; r.LAST = 7; r.LAST2 = r.LAST + nu; r.LAST3 = r.LAST2 + nu; r.MT = r.LAST3 + nu; r.AIR = r.MT + nu; r.PEAK = r.AIR + 2; r.PUSH = r.PEAK + 2;
  r.AHIST = r.PUSH + 2; r.IMU = r.AHIST + 3 * nu; r.EPSTEPS = r.IMU + 9; r.TRUNC = r.EPSTEPS + 1; r.DONE = r.TRUNC + 1; r.EPSUM = r.DONE + 1; r.EPLEN = r.EPSUM + 1;
  r.EPMET = r.EPLEN + 1; r.KEY0 = r.EPMET + ODK_NMETRIC; r.KEY1 = r.KEY0 + 1; r.CTR = r.KEY1 + 1; r.STEP = r.CTR + 1; r.PSTEP = r.STEP + 1; r.PINT = r.PSTEP + 1;
  r.IMI = r.PINT + 1; r.LCON = r.IMI + 1; r.NINFO = r.LCON + 1;
  return r;
}
static_assert(rec_lay(14).AHIST == 69 && rec_lay(14).IMU == 111 && rec_lay(14).EPSTEPS == 120 && rec_lay(14).KEY0 == 133 && rec_lay(14).NINFO == 141, "the duck's record layout");

// Observation row strides (joystick.py:570-615 / standing.py:524-565) for a robot with nu actuators: the duck's 101 / 212 and 85 / 153
constexpr int obs_nobs(int nu, bool standing) { return standing ? 15 + 5 * nu : 17 + 6 * nu; }
constexpr int obs_npriv(int nu, bool standing) { return obs_nobs(nu, standing) + 26 + 3 * nu + (standing ? 0 : 43); }
static_assert(obs_nobs(14, false) == ODK_NOBS && obs_npriv(14, false) == ODK_NPRIV && obs_nobs(14, true) == ODK_NOBS_STANDING && obs_npriv(14, true) == ODK_NPRIV_STANDING, "include/odk.h");
// Random draws of an env step (stream definition shared with oracle/odk_oracle_env.c): 0 action delay | 2, 3 push | 4-6 gyro | 7-9 accelerometer |
// 10-12 gravity | 13 .. 12 + nu joint angles | 13 + nu .. 12 + 2 nu joint velocities | 13 + 2 nu .. 19 + 2 nu command | 20 + 2 nu zero-command
// (the duck: 13, 27, 41, 48).  Reset stream: 0-1 dxy | 2 yaw | 3 .. 2 + nu joint scale | 3 + nu .. 8 + nu base qvel | 9 + nu .. 15 + nu command |
// 16 + nu zero-command | 17 + nu push interval (the duck: 17, 23, 30, 31).
constexpr int draw_qvel(int nu) { return 13 + nu; }
constexpr int draw_cmd(int nu) { return 13 + 2 * nu; }
constexpr int draw_count(int nu) { return (17 + 2 * nu + 1) & ~1; }      // draws 4 .. 20 + 2 nu, rounded up to whole generator blocks (the duck: 46)

template <class S> struct Rec {
  static constexpr RecLay L = rec_lay(S::NU);
  static constexpr int NOBS = obs_nobs(S::NU, false), NPRIV = obs_npriv(S::NU, false);
  static constexpr int INFO = S::NQ + 2 * S::NV;
  static constexpr int SIZE = ((INFO + L.NINFO + 3) / 4) * 4;
  static constexpr int FOBS = S::NQ + 2 * S::NV;
  static constexpr int FSIZE = ((FOBS + NOBS + NPRIV + 3) / 4) * 4;
};

// extra LDS used by the env logic, placed after the physics arrays
template <class S> struct EnvL {
  static constexpr int O_INFO = S::TOTAL;               // [N_INFO] the carried info (Rec::L)
  static constexpr int O_ACT = O_INFO + S::N_INFO;      // [N_ACT] this step's action, then the imitation phase (2)
  static_assert(rec_lay(S::NU).NINFO <= S::N_INFO && S::NU + 2 <= S::N_ACT, "Shape::N_INFO / N_ACT");
  // epilogue only, on top of the motion-column buffers (dead after the last forward pass): this step's random draws and the
  // reference motion (evaluated in the epilogue: reward and privileged obs are its only readers)
  static constexpr int NDRAW = draw_count(S::NU);
  static constexpr int O_NZ = S::O_BUF6;                          // [NDRAW] draw_block
  static constexpr int O_REF = S::O_BUF6 + ((NDRAW + 3) / 4) * 4;   // [40] current_reference_motion
  static_assert(((NDRAW + 3) / 4) * 4 + 40 <= 6 * S::NVR && NDRAW <= 64, "draws + reference motion must fit in BUF6");
  static constexpr int O_PRIV = S::O_M;            // [NPRIV] aliases M|HL (dead after the last forward)
  static constexpr int TOTAL = O_ACT + S::N_ACT;
  static_assert(TOTAL == S::ENV_STRIDE, "Shape::ENV_STRIDE is the distance between the two env images of a workgroup");
  static_assert(S::NMR + S::NHR >= Rec<S>::NPRIV, "privileged obs must fit in the M|HL region");
  // per WORKGROUP, behind the envs' images: static tables shared by the envs of the workgroup
  static constexpr int SHARED = S::SHARED;       // DevModel::R_ent | contact-row constants (forward_env: RT, CT)
  static constexpr int wg_floats(int envs) { return envs * TOTAL + SHARED; }
};

// ================================================================================================
// what the host passes to the env kernels
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
  const int32_t* delay;   // [nenv][delay_stride] bound action delays (odk_batch_bind_action_delays): the action-history row 0..2 env e's step
  int delay_stride;       // applies, negative: the sampled one; or null: every env samples.  A uniform pointer test, behind every older field
};

// DR buffer layout per env
template <class S> struct DRL {
  static constexpr int MASS = 0, IPOS = S::NB, FRL = S::NB + 3, ARM = FRL + S::NU, Q0 = ARM + S::NU, KP = Q0 + S::NU, SIZE = KP + S::NU;
};

using ShapeA = Shape<21, 20, 18, 14, 15, 145, 170, 76, 10, 15>;   // flat_terrain
using ShapeB = Shape<31, 30, 18, 14, 25, 285, 385, 86, 15, 25>;   // *_backlash
// the same two with the elliptic-cone code compiled in (Shape::ELL): launched for a duck model with <option cone="elliptic"> (plane floor, or
// the backlash model's height field), 32 lanes per env; the default kernels above stay the instruction streams they were
using ShapeAE = Shape<21, 20, 18, 14, 15, 145, 170, 76, 10, 15, true>;
using ShapeBE = Shape<31, 30, 18, 14, 25, 285, 385, 86, 15, 25, true>;
// A robot that is not the duck (tests/assets/tail_biped.xml: biped with a five-link tail, 21 dofs, 15 actuators, 19 bodies,
// box feet): reset / step / physics kernels -- the env kernels' task logic is joystick.py's with the robot's own tables (rec_lay, obs_nobs: sized
// by Shape::NU; actuators, default pose, sites and sensor addresses from the ModelBlob), the imitation reward with a joint map of its own (odk_batch_set_imitation_joints), Standing
// with head joints of its own (odk_batch_set_head_joints).  What adding it
// took: this line, the dispatch lines below that name it (tools/new_shape.py prints them for an XML), and nothing in odk_shape.h beyond
// admitting nv = 21 to the chain solver.
using ShapeC = Shape<22, 21, 19, 15, 16, 156, 181, 78, 10, 15>;
// A second one (tests/assets/biped12.xml): a biped with SIX-dof legs (hip yaw / roll / pitch, knee, ankle pitch / roll), 18 dofs, 12 actuators,
// 16 bodies: serial chains of six (the chain solve's block size is the shape's CL), contact wrenches in their own floats (16 bodies' cfrc | crb
// region is too small for them).  Env kernels as for ShapeC (12 actions, observations 89 / 194 floats).
using ShapeD = Shape<19, 18, 16, 12, 13, 135, 171, 72, 12, 18, false, 6, true>;      // (chains of six; equality rows and elliptic cones compiled in, as ShapeC)
// A biped with arms (tests/assets/biped_arms.xml): biped12's legs and two arms on the trunk (shoulder pitch, elbow), 22 dofs, 16 actuators, 20
// bodies: FOUR serial chains below the floating base (6 / 6 / 2 / 2), the chain solve's fourth 8-lane group (Shape::NCH).  The same shape takes
// tests/assets/biped_arms_between.xml (the arms declared between the legs).  Env kernels as for ShapeC (16 actions, observations 113 / 230 floats).
using ShapeE = Shape<23, 22, 20, 16, 17, 165, 201, 80, 11, 17, false, 6, true, 4>;
// The compiled model shapes, by the index odk_model carries: every per-shape dispatch of the host code below goes through this list, so a
// new robot is ONE `using` line above, ONE entry here and ONE kernel set below (tools/new_shape.py <xml> prints all three).  Entries 0 and 1
// are the duck's two models (their cone / height-field / 64-lane instantiations are chosen in launch()); entries from 2 on run reset / step /
// physics kernels at 32 lanes per env on a plane floor.
// Robots added without editing this file: `python tools/new_shape.py robot.xml --add` writes csrc/odk_shapes_user.h -- one `using ShapeU<k> = Shape<...>;`
// line and one `#define ODK_ENV_SET_U<k>(X) X(ShapeU<k>, 32, 0)` per robot, and `#define ODK_USER_SHAPES(X) X(4, ShapeU0) ...` -- and builds the
// new set's object.
#if __has_include("odk_shapes_user.h")
#include "odk_shapes_user.h"
#endif
#ifndef ODK_USER_SHAPES
#define ODK_USER_SHAPES(X)
#endif
// Further robots that ship with the library take indices from 16 on, clear of the user shapes (4, 5, ...: tools/new_shape.py --add).
#define ODK_SHIPPED_SHAPES(X) X(16, ShapeE)
#define ODK_SHAPES(X) X(0, ShapeA) X(1, ShapeB) X(2, ShapeC) X(3, ShapeD) ODK_SHIPPED_SHAPES(X) ODK_USER_SHAPES(X)

// The kernel sets: one shape each, with all of its instantiations X(shape, lanes per env, HF) -- HF the floor: 0 plane, 1 height field under hull
// feet, 2 height field under sphere / capsule feet.  Each set is ONE object: odk_env_unit.hip compiled with -DODK_ENV_SET=<name> instantiates
// launch_sg, and with it the reset / step / debug step / physics kernels, for the set's entries; the Makefile reads the names off these
// #define lines.  A shape's instantiations stay in one object because their code depends on each other's presence: the floor variants of one
// (shape, lanes) share out-of-line device functions (foot_foot_sat, prim_contacts, hfield_prim_floor, dump_lds), compiled against the callers
// the compiler sees next to them, and the 32-lane kernels of the duck's shapes A and B were observed to come out as other instruction streams
// once their 64-lane kernels were compiled elsewhere (seen for these two shapes, the only ones with two lane counts; the cause was not
// looked into: profiles/engine_units/NOTES.md).  launch() (odk_engine.hip) chooses among the entries; one it names that no set holds is an
// undefined symbol when libodk.so links.  A new robot's third line is its set (32 lanes, plane floor); tools/new_shape.py --add writes a user
// shape's next to its alias.
#define ODK_ENV_SET_A(X) X(ShapeA, 32, 0) X(ShapeA, 64, 0)
#define ODK_ENV_SET_B(X) X(ShapeB, 32, 0) X(ShapeB, 32, 1) X(ShapeB, 32, 2) X(ShapeB, 64, 0)
#define ODK_ENV_SET_AE(X) X(ShapeAE, 32, 0)
#define ODK_ENV_SET_BE(X) X(ShapeBE, 32, 0) X(ShapeBE, 32, 1)
#define ODK_ENV_SET_C(X) X(ShapeC, 32, 0)
#define ODK_ENV_SET_D(X) X(ShapeD, 32, 0)
#define ODK_ENV_SET_E(X) X(ShapeE, 32, 0)

// launch one instantiation's reset / step / physics kernel (`which`) on a stream: defined in odk_env_kernels.h, instantiated by the sets' objects
enum { K_RESET = 0, K_STEP = 1, K_PHYS = 2 };
template <class S, int G, int HF> hipError_t launch_sg(int which, const KArgs& a, hipStream_t st);

// occupancy by construction: 2 waves / SIMD = 8 single-wave workgroups per CU need <= 160 KiB / 8 of LDS per workgroup (2 envs)
#ifndef ODK_PROFILE   // (the phase-timing build carries 20 extra floats per env and may run 7 workgroups per CU)
static_assert(EnvL<ShapeA>::wg_floats(2) * sizeof(float) <= 20480, "shape A: LDS image too large for 8 workgroups per CU");
static_assert(EnvL<ShapeB>::wg_floats(2) * sizeof(float) <= 20480, "shape B: LDS image too large for 8 workgroups per CU");
#endif

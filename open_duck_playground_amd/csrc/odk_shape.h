// odk_shape.h -- what a compiled model shape IS, for host and device code alike: the env config's device copy (EnvCfg), the per-env LDS
// layout (Shape<>), and the per-lane statics (Statics, ActSt / FlSt / HotSt) with compute_statics, which the model loader runs on the host.
// Nothing here needs a device intrinsic: the host-only model loader and the batch API include this layer (through odk_shapes.h) and none
// above it.  Stands on odk_model.h alone.
#pragma once
#include "odk_model.h"

namespace odk {

struct EnvCfg {  // device copy of odk_env_config
  float ctrl_dt, action_scale, dof_vel_scale, max_motor_velocity;
  float noise_level, noise_gyro, noise_accelerometer, noise_gravity, noise_joint_vel;
  float qpos_noise_scale[16];
  float reward_scales[7];
  float tracking_sigma;
  float push_enable, push_interval_range[2], push_magnitude_range[2];
  float cmd_range[7][2];
  int use_imitation, use_motor_speed_limits, autoreset, episode_length, n_substeps;
  int kind, nobs, npriv;   // env kind (0 Joystick, 1 Standing) and its output row strides
  float reset_base_qvel;
};

// ------------------------------------------------------------------------------------------------
// LDS layout (floats), per environment.  Component-major (SoA) arrays: X[k * N + item].
template <int NQ_, int NV_, int NB_, int NU_, int NJ_, int NM_, int NH_, int NROW_, int DT_, int DV_, bool CONE_ = false, int CL_ = -1, bool OPT_ = false, int NCH_ = 3>
struct Shape {
  static constexpr int NQ = NQ_, NV = NV_, NB = NB_, NU = NU_, NJ = NJ_, NM = NM_, NH = NH_, NROW = NROW_;
  static constexpr int DT = DT_;    // max dof depth, kinematic tree
  static constexpr int DV = DV_;    // max dof depth, virtual (Hessian) tree
  static constexpr int NCROW = 48;  // contact rows
  // Twin dofs (the backlash model, nv 30): solves run on the reduced tree -- twins merged into their main dof, which is
  // the 20-dof robot's own tree (DevModel::paired; odk_kernels.h reduced_rhs / reduced_expand).
  static constexpr bool PAIRED = (NV_ == 30);
  // Hinges on one body: two only where a backlash twin shares its joint's body.  The joint-slot loops of forward_env's pose sweep run to
  // MAXJB and size their register arrays by it, so a shape without twins carries no second slot (its copies, zero fills and exec-mask
  // bookkeeping); the BodySt record keeps both slots.  The loader refuses a body with more hinges than its shape's MAXJB (select_shape).
  static constexpr int MAXJB = PAIRED ? 2 : 1;
  // <equality><joint> rows (DevModel::neq) are compiled into this shape's kernels: the third shape (tests/assets/tail_biped*.xml) -- the
  // duck's shapes have no equality and do not pay for the code
  static constexpr bool EQ = (NV_ == 21) || OPT_;      // (OPT_: a shape that asks for the optional constraint code -- equality rows, elliptic cones as a runtime switch)
  // <option cone="elliptic"> (DevModel::cone) is compiled into the same shape's kernels: a contact's four row lanes hold normal | tangent 1 |
  // tangent 2 | nothing instead of the four pyramid edges, and the cost of a contact is the cone's (odk_kernels.h "elliptic cones")
  static constexpr bool CONE = CONE_;                   // an instantiation that is ONLY launched for cone = 1 models: the pyramid code is compiled out
  static constexpr bool ELL = (NV_ == 21) || CONE_ || OPT_;    // (the duck's shapes: their own instantiations with CONE_ = true, launched for models with cone = 1 only)
  static constexpr int NVR = PAIRED ? 20 : NV_;    // reduced dofs
  static constexpr int NMR = PAIRED ? 145 : NM_;   // entries of the reduced tree layout
  static constexpr int NHR = PAIRED ? 170 : NH_;   // entries of the reduced virtual-tree layout
  static constexpr int DVR = PAIRED ? 15 : DV_;    // max dof depth, reduced virtual tree
  // workgroup-shared LDS tables behind the envs' images (odk_env_kernels.h load_shared): the packed reduced entries and the
  // contact-row constants.  (Friction-loss rows, actuator constants and the foot hull were tried there too: no gain, their
  // loads from the L2-resident model are already covered.)
  static constexpr int SH_CT = NMR, SH_HOT = SH_CT + 42;
  static constexpr int CL = CL_ >= 0 ? CL_ : ((NV_ == 20 || NV_ == 21 || PAIRED) ? 5 : 0);   // max (reduced) chain length for chain_solve: every compiled shape is a floating base + <= NCH serial chains of <= CL (reduced) dofs (0: generic path)
  static constexpr int NCH = NCH_;  // serial chains below the floating base that chain_solve eliminates: chain c on lanes 8 c .. 8 c + 6 (a biped with arms: 4)
  static_assert(NCH >= 1 && NCH <= 4, "chain_solve: one 8-lane group per chain, 32 lanes");
  // persistent over the env step
  static constexpr int O_QPOS = 0;
  static constexpr int O_QVEL = O_QPOS + NQ;
  static constexpr int O_WARM = O_QVEL + NV;
  static constexpr int O_CTRL = O_WARM + NV;
  // per-env effective model parameters (domain randomisation lands here)
  static constexpr int O_Q0 = O_CTRL + NU;     // qpos0
  static constexpr int O_MASS = O_Q0 + NQ;     // body_mass
  static constexpr int O_ARM = O_MASS + NB;    // dof_armature
  static constexpr int O_FRL = O_ARM + NV;     // dof_frictionloss
  static constexpr int O_KP = O_FRL + NV;      // actuator kp
  static constexpr int O_IPOS1 = O_KP + NU;    // body_ipos[1]
  // tree sweeps (component-major by body)
  static constexpr int O_XPOS = O_IPOS1 + 3;         // [3][NB]
  static constexpr int O_XQUAT = O_XPOS + 3 * NB;    // [4][NB]
  static constexpr int O_CVEL = O_XQUAT + 4 * NB;    // [6][NB]
  static constexpr int O_CACC = O_CVEL + 6 * NB;     // [6][NB] velocity-dependent part of cacc (gravity folded in)
  static constexpr int O_CFRC = O_CACC + 6 * NB;     // [6][NB] local then subtree-accumulated bias force
  static constexpr int O_CRB = O_CFRC + 6 * NB;      // [10][NB] cinert then composite inertia
  // matrix work runs on the REDUCED dofs (twins merged, DevModel::paired): one motion column per reduced dof
  static constexpr int O_CDOF = O_CRB + 10 * NB;     // [6][NVR]
  static constexpr int O_BUF6 = O_CDOF + 6 * NVR;    // [6][NVR] crb*cdof -> K_L*cdof
  static constexpr int O_BUF6B = O_BUF6 + 6 * NVR;   // [6][NVR] K_R*cdof
  static constexpr int O_M = O_BUF6B + 6 * NVR;      // [NMR] sparse reduced inertia (rows by ancestor depth; twin pairs: no armature)
  static constexpr int O_HL = O_M + NMR;             // [NHR] reduced inertia / Hessian with the diagonal terms, and its factor
  // dof vectors
  static constexpr int O_QFS = O_HL + NHR;           // qfrc_smooth
  static constexpr int O_QAS = O_QFS + NV;           // qacc_smooth
  static constexpr int O_X = O_QAS + NV;             // current qacc iterate
  static constexpr int O_MA = O_X + NV;              // scratch: per-dof friction-row hand-over
  static constexpr int O_GRAD = O_MA + NV;           // search direction
  static constexpr int O_MV = O_GRAD + NV;           // scratch: per-dof friction-row hand-over
  // constraint rows
  static constexpr int O_D = O_MV + NV;              // efc_D (0 = structurally inactive row)
  static constexpr int O_AREF = O_D + NROW;
  static constexpr int O_JAR = O_AREF + NROW;        // J qacc - aref (contact rows)
  static constexpr int O_JV = O_JAR + NROW;          // J search (scratch: candidate Jaref, forces, Hessian diagonal addend)
  static constexpr int O_SC = O_JAR;                 // [2][NJ] sin/cos of the half joint angles: P0 -> P1 only, ALIASES jar (born in P9)
  static_assert(2 * NJ <= NROW, "sin/cos must fit in the jar rows");
  // [NCROW][6] contact row wrenches [r x dir; dir]: ALIAS cfrc|crb, which are dead once the bias forces and M entries exist (P3/P4; W is
  // born in P8) -- where that region is large enough (18 bodies); a smaller robot gets its own floats behind the image
  static constexpr bool W_FITS = 6 * NCROW <= 16 * NB;
  static constexpr int O_CDIST = O_JV + NROW;        // [12]
  static constexpr int O_CR = O_CDIST + NCON;        // [12][3] contact position relative to the base origin
  static constexpr int O_SCR = O_CR + 3 * NCON;      // scratch: foot twists, wrenches, 6x6 blocks, sensor inputs
  // scratch sub-offsets
  static constexpr int S_VF = 0;      // [2][6] foot twist of the current vector
  static constexpr int S_FF = 12;     // [2][6] foot wrench sums
  static constexpr int S_K = 24;      // [3][36] K_L, K_R, K_X
  static constexpr int S_FR = S_K;    // [8][9] frames of the floor contacts (height field / primitive feet): contact phase -> row phase only, ALIASES
                                      // the K blocks (born in the solver).  NOT in the row arrays: the foot-foot routine's hull copies live there.
  static constexpr int S_VF2 = 132;   // [2][6] second foot twist (warmstart candidate)
  static constexpr int S_FFX = 144;   // [6] wrench sum of the foot-foot rows
  static constexpr int S_EQ = 150;    // [EQ_MAX] equality rows: the Hessian's off-diagonal addend -D c (force phase -> Hessian entries; the solve's scratch runs over it afterwards)
  // the chain solve's scratch starts at S_K and takes NCH CL 7 + 27 floats (three chains: 156 for chains of five, up to S_MISC; 177 for chains of six;
  // four chains of six: 219): it runs over
  // S_VF2 / S_FFX / S_EQ, which are dead by then -- but never over the misc scalars, which the env kernels' epilogue reads (foot heights, gravity)
  static constexpr int S_SOLVE_END = S_K + 7 * NCH * CL + 27;
  static constexpr int S_MISC = S_SOLVE_END > 156 ? S_SOLVE_END : 156;  // misc scalars (16)
  static constexpr int S_PROF = S_MISC + 16;   // [20] per-phase cycle counters (ODK_PROFILE builds)
  static constexpr int S_PROF2 = S_PROF + 20;  // [16] height-field contacts: hull setup, cull pass, register loads, pair loop, iterations, list length, -, -,
                                               //      then inside a pair: select + prism, face query, Gauss-map tests, passing pairs, faces / polygons, clip + manifold, merge
  static constexpr int S_PROF3 = S_PROF2 + 16; // [4] line search: passes of the bracketing loop, summed over the forwards (lane 0)
#ifdef ODK_PROFILE
  static constexpr int N_SCR = S_PROF3 + 4;
#else
  static constexpr int N_SCR = ((S_MISC + 16 + 3) / 4) * 4;      // no S_PROF slots outside profile builds (172 for chains of five)
#endif
  static constexpr int O_SENS = O_JV;                // sensordata[46]: born after the line search (P10, last substep only), ALIASES jv
  static_assert(NSENSD <= NROW, "sensordata must fit in the jv rows");
  static constexpr int O_ACTF = O_SCR + N_SCR;       // actuator_force
  static constexpr int O_QACC = O_X;                 // qacc of the last forward == final iterate
  // path rows of shapes with EQ (<equality><connect | weld>, DevModel::neqp): wrenches [EQP_ROWS][12] | J [EQP_ROWS][NV] | D | aref | residual
  static constexpr int O_EQP = ((O_ACTF + NU + 3) / 4) * 4;
  static constexpr int EQP_W = 0, EQP_J = 12 * EQP_ROWS, EQP_D = EQP_J + EQP_ROWS * NV, EQP_AREF = EQP_D + EQP_ROWS, EQP_POS = EQP_AREF + EQP_ROWS;
  static constexpr int N_EQP = EQ ? ((EQP_POS + EQP_ROWS + 3) / 4) * 4 : 0;
  static constexpr int O_WX = O_EQP + N_EQP;         // the contact row wrenches of a robot with fewer than 18 bodies
  static constexpr int O_W = W_FITS ? O_CFRC : O_WX;
  static constexpr int TOTAL = O_WX + (W_FITS ? 0 : 6 * NCROW);
  // the env logic's floats behind the physics image (odk_shapes.h EnvL): the carried info (43 + 7 NU floats, rec_lay) and this step's action + the
  // imitation phase, both rounded up to whole float4s (the duck: 144 + 16)
  static constexpr int N_INFO = ((43 + 7 * NU + 3) / 4) * 4, N_ACT = ((NU + 2 + 3) / 4) * 4;
  static constexpr int ENV_STRIDE = TOTAL + N_INFO + N_ACT;   // floats between the images of the two envs of a workgroup (odk_shapes.h EnvL::TOTAL)
  // The model's uniform floats of the substep (DevModel::hot_f) as a third shared table at SH_HOT, read by LDS broadcast instead of an L2
  // round trip -- for a shape whose two-env workgroup has the room: the HOT_NF floats must not cost a workgroup per CU (160 KiB of LDS,
  // 8 single-wave workgroups at most).  A shape without the room keeps the loads from the model.
  static constexpr int wgs_per_cu(int floats) { return 163840 / (4 * floats) > 8 ? 8 : 163840 / (4 * floats); }
  static constexpr bool HOT_LDS = wgs_per_cu(2 * ENV_STRIDE + SH_HOT + HOT_NF) == wgs_per_cu(2 * ENV_STRIDE + SH_HOT);
  static constexpr int SHARED = SH_HOT + (HOT_LDS ? HOT_NF : 0);
};

// ------------------------------------------------------------------------------------------------
// Per-lane static data, loaded once per launch.  A lane plays several roles (body `lane`, dof `lane`,
// joint `lane`, hull vertex `lane`, a few matrix entries and constraint rows); roles beyond the
// model's counts are disabled by their flags.
// Persistent part: what the factor / solve / solver phases need all the time (kept small: register pressure
// decides whether two wavefronts fit on a SIMD).
template <class S, int G>
struct Statics : LaneSt {   // (data members: odk_model.h LaneSt)
  static constexpr int NME = (S::NMR + G - 1) / G;  // reduced inertia entries per lane
  static constexpr int NHE = (S::NHR + G - 1) / G;  // reduced virtual-tree Hessian entries per lane
  static_assert((S::NVR + 1) / 2 <= 16, "LaneSt::m_adr");
};
// Phase-local statics: fetched from the model (L1/L2-resident, one batch of loads per phase and substep)
// right where they are used, so they do not occupy registers for the rest of the substep.
// (BodySt: odk_model.h -- the per-body records are part of the device model)
struct ActSt { float bias2, clo, chi, flo, fhi; int climited, flimited; };
struct FlSt { float D, R, b; int dof; };

// The same three records held over the whole launch instead (plane-floor kernels: ~40 registers are free there since round 3, and
// each of these loads sat exposed right behind a phase hand-off in every substep)
// ve: the 17th hull vertex of the lane's foot; pk: DevModel::hot_pk, the model's wave-uniform small integers as three packed words (held in
// vector registers; forward_env makes them uniform once per substep and extracts every field on the scalar unit); np: the lane's record of
// the subtree fold (DevModel::np_rec: the six sources, the target and the count as byte fields in two registers -- as eight plain registers
// the lists had cost 1 %: profiles/load_waits/NOTES.md).  (The limit rows' records the same way: over the register budget.)
struct HotSt { ActSt as; FlSt fs; float vb[3], ve[3]; int pk[HOT_NPK], np[2]; };

template <class S>
__host__ __device__ inline void compute_statics(LaneSt& st, const DevModel* m, int lane) {
  {
    const bool on = lane >= 1 && lane < S::NJ;
    st.j_qadr = on ? m->jnt_qposadr[on ? lane : 0] : -1;
    st.j_dadr = m->jnt_dofadr[on ? lane : 0];
  }
  {
    st.cs_pk = 0;
    const int c = lane >> 3;
    if (c < S::NCH && c < m->nrchain) {
      const int f = m->rchain_first[c];
      st.cs_pk = m->rchain_len[c] | (m->red_depth[f] << 3) | (f << 8) | (m->red_Madr[f] << 14);
    }
    int tb = 0, tb2 = 0;
    if (lane < 21) { while ((tb + 1) * (tb + 2) / 2 <= lane) tb++; tb2 = lane - tb * (tb + 1) / 2; }
    else if (lane < 27) { tb = lane - 21; tb2 = 6; }
    st.cs_pk |= (tb << 24) | (tb2 << 27);
  }
  st.ch_first = 0; st.ch_len = 0;
  for (int c = 0; c < 4; c++)
    if (c < m->nrchain && lane >= m->rchain_first[c] && lane < m->rchain_first[c] + m->rchain_len[c]) { st.ch_first = m->rchain_first[c]; st.ch_len = m->rchain_len[c]; }
  {
    const int r = lane < S::NVR ? lane : 0;
    st.r_on = lane < S::NVR;
    st.r_depth = m->red_depth[r]; st.r_Madr = m->red_Madr[r]; st.r_ancmask = m->red_ancmask[r]; st.r_descmask = m->red_descmask[r];
    st.r_foot = st.r_on ? m->red_foot[r] : 0;
    if (!st.r_on) { st.r_ancmask = 0; st.r_descmask = 0; st.r_depth = 0; }
    // dofs are numbered parents first: j < lane can only be an ancestor of this lane's dof (entry in this lane's row, column
    // depth_j), j > lane only a descendant (entry in j's row, column depth_lane), j == lane the diagonal.  Unrelated pairs
    // (and lanes past the reduced dofs) point at CDOF[0][0], the angular x component of the base's x translation: always 0.
    const int rel = st.r_ancmask | st.r_descmask | (st.r_on ? (1 << r) : 0);
    for (int jp = 0; jp < (S::NVR + 1) / 2; jp++) {
      int pk = 0;
      for (int h = 0; h < 2; h++) {
        const int j = 2 * jp + h;
        int off = S::O_CDOF * 4;
        if (j < S::NVR && ((rel >> j) & 1)) off = (S::O_M + (j < r ? st.r_Madr + m->red_depth[j] : m->red_Madr[j] + st.r_depth)) * 4;
        pk |= off << (16 * h);
      }
      st.m_adr[jp] = pk;
    }
  }
  const int i = lane < S::NV ? lane : 0;
  st.d_on = lane < S::NV;
  st.d_body = m->dof_body[i];
  st.d_act = st.d_on ? m->dof_act[i] : -1;
  st.d_flrow = st.d_on ? m->dof_flrow[i] : -1;
  st.d_limrow = st.d_on ? m->dof_limrow[i] : -1;
  st.d_foot = st.d_on ? (m->foot_dofmask[0][i] | (m->foot_dofmask[1][i] << 1)) : 0;
  st.d_damping = m->dof_damping[i];
  st.d_lim_on = st.d_limrow >= 0;
  st.d_qadr = m->dof_qadr[i];
  st.d_lo = m->dof_range[i][0]; st.d_hi = m->dof_range[i][1];
  st.d_tkind = (S::PAIRED && st.d_on) ? m->dof_tkind[i] : 0;
  st.d_red = S::PAIRED ? m->dof_red[i] : i;   // column of this dof's motion vector in CDOF / BUF6
}

}  // namespace odk

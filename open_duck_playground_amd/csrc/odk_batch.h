// odk_batch.h -- private to libodk.so: the batch behind include/odk.h's opaque odk_batch, shared by the translation unit that owns it
// (odk_engine.hip) and the one that only reads it (odk_reports.hip).  Needs no compiled shape: the sizes that depend on one are filled in at creation.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "odk_host.h"

struct XTerms;   // odk_shapes.h (the batch holds a device pointer to one)

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return odk::fail(ODK_ERR_HIP, "%s: %s", #x, hipGetErrorString(_e)); } while (0)

struct odk_batch {
  odk_model model;
  int nenv, device, G;
  odk_env_config cfg;
  odk::DevModel* d_model = nullptr; odk::DevPRM h_prm; float* d_table = nullptr;
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

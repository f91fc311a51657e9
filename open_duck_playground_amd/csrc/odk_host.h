// odk_host.h -- what the host code of libodk.so's translation units shares: the loaded model (odk_model_load.hip fills it, the batch
// API in odk_engine.hip reads it) and the thread's error string behind odk_last_error (defined once, in odk_model_load.hip).
#pragma once
#include <vector>

#include "../../include/odk.h"
#include "odk_model.h"

// shape: the model's entry of ODK_SHAPES (odk_shapes.h); hfield: [nrow][ncol] in [0, 1]; adr_global_linvel: the imu's global_linvel sensor
// (reward library), -1: none
struct odk_model { odk::DevModel h; int shape; std::vector<float> hfield; int adr_global_linvel = -1; };

// set the thread's error string and return `code`
int odk_fail_(int code, const char* msg);
namespace odk {
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// observation row strides of a robot with nu actuators (obs_nobs / obs_npriv of odk_shapes.h)
void obs_sizes_nu(int nu, int env_kind, int* nobs, int* npriv);
}  // namespace odk

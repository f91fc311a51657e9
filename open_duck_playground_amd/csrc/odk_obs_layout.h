// odk_obs_layout.h -- where the fields of an observation row sit, for a robot with nu actuators (joystick.py:570-615 / standing.py:524-565): the
// one statement that the producer (build_obs_table, odk_model_load.hip) and the readers of finished rows (the report kernels,
// odk_reports.hip) share.  Plain constexpr: no shape, no HIP.
#pragma once
namespace odk {
namespace obs_at {   // observed side, offsets into the row (both tasks)
constexpr int GYRO = 0, ACCELEROMETER = 3;                       // [3] each
constexpr int COMMAND = 6;                                       // [7]
constexpr int JOINT_POS = 13;                                    // [nu] angle minus default
constexpr int joint_vel(int nu) { return 13 + nu; }              // [nu]
constexpr int last_act(int nu) { return 13 + 2 * nu; }           // [nu]
constexpr int last_last_act(int nu) { return 13 + 3 * nu; }      // [nu]
constexpr int contact(int nu, bool joystick) { return 13 + (joystick ? 6 : 5) * nu; }   // [2] left, right (Standing's row has no motor targets)
}  // namespace obs_at
namespace priv_at {   // privileged tail, offsets from the row's float nobs (both tasks up to the reference frame, which only Joystick has)
constexpr int GYRO = 0, ACCELEROMETER = 3, GRAVITY = 6, LOCAL_LINVEL = 9, GLOBAL_ANGVEL = 12;   // [3] each
constexpr int JOINT_POS = 15;                                    // [nu] angle minus default
constexpr int joint_vel(int nu) { return 15 + nu; }              // [nu]
constexpr int root_height(int nu) { return 15 + 2 * nu; }        // [1]
constexpr int actuator_force(int nu) { return 16 + 2 * nu; }     // [nu]
constexpr int contact(int nu) { return 16 + 3 * nu; }            // [2] left, right
constexpr int feet_linvel(int nu) { return 18 + 3 * nu; }        // [2][3]
constexpr int air_time(int nu) { return 24 + 3 * nu; }           // [2]
constexpr int ref_frame(int nu) { return 26 + 3 * nu; }          // [40] the reference-motion frame the reward read
constexpr int imitation_counter(int nu) { return 66 + 3 * nu; }  // [1], then the phase [2]
}  // namespace priv_at
namespace ref_at { constexpr int JOINT_POS = 0, JOINT_VEL = 16, CONTACT = 32, PLANAR_VEL = 34; }   // within the reference frame
}  // namespace odk

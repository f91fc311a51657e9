// odk_env_unit.hip -- one kernel set of the env engine per object: compiled once per ODK_ENV_SET_<name> of odk_shapes.h with
// -DODK_ENV_SET=<name> (Makefile: odk_env_<name>.o), it instantiates launch_sg -- and through it the reset / step / debug step / physics
// kernels -- for each (shape, lanes per env, floor) entry of that set.  The development build of one robot's kernels is its set's object.
#ifndef ODK_ENV_SET
#error "odk_env_unit.hip: compile with -DODK_ENV_SET=<name> (one of odk_shapes.h's ODK_ENV_SET_<name>)"
#endif
#include "odk_env_kernels.h"

#define ODK_CAT_(a, b) a##b
#define ODK_CAT(a, b) ODK_CAT_(a, b)
#define X(S, G, HF) template hipError_t launch_sg<S, G, HF>(int, const KArgs&, hipStream_t);
ODK_CAT(ODK_ENV_SET_, ODK_ENV_SET)(X)
#undef X

/* Host stand-in for "device_launch_parameters.h".  The launch indices the
 * kernels read (threadIdx, blockIdx, blockDim) are supplied by the bridge as
 * per-thread host variables; nothing is needed here. */
#ifndef PTREF_SHIM_DEVICE_LAUNCH_PARAMETERS_H
#define PTREF_SHIM_DEVICE_LAUNCH_PARAMETERS_H
#include "cuda.h"
#endif

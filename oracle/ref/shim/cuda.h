/* Host stand-in for <cuda.h>: the version macro glm asks for and the CUDA
 * function qualifiers, emptied, so that __host__ __device__ code compiles as
 * ordinary C++.  Our own text; nothing here comes from the CUDA toolkit. */
#ifndef PTREF_SHIM_CUDA_H
#define PTREF_SHIM_CUDA_H

#define CUDA_VERSION 12000

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#ifndef __global__
#define __global__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif

#endif

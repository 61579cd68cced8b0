/* Host stand-in for <cuda_runtime_api.h>: the few cuda* names the reference's
 * memory pool and its memory report mention, over malloc/memcpy.  Our own
 * text; the bridge never calls a GPU runtime. */
#ifndef PTREF_SHIM_CUDA_RUNTIME_API_H
#define PTREF_SHIM_CUDA_RUNTIME_API_H

#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "cuda.h"

typedef int cudaError_t;
enum { cudaSuccess = 0, cudaErrorMemoryAllocation = 2 };
enum cudaMemcpyKind {
    cudaMemcpyHostToHost = 0, cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2,
    cudaMemcpyDeviceToDevice = 3, cudaMemcpyDefault = 4
};

template <typename T>
static inline cudaError_t cudaMallocManaged(T **p, size_t bytes)
{
    *p = static_cast<T *>(std::calloc(bytes ? bytes : 1, 1));
    return *p ? cudaSuccess : cudaErrorMemoryAllocation;
}

static inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t bytes, cudaMemcpyKind)
{
    if (bytes) std::memcpy(dst, src, bytes);
    return cudaSuccess;
}

static inline cudaError_t cudaFree(void *p)
{
    std::free(p);
    return cudaSuccess;
}

static inline cudaError_t cudaMemGetInfo(size_t *free_bytes, size_t *total_bytes)
{
    *free_bytes = 0;
    *total_bytes = 0;
    return cudaSuccess;
}

static inline const char *cudaGetErrorString(cudaError_t) { return "host build"; }

static inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }

#endif

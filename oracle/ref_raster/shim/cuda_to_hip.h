// Shared body of the cuda*.h shims: the reference rasterizer's CUDA runtime names on top of HIP.
// Test infrastructure only (oracle/ref_raster/README.md); never part of the product.
#pragma once
#include <hip/hip_runtime.h>

#define cudaError_t hipError_t
#define cudaSuccess hipSuccess
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaGetErrorString hipGetErrorString
#define cudaMemcpy hipMemcpy
#define cudaMemset hipMemset
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaMemcpyHostToDevice hipMemcpyHostToDevice

// The reference calls __trap() only on the prefiltered == true branch of in_frustum (auxiliary.h), which no caller of
// this oracle takes.  On a shared card a trap must not be able to fault the device: it is a no-op here, and the
// wrapper rejects prefiltered == true before anything is launched.
#define __trap() ((void)0)

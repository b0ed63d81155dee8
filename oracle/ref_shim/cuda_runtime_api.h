/* Shadows <cuda_runtime_api.h> for the `ref` target of oracle/Makefile: the handful of CUDA runtime names the reference's
 * four pointnet2 kernel files use, mapped to HIP.  Our own text; nothing of the reference's is in it.  Test infrastructure. */
#ifndef G4D_REF_SHIM_CUDA_RUNTIME_API_H
#define G4D_REF_SHIM_CUDA_RUNTIME_API_H

#include <hip/hip_runtime.h>

#include <algorithm>   /* with it HIP's headers declare the host-side int min / max that the reference's cuda_utils.h calls */

typedef hipStream_t cudaStream_t;
typedef hipError_t cudaError_t;
#define cudaSuccess hipSuccess
#define cudaGetLastError hipGetLastError
#define cudaGetErrorString hipGetErrorString

#endif

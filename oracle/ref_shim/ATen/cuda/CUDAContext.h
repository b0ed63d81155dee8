/* Shadows <ATen/cuda/CUDAContext.h> for the `ref` target of oracle/Makefile: the reference's sampling header reaches the CUDA
 * runtime types through it. */
#ifndef G4D_REF_SHIM_ATEN_CUDA_CUDACONTEXT_H
#define G4D_REF_SHIM_ATEN_CUDA_CUDACONTEXT_H
#include "../../cuda_runtime_api.h"
#endif

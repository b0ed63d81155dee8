/* Shadows <cuda.h> for the `ref` target of oracle/Makefile (see cuda_runtime_api.h next to this file). */
#ifndef G4D_REF_SHIM_CUDA_H
#define G4D_REF_SHIM_CUDA_H
#include "cuda_runtime_api.h"
#endif

// The inverse-distance weights of a garment vertex's K <= 256 nearest body vertices, as one wave holds them: the ONE routine behind the
// forward blend (garment_ops.hip: knn_blend_weights_kernel) and its adjoint (skin/skin_grad.hip: knn_blend_grad_kernel), so that the
// weights the gradient is taken of are the weights the forward used, bit for bit.
#pragma once
#include "g4d_common.h"

// Lane `lane` holds the pairs k = lane, lane + 64, lane + 128, lane + 192 of the row (ix, dd: its K indices and squared distances).  Declares
//   int iv[4]:   iv[q] = ix[k] (0 past the end of the list)
//   float wv[4]: wv[q] = r_k / s with inf -> 0, where r_k = 1 / d_k with inf -> 0 (0 past the end) -- the reference's two isinf fix-ups,
//                modules/mesh_encoder.py:342-345
//   float s:     the sum of the r_k over the wave (xor butterfly: the same bits in every lane)
// A macro, not an inline function: the statements are the forward kernel's own, pasted where they stood, so the forward's code object is the
// one it was before the adjoint existed (as an inlined function the 64-lane form of the kernel came out with another register allocation).
#define G4D_KNN_BLEND_LANE_WEIGHTS(ix, dd, K, lane)            \
    int iv[4];                                                 \
    float wv[4];                                               \
    float s = 0.f;                                             \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {            \
        const int k = q * 64 + lane;                           \
        iv[q] = k < K ? ix[k] : 0;                             \
        float w = k < K ? 1.0f / dd[k] : 0.f;                  \
        if (__builtin_isinf(w)) w = 0.f;                       \
        wv[q] = w;                                             \
        s += w;                                                \
    }                                                          \
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o); \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {            \
        float w = wv[q] / s;                                   \
        if (__builtin_isinf(w)) w = 0.f;                       \
        wv[q] = w;                                             \
    }

// The fixed-order sums of the mesh-side kernels (losses, batch-norm training, GCN backward, post-processing): every summation order is a
// function of the shape alone and nothing here uses atomics, so two runs give the same bits.
//
// Workgroup sum, block_sum<NWAVES>: a xor butterfly over the 64 lanes of each wave (strides 32, 16, 8, 4, 2, 1: 6 levels; a + b == b + a, so
// every lane of a wave holds the same bits), then sh[0] + sh[1] + ... + sh[NWAVES - 1] left to right (NWAVES - 1 more levels; 4 waves:
// ((s0 + s1) + s2) + s3, depth 9).  Every thread returns the same value.
//
// Column sums over row slices: a block owns one slice of the rows and a thread (ty, tx) a few columns of the rows ty, ty + TY, ...;
// slice_col_sums adds the TY partials of a column in ascending ty and writes the slice's sums to a workspace, reduce_slices adds the slices.
#pragma once
#include "g4d_common.h"

namespace g4d {

// `sh` holds NWAVES values.  The barrier sits BEFORE the write: the previous call's reads of sh (or any earlier use of it) are over when a
// wave stores its sum, so calls may follow each other on the same sh with nothing in between.
template <int NWAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T *sh) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = sh[0];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) s = s + sh[w];
    return s;
}

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// The tail of a 256-thread column-sum block (thread (ty, tx) = threadIdx.x / tx_n, % tx_n; VEC columns from `col` on; NOUT sums per column):
// the TY partials of a column are added in ascending ty by thread (0, tx) and go to ws[slice = blockIdx.x][o][c].  `part`: NOUT * 256 * VEC floats.
template <int VEC, int NOUT>
__device__ __forceinline__ void slice_col_sums(float (&acc)[NOUT][VEC], float *part, int tx, int ty, int tx_n, int ty_n, int col, int c, float *__restrict__ ws) {
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[(o * 256 + threadIdx.x) * VEC + j] = acc[o][j];
    __syncthreads();
    if (ty == 0 && col < c) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float s = part[(o * 256 + tx) * VEC + j];
                for (int k = 1; k < ty_n; ++k) s += part[(o * 256 + k * tx_n + tx) * VEC + j];
                ws[((size_t)blockIdx.x * NOUT + o) * c + col + j] = s;
            }
    }
}

// reduce.hip: out0[i] (i < n0) / out1[i - n0] = (sum over the slices of ws[s][i]) / div for the n elements of a slice, on `st`.  Per element
// four interleaved chains (slices j, j + 4, ... ascending), then ((chain 0 + chain 1) + chain 2) + chain 3.  A division, so that a column
// of equal values whose sum is exact has exactly that value as its mean; div = 1 leaves the sum as it is.
void reduce_slices(long long slices, long long n, long long n0, float div, const float *ws, float *out0, float *out1, hipStream_t st);

}  // namespace g4d

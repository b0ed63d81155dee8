// The one slice-reduction kernel behind reduce.h's reduce_slices (batch-norm statistics and parameter gradients, GCN bias and weight gradients).
#include "reduce.h"

namespace g4d {

constexpr int kChains = 4;   // interleaved chains per element

// Thread (j, x): element 64 * blockIdx.x + x, slices j, j + 4, ... ascending.
__global__ void __launch_bounds__(256) reduce_slices_kernel(long long slices, long long n, long long n0, float div, const float *__restrict__ ws,
                                                           float *__restrict__ out0, float *__restrict__ out1) {
    __shared__ float part[256];
    const int x = threadIdx.x & 63, j = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + x;
    float acc = 0.f;
    if (i < n) {
        long long s = j;
        for (; s + 3 * kChains < slices; s += 4 * kChains) {   // four loads in flight, added in slice order
            const float a0 = ws[(size_t)s * n + i], a1 = ws[(size_t)(s + kChains) * n + i], a2 = ws[(size_t)(s + 2 * kChains) * n + i],
                        a3 = ws[(size_t)(s + 3 * kChains) * n + i];
            acc += a0; acc += a1; acc += a2; acc += a3;
        }
        for (; s < slices; s += kChains) acc += ws[(size_t)s * n + i];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (j == 0 && i < n) {
        const float v = (((part[x] + part[64 + x]) + part[128 + x]) + part[192 + x]) / div;
        if (i < n0) out0[i] = v;
        else out1[i - n0] = v;
    }
}

void reduce_slices(long long slices, long long n, long long n0, float div, const float *ws, float *out0, float *out1, hipStream_t st) {
    hipLaunchKernelGGL(reduce_slices_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, slices, n, n0, div, ws, out0, out1);
}

}  // namespace g4d

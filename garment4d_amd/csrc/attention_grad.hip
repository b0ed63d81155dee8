// Backward of the temporal attention of the refinement rounds (csrc/attention.hip is the forward).  Per clip, with Q, K, V the three column
// blocks of the (F, Vg, 3C) qkv buffer, D = Vg * C:
//   S = Q K^T / sqrt(T)      A = softmax(S) (saved by the forward, T x T)      O = A V
//   dA = dO V^T                                      att_grad_scores_partial_kernel: the skinny contraction of the forward's score kernel, the
//                                                    A operand read from the strided feature-gradient window; per-workgroup partials
//   dS = A * (dA - rowsum(dA * A)) / sqrt(T)         att_grad_softmax_kernel: one workgroup per clip sums the partials in a fixed order
//   dQ = dS K     dK = dS^T Q     dV = A^T dO        att_grad_mix_kernel: three independent (T x T) . (T x D) products, each shaped like the
//                                                    forward's mix kernel: a thread holds the T values of FOUR consecutive columns of ONE source
//                                                    block, forms the T outputs with the (uniform) matrix and stores them; grid.z picks the block
// HBM traffic: dO and V once (scores), Q, K and dO once (mix), three blocks written: eight (T, D) blocks, nothing is read once per output
// frame.  No atomics anywhere: every sum has a fixed order and the gradient is bit-reproducible.
#include "g4d_common.h"

namespace g4d {

typedef float ag_f32x4 __attribute__((ext_vector_type(4)));
typedef float ag_f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at a 4-byte aligned address (column offset 195)

constexpr int kAgKsteps = 32;   // 16-wide k-steps per wave, as in the forward
constexpr int kAgMaxT = 32;

__global__ void __launch_bounds__(256) att_grad_scores_partial_kernel(int T, int vg, int C, const float *__restrict__ qkv, const float *__restrict__ dO,
                                                                     int ldg, int col0, float *__restrict__ partial, int slices) {
    const int lane = threadIdx.x & 63, fi = lane & 15, fq = lane >> 4;
    const int slice = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int c = blockIdx.y;
    const bool active = slice < slices;
    const long long total_ksteps = (long long)vg * C / 16;
    const long long s0 = (long long)slice * kAgKsteps;
    const int t0 = min(fi, T - 1), t1 = min(16 + fi, T - 1);
    const size_t ld = (size_t)vg * 3 * C, ldo = (size_t)vg * ldg;   // floats per frame of qkv / of the gradient buffer
    const float *vbase = qkv + (size_t)c * T * ld + 2 * C + fq * 4;
    const float *gbase = dO + (size_t)c * T * ldo + col0 + fq * 4;
    const float *v0 = vbase + (size_t)t0 * ld, *v1 = vbase + (size_t)t1 * ld;
    const float *g0 = gbase + (size_t)t0 * ldo, *g1 = gbase + (size_t)t1 * ldo;
    ag_f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = ag_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < kAgKsteps && active; ++s) {
        const long long ks = s0 + s;
        if (ks >= total_ksteps) break;
        const long long d = ks * 16;
        const size_t vtx = (size_t)(d / C), ch = (size_t)(d % C);
        const size_t off = vtx * 3 * C + ch, goff = vtx * ldg + ch;
        const ag_f32x4 a0 = *reinterpret_cast<const ag_f32x4u *>(g0 + goff), a1 = *reinterpret_cast<const ag_f32x4u *>(g1 + goff);
        const ag_f32x4 b0 = *reinterpret_cast<const ag_f32x4u *>(v0 + off), b1 = *reinterpret_cast<const ag_f32x4u *>(v1 + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b0[e], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b1[e], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b0[e], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b1[e], acc[1][1], 0, 0, 0);
        }
    }
    __shared__ float red[4][kAgMaxT * kAgMaxT];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][(rt * 16 + fq * 4 + r) * kAgMaxT + ct * 16 + fi] = acc[rt][ct][r];
    __syncthreads();
    float *p = partial + ((size_t)c * gridDim.x + blockIdx.x) * (kAgMaxT * kAgMaxT);
    for (int i = threadIdx.x; i < kAgMaxT * kAgMaxT; i += 256) p[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// dA = sum of the partials (fixed order), then dS[t][u] = A[t][u] (dA[t][u] - sum_w dA[t][w] A[t][w]) / sqrt(T)   (T x T per clip, row-major)
__global__ void __launch_bounds__(1024) att_grad_softmax_kernel(int T, int slices, const float *__restrict__ partial, const float *__restrict__ att,
                                                               float *__restrict__ dS) {
    __shared__ float da[kAgMaxT][kAgMaxT + 1], aa[kAgMaxT][kAgMaxT + 1];
    const int t = threadIdx.x >> 5, u = threadIdx.x & 31;
    const int c = blockIdx.x;
    const float *p = partial + (size_t)c * slices * (kAgMaxT * kAgMaxT) + threadIdx.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int w = 0;
    for (; w + 3 < slices; w += 4) {
        s0 += p[(size_t)w * (kAgMaxT * kAgMaxT)];
        s1 += p[(size_t)(w + 1) * (kAgMaxT * kAgMaxT)];
        s2 += p[(size_t)(w + 2) * (kAgMaxT * kAgMaxT)];
        s3 += p[(size_t)(w + 3) * (kAgMaxT * kAgMaxT)];
    }
    for (; w < slices; ++w) s0 += p[(size_t)w * (kAgMaxT * kAgMaxT)];
    const bool in = t < T && u < T;
    da[t][u] = in ? (s0 + s1) + (s2 + s3) : 0.f;
    aa[t][u] = in ? att[((size_t)c * T + t) * T + u] : 0.f;
    __syncthreads();
    if (in) {
        float r = 0.f;
        for (int j = 0; j < T; ++j) r = __builtin_fmaf(da[t][j], aa[t][j], r);
        dS[((size_t)c * T + t) * T + u] = aa[t][u] * (da[t][u] - r) / (float)sqrt((double)T);
    }
}

// grid.z = 0: dQ[t] = sum_u dS[t][u] K[u]     1: dK[t] = sum_u dS[u][t] Q[u]     2: dV[t] = sum_u A[u][t] dO[u]
__global__ void __launch_bounds__(256) att_grad_mix_kernel(int T, int vg, int C, const float *__restrict__ qkv, const float *__restrict__ att,
                                                          const float *__restrict__ dS, const float *__restrict__ dO, int ldg, int col0,
                                                          float *__restrict__ dqkv) {
    const long long col4 = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, which = blockIdx.z;
    const int c4 = C >> 2;
    if (col4 >= (long long)vg * c4) return;
    const int v = (int)(col4 / c4), ch = (int)(col4 - (long long)v * c4) * 4;
    const size_t ld = (size_t)vg * 3 * C;
    const float *src;
    size_t lds;
    if (which == 2) { src = dO + (size_t)c * T * vg * ldg + (size_t)v * ldg + col0 + ch; lds = (size_t)vg * ldg; }
    else { src = qkv + (size_t)c * T * ld + (size_t)v * 3 * C + (which == 0 ? C : 0) + ch; lds = ld; }
    ag_f32x4 val[kAgMaxT];
#pragma unroll
    for (int u = 0; u < kAgMaxT; ++u) val[u] = u < T ? (ag_f32x4)*reinterpret_cast<const ag_f32x4u *>(src + (size_t)u * lds) : (ag_f32x4){0.f, 0.f, 0.f, 0.f};
    const float *m = (which == 2 ? att : dS) + (size_t)c * T * T;
    const int st = which == 0 ? T : 1, su = which == 0 ? 1 : T;   // weight of (output t, source u): dS[t][u] | dS[u][t] | A[u][t]
    float *dst = dqkv + (size_t)c * T * ld + (size_t)v * 3 * C + which * C + ch;
    for (int t = 0; t < T; ++t) {
        ag_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kAgMaxT; ++u)
            if (u < T) {
                const float w = m[t * st + u * su];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(w, val[u][e], acc[e]);
            }
        *reinterpret_cast<ag_f32x4u *>(dst + (size_t)t * ld) = acc;
    }
}

}  // namespace g4d

extern "C" size_t g4d_temporal_attention_grad_scratch_floats(int nclips, int vg, int c) {
    using namespace g4d;
    const long long ksteps = (long long)vg * c / 16;
    const long long slices = (ksteps + kAgKsteps - 1) / kAgKsteps;
    return (size_t)nclips * ((slices + 3) / 4 + 1) * kAgMaxT * kAgMaxT;   // workgroup partials + dS
}

extern "C" int g4d_temporal_attention_grad_f32(int nclips, int t, int vg, int c, const float *qkv, const float *att, const float *dO, int ldg,
                                               int col0, float *scratch, float *dqkv, g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(nclips >= 0 && t >= 1 && t <= kAgMaxT && vg >= 0 && c > 0 && c % 16 == 0,
                "g4d_temporal_attention_grad_f32: need 1 <= T <= %d and C %% 16 == 0", kAgMaxT);
    if (nclips == 0 || vg == 0) return G4D_OK;
    G4D_REQUIRE(qkv && att && dO && scratch && dqkv && ldg >= col0 + c && col0 >= 0 && nclips <= 65535, "g4d_temporal_attention_grad_f32: bad arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long ksteps = (long long)vg * c / 16;
    const int slices = (int)((ksteps + kAgKsteps - 1) / kAgKsteps);
    const int groups = (slices + 3) / 4;
    float *dS = scratch + (size_t)nclips * groups * kAgMaxT * kAgMaxT;
    hipLaunchKernelGGL(att_grad_scores_partial_kernel, dim3(groups, nclips), dim3(256), 0, st, t, vg, c, qkv, dO, ldg, col0, scratch, slices);
    hipLaunchKernelGGL(att_grad_softmax_kernel, dim3(nclips), dim3(1024), 0, st, t, groups, scratch, att, dS);
    hipLaunchKernelGGL(att_grad_mix_kernel, dim3((unsigned)(((long long)vg * (c / 4) + 255) / 256), nclips, 3), dim3(256), 0, st, t, vg, c, qkv, att, dS,
                       dO, ldg, col0, dqkv);
    return check_launch("g4d_temporal_attention_grad_f32");
}

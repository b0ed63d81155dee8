// Adjoint of g4d_mgn_skin_f32 (csrc/mgn_skin.hip) with respect to `garment`, for a FIXED nearest index -- the index is a piecewise-constant
// function of the input, and torch's autograd treats it as a constant in the reference as well (knn_points(...).idx feeding torch.gather,
// modules/mesh_encoder.py:541-583).  Per (frame f, garment vertex g), with nn = nn_idx[f, g] clamped into [0, V-1]:
//   M_inv = sum_j W[f, nn, j] inv_A[f, j],   M = sum_j W[f, nn, j] A[f, j]     (the forward's blends, recomputed in the forward's order)
//   t = M[:3,:3]^T d_posed[f, g] + d_stage1[f, g]                               (stage 1 is an output of its own AND the input of the second blend)
//   d_garment[f, g] = M_inv[:3,:3]^T t
// The translation columns and the root add drop out.  One thread per (f, g), 256 consecutive (f, g) per workgroup, every output element
// written once by one thread: no atomics, two runs give the same bits.
//
// The transforms: a workgroup's queries lie in one frame, or in two when it straddles a frame boundary (Vg >= 255), so rows 0..2 of the two
// first frames' inv_A / A (2 x 2 x J x 3 float4, 12 KB at J = 64) are staged in LDS and every lane reads the same address (a broadcast).
// Lanes of a later frame (garments of fewer than 255 vertices) read the same rows from global memory through the same arithmetic.
// The gather of the 4 J-byte row W[f, nn, :] is the only irregular access.
#include "g4d_common.h"

namespace g4d {

constexpr int kMgnGradThreads = 256;
constexpr int kMgnGradFrames = 2;                          // frames whose transforms are staged per workgroup
constexpr int kMgnGradMaxJ = 64;

// The 3x3 parts of both blends, j ascending, each entry acc = fma(w_j, T_j[r][k], acc) from 0 -- the forward's order (mgn_skin.hip).  ia / pa:
// rows 0..2 of joint j's transform at [j * stride + r].
__device__ __forceinline__ void mgn_grad_blend(const float4 *ia, const float4 *pa, int stride, const float *__restrict__ w, int nj, float *mi,
                                               float *mp) {
#pragma unroll
    for (int e = 0; e < 9; ++e) mi[e] = 0.f, mp[e] = 0.f;
    for (int j = 0; j < nj; ++j) {
        const float wj = w[j];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float4 a = ia[j * stride + r], b = pa[j * stride + r];
            mi[r * 3 + 0] = fmaf(wj, a.x, mi[r * 3 + 0]); mi[r * 3 + 1] = fmaf(wj, a.y, mi[r * 3 + 1]); mi[r * 3 + 2] = fmaf(wj, a.z, mi[r * 3 + 2]);
            mp[r * 3 + 0] = fmaf(wj, b.x, mp[r * 3 + 0]); mp[r * 3 + 1] = fmaf(wj, b.y, mp[r * 3 + 1]); mp[r * 3 + 2] = fmaf(wj, b.z, mp[r * 3 + 2]);
        }
    }
}

__global__ void __launch_bounds__(kMgnGradThreads) mgn_skin_grad_kernel(long long total, int vg, int v, int nj, long long frames,
                                                                        const int *__restrict__ nn_idx, const float *__restrict__ W,
                                                                        const float *__restrict__ inv_A, const float *__restrict__ A,
                                                                        const float *__restrict__ d_posed, const float *__restrict__ d_stage1,
                                                                        float *__restrict__ d_garment) {
    __shared__ float4 sm[kMgnGradFrames * 2 * kMgnGradMaxJ * 3];       // [frame][inv_A | A][j][row 0..2]
    const long long q_first = (long long)blockIdx.x * kMgnGradThreads;
    const long long f_lo = q_first / vg;
    const int staged = (int)min((long long)kMgnGradFrames, frames - f_lo);
    for (int i = threadIdx.x; i < staged * 2 * nj * 3; i += kMgnGradThreads) {
        const int r = i % 3, j = (i / 3) % nj, m = (i / (3 * nj)) & 1, fr = i / (6 * nj);
        const float *src = (m ? A : inv_A) + ((size_t)(f_lo + fr) * nj + j) * 16;
        sm[i] = reinterpret_cast<const float4 *>(src)[r];
    }
    __syncthreads();
    const long long qi = q_first + threadIdx.x;
    if (qi >= total) return;
    const long long f = qi / vg;
    const int nn = min(max(nn_idx[qi], 0), v - 1);       // a stale or foreign index gives a wrong number, never an out-of-range read
    const float *w = W + ((size_t)f * v + nn) * nj;
    float mi[9], mp[9];
    const int fr = (int)(f - f_lo);
    if (fr < kMgnGradFrames) {
        const float4 *base = sm + (size_t)fr * 2 * nj * 3;
        mgn_grad_blend(base, base + nj * 3, 3, w, nj, mi, mp);
    } else {
        mgn_grad_blend(reinterpret_cast<const float4 *>(inv_A + (size_t)f * nj * 16), reinterpret_cast<const float4 *>(A + (size_t)f * nj * 16), 4, w,
                       nj, mi, mp);
    }
    const float *dp = d_posed + (size_t)qi * 3;
    const float g0 = dp[0], g1 = dp[1], g2 = dp[2];
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // column k of M . d_posed, on top of d_stage1: fma(M[2][k], g2, fma(M[1][k], g1, fma(M[0][k], g0, d_stage1[k])))
        const float s = d_stage1 ? d_stage1[(size_t)qi * 3 + k] : 0.f;
        t[k] = fmaf(mp[6 + k], g2, fmaf(mp[3 + k], g1, fmaf(mp[k], g0, s)));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)     // column k of M_inv . t: fma(Mi[2][k], t2, fma(Mi[1][k], t1, Mi[0][k] * t0))
        d_garment[(size_t)qi * 3 + k] = fmaf(mi[6 + k], t[2], fmaf(mi[3 + k], t[1], mi[k] * t[0]));
}

}  // namespace g4d

extern "C" int g4d_mgn_skin_grad_f32(int clips, int frames_per_clip, int vg, int v, int j, const int *nn_idx, const float *W, const float *inv_A,
                                     const float *A, const float *d_posed, const float *d_stage1, float *d_garment, g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(clips >= 0 && frames_per_clip >= 0 && vg >= 0 && v >= 0 && j >= 0, "g4d_mgn_skin_grad_f32: negative size");
    if (clips == 0 || frames_per_clip == 0 || vg == 0) return G4D_OK;
    G4D_REQUIRE(v >= 1, "g4d_mgn_skin_grad_f32: no body vertices (V = 0)");
    G4D_REQUIRE(j >= 1 && j <= kMgnGradMaxJ, "g4d_mgn_skin_grad_f32: need 1 <= J <= %d (got %d)", kMgnGradMaxJ, j);
    const long long frames = (long long)clips * frames_per_clip;
    const long long total = frames * vg;
    const long long blocks = (total + kMgnGradThreads - 1) / kMgnGradThreads;
    G4D_REQUIRE(blocks <= 0x7fffffffll, "g4d_mgn_skin_grad_f32: too many queries");
    G4D_REQUIRE(nn_idx && W && inv_A && A && d_posed && d_garment, "g4d_mgn_skin_grad_f32: null pointer");
    G4D_REQUIRE(((reinterpret_cast<uintptr_t>(inv_A) | reinterpret_cast<uintptr_t>(A)) & 15) == 0,
                "g4d_mgn_skin_grad_f32: inv_A and A must be 16-byte aligned");
    hipLaunchKernelGGL(mgn_skin_grad_kernel, dim3((unsigned)blocks), dim3(kMgnGradThreads), 0, reinterpret_cast<hipStream_t>(stream), total, vg, v,
                       j, frames, nn_idx, W, inv_A, A, d_posed, d_stage1, d_garment);
    return check_launch("g4d_mgn_skin_grad_f32");
}

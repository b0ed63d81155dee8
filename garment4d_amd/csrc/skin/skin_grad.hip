// libg4d_skin.so (include/g4d_skin.h): the adjoint of the garment skinning with respect to the T-pose garment.
//   garment_skin_grad : adjoint of lbs_skin_kernel (lbs.hip) in the garment's form -- d input vertices and d blended weights
//   knn_blend_grad    : adjoint of knn_blend_weights_kernel (garment_ops.hip), carried through the inverse-distance weights to the query points
// No atomics, one writer per value, every sum in an order fixed by the shapes: see the header for the orders.
#include "../g4d_common.h"
#include "../knn_blend_weights.h"
#include "../../../include/g4d_skin.h"

namespace g4d {

// A thread owns garment vertex v of clip c and walks the clip's frames in ascending order; a frame's transforms A (J x 3 x 4, the last row of
// the 4 x 4 dropped) are staged in LDS and read as broadcasts.  JR >= J: the joints a thread keeps in registers (its weight row and, with one
// table per clip, the running sum of d_W over the frames).
// One wave per workgroup: cfg4 has 8 clips x 4096 vertices, which 256-thread workgroups would spread over 128 of the 256 CUs only.
constexpr int kSkinThreads = 64;

template <int JR>
__global__ void __launch_bounds__(kSkinThreads) garment_skin_grad_kernel(int T, int vg, int J, int blocks_per_clip, const float *__restrict__ W, int w_per_clip,
                                                                const float *__restrict__ A, const float *__restrict__ verts,
                                                                const float *__restrict__ d_out, const float *d_add, float *d_verts,
                                                                float *__restrict__ d_W) {
    __shared__ float sA[G4D_SKIN_MAX_JOINTS * 12];
    const int c = blockIdx.x / blocks_per_clip;
    const int v = (blockIdx.x - c * blocks_per_clip) * kSkinThreads + threadIdx.x;
    const bool live = v < vg;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        const float *p = verts + ((size_t)c * vg + v) * 3;
        x = p[0]; y = p[1]; z = p[2];
    }
    float w[JR], acc[JR];
#pragma unroll
    for (int j = 0; j < JR; ++j) { w[j] = 0.f; acc[j] = 0.f; }
    float du0 = 0.f, du1 = 0.f, du2 = 0.f;
    for (int t = 0; t < T; ++t) {
        const size_t f = (size_t)c * T + t;
        __syncthreads();   // the previous frame's reads of sA are over
        for (int i = threadIdx.x; i < J * 12; i += kSkinThreads) sA[i] = A[(f * J + i / 12) * 16 + (i % 12)];
        __syncthreads();
        if (!live) continue;
        if (!w_per_clip || t == 0) {
            const float *wr = W + ((w_per_clip ? (size_t)c : f) * vg + v) * J;
#pragma unroll
            for (int j = 0; j < JR; ++j)
                if (j < J) w[j] = wr[j];
        }
        const float *g = d_out + (f * vg + v) * 3;
        const float g0 = g[0], g1 = g[1], g2 = g[2];
        float R[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = 0.f;
#pragma unroll
        for (int j = 0; j < JR; ++j) {
            if (j < J) {
                const float *a = sA + j * 12;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) R[r * 3 + k] = fmaf(w[j], a[r * 4 + k], R[r * 3 + k]);   // T^R = sum_j W_j A_j^R, j ascending
                if (d_W) {
                    const float h0 = fmaf(a[2], z, fmaf(a[1], y, a[0] * x)) + a[3];     // A_j [v; 1], row by row
                    const float h1 = fmaf(a[6], z, fmaf(a[5], y, a[4] * x)) + a[7];
                    const float h2 = fmaf(a[10], z, fmaf(a[9], y, a[8] * x)) + a[11];
                    const float dw = fmaf(g2, h2, fmaf(g1, h1, g0 * h0));
                    if (w_per_clip) acc[j] += dw;
                    else d_W[(f * vg + v) * J + j] = dw;
                }
            }
        }
        du0 += fmaf(R[6], g2, fmaf(R[3], g1, R[0] * g0));   // (T^R)^T dy
        du1 += fmaf(R[7], g2, fmaf(R[4], g1, R[1] * g0));
        du2 += fmaf(R[8], g2, fmaf(R[5], g1, R[2] * g0));
    }
    if (!live) return;
    if (d_verts) {
        const size_t o = ((size_t)c * vg + v) * 3;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (d_add) { a0 = d_add[o]; a1 = d_add[o + 1]; a2 = d_add[o + 2]; }
        d_verts[o] = a0 + du0; d_verts[o + 1] = a1 + du1; d_verts[o + 2] = a2 + du2;
    }
    if (d_W && w_per_clip) {
#pragma unroll
        for (int j = 0; j < JR; ++j)
            if (j < J) d_W[((size_t)c * vg + v) * J + j] = acc[j];
    }
}

// One wave per (clip, garment vertex); lane l owns the neighbours k = l, l + 64, l + 128, l + 192 (index, weight, 1 / d from the forward's own
// routine).  Per frame of the clip the row d_blend[f, v, :] is wave-uniform (scalar loads); a lane gathers the table rows W[f, idx_k, :] of its
// neighbours -- 16-byte loads where VEC -- and adds dW . W_row into c_k.  Two wave sums then give sum_m w_m c_m and d g.
template <bool VEC>
__global__ void __launch_bounds__(256) knn_blend_grad_kernel(long long rows, int T, int vg, int v, int K, int ldk, int J, const float *__restrict__ W,
                                                             const int *__restrict__ idx, const float *__restrict__ dists,
                                                             const float *__restrict__ d_blend, const float *__restrict__ pts,
                                                             const float *__restrict__ ref, const float *d_add, float *d_pts) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (clip, vertex), wave-uniform
    if (row >= rows) return;
    const long long c = row / vg;
    const int *ix = idx + (size_t)row * ldk;
    const float *dd = dists + (size_t)row * ldk;
    G4D_KNN_BLEND_LANE_WEIGHTS(ix, dd, K, lane)   // iv[4], wv[4], s
    float ck[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) iv[q] = min(max(iv[q], 0), v - 1);
    for (int t = 0; t < T; ++t) {
        const size_t f = (size_t)c * T + t;
        const float *dw = d_blend + (f * vg + (size_t)(row - c * vg)) * J;
        const float *Wf = W + f * v * J;
        if (VEC) {
            for (int j = 0; j < J; j += 4) {
                const float d0 = dw[j], d1 = dw[j + 1], d2 = dw[j + 2], d3 = dw[j + 3];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q * 64 < K) {   // wave-uniform
                        const float4 wr = *reinterpret_cast<const float4 *>(Wf + (size_t)iv[q] * J + j);
                        ck[q] = fmaf(d3, wr.w, fmaf(d2, wr.z, fmaf(d1, wr.y, fmaf(d0, wr.x, ck[q]))));
                    }
                }
            }
        } else {
            for (int j = 0; j < J; ++j) {
                const float d0 = dw[j];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q * 64 < K) ck[q] = fmaf(d0, Wf[(size_t)iv[q] * J + j], ck[q]);
            }
        }
    }
    // From here on in float64 (a few operations per lane): the terms 2 dd_k (g - body_k) of the near neighbours are large and of mixed sign, and
    // their sum is what is asked for.  wv and s are the forward's fp32 weights and sum, taken as they are.
    double wc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q * 64 + lane >= K) ck[q] = 0.f;   // past the end of the list: row 0 was read, nothing of it counts
        wc += (double)wv[q] * (double)ck[q];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wc += __shfl_xor(wc, o);
    const float *p = pts + (size_t)row * 3;
    const double px = p[0], py = p[1], pz = p[2];
    const float *body = ref + (size_t)c * v * 3;
    double gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = q * 64 + lane;
        if (k < K) {
            const float d = dd[k];
            float r32 = 1.0f / d;                 // the forward's r_k: 0 where it is infinite, i.e. at a coincident neighbour
            if (__builtin_isinf(r32)) r32 = 0.f;
            const double r = 1.0 / (double)d;
            const double dr = ((double)ck[q] - wc) / (double)s;
            const double dd2 = r32 == 0.f ? 0.0 : -2.0 * dr * r * r;   // coincident neighbour: defined as zero
            const F3 b = ld_point(body, iv[q]);
            gx += dd2 * (px - (double)b.x); gy += dd2 * (py - (double)b.y); gz += dd2 * (pz - (double)b.z);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gx += __shfl_xor(gx, o); gy += __shfl_xor(gy, o); gz += __shfl_xor(gz, o);
    }
    if (lane == 0) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (d_add) { a0 = d_add[row * 3]; a1 = d_add[row * 3 + 1]; a2 = d_add[row * 3 + 2]; }
        d_pts[row * 3] = a0 + (float)gx; d_pts[row * 3 + 1] = a1 + (float)gy; d_pts[row * 3 + 2] = a2 + (float)gz;
    }
}

}  // namespace g4d

using namespace g4d;
#define G4D_S(s) reinterpret_cast<hipStream_t>(s)

extern "C" int g4d_garment_skin_grad_f32(int clips, int frames_per_clip, int vg, int j, const float *W, int w_per_clip, const float *A,
                                         const float *verts, const float *d_out, const float *d_add, float *d_verts, float *d_W,
                                         g4d_stream_t stream) {
    G4D_REQUIRE(clips >= 0 && vg >= 0 && frames_per_clip >= 1 && j >= 1 && j <= G4D_SKIN_MAX_JOINTS,
                "g4d_garment_skin_grad_f32: bad sizes (frames_per_clip >= 1, 1 <= J <= %d)", G4D_SKIN_MAX_JOINTS);
    if (clips == 0 || vg == 0) return G4D_OK;
    G4D_REQUIRE(W && A && verts && d_out, "g4d_garment_skin_grad_f32: null pointer");
    if (!d_verts && !d_W) return G4D_OK;
    const int bpc = (vg + kSkinThreads - 1) / kSkinThreads;
    G4D_REQUIRE((long long)clips * bpc < (1ll << 31) && (long long)clips * frames_per_clip < (1ll << 31), "g4d_garment_skin_grad_f32: too large");
    const dim3 grid((unsigned)(clips * bpc)), block(kSkinThreads);
#define G4D_LAUNCH(JR)                                                                                                                        \
    hipLaunchKernelGGL(garment_skin_grad_kernel<JR>, grid, block, 0, G4D_S(stream), frames_per_clip, vg, j, bpc, W, w_per_clip, A, verts, d_out, \
                       d_add, d_verts, d_W)
    if (j <= 8) G4D_LAUNCH(8);
    else if (j <= 24) G4D_LAUNCH(24);
    else if (j <= 32) G4D_LAUNCH(32);
    else G4D_LAUNCH(64);
#undef G4D_LAUNCH
    return check_launch("g4d_garment_skin_grad_f32");
}

extern "C" int g4d_knn_blend_grad_f32(int frames, int frames_per_clip, int vg, int v, int k, int ldk, int j, const float *W, const int *idx,
                                      const float *dists, const float *d_blend, const float *pts, const float *ref, const float *d_add,
                                      float *d_pts, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && vg >= 0 && frames_per_clip >= 1 && frames % frames_per_clip == 0 && v >= 1 && k >= 1 && k <= G4D_SKIN_MAX_K && ldk >= k &&
                    j >= 1 && j <= G4D_SKIN_MAX_JOINTS,
                "g4d_knn_blend_grad_f32: bad sizes (frames a multiple of frames_per_clip >= 1, 1 <= K <= %d, ldk >= K, 1 <= J <= %d, V >= 1)",
                G4D_SKIN_MAX_K, G4D_SKIN_MAX_JOINTS);
    const long long rows = (long long)(frames / frames_per_clip) * vg;
    if (rows == 0) return G4D_OK;
    G4D_REQUIRE(W && idx && dists && d_blend && pts && ref && d_pts, "g4d_knn_blend_grad_f32: null pointer");
    G4D_REQUIRE((rows + 3) / 4 < (1ll << 31), "g4d_knn_blend_grad_f32: too large");
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    // 16-byte row loads: every table row starts at a multiple of 16 bytes
    if (j % 4 == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0)
        hipLaunchKernelGGL(knn_blend_grad_kernel<true>, grid, block, 0, G4D_S(stream), rows, frames_per_clip, vg, v, k, ldk, j, W, idx, dists, d_blend,
                           pts, ref, d_add, d_pts);
    else
        hipLaunchKernelGGL(knn_blend_grad_kernel<false>, grid, block, 0, G4D_S(stream), rows, frames_per_clip, vg, v, k, ldk, j, W, idx, dists, d_blend,
                           pts, ref, d_add, d_pts);
    return check_launch("g4d_knn_blend_grad_f32");
}

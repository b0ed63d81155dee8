// The stage-2 objective of the refinement head (smplx/loss/temporal_loss.py:147-201, `temporal_loss_PCA_LBS`) for ONE round's prediction
// p (F, Vg, 3), F = nbatch * T frames: the four differentiated terms, the MSRE metric, and -- when asked -- dL/dp in the same pass.
//
//   term          value                                                   gradient w.r.t. p
//   L2            mean_{f,i} |p - g|^2                                    2 (p - g) / (F Vg)
//   Laplacian     mean_{f,i} |(L p)_i|,  L = I - D^-1 A                   L^T u / (F Vg),  u_i = (L p)_i / |(L p)_i|   (0 where the norm is 0)
//   penetration   mean_{f,i} relu(-n_b . (p - b)),  b = nearest body v.   -n_b / (F Vg) where the dot is negative, else 0
//   temporal      mean_{clip, t < T-1, i} |p_t - p_{t+1}|  (last round)   +-d / |d| / (nbatch (T-1) Vg) to both frames  (0 where |d| is 0)
//   MSRE          mean_{f,i} |p - g|  (+ one mean per frame)              none
//
// Launches (all on the caller's stream, no atomics anywhere):
//   1. terms_kernel      one thread per (frame, vertex), 256-thread workgroups that never straddle a frame.  Per-vertex terms, the non-Laplacian
//                        part of the gradient written to grad, u written to the workspace, five partial sums per workgroup to the workspace.
//   2. lap_grad_kernel   grad += c_lap (L^T u): one thread per (frame, vertex) walks its row of the TRANSPOSED operator (the 2-ring of the
//                        Laplacian term) in CSR order.  u is staged through global memory, so there is ONE route for every Vg and every row
//                        length: nothing has to fit LDS, and the frame's u (48 KB at Vg = 4096) is read back out of L2.  Skipped without a
//                        gradient or with a zero Laplacian weight.
//   3. finish_kernel     one workgroup adds the partials in a fixed order (below) and writes the five means and the per-frame MSRE.
//
// Arithmetic (the file is built with -ffp-contract=off: every product and sum below is rounded on its own):
//   (L p)_i = sum_k val_k (p_col_k - p_i)  +  rowsum_i p_i        in CSR order.  The differences are formed FIRST: a Laplacian row sums to
//             zero up to the rounding of its fp32 entries (rowsum_i, computed by the host in float64), so the large common part p_i cancels
//             exactly instead of in the last bits of a sum of products.  Exact in exact arithmetic for ANY matrix, not only for a Laplacian.
//   |x|     = sqrtf((x0 x0 + x1 x1) + x2 x2)
//   the penetration dot product left to right, as g4d_interpenetration_f32
//
// Reduction tree of each of the five sums (depth = the number of additions on the longest path, what the error bound counts):
//   * workgroup: reduce.h's block_sum over the four waves (depth 9);
//   * frame:     its ceil(Vg / 256) workgroup partials added left to right by one thread of the finishing workgroup;
//   * total:     finishing thread t adds the frames t, t + 256, ... in that order, then the same workgroup tree over the 256 threads.
//   depth = 9 + (ceil(Vg / 256) - 1) + (ceil(F / 256) - 1) + 9.  The order depends on the shape alone: two runs give the same bits.
#include "reduce.h"

namespace g4d {
namespace {

constexpr int kRLBlock = 256;
constexpr int kRLTerms = 5;   // L2, MSRE, Laplacian, penetration, temporal
constexpr int kRLWaves = kRLBlock / 64;

struct RLArgs {
    int frames, t, vg, v, nblk, idx_stride, temporal;
    const float *p, *g, *body, *normals;
    const int *nn_idx, *rowptr, *colidx;
    const float *vals, *rowsum;
    float c_l2, c_pen, c_tmp;
    float *partials, *u, *grad;
};

__global__ void __launch_bounds__(kRLBlock) rl_terms_kernel(RLArgs a) {
    __shared__ float sh[kRLWaves];
    const int f = blockIdx.x / a.nblk, blk = blockIdx.x - f * a.nblk;
    const int i = blk * kRLBlock + threadIdx.x;
    float s_l2 = 0.f, s_ms = 0.f, s_lap = 0.f, s_pen = 0.f, s_tmp = 0.f;
    if (i < a.vg) {
        const size_t base = (size_t)f * a.vg;
        const float *pf = a.p + base * 3;
        const size_t e = (base + i) * 3;
        const float px = pf[i * 3 + 0], py = pf[i * 3 + 1], pz = pf[i * 3 + 2];
        // L2 + MSRE
        const float dx = px - a.g[e + 0], dy = py - a.g[e + 1], dz = pz - a.g[e + 2];
        s_l2 = (dx * dx + dy * dy) + dz * dz;
        s_ms = sqrtf(s_l2);
        // Laplacian
        float lx = 0.f, ly = 0.f, lz = 0.f;
        for (int k = a.rowptr[i], k1 = a.rowptr[i + 1]; k < k1; ++k) {
            const int j = a.colidx[k];
            const float w = a.vals[k];
            lx = lx + w * (pf[j * 3 + 0] - px);
            ly = ly + w * (pf[j * 3 + 1] - py);
            lz = lz + w * (pf[j * 3 + 2] - pz);
        }
        const float rs = a.rowsum[i];
        lx = lx + rs * px;
        ly = ly + rs * py;
        lz = lz + rs * pz;
        s_lap = norm3(lx, ly, lz);
        // penetration (the nearest body vertex is the search's; the clamp only keeps a corrupt index inside the frame)
        int bi = a.nn_idx[(base + i) * a.idx_stride];
        bi = min(max(bi, 0), a.v - 1);
        const size_t b = ((size_t)f * a.v + bi) * 3;
        const float nx = a.normals[b + 0], ny = a.normals[b + 1], nz = a.normals[b + 2];
        const float dot = nx * (px - a.body[b + 0]) + ny * (py - a.body[b + 1]) + nz * (pz - a.body[b + 2]);
        s_pen = fmaxf(-dot, 0.f);
        // temporal: d = p_t - p_{t+1} of the same clip; this vertex receives +d/|d| from its own pair and -d/|d| from the previous frame's
        float tx = 0.f, ty = 0.f, tz = 0.f;
        if (a.temporal && a.t > 1) {
            const int t = f % a.t;
            if (t < a.t - 1) {
                const float *q = pf + (size_t)a.vg * 3 + i * 3;
                const float ex = px - q[0], ey = py - q[1], ez = pz - q[2];
                s_tmp = norm3(ex, ey, ez);
                if (s_tmp > 0.f) { tx = ex / s_tmp; ty = ey / s_tmp; tz = ez / s_tmp; }
            }
            if (a.grad && t > 0) {
                const float *q = pf - (size_t)a.vg * 3 + i * 3;
                const float ex = q[0] - px, ey = q[1] - py, ez = q[2] - pz;
                const float n = norm3(ex, ey, ez);
                if (n > 0.f) { tx = tx - ex / n; ty = ty - ey / n; tz = tz - ez / n; }
            }
        }
        if (a.grad) {
            float ux = 0.f, uy = 0.f, uz = 0.f;
            if (s_lap > 0.f) { ux = lx / s_lap; uy = ly / s_lap; uz = lz / s_lap; }
            a.u[e + 0] = ux; a.u[e + 1] = uy; a.u[e + 2] = uz;
            const float m = dot < 0.f ? a.c_pen : 0.f;
            a.grad[e + 0] = (a.c_l2 * dx - m * nx) + a.c_tmp * tx;
            a.grad[e + 1] = (a.c_l2 * dy - m * ny) + a.c_tmp * ty;
            a.grad[e + 2] = (a.c_l2 * dz - m * nz) + a.c_tmp * tz;
        }
    }
    const float r0 = block_sum<kRLWaves>(s_l2, sh), r1 = block_sum<kRLWaves>(s_ms, sh), r2 = block_sum<kRLWaves>(s_lap, sh), r3 = block_sum<kRLWaves>(s_pen, sh),
                r4 = block_sum<kRLWaves>(s_tmp, sh);
    if (threadIdx.x == 0) {
        float *o = a.partials + (size_t)blockIdx.x * kRLTerms;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4;
    }
}

__global__ void __launch_bounds__(kRLBlock) rl_lap_grad_kernel(long long total, int vg, const int *__restrict__ rowptr_t, const int *__restrict__ colidx_t,
                                                               const float *__restrict__ vals_t, const float *__restrict__ u, float c_lap,
                                                               float *__restrict__ grad) {
    const long long gid = (long long)blockIdx.x * kRLBlock + threadIdx.x;
    if (gid >= total) return;
    const long long f = gid / vg;
    const int i = (int)(gid - f * vg);
    const float *uf = u + (size_t)f * vg * 3;
    float x = 0.f, y = 0.f, z = 0.f;
    for (int k = rowptr_t[i], k1 = rowptr_t[i + 1]; k < k1; ++k) {
        const int j = colidx_t[k];
        const float w = vals_t[k];
        x = x + w * uf[j * 3 + 0];
        y = y + w * uf[j * 3 + 1];
        z = z + w * uf[j * 3 + 2];
    }
    grad[gid * 3 + 0] = grad[gid * 3 + 0] + c_lap * x;
    grad[gid * 3 + 1] = grad[gid * 3 + 1] + c_lap * y;
    grad[gid * 3 + 2] = grad[gid * 3 + 2] + c_lap * z;
}

__global__ void __launch_bounds__(kRLBlock) rl_finish_kernel(int frames, int vg, int nblk, const float *__restrict__ partials, float inv_n, float inv_tmp,
                                                             float *__restrict__ out, float *__restrict__ msre_frames) {
    __shared__ float sh[kRLWaves];
    float acc[kRLTerms] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int f = threadIdx.x; f < frames; f += kRLBlock) {
        const float *pf = partials + (size_t)f * nblk * kRLTerms;
        float s[kRLTerms];
#pragma unroll
        for (int c = 0; c < kRLTerms; ++c) s[c] = pf[c];
        for (int b = 1; b < nblk; ++b) {
#pragma unroll
            for (int c = 0; c < kRLTerms; ++c) s[c] = s[c] + pf[b * kRLTerms + c];
        }
        if (msre_frames) msre_frames[f] = s[1] / (float)vg;
#pragma unroll
        for (int c = 0; c < kRLTerms; ++c) acc[c] = acc[c] + s[c];
    }
    float r[kRLTerms];
#pragma unroll
    for (int c = 0; c < kRLTerms; ++c) r[c] = block_sum<kRLWaves>(acc[c], sh);
    if (threadIdx.x == 0) {
        out[0] = r[0] * inv_n; out[1] = r[1] * inv_n; out[2] = r[2] * inv_n; out[3] = r[3] * inv_n; out[4] = r[4] * inv_tmp;
    }
}

inline long long rl_blocks(int frames, int vg) { return (long long)frames * ((vg + kRLBlock - 1) / kRLBlock); }

}  // namespace
}  // namespace g4d

extern "C" long long g4d_refine_loss_ws_bytes(int frames, int vg, int with_grad) {
    if (frames <= 0 || vg <= 0) return 0;
    long long floats = g4d::rl_blocks(frames, vg) * g4d::kRLTerms;
    if (with_grad) floats += (long long)frames * vg * 3;
    return floats * 4;
}

extern "C" int g4d_refine_loss_f32(int nbatch, int t, int vg, int v, const float *pred, const float *target, const float *body, const float *normals,
                                   const int *nn_idx, int idx_stride, const int *rowptr, const int *colidx, const float *vals, const float *rowsum,
                                   const int *rowptr_t, const int *colidx_t, const float *vals_t, float w_l2, float w_lap, float w_pen,
                                   float w_temporal, int temporal, float *ws, float *out, float *msre_frames, float *grad, g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(nbatch >= 0 && t >= 0 && vg >= 0 && v >= 0 && idx_stride >= 1, "g4d_refine_loss_f32: bad sizes (nbatch %d, t %d, vg %d, v %d, idx_stride %d)",
                nbatch, t, vg, v, idx_stride);
    G4D_REQUIRE(w_l2 == w_l2 && w_lap == w_lap && w_pen == w_pen && w_temporal == w_temporal, "g4d_refine_loss_f32: a weight is NaN");
    G4D_REQUIRE(out, "g4d_refine_loss_f32: out is null");
    const long long frames_ll = (long long)nbatch * t;
    G4D_REQUIRE(frames_ll <= 0x7fffffffLL, "g4d_refine_loss_f32: too many frames");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (frames_ll == 0 || vg == 0) {   // an empty problem: every sum is empty
        const hipError_t e = hipMemsetAsync(out, 0, kRLTerms * sizeof(float), st);
        if (e != hipSuccess) { set_error("g4d_refine_loss_f32: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
        return G4D_OK;
    }
    const int frames = (int)frames_ll;
    const int nblk = (vg + kRLBlock - 1) / kRLBlock;
    const long long blocks = rl_blocks(frames, vg), total = frames_ll * vg;
    G4D_REQUIRE(v > 0, "g4d_refine_loss_f32: no body vertices");
    G4D_REQUIRE(blocks <= 0x7fffffffLL && total * 3 <= 0x7fffffffffLL, "g4d_refine_loss_f32: problem too large (%lld workgroups)", blocks);
    G4D_REQUIRE(pred && target && body && normals && nn_idx && rowptr && colidx && vals && rowsum && ws, "g4d_refine_loss_f32: null pointer");
    const bool lap_grad = grad && w_lap != 0.f;
    G4D_REQUIRE(!lap_grad || (rowptr_t && colidx_t && vals_t), "g4d_refine_loss_f32: the gradient of the Laplacian term needs the transposed operator");
    const double n = (double)frames * vg, n_tmp = (double)nbatch * (t - 1) * vg;
    const bool has_tmp = temporal && t > 1;
    RLArgs a;
    a.frames = frames; a.t = t; a.vg = vg; a.v = v; a.nblk = nblk; a.idx_stride = idx_stride; a.temporal = has_tmp ? 1 : 0;
    a.p = pred; a.g = target; a.body = body; a.normals = normals; a.nn_idx = nn_idx; a.rowptr = rowptr; a.colidx = colidx; a.vals = vals; a.rowsum = rowsum;
    a.c_l2 = (float)(2.0 * w_l2 / n); a.c_pen = (float)(w_pen / n); a.c_tmp = has_tmp ? (float)(w_temporal / n_tmp) : 0.f;
    a.partials = ws; a.u = grad ? ws + blocks * kRLTerms : nullptr; a.grad = grad;
    hipLaunchKernelGGL(rl_terms_kernel, dim3((unsigned)blocks), dim3(kRLBlock), 0, st, a);
    if (lap_grad)
        hipLaunchKernelGGL(rl_lap_grad_kernel, dim3((unsigned)((total + kRLBlock - 1) / kRLBlock)), dim3(kRLBlock), 0, st, total, vg, rowptr_t, colidx_t, vals_t,
                           a.u, (float)(w_lap / n), grad);
    hipLaunchKernelGGL(rl_finish_kernel, dim3(1), dim3(kRLBlock), 0, st, frames, vg, nblk, ws, (float)(1.0 / n), has_tmp ? (float)(1.0 / n_tmp) : 0.f, out,
                       msre_frames);
    return check_launch("g4d_refine_loss_f32");
}

// The stage-1 objective of the garment encoder (smplx/loss/temporal_loss.py:60-119, `temporal_loss_PCA`): the cross-entropy of the point
// labels, the PCA-coefficient L2, and the three T-pose garment terms (L2 with its MSRE metric, interpenetration, the one-time cotangent
// Laplacian of smplx/loss/laplacian.py:199-305, 454-467) -- values and, when asked, the analytic gradient in the same pass.
//
//   term          value                                                            gradient
//   cross-entropy mean_r [log sum_c exp(x_rc) - x_r,y_r]                           (softmax - onehot) / rows                  w.r.t. the logits
//   PCA           mean_{b,k} (a - a_gt)^2                                          2 (a - a_gt) / (B P)                       w.r.t. the coefficients
//   L2            mean_{b,i} |p - g|^2                                             2 (p - g) / (B Vg)                         w.r.t. p
//   MSRE          mean_{b,i} |p - g|                                               none
//   penetration   mean_{b,i} relu(-n_b . (q - b)),  q = p + root_b, b = nearest    -n_b / (B Vg) where the dot is negative, else 0
//   Laplacian     mean_{b < Bp, i} | |(L(p_b) p_b)_i| - |(L(g_b) g_b)_i| |         L(p_b) u_b / (Bp Vg),  u_i = sign(n_i - c_i) (L p)_i / n_i
//                 n_i = |(L p)_i|, c_i = |(L g)_i|; items b >= B are copies of item 0: item 0 counts 1 + Bp - B times, nothing is copied.
//                 u_i = 0 where n_i = 0 or n_i = c_i.  L is a CONSTANT of the gradient (the reference's OnetimeLaplacian.backward returns
//                 L g_out: nothing flows through the cotangents), rebuilt from the predicted vertices on every call, and symmetric.
//
// The cotangent Laplacian.  Per face (v1, v2, v3) and corner k the reference's entry is half the cotangent of the corner's angle (its
// [cot23, cot31, cot12] / A / 4 with A = 2 sqrt(Heron); NaN and inf replaced by 0).  Here, with e1 = v2 - v1, e2 = v3 - v1 and the ONE cross
// product per face  x = e1 x e2,  |x| = sqrtf((x0 x0 + x1 x1) + x2 x2)  (twice the area, the same for the three corners):
//   h_k = 0.5f * (dot_k / |x|),   dot_k = (a0 b0 + a1 b1) + a2 b2  over the two edges a, b leaving corner k;   h_k = 0 where |x| is 0 (or NaN).
// No square roots of edge lengths, no Heron cancellation.  The corner of vertex i in a face (i, j, k) (cyclic) receives
//   h_j (x_k - x_i)  then  h_k (x_j - x_i)
// i.e. (L x)_i = sum_j w_ij (x_j - x_i) with the differences formed FIRST (as refine_loss.hip does); the sum runs over the vertex's
// (face, corner) incidences in CSR order -- a scatter of faces to vertices without atomics.  The incidence is built on the host.
//
// Launches (all on the caller's stream, no atomics anywhere):
//   cross-entropy entry point
//     1. s1_ce_kernel       one thread per row of C logits: m = max_c x_c (left to right), s = sum_c expf(x_c - m) (left to right),
//                           loss = logf(s) - (x_y - m); with a gradient buffer  scale * (expf(x_c - m) / s - [c == y])  in the same pass.
//                           A label outside [0, C) never indexes anything: its loss is NaN (so the mean is NaN) and its gradient row zero.
//                           (torch's ignore_index = -100 would drop such a row from the mean instead; the reference's loader never produces
//                           one, and ignore_index semantics are not implemented.)  One partial sum per workgroup.
//     2. s1_ce_finish       one workgroup: thread t adds the partials t, t + 256, ... in that order, then the workgroup tree.
//   garment entry point
//     1. s1_cot_kernel      one thread per (item, face), grid.y = 0: the target g, 1: the prediction p; the three h_k to the workspace.
//     2. s1_terms_kernel    one thread per (item, vertex), 256-thread workgroups that never straddle an item: the per-vertex terms, the
//                           non-Laplacian part of the gradient, u to the workspace, four partial sums per workgroup.
//     3. s1_lap_grad_kernel grad += c_lap_b (L(p_b) u_b): the same incidence walk over u, with the staged h of p.  Skipped without a gradient
//                           or with a zero Laplacian weight.  h (B x faces x 3) and u (B x Vg x 3) are staged through global memory: one
//                           route for every Vg, nothing has to fit LDS.
//     4. s1_finish_kernel   one workgroup: the four garment sums in a fixed order (below), the PCA term (B P numbers: thread t adds the
//                           squares of elements t, t + 256, ... in that order, then the workgroup tree) and its gradient.
//
// Arithmetic (the file is built with -ffp-contract=off: every product and sum is rounded on its own):
//   |x|     = sqrtf((x0 x0 + x1 x1) + x2 x2)
//   q       = p + root, then the penetration dot product left to right over (q - b), as g4d_refine_loss_f32
//   u       = +-(L p) / n  per coordinate
//   grad p  = c_l2 d - [dot < 0] c_pen n_b, then + c_lap_b (L u) by launch 3;  c_l2 = 2 w_l2 / (B Vg), c_pen = w_pen / (B Vg),
//             c_lap_b = w_lap (b == 0 ? 1 + Bp - B : 1) / (Bp Vg), each computed in double and rounded once
//
// Reduction tree of every sum (depth = the number of additions on the longest path, what the error bound counts):
//   * workgroup: reduce.h's block_sum over the four waves (depth 9);
//   * cross-entropy: finishing thread t adds the workgroup partials t, t + 256, ... in order, then the workgroup tree over the 256 threads:
//     depth = 9 + (ceil(nwg / 256) - 1) + 9,  nwg = ceil(rows / 256);
//   * garment: an item's ceil(Vg / 256) workgroup partials left to right by one finishing thread (item 0's Laplacian sum is then multiplied
//     by 1 + Bp - B), finishing thread t adds the items t, t + 256, ... in order, then the workgroup tree:
//     depth = 9 + (ceil(Vg / 256) - 1) + (ceil(B / 256) - 1) + 9  (+ 1 product for item 0's Laplacian weight);
//   * PCA: depth = (ceil(B P / 256) - 1) + 9.
//   The order depends on the shape alone: two runs give the same bits, with or without gradient buffers.
#include "reduce.h"

namespace g4d {
namespace {

constexpr int kS1Block = 256;
constexpr int kS1Terms = 4;   // L2, MSRE, penetration, Laplacian
constexpr int kS1Waves = kS1Block / 64;

// ---------------------------------------------------------------------------------------------------------------------- cross-entropy
__global__ void __launch_bounds__(kS1Block) s1_ce_kernel(long long rows, int c, const float *__restrict__ logits, const long long *__restrict__ labels,
                                                         float scale, float *__restrict__ partials, float *__restrict__ grad) {
    __shared__ float sh[kS1Waves];
    const long long r = (long long)blockIdx.x * kS1Block + threadIdx.x;
    float loss = 0.f;
    if (r < rows) {
        const float *x = logits + r * c;
        const long long y = labels[r];
        const bool ok = y >= 0 && y < c;
        float m = x[0];
        for (int k = 1; k < c; ++k) m = fmaxf(m, x[k]);
        float s = 0.f;
        for (int k = 0; k < c; ++k) s = s + expf(x[k] - m);
        loss = ok ? logf(s) - (x[ok ? y : 0] - m) : __builtin_nanf("");
        if (grad) {
            float *g = grad + r * c;
            for (int k = 0; k < c; ++k) g[k] = ok ? scale * (expf(x[k] - m) / s - (k == y ? 1.f : 0.f)) : 0.f;
        }
    }
    const float t = block_sum<kS1Waves>(loss, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ void __launch_bounds__(kS1Block) s1_ce_finish(long long nwg, const float *__restrict__ partials, float inv_rows, float *__restrict__ out) {
    __shared__ float sh[kS1Waves];
    float acc = 0.f;
    for (long long k = threadIdx.x; k < nwg; k += kS1Block) acc = acc + partials[k];
    const float t = block_sum<kS1Waves>(acc, sh);
    if (threadIdx.x == 0) out[0] = t * inv_rows;
}

// ---------------------------------------------------------------------------------------------------------------------------- garment
__global__ void __launch_bounds__(kS1Block) s1_cot_kernel(long long total, int vg, int nf, const float *__restrict__ target, const float *__restrict__ pred,
                                                          const int *__restrict__ faces, float *__restrict__ h_target, float *__restrict__ h_pred) {
    const long long gid = (long long)blockIdx.x * kS1Block + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / nf;
    const int f = (int)(gid - b * nf);
    const float *x = (blockIdx.y ? pred : target) + b * vg * 3;
    float *h = (blockIdx.y ? h_pred : h_target) + gid * 3;
    // (the clamp only keeps a corrupt face index inside the item)
    const int i1 = min(max(faces[f * 3 + 0], 0), vg - 1), i2 = min(max(faces[f * 3 + 1], 0), vg - 1), i3 = min(max(faces[f * 3 + 2], 0), vg - 1);
    const float ax = x[i1 * 3 + 0], ay = x[i1 * 3 + 1], az = x[i1 * 3 + 2];
    const float bx = x[i2 * 3 + 0], by = x[i2 * 3 + 1], bz = x[i2 * 3 + 2];
    const float cx = x[i3 * 3 + 0], cy = x[i3 * 3 + 1], cz = x[i3 * 3 + 2];
    const float abx = bx - ax, aby = by - ay, abz = bz - az;   // v2 - v1
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;   // v3 - v1
    const float bcx = cx - bx, bcy = cy - by, bcz = cz - bz;   // v3 - v2
    const float n = norm3(aby * acz - abz * acy, abz * acx - abx * acz, abx * acy - aby * acx);
    float h1 = 0.f, h2 = 0.f, h3 = 0.f;
    if (n > 0.f) {                                             // false for NaN as well
        const float d1 = (abx * acx + aby * acy) + abz * acz;              // (v2 - v1) . (v3 - v1)
        const float d2 = -((bcx * abx + bcy * aby) + bcz * abz);           // (v3 - v2) . (v1 - v2)
        const float d3 = (acx * bcx + acy * bcy) + acz * bcz;              // (v1 - v3) . (v2 - v3)
        h1 = 0.5f * (d1 / n); h2 = 0.5f * (d2 / n); h3 = 0.5f * (d3 / n);
        if (!(fabsf(h1) <= 3.0e38f && fabsf(h2) <= 3.0e38f && fabsf(h3) <= 3.0e38f)) { h1 = 0.f; h2 = 0.f; h3 = 0.f; }   // inf / NaN -> 0, as the reference
    }
    h[0] = h1; h[1] = h2; h[2] = h3;
}

// (L x)_i over the (face, corner) incidences of vertex i; x and h belong to one item
__device__ __forceinline__ void s1_lap_row(int i, int vg, int nf, const float *__restrict__ x, const float *__restrict__ h, const int *__restrict__ faces,
                                           const int *__restrict__ rowptr, const int *__restrict__ inc, float &lx, float &ly, float &lz) {
    const float xi = x[i * 3 + 0], yi = x[i * 3 + 1], zi = x[i * 3 + 2];
    lx = 0.f; ly = 0.f; lz = 0.f;
    for (int k = rowptr[i], k1 = rowptr[i + 1]; k < k1; ++k) {
        const int e = min(max(inc[k], 0), nf * 3 - 1);   // face * 3 + corner (the clamp only keeps a corrupt entry inside the arrays)
        const int f = e / 3, c = e - f * 3;
        const int c1 = c == 2 ? 0 : c + 1, c2 = c1 == 2 ? 0 : c1 + 1;
        const int j = min(max(faces[f * 3 + c1], 0), vg - 1), kk = min(max(faces[f * 3 + c2], 0), vg - 1);
        const float hj = h[f * 3 + c1], hk = h[f * 3 + c2];
        lx = lx + hj * (x[kk * 3 + 0] - xi); ly = ly + hj * (x[kk * 3 + 1] - yi); lz = lz + hj * (x[kk * 3 + 2] - zi);
        lx = lx + hk * (x[j * 3 + 0] - xi);  ly = ly + hk * (x[j * 3 + 1] - yi);  lz = lz + hk * (x[j * 3 + 2] - zi);
    }
}

struct S1Args {
    int b, vg, v, nf, nblk, idx_stride;
    const float *p, *g, *root, *body, *normals;
    const int *nn_idx, *faces, *rowptr, *inc;
    const float *h_target, *h_pred;
    float c_l2, c_pen;
    float *partials, *u, *grad;
};

__global__ void __launch_bounds__(kS1Block) s1_terms_kernel(S1Args a) {
    __shared__ float sh[kS1Waves];
    const int b = blockIdx.x / a.nblk, blk = blockIdx.x - b * a.nblk;
    const int i = blk * kS1Block + threadIdx.x;
    float s_l2 = 0.f, s_ms = 0.f, s_pen = 0.f, s_lap = 0.f;
    if (i < a.vg) {
        const size_t base = (size_t)b * a.vg;
        const float *pb = a.p + base * 3, *gb = a.g + base * 3;
        const size_t e = (base + i) * 3;
        const float px = pb[i * 3 + 0], py = pb[i * 3 + 1], pz = pb[i * 3 + 2];
        // L2 + MSRE
        const float dx = px - gb[i * 3 + 0], dy = py - gb[i * 3 + 1], dz = pz - gb[i * 3 + 2];
        s_l2 = (dx * dx + dy * dy) + dz * dz;
        s_ms = sqrtf(s_l2);
        // penetration against the T-pose body, the garment moved to the root joint (the nearest body vertex is the search's)
        const float qx = px + a.root[b * 3 + 0], qy = py + a.root[b * 3 + 1], qz = pz + a.root[b * 3 + 2];
        int bi = a.nn_idx[(base + i) * a.idx_stride];
        bi = min(max(bi, 0), a.v - 1);
        const size_t o = ((size_t)b * a.v + bi) * 3;
        const float nx = a.normals[o + 0], ny = a.normals[o + 1], nz = a.normals[o + 2];
        const float dot = nx * (qx - a.body[o + 0]) + ny * (qy - a.body[o + 1]) + nz * (qz - a.body[o + 2]);
        s_pen = fmaxf(-dot, 0.f);
        // Laplacian: the curvature target from g with g's cotangents, the prediction's from p with p's
        const size_t hb = (size_t)b * a.nf * 3;
        float tx, ty, tz, lx, ly, lz;
        s1_lap_row(i, a.vg, a.nf, gb, a.h_target + hb, a.faces, a.rowptr, a.inc, tx, ty, tz);
        s1_lap_row(i, a.vg, a.nf, pb, a.h_pred + hb, a.faces, a.rowptr, a.inc, lx, ly, lz);
        const float cn = norm3(tx, ty, tz), n = norm3(lx, ly, lz);
        s_lap = fabsf(n - cn);
        if (a.grad) {
            float ux = 0.f, uy = 0.f, uz = 0.f;
            if (n > 0.f && n != cn) {
                ux = lx / n; uy = ly / n; uz = lz / n;
                if (n < cn) { ux = -ux; uy = -uy; uz = -uz; }
            }
            a.u[e + 0] = ux; a.u[e + 1] = uy; a.u[e + 2] = uz;
            const float m = dot < 0.f ? a.c_pen : 0.f;
            a.grad[e + 0] = a.c_l2 * dx - m * nx;
            a.grad[e + 1] = a.c_l2 * dy - m * ny;
            a.grad[e + 2] = a.c_l2 * dz - m * nz;
        }
    }
    const float r0 = block_sum<kS1Waves>(s_l2, sh), r1 = block_sum<kS1Waves>(s_ms, sh), r2 = block_sum<kS1Waves>(s_pen, sh), r3 = block_sum<kS1Waves>(s_lap, sh);
    if (threadIdx.x == 0) {
        float *o = a.partials + (size_t)blockIdx.x * kS1Terms;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
    }
}

__global__ void __launch_bounds__(kS1Block) s1_lap_grad_kernel(long long total, int vg, int nf, const float *__restrict__ u, const float *__restrict__ h_pred,
                                                               const int *__restrict__ faces, const int *__restrict__ rowptr, const int *__restrict__ inc,
                                                               float c_lap0, float c_lap, float *__restrict__ grad) {
    const long long gid = (long long)blockIdx.x * kS1Block + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / vg;
    const int i = (int)(gid - b * vg);
    float x, y, z;
    s1_lap_row(i, vg, nf, u + b * vg * 3, h_pred + b * nf * 3, faces, rowptr, inc, x, y, z);
    const float c = b == 0 ? c_lap0 : c_lap;
    grad[gid * 3 + 0] = grad[gid * 3 + 0] + c * x;
    grad[gid * 3 + 1] = grad[gid * 3 + 1] + c * y;
    grad[gid * 3 + 2] = grad[gid * 3 + 2] + c * z;
}

__global__ void __launch_bounds__(kS1Block) s1_finish_kernel(int b, int nblk, const float *__restrict__ partials, float item0_weight, float inv_n, float inv_lap,
                                                             long long npca, const float *__restrict__ coeff, const float *__restrict__ coeff_gt, float inv_pca,
                                                             float c_pca, float *__restrict__ grad_coeff, float *__restrict__ out) {
    __shared__ float sh[kS1Waves];
    float acc[kS1Terms] = {0.f, 0.f, 0.f, 0.f};
    for (int it = threadIdx.x; it < b; it += kS1Block) {
        const float *pf = partials + (size_t)it * nblk * kS1Terms;
        float s[kS1Terms];
#pragma unroll
        for (int c = 0; c < kS1Terms; ++c) s[c] = pf[c];
        for (int k = 1; k < nblk; ++k) {
#pragma unroll
            for (int c = 0; c < kS1Terms; ++c) s[c] = s[c] + pf[k * kS1Terms + c];
        }
        if (it == 0) s[3] = s[3] * item0_weight;
#pragma unroll
        for (int c = 0; c < kS1Terms; ++c) acc[c] = acc[c] + s[c];
    }
    float pca = 0.f;
    for (long long k = threadIdx.x; k < npca; k += kS1Block) {
        const float d = coeff[k] - coeff_gt[k];
        pca = pca + d * d;
        if (grad_coeff) grad_coeff[k] = c_pca * d;
    }
    float r[kS1Terms];
#pragma unroll
    for (int c = 0; c < kS1Terms; ++c) r[c] = block_sum<kS1Waves>(acc[c], sh);
    const float rp = block_sum<kS1Waves>(pca, sh);
    if (threadIdx.x == 0) {
        out[0] = r[0] * inv_n; out[1] = r[1] * inv_n; out[2] = r[2] * inv_n; out[3] = r[3] * inv_lap; out[4] = rp * inv_pca;
    }
}

inline long long s1_ce_blocks(long long rows) { return rows <= 0 ? 0 : (rows + kS1Block - 1) / kS1Block; }
inline long long s1_blocks(int b, int vg) { return (long long)b * ((vg + kS1Block - 1) / kS1Block); }
inline bool s1_nan(float x) { return x != x; }

}  // namespace
}  // namespace g4d

extern "C" long long g4d_stage1_loss_ws_bytes(long long ce_rows, int b, int vg, int nf, int with_grad) {
    long long floats = g4d::s1_ce_blocks(ce_rows);
    if (b > 0 && vg > 0) {
        floats += g4d::s1_blocks(b, vg) * g4d::kS1Terms + 2LL * b * (nf > 0 ? nf : 0) * 3;
        if (with_grad) floats += (long long)b * vg * 3;
    }
    return floats * 4;
}

extern "C" int g4d_stage1_ce_f32(long long rows, int classes, const float *logits, const long long *labels, float w_sem, float *ws, float *out, float *grad,
                                 g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(rows >= 0 && classes >= 1 && classes <= 64, "g4d_stage1_ce_f32: bad sizes (rows %lld, classes %d: 1..64)", rows, classes);
    G4D_REQUIRE(!s1_nan(w_sem), "g4d_stage1_ce_f32: the weight is NaN");
    G4D_REQUIRE(out, "g4d_stage1_ce_f32: out is null");
    const long long nwg = s1_ce_blocks(rows);
    G4D_REQUIRE(nwg <= 0x7fffffffLL, "g4d_stage1_ce_f32: problem too large (%lld workgroups)", nwg);
    G4D_REQUIRE(rows == 0 || (logits && labels && ws), "g4d_stage1_ce_f32: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (rows == 0) {   // an empty problem: the sum is empty
        const hipError_t e = hipMemsetAsync(out, 0, sizeof(float), st);
        if (e != hipSuccess) { set_error("g4d_stage1_ce_f32: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
        return G4D_OK;
    }
    hipLaunchKernelGGL(s1_ce_kernel, dim3((unsigned)nwg), dim3(kS1Block), 0, st, rows, classes, logits, labels, (float)((double)w_sem / (double)rows), ws, grad);
    hipLaunchKernelGGL(s1_ce_finish, dim3(1), dim3(kS1Block), 0, st, nwg, ws, (float)(1.0 / (double)rows), out);
    return check_launch("g4d_stage1_ce_f32");
}

extern "C" int g4d_stage1_garment_f32(int b, int bp, int vg, int v, int nf, int pdim, const float *pred, const float *target, const float *root,
                                      const float *body, const float *normals, const int *nn_idx, int idx_stride, const int *faces, const int *inc_rowptr,
                                      const int *inc, const float *coeff, const float *coeff_gt, float w_pca, float w_l2, float w_pen, float w_lap, float *ws,
                                      float *out, float *grad_pred, float *grad_coeff, g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(b >= 0 && bp >= b && vg >= 0 && v >= 0 && nf >= 0 && pdim >= 0 && idx_stride >= 1,
                "g4d_stage1_garment_f32: bad sizes (b %d, bp %d >= b, vg %d, v %d, nf %d, pdim %d, idx_stride %d)", b, bp, vg, v, nf, pdim, idx_stride);
    G4D_REQUIRE(!s1_nan(w_pca) && !s1_nan(w_l2) && !s1_nan(w_pen) && !s1_nan(w_lap), "g4d_stage1_garment_f32: a weight is NaN");
    G4D_REQUIRE(out, "g4d_stage1_garment_f32: out is null");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (b == 0 || vg == 0) {   // an empty problem: every sum is empty
        const hipError_t e = hipMemsetAsync(out, 0, 5 * sizeof(float), st);
        if (e != hipSuccess) { set_error("g4d_stage1_garment_f32: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
        return G4D_OK;
    }
    const int nblk = (vg + kS1Block - 1) / kS1Block;
    const long long blocks = s1_blocks(b, vg), total = (long long)b * vg, nfaces = (long long)b * nf, fblocks = (nfaces + kS1Block - 1) / kS1Block;
    G4D_REQUIRE(v > 0, "g4d_stage1_garment_f32: no body vertices");
    G4D_REQUIRE(blocks <= 0x7fffffffLL && fblocks <= 0x7fffffffLL && (long long)nf * 3 <= 0x7fffffffLL && (long long)vg * 3 <= 0x7fffffffLL,
                "g4d_stage1_garment_f32: problem too large (%lld vertex, %lld face workgroups)", blocks, fblocks);
    G4D_REQUIRE(pred && target && root && body && normals && nn_idx && inc_rowptr && ws, "g4d_stage1_garment_f32: null pointer");
    G4D_REQUIRE(nf == 0 || (faces && inc), "g4d_stage1_garment_f32: faces without their arrays");
    G4D_REQUIRE(pdim == 0 || (coeff && coeff_gt), "g4d_stage1_garment_f32: PCA coefficients without their arrays");
    const double n = (double)b * vg, nl = (double)bp * vg, w0 = 1.0 + (double)bp - (double)b, np_ = (double)b * pdim;
    float *partials = ws, *h_target = ws + blocks * kS1Terms, *h_pred = h_target + nfaces * 3, *u = grad_pred ? h_pred + nfaces * 3 : nullptr;
    if (nf > 0)
        hipLaunchKernelGGL(s1_cot_kernel, dim3((unsigned)fblocks, 2), dim3(kS1Block), 0, st, nfaces, vg, nf, target, pred, faces, h_target, h_pred);
    S1Args a;
    a.b = b; a.vg = vg; a.v = v; a.nf = nf; a.nblk = nblk; a.idx_stride = idx_stride;
    a.p = pred; a.g = target; a.root = root; a.body = body; a.normals = normals; a.nn_idx = nn_idx; a.faces = faces; a.rowptr = inc_rowptr; a.inc = inc;
    a.h_target = h_target; a.h_pred = h_pred; a.c_l2 = (float)(2.0 * w_l2 / n); a.c_pen = (float)(w_pen / n);
    a.partials = partials; a.u = u; a.grad = grad_pred;
    hipLaunchKernelGGL(s1_terms_kernel, dim3((unsigned)blocks), dim3(kS1Block), 0, st, a);
    if (grad_pred && w_lap != 0.f && nf > 0)
        hipLaunchKernelGGL(s1_lap_grad_kernel, dim3((unsigned)((total + kS1Block - 1) / kS1Block)), dim3(kS1Block), 0, st, total, vg, nf, u, h_pred, faces,
                           inc_rowptr, inc, (float)(w_lap * w0 / nl), (float)(w_lap / nl), grad_pred);
    const long long npca = (long long)b * pdim;
    hipLaunchKernelGGL(s1_finish_kernel, dim3(1), dim3(kS1Block), 0, st, b, nblk, partials, (float)w0, (float)(1.0 / n), (float)(1.0 / nl), npca, coeff, coeff_gt,
                       npca ? (float)(1.0 / np_) : 0.f, npca ? (float)(2.0 * w_pca / np_) : 0.f, grad_coeff, out);
    return check_launch("g4d_stage1_garment_f32");
}

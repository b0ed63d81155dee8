// Garment post-processing (utils/post_processing.py:179-228, :299-319): what turns the last refinement round into the mesh the reference shows.
//   taubin_smooth       : the 100 alternating Laplacian steps  S <- S + c_it * (adj . S)  (c_it = lam on even, mu on odd steps) in ONE launch,
//                         the sibling of garment_ops.hip's jacobi_smooth_kernel (same slab layout, same arithmetic order per step).
//   vertex_normals_area : psbody's VertNormals -- SCALED face normals (v1 - v0) x (v2 - v0) summed per vertex, normalised once.
//   depen_targets       : one depenetration round's flags, targets and weights, and the per-frame count of flagged vertices.
//   depen_solve         : (L^T L + diag(w^2)) x = L^T L v + w^2 t by conjugate gradients from x0 = v, one workgroup per (frame, coordinate).
// No atomics; every reduction is a fixed tree over the workgroup, so two runs give the same bits.  A frame whose count is 0 passes through
// depen_solve unchanged: the count written by depen_targets IS the per-frame flag the later kernels read (no host round trip).
#include "g4d_common.h"

namespace g4d {

constexpr int kPThreads = 1024, kPCols = 4, kPDeg = 8, kPVerts = 5;   // up to 5 * 1024 vertices per workgroup; 5104 is what the LDS slab admits
constexpr int kPMaxVg = 5104;

__global__ void __launch_bounds__(kPThreads) taubin_smooth_kernel(int vg, int c, int iters, float lam, float mu, const float *__restrict__ S,
                                                                 const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                                 const float *__restrict__ vals, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float tbuf[];  // [2][vg][4]
    const int t = threadIdx.x;
    const int slabs = (c + kPCols - 1) / kPCols;
    const int f = blockIdx.x / slabs, c0 = (blockIdx.x - f * slabs) * kPCols;
    const float *src = S + (size_t)f * vg * c;
    float *dst = out + (size_t)f * vg * c;
    float4 *cur = reinterpret_cast<float4 *>(tbuf), *nxt = cur + vg;
    int col[kPVerts][kPDeg];
    float val[kPVerts][kPDeg];
#pragma unroll
    for (int i = 0; i < kPVerts; ++i) {
        const int v = t + i * kPThreads;
        const int beg = v < vg ? rowptr[v] : 0, end = v < vg ? rowptr[v + 1] : 0;
#pragma unroll
        for (int e = 0; e < kPDeg; ++e) {
            const bool ok = beg + e < end;
            col[i][e] = ok ? colidx[beg + e] : 0;
            val[i][e] = ok ? vals[beg + e] : 0.f;
        }
        if (v < vg) {
            float4 x;
            x.x = c0 + 0 < c ? src[(size_t)v * c + c0 + 0] : 0.f; x.y = c0 + 1 < c ? src[(size_t)v * c + c0 + 1] : 0.f;
            x.z = c0 + 2 < c ? src[(size_t)v * c + c0 + 2] : 0.f; x.w = c0 + 3 < c ? src[(size_t)v * c + c0 + 3] : 0.f;
            cur[v] = x;
        }
    }
    __syncthreads();
    for (int it = 0; it < iters; ++it) {
        const float coeff = (it & 1) ? mu : lam;
#pragma unroll
        for (int i = 0; i < kPVerts; ++i) {
            const int v = t + i * kPThreads;
            if (v >= vg) break;
            float4 acc = {0.f, 0.f, 0.f, 0.f};
            const int deg = rowptr[v + 1] - rowptr[v];   // only the loop bound; the entries are in registers
#pragma unroll
            for (int e = 0; e < kPDeg; ++e) {
                if (e >= deg) break;
                const float4 y = cur[col[i][e]];
                const float a = val[i][e];
                acc.x += a * y.x; acc.y += a * y.y; acc.z += a * y.z; acc.w += a * y.w;   // g4d_spmm_axpy_rows_f32's order: CSR order, then self + coeff * acc
            }
            const float4 self = cur[v];
            nxt[v] = make_float4(self.x + coeff * acc.x, self.y + coeff * acc.y, self.z + coeff * acc.z, self.w + coeff * acc.w);
        }
        __syncthreads();
        float4 *tmp = cur; cur = nxt; nxt = tmp;
    }
    for (int v = t; v < vg; v += kPThreads) {
        const float4 x = cur[v];
        if (c0 + 0 < c) dst[(size_t)v * c + c0 + 0] = x.x;
        if (c0 + 1 < c) dst[(size_t)v * c + c0 + 1] = x.y;
        if (c0 + 2 < c) dst[(size_t)v * c + c0 + 2] = x.z;
        if (c0 + 3 < c) dst[(size_t)v * c + c0 + 3] = x.w;
    }
}

__global__ void __launch_bounds__(256) vertex_normals_area_kernel(long long total, int v, const float *__restrict__ verts_all,
                                                                 const int *__restrict__ faces, const int *__restrict__ rowptr,
                                                                 const int *__restrict__ fid, const int *__restrict__ frame_active,
                                                                 float *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const long long f = gid / v;
    if (frame_active && frame_active[f] == 0) return;
    const int vid = (int)(gid - f * v);
    const float *verts = verts_all + (size_t)f * v * 3;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int e = rowptr[vid]; e < rowptr[vid + 1]; ++e) {
        const int *tri = faces + (size_t)fid[e] * 3;
        const float *p0 = verts + (size_t)tri[0] * 3, *p1 = verts + (size_t)tri[1] * 3, *p2 = verts + (size_t)tri[2] * 3;
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        sx += ay * bz - az * by; sy += az * bx - ax * bz; sz += ax * by - ay * bx;
    }
    const float d = sqrtf(sx * sx + sy * sy + sz * sz);
    const bool ok = d > 0.f;
    out[gid * 3 + 0] = ok ? sx / d : 0.f; out[gid * 3 + 1] = ok ? sy / d : 0.f; out[gid * 3 + 2] = ok ? sz / d : 0.f;
}

// sum of one int per thread over a 256-thread workgroup, the same value in every thread (integers: any order gives the same sum)
__device__ __forceinline__ int block_sum_256(int x, int *red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    const int s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(256) depen_targets_kernel(int vg, float eps, float ww, const float *__restrict__ verts, const float *__restrict__ near_p,
                                                           const float *__restrict__ near_n, const float *__restrict__ garment_n,
                                                           const int *__restrict__ frame_active, float *__restrict__ w2, float *__restrict__ target,
                                                           int *__restrict__ counts) {
    __shared__ int red[4];
    const int f = blockIdx.x;
    if (frame_active && frame_active[f] == 0) {   // block-uniform: a finished frame stays finished
        if (threadIdx.x == 0) counts[f] = 0;
        return;
    }
    int n = 0;
    for (int v = threadIdx.x; v < vg; v += 256) {
        const size_t g = ((size_t)f * vg + v) * 3;
        const float vx = verts[g], vy = verts[g + 1], vz = verts[g + 2];
        const float px = near_p[g], py = near_p[g + 1], pz = near_p[g + 2];
        const float nx = near_n[g], ny = near_n[g + 1], nz = near_n[g + 2];
        const float mx = garment_n[g], my = garment_n[g + 1], mz = garment_n[g + 2];
        const float side = ((vx - px) * nx + (vy - py) * ny) + (vz - pz) * nz;
        const bool flagged = side < 0.f;
        const float mn = (mx * nx + my * ny) + mz * nz;
        const float s = mn > 0.f ? 1.f : (mn < 0.f ? -1.f : 0.f);
        const float dx = (px - vx) * s, dy = (py - vy) * s, dz = (pz - vz) * s;
        const float len = 1.e-4f + sqrtf((dx * dx + dy * dy) + dz * dz);
        target[g] = flagged ? px + (eps * dx) / len : vx;
        target[g + 1] = flagged ? py + (eps * dy) / len : vy;
        target[g + 2] = flagged ? pz + (eps * dz) / len : vz;
        w2[(size_t)f * vg + v] = flagged ? ww * ww : 1.f;
        n += flagged ? 1 : 0;
    }
    n = block_sum_256(n, red);
    if (threadIdx.x == 0) counts[f] = n;
}

// sum over the 1024 threads in a fixed order: xor butterfly inside each wave (commutative pairs: every lane holds the same bits), then the
// sixteen wave sums left to right.  Returns the same value in every thread.
__device__ __forceinline__ float block_sum_1024(float x, float *red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < kPThreads / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

// One workgroup per (frame, coordinate).  A thread owns the vertices t, t + 1024, ...: their rows of L sit in registers (<= 8 values and
// 16-bit columns each); the rows of L^T are re-read from global memory (L2) at every product -- both operators at vg = 5104 would need most
// of the CU's 128k vector registers.  x, r, p, q = L p, b, m = L^T q and w^2 live in LDS (7 vg floats).  M y = L^T (L y) + w^2 y, in that order.
constexpr int kSolveArrays = 7;

template <int VERTS>
__global__ void __launch_bounds__(kPThreads) depen_solve_kernel(int vg, int iters, const float *__restrict__ verts, const float *__restrict__ w2_all,
                                                               const float *__restrict__ target, const int *__restrict__ counts,
                                                               const int *__restrict__ rowptr, const int *__restrict__ colidx, const float *__restrict__ vals,
                                                               const int *__restrict__ rowptr_t, const int *__restrict__ colidx_t,
                                                               const float *__restrict__ vals_t, float *__restrict__ out, float *__restrict__ residual) {
    extern __shared__ __attribute__((aligned(16))) float sbuf[];   // x | r | p | q | b | m | w2, vg floats each, then 16 partial sums
    const int t = threadIdx.x;
    const int f = blockIdx.x / 3, cc = blockIdx.x - f * 3;
    const float *src = verts + (size_t)f * vg * 3 + cc;
    float *dst = out + (size_t)f * vg * 3 + cc;
    if (counts[f] == 0) {   // block-uniform: nothing behind the body in this frame -- the vertices pass through bit for bit
        for (int v = t; v < vg; v += kPThreads) dst[(size_t)v * 3] = src[(size_t)v * 3];
        if (t == 0) residual[(size_t)f * 3 + cc] = 0.f;
        return;
    }
    float *xs = sbuf, *rs = xs + vg, *ps = rs + vg, *qs = ps + vg, *bs = qs + vg, *ms = bs + vg, *ws = ms + vg, *red = ws + vg;
    unsigned col2[VERTS][kPDeg / 2];   // two 16-bit column indices per register (vg <= 5104)
    float val[VERTS][kPDeg];
#pragma unroll
    for (int i = 0; i < VERTS; ++i) {
        const int v = t + i * kPThreads;
        const int beg = v < vg ? rowptr[v] : 0, end = v < vg ? rowptr[v + 1] : 0;
#pragma unroll
        for (int e = 0; e < kPDeg; ++e) {
            const bool ok = beg + e < end;
            const unsigned cj = ok ? (unsigned)colidx[beg + e] : 0u;    // padding: + 0 * y[0]
            col2[i][e >> 1] = (e & 1) ? (col2[i][e >> 1] | (cj << 16)) : cj;
            val[i][e] = ok ? vals[beg + e] : 0.f;
        }
        if (v < vg) {
            xs[v] = src[(size_t)v * 3];
            ws[v] = w2_all[(size_t)f * vg + v];
        }
    }
    __syncthreads();
    // ms = L^T (L y) for the owned vertices; y is an LDS array every thread may read.  qs is read here until the caller's next barrier: every
    // caller runs a block_sum (two barriers) before qs is written again.
    auto lt_l = [&](const float *y) {
#pragma unroll
        for (int i = 0; i < VERTS; ++i) {
            const int v = t + i * kPThreads;
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < kPDeg; ++e) acc += val[i][e] * y[(e & 1) ? (col2[i][e >> 1] >> 16) : (col2[i][e >> 1] & 0xffffu)];
            if (v < vg) qs[v] = acc;
        }
        __syncthreads();
        for (int v = t; v < vg; v += kPThreads) {
            const int beg = rowptr_t[v], end = rowptr_t[v + 1];
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < kPDeg; ++e) {
                const bool ok = beg + e < end;
                const int cj = ok ? colidx_t[beg + e] : 0;
                const float a = ok ? vals_t[beg + e] : 0.f;
                acc += a * qs[cj];
            }
            ms[v] = acc;   // read back by its owner only
        }
    };
    // b = L^T L v + w^2 t,  r0 = b - M x0 (x0 = v),  p0 = r0
    lt_l(xs);
    float part = 0.f;
    for (int v = t; v < vg; v += kPThreads) {
        const float b = ms[v] + ws[v] * target[((size_t)f * vg + v) * 3 + cc];
        const float r0 = b - (ms[v] + ws[v] * xs[v]);
        bs[v] = b; rs[v] = r0; ps[v] = r0;
        part += r0 * r0;
    }
    float rr = block_sum_1024(part, red);   // its barriers also publish ps and retire the reads of qs
    for (int it = 0; it < iters; ++it) {
        lt_l(ps);
        part = 0.f;
        for (int v = t; v < vg; v += kPThreads) {
            const float ap = ms[v] + ws[v] * ps[v];
            ms[v] = ap;
            part += ps[v] * ap;
        }
        const float pap = block_sum_1024(part, red);
        const float alpha = pap > 0.f ? rr / pap : 0.f;
        part = 0.f;
        for (int v = t; v < vg; v += kPThreads) {
            xs[v] = xs[v] + alpha * ps[v];
            const float r = rs[v] - alpha * ms[v];
            rs[v] = r;
            part += r * r;
        }
        const float rr_new = block_sum_1024(part, red);
        const float beta = rr > 0.f ? rr_new / rr : 0.f;
        for (int v = t; v < vg; v += kPThreads) ps[v] = rs[v] + beta * ps[v];
        rr = rr_new;
        __syncthreads();
    }
    // |b - M x| / |b| at exit, from a fresh product (not the recurrence's r)
    lt_l(xs);
    float pr = 0.f, pb = 0.f;
    for (int v = t; v < vg; v += kPThreads) {
        const float x = xs[v], b = bs[v];
        const float r = b - (ms[v] + ws[v] * x);
        pr += r * r; pb += b * b;
        dst[(size_t)v * 3] = x;
    }
    const float rn = block_sum_1024(pr, red), bn = block_sum_1024(pb, red);
    if (t == 0) residual[(size_t)f * 3 + cc] = bn > 0.f ? sqrtf(rn) / sqrtf(bn) : 0.f;
}

template <int VERTS>
static int launch_depen_solve(int frames, int vg, int iters, const float *verts, const float *w2, const float *target, const int *counts, const int *rowptr,
                              const int *colidx, const float *vals, const int *rowptr_t, const int *colidx_t, const float *vals_t, float *out,
                              float *residual, hipStream_t st) {
    const size_t lds = ((size_t)kSolveArrays * vg + kPThreads / 64) * sizeof(float);   // 142,976 bytes at vg = 5104
    static unsigned long long attr = 0;  // one bit per device (per instantiation)
    if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(depen_solve_kernel<VERTS>), 160 * 1024 - 512, attr, "g4d_depen_solve_f32")) return rc;
    hipLaunchKernelGGL(depen_solve_kernel<VERTS>, dim3((unsigned)frames * 3u), dim3(kPThreads), lds, st, vg, iters, verts, w2, target, counts, rowptr,
                       colidx, vals, rowptr_t, colidx_t, vals_t, out, residual);
    return check_launch("g4d_depen_solve_f32");
}

}  // namespace g4d

using namespace g4d;

extern "C" int g4d_taubin_smooth_f32(int frames, int vg, int c, int iters, float lam, float mu, int max_row_entries, const float *S, const int *rowptr,
                                     const int *colidx, const float *vals, float *out, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && vg >= 0 && c >= 0 && iters >= 0 && max_row_entries >= 0, "g4d_taubin_smooth_f32: negative size");
    G4D_REQUIRE(vg <= kPMaxVg && max_row_entries <= kPDeg, "g4d_taubin_smooth_f32: needs vg <= %d and <= %d entries per adjacency row (vg=%d, max row=%d)",
                kPMaxVg, kPDeg, vg, max_row_entries);
    if (frames == 0 || vg == 0 || c == 0) return G4D_OK;
    G4D_REQUIRE(S && rowptr && colidx && vals && out, "g4d_taubin_smooth_f32: null pointer");
    const long long blocks = (long long)frames * ((c + kPCols - 1) / kPCols);
    G4D_REQUIRE(blocks < (1ll << 31), "g4d_taubin_smooth_f32: too large");
    const size_t lds = (size_t)2 * vg * sizeof(float4);
    static unsigned long long attr = 0;  // one bit per device
    if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(taubin_smooth_kernel), 160 * 1024 - 512, attr, "g4d_taubin_smooth_f32")) return rc;
    hipLaunchKernelGGL(taubin_smooth_kernel, dim3((unsigned)blocks), dim3(kPThreads), lds, reinterpret_cast<hipStream_t>(stream), vg, c, iters, lam, mu, S,
                       rowptr, colidx, vals, out);
    return check_launch("g4d_taubin_smooth_f32");
}

extern "C" int g4d_vertex_normals_area_f32(int frames, int v, const float *verts, const int *faces, const int *vf_rowptr, const int *vf_fid,
                                           const int *frame_active, float *out, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && v >= 0, "g4d_vertex_normals_area_f32: negative size");
    const long long total = (long long)frames * v;
    if (total == 0) return G4D_OK;
    G4D_REQUIRE(verts && faces && vf_rowptr && vf_fid && out, "g4d_vertex_normals_area_f32: null pointer");
    G4D_REQUIRE((total + 255) / 256 < (1ll << 31), "g4d_vertex_normals_area_f32: too large");
    hipLaunchKernelGGL(vertex_normals_area_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), total, v,
                       verts, faces, vf_rowptr, vf_fid, frame_active, out);
    return check_launch("g4d_vertex_normals_area_f32");
}

extern "C" int g4d_depen_targets_f32(int frames, int vg, float eps, float ww, const float *verts, const float *near_p, const float *near_n,
                                     const float *garment_n, const int *frame_active, float *w2, float *target, int *counts, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && vg >= 0, "g4d_depen_targets_f32: negative size");
    if (frames == 0) return G4D_OK;
    G4D_REQUIRE(counts && (vg == 0 || (verts && near_p && near_n && garment_n && w2 && target)), "g4d_depen_targets_f32: null pointer");
    hipLaunchKernelGGL(depen_targets_kernel, dim3((unsigned)frames), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), vg, eps, ww, verts, near_p,
                       near_n, garment_n, frame_active, w2, target, counts);
    return check_launch("g4d_depen_targets_f32");
}

extern "C" int g4d_depen_solve_f32(int frames, int vg, int cg_iters, int max_row_entries, int max_row_entries_t, const float *verts, const float *w2,
                                   const float *target, const int *counts, const int *rowptr, const int *colidx, const float *vals,
                                   const int *rowptr_t, const int *colidx_t, const float *vals_t, float *out, float *residual, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && vg >= 0 && cg_iters >= 0 && max_row_entries >= 0 && max_row_entries_t >= 0, "g4d_depen_solve_f32: negative size");
    G4D_REQUIRE(vg <= kPMaxVg && max_row_entries <= kPDeg && max_row_entries_t <= kPDeg,
                "g4d_depen_solve_f32: needs vg <= %d and <= %d entries per row of L and of L^T (vg=%d, max row=%d, max row of L^T=%d)", kPMaxVg, kPDeg, vg,
                max_row_entries, max_row_entries_t);
    if (frames == 0 || vg == 0) return G4D_OK;
    G4D_REQUIRE(verts && w2 && target && counts && rowptr && colidx && vals && rowptr_t && colidx_t && vals_t && out && residual,
                "g4d_depen_solve_f32: null pointer");
    G4D_REQUIRE((long long)frames * 3 < (1ll << 31), "g4d_depen_solve_f32: too large");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define G4D_SOLVE(N) return launch_depen_solve<N>(frames, vg, cg_iters, verts, w2, target, counts, rowptr, colidx, vals, rowptr_t, colidx_t, vals_t, out, residual, st)
    switch ((vg + kPThreads - 1) / kPThreads) {
        case 1: G4D_SOLVE(1);
        case 2: G4D_SOLVE(2);
        case 3: G4D_SOLVE(3);
        case 4: G4D_SOLVE(4);
        default: G4D_SOLVE(5);
    }
#undef G4D_SOLVE
}

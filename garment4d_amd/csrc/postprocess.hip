// Garment post-processing (utils/post_processing.py:179-228, :299-319): what turns the last refinement round into the mesh the reference shows.
//   depen_targets       : one depenetration round's flags, targets and weights, and the per-frame count of flagged vertices.
//   depen_solve         : (L^T L + diag(w^2)) x = L^T L v + w^2 t by conjugate gradients from x0 = v, one workgroup per (frame, coordinate).
// (The Taubin smoothing in front of them is garment_ops.hip's smooth_steps_kernel, the garment's vertex normals mesh_ops.hip's area form.)
// No atomics; every reduction is reduce.h's block_sum, a fixed tree over the workgroup, so two runs give the same bits.  A frame whose count
// is 0 passes through depen_solve unchanged: the count written by depen_targets IS the per-frame flag the later kernels read (no host round trip).
#include "reduce.h"

namespace g4d {

constexpr int kPThreads = 1024, kPDeg = 8;
constexpr int kPMaxVg = 5104;   // the solver's own limit, set to the domain of the smoothing that runs in front of it (garment_ops.hip)

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
    n = block_sum<4>(n, red);   // (integers: any order gives the same sum)
    if (threadIdx.x == 0) counts[f] = n;
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
    float rr = block_sum<kPThreads / 64>(part, red);   // its barriers also publish ps and retire the reads of qs
    for (int it = 0; it < iters; ++it) {
        lt_l(ps);
        part = 0.f;
        for (int v = t; v < vg; v += kPThreads) {
            const float ap = ms[v] + ws[v] * ps[v];
            ms[v] = ap;
            part += ps[v] * ap;
        }
        const float pap = block_sum<kPThreads / 64>(part, red);
        const float alpha = pap > 0.f ? rr / pap : 0.f;
        part = 0.f;
        for (int v = t; v < vg; v += kPThreads) {
            xs[v] = xs[v] + alpha * ps[v];
            const float r = rs[v] - alpha * ms[v];
            rs[v] = r;
            part += r * r;
        }
        const float rr_new = block_sum<kPThreads / 64>(part, red);
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
    const float rn = block_sum<kPThreads / 64>(pr, red), bn = block_sum<kPThreads / 64>(pb, red);
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

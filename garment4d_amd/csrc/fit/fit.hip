// Point-to-surface loss and its gradient (include/g4d_fit.h is the contract; tests/fit_twin.py restates it in numpy).
//   point_face_kernel : one workgroup of kFitLanes lanes per frame, lanes on points.  The closest point on the face the search reported, by the
//                       search's own routine (closest_triangle.h: the same bits), as barycentric weights and residual; the frame's weighted
//                       sums by block_sum (reduce.h).  total_kernel: W and the loss, frames in ascending order.
//   group_kernel      : one workgroup per frame: the packed keys face << 15 | index of the inliers, bitonic-sorted in LDS.
//   vertex_grad_kernel: one thread per (frame, vertex): its corners in CSR order, the run of each face found by bisection in the sorted keys.
//   point_grad_kernel : one thread per (frame, point).
// No atomics: a value is written by the one thread that owns it; every sum has one order.
#include "../closest_triangle.h"
#include "../g4d_common.h"
#include "../reduce.h"
#include "../../../include/g4d_fit.h"

#include <math.h>

namespace g4d {

constexpr int kFitLanes = G4D_FIT_LANES, kFitWaves = kFitLanes / kWave;
constexpr int kIndexBits = 15;
constexpr unsigned kNoKey = 0xFFFFFFFFu;
static_assert((1 << kIndexBits) == G4D_FIT_MAX_POINTS && ((long long)G4D_FIT_MAX_FACES << kIndexBits) == (1ll << 32), "a key is 17 + 15 bits");

__global__ void __launch_bounds__(kFitLanes) point_face_kernel(int p, int v, int nf, const float *__restrict__ points, const float *__restrict__ verts_all,
                                                               const int *__restrict__ faces, const int *__restrict__ face,
                                                               const float *__restrict__ weights, float tau2, float *__restrict__ bary,
                                                               float *__restrict__ resid, float *__restrict__ dist2, int *__restrict__ inlier,
                                                               float *__restrict__ sums, int *__restrict__ count) {
    __shared__ float sh_f[kFitWaves];
    __shared__ int sh_i[kFitWaves];
    const int f = blockIdx.x;
    const float *verts = verts_all + (size_t)f * v * 3;
    float s_d2 = 0.f, s_in = 0.f, s_all = 0.f;
    int n = 0;
    for (int i = threadIdx.x; i < p; i += kFitLanes) {
        const size_t g = (size_t)f * p + i;
        const float wt = weights ? weights[g] : 1.f;
        const int t = face[g];
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, rx = 0.f, ry = 0.f, rz = 0.f, d2 = INFINITY;
        bool usable = (unsigned)t < (unsigned)nf;
        if (usable) {
            const int ia = faces[(size_t)t * 3], ib = faces[(size_t)t * 3 + 1], ic = faces[(size_t)t * 3 + 2];
            usable = (unsigned)ia < (unsigned)v && (unsigned)ib < (unsigned)v && (unsigned)ic < (unsigned)v;
            if (usable) {
                const float qx = points[g * 3], qy = points[g * 3 + 1], qz = points[g * 3 + 2];
                const float *a = verts + (size_t)ia * 3, *b = verts + (size_t)ib * 3, *c = verts + (size_t)ic * 3;
                const Closest o = closest_on_triangle(qx, qy, qz, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
                b0 = (1.f - o.v) - o.w; b1 = o.v; b2 = o.w;
                rx = qx - o.x; ry = qy - o.y; rz = qz - o.z;
                d2 = o.d2;
            }
        }
        const bool in = usable && wt > 0.f && d2 < tau2;
        bary[g * 3] = b0; bary[g * 3 + 1] = b1; bary[g * 3 + 2] = b2;
        resid[g * 3] = rx; resid[g * 3 + 1] = ry; resid[g * 3 + 2] = rz;
        dist2[g] = d2;
        inlier[g] = in ? 1 : 0;
        s_all = s_all + wt;
        if (in) {
            s_d2 = s_d2 + wt * d2;
            s_in = s_in + wt;
            ++n;
        }
    }
    s_d2 = block_sum<kFitWaves>(s_d2, sh_f);
    s_in = block_sum<kFitWaves>(s_in, sh_f);
    s_all = block_sum<kFitWaves>(s_all, sh_f);
    n = block_sum<kFitWaves>(n, sh_i);
    if (threadIdx.x == 0) {
        sums[(size_t)f * 3] = s_d2; sums[(size_t)f * 3 + 1] = s_in; sums[(size_t)f * 3 + 2] = s_all;
        count[f] = n;
    }
}

__global__ void __launch_bounds__(kWave) total_kernel(int frames, const float *__restrict__ sums, float *__restrict__ total) {
    if (threadIdx.x != 0) return;
    float W = 0.f, T = 0.f;
    for (int f = 0; f < frames; ++f) {
        T = T + sums[(size_t)f * 3];
        W = W + sums[(size_t)f * 3 + 2];
    }
    total[0] = W;
    total[1] = W > 0.f ? T / W : 0.f;
}

// n2: the power of two the network runs over (>= p, >= 64); blockDim.x = min(kFitLanes, n2 / 2) lanes, each on n2 / 2 / blockDim.x pairs per pass.
// Pair t of a pass with stride j is (i, i | j), i = t with a 0 inserted at bit j: for j >= 64 the lanes of a wave touch consecutive words.
__global__ void __launch_bounds__(kFitLanes) group_kernel(int p, int nf, int n2, const int *__restrict__ face, const int *__restrict__ inlier,
                                                          unsigned *__restrict__ keys) {
    extern __shared__ unsigned s_key[];
    const int f = blockIdx.x, T = blockDim.x;
    for (int i = threadIdx.x; i < n2; i += T) {
        unsigned k = kNoKey;
        if (i < p) {
            const size_t g = (size_t)f * p + i;
            const int t = face[g];
            if (inlier[g] != 0 && (unsigned)t < (unsigned)nf) k = ((unsigned)t << kIndexBits) | (unsigned)i;
        }
        s_key[i] = k;
    }
    __syncthreads();
    const int half = n2 >> 1;
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < half; t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned a = s_key[i], b = s_key[l];
                if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[l] = a; }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < p; i += T) keys[(size_t)f * p + i] = s_key[i];
}

struct GradScale {
    float gs, gp;
};

__device__ __forceinline__ GradScale grad_scale(const float *__restrict__ total, const float *__restrict__ grad_out) {
    const float W = total[0], g = grad_out[0];
    GradScale o;
    o.gs = W > 0.f ? (-2.f * g) / W : 0.f;
    o.gp = W > 0.f ? (2.f * g) / W : 0.f;
    return o;
}

__global__ void __launch_bounds__(256) vertex_grad_kernel(long long rows, int p, int v, int nf, const float *__restrict__ bary,
                                                          const float *__restrict__ resid, const float *__restrict__ weights,
                                                          const unsigned *__restrict__ keys_all, const int *__restrict__ count,
                                                          const float *__restrict__ total, const float *__restrict__ grad_out,
                                                          const int *__restrict__ rowptr, const int *__restrict__ corners, float *__restrict__ grad_verts) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows) return;
    const int f = (int)(gid / v), vi = (int)(gid - (long long)f * v);
    const float gs = grad_scale(total, grad_out).gs;
    const unsigned *keys = keys_all + (size_t)f * p;
    const int n = min(max(count[f], 0), p);
    const int beg = max(rowptr[vi], 0), end = min(rowptr[vi + 1], nf * 3);   // nf <= 2^17: no overflow
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int e = beg; e < end; ++e) {
        const int c = corners[e];
        if ((unsigned)c >= (unsigned)(nf * 3)) continue;
        const unsigned t = (unsigned)c / 3u, corner = (unsigned)c - t * 3u;
        const unsigned first = t << kIndexBits;
        int lo = 0, hi = n;   // the first position whose key is >= first
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < first) lo = mid + 1; else hi = mid;
        }
        for (int j = lo; j < n; ++j) {
            const unsigned key = keys[j];
            if ((key >> kIndexBits) != t) break;
            const int i = (int)(key & (unsigned)(G4D_FIT_MAX_POINTS - 1));
            if (i >= p) continue;
            const size_t g = (size_t)f * p + i;
            const float wt = weights ? weights[g] : 1.f;
            const float s = (gs * wt) * bary[g * 3 + corner];
            ax = ax + s * resid[g * 3]; ay = ay + s * resid[g * 3 + 1]; az = az + s * resid[g * 3 + 2];
        }
    }
    grad_verts[gid * 3] = ax; grad_verts[gid * 3 + 1] = ay; grad_verts[gid * 3 + 2] = az;
}

__global__ void __launch_bounds__(256) point_grad_kernel(long long rows, const float *__restrict__ resid, const int *__restrict__ inlier,
                                                         const float *__restrict__ weights, const float *__restrict__ total,
                                                         const float *__restrict__ grad_out, float *__restrict__ grad_points) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows) return;
    const float gp = grad_scale(total, grad_out).gp;
    const bool in = inlier[g] != 0;
    const float s = gp * (weights ? weights[g] : 1.f);
#pragma unroll
    for (int k = 0; k < 3; ++k) grad_points[g * 3 + k] = in ? s * resid[g * 3 + k] : 0.f;
}

static int sort_size(int p) {
    int n2 = kWave;
    while (n2 < p) n2 <<= 1;
    return n2;
}

}  // namespace g4d

using namespace g4d;

extern "C" int g4d_fit_point_face_f32(int frames, int p, int v, int nf, const float *points, const float *verts, const int *faces, const int *face,
                                      const float *weights, float tau2, float *bary, float *resid, float *dist2, int *inlier, float *sums, int *count,
                                      float *total, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && p >= 0 && v >= 0 && nf >= 0, "g4d_fit_point_face_f32: negative size");
    if (frames == 0 || p == 0) return G4D_OK;
    G4D_REQUIRE(v > 0 && nf > 0, "g4d_fit_point_face_f32: empty mesh (v=%d, nf=%d)", v, nf);
    G4D_REQUIRE(points && verts && faces && face && bary && resid && dist2 && inlier && sums && count && total, "g4d_fit_point_face_f32: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(point_face_kernel, dim3((unsigned)frames), dim3(kFitLanes), 0, st, p, v, nf, points, verts, faces, face, weights, tau2, bary, resid,
                       dist2, inlier, sums, count);
    if (const int rc = check_launch("g4d_fit_point_face_f32 (terms)")) return rc;
    hipLaunchKernelGGL(total_kernel, dim3(1), dim3(kWave), 0, st, frames, sums, total);
    return check_launch("g4d_fit_point_face_f32");
}

extern "C" size_t g4d_fit_group_lds_bytes(int p) {
    if (p < 0 || p > G4D_FIT_MAX_POINTS) return (size_t)-1;
    return (size_t)sort_size(p) * sizeof(unsigned);
}

extern "C" int g4d_fit_group_f32(int frames, int p, int nf, const int *face, const int *inlier, unsigned *keys, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && p >= 0 && nf >= 0, "g4d_fit_group_f32: negative size");
    G4D_REQUIRE(p <= G4D_FIT_MAX_POINTS, "g4d_fit_group_f32: p must be <= %d (p=%d)", G4D_FIT_MAX_POINTS, p);
    G4D_REQUIRE(nf <= G4D_FIT_MAX_FACES, "g4d_fit_group_f32: nf must be <= %d (nf=%d)", G4D_FIT_MAX_FACES, nf);
    if (frames == 0 || p == 0) return G4D_OK;
    G4D_REQUIRE(face && inlier && keys, "g4d_fit_group_f32: null pointer");
    const int n2 = sort_size(p), bytes = n2 * (int)sizeof(unsigned);
    static unsigned long long lds_done = 0;
    if (bytes > 65536)
        if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(group_kernel), bytes, lds_done, "g4d_fit_group_f32")) return rc;
    const int threads = n2 / 2 < kFitLanes ? n2 / 2 : kFitLanes;
    hipLaunchKernelGGL(group_kernel, dim3((unsigned)frames), dim3(threads), bytes, reinterpret_cast<hipStream_t>(stream), p, nf, n2, face, inlier, keys);
    return check_launch("g4d_fit_group_f32");
}

extern "C" int g4d_fit_vertex_grad_f32(int frames, int p, int v, int nf, const float *bary, const float *resid, const int *inlier, const float *weights,
                                       const unsigned *keys, const int *count, const float *total, const float *grad_out, const int *vc_rowptr,
                                       const int *vc_corners, float *grad_verts, float *grad_points, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && p >= 0 && v >= 0 && nf >= 0, "g4d_fit_vertex_grad_f32: negative size");
    G4D_REQUIRE(p <= G4D_FIT_MAX_POINTS, "g4d_fit_vertex_grad_f32: p must be <= %d (p=%d)", G4D_FIT_MAX_POINTS, p);
    G4D_REQUIRE(nf <= G4D_FIT_MAX_FACES, "g4d_fit_vertex_grad_f32: nf must be <= %d (nf=%d)", G4D_FIT_MAX_FACES, nf);
    const bool want_points = grad_points != nullptr && p > 0;
    if (frames == 0 || (v == 0 && !want_points)) return G4D_OK;
    G4D_REQUIRE(count && total && grad_out, "g4d_fit_vertex_grad_f32: null pointer");
    G4D_REQUIRE(p == 0 || (bary && resid && inlier && keys), "g4d_fit_vertex_grad_f32: null pointer");
    G4D_REQUIRE(v == 0 || (vc_rowptr && grad_verts && (nf == 0 || vc_corners)), "g4d_fit_vertex_grad_f32: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long rows = (long long)frames * v, prow = (long long)frames * p;
    G4D_REQUIRE((rows + 255) / 256 < (1ll << 31) && (prow + 255) / 256 < (1ll << 31), "g4d_fit_vertex_grad_f32: too large");
    if (v > 0) {
        hipLaunchKernelGGL(vertex_grad_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, rows, p, v, nf, bary, resid, weights, keys, count, total,
                           grad_out, vc_rowptr, vc_corners, grad_verts);
        if (const int rc = check_launch("g4d_fit_vertex_grad_f32 (vertices)")) return rc;
    }
    if (want_points) {
        hipLaunchKernelGGL(point_grad_kernel, dim3((unsigned)((prow + 255) / 256)), dim3(256), 0, st, prow, resid, inlier, weights, total, grad_out, grad_points);
        return check_launch("g4d_fit_vertex_grad_f32");
    }
    return G4D_OK;
}

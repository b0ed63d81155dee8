// Projective ray-depth loss and its gradient (include/g4d_depth.h is the contract; tests/depth_fit_twin.py restates it in numpy).
//   terms_kernel      : one workgroup per (frame, chunk of kChunk samples), lanes on samples, kPerLane samples per lane, consecutive lanes on
//                       consecutive columns of the images.  face_plane() + ray_hit(): face plane, ray, depth, residual.  The chunk's four
//                       sums by block_sum (reduce.h) -> 16 bytes of scratch per chunk.
//   frame_kernel      : one workgroup per frame adds its chunks.  total_kernel: W and the loss, frames in ascending order.
//   vertex_grad_kernel: one lane per (frame, vertex): per camera its corners in CSR order, the face's plane once per face, its sample box walked
//                       row by row; the samples that show the face recompute their terms with the forward's own routines (nothing is stored per
//                       sample, nothing sorted).
// No atomics: a value is written by the one thread that owns it; every sum has one order.
#include "../g4d_common.h"
#include "../reduce.h"
#include "../../../include/g4d_depth.h"
#include "../../../include/g4d_render.h"

#include <math.h>
#include <stdint.h>

namespace g4d {

constexpr int kDLanes = G4D_DEPTH_LANES, kDWaves = kDLanes / kWave, kDPerLane = G4D_DEPTH_PER_LANE, kDChunk = kDLanes * kDPerLane;
constexpr int kDCoordLimit = 1 << G4D_RENDER_COORD_BITS;
static_assert(G4D_DEPTH_MAX_SIDE == G4D_RENDER_MAX_SAMPLES, "a sensor is at most the rasterizer's image");
static_assert(3ll * G4D_DEPTH_MAX_FACES < (1ll << 31), "a corner index fits an int32");

struct DepthCams {
    float r[G4D_DEPTH_MAX_CAMS][9], s[G4D_DEPTH_MAX_CAMS];
};

struct DepthShape {
    int frames, cams, v, nf, w, h, nchunks;   // nchunks: chunks per frame
    long long samples;                        // cams * h * w, < 2^31
    float trunc, g2;                          // g2 = grazing * grazing
};

struct DepthIn {
    const float *cam;
    const int *faces, *face_id;
    const float *depth_obs, *weights;
    const int *labels_obs, *face_labels;
};

struct ChunkSums {
    float s, win, wobs;
    int n;
};
static_assert(sizeof(ChunkSums) == 16, "g4d_depth_ws_bytes: 16 bytes per chunk");

// The plane of face g under camera c of frame f, from the un-snapped camera-space vertices in the caller's order: per (camera, frame, face),
// not per sample -- the gradient's lane forms it once per box it walks.
struct FacePlane {
    float c0[3], u[3], v[3], n[3], nn;
};

__device__ __forceinline__ FacePlane face_plane(const float *__restrict__ c0, const float *__restrict__ c1, const float *__restrict__ c2) {
    FacePlane p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p.c0[k] = c0[k]; p.u[k] = c1[k] - c0[k]; p.v[k] = c2[k] - c0[k];
    }
    p.n[0] = p.u[1] * p.v[2] - p.u[2] * p.v[1]; p.n[1] = p.u[2] * p.v[0] - p.u[0] * p.v[2]; p.n[2] = p.u[0] * p.v[1] - p.u[1] * p.v[0];
    p.nn = (p.n[0] * p.n[0] + p.n[1] * p.n[1]) + p.n[2] * p.n[2];
    return p;
}

struct RayHit {
    float r, den, b0, b1, b2;
};

// Sample (i, j) against a plane: true iff facing and |r| < trunc (the part of `inlier` that needs arithmetic); the barycentrics only on request.
template <bool BARY>
__device__ __forceinline__ bool ray_hit(const DepthShape &sh, const FacePlane &p, float s, int i, int j, float D, RayHit &o) {
    const int hh = 128 * sh.h, hw = 128 * sh.w;
    const float shh = s * (float)hh;
    const float dx = (float)(256 * j + 128 - hw) / shh, dy = (float)(hh - (256 * i + 128)) / shh;
    const float den = (p.n[0] * dx + p.n[1] * dy) + p.n[2];
    const float dd = (dx * dx + dy * dy) + 1.f;
    const bool facing = den * den > (sh.g2 * p.nn) * dd;
    const float z = ((p.n[0] * p.c0[0] + p.n[1] * p.c0[1]) + p.n[2] * p.c0[2]) / den;
    const float r = z - D;
    o.r = r; o.den = den;
    if (!(facing && fabsf(r) < sh.trunc)) return false;
    if (BARY) {
        const float qx = z * dx - p.c0[0], qy = z * dy - p.c0[1], qz = z - p.c0[2];
        const float ax = qy * p.v[2] - qz * p.v[1], ay = qz * p.v[0] - qx * p.v[2], az = qx * p.v[1] - qy * p.v[0];   // q X e2
        const float bx = p.u[1] * qz - p.u[2] * qy, by = p.u[2] * qx - p.u[0] * qz, bz = p.u[0] * qy - p.u[1] * qx;   // e1 X q
        o.b1 = ((ax * p.n[0] + ay * p.n[1]) + az * p.n[2]) / p.nn;
        o.b2 = ((bx * p.n[0] + by * p.n[1]) + bz * p.n[2]) / p.nn;
        o.b0 = (1.f - o.b1) - o.b2;
    }
    return true;
}

__global__ void __launch_bounds__(kDLanes) terms_kernel(DepthShape sh, DepthCams cams, DepthIn in, ChunkSums *__restrict__ part, float *__restrict__ resid) {
    __shared__ float sh_f[kDWaves];
    __shared__ int sh_i[kDWaves];
    const int f = blockIdx.x / sh.nchunks, chunk = blockIdx.x - f * sh.nchunks;
    const long long hw = (long long)sh.h * sh.w;
    float s_r2 = 0.f, s_in = 0.f, s_obs = 0.f;
    int n = 0;
#pragma unroll
    for (int q = 0; q < kDPerLane; ++q) {
        const long long s = (long long)chunk * kDChunk + q * kDLanes + threadIdx.x;
        if (s >= sh.samples) continue;
        const int c = (int)(s / hw);
        const long long rest = s - (long long)c * hw;
        const int i = (int)(rest / sh.w), j = (int)(rest - (long long)i * sh.w);
        const size_t at = ((size_t)c * sh.frames + f) * (size_t)hw + (size_t)rest;
        const float wt = in.weights ? in.weights[at] : 1.f, D = in.depth_obs[at];
        const int g = in.face_id[at];
        const bool observed = D > 0.f && D < INFINITY;
        bool inlier = false;
        RayHit t;
        t.r = 0.f;
        if (observed) s_obs = s_obs + wt;
        if (observed && (unsigned)g < (unsigned)sh.nf) {
            const int i0 = in.faces[(size_t)g * 3], i1 = in.faces[(size_t)g * 3 + 1], i2 = in.faces[(size_t)g * 3 + 2];
            if ((unsigned)i0 < (unsigned)sh.v && (unsigned)i1 < (unsigned)sh.v && (unsigned)i2 < (unsigned)sh.v &&
                (!in.labels_obs || in.face_labels[g] == in.labels_obs[at])) {
                const float *base = in.cam + ((size_t)c * sh.frames + f) * (size_t)sh.v * 3;
                const FacePlane p = face_plane(base + (size_t)i0 * 3, base + (size_t)i1 * 3, base + (size_t)i2 * 3);
                inlier = ray_hit<false>(sh, p, cams.s[c], i, j, D, t) && wt > 0.f;
            }
        }
        if (inlier) {
            s_r2 = s_r2 + wt * (t.r * t.r);
            s_in = s_in + wt;
            ++n;
        }
        if (resid) resid[at] = inlier ? t.r : NAN;
    }
    s_r2 = block_sum<kDWaves>(s_r2, sh_f);
    s_in = block_sum<kDWaves>(s_in, sh_f);
    s_obs = block_sum<kDWaves>(s_obs, sh_f);
    n = block_sum<kDWaves>(n, sh_i);
    if (threadIdx.x == 0) {
        const ChunkSums o = {s_r2, s_in, s_obs, n};
        part[blockIdx.x] = o;
    }
}

__global__ void __launch_bounds__(kDLanes) frame_kernel(int nchunks, const ChunkSums *__restrict__ part, float *__restrict__ sums, int *__restrict__ count) {
    __shared__ float sh_f[kDWaves];
    __shared__ int sh_i[kDWaves];
    const int f = blockIdx.x;
    float s_r2 = 0.f, s_in = 0.f, s_obs = 0.f;
    int n = 0;
    for (int k = threadIdx.x; k < nchunks; k += kDLanes) {
        const ChunkSums p = part[(size_t)f * nchunks + k];
        s_r2 = s_r2 + p.s; s_in = s_in + p.win; s_obs = s_obs + p.wobs;
        n += p.n;
    }
    s_r2 = block_sum<kDWaves>(s_r2, sh_f);
    s_in = block_sum<kDWaves>(s_in, sh_f);
    s_obs = block_sum<kDWaves>(s_obs, sh_f);
    n = block_sum<kDWaves>(n, sh_i);
    if (threadIdx.x == 0) {
        sums[(size_t)f * 3] = s_r2; sums[(size_t)f * 3 + 1] = s_in; sums[(size_t)f * 3 + 2] = s_obs;
        count[f] = n;
    }
}

__global__ void __launch_bounds__(kWave) depth_total_kernel(int frames, const float *__restrict__ sums, float *__restrict__ total) {
    if (threadIdx.x != 0) return;
    float W = 0.f, T = 0.f;
    for (int f = 0; f < frames; ++f) {
        T = T + sums[(size_t)f * 3];
        W = W + sums[(size_t)f * 3 + 2];
    }
    total[0] = W;
    total[1] = W > 0.f ? T / W : 0.f;
}

__global__ void __launch_bounds__(256) depth_vertex_grad_kernel(long long rows, DepthShape sh, DepthCams cams, DepthIn in, const int *__restrict__ px,
                                                                const int *__restrict__ py, const float *__restrict__ invz,
                                                                const float *__restrict__ total, const float *__restrict__ grad_out,
                                                                const int *__restrict__ rowptr, const int *__restrict__ corners,
                                                                float *__restrict__ grad_verts) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows) return;
    const int f = (int)(gid / sh.v), vi = (int)(gid - (long long)f * sh.v);
    const float W = total[0];
    const float gs = W > 0.f ? (2.f * grad_out[0]) / W : 0.f;
    const int beg = max(rowptr[vi], 0), end = min(rowptr[vi + 1], sh.nf * 3);
    const size_t hw = (size_t)sh.h * sh.w;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < sh.cams; ++c) {
        const size_t vbase = ((size_t)c * sh.frames + f) * (size_t)sh.v, ibase = ((size_t)c * sh.frames + f) * hw;
        const float s = cams.s[c];
        float a[3] = {0.f, 0.f, 0.f};
        for (int e = beg; e < end; ++e) {
            const int ce = corners[e];
            if ((unsigned)ce >= (unsigned)(sh.nf * 3)) continue;
            const int t = ce / 3, corner = ce - t * 3;
            int x[3], y[3], id[3];
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                id[k] = in.faces[(size_t)t * 3 + k];
                ok = ok && (unsigned)id[k] < (unsigned)sh.v;
                if (!ok) id[k] = 0;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const size_t at = vbase + id[k];
                const float iz = invz[at];
                x[k] = px[at]; y[k] = py[at];
                ok = ok && iz > 0.f && iz < INFINITY && x[k] > -kDCoordLimit && x[k] < kDCoordLimit && y[k] > -kDCoordLimit && y[k] < kDCoordLimit;
            }
            if (!ok) continue;
            if ((long long)(x[1] - x[0]) * (y[2] - y[0]) - (long long)(x[2] - x[0]) * (y[1] - y[0]) == 0) continue;
            const int j0 = max((min(x[0], min(x[1], x[2])) - 128 + 255) >> 8, 0), j1 = min((max(x[0], max(x[1], x[2])) - 128) >> 8, sh.w - 1);
            const int i0 = max((min(y[0], min(y[1], y[2])) - 128 + 255) >> 8, 0), i1 = min((max(y[0], max(y[1], y[2])) - 128) >> 8, sh.h - 1);
            if (j0 > j1 || i0 > i1) continue;
            const float *cbase = in.cam + vbase * 3;
            const FacePlane p = face_plane(cbase + (size_t)id[0] * 3, cbase + (size_t)id[1] * 3, cbase + (size_t)id[2] * 3);
            const int flabel = in.labels_obs ? in.face_labels[t] : 0;
            for (int i = i0; i <= i1; ++i)
                for (int j = j0; j <= j1; ++j) {
                    const size_t at = ibase + (size_t)i * sh.w + j;
                    if (in.face_id[at] != t) continue;
                    const float D = in.depth_obs[at], wt = in.weights ? in.weights[at] : 1.f;
                    if (!(D > 0.f && D < INFINITY) || !(wt > 0.f) || (in.labels_obs && in.labels_obs[at] != flabel)) continue;
                    RayHit m;
                    if (!ray_hit<true>(sh, p, s, i, j, D, m)) continue;
                    const float bc = corner == 0 ? m.b0 : corner == 1 ? m.b1 : m.b2;
                    const float g = (((gs * wt) * m.r) * bc) / m.den;
                    a[0] = a[0] + g * p.n[0]; a[1] = a[1] + g * p.n[1]; a[2] = a[2] + g * p.n[2];
                }
        }
        const float *R = cams.r[c];
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + ((R[k] * a[0] + R[3 + k] * a[1]) + R[6 + k] * a[2]);
    }
    grad_verts[gid * 3] = acc[0]; grad_verts[gid * 3 + 1] = acc[1]; grad_verts[gid * 3 + 2] = acc[2];
}

// The checks both entry points share; on success *samples = cams * h * w.
static int check_shape(const char *who, int frames, int cams, int v, int nf, int w, int h, const int *labels_obs, const int *face_labels, long long *samples) {
    G4D_REQUIRE(frames >= 0 && v >= 0 && nf >= 0 && w >= 0 && h >= 0, "%s: negative size", who);
    G4D_REQUIRE(cams >= 1 && cams <= G4D_DEPTH_MAX_CAMS, "%s: cams must be in [1, %d] (cams=%d)", who, G4D_DEPTH_MAX_CAMS, cams);
    G4D_REQUIRE(w <= G4D_DEPTH_MAX_SIDE && h <= G4D_DEPTH_MAX_SIDE, "%s: w and h must be <= %d (w=%d, h=%d)", who, G4D_DEPTH_MAX_SIDE, w, h);
    *samples = (long long)cams * h * w;
    G4D_REQUIRE(*samples < (1ll << 31), "%s: cams * h * w must be < 2^31 (cams=%d, w=%d, h=%d)", who, cams, w, h);
    G4D_REQUIRE(nf <= G4D_DEPTH_MAX_FACES, "%s: nf must be <= %d (nf=%d)", who, G4D_DEPTH_MAX_FACES, nf);
    G4D_REQUIRE((labels_obs == nullptr) == (face_labels == nullptr), "%s: labels_obs and face_labels go together", who);
    return G4D_OK;
}

static DepthCams load_cams(int cams, const float *cams_host) {
    DepthCams o = {};
    for (int c = 0; c < cams; ++c) {
        for (int k = 0; k < 9; ++k) o.r[c][k] = cams_host[c * 10 + k];
        o.s[c] = cams_host[c * 10 + 9];
    }
    return o;
}

}  // namespace g4d

using namespace g4d;

extern "C" int g4d_depth_chunk(void) { return kDChunk; }

extern "C" size_t g4d_depth_ws_bytes(int frames, int cams, int w, int h) {
    if (frames < 0 || cams < 0 || w < 0 || h < 0) return (size_t)-1;
    if (frames == 0 || cams == 0 || w == 0 || h == 0) return 0;
    const long long rays = (long long)w * h;   // < 2^62; times cams only once it is known to be < 2^31
    if (rays >= (1ll << 31) || rays * cams >= (1ll << 31)) return (size_t)-1;
    return (size_t)frames * (size_t)((rays * cams + kDChunk - 1) / kDChunk) * sizeof(ChunkSums);
}

extern "C" int g4d_depth_fit_terms_f32(int frames, int cams, int v, int nf, int w, int h, const float *cam, const int *faces, const int *face_id,
                                       const float *depth_obs, const float *weights, const int *labels_obs, const int *face_labels,
                                       const float *cams_host, float trunc, float grazing, void *ws, size_t ws_bytes, float *sums, int *count,
                                       float *total, float *resid, g4d_stream_t stream) {
    const char *who = "g4d_depth_fit_terms_f32";
    long long samples = 0;
    if (const int rc = check_shape(who, frames, cams, v, nf, w, h, labels_obs, face_labels, &samples)) return rc;
    if (frames == 0 || w == 0 || h == 0) return G4D_OK;
    G4D_REQUIRE(face_id && depth_obs && cams_host && ws && sums && count && total && (cam || v == 0) && (faces || nf == 0), "%s: null pointer", who);
    const size_t need = g4d_depth_ws_bytes(frames, cams, w, h);
    G4D_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    G4D_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const long long nchunks = (samples + kDChunk - 1) / kDChunk;
    G4D_REQUIRE(nchunks * frames < (1ll << 31), "%s: too large (frames * chunks >= 2^31)", who);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const DepthShape sh = {frames, cams, v, nf, w, h, (int)nchunks, samples, trunc, grazing * grazing};
    const DepthIn in = {cam, faces, face_id, depth_obs, weights, labels_obs, face_labels};
    ChunkSums *part = reinterpret_cast<ChunkSums *>(ws);
    hipLaunchKernelGGL(terms_kernel, dim3((unsigned)(nchunks * frames)), dim3(kDLanes), 0, st, sh, load_cams(cams, cams_host), in, part, resid);
    if (const int rc = check_launch("g4d_depth_fit_terms_f32 (terms)")) return rc;
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned)frames), dim3(kDLanes), 0, st, (int)nchunks, part, sums, count);
    if (const int rc = check_launch("g4d_depth_fit_terms_f32 (frames)")) return rc;
    hipLaunchKernelGGL(depth_total_kernel, dim3(1), dim3(kWave), 0, st, frames, sums, total);
    return check_launch(who);
}

extern "C" int g4d_depth_fit_vertex_grad_f32(int frames, int cams, int v, int nf, int w, int h, const int *px, const int *py, const float *invz,
                                             const float *cam, const int *faces, const int *face_id, const float *depth_obs, const float *weights,
                                             const int *labels_obs, const int *face_labels, const float *cams_host, float trunc, float grazing,
                                             const float *total, const float *grad_out, const int *vc_rowptr, const int *vc_corners,
                                             float *grad_verts, g4d_stream_t stream) {
    const char *who = "g4d_depth_fit_vertex_grad_f32";
    long long samples = 0;
    if (const int rc = check_shape(who, frames, cams, v, nf, w, h, labels_obs, face_labels, &samples)) return rc;
    if (frames == 0 || v == 0 || w == 0 || h == 0) return G4D_OK;
    G4D_REQUIRE(px && py && invz && cam && face_id && depth_obs && cams_host && total && grad_out && vc_rowptr && grad_verts &&
                    ((faces && vc_corners) || nf == 0),
                "%s: null pointer", who);
    const long long rows = (long long)frames * v;
    G4D_REQUIRE((rows + 255) / 256 < (1ll << 31), "%s: too large", who);
    const DepthShape sh = {frames, cams, v, nf, w, h, 0, samples, trunc, grazing * grazing};
    const DepthIn in = {cam, faces, face_id, depth_obs, weights, labels_obs, face_labels};
    hipLaunchKernelGGL(depth_vertex_grad_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rows, sh,
                       load_cams(cams, cams_host), in, px, py, invz, total, grad_out, vc_rowptr, vc_corners, grad_verts);
    return check_launch(who);
}

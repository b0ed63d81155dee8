// Nearest-vertex two-stage garment skinning of the MGN model variant (`PCALBSGarmentUseSegEncoderSegMGN.lbs_garment_MGN`,
// modules/mesh_encoder.py:529-585) in ONE launch.  Per (frame f of clip c, garment vertex g):
//   q  = garment[f, g] + root[c]                                      (:538, one fp32 add)
//   nn = argmin_u d(q, tpose[c, u])  under g4d_knn_f32's rounding and (distance, index) order, i.e. knn_points(K = 1) (:541)
//   s  = (sum_j W[f, nn, j] inv_A[f, j]) [q; 1]                      (:549-558, stage 1)
//   p  = (sum_j W[f, nn, j] A[f, j]) [s; 1]                          (:566-583, posed)
// The reference builds the (F, V, 4, 4) blends of ALL body vertices and gathers one row per garment vertex; here only the nearest
// vertex's row of W is blended.
//
// Search: brute force.  A workgroup of 256 threads owns 1024 consecutive queries of ONE clip (the clip's frames flattened, frame-major),
// four per thread, processed as two packed-fp32 pairs: each point of the clip's T-pose is read from LDS once (a broadcast) and compared
// with four queries.  The T-pose streams through LDS in tiles of kMgnTile points, so any V works; a tile serves every frame of the
// clip that the workgroup's queries belong to.  Distances use dist2<knn_shape(mode)> on (q - x) exactly as knn.hip does, and the
// comparison is on the distance's bit pattern (the order of knn.hip's keys), strictly smaller wins, points in ascending index:
// index and distance equal g4d_knn_f32(K = 1) bit for bit.
#include "g4d_common.h"

namespace g4d {

constexpr int kMgnThreads = 256;
constexpr int kMgnQpt = 4;                                 // queries per thread (two packed pairs)
constexpr int kMgnQueries = kMgnThreads * kMgnQpt;         // per workgroup
constexpr int kMgnTile = 2048;                             // T-pose points per LDS tile: 24 KB
constexpr int kMgnMaxJ = 64;

__device__ __forceinline__ void mgn_consider(unsigned key, int u, unsigned &best, int &bi) {
    const bool lt = key < best;
    best = lt ? key : best;
    bi = lt ? u : bi;
}

template <int FM>
__global__ void __launch_bounds__(kMgnThreads) mgn_skin_kernel(int T, int vg, int v, int nj, const float *__restrict__ garment,
                                                               const float *__restrict__ root, const float *__restrict__ tpose,
                                                               const float *__restrict__ W, const float *__restrict__ inv_A,
                                                               const float *__restrict__ A, int *__restrict__ nn_idx,
                                                               float *__restrict__ nn_dist, float *__restrict__ stage1,
                                                               float *__restrict__ posed) {
    __shared__ __attribute__((aligned(16))) float tile[kMgnTile * 3];   // (x, y, z) of kMgnTile points, as in global memory
    const int c = blockIdx.y;
    const long long nq = (long long)T * vg;                             // queries of the clip
    const long long q0 = (long long)blockIdx.x * kMgnQueries + threadIdx.x;
    const float rx = root[c * 3 + 0], ry = root[c * 3 + 1], rz = root[c * 3 + 2];
    float qx[kMgnQpt], qy[kMgnQpt], qz[kMgnQpt];
    unsigned best[kMgnQpt];
    int bi[kMgnQpt];
#pragma unroll
    for (int k = 0; k < kMgnQpt; ++k) {
        const long long qi = q0 + (long long)k * kMgnThreads;
        float x = 0.f, y = 0.f, z = 0.f;
        if (qi < nq) {
            const float *gp = garment + ((size_t)c * nq + qi) * 3;
            x = gp[0] + rx;
            y = gp[1] + ry;
            z = gp[2] + rz;
        }
        qx[k] = x, qy[k] = y, qz[k] = z;
        best[k] = 0xffffffffu;
        bi[k] = 0;
    }
    const float *body = tpose + (size_t)c * v * 3;
    for (int base = 0; base < v; base += kMgnTile) {
        const int n = min(kMgnTile, v - base);
        __syncthreads();                                                // the previous tile is no longer read
        for (int i = threadIdx.x; i < n * 3; i += kMgnThreads) tile[i] = body[(size_t)base * 3 + i];
        __syncthreads();
        const g4d_f32x2 ax = {qx[0], qx[1]}, ay = {qy[0], qy[1]}, az = {qz[0], qz[1]};
        const g4d_f32x2 bx = {qx[2], qx[3]}, by = {qy[2], qy[3]}, bz = {qz[2], qz[3]};
#pragma unroll 4
        for (int u = 0; u < n; ++u) {
            const float px = tile[u * 3 + 0], py = tile[u * 3 + 1], pz = tile[u * 3 + 2];
            const g4d_f32x2 px2 = {px, px}, py2 = {py, py}, pz2 = {pz, pz};
            const g4d_f32x2 da = dist2<FM>(ax - px2, ay - py2, az - pz2);   // (q - x) per axis, as knn.hip
            const g4d_f32x2 db = dist2<FM>(bx - px2, by - py2, bz - pz2);
            const int ui = base + u;
            mgn_consider(__float_as_uint(da.x), ui, best[0], bi[0]);
            mgn_consider(__float_as_uint(da.y), ui, best[1], bi[1]);
            mgn_consider(__float_as_uint(db.x), ui, best[2], bi[2]);
            mgn_consider(__float_as_uint(db.y), ui, best[3], bi[3]);
        }
    }
    // ---- the two blends at the nearest vertex, j ascending, each entry accumulated as acc = fma(w_j, T_j, acc) from 0
#pragma unroll 1
    for (int k = 0; k < kMgnQpt; ++k) {
        const long long qi = q0 + (long long)k * kMgnThreads;
        if (qi >= nq) continue;
        const long long f = (long long)c * T + qi / vg;                 // global frame
        const size_t o = (size_t)c * nq + qi;                           // (f, g) row
        const float *w = W + ((size_t)f * v + bi[k]) * nj;
        const float4 *ia = reinterpret_cast<const float4 *>(inv_A + (size_t)f * nj * 16);
        const float4 *pa = reinterpret_cast<const float4 *>(A + (size_t)f * nj * 16);
        float mi[12], mp[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) mi[e] = 0.f, mp[e] = 0.f;
        for (int j = 0; j < nj; ++j) {
            const float wj = w[j];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float4 a = ia[j * 4 + r], b = pa[j * 4 + r];
                mi[r * 4 + 0] = fmaf(wj, a.x, mi[r * 4 + 0]); mi[r * 4 + 1] = fmaf(wj, a.y, mi[r * 4 + 1]);
                mi[r * 4 + 2] = fmaf(wj, a.z, mi[r * 4 + 2]); mi[r * 4 + 3] = fmaf(wj, a.w, mi[r * 4 + 3]);
                mp[r * 4 + 0] = fmaf(wj, b.x, mp[r * 4 + 0]); mp[r * 4 + 1] = fmaf(wj, b.y, mp[r * 4 + 1]);
                mp[r * 4 + 2] = fmaf(wj, b.z, mp[r * 4 + 2]); mp[r * 4 + 3] = fmaf(wj, b.w, mp[r * 4 + 3]);
            }
        }
        float s[3], p[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)   // M[r] . (x, y, z, 1) = fma(M[r][2], z, fma(M[r][1], y, fma(M[r][0], x, M[r][3])))
            s[r] = fmaf(mi[r * 4 + 2], qz[k], fmaf(mi[r * 4 + 1], qy[k], fmaf(mi[r * 4 + 0], qx[k], mi[r * 4 + 3])));
#pragma unroll
        for (int r = 0; r < 3; ++r)
            p[r] = fmaf(mp[r * 4 + 2], s[2], fmaf(mp[r * 4 + 1], s[1], fmaf(mp[r * 4 + 0], s[0], mp[r * 4 + 3])));
        nn_idx[o] = bi[k];
        nn_dist[o] = __uint_as_float(best[k]);
#pragma unroll
        for (int r = 0; r < 3; ++r) stage1[o * 3 + r] = s[r], posed[o * 3 + r] = p[r];
    }
}

}  // namespace g4d

extern "C" int g4d_mgn_skin_f32(int clips, int frames_per_clip, int vg, int v, int j, const float *garment, const float *root,
                                const float *tpose, const float *W, const float *inv_A, const float *A, int *nn_idx, float *nn_dist,
                                float *stage1, float *posed, g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(clips >= 0 && frames_per_clip >= 0 && vg >= 0 && v >= 0 && j >= 0, "g4d_mgn_skin_f32: negative size");
    if (clips == 0 || frames_per_clip == 0 || vg == 0) return G4D_OK;
    G4D_REQUIRE(v >= 1, "g4d_mgn_skin_f32: no body vertices to search (V = 0)");
    G4D_REQUIRE(j >= 1 && j <= kMgnMaxJ, "g4d_mgn_skin_f32: need 1 <= J <= %d (got %d)", kMgnMaxJ, j);
    G4D_REQUIRE(clips <= 65535, "g4d_mgn_skin_f32: clips <= 65535");
    const long long nq = (long long)frames_per_clip * vg;
    G4D_REQUIRE(nq <= (1ll << 40) && (long long)v * 3 <= (1ll << 40), "g4d_mgn_skin_f32: size out of range");
    G4D_REQUIRE(garment && root && tpose && W && inv_A && A && nn_idx && nn_dist && stage1 && posed, "g4d_mgn_skin_f32: null pointer");
    G4D_REQUIRE(((reinterpret_cast<uintptr_t>(inv_A) | reinterpret_cast<uintptr_t>(A)) & 15) == 0,
                "g4d_mgn_skin_f32: inv_A and A must be 16-byte aligned");
    const long long blocks = (nq + kMgnQueries - 1) / kMgnQueries;
    G4D_REQUIRE(blocks <= 0x7fffffffll, "g4d_mgn_skin_f32: too many queries per clip");
    const dim3 grid((unsigned)blocks, (unsigned)clips);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (knn_shape(distance_contraction()) == 0)
        hipLaunchKernelGGL(mgn_skin_kernel<0>, grid, dim3(kMgnThreads), 0, st, frames_per_clip, vg, v, j, garment, root, tpose, W, inv_A, A,
                           nn_idx, nn_dist, stage1, posed);
    else
        hipLaunchKernelGGL(mgn_skin_kernel<2>, grid, dim3(kMgnThreads), 0, st, frames_per_clip, vg, v, j, garment, root, tpose, W, inv_A, A,
                           nn_idx, nn_dist, stage1, posed);
    return check_launch("g4d_mgn_skin_f32");
}

// Exact nearest point on a triangle mesh (psbody's AabbTree.nearest(..., nearest_part=True) as utils/post_processing.py:145-177 uses it), per
// frame, for every query point: the triangle of smallest squared distance (ties: lowest face index), its closest point, which part of the
// triangle that point lies on, and the surface normal the reference derives from the part.
//
//   mesh_aabb    : a cheap per-frame pre-pass -- the bounding box of every block of 64 consecutive faces (the caller hands the faces in an
//                  order that keeps blocks compact: sorted once per topology by the Morton code of the template centroids).
//   mesh_nearest : one lane per query, one wave per workgroup.  A block of 64 triangles is staged through LDS (one triangle per lane) and
//                  every lane tests all of them; the wave skips a block whose box is farther from EVERY lane's query than that lane's best.
//
// The skip is conservative in fp32, so it never changes a bit of the result: a computed closest point lies within a few ulps of the
// coordinates of its triangle, hence of its block's box; the boxes are padded by 2^-18 of their largest coordinate per axis and a block is
// skipped only when (1 - 2^-18) * gap^2 still exceeds the lane's best.  Whatever is skipped could neither win nor tie.
#include "closest_triangle.h"
#include "g4d_common.h"

namespace g4d {

constexpr int kNBlock = 64;   // triangles per block = lanes per wave

__global__ void __launch_bounds__(256) mesh_aabb_kernel(long long total, int v, int nf, int nblocks, const float *__restrict__ verts_all,
                                                       const int *__restrict__ faces, float *__restrict__ boxes) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const long long f = gid / nblocks;
    const int b = (int)(gid - f * nblocks);
    const float *verts = verts_all + (size_t)f * v * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int end = min(nf, (b + 1) * kNBlock);
    for (int k = b * kNBlock; k < end; ++k)
        for (int c = 0; c < 3; ++c) {
            const float *p = verts + (size_t)faces[(size_t)k * 3 + c] * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pad = fmaxf(fabsf(lo[a]), fabsf(hi[a])) * 3.814697265625e-06f;   // 2^-18
        boxes[gid * 6 + a] = lo[a] - pad;
        boxes[gid * 6 + 3 + a] = hi[a] + pad;
    }
}

__global__ void __launch_bounds__(kNBlock) mesh_nearest_kernel(int p, int v, int nf, int nblocks, int waves_per_frame, int cull,
                                                              const float *__restrict__ points, const float *__restrict__ verts_all,
                                                              const int *__restrict__ faces, const int *__restrict__ face_ids,
                                                              const float *__restrict__ boxes_all, const float *__restrict__ vnormals_all,
                                                              const int *__restrict__ frame_active, float *__restrict__ out_point,
                                                              float *__restrict__ out_dist2, int *__restrict__ out_face, int *__restrict__ out_part,
                                                              float *__restrict__ out_normal, int *__restrict__ visited) {
    __shared__ __attribute__((aligned(16))) float4 tri[kNBlock][3];   // {ax ay az bx} {by bz cx cy} {cz, face id bits, -, -}
    const int lane = threadIdx.x;
    const int f = blockIdx.x / waves_per_frame;
    const int qi = (blockIdx.x - f * waves_per_frame) * kNBlock + lane;
    if (frame_active && frame_active[f] == 0) return;   // wave-uniform: a finished frame is not searched, its outputs are left as they are
    const bool live = qi < p;
    const size_t g = (size_t)f * p + (live ? qi : 0);
    const float qx = points[g * 3], qy = points[g * 3 + 1], qz = points[g * 3 + 2];
    const float *verts = verts_all + (size_t)f * v * 3;
    const float *boxes = boxes_all + (size_t)f * nblocks * 6;
    float best = INFINITY;
    int best_id = 0x7fffffff, best_pos = -1, seen = 0;
    for (int b = 0; b < nblocks; ++b) {
        const float *bx = boxes + (size_t)b * 6;
        const float gx = fmaxf(fmaxf(bx[0] - qx, qx - bx[3]), 0.f), gy = fmaxf(fmaxf(bx[1] - qy, qy - bx[4]), 0.f),
                    gz = fmaxf(fmaxf(bx[2] - qz, qz - bx[5]), 0.f);
        const float gap2 = ((gx * gx + gy * gy) + gz * gz) * 0.999996185302734375f;   // 1 - 2^-18
        const bool want = live && !(cull && gap2 > best);
        if (__builtin_amdgcn_ballot_w64(want) == 0ull) continue;   // wave-uniform
        ++seen;
        const int k = b * kNBlock + lane;
        if (k < nf) {
            const int *t = faces + (size_t)k * 3;
            const float *a = verts + (size_t)t[0] * 3, *bb = verts + (size_t)t[1] * 3, *c = verts + (size_t)t[2] * 3;
            tri[lane][0] = make_float4(a[0], a[1], a[2], bb[0]);
            tri[lane][1] = make_float4(bb[1], bb[2], c[0], c[1]);
            tri[lane][2] = make_float4(c[2], __int_as_float(face_ids[k]), 0.f, 0.f);
        }
        __syncthreads();
        const int cnt = min(kNBlock, nf - b * kNBlock);
        for (int j = 0; j < cnt; ++j) {
            const float4 t0 = tri[j][0], t1 = tri[j][1], t2 = tri[j][2];
            const Closest o = closest_on_triangle(qx, qy, qz, t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x);
            const int id = __float_as_int(t2.y);
            const bool better = o.d2 < best || (o.d2 == best && id < best_id);   // a NaN distance (zero-area triangle) never wins
            best = better ? o.d2 : best;
            best_id = better ? id : best_id;
            best_pos = better ? b * kNBlock + j : best_pos;
        }
        __syncthreads();
    }
    if (visited && lane == 0) visited[blockIdx.x] = seen;
    if (!live) return;
    if (best_pos < 0) {   // every triangle degenerate: nothing to report
        out_point[g * 3] = out_point[g * 3 + 1] = out_point[g * 3 + 2] = NAN;
        out_dist2[g] = INFINITY; out_face[g] = -1; out_part[g] = -1;
        out_normal[g * 3] = out_normal[g * 3 + 1] = out_normal[g * 3 + 2] = 0.f;
        return;
    }
    const int *t = faces + (size_t)best_pos * 3;
    const int ia = t[0], ib = t[1], ic = t[2];
    const float *a = verts + (size_t)ia * 3, *bb = verts + (size_t)ib * 3, *c = verts + (size_t)ic * 3;
    const Closest o = closest_on_triangle(qx, qy, qz, a[0], a[1], a[2], bb[0], bb[1], bb[2], c[0], c[1], c[2]);
    float nx, ny, nz;
    if (o.part == 0) {
        const float abx = bb[0] - a[0], aby = bb[1] - a[1], abz = bb[2] - a[2], acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
        const float cxn = aby * acz - abz * acy, cyn = abz * acx - abx * acz, czn = abx * acy - aby * acx;
        const float len = sqrtf((cxn * cxn + cyn * cyn) + czn * czn);
        const bool ok = len > 0.f;
        nx = ok ? cxn / len : 0.f; ny = ok ? cyn / len : 0.f; nz = ok ? czn / len : 0.f;
    } else {
        const float *vn = vnormals_all + (size_t)f * v * 3;
        if (o.part >= 4) {   // vertex a / b / c
            const float *n0 = vn + (size_t)(o.part == 4 ? ia : o.part == 5 ? ib : ic) * 3;
            nx = n0[0]; ny = n0[1]; nz = n0[2];
        } else {             // edge ab / bc / ca: first end + second end
            const float *n0 = vn + (size_t)(o.part == 1 ? ia : o.part == 2 ? ib : ic) * 3;
            const float *n1 = vn + (size_t)(o.part == 1 ? ib : o.part == 2 ? ic : ia) * 3;
            nx = n0[0] + n1[0]; ny = n0[1] + n1[1]; nz = n0[2] + n1[2];
        }
    }
    const float nn = sqrtf((nx * nx + ny * ny) + nz * nz) + 1.e-10f;
    out_point[g * 3] = o.x; out_point[g * 3 + 1] = o.y; out_point[g * 3 + 2] = o.z;
    out_dist2[g] = o.d2; out_face[g] = best_id; out_part[g] = o.part;
    out_normal[g * 3] = nx / nn; out_normal[g * 3 + 1] = ny / nn; out_normal[g * 3 + 2] = nz / nn;
}

}  // namespace g4d

using namespace g4d;

extern "C" int g4d_mesh_aabb_f32(int frames, int v, int nf, const float *verts, const int *faces, float *boxes, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && v >= 0 && nf >= 0, "g4d_mesh_aabb_f32: negative size");
    const int nblocks = (nf + kNBlock - 1) / kNBlock;
    const long long total = (long long)frames * nblocks;
    if (total == 0) return G4D_OK;
    G4D_REQUIRE(v > 0 && verts && faces && boxes, "g4d_mesh_aabb_f32: null pointer (or faces without vertices)");
    G4D_REQUIRE((total + 255) / 256 < (1ll << 31), "g4d_mesh_aabb_f32: too large");
    hipLaunchKernelGGL(mesh_aabb_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), total, v, nf, nblocks,
                       verts, faces, boxes);
    return check_launch("g4d_mesh_aabb_f32");
}

extern "C" int g4d_mesh_nearest_f32(int frames, int p, int v, int nf, int cull, const float *points, const float *verts, const int *faces,
                                    const int *face_ids, const float *boxes, const float *vnormals, const int *frame_active, float *point, float *dist2,
                                    int *face, int *part, float *normal, int *visited, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && p >= 0 && v >= 0 && nf >= 0, "g4d_mesh_nearest_f32: negative size");
    if (frames == 0 || p == 0) return G4D_OK;
    G4D_REQUIRE(v > 0 && nf > 0, "g4d_mesh_nearest_f32: empty mesh (v=%d, nf=%d)", v, nf);
    G4D_REQUIRE(points && verts && faces && face_ids && boxes && vnormals && point && dist2 && face && part && normal,
                "g4d_mesh_nearest_f32: null pointer");
    const int waves = (p + kNBlock - 1) / kNBlock;
    G4D_REQUIRE((long long)frames * waves < (1ll << 31), "g4d_mesh_nearest_f32: too large");
    hipLaunchKernelGGL(mesh_nearest_kernel, dim3((unsigned)(frames * waves)), dim3(kNBlock), 0, reinterpret_cast<hipStream_t>(stream), p, v, nf,
                       (nf + kNBlock - 1) / kNBlock, waves, cull, points, verts, faces, face_ids, boxes, vnormals, frame_active, point, dist2,
                       face, part, normal, visited);
    return check_launch("g4d_mesh_nearest_f32");
}

// The closest point of a triangle to a query, shared by the search (mesh_nearest.hip) and by the point-to-surface loss (fit/fit.hip), which
// recomputes it on the face the search reported and must arrive at the same bits: one routine, one operation order.
#pragma once
#include "g4d_common.h"

namespace g4d {

struct Closest {
    float x, y, z, d2;
    int part;
    float v, w;   // the barycentric weights of corners b and c (the search does not read them)
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

// The closest point of triangle (a, b, c) to q -- include/g4d.h (g4d_mesh_nearest_f32) states this operation order; the float32 mode of
// tests/postprocess_twin.py follows it.
__device__ __forceinline__ Closest closest_on_triangle(float qx, float qy, float qz, float ax, float ay, float az, float bx, float by, float bz,
                                                       float cx, float cy, float cz) {
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float d1 = dot3(abx, aby, abz, qx - ax, qy - ay, qz - az), d2 = dot3(acx, acy, acz, qx - ax, qy - ay, qz - az);
    const float d3 = dot3(abx, aby, abz, qx - bx, qy - by, qz - bz), d4 = dot3(acx, acy, acz, qx - bx, qy - by, qz - bz);
    const float d5 = dot3(abx, aby, abz, qx - cx, qy - cy, qz - cz), d6 = dot3(acx, acy, acz, qx - cx, qy - cy, qz - cz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const int part = (d1 <= 0.f && d2 <= 0.f)                  ? 4
                     : (d3 >= 0.f && d4 <= d3)                 ? 5
                     : (vc <= 0.f && d1 >= 0.f && d3 <= 0.f)   ? 1
                     : (d6 >= 0.f && d5 <= d6)                 ? 6
                     : (vb <= 0.f && d2 >= 0.f && d6 <= 0.f)   ? 3
                     : (va <= 0.f && e43 >= 0.f && e56 >= 0.f) ? 2
                                                               : 0;
    const float den = part == 0 ? (va + vb) + vc : part == 1 ? d1 - d3 : part == 2 ? e43 + e56 : part == 3 ? d2 - d6 : 1.f;
    const float r = 1.f / den;
    const float w = part == 0 ? vc * r : part == 2 ? e43 * r : part == 3 ? d2 * r : part == 6 ? 1.f : 0.f;
    const float v = part == 0 ? vb * r : part == 1 ? d1 * r : part == 2 ? 1.f - w : part == 5 ? 1.f : 0.f;
    Closest o;
    o.x = (ax + abx * v) + acx * w; o.y = (ay + aby * v) + acy * w; o.z = (az + abz * v) + acz * w;
    const float dx = qx - o.x, dy = qy - o.y, dz = qz - o.z;
    o.d2 = (dx * dx + dy * dy) + dz * dz;
    o.part = part;
    o.v = v; o.w = w;
    return o;
}

}  // namespace g4d

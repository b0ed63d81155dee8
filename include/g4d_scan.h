/*
 * g4d_scan.h -- C ABI of libg4d_scan.so: virtual depth-sensor scans.  Rasterized meshes seen from one or several cameras (the outputs of
 * g4d_render_project_f32 and g4d_render_raster, include/g4d_render.h) become fixed-size, labelled world-space point clouds: every point is
 * the exact unprojection of a sample some camera sees, so the cloud is one-sided, self-occluded and as dense as the sensor is -- the input a
 * depth camera or LiDAR delivers, in the form of the data loader's `pcd_torch` / `pcd_label_torch` (utils/dataloader.py:215-230, 279).
 *
 * Data generation, not part of the model's ABI: a third (header, library) pair after g4d.h and g4d_render.h.  The library links against
 * libg4d_hip.so and the boundary contract of g4d.h holds unchanged (raw device pointers + sizes + a HIP stream, status codes, ONE error state:
 * g4d_last_error()).  Every kernel is enqueued on `stream`; none synchronises, allocates or uses an atomic; all scratch comes through
 * g4d_scan_ws_bytes, so a call can be captured in a hipGraph.  The results depend on the inputs alone -- not on the chunk size, not on the
 * order in which workgroups run: two runs give the same bits.  Integer work is exact (64-bit where products need it); every fp32 expression
 * below is written with its order: one rounded operation per sign, nothing fused (-ffp-contract=off); division is the correctly rounded one.
 */
#ifndef G4D_SCAN_H
#define G4D_SCAN_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits: 1 <= cams <= G4D_SCAN_MAX_CAMS; w, h <= G4D_SCAN_MAX_SIDE rays (every edge function below then fits int64 with room to spare:
 * coordinates are used while |x|, |y| < 2^22, a sample centre is < 2^23, so |E| < 2^49); cams * h * w < 2^31. */
#define G4D_SCAN_MAX_CAMS 8
#define G4D_SCAN_MAX_SIDE 32768

/* Samples per workgroup of the counting and the selecting launch: a measurement / test aid ("one chunk plus one"). */
int g4d_scan_chunk(void);

/* Bytes of device scratch g4d_scan_points_f32 needs: two int32 per (frame, chunk of g4d_scan_chunk() samples), that is
 * 8 * frames * ceil(cams * h * w / g4d_scan_chunk()).  0 for an empty problem; (size_t)-1 for a negative size or cams * h * w >= 2^31. */
size_t g4d_scan_ws_bytes(int frames, int cams, int w, int h);

/* ---- scan -----------------------------------------------------------------------------------------------------------------------------------
 * K = cams cameras, F = frames, a sensor of w x h rays, ONE sample per ray (the rasterizer's ss == 1).  Per camera c, as g4d_render.h defines
 * them: px, py (K,F,V) int32 and invz (K,F,V) from g4d_render_project_f32, face_id (K,F,h,w) int32 from g4d_render_raster.  verts (F,V,3):
 * the WORLD-space vertices that were projected.  faces (nf,3) int32, shared by the frames.  face_labels (nf) int32 or NULL.
 *
 * Hits.  Sample s = (c * h + i) * w + j (camera c, row i, column j) of frame f is a hit iff face_id[c,f,i,j] is in [0, nf).  The hits of a
 * frame are ranked in ascending s -- by camera, then row, then column --: M_f of them, ranks r in [0, M_f).
 *
 * Selection of exactly N = n_points points per frame, in 64-bit integers (M = M_f):
 *   mix(x) = { x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16 }          (uint32, products modulo 2^32)
 *   key(seed, f, j) = mix(mix(mix(seed) ^ f) ^ j)
 *   M >= N:      stratified, without replacement: stratum j covers the ranks [lo_j, hi_j), lo_j = floor(j * M / N), hi_j = floor((j + 1) * M / N);
 *                point j is the hit of rank lo_j + key(seed, f, j) mod (hi_j - lo_j).  The picks are distinct and ascending.
 *   0 < M < N:   point j is the hit of rank j mod M: all of them, then more of the same; every hit appears floor(N / M) or ceil(N / M) times.
 *   M == 0:      the frame's points are (0, 0, 0) and its labels, face and sample are -1.
 * Per hit (what the kernel evaluates; the same rule): for M >= N the hit of rank r lies in stratum j = floor(((r + 1) * N - 1) / M) and is
 * selected iff that stratum's pick equals r; for M < N it owns the points r, r + M, r + 2 M, ... < N.
 *
 * Unprojection of a selected hit, sample (c, i, j), face g = face_id[c,f,i,j] = (i0, i1, i2), with camera c's px, py, invz of frame f:
 *   the face is oriented as g4d_render_raster orients it: area2 = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0) (int64); area2 < 0 -> vertices
 *   1 and 2 change places and area2 = -area2.  At the sample centre s = (256 j + 128, 256 i + 128), exactly as that header defines them:
 *   edge k runs p -> q with (p, q) = (v1, v2), (v2, v0), (v0, v1);   E_k = (q.x - p.x) * (s.y - p.y) - (q.y - p.y) * (s.x - p.x)     (int64)
 * then in fp32 ((float) of an int64 rounds to nearest even; iz_k: invz, v_k: the WORLD-space position of oriented vertex k):
 *   b_k = (float)E_k / (float)area2   for k = 0, 1, 2;    w_k = b_k * iz_k
 *   iz = (iz0 + b1 * (iz1 - iz0)) + b2 * (iz2 - iz0)
 *   p.x = ((w0 * v0.x + w1 * v1.x) + w2 * v2.x) / iz,   likewise p.y and p.z
 * -- the rasterizer's perspective-correct vert_rgb rule applied to positions: up to rounding the point is a convex combination of its
 * face's vertices, and it projects back onto its sample centre up to the snapping of the vertices (half a unit of 1/256 sample).
 * A face g4d_render_raster DROPS (a vertex index outside [0, v), an invz not in (0, inf), a |px| or |py| >= 2^22, area2 == 0) cannot occur
 * in its face_id.  If one is handed in all the same it still counts as a hit for the ranks, but its vertices are never read through: a
 * point it is selected for is written as a miss, (0, 0, 0) with label, face and sample -1.
 *
 * Outputs: points (F,N,3); labels (F,N) int32 = face_labels[g], or 0 when face_labels is NULL; face (F,N) int32 = g; sample (F,N) int32 =
 * the s above, so camera = s / (h * w); count (F) int32 = M_f.  Point order is scan order: camera, row, column.
 * ws: g4d_scan_ws_bytes(frames, cams, w, h) bytes, 16-byte aligned; ws_bytes: what the caller allocated (less: G4D_EINVAL).
 * Three launches: count the hits per chunk (ballot + popcount), scan the chunk counts of a frame into offsets, select + unproject.
 * Errors (G4D_EINVAL before any launch): a negative size, cams outside [1, G4D_SCAN_MAX_CAMS], w or h > G4D_SCAN_MAX_SIDE,
 * cams * h * w >= 2^31, a null pointer (face_labels may be NULL), a short or misaligned workspace.
 * frames, w, h or n_points == 0 ... an empty problem: returns 0 and writes nothing.  v == 0 or nf == 0 is no empty problem: every sample is
 * a miss or dropped, and the outputs are written as such. */
int g4d_scan_points_f32(int frames, int cams, int v, int nf, int w, int h, const int *px, const int *py, const float *invz, const int *face_id,
                        const float *verts, const int *faces, const int *face_labels, int n_points, unsigned seed, void *ws, size_t ws_bytes,
                        float *points, int *labels, int *face, int *sample, int *count, g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_SCAN_H */

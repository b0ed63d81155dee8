/*
 * g4d_fit.h -- C ABI of libg4d_fit.so: the distance of a point cloud to a triangle mesh and its gradient.  For every point of a scan the
 * squared distance to the nearest face of a predicted mesh (the face g4d_mesh_nearest_f32 of g4d.h reports), truncated, weighted and summed
 * into one loss; the adjoint of that loss with respect to the mesh vertices and to the points.  One direction only, points -> surface: a
 * one-sided scan says nothing about the surface it did not see.
 *
 * A fourth (header, library) pair after g4d.h, g4d_render.h and g4d_scan.h.  The library links against libg4d_hip.so and the boundary
 * contract of g4d.h holds unchanged (raw device pointers + sizes + a HIP stream, status codes, ONE error state: g4d_last_error()).  Every
 * kernel is enqueued on `stream`; none synchronises, allocates, reads anything back to the host or uses an atomic, so the calls can be captured in
 * a hipGraph.  Every sum below is taken in an order fixed by the shapes and the indices: two runs give the same bits.  All fp32; every
 * expression is written with its order, one rounded operation per sign, nothing fused (-ffp-contract=off) except the dot products g4d.h names;
 * division is the correctly rounded one.
 */
#ifndef G4D_FIT_H
#define G4D_FIT_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The domain of the grouping and of the gradient: a sort key holds a face in 17 bits and a point index in 15. */
#define G4D_FIT_MAX_POINTS 32768
#define G4D_FIT_MAX_FACES 131072
/* Lanes per frame of g4d_fit_point_face_f32: part of the summation order below. */
#define G4D_FIT_LANES 1024

/* ---- forward ---------------------------------------------------------------------------------------------------------------------------------
 * F = frames, P = p points per frame, points (F,P,3), verts (F,v,3), faces (nf,3) int32 in the CALLER'S OWN order (the order whose indices
 * `face` holds), face (F,P) int32 = the nearest face of every point as g4d_mesh_nearest_f32 reports it, weights (F,P) >= 0 or NULL (every
 * weight 1), tau2 = the squared truncation distance (+inf: none).
 *
 * Per point i of frame f, with g = face[f,i], wt = its weight and (a, b, c) = the corners of face g in frame f:
 *   usable = 0 <= g < nf and the three vertex indices of face g lie in [0, v)
 *   usable:      (v, w, point, dist2) exactly as g4d.h states them for g4d_mesh_nearest_f32 (the same fmaf dot products, region
 *                classification, r, v, w, point, dist2: dist2 has the search's bits);  u = (1 - v) - w;
 *                bary[f,i] = (u, v, w);   resid[f,i] = q - point;   dist2[f,i] = dist2
 *   not usable:  bary[f,i] = resid[f,i] = (0, 0, 0);   dist2[f,i] = +inf
 *   inlier[f,i] = 1 iff usable and wt > 0 and dist2 < tau2 (strict: a NaN distance or weight is never an inlier), else 0
 *
 * Per frame, lane t in [0, G4D_FIT_LANES) adds the terms of its points i = t, t + G4D_FIT_LANES, ... in ascending i, starting from 0:
 *   S += wt * dist2 (inliers),   Win += wt (inliers),   Wall += wt (EVERY point),   n += 1 (inliers)
 * and the lanes' partial sums meet by the fixed tree of the mesh kernels: within each run of 64 consecutive lanes a xor butterfly with strides
 * 32, 16, 8, 4, 2, 1 (x <- x + x of lane ^ stride), then the 16 runs left to right.  sums[f] = (S, Win, Wall); count[f] = n (int32).
 * Over the frames, in ascending f from 0:  W = sum Wall_f,  T = sum S_f;   total = (W, loss),  loss = T / W  if W > 0, else 0.
 * W counts every point, not only the inliers: truncating more never rescales the rest.
 *
 * Outputs: bary (F,P,3), resid (F,P,3), dist2 (F,P), inlier (F,P) int32, sums (F,3), count (F) int32, total (2).  Two launches.
 * Errors (G4D_EINVAL before any launch): a negative size, a null pointer (weights may be NULL), nf or v == 0 with points to compare.
 * frames == 0 or p == 0 ... an empty problem: returns 0 and writes nothing. */
int g4d_fit_point_face_f32(int frames, int p, int v, int nf, const float *points, const float *verts, const int *faces, const int *face,
                           const float *weights, float tau2, float *bary, float *resid, float *dist2, int *inlier, float *sums, int *count,
                           float *total, g4d_stream_t stream);

/* ---- grouping --------------------------------------------------------------------------------------------------------------------------------
 * The inliers of each frame ordered by (face ascending, point index ascending).  key(i) = face[f,i] << 15 | i (uint32) if inlier[f,i] != 0 and
 * 0 <= face[f,i] < nf, else 0xFFFFFFFF;  keys[f] (P) uint32 = the keys of frame f in ascending order, so the first count[f] entries are the
 * inliers and the rest is 0xFFFFFFFF.  (The one inlier key that equals 0xFFFFFFFF -- face 131071, point 32767 -- sorts among the fill; the
 * gradient tells it apart by count[f].)  One workgroup per frame sorts the keys in LDS: a bitonic network over the next power of two >= P.
 * g4d_fit_group_lds_bytes(p) = the LDS that takes, 4 * max(64, that power of two); (size_t)-1 outside the domain.
 * Errors (G4D_EINVAL before any launch): a negative size, p > G4D_FIT_MAX_POINTS, nf > G4D_FIT_MAX_FACES, a null pointer.
 * frames == 0 or p == 0: returns 0 and writes nothing. */
size_t g4d_fit_group_lds_bytes(int p);
int g4d_fit_group_f32(int frames, int p, int nf, const int *face, const int *inlier, unsigned *keys, g4d_stream_t stream);

/* ---- gradient --------------------------------------------------------------------------------------------------------------------------------
 * With grad_out (1) = the incoming gradient of the loss and total, count, bary, resid, inlier, weights as above, all in DEVICE memory:
 *   gs = (-2 * grad_out) / W,   gp = (2 * grad_out) / W   if W > 0, else both 0                                       (W = total[0])
 * grad_verts (F,v,3), one thread per (frame, vertex): the vertex's incidence entries e = face * 3 + corner are walked in the order of the
 * (vc_rowptr (v + 1), vc_corners) CSR -- ascending --; the run of each face in keys[f, 0 .. count[f]) is found by bisection and walked in
 * ascending position, that is in ascending point index i:
 *   acc.k = acc.k + ((gs * wt_i) * bary[f,i][corner]) * resid[f,i].k          k = x, y, z, starting from 0
 * Every vertex is written; one without faces, or whose faces hold no inlier, gets 0.
 * grad_points (F,P,3) or NULL:  ((gp * wt_i) * resid[f,i].k) for inliers, 0 otherwise.
 * By the envelope theorem this is the exact gradient of the loss with the nearest face held fixed: d dist2 / d corner = -2 bary (q - point)
 * and d dist2 / d q = 2 (q - point) in every region of the triangle.
 * Errors (G4D_EINVAL before any launch): a negative size, p > G4D_FIT_MAX_POINTS, nf > G4D_FIT_MAX_FACES, a null pointer (weights and
 * grad_points may be NULL).  frames == 0, or v == 0 and no grad_points: returns 0 and writes nothing. */
int g4d_fit_vertex_grad_f32(int frames, int p, int v, int nf, const float *bary, const float *resid, const int *inlier, const float *weights,
                            const unsigned *keys, const int *count, const float *total, const float *grad_out, const int *vc_rowptr,
                            const int *vc_corners, float *grad_verts, float *grad_points, g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_FIT_H */

/*
 * g4d_depth.h -- C ABI of libg4d_depth.so: the projective ray-depth loss of a triangle mesh against depth images, and its gradient to the mesh
 * vertices.  A depth sensor delivers one depth per ray of a known camera; the rasterizer (g4d_render.h) says which face of the current estimate
 * each ray sees (projective data association: no nearest-face search); this library intersects the ray with that face's plane, penalises the
 * difference in depth along the ray, truncated, weighted and summed into one loss, and gathers the adjoint of that loss to the vertices with the
 * visible face held fixed.  Nothing here is differentiated through the rasterizer or to the camera.
 *
 * A seventh (header, library) pair after g4d.h, g4d_render.h, g4d_scan.h, g4d_fit.h, g4d_smpl.h and g4d_skin.h.  The library links against
 * libg4d_hip.so and the boundary contract of g4d.h holds unchanged (raw device pointers + sizes + a HIP stream, status codes, ONE error state:
 * g4d_last_error()).  Every kernel is enqueued on `stream`; none synchronises, allocates, reads anything back to the host or uses an atomic; all
 * scratch comes through g4d_depth_ws_bytes, so the calls can be captured in a hipGraph.  Every sum below is taken in an order fixed by the shapes
 * and the indices: two runs give the same bits, and the gradient of a frame does not depend on the frames it is batched with (but for the one
 * shared factor 1 / W).  All fp32; every expression is written with its order, one rounded operation per sign, nothing fused
 * (-ffp-contract=off); division is the correctly rounded one; (float) of an integer below is exact.
 */
#ifndef G4D_DEPTH_H
#define G4D_DEPTH_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits: 1 <= cams <= G4D_DEPTH_MAX_CAMS; w, h <= G4D_RENDER_MAX_SAMPLES of g4d_render.h (4096; tests/test_depth_fit_cpu.py holds the two
 * together); cams * h * w < 2^31; nf <= G4D_DEPTH_MAX_FACES (3 * nf fits an int32). */
#define G4D_DEPTH_MAX_CAMS 8
#define G4D_DEPTH_MAX_SIDE 4096
#define G4D_DEPTH_MAX_FACES 715827882
/* Lanes per workgroup of the forward and samples per lane: part of the summation order below. */
#define G4D_DEPTH_LANES 256
#define G4D_DEPTH_PER_LANE 4

/* Samples per workgroup of the forward, G4D_DEPTH_LANES * G4D_DEPTH_PER_LANE: a measurement / test aid ("one chunk plus one"). */
int g4d_depth_chunk(void);

/* Bytes of device scratch g4d_depth_fit_terms_f32 needs: 16 per (frame, chunk of g4d_depth_chunk() samples), that is
 * 16 * frames * ceil(cams * h * w / g4d_depth_chunk()).  0 for an empty problem; (size_t)-1 for a negative size or cams * h * w >= 2^31. */
size_t g4d_depth_ws_bytes(int frames, int cams, int w, int h);

/* ---- one sample -------------------------------------------------------------------------------------------------------------------------------
 * K = cams cameras, F = frames, a sensor of w x h rays, ONE sample per ray (the rasterizer's ss == 1).  Layout is camera-major as in g4d_scan.h:
 * px, py (K,F,V) int32, invz (K,F,V) and cam (K,F,V,3) from g4d_render_project_f32 at ss = 1, face_id (K,F,h,w) int32 from g4d_render_raster;
 * depth_obs (K,F,h,w) the observed depth image (camera-space z; anything not finite or <= 0 is "no observation", so the rasterizer's +inf
 * background is a miss); weights (K,F,h,w) >= 0 or NULL (every weight 1); labels_obs (K,F,h,w) int32 and face_labels (nf) int32: both NULL or
 * neither; faces (nf,3) int32 in the CALLER'S OWN order, shared by the frames.
 * cams_host (K,10) fp32 in HOST memory, read during the call: per camera the rows (x, y, z) of the look-at basis R as g4d_render_project_f32
 * rounds them to fp32 (9 numbers, row-major), then s = that projection's fp32 1 / tan(half angle).
 * trunc: the truncation of |residual| (+inf: none); grazing: the smallest |cosine| between ray and face normal that is still used.
 *
 * Sample (c, i, j) of frame f, with g = face_id[c,f,i,j], wt = its weight, D = depth_obs[c,f,i,j]:
 *   observed   = D > 0 and D < +inf                                                                          (a NaN compares false)
 *   associated = observed and 0 <= g < nf and the three vertex indices of face g lie in [0, V)
 *                and, with labels, face_labels[g] == labels_obs[c,f,i,j]
 *   ray        hh = 128 h, hw = 128 w (exact);  sh = s * (float)hh;
 *              d.x = (float)(256 j + 128 - hw) / sh;   d.y = (float)(hh - (256 i + 128)) / sh;   d.z = 1
 *   face plane c0, c1, c2 = cam[c,f,faces[g][0 .. 2]] (un-snapped, the caller's order);   e1 = c1 - c0;  e2 = c2 - c0;
 *              n = e1 X e2  with (a X b).x = a.y * b.z - a.z * b.y (and cyclic);
 *              den = (n.x * d.x + n.y * d.y) + n.z;   nn = (n.x * n.x + n.y * n.y) + n.z * n.z;   dd = (d.x * d.x + d.y * d.y) + 1
 *   grazing    facing = den * den > ((grazing * grazing) * nn) * dd                (strict: a zero-area face, a NaN, an edge-on face all fail)
 *   depth      z = ((n.x * c0.x + n.y * c0.y) + n.z * c0.z) / den                   (d.z = 1: the camera-space z where the ray meets the plane)
 *   residual   r = z - D
 *   inlier     = wt > 0 and associated and facing and |r| < trunc                   (strict; a NaN never is an inlier)
 *   hit        q = (z * d.x - c0.x, z * d.y - c0.y, z - c0.z);
 *              b1 = (((q X e2).x * n.x + (q X e2).y * n.y) + (q X e2).z * n.z) / nn;   b2 = likewise from e1 X q;   b0 = (1 - b1) - b2
 * The depth is NOT the rasterizer's 1 / iz (a function of the snapped integer positions, piecewise constant in a vertex's lateral motion): the
 * rasterizer supplies the association only.  b0, b1, b2 may leave [0, 1] by the rasterizer's snapping (half a unit of 1/256 sample).
 *
 * ---- forward ----------------------------------------------------------------------------------------------------------------------------------
 * The samples of frame f in scan order, s = (c * h + i) * w + j, are cut into chunks of g4d_depth_chunk().  Lane t in [0, G4D_DEPTH_LANES) of
 * chunk k adds the terms of its samples s = k * chunk + q * G4D_DEPTH_LANES + t, q = 0 .. G4D_DEPTH_PER_LANE - 1 ascending, starting from 0:
 *   S += wt * (r * r) (inliers),   Win += wt (inliers),   Wobs += wt (OBSERVED samples, associated or not),   n += 1 (inliers)
 * and the lanes' sums meet by the fixed tree of the mesh kernels: within each run of 64 consecutive lanes a xor butterfly with strides
 * 32, 16, 8, 4, 2, 1 (x <- x + x of lane ^ stride), then the 4 runs left to right.  Per frame, lane t of a second workgroup of
 * G4D_DEPTH_LANES lanes adds the chunk sums k = t, t + G4D_DEPTH_LANES, ... ascending from 0 and the lanes meet by the same tree:
 * sums[f] = (S, Win, Wobs), count[f] = n (int32).  Over the frames, ascending f from 0:  W = sum Wobs_f,  T = sum S_f;
 * total = (W, loss),  loss = T / W if W > 0, else 0.  W counts every observed ray: one the estimate misses still weighs in the denominator.
 * resid (K,F,h,w) or NULL: r of every inlier, NaN elsewhere.
 * Three launches.  ws: g4d_depth_ws_bytes(frames, cams, w, h) bytes, 16-byte aligned; ws_bytes: what the caller allocated (less: G4D_EINVAL).
 * Errors (G4D_EINVAL before any launch): a negative size, cams outside [1, 8], w or h > 4096, cams * h * w >= 2^31, nf > G4D_DEPTH_MAX_FACES,
 * one of labels_obs / face_labels without the other, a null pointer (weights, resid, the labels may be NULL; faces and face_labels when
 * nf == 0; cam when v == 0), a short or misaligned workspace.
 * frames, w or h == 0 ... an empty problem: returns 0 and writes nothing.  nf == 0 or v == 0 is none: nothing associates, and sums, count, total
 * and resid are written as such. */
int g4d_depth_fit_terms_f32(int frames, int cams, int v, int nf, int w, int h, const float *cam, const int *faces, const int *face_id,
                            const float *depth_obs, const float *weights, const int *labels_obs, const int *face_labels, const float *cams_host,
                            float trunc, float grazing, void *ws, size_t ws_bytes, float *sums, int *count, float *total, float *resid,
                            g4d_stream_t stream);

/* ---- gradient ---------------------------------------------------------------------------------------------------------------------------------
 * With the visible face held fixed, dz = n . (b0 dc0 + b1 dc1 + b2 dc2) / den exactly (also when the hit lies just outside the triangle), and
 * cam = R_c (v - eye_c).  With grad_out (1) = the incoming gradient of the loss and total as above, both in DEVICE memory:
 *   gs = (2 * grad_out) / W  if W > 0, else 0                                                                              (W = total[0])
 * grad_verts (F,V,3), one lane per (frame, vertex), acc = 0:
 *   for c = 0 .. K - 1:   a = 0 (camera space);
 *     the vertex's incidence entries e = face * 3 + corner in the order of the (vc_rowptr (V + 1), vc_corners) CSR -- ascending --; a face that
 *     g4d_render_raster would drop under camera c (an index outside [0, V), an invz outside (0, inf), a |px| or |py| >= 2^22, area2 == 0) is
 *     skipped; else its sample box of g4d_render.h, [ceil((min x - 128) / 256), floor((max x - 128) / 256)] x [the same in y] from that camera's
 *     px, py, cut to the image, is walked row by row, columns ascending, and every sample whose face_id equals the face and that is an inlier
 *     (all terms recomputed as above) adds
 *         t = (((gs * wt) * r) * b_corner) / den;     a.k = a.k + t * n.k          k = x, y, z
 *     acc.j = acc.j + ((R_c[0][j] * a.x + R_c[1][j] * a.y) + R_c[2][j] * a.z)     j = x, y, z                              (R_c^T a)
 * Every vertex is written; one without faces, or whose faces hold no inlier, gets 0.  One launch, no scratch.
 * Errors (G4D_EINVAL before any launch): as for the forward, and a null px, py, invz, total, grad_out, vc_rowptr, grad_verts (vc_corners when
 * nf > 0).  frames, v, w or h == 0: returns 0 and writes nothing. */
int g4d_depth_fit_vertex_grad_f32(int frames, int cams, int v, int nf, int w, int h, const int *px, const int *py, const float *invz,
                                  const float *cam, const int *faces, const int *face_id, const float *depth_obs, const float *weights,
                                  const int *labels_obs, const int *face_labels, const float *cams_host, float trunc, float grazing,
                                  const float *total, const float *grad_out, const int *vc_rowptr, const int *vc_corners, float *grad_verts,
                                  g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_DEPTH_H */

/*
 * g4d_skin.h -- C ABI of libg4d_skin.so: the adjoint of the garment skinning (garment4d_amd/garment_lbs.py: lbs_garment_interpolation,
 * the reference's modules/mesh_encoder.py:312-410) with respect to the T-pose garment, its first argument.  What fitting the garment to a
 * scan needs: g4d_fit.h gives d loss / d posed garment, this carries it back to the T-pose garment and so to the PCA coefficients.
 *
 * A sixth (header, library) pair after g4d.h, g4d_render.h, g4d_scan.h, g4d_fit.h and g4d_smpl.h.  The library links against libg4d_hip.so and
 * the boundary contract of g4d.h holds unchanged (raw device pointers + sizes + a HIP stream, status codes, ONE error state:
 * g4d_last_error()).  Each entry point is ONE launch on `stream`; neither synchronises, allocates, reads anything back to the host or uses an
 * atomic, so the calls can be captured in a hipGraph.  Every value has one writer and every sum an order fixed by the shapes alone: two runs
 * give the same bits, and a clip's bits do not depend on the clips it is launched with.  Inputs and outputs are fp32.
 *
 * The forward, per clip c with T frames f = c T + t, garment vertex v, body vertex lists idx[c,v,0..K) (ascending distance, constants of the
 * graph as knn_points(...).idx is in the reference) and squared distances d_k = |g_v - body[c, idx_k]|^2:
 *   g     = x + root
 *   r_k   = 1 / d_k with inf -> 0,   s = sum_k r_k,   w_k = r_k / s with inf -> 0            (g4d_knn_blend_weights_f32 of g4d.h)
 *   Wb[f,v,:] = sum_k w_k W[f, idx_k, :]                                                    (one blend over K, one over its min(64, K) prefix)
 *   y[f,v] = T^R v_in[c,v] + T^t,   T = sum_j Wb[f,v,j] A[f,j]  (3 x 4)                     (g4d_lbs_pose_skin_f32 of g4d.h)
 * and, between the K-blend and the second skinning, 100 linear smoothing steps along the garment mesh, whose adjoint is the same kernel
 * (g4d_jacobi_smooth_f32) on the transposed operator.
 *
 * The adjoints here:
 *   skinning   d v_in[c,v]  = sum_t (T_f^R)^T dy[f,v]                      frames ascending, starting from 0
 *              d Wb[f,v,j]  = sum_{r<3} dy[f,v,r] (A[f,j,r,0:3] . v_in[c,v] + A[f,j,r,3])
 *                             (one table per clip: summed over the clip's frames, ascending, starting from 0)
 *   blend      c_k  = sum_t sum_j dWb[f,v,j] W[f, idx_k, j]                frames ascending, then j ascending, fused multiply-adds from 0
 *              dr_k = (c_k - sum_m w_m c_m) / s,   dd_k = -dr_k r_k^2,   d g[c,v] = sum_k 2 dd_k (g_v - body[c, idx_k])
 *              (the distances are differentiated, the choice of neighbours is not)
 * Coincident vertices.  Where d_k = 0 the forward's weight of that neighbour is 0 (1 / 0 = inf -> 0) and the reference's autograd returns NaN
 * for the garment vertex (0 * inf in reciprocal's backward).  Here the contribution of such a neighbour is DEFINED as zero: dd_k = 0 wherever
 * r_k = 0, the other neighbours' terms are as above.
 * Precision.  c_k is an fp32 sum.  Everything after it -- sum_m w_m c_m, dr_k, dd_k with r_k = 1 / d_k formed in float64, the differences
 * g - body[idx_k] and the sum over k -- is float64, rounded to fp32 once: the terms of the near neighbours are large and of mixed sign (in fp32
 * this tail alone missed the gate of the tests on one of eleven shapes).  w_k and s are the forward's own fp32 numbers.
 * Sums over the wave (sum_m w_m c_m and the three components of d g): a lane adds its up to four neighbours k = l, l + 64, l + 128, l + 192 in
 * ascending k, then a xor butterfly over the 64 lanes (strides 32 ... 1).
 */
#ifndef G4D_SKIN_H
#define G4D_SKIN_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The domain: the forward's. */
#define G4D_SKIN_MAX_K 256
#define G4D_SKIN_MAX_JOINTS 64

/* The adjoint of g4d_lbs_pose_skin_f32 in the garment's form: `clips` clips of `frames_per_clip` frames share the input vertices of their clip.
 * W (clips * frames_per_clip, vg, j), or (clips, vg, j) with w_per_clip != 0 (one table for the frames of a clip); A (frames, j, 16): the
 * 4 x 4 transforms, row major; verts (clips, vg, 3); d_out (frames, vg, 3).
 * Outputs, either may be NULL: d_verts (clips, vg, 3) = d_add + the sum above (d_add (clips, vg, 3) or NULL = zero; it may be d_verts itself),
 * d_W in W's shape.  frames_per_clip = T for the posing, 1 for the un-posing.
 * Errors (G4D_EINVAL before any launch): a negative size, frames_per_clip < 1, j outside 1 .. G4D_SKIN_MAX_JOINTS, a null input.
 * clips == 0 or vg == 0 ... an empty problem: nothing is read or written. */
int g4d_garment_skin_grad_f32(int clips, int frames_per_clip, int vg, int j, const float *W, int w_per_clip, const float *A, const float *verts,
                              const float *d_out, const float *d_add, float *d_verts, float *d_W, g4d_stream_t stream);

/* The adjoint of g4d_knn_blend_weights_f32, carried on to the query points.  W (frames, v, j), idx and dists (frames / frames_per_clip, vg, ldk)
 * of which the first k <= ldk entries of a row are used (the K-blend's list with k = min(64, K) is the prefix blend's), d_blend (frames, vg, j)
 * = d loss / d of that call's output, pts (clips, vg, 3) the query points g, ref (clips, v, 3) the body.
 * Output: d_pts (clips, vg, 3) = d_add + d g (d_add (clips, vg, 3) or NULL = zero; it may be d_pts itself).  One wave per (clip, vertex); an
 * index outside 0 .. v - 1 is clamped into it.
 * Errors (G4D_EINVAL before any launch): a negative size, frames_per_clip < 1 or not a divisor of frames, k outside 1 .. G4D_SKIN_MAX_K,
 * ldk < k, j outside 1 .. G4D_SKIN_MAX_JOINTS, v < 1, a null pointer (d_add may be NULL).
 * frames == 0 or vg == 0 ... an empty problem: nothing is read or written. */
int g4d_knn_blend_grad_f32(int frames, int frames_per_clip, int vg, int v, int k, int ldk, int j, const float *W, const int *idx,
                           const float *dists, const float *d_blend, const float *pts, const float *ref, const float *d_add, float *d_pts,
                           g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_SKIN_H */

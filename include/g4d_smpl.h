/*
 * g4d_smpl.h -- C ABI of libg4d_smpl.so: the adjoint of lbs(), SMPL's linear blend skinning -- the gradient of a loss to the pose
 * (axis-angle or rotation matrices) and to the betas, given its gradient to the skinned vertices and to the posed joints.  What registering
 * the body to a scan needs: g4d_fit.h gives d loss / d verts of any mesh, this carries it on to the 72 + 10 numbers of the body.
 *
 * A fifth (header, library) pair after g4d.h, g4d_render.h, g4d_scan.h and g4d_fit.h.  The library links against libg4d_hip.so and the
 * boundary contract of g4d.h holds unchanged (raw device pointers + sizes + a HIP stream, status codes, ONE error state: g4d_last_error()).
 * Every kernel is enqueued on `stream`; none synchronises, allocates, reads anything back to the host or uses an atomic, so the call can be
 * captured in a hipGraph.  Every sum is taken in an order fixed by the shapes alone: two runs give the same bits, and -- but for the one sum
 * over frames named below -- a frame's gradient does not depend on the frames it is launched with.  Inputs, outputs, the slabs and both
 * V-long contractions are fp32.
 *
 * The forward (smplx/smplx/lbs.py:152-248, as g4d_lbs_mfma_f32 of g4d.h computes it from the prepared constants blend_dirs =
 * [shapedirs^T ; posedirs] (NC, 3V), J_template (J,3), J_shapedirs (J,3,NB)), per frame, with R_j the rotation of joint j
 * (pose2rot: Rodrigues of the axis-angle, lbs.py:330-345: angle = ||t + 1e-8||, dir = t / angle, R = I + sin K + (1 - cos) K K):
 *   c       = [betas | R_1 - I, ..., R_{J-1} - I]                 NC = NB + 9 (J - 1) coefficients
 *   v_posed = v_template + c . blend_dirs
 *   Jr      = J_template + J_shapedirs betas
 *   G_0     = [R_0 | Jr_0],   G_j = G_parent(j) [R_j | Jr_j - Jr_parent(j)]          (parents precede their children)
 *   posed_j = G_j^t,          A_j = [G_j^R | G_j^t - G_j^R Jr_j]
 *   T_v     = sum_j W[v,j] A_j,       verts_v = T_v^R v_posed_v + T_v^t
 * Nothing of it is stored: R, Jr, G, A, v_posed and T are recomputed here from pose, betas and the constants.
 *
 * The adjoint, with g_v = d L / d verts (B,V,3) and g_p = d L / d posed_joints (B,J,3), either NULL = zero:
 *   dA_j (3x4)  = sum_v W[v,j] g_v (x) [v_posed_v ; 1]            d v_posed_v = (T_v^R)^T g_v
 *   dc          = blend_dirs . d v_posed                          (a 3V-long contraction per frame and coefficient)
 *   dG_j^R      = dA_j^R - dA_j^t (x) Jr_j,    dG_j^t = dA_j^t + g_p_j,    dJr_j = -(G_j^R)^T dA_j^t
 *   for j = J-1 .. 1, p = parent(j):   dL_j = (G_p^R)^T dG_j  (3x4: rotation part dL_j^R, translation part dt_j);
 *                                      dG_p += dG_j L_j^T  (dG_p^R += dG_j^R R_j^T + dG_j^t (x) (Jr_j - Jr_p);  dG_p^t += dG_j^t);
 *                                      dJr_j += dt_j,  dJr_p -= dt_j
 *   dL_0 = dG_0:  dJr_0 += dG_0^t
 *   dR_j        = dL_j^R + (dc)[NB + 9 (j-1) ...]   (j >= 1; dR_0 = dL_0^R)
 *   d betas     = (dc)[:NB] + J_shapedirs^T dJr
 *   pose2rot:   d pose_j = the adjoint of the Rodrigues formula above, term by term (finite at pose = 0: what autograd of the reference gives)
 *   otherwise:  d pose = dR (B,J,3,3)
 *
 * Layout and summation order.  The vertices are cut into runs of G4D_SMPL_SLAB_VERTS; one workgroup walks a run in tiles of 32 vertices
 * (their blend rows staged in LDS once per tile), rebuilds v_posed and T on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, k ascending), forms
 * d v_posed in registers and contracts over its vertices -- also on the matrix cores, one accumulator per output element, vertices in the
 * order (tile, 16-vertex half, r = 0..3, then within an instruction the four vertices 4 q + r, q = 0..3) -- into a partial dA (B,J,12) and a
 * partial dc (B,NC): one slab of the workspace per run.  Within a slab the products of a 16-vertex half are summed on their own, from zero, and
 * that sum is added to the slab's running sum.  The slabs are then added in ascending order, starting from 0, in float64 and rounded to fp32
 * once; a per-frame kernel (one wave per frame) runs the rigid part again and the chain, joint and Rodrigues adjoints, all in float64 -- the
 * sums along the kinematic chain are where fp32 would lose most -- and rounds its outputs to fp32.  d betas with betas_bstride == 0 (one row
 * of betas for all frames) is the fp32 sum of the frames' fp32 rows in ascending frame order, starting from 0: the one output that depends on
 * the batch.
 */
#ifndef G4D_SMPL_H
#define G4D_SMPL_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The domain, the forward's: J <= 32 joints and NB + 9 (J - 1) <= 224 blend coefficients. */
#define G4D_SMPL_MAX_JOINTS 32
#define G4D_SMPL_MAX_COEFFS 224
/* Vertices per slab of partial sums: part of the summation order. */
#define G4D_SMPL_SLAB_VERTS 128

/* 1 iff (j, nb) lies in the domain. */
int g4d_smpl_grad_supported(int j, int nb);
/* The number of slabs: ceil(v / G4D_SMPL_SLAB_VERTS) for b > 0 and v > 0, else 0 -- a function of (b, v) alone; -1 for a negative size. */
int g4d_smpl_grad_slabs(int b, int v);
/* The bytes of workspace g4d_smpl_lbs_grad_f32 needs (the matrix operands of the recomputed forward, the slabs, their sum, the frames' d betas
 * rows);
 * -1 outside the domain or for a negative size. */
long long g4d_smpl_grad_ws_bytes(int b, int v, int j, int nb);

/* d_pose (B,J,3) if pose2rot else (B,J,3,3), d_betas (B,NB) if betas_bstride == NB, (NB) if betas_bstride == 0.  betas, pose, the constants
 * and parents (J) int32 exactly as g4d_lbs_mfma_f32 takes them; d_verts (B,V,3) or NULL, d_joints (B,J,3) or NULL; ws: g4d_smpl_grad_ws_bytes
 * bytes of device memory, 16-byte aligned, owned by the caller, contents undefined before and after.  Four launches (five with
 * betas_bstride == 0).
 * Errors (G4D_EINVAL before any launch): a negative size, (j, nb) outside the domain, betas_bstride neither 0 nor nb, a null pointer (d_verts
 * and d_joints may be NULL), a workspace too small or misaligned.
 * b == 0 or v == 0 ... an empty problem: every output given (non-NULL) is set to zero, nothing else is read. */
int g4d_smpl_lbs_grad_f32(int b, int v, int j, int nb, int pose2rot, const float *betas, int betas_bstride, const float *pose,
                          const float *v_template, const float *blend_dirs, const float *J_template, const float *J_shapedirs,
                          const int *parents, const float *lbs_weights, const float *d_verts, const float *d_joints, float *d_pose,
                          float *d_betas, void *ws, long long ws_bytes, g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_SMPL_H */

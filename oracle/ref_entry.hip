/* oracle/ref_entry.hip -- C entry points of the reference build (oracle/_ref/libpointnet2_ref.so, `make -C oracle ref`).
 *
 * TEST INFRASTRUCTURE ONLY.  One extern "C" function per op of the reference's `pointnet2_cuda` extension, taking raw device
 * pointers and a stream; each only forwards to the launcher that the reference's own kernel file defines.  The operand order is
 * the one the reference's C++ wrappers pass (sampling.cpp, ball_query.cpp, group_points.cpp, interpolate.cpp).
 * ball_query.cpp passes the query centres (new_xyz) FIRST and the cloud (xyz) second, although the header names the launcher's
 * parameters the other way round; the kernel file's own definition takes (new_xyz, xyz).  Forwarded here as the wrapper does.
 *
 * The launchers are declared by the reference's headers, found through -I$(G4D_REFERENCE_DIR)/...; nothing of them is copied.
 */
#include "ball_query_gpu.h"
#include "cuda_utils.h"
#include "group_points_gpu.h"
#include "interpolate_gpu.h"
#include "sampling_gpu.h"

#define G4D_REF_API extern "C" __attribute__((visibility("default")))

/* the block size furthest_point_sampling_kernel_launcher picks for a cloud of n points (host only) */
G4D_REF_API int g4d_ref_opt_n_threads(int work_size) { return opt_n_threads(work_size); }

G4D_REF_API void g4d_ref_fps(int b, int n, int m, const float *points, float *temp, int *idx, void *stream) {
    furthest_point_sampling_kernel_launcher(b, n, m, points, temp, idx, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_gather(int b, int c, int n, int npoints, const float *points, const int *idx, float *out, void *stream) {
    gather_points_kernel_launcher_fast(b, c, n, npoints, points, idx, out, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_gather_grad(int b, int c, int n, int npoints, const float *grad_out, const int *idx, float *grad_points,
                                     void *stream) {
    gather_points_grad_kernel_launcher_fast(b, c, n, npoints, grad_out, idx, grad_points, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx,
                                    void *stream) {
    ball_query_kernel_launcher_fast(b, n, m, radius, nsample, new_xyz, xyz, idx, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_group(int b, int c, int n, int npoints, int nsample, const float *points, const int *idx, float *out,
                               void *stream) {
    group_points_kernel_launcher_fast(b, c, n, npoints, nsample, points, idx, out, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_group_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                                    float *grad_points, void *stream) {
    group_points_grad_kernel_launcher_fast(b, c, n, npoints, nsample, grad_out, idx, grad_points, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, void *stream) {
    three_nn_kernel_launcher_fast(b, n, m, unknown, known, dist2, idx, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_three_interp(int b, int c, int m, int n, const float *points, const int *idx, const float *weight, float *out,
                                      void *stream) {
    three_interpolate_kernel_launcher_fast(b, c, m, n, points, idx, weight, out, (cudaStream_t)stream);
}

G4D_REF_API void g4d_ref_three_interp_grad(int b, int c, int n, int m, const float *grad_out, const int *idx, const float *weight,
                                           float *grad_points, void *stream) {
    three_interpolate_grad_kernel_launcher_fast(b, c, n, m, grad_out, idx, weight, grad_points, (cudaStream_t)stream);
}

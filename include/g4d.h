/*
 * g4d.h -- C ABI of libg4d_hip.so: the MI355X (gfx950) implementation of Garment4D's point-cloud
 * encoder + skinning hot path.
 *
 * Boundary contract:
 *   - plain C, raw DEVICE pointers + sizes + a HIP stream; no torch / ATen types;
 *   - the caller allocates every output and pre-initialises what the reference's callers
 *     pre-initialise (noted per function); kernels are enqueued on `stream`, never synchronise,
 *     never allocate, keep no global state (except the process-wide numerics mode below) -> safe from several host threads
 *     on different streams;
 *   - every entry point returns 0 on success or a non-zero hipError_t / G4D_E* code; it NEVER
 *     calls exit() (the reference's launchers do: e.g. sampling_gpu.cu:248-252).
 *     g4d_last_error() returns a thread-local message for the last failure.
 *   - all tensors are contiguous; fp32 data, int32 indices (as the reference: §2a).
 *
 * Each legacy entry point replaces one `*_kernel_launcher*` of the reference
 * (modules/pointnet2/pointnet2/src/, cited per function) -- the raw-pointer seam
 * that the reference's pybind wrappers (src/pointnet2_api.cpp:10-24) already call.
 */
#ifndef G4D_H
#define G4D_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t *g4d_stream_t; /* == hipStream_t */

#define G4D_OK 0
#define G4D_EINVAL 10001 /* bad argument (negative size, null pointer, unsupported width) */

int g4d_version(void); /* 100 * major + minor: 200 = round 2 (the `boxes` scratch of g4d_ball_query_boxes_f32 grew to 16-point sub-blocks); 205 / 206 = round 5 (entry points added, none changed; 206: g4d_gcn_tile_meta_*, g4d_gcn_agg_linear_meta_f32); 260 = round 6 (added: g4d_mlp_run / g4d_mlp_args, g4d_mlp_chain_group_table_ws_f32, g4d_sa_table_ws_bytes, g4d_sa_table_supported; none changed); 261 (entry points added, none changed: g4d_mgn_skin_f32); 262 (entry points added, none changed: g4d_spmm_rows_grad_f32, g4d_col_sum_rows_f32, g4d_gemm_tn_f32 and their size queries); 263 (entry points added, none changed: g4d_pos_encode_grad_f32, g4d_temporal_attention_grad_f32 and their size queries); later additions that change nothing (g4d_mgn_skin_grad_f32, g4d_stage1_*, g4d_bn_*, g4d_pool_rows_max_grad_f32) keep 263 */
const char *g4d_last_error(void);

/* ---- numerics: how the squared distance of FPS / ball query / three_nn / knn is rounded ---------------------------------
 * The reference writes  d = (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1)  (sampling_gpu.cu:136,
 * ball_query_gpu.cu:30, interpolate_gpu.cu:33) and builds with `nvcc -O2` (setup.py:19-20), i.e. with -fmad=true: the
 * compiler contracts the expression into fused multiply-adds.  Which indices come out of FPS (arg-max), ball query (d < r^2)
 * and three_nn (ordering) depends on that rounding wherever two candidates are within an ulp, and one flipped FPS pick
 * changes every later pick.  The mode is process-wide, read when a kernel is launched:
 *   G4D_CONTRACT_NVCC  (default)  fma(dz,dz, fma(dx,dx, dy*dy)) -- the contraction the LLVM/NVVM DAG combiner performs on
 *                                 that expression (left product of the first sum fused, then the third product): matches
 *                                 the reference as built by its own setup.py; knn (chamferdist's accumulate loop) uses
 *                                 fma(dz,dz, fma(dy,dy, dx*dx));
 *   G4D_CONTRACT_OFF              every product and sum rounded separately (a reference built with -fmad=false, and the
 *                                 contract a plain C compiler without contraction reproduces);
 *   G4D_CONTRACT_CHAIN            fma(dz,dz, fma(dy,dy, dx*dx)) for every kernel (the other possible pairing).
 * Environment: G4D_DIST_CONTRACT=nvcc|off|chain sets the initial mode.  The setter returns the previous mode (-1 and an
 * error text for an unknown mode).  Box pruning inside the kernels is exact under every mode (monotone rounding). */
#define G4D_CONTRACT_OFF 0
#define G4D_CONTRACT_NVCC 1
#define G4D_CONTRACT_CHAIN 2
int g4d_get_distance_contraction(void);
int g4d_set_distance_contraction(int mode);
/* Override for the CALLING host thread only (-1 removes it): every launcher called on this thread uses it instead of the process-wide mode.
 * Two host threads driving the library on different streams with different modes do not interfere.  Returns the previous override
 * (-1 = none), -2 on a bad mode.  g4d_get_distance_contraction() reports what the calling thread's launches would use. */
int g4d_set_distance_contraction_thread(int mode);

/* ---- the reference's nine kernels ------------------------------------------------------- */

/* furthest_point_sampling_kernel_launcher (sampling_gpu.h:24-27, sampling_gpu.cu:93-253).
 * xyz (B,N,3); temp (B,N) in/out scratch, caller fills 1e10 (pointnet2_utils.py:26), holds the
 * final min-distances on return; idx (B,M) int32 out.  idx[:,0] = 0.  Tie-break identical to the
 * reference's block-size-dependent tree reduction.  Extension: temp may be NULL when 64 <= N <= 12800 (the
 * register-resident kernels then start from 1e10 themselves and skip the write-back). */
int g4d_fps_f32(int b, int n, int m, const float *xyz, float *temp, int *idx, g4d_stream_t stream);

/* The same sampling with the gather of the selected coordinates fused (pointnet2_modules.py:32-35 calls furthest_point_sample and
 * then gather_operation on xyz): new_xyz (B,m,3) = xyz[b, idx[b,j], :], written by the sampling kernel as each sample is chosen. */
int g4d_fps_gather_f32(int b, int n, int m, const float *xyz, float *temp, int *idx, float *new_xyz, g4d_stream_t stream);

/* gather_points_kernel_launcher_fast (sampling_gpu.h:9-13): out[b,c,j] = points[b,c,idx[b,j]].
 * points (B,C,N), idx (B,M), out (B,C,M). */
int g4d_gather_f32(int b, int c, int n, int m, const float *points, const int *idx, float *out,
                   g4d_stream_t stream);

/* gather_points_grad_kernel_launcher_fast (sampling_gpu.h:15-21): scatter-add of grad_out (B,C,M)
 * into grad_points (B,C,N), which the caller pre-zeroes (pointnet2_utils.py:67). */
int g4d_gather_grad_f32(int b, int c, int n, int m, const float *grad_out, const int *idx, float *grad_points,
                        g4d_stream_t stream);

/* ball_query_kernel_launcher_fast (ball_query_gpu.h:12-13, ball_query_gpu.cu:9-67).
 * new_xyz (B,M,3) queries, xyz (B,N,3); idx (B,M,nsample) int32, first `nsample` in-radius
 * (d2 < radius*radius, strict) indices in ascending order, padded with the first hit; rows with
 * no hit are written as zeros (the reference leaves the caller's pre-zeroed row untouched). */
int g4d_ball_query_f32(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                       int *idx, g4d_stream_t stream);

/* Multi-scale ball query: the same queries against `nscales` (<= 4) radii in ONE pass over the cloud (each distance
 * is evaluated once and compared with every radius) -- the MSG layers of the reference call ball_query once per scale
 * (pointnet2_modules.py:37-38).  radii / nsamples / idx are HOST arrays of length nscales; idx[s] is a device
 * (B,M,nsamples[s]) int32 buffer, fully written (no pre-zeroing needed).  Per-scale results identical to
 * g4d_ball_query_f32. */
int g4d_ball_query_msg_f32(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                           const float *new_xyz, const float *xyz, int *const *idx, g4d_stream_t stream);

/* g4d_ball_query_msg_f32 for clouds whose index order is spatially coherent (mesh vertices in mesh order: the body and
 * garment queries of modules/mesh_encoder.py:452-464): a pre-pass writes the bounds of every 16-point sub-block into `boxes`
 * (b * ceil(n/16) * 6 floats of scratch) and the search skips sub-blocks that lie outside the largest still-open ball
 * (monotone fp32 bound: never skips a hit).  Same results as g4d_ball_query_msg_f32 for ANY cloud; faster only for
 * coherent ones (a few % slower for random order). */
int g4d_ball_query_boxes_f32(int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *new_xyz,
                             const float *xyz, int *const *idx, float *boxes, g4d_stream_t stream);

/* g4d_ball_query_msg_f32 for COHERENT query sets (64 consecutive queries close together: mesh vertices in mesh order) against an
 * index-coherent cloud, dense balls (far more hits than nsample): one LANE per query, the cloud's 64-point blocks visited in index
 * order by the whole wave, blocks culled against the bounding box of the wave's still-collecting queries (`boxes` =
 * b * ceil(n/64) * 6 floats of scratch; the buffer of g4d_ball_query_boxes_f32 is large enough).  `qsort`: optional g4d_ball_query_lanes_qsort_bytes(b, m)
 * bytes of scratch -- when given, the queries are first counting-sorted into cells of half the largest radius, so that the 64
 * queries of a wave are compact WHATEVER order the caller's queries come in (NULL: the caller's order is used as is and had
 * better be coherent).  Same results as g4d_ball_query_msg_f32 for ANY input. */
size_t g4d_ball_query_lanes_qsort_bytes(int b, int m);
int g4d_ball_query_lanes_f32(int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *new_xyz,
                             const float *xyz, int *const *idx, float *boxes, void *qsort, g4d_stream_t stream);

/* Cell-bucketed ball query (csrc/ball_grid.hip): the same results as g4d_ball_query_msg_f32, bit for bit, for ANY input, with
 * work proportional to the points NEAR each query instead of to N -- for large clouds with small balls (BASELINE configs 2, 5).
 * `grid` is caller-provided device scratch of g4d_ball_grid_bytes(b, n) bytes: a per-cloud uniform grid (cell edge 1.01 * rmax)
 * with the cloud counting-sorted into cell order.  A grid depends on (xyz, rmax) only: build it once, query it with any
 * radii <= rmax as often as needed (e.g. on a side stream while FPS is still choosing the queries).
 *   g4d_ball_query_grid_f32 = build (rmax = the largest radius) + query in one call. */
size_t g4d_ball_grid_bytes(int b, int n);
int g4d_ball_grid_build_f32(int b, int n, float rmax, const float *xyz, void *grid, g4d_stream_t stream);
int g4d_ball_grid_query_f32(int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *new_xyz,
                            const float *xyz, int *const *idx, const void *grid, float grid_rmax, g4d_stream_t stream);
int g4d_ball_query_grid_f32(int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *new_xyz,
                            const float *xyz, int *const *idx, void *grid, g4d_stream_t stream);

/* group_points_kernel_launcher_fast (group_points_gpu.h:13-15): out[b,c,p,s] = points[b,c,idx[b,p,s]].
 * 64-bit offsets (the reference's int32 offsets wrap at 2^31 elements). */
int g4d_group_f32(int b, int c, int n, int npoints, int nsample, const float *points, const int *idx, float *out,
                  g4d_stream_t stream);

/* group_points_grad_kernel_launcher_fast (group_points_gpu.h:17-20): scatter-add, pre-zeroed dst. */
int g4d_group_grad_f32(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                       float *grad_points, g4d_stream_t stream);

/* three_nn_kernel_launcher_fast (interpolate_gpu.h:13-15, interpolate_gpu.cu:9-74).
 * unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3) SQUARED distances, idx (B,n,3) int32. */
int g4d_three_nn_f32(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                     g4d_stream_t stream);

/* The same search over a cell grid of the known points (csrc/ball_grid.hip): bit-identical output, work per unknown point ~ the
 * points of the 27 cells around it instead of m.  `grid`: g4d_ball_grid_bytes(b, m) bytes of device scratch (overwritten). */
int g4d_three_nn_grid_f32(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, void *grid,
                          g4d_stream_t stream);

/* three_interpolate_kernel_launcher_fast (interpolate_gpu.h:18-21):
 * out[b,c,p] = sum_i weight[b,p,i] * points[b,c,idx[b,p,i]];  points (B,C,m) -> out (B,C,n). */
int g4d_three_interp_f32(int b, int c, int m, int n, const float *points, const int *idx, const float *weight,
                         float *out, g4d_stream_t stream);

/* three_interpolate_grad_kernel_launcher_fast (interpolate_gpu.h:24-28): scatter-add, pre-zeroed dst. */
int g4d_three_interp_grad_f32(int b, int c, int n, int m, const float *grad_out, const int *idx,
                              const float *weight, float *grad_points, g4d_stream_t stream);

/* ---- fused shared-MLP layers on the matrix cores (garment4d_amd/csrc/mlp.hip) --------------------------
 * One call = one layer  Y = act((A . W^T) * scale + shift).  W is (CoutPad64, Kpad) row-major fp32, zero
 * padded (Kpad % 32 == 0, CoutPad64 % 64 == 0); scale/shift (CoutPad64) carry the folded BatchNorm affine /
 * conv bias.  Activations are POINT-MAJOR (rows, channels).  Outputs land at column `col0` of rows of width
 * `ldo` (multi-scale concat for free).  These replace the un-fused chain QueryAndGroup -> SharedMLP ->
 * max_pool2d (pointnet2_utils.py:242-265, pytorch_utils.py:5-32, pointnet2_modules.py:37-53), three_interpolate
 * -> cat -> SharedMLP (pointnet2_modules.py:139-156) and GraphConvolution.forward (modules/pygcn/layers.py:35-55). */

/* A = X (rows, ldx) point-major; pool (0 none | 1 max | 2 avg) over s_pool in {16,32,64} consecutive rows. */
int g4d_linear_f32(long long rows, int K, int Kpad, int Cout, const float *X, int ldx, const float *W,
                   const float *scale, const float *shift, int relu, int pool, int s_pool, float *out, int ldo,
                   int col0, g4d_stream_t stream);

/* A row (b,p,s) = [xyz[b,idx[b,p,s]] - new_xyz[b,p] (if use_xyz) | feats[b,idx[b,p,s],:]] ; feats (B,N,C)
 * point-major; pool: 0 none (out rows = B*P*S), 1 max, 2 avg over the S samples (out rows = B*P; S in {16,32,64}). */
int g4d_group_linear_f32(int b, int n, int p, int s, int c, int use_xyz, const float *xyz, const float *new_xyz,
                         const float *feats, const int *idx, int Kpad, int Cout, const float *W, const float *scale,
                         const float *shift, int relu, int pool, float *out, int ldo, int col0, g4d_stream_t stream);

/* A row (b,p) = [sum_i w_i known_feats[b,nn_idx[b,p,i],:] (C2) | skip[b,p,:] (C1)], w_i = normalised
 * 1/(sqrt(dist2_i)+1e-8); known_feats (B,m,C2), skip (B,n,C1) point-major; dist2/nn_idx from g4d_three_nn_f32. */
int g4d_interp_linear_f32(int b, int n, int m, int c2, int c1, const float *known_feats, const float *skip,
                          const float *dist2, const int *nn_idx, int Kpad, int Cout, const float *W,
                          const float *scale, const float *shift, int relu, float *out, int ldo, int col0,
                          g4d_stream_t stream);

/* GCN layer: A row (f,v) = sum_u Ahat[v,u] X[f,u,:] with Ahat in CSR (rowptr (Vg+1), colidx, vals);
 * out = A . W^T * scale + shift  ==  Ahat (X W) + b  with W^T = reference weight (Fin,Fout), shift = bias. */
int g4d_gcn_linear_f32(int frames, int vg, int fin, const float *X, int ldx, const int *rowptr, const int *colidx,
                       const float *vals, int Kpad, int Cout, const float *W, const float *scale, const float *shift,
                       int relu, float *out, int ldo, int col0, g4d_stream_t stream);

/* A whole shared-MLP stack (1..4 layers, hidden widths <= 128) in one launch with the activations resident in LDS
 * (garment4d_amd/csrc/mlp_stack.hip).  mode: 0 DIRECT (X, ldx) | 1 GROUP (N,P,S,C,use_xyz,xyz,new_xyz,feats,idx) |
 * 2 INTERP (n,m,C2,C1,known_feats,skip,dist2,nn_idx) | 3 CSR (X,ldx,Vg,rowptr,colidx,vals); arguments of the other
 * modes are ignored.  Layers are parallel HOST arrays of length nlayers; scale/shift as for g4d_linear_f32, but W[l]
 * is in FRAGMENT order [CoutPad64/16][Kpad/16][64][4]: element ((t*(Kpad/16) + s)*64 + q*16 + i)*4 + e holds
 * W[16t + i][16s + 4q + e], so that one B-fragment load of a wave is a contiguous 1 KB read.  pool over S in {4,8,16,32,64} rows applies to the last layer.  tap_out (or NULL): hidden layer
 * `tap_layer`'s output is also stored, rows x tap_ld. */
int g4d_mlp_stack_f32(int mode, long long rows, int K0, const float *X, int ldx, int N, int P, int S, int C, int use_xyz,
                      const float *xyz, const float *new_xyz, const float *feats, const int *idx, int n, int m, int C2,
                      int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx, int Vg,
                      const int *rowptr, const int *colidx, const float *vals, int nlayers, const float *const *W,
                      const float *const *scale, const float *const *shift, const int *Kpad, const int *Cout,
                      const int *relu, int pool, float *out, int ldo, int col0, int tap_layer, float *tap_out,
                      int tap_ld, g4d_stream_t stream);

/* bf16 variant of g4d_mlp_stack_f32 (BASELINE config 3: bf16 MLP operands, fp32 accumulate / affine / pooling / I/O):
 * W[l] is bf16 in fragment order [CoutPad64/16][Kpad/32][64][8] -- element ((t*(Kpad/32) + s)*64 + q*16 + i)*8 + e
 * holds W[16t + i][32s + 8q + e]; activations are rounded to bf16 (RNE) between layers.  Wide stacks fit too
 * (LDS holds 2 bytes per activation).  garment4d_amd/csrc/mlp_stack_bf16.hip. */
int g4d_mlp_stack_bf16(int mode, long long rows, int K0, const float *X, int ldx, int N, int P, int S, int C, int use_xyz,
                       const float *xyz, const float *new_xyz, const float *feats, const int *idx, int n, int m, int C2,
                       int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx, int Vg,
                       const int *rowptr, const int *colidx, const float *vals, int nlayers,
                       const unsigned short *const *W, const float *const *scale, const float *const *shift,
                       const int *Kpad, const int *Cout, const int *relu, int pool, float *out, int ldo, int col0,
                       int tap_layer, float *tap_out, int tap_ld, g4d_stream_t stream);

/* Wave-autonomous variant of g4d_mlp_stack_f32 for narrow stacks (every hidden width <= 64): each wave takes 64 rows
 * through all layers with no workgroup barrier (garment4d_amd/csrc/mlp_wave.hip).  Same arguments, no tap. */
int g4d_mlp_wave_f32(int mode, long long rows, int K0, const float *X, int ldx, int N, int P, int S, int C, int use_xyz,
                     const float *xyz, const float *new_xyz, const float *feats, const int *idx, int n, int m, int C2,
                     int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx, int Vg,
                     const int *rowptr, const int *colidx, const float *vals, int nlayers, const float *const *W,
                     const float *const *scale, const float *const *shift, const int *Kpad, const int *Cout,
                     const int *relu, int pool, float *out, int ldo, int col0, g4d_stream_t stream);

/* Register-resident variant of g4d_mlp_stack_f32 (garment4d_amd/csrc/mlp_chain.hip): hidden layers are evaluated
 * transposed, so a layer's MFMA accumulators ARE the next layer's operand fragments -- no LDS, no barrier between layers.
 * DIRECT (mode 0), GROUP (1) or INTERP (2) loader; 1..4 layers whose widths, rounded up to 16, form one of the combinations
 * g4d_mlp_chain_supported() accepts (16-16-32, 32-32-64, 64-64-128, 128-128-256, 32-32, 64-64, 128-128, 128-64, single layers
 * up to 128, 128-64-32-16).  Same arguments as g4d_mlp_stack_f32 without the CSR loader (W in fragment order); pool over S
 * in {4,8,16,32,64}; tap_out (or NULL): hidden layer tap_layer is also written to HBM. */
/* Set-abstraction stack over xyz-only neighbourhoods (QueryAndGroup(use_xyz=True, features=None) -> SharedMLP [3, c1, c2, c3] -> max / avg
 * over the nsample rows; pointnet2_modules.py:40-53, the first level of Pointnet2MSGSEG): persistent waves, all weights in registers,
 * layer 1 on the VALU.  (c1, c2, c3) in {(16,16,32), (32,32,64)}, nsample in {16, 32} (g4d_sa_xyz_mlp3_supported).  W1: (c1, ldw1) row-major,
 * columns 0..2; W2_frag / W3_frag: fragment order [16-channel tile][kpad/16 k-steps][lane][4] (the Wf of the LDS-resident kernels);
 * scale / shift: folded BatchNorm per channel, ReLU after every layer.  out (b*p, ldo) point-major at column col0. */
int g4d_sa_xyz_mlp3_supported(int c1, int c2, int c3, int nsample);
int g4d_sa_xyz_mlp3_f32(int b, int n, int p, int nsample, const float *xyz, const float *new_xyz, const int *idx, int c1, int c2, int c3,
                        const float *W1, int ldw1, const float *scale1, const float *shift1, const float *W2_frag, int kpad2,
                        const float *scale2, const float *shift2, const float *W3_frag, int kpad3, const float *scale3, const float *shift3,
                        int pool, float *out, int ldo, int col0, g4d_stream_t stream);

int g4d_mlp_chain_supported(int nlayers, const int *Cout);
int g4d_mlp_chain_f32(int mode, long long rows, int K0, const float *X, int ldx, int N, int P, int S, int C, int use_xyz,
                      const float *xyz, const float *new_xyz, const float *feats, const int *idx, int n, int m, int C2,
                      int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx, int nlayers,
                      const float *const *W, const float *const *scale, const float *const *shift, const int *Kpad,
                      const int *Cout, const int *relu, int pool, float *out, int ldo, int col0, int tap_layer,
                      float *tap_out, int tap_ld, g4d_stream_t stream);

/* bf16 variant of g4d_mlp_chain_f32 (BASELINE config 3): operands bf16 (RNE), fp32 accumulate / affine / pool / I/O.
 * W[l]: bf16 in CHAIN order [CoutPad64/16][Kpad/32][64 lanes][8]: lane (fi, g) element e holds
 * W[16 t + fi][32 s + (e < 4 ? 4 g + e : 16 + 4 g + e - 4)] (garment4d_amd/csrc/mlp_chain_bf16.hip explains the permutation). */
int g4d_mlp_chain_bf16(int mode, long long rows, int K0, const float *X, int ldx, int N, int P, int S, int C, int use_xyz,
                       const float *xyz, const float *new_xyz, const float *feats, const int *idx, int n, int m, int C2,
                       int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx, int nlayers,
                       const unsigned short *const *W, const float *const *scale, const float *const *shift, const int *Kpad,
                       const int *Cout, const int *relu, int pool, float *out, int ldo, int col0, int tap_layer,
                       float *tap_out, int tap_ld, g4d_stream_t stream);

/* g4d_mlp_chain_bf16 in its interpolating mode (mode 2) with the ball-grid workspace of the UNKNOWN cloud at hand (g4d_ball_grid_build_f32 on
 * `unknown`, any radius; n points per cloud): large launches walk the rows in the grid's cell order, so that consecutive rows share their
 * nearest known points (fp_head_bf16.hip) -- every output row holds the same bits as with g4d_mlp_chain_bf16 (a row is computed from its
 * own operands only); launches the cell-ordered kernel does not take run as g4d_mlp_chain_bf16 would.  dist2 / nn_idx / out / tap_out stay
 * in the cloud's ORIGINAL row order. */
int g4d_mlp_chain_cells_bf16(int mode, long long rows, int K0, const float *X, int ldx, int N, int P, int S, int C, int use_xyz,
                             const float *xyz, const float *new_xyz, const float *feats, const int *idx, int n, int m, int C2,
                             int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx, int nlayers,
                             const unsigned short *const *W, const float *const *scale, const float *const *shift, const int *Kpad,
                             const int *Cout, const int *relu, int pool, float *out, int ldo, int col0, int tap_layer,
                             float *tap_out, int tap_ld, const void *unknown_grid, g4d_stream_t stream);

/* ---- ONE argument block for the whole-stack launchers (round 6).  The seven entry points above take 34-41 positional arguments that every
 * binding has to mirror by hand; new code fills a g4d_mlp_args and calls g4d_mlp_run(family, &args, stream) -- the positional entry points stay
 * (same kernels behind both) for source compatibility.  `size` = sizeof(g4d_mlp_args) as the CALLER compiled it and `version` =
 * G4D_MLP_ARGS_VERSION: a block that is larger than the library's, or of another version, is refused (G4D_EINVAL) instead of misread; a
 * smaller one of the same version is accepted with its missing tail treated as zero (fields are only ever appended).  Fields of loaders the
 * chosen `mode` does not use are ignored.  g4d_mlp_args_size() returns the library's sizeof for bindings that cannot see this header. */
#define G4D_MLP_ARGS_VERSION 1
enum g4d_mlp_family {
    G4D_MLP_STACK_F32 = 0,   /* g4d_mlp_stack_f32:  LDS-resident stack, fp32; W = fp32 fragment order */
    G4D_MLP_STACK_BF16 = 1,  /* g4d_mlp_stack_bf16: W = bf16 fragment order */
    G4D_MLP_WAVE_F32 = 2,    /* g4d_mlp_wave_f32:   wave-autonomous narrow stacks (no tap) */
    G4D_MLP_CHAIN_F32 = 3,   /* g4d_mlp_chain_f32:  register chain (no CSR loader) */
    G4D_MLP_CHAIN_BF16 = 4,  /* g4d_mlp_chain_bf16 -- or g4d_mlp_chain_cells_bf16 when unknown_grid != NULL; W = bf16 chain order */
    G4D_MLP_CHAIN_BF16X3 = 5 /* g4d_mlp_chain_bf16x3: W = 3 * nlayers pointers (hi | mid | lo pieces) */
};
typedef struct g4d_mlp_args {
    unsigned size, version;
    int mode;                      /* 0 DIRECT | 1 GROUP | 2 INTERP | 3 CSR */
    int K0;                        /* input width of the first layer */
    long long rows;
    const float *X; int ldx;       /* DIRECT / CSR: the (rows, ldx) input */
    int N, P, S, C, use_xyz;       /* GROUP: source points / centroids per cloud, samples, feature columns; S is also the pooling window */
    const float *xyz, *new_xyz, *feats; const int *idx;
    int n, m, C2, C1;              /* INTERP: unknown / known points per cloud, known-feature and skip columns */
    const float *known_feats, *skip, *dist2; const int *nn_idx;
    int Vg; const int *rowptr, *colidx; const float *vals;   /* CSR */
    int nlayers;
    const void *const *W;          /* nlayers pointers (3 * nlayers for G4D_MLP_CHAIN_BF16X3), layout per family */
    const float *const *scale, *const *shift;
    const int *Kpad, *Cout, *relu; /* HOST arrays of nlayers */
    int pool;                      /* 0 none | 1 max | 2 avg over S rows, last layer */
    float *out; int ldo, col0;
    int tap_layer; float *tap_out; int tap_ld;   /* tap_out == NULL: no tap */
    const void *unknown_grid;      /* G4D_MLP_CHAIN_BF16, mode 2: the unknown cloud's ball-grid workspace (rows walked in cell order) or NULL */
} g4d_mlp_args;
unsigned g4d_mlp_args_size(void);
int g4d_mlp_run(int family, const g4d_mlp_args *args, g4d_stream_t stream);

/* Wide feature-propagation level with bf16 operands as two tiled GEMMs behind an interpolation pre-pass (csrc/gemm_bf16.hip): the
 * large-launch form of g4d_mlp_stack_bf16 in its interpolating mode, bit-identical to it.  Buffers in "fragment order" hold a (rows, kpad)
 * bf16 matrix as [16-row tile][32-column k-step][64 lanes][8] -- the A operand of v_mfma_f32_16x16x32_bf16 -- with the rows padded to whole
 * 128-row blocks: g4d_frag_bf16_elems(rows, kpad) = the number of bf16 elements to allocate (-1: bad arguments).
 *   g4d_interp_concat_frag_bf16: x16 = bf16([three_interpolate(known_feats (b, m, C2)) ; skip (b, n, C1)]) of every row, zero padded to kpad
 *     columns (C2 % 8 == 0; kpad % 32 == 0; pointnet2_modules.py:140-150, the interpolation in fp32, one RNE rounding per element).
 *   g4d_gemm_frag_bf16: act((A . W^T) * scale + shift) with A in fragment order (kpad % 64 == 0), W = the layer's bf16 weights in fragment
 *     order [16-channel tile][kpad / 32][64][8] padded to a multiple of 128 channels, fp32 accumulation; the result either rounded to bf16
 *     in fragment order for the next layer (out16, kpad_out columns) or fp32 row-major (out, ldo, col0) -- exactly one of the two. */
long long g4d_frag_bf16_elems(long long rows, int kpad);
int g4d_interp_concat_frag_bf16(int b, int n, int m, int C2, int C1, const float *known_feats, const float *skip, const float *dist2,
                                const int *nn_idx, int kpad, unsigned short *x16, g4d_stream_t stream);
int g4d_gemm_frag_bf16(long long rows, int kpad, const unsigned short *A16, const unsigned short *W16, const float *scale, const float *shift, int relu,
                       int Cout, unsigned short *out16, int kpad_out, float *out, int ldo, int col0, g4d_stream_t stream);

/* fp32-ACCURATE variant on the bf16 matrix cores ("bf16x3"): every fp32 operand is split exactly into three bf16 pieces
 * (hi = x & 0xffff0000, mid = (x - hi) & 0xffff0000, lo = x - hi - mid) and a product is the sum of the six largest piece products,
 * accumulated in fp32 -- error of the order of one fp32 rounding per product, six bf16 MFMAs instead of eight fp32 ones per
 * 16 x 16 x 32 block (gfx950: 157 TFLOP/s fp32 MFMA against 2.5 PFLOP/s bf16).  Same arguments as g4d_mlp_chain_bf16 except
 * W3: 3 * nlayers pointers, [3 l + 0 | 1 | 2] = the hi | mid | lo pieces of layer l, each bf16 in CHAIN order. */
int g4d_mlp_chain_bf16x3(int mode, long long rows, int K0, const float *X, int ldx, int N, int P, int S, int C, int use_xyz,
                         const float *xyz, const float *new_xyz, const float *feats, const int *idx, int n, int m, int C2,
                         int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx, int nlayers,
                         const unsigned short *const *W3, const float *const *scale, const float *const *shift, const int *Kpad,
                         const int *Cout, const int *relu, int pool, float *out, int ldo, int col0, int tap_layer,
                         float *tap_out, int tap_ld, g4d_stream_t stream);

/* Batched SpMM of the GCN layer: out (frames,Vg,C) = Ahat (CSR) . S (frames,Vg,C) + bias (C, may be NULL), optional ReLU
 * (the caller's F.relu, modules/mesh_encoder.py:479-480, fused), all point-major (modules/pygcn/layers.py:44-55 without
 * the transposes).  GraphConvolution = g4d_linear_f32 then this. */
int g4d_spmm_rows_f32(int frames, int vg, int c, const float *S, const int *rowptr, const int *colidx, const float *vals,
                      const float *bias, int relu, float *out, g4d_stream_t stream);

/* Aggregation of GCN layer i fused with the contraction of layer i+1 (modules/mesh_encoder.py:477-481: four chained
 * GraphConvolutions per refinement round), in the reference's operation order:
 *   h = act(Ahat . S + bias)   (S = X W_i already contracted, (frames,Vg,128) point-major; CSR Ahat; act = ReLU if relu)
 *   out = h . W_next           ((frames,Vg,cout) point-major, cout == 128 or cout <= 16)
 * h is written to `tap` ((frames,Vg,128)) when tap != NULL and never touches HBM otherwise.  h is bit-identical to
 * g4d_spmm_rows_f32.  Wp = W_next^T padded to (ceil(cout/16)*16, 128), fragment order [16-channel tile][8 k-steps of 16][lane =
 * 16*(k/4 mod 4) + channel mod 16][4 consecutive k].  c must be 128. */
int g4d_gcn_agg_linear_f32(int frames, int vg, int c, const float *S, const int *rowptr, const int *colidx, const float *vals,
                           const float *bias, int relu, float *tap, const float *Wp, int cout, float *out, g4d_stream_t stream);

/* The same launch with per-MESH tile metadata (round 5): the window of neighbouring rows and the padded (column, weight) rows of every
 * 128-vertex tile depend on the adjacency only -- the same for every frame, layer and refinement round -- so a caller that keeps the mesh
 * builds them once (g4d_gcn_tile_meta_build into g4d_gcn_tile_meta_bytes(vg) bytes of device memory) and passes them here; the kernel's
 * workgroups then skip three dependent round trips through the CSR arrays.  meta == NULL behaves as g4d_gcn_agg_linear_f32; results are
 * identical either way.  (The adjacency of modules/mesh_encoder.py:288-307 is built in the model's constructor and never changes.) */
long long g4d_gcn_tile_meta_bytes(int vg);
int g4d_gcn_tile_meta_build(int vg, const int *rowptr, const int *colidx, const float *vals, void *meta, g4d_stream_t stream);
int g4d_gcn_agg_linear_meta_f32(int frames, int vg, int c, const float *S, const int *rowptr, const int *colidx, const float *vals,
                                const float *bias, int relu, float *tap, const float *Wp, int cout, float *out, const void *meta,
                                g4d_stream_t stream);

/* ---- backward of the GCN layer  Y = act(Ahat . (X W) + b)  (csrc/gcn_grad.hip); rows = frames * Vg, everything point-major ----------
 * With G = dY where act is the identity and G = (Y > 0 ? dY : 0) where it is the fused ReLU (Y = the layer's OUTPUT; G is never stored):
 *   dS = Ahat^T . G   g4d_spmm_rows_grad_f32        db = column sums of G   g4d_col_sum_rows_f32
 *   dW = X^T . dS     g4d_gemm_tn_f32               dX = dS . W^T           g4d_linear_f32 with W as the (Cout = Fin, K = Cout) weight
 * All three are deterministic (no atomics; partial sums per row slice, added in a fixed order that depends on the shape only). */

/* dS (frames,Vg,C) = Ahat^T . G per frame.  rowptr_t / colidx_t / vals_t: the CSR of Ahat^T (row u lists the v with Ahat[v,u] != 0; the
 * order of a row's entries is the summation order).  Y == NULL: no mask (G = dY).  One thread per 4 channels of a row, as g4d_spmm_rows_f32. */
int g4d_spmm_rows_grad_f32(int frames, int vg, int c, const float *dY, const float *Y, const int *rowptr_t, const int *colidx_t,
                           const float *vals_t, float *dS, g4d_stream_t stream);

/* db (C) = sum over the rows of G (rows,C); Y == NULL: no mask.  ws: g4d_col_sum_rows_ws_bytes(rows, c) bytes.  rows == 0 writes zeros. */
long long g4d_col_sum_rows_ws_bytes(long long rows, int c);
int g4d_col_sum_rows_f32(long long rows, int c, const float *dY, const float *Y, float *ws, float *db, g4d_stream_t stream);

/* dW (Fin,Cout) = X^T . dS with X (rows, Fin) of row stride ldx >= Fin floats and dS (rows, Cout) dense: the contraction runs along the
 * ROWS, on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, the row as k; neither tensor is transposed or padded).  The rows are cut into
 * slices of g4d_gemm_tn_slice_rows(rows, Fin, Cout) rows -- a function of the shape alone -- whose partial tiles go to ws
 * (g4d_gemm_tn_ws_bytes bytes) and are then added in slice order.  Any Fin, Cout >= 1; X and dS are read once when Cout <= 128 and Fin
 * is 128, 193..224 or 321..352 (the model's 128 / 195 / 323), otherwise dS once per 128 features.  rows == 0 writes zeros. */
long long g4d_gemm_tn_slice_rows(long long rows, int fin, int cout);
long long g4d_gemm_tn_ws_bytes(long long rows, int fin, int cout);
int g4d_gemm_tn_f32(long long rows, int fin, int ldx, int cout, const float *X, const float *dS, float *ws, float *dW, g4d_stream_t stream);

/* max (is_max=1) / mean over S consecutive rows, any S: in (groups*S, ldi) -> out (groups, ldo) at col0. */
int g4d_pool_rows_f32(int groups, int s, int c, const float *in, int ldi, float *out, int ldo, int col0, int is_max,
                      g4d_stream_t stream);

/* ---- training-mode BatchNorm on point-major rows, and the adjoint of the row max-pool (csrc/bn_train.hip; garment4d_amd/mlp_train.py) ----
 * Y (rows, C) with a row stride ld >= C floats, one column = one channel.  fp32; every output is written once; no atomics; the rows are cut
 * into slices of g4d_bn_slice_rows(rows, c) rows -- a function of the shape alone -- whose partial sums go to ws and are added in slice
 * order, so two runs give the same bits.  Negative sizes, ld < C and null pointers (where not optional) return G4D_EINVAL before any launch.
 *
 * g4d_bn_stats_f32: mean (C) and BIASED variance (C) over the rows, two passes (sum y, then sum (y - mean)^2).  ws: g4d_bn_stats_ws_bytes
 * bytes.  rows == 0 writes zeros. */
long long g4d_bn_slice_rows(long long rows, int c);
long long g4d_bn_stats_ws_bytes(long long rows, int c);
int g4d_bn_stats_f32(long long rows, int c, const float *Y, int ldy, float *ws, float *mean, float *var, g4d_stream_t stream);
/* out = act(z), z = fma((y - mean) * invstd, gamma, beta), invstd = 1 / sqrt(var + eps); relu != 0: act(z) = z > 0 ? z : 0.  gamma / beta
 * NULL: 1 / 0. */
int g4d_bn_act_f32(long long rows, int c, const float *Y, int ldy, const float *mean, const float *var, float eps, const float *gamma,
                   const float *beta, int relu, float *out, int ldo, g4d_stream_t stream);
/* With G = dOut where the activation passed (z > 0, z recomputed from Y by the expression of g4d_bn_act_f32) and 0 elsewhere:
 * dbeta (C) = sum G, dgamma (C) = sum G * xhat, xhat = (y - mean) * invstd.  ws: g4d_bn_act_grad_reduce_ws_bytes bytes.  rows == 0 writes zeros. */
long long g4d_bn_act_grad_reduce_ws_bytes(long long rows, int c);
int g4d_bn_act_grad_reduce_f32(long long rows, int c, const float *dOut, int ldg, const float *Y, int ldy, const float *mean, const float *var,
                               float eps, const float *gamma, const float *beta, int relu, float *ws, float *dgamma, float *dbeta,
                               g4d_stream_t stream);
/* dY = gamma * invstd * (G - dbeta / rows - xhat * dgamma / rows); batch_stats == 0 (running statistics): dY = gamma * invstd * G and
 * dgamma / dbeta may be NULL. */
int g4d_bn_act_grad_f32(long long rows, int c, const float *dOut, int ldg, const float *Y, int ldy, const float *mean, const float *var, float eps,
                        const float *gamma, const float *beta, int relu, int batch_stats, const float *dgamma, const float *dbeta, float *dY,
                        int lddy, g4d_stream_t stream);
/* Adjoint of g4d_pool_rows_f32(is_max = 1): X (groups*S, ldx), dPooled (groups, ldp) read at col0, dX (groups*S, C) dense.  Per (group,
 * channel) the FIRST row attaining the maximum receives dPooled, the other S - 1 rows 0.  Any S >= 1. */
int g4d_pool_rows_max_grad_f32(int groups, int s, int c, const float *X, int ldx, const float *dPooled, int ldp, int col0, float *dX,
                               g4d_stream_t stream);

/* point-major row gather: out[b,j,:] = in[b,idx[b,j],:], rows of c floats (new_xyz = xyz[fps idx] with c=3;
 * same result as gather_points on the transposed tensor, pointnet2_modules.py:32-35, without the two transposes). */
int g4d_gather_rows_f32(int b, int n, int m, int c, const float *in, const int *idx, float *out, g4d_stream_t stream);

/* point-major three_interpolate + skip concat: out (B,n,C2+C1) = [sum_i w_i known_feats[b,nn_idx_i,:] | skip[b,p,:]],
 * w_i = normalised 1/(sqrt(dist2_i)+1e-8) (pointnet2_modules.py:139-149).  Used ahead of g4d_linear_f32 when the FP
 * stack is too wide for the LDS-resident kernels (each 64-channel tile would otherwise redo the interpolation). */
int g4d_interp_concat_f32(int b, int n, int m, int c2, int c1, const float *known_feats, const float *skip,
                          const float *dist2, const int *nn_idx, float *out, g4d_stream_t stream);

/* batched matrix transpose (b, r, c) -> (b, c, r): channel-major <-> point-major at the API boundary. */
int g4d_transpose_f32(int b, int r, int c, const float *in, float *out, g4d_stream_t stream);

/* Wide feature-propagation level, first layer with its known-feature part pre-contracted (pointnet2_modules.py:127-156):
 *   out = act((X . W^T + three_interpolate(table)) * scale + shift)
 * X (rows, ldx >= K): the skip features; W (CoutPad64, Kpad) row-major: the skip columns of the layer's weight; table (B*m rows, stride tab_ld >=
 * Cout): the known features times the remaining columns (one small g4d_linear_f32 over the m known rows instead of the n interpolated ones);
 * dist2 / nn_idx (rows, 3) as g4d_three_nn_f32 returns them; rows = B*n.  The interpolation is added to the finished contraction, then the
 * affine and the ReLU.  Same kernels, k order and tiling as g4d_linear_f32. */
int g4d_linear_interp_add_f32(long long rows, int n, int m, int K, int Kpad, int Cout, const float *X, int ldx, const float *W, const float *table,
                              int tab_ld, const float *dist2, const int *nn_idx, const float *scale, const float *shift, int relu, float *out, int ldo,
                              int col0, g4d_stream_t stream);

/* Run-time tuning switches of the large-launch kernels.  Keys: "sa_table_persistent", "sa_table_min_rows", "sa_table_128", "sa_table_oversub", "sa_table_dedup", "fp_table_persistent",
 * "fp_table_min_rows", "fp_init_persistent", "fp_init_min_rows", "fp_head_bf16_persistent", "fp_head_bf16_min_rows", "sa_group_bf16_persistent",
 * "sa_group_bf16_min_rows", "gemm_tile", "gemm_tile_min_rows", "gemm_tile_min_cout", "gemm_tile_min_kpad".  Resolution order, per launch, on the
 * launching host thread: the thread's override (g4d_tuning_set_thread) > the process-wide value (g4d_tuning_set) > the environment variable
 * G4D_<KEY IN UPPER CASE> (read once, on first use) > the built-in default.  For A/B measurements, tests and executors that carry their own
 * tuning (garment4d_amd/tuning.py) -- every setting computes the same bits.  g4d_tuning_set_thread(key, value, set): set != 0 installs the
 * override for launches made by the calling thread, set == 0 removes it. */
int g4d_tuning_set(const char *key, long long value);
int g4d_tuning_set_thread(const char *key, long long value, int set);

/* Up to 4 contiguous device-to-device copies (dst[i][0 .. nfloats[i]) = src[i][...]) in one launch -- the executor of
 * garment4d_amd/pipeline.py hands a step's cloud, betas and pose over with it (the reference moves them with three .cuda() copies per
 * batch, train_temporal.py:239-254).  dst / src / nfloats are HOST arrays of nseg entries. */
int g4d_copy_segments_f32(int nseg, float *const *dst, const float *const *src, const long long *nfloats, g4d_stream_t stream);

/* ---- SMPL linear blend skinning (garment4d_amd/csrc/lbs.hip; reference: smplx/smplx/lbs.py) ------------- */

/* v_shaped (B,V,3) = v_template (V,3) + shapedirs (V,3,NB) . betas (B,NB)       lbs.py:205, blend_shapes :288-309.
 * betas_bstride = NB, or 0 to broadcast one betas row over the batch. */
int g4d_lbs_shape_f32(int b, int v, int nb, const float *betas, int betas_bstride, const float *v_template,
                      const float *shapedirs, float *v_shaped, g4d_stream_t stream);

/* joints (B,J,3) = jreg . verts (B,V,3); jreg (J,V) shared (vertices2joints, lbs.py:251-268) or, with
 * jreg_batched = g > 0, (ceil(B/g),J,V): one regressor per g consecutive samples -- g = 1 per sample (vertices2jointsB,
 * lbs.py:270-286), g = T per clip of T frames. */
int g4d_joint_regress_f32(int b, int j, int v, const float *jreg, int jreg_batched, const float *verts, float *joints,
                          g4d_stream_t stream);

/* batch_rodrigues (lbs.py:312-346): rot_vecs (N,3) -> rot_mats (N,3,3). */
int g4d_rodrigues_f32(int n, const float *rot_vecs, float *rot_mats, g4d_stream_t stream);

/* batch_rigid_transform (lbs.py:362-419), optionally preceded by Rodrigues: pose is (B,J,3) axis-angle when
 * pose2rot != 0, else (B,J,3,3).  joints (B,J,3) rest joints, parents (J) int32 (parents[0] ignored).
 * Outputs: rel_transforms (B,J,4,4) [required]; rot_out (B,J,3,3), posed_joints (B,J,3), pose_feature
 * (B,(J-1)*9) = (R[1:]-I) flattened (lbs.py:217,222) are optional (null to skip).  J <= 64. */
int g4d_rigid_transform_f32(int b, int j, int pose2rot, const float *pose, const float *joints, const int *parents,
                            float *rot_out, float *posed_joints, float *rel_transforms, float *pose_feature,
                            g4d_stream_t stream);

/* verts (B,V,3) = (W . A) [v_in + pose_feature . posedirs ; 1]     (lbs.py:223-246).  v_in (B,V,3);
 * pose_feature (B,PF), posedirs (PF, V*3) -- pass pf = 0 to skip the pose blend shapes (plain skinning, e.g. the
 * garment skinning of modules/mesh_encoder.py:393,406-408); weights (V,J), or, with weights_batched = g > 0,
 * (ceil(B/g),V,J): one weight table per g consecutive samples (1 = per sample, T = per clip);
 * A (B,J,4,4); v_posed_scratch (B,V,3) receives v_posed when pf > 0 (may be NULL when pf == 0). */
int g4d_lbs_pose_skin_f32(int b, int v, int j, int pf, const float *v_in, const float *pose_feature,
                          const float *posedirs, const float *weights, int weights_batched, const float *A,
                          float *v_posed_scratch, float *verts, g4d_stream_t stream);

/* The whole lbs() (smplx/smplx/lbs.py:152-248) in three launches.  Model constants prepared once by the caller:
 * blend_dirs ((NB + (J-1)*9), V*3) = [shapedirs^T ; posedirs], J_template (J,3) = J_regressor v_template, J_shapedirs (J,3,NB) =
 * J_regressor shapedirs.  J_regressor (v_template + shapedirs beta) = J_template + J_shapedirs beta, so the joints need no
 * V-long reduction and v_shaped is never materialised.  coeff_scratch (B, NB + (J-1)*9); A_out (B,J,4,4); posed_joints (B,J,3) or
 * NULL; v_posed_scratch, verts (B,V,3).  pose: (B,J,3) axis-angle (pose2rot != 0) or (B,J,3,3). */
int g4d_lbs_fused_f32(int b, int v, int j, int nb, int pose2rot, const float *betas, int betas_bstride, const float *pose,
                      const float *v_template, const float *blend_dirs, const float *J_template, const float *J_shapedirs,
                      const int *parents, const float *lbs_weights, float *coeff_scratch, float *A_out, float *posed_joints,
                      float *v_posed_scratch, float *verts, g4d_stream_t stream);

/* Feature propagation WITHOUT skip features with its first layer pre-contracted (pointnet2_modules.py:127-156, the last FP level of
 * Pointnet2MSGSEG + the segmentation head): conv(sum_i w_i f_i) = sum_i w_i conv(f_i), so `table` (B*m, C2) holds the known
 * features already multiplied by the first layer's weight (g4d_linear_f32 with scale 1 / shift 0 / no ReLU over m rows per cloud
 * instead of n) and the layer itself is  h = relu(three_interpolate(table) * pre_scale + pre_shift)  inside the loader of the
 * register-chain kernel.  h is written to in_tap (rows x in_tap_ld, NULL: not kept); W / scale / shift / Kpad / Cout / relu describe
 * the REMAINING layers (fragment-order weights as for g4d_mlp_chain_f32; widths per g4d_mlp_chain_supported); tap_layer / tap_out as
 * there.  C2 must be a multiple of 16. */
int g4d_mlp_chain_table_f32(long long rows, int n, int m, int C2, const float *table, const float *dist2, const int *nn_idx,
                            const float *pre_scale, const float *pre_shift, float *in_tap, int in_tap_ld, int nlayers,
                            const float *const *W, const float *const *scale, const float *const *shift, const int *Kpad,
                            const int *Cout, const int *relu, float *out, int ldo, int col0, int tap_layer, float *tap_out, int tap_ld,
                            g4d_stream_t stream);

/* Set abstraction with the FEATURE part of its first layer pre-contracted (pointnet2_utils.py:232-265 + the first SharedMLP layer):
 *   W [x_j - q ; f_j] = Wx (x_j - q) + Wf f_j,   and Wf f_j depends on the source point j only.
 * `table` row j (row stride tab_ld floats, Kt columns used, Kt a multiple of 16, 16-byte aligned) = Wf f_j for source point j of the
 * level -- one g4d_linear_f32 over the B*N source points (scale 1, shift 0, no ReLU) instead of B*P*S grouped rows; tab_wx (3, Kt) =
 * Wx transposed.  The layer itself becomes relu((table[j] + Wx (x_j - q)) * pre_scale + pre_shift) inside the loader of the
 * register-chain kernel; W / scale / shift / Kpad / Cout / relu describe the REMAINING layers (widths per g4d_mlp_chain_supported),
 * pool / out / ldo / col0 as g4d_mlp_chain_f32.  rows = B*P*S. */
/* 1 when a g4d_mlp_chain_group_table_f32 launch of `rows` grouped rows with first-layer width Kt (stack Kt -> Kt -> 2 Kt), nsample S and
 * this pooling mode runs on the persistent kernel (csrc/sa_table.hip) under the calling thread's tuning state -- the only kernel that accepts
 * tab_ld == 0 (an xyz-only stack: one shared table row of zeros).  Hosts ask before choosing that route. */
int g4d_sa_table_supported(long long rows, int Kt, int S, int pool);
int g4d_mlp_chain_group_table_f32(long long rows, int N, int P, int S, const float *xyz, const float *new_xyz, const int *idx,
                                  const float *table, int tab_ld, int Kt, const float *tab_wx, const float *pre_scale,
                                  const float *pre_shift, int nlayers, const float *const *W, const float *const *scale,
                                  const float *const *shift, const int *Kpad, const int *Cout, const int *relu, int pool, float *out,
                                  int ldo, int col0, g4d_stream_t stream);

/* g4d_mlp_chain_group_table_f32 with caller-owned scratch.  ball_query pads a neighbourhood with copies of its first hit
 * (ball_query_gpu.cu:32-36); a padded row is the same (source point, centroid) pair as row 0, produces the same output, and max pooling does not
 * see it.  The persistent kernels therefore skip 16-row tiles / blocks that hold nothing but the neighbourhood's first index -- exact for ANY
 * index list.  The 32- / 64-wide stacks do it on their own; the 128-wide stack's lock-step kernel needs its neighbourhoods sorted by live blocks
 * first (two small pre-pass launches into `ws`: g4d_sa_table_ws_bytes(rows, Kt, S, pool) bytes, 16-byte aligned; 0 = this shape takes no
 * workspace).  ws == NULL or too small: every block is computed.  Tuning key "sa_table_dedup" = 0 switches the work list off. */
long long g4d_sa_table_ws_bytes(long long rows, int Kt, int S, int pool);
int g4d_mlp_chain_group_table_ws_f32(long long rows, int N, int P, int S, const float *xyz, const float *new_xyz, const int *idx,
                                     const float *table, int tab_ld, int Kt, const float *tab_wx, const float *pre_scale,
                                     const float *pre_shift, int nlayers, const float *const *W, const float *const *scale,
                                     const float *const *shift, const int *Kpad, const int *Cout, const int *relu, int pool, float *out,
                                     int ldo, int col0, void *ws, long long ws_bytes, g4d_stream_t stream);

/* three_nn (interpolate_gpu.cu:9-52) when the ball-grid workspace of the UNKNOWN cloud exists already (g4d_ball_grid_build_f32 on
 * `unknown`, any radius -- the encoder has built it for the first set-abstraction level): the scan of g4d_three_nn_f32 with the queries
 * taken in that workspace's cell order, so that the 64 queries of a wave are neighbours and its wave-uniform tests skip the inserts for
 * most known points.  dist2 / idx identical to g4d_three_nn_f32 (written at the original query positions); unknown_grid == NULL falls
 * through to it. */
int g4d_three_nn_cells_f32(int b, int n, int m, const float *unknown, const void *unknown_grid, const float *known, float *dist2, int *idx,
                           g4d_stream_t stream);

/* Feature propagation WITH skip features, the known-feature part of its first layer pre-contracted (pointnet2_modules.py:127-156):
 *   W [interp(f) ; s] = Wa interp(f) + Wb s = interp(Wa f) + Wb s.
 * `table` (B*m rows, row stride tab_ld floats, 16-byte aligned) = known features times Wa^T -- one g4d_linear_f32 over the m known rows
 * per cloud (scale 1, shift 0, no ReLU); the first layer's accumulators start from three_interpolate(table) and the matrix pipe adds the
 * C1 skip columns.  Layer 0 of W / Kpad describes Wb (K = C1, fragment order), its scale / shift / relu are the layer's own; >= 2
 * layers, Cout[0] a multiple of 16; widths per g4d_mlp_chain_supported.  Everything else as g4d_mlp_chain_f32 (mode 2). */
int g4d_mlp_chain_interp_init_f32(long long rows, int n, int m, int C1, const float *skip, const float *table, int tab_ld, const float *dist2,
                                  const int *nn_idx, int nlayers, const float *const *W, const float *const *scale,
                                  const float *const *shift, const int *Kpad, const int *Cout, const int *relu, float *out, int ldo, int col0,
                                  int tap_layer, float *tap_out, int tap_ld, g4d_stream_t stream);

/* Up to four three_nn problems (interpolate_gpu.cu:9-52) of the same batch size b in ONE launch: n[i] unknown / m[i] known points per
 * cloud, unknown[i] (b, n[i], 3), known[i] (b, m[i], 3), dist2[i] / idx[i] (b, n[i], 3).  Each result is identical to g4d_three_nn_f32's.
 * For the inner feature-propagation levels, whose searches are microseconds of work: a launch saved is 3-5 us of the 16-batch mix. */
int g4d_three_nn_multi_f32(int b, int count, const int *n, const int *m, const float *const *unknown, const float *const *known,
                           float *const *dist2, int *const *idx, g4d_stream_t stream);

/* Two ball queries (ball_query_gpu.cu:9-67) of the same batch size and the same number of scales in ONE launch -- the inner
 * set-abstraction levels, whose searches are microseconds of work.  Arguments per problem as g4d_ball_query_msg_f32; each output is
 * identical to that call's. */
int g4d_ball_query_msg2_f32(int b, int nscales, int n0, int m0, const float *radii0, const int *nsamples0, const float *new_xyz0,
                            const float *xyz0, int *const *idx0, int n1, int m1, const float *radii1, const int *nsamples1,
                            const float *new_xyz1, const float *xyz1, int *const *idx1, g4d_stream_t stream);

/* Two consecutive furthest-point-sampling levels in ONE launch (sampling_gpu.cu:93-253 twice: level B samples the m1 points level A
 * picked): idx1 (b, m1) / new_xyz1 (b, m1, 3) / idx2 (b, m2) / new_xyz2 (b, m2, 3) are exactly what g4d_fps_gather_f32(n -> m1) followed by
 * g4d_fps_gather_f32(m1 -> m2) on new_xyz1 give (idx2 indexes new_xyz1).  Shapes: g4d_fps_gather_pair_supported -- n = 1024, m1 = 256,
 * the two inner levels of the Pointnet2MSGSEG encoder. */
int g4d_fps_gather_pair_supported(int n, int m1, int m2);
int g4d_fps_gather_pair_f32(int b, int n, int m1, int m2, const float *xyz, int *idx1, float *new_xyz1, int *idx2, float *new_xyz2,
                            g4d_stream_t stream);

/* Both scales of an xyz-only MSG set-abstraction level in ONE launch: scale 0 = the 16-16-32 stack, scale 1 = the 32-32-64 stack of
 * g4d_sa_xyz_mlp3_f32 (arguments per scale as there: neighbour indices, layer 1 row-major with its affine, layers 2 / 3 in fragment
 * order with theirs, output column).  Same cloud, centroids, pooling mode and output tensor; results identical to the two calls. */
int g4d_sa_xyz_mlp3_pair_f32(int b, int n, int p, const float *xyz, const float *new_xyz, int pool, float *out, int ldo,
                             int nsample0, const int *idx0, const float *W1_0, int ldw1_0, const float *scale1_0, const float *shift1_0,
                             const float *W2_frag0, int kpad2_0, const float *scale2_0, const float *shift2_0, const float *W3_frag0, int kpad3_0,
                             const float *scale3_0, const float *shift3_0, int col0_0,
                             int nsample1, const int *idx1, const float *W1_1, int ldw1_1, const float *scale1_1, const float *shift1_1,
                             const float *W2_frag1, int kpad2_1, const float *scale2_1, const float *shift2_1, const float *W3_frag1, int kpad3_1,
                             const float *scale3_1, const float *shift3_1, int col0_1, g4d_stream_t stream);

/* ---- feature propagation over cell-ordered rows (round 3) ------------------------------------------------------------------------
 * g4d_three_nn_cells_sorted_f32: g4d_three_nn_cells_f32 with the results LEFT in the cell order of `unknown_grid` (row p of cloud b
 * belongs to that cloud's p-th grid record, whose 4th dword is the point's original index).
 * g4d_mlp_chain_table_cells_f32: g4d_mlp_chain_table_f32 whose launch rows are those cell-ordered points: dist2 / nn_idx in cell order,
 * outputs (out, tap_out, in_tap) written to the ORIGINAL rows; values bit-identical to the un-sorted pair of calls.  A workgroup's rows
 * are then spatial neighbours and the three table rows each of them gathers hit in L1 (interpolate_gpu.cu:77-117 + the first SharedMLP
 * layer of pointnet2_modules.py:127-156). */
int g4d_three_nn_cells_sorted_f32(int b, int n, int m, const void *unknown_grid, const float *known, float *dist2, int *idx, g4d_stream_t stream);

/* three_nn with exact block pruning (round 5; csrc/three_nn_prune.hip; replaces interpolate_gpu.cu:9-74 for well-spread known sets of up to
 * 1024 points -- the last feature-propagation level).  A pre-pass Morton-sorts each cloud's known points into blocks of 16 with bounding
 * boxes (workspace `ws`); a wave of 64 queries (cell order of `unknown_grid` when given, else index order of `unknown`) visits only the
 * blocks whose box -- tested with the same fp32 distance expression, whose rounding is monotone -- can still hold one of some lane's three
 * nearest, ties included; inserts order by (distance, original index).  Output identical to g4d_three_nn_f32 (sorted_out = 0) or to
 * g4d_three_nn_cells_sorted_f32 (sorted_out != 0, needs unknown_grid) for any input.  16 <= m <= 1024, b <= 65535;
 * ws >= g4d_three_nn_pruned_ws_bytes(b) bytes, 16-byte aligned, owned by the caller. */
int g4d_three_nn_pruned_supported(int n, int m);
long long g4d_three_nn_pruned_ws_bytes(int b);
int g4d_three_nn_pruned_f32(int b, int n, int m, const float *unknown, const void *unknown_grid, const float *known, float *dist2, int *idx,
                            int sorted_out, void *ws, long long ws_bytes, g4d_stream_t stream);
int g4d_mlp_chain_table_cells_f32(long long rows, int n, int m, int C2, const float *table, const float *dist2, const int *nn_idx,
                                  const void *unknown_grid, const float *pre_scale, const float *pre_shift, float *in_tap, int in_tap_ld,
                                  int nlayers, const float *const *W, const float *const *scale, const float *const *shift, const int *Kpad,
                                  const int *Cout, const int *relu, float *out, int ldo, int col0, int tap_layer, float *tap_out, int tap_ld,
                                  g4d_stream_t stream);

/* g4d_ball_query_msg2_f32 + g4d_three_nn_multi_f32 (1..4 problems) of the same batch in ONE launch: the searches of the encoder's inner
 * levels depend on the sampled coordinates only.  Outputs identical to the separate calls' (ball_query_gpu.cu:9-45, interpolate_gpu.cu:9-52). */
int g4d_search_multi_f32(int b, int nscales, int n0, int m0, const float *radii0, const int *nsamples0, const float *new_xyz0, const float *xyz0,
                         int *const *idx0, int n1, int m1, const float *radii1, const int *nsamples1, const float *new_xyz1, const float *xyz1,
                         int *const *idx1, int nn_count, const int *nn_n, const int *nn_m, const float *const *nn_unknown,
                         const float *const *nn_known, float *const *nn_dist2, int *const *nn_idx, g4d_stream_t stream);

/* ---- launch groups (round 3) --------------------------------------------------------------------------------------------------
 * Independent register-chain stacks (g4d_mlp_chain_f32 and its table variants) called between g4d_launch_group_begin() and
 * g4d_launch_group_end() on the same host thread are RECORDED instead of launched; _end() puts them on `stream` as ONE kernel launch
 * when a merged kernel is instantiated for the combination (the two scales of an MSG set-abstraction level: workgroups [0, nb0) run
 * the heavier stack, the rest the other one), else as one launch each, in the recorded order.  Results are bit-identical to the
 * separate launches either way.  Why: a launch costs the many-streams regime ~2.4 us of serialised dispatch on top of its own ramp
 * and tail (scripts/exp_dispatch.py).  The recorded calls must not depend on each other's outputs.  *launches (may be NULL) receives
 * the number of kernel launches _end() issued.  G4D_LAUNCH_GROUPS=0 turns merging off.  _abort() drops an open group. */
int g4d_launch_group_begin(void);
int g4d_launch_group_end(g4d_stream_t stream, int *launches);
int g4d_launch_group_abort(void);

/* g4d_fps_gather_f32 (no scratch) AND g4d_ball_grid_build_f32 of the same b clouds: for 4096 < n <= 8192 one launch -- workgroups [b, 2 b) of
 * the sampling launch build the cell grids (both depend on the cloud only; the build hides behind the sampling) -- two launches otherwise.
 * idx (b, m), new_xyz (b, m, 3), grid (g4d_ball_grid_bytes(b, n) bytes): identical to the two calls' outputs. */
int g4d_fps_gather_grid_f32(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, float rmax, void *grid, g4d_stream_t stream);

/* The whole lbs() in ONE launch (csrc/lbs.hip lbs_one_kernel): a workgroup owns 64 vertices x up to 8 frames; its 8 waves request
 * the tile's blend rows up front, do the per-frame work (Rodrigues, joints, coefficients, kinematic chain) while those loads fly,
 * meet in LDS and skin.  Same constants and outputs as g4d_lbs_fused_f32, no scratch.  Supported when J <= 32 and
 * NB + 9 (J - 1) <= 224 (g4d_lbs_one_supported; SMPL: 24 joints, 10 betas). */
int g4d_lbs_one_supported(int j, int nb);
int g4d_lbs_one_f32(int b, int v, int j, int nb, int pose2rot, const float *betas, int betas_bstride, const float *pose,
                    const float *v_template, const float *blend_dirs, const float *J_template, const float *J_shapedirs,
                    const int *parents, const float *lbs_weights, float *A_out, float *posed_joints, float *verts,
                    g4d_stream_t stream);

/* lbs() on the matrix pipe (round 5; csrc/lbs.hip lbs_frame_kernel + lbs_mfma_kernel), same constants and outputs as g4d_lbs_one_f32
 * (replaces smplx/smplx/lbs.py:152-248 for a batch of frames).  Launch 1, one wave per frame, ONCE per frame: Rodrigues, joints
 * from betas, kinematic chain -> A_out, posed_joints and the B operands of the two GEMMs (fragment order) in `ws`.  Launch 2, a workgroup per
 * 32 vertices: their blend rows (NC x 96 floats, 86 KB) in LDS, read from HBM once per launch; per (16-frame tile, 16-vertex half)
 * v_posed^T and T^T = (W . A)^T as fp32 MFMA tiles (vertices x frames), so a lane ends with the posed vertex and the full 3x4 transform of the
 * same four (vertex, frame) pairs.  Every output element is one accumulator chain over k ascending: a frame's bits do not depend on the batch.
 * ws: device memory, 16-byte aligned, >= g4d_lbs_mfma_ws_bytes(b, j) bytes, owned by the caller.  Supported when J <= 32, NB + 9 (J - 1) <= 224. */
int g4d_lbs_mfma_supported(int j, int nb);
long long g4d_lbs_mfma_ws_bytes(int b, int j);
int g4d_lbs_mfma_f32(int b, int v, int j, int nb, int pose2rot, const float *betas, int betas_bstride, const float *pose,
                     const float *v_template, const float *blend_dirs, const float *J_template, const float *J_shapedirs,
                     const int *parents, const float *lbs_weights, float *A_out, float *posed_joints, float *verts, void *ws,
                     long long ws_bytes, g4d_stream_t stream);

/* ---- callers around the hot path ---------------------------------------------- */

/* K nearest neighbours, K <= 256: for every query (B,P1,3) the K points of (B,P2,3) that are smallest under
 * (squared distance, index), ascending.  dists (B,P1,K) fp32 squared L2, idx (B,P1,K) int32.  Stands in for the
 * un-vendored chamferdist.knn_points used by modules/mesh_encoder.py:321-324 (parity unpinned: dependency absent). */
int g4d_knn_f32(int b, int p1, int p2, int k, const float *queries, const float *points, float *dists, int *idx,
                g4d_stream_t stream);

/* Inverse-distance blend of the K nearest body vertices' skinning weights (modules/mesh_encoder.py:339-347, 374-382):
 * out (F,Vg,J) = sum_k w_k W[f, idx[c,v,k], :],  c = f / frames_per_clip,  w = normalised 1/d with the reference's two
 * "inf -> 0" fix-ups.  W (F,V,J); idx / dists (F/frames_per_clip, Vg, K) from g4d_knn_f32.  K <= 256, J <= 64. */
int g4d_knn_blend_weights_f32(int frames, int frames_per_clip, int vg, int v, int k, int j, const float *W, const int *idx,
                              const float *dists, float *out, g4d_stream_t stream);

/* Nearest-vertex two-stage garment skinning of the MGN model variant (modules/mesh_encoder.py:529-585, csrc/mgn_skin.hip), one launch.
 * F = clips * frames_per_clip frames, clip c = f / frames_per_clip.  Per (frame f, garment vertex g):
 *   q  = garment[f,g] + root[c]                                  (one fp32 add)
 *   nn = the nearest of tpose[c, 0..V-1] to q: index and squared distance equal g4d_knn_f32(K = 1) on the same q bit for bit, in
 *        every distance-contraction mode (same rounding, same (distance, index) order: ties go to the lowest index)
 *   s  = M_inv[:3,:3] q + M_inv[:3,3],  M_inv = sum_j W[f,nn,j] inv_A[f,j]      (stage 1: the un-posed garment)
 *   p  = M[:3,:3] s + M[:3,3],          M     = sum_j W[f,nn,j] A[f,j]          (posed)
 * Summation order: every entry of M_inv / M is acc = fma(W[f,nn,j], T_j[r][k], acc) for j = 0, 1, ..., J-1 from acc = 0; the row
 * products are fma(M[r][2], z, fma(M[r][1], y, fma(M[r][0], x, M[r][3]))).  Only the nearest vertex's row of W is read.
 * garment (F,Vg,3); root (clips,3); tpose (clips,V,3); W (F,V,J); inv_A, A (F,J,4,4), 16-byte aligned.
 * Outputs: nn_idx (F,Vg) int32, nn_dist (F,Vg), stage1 (F,Vg,3), posed (F,Vg,3).  Any V >= 1 (the T-pose streams through LDS in
 * tiles), 1 <= J <= 64, any Vg and frames_per_clip; nothing is launched when clips, frames_per_clip or Vg is 0. */
int g4d_mgn_skin_f32(int clips, int frames_per_clip, int vg, int v, int j, const float *garment, const float *root, const float *tpose,
                     const float *W, const float *inv_A, const float *A, int *nn_idx, float *nn_dist, float *stage1, float *posed,
                     g4d_stream_t stream);

/* Adjoint of g4d_mgn_skin_f32 with respect to `garment` for a FIXED nearest index (csrc/mgn_skin_grad.hip), one launch: what MGN training
 * (train_temporal.py --MGN 1) needs to carry the loss gradient from the posed garment back to the displacement MLP.  The index is a
 * piecewise-constant function of the input; torch's autograd treats it as a constant in the reference too (knn_points(...).idx, torch.gather).
 * Per (frame f, garment vertex g), nn = nn_idx[f,g] CLAMPED into [0, V-1] (a stale index gives a wrong number, never an out-of-range read):
 *   M_inv = sum_j W[f,nn,j] inv_A[f,j],  M = sum_j W[f,nn,j] A[f,j]     (the 3x3 parts only: the translation columns and `root` drop out)
 *   t           = M[:3,:3]^T d_posed[f,g] + d_stage1[f,g]               (d_stage1 == NULL: zero)
 *   d_garment[f,g] = M_inv[:3,:3]^T t
 * Summation order: every entry of M_inv / M as in the forward, acc = fma(W[f,nn,j], T_j[r][k], acc) for j = 0, 1, ..., J-1 from acc = 0;
 * the transposed products are  t[k] = fma(M[2][k], d2, fma(M[1][k], d1, fma(M[0][k], d0, d_stage1[k])))  and
 * d_garment[k] = fma(M_inv[2][k], t2, fma(M_inv[1][k], t1, M_inv[0][k] * t0)).  No atomics: every output element is written once by one
 * thread, so two runs give the same bits.  The forward stores nothing for this: both blends are recomputed.
 * nn_idx (F,Vg) int32 (the forward's output); W (F,V,J); inv_A, A (F,J,4,4), 16-byte aligned; d_posed, d_stage1, d_garment (F,Vg,3).
 * Same domain as the forward: any V >= 1, 1 <= J <= 64, any Vg and frames_per_clip; nothing is launched when clips, frames_per_clip or
 * Vg is 0. */
int g4d_mgn_skin_grad_f32(int clips, int frames_per_clip, int vg, int v, int j, const int *nn_idx, const float *W, const float *inv_A,
                          const float *A, const float *d_posed, const float *d_stage1 /* may be NULL: zero */, float *d_garment,
                          g4d_stream_t stream);

/* One Jacobi smoothing step of the blended weights over the garment mesh (modules/mesh_encoder.py:385-390):
 * out (F,Vg,C) = S + coeff * (adj (CSR) . S).  out must not alias S (ping-pong two buffers for the 100 steps). */
int g4d_spmm_axpy_rows_f32(int frames, int vg, int c, const float *S, const int *rowptr, const int *colidx,
                           const float *vals, float coeff, float *out, g4d_stream_t stream);

/* ALL `iters` smoothing steps of mesh_encoder.py:385-390 in one launch: the (vg x 4-column) slab of a frame stays in LDS for the
 * whole iteration, adjacency rows in registers; HBM sees the weights once in and once out.  Bit-identical to `iters` calls of
 * g4d_spmm_axpy_rows_f32.  adj = D^-1 A - I in CSR (device arrays); max_row_entries = the longest CSR row (host-side knowledge of
 * the caller).  Needs vg <= 5104 and max_row_entries <= 8, else G4D_EINVAL (use the per-step entry point).  S and out may alias. */
int g4d_jacobi_smooth_f32(int frames, int vg, int c, int iters, float coeff, int max_row_entries, const float *S, const int *rowptr,
                          const int *colidx, const float *vals, float *out, g4d_stream_t stream);

/* One positional encoder of the refinement loop (modules/mesh_encoder.py:452-464): for every query q of new_xyz
 * (frames,p,3) and its nsample ball-query hits j = idx (frames,p,nsample) in xyz (frames,n,3):
 *   h = relu(W1 [x_j - q ; extra_j] + b1 + table_j),   y = W2 h + b2,   out[f*p + q, col0 .. col0+32) = max_j y
 * extra (frames,n,n_extra) or NULL (n_extra = 0); table (frames,n,32) or NULL: per-source-point part of the first
 * Linear (Wf f_j + b, see garment4d_amd/refine.py); W1 (32, 3+n_extra) row-major; b1 (32) or NULL (then table must be
 * given); W2_frag: the 32x32 second Linear in the fragment order of g4d_mlp_stack_f32; b2 (32).  nsample in
 * {4,8,16,32,64}.  Hidden and output width are the reference's feat_num = 32. */
int g4d_pos_encode_f32(int frames, int n, int p, int nsample, int n_extra, const float *xyz, const float *new_xyz,
                       const float *extra, const float *table, const int *idx, const float *W1, const float *b1,
                       const float *W2_frag, const float *b2, float *out, int ldo, int col0, g4d_stream_t stream);

/* Temporal attention of a refinement round (modules/mesh_encoder.py:467-476) for nclips clips of t <= 32 frames:
 * qkv (nclips*t, vg, 3c) = temporal_qkv(last_feat), [q | k | v] per vertex;  att (nclips, t, t) = softmax over the last axis
 * of q k^T / sqrt(t) with q, k flattened over (vg, c);  out[(clip*t + frame), vertex, col0 .. col0+c) = att v, row stride
 * ldo floats per vertex.  scratch: g4d_temporal_attention_scratch_floats(nclips, vg, c) floats.  c % 16 == 0. */
size_t g4d_temporal_attention_scratch_floats(int nclips, int vg, int c);
int g4d_temporal_attention_f32(int nclips, int t, int vg, int c, const float *qkv, float *scratch, float *att, float *out, int ldo,
                               int col0, g4d_stream_t stream);

/* Backward of g4d_pos_encode_f32 (same shape domain, same operands; W2 here is the second Linear's weight ROW-MAJOR (32,32), not in fragment
 * order).  dOut: the gradient of the encoder's 32 output columns, read at dOut[(f*p + q)*ldg + col0 .. +32).  The forward is recomputed per
 * query; per channel the gradient goes to the first sample that attains the maximum.  Every output pointer may be NULL ("nobody needs it":
 * its work is skipped):
 *   dW1 (32, 3+n_extra), db1 (32), dW2 (32,32), db2 (32): written; reduced without atomics (one partial per workgroup in ws, summed in a
 *     fixed order): bit-reproducible.  ws: g4d_pos_encode_grad_ws_bytes(frames, p, nsample) bytes, needed when any of the four is asked for.
 *   d_new_xyz (frames,p,3): written, one value per query, no atomics.
 *   d_xyz (frames,n,3), d_extra (frames,n,n_extra), d_table (frames,n,32): fp32 atomic scatter-ADDS into the source-point rows; the caller
 *     zero-fills them (or passes a buffer to accumulate into).  With a table, db1 is the caller's column sum of d_table. */
long long g4d_pos_encode_grad_ws_bytes(int frames, int p, int nsample);
int g4d_pos_encode_grad_f32(int frames, int n, int p, int nsample, int n_extra, const float *xyz, const float *new_xyz,
                            const float *extra, const float *table, const int *idx, const float *W1, const float *b1,
                            const float *W2, const float *dOut, int ldg, int col0, float *ws, float *dW1, float *db1, float *dW2,
                            float *db2, float *d_new_xyz, float *d_xyz, float *d_extra, float *d_table, g4d_stream_t stream);

/* Backward of g4d_temporal_attention_f32: qkv and att as the forward read / wrote them, dO the gradient of its output read at
 * dO[((clip*t + frame)*vg + vertex)*ldg + col0 .. +c);  dqkv (nclips*t, vg, 3c) = [dQ | dK | dV] in the layout of qkv, fully written.
 * dA = dO V^T, dS = A (dA - rowsum(dA A)) / sqrt(t), dQ = dS K, dK = dS^T Q, dV = A^T dO.  No atomics: bit-reproducible.
 * scratch: g4d_temporal_attention_grad_scratch_floats(nclips, vg, c) floats. */
size_t g4d_temporal_attention_grad_scratch_floats(int nclips, int vg, int c);
int g4d_temporal_attention_grad_f32(int nclips, int t, int vg, int c, const float *qkv, const float *att, const float *dO, int ldg,
                                    int col0, float *scratch, float *dqkv, g4d_stream_t stream);

/* Ordered per-frame compaction of `calc_segmentation_results` (modules/mesh_encoder.py:109-125): sel (frames,n_out) = the
 * indices k (ascending) of the points whose arg-max over `classes` logits (first maximum wins) equals `target`, the
 * first n_out of them, -1 padded; counts (frames, may be NULL) = number of matching points (may exceed n_out).
 * logits (frames,n,classes) point-major. */
int g4d_segment_select_f32(int frames, int n, int classes, int target, int n_out, const float *logits, int *sel, int *counts,
                           g4d_stream_t stream);

/* out (frames,n_out,c) = in (frames,n,c)[sel], zero rows where sel < 0 (the torch.cat with zeros, mesh_encoder.py:123-124). */
int g4d_segment_take_f32(int frames, int n, int n_out, int c, const float *in, const int *sel, float *out, g4d_stream_t stream);

/* Vertex normals (utils/mesh_utils.py:116-134 compute_fnorms + compute_vnorms): unit face normals (norm clamped at 1e-6)
 * summed over each vertex's incident faces in the CSR order (vf_rowptr (v+1), vf_fid), re-normalised with the same
 * clamp.  verts/out (frames,v,3); faces (nf,3) int32. */
int g4d_vertex_normals_f32(int frames, int v, const float *verts, const int *faces, const int *vf_rowptr, const int *vf_fid,
                           float *out, g4d_stream_t stream);

/* Per-vertex interpenetration penalty (smplx/loss/temporal_loss.py:20-46, forward): pen (frames,vg) =
 * relu(-(n_b . (g - b))) with b = body[f, nn_idx[(f*vg + i) * idx_stride]] the nearest body vertex of garment vertex i and
 * n_b its unit normal.  garment (frames,vg,3); body / normals (frames,v,3); nn_idx int32 with idx_stride ints per
 * garment vertex (3 for the output of g4d_three_nn_f32, whose first column is the nearest vertex). */
int g4d_interpenetration_f32(int frames, int vg, int v, const float *garment, const float *body, const float *normals,
                             const int *nn_idx, int idx_stride, float *pen, g4d_stream_t stream);

/* The stage-2 objective of the refinement head for ONE round's prediction (smplx/loss/temporal_loss.py:147-201; csrc/refine_loss.hip):
 * pred / target (nbatch*t, vg, 3); body / normals (nbatch*t, v, 3); nn_idx int32 with idx_stride ints per garment vertex, the first being the
 * nearest body vertex (the output of g4d_three_nn_f32: idx_stride 3).  (rowptr, colidx, vals): CSR of the Laplacian L = I - D^-1 A (vg rows,
 * any row length), rowsum (vg) its row sums (float64 sums of the fp32 entries, rounded); (rowptr_t, colidx_t, vals_t): CSR of L^T, needed
 * only for the gradient of the Laplacian term.  out (5) = [mean |p-g|^2, mean |p-g|, mean |(L p)_i|, mean relu(-n_b.(p-b)),
 * temporal != 0 && t > 1 ? mean over (clip, frame < t-1, vertex) of |p_f - p_{f+1}| : 0];  msre_frames (nbatch*t) or NULL: mean |p-g| per frame.
 * grad (nbatch*t, vg, 3) or NULL (values only): fully written with
 *   w_l2 d out[0] + w_lap d out[2] + w_pen d out[3] + w_temporal d out[4]  w.r.t. pred;
 * a zero |(L p)_i| or |p_f - p_{f+1}| contributes zero (the reference's sqrt gives NaN for the latter).  A weight of 0 leaves its value
 * reported.  No atomics: the sums go through per-workgroup partials in ws (g4d_refine_loss_ws_bytes(nbatch*t, vg, grad != NULL) bytes; with a
 * gradient it also stages u = L p / |L p|) and are added in an order that depends on the shape alone (the tree is written out in
 * csrc/refine_loss.hip): two runs give the same bits.  nbatch*t == 0 or vg == 0: out = zeros, nothing else is touched. */
long long g4d_refine_loss_ws_bytes(int frames, int vg, int with_grad);
int g4d_refine_loss_f32(int nbatch, int t, int vg, int v, const float *pred, const float *target, const float *body, const float *normals,
                        const int *nn_idx, int idx_stride, const int *rowptr, const int *colidx, const float *vals, const float *rowsum,
                        const int *rowptr_t, const int *colidx_t, const float *vals_t, float w_l2, float w_lap, float w_pen, float w_temporal,
                        int temporal, float *ws, float *out, float *msre_frames, float *grad, g4d_stream_t stream);

/* The stage-1 objective of the garment encoder (smplx/loss/temporal_loss.py:60-119 `temporal_loss_PCA`; csrc/stage1_loss.hip, which writes
 * out the arithmetic and the reduction trees).  No atomics; the order of every sum depends on the shape alone: two runs give the same bits,
 * with or without gradient buffers.
 *
 * g4d_stage1_loss_ws_bytes: the workspace of either entry point, or of both when they share one buffer one after the other:
 *   4 * (ceil(ce_rows / 256)  +  [b > 0 && vg > 0] (b ceil(vg / 256) 4 + 2 b nf 3 + [with_grad] b vg 3)).
 *
 * g4d_stage1_ce_f32: out (1) = the mean over `rows` rows of  log sum_c exp(x_c) - x_label  (torch's CrossEntropyLoss(), mean), logits
 * (rows, classes) row-major, 1 <= classes <= 64, labels int64.  grad (rows, classes) or NULL (value only): fully written with
 * w_sem d out[0] / d logits = (w_sem / rows) (softmax - onehot).  A label outside [0, classes) is never used as an index: out[0] is NaN and
 * the row's gradient zero (torch's ignore_index would drop the row from the mean; not implemented).  rows may exceed 2^31 - 1 (64-bit
 * offsets).  ws: g4d_stage1_loss_ws_bytes(rows, 0, 0, 0, 0) bytes.  rows == 0: out = 0, nothing else is touched.
 *
 * g4d_stage1_garment_f32: pred / target (b, vg, 3) the predicted T-pose garment and its target; root (b, 3) added to pred for the
 * penetration term; body / normals (b, v, 3); nn_idx int32 with idx_stride ints per garment vertex, the first being the nearest body vertex
 * of pred + root (the output of g4d_three_nn_f32: idx_stride 3); faces (nf, 3) int32 triangles over the vg vertices; (inc_rowptr (vg + 1),
 * inc) the vertex -> incidence CSR, each entry = face * 3 + corner with faces[entry] == the vertex; coeff / coeff_gt (b, pdim).
 * out (5) = [mean |p-g|^2, mean |p-g|, mean relu(-n_b.(p+root-b)), the one-time cotangent-Laplacian term
 * mean_{item < bp, i} | |(L(p) p)_i| - |(L(g) g)_i| | with the items b..bp-1 being copies of item 0 (a weight 1 + bp - b on item 0; nothing is
 * copied), mean (coeff - coeff_gt)^2].  grad_pred (b, vg, 3) or NULL: fully written with w_l2 d out[0] + w_pen d out[2] + w_lap d out[3]
 * w.r.t. pred, L held constant as in the reference's backward; a face of zero area has zero cotangents, a vertex with |(L p)_i| = 0 or
 * = |(L g)_i| contributes zero.  grad_coeff (b, pdim) or NULL: w_pca d out[4] / d coeff.  A weight of 0 leaves its value reported.
 * ws: g4d_stage1_loss_ws_bytes(0, b, vg, nf, grad_pred != NULL) bytes.  b == 0 or vg == 0: out = zeros, nothing else is touched. */
long long g4d_stage1_loss_ws_bytes(long long ce_rows, int b, int vg, int nf, int with_grad);
int g4d_stage1_ce_f32(long long rows, int classes, const float *logits, const long long *labels, float w_sem, float *ws, float *out, float *grad,
                      g4d_stream_t stream);
int g4d_stage1_garment_f32(int b, int bp, int vg, int v, int nf, int pdim, const float *pred, const float *target, const float *root,
                           const float *body, const float *normals, const int *nn_idx, int idx_stride, const int *faces, const int *inc_rowptr,
                           const int *inc, const float *coeff, const float *coeff_gt, float w_pca, float w_l2, float w_pen, float w_lap, float *ws,
                           float *out, float *grad_pred, float *grad_coeff, g4d_stream_t stream);

/* ---- garment post-processing (utils/post_processing.py:145-228, :299-319): Taubin smoothing and depenetration --------------------------------
 * What the reference runs on the CPU, one frame at a time, on the last refinement round before it shows a mesh (psbody AABB tree +
 * scipy spsolve).  psbody is third-party code that cannot be run here: the definitions below are the contract ("Unpinned").
 * All fp32, point-major, on `stream`; no atomics, every reduction order fixed by the shapes (two runs give the same bits); nothing is read back
 * to the host.  `frame_active` (frames) int32 or NULL, where it appears: a frame with frame_active[f] == 0 is skipped and its outputs are left
 * untouched (depenetration hands the previous round's counts in: a frame without a flagged vertex is finished for good).
 *
 * g4d_taubin_smooth_f32: `iters` steps  S <- S + c_it * (adj . S),  c_it = lam for even it, mu for odd it (:302-309: lam 0.05, mu -0.052,
 * 100 steps), adj = D^-1 A - I in CSR, in one launch with the (vg x 4-column) slab of a frame in LDS -- g4d_jacobi_smooth_f32's domain
 * (vg <= 5104, max_row_entries <= 8, else G4D_EINVAL) and arithmetic: bit-identical to `iters` alternating g4d_spmm_axpy_rows_f32 calls.
 * S and out may alias. */
int g4d_taubin_smooth_f32(int frames, int vg, int c, int iters, float lam, float mu, int max_row_entries, const float *S, const int *rowptr,
                          const int *colidx, const float *vals, float *out, g4d_stream_t stream);

/* Area-weighted unit vertex normals (psbody VertNormals): out (frames,v,3) = s / |s| with s = the sum over the incident faces, in the order of
 * the (vf_rowptr, vf_fid) CSR, of the SCALED face normals (v1 - v0) x (v2 - v0); |s| = sqrt((sx^2 + sy^2) + sz^2), no fused operation.
 * NOT g4d_vertex_normals_f32, which sums UNIT face normals.  Deviation: |s| == 0 (an isolated vertex, or faces that cancel) yields the zero
 * vector where the division would give NaN. */
int g4d_vertex_normals_area_f32(int frames, int v, const float *verts, const int *faces, const int *vf_rowptr, const int *vf_fid,
                                const int *frame_active, float *out, g4d_stream_t stream);

/* Nearest point on a triangle mesh, per frame.  faces (nf,3) in ANY order (the caller sorts them once per topology so that 64 consecutive
 * faces are close together; face_ids (nf) = the index each row has in the caller's own face list, which is what `face` reports and what
 * breaks ties).  g4d_mesh_aabb_f32 writes boxes (frames, ceil(nf / 64), 6) = {lo xyz, hi xyz} of every block of 64 faces, padded per axis by
 * 2^-18 * max(|lo|, |hi|); g4d_mesh_nearest_f32 needs them (also with cull == 0) and vnormals (frames,v,3) = g4d_vertex_normals_area_f32.
 *
 * Per query q (points (frames,p,3)): the triangle with the smallest dist2, ties to the lowest face id; with a, b, c its corners,
 *   dot(u, w) = fmaf(u.z, w.z, fmaf(u.y, w.y, u.x * w.x));   every other operation below is a single rounded fp32 operation, never fused
 *   ab = b - a, ac = c - a;  d1 = dot(ab, q - a), d2 = dot(ac, q - a), d3 = dot(ab, q - b), d4 = dot(ac, q - b), d5 = dot(ab, q - c), d6 = dot(ac, q - c)
 *   vc = d1 * d4 - d3 * d2,  vb = d5 * d2 - d1 * d6,  va = d3 * d6 - d5 * d4,  e43 = d4 - d3,  e56 = d5 - d6
 *   part = first that holds of:  4 (vertex a): d1 <= 0 && d2 <= 0;   5 (vertex b): d3 >= 0 && d4 <= d3;   1 (edge ab): vc <= 0 && d1 >= 0 && d3 <= 0;
 *          6 (vertex c): d6 >= 0 && d5 <= d6;   3 (edge ca): vb <= 0 && d2 >= 0 && d6 <= 0;   2 (edge bc): va <= 0 && e43 >= 0 && e56 >= 0;   else 0 (interior)
 *   den = (va + vb) + vc | d1 - d3 | e43 + e56 | d2 - d6   for part 0 | 1 | 2 | 3,   r = 1 / den
 *   w = vc * r | e43 * r | d2 * r | 1   for part 0 | 2 | 3 | 6, else 0;     v = vb * r | d1 * r | 1 - w | 1   for part 0 | 1 | 2 | 5, else 0
 *   point = (a + ab * v) + ac * w;   dist2 = (dx * dx + dy * dy) + dz * dz  with  d = q - point
 *   normal: part 0: n = ab x ac, n / sqrt((nx^2 + ny^2) + nz^2) (zero when that length is 0); part 4 / 5 / 6: vnormals of a / b / c;
 *           part 1 / 2 / 3: vnormals of (a, b) / (b, c) / (c, a) added;  then divided by (its length + 1e-10)  (:175).
 * A zero-area triangle gives a NaN dist2 and never wins; a mesh of nothing else reports face = part = -1, dist2 = inf, point = NaN, normal = 0.
 * cull != 0: a wave of 64 queries skips a block of faces whose box is farther from every one of its queries than that query's best so far
 * ((1 - 2^-18) * gap^2 > best): conservative, so cull 0 and 1 give the same bits.  visited (frames * ceil(p / 64)) int32 or NULL: the number of
 * face blocks each wave went through (a measurement aid). */
int g4d_mesh_aabb_f32(int frames, int v, int nf, const float *verts, const int *faces, float *boxes, g4d_stream_t stream);
int g4d_mesh_nearest_f32(int frames, int p, int v, int nf, int cull, const float *points, const float *verts, const int *faces,
                         const int *face_ids, const float *boxes, const float *vnormals, const int *frame_active, float *point, float *dist2,
                         int *face, int *part, float *normal, int *visited, g4d_stream_t stream);

/* One depenetration round (:179-228), after (near_p, near_n) = g4d_mesh_nearest_f32(verts, body) and garment_n = g4d_vertex_normals_area_f32:
 * g4d_depen_targets_f32, per garment vertex i (products and sums left to right, nothing fused):
 *   flagged = ((v - p) . n) < 0;   s = sign(m . n) (may be 0);   d = (p - v) * s;
 *   flagged:  target = p + (eps * d) / (1e-4 + |d|),  w2 = ww * ww;    otherwise:  target = v,  w2 = 1;      counts[f] = number flagged.
 * g4d_depen_solve_f32: out = x after exactly cg_iters conjugate-gradient steps from x0 = verts on
 *   (L^T L + diag(w2)) x = L^T L verts + w2 * target
 * per frame and coordinate (one workgroup each; dot products by a fixed tree over the workgroup), L given as CSR with its transpose,
 * vg <= 5104 and <= 8 entries per row of either (else G4D_EINVAL).  residual (frames,3) = |b - M x|_2 / |b|_2 at exit, from a fresh product.
 * A frame with counts[f] == 0 is copied through bit for bit with residual 0 (the reference solves once more and gets verts back up to
 * rounding).  Error after k steps <= 2 ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k in the M-norm, kappa <= ww^2 + |L|_2^2 (M >= I). */
int g4d_depen_targets_f32(int frames, int vg, float eps, float ww, const float *verts, const float *near_p, const float *near_n,
                          const float *garment_n, const int *frame_active, float *w2, float *target, int *counts, g4d_stream_t stream);
int g4d_depen_solve_f32(int frames, int vg, int cg_iters, int max_row_entries, int max_row_entries_t, const float *verts, const float *w2,
                        const float *target, const int *counts, const int *rowptr, const int *colidx, const float *vals, const int *rowptr_t,
                        const int *colidx_t, const float *vals_t, float *out, float *residual, g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_H */

/*
 * oracle/g4d_oracle.c -- CPU restatement of the reference's `pointnet2_cuda` kernels.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under garment4d_amd/ may import, link or call this
 * file; only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use it, and only
 * as the checker / the timed CPU baseline.
 *
 * Every function follows one reference kernel line by line (file:line given per function,
 * relative to modules/pointnet2/pointnet2/src/).  Arithmetic is IEEE fp32.  The one
 * expression whose rounding decides INDICES -- the squared distance of FPS, ball query and three_nn,
 *     d = (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1)      sampling_gpu.cu:136, ball_query_gpu.cu:30,
 *                                                                  interpolate_gpu.cu:33
 * -- is evaluated under a selectable CONTRACTION mode (g4d_oracle_set_contraction, same numbering as
 * include/g4d.h G4D_CONTRACT_*), because the reference is built by `nvcc -O2` (setup.py:19-20), whose default
 * -fmad=true contracts it:
 *   1 (default) fmaf(dz,dz, fmaf(dx,dx, dy*dy))  the LLVM/NVVM DAG-combiner contraction: of the two products of the
 *               first sum the LEFT one is fused (fold (fadd (fmul a,b), c) -> fma a,b,c), the third product is fused
 *               into the second sum.  clang and gcc in this container emit exactly this shape for the expression
 *               with -ffp-contract=fast (vmulss y; vfmadd x; vfmadd z) -- see DESIGN.md "Numerics contract";
 *   0           every product and sum rounded (a reference built with -fmad=false);
 *   2           fmaf(dz,dz, fmaf(dy,dy, dx*dx))  the other pairing / the accumulate-loop shape of chamferdist's knn.
 * This file is built with -ffp-contract=off, so the only fused operations are the explicit fmaf() calls.
 *
 * PARITY PINNING: the reference ships no tests or golden vectors for its native kernels, but its four kernel files hold
 * nothing CUDA-specific, and `make -C oracle ref` compiles them AS THEY ARE for gfx950 (hipcc -O2 -ffp-contract=off, four
 * shadow headers of our own under ref_shim/, C entry points in ref_entry.hip) into _ref/libpointnet2_ref.so.
 *   PINNED: the reference's own kernel source, executed on an MI355X, against this file in mode 0 (`off`) and against the
 *   product in mode `off`, bit for bit, for all nine ops -- tests/test_ref_kernels_gpu.py (live, where _ref/ was built) and
 *   tests/golden/ops_ref_hip_off.npz (its recorded outputs; tests/test_ref_kernels_cpu.py holds this file to them on any
 *   machine): the block-size-dependent tie-break of the FPS tree, opt_n_threads() for every n up to 40000, the temp in/out
 *   contract, the ball query's fill-with-the-first-hit and cnt handling, the strict `<` cascade and 1e40 sentinels of
 *   three_nn, NaN / inf coordinates, the three scatter-add backwards on exactly summable inputs.  No case disagreed.
 *   NOT PINNED: which multiply-adds `nvcc -O2` fuses in the squared distance -- mode 1 stays an assumption until somebody
 *   supplies tests/golden/ops_cuda.npz (tests/test_cuda_pin.py).  hipcc's own default contraction of that expression (two
 *   rounded products, one fma, one rounded add) is NONE of the three modes, which is why the reference build must be, and
 *   is, compiled with -ffp-contract=off and held to mode 0 only.
 * The index goldens in tests/golden/ops*.npz remain THIS file's output routed through the reference's Python wrappers (a
 * regression pin); the reference's own Python layer (pointnet2_utils / pointnet2_modules / lbs / GraphConvolution) executed on
 * top of these kernels is pinned by the rest of tests/golden/.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifdef _OPENMP
#include <omp.h>
#endif

/* cuda_utils.h:10-14  opt_n_threads(): 2^floor(log2(work_size)) clamped to [1, 1024],
 * computed through double log() exactly as the reference does. */
int g4d_oracle_block_size(int work_size) {
    const int pow_2 = (int)(log((double)work_size) / log(2.0));
    int v = 1 << pow_2;
    if (v > 1024) v = 1024;
    if (v < 1) v = 1;
    return v;
}

static int g_contract = 1; /* G4D_CONTRACT_NVCC */
void g4d_oracle_set_contraction(int mode) { g_contract = mode < 0 ? 0 : (mode > 2 ? 2 : mode); }
int g4d_oracle_get_contraction(void) { return g_contract; }

/* squared distance of the three coordinate differences under contraction shape `fm` (see header) */
static inline float dist2c(int fm, float dx, float dy, float dz) {
    if (fm == 0) return dx * dx + dy * dy + dz * dz;
    if (fm == 1) return fmaf(dz, dz, fmaf(dx, dx, dy * dy));
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

/* pairwise squared distances (b, p1, p2) under shape `fm`: the arithmetic of chamferdist / pytorch3d knn
 * (`dist += diff * diff` over the axes -> shape 2 under nvcc contraction, shape 0 without); used by
 * oracle/refine_oracle.knn_points so that numpy never has to emulate an fma. */
void g4d_oracle_pairwise_d2(int fm, int b, int p1, int p2, const float *q, const float *x, float *out) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int bi = 0; bi < b; ++bi)
        for (int i = 0; i < p1; ++i) {
            const float *qp = q + ((size_t)bi * p1 + i) * 3;
            const float *xp = x + (size_t)bi * p2 * 3;
            float *o = out + ((size_t)bi * p1 + i) * p2;
            for (int k = 0; k < p2; ++k) o[k] = dist2c(fm, qp[0] - xp[k * 3 + 0], qp[1] - xp[k * 3 + 1], qp[2] - xp[k * 3 + 2]);
        }
}

int g4d_oracle_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* bench.py cpu_baseline: run the kernels on `n` OpenMP threads (n <= 0: leave unchanged); returns the previous setting */
int g4d_oracle_set_threads(int n) {
#ifdef _OPENMP
    const int prev = omp_get_max_threads();
    if (n > 0) omp_set_num_threads(n);
    return prev;
#else
    (void)n;
    return 1;
#endif
}

/* sampling_gpu.cu:86-91  __update(): max of values, ties keep the lower slot's index. */
static inline void fps_update(float *dists, int *dists_i, int idx1, int idx2) {
    const float v1 = dists[idx1], v2 = dists[idx2];
    const int i1 = dists_i[idx1], i2 = dists_i[idx2];
    dists[idx1] = v1 > v2 ? v1 : v2; /* max(v1, v2) */
    dists_i[idx1] = v2 > v1 ? i2 : i1;
}

/* sampling_gpu.cu:93-209  furthest_point_sampling_kernel<block_size>, one "block" per batch
 * item, emulating every thread's strided scan and the shared-memory tree reduction literally
 * (so the tie-break is the reference's, not "lowest index").
 *   dataset (B,N,3) fp32, temp (B,N) fp32 in/out (caller pre-fills 1e10, pointnet2_utils.py:26),
 *   idxs (B,M) int32. */
void g4d_oracle_fps(int b, int n, int m, const float *dataset, float *temp, int *idxs) {
    if (m <= 0) return;
    const int block_size = g4d_oracle_block_size(n);
    const int fm = g_contract;
#pragma omp parallel for schedule(dynamic, 1)
    for (int batch_index = 0; batch_index < b; ++batch_index) {
        float *dists = (float *)malloc(sizeof(float) * (size_t)block_size);
        int *dists_i = (int *)malloc(sizeof(int) * (size_t)block_size);
        const float *ds = dataset + (size_t)batch_index * n * 3;
        float *tp = temp + (size_t)batch_index * n;
        int *out = idxs + (size_t)batch_index * m;
        const int stride = block_size;
        int old = 0;
        out[0] = old;
        for (int j = 1; j < m; j++) {
            const float x1 = ds[old * 3 + 0];
            const float y1 = ds[old * 3 + 1];
            const float z1 = ds[old * 3 + 2];
            for (int tid = 0; tid < block_size; ++tid) {
                int besti = 0;
                float best = -1;
                for (int k = tid; k < n; k += stride) {
                    const float x2 = ds[k * 3 + 0];
                    const float y2 = ds[k * 3 + 1];
                    const float z2 = ds[k * 3 + 2];
                    const float d = dist2c(fm, x2 - x1, y2 - y1, z2 - z1); /* :136 */
                    const float d2 = fminf(d, tp[k]); /* CUDA min(float,float) == fminf */
                    tp[k] = d2;
                    besti = d2 > best ? k : besti;
                    best = d2 > best ? d2 : best;
                }
                dists[tid] = best;
                dists_i[tid] = besti;
            }
            for (int s = block_size / 2; s >= 1; s >>= 1) { /* :154-203, the unrolled ladder */
                for (int tid = 0; tid < s; ++tid) fps_update(dists, dists_i, tid, tid + s);
            }
            old = dists_i[0];
            out[j] = old;
        }
        free(dists);
        free(dists_i);
    }
}

static inline unsigned bitrev_bits(unsigned v, int bits) {
    unsigned r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

/* The same FPS expressed through a total order: winner of a round =
 * arg-max of mind[k]; ties -> smallest bit-reversed (k mod bs), then smallest k.  This is the
 * formulation the HIP kernel implements; tests prove it equal to the literal emulation above
 * on tie-heavy clouds. */
void g4d_oracle_fps_keyed(int b, int n, int m, const float *dataset, float *temp, int *idxs) {
    if (m <= 0) return;
    const int bs = g4d_oracle_block_size(n);
    const int fm = g_contract;
    int bits = 0;
    while ((1 << bits) < bs) ++bits;
#pragma omp parallel for schedule(dynamic, 1)
    for (int bi = 0; bi < b; ++bi) {
        const float *ds = dataset + (size_t)bi * n * 3;
        float *tp = temp + (size_t)bi * n;
        int *out = idxs + (size_t)bi * m;
        int old = 0;
        out[0] = 0;
        for (int j = 1; j < m; ++j) {
            const float x1 = ds[old * 3 + 0], y1 = ds[old * 3 + 1], z1 = ds[old * 3 + 2];
            float best = -1;
            int besti = 0;
            unsigned bestr = 0;
            int have = 0;
            for (int k = 0; k < n; ++k) {
                const float x2 = ds[k * 3 + 0], y2 = ds[k * 3 + 1], z2 = ds[k * 3 + 2];
                const float d = dist2c(fm, x2 - x1, y2 - y1, z2 - z1);
                const float d2 = fminf(d, tp[k]);
                tp[k] = d2;
                if (!(d2 > -1.0f)) continue; /* NaN never wins (besti stays 0 if nothing wins) */
                const unsigned r = bitrev_bits((unsigned)(k % bs), bits);
                if (!have || d2 > best || (d2 == best && r < bestr)) {
                    /* equal value and equal class: smaller k was seen first and is kept */
                    have = 1; best = d2; besti = k; bestr = r;
                }
            }
            old = besti;
            out[j] = old;
        }
    }
}

/* sampling_gpu.cu:8-24  gather_points_kernel_fast: out[b,c,j] = points[b,c,idx[b,j]]. */
void g4d_oracle_gather(int b, int c, int n, int m, const float *points, const int *idx, float *out) {
#pragma omp parallel for collapse(2)
    for (int bs_idx = 0; bs_idx < b; ++bs_idx)
        for (int c_idx = 0; c_idx < c; ++c_idx)
            for (int pt_idx = 0; pt_idx < m; ++pt_idx)
                out[((size_t)bs_idx * c + c_idx) * m + pt_idx] =
                    points[((size_t)bs_idx * c + c_idx) * n + idx[(size_t)bs_idx * m + pt_idx]];
}

/* sampling_gpu.cu:46-63  gather_points_grad_kernel_fast: scatter-add (grad_points pre-zeroed
 * by the caller, pointnet2_utils.py:67).  Sequential order here; the GPU uses atomics. */
void g4d_oracle_gather_grad(int b, int c, int n, int m, const float *grad_out, const int *idx, float *grad_points) {
    for (int bs_idx = 0; bs_idx < b; ++bs_idx)
        for (int c_idx = 0; c_idx < c; ++c_idx)
            for (int pt_idx = 0; pt_idx < m; ++pt_idx)
                grad_points[((size_t)bs_idx * c + c_idx) * n + idx[(size_t)bs_idx * m + pt_idx]] +=
                    grad_out[((size_t)bs_idx * c + c_idx) * m + pt_idx];
}

/* ball_query_gpu.cu:9-45  ball_query_kernel_fast.  idx (B,M,nsample) is pre-zeroed by the
 * caller (pointnet2_utils.py:218); a query without any hit leaves its row untouched. */
void g4d_oracle_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz_all,
                           const float *xyz_all, int *idx_all) {
    const int fm = g_contract;
#pragma omp parallel for collapse(2) schedule(static)
    for (int bs_idx = 0; bs_idx < b; ++bs_idx) {
        for (int pt_idx = 0; pt_idx < m; ++pt_idx) {
            const float *new_xyz = new_xyz_all + (size_t)bs_idx * m * 3 + (size_t)pt_idx * 3;
            const float *xyz = xyz_all + (size_t)bs_idx * n * 3;
            int *idx = idx_all + (size_t)bs_idx * m * nsample + (size_t)pt_idx * nsample;
            const float radius2 = radius * radius;
            const float new_x = new_xyz[0], new_y = new_xyz[1], new_z = new_xyz[2];
            int cnt = 0;
            for (int k = 0; k < n; ++k) {
                const float x = xyz[k * 3 + 0], y = xyz[k * 3 + 1], z = xyz[k * 3 + 2];
                const float d2 = dist2c(fm, new_x - x, new_y - y, new_z - z); /* :30 */
                if (d2 < radius2) {
                    if (cnt == 0)
                        for (int l = 0; l < nsample; ++l) idx[l] = k;
                    idx[cnt] = k;
                    ++cnt;
                    if (cnt >= nsample) break;
                }
            }
        }
    }
}

/* group_points_gpu.cu:47-66  group_points_kernel_fast: out[b,c,p,s] = points[b,c,idx[b,p,s]].
 * (64-bit offsets here; the reference's int32 offsets wrap at 2^31 elements.) */
void g4d_oracle_group(int b, int c, int n, int npoints, int nsample, const float *points, const int *idx, float *out) {
#pragma omp parallel for collapse(2)
    for (int bs_idx = 0; bs_idx < b; ++bs_idx)
        for (int c_idx = 0; c_idx < c; ++c_idx) {
            const float *src = points + ((size_t)bs_idx * c + c_idx) * n;
            float *dst = out + ((size_t)bs_idx * c + c_idx) * npoints * nsample;
            const int *ix = idx + (size_t)bs_idx * npoints * nsample;
            for (size_t i = 0; i < (size_t)npoints * nsample; ++i) dst[i] = src[ix[i]];
        }
}

/* group_points_gpu.cu:8-25  group_points_grad_kernel_fast (scatter-add, pre-zeroed dst). */
void g4d_oracle_group_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                           float *grad_points) {
    for (int bs_idx = 0; bs_idx < b; ++bs_idx)
        for (int c_idx = 0; c_idx < c; ++c_idx) {
            float *dst = grad_points + ((size_t)bs_idx * c + c_idx) * n;
            const float *src = grad_out + ((size_t)bs_idx * c + c_idx) * npoints * nsample;
            const int *ix = idx + (size_t)bs_idx * npoints * nsample;
            for (size_t i = 0; i < (size_t)npoints * nsample; ++i) dst[ix[i]] += src[i];
        }
}

/* interpolate_gpu.cu:9-52  three_nn_kernel_fast.  best* are doubles initialised to 1e40, the
 * distance itself is fp32; stores convert back to fp32 (1e40 -> +inf). */
void g4d_oracle_three_nn(int b, int n, int m, const float *unknown_all, const float *known_all, float *dist2_all,
                         int *idx_all) {
    const int fm = g_contract;
#pragma omp parallel for collapse(2) schedule(static)
    for (int bs_idx = 0; bs_idx < b; ++bs_idx) {
        for (int pt_idx = 0; pt_idx < n; ++pt_idx) {
            const float *unknown = unknown_all + (size_t)bs_idx * n * 3 + (size_t)pt_idx * 3;
            const float *known = known_all + (size_t)bs_idx * m * 3;
            float *dist2 = dist2_all + (size_t)bs_idx * n * 3 + (size_t)pt_idx * 3;
            int *idx = idx_all + (size_t)bs_idx * n * 3 + (size_t)pt_idx * 3;
            const float ux = unknown[0], uy = unknown[1], uz = unknown[2];
            double best1 = 1e40, best2 = 1e40, best3 = 1e40;
            int besti1 = 0, besti2 = 0, besti3 = 0;
            for (int k = 0; k < m; ++k) {
                const float x = known[k * 3 + 0], y = known[k * 3 + 1], z = known[k * 3 + 2];
                const float d = dist2c(fm, ux - x, uy - y, uz - z); /* :33 */
                if (d < best1) {
                    best3 = best2; besti3 = besti2;
                    best2 = best1; besti2 = besti1;
                    best1 = d; besti1 = k;
                } else if (d < best2) {
                    best3 = best2; besti3 = besti2;
                    best2 = d; besti2 = k;
                } else if (d < best3) {
                    best3 = d; besti3 = k;
                }
            }
            dist2[0] = (float)best1; dist2[1] = (float)best2; dist2[2] = (float)best3;
            idx[0] = besti1; idx[1] = besti2; idx[2] = besti3;
        }
    }
}

/* interpolate_gpu.cu:77-97  three_interpolate_kernel_fast. */
void g4d_oracle_three_interp(int b, int c, int m, int n, const float *points_all, const int *idx_all,
                             const float *weight_all, float *out_all) {
#pragma omp parallel for collapse(2)
    for (int bs_idx = 0; bs_idx < b; ++bs_idx)
        for (int c_idx = 0; c_idx < c; ++c_idx) {
            const float *points = points_all + ((size_t)bs_idx * c + c_idx) * m;
            float *out = out_all + ((size_t)bs_idx * c + c_idx) * n;
            for (int pt_idx = 0; pt_idx < n; ++pt_idx) {
                const float *weight = weight_all + (size_t)bs_idx * n * 3 + (size_t)pt_idx * 3;
                const int *idx = idx_all + (size_t)bs_idx * n * 3 + (size_t)pt_idx * 3;
                out[pt_idx] = weight[0] * points[idx[0]] + weight[1] * points[idx[1]] + weight[2] * points[idx[2]];
            }
        }
}

/* interpolate_gpu.cu:120-142  three_interpolate_grad_kernel_fast (pre-zeroed dst). */
void g4d_oracle_three_interp_grad(int b, int c, int n, int m, const float *grad_out_all, const int *idx_all,
                                  const float *weight_all, float *grad_points_all) {
    for (int bs_idx = 0; bs_idx < b; ++bs_idx)
        for (int c_idx = 0; c_idx < c; ++c_idx) {
            const float *grad_out = grad_out_all + ((size_t)bs_idx * c + c_idx) * n;
            float *grad_points = grad_points_all + ((size_t)bs_idx * c + c_idx) * m;
            for (int pt_idx = 0; pt_idx < n; ++pt_idx) {
                const float *weight = weight_all + (size_t)bs_idx * n * 3 + (size_t)pt_idx * 3;
                const int *idx = idx_all + (size_t)bs_idx * n * 3 + (size_t)pt_idx * 3;
                grad_points[idx[0]] += grad_out[pt_idx] * weight[0];
                grad_points[idx[1]] += grad_out[pt_idx] * weight[1];
                grad_points[idx[2]] += grad_out[pt_idx] * weight[2];
            }
        }
}

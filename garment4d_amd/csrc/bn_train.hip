// Training-mode BatchNorm on point-major rows, and the adjoint of the row max-pool (garment4d_amd/mlp_train.py): fp32, Y (rows, C) with a row
// stride ld >= C, one column = one BatchNorm channel, the rows = batch x points (x samples).
//
//   g4d_bn_stats_f32            mean_c = sum_r y / R,  var_c = sum_r (y - mean_c)^2 / R  (biased), TWO passes: the second subtracts the rounded
//                               mean of the first, so a column of mean 1e3 and deviation 0.1 keeps its variance (E[y^2] - mean^2 would not)
//   g4d_bn_act_f32              out = act(z),  z = fma((y - mean) * invstd, gamma, beta),  invstd = 1 / sqrt(var + eps)     -- bn_z() below
//   g4d_bn_act_grad_reduce_f32  dbeta_c = sum_r G,  dgamma_c = sum_r G * xhat,  G = dOut where act passed (z > 0 with the ReLU, everywhere
//                               without), xhat = (y - mean) * invstd recomputed by bn_z(): the mask is the forward's, bit for bit
//   g4d_bn_act_grad_f32         dY = (gamma * invstd) * ((G - dbeta / R) - xhat * (dgamma / R)); running statistics (batch_stats = 0): dY = (gamma * invstd) * G
//   g4d_pool_rows_max_grad_f32  dX = dPooled at the FIRST row of each group of S attaining the column's maximum, 0 at the other S - 1 rows
//
// Layout of every kernel: a thread owns VEC consecutive columns (VEC = 4 with one 16-byte access per row when C % 4 == 0 -- a function of the
// shape alone, the loads are typed 4-byte aligned so any base pointer and any ld serve --, else 1) and walks rows; thread (ty, tx) of a
// block: columns VEC * (256 * blockIdx.y + tx), rows ty, ty + TY, ... of the block's row range, TX = the power of two >= C / VEC (<= 256),
// TY = 256 / TX.  The per-column constants (mean, invstd, gamma, beta) are formed once per thread, not once per element.
// There is NO vector body with a scalar tail: a width that is not a multiple of 4 (13, 67) runs the all-scalar instantiation, 4-byte accesses
// throughout (the model's widths are multiples of 4 except the 3-wide coordinate input, which no BatchNorm sees).
//
// Reductions: the rows are cut into slices of g4d_bn_slice_rows(rows, c) rows (a function of the shape alone); block = slice, a thread adds its
// rows in ascending order; the TY partials of a column and then the slice partials are added by reduce.h's slice_col_sums and reduce_slices.
// Every output is written once; no atomics.
#include "reduce.h"

namespace g4d {

typedef float bn_f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at a 4-byte aligned address

constexpr int kBnSliceMin = 64;       // rows of a slice at least
constexpr int kBnMaxSlices = 1024;    // a CONSTANT, not a device query: 4 blocks per CU on 256 CUs
constexpr int kBnRowsPerThread = 8;   // element-wise kernels: rows a thread walks (amortises the per-column constants)

__host__ __device__ inline long long bn_slice_rows(long long rows) {
    long long sr = (rows + kBnMaxSlices - 1) / kBnMaxSlices;
    sr = (sr + 7) / 8 * 8;
    return sr < kBnSliceMin ? kBnSliceMin : sr;
}
__host__ __device__ inline long long bn_slices(long long rows) {
    const long long sr = bn_slice_rows(rows);
    return rows <= 0 ? 0 : (rows + sr - 1) / sr;
}

__device__ __forceinline__ float bn_invstd(float var, float eps) { return 1.0f / sqrtf(var + eps); }

// THE forward expression (-ffp-contract=off: the one fused operation is the fmaf written here).  Shared by the forward and both backward kernels.
__device__ __forceinline__ float bn_z(float y, float mean, float invstd, float gamma, float beta, float &xhat) {
    xhat = (y - mean) * invstd;
    return fmaf(xhat, gamma, beta);
}

template <int VEC>
struct BnCols {   // the per-column constants of a thread
    float mean[VEC], invstd[VEC], gamma[VEC], beta[VEC];
    __device__ __forceinline__ void load(int col, const float *__restrict__ m, const float *__restrict__ v, float eps, const float *__restrict__ g,
                                         const float *__restrict__ b) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            mean[j] = m[col + j];
            invstd[j] = bn_invstd(v[col + j], eps);
            gamma[j] = g ? g[col + j] : 1.0f;
            beta[j] = b ? b[col + j] : 0.0f;
        }
    }
};

template <int VEC>
__device__ __forceinline__ void bn_load(const float *p, float (&x)[VEC]) {
    if constexpr (VEC == 4) {
        const bn_f32x4u v = *reinterpret_cast<const bn_f32x4u *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = v[j];
    } else {
        x[0] = p[0];
    }
}
template <int VEC>
__device__ __forceinline__ void bn_store(float *p, const float (&x)[VEC]) {
    if constexpr (VEC == 4) {
        bn_f32x4u v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x[j];
        *reinterpret_cast<bn_f32x4u *>(p) = v;
    } else {
        p[0] = x[0];
    }
}

// pass 1 (mean == NULL): slice sums of y; pass 2: slice sums of (y - mean)^2
template <int VEC>
__global__ void __launch_bounds__(256) bn_stats_kernel(long long rows, long long slice_rows, int c, int tx_n, const float *__restrict__ Y, long long ldy,
                                                      const float *__restrict__ mean, float *__restrict__ ws) {
    __shared__ float part[256 * VEC];
    const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n, ty_n = 256 / tx_n;
    const int col = (blockIdx.y * 256 + tx) * VEC;
    const long long r0 = (long long)blockIdx.x * slice_rows;
    const long long r1 = r0 + slice_rows < rows ? r0 + slice_rows : rows;
    float acc[1][VEC], m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[0][j] = 0.f, m[j] = 0.f;
    if (col < c) {
        if (mean)
#pragma unroll
            for (int j = 0; j < VEC; ++j) m[j] = mean[col + j];
#pragma unroll 4
        for (long long r = r0 + ty; r < r1; r += ty_n) {
            float y[VEC];
            bn_load<VEC>(Y + (size_t)r * ldy + col, y);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float d = y[j] - m[j];
                acc[0][j] += mean ? d * d : y[j];
            }
        }
    }
    slice_col_sums<VEC, 1>(acc, part, tx, ty, tx_n, ty_n, col, c, ws);
}

template <int VEC>
__global__ void __launch_bounds__(256) bn_act_kernel(long long rows, int c, int tx_n, const float *__restrict__ Y, long long ldy, const float *__restrict__ mean,
                                                    const float *__restrict__ var, float eps, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                    int relu, float *__restrict__ out, long long ldo) {
    const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n, ty_n = 256 / tx_n;
    const int col = (blockIdx.y * 256 + tx) * VEC;
    if (col >= c) return;
    const long long r0 = (long long)blockIdx.x * (kBnRowsPerThread * ty_n);
    BnCols<VEC> k;
    k.load(col, mean, var, eps, gamma, beta);
#pragma unroll
    for (int i = 0; i < kBnRowsPerThread; ++i) {
        const long long r = r0 + ty + (long long)i * ty_n;
        if (r < rows) {
            float y[VEC], o[VEC];
            bn_load<VEC>(Y + (size_t)r * ldy + col, y);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float xh;
                const float z = bn_z(y[j], k.mean[j], k.invstd[j], k.gamma[j], k.beta[j], xh);
                o[j] = (relu && !(z > 0.f)) ? 0.f : z;
            }
            bn_store<VEC>(out + (size_t)r * ldo + col, o);
        }
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) bn_grad_reduce_kernel(long long rows, long long slice_rows, int c, int tx_n, const float *__restrict__ dOut, long long ldg,
                                                            const float *__restrict__ Y, long long ldy, const float *__restrict__ mean,
                                                            const float *__restrict__ var, float eps, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, int relu, float *__restrict__ ws) {
    __shared__ float part[2 * 256 * VEC];
    const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n, ty_n = 256 / tx_n;
    const int col = (blockIdx.y * 256 + tx) * VEC;
    const long long r0 = (long long)blockIdx.x * slice_rows;
    const long long r1 = r0 + slice_rows < rows ? r0 + slice_rows : rows;
    float acc[2][VEC];   // [0]: dgamma, [1]: dbeta
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[0][j] = acc[1][j] = 0.f;
    if (col < c) {
        BnCols<VEC> k;
        k.load(col, mean, var, eps, gamma, beta);
#pragma unroll 2
        for (long long r = r0 + ty; r < r1; r += ty_n) {
            float y[VEC], g[VEC];
            bn_load<VEC>(Y + (size_t)r * ldy + col, y);
            bn_load<VEC>(dOut + (size_t)r * ldg + col, g);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float xh;
                const float z = bn_z(y[j], k.mean[j], k.invstd[j], k.gamma[j], k.beta[j], xh);
                const float gg = (relu && !(z > 0.f)) ? 0.f : g[j];
                acc[0][j] += gg * xh;
                acc[1][j] += gg;
            }
        }
    }
    slice_col_sums<VEC, 2>(acc, part, tx, ty, tx_n, ty_n, col, c, ws);
}

template <int VEC>
__global__ void __launch_bounds__(256) bn_grad_kernel(long long rows, int c, int tx_n, const float *__restrict__ dOut, long long ldg, const float *__restrict__ Y,
                                                     long long ldy, const float *__restrict__ mean, const float *__restrict__ var, float eps,
                                                     const float *__restrict__ gamma, const float *__restrict__ beta, int relu, int batch_stats,
                                                     const float *__restrict__ dgamma, const float *__restrict__ dbeta, float *__restrict__ dY, long long lddy) {
    const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n, ty_n = 256 / tx_n;
    const int col = (blockIdx.y * 256 + tx) * VEC;
    if (col >= c) return;
    const long long r0 = (long long)blockIdx.x * (kBnRowsPerThread * ty_n);
    BnCols<VEC> k;
    k.load(col, mean, var, eps, gamma, beta);
    float a[VEC], mg[VEC], mb[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        a[j] = k.gamma[j] * k.invstd[j];
        mg[j] = batch_stats ? dgamma[col + j] / (float)rows : 0.f;
        mb[j] = batch_stats ? dbeta[col + j] / (float)rows : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kBnRowsPerThread; ++i) {
        const long long r = r0 + ty + (long long)i * ty_n;
        if (r < rows) {
            float y[VEC], g[VEC], o[VEC];
            bn_load<VEC>(Y + (size_t)r * ldy + col, y);
            bn_load<VEC>(dOut + (size_t)r * ldg + col, g);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float xh;
                const float z = bn_z(y[j], k.mean[j], k.invstd[j], k.gamma[j], k.beta[j], xh);
                const float gg = (relu && !(z > 0.f)) ? 0.f : g[j];
                o[j] = batch_stats ? a[j] * ((gg - mb[j]) - xh * mg[j]) : a[j] * gg;
            }
            bn_store<VEC>(dY + (size_t)r * lddy + col, o);
        }
    }
}

// Built for the ball-query group sizes (S <= 64).  A GroupAll level (S = N, groups = B) leaves only B * C / VEC threads, each walking 2 N
// strided rows serially: correct, and slow -- that shape wants a row-parallel arg-max, which is not built.
// One thread = VEC columns of one group: the first row attaining the maximum (a strict > keeps the earliest; the comparison of
// pool_rows_kernel's fmaxf chain, which passes over NaN rows), then the S rows of dX.
template <int VEC>
__global__ void __launch_bounds__(256) pool_max_grad_kernel(int groups, int S, int c, const float *__restrict__ X, long long ldx, const float *__restrict__ dP,
                                                           long long ldp, int col0, float *__restrict__ dX) {
    const int per = c / VEC;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)groups * per) return;
    const long long g = gid / per;
    const int col = (int)(gid - g * per) * VEC;
    const float *p = X + (size_t)g * S * ldx + col;
    float best[VEC], x[VEC], d[VEC], o[VEC];
    int arg[VEC];
    bn_load<VEC>(p, best);
#pragma unroll
    for (int j = 0; j < VEC; ++j) arg[j] = 0;
    for (int s = 1; s < S; ++s) {
        bn_load<VEC>(p + (size_t)s * ldx, x);
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (x[j] > best[j] || (best[j] != best[j] && x[j] == x[j])) best[j] = x[j], arg[j] = s;
    }
    bn_load<VEC>(dP + (size_t)g * ldp + col0 + col, d);
    float *q = dX + (size_t)g * S * c + col;
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = arg[j] == s ? d[j] : 0.f;
        bn_store<VEC>(q + (size_t)s * c, o);
    }
}

struct BnShape {
    bool vec;
    int tx_n, ty_n;
    unsigned gy;
};
inline BnShape bn_shape(int c) {
    BnShape s;
    s.vec = (c & 3) == 0;   // a function of the shape alone: neither the summation order nor the kernel depends on where a tensor lies
    const int groups = s.vec ? c / 4 : c;
    s.tx_n = 1;
    while (s.tx_n < groups && s.tx_n < 256) s.tx_n *= 2;
    s.ty_n = 256 / s.tx_n;
    s.gy = (unsigned)((groups + 255) / 256);
    return s;
}

}  // namespace g4d

using namespace g4d;
#define G4D_STREAM(s) reinterpret_cast<hipStream_t>(s)
#define BN_ZERO(name, ptr, n, st)                                                                   \
    do {                                                                                            \
        const hipError_t e_ = hipMemsetAsync(ptr, 0, (size_t)(n) * sizeof(float), st);              \
        G4D_REQUIRE(e_ == hipSuccess, name ": hipMemsetAsync: %s", hipGetErrorString(e_));          \
    } while (0)

extern "C" long long g4d_bn_slice_rows(long long rows, int c) {
    return rows < 0 || c <= 0 ? 0 : bn_slice_rows(rows);
}

extern "C" long long g4d_bn_stats_ws_bytes(long long rows, int c) {
    if (rows <= 0 || c <= 0) return 0;
    return bn_slices(rows) * (long long)c * (long long)sizeof(float);
}

extern "C" long long g4d_bn_act_grad_reduce_ws_bytes(long long rows, int c) {
    if (rows <= 0 || c <= 0) return 0;
    return bn_slices(rows) * 2 * (long long)c * (long long)sizeof(float);
}

extern "C" int g4d_bn_stats_f32(long long rows, int c, const float *Y, int ldy, float *ws, float *mean, float *var, g4d_stream_t stream) {
    G4D_REQUIRE(rows >= 0 && c >= 0 && ldy >= 0, "g4d_bn_stats_f32: negative size");
    if (c == 0) return G4D_OK;
    G4D_REQUIRE(ldy >= c, "g4d_bn_stats_f32: ldy < C");
    G4D_REQUIRE(mean && var, "g4d_bn_stats_f32: null pointer");
    hipStream_t st = G4D_STREAM(stream);
    if (rows == 0) {
        BN_ZERO("g4d_bn_stats_f32", mean, c, st);
        BN_ZERO("g4d_bn_stats_f32", var, c, st);
        return G4D_OK;
    }
    G4D_REQUIRE(Y && ws, "g4d_bn_stats_f32: null pointer");
    const BnShape s = bn_shape(c);
    G4D_REQUIRE(s.gy <= 65535, "g4d_bn_stats_f32: too wide");
    const long long slices = bn_slices(rows), sr = bn_slice_rows(rows);
    const dim3 grid((unsigned)slices, s.gy);
    for (int pass = 0; pass < 2; ++pass) {
        const float *m = pass ? mean : nullptr;
        if (s.vec) hipLaunchKernelGGL(bn_stats_kernel<4>, grid, dim3(256), 0, st, rows, sr, c, s.tx_n, Y, (long long)ldy, m, ws);
        else hipLaunchKernelGGL(bn_stats_kernel<1>, grid, dim3(256), 0, st, rows, sr, c, s.tx_n, Y, (long long)ldy, m, ws);
        reduce_slices(slices, c, c, (float)rows, ws, pass ? var : mean, nullptr, st);
    }
    return check_launch("g4d_bn_stats_f32");
}

extern "C" int g4d_bn_act_f32(long long rows, int c, const float *Y, int ldy, const float *mean, const float *var, float eps, const float *gamma,
                              const float *beta, int relu, float *out, int ldo, g4d_stream_t stream) {
    G4D_REQUIRE(rows >= 0 && c >= 0 && ldy >= 0 && ldo >= 0, "g4d_bn_act_f32: negative size");
    if (c == 0 || rows == 0) return G4D_OK;
    G4D_REQUIRE(ldy >= c && ldo >= c, "g4d_bn_act_f32: ld < C");
    G4D_REQUIRE(Y && mean && var && out, "g4d_bn_act_f32: null pointer");
    const BnShape s = bn_shape(c);
    const long long per = (long long)kBnRowsPerThread * s.ty_n, gx = (rows + per - 1) / per;
    G4D_REQUIRE(s.gy <= 65535 && gx < (1ll << 31), "g4d_bn_act_f32: too large");
    const dim3 grid((unsigned)gx, s.gy);
    if (s.vec) hipLaunchKernelGGL(bn_act_kernel<4>, grid, dim3(256), 0, G4D_STREAM(stream), rows, c, s.tx_n, Y, (long long)ldy, mean, var, eps, gamma, beta, relu, out, (long long)ldo);
    else hipLaunchKernelGGL(bn_act_kernel<1>, grid, dim3(256), 0, G4D_STREAM(stream), rows, c, s.tx_n, Y, (long long)ldy, mean, var, eps, gamma, beta, relu, out, (long long)ldo);
    return check_launch("g4d_bn_act_f32");
}

extern "C" int g4d_bn_act_grad_reduce_f32(long long rows, int c, const float *dOut, int ldg, const float *Y, int ldy, const float *mean, const float *var,
                                          float eps, const float *gamma, const float *beta, int relu, float *ws, float *dgamma, float *dbeta,
                                          g4d_stream_t stream) {
    G4D_REQUIRE(rows >= 0 && c >= 0 && ldg >= 0 && ldy >= 0, "g4d_bn_act_grad_reduce_f32: negative size");
    if (c == 0) return G4D_OK;
    G4D_REQUIRE(ldg >= c && ldy >= c, "g4d_bn_act_grad_reduce_f32: ld < C");
    G4D_REQUIRE(dgamma && dbeta, "g4d_bn_act_grad_reduce_f32: null pointer");
    hipStream_t st = G4D_STREAM(stream);
    if (rows == 0) {
        BN_ZERO("g4d_bn_act_grad_reduce_f32", dgamma, c, st);
        BN_ZERO("g4d_bn_act_grad_reduce_f32", dbeta, c, st);
        return G4D_OK;
    }
    G4D_REQUIRE(dOut && Y && mean && var && ws, "g4d_bn_act_grad_reduce_f32: null pointer");
    const BnShape s = bn_shape(c);
    G4D_REQUIRE(s.gy <= 65535 && c < (1 << 30), "g4d_bn_act_grad_reduce_f32: too wide");
    const long long slices = bn_slices(rows), sr = bn_slice_rows(rows);
    const dim3 grid((unsigned)slices, s.gy);
    if (s.vec) hipLaunchKernelGGL(bn_grad_reduce_kernel<4>, grid, dim3(256), 0, st, rows, sr, c, s.tx_n, dOut, (long long)ldg, Y, (long long)ldy, mean, var, eps, gamma, beta, relu, ws);
    else hipLaunchKernelGGL(bn_grad_reduce_kernel<1>, grid, dim3(256), 0, st, rows, sr, c, s.tx_n, dOut, (long long)ldg, Y, (long long)ldy, mean, var, eps, gamma, beta, relu, ws);
    reduce_slices(slices, 2 * (long long)c, c, 1.0f, ws, dgamma, dbeta, st);
    return check_launch("g4d_bn_act_grad_reduce_f32");
}

extern "C" int g4d_bn_act_grad_f32(long long rows, int c, const float *dOut, int ldg, const float *Y, int ldy, const float *mean, const float *var, float eps,
                                   const float *gamma, const float *beta, int relu, int batch_stats, const float *dgamma, const float *dbeta, float *dY,
                                   int lddy, g4d_stream_t stream) {
    G4D_REQUIRE(rows >= 0 && c >= 0 && ldg >= 0 && ldy >= 0 && lddy >= 0, "g4d_bn_act_grad_f32: negative size");
    if (c == 0 || rows == 0) return G4D_OK;
    G4D_REQUIRE(ldg >= c && ldy >= c && lddy >= c, "g4d_bn_act_grad_f32: ld < C");
    G4D_REQUIRE(dOut && Y && mean && var && dY && (!batch_stats || (dgamma && dbeta)), "g4d_bn_act_grad_f32: null pointer");
    const BnShape s = bn_shape(c);
    const long long per = (long long)kBnRowsPerThread * s.ty_n, gx = (rows + per - 1) / per;
    G4D_REQUIRE(s.gy <= 65535 && gx < (1ll << 31), "g4d_bn_act_grad_f32: too large");
    const dim3 grid((unsigned)gx, s.gy);
    if (s.vec) hipLaunchKernelGGL(bn_grad_kernel<4>, grid, dim3(256), 0, G4D_STREAM(stream), rows, c, s.tx_n, dOut, (long long)ldg, Y, (long long)ldy, mean, var, eps, gamma, beta, relu, batch_stats, dgamma, dbeta, dY, (long long)lddy);
    else hipLaunchKernelGGL(bn_grad_kernel<1>, grid, dim3(256), 0, G4D_STREAM(stream), rows, c, s.tx_n, dOut, (long long)ldg, Y, (long long)ldy, mean, var, eps, gamma, beta, relu, batch_stats, dgamma, dbeta, dY, (long long)lddy);
    return check_launch("g4d_bn_act_grad_f32");
}

extern "C" int g4d_pool_rows_max_grad_f32(int groups, int s, int c, const float *X, int ldx, const float *dPooled, int ldp, int col0, float *dX,
                                          g4d_stream_t stream) {
    G4D_REQUIRE(groups >= 0 && c >= 0 && ldx >= 0 && ldp >= 0 && col0 >= 0, "g4d_pool_rows_max_grad_f32: negative size");
    G4D_REQUIRE(s >= 1, "g4d_pool_rows_max_grad_f32: S >= 1");
    if (groups == 0 || c == 0) return G4D_OK;
    G4D_REQUIRE(ldx >= c && (long long)col0 + c <= ldp, "g4d_pool_rows_max_grad_f32: ld < C");
    G4D_REQUIRE(X && dPooled && dX, "g4d_pool_rows_max_grad_f32: null pointer");
    const bool vec = (c & 3) == 0;
    const long long work = (long long)groups * (vec ? c / 4 : c), gx = (work + 255) / 256;
    G4D_REQUIRE(gx < (1ll << 31), "g4d_pool_rows_max_grad_f32: too large");
    if (vec) hipLaunchKernelGGL(pool_max_grad_kernel<4>, dim3((unsigned)gx), dim3(256), 0, G4D_STREAM(stream), groups, s, c, X, (long long)ldx, dPooled, (long long)ldp, col0, dX);
    else hipLaunchKernelGGL(pool_max_grad_kernel<1>, dim3((unsigned)gx), dim3(256), 0, G4D_STREAM(stream), groups, s, c, X, (long long)ldx, dPooled, (long long)ldp, col0, dX);
    return check_launch("g4d_pool_rows_max_grad_f32");
}

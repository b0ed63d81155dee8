// Backward of the GCN layer  Y = act(Ahat . (X W) + b)  (modules/pygcn/layers.py:41-55), all tensors point-major, rows = frames x Vg:
//   G  = dY (act = identity) or dY where Y > 0, else 0 (act = the fused ReLU) -- never stored: the mask is applied where dY is loaded
//   dS = Ahat^T . G per frame          g4d_spmm_rows_grad_f32: gather form over the CSR of Ahat^T, the thread layout of spmm_rows_kernel
//   db = column sums of G              g4d_col_sum_rows_f32
//   dW = X^T . dS                      g4d_gemm_tn_f32: the contraction runs along the ROWS (every other GEMM of csrc/ reduces along features)
//   dX = dS . W^T                      g4d_linear_f32 with W packed as the transposed weight: no kernel here
//
// g4d_gemm_tn_f32 on v_mfma_f32_32x32x2_f32, the row as the k index: lane l of an A fragment holds X[row r + (l >> 5)][feature of (l & 31)], of
// a B fragment dS[row r + (l >> 5)][channel n0 + (l & 31)] -- both tensors are row-major with the row as the slow dimension, so the lanes of
// every fragment load run along the contiguous feature / channel dimension and nothing is transposed anywhere.  One 16-byte load of a lane
// feeds FOUR 32-feature tiles: the tile's m index is a label of dW's rows, so tile e of a 128-feature group is given the features
// f0 + 4 q + e (q = l & 31) and the lane's float4 at f0 + 4 q is the A operand of the four tiles (an 8-byte load feeds two, a 4-byte load one).
// A feature range is cut into 128-wide groups, then a 64-wide one, then at most two 32-wide ones whose lanes are predicated: 323 = 2 x 128 +
// 64 + 3 -> 11 tiles, no lane of a vector load ever passes the end of a row (rows are 4-byte aligned only: ldx = 323).
//
// Work unit = one WAVE: (slice of the rows) x (32-channel tile), every feature tile of the M block in its registers (11 x 16 accumulators at
// Fin = 323) across the whole slice; no LDS, no barrier.  The four waves of a workgroup are the four channel tiles of one slice when
// Cout = 128 (they read the same rows of X at the same time: once from HBM, three times from the vector cache) and four different slices
// when Cout <= 32.  Loads run AHEAD - 1 k-steps in front of the MFMAs: AHEAD register slots, each refilled right after it is consumed.
//
// Deterministic: the number of slices is a function of (rows, Fin, Cout) alone; every slice writes its partial (Fin x Cout) tile to the
// workspace and reduce.h's reduce_slices sums the slices in a fixed order.  No atomics in this file.
#include "reduce.h"

namespace g4d {

typedef float gg_f32x16 __attribute__((ext_vector_type(16)));
typedef float gg_f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte load from a 4-byte aligned address
typedef float gg_f32x2u __attribute__((ext_vector_type(2), aligned(4)));

constexpr int kSliceMin = 256;      // rows of a slice at least (any length works: rows behind a slice's end are predicated)
constexpr int kWorkUnits = 2048;    // slices x channel tiles aimed at: 2 waves on each of the 1024 SIMDs -- a CONSTANT, not a device query

// rows per slice / number of slices: functions of the shape only
__host__ __device__ inline long long tn_slice_rows(long long rows, int cout) {
    const int ntile = (cout + 31) / 32;
    const long long max_slices = kWorkUnits / ntile > 0 ? kWorkUnits / ntile : 1;
    long long sr = (rows + max_slices - 1) / max_slices;
    sr = (sr + 7) / 8 * 8;
    return sr < kSliceMin ? kSliceMin : sr;
}
__host__ __device__ inline long long tn_slices(long long rows, int cout) {
    const long long sr = tn_slice_rows(rows, cout);
    return rows == 0 ? 0 : (rows + sr - 1) / sr;
}

// ---- dS = Ahat^T . G ----------------------------------------------------------------------------------------------------------------
// One thread = 4 channels of one (frame, vertex) row, as spmm_rows_kernel; the CSR is the one of Ahat^T (row u lists the v with
// Ahat[v, u] != 0 in ascending v: the summation order of dS is defined by the host's builder).
__global__ void __launch_bounds__(256) spmm_rows_grad_kernel(long long rows, int vg, int c, const float *__restrict__ dY, const float *__restrict__ Y,
                                                            const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                            const float *__restrict__ vals, float *__restrict__ dS) {
    const int per_row = (c + 3) >> 2;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows * per_row) return;
    const long long row = gid / per_row;
    const int c0 = (int)(gid - row * per_row) * 4;
    const long long f = row / vg;
    const int u = (int)(row - f * vg);
    const int beg = rowptr[u], end = rowptr[u + 1];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const bool full = (c0 + 3 < c) && ((c & 3) == 0);
    for (int e = beg; e < end; ++e) {
        const float a = vals[e];
        const size_t off = ((size_t)f * vg + colidx[e]) * c + c0;
        if (full) {
            float4 g = *reinterpret_cast<const float4 *>(dY + off);
            if (Y) {
                const float4 y = *reinterpret_cast<const float4 *>(Y + off);
                g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f; g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
            }
            acc[0] = fmaf(a, g.x, acc[0]); acc[1] = fmaf(a, g.y, acc[1]); acc[2] = fmaf(a, g.z, acc[2]); acc[3] = fmaf(a, g.w, acc[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < c) {
                    const float g = (!Y || Y[off + j] > 0.f) ? dY[off + j] : 0.f;
                    acc[j] = fmaf(a, g, acc[j]);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c0 + j < c) dS[(size_t)row * c + c0 + j] = acc[j];
}

// ---- db: column sums of G, two passes ------------------------------------------------------------------------------------------------
// Block = one slice of the rows; thread (ty, tx): VEC columns from VEC * tx on (one 16-byte load per row when c % 4 == 0), rows ty, ty + TY, ...
// of the slice; the TY partial sums of a column are added by slice_col_sums.  TX = the power of two >= c / VEC (<= 256); wider matrices
// take grid.y blocks of 256 * VEC columns.
template <int VEC>
__global__ void __launch_bounds__(256) col_sum_kernel(long long rows, long long slice_rows, int c, int tx_n, const float *__restrict__ dY,
                                                     const float *__restrict__ Y, float *__restrict__ ws) {
    __shared__ float part[256 * VEC];
    const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n, ty_n = 256 / tx_n;
    const int col = (blockIdx.y * 256 + tx) * VEC;
    const long long r0 = (long long)blockIdx.x * slice_rows;
    const long long r1 = r0 + slice_rows < rows ? r0 + slice_rows : rows;
    float acc[1][VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[0][j] = 0.f;
    if (col < c)
        for (long long r = r0 + ty; r < r1; r += ty_n) {
            const size_t off = (size_t)r * c + col;
            if constexpr (VEC == 4) {
                const gg_f32x4u g = *reinterpret_cast<const gg_f32x4u *>(dY + off);   // (4-byte aligned type: any base pointer)
                gg_f32x4u y = {1.f, 1.f, 1.f, 1.f};
                if (Y) y = *reinterpret_cast<const gg_f32x4u *>(Y + off);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[0][j] += y[j] > 0.f ? g[j] : 0.f;
            } else {
                acc[0][0] += (!Y || Y[off] > 0.f) ? dY[off] : 0.f;
            }
        }
    slice_col_sums<VEC, 1>(acc, part, tx, ty, tx_n, ty_n, col, c, ws);
}

// ---- dW = X^T . dS ---------------------------------------------------------------------------------------------------------------------
// The A operands of one k-step (2 rows) of a wave: N4 float4 groups (4 tiles each), N2 float2 groups (2 tiles), N1 predicated scalars.
template <int N4, int N2, int N1>
struct TnFrag {
    gg_f32x4u a4[N4 > 0 ? N4 : 1];
    gg_f32x2u a2[N2 > 0 ? N2 : 1];
    float a1[N1 > 0 ? N1 : 1];
    float b;
};

// Loads only -- nothing here waits for a loaded value.  A lane whose feature (scalar tiles) or channel does not exist reads a clamped, valid
// address and keeps what it read: that value only reaches row m / column n of the accumulator tile that belongs to the missing feature /
// channel, which is never stored.  A row behind the slice reads the slice's last row; the caller zeroes its B operand where it is consumed.
template <int N4, int N2, int N1>
__device__ __forceinline__ void tn_load(TnFrag<N4, N2, N1> &fr, const float *__restrict__ X, const float *__restrict__ dS, long long row, long long row_end,
                                        long long ldx, int cout, int q, int f1, int ncol) {
    const long long r = row < row_end ? row : row_end - 1;
    const float *xr = X + r * ldx;
#pragma unroll
    for (int g = 0; g < N4; ++g) fr.a4[g] = *reinterpret_cast<const gg_f32x4u *>(xr + 128 * g + 4 * q);
#pragma unroll
    for (int g = 0; g < N2; ++g) fr.a2[g] = *reinterpret_cast<const gg_f32x2u *>(xr + 128 * N4 + 64 * g + 2 * q);
#pragma unroll
    for (int g = 0; g < N1; ++g) {
        const int f = 128 * N4 + 64 * N2 + 32 * g + q;
        fr.a1[g] = xr[f < f1 ? f : f1];
    }
    fr.b = dS[r * (long long)cout + ncol];
}

// One launch covers the features from f_begin on in blocks of `mblock` (grid.y); fvalid = features that exist from the block's first one on
// (every vector group lies inside them by the dispatch below; only the scalar tiles are predicated).
template <int N4, int N2, int N1, int AHEAD>
__global__ void __launch_bounds__(256) gemm_tn_kernel(long long rows, long long slice_rows, int fin, long long ldx, int cout, int f_begin, int mblock,
                                                     const float *__restrict__ X, const float *__restrict__ dS, float *__restrict__ ws) {
    constexpr int MT = 4 * N4 + 2 * N2 + N1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane & 31, h = lane >> 5;
    const int ntile = (cout + 31) >> 5;
    const long long unit = (long long)blockIdx.x * 4 + wave;      // channel tile fastest: the waves of a block share rows of X when ntile > 1
    const long long slice = unit / ntile;
    const int nt = (int)(unit - slice * ntile);
    const long long r0 = slice * slice_rows;
    if (r0 >= rows) return;                                       // (wave-uniform; no barrier in this kernel)
    const long long r1 = r0 + slice_rows < rows ? r0 + slice_rows : rows;
    const int f0 = f_begin + blockIdx.y * mblock;
    const int fvalid = fin - f0;                                   // > 0 by the launch
    X += f0;
    const int ncol_raw = nt * 32 + q;
    const bool nok = ncol_raw < cout;
    const int ncol = nok ? ncol_raw : cout - 1;

    gg_f32x16 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    TnFrag<N4, N2, N1> buf[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) tn_load<N4, N2, N1>(buf[u], X, dS, r0 + 2 * u + h, r1, ldx, cout, q, fvalid - 1, ncol);

    for (long long r = r0; r < r1; r += 2 * AHEAD) {
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            // consume slot u, then refill the SAME registers for AHEAD k-steps on (behind the slice: the clamped row, a cache hit).  The
            // scheduling barriers keep that order: left alone the scheduler renames the slot and copies it back at the loop's end, which
            // waits for every load just issued (vmcnt(0)) -- the distance AHEAD buys would be gone.
            const float b = r + 2 * u + h < r1 ? buf[u].b : 0.f;   // the slice's ragged end: a row outside it contributes nothing
#pragma unroll
            for (int g = 0; g < N4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * g + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(buf[u].a4[g][e], b, acc[4 * g + e], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < N2; ++g)
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    acc[4 * N4 + 2 * g + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(buf[u].a2[g][e], b, acc[4 * N4 + 2 * g + e], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < N1; ++g)
                acc[4 * N4 + 2 * N2 + g] = __builtin_amdgcn_mfma_f32_32x32x2f32(buf[u].a1[g], b, acc[4 * N4 + 2 * N2 + g], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            tn_load<N4, N2, N1>(buf[u], X, dS, r + 2 * (AHEAD + u) + h, r1, ldx, cout, q, fvalid - 1, ncol);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // C/D layout of the 32x32 forms: register e of lane l is (m = (e & 3) + 8 (e >> 2) + 4 (l >> 5), n = l & 31); m -> feature by the group's rule
    if (!nok) return;
    float *wp = ws + (size_t)slice * fin * cout + ncol;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = (e & 3) + 8 * (e >> 2) + 4 * h;
            int f;
            if (t < 4 * N4) f = 128 * (t >> 2) + 4 * m + (t & 3);
            else if (t < 4 * N4 + 2 * N2) f = 128 * N4 + 64 * ((t - 4 * N4) >> 1) + 2 * m + ((t - 4 * N4) & 1);
            else f = 128 * N4 + 64 * N2 + 32 * (t - 4 * N4 - 2 * N2) + m;
            if (f < fvalid) wp[(size_t)(f0 + f) * cout] = acc[t][e];
        }
}

template <int N4, int N2, int N1, int AHEAD>
static void tn_launch(long long rows, int fin, long long ldx, int cout, int f_begin, int mblock, int mblocks, const float *X, const float *dS, float *ws, hipStream_t st) {
    const long long sr = tn_slice_rows(rows, cout), units = tn_slices(rows, cout) * ((cout + 31) / 32);
    hipLaunchKernelGGL((gemm_tn_kernel<N4, N2, N1, AHEAD>), dim3((unsigned)((units + 3) / 4), mblocks), dim3(256), 0, st, rows, sr, fin, ldx, cout, f_begin, mblock, X, dS, ws);
}

}  // namespace g4d

using namespace g4d;
#define G4D_STREAM(s) reinterpret_cast<hipStream_t>(s)
#define G4D_DIMS_OK(name, ...)                                         \
    do {                                                               \
        const long long dims_[] = {__VA_ARGS__};                       \
        for (long long d_ : dims_) G4D_REQUIRE(d_ >= 0, name ": negative size"); \
    } while (0)

extern "C" int g4d_spmm_rows_grad_f32(int frames, int vg, int c, const float *dY, const float *Y, const int *rowptr_t, const int *colidx_t,
                                      const float *vals_t, float *dS, g4d_stream_t stream) {
    G4D_DIMS_OK("g4d_spmm_rows_grad_f32", frames, vg, c);
    const long long rows = (long long)frames * vg;
    if (rows == 0 || c == 0) return G4D_OK;
    G4D_REQUIRE(dY && rowptr_t && colidx_t && vals_t && dS, "g4d_spmm_rows_grad_f32: null pointer");
    const long long work = rows * ((c + 3) / 4);
    G4D_REQUIRE((work + 255) / 256 < (1ll << 31), "g4d_spmm_rows_grad_f32: too large");
    hipLaunchKernelGGL(spmm_rows_grad_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, G4D_STREAM(stream), rows, vg, c, dY, Y, rowptr_t,
                       colidx_t, vals_t, dS);
    return check_launch("g4d_spmm_rows_grad_f32");
}

extern "C" long long g4d_gemm_tn_slice_rows(long long rows, int fin, int cout) {
    (void)fin;
    return rows < 0 || cout <= 0 ? 0 : tn_slice_rows(rows, cout);
}

extern "C" long long g4d_gemm_tn_ws_bytes(long long rows, int fin, int cout) {
    if (rows <= 0 || fin <= 0 || cout <= 0) return 0;
    return tn_slices(rows, cout) * (long long)fin * cout * (long long)sizeof(float);
}

extern "C" long long g4d_col_sum_rows_ws_bytes(long long rows, int c) {
    if (rows <= 0 || c <= 0) return 0;
    return tn_slices(rows, 32) * (long long)c * (long long)sizeof(float);
}

extern "C" int g4d_col_sum_rows_f32(long long rows, int c, const float *dY, const float *Y, float *ws, float *db, g4d_stream_t stream) {
    G4D_DIMS_OK("g4d_col_sum_rows_f32", rows, c);
    if (c == 0) return G4D_OK;
    G4D_REQUIRE(db, "g4d_col_sum_rows_f32: null pointer");
    hipStream_t st = G4D_STREAM(stream);
    if (rows == 0) {
        const hipError_t e = hipMemsetAsync(db, 0, (size_t)c * sizeof(float), st);
        G4D_REQUIRE(e == hipSuccess, "g4d_col_sum_rows_f32: hipMemsetAsync: %s", hipGetErrorString(e));
        return G4D_OK;
    }
    G4D_REQUIRE(dY && ws, "g4d_col_sum_rows_f32: null pointer");
    G4D_REQUIRE(c <= 65535 * 256, "g4d_col_sum_rows_f32: too wide");
    const long long slices = tn_slices(rows, 32), sr = tn_slice_rows(rows, 32);
    const bool vec = (c & 3) == 0;   // a function of the shape alone: the summation order never depends on where a tensor lies
    const int groups = vec ? c / 4 : c;
    int tx_n = 1;
    while (tx_n < groups && tx_n < 256) tx_n *= 2;
    const dim3 grid((unsigned)slices, (groups + 255) / 256);
    if (vec) hipLaunchKernelGGL(col_sum_kernel<4>, grid, dim3(256), 0, st, rows, sr, c, tx_n, dY, Y, ws);
    else hipLaunchKernelGGL(col_sum_kernel<1>, grid, dim3(256), 0, st, rows, sr, c, tx_n, dY, Y, ws);
    reduce_slices(slices, c, c, 1.0f, ws, db, nullptr, st);
    return check_launch("g4d_col_sum_rows_f32");
}

extern "C" int g4d_gemm_tn_f32(long long rows, int fin, int ldx, int cout, const float *X, const float *dS, float *ws, float *dW,
                               g4d_stream_t stream) {
    G4D_DIMS_OK("g4d_gemm_tn_f32", rows, fin, ldx, cout);
    if (fin == 0 || cout == 0) return G4D_OK;
    G4D_REQUIRE(ldx >= fin, "g4d_gemm_tn_f32: ldx < Fin");
    G4D_REQUIRE(dW, "g4d_gemm_tn_f32: null pointer");
    hipStream_t st = G4D_STREAM(stream);
    const long long n = (long long)fin * cout;
    if (rows == 0) {
        const hipError_t e = hipMemsetAsync(dW, 0, (size_t)n * sizeof(float), st);
        G4D_REQUIRE(e == hipSuccess, "g4d_gemm_tn_f32: hipMemsetAsync: %s", hipGetErrorString(e));
        return G4D_OK;
    }
    G4D_REQUIRE(X && dS && ws, "g4d_gemm_tn_f32: null pointer");
    const long long slices = tn_slices(rows, cout);
    G4D_REQUIRE((slices * ((cout + 31) / 32) + 3) / 4 < (1ll << 31) && (n + 63) / 64 < (1ll << 31) && (fin + 127) / 128 <= 65535, "g4d_gemm_tn_f32: too large");
    // the model's ragged widths in ONE M block (X and dS read once); any other width in 128-feature blocks plus a block of predicated 32-feature
    // tiles for the rest (dS re-read per block)
    if (fin > 320 && fin <= 352) tn_launch<2, 1, 1, 3>(rows, fin, ldx, cout, 0, 352, 1, X, dS, ws, st);
    else if (fin > 192 && fin <= 224) tn_launch<1, 1, 1, 4>(rows, fin, ldx, cout, 0, 224, 1, X, dS, ws, st);
    else {
        const int full = fin / 128, tiles = (fin - 128 * full + 31) / 32;
        if (full) tn_launch<1, 0, 0, 4>(rows, fin, ldx, cout, 0, 128, full, X, dS, ws, st);
        if (tiles == 1) tn_launch<0, 0, 1, 4>(rows, fin, ldx, cout, 128 * full, 128, 1, X, dS, ws, st);
        else if (tiles == 2) tn_launch<0, 0, 2, 4>(rows, fin, ldx, cout, 128 * full, 128, 1, X, dS, ws, st);
        else if (tiles == 3) tn_launch<0, 0, 3, 4>(rows, fin, ldx, cout, 128 * full, 128, 1, X, dS, ws, st);
        else if (tiles == 4) tn_launch<0, 0, 4, 4>(rows, fin, ldx, cout, 128 * full, 128, 1, X, dS, ws, st);
    }
    reduce_slices(slices, n, n, 1.0f, ws, dW, nullptr, st);
    return check_launch("g4d_gemm_tn_f32");
}

// Backward of the positional encoders of the refinement loop (csrc/pos_encode.hip is the forward).  Per query q with the ball-query hits
// j_s = idx[q, s], s < S:
//   in_s = [x_j - q ; e_j]    z1_s = W1 in_s + (b1 | t_j)    h_s = relu(z1_s)    z2_s = W2 h_s    out[c] = max_s z2_s[c] + b2[c]
// Given dOut (a 32-column window of the gradient of the padded GCN input) the kernel RECOMPUTES the forward of the query instead of reading
// 31 M rows of stored activations: the forward launch is untouched, nothing is saved for the backward but the inputs.
//
// Max-pool: per channel c the gradient goes to the FIRST sample that attains the maximum (strict > while s ascends).  Ball-query padding rows
// are copies of the first hit: every copy has the same source point j and the same bits of z2, so a tie among copies sends the gradient to
// the same source point whichever copy is taken -- and the first copy is the hit itself.
//
// Layout: lane = channel.  A wave works on two queries at a time (lanes 0-31 / 32-63), lane c of a half owns channel c of its query:
//   stage    the half's S grouped rows [x_j - q ; e_j] (difference formed first, in fp32, like the forward) and source rows j -> LDS
//   layer 1  lane c: h_s[c] for every s (3 + E FMAs each, its row of W1 in registers; t_j[c] is one 128-byte load per row) -> LDS
//   layer 2  lane c: z2_s[c] = sum_k W2[c][k] h_s[k], h_s broadcast from LDS as float4s, its row of W2 in registers; running max + first argmax s*
//   backward lane c holds the ONE non-zero of column c of dz2: go = dOut[q][c] at row s*.  With h = h_{s*}:
//              dW2[c][:] += go h           db2[c] += go                      (32 + 1 accumulators in the lane's registers for the whole launch)
//              g[k] = go W2[c][k] [h[k] > 0]                                 (this lane's share of dz1_{s*}; other lanes may share the row)
//              dxin = W1^T g   -> d new_xyz = -sum over the 32 lanes (fixed xor tree), d xyz / d extra: atomic adds at row j_{s*}
//              g -> LDS;  dW1[k][i] += sum over the wave's 64 (query, channel) pairs of g[k] in_{s*}[i],  db1[k] += sum g[k]:
//                lane (k, half) owns dW1[k][4 half .. 4 half + 3]; d table[j_{s*}][:] += g as 128-byte atomic row segments
// The dense form of layer 2's backward (dh = W2^T dz2, dW2 += dz2 h^T over all S rows) would multiply S x 32 matrices that hold at most 32
// non-zeros; on v_mfma_f32_16x16x4_f32 that is 2 x 64 MFMAs per 64 rows for 1/S of useful work, and dz2 / h would first have to be brought
// into fragment order.  In the lane = channel form the sparse products are 32 + 32 FMAs per lane, so the whole backward stays on the VALU
// and costs less than the recomputed forward (S x (3 + E + 32) FMAs per lane).  DESIGN.md section 8 has the register count and timings.
//
// Deterministic part: dW1, db1, dW2, db2 (per-lane accumulators over a fixed assignment of queries to waves -- the grid is a function of the
// shape alone --, halves and waves added in a fixed order, one partial per workgroup, partials summed in block order by a second kernel) and
// d new_xyz (one store per query).  d xyz, d extra, d table are fp32 atomic scatter-adds like g4d_group_grad_f32: the caller zero-fills them.
#include "g4d_common.h"

namespace g4d {

typedef float pg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPgPartial = 32 * 32 + 32 + 32 * 8 + 32;   // dW2 | db2 | dW1 (row stride 8) | db1
constexpr int kPgMaxBlocks = 512;
constexpr int kPgHs = 36;                                // LDS row stride of h (16-byte aligned rows)
constexpr int kPgGs = 33;                                // LDS row stride of g (conflict-free scalar rows)

struct PeGradArgs {
    int n, p, S, iters;
    long long Q;
    const float *xyz, *new_xyz, *extra, *table;
    const int *idx;
    const float *W1, *b1, *W2, *dOut;
    int ldg, col0;
    float *partial, *d_new_xyz, *d_xyz, *d_extra, *d_table;
    int need_w1, need_in;
};

__host__ __device__ inline int pg_wave_floats(int S) {
    const int h = 2 * S * kPgHs, g = 64 * kPgGs;
    return 2 * S * 8 + 2 * S + (h > g ? h : g) + 64;
}

template <int E, bool TABLE>
__global__ void __launch_bounds__(256, 2) pos_encode_grad_kernel(const PeGradArgs a) {
    constexpr int KX = 3 + E;
    extern __shared__ float pg_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int half = lane >> 5, c = lane & 31;
    const int S = a.S;
    float *inb = pg_lds + (size_t)wave * pg_wave_floats(S);     // [2][S][8]
    int *jb = reinterpret_cast<int *>(inb + 2 * S * 8);          // [2][S] source row f * n + j
    float *hb = reinterpret_cast<float *>(jb + 2 * S);           // [2][S][kPgHs], later g: [64][kPgGs]
    float *gb = hb;
    int *sb = reinterpret_cast<int *>(hb + max(2 * S * kPgHs, 64 * kPgGs));   // [64] winner row (half * S + s*) of (half, channel)

    float *w1s = pg_lds + (size_t)nwaves * pg_wave_floats(S);    // [32][8] W1, shared by the workgroup: dxin = W1^T g reads it as broadcasts
    for (int i = threadIdx.x; i < 256; i += blockDim.x) w1s[i] = (i & 7) < KX ? a.W1[(i >> 3) * KX + (i & 7)] : 0.f;
    float w1[KX], w2[32];
#pragma unroll
    for (int i = 0; i < KX; ++i) w1[i] = a.W1[c * KX + i];
#pragma unroll
    for (int k = 0; k < 32; ++k) w2[k] = a.W2[c * 32 + k];
    const float b1c = a.b1 ? a.b1[c] : 0.f;
    float aW2[32], ab2 = 0.f, aW1[4] = {0.f, 0.f, 0.f, 0.f}, ab1 = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) aW2[k] = 0.f;

    for (int it = 0; it < a.iters; ++it) {
        const long long pair = ((long long)it * gridDim.x + blockIdx.x) * nwaves + wave;
        const long long q = pair * 2 + half;
        const bool valid = q < a.Q;
        const long long qc = valid ? q : a.Q - 1;               // a query past the end recomputes the last one and contributes go = 0
        const int f = (int)(qc / a.p);
        const float qx = a.new_xyz[qc * 3], qy = a.new_xyz[qc * 3 + 1], qz = a.new_xyz[qc * 3 + 2];
        for (int r = c; r < S; r += 32) {
            const int src = f * a.n + a.idx[qc * S + r];
            float *in = inb + (half * S + r) * 8;
            in[0] = a.xyz[(size_t)src * 3] - qx;
            in[1] = a.xyz[(size_t)src * 3 + 1] - qy;
            in[2] = a.xyz[(size_t)src * 3 + 2] - qz;
#pragma unroll
            for (int e = 0; e < 5; ++e) in[3 + e] = e < E ? a.extra[(size_t)src * E + e] : 0.f;
            jb[half * S + r] = src;
        }
        __syncthreads();
        // layer 1: h_s[c]
#pragma unroll 4
        for (int s = 0; s < S; ++s) {
            const float *in = inb + (half * S + s) * 8;
            const pg_f32x4 i0 = *reinterpret_cast<const pg_f32x4 *>(in), i1 = *reinterpret_cast<const pg_f32x4 *>(in + 4);
            float z = TABLE ? a.table[(size_t)jb[half * S + s] * 32 + c] + b1c : b1c;
#pragma unroll
            for (int i = 0; i < KX; ++i) z = __builtin_fmaf(w1[i], i < 4 ? i0[i] : i1[i - 4], z);
            hb[(half * S + s) * kPgHs + c] = fmaxf(z, 0.f);
        }
        __syncthreads();
        // layer 2 + first argmax
        float best = -INFINITY;
        int bs = 0;
#pragma unroll 2
        for (int s = 0; s < S; ++s) {
            const float *h = hb + (half * S + s) * kPgHs;
            float z = 0.f;
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) {
                const pg_f32x4 hv = *reinterpret_cast<const pg_f32x4 *>(h + 4 * k4);
#pragma unroll
                for (int e = 0; e < 4; ++e) z = __builtin_fmaf(hv[e], w2[4 * k4 + e], z);
            }
            if (z > best) { best = z; bs = s; }
        }
        const float go = valid ? a.dOut[(size_t)q * a.ldg + a.col0 + c] : 0.f;
        const int win = half * S + bs;
        const float *hw = hb + win * kPgHs;
        float g[32];
#pragma unroll
        for (int k4 = 0; k4 < 8; ++k4) {
            const pg_f32x4 hv = *reinterpret_cast<const pg_f32x4 *>(hw + 4 * k4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * k4 + e;
                aW2[k] = __builtin_fmaf(go, hv[e], aW2[k]);
                g[k] = hv[e] > 0.f ? w2[k] * go : 0.f;
            }
        }
        ab2 += go;
        __syncthreads();   // every lane has read its winner's h: the buffer becomes g
        if (a.need_w1 || a.need_in || (TABLE && a.d_table)) {
#pragma unroll
            for (int k = 0; k < 32; ++k) gb[lane * kPgGs + k] = g[k];
            sb[lane] = win;
        }
        __syncthreads();
        if (a.need_in) {   // dxin = W1^T g
            float dxin[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) dxin[i] = 0.f;
#pragma unroll 4
            for (int k = 0; k < 32; ++k) {   // g from the lane's own LDS row: a rolled loop, W1 rows as broadcasts
                const float gk = gb[lane * kPgGs + k];
                const pg_f32x4 wa = *reinterpret_cast<const pg_f32x4 *>(w1s + k * 8), wb = *reinterpret_cast<const pg_f32x4 *>(w1s + k * 8 + 4);
#pragma unroll
                for (int i = 0; i < KX; ++i) dxin[i] = __builtin_fmaf(i < 4 ? wa[i] : wb[i - 4], gk, dxin[i]);
            }
            const size_t src = (size_t)jb[win];
            if (go != 0.f) {
                if (a.d_xyz) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) atomicAdd(a.d_xyz + src * 3 + i, dxin[i]);
                }
                if (E > 0 && a.d_extra) {
#pragma unroll
                    for (int e = 0; e < E; ++e) atomicAdd(a.d_extra + src * E + e, dxin[3 + e]);
                }
            }
            if (a.d_new_xyz) {
                float sx = dxin[0], sy = dxin[1], sz = dxin[2];
#pragma unroll
                for (int m = 16; m >= 1; m >>= 1) {   // stays inside the 32 lanes of the half; a fixed tree
                    sx += __shfl_xor(sx, m, 64);
                    sy += __shfl_xor(sy, m, 64);
                    sz += __shfl_xor(sz, m, 64);
                }
                if (c == 0 && valid) {
                    a.d_new_xyz[q * 3] = -sx;
                    a.d_new_xyz[q * 3 + 1] = -sy;
                    a.d_new_xyz[q * 3 + 2] = -sz;
                }
            }
        }
        if (a.need_w1) {   // lane (k = c, half): dW1[k][4 half ..], db1[k] over the wave's 64 (query, channel) pairs, in pair order
#pragma unroll 4
            for (int vr = 0; vr < 64; ++vr) {
                const float gv = gb[vr * kPgGs + c];
                const pg_f32x4 iv = *reinterpret_cast<const pg_f32x4 *>(inb + sb[vr] * 8 + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) aW1[e] = __builtin_fmaf(gv, iv[e], aW1[e]);
                ab1 += gv;
            }
        }
        if (TABLE && a.d_table) {   // 128-byte row segments: half h takes the pairs 2 i + h
#pragma unroll 4
            for (int i = 0; i < 32; ++i) {
                const int vr = 2 * i + half;
                const float gv = gb[vr * kPgGs + c];
                if (gv != 0.f) atomicAdd(a.d_table + (size_t)jb[sb[vr]] * 32 + c, gv);
            }
        }
        __syncthreads();
    }
    if (!a.partial) return;
    // halves (lower + upper), then the waves in wave order, one partial per workgroup
    float *red = pg_lds;   // [nwaves][kPgPartial]: fits (a wave's region is larger), and the loop's last barrier has passed
    float *mine = red + wave * kPgPartial;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const float o = __shfl_xor(aW2[k], 32, 64);
        if (half == 0) mine[c * 32 + k] = aW2[k] + o;
    }
    {
        const float o = __shfl_xor(ab2, 32, 64);
        if (half == 0) mine[1024 + c] = ab2 + o;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) mine[1056 + c * 8 + 4 * half + e] = aW1[e];
    if (half == 0) mine[1312 + c] = ab1;
    __syncthreads();
    float *p = a.partial + (size_t)blockIdx.x * kPgPartial;
    for (int i = threadIdx.x; i < kPgPartial; i += blockDim.x) {
        float s = red[i];
        for (int w = 1; w < nwaves; ++w) s += red[w * kPgPartial + i];
        p[i] = s;
    }
}

// sums the workgroup partials in block order (four interleaved chains, then ((0 + 1) + 2) + 3) and writes the compact gradients
__global__ void __launch_bounds__(256) pos_encode_grad_reduce_kernel(int nblocks, int kx, const float *__restrict__ partial, float *dW1, float *db1,
                                                                    float *dW2, float *db2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kPgPartial) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int b = 0;
    for (; b + 3 < nblocks; b += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += partial[(size_t)(b + j) * kPgPartial + i];
    }
    for (; b < nblocks; ++b) s[0] += partial[(size_t)b * kPgPartial + i];
    const float v = ((s[0] + s[1]) + s[2]) + s[3];
    if (i < 1024) { if (dW2) dW2[i] = v; }
    else if (i < 1056) { if (db2) db2[i - 1024] = v; }
    else if (i < 1312) {
        const int k = (i - 1056) >> 3, col = (i - 1056) & 7;
        if (dW1 && col < kx) dW1[k * kx + col] = v;
    } else if (db1) db1[i - 1312] = v;
}

static void pg_grid(long long Q, int S, int *waves, int *blocks, int *iters) {
    const int w = S > 32 ? 2 : 4;   // S = 64: two waves per workgroup keep the dynamic LDS under 64 KB
    const long long pairs = (Q + 1) / 2;
    long long want = (pairs + w - 1) / w;
    if (want > kPgMaxBlocks) want = kPgMaxBlocks;
    if (want < 1) want = 1;
    *waves = w;
    *blocks = (int)want;
    *iters = (int)((pairs + want * w - 1) / (want * w));
}

}  // namespace g4d

extern "C" long long g4d_pos_encode_grad_ws_bytes(int frames, int p, int nsample) {
    using namespace g4d;
    int w, b, it;
    pg_grid((long long)frames * p, nsample, &w, &b, &it);
    return (long long)b * kPgPartial * 4;
}

extern "C" int g4d_pos_encode_grad_f32(int frames, int n, int p, int nsample, int n_extra, const float *xyz, const float *new_xyz,
                                       const float *extra, const float *table, const int *idx, const float *W1, const float *b1,
                                       const float *W2, const float *dOut, int ldg, int col0, float *ws, float *dW1, float *db1, float *dW2,
                                       float *db2, float *d_new_xyz, float *d_xyz, float *d_extra, float *d_table, g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(frames >= 0 && n > 0 && p >= 0 && n_extra >= 0 && n_extra <= 5, "g4d_pos_encode_grad_f32: bad sizes (n_extra <= 5)");
    G4D_REQUIRE(nsample == 4 || nsample == 8 || nsample == 16 || nsample == 32 || nsample == 64,
                "g4d_pos_encode_grad_f32: nsample must be 4|8|16|32|64 (got %d)", nsample);
    const long long Q = (long long)frames * p, rows = Q * nsample;
    if (rows == 0) return G4D_OK;
    G4D_REQUIRE(xyz && new_xyz && idx && W1 && W2 && dOut && (extra || n_extra == 0) && (b1 || table), "g4d_pos_encode_grad_f32: null pointer");
    G4D_REQUIRE(ldg >= col0 + 32 && col0 >= 0, "g4d_pos_encode_grad_f32: gradient window out of range");
    G4D_REQUIRE(rows < (1ll << 31) - 64 && (long long)frames * n * 32 * 4 < (1ll << 32) && (long long)p * nsample >= 64,
                "g4d_pos_encode_grad_f32: needs rows < 2^31, frames*n*128 B < 4 GB and p*nsample >= 64 (the forward's domain)");
    const bool need_w = dW1 || db1 || dW2 || db2;
    G4D_REQUIRE(ws || !need_w, "g4d_pos_encode_grad_f32: weight gradients need the workspace (g4d_pos_encode_grad_ws_bytes)");
    if (!need_w && !d_new_xyz && !d_xyz && !(d_extra && n_extra) && !(d_table && table)) return G4D_OK;
    PeGradArgs a;
    int waves, blocks, iters;
    pg_grid(Q, nsample, &waves, &blocks, &iters);
    a.n = n; a.p = p; a.S = nsample; a.iters = iters; a.Q = Q;
    a.xyz = xyz; a.new_xyz = new_xyz; a.extra = extra; a.table = table; a.idx = idx;
    a.W1 = W1; a.b1 = b1; a.W2 = W2; a.dOut = dOut; a.ldg = ldg; a.col0 = col0;
    a.partial = need_w ? ws : nullptr;
    a.d_new_xyz = d_new_xyz; a.d_xyz = d_xyz; a.d_extra = n_extra ? d_extra : nullptr; a.d_table = table ? d_table : nullptr;
    a.need_w1 = (dW1 || db1) ? 1 : 0;
    a.need_in = (d_new_xyz || d_xyz || a.d_extra) ? 1 : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = ((size_t)waves * pg_wave_floats(nsample) + 256) * sizeof(float);
#define G4D_PG_LAUNCH(EE)                                                                                                      \
    case EE:                                                                                                                   \
        if (table) hipLaunchKernelGGL((pos_encode_grad_kernel<EE, true>), dim3(blocks), dim3(64 * waves), lds, st, a);          \
        else hipLaunchKernelGGL((pos_encode_grad_kernel<EE, false>), dim3(blocks), dim3(64 * waves), lds, st, a);               \
        break;
    switch (n_extra) {
        G4D_PG_LAUNCH(0) G4D_PG_LAUNCH(1) G4D_PG_LAUNCH(2) G4D_PG_LAUNCH(3) G4D_PG_LAUNCH(4)
        default:
            if (table) hipLaunchKernelGGL((pos_encode_grad_kernel<5, true>), dim3(blocks), dim3(64 * waves), lds, st, a);
            else hipLaunchKernelGGL((pos_encode_grad_kernel<5, false>), dim3(blocks), dim3(64 * waves), lds, st, a);
    }
#undef G4D_PG_LAUNCH
    if (need_w)
        hipLaunchKernelGGL(pos_encode_grad_reduce_kernel, dim3((kPgPartial + 255) / 256), dim3(256), 0, st, blocks, 3 + n_extra, ws, dW1, db1, dW2, db2);
    return check_launch("g4d_pos_encode_grad_f32");
}

// The adjoint of lbs() (include/g4d_smpl.h is the contract; tests/smpl_grad_twin.py restates it in numpy).
//   grad_pre_kernel   one wave per frame: the rigid part again (smpl_rigid.h) and the B operands of the two forward GEMMs in fragment order,
//                     as lbs.hip's lbs_frame_kernel writes them for the forward: coefficients C[tile][g][q * 16 + frame][s] = c[16 g + 4 s + q],
//                     transforms At[tile][flat / 4][q * 16 + frame][flat % 4] = A[4 js + q][e], flat = e JS + js.
//   grad_main_kernel  workgroup = (a slab of G4D_SMPL_SLAB_VERTS vertices, four 16-frame tiles), one wave per frame tile.  Per 32-vertex tile
//                     the blend rows (NC x 96 floats, 86 KB) are staged in LDS once; per 16-vertex half a wave rebuilds v_posed^T and T^T
//                     (vertices x frames tiles, as lbs_mfma_kernel does), so that a lane holds the posed vertex, the 3x4 transform and -- read
//                     from d_verts -- the incoming gradient of the same four (vertex, frame) pairs: d v_posed = (T^R)^T g is 9 FMAs in
//                     registers.  Both contractions over the vertices then run on the matrix cores with those registers as B operands
//                     (k = the four vertices 4 q + r of an instruction, columns = frames):
//                        dA  (joints x frames, one tile per entry of the 3x4)   A operand = W^T           from LDS
//                        dc  (coefficients x frames, 14 tiles)                   A operand = the blend rows from LDS (the staged copy)
//                     The accumulators stay in registers across the slab's tiles and are stored once, to the slab: no read-modify-write.
//   slab_sum_kernel   one thread per (frame, entry): the slabs added in ascending order, in float64, rounded once.
//   grad_post_kernel  one wave per frame, in float64: the chain, joint and Rodrigues adjoints.
//   betas_sum_kernel  betas_bstride == 0: the frames' rows added in ascending order.
// No atomics: every value has one writer and every sum one order.
#include "../g4d_common.h"
#include "../smpl_rigid.h"
#include "../../../include/g4d_smpl.h"

namespace g4d {

namespace {
constexpr int kKS = G4D_SMPL_MAX_COEFFS / 4;   // k-steps of 4 blend rows
constexpr int kKG = kKS / 4;                   // groups of 16 blend rows
constexpr int kVT = 32;                        // vertices per tile (two 16-vertex halves)
constexpr int kSlabTiles = G4D_SMPL_SLAB_VERTS / kVT;
constexpr int kWaves = 4;                      // = frame tiles per workgroup
constexpr int kMaxJ = G4D_SMPL_MAX_JOINTS;
constexpr int kBlendFloats = 2 * 3 * kKG * 256;
typedef float sg_f4 __attribute__((ext_vector_type(4)));
static_assert(kKG * 16 == G4D_SMPL_MAX_COEFFS && kSlabTiles * kVT == G4D_SMPL_SLAB_VERTS && kMaxJ == 32, "tile constants");

// where blend row k, coordinate c of vertex vv (0..15) of half st sits.  The forward's A operand (lane = vertex, quarter = k % 4) reads the four
// floats s = (k / 4) % 4 at once; the adjoint's (lane = k % 16, quarter q = vertex / 4) reads single floats: the xor spreads those over the banks.
__device__ __forceinline__ int blend_at(int st, int c, int k, int vv) {
    return ((st * 3 + c) * kKG + (k >> 4)) * 256 + (k & 3) * 64 + ((vv ^ (k & 3)) << 2) + ((k >> 2) & 3);
}
}  // namespace

__global__ void __launch_bounds__(256) grad_pre_kernel(int B, int J, int NB, int JS, int pose2rot, const float *__restrict__ betas, int betas_bstride,
                                                       const float *__restrict__ pose, const float *__restrict__ Jt, const float *__restrict__ Js,
                                                       const int *__restrict__ parents, float *__restrict__ Cws, float *__restrict__ Aws) {
    __shared__ float sR_[4][kMaxJ * 9], sJ_[4][kMaxJ * 3], sL_[4][kMaxJ * 12], sG_[4][kMaxJ * 12], sC_[4][4 * kKS];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + w;              // frames of whole 16-frame tiles: those past B get zero operands
    const int ntile = (B + 15) / 16;
    if (b >= ntile * 16) return;                   // (wave-local LDS exchange only: no workgroup barrier below)
    float *R_ = sR_[w], *J_ = sJ_[w], *L_ = sL_[w], *G_ = sG_[w], *C_ = sC_[w];
    const int NC = NB + (J - 1) * 9;
    for (int i = l; i < 4 * kKS; i += 64) C_[i] = 0.f;
    for (int i = l; i < kMaxJ * 12; i += 64) L_[i] = 0.f;
    wave_sync_lds();
    if (b < B) {
        rigid_wave(l, b, J, NB, pose2rot, betas, betas_bstride, pose, Jt, Js, parents, R_, J_, L_, G_);
        if (l < J && l > 0) {                      // lbs.py:217 / :222  (R[1:] - I)
#pragma unroll
            for (int k = 0; k < 9; ++k) C_[NB + (l - 1) * 9 + k] = R_[l * 9 + k] - ((k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f);
        }
        for (int i = l; i < NB; i += 64) C_[i] = betas[(size_t)b * betas_bstride + i];
        wave_sync_lds();
        if (l < J) {  // A = G with the rest-pose joint removed (lbs.py:414-417), kept in L_
            const float jx = J_[l * 3 + 0], jy = J_[l * 3 + 1], jz = J_[l * 3 + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float g0 = G_[l * 12 + r * 4 + 0], g1 = G_[l * 12 + r * 4 + 1], g2 = G_[l * 12 + r * 4 + 2], g3 = G_[l * 12 + r * 4 + 3];
                L_[l * 12 + r * 4 + 0] = g0; L_[l * 12 + r * 4 + 1] = g1; L_[l * 12 + r * 4 + 2] = g2;
                L_[l * 12 + r * 4 + 3] = g3 - fmaf(g2, jz, fmaf(g1, jy, g0 * jx));
            }
        }
        wave_sync_lds();
    }
    const int tile = b >> 4, bi = b & 15;
    float *cw = Cws + (size_t)tile * kKG * 256;
    for (int i = l; i < 4 * kKS; i += 64) {          // i = (g, q, s): coefficient k = 16 g + 4 s + q
        const int g = i >> 4, q = (i >> 2) & 3, s4 = i & 3, k = 4 * (4 * g + s4) + q;
        cw[(g * 64 + q * 16 + bi) * 4 + s4] = k < NC ? C_[k] : 0.f;
    }
    float *aw = Aws + (size_t)tile * 3 * JS * 256;
    for (int i = l; i < 4 * 12 * JS; i += 64) {      // i = (q, flat = e JS + js): transform entry e of joint j = 4 js + q
        const int q = i / (12 * JS), flat = i - q * 12 * JS, e = flat / JS, js = flat - e * JS, j = 4 * js + q;
        aw[((flat >> 2) * 64 + q * 16 + bi) * 4 + (flat & 3)] = (b < B && j < J) ? L_[j * 12 + e] : 0.f;
    }
}

template <int JS>
__global__ void __launch_bounds__(64 * kWaves) grad_main_kernel(int B, int V, int J, int NC, const float *__restrict__ v_template,
                                                                const float *__restrict__ blend_dirs, const float *__restrict__ weights,
                                                                const float *__restrict__ Cws, const float *__restrict__ Aws,
                                                                const float *__restrict__ d_verts, float *__restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float sg_smem[];
    float *s_w = sg_smem + kBlendFloats;              // [2][JS][64]     W[v = lane % 16][4 js + lane / 16]: A operand of T = W . A
    float *s_wb = s_w + 2 * JS * 64;                  // [2][2][4][64]   W[v = 4 (lane / 16) + r][16 jt + lane % 16]: A operand of dA = W^T . P
    float *s_t = s_wb + 2 * 2 * 4 * 64;               // [32][3]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, fq = lane >> 4;
    const int nft = (B + 15) / 16;
    const int ft = blockIdx.y * kWaves + wave;
    const bool active = ft < nft;
    const int ftc = min(ft, nft - 1);                 // idle waves read the last tile's operands and store nothing
    const int slab = blockIdx.x;
    const size_t E = (size_t)V * 3;

    sg_f4 cf4[kKG];
    {
        const sg_f4 *cp = reinterpret_cast<const sg_f4 *>(Cws + (size_t)ftc * kKG * 256) + lane;
#pragma unroll
        for (int g = 0; g < kKG; ++g) cf4[g] = cp[g * 64];
    }
    sg_f4 dA[2][12], dC[kKG];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int e = 0; e < 12; ++e) dA[jt][e] = (sg_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < kKG; ++g) dC[g] = (sg_f4){0.f, 0.f, 0.f, 0.f};
    const int f = ftc * 16 + fi;
    const bool frame_ok = active && f < B;

    for (int t = 0; t < kSlabTiles; ++t) {
        const int v0 = (slab * kSlabTiles + t) * kVT;
        if (v0 >= V) break;                            // (the same for every thread of the workgroup)
        if (t > 0) __syncthreads();                    // the previous tile's rows have been read
        {   // the tile's blend rows, zero beyond NC and beyond V
            const int ncol = min(kVT * 3, (int)(E - (size_t)v0 * 3));
#pragma unroll 12
            for (int i = tid; i < 4 * kKS * kVT * 3; i += 64 * kWaves) {
                const int k = i / (kVT * 3), e = i - k * (kVT * 3);
                const int vv = e / 3, c = e - vv * 3;
                const float d = (k < NC && e < ncol) ? blend_dirs[(size_t)k * E + (size_t)v0 * 3 + e] : 0.f;
                sg_smem[blend_at(vv >> 4, c, k, vv & 15)] = d;
            }
        }
        for (int i = tid; i < 2 * JS * 64; i += 64 * kWaves) {
            const int st = i / (JS * 64), js = (i / 64) % JS, ln = i & 63;
            const int v = v0 + st * 16 + (ln & 15), j = 4 * js + (ln >> 4);
            s_w[i] = (v < V && j < J) ? weights[(size_t)v * J + j] : 0.f;
        }
        for (int i = tid; i < 2 * 2 * 4 * 64; i += 64 * kWaves) {
            const int ln = i & 63, r = (i >> 6) & 3, jt = (i >> 8) & 1, st = i >> 9;
            const int v = v0 + st * 16 + 4 * (ln >> 4) + r, j = jt * 16 + (ln & 15);
            s_wb[i] = (v < V && j < J) ? weights[(size_t)v * J + j] : 0.f;
        }
        for (int i = tid; i < kVT * 3; i += 64 * kWaves) s_t[i] = ((size_t)v0 * 3 + i < E) ? v_template[(size_t)v0 * 3 + i] : 0.f;
        __syncthreads();
        if (!active) continue;                         // (idle waves still take part in the staging and its barriers)

#pragma unroll 1
        for (int st = 0; st < 2; ++st) {
            sg_f4 am4[3 * JS];                         // am4[flat / 4][flat % 4], flat = e JS + js: A_f[4 js + fq][e]
            {
                const sg_f4 *ap = reinterpret_cast<const sg_f4 *>(Aws + (size_t)ftc * 3 * JS * 256) + lane;
#pragma unroll
                for (int i4 = 0; i4 < 3 * JS; ++i4) am4[i4] = ap[i4 * 64];
            }
            // the incoming gradient of the lane's four (vertex, frame) pairs
            float gg[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = v0 + st * 16 + 4 * fq + r;
                const bool ok = frame_ok && d_verts != nullptr && v < V;
                const float *gp = d_verts + ((size_t)(ok ? f : 0) * V + (ok ? v : 0)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) gg[r][c] = ok ? gp[c] : 0.f;
            }
            // v_posed^T: rows = the half's 16 vertices, columns = the tile's 16 frames, k ascending in every accumulator
            sg_f4 vp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) vp[c] = (sg_f4){0.f, 0.f, 0.f, 0.f};
            {
                const float *dl = sg_smem + (size_t)st * 3 * kKG * 256 + fq * 64 + ((fi ^ fq) << 2);
#pragma unroll
                for (int g = 0; g < kKG; ++g) {
                    sg_f4 a4[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) a4[c] = *reinterpret_cast<const sg_f4 *>(dl + (c * kKG + g) * 256);
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                        for (int c = 0; c < 3; ++c) vp[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[c][s4], cf4[g][s4], vp[c], 0, 0, 0);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) vp[c][r] += s_t[(st * 16 + 4 * fq + r) * 3 + c];
            float wfr[JS];
#pragma unroll
            for (int js = 0; js < JS; ++js) wfr[js] = s_w[(st * JS + js) * 64 + lane];
            sg_f4 dvp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dvp[c] = (sg_f4){0.f, 0.f, 0.f, 0.f};
            // row c of the transform: T[c][0..3] = W . A;  d v_posed += T[c][0..2] g_c;  dA[c][e] += W^T . (g_c [v_posed ; 1]_e)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sg_f4 T[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    T[e] = (sg_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int js = 0; js < JS; ++js) {
                        const int flat = (4 * c + e) * JS + js;
                        T[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wfr[js], am4[flat / 4][flat % 4], T[e], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int cp = 0; cp < 3; ++cp)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dvp[cp][r] = fmaf(T[cp][r], gg[r][c], dvp[cp][r]);
                sg_f4 pa[2][4];   // the half's 16 vertices on their own (4 instructions from zero), then added to the running sums
#pragma unroll
                for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) pa[jt][e] = (sg_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float wb[2];
#pragma unroll
                    for (int jt = 0; jt < 2; ++jt) wb[jt] = s_wb[((st * 2 + jt) * 4 + r) * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float p = e < 3 ? gg[r][c] * vp[e][r] : gg[r][c];
#pragma unroll
                        for (int jt = 0; jt < 2; ++jt) pa[jt][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[jt], p, pa[jt][e], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) dA[jt][4 * c + e] = dA[jt][4 * c + e] + pa[jt][e];
            }
            // dc: rows = 16 coefficients, columns = frames, k = the vertices 4 q + r of coordinate c.  The half's 48 products are summed on
            // their own (12 instructions from zero) and then added to the running sum: 8 additions per slab instead of a chain of 96
            {
                const float *bl = sg_smem + (size_t)st * 3 * kKG * 256 + (fi & 3) * 64 + (fi >> 2);
                sg_f4 part[kKG];
#pragma unroll
                for (int g = 0; g < kKG; ++g) part[g] = (sg_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int off = ((4 * fq + r) ^ (fi & 3)) << 2;
#pragma unroll
                        for (int g = 0; g < kKG; ++g)
                            part[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(bl[(c * kKG + g) * 256 + off], dvp[c][r], part[g], 0, 0, 0);
                    }
#pragma unroll
                for (int g = 0; g < kKG; ++g) dC[g] = dC[g] + part[g];
            }
        }
    }

    if (frame_ok) {   // lane (frame fi, rows 4 fq + r): joints 16 jt + 4 fq + r of dA, coefficients 16 g + 4 fq + r of dc
        const int rec = J * 12 + NC;
        float *o = slabs + ((size_t)slab * B + f) * rec;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jt * 16 + 4 * fq + r;
                if (j < J) {
#pragma unroll
                    for (int e = 0; e < 12; ++e) o[j * 12 + e] = dA[jt][e][r];
                }
            }
#pragma unroll
        for (int g = 0; g < kKG; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = g * 16 + 4 * fq + r;
                if (k < NC) o[J * 12 + k] = dC[g][r];
            }
    }
}

// sums[b][i] = slab 0 + slab 1 + ... (ascending, in float64, rounded once): one thread per (frame, entry), consecutive threads on consecutive
// entries -- the 26 MB of slabs at cfg4 stream through 474 workgroups instead of through the 240 waves of the per-frame kernel.
__global__ void __launch_bounds__(256) slab_sum_kernel(long long n, int nslab, const float *__restrict__ slabs, float *__restrict__ sums) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
#pragma unroll 6
    for (int s = 0; s < nslab; ++s) acc = acc + (double)slabs[(size_t)s * n + i];
    sums[i] = (float)acc;
}

// The per-frame part in float64: 24 joints' worth of arithmetic whose sums run along the whole kinematic chain (the root's dG^t is the sum of
// every joint's), where fp32 rounding would be the largest error of the whole adjoint.  Inputs and outputs stay fp32.
__device__ __forceinline__ void rigid_wave_f64(int l, int b, int J, int NB, int pose2rot, const float *__restrict__ betas, int betas_bstride,
                                               const float *__restrict__ pose, const float *__restrict__ Jt, const float *__restrict__ Js,
                                               const int *__restrict__ parents, double *R_, double *J_, double *L_, double *G_) {
    if (l < J) {
        double R[9];
        if (pose2rot) {   // lbs.py:330-345
            const float *pp = pose + ((size_t)b * J + l) * 3;
            const double rx = pp[0], ry = pp[1], rz = pp[2];
            const double ax = rx + 1e-8, ay = ry + 1e-8, az = rz + 1e-8;
            const double angle = sqrt(ax * ax + ay * ay + az * az);
            const double x = rx / angle, y = ry / angle, z = rz / angle;
            const double s = sin(angle), c1 = 1.0 - cos(angle);
            R[0] = 1.0 + c1 * (-(z * z + y * y)); R[1] = s * (-z) + c1 * (x * y);        R[2] = s * y + c1 * (x * z);
            R[3] = s * z + c1 * (x * y);          R[4] = 1.0 + c1 * (-(z * z + x * x)); R[5] = s * (-x) + c1 * (y * z);
            R[6] = s * (-y) + c1 * (x * z);       R[7] = s * x + c1 * (y * z);           R[8] = 1.0 + c1 * (-(y * y + x * x));
        } else {
            const float *pp = pose + ((size_t)b * J + l) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = pp[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) R_[l * 9 + k] = R[k];
        const float *be = betas + (size_t)b * betas_bstride;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double acc = Jt[l * 3 + r];
            for (int k = 0; k < NB; ++k) acc = fma((double)Js[(l * 3 + r) * NB + k], (double)be[k], acc);
            J_[l * 3 + r] = acc;
        }
    }
    wave_sync_lds();
    if (l < J) {
        const int p = chain_parent(parents, l);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            L_[l * 12 + r * 4 + 0] = R_[l * 9 + r * 3 + 0];
            L_[l * 12 + r * 4 + 1] = R_[l * 9 + r * 3 + 1];
            L_[l * 12 + r * 4 + 2] = R_[l * 9 + r * 3 + 2];
            L_[l * 12 + r * 4 + 3] = (l > 0) ? (J_[l * 3 + r] - J_[p * 3 + r]) : J_[l * 3 + r];
        }
    }
    wave_sync_lds();
    if (l < 12) G_[l] = L_[l];
    wave_sync_lds();
    for (int i = 1; i < J; ++i) {
        if (l < 12) {
            const int p = chain_parent(parents, i), r = l >> 2, c = l & 3;
            double acc = G_[p * 12 + r * 4 + 0] * L_[i * 12 + 0 * 4 + c];
            acc = fma(G_[p * 12 + r * 4 + 1], L_[i * 12 + 1 * 4 + c], acc);
            acc = fma(G_[p * 12 + r * 4 + 2], L_[i * 12 + 2 * 4 + c], acc);
            if (c == 3) acc += G_[p * 12 + r * 4 + 3];
            G_[i * 12 + l] = acc;
        }
        wave_sync_lds();
    }
}

__global__ void __launch_bounds__(128) grad_post_kernel(int B, int J, int NB, int pose2rot, const float *__restrict__ betas, int betas_bstride,
                                                        const float *__restrict__ pose, const float *__restrict__ Jt, const float *__restrict__ Js,
                                                        const int *__restrict__ parents, const float *__restrict__ sums,
                                                        const float *__restrict__ d_joints, float *__restrict__ d_pose, float *__restrict__ d_betas_rows) {
    __shared__ double sR_[2][kMaxJ * 9], sJ_[2][kMaxJ * 3], sL_[2][kMaxJ * 12], sG_[2][kMaxJ * 12];
    __shared__ double sdA_[2][kMaxJ * 12], sdG_[2][kMaxJ * 12], sdL_[2][kMaxJ * 12], sdJ_[2][kMaxJ * 3], sdc_[2][4 * kKS];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 2 + w;
    if (b >= B) return;   // (wave-local LDS exchange only: no workgroup barrier below)
    double *R_ = sR_[w], *J_ = sJ_[w], *L_ = sL_[w], *G_ = sG_[w], *dA = sdA_[w], *dG = sdG_[w], *dL = sdL_[w], *dJ = sdJ_[w], *dc = sdc_[w];
    const int NC = NB + (J - 1) * 9, rec = J * 12 + NC;
    rigid_wave_f64(l, b, J, NB, pose2rot, betas, betas_bstride, pose, Jt, Js, parents, R_, J_, L_, G_);
    for (int i = l; i < rec; i += 64) {   // the frame's summed slabs
        const double acc = sums[(size_t)b * rec + i];
        if (i < J * 12) dA[i] = acc; else dc[i - J * 12] = acc;
    }
    wave_sync_lds();
    if (l < J) {   // A_j = [G_j^R | G_j^t - G_j^R Jr_j], posed_j = G_j^t
        const double *a = dA + l * 12;
        const double jr[3] = {J_[l * 3 + 0], J_[l * 3 + 1], J_[l * 3 + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double at = a[r * 4 + 3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dG[l * 12 + r * 4 + c] = a[r * 4 + c] - at * jr[c];
            dG[l * 12 + r * 4 + 3] = at + (d_joints ? (double)d_joints[((size_t)b * J + l) * 3 + r] : 0.0);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            dJ[l * 3 + c] = -fma(G_[l * 12 + 8 + c], a[11], fma(G_[l * 12 + 4 + c], a[7], G_[l * 12 + c] * a[3]));
    }
    wave_sync_lds();
    for (int i = J - 1; i >= 1; --i) {   // G_i = G_p L_i:  dL_i = (G_p^R)^T dG_i,  dG_p += dG_i L_i^T (4x4, implicit row [0 0 0 1])
        if (l < 12) {
            const int p = chain_parent(parents, i), r = l >> 2, c = l & 3;
            const double dl = fma(G_[p * 12 + 8 + r], dG[i * 12 + 8 + c], fma(G_[p * 12 + 4 + r], dG[i * 12 + 4 + c], G_[p * 12 + r] * dG[i * 12 + c]));
            double add;
            if (c < 3) {
                add = dG[i * 12 + r * 4 + 0] * L_[i * 12 + c * 4 + 0];
                add = fma(dG[i * 12 + r * 4 + 1], L_[i * 12 + c * 4 + 1], add);
                add = fma(dG[i * 12 + r * 4 + 2], L_[i * 12 + c * 4 + 2], add);
                add = fma(dG[i * 12 + r * 4 + 3], L_[i * 12 + c * 4 + 3], add);
            } else {
                add = dG[i * 12 + r * 4 + 3];
            }
            dL[i * 12 + l] = dl;
            dG[p * 12 + l] = dG[p * 12 + l] + add;
        }
        wave_sync_lds();
    }
    if (l < 12) dL[l] = dG[l];   // G_0 = L_0
    wave_sync_lds();
    if (l < J) {
        // L_j^t = Jr_j - Jr_parent (j >= 1), L_0^t = Jr_0: this joint's own dt, minus its children's in ascending order
        double dj[3] = {dJ[l * 3 + 0] + dL[l * 12 + 3], dJ[l * 3 + 1] + dL[l * 12 + 7], dJ[l * 3 + 2] + dL[l * 12 + 11]};
        for (int i = l + 1; i < J; ++i)
            if (chain_parent(parents, i) == l) { dj[0] = dj[0] - dL[i * 12 + 3]; dj[1] = dj[1] - dL[i * 12 + 7]; dj[2] = dj[2] - dL[i * 12 + 11]; }
        double dR[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) dR[k] = dL[l * 12 + (k / 3) * 4 + (k % 3)] + (l > 0 ? dc[NB + (l - 1) * 9 + k] : 0.0);
        if (!pose2rot) {
            float *o = d_pose + ((size_t)b * J + l) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) o[k] = (float)dR[k];
        } else {
            // lbs.py:330-345, backwards: R = I + s K + c1 K K, K from dir = t / angle, angle = ||t + 1e-8||
            const float *pp = pose + ((size_t)b * J + l) * 3;
            const double rx = pp[0], ry = pp[1], rz = pp[2];
            const double ax = rx + 1e-8, ay = ry + 1e-8, az = rz + 1e-8;
            const double angle = sqrt(ax * ax + ay * ay + az * az);
            const double x = rx / angle, y = ry / angle, z = rz / angle;
            const double s = sin(angle), co = cos(angle), c1 = 1.0 - co;
            const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
            double KK[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) KK[r * 3 + c] = fma(K[r * 3 + 2], K[6 + c], fma(K[r * 3 + 1], K[3 + c], K[r * 3] * K[c]));
            double ds = 0.0, dc1 = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) { ds = fma(dR[k], K[k], ds); dc1 = fma(dR[k], KK[k], dc1); }
            double dK[9];   // s dR + c1 (dR K^T + K^T dR)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double m = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) m = fma(dR[r * 3 + k], K[c * 3 + k], fma(K[k * 3 + r], dR[k * 3 + c], m));
                    dK[r * 3 + c] = fma(c1, m, s * dR[r * 3 + c]);
                }
            const double ddx = dK[7] - dK[5], ddy = dK[2] - dK[6], ddz = dK[3] - dK[1];
            const double dangle = fma(dc1, s, ds * co) - fma(ddz, rz, fma(ddy, ry, ddx * rx)) / (angle * angle);
            float *o = d_pose + ((size_t)b * J + l) * 3;
            o[0] = (float)(ddx / angle + dangle * (ax / angle));
            o[1] = (float)(ddy / angle + dangle * (ay / angle));
            o[2] = (float)(ddz / angle + dangle * (az / angle));
        }
        dJ[l * 3 + 0] = dj[0]; dJ[l * 3 + 1] = dj[1]; dJ[l * 3 + 2] = dj[2];
    }
    wave_sync_lds();
    for (int k = l; k < NB; k += 64) {   // d betas = dc[:NB] + J_shapedirs^T dJr, joints and coordinates ascending
        double acc = dc[k];
        for (int i = 0; i < J * 3; ++i) acc = fma((double)Js[(size_t)i * NB + k], dJ[i], acc);
        d_betas_rows[(size_t)b * NB + k] = (float)acc;
    }
}

__global__ void __launch_bounds__(256) betas_sum_kernel(int B, int NB, const float *__restrict__ rows, float *__restrict__ d_betas) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= NB) return;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = acc + rows[(size_t)b * NB + k];
    d_betas[k] = acc;
}

static long long up4(long long n) { return (n + 3) / 4 * 4; }

struct WsLayout {
    long long c, a, slabs, sums, rows, total;   // float offsets, total in floats
};

static WsLayout ws_layout(int b, int v, int j, int nb) {
    const int js = j <= 24 ? 6 : 8;
    const long long ntile = ((long long)b + 15) / 16, nslab = (b > 0 && v > 0) ? ((long long)v + G4D_SMPL_SLAB_VERTS - 1) / G4D_SMPL_SLAB_VERTS : 0;
    WsLayout w;
    w.c = 0;
    w.a = w.c + ntile * kKG * 256;
    w.slabs = w.a + ntile * 3 * js * 256;
    const long long rec = (long long)j * 12 + nb + 9ll * (j - 1);
    w.sums = w.slabs + up4(nslab * b * rec);
    w.rows = w.sums + up4((long long)b * rec);
    w.total = w.rows + up4((long long)b * nb);
    return w;
}

}  // namespace g4d

using namespace g4d;

extern "C" int g4d_smpl_grad_supported(int j, int nb) {
    return j > 0 && j <= G4D_SMPL_MAX_JOINTS && nb >= 0 && nb <= G4D_SMPL_MAX_COEFFS && nb + (j - 1) * 9 <= G4D_SMPL_MAX_COEFFS;
}

extern "C" int g4d_smpl_grad_slabs(int b, int v) {
    if (b < 0 || v < 0) return -1;
    if (b == 0 || v == 0) return 0;
    return (int)(((long long)v + G4D_SMPL_SLAB_VERTS - 1) / G4D_SMPL_SLAB_VERTS);
}

extern "C" long long g4d_smpl_grad_ws_bytes(int b, int v, int j, int nb) {
    if (b < 0 || v < 0 || !g4d_smpl_grad_supported(j, nb)) return -1;
    return ws_layout(b, v, j, nb).total * (long long)sizeof(float);
}

extern "C" int g4d_smpl_lbs_grad_f32(int b, int v, int j, int nb, int pose2rot, const float *betas, int betas_bstride, const float *pose,
                                     const float *v_template, const float *blend_dirs, const float *J_template, const float *J_shapedirs,
                                     const int *parents, const float *lbs_weights, const float *d_verts, const float *d_joints, float *d_pose,
                                     float *d_betas, void *ws, long long ws_bytes, g4d_stream_t stream) {
    G4D_REQUIRE(b >= 0 && v >= 0, "g4d_smpl_lbs_grad_f32: negative size (b=%d, v=%d)", b, v);
    G4D_REQUIRE(g4d_smpl_grad_supported(j, nb), "g4d_smpl_lbs_grad_f32: need 1 <= J <= 32 and NB + 9 (J - 1) <= 224 (j=%d, nb=%d)", j, nb);
    G4D_REQUIRE(betas_bstride == 0 || betas_bstride == nb, "g4d_smpl_lbs_grad_f32: betas_bstride must be 0 or nb (%d)", betas_bstride);
    G4D_REQUIRE(b <= (1 << 20) && v <= (1 << 24), "g4d_smpl_lbs_grad_f32: too large (b=%d, v=%d)", b, v);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t pose_n = (size_t)b * j * (pose2rot ? 3 : 9), betas_n = (size_t)(betas_bstride == 0 ? 1 : b) * nb;
    if (b == 0 || v == 0) {   // an empty problem: zeros
        if (d_pose && pose_n && hipMemsetAsync(d_pose, 0, pose_n * sizeof(float), st) != hipSuccess) return check_launch("g4d_smpl_lbs_grad_f32 (zero)");
        if (d_betas && betas_n && hipMemsetAsync(d_betas, 0, betas_n * sizeof(float), st) != hipSuccess) return check_launch("g4d_smpl_lbs_grad_f32 (zero)");
        return G4D_OK;
    }
    G4D_REQUIRE(betas && pose && v_template && blend_dirs && J_template && J_shapedirs && parents && lbs_weights && d_pose && (d_betas || nb == 0) && ws,
                "g4d_smpl_lbs_grad_f32: null pointer");
    const WsLayout L = ws_layout(b, v, j, nb);
    G4D_REQUIRE(ws_bytes >= L.total * (long long)sizeof(float) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                "g4d_smpl_lbs_grad_f32: workspace too small or not 16-byte aligned");
    float *W = reinterpret_cast<float *>(ws), *Cws = W + L.c, *Aws = W + L.a, *slabs = W + L.slabs, *sums = W + L.sums, *rows = W + L.rows;
    const int js = j <= 24 ? 6 : 8, nc = nb + (j - 1) * 9, ntile = (b + 15) / 16, nslab = g4d_smpl_grad_slabs(b, v);
    hipLaunchKernelGGL(grad_pre_kernel, dim3(ntile * 4), dim3(256), 0, st, b, j, nb, js, pose2rot, betas, betas_bstride, pose, J_template, J_shapedirs,
                       parents, Cws, Aws);
    if (const int rc = check_launch("g4d_smpl_lbs_grad_f32 (frames)")) return rc;
    const int lds = (int)sizeof(float) * (kBlendFloats + 2 * js * 64 + 2 * 2 * 4 * 64 + kVT * 3 + 32);
    const dim3 grid((unsigned)nslab, (unsigned)((ntile + kWaves - 1) / kWaves));
    if (js == 6) {
        static unsigned long long attr = 0;
        if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(grad_main_kernel<6>), lds, attr, "g4d_smpl_lbs_grad_f32")) return rc;
        hipLaunchKernelGGL(grad_main_kernel<6>, grid, dim3(64 * kWaves), lds, st, b, v, j, nc, v_template, blend_dirs, lbs_weights, Cws, Aws, d_verts, slabs);
    } else {
        static unsigned long long attr = 0;
        if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(grad_main_kernel<8>), lds, attr, "g4d_smpl_lbs_grad_f32")) return rc;
        hipLaunchKernelGGL(grad_main_kernel<8>, grid, dim3(64 * kWaves), lds, st, b, v, j, nc, v_template, blend_dirs, lbs_weights, Cws, Aws, d_verts, slabs);
    }
    if (const int rc = check_launch("g4d_smpl_lbs_grad_f32 (vertices)")) return rc;
    const long long nsum = (long long)b * (j * 12 + nc);
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((nsum + 255) / 256)), dim3(256), 0, st, nsum, nslab, slabs, sums);
    if (const int rc = check_launch("g4d_smpl_lbs_grad_f32 (slabs)")) return rc;
    float *row_out = betas_bstride == 0 ? rows : d_betas;
    hipLaunchKernelGGL(grad_post_kernel, dim3((b + 1) / 2), dim3(128), 0, st, b, j, nb, pose2rot, betas, betas_bstride, pose, J_template, J_shapedirs,
                       parents, sums, d_joints, d_pose, row_out);
    if (const int rc = check_launch("g4d_smpl_lbs_grad_f32 (joints)")) return rc;
    if (betas_bstride == 0 && nb > 0) {
        hipLaunchKernelGGL(betas_sum_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, b, nb, rows, d_betas);
        return check_launch("g4d_smpl_lbs_grad_f32 (betas)");
    }
    return G4D_OK;
}

// Shared pieces of the MFMA shared-MLP kernels (mlp.hip: one layer per launch; mlp_stack.hip: up to four layers
// per launch with activations resident in LDS): argument block, per-row loader state and the element loader of
// the four A-operand sources (DIRECT / GROUP / INTERP / CSR) -- and, for the host side of the whole-stack launchers,
// the call description they all take (StackCall) with the checks they share.  Also the one home of the epilogue / loader pieces that the
// persistent kernels (sa_*.hip, fp_*.hip) share with them: pool4_rows_max, interp_weights.
#pragma once
#include "g4d_common.h"

namespace g4d {

enum { LOAD_DIRECT = 0, LOAD_GROUP = 1, LOAD_INTERP = 2, LOAD_CSR = 3 };

struct LinearArgs {
    // contraction
    int rows, K, Kpad, Cout;
    const float *W;      // [CoutPad64][Kpad] row-major, zero padded (packed once on the host side)
    const float *scale;  // [CoutPad64]
    const float *shift;  // [CoutPad64]
    int relu;
    // output
    float *out;
    int ldo, col0;
    int pool;  // 0 none, 1 max, 2 avg  over S consecutive rows
    int S;
    // DIRECT / CSR source
    const float *X;
    int ldx;
    // GROUP
    const float *xyz, *new_xyz, *feats;
    const int *idx;
    int N, P, C, use_xyz;
    // INTERP
    const float *known_feats, *skip, *dist2;
    const int *nn_idx;
    int C2, C1, m, n;
    // CSR
    const int *rowptr, *colidx;
    const float *vals;
    int Vg;
    // INTERP over a pre-contracted table (register-chain kernel only): the loader's row becomes relu(row * pre_scale + pre_shift)
    // and, when in_tap is set, is also written to in_tap[row * in_tap_ld + column]
    const float *pre_scale, *pre_shift;
    float *in_tap;
    int in_tap_ld;
    // INTERP WITH skip features (register-chain kernel only, C2 == 0 in these arguments): `tab` (stride tab_ld) holds the known features
    // already multiplied by the known-feature columns of the first layer's weight; the first layer's accumulators START from
    // three_interpolate(tab) and the matrix pipe adds the skip columns (K = C1).
    // GROUP over a pre-contracted table (register-chain kernel only): row j of `tab` (stride tab_ld) holds the feature part of the
    // first layer for source point j; the loader's row is relu((tab[j] + tab_wx . (x_j - q)) * pre_scale + pre_shift), tab_wx = [3][K]
    const float *tab, *tab_wx;
    int tab_ld;
    // INTERP over CELL-ORDERED rows (register-chain kernel only): row p of the launch is the p-th point of its cloud's ball-grid order
    // (dist2 / nn_idx are stored in that order); its skip features are read from, and its outputs written to, row perm(p) = the
    // original index kept in the 4th dword of the cloud's 16-byte grid records (perm_rec + cloud * perm_stride bytes).  NULL: rows in place.
    const unsigned char *perm_rec;
    size_t perm_stride;
    // live-cloud scope of the launch (g4d_common.h; count == nullptr: none).  Honoured by linear_kernel, gemm_narrow_kernel and gemm_tile_kernel;
    // every other kernel that takes a LinearArgs ignores it and computes all rows.
    LiveRows live;
};

// output / skip row of launch row `row` (see LinearArgs::perm_rec)
__device__ __forceinline__ int out_row(const LinearArgs &a, int row) {
    if (!a.perm_rec) return row;
    const int b = row / a.n, p = row - b * a.n;
    return b * a.n + reinterpret_cast<const int *>(a.perm_rec + (size_t)b * a.perm_stride)[4 * p + 3];
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// max over the 16 rows of FOUR row-major tiles at once.  v_c (c = 0..3) holds, in lane (fi, fq), a value already reduced over that lane's
// rows 4 fq + r; what is left is the max over the four 16-lane rows of the wave, per tile.  v_permlane16_swap(a, b) leaves
// {a.row0, b.row0, a.row2, b.row2} / {a.row1, b.row1, a.row3, b.row3}, so ONE swap + ONE max halves two tiles at once and parks them in
// alternating rows; v_permlane32_swap does the same for the two halves of the wave.  Result: lane 16 c + fi = max over all 16 rows of
// tile c at column fi -- 64 different outputs in one register (one 256-byte store) after 3 swaps + 3 max, where reducing the tiles one by
// one (lane_xor16 / lane_xor32: copies, swap, select, max per step) took ~40 instructions and four quarter-wave stores.
__device__ __forceinline__ float pool4_rows_max(float v0, float v1, float v2, float v3) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v2), __float_as_uint(v3), false, false);
    const float m01 = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));   // rows: tile 0 (fq 0|1), tile 1 (fq 0|1), tile 0 (fq 2|3), tile 1 (fq 2|3)
    const float m23 = fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
    const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(m01), __float_as_uint(m23), false, false);
    return fmaxf(__uint_as_float(c[0]), __uint_as_float(c[1]));              // rows: tile 0, tile 1, tile 2, tile 3
}

// The inverse-distance weights of three_interpolate from the three squared distances of three_nn (pointnet2_utils.py:98 sqrt;
// pointnet2_modules.py:140-142): a numerics contract -- these operations, each rounded, in this order -- that every kernel forming the
// weights on the fly shares by calling this.
struct InterpW { float w0, w1, w2; };
__device__ __forceinline__ InterpW interp_weights(float d0, float d1, float d2) {
    const float r0 = 1.0f / (__fsqrt_rn(d0) + 1e-8f), r1 = 1.0f / (__fsqrt_rn(d1) + 1e-8f), r2 = 1.0f / (__fsqrt_rn(d2) + 1e-8f);
    const float norm = (r0 + r1) + r2;
    return {r0 / norm, r1 / norm, r2 / norm};
}

// DIRECT launches with `tab` set (g4d_linear_interp_add_f32): the GEMM result of a row gets three_interpolate(tab) of that row added before the
// affine -- the known-feature part of a feature-propagation level's first layer, pre-contracted over the m known rows (conv(sum_i w_i f_i) =
// sum_i w_i conv(f_i); pointnet2_modules.py:139-149).  Weights as make_ctx<LOAD_INTERP> computes them; offsets in floats into `tab`.
struct InterpRow { float w0, w1, w2; size_t k0, k1, k2; };
__device__ __forceinline__ InterpRow interp_row(const LinearArgs &a, int row) {
    InterpRow c;
    const int b = row / a.n;
    const int *ix = a.nn_idx + (size_t)row * 3;
    const float *d2 = a.dist2 + (size_t)row * 3;
    const InterpW w = interp_weights(d2[0], d2[1], d2[2]);
    c.w0 = w.w0; c.w1 = w.w1; c.w2 = w.w2;
    c.k0 = ((size_t)b * a.m + ix[0]) * a.tab_ld; c.k1 = ((size_t)b * a.m + ix[1]) * a.tab_ld; c.k2 = ((size_t)b * a.m + ix[2]) * a.tab_ld;
    return c;
}
__device__ __forceinline__ float interp_at(const LinearArgs &a, const InterpRow &c, int ch) {
    return c.w0 * a.tab[c.k0 + ch] + c.w1 * a.tab[c.k1 + ch] + c.w2 * a.tab[c.k2 + ch];
}

// gemm_stream.hip: persistent row-streaming GEMM for tall DIRECT launches; returns false when the launch is not its kind
bool gemm_stream_try(const LinearArgs &a, hipStream_t s, int *rc);
bool gemm_narrow_try(const LinearArgs &a, hipStream_t s, int *rc);   // gemm_narrow.hip: K = Cout = 96, weights in registers
// gemm_tile.hip: 128 x 128-tile GEMM for tall DIRECT launches with a deep contraction; same contract
bool gemm_tile_try(const LinearArgs &a, hipStream_t s, int *rc);

// ---- the host side of a whole-stack launch --------------------------------------------------------------------------------------------
// ONE description of the call, from the C entry point down to the kernel launch: g4d_mlp_run and the positional entry points (api.hip) build it
// from a g4d_mlp_args, the table entry points (mlp_chain.hip) by naming the fields they set; the launchers and the persistent-kernel hooks below
// read it.  `in` reaches the kernels as it stands, apart from `rows` (checked against the family's limit first) and `S` (kept as the caller
// gave it -- the checks and the hooks look at that value -- and raised to 1 for the kernels): kernel_in().
struct StackCall {
    const char *name;   // the entry point that error texts speak of
    int mode;
    long long rows;
    LinearArgs in;      // loaders, pooling and output window; in.K = the first layer's input width
    int nlayers;        // HOST arrays of nlayers (W: 3 * nlayers pointers -- hi | mid | lo -- for g4d_mlp_chain_bf16x3)
    const void *const *W;
    const float *const *scale, *const *shift;
    const int *Kpad, *Cout, *relu;
    int tap_layer;      // with tap_out: the hidden layer whose output is also stored to HBM
    float *tap_out;
    int tap_ld;
    const void *unknown_grid;   // INTERP: ball-grid workspace of the unknown cloud, rows walked in its cell order (or NULL)
    void *ws;                   // g4d_mlp_chain_group_table_ws_f32: scratch of sa_table.hip's work list (g4d_sa_table_ws_bytes)
    long long ws_bytes;
};
inline bool has_layer_arrays(const StackCall &c) { return c.W && c.scale && c.shift && c.Kpad && c.Cout && c.relu && c.in.out; }
inline int tap_layer_of(const StackCall &c) { return c.tap_out ? c.tap_layer : -1; }
// LinearArgs::perm_rec (and *stride = perm_stride) of a launch whose rows walk the cell order of c.unknown_grid; no grid: NULL, rows in place
inline const unsigned char *cell_records(const StackCall &c, size_t *stride) {
    size_t off = 0;
    *stride = 0;
    if (!c.unknown_grid) return nullptr;
    grid_sorted_layout(c.in.n, &off, stride);
    return static_cast<const unsigned char *>(c.unknown_grid) + off;
}
inline LinearArgs kernel_in(const StackCall &c) {
    LinearArgs in = c.in;
    in.rows = (int)c.rows;
    in.S = c.in.S > 0 ? c.in.S : 1;
    return in;
}

// The checks the families share (api.hip), with what differs between them.  Mode, layer count, sizes | rows == 0: kEmptyLaunch, the launcher
// returns G4D_OK | array pointers, supported widths, pool window, every layer's pointers and padding, the tap.  A family's own checks run after.
constexpr int kEmptyLaunch = -2;   // private, like the hooks' -1 ("not its kind"): neither may leave through an extern "C" entry point
struct StackRules {
    const char *bad_mode;   // text of the mode check
    bool csr;               // mode 3 allowed
    int max_layers;         // 0: g4d_mlp_chain_supported() decides (register-chain kernels)
    long long max_rows;     // rows < max_rows
    int kpad_multiple, w_pieces;   // (w_pieces: weight pointers per layer)
};
int stack_call_check(const StackCall &c, const StackRules &r);

// the kernel families behind g4d_mlp_run, each in the file of its name (mlp_chain_bf16_run with c.unknown_grid: g4d_mlp_chain_cells_bf16)
int mlp_stack_f32_run(const StackCall &c, hipStream_t st);
int mlp_stack_bf16_run(const StackCall &c, hipStream_t st);
int mlp_wave_f32_run(const StackCall &c, hipStream_t st);
int mlp_chain_f32_run(const StackCall &c, hipStream_t st);
int mlp_chain_bf16_run(const StackCall &c, hipStream_t st);
int mlp_chain_bf16x3_run(const StackCall &c, hipStream_t st);

// The persistent forms of the register-chain launches: each takes the launch when it is its kind and returns -1 when it is not.
// fp_table.hip: g4d_mlp_chain_table(_cells)_f32 for the 128 -> 64 -> 32 -> <= 16 stack, software-pipelined; c.unknown_grid: rows in cell order
int fp_table_try(const StackCall &c, hipStream_t st);
// fp_init.hip: g4d_mlp_chain_interp_init_f32 for the skip 96 -> 256 -> 128 -> 128 stack, weights shared through LDS
int fp_init_try(const StackCall &c, hipStream_t st);
// fp_head_bf16.hip: g4d_mlp_chain_bf16 (interpolating mode) for the 128 -> 128 -> 64 -> 32 -> <= 16 stack of config 3; c.unknown_grid as above
int fp_head_bf16_try(const StackCall &c, hipStream_t st);
// sa_group_bf16.hip: g4d_mlp_chain_bf16 (grouping mode) for the encoder's three-layer SA stacks
int sa_group_bf16_try(const StackCall &c, hipStream_t st);
// sa_table.hip: g4d_mlp_chain_group_table_f32 for large launches, software-pipelined; c.ws: scratch for the work list that skips blocks of padding
int sa_table_try(const StackCall &c, hipStream_t st);

template <int MODE>
struct RowCtx {  // per-thread, per-row state reused across K chunks
    bool valid;
    // GROUP
    size_t pt_base;   // (b*N + j)
    float cx, cy, cz;
    // INTERP
    size_t k0, k1, k2, sk;
    float w0, w1, w2;
    // CSR
    int f, beg, end;
};

template <int MODE>
__device__ __forceinline__ RowCtx<MODE> make_ctx(const LinearArgs &a, int row) {
    RowCtx<MODE> c;
    c.valid = row < a.rows;
    if (!c.valid) return c;
    if constexpr (MODE == LOAD_GROUP) {
        const int q = row / a.S;  // (b*P + p)
        const int b = q / a.P;
        const int j = a.idx[row];
        c.pt_base = (size_t)b * a.N + j;
        const float *ctr = a.new_xyz + (size_t)q * 3;
        c.cx = ctr[0]; c.cy = ctr[1]; c.cz = ctr[2];
    } else if constexpr (MODE == LOAD_INTERP) {
        const int b = row / a.n;
        const int *ix = a.nn_idx + (size_t)row * 3;
        const float *d2 = a.dist2 + (size_t)row * 3;
        const InterpW w = interp_weights(d2[0], d2[1], d2[2]);
        c.w0 = w.w0; c.w1 = w.w1; c.w2 = w.w2;
        const size_t ks = (a.tab && a.C2 == 0) ? (size_t)a.tab_ld : (size_t)a.C2;   // register-chain kernel with an accumulator-init table: offsets into it
        c.k0 = ((size_t)b * a.m + ix[0]) * ks;
        c.k1 = ((size_t)b * a.m + ix[1]) * ks;
        c.k2 = ((size_t)b * a.m + ix[2]) * ks;
        c.sk = (size_t)(a.C1 ? out_row(a, row) : row) * a.C1;
    } else if constexpr (MODE == LOAD_CSR) {
        c.f = row / a.Vg;
        const int v = row - c.f * a.Vg;
        c.beg = a.rowptr[v];
        c.end = a.rowptr[v + 1];
    }
    return c;
}

template <int MODE>
__device__ __forceinline__ float load_elem(const LinearArgs &a, const RowCtx<MODE> &c, int row, int k) {
    if (!c.valid || k >= a.K) return 0.f;
    if constexpr (MODE == LOAD_DIRECT) {
        return a.X[(size_t)row * a.ldx + k];
    } else if constexpr (MODE == LOAD_GROUP) {
        if (a.use_xyz) {
            if (k < 3) {
                const float g = a.xyz[c.pt_base * 3 + k];
                return g - (k == 0 ? c.cx : (k == 1 ? c.cy : c.cz));
            }
            return a.feats[c.pt_base * a.C + (k - 3)];
        }
        return a.feats[c.pt_base * a.C + k];
    } else if constexpr (MODE == LOAD_INTERP) {
        if (k < a.C2) return c.w0 * a.known_feats[c.k0 + k] + c.w1 * a.known_feats[c.k1 + k] + c.w2 * a.known_feats[c.k2 + k];
        return a.skip[c.sk + (k - a.C2)];
    } else {
        float s = 0.f;
        for (int e = c.beg; e < c.end; ++e) s += a.vals[e] * a.X[((size_t)c.f * a.Vg + a.colidx[e]) * a.ldx + k];
        return s;
    }
}

}  // namespace g4d

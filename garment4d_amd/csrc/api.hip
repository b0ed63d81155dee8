// Library-level entry points of libg4d_hip: version + thread-local error text, tuning switches, and the C doors of the whole-stack MLP launchers.
#include <stdarg.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "mlp_common.h"

namespace g4d {
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Distance contraction mode (include/g4d.h).  -1 = not initialised: first use reads G4D_DIST_CONTRACT.
static int g_contract = -1;

static int parse_contract(const char *e) {
    if (!e || !*e) return G4D_CONTRACT_NVCC;
    if (!strcmp(e, "0") || !strcmp(e, "off") || !strcmp(e, "none")) return G4D_CONTRACT_OFF;
    if (!strcmp(e, "2") || !strcmp(e, "chain") || !strcmp(e, "inner")) return G4D_CONTRACT_CHAIN;
    return G4D_CONTRACT_NVCC;
}

// per host thread override (-1: none): what a launcher called on this thread uses; the process-wide mode is only the default
static thread_local int t_contract = -1;

int distance_contraction() {
    if (t_contract >= 0) return t_contract;
    int m = __atomic_load_n(&g_contract, __ATOMIC_RELAXED);
    if (m < 0) {
        m = parse_contract(getenv("G4D_DIST_CONTRACT"));
        __atomic_store_n(&g_contract, m, __ATOMIC_RELAXED);
    }
    return m;
}
}  // namespace g4d

// ---- run-time tuning switches of the large-launch kernels (A/B experiments and tests that must drive a small shape through a kernel that would
// otherwise only see large ones).  A value set here wins over the environment variable of the same name in upper case with a G4D_ prefix
// (G4D_SA_TABLE_MIN_ROWS, ...), which wins over the built-in default.  Process-wide, like the distance contraction mode.
namespace g4d {
namespace {
struct Tune { const char *key; long long value; int state; };   // state: 0 unset, 1 from the environment / default (cached), 2 set by g4d_tuning_set
Tune g_tune[] = {{"sa_table_persistent", 0, 0}, {"sa_table_min_rows", 0, 0}, {"sa_table_128", 0, 0}, {"sa_table_oversub", 0, 0}, {"sa_table_dedup", 0, 0}, {"fp_table_persistent", 0, 0},
                 {"fp_table_min_rows", 0, 0}, {"gemm_tile", 0, 0}, {"gemm_tile_min_rows", 0, 0}, {"gemm_tile_min_cout", 0, 0}, {"gemm_tile_min_kpad", 0, 0}, {"fp_init_persistent", 0, 0}, {"fp_init_min_rows", 0, 0},
                 {"fp_head_bf16_persistent", 0, 0}, {"fp_head_bf16_min_rows", 0, 0}, {"sa_group_bf16_persistent", 0, 0}, {"sa_group_bf16_min_rows", 0, 0}};
}
// per-host-thread overrides (g4d_tuning_set_thread): an executor that holds its own tuning applies it around its launches without touching
// the process-wide table -- two executors driven from two threads do not see each other's settings (kernel selection happens on the host, at
// launch time, on the launching thread)
struct ThreadTune { long long value; bool set; };
thread_local ThreadTune t_tune[sizeof(g_tune) / sizeof(g_tune[0])] = {};

long long tuning(const char *key, long long dflt) {
    int i = 0;
    for (Tune &t : g_tune) {
        const int slot = i++;
        if (strcmp(t.key, key)) continue;
        if (t_tune[slot].set) return t_tune[slot].value;
        int st = __atomic_load_n(&t.state, __ATOMIC_ACQUIRE);
        if (st == 0) {
            char env[64] = "G4D_";
            size_t n = 4;
            for (const char *c = key; *c && n + 1 < sizeof(env); ++c) env[n++] = (char)((*c >= 'a' && *c <= 'z') ? *c - 32 : *c);
            env[n] = 0;
            const char *e = getenv(env);
            const long long v = e && *e ? atoll(e) : dflt;
            // state 0 -> 3 (being initialised) by ONE thread; a concurrent g4d_tuning_set (state 2) is never overwritten, a concurrent reader
            // that loses the race computes the same value from the same environment and returns it without storing
            int expect = 0;
            if (__atomic_compare_exchange_n(&t.state, &expect, 3, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
                __atomic_store_n(&t.value, v, __ATOMIC_RELAXED);
                expect = 3;
                __atomic_compare_exchange_n(&t.state, &expect, 1, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
                return v;
            }
            st = expect;
            if (st == 3) return v;
        }
        return __atomic_load_n(&t.value, __ATOMIC_RELAXED);
    }
    return dflt;
}
}  // namespace g4d

extern "C" int g4d_tuning_set(const char *key, long long value) {
    if (key)
        for (g4d::Tune &t : g4d::g_tune)
            if (!strcmp(t.key, key)) {
                __atomic_store_n(&t.value, value, __ATOMIC_RELAXED);
                __atomic_store_n(&t.state, 2, __ATOMIC_RELEASE);
                return G4D_OK;
            }
    g4d::set_error("g4d_tuning_set: unknown key '%s'", key ? key : "(null)");
    return G4D_EINVAL;
}

// set != 0: `value` overrides the key for launches made by the CALLING host thread; set == 0: the override is dropped (value ignored).
extern "C" int g4d_tuning_set_thread(const char *key, long long value, int set) {
    if (key) {
        int i = 0;
        for (g4d::Tune &t : g4d::g_tune) {
            const int slot = i++;
            if (!strcmp(t.key, key)) {
                g4d::t_tune[slot].value = value;
                g4d::t_tune[slot].set = set != 0;
                return G4D_OK;
            }
        }
    }
    g4d::set_error("g4d_tuning_set_thread: unknown key '%s'", key ? key : "(null)");
    return G4D_EINVAL;
}

// ---- live-cloud scope (include/g4d_live.h): per host thread, like the tuning overrides -- launchers ask on the thread that launches / captures
#include "../../include/g4d_live.h"
namespace g4d {
static thread_local const int *t_live_count = nullptr;
static thread_local int t_live_cap = 0;
LiveRows live_for_clouds(long long b, long long rows_per_cloud) {
    if (!t_live_count || b != t_live_cap || rows_per_cloud <= 0 || rows_per_cloud * b >= (1ll << 31)) return {nullptr, 0, 0};
    return {t_live_count, t_live_cap, (int)rows_per_cloud};
}
LiveRows live_for_rows(long long rows) {
    if (!t_live_count || rows <= 0 || rows % t_live_cap != 0) return {nullptr, 0, 0};
    return live_for_clouds(t_live_cap, rows / t_live_cap);
}
}  // namespace g4d

extern "C" int g4d_live_scope_begin(const int *live_clouds_dev, int capacity_clouds) {
    G4D_REQUIRE(live_clouds_dev && capacity_clouds >= 1, "g4d_live_scope_begin: needs a device pointer and a capacity >= 1");
    G4D_REQUIRE(!g4d::t_live_count, "g4d_live_scope_begin: a scope of %d clouds is already open on this thread (scopes do not nest)", g4d::t_live_cap);
    g4d::t_live_count = live_clouds_dev;
    g4d::t_live_cap = capacity_clouds;
    return G4D_OK;
}
extern "C" int g4d_live_scope_end(void) {
    G4D_REQUIRE(g4d::t_live_count, "g4d_live_scope_end: no scope is open on this thread");
    g4d::t_live_count = nullptr;
    g4d::t_live_cap = 0;
    return G4D_OK;
}
extern "C" int g4d_live_scope_capacity(void) { return g4d::t_live_count ? g4d::t_live_cap : 0; }
extern "C" long long g4d_live_scope_rows_per_cloud(long long clouds, long long rows) {
    if (clouds == 0) return 0;
    const g4d::LiveRows l = clouds < 0 ? g4d::live_for_rows(rows) : (rows % clouds == 0 ? g4d::live_for_clouds(clouds, rows / clouds) : g4d::LiveRows{nullptr, 0, 0});
    return l.count ? l.per_cloud : 0;
}

extern "C" int g4d_version(void) { return 263; /* 263: g4d_pos_encode_grad_f32, g4d_temporal_attention_grad_f32 (+ size queries) added, none changed; 262: g4d_spmm_rows_grad_f32, g4d_col_sum_rows_f32, g4d_gemm_tn_f32 (+ size queries) added, none changed; 261: g4d_mgn_skin_f32 added, none changed; 260 = round 6: g4d_mlp_run / g4d_mlp_args, g4d_mlp_chain_group_table_ws_f32 + g4d_sa_table_ws_bytes / _supported (include/g4d.h); 206: round 2 */ }
extern "C" const char *g4d_last_error(void) { return g4d::g_err; }

extern "C" int g4d_get_distance_contraction(void) { return g4d::distance_contraction(); }
extern "C" int g4d_set_distance_contraction_thread(int mode) {
    const int prev = g4d::t_contract;
    if (mode < -1 || mode > G4D_CONTRACT_CHAIN) {
        g4d::set_error("g4d_set_distance_contraction_thread: mode %d is not -1 (no override) or one of G4D_CONTRACT_OFF/NVCC/CHAIN", mode);
        return -2;
    }
    g4d::t_contract = mode;
    return prev;
}

extern "C" int g4d_set_distance_contraction(int mode) {
    const int saved = g4d::t_contract;
    g4d::t_contract = -1;
    const int prev = g4d::distance_contraction();   // the process-wide mode, not this thread's override
    g4d::t_contract = saved;
    if (mode < G4D_CONTRACT_OFF || mode > G4D_CONTRACT_CHAIN) {
        g4d::set_error("g4d_set_distance_contraction: mode %d is not one of G4D_CONTRACT_OFF/NVCC/CHAIN", mode);
        return -1;
    }
    __atomic_store_n(&g4d::g_contract, mode, __ATOMIC_RELAXED);
    return prev;
}

// ---- g4d_copy_segments_f32: up to 4 device-to-device copies in ONE launch (the executor's per-step input hand-over: cloud, betas, pose --
// three runtime copy kernels cost a coalesced call of 30 steps 90 launches, ~0.5 ms of its 6)
namespace g4d {
struct CopySegs { float *dst[4]; const float *src[4]; long long n[4]; long long first_block[5]; };
__global__ void __launch_bounds__(256) copy_segments_kernel(const CopySegs c, int nseg) {
    int s = 0;
    while (s + 1 < nseg && (long long)blockIdx.x >= c.first_block[s + 1]) ++s;
    const long long i0 = ((long long)blockIdx.x - c.first_block[s]) * 1024 + threadIdx.x * 4;
    float *d = c.dst[s];
    const float *p = c.src[s];
    const long long n = c.n[s];
    if (i0 + 3 < n && ((reinterpret_cast<size_t>(d) | reinterpret_cast<size_t>(p)) & 15) == 0) {
        *reinterpret_cast<float4 *>(d + i0) = *reinterpret_cast<const float4 *>(p + i0);
    } else {
        for (int e = 0; e < 4; ++e)
            if (i0 + e < n) d[i0 + e] = p[i0 + e];
    }
}
}  // namespace g4d

extern "C" int g4d_copy_segments_f32(int nseg, float *const *dst, const float *const *src, const long long *nfloats, g4d_stream_t stream) {
    G4D_REQUIRE(nseg >= 0 && nseg <= 4 && (nseg == 0 || (dst && src && nfloats)), "g4d_copy_segments_f32: 0..4 segments");
    g4d::CopySegs c = {};
    long long blocks = 0;
    int k = 0;
    for (int i = 0; i < nseg; ++i) {
        G4D_REQUIRE(nfloats[i] >= 0 && (nfloats[i] == 0 || (dst[i] && src[i])), "g4d_copy_segments_f32: bad segment %d", i);
        if (nfloats[i] == 0) continue;
        c.dst[k] = dst[i]; c.src[k] = src[i]; c.n[k] = nfloats[i]; c.first_block[k] = blocks;
        blocks += (nfloats[i] + 1023) / 1024;
        ++k;
    }
    if (k == 0) return G4D_OK;
    c.first_block[k] = blocks;
    G4D_REQUIRE(blocks < (1ll << 31), "g4d_copy_segments_f32: too large");
    hipLaunchKernelGGL(g4d::copy_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), c, k);
    return g4d::check_launch("g4d_copy_segments_f32");
}

// ---- the whole-stack launchers behind ONE argument block (include/g4d.h): g4d_mlp_run and the seven positional entry points --------------
// Both doors end in the same StackCall (mlp_common.h) handed to the family's launcher; nothing below them takes positional arguments.
namespace g4d {
static StackCall stack_call(const char *name, const g4d_mlp_args &a) {
    StackCall c = {};
    c.name = name; c.mode = a.mode; c.rows = a.rows;
    LinearArgs &in = c.in;
    in.K = a.K0; in.out = a.out; in.ldo = a.ldo; in.col0 = a.col0; in.pool = a.pool; in.S = a.S;
    in.X = a.X; in.ldx = a.ldx;
    in.xyz = a.xyz; in.new_xyz = a.new_xyz; in.feats = a.feats; in.idx = a.idx; in.N = a.N; in.P = a.P; in.C = a.C; in.use_xyz = a.use_xyz;
    in.known_feats = a.known_feats; in.skip = a.skip; in.dist2 = a.dist2; in.nn_idx = a.nn_idx; in.C2 = a.C2; in.C1 = a.C1; in.m = a.m; in.n = a.n;
    in.rowptr = a.rowptr; in.colidx = a.colidx; in.vals = a.vals; in.Vg = a.Vg;
    c.nlayers = a.nlayers; c.W = a.W; c.scale = a.scale; c.shift = a.shift; c.Kpad = a.Kpad; c.Cout = a.Cout; c.relu = a.relu;
    c.tap_layer = a.tap_layer; c.tap_out = a.tap_out; c.tap_ld = a.tap_ld; c.unknown_grid = a.unknown_grid;
    return c;
}

int stack_call_check(const StackCall &c, const StackRules &r) {
    const int S = c.in.S, pool = c.in.pool;
    G4D_REQUIRE(c.mode >= 0 && c.mode <= (r.csr ? LOAD_CSR : LOAD_INTERP), "%s: %s", c.name, r.bad_mode);
    if (r.max_layers) G4D_REQUIRE(c.nlayers >= 1 && c.nlayers <= r.max_layers, "%s: 1..%d layers", c.name, r.max_layers);
    G4D_REQUIRE(c.rows >= 0 && c.rows < r.max_rows && c.in.K > 0, "%s: bad sizes", c.name);
    if (c.rows == 0) return kEmptyLaunch;
    G4D_REQUIRE(has_layer_arrays(c), "%s: null pointer", c.name);
    if (!r.max_layers) G4D_REQUIRE(g4d_mlp_chain_supported(c.nlayers, c.Cout), "%s: unsupported layer widths (see g4d_mlp_chain_supported)", c.name);
    G4D_REQUIRE(pool >= 0 && pool <= 2, "%s: pool must be 0|1|2", c.name);
    if (pool) G4D_REQUIRE((S == 4 || S == 8 || S == 16 || S == 32 || S == 64) && c.rows % S == 0, "%s: pooling needs S in {4,8,16,32,64}", c.name);
    for (int l = 0; l < c.nlayers; ++l) {
        const void *const *Wl = c.W + (size_t)l * r.w_pieces;   // w_pieces consecutive pointers per layer: hi[, mid, lo]
        G4D_REQUIRE(Wl[0] && (r.w_pieces == 1 || (Wl[1] && Wl[2])) && c.scale[l] && c.shift[l] && c.Kpad[l] % r.kpad_multiple == 0 && c.Cout[l] > 0, "%s: bad layer %d", c.name, l);
    }
    G4D_REQUIRE(tap_layer_of(c) < c.nlayers - 1, "%s: tap must be a hidden layer", c.name);
    return G4D_OK;
}
}  // namespace g4d

extern "C" unsigned g4d_mlp_args_size(void) { return (unsigned)sizeof(g4d_mlp_args); }

extern "C" int g4d_mlp_run(int family, const g4d_mlp_args *args, g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(args, "g4d_mlp_run: null argument block");
    G4D_REQUIRE(args->version == G4D_MLP_ARGS_VERSION, "g4d_mlp_run: argument block version %u, this library speaks %d", args->version, G4D_MLP_ARGS_VERSION);
    G4D_REQUIRE(args->size >= 16 && args->size <= sizeof(g4d_mlp_args), "g4d_mlp_run: argument block of %u bytes, this library's is %u (a newer caller?)",
                args->size, (unsigned)sizeof(g4d_mlp_args));
    g4d_mlp_args a;
    memset(&a, 0, sizeof(a));
    memcpy(&a, args, args->size);                 // an older caller's shorter block: the appended fields read as zero
    if (args->size < offsetof(g4d_mlp_args, tap_layer) + sizeof(int)) a.tap_layer = -1;   // ... but a tap layer it does not hold WHOLE reads as "none"
    if (family != G4D_MLP_CHAIN_BF16) a.unknown_grid = nullptr;   // (the one family whose positional forms take it)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (family) {
        case G4D_MLP_STACK_F32: return mlp_stack_f32_run(stack_call("g4d_mlp_stack_f32", a), st);
        case G4D_MLP_STACK_BF16: return mlp_stack_bf16_run(stack_call("g4d_mlp_stack_bf16", a), st);
        case G4D_MLP_WAVE_F32: return mlp_wave_f32_run(stack_call("g4d_mlp_wave_f32", a), st);
        case G4D_MLP_CHAIN_F32: return mlp_chain_f32_run(stack_call("g4d_mlp_chain_f32", a), st);
        case G4D_MLP_CHAIN_BF16: return mlp_chain_bf16_run(stack_call("g4d_mlp_chain_bf16", a), st);   // (with a.unknown_grid: g4d_mlp_chain_cells_bf16)
        case G4D_MLP_CHAIN_BF16X3: return mlp_chain_bf16x3_run(stack_call("g4d_mlp_chain_bf16x3", a), st);
    }
    set_error("g4d_mlp_run: unknown kernel family %d", family);
    return G4D_EINVAL;
}

// The positional entry points: the arguments go into a g4d_mlp_args and through g4d_mlp_run.  The 33 arguments all seven share are spelled
// ONCE, here (parameters, and the names in the same order for pack_args); each entry point adds its own (CSR loader, grid) by field name.
#define G4D_MLP_LOADERS                                                                                                                       \
    int mode, long long rows, int K0, /* DIRECT / CSR */ const float *X, int ldx,                                                            \
    /* GROUP  */ int N, int P, int S, int C, int use_xyz, const float *xyz, const float *new_xyz, const float *feats, const int *idx,        \
    /* INTERP */ int n, int m, int C2, int C1, const float *known_feats, const float *skip, const float *dist2, const int *nn_idx
#define G4D_MLP_LAYERS(WT)                                                                                                                    \
    int nlayers, const WT *const *W, const float *const *scale, const float *const *shift, const int *Kpad, const int *Cout, const int *relu, \
    /* output */ int pool, float *out, int ldo, int col0
#define G4D_MLP_COMMON                                                                                                                        \
    mode, rows, K0, X, ldx, N, P, S, C, use_xyz, xyz, new_xyz, feats, idx, n, m, C2, C1, known_feats, skip, dist2, nn_idx, nlayers,         \
    reinterpret_cast<const void *const *>(W), scale, shift, Kpad, Cout, relu, pool, out, ldo, col0

static g4d_mlp_args pack_args(G4D_MLP_LOADERS, G4D_MLP_LAYERS(void), int tap_layer = -1, float *tap_out = nullptr, int tap_ld = 0) {
    g4d_mlp_args a;
    memset(&a, 0, sizeof(a));
    a.size = (unsigned)sizeof(a); a.version = G4D_MLP_ARGS_VERSION;
    a.mode = mode; a.rows = rows; a.K0 = K0; a.X = X; a.ldx = ldx;
    a.N = N; a.P = P; a.S = S; a.C = C; a.use_xyz = use_xyz; a.xyz = xyz; a.new_xyz = new_xyz; a.feats = feats; a.idx = idx;
    a.n = n; a.m = m; a.C2 = C2; a.C1 = C1; a.known_feats = known_feats; a.skip = skip; a.dist2 = dist2; a.nn_idx = nn_idx;
    a.nlayers = nlayers; a.W = W; a.scale = scale; a.shift = shift; a.Kpad = Kpad; a.Cout = Cout; a.relu = relu;
    a.pool = pool; a.out = out; a.ldo = ldo; a.col0 = col0; a.tap_layer = tap_layer; a.tap_out = tap_out; a.tap_ld = tap_ld;
    return a;
}

// One C entry point for all loaders: `mode` 0 DIRECT, 1 GROUP, 2 INTERP, 3 CSR; loader pointers that a mode does
// not use are ignored.  Layer descriptors arrive as parallel arrays (host memory) of length nlayers <= 4.
extern "C" int g4d_mlp_stack_f32(G4D_MLP_LOADERS, /* CSR */ int Vg, const int *rowptr, const int *colidx, const float *vals, G4D_MLP_LAYERS(float),
                                 int tap_layer, float *tap_out, int tap_ld, g4d_stream_t stream) {
    g4d_mlp_args a = pack_args(G4D_MLP_COMMON, tap_layer, tap_out, tap_ld);
    a.Vg = Vg; a.rowptr = rowptr; a.colidx = colidx; a.vals = vals;
    return g4d_mlp_run(G4D_MLP_STACK_F32, &a, stream);
}

extern "C" int g4d_mlp_stack_bf16(G4D_MLP_LOADERS, /* CSR */ int Vg, const int *rowptr, const int *colidx, const float *vals, G4D_MLP_LAYERS(unsigned short),
                                  int tap_layer, float *tap_out, int tap_ld, g4d_stream_t stream) {
    g4d_mlp_args a = pack_args(G4D_MLP_COMMON, tap_layer, tap_out, tap_ld);
    a.Vg = Vg; a.rowptr = rowptr; a.colidx = colidx; a.vals = vals;
    return g4d_mlp_run(G4D_MLP_STACK_BF16, &a, stream);
}

extern "C" int g4d_mlp_wave_f32(G4D_MLP_LOADERS, /* CSR */ int Vg, const int *rowptr, const int *colidx, const float *vals, G4D_MLP_LAYERS(float),
                                g4d_stream_t stream) {
    g4d_mlp_args a = pack_args(G4D_MLP_COMMON);
    a.Vg = Vg; a.rowptr = rowptr; a.colidx = colidx; a.vals = vals;
    return g4d_mlp_run(G4D_MLP_WAVE_F32, &a, stream);
}

extern "C" int g4d_mlp_chain_f32(G4D_MLP_LOADERS, G4D_MLP_LAYERS(float), int tap_layer, float *tap_out, int tap_ld, g4d_stream_t stream) {
    g4d_mlp_args a = pack_args(G4D_MLP_COMMON, tap_layer, tap_out, tap_ld);
    return g4d_mlp_run(G4D_MLP_CHAIN_F32, &a, stream);
}

extern "C" int g4d_mlp_chain_bf16(G4D_MLP_LOADERS, G4D_MLP_LAYERS(unsigned short), int tap_layer, float *tap_out, int tap_ld, g4d_stream_t stream) {
    g4d_mlp_args a = pack_args(G4D_MLP_COMMON, tap_layer, tap_out, tap_ld);
    return g4d_mlp_run(G4D_MLP_CHAIN_BF16, &a, stream);
}

extern "C" int g4d_mlp_chain_cells_bf16(G4D_MLP_LOADERS, G4D_MLP_LAYERS(unsigned short), int tap_layer, float *tap_out, int tap_ld, const void *unknown_grid,
                                        g4d_stream_t stream) {
    g4d_mlp_args a = pack_args(G4D_MLP_COMMON, tap_layer, tap_out, tap_ld);
    a.unknown_grid = unknown_grid;
    return g4d_mlp_run(G4D_MLP_CHAIN_BF16, &a, stream);
}

extern "C" int g4d_mlp_chain_bf16x3(G4D_MLP_LOADERS, G4D_MLP_LAYERS(unsigned short), int tap_layer, float *tap_out, int tap_ld, g4d_stream_t stream) {
    g4d_mlp_args a = pack_args(G4D_MLP_COMMON, tap_layer, tap_out, tap_ld);
    return g4d_mlp_run(G4D_MLP_CHAIN_BF16X3, &a, stream);
}

"""float64 numpy references for the forward kernels of the refinement head's inference path -- g4d_spmm_rows_f32 (csrc/pointnet2_ops.hip),
g4d_gcn_agg_linear(_meta)_f32 / g4d_gcn_tile_meta_build (csrc/gcn_fused.hip), g4d_temporal_attention_f32 (csrc/attention.hip) -- and the
builders of the inputs that drive them to their tile edges.

Every reference is a float64 evaluation of the same operation from the same fp32 inputs, with a per-element bound DERIVED from the kernel's
operation order (the derivations stand in the docstrings; u = 2^-24 and gamma(n) = n u / (1 - n u) as in tests/model_kernels_twin.py).  The one
quantity the sources cannot give is the accuracy of expf: EXPF_ULPS below, twice a full sweep's measured maximum.
tile_plan / attention_layout restate the launch arithmetic in plain Python, so that a test can prove which path a case took.

Not a test module: tests/test_refine_forward_cpu.py ties the twins to the oracle, asserts every case's precondition and shows that an fp32
restatement of each kernel stays inside its bound; tests/test_refine_forward_gpu.py runs the kernels against them."""
import functools
import math

import numpy as np

from model_kernels_twin import U, gamma

F32, F64 = np.float32, np.float64

K_ELL = 8                            # padded (offset, weight) pairs per row on the FAST path (gcn_fused.hip kEll)
K_WIN = {128: 288, 64: 224}          # tile rows -> window rows kept in LDS (Geo<TILE>::kWin)
KC = 128                             # support width of the fused kernel
EMPTY_LO = 0x7FFFFFFF                # window bounds of a tile without entries: [0x7fffffff, 0)

# v_mfma_f32_16x16x4_f32 adds FOUR products to an fp32 accumulator; the order and the width of those four additions inside the instruction
# are not documented.  Assumed here, conservatively: each product is rounded to fp32 and each of the four additions rounds.  One output of
# the fused contraction is 128 products through 32 chained MFMAs: the first product then passes its own rounding and 4 * 32 additions.
N_MFMA = 1 + 4 * 32

# expf of the library's build (OCML, -O3 -ffp-contract=off, no fast-math) against float64 exp over EVERY fp32 argument in [-104, -2^-126],
# 1,112,539,137 of them, on MI355X: the measured maximum is 0.8567 ulp of the true result wherever that is a normal number (at x = -5.28543615;
# 1.41 u relative), and 1 ulp of 2^-149 below (nothing is flushed).  No document installed with ROCm states a figure.
# Twice the measured maximum, rounded up to a whole ulp.  One ulp is at most 2^-23 = 2 u relative.
EXPF_ULPS = 2
EXPF_REL = EXPF_ULPS * 2.0 * U
TINY = 2.0 ** -126                   # results below this may be flushed or lose bits: an ABSOLUTE error of at most this much each


def held(got, want, bound):
    """-> (every element within its bound, worst err / bound).  The non-finite pattern of `got` must EQUAL that of `want` (NaN where NaN, the
    same infinity where infinite: asserted); the finite elements are compared, an element whose bound is 0 must be exact."""
    got, want, bound = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(bound, dtype=F64)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs from the float64 reference's"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "infinities differ from the float64 reference's"
    err, b = np.abs(got[fin] - want[fin]), bound[fin]
    assert np.isfinite(b).all(), "a finite reference element without a finite bound"
    ratio = np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))
    return bool((err <= b).all()), float(ratio.max()) if ratio.size else 0.0


# ============================================================================================================================== SpMM
def spmm_rows_f64(S, rowptr, colidx, vals, bias, relu):
    """out[f, v, :] = act(sum_e vals[e] S[f, colidx[e], :] + bias) over the CSR entries e of row v, in float64 from the fp32 inputs.
    S (F, vg, c) -> (h (F, vg, c) float64, bound (F, vg, c) float64).

    spmm_rows_kernel (and the aggregation of gcn_fused_tile, the same arithmetic) forms acc = fmaf(w_e, x_e, acc) over the row's entries in
    CSR order, starting from 0, then y = acc + bias (one addition; + 0.f without a bias: exact), then fmaxf(y, 0) (exact).  A row of n
    entries is n fused steps and one addition: the first term passes n + 1 roundings, every other term and the bias fewer, so
        |h^ - h| <= gamma(n + 1) (sum_e |w_e x_e| + |b|).
    ReLU is 1-Lipschitz: the bound passes through it unchanged.  Non-finite inputs give non-finite h and bound in the rows that reference
    them, and only there.  The project's ReLU is fmaxf(y, 0), which maps NaN to 0 as it maps -inf (csrc/Makefile on -fno-honor-nans: "ReLU
    already maps NaN to 0 in these kernels"): np.fmax here, and where a non-finite pre-activation became 0 the bound is 0 -- exactly 0 is
    required."""
    S = np.asarray(S)
    assert S.dtype == F32 and np.asarray(vals).dtype == F32
    F_, vg, c = S.shape
    S64 = S.astype(F64)
    h = np.zeros((F_, vg, c), F64)
    mag = np.zeros((F_, vg, c), F64)
    lens = np.diff(rowptr).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(vg):
            b, e = int(rowptr[r]), int(rowptr[r + 1])
            if e > b:
                terms = S64[:, colidx[b:e], :] * vals[b:e].astype(F64)[None, :, None]
                h[:, r] = terms.sum(1)
                mag[:, r] = np.abs(terms).sum(1)
        if bias is not None:
            h = h + bias.astype(F64)
            mag = mag + np.abs(bias.astype(F64))
        bound = gamma(lens + 1.0)[None, :, None] * mag
        if relu:
            h = np.fmax(h, 0.0)
            bound = np.where(np.isfinite(h) & ~np.isfinite(bound), 0.0, bound)
    return h, bound


def agg_linear_f64(S, rowptr, colidx, vals, bias, relu, W):
    """g4d_gcn_agg_linear_f32 in float64: h = spmm_rows_f64(...), out = h W with W (128, cout) the next layer's weight.
    -> (h64, out64, bound_h, bound_out).

    The kernel contracts its fp32 h^ = h + dh, |dh| <= bound_h, through 32 chained v_mfma_f32_16x16x4_f32 per output (4 slices of 32 channels x
    2 halves x 4 instructions, 4 products each).  With the count of N_MFMA above (every product and every addition rounds: the deepest term
    passes 1 + 4 * 32 = 129 roundings)
        |out^ - out| <= |W|^T bound_h + gamma(129) (|h| + bound_h) . |W|.
    (The project's bf16-exact suite shows that nothing is lost where all sums are representable; that is a floor, this is the ceiling.)"""
    h, bound_h = spmm_rows_f64(S, rowptr, colidx, vals, bias, relu)
    W64 = np.asarray(W).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = h @ W64
        bound_out = bound_h @ np.abs(W64) + gamma(N_MFMA) * ((np.abs(h) + bound_h) @ np.abs(W64))
    return h, out, bound_h, bound_out


def tile_plan(rowptr, colidx, vg, tile):
    """The per-workgroup rule of gcn_fused_kernel (and of gcn_meta_kernel, which must restate it): per tile of `tile` consecutive rows
    -> (lo, hi, ell, fast): the window [lo, hi) over the column indices of the tile's rows ([0x7fffffff, 0) without entries), its longest
    row, and whether it takes the LDS path: ell <= 8, hi - lo <= kWin, hi > lo."""
    kwin = K_WIN[tile]
    plan = []
    for r0 in range(0, vg, tile):
        nrows = min(tile, vg - r0)
        e0, e1 = int(rowptr[r0]), int(rowptr[r0 + nrows])
        cols = np.asarray(colidx[e0:e1])
        lo = int(cols.min()) if cols.size else EMPTY_LO
        hi = int(cols.max()) + 1 if cols.size else 0
        ell = int(np.diff(rowptr[r0:r0 + nrows + 1]).max())
        plan.append((lo, hi, ell, int(ell <= K_ELL and hi - lo <= kwin and hi > lo)))
    return plan


def meta_ints(tile):
    """ints per tile of the metadata g4d_gcn_tile_meta_build writes: 4 header ints + tile * 8 (offset, weight bits) pairs."""
    return 4 + tile * K_ELL * 2


# ========================================================================================================================= attention
K_STEPS = 32                         # 16-wide k-steps per wave (kAttKsteps)
MAX_T = 32


def attention_layout(Vg, C):
    """-> (ksteps, slices, workgroups) of att_scores_partial_kernel: D = Vg C is cut into 16-wide k-steps, 32 of them per wave (slice),
    4 waves per workgroup; one partial tile per workgroup reaches the softmax kernel.  g4d_temporal_attention_scratch_floats is
    nclips * slices * 1024."""
    ksteps = Vg * C // 16
    slices = (ksteps + K_STEPS - 1) // K_STEPS
    return ksteps, slices, (slices + 3) // 4


def score_roundings(Vg, C):
    """Roundings the deepest product of one score passes (see attention_f64)."""
    ksteps, _, wgs = attention_layout(Vg, C)
    return 1 + 16 * min(K_STEPS, ksteps) + 3 + (wgs // 4 + wgs % 4) + 2 + 2


def attention_f64(qkv, nclips, T, Vg, C):
    """modules/mesh_encoder.py:467-476 in float64 from the fp32 qkv (nclips * T, Vg, 3 C): per clip att = softmax(q k^T / sqrt(T)) over
    D = Vg C, out = att v.  -> (att64 (nclips, T, T), out64 (nclips * T, Vg, C), bound_att, bound_out).

    Scores.  A wave adds up to 32 k-steps x 16 products through chained MFMAs (counted as N_MFMA is: each product and each addition
    rounds: 1 + 16 * min(32, ksteps)), the 4 waves of a workgroup meet as ((w0 + w1) + w2) + w3 (3), att_scores_softmax_kernel adds
    the workgroups' partials in four chains, chain 0 also taking the remainder (W // 4 + W % 4 additions at most), then (s0 + s1) + (s2 + s3)
    (2), then one division by (float)sqrt((double)T) -- the divisor is itself rounded once (2).  All terms of a score are products
    q k, so with n = score_roundings(Vg, C)
        |s^ - s| <= ds = gamma(n) sum_d |q_d| |k_d| / sqrt(T).
    Softmax.  The kernel takes m^ = max_j s^_j (exact), d_j = fl(s^_j - m^) (one rounding of a difference no larger than the row's score
    range R plus 2 ds), E_j = expf(d_j) (1 + eps_j) with |eps_j| <= e = EXPF_REL, Z^ = the sum of the T values E_j >= 0 in order
    (gamma(T)), att^ = fl(E_u / Z^) (u).  Softmax does not depend on the constant subtracted, so against the exact value
        att^_u / att_u = exp(eta_u) (1 + eps_u) (1 + delta) / (a weighted mean of exp(eta_j) (1 + eps_j) (1 + theta_j)),
        |eta_j| <= a = max_j ds_j + u (R + 2 max_j ds_j),
    which lies within  rel = exp(2 a) (1 + e) (1 + u) / ((1 - e) (1 - gamma(T))) - 1  of 1 on either side: not a first-order statement, the
    remainder is inside the closed form.  A value E_j or att^ below 2^-126 may lose bits or be flushed: TINY absolute each, (T + 2) TINY on
    att^ (Z^ >= 1 - e).
        bound_att = rel att + (T + 2) TINY.
    Mix.  out_t = sum_u att^_tu v_u as T fused steps: |out^ - out| <= sum_u bound_att_tu |v_u| + gamma(T) sum_u (att + bound_att)_tu |v_u|."""
    qkv = np.asarray(qkv)
    assert qkv.dtype == F32 and qkv.shape == (nclips * T, Vg, 3 * C)
    x = qkv.astype(F64).reshape(nclips, T, Vg, 3, C)
    q, k, v = (x[:, :, :, i, :].reshape(nclips, T, Vg * C) for i in range(3))
    rt = math.sqrt(T)
    s = q @ k.transpose(0, 2, 1) / rt
    ds = gamma(score_roundings(Vg, C)) * (np.abs(q) @ np.abs(k).transpose(0, 2, 1)) / rt
    m = s.max(-1, keepdims=True)
    E = np.exp(s - m)
    att = E / E.sum(-1, keepdims=True)
    dsm = ds.max(-1, keepdims=True)
    a = dsm + U * ((m - s.min(-1, keepdims=True)) + 2.0 * dsm)
    rel = np.exp(2.0 * a) * (1.0 + EXPF_REL) * (1.0 + U) / ((1.0 - EXPF_REL) * (1.0 - gamma(T))) - 1.0
    bound_att = rel * att + (T + 2) * TINY
    out = att @ v
    bound_out = bound_att @ np.abs(v) + gamma(T) * ((att + bound_att) @ np.abs(v))
    shape = (nclips * T, Vg, C)
    return att, out.reshape(shape), bound_att, bound_out.reshape(shape)


def row_sum_tolerance(T):
    """|sum_u att^_tu - 1|, the sum taken exactly: the E_u of the numerators are the terms of Z^, so the exact sum of E_u / Z^ is 1 / (1 + theta),
    |theta| <= gamma(T), and each division rounds once; gamma(T + 2) with the expf term on top (both evaluations of expf(d_u) agree, so the
    term is slack, kept as the issue states it)."""
    return gamma(T + 2) + EXPF_REL


# ====================================================================================================================== GCN case builders
def _csr(rows, rng):
    """rows: one list of column indices per row (any order, repeats allowed) -> (rowptr, colidx, vals) with weights of both signs, |w| up to
    ~4 (a GENERAL sparse matrix, not a normalised adjacency)."""
    rowptr = np.zeros(len(rows) + 1, np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.array([c for r in rows for c in r], np.int32)
    assert colidx.size > 0
    vals = (rng.standard_normal(colidx.size) * 1.5).astype(F32)
    vals[vals == 0] = F32(0.5)
    return rowptr, colidx, vals


def _band(vg, rng, lo=1, hi=7, reach=12):
    """Rows of lo..hi entries each, columns drawn (unsorted, with repeats) from [r - reach, r + reach]: every tile's window stays far
    below kWin."""
    return [list(rng.integers(max(0, r - reach), min(vg, r + reach + 1), int(rng.integers(lo, hi + 1)))) for r in range(vg)]


def _near(r, vg, n, rng, reach=12):
    return list(rng.integers(max(0, r - reach), min(vg, r + reach + 1), n))


def _gcn(name, tile, rows, frames, rng, cout=128, bias=True, relu=1, tap=True, expect=None, **extra):
    vg = len(rows)
    rowptr, colidx, vals = _csr(rows, rng)
    c = dict(name=name, tile=tile, vg=vg, frames=frames, rowptr=rowptr, colidx=colidx, vals=vals,
             S=rng.standard_normal((frames, vg, KC)).astype(F32), bias=rng.standard_normal(KC).astype(F32) if bias else None,
             relu=int(relu), tap=bool(tap), cout=cout, W=(rng.standard_normal((KC, cout)) * 0.1).astype(F32), expect=expect or {})
    c.update(extra)
    return c


TILES_TOTAL = {1: (1, 1), 7: (7, 1), 8: (4, 2), 9: (3, 3), 17: (17, 1)}      # frames x tiles per frame
COUTS = (128, 16, 3, 1)


def gcn_case_names(tile):
    names = [f"vg_{n}" for n in (1, tile - 1, tile, tile + 1, 2 * tile + 1)]
    names += [f"tiles_{k}" for k in TILES_TOTAL]
    names += ["ell8", "ell9", "win_at", "win_over", "empty_tiles_bias", "empty_tiles_nobias", "empty_rows"]
    names += [f"cout_{c}" for c in COUTS]
    names += [f"epi_b{b}r{r}t{t}" for b in (0, 1) for r in (0, 1) for t in (0, 1)]
    names += ["nonfinite_relu0", "nonfinite_relu1"]
    return names


def _mixed_mesh(tile, rng):
    """tile + 30 rows: tile 0 fast, tile 1 (30 rows) slow through one row of 9 entries."""
    rows = _band(tile + 30, rng)
    rows[tile + 7] = _near(tile + 7, tile + 30, 9, rng)
    return rows, {0: "fast", 1: "slow"}


@functools.lru_cache(maxsize=None)
def gcn_case(name, tile=128):
    """-> dict(name, tile, vg, frames, rowptr, colidx, vals, S (frames, vg, 128), bias | None, relu, tap, cout, W (128, cout), expect).
    expect = {tile index: "fast" | "slow"} (tiles not named: fast), plus "ell" / "win" = {tile index: longest row / window rows} and "total"
    = frames x tiles where the case is about that number; tests/test_refine_forward_cpu.py asserts all of it with tile_plan.  T = tile, K = kWin:
      vg_<n>            banded rows, 2 frames: n in {1, T - 1, T, T + 1, 2 T + 1} -- the ragged last tile
      tiles_<k>         frames x tiles = k in {1, 7, 8, 9, 17}, last tile ragged: the XCD remap (grid = 8 ceil(k / 8)) and both early returns
                        (17 is prime: 17 frames of a 37-vertex mesh, the one case above 9 frames)
      ell8 / ell9       three tiles; the middle one has a row of exactly 8 entries (fast at the kEll limit) / also one of 9 and rows of every
                        length 1..9 (slow, `j < len[p]` select; neighbours stay fast)
      win_at / _over    the middle tile's window is exactly K / K + 1 rows (fast at the kWin limit / slow just beyond)
      empty_tiles_*     tile 1 and the (ragged) last tile have no entry at all: slow with a zero trip count, act(bias) (bias, relu) or 0 (neither)
      empty_rows        empty rows inside a fast tile (the zero-row pair), inside a slow one (the e0 fallback; the tile's first row and one whole
                        8-row group of a wave among them) and as the very last row
      cout_<c>          c in {128, 16, 3, 1} on a fast + slow mesh: both channel mappings and the ch < cout store guard
      epi_b?r?t?        bias x relu x tap on the same mesh
      nonfinite_relu?   frame 0: one row of S holds +inf in every third channel, another NaN in channels 5..40, inside a fast tile's window and
                        again inside a slow tile; most rows of either tile reference neither.  Frame 1 is finite."""
    T_, K = tile, K_WIN[tile]
    rng = np.random.default_rng(1000 * tile + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    kind, _, arg = name.partition("_")
    if kind == "vg":
        return _gcn(name, tile, _band(int(arg), rng), 2, rng)
    if kind == "tiles":
        frames, tpf = TILES_TOTAL[int(arg)]
        return _gcn(name, tile, _band((tpf - 1) * T_ + 37, rng), frames, rng, expect={"total": int(arg)})
    if name in ("ell8", "ell9"):
        vg = 3 * T_
        rows = _band(vg, rng)
        rows[T_ + 5] = _near(T_ + 5, vg, 8, rng)
        expect = {"ell": {1: 8}}
        if name == "ell9":
            for i in range(9):                                       # rows of ar 10..18: the second and third wave of the workgroup
                rows[T_ + 10 + i] = _near(T_ + 10 + i, vg, i + 1, rng)
            expect = {0: "fast", 1: "slow", 2: "fast", "ell": {1: 9}}
        return _gcn(name, tile, rows, 2, rng, expect=expect)
    if name in ("win_at", "win_over"):
        lo = 20
        width = K + (name == "win_over")
        vg = max(3 * T_ + 20, lo + width + 12)
        rows = _band(vg, rng)
        for r in range(T_, 2 * T_):
            rows[r] = list(rng.integers(lo, lo + width, int(rng.integers(1, 8))))
        rows[T_ + 3][0] = lo
        rows[T_ + 77 % T_][-1] = lo + width - 1
        return _gcn(name, tile, rows, 2, rng, expect={1: "fast" if name == "win_at" else "slow", "win": {1: width}})
    if kind == "empty" and arg.startswith("tiles"):
        vg = 3 * T_ + 17
        rows = _band(vg, rng)
        for r in list(range(T_, 2 * T_)) + list(range(3 * T_, vg)):
            rows[r] = []
        with_bias = name.endswith("_bias")
        return _gcn(name, tile, rows, 2, rng, bias=with_bias, relu=with_bias, expect={1: "slow", 3: "slow", "ell": {1: 0, 3: 0}})
    if name == "empty_rows":
        vg = 2 * T_ + 9
        rows = _band(vg, rng)
        rows[T_ + 50] = _near(T_ + 50, vg, 9, rng)
        empty = [0, 5, 6, 31, T_ - 1, T_, T_ + 1, T_ + 33, vg - 1] + list(range(T_ + 8, T_ + 16))
        for r in empty:
            rows[r] = []
        return _gcn(name, tile, rows, 2, rng, expect={1: "slow"}, empty=tuple(empty))
    if kind == "cout":
        rows, expect = _mixed_mesh(tile, rng)
        return _gcn(name, tile, rows, 2, rng, cout=int(arg), expect=expect)
    if kind == "epi":
        rows, expect = _mixed_mesh(tile, rng)
        return _gcn(name, tile, rows, 2, rng, bias=arg[1] == "1", relu=arg[3] == "1", tap=arg[5] == "1", expect=expect)
    if kind == "nonfinite":
        vg = 2 * T_ + 10
        rows = _band(vg, rng)
        rows[T_ + 40] = _near(T_ + 40, vg, 9, rng)
        # the fast tile's +inf row is row 0 of its WINDOW (a padded pair pointed at window row 0 instead of the zero row would read it), and the
        # window's last row holds NaN as well
        bad = {"inf": (0, T_ + 10), "nan": (20, T_ + 20)}
        rows[1] = [0, 2]
        for b, (ri, rn) in zip((0, T_), zip(bad["inf"], bad["nan"])):  # + 2 inf -> +inf;  - 2 inf -> -inf (0 behind the ReLU);  inf and NaN -> NaN (0)
            rows[b + 30], rows[b + 32], rows[b + 34] = [ri, b + 31], [ri], [rn, ri]
        c = _gcn(name, tile, rows, 2, rng, relu=arg == "relu1", expect={0: "fast", 1: "slow"}, bad=bad)
        for b in (0, T_):
            c["vals"][c["rowptr"][b + 30]], c["vals"][c["rowptr"][b + 32]] = F32(2.0), F32(-2.0)
        for r in bad["inf"]:
            c["S"][0, r, ::3] = np.inf
        c["window_end"] = tile_plan(c["rowptr"], c["colidx"], vg, tile)[0][1] - 1
        for r in bad["nan"] + (c["window_end"],):
            c["S"][0, r, 5:41] = np.nan
        return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def gcn_reference(name, tile=128):
    """agg_linear_f64 of gcn_case(name, tile), computed once: (h64, out64, bound_h, bound_out)."""
    c = gcn_case(name, tile)
    return agg_linear_f64(c["S"], c["rowptr"], c["colidx"], c["vals"], c["bias"], c["relu"], c["W"])


SPMM_C = (1, 3, 4, 5, 128, 130)


@functools.lru_cache(maxsize=None)
def spmm_case(c, vg=41):
    """g4d_spmm_rows_f32 at width c: 3 frames of vg rows with lengths 0 (rows 2, 7, vg - 1), 1 (row 0) and 40 (row 4) among banded ones."""
    rng = np.random.default_rng(77 + 13 * c + vg)
    rows = _band(vg, rng)
    if vg > 1:
        rows[0] = [vg - 1]
        rows[4] = list(rng.integers(0, vg, 40))
        for r in (2, 7, vg - 1):
            rows[r] = []
    rowptr, colidx, vals = _csr(rows, rng)
    return dict(vg=vg, c=c, frames=3, rowptr=rowptr, colidx=colidx, vals=vals, S=rng.standard_normal((3, vg, c)).astype(F32),
                bias=rng.standard_normal(c).astype(F32))


# ================================================================================================================ attention case builders
def _att(name, nclips, T, Vg, C, rng, col0=0, pad=0, expect=None, kind="random"):
    """random: q, k ~ N(0, s^2) with s^2 sqrt(D / T) = 2 -- scores of a few units (a softmax far from uniform) while ds stays ~1e-2; v ~ N(0, 1)."""
    D = Vg * C
    x = rng.standard_normal((nclips * T, Vg, 3, C))
    if kind == "random":
        x[:, :, :2] *= math.sqrt(2.0 / math.sqrt(D / T))
    elif kind == "peaked":                                           # k = q per frame, |q_t|^2 / sqrt(T) = 30 .. 80 down the frames
        g = x[:, :, 0].reshape(nclips, T, D)
        g /= np.linalg.norm(g, axis=-1, keepdims=True)
        g *= np.sqrt(np.linspace(30.0, 80.0, T) * math.sqrt(T))[None, :, None]
        x[:, :, 0] = g.reshape(nclips * T, Vg, C)
        x[:, :, 1] = x[:, :, 0]
    elif kind == "uniform":
        x[:, :, 0] = 0.0
    qkv = np.ascontiguousarray(x.reshape(nclips * T, Vg, 3 * C).astype(F32))
    qkv.setflags(write=False)
    return dict(name=name, nclips=nclips, T=T, Vg=Vg, C=C, qkv=qkv, col0=col0, ldo=col0 + C + pad, expect=expect or {}, kind=kind)


ATT_T = (1, 2, 15, 16, 17, 31, 32)
ATT_KSTEPS = (1, 15, 32, 33)
ATT_WGS = (1, 2, 3, 4, 5, 7, 8)
ATT_C = (16, 48, 128, 256)
ATT_COLS = [(c0, pad) for c0 in (0, 3, 4) for pad in (0, 5)]


def attention_case_names():
    names = [f"T_{t}" for t in ATT_T] + [f"ksteps_{k}" for k in ATT_KSTEPS] + ["slices_4", "slices_5"] + [f"wgs_{w}" for w in ATT_WGS]
    names += [f"C_{c}" for c in ATT_C] + [f"col_{c0}_{pad}" for c0, pad in ATT_COLS]
    return names + ["clips", "peaked_8", "peaked_17", "uniform_9", "uniform_32"]


@functools.lru_cache(maxsize=None)
def attention_case(name):
    """-> dict(name, nclips, T, Vg, C, qkv (nclips * T, Vg, 3 C) read-only, col0, ldo, expect, kind); expect holds what the name promises of
    attention_layout (ksteps / slices / wgs).
      T_<t>          one clip at Vg = 37, C = 48: T on either side of the 16-row MFMA tile and at both ends
      ksteps_<k>     C = 16, Vg = k: a partial slice, an exact one, a one-k-step tail slice
      slices_4 / 5   a full workgroup / one more with three inactive waves
      wgs_<w>        w partial tiles: the four-chain loop with and without a remainder
      C_<c>          the d / C, d % C addressing
      col_<c0>_<pad> column offset and row stride of the destination
      clips          3 clips of different data
      peaked_<T>     k = q, diagonal scores 30..80: the max subtraction (sum |q| |k| equals the score on the diagonal)
      uniform_<T>    q = 0: every score 0, att = 1 / T"""
    rng = np.random.default_rng(sum(ord(ch) * (i + 3) for i, ch in enumerate(name)))
    kind, _, arg = name.partition("_")
    if kind == "T":
        return _att(name, 1, int(arg), 37, 48, rng, expect={"wgs": 1})
    if kind == "ksteps":
        return _att(name, 1, 5, int(arg), 16, rng, expect={"ksteps": int(arg)})
    if kind == "slices":
        return _att(name, 1, 6, {"4": 128, "5": 129}[arg], 16, rng, expect={"slices": int(arg)})
    if kind == "wgs":
        return _att(name, 1, 7, 128 * int(arg) - 5, 16, rng, expect={"wgs": int(arg)})
    if kind == "C":
        return _att(name, 1, 6, 19, int(arg), rng)
    if kind == "col":
        c0, pad = arg.split("_")
        return _att(name, 2, 4, 21, 32, rng, col0=int(c0), pad=int(pad))
    if name == "clips":
        return _att(name, 3, 5, 23, 32, rng)
    if kind == "peaked":
        return _att(name, 2, int(arg), 40, 32, rng, kind="peaked")
    if kind == "uniform":
        return _att(name, 1, int(arg), 11, 16, rng, kind="uniform")
    raise KeyError(name)

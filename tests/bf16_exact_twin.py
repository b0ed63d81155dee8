"""Float64 twin of the shared-MLP kernels on inputs where their arithmetic is EXACT (tests/test_bf16_exact_{cpu,gpu}.py).

Inputs, weights, scales and shifts sit on a dyadic lattice chosen so that every product and every partial sum of every layer is exactly
representable in fp32 whatever the summation order.  The only roundings left in a bf16-operand kernel are then the conversions of the operands
to bf16, whose inputs are exact and whose results round-to-nearest-even fully determines; a float64 evaluation that rounds at the same points
gives the kernel's output EXACTLY, and the GPU tests compare with torch.equal.  In "fp32" and "bf16x3" nothing rounds at all.

    make_stack(widths, seed)          per-layer (W, scale, shift, relu), float64
    make_inputs(kind, ...)            layer-0 operands for the three loaders: "direct", "group", "interp"
    expected(inp, stack, precision)   (output, tapped hidden layer | None), float64; `mut=` applies one deliberate fault (the CPU tests prove
                                      that each of them changes the expected output of every case, so a kernel with that fault cannot pass)
    check_conditions(...)             asserts that the case is inside the exact regime and exercises the roundings (see its docstring)

The span condition (a) of check_conditions is 2^SPAN_BITS = 2^22 lattice units per accumulated sum: two bits inside fp32's 24, for a matrix
core whose internal alignment might be narrower than fp32.  Measured on MI355X (gfx950): v_mfma_f32_16x16x32_bf16 and v_mfma_f32_16x16x4_f32
reproduce the twin bit for bit on every case of tests/test_bf16_exact_gpu.py (sums of up to 2^21.7 units), so the limit was not lowered; see
DESIGN.md, parity section.
"""
import torch

SPAN_BITS = 22
_FIX = 40           # lattice arithmetic below is done on integers x * 2^_FIX (every value here is a multiple of 2^-30 and below 2^22)

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------- bf16 roundings
def _bits(x):
    f = x.to(torch.float32)
    assert torch.equal(f.to(F64), x), "value not exactly representable in fp32: outside the exact regime"
    return f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(b):
    b = b & 0xFFFFFFFF
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32)
    return b.view(torch.float32).to(F64)


def round_bf16(x, rule="rne"):
    """fp32 -> bf16 -> float64 under `rule`: "rne" (what the kernels do), "trunc", "away" (ties away from zero; differs from rne on ties only)."""
    b = _bits(x)
    if rule == "rne":
        r = b + 0x7FFF + ((b >> 16) & 1)
    elif rule == "away":
        r = b + 0x8000
    else:
        assert rule == "trunc"
        r = b
    out = _from_bits(r & 0xFFFF0000)
    if rule == "rne":
        assert torch.equal(out, x.to(torch.float32).to(torch.bfloat16).to(F64))
    return out


def not_bf16(x):
    return (_bits(x) & 0xFFFF) != 0


def is_tie(x):
    return (_bits(x) & 0xFFFF) == 0x8000


def lowest_bit(*tensors):
    """u = the lowest set bit over all non-zero entries (a power of two)."""
    u = None
    for t in tensors:
        v = (t.to(F64) * 2.0 ** _FIX)
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 2.0 ** 62
        v = v.to(torch.int64)
        v = v[v != 0]
        if v.numel():
            m = int((v & -v).min())
            u = m if u is None else min(u, m)
    return (u if u is not None else 2 ** _FIX) / 2.0 ** _FIX


def _fp32_exact(x, what):
    assert torch.equal(x.to(torch.float32).to(F64), x), f"{what}: not exactly representable in fp32"


# ---------------------------------------------------------------------------------------------------------------- generators
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def lattice_values(shape, g, ties=0.08, frac=8):
    """Multiples of 2^-8 in [-8, 8) (about 70% not bf16-representable); a fraction `ties` replaced by exact bf16 ties: nine significant bits,
    the ninth set -- half of them with an even and half with an odd eighth bit, so that ties-to-even rounds down as often as up.
    frac < 8: multiples of 2^-frac, no ties (a coarser lattice for deep stacks whose operands are not rounded)."""
    if frac < 8:
        return torch.randint(-8 * 2 ** frac, 8 * 2 ** frac, shape, generator=g).to(F64) / 2.0 ** frac
    x = torch.randint(-2048, 2048, shape, generator=g).to(F64) / 256.0
    t = (2 * torch.randint(128, 256, shape, generator=g) + 1).to(F64) / 256.0 * (2.0 ** torch.randint(-2, 3, shape, generator=g).to(F64))
    t = t * (2 * torch.randint(0, 2, shape, generator=g) - 1).to(F64)
    return torch.where(torch.rand(shape, generator=g) < ties, t, x)


def make_stack(widths, seed, nnz=10, relu_last=False, unit_scale=False, probe=None):
    """[(W (Cout, K), scale (Cout), shift (Cout), relu)] for widths = (K0, C1, ..., Cn).  Every weight row has up to `nnz` non-zeros in +-{1, 2};
    every input column is used by at least one output channel (a dropped or permuted column must show): rows get ceil(K / Cout) columns of a
    random cover first, random columns after that; with `probe` (rows of layer-0 inputs) a channel that ReLU would leave zero in more than 90% of those rows gets |w| and |shift| instead.  scale in {1, 0.5} (1 with unit_scale: a conv bias without BatchNorm), shift a multiple of
    0.25 in [-2, 2], ReLU on the hidden layers (and on the last with relu_last)."""
    g = _gen(seed)
    out = []
    for l, (K, C) in enumerate(zip(widths[:-1], widths[1:])):
        W = torch.zeros(C, K, dtype=F64)
        val = lambda n: (torch.randint(1, 3, (n,), generator=g) * (2 * torch.randint(0, 2, (n,), generator=g) - 1)).to(F64)
        cols = torch.randperm(K, generator=g)
        rows = torch.randperm(C, generator=g)
        W[rows[torch.arange(K) % C], cols] = val(K)                     # the cover
        for c in range(C):
            extra = max(0, min(nnz[l] if isinstance(nnz, (tuple, list)) else nnz, K) - int((W[c] != 0).sum()))
            if extra:
                free = torch.nonzero(W[c] == 0).flatten()
                pick = free[torch.randperm(free.numel(), generator=g)[:extra]]
                W[c, pick] = val(extra)
        scale = torch.ones(C, dtype=F64) if unit_scale else 2.0 ** -torch.randint(0, 2, (C,), generator=g).to(F64)
        shift = torch.randint(-8, 9, (C,), generator=g).to(F64) / 4.0
        relu = bool(l < len(widths) - 2 or relu_last)
        if probe is not None:                            # (rows, K) inputs of this layer: a channel ReLU leaves (almost) always zero gets |w| and |shift|
            h = (probe @ W.T) * scale + shift
            if relu:
                dead = (h > 0).double().mean(0) < 0.10
                W[dead], shift[dead] = W[dead].abs(), shift[dead].abs()
                h = ((probe @ W.T) * scale + shift).clamp_min(0.0)
            probe = h
        out.append((W, scale, shift, relu))
    return out


def make_inputs(kind, seed, rows=None, K0=None, B=None, N=None, P=None, S=None, C=None, n=None, m=None, C2=None, C1=0, idx=None, frac=8):
    """Layer-0 operands on the lattice.
    "direct": X (rows, K0).
    "group":  xyz (B, N, 3), new_xyz (B, P, 3) multiples of 2^-8 in [-4, 4) (their fp32 difference is exact, in [-8, 8)), feats (B, N, C) | None,
              idx (B, P, S) int32 (random unless given); K0 = 3 + C.
    "interp": known (B, m, C2), skip (B, n, C1) | None, nn_idx (B, n, 3) int32, dist2 (B, n, 3): one entry 1.0 and two 4.0 per row, so that the
              inverse-distance weights 1 / (sqrt(d) + 1e-8) are exactly 1 and 0.5 (1e-8 is below half an ulp of either) and normalise to
              (0.5, 0.25, 0.25) in some order."""
    g = _gen(seed)
    if kind == "direct":
        return dict(kind=kind, X=lattice_values((rows, K0), g, frac=frac), rows=rows, K0=K0)
    if kind == "group":
        xyz = torch.randint(-1024, 1024, (B, N, 3), generator=g).to(F64) / 256.0
        new_xyz = torch.randint(-1024, 1024, (B, P, 3), generator=g).to(F64) / 256.0
        feats = lattice_values((B, N, C), g, frac=frac) if C else None
        if idx is None:
            idx = torch.randint(0, N, (B, P, S), generator=g, dtype=torch.int32)
        assert tuple(idx.shape) == (B, P, S)
        return dict(kind=kind, xyz=xyz, new_xyz=new_xyz, feats=feats, idx=idx, B=B, N=N, P=P, S=S, C=C, rows=B * P * S, K0=3 + C)
    assert kind == "interp"
    known = lattice_values((B, m, C2), g, frac=frac)
    skip = lattice_values((B, n, C1), g, frac=frac) if C1 else None
    nn_idx = torch.randint(0, m, (B, n, 3), generator=g, dtype=torch.int32)
    near = torch.randint(0, 3, (B, n), generator=g)
    dist2 = torch.full((B, n, 3), 4.0, dtype=F64)
    dist2.scatter_(2, near[..., None], 1.0)
    assert bool(((dist2 == 1.0).sum(2) == 1).all()) and bool(((dist2 == 4.0).sum(2) == 2).all())
    return dict(kind=kind, known=known, skip=skip, nn_idx=nn_idx, dist2=dist2, B=B, n=n, m=m, C2=C2, C1=C1, rows=B * n, K0=C2 + C1)


def layer0_rows(inp):
    """(rows, K0) float64: what the loader hands to the first layer, before any rounding."""
    if inp["kind"] == "direct":
        return inp["X"]
    if inp["kind"] == "group":
        B, P, S = inp["B"], inp["P"], inp["S"]
        j = inp["idx"].long()
        b = torch.arange(B)[:, None, None].expand(B, P, S)
        d = inp["xyz"][b, j] - inp["new_xyz"][:, :, None, :]
        _fp32_exact(d, "grouped coordinate difference")
        x = d if inp["feats"] is None else torch.cat([d, inp["feats"][b, j]], -1)
        return x.reshape(B * P * S, -1)
    B, n = inp["B"], inp["n"]
    r = 1.0 / inp["dist2"].sqrt()                     # exactly 1 or 0.5: what fp32 gives for 1 / (sqrt(d) + 1e-8)
    w = r / r.sum(2, keepdim=True)                    # norm = 2: exactly (0.5, 0.25, 0.25) in some order
    assert bool(((w == 0.5).sum(2) == 1).all()) and bool(((w == 0.25).sum(2) == 2).all())
    b = torch.arange(B)[:, None].expand(B, n)
    k = inp["nn_idx"].long()
    f = sum(w[..., i, None] * inp["known"][b, k[..., i]] for i in range(3))
    _fp32_exact(f, "interpolated features")
    x = f if inp["skip"] is None else torch.cat([f, inp["skip"]], -1)
    return x.reshape(B * n, -1)


# ---------------------------------------------------------------------------------------------------------------- the twin
MUTATIONS = ("trunc", "away", "drop_last_col", "swap_cols", "pool_shift")


def expected(inp, stack, precision, pool=0, S=1, tap=None, mut=None, mut_layer=0, stats=None):
    """(out, tap_out): the stack over layer0_rows(inp) in float64.  "bf16": the operands (activations and weights) of every layer rounded to
    bf16 (RNE); accumulation, affine, ReLU, pooling and the tap stay exact (fp32 in the kernels).  "fp32" / "bf16x3": no rounding.
    pool = 1 max / 2 avg over windows of S consecutive rows; tap = index of a hidden layer whose activation is returned as well.
    mut (one of MUTATIONS) applies a deliberate fault at layer `mut_layer` (the roundings: at every layer); stats, a list, receives one dict
    per layer for check_conditions."""
    assert precision in ("fp32", "bf16", "bf16x3") and mut in (None,) + MUTATIONS
    rule = {"trunc": "trunc", "away": "away"}.get(mut, "rne")
    h = layer0_rows(inp)
    tap_out = None
    for l, (W, scale, shift, relu) in enumerate(stack):
        K = W.shape[1]
        assert h.shape[1] == K
        if mut == "drop_last_col" and l == mut_layer:
            h = h.clone()
            h[:, K - 1] = 0.0
        if mut == "swap_cols" and l == mut_layer:     # two columns of one 32-wide k-step change places (the last step when it holds two)
            c1 = K - 1
            c0 = c1 - 1 if c1 % 32 else c1 - 31
            h = h.clone()
            h[:, [c0, c1]] = h[:, [c1, c0]]
        _fp32_exact(h, f"layer {l} input")
        if precision == "bf16":
            hr, Wr = round_bf16(h, rule), round_bf16(W, rule)
        else:
            hr, Wr = h, W
        acc = hr @ Wr.T
        if stats is not None:
            stats.append(dict(layer=l, span=float((hr.abs() @ Wr.abs().T).max()), u=lowest_bit(hr, Wr), cover=bool(((Wr != 0).sum(0) > 0).all()),
                              live=float((hr != 0).double().mean(0).min()),
                              rounded=precision == "bf16", inexact=float(not_bf16(h).double().mean()), ties=float(is_tie(h).double().mean())))
        _fp32_exact(acc, f"layer {l} accumulator")
        h = acc * scale + shift
        _fp32_exact(h, f"layer {l} output")
        if relu:
            h = h.clamp_min(0.0)
        if tap is not None and l == tap:
            assert l < len(stack) - 1
            tap_out = h
    if pool:
        if mut == "pool_shift":
            h = torch.roll(h, -1, 0)
        h = h.view(-1, S, h.shape[1])
        if pool == 1:
            h = h.max(1).values
        else:
            if stats is not None:
                stats.append(dict(layer="avg", span=float(h.abs().sum(1).max()), u=lowest_bit(h), S=S))
            h = h.sum(1)
            _fp32_exact(h, "average-pool sum")
            h = h / S
            _fp32_exact(h, "average-pool output")
    return h, tap_out


def check_conditions(inp, stack, precision, pool=0, S=1):
    """Asserts, on the reference alone, that the case is inside the exact regime and exercises what it is meant to:
    (a) at every layer  max_row sum_k |h_k| |w_k| < 2^SPAN_BITS u,  u = the lowest set bit over the layer's non-zero operands (so every partial
        sum, in any order, is a multiple of u below 2^22 u: exact in fp32 with two bits to spare); the same for the average pool's sum over S rows;
    (b) every input column of every layer carries a non-zero weight in at least one output channel;
    (c) in every rounded layer at least 10% of the inputs are not bf16-representable and at least 0.5% are exact ties;
    (d) at least 25% of the final outputs are non-zero;
    (e) average pooling only over a power-of-two window;
    (f) no dead channel: every input column of every layer is non-zero in at least 2% of the rows (with (b): a fault in any column shows).
    expected() itself asserts that every intermediate value is exactly representable in fp32.  Returns the per-layer figures."""
    stats = []
    out, _ = expected(inp, stack, precision, pool=pool, S=S, stats=stats)
    for s in stats:
        assert s["span"] < 2.0 ** SPAN_BITS * s["u"], f"(a) layer {s['layer']}: span {s['span']} >= 2^{SPAN_BITS} * {s['u']}"
        if s["layer"] == "avg":
            assert S & (S - 1) == 0, "(e) average pooling needs a power-of-two window"
            continue
        assert s["cover"], f"(b) layer {s['layer']}: an input column without a weight"
        assert s["live"] >= 0.02, f"(f) layer {s['layer']}: an input column that is zero in all but {s['live']:.3f} of the rows"
        if s["rounded"]:
            assert s["inexact"] >= 0.10, f"(c) layer {s['layer']}: only {s['inexact']:.3f} of the inputs round"
            assert s["ties"] >= 0.005, f"(c) layer {s['layer']}: only {s['ties']:.4f} of the inputs are ties"
    assert float((out != 0).double().mean()) >= 0.25, "(d) degenerate output"
    return stats


# ---------------------------------------------------------------------------------------------------------------- the cases (shared by the CPU and GPU tests)
NNZ = (10, 6, 4, 4)       # non-zeros per weight row, by layer: as dense as condition (a) allows ("bf16" stays below 2^20 u, unrounded operands below 2^22 u)
ALL = ("bf16", "fp32", "bf16x3")
_DEEP = dict(exact_nnz=(8, 4, 4, 4), exact_frac=5)   # four layers with unrounded operands: a coarser input lattice keeps condition (a)


def _case(id, widths, kind, shape, pool=0, S=1, tap=None, window=None, precisions=("bf16",), nnz=NNZ, relu_last=False, unit_scale=False, seed=None, **extra):
    return dict(id=id, widths=tuple(widths), kind=kind, shape=shape, pool=pool, S=S, tap=tap, window=window, precisions=precisions, nnz=nnz,
                relu_last=relu_last, unit_scale=unit_scale, seed=seed if seed is not None else sum(widths) + 7 * len(id), **extra)


def _grp(B, N, P, S, C):
    return dict(B=B, N=N, P=P, S=S, C=C)


def _itp(B, n, m, C2, C1=0):
    return dict(B=B, n=n, m=m, C2=C2, C1=C1)


# fused.mlp_stack: every case label of the bf16 switch in csrc/mlp_chain_bf16.hip, the six width keys the fp32 chain kernel alone instantiates
# (LDS stack kernel in "bf16", fp32 chain kernel in "bf16x3"), stacks no chain kernel takes; ragged K0 in {3, 40, 67, 99, 195, 188}; the three
# loaders; no pool, max over 4 / 8 / 16 / 32 / 64, average over 4 / 64; row counts that are no multiple of 16 / 32 / 64 / 128 wherever the pool
# window allows, one single row tile, one launch of >= 65,600 rows (32 rows per wave); a tapped hidden layer; an output window.
STACK_CASES = [
    _case("16-16-32.group.max16", (3, 16, 16, 32), "group", _grp(2, 50, 5, 16, 0), pool=1, S=16, precisions=ALL),
    _case("32-32-64.group.max32", (99, 32, 32, 64), "group", _grp(1, 40, 3, 32, 96), pool=1, S=32, precisions=ALL),
    _case("64-64-128.group.max64", (195, 64, 64, 128), "group", _grp(1, 70, 3, 64, 192), pool=1, S=64, precisions=ALL),
    _case("128-128-256.group.max8", (195, 128, 128, 256), "group", _grp(1, 30, 13, 8, 192), pool=1, S=8, precisions=ALL),
    _case("32-32.direct", (67, 32, 32), "direct", dict(rows=77), precisions=ALL),
    _case("64-64.direct.avg4", (40, 64, 64), "direct", dict(rows=148), pool=2, S=4, precisions=ALL),
    _case("128-128.interp", (188, 128, 128), "interp", _itp(2, 45, 7, 128, 60), precisions=ALL),
    _case("128-64.direct.one_tile", (99, 128, 64), "direct", dict(rows=13), precisions=ALL),
    _case("256-128.interp", (352, 256, 128), "interp", _itp(1, 70, 9, 256, 96), precisions=ALL),
    _case("16.direct.max4", (40, 16), "direct", dict(rows=76), pool=1, S=4, precisions=ALL),
    _case("32.direct.window", (67, 32), "direct", dict(rows=100), window=(5, 4), precisions=ALL),
    _case("64.group.avg64", (3, 64), "group", _grp(1, 80, 3, 64, 0), pool=2, S=64, precisions=ALL),
    _case("128.direct", (195, 128), "direct", dict(rows=150), precisions=ALL),
    _case("128-64-32-7.interp.tap", (128, 128, 64, 32, 7), "interp", _itp(1, 75, 9, 128), tap=1, nnz=(8, 4, 4, 4), precisions=ALL, **_DEEP),
    _case("128-64-32-16.direct.window", (40, 128, 64, 32, 16), "direct", dict(rows=45), window=(3, 6), tap=2, nnz=(8, 4, 4, 4), precisions=ALL, **_DEEP),
    _case("32-32.direct.65611rows", (40, 32, 32), "direct", dict(rows=65611), precisions=("bf16", "bf16x3")),
    # the six keys without a bf16 instantiation
    _case("256.direct", (40, 256), "direct", dict(rows=70), precisions=ALL),
    _case("256-128-128.direct", (99, 256, 128, 128), "direct", dict(rows=83), tap=1, precisions=ALL),
    _case("64-32-7.direct", (67, 64, 32, 7), "direct", dict(rows=90), precisions=ALL),
    _case("32-64.group.max16", (35, 32, 64), "group", _grp(2, 40, 5, 16, 32), pool=1, S=16, precisions=ALL),
    _case("64-128.direct.max32", (67, 64, 128), "direct", dict(rows=96), pool=1, S=32, precisions=ALL),
    _case("128-256.interp", (99, 128, 256), "interp", _itp(1, 50, 6, 64, 35), precisions=ALL),
    # no chain kernel at all: the LDS stack kernel
    _case("64-48.group.max16", (70, 64, 48), "group", _grp(1, 33, 7, 16, 67), pool=1, S=16),
    _case("512-256.interp", (576, 512, 256), "interp", _itp(1, 90, 11, 384, 192)),
    _case("64-32-16-8.direct.tap", (40, 64, 32, 16, 8), "direct", dict(rows=110), tap=2, nnz=(8, 4, 4, 4)),
]

# the bf16 switch's case labels (16-channel tiles per layer) -> the STACK_CASES that run them; tests/test_bf16_exact_cpu.py checks this against the source
BF16_SWITCH_TILES = {(1, 1, 2), (2, 2, 4), (4, 4, 8), (8, 8, 16), (2, 2), (4, 4), (8, 8), (8, 4), (16, 8), (1,), (2,), (4,), (8,), (8, 4, 2, 1)}
FP32_ONLY_TILES = {(16,), (16, 8, 8), (4, 2, 1), (2, 4), (4, 8), (8, 16)}


def tiles(widths):
    return tuple((c + 15) // 16 for c in widths[1:])


# csrc/sa_group_bf16.hip through fused.sa_forward: one case per instantiation (T1, S, C) at two sizes -- `small`: a ragged number of
# neighbourhoods (no multiple of the 4 or 8 waves of a workgroup), three different clouds; `large`: ONE cloud of P neighbourhoods repeated
# `rep` times (the expected output is computed once), sized from the grid computation at the end of sa_group_bf16_launch: the grid is
# min(ceil(units / NW), resident workgroups), resident <= 8 per CU (32 wave slots / 4 waves) x 256 CUs for the 4-wave kernels and 1 per CU
# (157 KB of LDS) for the 8-wave one, so rep * P >= 3 * 8192 units of one tile (S = 16), 2 * 8192 units of two tiles (S = 32) and
# 2 * 2048 units of four tiles (S = 64) give every resident wave at least three tiles across at least one neighbourhood boundary.
def _sa(T1, S, C, B, N, P, rep=1, pad=False):
    w = (3 + C, 16 * T1, 16 * T1, 32 * T1)
    return _case(f"T{T1}.S{S}.C{C}.{'large' if rep > 1 else 'pad' if pad else 'small'}", w, "group", _grp(B, N, P, S, C), pool=1, S=S, relu_last=True,
                 unit_scale=True, rep=rep, pad=pad)


SA_CASES = [
    _sa(1, 16, 0, 3, 60, 7), _sa(1, 16, 0, 1, 100, 193, rep=128),
    _sa(2, 32, 0, 3, 60, 7), _sa(2, 32, 0, 1, 100, 129, rep=128),
    _sa(2, 16, 96, 3, 60, 7), _sa(2, 16, 96, 1, 100, 193, rep=128),
    _sa(4, 32, 96, 3, 60, 7), _sa(4, 32, 96, 1, 100, 129, rep=128),
    _sa(4, 32, 192, 3, 60, 7), _sa(4, 32, 192, 1, 100, 129, rep=128),
    _sa(8, 64, 192, 3, 60, 11), _sa(8, 64, 192, 1, 70, 33, rep=128),
    _sa(8, 64, 192, 2, 60, 11, pad=True),
]

# csrc/fp_head_bf16.hip through fused.fp_forward(..., head=): interpolated 128 -> 128 -> 64 (the FP output, tapped) -> 32 -> 7
FP_HEAD_CASES = [_case(f"B{B}.n{n}.m{m}", (128, 128, 64, 32, 7), "interp", _itp(B, n, m, 128), tap=1, nnz=(8, 4, 4, 4), unit_scale=True)
                 for B, n, m in [(3, 5000, 300), (1, 4100, 257), (2, 16, 5)]]

# csrc/gemm_bf16.hip through fused.fp_forward: (C2, C1, mlp); row counts that are no multiple of 128
GEMM_CASES = [_case("188-512-128", (188, 512, 128), "interp", _itp(2, 333, 40, 128, 60), relu_last=True, unit_scale=True),
              _case("576-512-256", (576, 512, 256), "interp", _itp(1, 205, 33, 384, 192), relu_last=True, unit_scale=True)]

# the public routes onto widths without a bf16 instantiation: an SA module with mlp = [C, 32, 64], an FP module and an FC stack with a single 256-wide layer
MODULE_CASES = [_case("sa.32-64", (35, 32, 64), "group", _grp(2, 40, 5, 16, 32), pool=1, S=16, relu_last=True, unit_scale=True, precisions=("bf16", "bf16x3")),
                _case("fp.256", (40, 256), "interp", _itp(2, 37, 6, 40), relu_last=True, unit_scale=True, precisions=("bf16", "bf16x3")),
                _case("fc.256", (40, 256), "direct", dict(rows=70), relu_last=True, unit_scale=True, precisions=("bf16", "bf16x3"))]

_BUILT = {}


def build(case, precision="bf16"):
    """(inputs, stack) of a case, built once.  The same for every precision, except where the case names another stack / coarser inputs for
    the precisions that do not round ("fp32", "bf16x3": every layer then ADDS lattice bits instead of being cut back to eight)."""
    exact = precision != "bf16" and "exact_nnz" in case
    key = (id(case), exact)
    if key not in _BUILT:
        sh = dict(case["shape"])
        idx = None
        if case.get("pad"):        # ball-query padding: whole 16-row tiles repeating the neighbourhood's first index (dead tiles), a dead tile with live rows behind it
            g = _gen(case["seed"] + 1)
            idx = torch.randint(0, sh["N"], (sh["B"], sh["P"], sh["S"]), generator=g, dtype=torch.int32)
            first = idx[..., :1]
            idx[:, 0::4, 16:] = first[:, 0::4]
            idx[:, 1::4, 16:32] = first[:, 1::4]
            idx[:, 2::4, :] = first[:, 2::4]
        if case["kind"] == "direct":
            sh["K0"] = case["widths"][0]
        inp = make_inputs(case["kind"], case["seed"], idx=idx, frac=case["exact_frac"] if exact else 8, **sh)
        assert inp["K0"] == case["widths"][0]
        stack = make_stack(case["widths"], case["seed"] + 100, nnz=case["exact_nnz"] if exact else case["nnz"], relu_last=case["relu_last"], unit_scale=case["unit_scale"],
                           probe=layer0_rows(inp)[:1024])
        _BUILT[key] = (inp, stack)
    return _BUILT[key]


_WANT = {}


def want(case, precision):
    """expected(...) of a case, computed once per precision and shared by the tests that need it (treat as read-only)."""
    key = (id(case), precision)
    if key not in _WANT:
        inp, stack = build(case, precision)
        _WANT[key] = expected(inp, stack, precision, pool=case["pool"], S=case["S"], tap=case["tap"])
    return _WANT[key]

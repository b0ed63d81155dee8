"""The two doors of the whole-stack MLP launchers (include/g4d.h): ONE description of a call -- a dict keyed by the field names of g4d_mlp_args --
goes through the family's positional entry point and through g4d_mlp_run.  Shared by test_mlp_doors_cpu.py (the error behaviour of both) and
test_mlp_doors_gpu.py (both launch the same thing)."""
import ctypes

from garment4d_amd import _lib

_LOADERS = ["mode", "rows", "K0", "X", "ldx", "N", "P", "S", "C", "use_xyz", "xyz", "new_xyz", "feats", "idx",
            "n", "m", "C2", "C1", "known_feats", "skip", "dist2", "nn_idx"]
_CSR = ["Vg", "rowptr", "colidx", "vals"]
_LAYERS = ["nlayers", "W", "scale", "shift", "Kpad", "Cout", "relu", "pool", "out", "ldo", "col0"]
_TAP = ["tap_layer", "tap_out", "tap_ld"]

# family -> (positional entry point, g4d_mlp_family, the argument names of the entry point in its order)
FAMILIES = {
    "stack_f32": ("g4d_mlp_stack_f32", _lib.MLP_STACK_F32, _LOADERS + _CSR + _LAYERS + _TAP),
    "stack_bf16": ("g4d_mlp_stack_bf16", _lib.MLP_STACK_BF16, _LOADERS + _CSR + _LAYERS + _TAP),
    "wave_f32": ("g4d_mlp_wave_f32", _lib.MLP_WAVE_F32, _LOADERS + _CSR + _LAYERS),
    "chain_f32": ("g4d_mlp_chain_f32", _lib.MLP_CHAIN_F32, _LOADERS + _LAYERS + _TAP),
    "chain_bf16": ("g4d_mlp_chain_bf16", _lib.MLP_CHAIN_BF16, _LOADERS + _LAYERS + _TAP),
    "chain_cells_bf16": ("g4d_mlp_chain_cells_bf16", _lib.MLP_CHAIN_BF16, _LOADERS + _LAYERS + _TAP + ["unknown_grid"]),
    "chain_bf16x3": ("g4d_mlp_chain_bf16x3", _lib.MLP_CHAIN_BF16X3, _LOADERS + _LAYERS + _TAP),
}


def host_ints(values):
    return (ctypes.c_int * len(values))(*values)


def host_ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def _arg(v):
    return ctypes.cast(v, ctypes.c_void_p) if isinstance(v, ctypes.Array) else v


def _status(rc):
    return rc, (_lib.lib().g4d_last_error().decode() if rc else "")


def positional(family, fields, stream=None):
    """(status, error text) of the call through the family's positional entry point; fields the entry point does not take must be unset."""
    name, _, order = FAMILIES[family]
    assert set(fields) <= set(order), (family, sorted(set(fields) - set(order)))
    args = [_arg(fields.get(k, -1 if k == "tap_layer" else 0)) for k in order]
    return _status(getattr(_lib.lib(), name)(*args, stream))


def block(fields):
    a = _lib.MlpArgs(**{k: _arg(v) for k, v in fields.items() if k != "tap_layer"})
    a.tap_layer = fields.get("tap_layer", -1)
    a._keep = fields     # the host arrays the block points at
    return a


def run(family, fields, stream=None):
    """(status, error text) of the same call through g4d_mlp_run."""
    a = block(fields)
    return _status(_lib.lib().g4d_mlp_run(FAMILIES[family][1], ctypes.addressof(a), stream))


# ---- GPU side (test_mlp_doors_gpu.py): exact-lattice tensors on the device, packed layers, comparison with the float64 twin
SENTINEL = -12345.0


def dev(t):
    """A float64 twin tensor as fp32 on the GPU; it must be exactly representable."""
    import torch
    assert torch.equal(t.to(torch.float32).to(torch.float64), t)
    return t.to(torch.float32).cuda().contiguous()


def packed(stack):
    from garment4d_amd import fused
    return [fused.PackedLayer(dev(W), dev(sc), dev(sh), relu=relu) for W, sc, sh, relu in stack]


def same(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} values differ from the exact twin, first at {bad.nonzero()[0].tolist()}"

"""Error behaviour of the whole-stack MLP launchers, pinned: every bad call below is refused before the device is touched, with the SAME status
and g4d_last_error() text through the positional entry point and through g4d_mlp_run -- and that pair equals the literal recorded here from the
library as it was before the argument block became the launchers' internal interface (the shared validation must not have changed what any
family says, nor which entry point's name a message carries)."""
import ctypes

import pytest

import mlp_doors as D
from garment4d_amd import _lib

EINVAL = 10001
DEV = 0x10000   # stands for device memory: never dereferenced by a call that is refused


def call(family, Kpad=(32, 32, 32), Cout=(32, 32, 64), W="dev", **over):
    """A DIRECT 64 x 32 launch of the 32-32-64 stack (valid as it stands) with `over` laid over it."""
    n = len(Cout)
    pieces = 3 if family == "chain_bf16x3" else 1
    f = dict(mode=0, rows=64, K0=32, X=DEV, ldx=32, nlayers=n, W=D.host_ptrs([DEV] * (pieces * n)) if W == "dev" else W,
             scale=D.host_ptrs([DEV] * n), shift=D.host_ptrs([DEV] * n), Kpad=D.host_ints(Kpad), Cout=D.host_ints(Cout),
             relu=D.host_ints([1] * (n - 1) + [0]), out=DEV, ldo=64)
    if family == "chain_cells_bf16":
        f["unknown_grid"] = DEV
    f.update(over)
    return f


STACKS, CHAINS = ("stack_f32", "stack_bf16", "wave_f32"), ("chain_f32", "chain_bf16", "chain_cells_bf16", "chain_bf16x3")
TAPPED = ("stack_f32", "stack_bf16") + CHAINS
BF16_CHAINS = ("chain_bf16", "chain_cells_bf16", "chain_bf16x3")

# (case, families, the call)
CASES = [
    ("bad mode", STACKS + CHAINS, lambda fam: call(fam, mode=4)),
    ("csr mode", CHAINS, lambda fam: call(fam, mode=3)),
    ("no layers", STACKS + CHAINS, lambda fam: call(fam, nlayers=0)),
    ("five layers", STACKS + CHAINS, lambda fam: call(fam, Kpad=(32,) * 5, Cout=(32,) * 5)),
    ("rows < 0", STACKS + CHAINS, lambda fam: call(fam, rows=-64)),
    ("K0 = 0", STACKS + CHAINS, lambda fam: call(fam, K0=0)),
    ("null W", STACKS + CHAINS, lambda fam: call(fam, W=0)),
    ("pool = 3", STACKS + CHAINS, lambda fam: call(fam, pool=3, S=16)),
    ("pool over S = 5", STACKS + CHAINS, lambda fam: call(fam, pool=1, S=5)),
    ("Kpad % 32", STACKS + BF16_CHAINS, lambda fam: call(fam, Kpad=(32, 48, 32))),
    ("Kpad % 16", ("chain_f32",), lambda fam: call(fam, Kpad=(32, 40, 32))),
    ("K does not chain", ("stack_f32", "stack_bf16"), lambda fam: call(fam, Kpad=(32, 128, 32))),
    ("Kpad of a hidden layer too small", CHAINS, lambda fam: call(fam, Kpad=(32, 0, 32))),
    ("Kpad[0] < K0", STACKS + CHAINS, lambda fam: call(fam, K0=40, ldx=40)),
    ("tap on the last layer", TAPPED, lambda fam: call(fam, tap_layer=2, tap_out=DEV, tap_ld=64)),
    ("too wide for LDS", ("stack_f32",), lambda fam: call(fam, Kpad=(320, 320), Cout=(320, 64), K0=320, ldx=320)),
    ("too wide for LDS", ("stack_bf16",), lambda fam: call(fam, Kpad=(608, 608), Cout=(608, 64), K0=608, ldx=608)),
    ("hidden width > 64", ("wave_f32",), lambda fam: call(fam, Kpad=(32, 96, 32), Cout=(96, 32, 64))),
    ("unsupported chain widths", CHAINS, lambda fam: call(fam, Kpad=(32, 64), Cout=(48, 48))),
    ("no bf16 instantiation", BF16_CHAINS, lambda fam: call(fam, Kpad=(32, 32), Cout=(32, 64))),
    ("null mid piece", ("chain_bf16x3",), lambda fam: call(fam, W=D.host_ptrs([DEV, 0, DEV] + [DEV] * 6))),
]

# (family, case) -> the text both doors report with status 10001; recorded from the library of the commit before this file existed
EXPECTED = {
    ('stack_f32', 'bad mode'): 'g4d_mlp_stack_f32: bad mode',
    ('stack_bf16', 'bad mode'): 'g4d_mlp_stack_bf16: bad mode',
    ('wave_f32', 'bad mode'): 'g4d_mlp_wave_f32: bad mode',
    ('chain_f32', 'bad mode'): 'g4d_mlp_chain_f32: mode must be 0 (direct), 1 (group) or 2 (interp)',
    ('chain_bf16', 'bad mode'): 'g4d_mlp_chain_bf16: mode must be 0, 1 or 2',
    ('chain_cells_bf16', 'bad mode'): 'g4d_mlp_chain_bf16: mode must be 0, 1 or 2',
    ('chain_bf16x3', 'bad mode'): 'g4d_mlp_chain_bf16x3: mode must be 0, 1 or 2',
    ('chain_f32', 'csr mode'): 'g4d_mlp_chain_f32: mode must be 0 (direct), 1 (group) or 2 (interp)',
    ('chain_bf16', 'csr mode'): 'g4d_mlp_chain_bf16: mode must be 0, 1 or 2',
    ('chain_cells_bf16', 'csr mode'): 'g4d_mlp_chain_bf16: mode must be 0, 1 or 2',
    ('chain_bf16x3', 'csr mode'): 'g4d_mlp_chain_bf16x3: mode must be 0, 1 or 2',
    ('stack_f32', 'no layers'): 'g4d_mlp_stack_f32: 1..4 layers',
    ('stack_bf16', 'no layers'): 'g4d_mlp_stack_bf16: 1..4 layers',
    ('wave_f32', 'no layers'): 'g4d_mlp_wave_f32: 1..4 layers',
    ('chain_f32', 'no layers'): 'g4d_mlp_chain_f32: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_bf16', 'no layers'): 'g4d_mlp_chain_bf16: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_cells_bf16', 'no layers'): 'g4d_mlp_chain_bf16: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_bf16x3', 'no layers'): 'g4d_mlp_chain_bf16x3: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('stack_f32', 'five layers'): 'g4d_mlp_stack_f32: 1..4 layers',
    ('stack_bf16', 'five layers'): 'g4d_mlp_stack_bf16: 1..4 layers',
    ('wave_f32', 'five layers'): 'g4d_mlp_wave_f32: 1..4 layers',
    ('chain_f32', 'five layers'): 'g4d_mlp_chain_f32: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_bf16', 'five layers'): 'g4d_mlp_chain_bf16: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_cells_bf16', 'five layers'): 'g4d_mlp_chain_bf16: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_bf16x3', 'five layers'): 'g4d_mlp_chain_bf16x3: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('stack_f32', 'rows < 0'): 'g4d_mlp_stack_f32: bad sizes',
    ('stack_bf16', 'rows < 0'): 'g4d_mlp_stack_bf16: bad sizes',
    ('wave_f32', 'rows < 0'): 'g4d_mlp_wave_f32: bad sizes',
    ('chain_f32', 'rows < 0'): 'g4d_mlp_chain_f32: bad sizes',
    ('chain_bf16', 'rows < 0'): 'g4d_mlp_chain_bf16: bad sizes',
    ('chain_cells_bf16', 'rows < 0'): 'g4d_mlp_chain_bf16: bad sizes',
    ('chain_bf16x3', 'rows < 0'): 'g4d_mlp_chain_bf16x3: bad sizes',
    ('stack_f32', 'K0 = 0'): 'g4d_mlp_stack_f32: bad sizes',
    ('stack_bf16', 'K0 = 0'): 'g4d_mlp_stack_bf16: bad sizes',
    ('wave_f32', 'K0 = 0'): 'g4d_mlp_wave_f32: bad sizes',
    ('chain_f32', 'K0 = 0'): 'g4d_mlp_chain_f32: bad sizes',
    ('chain_bf16', 'K0 = 0'): 'g4d_mlp_chain_bf16: bad sizes',
    ('chain_cells_bf16', 'K0 = 0'): 'g4d_mlp_chain_bf16: bad sizes',
    ('chain_bf16x3', 'K0 = 0'): 'g4d_mlp_chain_bf16x3: bad sizes',
    ('stack_f32', 'null W'): 'g4d_mlp_stack_f32: null pointer',
    ('stack_bf16', 'null W'): 'g4d_mlp_stack_bf16: null pointer',
    ('wave_f32', 'null W'): 'g4d_mlp_wave_f32: null pointer',
    ('chain_f32', 'null W'): 'g4d_mlp_chain_f32: null pointer',
    ('chain_bf16', 'null W'): 'g4d_mlp_chain_bf16: null pointer',
    ('chain_cells_bf16', 'null W'): 'g4d_mlp_chain_bf16: null pointer',
    ('chain_bf16x3', 'null W'): 'g4d_mlp_chain_bf16x3: null pointer',
    ('stack_f32', 'pool = 3'): 'g4d_mlp_stack_f32: pool must be 0|1|2',
    ('stack_bf16', 'pool = 3'): 'g4d_mlp_stack_bf16: pool must be 0|1|2',
    ('wave_f32', 'pool = 3'): 'g4d_mlp_wave_f32: pool must be 0|1|2',
    ('chain_f32', 'pool = 3'): 'g4d_mlp_chain_f32: pool must be 0|1|2',
    ('chain_bf16', 'pool = 3'): 'g4d_mlp_chain_bf16: pool must be 0|1|2',
    ('chain_cells_bf16', 'pool = 3'): 'g4d_mlp_chain_bf16: pool must be 0|1|2',
    ('chain_bf16x3', 'pool = 3'): 'g4d_mlp_chain_bf16x3: pool must be 0|1|2',
    ('stack_f32', 'pool over S = 5'): 'g4d_mlp_stack_f32: pooling needs S in {4,8,16,32,64}',
    ('stack_bf16', 'pool over S = 5'): 'g4d_mlp_stack_bf16: pooling needs S in {4,8,16,32,64}',
    ('wave_f32', 'pool over S = 5'): 'g4d_mlp_wave_f32: pooling needs S in {4,8,16,32,64}',
    ('chain_f32', 'pool over S = 5'): 'g4d_mlp_chain_f32: pooling needs S in {4,8,16,32,64}',
    ('chain_bf16', 'pool over S = 5'): 'g4d_mlp_chain_bf16: pooling needs S in {4,8,16,32,64}',
    ('chain_cells_bf16', 'pool over S = 5'): 'g4d_mlp_chain_bf16: pooling needs S in {4,8,16,32,64}',
    ('chain_bf16x3', 'pool over S = 5'): 'g4d_mlp_chain_bf16x3: pooling needs S in {4,8,16,32,64}',
    ('stack_f32', 'Kpad % 32'): 'g4d_mlp_stack_f32: bad layer 1',
    ('stack_bf16', 'Kpad % 32'): 'g4d_mlp_stack_bf16: bad layer 1',
    ('wave_f32', 'Kpad % 32'): 'g4d_mlp_wave_f32: bad layer 1',
    ('chain_bf16', 'Kpad % 32'): 'g4d_mlp_chain_bf16: bad layer 1',
    ('chain_cells_bf16', 'Kpad % 32'): 'g4d_mlp_chain_bf16: bad layer 1',
    ('chain_bf16x3', 'Kpad % 32'): 'g4d_mlp_chain_bf16x3: bad layer 1',
    ('chain_f32', 'Kpad % 16'): 'g4d_mlp_chain_f32: bad layer 1',
    ('stack_f32', 'K does not chain'): 'g4d_mlp_stack_f32: layer 1 K does not chain',
    ('stack_bf16', 'K does not chain'): 'g4d_mlp_stack_bf16: layer 1 K does not chain',
    ('chain_f32', 'Kpad of a hidden layer too small'): 'g4d_mlp_chain_f32: Kpad of layer 1 too small',
    ('chain_bf16', 'Kpad of a hidden layer too small'): 'g4d_mlp_chain_bf16: Kpad of layer 1 too small',
    ('chain_cells_bf16', 'Kpad of a hidden layer too small'): 'g4d_mlp_chain_bf16: Kpad of layer 1 too small',
    ('chain_bf16x3', 'Kpad of a hidden layer too small'): 'g4d_mlp_chain_bf16x3: Kpad of layer 1 too small',
    ('stack_f32', 'Kpad[0] < K0'): 'g4d_mlp_stack_f32: Kpad[0] < K0',
    ('stack_bf16', 'Kpad[0] < K0'): 'g4d_mlp_stack_bf16: Kpad[0] < K0',
    ('wave_f32', 'Kpad[0] < K0'): 'g4d_mlp_wave_f32: Kpad[0] < K0',
    ('chain_f32', 'Kpad[0] < K0'): 'g4d_mlp_chain_f32: Kpad of layer 0 too small',
    ('chain_bf16', 'Kpad[0] < K0'): 'g4d_mlp_chain_bf16: Kpad of layer 0 too small',
    ('chain_cells_bf16', 'Kpad[0] < K0'): 'g4d_mlp_chain_bf16: Kpad of layer 0 too small',
    ('chain_bf16x3', 'Kpad[0] < K0'): 'g4d_mlp_chain_bf16x3: Kpad of layer 0 too small',
    ('stack_f32', 'tap on the last layer'): 'g4d_mlp_stack_f32: tap must be a hidden layer',
    ('stack_bf16', 'tap on the last layer'): 'g4d_mlp_stack_bf16: tap must be a hidden layer',
    ('chain_f32', 'tap on the last layer'): 'g4d_mlp_chain_f32: tap must be a hidden layer',
    ('chain_bf16', 'tap on the last layer'): 'g4d_mlp_chain_bf16: tap must be a hidden layer',
    ('chain_cells_bf16', 'tap on the last layer'): 'g4d_mlp_chain_bf16: tap must be a hidden layer',
    ('chain_bf16x3', 'tap on the last layer'): 'g4d_mlp_chain_bf16x3: tap must be a hidden layer',
    ('stack_f32', 'too wide for LDS'): 'g4d_mlp_stack_f32: stack too wide for LDS (167936 bytes)',
    ('stack_bf16', 'too wide for LDS'): 'g4d_mlp_stack_bf16: stack too wide for LDS (157696 bytes)',
    ('wave_f32', 'hidden width > 64'): 'g4d_mlp_wave_f32: hidden width of layer 0 > 64',
    ('chain_f32', 'unsupported chain widths'): 'g4d_mlp_chain_f32: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_bf16', 'unsupported chain widths'): 'g4d_mlp_chain_bf16: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_cells_bf16', 'unsupported chain widths'): 'g4d_mlp_chain_bf16: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_bf16x3', 'unsupported chain widths'): 'g4d_mlp_chain_bf16x3: unsupported layer widths (see g4d_mlp_chain_supported)',
    ('chain_bf16', 'no bf16 instantiation'): 'g4d_mlp_chain_bf16: no bf16 instantiation for these widths (key 2040000)',
    ('chain_cells_bf16', 'no bf16 instantiation'): 'g4d_mlp_chain_bf16: no bf16 instantiation for these widths (key 2040000)',
    ('chain_bf16x3', 'no bf16 instantiation'): 'g4d_mlp_chain_bf16x3: no bf16 instantiation for these widths (key 2040000)',
    ('chain_bf16x3', 'null mid piece'): 'g4d_mlp_chain_bf16x3: bad layer 0',
}


@pytest.mark.parametrize("case,family", [(c, fam) for c, fams, _ in CASES for fam in fams])
def test_bad_call_is_refused_alike_through_both_doors(case, family):
    make = next(m for c, fams, m in CASES if c == case and family in fams)
    pos, blk = D.positional(family, make(family)), D.run(family, make(family))
    assert pos == blk, (pos, blk)
    assert pos == (EINVAL, EXPECTED[family, case]), pos


# Two faults in one call: the checks the families share run first, in the order of stack_call_check, then the family's own.  (Before the shared
# validation a family interleaved them -- "K does not chain" of layer 1 came before "bad layer 2" -- so these texts are the order as it is now.)
TWO_FAULTS = {
    "stack_f32": (dict(Kpad=(32, 128, 40)), "g4d_mlp_stack_f32: bad layer 2"),
    "stack_bf16": (dict(Kpad=(32, 128, 40)), "g4d_mlp_stack_bf16: bad layer 2"),
    "wave_f32": (dict(Kpad=(32, 96, 40), Cout=(96, 32, 64)), "g4d_mlp_wave_f32: bad layer 2"),
    "chain_f32": (dict(Kpad=(32, 0, 32), tap_layer=2, tap_out=DEV, tap_ld=64), "g4d_mlp_chain_f32: tap must be a hidden layer"),
    "chain_bf16": (dict(Kpad=(32, 0, 32), tap_layer=2, tap_out=DEV, tap_ld=64), "g4d_mlp_chain_bf16: tap must be a hidden layer"),
    "chain_cells_bf16": (dict(Kpad=(32, 0, 40)), "g4d_mlp_chain_bf16: bad layer 2"),
    "chain_bf16x3": (dict(Kpad=(32, 0, 32), pool=3), "g4d_mlp_chain_bf16x3: pool must be 0|1|2"),
}


@pytest.mark.parametrize("family", sorted(TWO_FAULTS))
def test_two_faults_report_the_shared_check_first(family):
    over, text = TWO_FAULTS[family]
    assert D.positional(family, call(family, **over)) == D.run(family, call(family, **over)) == (EINVAL, text)


def test_wave_refuses_a_tap_through_the_block():
    """(the positional entry point has no tap arguments)"""
    assert D.run("wave_f32", call("wave_f32", tap_layer=0, tap_out=DEV, tap_ld=32)) == \
        (EINVAL, "g4d_mlp_run(G4D_MLP_WAVE_F32): the wave-autonomous kernel has no tap")


@pytest.mark.parametrize("family", STACKS + CHAINS)
def test_empty_launch_returns_before_the_pointer_checks(family):
    """rows == 0 is G4D_OK once mode, layer count and sizes are sane -- null arrays and all -- and an error before that."""
    empty = lambda **over: dict(call(family, rows=0, **over), W=0, scale=0, shift=0, Kpad=0, Cout=0, relu=0, out=0)
    assert D.positional(family, empty()) == D.run(family, empty()) == (0, "")
    pos, blk = D.positional(family, empty(mode=5)), D.run(family, empty(mode=5))
    assert pos == blk and pos[0] == EINVAL and "mode" in pos[1]


# the table entry points have one door; they report as the register-chain launcher they end in (or under their own name for their own checks)
TABLE_CASES = {
    "table: unsupported widths": ("g4d_mlp_chain_table_f32", lambda c: (64, 32, 8, 32, DEV, DEV, DEV, DEV, DEV, 0, 0, 2, *c((32, 64), (48, 48)), DEV, 64, 0, -1, 0, 0, None)),
    "table: C2 % 16": ("g4d_mlp_chain_table_f32", lambda c: (64, 32, 8, 24, DEV, DEV, DEV, DEV, DEV, 0, 0, 2, *c((32, 32), (32, 32)), DEV, 64, 0, -1, 0, 0, None)),
    "table: null table": ("g4d_mlp_chain_table_f32", lambda c: (64, 32, 8, 32, 0, DEV, DEV, DEV, DEV, 0, 0, 2, *c((32, 32), (32, 32)), DEV, 64, 0, -1, 0, 0, None)),
    "cells: broken clouds": ("g4d_mlp_chain_table_cells_f32", lambda c: (64, 48, 8, 32, DEV, DEV, DEV, DEV, DEV, DEV, 0, 0, 2, *c((32, 32), (32, 32)), DEV, 64, 0, -1, 0, 0, None)),
    "cells: null grid": ("g4d_mlp_chain_table_cells_f32", lambda c: (64, 32, 8, 32, DEV, DEV, DEV, 0, DEV, DEV, 0, 0, 2, *c((32, 32), (32, 32)), DEV, 64, 0, -1, 0, 0, None)),
    "group table: pool = 3": ("g4d_mlp_chain_group_table_f32", lambda c: (64, 32, 2, 16, DEV, DEV, DEV, DEV, 32, 32, DEV, DEV, DEV, 2, *c((32, 32), (32, 64)), 3, DEV, 64, 0, None)),
    "group table: Kt % 16": ("g4d_mlp_chain_group_table_ws_f32", lambda c: (64, 32, 2, 16, DEV, DEV, DEV, DEV, 40, 40, DEV, DEV, DEV, 2, *c((64, 32), (32, 64)), 1, DEV, 64, 0, 0, 0, None)),
    "group table: null table": ("g4d_mlp_chain_group_table_f32", lambda c: (64, 32, 2, 16, DEV, DEV, DEV, 0, 32, 32, DEV, DEV, DEV, 2, *c((32, 32), (32, 64)), 1, DEV, 64, 0, None)),
    "interp init: one layer": ("g4d_mlp_chain_interp_init_f32", lambda c: (64, 32, 8, 32, DEV, DEV, 32, DEV, DEV, 1, *c((32,), (32,)), DEV, 64, 0, -1, 0, 0, None)),
    "interp init: tap on the last layer": ("g4d_mlp_chain_interp_init_f32", lambda c: (64, 32, 8, 32, DEV, DEV, 32, DEV, DEV, 2, *c((32, 32), (32, 32)), DEV, 64, 0, 1, DEV, 32, None)),
}
TABLE_EXPECTED = {
    'cells: broken clouds': 'g4d_mlp_chain_*_cells_f32: cell-ordered rows need the interpolating loader, no pooling, whole clouds',
    'cells: null grid': 'g4d_mlp_chain_table_cells_f32: null pointer',
    'group table: Kt % 16': 'g4d_mlp_chain_group_table_f32: needs a 16-byte aligned table whose width is a multiple of 16, the xyz weights, the affine and the grouping inputs',
    'group table: null table': 'g4d_mlp_chain_group_table_f32: null table',
    'group table: pool = 3': 'g4d_mlp_chain_f32: pool must be 0|1|2',
    'interp init: one layer': 'g4d_mlp_chain_interp_init_f32: needs skip features, >= 2 layers, a first-layer width that is a multiple of 16 and a 16-byte aligned table at least that wide',
    'interp init: tap on the last layer': 'g4d_mlp_chain_f32: tap must be a hidden layer',
    'table: C2 % 16': 'g4d_mlp_chain_table_f32: needs the interpolating loader, no skip features and a table width that is a multiple of 16',
    'table: null table': 'g4d_mlp_chain_table_f32: null pointer',
    'table: unsupported widths': 'g4d_mlp_chain_f32: unsupported layer widths (see g4d_mlp_chain_supported)',
}


@pytest.mark.parametrize("case", sorted(TABLE_CASES))
def test_table_entry_points_report_as_before(case):
    keep = []

    def layers(Kpad, Cout):   # W, scale, shift, Kpad, Cout, relu
        n = len(Cout)
        keep.extend([D.host_ptrs([DEV] * n), D.host_ptrs([DEV] * n), D.host_ptrs([DEV] * n), D.host_ints(Kpad), D.host_ints(Cout), D.host_ints([1] * n)])
        return [ctypes.cast(a, ctypes.c_void_p) for a in keep[-6:]]

    name, args = TABLE_CASES[case]
    rc = getattr(_lib.lib(), name)(*args(layers))
    assert (rc, _lib.lib().g4d_last_error().decode()) == (EINVAL, TABLE_EXPECTED[case])


def test_short_block_without_a_whole_tap_layer_is_accepted():
    """An older caller's block may end anywhere.  One that ends INSIDE tap_layer (two of its four bytes) is accepted, and the half-copied field
    reads as -1 ("no tap") instead of as its two low bytes; tap_out, which lies beyond such a block, reads as NULL either way."""
    a = D.block(call("stack_f32", rows=0))
    a.tap_layer = 0x00020002   # the low half alone would read as layer 2
    a.tap_out = DEV            # beyond the short block: not seen
    a.size = _lib.MlpArgs.tap_layer.offset + 2
    assert _lib.lib().g4d_mlp_run(_lib.MLP_STACK_F32, ctypes.addressof(a), None) == 0
    a.rows, a.K0 = 64, 40      # ... and the launch is checked like any other
    assert _lib.lib().g4d_mlp_run(_lib.MLP_STACK_F32, ctypes.addressof(a), None) == EINVAL
    assert _lib.lib().g4d_last_error().decode() == "g4d_mlp_stack_f32: Kpad[0] < K0"
    a.size = 12
    assert _lib.lib().g4d_mlp_run(_lib.MLP_STACK_F32, ctypes.addressof(a), None) == EINVAL and b"bytes" in _lib.lib().g4d_last_error()
    a = D.block(call("stack_f32"))
    assert _lib.lib().g4d_mlp_run(17, ctypes.addressof(a), None) == EINVAL
    assert _lib.lib().g4d_last_error().decode() == "g4d_mlp_run: unknown kernel family 17"


def test_layer_arrays_point_at_the_layers():
    """fused.layer_arrays: the six host arrays of the entry points hold the layers' pointers and sizes, in order, and outlive their construction."""
    import gc
    import torch
    from garment4d_amd import fused
    torch.manual_seed(0)
    layers = [fused.PackedLayer(torch.randn(co, k), torch.ones(co), torch.zeros(co), relu=r) for k, co, r in ((13, 32, True), (32, 48, True), (48, 7, False))]
    for weight in ("Wf", "Wf16", "Wc16"):
        arrays = fused.layer_arrays(layers, weight)
        gc.collect()
        assert all(isinstance(a, ctypes.c_void_p) for a in arrays) and len(arrays) == 6
        W, scale, shift = (ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p))[:3] for a in arrays[:3])
        Kpad, Cout, relu = (ctypes.cast(a, ctypes.POINTER(ctypes.c_int))[:3] for a in arrays[3:])
        assert W == [getattr(L, weight).data_ptr() for L in layers]
        assert scale == [L.scale.data_ptr() for L in layers] and shift == [L.shift.data_ptr() for L in layers]
        assert (Kpad, Cout, relu) == ([32, 32, 64], [32, 48, 7], [1, 1, 0])

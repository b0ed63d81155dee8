"""The training-mode shared MLP on HIP (opt-in Tuning.mlp_autograd): the five kernels of csrc/bn_train.hip against the float64 twin
(tests/mlp_train_twin.py) within the twin's derived bounds; then blocks and whole SA / FP modules, flag on against flag off (torch /
MIOpen, the route every grad-enabled call took before) on the same inputs and the same float64 replay (tests/test_backward_gpu.py's
_step / oracle.autograd_twin.Replay).

Module-level criterion, per quantity (outputs, every parameter gradient, running statistics, input gradients; errors relative to
max|reference|):  e_on <= max(3 e_off, derived)  with e_off the flag-off route's error in the same test -- 3 is the project's convention for
two fp32 routes that differ only in summation order -- and `derived` a floor for the cases where torch happens to be almost exact:
2^-24 x (the contraction depths of the stack, sum of Cin, + 32 roundings per layer of BatchNorm / activation arithmetic + the statistics'
reduction depth), times the number of layers a gradient passes through for gradients.  The measured values are printed as BACKWARD_MEASURED lines."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from garment4d_amd import _lib, fused, grad_ops, mlp_train, tuning
from garment4d_amd import pointnet2_modules as PM
from garment4d_amd import pointnet2_utils as PU
from garment4d_amd import pytorch_utils as PT
from garment4d_amd import synthetic as syn
from garment4d_amd.encoder import seed_encoder
from oracle import autograd_twin as AT

import mlp_train_twin as TW

pytestmark = pytest.mark.gpu

EPS = 1e-5
# every slice boundary of the statistics / reduce kernels: the minimum slice (64 rows: 63 / 64 / 65 and the second boundary 127 / 128 / 129)
# and the row count from which slices grow (64 * 1024: one below, at, above -- 65537 rows are cut into slices of 72)
ROWS = [2, 3, 63, 64, 65, 127, 128, 129, 257, 4099]
ROWS_BIG = [65535, 65536, 65537]
CS = [1, 3, 4, 13, 64, 67, 128]
SHAPES = [(r, c) for r in ROWS for c in CS] + [(r, c) for r in ROWS_BIG for c in (3, 4)]


def on():
    return tuning.use(tuning.current().replace(mlp_autograd=True))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


JUNK = 7.5e8


def window(a, wide):
    """The fp32 matrix `a` (rows, c) on the device as (tensor, ld): dense, or -- wide -- the column window [3, 3 + c) of a buffer of c + 5
    columns (a base pointer that is only 4-byte aligned, rows an odd number of floats apart) whose other columns hold junk."""
    rows, c = a.shape
    if not wide:
        return dev(a), c
    buf = torch.full((rows, c + 5), JUNK, dtype=torch.float32, device="cuda")
    buf[:, 3:3 + c] = dev(a)
    return buf[:, 3:], c + 5


def _inputs(rows, c, seed):
    rng = np.random.default_rng(seed)
    Y = (rng.standard_normal((rows, c)) * rng.uniform(0.5, 2.0, c) + rng.standard_normal(c)).astype(np.float32)
    d = rng.standard_normal((rows, c)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = (rng.standard_normal(c) * 0.3).astype(np.float32)
    mean, var, _, _ = TW.stats(Y)
    return Y, d, gamma, beta, mean.astype(np.float32), var.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("rows,c", SHAPES)
def test_bn_stats_vs_twin(rows, c):
    Y = _inputs(rows, c, rows * 131 + c)[0]
    mean, var, b_mean, b_var = TW.stats(Y)
    for wide in (False, True):
        y, ld = window(Y, wide)
        m1, v1 = grad_ops.bn_stats(rows, c, y, ld)
        m2, v2 = grad_ops.bn_stats(rows, c, y, ld)
        assert torch.equal(m1, m2) and torch.equal(v1, v2), "two runs differ"
        em, ev = np.abs(host(m1) - mean), np.abs(host(v1) - var)
        assert (em <= b_mean).all(), (rows, c, wide, (em / b_mean).max())
        assert (ev <= b_var).all(), (rows, c, wide, (ev / b_var).max())
        assert (host(v1) >= 0).all()


@pytest.mark.parametrize("rows", [65, 4099])
def test_bn_stats_offset_and_constant_columns(rows):
    """Column 0: mean 1e3, deviation 0.1 -- held to the same bound as every other column, which E[y^2] - mean^2 misses
    (tests/test_mlp_train_cpu.py shows by how much).  Column 1: the constant 0.75 -- every partial sum exact, so mean 0.75 and variance 0
    exactly.  Column 2: the constant 0.1 -- variance within the bound (at most the square of the mean's rounding).  out = beta on both constant
    columns and every gradient is finite."""
    rng = np.random.default_rng(rows)
    Y = rng.standard_normal((rows, 4)).astype(np.float32)
    Y[:, 0] = (1e3 + 0.1 * rng.standard_normal(rows)).astype(np.float32)
    Y[:, 1] = 0.75
    Y[:, 2] = np.float32(0.1)
    mean, var, b_mean, b_var = TW.stats(Y)
    y = dev(Y)
    m, v = grad_ops.bn_stats(rows, 4, y, 4)
    assert (np.abs(host(m) - mean) <= b_mean).all() and (np.abs(host(v) - var) <= b_var).all(), (host(m), host(v), var, b_var)
    assert b_var[0] < 0.1 * var[0]                                    # the bound is a real one: E[y^2] - mean^2 carries 2^-24 * 1e6 = 6 x the variance
    assert host(m)[1] == 0.75 and host(v)[1] == 0.0
    beta = dev(np.array([0.1, -0.2, 0.3, 0.4], np.float32))
    out = grad_ops.bn_act(rows, 4, y, 4, m, v, EPS, None, beta, False)
    assert (host(out)[:, 1] == np.float32(-0.2)).all()
    assert np.abs(host(out)[:, 2] - np.float32(0.3)).max() <= 1.01 * b_mean[2] / np.sqrt(EPS) + 2 * TW.U      # |y - mean^| <= b_mean, invstd <= 1 / sqrt(eps)
    d = dev(rng.standard_normal((rows, 4)).astype(np.float32))
    dg, db = grad_ops.bn_act_grad_reduce(rows, 4, d, 4, y, 4, m, v, EPS, None, beta, True)
    dy = grad_ops.bn_act_grad(rows, 4, d, 4, y, 4, m, v, EPS, None, beta, True, True, dg, db)
    assert torch.isfinite(dg).all() and torch.isfinite(db).all() and torch.isfinite(dy).all()


@pytest.mark.parametrize("rows,c", SHAPES)
def test_bn_act_vs_twin(rows, c):
    Y, _, gamma, beta, mean, var = _inputs(rows, c, rows * 17 + c)
    for relu in (False, True):
        for affine in (False, True):
            g, b = (gamma, beta) if affine else (None, None)
            want, _, _, b_z, flagged = TW.act(Y, mean, var, EPS, g, b, relu)
            assert flagged.mean() < 0.01
            for wide in (False, True):
                y, ld = window(Y, wide)
                out = torch.full((rows, ld), JUNK, dtype=torch.float32, device="cuda")
                ov = out[:, 3:] if wide else out
                grad_ops.bn_act(rows, c, y, ld, dev(mean), dev(var), EPS, None if g is None else dev(g), None if b is None else dev(b), relu, out=ov, ldo=ld)
                got = host(out)[:, 3:3 + c] if wide else host(out)
                err = np.abs(got - want)
                assert (err <= np.where(flagged, 2 * b_z, b_z)).all(), (rows, c, relu, affine, wide, (err / b_z).max())
                if wide:                                  # nothing outside the window is written
                    rest = np.delete(host(out), np.s_[3:3 + c], axis=1)
                    assert (rest == np.float32(JUNK)).all()


@pytest.mark.parametrize("rows,c", SHAPES)
def test_bn_act_grad_reduce_vs_twin(rows, c):
    Y, d, gamma, beta, mean, var = _inputs(rows, c, rows * 29 + c)
    for relu in (False, True):
        for affine in (False, True):
            g, b = (gamma, beta) if affine else (None, None)
            dg, db, b_dg, b_db, flagged = TW.grad_reduce(d, Y, mean, var, EPS, g, b, relu)
            assert flagged.mean() < 0.01
            for wide in (False, True):
                y, ldy = window(Y, wide)
                dd, ldg = window(d, wide)
                args = (rows, c, dd, ldg, y, ldy, dev(mean), dev(var), EPS, None if g is None else dev(g), None if b is None else dev(b), relu)
                a1, b1 = grad_ops.bn_act_grad_reduce(*args)
                a2, b2 = grad_ops.bn_act_grad_reduce(*args)
                assert torch.equal(a1, a2) and torch.equal(b1, b2), "two runs differ"
                eg, eb = np.abs(host(a1) - dg), np.abs(host(b1) - db)
                assert (eg <= b_dg).all(), (rows, c, relu, affine, wide, (eg / np.maximum(b_dg, 1e-300)).max())
                assert (eb <= b_db).all(), (rows, c, relu, affine, wide, (eb / np.maximum(b_db, 1e-300)).max())


@pytest.mark.parametrize("rows,c", SHAPES)
def test_bn_act_grad_vs_twin(rows, c):
    Y, d, gamma, beta, mean, var = _inputs(rows, c, rows * 43 + c)
    for batch_stats in (True, False):
        for relu in (False, True):
            for affine in (False, True):
                g, b = (gamma, beta) if affine else (None, None)
                dg64, db64, _, _, _ = TW.grad_reduce(d, Y, mean, var, EPS, g, b, relu)
                dg, db = dg64.astype(np.float32), db64.astype(np.float32)          # the kernel's inputs, the same for the twin
                want, bound, flagged = TW.grad(d, Y, mean, var, EPS, g, b, relu, batch_stats, dg, db)
                assert flagged.mean() < 0.01
                for wide in (False, True):
                    y, ldy = window(Y, wide)
                    dd, ldg = window(d, wide)
                    args = (rows, c, dd, ldg, y, ldy, dev(mean), dev(var), EPS, None if g is None else dev(g), None if b is None else dev(b), relu,
                            batch_stats, dev(dg) if batch_stats else None, dev(db) if batch_stats else None)
                    g1 = grad_ops.bn_act_grad(*args)
                    assert torch.equal(g1, grad_ops.bn_act_grad(*args)), "two runs differ"
                    err = np.abs(host(g1) - want)
                    ok = (err <= bound) | flagged
                    assert ok.all(), (rows, c, batch_stats, relu, affine, wide, (err / np.maximum(bound, 1e-300))[~flagged].max())


def test_mask_of_the_backward_is_the_forwards_bit_for_bit():
    """Pre-activations AT rounding distance from 0 (y = mean + k ulps): wherever the forward wrote 0 the backward passes no gradient, wherever it
    wrote a positive value it passes dOut -- the twin flags these entries, the two kernels must simply agree with each other."""
    rows, c = 513, 8
    rng = np.random.default_rng(1)
    mean = rng.standard_normal(c).astype(np.float32)
    var = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = (1e-7 * rng.standard_normal(c)).astype(np.float32)
    Y = mean[None, :] + (rng.integers(-3, 4, size=(rows, c)) * np.spacing(np.abs(mean))[None, :]).astype(np.float32)
    Y = Y.astype(np.float32)
    y, m, v, bt = dev(Y), dev(mean), dev(var), dev(beta)
    out = grad_ops.bn_act(rows, c, y, c, m, v, EPS, None, bt, True)
    d = torch.ones((rows, c), device="cuda")
    dy = grad_ops.bn_act_grad(rows, c, d, c, y, c, m, v, EPS, None, bt, True, False)
    assert torch.equal(dy != 0, out > 0)
    _, db = grad_ops.bn_act_grad_reduce(rows, c, d, c, y, c, m, v, EPS, None, bt, True)
    assert torch.equal(db, (out > 0).sum(dim=0).float())               # counts below 2^24: exact in any order
    assert 0 < int((out > 0).sum()) < rows * c


@pytest.mark.parametrize("S", [1, 2, 8, 16, 33])
def test_pool_rows_max_grad_first_maximum(S):
    """Element for element against the twin: exact ties between duplicated rows (a ball query pads a neighbourhood with copies of its first
    hit) and between rows clamped to 0 by the ReLU; dense and windowed X / dPooled; and the forward pool's value is X at the chosen row."""
    for c in CS:
        for groups in (1, 67):
            rng = np.random.default_rng(S * 1000 + c * 10 + groups)
            X = np.maximum(rng.standard_normal((groups, S, c)), 0).astype(np.float32)         # about half the entries tie at 0
            for g in range(groups):
                if S > 1:
                    X[g, rng.integers(1, S):] = X[g, 0]                                           # the tail repeats row 0
            X = X.reshape(groups * S, c)
            dP = rng.standard_normal((groups, c)).astype(np.float32)
            want = TW.pool_max_grad(X, dP, S)
            for wide in (False, True):
                x, ldx = window(X, wide)
                dp, ldp, col0 = dev(dP), c, 0
                if wide:                                  # the cotangent as the column window [3, 3 + c) of a wider (concatenated) buffer
                    dp, ldp, col0 = torch.full((groups, c + 5), JUNK, dtype=torch.float32, device="cuda"), c + 5, 3
                    dp[:, 3:3 + c] = dev(dP)
                got = grad_ops.pool_rows_max_grad(groups, S, c, x, ldx, dp, ldp, col0)
                assert torch.equal(got, grad_ops.pool_rows_max_grad(groups, S, c, x, ldx, dp, ldp, col0))
                assert np.array_equal(host(got), want), (S, c, groups, wide, int((host(got) != want).sum()))
            pooled = mlp_train.pool_rows_max([dev(X)], [S])
            assert np.array_equal(host(pooled), X.reshape(groups, S, c).max(axis=1))


def test_zero_sizes():
    z = torch.empty((0, 5), device="cuda")
    m, v = grad_ops.bn_stats(0, 5, z, 5)
    assert host(m).tolist() == [0.0] * 5 and host(v).tolist() == [0.0] * 5
    dg, db = grad_ops.bn_act_grad_reduce(0, 5, z, 5, z, 5, m, v, EPS, None, None, True)
    assert host(dg).tolist() == [0.0] * 5 and host(db).tolist() == [0.0] * 5
    assert grad_ops.bn_act(0, 5, z, 5, m, v, EPS, None, None, True).shape == (0, 5)
    assert grad_ops.bn_act_grad(0, 5, z, 5, z, 5, m, v, EPS, None, None, True, True, dg, db).shape == (0, 5)
    assert grad_ops.pool_rows_max_grad(0, 4, 5, z, 5, z, 5).shape == (0, 5)
    e = torch.empty((7, 0), device="cuda")
    assert grad_ops.bn_stats(7, 0, e, 0)[0].shape == (0,)
    assert grad_ops.pool_rows_max_grad(7, 1, 0, e, 0, e, 0).shape == (7, 0)


# -------------------------------------------------------------------------------------------------------------- blocks and modules
def _rel(got, ref):
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((g - r).abs().max().item() / max(r.abs().max().item(), 1e-300)) if r.numel() else 0.0


def _measure(model, twin, outs, refs, gx, cx):
    m = {"out": max(_rel(o, r) for o, r in zip(outs, refs)), "bn": 0.0, "input": 0.0}
    for (name, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if q.grad is not None:
            m["grad:" + name] = _rel(p.grad, q.grad)
    for (name, b), (_, c) in zip(model.named_buffers(), twin.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(c), (name, int(b), int(c))
        else:
            m["bn"] = max(m["bn"], _rel(b, c))
    for a, c in zip(gx, cx):
        if a is not None:
            assert (a.grad is None) == (c.grad is None)
            if a.grad is not None:
                m["input"] = max(m["input"], _rel(a.grad, c.grad))
    return m


def _step(monkeypatch, model, call, inputs, seed):
    """One forward + backward on the GPU (fp32, the model's mode) and on the float64 CPU twin replaying its discrete ops (the scheme of
    tests/test_backward_gpu.py).  inputs: numpy fp32 arrays (each a leaf requiring grad) or None; the loss is a fixed random weighting."""
    twin = AT.Replay.twin(model)
    model = model.cuda()
    rp = AT.Replay(monkeypatch, PU)
    gx = [None if a is None else dev(a).requires_grad_(True) for a in inputs]
    cx = [None if a is None else torch.from_numpy(a).double().requires_grad_(True) for a in inputs]
    with rp.recording():
        outs = call(model, *gx)
    g = torch.Generator().manual_seed(seed)
    Ws = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    sum((o * W.cuda().float()).sum() for o, W in zip(outs, Ws)).backward()
    with rp.replaying():
        refs = call(twin, *cx)
    sum((o * W).sum() for o, W in zip(refs, Ws)).backward()
    return model, twin, outs, refs, gx, cx


def _stack_specs(model):
    """[(Cin, ...) per stack] of the model's conv blocks, in order."""
    return [m.weight.shape[1] for m in model.modules() if isinstance(m, (nn.Conv1d, nn.Conv2d))]


def _both_routes(monkeypatch, base, call, inputs, seed, rows, what):
    """The flag-off and the flag-on route on copies of `base`, each against the float64 replay; asserts e_on <= max(3 e_off, derived)."""
    r_off = _step(monkeypatch, copy.deepcopy(base), call, inputs, seed)
    with on():
        r_on = _step(monkeypatch, copy.deepcopy(base), call, inputs, seed)
    e_off, e_on = _measure(*r_off), _measure(*r_on)
    cins = _stack_specs(base)
    fwd = TW.U * (sum(cins) + 32 * len(cins) + TW.depth(rows, 64))
    derived = {k: fwd * (len(cins) if k.startswith("grad:") or k == "input" else 1) for k in e_on}
    print(f"\nBACKWARD_MEASURED {what} " + " ".join(f"{k.replace('grad:', 'd_')}=on:{e_on[k]:.2e}/off:{e_off[k]:.2e}" for k in e_on))
    for k in e_on:
        assert e_on[k] <= max(3 * e_off[k], derived[k]), (what, k, e_on[k], e_off[k], derived[k])
    return r_on, r_off


@pytest.mark.parametrize("cin,cout", [(3, 16), (67, 64), (128, 128)])
@pytest.mark.parametrize("rows", [2, 240, 4099])
def test_block_train_step_both_routes_vs_float64(monkeypatch, rows, cin, cout):
    """One Conv1d + BatchNorm1d(train) + ReLU block on (1, Cin, rows)."""
    torch.manual_seed(rows + cin)
    blk = seed_encoder(PT.Conv1d(cin, cout, bn=True), seed=cin).train()
    x = np.random.default_rng(rows * 7 + cin).standard_normal((1, cin, rows)).astype(np.float32)
    r_on, _ = _both_routes(monkeypatch, blk, lambda m, t: (m(t),), [x], seed=3, rows=rows, what=f"block rows={rows} {cin}->{cout}")
    assert int(r_on[0].bn.bn.num_batches_tracked) == 1


@pytest.mark.parametrize("feats", [False, True], ids=["xyz", "xyz+feats"])
def test_sa_module_msg_both_routes_vs_float64(monkeypatch, feats):
    torch.manual_seed(1)
    c = 6 if feats else 0
    sa = PM.PointnetSAModuleMSG(npoint=64, radii=[0.1, 0.2], nsamples=[8, 16], mlps=[[c, 16, 32], [c, 32, 32, 64]], use_xyz=True).train()
    seed_encoder(sa, seed=2)
    rng = np.random.default_rng(3)
    xyz = syn.unit_cloud(2, 512, seed=3)
    f = rng.standard_normal((2, c, 512)).astype(np.float32) if feats else None
    r_on, _ = _both_routes(monkeypatch, sa, lambda m, x, ft: (m(x, ft)[1],), [xyz, f], seed=4, rows=2 * 64 * 16, what=f"sa_msg feats={feats}")
    assert all(int(b) == 1 for n, b in r_on[0].named_buffers() if n.endswith("num_batches_tracked"))
    assert r_on[2][0].shape == (2, 96, 64)


@pytest.mark.parametrize("skip", [False, True], ids=["no-skip", "skip"])
def test_fp_module_both_routes_vs_float64(monkeypatch, skip):
    torch.manual_seed(5)
    c1, c2 = (16 if skip else 0), 32
    fp = PM.PointnetFPModule(mlp=[c2 + c1, 64, 32]).train()
    seed_encoder(fp, seed=6)
    rng = np.random.default_rng(7)
    unknown = syn.unit_cloud(2, 512, seed=7)
    known = np.ascontiguousarray(unknown[:, rng.permutation(512)[:64]])
    uf = rng.standard_normal((2, c1, 512)).astype(np.float32) if skip else None
    kf = rng.standard_normal((2, c2, 64)).astype(np.float32)
    _both_routes(monkeypatch, fp, lambda m, u, k, a, b: (m(u, k, a, b),), [unknown, known, uf, kf], seed=8, rows=1024, what=f"fp skip={skip}")


def _fp_and_inputs(seed=0):
    fp = seed_encoder(PM.PointnetFPModule(mlp=[24, 32, 16]), seed=seed).cuda().train()
    rng = np.random.default_rng(seed)
    unknown = dev(syn.unit_cloud(2, 128, seed=seed))
    known = unknown[:, :32].contiguous()
    uf = dev(rng.standard_normal((2, 8, 128)).astype(np.float32))
    kf = dev(rng.standard_normal((2, 16, 32)).astype(np.float32))
    return fp, (unknown, known, uf, kf)


def test_momentum_none_is_the_cumulative_average():
    """Two training steps of momentum = None layers: the running statistics are the plain average of the two batches' statistics, as torch's."""
    fp, args = _fp_and_inputs(1)
    for m in fp.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = None
    ref = copy.deepcopy(fp)
    args2 = tuple(a * 1.5 + 0.1 for a in args[:2]) + tuple(a * 0.5 for a in args[2:])
    for a in (args, args2):
        ref(*a)
        with on():
            fp(*a)
    for (n, b), (_, r) in zip(fp.named_buffers(), ref.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(r) == 2
        else:
            assert _rel(b, r) <= 1e-5, (n, _rel(b, r))


def test_eval_batchnorm_under_grad_reads_running_statistics_and_touches_no_buffer():
    fp, args = _fp_and_inputs(2)
    fp.eval()
    ref = copy.deepcopy(fp)
    before = {n: b.clone() for n, b in fp.named_buffers()}
    kf = args[3].clone().requires_grad_(True)
    kr = args[3].clone().requires_grad_(True)
    with on(), _lib.timed_calls() as t:
        out = fp(*args[:3], kf)
        out.square().sum().backward()
    names = [r[0] for r in t.results()]
    assert "g4d_bn_act_f32" in names and "g4d_bn_act_grad_f32" in names and "g4d_bn_stats_f32" not in names
    want = ref(*args[:3], kr)
    want.square().sum().backward()
    for n, b in fp.named_buffers():
        assert torch.equal(b, before[n]), n
    assert _rel(out, want) <= 1e-5 and _rel(kf.grad, kr.grad) <= 1e-4
    for (n, p), (_, q) in zip(fp.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad, q.grad) <= 1e-4, n


def test_one_value_per_channel_raises_in_training_mode():
    blk = PT.Conv1d(4, 8, bn=True).cuda().train()
    x = torch.randn(1, 4, 1, device="cuda")
    with on():
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            blk(x)
        blk.eval()
        assert blk(x).shape == (1, 8, 1)                 # running statistics: one value is fine


def test_no_grad_train_mode_takes_the_route_and_updates_the_buffers():
    """The route's other condition: grad disabled but a BatchNorm in train() (BN recalibration)."""
    blk = seed_encoder(PT.Conv1d(4, 8, bn=True), seed=3).cuda().train()
    ref = copy.deepcopy(blk)
    x = torch.randn(2, 4, 50, device="cuda")
    with torch.no_grad():
        want = ref(x)
        with _lib.timed_calls() as t, on():
            got = blk(x)
    assert "g4d_bn_stats_f32" in [r[0] for r in t.results()]
    assert _rel(got, want) <= 1e-5 and _rel(blk.bn.bn.running_var, ref.bn.bn.running_var) <= 1e-5
    assert int(blk.bn.bn.num_batches_tracked) == 1


def test_packs_follow_adam_and_ten_steps_lower_a_fixed_loss():
    fp, args = _fp_and_inputs(4)
    target = torch.randn(2, 16, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    opt = torch.optim.Adam(fp.parameters(), lr=1e-2)
    conv = fp.mlp[1].conv                                  # the second layer: its input needs a gradient, so both packs exist
    losses, keys = [], []
    with on():
        for _ in range(10):
            opt.zero_grad()
            loss = (fp(*args) - target).square().mean()
            loss.backward()
            slots = getattr(conv, "_g4d_cache")
            keys.append((slots["mlp_train_fwd"][0], slots["mlp_train_t"][0]))
            L, Lt = slots["mlp_train_fwd"][1], slots["mlp_train_t"][1]
            w = conv.weight.detach().reshape(conv.weight.shape[0], -1)
            assert torch.equal(L.W[:L.Cout, :L.K], w) and torch.equal(Lt.W[:Lt.Cout, :Lt.K], w.t())    # the packs of THIS step's weight
            opt.step()
            losses.append(loss.item())
    assert all(a != b for a, b in zip(keys, keys[1:])), "a pack survived an optimizer step"
    assert losses[-1] < losses[0], losses


def test_flag_off_is_the_torch_route_bit_for_bit(monkeypatch):
    """Flag off: the HIP training route is never entered and every output, gradient and buffer equals the plain torch layers'."""
    def boom(*a, **k):
        raise AssertionError("the HIP training route ran with the flag off")
    monkeypatch.setattr(mlp_train, "run_blocks", boom)
    assert not tuning.current().mlp_autograd
    torch.manual_seed(0)
    mlp = seed_encoder(PT.SharedMLP([6, 8, 8], bn=True), seed=1).cuda().train()
    ref = copy.deepcopy(mlp)
    x = torch.randn(2, 6, 15, 4, device="cuda", requires_grad=True)
    xr = x.detach().clone().requires_grad_(True)
    out, want = mlp(x), nn.Sequential.forward(ref, xr)
    out.square().sum().backward()
    want.square().sum().backward()
    assert torch.equal(out, want) and torch.equal(x.grad, xr.grad)
    for (n, p), (_, q) in zip(mlp.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, b), (_, c) in zip(mlp.named_buffers(), ref.named_buffers()):
        assert torch.equal(b, c), n
    # and the SA / FP modules and Conv1d make no HIP-training call either
    fp, args = _fp_and_inputs(5)
    fp(*args).sum().backward()
    sa = PM.PointnetSAModuleMSG(npoint=16, radii=[0.2], nsamples=[8], mlps=[[0, 8]], use_xyz=True).cuda().train()
    sa(args[0])[1].sum().backward()
    PT.Conv1d(4, 8, bn=True).cuda().train()(torch.randn(2, 4, 9, device="cuda")).sum().backward()


def test_flag_on_route_is_taken_and_other_stacks_fall_back():
    """With the flag on the SA level launches the new kernels (and no torch BatchNorm); bf16 precision, avg_pool and instance norm keep torch."""
    sa = seed_encoder(PM.PointnetSAModuleMSG(npoint=16, radii=[0.2], nsamples=[8], mlps=[[0, 8]], use_xyz=True), seed=1).cuda().train()
    xyz = dev(syn.unit_cloud(2, 128, seed=1))
    with on():
        with _lib.timed_calls() as t:
            out = sa(xyz)[1]
            out.sum().backward()
        names = [r[0] for r in t.results()]
        for k in ("g4d_bn_stats_f32", "g4d_bn_act_f32", "g4d_pool_rows_f32", "g4d_pool_rows_max_grad_f32", "g4d_bn_act_grad_reduce_f32",
                  "g4d_bn_act_grad_f32", "g4d_gemm_tn_f32"):
            assert k in names, (k, names)
        assert "ToChannels" in type(out.grad_fn).__name__
        with fused.precision("bf16"), _lib.timed_calls() as t:
            sa(xyz)
        assert "g4d_bn_stats_f32" not in [r[0] for r in t.results()]
        sa.pool_method = "avg_pool"
        with _lib.timed_calls() as t:
            sa(xyz)
        assert "g4d_bn_stats_f32" in [r[0] for r in t.results()] and "g4d_pool_rows_f32" not in [r[0] for r in t.results()]   # the stack yes, the pool no
        inn = PT.SharedMLP([3, 8], bn=False, instance_norm=True).cuda().train()
        with _lib.timed_calls() as t:
            inn(torch.randn(2, 3, 9, 4, device="cuda"))
        assert "g4d_bn_act_f32" not in [r[0] for r in t.results()]

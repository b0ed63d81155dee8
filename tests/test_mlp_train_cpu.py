"""The training-mode shared MLP without a GPU: the float64 twin of csrc/bn_train.hip (tests/mlp_train_twin.py) against torch's float64
autograd, the argument checks of the five entry points, the slicing the twin's bounds assume, and the opt-in's default."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mlp_train_twin as TW

EINVAL = 10001


def _torch_block(x, W, bias, gamma, beta, eps, momentum, train, running, S, Wt):
    """Conv2d + BatchNorm2d + ReLU + max_pool2d in float64 on (B, Cin, P, S); returns what the twin's block_step returns."""
    cout, cin = W.shape
    conv = nn.Conv2d(cin, cout, 1, bias=bias is not None).double()
    bn = nn.BatchNorm2d(cout, eps=eps, momentum=momentum).double()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(W).reshape(cout, cin, 1, 1))
        if bias is not None:
            conv.bias.copy_(torch.from_numpy(bias))
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(running[0]))
        bn.running_var.copy_(torch.from_numpy(running[1]))
    bn.train(train)
    xt = torch.from_numpy(x).requires_grad_(True)
    h = F.relu(bn(conv(xt)))
    out = F.max_pool2d(h, kernel_size=[1, S]).squeeze(-1)              # (B, Cout, P)
    (out * torch.from_numpy(Wt)).sum().backward()
    return conv, bn, xt, out


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("momentum", [0.1, None], ids=["momentum", "cumulative"])
def test_twin_equals_torch_float64_autograd(train, bias, momentum):
    rng = np.random.default_rng(11)
    B, cin, cout, P, S, eps = 2, 5, 7, 6, 4, 1e-5
    x = rng.standard_normal((B, cin, P, S))
    W = rng.standard_normal((cout, cin))
    bv = rng.standard_normal(cout) if bias else None
    gamma, beta = rng.uniform(0.5, 1.5, cout), rng.standard_normal(cout) * 0.3
    running = (rng.standard_normal(cout) * 0.1, rng.uniform(0.5, 1.5, cout))
    Wt = rng.standard_normal((B, cout, P))
    # the twin takes eps through fp32, as the kernels do: torch's float64 layer is given the same value
    conv, bn, xt, out = _torch_block(x, W, bv, gamma, beta, float(np.float32(eps)), momentum, train, running, S, Wt)
    rows = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, -1)).reshape(-1, a.shape[1])     # (B, C, ...) -> (B * ..., C)
    r = TW.block_step(rows(x), W, bv, gamma, beta, eps, True, rows(Wt), train, running, pool_S=S)
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=0, atol=1e-11)
    close(r["out"], rows(out.detach().numpy()))
    close(r["dW"], conv.weight.grad.numpy().reshape(cout, cin))
    close(r["dgamma"], bn.weight.grad.numpy())
    close(r["dbeta"], bn.bias.grad.numpy())
    close(r["dX"], rows(xt.grad.numpy()))
    if bias:
        close(r["dbias"], conv.bias.grad.numpy())
    if train:
        m = 1.0 if momentum is None else momentum                 # first batch of the cumulative average: the batch statistics themselves
        close((1 - m) * running[0] + m * r["mean"], bn.running_mean.numpy())
        close((1 - m) * running[1] + m * r["var_unbiased"], bn.running_var.numpy())
        assert int(bn.num_batches_tracked) == 1
    else:
        close(running[0], bn.running_mean.numpy())
        close(running[1], bn.running_var.numpy())
        assert int(bn.num_batches_tracked) == 0


def test_twin_pieces_compose_to_the_block():
    """stats -> act -> grad_reduce -> grad, the pieces the kernel tests use one by one, give block_step's gradients."""
    rng = np.random.default_rng(5)
    R, c, eps = 37, 6, 1e-5
    Y = rng.standard_normal((R, c)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), (rng.standard_normal(c) * 0.3).astype(np.float32)
    d = rng.standard_normal((R, c)).astype(np.float32)
    mean, var, _, _ = TW.stats(Y)
    out, _, _, _, flagged = TW.act(Y, mean, var, eps, gamma, beta, True)
    dgamma, dbeta, _, _, _ = TW.grad_reduce(d, Y, mean, var, eps, gamma, beta, True)
    dY, _, _ = TW.grad(d, Y, mean, var, eps, gamma, beta, True, True, dgamma, dbeta)
    r = TW.block_step(Y, np.eye(c), None, gamma, beta, eps, True, d, True)
    for a, b in ((out, r["out"]), (dgamma, r["dgamma"]), (dbeta, r["dbeta"]), (dY, r["dX"])):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    assert not flagged.any()


def test_flagged_entries_stay_below_one_percent():
    """Pre-activations at rounding distance from 0 are flagged by the twin alone; on continuous inputs -- what the GPU tests feed -- they are
    rare: the cap the GPU tests assert, here on the same generator."""
    rng = np.random.default_rng(0)
    for R, c in ((257, 13), (4099, 64)):
        Y = rng.standard_normal((R, c)).astype(np.float32)
        Y[::7, 0] = Y[0, 0]                            # repeated values
        mean, var, _, _ = TW.stats(Y)
        beta = (rng.standard_normal(c) * 0.3).astype(np.float32)
        _, _, _, _, flagged = TW.act(Y, mean.astype(np.float32), var.astype(np.float32), 1e-5, None, beta, True)
        assert flagged.mean() < 0.01
    # and an input built to sit ON the threshold is flagged
    Y = np.zeros((4, 1), np.float32)
    _, _, _, _, flagged = TW.act(Y, np.zeros(1, np.float32), np.ones(1, np.float32), 1e-5, None, None, True)
    assert flagged.all()


def test_naive_variance_formula_misses_the_twin_bound():
    """The column the GPU test holds the statistics kernel to (mean 1e3, deviation 0.1): E[y^2] - mean^2 evaluated in fp32 misses the
    bound by orders of magnitude, the centred second pass meets it -- both emulated here in fp32 numpy."""
    rng = np.random.default_rng(3)
    Y = (1e3 + 0.1 * rng.standard_normal((4099, 1))).astype(np.float32)
    _, var, _, b_var = TW.stats(Y)
    m32 = np.float32(Y.sum(dtype=np.float32) / np.float32(len(Y)))
    naive = np.float32((Y * Y).sum(dtype=np.float32) / np.float32(len(Y))) - m32 * m32
    centred = (((Y - m32) ** 2).sum(dtype=np.float32) / np.float32(len(Y)))
    assert abs(float(naive) - var[0]) > b_var[0]
    assert abs(float(centred) - var[0]) <= b_var[0]


def test_pool_twin_first_maximum():
    X = np.array([[1, 5, 0], [3, 5, 0], [3, 2, 0], [0, 0, 0]], np.float32)          # one group of S = 4
    dP = np.array([[10, 20, 30]], np.float32)
    want = np.zeros((4, 3), np.float32)
    want[1, 0], want[0, 1], want[0, 2] = 10, 20, 30
    assert np.array_equal(TW.pool_max_grad(X, dP, 4), want)


def test_slicing_of_the_library_is_the_twins():
    from garment4d_amd import _lib
    L = _lib.lib()
    for rows in (1, 2, 63, 64, 65, 4099, 65535, 65536, 65537, 1 << 20, (1 << 31) + 5):
        assert L.g4d_bn_slice_rows(rows, 4) == TW.slice_rows(rows), rows
        assert L.g4d_bn_stats_ws_bytes(rows, 3) == TW.slices(rows) * 3 * 4
        assert L.g4d_bn_act_grad_reduce_ws_bytes(rows, 3) == TW.slices(rows) * 2 * 3 * 4
    assert L.g4d_bn_stats_ws_bytes(0, 3) == 0 and L.g4d_bn_slice_rows(-1, 3) == 0


def test_argument_checks_need_no_gpu():
    """Bad arguments return G4D_EINVAL before any launch; empty problems with nothing to write return 0."""
    from garment4d_amd import _lib
    L = _lib.lib()
    p = 64                                            # a non-null pointer value that is never dereferenced: the checks come first
    bad = [
        ("g4d_bn_stats_f32", (-1, 4, p, 4, p, p, p, 0), "negative"),
        ("g4d_bn_stats_f32", (8, 4, p, 3, p, p, p, 0), "ldy < C"),
        ("g4d_bn_stats_f32", (8, 4, 0, 4, p, p, p, 0), "null"),
        ("g4d_bn_stats_f32", (8, 4, p, 4, 0, p, p, 0), "null"),
        ("g4d_bn_stats_f32", (8, 4, p, 4, p, 0, p, 0), "null"),
        ("g4d_bn_act_f32", (8, -1, p, 4, p, p, 1e-5, 0, 0, 1, p, 4, 0), "negative"),
        ("g4d_bn_act_f32", (8, 4, p, 4, p, p, 1e-5, 0, 0, 1, p, 3, 0), "ld < C"),
        ("g4d_bn_act_f32", (8, 4, p, 4, 0, p, 1e-5, 0, 0, 1, p, 4, 0), "null"),
        ("g4d_bn_act_f32", (8, 4, p, 4, p, p, 1e-5, 0, 0, 1, 0, 4, 0), "null"),
        ("g4d_bn_act_grad_reduce_f32", (-2, 4, p, 4, p, 4, p, p, 1e-5, 0, 0, 1, p, p, p, 0), "negative"),
        ("g4d_bn_act_grad_reduce_f32", (8, 4, p, 3, p, 4, p, p, 1e-5, 0, 0, 1, p, p, p, 0), "ld < C"),
        ("g4d_bn_act_grad_reduce_f32", (8, 4, p, 4, p, 4, p, p, 1e-5, 0, 0, 1, 0, p, p, 0), "null"),
        ("g4d_bn_act_grad_reduce_f32", (8, 4, p, 4, p, 4, p, p, 1e-5, 0, 0, 1, p, 0, p, 0), "null"),
        ("g4d_bn_act_grad_f32", (8, 4, p, 4, p, 4, p, p, 1e-5, 0, 0, 1, 1, p, p, p, 3, 0), "ld < C"),
        ("g4d_bn_act_grad_f32", (8, 4, p, 4, p, 4, p, p, 1e-5, 0, 0, 1, 1, 0, p, p, 4, 0), "null"),     # batch statistics need the sums
        ("g4d_bn_act_grad_f32", (8, 4, p, 4, p, 4, p, p, 1e-5, 0, 0, 1, 0, 0, 0, 0, 4, 0), "null"),     # dY
        ("g4d_bn_act_grad_f32", (8, 4, p, -4, p, 4, p, p, 1e-5, 0, 0, 1, 0, 0, 0, p, 4, 0), "negative"),
        ("g4d_pool_rows_max_grad_f32", (4, 0, 4, p, 4, p, 4, 0, p, 0), "S >= 1"),
        ("g4d_pool_rows_max_grad_f32", (-1, 2, 4, p, 4, p, 4, 0, p, 0), "negative"),
        ("g4d_pool_rows_max_grad_f32", (4, 2, 4, p, 3, p, 4, 0, p, 0), "ld < C"),
        ("g4d_pool_rows_max_grad_f32", (4, 2, 4, p, 4, p, 6, 3, p, 0), "ld < C"),                       # the window col0 + C passes ldp
        ("g4d_pool_rows_max_grad_f32", (4, 2, 4, p, 4, 0, 4, 0, p, 0), "null"),
    ]
    for name, args, needle in bad:
        rc = getattr(L, name)(*args)
        assert rc == EINVAL, (name, args, rc)
        msg = L.g4d_last_error().decode()
        assert name in msg and needle.lower() in msg.lower(), (name, msg)
    # nothing to do, nothing dereferenced
    assert L.g4d_bn_stats_f32(8, 0, 0, 0, 0, 0, 0, 0) == 0
    assert L.g4d_bn_act_f32(0, 4, 0, 4, 0, 0, 1e-5, 0, 0, 1, 0, 4, 0) == 0
    assert L.g4d_bn_act_grad_f32(0, 4, 0, 4, 0, 4, 0, 0, 1e-5, 0, 0, 1, 1, 0, 0, 0, 4, 0) == 0
    assert L.g4d_pool_rows_max_grad_f32(0, 2, 4, 0, 4, 0, 4, 0, 0, 0) == 0
    assert L.g4d_bn_act_grad_reduce_f32(8, 0, 0, 0, 0, 0, 0, 0, 1e-5, 0, 0, 1, 0, 0, 0, 0) == 0
    assert ctypes.sizeof(ctypes.c_longlong) == 8


def test_flag_defaults_to_off_and_reads_its_variable(monkeypatch):
    from garment4d_amd import tuning
    assert tuning.Tuning().mlp_autograd is False
    monkeypatch.delenv("G4D_MLP_AUTOGRAD", raising=False)
    assert tuning.from_environment().mlp_autograd is False
    monkeypatch.setenv("G4D_MLP_AUTOGRAD", "1")
    assert tuning.from_environment().mlp_autograd is True


def test_cpu_tensors_and_other_stacks_keep_torchs_layers():
    """With the flag ON: a CPU tensor never takes the HIP route (it gives torch's result), and plain_block refuses what the kernels do not cover."""
    from garment4d_amd import mlp_train, pytorch_utils as PT, tuning
    torch.manual_seed(0)
    mlp = PT.SharedMLP([4, 8, 8], bn=True).train()
    x = torch.randn(2, 4, 5, 3)
    with tuning.use(tuning.current().replace(mlp_autograd=True)):
        assert not mlp_train.applies(mlp, x)
        a = mlp(x)
    ref = PT.SharedMLP([4, 8, 8], bn=True).train()
    ref.load_state_dict({k: v for k, v in mlp.state_dict().items()}, strict=True)
    for m in ref.modules():                          # same running statistics as `mlp` had BEFORE its step
        if isinstance(m, nn.BatchNorm2d):
            m.reset_running_stats()
    assert torch.equal(a, nn.Sequential.forward(ref, x))
    assert mlp_train.plain_stack(mlp) is not None and len(mlp_train.plain_stack(mlp)) == 2
    assert mlp_train.plain_block(PT.Conv1d(4, 8, bn=True)) is not None
    assert mlp_train.plain_block(PT.Conv1d(4, 8, activation=None)) is not None
    assert mlp_train.plain_block(PT.Conv2d(4, 8, bn=True, preact=True)) is None
    assert mlp_train.plain_block(PT.Conv2d(4, 8, instance_norm=True)) is None
    assert mlp_train.plain_block(PT.Conv2d(4, 8, activation=nn.Tanh())) is None
    assert mlp_train.plain_block(PT.Conv2d(4, 8, kernel_size=(1, 3))) is None
    assert mlp_train.plain_stack(PT.SharedMLP([4, 8], bn=True, preact=True)) is None

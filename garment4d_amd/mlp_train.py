"""The trainable shared MLP on HIP (opt-in: tuning.Tuning.mlp_autograd / G4D_MLP_AUTOGRAD): every 1x1 conv (+ BatchNorm) (+ ReLU) block of a
SharedMLP / Conv1d as ONE autograd node on point-major rows (rows = batch x points (x samples), one column per channel), and the SA level's
max-pool on the same rows.

Forward of a block:  Y = X W^T (+ conv bias)  -- fused.linear on a pack of the conv weight (scale 1, shift = bias or 0, no ReLU) cached on
the conv under the weight's version --, then the batch statistics (g4d_bn_stats_f32: mean and biased variance, two passes) or, for a
BatchNorm in eval(), its running statistics, then  out = act(gamma (Y - mean) / sqrt(var + eps) + beta)  (g4d_bn_act_f32).  Saved: X, Y,
mean, var -- neither xhat nor the ReLU mask (both are recomputed from Y by the forward's own expression).
Backward:  (dgamma, dbeta) = g4d_bn_act_grad_reduce_f32,  dY = g4d_bn_act_grad_f32,  dW = dY^T X (g4d_gemm_tn_f32, written as (Cout, Cin)),
d bias = column sums of dY (g4d_col_sum_rows_f32),  dX = dY W through the transposed pack (cached under the weight's version: rebuilt after
an optimizer step), only when the input needs it.

BatchNorm bookkeeping as nn.BatchNorm*d in training mode: num_batches_tracked += 1, running_mean / running_var moved by `momentum` (None:
cumulative average) towards the batch mean / the UNBIASED batch variance, in place under no_grad; one value per channel raises torch's
ValueError.  In eval() the running statistics are read and no buffer is touched.
"""
import torch
import torch.nn as nn

from . import _cache
from . import fused
from . import grad_ops
from .tuning import current as _T


def plain_block(block):
    """(conv, bn | None, relu) of a pytorch_utils.Conv{1,2}d block that is a 1x1 conv [+ BatchNorm] [+ ReLU], else None (pre-activation,
    instance norm, other activations, other kernel sizes: torch's layers run those)."""
    names = [n for n, _ in block.named_children()]
    conv = getattr(block, "conv", None)
    if not isinstance(conv, (nn.Conv1d, nn.Conv2d)) or not names or names[0] != "conv" or any(n not in ("conv", "bn", "activation") for n in names):
        return None
    one = (1,) * len(conv.kernel_size)
    if conv.kernel_size != one or conv.stride != one or conv.padding != (0,) * len(one) or conv.dilation != one or conv.groups != 1:
        return None
    act = getattr(block, "activation", None)
    if not (act is None or isinstance(act, nn.ReLU)):
        return None
    bn = fused._unwrap_bn(block.bn) if "bn" in names else None
    if bn is not None and not isinstance(bn, (nn.BatchNorm1d, nn.BatchNorm2d)):
        return None
    return conv, bn, act is not None


def plain_stack(stack):
    """[(conv, bn, relu)] of a SharedMLP whose blocks are all plain, else None."""
    blocks = [plain_block(b) for b in stack.children()]
    return blocks if blocks and all(b is not None for b in blocks) else None


def applies(module, *tensors):
    """Does this call of `module` (a SharedMLP, a Conv1d block, an SA level) on `tensors` (None entries skipped) take the HIP training
    route?  The flag is on, every tensor is a non-empty fp32 HIP tensor, fp32 operand precision, and grad is enabled or some BatchNorm below
    `module` is in training mode."""
    if not _T().mlp_autograd or fused.current_precision() != "fp32":
        return False
    if any(t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() > 0) for t in tensors):
        return False
    return torch.is_grad_enabled() or any(m.training for m in module.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))


def _packed_forward(conv):
    w, b = conv.weight, conv.bias
    cout = w.shape[0]
    return _cache.packed(conv, "mlp_train_fwd", [w] if b is None else [w, b], lambda: fused.PackedLayer(
        w.detach().float().reshape(cout, -1), torch.ones(cout, device=w.device),
        torch.zeros(cout, device=w.device) if b is None else b.detach().float(), relu=False), extra=str(w.device))


def _packed_transposed(conv):
    w = conv.weight
    cout, cin = w.shape[0], w.shape[1]
    return _cache.packed(conv, "mlp_train_t", [w], lambda: fused.PackedLayer(
        w.detach().float().reshape(cout, cin).t().contiguous(), torch.ones(cin, device=w.device), torch.zeros(cin, device=w.device), relu=False),
        extra=str(w.device))


def _update_running(bn, mean, var, rows):
    """nn.BatchNorm's training-mode bookkeeping (torch/nn/modules/batchnorm.py, _BatchNorm.forward), in place."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    eaf = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
    bn.running_mean.mul_(1.0 - eaf).add_(mean.to(bn.running_mean.dtype), alpha=eaf)
    bn.running_var.mul_(1.0 - eaf).add_(var.to(bn.running_var.dtype), alpha=eaf * rows / (rows - 1))


class _ConvBNActFn(torch.autograd.Function):
    """x (rows, Cin) -> act(BN(x W^T + bias)) (rows, Cout); see the module docstring."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, conv, bn, relu):
        rows, cout = x.shape[0], weight.shape[0]
        y = fused.linear(x, _packed_forward(conv))
        mean = var = None
        batch_stats = False
        eps = 0.0
        if bn is not None:
            eps = bn.eps
            batch_stats = bn.training or bn.running_mean is None
            if batch_stats:
                if rows == 1:
                    raise ValueError(f"Expected more than 1 value per channel when training, got input size {[rows, cout]}")
                mean, var = grad_ops.bn_stats(rows, cout, y, cout)
                if bn.training and bn.track_running_stats and bn.running_mean is not None:
                    _update_running(bn, mean, var, rows)
            else:
                mean, var = bn.running_mean.detach().float().contiguous(), bn.running_var.detach().float().contiguous()
        elif relu:   # conv bias + ReLU: the same kernels on the identity statistics (xhat = y exactly)
            mean, var = torch.zeros(cout, device=x.device), torch.ones(cout, device=x.device)
        if mean is None:
            out = y
        else:
            g = None if gamma is None else gamma.detach().float().contiguous()
            b = None if beta is None else beta.detach().float().contiguous()
            out = grad_ops.bn_act(rows, cout, y, cout, mean, var, eps, g, b, relu)
        ctx.conv, ctx.relu, ctx.eps, ctx.batch_stats = conv, relu, eps, batch_stats
        ctx.save_for_backward(x, weight, gamma, beta, None if mean is None else y, mean, var)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x, weight, gamma, beta, y, mean, var = ctx.saved_tensors
        rows, cin = x.shape
        cout = weight.shape[0]
        need = ctx.needs_input_grad
        dy = dout.float().contiguous()
        dgamma = dbeta = None
        if mean is not None:
            g = None if gamma is None else gamma.detach().float().contiguous()
            b = None if beta is None else beta.detach().float().contiguous()
            args = (rows, cout, dy, cout, y, cout, mean, var, ctx.eps, g, b, ctx.relu)
            if ctx.batch_stats or need[3] or need[4]:
                dgamma, dbeta = grad_ops.bn_act_grad_reduce(*args)
            if need[0] or need[1] or need[2]:
                dy = grad_ops.bn_act_grad(*args, ctx.batch_stats, dgamma, dbeta)
        dx = dw = db = None
        if need[1]:
            dw = grad_ops.gemm_tn(rows, cout, cout, cin, dy, x).reshape(weight.shape).to(weight.dtype)
        if need[2]:
            db = grad_ops.col_sum(rows, cout, dy).to(weight.dtype)
        if need[0]:
            dx = fused.linear(dy, _packed_transposed(ctx.conv))
        return (dx, dw, db, dgamma.to(gamma.dtype) if need[3] else None, dbeta.to(beta.dtype) if need[4] else None, None, None, None)


class _ToRowsFn(torch.autograd.Function):
    """(B, C, N) -> (B, N, C); the transpose kernel is its own adjoint."""

    @staticmethod
    def forward(ctx, cm):
        return fused.to_point_major(cm)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return fused.to_channel_major(g.float().contiguous())


class _ToChannelsFn(torch.autograd.Function):
    """(B, N, C) -> (B, C, N)."""

    @staticmethod
    def forward(ctx, pm):
        return fused.to_channel_major(pm)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return fused.to_point_major(g.float().contiguous())


class _PoolRowsMaxFn(torch.autograd.Function):
    """The scales of an SA level pooled into ONE buffer: x_i (groups * S_i, C_i) -> (groups, sum C_i), scale i in the column window
    [col0_i, col0_i + C_i): g4d_pool_rows_f32 forward, g4d_pool_rows_max_grad_f32 backward reading its window of the cotangent in place (the
    first maximum takes it).  No concatenation forward, no split backward."""

    @staticmethod
    def forward(ctx, Ss, *xs):
        groups = xs[0].shape[0] // Ss[0]
        out = torch.empty((groups, sum(x.shape[1] for x in xs)), dtype=torch.float32, device=xs[0].device)
        col0 = 0
        for x, S in zip(xs, Ss):
            assert x.shape[0] == groups * S
            fused._pool_rows(x, groups, S, out, col0, True)
            col0 += x.shape[1]
        ctx.Ss = Ss
        ctx.save_for_backward(*xs)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = g.float().contiguous()
        grads, col0 = [], 0
        for i, (x, S) in enumerate(zip(ctx.saved_tensors, ctx.Ss)):
            rows, c = x.shape
            grads.append(grad_ops.pool_rows_max_grad(rows // S, S, c, x, c, g, g.shape[1], col0) if ctx.needs_input_grad[1 + i] else None)
            col0 += c
        return (None, *grads)


def to_rows(cm):
    """Channel-major features (B, C, N) or (B, C, N, S) -> rows (B * N (* S), C), differentiable."""
    B, C = cm.shape[0], cm.shape[1]
    return _ToRowsFn.apply(cm.reshape(B, C, -1).contiguous()).reshape(-1, C)


def to_channels(rows2d, B):
    """Rows (B * N, C) -> channel-major (B, C, N), differentiable."""
    return _ToChannelsFn.apply(rows2d.reshape(B, -1, rows2d.shape[1]))


def run_blocks(blocks, x2d):
    """The plain blocks [(conv, bn, relu)] chained on rows."""
    h = x2d
    for conv, bn, relu in blocks:
        if h.shape[1] != conv.weight.shape[1]:
            raise RuntimeError(f"expected {conv.weight.shape[1]} input channels, got {h.shape[1]}")
        h = _ConvBNActFn.apply(h.contiguous(), conv.weight, conv.bias, None if bn is None else bn.weight, None if bn is None else bn.bias, conv, bn, relu)
    return h


def pool_rows_max(xs, Ss):
    """Row max-pool of the matrices xs[i] (groups * Ss[i], C_i) into one (groups, sum C_i) matrix, differentiable."""
    return _PoolRowsMaxFn.apply(tuple(int(S) for S in Ss), *[x.contiguous() for x in xs])


def forward_channel_major(blocks, x):
    """x (B, Cin, ...) through the blocks, returned in x's layout (B, Cout, ...)."""
    B = x.shape[0]
    out = to_channels(run_blocks(blocks, to_rows(x)), B)
    return out.reshape(B, out.shape[1], *x.shape[2:])

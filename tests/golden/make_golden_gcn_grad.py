#!/usr/bin/env python
"""Generate tests/golden/gcn_grad.npz: gradients of the REFERENCE's own `GraphConvolution` (modules/pygcn/layers.py, plain torch) from
torch's autograd on the CPU, in fp32 and from a float64 copy of the same layers.

Run from the repo root:  G4D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_gcn_grad.py
(its own process; G4D_GOLDEN_OUT=<dir> writes elsewhere, to compare).  Needs no GPU.  Only DATA is written.

What runs unmodified from the reference: modules/pygcn/layers.py (`GraphConvolution`), modules/pygcn/utils.py (`normalize`,
`sparse_mx_to_torch_sparse_tensor`); F.relu between the layers of the stack as in modules/mesh_encoder.py:477-481.

Cases (the 64-vertex quad cylinder of gcn.npz):
  * single layers, the cases of gcn.npz: GraphConvolution(12, 20) on (3, 64, 12) [`l3d`], on its first frame [`l2d`], with ismlp=True
    [`mlp`]; GraphConvolution(12, 3, bias=False) [`nb`].  Stored per case: x, W, b, dy and dx, dW, db (fp32) + dx64, dW64, db64.
  * `stack`: the regressor 323 -> 128 -> 128 -> 128 -> 3, B = 2.  Stored: x, W0..3, b0..3, dy, the fp32 gradients dx, dW0..3, db0..3 and, per
    gradient tensor, eref_<name> = max |fp32 - float64| and max64_<name> = max |float64|; min_preact = the smallest float64
    |pre-activation| over the three hidden layers.  A ReLU whose pre-activation is nearly zero can fall on either side in two correct fp32
    forwards, and one flip changes every gradient behind it by a discrete amount: the seed is the first of SEEDS whose min_preact is at
    least MIN_PREACT (asserted), so no element of the fixture is such a coin toss and the tests mask nothing.
"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = os.environ.get("G4D_REFERENCE_DIR") or sys.exit("set G4D_REFERENCE_DIR to a checkout of the reference")
OUT = os.environ.get("G4D_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")

from garment4d_amd import synthetic as syn  # noqa: E402

WIDTHS = (323, 128, 128, 128, 3)
SEEDS = range(1000, 1200)
MIN_PREACT = 2e-5   # ~4 x the worst forward error measured against the reference at the widest layer (4.7e-6, README)


def N(t):
    return t.detach().cpu().numpy().copy()


def reference_adjacency(gu):
    import scipy.sparse as sp
    _, faces = syn.quad_cylinder(8, 8)
    raw = sp.coo_matrix((np.ones(faces.shape[0] * 4), (np.concatenate([faces[:, a] for a in range(4)]),
                                                       np.concatenate([faces[:, (a + 1) % 4] for a in range(4)]))),
                        shape=(64, 64), dtype=np.float32).tocsr()
    raw = raw.maximum(raw.T)
    return gu.sparse_mx_to_torch_sparse_tensor(gu.normalize(raw + sp.eye(64)))


def layer_grads(layer, x, adj, dy, **kw):
    """(dx, dW, db) of one reference layer by autograd, in the dtype of its parameters."""
    dt = layer.weight.dtype
    xi = x.detach().to(dt).requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    y = layer(xi, adj.to(dt), **kw)
    y.backward(dy.to(dt))
    return xi.grad, layer.weight.grad, None if layer.bias is None else layer.bias.grad


def stack_run(layers, x, adj, dy):
    """Forward + backward of the regressor loop; returns the gradients [dx, dW0, db0, ...] and the hidden pre-activations."""
    dt = layers[0].weight.dtype
    xi = x.detach().to(dt).requires_grad_(True)
    for m in layers:
        for p in m.parameters():
            p.grad = None
    h, pre = xi, []
    for i, m in enumerate(layers):
        h = m(h, adj.to(dt))
        if i + 1 < len(layers):
            pre.append(h.detach())
            h = F.relu(h)
    h.backward(dy.to(dt))
    grads = {"dx": xi.grad}
    for i, m in enumerate(layers):
        grads[f"dW{i}"], grads[f"db{i}"] = m.weight.grad, m.bias.grad
    return grads, pre


def make_stack(gl, seed):
    import copy
    torch.manual_seed(seed)
    layers = [gl.GraphConvolution(WIDTHS[i], WIDTHS[i + 1]) for i in range(4)]
    layers64 = [copy.deepcopy(m).double() for m in layers]
    x = torch.randn(2, 64, WIDTHS[0])
    return layers, layers64, x


def compute():
    sys.path.insert(0, os.path.join(REF, "modules"))
    gl = importlib.import_module("pygcn.layers")
    gu = importlib.import_module("pygcn.utils")
    import copy
    adj = reference_adjacency(gu)
    out = {}
    # ---- single layers: the parameters and the input of gcn.npz (same seed, same construction order)
    torch.manual_seed(50)
    layer = gl.GraphConvolution(12, 20)
    x = torch.randn(3, 64, 12)
    layer_nb = gl.GraphConvolution(12, 3, bias=False)
    torch.manual_seed(51)
    dy20, dy3 = torch.randn(3, 64, 20), torch.randn(3, 64, 3)
    cases = {"l3d": (layer, x, dy20, {}), "l2d": (layer, x[0], dy20[0], {}), "mlp": (layer, x, dy20, {"ismlp": True}), "nb": (layer_nb, x, dy3, {})}
    for name, (m, xi, dy, kw) in cases.items():
        g32 = layer_grads(m, xi, adj, dy, **kw)
        g64 = layer_grads(copy.deepcopy(m).double(), xi, adj, dy, **kw)
        out.update({f"{name}_x": N(xi), f"{name}_W": N(m.weight), f"{name}_dy": N(dy)})
        if m.bias is not None:
            out[f"{name}_b"] = N(m.bias)
        for k, a, b in zip(("dx", "dW", "db"), g32, g64):
            if a is not None:
                assert a.dtype == torch.float32 and b.dtype == torch.float64
                out[f"{name}_{k}"], out[f"{name}_{k}64"] = N(a), N(b)
    # ---- the regressor stack: the first seed without a near-zero pre-activation
    for seed in SEEDS:
        layers, layers64, xs = make_stack(gl, seed)
        with torch.no_grad():
            h, mn = xs.double(), np.inf
            for i, m in enumerate(layers64[:-1]):
                h = m(h, adj.double())
                mn = min(mn, float(h.abs().min()))
                h = F.relu(h)
        if mn >= MIN_PREACT:
            break
    else:
        raise SystemExit("no seed of SEEDS keeps every hidden pre-activation away from zero")
    dys = torch.randn(2, 64, WIDTHS[-1])
    g32, _ = stack_run(layers, xs, adj, dys)
    g64, pre64 = stack_run(layers64, xs, adj, dys)
    min_preact = min(float(p.abs().min()) for p in pre64)
    assert min_preact >= MIN_PREACT and min_preact == mn, (min_preact, mn)
    out.update(stack_seed=np.int64(seed), stack_min_preact=np.float64(min_preact), stack_x=N(xs), stack_dy=N(dys))
    for i, m in enumerate(layers):
        out[f"stack_W{i}"], out[f"stack_b{i}"] = N(m.weight), N(m.bias)
    for k in g32:
        assert g32[k].dtype == torch.float32 and g64[k].dtype == torch.float64
        out[f"stack_{k}"] = N(g32[k])
        out[f"stack_eref_{k}"] = np.float64((g32[k].double() - g64[k]).abs().max())
        out[f"stack_max64_{k}"] = np.float64(g64[k].abs().max())
    return out


if __name__ == "__main__":
    out = compute()
    path = os.path.join(OUT, "gcn_grad.npz")
    np.savez_compressed(path, **out)
    print("gcn_grad.npz", len(out), "arrays,", os.path.getsize(path), "bytes; stack seed", int(out["stack_seed"]), "min |pre-activation|",
          float(out["stack_min_preact"]))

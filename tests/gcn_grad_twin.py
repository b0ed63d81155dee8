"""float64 twin of the GCN layer's forward and backward in dense numpy, shared by tests/test_gcn_grad_cpu.py (which ties it to the reference's
autograd through tests/golden/gcn_grad.npz) and tests/test_gcn_grad_gpu.py (which holds the HIP kernels to it).  Not a test module.

Layer: Y = act(A (X W) + b) per frame.  Backward with cotangent dY:  G = dY masked by the ReLU (pre-activation > 0),  dS = A^T G,
dW = sum over frames of X^T dS,  db = column sums of G,  dX = dS W^T."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = (323, 128, 128, 128, 3)


def load():
    return np.load(os.path.join(GOLDEN, "gcn_grad.npz")), np.load(os.path.join(GOLDEN, "gcn.npz"))


def dense_adjacency(gcn_npz, n=64):
    """The fixture's row-normalised adjacency as a dense float64 matrix (its stored fp32 values, exactly)."""
    A = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (gcn_npz["adj_row"], gcn_npz["adj_col"]), gcn_npz["adj_val"].astype(np.float64))
    return A


def layer_forward(x, W, b, A, ismlp=False, dt=np.float64):
    s = x.astype(dt) @ W.astype(dt)
    y = s if ismlp else np.einsum("vu,...uc->...vc", A.astype(dt), s)
    return y if b is None else y + b.astype(dt)


def layer_backward(x, W, A, g, ismlp=False, need_abs=False, dt=np.float64):
    """g = the masked cotangent (float64).  Returns dx, dW, db (+ dS and the sums of |term| of dS, dW, db, dX with need_abs)."""
    x, W, A, g = x.astype(dt), W.astype(dt), A.astype(dt), g.astype(dt)
    ds = g if ismlp else np.einsum("vu,...vc->...uc", A, g)
    x2, ds2, g2 = x.reshape(-1, x.shape[-1]), ds.reshape(-1, ds.shape[-1]), g.reshape(-1, g.shape[-1])
    dW, db, dx = x2.T @ ds2, g2.sum(0), ds @ W.T
    if not need_abs:
        return dx, dW, db
    a_ds = np.abs(g) if ismlp else np.einsum("vu,...vc->...uc", np.abs(A), np.abs(g))
    return dx, dW, db, ds, dict(ds=a_ds, dW=np.abs(x2).T @ np.abs(ds2), db=np.abs(g2).sum(0), dx=np.abs(ds) @ np.abs(W).T)


def stack_grads(x, Ws, bs, A, dy, need_abs=False, dt=np.float64):
    """The regressor loop (ReLU after every layer but the last) forward + backward in float64 (or `dt`: np.longdouble where float64's own
    rounding matters).  Returns {dx, dW_i, db_i}, the hidden pre-activations, and with need_abs per tensor the sum |term| of the LAST step
    that produced it (that step's inputs taken as exact)."""
    hs, pres = [x.astype(dt)], []
    for i, (W, b) in enumerate(zip(Ws, bs)):
        y = layer_forward(hs[-1], W, b, A, dt=dt)
        if i + 1 < len(Ws):
            pres.append(y)
            y = np.maximum(y, 0.0)
        hs.append(y)
    grads, absb = {}, {}
    g = dy.astype(dt)
    for i in reversed(range(len(Ws))):
        if i + 1 < len(Ws):
            g = g * (pres[i] > 0)
        dx, dW, db, _, ab = layer_backward(hs[i], Ws[i], A, g, need_abs=True, dt=dt)
        grads[f"dW{i}"], grads[f"db{i}"] = dW, db
        absb[f"dW{i}"], absb[f"db{i}"] = ab["dW"], ab["db"]
        g = dx
    grads["dx"], absb["dx"] = g, ab["dx"]
    return (grads, pres, absb) if need_abs else (grads, pres)


def sum_bound(k, abs_sum):
    """First-order bound of a k-term fp32 sum of exactly known terms' products in any order: (k + 2) 2^-24 sum |term|."""
    return (k + 2) * 2.0 ** -24 * abs_sum

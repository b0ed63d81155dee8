"""Float64 autograd twin of the pointnet2 ops -- TEST INFRASTRUCTURE ONLY (never imported by garment4d_amd/).

Three faces:
  * grouping_operation / gather_operation / three_interpolate as float64 torch functions built on torch.gather, so autograd
    differentiates them natively (their backward is torch's own scatter-add in float64).  `weight` of three_interpolate gets no
    gradient, as in the product (pointnet2_utils.ThreeInterpolate.backward).
  * scatter_add_exact(): the backward of those ops as an explicit float64 scatter-add that also returns, per output element, the
    number of contributions k and sum |term| -- what an error bound for an fp32 atomic sum in any order needs.
  * Replay: records the DISCRETE outputs of a HIP forward (FPS indices, ball-query indices, three_nn indices and distances) and
    feeds them to a float64 CPU copy of the same module, with the continuous ops swapped for the ones above.  The modules look the
    ops up through the `pointnet2_utils` module at call time, so patching its attributes is enough.
"""
import copy

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------------------------- ops
def grouping_operation(features, idx):
    """features (B,C,N), idx (B,P,S) int -> (B,C,P,S): out[b,c,p,s] = features[b,c,idx[b,p,s]]."""
    B, C, _ = features.shape
    _, P, S = idx.shape
    ix = idx.to(device=features.device, dtype=torch.int64).reshape(B, 1, P * S).expand(B, C, P * S)
    return torch.gather(features, 2, ix).reshape(B, C, P, S)


def gather_operation(features, idx):
    """features (B,C,N), idx (B,M) int -> (B,C,M)."""
    return grouping_operation(features, idx.unsqueeze(-1)).squeeze(-1)


def three_interpolate(features, idx, weight):
    """features (B,C,m), idx (B,n,3), weight (B,n,3) -> (B,C,n) = w0 f[i0] + w1 f[i1] + w2 f[i2]; no gradient w.r.t. weight."""
    g = grouping_operation(features, idx)                              # (B,C,n,3)
    w = weight.detach().to(device=features.device, dtype=features.dtype).unsqueeze(1)
    return g[..., 0] * w[..., 0] + g[..., 1] * w[..., 1] + g[..., 2] * w[..., 2]


# ------------------------------------------------------------------------------------------------------------- exact scatter-add
def scatter_add_exact(grad_out, idx, n, weight=None):
    """grad[b,c,k] = sum over e with idx[b,e] == k of grad_out[b,c,e] * weight[b,e] (weight 1 when None), in float64.

    grad_out (B,C,E), idx (B,E) in [0, n), weight (B,E) or None (all numpy).  Returns (sum (B,C,n) float64, k (B,n) int64 -- the
    number of contributions, the same for every channel --, abs_sum (B,C,n) float64 = sum |term|).  Each term is formed as the
    float64 product of the two fp32 inputs, i.e. exactly.
    For group_grad E = P*S and idx is the flattened (B,P,S) index; for three_interpolate_grad E = 3n', idx the flattened (B,n',3)
    index and weight the matching flattened weights, grad_out repeated over the 3 slots."""
    g = np.asarray(grad_out, dtype=np.float64)
    B, C, E = g.shape
    ix = np.asarray(idx, dtype=np.int64).reshape(B, E)
    assert ix.size == 0 or (ix.min() >= 0 and ix.max() < n), "index out of range"
    terms = g if weight is None else g * np.asarray(weight, dtype=np.float64).reshape(B, 1, E)
    flat = (np.arange(B * C, dtype=np.int64).reshape(B, C, 1) * n + ix[:, None, :]).reshape(-1)
    s = np.bincount(flat, weights=terms.reshape(-1), minlength=B * C * n).reshape(B, C, n)
    a = np.bincount(flat, weights=np.abs(terms).reshape(-1), minlength=B * C * n).reshape(B, C, n)
    k = np.stack([np.bincount(ix[b], minlength=n) for b in range(B)]) if B else np.zeros((0, n), np.int64)
    return s, k.astype(np.int64), a


def group_grad_exact(grad_out, idx, n):
    """grouping_operation backward: grad_out (B,C,P,S), idx (B,P,S) -> (sum, k, abs_sum) as scatter_add_exact."""
    B, C = grad_out.shape[:2]
    return scatter_add_exact(np.asarray(grad_out).reshape(B, C, -1), np.asarray(idx).reshape(B, -1), n)


def gather_grad_exact(grad_out, idx, n):
    """gather_operation backward: grad_out (B,C,M), idx (B,M)."""
    return scatter_add_exact(grad_out, idx, n)


def three_interpolate_grad_exact(grad_out, idx, weight, m):
    """three_interpolate backward: grad_out (B,C,n), idx/weight (B,n,3) -> (sum (B,C,m), k (B,m), abs_sum (B,C,m))."""
    g = np.asarray(grad_out)
    B, C, n = g.shape
    g3 = np.repeat(g[..., None], 3, axis=-1).reshape(B, C, 3 * n)
    return scatter_add_exact(g3, np.asarray(idx).reshape(B, 3 * n), m, np.asarray(weight).reshape(B, 3 * n))


def atomic_sum_bound(k, abs_sum):
    """|fp32 sum of k terms in any order (each term one fp32 product) - exact sum| <= (k + 2) * 2^-24 * sum |term|."""
    return (np.asarray(k, dtype=np.float64) + 2.0) * 2.0 ** -24 * abs_sum


# -------------------------------------------------------------------------------------------------------------------------- replay
_DISCRETE = ("furthest_point_sample", "ball_query", "three_nn")
_CONTINUOUS = {"gather_operation": gather_operation, "grouping_operation": grouping_operation,
               "three_interpolate": three_interpolate}


class Replay:
    """Record the discrete op outputs of a forward on the HIP path, then replay them into a float64 CPU twin of the module.

        rp = Replay(monkeypatch, pointnet2_utils)
        twin = Replay.twin(model)                  # before the HIP step: same parameters and BN statistics
        with rp.recording():
            out = model(x_gpu)                     # HIP forward; FPS / ball-query / three_nn outputs are recorded
        with rp.replaying():
            ref = twin(x_cpu_double)               # same indices, float64 continuous ops

    `monkeypatch` is pytest's fixture (or anything with setattr(obj, name, value) and undo()); everything patched is undone when
    each block ends.  Calls are matched by order, and replay checks each op name and its argument shapes against the record."""

    def __init__(self, monkeypatch, pointnet2_utils):
        self.mp, self.pu = monkeypatch, pointnet2_utils
        self.tape = []

    @staticmethod
    def twin(model):
        return copy.deepcopy(model).double().cpu()

    def _undo(self):
        self.mp.undo()

    def recording(self):
        rp = self
        orig = {name: getattr(self.pu, name) for name in _DISCRETE}

        def rec(name):
            def f(*args):
                out = orig[name](*args)
                shapes = tuple(tuple(a.shape) for a in args if isinstance(a, torch.Tensor))
                held = tuple(o.detach().cpu() for o in out) if isinstance(out, tuple) else out.detach().cpu()
                rp.tape.append((name, shapes, held))
                return out
            return f
        return _Patched(self, {name: rec(name) for name in _DISCRETE})

    def replaying(self):
        rp = self
        pos = [0]

        def play(name):
            def f(*args):
                assert pos[0] < len(rp.tape), f"replay: more {name} calls than recorded"
                rname, shapes, held = rp.tape[pos[0]]
                pos[0] += 1
                got = tuple(tuple(a.shape) for a in args if isinstance(a, torch.Tensor))
                assert (rname, shapes) == (name, got), f"replay: recorded {rname}{shapes}, called {name}{got}"
                if name == "three_nn":
                    dist, idx = held
                    return dist.to(torch.float64), idx.clone()
                return held.clone()
            return f
        patch = {name: play(name) for name in _DISCRETE}
        patch.update(_CONTINUOUS)
        return _Patched(self, patch, done=lambda: pos[0] == len(rp.tape))


class _Patched:
    def __init__(self, rp, patch, done=None):
        self.rp, self.patch, self.done = rp, patch, done

    def __enter__(self):
        for name, fn in self.patch.items():
            self.rp.mp.setattr(self.rp.pu, name, fn)
        return self.rp

    def __exit__(self, exc_type, exc, tb):
        self.rp._undo()
        if exc_type is None and self.done is not None:
            assert self.done(), "replay: fewer calls than recorded"
        return False

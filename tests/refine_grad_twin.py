"""float64 twin of the two operators the refinement head's training route adds -- the positional encoder (csrc/pos_encode_grad.hip) and the
temporal attention (csrc/attention_grad.hip) -- in dense numpy, shared by tests/test_refine_grad_cpu.py (which ties it to the reference's own
autograd through tests/golden/refine_grad.npz) and tests/test_refine_grad_gpu.py (which holds the HIP kernels to it); the forward of the
positional encoder (csrc/pos_encode.hip) is held to pe_forward within pe_forward_bound by tests/test_pos_encode_cpu.py (the oracle) and
tests/test_pos_encode_gpu.py (the kernel and the generic route).  Not a test module.

Positional encoder, per query q with samples s and source point j_s = idx[q, s]:
    in_s = [x_j - q ; e_j]   z1_s = W1 in_s + (b1 | t_j)   h_s = relu(z1_s)   z2_s = W2 h_s   out[c] = max_s z2_s[c] + b2[c]
Backward: per channel c the cotangent goes to the first s attaining the maximum (np.argmax).

Error bounds (first order, u = 2^-24).  A value computed in fp32 as a sum of n products, each product carrying m roundings of its own,
differs from the exact value by at most (n + m) u A, whatever the order of the sum, where A is the same expression with every leaf replaced by
its absolute value.  The twin evaluates those A next to the values:
  * hA = |t| + |b1| + |W1| |in| bounds |h| and, times (KX + 3) u, its error (KX products + the bias / table additions + the rounding of the
    coordinate difference, which the kernels form first in fp32);
  * every gradient is a sum over (query, channel) pairs of terms built from go = dOut[q, c], one row of W2, the ReLU mask, h or in of the winning
    row and (for the input gradients) a 32-term product with W1: PATH = 32 + KX + 8 roundings bound the longest such term;
  * the number of terms n is the number of pairs that reach the element -- or, where the kernel documents a fixed reduction tree, the depth of
    that tree if it is smaller (`depth=` of bound()): a summation tree of depth d errs by at most d u A.
A decision (argmax, ReLU sign) is discrete and is not covered by any such bound: `flags` marks every (query, channel) whose decision could fall
either way within `margin`, and the tests zero the cotangent there on both sides."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24


def load():
    return np.load(os.path.join(GOLDEN, "refine_grad.npz"))


def pe_forward(xyz, new_xyz, extra, table, idx, W1, b1, W2, b2):
    """All float64.  xyz (F,N,3), new_xyz (F,P,3), extra (F,N,E) or None, table (F,N,32) or None, idx (F,P,S).  Returns a dict with the grouped
    input `inp` (F,P,S,KX), z1, h, z2, out, the winning sample `win` (F,P,32), hA (masked by z1 > 0: the yardstick of the gradients) and
    hA_full (unmasked: the yardstick of the forward, see pe_forward_bound)."""
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
    xyz, new_xyz, extra, table, W1, b1, W2, b2 = map(f64, (xyz, new_xyz, extra, table, W1, b1, W2, b2))
    F_, P, S = idx.shape
    fi = np.arange(F_)[:, None, None]
    ix = idx.astype(np.int64)
    inp = xyz[fi, ix] - new_xyz[:, :, None, :]
    if extra is not None and extra.shape[2]:
        inp = np.concatenate([inp, extra[fi, ix]], -1)
    add = np.zeros(32) if b1 is None else b1
    z1 = inp @ W1.T + add
    hA = np.abs(inp) @ np.abs(W1).T + np.abs(add)
    if table is not None:
        z1 = z1 + table[fi, ix]
        hA = hA + np.abs(table[fi, ix])
    h = np.maximum(z1, 0.0)
    z2 = h @ W2.T
    win = np.argmax(z2, axis=2)                                  # (F,P,32), first maximum
    out = np.take_along_axis(z2, win[:, :, None, :], 2)[:, :, 0, :] + b2
    return dict(inp=inp, z1=z1, h=h, hA=hA * (z1 > 0), hA_full=hA, z2=z2, out=out, win=win, idx=ix)


def pe_forward_bound(fw, W2, b2, table_err=None):
    """(F,P,32): first-order bound of |fp32 forward - fw["out"]|, per output element
        max over the S rows of (32 + KX + 5) u (|W2| hA_full)  +  u (|out| + |b2|),           hA_full = |t| + |b1| + |W1| |in|.
    Derivation (the rule of the module header: a sum of n products with m roundings of their own errs by at most (n + m) u A):
      * layer 1, z1 = (t | b1) + W1 in: KX products, the bias / table addition and the rounding of the coordinate difference, which every
        implementation forms first in fp32: |dz1| <= (KX + 3) u hA_full.  hA_full is NOT masked by the sign of z1: a row whose float64
        pre-activation is slightly negative may be slightly positive in fp32, and its error still counts;
      * |relu(a) - relu(b)| <= |a - b|, so h inherits the error of z1, and |h| <= hA_full;
      * layer 2, z2 = W2 h: 32 products of inexact h: |dz2| <= |W2| |dz1| + (32 + 2) u |W2| |h| <= (32 + KX + 5) u |W2| hA_full;
      * |max_s a_s - max_s b_s| <= max_s |a_s - b_s|: the pooled value errs by at most the largest row error of its query;
      * out = max + b2: one more rounding, u (|out| + |b2|) bounds it to first order.
    table_err (F,N,32), optional: the absolute error of the TABLE's entries where the fp32 table was itself computed (table_forward); it
    enters layer 1's error term per source point and is carried through |W2| like the rest.  Nothing here is a measured number."""
    W2a, b2 = np.abs(np.asarray(W2, np.float64)), np.asarray(b2, np.float64)
    hA, ix = fw["hA_full"], fw["idx"]
    kx = fw["inp"].shape[-1]
    e1 = (kx + 3) * U * hA
    if table_err is not None:
        e1 = e1 + np.asarray(table_err, np.float64)[np.arange(ix.shape[0])[:, None, None], ix]
    e2 = e1 @ W2a.T + (32 + 2) * U * (hA @ W2a.T)                  # (F,P,S,32)
    return e2.max(axis=2) + U * (np.abs(fw["out"]) + np.abs(b2))


def table_forward(feats, Wf, b1):
    """The per-source-point first-layer table t = Wf f + b1 (refine.feature_table) in float64, and the bound of an fp32 evaluation's error:
    C products plus the bias addition, (C + 2) u (|Wf| |f| + |b1|) with C the width of the Linear the table is split from (its three
    coordinate columns counted too: a looser count than the C - 3 products the table contracts, never a tighter one)."""
    feats, Wf, b1 = (np.asarray(a, np.float64) for a in (feats, Wf, b1))
    C = Wf.shape[1] + 3
    return feats @ Wf.T + b1, (C + 2) * U * (np.abs(feats) @ np.abs(Wf).T + np.abs(b1))


def pe_case(seed, F_, N, P, S, E, table, hits=None):
    """Synthetic encoder inputs.  idx: per query `hits` distinct source points (1 .. S; default uniform in 1 .. S), then copies of the first
    hit -- the shape of a ball query's output."""
    rng = np.random.default_rng(seed)
    c = dict(F=F_, N=N, P=P, S=S, E=E)
    c["xyz"] = rng.standard_normal((F_, N, 3)).astype(np.float32)
    c["new_xyz"] = rng.standard_normal((F_, P, 3)).astype(np.float32)
    c["extra"] = rng.standard_normal((F_, N, E)).astype(np.float32) if E else None
    c["table"] = (rng.standard_normal((F_, N, 32)) * 0.5).astype(np.float32) if table else None
    idx = rng.integers(0, N, (F_, P, S)).astype(np.int32)
    nh = rng.integers(1, S + 1, (F_, P)) if hits is None else np.minimum(rng.integers(1, hits + 1, (F_, P)), S)
    idx = np.where(np.arange(S)[None, None, :] < nh[..., None], idx, idx[..., :1])
    c["idx"] = idx
    c["W1"] = (rng.uniform(-1, 1, (32, 3 + E)) / np.sqrt(3 + E)).astype(np.float32)
    c["b1"] = None if table else rng.uniform(-0.3, 0.3, 32).astype(np.float32)
    c["W2"] = (rng.uniform(-1, 1, (32, 32)) / np.sqrt(32)).astype(np.float32)
    c["b2"] = rng.uniform(-0.3, 0.3, 32).astype(np.float32)
    c["dOut"] = rng.standard_normal((F_, P, 32)).astype(np.float32)
    return c


def _distinct_rows(rng, rows, cols, lo=-2, hi=2):
    """An integer matrix with entries in [lo, hi] whose rows are pairwise distinct (drawn without replacement among the base-(hi-lo+1) codes)."""
    base = hi - lo + 1
    codes = rng.choice(base ** min(cols, 12), rows, replace=False)
    m = np.stack([(codes // base ** i) % base for i in range(min(cols, 12))], 1) + lo
    if cols > 12:
        m = np.concatenate([m, rng.integers(lo, hi + 1, (rows, cols - 12))], 1)
    return m.astype(np.float32)


def pe_exact_case(seed, F_, N, P, S, E, table, hits=None):
    """pe_case with integer-valued operands small enough that every partial sum of the forward is an integer below 2^24, whatever its order:
    coordinates in [-4, 4], extras in [-3, 3], W1 / W2 entries in [-2, 2], biases and table entries in [-8, 8]
    (|z1| <= 8 + 2 (3 x 8 + 5 x 3) = 86, |z2| <= 32 x 2 x 86 = 5504).  fp32 and float64 then agree bit for bit.  W1 and W2 have pairwise distinct
    rows and columns and W2 is not symmetric, so a permuted channel, a wrong k-step or a neighbour's sample changes the result."""
    rng = np.random.default_rng(seed)
    c = pe_case(seed, F_, N, P, S, E, table, hits=hits)
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    c["xyz"], c["new_xyz"] = ints(-4, 4, (F_, N, 3)), ints(-4, 4, (F_, P, 3))
    c["extra"] = ints(-3, 3, (F_, N, E)) if E else None
    c["table"] = ints(-8, 8, (F_, N, 32)) if table else None
    c["W1"], c["W2"] = _distinct_rows(rng, 32, 3 + E), _distinct_rows(rng, 32, 32)
    c["b1"] = None if table else ints(-8, 8, 32)
    c["b2"] = ints(-8, 8, 32)
    for w in (c["W1"], c["W2"]):
        assert len({tuple(r) for r in w}) == 32 and len({tuple(r) for r in w.T}) == w.shape[1], "rows / columns must be pairwise distinct"
    assert not np.array_equal(c["W2"], c["W2"].T)
    return c


def pe_exact_expected(c):
    """The float64 output of an exact case, with the checks that make it one: every sum stays below 2^24 and the result is not degenerate
    (more than half of the entries differ from b2, i.e. the ReLU did not kill everything)."""
    fw = pe_forward(c["xyz"], c["new_xyz"], c["extra"], c["table"], c["idx"], c["W1"], c["b1"], c["W2"], c["b2"])
    assert np.abs(fw["z2"]).max() + np.abs(c["b2"]).max() < 2.0 ** 24 and (np.abs(fw["hA_full"]) @ np.abs(c["W2"]).T.astype(np.float64)).max() < 2.0 ** 24
    assert np.array_equal(fw["out"], np.rint(fw["out"]))
    assert (fw["out"] != c["b2"].astype(np.float64)).mean() > 0.5, "degenerate expected output: change the draw"
    return fw["out"]


def pe_twin(c, frames=None, table_err=None):
    """(out, bound) of a pe_case-shaped dict in float64, frame by frame so that a full-size launch fits; `frames`: only these (default all)."""
    frames = range(c["F"]) if frames is None else frames
    outs, bnds = [], []
    for f in frames:
        s = slice(f, f + 1)
        fw = pe_forward(c["xyz"][s], c["new_xyz"][s], None if c["extra"] is None else c["extra"][s], None if c["table"] is None else c["table"][s],
                        c["idx"][s], c["W1"], c["b1"], c["W2"], c["b2"])
        outs.append(fw["out"])
        bnds.append(pe_forward_bound(fw, c["W2"], c["b2"], None if table_err is None else table_err[s]))
    return np.concatenate(outs, 0), np.concatenate(bnds, 0)


def pe_flags(fw, margin):
    """(F,P,32) bool: the max-pool's top-two margin between DISTINCT source points, or the winning row's smallest |pre-activation|, is below
    `margin`.  (Copies of one source point -- ball-query padding -- tie exactly and send the gradient to the same point.)"""
    z2, win, ix, z1 = fw["z2"], fw["win"], fw["idx"], fw["z1"]
    best = np.take_along_axis(z2, win[:, :, None, :], 2)                          # (F,P,1,32)
    jwin = np.take_along_axis(ix[:, :, :, None], win[:, :, None, :], 2)           # (F,P,1,32) source point of the winner
    other = np.where(ix[:, :, :, None] != jwin, z2, -np.inf).max(2)               # best among other source points
    close = (best[:, :, 0, :] - other) < margin
    minpre = np.abs(z1).min(-1)                                                   # (F,P,S)
    relu = np.take_along_axis(minpre[:, :, :, None], win[:, :, None, :], 2)[:, :, 0, :] < margin
    return close | relu


def forward_error_bound(fw, W2):
    """max over the case of the first-order fp32 error bound of z2: (32 + KX + 3 + 2) u |W2| hA."""
    kx = fw["inp"].shape[-1]
    return float(((32 + kx + 5) * U * (np.abs(fw["hA"]) @ np.abs(np.asarray(W2, np.float64)).T)).max())


def _scatter(vals, ix, n):
    """vals (F,P,R,C) added into rows ix (F,P,R) of (F,n,C)."""
    F_, P, R, C = vals.shape
    out = np.zeros((F_, n, C))
    for f in range(F_):
        np.add.at(out[f], ix[f].reshape(-1), vals[f].reshape(-1, C))
    return out


def pe_backward(fw, W1, W2, dOut, n, n_extra, has_table):
    """dOut (F,P,32) float64 (already zeroed at flagged entries).  Returns (grads, A, cnt): the gradients, their absolute-value twins and the
    number of (query, channel) pairs that reach each element (an int, or an array for the scatter outputs)."""
    W1, W2, dOut = np.asarray(W1, np.float64), np.asarray(W2, np.float64), np.asarray(dOut, np.float64)
    inp, h, hA, z1, win, ix = fw["inp"], fw["h"], fw["hA"], fw["z1"], fw["win"], fw["idx"]
    F_, P, S, KX = inp.shape
    fi, pi = np.arange(F_)[:, None, None], np.arange(P)[None, :, None]
    hw, hAw, inw, jw = h[fi, pi, win], hA[fi, pi, win], inp[fi, pi, win], ix[fi, pi, win]   # (F,P,32c,32k) x2, (F,P,32c,KX), (F,P,32c): row of channel c
    go = dOut[:, :, :, None]                                                      # (F,P,32c,1)
    g = go * W2[None, None] * (hw > 0)                                            # (F,P,32c,32k): this pair's share of dz1 of its row
    gA = np.abs(go) * np.abs(W2)[None, None] * (hw > 0)
    G, A, cnt = {}, {}, {}
    nz = int(np.count_nonzero(dOut))
    G["dW2"], A["dW2"], cnt["dW2"] = np.einsum("fpc,fpck->ck", dOut, hw), np.einsum("fpc,fpck->ck", np.abs(dOut), hAw), F_ * P
    G["db2"], A["db2"], cnt["db2"] = dOut.sum((0, 1)), np.abs(dOut).sum((0, 1)), F_ * P
    G["dW1"], A["dW1"], cnt["dW1"] = np.einsum("fpck,fpci->ki", g, inw), np.einsum("fpck,fpci->ki", gA, np.abs(inw)), nz
    G["db1"], A["db1"], cnt["db1"] = g.sum((0, 1, 2)), gA.sum((0, 1, 2)), nz
    din, dinA = g @ W1, gA @ np.abs(W1)                                           # (F,P,32c,KX)
    G["d_new_xyz"], A["d_new_xyz"], cnt["d_new_xyz"] = -din[..., :3].sum(2), dinA[..., :3].sum(2), 32
    live = (dOut != 0).astype(np.float64)[..., None]
    G["d_xyz"], A["d_xyz"] = _scatter(din[..., :3], jw, n), _scatter(dinA[..., :3], jw, n)
    cnt["d_xyz"] = _scatter(live, jw, n)
    if n_extra:
        G["d_extra"], A["d_extra"], cnt["d_extra"] = _scatter(din[..., 3:], jw, n), _scatter(dinA[..., 3:], jw, n), cnt["d_xyz"]
    if has_table:
        G["d_table"], A["d_table"], cnt["d_table"] = _scatter(g, jw, n), _scatter(gA, jw, n), cnt["d_xyz"]
    return G, A, cnt


def bound(cnt, A, kx, depth=None):
    """(n + PATH) u A with n = cnt, or the documented depth of the kernel's reduction tree where that is smaller."""
    n = np.asarray(cnt, dtype=np.float64)
    if depth is not None:
        n = np.minimum(n, depth)
    return (n + 32 + kx + 8) * U * A


# ------------------------------------------------------------------------------------------------------------------------ temporal attention
def att_forward(qkv, T):
    """qkv (F,Vg,3C) float64 -> dict(q, k, v (clips,T,D), att (clips,T,T), out (F,Vg,C))."""
    qkv = np.asarray(qkv, np.float64)
    F_, Vg, C3 = qkv.shape
    C, n = C3 // 3, F_ // T
    q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(n, T, Vg * C) for i in range(3))
    s = q @ k.transpose(0, 2, 1) / np.sqrt(T)
    e = np.exp(s - s.max(-1, keepdims=True))
    att = e / e.sum(-1, keepdims=True)
    return dict(q=q, k=k, v=v, att=att, out=(att @ v).reshape(F_, Vg, C), C=C, Vg=Vg)


def att_backward(fw, dO, att=None):
    """dO (F,Vg,C).  att: the attention matrix to use (the kernel reads the one its forward SAVED; pass it to test the backward alone).
    Returns (dqkv (F,Vg,3C), bound (F,Vg,3C)): first-order fp32 bounds, see the module docstring: dA is a D-term sum ((D + 2) u |dO| |V|^T);
    its error and dS's own roundings carry through the T-term products."""
    q, k, v, C, Vg = fw["q"], fw["k"], fw["v"], fw["C"], fw["Vg"]
    A = fw["att"] if att is None else np.asarray(att, np.float64)
    n, T, D = q.shape
    dO = np.asarray(dO, np.float64).reshape(n, T, D)
    dA = dO @ v.transpose(0, 2, 1)
    dA_err = (D + 2) * U * (np.abs(dO) @ np.abs(v).transpose(0, 2, 1))
    r = (dA * A).sum(-1, keepdims=True)
    dS = A * (dA - r) / np.sqrt(T)
    # |d dS| <= A (|d dA| + sum_w A |d dA|) / sqrt(T) + (T + 6) u A (|dA| + sum A |dA|) / sqrt(T)
    dS_err = A * (dA_err + (A * dA_err).sum(-1, keepdims=True)) / np.sqrt(T) + (T + 6) * U * A * (np.abs(dA) + (A * np.abs(dA)).sum(-1, keepdims=True)) / np.sqrt(T)
    dQ, dK, dV = dS @ k, dS.transpose(0, 2, 1) @ q, A.transpose(0, 2, 1) @ dO
    bQ = dS_err @ np.abs(k) + (T + 2) * U * (np.abs(dS) @ np.abs(k))
    bK = dS_err.transpose(0, 2, 1) @ np.abs(q) + (T + 2) * U * (np.abs(dS).transpose(0, 2, 1) @ np.abs(q))
    bV = (T + 2) * U * (A.transpose(0, 2, 1) @ np.abs(dO))
    F_ = n * T
    cat = lambda a, b, c: np.concatenate([x.reshape(F_, Vg, C) for x in (a, b, c)], -1)
    return cat(dQ, dK, dV), cat(bQ, bK, bV)

"""float64 twin of the stage-1 objective (garment4d_amd/csrc/stage1_loss.hip; smplx/loss/temporal_loss.py:60-119 and smplx/loss/laplacian.py
in the reference) in numpy, shared by tests/test_stage1_loss_cpu.py (which ties it to the reference's own run through
tests/golden/stage1_loss.npz) and tests/test_stage1_loss_gpu.py (which holds the kernels to it).  Not a test module.

The twin evaluates the KERNEL's documented arithmetic (its file header) in float64: cotangents in the dot / cross form with one cross product
per face, (L x)_i = sum over the vertex's (face, corner) incidences of h_j (x_k - x_i) + h_k (x_j - x_i), the padding as a weight on item 0.

Error bounds (first order, u = 2^-24; the rules of stage2_loss_twin, from which U and nearest() are imported: a sum of n products with m
roundings of their own errs by at most (n + m) u A, A = the same expression over absolute values; a summation tree of depth d errs by at most
d u A).  Every product and sum of the kernel is rounded on its own:
  expf / logf                    E ulp each = 2 E u relative.  E = 2: ASSUMED, not measured -- no HIP math accuracy table ships with the ROCm
                                 installation this was written against (its documentation names 1 ulp for both).
  cross-entropy row              x - m: 1 rounding; e_k = expf(x_k - m): relative u |x_k - m| + 2 E u; s = sum e_k left to right: sum of the
                                 e_k errors + (C - 1) u s; loss = logf(s) - (x_y - m): e_s / s + 2 E u |log s| + u |x_y - m| + u |loss|
  its gradient element           scale (e_k / s - [k = y]): p_k (rel_k + e_s / s + u) + u |p_k - [k = y]|, + 2 u of the result (rounded scale, product)
                                 (an expf or a product below the smallest normal number may come out as zero: + 2^-126 absolute each)
  PCA                            d = a - b 1, d d 1: 3 u d^2; gradient c d: 3 u
  edge x_b - x_a                 1 rounding of exact inputs
  dot_k of two edges             products 3 u (two rounded operands + their own), two additions: 5 u A_k, A_k = sum_c |a_c| |b_c|
  cross component                a b - c d: 3 u each product + the subtraction: 4 u (|a b| + |c d|)
  |x| of the cross product       sum_c |x_c| e_c / |x| + 3 u |x|
  h_k = 0.5 (dot_k / |x|)        e_dot / |x| + |dot| e_|x| / |x|^2 + u |h|.  e_dot / |x| <= 5 u / sin(corner angle): the bound carries the
                                 conditioning, computed from the float64 data
  (L x)_i,c                      per term: h inexact (e_h |D|), D = x_k - x_i 1 rounding, product 1; 2 r terms in a row of r incidences, 2 r
                                 additions: sum e_h |D| + (2 r + 2) u A_c, A_c = sum |h| |D_c|; for inexact x (the pass over u) + sum |h| (e_k + e_i)
  |L x|                          sum_c of the coordinate errors + 4 u |L x|
  | n_i - c_i |                  e_n + e_c + u | n - c |
  q = p + root                   u |q|; dot = n . (q - b): sum_c |n_c| (u |q_c| + 4 u |q_c - b_c|)
  a scalar mean                  sum of the per-element errors + (DEPTH + 2) u sum |term| (+ 1 for item 0's weight in the Laplacian term),
                                 DEPTH = the documented tree's
  u_i = +-(L p) / n              e_Lp / n + |u| e_n / n + u |u|
  gradient element               c_l2 d (3 u) - [dot < 0] c_pen n_b (2 u) + c_lap_b (L u)_i (its own error + 2 u), + 3 u of the sum of the magnitudes
Nothing here is a measured number.

Discrete decisions and near-singular points, where two correct fp32 evaluations may differ: flags() marks an (item, vertex) when |dot| or the gap
between the nearest and second-nearest squared body distance is below 4 x its forward error bound; when the vertex, or a vertex it shares a
face with, has n_i or | n_i - c_i | below 4 x its bound (u_i may be zero, or of either sign) or belongs to a face of p or g one of whose
corners has sin(angle) < SIN_MIN = 1e-3 (the first-order bound of its cotangents stops meaning anything)."""
import os

import numpy as np

from stage2_loss_twin import GOLDEN, U, garment_case as _stage2_garment_case, nearest, vertex_normals64  # noqa: F401

E_ULP = 2.0
TINY = 2.0 ** -126
SIN_MIN = 1e-3
TERMS = ("l2", "msre", "pen", "lap", "pca")
LAMBDAS = (0.05, 0.001, 40.0, 50.0, 1.0)     # tshirt.yaml: sem_seg, PCA coefficients, L2, interpenetration, Laplacian
KEYS = ("sem_seg_loss", "garment_pca_coeff_l2", "garment_l2_loss", "garment_msre", "interpenetration_loss", "garment_lap_loss", "total_loss")


def load():
    return np.load(os.path.join(GOLDEN, "stage1_loss.npz"))


def ce_depth(rows):
    return 9 + (-(-(-(-rows // 256)) // 256) - 1) + 9


def garment_depth(B, Vg):
    return 9 + (-(-Vg // 256) - 1) + (-(-B // 256) - 1) + 9


def pca_depth(n):
    return max(-(-n // 256) - 1, 0) + 9


# ---------------------------------------------------------------------------------------------------------------------- cross-entropy
def cross_entropy(x, y, weight=1.0):
    """x (rows, C) fp32 logits, y (rows,) labels in [0, C).  Returns dict(value, bound, grad (rows, C) of weight * value, grad_bound)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.int64)
    rows, C = x.shape
    r = np.arange(rows)
    m = x.max(1, keepdims=True)
    z = x - m
    e = np.exp(z)
    rel = U * np.abs(z) + 2 * E_ULP * U
    s = e.sum(1)
    e_e = e * rel + TINY
    e_s = e_e.sum(1) + (C - 1) * U * s
    logs = np.log(s)
    zy = z[r, y]
    loss = logs - zy
    e_loss = e_s / s + 2 * E_ULP * U * np.abs(logs) + U * np.abs(zy) + U * np.abs(loss)
    D = ce_depth(rows)
    value = loss.sum() / rows
    bound = (e_loss.sum() + (D + 2) * U * np.abs(loss).sum()) / rows
    p = e / s[:, None]
    oh = np.zeros_like(p)
    oh[r, y] = 1.0
    scale = weight / rows
    grad = scale * (p - oh)
    gb = abs(scale) * (e_e / s[:, None] + p * ((e_s / s)[:, None] + U) + U * np.abs(p - oh)) + 2 * U * np.abs(grad) + TINY
    return dict(value=value, bound=bound, grad=grad, grad_bound=gb)


# ------------------------------------------------------------------------------------------------------------------------- cotangents
def cotangents(x, faces):
    """x (B, Vg, 3), faces (nf, 3).  Returns (h (B, nf, 3) half-cotangents per corner, e_h their bounds, sin (B, nf, 3) per corner)."""
    x, f = np.asarray(x, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = x[:, f[:, 0]], x[:, f[:, 1]], x[:, f[:, 2]]
    ab, ac, bc = b - a, c - a, c - b
    cr = np.cross(ab, ac)
    yz = lambda p, q: np.stack([np.abs(p[..., 1] * q[..., 2]) + np.abs(p[..., 2] * q[..., 1]), np.abs(p[..., 2] * q[..., 0]) + np.abs(p[..., 0] * q[..., 2]),
                                np.abs(p[..., 0] * q[..., 1]) + np.abs(p[..., 1] * q[..., 0])], -1)
    e_cr = 4 * U * yz(ab, ac)
    n = np.linalg.norm(cr, axis=-1)
    pairs = ((ab, ac, 1.0), (bc, ab, -1.0), (ac, bc, 1.0))
    d = np.stack([sg * (p * q).sum(-1) for p, q, sg in pairs], -1)
    e_d = np.stack([5 * U * (np.abs(p) * np.abs(q)).sum(-1) for p, q, _ in pairs], -1)
    ll = np.stack([np.linalg.norm(p, axis=-1) * np.linalg.norm(q, axis=-1) for p, q, _ in pairs], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_n = np.where(n > 0, (np.abs(cr) * e_cr).sum(-1) / n, 0.0) + 3 * U * n
        h = np.where(n[..., None] > 0, 0.5 * d / n[..., None], 0.0)
        e_h = np.where(n[..., None] > 0, 0.5 * (e_d / n[..., None] + np.abs(d) * e_n[..., None] / n[..., None] ** 2) + U * np.abs(h), 0.0)
        sin = np.where(ll > 0, n[..., None] / ll, 0.0)
    return h, e_h, sin


def lap_apply(x, h, e_h, faces, e_x=None):
    """(L x)_i = sum over the incidences of vertex i (corner c of face f, the other corners c1, c2 cyclic) of
    h[f, c1] (x[f[c2]] - x_i) + h[f, c2] (x[f[c1]] - x_i).  Returns (L x (B, Vg, 3), its bound)."""
    x, f = np.asarray(x, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    B, Vg, _ = x.shape
    out, A, Eh, Ex = (np.zeros((B, Vg, 3)) for _ in range(4))
    cnt = np.zeros(Vg)
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        i = f[:, c]
        np.add.at(cnt, i, 1.0)
        for hc, other in ((c1, f[:, c2]), (c2, f[:, c1])):
            D = x[:, other] - x[:, i]
            w = h[:, :, hc][..., None]
            np.add.at(out, (slice(None), i), w * D)
            np.add.at(A, (slice(None), i), np.abs(w) * np.abs(D))
            np.add.at(Eh, (slice(None), i), e_h[:, :, hc][..., None] * np.abs(D))
            if e_x is not None:
                np.add.at(Ex, (slice(None), i), np.abs(w) * (e_x[:, other] + e_x[:, i]))
    return out, Eh + Ex + (2 * cnt[None, :, None] + 2) * U * A


def neighbours(faces, Vg):
    """(Vg, Vg) scipy CSR 0/1 matrix: i and j share a face (i == j included)."""
    import scipy.sparse as sp
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rows = np.concatenate([f[:, a] for a in range(3) for _ in range(3)] + [np.arange(Vg)])
    cols = np.concatenate([f[:, b] for _ in range(3) for b in range(3)] + [np.arange(Vg)])
    M = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(Vg, Vg))
    M.data[:] = 1.0
    return M


# ---------------------------------------------------------------------------------------------------------------------------- garment
def evaluate(p, g, root, body, normals, faces, coeff, coeff_gt, pad_batch, nn=None):
    """Everything of the garment entry point in float64: per-vertex terms, their forward error bounds, the five means and their bounds, the
    pieces of the gradient.  nn: the nearest-vertex index to use (default: this module's own search)."""
    p, g, root, body, normals, coeff, coeff_gt = (np.asarray(a, np.float64) for a in (p, g, root, body, normals, coeff, coeff_gt))
    B, Vg, _ = p.shape
    Bp = int(pad_batch)
    assert Bp >= B and root.shape == (B, 3)
    wt = np.ones(B)
    wt[0] = 1 + Bp - B
    r = dict(B=B, Bp=Bp, Vg=Vg, faces=np.asarray(faces, np.int64).reshape(-1, 3), wt=wt)
    q = p + root[:, None, :]
    e_q = U * np.abs(q)
    r["idx"], d1, d2 = nearest(q, body)
    fin = np.where(np.isfinite(d2), d2, 0.0)
    qn = np.linalg.norm(e_q, axis=-1)
    r["nn_gap"], r["nn_gap_err"] = d2 - d1, 5 * U * (d1 + fin) + 2 * qn * (np.sqrt(d1) + np.sqrt(fin))
    nn = r["idx"] if nn is None else np.asarray(nn, np.int64)
    bi = np.arange(B)[:, None]
    d = p - g
    l2 = (d ** 2).sum(-1)
    ms = np.sqrt(l2)
    b, n = body[bi, nn], normals[bi, nn]
    dot = (n * (q - b)).sum(-1)
    e_dot = (np.abs(n) * (e_q + 4 * U * np.abs(q - b))).sum(-1)
    pen = np.maximum(-dot, 0.0)
    hg, e_hg, sin_g = cotangents(g, r["faces"])
    hp, e_hp, sin_p = cotangents(p, r["faces"])
    Lg, e_Lg = lap_apply(g, hg, e_hg, r["faces"])
    Lp, e_Lp = lap_apply(p, hp, e_hp, r["faces"])
    cn, nn_ = np.linalg.norm(Lg, axis=-1), np.linalg.norm(Lp, axis=-1)
    e_c, e_n = e_Lg.sum(-1) + 4 * U * cn, e_Lp.sum(-1) + 4 * U * nn_
    lap = np.abs(nn_ - cn)
    e_lap = e_n + e_c + U * lap
    pd = coeff - coeff_gt
    r.update(q_minus_b=q - b, d=d, dot=dot, e_dot=e_dot, n=n, hp=hp, e_hp=e_hp, sin=np.minimum(sin_g, sin_p), Lp=Lp, e_Lp=e_Lp, lap_n=nn_, lap_c=cn,
             e_n=e_n, e_c=e_c, pd=pd)
    D = garment_depth(B, Vg)
    cnt = B * Vg
    r["values"], r["value_bounds"] = {}, {}
    for k, (v, err) in dict(l2=(l2, 5 * U * l2), msre=(ms, 4 * U * ms), pen=(pen, e_dot)).items():
        r["values"][k] = v.sum() / cnt
        r["value_bounds"][k] = (err.sum() + (D + 2) * U * np.abs(v).sum()) / cnt
    r["values"]["lap"] = (wt[:, None] * lap).sum() / (Bp * Vg)
    r["value_bounds"]["lap"] = ((wt[:, None] * e_lap).sum() + (D + 3) * U * (wt[:, None] * lap).sum()) / (Bp * Vg)
    npca = pd.size
    r["values"]["pca"] = (pd ** 2).sum() / npca if npca else 0.0
    r["value_bounds"]["pca"] = ((3 * U * pd ** 2).sum() + (pca_depth(npca) + 2) * U * (pd ** 2).sum()) / npca if npca else 0.0
    return r


def gradient(r, weights):
    """((grad_pred (B,Vg,3), bound), (grad_coeff (B,P), bound)) of  w_pca PCA + w_l2 L2 + w_pen Pen + w_lap Lap  from evaluate()'s record."""
    B, Bp, Vg = r["B"], r["Bp"], r["Vg"]
    w_pca, w_l2, w_pen, w_lap = (float(w) for w in weights)
    c = 2.0 * w_l2 / (B * Vg)
    g_l2, b_l2 = c * r["d"], 3 * U * np.abs(c * r["d"])
    c = w_pen / (B * Vg)
    g_pen = -c * r["n"] * (r["dot"] < 0)[..., None]
    b_pen = 2 * U * np.abs(g_pen)
    n, cn = r["lap_n"][..., None], r["lap_c"][..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        live = (n > 0) & (n != cn)
        u = np.where(live, np.sign(n - cn) * r["Lp"] / n, 0.0)
        e_u = np.where(live, r["e_Lp"] / n + np.abs(u) * (r["e_n"][..., None] / n) + U * np.abs(u), 0.0)
    Lu, e_Lu = lap_apply(u, r["hp"], r["e_hp"], r["faces"], e_x=e_u)
    cl = (w_lap * r["wt"] / (Bp * Vg))[:, None, None]
    g_lap = cl * Lu
    b_lap = np.abs(cl) * e_Lu + 2 * U * np.abs(g_lap)
    mag = np.abs(g_l2) + np.abs(g_pen) + np.abs(g_lap)
    npca = r["pd"].size
    g_pca = (2.0 * w_pca / npca) * r["pd"] if npca else r["pd"]
    return (g_l2 + g_pen + g_lap, b_l2 + b_pen + b_lap + 3 * U * mag), (g_pca, 3 * U * np.abs(g_pca))


def flags(r):
    """(B, Vg) bool: see the module docstring.  margin = 4 x the forward error bound of the quantity."""
    fl = np.abs(r["dot"]) < 4 * r["e_dot"]
    fl |= r["nn_gap"] < 4 * r["nn_gap_err"]
    unsure = (r["lap_n"] < 4 * r["e_n"]) | (np.abs(r["lap_n"] - r["lap_c"]) < 4 * (r["e_n"] + r["e_c"]))
    sliver = (r["sin"] < SIN_MIN).any(-1)                                 # (B, nf)
    f = r["faces"]
    for c in range(3):
        for b in range(r["B"]):
            unsure[b, f[sliver[b], c]] = True
    fl |= (neighbours(f, r["Vg"]) @ unsure.astype(np.float64).T).T > 0
    return fl


def total(ce_value, values, weights):
    """total_loss in the reference's order from the cross-entropy value and evaluate()['values']; weights = the five lambdas."""
    w_sem, w_pca, w_l2, w_pen, w_lap = weights
    return w_sem * ce_value + w_pca * values["pca"] + w_l2 * values["l2"] + w_pen * values["pen"] + w_lap * values["lap"]


def total_bound(ce_value, ce_bound, values, bounds, weights):
    """Bound of total_loss: the terms' bounds carried through the weights, plus 6 roundings (a weight product and up to four additions on a path,
    the rounded weight) relative to each term."""
    w = [abs(float(x)) for x in weights]
    out = w[0] * (ce_bound + 6 * U * abs(ce_value))
    for k, wk in zip(("pca", "l2", "pen", "lap"), w[1:]):
        out += wk * (bounds[k] + 6 * U * abs(values[k]))
    return out


def golden_inputs(case):
    """The operands of evaluate() for synthetic.stage1_loss_case, as the reference's loss assembles them (float64 normals of the T-pose body)."""
    B = case["nbatch"]
    o, i = case["output"], case["inputs"]
    body = i["Tpose_smpl_vertices_torch"].reshape(B, -1, 3)
    return dict(p=o["tpose_garment"].reshape(B, -1, 3), g=i["garment_template_vertices"].reshape(B, -1, 3), root=i["Tpose_smpl_root_joints_torch"].reshape(B, 3),
                body=body, normals=vertex_normals64(body, case["body"]["faces"]), faces=o["garment_f_3"], coeff=o["garment_PCA_coeff"],
                coeff_gt=i["PCACoeff"].reshape(B, -1), pad_batch=case["pad_batch"])


GRIDS = ((8, 8), (13, 15), (64, 64))                  # Vg = 64, ragged 195, 4096 (16 workgroups per item)
PADS = ((1, 1), (2, 2), (2, 4), (3, 5))               # (B, Bp)
GPU_CASES = [(rows, cols, B, Bp) for rows, cols in GRIDS for B, Bp in PADS]
CE_ROWS, CE_CLASSES = (1, 63, 64, 257, 2 * 3 * 100), (1, 2, 7, 13)


def case_seed(rows, cols, B, Bp):
    return 300 + rows + 7 * B + Bp


def ce_case(rows, C):
    """Logits of a few units with one row of +-80 spread (the max subtraction), labels over all classes."""
    rng = np.random.default_rng(1000 * C + rows)
    x = (rng.standard_normal((rows, C)) * 3.0).astype(np.float32)
    x[rows // 2] = np.linspace(-80.0, 80.0, C, dtype=np.float32) if C > 1 else np.float32(80.0)
    return x, rng.integers(0, C, rows).astype(np.int64)


def garment_case(seed, B, rows, cols, P=16):
    """Synthetic kernel inputs on a rows x cols quad-cylinder garment (its quads split into triangles) around a body cylinder: stage2_loss_twin's
    garment_case with one frame per item, plus root joints (the prediction is stored relative to them), PCA coefficients and targets.  The target
    is moved by another N(0, 0.03) per coordinate: with stage 2's centimetre, n_i - c_i is within rounding distance of zero at 0.15 % of the
    vertices, and each of those flags its whole one-ring."""
    c = _stage2_garment_case(seed, B, 1, rows, cols)
    rng = np.random.default_rng(seed + 1000)
    root = rng.normal(0.0, 0.05, (B, 3)).astype(np.float32)
    q = c["faces"]
    faces3 = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    coeff = rng.standard_normal((B, P)).astype(np.float32)
    coeff_gt = (coeff + rng.normal(0.0, 0.3, (B, P))).astype(np.float32)
    return dict(B=B, Vg=c["Vg"], p=(c["p"] - root[:, None, :]).astype(np.float32), g=(c["g"] + rng.normal(0.0, 0.03, c["g"].shape) - root[:, None, :]).astype(np.float32), root=root,
                body=c["body"], normals=c["normals"], faces=faces3, coeff=coeff, coeff_gt=coeff_gt)

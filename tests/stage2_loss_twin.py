"""float64 twin of the stage-2 objective (garment4d_amd/csrc/refine_loss.hip; smplx/loss/temporal_loss.py:147-201 in the reference) in numpy,
shared by tests/test_stage2_loss_cpu.py (which ties it to the reference's own run through tests/golden/stage2_loss.npz) and
tests/test_stage2_loss_gpu.py (which holds the kernel to it).  Not a test module.

One round's prediction p (F,Vg,3), F = nbatch * T; target g; body vertices / unit normals (F,V,3); L the (Vg,Vg) Laplacian as the fp32 values the
kernel receives (promoted exactly).  Terms: L2 = mean |p-g|^2, MSRE = mean |p-g|, Laplacian = mean |(L p)_i|, penetration =
mean relu(-n_b.(p-b)) with b the nearest body vertex (lowest index on ties), temporal = mean over (clip, t < T-1, vertex) of |p_t - p_{t+1}|.
A zero norm contributes a zero gradient (the kernel's documented convention; torch.norm agrees for the Laplacian term).

Error bounds (first order, u = 2^-24; the rule of refine_grad_twin: a sum of n products with m roundings of their own errs by at most
(n + m) u A, A = the same expression over absolute values; a summation tree of depth d errs by at most d u A).  The kernel's arithmetic, as
its header documents it (every product and sum rounded on its own):
  d = p - g                      1 rounding per coordinate
  |x|^2 = (x0 x0 + x1 x1) + x2 x2  coordinates with relative error e: (2 e + 3) u |x|^2 -> 5 u |x|^2 for a rounded difference
  |x| = sqrt(|x|^2)              2.5 u + 1 u -> 4 u |x|
  (L p)_i,c = sum_k val_k (p_j - p_i)_c + rowsum_i p_i,c: difference 1, product 1, row-length additions (the last one adds the row-sum
                                 product, itself 2 roundings): (r + 3) u A_c,  A_c = sum_k |val_k| |p_j - p_i|_c + |rowsum_i p_i,c|
  |L p|                          sum_c of the coordinate errors + 4 u |L p|
  dot = n . (p - b)              difference 1, product 1, two additions: 4 u sum_c |n_c| |p_c - b_c|
  a scalar mean                  sum of the per-vertex errors + (DEPTH + 2) u sum |term|, times 1/n; DEPTH = reduction_depth(F, Vg), the
                                 documented tree; + 2 = the rounded 1/n and the final product
  unit vector x / |x|            coordinate 1, norm 4, division 1: 6 u per coordinate for a rounded difference x; for u_i = L p / |L p| the
                                 coordinate error of L p and the error of its norm are carried instead
  gradient element               c_l2 d (3 u: constant, d, product) - [dot < 0] c_pen n (2 u) + c_tmp (t_own - t_prev) (6 u each + the
                                 subtraction + constant + product: 9 u) + c_lap (L^T u)_i (row of r' products of inexact u: sum |val| e_u +
                                 (r' + 3) u sum |val| |u|), and 4 u times the sum of the four magnitudes for the three additions and the update.
Nothing here is a measured number.

Discrete decisions and near-singular points, where two correct fp32 evaluations may differ: flags() marks a (frame, vertex) when |dot|, the
gap between the nearest and second-nearest squared body distance, |L p| of the vertex or of any vertex in its row of L^T, or |p_t - p_{t+1}| of
one of its (up to two) frame pairs is below 4 x the forward error bound of that quantity."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
TERMS = ("l2", "msre", "lap", "pen", "tmp")
LAMBDAS = (20.0, 10.0, 100.0, 5.0)     # tshirt.yaml: L2, Laplacian, interpenetration, temporal


def load():
    return np.load(os.path.join(GOLDEN, "stage2_loss.npz"))


def reduction_depth(F_, Vg):
    """The kernel's documented tree: 9 per workgroup, the frame's workgroups left to right, the finishing thread's frames in order, 9 again."""
    return 9 + (-(-Vg // 256) - 1) + (-(-F_ // 256) - 1) + 9


def laplacian_from_faces(faces, vg):
    """lap_adj as the model builds it (mesh_encoder.py: I - D^-1 adj_old, cast to fp32): scipy CSR with float32 data."""
    import scipy.sparse as sp
    from garment4d_amd import gcn
    adj_old = gcn.adjacency_old_from_faces(faces, vg)
    return sp.csr_matrix((sp.eye(vg) - gcn.normalize(adj_old)).astype(np.float32))


def vertex_normals64(verts, faces):
    """utils/mesh_utils.py:116-134 (compute_fnorms + compute_vnorms) in float64: unit face normals (norm clamped at 1e-6) summed over each
    vertex's incident faces, re-normalised with the same clamp."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    fn = np.cross(v[:, f[:, 1]] - v[:, f[:, 0]], v[:, f[:, 2]] - v[:, f[:, 0]])
    fn = fn / np.maximum(np.linalg.norm(fn, axis=-1, keepdims=True), 1e-6)
    vn = np.zeros_like(v)
    for fr in range(v.shape[0]):
        for c in range(3):
            np.add.at(vn[fr], f[:, c], fn[fr])
    return vn / np.maximum(np.linalg.norm(vn, axis=-1, keepdims=True), 1e-6)


def golden_inputs(case):
    """(rounds, target, body, float64 normals, L, nbatch, T) of synthetic.stage2_loss_case, as the reference's loss assembles them."""
    nbatch, T, Vg = case["nbatch"], case["T"], case["Vg"]
    F_ = nbatch * T
    body = case["inputs"]["smpl_vertices_torch"].reshape(F_, -1, 3)
    gt = (case["inputs"]["garment_torch"].astype(np.float64) + case["inputs"]["smpl_root_joints_torch"].astype(np.float64)[:, :, None, :]).reshape(F_, Vg, 3)
    return case["rounds"], gt, body, vertex_normals64(body, case["body"]["faces"]), laplacian_from_faces(case["template_faces"], Vg), nbatch, T


def nearest(p, body, chunk=64):
    """float64 brute force: (index of the nearest body vertex, lowest on ties (F,Vg); nearest and second-nearest squared distance)."""
    p, body = np.asarray(p, np.float64), np.asarray(body, np.float64)
    F_, Vg, _ = p.shape
    idx = np.empty((F_, Vg), np.int64)
    d1, d2 = np.empty((F_, Vg)), np.empty((F_, Vg))
    for f in range(F_):
        for lo in range(0, Vg, chunk):
            d = ((p[f, lo:lo + chunk, None, :] - body[f][None]) ** 2).sum(-1)
            i = np.argmin(d, 1)
            idx[f, lo:lo + chunk] = i
            d1[f, lo:lo + chunk] = d[np.arange(d.shape[0]), i]
            d[np.arange(d.shape[0]), i] = np.inf
            d2[f, lo:lo + chunk] = d.min(1) if d.shape[1] > 1 else np.inf
    return idx, d1, d2


def evaluate(p, g, body, normals, L, nbatch, T, temporal=True, nn=None):
    """Everything of one round in float64: per-vertex terms, their forward error bounds, the five means and their bounds, the pieces of the
    gradient.  nn: the nearest-vertex index to use (default: this module's own search)."""
    import scipy.sparse as sp
    p, g, body, normals = (np.asarray(a, np.float64) for a in (p, g, body, normals))
    F_, Vg, _ = p.shape
    assert F_ == nbatch * T
    L = sp.csr_matrix(L).astype(np.float64)
    r = {"F": F_, "Vg": Vg, "nbatch": nbatch, "T": T, "L": L}
    r["idx"], d1, d2 = nearest(p, body)
    r["nn_gap"], r["nn_gap_err"] = d2 - d1, 5 * U * (d1 + np.where(np.isfinite(d2), d2, 0.0))
    nn = r["idx"] if nn is None else np.asarray(nn, np.int64)
    fi = np.arange(F_)[:, None]
    # L2 / MSRE
    d = p - g
    l2 = (d ** 2).sum(-1)
    ms = np.sqrt(l2)
    # Laplacian, in the kernel's difference form (exact rearrangement of L p)
    rowlen = np.diff(L.indptr)
    rowsum = np.asarray(L.sum(1)).reshape(-1)
    pv = p.transpose(1, 0, 2).reshape(Vg, F_ * 3)
    Lp = (L @ pv).reshape(Vg, F_, 3).transpose(1, 0, 2)
    La = abs(L).tocsr()
    A = np.zeros((F_, Vg, 3))
    coo = La.tocoo()
    np.add.at(A, (slice(None), coo.row), coo.data[None, :, None] * np.abs(p[:, coo.col] - p[:, coo.row]))
    A += np.abs(rowsum)[None, :, None] * np.abs(p)
    e_Lp = (rowlen[None, :, None] + 3) * U * A
    lap = np.linalg.norm(Lp, axis=-1)
    e_lap = e_Lp.sum(-1) + 4 * U * lap
    # penetration
    b, n = body[fi, nn], normals[fi, nn]
    dot = (n * (p - b)).sum(-1)
    e_dot = 4 * U * (np.abs(n) * np.abs(p - b)).sum(-1)
    pen = np.maximum(-dot, 0.0)
    # temporal
    has_tmp = bool(temporal) and T > 1
    tmp = np.zeros((F_, Vg))
    pair = np.zeros(F_, bool)
    e = np.zeros((F_, Vg, 3))
    if has_tmp:
        pair = (np.arange(F_) % T) < T - 1
        e[pair] = p[pair] - p[np.nonzero(pair)[0] + 1]
        tmp = np.linalg.norm(e, axis=-1)
    r.update(p_minus_b=p - b, d=d, l2=l2, msre=ms, Lp=Lp, e_Lp=e_Lp, lap=lap, e_lap=e_lap, dot=dot, e_dot=e_dot, pen=pen, n=n, e=e, tmp=tmp, e_tmp=4 * U * tmp, pair=pair,
             has_tmp=has_tmp, rowlen=rowlen)
    per = dict(l2=(l2, 5 * U * l2), msre=(ms, 4 * U * ms), lap=(lap, e_lap), pen=(pen, e_dot), tmp=(tmp, 4 * U * tmp))
    D = reduction_depth(F_, Vg)
    n_all, n_tmp = F_ * Vg, nbatch * (T - 1) * Vg
    r["values"], r["value_bounds"] = {}, {}
    for k, (v, err) in per.items():
        cnt = n_tmp if k == "tmp" else n_all
        if k == "tmp" and not has_tmp:
            r["values"][k], r["value_bounds"][k] = 0.0, 0.0
            continue
        r["values"][k] = v.sum() / cnt
        r["value_bounds"][k] = (err.sum() + (D + 2) * U * np.abs(v).sum()) / cnt
    r["msre_frames"] = ms.mean(1)
    r["msre_frames_bound"] = ((4 * U * ms).sum(1) + (9 + (-(-Vg // 256) - 1) + 2) * U * ms.sum(1)) / Vg
    return r


def gradient(r, weights):
    """(grad (F,Vg,3), bound (F,Vg,3)) of  w_l2 L2 + w_lap Lap + w_pen Pen + w_tmp Tmp  w.r.t. p, from evaluate()'s record."""
    F_, Vg, nbatch, T, L = r["F"], r["Vg"], r["nbatch"], r["T"], r["L"]
    w_l2, w_lap, w_pen, w_tmp = (float(w) for w in weights)
    n_all = F_ * Vg
    # L2
    c = 2.0 * w_l2 / n_all
    g_l2 = c * r["d"]
    b_l2 = 3 * U * np.abs(g_l2)
    # penetration
    c = w_pen / n_all
    g_pen = -c * r["n"] * (r["dot"] < 0)[..., None]
    b_pen = 2 * U * np.abs(g_pen)
    # temporal
    g_tmp, b_tmp = np.zeros((F_, Vg, 3)), np.zeros((F_, Vg, 3))
    if r["has_tmp"]:
        c = w_tmp / (nbatch * (T - 1) * Vg)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(r["tmp"][..., None] > 0, r["e"] / r["tmp"][..., None], 0.0)
        own, prev = t.copy(), np.zeros_like(t)
        prev[1:] = t[:-1]                      # frame f receives -t of the pair (f-1, f); t is zero where f-1 starts no pair
        g_tmp = c * (own - prev)
        b_tmp = 9 * U * np.abs(c) * (np.abs(own) + np.abs(prev))
    # Laplacian
    c = w_lap / n_all
    lapn = r["lap"][..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(lapn > 0, r["Lp"] / lapn, 0.0)
        e_u = np.where(lapn > 0, r["e_Lp"] / lapn + np.abs(u) * (r["e_lap"][..., None] / lapn) + U * np.abs(u), 0.0)
    Lt = L.T.tocsr()
    rt = np.diff(Lt.indptr)
    flat = lambda a: a.transpose(1, 0, 2).reshape(Vg, F_ * 3)
    back = lambda a: a.reshape(Vg, F_, 3).transpose(1, 0, 2)
    g_lap = c * back(Lt @ flat(u))
    b_lap = np.abs(c) * (back(abs(Lt) @ flat(e_u)) + (rt[None, :, None] + 3) * U * back(abs(Lt) @ flat(np.abs(u))))
    grad = g_l2 + g_pen + g_tmp + g_lap
    mag = np.abs(g_l2) + np.abs(g_pen) + np.abs(g_tmp) + np.abs(g_lap)
    return grad, b_l2 + b_pen + b_tmp + b_lap + 4 * U * mag


def flags(r):
    """(F,Vg) bool: see the module docstring.  margin = 4 x the forward error bound of the quantity."""
    F_, Vg, T, L = r["F"], r["Vg"], r["T"], r["L"]
    fl = np.abs(r["dot"]) < 4 * r["e_dot"]
    fl |= r["nn_gap"] < 4 * r["nn_gap_err"]
    small = (r["lap"] < 4 * r["e_lap"]).astype(np.float64)           # (F,Vg)
    pattern = (abs(L.T.tocsr()) > 0).astype(np.float64)
    fl |= small > 0
    fl |= (pattern @ small.T).T > 0                                   # a vertex whose row of L^T holds such a vertex
    if r["has_tmp"]:
        close = r["pair"][:, None] & (r["tmp"] < 4 * r["e_tmp"])
        fl |= close
        fl[1:] |= close[:-1]
    return fl


def total(values_per_round, weights):
    """total_loss from the per-round values (dicts of evaluate()['values']); the temporal term counts for the last round only."""
    w_l2, w_lap, w_pen, w_tmp = weights
    return (w_l2 * sum(v["l2"] for v in values_per_round) + w_lap * sum(v["lap"] for v in values_per_round)
            + w_pen * sum(v["pen"] for v in values_per_round) + w_tmp * values_per_round[-1]["tmp"])


def total_bound(values_per_round, bounds_per_round, weights):
    """Bound of total_loss: the per-round bounds carried through the weights, plus (R + 4) roundings of the accumulation over the R rounds, the
    weight products and the final additions."""
    R = len(values_per_round)
    ws = dict(zip(("l2", "lap", "pen", "tmp"), (abs(float(w)) for w in weights)))
    out = 0.0
    for k, w in ws.items():
        rounds = range(R) if k != "tmp" else [R - 1]
        out += w * sum(bounds_per_round[i][k] + (R + 4) * U * abs(values_per_round[i][k]) for i in rounds)
    return out


def acceleration_error(pred, gt, nbatch, T):
    def accel(v):
        v = np.asarray(v, np.float64).reshape(nbatch, T, -1, 3)
        vel = (v[:, 1:] - v[:, :-1]) / (1 / 30)
        return (vel[:, 1:] - vel[:, :-1]) / (1 / 30)
    return float(np.sqrt(((accel(pred) - accel(gt)) ** 2).sum(-1)).mean())


def acceleration_error_bound(pred, gt, nbatch, T):
    """Bound of an fp32 evaluation of acceleration_error in ANY summation order.  Per coordinate a = ((p2 - p1) / dt - (p1 - p0) / dt) / dt: three
    differences and three divisions by the rounded dt, at most 9 roundings on a path, each relative to a magnitude of at most
    900 (|p2| + 2 |p1| + |p0|); the same for the target, one more for their difference; the norm carries the coordinate errors + 4 u of
    itself; a mean of n terms in any order adds (n - 1) u, + 1 for the division."""
    def mag(v):
        v = np.abs(np.asarray(v, np.float64)).reshape(nbatch, T, -1, 3)
        return 900.0 * (v[:, 2:] + 2 * v[:, 1:-1] + v[:, :-2])
    def accel(v):
        v = np.asarray(v, np.float64).reshape(nbatch, T, -1, 3)
        return 900.0 * (v[:, 2:] - 2 * v[:, 1:-1] + v[:, :-2])
    e = 10 * U * (mag(pred) + mag(gt))
    norm = np.sqrt(((accel(pred) - accel(gt)) ** 2).sum(-1))
    return float((e.sum(-1) + 4 * U * norm).mean() + norm.size * U * norm.mean())


def garment_case(seed, nbatch, T, rows, cols, V=700, body_rc=(25, 28)):
    """Synthetic kernel inputs on a rows x cols quad-cylinder garment around a body cylinder: body vertices / their unit normals, garments
    placed by synthetic.garment_around_body (about half of the vertices penetrate, none at rounding distance of the surface)."""
    from garment4d_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    F_ = nbatch * T
    bv, bq = syn.quad_cylinder(*body_rc)
    bv = (bv * np.array([0.75, 0.7, 0.5], np.float32) + np.array([0, -0.35, 0], np.float32)).astype(np.float32)
    faces = np.concatenate([bq[:, [0, 1, 2]], bq[:, [0, 2, 3]]], 0).astype(np.int64)
    drift = np.cumsum(rng.standard_normal((nbatch, T, 1, 3)) * 0.004, axis=1).reshape(F_, 1, 3)
    body = (bv[None] + drift + rng.standard_normal((F_, bv.shape[0], 3)) * 0.001).astype(np.float32)
    normals = syn.vertex_normals(body, faces)
    _, gq = syn.quad_cylinder(rows, cols)
    Vg = rows * cols
    sel = rng.integers(0, body.shape[1], Vg)
    p = syn.garment_around_body(rng, body, normals, sel)
    g = (body[:, sel] + rng.normal(0.0, 0.01, (F_, Vg, 3))).astype(np.float32)
    return dict(nbatch=nbatch, T=T, Vg=Vg, p=p, g=g, body=body, normals=normals, L=laplacian_from_faces(gq, Vg), faces=gq)

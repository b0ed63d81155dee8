"""numpy restatement of include/g4d_fit.h (test infrastructure; the package never imports it), on top of tests/postprocess_twin.py, whose
float64 search and scenes it uses.  dtype=np.float64 is the reference; dtype=np.float32 replays the header's operation order bit for bit: the
closest point with PT._dot's emulated fused multiply-adds, the frame sums lane by lane and through the fixed tree, the gradient one addition
after the other in the stated order.  err_* are bounds of |fp32 - float64| derived from the operation counts (see error_bounds).

Not a test module: tests/test_fit_cpu.py and tests/test_fit_gpu.py import it."""
import numpy as np

import postprocess_twin as PT

F32, F64 = np.float32, np.float64
LANES, WAVE = 1024, 64
INDEX_BITS, MAX_POINTS, MAX_FACES = 15, 32768, 131072
NO_KEY = np.uint32(0xFFFFFFFF)
EPS32 = 2.0 ** -24            # half an ulp of 1: the relative error of one rounded fp32 operation


# ------------------------------------------------------------------------------------------------------------------------ closest point
def closest_bary(q, a, b, c):
    """PT.closest_on_triangle with the weights it drops: (bary (...,3) = (u, v, w), point, resid = q - point, dist2, part), all of q's dtype,
    in the operation order include/g4d.h states for g4d_mesh_nearest_f32 and u = (1 - v) - w."""
    q, a, b, c = np.broadcast_arrays(q, a, b, c)
    dt = q.dtype
    ab, ac = b - a, c - a
    d1, d2 = PT._dot(ab, q - a), PT._dot(ac, q - a)
    d3, d4 = PT._dot(ab, q - b), PT._dot(ac, q - b)
    d5, d6 = PT._dot(ab, q - c), PT._dot(ac, q - c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
    part = np.select(conds, [4, 5, 1, 6, 3, 2], default=0)
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    den = np.select([part == 0, part == 1, part == 2, part == 3], [(va + vb) + vc, d1 - d3, e43 + e56, d2 - d6], default=one)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (one / den).astype(dt)
        w = np.select([part == 0, part == 2, part == 3, part == 6], [vc * r, e43 * r, d2 * r, one], default=zero).astype(dt)
        v = np.select([part == 0, part == 1, part == 2, part == 5], [vb * r, d1 * r, one - w, one], default=zero).astype(dt)
        point = ((a + ab * v[..., None]) + ac * w[..., None]).astype(dt)
        resid = (q - point).astype(dt)
        dist2 = ((resid[..., 0] * resid[..., 0] + resid[..., 1] * resid[..., 1]) + resid[..., 2] * resid[..., 2]).astype(dt)
        u = ((one - v) - w).astype(dt)
    return np.stack([u, v, w], -1), point, resid, dist2, part.astype(np.int32)


def point_terms(points, verts, faces, face, weights=None, tau2=np.inf, dtype=F64):
    """All frames: points (F,P,3), verts (F,V,3), faces (nf,3), face (F,P) -> dict(bary, resid, dist2, inlier (bool), usable, part, wt)."""
    p, v = np.asarray(points, dtype), np.asarray(verts, dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    face = np.asarray(face, np.int64)
    F_, P = face.shape
    V, nf = v.shape[1], len(f)
    wt = np.ones((F_, P), dtype) if weights is None else np.asarray(weights, dtype).reshape(F_, P)
    usable = (face >= 0) & (face < nf)
    tri = f[np.where(usable, face, 0)] if nf else np.zeros((F_, P, 3), np.int64)
    usable &= ((tri >= 0) & (tri < V)).all(-1)
    tri = np.where(usable[..., None], tri, 0)
    rows = np.arange(F_)[:, None]
    bary, _, resid, dist2, part = closest_bary(p, v[rows, tri[..., 0]], v[rows, tri[..., 1]], v[rows, tri[..., 2]])
    bary = np.where(usable[..., None], bary, 0).astype(dtype)
    resid = np.where(usable[..., None], resid, 0).astype(dtype)
    dist2 = np.where(usable, dist2, np.inf).astype(dtype)
    with np.errstate(invalid="ignore"):
        inlier = usable & (wt > 0) & (dist2 < dtype(tau2))
    return dict(bary=bary, resid=resid, dist2=dist2, inlier=inlier, usable=usable, part=np.where(usable, part, -1), wt=wt)


# -------------------------------------------------------------------------------------------------------------------------------- sums
def tree_sum(lanes):
    """The frame tree of the header on LANES partial sums (any dtype with exact '+' semantics of that dtype): a xor butterfly with strides
    32 .. 1 inside every run of 64 lanes, then the runs left to right."""
    x = np.asarray(lanes).reshape(LANES // WAVE, WAVE).copy()
    idx = np.arange(WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[:, idx ^ m]
    s = x[0, 0]
    for r in range(1, LANES // WAVE):
        s = s + x[r, 0]
    return s


def lane_sums(terms):
    """terms (P,) -> (LANES,): lane t adds terms[t], terms[t + LANES], ... in ascending order starting from 0 (a term of 0 leaves the bits alone)."""
    t = np.asarray(terms)
    P = len(t)
    acc = np.zeros(LANES, t.dtype)
    for s in range(0, P, LANES):
        chunk = t[s:s + LANES]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    return acc


def forward(points, verts, faces, face, weights=None, tau2=np.inf, dtype=F64, inlier=None):
    """point_terms plus the header's reductions: sums (F,3) = (S, Win, Wall), count (F) int32, W, loss -- in the header's order in either
    dtype.  inlier: take these flags instead of deciding them here (the float64 reference of an fp32 run whose decisions are known)."""
    t = point_terms(points, verts, faces, face, weights, tau2, dtype)
    if inlier is not None:
        t["inlier"] = np.asarray(inlier).astype(bool)
    F_, P = t["wt"].shape
    zero = dtype(0)
    sums = np.zeros((F_, 3), dtype)
    for f in range(F_):
        inl, wt = t["inlier"][f], t["wt"][f]
        with np.errstate(invalid="ignore"):
            wd2 = np.where(inl, wt * np.where(inl, t["dist2"][f], zero), zero).astype(dtype)
        sums[f] = [tree_sum(lane_sums(wd2)), tree_sum(lane_sums(np.where(inl, wt, zero).astype(dtype))), tree_sum(lane_sums(wt))]
    W, T = zero, zero
    for f in range(F_):
        T = dtype(T + sums[f, 0])
        W = dtype(W + sums[f, 2])
    t.update(sums=sums, count=t["inlier"].sum(1).astype(np.int32), W=W, loss=dtype(T / W) if W > 0 else zero)
    return t


# ---------------------------------------------------------------------------------------------------------------------------- grouping
def group(face, inlier, nf):
    """keys (F,P) uint32: face << 15 | index of the inliers with 0 <= face < nf in ascending order, 0xFFFFFFFF after them."""
    face, inlier = np.asarray(face, np.int64), np.asarray(inlier).astype(bool)
    F_, P = face.shape
    assert P <= MAX_POINTS and nf <= MAX_FACES
    ok = inlier & (face >= 0) & (face < nf)
    keys = np.where(ok, (np.where(ok, face, 0) << INDEX_BITS) | np.arange(P)[None], int(NO_KEY)).astype(np.uint32)
    return np.sort(keys, axis=1)


# ---------------------------------------------------------------------------------------------------------------------------- gradient
def grad_scales(W, grad_out, dtype):
    W, g = dtype(W), dtype(grad_out)
    if not W > 0:
        return dtype(0), dtype(0)
    return dtype(dtype(dtype(-2) * g) / W), dtype(dtype(dtype(2) * g) / W)


def gradients(t, keys, faces, num_verts, grad_out=1.0, dtype=F64):
    """t: a forward() dict of `dtype`; keys: group() of its face / inlier -> (grad_verts (F,V,3), grad_points (F,P,3)) in the header's order:
    per vertex its entries face * 3 + corner ascending, within a face the points in key order, one addition after the other."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F_, P = t["wt"].shape
    gs, gp = grad_scales(t["W"], grad_out, dtype)
    gv = np.zeros((F_, num_verts, 3), dtype)
    for fr in range(F_):
        n = int(t["count"][fr])
        k = keys[fr, :n].astype(np.int64)
        kf, ki = k >> INDEX_BITS, k & (MAX_POINTS - 1)
        pos = np.arange(n)
        ent = (kf[:, None] * 3 + np.arange(3)[None]).reshape(-1)                # entry of every (key, corner)
        vert = f[kf].reshape(-1)
        i3, pos3, corner = np.repeat(ki, 3), np.repeat(pos, 3), np.tile(np.arange(3), n)
        order = np.lexsort((pos3, ent, vert))                                    # by vertex, then entry, then position in the keys
        s = ((gs * t["wt"][fr, i3]) * t["bary"][fr, i3, corner]).astype(dtype)
        contrib = (s[:, None] * t["resid"][fr, i3]).astype(dtype)
        np.add.at(gv[fr], vert[order], contrib[order])                           # unbuffered: one addition after the other, in this order
    with np.errstate(invalid="ignore"):
        gpts = np.where(t["inlier"][..., None], ((gp * t["wt"])[..., None] * t["resid"]).astype(dtype), dtype(0)).astype(dtype)
    return gv, gpts


# ------------------------------------------------------------------------------------------------------------------------ error bounds
def error_bounds(t64, verts, faces, face, points, keys, num_verts, grad_out=1.0):
    """Bounds of |fp32 replay - float64| from the operation counts, per quantity, with e = EPS32 (one rounding), L = the longest edge of the
    point's triangle, R = the largest distance of the query to a corner, M = the largest coordinate involved, A = the triangle's area:

      a dot product of the routine:  two rounded differences per factor, a product and two fused steps        <= 5 e L R
      vc, vb, va (two products of two dots, one difference):   2 (5 + 5 + 1) + 1                               <= 23 e (L R)^2
      den = (va + vb) + vc = 4 A^2:  3 x 23 + 2                                                                <= 71 e (L R)^2
      v, w in the interior:  (23 + 71 + 2) e (L R)^2 / (4 A^2);  on an edge  (5 + 11 + 2) e L R / |edge|^2;  a corner is exact
      u = (1 - v) - w:  the two of them plus two roundings
    C_BARY = 128 per weight covers each case with room for the second-order terms; 2 C_BARY + 2 for u.
      point = (a + ab v) + ac w and resid = q - point:  L (dv + dw) + 6 e M
      dist2:  2 |resid| d_resid + d_resid^2 + 3 e dist2
      a frame sum of n terms through ceil(P / LANES) + 6 + 15 additions per path:  sum of the terms' bounds + (depth + 1) e sum |term|
      W likewise;  loss = T / W:  relative errors of both plus F additions each and the division
      a gradient term ((gs w) b) r:  |gs w| (db |r| + |b| dr) + (3 e + d_gs) |term|,  d_gs = relative error of gs;  summed over a vertex's n
      terms:  + n e sum |term|."""
    e = EPS32
    v = np.asarray(verts, F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F_, P = t64["wt"].shape
    tri = f[np.where(t64["usable"], np.asarray(face, np.int64), 0)]
    rows = np.arange(F_)[:, None]
    a, b, c = v[rows, tri[..., 0]], v[rows, tri[..., 1]], v[rows, tri[..., 2]]
    q = np.asarray(points, F64)
    edges = np.stack([np.linalg.norm(b - a, axis=-1), np.linalg.norm(c - b, axis=-1), np.linalg.norm(a - c, axis=-1)], -1)
    L, Lmin = edges.max(-1), edges.min(-1)
    R = np.stack([np.linalg.norm(q - a, axis=-1), np.linalg.norm(q - b, axis=-1), np.linalg.norm(q - c, axis=-1)], -1).max(-1)
    M = np.maximum(np.abs(q).max(-1), np.maximum(np.abs(a).max(-1), np.maximum(np.abs(b).max(-1), np.abs(c).max(-1))))
    area4 = (np.cross(b - a, c - a) ** 2).sum(-1)
    C = 128.0
    with np.errstate(divide="ignore", invalid="ignore"):
        dvw = C * e * np.maximum((L * R) ** 2 / area4, L * R / Lmin ** 2)
    d_bary = np.stack([2 * dvw + 2 * e, dvw, dvw], -1)
    d_resid = L * 2 * dvw + 6 * e * M
    rn = np.linalg.norm(t64["resid"], axis=-1)
    d_d2 = 2 * rn * d_resid + d_resid ** 2 + 3 * e * np.where(t64["usable"], t64["dist2"], 0)
    depth = -(-P // LANES) + 6 + 15 + 1
    inl, wt = t64["inlier"], t64["wt"]
    term = np.where(inl, wt * np.where(inl, t64["dist2"], 0), 0)
    d_sums = np.stack([np.where(inl, wt * d_d2 + e * term, 0).sum(1) + depth * e * term.sum(1), depth * e * np.where(inl, wt, 0).sum(1),
                       depth * e * wt.sum(1)], -1)
    W, T = float(t64["W"]), float(t64["sums"][:, 0].sum())
    d_W, d_T = d_sums[:, 2].sum() + F_ * e * W, d_sums[:, 0].sum() + F_ * e * T
    d_loss = (d_T / W + T * d_W / W ** 2 + e * T / W) if W > 0 else 0.0
    gs = abs(2.0 * grad_out / W) if W > 0 else 0.0
    d_gs_rel = (d_W / W + 2 * e) if W > 0 else 0.0
    d_gv = np.zeros((F_, num_verts, 3))
    for fr in range(F_):
        n = int(t64["count"][fr])
        k = keys[fr, :n].astype(np.int64)
        kf, ki = k >> INDEX_BITS, k & (MAX_POINTS - 1)
        i3, corner, vert = np.repeat(ki, 3), np.tile(np.arange(3), n), f[kf].reshape(-1)
        w_, b_, r_ = t64["wt"][fr, i3], np.abs(t64["bary"][fr, i3, corner]), np.abs(t64["resid"][fr, i3])
        mag = (gs * w_ * b_)[:, None] * r_
        bound = (gs * w_)[:, None] * (d_bary[fr, i3, corner][:, None] * r_ + b_[:, None] * d_resid[fr, i3][:, None]) + (3 * e + d_gs_rel) * mag
        tot, cnt = np.zeros((num_verts, 3)), np.zeros(num_verts)
        np.add.at(d_gv[fr], vert, bound)
        np.add.at(tot, vert, mag)
        np.add.at(cnt, vert, 1.0)
        d_gv[fr] += cnt[:, None] * e * tot
    d_gp = np.where(inl[..., None], (gs * wt)[..., None] * d_resid[..., None] + (2 * e + d_gs_rel) * np.abs((gs * wt)[..., None] * t64["resid"]), 0)
    return dict(bary=d_bary, resid=d_resid, dist2=d_d2, sums=d_sums, W=d_W, loss=d_loss, grad_verts=d_gv, grad_points=d_gp)


# ------------------------------------------------------------------------------------------------------------------------------ scenes
def fit_scene(name, P=300, seed=0):
    """The garment mesh of PT.scene(name) (195 vertices, 360 faces, F = 3) and P query points per frame: points scattered around a third of
    the faces (a random interior point moved along the face normal by N(0, 0.01) and by N(0, 0.004) per coordinate), the last P // 8 + 2 of them
    around and beyond the rims (their face's first edge midpoint pushed outward along the cylinder's axis), weights in {0, 0.5, 1, 2}.
    corner_points() gives the points past corners that the tests append so that every part occurs."""
    s = PT.scene(name)
    rng = np.random.default_rng(1000 + seed)
    v, f = s["garment_v"].astype(F64), s["garment_faces"].astype(np.int64)
    F_, nf = len(v), len(f)
    some = rng.choice(nf, nf // 3, replace=False)
    pts = np.zeros((F_, P, 3))
    for fr in range(F_):
        g = some[rng.integers(0, len(some), P)]
        bc = rng.dirichlet([1.0, 1.0, 1.0], P)
        tri = v[fr][f[g]]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
        pts[fr] = (bc[:, :, None] * tri).sum(1) + n * rng.normal(0.0, 0.01, (P, 1)) + rng.normal(0.0, 0.004, (P, 3))
        far = P // 8 + 2 if P >= 8 else 0
        if far:
            y = v[fr][:, 1]
            top = rng.random(far) < 0.5
            rim = np.where(top, y.max(), y.min())
            pick = rng.integers(0, v.shape[1], far)
            pts[fr, P - far:] = v[fr][pick] * np.array([1.0, 0.0, 1.0]) + np.stack([np.zeros(far), rim + np.where(top, 1, -1) * rng.uniform(0.01, 0.06, far),
                                                                                  np.zeros(far)], 1) + rng.normal(0.0, 0.004, (far, 3))
    weights = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], F32), (F_, P), p=[0.2, 0.2, 0.4, 0.2])
    return dict(points=pts.astype(F32), verts=s["garment_v"].astype(F32), faces=s["garment_faces"].astype(np.int32), weights=weights)


def corner_points(verts, faces, per_part=4, seed=0):
    """Points whose closest feature is a corner of their nearest face, per_part of them for each of the parts 4, 5, 6 (vertex a, b, c) and frame
    where that many exist: (F, 3 * per_part, 3) float32, the shortfall filled with the frame's first pick.  Candidates: every vertex pushed
    0.03 along its normal, either way (the mesh is bumpy: a vertex that sticks out owns a cone of space), and points below the rim next to
    vertex 0, the one vertex that is corner a of its first face (PT.scene does the same).  Which corner a vertex is of the face that wins
    the tie among its faces is decided by the float32 search, so the candidates are sorted by PT's float32 twin of it."""
    rng = np.random.default_rng(2000 + seed)
    v, f = np.asarray(verts, F32), np.asarray(faces, np.int64)
    out = []
    for fr in range(len(v)):
        n = PT.vertex_normals_area(v[fr].astype(F64), f)
        cand = np.concatenate([v[fr] + 0.03 * n, v[fr] - 0.03 * n, v[fr][:1] + np.array([0.05, -0.05, 0.0]) + rng.normal(0.0, 0.002, (12, 3))]).astype(F32)
        near = PT.nearest_on_mesh(cand, v[fr], f, F32)
        near64 = PT.nearest_on_mesh(cand, v[fr], f, F64)
        safe = PT.safe_to_compare(near64) & (near64["part"] >= 4)
        rows = []
        for part in (4, 5, 6):
            pick = np.nonzero(safe & (near["part"] == part))[0][:per_part]
            rows.append(cand[pick])
        got = np.concatenate(rows)
        fill = np.repeat(got[:1] if len(got) else cand[:1], 3 * per_part - len(got), 0)
        out.append(np.concatenate([got, fill]))
    return np.stack(out).astype(F32)


_search_cache = {}


def search(points, verts, faces, dtype=F64, key=None):
    """PT.nearest_on_mesh frame by frame (a list of dicts), cached under `key` when one is given."""
    k = (key, np.dtype(dtype).name)
    if key is None or k not in _search_cache:
        res = [PT.nearest_on_mesh(points[f], verts[f], faces, dtype) for f in range(len(points))]
        if key is None:
            return res
        _search_cache[k] = res
    return _search_cache[k]

"""numpy restatement of include/g4d_depth.h (test infrastructure; the package never imports it).  Everything takes a dtype: np.float32 replays the
header's operations in the header's order, one rounded operation per sign, so the kernels can be compared bit for bit -- the tree sums of the
forward and the per-vertex order of the gradient included --; np.float64 is the same mathematics in double, the reference the central differences
are taken on.  Projection and coverage come from tests/render_twin.py (include/g4d_render.h)."""
import math

import numpy as np

import render_twin as RT

F32, F64, I64 = np.float32, np.float64, np.int64
LANES, PER_LANE, WAVE = 256, 4, 64
CHUNK = LANES * PER_LANE
MAX_CAMS, MAX_SIDE, MAX_FACES = 8, 4096, 715827882
COORD_LIMIT = 1 << 22


# ------------------------------------------------------------------------------------------------------------------------------ cameras, scenes
def look_at(distance, elevation, azimuth, half_angle=30.0, near=0.1):
    """(eye, at, up, half_angle, near) of render.look_at_camera -- the fields of render.Camera, in its order."""
    el, az = math.radians(elevation), math.radians(azimuth)
    return ((distance * math.cos(el) * math.sin(az), distance * math.sin(el), -distance * math.cos(el) * math.cos(az)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0),
            float(half_angle), float(near))


def camera_constants(cameras, w, h):
    """Per camera RT.camera's dict (R, eye, s, hh, hw as fp32) -- R and s are what cams_host carries."""
    return [RT.camera(c[0], c[1], c[2], c[3], w, h, 1) for c in cameras]


def cams_host(consts):
    return np.stack([np.concatenate([k["R"].reshape(9), [k["s"]]]).astype(F32) for k in consts])


def bent_grid(rows=8, cols=8, frames=2, seed=0, size=0.45, bend=0.12, jitter=0.01):
    """A bent grid of rows x cols vertices facing +z (2 (rows - 1) (cols - 1) faces: 98 for 8 x 8), one pose per frame: verts (F,V,3) fp32,
    faces (nf,3) int32 with alternating diagonals."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-size, size, rows), np.linspace(-size, size, cols), indexing="ij")
    verts = []
    for f in range(frames):
        z = bend * np.cos(2.5 * x + 0.4 * f) * np.cos(1.5 * y - 0.3 * f) + 0.03 * f
        verts.append(np.stack([x, y, z], -1).reshape(-1, 3) + jitter * rng.standard_normal((rows * cols, 3)))
    faces = []
    for r in range(rows - 1):
        for c in range(cols - 1):
            a, b, d, e = r * cols + c, r * cols + c + 1, (r + 1) * cols + c, (r + 1) * cols + c + 1
            faces += [[a, b, e], [a, e, d]] if (r + c) % 2 == 0 else [[a, b, d], [b, e, d]]
    return np.asarray(verts, F32), np.asarray(faces, np.int32)


FRONT = (look_at(1.5, 0.0, 160.0), look_at(1.5, 10.0, 205.0))   # two cameras in front of bent_grid (azimuth 180 looks down -z)


def project(verts, consts, near=0.1):
    """verts (F,V,3) fp32 under every camera: px, py (K,F,V) int32, invz (K,F,V), cam (K,F,V,3) fp32, as g4d_render_project_f32 gives them."""
    out = [RT.project_f32(verts, k, near) for k in consts]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def rasterize(px, py, invz, faces, w, h):
    """face_id (K,F,h,w) int32 and depth (K,F,h,w) fp32 (+inf on the background) of g4d_render_raster at ss = 1."""
    K, F_ = px.shape[:2]
    ids, depth = np.zeros((K, F_, h, w), np.int32), np.zeros((K, F_, h, w), F32)
    for c in range(K):
        for f in range(F_):
            r = RT.raster(px[c, f], py[c, f], invz[c, f], faces, w, h, shade=False)
            ids[c, f], depth[c, f] = r["face_id"], r["depth"]
    return ids, depth


def world_to_cam64(verts, consts):
    """cam = R_c (v - eye_c) in float64 from the fp32-rounded camera constants: (K,F,V,3)."""
    v = np.asarray(verts, F64)
    return np.stack([(v - k["eye"].astype(F64)) @ k["R"].astype(F64).T for k in consts])


# ------------------------------------------------------------------------------------------------------------------------------- one sample
def sample_terms(camc, faces, face_id, depth_obs, weights, labels_obs, face_labels, s, trunc, grazing, dt, inlier=None):
    """One (camera, frame): camc (V,3), face_id, depth_obs (h,w) [, weights, labels_obs (h,w), face_labels (nf)] -> dict of (h,w) arrays in dtype
    dt: observed, associated, facing, inlier, wt, r, z, den, n (h,w,3), b (h,w,3).  inlier: hold this inlier set instead of deciding it."""
    h, w = face_id.shape
    nf, V = len(faces), len(camc)
    camc = np.asarray(camc, dt)
    D = np.asarray(depth_obs, dt)
    wt = np.ones((h, w), dt) if weights is None else np.asarray(weights, dt)
    with np.errstate(invalid="ignore"):
        observed = (D > 0) & (D < np.inf)
    g = np.asarray(face_id, I64)
    has = (g >= 0) & (g < nf)
    gs = np.where(has, g, 0)
    fv = np.asarray(faces, I64).reshape(-1, 3)[gs] if nf else np.zeros((h, w, 3), I64)
    valid = has & ((fv >= 0) & (fv < V)).all(-1)
    fv = np.where(valid[..., None], fv, 0)
    assoc = observed & valid
    if labels_obs is not None and nf:
        assoc &= np.asarray(face_labels)[gs] == np.asarray(labels_obs)
    hh, hw = 128 * h, 128 * w
    shh = dt(s) * dt(hh)
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    dx = (256 * j + 128 - hw).astype(dt) / shh
    dy = (hh - (256 * i + 128)).astype(dt) / shh
    if V == 0:
        camc = np.zeros((1, 3), dt)
    c0, c1, c2 = camc[fv[..., 0]], camc[fv[..., 1]], camc[fv[..., 2]]
    with np.errstate(all="ignore"):
        u, v = c1 - c0, c2 - c0
        cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                       a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
        dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        n = cross(u, v)
        den = (n[..., 0] * dx + n[..., 1] * dy) + n[..., 2]
        nn = dot(n, n)
        dd = (dx * dx + dy * dy) + dt(1)
        g2 = dt(F32(grazing)) * dt(F32(grazing))
        facing = den * den > (g2 * nn) * dd
        z = dot(n, c0) / den
        r = z - D
        tr = dt(np.inf) if trunc is None else dt(F32(trunc))
        decided = (wt > 0) & assoc & facing & (np.abs(r) < tr)
        inl = decided if inlier is None else np.asarray(inlier, bool)
        q = np.stack([z * dx - c0[..., 0], z * dy - c0[..., 1], z - c0[..., 2]], -1)
        b1 = dot(cross(q, v), n) / nn
        b2 = dot(cross(u, q), n) / nn
        b = np.stack([(dt(1) - b1) - b2, b1, b2], -1)
        margin = np.where(assoc & (nn > 0), np.abs(den) / np.sqrt(nn * dd), np.nan)    # |cosine| between ray and normal
    return dict(observed=observed, associated=assoc, facing=facing, inlier=inl, decided=decided, wt=wt, r=r, z=z, den=den, n=n, b=b, cosine=margin)


# ---------------------------------------------------------------------------------------------------------------------------------- tree sums
def block_sum(lanes):
    """(..., 256) lane values -> (...): the xor butterfly within every run of 64 lanes, then the four runs left to right (csrc/reduce.h)."""
    w = lanes.reshape(lanes.shape[:-1] + (LANES // WAVE, WAVE))
    idx = np.arange(WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        w = w + w[..., idx ^ m]
    s = w[..., 0, 0]
    for k in range(1, LANES // WAVE):
        s = s + w[..., k, 0]
    return s


def chunk_sums(x):
    """(samples) terms of one frame in scan order -> (nchunks) chunk sums."""
    n = -(-len(x) // CHUNK)
    pad = np.zeros(n * CHUNK, x.dtype)
    pad[:len(x)] = x
    pad = pad.reshape(n, PER_LANE, LANES)
    acc = np.zeros((n, LANES), x.dtype)
    for q in range(PER_LANE):
        acc = acc + pad[:, q]
    return block_sum(acc)


def frame_sum(parts):
    """(nchunks) chunk sums -> the frame's sum: lane t adds chunks t, t + 256, ... ascending, then the tree."""
    n = -(-len(parts) // LANES)
    pad = np.zeros(n * LANES, parts.dtype)
    pad[:len(parts)] = parts
    acc = np.zeros(LANES, parts.dtype)
    for k in range(n):
        acc = acc + pad[k * LANES:(k + 1) * LANES]
    return block_sum(acc)


def tree(x):
    return frame_sum(chunk_sums(x))


# ----------------------------------------------------------------------------------------------------------------------------------- forward
def forward(cam, faces, face_id, depth_obs, consts, weights=None, labels_obs=None, face_labels=None, trunc=None, grazing=0.1, dt=F32, inlier=None):
    """g4d_depth_fit_terms_f32: cam (K,F,V,3), face_id, depth_obs [, weights, labels_obs] (K,F,h,w) -> dict: per-sample arrays (K,F,h,w[,3]) as
    sample_terms names them, resid (NaN where no inlier), sums (F,3), count (F) int32, W, loss."""
    K, F_, h, w = face_id.shape
    per = [[sample_terms(cam[c, f], faces, face_id[c, f], depth_obs[c, f], None if weights is None else weights[c, f],
                         None if labels_obs is None else labels_obs[c, f], face_labels, consts[c]["s"], trunc, grazing, dt,
                         None if inlier is None else inlier[c, f]) for f in range(F_)] for c in range(K)]
    out = {k: np.stack([np.stack([per[c][f][k] for f in range(F_)]) for c in range(K)]) for k in per[0][0]} if K and F_ else {}
    sums, count = np.zeros((F_, 3), dt), np.zeros(F_, np.int32)
    for f in range(F_):
        inl, wt, r, obs = (out[k][:, f].reshape(-1) for k in ("inlier", "wt", "r", "observed"))
        with np.errstate(all="ignore"):
            sums[f, 0] = tree(np.where(inl, wt * (r * r), dt(0)).astype(dt))
        sums[f, 1] = tree(np.where(inl, wt, dt(0)).astype(dt))
        sums[f, 2] = tree(np.where(obs, wt, dt(0)).astype(dt))
        count[f] = inl.sum()
    W, T = dt(0), dt(0)
    for f in range(F_):
        T = T + sums[f, 0]
        W = W + sums[f, 2]
    out.update(sums=sums, count=count, W=W, loss=(T / W if W > 0 else dt(0)), resid=np.where(out["inlier"], out["r"], dt(np.nan)).astype(dt))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------- gradient
def vertex_corners(faces, V):
    """mesh_tables.vertex_corners: (rowptr (V + 1), entries face * 3 + corner ascending per vertex)."""
    flat = np.asarray(faces, I64).reshape(-1)
    rowptr = np.zeros(V + 1, I64)
    np.cumsum(np.bincount(flat, minlength=V), out=rowptr[1:])
    return rowptr, np.argsort(flat, kind="stable")


def face_boxes(px, py, invz, faces, w, h):
    """One (camera, frame): per face (j0, j1, i0, i1), the sample box of g4d_render.h cut to the image, or None for a face the rasterizer drops."""
    x, y, iz = np.asarray(px, I64)[faces], np.asarray(py, I64)[faces], np.asarray(invz, F32)[faces]
    out = []
    for k in range(len(faces)):
        with np.errstate(invalid="ignore"):
            ok = ((iz[k] > 0) & (iz[k] < np.inf)).all() and (np.abs(x[k]) < COORD_LIMIT).all() and (np.abs(y[k]) < COORD_LIMIT).all()
        if not ok or (x[k, 1] - x[k, 0]) * (y[k, 2] - y[k, 0]) - (x[k, 2] - x[k, 0]) * (y[k, 1] - y[k, 0]) == 0:
            out.append(None)
            continue
        out.append((max(int((x[k].min() - 128 + 255) >> 8), 0), min(int((x[k].max() - 128) >> 8), w - 1),
                    max(int((y[k].min() - 128 + 255) >> 8), 0), min(int((y[k].max() - 128) >> 8), h - 1)))
    return out


def gradient(t, px, py, invz, faces, face_id, consts, V, grad_out=1.0, dt=F32):
    """g4d_depth_fit_vertex_grad_f32 from a forward's dict t: (F,V,3) in dtype dt, the header's order of summation."""
    K, F_, h, w = face_id.shape
    faces = np.asarray(faces, I64).reshape(-1, 3)
    rowptr, entries = vertex_corners(faces, V)
    W = t["W"]
    gs = (dt(2) * dt(F32(grad_out))) / W if W > 0 else dt(0)
    out = np.zeros((F_, V, 3), dt)
    R = [k["R"].astype(dt) for k in consts]
    for f in range(F_):
        boxes = [face_boxes(px[c, f], py[c, f], invz[c, f], faces, w, h) for c in range(K)]
        for vi in range(V):
            acc = np.zeros(3, dt)
            for c in range(K):
                a = np.zeros(3, dt)
                for e in entries[rowptr[vi]:rowptr[vi + 1]]:
                    face, corner = int(e) // 3, int(e) % 3
                    box = boxes[c][face]
                    if box is None:
                        continue
                    j0, j1, i0, i1 = box
                    for i in range(i0, i1 + 1):
                        for j in range(j0, j1 + 1):
                            if face_id[c, f, i, j] != face or not t["inlier"][c, f, i, j]:
                                continue
                            g = (((gs * t["wt"][c, f, i, j]) * t["r"][c, f, i, j]) * t["b"][c, f, i, j, corner]) / t["den"][c, f, i, j]
                            a = a + g * t["n"][c, f, i, j]
                for k in range(3):
                    acc[k] = acc[k] + ((R[c][0, k] * a[0] + R[c][1, k] * a[1]) + R[c][2, k] * a[2])
            out[f, vi] = acc
    return out

"""numpy restatement of include/g4d_scan.h (test infrastructure; the package never imports it), on top of tests/render_twin.py, whose
orientation and projection it uses.  Written from the header:

  - exact hit ranks: the samples of a frame whose face id is in [0, nf), in ascending s = (c h + i) w + j;
  - the selection of exactly N of M hits, forward (point j -> rank) and in the per-hit form the kernel evaluates (rank -> its points);
  - the unprojection as an fp32 replay: the header's operations in the header's order on np.float32, so the kernels can be compared bit for bit;
  - the same in float64 with a bound on |fp32 - float64| from the header's operation counts, in render_twin's manner (u = 2^-24 per rounded
    operation, gamma(n) for n in sequence, SLOP for second-order terms), and a bound on how far a point can project from its sample centre.
    Nothing here is measured.
"""
import numpy as np

import render_twin as RT
from render_twin import F32, F64, I64, SLOP, U, gamma

MAX_CAMS = 8


# ---------------------------------------------------------------------------------------------------------------------------- selection
def mix(x):
    """The header's 32-bit mixer on uint64 arrays holding uint32 values."""
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x, np.uint64) & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def key(seed, f, j):
    return mix(mix(mix(np.uint64(seed & 0xFFFFFFFF)) ^ np.uint64(f)) ^ np.asarray(j, np.uint64))


def select_forward(M, N, seed, f):
    """Point j -> the rank of its hit, (N) int64; -1 everywhere when M == 0."""
    j = np.arange(N, dtype=I64)
    if M == 0:
        return np.full(N, -1, I64)
    if M < N:
        return j % M
    lo, hi = j * M // N, (j + 1) * M // N
    return lo + (key(seed, f, j) % (hi - lo).astype(np.uint64)).astype(I64)


def select_per_hit(M, N, seed, f):
    """The same from the hits' side: every rank r decides alone which points it writes.  Returns (ranks (N) int64, writes (N) int64: how many
    hits wrote each point -- 1 everywhere if the rule inverts the forward form; 0 everywhere for M == 0, where the fill is not a hit's)."""
    out, writes = np.full(N, -1, I64), np.zeros(N, I64)
    r = np.arange(M, dtype=I64)
    if M >= N > 0:
        j = ((r + 1) * N - 1) // M
        lo, hi = j * M // N, (j + 1) * M // N
        sel = lo + (key(seed, f, j) % (hi - lo).astype(np.uint64)).astype(I64) == r
        np.add.at(writes, j[sel], 1)
        out[j[sel]] = r[sel]
    else:
        for rr in r:
            mine = np.arange(rr, N, M)
            writes[mine] += 1
            out[mine] = rr
    return out, writes


# ------------------------------------------------------------------------------------------------------------------------- unprojection
def _project64(p, cam):
    """(.., 3) float64 world points -> (fx, fy) float64 in 1/256 sample, by the formula of g4d_render_project_f32 on the fp32 camera constants."""
    R, e, s, hh, hw = cam["R"].astype(F64), cam["eye"].astype(F64), F64(cam["s"]), F64(cam["hh"]), F64(cam["hw"])
    c = (p - e) @ R.T
    q = 1.0 / c[..., 2]
    return c[..., 0] * q * s * hh + hw, hh - c[..., 1] * q * s * hh


def scan_frame(px, py, invz, face_id, verts, faces, n_points, seed, f, face_labels=None, cams=None):
    """One frame of g4d_scan_points_f32.  px, py (K,V) ints, invz (K,V) fp32, face_id (K,h,w) ints, verts (V,3) fp32, faces (nf,3).
    Returns a dict: points (N,3) fp32 replay, labels, face, sample (N) int32, count;
      points64 (N,3) and err (N,3): the float64 unprojection and the bound on |points - points64|;  inside (N) bool: all three b_k >= 0;
      with cams (the K dicts of render_twin.camera): centre (N,2) = the points' sample centres in 1/256 sample, reproj (N,2) = where points64
      project in float64, err_reproj (N) = the bound on |reproj - centre| per axis for the points that are `inside`.

    fp32 - float64, per coordinate c (the rule is render_twin._shade's vertex-colour rule, so is the count):
      b_k = fl(E_k) / fl(area2), E exact: 3 roundings;  w_k = b_k iz_k: 4;  ((w0 c0 + w1 c1) + w2 c2): <= 7 per term -> gamma(7) sum |w_k c_k|;
      iz = (iz0 + b1 (iz1 - iz0)) + b2 (iz2 - iz0): <= 6 per term -> err iz <= gamma(6) (|iz0| + |b1 (iz1 - iz0)| + |b2 (iz2 - iz0)|);
      p = sum / iz:  |err p| <= gamma(7) sum |w_k c_k| / iz + |p| err iz / iz + u |p|.
    reprojection: with true depths z_k, true screen positions X_k of the vertices and iz_k = (1 + d_k) / z_k (|d_k| <= rel_q of
      render_twin.project_f64), the point sum_k (b_k iz_k) v_k / sum_k b_k iz_k projects to sum_k m_k X_k, m_k = b_k (1 + d_k) / sum_j b_j (1 + d_j),
      while its sample centre is sum_k b_k x_k exactly (x_k the snapped integers; sum b_k = 1).  For b >= 0:
      |reproj - centre| <= max_k |X_k - x_k| + sum_k |m_k - b_k| max_k |x_k - centre| <= (0.5 + max err_fx) + 2 d / (1 - d) max_k |x_k - centre|:
      half a unit from the snap, the fp32 projection's own error, and the depth rounding times the triangle's reach."""
    px, py, invz, ids = np.asarray(px, I64), np.asarray(py, I64), np.asarray(invz, F32), np.asarray(face_id, I64)
    verts32, faces = np.asarray(verts, F32), np.asarray(faces, I64).reshape(-1, 3)
    K, h, w = ids.shape
    N, nf = int(n_points), len(faces)
    flat = ids.reshape(-1)
    hits = np.nonzero((flat >= 0) & (flat < nf))[0]                   # ascending s: the rank of hits[r] is r
    M = len(hits)
    out = dict(points=np.zeros((N, 3), F32), labels=np.full(N, -1, np.int32), face=np.full(N, -1, np.int32), sample=np.full(N, -1, np.int32),
               count=M, points64=np.zeros((N, 3)), err=np.zeros((N, 3)), inside=np.zeros(N, bool), centre=np.zeros((N, 2)), reproj=np.zeros((N, 2)),
               err_reproj=np.zeros(N))
    if M == 0 or N == 0:
        return out
    s = hits[select_forward(M, N, seed, f)]
    c, rest = s // (h * w), s % (h * w)
    i, j = rest // w, rest % w
    g = flat[s]
    o = [RT.orient(px[k], py[k], invz[k], faces, nverts=len(verts32)) for k in range(K)]
    pick = lambda name: np.stack([o[k][name] for k in range(K)])[c, g]
    drawn, x, y, iz, vid, area2 = (pick(n) for n in ("drawn", "x", "y", "iz", "vid", "area2"))
    sx, sy = 256 * j + 128, 256 * i + 128
    E = []
    for e in range(3):
        p, q = (e + 1) % 3, (e + 2) % 3
        E.append((x[:, q] - x[:, p]) * (sy - y[:, p]) - (y[:, q] - y[:, p]) * (sx - x[:, p]))
    a2 = np.where(drawn, area2, 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        b32 = [E[e].astype(F32) / a2.astype(F32) for e in range(3)]
        w32 = [b32[e] * iz[:, e] for e in range(3)]
        iz32 = (iz[:, 0] + b32[1] * (iz[:, 1] - iz[:, 0])) + b32[2] * (iz[:, 2] - iz[:, 0])
        v = verts32[vid]                                              # (N, 3 vertices, 3 coordinates)
        p32 = ((w32[0][:, None] * v[:, 0] + w32[1][:, None] * v[:, 1]) + w32[2][:, None] * v[:, 2]) / iz32[:, None]
        b64 = [E[e].astype(F64) / a2.astype(F64) for e in range(3)]
        zd, vd = iz.astype(F64), v.astype(F64)
        w64 = [b64[e] * zd[:, e] for e in range(3)]
        iz64 = (zd[:, 0] + b64[1] * (zd[:, 1] - zd[:, 0])) + b64[2] * (zd[:, 2] - zd[:, 0])
        p64 = ((w64[0][:, None] * vd[:, 0] + w64[1][:, None] * vd[:, 1]) + w64[2][:, None] * vd[:, 2]) / iz64[:, None]
        e_iz = SLOP * gamma(6) * (np.abs(zd[:, 0]) + np.abs(b64[1] * (zd[:, 1] - zd[:, 0])) + np.abs(b64[2] * (zd[:, 2] - zd[:, 0])))
        mag = sum(np.abs(w64[e])[:, None] * np.abs(vd[:, e]) for e in range(3))
        err = SLOP * (gamma(7) * mag / np.abs(iz64)[:, None] + np.abs(p64) * (e_iz / np.abs(iz64))[:, None] + U * np.abs(p64))
    d3 = drawn[:, None]
    out.update(points=np.where(d3, p32, F32(0)).astype(F32), points64=np.where(d3, p64, 0.0), err=np.where(d3, err, 0.0),
               labels=np.where(drawn, 0 if face_labels is None else np.asarray(face_labels, np.int32)[g], -1).astype(np.int32),
               face=np.where(drawn, g, -1).astype(np.int32), sample=np.where(drawn, s, -1).astype(np.int32),
               inside=drawn & (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0), centre=np.stack([sx, sy], 1).astype(F64))
    if cams is not None:
        reproj, bound = np.zeros((N, 2)), np.zeros(N)
        for k in range(K):
            sel = np.nonzero((c == k) & drawn)[0]
            if not len(sel):
                continue
            _, _, q, efx, efy, eq = RT.project_f64(verts32, cams[k])
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = (eq / np.abs(q))[vid[sel]].max(1)                                               # d: the largest of the three vertices'
            snap = 0.5 + np.maximum(efx, efy)[vid[sel]].max(1)
            reach = np.maximum(np.abs(x[sel] - sx[sel, None]), np.abs(y[sel] - sy[sel, None])).max(1)
            bound[sel] = SLOP * (snap + 2 * rel / (1 - rel) * reach) + 1e-9                           # (+ the float64 evaluation itself)
            reproj[sel] = np.stack(_project64(out["points64"][sel], cams[k]), 1)
        out.update(reproj=reproj, err_reproj=bound)
    return out


def scan(px, py, invz, face_id, verts, faces, n_points, seed, face_labels=None, cams=None):
    """All frames: px, py, invz (K,F,V), face_id (K,F,h,w), verts (F,V,3) -> the dict of scan_frame with a leading frame axis on every entry."""
    frames = [scan_frame(np.asarray(px)[:, f], np.asarray(py)[:, f], np.asarray(invz)[:, f], np.asarray(face_id)[:, f], np.asarray(verts)[f], faces,
                         n_points, seed, f, face_labels, cams) for f in range(np.asarray(verts).shape[0])]
    return {k: np.stack([fr[k] for fr in frames]) for k in frames[0]}

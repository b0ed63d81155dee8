"""numpy restatement of include/g4d_render.h (test infrastructure; the package never imports it).  Three parts, all written from the header:

  - integer coverage: orientation, the three edge functions and the top-left rule in int64, one face at a time over its own sample box
    (no tiles, no chunks, no compaction: the kernel's binning has nothing to correspond to here);
  - an fp32 replay of the projection, the depth and the shading: the header's operations in the header's order on np.float32, so the
    kernels can be compared bit for bit;
  - the same in float64, with bounds on |fp32 - float64| from the header's operation counts: u = 2^-24 per rounded operation,
    gamma(n) = n u / (1 - n u) for n of them in sequence (Higham, Accuracy and Stability of Numerical Algorithms, 3.1), second-order products
    of such terms covered by the factor SLOP.  Nothing here is measured.
"""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
U = 2.0 ** -24
SLOP = 1.001          # (1 + gamma(8))^2 - 1 < 1e-6: covers every product of two error terms below with a wide margin
COORD_LIMIT = 1 << 22
NO_COORD = 1 << 30


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------------------------------------- camera
def camera(eye, at, up, half_angle_deg, w, h, ss):
    """The host part of g4d_render_project_f32: the look-at basis in float64, rounded to fp32.  The entry point takes fp32 arguments."""
    eye, at, up = (np.asarray(a, F32).astype(F64) for a in (eye, at, up))

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    def unit(a):
        return a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    z = unit(at - eye)
    x = unit(cross(up, z))
    y = unit(cross(z, x))
    s = 1.0 / np.tan(F64(F32(half_angle_deg)) * (np.pi / 180.0))
    return dict(R=np.stack([x, y, z]).astype(F32), eye=eye.astype(F32), s=F32(s), hh=F32(128 * ss * h), hw=F32(128 * ss * w))


def light_in_camera(cam, light_world):
    """A world-space direction in camera space, as fp32 (what the Python layer hands to g4d_render_raster)."""
    return (cam["R"].astype(F64) @ np.asarray(light_world, F64)).astype(F32)


# --------------------------------------------------------------------------------------------------------------------------- projection
def project_f32(verts, cam, near):
    """verts (..., 3) fp32 -> px, py int32, invz fp32, cam-space positions fp32: the header's operations in its order."""
    v = np.asarray(verts, F32)
    R, e, s, hh, hw = cam["R"], cam["eye"], cam["s"], cam["hh"], cam["hw"]
    d = [v[..., k] - e[k] for k in range(3)]
    c = [(R[k, 0] * d[0] + R[k, 1] * d[1]) + R[k, 2] * d[2] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = F32(1) / c[2]
        fx = ((c[0] * q) * s) * hh + hw
        fy = hh - ((c[1] * q) * s) * hh

        def snap(f):
            ok = np.abs(f) < F32(2.0 ** 30)
            return np.where(ok, np.rint(np.where(ok, f, 0)), NO_COORD).astype(np.int32)
        return snap(fx), snap(fy), np.where(c[2] >= F32(near), q, F32(0)).astype(F32), np.stack(c, -1)


def project_f64(verts, cam):
    """The same formula in float64 on the same fp32 inputs and fp32 camera constants -> fx, fy (unrounded, 1/256 sample), q = 1 / z,
    and bounds (err_fx, err_fy, err_q) on what project_f32's fx, fy (before the snap) and q can differ by.

    d_j = v_j - e_j: 1 rounding.  cam_k = (R0 d0 + R1 d1) + R2 d2: each term passes <= 4 roundings (subtraction, product, two sums)
      -> |err cam_k| <= gamma(4) A_k, A_k = sum_j |R_kj d_j|.
    q = 1 / cam_z: rel(q) <= (rel(cam_z) + u) / (1 - rel(cam_z)), rel(cam_z) = gamma(4) A_z / |cam_z|.
    t = ((cam_x q) s) hh: |err t| <= |q s hh| err(cam_x) + |t| (rel(q) + 3 u);   fx = t + hw: + u |fx|."""
    v = np.asarray(verts, F32).astype(F64)
    R, e, s, hh, hw = cam["R"].astype(F64), cam["eye"].astype(F64), F64(cam["s"]), F64(cam["hh"]), F64(cam["hw"])
    d = v - e
    c = d @ R.T
    A = np.abs(d) @ np.abs(R).T
    with np.errstate(divide="ignore", invalid="ignore"):
        q = 1.0 / c[..., 2]
        rel_z = gamma(4) * A[..., 2] / np.abs(c[..., 2])
        rel_q = np.where(rel_z < 1e-3, (rel_z + U) / (1.0 - rel_z), np.inf)
        tx, ty = c[..., 0] * q * s * hh, c[..., 1] * q * s * hh
        fx, fy = tx + hw, hh - ty
        err_fx = SLOP * (np.abs(q * s * hh) * gamma(4) * A[..., 0] + np.abs(tx) * (rel_q + 3 * U) + U * np.abs(fx))
        err_fy = SLOP * (np.abs(q * s * hh) * gamma(4) * A[..., 1] + np.abs(ty) * (rel_q + 3 * U) + U * np.abs(fy))
    return fx, fy, q, err_fx, err_fy, np.abs(q) * rel_q


# ----------------------------------------------------------------------------------------------------------------------------- coverage
def orient(px, py, invz, faces, nverts=None):
    """One frame: px, py (V) ints, invz (V) fp32, faces (nf, 3) -> dict of the ORIENTED faces: vid (nf, 3), x, y (nf, 3) int64, iz (nf, 3) fp32,
    area2 (nf) int64 (0 where the face is dropped), drawn (nf) bool."""
    px, py, invz, f = np.asarray(px, I64), np.asarray(py, I64), np.asarray(invz, F32), np.asarray(faces, I64).reshape(-1, 3)
    V = len(px) if nverts is None else nverts
    valid = ((f >= 0) & (f < V)).all(1)
    fs = np.where(valid[:, None], f, 0)
    x, y, iz = px[fs], py[fs], invz[fs]
    with np.errstate(invalid="ignore"):
        ok = valid & ((iz > 0) & (iz < np.inf)).all(1) & (np.abs(x) < COORD_LIMIT).all(1) & (np.abs(y) < COORD_LIMIT).all(1)
    x, y = np.where(ok[:, None], x, 0), np.where(ok[:, None], y, 0)
    area2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    swap = area2 < 0
    perm = np.where(swap[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    take = lambda a: np.take_along_axis(a, perm, 1)
    area2 = np.abs(area2)
    return dict(vid=take(fs), x=take(x), y=take(y), iz=take(iz), area2=area2, drawn=ok & (area2 > 0), faces_in_order=fs)


def _edge_values(o, k, sx, sy):
    """E_0, E_1, E_2 of oriented face k at the sample centres (sx, sy) (int64 arrays), and which edges own their line."""
    x, y = o["x"][k], o["y"][k]
    E, owns = [], []
    for e in range(3):
        p, q = (e + 1) % 3, (e + 2) % 3
        dx, dy = x[q] - x[p], y[q] - y[p]
        E.append(dx * (sy - y[p]) - dy * (sx - x[p]))
        owns.append(bool(dy < 0 or (dy == 0 and dx > 0)))
    return E, owns


def raster(px, py, invz, faces, ws, hs, ss=1, cam=None, light=(0, 0, 0), ambient=1.0, directional=0.0, face_rgb=None, vert_rgb=None,
           bg=(0, 0, 0), ids=None, shade=True):
    """One frame of g4d_render_raster on ws x hs samples.  Returns a dict:
      face_id (hs, ws) int32, iz (hs, ws) fp32 (0 where background), depth = 1 / iz or +inf, ncover (hs, ws): how many faces cover each sample,
      iz64 / err_iz: the float64 depth of the winning face and the bound on |iz - iz64|,
      image (hs / ss, ws / ss, 3) fp32 replay, image64 and err_image: float64 and the bound on |image - image64| GIVEN these face ids.
    ids: (hs, ws) face ids to shade instead of this function's own winners (to bound a kernel's image given the kernel's ids)."""
    o = orient(px, py, invz, faces)
    nf = len(o["area2"])
    face_id = np.full((hs, ws), -1, np.int32)
    best = np.zeros((hs, ws), F32)
    ncover = np.zeros((hs, ws), np.int32)
    for k in np.nonzero(o["drawn"])[0]:
        i0, i1 = max(-((128 - o["x"][k].min()) // 256), 0), min((o["x"][k].max() - 128) // 256, ws - 1)      # ceil((min - 128) / 256) .. floor(..)
        j0, j1 = max(-((128 - o["y"][k].min()) // 256), 0), min((o["y"][k].max() - 128) // 256, hs - 1)
        if i0 > i1 or j0 > j1:
            continue
        sx, sy = np.meshgrid(256 * np.arange(i0, i1 + 1, dtype=I64) + 128, 256 * np.arange(j0, j1 + 1, dtype=I64) + 128)
        E, owns = _edge_values(o, k, sx, sy)
        cov = np.ones(sx.shape, bool)
        for e in range(3):
            cov &= (E[e] > 0) | ((E[e] == 0) & owns[e])
        if not cov.any():
            continue
        a2 = F32(o["area2"][k])
        b1, b2 = E[1].astype(F32) / a2, E[2].astype(F32) / a2
        z = o["iz"][k]
        iz = (z[0] + b1 * (z[1] - z[0])) + b2 * (z[2] - z[0])
        sub_id, sub_best = face_id[j0:j1 + 1, i0:i1 + 1], best[j0:j1 + 1, i0:i1 + 1]
        win = cov & ((sub_id < 0) | (iz > sub_best))
        sub_id[win] = k
        sub_best[win] = iz[win]
        ncover[j0:j1 + 1, i0:i1 + 1] += cov
    with np.errstate(divide="ignore"):
        out = dict(face_id=face_id, iz=best, depth=np.where(face_id >= 0, F32(1) / best, F32(np.inf)).astype(F32), ncover=ncover, oriented=o)
    if shade:
        out.update(_shade(o, face_id if ids is None else np.asarray(ids), ws, hs, ss, cam, light, ambient, directional, face_rgb, vert_rgb, bg, nf))
    return out


def face_shades(o_faces, cam, light, ambient, directional):
    """The flat shade of faces (nf, 3) (the caller's vertex order) from cam (V, 3) fp32: (fp32 replay, float64, bound on their difference).

    n_x = u_y w_z - u_z w_y with u, w differences of inputs: each product passes 3 roundings, the subtraction a 4th:
      |err n_k| <= gamma(4) (|.| + |.|) =: en_k.   d = n . c0: |err d| <= sum |c0_k| en_k + gamma(3) sum |n_k c0_k|; where |d| is within that,
      the turn towards the viewer may go either way and the bound is the trivial one, directional * |l| (cosl in [0, |l|]).
    S = sum n_k^2: |err S| <= sum 2 |n_k| en_k + gamma(3) S;  len = sqrt(S): |err| <= err S / (2 len) + u len.
    dot = n . l: |err| <= sum |l_k| en_k + gamma(3) sum |n_k l_k|;  cosl = dot / len: |err| <= err dot / len + |dot| err len / len^2 + u |cosl|;
    max(0, .) does not increase it;  shade = ambient + directional cosl: |err| <= |directional| err cosl + 2 u (|ambient| + |directional cosl|)."""
    f = np.asarray(o_faces, I64).reshape(-1, 3)
    if cam is None:
        one = np.ones(len(f))
        return one.astype(F32), one, np.zeros(len(f))
    c32 = np.asarray(cam, F32)
    l32, amb32, dir32 = np.asarray(light, F32), F32(ambient), F32(directional)

    def run(c, l, amb, dr):
        c0, c1, c2 = c[f[:, 0]], c[f[:, 1]], c[f[:, 2]]
        u, w = c1 - c0, c2 - c0
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        en = np.stack([np.abs(u[:, 1] * w[:, 2]) + np.abs(u[:, 2] * w[:, 1]), np.abs(u[:, 2] * w[:, 0]) + np.abs(u[:, 0] * w[:, 2]),
                       np.abs(u[:, 0] * w[:, 1]) + np.abs(u[:, 1] * w[:, 0])], 1)
        d = (n[:, 0] * c0[:, 0] + n[:, 1] * c0[:, 1]) + n[:, 2] * c0[:, 2]
        n = np.where((d > 0)[:, None], -n, n)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        dot = (n[:, 0] * l[0] + n[:, 1] * l[1]) + n[:, 2] * l[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            cosl = np.where(ln > 0, dot / np.where(ln > 0, ln, 1), 0)
        cosl = np.where(cosl > 0, cosl, 0)
        return amb + dr * cosl, (c0, n, en, d, ln, dot, cosl)
    s32, _ = run(c32, l32, amb32, dir32)
    l, amb, dr = l32.astype(F64), F64(amb32), F64(dir32)
    s64, (c0, n, en, d, ln, dot, cosl) = run(c32.astype(F64), l, amb, dr)
    en = gamma(4) * en
    err_d = (np.abs(c0) * en).sum(1) + gamma(3) * np.abs(n * c0).sum(1)
    S = ln * ln
    err_S = (2 * np.abs(n) * en).sum(1) + gamma(3) * S
    with np.errstate(divide="ignore", invalid="ignore"):
        err_len = err_S / (2 * ln) + U * ln
        err_dot = (np.abs(l) * en).sum(1) + gamma(3) * np.abs(n * l).sum(1)
        err_cos = err_dot / ln + np.abs(dot) * err_len / S + U * np.abs(cosl)
    trivial = np.sqrt((l * l).sum())
    err_cos = np.where((np.abs(d) <= err_d) | ~(err_len < 0.25 * ln) | ~np.isfinite(err_cos), trivial, np.minimum(err_cos, trivial))
    err = SLOP * (np.abs(dr) * err_cos + 2 * U * (np.abs(amb) + np.abs(dr * cosl)))
    return s32.astype(F32), s64, err


def _shade(o, ids, ws, hs, ss, cam, light, ambient, directional, face_rgb, vert_rgb, bg, nf):
    """Colours of the samples given their face ids, and the resolved image: fp32 replay, float64, bound.

    b_k = fl(E_k) / fl(area2): E exact, 3 roundings -> rel 3 u.  iz = (iz0 + b1 (iz1 - iz0)) + b2 (iz2 - iz0): the terms pass <= 6 roundings
      -> |err iz| <= gamma(6) (|iz0| + |b1 (iz1 - iz0)| + |b2 (iz2 - iz0)|).
    vertex colours: w_k = b_k iz_k (4 u), ((w0 c0 + w1 c1) + w2 c2): <= 7 roundings per term -> gamma(7) sum |w_k c_k|; divided by iz:
      |err albedo| <= gamma(7) sum |w_k c_k| / iz + |albedo| err iz / iz + u |albedo|.
    colour = albedo * shade: |err| <= |albedo| err shade + shade err albedo + u |colour|.
    pixel = (n samples added one by one) / n, n = ss^2: |err| <= (sum err_s + gamma(n - 1) sum |colour_s|) / n  (the division by n is exact)."""
    bg32 = np.asarray(bg, F32)
    col32 = np.broadcast_to(bg32, (hs, ws, 3)).copy()
    col64 = col32.astype(F64)
    err = np.zeros((hs, ws, 3))
    iz64 = np.zeros((hs, ws))
    err_iz = np.zeros((hs, ws))
    # the shade is per ORIGINAL face; o["vid"] is a permutation of it per face whose cross product differs by the sign the turn removes --
    # the header says "from the vertices in the caller's order", which is what `faces_in_order` restores
    covered = ids >= 0
    if covered.any():
        jj, ii = np.nonzero(covered)
        k = ids[jj, ii].astype(I64)
        sx, sy = 256 * ii.astype(I64) + 128, 256 * jj.astype(I64) + 128
        x, y, z = o["x"][k], o["y"][k], o["iz"][k]
        E = []
        for e in range(3):
            p, q = (e + 1) % 3, (e + 2) % 3
            E.append((x[:, q] - x[:, p]) * (sy - y[:, p]) - (y[:, q] - y[:, p]) * (sx - x[:, p]))
        a2 = o["area2"][k]
        b32 = [E[e].astype(F32) / a2.astype(F32) for e in range(3)]
        b64 = [E[e].astype(F64) / a2.astype(F64) for e in range(3)]
        iz32 = (z[:, 0] + b32[1] * (z[:, 1] - z[:, 0])) + b32[2] * (z[:, 2] - z[:, 0])
        zd = z.astype(F64)
        izd = (zd[:, 0] + b64[1] * (zd[:, 1] - zd[:, 0])) + b64[2] * (zd[:, 2] - zd[:, 0])
        e_iz = SLOP * gamma(6) * (np.abs(zd[:, 0]) + np.abs(b64[1] * (zd[:, 1] - zd[:, 0])) + np.abs(b64[2] * (zd[:, 2] - zd[:, 0])))
        iz64[jj, ii], err_iz[jj, ii] = izd, e_iz
        s32, s64, e_s = (a[k] for a in face_shades(o["faces_in_order"], cam, light, ambient, directional))
        if face_rgb is not None:
            a32 = np.asarray(face_rgb, F32)[k]
            a64, e_a = a32.astype(F64), np.zeros(a32.shape)
        elif vert_rgb is not None:
            c = np.asarray(vert_rgb, F32)[o["vid"][k]]                  # (n, 3 vertices, 3 channels)
            w32 = [b32[e] * z[:, e] for e in range(3)]
            with np.errstate(divide="ignore", invalid="ignore"):
                a32 = ((w32[0][:, None] * c[:, 0] + w32[1][:, None] * c[:, 1]) + w32[2][:, None] * c[:, 2]) / iz32[:, None]
                cd = c.astype(F64)
                w64 = [b64[e] * zd[:, e] for e in range(3)]
                a64 = ((w64[0][:, None] * cd[:, 0] + w64[1][:, None] * cd[:, 1]) + w64[2][:, None] * cd[:, 2]) / izd[:, None]
                mag = sum(np.abs(w64[e])[:, None] * np.abs(cd[:, e]) for e in range(3))
                e_a = SLOP * (gamma(7) * mag / np.abs(izd)[:, None] + np.abs(a64) * (e_iz / np.abs(izd))[:, None] + U * np.abs(a64))
        else:
            a32 = np.ones((len(k), 3), F32)
            a64, e_a = a32.astype(F64), np.zeros(a32.shape)
        col32[jj, ii] = a32 * s32[:, None]
        c64 = a64 * s64[:, None]
        col64[jj, ii] = c64
        err[jj, ii] = SLOP * (np.abs(a64) * e_s[:, None] + np.abs(s64)[:, None] * e_a + U * np.abs(c64))
    h, w, n = hs // ss, ws // ss, ss * ss
    t32 = col32.reshape(h, ss, w, ss, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, n, 3)     # a pixel's samples: rows top to bottom, then left to right
    t64 = col64.reshape(h, ss, w, ss, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, n, 3)
    terr = err.reshape(h, ss, w, ss, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, n, 3)
    acc = t32[:, :, 0].copy()
    for s in range(1, n):
        acc = acc + t32[:, :, s]
    image = acc * F32(1.0 / n)
    err_image = SLOP * (terr.sum(2) + gamma(max(n - 1, 1)) * np.abs(t64).sum(2)) / n
    return dict(colour=col32, image=image.astype(F32), image64=t64.sum(2) / n, err_image=err_image, iz64=iz64, err_iz=err_iz)


# ------------------------------------------------------------------------------------------------------------------------------ scenes
def watertight_grid(rows, cols, ws, hs, seed=0, reach=1.25, on_centres=4):
    """A jittered triangulated grid of 2 * rows * cols faces with random windings and random diagonals, in the fixed-point coordinates of
    a ws x hs sample screen, reaching beyond it by the factor `reach` about its middle; `on_centres` interior vertices sit exactly on sample
    centres.  Returns px, py (V) int64, faces (nf, 3) int32.  Every sample of the screen lies inside the grid."""
    rng = np.random.default_rng(seed)
    gx = np.linspace(-(reach - 1) / 2, 1 + (reach - 1) / 2, cols + 1) * ws * 256
    gy = np.linspace(-(reach - 1) / 2, 1 + (reach - 1) / 2, rows + 1) * hs * 256
    X, Y = np.meshgrid(gx, gy)
    # +-0.2 of a cell per axis: two corners moving towards a quad's diagonal cover < 0.57 of the 0.71 between them, so every quad stays convex
    jx, jy = (rng.random(X.shape) - 0.5) * 0.4 * (gx[1] - gx[0]), (rng.random(X.shape) - 0.5) * 0.4 * (gy[1] - gy[0])
    jx[[0, -1], :] = 0; jx[:, [0, -1]] = 0; jy[[0, -1], :] = 0; jy[:, [0, -1]] = 0       # the rim stays put: the screen stays inside
    px, py = np.rint(X + jx).astype(I64).reshape(-1), np.rint(Y + jy).astype(I64).reshape(-1)
    inner = [(r, c) for r in range(1, rows) for c in range(1, cols)]
    for r, c in [inner[i] for i in rng.permutation(len(inner))[:on_centres]]:
        v = r * (cols + 1) + c
        px[v], py[v] = (px[v] // 256) * 256 + 128, (py[v] // 256) * 256 + 128
    faces = []
    for r in range(rows):
        for c in range(cols):
            a, b = r * (cols + 1) + c, r * (cols + 1) + c + 1
            d, e = a + cols + 1, b + cols + 1
            tris = [[a, b, e], [a, e, d]] if rng.random() < 0.5 else [[a, b, d], [b, e, d]]
            for t in tris:
                t = list(np.roll(t, rng.integers(0, 3)))
                faces.append(t[::-1] if rng.random() < 0.5 else t)
    return px, py, np.asarray(faces, np.int32)

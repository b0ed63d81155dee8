"""Time the virtual depth-sensor scan (garment4d_amd/scan.py, csrc/scan/scan.hip) at BASELINE cfg4's mesh sizes: 240 frames of a 6890-vertex
body plus a 4096-vertex garment (13568 + 8064 = 21632 faces), a 256 x 256 sensor, K = 4 cameras around the scene, N = 8192 points per frame.
usage: python scripts/time_scan.py [frames] [iters] [cams] [n_points]
Prints, from HIP events around `iters` calls after a warm-up: the K project + raster calls a scan follows, the three launches of
g4d_scan_points_f32 on their own, the whole scan_meshes call, and the same selection and unprojection written as device torch ops on the same
GPU (cumsum over the hit mask + searchsorted, then gathers) -- with the ratio, the hit fraction and whether the two give the same bits."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from garment4d_amd import _lib, render, scan
from garment4d_amd import synthetic as syn

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 240
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K = int(sys.argv[3]) if len(sys.argv) > 3 else 4
N = int(sys.argv[4]) if len(sys.argv) > 4 else 8192
W = H = 256
T = 30
nbatch = (frames + T - 1) // T

scene = syn.garment_scene(nbatch, T, 4, body_rc=(65, 106), garment_rc=(64, 64), seed=1)
body_v = scene["batch"]["smpl_vertices_torch"].reshape(-1, 6890, 3)[:frames]
gv, gq = scene["template"]
rng = np.random.default_rng(2)
cloth_v = (gv[None] + np.cumsum(rng.standard_normal((frames, 1, 3)) * 0.004, 0) + rng.standard_normal((frames,) + gv.shape) * 0.001).astype(np.float32)
faces = np.concatenate([scene["body"]["faces"], np.concatenate([gq[:, [0, 1, 2]], gq[:, [0, 2, 3]]], 0) + 6890]).astype(np.int32)
nfb = len(scene["body"]["faces"])
v = torch.from_numpy(np.ascontiguousarray(np.concatenate([body_v, cloth_v], 1))).cuda()
labels = torch.from_numpy(np.where(np.arange(len(faces)) >= nfb, 6, 0).astype(np.int32)).cuda()
cameras = scan.ring_cameras(K)
f_dev, _ = render._faces(faces, v.device)
nf, V = len(faces), v.shape[1]


def timed(fn):
    """Milliseconds per call of fn: two warm-up calls, then HIP events around `iters` calls."""
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def views():
    ps = [render.project(v, cam, (W, H), 1) for cam in cameras]
    ids = torch.stack([render.rasterize(p.px, p.py, p.invz, faces, (W, H), 1, want_image=False).face_id for p in ps])
    return tuple(torch.stack([getattr(p, n) for p in ps]) for n in ("px", "py", "invz")) + (ids,)


ms_views, (px, py, invz, ids) = timed(views)
L, _, _ = _lib.scan_lib()
ws = _lib.workspace(int(L.g4d_scan_ws_bytes(frames, K, W, H)), v.device)
out = scan.Scan(torch.empty((frames, N, 3), device="cuda"), *(torch.empty((frames, N), dtype=torch.int32, device="cuda") for _ in range(3)),
                torch.empty((frames,), dtype=torch.int32, device="cuda"))


def kernels():
    _lib.call("g4d_scan_points_f32", frames, K, V, nf, W, H, px.data_ptr(), py.data_ptr(), invz.data_ptr(), ids.data_ptr(), v.data_ptr(), f_dev.data_ptr(),
              labels.data_ptr(), N, 0, ws.data_ptr(), ws.numel(), out.points.data_ptr(), out.labels.data_ptr(), out.face.data_ptr(), out.sample.data_ptr(),
              out.count.data_ptr(), _lib.stream_ptr())
    return out


def mix(x):
    m = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m       # (wraps modulo 2^64: the low 32 bits are the product's)
    return x ^ (x >> 16)


def torch_scan(seed=0):
    """include/g4d_scan.h in device torch ops: ranks by cumsum over the hit mask, the point's hit by searchsorted, gathers, the same arithmetic."""
    flat = ids.permute(1, 0, 2, 3).reshape(frames, -1)
    hit = (flat >= 0) & (flat < nf)
    csum = hit.cumsum(1)
    M = csum[:, -1:]
    j = torch.arange(N, device="cuda")[None]
    lo, hi = j * M // N, (j + 1) * M // N
    fk = mix(mix(torch.tensor(seed, device="cuda")) ^ torch.arange(frames, device="cuda"))[:, None]
    rank = torch.where(M >= N, lo + mix(fk ^ j) % (hi - lo).clamp_min(1), j % M.clamp_min(1))
    s = torch.searchsorted(csum, rank + 1).clamp_max(flat.shape[1] - 1)
    g = flat.gather(1, s).long().clamp(0, nf - 1)
    c, rest = s // (H * W), s % (H * W)
    sy, sx = 256 * (rest // W) + 128, 256 * (rest % W) + 128
    vid = f_dev.long()[g]                                                   # (F, N, 3)
    at = (c[..., None] * V + vid).reshape(frames, -1)
    take = lambda a: a.permute(1, 0, 2).reshape(frames, -1).gather(1, at).reshape(frames, N, 3)
    x, y, iz = take(px).long(), take(py).long(), take(invz)
    area2 = (x[..., 1] - x[..., 0]) * (y[..., 2] - y[..., 0]) - (x[..., 2] - x[..., 0]) * (y[..., 1] - y[..., 0])
    perm = torch.where((area2 < 0)[..., None], torch.tensor([0, 2, 1], device="cuda"), torch.tensor([0, 1, 2], device="cuda"))
    x, y, iz, vid = x.gather(2, perm), y.gather(2, perm), iz.gather(2, perm), vid.gather(2, perm)
    a2 = area2.abs().float()
    b = [((x[..., (e + 2) % 3] - x[..., (e + 1) % 3]) * (sy - y[..., (e + 1) % 3]) - (y[..., (e + 2) % 3] - y[..., (e + 1) % 3]) * (sx - x[..., (e + 1) % 3])).float() / a2
         for e in range(3)]
    izs = (iz[..., 0] + b[1] * (iz[..., 1] - iz[..., 0])) + b[2] * (iz[..., 2] - iz[..., 0])
    p = [v.gather(1, vid[..., e:e + 1].expand(-1, -1, 3)) for e in range(3)]
    w = [(b[e] * iz[..., e])[..., None] for e in range(3)]
    points = ((w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]) / izs[..., None]
    seen = (M > 0)
    return scan.Scan(torch.where(seen[..., None], points, 0.0), torch.where(seen, labels[g], -1), torch.where(seen, g.int(), -1), torch.where(seen, s.int(), -1),
                     M[:, 0].int())


ms_kernels, got = timed(kernels)
ms_torch, ref = timed(torch_scan)
ms_whole, _ = timed(lambda: scan.scan_meshes(v, faces, cameras, (W, H), N, labels))
same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(got, ref))
count = got.count.float()
print(f"frames={frames} V={V} faces={nf} sensor {W}x{H} K={K} N={N}: {K} x (project + raster) {ms_views:.2f} ms; g4d_scan_points_f32 (3 launches) {ms_kernels:.3f} ms; "
      f"whole scan_meshes {ms_whole:.2f} ms ({frames / ms_whole * 1e3:.0f} frames/s); torch formulation of the 3 launches {ms_torch:.2f} ms = "
      f"{ms_torch / ms_kernels:.1f} x; same bits as torch: {same}; hit fraction {float(count.mean()) / (K * H * W):.4f} (hits per frame: mean {float(count.mean()):.0f}, "
      f"min {int(count.min())}, max {int(count.max())}); labels: body {int((got.labels == 0).sum())}, garment {int((got.labels == 6).sum())}")

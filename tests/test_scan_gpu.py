"""The scan kernels (csrc/scan/scan.hip) against the numpy twin of include/g4d_scan.h (tests/scan_twin.py): EVERY bit of points, labels, face,
sample and count equals the twin's fp32 replay -- at sensor sizes around the chunk size (g4d_scan_chunk()), with frames that see nothing /
everything / something in one call, with N below, at and above the number of hits, with face ids the rasterizer cannot have written -- and
whole calls: repeatable, seeded, capturable in a graph, scan_batch on a synthetic loader batch."""
import functools
import types

import numpy as np
import pytest
import torch

import render_twin as RT
import scan_twin as ST
from garment4d_amd import _lib, render, scan
from garment4d_amd import synthetic as syn

pytestmark = pytest.mark.gpu

FIELDS = ("points", "labels", "face", "sample", "count")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def run_scan(px, py, invz, ids, verts, faces, n_points, seed=0, face_labels=None):
    """g4d_scan_points_f32 itself on numpy inputs: px, py, invz (K,F,V), ids (K,F,h,w), verts (F,V,3) -> dict of numpy outputs."""
    K, F_, V = px.shape
    h, w = ids.shape[2:]
    L, _, _ = _lib.scan_lib()
    t = [dev(np.asarray(px, np.int32)), dev(np.asarray(py, np.int32)), dev(np.asarray(invz, np.float32)), dev(np.asarray(ids, np.int32)),
         dev(np.asarray(verts, np.float32)), dev(np.asarray(faces, np.int32).reshape(-1, 3))]
    lab = dev(np.asarray(face_labels, np.int32)) if face_labels is not None else None
    ws = _lib.workspace(L.g4d_scan_ws_bytes(F_, K, w, h), "cuda")
    ws.fill_(0x5A)                                                           # nothing may depend on what the scratch held
    N = int(n_points)
    out = dict(points=torch.full((F_, N, 3), -7.0, device="cuda"), **{k: torch.full((F_, N), -7, dtype=torch.int32, device="cuda") for k in FIELDS[1:4]},
               count=torch.full((F_,), -7, dtype=torch.int32, device="cuda"))
    _lib.call("g4d_scan_points_f32", F_, K, V, len(faces), w, h, *(a.data_ptr() for a in t), lab.data_ptr() if lab is not None else None, N, int(seed),
              ws.data_ptr(), ws.numel(), *(out[k].data_ptr() for k in FIELDS), _lib.stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equals_twin(got, want):
    for k in FIELDS:
        g, t = _bits(got[k]), _bits(np.asarray(want[k], got[k].dtype))
        assert g.shape == t.shape and np.array_equal(g, t), (k, np.argwhere(g != t)[:5], g[g != t][:5], t[g != t][:5])


def integer_scene(seed, K, F_, V, nf, w, h):
    """Random triangles in fixed-point sample coordinates reaching a fifth beyond the w x h sensor, per camera and frame (any integers will
    do: the stage is defined on them), random world positions, and the face ids of the numpy rasterizer."""
    rng = np.random.default_rng(seed)
    px = rng.integers(int(-0.2 * w * 256), int(1.2 * w * 256) + 1, (K, F_, V))
    py = rng.integers(int(-0.2 * h * 256), int(1.2 * h * 256) + 1, (K, F_, V))
    invz = (0.5 + rng.random((K, F_, V))).astype(np.float32)
    verts = rng.standard_normal((F_, V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (nf, 3)).astype(np.int32)
    return px, py, invz, verts, faces


def twin_ids(px, py, invz, faces, w, h):
    K, F_ = px.shape[:2]
    return np.stack([np.stack([RT.raster(px[k, f], py[k, f], invz[k, f], faces, w, h, shade=False)["face_id"] for f in range(F_)]) for k in range(K)])


def _sizes():
    c = scan.chunk()
    return {"less than a chunk": (20, 12, 1), "exactly one chunk": (32, c // 32, 1), "two chunks minus a few": (33, (2 * c - 2) // 66, 2),
            "one chunk plus one": (c + 1, 1, 1), "waves straddle rows and cameras": (50, 30, 3)}


@pytest.mark.parametrize("size", ["less than a chunk", "exactly one chunk", "two chunks minus a few", "one chunk plus one", "waves straddle rows and cameras"])
def test_scan_equals_the_twin_at_sensor_sizes_around_the_chunk(size):
    w, h, K = _sizes()[size]
    c = scan.chunk()
    assert c % 32 == 0 and {"exactly one chunk": w * h * K == c, "two chunks minus a few": 0 < 2 * c - w * h * K < 66,
                            "one chunk plus one": w * h * K == c + 1, "less than a chunk": w * h * K < c}.get(size, w % 64 != 0)
    px, py, invz, verts, faces = integer_scene(w + 3 * h + K, K, 2, 24, 40, w, h)
    ids = twin_ids(px, py, invz, faces, w, h)
    labels = (np.arange(len(faces)) * 7 % 5).astype(np.int32)
    want = ST.scan(px, py, invz, ids, verts, faces, 100, 11, labels)
    assert (want["count"] > 0).all() and (ids < 0).any()
    assert_equals_twin(run_scan(px, py, invz, ids, verts, faces, 100, 11, labels), want)


def test_scan_frames_that_see_nothing_everything_and_something_in_one_call():
    """F = 3: no face covers frame 0 (M = 0), one quad nearer than everything fills the screen of frame 1 in every camera (M = K h w), frame 2
    is an ordinary one: a chunk offset leaking from one frame into the next would show."""
    w, h, K, N = 33, 31, 2, 200
    px, py, invz, verts, faces = integer_scene(5, K, 3, 28, 40, w, h)
    faces = np.concatenate([faces % 24, [[24, 25, 26], [26, 25, 27]]]).astype(np.int32)
    px[:, :, 24:] = np.array([-256, w * 256 + 256, -256, w * 256 + 256])
    py[:, :, 24:] = np.array([-256, -256, h * 256 + 256, h * 256 + 256])
    invz[:, :, 24:] = 0                                                      # the quad is dropped ...
    invz[:, 1, 24:] = 5                                                      # ... except in frame 1, where it is the nearest thing
    invz[:, 0] = 0                                                           # frame 0: every face is dropped
    ids = twin_ids(px, py, invz, faces, w, h)
    want = ST.scan(px, py, invz, ids, verts, faces, N, 3)
    assert want["count"][0] == 0 and want["count"][1] == K * h * w and 0 < want["count"][2] < K * h * w
    assert (want["face"][0] == -1).all() and (want["face"][1] >= 40).all() and (want["face"][2] < 40).all()
    got = run_scan(px, py, invz, ids, verts, faces, N, 3)
    assert_equals_twin(got, want)
    assert (got["points"][0] == 0).all() and (got["labels"][0] == -1).all() and (got["sample"][0] == -1).all()


@functools.lru_cache(maxsize=None)
def _one_scene():
    w, h, K = 33, 31, 2
    px, py, invz, verts, faces = integer_scene(21, K, 1, 24, 40, w, h)
    ids = twin_ids(px, py, invz, faces, w, h)
    return px, py, invz, verts, faces, ids, int((ids >= 0).sum())


@pytest.mark.parametrize("n", ["M - 1", "M", "M + 1", "1", "2 M + 3"])
def test_scan_point_counts_below_at_and_above_the_number_of_hits(n):
    px, py, invz, verts, faces, ids, M = _one_scene()
    N = {"M - 1": M - 1, "M": M, "M + 1": M + 1, "1": 1, "2 M + 3": 2 * M + 3}[n]     # (of three in a row at most one is a multiple of 64)
    assert M > 300
    want = ST.scan(px, py, invz, ids, verts, faces, N, 9)
    got = run_scan(px, py, invz, ids, verts, faces, N, 9)
    assert_equals_twin(got, want)
    assert got["count"][0] == M and (got["face"] >= 0).all()
    if N <= M:
        assert (np.diff(got["sample"][0]) > 0).all()                         # distinct hits in scan order
    else:
        assert set(np.bincount(np.unique(got["sample"][0], return_inverse=True)[1])) <= {N // M, -(-N // M)}


def test_scan_writes_a_face_id_the_rasterizer_cannot_have_written_as_a_miss():
    """Zero area, a vertex behind `near`, a coordinate past the limit, a vertex index outside the mesh: ranked as hits, never read through."""
    px, py, invz, verts, faces, ids, M = _one_scene()
    px, invz, faces, ids = px.copy(), invz.copy(), faces.copy(), ids.copy()
    faces[1], faces[2], faces[3], faces[4], faces[5] = [0, 0, 1], [20, 1, 2], [21, 1, 3], [2, 24, 3], [-1, 2, 3]
    invz[:, :, 20] = 0
    px[:, :, 21] = 1 << 22
    rng = np.random.default_rng(0)
    ids[rng.random(ids.shape) < 0.3] = -1
    bad = rng.random(ids.shape) < 0.3
    ids[bad] = rng.integers(1, 6, int(bad.sum()))
    ids[0, 0, 0, :4] = [len(faces), len(faces) + 5, -2, 1 << 30]             # no faces at all: misses
    for N in (150, 3000):
        want = ST.scan(px, py, invz, ids, verts, faces, N, 2)
        got = run_scan(px, py, invz, ids, verts, faces, N, 2)
        assert_equals_twin(got, want)
        assert (got["face"] == -1).any() and (got["face"] >= 6).any() and not np.isin(got["face"], [1, 2, 3, 4, 5]).any()
        assert (got["points"][got["face"] == -1] == 0).all() and got["count"][0] == ((ids >= 0) & (ids < len(faces))).sum()


# --------------------------------------------------------------------------------------------------------------------------- whole calls
CAMERAS = [render.look_at_camera(1.5, 10.0, 45.0), render.look_at_camera(1.5, -5.0, 200.0)]
SIZE = (64, 48)


def _cylinder_meshes(F_, seed=0):
    """The quad cylinder of the render tests with two faces the rasterizer drops: a zero-area one, and one with a vertex 5 % of the way
    from the first camera's eye to the origin -- nearer than `near` for that camera, in plain sight of the second."""
    rng = np.random.default_rng(seed)
    v, q = syn.quad_cylinder(14, 18)
    v = (v * np.array([1.4, 0.9, 1.4], np.float32) + np.array([0, -0.45, 0], np.float32)).astype(np.float32)
    v = np.concatenate([v, np.float32(CAMERAS[0].eye)[None] * np.float32(0.95)])
    faces = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]], [[3, 3, 40], [len(v) - 1, 5, 60]]], 0).astype(np.int32)
    verts = (v[None] + rng.standard_normal((F_,) + v.shape).astype(np.float32) * 0.01).astype(np.float32)
    verts[:, -1] = v[-1]
    return verts, faces


def twin_scan_of_meshes(verts, faces, cameras, n_points, seed, face_labels=None):
    w, h = SIZE
    cams = [RT.camera(c.eye, c.at, c.up, c.half_angle, w, h, 1) for c in cameras]
    proj = [RT.project_f32(verts, cam, c.near) for cam, c in zip(cams, cameras)]
    px, py, invz = (np.stack([p[k] for p in proj]) for k in range(3))
    return ST.scan(px, py, invz, twin_ids(px, py, invz, faces, w, h), verts, faces, n_points, seed, face_labels, cams)


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_scan_meshes_equals_the_twin_and_never_shows_a_dropped_face():
    verts, faces = _cylinder_meshes(2)
    nf = len(faces)
    labels = (np.arange(nf) % 3 + 1).astype(np.int32)
    want = twin_scan_of_meshes(verts, faces, CAMERAS, 300, 4, labels)
    got = scan.scan_meshes(dev(verts), faces, CAMERAS, SIZE, 300, dev(labels), seed=4)
    torch.cuda.synchronize()
    assert got.points.shape == (2, 300, 3) and got.labels.shape == got.face.shape == got.sample.shape == (2, 300) and got.count.shape == (2,)
    assert_equals_twin({k: getattr(got, k).cpu().numpy() for k in FIELDS}, want)
    face, camera = got.face.cpu().numpy(), got.sample.cpu().numpy() // (SIZE[0] * SIZE[1])
    assert (face >= 0).all() and set(np.unique(camera)) == {0, 1} and (want["count"] > 300).all()
    assert not (face == nf - 2).any() and not (face[camera == 0] == nf - 1).any()      # no area; behind the first camera's near plane
    assert np.array_equal(got.labels.cpu().numpy(), labels[face])
    # the points are where the twin's float64 says, on the cylinder and back on their rays
    assert (np.abs(got.points.cpu().numpy() - want["points64"]) <= want["err"]).all() and want["inside"].all()
    assert (np.abs(want["reproj"] - want["centre"]).max(-1) <= want["err_reproj"]).all() and want["err_reproj"].max() < 256 / 64
    # without labels: all 0
    plain = scan.scan_meshes(dev(verts), faces, CAMERAS, SIZE, 300, seed=4)
    assert (plain.labels == 0).all() and _same(plain[:1] + plain[2:], got[:1] + got[2:])


def test_same_seed_same_bits_and_another_seed_other_samples():
    verts, faces = _cylinder_meshes(2, seed=1)
    v = dev(verts)
    a, b = scan.scan_meshes(v, faces, CAMERAS, SIZE, 250, seed=5), scan.scan_meshes(v, faces, CAMERAS, SIZE, 250, seed=5)
    c = scan.scan_meshes(v, faces, CAMERAS, SIZE, 250, seed=6)
    assert _same(a, b) and torch.equal(a.count, c.count) and int(a.count.min()) > 250
    assert not torch.equal(a.sample, c.sample) and not torch.equal(a.sample[0], a.sample[1])
    g = torch.Generator(device="cuda").manual_seed(1)
    noisy = scan.scan_meshes(v, faces, CAMERAS, SIZE, 250, seed=5, noise_sigma=0.01, generator=g)
    moved = (noisy.points - a.points).cpu().numpy().astype(np.float64)
    eyes = np.array([cam.eye for cam in CAMERAS])[a.sample.cpu().numpy() // (SIZE[0] * SIZE[1])]
    ray = a.points.cpu().numpy() - eyes
    assert _same(noisy[1:], a[1:]) and 0.007 < np.sqrt((moved ** 2).sum(-1).mean()) < 0.014           # sigma = 0.01 over 500 draws
    assert (np.linalg.norm(np.cross(moved, ray), axis=-1) <= 1e-5 * np.linalg.norm(ray, axis=-1)).all()   # along the viewing ray only


def test_captured_scan_replays_to_the_eager_bits():
    all_verts, faces = _cylinder_meshes(6, seed=5)
    sets = [dev(all_verts[i:i + 2]) for i in (0, 2, 4)]
    labels = dev((np.arange(len(faces)) % 2).astype(np.int32))
    static = sets[0].clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        scan.scan_meshes(static, faces, CAMERAS, SIZE, 300, labels, seed=8)   # eager first: the faces go to the host and back once
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = scan.scan_meshes(static, faces, CAMERAS, SIZE, 300, labels, seed=8)
    for s in (1, 2, 1):
        static.copy_(sets[s])
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = scan.scan_meshes(sets[s], faces, CAMERAS, SIZE, 300, labels, seed=8)
        torch.cuda.synchronize()
        assert _same(got, want), s
    assert not torch.equal(scan.scan_meshes(sets[1], faces, CAMERAS, SIZE, 300).points, scan.scan_meshes(sets[2], faces, CAMERAS, SIZE, 300).points)


def test_timed_calls_sees_the_scan_entry_point():
    verts, faces = _cylinder_meshes(1)
    with _lib.timed_calls() as t:
        scan.scan_meshes(dev(verts), faces, CAMERAS, SIZE, 64)
    names = [r[0] for r in t.results()]
    assert names == ["g4d_render_project_f32", "g4d_render_project_f32", "g4d_render_raster", "g4d_render_raster", "g4d_scan_points_f32"]


def test_scan_batch_on_a_synthetic_loader_batch():
    """Body + garment of synthetic.garment_scene as the loader hands them over (the garment relative to the root joint), three cameras around
    them: the dict that goes into `inputs`, both labels present, every frame seen, a garment label only on a garment face."""
    nbatch, T, N, label = 1, 2, 500, 6
    scene = syn.garment_scene(nbatch, T, 64, seed=1)
    body_v = scene["batch"]["smpl_vertices_torch"]
    gv, gq = scene["template"]
    rng = np.random.default_rng(3)
    root = rng.normal(0.0, 0.05, (nbatch, T, 3)).astype(np.float32)
    garment = (gv[None, None] + rng.standard_normal((nbatch, T, 1, 3)).astype(np.float32) * 0.004).astype(np.float32) - root[:, :, None]
    inputs = dict(smpl_vertices_torch=dev(body_v), garment_torch=dev(garment), smpl_root_joints_torch=dev(root))
    body_model = types.SimpleNamespace(faces=scene["body"]["faces"])
    garment_f = np.concatenate([gq[:, [0, 1, 2]], gq[:, [0, 2, 3]]], 0).astype(np.int32)
    cams = scan.ring_cameras(3)
    out = scan.scan_batch(inputs, body_model, garment_f, label, cameras=cams, n_points=N, seed=1, image_size=64)
    torch.cuda.synchronize()
    assert sorted(out) == ["count", "pcd_label_torch", "pcd_torch"]
    assert out["pcd_torch"].shape == (nbatch, T, N, 3) and out["pcd_torch"].dtype == torch.float32 and out["pcd_torch"].is_cuda
    assert out["pcd_label_torch"].shape == (nbatch, T, N, 1) and out["pcd_label_torch"].dtype == torch.int32
    assert out["count"].shape == (nbatch, T) and out["count"].dtype == torch.int32 and bool((out["count"] > 0).all())
    lab = out["pcd_label_torch"].cpu().numpy().reshape(T, N)
    assert all(set(np.unique(lab[f])) == {0, label} for f in range(T)), "both labels in every frame"
    # the same mesh through scan_meshes, which also says which face a point lies on
    Vb, nfb = body_v.shape[2], len(scene["body"]["faces"])
    verts = torch.cat([inputs["smpl_vertices_torch"], inputs["garment_torch"] + inputs["smpl_root_joints_torch"][:, :, None]], 2).reshape(nbatch * T, -1, 3)
    faces = np.concatenate([scene["body"]["faces"].astype(np.int32), garment_f + Vb])
    face_labels = dev(np.where(np.arange(len(faces)) >= nfb, label, 0).astype(np.int32))
    direct = scan.scan_meshes(verts, faces, cams, 64, N, face_labels, seed=1)
    assert torch.equal(direct.points.view(torch.int32), out["pcd_torch"].view(torch.int32).reshape(T, N, 3)) and torch.equal(direct.count, out["count"].reshape(T))
    face = direct.face.cpu().numpy()
    assert np.array_equal(direct.labels.cpu().numpy(), lab) and ((lab == label) == (face >= nfb)).all() and (face >= 0).all()
    # a scan is one-sided: every point lies in front of the camera that saw it, no farther than the far side of the scene
    eyes = np.array([c.eye for c in cams])[direct.sample.cpu().numpy() // (64 * 64)]
    dist = np.linalg.norm(direct.points.cpu().numpy() - eyes, axis=-1)
    assert (dist > 0.5).all() and (dist < 2.5).all()

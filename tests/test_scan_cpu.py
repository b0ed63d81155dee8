"""Virtual depth-sensor scans without a GPU: the third (header, library) pair -- include/g4d_scan.h against its record
tests/scan_abi_snapshot.txt, libg4d_scan.so's exports and argument checks -- and the properties of the numpy twin (tests/scan_twin.py) that the
GPU tests compare the kernels with: the selection inverts per hit, the picks are distinct and ascending, a point lies on its triangle and
projects back onto its sample centre, the fp32 replay stays within the derived bound of float64."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_twin as RT
import scan_twin as ST
from conftest import ROOT
from test_abi_cpu import _LETTERS

EINVAL = 10001
HEADER = os.path.join(ROOT, "include", "g4d_scan.h")
NAME = "g4d_scan_points_f32"


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


def test_parsed_scan_header_equals_its_snapshot():
    """include/g4d_scan.h as _lib.parse_header reads it == tests/scan_abi_snapshot.txt, both ways and in the header's order, constants included."""
    from garment4d_amd import _lib, scan
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "scan_abi_snapshot.txt")).read().splitlines()]
    recorded = dict(ln for ln in lines if ln[0].startswith("g4d_"))
    rec_consts = {ln[0]: int(ln[1]) for ln in lines if ln[0].startswith("G4D_")}
    assert all(len(ln) == 2 for ln in lines) and fields == []
    assert set(parsed) == set(_declared()) and len(parsed) == 3
    assert {n: (parsed.get(n), recorded.get(n)) for n in set(parsed) | set(recorded) if parsed.get(n) != recorded.get(n)} == {}
    assert list(parsed) == list(recorded)
    assert consts == rec_consts
    assert consts["G4D_SCAN_MAX_CAMS"] == 8 == scan.MAX_CAMS == ST.MAX_CAMS


def test_scan_library_exports_every_declared_symbol_and_leaves_the_first_two_pairs_alone():
    from garment4d_amd import _lib
    assert os.path.exists(_lib.SCAN_LIB_PATH), "run __graft_entry__.build() first"
    L, protos, consts = _lib.scan_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
    assert L.g4d_scan_chunk() >= 64 and L.g4d_scan_chunk() % 64 == 0
    assert not any(n.startswith("g4d_scan") for n in _lib.PROTOTYPES) and not any(n.startswith("g4d_scan") for n in _lib.render_lib()[1])
    assert len(_lib.render_lib()[1]) == 4 and not any(k.startswith("G4D_SCAN") for k in _lib.render_lib()[2])
    assert not hasattr(_lib.lib(), NAME) and not hasattr(_lib.render_lib()[0], NAME) and _lib.lib().g4d_version() == 263
    assert _lib.scan_lib()[0] is L                                          # loaded once
    assert _lib._entry(NAME) is getattr(L, NAME) and _lib._entry("g4d_render_chunk") is getattr(_lib.render_lib()[0], "g4d_render_chunk")


def test_scan_ws_bytes_query():
    from garment4d_amd import _lib
    L, _, _ = _lib.scan_lib()
    chunk = L.g4d_scan_chunk()
    want = lambda frames, cams, w, h: 8 * frames * -(-(cams * w * h) // chunk)
    for zero in ((0, 2, 8, 8), (3, 0, 8, 8), (3, 2, 0, 8), (3, 2, 8, 0)):
        assert L.g4d_scan_ws_bytes(*zero) == 0, zero
    assert L.g4d_scan_ws_bytes(1, 1, 1, 1) == 8
    for shape in ((1, 1, 20, 12), (3, 2, 33, 31), (2, 1, chunk, 1), (2, 1, chunk + 1, 1), (240, 4, 256, 256)):
        assert L.g4d_scan_ws_bytes(*shape) == want(*shape), shape
    assert L.g4d_scan_ws_bytes(3000, 8, 4096, 4096) == want(3000, 8, 4096, 4096) > 1 << 31           # size_t, not int
    for neg in ((-1, 1, 4, 4), (1, -1, 4, 4), (1, 1, -4, 4), (1, 1, 4, -4)):
        assert L.g4d_scan_ws_bytes(*neg) == ctypes.c_size_t(-1).value, neg
    assert L.g4d_scan_ws_bytes(1, 2, 32768, 32768) == ctypes.c_size_t(-1).value                      # cams * h * w = 2^31
    assert L.g4d_scan_ws_bytes(1, 1, 32768, 32768) == want(1, 1, 32768, 32768)                       # 2^30: fine


def _args(frames=2, cams=2, v=8, nf=4, w=16, h=16, px=1, py=1, invz=1, face_id=1, verts=1, faces=1, face_labels=0, n_points=32, seed=7, ws=16,
          ws_bytes=1 << 20, points=1, labels=1, face=1, sample=1, count=1):
    return (frames, cams, v, nf, w, h, px, py, invz, face_id, verts, faces, face_labels, n_points, seed, ws, ws_bytes, points, labels, face, sample, count, 0)


def test_scan_argument_validation_needs_no_gpu():
    """Every check of include/g4d_scan.h comes before any launch: G4D_EINVAL with the entry point's name in the ONE error state,
    g4d_last_error() of libg4d_hip.so -- through _lib.call, which raises G4DError with that text."""
    from garment4d_amd import _lib
    L, _, _ = _lib.scan_lib()
    main = _lib.lib()
    need = L.g4d_scan_ws_bytes(2, 2, 16, 16)
    bad = [(dict(frames=-1), "negative"), (dict(v=-2), "negative"), (dict(nf=-1), "negative"), (dict(w=-1), "negative"), (dict(h=-3), "negative"),
           (dict(n_points=-1), "n_points"), (dict(cams=0), "cams must be"), (dict(cams=9), "cams must be"), (dict(cams=-1), "cams must be"),
           (dict(w=32769), "<= 32768"), (dict(h=40000), "<= 32768"), (dict(cams=2, w=32768, h=32768), "< 2^31"), (dict(cams=8, w=32768, h=8192), "< 2^31"),
           (dict(ws_bytes=need - 1), "workspace"), (dict(ws_bytes=0), "workspace"), (dict(ws=24), "aligned"), (dict(ws=4), "aligned")]
    bad += [({p: 0}, "null") for p in ("px", "py", "invz", "face_id", "verts", "faces", "ws", "points", "labels", "face", "sample", "count")]
    for kw, needle in bad:
        rc = L.g4d_scan_points_f32(*_args(**kw))
        assert rc == EINVAL, (kw, rc)
        msg = main.g4d_last_error().decode()                                 # libg4d_hip.so's accessor: one error state for the three libraries
        assert NAME in msg and needle in msg, (kw, msg)
        with pytest.raises(_lib.G4DError, match=NAME):
            _lib.call(NAME, *_args(**kw))
    # face_labels may be NULL or not: either way the call gets as far as the next check
    for fl in (0, 1):
        assert L.g4d_scan_points_f32(*_args(face_labels=fl, count=0)) == EINVAL and "null" in main.g4d_last_error().decode()
    assert need == 8 * 2 * -(-512 // L.g4d_scan_chunk())


def test_empty_scan_problems_return_zero():
    from garment4d_amd import _lib
    L, _, _ = _lib.scan_lib()
    nothing = dict(px=0, py=0, invz=0, face_id=0, verts=0, faces=0, ws=0, ws_bytes=0, points=0, labels=0, face=0, sample=0, count=0)
    for kw in (dict(frames=0), dict(w=0), dict(h=0), dict(n_points=0)):
        assert L.g4d_scan_points_f32(*_args(**kw)) == 0, kw
        assert L.g4d_scan_points_f32(*_args(**kw, **nothing)) == 0, kw
    assert _lib.call(NAME, *_args(frames=0)) == 0
    assert L.g4d_scan_points_f32(*_args(frames=0, cams=9)) == EINVAL        # an empty problem is still checked


def test_call_traces_the_third_library(capfd, monkeypatch):
    from garment4d_amd import _lib
    _lib.scan_lib()
    monkeypatch.setattr(_lib, "_TRACE", True)
    assert _lib.call(NAME, *_args(frames=0, w=20, h=12)) == 0
    assert "g4d call g4d_scan_points_f32 0 2 8 4 20 12" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------------------------------ twin: selection
CASES = [(1, 1), (1, 7), (5, 7), (7, 7), (8, 7), (13, 7), (14, 7), (1000, 7), (2046, 512), (1025, 1024), (262144, 8192)]


def test_twin_mixer_is_the_headers():
    """The constants and shifts of the header, on Python integers."""
    def mix(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF
        return x ^ x >> 16
    for seed, f, j in ((0, 0, 0), (1, 2, 3), (0xFFFFFFFF, 239, 8191), (12345, 7, 65535)):
        assert int(ST.key(seed, f, j)) == mix(mix(mix(seed) ^ f) ^ j)
    assert mix(0) == 0 and int(ST.key(0, 0, 0)) == 0 and len(set(int(ST.key(0, 0, j)) % 64 for j in range(1, 200))) > 32


@pytest.mark.parametrize("M,N", CASES)
def test_twin_selection_forward_and_per_hit_forms_agree(M, N):
    for seed, f in ((0, 0), (1, 0), (1, 5), (0xDEADBEEF, 239)):
        fwd = ST.select_forward(M, N, seed, f)
        inv, writes = ST.select_per_hit(M, N, seed, f)
        assert (writes == 1).all() and np.array_equal(fwd, inv), (M, N, seed, f)
        assert fwd.shape == (N,) and (fwd >= 0).all() and (fwd < M).all()
        if M >= N:
            assert (np.diff(fwd) > 0).all()                                 # distinct and strictly ascending
            j = np.arange(N)
            assert (fwd >= j * M // N).all() and (fwd < (j + 1) * M // N).all()
        else:
            times = np.bincount(fwd, minlength=M)
            assert set(times) <= {N // M, -(-N // M)} and times.sum() == N and (times >= 1).all()
    if M >= 2 * N and N > 1:                                                # seed and frame both matter where several strata have a choice
        assert not np.array_equal(ST.select_forward(M, N, 0, 0), ST.select_forward(M, N, 1, 0))
        assert not np.array_equal(ST.select_forward(M, N, 0, 0), ST.select_forward(M, N, 0, 1))


def test_twin_frame_without_hits_gets_the_documented_fill():
    assert (ST.select_forward(0, 5, 3, 0) == -1).all()
    inv, writes = ST.select_per_hit(0, 5, 3, 0)
    assert (inv == -1).all() and (writes == 0).all()
    r = ST.scan_frame(np.zeros((2, 4), int), np.zeros((2, 4), int), np.ones((2, 4), np.float32), np.full((2, 3, 5), -1), np.zeros((4, 3), np.float32),
                      np.array([[0, 1, 2]]), 6, 0, 0)
    assert r["count"] == 0 and (r["points"] == 0).all() and r["points"].shape == (6, 3) and r["points"].dtype == np.float32
    assert all((r[k] == -1).all() and r[k].dtype == np.int32 and r[k].shape == (6,) for k in ("labels", "face", "sample"))


# --------------------------------------------------------------------------------------------------------------------- twin: unprojection
EYES = ((1.06, 0.2, -1.06), (-1.2, 0.1, 0.9), (0.1, 1.4, 0.3))


def _random_scene(seed, V=40, nf=60, w=24, h=16):
    """The recipe of tests/test_render_cpu.py's _random_scene at ss = 1, seen by the cameras of EYES."""
    rng = np.random.default_rng(seed)
    verts = (rng.random((V, 3)) - 0.5).astype(np.float32) * np.array([1.2, 1.0, 0.8], np.float32)
    faces = rng.integers(0, V, (nf, 3)).astype(np.int32)
    cams = [RT.camera(eye, (0, 0, 0), (0, 1, 0) if k < 2 else (0, 0, 1), 30.0, w, h, 1) for k, eye in enumerate(EYES)]
    proj = [RT.project_f32(verts, cam, 0.1) for cam in cams]
    px, py, invz = (np.stack([p[k] for p in proj]) for k in range(3))
    ids = np.stack([RT.raster(px[k], py[k], invz[k], faces, w, h, shade=False)["face_id"] for k in range(len(cams))])
    return verts, faces, cams, px, py, invz, ids


@pytest.mark.parametrize("seed", range(4))
def test_twin_points_lie_on_their_triangles_and_project_back_onto_their_samples(seed):
    verts, faces, cams, px, py, invz, ids = _random_scene(seed)
    M = int((ids >= 0).sum())
    labels = np.arange(len(faces), dtype=np.int32) % 5
    for N in (64, M, 2 * M + 3):
        r = ST.scan_frame(px, py, invz, ids, verts, faces, N, seed, 1, face_labels=labels, cams=cams)
        assert r["count"] == M > 150 and (r["face"] >= 0).all() and r["inside"].all()
        assert np.array_equal(r["labels"], labels[r["face"]]) and len(np.unique(r["sample"] // (16 * 24))) == 3
        assert np.array_equal(ids.reshape(-1)[r["sample"]], r["face"])
        # the fp32 replay within the derived bound of float64
        p, p64, err = r["points"].astype(np.float64), r["points64"], r["err"]
        assert np.isfinite(err).all() and (np.abs(p - p64) <= err).all() and err.max() < 1e-5
        # on its own triangle: within |err| of the plane, and inside the box of the three vertices widened by err
        tri = verts.astype(np.float64)[faces[r["face"]]]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        assert (np.abs(((p - tri[:, 0]) * n).sum(1)) <= np.linalg.norm(err, axis=1) + 1e-12).all()
        assert (p >= tri.min(1) - err).all() and (p <= tri.max(1) + err).all()
        # back onto its sample centre: within the derived bound, which is far below 1/64 of a sample (4 units of 1/256)
        off = np.abs(r["reproj"] - r["centre"]).max(1)
        print(f"seed {seed} N {N}: max |fp32 - float64| {np.abs(p - p64).max():.3g} (bound {err.max():.3g}); max reprojection offset {off.max():.3f} / 256 sample "
              f"(bound {r['err_reproj'].max():.3f})")
        assert (off <= r["err_reproj"]).all() and r["err_reproj"].max() < 256 / 64 and r["err_reproj"].min() >= 0.5


def test_twin_writes_a_selected_dropped_face_as_a_miss():
    """A face id the rasterizer cannot have written (zero area, a vertex behind `near`, an index outside the mesh): ranked as a hit, written as a miss."""
    px = np.array([[300, 5000, 300, 5000, 2650]])
    py = np.array([[300, 300, 5000, 5000, 300]])
    invz = np.array([[1, 1, 1, 0, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 4, 1], [3, 1, 2], [0, 1, 9]])          # fine, no area, behind near, outside the mesh
    ids = np.array([[[0, 1, 2, 3, -1, 0, 4, 0]]])                           # (1, 1, 8): 4 is no face at all -- a miss
    r = ST.scan_frame(px, py, invz, ids, np.eye(5, 3, dtype=np.float32), faces, 6, 0, 0)
    assert r["count"] == 6 and list(r["face"]) == [0, -1, -1, -1, 0, 0] and list(r["sample"]) == [0, -1, -1, -1, 5, 7]
    assert (r["points"][1:4] == 0).all() and list(r["labels"]) == [0, -1, -1, -1, 0, 0]


# ------------------------------------------------------------------------------------------------------------------------- Python layer
def test_scan_calls_refuse_cpu_tensors_and_wrong_shapes():
    import torch
    from garment4d_amd import render, scan
    faces = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(TypeError, match=r"scan_meshes: verts: a float32 HIP tensor .* \(no CPU fallback\)"):
        scan.scan_meshes(torch.zeros(2, 5, 3), faces)
    with pytest.raises(TypeError, match="HIP tensor"):
        scan.scan_meshes(torch.zeros(2, 5, 3, dtype=torch.float64), faces)
    for wrong in (torch.zeros(5, 3), torch.zeros(2, 5, 2), np.zeros((2, 5, 3), np.float32)):
        with pytest.raises(ValueError, match=r"scan_meshes: verts must be \(F, V, 3\)"):
            scan.scan_meshes(wrong, faces)
    for cams in ([], scan.ring_cameras(9)):
        with pytest.raises(ValueError, match="scan_meshes: 1 to 8 cameras"):
            scan.scan_meshes(torch.zeros(2, 5, 3), faces, cameras=cams)
    good = dict(smpl_vertices_torch=torch.zeros(1, 2, 6, 3), garment_torch=torch.zeros(1, 2, 4, 3), smpl_root_joints_torch=torch.zeros(1, 2, 3))
    with pytest.raises(TypeError, match=r"scan_batch: inputs\['smpl_vertices_torch'\] must be a float32 HIP tensor \(no CPU fallback\)"):
        scan.scan_batch(good, None, faces, 6)
    for key, wrong in (("garment_torch", torch.zeros(1, 3, 4, 3)), ("smpl_root_joints_torch", torch.zeros(1, 3)), ("smpl_vertices_torch", torch.zeros(2, 6, 3)),
                       ("garment_torch", np.zeros((1, 2, 4, 3), np.float32))):
        with pytest.raises(ValueError, match="scan_batch: smpl_vertices_torch"):
            scan.scan_batch({**good, key: wrong}, None, faces, 6)
    ring = scan.ring_cameras(4, distance=2.0, elevation=10.0, start=30.0)
    assert ring == [render.look_at_camera(2.0, 10.0, 30.0 + 90.0 * i) for i in range(4)] and scan.ring_cameras(1) == [render.look_at_camera(1.5, 0.0, 45.0)]

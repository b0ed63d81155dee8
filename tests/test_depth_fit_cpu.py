"""The projective ray-depth loss without a GPU: the seventh (header, library) pair -- include/g4d_depth.h against its record
tests/depth_abi_snapshot.txt, libg4d_depth.so's exports, argument checks and empty problems --, the Python layer's refusals, and the properties of
the numpy twin (tests/depth_fit_twin.py) that the GPU tests compare the kernels with: its tree adds everything once, a face at constant depth
gives exactly that depth, the float64 gradient equals central differences of the float64 loss with the association held fixed, and W == 0 gives a
zero loss with zero gradients."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import depth_fit_twin as DT
from conftest import ROOT
from test_abi_cpu import _LETTERS

F32, F64 = np.float32, np.float64
EINVAL = 10001
HEADER = os.path.join(ROOT, "include", "g4d_depth.h")
FWD, GRAD = "g4d_depth_fit_terms_f32", "g4d_depth_fit_vertex_grad_f32"


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


# ------------------------------------------------------------------------------------------------------------------------- the seventh pair
def test_parsed_depth_header_equals_its_snapshot():
    """include/g4d_depth.h as _lib.parse_header reads it == tests/depth_abi_snapshot.txt, both ways and in the header's order, constants included."""
    from garment4d_amd import _lib, depth_fit
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "depth_abi_snapshot.txt")).read().splitlines()]
    recorded = dict(ln for ln in lines if ln[0].startswith("g4d_"))
    rec_consts = {ln[0]: int(ln[1]) for ln in lines if ln[0].startswith("G4D_")}
    assert all(len(ln) == 2 for ln in lines) and fields == []
    assert set(parsed) == set(_declared()) and len(parsed) == 4
    assert {n: (parsed.get(n), recorded.get(n)) for n in set(parsed) | set(recorded) if parsed.get(n) != recorded.get(n)} == {}
    assert list(parsed) == list(recorded)
    assert consts == rec_consts
    assert (consts["G4D_DEPTH_MAX_CAMS"], consts["G4D_DEPTH_MAX_SIDE"], consts["G4D_DEPTH_MAX_FACES"]) == (DT.MAX_CAMS, DT.MAX_SIDE, DT.MAX_FACES)
    assert (consts["G4D_DEPTH_LANES"], consts["G4D_DEPTH_PER_LANE"]) == (DT.LANES, DT.PER_LANE)
    assert (depth_fit.MAX_CAMS, depth_fit.MAX_SIDE) == (DT.MAX_CAMS, DT.MAX_SIDE)
    assert consts["G4D_DEPTH_MAX_SIDE"] == _lib.render_lib()[2]["G4D_RENDER_MAX_SAMPLES"] and 3 * DT.MAX_FACES < 1 << 31 <= 3 * (DT.MAX_FACES + 1)


def test_depth_library_exports_every_declared_symbol_and_leaves_the_other_six_pairs_alone():
    from garment4d_amd import _lib
    assert os.path.exists(_lib.DEPTH_LIB_PATH), "run __graft_entry__.build() first"
    L, protos, consts = _lib.depth_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
    pairs = (_lib.render_lib(), _lib.scan_lib(), _lib.fit_lib(), _lib.smpl_lib(), _lib.skin_lib())
    assert not any(n.startswith("g4d_depth") for protos_ in (_lib.PROTOTYPES,) + tuple(p[1] for p in pairs) for n in protos_)
    assert [len(p[1]) for p in pairs] == [4, 3, 4, 4, 2]
    assert not any(k.startswith("G4D_DEPTH") for p in pairs for k in p[2]) and not any(k.startswith("G4D_DEPTH") for k in _lib.CONSTANTS)
    for other in (_lib.lib(),) + tuple(p[0] for p in pairs):
        assert not any(hasattr(other, n) for n in _declared())
    assert _lib.lib().g4d_version() == 263                                    # libg4d_hip.so's ABI is the parent's
    assert _lib.depth_lib()[0] is L                                           # loaded once
    assert _lib._entry(FWD) is getattr(L, FWD) and _lib._entry("g4d_scan_chunk") is getattr(_lib.scan_lib()[0], "g4d_scan_chunk")
    assert L.g4d_depth_chunk() == DT.CHUNK == 1024


def test_ws_bytes_query():
    from garment4d_amd import _lib
    L, _, _ = _lib.depth_lib()
    for args, want in (((2, 2, 32, 32), 2 * 2 * 16), ((2, 2, 33, 17), 2 * 2 * 16), ((1, 1, 1025, 1), 32), ((3, 1, 1024, 1), 48), ((240, 4, 256, 256), 240 * 256 * 16),
                       ((0, 2, 32, 32), 0), ((2, 0, 32, 32), 0), ((2, 2, 0, 32), 0), ((2, 2, 32, 0), 0)):
        assert L.g4d_depth_ws_bytes(*args) == want, args
    for args in ((-1, 1, 8, 8), (1, -1, 8, 8), (1, 1, -8, 8), (1, 1, 8, -8), (1, 2, 1 << 15, 1 << 15), (1, 1, 1 << 16, 1 << 15)):
        assert L.g4d_depth_ws_bytes(*args) == ctypes.c_size_t(-1).value, args


def _fwd(frames=2, cams=2, v=6, nf=4, w=8, h=8, cam=16, faces=16, face_id=16, depth_obs=16, weights=0, labels_obs=0, face_labels=0, cams_host=16, trunc=1.0,
         grazing=0.1, ws=16, ws_bytes=1 << 20, sums=16, count=16, total=16, resid=0):
    return (frames, cams, v, nf, w, h, cam, faces, face_id, depth_obs, weights, labels_obs, face_labels, cams_host, trunc, grazing, ws, ws_bytes, sums, count,
            total, resid, 0)


def _grd(frames=2, cams=2, v=6, nf=4, w=8, h=8, px=16, py=16, invz=16, cam=16, faces=16, face_id=16, depth_obs=16, weights=0, labels_obs=0, face_labels=0,
         cams_host=16, trunc=1.0, grazing=0.1, total=16, grad_out=16, vc_rowptr=16, vc_corners=16, grad_verts=16):
    return (frames, cams, v, nf, w, h, px, py, invz, cam, faces, face_id, depth_obs, weights, labels_obs, face_labels, cams_host, trunc, grazing, total,
            grad_out, vc_rowptr, vc_corners, grad_verts, 0)


def test_depth_argument_validation_needs_no_gpu():
    """Every check of include/g4d_depth.h comes before any launch: G4D_EINVAL with the entry point's name in the ONE error state,
    g4d_last_error() of libg4d_hip.so -- through _lib.call, which raises G4DError with that text."""
    from garment4d_amd import _lib
    L, _, _ = _lib.depth_lib()
    main = _lib.lib()
    shape = [(dict(frames=-1), "negative"), (dict(v=-1), "negative"), (dict(nf=-2), "negative"), (dict(w=-1), "negative"), (dict(h=-8), "negative"),
             (dict(cams=0), "cams must be in [1, 8]"), (dict(cams=9), "cams must be in [1, 8]"), (dict(cams=-1), "cams must be in [1, 8]"),
             (dict(w=4097), "<= 4096"), (dict(h=4097), "<= 4096"), (dict(nf=DT.MAX_FACES + 1), "nf must be <="),
             (dict(labels_obs=16), "go together"), (dict(face_labels=16), "go together")]
    bad = [(name, args, kw, needle) for name, args in ((FWD, _fwd), (GRAD, _grd)) for kw, needle in shape]
    bad += [(FWD, _fwd, {k: 0}, "null") for k in ("cam", "faces", "face_id", "depth_obs", "cams_host", "ws", "sums", "count", "total")]
    bad += [(FWD, _fwd, dict(ws_bytes=2 * 16 - 1), "workspace of 31 bytes, 32 needed"), (FWD, _fwd, dict(ws=8), "16-byte aligned")]
    bad += [(GRAD, _grd, {k: 0}, "null") for k in ("px", "py", "invz", "cam", "faces", "face_id", "depth_obs", "cams_host", "total", "grad_out", "vc_rowptr",
                                                   "vc_corners", "grad_verts")]
    for name, args, kw, needle in bad:
        rc = getattr(L, name)(*args(**kw))
        assert rc == EINVAL, (name, kw, rc)
        msg = main.g4d_last_error().decode()                                 # libg4d_hip.so's accessor: one error state for the seven libraries
        assert name in msg and needle in msg, (name, kw, msg)
        with pytest.raises(_lib.G4DError, match=name):
            _lib.call(name, *args(**kw))
    # the domain is checked on an empty problem too, and before the pointers
    assert L.g4d_depth_fit_terms_f32(*_fwd(frames=0, cams=9)) == EINVAL and L.g4d_depth_fit_vertex_grad_f32(*_grd(v=0, w=4097)) == EINVAL
    assert L.g4d_depth_fit_terms_f32(*_fwd(cams=9, cam=0)) == EINVAL and "cams must be" in main.g4d_last_error().decode()


def test_empty_depth_problems_return_zero():
    from garment4d_amd import _lib
    L, _, _ = _lib.depth_lib()
    none_f = dict(cam=0, faces=0, face_id=0, depth_obs=0, cams_host=0, ws=0, ws_bytes=0, sums=0, count=0, total=0)
    for kw in (dict(frames=0), dict(w=0), dict(h=0), dict(frames=0, v=0, nf=0)):
        assert L.g4d_depth_fit_terms_f32(*_fwd(**kw)) == 0 and L.g4d_depth_fit_terms_f32(*_fwd(**{**none_f, **kw})) == 0, kw
    none_g = dict(px=0, py=0, invz=0, cam=0, faces=0, face_id=0, depth_obs=0, cams_host=0, total=0, grad_out=0, vc_rowptr=0, vc_corners=0, grad_verts=0)
    for kw in (dict(frames=0), dict(v=0), dict(w=0), dict(h=0)):
        assert L.g4d_depth_fit_vertex_grad_f32(*_grd(**kw)) == 0 and L.g4d_depth_fit_vertex_grad_f32(*_grd(**{**none_g, **kw})) == 0, kw
    assert _lib.call(FWD, *_fwd(frames=0)) == 0 and _lib.call(GRAD, *_grd(v=0)) == 0


def test_depth_calls_refuse_cpu_tensors_wrong_shapes_and_the_limits_before_any_launch():
    import torch
    from garment4d_amd import depth_fit, render
    faces = np.array([[0, 1, 2]], np.int32)
    cams = [render.Camera(*c) for c in DT.FRONT]
    d, v = torch.zeros(2, 2, 8, 8), torch.zeros(2, 4, 3)
    with pytest.raises(TypeError, match=r"depth_mesh_distance: verts: a float32 HIP tensor .* \(no CPU fallback\)"):
        depth_fit.depth_mesh_distance(d, v, faces, cams)
    with pytest.raises(TypeError, match=r"sensor_depth: verts: a float32 HIP tensor .* \(no CPU fallback\)"):
        depth_fit.sensor_depth(v, faces, cams, 8)
    with pytest.raises(TypeError, match="HIP tensor"):
        depth_fit.depth_mesh_distance(d, v.double(), faces, cams)
    for wrong in (torch.zeros(2, 8, 8), np.zeros((2, 2, 8, 8), np.float32)):
        with pytest.raises(ValueError, match=r"depth_mesh_distance: depth_obs must be \(K, F, h, w\)"):
            depth_fit.depth_mesh_distance(wrong, v, faces, cams)
    for wrong in (torch.zeros(4, 3), torch.zeros(2, 4, 2)):
        with pytest.raises(ValueError, match=r"verts must be \(F, V, 3\)"):
            depth_fit.depth_mesh_distance(d, wrong, faces, cams)
        with pytest.raises(ValueError, match=r"verts must be \(F, V, 3\)"):
            depth_fit.sensor_depth(wrong, faces, cams, 8)
    with pytest.raises(ValueError, match="1 to 8 cameras"):
        depth_fit.depth_mesh_distance(torch.zeros(9, 2, 8, 8), v, faces, cams * 5)
    with pytest.raises(ValueError, match="1 to 8 cameras"):
        depth_fit.sensor_depth(v, faces, [], 8)
    with pytest.raises(ValueError, match="at most 4096 x 4096"):
        depth_fit.sensor_depth(v, faces, cams, (4097, 8))
    with pytest.raises(ValueError, match="at most 4096 x 4096"):
        depth_fit.depth_mesh_distance(torch.zeros(2, 2, 1, 4097), v, faces, cams)
    with pytest.raises(ValueError, match="2 cameras and 2 frames"):
        depth_fit.depth_mesh_distance(torch.zeros(2, 3, 8, 8), v, faces, cams)
    with pytest.raises(ValueError, match="image_size"):
        depth_fit.depth_mesh_distance(d, v, faces, cams, image_size=16)
    with pytest.raises(ValueError, match="go together"):
        depth_fit.depth_mesh_distance(d, v, faces, cams, labels=torch.zeros(2, 2, 8, 8, dtype=torch.int32))
    # the camera constants are the projection's: the twin's come from the render twin's restatement of it
    got, want = depth_fit.camera_constants(cams), DT.cams_host(DT.camera_constants(DT.FRONT, 8, 8))
    assert got.dtype == F32 and np.array_equal(got.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------------------------ twin
def test_twin_tree_adds_everything_once():
    x = np.arange(1, 3001, dtype=F64)
    assert DT.tree(x) == x.sum() and DT.tree(x[:1]) == 1 and DT.tree(x[:0]) == 0 and DT.tree(x[:1025]) == x[:1025].sum()
    assert len(DT.chunk_sums(x)) == 3 and DT.chunk_sums(x)[2] == x[2048:].sum()
    y = np.random.default_rng(1).random(2500).astype(F32)
    s = DT.tree(y)
    # a term passes 3 adds in its lane, 6 + 3 in the chunk's tree, then 1 + 6 + 3 in the frame's: 22 roundings at the most
    assert s.dtype == F32 and abs(float(s) - y.astype(F64).sum()) <= 22 * 2.0 ** -24 * y.astype(F64).sum()


def test_twin_depth_of_a_face_at_constant_depth_is_that_depth_exactly():
    """All three vertices at camera-space z = Z: n = (0, 0, n.z) exactly (every product with a z difference is 0), den = (0 + 0) + n.z and
    n . c0 = (0 + 0) + n.z * Z, so z = fl(fl(n.z * Z) / n.z).  For Z a power of two the product is exact and the quotient is Z itself: equality in
    every bit, in either dtype and at every sample.  For any other Z the two roundings can leave one unit in the last place, no more."""
    face_id = np.zeros((5, 7), np.int32)
    for Z in (2.0, 1.0, 0.5, 4.0, 1.5, 0.75, 1.3):
        camc = np.array([[-0.31, -0.27, Z], [0.43, -0.11, Z], [0.07, 0.39, Z]], F32)
        for dt in (F32, F64):
            Zd = dt(F32(Z))
            t = DT.sample_terms(camc, np.array([[0, 1, 2]]), face_id, np.full((5, 7), 0.25, F32), None, None, None, F32(1.7320508), None, 0.1, dt)
            assert t["inlier"].all() and t["z"].dtype == dt
            assert (t["n"][..., :2] == 0).all() and (t["den"] == t["n"][..., 2]).all()
            if Z in (2.0, 1.0, 0.5, 4.0):
                assert (t["z"] == Zd).all() and (t["r"] == Zd - dt(0.25)).all()
            assert np.abs(t["z"] - Zd).max() <= np.spacing(Zd)
            assert np.abs(t["b"].sum(-1) - 1).max() <= 4 * np.finfo(dt).eps


@functools.lru_cache(maxsize=None)
def scene(w=32, h=32, seed=0):
    """The GPU tests' kind of input, on the CPU: the bent grid of 98 faces, F = 2, the two front cameras, a sensor of w x h rays observing a
    displaced copy of the mesh (the twin's own projection and coverage), weights in (0.5, 1.5) with a tenth of them 0."""
    verts, faces = DT.bent_grid(8, 8, 2, seed)
    consts = DT.camera_constants(DT.FRONT, w, h)
    rng = np.random.default_rng(seed + 1)
    target = (verts + 0.02 * rng.standard_normal(verts.shape)).astype(F32)
    tp = DT.project(target, consts)
    _, depth_obs = DT.rasterize(tp[0], tp[1], tp[2], faces, w, h)
    px, py, invz, cam = DT.project(verts, consts)
    face_id, _ = DT.rasterize(px, py, invz, faces, w, h)
    weights = np.where(rng.random(face_id.shape) < 0.1, 0, 0.5 + rng.random(face_id.shape)).astype(F32)
    return dict(verts=verts, faces=faces, consts=consts, depth_obs=depth_obs, px=px, py=py, invz=invz, cam=cam, face_id=face_id, weights=weights, w=w, h=h)


@pytest.mark.parametrize("size", [(32, 32), (33, 17)])
def test_twin_float64_gradient_equals_central_differences_with_the_association_held_fixed(size):
    """Central differences (step 1e-6) of the twin's float64 loss in 12 vertices x 3 coordinates per frame, trunc=None, face_id fixed.  No sample
    may change sides of the grazing bound within the step: a vertex moving by 1e-6 turns a face of edge length >= 0.05 by at most 4e-5 in
    cosine, so every associated sample must keep |cosine - grazing| > 1e-4 -- asserted, as is that the decided inlier set never moves.
    Tolerance, relative to the largest gradient entry: the loss is a rational function of the vertices that varies over the length den / |n|
    >= grazing * (distance to the camera) ~ 0.1, so the difference quotient's truncation error step^2 f''' / 6 is of the order
    (1e-6 / 0.1)^2 = 1e-10 of the gradient, and its rounding error 2^-53 loss / step ~ 1e-10 * loss; 1e-7 leaves three orders for the constants."""
    s = scene(*size)
    faces, consts, V = s["faces"], s["consts"], s["verts"].shape[1]
    v0 = s["verts"].astype(F64)
    kw = dict(weights=s["weights"], trunc=None, grazing=0.1, dt=F64)
    base = DT.forward(DT.world_to_cam64(v0, consts), faces, s["face_id"], s["depth_obs"], consts, **kw)
    assert base["inlier"].sum() > 150 and base["W"] > 0 and base["loss"] > 0
    assoc = base["associated"]
    assert np.abs(base["cosine"][assoc] - 0.1).min() > 1e-4
    grad = DT.gradient(base, s["px"], s["py"], s["invz"], faces, s["face_id"], consts, V, 1.0, F64)
    assert grad.dtype == F64 and np.isfinite(grad).all()
    rng = np.random.default_rng(3)
    step, scale, worst = 1e-6, np.abs(grad).max(), 0.0
    for f in range(2):
        touched = np.unique(faces[np.unique(s["face_id"][:, f][base["inlier"][:, f]])])
        for i in rng.choice(touched, 12, replace=False):
            for k in range(3):
                vals = []
                for sign in (1, -1):
                    v = v0.copy()
                    v[f, i, k] += sign * step
                    t = DT.forward(DT.world_to_cam64(v, consts), faces, s["face_id"], s["depth_obs"], consts, **kw)
                    assert np.array_equal(t["decided"], base["decided"])
                    vals.append(float(t["loss"]))
                worst = max(worst, abs((vals[0] - vals[1]) / (2 * step) - grad[f, i, k]) / scale)
    print(f"{size}: central differences vs the twin's float64 gradient, relative to the largest entry {scale:.3g}: {worst:.3g}")
    assert worst <= 1e-7


def test_twin_float32_replay_is_close_to_float64_on_the_same_inliers():
    """The fp32 replay against float64 on the replay's own inlier set: loss within 1e-4 relative, gradient within 1e-3 of its largest entry --
    a sanity bound (the kernels are held to the replay's bits, not to this)."""
    s = scene()
    faces, consts, V = s["faces"], s["consts"], s["verts"].shape[1]
    t32 = DT.forward(s["cam"], faces, s["face_id"], s["depth_obs"], consts, weights=s["weights"], trunc=0.03, dt=F32)
    t64 = DT.forward(DT.world_to_cam64(s["verts"], consts), faces, s["face_id"], s["depth_obs"], consts, weights=s["weights"], trunc=0.03, dt=F64,
                     inlier=t32["inlier"])
    assert t32["loss"].dtype == F32 and 0 < t32["inlier"].sum() < t32["associated"].sum()             # the truncation excludes some
    assert abs(float(t32["loss"]) - float(t64["loss"])) <= 1e-4 * float(t64["loss"]) and np.array_equal(t32["count"], t64["count"])
    g32 = DT.gradient(t32, s["px"], s["py"], s["invz"], faces, s["face_id"], consts, V, 1.0, F32)
    g64 = DT.gradient(t64, s["px"], s["py"], s["invz"], faces, s["face_id"], consts, V, 1.0, F64)
    assert g32.dtype == F32 and np.abs(g32 - g64).max() <= 1e-3 * np.abs(g64).max()
    assert np.isnan(t32["resid"][~t32["inlier"]]).all() and np.isfinite(t32["resid"][t32["inlier"]]).all()


def test_twin_zero_weight_sum_gives_zero_loss_and_gradients():
    s = scene()
    faces, consts, V = s["faces"], s["consts"], s["verts"].shape[1]
    for kw in (dict(weights=np.zeros_like(s["weights"])), dict(weights=s["weights"], depth_obs=np.full_like(s["depth_obs"], np.inf))):
        t = DT.forward(s["cam"], faces, s["face_id"], kw.get("depth_obs", s["depth_obs"]), consts, weights=kw["weights"], dt=F32)
        g = DT.gradient(t, s["px"], s["py"], s["invz"], faces, s["face_id"], consts, V, 1.0, F32)
        assert t["W"] == 0 and t["loss"] == 0 and not t["inlier"].any() and (g == 0).all() and (t["count"] == 0).all() and (t["sums"] == 0).all()

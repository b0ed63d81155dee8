"""The point-to-surface loss without a GPU: the fourth (header, library) pair -- include/g4d_fit.h against its record
tests/fit_abi_snapshot.txt, libg4d_fit.so's exports, argument checks and empty problems -- and the properties of the numpy twin
(tests/fit_twin.py) that the GPU tests compare the kernels with: the weights sum to 1 and give back the search's point, the grouped order is
(face, index), translating the mesh equals translating the points the other way, the float64 gradient equals central differences of the
truncated loss, the fp32 replay stays within the derived bounds of float64, and the test inputs cover every part of the classification."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import fit_twin as FT
import postprocess_twin as PT
from conftest import ROOT
from test_abi_cpu import _LETTERS

F32, F64 = np.float32, np.float64
EINVAL = 10001
HEADER = os.path.join(ROOT, "include", "g4d_fit.h")
FWD, GROUP, GRAD = "g4d_fit_point_face_f32", "g4d_fit_group_f32", "g4d_fit_vertex_grad_f32"
TRUNC = 0.05
TAU2 = float(F32(TRUNC) * F32(TRUNC))


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


# ------------------------------------------------------------------------------------------------------------------------- the fourth pair
def test_parsed_fit_header_equals_its_snapshot():
    """include/g4d_fit.h as _lib.parse_header reads it == tests/fit_abi_snapshot.txt, both ways and in the header's order, constants included."""
    from garment4d_amd import _lib
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "fit_abi_snapshot.txt")).read().splitlines()]
    recorded = dict(ln for ln in lines if ln[0].startswith("g4d_"))
    rec_consts = {ln[0]: int(ln[1]) for ln in lines if ln[0].startswith("G4D_")}
    assert all(len(ln) == 2 for ln in lines) and fields == []
    assert set(parsed) == set(_declared()) and len(parsed) == 4
    assert {n: (parsed.get(n), recorded.get(n)) for n in set(parsed) | set(recorded) if parsed.get(n) != recorded.get(n)} == {}
    assert list(parsed) == list(recorded)
    assert consts == rec_consts
    assert (consts["G4D_FIT_MAX_POINTS"], consts["G4D_FIT_MAX_FACES"], consts["G4D_FIT_LANES"]) == (FT.MAX_POINTS, FT.MAX_FACES, FT.LANES)
    assert consts["G4D_FIT_MAX_POINTS"] == 1 << FT.INDEX_BITS and consts["G4D_FIT_MAX_FACES"] << FT.INDEX_BITS == 1 << 32


def test_fit_library_exports_every_declared_symbol_and_leaves_the_other_three_pairs_alone():
    from garment4d_amd import _lib
    assert os.path.exists(_lib.FIT_LIB_PATH), "run __graft_entry__.build() first"
    L, protos, consts = _lib.fit_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
    others = (_lib.PROTOTYPES, _lib.render_lib()[1], _lib.scan_lib()[1])
    assert not any(n.startswith("g4d_fit") for protos_ in others for n in protos_)
    assert len(_lib.render_lib()[1]) == 4 and len(_lib.scan_lib()[1]) == 3
    assert not any(k.startswith("G4D_FIT") for lib_ in (_lib.render_lib(), _lib.scan_lib()) for k in lib_[2]) and not any(k.startswith("G4D_FIT") for k in _lib.CONSTANTS)
    for other in (_lib.lib(), _lib.render_lib()[0], _lib.scan_lib()[0]):
        assert not any(hasattr(other, n) for n in (FWD, GROUP, GRAD))
    assert _lib.lib().g4d_version() == 263
    assert _lib.fit_lib()[0] is L                                            # loaded once
    assert _lib._entry(FWD) is getattr(L, FWD) and _lib._entry("g4d_scan_chunk") is getattr(_lib.scan_lib()[0], "g4d_scan_chunk")


def test_group_lds_bytes_query():
    from garment4d_amd import _lib
    L, _, _ = _lib.fit_lib()
    for p, want in ((0, 256), (1, 256), (63, 256), (64, 256), (65, 512), (300, 2048), (8192, 32768), (8193, 65536), (32768, 131072)):
        assert L.g4d_fit_group_lds_bytes(p) == want, p
    for p in (-1, 32769, 1 << 30):
        assert L.g4d_fit_group_lds_bytes(p) == ctypes.c_size_t(-1).value, p
    assert L.g4d_fit_group_lds_bytes(32768) <= 160 * 1024                     # the sort's keys fit the LDS of one compute unit


def _fwd(frames=2, p=8, v=6, nf=4, points=1, verts=1, faces=1, face=1, weights=0, tau2=1.0, bary=1, resid=1, dist2=1, inlier=1, sums=1, count=1, total=1):
    return (frames, p, v, nf, points, verts, faces, face, weights, tau2, bary, resid, dist2, inlier, sums, count, total, 0)


def _grp(frames=2, p=8, nf=4, face=1, inlier=1, keys=1):
    return (frames, p, nf, face, inlier, keys, 0)


def _grd(frames=2, p=8, v=6, nf=4, bary=1, resid=1, inlier=1, weights=0, keys=1, count=1, total=1, grad_out=1, vc_rowptr=1, vc_corners=1, grad_verts=1,
         grad_points=0):
    return (frames, p, v, nf, bary, resid, inlier, weights, keys, count, total, grad_out, vc_rowptr, vc_corners, grad_verts, grad_points, 0)


def test_fit_argument_validation_needs_no_gpu():
    """Every check of include/g4d_fit.h comes before any launch: G4D_EINVAL with the entry point's name in the ONE error state,
    g4d_last_error() of libg4d_hip.so -- through _lib.call, which raises G4DError with that text."""
    from garment4d_amd import _lib
    L, _, _ = _lib.fit_lib()
    main = _lib.lib()
    bad = [(FWD, _fwd, dict(frames=-1), "negative"), (FWD, _fwd, dict(p=-1), "negative"), (FWD, _fwd, dict(v=-3), "negative"), (FWD, _fwd, dict(nf=-1), "negative"),
           (FWD, _fwd, dict(v=0), "empty mesh"), (FWD, _fwd, dict(nf=0), "empty mesh"),
           (GROUP, _grp, dict(frames=-1), "negative"), (GROUP, _grp, dict(p=-2), "negative"), (GROUP, _grp, dict(nf=-1), "negative"),
           (GROUP, _grp, dict(p=32769), "<= 32768"), (GROUP, _grp, dict(nf=131073), "<= 131072"), (GROUP, _grp, dict(p=1 << 30, nf=1 << 30), "<= 32768"),
           (GRAD, _grd, dict(frames=-1), "negative"), (GRAD, _grd, dict(p=-1), "negative"), (GRAD, _grd, dict(v=-1), "negative"), (GRAD, _grd, dict(nf=-5), "negative"),
           (GRAD, _grd, dict(p=32769), "<= 32768"), (GRAD, _grd, dict(nf=131073), "<= 131072")]
    bad += [(FWD, _fwd, {k: 0}, "null") for k in ("points", "verts", "faces", "face", "bary", "resid", "dist2", "inlier", "sums", "count", "total")]
    bad += [(GROUP, _grp, {k: 0}, "null") for k in ("face", "inlier", "keys")]
    bad += [(GRAD, _grd, {k: 0}, "null") for k in ("bary", "resid", "inlier", "keys", "count", "total", "grad_out", "vc_rowptr", "vc_corners", "grad_verts")]
    for name, args, kw, needle in bad:
        rc = getattr(L, name)(*args(**kw))
        assert rc == EINVAL, (name, kw, rc)
        msg = main.g4d_last_error().decode()                                 # libg4d_hip.so's accessor: one error state for the four libraries
        assert name in msg and needle in msg, (name, kw, msg)
        with pytest.raises(_lib.G4DError, match=name):
            _lib.call(name, *args(**kw))
    # the domain is checked on an empty problem too, and before the pointers
    assert L.g4d_fit_group_f32(*_grp(frames=0, p=32769)) == EINVAL and L.g4d_fit_vertex_grad_f32(*_grd(frames=0, nf=131073)) == EINVAL
    assert L.g4d_fit_group_f32(*_grp(p=32769, face=0)) == EINVAL and "<= 32768" in main.g4d_last_error().decode()


def test_empty_fit_problems_return_zero():
    from garment4d_amd import _lib
    L, _, _ = _lib.fit_lib()
    none_f = dict(points=0, verts=0, faces=0, face=0, bary=0, resid=0, dist2=0, inlier=0, sums=0, count=0, total=0)
    for kw in (dict(frames=0), dict(p=0), dict(frames=0, v=0, nf=0)):
        assert L.g4d_fit_point_face_f32(*_fwd(**kw)) == 0 and L.g4d_fit_point_face_f32(*_fwd(**kw, **none_f)) == 0, kw
    for kw in (dict(frames=0), dict(p=0)):
        assert L.g4d_fit_group_f32(*_grp(**kw)) == 0 and L.g4d_fit_group_f32(*_grp(**kw, face=0, inlier=0, keys=0)) == 0, kw
    none_g = dict(bary=0, resid=0, inlier=0, keys=0, count=0, total=0, grad_out=0, vc_rowptr=0, vc_corners=0, grad_verts=0)
    for kw in (dict(frames=0), dict(v=0), dict(v=0, p=0, grad_points=1)):
        assert L.g4d_fit_vertex_grad_f32(*_grd(**kw)) == 0 and L.g4d_fit_vertex_grad_f32(*_grd(**{**none_g, **kw})) == 0, kw
    assert _lib.call(FWD, *_fwd(frames=0)) == 0 and _lib.call(GROUP, *_grp(p=0)) == 0 and _lib.call(GRAD, *_grd(frames=0)) == 0


def test_call_traces_the_fourth_library(capfd, monkeypatch):
    from garment4d_amd import _lib
    _lib.fit_lib()
    monkeypatch.setattr(_lib, "_TRACE", True)
    assert _lib.call(GROUP, *_grp(frames=0, p=300, nf=360)) == 0
    assert "g4d call g4d_fit_group_f32 0 300 360" in capfd.readouterr().err


def test_fit_calls_refuse_cpu_tensors_and_wrong_shapes():
    import torch
    from garment4d_amd import fit
    faces = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(TypeError, match=r"point_mesh_distance: points: a float32 HIP tensor .* \(no CPU fallback\)"):
        fit.point_mesh_distance(torch.zeros(2, 5, 3), torch.zeros(2, 4, 3), faces)
    with pytest.raises(TypeError, match="HIP tensor"):
        fit.point_mesh_distance(torch.zeros(2, 5, 3, dtype=torch.float64), torch.zeros(2, 4, 3), faces)
    for wrong in (torch.zeros(5, 3), torch.zeros(2, 5, 2), np.zeros((2, 5, 3), np.float32)):
        with pytest.raises(ValueError, match=r"point_mesh_distance: points must be \(F, n, 3\)"):
            fit.point_mesh_distance(wrong, torch.zeros(2, 4, 3), faces)
    good = dict(pcd_torch=torch.zeros(1, 2, 6, 3), pcd_label_torch=torch.zeros(1, 2, 6, 1, dtype=torch.int32), smpl_root_joints_torch=torch.zeros(1, 2, 3))
    out = dict(iter_regressed_lbs_garment_v=[torch.zeros(2, 4, 3)])
    with pytest.raises(TypeError, match=r"scan_fit_loss: inputs\['pcd_torch'\] must be a float32 HIP tensor \(no CPU fallback\)"):
        fit.scan_fit_loss(out, good, faces, 6)
    for key, wrong in (("pcd_torch", torch.zeros(2, 6, 3)), ("pcd_label_torch", torch.zeros(1, 2, 5, 1)), ("smpl_root_joints_torch", torch.zeros(1, 3))):
        with pytest.raises(ValueError, match="scan_fit_loss: inputs"):
            fit.scan_fit_loss(out, {**good, key: wrong}, faces, 6)
    assert fit._tau2(None) == np.inf and fit._tau2(0.05) == TAU2


# ------------------------------------------------------------------------------------------------------------------------- twin: the input
@functools.lru_cache(maxsize=None)
def case(name):
    """The GPU tests' input, on the CPU: FT.fit_scene(name) plus corner points, the float64 search, the float32 search (whose faces stand in
    for the kernel's), and both forwards and gradients on those faces."""
    sc = FT.fit_scene(name)
    corner = FT.corner_points(sc["verts"], sc["faces"])
    pts = np.concatenate([sc["points"], corner], 1)
    wts = np.concatenate([sc["weights"], np.ones(corner.shape[:2], F32)], 1)
    faces, V = sc["faces"], sc["verts"].shape[1]
    near64, near32 = FT.search(pts, sc["verts"], faces, F64, ("case", name)), FT.search(pts, sc["verts"], faces, F32, ("case", name))
    face32 = np.stack([n["face"] for n in near32])
    t32 = FT.forward(pts, sc["verts"], faces, face32, wts, TAU2, F32)
    t64 = FT.forward(pts, sc["verts"], faces, face32, wts, TAU2, F64, inlier=t32["inlier"])
    keys = FT.group(face32, t32["inlier"], len(faces))
    g32, g64 = FT.gradients(t32, keys, faces, V, 1.0, F32), FT.gradients(t64, keys, faces, V, 1.0, F64)
    return dict(points=pts, weights=wts, verts=sc["verts"], faces=faces, V=V, near64=near64, near32=near32, face32=face32, t32=t32, t64=t64, keys=keys,
                g32=g32, g64=g64, bounds=FT.error_bounds(t64, sc["verts"], faces, face32, pts, keys, V))


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_input_covers_every_part_and_the_twin_alone_leaves_out_few_points(name):
    """What the GPU tests assume of their input, checked from the twin alone: 195 vertices, 360 faces, F = 3; every part 0 .. 6 occurs in the
    float32 search; at most 10 % of the points are unsafe to compare index by index; points beyond the truncation distance exist; no
    inlier decision lies within the distance bound of tau2."""
    c = case(name)
    assert c["verts"].shape == (3, 195, 3) and c["faces"].shape == (360, 3) and c["points"].shape == (3, 312, 3)
    for f in range(3):
        census = np.bincount(c["near32"][f]["part"], minlength=7)
        assert (census > 0).all() and len(census) == 7, (name, f, census)
        unsafe = ~PT.safe_to_compare(c["near64"][f])
        assert unsafe.mean() <= 0.10, (name, f, unsafe.mean())
        assert len(np.unique(c["face32"][f])) > 60 and (np.bincount(c["face32"][f]) > 3).any()
    t = c["t32"]
    beyond = t["usable"] & (t["wt"] > 0) & ~t["inlier"]
    assert beyond.sum() >= 10 and (t["wt"] == 0).sum() > 100 and len(set(t["count"])) > 1
    assert (np.abs(c["t64"]["dist2"] - TAU2) > c["bounds"]["dist2"]).all()               # float32 cannot decide an inlier otherwise
    assert np.array_equal(c["t64"]["inlier"], FT.point_terms(c["points"], c["verts"], c["faces"], c["face32"], c["weights"], TAU2, F64)["inlier"])


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_twin_weights_sum_to_one_and_give_the_search_its_point(name):
    c = case(name)
    for dt, t, near, tol in ((F64, c["t64"], None, 4 * 2.0 ** -53), (F32, c["t32"], c["near32"], 4 * FT.EPS32)):
        assert t["bary"].dtype == dt and (np.abs(t["bary"].sum(-1) - 1) <= tol).all()           # (1 - v) - w, v, w: two roundings apart from 1
        assert (t["bary"] >= -tol).all() and (t["bary"] <= 1 + tol).all()
    # float32: the same bits as the float32 search, distance and part; the residual is q - that point
    for f in range(3):
        n = c["near32"][f]
        assert np.array_equal(c["t32"]["dist2"][f].view(np.int32), n["dist2"].view(np.int32)) and np.array_equal(c["t32"]["part"][f], n["part"])
        assert np.array_equal((c["points"][f] - n["point"]).view(np.int32), c["t32"]["resid"][f].view(np.int32))
    # float64, on the float64 search's own faces: the weighted corners are the search's point, the residual its distance
    face64 = np.stack([n["face"] for n in c["near64"]])
    t = FT.point_terms(c["points"], c["verts"], c["faces"], face64, None, np.inf, F64)
    tri = c["verts"].astype(F64)[np.arange(3)[:, None, None], c["faces"][face64]]
    point = (t["bary"][..., None] * tri).sum(2)
    want = np.stack([n["point"] for n in c["near64"]])
    assert np.abs(point - want).max() < 1e-15 and np.abs(t["dist2"] - np.stack([n["dist2"] for n in c["near64"]])).max() == 0
    assert np.abs((c["points"] - point) - t["resid"]).max() < 1e-15


def test_twin_groups_by_face_then_index():
    rng = np.random.default_rng(0)
    face = rng.integers(-1, 40, (3, 500))
    inlier = rng.random((3, 500)) < 0.6
    keys = FT.group(face, inlier, 40)
    for f in range(3):
        n = int((inlier[f] & (face[f] >= 0)).sum())
        k = keys[f, :n].astype(np.int64)
        assert (keys[f, n:] == FT.NO_KEY).all() and (np.diff(k) > 0).all()
        kf, ki = k >> 15, k & 32767
        pairs = sorted((int(face[f, i]), i) for i in range(500) if inlier[f, i] and face[f, i] >= 0)
        assert list(zip(kf.tolist(), ki.tolist())) == pairs
    # the largest key of the domain equals the fill: told apart by the count alone
    face = np.full((1, 32768), 131071)
    assert FT.group(face, np.ones((1, 32768), bool), 131072)[0, -1] == FT.NO_KEY


def test_twin_tree_sum_adds_everything_once():
    x = np.arange(1, 3001, dtype=F64)
    assert FT.tree_sum(FT.lane_sums(x)) == x.sum() and FT.tree_sum(FT.lane_sums(x[:1])) == 1 and FT.tree_sum(FT.lane_sums(x[:0])) == 0
    y = np.random.default_rng(1).random(2500).astype(F32)
    s = FT.tree_sum(FT.lane_sums(y))
    assert s.dtype == F32 and abs(float(s) - y.astype(F64).sum()) <= (3 + 6 + 15) * FT.EPS32 * y.astype(F64).sum()


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_twin_vertex_gradients_sum_to_minus_the_point_gradients(name):
    """Translating the mesh equals translating the points the other way: per frame and coordinate the vertex gradients add up to minus the
    point gradients.  Term by term ((gs w) u + (gs w) v + (gs w) w') r = -(gp w) r up to the weights' sum (1 within 2 roundings) and three
    roundings per product, so in either dtype |sum| <= n (5 + n_v) e * max|term| with n = 3 * inliers terms on the vertex side (each
    added into a vertex sum of at most n_v terms, then summed here in float64) -- evaluated with the sum of |terms| in place of n max|term|."""
    c = case(name)
    for dt, t, (gv, gp), e in ((F64, c["t64"], c["g64"], 2.0 ** -53), (F32, c["t32"], c["g32"], FT.EPS32)):
        assert gv.dtype == dt and gp.dtype == dt and gv.shape == (3, 195, 3) and gp.shape == c["points"].shape
        total = gv.astype(F64).sum(1) + gp.astype(F64).sum(1)
        mag = np.abs(gp.astype(F64)).sum(1)                                  # sum over the inliers of |gp w r|: the vertex side is the same, split in three
        n_v = max(int(np.bincount(c["faces"][c["face32"][f][t["inlier"][f]]].reshape(-1), minlength=195).max()) for f in range(3))
        bound = (5 + n_v) * e * mag
        print(f"{name} {np.dtype(dt).name}: worst |sum gv + sum gp| / bound {np.max(total_ratio(total, bound)):.3g} (longest vertex sum {n_v} terms)")
        assert (np.abs(total) <= bound).all()
        assert (gp[~t["inlier"]] == 0).all() and np.isfinite(gv).all()


def total_ratio(total, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, np.abs(total) / bound, 0.0)


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_twin_float32_replay_stays_within_the_derived_bounds_of_float64(name):
    c = case(name)
    t32, t64, b = c["t32"], c["t64"], c["bounds"]
    worst = {}
    for k, got, want, bound in (("bary", t32["bary"], t64["bary"], b["bary"]), ("resid", t32["resid"], t64["resid"], b["resid"][..., None]),
                                ("dist2", t32["dist2"], t64["dist2"], b["dist2"]), ("sums", t32["sums"], t64["sums"], b["sums"]),
                                ("loss", t32["loss"], t64["loss"], b["loss"]), ("W", t32["W"], t64["W"], b["W"]),
                                ("grad_verts", c["g32"][0], c["g64"][0], b["grad_verts"]), ("grad_points", c["g32"][1], c["g64"][1], b["grad_points"])):
        diff = np.abs(np.asarray(got, F64) - np.asarray(want, F64))
        bound = np.broadcast_to(bound, diff.shape)
        assert (diff <= bound).all(), k
        worst[k] = float(total_ratio(diff, bound).max())
    print(name, "worst |fp32 - float64| / bound:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert b["bary"].max() < 0.02 and b["resid"].max() < 2e-3 and b["loss"] < 1e-3 * float(t64["loss"])     # the bounds say something


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_twin_float64_gradient_equals_central_differences_of_the_truncated_loss(name):
    """Central differences (h = 1e-6) of the whole truncated, weighted float64 loss in 25 vertices x 3 coordinates and 25 points x 3
    coordinates per frame, over the points that are safe to compare and not within rounding of tau2 (the rest get weight 0), once with the
    faces held fixed and, for a tenth of the coordinates, with the nearest face searched again at both displaced positions.
    Measured on these scenes, relative to the largest gradient entry: 2.3e-10 (faces fixed, 'ragged') and 8.8e-11 (searched again); the tolerance is
    100 times the worse of the two, 2.3e-8.  (The truncation error of the difference quotient is h^2 * third derivative / 6, far below.)"""
    c = case(name)
    pts, v0, faces, V = c["points"].astype(F64), c["verts"].astype(F64), c["faces"], c["V"]
    safe = np.stack([PT.safe_to_compare(n) for n in c["near64"]]) & (np.abs(c["t64"]["dist2"] - TAU2) > 1e-6)
    wts = np.where(safe, c["weights"], 0).astype(F64)
    face = np.stack([n["face"] for n in c["near64"]])
    t = FT.forward(pts, v0, faces, face, wts, TAU2, F64)
    gv, gp = FT.gradients(t, FT.group(face, t["inlier"], len(faces)), faces, V, 1.0, F64)
    assert t["inlier"].sum() > 500

    W = float(t["W"])

    def frame_loss(f, p, v, again):
        """Frame f's share of the loss at displaced points / vertices of that frame (the other frames' terms do not move)."""
        fc = PT.nearest_on_mesh(p, v, faces)["face"][None] if again else face[f:f + 1]
        return float(FT.forward(p[None], v[None], faces, fc, wts[f:f + 1], TAU2, F64)["sums"][0, 0]) / W

    rng = np.random.default_rng(7)
    h, scale, worst = 1e-6, max(np.abs(gv).max(), np.abs(gp).max()), [0.0, 0.0]
    for f in range(3):
        touched = np.unique(faces[face[f][t["inlier"][f]]])
        for which, grad, idx in (("v", gv, rng.choice(touched, 25, replace=False)), ("p", gp, rng.choice(np.nonzero(t["inlier"][f])[0], 25, replace=False))):
            for n_, i in enumerate(idx):
                for k in range(3):
                    again = (n_ * 3 + k) % 10 == 0
                    plus, minus = [pts[f].copy(), v0[f].copy()], [pts[f].copy(), v0[f].copy()]
                    plus[which == "v"][i, k] += h
                    minus[which == "v"][i, k] -= h
                    cd = (frame_loss(f, *plus, again) - frame_loss(f, *minus, again)) / (2 * h)
                    worst[again] = max(worst[again], abs(cd - grad[f, i, k]) / scale)
    print(f"{name}: central differences vs the twin's gradient, relative to the largest entry {scale:.3g}: faces fixed {worst[0]:.3g}, searched again {worst[1]:.3g}")
    assert worst[0] <= 2.3e-8 and worst[1] <= 2.3e-8


def test_twin_zero_weight_sum_gives_zero_loss_and_gradients():
    c = case("small")
    t = FT.forward(c["points"], c["verts"], c["faces"], c["face32"], np.zeros_like(c["weights"]), TAU2, F32)
    gv, gp = FT.gradients(t, FT.group(c["face32"], t["inlier"], 360), c["faces"], 195, 1.0, F32)
    assert t["W"] == 0 and t["loss"] == 0 and not t["inlier"].any() and (gv == 0).all() and (gp == 0).all() and (t["count"] == 0).all()

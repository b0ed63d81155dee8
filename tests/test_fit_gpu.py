"""The point-to-surface loss kernels (csrc/fit/fit.hip) against the numpy twin of include/g4d_fit.h (tests/fit_twin.py): the distance has the
search's bits; EVERY bit of bary, resid, dist2, inlier, the frame sums, W, the loss, the sorted keys and both gradients equals the twin's
fp32 replay on the faces the search reported, and all of it stays within the derived bounds of float64 -- on inputs that cover every part of the
classification, at point counts around the wave, the lane count and the sort's limit, with the edge contents the header names -- and whole
calls: repeatable, capturable in a graph, the closed loop with scan.py, one backward through the model's refinement head."""
import types

import numpy as np
import pytest
import torch

import fit_twin as FT
import postprocess_twin as PT
from garment4d_amd import _lib, fit, postprocess, scan, tuning
from garment4d_amd import synthetic as syn
from test_fit_cpu import TAU2, TRUNC, case, total_ratio

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(got, want, what):
    g, w = _bits(np.asarray(got)), _bits(np.asarray(want, np.asarray(got).dtype))
    assert g.shape == w.shape and np.array_equal(g, w), (what, g.shape, w.shape, np.argwhere(g != w)[:5] if g.shape == w.shape else None)


def run(points, verts, faces, weights=None, tau2=np.inf, grad_out=1.0, face=None):
    """The search and the three functional calls on numpy inputs -> dict of numpy outputs (face: skip the search and take these)."""
    pts, v = dev(np.asarray(points, F32)), dev(np.asarray(verts, F32))
    w = dev(np.asarray(weights, F32)) if weights is not None else None
    V, nf = v.shape[1], len(faces)
    near = postprocess.nearest_on_mesh(pts, v, faces)
    fc = near.face if face is None else dev(np.asarray(face, np.int32))
    faces_dev = postprocess.mesh_topology(faces, V, v.device)["faces"]
    terms = fit.point_face_terms(pts, v, faces_dev, fc, w, tau2)
    keys = fit.group_by_face(fc, terms.inlier, nf)
    gv, gp = fit.vertex_gradient(terms, keys, dev(np.array([grad_out], F32)), fit.vertex_corner_table(faces, V, v.device), V, w, want_points=True)
    torch.cuda.synchronize()
    out = {k: host(getattr(terms, k)) for k in terms._fields}
    out.update(keys=host(keys).view(np.uint32), grad_verts=host(gv), grad_points=host(gp), face=host(fc), near_dist2=host(near.dist2), near_face=host(near.face),
               near_part=host(near.part))
    return out


def assert_equals_replay(out, points, verts, faces, weights, tau2, grad_out=1.0):
    """Every output equals the twin's fp32 replay on the faces the kernels worked on, bit for bit.  Returns the replay."""
    V = np.asarray(verts).shape[1]
    t = FT.forward(points, verts, faces, out["face"], weights, tau2, F32)
    for k in ("bary", "resid", "dist2", "sums"):
        same_bits(out[k], t[k], k)
    same_bits(out["inlier"], t["inlier"].astype(np.int32), "inlier")
    same_bits(out["count"], t["count"], "count")
    same_bits(out["total"], np.array([t["W"], t["loss"]], F32), "total")
    keys = FT.group(out["face"], t["inlier"], len(faces))
    same_bits(out["keys"], keys, "keys")
    gv, gp = FT.gradients(t, keys, faces, V, grad_out, F32)
    same_bits(out["grad_verts"], gv, "grad_verts")
    same_bits(out["grad_points"], gp, "grad_points")
    t["keys"], t["grad_verts"], t["grad_points"] = keys, gv, gp
    return t


# ------------------------------------------------------------------------------------------------------------- the search's bits, the twin's bits
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_distance_has_the_search_bits_and_everything_equals_the_twin(name):
    """The input of tests/test_fit_cpu.py's case(): 300 scattered points per frame (40 of them around and beyond the rims) plus 12 past corners.
    Census: every part 0 .. 6 occurs in every frame.  Face indices are compared with the float64 search only where it says that is safe
    (at most 10 % of the points are left out: test_fit_cpu.py checks the twin's own share)."""
    c = case(name)
    out = run(c["points"], c["verts"], c["faces"], c["weights"], TAU2, grad_out=0.75)
    # search bits: for every point
    same_bits(out["dist2"], out["near_dist2"], "dist2 against the search's")
    for f in range(3):
        census = np.bincount(out["near_part"][f], minlength=7)
        assert len(census) == 7 and (census > 0).all(), (name, f, census)
    t32 = assert_equals_replay(out, c["points"], c["verts"], c["faces"], c["weights"], TAU2, 0.75)
    assert np.array_equal(t32["part"], out["near_part"]) and len(set(out["count"])) > 1
    # the faces: the float64 search's wherever that is safe to say
    safe = np.stack([PT.safe_to_compare(n) for n in c["near64"]])
    face64 = np.stack([n["face"] for n in c["near64"]])
    feat64 = np.stack([n["feature"] for n in c["near64"]])
    feat = np.stack([PT.feature_of(c["faces"], out["face"][f], out["near_part"][f]) for f in range(3)])
    assert (~safe).mean() <= 0.10 and np.array_equal(feat[safe], feat64[safe])
    agree = safe & (out["face"] == face64)
    assert agree.mean() > 0.85
    # float64: within the bounds derived from the operation counts (per point where the faces agree; the sums over everything)
    t64 = FT.forward(c["points"], c["verts"], c["faces"], out["face"], c["weights"], TAU2, F64, inlier=out["inlier"])
    g64 = FT.gradients(t64, t32["keys"], c["faces"], c["V"], 0.75, F64)
    b = FT.error_bounds(t64, c["verts"], c["faces"], out["face"], c["points"], t32["keys"], c["V"], 0.75)
    assert np.array_equal(t64["inlier"], FT.point_terms(c["points"], c["verts"], c["faces"], out["face"], c["weights"], TAU2, F64)["inlier"])
    worst = {}
    for k, got, want, bound, mask in (("bary", out["bary"], t64["bary"], b["bary"], agree[..., None]), ("resid", out["resid"], t64["resid"], b["resid"][..., None], agree[..., None]),
                                      ("dist2", out["dist2"], t64["dist2"], b["dist2"], agree), ("sums", out["sums"], t64["sums"], b["sums"], True),
                                      ("W", out["total"][0], t64["W"], b["W"], True), ("loss", out["total"][1], t64["loss"], b["loss"], True),
                                      ("grad_verts", out["grad_verts"], g64[0], b["grad_verts"], True),
                                      ("grad_points", out["grad_points"], g64[1], b["grad_points"], agree[..., None])):
        diff = np.abs(np.asarray(got, F64) - np.asarray(want, F64))
        bound, mask = np.broadcast_to(bound, diff.shape), np.broadcast_to(mask, diff.shape)
        assert (diff[mask] <= bound[mask]).all(), k
        worst[k] = float(total_ratio(diff, bound)[mask].max())
    print(name, "worst |kernel - float64| / bound:", {k: f"{v:.3g}" for k, v in worst.items()})


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_autograd_function_gives_the_functional_bits(name):
    c = case(name)
    out = run(c["points"], c["verts"], c["faces"], c["weights"], TAU2, grad_out=1.0)
    pts, v = dev(c["points"]).requires_grad_(True), dev(c["verts"]).requires_grad_(True)
    res = fit.point_mesh_distance(pts, v, c["faces"], dev(c["weights"]), TRUNC)
    res.loss.backward()
    torch.cuda.synchronize()
    assert res.loss.shape == () and res.per_frame.shape == (3, 3) and res.rms.shape == (3,) and res.inliers.dtype == torch.int32
    same_bits(host(res.loss), out["total"][1], "loss")
    same_bits(host(res.inliers), out["count"], "inliers")
    same_bits(host(res.per_frame), np.stack([out["sums"][:, 0], out["sums"][:, 1], out["count"].astype(F32)], 1), "per_frame")
    same_bits(host(res.nearest.face), out["near_face"], "nearest.face")
    same_bits(host(v.grad), out["grad_verts"], "verts.grad")
    same_bits(host(pts.grad), out["grad_points"], "points.grad")
    rms = np.sqrt(out["sums"][:, 0].astype(F64) / out["sums"][:, 1])
    assert np.abs(host(res.rms) - rms).max() <= 4 * FT.EPS32 * rms.max() and (rms < TRUNC).all() and (rms > 1e-3).all()
    # only the mesh asks for a gradient: the points get none, the vertices the same bits; a scaled loss scales on the device
    v2 = dev(c["verts"]).requires_grad_(True)
    (fit.point_mesh_distance(dev(c["points"]), v2, c["faces"], dev(c["weights"]), TRUNC).loss * 0.75).backward()
    same_bits(host(v2.grad), run(c["points"], c["verts"], c["faces"], c["weights"], TAU2, grad_out=0.75)["grad_verts"], "verts.grad at 0.75")


# ------------------------------------------------------------------------------------------------------------------------------ edge sizes
@pytest.mark.parametrize("P", [1, 63, 64, 65, 300, 32768])
def test_point_counts_around_the_wave_and_up_to_the_sort_limit(P):
    """P = 1, one below / at / one above a wave, 300 (no power of two: the sort pads), 32768: the sort's LDS limit (128 KB of keys, 32 points per
    lane of the forward), against the 360-face mesh -- about 90 points per face, hundreds on some."""
    sc = FT.fit_scene("ragged", P=P, seed=P)
    out = run(sc["points"], sc["verts"], sc["faces"], sc["weights"], TAU2, grad_out=1.25)
    same_bits(out["dist2"], out["near_dist2"], "dist2 against the search's")
    t = assert_equals_replay(out, sc["points"], sc["verts"], sc["faces"], sc["weights"], TAU2, 1.25)
    assert out["keys"].shape == (3, P)
    if P >= 63:
        assert (t["count"] > P // 3).all() and (t["count"] < P).all() and np.abs(out["grad_verts"]).max() > 0


# --------------------------------------------------------------------------------------------------------------------------- edge contents
def test_every_point_on_one_face_and_duplicate_points():
    """200 points above ONE face (three threads walk the whole run), 60 of them copies of the first: the order within the face is the index."""
    c = case("small")
    verts, faces = c["verts"], c["faces"]
    rng = np.random.default_rng(3)
    g = 100
    pts = np.zeros((3, 200, 3), F32)
    for f in range(3):
        tri = verts[f][faces[g]].astype(F64)
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        bc = rng.dirichlet([4.0, 4.0, 4.0], 200)
        pts[f] = (bc @ tri + n / np.linalg.norm(n) * rng.uniform(0.001, 0.004, (200, 1))).astype(F32)
        pts[f, 140:] = pts[f, 0]
    face = np.full((3, 200), g, np.int32)
    out = run(pts, verts, faces, None, TAU2, face=face)
    t = assert_equals_replay(out, pts, verts, faces, None, TAU2)
    assert (t["count"] == 200).all() and (out["keys"] == (g << 15) + np.arange(200)).all()
    touched = np.zeros(195, bool)
    touched[faces[g]] = True
    assert (out["grad_verts"][:, ~touched] == 0).all() and (np.abs(out["grad_verts"][:, touched]).max(-1) > 0).all()
    same_bits(out["grad_points"][:, 140:], np.broadcast_to(out["grad_points"][:, :1], (3, 60, 3)), "copies of a point get its gradient")
    # and through the search: whatever face it picks, the same bits as the replay
    out = run(pts, verts, faces, None, TAU2)
    assert_equals_replay(out, pts, verts, faces, None, TAU2)


def test_zero_weights_tiny_truncation_no_truncation_and_a_nan_point():
    c = case("ragged")
    pts, verts, faces, wts = c["points"], c["verts"], c["faces"], c["weights"]
    # all weights 0: W == 0, zeros everywhere, no NaN
    out = run(pts, verts, faces, np.zeros_like(wts), TAU2)
    assert_equals_replay(out, pts, verts, faces, np.zeros_like(wts), TAU2)
    assert (out["total"] == 0).all() and (out["count"] == 0).all() and (out["grad_verts"] == 0).all() and (out["grad_points"] == 0).all()
    assert (out["keys"] == 0xFFFFFFFF).all() and not out["inlier"].any()
    # a truncation distance below every distance: nothing is an inlier, W stays the sum of all weights
    out = run(pts, verts, faces, wts, 1e-12)
    assert_equals_replay(out, pts, verts, faces, wts, 1e-12)
    assert out["total"][0] == wts.sum() and out["total"][1] == 0 and (out["count"] == 0).all() and (out["grad_verts"] == 0).all()
    # none: every weighted point with a face is an inlier
    out = run(pts, verts, faces, wts, np.inf)
    t = assert_equals_replay(out, pts, verts, faces, wts, np.inf)
    assert np.array_equal(out["count"], (wts > 0).sum(1)) and out["total"][1] > 0
    res = fit.point_mesh_distance(dev(pts), dev(verts), faces, dev(wts), trunc=None)
    same_bits(host(res.loss), t["loss"], "trunc=None")
    # a NaN point: no face, excluded; its neighbours and the sums stay finite
    bad = pts.copy()
    bad[1, 7] = np.nan
    bad[2, 0, 1] = np.nan
    out = run(bad, verts, faces, wts, TAU2)
    assert_equals_replay(out, bad, verts, faces, wts, TAU2)
    assert out["face"][1, 7] == -1 and out["inlier"][1, 7] == 0 and out["dist2"][1, 7] == np.inf and (out["grad_points"][1, 7] == 0).all()
    assert np.isfinite(out["total"]).all() and np.isfinite(out["grad_verts"]).all() and np.isfinite(out["sums"]).all()
    # a NaN distance handed in with a face (not the search's doing): never an inlier
    face = out["face"].copy()
    face[2, 0] = 5
    out = run(bad, verts, faces, None, np.inf, face=face)
    assert np.isnan(out["dist2"][2, 0]) and out["inlier"][2, 0] == 0 and np.isfinite(out["total"]).all() and np.isfinite(out["grad_verts"]).all()


def test_zero_area_mesh_and_an_isolated_vertex():
    """A mesh of zero-area triangles only.  The search classifies a query against such a triangle like any other: a triangle collapsed to a
    point or a segment is a vertex or an edge region with a finite distance, and only an interior classification with den == 0 gives the NaN
    that never wins.  So these meshes do get faces -- and the loss on them must still equal the replay and stay finite.  The face -1 the
    search reports when NOTHING can win is reached with a frame whose vertices are NaN: every point of it is excluded, W still counts it."""
    c = case("small")
    pts, wts = c["points"][:, :100], c["weights"][:, :100]
    flat = np.array([[0, 0, 1], [2, 2, 2], [3, 4, 3]], np.int32)
    out = run(pts, c["verts"], flat, wts, np.inf)
    assert_equals_replay(out, pts, c["verts"], flat, wts, np.inf)
    same_bits(out["dist2"], out["near_dist2"], "dist2 against the search's")
    usable = out["face"] >= 0
    assert np.isfinite(out["total"]).all() and np.isfinite(out["grad_verts"]).all() and np.isfinite(out["dist2"][usable]).all()
    assert np.array_equal(out["inlier"] != 0, usable & (wts > 0)) and (out["grad_verts"][:, 5:] == 0).all()
    lost = c["verts"].copy()
    lost[1] = np.nan
    out = run(pts, lost, c["faces"], wts, np.inf)
    assert_equals_replay(out, pts, lost, c["faces"], wts, np.inf)
    assert (out["face"][1] == -1).all() and not out["inlier"][1].any() and (out["dist2"][1] == np.inf).all() and (out["bary"][1] == 0).all() and (out["resid"][1] == 0).all()
    assert out["count"][1] == 0 and (out["sums"][1] == [0, 0, wts[1].sum()]).all() and (out["grad_verts"][1] == 0).all() and (out["grad_points"][1] == 0).all()
    assert out["total"][0] == wts.sum() and out["total"][1] > 0 and np.isfinite(out["grad_verts"]).all() and np.abs(out["grad_verts"][0]).max() > 0
    # a vertex no face names (and one past the faces' range of vertices): gradient 0, everything else as without it
    verts = np.concatenate([c["verts"], c["verts"][:, :2] + 0.01], 1)
    faces = c["faces"].copy()
    out = run(pts, verts, faces, wts, TAU2)
    t = assert_equals_replay(out, pts, verts, faces, wts, TAU2)
    assert out["grad_verts"].shape == (3, 197, 3) and (out["grad_verts"][:, 195:] == 0).all() and np.abs(out["grad_verts"][:, :195]).max() > 0
    ref = run(pts, c["verts"], c["faces"], wts, TAU2)
    same_bits(out["grad_verts"][:, :195], ref["grad_verts"], "the isolated vertices change nothing")
    assert t["count"].sum() > 100


def test_outside_the_domain_raises_before_any_launch():
    face = torch.zeros((1, 32769), dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.G4DError, match=r"g4d_fit_group_f32: p must be <= 32768 \(p=32769\)"):
        fit.group_by_face(face, face, 360)
    with pytest.raises(_lib.G4DError, match=r"g4d_fit_group_f32: nf must be <= 131072 \(nf=131073\)"):
        fit.group_by_face(face[:, :100], face[:, :100], 131073)
    c = case("small")
    pts = dev(np.resize(c["points"][:1], (1, 32769, 3)))
    v = dev(c["verts"][:1]).requires_grad_(True)
    res = fit.point_mesh_distance(pts, v, c["faces"], trunc=TRUNC)            # the forward has no such limit ...
    assert torch.isfinite(res.loss) and int(res.inliers[0]) > 1000
    with pytest.raises(_lib.G4DError, match="p must be <= 32768"):           # ... the backward does
        res.loss.backward()
    torch.cuda.synchronize()
    assert v.grad is None


# --------------------------------------------------------------------------------------------------------------------------- whole calls
def test_two_runs_give_the_same_bits():
    sc = FT.fit_scene("small", P=5000, seed=9)
    a = run(sc["points"], sc["verts"], sc["faces"], sc["weights"], TAU2)
    b = run(sc["points"], sc["verts"], sc["faces"], sc["weights"], TAU2)
    for k in a:
        same_bits(a[k], b[k], k)
    assert np.abs(a["grad_verts"]).max() > 0


def test_captured_functional_calls_replay_to_the_eager_bits():
    """The three functional calls on one stream in a hipGraph, replayed on three inputs: the eager bits each time."""
    sets = [FT.fit_scene("ragged", P=700, seed=s) for s in (1, 2, 3)]
    faces = sets[0]["faces"]
    V, nf = 195, len(faces)

    def calls(pts, v, w, face, g, faces_dev, table):
        terms = fit.point_face_terms(pts, v, faces_dev, face, w, TAU2)
        keys = fit.group_by_face(face, terms.inlier, nf)
        return (*terms, keys, *fit.vertex_gradient(terms, keys, g, table, V, w, want_points=True))

    static = [dev(sets[0][k]) for k in ("points", "verts", "weights")]
    g = dev(np.array([0.5], F32))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        face = postprocess.nearest_on_mesh(static[0], static[1], faces).face.clone()       # eager first: the tables are built on the host once
        faces_dev, table = postprocess.mesh_topology(faces, V, face.device)["faces"], fit.vertex_corner_table(faces, V, face.device)
        calls(*static, face, g, faces_dev, table)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = calls(*static, face, g, faces_dev, table)
    for s in (1, 2, 1):
        new = [dev(sets[s][k]) for k in ("points", "verts", "weights")]
        new_face = postprocess.nearest_on_mesh(new[0], new[1], faces).face
        for dst, src in zip(static + [face], new + [new_face]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [host(o) for o in outs]
        want = [host(o) for o in calls(*new, new_face, g, faces_dev, table)]
        for i, (a, b) in enumerate(zip(got, want)):
            same_bits(a, b, (s, i))
    assert not np.array_equal(sets[1]["points"], sets[2]["points"]) and np.abs(got[-2]).max() > 0


def test_timed_calls_sees_the_fit_entry_points():
    c = case("small")
    v = dev(c["verts"]).requires_grad_(True)
    with _lib.timed_calls() as t:
        fit.point_mesh_distance(dev(c["points"]), v, c["faces"], trunc=TRUNC).loss.backward()
    names = [r[0] for r in t.results()]
    assert names[-3:] == ["g4d_fit_point_face_f32", "g4d_fit_group_f32", "g4d_fit_vertex_grad_f32"] and "g4d_mesh_nearest_f32" in names


def test_closed_loop_a_mesh_fits_its_own_scan():
    """scan.scan_meshes of a posed cylinder, then that same mesh against its scan.  A scan point is the fp32 unprojection of a point ON its
    face: it lies within the bound tests/scan_twin.py derives (`err`) of that face -- checked in float64 --, so its fp32 squared distance to
    that face is at most |err|^2 plus the rounding of the distance itself (FT.error_bounds' dist2); the search minimises that same fp32
    distance over all faces, so what it reports is no larger -- exactly.  The gradient: a vertex entry is at most (2 / W) * the sum of its frame's distances."""
    import test_scan_gpu as TS
    verts, faces = TS._cylinder_meshes(2)
    N = 300
    want = TS.twin_scan_of_meshes(verts, faces, TS.CAMERAS, N, 4)
    s = scan.scan_meshes(dev(verts), faces, TS.CAMERAS, TS.SIZE, N, seed=4)
    pts = host(s.points)
    assert np.array_equal(host(s.face), want["face"]) and (want["face"] >= 0).all()
    on_own = run(pts, verts, faces, None, np.inf, face=want["face"])          # the distance to the face each point was unprojected from
    out = run(pts, verts, faces, None, np.inf)
    assert (out["dist2"] <= on_own["dist2"]).all()
    t64 = FT.forward(pts, verts, faces, want["face"], None, np.inf, F64)
    keys = FT.group(want["face"], t64["inlier"], len(faces))
    b = FT.error_bounds(t64, verts, faces, want["face"], pts, keys, verts.shape[1])
    own64, err = np.sqrt(t64["dist2"]), np.linalg.norm(want["err"], axis=-1)
    assert (own64 <= err).all() and err.max() < 1e-4                          # float64: the scan's bound alone
    assert (np.abs(on_own["dist2"].astype(F64) - t64["dist2"]) <= b["dist2"]).all()
    limit2 = err ** 2 + b["dist2"]                                            # fp32: plus the rounding of the distance itself
    dist = np.sqrt(out["dist2"].astype(F64))
    print(f"closed loop: largest distance {dist.max():.3g} (float64, to the own face: {own64.max():.3g}), largest unprojection bound {err.max():.3g}, "
          f"worst distance / bound {(own64 / err).max():.3g}, worst kernel dist2 / its bound {(out['dist2'] / limit2).max():.3g}; "
          f"largest gradient entry {np.abs(out['grad_verts']).max():.3g}")
    assert (out["dist2"] <= limit2).all() and (out["count"] == N).all()
    W = float(out["total"][0])
    assert W == 2 * N and out["total"][1] <= limit2.mean() * (1 + 1e-5)
    cap = 2.0 / W * dist.sum(1) * (1 + 1e-5)
    assert (np.abs(out["grad_verts"]).max((1, 2)) <= cap).all() and cap.max() <= err.max()
    res = fit.point_mesh_distance(s.points, dev(verts), faces, trunc=0.05)
    assert float(res.rms.max()) <= np.sqrt(limit2.max()) and int(res.inliers.min()) == N


def test_scan_fit_loss_trains_the_head_and_nothing_of_the_encoder():
    """One scan_fit_loss(...).backward() on the small synthetic scene of tests/test_stage2_loss_gpu.py under tuning.refine_autograd."""
    import test_stage2_loss_gpu as S2
    nbatch, T, N, label = 2, 3, 2048, 6
    scene = syn.garment_scene(nbatch, T, N, garment_rc=(8, 8), seed=70)
    m = S2.small_model(scene)
    body = scene["body"]
    bm = types.SimpleNamespace(parents=torch.from_numpy(body["parents"]).cuda(), faces=body["faces"], J_regressor=dev(body["J_regressor"]),
                               v_template=dev(body["v_template"]))
    x, batch = dev(scene["x"]), {k: dev(v) for k, v in scene["batch"].items()}
    m.train()
    m.PCA_garment_encoder.eval()
    with tuning.use(tuning.current().replace(refine_autograd=True)):
        out = m(x, bm, batch)
    rng = np.random.default_rng(72)
    root = rng.normal(0.0, 0.02, (nbatch, T, 3)).astype(F32)
    labels = np.where(rng.random((nbatch, T, N, 1)) < 0.5, label, 0).astype(np.int32)
    inputs = dict(pcd_torch=x + dev(root)[:, :, None], pcd_label_torch=dev(labels), smpl_root_joints_torch=dev(root))
    ld = fit.scan_fit_loss(out, inputs, out["garment_f_3"], label, trunc=0.3)
    assert sorted(ld) == ["scan_fit_inliers", "scan_fit_loss", "scan_fit_rms_list"]
    assert ld["scan_fit_rms_list"].shape == (nbatch, T) and ld["scan_fit_inliers"].shape == (nbatch, T) and ld["scan_fit_inliers"].dtype == torch.int32
    assert torch.isfinite(ld["scan_fit_loss"]) and ld["scan_fit_loss"].requires_grad and float(ld["scan_fit_loss"].detach()) > 0
    assert int(ld["scan_fit_inliers"].min()) > 50 and int(ld["scan_fit_inliers"].max()) <= int((labels == label).sum((2, 3)).max())
    # the root offset is added to the prediction: the same cloud without it, against the bare prediction, gives the same faces and about the same loss
    bare = fit.point_mesh_distance(x.reshape(nbatch * T, N, 3), out["iter_regressed_lbs_garment_v"][-1].detach().reshape(nbatch * T, -1, 3), out["garment_f_3"],
                                   dev((labels == label).astype(F32).reshape(nbatch * T, N)), trunc=0.3)
    assert abs(float(bare.loss) - float(ld["scan_fit_loss"].detach())) <= 1e-3 * float(bare.loss)
    ld["scan_fit_loss"].backward()
    for name, p in m.named_parameters():
        if name.startswith("PCA_garment_encoder."):
            assert p.grad is None, name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    # an earlier round on request
    first = fit.scan_fit_loss(out, inputs, out["garment_f_3"], label, trunc=0.3, round=0)
    assert torch.isfinite(first["scan_fit_loss"]) and float(first["scan_fit_loss"].detach()) != float(ld["scan_fit_loss"].detach())

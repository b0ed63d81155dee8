"""The adjoint of the garment skinning without a GPU: the sixth (header, library) pair -- include/g4d_skin.h against its record
tests/skin_abi_snapshot.txt, libg4d_skin.so's exports, argument checks and empty problems --, the opt-in's default, and the numpy twin
(tests/garment_skin_grad_twin.py) that the GPU tests compare the kernels with: its float64 adjoint equals float64 torch autograd of its own
forward and central differences with the neighbour lists held fixed, reproduces the float64 gradients the reference's autograd gave
(tests/golden/garment_skin_grad.npz), and holds the zero-gradient rule at a coincident vertex."""
import os
import re

import numpy as np
import pytest

import garment_skin_grad_twin as GT
from conftest import ROOT, load_golden
from test_abi_cpu import _LETTERS

EINVAL = 10001
HEADER = os.path.join(ROOT, "include", "g4d_skin.h")
SKIN, BLEND = "g4d_garment_skin_grad_f32", "g4d_knn_blend_grad_f32"


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


def test_parsed_skin_header_equals_its_snapshot():
    """include/g4d_skin.h as _lib.parse_header reads it == tests/skin_abi_snapshot.txt, both ways and in the header's order, constants included."""
    from garment4d_amd import _lib
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "skin_abi_snapshot.txt")).read().splitlines()]
    recorded = dict(ln for ln in lines if ln[0].startswith("g4d_"))
    rec_consts = {ln[0]: int(ln[1]) for ln in lines if ln[0].startswith("G4D_")}
    assert all(len(ln) == 2 for ln in lines) and fields == []
    assert set(parsed) == set(_declared()) and sorted(parsed) == sorted([SKIN, BLEND])
    assert {n: (parsed.get(n), recorded.get(n)) for n in set(parsed) | set(recorded) if parsed.get(n) != recorded.get(n)} == {}
    assert list(parsed) == list(recorded)
    assert consts == rec_consts == {"G4D_SKIN_MAX_K": 256, "G4D_SKIN_MAX_JOINTS": 64}


def test_skin_library_exports_every_declared_symbol_and_leaves_the_other_five_pairs_alone():
    from garment4d_amd import _lib
    assert os.path.exists(_lib.SKIN_LIB_PATH), "run __graft_entry__.build() first"
    L, protos, consts = _lib.skin_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
    others = (_lib.PROTOTYPES, _lib.render_lib()[1], _lib.scan_lib()[1], _lib.fit_lib()[1], _lib.smpl_lib()[1])
    assert not any(n in (SKIN, BLEND) for protos_ in others for n in protos_)
    assert len(_lib.render_lib()[1]) == 4 and len(_lib.scan_lib()[1]) == 3 and len(_lib.fit_lib()[1]) == 4 and len(_lib.smpl_lib()[1]) == 4
    assert not any(k.startswith("G4D_SKIN") for lib_ in (_lib.render_lib(), _lib.scan_lib(), _lib.fit_lib(), _lib.smpl_lib()) for k in lib_[2])
    assert not any(k.startswith("G4D_SKIN") for k in _lib.CONSTANTS)
    for other in (_lib.lib(), _lib.render_lib()[0], _lib.scan_lib()[0], _lib.fit_lib()[0], _lib.smpl_lib()[0]):
        assert not hasattr(other, SKIN) and not hasattr(other, BLEND)
    assert _lib.lib().g4d_version() == 263                                    # libg4d_hip.so's ABI is the parent's
    assert _lib.skin_lib()[0] is L                                            # loaded once
    assert _lib._entry(BLEND) is getattr(L, BLEND) and _lib._entry("g4d_knn_blend_weights_f32") is getattr(_lib.lib(), "g4d_knn_blend_weights_f32")


def _skin_args(clips=2, T=3, vg=5, j=24, W=1, per_clip=0, A=1, verts=1, d_out=1, d_add=0, d_verts=1, d_W=1):
    return (clips, T, vg, j, W, per_clip, A, verts, d_out, d_add, d_verts, d_W, 0)


def _blend_args(frames=6, T=3, vg=5, v=40, k=8, ldk=None, j=24, W=1, idx=1, dists=1, d_blend=1, pts=1, ref=1, d_add=0, d_pts=1):
    return (frames, T, vg, v, k, k if ldk is None else ldk, j, W, idx, dists, d_blend, pts, ref, d_add, d_pts, 0)


def test_argument_validation_needs_no_gpu():
    """Every check of include/g4d_skin.h comes before any launch: G4D_EINVAL with the entry point's name in the ONE error state."""
    from garment4d_amd import _lib
    L, _, _ = _lib.skin_lib()
    main = _lib.lib()
    bad = [(SKIN, _skin_args, kw, needle) for kw, needle in
           [(dict(clips=-1), "bad sizes"), (dict(vg=-1), "bad sizes"), (dict(T=0), "frames_per_clip >= 1"), (dict(j=0), "1 <= J <= 64"), (dict(j=65), "1 <= J <= 64"),
            (dict(W=0), "null"), (dict(A=0), "null"), (dict(verts=0), "null"), (dict(d_out=0), "null")]]
    bad += [(BLEND, _blend_args, kw, needle) for kw, needle in
            [(dict(frames=-1), "bad sizes"), (dict(vg=-1), "bad sizes"), (dict(T=0), "frames_per_clip >= 1"), (dict(frames=7), "multiple of frames_per_clip"),
             (dict(k=0), "1 <= K <= 256"), (dict(k=257), "1 <= K <= 256"), (dict(k=8, ldk=7), "ldk >= K"), (dict(j=0), "1 <= J <= 64"), (dict(j=65), "1 <= J <= 64"),
             (dict(v=0), "V >= 1")] + [({k: 0}, "null") for k in ("W", "idx", "dists", "d_blend", "pts", "ref", "d_pts")]]
    for name, args, kw, needle in bad:
        rc = getattr(L, name)(*args(**kw))
        assert rc == EINVAL, (name, kw, rc)
        msg = main.g4d_last_error().decode()                                  # libg4d_hip.so's accessor: one error state for the six libraries
        assert name in msg and needle in msg, (kw, msg)
        with pytest.raises(_lib.G4DError, match=name):
            _lib.call(name, *args(**kw))
    # the domain is checked on an empty problem too, and before the pointers
    assert L.g4d_knn_blend_grad_f32(*_blend_args(frames=0, k=257)) == EINVAL and L.g4d_garment_skin_grad_f32(*_skin_args(clips=0, j=65, W=0)) == EINVAL


def test_empty_problems_return_ok_and_touch_nothing():
    from garment4d_amd import _lib
    L, _, _ = _lib.skin_lib()
    none_s = dict(W=0, A=0, verts=0, d_out=0, d_verts=0, d_W=0)
    for kw in (dict(clips=0), dict(vg=0), dict(clips=0, vg=0, per_clip=1)):
        assert L.g4d_garment_skin_grad_f32(*_skin_args(**{**none_s, **kw})) == 0, kw
    assert L.g4d_garment_skin_grad_f32(*_skin_args(d_verts=0, d_W=0)) == 0     # nothing asked for: nothing launched
    none_b = dict(W=0, idx=0, dists=0, d_blend=0, pts=0, ref=0, d_pts=0)
    for kw in (dict(frames=0), dict(vg=0), dict(frames=0, vg=0)):
        assert L.g4d_knn_blend_grad_f32(*_blend_args(**{**none_b, **kw})) == 0, kw
    assert _lib.call(BLEND, *_blend_args(**{**none_b, "vg": 0})) == 0


def test_garment_lbs_autograd_defaults_to_off(monkeypatch):
    from garment4d_amd import tuning
    assert tuning.Tuning().garment_lbs_autograd is False
    monkeypatch.delenv("G4D_GARMENT_LBS_AUTOGRAD", raising=False)
    assert tuning.from_environment().garment_lbs_autograd is False
    monkeypatch.setenv("G4D_GARMENT_LBS_AUTOGRAD", "1")
    assert tuning.from_environment().garment_lbs_autograd is True
    with tuning.use(tuning.current().replace(garment_lbs_autograd=True)):
        assert tuning.current().garment_lbs_autograd is True
    assert tuning.current().garment_lbs_autograd is tuning.DEFAULT.garment_lbs_autograd


def _recorded_interpolation(monkeypatch):
    """lbs_garment_interpolation with every launch replaced by a recorder (no GPU): the argument tensors of a tiny scene on the CPU."""
    import torch
    from garment4d_amd import _lib, garment_lbs as GL, gcn, knn as KN, lbs as L, synthetic as syn
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name) or 0)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(L, "_f32", lambda t, name: t.contiguous())

    def knn_points(p1, p2, K=1):
        B, Vg = p1.shape[:2]
        return KN.KNN(dists=torch.ones(B, Vg, K), idx=torch.zeros(B, Vg, K, dtype=torch.long), knn=None)
    monkeypatch.setattr(GL, "knn_points", knn_points)
    monkeypatch.setattr(GL, "_smoothing_csr", lambda adj, dev: (torch.zeros(1, dtype=torch.int32),) * 2 + (torch.zeros(1), adj.shape[0], 4))
    sc = syn.garment_scene(1, 2, 4, body_rc=(5, 6), garment_rc=(4, 4), seed=3)
    b = {k: torch.from_numpy(v) for k, v in sc["batch"].items()}
    gv, gq = sc["template"]
    adj_old = gcn.adjacency_old_from_faces(gq, gv.shape[0])
    x = torch.from_numpy(gv[None].copy())
    args = lambda x_, **kw: (x_, kw.get("tv", b["Tpose_smpl_vertices_torch"]), b["Tpose_smpl_root_joints_torch"], b["zeropose_smpl_vertices_torch"],
                             torch.from_numpy(sc["body"]["parents"]), kw.get("pose", b["pose_torch"]), b["T_J_regressor"], b["T_lbs_weights"], adj_old)
    return GL, calls, x, args, b


def test_flag_off_a_grad_requiring_call_is_left_without_a_graph_exactly_as_before(monkeypatch):
    import torch
    from garment4d_amd import tuning
    GL, calls, x, args, b = _recorded_interpolation(monkeypatch)
    assert tuning.current().garment_lbs_autograd is False
    with torch.no_grad():
        GL.lbs_garment_interpolation(*args(x), K=3)
    plain = list(calls)
    assert "g4d_knn_blend_weights_f32" in plain and "g4d_jacobi_smooth_f32" in plain and plain.count("g4d_lbs_pose_skin_f32") == 2
    del calls[:]
    posed, nn1, stage1 = GL.lbs_garment_interpolation(*args(x.clone().requires_grad_(True)), K=3)
    assert calls == plain                                                     # the same launches in the same order
    assert posed.grad_fn is None and stage1.grad_fn is None and not posed.requires_grad and not stage1.requires_grad
    # ... and a grad-requiring body is not looked at either
    GL.lbs_garment_interpolation(*args(x, tv=b["Tpose_smpl_vertices_torch"].clone().requires_grad_(True)), K=3)


def test_flag_on_same_launches_a_graph_and_refusals(monkeypatch):
    import torch
    from garment4d_amd import tuning
    GL, calls, x, args, b = _recorded_interpolation(monkeypatch)
    with torch.no_grad():
        GL.lbs_garment_interpolation(*args(x), K=3)
    plain = list(calls)
    del calls[:]
    with tuning.use(tuning.current().replace(garment_lbs_autograd=True)):
        xr = x.clone().requires_grad_(True)
        posed, nn1, stage1 = GL.lbs_garment_interpolation(*args(xr), K=3)
        assert calls == plain
        assert posed.grad_fn is not None and stage1.grad_fn is not None and tuple(stage1.shape) == tuple(posed.shape)
        assert not nn1.dists.requires_grad and not nn1.idx.requires_grad
        with torch.no_grad():
            assert GL.lbs_garment_interpolation(*args(xr), K=3)[0].grad_fn is None       # grad off: no graph
        assert GL.lbs_garment_interpolation(*args(x), K=3)[0].grad_fn is None            # nothing requires grad: no graph
        for kw in (dict(tv=b["Tpose_smpl_vertices_torch"].clone().requires_grad_(True)), dict(pose=b["pose_torch"].clone().requires_grad_(True))):
            with pytest.raises(NotImplementedError, match="only pred_template_garment_v is differentiated"):
                GL.lbs_garment_interpolation(*args(xr, **kw), K=3)


# ------------------------------------------------------------------------------------------------------------------------- the twin
CASES = [dict(), dict(per_clip=True), dict(K=1), dict(K=70, V=90, J=24, Vg=7, T=1), dict(B=1, K=3, J=24, seed=4)]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "base")
def test_twin_adjoint_equals_float64_torch_autograd_of_its_forward(kw):
    """To float64 rounding: 1e-12 of the largest entry (observed <= 1e-15 .. 5e-15 of gradients of size 5 .. 7)."""
    import torch
    x, c = GT.make_case(**kw)
    rng = np.random.default_rng(1)
    y, u, _ = GT.forward(x, c)
    dy, du = rng.standard_normal(y.shape), rng.standard_normal(u.shape)
    for a, b in ((dy, du), (dy, None), (None, du)):
        mine, want = GT.adjoint(x, c, a, b), GT.torch_grad(x, c, a, b, torch.float64)
        err = np.abs(mine - want).max() / np.abs(want).max()
        print(f"{kw} dy={a is not None} du={b is not None}: twin vs float64 autograd, relative {err:.3g}")
        assert mine.shape == x.shape and err <= 1e-12
    if kw.get("K") == 1:                                                      # one neighbour: weight 1 whatever the distance
        _, _, s = GT.forward(x, c)
        assert (GT.blend_grad(c["Wt"], s["T"], c["idx"], s["d"], rng.standard_normal(s["nn_W"].shape), s["g"], c["body"]) == 0).all()


def test_twin_adjoint_equals_central_differences_with_the_lists_held_fixed():
    """Central differences, h = 1e-6, of L = sum(posed dy) + sum(u du) in 40 entries of x with idx fixed.  The quotient's rounding is
    eps |L| / h ~ 1e-16 * 30 / 1e-6 = 3e-9 absolute, the truncation h^2 f''' / 6 ~ 1e-12 f''': the tolerance is 1e-7 of the largest entry."""
    x, c = GT.make_case()
    rng = np.random.default_rng(2)
    y, u, _ = GT.forward(x, c)
    dy, du = rng.standard_normal(y.shape), rng.standard_normal(u.shape)
    grad = GT.adjoint(x, c, dy, du)

    def loss(x_):
        y_, u_, _ = GT.forward(x_, c)
        return (y_ * dy).sum() + (u_ * du).sum()
    h, worst = 1e-6, 0.0
    for i in rng.choice(x.size, 40, replace=False):
        p, m = x.copy(), x.copy()
        p.reshape(-1)[i] += h
        m.reshape(-1)[i] -= h
        worst = max(worst, abs((loss(p) - loss(m)) / (2 * h) - grad.reshape(-1)[i]) / np.abs(grad).max())
    print(f"central differences vs the twin's adjoint, relative: {worst:.3g}")
    assert worst <= 1e-7


def test_twin_reproduces_the_golden_float64_gradients():
    """On both golden cases (K = 3, K = 256; the second clip's pose all zero) the twin's float64 adjoint, given the neighbour lists and the float64
    transforms the reference computed, equals the float64 autograd of the reference's own lbs_garment_interpolation to 1e-11 of the largest
    entry (100 smoothing steps as spmm there, as dense products here)."""
    g = load_golden("garment_skin_grad.npz")
    case = GT.golden_case()
    assert (case["batch"]["pose_torch"][1] == 0).all() and (case["batch"]["pose_torch"][0] != 0).any()
    B, T, Vg = case["nbatch"], case["T"], case["Vg"]
    x = case["tpose_garment"].astype(np.float64)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "garment_skin_grad.npz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "smpl_grad.npz")) // 2
    for K in (3, 256):
        c = GT.golden_constants(case, g, K)
        assert c["idx"].shape == (B, Vg, K)
        _, _, s = GT.forward(x, c)
        assert (s["d"] > 0).all()                                             # no coincident vertex in the golden
        dy, ds = case["dy"].reshape(B * T, Vg, 3).astype(np.float64), case["ds"].astype(np.float64).sum(1)
        for name, du in (("posed", None), ("both", ds)):
            got, want = GT.adjoint(x, c, dy, du), g[f"k{K}_{name}_dx64"]
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"golden K={K} {name}: twin vs the reference's float64 autograd, relative {err:.3g}; reference fp32 error {float(g[f'k{K}_{name}_eref']):.3g}")
            assert got.shape == want.shape and err <= 1e-11 and float(g[f"k{K}_{name}_eref"]) > 0


def test_a_coincident_vertex_has_a_finite_gradient_by_the_zero_rule():
    """Garment vertex (0, 3) placed exactly on its nearest body vertex: d_0 = 0, the forward weight of that neighbour is 0, torch autograd of the
    restatement gives NaN there (0 * inf in reciprocal's backward).  The twin's gradient is finite, equals autograd at every other vertex, and
    at the coincident vertex equals the (smooth) gradient of the same problem with that neighbour REMOVED from the vertex's list -- checked
    without the smoothing, where a vertex's gradient depends on its own list alone; with the smoothing it is checked to be finite."""
    import torch
    for smooth_it in (False, True):
        x, c = GT.make_case(K=8, smooth_it=smooth_it)
        x = x.copy()
        x[0, 3] = c["body"][0, c["idx"][0, 3, 0]] - c["root"][0]
        assert ((x + c["root"][:, None])[0, 3] == c["body"][0, c["idx"][0, 3, 0]]).all()
        rng = np.random.default_rng(3)
        y, u, s = GT.forward(x, c)
        assert s["d"][0, 3, 0] == 0 and (s["d"][0, 3, 1:] > 0).all() and np.isfinite(y).all()
        dy, du = rng.standard_normal(y.shape), rng.standard_normal(u.shape)
        mine = GT.adjoint(x, c, dy, du)
        auto = GT.torch_grad(x, c, dy, du, torch.float64)
        assert np.isfinite(mine).all() and np.isnan(auto[0, 3]).all()
        if smooth_it:
            continue
        keep = np.ones(x.shape[:2], bool)
        keep[0, 3] = False
        assert np.abs(mine[keep] - auto[keep]).max() <= 1e-12 * np.abs(mine).max()
        sub = dict(c, idx=c["idx"][:, 3:4, 1:])                               # vertex 3 alone, its nearest neighbour dropped
        want = GT.torch_grad(x[:, 3:4], sub, dy[:, 3:4], du[:, 3:4], torch.float64)
        assert np.isfinite(want).all() and np.abs(mine[0, 3] - want[0, 0]).max() <= 1e-12 * np.abs(want).max()

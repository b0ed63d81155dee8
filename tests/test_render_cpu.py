"""The rasterizer without a GPU: the second (header, library) pair -- include/g4d_render.h against its record tests/render_abi_snapshot.txt,
libg4d_render.so's exports and argument checks -- and the properties of the numpy twin (tests/render_twin.py) that the GPU tests compare the
kernels with: exact watertightness, winding independence, the top-left rule's counts, the tie rule, fp32 replay within the derived bounds."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_twin as RT
from conftest import ROOT
from test_abi_cpu import _LETTERS

EINVAL = 10001
HEADER = os.path.join(ROOT, "include", "g4d_render.h")


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


def test_parsed_render_header_equals_its_snapshot():
    """include/g4d_render.h as _lib.parse_header reads it == tests/render_abi_snapshot.txt, both ways and in the header's order (the letters
    of tests/test_abi_cpu.py); the constants the kernels and the twin share are recorded with it."""
    from garment4d_amd import _lib
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "render_abi_snapshot.txt")).read().splitlines()]
    recorded = dict(ln for ln in lines if ln[0].startswith("g4d_"))
    rec_consts = {ln[0]: int(ln[1]) for ln in lines if ln[0].startswith("G4D_")}
    assert all(len(ln) == 2 for ln in lines) and fields == []
    assert set(parsed) == set(_declared()) and len(parsed) == 4
    assert {n: (parsed.get(n), recorded.get(n)) for n in set(parsed) | set(recorded) if parsed.get(n) != recorded.get(n)} == {}
    assert list(parsed) == list(recorded)
    assert consts == rec_consts
    assert consts["G4D_RENDER_COORD_BITS"] == 22 and (1 << 22) == RT.COORD_LIMIT and consts["G4D_RENDER_SUBSAMPLE_BITS"] == 8


def test_render_library_exports_every_declared_symbol_and_leaves_the_first_pair_alone():
    from garment4d_amd import _lib
    assert os.path.exists(_lib.RENDER_LIB_PATH), "run __graft_entry__.build() first"
    L, protos, consts = _lib.render_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
    assert L.g4d_render_chunk() >= 64 and consts["G4D_RENDER_TILE"] == 16
    # g4d.h's names keep their meaning: nothing of the second pair leaks into them
    assert not any(n.startswith("g4d_render") for n in _lib.PROTOTYPES) and _lib.HEADER_PATH.endswith("g4d.h") and _lib.LIB_PATH.endswith("libg4d_hip.so")
    assert not hasattr(_lib.lib(), "g4d_render_raster") and _lib.lib().g4d_version() == 263
    assert _lib.render_lib()[0] is L                                        # loaded once


def test_ws_bytes_query():
    from garment4d_amd import _lib
    L, _, _ = _lib.render_lib()
    assert L.g4d_render_ws_bytes(0, 100) == 0 and L.g4d_render_ws_bytes(3, 0) == 0
    up16 = lambda n: (n + 15) // 16 * 16
    want = lambda frames, nf: up16(frames * nf * 8) + up16(frames * -(-nf // L.g4d_render_chunk()) * 8) + frames * nf * 96
    assert L.g4d_render_ws_bytes(1, 1) == 16 + 16 + 96 == want(1, 1) and L.g4d_render_ws_bytes(3, 1000) == want(3, 1000)
    assert L.g4d_render_ws_bytes(240, 22000) == want(240, 22000) > 1 << 29                # size_t, not int
    assert L.g4d_render_ws_bytes(-1, 4) == ctypes.c_size_t(-1).value


_CAM = (1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 30.0, 0.1)


def _project_args(frames=1, v=8, w=16, h=16, ss=2, cam=_CAM, verts=1, px=1, py=1, invz=1):
    return (frames, v, 0, verts) + tuple(cam) + (w, h, ss, px, py, invz, 0, 0)


def _raster_args(frames=1, v=8, nf=4, w=16, h=16, ss=2, px=1, py=1, invz=1, faces=1, faces_host=0, face_rgb=0, vert_rgb=0, ws=16, ws_bytes=1 << 20,
                 face_id=1, depth=1):
    return (frames, v, nf, w, h, ss, 1, px, py, invz, 0, faces, faces_host, face_rgb, vert_rgb, 0.0, 1.0, 0.0, 0.5, 0.5, 0.0, 0.0, 0.0, ws, ws_bytes,
            face_id, depth, 0, 0, 0)


def test_render_argument_validation_needs_no_gpu():
    """Every check of include/g4d_render.h comes before any launch: the invalid-argument status with the entry point's name in the ONE error
    state, g4d_last_error() of libg4d_hip.so -- through _lib.call, which raises G4DError with that text."""
    from garment4d_amd import _lib
    L, _, _ = _lib.render_lib()
    main = _lib.lib()
    host_faces = np.array([[0, 1, 2], [2, 3, 8]], np.int32)                  # 8 is outside [0, 8)
    neg_faces = np.array([[0, 1, -1]], np.int32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad = [
        ("g4d_render_project_f32", _project_args(frames=-1), "negative"),
        ("g4d_render_project_f32", _project_args(ss=3), "ss must be"),
        ("g4d_render_project_f32", _project_args(w=2049, ss=2), "<= 4096"),
        ("g4d_render_project_f32", _project_args(h=1025, ss=4), "<= 4096"),
        ("g4d_render_project_f32", _project_args(verts=0), "null"),
        ("g4d_render_project_f32", _project_args(invz=0), "null"),
        ("g4d_render_project_f32", _project_args(cam=_CAM[:10] + (0.0,)), "near > 0"),
        ("g4d_render_project_f32", _project_args(cam=(1.0, 0.0, -1.0, 1.0, 0.0, -1.0) + _CAM[6:]), "coincide"),
        ("g4d_render_project_f32", _project_args(cam=(0.0, 2.0, 0.0) + _CAM[3:]), "parallel"),
        ("g4d_render_raster", _raster_args(nf=-1), "negative"),
        ("g4d_render_raster", _raster_args(v=-2), "negative"),
        ("g4d_render_raster", _raster_args(ss=0), "ss must be"),
        ("g4d_render_raster", _raster_args(ss=8), "ss must be"),
        ("g4d_render_raster", _raster_args(w=4097, ss=1), "<= 4096"),
        ("g4d_render_raster", _raster_args(h=1025, ss=4), "<= 4096"),
        ("g4d_render_raster", _raster_args(px=0), "null"),
        ("g4d_render_raster", _raster_args(faces=0), "null"),
        ("g4d_render_raster", _raster_args(face_id=0), "null"),
        ("g4d_render_raster", _raster_args(depth=0), "null"),
        ("g4d_render_raster", _raster_args(ws=0), "null"),
        ("g4d_render_raster", _raster_args(ws_bytes=32 + 16 + 4 * 96 - 1), "workspace"),
        ("g4d_render_raster", _raster_args(ws=24), "aligned"),
        ("g4d_render_raster", _raster_args(face_rgb=1, vert_rgb=1), "not both"),
        ("g4d_render_raster", _raster_args(nf=2, faces_host=hp(host_faces)), "outside [0, 8)"),
        ("g4d_render_raster", _raster_args(nf=1, faces_host=hp(neg_faces)), "outside [0, 8)"),
    ]
    for name, args, needle in bad:
        rc = getattr(L, name)(*args)
        assert rc == EINVAL, (name, needle, rc)
        msg = main.g4d_last_error().decode()                                 # libg4d_hip.so's accessor: one error state for both libraries
        assert name.split("_f32")[0] in msg and needle.lower() in msg.lower(), (name, needle, msg)
        with pytest.raises(_lib.G4DError, match=name):
            _lib.call(name, *args)
    # an in-range host copy passes the check (and the call then stops at the next one, not at the faces)
    assert L.g4d_render_raster(*_raster_args(nf=1, faces_host=hp(np.array([[0, 1, 7]], np.int32)), ws=0)) == EINVAL
    assert "null" in main.g4d_last_error().decode()


def test_empty_render_problems_return_zero():
    from garment4d_amd import _lib
    L, _, _ = _lib.render_lib()
    for kw in (dict(frames=0), dict(w=0), dict(h=0)):
        assert L.g4d_render_raster(*_raster_args(**kw)) == 0, kw
        assert L.g4d_render_project_f32(*_project_args(**kw)) == 0, kw
    assert L.g4d_render_raster(*_raster_args(frames=0, nf=0, px=0, py=0, invz=0, faces=0, ws=0, face_id=0, depth=0)) == 0
    assert L.g4d_render_project_f32(*_project_args(v=0, verts=0, px=0, py=0, invz=0)) == 0
    assert _lib.call("g4d_render_raster", *_raster_args(frames=0)) == 0


def test_call_traces_and_times_the_second_library_without_a_second_copy(capfd, monkeypatch):
    """G4D_TRACE_CALLS and the status -> G4DError conversion are call()'s own: an entry point of libg4d_render.so goes through the same lines."""
    from garment4d_amd import _lib
    _lib.render_lib()
    monkeypatch.setattr(_lib, "_TRACE", True)
    assert _lib.call("g4d_render_raster", *_raster_args(frames=0, w=20, h=12)) == 0
    assert "g4d call g4d_render_raster 0 8 4 20 12 2 1" in capfd.readouterr().err
    assert _lib._entry("g4d_render_chunk") is getattr(_lib.render_lib()[0], "g4d_render_chunk")
    assert _lib._entry("g4d_version") is getattr(_lib.lib(), "g4d_version")


# ------------------------------------------------------------------------------------------------------------------------ twin properties
def _grid_scene(ws=33, hs=17, seed=0):
    px, py, faces = RT.watertight_grid(8, 8, ws, hs, seed=seed)
    invz = (0.5 + np.random.default_rng(seed + 1).random(len(px))).astype(np.float32)
    return px, py, invz, faces


def test_twin_watertight_grid_gives_every_sample_exactly_one_face():
    """A jittered triangulated grid of 128 faces with random windings, reaching beyond a 33 x 17 screen, four vertices exactly on sample
    centres: the top-left rule in integers leaves no sample uncovered and none covered twice."""
    for seed in range(4):
        px, py, invz, faces = _grid_scene(seed=seed)
        assert len(faces) == 128 and ((px - 128) % 256 == 0).sum() >= 4
        r = RT.raster(px, py, invz, faces, 33, 17, shade=False)
        assert r["oriented"]["drawn"].all()
        assert (r["ncover"] == 1).all(), (seed, np.argwhere(r["ncover"] != 1)[:5])
        assert (r["face_id"] >= 0).all()
        # the four on-centre vertices: the sample under each is covered once although six faces meet there
        on = np.nonzero(((px - 128) % 256 == 0) & ((py - 128) % 256 == 0) & (px > 0) & (py > 0) & (px < 33 * 256) & (py < 17 * 256))[0]
        assert len(on) >= 1
        for v in on:
            assert r["ncover"][(py[v] - 128) // 256, (px[v] - 128) // 256] == 1


def test_twin_coverage_ignores_vertex_order():
    px, py, invz, faces = _grid_scene(seed=5)
    want = RT.raster(px, py, invz, faces, 33, 17, shade=False)
    for perm in ([1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]):
        got = RT.raster(px, py, invz, faces[:, perm], 33, 17, shade=False)
        assert np.array_equal(got["face_id"], want["face_id"]) and np.array_equal(got["ncover"], want["ncover"]), perm


@pytest.mark.parametrize("n", [1, 2, 5, 16])
def test_twin_right_triangle_covers_what_the_top_left_rule_predicts(n):
    """Legs of n samples along the axes.  Corners on sample CORNERS: centre (i, j) is inside iff i + j + 1 < n -> n (n - 1) / 2.  Corners on
    sample CENTRES: the top and the left leg own their samples, the hypotenuse does not -> i + j < n, n (n + 1) / 2; mirrored to the right /
    bottom, the legs are a right and a bottom edge and own nothing while the hypotenuse, now a left edge, does: i, j < n <= i + j -> n (n - 1) / 2."""
    iz = np.ones(3, np.float32)
    f = np.array([[0, 1, 2]])
    count = lambda x, y: int((RT.raster(np.array(x), np.array(y), iz, f, 40, 40, shade=False)["face_id"] == 0).sum())
    L = 256 * n
    assert count([512, 512 + L, 512], [512, 512, 512 + L]) == n * (n - 1) // 2
    assert count([640, 640 + L, 640], [640, 640, 640 + L]) == n * (n + 1) // 2
    assert count([640 + L, 640, 640 + L], [640 + L, 640 + L, 640]) == n * (n - 1) // 2


def test_twin_coincident_faces_give_the_lower_index_and_the_nearer_face_wins():
    x, y = np.array([300, 5000, 300, 5000]), np.array([300, 300, 5000, 5000])
    iz = np.array([1, 1, 1, 1], np.float32)
    same = RT.raster(x, y, iz, np.array([[3, 3, 3], [0, 1, 2], [2, 1, 0], [0, 1, 2]]), 24, 24, shade=False)      # face 0 has no area
    assert not same["oriented"]["drawn"][0] and set(np.unique(same["face_id"])) == {-1, 1} and same["ncover"].max() == 3
    # two faces through each other: the one with the larger invz at a sample is seen there, and both are seen somewhere
    x2, y2 = np.array([300, 5000, 300, 300, 5000, 300]), np.array([300, 300, 5000, 300, 300, 5000])
    iz2 = np.array([2, 1, 1, 1, 2, 2], np.float32)
    r = RT.raster(x2, y2, iz2, np.array([[0, 1, 2], [3, 4, 5]]), 24, 24, shade=False)
    assert set(np.unique(r["face_id"])) == {-1, 0, 1} and (r["ncover"][r["face_id"] >= 0] == 2).all()


def _random_scene(seed, V=40, nf=60, w=24, h=16, ss=2):
    rng = np.random.default_rng(seed)
    verts = (rng.random((V, 3)) - 0.5).astype(np.float32) * np.array([1.2, 1.0, 0.8], np.float32)
    faces = rng.integers(0, V, (nf, 3)).astype(np.int32)
    cam = RT.camera((1.06, 0.2, -1.06), (0, 0, 0), (0, 1, 0), 30.0, w, h, ss)
    return verts, faces, cam, w, h, ss


@pytest.mark.parametrize("seed", range(4))
def test_twin_fp32_replay_lies_within_the_derived_bounds_of_float64(seed):
    verts, faces, cam, w, h, ss = _random_scene(seed)
    px, py, invz, c = RT.project_f32(verts, cam, 0.1)
    fx, fy, q, efx, efy, eq = RT.project_f64(verts, cam)
    assert (invz > 0).all() and np.isfinite(efx).all()
    assert (np.abs(px - fx) <= 0.5 + efx).all() and (np.abs(py - fy) <= 0.5 + efy).all() and (efx < 0.5).all()
    assert (np.abs(invz.astype(np.float64) - q) <= eq).all() and (eq <= 1e-5 * q).all()
    rng = np.random.default_rng(seed)
    light = RT.light_in_camera(cam, (0, 1, 0))
    for colours in ({}, dict(face_rgb=rng.random((len(faces), 3)).astype(np.float32)), dict(vert_rgb=rng.random((len(verts), 3)).astype(np.float32))):
        r = RT.raster(px, py, invz, faces, ss * w, ss * h, ss, cam=c, light=light, ambient=0.5, directional=0.5, bg=(0.1, 0.2, 0.3), **colours)
        seen = r["face_id"] >= 0
        assert seen.sum() > 100 and r["image"].shape == (h, w, 3) and r["image"].dtype == np.float32
        assert (np.abs(r["iz"].astype(np.float64) - r["iz64"]) <= r["err_iz"])[seen].all()
        assert (np.abs(r["image"].astype(np.float64) - r["image64"]) <= r["err_image"]).all()
        assert np.isfinite(r["err_image"]).all() and np.median(r["err_image"]) < 1e-5


def test_error_colours_follow_the_reference_ramp():
    """utils/post_processing.py:260-269 on numpy against render.error_colours (CPU tensors: plain torch arithmetic)."""
    import torch
    from garment4d_amd import render
    rng = np.random.default_rng(0)
    pred, gt = rng.random((2, 50, 3)).astype(np.float32), rng.random((2, 50, 3)).astype(np.float32)
    value = np.linalg.norm(pred - gt, axis=-1).reshape(-1, 1)
    lo, hi = 0.1, 0.9
    ratio = 2 * (value - lo) / (hi - lo)
    b = (255 * (1 - ratio)).astype(np.int32)
    r = (255 * (ratio - 1)).astype(np.int32)
    b[b < 0] = 0
    r[r < 0] = 0
    want = np.concatenate([r, 255 - b - r, b], 1).reshape(2, 50, 3)
    got = render.error_colours(torch.from_numpy(pred), torch.from_numpy(gt), lo, hi).numpy() * 255
    near_step = np.abs(255 * (1 - ratio) - np.rint(255 * (1 - ratio))).reshape(2, 50) < 1e-3     # float32 vs float64 at an integer step
    assert np.abs(got - want)[~near_step].max() < 1e-3


def test_look_at_camera_is_the_reference_eye():
    from garment4d_amd import render
    c = render.look_at_camera(1.5, 0, 45)
    np.testing.assert_allclose(c.eye, (1.5 * np.sin(np.pi / 4), 0.0, -1.5 * np.cos(np.pi / 4)), atol=1e-12)
    assert c.at == (0.0, 0.0, 0.0) and c.up == (0.0, 1.0, 0.0) and c.half_angle == 30.0
    R = render.camera_rotation(c)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    np.testing.assert_allclose(R, RT.camera(c.eye, c.at, c.up, 30.0, 4, 4, 1)["R"], atol=1e-7)

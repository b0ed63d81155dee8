"""The rasterizer's kernels (csrc/render/raster.hip) against the numpy twin of include/g4d_render.h (tests/render_twin.py).

Raster stage, from integer inputs: the face id and the depth BITS of every sample equal the twin's fp32 replay -- no sample is exempt -- and the
image stays within the bound the twin derives for |fp32 - float64| given those face ids.  Projection stage: snapped coordinates, invz and
camera-space bits equal the replay, and stay within half a fixed-point unit plus the derived bound of float64.  Whole calls: repeatable,
independent of the culling, capturable in a graph, and render_output on a model's own output dict."""
import numpy as np
import pytest
import torch

import render_twin as RT
from garment4d_amd import _lib, render
from garment4d_amd import synthetic as syn

pytestmark = pytest.mark.gpu

LIGHT = (np.array([0.3, 0.8, -0.5]) / np.linalg.norm([0.3, 0.8, -0.5])).astype(np.float32)
BG = (0.125, 0.25, 0.5)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_raster(px, py, invz, faces, w, h, ss, cam=None, face_rgb=None, vert_rgb=None, cull=True):
    """px, py, invz (F,V), cam (F,V,3) numpy -> the kernel's result, compared with the twin frame by frame.  Returns (Rendered on the host, twins)."""
    px, py, invz = np.asarray(px, np.int32), np.asarray(py, np.int32), np.asarray(invz, np.float32)
    opt = lambda a: None if a is None else dev(np.asarray(a, np.float32))
    got = render.rasterize(dev(px), dev(py), dev(invz), faces, (w, h), ss, cam=opt(cam), face_colours=opt(face_rgb), vertex_colours=opt(vert_rgb),
                           light=LIGHT, ambient=0.5, directional=0.5, background=BG, cull=cull)
    torch.cuda.synchronize()
    image, depth, ids = got.image.cpu().numpy(), got.depth.cpu().numpy(), got.face_id.cpu().numpy()
    assert image.shape == (len(px), h, w, 3) and depth.shape == ids.shape == (len(px), ss * h, ss * w) and ids.dtype == np.int32
    twins = []
    for f in range(len(px)):
        t = RT.raster(px[f], py[f], invz[f], faces, ss * w, ss * h, ss, cam=None if cam is None else cam[f], light=LIGHT, ambient=0.5, directional=0.5,
                      face_rgb=face_rgb, vert_rgb=vert_rgb, bg=BG)
        assert np.array_equal(ids[f], t["face_id"]), (f, np.argwhere(ids[f] != t["face_id"])[:5])
        assert np.array_equal(_bits(depth[f]), _bits(t["depth"])), (f, np.argwhere(_bits(depth[f]) != _bits(t["depth"]))[:5])
        excess = np.abs(image[f].astype(np.float64) - t["image64"]) - t["err_image"]
        print(f"frame {f}: image max |kernel - float64| {np.abs(image[f] - t['image64']).max():.3g}, bound max {t['err_image'].max():.3g}, "
              f"kernel == fp32 replay: {np.array_equal(_bits(image[f]), _bits(t['image']))}")
        assert (excess <= 0).all(), (f, float(excess.max()))
        twins.append(t)
    return render.Rendered(image, depth, ids), twins


def random_scene(seed, F_, V, nf, ws, hs):
    """Random triangles in fixed-point sample coordinates reaching a fifth beyond the ws x hs screen; when there are faces, the LAST one is made
    of three extra vertices nearer than everything else, so that the face behind a chunk boundary is seen."""
    rng = np.random.default_rng(seed)
    V = V + 3
    px = rng.integers(int(-0.2 * ws * 256), int(1.2 * ws * 256), (F_, V))
    py = rng.integers(int(-0.2 * hs * 256), int(1.2 * hs * 256), (F_, V))
    invz = (0.5 + rng.random((F_, V))).astype(np.float32)
    cam = rng.standard_normal((F_, V, 3)).astype(np.float32)
    faces = rng.integers(0, V - 3, (nf, 3)).astype(np.int32)
    if nf:
        faces[-1] = [V - 3, V - 2, V - 1]
        invz[:, V - 3:] = 3.0
        px[:, V - 3:] = np.array([0.2, 0.8, 0.5]) * ws * 256
        py[:, V - 3:] = np.array([0.2, 0.4, 0.9]) * hs * 256
    return px, py, invz, cam, faces


@pytest.mark.parametrize("size", [(20, 12, 1), (20, 12, 2), (33, 17, 1), (33, 17, 2)])
@pytest.mark.parametrize("nf", [0, 1, 63, 64, 65, "chunk+1"])
def test_raster_face_counts_and_ragged_images(nf, size):
    w, h, ss = size
    nf = render.chunk() + 1 if nf == "chunk+1" else nf
    px, py, invz, cam, faces = random_scene(nf * 7 + w + ss, 1, 24, nf, ss * w, ss * h)
    got, _ = check_raster(px, py, invz, faces, w, h, ss, cam=cam)
    if nf == 0:
        assert (got.face_id == -1).all() and np.isinf(got.depth).all() and np.array_equal(got.image, np.broadcast_to(np.float32(BG), got.image.shape))
    else:
        assert (got.face_id == nf - 1).any()


@pytest.mark.parametrize("frames", [1, 3])
def test_raster_per_frame_geometry_and_colours(frames):
    w, h, ss = 33, 17, 2
    px, py, invz, cam, faces = random_scene(40 + frames, frames, 30, 90, ss * w, ss * h)
    rng = np.random.default_rng(3)
    a, _ = check_raster(px, py, invz, faces, w, h, ss, cam=cam, face_rgb=rng.random((len(faces), 3)).astype(np.float32))
    b, _ = check_raster(px, py, invz, faces, w, h, ss, cam=cam, vert_rgb=rng.random((px.shape[1], 3)).astype(np.float32))
    c, _ = check_raster(px, py, invz, faces, w, h, ss)                                    # unlit, white
    assert np.array_equal(a.face_id, b.face_id) and np.array_equal(a.face_id, c.face_id) and not np.array_equal(a.image, b.image)
    if frames > 1:
        assert not np.array_equal(a.face_id[0], a.face_id[1])


def test_raster_256_at_two_samples_per_pixel_edge():
    w = h = 256
    ss = 2
    gx, gy, gf = RT.watertight_grid(12, 12, ss * w, ss * h, seed=9, reach=0.9)           # 288 faces inside the screen, background around them
    px, py, invz, cam, faces = random_scene(11, 1, 20, 40, ss * w, ss * h)
    px, py = np.concatenate([px[0], gx])[None], np.concatenate([py[0], gy])[None]
    rng = np.random.default_rng(12)
    invz = np.concatenate([invz[0], (0.5 + rng.random(len(gx))).astype(np.float32)])[None]
    cam = np.concatenate([cam[0], rng.standard_normal((len(gx), 3)).astype(np.float32)])[None]
    faces = np.concatenate([gf + 23, faces]).astype(np.int32)
    got, _ = check_raster(px, py, invz, faces, w, h, ss, cam=cam)
    assert (got.face_id == -1).any() and len(np.unique(got.face_id)) > 50


def test_raster_watertight_grid_reaching_beyond_the_screen():
    """Every sample gets exactly one face of the grid (vertices on sample centres included): none is background, and the kernel's ids are the twin's."""
    w, h, ss = 33, 17, 1
    for seed in (0, 1):
        px, py, faces = RT.watertight_grid(8, 8, w, h, seed=seed)
        invz = (0.5 + np.random.default_rng(seed).random(len(px))).astype(np.float32)
        got, twins = check_raster(px[None], py[None], invz[None], faces, w, h, ss)
        assert (twins[0]["ncover"] == 1).all() and (got.face_id >= 0).all()
    px, py, faces = RT.watertight_grid(8, 8, 40, 24, seed=2)                               # the same at 2 x 2 samples per pixel
    invz = np.ones(len(px), np.float32)
    got, twins = check_raster(px[None], py[None], invz[None], faces, 20, 12, 2)
    assert (twins[0]["ncover"] == 1).all() and (got.face_id >= 0).all()


def edge_case_scene(ws, hs):
    """One frame with every documented drop and tie: returns px, py, invz, faces and the indices of the faces that must never be seen."""
    big = 1 << 22
    P = [  # (x, y, invz)
        (300, 300, 1), (5000, 300, 1), (300, 5000, 1), (5000, 5000, 1),                  # 0-3   a square
        (300, 300, 2), (5000, 300, .5), (300, 5000, .5),                                 # 4-6   through the next one
        (300, 300, .5), (5000, 300, 2), (300, 5000, 2),                                  # 7-9
        (2650, 300, 1),                                                                  # 10    on the line 0-1
        (-5000, 100, 1), (-3000, 200, 1), (-4000, 3000, 1),                              # 11-13 left of the screen
        (3000, 3000, 0), (3000, 3000, -1), (3000, 3000, np.nan), (3000, 3000, np.inf),   # 14-17 not drawable: behind near, behind the eye, ...
        (big, 3000, 1), (big - 1, 3000, 4), (RT.NO_COORD, 2000, 1),                      # 18-20 at, just inside, far past the coordinate limit
        (3000, -big, 1), (3000, -big + 1, 4),                                            # 21-22
        (ws * 256 + 1000, 500, 1), (ws * 256 + 3000, 900, 1), (ws * 256 + 2000, 4000, 1),   # 23-25 right of the screen
        (1000, hs * 256 + 200, 1), (3000, hs * 256 + 200, 1), (2000, hs * 256 + 4000, 1),   # 26-28 below it
        (4000, 1000, 3), (4100, 1000, 3), (4050, 1040, 3),                               # 29-31 a sliver between sample centres (empty box in y)
    ]
    x, y, iz = (np.array(c) for c in zip(*P))
    faces = [[0, 1, 2], [2, 1, 0], [0, 1, 2],          # 0-2 coincident: 0 is seen
             [4, 5, 6], [7, 8, 9],                     # 3-4 interpenetrating
             [0, 0, 1], [3, 3, 3], [0, 10, 1],         # 5-7 no area
             [11, 12, 13], [23, 24, 25], [26, 27, 28],  # 8-10 off screen
             [14, 1, 3], [15, 1, 3], [16, 1, 3], [17, 1, 3],   # 11-14 dropped for their invz
             [18, 1, 3], [20, 1, 2], [21, 0, 1],       # 15-17 dropped for a coordinate
             [19, 1, 3], [22, 0, 1],                   # 18-19 drawn: one unit inside the limit, nearest of all
             [29, 30, 31]]                             # 20 drawn, covers nothing
    never = [1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20]
    return x.astype(np.int64), y.astype(np.int64), iz.astype(np.float32), np.array(faces, np.int32), never


@pytest.mark.parametrize("colours", ["white", "face", "vertex"])
def test_raster_documented_drops_ties_and_interpenetration(colours):
    w, h, ss = 33, 17, 2
    x, y, iz, faces, never = edge_case_scene(ss * w, ss * h)
    rng = np.random.default_rng(5)
    cam = rng.standard_normal((1, len(x), 3)).astype(np.float32)
    kw = {"face": dict(face_rgb=rng.random((len(faces), 3)).astype(np.float32)), "vertex": dict(vert_rgb=rng.random((len(x), 3)).astype(np.float32))}.get(colours, {})
    got, twins = check_raster(x[None], y[None], iz[None], faces, w, h, ss, cam=cam, **kw)
    seen = set(np.unique(got.face_id))
    assert not seen & set(never), seen & set(never)
    assert {18, 19} <= seen and (3 in seen) and (4 in seen)                             # the two faces through each other are both seen
    drawn = twins[0]["oriented"]["drawn"]
    assert not drawn[[5, 6, 7, 11, 12, 13, 14, 15, 16, 17]].any() and drawn[[0, 1, 2, 3, 4, 8, 9, 10, 18, 19, 20]].all()


def test_raster_drops_a_face_with_an_index_outside_the_mesh_when_no_host_copy_is_given():
    """With faces_host the entry point refuses such a face (tests/test_render_cpu.py); without it the kernel must not read through the index."""
    w, h, ss, V = 20, 12, 1, 8
    px, py, invz, cam, faces = random_scene(77, 1, V - 3, 6, w, h)
    faces[1], faces[3] = [0, 1, V], [2, -1, 3]
    L, _, _ = _lib.render_lib()
    ws = _lib.workspace(L.g4d_render_ws_bytes(1, len(faces)), "cuda")
    ids = torch.full((1, h, w), -7, dtype=torch.int32, device="cuda")
    depth = torch.empty((1, h, w), dtype=torch.float32, device="cuda")
    t = [dev(px.astype(np.int32)), dev(py.astype(np.int32)), dev(invz), dev(faces)]
    _lib.call("g4d_render_raster", 1, V, len(faces), w, h, ss, 1, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, t[3].data_ptr(), None, None, None,
              0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, ws.data_ptr(), ws.numel(), ids.data_ptr(), depth.data_ptr(), None, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    want = RT.raster(px[0], py[0], invz[0], faces, w, h, shade=False)
    assert not want["oriented"]["drawn"][[1, 3]].any() and np.array_equal(ids.cpu().numpy()[0], want["face_id"])
    with pytest.raises(_lib.G4DError, match="outside"):
        render.rasterize(t[0], t[1], t[2], faces, (w, h), ss)


# ---------------------------------------------------------------------------------------------------------------------------- projection
CAMERA = render.look_at_camera(1.5, 10.0, 45.0)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("V", [1, 63, 65])
def test_projection_equals_the_replay_and_stays_within_the_float64_bound(V, shared):
    F_, w, h, ss = 3, 33, 17, 2
    rng = np.random.default_rng(V)
    verts = (rng.random((V, 3) if shared else (F_, V, 3)) - 0.5).astype(np.float32)
    if V > 1:
        flat = verts.reshape(-1, 3)
        flat[0] = np.float32(CAMERA.eye)                                                # at the eye: z = 0, the division gives inf / NaN
        flat[1] = np.float32(CAMERA.eye) * np.float32(1.2)                              # behind the eye
        flat[2] = np.float32(CAMERA.eye) * np.float32(0.95)                             # in front of it, nearer than `near`
    got = render.project(dev(verts), CAMERA, (w, h), ss, frames=F_ if shared else None)
    torch.cuda.synchronize()
    cam = RT.camera(CAMERA.eye, CAMERA.at, CAMERA.up, CAMERA.half_angle, w, h, ss)
    full = np.broadcast_to(verts, (F_, V, 3))
    px, py, invz, c = RT.project_f32(full, cam, CAMERA.near)
    assert got.px.shape == (F_, V) and np.array_equal(got.px.cpu().numpy(), px) and np.array_equal(got.py.cpu().numpy(), py)
    assert np.array_equal(_bits(got.invz.cpu().numpy()), _bits(invz))
    gc = got.cam.cpu().numpy()
    assert np.array_equal(_bits(gc)[~np.isnan(c)], _bits(c)[~np.isnan(c)])
    if V > 1:
        assert (invz[0, :3] == 0).all() and px[0, 0] == RT.NO_COORD and py[0, 0] == RT.NO_COORD
    fx, fy, q, efx, efy, eq = RT.project_f64(full, cam)
    ok = invz > 0
    assert ok.sum() >= F_ * max(V - 3, 1)
    print(f"max |px - fx64| {np.abs(px - fx)[ok].max():.3f}, bound 0.5 + {efx[ok].max():.3g}")
    assert (np.abs(px - fx) <= 0.5 + efx)[ok].all() and (np.abs(py - fy) <= 0.5 + efy)[ok].all() and (0.5 + efx[ok] <= 1.0).all()
    assert (np.abs(invz.astype(np.float64) - q) <= eq)[ok].all()


# --------------------------------------------------------------------------------------------------------------------------- whole calls
def _cylinder_meshes(F_, seed=0):
    rng = np.random.default_rng(seed)
    v, q = syn.quad_cylinder(14, 18)
    v = (v * np.array([1.4, 0.9, 1.4], np.float32) + np.array([0, -0.45, 0], np.float32)).astype(np.float32)
    faces = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 0).astype(np.int32)
    verts = (v[None] + rng.standard_normal((F_,) + v.shape).astype(np.float32) * 0.01).astype(np.float32)
    return verts, faces


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_render_meshes_is_repeatable_and_equals_the_twin():
    verts, faces = _cylinder_meshes(2)
    rng = np.random.default_rng(1)
    vc = rng.random((verts.shape[1], 3)).astype(np.float32)
    a = render.render_meshes(dev(verts), faces, CAMERA, vertex_colours=dev(vc), image_size=(40, 24), background=BG)
    b = render.render_meshes(dev(verts), faces, CAMERA, vertex_colours=dev(vc), image_size=(40, 24), background=BG)
    assert a.image.shape == (2, 24, 40, 3) and a.depth.shape == a.face_id.shape == (2, 48, 80) and _same(a, b)
    cam = RT.camera(CAMERA.eye, CAMERA.at, CAMERA.up, CAMERA.half_angle, 40, 24, 2)
    light = RT.light_in_camera(cam, render.LIGHT_DIRECTION)
    for f in range(2):
        px, py, invz, c = RT.project_f32(verts[f], cam, CAMERA.near)
        t = RT.raster(px, py, invz, faces, 80, 48, 2, cam=c, light=light, ambient=0.5, directional=0.5, vert_rgb=vc, bg=BG)
        assert np.array_equal(a.face_id[f].cpu().numpy(), t["face_id"]) and np.array_equal(_bits(a.depth[f].cpu().numpy()), _bits(t["depth"]))
        assert (np.abs(a.image[f].cpu().numpy() - t["image64"]) <= t["err_image"]).all()
        assert (t["face_id"] >= 0).mean() > 0.05 and (t["face_id"] < 0).any()
        d = a.depth[f].cpu().numpy()
        assert (d[t["face_id"] >= 0] > 0.5).all() and (d[t["face_id"] >= 0] < 2.5).all() and np.isinf(d[t["face_id"] < 0]).all()
    no_aa = render.render_meshes(dev(verts), faces, CAMERA, image_size=(40, 24), anti_aliasing=False)
    assert no_aa.face_id.shape == (2, 24, 40) and float(no_aa.image.max()) <= 1.0 and float(no_aa.image.min()) >= 0.0


def test_bits_do_not_depend_on_the_culling():
    """cull on: a tile keeps the faces whose box meets it; off: every drawn face.  The kept-face counts differ, the bits do not."""
    verts, faces = _cylinder_meshes(2, seed=3)
    p = render.project(dev(verts), CAMERA, (40, 24), 2)
    tiles = 2 * 3 * 5
    kept = [torch.zeros(tiles, dtype=torch.int32, device="cuda") for _ in range(2)]
    on = render.rasterize(p.px, p.py, p.invz, faces, (40, 24), 2, cam=p.cam, light=LIGHT, ambient=0.5, directional=0.5, cull=True, kept=kept[0])
    off = render.rasterize(p.px, p.py, p.invz, faces, (40, 24), 2, cam=p.cam, light=LIGHT, ambient=0.5, directional=0.5, cull=False, kept=kept[1])
    assert _same(on, off)
    k_on, k_off = kept[0].cpu().numpy(), kept[1].cpu().numpy()
    k_on, k_off = k_on.reshape(2, -1), k_off.reshape(2, -1)
    assert (k_off == k_off[:, :1]).all() and (k_off > 0).all() and (k_on <= k_off).all()
    assert k_on.sum() < 0.5 * k_off.sum()       # 15 tiles a frame and faces a few samples wide: a face meets one or two of them


def test_captured_render_replays_bit_exactly_on_new_vertices():
    all_verts, faces = _cylinder_meshes(6, seed=5)
    sets = [dev(all_verts[i:i + 2]) for i in (0, 2, 4)]
    static = sets[0].clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(2):
            render.render_meshes(static, faces, CAMERA, image_size=(40, 24))             # eager first: the faces go to the host and back once
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = render.render_meshes(static, faces, CAMERA, image_size=(40, 24))
    for s in (1, 2, 1):
        static.copy_(sets[s])
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = render.render_meshes(sets[s], faces, CAMERA, image_size=(40, 24))
        torch.cuda.synchronize()
        assert _same(got, want), s
    assert not torch.equal(render.render_meshes(sets[1], faces, CAMERA, image_size=(40, 24)).depth, render.render_meshes(sets[2], faces, CAMERA, image_size=(40, 24)).depth)


def test_timed_calls_sees_the_render_entry_points():
    verts, faces = _cylinder_meshes(1)
    with _lib.timed_calls() as t:
        render.render_meshes(dev(verts), faces, CAMERA, image_size=(20, 12))
    names = [r[0] for r in t.results()]
    assert names == ["g4d_render_project_f32", "g4d_render_raster"] and all(r[2] > 0 for r in t.results())


def test_render_output_on_the_models_own_output_dict():
    """render_one_batch's tuple (utils/nr_utils.py:77-81) from a forward of the wired model: shapes, dtypes and range, both meshes visible, and
    the picture equal to the twin's composition of the same meshes (same face ids, image within the derived bound)."""
    from garment4d_amd.body_models import SMPLLayer, Struct
    from test_model_gpu import _body_model, _model
    nbatch, T = 1, 2
    scene = syn.garment_scene(nbatch, T, 2048, seed=1)
    m = _model(scene)
    batch = {k: dev(v) for k, v in scene["batch"].items()}
    with torch.no_grad():
        out = m(dev(scene["x"]), _body_model(scene["body"]), batch)
    P = syn.smpl_like_params(V=scene["body"]["v_template"].shape[0], J=24, seed=2)
    P["v_template"] = scene["body"]["v_template"]
    body = SMPLLayer("", data_struct=Struct(**syn.smpl_data_struct(P, scene["body"]["faces"])), gender="female", num_betas=10).cuda()
    inputs = dict(pose_torch=torch.from_numpy(scene["batch"]["pose_torch"]), beta_torch=torch.zeros(nbatch, T, 10))
    images, bv, bf, cv, cf = render.render_output(out, inputs, body, add_cloth=True)
    V, Vg, nfb, nfg = scene["body"]["v_template"].shape[0], scene["template"][0].shape[0], len(scene["body"]["faces"]), len(out["garment_f_3"])
    assert images.shape == (nbatch, T, 256, 256, 3) and images.dtype == np.float32 and images.min() >= 0 and images.max() <= 255
    assert bv.shape == (nbatch, T, V, 3) and bf.shape == (nbatch, T, nfb, 3) and cv.shape == (nbatch, T, Vg, 3) and cf.shape == (nbatch, T, nfg, 3)
    assert np.array_equal(bf[0, 1], scene["body"]["faces"]) and np.array_equal(cf[0, 0], out["garment_f_3"])
    assert np.array_equal(cv.reshape(-1, Vg, 3), out["iter_regressed_lbs_garment_v"][-1].reshape(-1, Vg, 3).cpu().numpy())
    # the twin's composition: body ++ garment through the axis swap, the reference's camera, white faces
    swap = np.array(render._AXIS_SWAP, np.float32)
    faces = np.concatenate([scene["body"]["faces"].astype(np.int32), out["garment_f_3"].astype(np.int32) + V])
    camera = render.look_at_camera(1.5, 0.0, 45.0)
    cam = RT.camera(camera.eye, camera.at, camera.up, camera.half_angle, 256, 256, 2)
    light = RT.light_in_camera(cam, render.LIGHT_DIRECTION)
    for f in range(T):
        verts = (np.concatenate([bv[0, f], cv[0, f]]).astype(np.float64) @ swap.astype(np.float64)).astype(np.float32)     # entries 0 / +-1: exact
        px, py, invz, c = RT.project_f32(verts, cam, camera.near)
        t = RT.raster(px, py, invz, faces, 512, 512, 2, cam=c, light=light, ambient=0.5, directional=0.5)
        ids = t["face_id"]
        assert (ids >= nfb).any() and ((ids >= 0) & (ids < nfb)).any(), "both meshes must be visible"
        g, want64, bound = images[0, f].astype(np.float64), t["image64"] * 256, t["err_image"] * 256        # (the scaling by 256 is exact)
        assert ((np.abs(g - want64) <= bound) | ((g == 255) & (want64 >= 255 - bound))).all()               # 255 stands for everything from 255 up (:75)
        direct = render.render_meshes(dev(verts[None]), faces, camera)
        assert np.array_equal(direct.face_id[0].cpu().numpy(), ids) and np.array_equal(_bits(direct.depth[0].cpu().numpy()), _bits(t["depth"]))
    body_only = render.render_output(out, inputs, body)[0]
    assert body_only.shape == images.shape and not np.array_equal(body_only, images)

"""The projective ray-depth loss on the GPU (garment4d_amd/depth_fit.py, csrc/depth/depth_fit.hip) against the numpy twin
(tests/depth_fit_twin.py), fed with what the device's own projection and rasterizer gave: residual image, inlier set, per-frame sums, loss
and the vertex gradient are the twin's fp32 replay in every bit -- the forward's tree and the gradient's per-vertex order are part of
include/g4d_depth.h, so nothing is held to a tolerance.  Small shapes: F = 2, K = 2, a bent grid of 98 faces, sensors of 32 x 32 (2 x 2 tiles of
the rasterizer), 33 x 17 (ragged edges) and 41 x 25 = g4d_depth_chunk() + 1 samples; the edge cases each on the smallest scene that shows them.
Then the fits on top: fit_body_to_depth and fit_garment_to_depth are the plain Adam loops they say they are, and lower the loss."""
import functools

import numpy as np
import pytest
import torch

import depth_fit_twin as DT
from garment4d_amd import body_fit, depth_fit, fit, garment_fit, render, scan

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
CAMS = [render.Camera(*c) for c in DT.FRONT]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = np.int32 if got.dtype.itemsize == 4 else np.int64
    differ = got.reshape(-1).view(view) != want.reshape(-1).view(view)
    assert not differ.any(), (what, int(differ.sum()), got.reshape(-1)[differ][:4], want.reshape(-1)[differ][:4])


def run(verts, faces, depth_obs, cams=CAMS, weights=None, labels=None, face_labels=None, trunc=None, grazing=0.1, grad_out=1.0):
    """The three calls on the device, and the twin's fp32 replay on what the device's projection and rasterizer gave.  Returns (got, want, twin
    dict, views): got / want = dicts of resid, sums, count, total, grad."""
    v = dev(verts)
    K, F_, h, w = depth_obs.shape
    s = depth_fit.views(v, faces, cams, w, h)
    f_dev, _ = render._faces(faces, v.device)
    table = fit.vertex_corner_table(faces, v.shape[1], v.device)
    d, wt, lab, fl = dev(depth_obs), None if weights is None else dev(weights), None if labels is None else dev(labels), None if face_labels is None else dev(face_labels)
    tr = np.inf if trunc is None else float(F32(trunc))
    terms = depth_fit.depth_terms(s, f_dev, d, wt, lab, fl, tr, grazing, want_resid=True)
    grad = depth_fit.depth_vertex_gradient(s, f_dev, d, terms.total, dev(np.array([grad_out], F32)), table, wt, lab, fl, tr, grazing)
    got = dict(resid=host(terms.resid), sums=host(terms.sums), count=host(terms.count), total=host(terms.total), grad=host(grad))
    px, py, invz, cam, face_id = (host(x) for x in (s.px, s.py, s.invz, s.cam, s.face_id))
    consts = DT.camera_constants([tuple(c) for c in cams], w, h)
    same_bits(s.cams_host, DT.cams_host(consts), "camera constants")
    t = DT.forward(cam, faces, face_id, depth_obs, consts, weights, labels, face_labels, trunc, grazing, F32)
    g = DT.gradient(t, px, py, invz, faces, face_id, consts, verts.shape[1], grad_out, F32)
    want = dict(resid=t["resid"], sums=t["sums"], count=t["count"], total=np.array([t["W"], t["loss"]], F32), grad=g)
    return got, want, t, dict(px=px, py=py, invz=invz, cam=cam, face_id=face_id, consts=consts)


def check(got, want, what):
    for k in ("resid", "sums", "count", "total", "grad"):
        same_bits(got[k], want[k], (what, k))


@functools.lru_cache(maxsize=None)
def scene(w, h, K=2):
    """The bent grid (98 faces, F = 2) under the front cameras, a sensor of w x h rays observing a displaced copy (the twin's own projection and
    coverage: the reference is computed once, on the CPU), NaNs in a twentieth of the observed rays, weights in (0.5, 1.5) with a tenth 0, and
    labels: a face's label is its index mod 3, a ray's the label of the face the OBSERVED mesh shows there."""
    verts, faces = DT.bent_grid(8, 8, 2, 0)
    cams = DT.FRONT[:K]
    consts = DT.camera_constants(cams, w, h)
    rng = np.random.default_rng(1)
    target = (verts + 0.02 * rng.standard_normal(verts.shape)).astype(F32)
    tp = DT.project(target, consts)
    obs_id, depth_obs = DT.rasterize(tp[0], tp[1], tp[2], faces, w, h)
    depth_obs = np.where(rng.random(depth_obs.shape) < 0.05, F32(np.nan), depth_obs).astype(F32)
    weights = np.where(rng.random(depth_obs.shape) < 0.1, 0, 0.5 + rng.random(depth_obs.shape)).astype(F32)
    face_labels = (np.arange(len(faces)) % 3).astype(np.int32)
    labels = np.where(obs_id >= 0, face_labels[np.maximum(obs_id, 0)], -1).astype(np.int32)
    return dict(verts=verts, faces=faces, cams=[render.Camera(*c) for c in cams], depth_obs=depth_obs, weights=weights, labels=labels, face_labels=face_labels)


# ------------------------------------------------------------------------------------------------------------------------ bits of the twin
@pytest.mark.parametrize("size,K", [((32, 32), 2), ((33, 17), 2), ((41, 25), 1)])
def test_forward_and_gradient_equal_the_twins_replay_in_every_bit(size, K):
    """Weights, labels that veto some pairs, a trunc and a grazing bound that exclude some samples, NaN and +inf in depth_obs, two cameras seeing
    the same faces -- each asserted to occur.  41 x 25 with one camera is g4d_depth_chunk() + 1 samples per frame: two chunks, the second of one sample."""
    w, h = size
    sc = scene(w, h, K)
    assert K * w * h == depth_fit.chunk() + 1 or K == 2
    got, want, t, s = run(sc["verts"], sc["faces"], sc["depth_obs"], sc["cams"], sc["weights"], sc["labels"], sc["face_labels"], trunc=0.03, grazing=0.8)
    check(got, want, size)
    inl, obs, assoc = t["inlier"], t["observed"], t["associated"]
    hit = (s["face_id"] >= 0)
    assert inl.sum() > 60 and (got["count"] > 20).all() and got["total"][1] > 0 and np.abs(got["grad"]).max() > 0
    assert np.isnan(sc["depth_obs"]).any() and np.isinf(sc["depth_obs"]).any() and (obs & ~hit).any() and (hit & ~obs).any()
    assert (obs & hit & ~assoc).any()                                                      # labels veto
    live = assoc & (t["wt"] > 0)
    assert (live & ~t["facing"]).any() and (live & t["facing"] & ~inl).any()               # grazing excludes, trunc excludes
    assert ((t["wt"] == 0) & assoc).any() and np.array_equal(np.isnan(got["resid"]), ~inl)
    if K == 2:
        both = np.intersect1d(s["face_id"][0][inl[0]], s["face_id"][1][inl[1]])
        assert len(both) > 10                                                              # the sum over cameras has two terms
    # the public call: the same loss and, through autograd, the same gradient (scaled by the incoming gradient on the device)
    v = dev(sc["verts"]).requires_grad_(True)
    out = depth_fit.depth_mesh_distance(dev(sc["depth_obs"]), v, sc["faces"], sc["cams"], dev(sc["weights"]), 0.03, 0.8, dev(sc["labels"]), dev(sc["face_labels"]),
                                        image_size=size)
    (out.loss * 1.0).backward()
    same_bits(host(out.loss).reshape(1), want["total"][1:], "loss")
    same_bits(host(v.grad), want["grad"], "autograd")
    same_bits(host(out.inliers), want["count"], "inliers")
    same_bits(host(out.per_frame[:, :2]), want["sums"][:, :2], "per_frame")
    assert tuple(out.face_id.shape) == (K, 2, h, w) and tuple(out.rms.shape) == (2,) and (host(out.rms) > 0).all() and (host(out.rms) < 0.03).all()


def test_two_runs_give_the_same_bits():
    sc = scene(33, 17)
    a = run(sc["verts"], sc["faces"], sc["depth_obs"], sc["cams"], sc["weights"], trunc=0.03)[0]
    b = run(sc["verts"], sc["faces"], sc["depth_obs"], sc["cams"], sc["weights"], trunc=0.03)[0]
    check(a, b, "again")


def test_weights_none_and_all_zero():
    sc = scene(32, 32)
    got, want, t, _ = run(sc["verts"], sc["faces"], sc["depth_obs"], sc["cams"])
    check(got, want, "no weights")
    assert got["total"][0] == t["observed"].sum() and got["total"][1] > 0                  # every weight 1: W counts the observed rays
    got, want, t, _ = run(sc["verts"], sc["faces"], sc["depth_obs"], sc["cams"], np.zeros_like(sc["weights"]))
    check(got, want, "zero weights")
    assert (got["total"] == 0).all() and (got["grad"] == 0).all() and (got["count"] == 0).all() and np.isnan(got["resid"]).all()


def test_a_frame_no_ray_hits_counts_in_W_and_gets_zero_gradients():
    sc = scene(32, 32)
    verts = sc["verts"].copy()
    verts[1, :, 0] += 10                                                                   # frame 1 leaves every camera's image
    got, want, t, s = run(verts, sc["faces"], sc["depth_obs"], sc["cams"], sc["weights"])
    check(got, want, "empty frame")
    assert (s["face_id"][:, 1] == -1).all() and got["count"][1] == 0 and got["sums"][1, 0] == 0 and got["sums"][1, 2] > 0
    assert (got["grad"][1] == 0).all() and np.abs(got["grad"][0]).max() > 0
    alone = run(verts[:1], sc["faces"], sc["depth_obs"][:, :1], sc["cams"], sc["weights"][:, :1])[0]
    assert alone["total"][1] > got["total"][1] > 0                                         # the missed frame weighs in the denominator


def test_dropped_faces_a_vertex_without_faces_and_indices_at_the_edge():
    """A vertex behind camera 0's near plane (cam z = 0.05 < 0.1) drops its faces there -- their boxes are not walked --, and one more vertex
    that no face names gets a zero gradient."""
    sc = scene(32, 32)
    verts = np.concatenate([sc["verts"], np.zeros((2, 1, 3), F32)], 1)
    eye = np.asarray(sc["cams"][0].eye, F64)
    verts[:, 27] = (eye * (1 - 0.05 / np.linalg.norm(eye))).astype(F32)
    got, want, t, s = run(verts, sc["faces"], sc["depth_obs"], sc["cams"], sc["weights"], trunc=0.03)
    check(got, want, "dropped")
    assert ((s["invz"][0, :, 27] == 0).all() and (s["invz"][1, :, 27] > 0).all())
    boxes = DT.face_boxes(s["px"][0, 0], s["py"][0, 0], s["invz"][0, 0], sc["faces"], 32, 32)
    gone = [k for k, b in enumerate(boxes) if b is None]
    assert sorted(gone) == sorted(np.nonzero((sc["faces"] == 27).any(1))[0]) and not np.isin(s["face_id"][0], gone).any()
    assert (got["grad"][:, -1] == 0).all() and got["grad"].shape == (2, 65, 3) and np.isfinite(got["grad"]).all()


def test_one_triangle_covering_more_than_a_tile():
    """ONE face over 32 x 32 rays: a box of more than 16 x 16 samples walked by each of its three lanes, and both frames in one chunk."""
    verts = np.array([[[-0.6, -0.5, 0.1], [0.62, -0.45, -0.1], [0.03, 0.66, 0.05]], [[-0.5, -0.6, 0.0], [0.6, -0.5, 0.12], [-0.05, 0.6, -0.07]]], F32)
    faces = np.array([[0, 1, 2]], np.int32)
    consts = DT.camera_constants(DT.FRONT, 32, 32)
    tp = DT.project(verts + F32(0.01), consts)
    depth_obs = DT.rasterize(tp[0], tp[1], tp[2], faces, 32, 32)[1]
    got, want, t, s = run(verts, faces, depth_obs)
    check(got, want, "one triangle")
    j0, j1, i0, i1 = DT.face_boxes(s["px"][0, 0], s["py"][0, 0], s["invz"][0, 0], faces, 32, 32)[0]
    assert j1 - j0 >= 17 and i1 - i0 >= 17 and (got["count"] > 300).all() and (np.abs(got["grad"]) > 0).all()
    # the barycentric weights the gradient multiplies by sum to 1: the three corners' gradients add up to the whole-face translation gradient
    b = t["b"][t["inlier"]]
    assert np.abs(b.sum(-1) - 1).max() <= 4 * 2.0 ** -23 and b.min() > -0.02 and b.max() < 1.02


def test_a_frames_gradient_does_not_depend_on_its_batch():
    """Every ray observed and every weight 1 make W_0 = W_1 = K h w, so W of the batch is exactly 2 W_0: with grad_out = 2 the batch's
    gs = (2 * 2) / (2 W_0) has the bits of the single frame's 2 / W_0, and everything else of frame 0 is frame 0's alone."""
    sc = scene(33, 17)
    depth_obs = np.where(np.isfinite(sc["depth_obs"]), sc["depth_obs"], F32(1.5)).astype(F32)
    both = run(sc["verts"], sc["faces"], depth_obs, sc["cams"], trunc=0.03, grad_out=2.0)[0]
    for f in (0, 1):
        alone = run(sc["verts"][f:f + 1], sc["faces"], depth_obs[:, f:f + 1], sc["cams"], trunc=0.03, grad_out=1.0)[0]
        assert both["total"][0] == 2 * alone["total"][0] == 2 * 2 * 33 * 17
        same_bits(both["grad"][f:f + 1], alone["grad"], ("grad", f))
        same_bits(both["sums"][f:f + 1], alone["sums"], ("sums", f))
        same_bits(both["resid"][:, f:f + 1], alone["resid"], ("resid", f))
        assert np.abs(alone["grad"]).max() > 0


def test_a_hip_graph_capture_replays_to_the_eager_bits():
    sc = scene(32, 32)
    faces = sc["faces"]
    other = (sc["verts"] + 0.01 * np.random.default_rng(9).standard_normal(sc["verts"].shape)).astype(F32)
    g = dev(np.array([0.5], F32))
    d, wt = dev(sc["depth_obs"]), dev(sc["weights"])

    def calls(v, table, f_dev):
        s = depth_fit.views(v, faces, sc["cams"], 32, 32)
        terms = depth_fit.depth_terms(s, f_dev, d, wt, None, None, 0.03, 0.1, want_resid=True)
        return (s.face_id, *terms, depth_fit.depth_vertex_gradient(s, f_dev, d, terms.total, g, table, wt, None, None, 0.03, 0.1))

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        static = dev(sc["verts"])
        table, f_dev = fit.vertex_corner_table(faces, static.shape[1], static.device), render._faces(faces, static.device)[0]   # eager first: host tables
        calls(static, table, f_dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = calls(static, table, f_dev)
    for verts in (other, sc["verts"], other):
        static.copy_(dev(verts))
        graph.replay()
        torch.cuda.synchronize()
        got = [host(o) for o in outs]
        want = [host(o) for o in calls(dev(verts), table, f_dev)]
        for i, (a, b) in enumerate(zip(got, want)):
            same_bits(a, b, i)
    assert np.abs(got[-1]).max() > 0 and got[2].sum() > 100


def test_sensor_depth_then_depth_mesh_distance_on_the_same_mesh_is_at_rounding_level():
    """The sensor's depth is the rasterizer's 1 / iz: exact for the triangle whose vertices sit at the SNAPPED screen positions, each at most half a
    unit of 1/256 sample (plus the fp32 rounding of its screen coordinate, < 2^-8 unit at these sizes) from where the un-snapped vertex projects.
    Seen from the ray, that is this face's plane met by a ray displaced by at most delta = (0.5 + 2^-8) / (s hh) in d.x and in d.y, scaled by
    z_vertex / z_hit <= zmax / z; with z = (n . c0) / den the depth slope is |dz / dd.x| = z |n.x| / |den|, so
        |r| <= zmax (|n.x| + |n.y|) / |den| * delta  +  rounding,
    rounding = 32 * 2^-24 * z / |cosine|: the few roundings of n . c0 and den are relative to |n| |c0| and |n| |d|, and den = cosine |n| |d|.
    The second order of delta (1e-8) is far below.  The loss is then at most the weighted mean of the squared bounds."""
    sc = scene(32, 32)
    v = dev(sc["verts"])
    fl = dev(sc["face_labels"])
    sensor = depth_fit.sensor_depth(v, sc["faces"], sc["cams"], 32, fl)
    ids = host(sensor.face_id)
    assert tuple(sensor.depth.shape) == (2, 2, 32, 32) and sensor.labels.dtype == torch.int32
    assert np.array_equal(host(sensor.labels), np.where(ids >= 0, sc["face_labels"][np.maximum(ids, 0)], -1))
    assert np.array_equal(np.isinf(host(sensor.depth)), ids < 0) and depth_fit.sensor_depth(v, sc["faces"], sc["cams"], 32).labels is None
    got, want, t, s = run(sc["verts"], sc["faces"], host(sensor.depth), sc["cams"], labels=host(sensor.labels), face_labels=sc["face_labels"])
    check(got, want, "own depth")
    inl = t["inlier"]
    assert np.array_equal(inl, (ids >= 0) & t["facing"]) and inl.sum() > 400 and np.array_equal(ids, s["face_id"])
    t64 = DT.forward(s["cam"].astype(F64), sc["faces"], ids, host(sensor.depth), s["consts"], dt=F64, inlier=inl)
    corner_z = s["cam"][..., 2][np.arange(2)[:, None, None, None, None], np.arange(2)[None, :, None, None, None], sc["faces"][np.maximum(ids, 0)]]
    zmax = corner_z.max(-1).astype(F64)
    n, den, z = t64["n"], t64["den"], t64["z"]
    bound = np.zeros(ids.shape)
    with np.errstate(all="ignore"):                                                        # (samples without a face: not looked at)
        for c in range(2):
            delta = (0.5 + 2.0 ** -8) / (float(s["consts"][c]["s"]) * 128 * 32)
            bound[c] = zmax[c] * (np.abs(n[c, ..., 0]) + np.abs(n[c, ..., 1])) / np.abs(den[c]) * delta + 32 * 2.0 ** -24 * z[c] / t64["cosine"][c]
    r = np.abs(got["resid"][inl].astype(F64))
    print(f"own depth: largest |r| {r.max():.3e}, largest |r| / bound {np.max(r / bound[inl]):.3f}, loss {got['total'][1]:.3e}, "
          f"bound on the loss {np.sum(bound[inl] ** 2) / got['total'][0]:.3e}")
    assert (r <= bound[inl]).all() and got["total"][1] <= np.sum(bound[inl] ** 2) / got["total"][0]
    # ... and the bound says something: a thousandth of what the displaced mesh of the other tests (0.02 per coordinate) gives
    assert np.sum(bound[inl] ** 2) / got["total"][0] < 1e-3 * run(sc["verts"], sc["faces"], sc["depth_obs"], sc["cams"])[0]["total"][1]


# ----------------------------------------------------------------------------------------------------------------------------- the fits
def test_fit_body_to_depth_is_the_plain_adam_loop_and_lowers_the_loss():
    """The closed quad-cylinder body of tests/test_body_fit_gpu.py (B = 3), seen by four ring cameras at distance 3 through 64 x 64 rays: the
    sensor's depth at the generating parameters is the target; from the perturbed start of that file's loop test, fit_body_to_depth is the
    hand-written Adam loop bit for bit over 5 steps, and after 30 steps the loss is below the loss before."""
    from test_body_fit_gpu import _body, _dev, _setup
    _, _, betas, pose, transl = _setup()
    body = _body()
    cams = scan.ring_cameras(4, distance=3.0, start=0.0)
    with torch.no_grad():
        target = body(betas=_dev(betas), global_orient=_dev(pose)[:, :3], body_pose=_dev(pose)[:, 3:], transl=_dev(transl)).vertices
    depth_obs = depth_fit.sensor_depth(target, body.faces, cams, 64).depth
    assert tuple(depth_obs.shape) == (4, 3, 64, 64) and int(torch.isfinite(depth_obs).sum()) > 1000
    rng = np.random.default_rng(55)
    b0, p0, t0 = _dev(betas + 0.2 * rng.standard_normal(betas.shape)), _dev(pose + 0.03 * rng.standard_normal(pose.shape)), _dev(transl + 0.01)
    kw = dict(trunc=0.05, grazing=0.1, pose_prior=1e-3, shape_prior=1e-3)
    fb, fp, ft, losses = body_fit.fit_body_to_depth(body, depth_obs, cams, None, b0, p0, t0, steps=5, lr=0.01, **kw)
    b, p, t = (x.detach().clone().requires_grad_(True) for x in (b0, p0, t0))
    opt = torch.optim.Adam([b, p, t], lr=0.01)
    mine = []
    for _ in range(5):
        opt.zero_grad()
        out = body_fit.depth_body_fit_loss(body, b, p, t, depth_obs, cams, None, **kw)
        out["total"].backward()
        mine.append(out["total"].detach())
        opt.step()
    with torch.no_grad():
        mine.append(body_fit.depth_body_fit_loss(body, b, p, t, depth_obs, cams, None, **kw)["total"])
    assert losses.shape == (6,) and losses.is_cuda and torch.equal(losses, torch.stack(mine))
    assert torch.equal(fb, b.detach()) and torch.equal(fp, p.detach()) and torch.equal(ft, t.detach()) and not torch.equal(fb, b0) and not fb.requires_grad
    assert sorted(out) == ["data", "inliers", "pose", "rms", "shape", "total"] and torch.equal(out["total"], out["data"] + out["pose"] + out["shape"])
    assert tuple(out["rms"].shape) == (3,) and out["inliers"].dtype == torch.int32 and (out["inliers"] > 100).all()
    _, _, _, long = body_fit.fit_body_to_depth(body, depth_obs, cams, None, b0, p0, t0, steps=30, lr=0.01, **kw)
    print(f"body to depth, 30 Adam steps at lr 0.01: {float(long[0]):.6e} -> {float(long[-1]):.6e}")
    assert torch.equal(long[:5], losses[:5]) and float(long[-1]) < float(long[0])


def test_fit_garment_to_depth_is_the_plain_adam_loop_and_lowers_the_loss():
    """The 64-vertex garment over the 700-vertex body of tests/test_garment_fit_gpu.py (2 clips of 3 frames), seen by two ring cameras through
    64 x 64 rays with scan.scan_batch's labelling (body 0, garment 6): the sensor's depth and labels at the generating coefficients are the
    target.  The body occludes the garment and takes its own rays; a garment ray pairs only with a garment face."""
    from test_garment_fit_gpu import NB, T, _dev, _posed_plus_root, _setup
    sc, model, batch, body_model, faces, coeff = _setup()
    cams = scan.ring_cameras(2)
    Vb = batch["smpl_vertices_torch"].shape[2]
    joined = render._joined_faces(body_model.faces, faces, Vb)
    face_labels = torch.cat([torch.zeros(len(body_model.faces), dtype=torch.int32), torch.full((len(faces),), 6, dtype=torch.int32)]).cuda()
    verts = torch.cat([batch["smpl_vertices_torch"].reshape(NB * T, Vb, 3), _posed_plus_root(model, body_model, batch, _dev(coeff))], 1)
    sensor = depth_fit.sensor_depth(verts, joined, cams, 64, face_labels)
    n_body, n_garment = int((sensor.labels == 0).sum()), int((sensor.labels == 6).sum())
    assert n_body > 500 and n_garment > 500
    c0 = _dev(coeff + 0.5 * np.random.default_rng(64).standard_normal(coeff.shape))
    wt = (sensor.labels == 6).float()
    kw = dict(weights=wt, trunc=0.05, grazing=0.1, coeff_prior=1e-3)
    fitted, losses = garment_fit.fit_garment_to_depth(model, body_model, batch, c0, sensor.depth, sensor.labels, cams, faces, 6, steps=5, lr=0.05, **kw)
    c = c0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([c], lr=0.05)
    mine = []
    for _ in range(5):
        opt.zero_grad()
        out = garment_fit.depth_garment_fit_loss(model, body_model, batch, c, sensor.depth, sensor.labels, cams, faces, 6, **kw)
        out["total"].backward()
        mine.append(out["total"].detach())
        opt.step()
    with torch.no_grad():
        mine.append(garment_fit.depth_garment_fit_loss(model, body_model, batch, c, sensor.depth, sensor.labels, cams, faces, 6, **kw)["total"])
    assert losses.shape == (6,) and losses.is_cuda and torch.equal(losses, torch.stack(mine))
    assert torch.equal(fitted, c.detach()) and not torch.equal(fitted, c0) and not fitted.requires_grad
    assert sorted(out) == ["data", "inliers", "posed", "prior", "rms", "total"] and torch.isfinite(c.grad).all() and float(c.grad.abs().max()) > 0
    assert tuple(out["rms"].shape) == (NB * T,) and (out["inliers"] > 50).all() and (out["inliers"] <= n_garment).all()
    # without the weights the body's rays count too (in W and in the inliers) and still move nothing but the garment
    c.grad = None
    full = garment_fit.depth_garment_fit_loss(model, body_model, batch, c, sensor.depth, sensor.labels, cams, faces, 6)
    full["total"].backward()
    assert int(full["inliers"].sum()) > int(out["inliers"].sum()) + n_body // 2 and float(c.grad.abs().max()) > 0
    _, long = garment_fit.fit_garment_to_depth(model, body_model, batch, c0, sensor.depth, sensor.labels, cams, faces, 6, steps=30, lr=0.05, **kw)
    print(f"garment to depth, 30 Adam steps at lr 0.05: {float(long[0]):.6e} -> {float(long[-1]):.6e}")
    assert torch.equal(long[:5], losses[:5]) and float(long[-1]) < float(long[0])

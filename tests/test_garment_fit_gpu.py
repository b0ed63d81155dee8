"""Fitting the garment to a scan (garment4d_amd/garment_fit.py) on synthetic.garment_scene with the 64-vertex garment (garment_rc = (8, 8)), 2 clips
of 3 frames, K = 16: (i) points on the posed garment's own surface give a loss and a gradient at rounding level, and the coefficients' gradient
is the vertices' gradient carried through PCA_inverse_transform, (ii) fit_garment_to_scan is the plain Adam loop it says it is, bit for bit,
(iii) 30 Adam steps on the vertex-correspondence L2 loss from perturbed coefficients end where the float64 restatement of the same loop ends."""
import functools
import types

import numpy as np
import pytest
import torch

import garment_skin_grad_twin as GT
from garment4d_amd import garment_fit, synthetic as syn, tuning
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSeg

pytestmark = pytest.mark.gpu
NB, T, K = 2, 3, 16


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def _setup():
    sc = syn.garment_scene(NB, T, 4, garment_rc=(8, 8), seed=61)
    model = PCALBSGarmentUseSegEncoderSeg(garment_name="Tshirt", pca_dim=64, pca=sc["pca"], template=sc["template"], lbs_k=K, iteration=1).cuda().eval()
    batch = {k: _dev(v) for k, v in sc["batch"].items()}
    rng = np.random.default_rng(62)
    batch["smpl_root_joints_torch"] = _dev(rng.standard_normal((NB, T, 3)) * 0.05)
    body_model = types.SimpleNamespace(parents=torch.from_numpy(sc["body"]["parents"]).cuda(), faces=sc["body"]["faces"])
    gq = sc["template"][1]
    faces = np.concatenate([gq[:, [0, 1, 2]], gq[:, [0, 2, 3]]], 0).astype(np.int64)
    coeff = (rng.standard_normal((NB, 64)) * 0.5).astype(np.float32)
    return sc, model, batch, body_model, faces, coeff


def _surface_points(posed_plus_root, faces, per_face=2, seed=63):
    """Points on the surface of the posed garment: barycentric combinations of its triangles, in fp32 on the device.  (F,Vg,3) -> (F,P,3)."""
    f = torch.from_numpy(faces).cuda()
    w = np.random.default_rng(seed).dirichlet(np.ones(3), (posed_plus_root.shape[0], len(faces) * per_face)).astype(np.float32)
    tri = posed_plus_root[:, f.repeat(per_face, 1)]
    return (tri * _dev(w)[..., None]).sum(2).contiguous()


def _posed_plus_root(model, body_model, batch, coeff):
    with torch.no_grad():
        tpose = model.PCA_garment_encoder.PCA_inverse_transform(coeff)
        posed = model.skin_garment(tpose, body_model, batch)[0]
    return posed.reshape(NB * T, -1, 3) + batch["smpl_root_joints_torch"].reshape(NB * T, 1, 3)


def test_on_its_own_surface_the_loss_and_the_gradient_are_at_rounding_level_and_reach_the_coefficients():
    """Points taken on the posed surface (fp32 combinations of its triangles: off it by a few ulp of coordinates of size <= 2, i.e. <= 1e-6) give
    data <= (1e-6)^2 = 1e-12 and, as in tests/test_body_fit_gpu.py, gradient entries of the size of the residual times d verts / d parameter:
    <= 1e-5.  One truncation distance away neither is small, and the coefficients' gradient is the T-pose vertices' gradient times the PCA basis."""
    sc, model, batch, body_model, faces, coeff = _setup()
    c = _dev(coeff).requires_grad_(True)
    pts = _surface_points(_posed_plus_root(model, body_model, batch, c.detach()), faces)
    out = garment_fit.garment_fit_loss(model, body_model, batch, c, pts, None, faces, trunc=0.05)
    assert out["posed"].grad_fn is not None and tuple(out["posed"].shape) == (NB, T, 64, 3)
    out["total"].backward()
    data, worst = float(out["data"].detach()), float(c.grad.abs().max())
    print(f"on the surface: data {data:.3e}, largest coefficient gradient {worst:.3e}, inliers {out['inliers'].tolist()} of {pts.shape[1]}")
    assert data <= 1e-12 and worst <= 1e-5 and torch.equal(out["total"], out["data"]) and (out["inliers"] == pts.shape[1]).all()
    assert tuning.current().garment_lbs_autograd is False and tuning.current().stage1_autograd is False      # the caller's setting is left alone
    # displaced points: a loss, a gradient, and the chain rule through PCA_inverse_transform
    c.grad = None
    far = garment_fit.garment_fit_loss(model, body_model, batch, c, pts + 0.01, None, faces, trunc=0.05, coeff_prior=0.5)
    far["total"].backward()
    assert float(far["data"].detach()) > 1e-6 and torch.allclose(far["prior"], 0.5 * (c ** 2).mean()) and torch.equal(far["total"], far["data"] + far["prior"])
    enc = model.PCA_garment_encoder
    with torch.no_grad():
        v = enc.PCA_inverse_transform(c.detach())
    v = v.clone().requires_grad_(True)
    as_verts = garment_fit.garment_fit_loss(model, body_model, batch, v, pts + 0.01, None, faces, trunc=0.05)
    as_verts["total"].backward()
    assert torch.equal(as_verts["data"], far["data"]) and float(as_verts["prior"]) == 0
    scale = enc.PCA_scale.float().reshape(-1).expand(enc.PCA_comp.shape[1])
    chain = (v.grad.reshape(NB, -1) * scale) @ enc.PCA_comp.float().t() + 0.5 * 2 * c.detach() / c.numel()
    assert torch.isfinite(c.grad).all() and float(c.grad.abs().max()) > 1e-6
    torch.testing.assert_close(c.grad, chain, rtol=1e-4, atol=1e-7 * float(chain.abs().max()) + 1e-12)


def test_fit_garment_to_scan_is_the_plain_adam_loop_bit_for_bit():
    sc, model, batch, body_model, faces, coeff = _setup()
    pts = _surface_points(_posed_plus_root(model, body_model, batch, _dev(coeff)), faces)
    w = (torch.rand(pts.shape[:2], generator=torch.Generator().manual_seed(5)) < 0.8).float().cuda()
    c0 = _dev(coeff + 0.5 * np.random.default_rng(64).standard_normal(coeff.shape))
    kw = dict(trunc=0.05, coeff_prior=1e-3)
    fitted, losses = garment_fit.fit_garment_to_scan(model, body_model, batch, c0, pts, w, faces, steps=5, lr=0.05, **kw)
    c = c0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([c], lr=0.05)
    mine = []
    for _ in range(5):
        opt.zero_grad()
        total = garment_fit.garment_fit_loss(model, body_model, batch, c, pts, w, faces, **kw)["total"]
        total.backward()
        mine.append(total.detach())
        opt.step()
    with torch.no_grad():
        mine.append(garment_fit.garment_fit_loss(model, body_model, batch, c, pts, w, faces, **kw)["total"])
    assert losses.shape == (6,) and losses.is_cuda and torch.equal(losses, torch.stack(mine))
    assert torch.equal(fitted, c.detach()) and not torch.equal(fitted, c0) and not fitted.requires_grad and float(losses[-1]) < float(losses[0])
    # the loader's form gives the same numbers
    lab = torch.where(w > 0, 6, 0).reshape(NB, T, -1, 1)
    inputs = dict(batch, pcd_torch=pts.reshape(NB, T, -1, 3), pcd_label_torch=lab)
    with torch.no_grad():
        a = garment_fit.scan_garment_fit_loss(model, body_model, inputs, fitted, faces, 6, **kw)
        b = garment_fit.garment_fit_loss(model, body_model, batch, fitted, pts, w, faces, **kw)
    assert torch.equal(a["total"], b["total"]) and tuple(a["rms"].shape) == (NB, T) and torch.equal(a["inliers"].reshape(-1), b["inliers"])


# ------------------------------------------------------------------------------------------------------------------------- (iii)
STEPS, LR = 30, 0.05


def test_thirty_adam_steps_on_the_correspondence_loss_end_where_the_float64_loop_ends():
    """Target: the garment posed at the generating coefficients; start: coefficients + 1.0 N(0,1).  The float64 loop restates every step on the CPU
    (decode, neighbour search by a stable sort of the float64 distances, the twin's torch restatement, torch's mean of squares and Adam) with the
    fp32 joint transforms of the HIP run as constants.  The HIP loop -- PCA_inverse_transform and skin_garment under the two flags -- must end at
    <= 2 x the float64 loop's final loss (Adam's normalisation amplifies rounding differences: the body fit's gate) and below its own first."""
    sc, model, batch, body_model, faces, coeff = _setup()
    enc = model.PCA_garment_encoder
    start = coeff + np.random.default_rng(65).standard_normal(coeff.shape).astype(np.float32)
    # ---- HIP, fp32
    with torch.no_grad():
        target = model.skin_garment(enc.PCA_inverse_transform(_dev(coeff)), body_model, batch)[0]
    c = _dev(start).requires_grad_(True)
    opt = torch.optim.Adam([c], lr=LR)
    losses = []
    with tuning.use(tuning.current().replace(garment_lbs_autograd=True, stage1_autograd=True)):
        for _ in range(STEPS + 1):
            opt.zero_grad()
            posed = model.skin_garment(enc.PCA_inverse_transform(c), body_model, batch)[0]
            loss = ((posed - target) ** 2).mean()
            losses.append(loss.detach())
            loss.backward()
            opt.step()
    first, last = float(losses[0]), float(losses[-1])
    # ---- float64, CPU: the node's constants from a forward of its own
    with tuning.use(tuning.current().replace(garment_lbs_autograd=True)):
        alive = model.skin_garment(enc.PCA_inverse_transform(_dev(start)).requires_grad_(True), body_model, batch)   # (the outputs keep the node's tensors)
    g, body, idx_k, d_k, cW, inv_nn_W, inv_A, u, Wt, nn_W, A = alive[0].grad_fn.saved_tensors
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    consts = dict(root=f64(batch["Tpose_smpl_root_joints_torch"]).reshape(NB, 3), body=f64(body), cW=f64(cW), Wt=f64(Wt), inv_A=f64(inv_A), A=f64(A),
                  M=GT.step_operator(model.adj_old), iters=100)
    comp, mean = torch.from_numpy(f64(enc.PCA_comp)), torch.from_numpy(f64(enc.PCA_mean))
    scale = torch.from_numpy(f64(enc.PCA_scale)).reshape(-1).expand(comp.shape[1])

    def posed64(cc):
        x = ((cc @ comp + mean) * scale).reshape(NB, -1, 3)
        gg = x.detach().numpy() + consts["root"][:, None]
        d2 = ((gg[:, :, None] - consts["body"][:, None]) ** 2).sum(-1)
        idx = np.argsort(d2, axis=-1, kind="stable")[..., :K].astype(np.int32)
        return GT.torch_forward(x, dict(consts, idx=idx), torch.float64)[0]
    with torch.no_grad():
        target64 = posed64(torch.from_numpy(coeff.astype(np.float64)))
    c64 = torch.from_numpy(start.astype(np.float64)).requires_grad_(True)
    opt64 = torch.optim.Adam([c64], lr=LR)
    l64 = []
    for _ in range(STEPS + 1):
        opt64.zero_grad()
        loss = ((posed64(c64) - target64) ** 2).mean()
        l64.append(float(loss.detach()))
        loss.backward()
        opt64.step()
    first64, last64 = l64[0], l64[-1]
    print(f"correspondence fit, {STEPS} Adam steps at lr {LR}: float64 CPU {first64:.6e} -> {last64:.6e}; HIP fp32 {first:.6e} -> {last:.6e}; final ratio {last / last64:.4f}")
    assert last64 < first64, (first64, last64)
    assert last <= 2 * last64 and last < first

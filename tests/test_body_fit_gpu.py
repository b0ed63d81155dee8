"""Registering the body to a scan (garment4d_amd/body_fit.py) on a closed quad-cylinder body (synthetic.quad_cylinder as v_template, 12 x 12 = 144
vertices, smpl_like_params' other constants at that size), B = 3 frames: (i) at the generating parameters the loss and every gradient are at
rounding level, (ii) fit_body_to_scan is the plain Adam loop it says it is, bit for bit, (iii) 30 Adam steps on the vertex-correspondence L2
loss end where the float64 restatement of the same loop ends."""
import functools

import numpy as np
import pytest
import torch

import smpl_grad_twin as ST
from garment4d_amd import body_fit, synthetic as syn, tuning
from garment4d_amd.body_models import SMPL, Struct

pytestmark = pytest.mark.gpu
B, ROWS, COLS = 3, 12, 12


@functools.lru_cache(maxsize=None)
def _setup():
    verts, quads = syn.quad_cylinder(ROWS, COLS)
    faces = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 0).astype(np.int64)
    P = syn.smpl_like_params(V=len(verts), seed=51)
    P["v_template"] = verts
    betas, pose = syn.smpl_like_pose(B, seed=52)
    transl = (np.random.default_rng(53).standard_normal((B, 3)) * 0.1).astype(np.float32)
    return P, faces, betas, pose, transl


def _body():
    P, faces, *_ = _setup()
    return SMPL("", data_struct=Struct(**syn.smpl_data_struct(P, faces)), gender="female", num_betas=10, create_betas=False, create_global_orient=False,
                create_body_pose=False, create_transl=False).cuda()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _surface_points(body, betas, pose, transl, per_face=2, seed=54):
    """Points on the surface of the body at (betas, pose, transl): barycentric combinations of its posed triangles, in fp32 on the device."""
    with torch.no_grad():
        v = body(betas=betas, global_orient=pose[:, :3], body_pose=pose[:, 3:], transl=transl).vertices
    faces = torch.from_numpy(np.asarray(body.faces)).cuda()
    w = np.random.default_rng(seed).dirichlet(np.ones(3), (B, len(faces) * per_face)).astype(np.float32)
    tri = v[:, faces.repeat(per_face, 1)]                                   # (B, P, 3 corners, 3)
    return (tri * _dev(w)[..., None]).sum(2).contiguous()


def test_at_the_generating_parameters_the_loss_and_every_gradient_are_at_rounding_level():
    """Points taken on the posed surface (fp32 combinations of its triangles: off the surface by a few ulp of coordinates of size <= 2, i.e.
    <= 1e-6) give data <= (1e-6)^2 = 1e-12.  d data / d verts is 2 w bary resid / W per point, so the gradient of the mean is of the size of
    the residual times d verts / d parameter (a few units): every entry <= 1e-5 -- against entries of order 0.1 one truncation distance away."""
    _, _, betas, pose, transl = _setup()
    body = _body()
    b, p, t = (_dev(x).requires_grad_(True) for x in (betas, pose, transl))
    pts = _surface_points(body, b.detach(), p.detach(), t.detach())
    out = body_fit.body_fit_loss(body, b, p, t, pts, None, trunc=0.05)
    out["total"].backward()
    worst = max(float(x.grad.abs().max()) for x in (b, p, t))
    data = float(out["data"].detach())
    print(f"on the surface: data {data:.3e}, largest gradient entry {worst:.3e}, inliers {out['inliers'].tolist()} of {pts.shape[1]}")
    assert data <= 1e-12 and torch.equal(out["total"], out["data"]) and worst <= 1e-5
    assert (out["inliers"] == pts.shape[1]).all()
    # ... and it is a loss: the same points against a displaced body are not at rounding level, and the priors add what they say
    far = body_fit.body_fit_loss(body, b, p, t + 0.02, pts, None, trunc=0.05, pose_prior=0.5, shape_prior=0.25)
    assert float(far["data"].detach()) > 1e-6
    assert torch.allclose(far["pose"], 0.5 * (p[:, 3:] ** 2).mean()) and torch.allclose(far["shape"], 0.25 * (b ** 2).mean())
    assert torch.equal(far["total"], far["data"] + far["pose"] + far["shape"])


def test_fit_body_to_scan_is_the_plain_adam_loop_bit_for_bit():
    _, _, betas, pose, transl = _setup()
    body = _body()
    pts = _surface_points(body, _dev(betas), _dev(pose), _dev(transl))
    w = (torch.rand(pts.shape[:2], generator=torch.Generator().manual_seed(5)) < 0.8).float().cuda()
    rng = np.random.default_rng(55)
    b0, p0, t0 = _dev(betas + 0.2 * rng.standard_normal(betas.shape)), _dev(pose + 0.03 * rng.standard_normal(pose.shape)), _dev(transl + 0.01)
    kw = dict(trunc=0.05, pose_prior=1e-3, shape_prior=1e-3)
    fb, fp, ft, losses = body_fit.fit_body_to_scan(body, pts, w, b0, p0, t0, steps=5, lr=0.01, **kw)
    b, p, t = (x.detach().clone().requires_grad_(True) for x in (b0, p0, t0))
    opt = torch.optim.Adam([b, p, t], lr=0.01)
    mine = []
    for _ in range(5):
        opt.zero_grad()
        total = body_fit.body_fit_loss(body, b, p, t, pts, w, **kw)["total"]
        total.backward()
        mine.append(total.detach())
        opt.step()
    with torch.no_grad():
        mine.append(body_fit.body_fit_loss(body, b, p, t, pts, w, **kw)["total"])
    assert losses.shape == (6,) and losses.is_cuda and torch.equal(losses, torch.stack(mine))
    assert torch.equal(fb, b.detach()) and torch.equal(fp, p.detach()) and torch.equal(ft, t.detach())
    assert not torch.equal(fb, b0) and not fb.requires_grad and float(losses[-1]) < float(losses[0])
    assert tuning.current().lbs_autograd is False                            # the caller's setting is left alone


# ------------------------------------------------------------------------------------------------------------------------- (iii)
STEPS, LR = 30, 0.02


def _perturbed():
    _, _, betas, pose, transl = _setup()
    rng = np.random.default_rng(56)
    return betas + 0.5 * rng.standard_normal(betas.shape).astype(np.float32), pose + 0.1 * rng.standard_normal(pose.shape).astype(np.float32), transl


def float64_loop():
    """The 30 Adam steps on mean ||verts - target||^2 with the reference-form float64 restatement on the CPU: (initial, final) loss."""
    P, _, betas, pose, transl = _setup()
    tp = ST.torch_params(P, torch.float64)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    with torch.no_grad():
        target = ST.torch_lbs(t64(betas), t64(pose), tp)[0] + t64(transl)[:, None]
    b, p, t = (t64(x).requires_grad_(True) for x in _perturbed())
    opt = torch.optim.Adam([b, p, t], lr=LR)
    losses = []
    for _ in range(STEPS + 1):
        opt.zero_grad()
        loss = ((ST.torch_lbs(b, p, tp)[0] + t[:, None] - target) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return losses[0], losses[-1], target


def test_thirty_adam_steps_on_the_correspondence_loss_end_where_the_float64_loop_ends():
    """Perturbation (betas + 0.5 N(0,1), pose + 0.1 N(0,1)) chosen on the CPU so that the float64 loop lowers the loss at least tenfold (asserted).
    The HIP loop -- SMPL.forward under the flag, torch's mean of squares, lbs()'s adjoint on HIP -- must end at <= 2 x the float64 loop's final
    loss (Adam's normalisation amplifies rounding differences) and below its own initial loss."""
    first64, last64, target = float64_loop()
    assert last64 * 10 <= first64, (first64, last64)
    body = _body()
    tgt = target.float().cuda()
    b, p, t = (_dev(x).requires_grad_(True) for x in _perturbed())
    opt = torch.optim.Adam([b, p, t], lr=LR)
    losses = []
    with tuning.use(tuning.current().replace(lbs_autograd=True)):
        for _ in range(STEPS + 1):
            opt.zero_grad()
            loss = ((body(betas=b, global_orient=p[:, :3], body_pose=p[:, 3:], transl=t).vertices - tgt) ** 2).mean()
            losses.append(loss.detach())
            loss.backward()
            opt.step()
    first, last = float(losses[0]), float(losses[-1])
    print(f"correspondence fit, {STEPS} Adam steps at lr {LR}: float64 CPU {first64:.6e} -> {last64:.6e}; HIP fp32 {first:.6e} -> {last:.6e}; final ratio {last / last64:.4f}")
    assert last <= 2 * last64 and last < first

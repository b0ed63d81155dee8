"""The adjoint of lbs() on HIP (csrc/smpl/smpl_grad.hip, include/g4d_smpl.h) behind tuning.Tuning.lbs_autograd: against the reference's own
autograd (tests/golden/smpl_grad.npz, 3 x the reference's fp32 error), against the float64 numpy twin (tests/smpl_grad_twin.py) over the
launch edges of the kernels (3 x the error fp32 torch autograd makes on the same inputs), its exact properties (same bits on every run, a
frame's bits independent of the batch, zero in -> zero out, a NaN frame stays alone, hipGraph replay), and the body models' graph."""
import functools

import numpy as np
import pytest
import torch

import smpl_grad_twin as ST
from conftest import load_golden
from garment4d_amd import _lib, lbs as L, synthetic as syn, tuning
from garment4d_amd.body_models import SMPL, SMPLLayer, Struct

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _consts(P):
    return (_dev(P["v_template"]), _dev(P["shapedirs"]), _dev(P["posedirs"]), _dev(P["J_regressor"]), torch.from_numpy(np.asarray(P["parents"])), _dev(P["lbs_weights"]))


def _on():
    return tuning.use(tuning.current().replace(lbs_autograd=True))


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_gradients_match_the_references_autograd_within_three_times_its_own_fp32_error(name):
    """lbs() under the flag, then backward of sum(verts g_v) + sum(joints g_p), on the golden cases (a: axis-angle, b: rotation matrices,
    c: all-zero joints and an all-zero frame): max |d - reference fp32| <= 3 eref per tensor; the forward outputs have the flag-off call's bits."""
    g = load_golden("smpl_grad.npz")
    P = {k[2:]: v for k, v in g.items() if k.startswith("P_")}
    consts, p2r = _consts(P), bool(g[f"{name}_pose2rot"])
    betas, pose = _dev(g[f"{name}_betas"]).requires_grad_(True), _dev(g[f"{name}_pose"]).requires_grad_(True)
    v0, j0 = L.lbs(betas, pose, *consts, pose2rot=p2r)
    assert v0.grad_fn is None and j0.grad_fn is None
    with _on():
        verts, joints = L.lbs(betas, pose, *consts, pose2rot=p2r)
    assert verts.grad_fn is not None and joints.grad_fn is not None
    assert np.array_equal(_bits(verts), _bits(v0)) and np.array_equal(_bits(joints), _bits(j0))
    ((verts * _dev(g[f"{name}_g_v"])).sum() + (joints * _dev(g[f"{name}_g_p"])).sum()).backward()
    failures = []
    for k, got in (("d_pose", pose.grad), ("d_betas", betas.grad)):
        want, eref = g[f"{name}_{k}"], float(g[f"{name}_eref_{k}"])
        assert tuple(got.shape) == want.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()
        print(f"golden {name} {k}: max |err| {err:.3e}  eref {eref:.3e}  err / (3 eref) {err / (3 * eref):.3f}")
        if not err <= 3 * eref:
            failures.append((k, err, eref))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------------- twin sweep
_SLAB = 128   # G4D_SMPL_SLAB_VERTS: checked against g4d_smpl_grad_slabs below
#         V     B   J   NB  pose2rot broadcast which
SWEEP = [(1,    1,  24, 10, True,  False, "both"),
         (31,   15, 24, 10, True,  False, "v"),
         (33,   17, 24, 10, False, False, "both"),
         (97,   33, 24, 10, True,  True,  "both"),
         (500,  17, 5,  1,  False, False, "both"),
         (500,  15, 5,  10, True,  True,  "j"),
         (_SLAB, 17, 24, 1, True,  False, "both"),
         (_SLAB + 1, 33, 24, 10, False, True, "v"),
         (97,   1,  5,  1,  True,  False, "j"),
         (31,   33, 5,  10, False, False, "v"),
         (33,   65, 5,  1,  True,  False, "both"),      # five 16-frame tiles: a second workgroup along the frames (four tiles each)
         (6890, 2,  24, 10, True,  False, "both")]


@functools.lru_cache(maxsize=None)
def _sweep_case(V, B, J, NB, pose2rot, broadcast, which):
    P = syn.smpl_like_params(V=V, J=J, num_betas=NB, seed=V + B)
    betas, pose = syn.smpl_like_pose(B, J=J, num_betas=NB, seed=V + B + 1)
    rng = np.random.default_rng(V + B + 2)
    if not pose2rot:
        pose = (ST.rodrigues(pose.reshape(-1, 3))[0].reshape(B, J, 3, 3) + 0.01 * rng.standard_normal((B, J, 3, 3))).astype(np.float32)
    if broadcast:
        betas = betas[:1]
    gv = rng.standard_normal((B, V, 3)).astype(np.float32) if which in ("v", "both") else None
    gj = rng.standard_normal((B, J, 3)).astype(np.float32) if which in ("j", "both") else None
    return P, betas, pose, gv, gj


@pytest.mark.parametrize("V,B,J,NB,pose2rot,broadcast,which", SWEEP)
def test_gradients_match_the_float64_twin_within_three_times_fp32_autograds_own_error(V, B, J, NB, pose2rot, broadcast, which):
    """lbs_backward against the float64 twin; the bound per tensor is 3 x max |fp32 torch autograd of the twin's restatement - float64 twin| on
    the same inputs, both measured here."""
    slabs = _lib.smpl_lib()[0].g4d_smpl_grad_slabs
    assert slabs(B, _SLAB) == 1 and slabs(B, _SLAB + 1) == 2
    P, betas, pose, gv, gj = _sweep_case(V, B, J, NB, pose2rot, broadcast, which)
    want = ST.adjoint(betas, pose, P, gv, gj, pose2rot)
    t32 = ST.torch_grads(betas, pose, P, gv, gj, pose2rot, torch.float32)
    got = L.lbs_backward(_dev(betas), _dev(pose), *_consts(P), None if gv is None else _dev(gv), None if gj is None else _dev(gj), pose2rot=pose2rot)
    failures = []
    for k, g_, w_, t_ in zip(("d_betas", "d_pose"), got, want, t32):
        assert tuple(g_.shape) == w_.shape
        err, eref = np.abs(g_.cpu().numpy().astype(np.float64) - w_).max(), np.abs(t_ - w_).max()
        print(f"sweep {(V, B, J, NB, pose2rot, broadcast, which)} {k}: max |err| {err:.3e}  torch fp32 {eref:.3e}  err / (3 torch) {err / (3 * eref) if eref else float('inf'):.3f}"
              f"  (max |grad| {np.abs(w_).max():.3e})")
        if not err <= 3 * eref:
            failures.append((k, err, eref))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------------- exact properties
@functools.lru_cache(maxsize=None)
def _exact_case():
    V, B = 161, 17
    P = syn.smpl_like_params(V=V, seed=31)
    betas, pose = syn.smpl_like_pose(B, seed=32)
    rng = np.random.default_rng(33)
    return P, betas, pose, rng.standard_normal((B, V, 3)).astype(np.float32), rng.standard_normal((B, 24, 3)).astype(np.float32)


def test_two_runs_give_equal_bits_and_a_frames_bits_do_not_depend_on_its_batch():
    P, betas, pose, gv, gj = _exact_case()
    consts = _consts(P)
    a = L.lbs_backward(_dev(betas), _dev(pose), *consts, _dev(gv), _dev(gj))
    b = L.lbs_backward(_dev(betas), _dev(pose), *consts, _dev(gv), _dev(gj))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    for f in (0, 5, 16):
        one = L.lbs_backward(_dev(betas[f:f + 1]), _dev(pose[f:f + 1]), *consts, _dev(gv[f:f + 1]), _dev(gj[f:f + 1]))
        assert np.array_equal(_bits(one[0])[0], _bits(a[0])[f]) and np.array_equal(_bits(one[1])[0], _bits(a[1])[f]), f


def test_zero_upstream_gradients_give_zero_outputs():
    P, betas, pose, gv, gj = _exact_case()
    consts = _consts(P)
    for zv, zj in ((torch.zeros_like(_dev(gv)), torch.zeros_like(_dev(gj))), (None, None), (torch.zeros_like(_dev(gv)), None)):
        for bt in (betas, betas[:1]):
            db, dp = L.lbs_backward(_dev(bt), _dev(pose), *consts, zv, zj)
            assert tuple(db.shape) == bt.shape and (db == 0).all() and (dp == 0).all()


def test_a_frame_with_nan_pose_leaves_every_other_frames_bits():
    P, betas, pose, gv, gj = _exact_case()
    consts = _consts(P)
    a = L.lbs_backward(_dev(betas), _dev(pose), *consts, _dev(gv), _dev(gj))
    bad = pose.copy()
    bad[3] = np.nan
    b = L.lbs_backward(_dev(betas), _dev(bad), *consts, _dev(gv), _dev(gj))
    keep = np.arange(17) != 3
    assert np.array_equal(_bits(a[0])[keep], _bits(b[0])[keep]) and np.array_equal(_bits(a[1])[keep], _bits(b[1])[keep])
    assert torch.isnan(b[1][3]).any()


def test_lbs_backward_replayed_from_a_hip_graph_gives_the_eager_bits():
    P, betas, pose, gv, gj = _exact_case()
    consts = _consts(P)
    args = (_dev(betas), _dev(pose), *consts, _dev(gv), _dev(gj))
    eager = L.lbs_backward(*args)      # (also prepares the model constants: host work stays outside the capture)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        L.lbs_backward(*args)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = L.lbs_backward(*args)
    for _ in range(2):
        out[0].fill_(7.0)
        out[1].fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(out, eager))


# ------------------------------------------------------------------------------------------------------------------------- the body models
def _body(cls, V=97, **kw):
    P = syn.smpl_like_params(V=V, seed=41)
    faces = np.stack([np.arange(V - 2), np.arange(1, V - 1), np.arange(2, V)], 1).astype(np.int64)
    return cls("", data_struct=Struct(**syn.smpl_data_struct(P, faces)), gender="female", num_betas=10, **kw).cuda()


def test_smpl_with_its_own_parameters_gets_gradients_on_those_four_and_nothing_else():
    B = 3
    betas, pose = syn.smpl_like_pose(B, seed=42)
    rng = np.random.default_rng(43)
    body = _body(SMPL, batch_size=B, betas=betas, global_orient=pose[:, :3], body_pose=pose[:, 3:], transl=rng.standard_normal((B, 3)).astype(np.float32))
    out0 = body()
    assert out0.vertices.grad_fn is None and out0.joints.grad_fn is None and not out0.vertices.requires_grad        # flag off: no graph
    with torch.no_grad(), _on():
        assert body().vertices.grad_fn is None                                                                      # flag on, grad off: no graph
    gv = _dev(rng.standard_normal((B, 97, 3)))
    with _on():
        out = body()
        assert np.array_equal(_bits(out.vertices), _bits(out0.vertices))
        (out.vertices * gv).sum().backward()
    named = dict(body.named_parameters())
    assert sorted(named) == ["betas", "body_pose", "global_orient", "transl"]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any() for p in named.values())
    assert all(b.grad is None for b in body.buffers())
    assert torch.equal(body.transl.grad, gv.sum(1))                                                                 # torch's own add
    # the same numbers through the functional form
    full = torch.cat([body.global_orient, body.body_pose], 1).detach()
    db, dp = L.lbs_backward(body.betas.detach(), full, body.v_template, body.shapedirs, body.posedirs, body.J_regressor, body.parents, body.lbs_weights, gv, None)
    assert torch.equal(db, body.betas.grad) and torch.equal(dp[:, :3], body.global_orient.grad) and torch.equal(dp[:, 3:], body.body_pose.grad)


def test_smpl_layer_with_rotation_matrices_gets_gradients_on_its_inputs():
    B = 2
    betas, pose = syn.smpl_like_pose(B, seed=44)
    rng = np.random.default_rng(45)
    rot = ST.rodrigues(pose.reshape(-1, 3))[0].reshape(B, 24, 3, 3)
    body = _body(SMPLLayer)
    ins = dict(betas=_dev(betas).requires_grad_(True), global_orient=_dev(rot[:, :1]).requires_grad_(True), body_pose=_dev(rot[:, 1:]).requires_grad_(True),
               transl=_dev(rng.standard_normal((B, 3))).requires_grad_(True))
    out0 = body(**ins)
    assert out0.vertices.grad_fn is None and out0.joints.grad_fn is None                                            # flag off: no graph
    gv, gj = _dev(rng.standard_normal((B, 97, 3))), _dev(rng.standard_normal((B, 24, 3)))
    with _on():
        out = body(**ins)
        assert np.array_equal(_bits(out.vertices), _bits(out0.vertices))
        ((out.vertices * gv).sum() + (out.joints[:, :24] * gj).sum()).backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() for t in ins.values())
    assert list(body.parameters()) == [] and all(b.grad is None for b in body.buffers())
    assert torch.equal(ins["transl"].grad, gv.sum(1) + gj.sum(1))
    # the same numbers through the functional form
    full = torch.cat([ins["global_orient"], ins["body_pose"]], 1).detach()
    db, dp = L.lbs_backward(ins["betas"].detach(), full, body.v_template, body.shapedirs, body.posedirs, body.J_regressor, body.parents, body.lbs_weights, gv, gj,
                            pose2rot=False)
    assert torch.equal(db, ins["betas"].grad) and torch.equal(dp[:, :1], ins["global_orient"].grad) and torch.equal(dp[:, 1:], ins["body_pose"].grad)

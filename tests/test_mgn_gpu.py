"""The MGN model variant (`PCALBSGarmentUseSegEncoderSegMGN`, modules/mesh_encoder.py:489-614) on the GPU: the fused nearest-vertex
skinning launch (g4d_mgn_skin_f32) against g4d_knn_f32(K = 1) and a float64 restatement, `lbs_garment_MGN` and the post-encoder
`forward` against the reference's own outputs (tests/golden/mgn.npz), the NaN guard of the displacement path, and the model as a whole."""
import os
import types

import numpy as np
import pytest
import torch

from garment4d_amd import _lib
from garment4d_amd import lbs as L
from garment4d_amd import numerics
from garment4d_amd import synthetic as syn
from garment4d_amd.knn import knn_points
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSegMGN
from oracle import pointnet2_oracle as PO
from oracle import refine_oracle as RO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mgn.npz")
MODES = ("nvcc", "off", "chain")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _transforms(F_, J, seed):
    """(F,J,4,4) rigid joint transforms from the lbs helpers: random axis-angle poses about random joints."""
    rng = np.random.default_rng(seed)
    parents = syn.SMPL_PARENTS if J == 24 else np.array([-1] + [int(rng.integers(0, i)) for i in range(1, J)], dtype=np.int64)
    rot = L.batch_rodrigues(dev((rng.standard_normal((F_ * J, 3)) * 0.3).astype(np.float32))).reshape(F_, J, 3, 3)
    joints = dev((rng.standard_normal((F_, J, 3)) * 0.3).astype(np.float32))
    return L.batch_rigid_transform(rot, joints, parents)[1]


def _weights(F_, V, J, seed):
    rng = np.random.default_rng(seed)
    w = rng.random((F_, V, J)).astype(np.float32) ** 4
    return (w / w.sum(-1, keepdims=True)).astype(np.float32)


def _skin(clips, T, garment, root, tpose, W, inv_A, A):
    """g4d_mgn_skin_f32 -> (idx (F,Vg), dist (F,Vg), stage1 (F,Vg,3), posed (F,Vg,3))."""
    F_, Vg = clips * T, garment.shape[-2]
    V, J = tpose.shape[-2], W.shape[-1]
    d = garment.device
    idx = torch.full((F_, Vg), -7, dtype=torch.int32, device=d)
    dist = torch.full((F_, Vg), -7.0, dtype=torch.float32, device=d)
    s1 = torch.full((F_, Vg, 3), -7.0, dtype=torch.float32, device=d)
    p = torch.full((F_, Vg, 3), -7.0, dtype=torch.float32, device=d)
    _lib.call("g4d_mgn_skin_f32", clips, T, Vg, V, J, garment.data_ptr(), root.data_ptr(), tpose.data_ptr(), W.data_ptr(), inv_A.data_ptr(),
              A.data_ptr(), idx.data_ptr(), dist.data_ptr(), s1.data_ptr(), p.data_ptr(), _lib.stream_ptr())
    return idx, dist, s1, p


def _case(clips, T, Vg, V, J=24, seed=0, ties=False):
    rng = np.random.default_rng(seed)
    if ties:   # body on an integer lattice with every vertex duplicated, queries at cell centres and on lattice points: exact ties
        base = rng.integers(-3, 4, size=(clips, (V + 1) // 2, 3)).astype(np.float32)
        tpose = np.repeat(base, 2, axis=1)[:, :V] * np.float32(0.25)
        garment = (rng.integers(-6, 7, size=(clips * T, Vg, 3)).astype(np.float32) * np.float32(0.125))
        root = np.zeros((clips, 3), np.float32)
    else:
        tpose = (rng.standard_normal((clips, V, 3)) * np.array([0.25, 0.6, 0.15])).astype(np.float32)
        garment = (rng.standard_normal((clips * T, Vg, 3)) * np.array([0.3, 0.6, 0.2])).astype(np.float32)
        root = (rng.standard_normal((clips, 3)) * 0.05).astype(np.float32)
    return dict(garment=dev(garment), root=dev(root), tpose=dev(tpose), W=dev(_weights(clips * T, V, J, seed + 1)),
                inv_A=_transforms(clips * T, J, seed + 2), A=_transforms(clips * T, J, seed + 3))


def _queries(c, clips, T):
    """q = garment + root[c] (one fp32 add, as the kernel and the reference), clip-major (clips, T*Vg, 3)."""
    g = c["garment"].reshape(clips, -1, 3)
    return (g + c["root"].reshape(clips, 1, 3)).contiguous()


# (clips, frames_per_clip, Vg, V)
KNN_SHAPES = [(1, 30, 4096, 6890),                                                     # the cfg4 clip
              (2, 3, 100, 1), (2, 3, 100, 2), (2, 3, 100, 63), (2, 3, 100, 64), (2, 3, 100, 65), (2, 3, 100, 257),
              (3, 1, 77, 300), (2, 30, 65, 500),                                       # frames_per_clip 1 and 30, Vg not a multiple of 64
              (1, 2, 300, 20000)]                                                      # T-pose of 240 KB: many LDS tiles


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("clips,T,Vg,V", KNN_SHAPES)
def test_search_equals_knn_k1(mode, clips, T, Vg, V):
    c = _case(clips, T, Vg, V, seed=clips * 7 + V)
    with numerics.distance_contraction(mode):
        idx, dist, _, _ = _skin(clips, T, **c)
        want = knn_points(_queries(c, clips, T), c["tpose"], K=1)
    assert torch.equal(idx.reshape(-1).long(), want.idx.reshape(-1))
    assert torch.equal(dist.reshape(-1).view(torch.int32), want.dists.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("clips,T,Vg,V", [(2, 3, 130, 64), (1, 4, 65, 257), (2, 1, 200, 2049)])
def test_search_ties_equal_knn_k1(mode, clips, T, Vg, V):
    """Duplicated body vertices and queries exactly equidistant from several vertices: the lowest index wins, as in g4d_knn_f32."""
    c = _case(clips, T, Vg, V, seed=V, ties=True)
    with numerics.distance_contraction(mode):
        idx, dist, _, _ = _skin(clips, T, **c)
        want = knn_points(_queries(c, clips, T), c["tpose"], K=1)
    d_all = ((_queries(c, clips, T).double().unsqueeze(2) - c["tpose"].double().unsqueeze(1)) ** 2).sum(-1)    # exact: lattice coordinates
    assert int((d_all == d_all.min(-1, keepdim=True)[0]).sum(-1).max()) >= 4        # the case really has ties
    assert torch.equal(idx.reshape(-1).long(), want.idx.reshape(-1))
    assert torch.equal(dist.reshape(-1).view(torch.int32), want.dists.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("mode", MODES)
def test_search_beyond_knn_limit_equals_oracle(mode):
    """V = 40000 > 32768, which g4d_knn_f32 refuses: the CPU oracle's knn_points under the same contraction mode."""
    clips, T, Vg, V = 1, 2, 40, 40000
    c = _case(clips, T, Vg, V, seed=5)
    prev = PO.set_contraction(mode)
    try:
        with numerics.distance_contraction(mode):
            idx, dist, _, _ = _skin(clips, T, **c)
        wd, wi = RO.knn_points(_queries(c, clips, T).cpu().numpy(), c["tpose"].cpu().numpy(), 1)
    finally:
        PO.set_contraction(prev)
    np.testing.assert_array_equal(idx.cpu().numpy().reshape(-1), wi.reshape(-1))
    np.testing.assert_array_equal(dist.cpu().numpy().reshape(-1).view(np.int32), wd.astype(np.float32).reshape(-1).view(np.int32))


@pytest.mark.parametrize("clips,T,Vg", [(0, 3, 10), (2, 0, 10), (2, 3, 0)])
def test_zero_sizes_launch_nothing(clips, T, Vg):
    c = _case(2, 3, 10, 50)
    sentinel = torch.full((4,), -7.0, device="cuda")
    _lib.call("g4d_mgn_skin_f32", clips, T, Vg, 50, 24, c["garment"].data_ptr(), c["root"].data_ptr(), c["tpose"].data_ptr(), c["W"].data_ptr(),
              c["inv_A"].data_ptr(), c["A"].data_ptr(), sentinel.data_ptr(), sentinel.data_ptr(), sentinel.data_ptr(), sentinel.data_ptr(),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (sentinel == -7.0).all()


def test_bad_sizes_are_refused():
    c = _case(1, 1, 8, 16, J=8)
    with pytest.raises(_lib.G4DError, match="J"):
        _lib.call("g4d_mgn_skin_f32", 1, 1, 8, 16, 65, c["garment"].data_ptr(), c["root"].data_ptr(), c["tpose"].data_ptr(), c["W"].data_ptr(),
                  c["inv_A"].data_ptr(), c["A"].data_ptr(), 0, 0, 0, 0, _lib.stream_ptr())
    with pytest.raises(_lib.G4DError, match="V = 0"):
        _lib.call("g4d_mgn_skin_f32", 1, 1, 8, 0, 8, c["garment"].data_ptr(), c["root"].data_ptr(), c["tpose"].data_ptr(), c["W"].data_ptr(),
                  c["inv_A"].data_ptr(), c["A"].data_ptr(), 0, 0, 0, 0, _lib.stream_ptr())


def _restate64(c, clips, T, nn):
    """float64 restatement of the two blends at the given nearest vertices: s = (sum_j W inv_A_j) [q; 1], p = (sum_j W A_j) [s; 1]."""
    F_, Vg = nn.shape
    q = _queries(c, clips, T).reshape(F_, Vg, 3).double()
    w = torch.gather(c["W"].double(), 1, nn.long().unsqueeze(-1).expand(F_, Vg, c["W"].shape[-1]))          # (F,Vg,J)
    Mi = torch.einsum("fgj,fjab->fgab", w, c["inv_A"].double())
    M = torch.einsum("fgj,fjab->fgab", w, c["A"].double())
    s = (Mi[..., :3, :3] @ q.unsqueeze(-1)).squeeze(-1) + Mi[..., :3, 3]
    p = (M[..., :3, :3] @ s.unsqueeze(-1)).squeeze(-1) + M[..., :3, 3]
    return s, p, q


@pytest.mark.parametrize("clips,T,Vg,V,J", [(1, 2, 4096, 6890, 24), (2, 3, 100, 1, 24), (3, 5, 70, 257, 64), (1, 2, 300, 20000, 1),
                                            (2, 1, 65, 65, 7)])
def test_blends_against_float64(clips, T, Vg, V, J):
    c = _case(clips, T, Vg, V, J=J, seed=V + J)
    idx, dist, s1, p = _skin(clips, T, **c)
    s64, p64, q64 = _restate64(c, clips, T, idx)
    np.testing.assert_allclose(s1.cpu().numpy(), s64.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(p.cpu().numpy(), p64.cpu().numpy(), rtol=1e-5, atol=1e-5)
    # nearest vertex against a float64 argmin: a flip only where the two float64 distances are within a few fp32 ulps
    tp = c["tpose"].double().reshape(clips, 1, V, 3)
    F_ = clips * T
    d64 = ((q64.reshape(clips, T * Vg, 1, 3) - tp) ** 2).sum(-1).reshape(F_, Vg, V)
    best = d64.min(-1)[0]
    mine = torch.gather(d64, 2, idx.long().unsqueeze(-1)).squeeze(-1)
    flips = mine != best
    ulp = torch.from_numpy(np.spacing(best.cpu().numpy().astype(np.float32)).astype(np.float64)).cuda()
    assert bool(((mine - best) <= 4 * ulp).all()), f"{int(flips.sum())} flips, worst {float(((mine - best) / ulp).max())} ulp"
    assert int(flips.sum()) <= max(1, F_ * Vg // 1000)


# ---------------------------------------------------------------- against the reference's own outputs (tests/golden/make_golden_mgn.py)

def _golden():
    z = np.load(GOLDEN)
    sd = syn.mgn_displacement_state_dict(int(z["in_template_verts"].shape[0]), seed=int(z["seed"]) + 100)
    np.testing.assert_allclose(np.array([float(np.asarray(sd[k], np.float64).sum()) for k in sorted(sd)]), z["displacement_checksum"], rtol=1e-12)
    return z, sd


def _golden_model(z, sd):
    pca = dict(components=np.zeros((72, z["in_template_verts"].size), np.float32), mean=z["in_template_verts"].reshape(-1), explained=np.ones(72),
               ss_scale=np.ones(z["in_template_verts"].size))
    m = PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=pca, template=(z["in_template_verts"], z["in_template_faces"]))
    m.displacement_encoder.load_state_dict({k.split(".", 1)[1]: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda().eval()


def _golden_batch(z):
    return {k[3:]: dev(z[k]) for k in z.files if k.startswith("in_") and k[3:] in (
        "Tpose_smpl_vertices_torch", "Tpose_smpl_root_joints_torch", "zeropose_smpl_vertices_torch", "pose_torch", "T_J_regressor", "T_lbs_weights")}


def _body_model_from(z):
    return types.SimpleNamespace(parents=torch.from_numpy(z["in_parents"]).cuda(), faces=None, J_regressor=dev(z["in_J_regressor"]))


def test_lbs_garment_mgn_matches_reference():
    z, sd = _golden()
    m = _golden_model(z, sd)
    b = _golden_batch(z)
    with torch.no_grad():
        posed, nn1, stage1 = m.lbs_garment_MGN(dev(z["in_pred_template"]), b["Tpose_smpl_vertices_torch"], b["Tpose_smpl_root_joints_torch"],
                                               b["zeropose_smpl_vertices_torch"], _body_model_from(z), b["pose_torch"], b["T_J_regressor"],
                                               b["T_lbs_weights"], K=1)
    assert nn1.idx.dtype == torch.int64 and tuple(nn1.idx.shape) == tuple(z["lbs_nn_idx"].shape)
    np.testing.assert_array_equal(nn1.idx.cpu().numpy(), z["lbs_nn_idx"])
    np.testing.assert_array_equal(nn1.dists.cpu().numpy(), z["lbs_nn_dists"])
    np.testing.assert_allclose(stage1.cpu().numpy(), z["lbs_stage1"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(posed.cpu().numpy(), z["lbs_posed"], rtol=1e-5, atol=1e-5)
    with pytest.raises(AssertionError):
        m.lbs_garment_MGN(dev(z["in_pred_template"]), b["Tpose_smpl_vertices_torch"], b["Tpose_smpl_root_joints_torch"],
                          b["zeropose_smpl_vertices_torch"], _body_model_from(z), b["pose_torch"], b["T_J_regressor"], b["T_lbs_weights"], K=3)


def _post_encoder_forward(m, z, nan_rows=None):
    """forward() with the garment encoder's output replaced by the golden's (tpose_garment, garment_summary), as the generator's stub."""
    nb, T = z["in_garment_summary"].shape[:2]
    enc = dict(tpose_garment=dev(z["in_tpose_garment"]), garment_summary=dev(z["in_garment_summary"]))
    m.PCA_garment_encoder.forward = lambda *a, **k: dict(enc)
    if nan_rows is not None:
        with torch.no_grad():
            m.displacement_encoder[4].weight[torch.from_numpy(nan_rows).cuda()] = float("nan")
    with torch.no_grad():
        return m(torch.zeros(nb, T, 4, 3, device="cuda"), _body_model_from(z), _golden_batch(z))


@pytest.mark.parametrize("tag", ["fwd", "fwd_nan"])
def test_forward_matches_reference(tag):
    z, sd = _golden()
    m = _golden_model(z, sd)
    out = _post_encoder_forward(m, z, z["nan_rows"] if tag == "fwd_nan" else None)
    # the displacement MLP runs on the matrix cores here and in torch's CPU GEMM there: the queries agree to rounding, the nearest vertices exactly
    np.testing.assert_array_equal(out["lbs_nn"].idx.cpu().numpy(), z[tag + "_nn_idx"])
    np.testing.assert_allclose(out["lbs_nn"].dists.cpu().numpy(), z[tag + "_nn_dists"], rtol=1e-5, atol=1e-7)
    for key, want in (("lbs_stage1_pred_garment_v", z[tag + "_stage1"]), ("lbs_pred_garment_v", z[tag + "_posed"])):
        got = out[key].cpu().numpy()
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=key)
    assert len(out["iter_regressed_lbs_garment_v"]) == 1
    np.testing.assert_allclose(out["iter_regressed_lbs_garment_v"][0].cpu().numpy(), z[tag + "_iter0"], rtol=1e-5, atol=1e-5)
    lap = out["lap_adj"].coalesce()
    np.testing.assert_array_equal(lap.indices()[0].cpu().numpy(), z["lap_row"])
    np.testing.assert_array_equal(lap.indices()[1].cpu().numpy(), z["lap_col"])
    np.testing.assert_allclose(lap.values().cpu().numpy(), z["lap_val"], rtol=1e-6)


def test_nan_rows_get_exactly_zero_displacement():
    z, sd = _golden()
    m = _golden_model(z, sd)
    summary = dev(z["in_garment_summary"]).reshape(-1, 512)
    with torch.no_grad():
        clean = m.displacements(summary).reshape(summary.shape[0], -1).cpu().numpy()
        m.displacement_encoder[4].weight[torch.from_numpy(z["nan_rows"]).cuda()] = float("nan")
        dirty = m.displacements(summary).reshape(summary.shape[0], -1).cpu().numpy()
    rows = z["nan_rows"]
    assert (dirty[:, rows] == 0).all() and not (clean[:, rows] == 0).any()
    keep = np.setdiff1d(np.arange(clean.shape[1]), rows)
    assert np.isfinite(dirty).all()
    np.testing.assert_array_equal(dirty[:, keep], clean[:, keep])


# ---------------------------------------------------------------- the model on the synthetic scene

def _scene_model(scene, seed=0):
    from garment4d_amd.encoder import seed_encoder
    torch.manual_seed(seed)
    m = PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"])
    seed_encoder(m.PCA_garment_encoder, seed)
    return m.cuda().eval()


def _scene_body_model(body):
    return types.SimpleNamespace(parents=torch.from_numpy(body["parents"]).cuda(), faces=body["faces"], J_regressor=dev(body["J_regressor"]))


def test_model_outputs_and_state_dict():
    nbatch, T, N = 2, 3, 2048
    scene = syn.garment_scene(nbatch, T, N, seed=31)
    m = _scene_model(scene)
    Vg = scene["template"][0].shape[0]
    with torch.no_grad():
        out = m(dev(scene["x"]), _scene_body_model(scene["body"]), {k: dev(v) for k, v in scene["batch"].items()})
    for k in ("feat_global", "sem_logits", "garment_v_list", "garment_summary", "garment_PCA_coeff", "tpose_garment", "lap_adj",
              "lbs_pred_garment_v", "lbs_nn", "lbs_stage1_pred_garment_v", "iter_regressed_lbs_garment_v"):
        assert k in out, k
    assert tuple(out["lbs_pred_garment_v"].shape) == (nbatch, T, Vg, 3)
    assert tuple(out["lbs_stage1_pred_garment_v"].shape) == (nbatch, T, Vg, 3)
    assert tuple(out["lbs_nn"].idx.shape) == (nbatch * T, Vg, 1) and out["lbs_nn"].idx.dtype == torch.int64
    assert tuple(out["lbs_nn"].dists.shape) == (nbatch * T, Vg, 1)
    assert len(out["iter_regressed_lbs_garment_v"]) == 1 and tuple(out["iter_regressed_lbs_garment_v"][0].shape) == (nbatch * T, Vg, 3)
    assert torch.isfinite(out["lbs_pred_garment_v"]).all()
    # a reference checkpoint's keys (the golden's list, from the reference's own constructor) load strictly
    keys = np.load(GOLDEN)["state_dict_keys"].tolist()
    mine = m.state_dict()
    m.load_state_dict({k: mine[k].clone() for k in keys}, strict=True)


def _mgn_rank_worker(rank, world, port, nbatch, T, N, ret):
    """One rank of the frame-sharded MGN forward; both ranks share cuda:0, the clip max over gloo."""
    import torch.distributed as dist
    from garment4d_amd import dist as gd
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        scene = syn.garment_scene(nbatch, T, N, seed=21)
        m = _scene_model(scene)
        b, e = gd.shard_range(nbatch * T, rank, world)
        flat = {k: v.reshape((nbatch * T,) + v.shape[2:]) for k, v in scene["batch"].items()
                if k in ("zeropose_smpl_vertices_torch", "pose_torch", "T_J_regressor", "T_lbs_weights")}
        batch = {k: dev(v[b:e]) for k, v in flat.items()}
        batch["Tpose_smpl_vertices_torch"] = dev(scene["batch"]["Tpose_smpl_vertices_torch"].reshape(nbatch, -1, 3))
        batch["Tpose_smpl_root_joints_torch"] = dev(scene["batch"]["Tpose_smpl_root_joints_torch"].reshape(nbatch, 3))
        x = dev(scene["x"].reshape(nbatch * T, N, 3)[b:e])
        with torch.no_grad():
            out = m.forward_frames(x, _scene_body_model(scene["body"]), batch, nbatch=nbatch, T=T, frame_ids=range(b, e))
        ret[rank] = dict(range=(b, e), coeff=out["garment_PCA_coeff"].cpu().numpy(), posed=out["lbs_pred_garment_v"].cpu().numpy(),
                         stage1=out["lbs_stage1_pred_garment_v"].cpu().numpy(), idx=out["lbs_nn"].idx.cpu().numpy(),
                         final=out["iter_regressed_lbs_garment_v"][-1].cpu().numpy())
    finally:
        dist.destroy_process_group()


def test_forward_frames_two_ranks_equals_unsharded():
    """Frames split over two ranks with the boundary inside a clip: the union of the ranks' outputs equals the single-process forward."""
    import socket
    import torch.multiprocessing as mp
    nbatch, T, N = 3, 3, 2048
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_mgn_rank_worker, args=(r, 2, port, nbatch, T, N, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    scene = syn.garment_scene(nbatch, T, N, seed=21)
    m = _scene_model(scene)
    with torch.no_grad():
        ref = m(dev(scene["x"]), _scene_body_model(scene["body"]), {k: dev(v) for k, v in scene["batch"].items()})
    assert ret[0]["range"] == (0, 5) and ret[1]["range"] == (5, 9)
    for r in (0, 1):
        np.testing.assert_allclose(ret[r]["coeff"], ref["garment_PCA_coeff"].cpu().numpy(), rtol=1e-6, atol=1e-6, err_msg="coeff")
    cat = lambda k: np.concatenate([ret[0][k], ret[1][k]], 0)
    np.testing.assert_array_equal(cat("idx"), ref["lbs_nn"].idx.cpu().numpy())
    np.testing.assert_allclose(cat("posed"), ref["lbs_pred_garment_v"].reshape(nbatch * T, -1, 3).cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg="posed")
    np.testing.assert_allclose(cat("stage1"), ref["lbs_stage1_pred_garment_v"].reshape(nbatch * T, -1, 3).cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cat("final"), ref["iter_regressed_lbs_garment_v"][-1].cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg="final")

"""The HIP encoders against tests/golden/encoder.npz -- outputs of the REFERENCE's own PCAGarmentEncoderSeg.forward (E1) and
Pointnet2MSGSEG(input_channels=3, global_feat=True) in eval (E2) and BatchNorm-recalibration (E3) mode (make_golden_encoder.py) -- plus
the guards those modes need: a model whose BatchNorm was switched back to train() must take the op-by-op route (or be refused by the
inference-only classes), and a feature tensor of the wrong width or point count must raise instead of being contracted against part of
the first layer.  Reads only tests/golden/."""
import numpy as np
import pytest
import torch

import encoder_golden as EG
from garment4d_amd import mesh_utils as MU, pointnet2_modules as PM
from garment4d_amd.encoder import Pointnet2MSGSEG
from garment4d_amd.mesh_encoder import PCAGarmentEncoderSeg
from oracle import model_oracle as MOr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return EG.golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def npy(t):
    return None if t is None else t.detach().cpu().numpy()


def _load(model, sd):
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model.cuda().eval()


def _e1_models(case, g):
    kw = dict(garment_name="Tshirt", pca_dim=64, pca=case["pca"], template=case["template"])
    model = PCAGarmentEncoderSeg(**kw)
    sd = EG.e1_state_dict(g, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    seg = PCAGarmentEncoderSeg(only_seg=True, **kw)
    return _load(model, sd), _load(seg, {k: v for k, v in sd.items() if k.startswith("pointnet.")})


def _e2_model(case, g):
    model = Pointnet2MSGSEG(input_channels=3, global_feat=True)
    return _load(model, EG.e2_state_dict(g, {k: tuple(v.shape) for k, v in model.state_dict().items()}, case))


def _recalibration_mode(model):
    """model.eval(), then every BatchNorm back to train(): the reference then normalises with batch statistics and updates the running
    stats (ordinary BN recalibration); Dropout stays in eval."""
    model.eval()
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.train()
    return model


def test_pca_garment_encoder_vs_reference(golden):
    """E1 through the HIP PCAGarmentEncoderSeg: labels equal (or admissible where non-garment classes tie), sampled / compacted
    coordinates and the triangle list exact, every float output at rtol = atol = 1e-5 -- except what follows the group-all summary
    (garment_summary, garment_PCA_coeff, tpose_garment) at 2e-5: GarmentSummarize contracts 387 then 512 channels to |v| up to 54
    with another summation order than the reference's CPU GEMM.  Measured on an MI355X: sem_logits 2.4e-6, feature_list 2.9e-6,
    garment_f_list 6.0e-6, garment_summary 1.03e-5, garment_PCA_coeff 1.20e-5, tpose_garment 2.9e-6."""
    g, case = golden
    model, seg = _e1_models(case, g)
    with torch.no_grad():
        od = model(dev(case["x"]))
        od_seg = seg(dev(case["x"]))
    logits = npy(od["sem_logits"])
    labels = np.argmax(logits, 2)
    want = g["e1_labels"].astype(np.int64)
    assert np.array_equal(labels == EG.TARGET, want == EG.TARGET)           # the garment decision: exact at every point
    MOr.admissible_labels(logits, want)                                      # elsewhere: the reference's class is tied with ours
    errs = {"sem_logits": EG.check_logits(g, "e1_sem_logits", logits), "only_seg": EG.check_logits(g, "e1_seg_sem_logits", npy(od_seg["sem_logits"]))}
    assert np.array_equal(npy(od_seg["sem_logits"]), logits)
    assert np.array_equal(npy(od["xyz_list"][0]), case["x"].reshape(4, -1, 3))
    for lvl in (1, 2, 3):
        assert np.array_equal(npy(od["xyz_list"][lvl]), g[f"e1_xyz{lvl}"]), lvl
    for lvl in (0, 1, 2):
        assert np.array_equal(npy(od["garment_v_list"][lvl]), g[f"e1_garment_v{lvl}"]), lvl
    assert np.array_equal(np.asarray(od["garment_f_3"]), g["e1_garment_f_3"])
    errs["feature_list"] = EG.check_feats(g, "e1_feature", [npy(f) for f in od["feature_list"]])
    errs["garment_f_list"] = EG.check_feats(g, "e1_garment_f", [npy(f) for f in od["garment_f_list"]])
    for k in ("garment_summary", "garment_PCA_coeff", "tpose_garment"):
        errs[k] = EG.err(npy(od[k]), g["e1_" + k])
        assert npy(od[k]).shape == g["e1_" + k].shape, k
    print("E1 max elementwise errors:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k in ("garment_summary", "garment_PCA_coeff", "tpose_garment"):
        assert errs[k] <= 2e-5, f"{k}: max elementwise err {errs[k]:.3e} > 2e-5"


def _check_e(g, tag, out, tol):
    mid, logits, l_f, l_xyz = out
    for lvl in (1, 2, 3):
        assert np.array_equal(npy(l_xyz[lvl]), g[f"{tag}_xyz{lvl}"]), lvl
    return max(EG.close(npy(mid), g[f"{tag}_feat_global"], tol, "feat_global"), EG.check_logits(g, f"{tag}_sem_logits", npy(logits), tol),
               EG.check_feats(g, f"{tag}_feature", [npy(f) for f in l_f], tol))


def test_pointnet2msgseg_with_input_features_and_middle_vs_reference(golden):
    """E2 -- input_channels = 3, global_feat = True, eval -- by all four routes: model(pc) (the whole-model drop-in), forward_fused, the
    op-by-op modules, and the reference's own loop over the drop-in modules.  Measured on an MI355X: 1.78e-5 (both fused routes), 1.87e-5
    (reference loop), 1.94e-5 (op-by-op), all at feat_global, |v| ~ 17 after the Middle module's 387-channel contraction (the CPU oracle:
    1.04e-5); gate 3e-5."""
    g, case = golden
    model = _e2_model(case, g)
    pc = dev(case["pc"])
    errs = {}
    with torch.no_grad():
        errs["model(pc)"] = _check_e(g, "e2", model(pc), 3e-5)
        errs["forward_fused"] = _check_e(g, "e2", model.forward_fused(pc, channel_major=True), 3e-5)
        with PM.op_by_op():
            errs["op_by_op"] = _check_e(g, "e2", model(pc), 3e-5)
        errs["reference_loop"] = _check_e(g, "e2", EG.reference_encoder_loop(model, pc), 3e-5)
    print("E2 max elementwise errors:", {k: f"{v:.2e}" for k, v in errs.items()})


E3_TOL = 1e-4


def test_bn_recalibration_takes_batch_statistics(golden):
    """E3 -- E2's model with every BatchNorm back in train() under no_grad -- through model(pc) and the reference's loop over the drop-in
    modules: batch statistics, and the running stats updated as the reference updates them.  (Before the guard, the fused route folded
    BN from the running stats and never updated them: feat_global off by 12.4.)  Batch statistics are reduced in another order on the GPU
    than on the CPU.  Measured on an MI355X over two runs: outputs 3.9e-5 and 5.6e-5 (both routes), running stats 1.1e-6; gate E3_TOL = 1e-4, the cap (3x the
    measured maximum would exceed it)."""
    g, case = golden
    keys = [str(k) for k in g["e3_bn_keys"]]
    errs, outs = {}, {}
    for route in ("model(pc)", "reference_loop"):
        model = _recalibration_mode(_e2_model(case, g))
        pc = dev(case["pc"])
        with torch.no_grad():
            out = model(pc) if route == "model(pc)" else EG.reference_encoder_loop(model, pc)
        sd = model.state_dict()
        outs[route] = (out, sd)
        errs[route] = _check_e(g, "e3", out, 1.0)
        errs[route + " running stats"] = max(EG.close(npy(sd[k]), g[f"e3_bn{i}"], 1.0, k) for i, k in enumerate(keys))
    print("E3 max elementwise errors:", {k: f"{v:.2e}" for k, v in errs.items()})
    for route, (out, sd) in outs.items():
        _check_e(g, "e3", out, E3_TOL)
        for i, k in enumerate(keys):
            EG.close(npy(sd[k]), g[f"e3_bn{i}"], E3_TOL, k)


def test_inference_only_classes_refuse_a_training_submodule(golden):
    """PCAGarmentEncoderSeg folds every BatchNorm from its running stats: a submodule left in train mode is refused, not run."""
    g, case = golden
    model, _ = _e1_models(case, g)
    model.PCAEncoder[1].train()
    with torch.no_grad(), pytest.raises(AssertionError, match="inference only"):
        model(dev(case["x"]))
    model.eval()
    model.pointnet.SA_modules[1].mlps[0].layer0.bn.bn.train()
    with torch.no_grad(), pytest.raises(AssertionError, match="inference only"):
        model(dev(case["x"]))


def test_middle_pool_method_falls_back():
    """A Middle module with a pool method the kernels lack sends model(pc) to the op-by-op route (which raises NotImplementedError, as the
    reference's module does) instead of failing inside the fused route with a KeyError."""
    model = Pointnet2MSGSEG(input_channels=0, global_feat=True).cuda().eval()
    model.Middle_modules.pool_method = "none"
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model(torch.rand(1, 2048, 3, device="cuda"))


# ---- shape guards of the fused SA / FP branches: each bad tensor is WIDER or LONGER than expected, so it is read in bounds even unguarded ----
def _sa(group_all=False):
    torch.manual_seed(5)
    if group_all:
        return PM.PointnetSAModule(mlp=[5, 16, 32]).cuda().eval()
    return PM.PointnetSAModuleMSG(npoint=64, radii=[0.2, 0.4], nsamples=[8, 16], mlps=[[5, 16, 32], [5, 16, 32]]).cuda().eval()


@pytest.mark.parametrize("group_all", [False, True])
def test_sa_refuses_wider_features(group_all):
    """5 feature channels expected (first layer K = 3 + 5); 7 given: the op-by-op route's convolution raises, and so must the fused one."""
    sa = _sa(group_all)
    xyz = torch.rand(2, 512, 3, device="cuda")
    feats = torch.randn(2, 7, 512, device="cuda")
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            sa(xyz, feats)
        with PM.op_by_op(), pytest.raises(RuntimeError):
            sa(xyz, feats)


@pytest.mark.parametrize("group_all", [False, True])
def test_sa_refuses_features_of_more_points(group_all):
    """Features of 520 points for 512 coordinates: refused by the fused route (the op-by-op group-all concatenation raises too)."""
    sa = _sa(group_all)
    xyz = torch.rand(2, 512, 3, device="cuda")
    feats = torch.randn(2, 5, 520, device="cuda")
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            sa(xyz, feats)
        if group_all:
            with PM.op_by_op(), pytest.raises(RuntimeError):
                sa(xyz, feats)


@pytest.mark.parametrize("bad", ["wider_skip", "longer_skip", "longer_known"])
def test_fp_refuses_mismatched_features(bad):
    """FP with C1 = 6 skip and C2 = 16 known channels (first layer K = 22): a wider skip tensor, a skip tensor of more points than
    `unknown`, or known features of more points than `known` are refused (the first two raise on the op-by-op route as well)."""
    torch.manual_seed(6)
    fp = PM.PointnetFPModule(mlp=[22, 32, 16]).cuda().eval()
    unknown, known = torch.rand(2, 512, 3, device="cuda"), torch.rand(2, 64, 3, device="cuda")
    skip = torch.randn(2, 8 if bad == "wider_skip" else 6, 516 if bad == "longer_skip" else 512, device="cuda")
    kf = torch.randn(2, 16, 70 if bad == "longer_known" else 64, device="cuda")
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            fp(unknown, known, skip, kf)
        if bad != "longer_known":
            with PM.op_by_op(), pytest.raises(RuntimeError):
                fp(unknown, known, skip, kf)


def test_whole_model_refuses_wider_input():
    """Pointnet2MSGSEG(input_channels=3) fed 5 feature channels: model(pc) raises on both routes."""
    model = Pointnet2MSGSEG(input_channels=3, global_feat=True).cuda().eval()
    pc = torch.rand(2, 2048, 8, device="cuda")
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            model(pc)
        with PM.op_by_op(), pytest.raises(RuntimeError):
            model(pc)


# ---- segmentation at full size: several 1024-point chunks of the selection kernel ----
def _labels_with_nth_at(rng, N, n, p, extra):
    """Garment mask with the n-th garment point at index p (n - 1 before it), then each later point garment with probability `extra`."""
    m = np.zeros(N, bool)
    m[rng.choice(p, n - 1, replace=False)] = True
    m[p] = True
    m[p + 1:] = rng.random(N - p - 1) < extra
    return m


def test_segment_points_full_size():
    """mesh_utils.segment_points at N = 6890 (n = 1722) against calc_segmentation_results: garment counts n - 1, n and n + 1, the n-th
    garment point inside a chunk (index 1900) and on each side of a chunk boundary (indices 2047 and 2048)."""
    rng = np.random.default_rng(12)
    N, n, C, tgt = 6890, 6890 // 4, 64, EG.TARGET
    masks = []
    for cnt in (n - 1, n, n + 1):
        m = np.zeros(N, bool)
        m[rng.choice(N, cnt, replace=False)] = True
        masks.append(m)
    masks += [_labels_with_nth_at(rng, N, n, p, 0.3) for p in (1900, 2047, 2048)]
    F_ = len(masks)
    logits = rng.standard_normal((F_, N, 7)).astype(np.float32)
    mask = np.stack(masks)
    logits[..., tgt] = np.where(mask, logits.max(2) + 1.0, logits.min(2) - 1.0)
    xyz = rng.standard_normal((F_, N, 3)).astype(np.float32)
    feats = rng.standard_normal((F_, N, C)).astype(np.float32)
    gv, gf, counts = MU.segment_points(dev(logits), tgt, n, dev(xyz), dev(feats))
    wv, wf = MOr.calc_segmentation_results(xyz, logits, n, tgt, feats)
    assert np.array_equal(counts.cpu().numpy(), mask.sum(1))
    assert np.array_equal(gv.cpu().numpy(), wv) and np.array_equal(gf.cpu().numpy(), wf)

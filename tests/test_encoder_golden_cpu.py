"""The numpy oracles of the two encoders against tests/golden/encoder.npz -- outputs of the REFERENCE's own PCAGarmentEncoderSeg.forward
(E1) and Pointnet2MSGSEG(input_channels=3, global_feat=True) in eval (E2) and BatchNorm-recalibration (E3) mode, written by
tests/golden/make_golden_encoder.py.  Pins oracle/model_oracle.garment_encoder_forward and modules_oracle.encoder_forward_full (and so
every GPU test that trusts them) to the reference's wiring.  CPU only."""
import numpy as np
import pytest

import encoder_golden as EG
from garment4d_amd.encoder import Pointnet2MSGSEG
from garment4d_amd.mesh_encoder import PCAGarmentEncoderSeg
from oracle import model_oracle as MOr, modules_oracle as MO, pointnet2_oracle as K


@pytest.fixture(scope="module")
def golden():
    return EG.golden()


def _shapes(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


def _e1_model(case):
    return PCAGarmentEncoderSeg(garment_name="Tshirt", pca_dim=64, pca=case["pca"], template=case["template"])


def test_seeded_state_dicts_regenerate(golden):
    """This package's models have the reference models' keys, and the seeded weights regenerate to the stored per-key checksums."""
    g, case = golden
    sd = EG.e1_state_dict(g, _shapes(_e1_model(case)))
    pca_bn = [k for k in sd if k.startswith("PCAEncoder.") and k.endswith(".weight") and sd[k].ndim == 1]
    assert pca_bn == ["PCAEncoder.1.weight", "PCAEncoder.4.weight"]
    bn_scales = [v for k, v in sd.items() if k[:k.rfind(".") + 1] + "running_mean" in sd and k.endswith(".weight")]
    assert all(((np.abs(v) >= 0.5) & (np.abs(v) <= 1.5)).all() for v in bn_scales)      # every BN non-degenerate, the PCA head's too
    EG.e2_state_dict(g, _shapes(Pointnet2MSGSEG(input_channels=3, global_feat=True)), case)


def test_frame_counts_cover_the_segmentation_edges(golden):
    """The four E1 frames keep every edge of calc_segmentation_results (mesh_encoder.py:109-125): a frame with more than n garment points
    interleaved with others (truncation to the first n), one with 1..n-1 (zero-padded rows), one with none."""
    g, _ = golden
    n, counts, labels = int(g["e1_n"]), g["e1_counts"], g["e1_labels"]
    assert n == 6890 // 4 and labels.shape == (4, 6890)
    assert np.array_equal(counts, (labels == EG.TARGET).sum(1))
    assert ((counts > n) & (counts < 6890)).any()
    assert ((counts >= 1) & (counts < n)).any()
    assert (counts == 0).any()
    assert float(g["e1_min_margin"]) >= 1e-4


def test_model_oracle_reproduces_pca_garment_encoder(golden):
    """E1: garment_encoder_forward = the reference's PCAGarmentEncoderSeg.forward, index tensors exact, floats at 1e-5."""
    g, case = golden
    prev = K.set_contraction("nvcc")
    try:
        sd = EG.e1_state_dict(g, _shapes(_e1_model(case)))
        x = case["x"].reshape(4, case["N"], 3)
        out = MOr.garment_encoder_forward(sd, x, 2, 2, EG.TARGET, case["pca"], decisions=g["e1_labels"].astype(np.int64))
    finally:
        K.set_contraction(prev)
    # the reference's labels: admissible (checked inside) and the same garment decision at every point
    assert np.array_equal(np.argmax(out["sem_logits"], 2) == EG.TARGET, g["e1_labels"] == EG.TARGET)
    EG.check_logits(g, "e1_sem_logits", out["sem_logits"])
    EG.check_logits(g, "e1_seg_sem_logits", out["sem_logits"])
    for lvl in (1, 2, 3):
        assert np.array_equal(out["xyz_list"][lvl], g[f"e1_xyz{lvl}"])
    for lvl in (0, 1, 2):
        assert np.array_equal(out["garment_v_list"][lvl], g[f"e1_garment_v{lvl}"])
    EG.check_feats(g, "e1_feature", out["feature_list"])
    EG.check_feats(g, "e1_garment_f", out["garment_f_list"])
    EG.close(out["garment_summary"], g["e1_garment_summary"], what="garment_summary")
    EG.close(out["garment_PCA_coeff"], g["e1_garment_PCA_coeff"], what="garment_PCA_coeff")
    EG.close(out["tpose_garment"], g["e1_tpose_garment"], what="tpose_garment")
    from garment4d_amd import mesh_utils
    assert np.array_equal(mesh_utils.quads2tris(case["template"][1]), g["e1_garment_f_3"])


@pytest.mark.parametrize("tag", ["e2", "e3"])
def test_modules_oracle_reproduces_pointnet2msgseg(golden, tag):
    """E2 (eval) / E3 (BatchNorm in batch-statistics mode, running stats updated): encoder_forward_full = the reference's
    Pointnet2MSGSEG(input_channels=3, global_feat=True) incl. the Middle group-all module and the input-feature channels."""
    g, case = golden
    sd = EG.e2_state_dict(g, _shapes(Pointnet2MSGSEG(input_channels=3, global_feat=True)), case)
    stats = {} if tag == "e3" else None
    prev = K.set_contraction("nvcc")
    try:
        mid, logits, l_f, l_xyz = MO.encoder_forward_full(case["pc"], sd, global_feat=True, training=tag == "e3", stats=stats)
    finally:
        K.set_contraction(prev)
    # measured: E2 1.04e-5 (feat_global, |v| ~ 17 after the Middle module's 387-channel contraction: float32 summation order), E3 see below;
    # batch statistics are reduced in float64 here and in float32 by torch
    tol = 2e-5 if tag == "e2" else 1e-4
    for lvl in (1, 2, 3):
        assert np.array_equal(l_xyz[lvl], g[f"{tag}_xyz{lvl}"])
    EG.close(mid, g[f"{tag}_feat_global"], tol, "feat_global")
    EG.check_logits(g, f"{tag}_sem_logits", logits, tol)
    EG.check_feats(g, f"{tag}_feature", l_f, tol)
    if tag == "e3":
        keys = [str(k) for k in g["e3_bn_keys"]]
        assert len(stats) * 2 == len(keys) == 54
        for i, k in enumerate(keys):
            prefix, leaf = k[:k.rfind(".") + 1], k[k.rfind(".") + 1:]
            mean, var = stats[prefix]
            want = 0.9 * sd[k].astype(np.float64) + 0.1 * (mean if leaf == "running_mean" else var)     # momentum 0.1
            EG.close(want, g[f"e3_bn{i}"], 1e-5, k)

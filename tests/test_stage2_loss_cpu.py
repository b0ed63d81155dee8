"""The stage-2 objective without a GPU: the float64 twin (tests/stage2_loss_twin.py) against the reference's own run stored in
tests/golden/stage2_loss.npz, the argument checks of g4d_refine_loss_f32 (they happen before the device is touched), its workspace query, and
the opt-in's semantics (tuning.Tuning.refine_autograd: no new field, the asserts where they were)."""
import ctypes
import dataclasses
import types

import numpy as np
import pytest
import torch

import stage2_loss_twin as TW
from garment4d_amd import _lib, synthetic as syn, tuning


@pytest.fixture(scope="module")
def golden():
    g, case = TW.load(), syn.stage2_loss_case()
    assert np.array_equal(g["checksum"], syn.stage2_loss_checksum(case)), "stage2_loss.npz belongs to other inputs: regenerate it"
    return g, case


def test_fixture_conditions(golden):
    g, _ = golden
    assert (g["decisions"] == 0).all()                                        # the reference alone takes the same decisions in both precisions
    assert ((g["penetrating_share"] >= 0.2) & (g["penetrating_share"] <= 0.8)).all()


def test_twin_reproduces_the_reference_float64(golden):
    g, case = golden
    rounds, gt, body, normals, L, nbatch, T = TW.golden_inputs(case)
    rs = [TW.evaluate(p, gt, body, normals, L, nbatch, T, temporal=(i == len(rounds) - 1)) for i, p in enumerate(rounds)]
    vals = [r["values"] for r in rs]
    lbs_pred = case["lbs_pred_garment_v"].reshape(nbatch * T, -1, 3).astype(np.float64)
    twin = {
        "lbs_garment_msre": vals[-1]["msre"], "only_lbs_garment_msre": np.sqrt(((lbs_pred - gt) ** 2).sum(-1)).mean(),
        "lbs_garment_l2_loss": sum(v["l2"] for v in vals), "lbs_garment_lap_loss": sum(v["lap"] for v in vals),
        "lbs_interpenetration_loss": sum(v["pen"] for v in vals), "temporal_constraint_loss": vals[-1]["tmp"],
        "acceleration_error": TW.acceleration_error(rounds[-1], gt, nbatch, T),
        "only_lbs_acceleration_error": TW.acceleration_error(lbs_pred, gt, nbatch, T), "total_loss": TW.total(vals, TW.LAMBDAS),
    }
    for k, v in twin.items():
        ref = float(g[f"f64_{k}"])
        assert abs(v - ref) <= 1e-11 * max(abs(ref), 1e-3), (k, v, ref)
    np.testing.assert_allclose(rs[-1]["msre_frames"].reshape(nbatch, T), g["f64_lbs_garment_msre_list"], rtol=1e-11)
    # the float64 gradients are not stored: the twin's lie within the reference's own fp32 error of the stored fp32 ones
    for i, r in enumerate(rs):
        gr, bound = TW.gradient(r, TW.LAMBDAS if i == len(rs) - 1 else TW.LAMBDAS[:3] + (0.0,))
        err = np.abs(gr - g[f"grad{i}"]).max()
        assert err <= float(g[f"eref_grad{i}"]) * (1 + 1e-6) + 1e-12, (i, err, float(g[f"eref_grad{i}"]))
        assert np.abs(gr).max() == pytest.approx(float(g[f"max64_grad{i}"]), rel=1e-9)
        assert TW.flags(r).mean() <= 0.01
        assert 0.2 <= (r["dot"] < 0).mean() <= 0.8


def test_twin_gradient_is_the_derivative():
    """Central differences of the twin's own total along a random direction (nearest index held fixed, as a constant of the graph)."""
    c = TW.garment_case(5, 2, 3, 13, 15)
    r = TW.evaluate(c["p"], c["g"], c["body"], c["normals"], c["L"], 2, 3)
    g, _ = TW.gradient(r, TW.LAMBDAS)
    dp = np.random.default_rng(0).standard_normal(c["p"].shape)
    p64, h = c["p"].astype(np.float64), 1e-7
    tot = lambda p: TW.total([TW.evaluate(p, c["g"], c["body"], c["normals"], c["L"], 2, 3, nn=r["idx"])["values"]], TW.LAMBDAS)
    fd = (tot(p64 + h * dp) - tot(p64 - h * dp)) / (2 * h)
    assert fd == pytest.approx((g * dp).sum(), rel=1e-6)


def test_workspace_query():
    L = _lib.lib()
    assert L.g4d_refine_loss_ws_bytes(0, 64, 1) == 0 and L.g4d_refine_loss_ws_bytes(6, 0, 1) == 0
    assert L.g4d_refine_loss_ws_bytes(6, 64, 0) == 6 * 1 * 5 * 4
    assert L.g4d_refine_loss_ws_bytes(6, 257, 0) == 6 * 2 * 5 * 4
    assert L.g4d_refine_loss_ws_bytes(240, 4096, 0) == 240 * 16 * 5 * 4
    assert L.g4d_refine_loss_ws_bytes(240, 4096, 1) == 240 * 16 * 5 * 4 + 240 * 4096 * 3 * 4      # + the staged u


def _call(**kw):
    """g4d_refine_loss_f32 with fake non-null pointers (never dereferenced: every case below is refused before the device is touched)."""
    a = dict(nbatch=2, t=3, vg=64, v=700, pred=8, target=8, body=8, normals=8, nn_idx=8, idx_stride=3, rowptr=8, colidx=8, vals=8, rowsum=8,
             rowptr_t=8, colidx_t=8, vals_t=8, w_l2=20.0, w_lap=10.0, w_pen=100.0, w_tmp=5.0, temporal=1, ws=8, out=8, msre=0, grad=0)
    a.update(kw)
    return _lib.lib().g4d_refine_loss_f32(*a.values(), None)


@pytest.mark.parametrize("kw,text", [(dict(nbatch=-1), "bad sizes"), (dict(vg=-5), "bad sizes"), (dict(idx_stride=0), "bad sizes"), (dict(out=0), "out is null"),
                                     (dict(pred=0), "null pointer"), (dict(rowsum=0), "null pointer"), (dict(ws=0), "null pointer"),
                                     (dict(v=0), "no body vertices"), (dict(w_lap=float("nan")), "NaN"),
                                     (dict(grad=8, rowptr_t=0), "transposed operator"), (dict(nbatch=1 << 20, t=1 << 12), "too many frames")])
def test_einval_before_the_device_is_touched(kw, text):
    assert _call(**kw) == 10001
    assert text in _lib.lib().g4d_last_error().decode()


def test_signature_matches_the_header():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "g4d.h")).read()
    decl = hdr[hdr.index("int g4d_refine_loss_f32("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(_lib.SIGNATURES["g4d_refine_loss_f32"])
    assert _lib.RESTYPES["g4d_refine_loss_ws_bytes"] is ctypes.c_longlong


def test_opt_in_is_the_existing_switch():
    names = [f.name for f in dataclasses.fields(tuning.Tuning)]
    assert "refine_autograd" in names and tuning.Tuning().refine_autograd is False
    assert not [n for n in names if "stage2" in n or "loss" in n], "the stage-2 route adds no tuning field"
    assert tuning.current().replace(refine_autograd=True).refine_autograd is True


def test_model_class_asserts_stay():
    """Under grad: the switch off keeps the inference-only assert; the switch on demands an encoder entirely in eval().  Both fire before any
    kernel runs, so this needs no GPU."""
    from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSeg
    scene = syn.garment_scene(1, 2, 64, garment_rc=(8, 8), seed=3)
    m = PCALBSGarmentUseSegEncoderSeg(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"], lbs_k=3, iteration=3).eval()
    x = torch.from_numpy(scene["x"])
    body_model = types.SimpleNamespace(parents=None, faces=scene["body"]["faces"])
    with pytest.raises(AssertionError, match="inference only"):
        m(x, body_model, {})
    with tuning.use(tuning.current().replace(refine_autograd=True)):
        next(mod for mod in m.PCA_garment_encoder.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)).train()
        with pytest.raises(AssertionError, match="inference only"):
            m(x, body_model, {})
        m.eval()
        with pytest.raises(AssertionError, match="inference only"):       # forward_frames: unchanged, whatever the switch says
            m.forward_frames(x[0], body_model, {}, nbatch=1, T=2, frame_ids=[0, 1])


def test_refusals_need_no_device():
    from garment4d_amd.losses import stage2_loss, temporal_loss_PCA_LBS
    p = torch.zeros(2, 4, 3, requires_grad=True)
    z = torch.zeros(2, 4, 3)
    for bad in range(3):
        args = [z.clone().requires_grad_(True) if i == bad else z for i in range(3)]
        with pytest.raises(NotImplementedError, match="requires grad"):
            stage2_loss([p], *args, None, 1, 2, TW.LAMBDAS)
    inputs = dict(pose_torch=torch.zeros(1, 2, 72), smpl_vertices_torch=z.reshape(1, 2, 4, 3), smpl_root_joints_torch=torch.zeros(1, 2, 3),
                  garment_torch=z.reshape(1, 2, 4, 3).clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="garment_torch"):
        temporal_loss_PCA_LBS(dict(iter_regressed_lbs_garment_v=[p], lbs_pred_garment_v=z, lap_adj=None), inputs, None, None,
                              loss_cfg=dict(zip(("LBS_GARMENT_L2_LOSS_LAMBDA", "LBS_GARMENT_LAP_LOSS_LAMBDA", "LBS_INTERPENETRATION_LOSS_LAMBDA",
                                                 "TEMPORAL_CONSTRAINT_LOSS_LAMBDA"), TW.LAMBDAS)))

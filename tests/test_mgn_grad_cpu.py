"""The MGN training route without a GPU: the float64 twin (tests/mgn_grad_twin.py) against torch-float64 autograd of the reference-shaped
gather/matmul blend and against the reference's own run stored in tests/golden/mgn_grad.npz, the golden file's size and checksum, the argument
checks of g4d_mgn_skin_grad_f32 (they happen before the device is touched), and the opt-in's semantics (tuning.Tuning.mgn_autograd)."""
import os
import types

import numpy as np
import pytest
import torch

import mgn_grad_twin as MT
from garment4d_amd import _lib, synthetic as syn, tuning


@pytest.fixture(scope="module")
def golden():
    g = MT.load()
    case, targets, sd = MT.golden_inputs()
    assert np.array_equal(g["checksum"], syn.mgn_grad_checksum(case, targets)), "mgn_grad.npz belongs to other inputs: regenerate it"
    return g, case, targets, sd


@pytest.fixture(scope="module")
def twin_step(golden):
    _, case, targets, sd = golden
    return MT.train_step64(case, targets, sd)


def test_fixture_conditions(golden):
    g = golden[0]
    assert (g["decisions"] == 0).all()             # nearest indices, ReLU decisions, penetration signs: the same in both precisions of the reference
    assert 0.2 <= float(g["penetrating_share"]) <= 0.8
    assert (g["min_abs_preact"] > 0).all()


def test_golden_file_is_small():
    size = lambda n: os.path.getsize(os.path.join(MT.GOLDEN, n))
    assert size("mgn_grad.npz") <= size("gcn_grad.npz") and size("mgn_grad.npz") <= 1 << 20


@pytest.mark.parametrize("with_stage1", [False, True])
def test_adjoint_equals_autograd_of_the_reference_blend(with_stage1):
    """The twin's adjoint against torch-float64 autograd of the reference's formulation: all body vertices blended by a matmul, one row gathered."""
    rng = np.random.default_rng(3)
    clips, T, Vg, V, J = 2, 3, 37, 50, 24
    F_ = clips * T
    W = rng.random((F_, V, J)) ** 4
    W /= W.sum(-1, keepdims=True)
    inv_A, A = rng.standard_normal((2, F_, J, 4, 4))
    idx = rng.integers(0, V, (F_, Vg))
    g = torch.from_numpy(rng.standard_normal((F_, Vg, 3))).requires_grad_(True)
    dp, ds = rng.standard_normal((2, F_, Vg, 3))
    s, p = MT.reference_blend_torch(g, torch.from_numpy(rng.standard_normal((clips, 3))), torch.from_numpy(idx), torch.from_numpy(W), torch.from_numpy(inv_A),
                                    torch.from_numpy(A), T)
    loss = (p * torch.from_numpy(dp)).sum() + ((s * torch.from_numpy(ds)).sum() if with_stage1 else 0.0)
    loss.backward()
    mine, bound = MT.skin_adjoint64(idx, W, inv_A, A, dp, ds if with_stage1 else None)
    np.testing.assert_allclose(mine, g.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(g.grad.numpy()).max())
    assert (bound > 0).all() and (bound < 1e-4 * np.abs(mine).max()).all()
    s64, p64, terms = MT.skin64((g.detach() + 0).numpy(), idx, W, inv_A, A)        # root added by the caller: here the forward at root = 0
    assert (terms >= np.abs(p64)).all()


def test_twin_forward_equals_the_reference_blend():
    rng = np.random.default_rng(4)
    clips, T, Vg, V, J = 2, 2, 11, 20, 24
    F_ = clips * T
    W = rng.random((F_, V, J))
    inv_A, A = rng.standard_normal((2, F_, J, 4, 4))
    idx = rng.integers(0, V, (F_, Vg))
    g, root = rng.standard_normal((F_, Vg, 3)), rng.standard_normal((clips, 3))
    s, p = MT.reference_blend_torch(torch.from_numpy(g), torch.from_numpy(root), torch.from_numpy(idx), torch.from_numpy(W), torch.from_numpy(inv_A),
                                    torch.from_numpy(A), T)
    s64, p64, _ = MT.skin64(g + np.repeat(root, T, 0)[:, None, :], idx, W, inv_A, A)
    np.testing.assert_allclose(s64, s.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(p64, p.numpy(), rtol=1e-12, atol=1e-12)


def test_twin_reproduces_the_reference_within_its_fp32_error(golden, twin_step):
    """The project's rule: within three times the reference's own fp32 rounding error (eref) of the stored fp32 values, per stored array."""
    g, case, _, _ = golden
    r = twin_step
    for k, v in r["scalars"].items():
        assert abs(v - float(g[k])) <= 3 * float(g[f"eref_{k}"]) + 1e-12 * float(g[f"max64_{k}"]), (k, v, float(g[k]), float(g[f"eref_{k}"]))
    for k, a in MT.stored_arrays(r["grads"], r["d_lbs_pred"], g).items():
        err = np.abs(a - g[k].astype(np.float64)).max()
        assert err <= 3 * float(g[f"eref_{k}"]) + 1e-12 * float(g[f"max64_{k}"]), (k, err, float(g[f"eref_{k}"]))
        assert np.abs(a).max() == pytest.approx(float(g[f"max64_{k}"]), rel=1e-6)
    share = (r["dot"] < 0).mean()
    assert share == pytest.approx(float(g["penetrating_share"]), abs=1e-12)
    assert [float(np.abs(p).min()) for p in r["pre"][:2]] == pytest.approx(list(g["min_abs_preact"]), rel=1e-2)


def test_reference_computation_decreases_under_adam(golden):
    """Ten Adam steps at lr 1e-3 on the golden batch, in the float64 twin: the objective the GPU test minimises does go down on this batch."""
    _, case, targets, sd = golden
    params = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-3)
    losses = []
    for _ in range(11):
        r = MT.train_step64(case, targets, {k: p.detach().numpy() for k, p in params.items()})
        losses.append(r["scalars"]["total_loss"])
        for k, p in params.items():
            p.grad = torch.from_numpy(r["grads"][k].copy())
        opt.step()
    assert losses[10] < losses[0], losses


# ---------------------------------------------------------------- the C ABI: refused before the device is touched
def _call(**kw):
    """g4d_mgn_skin_grad_f32 with fake non-null pointers (never dereferenced: every case below is refused before the device is touched)."""
    a = dict(clips=2, t=3, vg=16, v=50, j=24, nn_idx=16, W=16, inv_A=16, A=16, d_posed=16, d_stage1=0, d_garment=16)
    a.update(kw)
    return _lib.lib().g4d_mgn_skin_grad_f32(*a.values(), None)


@pytest.mark.parametrize("kw,text", [(dict(clips=-1), "negative size"), (dict(vg=-3), "negative size"), (dict(j=0), "1 <= J <= 64"), (dict(j=65), "1 <= J <= 64"),
                                     (dict(v=0), "V = 0"), (dict(nn_idx=0), "null pointer"), (dict(W=0), "null pointer"), (dict(inv_A=0), "null pointer"),
                                     (dict(A=0), "null pointer"), (dict(d_posed=0), "null pointer"), (dict(d_garment=0), "null pointer"),
                                     (dict(A=20), "16-byte aligned"), (dict(inv_A=24), "16-byte aligned")])
def test_einval_before_the_device_is_touched(kw, text):
    assert _call(**kw) == 10001
    assert text in _lib.lib().g4d_last_error().decode()


@pytest.mark.parametrize("kw", [dict(clips=0), dict(t=0), dict(vg=0)])
def test_zero_sizes_return_ok_without_looking_at_the_pointers(kw):
    assert _call(nn_idx=0, W=0, inv_A=0, A=0, d_posed=0, d_garment=0, **kw) == 0


def test_signature_matches_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "g4d.h")).read()
    decl = hdr[hdr.index("int g4d_mgn_skin_grad_f32("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(_lib.SIGNATURES["g4d_mgn_skin_grad_f32"])


# ---------------------------------------------------------------- the opt-in
def test_switch_defaults_off_and_follows_the_environment(monkeypatch):
    assert tuning.Tuning().mgn_autograd is False
    monkeypatch.delenv("G4D_MGN_AUTOGRAD", raising=False)
    assert tuning.from_environment().mgn_autograd is False
    monkeypatch.setenv("G4D_MGN_AUTOGRAD", "1")
    assert tuning.from_environment().mgn_autograd is True
    with tuning.use(tuning.current().replace(mgn_autograd=True)):
        assert tuning.current().mgn_autograd is True
    assert tuning.current().mgn_autograd is tuning.DEFAULT.mgn_autograd


def _cpu_model():
    from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSegMGN
    scene = syn.garment_scene(1, 2, 64, garment_rc=(8, 8), seed=3)
    m = PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"]).eval()
    return m, torch.from_numpy(scene["x"]), types.SimpleNamespace(parents=None, faces=scene["body"]["faces"])


def test_model_asserts_and_refusals_need_no_device():
    """Under grad: the switch off keeps the inference-only assert; the switch on demands an encoder entirely in eval(), fp32, and whole clips.  All
    fire before any kernel runs."""
    m, x, body_model = _cpu_model()
    with pytest.raises(AssertionError, match="inference only"):
        m(x, body_model, {})
    with pytest.raises(AssertionError, match="inference only"):
        m.forward_frames(x[0], body_model, {}, nbatch=1, T=2, frame_ids=[0, 1])
    with tuning.use(tuning.current().replace(mgn_autograd=True)):
        with pytest.raises(NotImplementedError, match="bf16"):
            m(x, body_model, {}, precision="bf16")
        with pytest.raises(NotImplementedError, match="frame-sharded"):
            m.forward_frames(x[0], body_model, {}, nbatch=1, T=2, frame_ids=[0, 1])
        next(mod for mod in m.PCA_garment_encoder.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)).train()
        with pytest.raises(AssertionError, match="inference only"):
            m(x, body_model, {})


def test_skinning_refuses_other_grad_inputs():
    from garment4d_amd.garment_lbs import lbs_garment_MGN
    z = lambda *s: torch.zeros(*s)
    args = dict(pred_template_garment_v=z(1, 2, 4, 3), Tpose_vertices=z(1, 5, 3), Tpose_root_joints=z(1, 3), zeropose_vertices=z(1, 2, 5, 3), parents=None,
                gt_pose=z(1, 2, 72), T_J_regressor=z(1, 2, 24, 5), T_lbs_weights=z(1, 2, 5, 24))
    for name in ("Tpose_vertices", "Tpose_root_joints", "zeropose_vertices", "gt_pose", "T_J_regressor", "T_lbs_weights"):
        bad = dict(args)
        bad[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=name):
            lbs_garment_MGN(**bad)

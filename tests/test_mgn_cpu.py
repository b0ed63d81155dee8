"""The MGN model variant (`PCALBSGarmentUseSegEncoderSegMGN`, modules/mesh_encoder.py:489-614) without a GPU: construction from arrays,
the reference's state-dict names (tests/golden/mgn.npz holds the list the reference's own constructor produced) and the mesh adjacency."""
import os
import types

import numpy as np
import pytest
import torch

from garment4d_amd import synthetic as syn
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSegMGN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mgn.npz")


def _model(z):
    gv = z["in_template_verts"]
    pca = dict(components=np.zeros((72, gv.size), np.float32), mean=gv.reshape(-1), explained=np.ones(72), ss_scale=np.ones(gv.size))
    return PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=pca, template=(gv, z["in_template_faces"]))


def test_constructor_from_arrays():
    z = np.load(GOLDEN)
    m = _model(z)
    Vg = z["in_template_verts"].shape[0]
    assert m.PCA_garment_encoder.garment_v_num == Vg
    lin = [mod for mod in m.displacement_encoder if isinstance(mod, torch.nn.Linear)]
    assert [(l.in_features, l.out_features) for l in lin] == [(512, 1024), (1024, 2048), (2048, Vg * 3)]
    assert [type(mod).__name__ for mod in m.displacement_encoder] == ["Linear", "ReLU", "Linear", "ReLU", "Linear"]
    assert m.adj_old.shape == (Vg, Vg) and tuple(m.adj.shape) == (Vg, Vg)


def test_state_dict_keys_match_reference():
    z = np.load(GOLDEN)
    m = _model(z)
    assert list(m.state_dict().keys()) == z["state_dict_keys"].tolist()
    sd = syn.mgn_displacement_state_dict(z["in_template_verts"].shape[0], seed=int(z["seed"]) + 100)
    np.testing.assert_allclose(np.array([float(np.asarray(sd[k], np.float64).sum()) for k in sorted(sd)]), z["displacement_checksum"], rtol=1e-12)
    full = {k: v.clone() for k, v in m.state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in sd.items()})
    m.load_state_dict(full, strict=True)


def test_lap_adjacency_matches_reference():
    z = np.load(GOLDEN)
    m = _model(z)
    lap = m._lap_adj_on(torch.device("cpu")).coalesce()
    np.testing.assert_array_equal(lap.indices()[0].numpy(), z["lap_row"])
    np.testing.assert_array_equal(lap.indices()[1].numpy(), z["lap_col"])
    np.testing.assert_allclose(lap.values().numpy(), z["lap_val"], rtol=1e-6)


def test_lbs_garment_mgn_asserts_k1_like_the_reference():
    z = np.load(GOLDEN)
    m = _model(z)
    with pytest.raises(AssertionError):
        m.lbs_garment_MGN(torch.zeros(1, 2, 4, 3), None, None, None, types.SimpleNamespace(parents=None), torch.zeros(1, 2, 72), None, None, K=3)

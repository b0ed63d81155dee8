"""Shared by the tests of tests/golden/encoder.npz (test_encoder_golden_cpu.py, test_encoder_golden_gpu.py) and the drop-in tests: the
golden's inputs and seeded weights regenerated on this side, the comparison rules, and the reference's own encoder loop."""
import numpy as np

from conftest import load_golden
from garment4d_amd import synthetic as syn

TARGET = 6                 # label_dict["Tshirt"] - 1
TOL = 1e-5                 # rtol = atol


def golden():
    """(encoder.npz as a dict, the regenerated synthetic case); the inputs are checked against the stored checksums."""
    g = load_golden("encoder.npz")
    case = syn.encoder_golden_case(int(g["seed"]))
    assert np.array_equal(syn.encoder_golden_checksum(case), g["checksum"]), "synthetic.encoder_golden_case drifted from encoder.npz"
    return g, case


def seeded(shapes, keys, checksum, seed):
    """Seeded weights for a model with these {key: shape}; the key list and per-key checksums must be the generator's."""
    sd = syn.encoder_state_dict(shapes, seed=seed)
    assert sorted(sd) == [str(k) for k in keys], "state-dict keys differ from the reference model's"
    assert np.array_equal(syn.state_dict_checksum(sd), checksum), "synthetic.encoder_state_dict drifted from encoder.npz"
    return sd


def e1_state_dict(g, shapes):
    """PCAGarmentEncoderSeg's weights (keys relative to the encoder) with the generator's garment-bias shift applied."""
    sd = seeded(shapes, g["e1_sd_keys"], g["e1_sd_checksum"], int(g["e1_weight_seed"]))
    b = sd["pointnet.FC_layer.2.conv.bias"].copy()
    b[TARGET] = np.float32(b[TARGET] + g["e1_bias_shift"])     # the generator adds the shift to the float32 bias
    sd["pointnet.FC_layer.2.conv.bias"] = b
    return sd


def e2_state_dict(g, shapes, case):
    return seeded(shapes, g["e2_sd_keys"], g["e2_sd_checksum"], case["seed"] + 30)


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max()) if a.size else 0.0


def close(a, b, tol=TOL, what=""):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    e = err(a, b)
    assert e <= tol, f"{what}: max elementwise err {e:.3e} > {tol:.0e} (rtol = atol)"
    return e


def check_feats(g, tag, feats, tol=TOL):
    """Channel-major feature tensors (F, C, n_l) per level against the stored subsets and per-channel sums (the sum gate is the
    elementwise gate summed over the points).  Returns the largest elementwise error."""
    worst = 0.0
    for lvl, f in enumerate(feats):
        key = f"{tag}{lvl}"
        if key not in g:
            assert f is None, key
            continue
        f = np.asarray(f, np.float32)
        idx = g[key + "_idx"]
        sub = np.stack([f[i][:, idx[i]] for i in range(f.shape[0])])
        worst = max(worst, close(sub, g[key], tol, key))
        s = f.astype(np.float64).sum(2)
        bound = tol * (f.shape[2] + np.abs(f.astype(np.float64)).sum(2))
        assert (np.abs(s - g[key + "_chsum"]) <= bound).all(), f"{key}: per-channel sums over the points differ"
    return worst


def check_logits(g, tag, logits, tol=TOL):
    logits = np.asarray(logits)
    idx = g[tag + "_idx"]
    return close(np.stack([logits[i][idx[i]] for i in range(logits.shape[0])]), g[tag], tol, tag)


def reference_encoder_loop(model, pc):
    """The forward of modules/pointnet2encoder.py:112-145, statement for statement, over whatever modules `model` holds -- this is what
    the reference's file runs when it imports this package's pointnet2_modules / pytorch_utils in place of its own."""
    xyz = pc[..., 0:3].contiguous()
    features = pc[..., 3:].transpose(1, 2).contiguous() if pc.size(-1) > 3 else None
    l_xyz, l_features = [xyz], [features]
    for i in range(len(model.SA_modules)):
        li_xyz, li_features = model.SA_modules[i](l_xyz[i], l_features[i])
        l_xyz.append(li_xyz)
        l_features.append(li_features)
    middle = model.Middle_modules(l_xyz[-1], l_features[-1])[1] if model.global_feat else None
    for i in range(-1, -(len(model.FP_modules) + 1), -1):
        l_features[i - 1] = model.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])
    sem_logits = model.FC_layer(l_features[0]).transpose(1, 2).contiguous()
    return middle, sem_logits, l_features, l_xyz

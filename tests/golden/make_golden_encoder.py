#!/usr/bin/env python
"""Generate tests/golden/encoder.npz by running the REFERENCE's own encoders on CPU: `PCAGarmentEncoderSeg.forward`
(modules/mesh_encoder.py:43-169) and `Pointnet2MSGSEG(input_channels=3, global_feat=True).forward` (modules/pointnet2encoder.py).

Run from the repo root:  G4D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_encoder.py
(its own process, like make_golden_refine.py, whose loader it uses: the C oracle as `pointnet2_cuda`, `.cuda()` = identity,
`utils.config` / `utils.dataloader` stubbed).  Needs no GPU.  Only DATA is written: the reference's outputs, the search results
below, per-key checksums of the seeded weights and of the inputs -- the weights and inputs themselves are regenerated from seeds by
garment4d_amd/synthetic.py (encoder_state_dict, encoder_golden_case).

E1  PCAGarmentEncoderSeg(cfg, args) built by the reference's own __init__ from a PCA pickle and a template OBJ written to a temporary
    directory; Tshirt, nbatch = 2, T = 2, N = 6890 (mesh_encoder.py:111 hard-codes 6890).  The garment class's head bias is shifted
    by a searched amount so that the four frames' garment-point counts cover: more than n = N // 4 (truncation to the first n points),
    between 1 and n - 1 (zero-padded rows) and none at all.  Every point's garment-vs-best-other logit margin is >= 1e-4.  The template is
    all quads: the reference's `np.array(list(F))` (mesh_encoder.py:97) rejects a ragged quad + triangle face list under numpy >= 1.24.
    Also run with args.only_seg = True.
E2  Pointnet2MSGSEG(input_channels=3, global_feat=True) called as model(pc), eval mode, B = 2, N = 2048.
E3  E2's model in BatchNorm-recalibration mode: model.eval(), then .train() on every BatchNorm submodule, under no_grad (Dropout stays
    in eval); the outputs of one call and every BatchNorm's running_mean / running_var after it.

Wide per-point tensors (feature_list, garment_f_list, l_features) are stored at a fixed point subset per frame and level (the first 4,
the last 4 and 8 seeded random points) plus their per-channel sums over all points; sem_logits at the first 32, the last 32 and 192
seeded random points; everything else in full.
"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_refine as MR  # noqa: E402  (exits unless G4D_REFERENCE_DIR is set; puts the repository root on sys.path)

from garment4d_amd import synthetic as syn  # noqa: E402
from oracle import pointnet2_oracle as K  # noqa: E402

T, N = MR.T, MR.N
GARMENT = "Tshirt"
TARGET = 6                     # label_dict["Tshirt"] - 1
MIN_MARGIN = 1e-4              # ten times the 1e-5 gate: no rounding difference can move a point across the garment decision
SEARCH_SEEDS = range(200, 240)


def subset(n, seed, first, rand):
    """Sorted point indices: the first `first`, the last `first` and `rand` seeded random others (all points when n is small)."""
    if n <= 2 * first + rand:
        return np.arange(n, dtype=np.int64)
    mid = np.random.default_rng(seed).choice(np.arange(first, n - first), rand, replace=False)
    return np.sort(np.concatenate([np.arange(first), mid, np.arange(n - first, n)])).astype(np.int64)


def feat_subsets(n, seed, frames):
    return np.stack([subset(n, seed + 1000 * f, 4, 8) for f in range(frames)])


def logit_subsets(n, seed, frames):
    return np.stack([subset(n, seed + 1000 * f, 32, 192) for f in range(frames)])


def take_cm(a, idx):
    """a (F, C, n) channel-major, idx (F, k) -> (F, C, k)."""
    return np.stack([a[f][:, idx[f]] for f in range(a.shape[0])]).astype(np.float32)


def store_feats(out, tag, feats, seed):
    """feature tensors (F, C, n_l) per level: subset + per-channel sums over the points."""
    for lvl, f in enumerate(feats):
        if f is None:
            continue
        f = N(f)
        idx = feat_subsets(f.shape[2], seed + 17 * lvl, f.shape[0])
        out[f"{tag}{lvl}_idx"] = idx
        out[f"{tag}{lvl}"] = take_cm(f, idx)
        out[f"{tag}{lvl}_chsum"] = f.astype(np.float64).sum(2).astype(np.float32)


def store_logits(out, tag, logits, seed):
    """sem_logits (F, n, classes) at the logit subset."""
    L = N(logits)
    idx = logit_subsets(L.shape[1], seed, L.shape[0])
    out[tag + "_idx"] = idx
    out[tag] = np.stack([L[f][idx[f]] for f in range(L.shape[0])]).astype(np.float32)


def margins(logits, shift):
    L = logits.astype(np.float64)
    return L[..., TARGET] + shift - np.delete(L, TARGET, axis=2).max(2)


def covers(c, n, npts):
    return bool(((c > n) & (c < npts)).any() and ((c >= 1) & (c < n)).any() and (c == 0).any())


def search_shift(logits, n):
    """Smallest-magnitude shift of the garment logit (grid of 1e-4) whose frame counts hit all three categories (> n with garment and
    other points interleaved, 1..n-1, 0) and leave every point at least MIN_MARGIN from the decision; None if there is none."""
    base = margins(logits, 0.0)
    for step in sorted(range(-6000, 6001), key=abs):
        s = step * 1e-4
        m = base + s
        if np.abs(m).min() < 2 * MIN_MARGIN:
            continue
        c = (m > 0).sum(1)
        if covers(c, n, logits.shape[1]):
            return np.float32(s)
    return None


def reference_encoder(me, case, d, only_seg):
    gv, gq = case["template"]
    with open(os.path.join(d, "pca.pkl"), "wb") as fd:
        pickle.dump(case["pca"], fd)
    with open(os.path.join(d, "t.obj"), "w") as fd:
        fd.writelines("v %r %r %r\n" % tuple(float(c) for c in v) for v in gv)
        fd.writelines("f " + " ".join(str(int(i) + 1) for i in f) + "\n" for f in gq)
    cfg = types.SimpleNamespace(GARMENT=types.SimpleNamespace(NAME=GARMENT, PCADIM=64, PCACOMPONENTSFILE=os.path.join(d, "pca.pkl"),
                                                              TEMPLATE=os.path.join(d, "t.obj")))
    return me.PCAGarmentEncoderSeg(cfg, types.SimpleNamespace(only_seg=only_seg))


def load_seeded(model, seed, shift=None):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = syn.encoder_state_dict(shapes, seed=seed)
    model.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    if shift is not None:
        model.pointnet.FC_layer[2].conv.bias.data[TARGET] += torch.tensor(shift)
    return sd


def gen_e1(me, case, out):
    x = T(case["x"])
    nbatch, Tn, Np = case["nbatch"], case["T"], case["N"]
    n = Np // 4
    body_model = object()
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        model = reference_encoder(me, case, d, only_seg=False).eval()
        seg = reference_encoder(me, case, d, only_seg=True).eval()
    for wseed in SEARCH_SEEDS:              # deterministic search: the first weight seed whose logits admit a shift
        load_seeded(model, wseed)
        with torch.no_grad():
            logits = N(model.pointnet(x.reshape(nbatch * Tn, Np, 3))[1])
        shift = search_shift(logits, n)
        if shift is not None:
            break
    else:
        sys.exit("no weight seed in SEARCH_SEEDS reaches all garment-count categories")
    sd = load_seeded(model, wseed, shift)
    seg.load_state_dict({k: v for k, v in model.state_dict().items() if k.startswith("pointnet.")}, strict=True)
    with torch.no_grad():
        od = model(x, body_model)
        od_seg = seg(x, body_model)
    L = N(od["sem_logits"])
    m = margins(L, 0.0)
    assert np.abs(m).min() >= MIN_MARGIN, f"a point's garment margin is {np.abs(m).min():.3g} < {MIN_MARGIN}"
    labels = np.argmax(L, 2)
    counts = (labels == TARGET).sum(1)
    assert covers(counts, n, Np), counts
    assert set(od_seg) == {"middle_results", "feat_global", "feature_list", "xyz_list", "sem_logits"} and od_seg["feat_global"] is None
    out.update(e1_weight_seed=np.int64(wseed), e1_bias_shift=shift, e1_sd_keys=np.array(sorted(sd)), e1_sd_checksum=syn.state_dict_checksum(sd),
               e1_labels=labels.astype(np.int8), e1_counts=counts.astype(np.int64), e1_n=np.int64(n), e1_min_margin=np.float64(np.abs(m).min()))
    for lvl, t in enumerate(od["xyz_list"][1:], 1):
        out[f"e1_xyz{lvl}"] = N(t)
    for lvl, t in enumerate(od["garment_v_list"]):
        out[f"e1_garment_v{lvl}"] = N(t)
    out["e1_garment_summary"] = N(od["garment_summary"])
    out["e1_garment_PCA_coeff"] = N(od["garment_PCA_coeff"])
    out["e1_tpose_garment"] = N(od["tpose_garment"])
    out["e1_garment_f_3"] = np.asarray(od["garment_f_3"], np.int32)
    store_logits(out, "e1_sem_logits", od["sem_logits"], 301)
    store_logits(out, "e1_seg_sem_logits", od_seg["sem_logits"], 301)
    store_feats(out, "e1_feature", od["feature_list"], 311)
    store_feats(out, "e1_garment_f", od["garment_f_list"], 331)
    print("E1: weight seed", wseed, "bias shift", float(shift), "counts", counts.tolist(), "n", n, "min margin", float(np.abs(m).min()))


def gen_e23(me, case, out):
    import importlib
    pe = importlib.import_module("modules.pointnet2encoder")
    model = pe.Pointnet2MSGSEG(input_channels=3, bn=True, global_feat=True)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = syn.encoder_state_dict(shapes, seed=case["seed"] + 30)
    model.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    out.update(e2_sd_keys=np.array(sorted(sd)), e2_sd_checksum=syn.state_dict_checksum(sd))
    pc = T(case["pc"])
    for tag in ("e2", "e3"):
        model.eval()
        if tag == "e3":
            for mod in model.modules():
                if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                    mod.train()
        with torch.no_grad():
            mid, logits, l_f, l_xyz = model(pc)
        out[tag + "_feat_global"] = N(mid)
        for lvl, t in enumerate(l_xyz[1:], 1):
            out[f"{tag}_xyz{lvl}"] = N(t)
        store_logits(out, tag + "_sem_logits", logits, 401)
        store_feats(out, tag + "_feature", l_f, 411)
    after = {k: N(v) for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    out["e3_bn_keys"] = np.array(sorted(after))
    for i, k in enumerate(sorted(after)):
        out[f"e3_bn{i}"] = after[k]
    print("E3:", len(after), "running-stat buffers")


def main():
    torch.set_num_threads(1)
    K.set_contraction("nvcc")
    me = MR.load_reference()
    case = syn.encoder_golden_case()
    out = dict(seed=np.int64(case["seed"]), checksum=syn.encoder_golden_checksum(case))
    gen_e1(me, case, out)
    gen_e23(me, case, out)
    path = os.path.join(MR.OUT, "encoder.npz")
    np.savez_compressed(path, **out)
    print("encoder.npz", len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

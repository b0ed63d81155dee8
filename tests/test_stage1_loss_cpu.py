"""The stage-1 objective without a GPU: the float64 twin (tests/stage1_loss_twin.py) against the reference's own run stored in
tests/golden/stage1_loss.npz, the conditions every GPU case must meet (flagged share, penetrating share), the argument checks of the new entry
points (they happen before the device is touched), the workspace query's closed form, header / ctypes agreement, and the opt-in's semantics."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import stage1_loss_twin as TW
from garment4d_amd import _lib, losses, synthetic as syn, tuning


@pytest.fixture(scope="module")
def golden():
    g, case = TW.load(), syn.stage1_loss_case()
    assert np.array_equal(g["checksum"], syn.stage1_loss_checksum(case)), "stage1_loss.npz belongs to other inputs: regenerate it"
    return g, case


def test_fixture_conditions(golden):
    g, case = golden
    assert (g["decisions"] == 0).all()                                        # the reference alone takes the same decisions in both precisions
    assert ((g["penetrating_share"] >= 0.2) & (g["penetrating_share"] <= 0.8)).all()
    assert case["pad_batch"] > case["nbatch"]                                 # the padding is exercised
    assert set(np.unique(case["inputs"]["pcd_label_torch"])) == set(range(case["C"]))
    assert list(g["os_keys"]) == ["sem_seg_loss", "total_loss"]


def test_twin_reproduces_the_reference_float64(golden):
    g, case = golden
    r = TW.evaluate(**TW.golden_inputs(case))
    ce = TW.cross_entropy(case["output"]["sem_logits"].reshape(-1, case["C"]), case["inputs"]["pcd_label_torch"].reshape(-1), TW.LAMBDAS[0])
    v = r["values"]
    twin = {"sem_seg_loss": ce["value"], "garment_pca_coeff_l2": v["pca"], "garment_l2_loss": v["l2"], "garment_msre": v["msre"],
            "interpenetration_loss": v["pen"], "garment_lap_loss": v["lap"], "total_loss": TW.total(ce["value"], v, TW.LAMBDAS)}
    assert set(twin) == set(TW.KEYS)
    for k, x in twin.items():
        ref = float(g[f"f64_{k}"])
        assert abs(x - ref) <= 1e-11 * max(abs(ref), 1e-3), (k, x, ref)
    assert abs(TW.LAMBDAS[0] * ce["value"] - float(g["f64_os_total_loss"])) <= 1e-11 and abs(ce["value"] - float(g["f64_os_sem_seg_loss"])) <= 1e-11
    (gp, _), (gc, _) = TW.gradient(r, TW.LAMBDAS[1:])
    for name, mine in (("pred", gp), ("coeff", gc), ("logits", ce["grad"].reshape(g["f64_grad_logits"].shape))):
        ref = g[f"f64_grad_{name}"]
        assert np.abs(mine - ref).max() <= 1e-11 * max(float(np.abs(ref).max()), 1e-3), name
    assert np.abs(ce["grad"].reshape(g["f64_os_grad_logits"].shape) - g["f64_os_grad_logits"]).max() <= 1e-14
    assert TW.flags(r).mean() <= 0.01
    assert 0.2 <= (r["dot"] < 0).mean() <= 0.8


@pytest.mark.parametrize("rows,cols,B,Bp", TW.GPU_CASES)
def test_gpu_cases_meet_their_conditions(rows, cols, B, Bp):
    c = TW.garment_case(TW.case_seed(rows, cols, B, Bp), B, rows, cols)
    r = TW.evaluate(c["p"], c["g"], c["root"], c["body"], c["normals"], c["faces"], c["coeff"], c["coeff_gt"], Bp)
    assert TW.flags(r).mean() <= 0.01
    assert 0.2 <= (r["dot"] < 0).mean() <= 0.8
    assert (r["lap_n"] > 0).all() and np.isfinite(TW.gradient(r, TW.LAMBDAS[1:])[0][1]).all()


def test_padding_is_a_weight_on_item_zero():
    """The twin itself: (B = 2, Bp = 4) against the explicitly concatenated batch [p0, p1, p0, p0] with Bp = B = 4."""
    c = TW.garment_case(11, 2, 8, 8)
    cat = lambda a: np.concatenate([a, a[:1], a[:1]], 0)
    r = TW.evaluate(c["p"], c["g"], c["root"], c["body"], c["normals"], c["faces"], c["coeff"], c["coeff_gt"], 4)
    r4 = TW.evaluate(*[cat(c[k]) for k in ("p", "g", "root", "body", "normals")], c["faces"], cat(c["coeff"]), cat(c["coeff_gt"]), 4)
    assert r["values"]["lap"] == pytest.approx(r4["values"]["lap"], rel=1e-12)
    w = (0.0, 0.0, 0.0, 1.0)
    g, g4 = TW.gradient(r, w)[0][0], TW.gradient(r4, w)[0][0]
    np.testing.assert_allclose(g[0], g4[0] + g4[2] + g4[3], rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(g[1], g4[1], rtol=1e-12, atol=1e-18)


def test_workspace_query():
    L = _lib.lib()
    q = L.g4d_stage1_loss_ws_bytes
    assert q(0, 0, 64, 112, 1) == 0 and q(0, 2, 0, 112, 1) == 0
    assert q(1, 0, 0, 0, 0) == 4 and q(256, 0, 0, 0, 0) == 4 and q(257, 0, 0, 0, 1) == 8
    assert q(8 * 30 * 8192, 0, 0, 0, 0) == 7680 * 4
    assert q((1 << 33) + 1, 0, 0, 0, 0) == ((1 << 25) + 1) * 4
    assert q(0, 2, 64, 112, 0) == (2 * 1 * 4 + 2 * 2 * 112 * 3) * 4
    assert q(0, 2, 257, 500, 0) == (2 * 2 * 4 + 2 * 2 * 500 * 3) * 4
    assert q(0, 8, 4096, 8064, 1) == (8 * 16 * 4 + 2 * 8 * 8064 * 3 + 8 * 4096 * 3) * 4       # + the staged u
    assert q(1536, 2, 64, 112, 1) == q(1536, 0, 0, 0, 0) + q(0, 2, 64, 112, 1)


def _ce(**kw):
    a = dict(rows=1536, classes=7, logits=8, labels=8, w=0.05, ws=8, out=8, grad=0)
    a.update(kw)
    return _lib.lib().g4d_stage1_ce_f32(*a.values(), None)


def _garment(**kw):
    """g4d_stage1_garment_f32 with fake non-null pointers (never dereferenced: every case below is refused before the device is touched)."""
    a = dict(b=2, bp=4, vg=64, v=700, nf=112, pdim=64, pred=8, target=8, root=8, body=8, normals=8, nn_idx=8, idx_stride=3, faces=8, inc_rowptr=8, inc=8,
             coeff=8, coeff_gt=8, w_pca=0.001, w_l2=40.0, w_pen=50.0, w_lap=1.0, ws=8, out=8, grad_pred=0, grad_coeff=0)
    a.update(kw)
    return _lib.lib().g4d_stage1_garment_f32(*a.values(), None)


@pytest.mark.parametrize("fn,kw,text", [
    (_ce, dict(rows=-1), "bad sizes"), (_ce, dict(classes=0), "bad sizes"), (_ce, dict(classes=65), "bad sizes"), (_ce, dict(out=0), "out is null"),
    (_ce, dict(logits=0), "null pointer"), (_ce, dict(labels=0), "null pointer"), (_ce, dict(ws=0), "null pointer"), (_ce, dict(w=float("nan")), "NaN"),
    (_ce, dict(rows=1 << 40), "too large"),
    (_garment, dict(b=-1), "bad sizes"), (_garment, dict(bp=1), "bad sizes"), (_garment, dict(vg=-5), "bad sizes"), (_garment, dict(idx_stride=0), "bad sizes"),
    (_garment, dict(nf=-1), "bad sizes"), (_garment, dict(out=0), "out is null"), (_garment, dict(pred=0), "null pointer"), (_garment, dict(root=0), "null pointer"),
    (_garment, dict(ws=0), "null pointer"), (_garment, dict(v=0), "no body vertices"), (_garment, dict(w_lap=float("nan")), "NaN"),
    (_garment, dict(faces=0), "faces without"), (_garment, dict(coeff_gt=0), "PCA coefficients without"),
    (_garment, dict(b=1 << 30, bp=1 << 30, vg=1 << 20), "too large")])
def test_einval_before_the_device_is_touched(fn, kw, text):
    assert fn(**kw) == 10001
    assert text in _lib.lib().g4d_last_error().decode()


def test_signatures_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "g4d.h")).read()
    for name, ret in (("g4d_stage1_ce_f32", "int"), ("g4d_stage1_garment_f32", "int"), ("g4d_stage1_loss_ws_bytes", "long long")):
        decl = hdr[hdr.index(f"{ret} {name}("):]
        decl = decl[:decl.index(";")]
        args = [a.strip() for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
        sig = _lib.SIGNATURES[name]
        assert len(args) == len(sig), name
        for a, t in zip(args, sig):
            want = ctypes.c_void_p if ("*" in a or a.startswith("g4d_stream_t")) else {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}[a.rsplit(" ", 1)[0]]
            assert t is want, (name, a)
    assert _lib.RESTYPES["g4d_stage1_loss_ws_bytes"] is ctypes.c_longlong


def test_opt_in_switch(monkeypatch):
    assert tuning.Tuning().stage1_autograd is False
    monkeypatch.delenv("G4D_STAGE1_AUTOGRAD", raising=False)
    assert tuning.from_environment().stage1_autograd is False
    monkeypatch.setenv("G4D_STAGE1_AUTOGRAD", "1")
    assert tuning.from_environment().stage1_autograd is True


def test_refusals_need_no_device():
    z = torch.zeros(2, 4, 3)
    lg, lb, a = torch.zeros(2, 5, 7, requires_grad=True), torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 3)
    names = ("coeff_gt", "garment_gt", "root", "body_v", "body_vn")
    for bad, name in enumerate(names):
        consts = [a, z, torch.zeros(2, 3), z, z]
        consts[bad] = consts[bad].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=f"{name} requires grad"):
            losses.stage1_loss(lg, lb, a, consts[0], z, *consts[1:], np.zeros((1, 3), np.int32), 2, TW.LAMBDAS)
    inputs = dict(pose_torch=torch.zeros(2, 1, 72), pcd_label_torch=lb, PCACoeff=a, garment_template_vertices=z.clone().requires_grad_(True),
                  Tpose_smpl_vertices_torch=z, Tpose_smpl_root_joints_torch=torch.zeros(2, 1, 3))
    with pytest.raises(NotImplementedError, match="garment_template_vertices"):
        losses.temporal_loss_PCA(dict(sem_logits=lg, garment_PCA_coeff=a, tpose_garment=z, garment_f_3=np.zeros((1, 3), np.int32)), inputs, None,
                                 types.SimpleNamespace(only_seg=False, batch_size=2), loss_cfg=dict(zip(losses.STAGE1_LAMBDAS, TW.LAMBDAS)))


def test_incidence_lists_every_corner_once():
    c = TW.garment_case(3, 1, 13, 15)
    faces, rowptr, inc = (t.numpy() for t in losses.face_incidence(c["faces"], c["Vg"], "cpu"))
    assert rowptr[0] == 0 and rowptr[-1] == faces.size == inc.size and sorted(inc) == list(range(faces.size))
    for i in (0, 7, c["Vg"] - 1):
        ent = inc[rowptr[i]:rowptr[i + 1]]
        assert (faces.reshape(-1)[ent] == i).all() and (np.diff(ent) > 0).all()


def test_vertex_corner_table_orders_faces_per_vertex_and_keeps_an_isolated_vertex():
    """mesh_tables.vertex_corners serves the incidence above and postprocess.mesh_topology's vertex -> face CSR: its entries // 3 are the
    faces of each vertex ascending (the lexsort by (vertex, face) the normals' summation order is defined by); a vertex no face names has
    an empty row."""
    from garment4d_amd import mesh_tables
    c = TW.garment_case(3, 1, 13, 15)
    f = np.asarray(c["faces"]).reshape(-1, 3).astype(np.int64)
    nv = c["Vg"] + 1                                     # one vertex more than the faces name
    rowptr, corners = mesh_tables.vertex_corners(f, nv)
    vid, fid = f.reshape(-1), np.repeat(np.arange(len(f)), 3)
    by_vertex = np.lexsort((fid, vid))
    assert np.array_equal(corners // 3, fid[by_vertex]) and np.array_equal(vid[corners], vid[by_vertex])
    assert np.array_equal(rowptr[1:], np.cumsum(np.bincount(vid, minlength=nv))) and rowptr[0] == 0 and rowptr[-1] == rowptr[-2] == f.size

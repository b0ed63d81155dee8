"""The adjoint of lbs() without a GPU: the fifth (header, library) pair -- include/g4d_smpl.h against its record tests/smpl_abi_snapshot.txt,
libg4d_smpl.so's exports, argument checks, empty problems and the size queries --, the opt-in's default, and the numpy twin
(tests/smpl_grad_twin.py) that the GPU tests compare the kernels with: its float64 adjoint equals central differences of its own forward and
reproduces the float64 gradients the reference's autograd gave (tests/golden/smpl_grad.npz)."""
import os
import re

import numpy as np
import pytest

import smpl_grad_twin as ST
from conftest import ROOT, load_golden
from test_abi_cpu import _LETTERS

EINVAL = 10001
HEADER = os.path.join(ROOT, "include", "g4d_smpl.h")
GRAD = "g4d_smpl_lbs_grad_f32"


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


def test_parsed_smpl_header_equals_its_snapshot():
    """include/g4d_smpl.h as _lib.parse_header reads it == tests/smpl_abi_snapshot.txt, both ways and in the header's order, constants included."""
    from garment4d_amd import _lib
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "smpl_abi_snapshot.txt")).read().splitlines()]
    recorded = dict(ln for ln in lines if ln[0].startswith("g4d_"))
    rec_consts = {ln[0]: int(ln[1]) for ln in lines if ln[0].startswith("G4D_")}
    assert all(len(ln) == 2 for ln in lines) and fields == []
    assert set(parsed) == set(_declared()) and len(parsed) == 4
    assert {n: (parsed.get(n), recorded.get(n)) for n in set(parsed) | set(recorded) if parsed.get(n) != recorded.get(n)} == {}
    assert list(parsed) == list(recorded)
    assert consts == rec_consts
    assert all(n.startswith("g4d_smpl_") for n in parsed) and all(k.startswith("G4D_SMPL_") for k in consts)
    assert consts["G4D_SMPL_SLAB_VERTS"] % 32 == 0


def test_smpl_library_exports_every_declared_symbol_and_leaves_the_other_four_pairs_alone():
    from garment4d_amd import _lib
    assert os.path.exists(_lib.SMPL_LIB_PATH), "run __graft_entry__.build() first"
    L, protos, consts = _lib.smpl_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
    others = (_lib.PROTOTYPES, _lib.render_lib()[1], _lib.scan_lib()[1], _lib.fit_lib()[1])
    assert not any(n.startswith("g4d_smpl") for protos_ in others for n in protos_)
    assert len(_lib.render_lib()[1]) == 4 and len(_lib.scan_lib()[1]) == 3 and len(_lib.fit_lib()[1]) == 4
    assert not any(k.startswith("G4D_SMPL") for lib_ in (_lib.render_lib(), _lib.scan_lib(), _lib.fit_lib()) for k in lib_[2])
    assert not any(k.startswith("G4D_SMPL") for k in _lib.CONSTANTS)
    for other in (_lib.lib(), _lib.render_lib()[0], _lib.scan_lib()[0], _lib.fit_lib()[0]):
        assert not hasattr(other, GRAD)
    assert _lib.lib().g4d_version() == 263
    assert _lib.smpl_lib()[0] is L                                           # loaded once
    assert _lib._entry(GRAD) is getattr(L, GRAD) and _lib._entry("g4d_fit_group_f32") is getattr(_lib.fit_lib()[0], "g4d_fit_group_f32")


def _args(b=2, v=40, j=24, nb=10, pose2rot=1, betas=1, bstride=None, pose=1, v_template=1, blend_dirs=1, Jt=1, Js=1, parents=1, weights=1, d_verts=1, d_joints=1,
          d_pose=1, d_betas=1, ws=16, ws_bytes=1 << 40):
    return (b, v, j, nb, pose2rot, betas, nb if bstride is None else bstride, pose, v_template, blend_dirs, Jt, Js, parents, weights, d_verts, d_joints, d_pose,
            d_betas, ws, ws_bytes, 0)


def test_smpl_grad_argument_validation_needs_no_gpu():
    """Every check of include/g4d_smpl.h comes before any launch: G4D_EINVAL with the entry point's name in the ONE error state."""
    from garment4d_amd import _lib
    L, _, _ = _lib.smpl_lib()
    main = _lib.lib()
    bad = [(dict(b=-1), "negative"), (dict(v=-1), "negative"), (dict(j=0), "J <= 32"), (dict(j=33), "J <= 32"), (dict(j=-4), "J <= 32"), (dict(nb=-1), "J <= 32"),
           (dict(j=24, nb=18), "<= 224"), (dict(j=2, nb=216), "<= 224"), (dict(j=1, nb=1 << 30), "<= 224"), (dict(bstride=3), "betas_bstride"), (dict(bstride=-10), "betas_bstride"),
           (dict(ws_bytes=64), "workspace"), (dict(ws=8), "workspace"), (dict(ws_bytes=-1), "workspace")]
    bad += [({k: 0}, "null") for k in ("betas", "pose", "v_template", "blend_dirs", "Jt", "Js", "parents", "weights", "d_pose", "d_betas", "ws")]
    for kw, needle in bad:
        rc = L.g4d_smpl_lbs_grad_f32(*_args(**kw))
        assert rc == EINVAL, (kw, rc)
        msg = main.g4d_last_error().decode()                                 # libg4d_hip.so's accessor: one error state for the five libraries
        assert GRAD in msg and needle in msg, (kw, msg)
        with pytest.raises(_lib.G4DError, match=GRAD):
            _lib.call(GRAD, *_args(**kw))
    # the domain is checked on an empty problem too, and before the pointers
    assert L.g4d_smpl_lbs_grad_f32(*_args(b=0, j=33)) == EINVAL and L.g4d_smpl_lbs_grad_f32(*_args(j=33, betas=0)) == EINVAL
    assert "J <= 32" in main.g4d_last_error().decode()


def test_empty_smpl_grad_problems_return_zero():
    """b == 0 or v == 0: nothing is read and nothing launched; with no output given there is nothing to zero either."""
    from garment4d_amd import _lib
    L, _, _ = _lib.smpl_lib()
    none = dict(betas=0, pose=0, v_template=0, blend_dirs=0, Jt=0, Js=0, parents=0, weights=0, d_verts=0, d_joints=0, d_pose=0, d_betas=0, ws=0, ws_bytes=0)
    for kw in (dict(b=0), dict(v=0), dict(b=0, v=0), dict(b=0, bstride=0), dict(b=0, pose2rot=0)):
        assert L.g4d_smpl_lbs_grad_f32(*_args(**{**none, **kw})) == 0, kw
    assert _lib.call(GRAD, *_args(**{**none, "b": 0})) == 0


def test_slabs_and_workspace_are_functions_of_the_shape_alone():
    from garment4d_amd import _lib
    L, _, consts = _lib.smpl_lib()
    S = consts["G4D_SMPL_SLAB_VERTS"]
    assert (S, consts["G4D_SMPL_MAX_JOINTS"], consts["G4D_SMPL_MAX_COEFFS"]) == (128, 32, 224)
    for b, v, want in ((1, 1, 1), (240, S, 1), (240, S + 1, 2), (1, 6890, 54), (17, 6890, 54), (0, 6890, 0), (5, 0, 0), (-1, 5, -1), (5, -1, -1)):
        assert L.g4d_smpl_grad_slabs(b, v) == want, (b, v)
    assert [L.g4d_smpl_grad_supported(j, nb) for j, nb in ((24, 10), (24, 17), (24, 18), (32, 0), (33, 0), (0, 1), (1, 224), (1, 225), (5, -1))] == [1, 1, 0, 0, 0, 0, 1, 0, 0]
    for b, v, j, nb in ((1, 1, 24, 10), (17, 500, 5, 1), (240, 6890, 24, 10), (33, 129, 25, 4)):
        n = L.g4d_smpl_grad_ws_bytes(b, v, j, nb)
        js, ntile, nc = (6 if j <= 24 else 8), (b + 15) // 16, nb + 9 * (j - 1)
        up4 = lambda x: (x + 3) // 4 * 4
        assert n == 4 * (ntile * 14 * 256 + ntile * 3 * js * 256 + up4(L.g4d_smpl_grad_slabs(b, v) * b * (12 * j + nc)) + up4(b * (12 * j + nc)) + up4(b * nb)), (b, v, j, nb)
        assert n == L.g4d_smpl_grad_ws_bytes(b, v, j, nb) and n % 16 == 0
    assert L.g4d_smpl_grad_ws_bytes(240, 6890, 24, 10) == 27_165_120                  # cfg4: 54 slabs of 240 x 505 floats, their sum, the operands
    assert L.g4d_smpl_grad_ws_bytes(0, 0, 24, 10) == 0
    assert [L.g4d_smpl_grad_ws_bytes(*a) for a in ((-1, 5, 24, 10), (5, -1, 24, 10), (5, 5, 33, 0), (5, 5, 24, 18))] == [-1] * 4


def test_lbs_autograd_defaults_to_off(monkeypatch):
    from garment4d_amd import tuning
    assert tuning.Tuning().lbs_autograd is False
    monkeypatch.delenv("G4D_LBS_AUTOGRAD", raising=False)
    assert tuning.from_environment().lbs_autograd is False
    monkeypatch.setenv("G4D_LBS_AUTOGRAD", "1")
    assert tuning.from_environment().lbs_autograd is True
    with tuning.use(tuning.current().replace(lbs_autograd=True)):
        assert tuning.current().lbs_autograd is True
    assert tuning.current().lbs_autograd is tuning.DEFAULT.lbs_autograd


def test_flag_off_lbs_of_grad_requiring_tensors_builds_no_graph(monkeypatch):
    """With the flag off lbs() never looks at requires_grad: the call goes to the inference route as it always did (shown here with the C-ABI
    call replaced by a recorder: no GPU), and its outputs carry no grad_fn."""
    import torch
    from garment4d_amd import _lib, lbs as L, synthetic as syn, tuning
    assert tuning.current().lbs_autograd is False
    calls = []
    monkeypatch.setattr(L, "_f32", lambda t, name: t.contiguous())
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name) or 0)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(_lib, "lib", lambda: type("Fake", (), {"g4d_lbs_mfma_supported": staticmethod(lambda j, nb: 1), "g4d_lbs_mfma_ws_bytes": staticmethod(lambda b, j: 64)})())
    P = syn.smpl_like_params(V=20, seed=1)
    betas, pose = syn.smpl_like_pose(2, seed=2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    b, p = t(betas).requires_grad_(True), t(pose).requires_grad_(True)
    verts, joints = L.lbs(b, p, t(P["v_template"]), t(P["shapedirs"]), t(P["posedirs"]), t(P["J_regressor"]), t(P["parents"]), t(P["lbs_weights"]))
    assert calls == ["g4d_lbs_mfma_f32"] and verts.grad_fn is None and joints.grad_fn is None and not verts.requires_grad
    # flag on: a model constant that requires grad is refused before anything runs
    with tuning.use(tuning.current().replace(lbs_autograd=True)):
        with pytest.raises(NotImplementedError, match="model constants"):
            L.lbs(b, p, t(P["v_template"]).requires_grad_(True), t(P["shapedirs"]), t(P["posedirs"]), t(P["J_regressor"]), t(P["parents"]), t(P["lbs_weights"]))
    assert calls == ["g4d_lbs_mfma_f32"]


# ------------------------------------------------------------------------------------------------------------------------- the twin
def _case(J=24, NB=10, V=37, B=2, pose2rot=True, broadcast=False, seed=20):
    from garment4d_amd import synthetic as syn
    P = syn.smpl_like_params(V=V, J=J, num_betas=NB, seed=seed)
    betas, pose = syn.smpl_like_pose(B, J=J, num_betas=NB, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    if not pose2rot:
        pose = ST.rodrigues(pose.reshape(-1, 3))[0].reshape(B, J, 3, 3) + 0.01 * rng.standard_normal((B, J, 3, 3))
    return P, (betas[:1] if broadcast else betas).astype(np.float64), pose.astype(np.float64), rng.standard_normal((B, V, 3)), rng.standard_normal((B, J, 3))


@pytest.mark.parametrize("J,NB,pose2rot,broadcast", [(24, 10, True, False), (5, 1, False, False), (5, 3, True, True)])
def test_twin_float64_adjoint_equals_central_differences_of_its_forward(J, NB, pose2rot, broadcast):
    """Central differences with step h = 1e-5 of L = sum(verts g_v) + sum(joints g_p) in every beta and in (up to) 40 pose entries.  Observed,
    relative to the largest entry of the gradient: 6.5e-10, 1.1e-9 and 6.7e-10 on the three cases -- the rounding of the quotient, eps |L| / h
    with |L| of order 10 .. 100; the truncation error h^2 f''' / 6 is of order 1e-11.  The tolerance is 1e-8, ten times the worst observed."""
    P, betas, pose, gv, gp = _case(J=J, NB=NB, pose2rot=pose2rot, broadcast=broadcast)
    d_betas, d_pose = ST.adjoint(betas, pose, P, gv, gp, pose2rot)
    assert d_betas.shape == betas.shape and d_pose.shape == pose.shape

    def loss(b, p):
        v, j = ST.forward(b, p, P, pose2rot)
        return (v * gv).sum() + (j * gp).sum()

    h, rng, worst = 1e-5, np.random.default_rng(3), 0.0
    for which, x, grad, idx in (("b", betas, d_betas, range(betas.size)), ("p", pose, d_pose, rng.choice(pose.size, min(40, pose.size), replace=False))):
        for i in idx:
            plus, minus = x.copy(), x.copy()
            plus.reshape(-1)[i] += h
            minus.reshape(-1)[i] -= h
            cd = (loss(plus, pose) - loss(minus, pose)) / (2 * h) if which == "b" else (loss(betas, plus) - loss(betas, minus)) / (2 * h)
            worst = max(worst, abs(cd - grad.reshape(-1)[i]) / np.abs(grad).max())
    print(f"J={J} NB={NB} pose2rot={pose2rot} broadcast={broadcast}: central differences vs the twin's adjoint, relative: {worst:.3g}")
    assert worst <= 1e-8


def test_twin_reproduces_the_golden_float64_gradients_and_none_means_zero():
    """On the three golden cases the twin's float64 adjoint equals the float64 autograd of the reference's own lbs() to 1e-12 of the largest entry
    (observed 1e-15), the all-zero joints and the all-zero frame of case c included; a missing upstream gradient equals a zero one."""
    g = load_golden("smpl_grad.npz")
    P = {k[2:]: v for k, v in g.items() if k.startswith("P_")}
    for name in "abc":
        p2r = bool(g[f"{name}_pose2rot"])
        d_betas, d_pose = ST.adjoint(g[f"{name}_betas"], g[f"{name}_pose"], P, g[f"{name}_g_v"], g[f"{name}_g_p"], p2r)
        for k, got in (("d_betas", d_betas), ("d_pose", d_pose)):
            want = g[f"{name}_{k}64"]
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"golden {name} {k}: twin vs the reference's float64 autograd, relative {err:.3g}")
            assert got.shape == want.shape and err <= 1e-12 and np.isfinite(got).all()
        assert float(g[f"{name}_eref_d_pose"]) > 0 and float(g[f"{name}_eref_d_betas"]) > 0
    assert (g["c_pose"].reshape(5, 24, 3)[:, [0, 3, 7, 23]] == 0).all() and (g["c_pose"][2] == 0).all() and not bool(g["b_pose2rot"])
    a = ST.adjoint(g["a_betas"], g["a_pose"], P, None, g["a_g_p"])
    b = ST.adjoint(g["a_betas"], g["a_pose"], P, np.zeros_like(g["a_g_v"]), g["a_g_p"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    z = ST.adjoint(g["a_betas"], g["a_pose"], P, None, None)
    assert all((x == 0).all() for x in z)

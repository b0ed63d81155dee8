"""The kernels the model runs AROUND the hot path, at their launch edges: g4d_knn_f32 (csrc/knn.hip), g4d_knn_blend_weights_f32
(csrc/garment_ops.hip), g4d_segment_select_f32 / g4d_segment_take_f32 / g4d_vertex_normals_f32 (csrc/mesh_ops.hip), against the references of
tests/model_kernels_twin.py.  tests/test_model_kernels_cpu.py asserts the precondition of every case here (more ties than needed, spread over
every index byte; row counts off the 4-row block; the cut where the layout's name puts it; ...).

KNN and segmentation are bit-exact contracts (array_equal).  Blend weights and vertex normals are held to float64 with a bound derived from
the kernel's operation order (the twin's docstrings); each such test prints its worst err / bound ratio."""
import numpy as np
import pytest
import torch

import model_kernels_twin as T
from garment4d_amd import _lib
from garment4d_amd import mesh_utils as MU
from garment4d_amd.knn import knn_points

pytestmark = pytest.mark.gpu
both_modes = pytest.mark.usefixtures("contraction_mode")       # KNN: once per distance-contraction mode, library and oracle switched together


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# =============================================================================================================================== KNN
def _knn_check(q, pts, K):
    wd, wi = T.knn_exact(q, pts, K)
    r = knn_points(dev(q), dev(pts), K)
    gi, gd = host(r.idx), host(r.dists)
    assert np.array_equal(gi, wi), f"{int((gi != wi).sum())} of {wi.size} indices differ"
    assert np.array_equal(gd, wd, equal_nan=False)
    ok, why = T.knn_valid_in_float64(q, pts, gi, gd)
    assert ok, why
    return gi, gd


@both_modes
@pytest.mark.parametrize("K", [1, 64, 256])
@pytest.mark.parametrize("p2", T.LDS_P2)
def test_knn_large_lds(p2, K):
    """64 KB < 4 p2 <= 128 KB of distance keys behind ensure_dynamic_lds, up to the entry point's limit; p2 % 4 in {0, 1, 3} moves the
    histogram behind `dk + ((p2 + 3) & ~3)`."""
    _knn_check(*T.knn_case(f"lds_{p2}"), K)


def test_knn_refuses_p2_above_the_limit():
    q, pts = dev(np.zeros((1, 2, 3), np.float32)), dev(np.zeros((1, 32769, 3), np.float32))
    with pytest.raises(_lib.G4DError, match=r"p2 <= 32768"):
        knn_points(q, pts, 4)


@both_modes
@pytest.mark.parametrize("p2", [1, 2, 3, 255, 256])
def test_knn_k_equals_p2(p2):
    _knn_check(*T.knn_case(f"small_{p2}"), p2)


@both_modes
@pytest.mark.parametrize("K", [3, 256])
@pytest.mark.parametrize("p2", [257, 258, 259])
def test_knn_p2_off_a_multiple_of_4(p2, K):
    _knn_check(*T.knn_case(f"small_{p2}"), K)


@both_modes
@pytest.mark.parametrize("case,K", T.KNN_TIE_CASES)
def test_knn_boundary_ties(case, K):
    """More points AT the K-th distance than the answer needs, their indices spread over both index bytes p2 reaches: the second radix select
    (on the index) decides in its last TWO passes.  `shell`: the distances agree in their top 24 bits, the value select's first three passes find the
    whole shell in one bin."""
    q, pts = T.knn_case(case)
    gi, _ = _knn_check(q, pts, K)
    if case == "coincident":
        assert np.array_equal(gi, np.broadcast_to(np.arange(K), gi.shape))


@both_modes
@pytest.mark.parametrize("K", T.KNN_INF_K)
def test_knn_inf_distances(K):
    """Points with a +inf coordinate are at distance +inf (finite queries: no NaN), in index order behind the 20 finite ones."""
    q, pts = T.knn_case("inf")
    _, gd = _knn_check(q, pts, K)
    assert not np.isnan(gd).any() and np.array_equal(np.isinf(gd), np.broadcast_to(np.arange(K) >= 20, gd.shape))


# ===================================================================================================================== blend weights
SENTINEL = -12345.5


@pytest.mark.parametrize("case", T.blend_cases(), ids=lambda c: "F{}T{}Vg{}-K{}-J{}{}".format(*c[:5], "-nanrow" if c[5] else ""))
def test_blend_weights_vs_float64(case):
    """Direct g4d_knn_blend_weights_f32 calls: |out - float64| <= blend_gamma(K, J) sum_k |w_k W| per element, 8 sentinel rows behind the last
    row intact, the all-distances-zero row NaN in every joint with its neighbours within bound.
    Measured on MI355X, worst err / bound per case: 0.04 .. 0.19 (0.19 at K = 2, J = 64 and at Vg = 131, K = 65; 0.05 .. 0.10 at K = 256): the bound adds
    up to 268 worst-case roundings linearly where the real ones largely cancel, so a ratio of 0.1 at K = 256 is what to expect, and one near 1 would mean
    a lost term, not rounding.  K = 1 gives exactly 0: w = r / r = 1 and the one product W * 1 is exact."""
    F_, Tc, Vg, K, J, nan_row = case
    c = T.blend_case(*case)
    C = F_ // Tc
    want, bound = T.blend_weights_f64(c["W"][:F_], c["idx"][:C], c["d"][:C], Tc)
    W, idx, d = dev(c["W"]), dev(c["idx"]), dev(c["d"])
    rows = F_ * Vg
    out = torch.full((rows + 8, J), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.call("g4d_knn_blend_weights_f32", F_, Tc, Vg, c["V"], K, J, W.data_ptr(), idx.data_ptr(), d.data_ptr(), out.data_ptr(), _lib.stream_ptr())
    out = host(out)
    assert (out[rows:] == SENTINEL).all(), "rows behind the last one were written"
    got = out[:rows].reshape(F_, Vg, J).astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert nan.any() == nan_row and (not nan_row or nan[:, Vg // 2].all() and nan.sum() == Tc * J)
    err = np.abs(got - want)[~nan]
    ratio = np.max(err / np.maximum(bound[~nan], 1e-300))
    print(f"blend F={F_} T={Tc} Vg={Vg} K={K} J={J}: worst err/bound {ratio:.4f} (gamma = {T.blend_gamma(K, J) / T.U:.1f} u)")
    assert (err <= bound[~nan]).all(), f"worst err/bound {ratio}"


# ====================================================================================================================== segmentation
def _segment_check(name, c):
    case = T.segment_case(name, c)
    logits, target, n_out, xyz, feats = case["logits"], case["target"], case["n_out"], case["xyz"], case["feats"]
    wv, wf, wcounts, wsel = T.segment_exact(logits, target, n_out, xyz, feats)
    lg = dev(logits)
    # the selection itself first, with 8 sentinel slots behind the last frame's (a write past the end is caught here, inside the buffer)
    F_, n, classes = logits.shape
    sel = torch.full((F_ * n_out + 8,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((F_ + 8,), -7, dtype=torch.int32, device="cuda")
    _lib.call("g4d_segment_select_f32", F_, n, classes, target, n_out, lg.data_ptr(), sel.data_ptr(), cnt.data_ptr(), _lib.stream_ptr())
    sel, cnt = host(sel), host(cnt)
    assert (sel[F_ * n_out:] == -7).all() and (cnt[F_:] == -7).all(), "slots behind the last frame's were written"
    assert np.array_equal(sel[:F_ * n_out].reshape(F_, n_out), wsel) and np.array_equal(cnt[:F_], wcounts)
    gv, gf, counts = MU.segment_points(lg, target, n_out, dev(xyz), dev(feats))
    assert np.array_equal(host(counts), wcounts)
    assert np.array_equal(host(gv), wv) and np.array_equal(host(gf), wf)


@pytest.mark.parametrize("n", T.SEG_N)
def test_segment_sizes(n):
    """n around the wave (64) and the 1024-thread chunk, up to 9 chunks; three frames with three hit counts; take widths by turns."""
    _segment_check(f"n_{n}", T.SEG_WIDTHS[T.SEG_N.index(n) % 4])


@pytest.mark.parametrize("layout", T.SEG_LAYOUTS)
def test_segment_layouts(layout):
    """Where the n_out cut falls (inside a wave, on a wave boundary, on a chunk boundary, in the third chunk), count == n_out, no hit, all hits,
    n_out > n, one class, all-equal rows hitting target 0, NaN / +-inf / +-0.0 rows against np.argmax."""
    _segment_check(layout, T.SEG_WIDTHS[T.SEG_LAYOUTS.index(layout) % 4])


@pytest.mark.parametrize("c", T.SEG_WIDTHS)
def test_segment_take_widths(c):
    _segment_check("cut_third_chunk", c)


# ==================================================================================================================== vertex normals
def _vnorm_run(verts, faces):
    fid, vid = MU.calc_mesh_info(faces, verts.shape[-2])
    return host(MU.compute_vnorms(dev(verts), torch.from_numpy(np.array(faces)).cuda(), vid.cuda(), fid.cuda())).astype(np.float64)


@pytest.mark.parametrize("frames", [1, 3])
def test_vertex_normals_vs_float64(frames):
    """The hand-built mesh of model_kernels_twin.vnorm_mesh (472 vertices: frames * v is no multiple of 256): per vertex |got - float64| <= the twin's
    bound wherever that bound is <= 1e-4 (all but the 6 vertices built not to be); a vertex without faces, one with only zero-area faces and the three
    of the coincident opposite faces come out as exactly (0, 0, 0).
    Measured on MI355X: worst err / bound 0.102 (1 frame) and 0.105 (3 frames) over the compared vertices.  The 40-face fan centre sits at 0.005: its bound
    charges every face its worst case and the 39-deep sum 39 u on 40 unit vectors, while the fan's normals nearly agree and their errors do not add up --
    far below 1e-2 because the bound is loose there, not because the case is easy.  The 6 excluded vertices (bounds 1.4e-3 and 0.96) were off by 5e-7 at
    most."""
    m = T.vnorm_mesh(frames)
    want, bound = T.vertex_normals_f64(m["verts"], m["faces"])
    got = _vnorm_run(m["verts"], m["faces"])
    assert np.isfinite(got).all()
    for v in (m["lonely"], m["degenerate"], *m["opposite"]):
        assert (got[:, v] == 0).all(), f"vertex {v}: {got[:, v]}"
    cmp = bound <= T.VNORM_FLOAT_LIMIT
    assert cmp.sum() >= 0.98 * cmp.size
    err = np.linalg.norm(got - want, axis=-1)
    pos = cmp & (bound > 0)
    ratio = np.max(err[pos] / bound[pos])
    print(f"vertex normals frames={frames}: worst err/bound {ratio:.4f} over {int(cmp.sum())} of {cmp.size} vertices; "
          f"fan centre {err[:, m['centre']].max() / bound[:, m['centre']].min():.4f}; "
          f"excluded vertices' err {err[~cmp].max():.3e} (bound {bound[~cmp].min():.3e}..{bound[~cmp].max():.3e})")
    assert (err[cmp] <= bound[cmp]).all(), f"worst err/bound {ratio}"
    lens = np.linalg.norm(got, axis=-1)
    unit = np.linalg.norm(want, axis=-1) > 0.5
    assert np.abs(lens[unit & cmp] - 1.0).max() <= 1e-6                  # the final normalisation alone: 4 u = 2.4e-7


def test_vertex_normals_single_vertex():
    one = T.vnorm_single()
    got = _vnorm_run(one["verts"], one["faces"])
    assert got.shape == (3, 1, 3) and (got == 0).all()

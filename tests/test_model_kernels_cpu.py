"""tests/model_kernels_twin.py without a GPU: each twin is tied to the existing oracle on ordinary inputs, and the PRECONDITIONS of every case
of tests/test_model_kernels_gpu.py are asserted, so that no case there can pass vacuously -- a boundary-tie case really has more ties than it
needs, spread over every index byte; the shell case really keeps the value passes in one bin; a rows % 4 != 0 case really has such a row count;
every segmentation layout really puts its cut where its name says.  These are conditions on the inputs, not measurements of the kernels."""
import numpy as np
import pytest
import torch

import model_kernels_twin as T
from garment4d_amd import synthetic as syn
from oracle import model_oracle as MOr
from oracle import pointnet2_oracle as PO
from oracle import refine_oracle as RO

F32 = np.float32


@pytest.fixture(params=["nvcc", "off"])
def oracle_mode(request):
    prev = PO.set_contraction(request.param)
    yield request.param
    PO.set_contraction(prev)


# =============================================================================================================================== KNN
def test_knn_exact_is_the_oracle_and_valid_in_float64(oracle_mode):
    q, pts = syn.unit_cloud(2, 20, seed=1), syn.body_like_cloud(2, 500, seed=2, dup_frac=0.3, zero_frac=0.1)
    q[:, :5] = pts[:, :5]
    d, i = T.knn_exact(q, pts, 64)
    wd, wi = RO.knn_points(q, pts, 64)
    assert np.array_equal(d, wd) and np.array_equal(i, wi)
    ok, why = T.knn_valid_in_float64(q, pts, i, d)
    assert ok, why


def test_knn_valid_in_float64_rejects_wrong_answers():
    q, pts = syn.unit_cloud(1, 8, seed=3), syn.unit_cloud(1, 400, seed=4)
    d, i = T.knn_exact(q, pts, 16)
    assert T.knn_valid_in_float64(q, pts, i, d)[0]
    far = np.argmax(PO.pairwise_d2(q, pts), -1)
    j = i.copy(); j[0, :, -1] = far[0]                                # the farthest point in place of the 16th nearest
    dj = d.copy(); dj[0, :, -1] = np.take_along_axis(PO.pairwise_d2(q, pts), far[..., None], -1)[0, :, 0]
    assert not T.knn_valid_in_float64(q, pts, j, dj)[0]
    j = i.copy(); j[0, 2, 5] = j[0, 2, 4]                             # a repeated index
    assert not T.knn_valid_in_float64(q, pts, j, d)[0]
    assert not T.knn_valid_in_float64(q, pts, i, d * F32(1.0001))[0]  # distances that are not their indices' distances
    assert not T.knn_valid_in_float64(q, pts, i[..., ::-1], d[..., ::-1])[0]
    # the nearest neighbour swapped for a point one part in 10^9 farther (float64) is still a valid answer: fp32 cannot tell them apart
    q1 = np.zeros((1, 1, 3), F32)
    p1 = np.array([[[0.5, 0.25, 0.125], [0.5, 0.25, 0.125 + 2.0 ** -26], [3, 3, 3]]], F32)
    dd = PO.pairwise_d2(q1, p1)
    assert T.knn_valid_in_float64(q1, p1, np.array([[[1]]]), dd[..., 1:2])[0] and T.knn_valid_in_float64(q1, p1, np.array([[[0]]]), dd[..., :1])[0]


@pytest.mark.parametrize("p2", T.LDS_P2)
def test_knn_lds_cases_are_above_64_kb(p2):
    q, pts = T.knn_case(f"lds_{p2}")
    assert pts.shape == (2, p2, 3) and q.shape == (2, 9, 3)
    assert 4 * p2 > 64 * 1024 and p2 <= 32768
    assert {p % 4 for p in T.LDS_P2} == {0, 1, 3} and max(T.LDS_P2) == 32768          # the limit itself, and keys that end off a multiple of 4


@pytest.mark.parametrize("case,K", T.KNN_TIE_CASES)
def test_knn_tie_cases_reach_the_index_select(case, K, oracle_mode):
    q, pts = T.knn_case(case)
    p2 = pts.shape[1]
    reached = T.index_bytes_reached(p2)
    assert reached == [0, 1]                                                          # 256 < p2 <= 65536: two index passes have work
    hit = 0
    for (nties, need, group, distinct) in T.tie_stats(q[0], pts[0], K):
        if nties > need:
            hit += 1
            for b in reached:
                assert np.unique((group >> (8 * b)) & 255).size >= 2, f"{case}: tie group constant in index byte {b}"
            assert group.max() >= 2 ** 8                                              # ties above one byte's reach ...
            if case != "shell" or K > 2:
                assert group.size > K                                                 # ... in a group larger than K
    assert hit == q.shape[1], f"{case} K={K}: only {hit} of {q.shape[1]} queries have more ties than they need"


def test_knn_copies_cases_are_what_they_say(oracle_mode):
    q, pts = T.knn_case("copies_on")
    d, i = T.knn_exact(q, pts, 256)
    copies = np.nonzero((pts[0] == F32(0.5)).all(-1))[0]
    assert copies.size == 1000 and copies.max() >= 2 ** 14 and (d == 0).all()   # up to the top index bit p2 reaches
    assert np.array_equal(i[0, 0], copies[:256])                                      # the 256 lowest copy indices, in order
    q, pts = T.knn_case("copies_off")
    d, i = T.knn_exact(q, pts, 256)
    for r in range(q.shape[1]):
        nearer = int((~np.isin(i[0, r], copies)).sum())
        assert 1 <= nearer <= 16, nearer                                              # a few nearer points first ...
        assert np.array_equal(i[0, r, nearer:], copies[:256 - nearer])                # ... then the lowest copies
        assert (d[0, r, :nearer] < d[0, r, nearer]).all()


def test_knn_shell_case_keeps_the_value_passes_in_one_bin(oracle_mode):
    q, pts = T.knn_case("shell")
    d, i = T.knn_exact(q, pts, 256)
    assert i[0, 0, 0] == 0 and d[0, 0, 0] == 0
    vals = np.unique(d[0, 0])
    assert vals.size <= 4, vals.size                                                  # 0 and at most 3 values of R^2 up to rounding
    bits = vals[1:].view(np.uint32)
    assert np.unique(bits >> 8).size == 1                                             # they agree in their top 24 bits


def test_knn_inf_case(oracle_mode):
    q, pts = T.knn_case("inf")
    finite = np.isfinite(pts).all(-1)
    assert (finite.sum(1) == 20).all() and np.isfinite(q).all()
    assert min(T.KNN_INF_K) < 20 < max(T.KNN_INF_K) and 20 in T.KNN_INF_K
    d, i = T.knn_exact(q, pts, 256)
    assert not np.isnan(d).any() and np.isfinite(d[..., :20]).all() and np.isinf(d[..., 20:]).all()
    for b in range(2):
        assert np.array_equal(i[b, 0, 20:], np.nonzero(~finite[b])[0][:236])          # +inf distances in index order
    ok, why = T.knn_valid_in_float64(q, pts, i, d)
    assert ok, why


@pytest.mark.parametrize("p2", [1, 2, 3, 255, 256, 257, 258, 259])
def test_knn_small_cases(p2):
    q, pts = T.knn_case(f"small_{p2}")
    assert pts.shape == (2, p2, 3)
    assert {p % 4 for p in (257, 258, 259)} == {1, 2, 3}


# ===================================================================================================================== blend weights
def test_blend_gamma_is_the_documented_count():
    assert T.blend_gamma(256, 24) == T.gamma(12 + 129) and T.blend_gamma(256, 33) == T.gamma(12 + 256)
    assert T.blend_gamma(65, 32) == T.gamma(12 + 34) and T.blend_gamma(1, 1) == T.gamma(12 + 2)


@pytest.mark.parametrize("K,J", [(7, 24), (64, 24), (256, 40)])
def test_blend_twin_vs_oracle(K, J):
    rng = np.random.default_rng(K)
    F_, Tc, V, Vg = 6, 3, 500, 130
    W = rng.random((F_, V, J)).astype(F32)
    idx = rng.integers(0, V, (F_ // Tc, Vg, K)).astype(np.int32)
    d = rng.random((F_ // Tc, Vg, K)).astype(F32)
    d[0, :5, 0] = 0.0
    w = RO._interp_weights(d)
    want = np.stack([(W[f][idx[f // Tc]] * w[f // Tc][..., None]).sum(-2) for f in range(F_)])
    out, bound = T.blend_weights_f64(W, idx, d, Tc)
    err = np.abs(want.astype(np.float64) - out)
    print(f"K={K} J={J}: fp32 oracle vs float64 twin, worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()


def test_blend_twin_special_rows():
    W = np.arange(12, dtype=F32).reshape(1, 4, 3) + 1
    idx = np.array([[[0, 1, 2], [3, 2, 1], [0, 0, 3]]], np.int32)
    d = np.array([[[1.0, 0.0, 0.5], [0.0, 0.0, 0.0], [1e-42, 2.0, 2.0]]], F32)        # a zero, an all-zero row, a subnormal (fp32 1/d = inf)
    out, bound = T.blend_weights_f64(W, idx, d, 1)
    np.testing.assert_allclose(out[0, 0], (1 * W[0, 0] + 2 * W[0, 2]) / 3.0, rtol=1e-15)
    assert np.isnan(out[0, 1]).all() and np.isnan(bound[0, 1]).all()
    np.testing.assert_allclose(out[0, 2], (W[0, 0] + W[0, 3]) / 2.0, rtol=1e-15)      # the subnormal's weight is 0, as in fp32
    with np.errstate(over="ignore"):
        want = np.stack([(W[0][idx[0]] * RO._interp_weights(d)[0][..., None]).sum(-2)])
    assert np.array_equal(np.isnan(want), np.isnan(out))


@pytest.mark.parametrize("case", T.blend_cases())
def test_blend_case_preconditions(case):
    F_, Tc, Vg, K, J, nan_row = case
    c = T.blend_case(*case)
    C = F_ // Tc
    assert F_ % Tc == 0 and c["W"].shape == (F_ + 4, c["V"], J) and c["idx"].shape == c["d"].shape == (C + 4, Vg, K)
    d = c["d"]
    assert (d >= 0).all() and np.isfinite(d).all()
    assert not ((d > 0) & (d < np.finfo(F32).tiny)).any()                             # no subnormal distance
    assert (c["idx"] == 0).any(-1).all() if K > 1 else (c["idx"] == 0).any()
    assert (c["idx"] == c["V"] - 1).any(-1).all() if K > 1 else (c["idx"] == c["V"] - 1).any()
    allzero = (d[:C] == 0).all(-1)
    if nan_row:
        assert allzero.sum() == 1 and allzero[0, Vg // 2] and 0 < Vg // 2 < Vg - 1    # one NaN row, with neighbours on both sides
    else:
        assert not allzero.any()
    if K >= 2:
        assert ((d[:C] == 0).sum(-1) == 1).any()                                      # rows with exactly one zero distance
    out, bound = T.blend_weights_f64(c["W"][:F_], c["idx"][:C], d[:C], Tc)
    assert np.array_equal(np.isnan(out).any(-1), np.repeat(allzero, Tc, 0))


def test_blend_case_matrix_is_the_issues():
    cases = T.blend_cases()
    rows = {(F_, Tc, Vg) for (F_, Tc, Vg, *_r) in cases}
    assert rows == set(T.BLEND_ROWS)
    assert [F_ * Vg % 4 for (F_, _t, Vg) in T.BLEND_ROWS] == [1, 1, 2, 2, 0]            # the row tail of the 4-rows-per-block launch: 1, 2 rows
    assert {K for (_f, _t, _v, K, J, _n) in cases if J == 24} >= set(T.BLEND_K)
    for K in (65, 256):
        assert {J for (_f, _t, _v, k, J, _n) in cases if k == K} >= set(T.BLEND_J)
    assert {K % 64 for K in T.BLEND_K} >= {1, 63, 0} and {(K - 1) // 64 for K in T.BLEND_K if K % 2} == {0, 1, 2, 3}   # odd K in every register quarter
    assert any(n for (*_r, n) in cases)


# ====================================================================================================================== segmentation
@pytest.mark.parametrize("name", T.segment_case_names())
def test_segment_exact_vs_oracle(name):
    c = T.segment_case(name)
    gv, gf, counts, sel = T.segment_exact(c["logits"], c["target"], c["n_out"], c["xyz"], c["feats"])
    wv, wf = MOr.calc_segmentation_results(c["xyz"], c["logits"], c["n_out"], c["target"], c["feats"])
    assert np.array_equal(gv, wv) and np.array_equal(gf, wf)
    assert np.array_equal(counts, (np.argmax(c["logits"], 2) == c["target"]).sum(1))
    assert np.array_equal((sel >= 0).sum(1), np.minimum(counts, c["n_out"]))
    # torch.argmax (the reference's) and np.argmax (the twin's) agree on every row, the NaN / inf / signed-zero rows included
    assert np.array_equal(torch.argmax(torch.from_numpy(c["logits"].copy()), dim=2).numpy(), np.argmax(c["logits"], 2))


def test_segment_case_preconditions():
    counts = {}
    for name in T.segment_case_names():
        c = T.segment_case(name)
        hits = np.argmax(c["logits"], 2) == c["target"]
        counts[name] = hits.sum(1)
        assert c["logits"].shape[0] == 3
        if name.startswith("n_"):
            assert len(set(counts[name])) == 3 or c["logits"].shape[1] < 8, name       # three frames, three hit counts
    assert [T.segment_case(f"n_{n}")["logits"].shape[1] for n in T.SEG_N] == list(T.SEG_N)
    for name, cut in (("cut_in_wave", 1000), ("cut_on_wave", 1216), ("cut_on_1024", 2048), ("cut_third_chunk", 2500)):
        c = T.segment_case(name)
        hits = (np.argmax(c["logits"], 2) == c["target"])[0]
        first_out = np.nonzero(hits)[0][c["n_out"]]                                    # the hit that takes slot n_out: the first one cut
        assert first_out == cut == c["cut"] and hits[cut - 1]
        assert len(set(counts[name])) == 3 and counts[name][2] > c["n_out"]            # the LAST frame overflows too: a write at slot n_out lands behind sel
    assert 1000 % 64 != 0 and 1000 < 1024 and 1216 % 64 == 0 and 1216 % 1024 != 0 and 2048 % 1024 == 0 and 2048 < 2500 < 3072
    c = T.segment_case("count_eq_nout"); assert counts["count_eq_nout"][0] == c["n_out"]
    assert (counts["none_hit"] == 0).all() and (counts["all_hit"] == 2049).all() and T.segment_case("all_hit")["n_out"] < 2049
    c = T.segment_case("nout_gt_n"); assert c["n_out"] > c["logits"].shape[1] and counts["nout_gt_n"][1] == c["logits"].shape[1]
    c = T.segment_case("one_class"); assert c["logits"].shape[2] == 1 and c["target"] == 0 and (counts["one_class"] == 1500).all()
    c = T.segment_case("all_equal_target0")
    eq = (c["logits"] == c["logits"][..., :1]).all(-1)
    assert c["target"] == 0 and eq.any(1).all() and eq[2].all() and (np.argmax(c["logits"], 2)[eq] == 0).all()
    c = T.segment_case("specials")
    lg = c["logits"]
    assert np.isnan(lg).any() and np.isposinf(lg).any() and np.isneginf(lg).any() and (np.signbit(lg) & (lg == 0)).any()
    want = [1, 2, 1, 2, 2, 1, 0, 2, 2, 2, 1, 0, 2, 0, 2]                               # the arg-max of each SPECIAL_ROWS row, by hand
    assert list(np.argmax(T.SPECIAL_ROWS, 1)) == want
    assert list(torch.argmax(torch.from_numpy(T.SPECIAL_ROWS), 1).numpy()) == want
    assert 0 < counts["specials"].min() and len(T.SEG_WIDTHS) == 4


# ==================================================================================================================== vertex normals
def test_vertex_normals_twin_vs_oracle():
    scene = syn.garment_scene(2, 2, 64, seed=2)
    v = scene["batch"]["smpl_vertices_torch"].reshape(4, -1, 3)
    faces = scene["body"]["faces"]
    n, bound = T.vertex_normals_f64(v, faces)
    assert np.array_equal(n.astype(F32), MOr.compute_vnorms(v, faces))
    assert bound.shape == v.shape[:-1] and (bound > 0).all() and bound.max() < 1e-5    # an ordinary mesh: a few ulps per vertex
    for frames in (1, 3):
        m = T.vnorm_mesh(frames)
        n, _ = T.vertex_normals_f64(m["verts"], m["faces"])
        assert np.array_equal(n.astype(F32), MOr.compute_vnorms(m["verts"], m["faces"]))


@pytest.mark.parametrize("frames", [1, 3])
def test_vnorm_mesh_preconditions(frames):
    m = T.vnorm_mesh(frames)
    verts, faces = m["verts"], m["faces"]
    nv = verts.shape[1]
    assert verts.shape[0] == frames and (frames * nv) % 256 != 0 and frames * nv > 256
    n, bound = T.vertex_normals_f64(verts, faces)
    corners = np.bincount(faces.reshape(-1), minlength=nv)
    assert corners[m["lonely"]] == 0 and (n[:, m["lonely"]] == 0).all() and (bound[:, m["lonely"]] == 0).all()
    mine = faces[(faces == m["degenerate"]).any(1)]
    assert len(mine) >= 2 and all(len(set(f)) < 3 for f in mine.tolist())             # only faces that repeat an index
    assert (n[:, m["degenerate"]] == 0).all() and (bound[:, m["degenerate"]] == 0).all()
    opp = list(m["opposite"])
    assert (verts[:, opp] * 64 == np.round(verts[:, opp] * 64)).all()                 # dyadic coordinates
    assert (n[:, opp] == 0).all()                                                     # the float64 sum is exactly zero as well
    assert corners[m["centre"]] == 40
    s0, s1 = m["slivers"]
    strip = faces[((faces >= s0) & (faces < s1)).all(1)]
    e = verts[0][strip].astype(np.float64)
    sides = np.stack([np.linalg.norm(e[:, i] - e[:, (i + 1) % 3], axis=-1) for i in range(3)], -1)
    assert len(strip) == 24 and (sides.max(1) / sides.min(1) > 0.9e4).all()           # aspect 1e4 (the z jitter lengthens the short side a little)
    big = bound > T.VNORM_FLOAT_LIMIT
    assert big.sum(1).max() <= 0.02 * nv, big.sum(1)                                  # at most 2 % of the vertices leave the float comparison
    assert big[:, opp].all()
    tip = faces[list(m["tip_first"])].reshape(-1)
    assert set(np.nonzero(big[0])[0]) == set(opp) | set(tip.tolist())                 # ... and they are exactly the ones built to
    one = T.vnorm_single()
    assert one["verts"].shape == (3, 1, 3)
    n1, b1 = T.vertex_normals_f64(one["verts"], one["faces"])
    assert (n1 == 0).all() and (b1 == 0).all()

"""Garment post-processing without a GPU: the float64 twin against brute force, the algebra the solver rests on, argument validation of the
new entry points, and -- from the twin alone -- that the scenes tests/test_postprocess_gpu.py runs keep clear of every sign decision."""
import numpy as np
import pytest

import postprocess_twin as tw

EINVAL = 10001


# ------------------------------------------------------------------------------------------------------------- the twin's closest point
A, B, C = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 2.0, 0.0])


@pytest.mark.parametrize("q, part, point", [
    ((0.5, 0.5, 1.0), 0, (0.5, 0.5, 0.0)),      # above the interior
    ((1.0, -1.0, 0.5), 1, (1.0, 0.0, 0.0)),     # beyond edge ab
    ((2.0, 2.0, -0.5), 2, (1.0, 1.0, 0.0)),     # beyond edge bc
    ((-1.0, 1.0, 0.5), 3, (0.0, 1.0, 0.0)),     # beyond edge ca
    ((-1.0, -1.0, 0.5), 4, (0.0, 0.0, 0.0)),    # vertex a
    ((3.0, -0.5, 0.5), 5, (2.0, 0.0, 0.0)),     # vertex b
    ((-0.5, 3.0, 0.5), 6, (0.0, 2.0, 0.0)),     # vertex c
])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_closest_point_names_all_seven_parts(q, part, point, dtype):
    q = np.asarray(q, dtype=dtype)
    pt, d2, pr = tw.closest_on_triangle(q, A.astype(dtype), B.astype(dtype), C.astype(dtype))
    assert int(pr) == part and pt.dtype == dtype
    np.testing.assert_allclose(pt, point, atol=1e-6)
    np.testing.assert_allclose(d2, ((q - np.asarray(point, dtype=dtype)) ** 2).sum(), rtol=1e-5)


def test_twin_closest_point_against_a_barycentric_grid_search():
    """Random triangles and queries: the minimum over a 64-step barycentric grid is never below the twin's squared distance and exceeds it by
    at most the grid spacing squared, spacing = longest edge / 64.  Why: the grid cuts the triangle into cells similar to it, scaled by 1/64,
    so a grid point g lies within one spacing of the closest point cp -- and on cp's own edge when cp is on an edge, at cp when it is a
    vertex.  |q - g|^2 = |q - cp|^2 + 2 (q - cp).(cp - g) + |cp - g|^2, and the middle term vanishes: q - cp is normal to the plane for an
    interior hit and normal to the edge for an edge hit."""
    rng = np.random.default_rng(3)
    n, steps = 400, 64
    a, b, c = (rng.normal(0.0, 1.0, (n, 3)) for _ in range(3))
    q = rng.normal(0.0, 1.5, (n, 3))
    _, d2, part = tw.closest_on_triangle(q, a, b, c)
    assert set(np.unique(part)) == set(range(7))
    i, j = np.meshgrid(np.arange(steps + 1), np.arange(steps + 1), indexing="ij")
    keep = i + j <= steps
    v, w = i[keep] / steps, j[keep] / steps
    grid = a[:, None] + (b - a)[:, None] * v[None, :, None] + (c - a)[:, None] * w[None, :, None]
    gmin = ((q[:, None] - grid) ** 2).sum(-1).min(1)
    longest = np.sqrt(np.maximum(np.maximum(((b - a) ** 2).sum(1), ((c - a) ** 2).sum(1)), ((c - b) ** 2).sum(1)))
    step = longest / steps
    assert np.all(gmin >= d2 * (1 - 1e-12) - 1e-15)        # float64 rounding of the two evaluations only
    assert np.all(gmin - d2 <= step ** 2 + 1e-12)


def test_normal_equations_equal_the_stacked_least_squares_form():
    s = tw.scene("small")
    L = tw.laplacian(s["adj_old"])
    r = tw.scene_round("small")[0]
    assert r["count"] > 0
    M, b = tw.normal_equations(L, s["garment_v"][0], r["target"], r["w2"])
    import scipy.sparse.linalg as spla
    x = spla.spsolve(M, b)
    y = tw.stacked_least_squares(L, s["garment_v"][0], r["target"], r["w2"])
    np.testing.assert_allclose(x, y, rtol=0, atol=1e-12)
    lam = np.linalg.eigvalsh(M.toarray())
    assert lam[0] >= 1.0 - 1e-12 and lam[-1] <= 4.0 + np.linalg.norm(L.toarray(), 2) ** 2 + 1e-9     # spectrum in [1, ww^2 + |L|^2]


def test_laplacian_rows():
    import scipy.sparse as sp
    adj = sp.csr_matrix(np.array([[0, 2.0, 1.0, 0], [1.0, 0, 0, 0], [3.0, -1.0, 0, 0], [0, 0, 0, 0]]))
    L = tw.laplacian(adj).toarray()
    np.testing.assert_allclose(L, [[1, -0.5, -0.5, 0], [-1, 1, 0, 0], [-1, 0, 1, 0], [0, 0, 0, 1]])    # clip to [0,1]; empty row = identity row


# ----------------------------------------------------------------------------------------------------------------- argument validation
def _bad_calls():
    P = 1     # any non-null value: validation comes before the first dereference
    return {
        "g4d_taubin_smooth_f32": {"null": (1, 8, 3, 2, 0.05, -0.052, 5, 0, P, P, P, P, 0), "negative": (-1, 8, 3, 2, 0.05, -0.052, 5, P, P, P, P, P, 0),
                                  "vg": (1, 5105, 3, 2, 0.05, -0.052, 5, P, P, P, P, P, 0), "row": (1, 8, 3, 2, 0.05, -0.052, 9, P, P, P, P, P, 0),
                                  "empty": (0, 5104, 3, 2, 0.05, -0.052, 8, 0, 0, 0, 0, 0, 0)},
        "g4d_vertex_normals_area_f32": {"null": (1, 8, P, P, P, P, 0, 0, 0), "negative": (1, -8, P, P, P, P, 0, P, 0), "empty": (0, 8, 0, 0, 0, 0, 0, 0, 0)},
        "g4d_mesh_aabb_f32": {"null": (1, 8, 4, P, P, 0, 0), "negative": (1, 8, -4, P, P, P, 0), "empty": (0, 8, 4, 0, 0, 0, 0)},
        "g4d_mesh_nearest_f32": {"null": (1, 8, 8, 4, 1, P, P, P, P, P, P, 0, P, P, P, P, 0, 0, 0), "negative": (1, -8, 8, 4, 1) + (P,) * 6 + (0,) + (P,) * 5 + (0, 0),
                                 "empty": (0, 8, 8, 4, 1) + (0,) * 14},
        "g4d_depen_targets_f32": {"null": (1, 8, 0.008, 2.0, P, P, P, P, 0, P, P, 0, 0), "negative": (1, -8, 0.008, 2.0, P, P, P, P, 0, P, P, P, 0),
                                  "empty": (0, 8, 0.008, 2.0) + (0,) * 9},
        "g4d_depen_solve_f32": {"null": (1, 8, 32, 5, 5) + (P,) * 10 + (0, P, 0), "negative": (1, 8, -1, 5, 5) + (P,) * 12 + (0,),
                                "vg": (1, 5105, 32, 5, 5) + (P,) * 12 + (0,), "row": (1, 8, 32, 9, 5) + (P,) * 12 + (0,),
                                "row_t": (1, 8, 32, 5, 9) + (P,) * 12 + (0,), "empty": (0, 5104, 32, 8, 8) + (0,) * 13},
    }


@pytest.mark.parametrize("name", sorted(_bad_calls()))
def test_new_entry_points_validate_before_touching_the_device(name):
    from garment4d_amd import _lib
    L = _lib.lib()
    assert name in _lib.SIGNATURES
    for kind, args in _bad_calls()[name].items():
        assert len(args) == len(_lib.SIGNATURES[name]), (name, kind)
        rc = getattr(L, name)(*args)
        if kind == "empty":      # frames = 0 (with vg = 5104 where there is a limit): passes validation, launches nothing
            assert rc == 0, (name, kind, rc, L.g4d_last_error())
            continue
        assert rc == EINVAL, (name, kind, rc)
        msg = L.g4d_last_error().decode()
        assert name.split("_f32")[0] in msg, (name, kind, msg)
        needle = {"null": "null", "negative": "negative", "vg": "5104", "row": "8 entries", "row_t": "8 entries"}[kind]
        assert needle in msg.lower(), (name, kind, msg)


def test_nearest_cull_is_a_tuning_field(monkeypatch):
    from garment4d_amd import tuning
    assert tuning.Tuning().nearest_cull is True
    monkeypatch.setenv("G4D_NEAREST_CULL", "0")
    assert tuning.from_environment().nearest_cull is False
    monkeypatch.delenv("G4D_NEAREST_CULL")
    assert tuning.from_environment().nearest_cull is True


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    from garment4d_amd import postprocess as pp
    s = tw.scene("small")
    with pytest.raises(TypeError):
        pp.taubin_smooth(torch.from_numpy(s["garment_v"]), s["adj_old"])
    with pytest.raises(TypeError):
        pp.nearest_on_mesh(torch.from_numpy(s["garment_v"]), torch.from_numpy(s["body_v"]), s["body_faces"])


# ------------------------------------------------------------------------------------------- the GPU tests' inputs, judged by the twin alone
@pytest.mark.parametrize("name", ["small", "ragged", "large"])
def test_gpu_scenes_keep_clear_of_every_sign_decision(name):
    """No vertex of a GPU test scene has |(v - p) . n| or |m . n| inside the sign margins, so the float32 kernels must flag exactly the
    twin's vertices; at most 2 % of the queries sit within the classification margins (of a region boundary, or of a tie with another feature)."""
    rounds = tw.scene_round(name)
    unsafe = total = 0
    parts = set()
    for f, r in enumerate(rounds):
        assert np.abs(r["side"]).min() > tw.SIDE_MARGIN, (name, f, np.abs(r["side"]).min())
        assert np.abs(r["facing"]).min() > tw.FACING_MARGIN, (name, f, np.abs(r["facing"]).min())
        unsafe += int((~tw.safe_to_compare(r["near"])).sum())
        total += len(r["side"])
        parts |= set(np.unique(r["near"]["part"]).tolist())
    assert unsafe <= tw.MAX_UNSAFE_SHARE * total, (name, unsafe, total)
    if name != "large":                  # the nearest-point tests' queries: garment plus points farther out -- every part occurs
        near = tw.scene_nearest(name)
        parts = set(np.unique(np.concatenate([n["part"] for n in near])).tolist())
        assert parts == set(range(7)), (name, parts)
        safe = np.concatenate([tw.safe_to_compare(n) for n in near])
        assert (~safe).sum() <= tw.MAX_UNSAFE_SHARE * len(safe), (name, (~safe).sum(), len(safe))
    s = tw.scene(name)
    if s["clear_frame"] is not None:
        assert rounds[s["clear_frame"]]["count"] == 0
    assert all(r["count"] > 0 for f, r in enumerate(rounds) if f != s["clear_frame"])

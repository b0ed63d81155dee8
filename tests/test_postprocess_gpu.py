"""Garment post-processing on the GPU (garment4d_amd/postprocess.py over csrc/postprocess.hip and csrc/mesh_nearest.hip) against the float64
twin (tests/postprocess_twin.py).  Error yardsticks are the float32 twin's own error against float64, times 3 -- no constants.  The scenes
(twin.scene) are judged clear of every sign decision by tests/test_postprocess_cpu.py, from the twin alone.

How `face` / `part` are compared: a closest point on an edge or a vertex of a closed mesh belongs to two or more triangles that are exactly
tied in exact arithmetic, and which of them float32 or float64 rounding prefers is not a property of the kernel.  So away from region
boundaries and near-ties between features (twin.safe_to_compare; the rest is capped at 2 %) the FEATURE must agree -- the face for an interior hit, the vertex pair
of an edge, the vertex -- and where the twin's hit is interior (no tie possible) face and part must agree as they are.  The lowest-index
rule itself is pinned by an exact tie case."""
import numpy as np
import pytest
import torch

import postprocess_twin as tw

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def pp():
    from garment4d_amd import postprocess
    return postprocess


def within(got, want64, yard32, what):
    """|got - want64| <= 3 |yard32 - want64| elementwise; the figures are printed first."""
    err = np.abs(got.astype(F64) - want64)
    yard = np.abs(yard32.astype(F64) - want64)
    print(f"{what}: max error {err.max():.3e}, max yardstick {yard.max():.3e}, worst ratio over non-zero yardsticks "
          f"{(err[yard > 0] / yard[yard > 0]).max() if (yard > 0).any() else 0:.3f}, elements over: {(err > 3 * yard).sum()} of {err.size}")
    assert np.all(err <= 3 * yard), what


# ------------------------------------------------------------------------------------------------------------------------ smoothing
@pytest.mark.parametrize("name", ["small", "large"])
def test_taubin_smooth_equals_the_per_step_kernel_bit_for_bit_and_the_twin(name):
    from garment4d_amd import _lib
    from garment4d_amd.garment_lbs import _smoothing_csr
    s = tw.scene(name)
    x = dev(s["garment_v"])
    got = pp().taubin_smooth(x, s["adj_old"])
    rowptr, colidx, vals, n, _ = _smoothing_csr(s["adj_old"], x.device)
    a, b = x.clone(), torch.empty_like(x)
    for it in range(100):
        _lib.call("g4d_spmm_axpy_rows_f32", x.shape[0], x.shape[1], 3, a.data_ptr(), rowptr.data_ptr(), colidx.data_ptr(), vals.data_ptr(),
                  -0.052 if it & 1 else 0.05, b.data_ptr(), _lib.stream_ptr())
        a, b = b, a
    assert torch.equal(got, a)
    assert torch.equal(x, dev(s["garment_v"]))                                  # the input is read, never written
    within(host(got), tw.taubin_smooth(s["garment_v"], s["adj_old"], dtype=F64), tw.taubin_smooth(s["garment_v"], s["adj_old"], dtype=F32), "taubin " + name)


def test_taubin_smooth_refuses_a_mesh_outside_the_kernel_domain():
    import scipy.sparse as sp
    n = 12
    adj = sp.lil_matrix((n, n))
    adj[0, 1:11] = 1.0                   # a row of 10 entries (11 with the diagonal of D^-1 A - I)
    adj[1:11, 0] = 1.0
    with pytest.raises(NotImplementedError):
        pp().taubin_smooth(torch.zeros(1, n, 3, device="cuda"), adj.tocsr())


# --------------------------------------------------------------------------------------------------------------------- nearest point
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_nearest_on_mesh_against_the_twin(name):
    s = tw.scene(name)
    got = pp().nearest_on_mesh(dev(s["queries"]), dev(s["body_v"]), s["body_faces"])
    t64, t32 = tw.scene_nearest(name, F64), tw.scene_nearest(name, F32)
    cat = lambda rs, k: np.stack([r[k] for r in rs])
    within(host(got.dist2), cat(t64, "dist2"), cat(t32, "dist2"), "dist2 " + name)
    within(host(got.point), cat(t64, "point"), cat(t32, "point"), "point " + name)
    safe = np.stack([tw.safe_to_compare(r) for r in t64])
    assert (~safe).mean() <= tw.MAX_UNSAFE_SHARE, (~safe).mean()
    face, part = host(got.face), host(got.part)
    assert set(np.unique(part).tolist()) == set(range(7))                        # all seven parts are hit
    feature = np.stack([tw.feature_of(s["body_faces"], face[f], part[f]) for f in range(len(face))])
    assert np.array_equal(feature[safe], cat(t64, "feature")[safe])
    interior = safe & (cat(t64, "part") == 0)
    assert interior.sum() > 0.5 * safe.sum()
    assert np.array_equal(face[interior], cat(t64, "face")[interior]) and np.array_equal(part[interior], cat(t64, "part")[interior])
    n_got, n64, n32 = host(got.normal), cat(t64, "normal"), cat(t32, "normal")
    within(n_got[safe], n64[safe], n32[safe], "normal " + name)


def test_nearest_on_mesh_breaks_an_exact_tie_towards_the_lower_face_index():
    """Two triangles share the edge (0,0,0)-(1,0,0) and fold away from the query on their bisecting plane: both report the edge point
    (0.5, 0, 0) at squared distance 1, exactly (small dyadic coordinates) -- the lower face index wins, whichever way the faces are ordered."""
    verts = np.array([[[0, 0, 0], [1, 0, 0], [0.5, -1, -1], [0.5, 1, -1]]], dtype=F32)
    q = dev(np.array([[[0.5, 0, 1]]], dtype=F32))
    for faces, want_part in ((np.array([[0, 1, 3], [1, 0, 2]], dtype=np.int32), 1), (np.array([[2, 1, 0], [0, 1, 3]], dtype=np.int32), 2)):
        got = pp().nearest_on_mesh(q, dev(verts), faces)
        assert host(got.face).tolist() == [[0]] and host(got.part).tolist() == [[want_part]]
        assert host(got.dist2).tolist() == [[1.0]] and host(got.point).tolist() == [[[0.5, 0.0, 0.0]]]
        n = host(got.normal)[0, 0]
        assert abs(n[1]) < 1e-7 and n[2] > 0.99 and abs(n[0]) < 1e-7            # the two corner normals' sum: straight up the ridge


@pytest.mark.parametrize("name", ["small", "ragged", "large"])
def test_nearest_cull_on_and_off_give_the_same_bits(name, tune):
    s = tw.scene(name)
    q, bv = dev(s["queries"]), dev(s["body_v"])
    waves = q.shape[0] * ((q.shape[1] + 63) // 64)
    nblocks = (len(s["body_faces"]) + 63) // 64
    seen_on = torch.zeros(waves, dtype=torch.int32, device="cuda")
    on = pp().nearest_on_mesh(q, bv, s["body_faces"], visited=seen_on)
    tune(nearest_cull=False)
    seen_off = torch.zeros(waves, dtype=torch.int32, device="cuda")
    off = pp().nearest_on_mesh(q, bv, s["body_faces"], visited=seen_off)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    assert int(seen_off.min()) == nblocks == int(seen_off.max())
    print(f"cull {name}: {float(seen_on.float().mean()):.2f} of {nblocks} face blocks visited per wave")
    assert int(seen_on.max()) <= nblocks and float(seen_on.float().mean()) < nblocks


# -------------------------------------------------------------------------------------------------------------------- depenetration
def gpu_flags(s):
    """The flags of the first round as the kernels decide them (w2 == ww^2), through the same calls remove_interpenetration makes."""
    from garment4d_amd import _lib
    P = pp()
    v = dev(s["garment_v"])
    F_, Vg, _ = v.shape
    body = P._SearchMesh(dev(s["body_v"]), s["body_faces"])
    near = body.nearest(v)
    m = P.vertex_normals_area(v, P.mesh_topology(s["garment_faces"], Vg, v.device, v[0]))
    w2 = torch.empty((F_, Vg), device="cuda")
    target = torch.empty((F_, Vg, 3), device="cuda")
    counts = torch.empty(F_, dtype=torch.int32, device="cuda")
    _lib.call("g4d_depen_targets_f32", F_, Vg, 0.008, 2.0, v.data_ptr(), near.point.data_ptr(), near.normal.data_ptr(), m.data_ptr(), None,
              w2.data_ptr(), target.data_ptr(), counts.data_ptr(), _lib.stream_ptr())
    return host(w2) == 4.0, host(counts)


@pytest.mark.parametrize("name", ["small", "ragged", "large"])
def test_one_depenetration_round_against_the_twin(name):
    s = tw.scene(name)
    t64, t32 = tw.scene_round(name, F64), tw.scene_round(name, F32)
    flags, counts0 = gpu_flags(s)
    assert np.array_equal(flags, np.stack([r["flagged"] for r in t64]))          # the flags equal the twin's
    g = dev(s["garment_v"])
    verts, counts, residual = pp().remove_interpenetration(g, s["garment_faces"], dev(s["body_v"]), s["body_faces"], s["adj_old"], rounds=1)
    assert torch.equal(g, dev(s["garment_v"]))
    verts, counts, residual = host(verts), host(counts), host(residual)
    assert counts.shape == (1, len(t64)) and residual.shape == (1, len(t64), 3)
    assert counts[0].tolist() == [r["count"] for r in t64] == counts0.tolist()
    for f, (r64, r32) in enumerate(zip(t64, t32)):
        if r64["count"] == 0:                                                    # nothing behind the body: bit-unchanged, nothing solved
            assert np.array_equal(verts[f], s["garment_v"][f]) and not residual[0, f].any()
            continue
        err = np.linalg.norm(verts[f].astype(F64) - r64["verts"], axis=0)
        yard = np.linalg.norm(r32["verts"].astype(F64) - r64["verts"], axis=0)
        trunc = residual[0, f].astype(F64) * np.linalg.norm(r64["b"], axis=0)    # |x - x*| <= |M^-1| |b - M x| <= residual |b|: M >= I
        print(f"depen {name} frame {f}: |x - x64| {err}, 3 x float32 twin {3 * yard}, truncation bound {trunc}, residual {residual[0, f]}, "
              f"float32 twin residual {r32['residual']}")
        assert np.all(err <= 3 * yard + trunc)
        assert np.all(residual[0, f] <= 3 * r32["residual"])


def test_five_rounds_equal_five_chained_calls_and_stop_per_frame():
    s = tw.scene("small")
    args = (s["garment_faces"], dev(s["body_v"]), s["body_faces"], s["adj_old"])
    verts, counts, residual = pp().remove_interpenetration(dev(s["garment_v"]), *args, rounds=5)
    v, chained = dev(s["garment_v"]), []
    for _ in range(5):
        v, c, _ = pp().remove_interpenetration(v, *args, rounds=1)
        chained.append(host(c)[0])
    assert torch.equal(verts, v)
    counts = host(counts)
    assert np.array_equal(counts, np.stack(chained))
    print("counts per round and frame:\n", counts)
    for f in range(counts.shape[1]):
        zero = np.nonzero(counts[:, f] == 0)[0]
        if len(zero):
            assert not counts[zero[0]:, f].any()                                 # never increases after reaching 0
    clear = s["clear_frame"]
    assert counts[0, clear] == 0 and torch.equal(verts[clear], dev(s["garment_v"])[clear])     # bit-unchanged through all five rounds
    _, twin_counts = tw.remove_interpenetration(s["garment_v"], s["garment_faces"], s["body_v"], s["body_faces"], s["adj_old"], rounds=5)
    print("twin counts:\n", twin_counts)
    for f in range(counts.shape[1]):
        assert counts[-1, f] == 0 or counts[-1, f] == twin_counts[-1, f]


def test_post_process_is_reproducible_and_composes():
    s = tw.scene("ragged")
    P = pp()
    args = (s["garment_faces"], dev(s["body_v"]), s["body_faces"], s["adj_old"])
    a = P.post_process(dev(s["garment_v"]), *args)
    b = P.post_process(dev(s["garment_v"]), *args)
    c = P.remove_interpenetration(P.taubin_smooth(dev(s["garment_v"]), s["adj_old"]), *args)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)                            # two runs give equal bits; post_process = the composition

    class Model:
        adj_old = s["adj_old"]
    out = {"iter_regressed_lbs_garment_v": [None, dev(s["garment_v"])], "garment_f_3": s["garment_faces"]}
    batch = {"smpl_vertices_torch": torch.from_numpy(s["body_v"]).reshape(1, *s["body_v"].shape)}
    d = P.post_process_output(out, batch, Model(), body_faces=s["body_faces"])
    assert torch.equal(d[0], a[0]) and torch.equal(d[1], a[1])


def test_post_process_under_graph_capture_replays_the_eager_result():
    s = tw.scene("small")
    P = pp()
    g, bv = dev(s["garment_v"]), dev(s["body_v"])
    eager = P.post_process(g, s["garment_faces"], bv, s["body_faces"], s["adj_old"])     # also builds the per-topology tables
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P.post_process(g, s["garment_faces"], bv, s["body_faces"], s["adj_old"])         # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = P.post_process(g, s["garment_faces"], bv, s["body_faces"], s["adj_old"])
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert torch.equal(x, y)

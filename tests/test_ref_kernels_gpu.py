"""The nine point-set ops against the reference's OWN kernel source: oracle/_ref/libpointnet2_ref.so is the reference's four
pointnet2 kernel files compiled for gfx950 with -O2 -ffp-contract=off (`make -C oracle ref`, run by build() where a checkout of the
reference is at hand).  Every test asserts two things, bit for bit unless it says otherwise:

    reference build == oracle in `off` mode       pins the restatement oracle/g4d_oracle.c, which every other index test rests on
    reference build == product in `off` mode      pins the HIP kernels without the oracle in between

What this does NOT pin is nvcc's choice of fused multiply-adds in the squared distance (tests/test_cuda_pin.py, ops_cuda.npz).

The reference's kernels check nothing, so it is never given an empty grid or an index outside its array (oracle/ref_pointnet2.py
refuses both before it launches anything)."""
import numpy as np
import pytest

import ref_kernel_cases as RC
from oracle import pointnet2_oracle as K
from oracle import ref_pointnet2 as REF

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not REF.available(), reason="oracle/_ref/libpointnet2_ref.so is absent: build it with "
                                 "`G4D_REFERENCE_DIR=<checkout of the reference> make -C oracle ref` (build() does where it finds one)")]
TOL = dict(rtol=1e-5, atol=1e-5)     # tests/test_ops_gpu.py: the project's stated bound for float outputs


@pytest.fixture(autouse=True)
def off_mode():
    """Oracle and product both in contraction mode `off` for the length of one test, whatever the process-wide mode is."""
    from garment4d_amd import numerics
    prev = K.set_contraction("off")
    try:
        with numerics.distance_contraction("off"):
            yield
    finally:
        K.set_contraction(prev)


@pytest.fixture(scope="module")
def mods():
    """(reference build, oracle, product): three modules with the reference extension's nine entry points."""
    from garment4d_amd import pointnet2_cuda as product
    return REF, K.as_pointnet2_cuda_module(), product


def check(ref, oracle, product, what):
    """ref / oracle / product: an array or a tuple of arrays each."""
    for r, o, p, name in zip(*[x if isinstance(x, tuple) else (x,) for x in (ref, oracle, product)], what.split(",")):
        assert RC.same(r, o), f"{name}: reference build != oracle(off): {RC.first_diff(r, o)}"
        assert RC.same(r, p), f"{name}: reference build != product(off): {RC.first_diff(r, p)}"


def test_fps_block_size_choice_for_every_cloud_size():
    """opt_n_threads() goes through log()/log(2) in double: the oracle's restatement against the reference's own function, compiled,
    for every n up to 40000 (host only)."""
    got = np.array([K.block_size(n) for n in range(1, RC.BLOCK_SIZE_MAX_N + 1)])
    want = np.array([REF.opt_n_threads(n) for n in range(1, RC.BLOCK_SIZE_MAX_N + 1)])
    assert np.array_equal(got, want), f"first mismatch at n = {1 + int(np.argmax(got != want))}"
    assert set(want.tolist()) == {1 << k for k in range(11)}


def test_fps_sizes_reach_every_template_block_size():
    assert {K.block_size(n) for n in RC.FPS_SIZES} == {1 << k for k in range(11)}


@pytest.mark.parametrize("case", RC.fps_cases(), ids=RC.case_id)
def test_fps(case, mods):
    """idx and the final temp; sizes at and around every power of two up to the 1024-thread block, duplicates and zero padding (the
    block-size-dependent tie-break of the tree reduction), a NaN point, an inf coordinate."""
    xyz, m = RC.fps_inputs(case)
    ref, orc, prod = (RC.run_fps(mod, dev, xyz, m) for mod, dev in zip(mods, ("cuda", "cpu", "cuda")))
    assert ref[0].min() >= 0 and ref[0].max() < case["n"]
    check(ref, orc, prod, "idx,temp")


@pytest.mark.parametrize("case", RC.ball_cases(), ids=RC.case_id)
def test_ball_query(case, mods):
    """`fill with the first hit`, the cnt handling and the strict `<` against radius^2: a query with no neighbour (row stays zero),
    queries on duplicated points and on the zero padding, radius 0, nsample 1 / 5 / 64 / 128."""
    xyz, q = RC.ball_inputs(case)
    ref, orc, prod = (RC.run_ball(mod, dev, xyz, q, case["radius"], case["nsample"]) for mod, dev in zip(mods, ("cuda", "cpu", "cuda")))
    assert not ref[:, 0].any()                       # query 0 has no neighbour: the caller's zeros stay
    if case["radius"] == 0.0:
        assert not ref.any()
    check(ref, orc, prod, "idx")


@pytest.mark.parametrize("case", RC.nn_cases(), ids=RC.case_id)
def test_three_nn(case, mods):
    """dist2 and idx: the strict `<` cascade (ties keep the lower index), the 1e40 sentinels for fewer than three known points,
    non-finite coordinates."""
    un, kn = RC.nn_inputs(case)
    ref, orc, prod = (RC.run_nn(mod, dev, un, kn) for mod, dev in zip(mods, ("cuda", "cpu", "cuda")))
    if kn.shape[1] < 3:
        assert np.isinf(ref[0][..., kn.shape[1]:]).all() and not ref[1][..., kn.shape[1]:].any()
    check(ref, orc, prod, "dist2,idx")


@pytest.mark.parametrize("B,C,N,P,S", RC.GGI_SHAPES)
def test_group_gather_interpolate_forward(B, C, N, P, S, mods):
    pts, idx, i3, w = RC.ggi_inputs(B, C, N, P, S)
    devs = ("cuda", "cpu", "cuda")
    check(*(RC.run_group(mod, dev, pts, idx) for mod, dev in zip(mods, devs)), "group")
    check(*(RC.run_gather(mod, dev, pts, idx[:, :, 0]) for mod, dev in zip(mods, devs)), "gather")
    ref, orc, prod = (RC.run_interp(mod, dev, pts, i3, w) for mod, dev in zip(mods, devs))
    assert RC.same(ref, orc), f"three_interpolate: reference build != oracle: {RC.first_diff(ref, orc)}"
    np.testing.assert_allclose(prod, ref, **TOL)     # the product's contraction of the weighted sum is not part of the `off` contract


@pytest.mark.parametrize("collide", [False, True], ids=["spread", "colliding"])
@pytest.mark.parametrize("B,C,N,P,S", [(2, 7, 100, 13, 5), (2, 3, 1024, 256, 32), (1, 195, 256, 64, 64), (2, 5, 300, 257, 3)])
def test_backward_kernels_on_exact_sums(B, C, N, P, S, collide, mods):
    """The three scatter-add kernels on inputs whose every partial sum is exact (RC.exact_grad_inputs): the order of the atomics
    cannot show, so all three implementations agree bit for bit -- also where a whole neighbourhood, and half of all neighbourhoods,
    hit one source."""
    idx, i3, w, go_group, go_gather, go_interp = RC.exact_grad_inputs(B, C, N, P, S, collide)
    devs = ("cuda", "cpu", "cuda")
    ref = RC.run_group_grad(mods[0], "cuda", go_group, idx, N)
    assert np.array_equal(ref, np.round(ref))        # integer cotangents: the sums are integers, nothing was rounded away
    check(ref, *(RC.run_group_grad(mod, dev, go_group, idx, N) for mod, dev in zip(mods[1:], devs[1:])), "group_grad")
    check(*(RC.run_gather_grad(mod, dev, go_gather, idx[:, :, 0], N) for mod, dev in zip(mods, devs)), "gather_grad")
    ref = RC.run_interp_grad(mods[0], "cuda", go_interp, i3, w, N)
    assert np.array_equal(ref * 4, np.round(ref * 4))
    check(ref, *(RC.run_interp_grad(mod, dev, go_interp, i3, w, N) for mod, dev in zip(mods[1:], devs[1:])), "interp_grad")


def test_loader_refuses_what_the_kernels_would_not_survive():
    """Empty grids and out-of-range indices never reach the reference's kernels."""
    import torch
    x = torch.zeros((1, 4, 3), device="cuda")
    with pytest.raises(ValueError):
        REF.furthest_point_sampling_wrapper(1, 4, 0, x, torch.zeros((1, 4), device="cuda"), torch.zeros((1, 0), dtype=torch.int32, device="cuda"))
    pts = torch.zeros((1, 2, 4), device="cuda")
    bad = torch.tensor([[0, 4]], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        REF.gather_points_wrapper(1, 2, 4, 2, pts, bad, torch.zeros((1, 2, 2), device="cuda"))
    with pytest.raises(ValueError):
        REF.gather_points_wrapper(1, 2, 4, 2, pts, bad.clamp(max=3), torch.zeros((1, 2, 3), device="cuda"))

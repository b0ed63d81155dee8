"""The pose-domain cases of tests/smpl_domain_cases.py without a GPU: the builder is reproducible and every kind is what its name says; both
fp32 restatements of lbs() and the float64 twin stay finite on every shape and kind; the twin's float64 adjoint -- the yardstick of
tests/test_smpl_domain_gpu.py -- equals central differences of its own forward at pi, beyond it and at tens of radians as it does at ordinary
poses; and the comparison the GPU tests use rejects a result that is off by 10 x the baseline fp32 error on one kind."""
import functools

import numpy as np
import pytest

import smpl_domain_cases as D
import smpl_grad_twin as ST

PI32 = float(np.float32(np.pi))


@functools.lru_cache(maxsize=None)
def _case(V, J, NB):
    return D.case(V, J, NB, seed=V + J + NB)


# ------------------------------------------------------------------------------------------------------------------------- the builder
CHECKSUMS = {(97, 24, 10): [-20.20850913056343, -57.34023624509097, 8032.914915790532],     # smpl_domain_cases.checksum of (betas, pose)
             (65, 25, 8): [23.66733276081919, 35.60091270926426, 8291.735337277447],
             (65, 25, 9): [9.494134208736323, 83.79382441704, 8043.699650865946],
             (33, 2, 1): [-8.391445830878581, -134.3726336436463, 701.6350717422499],
             (130, 5, 16): [84.99504851412094, 123.96592186522552, 1495.9872228935742]}


@pytest.mark.parametrize("V,J,NB", D.SHAPES)
def test_builder_is_reproducible_and_pinned(V, J, NB):
    P, betas, pose, kinds = _case(V, J, NB)
    P2, betas2, pose2, kinds2 = D.case(V, J, NB, seed=V + J + NB)
    assert np.array_equal(betas, betas2) and np.array_equal(pose, pose2) and kinds == kinds2
    assert all(np.array_equal(P[k], P2[k]) for k in P)
    assert betas.dtype == np.float32 and pose.dtype == np.float32 and betas.shape == (33, NB) and pose.shape == (33, J * 3)
    assert kinds == [k for k in D.KINDS for _ in range(3)] and len(D.KINDS) == 11
    assert 33 % 8 and 33 % 16 and 33 % 2
    assert P["v_template"].shape == (V, 3) and P["lbs_weights"].shape == (V, J) and P["shapedirs"].shape == (V, 3, NB)
    np.testing.assert_allclose(D.checksum(betas, pose), CHECKSUMS[(V, J, NB)], rtol=1e-12, atol=0)
    assert not np.array_equal(D.case(V, J, NB, seed=V + J + NB + 1)[2], pose)


def test_shapes_reach_the_domain_edges():
    nc = {s: s[2] + 9 * (s[1] - 1) for s in D.SHAPES}
    assert nc[(97, 24, 10)] == 217 and nc[(65, 25, 8)] == 224 and nc[(65, 25, 9)] == 225 and D.MAX_COEFFS == 224
    assert [D.in_fast_domain(J, NB) for _, J, NB in D.SHAPES] == [True, True, False, True, True]
    assert (5 * 4) % 16 != 0 and all(V % 32 for V, _, _ in D.SHAPES)


@pytest.mark.parametrize("V,J,NB", D.SHAPES)
def test_every_kind_is_what_its_name_says(V, J, NB):
    _, betas, pose, kinds = _case(V, J, NB)
    ang = D.angles(pose, J)
    p = pose.reshape(33, J, 3).astype(np.float64)
    rows = lambda k: [i for i, kk in enumerate(kinds) if kk == k]
    u32 = lambda x: float(np.spacing(np.float32(x)))                         # one float32 ulp at x: the rounding of a component
    for k in D.KINDS:
        f = rows(k)
        assert len(f) == 3
        a = ang[f]
        if J > 1 and k not in ("zeros",):                                    # different random axes per frame
            assert not np.array_equal(p[f[0]], p[f[1]]) and not np.array_equal(p[f[1]], p[f[2]])
        if k == "baseline":
            assert 0.0 < a.min() and a.max() < 0.2 * 6 and np.abs(p[f]).std() > 0.1
        elif k == "zeros":
            assert (pose[f] == 0).all()
        elif k == "tiny":
            assert 0.0 < a.min() and a.max() < 6e-6 and a.max() > 1e-7
        elif k == "small":
            assert 0.0 < a.min() and a.max() < 6e-3 and a.max() > 1e-4
        elif k == "single_axis":
            assert ((p[f] != 0).sum(2) == 1).all()
            vals = np.abs(p[f]).max(2)
            assert all(min(abs(v - w) for w in (np.pi / 2, 0.3, np.pi)) <= u32(np.pi) for v in vals.ravel())
            assert (p[f].reshape(-1, 3)[np.isclose(np.abs(p[f]).max(2).ravel(), np.pi)] >= 0).all()     # pi only with the plus sign
        elif k == "near_pi":
            assert np.abs(a - (np.pi - 1e-3)).max() <= 2 * u32(np.pi) and a.max() < np.pi
        elif k == "at_pi":
            assert np.abs(a - PI32).max() <= 2 * u32(np.pi)
        elif k == "pi_to_2pi":
            assert a.min() >= np.pi - 2 * u32(np.pi) and a.max() <= 2 * np.pi + 2 * u32(2 * np.pi) and (J < 3 or a.max() - a.min() > 0.1)
        elif k == "near_2pi":
            assert np.abs(np.abs(a - 2 * np.pi) - 1e-3).max() <= 2 * u32(2 * np.pi)
        elif k == "large":
            assert a.min() >= 10 - 1e-4 and a.max() <= 100 + 1e-4
        elif k == "mixed":
            m = D.mixed_joint(J)
            assert m == (3 if J > 3 else J - 1) and m >= 1
            assert np.abs(a[:, 0] - (np.pi - 1e-2)).max() <= 2 * u32(np.pi)
            assert (p[f][:, m] == np.array([0, 0, 1.5])).all()
            rest = [j for j in range(1, J) if j != m]
            assert not rest or (0 < a[:, rest].min() and a[:, rest].max() < 6e-5)
    assert {k for k in D.KINDS if len({tuple(np.round(ang[i], 3)) for i in rows(k)}) > 1} >= {"baseline", "pi_to_2pi", "large"} or J < 3
    scale = np.abs(betas).max(1)
    assert betas[:3].std() < betas[-3:].std() and scale[-1] > 2.0 and scale.max() < 3 * 5


def test_one_frame_per_kind_takes_the_first_frame_of_each():
    _, betas, pose, kinds = _case(97, 24, 10)
    b, p, k = D.one_frame_per_kind(betas, pose, kinds)
    assert k == list(D.KINDS) and np.array_equal(b, betas[::3]) and np.array_equal(p, pose[::3])


# ------------------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("pose2rot", [True, False])
@pytest.mark.parametrize("V,J,NB", D.SHAPES)
def test_both_fp32_restatements_and_the_float64_twin_are_finite_on_every_kind(V, J, NB, pose2rot):
    P, betas, pose, kinds = _case(V, J, NB)
    pose_in = pose if pose2rot else D.rot_input(pose, J)
    want, refs = D.forward_refs(P, betas, pose_in, pose2rot)
    for name, (v, j) in (("twin", want), ("torch fp32", refs[0]), ("oracle fp32", refs[1])):
        assert v.shape == (33, V, 3) and j.shape == (33, J, 3), name
        assert np.isfinite(v).all() and np.isfinite(j).all(), name
    # and the restatements are fp32-close to the twin on every kind: the bounds of the GPU tests are finite and small
    for t, what in ((0, "verts"), (1, "joints")):
        b = D.kind_bounds([r[t] for r in refs], want[t], kinds)
        print(f"({V},{J},{NB}) pose2rot={pose2rot} {what}: bounds " + "  ".join(f"{k} {x:.2e}" for k, x in b.items()))
        assert all(x < 1e-3 for x in b.values()), b


def test_rigid_f64_is_the_twins_chain():
    P, betas, pose, _ = _case(97, 24, 10)
    _, Gt, S = ST.forward(betas, pose, P, keep=True)
    GR, Gt2, At = D.rigid_f64(S["R"], S["Jr"], P["parents"])
    assert np.array_equal(GR, S["GR"]) and np.array_equal(Gt2, Gt) and np.array_equal(Gt2, S["Gt"])
    assert np.array_equal(At, Gt - np.einsum("bjrc,bjc->bjr", S["GR"], S["Jr"]))


def _central_differences(P, betas, pose, gv, gp, pose2rot, seed):
    """tests/test_smpl_grad_cpu.py's convention: h = 1e-5, every beta and (up to) 40 pose entries, error relative to the gradient's largest entry."""
    d_betas, d_pose = ST.adjoint(betas, pose, P, gv, gp, pose2rot)
    assert d_betas.shape == betas.shape and d_pose.shape == pose.shape and np.isfinite(d_betas).all() and np.isfinite(d_pose).all()

    def loss(b, p):
        v, j = ST.forward(b, p, P, pose2rot)
        return (v * gv).sum() + (j * gp).sum()

    h, rng, worst = 1e-5, np.random.default_rng(seed), 0.0
    for which, x, grad, idx in (("b", betas, d_betas, range(betas.size)), ("p", pose, d_pose, rng.choice(pose.size, min(40, pose.size), replace=False))):
        for i in idx:
            plus, minus = x.copy(), x.copy()
            plus.reshape(-1)[i] += h
            minus.reshape(-1)[i] -= h
            cd = (loss(plus, pose) - loss(minus, pose)) / (2 * h) if which == "b" else (loss(betas, plus) - loss(betas, minus)) / (2 * h)
            worst = max(worst, abs(cd - grad.reshape(-1)[i]) / np.abs(grad).max())
    return worst


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("V,J,NB", [s for s in D.SHAPES if D.in_fast_domain(s[1], s[2])])
def test_twin_adjoint_equals_central_differences_on_every_kind(V, J, NB, kind):
    """The three frames of one kind (the loss is a sum over frames: a kind's gradient does not see the others), float64 throughout, step 1e-5 and
    tolerance 1e-8 of the gradient's largest entry as tests/test_smpl_grad_cpu.py has them at baseline poses.  lbs() is smooth in the pose through
    0 (sin a / a and (1 - cos a) / a^2 are functions of a^2 = |theta + 1e-8|^2), periodic in the angle and of bounded derivatives at any angle, so
    the truncation term h^2 f''' / 6 ~ 1e-11 and the quotient's rounding eps |L| / h ~ 1e-9 hold for every kind."""
    P, betas, pose, kinds = _case(V, J, NB)
    f = [i for i, k in enumerate(kinds) if k == kind]
    rng = np.random.default_rng(7)
    gv, gp = rng.standard_normal((3, V, 3)), rng.standard_normal((3, J, 3))
    worst = _central_differences(P, betas[f].astype(np.float64), pose[f].astype(np.float64), gv, gp, True, seed=3)
    print(f"({V},{J},{NB}) {kind}: central differences vs the twin's adjoint, relative: {worst:.3g}")
    assert worst <= 1e-8


@pytest.mark.parametrize("broadcast", [False, True])
def test_twin_adjoint_equals_central_differences_on_rotation_matrices_of_every_kind(broadcast):
    """pose2rot = False on the float32-rounded rotations of one frame per kind, with and without a broadcast betas row."""
    P, betas, pose, kinds = _case(130, 5, 16)
    b, p, _ = D.one_frame_per_kind(betas, pose, kinds)
    rng = np.random.default_rng(8)
    gv, gp = rng.standard_normal((11, 130, 3)), rng.standard_normal((11, 5, 3))
    worst = _central_differences(P, (b[:1] if broadcast else b).astype(np.float64), D.rot_input(p, 5).astype(np.float64), gv, gp, False, seed=4)
    print(f"rotation matrices, broadcast={broadcast}: central differences vs the twin's adjoint, relative: {worst:.3g}")
    assert worst <= 1e-8


# ------------------------------------------------------------------------------------------------------------------------- the comparison
def test_comparison_rejects_an_offset_of_ten_baseline_errors_on_one_kind(capsys):
    """What a subtly wrong kernel would look like to the GPU tests, shown without one: the float64 result itself passes; the fp32 restatements
    pass (they define the bound); the float64 result with 10 x e_baseline added to the verts of ONE kind's frames is rejected, on that kind only --
    also where the kind's own fp32 error is exactly zero (`zeros`, Rodrigues) and the baseline alone sets the bound."""
    P, betas, pose, kinds = _case(97, 24, 10)
    want, refs = D.forward_refs(P, betas, pose, True)
    rv = [r[0] for r in refs]
    e = D.kind_errors(refs[0][0], want[0], kinds)
    e2 = D.kind_errors(refs[1][0], want[0], kinds)
    e_base = max(e["baseline"], e2["baseline"])
    assert 1e-8 < e_base < 5e-6                                              # fp32 on coordinates of order 1
    assert D.parity("verts", want[0], want[0], rv, kinds) == []
    assert D.parity("verts", refs[0][0], want[0], rv, kinds) == [] and D.parity("verts", refs[1][0], want[0], rv, kinds) == []
    bounds = D.kind_bounds(rv, want[0], kinds)
    assert all(b >= 3 * e_base for b in bounds.values()) and bounds["baseline"] == 3 * e_base
    rejected = []
    for kind in D.KINDS:
        bad = want[0].copy()
        rows = [i for i, k in enumerate(kinds) if k == kind]
        bad[rows[1]] += 10 * e_base
        fails = D.parity("verts", bad, want[0], rv, kinds)
        # rejected on that kind and no other, unless fp32 itself loses more than 10 / 3 baselines there (the bound is 3 e_kind)
        assert [f[1] for f in fails] == ([kind] if 3 * max(e[kind], e2[kind]) < 10 * e_base * (1 - 1e-6) else [])
        rejected += [f[1] for f in fails]
    assert set(rejected) >= {"baseline", "zeros", "tiny", "small", "single_axis"} and len(rejected) >= 6, rejected
    one = want[0].copy()
    one[4, 50, 1] += 10 * e_base                                             # a single coordinate of a single vertex is enough
    assert [f[1] for f in D.parity("verts", one, want[0], rv, kinds)] == ["zeros"]
    nan = want[0].copy()
    nan[28, 0, 0] = np.nan                                                   # and a NaN is an error, not a comparison that is silently False
    assert [f[1] for f in D.parity("verts", nan, want[0], rv, kinds)] == ["large"]
    assert capsys.readouterr().out.count("[parity] verts") == 3 + 11 + 2
    # Rodrigues alone: on `zeros` the restatement's error is exactly 0, the bound is the baseline's plus half an ulp of 1
    from oracle import lbs_oracle
    R64 = ST.rodrigues(pose.reshape(-1, 3))[0].reshape(33, 24, 3, 3)
    R32 = lbs_oracle.batch_rodrigues(pose.reshape(-1, 3)).reshape(33, 24, 3, 3)
    er = D.kind_errors(R32, R64, kinds)
    assert er["zeros"] == 0.0 and er["baseline"] > 0
    br = D.kind_bounds([R32], R64, kinds, extra=2.0 ** -24)
    assert br["zeros"] == 3 * er["baseline"] + 2.0 ** -24
    # the whole-tensor form (d_betas of a broadcast row)
    w = np.arange(1.0, 11.0)[None]
    assert D.parity_whole("d_betas", w + 2e-7, w, [w + 1e-7]) == [] and D.parity_whole("d_betas", w + 4e-7, w, [w + 1e-7]) != []
    assert D.parity_whole("d_betas", w * np.nan, w, [w + 1e-7]) != []

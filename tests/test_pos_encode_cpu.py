"""The float64 yardstick of the positional encoder's forward (tests/refine_grad_twin.py: pe_forward, pe_forward_bound) tied to what the suite
already trusts: oracle.refine_oracle.positional_encoding, the fp32 numpy restatement of the reference (ball query included), lies within the
derived bound of the twin fed with the oracle's own ball-query indices, and agrees with it bit for bit where every sum is exact.  The sizes
are those of tests/test_pos_encode_gpu.py: P = 259 queries, so that P * S is no multiple of 64 for S <= 32."""
import numpy as np
import pytest

import refine_grad_twin as TW
from oracle import pointnet2_oracle as K
from oracle import refine_oracle as RO


def oracle_forward(c, radius):
    """(oracle output (F,P,32) fp32, the ball-query indices it grouped with)."""
    sd = {"pe.0.weight": c["W1"], "pe.0.bias": c["b1"], "pe.2.weight": c["W2"], "pe.2.bias": c["b2"]}
    feats_cm = None if c["extra"] is None else np.ascontiguousarray(np.transpose(c["extra"], (0, 2, 1)))
    out = RO.positional_encoding(sd, "pe", radius, c["S"], c["xyz"], c["new_xyz"], feats_cm)
    return out, K.ball_query(radius, c["S"], c["xyz"], c["new_xyz"])


@pytest.mark.parametrize("S", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("E", [0, 1, 3, 5])
def test_oracle_within_the_bound_of_the_twin(S, E):
    c = TW.pe_case(300 + S + 7 * E, 2, 301, 259, S, E, False)
    assert (259 * S) % 64 != 0 or S == 64
    got, idx = oracle_forward(c, 0.9)
    nh = (idx != idx[..., :1]).sum(-1) + 1                       # distinct hits per query (copies of the first hit pad the row)
    assert nh.min() < S and (nh.max() == S or S == 64) and nh.max() > S // 2, "the radius must give both padded and full rows"
    c["idx"] = idx
    ref, bnd = TW.pe_twin(c)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"oracle S={S} E={E}: worst err / bound = {float((err / bnd).max()):.4f}")
    assert got.dtype == np.float32 and (bnd > 0).all()
    assert not (err > bnd).any(), f"{int((err > bnd).sum())} of {err.size} elements beyond the derived bound"


@pytest.mark.parametrize("S", [4, 32])
@pytest.mark.parametrize("E", [0, 3, 5])
def test_oracle_equals_the_twin_where_every_sum_is_exact(S, E):
    c = TW.pe_exact_case(400 + S + 7 * E, 2, 301, 259, S, E, False)
    got, idx = oracle_forward(c, 1.2 if S == 4 else 2.5)         # integer lattice: squared distances <= 1 | <= 6
    nh = (idx != idx[..., :1]).sum(-1) + 1
    assert (nh < S).any() and (nh > 1).any() and nh.max() == S, "the radius must give both padded and full rows"
    c["idx"] = idx
    want = TW.pe_exact_expected(c)
    assert np.array_equal(got.astype(np.float64), want)


def test_bound_is_the_documented_formula():
    """pe_forward_bound against its one-line statement, and the unmasked hA_full against the masked hA the gradients use."""
    c = TW.pe_case(9, 2, 50, 37, 8, 3, False)
    fw = TW.pe_forward(c["xyz"], c["new_xyz"], c["extra"], None, c["idx"], c["W1"], c["b1"], c["W2"], c["b2"])
    hA = np.abs(fw["inp"]) @ np.abs(c["W1"].astype(np.float64)).T + np.abs(c["b1"].astype(np.float64))
    assert np.array_equal(fw["hA_full"], hA) and np.array_equal(fw["hA"], hA * (fw["z1"] > 0)) and (fw["hA"] != hA).any()
    want = ((32 + 6 + 5) * TW.U * (hA @ np.abs(c["W2"].astype(np.float64)).T)).max(2) + TW.U * (np.abs(fw["out"]) + np.abs(c["b2"].astype(np.float64)))
    np.testing.assert_allclose(TW.pe_forward_bound(fw, c["W2"], c["b2"]), want, rtol=1e-12)
    t, terr = TW.table_forward(c["extra"], c["W1"][:, 3:], c["b1"])
    assert t.shape == terr.shape == (2, 50, 32) and (terr > 0).all()
    wider = TW.pe_forward_bound(fw, c["W2"], c["b2"], table_err=terr)
    assert (wider > want).all()

"""The oracle's `off` mode against what the reference's own kernel source computed: tests/golden/ops_ref_hip_off.npz is the output
of the reference build (the reference's pointnet2 kernel files compiled for gfx950 with -O2 -ffp-contract=off) recorded on an
MI355X by scripts/dump_ref_kernels.py -- generator arguments and outputs only.  The inputs are regenerated here, so the pin of
oracle/g4d_oracle.c holds on any machine, with or without oracle/_ref/ (tests/test_ref_kernels_gpu.py is the live comparison)."""
import json
import os

import numpy as np
import pytest

import ref_kernel_cases as RC
from oracle import pointnet2_oracle as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = os.path.join(ROOT, "tests", "golden", "ops_ref_hip_off.npz")

pytestmark = pytest.mark.skipif(not os.path.exists(PIN), reason="tests/golden/ops_ref_hip_off.npz not recorded (run scripts/dump_ref_kernels.py "
                                                                "on an MI355X with oracle/_ref/ built)")


@pytest.fixture(scope="module")
def pin():
    return np.load(PIN)


@pytest.fixture(autouse=True)
def off_mode():
    prev = K.set_contraction("off")
    yield
    K.set_contraction(prev)


def _recorded(pin):
    keys = sorted(k for k in pin.files if k.startswith("case_"))
    return [(k[5:], json.loads(str(pin[k]))) for k in keys]


def test_fixture_holds_the_cases_this_tree_names(pin):
    """The file records exactly the fixture subset of tests/ref_kernel_cases.py, each op of it, and nothing but arguments and outputs."""
    got = [c for _, c in _recorded(pin)]
    assert got == json.loads(json.dumps(RC.fixture_cases()))
    assert {c["op"] for c in got} == {"fps", "ball", "nn"}
    assert {c["special"] for c in got if c["op"] == "fps"} == {"", "nan_point", "inf_coord"}
    assert max(c["n"] for c in got if c["op"] == "fps") == RC.FIXTURE_MAX_N
    assert os.path.getsize(PIN) < 200 * 1024


def test_block_size_choice_matches_the_recorded_one(pin):
    want = pin["block_size"].astype(np.int64)
    assert want.shape == (RC.BLOCK_SIZE_MAX_N,)
    got = np.array([K.block_size(n) for n in range(1, RC.BLOCK_SIZE_MAX_N + 1)])
    assert np.array_equal(got, want), f"first mismatch at n = {1 + int(np.argmax(got != want))}"


def test_oracle_off_mode_reproduces_the_reference_build(pin):
    """Every recorded output, bit for bit."""
    mod = K.as_pointnet2_cuda_module()
    bad = []
    for tag, case in _recorded(pin):
        for name, got in RC.fixture_outputs(case, mod, "cpu").items():
            want = pin[f"out_{tag}_{name}"]
            if not RC.same(got, want):
                bad.append(f"{RC.case_id(case)} {name}: {RC.first_diff(want, got)}")
    assert not bad, "\n".join(bad)


def test_oracle_other_modes_are_told_apart_by_the_fixture(pin):
    """The fixture is not blind to the rounding of the squared distance: in `nvcc` and `chain` mode the oracle does NOT reproduce it
    (some min-distance of some FPS case differs in its last bit)."""
    mod = K.as_pointnet2_cuda_module()
    for mode in ("nvcc", "chain"):
        K.set_contraction(mode)
        differs = False
        for tag, case in _recorded(pin):
            if case["op"] == "fps" and case["n"] >= 255 and not differs:
                differs = not RC.same(RC.fixture_outputs(case, mod, "cpu")["temp"], pin[f"out_{tag}_temp"])
        assert differs, mode

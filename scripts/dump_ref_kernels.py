"""Record what the reference build computes: tests/golden/ops_ref_hip_off.npz.

Runs on the GPU.  The reference build (oracle/_ref/libpointnet2_ref.so: the reference's own pointnet2 kernel files compiled for
gfx950 with -O2 -ffp-contract=off, `make -C oracle ref`) is run on the fixture subset of tests/ref_kernel_cases.py -- FPS idx and
temp, ball-query idx, three_nn dist2 and idx, clouds of at most 1025 points -- and on opt_n_threads(n) for n = 1..40000.  The file
holds the generator arguments of each case (json) and the outputs; no cloud, no code.  tests/test_ref_kernels_cpu.py regenerates
the inputs and holds the oracle's `off` mode to the file on any machine.

    python scripts/dump_ref_kernels.py [--out tests/golden/ops_ref_hip_off.npz]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ops_ref_hip_off.npz"))
    args = ap.parse_args()
    import torch
    import ref_kernel_cases as RC
    from oracle import ref_pointnet2 as REF
    if not REF.available():
        sys.exit(f"{REF.LIB_PATH} is missing: run `G4D_REFERENCE_DIR=<checkout of the reference> make -C oracle ref` first")
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: the reference build is gfx950 code")
    out = {"meta": np.array(json.dumps({"build": "hipcc --offload-arch=gfx950 -O2 -ffp-contract=off", "device": torch.cuda.get_device_name(0),
                                        "nn_rows": RC.FIXTURE_NN_ROWS}))}
    out["block_size"] = np.array([REF.opt_n_threads(n) for n in range(1, RC.BLOCK_SIZE_MAX_N + 1)], dtype=np.int16)
    cases = RC.fixture_cases()
    for i, case in enumerate(cases):
        out[f"case_{i:03d}"] = np.array(RC.case_key(case))
        for name, a in RC.fixture_outputs(case, REF, "cuda").items():
            out[f"out_{i:03d}_{name}"] = a
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(cases)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()

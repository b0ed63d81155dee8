"""Forward + backward of each cfg2 level's shared MLP in training mode (batch-statistics BatchNorm), with the max-pool for the SA levels:
Tuning.mlp_autograd on (csrc/bn_train.hip + the existing contraction kernels, on rows) against off (torch's Conv2d / BatchNorm2d / ReLU /
max_pool2d on MIOpen, what every grad-enabled call ran before the flag).  Device events around each step, median after warm-up, the two
routes alternating step by step; with --launches also the per-entry-point times of one flag-on step (_lib.timed_calls).  Needs a GPU.

What a step is: the level's SharedMLP (+ pool) on an already grouped / interpolated random tensor (B, Cin, npoint, nsample), NOT the whole
module -- sampling, query, grouping and interpolation are the same kernels on both routes and are left out.  Flag on, an SA level runs the
functions the module's forward calls (to_rows -> run_blocks -> pool_rows_max -> to_channels), one scale at a time; an FP level and the
flag-off route call the SharedMLP.  The input requires grad (the first layer's dX is computed) except at SA 1, whose grouped input holds
coordinates only, as in the encoder.

    python scripts/time_mlp_train.py [--warmup 10] [--steps 30] [--launches]

One JSON line per level: {"level", "rows", "spec", "on_ms", "off_ms", "on_over_off"}."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garment4d_amd import _lib, mlp_train, tuning   # noqa: E402
from garment4d_amd import pytorch_utils as PT        # noqa: E402
from garment4d_amd.encoder import seed_encoder       # noqa: E402

B = 8
# cfg2 = Pointnet2MSGSEG(input_channels=0) on B = 8 clouds of 8192 points: (level, npoint, nsample, SharedMLP spec); nsample 0: an FP level
LEVELS = [("SA1.0", 1024, 16, [3, 16, 16, 32]), ("SA1.1", 1024, 32, [3, 32, 32, 64]),
          ("SA2.0", 256, 16, [99, 32, 32, 64]), ("SA2.1", 256, 32, [99, 64, 64, 128]),
          ("SA3.0", 64, 32, [195, 64, 64, 128]), ("SA3.1", 64, 64, [195, 128, 128, 256]),
          ("FP3", 256, 0, [576, 512, 256]), ("FP2", 1024, 0, [352, 256, 128]), ("FP1", 8192, 0, [128, 128, 64])]


def step(mlp, x, S, g, flag):
    if x.requires_grad:
        x.grad = None
    mlp.zero_grad(set_to_none=True)
    with tuning.use(tuning.current().replace(mlp_autograd=flag)):
        if flag and S:
            out = mlp_train.to_channels(mlp_train.pool_rows_max([mlp_train.run_blocks(mlp_train.plain_stack(mlp), mlp_train.to_rows(x))], [S]), B)
        else:
            out = mlp(x)
            out = F.max_pool2d(out, kernel_size=[1, S]).squeeze(-1) if S else out.squeeze(-1)
        out.backward(g)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mlp_train.py measures on the GPU; there is no CPU fallback"
    for name, npoint, S, spec in LEVELS:
        torch.manual_seed(0)
        mlp = seed_encoder(PT.SharedMLP(list(spec), bn=True), seed=1).cuda().train()
        x = torch.randn(B, spec[0], npoint, max(S, 1), device="cuda", requires_grad=spec[0] != 3)   # SA 1 groups coordinates only: no dX there
        g = torch.randn(B, spec[-1], npoint, device="cuda")
        times = {True: [], False: []}
        for i in range(args.warmup + args.steps):
            for flag in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(mlp, x, S, g, flag)
                e1.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[flag].append(e0.elapsed_time(e1))
        on_ms, off_ms = statistics.median(times[True]), statistics.median(times[False])
        print(json.dumps({"level": name, "rows": B * npoint * max(S, 1), "spec": spec, "on_ms": round(on_ms, 4), "off_ms": round(off_ms, 4),
                          "on_over_off": round(on_ms / off_ms, 3)}), flush=True)
        if args.launches:
            with _lib.timed_calls() as t:
                step(mlp, x, S, g, True)
            agg = {}
            for entry, _, us in t.results():
                agg[entry] = agg.get(entry, 0.0) + us
            print(json.dumps({"level": name, "launch_us": {k: round(v, 1) for k, v in sorted(agg.items(), key=lambda kv: -kv[1])}}), flush=True)


if __name__ == "__main__":
    main()

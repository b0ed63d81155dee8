"""Partially filled calls of the executor (garment4d_amd/pipeline.py): a captured graph is replayed on fewer clouds than it was captured for
through the live-cloud scope (include/g4d_live.h) -- the slot's device-side count is rewritten ahead of every launch.  The steps of a call
that was launched before it was full must get, bit for bit, what the same steps get (a) from the eager call on one step, (b) inside a full
call and (c) from an executor whose `coalesce` is the number of steps submitted; and a full call on a slot that has just run a partial one
must be complete again.  With the graph and with use_graph=False (where a partial call is made on the filled clouds themselves)."""
import pytest
import torch

from garment4d_amd import lbs as L
from garment4d_amd import synthetic as syn
from garment4d_amd.encoder import Pointnet2MSGSEG, seed_encoder
from garment4d_amd.pipeline import StepPipeline

pytestmark = pytest.mark.gpu

B, N, K = 2, 4096, 3


@pytest.fixture(scope="module")
def world():
    """The model, 6 steps of inputs and, per step, the eager call's results (computed once, shared by both cases, never modified)."""
    model = seed_encoder(Pointnet2MSGSEG(input_channels=0, global_feat=False), seed=0).cuda().eval()
    smpl = {k: torch.from_numpy(v).cuda() for k, v in syn.smpl_like_params(seed=1).items()}
    nstep = 6
    clouds = torch.from_numpy(syn.unit_cloud(nstep * B, N, seed=21)).cuda().view(nstep, B, N, 3)
    betas, pose = (torch.from_numpy(a).cuda() for a in syn.smpl_like_pose(nstep * B, seed=9))
    steps = [(clouds[i].contiguous(), betas[i * B:(i + 1) * B].contiguous(), pose[i * B:(i + 1) * B].contiguous()) for i in range(nstep)]
    ref = []
    with torch.no_grad():
        for c, b, p in steps:
            logits = model.forward_fused(c, precision="fp32")[1]
            v, j = L.lbs(b, p, smpl["v_template"], smpl["shapedirs"], smpl["posedirs"], smpl["J_regressor"], smpl["parents"], smpl["lbs_weights"])
            ref.append((logits.clone(), v.clone(), j.clone()))
    return model, smpl, steps, ref


def _same(got, want, what):
    for name, g, w in zip(("sem_logits", "verts", "joints"), got, want):
        assert g.shape == w.shape and torch.equal(g, w), f"{what}: {name} differs"


@pytest.mark.parametrize("use_graph", [True, False])
def test_partially_filled_calls_are_exact_and_the_count_is_rewritten(world, use_graph):
    model, smpl, steps, ref = world
    pipe = StepPipeline(model, smpl, clouds_per_step=B, n_points=N, coalesce=K, streams=2, use_graph=use_graph)
    s0, s1 = pipe.slots
    # a full call on slot 0: the steps inside a full call
    futs = [pipe.submit(*steps[i]) for i in range(K)]
    assert s0.launched_gen == 1 and pipe.slots[pipe._cur] is s1
    full = [f.result(copy=True) for f in futs]
    for i in range(K):
        _same(full[i], ref[i], f"step {i} of a full call")
    # 1 of 3 steps on slot 1, launched by result()
    f = pipe.submit(*steps[3])
    assert s1.launched_gen == 0 and s1.fill == 1
    _same(f.result(copy=True), ref[3], "1 step of 3")
    assert s1.launched_gen == 1 and s1.fill == 0 and pipe.slots[pipe._cur] is s0
    if use_graph:
        assert int(s1.live) == 1 * B and int(s0.live) == K * B
    # 2 of 3 steps on slot 0, launched by flush(); other inputs than the slot's full call before
    fa, fb = pipe.submit(*steps[4]), pipe.submit(*steps[5])
    pipe.flush()
    _same(fa.result(copy=True), ref[4], "step 1 of 2 of 3")
    _same(fb.result(copy=True), ref[5], "step 2 of 2 of 3")
    if use_graph:
        assert int(s0.live) == 2 * B
    # a full call on slot 1, which ran the 1-step call last: every step is computed again
    futs = [pipe.submit(*steps[i]) for i in (5, 0, 4)]
    assert s1.launched_gen == 2
    for f, i in zip(futs, (5, 0, 4)):
        _same(f.result(copy=True), ref[i], f"step {i} of a full call after a partial one")
    if use_graph:
        assert int(s1.live) == K * B
    # ... and through synchronize(), with one step pending on slot 0
    f = pipe.submit(*steps[1])
    pipe.synchronize()
    _same(f.result(copy=True), ref[1], "1 step of 3, launched by synchronize()")
    # an executor whose coalesce is the number of steps submitted gives the same bits
    for nsub in (1, 2):
        small = StepPipeline(model, smpl, clouds_per_step=B, n_points=N, coalesce=nsub, streams=1, use_graph=use_graph)
        futs = [small.submit(*steps[3 + i]) for i in range(nsub)]
        part = [pipe.submit(*steps[3 + i]) for i in range(nsub)]
        for i in range(nsub):
            a, b = futs[i].result(copy=True), part[i].result(copy=True)
            _same(b, a, f"step {i} of {nsub} submitted against coalesce = {nsub}")
            _same(a, ref[3 + i], f"coalesce = {nsub}")


def test_dropin_encoder_call_route_takes_the_scope(world):
    """The reference's call form `model(pc)` as the executor's encoder_call: the same partially filled replay, the same bits."""
    model, smpl, steps, ref = world
    pipe = StepPipeline(model, smpl, clouds_per_step=B, n_points=N, coalesce=K, streams=1, encoder_call=lambda m, pc: m(pc)[1])
    fa, fb = pipe.submit(*steps[0]), pipe.submit(*steps[1])
    _same(fb.result(copy=True), ref[1], "drop-in route, step 2 of 2 of 3")
    _same(fa.result(copy=True), ref[0], "drop-in route, step 1 of 2 of 3")
    futs = [pipe.submit(*steps[i]) for i in (2, 3, 4)]
    for f, i in zip(futs, (2, 3, 4)):
        _same(f.result(copy=True), ref[i], f"drop-in route, step {i} of a full call after a partial one")

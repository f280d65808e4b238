"""GPU (run with `-m gpu`): occupancy votes and stat update off the training step's main queue (ExpRunner.votes_off_main).

Step level: training steps with the votes (f2n_oct_mark_visit) and the stat update (f2n_oct_update_stats_ex) on the tail stream,
behind f2n_early_stop + f2n_segment_scan_ex on the main queue, against the fused launches on the main queue (f2n_early_stop_votes,
f2n_oct_update_stats_scan).  The votes are integer maxima and the stat update is per node, so nothing may differ: every comparison
is of bytes.  (The kernels themselves are held against each other in tests/test_gpu_parity.py: the fused launches equal the
separate ones bit for bit.)

Kernel level: f2n_compact_samples_src with o_anchors = NULL, which the streaming training step now passes -- every other output as
with the array, and nothing written where the array would have been.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_parity import DEV, F32, N, T, assert_same, ragged  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    runtime.host()
    return runtime


@pytest.mark.parametrize("n_rays", [1, 3, 4, 5, 700])  # four rays per block: one block, its edge, a partial block, many blocks
def test_compaction_without_the_anchor_array(hip, n_rays):
    """o_anchors = NULL: o_pts, o_dirs, o_dt, o_t, o_src, o_vol and o_ray_val are the bytes of the call that is given the array.
    Rays of 0 .. 150 samples (more than one 64-lane pass per ray), a mask that is not a prefix."""
    rng = np.random.default_rng(40 + n_rays)
    se, n = ragged(rng, n_rays, 150)
    n_real, n = n, max(n, 1)
    mask_np = (rng.random(n) < 0.6).astype(np.int32)
    mask_np[n_real:] = 0  # (the filler sample of a batch without samples belongs to no ray)
    kept = np.array([mask_np[s:e].sum() for s, e in se], np.int32)
    ends = np.cumsum(kept)
    new_se = T(np.stack([ends - kept, ends], 1).astype(np.int32))
    m = max(int(ends[-1]), 1)
    pts, dirs = rng.random((n, 3), dtype=F32), rng.random((n, 3), dtype=F32)
    dt, t = rng.random(n, dtype=F32), rng.random(n, dtype=F32)
    anchors = rng.integers(0, 1000, (n, 3)).astype(np.int32)
    ray_val = T(rng.integers(0, 50, n_rays).astype(np.int32))
    outs = []
    for with_anchors in (True, False):
        o = [torch.full((m, 3), -7.0, device=DEV), torch.full((m, 3), -7.0, device=DEV), torch.full((m,), -7.0, device=DEV),
             torch.full((m,), -7.0, device=DEV)]
        oa = torch.full((m, 3), -7, dtype=torch.int32, device=DEV) if with_anchors else None
        src, vol, rv = (torch.full((m,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
        hip.compact_samples_src(n_rays, T(se), new_se, T(mask_np), T(pts), T(dirs), T(dt), T(t), T(anchors), *o, oa, src, vol, ray_val, rv)
        torch.cuda.synchronize()
        outs.append([N(x) for x in o + [src, vol, rv]] + [N(oa) if with_anchors else None])
    for k, name in enumerate(("o_pts", "o_dirs", "o_dt", "o_t", "o_src", "o_vol", "o_ray_val")):
        assert_same(outs[1][k], outs[0][k], "%d rays: %s" % (n_rays, name))
    live = int(ends[-1])
    assert_same(outs[0][7][:live], anchors[mask_np != 0], "o_anchors of the call that has it")
    assert_same(outs[0][5][:live], outs[0][7][:live, 0], "o_vol = column 0 of the anchors")


def run_steps(rt, st, batches, knob, speculative):
    runner, cfg, _ = rt.make_runner(st, "wanjinyou", [], seed=2022, device="cuda:0")
    torch.manual_seed(2022)
    runner.votes_off_main = knob
    if speculative:
        runner.speculative_sampling, runner.speculation_depth = True, 3
    losses = []
    for i in range(5):
        b, nb, nb2 = batches[i], batches[i + 1], batches[i + 2]
        if runner.speculation_depth >= 2:  # (prefetch arguments as bench.py passes them)
            s = runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2], nb2[0], nb2[1])
        else:
            s = runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2])
        losses.append(float(s["loss"]))
    runner.flush()
    states = [t.detach().cpu().contiguous().numpy().tobytes() for t in runner.states()]
    nodes = runner.tree_nodes().cpu().numpy().tobytes()
    occ = [t.cpu().numpy().tobytes() for t in runner.occupancy_buffers()]
    out = dict(states=states, nodes=nodes, occ=occ, losses=losses, spec=dict(runner.speculation_counters()), taken=int(runner.votes_off_main_steps))
    del runner
    return out


@pytest.fixture(scope="module")
def batches(rt, fox_state):
    rng = np.random.default_rng(5)
    return [rt.to_dev(*rt.synthetic_ray_batch(fox_state, 512, rng)) for _ in range(7)]


@pytest.mark.parametrize("speculative", [False, True], ids=["default", "two_deep"])
def test_train_steps_are_bit_identical_with_votes_off_and_on_the_main_queue(rt, fox_state, batches, speculative):
    """Two runners from one seed, ExpRunner.votes_off_main 1 and 0, five streaming steps at 512 rays on the fox state: equal bytes of
    every state tensor (octree nodes, table, both MLPs, embeddings, visit counts), of the node array and the occupancy statistics, equal
    losses, equal speculation counters.  Once more with speculative sampling on at depth 3: the two-deep route with the knob forced
    to 1.  Iteration 0 is a maintenance iteration and keeps the fused launches; the four behind it take the new route."""
    tail = run_steps(rt, fox_state, batches, 1, speculative)
    fused = run_steps(rt, fox_state, batches, 0, speculative)
    print("votes_off_main steps taken:", tail["taken"], "of 5; losses", tail["losses"], "speculation", tail["spec"])
    assert fused["taken"] == 0 and tail["taken"] == 4, (fused["taken"], tail["taken"])
    assert tail["losses"] == fused["losses"] and all(x == x for x in tail["losses"])
    assert len(tail["states"]) == len(fused["states"])
    for k, (a, b) in enumerate(zip(tail["states"], fused["states"])):
        assert a == b, "state tensor %d differs" % k
    assert tail["nodes"] == fused["nodes"], "octree nodes differ"
    assert tail["occ"] == fused["occ"], "occupancy statistics / visit counts differ"
    assert tail["spec"] == fused["spec"]


def test_knob_two_leaves_the_two_deep_regime_alone(rt, fox_state, batches):
    """votes_off_main = 2: eligible steps of the one-batch-ahead regime only -- with the batch after next begun two steps ahead
    (speculation_depth 3) no step takes the new route; without, the four steps behind the maintenance iteration do."""
    assert run_steps(rt, fox_state, batches, 2, True)["taken"] == 0
    assert run_steps(rt, fox_state, batches, 2, False)["taken"] == 4

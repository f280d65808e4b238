"""CPU: self-consistency of the oracle's host-pipeline restatement (oracle/pipeline.py): its hand-written
backward chains are checked against float64 torch autograd of the same formulas, and the MLP restatement
against a plain fp32 network."""
import os

import numpy as np
import pytest
import torch

from oracle import capi as oc
from oracle import pipeline as op

F32 = np.float32


def ragged(rng, R, hi=40):
    cnt = rng.integers(0, hi, R)
    cnt[::11] = 0
    end = np.cumsum(cnt)
    return np.stack([end - cnt, end], -1).astype(np.int32), int(end[-1])


def test_composite_backward_matches_autograd():
    rng = np.random.default_rng(1)
    R = 120
    se, n = ragged(rng, R)
    feat = rng.standard_normal((n, 16)).astype(F32); feat[:, 0] = feat[:, 0] + 2
    dt = (rng.random(n) * 0.03).astype(F32); t = (rng.random(n) * 5).astype(F32)
    rgb = rng.random((n, 3)).astype(F32); bg = rng.random((R, 3)).astype(F32)
    dcol = rng.standard_normal((R, 3)).astype(F32); ddisp = rng.standard_normal(R).astype(F32)
    ddep = (rng.standard_normal(R) * 0.1).astype(F32); dw = (rng.standard_normal(n) * 0.1).astype(F32)
    out = op.composite_fwd(feat, dt, t, rgb, bg, se, want_ctx=True)
    drgb, df0 = op.composite_bwd(out["ctx"], dt, rgb, bg, se, dcol, ddisp, ddep, dw, 1.0)
    # float64 autograd of the same maths
    f0 = torch.tensor(feat[:, 0], dtype=torch.float64, requires_grad=True)
    c = torch.tensor(rgb, dtype=torch.float64, requires_grad=True)
    loss = 0
    cols, disps, deps, ws = [], [], [], []
    for r in range(R):
        s, e = se[r]
        sig = torch.exp(f0[s:e] - 3); sec = sig * torch.tensor(dt[s:e], dtype=torch.float64)
        acc = torch.cumsum(sec, 0) - sec
        T = torch.exp(-acc); w = T * (1 - torch.exp(-sec)); last = torch.exp(-sec.sum())
        tt = torch.tensor(t[s:e], dtype=torch.float64) + 1e-2
        col = (w[:, None] * c[s:e]).sum(0) + last * torch.tensor(bg[r], dtype=torch.float64)
        loss = loss + (col * torch.tensor(dcol[r], dtype=torch.float64)).sum() + (w / tt).sum() * float(ddisp[r]) \
            + (w * tt).sum() / (1 - last + 1e-4) * float(ddep[r]) + (w * torch.tensor(dw[s:e], dtype=torch.float64)).sum()
        cols.append(col.detach().numpy())
    loss.backward()
    np.testing.assert_allclose(out["colors"], np.array(cols), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(drgb, c.grad.numpy(), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(df0, f0.grad.numpy(), rtol=2e-3, atol=2e-5)
    # gradient scaling only rescales per-sample gradients
    drgb2, df02 = op.composite_bwd(out["ctx"], dt, rgb, bg, se, dcol, ddisp, ddep, dw, 0.25)
    sc = oc.grad_scaling_bwd(np.ones(n, F32), se, 0.25)
    np.testing.assert_allclose(drgb2, drgb * sc[:, None], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(df02, df0 * sc, rtol=1e-5, atol=1e-9)


def _params(rng, n_hidden):
    n = oc.mlp_n_params(32, 64, n_hidden)
    return (rng.standard_normal(n) * 0.15).astype(F32)


def _torch_mlp(params, x, n_hidden):
    off, h = 0, x
    dims = [(64, 32)] + [(64, 64)] * (n_hidden - 1) + [(16, 64)]
    for li, (r, c) in enumerate(dims):
        h = h @ params[off:off + r * c].reshape(r, c).t()
        off += r * c
        if li < len(dims) - 1:
            h = torch.relu(h)
    return h


def test_mlp_restatement_close_to_fp32_network():
    rng = np.random.default_rng(2)
    for nh in (1, 2):
        p = _params(rng, nh)
        x = rng.standard_normal((300, 32)).astype(F32)
        out_h, acts = oc.mlp_fwd(p, x, 64, nh, want_acts=True)
        pt = torch.tensor(p, requires_grad=True); xt = torch.tensor(x, requires_grad=True)
        y = _torch_mlp(pt, xt, nh)
        np.testing.assert_allclose(oc.h2f(out_h), y.detach().numpy(), rtol=0, atol=2e-2)
        dy = (rng.standard_normal((300, 16)) * 1e-2).astype(F32)
        (y * torch.tensor(dy)).sum().backward()
        dp, dx, dxh = oc.mlp_bwd(p, x, acts, dy, 64, nh, 128.0)
        assert np.abs(dp - pt.grad.numpy()).max() <= 3e-2 * np.abs(pt.grad.numpy()).max()
        # fp16 activations flip a few ReLU masks relative to the fp32 network: rare elements move by a few percent
        edx = np.abs(dx - xt.grad.numpy())
        assert edx.max() <= 0.12 * np.abs(xt.grad.numpy()).max() and edx.mean() <= 2e-3 * np.abs(xt.grad.numpy()).max()
        np.testing.assert_array_equal(dxh, oc.f2h(dx * F32(128.)))


def test_shade_and_field_pipeline_shapes(fox_state, fox_golden):
    rng = np.random.default_rng(3)
    g = fox_golden
    n = 500
    grid = op.HashGrid((rng.standard_normal((16 << 10, 2)) * 0.5).astype(F32), fox_state["prim_pool"], fox_state["bias_pool"],
                       int(fox_state["n_volumes"]), 10)
    p1, p2 = _params(rng, 1), _params(rng, 2)
    feat, ctx = op.field_fwd(grid, p1, g["march_pts"][:n], g["march_anchors"][:n, 0], want_ctx=True)
    assert feat.shape == (n, 16)
    dparams, gtab, _ = op.field_bwd(grid, p1, ctx, (rng.standard_normal((n, 16)) * 1e-3).astype(F32))
    assert dparams.shape == (3072,) and gtab.shape == (grid.table_f32.size,)
    # only halves [0, 17 * 2^(log2-1)*... ) are addressed: the level-overlap quirk
    touched = np.nonzero(gtab)[0]
    assert touched.max() < 17 * (1 << 10)
    rgb, sctx = op.shade_fwd(p2, feat, g["march_dirs"][:n], want_ctx=True)
    assert rgb.shape == (n, 3) and (rgb > -1e-3 - 1e-6).all() and (rgb < 1 + 1e-3 + 1e-6).all()
    dp, dfeat, demb = op.shade_bwd(p2, sctx, (rng.standard_normal((n, 3)) * 1e-3).astype(F32))
    assert dp.shape == (7168,) and (dfeat[:, 0] == 0).all() and demb is None


def test_mlp_accumulator_readings_are_closer_than_the_parity_tolerance(fox_state, fox_golden):
    """The MLP rows of the oracle are "parity unpinned" (tiny-cuda-nn is not in the reference tree); what the published
    FullyFusedMLP contract leaves open in the FORWARD arithmetic is the accumulator of the matrix products.  The oracle's
    default is fp32 in k order; `mlp_accumulator(1)` is the other plausible reading of a WMMA kernel (binary16 accumulator
    fragment, rounded after every 16-wide k-block).  This measures how far the two are apart through density MLP -> colour
    MLP -> compositing on the golden march with trained-looking weights: well inside the 1e-3 RGB tolerance the GPU path is
    held to against the default reading, so that tolerance also covers the reading nobody can pin."""
    rng = np.random.default_rng(3)
    st, g = fox_state, fox_golden
    log2 = 14
    grid = op.HashGrid((rng.standard_normal((16 << log2, 2)) * 0.3).astype(F32), st["prim_pool"], st["bias_pool"],
                       int(st["n_volumes"]), log2)
    p1, p2 = _params(rng, 1), _params(rng, 2)
    se = g["march_pts_idx_bounds"]
    bg = np.zeros((len(se), 3), F32)
    out = {}
    for mode in (0, 1):
        with oc.mlp_accumulator(mode):
            feat = op.field_fwd(grid, p1, g["march_pts"], g["march_anchors"][:, 0])
            rgb = op.shade_fwd(p2, feat, g["march_dirs"])
            comp = op.composite_fwd(feat, g["march_dt"], g["march_t"], rgb, bg, se)
        out[mode] = (feat, rgb, comp["colors"])
    d_feat, d_rgb, d_col = (float(np.abs(out[0][k] - out[1][k]).max()) for k in range(3))
    assert 0.0 < d_feat <= 2e-3, d_feat   # the readings do differ (a few f16 ulps of the 16 field outputs) ...
    assert d_rgb <= 5e-4, d_rgb           # ... by < 2e-4 in a sample's colour (measured 1.8e-4)
    assert d_col <= 1e-4, d_col           # ... and by ~5e-6 in a composited ray colour


def test_early_stop_prefix_and_adam():
    rng = np.random.default_rng(4)
    se, n = ragged(rng, 200, 80)
    f0 = (rng.standard_normal(n) * 2 + 4).astype(F32); dt = (rng.random(n) * 0.05).astype(F32)
    w, a, mask, nse = op.early_stop(f0, dt, se)
    for s, e in se:  # the kept set of every ray is a prefix (T is non-increasing)
        m = mask[s:e]
        assert (np.diff(m) <= 0).all()
    assert nse[-1, 1] == mask.sum()
    p = rng.standard_normal(1000).astype(F32); g = (rng.standard_normal(1000) * 1e-3).astype(F32)
    pt = torch.tensor(p.copy(), requires_grad=True)
    opt = torch.optim.Adam([pt], lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=1e-6)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step in range(1, 4):
        pt.grad = torch.tensor(g)
        opt.step()
        p, m, v = op.adam_step(p, g, m, v, step, 1e-2, 0.9, 0.99, 1e-15, 1e-6)
        np.testing.assert_allclose(p, pt.detach().numpy(), rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("name", ["wanjinyou", "wanjinyou_big", "llff", "nerf-360", "free"])
def test_presets_equal_the_reference_config_files(name, tmp_path):
    """config.PRESETS / GROUP_DEFAULTS are data copied by hand from the reference's confs/: here they are tied to those files,
    composed hydra-style by config.compose_yaml and recorded in tests/golden/reference_confs.json (tests/golden/make_confs.py)."""
    import json
    import yaml
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_confs.json")) as f:
        want = json.load(f)[name]
    got = config.preset(name)
    def norm(flat):  # (PyYAML reads `1e-1` as a string; the C++ host parses the strings, so compare the values)
        out = {}
        for k, v in flat.items():
            parts = []
            for item in v.split(","):
                try:
                    parts.append(float(item))
                except ValueError:
                    parts.append(item)
            out[k] = parts
        return out
    for group in ("train", "dataset", "renderer", "pts_sampler", "field", "shader"):
        assert norm(config.flatten({group: want[group]})) == norm(config.flatten({group: got[group]})), (name, group)
    assert want["mode"] == got["mode"] == "train" and want["is_continue"] == got["is_continue"]
    # the launcher's argument handling (scripts/run.py's hydra overrides), on a confs/ directory laid out as the reference's:
    # one file per group under <group>/<option>.yaml, named by the experiment file's `defaults:` list
    groups = ("train", "dataset", "renderer", "pts_sampler", "field", "shader")
    root = {k: v for k, v in want.items() if k not in groups}
    root["defaults"] = [{g: name + "_" + g} for g in groups] + ["_self_"]
    for g in groups:
        (tmp_path / g).mkdir()
        (tmp_path / g / (name + "_" + g + ".yaml")).write_text(yaml.safe_dump(want[g]))
    (tmp_path / (name + ".yaml")).write_text(yaml.safe_dump(root))
    from f2_nerf_amd import run
    n, d, ov = run.parse_args(["--config-name=%s" % name, "--config-dir=%s" % tmp_path, "case_name=ngp_fox", "+work_dir=/tmp/x",
                               "train.end_iter=100"])
    cfg = config.compose_yaml(d, n, ov)
    assert {g: cfg[g] for g in groups if g != "train"} == {g: want[g] for g in groups if g != "train"}
    assert cfg["case_name"] == "ngp_fox" and cfg["work_dir"] == "/tmp/x" and cfg["train"]["end_iter"] == 100


def test_step_and_gradient_exchange_interleave_in_the_documented_order():
    """GradSyncPipeline (csrc/host/GradSyncPipeline.h) is the piece of ExpRunner::TrainStep that decides WHEN the data-parallel
    exchange, the optimiser and the next step's ray sampling run relative to each other.  It touches no device, so the host
    extension's own object is driven here with recording callbacks: blocking exchange, pipelined exchange (begin after
    backward, end + the PREVIOUS step's Adam with ITS learning rate behind the next step's sampling), the non-optimising step
    in pipelined mode, and flush."""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    host = runtime.host()
    log = []

    def make(pipelined, blocking):
        p = host.GradSyncPipeline()
        p.set_apply(lambda a, lr: log.append("adam(apply=%d, lr=%.3f)" % (a, lr)))
        p.set_defer_flags(lambda: log.append("defer_flags"))
        if blocking:
            p.set_blocking(lambda: log.append("allreduce"))
        if pipelined:
            p.set_begin_end(lambda: log.append("begin"), lambda: log.append("end"))
            p.pipelined = True
        return p

    def step(p, lr, apply=True):
        p.begin_step(apply, lambda: log.append("sample"))
        log.append("fwd_bwd")
        return p.gradients_ready(apply, lr)

    # no exchange at all (one GPU): nothing but the optimiser, nothing pending
    p = make(False, False)
    assert not p.installed() and step(p, 0.01) and not p.pending()
    assert log == ["fwd_bwd", "adam(apply=1, lr=0.010)"]
    # blocking exchange: in front of the optimiser, same step
    del log[:]
    p = make(False, True)
    assert p.installed() and step(p, 0.01) and step(p, 0.02, apply=False)
    assert log == ["fwd_bwd", "allreduce", "adam(apply=1, lr=0.010)", "fwd_bwd", "allreduce", "adam(apply=0, lr=0.020)"]
    # pipelined exchange
    del log[:]
    p = make(True, False)
    assert step(p, 0.01) is False and p.pending()
    assert log == ["sample", "fwd_bwd", "begin"]  # (the first step has nothing to wait for)
    del log[:]
    assert step(p, 0.02) is False
    # the next step's sampling is queued BEFORE the wait; the previous step is applied with the previous learning rate
    assert log == ["sample", "end", "adam(apply=1, lr=0.010)", "defer_flags", "fwd_bwd", "begin"]
    del log[:]
    p.finish_pending_step()  # flush (FinishPending / states() / render)
    p.finish_pending_step()
    assert log == ["end", "adam(apply=1, lr=0.020)", "defer_flags"] and not p.pending()
    # a step that does not apply the optimiser (tests, gradient inspection) never leaves an exchange in flight, first completes
    # the one that is -- and still exchanges its own gradients, begin / end back to back (round 6: every rank must issue the same
    # collectives whether or not the step applies; before, the table buckets its scatter reported went out without the rest)
    del log[:]
    assert step(p, 0.03) is False
    assert step(p, 0.04, apply=False) is True and not p.pending()
    assert log == ["sample", "fwd_bwd", "begin", "end", "adam(apply=1, lr=0.030)", "defer_flags", "fwd_bwd", "begin", "end", "adam(apply=0, lr=0.040)"]


def test_table_gradient_buckets_travel_in_order_and_the_exchange_sends_the_rest():
    """Bucketed table exchange (GradSyncPipeline::BucketReady, round 5): the scatter reports the finished ranges of the gradient table
    while the backward's last kernels run; range b's all-reduce starts at once, `begin` (or the blocking exchange) sends the buckets
    that were not reported -- all of them for a batch that took the small-batch path -- and then the flat small-gradient buffer.  The
    sequence of collectives a rank issues per step is therefore always b0 b1 b2 b3 flat, whatever its scatter did: pinned here with
    the host extension's own object; out-of-order or repeated buckets throw."""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    host = runtime.host()
    log = []
    N = 4
    p = host.GradSyncPipeline()
    p.set_apply(lambda a, lr: log.append("adam"))
    p.set_defer_flags(lambda: None)
    p.set_bucket(lambda b, n: log.append("allreduce(table bucket %d/%d)" % (b, n)))

    def begin():
        for b in range(p.buckets_sent, N):  # what DataParallel::GradSyncBegin does
            log.append("allreduce(table bucket %d/%d)" % (b, N))
        log.append("allreduce(flat)")
    p.set_begin_end(begin, lambda: log.append("wait"))
    p.pipelined = True
    want = ["allreduce(table bucket %d/%d)" % (b, N) for b in range(N)] + ["allreduce(flat)"]
    for reported in (4, 2, 0, 4):  # the scatter reported every bucket / two of them / none (small batch) / every one again
        del log[:]
        p.begin_step(True, lambda: None)
        for b in range(reported):
            p.bucket_ready(b, N)
        assert p.buckets_sent == reported
        p.gradients_ready(True, 0.01)
        assert [x for x in log if x.startswith("allreduce")] == want, log
        assert p.buckets_sent == 0
    p.begin_step(True, lambda: None)
    p.bucket_ready(0, N)
    with pytest.raises(Exception):
        p.bucket_ready(0, N)  # twice
    with pytest.raises(Exception):
        p.bucket_ready(2, N)  # skipping one
    p.begin_step(True, lambda: None)  # a new step starts from bucket 0 again
    p.bucket_ready(0, N)
    p.gradients_ready(True, 0.01)
    # A step that does NOT apply the optimiser (round-5 advisor, medium): the buckets its scatter reports and the rest of the
    # exchange go out all the same -- b0 b1 b2 b3 flat, then the wait, then the (non-applying) optimiser call -- so a rank on the
    # binned scatter path and a rank on the small-batch path keep issuing the same collectives.
    for reported in (4, 1, 0):
        del log[:]
        p.begin_step(False, lambda: None)
        log_before = list(log)  # (the pending step of the loop above completes here: wait + adam)
        for b in range(reported):
            p.bucket_ready(b, N)
        assert p.gradients_ready(False, 0.01) is True and not p.pending()
        mine = log[len(log_before):]
        assert mine == want + ["wait", "adam"], mine
    # OUTSIDE a step nobody's scatter starts an all-reduce: a test calling f2n_hash_bwd, a second runner on the device, a taped
    # backward -- the notification is dropped (the other ranks would never issue its partner)
    del log[:]
    p.bucket_ready(0, N)
    assert log == [] and p.buckets_sent == 0
    # without a bucket callback (one GPU, or the torch.distributed hooks) the notifications are ignored
    q = host.GradSyncPipeline()
    q.bucket_ready(3, N)
    assert q.buckets_sent == 0


def test_small_gradient_buffers_travel_first_on_every_rank_of_a_tail_step():
    """Round 6: a data-parallel step that goes through f2n_field_bwd_step_tail exchanges the small gradient buffers from the step's tail
    chain, beside the scatter -- BEFORE the table's buckets.  A rank whose batch missed the scene never reaches that chain; its `begin`
    must then send the small buffers in front of the buckets all the same (GradSyncPipeline::small_first), or the ranks' collectives
    pair up wrongly.  The sequence a rank issues, whatever happened to its batch: flat, b0 .. b3 in a tail step; b0 .. b3, flat otherwise."""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    host = runtime.host()
    N = 4

    def make(log):
        p = host.GradSyncPipeline()
        p.set_apply(lambda a, lr: None)
        p.set_defer_flags(lambda: None)
        p.set_bucket(lambda b, n: log.append("b%d" % b))
        p.set_small_exchange(lambda: log.append("flat"))

        def begin():  # DataParallel::GradSyncBegin
            need = not p.small_sent
            if need and p.small_first:
                assert p.buckets_sent == 0
                log.append("flat")
            for b in range(p.buckets_sent, N):
                log.append("b%d" % b)
            if need and not p.small_first:
                log.append("flat")
        p.set_begin_end(begin, lambda: None)
        p.pipelined = True
        return p
    want_tail = ["flat"] + ["b%d" % b for b in range(N)]
    for reported, has_samples in ((4, True), (2, True), (0, True), (0, False)):
        log = []
        p = make(log)
        p.begin_step(True, lambda: None)
        p.small_first = True                 # ExpRunner::TrainStep: this step is eligible for the early exchange
        if has_samples:
            p.small_grads_ready()            # f2n_field_bwd_step_tail's after_reduce
            p.small_grads_ready()            # (at most once per step)
            for b in range(reported):
                p.bucket_ready(b, N)
        p.gradients_ready(True, 0.01)
        assert log == want_tail, (reported, has_samples, log)
        assert not p.small_sent and p.buckets_sent == 0
    # a step that is not eligible (taped, gradient inspection): the small buffers behind the table, as before
    log = []
    p = make(log)
    p.begin_step(True, lambda: None)
    p.small_first = False
    p.bucket_ready(0, N)
    p.gradients_ready(True, 0.01)
    assert log == ["b%d" % b for b in range(N)] + ["flat"]
    # outside a step the early exchange is ignored like a stray bucket
    log = []
    p = make(log)
    p.small_grads_ready()
    assert log == []


def test_bench_reads_the_node_layout_of_the_checkpoint():
    """bench.py's PSNR study identifies surviving leaves from the raw TreeNode bytes with its own numpy dtype (it may not import the
    oracle): field offsets and size must be those of the 64-byte checkpoint layout (PersSampler.h:22-29)."""
    import importlib.util
    import os
    from oracle import octree_construct as octc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.NODE_DT.itemsize == octc.NODE_DT.itemsize == 64
    for f in ("center", "side_len", "parent", "childs", "is_leaf_node", "trans_idx"):
        assert bench.NODE_DT.fields[f][1] == octc.NODE_DT.fields[f][1], f
        assert bench.NODE_DT.fields[f][0].itemsize == octc.NODE_DT.fields[f][0].itemsize, f


def test_bench_reads_the_0p1_db_question_off_the_pooled_interval(tmp_path):
    """bench.py folds its own invocation's PSNR A/B into the pooled estimate over every committed session (profiles/psnr_estimates.json)
    and answers "within 0.1 dB" from the pooled 95 % interval with the UNPAIRED standard errors: true only when the whole interval lies
    inside +-0.1 dB, false only when it lies outside, "inconclusive" otherwise (round-5 verdict, weak 1 / next 4b)."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_test2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    committed = bench.pool_psnr_estimates(None, None, None, 0, 0)
    assert len(committed["estimates"]) >= 4 and committed["pooled_unpaired"]["standard_error_db"] < 0.06
    lo, hi = committed["pooled_unpaired"]["interval_95_db"]
    assert committed["within_0p1_db"] == (True if (lo >= -0.1 and hi <= 0.1) else False if (lo > 0.1 or hi < -0.1) else "inconclusive")
    f = tmp_path / "est.json"
    f.write_text(json.dumps({"estimates": [{"session": "a", "delta_db": 0.01, "standard_error_unpaired_db": 0.02, "standard_error_paired_db": 0.01}]}))
    r = bench.pool_psnr_estimates(0.03, 0.04, {"standard_error_db": 0.01, "mean_db": 0.02}, 4, 3, path=str(f))
    assert r["within_0p1_db"] is True and len(r["estimates"]) == 2 and r["pooled_unpaired"]["standard_error_db"] < 0.02
    assert abs(r["pooled_unpaired"]["delta_db"] - (0.01 / 0.02 ** 2 + 0.03 / 0.04 ** 2) / (1 / 0.02 ** 2 + 1 / 0.04 ** 2)) < 1e-3
    assert bench.pool_psnr_estimates(0.5, 0.04, None, 4, 3, path=str(tmp_path / "none.json"))["within_0p1_db"] is False
    assert bench.pool_psnr_estimates(0.05, 0.1, None, 4, 3, path=str(tmp_path / "none.json"))["within_0p1_db"] == "inconclusive"
    # an invocation whose paired error is tiny does not talk the pooled figure into a verdict: the unpaired error is what is weighted
    r = bench.pool_psnr_estimates(0.02, 0.15, {"standard_error_db": 0.005, "mean_db": 0.02}, 4, 3, path=str(tmp_path / "none.json"))
    assert r["within_0p1_db"] == "inconclusive" and r["pooled_paired_for_comparison"]["standard_error_db"] < 0.01


def test_philox_reference_matches_the_published_known_answers():
    """tests/philox_ref.py (the checker of the kernels' keyed draws: tests/test_gpu_determinism.py) against the known-answer vectors of
    Random123's Philox4x32-10 (kat_vectors: zero, all-ones and the pi-digit counter / key)."""
    import numpy as np
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from philox_ref import philox4x32_10
    kats = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kats:
        got = philox4x32_10(np.array([c], np.uint32), k)[0]
        assert tuple(int(v) for v in got) == want


def test_data_parallel_replicas_draw_their_own_streams():
    """Keyed draws (csrc/host/KeyedDraws.h) take their Philox key from (seed, purpose) -- and, in a data-parallel run, from the rank:
    with one seed on every rank (the replicas' parameters and octree come from it) the ranks would otherwise draw the same rays in
    ExpRunner::Train, the same march noise, background colours and edge samples, and N GPUs would render one batch N times.  Rank 0
    (and a single GPU) keeps the key of seed ^ purpose: the single-GPU bits do not change."""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    host = runtime.host()
    purposes = (0xA0761D6478BD642F, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03)  # rays, march noise, step draws (Dataset.h, PersSampler.h, Renderer.h)
    for seed in (2022, 67280421310721, 0):
        keys = set()
        for p in purposes:
            assert host.keyed_draw_key(seed, p, 0) == seed ^ p
            for rank in range(8):
                keys.add(host.keyed_draw_key(seed, p, rank))
        assert len(keys) == len(purposes) * 8  # every (purpose, rank) its own key


def test_adam_restatement_is_libtorch_op_sequence_up_to_fma_contraction():
    """oracle.pipeline.adam_step (what the GPU tests hold f2n_adam_* against, and what tests/test_lane_code_cpu.py holds the kernels'
    own update function against bit for bit) versus the op sequence of LibTorch's Adam::step (torch/csrc/api/src/optim/adam.cpp, the
    optimiser of ExpRunner.cpp:136) run with ATen itself: exp_avg.mul_(b1).add_(g, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2);
    denom = (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps); p.addcdiv_(exp_avg, denom, -lr / bc1).  Same scalars (doubles narrowed where
    they meet the float tensors); ATen's kernels fuse `a + alpha * b` into one FMA (as nvcc does by default in the reference's CUDA
    build -- DESIGN section 6, 'not reproducible'), the restatement and the product (-ffp-contract=off) round the product first.
    With the FMA emulated in float64 the moments agree in EVERY element; without it they agree to the last place or two."""
    import math
    rng = np.random.default_rng(8)
    n = 100000
    F64 = np.float64
    p = rng.standard_normal(n).astype(F32); g = (rng.standard_normal(n) * 1e-3).astype(F32)
    m = (rng.standard_normal(n) * 1e-3).astype(F32); v = (rng.random(n) * 1e-6).astype(F32)
    b1, b2, eps = 0.9, 0.99, 1e-15
    for step, lr in ((1, 1e-2), (10, 1e-2), (5000, 3e-3)):
        lr = float(F32(lr))
        rp, rm, rv = op.adam_step(p, g, m, v, step, lr, b1, b2, eps, 0.0)
        tp, tg, tm, tv = [torch.from_numpy(a.copy()) for a in (p, g, m, v)]
        tm.mul_(b1).add_(tg, alpha=1 - b1)
        tv.mul_(b2).addcmul_(tg, tg, value=1 - b2)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        denom = (tv.sqrt() / math.sqrt(bc2)).add_(eps)
        tp.addcdiv_(tm, denom, value=-(lr / bc1))
        # the moments with ATen's fused multiply-adds spelled out: one rounding of alpha * b + a
        fm = (g.astype(F64) * F64(F32(1 - b1)) + (m * F32(b1)).astype(F32).astype(F64)).astype(F32)
        fv = (((F32(1 - b2) * g).astype(F32)).astype(F64) * g.astype(F64) + (v * F32(b2)).astype(F32).astype(F64)).astype(F32)
        assert (fm == tm.numpy()).all() and (fv == tv.numpy()).all(), step
        # ... and the restatement's separately rounded form stays within rounding of them
        assert np.abs(rm - tm.numpy()).max() <= 2.0 ** -22 * np.abs(rm).max() and np.abs(rv - tv.numpy()).max() <= 2.0 ** -22 * np.abs(rv).max()
        assert np.abs(rp - tp.numpy()).max() <= 4e-7 * np.abs(rp).max(), step

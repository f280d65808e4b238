"""The distortion loss on warped ray intervals on the MI355X (csrc/render.hip, host/RendererTrain.cpp; run with `-m gpu`): the bodies of
tests/test_distortion_cpu.py through the ctypes binding, bit for bit with the numpy restatement (tests/distortion_ref.py);
host.ray_distortion; train.dist_loss_weight end to end on the set-up of tests/test_gpu_e2e.py::test_config1_end_to_end_parity (256 fox
rays, a 2^14 table, forced randoms, iteration 1): absent == 0, the untaped step against the taped one, the term in the gradient against
the CPU oracle, a streaming step against the synchronous one, runner.ray_distortion over chunks; the launcher's test.distortion."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import distortion_ref as dr  # noqa: E402
import test_distortion_cpu as cpu  # noqa: E402
import test_gpu_e2e as e2e  # noqa: E402

from oracle import capi as oc  # noqa: E402
from oracle import pipeline as op  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
EPS = 2.0 ** -24
N_EDGE = e2e.N_EDGE
rel_err = e2e.rel_err


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    runtime.host()
    return runtime


@pytest.fixture(scope="module")
def impl(rt):
    from f2_nerf_amd import capi
    return cpu.tensor_impl(capi, lambda x: x.cuda())


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def test_kernels_match_the_restatement_on_the_device(impl):
    cpu.check_known_answers(impl)
    cpu.check_bits(impl)
    cpu.check_bits(impl)  # twice in a row


def test_nan_stays_in_its_ray_on_the_device(impl):
    cpu.check_nan_containment(impl)


def test_loss_add_mean_on_the_device(impl):
    cpu.check_add_mean(impl)


def test_contract_cases_on_the_device(rt, impl):
    from f2_nerf_amd import capi
    cpu.check_contract(impl, capi.F2nError)
    r = cpu.rays()
    se, w, dt, dd = rt.to_dev(r["se"], r["w"], r["dt"], r["ddist"])
    out, dist = torch.zeros_like(w), torch.zeros(len(r["se"]), device="cuda")
    with pytest.raises(capi.F2nError):
        capi.distortion_fwd(-1, se, w, dt, dist)
    with pytest.raises(capi.F2nError):
        capi.distortion_bwd(-1, se, w, dt, dd, out)
    with pytest.raises(capi.F2nError):
        capi.distortion_bwd(len(r["se"]), se, w, dt, dd, w)  # (dweights is the scratch for D: it must not be the weights)
    assert capi.lib().f2n_abi_version() == 13


def test_host_ray_distortion_equals_the_binding(rt):
    from f2_nerf_amd import capi
    r = cpu.rays()
    se, w, dt = rt.to_dev(r["se"], r["w"], r["dt"])
    out = torch.full((len(r["se"]),), -1.0, device="cuda")
    capi.distortion_fwd(len(r["se"]), se, w, dt, out)
    got = rt.host().ray_distortion(w, dt, se)
    assert torch.equal(got, out) and dr.same_bits(got.cpu().numpy(), r["dist"])


# ---- end to end: the set-up of test_config1_end_to_end_parity ------------------------------------------------------------------------
def _setup(rt, st):
    rng = np.random.default_rng(42)
    R = 256
    cfg = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=14"], seed=7, table_init=0.3)
    runner, arrays = cfg[0], cfg[2]
    runner.iter_step = 1
    runner.update_ada_params()
    ro, rd, bounds, cam = e2e.fox_batch(st, rng, R)
    gt = rng.random((R, 3), dtype=F32)
    fineness = float(runner.fineness)
    noise = (((rng.random(1024 + R + 10, dtype=F32) - F32(.5)) + F32(1.)) * F32(fineness)).astype(F32)
    bg = rng.random((R, 3), dtype=F32)
    n_edges = st["edge_pool"].size // 64
    eidx = rng.integers(0, n_edges, N_EDGE).astype(np.int32)
    ecoord = (rng.random((N_EDGE, 2), dtype=F32) * F32(2.) - F32(1.)).astype(F32)
    host = dict(ro=ro, rd=rd, bounds=bounds, cam=cam, gt=gt, noise=noise, bg=bg, eidx=eidx, ecoord=ecoord)
    return dict(R=R, cfg=cfg[1], arrays=arrays, host=host, dev=rt.to_dev(ro, rd, bounds, gt, cam, noise, bg, eidx, ecoord))


def _runner(rt, st, s, extra):
    runner, _, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=14"] + list(extra), seed=7, table_init=0.3)
    runner.n_edge_pts = N_EDGE
    runner.iter_step = 1  # keep the iteration-0 compaction out of the comparison
    runner.update_ada_params()
    d = s["dev"]
    runner.set_forced_randoms(d[5], d[6], d[7], d[8])
    return runner


def _step(runner, s, taped=False):
    d = s["dev"]
    runner.zero_grad()
    stats = (runner.train_step_autograd if taped else runner.train_step)(d[0], d[1], d[2], d[3], d[4], False)
    return stats, {k: v.cpu().numpy().copy() for k, v in runner.grads().items()}


def _cos(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    return float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))


def _oracle_forward(st, s):
    """tests/test_gpu_e2e.py::oracle_train_iteration up to the loss (iteration 1), keeping what its backward needs"""
    cfg, h = s["cfg"], s["host"]
    tn, tr, _, _, table, prim, bias, nvol, p_field, p_color, app_emb = s["arrays"]
    grid = op.HashGrid(table, prim, bias, int(nvol[0]), int(cfg["field"]["log2_table_size"]))
    rays_d = oc.normalize_dirs(h["rd"])
    ps = cfg["pts_sampler"]
    hits = oc.oct_intersect(st["search_order"], h["ro"], rays_d, float(ps["near"]), 1e8, tn, int(ps["max_oct_intersect_per_ray"]))
    smp = oc.ray_march(h["ro"], rays_d, h["noise"], float(ps["sample_l"]), bool(ps["scale_by_dis"]), *hits, tn, tr)
    fsh = dict(d_hidden=int(cfg["field"]["mlp_hidden_dim"]), n_hidden=int(cfg["field"]["n_hidden_layers"]))
    ssh = dict(d_hidden=int(cfg["shader"]["d_hidden"]), n_hidden=int(cfg["shader"]["n_hiddens"]), degree=int(cfg["shader"]["degree"]))
    feat_all = op.field_fwd(grid, p_field, smp["pts"], smp["anchors"][:, 0], **fsh)
    _, _, mask, new_se = op.early_stop(feat_all[:, 0], smp["dt"], smp["pts_idx_bounds"])
    pts, dirs, dt, t, anchors = op.compact(mask, smp["pts"], smp["dirs"], smp["dt"], smp["t"], smp["anchors"])
    m = len(pts)
    e_pts, e_idx = oc.edge_samples(st["edge_pool"], tr, h["eidx"], h["ecoord"])
    q_pts = np.concatenate([pts, e_pts.reshape(-1, 3)], 0)
    q_vol = np.concatenate([anchors[:, 0], e_idx.reshape(-1)], 0).astype(np.int32)
    feat, fctx = op.field_fwd(grid, p_field, q_pts, q_vol, want_ctx=True, **fsh)
    scene_feat, edge_feat = feat[:m], feat[m:].reshape(len(h["eidx"]), 2, 16)
    use_emb = bool(cfg["renderer"]["use_app_emb"])
    sidx = oc.scatter_idx(m, new_se, h["cam"]) if use_emb else None
    rgb, sctx = op.shade_fwd(p_color, scene_feat, dirs, app_emb if use_emb else None, sidx, want_ctx=True, **ssh)
    comp = op.composite_fwd(scene_feat, dt, t, rgb, h["bg"], new_se, want_ctx=True)
    tcfg = cfg["train"]
    assert 1 <= tcfg["var_loss_start"]  # (iteration 1: the weight-variance term is off)
    lg = op.losses_and_grads(comp["colors"], h["gt"], comp["disparity"], comp["weights"], new_se, edge_feat, 0.0,
                             float(tcfg["disp_loss_weight"]), float(tcfg["tv_loss_weight"]))
    gs0, gs1 = float(tcfg["gradient_scaling_start"]), float(tcfg["gradient_scaling_end"])
    gs = 1.0 if 1 >= gs1 else max(0.0, (1 - gs0) / (gs1 - gs0 + 1e-9))
    # d dist / d w of the fp64 pairwise definition on the oracle's own weights and dt
    g_ref = np.zeros(m, np.float64)
    dist = np.zeros(len(new_se), np.float64)
    for r, (a, b) in enumerate(new_se):
        if a < b:
            dist[r], g_ref[a:b] = dr.ray64(comp["weights"][a:b], dt[a:b])
    return dict(grid=grid, p_field=p_field, p_color=p_color, fctx=fctx, sctx=sctx, comp=comp, lg=lg, gs=gs, dt=dt, rgb=rgb, new_se=new_se, m=m,
                feat=feat, sidx=sidx, n_emb=len(app_emb) if use_emb else 0, g_ref=g_ref, dist=dist, bg=h["bg"])


def _oracle_backward(o, W, R):
    dweights = (F32(W) / F32(R) * o["g_ref"]).astype(F32) if W > 0 else None
    drgb, df0 = op.composite_bwd(o["comp"]["ctx"], o["dt"], o["rgb"], o["bg"], o["new_se"], o["lg"]["dcolors"], o["lg"]["ddisparity"], None,
                                 dweights, o["gs"])
    dp_color, dfeat_sh, demb = op.shade_bwd(o["p_color"], o["sctx"], drgb, o["n_emb"], o["sidx"])
    m = o["m"]
    dfeat = np.zeros_like(o["feat"])
    dfeat[:m] = dfeat_sh
    dfeat[:m, 0] += df0
    dfeat[m:] = o["lg"]["dedge"].reshape(-1, 16)
    dp_field, gtab, _ = op.field_bwd(o["grid"], o["p_field"], o["fctx"], dfeat, 128.0, fp32_accumulate=True)
    return dict(feat_pool=gtab.reshape(-1, 2), field_mlp=dp_field, color_mlp=dp_color, app_emb=demb)


BAR_MLP, BAR_COS = 3e-2, 0.999  # test_config1_end_to_end_parity's bars against the oracle


@pytest.fixture(scope="module")
def scene(rt, fox_state):
    """The batch, the oracle's iteration on it, and the weight W of bodies (b) to (d): the smallest power of four at which the ORACLE's
    gradients with and without the term are at least three bars apart -- relative difference >= 3 x 3e-2 for the field MLP, 1 - cosine >=
    3 x 1e-3 for the table.  The term reaches the parameters through d f0 alone (compositing's drgb does not depend on dweights), so the
    colour MLP's and the appearance embedding's gradients are the same arrays with and without it, whatever W: for those two the
    precondition cannot hold and is replaced by the assertion that they are identical; the product is held to their bars all the same.
    All of this runs on the CPU, before the first launch of the bodies that use W."""
    s = _setup(rt, fox_state)
    o = _oracle_forward(fox_state, s)
    g0 = _oracle_backward(o, 0.0, s["R"])
    W, gW = 4.0 ** -6, None
    while W <= 4.0 ** 12:
        gW = _oracle_backward(o, W, s["R"])
        sep_mlp, sep_cos = rel_err(g0["field_mlp"], gW["field_mlp"]), 1.0 - _cos(g0["feat_pool"], gW["feat_pool"])
        if sep_mlp >= 3 * BAR_MLP and sep_cos >= 3 * (1.0 - BAR_COS):
            break
        W *= 4.0
    print("W = %g: oracle with / without the term: field MLP %.3f, table 1 - cos %.4f" % (W, sep_mlp, sep_cos))
    assert sep_mlp >= 3 * BAR_MLP and sep_cos >= 3 * (1.0 - BAR_COS), (W, sep_mlp, sep_cos)
    assert np.array_equal(g0["color_mlp"], gW["color_mlp"]) and np.array_equal(g0["app_emb"], gW["app_emb"])
    s.update(o=o, g0=g0, gW=gW, W=W)
    return s


def test_absent_key_is_weight_zero(rt, fox_state, scene):
    """(a) no key == weight 0, bit for bit; a weight > 0 leaves the sampler alone"""
    plain, zero, on = (_runner(rt, fox_state, scene, x) for x in ([], ["train.dist_loss_weight=0"], ["train.dist_loss_weight=%r" % scene["W"]]))
    assert plain.dist_loss_weight == 0.0 and zero.dist_loss_weight == 0.0 and on.dist_loss_weight == F32(scene["W"])
    (s0, g0), (s1, g1) = _step(plain, scene), _step(zero, scene)
    assert float(s0["loss"]) == float(s1["loss"]) and set(s0) == set(s1)
    assert torch.equal(plain.last_losses(), zero.last_losses())
    # The three small gradients, bit for bit: the field MLP's is a function of every row of dfeat, the density column included, so
    # everything in front of the hash scatter is covered.  The table's gradient is NOT reproducible from run to run at this batch
    # size, with or without this feature: below 32768 samples the scatter adds in f16 atomics, in the order the waves arrive (two runners
    # without the key, and one runner stepped twice, differ by 1.2e-3 .. 1.9e-3 of the largest entry on the MI355X).  It is held to the
    # bar test_config1_end_to_end_parity sets between two routes that differ in exactly that order (cosine > 0.99999).
    assert all(dr.same_bits(g0[k], g1[k]) for k in ("field_mlp", "color_mlp", "app_emb"))
    print("table gradient, no key against weight 0: 1 - cosine %.3g" % (1.0 - _cos(g0["feat_pool"], g1["feat_pool"])))
    assert _cos(g0["feat_pool"], g1["feat_pool"]) > 0.99999
    assert float(plain.last_losses()[6]) == 0.0 and float(plain.last_losses()[0]) == float(s0["loss"])
    d = scene["dev"]
    a, b = plain.get_samples(d[0], d[1], d[2]), on.get_samples(d[0], d[1], d[2])
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(Exception):
            _runner(rt, fox_state, scene, ["train.dist_loss_weight=%s" % bad])


def check_untaped_equals_taped(rt, st, s, W):
    """(b) train_step against train_step_autograd with the bars test_config1_end_to_end_parity uses between the two; the reported
    term against the fp64 definition; loss(W) - loss(0) = W x term"""
    d = s["dev"]
    on, off = _runner(rt, st, s, ["train.dist_loss_weight=%r" % W]), _runner(rt, st, s, [])
    stats, g = _step(on, s)
    losses = on.last_losses().cpu().numpy()
    stats_a, ga = _step(on, s, taped=True)
    losses_a = on.last_losses().cpu().numpy()
    assert stats_a["n_samples"] == stats["n_samples"] and stats_a["n_meaningful"] == stats["n_meaningful"]
    assert abs(float(stats_a["loss"]) - float(stats["loss"])) <= 1e-6 * max(1.0, abs(float(stats["loss"])))
    for k in ("color_mlp", "field_mlp", "app_emb"):
        assert rel_err(g[k], ga[k]) <= 2e-3, (k, rel_err(g[k], ga[k]))
    assert _cos(g["feat_pool"], ga["feat_pool"]) > 0.99999
    # the reported term: the mean over the rays of the fp64 pairwise definition on render_train's weights and the survivors' dt
    out = on.render_train(d[0], d[1], d[2], d[4])
    se, w, dt = (out[k].detach().cpu().numpy() for k in ("idx_start_end", "weights", "dt"))
    want = float(dr.dist64(se, w, dt).mean())
    n_max = int((se[:, 1] - se[:, 0]).max())
    tol = ((3 * n_max + 8) * EPS + 1e-6) * want
    print("W = %g: losses[6] %.9g (taped %.9g), fp64 %.9g, longest ray %d samples; loss %.7g" % (W, losses[6], losses_a[6], want, n_max, losses[0]))
    assert want > 0 and abs(float(losses[6]) - want) <= tol and abs(float(losses_a[6]) - want) <= tol
    assert float(losses[0]) == float(stats["loss"]) and float(losses[5]) == float(stats["mse"]) and losses[7] == 0.0
    # loss(W) - loss(0) = W x term: every loss value is an fp32 number of the size of loss(W), so 1e-5 is taken relative to that
    stats0, _ = _step(off, s)
    assert abs((float(stats["loss"]) - float(stats0["loss"])) - W * float(losses[6])) <= 1e-5 * abs(float(stats["loss"]))
    assert W * float(losses[6]) > 100 * 1e-5 * abs(float(stats["loss"]))  # (... and the term is far above that resolution)
    assert all(losses[k] == off.last_losses().cpu().numpy()[k] for k in (1, 2, 3, 4, 5))


def test_untaped_step_equals_taped_step_with_the_term(rt, fox_state, scene):
    check_untaped_equals_taped(rt, fox_state, scene, scene["W"])


def test_the_term_is_in_the_gradient(rt, fox_state, scene):
    """(c) the product's gradients with weight W against the oracle iteration whose compositing backward was handed W / R x d dist / d w:
    the bars of test_config1_end_to_end_parity.  The oracle without the term is at least three bars away (the `scene` fixture)."""
    on = _runner(rt, fox_state, scene, ["train.dist_loss_weight=%r" % scene["W"]])
    _, g = _step(on, scene)
    rg = scene["gW"]
    errs = {k: rel_err(g[k], rg[k]) for k in ("color_mlp", "field_mlp", "app_emb")}
    cos = _cos(g["feat_pool"], rg["feat_pool"])
    print("W = %g: against the oracle with the term: %s, table cosine %.6f; without: field MLP %.3f, cosine %.6f"
          % (scene["W"], errs, cos, rel_err(g["field_mlp"], scene["g0"]["field_mlp"]), _cos(g["feat_pool"], scene["g0"]["feat_pool"])))
    assert all(e <= BAR_MLP for e in errs.values()), errs
    assert cos > BAR_COS, cos


def test_streaming_step_equals_synchronous_step_with_the_term(rt, fox_state, scene):
    """(d) tests/test_gpu_e2e.py::test_streaming_step_equals_synchronous_step with weight W: both routes take the three launches"""
    st = fox_state
    rng = np.random.default_rng(61)
    R, NE = 1024, 512
    ro, rd, bounds, cam = e2e.fox_batch(st, rng, R)
    gt = rng.random((R, 3), dtype=F32)
    noise = (((rng.random(1024 + R + 10, dtype=F32) - F32(.5)) + F32(1.)) * F32(8.)).astype(F32)
    bg = rng.random((R, 3), dtype=F32)
    eidx = rng.integers(0, st["edge_pool"].size // 64, NE).astype(np.int32)
    ecoord = (rng.random((NE, 2), dtype=F32) * F32(2.) - F32(1.)).astype(F32)
    d = rt.to_dev(ro, rd, bounds, gt, cam, noise, bg, eidx, ecoord)
    ro2, rd2, bounds2, _ = e2e.fox_batch(st, rng, R)
    nxt = rt.to_dev(ro2, rd2, bounds2)
    res = []
    for mode in (0, 2, "next"):  # 0: read the count back; 2: never (the streaming route); "next": handed the next batch, optimiser applied
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=16", "train.dist_loss_weight=%r" % scene["W"]], seed=21, table_init=0.5)
        states = [t.cpu().clone() for t in runner.states()]
        states[8][-16 * 64:-15 * 64] *= 16.0  # the density row of the field MLP's output layer: opaque stretches -> early stop
        runner.load_states(states)
        runner.n_edge_pts = NE
        if mode != "next":
            runner.async_counts = mode
        runner.iter_step = 1
        runner.update_ada_params()
        runner.set_forced_randoms(d[5], d[6], d[7], d[8])
        runner.zero_grad()
        if mode == "next":
            stats = runner.train_step(d[0], d[1], d[2], d[3], d[4], True, nxt[0], nxt[1], nxt[2])
            g = None  # (the optimiser has consumed them; the gradients of the streaming route are those of mode 2)
        else:
            stats = runner.train_step(d[0], d[1], d[2], d[3], d[4], False)
            g = {k: v.cpu().numpy().copy() for k, v in runner.grads().items()}
        res.append((float(stats["loss"]), float(runner.last_losses()[6]), stats["n_samples"], g))
        runner.flush()
    (l0, t0, n0, g0) = res[0]
    assert t0 > 0
    for l1, t1, n1, g1 in res[1:]:
        assert n0 == n1 and l0 == l1 and t0 == t1
        if g1 is None:
            continue
        for k in ("color_mlp", "field_mlp", "app_emb"):
            assert rel_err(g1[k], g0[k]) <= 2e-3, (k, rel_err(g1[k], g0[k]))  # (per-block partial sums see the rows in another order)
        a, b = g0["feat_pool"].reshape(-1).astype(np.float64), g1["feat_pool"].reshape(-1).astype(np.float64)
        assert float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b))) > 0.999999
        assert np.abs(a - b).max() <= 2.0 ** -9 * np.abs(a).max()


def test_runner_ray_distortion_over_chunks(rt, fox_state, scene):
    """(e) runner.ray_distortion over three chunks == host.ray_distortion on render_geometry(return_samples=True) of each chunk"""
    runner = _runner(rt, fox_state, scene, [])
    d = scene["dev"]
    R = scene["R"]
    runner.render_chunk_rays = 100  # 100 + 100 + 56
    got = runner.ray_distortion(d[0], d[1], d[2])
    again = runner.ray_distortion(d[0], d[1], d[2])
    assert got.shape == (R,) and torch.equal(got, again)
    parts = []
    for i in range(0, R, 100):
        g = runner.render_geometry(d[0][i:i + 100].contiguous(), d[1][i:i + 100].contiguous(), d[2][i:i + 100].contiguous(), return_samples=True)
        parts.append(rt.host().ray_distortion(g["weights"], g["dt"], g["idx_start_end"]))
    want = torch.cat(parts)
    assert torch.equal(got, want) and float(got.max()) > 0 and bool(torch.isfinite(got).all())
    runner.render_chunk_rays = 65536


# ---- the launcher --------------------------------------------------------------------------------------------------------------------
def test_launcher_writes_distortion(tmp_path, capsys):
    """The synthetic rig of tests/test_gpu_ssim.py's launcher test: mode=test with test.distortion=true adds distortion / mean_distortion to
    info.yaml and one line to the output; without the option info.yaml is the old file byte for byte."""
    import yaml
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import rigs, run
    rng = np.random.default_rng(2)
    meta, hw = rigs.forward_facing(rng, n_side=(5, 4), hw=(48, 64), focal=56.0)
    meta[:, 12:14] *= 4.0; meta[:, 14] *= 4.0; meta[:, 16:18] *= 4.0
    data = tmp_path / "data" / "synth" / "rig"
    (data / "images_4").mkdir(parents=True)
    np.save(data / "cams_meta.npy", meta)
    yy, xx = np.mgrid[0:48, 0:64]
    for i in range(len(meta)):
        base = 127 + 90 * np.sin(0.2 * xx[..., None] + 0.15 * yy[..., None] + 0.9 * np.arange(3) + i)
        Image.fromarray(np.clip(base + rng.integers(-6, 7, (48, 64, 3)), 0, 255).astype(np.uint8)).save(data / "images_4" / ("%03d.png" % i))
    common = ["--config-name=llff", "dataset_name=synth", "case_name=rig", "exp_name=t", "+work_dir=%s" % tmp_path,
              "field.log2_table_size=14", "train.end_iter=60", "train.save_freq=30", "train.learning_rate_warm_up_end_iter=10",
              "pts_sampler.sub_div_milestones=[20]", "pts_sampler.compact_freq=25", "train.pts_batch_size=32768"]
    out_dir = tmp_path / "exp" / "rig" / "t" / "test_images"
    assert run.main(common + ["mode=train"]) == 0
    capsys.readouterr()
    assert run.main(common + ["mode=test", "is_continue=true"]) == 0
    plain_out = capsys.readouterr().out
    plain_text = open(out_dir / "info.yaml").read()
    plain = yaml.safe_load(plain_text)
    views = sorted(k for k in plain if k != "mean_psnr")
    assert len(views) >= 2 and "Mean distortion" not in plain_out
    assert run.main(common + ["mode=test", "is_continue=true", "test.distortion=true"]) == 0
    out = capsys.readouterr().out
    info = yaml.safe_load(open(out_dir / "info.yaml"))
    assert set(info) == set(plain) | {"distortion", "mean_distortion"} and all(info[k] == plain[k] for k in plain)
    order = [str(k) for k in sorted(int(v) for v in views)]
    assert set(info["distortion"]) == set(views) and all(np.isfinite(v) and v >= 0 for v in info["distortion"].values())
    assert info["mean_distortion"] == sum(info["distortion"][k] for k in order) / len(views) and info["mean_distortion"] > 0
    means = lambda text: [ln for ln in text.split("\n") if ln.startswith("Mean ")]  # noqa: E731
    assert means(out) == means(plain_out) + ["Mean distortion: %s" % info["mean_distortion"]]
    assert len(out.split("\n")) == len(plain_out.split("\n")) + 1
    with capsys.disabled():
        print("launcher: mean_distortion %.6g over %d views" % (info["mean_distortion"], len(views)))
    assert run.main(common + ["mode=test", "is_continue=true"]) == 0
    assert open(out_dir / "info.yaml").read() == plain_text and "Mean distortion" not in capsys.readouterr().out

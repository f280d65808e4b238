"""Render geometry buffers on the MI355X (csrc/render.hip f2n_composite_geometry, host/RendererQuery.cpp Renderer::RenderGeometry):
the entry point on synthetic rays (bit for bit against f2n_density_grad_scatter and the float32 restatement of tests/geometry_ref.py),
runner.render_geometry on the fox scene (the colours of render_rays bit for bit, the samples' gradient against the float64
restatement with the bar of tests/test_gpu_density_grad.py, the per-ray buffers bit for bit), a field shape without the fused kernels,
no effect on training, and the launcher's mode=extract_points."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import density_grad_ref as dr  # noqa: E402
import geometry_ref as gr  # noqa: E402
from oracle import capi as oc, pipeline as op  # noqa: E402
from test_geometry_cpu import check_case  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
N_FOX_RAYS = 2000
PER_RAY = ("opacity", "normals", "surf_t", "surf_points", "surf_normals")


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def fox_runner(rt, fox_state):
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14"], seed=1, table_init=0.3)
    return runner, arrays


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def device_geometry(c, want_grad=True, want_normal=True):
    from f2_nerf_amd import capi
    R, M = len(c["se"]), len(c["t"])
    nan = float("nan")
    o = dict(opacity=torch.full((R,), nan, device="cuda"), normals=torch.full((R, 3), nan, device="cuda"),
             surf_idx=torch.full((R,), -7, dtype=torch.int32, device="cuda"), surf_t=torch.full((R,), nan, device="cuda"),
             surf_points=torch.full((R, 3), nan, device="cuda"), surf_normals=torch.full((R, 3), nan, device="cuda"),
             sample_grad=torch.full((M, 3), nan, device="cuda") if want_grad else None,
             sample_normals=torch.full((M, 3), nan, device="cuda") if want_normal else None)
    capi.composite_geometry(R, _dev(c["se"], np.int32), _dev(c["weights"], F32), _dev(c["t"], F32), _dev(c["rays_o"], F32), _dev(c["rays_d"], F32),
                            _dev(c["anchors"], np.int32), _dev(c["transes"], np.uint8), _dev(c["df0_dw"], F32), c["tau"], o["opacity"], o["normals"],
                            o["surf_idx"], o["surf_t"], o["surf_points"], o["surf_normals"], o["sample_grad"], o["sample_normals"])
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def device_scatter(c):
    from f2_nerf_amd import capi
    M = len(c["t"])
    x = gr.world_points(c["rays_o"], c["rays_d"], c["t"], c["se"])
    se = np.stack([np.arange(M), np.arange(M) + 1], 1)
    dens, grad, nrm = (torch.full(s, float("nan"), device="cuda") for s in ((M,), (M, 3), (M, 3)))
    capi.density_grad_scatter(M, _dev(x, F32), _dev(c["anchors"], np.int32), _dev(se, np.int32), _dev(c["transes"], np.uint8),
                              torch.full((M,), 3.0, device="cuda"), _dev(c["df0_dw"], F32), dens, grad, nrm)
    dens = dens.cpu().numpy()
    assert (dens == 1).all()
    return dens, grad.cpu().numpy(), nrm.cpu().numpy()


@pytest.mark.parametrize("n_rays,max_len,special", [(37, 100, True), (4099, 400, False)])
def test_entry_point_matches_the_restatement(fox_state, n_rays, max_len, special):
    """The cases of tests/test_geometry_cpu.py (37 rays, every chunk boundary, the special rays) and 4099 rays of 0..400 samples."""
    c = gr.synthetic_case(fox_state["pers_trans"], n_rays=n_rays, seed=5 if special else 9, max_len=max_len, special=special)
    out = device_geometry(c)
    ref = check_case(c, out, device_scatter(c))
    lens = c["se"][:, 1] - c["se"][:, 0]
    assert (lens == 0).any() and lens.max() > (99 if special else 380)
    assert (ref["surf_idx"] >= 0).any() and (ref["surf_idx"][lens > 0] < 0).any()
    for kw in (dict(want_grad=False, want_normal=False), dict()):  # NULL optional outputs; a second call
        o2 = device_geometry(c, **kw)
        for k, v in out.items():
            if o2[k] is not None:
                assert gr.same_bits(o2[k], v), (kw, k)
    from f2_nerf_amd import capi
    with pytest.raises(capi.F2nError):
        bad = dict(c)
        bad["tau"] = 1.5
        device_geometry(bad)


def _camera_rays(st, cam, n):
    H, W = [int(v) for v in st["image_hw"]]
    k = np.linspace(0, H * W - 1, n).astype(np.int64)
    ij = np.stack([k // W, k % W], 1).astype(np.int32)
    ro, rd = oc.img2world(st["poses"], st["intri"], st["dist_params"], np.full(n, cam, np.int32), ij)
    return ro, rd, np.tile(st["bounds"][cam][None], (n, 1)).astype(F32)


def _check_fox(rt, runner, st, grid, params, d_hidden=64, dx_of=None):
    ro, rd, bounds = _camera_rays(st, int(st["train_set"][0]), N_FOX_RAYS)
    d = rt.to_dev(ro, rd, bounds)
    base = [x.cpu().numpy() for x in runner.render_rays(*d)]  # colors, disparity, first_oct_dis, depth
    g = _np(runner.render_geometry(*d, return_samples=True))
    assert sorted(g) == sorted(["colors", "disparity", "depth", "opacity", "normals", "surf_idx", "surf_t", "surf_points", "surf_normals", "pts", "anchors",
                                "t", "dt", "weights", "idx_start_end", "sample_grad", "sample_normals"])
    assert gr.same_bits(g["colors"], base[0]) and gr.same_bits(g["disparity"], base[1]) and gr.same_bits(g["depth"], base[3])
    plain = _np(runner.render_geometry(*d))
    assert sorted(plain) == sorted(["colors", "disparity", "depth", "opacity", "normals", "surf_idx", "surf_t", "surf_points", "surf_normals"])
    for k, v in plain.items():  # keeping the samples changes nothing; a second call gives the same bits
        assert gr.same_bits(v, g[k]), k
    se, M = g["idx_start_end"], len(g["t"])
    assert se.shape == (N_FOX_RAYS, 2) and se[-1, 1] == M and M > 0 and (se[:, 1] > se[:, 0]).any()  # some ray has samples
    assert g["pts"].shape == (M, 3) and g["anchors"].shape == (M, 3) and g["weights"].shape == (M,) and g["sample_grad"].shape == (M, 3)
    unit_d = oc.normalize_dirs(rd)
    x = gr.world_points(ro, unit_d, g["t"], se)
    # the samples' gradient against the float64 restatement (metric and bar of tests/test_gpu_density_grad.py)
    ref64, ref32, S, keep = gr.restated_sample_grad(st["pers_trans"], grid, params, g["pts"], g["anchors"], x, d_hidden, dx_of)
    assert (~keep).mean() <= 0.01
    disc, err = dr.rel_err(ref32, ref64, S, keep), dr.rel_err(g["sample_grad"], ref64, S, keep)
    print("%d samples of %d rays: restatement f32-vs-f64 %.3g, bar %.3g, device %.3g, left out %.5f" % (M, N_FOX_RAYS, disc, 8 * disc, err, (~keep).mean()))
    assert err <= 8.0 * disc, (err, 8.0 * disc)
    assert gr.same_bits(g["sample_normals"], gr.unit(g["sample_grad"], -1.0))
    # the per-ray buffers against the float32 restatement fed the returned weights and sample normals
    ref = gr.ray_buffers(se, g["weights"], g["t"], ro, unit_d, g["sample_normals"], 0.5)
    assert (g["surf_idx"] == ref["surf_idx"]).all()
    for k in PER_RAY:
        assert gr.same_bits(g[k], ref[k]), k
    print("opacity: max %.3g, rays with a surface at tau = 0.5: %d" % (g["opacity"].max(), (g["surf_idx"] >= 0).sum()))
    # a lower threshold: the same sums, another surface
    lo = _np(runner.render_geometry(*d, tau=1e-3))
    assert gr.same_bits(lo["opacity"], g["opacity"]) and gr.same_bits(lo["normals"], g["normals"])
    ref_lo = gr.ray_buffers(se, g["weights"], g["t"], ro, unit_d, g["sample_normals"], 1e-3)
    assert (lo["surf_idx"] == ref_lo["surf_idx"]).all() and gr.same_bits(lo["surf_points"], ref_lo["surf_points"])
    return d, g


def test_render_geometry_on_the_fox(rt, fox_runner, fox_state):
    runner, arrays = fox_runner
    grid = op.HashGrid(arrays[4], arrays[5], arrays[6], int(arrays[7][0]), 14)
    d, g = _check_fox(rt, runner, fox_state, grid, np.asarray(arrays[8], F32))
    # chunks: the same per-ray outputs (surf_idx counts within the chunk), and return_samples refuses them
    chunk = runner.render_chunk_rays
    runner.render_chunk_rays = 768
    try:
        c = _np(runner.render_geometry(*d))
        for k in ("colors", "disparity", "depth") + PER_RAY:
            assert gr.same_bits(c[k], g[k]), k
        assert ((c["surf_idx"] >= 0) == (g["surf_idx"] >= 0)).all()
        with pytest.raises(RuntimeError):
            runner.render_geometry(*d, return_samples=True)
    finally:
        runner.render_chunk_rays = chunk
    with pytest.raises(RuntimeError):
        runner.render_geometry(*d, tau=0.0)
    # rays that miss the scene: render_rays' empty result, zeros and -1
    far = torch.full((5, 3), 1.0e4, device="cuda")
    away = torch.tensor([[1.0, 0.0, 0.0]], device="cuda").repeat(5, 1)
    e = _np(runner.render_geometry(far, away, d[2][:5].contiguous(), return_samples=True))
    b = [x.cpu().numpy() for x in runner.render_rays(far, away, d[2][:5].contiguous())]
    assert gr.same_bits(e["colors"], b[0]) and gr.same_bits(e["disparity"], b[1]) and gr.same_bits(e["depth"], b[3])
    assert (e["surf_idx"] == -1).all() and all((e[k] == 0).all() for k in PER_RAY)
    assert len(e["t"]) == 0 and e["sample_grad"].shape == (0, 3) and e["idx_start_end"].shape == (5, 2)


def test_a_field_shape_without_the_fused_kernels(rt, fox_state):
    """field.mlp_hidden_dim=32: op-by-op rendering, df0/dx from f2n_mlp_bwd (h16 hidden gradients) and f2n_hash_pos_grad.  Bar: 8 x the
    discrepancy between the restatement fed the oracle's mlp_bwd dx and the float64 restatement."""
    runner, cfg, arrays = rt.make_runner(fox_state, "wanjinyou", ["field.log2_table_size=14", "field.mlp_hidden_dim=32"], seed=1, table_init=0.3)
    params = np.asarray(arrays[8], F32)
    assert len(params) == 32 * 32 + 16 * 32

    def oracle_dx(c):
        x = oc.h2f(c["x_h"])
        _, acts = oc.mlp_fwd(params, x, 32, 1, want_acts=True)
        dy = np.zeros((len(x), 16), F32)
        dy[:, 0] = 1
        return oc.mlp_bwd(params, x, acts, dy, 32, 1, 1.0)[1]

    grid = op.HashGrid(arrays[4], arrays[5], arrays[6], int(arrays[7][0]), 14)
    _check_fox(rt, runner, fox_state, grid, params, 32, oracle_dx)


def test_render_geometry_has_no_effect_on_training(rt, fox_state):
    st = fox_state
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]
    view = rt.to_dev(*_camera_rays(st, int(st["train_set"][1]), 1500))

    def run(query):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if query and k == 3:
                g = runner.render_geometry(*view, return_samples=True)
                assert len(g["t"]) > 0 and (g["sample_normals"] != 0).any()
                runner.render_chunk_rays = 600
                assert runner.render_geometry(*view)["opacity"].shape == (1500,)
                runner.render_chunk_rays = 65536
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [t.detach().cpu().numpy().copy() for t in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


def test_launcher_extract_points(tmp_path, monkeypatch):
    """mode=extract_points on the tiny scene of tests/test_gpu_mesh.py::test_launcher_extract_mesh.  A scene trained for 60 iterations
    is translucent, so the thresholds are lowered until rays qualify; the counts are taken from the renders themselves."""
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh, rigs, run
    from test_geometry_cpu import _read_ply
    rng = np.random.default_rng(2)
    meta, hw = rigs.forward_facing(rng, n_side=(5, 4), hw=(48, 64), focal=56.0)
    meta[:, 12:14] *= 4.0; meta[:, 14] *= 4.0; meta[:, 16:18] *= 4.0
    data = tmp_path / "data" / "synth" / "rig"
    (data / "images_4").mkdir(parents=True)
    np.save(data / "cams_meta.npy", meta)
    for i in range(len(meta)):
        Image.fromarray(rng.integers(0, 255, (48, 64, 3), dtype=np.uint8)).save(data / "images_4" / ("%03d.png" % i))
    common = ["--config-name=llff", "dataset_name=synth", "case_name=rig", "exp_name=t", "+work_dir=%s" % tmp_path,
              "field.log2_table_size=14", "train.end_iter=60", "train.save_freq=30", "train.learning_rate_warm_up_end_iter=10",
              "pts_sampler.sub_div_milestones=[20]", "pts_sampler.compact_freq=25", "train.pts_batch_size=32768"]
    assert run.main(common + ["mode=train"]) == 0
    seen = {"kept": 0, "views": 0}
    orig = mesh.camera_rays

    def spy_rays(dataset, bounds, idx, res_level):
        seen["rays"] = orig(dataset, bounds, idx, res_level)
        assert res_level == 2 and seen["rays"][0].shape == (24 * 32, 3)
        return seen["rays"]

    class Spy:  # counts the rays the export has to keep, from the very renders it makes
        def __init__(self, runner):
            self.runner = runner

        def __getattr__(self, name):
            return getattr(self.runner, name)

        def render_geometry(self, ro, rd, b, tau=0.5):
            g = self.runner.render_geometry(ro, rd, b, tau=tau)
            seen["kept"] += int(((g["surf_idx"] >= 0) & (g["opacity"] >= seen["min_opacity"])).sum())
            seen["views"] += 1
            return g

    orig_extract = mesh.extract_points
    monkeypatch.setattr(mesh, "camera_rays", spy_rays)
    monkeypatch.setattr(mesh, "extract_points", lambda runner, cfg, scene, ds, exp_dir: seen.update(
        n_train=len(scene["train_set"]), min_opacity=mesh.points_options(cfg)["min_opacity"]) or orig_extract(Spy(runner), cfg, scene, ds, exp_dir))
    # (any ray that meets the scene accumulates 1e-4 of weight within a few samples, whatever the 60 iterations made of the table)
    opts = ["mode=extract_points", "is_continue=true", "points.res_level=2", "points.tau=0.0001", "points.min_opacity=0.0001"]
    path = str(tmp_path / "exp" / "rig" / "t" / "points" / "60.ply")
    for capped in (False, True):
        cap = max(1, seen["kept"] // 3) if capped else None  # (a third of what the uncapped run kept)
        extra = ["points.max_points=%d" % cap, "points.normals=composited"] if capped else []
        seen.update(kept=0, views=0)
        if os.path.exists(path):
            os.remove(path)
        assert run.main(common + opts + extra) == 0
        print("kept rays: %d of %d views x 768" % (seen["kept"], seen["views"]))
        assert os.path.exists(path) and seen["views"] == seen["n_train"] > 0 and seen["kept"] > 3
        lines, v, rest = _read_ply(path)
        assert rest == b"" and v.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
        assert len(v) == (seen["kept"] if cap is None else len(mesh.stride_subset(seen["kept"], cap))) and (cap is None or len(v) <= cap)
        ln = np.sqrt(v["nx"].astype(F64) ** 2 + v["ny"].astype(F64) ** 2 + v["nz"].astype(F64) ** 2)
        assert ((np.abs(ln - 1) < 1e-5) | (ln == 0)).all()
        assert np.isfinite(np.stack([v["x"], v["y"], v["z"]])).all()
    with pytest.raises(ValueError):
        run.main(common + ["mode=extract_points", "is_continue=true", "points.normals=mesh"])

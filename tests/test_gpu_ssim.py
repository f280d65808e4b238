"""SSIM on the MI355X (csrc/dataset.hip, host/RendererQuery.cpp ImageSSIM, metrics.py): the bodies of tests/test_ssim_cpu.py against the device
through host.image_ssim and capi.image_ssim, each twice in a row (a statistics buffer that the call did not zero shows on the second),
bit for bit with the numpy restatement (tests/ssim_ref.py); runner.test_image_metrics on the fox scene at 135 x 240 and its lack of effect
on training; the launcher's test.ssim / test.write_images against metrics.compare_dirs over the files it wrote."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ssim_ref as sr  # noqa: E402
import test_ssim_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    return runtime


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=F32, order="C")).cuda()


def _ssim(mod, window):
    def ssim(a, b, return_map=False, **kw):
        mean, per, m = mod.image_ssim(_dev(a), _dev(b), return_map=return_map, **kw)
        assert (m is None) == (not return_map) and per.dtype == torch.float64 and not per.is_cuda
        return float(mean), per.numpy(), None if m is None else m.cpu().numpy()
    return cpu.Ssim(window, ssim)


@pytest.fixture(scope="module")
def impls(rt):
    from f2_nerf_amd import capi
    window = lambda fs, sigma: np.array(capi.ssim_window(fs, sigma), np.float64)  # noqa: E731  (the one f2n_ssim_window of the library)
    return _ssim(rt.host(), window), _ssim(capi, window)


@pytest.mark.parametrize("case", cpu.CASES, ids=lambda c: "%dx%dx%d_fs%d" % c[:4])
def test_device_matches_the_restatement(impls, case):
    host, capi = impls
    cpu.check_case(host, case)
    cpu.check_case(host, case, seed=1)  # twice in a row
    cpu.check_case(capi, case)
    cpu.check_case(capi, case, seed=1)


def test_more_tile_rows_than_a_grid_has_in_y(impls):
    cpu.check_case(impls[0], cpu.TALL)


def test_window_identical_pair_and_nan_pixel(impls):
    host, capi = impls
    assert cpu.check_window(host) <= cpu.WINDOW_BAR
    for S in impls:
        cpu.check_identical(S)
        cpu.check_nan_pixel(S)
        cpu.check_nan_pixel(S)


def test_shape_rules_raise(rt):
    from f2_nerf_amd import capi
    a = torch.zeros((16, 16, 3), device="cuda")
    for mod in (rt.host(), capi):
        assert mod.image_ssim(a, a)[0] == 1.0
        for bad in (dict(filter_size=17), dict(filter_size=0), dict(filter_size=34), dict(filter_sigma=0.0), dict(filter_sigma=float("nan"))):
            with pytest.raises(ValueError) as e:
                mod.image_ssim(a, a, **bad)
            assert "filter_size in [1, 33]" in str(e.value) and "C in [1, 4]" in str(e.value)
        for x, y in ((a[:, :, :0], a[:, :, :0]), (torch.zeros((16, 16, 5), device="cuda"),) * 2, (a, a[:15]), (a[0], a[0]), (a.double(), a.double())):
            with pytest.raises(ValueError):
                mod.image_ssim(x, y)


def test_metrics_module(impls, tmp_path):
    """metrics.ssim on numpy and torch images, metrics.compare_dirs with the device behind it"""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import metrics
    host, _ = impls
    a, b = cpu.image_pair(40, 52, 3, 1)
    want = sr.ssim(a, b, w=host.window(11, 1.5))
    assert metrics.ssim(a, b) == want == metrics.ssim(torch.from_numpy(a), torch.from_numpy(b).cuda()) == metrics.ssim(a.astype(np.float64), b)
    mean, m = metrics.ssim(a, b, filter_size=4, filter_sigma=1.0, return_map=True)
    assert isinstance(m, np.ndarray) and cpu.same(m, sr.ssim_map(a, b, host.window(4, 1.0), *sr.constants())) and mean == sr.ssim(a, b, filter_size=4, w=host.window(4, 1.0))
    cpu.check_compare_dirs(tmp_path, metrics.ssim)
    assert metrics.main([str(tmp_path / "gt")]) == 2


# ---- the fox scene -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fox(rt):
    from f2_nerf_amd import fox_data
    sc, images = fox_data.scene(8)  # 135 x 240
    return fox_data.load_state(), sc, images, rt.make_dataset(sc, images.cuda())


def test_image_metrics_on_the_fox(rt, fox, impls):
    st, sc, images, ds = fox
    runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=14"], seed=3, table_init=0.3)
    idx = int(sc["test_set"][0])
    H, W = (int(v) for v in sc["image_hw"])
    psnr = runner.test_image_psnr(ds, idx)
    m = runner.test_image_metrics(ds, idx)
    assert set(m) == {"psnr", "ssim", "pred", "disp", "oct_disp"}
    assert np.float32(m["psnr"]).tobytes() == np.float32(psnr).tobytes()
    pred, gt = m["pred"].cpu().numpy(), images[idx].numpy()
    assert pred.shape == (H, W, 3) and m["disp"].shape == (H, W, 1) and m["oct_disp"].shape == (H, W, 1)
    assert cpu.same(pred, ((pred * 255.0 + 0.5).astype(np.uint8) / F32(255.0)).astype(F32))  # quantised: k / 255 in fp32
    img = runner.render_whole_image(*ds.rays_of_camera(idx))
    assert torch.equal((m["pred"].reshape(-1, 3) * 255. + .5).to(torch.uint8), (img[0].clip(0, 1) * 255.).to(torch.uint8))
    assert torch.equal(m["oct_disp"].reshape(-1, 1), img[1]) and torch.equal(m["disp"].reshape(-1, 1), img[2])
    want = sr.ssim(pred, gt, w=impls[0].window(11, 1.5))
    print("fox view %d at %dx%d, untrained field: psnr %.3f ssim %.6f" % (idx, H, W, psnr, m["ssim"]))
    assert m["ssim"] == want and 0.0 < want < 1.0
    assert runner.test_image_metrics(ds, idx)["ssim"] == want


def test_image_metrics_have_no_effect_on_training(rt, fox):
    st, sc, images, ds = fox
    rng = np.random.default_rng(5)
    batches = [rt.to_dev(*rt.synthetic_ray_batch(st, 4096, rng)) for _ in range(6)]

    def run(measure):
        runner, cfg, _ = rt.make_runner(st, "wanjinyou", ["field.log2_table_size=15"], seed=3, table_init=0.3)
        runner.n_edge_pts = 512
        losses = []
        for k, b in enumerate(batches):
            if measure and k == 3:
                assert np.isfinite(runner.test_image_metrics(ds, int(sc["test_set"][1]))["ssim"])
            ro, rd, bounds, gt, cam = b
            s = runner.train_step(ro, rd, bounds, gt, cam, True)
            losses.append((float(s["loss"]), float(s["mse"])))
        runner.flush()
        return losses, [x.detach().cpu().numpy().copy() for x in runner.states()]

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    assert len(s0) == len(s1) and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(s0, s1))


# ---- the launcher ------------------------------------------------------------------------------------------------------------------
def test_launcher_writes_ssim_and_images(tmp_path, capsys):
    """The synthetic rig of tests/test_gpu_mesh_texture.py's launcher test: mode=test with test.ssim=true test.write_images=true adds ssim /
    mean_ssim to info.yaml and writes the reference's three PNGs per test view; metrics.compare_dirs over the colour files and the
    ground-truth PNGs gives mean_ssim exactly and the PSNRs to fp32 rounding; without the options info.yaml and the output are the old."""
    import yaml
    from PIL import Image
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import metrics, rigs, run
    rng = np.random.default_rng(2)
    meta, hw = rigs.forward_facing(rng, n_side=(5, 4), hw=(48, 64), focal=56.0)
    meta[:, 12:14] *= 4.0; meta[:, 14] *= 4.0; meta[:, 16:18] *= 4.0
    data = tmp_path / "data" / "synth" / "rig"
    (data / "images_4").mkdir(parents=True)
    np.save(data / "cams_meta.npy", meta)
    photos = []
    yy, xx = np.mgrid[0:48, 0:64]
    for i in range(len(meta)):  # smooth pictures with a little noise: the images SSIM is about
        base = 127 + 90 * np.sin(0.2 * xx[..., None] + 0.15 * yy[..., None] + 0.9 * np.arange(3) + i)
        photos.append(np.clip(base + rng.integers(-6, 7, (48, 64, 3)), 0, 255).astype(np.uint8))
        Image.fromarray(photos[-1]).save(data / "images_4" / ("%03d.png" % i))
    common = ["--config-name=llff", "dataset_name=synth", "case_name=rig", "exp_name=t", "+work_dir=%s" % tmp_path,
              "field.log2_table_size=14", "train.end_iter=60", "train.save_freq=30", "train.learning_rate_warm_up_end_iter=10",
              "pts_sampler.sub_div_milestones=[20]", "pts_sampler.compact_freq=25", "train.pts_batch_size=32768"]
    out_dir = tmp_path / "exp" / "rig" / "t" / "test_images"
    assert run.main(common + ["mode=train"]) == 0
    plain_train = yaml.safe_load(open(out_dir / "info.yaml"))
    capsys.readouterr()
    assert run.main(common + ["mode=test", "is_continue=true"]) == 0
    plain_out = capsys.readouterr().out
    plain = yaml.safe_load(open(out_dir / "info.yaml"))
    plain_text = open(out_dir / "info.yaml").read()
    views = sorted(k for k in plain if k != "mean_psnr")
    assert plain == plain_train and len(views) >= 2 and all(isinstance(plain[k], float) for k in plain)
    assert "Mean ssim" not in plain_out and not [p for p in os.listdir(out_dir) if p.endswith(".png")]
    # ssim alone: the old keys with the old values, two new ones, one new line, no image
    assert run.main(common + ["mode=test", "is_continue=true", "test.ssim=true"]) == 0
    out = capsys.readouterr().out
    info = yaml.safe_load(open(out_dir / "info.yaml"))
    assert set(info) == set(plain) | {"ssim", "mean_ssim"} and all(info[k] == plain[k] for k in plain)
    order = [str(k) for k in sorted(int(v) for v in views)]  # the test set's order: the launcher sums in it
    assert set(info["ssim"]) == set(views) and info["mean_ssim"] == sum(info["ssim"][k] for k in order) / len(views)
    means = lambda text: [ln for ln in text.split("\n") if ln.startswith("Mean ")]  # noqa: E731
    assert means(plain_out) == ["Mean psnr: %s" % plain["mean_psnr"]] and means(out) == means(plain_out) + ["Mean ssim: %s" % info["mean_ssim"]]
    assert len(out.split("\n")) == len(plain_out.split("\n")) + 1 and not [p for p in os.listdir(out_dir) if p.endswith(".png")]
    # both: the same numbers and the reference's file names
    assert run.main(common + ["mode=test", "is_continue=true", "test.ssim=true", "test.write_images=true"]) == 0
    capsys.readouterr()
    assert yaml.safe_load(open(out_dir / "info.yaml")) == info
    colour = [str(out_dir / ("color_60_%03d.png" % int(k))) for k in sorted(int(v) for v in views)]
    for k in views:
        for name in ("color", "depth", "oct_depth"):
            img = np.asarray(Image.open(out_dir / ("%s_60_%03d.png" % (name, int(k)))))
            assert img.shape == (48, 64, 3) and img.dtype == np.uint8
            assert name == "color" or ((img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all())
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    for k in views:
        Image.fromarray(photos[int(k)]).save(gt_dir / ("%03d.png" % int(k)))
    cmp_ = metrics.compare_dirs(str(gt_dir), str(out_dir), pred_files=colour)
    assert [cmp_["ssim"][str(i)] for i in range(len(order))] == [info["ssim"][k] for k in order]
    # (the launcher sums in the test set's order, compare_dirs in the files': both ascending here)
    assert cmp_["ssim"]["mean"] == info["mean_ssim"]
    # The launcher's PSNR is the fp32 evaluation of the same mean square (ExpRunner::TestImagePSNR): a difference of two k / 255 carries
    # two roundings of 2^-24 relative to values below 1, so the mean square m is off by at most 2 sqrt(m) 2^-23 plus the fp32 summation
    # (taken as 2^-18 relative: 9216 addends, pairwise), and 20 log10 turns a relative error e of m into 4.35 e dB.  For a PSNR below 40 dB
    # (sqrt(m) >= 0.01) that is 4.35 (2.4e-5 + 3.8e-6) = 1.2e-4 dB, plus the fp32 rounding of the result (40 x 2^-24): 1.3e-4 dB.
    for i, k in enumerate(order):
        assert info[k] < 40.0 and abs(cmp_["psnr"][str(i)] - info[k]) <= 1.3e-4, (cmp_["psnr"][str(i)], info[k])
    with capsys.disabled():
        print("launcher: mean_psnr %.3f mean_ssim %.6f over %d views" % (info["mean_psnr"], info["mean_ssim"], len(views)))
    # images alone: the old info.yaml byte for byte
    assert run.main(common + ["mode=test", "is_continue=true", "test.write_images=true"]) == 0
    assert open(out_dir / "info.yaml").read() == plain_text and "Mean ssim" not in capsys.readouterr().out

#!/usr/bin/env python3
"""Launcher of the hot path: what scripts/run.py (hydra composition, image list, runtime_config.yaml) + main.cpp
(torch::manual_seed(2022), ExpRunner(conf).Execute()) + ExpRunner::Execute (ExpRunner.cpp:385-399) do in the reference.

    python -m f2_nerf_amd.run --config-name=wanjinyou dataset_name=example case_name=ngp_fox mode=train +work_dir=$(pwd)
    python -m f2_nerf_amd.run --config-name=wanjinyou ... mode=render_path is_continue=true

  * config: `--config-name NAME` composes NAME.yaml of a hydra-style directory (`--config-dir`, e.g. the reference's confs/)
    or, without a directory, the built-in copy of the shipped experiment files (config.PRESETS); `key=value` / `+key=value`
    are hydra-style overrides.  The composed config is written to <exp>/record/runtime_config.yaml like the reference does.
  * data: <work_dir>/data/<dataset_name>/<case_name>/{cams_meta.npy, images[_<factor>]/*.jpg|png, (poses_render.npy),
    (split.npy)} -- the reference's layout (Dataset.cpp:16-146); NormalizeScene, bounds relaxation and the 8th-image test split
    are applied as there; images are decoded with PIL and kept resident in HBM.
  * modes (ExpRunner::Execute): train (ExpRunner::Train with checkpoints every save_freq and the final TestImages),
    test (TestImages of the latest checkpoint; with test.distortion=true info.yaml gains `distortion: {view: mean}` and
    `mean_distortion`, the distortion loss of the views' rays on their warped intervals; with test.ssim=true `ssim: {view: value}` and `mean_ssim` -- the
    reference's rgb_ssim of scripts/eval.py on the device, metrics.py -- and with test.write_images=true the reference's
    test_images/color_<iter>_<idx>.png, depth_... and oct_depth_... are written), render_path (RenderPath over poses_render.npy), extract_mesh (with is_continue:
    <exp>/meshes/<iter>_<res>.ply, the density iso-surface in the data set's world frame, or with mesh.source=tsdf the surface fused from
    the training views' rendered depth; with mesh.sparse=true|4|8|16 the same density mesh from the non-empty bricks of the box only,
    mesh.resolution up to 8192; mesh.py), extract_points (with
    is_continue: <exp>/points/<iter>.ply, the training views' surface points with normals and colours; mesh.py).  Image files are written with
    PIL; everything per-ray runs in the C++/HIP host (there is no Python in the training loop: ExpRunner::Train).
  * data-parallel training (the reference is single-GPU): launched as N ranks -- `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 -m f2_nerf_amd.run ...` -- every rank builds the same scene from the same seed, the
    C++ host attaches its RCCL communicator (parallel.attach: rank 0's state is broadcast, gradients are averaged and occupancy
    votes max-combined inside TrainStep) and draws its own rays / noise / background (host/KeyedDraws.h: a stream per rank), so one
    iteration trains on N x pts_batch_size samples; rank 0 writes checkpoints, logs and test images.  NOT run on hardware in this
    build (every lease had one GPU): the same exchange is what bench.py --gpus N times.
File IO and the command line are outside the hot path proper; this module exists so that a user of the
reference finds the same entry point."""
import glob
import os
import sys
import time

import numpy as np


def parse_args(argv):
    name, conf_dir, overrides = "wanjinyou", None, []
    for a in argv:
        if a.startswith("--config-name"):
            name = a.split("=", 1)[1] if "=" in a else None
        elif a.startswith("--config-dir"):
            conf_dir = a.split("=", 1)[1] if "=" in a else None
        elif "=" in a:
            overrides.append(a.lstrip("+"))
        elif name is None:
            name = a
        elif conf_dir is None and os.path.isdir(a):
            conf_dir = a
    return name, conf_dir, overrides


def image_list(data_path, factor):
    """scripts/run.py:22-36."""
    pats = ["*.jpg", "*.png", "*.JPG", "*.jpeg"]
    dirs = ["images", "images_1"] if 0.999 < factor < 1.001 else ["images_%d" % int(np.round(factor))]
    files = []
    for d in dirs:
        for p in pats:
            files += glob.glob(os.path.join(data_path, d, p))
    if not files:
        raise FileNotFoundError("No image found under %s (%s)" % (data_path, dirs))
    return sorted(files)


def load_dataset(cfg, data_path):
    """Dataset::Dataset (Dataset.cpp:16-146) up to the tensors the host Dataset keeps resident."""
    import torch
    from PIL import Image
    from . import rigs, runtime
    factor = float(cfg["dataset"]["factor"])
    meta = np.load(os.path.join(data_path, "cams_meta.npy"))
    files = image_list(data_path, factor)
    first = np.asarray(Image.open(files[0]).convert("RGB"))
    sc = rigs.prepare_scene(meta, first.shape[:2], factor, tuple(float(v) for v in cfg["dataset"]["bounds_factor"]),
                            intrinsics_already_scaled=False)
    n = len(sc["poses"])
    if len(files) != n:
        raise ValueError("%d images for %d cameras" % (len(files), n))
    images = np.stack([np.asarray(Image.open(f).convert("RGB"), np.uint8) for f in files])
    sp = os.path.join(data_path, "split.npy")
    if os.path.exists(sp):  # Dataset.cpp:92-104
        st = np.load(sp).astype(np.uint8)
        sc["train_set"] = np.nonzero(st & 1)[0].astype(np.int32)
        sc["test_set"] = np.nonzero(st & 2)[0].astype(np.int32)
    rp = os.path.join(data_path, "poses_render.npy")
    if os.path.exists(rp):  # Dataset.cpp:55-70
        poses = np.load(rp).astype(np.float32).reshape(-1, 3, 4)
        poses[:, :3, 3] = (poses[:, :3, 3] - sc["center"][None]) / sc["radius"]
        sc["render_poses"] = poses
    ds = runtime.make_dataset(sc, torch.from_numpy(images.astype(np.float32) / np.float32(255.)))
    return sc, ds


def save_png(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    a = (img.detach().clamp(0, 1) * 255.).to("cpu").numpy().astype(np.uint8)
    Image.fromarray(a).save(path)


def main(argv=None):
    import torch
    from . import config, runtime
    name, conf_dir, overrides = parse_args(sys.argv[1:] if argv is None else argv)
    cfg = config.compose_yaml(conf_dir, name, overrides) if conf_dir else config.preset(name, overrides)
    base_dir = cfg.get("work_dir", os.getcwd())
    data_path = os.path.join(base_dir, "data", str(cfg.get("dataset_name", "example")), str(cfg["case_name"]))
    exp_dir = os.path.join(base_dir, "exp", str(cfg["case_name"]), str(cfg["exp_name"]))
    os.makedirs(os.path.join(exp_dir, "record"), exist_ok=True)
    cfg.setdefault("dataset", {})["data_path"] = data_path
    cfg["base_dir"], cfg["base_exp_dir"] = base_dir, exp_dir
    import yaml
    with open(os.path.join(exp_dir, "record", "runtime_config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    print("Working directory is", base_dir)
    # one process per GPU when launched by torch.distributed.run (see the module docstring); a plain launch is rank 0 of 1
    world, rank, local_rank = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    dev = "cuda:%d" % local_rank
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        # (the ranks' last rendezvous waits for rank 0's test / path renders: minutes at full resolution -- the default watchdog of ten
        # minutes would abort a healthy job; round-5 advisor)
        dist.init_process_group("nccl", device_id=torch.device(dev), timeout=datetime.timedelta(hours=6))
    torch.cuda.set_device(dev)
    torch.manual_seed(2022)  # main.cpp:9 (the same on every rank: the replicas' octree and parameters come from it)
    sc, ds = load_dataset(cfg, data_path)
    runner, cfg, built = runtime.make_runner_from_cameras(sc["poses"], sc["intri"], sc["bounds"], sc["train_set"], cfg=cfg, device=dev)
    if world > 1:
        from . import parallel
        parallel.attach(runner, int(cfg["field"]["log2_table_size"]))
    ck_latest = os.path.join(exp_dir, "checkpoints", "latest")
    if bool(cfg.get("is_continue", False)):  # ExpRunner.cpp:56-58
        runner.load_checkpoint(ck_latest)
    mode = str(cfg.get("mode", "train"))

    def save_checkpoint():  # ExpRunner.cpp:205-219
        if rank != 0:  # (replicas are identical: one writer)
            return
        d = os.path.join(exp_dir, "checkpoints", "%08d" % runner.iter_step)
        os.makedirs(d, exist_ok=True)
        runner.save_checkpoint(d)
        os.makedirs(ck_latest, exist_ok=True)
        for f in ("renderer.pt", "scalars.pt"):
            link = os.path.join(ck_latest, f)
            if os.path.lexists(link):
                os.remove(link)
            os.symlink(os.path.join(d, f), link)

    from . import metrics
    topt = metrics.launcher_options(cfg)  # (test.ssim / test.write_images / test.distortion: a bad value raises before anything is trained or rendered)

    def test_images():  # ExpRunner.cpp:343-383
        if rank != 0:
            return None
        ssims = {}
        if not (topt["ssim"] or topt["write_images"]):
            views = [float(v) for v in runner.test_images(ds)]
        else:  # one render per view gives the PSNR, the SSIM and the three images the reference writes (ExpRunner.cpp:353-379)
            from . import mesh
            views, acc = [], np.float32(0.)
            for i in sc["test_set"]:
                m = runner.test_image_metrics(ds, int(i))
                views.append(float(m["psnr"]))
                acc = np.float32(acc + np.float32(m["psnr"]))  # (ExpRunner::TestImages' own float sum)
                ssims[str(int(i))] = float(m["ssim"])
                if topt["write_images"]:
                    # Utils::WriteImageTensor truncates (x * 255); pred holds k / 255 in fp32 and its file must hold that k, so it is rounded
                    for name, img, half in (("color", m["pred"], .5), ("depth", m["disp"].repeat(1, 1, 3), 0.), ("oct_depth", m["oct_disp"].repeat(1, 1, 3), 0.)):
                        u8 = (img.detach().clamp(0, 1) * 255. + half).to(torch.uint8).cpu().numpy()
                        mesh.write_png(os.path.join(exp_dir, "test_images", "%s_%d_%03d.png" % (name, runner.iter_step, int(i))), u8)
            views.append(float(acc / np.float32(len(views))) if views else 0.)
        out = {str(int(i)): p for i, p in zip(sc["test_set"], views[:-1])}
        out["mean_psnr"] = views[-1]
        if topt["ssim"]:
            out["ssim"] = ssims
            out["mean_ssim"] = sum(ssims.values()) / len(ssims) if ssims else 0.
        if topt["distortion"]:  # the mean over a view's rays of runner.ray_distortion (the distortion loss on the warped intervals)
            dist = {}
            for i in sc["test_set"]:
                co, cd, cb = ds.rays_of_camera(int(i))
                dist[str(int(i))] = float(runner.ray_distortion(co, cd, cb).mean(dtype=torch.float64))
            out["distortion"] = dist
            out["mean_distortion"] = sum(dist.values()) / len(dist) if dist else 0.
        os.makedirs(os.path.join(exp_dir, "test_images"), exist_ok=True)
        with open(os.path.join(exp_dir, "test_images", "info.yaml"), "w") as f:
            yaml.safe_dump(out, f)
        print("Mean psnr: %s" % views[-1])
        if topt["ssim"]:
            print("Mean ssim: %s" % out["mean_ssim"])
        if topt["distortion"]:
            print("Mean distortion: %s" % out["mean_distortion"])
        return out

    try:
        if rank != 0 and mode != "train":
            pass  # (the rendering modes are one rank's work; the others wait at the barrier below)
        elif mode == "train":
            t = cfg["train"]
            end, save_freq, report = int(t["end_iter"]), int(t["save_freq"]), int(t["report_freq"])
            t0 = time.time()
            psnr_smooth = -1.0
            while runner.iter_step < end:
                # the native loop runs up to the next report / checkpoint boundary (ExpRunner.cpp:157-172); the reference smooths
                # the PSNR over every iteration (one host read-back each: :120-122) -- here the loss stays on the device inside
                # the loop, so the same 0.9 / 0.1 smoothing is applied over the report boundaries' batches instead
                nxt = min(end, (runner.iter_step // report + 1) * report, (runner.iter_step // save_freq + 1) * save_freq)
                s = runner.train(ds, nxt, 1)
                if rank == 0 and (runner.iter_step % report == 0 or runner.iter_step >= end):
                    torch.cuda.synchronize()
                    mse = max(float(s["mse"]), 1e-12)
                    psnr = 20 * np.log10(1 / np.sqrt(mse))
                    psnr_smooth = psnr if psnr_smooth < 0 else psnr * .1 + psnr_smooth * .9
                    # (labelled differently from the reference's per-iteration EMA, with which it is not comparable line by line)
                    print("Iter: %6d PSNR(report-batch EMA): %.2f NRays: %5d OctSamples: %.1f Samples: %.1f MeaningfulSamples: %.1f IPS: %.1f LR: %.4f" % (
                        runner.iter_step, psnr_smooth, s["n_rays"], runner.oct_per_ray, runner.sampled_per_ray,
                        runner.meaningful_per_ray, runner.iter_step / max(time.time() - t0, 1e-9), runner.cur_lr), flush=True)
                if runner.iter_step % save_freq == 0:
                    save_checkpoint()
            if rank == 0:
                with open(os.path.join(exp_dir, "train_info.txt"), "w") as f:
                    f.write("%f\n" % (time.time() - t0))
                print("Train done, test.")
            test_images()
        elif mode == "test":
            test_images()
        elif mode == "render_path":
            if "render_poses" not in sc:
                raise FileNotFoundError("poses_render.npy not found under " + data_path)
            runner.render_path(ds, torch.from_numpy(sc["render_poses"]),
                               lambda i, img: save_png(os.path.join(exp_dir, "novel_images", "%d_%03d.png" % (runner.iter_step, i)), img), 1)
        elif mode == "render_all":  # ExpRunner::RenderAllImages (ExpRunner.cpp:295-299): every image of the data set, as VisualizeImage writes it
            for idx in range(int(ds.n_images)):
                save_png(os.path.join(exp_dir, "images", "%d_%d.png" % (runner.iter_step, idx)), runner.visualize_image(ds, idx))
        elif mode == "extract_mesh":  # no reference counterpart: <exp>/meshes/<iter>_<res>.ply (mesh.py; options mesh.*)
            from . import mesh
            mesh.texture_options(cfg)  # (mesh.texture / texture.*: a bad value raises before anything is extracted or written)
            # (the TSDF is fused from renders of the training cameras, mesh.check casts their rays at the mesh, and the views colour
            # sources project into them: all need them)
            views = mesh.view_color_options(cfg)["color_source"] == "views" or mesh.texture_options(cfg)["source"] == "views"
            if mesh.options(cfg)["source"] == "tsdf" or mesh.check_options(cfg)["check"] or views:
                mesh.extract(runner, cfg, sc, exp_dir, dataset=ds)
            else:
                mesh.extract(runner, cfg, sc, exp_dir)
        elif mode == "extract_points":  # no reference counterpart: <exp>/points/<iter>.ply (mesh.py; options points.*)
            from . import mesh
            mesh.extract_points(runner, cfg, sc, ds, exp_dir)
        else:
            raise ValueError("unknown mode: %s" % mode)
    finally:
        # every rank reaches the rendezvous, also when its own work threw: the others are waiting there (rank 0 renders alone)
        if world > 1:
            try:
                runner.flush()
            finally:
                dist.barrier()
                dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())

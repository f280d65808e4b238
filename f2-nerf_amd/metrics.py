"""Image-quality metrics of test renders: what the reference's scripts/eval.py computes over folders of PNGs, without skimage, scipy or
lpips.

  ssim(a, b, **kw)          the reference's rgb_ssim (eval.py:29-75, the mip-NeRF definition) on the device: host.image_ssim, an fp64
                            kernel with a fixed order of operations and an exact integer mean (include/f2n_abi.h, f2n_image_ssim).
                            numpy or torch images [H,W,C] in, a float out (return_map=True: (float, map [H-fs+1,W-fs+1,C] float64)).
  psnr_u8(a, b)             skimage's peak_signal_noise_ratio of two uint8 images: 10 log10(255^2 / mse), in fp64.
  compare_dirs(gt, pred)    eval.py:86-117 for one pair of folders: sorted file lists, [:, :, :3], per-image psnr / ssim under str(i), their
                            means under "mean"; written to <pred>/info.json and returned.

    python -m f2_nerf_amd.metrics GT_DIR PRED_DIR

LPIPS is not computed: it needs the VGG weights of the lpips package, which this project does not ship; there is no "lpips" key.
There is no CPU path: ssim needs the device."""
import glob
import json
import os
import sys

import numpy as np


def launcher_options(cfg):
    """test.ssim, test.write_images and test.distortion of the launcher (run.py): all off unless asked for."""
    from .mesh import _flag
    t = cfg.get("test") or {}
    return {"ssim": _flag(t.get("ssim", False)), "write_images": _flag(t.get("write_images", False)),
            "distortion": _flag(t.get("distortion", False))}


def ssim(a, b, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    import torch
    from . import runtime
    ta, tb = (x.detach() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in (a, b))
    ta, tb = (x.to(torch.float32).cuda().contiguous() for x in (ta, tb))
    mean, _, m = runtime.host().image_ssim(ta, tb, float(max_val), int(filter_size), float(filter_sigma), float(k1), float(k2), bool(return_map))
    if not return_map:
        return float(mean)
    return float(mean), (m if torch.is_tensor(a) else m.cpu().numpy())


def psnr_u8(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape != b.shape:
        raise ValueError("psnr_u8: two uint8 images of one shape")
    with np.errstate(divide="ignore"):
        mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2, dtype=np.float64)
        return float(10 * np.log10((255.0 ** 2) / mse))


def glob_images(image_dir):
    """eval.py:16-20"""
    ret = []
    for suff in ["*.jpg", "*.JPG", "*.png", "*.PNG"]:
        ret += glob.glob(os.path.join(image_dir, suff))
    return sorted(ret)


def _read(path):
    from PIL import Image
    img = Image.open(path)
    if img.mode not in ("RGB", "RGBA"):
        img = img.convert("RGB")
    return np.asarray(img, np.uint8)[:, :, :3]


def compare_dirs(gt_dir, pred_dir, ssim_fn=None, pred_files=None):
    """pred_files: the prediction files in place of every image of pred_dir (the launcher's folder also holds depth images).
    ssim_fn(a, b) on float64 images in [0, 1]: in place of ssim (the tests' emulated kernel)."""
    ssim_fn = ssim if ssim_fn is None else ssim_fn
    gt_paths = glob_images(gt_dir)
    pd_paths = glob_images(pred_dir) if pred_files is None else list(pred_files)
    if len(gt_paths) != len(pd_paths) or not gt_paths:
        raise ValueError("compare_dirs: %d ground-truth images in %s, %d predictions in %s" % (len(gt_paths), gt_dir, len(pd_paths), pred_dir))
    info = {"psnr": {}, "ssim": {}}
    psnr_tot, ssim_tot = 0.0, 0.0
    for i, (gt_path, pd_path) in enumerate(zip(gt_paths, pd_paths)):
        gt, pd = _read(gt_path), _read(pd_path)
        if gt.shape != pd.shape:
            raise ValueError("compare_dirs: %s is %s, %s is %s" % (gt_path, gt.shape, pd_path, pd.shape))
        p = psnr_u8(gt, pd)
        s = float(ssim_fn(gt / 255.0, pd / 255.0))
        psnr_tot += p
        ssim_tot += s
        info["psnr"][str(i)] = p
        info["ssim"][str(i)] = s
    info["psnr"]["mean"] = psnr_tot / len(gt_paths)
    info["ssim"]["mean"] = ssim_tot / len(gt_paths)
    with open(os.path.join(pred_dir, "info.json"), "w") as f:
        json.dump(info, f, indent=2)
    return info


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        print("usage: python -m f2_nerf_amd.metrics GT_DIR PRED_DIR", file=sys.stderr)
        return 2
    info = compare_dirs(argv[0], argv[1])
    print("psnr %.4f ssim %.4f over %d images -> %s" % (info["psnr"]["mean"], info["ssim"]["mean"], len(info["psnr"]) - 1,
                                                         os.path.join(argv[1], "info.json")))
    return 0


if __name__ == "__main__":
    sys.exit(main())

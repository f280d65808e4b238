#!/usr/bin/env python3
"""Records tests/golden/ssim_reference.npz: small float32 image pairs and the SSIM maps that the reference's own rgb_ssim
(scripts/eval.py:29-75) returns for them -- the data tests/test_ssim_cpu.py holds the numpy restatement (tests/ssim_ref.py) against.
The function is read in place: its text is cut out of the reference's file (the module itself imports lpips and skimage) and run
with numpy and scipy.  Nothing of the reference is copied into the fixture; it holds inputs and results only.

Usage:  python tests/golden/make_ssim_reference.py <the reference's scripts/eval.py>

Pairs: noise, a smooth sinusoid, two flats one grey level apart, an identical pair, 8-bit-quantised images.
Shapes: 11x11, 12x43, 43x44 (C = 3: the reference asserts it).  Filters: 11 (sigma 1.5) for all, 3 and 4 (sigma 1.0) on 12x43 noise."""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(11, 11), (12, 43), (43, 44)]


def pairs(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = np.arange(3)[None, None, :]
    smooth = 0.5 + 0.4 * np.sin(0.11 * xx[..., None] + 0.07 * yy[..., None] + 0.5 * ch)
    smooth_b = 0.5 + 0.4 * np.sin(0.11 * xx[..., None] + 0.07 * yy[..., None] + 0.5 * ch + 0.02)
    noise_a, noise_b = rng.random((h, w, 3)), rng.random((h, w, 3))
    q = lambda z: np.round(np.clip(z, 0, 1) * 255.0) / 255.0  # noqa: E731
    out = {
        "noise": (noise_a, noise_b),
        "smooth": (smooth, smooth_b),
        "flat": (np.full((h, w, 3), 100.0 / 255.0), np.full((h, w, 3), 101.0 / 255.0)),
        "same": (smooth, smooth),
        "quant": (q(smooth), q(smooth + 0.03 * (noise_a - 0.5))),
    }
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in out.items()}


def load_rgb_ssim(path):
    import scipy
    import scipy.signal  # noqa: F401
    with open(path) as f:
        text = f.read()
    fn = [n for n in ast.parse(text).body if isinstance(n, ast.FunctionDef) and n.name == "rgb_ssim"][0]
    ns = {"np": np, "scipy": scipy}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["rgb_ssim"]


def main():
    rgb_ssim = load_rgb_ssim(sys.argv[1])
    rng = np.random.default_rng(20)
    out, names = {}, []
    for h, w in SHAPES:
        for kind, (a, b) in pairs(h, w, rng).items():
            cases = [(11, 1.5)] + ([(3, 1.0), (4, 1.0)] if (h, w) == (12, 43) and kind == "noise" else [])
            for fs, sigma in cases:
                name = "%s_%dx%d_fs%d" % (kind, h, w, fs)
                names.append(name)
                out[name + "/a"], out[name + "/b"] = a, b
                out[name + "/par"] = np.array([fs, sigma], np.float64)
                # (the reference is called with float64 images, as eval.py:100 calls it; the float32 values convert exactly)
                out[name + "/map"] = rgb_ssim(a.astype(np.float64), b.astype(np.float64), 1.0, filter_size=fs, filter_sigma=sigma,
                                              return_map=True)
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "ssim_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()

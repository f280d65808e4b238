"""SSIM without a GPU: the numpy restatement (tests/ssim_ref.py) against maps recorded from the reference's own rgb_ssim
(tests/golden/ssim_reference.npz, scripts/eval.py:29-75); f2n_image_ssim (csrc/dataset.hip) under the wavefront emulator (tests/wave_emul)
against the restatement, bit for bit, map and statistics, with and without the map; the edge cases (identical pair, a NaN pixel, every
INVALID case); f2n_ssim_window against numpy's window; and metrics.compare_dirs over two folders of PNGs.  The bodies take an `Ssim` and
run against the device as well (tests/test_gpu_ssim.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import ssim_ref as sr  # noqa: E402

F32 = np.float32
INVALID = -1  # F2N_ERR_INVALID_ARG
_d, _i = ctypes.c_double, ctypes.c_int
# (a) the restatement against the reference's maps: the largest difference of a map value over the committed fixture was 8.42e-13 (the
# 8-bit-quantised 43x44 pair; measured on the CPU), of a mean 1.6e-13.  The bar is 50 times the first: scipy sums the taps in another
# order, nothing else differs.  Seven orders of magnitude below the fourth decimal that the tables print.
REFERENCE_BAR = 4.2e-11
# (d) f2n_ssim_window against numpy's window over fs = 1 .. 33 and sigma in SIGMAS: the largest difference was 1.11e-16 (one
# ulp of a weight in [0.5, 1), at sigma 0.5: np.sum adds the taps pairwise, the library in ascending order).  Asserted at twice that.
WINDOW_BAR = 2.23e-16
SIGMAS = (0.5, 1.0, 1.5, 2.5, 7.0)
TILE_H, TILE_W = 16, 32  # F2N_SSIM_TILE_H / _W of csrc/dataset.hip; test_tile_constants holds them against f2n_ssim_tile


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    L.f2n_ssim_tile.restype = None
    return L


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ssim_reference.npz")))


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


class EmulError(RuntimeError):
    def __init__(self, name, rc):
        RuntimeError.__init__(self, "%s failed with status %d" % (name, rc))
        self.rc = rc


def emul_window(L, fs, sigma):
    out = np.full(fs, -9.0, np.float64)
    rc = L.f2n_ssim_window(_i(fs), _d(sigma), _vp(out))
    if rc != 0:
        raise EmulError("f2n_ssim_window", rc)
    return out


def emul_raw(L, a, b, w, c1, c2, return_map):
    """(map or None, stats [C,2]) of f2n_image_ssim; stats arrives dirty: the call zeroes it"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    H, W, C = a.shape
    fs = len(w)
    m = np.full((H - fs + 1, W - fs + 1, C), -9.0, np.float64) if return_map else None
    st = np.full((C, 2), 12345, np.int64)
    rc = L.f2n_image_ssim(None, _i(H), _i(W), _i(C), _vp(a), _vp(b), _vp(np.ascontiguousarray(w, np.float64)), _i(fs), _d(c1), _d(c2), _vp(m), _vp(st))
    if rc != 0:
        raise EmulError("f2n_image_ssim", rc)
    return m, st


class Ssim:
    """window(fs, sigma) -> [fs] float64, the library's;  ssim(a, b, return_map=False, **kw) -> (mean, per_channel [C] float64, map or None)
    with kw of host.image_ssim;  raw(a, b, w, c1, c2, return_map) -> (map, stats) or None where the statistics are not exposed"""
    def __init__(self, window, ssim, raw=None):
        self.window, self.ssim, self.raw = window, ssim, raw


def emul_ssim(L):
    """ImageSSIM of csrc/host/RendererQuery.cpp call for call"""
    def ssim(a, b, return_map=False, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
        w = emul_window(L, filter_size, filter_sigma)
        m, st = emul_raw(L, a, b, w, *sr.constants(max_val, k1, k2), return_map)
        mean, per = sr.mean_from_stats(st, (a.shape[0] - filter_size + 1) * (a.shape[1] - filter_size + 1))
        return mean, per, m
    return Ssim(lambda fs, sigma: emul_window(L, fs, sigma), ssim, lambda *a: emul_raw(L, *a))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()


def same_floats(a, b):
    """bit for bit where finite; a value that is not finite must be of the same class (NaN, +inf, -inf): NaN payloads are no one's contract"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    fin = np.isfinite(a)
    return bool((fin == np.isfinite(b)).all() and same(a[fin], b[fin]) and (np.isnan(a) == np.isnan(b)).all() and (a[~fin & ~np.isnan(a)] == b[~fin & ~np.isnan(b)]).all())


# ---- images ------------------------------------------------------------------------------------------------------------------------
def image_pair(h, w, c, seed, kind="mixed"):
    """float32 [h,w,c] pairs: a smooth sinusoid with noise on it, 8-bit-quantised in its lower half (the images that matter are smooth)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.4 * np.sin(0.13 * xx[..., None] + 0.09 * yy[..., None] + 0.7 * np.arange(c)[None, None, :])
    a = base + 0.02 * (rng.random((h, w, c)) - 0.5)
    b = base + 0.05 * (rng.random((h, w, c)) - 0.5)
    if kind == "noise":
        a, b = rng.random((h, w, c)), rng.random((h, w, c))
    q = lambda z: np.round(np.clip(z, 0, 1) * 255.0) / 255.0  # noqa: E731
    a[h // 2:], b[h // 2:] = q(a[h // 2:]), q(b[h // 2:])
    return a.astype(F32), b.astype(F32)


# (h, w, c, fs, sigma): a single output; the fixture's shapes; one output more than a tile in each direction and exactly a tile (both
# with every channel count's neighbours); C = 4; fs = 1, 3, 4, 11, 33
CASES = [(11, 11, 1, 11, 1.5), (12, 43, 3, 11, 1.5), (43, 44, 3, 11, 1.5), (TILE_H + 3, TILE_W + 3, 2, 3, 1.0), (TILE_H + 3, TILE_W + 3, 3, 4, 1.2),
         (13, 14, 4, 3, 0.8), (12, 43, 3, 1, 1.5), (43, 44, 3, 33, 5.0)]


def check_case(S, case, seed=0):
    """map, mean and per-channel means (and the statistics, where exposed) bit for bit with the restatement; the statistics do not depend on
    whether the map is asked for"""
    h, w, c, fs, sigma = case
    a, b = image_pair(h, w, c, seed + 7 * h + w)
    win = S.window(fs, sigma)
    c1, c2 = sr.constants()
    ref = sr.ssim_map(a, b, win, c1, c2)
    rst = sr.stats(ref)
    n = ref.shape[0] * ref.shape[1]
    assert ref.shape == (h - fs + 1, w - fs + 1, c) and (rst[:, 1] == n).all()
    if case[:2] == (TILE_H + 3, TILE_W + 3):
        assert ref.shape[:2] == ((TILE_H + 1, TILE_W + 1) if fs == 3 else (TILE_H, TILE_W))
    want_mean, want_per = sr.mean_from_stats(rst, n)
    for return_map in (True, False):
        mean, per, m = S.ssim(a, b, return_map, filter_size=fs, filter_sigma=sigma)
        assert (m is not None) == return_map
        if return_map:
            assert m.dtype == np.float64 and same(m, ref), np.abs(m - ref).max()
        assert same(np.float64(mean), np.float64(want_mean)) and same(np.asarray(per, np.float64), want_per)
        if S.raw is not None:
            m2, st = S.raw(a, b, win, c1, c2, return_map)
            assert same(st, rst) and (m2 is None or same(m2, ref))
    return want_mean


def check_identical(S):
    """a == b: exactly 1.0 everywhere, stats[c][0] == 2^36 count"""
    for h, w, c, fs in ((43, 44, 3, 11), (20, 37, 4, 4)):
        a, _ = image_pair(h, w, c, 3)
        mean, per, m = S.ssim(a, a.copy(), True, filter_size=fs)
        assert (m == 1.0).all() and mean == 1.0 and (np.asarray(per) == 1.0).all()
        if S.raw is not None:
            _, st = S.raw(a, a.copy(), S.window(fs, 1.5), *sr.constants(), False)
            n = (h - fs + 1) * (w - fs + 1)
            assert (st[:, 1] == n).all() and (st[:, 0] == 2 ** 36 * n).all()
    flat = np.zeros((12, 12, 1), F32)  # all black: 0 / 0 nowhere, (c1 c2) / (c1 c2)
    assert (S.ssim(flat, flat, True)[2] == 1.0).all()


def check_nan_pixel(S):
    """one NaN pixel (and one inf pixel in another channel): only the windows that touch it are not finite, the counts are right, the means
    of those channels and the mean are NaN"""
    h, w, c, fs = 30, 41, 3, 11
    a, b = image_pair(h, w, c, 5)
    a[14, 20, 1] = np.nan
    b[3, 35, 2] = np.inf
    win = S.window(fs, 1.5)
    ref = sr.ssim_map(a, b, win, *sr.constants())
    mean, per, m = S.ssim(a, b, True)
    oh, ow = h - fs + 1, w - fs + 1
    touched = np.zeros((oh, ow, c), bool)
    touched[max(0, 14 - fs + 1):14 + 1, max(0, 20 - fs + 1):20 + 1, 1] = True
    touched[max(0, 3 - fs + 1):3 + 1, max(0, 35 - fs + 1):35 + 1, 2] = True
    assert (np.isfinite(m) == ~touched).all() and same_floats(m, ref)
    assert np.isnan(mean) and np.isfinite(per[0]) and np.isnan(per[1]) and np.isnan(per[2])
    assert same(np.float64(per[0]), sr.mean_from_stats(sr.stats(ref), oh * ow)[1][0])
    mean2, per2, none = S.ssim(a, b, False)
    assert none is None and np.isnan(mean2) and same_floats(per2, per)
    if S.raw is not None:
        for return_map in (True, False):
            _, st = S.raw(a, b, win, *sr.constants(), return_map)
            assert same(st, sr.stats(ref)) and st[:, 1].tolist() == [oh * ow, oh * ow - int(touched[..., 1].sum()), oh * ow - int(touched[..., 2].sum())]


# ---- (a) the restatement against the reference ----------------------------------------------------------------------------------------
def test_restatement_against_the_reference_maps(fixture):
    """largest |restatement - rgb_ssim| over the fixture: 8.42e-13 per map value, 1.6e-13 per mean (printed); bar REFERENCE_BAR = 50 x"""
    z = fixture
    names = [str(n) for n in z["names"]]
    assert len(names) == 17 and {n.split("_")[0] for n in names} == {"noise", "smooth", "flat", "same", "quant"}
    assert {n.split("_")[1] for n in names} == {"11x11", "12x43", "43x44"} and {n.split("fs")[1] for n in names} == {"11", "3", "4"}
    worst, worst_mean, worst_fixed = 0.0, 0.0, 0.0
    for n in names:
        a, b, par, want = z[n + "/a"], z[n + "/b"], z[n + "/par"], z[n + "/map"]
        assert a.dtype == F32 and b.dtype == F32 and want.dtype == np.float64
        got = sr.ssim_map(a, b, sr.window(int(par[0]), float(par[1])), *sr.constants())
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got - want).max()))
        worst_mean = max(worst_mean, abs(float(got.mean()) - float(want.mean())))
        # the fixed-point mean: every addend is rounded to 2^-36, half a unit at most each
        fixed = sr.mean_from_stats(sr.stats(got), got.shape[0] * got.shape[1])[0]
        worst_fixed = max(worst_fixed, abs(fixed - float(want.mean())))
        if n.startswith("same"):
            assert (got == 1.0).all() and fixed == 1.0
    print("restatement against the reference over %d cases: map %.3g, mean %.3g, fixed-point mean %.3g" % (len(names), worst, worst_mean, worst_fixed))
    assert worst <= REFERENCE_BAR and worst_mean <= REFERENCE_BAR
    assert worst_fixed <= REFERENCE_BAR + 2.0 ** -37


# ---- (b) the kernel under the emulator ----------------------------------------------------------------------------------------------
def test_tile_constants(emul):
    th, tw = _i(0), _i(0)
    emul.f2n_ssim_tile(ctypes.byref(th), ctypes.byref(tw))
    assert (th.value, tw.value) == (TILE_H, TILE_W)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d_fs%d" % c[:4])
def test_kernel_matches_the_restatement(emul, case):
    check_case(emul_ssim(emul), case)


# more rows of tiles than a grid's y extent holds (the tiles are numbered along x).  The device runs it (tests/test_gpu_ssim.py); the
# emulator would take two minutes over its 65537 workgroups, and the cases above already cross tile rows and columns.
TALL = (16 * 65535 + 17, 1, 1, 1, 1.5)


def test_fixture_images_through_the_kernel(emul, fixture):
    """the library's window, the reference's images: the kernel's map is the restatement's, and within REFERENCE_BAR of the reference's"""
    S = emul_ssim(emul)
    for n in ("smooth_12x43_fs11", "flat_12x43_fs11", "noise_12x43_fs4"):
        a, b, par, want = (fixture[n + k] for k in ("/a", "/b", "/par", "/map"))
        fs, sigma = int(par[0]), float(par[1])
        mean, per, m = S.ssim(a, b, True, filter_size=fs, filter_sigma=sigma)
        assert same(m, sr.ssim_map(a, b, S.window(fs, sigma), *sr.constants()))
        assert np.abs(m - want).max() <= REFERENCE_BAR and abs(mean - want.mean()) <= REFERENCE_BAR + 2.0 ** -37


def test_schedule_independence(emul):
    """workgroups and waves in another order: the same map and statistics (the sums are integers)"""
    a, b = image_pair(TILE_H + 14, 2 * TILE_W + 13, 3, 9)
    w = emul_window(emul, 11, 1.5)
    base = emul_raw(emul, a, b, w, *sr.constants(), True)
    try:
        for sched in (1, 2):
            emul.wemu_set_schedule(sched)
            m, st = emul_raw(emul, a, b, w, *sr.constants(), True)
            assert same(m, base[0]) and same(st, base[1])
    finally:
        emul.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))


# ---- (c) edge cases ------------------------------------------------------------------------------------------------------------------
def test_identical_pair_is_exactly_one(emul):
    check_identical(emul_ssim(emul))


def test_nan_pixel(emul):
    check_nan_pixel(emul_ssim(emul))


def test_invalid_arguments(emul):
    L = emul
    w = emul_window(L, 11, 1.5)
    a = np.zeros((16, 16, 4), F32)
    st = np.zeros((4, 2), np.int64)
    m = np.zeros((16, 16, 4), np.float64)

    def call(H=16, W=16, C=3, a=a, b=a, w=w, fs=11, m=m, st=st):
        return L.f2n_image_ssim(None, _i(H), _i(W), _i(C), _vp(a), _vp(b), _vp(w), _i(fs), _d(1e-4), _d(9e-4), _vp(m), _vp(st))

    assert call() == 0 and call(m=None) == 0 and call(C=1) == 0 and call(C=4) == 0 and call(fs=1) == 0 and call(H=11, W=11) == 0
    assert call(C=0) == INVALID and call(C=5) == INVALID
    assert call(fs=0) == INVALID and call(fs=34) == INVALID and call(fs=-1) == INVALID
    assert call(H=10) == INVALID and call(W=10) == INVALID  # fs > min(H, W)
    assert call(a=None) == INVALID and call(b=None) == INVALID and call(w=None) == INVALID and call(st=None) == INVALID
    assert call(H=8192 + 10, W=8192 + 11) == INVALID  # (8192)(8193) outputs > 2^26: refused before anything is read
    out = np.zeros(40, np.float64)
    win = lambda fs, sigma, o=out: L.f2n_ssim_window(_i(fs), _d(sigma), _vp(o))  # noqa: E731
    assert win(1, 1.5) == 0 and out[0] == 1.0 and win(33, 1.5) == 0 and win(4, 0.1) == 0
    assert win(0, 1.5) == INVALID and win(34, 1.5) == INVALID and win(-3, 1.5) == INVALID
    assert win(11, 0.0) == INVALID and win(11, -1.0) == INVALID and win(11, float("nan")) == INVALID and win(11, float("inf")) == INVALID
    assert L.f2n_ssim_window(_i(11), _d(1.5), None) == INVALID


# ---- (d) the window ------------------------------------------------------------------------------------------------------------------
def check_window(S):
    worst = 0.0
    for fs in range(1, 34):
        for sigma in SIGMAS:
            w = S.window(fs, sigma)
            assert w.shape == (fs,) and w.dtype == np.float64 and same(w, w[::-1]) and abs(w.sum() - 1.0) < 1e-15
            worst = max(worst, float(np.abs(w - sr.window(fs, sigma)).max()))
    return worst


def test_window_against_numpy(emul):
    """largest |f2n_ssim_window - numpy's window| over fs = 1 .. 33, five sigmas: 1.11e-16 (printed); asserted at twice that"""
    worst = check_window(emul_ssim(emul))
    print("f2n_ssim_window against numpy: max difference %.3g" % worst)
    assert worst <= WINDOW_BAR


# ---- (e) metrics.compare_dirs -------------------------------------------------------------------------------------------------------
def write_dirs(tmp_path, n=3, hw=(24, 31), alpha=False):
    """n ground-truth / prediction PNG pairs; returns the uint8 arrays"""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import mesh
    rng = np.random.default_rng(11)
    gts, pds = [], []
    for i in range(n):
        a, b = image_pair(hw[0], hw[1], 3, 20 + i)
        g, p = (a * 255.0 + 0.5).astype(np.uint8), (b * 255.0 + 0.5).astype(np.uint8)
        if i == 1:
            p = g.copy()  # an identical pair: ssim 1, psnr inf
            p[0, 0, 0] ^= 1
        gts.append(g)
        pds.append(p)
        mesh.write_png(str(tmp_path / "gt" / ("%03d.png" % i)), g)
        mesh.write_png(str(tmp_path / "pred" / ("color_7_%03d.png" % i)), p)
    return gts, pds


def check_compare_dirs(tmp_path, ssim_fn):
    """file order, the JSON layout of eval.py:86-117 without lpips, psnr as skimage's peak_signal_noise_ratio of two uint8 images"""
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import metrics
    gts, pds = write_dirs(tmp_path)
    info = metrics.compare_dirs(str(tmp_path / "gt"), str(tmp_path / "pred"), ssim_fn=ssim_fn)
    assert set(info) == {"psnr", "ssim"} and set(info["psnr"]) == set(info["ssim"]) == {"0", "1", "2", "mean"}
    assert json.load(open(tmp_path / "pred" / "info.json")) == info
    for i, (g, p) in enumerate(zip(gts, pds)):
        mse = np.mean((g.astype(np.float64) - p.astype(np.float64)) ** 2)
        assert info["psnr"][str(i)] == 10 * np.log10(255.0 ** 2 / mse) == metrics.psnr_u8(g, p)
        assert info["ssim"][str(i)] == ssim_fn(g / 255.0, p / 255.0)
    assert info["psnr"]["mean"] == sum(info["psnr"][str(i)] for i in range(3)) / 3
    assert info["ssim"]["mean"] == sum(info["ssim"][str(i)] for i in range(3)) / 3
    assert 0.5 < info["ssim"]["0"] < 1.0 and info["ssim"]["1"] > 0.999
    with pytest.raises(ValueError):
        os.remove(tmp_path / "pred" / "color_7_002.png")
        metrics.compare_dirs(str(tmp_path / "gt"), str(tmp_path / "pred"), ssim_fn=ssim_fn)
    return info


@pytest.fixture(scope="module")
def emul_host(emul):
    """the C++ host layer compiled against the emulated kernel library (tests/wave_emul/wemu_build.py build_host): ImageSSIM on CPU tensors"""
    import importlib.util
    import wemu_build
    path = wemu_build.build_host()  # (it finds libf2n_emul.so through its own rpath: nothing is put into the process's global scope here)
    spec = importlib.util.spec_from_file_location("_f2n_host_emul", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_ssim(mod, window):
    import torch

    def ssim(a, b, return_map=False, **kw):
        mean, per, m = mod.image_ssim(torch.from_numpy(np.array(a, F32)), torch.from_numpy(np.array(b, F32)), return_map=return_map, **kw)
        assert (m is None) == (not return_map) and per.dtype == torch.float64
        return float(mean), per.numpy(), None if m is None else m.numpy()
    return Ssim(window, ssim)


def test_host_wrapper_on_the_emulator(emul, emul_host, tmp_path, monkeypatch):
    """host.image_ssim (ImageSSIM of csrc/host/RendererQuery.cpp) over the emulated kernel: the means it forms from the statistics, the NaN
    rule, the shape rules; then metrics.ssim and metrics.compare_dirs with that module behind runtime.host()"""
    import torch
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import metrics, runtime
    S = host_ssim(emul_host, lambda fs, sigma: emul_window(emul, fs, sigma))
    for case in (CASES[1], CASES[4], CASES[5]):
        check_case(S, case)
        check_case(S, case, seed=1)
    check_identical(S)
    check_nan_pixel(S)
    a = torch.zeros((16, 16, 3))
    for bad in (dict(filter_size=17), dict(filter_size=0), dict(filter_size=34), dict(filter_sigma=0.0)):
        with pytest.raises(ValueError) as e:
            emul_host.image_ssim(a, a, **bad)
        assert "filter_size in [1, 33]" in str(e.value)
    for x, y in ((a[:, :, :0], a[:, :, :0]), (torch.zeros((16, 16, 5)),) * 2, (a, a[:15]), (a[0], a[0]), (a.double(), a.double())):
        with pytest.raises(ValueError):
            emul_host.image_ssim(x, y)
    monkeypatch.setattr(runtime, "_host", emul_host)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    x, y = image_pair(30, 33, 3, 4)
    want = sr.ssim(x, y, w=emul_window(emul, 11, 1.5))
    assert metrics.ssim(x, y) == want == metrics.ssim(torch.from_numpy(x), y.astype(np.float64))
    mean, m = metrics.ssim(x, y, filter_size=4, filter_sigma=1.0, return_map=True)
    assert isinstance(m, np.ndarray) and same(m, sr.ssim_map(x, y, emul_window(emul, 4, 1.0), *sr.constants()))
    check_compare_dirs(tmp_path, metrics.ssim)
    assert metrics.main([str(tmp_path / "gt")]) == 2
    write_dirs(tmp_path)
    assert metrics.main([str(tmp_path / "gt"), str(tmp_path / "pred")]) == 0


def test_compare_dirs(emul, tmp_path):
    """the module's file handling with the emulated kernel alone in the place of the device"""
    S = emul_ssim(emul)
    info = check_compare_dirs(tmp_path, lambda a, b: S.ssim(np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32))[0])
    gts, pds = write_dirs(tmp_path)
    a, b = (gts[0] / 255.0).astype(F32), (pds[0] / 255.0).astype(F32)
    assert info["ssim"]["0"] == sr.mean_from_stats(sr.stats(sr.ssim_map(a, b, S.window(11, 1.5), *sr.constants())), 14 * 21)[0]

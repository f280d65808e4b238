"""Numpy restatement of f2n_ssim_window / f2n_image_ssim (include/f2n_abi.h; the reference's scripts/eval.py:29-75): the window, the SSIM map
with explicit ascending tap loops (every numpy operation below is one fp64 rounding, never an FMA), and the fixed-point statistics.
Test infrastructure: the product has no CPU path."""
import numpy as np

SCALE = 2.0 ** 36


def window(filter_size=11, sigma=1.5):
    """numpy's own window, eval.py:40-45 word for word (np.sum is pairwise: the library sums in ascending order, and its exp is libm's)"""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)
    return filt


def constants(max_val=1.0, k1=0.01, k2=0.03):
    return (k1 * max_val) ** 2, (k2 * max_val) ** 2


def _blur(z, w):
    """down the columns, then along the rows; acc = acc + w[k] * z[. + k] for k ascending from acc = 0"""
    fs = len(w)
    oh, ow = z.shape[0] - fs + 1, z.shape[1] - fs + 1
    v = np.zeros((oh,) + z.shape[1:], np.float64)
    for k in range(fs):
        v = v + w[k] * z[k:k + oh]
    out = np.zeros((oh, ow) + z.shape[2:], np.float64)
    for k in range(fs):
        out = out + w[k] * v[:, k:k + ow]
    return out


def ssim_map(a, b, w, c1, c2):
    """[H-fs+1, W-fs+1, C] float64 from a, b [H,W,C] float32 and the window w [fs] float64"""
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and a.ndim == 3
    w = np.asarray(w, np.float64)
    with np.errstate(all="ignore"):
        x, y = a.astype(np.float64), b.astype(np.float64)
        mu0, mu1 = _blur(x, w), _blur(y, w)
        mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
        s00, s11, s01 = _blur(x * x, w) - mu00, _blur(y * y, w) - mu11, _blur(x * y, w) - mu01
        s00 = np.where(s00 < 0, 0.0, s00)
        s11 = np.where(s11 < 0, 0.0, s11)
        t, m = np.sqrt(s00 * s11), np.abs(s01)
        m = np.where(t < m, t, m)
        s01 = np.where(s01 < 0, -m, m)
        numer = (2.0 * mu01 + c1) * (2.0 * s01 + c2)
        denom = ((mu00 + mu11) + c1) * ((s00 + s11) + c2)
        return numer / denom


def stats(m):
    """[C,2] int64: the sum of llrint(v 2^36) (np.rint: half to even) and the count, over the finite v of every channel"""
    out = np.zeros((m.shape[2], 2), np.int64)
    for c in range(m.shape[2]):
        v = m[:, :, c]
        v = v[np.isfinite(v)]
        out[c, 0] = int(np.rint(v * SCALE).astype(np.int64).sum())
        out[c, 1] = v.size
    return out


def mean_from_stats(st, n_outputs):
    """(mean, per_channel [C]) as the wrappers form them: NaN where a count falls short of the number of outputs"""
    st = np.asarray(st, np.int64)
    per = np.array([float(int(s)) / (SCALE * n_outputs) if int(n) == n_outputs else float("nan") for s, n in st])
    tot = sum(int(s) for s in st[:, 0])
    mean = float(tot) / (SCALE * n_outputs * len(st)) if (st[:, 1] == n_outputs).all() else float("nan")
    return mean, per


def ssim(a, b, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, w=None):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    c1, c2 = constants(max_val, k1, k2)
    m = ssim_map(a, b, window(filter_size, filter_sigma) if w is None else w, c1, c2)
    return mean_from_stats(stats(m), m.shape[0] * m.shape[1])[0]

"""Numpy restatements of the distortion loss on warped ray intervals (include/f2n_abi.h: f2n_distortion_fwd / _bwd, f2n_loss_add_mean).
Not part of the product.

  dist32 / grad32   fp32, one rounding per operation, the running sums in the order the header writes them: what the kernels must
                    produce bit for bit
  dist64 / grad64   the pairwise definition in fp64 from explicit midpoints (O(n^2)): what the O(n) form is held against
  mean_tree         f2n_loss_add_mean's fp64 sum (stride 256, then the tree) and its two fp32 roundings"""
import numpy as np

F32 = np.float32
HALF, TWO = F32(0.5), F32(2.0)
THIRD = F32(1.0) / F32(3.0)
TWO_THIRDS = F32(2.0) / F32(3.0)


def _ray32(w, dt, dd):
    """(dist, g [n], D [n]) of one ray, fp32 throughout (numpy scalars of type float32 round after every operation)"""
    n = len(w)
    w = np.asarray(w, F32)
    dt = np.asarray(dt, F32)
    D = np.zeros(n, F32)
    g = np.zeros(n, F32)
    P, Dk, dist = F32(0), F32(0), F32(0)
    with np.errstate(all="ignore"):
        for k in range(n):
            h = HALF * (dt[k - 1] + dt[k]) if k > 0 else F32(0)
            if k > 0:
                P = P + w[k - 1]
            Dk = Dk + P * h
            D[k] = Dk
            l = w[k] * (TWO * Dk) + ((w[k] * w[k]) * dt[k]) * THIRD
            dist = dist + l
        S, U = F32(0), F32(0)
        for k in range(n - 1, -1, -1):
            h = HALF * (dt[k] + dt[k + 1]) if k < n - 1 else F32(0)
            if k < n - 1:
                S = S + w[k + 1]
            U = U + S * h
            g[k] = dd * (TWO * (D[k] + U) + (TWO_THIRDS * w[k]) * dt[k])
    return dist, g, D


def dist32(se, w, dt):
    se = np.asarray(se).reshape(-1, 2)
    out = np.zeros(len(se), F32)
    for r, (s, e) in enumerate(se):
        if s < e:
            out[r] = _ray32(w[s:e], dt[s:e], F32(0))[0]
    return out


def grad32(se, w, dt, ddist, out):
    """writes g into `out` [M] for the samples of non-empty rays and returns (out, dist [R])"""
    se = np.asarray(se).reshape(-1, 2)
    ddist = np.asarray(ddist, F32)
    dist = np.zeros(len(se), F32)
    for r, (s, e) in enumerate(se):
        if s < e:
            dist[r], out[s:e], _ = _ray32(w[s:e], dt[s:e], ddist[r])
    return out, dist


def ray64(w, dt):
    """the pairwise definition: (dist, d dist / d w [n]) of one ray in fp64"""
    w = np.asarray(w, np.float64)
    dt = np.asarray(dt, np.float64)
    m = np.cumsum(dt) - 0.5 * dt
    a = np.abs(m[:, None] - m[None, :])
    dist = float(w @ a @ w + np.sum(w * w * dt) / 3.0)
    g = 2.0 * (a @ w) + (2.0 / 3.0) * w * dt
    return dist, g


def dist64(se, w, dt):
    se = np.asarray(se).reshape(-1, 2)
    return np.array([ray64(w[s:e], dt[s:e])[0] if s < e else 0.0 for s, e in se], np.float64)


def mean_tree(x, weight, losses, slot):
    """f2n_loss_add_mean on a copy of losses [8]"""
    x = np.asarray(x, F32)
    n = len(x)
    a = np.zeros(256, np.float64)
    for t in range(min(n, 256)):
        acc = 0.0
        for v in x[t::256]:
            acc += float(v)
        a[t] = acc
    off = 128
    while off >= 1:
        a[:off] = a[:off] + a[off:2 * off]
        off //= 2
    mean = F32(a[0] / float(n))
    out = np.array(losses, F32)
    out[slot] = mean
    out[0] = out[0] + F32(weight) * mean
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 0, 2, 15, 16, 17, 0, 31, 32, 33, 100, 1024, 0]


def make_rays(n_rays=37, seed=5, sample_l=1.0 / 256):
    """37 rays (not a multiple of the 16 rays of a block) whose lengths cycle through LENGTHS: empty rays first, last and in between.
    Weights are composited from log-normal densities (one ray ends in a fully opaque sample, one is near-empty),
    dt = sample_l * U[0.5, 1.5] * {1, 4, 16}.  Every weight is >= 2^-30 and every dt >= 2^-10, so no product of the recurrences falls
    below 2^-100: no subnormal is formed and flush modes cannot matter."""
    rng = np.random.default_rng(seed)
    lens = [LENGTHS[r % len(LENGTHS)] for r in range(n_rays)]
    lens[-1] = 0
    se = np.zeros((n_rays, 2), np.int32)
    ws, dts = [], []
    pos = 0
    for r, n in enumerate(lens):
        se[r] = (pos, pos + n)
        pos += n
        if n == 0:
            continue
        dt = (sample_l * rng.uniform(0.5, 1.5, n) * rng.choice([1.0, 4.0, 16.0], n)).astype(F32)
        sigma = np.exp(rng.normal(1.0, 2.0, n))
        if r % 5 == 1:
            sigma *= 1e-6  # near-empty
        if r % 7 == 3:
            sigma[n // 2] = 1e9  # fully opaque sample
        sec = sigma * dt
        trans = np.exp(-np.concatenate([[0.0], np.cumsum(sec)[:-1]]))
        w = np.maximum(trans * (1.0 - np.exp(-sec)), 2.0 ** -30).astype(F32)
        ws.append(w)
        dts.append(dt)
    w = np.concatenate(ws)
    dt = np.concatenate(dts)
    assert w.min() >= 2.0 ** -30 and dt.min() >= 2.0 ** -10
    return se, w, dt

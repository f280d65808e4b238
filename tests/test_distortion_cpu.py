"""The distortion loss on warped ray intervals without a GPU: known answers and the fp64 pairwise definition on the numpy restatement
(tests/distortion_ref.py), then distortion_fwd_kernel / distortion_bwd_kernel / loss_add_mean_kernel (csrc/render.hip) under the
wavefront emulator (tests/wave_emul) against that restatement, bit for bit (both builds use -ffp-contract=off).  The bodies that take an
`impl` run against the device as well (tests/test_gpu_distortion.py).

An `impl` is an object with
  fwd(se, w, dt) -> dist [R]
  bwd(se, w, dt, ddist, out, want_dist) -> (out [M] written in place of a copy of `out`, dist [R] or None)
  add_mean(x, weight, losses, slot) -> losses [8]
on numpy arrays; a bad argument raises."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emul"))

import distortion_ref as dr  # noqa: E402

F32 = np.float32
EPS = 2.0 ** -24
SENTINEL = F32(-12345.5)
INVALID = -1  # F2N_ERR_INVALID_ARG
_f, _i = ctypes.c_float, ctypes.c_int


@pytest.fixture(scope="module")
def emul():
    import wemu_build
    lib, _ = wemu_build.build()
    L = ctypes.CDLL(lib)
    L.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))
    return L


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size > 0 else None


class EmulError(RuntimeError):
    def __init__(self, name, rc):
        RuntimeError.__init__(self, "%s failed with status %d" % (name, rc))
        self.rc = rc


def _ck(rc, name):
    if rc != 0:
        raise EmulError(name, rc)


def _arrays(se, w, dt):
    return np.ascontiguousarray(se, np.int32).reshape(-1, 2), np.ascontiguousarray(w, F32), np.ascontiguousarray(dt, F32)


def emul_impl(L):
    def fwd(se, w, dt):
        se, w, dt = _arrays(se, w, dt)
        out = np.full(len(se), SENTINEL, F32)
        _ck(L.f2n_distortion_fwd(None, len(se), _vp(se), _vp(w), _vp(dt), _vp(out)), "f2n_distortion_fwd")
        return out

    def bwd(se, w, dt, ddist, out, want_dist):
        se, w, dt = _arrays(se, w, dt)
        out = np.array(out, F32)
        dist = np.full(len(se), SENTINEL, F32) if want_dist else None
        _ck(L.f2n_distortion_bwd(None, len(se), _vp(se), _vp(w), _vp(dt), _vp(np.ascontiguousarray(ddist, F32)), _vp(out), _vp(dist)),
            "f2n_distortion_bwd")
        return out, dist

    def add_mean(x, weight, losses, slot):
        x = np.ascontiguousarray(x, F32)
        out = np.array(losses, F32)
        _ck(L.f2n_loss_add_mean(None, len(x), _vp(x), _f(weight), _vp(out), _i(slot)), "f2n_loss_add_mean")
        return out

    return types.SimpleNamespace(fwd=fwd, bwd=bwd, add_mean=add_mean)


def tensor_impl(mod, dev):
    """an `impl` over the ctypes binding (distortion_fwd / distortion_bwd / loss_add_mean on torch tensors); dev(tensor) puts a tensor
    where that module wants it"""
    import torch

    def t(a, dtype):
        return dev(torch.from_numpy(np.ascontiguousarray(a, dtype)))

    def fwd(se, w, dt):
        se, w, dt = _arrays(se, w, dt)
        out = t(np.full(len(se), SENTINEL, F32), F32)
        mod.distortion_fwd(len(se), t(se, np.int32), t(w, F32), t(dt, F32), out)
        return out.cpu().numpy()

    def bwd(se, w, dt, ddist, out, want_dist):
        se, w, dt = _arrays(se, w, dt)
        o = t(out, F32)
        dist = t(np.full(len(se), SENTINEL, F32), F32) if want_dist else None
        mod.distortion_bwd(len(se), t(se, np.int32), t(w, F32), t(dt, F32), t(ddist, F32), o, dist)
        return o.cpu().numpy(), (dist.cpu().numpy() if want_dist else None)

    def add_mean(x, weight, losses, slot):
        o = t(losses, F32)
        mod.loss_add_mean(len(x), t(x, F32), float(weight), o, int(slot))
        return o.cpu().numpy()

    return types.SimpleNamespace(fwd=fwd, bwd=bwd, add_mean=add_mean)


def _ref_bwd(se, w, dt, ddist, out, want_dist):
    o, dist = dr.grad32(se, w, dt, ddist, np.array(out, F32))
    return o, (dist if want_dist else None)


REF = types.SimpleNamespace(fwd=dr.dist32, bwd=_ref_bwd, add_mean=dr.mean_tree)

_RAYS = {}


def rays():
    """the batch of tests/distortion_ref.make_rays and the restatement's answers for it, computed once and never written to"""
    if not _RAYS:
        se, w, dt = dr.make_rays()
        ddist = (np.random.default_rng(9).uniform(0.5, 2.0, len(se)) / len(se)).astype(F32)
        g, dist = dr.grad32(se, w, dt, ddist, np.full(len(w) + 8, SENTINEL, F32))
        for a in (se, w, dt, ddist, g, dist):
            a.setflags(write=False)
        _RAYS.update(se=se, w=w, dt=dt, ddist=ddist, g=g, dist=dist)
    return _RAYS


def _one(w, dt):
    return np.array([[0, len(w)]], np.int32), np.asarray(w, F32), np.asarray(dt, F32)


# ---- bodies --------------------------------------------------------------------------------------------------------------------------
def check_known_answers(impl):
    # one sample: w^2 dt / 3, the very roundings of l_k (the pair term is an exact zero)
    w, dt = F32(0.7), F32(0.013)
    assert impl.fwd(*_one([w], [dt]))[0] == ((w * w) * dt) * dr.THIRD
    # two samples: w0 w1 (dt0 + dt1) + (w0^2 dt0 + w1^2 dt1) / 3
    w, dt = np.array([0.3, 0.45], F32).astype(np.float64), np.array([0.02, 0.005], F32).astype(np.float64)
    want = w[0] * w[1] * (dt[0] + dt[1]) + (w[0] ** 2 * dt[0] + w[1] ** 2 * dt[1]) / 3.0
    got = float(impl.fwd(*_one(w, dt))[0])
    print("two samples: %.9g, fp64 %.9g" % (got, want))
    assert abs(got - want) <= (3 * 2 + 8) * EPS * want
    # all mass in one sample: the pair term is 0, what is left is that sample's own w^2 dt / 3, exactly
    n, k = 40, 17
    w, dt = np.zeros(n, F32), np.linspace(0.01, 0.05, n).astype(F32)
    w[k] = F32(0.9)
    assert impl.fwd(*_one(w, dt))[0] == ((w[k] * w[k]) * dt[k]) * dr.THIRD
    # an empty ray
    assert impl.fwd(np.array([[3, 3]], np.int32), np.ones(4, F32), np.ones(4, F32))[0] == 0.0


def check_bits(impl):
    r = rays()
    dist = impl.fwd(r["se"], r["w"], r["dt"])
    assert dr.same_bits(dist, r["dist"]), np.flatnonzero(dist != r["dist"])
    pre = np.full(len(r["w"]) + 8, SENTINEL, F32)  # (8 floats behind the last sample: nothing is written past e)
    for want_dist in (True, False):
        g, d = impl.bwd(r["se"], r["w"], r["dt"], r["ddist"], pre, want_dist)
        assert dr.same_bits(g, r["g"]), np.flatnonzero(g != r["g"])[:8]
        assert (g[len(r["w"]):] == SENTINEL).all()
        if want_dist:
            assert dr.same_bits(d, r["dist"])
    # rows of empty rays are untouched: the same rays with a gap of 3 samples in front of every ray that belongs to nobody
    se = np.array(r["se"])
    shift = 3 * (np.arange(len(se), dtype=np.int32) + 1)
    se2 = se + shift[:, None]
    m2 = int(se2.max()) + 3
    w2, dt2, want = np.ones(m2, F32), np.ones(m2, F32), np.full(m2, SENTINEL, F32)
    for (s, e), (s2, e2) in zip(se, se2):
        w2[s2:e2], dt2[s2:e2], want[s2:e2] = r["w"][s:e], r["dt"][s:e], r["g"][s:e]
    g, _ = impl.bwd(se2, w2, dt2, r["ddist"], np.full(m2, SENTINEL, F32), False)
    assert dr.same_bits(g, want)
    assert dr.same_bits(impl.fwd(se2, w2, dt2), r["dist"])


def check_nan_containment(impl):
    r = rays()
    lens = r["se"][:, 1] - r["se"][:, 0]
    victim = int(np.flatnonzero(lens == 33)[0])
    w = np.array(r["w"])
    w[r["se"][victim, 0] + 20] = np.nan
    dist = impl.fwd(r["se"], w, r["dt"])
    g, d = impl.bwd(r["se"], w, r["dt"], r["ddist"], np.full(len(w) + 8, SENTINEL, F32), True)
    s, e = r["se"][victim]
    assert np.isnan(dist[victim]) and np.isnan(d[victim]) and np.isnan(g[s:e]).all()
    keep = np.ones(len(g), bool)
    keep[s:e] = False
    others = np.arange(len(dist)) != victim
    assert dr.same_bits(g[keep], r["g"][keep]) and dr.same_bits(dist[others], r["dist"][others]) and dr.same_bits(d[others], r["dist"][others])


def check_add_mean(impl):
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 8192):
        x = (rng.uniform(0.0, 1.0, n) ** 4 * 1e-3).astype(F32)
        losses = np.array([0.25, 1, 2, 3, 4, 5, -1, 7], F32)
        out = impl.add_mean(x, 0.37, losses, 6)
        assert dr.same_bits(out, dr.mean_tree(x, 0.37, losses, 6))
        mean = np.sum(x.astype(np.float64)) / n
        # an fp64 sum in another order differs by ~n 2^-53 relative; then one fp32 rounding
        assert abs(float(out[6]) - mean) <= (EPS + n * 2.0 ** -52) * mean
        assert out[0] == F32(0.25) + F32(0.37) * out[6] and dr.same_bits(out[[1, 2, 3, 4, 5, 7]], losses[[1, 2, 3, 4, 5, 7]])


def check_contract(impl, errors):
    r = rays()
    se, w, dt, dd = r["se"], r["w"], r["dt"], r["ddist"]
    # no rays: nothing is touched
    none = np.zeros((0, 2), np.int32)
    assert len(impl.fwd(none, w, dt)) == 0
    g, _ = impl.bwd(none, w, dt, np.zeros(0, F32), np.full(4, SENTINEL, F32), False)
    assert (g == SENTINEL).all()
    x, losses = np.ones(4, F32), np.zeros(8, F32)
    for bad in (lambda: impl.add_mean(x[:0], 1.0, losses, 6), lambda: impl.add_mean(x, 1.0, losses, 0), lambda: impl.add_mean(x, 1.0, losses, 8),
                lambda: impl.add_mean(x, 1.0, losses, -1)):
        with pytest.raises(errors):
            bad()


# ---- the restatement alone -----------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_restatement():
    check_known_answers(REF)
    check_add_mean(REF)


def test_splitting_a_uniform_interval_leaves_dist_unchanged():
    """One interval whose weight is spread evenly over its length (the step function the loss integrates), cut in two halves that carry
    half the weight each: the same histogram, so the same loss -- the pair term of the halves makes up for their smaller self terms."""
    rng = np.random.default_rng(1)
    w, dt = rng.uniform(0.01, 0.2, 9), rng.uniform(0.01, 0.1, 9)
    base, _ = dr.ray64(w, dt)
    for k in (0, 4, 8):
        w2 = np.concatenate([w[:k], [w[k] / 2, w[k] / 2], w[k + 1:]])
        dt2 = np.concatenate([dt[:k], [dt[k] / 2, dt[k] / 2], dt[k + 1:]])
        assert abs(dr.ray64(w2, dt2)[0] - base) <= 1e-12 * base


def test_fp64_gradient_is_the_derivative():
    rng = np.random.default_rng(2)
    w, dt = rng.uniform(0.01, 0.2, 12), rng.uniform(0.01, 0.1, 12)
    _, g = dr.ray64(w, dt)
    for k in range(12):
        hp, hm = np.array(w), np.array(w)
        hp[k] += 1e-6
        hm[k] -= 1e-6
        fd = (dr.ray64(hp, dt)[0] - dr.ray64(hm, dt)[0]) / 2e-6
        assert abs(fd - g[k]) <= 1e-8 * abs(g[k])


def test_restatement_against_the_pairwise_definition():
    """per ray |dist - dist64| <= (3n+8) 2^-24 dist64, per sample |g - g64| <= (2n+8) 2^-24 g64: the first-order bounds of recursive
    summation of non-negative terms"""
    r = rays()
    worst_d = worst_g = 0.0
    for ray, (s, e) in enumerate(r["se"]):
        n = e - s
        if n == 0:
            assert r["dist"][ray] == 0.0
            continue
        d64, g64 = dr.ray64(r["w"][s:e], r["dt"][s:e])
        g64 = g64 * float(r["ddist"][ray])
        ed = abs(float(r["dist"][ray]) - d64) / d64
        eg = np.max(np.abs(r["g"][s:e].astype(np.float64) - g64) / g64)
        worst_d, worst_g = max(worst_d, ed / ((3 * n + 8) * EPS)), max(worst_g, eg / ((2 * n + 8) * EPS))
        assert ed <= (3 * n + 8) * EPS and eg <= (2 * n + 8) * EPS, (ray, n, ed, eg)
    print("largest error as a fraction of its bound: dist %.3f, gradient %.3f" % (worst_d, worst_g))


def test_no_subnormal_is_formed():
    r = rays()
    assert r["w"].min() >= 2.0 ** -30 and r["dt"].min() >= 2.0 ** -10 and r["ddist"].min() >= 2.0 ** -10
    assert r["g"][:len(r["w"])].min() >= 2.0 ** -100 and r["dist"][r["se"][:, 1] > r["se"][:, 0]].min() >= 2.0 ** -100


def test_shapes_of_the_batch():
    r = rays()
    lens = (r["se"][:, 1] - r["se"][:, 0]).tolist()
    assert len(lens) == 37 and set(lens) == {0, 1, 2, 15, 16, 17, 31, 32, 33, 100, 1024} and lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1]


# ---- the kernels under the emulator --------------------------------------------------------------------------------------------------
def test_kernels_match_the_restatement(emul):
    impl = emul_impl(emul)
    check_known_answers(impl)
    check_bits(impl)


def test_nan_stays_in_its_ray(emul):
    check_nan_containment(REF)
    check_nan_containment(emul_impl(emul))


def test_loss_add_mean(emul):
    check_add_mean(emul_impl(emul))


@pytest.mark.parametrize("schedule", [1, 2])
def test_schedule_independence(emul, schedule):
    emul.wemu_set_schedule(schedule)
    try:
        check_bits(emul_impl(emul))
        check_add_mean(emul_impl(emul))
    finally:
        emul.wemu_set_schedule(int(os.environ.get("WEMU_SCHEDULE", "0")))


def test_error_codes_of_the_entry_points(emul):
    check_contract(emul_impl(emul), EmulError)
    L = emul
    r = rays()
    se, w, dt, dd = (np.array(r[k]) for k in ("se", "w", "dt", "ddist"))
    out, dist = np.zeros(len(w), F32), np.zeros(len(se), F32)
    R = len(se)
    assert L.f2n_distortion_fwd(None, -1, _vp(se), _vp(w), _vp(dt), _vp(dist)) == INVALID
    assert L.f2n_distortion_bwd(None, -1, _vp(se), _vp(w), _vp(dt), _vp(dd), _vp(out), None) == INVALID
    for k in range(4):
        a = [_vp(se), _vp(w), _vp(dt), _vp(dist)]
        a[k] = None
        assert L.f2n_distortion_fwd(None, R, *a) == INVALID
    for k in range(5):
        a = [_vp(se), _vp(w), _vp(dt), _vp(dd), _vp(out)]
        a[k] = None
        assert L.f2n_distortion_bwd(None, R, *a, None) == INVALID
    assert L.f2n_distortion_bwd(None, R, _vp(se), _vp(w), _vp(dt), _vp(dd), _vp(w), None) == INVALID  # (dweights is the scratch for D)
    assert L.f2n_distortion_bwd(None, R, _vp(se), _vp(w), _vp(dt), _vp(dd), _vp(dt), None) == INVALID
    assert L.f2n_distortion_fwd(None, 0, None, None, None, None) == 0
    x, losses = np.ones(4, F32), np.zeros(8, F32)
    assert L.f2n_loss_add_mean(None, 4, None, _f(1.0), _vp(losses), 6) == INVALID
    assert L.f2n_loss_add_mean(None, 4, _vp(x), _f(1.0), None, 6) == INVALID
    assert (losses == 0).all()
    assert L.f2n_abi_version() == 13


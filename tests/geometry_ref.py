"""numpy restatement of the render geometry buffers (f2n_composite_geometry, csrc/render.hip) -- test infrastructure.

Two halves, as the kernel has two:
  * per sample, g = J^T df0/dw and n = -g / |g|: float64 (and float32 in the kernel's order) through density_grad_ref.grad_sigma with
    sigma = 1 and the oracle's Jacobian (oc.warp);
  * per ray, float32 sums that add left to right, one term after the other (np.cumsum of float32 is that loop), fed the kernel's own
    sample normals and weights: the product and the emulator are built with -ffp-contract=off, so these are held bit for bit."""
import numpy as np

import density_grad_ref as dr
from oracle import capi as oc

F32, F64 = np.float32, np.float64


def world_points(rays_o, rays_d, t, se):
    """x_i = o_r + d_r * t_i with the march's two float32 roundings (csrc/sampler.hip: xyz = o + d * cur_t)."""
    ray = np.repeat(np.arange(len(se)), se[:, 1] - se[:, 0])
    assert len(ray) == len(t)
    o, d = np.asarray(rays_o, F32)[ray], np.asarray(rays_d, F32)[ray]
    return (o + (d * np.asarray(t, F32)[:, None]).astype(F32)).astype(F32)


def unit(v, sign=1.0):
    """sign * v / |v| in float32 by the rule of f2n_grid_normals: sqrt((v0 v0 + v1 v1) + v2 v2), zero where that is 0 or not finite."""
    v = np.asarray(v, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ln = np.sqrt(((v[:, 0] * v[:, 0]).astype(F32) + (v[:, 1] * v[:, 1]).astype(F32)).astype(F32) + (v[:, 2] * v[:, 2]).astype(F32)).astype(F32)
        ok = (ln > 0) & (ln < np.inf)
        out = np.where(ok[:, None], F32(sign) * (v / np.where(ok, ln, F32(1))[:, None]).astype(F32), F32(0))
    return out.astype(F32)


def _running(x):
    """((0 + x_0) + x_1) + ... in float32, every prefix."""
    return np.cumsum(np.concatenate([np.zeros(1, F32), np.asarray(x, F32)]), dtype=F32)[1:]


def ray_buffers(se, weights, t, rays_o, rays_d, sample_normals, tau):
    """The per-ray outputs of f2n_composite_geometry from the weights and the per-sample normals, float32 left to right."""
    R = len(se)
    w, nrm = np.asarray(weights, F32), np.asarray(sample_normals, F32)
    x = world_points(rays_o, rays_d, t, se) if len(t) else np.zeros((0, 3), F32)
    out = dict(opacity=np.zeros(R, F32), N=np.zeros((R, 3), F32), surf_idx=np.full(R, -1, np.int32), surf_t=np.zeros(R, F32),
               surf_points=np.zeros((R, 3), F32), surf_normals=np.zeros((R, 3), F32))
    tau = F32(tau)
    for r in range(R):
        s, e = int(se[r, 0]), int(se[r, 1])
        if s >= e:
            continue
        incl = _running(w[s:e])
        out["opacity"][r] = incl[-1]
        for k in range(3):
            out["N"][r, k] = _running((w[s:e] * nrm[s:e, k]).astype(F32))[-1]
        hit = np.nonzero(incl >= tau)[0]
        if len(hit):
            i = s + int(hit[0])
            out["surf_idx"][r] = i
            out["surf_t"][r] = t[i]
            out["surf_points"][r] = x[i]
            out["surf_normals"][r] = nrm[i]
    out["normals"] = unit(out["N"])
    return out


def sample_grad(pers_trans, anchors, x_world, df0_dw, dtype=F64, S_g=None):
    """J^T df0/dw at the world points (float64, or float32 in the kernel's order) and its S (density_grad_ref.grad_sigma, sigma = 1)."""
    _, jac = oc.warp(pers_trans, np.ascontiguousarray(anchors[:, 0]), np.ascontiguousarray(x_world, F32))
    return dr.grad_sigma(np.ones(len(x_world), F32), jac, df0_dw, dtype, S_g)


def restated_sample_grad(pers_trans, grid, params, pts_warped, anchors, x_world, d_hidden=64, dx_of=None):
    """(ref64, ref32, S, keep) of the samples' world-space gradient of f0: the field chain of the restatement on the warped points the
    renderer returned, the oracle's Jacobian at o + t d.  dx_of(chain): df0/dx of the float32 evaluation (the oracle's mlp_bwd for field
    shapes without the fused kernels)."""
    tr = np.ascontiguousarray(anchors[:, 0])
    c = dr.field_chain(grid, params, np.ascontiguousarray(pts_warped, F32), tr, d_hidden=d_hidden)
    g32 = c["g32"] if dx_of is None else dr.df0_dw(c["cells"], dx_of(c), F32)[0]
    ref64, S = sample_grad(pers_trans, anchors, x_world, c["g"], F64, c["S_g"])
    ref32, _ = sample_grad(pers_trans, anchors, x_world, g32, F32)
    return ref64, ref32, S, ~c["ties"]


TAU = 0.5
LENGTHS = (0, 1, 15, 16, 17, 33, 100)  # every boundary of the kernel's 16-sample chunks


def synthetic_case(pers_trans, n_rays=37, seed=0, max_len=100, tau=TAU, special=True):
    """Rays with synthetic weights / t / df0_dw on a scene's transforms.  Ray r looks through the centre of transform T_r; its samples
    sit within 0.1 of it.  special: rays 0..6 have the LENGTHS; 7 never reaches tau; 8 reaches it at its first sample; 9 has an
    inclusive sum equal to tau exactly at its third sample; 10 holds a sample with df0_dw = 0 and one with an infinite component; 11
    spreads its 100 samples over four transforms.  The other lengths are drawn from 0..max_len."""
    rng = np.random.default_rng(seed)
    tr = np.ascontiguousarray(pers_trans).view(np.uint8).reshape(-1, 544)
    centers = np.ascontiguousarray(tr[:, 528:540]).view(F32).reshape(-1, 3)
    n_tr = len(tr)
    lens = rng.integers(0, max_len + 1, n_rays)
    if special:
        assert n_rays >= 12
        lens[:7] = LENGTHS
        lens[7:12] = (20, 18, 40, 35, 100)
    se = np.zeros((n_rays, 2), np.int32)
    se[:, 1] = np.cumsum(lens)
    se[:, 0] = se[:, 1] - lens
    M = int(se[-1, 1])
    T = rng.integers(0, n_tr, n_rays)
    d = rng.standard_normal((n_rays, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    o = (centers[T] - d + rng.uniform(-0.01, 0.01, (n_rays, 3))).astype(F32)
    ray = np.repeat(np.arange(n_rays), lens)
    t = np.empty(M, F32)
    w = np.empty(M, F32)
    for r in range(n_rays):
        s, e = se[r]
        t[s:e] = np.sort(rng.uniform(0.9, 1.1, e - s)).astype(F32)
        w[s:e] = (rng.random(e - s) * rng.uniform(0.2, 2.5) / max(e - s, 1)).astype(F32)  # sums from ~0.1 to ~1.2
    anchors = np.stack([T[ray], rng.integers(0, 1000, M), np.zeros(M, np.int64)], 1).astype(np.int32)
    g = (rng.standard_normal((M, 3)) * 50).astype(F32)
    if special:
        s = se[7, 0]
        w[s:se[7, 1]] = F32(0.01)                       # 0.2 in all: below tau
        w[se[8, 0]] = F32(0.9)                          # reaches tau at once
        s = se[9, 0]
        w[s:s + 3] = (0.125, 0.125, 0.25)               # exactly 0.5 at the third sample (dyadic: no rounding)
        s = se[10, 0]
        g[s + 3] = 0
        g[s + 17, 1] = np.inf
        w[s:se[10, 1]] = F32(0.05)                      # both samples carry weight
        s = se[11, 0]
        anchors[s:s + 100, 0] = (T[11] + np.arange(100) // 25) % n_tr
    return dict(se=se, weights=w, t=t, rays_o=o, rays_d=d, anchors=anchors, df0_dw=g, tau=tau, transes=tr)


def same_bits(a, b):
    """Equal bit patterns; a NaN matches any NaN (its sign and payload are not part of any contract)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    bits = "u%d" % a.dtype.itemsize
    return bool(((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))).all())

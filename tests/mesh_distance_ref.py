"""Numpy restatement of the mesh-to-mesh distance primitives (include/f2n_abi.h, "Closest point on a triangle mesh" and "Area-uniform
surface samples"): the fp64 region walk over all (point, face) pairs with every rounding as stated, the brute-force choice among them,
the shell walk over the ray caster's face grid with its LB rule, and the weights / targets / barycentrics of the surface samples on
tests/philox_ref.py.  Nothing here imports the package."""
import numpy as np

import mesh_raycast_ref as rr
from philox_ref import philox4x32_10

F32, F64 = np.float32, np.float64
SAMPLE_PURPOSE = 0x8CB92BA72F3D8DD7  # host/Renderer.h: kMeshSamplePurpose


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_table(verts, faces, points):
    """steps 1-3 for every (point, face) pair: (d2 [N,F] f64, bary [N,F,3] f64).  A face index outside [0, V) raises ValueError."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(points, F32).reshape(-1, 3).astype(F64)[:, None, :]
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("face index out of range")
    P = v[f].astype(F64) if len(f) else np.zeros((0, 3, 3))
    A, B, C = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    with np.errstate(all="ignore"):
        ab, ac = B - A, C - A
        ap, bp, cp = p - A, p - B, p - C
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        g, k = d4 - d3, d5 - d6
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = g / (g + k)
        s = (va + vb) + vc
        v_in, w_in = vb / s, vc / s
        cases = [((d1 <= 0) & (d2 <= 0), (one, zero, zero)),
                 ((d3 >= 0) & (d4 <= d3), (zero, one, zero)),
                 ((d6 >= 0) & (d5 <= d6), (zero, zero, one)),
                 ((vc <= 0) & (d1 >= 0) & (d3 <= 0), (1.0 - v_ab, v_ab, zero)),
                 ((vb <= 0) & (d2 >= 0) & (d6 <= 0), (1.0 - w_ac, zero, w_ac)),
                 ((va <= 0) & (g >= 0) & (k >= 0), (zero, 1.0 - w_bc, w_bc))]
        u, vv, w = (1.0 - v_in) - w_in, v_in, w_in  # the interior, and every NaN
        for cond, (cu, cv, cw) in reversed(cases):  # (the first test that holds wins: applied last)
            u, vv, w = np.where(cond, cu, u), np.where(cond, cv, vv), np.where(cond, cw, w)
        q = (u[..., None] * A + vv[..., None] * B) + w[..., None] * C
        e = p - q
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return dd, np.stack([u, vv, w], -1)


def _finish(dd, bary, best_face, points, max_dist):
    """step 4's conversion and step 5 from the winning face per point (-1: none)"""
    n = len(best_face)
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    rows = np.arange(n)
    fi = np.maximum(best_face, 0)
    have = (best_face >= 0) & np.isfinite(p).all(1)
    with np.errstate(all="ignore"):
        dist = np.sqrt(dd[rows, fi] if dd.shape[1] else np.zeros(n)).astype(F32)
    b = bary[rows, fi].astype(F32) if dd.shape[1] else np.zeros((n, 3), F32)
    hit = have & ~(dist > F32(max_dist))
    return (np.where(hit, dist, F32(np.inf)).astype(F32), np.where(hit, best_face, -1).astype(np.int32),
            np.where(hit[:, None], b, F32(0)).astype(F32))


def _winner(dd_row, tested):
    """the tested face of the smallest d2, the lowest index among equals; NaN and +inf never win: -1 for none"""
    d = np.where(tested & np.isfinite(dd_row), dd_row, np.inf)
    if not len(d) or not np.isfinite(d.min()):
        return -1
    return int(np.argmin(d))  # (argmin returns the first of equal minima)


def closest_point(verts, faces, points, max_dist=np.inf, table=None):
    """(dist [N] f32, face [N] i32, bary [N,3] f32): the contract's brute force"""
    dd, bary = table if table is not None else pair_table(verts, faces, points)
    all_f = np.ones(dd.shape[1], bool)
    best = np.array([_winner(dd[i], all_f) for i in range(dd.shape[0])], np.int64).reshape(-1)
    return _finish(dd, bary, best, points, max_dist)


def closest_point_grid(verts, faces, accel, points, max_dist=np.inf, table=None, shells=None):
    """The shell walk over accel = (lo, cell, dims, cell_start, cell_faces) with the LB rule, every fp32 rounding as stated; it picks
    among the SAME pair table as the brute force, so the two differ only if the walk stops too early.  shells (a list) receives the
    number of shells every point walked."""
    lo, cell, dims, cs, cf = accel
    lo, cell = np.asarray(lo, F32), F32(cell)
    nx, ny, nz = (int(d) for d in dims)
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    dd, bary = table if table is not None else pair_table(verts, faces, points)
    nf = dd.shape[1]
    best = np.full(len(p), -1, np.int64)
    md = F32(max_dist)
    for i in range(len(p)):
        if not np.isfinite(p[i]).all():
            continue
        c = [int(rr.cell_of(p[i, k], lo[k], cell, dims[k])) for k in range(3)]
        tested = np.zeros(nf, bool)
        r = 0
        while True:
            z, y, x = np.meshgrid(np.arange(max(c[2] - r, 0), min(c[2] + r, nz - 1) + 1), np.arange(max(c[1] - r, 0), min(c[1] + r, ny - 1) + 1),
                                  np.arange(max(c[0] - r, 0), min(c[0] + r, nx - 1) + 1), indexing="ij")
            on = np.maximum(np.maximum(np.abs(z - c[2]), np.abs(y - c[1])), np.abs(x - c[0])) == r
            for cc in ((z * ny + y) * nx + x)[on].reshape(-1):
                tested[cf[cs[cc]:cs[cc + 1]]] = True
            best[i] = _winner(dd[i], tested)
            terms = []
            for k, n_k in enumerate((nx, ny, nz)):
                if c[k] - r > 0:
                    terms.append(F32(p[i, k] - F32(lo[k] + F32(F32(c[k] - r) * cell))))
                if c[k] + r < n_k - 1:
                    terms.append(F32(F32(lo[k] + F32(F32(c[k] + r + 1) * cell)) - p[i, k]))
            r += 1
            if not terms:
                break
            lb = min(terms)
            if (best[i] >= 0 and F32(np.sqrt(dd[i, best[i]])) < lb) or lb > md:
                break
        if shells is not None:
            shells.append(r)
    return _finish(dd, bary, best, points, max_dist)


def in_domain(lo, cell, dims, points):
    """the walk's domain for the points: the finite ones (the others miss by contract) within 2^15 cells of the frame's origin"""
    p = np.asarray(points, F64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    return rr.in_domain(lo, cell, dims, p)


# ---- surface samples -------------------------------------------------------------------------------------------------------------
def face_area2(verts, faces):
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    P = v[np.where(ok[:, None], f, 0)].astype(F64) if len(v) else np.zeros((len(f), 3, 3))
    ok &= np.isfinite(P).all((1, 2))
    with np.errstate(all="ignore"):
        p, q = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        n = np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)
        a = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return np.where(ok, a, 0.0)


def face_weights(verts, faces):
    """(weights [F] int64, cum [F] int64, T): ValueError for a mesh without area"""
    a = face_area2(verts, faces)
    if not len(a) or not a.max() > 0:
        raise ValueError("the mesh has no face with an area")
    quantum = a.max() * 2.0 ** -31
    w = np.floor(a / quantum).astype(np.int64)
    cum = np.cumsum(w, dtype=np.int64)
    return w, cum, int(cum[-1])


def sample_key(seed):
    return (int(seed) ^ SAMPLE_PURPOSE) & 0xFFFFFFFFFFFFFFFF


def sample_surface(verts, faces, n, seed=0, exact=False):
    """(points [n,3] f32, face [n] i32, bary [n,3] f32); exact: the points instead in float64 from the float64 weights (1 - s, s (1 - r),
    s r) before their rounding to float32 -- points of the faces themselves, to one float64 rounding"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    _, cum, T = face_weights(v, f)
    key = sample_key(seed)
    j = np.arange(n, dtype=np.int64)
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = j.astype(np.uint32)
    x = philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32)).astype(F64)
    two32 = 2.0 ** -32
    at = (j.astype(F64) + (x[:, 0] + 0.5) * two32) / F64(n) * F64(T)
    target = np.minimum(np.floor(at).astype(np.int64), T - 1)
    face = np.searchsorted(cum, target, side="right")
    s, r = np.sqrt((x[:, 1] + 0.5) * two32), (x[:, 2] + 0.5) * two32
    b64 = np.stack([1.0 - s, s * (1.0 - r), s * r], 1)
    b = b64.astype(F32)
    P = v[f[face]]
    if exact:
        return (b64[:, :, None] * P.astype(F64)).sum(1), face.astype(np.int32), b
    pts = ((b[:, 0:1] * P[:, 0] + b[:, 1:2] * P[:, 1]).astype(F32) + b[:, 2:3] * P[:, 2]).astype(F32)
    return pts, face.astype(np.int32), b

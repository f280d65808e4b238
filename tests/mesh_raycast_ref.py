"""Numpy restatement of the mesh ray caster (include/f2n_abi.h, "Ray casting against a triangle mesh"): the brute force over all
ray-face pairs with every rounding as stated (float32 for steps 2-3, float64 for steps 4-7), chunked over rays; the binning of faces
into the acceleration grid's cells; compare_depth.  Nothing here imports the package."""
import numpy as np

F32, F64 = np.float32, np.float64
GUARD = F32(0.0625)         # guard = cell * 2^-4
DOMAIN_CELLS = 32768.0      # the traversal's domain: coordinates up to 2^15 cells
MAX_CELLS = 1 << 27


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _frames(o, d):
    """steps 1-2 for rays [R,3]: (ok, kx, ky, kz, Sx, Sy, Sz)"""
    ad = np.abs(d)
    R = len(d)
    kz = np.zeros(R, np.int64)
    m = ad[:, 0].copy()
    with np.errstate(invalid="ignore"):
        up = ad[:, 1] > m
        kz[up], m[up] = 1, ad[up, 1]
        kz[ad[:, 2] > m] = 2
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    rows = np.arange(R)
    dz = d[rows, kz]
    with np.errstate(invalid="ignore"):
        neg = dz < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    ok = np.isfinite(d).all(1) & (dz != 0)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = d[rows, kx] / dz, d[rows, ky] / dz, F32(1.0) / dz
    return ok, kx, ky, kz, Sx.astype(F32), Sy.astype(F32), Sz.astype(F32)


def raycast(verts, faces, rays_o, rays_d, bounds=None, chunk=None):
    """(t [R] f32, face [R] i32, bary [R,3] f32): the contract's brute force.  A face with an index outside [0, V) raises ValueError."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    o = np.ascontiguousarray(rays_o, F32).reshape(-1, 3)
    d = np.ascontiguousarray(rays_d, F32).reshape(-1, 3)
    R, nf = len(o), len(f)
    if nf and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("face index out of range")
    t_min = np.zeros(R, F32) if bounds is None else np.asarray(bounds, F32).reshape(-1, 2)[:, 0]
    t_max = np.full(R, np.inf, F32) if bounds is None else np.asarray(bounds, F32).reshape(-1, 2)[:, 1]
    out_t, out_f, out_b = np.zeros(R, F32), np.full(R, -1, np.int32), np.zeros((R, 3), F32)
    if R == 0 or nf == 0:
        return out_t, out_f, out_b
    ok, kx, ky, kz, Sx, Sy, Sz = _frames(o, d)
    P = v[f]  # [F,3 corners,3]
    chunk = chunk or max(1, (1 << 21) // nf)
    for s in range(0, R, chunk):
        e = min(R, s + chunk)
        n = e - s
        with np.errstate(all="ignore"):
            q = P[None] - o[s:e, None, None, :]  # [n,F,3,3] float32
            qx, qy, qz = (np.take_along_axis(q, np.broadcast_to(k[s:e, None, None, None], (n, nf, 3, 1)), 3)[..., 0] for k in (kx, ky, kz))
            x = qx - Sx[s:e, None, None] * qz
            y = qy - Sy[s:e, None, None] * qz
            z = Sz[s:e, None, None] * qz
            assert x.dtype == F32 and z.dtype == F32
            x, y, z = x.astype(F64), y.astype(F64), z.astype(F64)
            A, B, C = 0, 1, 2
            U = x[..., C] * y[..., B] - y[..., C] * x[..., B]
            V = x[..., A] * y[..., C] - y[..., A] * x[..., C]
            W = x[..., B] * y[..., A] - y[..., B] * x[..., A]
            inside = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
            det = (U + V) + W
            inside &= det != 0
            T = (U * z[..., A] + V * z[..., B]) + W * z[..., C]
            t = (T / det).astype(F32)
            acc = inside & (t > t_min[s:e, None]) & (t < t_max[s:e, None]) & ok[s:e, None]
            tt = np.where(acc, t, np.inf).astype(F32)
            best = tt.min(1)
            hit = acc.any(1)
            first = np.argmax(acc & (tt == best[:, None]), 1)  # the lowest index among equal t
            r = np.arange(n)
            bary = np.stack([(U[r, first] / det[r, first]).astype(F32), (V[r, first] / det[r, first]).astype(F32),
                             (W[r, first] / det[r, first]).astype(F32)], 1)
        # (an accepted t is finite -- t < t_max -- so best is the accepted minimum wherever hit)
        out_t[s:e] = np.where(hit, t[r, first], F32(0))
        out_f[s:e] = np.where(hit, first, -1)
        out_b[s:e] = np.where(hit[:, None], bary, F32(0))
    return out_t, out_f, out_b


# ---- the acceleration grid ---------------------------------------------------------------------------------------------------------
def default_cell(verts, faces):
    """The documented default: the cell at which a surface of the bounding box's area would hold about ten faces per cell, at least
    1/500 of the box's longest side (float32 of a float64 formula)."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    nf = len(np.asarray(faces).reshape(-1, 3))
    if len(v) == 0:
        return 1.0
    e = (v.max(0).astype(F64) - v.min(0).astype(F64))
    area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    cell = max(np.sqrt(10.0 * area / max(nf, 1)), e.max() / 500.0)
    return float(F32(cell)) if cell > 0 and np.isfinite(cell) else 1.0


def grid_for(verts, cell, lo=None):
    """(lo [3] f32, dims [3]) as the host derives them: lo = the minimum of the finite coordinates unless given, dims from the maximum"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    cell = F32(cell)
    lo3 = np.zeros(3, F32) if lo is None else np.asarray(lo, F32).copy()
    dims = [1, 1, 1]
    for k in range(3):
        col = v[:, k][np.isfinite(v[:, k])]
        if len(col):
            if lo is None:
                lo3[k] = col.min()
            u = F32(F32(col.max() - lo3[k]) / cell)
            dims[k] = int(np.floor(u)) + 1 if u >= 0 else 1
    return lo3, dims


def cell_of(p, lo_k, cell, n_k):
    with np.errstate(all="ignore"):
        u = np.floor((np.asarray(p, F32) - F32(lo_k)).astype(F32) / F32(cell))
    u = np.where(np.isnan(u), F32(0), u)  # (fmaxf(NaN, 0) is 0 on the device)
    return np.minimum(np.maximum(u, F32(0)), F32(n_k - 1)).astype(np.int64)


def bin_faces(verts, faces, lo, cell, dims):
    """(cell_start [ncells+1] int32, cell_faces [E] int32): which faces every cell lists, in ascending (cell, face) order"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nf, ncells = len(f), int(dims[0]) * int(dims[1]) * int(dims[2])
    guard = F32(F32(cell) * GUARD)
    keys = []
    if nf:
        P = v[f]
        fin = np.isfinite(P).all((1, 2))
        with np.errstate(all="ignore"):
            mn, mx = (P.min(1) - guard).astype(F32), (P.max(1) + guard).astype(F32)
        i0 = np.stack([cell_of(mn[:, k], lo[k], cell, dims[k]) for k in range(3)], 1)
        i1 = np.stack([cell_of(mx[:, k], lo[k], cell, dims[k]) for k in range(3)], 1)
        for i in np.nonzero(fin)[0]:
            z, y, x = np.meshgrid(*(np.arange(i0[i, k], i1[i, k] + 1) for k in (2, 1, 0)), indexing="ij")
            keys.append((((z * dims[1] + y) * dims[0] + x) * nf + i).reshape(-1))
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    cell_start = np.searchsorted(keys, np.arange(ncells + 1, dtype=np.int64) * max(nf, 1)).astype(np.int32)
    return cell_start, (keys % max(nf, 1)).astype(np.int32)


def in_domain(lo, cell, dims, rays_o):
    lo = np.asarray(lo, F64)
    hi = lo + np.asarray(dims, F64) * float(cell)
    o = np.asarray(rays_o, F64).reshape(-1, 3)
    m = max(np.abs(lo).max(), np.abs(hi).max(), np.abs(o).max() if len(o) else 0.0)
    return bool(m <= DOMAIN_CELLS * float(cell))


# ---- render_mesh / compare_depth -----------------------------------------------------------------------------------------------------
def render(verts, faces, rays_o, rays_d, t, face, bary, normals=None, colors=None):
    """points, face_normals, facing and the attribute blends of mesh.render_mesh recomputed in float64 from (t, face, bary)"""
    v, f = np.asarray(verts, F64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    o, d = np.asarray(rays_o, F64).reshape(-1, 3), np.asarray(rays_d, F64).reshape(-1, 3)
    hit = np.asarray(face) >= 0
    fi = np.maximum(np.asarray(face), 0)
    P = v[f[fi]] if len(f) else np.zeros((len(o), 3, 3))
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(hit[:, None] & (ln > 0), n / np.where(ln > 0, ln, 1.0), 0.0)
    out = {"hit": hit, "points": np.where(hit[:, None], o + np.asarray(t, F64)[:, None] * d, 0.0), "face_normals": n,
           "facing": hit & (-(n * d).sum(1) > 0)}
    b = np.asarray(bary, F64)
    for name, attr in (("normals", normals), ("colors", colors)):
        if attr is not None:
            a = np.asarray(attr, F64).reshape(-1, 3)[f[fi]] if len(f) else np.zeros((len(o), 3, 3))
            x = (a * b[:, :, None]).sum(1)
            if name == "normals":
                lx = np.linalg.norm(x, axis=1, keepdims=True)
                x = np.where(lx > 0, x / np.where(lx > 0, lx, 1.0), 0.0)
            out[name] = np.where(hit[:, None], x, 0.0)
    return out


def quantile(sorted_e, q):
    """the element at index min(n - 1, floor(q n)) of the ascending errors (0 for none)"""
    n = len(sorted_e)
    return float(sorted_e[min(n - 1, int(np.floor(q * n)))]) if n else 0.0


def compare_depth(t_field, has_field, t_mesh, has_mesh, step):
    tf, tm = np.asarray(t_field, F32).reshape(-1), np.asarray(t_mesh, F32).reshape(-1)
    hf, hm = np.asarray(has_field, bool).reshape(-1), np.asarray(has_mesh, bool).reshape(-1)
    both = hf & hm
    e = np.sort((np.abs(tm[both] - tf[both]) / F32(step)).astype(F32))
    n, nb = len(tf), int(both.sum())
    share = lambda a, b: float(a) / float(b) if b else 0.0  # noqa: E731
    return {"n_rays": n, "n_field": int(hf.sum()), "n_mesh": int(hm.sum()), "n_both": nb, "completeness": share(nb, hf.sum()),
            "extra": share((hm & ~hf).sum(), n), "mean": float(e.astype(F64).mean()) if nb else 0.0, "median": quantile(e, 0.5),
            "p90": quantile(e, 0.9), "max": float(e[-1]) if nb else 0.0, "within_1": share((e <= 1).sum(), nb),
            "within_2": share((e <= 2).sum(), nb)}

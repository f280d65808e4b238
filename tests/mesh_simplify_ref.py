"""numpy restatement of the mesh simplification of include/f2n_abi.h ("Mesh simplification by vertex clustering"): cluster keys, the
exact int64 sums of the quantised plane quadrics, the float64 placement in the header's operation order, the re-indexed faces -- the
tests' reference, written from the definitions in the header, not from the kernels.  float32 arrays keep every operation at one float32
rounding, float64 arrays at one float64 rounding; numpy contracts nothing into an FMA."""
import numpy as np

F32 = np.float32
SLOTS = 16
MAX_RECORDS = 1 << 18
SCALE = 2.0 ** 40
UNSUPPORTED = -2  # F2N_ERR_UNSUPPORTED


class Unsupported(ValueError):
    """the guard of f2n_mesh_cluster_accumulate: more than 2^18 corner records or vertices in one cluster"""


def grid_for(verts, cell, lo=None):
    """(lo [3] f32, dims [3]) as the host derives them: lo = the minimum of the finite coordinates unless given,
    dims_k = floor((max_k - lo_k) / cell) + 1 in float32."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    cell = F32(cell)
    lo3 = np.zeros(3, F32) if lo is None else np.asarray(lo, F32).copy()
    dims = [1, 1, 1]
    for k in range(3):
        col = v[np.isfinite(v[:, k]), k]  # (per coordinate, over its finite values)
        if len(col) > 0 and cell > 0 and np.isfinite(cell):
            if lo is None:
                lo3[k] = col.min()
            with np.errstate(all="ignore"):
                u = F32(F32(col.max() - lo3[k]) / cell)
            assert not u >= 1048575.0
            dims[k] = int(np.floor(u)) + 1 if u >= 0 else 1
    return lo3, dims


def cell_index(p, lo_k, cell, dim):
    with np.errstate(all="ignore"):
        u = np.floor((np.asarray(p, F32) - F32(lo_k)) / F32(cell))
        u = np.minimum(np.maximum(u, F32(0)), F32(dim - 1))  # (clamped as floats, then cast)
        return np.where(np.isfinite(u), u, 0).astype(np.int64)


def centre(i, lo_k, cell):
    return F32(lo_k) + (np.asarray(i).astype(F32) + F32(0.5)) * F32(cell)


def local(p, lo, cell, dims):
    """q [n,3] f32: the local coordinates of the points p [n,3] in their own cells."""
    p = np.asarray(p, F32).reshape(-1, 3)
    q = np.empty_like(p)
    with np.errstate(all="ignore"):
        for k in range(3):
            c = centre(cell_index(p[:, k], lo[k], cell, dims[k]), lo[k], cell)
            q[:, k] = np.minimum(np.maximum((p[:, k] - c) / F32(cell), F32(-0.5)), F32(0.5))
    return q


def quant(x):
    with np.errstate(all="ignore"):
        return np.rint(np.asarray(x, F32).astype(np.float64) * SCALE).astype(np.int64)  # (rint: to nearest even)


def keys(verts, lo, cell, dims):
    v = np.asarray(verts, F32).reshape(-1, 3)
    i = [cell_index(v[:, k], lo[k], cell, dims[k]) for k in range(3)]
    key = (i[2] * dims[1] + i[1]) * dims[0] + i[0]
    return np.where(np.isfinite(v).all(1), key, -1).astype(np.int64)


def clusters(key):
    """(cluster_keys [C] int64 ascending, cluster_of [V] int32, -1 for key -1)"""
    uk, inv = np.unique(key, return_inverse=True)
    bad = 1 if len(uk) > 0 and uk[0] < 0 else 0
    return uk[bad:].astype(np.int64), (inv.reshape(-1) - bad).astype(np.int32)


def accumulate(verts, faces, cluster_of, n_clusters, lo, cell, dims):
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cell = F32(cell)
    acc = np.zeros((n_clusters, SLOTS), np.int64)
    has = cluster_of >= 0
    q = local(v[has], lo, cell, dims)
    for k in range(3):
        np.add.at(acc[:, 12 + k], cluster_of[has], quant(q[:, k]))
    np.add.at(acc[:, 15], cluster_of[has], 1)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    f = f[(cluster_of[f] >= 0).all(1)]
    with np.errstate(all="ignore"):
        p = v[f]  # [F,3 corners,3]
        e1, e2 = (p[:, 1] - p[:, 0]) / cell, (p[:, 2] - p[:, 0]) / cell
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = (l > 0) & np.isfinite(l)
    f, p, n, l = f[ok], p[ok], n[ok], l[ok]
    w = np.minimum(l * F32(0.5), F32(16))
    u = n / l[:, None]
    wu = w[:, None] * u
    shared = [quant(wu[:, i] * u[:, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    qw = quant(w)
    for x in range(3):
        c = cluster_of[f[:, x]]
        q = local(p[:, x], lo, cell, dims)
        d = -((u[:, 0] * q[:, 0] + u[:, 1] * q[:, 1]) + u[:, 2] * q[:, 2])
        wd = w * d
        for s in range(6):
            np.add.at(acc[:, s], c, shared[s])
        for k in range(3):
            np.add.at(acc[:, 6 + k], c, quant(wd * u[:, k]))
        np.add.at(acc[:, 9], c, quant(wd * d))
        np.add.at(acc[:, 10], c, qw)
        np.add.at(acc[:, 11], c, 1)
    if n_clusters and (acc[:, 11].max() > MAX_RECORDS or acc[:, 15].max() > MAX_RECORDS):
        raise Unsupported("more than 2^18 corner records or vertices in one cluster")
    return acc


def place(acc, cluster_keys, lo, cell, dims, lam, mean_only=False):
    a = acc.astype(np.float64) * (1.0 / SCALE)  # ((double) acc * 2^-40: the conversion rounds to nearest even, the product is exact)
    cnt = acc[:, 15].astype(np.float64)
    lam = np.float64(lam)
    with np.errstate(all="ignore"):
        m = [a[:, 12 + k] / cnt for k in range(3)]
        W = a[:, 10]
        gl = lam * W
        Mxx, Mxy, Mxz, Myy, Myz, Mzz = a[:, 0] + gl, a[:, 1], a[:, 2], a[:, 3] + gl, a[:, 4], a[:, 5] + gl
        r = [gl * m[k] - a[:, 6 + k] for k in range(3)]
        C00, C01, C02 = Myy * Mzz - Myz * Myz, Mxz * Myz - Mxy * Mzz, Mxy * Myz - Mxz * Myy
        C11, C12, C22 = Mxx * Mzz - Mxz * Mxz, Mxy * Mxz - Mxx * Myz, Mxx * Myy - Mxy * Mxy
        det = Mxx * C00 + (Mxy * C01 + Mxz * C02)
        t = [C00 * r[0] + (C01 * r[1] + C02 * r[2]), C01 * r[0] + (C11 * r[1] + C12 * r[2]), C02 * r[0] + (C12 * r[1] + C22 * r[2])]
        solved = (W > 0) & (det > 0) & np.isfinite(det) & (not mean_only)
        q = [np.where(solved, t[k] / det, m[k]) for k in range(3)]
    i = [cluster_keys % dims[0], (cluster_keys // dims[0]) % dims[1], cluster_keys // (dims[0] * dims[1])]
    out = np.empty((len(acc), 3), F32)
    for k in range(3):
        qk = np.minimum(np.maximum(q[k], -0.5), 0.5).astype(F32)
        out[:, k] = centre(i[k], lo[k], cell) + F32(cell) * qk
    return out


def cluster_faces(faces, cluster_of, n_verts):
    """rows [F,3] int32: the corners' cluster ids, smallest first, orientation kept; (-1, -1, -1) for a dropped face"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < n_verts)).all(1)
    c = np.where(ok[:, None], cluster_of[np.where(ok[:, None], f, 0)], -1).astype(np.int64)
    ok &= (c >= 0).all(1) & (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    first = np.argmin(c, 1)
    rows = np.stack([c[np.arange(len(c)), (first + j) % 3] for j in range(3)], 1) if len(c) else c
    return np.where(ok[:, None], rows, -1).astype(np.int32)


def simplify(verts, faces, cell, lo=None, lam=1e-3, mean_only=False, with_acc=False):
    """(verts [V',3] f32, faces [F',3] int32, vert_map [V] int32) -- and the raw accumulators [C,16] int64 with with_acc."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    lo3, dims = grid_for(v, cell, lo)
    ckeys, cluster_of = clusters(keys(v, lo3, cell, dims))
    C = len(ckeys)
    acc = accumulate(v, f, cluster_of, C, lo3, cell, dims)
    cverts = place(acc, ckeys, lo3, cell, dims, lam, mean_only)
    rows = cluster_faces(f, cluster_of, len(v))
    rows = np.unique(rows, axis=0) if len(rows) else rows  # merged, sorted lexicographically
    if len(rows) and rows[0, 0] < 0:
        rows = rows[1:]
    used = np.zeros(C, bool)
    used[rows.reshape(-1)] = True
    new_of_cluster = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    out_f = new_of_cluster[rows].astype(np.int32).reshape(-1, 3)
    vert_map = np.where(cluster_of >= 0, new_of_cluster[np.maximum(cluster_of, 0)], -1).astype(np.int32) if C else np.full(len(v), -1, np.int32)
    out = (cverts[used].reshape(-1, 3), out_f, vert_map)
    return out + (acc,) if with_acc else out


# ---- what every simplified mesh is held to ------------------------------------------------------------------------------------
def check_structure(v_in, f_in, cell, lo, ov, of, vert_map):
    """Indices in range, no repeated index in a face, no two equal rows, every vertex used, vert_map consistent with the faces, every
    output vertex inside its cluster's cell.  The cell test allows 2 ulp of the coordinate: the cell's borders lo + i cell and the
    placed vertex c + cell q are each rounded to float32 (two products and sums of at most 1 ulp in all)."""
    v_in = np.asarray(v_in, F32).reshape(-1, 3)
    f_in = np.asarray(f_in, np.int64).reshape(-1, 3)
    assert ov.dtype == F32 and of.dtype == np.int32 and vert_map.dtype == np.int32 and vert_map.shape == (len(v_in),)
    assert ov.ndim == 2 and ov.shape[1] == 3 and of.ndim == 2 and of.shape[1] == 3
    if len(of):
        assert of.min() >= 0 and of.max() < len(ov)
        assert (of[:, 0] != of[:, 1]).all() and (of[:, 1] != of[:, 2]).all() and (of[:, 0] != of[:, 2]).all()
        assert (of[:, 0] < of[:, 1]).all() and (of[:, 0] < of[:, 2]).all()  # rotated: the smallest index first
        assert len(np.unique(of, axis=0)) == len(of)
        assert (np.lexsort((of[:, 2], of[:, 1], of[:, 0])) == np.arange(len(of))).all()
    assert len(np.unique(of.reshape(-1))) == len(ov)
    assert vert_map.min(initial=-1) >= -1 and vert_map.max(initial=-1) < len(ov)
    # the faces are the input's, mapped: dropped where collapsed or where a corner has no output vertex
    ok = ((f_in >= 0) & (f_in < len(v_in))).all(1)
    m = np.where(ok[:, None], vert_map[np.where(ok[:, None], f_in, 0)], -1).astype(np.int64)
    ok &= (m >= 0).all(1) & (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    m = m[ok]
    first = np.argmin(m, 1) if len(m) else np.zeros(0, np.int64)
    m = np.stack([m[np.arange(len(m)), (first + j) % 3] for j in range(3)], 1) if len(m) else m.reshape(0, 3)
    assert (np.unique(m, axis=0).reshape(-1, 3) == of).all()
    lo3, dims = grid_for(v_in, cell, lo)
    fin = vert_map >= 0
    for k in range(3):
        i = cell_index(v_in[fin, k], lo3[k], cell, dims[k])
        a = lo3[k].astype(np.float64) + i * np.float64(F32(cell))
        p = ov[vert_map[fin], k].astype(np.float64)
        tol = 2 * np.spacing(np.abs(ov[vert_map[fin], k]).astype(F32)).astype(np.float64) + 2 * np.spacing(F32(abs(lo3[k])))
        assert (p >= a - tol).all() and (p <= a + np.float64(F32(cell)) + tol).all(), k


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()

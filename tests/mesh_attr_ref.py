"""numpy restatements of the mesh-attribute rules of include/f2n_abi.h (f2n_grid_normals, f2n_mesh_components, f2n_mesh_filter_count /
f2n_mesh_filter_emit): the tests' reference, written from the definitions in the header, not from the kernels."""
import numpy as np

F32 = np.float32


# ---- normals from a grid's gradient ------------------------------------------------------------------------------------------------
def corner_gradients(g, step, dtype=F32):
    """G [3, nz, ny, nx] (components x, y, z): central differences over 2 step in the interior, one-sided over step on the border
    planes, every operation rounded to `dtype`."""
    g = np.asarray(g, F32).astype(dtype)
    step = dtype(F32(step))
    out = np.empty((3,) + g.shape, dtype)
    for k, ax in enumerate((2, 1, 0)):  # x is the fastest (last) axis of [nz, ny, nx]
        a = np.moveaxis(g, ax, 0)
        o = np.moveaxis(out[k], ax, 0)
        o[1:-1] = (a[2:] - a[:-2]) / (dtype(2) * step)
        o[0] = (a[1] - a[0]) / step
        o[-1] = (a[-1] - a[-2]) / step
    return out


def gradient_blend(g, pts, lo=(0.0, 0.0, 0.0), step=1.0, dtype=F32):
    """The unnormalised blend g(p) [n,3] of f2n_grid_normals and max|G|: trilinear in the cell of p, along x, then y, then z."""
    G = corner_gradients(g, step, dtype)
    nz, ny, nx = G.shape[1:]
    dims = (nx, ny, nz)
    p = np.asarray(pts, F32).reshape(-1, 3).astype(dtype)
    step = dtype(F32(step))
    c, f = [], []
    for k in range(3):
        u = (p[:, k] - dtype(F32(lo[k]))) / step
        u = np.minimum(np.maximum(u, dtype(0)), dtype(dims[k] - 1))
        ck = np.minimum(np.floor(u).astype(np.int64), dims[k] - 2)
        c.append(ck)
        f.append((u - ck.astype(dtype)).astype(dtype))
    one = dtype(1)

    def lerp(a, b, t):
        return a * (one - t) + b * t

    out = np.empty((len(p), 3), dtype)
    for k in range(3):
        Gk = G[k]
        corner = lambda dx, dy, dz: Gk[c[2] + dz, c[1] + dy, c[0] + dx]  # noqa: E731
        y0 = lerp(lerp(corner(0, 0, 0), corner(1, 0, 0), f[0]), lerp(corner(0, 1, 0), corner(1, 1, 0), f[0]), f[1])
        y1 = lerp(lerp(corner(0, 0, 1), corner(1, 0, 1), f[0]), lerp(corner(0, 1, 1), corner(1, 1, 1), f[0]), f[1])
        out[:, k] = lerp(y0, y1, f[2])
    return out, float(np.abs(G).max()) if G.size else 0.0


def normals_of(gp):
    """-g / |g|, (0, 0, 0) where |g| is 0 or not finite."""
    gp = np.asarray(gp)
    with np.errstate(all="ignore"):
        ln = np.sqrt((gp * gp).sum(1))
        ok = (ln > 0) & np.isfinite(ln)
        n = np.where(ok[:, None], -gp / np.where(ok, ln, 1)[:, None], 0)
    return n.astype(gp.dtype)


def blend_discrepancy(g, pts, lo=(0.0, 0.0, 0.0), step=1.0):
    """max |g32(p) - g64(p)| / max|G|: the float32-vs-float64 discrepancy of the restatement itself on this grid and these points."""
    a, _ = gradient_blend(g, pts, lo, step, F32)
    b, gmax = gradient_blend(g, pts, lo, step, np.float64)
    return float(np.abs(a.astype(np.float64) - b).max() / gmax) if len(a) else 0.0


def normal_error(normals, g, pts, lo=(0.0, 0.0, 0.0), step=1.0):
    """How far computed unit normals are from the float64 restatement, as an error of the BLEND relative to max|G|: a normal that is off
    by d belongs to a blend that is off by d |g_ref|.  Vertices with |g_ref| < 1e-3 max|G| are left out.
    Returns (error, fraction of vertices left out)."""
    ref, gmax = gradient_blend(g, pts, lo, step, np.float64)
    ln = np.sqrt((ref * ref).sum(1))
    use = ln >= 1e-3 * gmax
    d = np.abs(np.asarray(normals, np.float64) - normals_of(ref)).max(1) * ln / gmax
    return (float(d[use].max()) if use.any() else 0.0), float(1.0 - use.mean()) if len(use) else 0.0


# ---- connected components ---------------------------------------------------------------------------------------------------------
def components(faces, n_verts):
    """labels [V] int32: the smallest vertex index of every vertex's component (union-find; an unused vertex is its own)."""
    parent = list(range(n_verts))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)  # the smaller index stays the root: the root is the component's minimum
    return np.array([find(v) for v in range(n_verts)], np.int32).reshape(n_verts)


def filter_components(verts, faces, min_faces):
    """(verts, faces, vert_src): faces of components with >= min_faces faces, the vertices they use, both in their original order."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    if min_faces <= 1:
        return verts, faces, np.arange(len(verts), dtype=np.int32)
    labels = components(faces, len(verts))
    size = np.bincount(labels[faces[:, 0]], minlength=len(verts)) if len(faces) else np.zeros(len(verts), np.int64)
    keep_f = size[labels[faces[:, 0]]] >= min_faces if len(faces) else np.zeros(0, bool)
    keep_v = np.zeros(len(verts), bool)
    keep_v[faces[keep_f].reshape(-1)] = True
    new_idx = np.cumsum(keep_v) - 1
    return verts[keep_v], new_idx[faces[keep_f]].astype(np.int32).reshape(-1, 3), np.nonzero(keep_v)[0].astype(np.int32)


def component_face_counts(faces, n_verts):
    """{label: number of faces} of a mesh."""
    faces = np.asarray(faces).reshape(-1, 3)
    if not len(faces):
        return {}
    lab, cnt = np.unique(components(faces, n_verts)[faces[:, 0]], return_counts=True)
    return dict(zip(lab.tolist(), cnt.tolist()))


# ---- test grids ---------------------------------------------------------------------------------------------------------------------
def sphere_field(shape, center, r):
    """[nz, ny, nx] float32: r - distance from center (x, y, z), > 0 inside."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return (r - np.sqrt((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2)).astype(F32)

"""numpy restatement of the sparse mesher's definitions in include/f2n_abi.h ("Sparse mesh extraction on bricks"): the brick grid, which
corners and cells a brick reads and owns, the keys, and the mark descent of f2n_brick_mark.  Written from the header text, not from
the kernels; the octree records are those of tests/mesh_ref.py (parse_nodes)."""
import numpy as np

import mesh_ref as mr

F32 = np.float32
MAX_DEPTH = 32  # nodes of depth 0..31 are entered (f2n_oct_locate_warp's bound)


def grid_spec(lo, hi, res):
    """(step, (nx, ny, nz)) of Renderer::MakeGridSpec: float32 arithmetic, n = max(2, lround(ext / step) + 1)."""
    ext = [F32(F32(hi[k]) - F32(lo[k])) for k in range(3)]
    step = F32(max(ext) / F32(res))
    return step, tuple(max(2, int(np.floor(np.float64(F32(ext[k] / step)) + 0.5)) + 1) for k in range(3))


def n_bricks(n, B):
    """nb[k] = ceil((n[k] - 1) / B), (nbx, nby, nbz)."""
    return tuple((n[k] - 1 + B - 1) // B for k in range(3))


def brick_coords(b, nb):
    return b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1])


def brick_id(bc, nb):
    return (bc[2] * nb[1] + bc[1]) * nb[0] + bc[0]


def brick_corner_indices(b, n, B):
    """[(B+1)^3, 3] grid indices of the corners brick b reads (local x fastest) and exists [(B+1)^3] bool."""
    nb = n_bricks(n, B)
    bc = brick_coords(b, nb)
    S = B + 1
    l = np.arange(S ** 3)
    lc = np.stack([l % S, (l // S) % S, l // (S * S)], 1)
    idx = lc + np.array(bc) * B
    return idx, (idx <= np.array(n) - 1).all(1)


def corner_key(idx, n):
    idx = np.asarray(idx, np.int64)
    return (idx[..., 2] * n[1] + idx[..., 1]) * n[0] + idx[..., 0]


def brick_values(grid, ids, B, fill=np.nan):
    """values [len(ids), (B+1)^3] of a dense grid [nz, ny, nx]; the corners that do not exist get `fill` (they are never read)."""
    nz, ny, nx = grid.shape
    n = (nx, ny, nz)
    out = np.full((len(ids), (B + 1) ** 3), fill, F32)
    flat = np.asarray(grid, F32).reshape(-1)
    for j, b in enumerate(ids):
        idx, ex = brick_corner_indices(int(b), n, B)
        out[j, ex] = flat[corner_key(idx[ex], n)]
    return out


def bricks_with_both_sides(grid, level, B):
    """ids (ascending) of the bricks whose (B+1)^3 closure has a corner inside (g > level) and a corner that is not."""
    nz, ny, nx = grid.shape
    n = (nx, ny, nz)
    nb = n_bricks(n, B)
    inside = (np.asarray(grid, F32) > F32(level)).reshape(-1)
    out = []
    for b in range(nb[0] * nb[1] * nb[2]):
        idx, ex = brick_corner_indices(b, n, B)
        v = inside[corner_key(idx[ex], n)]
        if v.any() and not v.all():
            out.append(b)
    return np.array(out, np.int32)


def box_meets_live_leaf(nodes, blo, bhi):
    """the descent of f2n_brick_mark for one closed box (float32 [3] each)."""
    h = F32(nodes["side"][0] * F32(0.5))
    c0 = nodes["center"][0]
    for k in range(3):
        if not (bhi[k] >= F32(c0[k] - h) and blo[k] <= F32(c0[k] + h)):
            return False
    stack = [(0, 0)]
    while stack:
        u, depth = stack.pop()
        ch = nodes["childs"][u]
        if (ch < 0).all():
            if nodes["trans"][u] >= 0:
                return True
            continue
        if depth + 1 >= MAX_DEPTH:
            continue
        c = nodes["center"][u]
        for slot in range(8):
            if ch[slot] < 0:
                continue
            s = ((slot >> 2) & 1, (slot >> 1) & 1, slot & 1)
            if all((bhi[k] >= c[k]) if s[k] else (blo[k] < c[k]) for k in range(3)):
                stack.append((int(ch[slot]), depth + 1))
    return False


def brick_mark(nodes, lo, step, n, B, b0=(0, 0, 0), b1=None):
    """flags [nbz, nby, nbx] uint8 -- of the bricks b0 <= (bx, by, bz) <= b1 only when a box of bricks is given (shape b1 - b0 + 1,
    reversed): a virtual grid is never walked whole."""
    nb = n_bricks(n, B)
    b1 = tuple(v - 1 for v in nb) if b1 is None else b1
    ax = mr.grid_points(lo, step, n)
    flags = np.zeros((b1[2] - b0[2] + 1, b1[1] - b0[1] + 1, b1[0] - b0[0] + 1), np.uint8)
    for bz in range(b0[2], b1[2] + 1):
        for by in range(b0[1], b1[1] + 1):
            for bx in range(b0[0], b1[0] + 1):
                bc = (bx, by, bz)
                blo = [ax[k][bc[k] * B] for k in range(3)]
                bhi = [ax[k][min(bc[k] * B + B, n[k] - 1)] for k in range(3)]
                flags[bz - b0[2], by - b0[1], bx - b0[0]] = 1 if box_meets_live_leaf(nodes, blo, bhi) else 0
    return flags


def bricks_reading(i, n, B):
    """ids of every brick whose (B+1)^3 closure holds the grid point i = (ix, iy, iz)."""
    nb = n_bricks(n, B)
    cands = []
    for k in range(3):
        c = [min(i[k] // B, nb[k] - 1)]
        if i[k] % B == 0 and 0 < i[k] // B <= nb[k] - 1 and i[k] // B - 1 not in c:
            c.append(i[k] // B - 1)
        cands.append(c)
    return [brick_id((a, b, c), nb) for a in cands[0] for b in cands[1] for c in cands[2]]


def mesh_keys(grid, level):
    """(vertex keys [V], face keys [F]) of the dense mesh of `grid`, in f2n_mesh_emit's order: both ascending."""
    g = np.asarray(grid, F32)
    nz, ny, nx = g.shape
    inside = g > F32(level)
    flat = inside.reshape(-1)
    idx = np.arange(nx * ny * nz)
    xs, ys, zs = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    vk = []
    for t, o in enumerate(mr.EDGE_OFFSETS):
        d = (o & 1, (o >> 1) & 1, (o >> 2) & 1)
        ok = (xs + d[0] < nx) & (ys + d[1] < ny) & (zs + d[2] < nz)
        nb_ = np.where(ok, idx + d[0] + d[1] * nx + d[2] * nx * ny, 0)
        vk.append(8 * idx[ok & (flat != flat[nb_])].astype(np.int64) + t)
    vk = np.sort(np.concatenate(vk))
    fk = []
    for z in range(nz - 1):
        for y in range(ny - 1):
            for x in range(nx - 1):
                cm = [bool(inside[z + ((o >> 2) & 1), y + ((o >> 1) & 1), x + (o & 1)]) for o in range(8)]
                k = 0
                for axes in mr.TET_AXES:
                    ins = sum(cm[o] for o in (0, axes[0], axes[0] | axes[1], 7))
                    k += {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[ins]
                cell = (z * (ny - 1) + y) * (nx - 1) + x
                fk.extend(16 * cell + q for q in range(k))
    return vk, np.array(fk, np.int64)


# ---- virtual grids whose indices need more than 32 bits --------------------------------------------------------------------------
# Only a WINDOW of at most 64 bricks of such a grid is ever touched: its dense sub-grid, with lo translated by whole steps, is an
# ordinary small grid.  step is a power of two and lo a multiple of it, small enough for every coordinate lo + step i to be exact in
# float32 -- the sub-grid's points are then the same floats as the big grid's, and every result can be compared bit for bit.
HUGE_STEP = 2.0 ** -6
# n, B, lo, the window's size in bricks, the first brick of the inner window (the far window ends at the last brick of every axis)
HUGE_GRIDS = {
    "wide16": dict(n=(65537, 65537, 33), B=16, lo=(-512.0, -600.25, 3.5), wb=(2, 2, 1), inner=(2049, 1365, 1)),
    "wide8": dict(n=(65537, 65537, 33), B=8, lo=(-512.0, -600.25, 3.5), wb=(3, 3, 2), inner=(4097, 2731, 1)),
    "full": dict(n=(524288, 32765, 9), B=4, lo=(-4096.0, -250.5, -0.0625), wb=(4, 4, 2), inner=(65537, 4099, 0)),
}
HUGE_REFUSED = ((524288, 32769, 9), 4)  # 131072 x 8192 x 2 = 2^31 bricks exactly: one too many


def huge_window(name, which, lo_w=None, step=HUGE_STEP):
    """The window `which` ("far": ends at the last brick of every axis; "inner": strictly inside along every axis that has more bricks
    than the window) of HUGE_GRIDS[name].  lo_w given: the grid is placed so that the window's first corner lies there (lo = lo_w -
    step i0) instead of at the table's lo.  Returns n, B, lo, step, nb, w0 / wb (first brick, bricks per axis), i0 (first corner), m
    (points per axis: clipped at n - 1), lo_w, ids (the window's bricks, ascending: the order of local_ids, their ids on the
    window's own grid m)."""
    spec = HUGE_GRIDS[name]
    n, B, wb = spec["n"], spec["B"], spec["wb"]
    nb = n_bricks(n, B)
    w0 = tuple(nb[k] - wb[k] for k in range(3)) if which == "far" else spec["inner"]
    assert all(0 <= w0[k] and w0[k] + wb[k] <= nb[k] for k in range(3)) and wb[0] * wb[1] * wb[2] <= 64
    if which == "inner":
        assert all(0 < w0[k] and w0[k] + wb[k] < nb[k] for k in range(3) if nb[k] > wb[k] + 1)
    i0 = tuple(w0[k] * B for k in range(3))
    m = tuple(min(i0[k] + wb[k] * B, n[k] - 1) - i0[k] + 1 for k in range(3))
    if lo_w is None:
        lo = tuple(float(v) for v in spec["lo"])
        lo_w = tuple(lo[k] + step * i0[k] for k in range(3))  # (float64: exact)
    else:
        lo_w = tuple(float(v) for v in lo_w)
        lo = tuple(lo_w[k] - step * i0[k] for k in range(3))
    for k in range(3):  # every coordinate of the window is exact in float32, on the big grid and on the sub-grid
        i = np.arange(i0[k], i0[k] + m[k])
        exact = lo[k] + step * i.astype(np.float64)
        big = F32(lo[k]) + F32(step) * i.astype(F32)
        sub = F32(lo_w[k]) + F32(step) * np.arange(m[k], dtype=F32)
        assert F32(lo[k]) == lo[k] and F32(lo_w[k]) == lo_w[k] and (big.astype(np.float64) == exact).all() and big.tobytes() == sub.tobytes()
    assert n_bricks(m, B) == wb
    local_ids = np.arange(wb[0] * wb[1] * wb[2], dtype=np.int32)
    ids = np.array([brick_id(tuple(brick_coords(int(b), wb)[k] + w0[k] for k in range(3)), nb) for b in local_ids], np.int64)
    assert (np.diff(ids) > 0).all() and ids[-1] < 2 ** 31
    return dict(name=name, which=which, n=n, B=B, lo=lo, step=step, nb=nb, w0=w0, wb=wb, i0=i0, m=m, lo_w=lo_w, ids=ids.astype(np.int32),
                local_ids=local_ids)


def huge_magnitudes(w):
    """Python integers: the largest corner, vertex and cell / face keys and brick id a window touches, and the grid's brick count."""
    n, nb = w["n"], w["nb"]
    top = [w["i0"][k] + w["m"][k] - 1 for k in range(3)]
    corner = (top[2] * n[1] + top[1]) * n[0] + top[0]
    cell = ((top[2] - 1) * (n[1] - 1) + top[1] - 1) * (n[0] - 1) + top[0] - 1
    return dict(corner=corner, vertex_key=8 * corner + 6, face_key=16 * cell + 11, brick_id=int(w["ids"][-1]), bricks=nb[0] * nb[1] * nb[2])


def window_sphere(w):
    """[mz, my, mx] float32 of the window's sub-grid: radius - distance to a centre near the window's middle, evaluated in float64 at
    the corners' world positions.  The inside corners keep two planes away from the window's faces: every crossing edge lies at least
    one cell inside the window."""
    m, step = w["m"], w["step"]
    off = (0.13, -0.21, 0.07)
    r = ((min(m) - 1) / 2.0 - 1.3) * step
    ax = [w["lo_w"][k] + step * np.arange(m[k], dtype=np.float64) for k in range(3)]
    c = [w["lo_w"][k] + step * ((m[k] - 1) / 2.0 + off[k]) for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    g = (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(F32)
    ins = np.argwhere(g > 0)
    assert len(ins) > 0 and (ins >= 2).all() and (ins <= np.array(g.shape) - 3).all()
    return g

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


def brick_mark(nodes, lo, step, n, B):
    """flags [nbz, nby, nbx] uint8."""
    nb = n_bricks(n, B)
    ax = mr.grid_points(lo, step, n)
    flags = np.zeros((nb[2], nb[1], nb[0]), np.uint8)
    for bz in range(nb[2]):
        for by in range(nb[1]):
            for bx in range(nb[0]):
                bc = (bx, by, bz)
                blo = [ax[k][bc[k] * B] for k in range(3)]
                bhi = [ax[k][min(bc[k] * B + B, n[k] - 1)] for k in range(3)]
                flags[bz, by, bx] = 1 if box_meets_live_leaf(nodes, blo, bhi) else 0
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

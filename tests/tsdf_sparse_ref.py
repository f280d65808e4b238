"""numpy restatement of "Sparse TSDF fusion on bricks" (include/f2n_abi.h): the hit of a (grid point, view) pair, the flags of
f2n_tsdf_brick_mark, the rows of f2n_tsdf_integrate_bricks and the vertex rule of the masked brick mesher.  Written from the header's
text on top of tests/tsdf_ref.py (the twelve steps, the masked dense mesher) and tests/mesh_sparse_ref.py (bricks, rows, keys)."""
import numpy as np

import mesh_ref as mr
import mesh_sparse_ref as sr
import tsdf_ref as tr

F32 = np.float32


def hits(c, v0=0, v1=None, conf="case"):
    """[nz, ny, nx] bool: the grid point has a HIT in some view of [v0, v1) of case c (a dict of tsdf_ref.synthetic_case): the view
    passes steps 1-9, !(sdf < -trunc), and sdf < 0.  float32, one rounding per operation, in the header's order."""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    poses, intri, dist = (np.asarray(c[k], F32) for k in ("poses", "intri", "dist"))
    depth = np.asarray(c["depth"], F32)
    cf = c["conf"] if isinstance(conf, str) else conf
    V, h, w = depth.shape
    v1 = V if v1 is None else v1
    trunc = F32(c["trunc"])
    px, py, pz = tr.voxel_points(c["lo"], c["step"], nx, ny, nz)
    out = np.zeros(nx * ny * nz, bool)
    with np.errstate(all="ignore"):
        for v in range(v0, v1):
            P, K = poses[v], intri[v]
            q = [px - P[0, 3], py - P[1, 3], pz - P[2, 3]]
            cc = [P[0, j] * q[0] + (P[1, j] * q[1] + P[2, j] * q[2]) for j in range(3)]
            s = -cc[2]
            u, vv = cc[0] / s, (-cc[1]) / s
            du, dv = tr.distort(dist[v], u, vv)
            x = K[0, 0] * (u + du) + K[0, 2]
            y = K[1, 1] * (vv + dv) + K[1, 2]
            fb, fa = np.floor(x), np.floor(y)
            ok = (s > 0) & (fa >= 0) & (fa < F32(h)) & (fb >= 0) & (fb < F32(w))
            ia, ib = np.where(ok, fa, 0).astype(np.int64), np.where(ok, fb, 0).astype(np.int64)
            D = depth[v, ia, ib]
            ok &= D > 0
            if cf is not None:
                ok &= np.asarray(cf, F32)[v, ia, ib] > 0
            sdf = D - np.sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2]))
            out |= ok & ~(sdf < -trunc) & (sdf < 0)
    return out.reshape(nz, ny, nx)


def brick_mark(c, B, v0=0, v1=None, conf="case"):
    """flags [nbz, nby, nbx] uint8: some EXISTING corner of the brick's (B+1)^3 row has a hit."""
    n = (c["nx"], c["ny"], c["nz"])
    nb = sr.n_bricks(n, B)
    hit = hits(c, v0, v1, conf).reshape(-1)
    flags = np.zeros(nb[0] * nb[1] * nb[2], np.uint8)
    for b in range(len(flags)):
        idx, ex = sr.brick_corner_indices(b, n, B)
        flags[b] = 1 if hit[sr.corner_key(idx[ex], n)].any() else 0
    return flags.reshape(nb[2], nb[1], nb[0])


def brick_rows(grid, ids, n, B, prefill):
    """rows [len(ids), (B+1)^3] of a dense grid [nz, ny, nx] (any dtype): existing corners of bricks inside the grid from the grid, every
    other entry (a corner that does not exist, a brick id outside the grid) keeps prefill's."""
    out = np.array(prefill, copy=True).reshape(len(ids), (B + 1) ** 3)
    flat = np.asarray(grid).reshape(-1)
    nb = sr.n_bricks(n, B)
    for j, b in enumerate(ids):
        if 0 <= int(b) < nb[0] * nb[1] * nb[2]:
            idx, ex = sr.brick_corner_indices(int(b), n, B)
            out[j, ex] = flat[sr.corner_key(idx[ex], n)]
    return out


def masked_brick_vertex_keys(g, valid, level, ids, B):
    """The sorted vertex keys the masked brick mesher EMITS over the bricks ids (before unreferenced vertices are dropped): 8 corner + type
    for every owned corner's edge that crosses the level with both endpoints valid -- every brick of ids inside the grid."""
    g = np.asarray(g, F32)
    nz, ny, nx = g.shape
    n = (nx, ny, nz)
    nb = sr.n_bricks(n, B)
    inside, ok = (g > F32(level)).reshape(-1), (np.asarray(valid) != 0).reshape(-1)
    keys = []
    for b in ids:
        bc = sr.brick_coords(int(b), nb)
        idx, ex = sr.brick_corner_indices(int(b), n, B)
        lc = idx - np.array(bc) * B
        own = ex & np.all((lc < B) | (np.array(bc) == np.array(nb) - 1), axis=1)
        for i in idx[own]:
            a = int(sr.corner_key(i, n))
            for t, o in enumerate(mr.EDGE_OFFSETS):
                j = i + np.array([o & 1, (o >> 1) & 1, (o >> 2) & 1])
                if (j > np.array(n) - 1).any():
                    continue
                e = int(sr.corner_key(j, n))
                if ok[a] and ok[e] and inside[a] != inside[e]:
                    keys.append(8 * a + t)
    return np.array(sorted(keys), np.int64)
